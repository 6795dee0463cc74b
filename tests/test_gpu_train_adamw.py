"""GPU: the device optimiser (csrc/train.hip.h k_adamw_onecycle / k_adamw_step_advance; train.adamw_update, train.DeviceAdamW) and
train.train(device_optimizer=True / graph_step=True).

One step against the float64 restatement of tests/test_train_adamw_surface.py (adamw_f64, float64 scalars read from torch's own scheduler),
within that file's three bounds -- which torch's CPU AdamW meets there, and torch's GPU AdamW must meet here on the same inputs.  One table
holds segments of 1, 3, 4, 5, 2047, 2048, 2049 and 4097 floats (several segments, a chunk boundary, tails) at 16-byte aligned offsets, and
one of 2051 floats whose p / g / m / v start one float past a 16-byte boundary (the single-float path, a whole chunk of it included).
Every float of the four flat buffers outside the segments is a guard of -7 and must still be -7.

End to end on the fixtures and sizes of test_gpu_train_batches.py (V80 module, dropout 0, 256 examples, batch 32, 8 steps, fixed batch_ids):
the three device runs against the legacy path within max(4 x the legacy path's run-to-run spread, 1e-5 max|w|) per tensor, loss histories
to 1e-5 relative -- that test's own tolerance.  The fixture net's BatchNorm counters start at the shipped checkpoint's value, not at 0: eight
steps are checked as start + 8.  The hook's probe sums its parameter in f64: the schedule's last step (lr 1.2e-8) moves a weight by less
than an f32 sum of 6561 weights resolves.

Measured on one MI355X: the kernel uses at most 0.72 / 0.24 / 0.43 of the p / m / v bounds, torch's GPU AdamW 0.72 / 0.24 / 0.42; 0-51 /
2348-3662 / 866-1064 of 12 305 p / m / v values differ in some bit between the two; device_optimizer and graph_step end within 0.18 of the
legacy tolerance and are bit-equal to each other."""
import numpy as np
import pytest

from test_gpu_train_batches import _examples, _module
from test_train_adamw_surface import adamw_bounds, adamw_f64, torch_schedule

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 2047, 2048, 2049, 4097)
ODD = 2051
TOTAL, MAX_LR = 10, 3e-3
BETA2, EPS, WD = 0.999, 1e-8, 1e-2


def _layout():
    """-> [(offset, size)] in a flat buffer, its length: 4 guards, every aligned segment at a multiple of 4 floats with at least 4 guards
    behind it, then the odd segment at an offset of 1 modulo 4, then 7 guards"""
    segs, o = [], 4
    for n in SIZES:
        segs.append((o, n))
        o = -(-(o + n) // 4) * 4 + 4
    segs.append((o + 1, ODD))
    return segs, o + 1 + ODD + 7


def _inputs(zero_state_segment):
    segs, total = _layout()
    r = np.random.RandomState(11)
    p, g, m, v = (np.full(total, -7.0, dtype=np.float32) for _ in range(4))
    inside = np.zeros(total, dtype=bool)
    for k, (o, n) in enumerate(segs):
        scale = 1.0 if k % 2 == 0 else 1e-4
        inside[o:o + n] = True
        p[o:o + n] = r.randn(n)
        g[o:o + n] = r.randn(n) * scale
        m[o:o + n] = r.randn(n) * 0.1 * scale
        v[o:o + n] = (r.randn(n) * 0.1 * scale) ** 2
        if k == zero_state_segment:                                                  # a fresh optimiser's state
            m[o:o + n] = 0
            v[o:o + n] = 0
    return segs, inside, p, g, m, v


@pytest.fixture(scope='module')
def schedule():
    return torch_schedule(TOTAL, MAX_LR)


@pytest.mark.parametrize('s', [0, 1, TOTAL - 1, 12])
def test_one_step_against_float64_guards_and_torch(s, schedule):
    import torch
    from azg_amd import train
    segs, inside, p, g, m, v = _inputs(zero_state_segment=5 if s == 0 else -1)
    row = min(s, TOTAL - 1)                                                          # 12: the clamp gives the last row
    lr, beta1 = schedule[row]
    k = row + 1
    dev = [torch.from_numpy(x.copy()).cuda() for x in (p, g, m, v)]
    for t in dev:
        assert t.data_ptr() % 16 == 0
    quads = [tuple(t[o:o + n] for t in dev) for o, n in segs]
    assert all(q[0].data_ptr() % 16 == 0 for q in quads[:-1]) and all(t.data_ptr() % 16 == 4 for t in quads[-1])
    seg_t, chunk_t = train.adamw_tables(quads)
    assert tuple(seg_t.shape) == (len(segs), 5) and chunk_t.shape[0] == sum(-(-n // 2048) for _, n in segs)
    table = torch.from_numpy(np.asarray(train.onecycle_adamw_table(MAX_LR, TOTAL))).cuda()
    step = torch.tensor([s], dtype=torch.int64, device='cuda:0')
    train.adamw_update(seg_t, chunk_t, table, step)
    assert int(step.item()) == s                                                     # the update only reads the counter
    train.adamw_step_advance(step)
    assert int(step.item()) == s + 1
    got_p, got_g, got_m, got_v = (t.cpu().numpy() for t in dev)
    # guards: before, between and behind the segments, in every buffer; the gradients untouched altogether
    for name, x in (('p', got_p), ('m', got_m), ('v', got_v)):
        assert (x[~inside] == -7).all(), name
    assert np.array_equal(got_g.view(np.uint32), g.view(np.uint32))
    assert (~inside).sum() >= 4 * (len(segs) + 1)
    # the restatement and its bounds
    want_p, want_m, want_v, delta, ssd = adamw_f64(p[inside], g[inside], m[inside], v[inside], lr, beta1, BETA2, EPS, WD, k)
    bp, bm, bv = adamw_bounds(p[inside], g[inside], m[inside], want_v, delta, ssd)

    def check(who, xp, xm, xv):
        ep, em, ev = np.abs(xp.astype(np.float64) - want_p), np.abs(xm.astype(np.float64) - want_m), np.abs(xv.astype(np.float64) - want_v)
        share = lambda e, b: float(np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e > 0, np.inf, 0)).max())  # noqa: E731
        print('%s, step %d: largest share of the bounds used: p %.2f, m %.2f, v %.2f' % (who, s, share(ep, bp), share(em, bm), share(ev, bv)))
        assert np.isfinite(xp).all() and np.isfinite(xm).all() and np.isfinite(xv).all(), who
        assert (ep <= bp).all() and (em <= bm).all() and (ev <= bv).all(), who

    check('kernel', got_p[inside], got_m[inside], got_v[inside])
    assert not np.array_equal(got_p[inside], p[inside])
    # torch's own AdamW on the GPU, same inputs, the scalars of the same row
    w = torch.nn.Parameter(torch.from_numpy(p[inside]).cuda())
    w.grad = torch.from_numpy(g[inside]).cuda()
    opt = torch.optim.AdamW([w], lr=lr, betas=(beta1, BETA2), eps=EPS, weight_decay=WD)
    opt.state[w] = dict(step=torch.tensor(float(k - 1)), exp_avg=torch.from_numpy(m[inside]).cuda(), exp_avg_sq=torch.from_numpy(v[inside]).cuda())
    opt.step()
    t_p, t_m, t_v = w.detach().cpu().numpy(), opt.state[w]['exp_avg'].cpu().numpy(), opt.state[w]['exp_avg_sq'].cpu().numpy()
    check('torch', t_p, t_m, t_v)
    diff = [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in ((got_p[inside], t_p), (got_m[inside], t_m), (got_v[inside], t_v))]
    print('step %d: of %d elements, %d / %d / %d of p / m / v differ in some bit between the kernel and torch' % ((s, int(inside.sum())) + tuple(diff)))


def test_counter_refusal_after_the_last_step_and_a_parameter_without_gradient():
    import torch
    from azg_amd import train
    torch.manual_seed(3)
    a, b = torch.nn.Parameter(torch.randn(5, device='cuda:0')), torch.nn.Parameter(torch.randn(3, 7, device='cuda:0'))
    opt = train.DeviceAdamW([a, b], MAX_LR, TOTAL)
    assert a.grad is None and b.grad is None
    assert opt.flat_grad.numel() == 8 + 24 and opt.offsets == [0, 8]                 # segments start at multiples of 4 floats

    def one():
        opt.zero_grad()
        (a.sum() + (b * b).sum()).backward()
        b_then = b.detach().clone()
        opt.step()
        return b_then

    for _ in range(3):
        b_then = one()
    assert int(opt.step_counter.item()) == 3 and opt.steps_taken == 3
    assert a.grad.data_ptr() == opt.flat_grad.data_ptr() and b.grad.data_ptr() == opt.flat_grad.data_ptr() + 32    # views of the flat buffer
    assert torch.equal(a.grad, torch.ones(5, device='cuda:0')) and torch.equal(b.grad, 2 * b_then)              # 0 + g: one backward's worth
    for _ in range(7):
        one()
    assert int(opt.step_counter.item()) == 10
    before = [a.detach().clone(), b.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
    opt.zero_grad()
    (a.sum() + (b * b).sum()).backward()
    with pytest.raises(ValueError, match='total_steps'):
        opt.step()
    assert int(opt.step_counter.item()) == 10 and opt.steps_taken == 10              # nothing was launched
    for x, y in zip(before, [a.detach(), b.detach(), opt.exp_avg, opt.exp_avg_sq]):
        assert torch.equal(x, y)
    # a parameter that requires grad and gets none: torch would skip it, one launch over fixed tables cannot
    c, d = torch.nn.Parameter(torch.randn(4, device='cuda:0')), torch.nn.Parameter(torch.randn(4, device='cuda:0'))
    opt2 = train.DeviceAdamW([c, d], MAX_LR, TOTAL)
    c.sum().backward()
    keep = c.detach().clone()
    with pytest.raises(ValueError, match='received none'):
        opt2.step()
    assert torch.equal(c.detach(), keep) and int(opt2.step_counter.item()) == 0


def test_device_adamw_follows_torchs_adamw_under_onecycle():
    """five steps of both optimisers on one quadratic: every step's scalars come from the table row that the device counter picks"""
    import torch
    from azg_amd import train
    torch.manual_seed(4)
    w0 = torch.randn(3000, device='cuda:0')
    target = torch.randn(3000, device='cuda:0')
    a, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone())
    mine = train.DeviceAdamW([a], MAX_LR, 5)
    ref = torch.optim.AdamW([b], lr=MAX_LR)
    sched = torch.optim.lr_scheduler.OneCycleLR(ref, max_lr=MAX_LR, total_steps=5)
    for _ in range(5):
        mine.zero_grad()
        ((a - target) ** 2).sum().backward()
        mine.step()
        ref.zero_grad(set_to_none=True)
        ((b - target) ** 2).sum().backward()
        ref.step()
        sched.step()
    # per step either f32 evaluation is within 3u |w| + 16u |D| + the m term of the exact step (the bounds of test_train_adamw_surface.py,
    # |D| < |w| here): under 8u max|w| each, 16u between the two; what a difference feeds back through the gradient is damped by lr
    err = float((a.detach() - b.detach()).abs().max())
    print('DeviceAdamW vs torch AdamW + OneCycleLR after 5 steps: max |difference| %.3g (max |w| %.3g)' % (err, float(b.detach().abs().max())))
    assert err <= 5 * 16 * 2.0 ** -24 * float(b.detach().abs().max())
    assert float((a.detach() - w0).abs().max()) > 1e-3                               # (and they moved)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _run(ex, **kw):
    from azg_amd import train
    m = _module()
    hist = train.train(m, ex, learn_rate=3e-3, batch_size=32, epochs=1, q_weight=0.5, device='cuda:0', **kw)
    return np.array(hist, dtype=np.float64), {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def test_device_optimizer_and_graph_step_train_like_the_legacy_path():
    ex = _examples()
    n = len(ex[0])
    assert n == 256
    batch_ids = np.stack([np.random.RandomState(100 + s).permutation(n)[:32] for s in range(8)])
    h1, w1 = _run(ex, batch_ids=batch_ids)
    h2, w2 = _run(ex, batch_ids=batch_ids)
    hb, wb = _run(ex, batch_ids=batch_ids, device_batches=True)
    info_o, info_g, seen = {}, {}, []
    ho, wo = _run(ex, batch_ids=batch_ids, device_batches=True, device_optimizer=True, info=info_o)
    probe = {}

    def on_step(ep, i_batch, step):
        # (summed in f64: the schedule's last step moves a weight by about 1e-8, which a sum in f32 of 6561 weights would round away)
        seen.append((ep, i_batch, step, float(probe['p'].detach().double().sum().item())))

    from azg_amd import train
    m = _module()
    probe['p'] = m.output_layers_PI[4].weight
    hg = np.array(train.train(m, ex, learn_rate=3e-3, batch_size=32, epochs=1, q_weight=0.5, device='cuda:0', batch_ids=batch_ids,
                              device_batches=True, graph_step=True, info=info_g, on_step=on_step), dtype=np.float64)
    wg = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    assert h1.shape == hb.shape == ho.shape == hg.shape == (8, 2)

    def within(name, wx, wref):
        worst = 0.0
        for k in w1:
            r = np.abs(w1[k] - w2[k]).max()
            bound = max(4 * r, 1e-5 * np.abs(w1[k]).max())
            diff = np.abs(wx[k] - wref[k]).max()
            worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
            assert diff <= bound, (name, k, diff, r, bound)
        print('%s: largest weight difference as a fraction of its bound: %.3g' % (name, worst))

    for name, wx, hx in (('device_batches vs legacy', wb, hb), ('device_optimizer vs legacy', wo, ho), ('graph_step vs legacy', wg, hg)):
        within(name, wx, w1)
        print('%s: loss histories, max relative difference %.3g' % (name, (np.abs(hx - h1) / np.abs(h1)).max()))
        assert (np.abs(hx - h1) <= 1e-5 * np.abs(h1)).all(), (name, hx, h1)
    within('graph_step vs eager device_optimizer', wg, wo)
    assert (np.abs(hg - ho) <= 1e-5 * np.abs(ho)).all()
    print('graph_step and eager device_optimizer are bit-equal: weights %s, loss histories %s'
          % (all(np.array_equal(wg[k], wo[k]) for k in wo), np.array_equal(hg, ho)))
    assert info_o == {'optimizer': 'device', 'graph_replays': 0}
    assert info_g == {'optimizer': 'device', 'graph_replays': 7}
    tracked = [k for k in wg if k.endswith('num_batches_tracked')]
    start = {k: float(v) for k, v in _module().state_dict().items() if k.endswith('num_batches_tracked')}     # (the shipped net's counts)
    assert len(tracked) == 10 and all(wg[k] - start[k] == 8 and wg[k] == w1[k] for k in tracked), {k: wg[k] - start[k] for k in tracked}
    assert [x[:3] for x in seen] == [(0, s, s) for s in range(8)]
    assert len({x[3] for x in seen}) == 8, seen                                      # the hook saw eight different nets


def test_graph_step_draws_its_batches_like_the_eager_device_path():
    from azg_amd import train
    ex = _examples()
    n = len(ex[0])
    s1, _ = _run(ex, device_batches=True, graph_step=True, seed=5)
    s2, _ = _run(ex, device_batches=True, graph_step=True, seed=5)
    assert np.array_equal(s1, s2)
    drawn = train.sample_ids(n, 32, 8, 5, 0).cpu().numpy()
    s3, _ = _run(ex, device_batches=True, batch_ids=drawn)
    print('graph_step(seed=5) vs device_batches on sample_ids(n, 32, 8, 5, 0): max relative difference of the histories %.3g'
          % (np.abs(s1 - s3) / np.abs(s3)).max())
    assert (np.abs(s1 - s3) <= 1e-5 * np.abs(s3)).all(), (s1, s3)


def test_a_single_step_captures_nothing():
    ex = _examples()
    info = {}
    h, _ = _run(tuple(x[:32] for x in ex), device_batches=True, graph_step=True, seed=1, info=info)
    assert h.shape == (1, 2) and info == {'optimizer': 'device', 'graph_replays': 0}
