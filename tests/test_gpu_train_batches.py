"""GPU: the training step's batch kernels (csrc/train.hip.h; train.sample_ids / gather_batch / train_losses / fused_loss) and
train.train(device_batches=True) against restatements written here from the definitions of include/azg.h -- a kernel is never compared
with itself.

Sampler: mix64 / u01 in Python integers, the Fisher-Yates chain over a dict as the virtual identity; id for id.  Uniformity is a property of
the definition (checked on the restatement: n = 8, batch = 3, 8192 streams, chi^2 over the 336 ordered triples = 321.4 / 342.3 / 332.9 for
seeds 0 / 1 / 12345 against 335 degrees of freedom); the GPU repeats seed 0 with the cap 335 + 5 sqrt(670) ~ 465.

Gather: bit-equal to torch indexing of each column.

Losses: the input recipe of tests/test_gpu_eval_losses.py (copied), log_pi = log(pi) where pi > 0 and -1e8 elsewhere (masked actions, and the
support entries that recipe zeroes: a log-softmax holds no -inf).  rows / out against float64 NumPy with that file's derived bound,
(A + 8) 2^-52 sum |terms| per row entry and B 2^-52 sum |rows| for the totals.  Gradients against torch autograd of train.loss_pi + 0.25
train.loss_v on the same f32 tensors: bit-equal where B and B P are powers of two (every scale factor is then exact), else relative 2^-21
-- at most three roundings on either side of a product of one difference with one constant.

End to end: SplendorV80Module on 256 examples, batch 32, 8 steps on one fixed batch_ids; the device path's final weights within
max(4 r, 1e-5 max|w|) per tensor of the legacy path's, r = the legacy path's own run-to-run spread; loss histories to 1e-5 relative."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
M64 = (1 << 64) - 1
FLT_MIN = np.float32(1.17549435e-38)
Q_WEIGHT = 0.3


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------
def mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def u01(seed, stream, counter):
    raw = mix64((mix64((mix64((seed ^ 0x9E3779B97F4A7C15) & M64) + stream) & M64) + counter) & M64)
    return (raw >> 11) * 2.0 ** -53


def restate_ids(n, batch, seed, stream):
    p, ids = {}, []
    for i in range(batch):
        m = n - i
        j = i + min(int(math.floor(u01(seed, stream & M64, i) * m)), m - 1)
        ids.append(p.get(j, j))
        p[j] = p.get(i, i)
    return np.array(ids, dtype=np.int64)


SAMPLER_CASES = [(1, 1), (5, 5), (64, 64), (100, 65), (1000, 512), (2 ** 31 - 1, 512), (8192, 8192)]


@pytest.mark.parametrize('n,batch', SAMPLER_CASES)
def test_sampler_equals_the_restatement_id_for_id(n, batch):
    from azg_amd import train
    seed, stream0 = 12345, 7
    want = np.stack([restate_ids(n, batch, seed, stream0 + s) for s in range(3)])
    three = train.sample_ids(n, batch, 3, seed, stream0).cpu().numpy()
    again = train.sample_ids(n, batch, 3, seed, stream0).cpu().numpy()
    assert three.dtype == np.int32 and three.shape == (3, batch)
    assert np.array_equal(three, want)
    assert np.array_equal(three, again)                                            # two calls give the same bits
    for s in range(3):                                                             # row s == a one-step call at stream0 + s
        one = train.sample_ids(n, batch, 1, seed, stream0 + s).cpu().numpy()
        assert np.array_equal(one[0], three[s]), s
        assert three[s].min() >= 0 and three[s].max() < n and len(np.unique(three[s])) == batch
    if n == batch:
        assert np.array_equal(np.sort(three[0]), np.arange(n))                     # a full permutation


def test_sampler_is_uniform_over_ordered_triples():
    from azg_amd import train
    ids = train.sample_ids(8, 3, 8192, 0, 0).cpu().numpy().astype(np.int64)
    counts = np.bincount(ids[:, 0] * 64 + ids[:, 1] * 8 + ids[:, 2], minlength=512)
    triples = np.array([a * 64 + b * 8 + c for a in range(8) for b in range(8) for c in range(8) if len({a, b, c}) == 3])
    assert len(triples) == 336 and counts[triples].sum() == 8192                   # every row holds three distinct ids below 8
    counts = counts[triples]
    e = 8192 / 336.0
    chi2 = float(((counts - e) ** 2 / e).sum())
    print('chi^2 over the 336 ordered triples: %.1f (335 degrees of freedom)' % chi2)
    assert chi2 <= 335 + 5 * math.sqrt(670)


def test_sampler_with_no_steps_launches_nothing():
    from azg_amd import train
    assert tuple(train.sample_ids(10, 4, 0, 1, 0).shape) == (0, 4)


# ---- gather ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,A,P', [(75, 21, 5), (392, 81, 2), (324, 3402, 2)])
@pytest.mark.parametrize('B', [1, 65])
def test_gather_is_bit_equal_to_torch_indexing(S, A, P, B):
    import torch
    from azg_amd import train
    n = 97
    r = np.random.RandomState(S + A + P + B)
    valids = r.randint(0, 2, (n, A)).astype(np.uint8) * r.randint(1, 256, (n, A)).astype(np.uint8)        # bytes other than 0 / 1
    assert valids.max() > 1 and (valids == 0).any()
    cols = (r.randint(-128, 128, (n, S)).astype(np.int8), r.rand(n, A).astype(np.float32), r.randn(n, P).astype(np.float32), valids,
            r.randn(n, P).astype(np.float32))
    ids = r.randint(0, n, B)
    ids[0] = n - 1
    if B > 1:
        ids[1], ids[2], ids[3], ids[-1] = 0, 5, 5, 0                                   # 0, n - 1 and repeated ids
    dev = tuple(torch.from_numpy(c).cuda() for c in cols)
    tid = torch.from_numpy(ids.astype(np.int32)).cuda()
    out = train.gather_batch(dev, tid)
    long = tid.long()
    for k, (o, c) in enumerate(zip(out, dev)):
        want = c[long] if k != 3 else (c[long] != 0).to(torch.uint8)
        assert o.dtype == c.dtype and o.shape == want.shape
        assert torch.equal(o.view(torch.uint8) if k != 3 else o, want.view(torch.uint8) if k != 3 else want), k     # bit for bit
    assert int(out[3].max()) == 1 and torch.equal(out[3].view(torch.bool), dev[3][long] != 0)


# ---- losses ----------------------------------------------------------------------------------------------------------------------------
def make_inputs(A, P, B, seed=0):
    """tests/test_gpu_eval_losses.py's recipe (support_only): targets random on a random set of 'valid' actions, normalised, EXACT zeros
    elsewhere; pi a softmax over the valid actions, 0 on the others, then per row  b % 3 == 0: pi = 0 on one action with t > 0;  b % 3 == 1
    (and the single row of B == 1): the maximum of pi twice;  b % 3 == 2: a subnormal pi on one action with t > 0.
    Here: log_pi = log(pi) (f64 log, rounded to f32) where pi > 0, -1e8 where pi == 0."""
    r = np.random.RandomState(seed + 7 * A + 100 * P + B)
    valid = r.rand(B, A) < 0.5
    valid[:, :4] = True
    t = np.where(valid, r.rand(B, A) + 0.01, 0.0)
    t = (t / t.sum(1, keepdims=True)).astype(np.float32)
    logits = r.randn(B, A) * 2.0
    e = np.where(valid, np.exp(logits), 0.0)
    pi = (e / e.sum(1, keepdims=True)).astype(np.float32)
    for b in range(B):
        sup = np.flatnonzero(valid[b])
        if b % 3 == 0:
            pi[b, sup[1]] = 0.0
        if b % 3 == 1 or B == 1:
            i, j = sup[2], sup[-1]
            pi[b, i] = pi[b, j] = np.float32(pi[b].max() * 1.5)
            t[b, j if b % 2 == 0 and B > 1 else i] = np.float32(t[b].max() * 1.25)
        if b % 3 == 2:
            pi[b, sup[3]] = np.float32(1e-40)
    assert (t[~valid] == 0).all() and (pi[~valid] == 0).all()
    with np.errstate(divide='ignore'):
        log_pi = np.where(pi > 0, np.log(pi.astype(np.float64)), -1e8).astype(np.float32)
    assert np.isfinite(log_pi).all() and (log_pi[t == 0] == np.float32(-1e8)).any()
    v = np.tanh(r.randn(B, P)).astype(np.float32)
    z = r.uniform(-1, 1, (B, P)).astype(np.float32)
    q = r.uniform(-1, 1, (B, P)).astype(np.float32)
    return dict(log_pi=log_pi, v=v, target_pi=t, z=z, q=q)


def restate(d, q_weight):
    """-> rows f64[B, 2], the sums of the terms' magnitudes f64[B, 2]"""
    t, lp = d['target_pi'].astype(np.float64), d['log_pi'].astype(np.float64)
    pos = d['target_pi'] > 0
    lt = np.where(pos, np.log(np.where(pos, t, 1.0)), 0.0)
    kl, kl_abs = np.where(pos, t * (lt - lp), 0.0), np.where(pos, t * (np.abs(lt) + np.abs(lp)), 0.0)
    qw = np.float64(np.float32(q_weight))
    dv = (d['z'].astype(np.float64) + qw * d['q'].astype(np.float64)) / (1.0 + qw) - d['v'].astype(np.float64)
    return np.stack([kl.sum(1), (dv * dv).sum(1)], axis=1), np.stack([kl_abs.sum(1), (dv * dv).sum(1)], axis=1)


def autograd_gradients(dev, q_weight):
    import torch
    from azg_amd import train
    lp, v = dev['log_pi'].clone().requires_grad_(True), dev['v'].clone().requires_grad_(True)
    (train.loss_pi(dev['target_pi'], lp) + 0.25 * train.loss_v(dev['z'], dev['q'], v, q_weight)).backward()
    torch.cuda.synchronize()
    return lp.grad, v.grad


LOSS_SHAPES = [(A, P, B) for A in (21, 81, 3402) for P in (2, 5) for B in (1, 3, 65)] + [(A, 2, 32) for A in (21, 81, 3402)]


@pytest.mark.parametrize('A,P,B', LOSS_SHAPES)
def test_losses_rows_totals_and_gradients(A, P, B):
    import torch
    from azg_amd import train
    d = make_inputs(A, P, B)
    dev = {k: torch.from_numpy(x).cuda() for k, x in d.items()}
    g_pi, g_v, rows, out = train.train_losses(dev['log_pi'], dev['v'], dev['target_pi'], dev['z'], dev['q'], Q_WEIGHT)
    g_pi2, g_v2, rows2, out2 = train.train_losses(dev['log_pi'], dev['v'], dev['target_pi'], dev['z'], dev['q'], Q_WEIGHT)
    assert torch.equal(rows, rows2) and torch.equal(out, out2) and torch.equal(g_pi, g_pi2) and torch.equal(g_v, g_v2)     # the same bits
    rows, out = rows.cpu().numpy(), out.cpu().numpy()
    want, mags = restate(d, Q_WEIGHT)
    bound = (A + 8) * 2.0 ** -52 * mags
    err = np.abs(rows - want)
    print('max |kernel - restatement| / bound: KL %.3g, SE %.3g' % tuple((err / np.maximum(bound, 1e-300)).max(0)))
    assert np.isfinite(rows).all() and (err <= bound).all(), (err.max(0), bound.min(0))
    tb = B * 2.0 ** -52 * np.abs(rows).sum(0)
    assert abs(out[0] - rows[:, 0].sum() / B) <= tb[0] / B and abs(out[1] - rows[:, 1].sum() / (B * P)) <= tb[1] / (B * P), (out, rows.sum(0), tb)
    # gradients against autograd on the same f32 tensors
    a_pi, a_v = autograd_gradients(dev, Q_WEIGHT)
    assert (g_pi[dev['target_pi'] == 0] == 0).all()                                 # t == 0: gradient 0, whatever log_pi holds
    pow2 = B & (B - 1) == 0 and (B * P) & (B * P - 1) == 0
    for name, g, a in (('log_pi', g_pi, a_pi), ('v', g_v, a_v)):
        rel = float(((g - a).abs() / a.abs().clamp_min(1e-30)).max())
        print('grad %s: max relative difference to autograd %.3g%s' % (name, rel, '  (bit-equal required)' if pow2 else ''))
        if pow2:
            assert torch.equal(g, a), name
        else:
            assert ((g - a).abs() <= 2.0 ** -21 * a.abs()).all(), (name, rel)


def test_fused_loss_value_and_backward_scale():
    import torch
    from azg_amd import train
    A, P, B = 81, 2, 32
    dev = {k: torch.from_numpy(x).cuda() for k, x in make_inputs(A, P, B).items()}
    g_pi, g_v, _, out_ref = train.train_losses(dev['log_pi'], dev['v'], dev['target_pi'], dev['z'], dev['q'], Q_WEIGHT)
    for scale in (1.0, 3.0):
        lp, v = dev['log_pi'].clone().requires_grad_(True), dev['v'].clone().requires_grad_(True)
        out = torch.zeros(2, dtype=torch.float64, device='cuda:0')
        L = train.fused_loss(lp, v, dev['target_pi'], dev['z'], dev['q'], Q_WEIGHT, out=out)
        assert L.dtype == torch.float32 and L.dim() == 0 and torch.equal(out, out_ref)
        o = out.cpu().numpy()
        assert L.item() == np.float32(o[0] + 0.25 * o[1])
        (scale * L).backward()
        assert torch.equal(lp.grad, g_pi * scale) and torch.equal(v.grad, g_v * scale), scale


def test_refused_arguments_launch_nothing():
    import ctypes as C
    import torch
    from azg_amd import _lib
    L = _lib.lib()
    ids = torch.full((2, 4), -7, dtype=torch.int32, device='cuda:0')
    for n, batch in ((3, 4), (2 ** 31, 4)):
        assert L.azg_train_sample_ids(n, batch, 2, 0, 0, C.c_void_p(ids.data_ptr()), None) == -1
        assert 'azg_train_sample_ids' in L.azg_last_error().decode()
    torch.cuda.synchronize()
    assert (ids == -7).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _module():
    import torch
    from azg_amd.train import SplendorV80Module
    z = np.load(os.path.join(GOLDEN, 'weights_splendor2_v80.npz'))
    m = SplendorV80Module(num_players=2, dropout=0.0)
    m.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
    return m


def _examples():
    d = np.load(os.path.join(GOLDEN, 'netfwd_splendor2_v80.npz'))
    n = len(d['boards'])
    rng = np.random.default_rng(0)
    z = np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0).astype(np.float32) * np.array([[1.0, -1.0]], dtype=np.float32)
    q = (0.5 * z).astype(np.float32)
    return (d['boards'].reshape(n, -1), d['pi'], z, d['masks'], q)


def _run(ex, **kw):
    from azg_amd import train
    m = _module()
    hist = train.train(m, ex, learn_rate=3e-3, batch_size=32, epochs=1, q_weight=0.5, device='cuda:0', **kw)
    return np.array(hist, dtype=np.float64), {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def test_device_batches_train_like_the_legacy_path():
    from azg_amd import train
    ex = _examples()
    n = len(ex[0])
    assert n == 256
    batch_ids = np.stack([np.random.RandomState(100 + s).permutation(n)[:32] for s in range(8)])
    h1, w1 = _run(ex, batch_ids=batch_ids)
    h2, w2 = _run(ex, batch_ids=batch_ids)
    hd, wd = _run(ex, batch_ids=batch_ids, device_batches=True)
    assert h1.shape == hd.shape == (8, 2)
    worst = 0.0
    for k in w1:
        r = np.abs(w1[k] - w2[k]).max()
        bound = max(4 * r, 1e-5 * np.abs(w1[k]).max())
        diff = np.abs(wd[k] - w1[k]).max()
        worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
        assert diff <= bound, (k, diff, r, bound)
    print('largest weight difference device vs legacy, as a fraction of its bound: %.3g' % worst)
    print('loss histories: max relative difference %.3g' % (np.abs(hd - h1) / np.abs(h1)).max())
    assert (np.abs(hd - h1) <= 1e-5 * np.abs(h1)).all(), (hd, h1)
    # drawn on the device: seed 5 twice gives the same history, and its ids are sample_ids(n, 32, 8, 5, 0)
    s1, _ = _run(ex, device_batches=True, seed=5)
    s2, _ = _run(ex, device_batches=True, seed=5)
    assert np.array_equal(s1, s2)
    drawn = train.sample_ids(n, 32, 8, 5, 0).cpu().numpy()
    assert np.array_equal(drawn, np.stack([restate_ids(n, 32, 5, s) for s in range(8)]))
    s3, _ = _run(ex, device_batches=True, batch_ids=drawn)
    assert np.array_equal(s1, s3)
    assert not np.array_equal(s1, hd)
