"""GPU: the validation leg of the NeuralNet plugin surface -- NNetWrapper.evaluate / evaluate_details (GenericNNetWrapper.py:159-177),
train(..., validation_set, save_folder, every) (:86-90) and tools/train_offline.py (:347-441) -- on Splendor-2p (V80, A = 81) and
Minivilles-2 (V82, A = 21: a second net family and a row shorter than a wave).

The yardstick of `evaluate` is the reference's definition: the trainable module in eval() mode, converted to float64, loss_pi + loss_v of
train.py.  The tolerance is not a constant: the same expression is evaluated in float32 torch on the GPU and its deviation from the float64
result is measured; the engine path (fp32-accurate forward, DESIGN.md 3.3, f64 losses) may deviate at most ENGINE_FACTOR times as much --
the slack of a different but equally precise summation order and no more -- with a floor of 1e-6 relative.
Measured (profiles/r12_eval_losses.md): relative deviation of loss_pi + loss_v from the float64 module on the 256 examples --
Splendor-2p: float32 torch 1.17e-07, engine 5.7e-08; Minivilles-2: float32 torch 1.12e-07, engine 7.5e-08."""
import copy
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_FACTOR = 4.0
REL_FLOOR = 1e-6
PLIES = (2, 5, 9, 14)                # random plies from the initial boards: 64 boards each, mid-game (status "cap") rows
NETS = {'splendor2': ('splendor', 2, 80, 'weights_splendor2_v80.npz'), 'minivilles2': ('minivilles', 2, 82, 'weights_minivilles2_v82.npz')}
_CACHE = {}


def setup(name, golden_dir):
    """-> (game, state_dict, cols = (boards int8[n, S], pi, z, valids u8, q) numpy arrays, examples: the reference's compressed 5-tuples)"""
    if name in _CACHE:
        return _CACHE[name]
    import torch
    from azg_amd import formats, games
    gname, P, _, wfile = NETS[name]
    g = games.import_game(gname, num_players=P)
    z = np.load(os.path.join(golden_dir, wfile))
    sd = {k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')}
    boards = []
    for m in PLIES:
        start = g.init_boards_batch(64, stream0=1000 * m)
        po = g.playouts_batch(start, None, k=1, max_plies=m, stream0=50000 + 1000 * m, final_boards=True)
        cap = po.status[:, 0] == 1                                                  # the playout stopped at max_plies: a mid-game board
        boards.append(g.canonical_batch(po.boards[:, 0][cap].contiguous(), po.players[:, 0][cap].contiguous()))
    boards = torch.cat(boards)
    valids = g.valid_moves_batch(boards, None)
    keep = valids.sum(1) > 0
    boards, valids = boards[keep].cpu().numpy(), valids[keep].cpu().numpy()
    n = len(boards)
    assert n >= 128, n
    r = np.random.RandomState(len(name))
    pi = np.where(valids != 0, r.rand(n, g.A) + 0.01, 0.0)
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    cols = (boards, pi, r.uniform(-1, 1, (n, g.P)).astype(np.float32), valids, r.uniform(-1, 1, (n, g.P)).astype(np.float32))
    examples = list(formats.examples_to_iteration(cols, g.getBoardSize(), compress=True))
    _CACHE[name] = (g, sd, cols, examples)
    return _CACHE[name]


def wrapper(name, g, sd, **kw):
    from azg_amd.nnet_wrapper import NNetWrapper
    args = dict(nn_version=NETS[name][2], learn_rate=1e-3, batch_size=64, epochs=1, dropout=0.0, q_weight=0.5)
    args.update(kw)
    w = NNetWrapper(g, args)
    w.nnet.load_state_dict(sd, strict=True)
    return w


def module_losses(module, cols, dtype, q_weight=0.5):
    """the reference's evaluate on the trainable module in eval() mode at `dtype` -> (loss_pi + loss_v, pi probabilities [n, A])"""
    import torch
    from azg_amd import train
    m = copy.deepcopy(module).to('cuda:0').to(dtype).eval()
    # (the modules cast their int8 boards with .float(): the float64 copy takes them as float64 at its first layer)
    m.first_layer.register_forward_pre_hook(lambda mod, inp: (inp[0].to(dtype),))
    boards, pi, z, valids, q = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in cols]
    with torch.no_grad():
        log_pi, v = m(boards, valids.bool())
        assert log_pi.dtype == dtype and v.dtype == dtype
        loss = train.loss_pi(pi.to(dtype), log_pi) + train.loss_v(z.to(dtype), q.to(dtype), v, q_weight)
    return loss.item(), torch.exp(log_pi)


@pytest.mark.parametrize('name', sorted(NETS))
def test_evaluate_against_the_float64_module(name, golden_dir):
    import torch
    g, sd, cols, examples = setup(name, golden_dir)
    w = wrapper(name, g, sd)
    want, _ = module_losses(w.nnet, cols, torch.float64)
    f32, _ = module_losses(w.nnet, cols, torch.float32)
    got = w.evaluate(examples)
    dev32, dev_engine = abs(f32 - want) / abs(want), abs(got - want) / abs(want)
    print('%s: n %d  float64 %.12g  float32 torch %.12g (rel %.3g)  engine %.12g (rel %.3g)' % (name, len(examples), want, f32, dev32, got, dev_engine))
    assert isinstance(got, float)
    assert dev_engine <= max(ENGINE_FACTOR * dev32, REL_FLOOR), (dev_engine, dev32)
    d = w.evaluate_details(examples)
    assert d['loss_pi'] + d['loss_v'] == got and w.evaluate(cols) == got             # (five arrays are taken like the example list)


@pytest.mark.parametrize('name', sorted(NETS))
def test_evaluate_details(name, golden_dir):
    import torch
    g, sd, cols, examples = setup(name, golden_dir)
    w = wrapper(name, g, sd)
    n = len(examples)
    d = w.evaluate_details(examples)
    assert sorted(d) == ['floored', 'loss_pi', 'loss_v', 'n', 'top1'] and d['n'] == n and d['floored'] == 0
    # top-1 agreement: exact on the rows whose float64 argmax is further ahead than the forward of the engine deviates (both of the two
    # leading probabilities can move by that much)
    _, pi64 = module_losses(w.nnet, cols, torch.float64)
    pi_e, _ = w.predict_batch(torch.from_numpy(cols[0]).cuda(), torch.from_numpy(cols[3]).cuda())
    fwd_dev = float((pi_e.double() - pi64).abs().max())
    top2 = torch.topk(pi64, 2, dim=1).values
    safe = ((top2[:, 0] - top2[:, 1]) > 2 * fwd_dev).cpu().numpy()
    print('%s: forward deviation %.3g, %d of %d rows below the margin' % (name, fwd_dev, int((~safe).sum()), n))
    assert (~safe).sum() <= 0.05 * n
    agree = (pi64.argmax(1).cpu().numpy() == np.argmax(cols[1], 1))[safe]
    ds = w.evaluate_details([c[safe] for c in cols])
    assert ds['n'] == int(safe.sum()) and round(ds['top1'] * ds['n']) == int(agree.sum()) and abs(ds['top1'] * ds['n'] - agree.sum()) < 1e-9
    # in two chunks (the second one short): every example counted once; both are fp32-accurate evaluations of the same losses
    d2 = w.evaluate_details(examples, batch=n - 37)
    assert d2['n'] == n and d2['floored'] == 0 and abs(d2['loss_pi'] - d['loss_pi']) <= REL_FLOOR * d['loss_pi'] \
        and abs(d2['loss_v'] - d['loss_v']) <= REL_FLOOR * d['loss_v']


def test_periodic_validation_in_train(golden_dir, tmp_path):
    import torch
    from azg_amd.nnet_wrapper import NNetWrapper
    g, sd, cols, examples = setup('splendor2', golden_dir)
    n = len(examples)
    assert n >= 192                                                                # three steps of 64: the step that saves exists
    steps = n // 64
    val = examples[:64]
    w = wrapper('splendor2', g, sd)
    before = w.evaluate(val)
    said = []
    hist = w.train(examples, validation_set=val, save_folder=str(tmp_path), every=2, seed=3, log=said.append)
    due = [s for s in range(steps) if s % 2 == 0]
    assert [s for s, _ in w.validation_history] == due and all(isinstance(x, float) and np.isfinite(x) for _, x in w.validation_history)
    assert len([t for t in said if 'validation' in t]) == len(due)
    assert sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / 'intermediary_*.pt'))) == ['intermediary_%d.pt' % s for s in due if s > 0]
    w2 = NNetWrapper(g, dict(nn_version=80))
    assert w2.load_checkpoint(str(tmp_path), 'intermediary_2.pt') is not None and not w2.requestKnowledgeTransfer
    # the evaluator was rebuilt from the weights of the moment: every validation saw another net
    losses = [before] + [x for _, x in w.validation_history] + [w.evaluate(val)]
    print('validation losses: before %.6f, during %s, after %.6f' % (losses[0], ['%.6f' % x for x in losses[1:-1]], losses[-1]))
    assert len(set(losses)) == len(losses)
    assert w2.evaluate(val) == w.validation_history[1][1]                          # intermediary_2.pt is the net validated at step 2
    assert w.nnet.training is False                                                # train() leaves the module in eval(), as before
    # validation does not disturb training: the same call without a validation set gives the same history, bit for bit
    plain = wrapper('splendor2', g, sd)
    hist0 = plain.train(examples, seed=3)
    assert len(hist) == steps and hist == hist0
    assert plain.validation_history == []
    for k, t in w.nnet.state_dict().items():
        assert torch.equal(t.cpu(), plain.nnet.state_dict()[k].cpu()), k


def test_validation_set_needs_every(golden_dir):
    g, sd, cols, examples = setup('splendor2', golden_dir)
    w = wrapper('splendor2', g, sd)
    for every in (0, -1):
        with pytest.raises(ValueError):
            w.train(examples, validation_set=examples[:64], every=every)
    assert w.validation_history == []


def test_offline_trainer(golden_dir, tmp_path):
    from azg_amd import formats
    from azg_amd.nnet_wrapper import NNetWrapper
    g, sd, cols, examples = setup('splendor2', golden_dir)
    wrapper('splendor2', g, sd).save_checkpoint(str(tmp_path), 'in.pt', additional_keys=dict(nn_version=80, cpuct=1.25))
    half = len(examples) // 2
    formats.save_train_examples(str(tmp_path / 'checkpoint.examples'), [examples[:half], examples[half:]])
    tool = os.path.join(ROOT, 'tools', 'train_offline.py')
    common = [sys.executable, tool, 'splendor', '-i', str(tmp_path / 'in.pt')]
    p = subprocess.run(common + ['-T', str(tmp_path / 'checkpoint.examples'), '-o', str(tmp_path / 'out_'), '-b', '32', '-p', '1', '-d', '0.0'],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    n_test = len(examples) // 10
    assert 'V80 -> nb params' in p.stdout and 'training %d, testing %d; number of epochs 1' % (len(examples) - n_test, n_test) in p.stdout
    assert 'validation loss' in p.stdout
    out = glob.glob(str(tmp_path / 'out_*' / 'last.pt'))
    assert len(out) == 1, out
    w = NNetWrapper(g, dict(nn_version=80))
    assert w.load_checkpoint(os.path.dirname(out[0]), 'last.pt') is not None and not w.requestKnowledgeTransfer
    assert any(not np.array_equal(t.cpu().numpy(), sd[k].numpy()) for k, t in w.nnet.state_dict().items() if k.endswith('weight'))
