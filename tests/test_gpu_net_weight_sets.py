"""GPU: every engine net, in every operand form its constructor offers, on weights other than the shipped ones -- the fresh and the
calibrated set of tests/netweights.py (what they can detect is proved on the CPU, tests/test_net_weight_sets.py) and, for the nets
without an after-training check elsewhere, the weights after one training epoch from the calibrated set.  The reference is the
trainable module itself in float64; the bound is the project's own, element by element:
|kernel - f64| <= 1e-5 + |f32 torch module - f64|.  One batch of 70 boards per case (ragged for every per-workgroup sample count in
use: 4, 8, 16, 64), with a no-valid-action row, a single-valid-action row and the four leave-one-out rows of the CPU test in it."""
import functools

import numpy as np
import pytest
import torch

import netweights as nw

pytestmark = pytest.mark.gpu

B = 70
DEV = 'cuda:0'
MB1D = nw.MB1D


CASES = [(c.tag, f) for c in nw.configs() for f in nw.forms(c)]
# the nets without an after-training check elsewhere (V82 / V83 and Botanik have one).  Akropolis (V31) is not trained here: DESIGN.md
# §5, "Open fault: training AkropolisV31Module on the GPU"
TRAINED = [c.tag for c in nw.configs() if c.row.version not in (82, 83, 10, 11, 31)]


@functools.lru_cache(maxsize=None)
def _game(tag):
    return nw.game(nw.config(tag))


@functools.lru_cache(maxsize=None)
def _batch(tag):
    b, m = nw.gpu_boards(tag, B)
    return b.reshape(B, -1).contiguous().to(DEV), m.contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(tag, weights):
    """(module on the GPU, f64 pi, f64 v, |f32 - f64| of pi, of v): computed once per weight set, shared by its operand forms"""
    module = nw.WEIGHT_SETS[weights](nw.config(tag)).to(DEV)
    return (module,) + _module_reference(tag, module)


def _module_reference(tag, module):
    b, m = _batch(tag)
    shaped = b.reshape((B,) + tuple(nw._fixture(tag)[0].shape[1:]))
    p64, v64 = nw.float64_outputs(module, shaped, m)
    p32, v32 = nw.float32_outputs(module, shaped, m)
    return p64, v64, (p32 - p64).abs(), (v32 - v64).abs()


def _check(label, ev, tag, p64, v64, dp, dv):
    b, m = _batch(tag)
    pi, v = (t.clone() for t in ev.predict_batch(b, m))
    pi2, v2 = ev.predict_batch(b, m)
    torch.cuda.synchronize()
    share_pi = ((pi.double() - p64).abs() / (1e-5 + dp))
    share_v = ((v.double() - v64).abs() / (1e-5 + dv))
    print('%s: largest share of the bound used: pi %.3f, v %.3f' % (label, float(share_pi.max()), float(share_v.max())))
    assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all())
    assert float(share_pi.max()) <= 1.0, (label, 'pi', float(share_pi.max()), int(share_pi.amax(dim=1).argmax()))
    assert float(share_v.max()) <= 1.0, (label, 'v', float(share_v.max()), int(share_v.amax(dim=1).argmax()))
    some = m.bool().any(dim=1)
    assert int((~some).sum()) >= 1 and int((m.sum(dim=1) == 1).sum()) >= 1                   # the two edited rows are in the batch
    assert bool((pi[some][m[some] == 0] == 0).all())
    assert float((pi.double().sum(dim=1) - 1.0).abs().max()) <= 1e-5
    assert torch.equal(pi, pi2) and torch.equal(v, v2)


@pytest.mark.parametrize('weights', sorted(nw.WEIGHT_SETS))
@pytest.mark.parametrize('tag,form', CASES)
def test_kernel_matches_float64_module(tag, form, weights):
    from azg_amd import nnet
    cfg = nw.config(tag)
    module, p64, v64, dp, dv = _reference(tag, weights)
    ev = nw.evaluator(cfg, form, module, B, DEV)
    assert isinstance(ev, nnet._EngineNet)
    if form == 'default' and tag.startswith(MB1D):
        assert ev.h2                                                                          # (the f16 x 2 form is the default)
    _check('%s %s %s' % (tag, form, weights), ev, tag, p64, v64, dp, dv)


@pytest.mark.parametrize('tag', TRAINED)
def test_evaluator_after_training_from_the_calibrated_set(tag):
    """NNetWrapper on the calibrated weights, one epoch on 64 examples: the evaluator is rebuilt (the cache is invalidated) and meets
    the same bound against the float64 copy of the module as it is now, running statistics after their momentum updates included"""
    from azg_amd import nnet
    from azg_amd.nnet_wrapper import NNetWrapper
    cfg = nw.config(tag)
    g = _game(tag)
    w = NNetWrapper(g, dict(nn_version=cfg.row.version, learn_rate=1e-3, batch_size=32, epochs=1, dropout=0.0))
    assert type(w.nnet) is cfg.row.module
    w.nnet.load_state_dict(nw.calibrated(cfg).state_dict(), strict=True)
    before = w.evaluator(B)
    eb, em = nw.raw_boards(tag, 64)
    pi, _ = nw.float32_outputs(w.nnet.to(DEV), eb, em)
    rng = np.random.default_rng(0)
    P = nw.shape(cfg)[0]
    ex = (eb.reshape(64, -1).numpy(), pi.float().cpu().numpy(), rng.uniform(-1, 1, (64, P)).astype(np.float32), em.numpy(),
          rng.uniform(-1, 1, (64, P)).astype(np.float32))
    sd0 = {k: t.detach().clone().cpu() for k, t in w.nnet.state_dict().items()}
    hist = w.train(ex, seed=0)
    assert len(hist) >= 1 and np.all(np.isfinite(np.asarray(hist, dtype=np.float64)))
    sd1 = {k: t.detach().cpu() for k, t in w.nnet.state_dict().items()}
    assert any(not torch.equal(sd0[k], sd1[k]) for k in sd0 if k.endswith('weight'))
    stats = [k for k in sd0 if k.endswith('running_var')]
    assert all(not torch.equal(sd0[k], sd1[k]) for k in stats)
    after = w.evaluator(B)
    assert after is not before and isinstance(after, nnet._EngineNet)
    w.nnet.eval()
    _check('%s trained' % tag, after, tag, *_module_reference(tag, w.nnet.to(DEV)))
