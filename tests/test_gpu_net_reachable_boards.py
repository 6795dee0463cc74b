"""GPU: every engine net, in every operand form its constructor offers, on the boards of every reachable position -- the batches of
tests/reachboards.py (the canonical boards of the env-coverage fixtures with the oracle's masks; what they can detect is proved on the
CPU, tests/test_net_reachable_boards.py) -- with the shipped and the calibrated weights.  The reference is the trainable module itself in
float64; the bound is the project's own, element by element: |kernel - f64| <= 1e-5 + |f32 torch module - f64|.  One predict_batch over
the whole batch (411 to 5722 rows) per case, evaluated twice for bit equality, and its first 1, 63 and 65 rows evaluated alone."""
import copy
import functools

import pytest
import torch

import netweights as nw
import reachboards as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CHUNK = 1024                   # rows per forward of the float64 / float32 module
TAILS = (1, 63, 65)
# (tag, weight set, form), the forms of one weight set next to each other: they share its reference
CASES = [(t, w, f) for t in R.tags() for w in R.weight_sets(t) for f in nw.forms(R.config(t))]


@functools.lru_cache(maxsize=2)
def _batch(tag):
    b, m, meta = R.batch(tag)
    return b.reshape(len(b), -1).contiguous().to(DEV), m.contiguous().to(DEV), tuple(b.shape[1:]), meta


@functools.lru_cache(maxsize=2)
def _reference(tag, weights):
    """(module on the GPU, f64 pi, f64 v, |f32 - f64| of pi, of v): computed once per weight set, shared by its operand forms"""
    module = copy.deepcopy(R.module(tag, weights)).to(DEV)
    b, m, shape, _ = _batch(tag)
    shaped = b.reshape((len(b),) + shape)
    p64, v64, _ = nw.float64_outputs_and_max_activation(module, shaped, m, chunk=CHUNK)
    f32 = [nw.float32_outputs(module, shaped[lo:lo + CHUNK], m[lo:lo + CHUNK]) for lo in range(0, len(b), CHUNK)]
    p32, v32 = torch.cat([p for p, _ in f32]), torch.cat([v for _, v in f32])
    return module, p64, v64, (p32 - p64).abs(), (v32 - v64).abs()


def _worst(label, what, share, meta):
    """the failure text: the worst element of a [rows, outputs] tensor of shares of the bound"""
    row = int(share.amax(dim=1).argmax())
    col = int(share[row].argmax())
    return '%s: %s %d of %s uses %.3f of the bound (%d elements over it)' % (label, what, col, R.name(meta, row), float(share[row, col]),
                                                                             int((share > 1.0).sum()))


@pytest.mark.parametrize('tag,weights,form', CASES)
def test_kernel_matches_float64_module_on_reachable_boards(tag, weights, form):
    from azg_amd import nnet
    cfg = R.config(tag)
    b, m, _, meta = _batch(tag)
    n = len(b)
    module, p64, v64, dp, dv = _reference(tag, weights)
    ev = nw.evaluator(cfg, form, module, n, DEV)
    assert isinstance(ev, nnet._EngineNet)
    label = '%s %s %s' % (tag, form, weights)
    pi, v = (t.clone() for t in ev.predict_batch(b, m))
    pi2, v2 = (t.clone() for t in ev.predict_batch(b, m))
    torch.cuda.synchronize()
    assert pi.shape == p64.shape and v.shape == v64.shape
    share_pi = (pi.double() - p64).abs() / (nw.CONTRACT + dp)
    share_v = (v.double() - v64).abs() / (nw.CONTRACT + dv)
    print('%s: %d rows, largest share of the bound used: pi %.3f, v %.3f (f32 module: pi %.1e, v %.1e)'
          % (label, n, float(share_pi.max()), float(share_v.max()), float(dp.max()), float(dv.max())))
    assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all()), label
    assert float(share_pi.max()) <= 1.0, _worst(label, 'pi of action', share_pi, meta)
    assert float(share_v.max()) <= 1.0, _worst(label, 'v of seat', share_v, meta)
    some = m.bool().any(dim=1)
    assert int((~some).sum()) >= 1 and int((m.sum(dim=1) == 1).sum()) >= 1
    leak = ((pi != 0) & (m == 0) & some[:, None]).any(dim=1)
    assert not bool(leak.any()), '%s: pi is not 0 on a masked action of %s' % (label, R.name(meta, int(leak.int().argmax())))
    off = (pi.double().sum(dim=1) - 1.0).abs()
    assert float(off.max()) <= 1e-5, '%s: pi sums to 1 %+.1e in %s' % (label, float(off.max()), R.name(meta, int(off.argmax())))
    same = (pi == pi2).all(dim=1) & (v == v2).all(dim=1)
    assert bool(same.all()), '%s: the second evaluation differs in %s' % (label, R.name(meta, int((~same).int().argmax())))
    for k in TAILS:                                                   # ragged tails: a short batch gives the same rows bit for bit
        pk, vk = ev.predict_batch(b[:k].contiguous(), m[:k].contiguous())
        assert torch.equal(pk[:k], pi[:k]) and torch.equal(vk[:k], v[:k]), '%s: the first %d rows alone differ from the full batch' % (label, k)
