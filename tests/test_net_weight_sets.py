"""CPU: what the weight sets of tests/netweights.py can detect, proved on the reference (the trainable module in float64) alone --
every tensor of the calibrated set moves the output clear of the bound the GPU test applies, activations stay inside the f16 x 2
kernels' range, both sets give non-degenerate outputs, and the plain-torch nets the evaluators are packed from (BatchNorm folded,
layouts re-expressed) agree with the modules in float64."""
import pytest
import torch

import netweights as nw

TAGS = [c.tag for c in nw.configs()]
SETS = sorted(nw.WEIGHT_SETS)


def test_there_are_21_configs_covering_every_engine_net():
    from azg_amd.nnet_wrapper import ENGINE_NETS
    assert len(TAGS) == 21 == len(set(TAGS))
    assert {c.row for c in nw.configs()} == set(ENGINE_NETS)
    assert all(len(v) <= 2 for v in nw.EXCUSED.values())


def test_boards_edits_the_last_two_masks():
    b, m = nw.boards('botanik_v10', 6)
    rb, rm = nw.raw_boards('botanik_v10', 6)
    assert torch.equal(b, rb) and torch.equal(m[:4], rm[:4])
    assert int(m[4].sum()) == 0 and int(m[5].sum()) == 1
    b, m = nw.boards('splendor2_v80', 300)                           # (longer than the fixture: tiled)
    assert b.shape[0] == 300 and torch.equal(b[256], b[0])


@pytest.mark.parametrize('tag', TAGS)
def test_every_tensor_counts(tag):
    """a. removing the perturbation of any single tensor of the calibrated set moves the float64 pi or v by at least
    10 x (1e-5 + max |f32 - f64| of that net on those boards): a kernel that lost the tensor, or applied it a tenth off, lies clear of
    the GPU test's bound"""
    cfg = nw.config(tag)
    err, effects = nw.leave_one_out(cfg)
    want = nw.bound(err)
    names = set(nw.tensors(nw.fresh(cfg)))
    assert set(effects) == names and 'lowvalue' not in names and set(nw.amplitudes()[tag]) == names
    excused = nw.EXCUSED.get(tag, {})
    low = {k: e for k, e in effects.items() if e < want and k not in excused}
    print('%s: %d tensors, f32 error %.2e, bound %.2e, smallest effect %.2e' % (tag, len(effects), err, want, min(effects.values())))
    assert not low, (want, low)


@pytest.mark.parametrize('weights', SETS)
@pytest.mark.parametrize('tag', TAGS)
def test_activations_stay_in_range(tag, weights):
    """b. the largest |output| of any submodule is at most 256, a quarter of the f16 x 2 kernels' documented range (|x| < 1023): room
    for their 6 x Hardswish and pre-activation values.  Measured on the 70 boards the GPU test evaluates, so the claim covers the batch
    the f16 x 2 kernels see"""
    cfg = nw.config(tag)
    top = nw.max_activation(nw.WEIGHT_SETS[weights](cfg), *nw.gpu_boards(tag))
    print('%s %s: largest activation %.1f' % (tag, weights, top))
    assert top <= 256.0


@pytest.mark.parametrize('weights', SETS)
@pytest.mark.parametrize('tag', TAGS)
def test_outputs_are_not_degenerate(tag, weights):
    """c. on the fixture boards, at least half the rows are informative: the largest pi differs from uniform over the valid actions by
    more than 1e-3 and no component of v is saturated (|v| < 0.999) in the same row.  (A fresh module cannot be steered: some of its
    rows do saturate v, so the count is of rows that pass both conditions.)"""
    cfg = nw.config(tag)
    b, m = nw.raw_boards(tag, 64)
    pi, v = nw.float64_outputs(nw.WEIGHT_SETS[weights](cfg), b, m)
    n = m.sum(dim=1).double()
    peaked = (((pi * m).amax(dim=1) - 1.0 / n.clamp(min=1)).abs() > 1e-3) & (n > 0)
    good = peaked & (v.abs().amax(dim=1) < 0.999)
    print('%s %s: %d of %d rows peaked, %d of them with unsaturated v' % (tag, weights, int(peaked.sum()), len(b), int(good.sum())))
    assert int(good.sum()) * 2 >= len(b), (int(peaked.sum()), int(good.sum()))


@pytest.mark.parametrize('weights', SETS)
@pytest.mark.parametrize('tag', TAGS)
def test_folded_net_agrees_with_the_module(tag, weights):
    """d. the plain-torch nnet.* net the evaluator is packed from, built in float64 from the module's state_dict, equals the float64
    module within 1e-9 (BatchNorm folds, flatten permutations, lookup-table folds)"""
    cfg = nw.config(tag)
    module = nw.WEIGHT_SETS[weights](cfg)
    b, m = nw.boards(tag, nw.LOO_BOARDS)
    p64, v64 = nw.float64_outputs(module, b, m)
    net = nw.base_net(cfg, module, device='cpu', dtype=torch.float64)
    pi, v = net.predict_batch(b, m)
    assert pi.dtype == torch.float64 and v.dtype == torch.float64
    assert float((pi - p64).abs().max()) <= 1e-9, float((pi - p64).abs().max())
    assert float((v - v64).abs().max()) <= 1e-9, float((v - v64).abs().max())
