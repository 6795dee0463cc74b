"""CPU: what the batches of tests/reachboards.py (the canonical boards of the env-coverage fixtures, with the oracle's masks) can detect,
proved on the reference alone -- the trainable module in float64 -- so that tests/test_gpu_net_reachable_boards.py cannot pass for lack
of teeth: the boards hold (cell, value) pairs that no netfwd_<tag>.npz row has, activations of the shipped and the calibrated weights stay
inside the f16 x 2 kernels' range on them, the value head is not saturated away, finished games and single-action masks are in every
batch, and the shipped module is the one the reference's forward vectors were computed with."""
import os

import numpy as np
import pytest
import torch

import netweights as nw
import reachboards as R

TAGS = R.tags()
CASES = [(t, w) for t in TAGS for w in R.weight_sets(t)]
MIN_NEW_PAIRS = 40             # the smallest count is Abalone Belgian's: 43 on the plain file alone
MAX_ACTIVATION = 256.0         # the limit of test_net_weight_sets.py: a quarter of the f16 x 2 range (|x| < 1023)
MIN_UNSATURATED = 0.25         # share of rows with |v| < 0.999 in every seat
CHUNK = 1024                   # rows per float64 forward


def test_the_batches_are_the_fixture_rows_of_every_config():
    assert TAGS[:21] == [c.tag for c in nw.configs()] and len(TAGS) == 23
    for tag in TAGS:
        b, m, meta = R.batch(tag)
        P, A = nw.shape(R.config(tag))
        files = ['envcover_%s.npz' % v for v in R.variants(tag)]
        assert all(os.path.exists(os.path.join(R.GOLDEN, f)) for f in files)
        plain = meta['edit'] == ''
        n = int(plain.sum())
        assert n == sum(len(np.load(os.path.join(R.GOLDEN, f))['action']) for f in files) and plain[:n].all()
        assert len(b) == len(m) == n + 2 + (R.EDIT_ROWS if tag.startswith('akropolis') else 0) and m.shape[1] == A
        assert all(len(v) == len(b) for v in meta.values()) and set(meta['file'].tolist()) == set(files)
        assert b.dtype == torch.int8 and m.dtype == torch.uint8 and tuple(b.shape[1:]) == tuple(nw._fixture(tag)[0].shape[1:])
        d = np.load(os.path.join(R.GOLDEN, files[0]))
        assert np.array_equal(b[:len(d['action'])].reshape(len(d['action']), -1).numpy(), d['canonical'])
        assert np.array_equal(meta['row'][:len(d['row'])], d['row']) and np.array_equal(meta['group'][:len(d['row'])], d['group'])
        # the edited rows: copies of batch rows, as netweights.boards edits them
        assert list(meta['edit'][n:n + 2]) == ['no valid action', 'one valid action']
        assert int(m[n].sum()) == 0 and int(m[n + 1].sum()) == 1 and torch.equal(b[n:n + 2], b[meta['source'][n:n + 2]])
        assert bool(m[meta['source'][n + 1], int(m[n + 1].argmax())])
    assert len(R.batch('abalone_v21')[0]) > 5000 and max(len(R.batch(t)[0]) for t in TAGS) < 6000
    assert R.batch('botanik_v10')[2]['file'][0] == R.batch('botanik_v11')[2]['file'][0] == 'envcover_botanik.npz'


@pytest.mark.parametrize('tag', TAGS)
def test_boards_hold_pairs_the_old_fixture_lacks(tag):
    """a. at least 40 (cell, value) pairs of the batch occur in no row of netfwd_<tag>.npz"""
    new = R.new_pairs(tag)
    count, cells = int(new.sum()), int(new.any(axis=1).sum())
    print('%s: %d rows, %d new (cell, value) pairs, %d of %d cells with a never-seen value' % (tag, len(R.batch(tag)[0]), count, cells, len(new)))
    assert count >= MIN_NEW_PAIRS
    if tag.startswith('akropolis'):
        b, _, meta = R.batch(tag)
        P = nw.shape(R.config(tag))[0]
        plain = b[meta['edit'] == ''].numpy()
        old = nw._fixture(tag)[0]
        for p in range(P):
            codes = np.unique(plain[..., p])
            print('%s: description plane %d holds the codes %s (netfwd: %s)' % (tag, p, codes.tolist(), np.unique(old[..., p]).tolist()))
            assert codes.min() >= 0 and codes.max() <= 11 and len(codes) >= 10
        sites = np.unique(plain[:, :P + 2, :3, 3 * P + 1])
        print('%s: the construction sites hold the codes %s' % (tag, sites.tolist()))


def _outputs(tag, weights):
    b, m, _ = R.batch(tag)
    return nw.float64_outputs_and_max_activation(R.module(tag, weights), b, m, chunk=CHUNK)


@pytest.mark.parametrize('tag,weights', CASES)
def test_activations_stay_in_range_and_values_show(tag, weights):
    """b. the largest |output| of any submodule over the whole batch is at most 256 for the shipped and the calibrated weights;
    c. at least a quarter of the rows have |v| < 0.999 in every seat: a saturated tanh would hide the value head from a 1e-5 bound"""
    pi, v, top = _outputs(tag, weights)
    unsaturated = float((v.abs().amax(dim=1) < 0.999).double().mean())
    print('%s %s: %d rows, largest activation %.1f, %.0f %% of the rows with unsaturated v' % (tag, weights, len(v), top, 100 * unsaturated))
    assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all())
    assert top <= MAX_ACTIVATION
    assert unsaturated >= MIN_UNSATURATED


@pytest.mark.parametrize('tag', TAGS)
def test_masks_of_finished_games_and_single_actions(tag):
    """d. at least one row has an empty real mask or a finished game; rows with exactly one valid action: the real ones are counted, the
    edited row is always there"""
    _, m, meta = R.batch(tag)
    plain = meta['edit'] == ''
    n_valid = m.sum(dim=1).numpy()
    empty, over, single = int((n_valid[plain] == 0).sum()), int(meta['ended'][plain].sum()), int((n_valid[plain] == 1).sum())
    print('%s: %d rows with an empty mask, %d of finished games, %d with exactly one valid action (%s)'
          % (tag, empty, over, single, 'real masks' if single else 'only the edited row'))
    assert empty + over >= 1
    assert int((n_valid == 1).sum()) >= 1 and int((n_valid[~plain] == 0).sum()) == 1


@pytest.mark.parametrize('tag', TAGS)
def test_shipped_module_reproduces_the_reference_vectors(tag):
    """e. the shipped weights in the float64 module, on the rows of netfwd_<tag>.npz, give netfwd64_<tag>.npz within 1e-9"""
    b, m = nw.raw_boards(tag, len(nw._fixture(tag)[0]))
    d = np.load(os.path.join(R.GOLDEN, 'netfwd64_%s.npz' % tag))
    pi, v = nw.float64_outputs(R.module(tag, 'shipped'), b, m)
    dp, dv = float((pi - torch.from_numpy(d['pi64'])).abs().max()), float((v - torch.from_numpy(d['v64'])).abs().max())
    print('%s: shipped module vs netfwd64: pi %.1e, v %.1e' % (tag, dp, dv))
    assert dp <= 1e-9 and dv <= 1e-9


@pytest.mark.parametrize('tag,weights', [c for c in CASES if c[0].startswith('akropolis')])
def test_akropolis_edited_codes_change_the_output(tag, weights):
    """the eight rows with description codes overwritten by -128, -1, 12 and 127 (the reference clamps to 0..11) differ from the rows
    they were copied from, in the float64 output, by far more than the GPU test's bound"""
    b, m, meta = R.batch(tag)
    pi, v, _ = _outputs(tag, weights)
    rows = np.flatnonzero(np.char.startswith(meta['edit'], 'codes'))
    assert len(rows) == R.EDIT_ROWS and sorted({int(e.split()[1]) for e in meta['edit'][rows]}) == sorted(R.CODE_EDITS)
    for i in rows:
        s = int(meta['source'][i])
        assert torch.equal(m[i], m[s]) and not torch.equal(b[i], b[s])
        moved = max(float((pi[i] - pi[s]).abs().max()), float((v[i] - v[s]).abs().max()))
        print('%s %s: %s moves the output by %.2e' % (tag, weights, R.name(meta, i), moved))
        assert moved >= 100 * nw.CONTRACT
