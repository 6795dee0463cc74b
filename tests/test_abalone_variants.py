"""Abalone's starting layouts and dynamic komi without a GPU: the C-ABI's variant word (azg_game_info), games.AbaloneGame's arguments and their
encoding, the conditions the fixtures of tools/gen_golden_abalone_variants.py must meet, the plain-torch net on the two other shipped
checkpoints, and one live look at the reference's init_game per layout."""
import os

import numpy as np
import pytest
import torch

from test_nnet import assert_net_close

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
CONFIGS = {'abalone_classic': ('classic', False), 'abalone_german': ('german', False), 'abalone_classic_komi': ('classic', True),
           'abalone_belgian_komi': ('belgian', True)}


def test_game_info_accepts_the_variant_word_and_nothing_else():
    from azg_amd import _lib
    for v in range(8):                       # layout 0 = the default (Belgian Daisy), with and without komi
        assert _lib.game_info(_lib.ABALONE, v)[:3] == (324, 3402, 2), v
    for v in (8, 9, 12, 16, 99, -1, -4, 1 << 20):
        with pytest.raises(_lib.AzgError, match='unsupported game/variant'):
            _lib.game_info(_lib.ABALONE, v)


def test_variant_encoding_and_argument_validation():
    from azg_amd import games
    enc = games.abalone_variant
    assert enc() == ('belgian', False, 1)
    assert [enc(l)[2] for l in ('classic', 'belgian', 'german')] == [3, 1, 2]
    assert [enc(l)[:2] for l in (0, 1, 2)] == [('classic', False), ('belgian', False), ('german', False)]      # the reference's INITIAL_LAYOUT
    assert [enc(l, True)[2] for l in ('classic', 'belgian', 'german')] == [7, 5, 6]
    assert enc(np.int64(2), np.bool_(True)) == ('german', True, 6) and enc('German')[0] == 'german'
    for bad in ('daisy', 3, -1, None, 1.0, True):
        with pytest.raises(ValueError):
            enc(bad)
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError):
            enc('classic', bad)
    # the constructor validates before it asks for a GPU
    with pytest.raises(ValueError):
        games.AbaloneGame(layout='daisy')
    with pytest.raises(ValueError):
        games.import_game('abalone', layout='classic', dynamic_komi=2)
    if torch.cuda.is_available():
        g = games.import_game('abalone', layout=0, dynamic_komi=True)
        assert (g.layout, g.dynamic_komi, g.variant) == ('classic', True, 7)
        g = games.AbaloneGame()
        assert (g.layout, g.dynamic_komi, g.variant) == ('belgian', False, 1)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_fixture_conditions(config):
    layout, komi = CONFIGS[config]
    d = np.load(os.path.join(ROOT, 'env_%s.npz' % config))
    assert 300 <= len(d['state']) and os.path.getsize(os.path.join(ROOT, 'env_%s.npz' % config)) < 256 * 1024
    tie = (d['round'] >= 127) & (d['score'][:, 0] == d['score'][:, 1]) & (d['score'].max(axis=1) < 6)
    ends = d['ended'][tie]
    bits = d['state'].reshape(-1, 81, 4)[:, 3, 3]
    if komi:
        assert not np.isclose(d['ended'], 0.001).any()
        assert (ends == np.float32([1, -1])).all(axis=1).any() and (ends == np.float32([-1, 1])).all(axis=1).any()
        # the bit decided them: the recorded next_state is in absolute seats
        nb = d['next_state'].reshape(-1, 81, 4)[tie][:, 3, 3]
        assert np.array_equal(ends[:, 0], np.where(nb == 1, 1, -1).astype(np.float32))
        assert set(np.unique(bits)) == {0, 1}
    else:
        assert len(ends) >= 1 and np.isclose(ends, 0.001).all()
        assert not bits.any()
    # the layout: marbles of the first init board, 14 a side, in the rows of abalone/AbaloneLogicNumba.py:179-227
    b = d['init_boards'][0].reshape(9, 9, 4)
    rows = {'classic': ([6, 7, 8], [0, 1, 2]), 'belgian': ([0, 1, 2, 6, 7, 8], [0, 1, 2, 6, 7, 8]), 'german': ([1, 2, 3, 5, 6, 7], [1, 2, 3, 5, 6, 7])}[layout]
    for z in (0, 1):
        assert int(b[:, :, z].sum()) == 14 and sorted(set(np.nonzero(b[:, :, z])[0].tolist())) == rows[z]
    m = np.load(os.path.join(ROOT, 'mcts_%s_numba.npz' % config))
    assert set(m['case_sims'].tolist()) == {25, 200}
    if komi:
        late = m['case_round'] >= 124
        assert late.any() and (m['case_tied_terminals'][late] > 0).all()
        assert (m['case_root'].reshape(-1, 81, 4)[late][:, 0, 3] == m['case_root'].reshape(-1, 81, 4)[late][:, 1, 3]).all()


@pytest.mark.parametrize('tag', ['abalone_v21_german', 'abalone_v21_classic'])
def test_torch_net_on_the_other_shipped_checkpoints(tag):
    from azg_amd import nnet
    d = np.load(os.path.join(ROOT, 'netfwd_%s.npz' % tag))
    z = np.load(os.path.join(ROOT, 'weights_%s.npz' % tag))
    assert int(z['arg/nn_version']) == 21 and sum(k.startswith('sd/') for k in z.files) == 97
    net = nnet.AbaloneV21.from_npz(os.path.join(ROOT, 'weights_%s.npz' % tag), device='cpu')
    pi, v = net.predict_batch(torch.from_numpy(d['boards']).reshape(len(d['boards']), -1), torch.from_numpy(d['masks']))
    assert_net_close(pi, v, tag, d)
    if tag == 'abalone_v21_classic':           # boards with the komi bit set are among them
        assert d['boards'].reshape(-1, 81, 4)[:, 3, 3].any()


@pytest.mark.parametrize('config', list(CONFIGS))
def test_live_reference_init_game(config):
    """the reference itself, constants patched: its init_game gives the marble planes of the fixture, and a komi bit only with komi"""
    import sys
    tools = os.path.join(os.path.dirname(__file__), '..', 'tools', 'refshim')
    sys.path.insert(0, tools)
    try:
        import harness as H
    finally:
        sys.path.remove(tools)
    if not os.path.isdir(os.path.join(H.REFERENCE, 'abalone')):
        pytest.skip('the reference is not on this machine')
    layout, komi = CONFIGS[config]
    m = H.load_reference(abalone_layout=('classic', 'belgian', 'german').index(layout), abalone_dynamic_komi=komi)
    try:
        g = m['AbaloneGame'].AbaloneGame()
        want = np.load(os.path.join(ROOT, 'env_%s.npz' % config))['init_boards'][0].reshape(9, 9, 4)
        bits = set()
        for seed in range(8):
            np.random.seed(seed)
            b = g.getInitBoard()
            assert np.array_equal(b[:, :, :3], want[:, :, :3])
            bits.add(int(b[0, 3, 3]))
        assert bits == ({0, 1} if komi else {0})
    finally:
        H.cleanup()
