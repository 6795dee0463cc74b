"""CPU: the rows of tests/envcover.py for the games whose step always draws (Botanik, Minivilles 2-4p, The Little Prince 3-5p: whole
oracle games on a counter stream per game, every selected row re-evaluated on the stream it has in a launch of the env kernels) and for
Abalone games won by six marbles (rows_six) -- how much they cover, proved on the oracle alone; that random_seed changes nothing for
the first family; the oracle against the committed reference answers (tests/golden/envcover_<variant>.npz, envcover_<set-up>_six.npz,
tools/gen_golden_envcover.py); and, where the reference tree is present, the oracle against the LIVE reference on every selected row,
bit for bit, uniforms consumed included.  The GPU kernels meet the same rows in tests/test_gpu_env_coverage_drawing.py."""
import os
import sys

import numpy as np
import pytest

import envcover as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('AZG_REFERENCE', '/root/reference')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

BOTANIK_TAKEN, BOTANIK_VALID = 292, 348                      # what the plain rule (no lookahead) reaches in 1600 games
# distinct (action id, uniforms the step consumed) pairs: Minivilles' 21 ids with 0..6 uniforms, The Little Prince's refill ids twice
PAIRS = {'minivilles2': 104, 'minivilles3': 104, 'minivilles4': 104, 'tlp3': 12, 'tlp4': 20, 'tlp5': 30}
# rows that end the game AFTER the re-evaluation on the batch's streams (Minivilles' dice decide the end; the others' draws do not)
MIN_TERMINAL = {'botanik': 400, 'minivilles2': 200, 'minivilles3': 200, 'minivilles4': 200, 'tlp3': 400, 'tlp4': 400, 'tlp5': 400}
SIX_WINS, SIX_WINS_EACH, SIX_EJECTING = 8, 2, 130
# rows of group 4 that the live comparison keeps where the pure-Python reference is too slow for all of them; groups 1-3 are always
# whole.  Nothing is thinned: Botanik, the slowest, takes 20 s for its 16384 rows.
LIVE_SPACED = {}
COMPARED = ('valid', 'next_state', 'next_player', 'ended', 'score', 'round', 'canonical')
DRAWN = COMPARED + ('n_uniforms', 'counter_after')
_taken = {}


def selected(variant):
    """(rows, idx, group, take(rows, idx)) of a DRAWING variant, evaluated once"""
    if variant not in _taken:
        r = E.rows(variant)
        idx, group = E.select(r)
        _taken[variant] = (r, idx, group, E.take(r, idx))
    return _taken[variant]


def selected_six(variant):
    if (variant, 6) not in _taken:
        r = E.rows_six(variant)
        idx, group = E.select_six(r)
        _taken[variant, 6] = (r, idx, group, E.take(r, idx))
    return _taken[variant, 6]


def patterns(ended):
    return set(map(tuple, ended[ended.any(axis=1)].tolist()))


def test_the_tables_are_the_ones_meant():
    assert list(E.DRAWING) == ['botanik', 'minivilles2', 'minivilles3', 'minivilles4', 'tlp3', 'tlp4', 'tlp5']
    assert not set(E.DRAWING) & set(E.VARIANTS) and set(PAIRS) | {'botanik'} == set(E.DRAWING) == set(MIN_TERMINAL)
    for v in E.DRAWING:
        assert os.path.exists(os.path.join(GOLDEN, E.fixture_name(v)))
    assert set(E.SIX_GAMES) == {v for v, (name, _) in E.VARIANTS.items() if name == 'ABALONE'} and len(E.SIX_GAMES) == 5
    assert E.COVER_SEED != E.INIT_SEED and E.COVER_SEED not in E.MAGIC_SEEDS


@pytest.mark.parametrize('variant', list(E.DRAWING))
def test_floors_on_the_oracle(variant):
    r, idx, group, sel = selected(variant)
    n, A = len(r['action']), r['A']
    assert len(idx) == len(group) <= 16384 and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n
    assert (np.diff(group) >= 0).all() and all((np.diff(idx[group == k]) > 0).all() for k in (1, 2, 3, 4))
    assert len(idx) == min(n, 16384)
    assert r['seed'].min() > 0 and set(np.unique(r['seed']).tolist()) <= set(E.MAGIC_SEEDS)
    # one stream per game, continued from getInitBoard on: a row starts where the row before it stopped
    same = r['game'][1:] == r['game'][:-1]
    assert np.array_equal(r['counter'][1:][same], (r['counter'] + r['n_uniforms'])[:-1][same]) and (r['counter'][r['ply'] == 0] > 0).all()
    assert np.array_equal(sel['counter'], r['counter'][idx]) and np.array_equal(sel['counter_after'], sel['counter'] + sel['n_uniforms'])
    taken, valid, _ = E.counts(r, idx)
    games = int(r['game'].max()) + 1
    key = r['action'].astype(np.int64) * 256 + r['n_uniforms']
    pairs = len(np.unique(key[idx]))
    terminal = int(sel['ended'].any(axis=1).sum())
    ties = int(((sel['ended'] == np.float32(0.01)).sum(axis=1) >= 2).sum())
    old = np.load(os.path.join(GOLDEN, E.fixture_name(variant)))
    print('%s: %d games, %d rows, %d selected: ids taken %d, ids valid %d of %d, (id, uniforms) pairs %d, terminal rows as played %d, '
          're-evaluated %d, result patterns %d, rows with two players at 0.01: %d'
          % (variant, games, n, len(idx), taken, valid, A, pairs, int(r['ended'][idx].any(axis=1).sum()), terminal, len(patterns(sel['ended'])), ties))
    # nothing the whole run reached is lost by the selection, and groups 1-2 alone carry ids and pairs
    head = idx[group <= 2]
    assert E.counts(r, head)[:2] == E.counts(r)[:2] == (taken, valid)
    assert len(np.unique(key[idx[group == 1]])) == len(np.unique(key)) == pairs
    assert E.unpack(r['valid'][idx], A)[np.arange(len(idx)), r['action'][idx]].all()
    missing = np.setdiff1d(np.unique(old['action']), r['action'][idx])
    assert len(missing) == 0, (variant, missing.tolist())
    assert terminal >= MIN_TERMINAL[variant], (variant, terminal)
    assert terminal > int(old['ended'].any(axis=1).sum())
    if variant == 'botanik':
        plain = E.rows_drawing(variant, games=games, lookahead=False)
        p_taken, p_valid, _ = E.counts(plain)
        ever = E.unpack(r['valid'], A).any(axis=0)
        print('botanik: the plain rule in %d games: ids taken %d, ids valid %d; ids never valid: %s; valid but never taken: %s'
              % (games, p_taken, p_valid, np.flatnonzero(~ever).tolist(), np.setdiff1d(np.flatnonzero(ever), r['action']).tolist()))
        assert taken >= BOTANIK_TAKEN and valid >= BOTANIK_VALID, (taken, valid)
        assert taken >= p_taken and valid >= p_valid, (taken, p_taken, valid, p_valid)
        assert games <= 1600 and 'state' not in r
        # the 14 ids no game can reach are never valid
        assert not ever[[75, 102, 103, 104, 105, 106, 108, 271, 298, 299, 300, 301, 302, 304]].any()
    else:
        assert taken == A, (variant, taken)
        assert pairs >= PAIRS[variant], (variant, pairs)
        assert patterns(old['ended']) <= patterns(sel['ended']), (variant, patterns(old['ended']) - patterns(sel['ended']))
        assert ties >= 1, variant


def test_botanik_states_are_the_replayed_ones():
    """Botanik's run keeps no states: states() plays the games of the asked rows again.  Against a run small enough to check by hand."""
    og = E.oracle_game('botanik')
    r = E.rows_drawing('botanik', games=3)
    n = len(r['action'])
    st = E.states(r, np.arange(n)[::-1])[::-1]
    assert np.array_equal(st[r['ply'] == 0], np.stack([og.getInitBoard(og.rng(seed=E.INIT_SEED, stream=g)).reshape(-1) for g in range(3)]))
    for i in range(n):
        assert np.array_equal(np.packbits(og.getValidMoves(st[i].reshape(og.shape), int(r['player'][i]))), r['valid'][i]), i
        if i + 1 < n and r['game'][i + 1] == r['game'][i]:
            rng = og.rng(seed=E.INIT_SEED, stream=int(r['game'][i]))
            rng.counter = int(r['counter'][i])
            nb, npl = og.getNextState(st[i].reshape(og.shape), int(r['player'][i]), int(r['action'][i]), 0, rng)
            assert np.array_equal(nb.reshape(-1), st[i + 1]) and npl == r['player'][i + 1] and rng.counter == r['counter'][i + 1], i
    assert np.array_equal(E.states(r, np.array([5, n - 1, 0])), st[[5, n - 1, 0]])


@pytest.mark.parametrize('variant', list(E.DRAWING))
def test_the_seed_does_not_matter(variant):
    """the step of these games draws from the stream it is given whatever random_seed says: 0 (the stream, for every other game) and
    31416 (a seeded draw, for every other game) give the same bytes on the same (stream, counter), and those are the selected rows'"""
    _, idx, _, sel = selected(variant)
    a, b = E.oracle_outputs_drawing(variant, sel, seed=0), E.oracle_outputs_drawing(variant, sel, seed=31416)
    for k in DRAWN:
        E.check_equal(variant, 'random_seed 0 vs 31416, %s' % k, a[k], b[k], sel['action'], idx)
        E.check_equal(variant, 'random_seed 0 vs the recorded seed, %s' % k, a[k], sel[k], sel['action'], idx)
    # steps that draw and (Minivilles rolls at least one die in every step) steps that do not
    assert sel['n_uniforms'].max() > 1 and sel['n_uniforms'].min() == (1 if variant.startswith('minivilles') else 0)


@pytest.mark.parametrize('variant', list(E.SIX_GAMES))
def test_floors_of_the_games_won_by_six(variant):
    r, idx, group, sel = selected_six(variant)
    n = len(r['action'])
    assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n and len(idx) <= 16384
    assert (np.diff(group) >= 0).all() and all((np.diff(idx[group == k]) > 0).all() for k in (1, 2, 3))
    last = np.flatnonzero(np.append(r['game'][1:] != r['game'][:-1], True))
    score = E.scores_after(r)
    assert r['ended'][last].any(axis=1).all() and not r['ended'][np.setdiff1d(np.arange(n), last)].any()
    six = [int((score[last, p] == 6).sum()) for p in (0, 1)]
    ejecting = np.unique(r['action'][r['eject']])
    print('%s: %d games, %d rows, %d selected (%s by group): won by six %d + %d, distinct ejecting ids %d, rows with a score of 5 / 6 after: %d / %d'
          % (variant, len(last), n, len(idx), [int((group == k).sum()) for k in (1, 2, 3)], six[0], six[1], len(ejecting),
             int((score == 5).any(axis=1).sum()), int((score == 6).any(axis=1).sum())))
    assert sum(six) >= SIX_WINS and min(six) >= SIX_WINS_EACH, (variant, six)
    assert len(ejecting) >= SIX_EJECTING, (variant, len(ejecting))
    # the selection holds every ejecting id on a row that ejects, every row with a 5 or a 6 after it, every last transition
    assert np.array_equal(np.unique(r['action'][idx[group == 1]]), ejecting) and r['eject'][idx[group == 1]].all()
    assert np.isin(np.flatnonzero((score >= 5).any(axis=1)), idx).all() and np.isin(last, idx).all()
    assert np.array_equal(sel['score'], score[idx].astype(np.int16))
    # a win by six is what game_ended says of it, for either player, and the scores never pass 6
    won = sel['score'].max(axis=1) == 6
    assert score.max() == 6 and won.sum() >= sum(six)
    assert np.array_equal(sel['ended'][won], np.where(sel['score'][won] == 6, 1.0, -1.0).astype(np.float32))
    assert E.unpack(r['valid'][idx], r['A'])[np.arange(len(idx)), r['action'][idx]].all()


def committed(name, r, idx, group):
    """the committed file of a selection: it is the head of the selection order and says how many rows it leaves off"""
    path = os.path.join(GOLDEN, 'envcover_%s.npz' % name)
    assert os.path.getsize(path) <= 1000000
    d = dict(np.load(path))
    n = len(d['action'])
    keep = group <= 3
    assert n > 0 and int(d['dropped']) == keep.sum() - n
    assert np.array_equal(d['row'], idx[keep][:n]) and np.array_equal(d['group'], group[keep][:n])
    return d


@pytest.mark.parametrize('variant', list(E.DRAWING))
def test_oracle_reproduces_the_committed_reference_rows(variant):
    r, idx, group, sel = selected(variant)
    d = committed(variant, r, idx, group)
    n = len(d['action'])
    for k in ('state', 'action', 'seed', 'player', 'counter'):
        assert np.array_equal(d[k], sel[k][:n]), k
    assert int(d['dropped']) == 0                              # (every covering and every final row travels with the repository)
    got = E.oracle_outputs_drawing(variant, d)
    for k in DRAWN:
        assert got[k].dtype == d[k].dtype, (k, got[k].dtype, d[k].dtype)
        E.check_equal(variant, 'oracle vs envcover_%s.npz, %s' % (variant, k), got[k], d[k], d['action'], d['row'])


@pytest.mark.parametrize('variant', list(E.SIX_GAMES))
def test_oracle_reproduces_the_committed_reference_rows_won_by_six(variant):
    r, idx, group, sel = selected_six(variant)
    d = committed(variant + '_six', r, idx, group)
    n = len(d['action'])
    for k in ('state', 'action', 'seed', 'player'):
        assert np.array_equal(d[k], sel[k][:n]), k
    assert int(d['dropped']) == 0 and (d['score'] == 6).any(axis=0).all() and (d['score'] == 5).any(axis=0).all()
    got = E.oracle_outputs(variant, d)
    for k in COMPARED:
        assert got[k].dtype == d[k].dtype, (k, got[k].dtype, d[k].dtype)
        E.check_equal(variant, 'oracle vs envcover_%s_six.npz, %s' % (variant, k), got[k], d[k], d['action'], d['row'])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference tree is not on this machine')
@pytest.mark.parametrize('variant', list(E.DRAWING))
def test_oracle_equals_live_reference_on_every_selected_row(variant):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_golden_envcover as T
    r = E.rows(variant)
    idx, group = E.select(r, spaced=LIVE_SPACED.get(variant))
    assert (group <= 3).sum() == (E.select(r)[1] <= 3).sum()
    sel = E.take(r, idx)                                       # (thinned: row j is re-evaluated on the stream of ITS position here)
    try:
        ref = T.ref_outputs_drawing(T.ref_game(variant), sel)
    finally:
        T.H.cleanup()
    for k in DRAWN:
        E.check_equal(variant, 'oracle vs live reference, %s' % k, sel[k], ref[k], sel['action'], idx)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference tree is not on this machine')
@pytest.mark.parametrize('variant', list(E.SIX_GAMES))
def test_oracle_equals_live_reference_on_the_games_won_by_six(variant):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_golden_envcover as T
    _, idx, _, sel = selected_six(variant)
    try:
        ref = T.ref_outputs(T.ref_game(variant), sel)
    finally:
        T.H.cleanup()
    for k in COMPARED:
        E.check_equal(variant, 'oracle vs live reference, won by six, %s' % k, sel[k], ref[k], sel['action'], idx)
