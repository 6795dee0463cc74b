"""CPU: the rows of tests/envcover.py (oracle games steered towards every reachable action id) -- how much they cover, proved on the oracle
alone; the oracle against the committed reference answers for them (tests/golden/envcover_*.npz, tools/gen_golden_envcover.py); and,
where the reference tree is present, the oracle against the LIVE reference on every selected row, bit for bit.  The GPU kernels meet the
same rows in tests/test_gpu_env_coverage.py."""
import os
import sys

import numpy as np
import pytest

import envcover as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('AZG_REFERENCE', '/root/reference')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# distinct action ids the selected rows must take: the saturation value of the recipe where there is one (more games reach no more), a
# little under the measured count for Akropolis and Smallworld, whose counts move with the recipe (DESIGN.md §5 has the counts reached)
FLOORS = {'santorini11': 834, 'santorini1': 128, 'abalone': 1734, 'abalone_classic': 1734, 'abalone_german': 1734,
          'abalone_classic_komi': 1734, 'abalone_belgian_komi': 1734, 'splendor2': 81, 'splendor3': 81, 'splendor4': 81, 'azul': 180,
          'smallworld': 120, 'smallworld3': 120, 'smallworld4': 198, 'akropolis': 2000, 'akropolis3': 2000, 'akropolis4': 2600}
MIN_TERMINAL = 200
# rows of group 4 (the evenly spaced rest) that the live comparison keeps, where the reference is too slow for all of them in a minute;
# groups 1-3 are always whole
LIVE_SPACED = {}
COMPARED = ('valid', 'next_state', 'next_player', 'ended', 'score', 'round', 'canonical')


def test_the_variants_and_seeds_are_the_ones_meant():
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'refshim'))
    import harness as H
    import test_gpu_env
    import test_gpu_abalone_variants
    assert tuple(H.MAGIC_SEEDS) == E.MAGIC_SEEDS
    assert list(E.VARIANTS)[:13] == list(test_gpu_env.VARIANTS) and list(E.VARIANTS)[13:] == list(test_gpu_abalone_variants.CONFIGS)
    assert set(FLOORS) == set(E.VARIANTS)
    for v, (name, var) in E.VARIANTS.items():
        if v in test_gpu_abalone_variants.CONFIGS:
            assert var == test_gpu_abalone_variants.CONFIGS[v]
        assert os.path.exists(os.path.join(GOLDEN, E.fixture_name(v)))


@pytest.mark.parametrize('variant', list(E.VARIANTS))
def test_floors_on_the_oracle(variant):
    r = E.rows(variant)
    idx, group = E.select(r)
    n, A = len(r['action']), r['A']
    assert len(idx) == len(group) <= 16384 and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n
    assert (np.diff(group) >= 0).all() and all((np.diff(idx[group == k]) > 0).all() for k in (1, 2, 3, 4))
    assert len(idx) == min(n, 16384)                                           # group 4 fills the cap
    assert r['seed'].min() > 0 and set(np.unique(r['seed']).tolist()) <= set(E.MAGIC_SEEDS)
    taken, valid, terminal = E.counts(r, idx)
    print('%s: %d games, %d rows, %d selected: ids taken %d, ids valid %d of %d, terminal rows %d' % (variant, r['game'].max() + 1, n, len(idx), taken, valid, A, terminal))
    assert taken >= FLOORS[variant], (variant, taken)
    assert terminal >= MIN_TERMINAL, (variant, terminal)
    # nothing the whole run reached is lost by the selection, and groups 1-2 alone carry it
    head = idx[group <= 2]
    assert E.counts(r, head)[:2] == E.counts(r)[:2] == (taken, valid)
    assert np.array_equal(np.sort(idx[group == 3]), np.setdiff1d(np.flatnonzero(r['ended'].any(axis=1)), head))
    # every action really was valid where it was taken
    m = E.unpack(r['valid'][idx], A)
    assert m[np.arange(len(idx)), r['action'][idx]].all()
    # what the old fixture takes is taken here
    old = np.load(os.path.join(GOLDEN, E.fixture_name(variant)))
    missing = np.setdiff1d(np.unique(old['action']), r['action'][idx])
    assert len(missing) == 0, (variant, missing.tolist())
    assert taken > len(np.unique(old['action'])) or taken == A
    assert terminal > int(old['ended'].any(axis=1).sum())


def test_select_equals_the_row_by_row_pass():
    """select() finds group 2 with one vectorised pass; the definition is sequential (a row is selected when an id is valid in it that is
    valid in no row selected before).  Both on a run small enough for the plain loop."""
    r = E.rows('akropolis', games=12)
    idx, group = E.select(r)
    A = r['A']
    m = E.unpack(r['valid'], A).astype(bool)
    g1 = idx[group == 1]
    seen = m[g1].any(axis=0)
    g2 = []
    for i in range(len(m)):
        if i not in set(g1.tolist()) and (m[i] & ~seen).any():
            g2.append(i)
            seen |= m[i]
    assert g2 == idx[group == 2].tolist() and len(g2) > 0
    assert np.array_equal(np.sort(np.unique(r['action'], return_index=True)[1]), g1)
    assert len(idx) == len(m) and np.array_equal(np.sort(idx), np.arange(len(m)))           # under the cap every row is selected
    head = int((group <= 3).sum())
    assert len(m) - head > 10
    few, gfew = E.select(r, cap=head + 5)                                                   # the cap cuts group 4 alone, evenly
    assert len(few) == head + 5 and np.array_equal(few[:head], idx[:head]) and (gfew[head:] == 4).all()
    rest = idx[head:]
    assert few[head] == rest[0] and few[-1] == rest[-1]


@pytest.mark.parametrize('variant', list(E.VARIANTS))
def test_oracle_reproduces_the_committed_reference_rows(variant):
    path = os.path.join(GOLDEN, 'envcover_%s.npz' % variant)
    assert os.path.getsize(path) <= 1000000
    d = dict(np.load(path))
    r = E.rows(variant)
    idx, group = E.select(r)
    n = len(d['action'])
    keep = group <= 3
    assert n > 0 and int(d['dropped']) == keep.sum() - n                      # the file is the head of the selection, group by group
    assert np.array_equal(d['row'], idx[keep][:n]) and np.array_equal(d['group'], group[keep][:n])
    assert np.array_equal(d['state'], r['state'][d['row']]) and np.array_equal(d['action'], r['action'][d['row']])
    assert np.array_equal(d['seed'], r['seed'][d['row']]) and np.array_equal(d['player'], r['player'][d['row']])
    got = E.oracle_outputs(variant, d)
    for k in COMPARED:
        assert got[k].dtype == d[k].dtype, (k, got[k].dtype, d[k].dtype)
        E.check_equal(variant, 'oracle vs envcover_%s.npz, %s' % (variant, k), got[k], d[k], d['action'], d['row'])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference tree is not on this machine')
@pytest.mark.parametrize('variant', list(E.VARIANTS))
def test_oracle_equals_live_reference_on_every_selected_row(variant):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_golden_envcover as T
    r = E.rows(variant)
    idx, group = E.select(r, spaced=LIVE_SPACED.get(variant))
    assert (group <= 3).sum() == (E.select(r)[1] <= 3).sum()
    sel = E.take(r, idx)
    try:
        ref = T.ref_outputs(T.ref_game(variant), sel)
    finally:
        T.H.cleanup()
    for k in COMPARED:
        E.check_equal(variant, 'oracle vs live reference, %s' % k, sel[k], ref[k], sel['action'], idx)
