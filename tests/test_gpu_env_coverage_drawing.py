"""GPU: the env kernels (csrc/game_*.hip.h through azg_env_*) of the games whose step always draws -- Botanik, Minivilles 2-4p, The Little
Prince 3-5p -- on every action id a game reaches and on hundreds of final positions, and Abalone's on games won by six marbles.  The rows
are tests/envcover.py's (whole oracle games on a counter stream per game; row j of the selection re-evaluated by the oracle on the stream
(COVER_SEED, j) at the row's counter, which is the stream row j has in a launch with rng_seed = COVER_SEED, stream0 = 0); the expected
values are the oracle's, which tests/test_env_coverage_drawing.py holds to the live reference on the same rows, and the reference's own
on the committed head of the selection (tests/golden/envcover_<variant>.npz, envcover_<set-up>_six.npz).  Bit-exact: valid masks, next
state, next player and the counter after the step, game_ended / scores / round, canonical form, the launch tail (1, 63, 65 rows),
init_boards on 64 streams, and the symmetries with random parts (Botanik's 13-14 forms, The Little Prince's shuffles, Smallworld's
offsets) on cover and last-ply positions."""
import os

import numpy as np
import pytest

import envcover as E
import test_gpu_env_coverage as C

pytestmark = pytest.mark.gpu

OUTPUTS = C.OUTPUTS + ('counter_after',)
SYM_SEED = 515
RANDOM_SYMMETRIES = ('tlp3', 'tlp4', 'tlp5', 'smallworld', 'smallworld3', 'smallworld4')


def make_game(variant):
    from azg_amd import games
    if variant == 'botanik':
        return games.BotanikGame(rng_seed=E.COVER_SEED)
    n = int(variant[-1])
    return (games.MinivillesGame if variant.startswith('minivilles') else games.TLPGame)(n, rng_seed=E.COVER_SEED)


def kernel_outputs(g, d, n=None):
    """C.kernel_outputs for the games that always draw: row j steps on the stream (g.rng_seed, 0 + j) from d['counter'][j]; also the
    counters the launch left"""
    import torch
    dev = g.device
    n = len(d['action']) if n is None else n

    def t(k, dt):
        return torch.from_numpy(np.ascontiguousarray(d[k][:n].astype(dt))).to(dev)
    st, pl, act, seeds = t('state', np.int8), t('player', np.int32), t('action', np.int32), t('seed', np.int64)
    ns, npl, counters = t('next_state', np.int8), t('next_player', np.int32), t('counter', np.int64)
    valid = g.valid_moves_batch(st, pl)
    nxt, nxt_pl = g.next_state_batch(st, pl, act, seeds, stream0=0, counters=counters)
    ended, score, rnd = g.game_ended_batch(ns, npl)
    canon = g.canonical_batch(ns, npl)
    torch.cuda.synchronize()
    return dict(valid=np.packbits(valid.cpu().numpy(), axis=1), next_state=nxt.cpu().numpy(), next_player=nxt_pl.cpu().numpy().astype(np.int8),
                ended=ended.cpu().numpy(), score=score.cpu().numpy().astype(np.int16), round=rnd.cpu().numpy().astype(np.int16),
                canonical=canon.cpu().numpy(), counter_after=counters.cpu().numpy())


def compare(variant, what, got, exp, actions, rows_idx):
    for k in OUTPUTS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k][:len(got[k])].shape, (variant, what, k, got[k].dtype, got[k].shape)
        E.check_equal(variant, '%s, %s' % (what, k), got[k], exp[k][:len(got[k])], actions, rows_idx)


def sym_positions(pool, last, must=()):
    """256 rows: 128 spread over `pool` (those of `must` first), 128 spread over `last`"""
    must = np.asarray(must, dtype=np.int64)[:32]
    cover = np.concatenate([must, pool[np.linspace(0, len(pool) - 1, 128 - len(must)).astype(np.int64)]])
    return np.concatenate([cover, last[np.linspace(0, len(last) - 1, 128).astype(np.int64)]])


def symmetries(variant, g, og, states, players, where, masked_pi, seed=None):
    """symmetries_batch vs og.getSymmetries on the canonical forms of (states, players); seed: position t draws from the stream
    (seed, 7 + t) in both.  -> the number of forms of each position"""
    import torch
    K = g.max_symmetries()
    can = np.stack([og.getCanonicalForm(s.reshape(og.shape), int(p)).reshape(-1) for s, p in zip(states, players)])
    vas = np.stack([og.getValidMoves(s.reshape(og.shape), 0) for s in can]).astype(np.uint8)
    vas[~vas.any(axis=1)] = 1
    pis = np.random.default_rng(3).random(vas.shape).astype(np.float32) * (vas if masked_pi else 1)
    dev = g.device
    kw = {} if seed is None else dict(rng_seed=seed, stream0=7)
    ob, op, ov, cnt = g.symmetries_batch(torch.from_numpy(can).to(dev), torch.from_numpy(pis).to(dev), torch.from_numpy(vas).to(dev), **kw)
    ob, op, ov, cnt = ob.cpu().numpy(), op.cpu().numpy(), ov.cpu().numpy(), cnt.cpu().numpy()
    for j in range(len(can)):
        rng = None if seed is None else og.rng(seed=seed, stream=7 + j)
        syms = og.getSymmetries(can[j].reshape(og.shape), pis[j], vas[j], max_sym=K, rng=rng)
        at = '%s symmetries: position %d (%s)' % (variant, j, where[j])
        assert len(syms) == int(cnt[j]), (at, len(syms), int(cnt[j]))
        for k, (s, p_, v_) in enumerate(syms):
            for what, got, exp in (('board', ob[j, k], s.reshape(-1)), ('pi', op[j, k], p_), ('valids', ov[j, k], v_.astype(np.uint8))):
                if not np.array_equal(got, exp):
                    b = int(np.flatnonzero(got != exp)[0])
                    raise AssertionError('%s, form %d, %s: first differing element %d: got %r, expected %r' % (at, k, what, b, got[b], exp[b]))
    return cnt


@pytest.mark.parametrize('variant', list(E.DRAWING))
def test_env_kernels_of_the_games_that_always_draw(golden_dir, variant):
    import torch
    g, og = make_game(variant), E.oracle_game(variant)
    assert (g.S, g.A, g.P) == (og.S, og.A, og.P) and g.rng_seed == E.COVER_SEED
    r = E.rows(variant)
    idx, group = E.select(r)
    sel = E.take(r, idx)
    assert len(idx) <= 16384
    # 1. the whole selection against the oracle
    full = kernel_outputs(g, sel)
    compare(variant, 'kernels vs oracle rows', full, sel, sel['action'], idx)
    assert (full['counter_after'] > sel['counter']).any()
    # 2. the launch tail: the first n rows alone give what they gave inside the full batch
    for n in C.TAILS:
        compare(variant, 'first %d rows alone vs the same rows of the full batch' % n, kernel_outputs(g, sel, n), full, sel['action'], idx)
    # 3. the reference's own answers on the committed head of the selection (row j of the file is row j of the selection: same stream)
    d = dict(np.load(os.path.join(golden_dir, 'envcover_%s.npz' % variant)))
    assert len(d['action']) > 0 and np.array_equal(d['row'], idx[:len(d['row'])]) and np.array_equal(d['state'], sel['state'][:len(d['row'])])
    compare(variant, 'kernels vs envcover_%s.npz' % variant, kernel_outputs(g, d), d, d['action'], d['row'])
    # 4. init_game on 64 streams
    counters = torch.zeros(64, dtype=torch.int64, device=g.device)
    boards = g.init_boards_batch(64, stream0=0, counters=counters).cpu().numpy()
    rngs = [og.rng(seed=E.COVER_SEED, stream=t) for t in range(64)]
    exp = np.stack([og.getInitBoard(x).reshape(-1) for x in rngs])
    E.check_equal(variant, 'init_boards_batch vs getInitBoard', boards, exp, np.zeros(64, dtype=np.int64))
    assert np.array_equal(counters.cpu().numpy(), np.array([x.counter for x in rngs], dtype=np.int64)) and counters.min() > 0


@pytest.mark.parametrize('variant', list(E.SIX_GAMES))
def test_abalone_kernels_on_games_won_by_six(golden_dir, variant):
    g = C.make_game(variant)
    r = E.rows_six(variant)
    idx, _ = E.select_six(r)
    sel = E.take(r, idx)
    assert (sel['score'] == 6).any(axis=0).all() and (sel['ended'][sel['score'].max(axis=1) == 6] != 0).all()
    C.compare(variant, 'kernels vs oracle rows won by six', C.kernel_outputs(g, sel), sel, sel['action'], idx)
    d = dict(np.load(os.path.join(golden_dir, 'envcover_%s_six.npz' % variant)))
    assert len(d['action']) > 0 and np.array_equal(d['row'], idx[:len(d['row'])]) and np.array_equal(d['state'], sel['state'][:len(d['row'])])
    C.compare(variant, 'kernels vs envcover_%s_six.npz' % variant, C.kernel_outputs(g, d), d, d['action'], d['row'])


def test_botanik_symmetries_on_cover_and_last_ply_positions():
    """13 forms, 14 where both freed cards of the player to move are there (the reference has no position with fewer: the identity,
    two mirrors, three arrival and five register permutations and two colour rolls are unconditional)"""
    g, og = make_game('botanik'), E.oracle_game('botanik')
    r = E.rows('botanik')
    idx, group = E.select(r)
    sel = E.take(r, idx)
    own = 7 * (25 + 2 * sel['player'].astype(np.int64))         # colour byte of the mover's first freed card; the second is 7 further
    both = np.flatnonzero((sel['state'][np.arange(len(idx)), own] != 0) & (sel['state'][np.arange(len(idx)), own + 7] != 0))
    pos = sym_positions(np.flatnonzero(group <= 2), np.flatnonzero(r['ended'][idx].any(axis=1)), must=both)
    where = ['row %d of rows(), action %d' % (idx[i], sel['action'][i]) for i in pos]
    cnt = symmetries('botanik', g, og, sel['state'][pos], sel['player'][pos], where, masked_pi=False)
    assert len(cnt) == 256 and set(cnt.tolist()) == {13, 14}, sorted(set(cnt.tolist()))


@pytest.mark.parametrize('variant', RANDOM_SYMMETRIES)
def test_random_symmetries_on_cover_and_last_ply_positions(variant):
    drawing = variant in E.DRAWING
    g, og = (make_game(variant) if drawing else C.make_game(variant)), E.oracle_game(variant)
    r = E.rows(variant)
    idx, group = E.select(r)
    head = idx[group <= 2]
    pos = sym_positions(head if len(head) >= 128 else idx, np.flatnonzero(r['ended'].any(axis=1)))
    where = ['row %d of rows(), action %d' % (i, r['action'][i]) for i in pos]
    cnt = symmetries(variant, g, og, r['state'][pos], r['player'][pos], where, masked_pi=drawing, seed=SYM_SEED)
    assert len(cnt) == 256 and cnt.min() >= 1 and cnt.max() > 1
