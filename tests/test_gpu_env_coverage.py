"""GPU: the env kernels (csrc/game_*.hip.h through azg_env_*) on every action id a game can reach.  The rows are whole oracle games steered
towards untaken action ids (tests/envcover.py: up to 16384 selected rows per variant -- a cover of every id taken, every id ever valid,
the last transition of every game, evenly spaced others); the expected values are the oracle's, which tests/test_env_coverage.py holds to
the live reference on the same rows, and the reference's own on the committed head of the selection (tests/golden/envcover_*.npz).
Bit-exact: valid masks, next state and player (seeded and, for the games that draw, random_seed == 0 on the counter stream), game_ended /
scores / round, canonical form, the launch tail (1, 63, 65 rows) and getSymmetries on cover and last-ply positions."""
import os

import numpy as np
import pytest

import envcover as E

pytestmark = pytest.mark.gpu

TAILS = (1, 63, 65)
# the variants of test_gpu_env.test_symmetries_vs_golden_and_oracle and the other Abalone set-ups (one rule set for the symmetries)
SYMMETRIES = ('splendor2', 'splendor3', 'splendor4', 'santorini1', 'santorini11', 'azul', 'abalone', 'akropolis', 'akropolis3', 'akropolis4',
              'abalone_classic', 'abalone_german', 'abalone_classic_komi', 'abalone_belgian_komi')
OUTPUTS = ('valid', 'next_state', 'next_player', 'ended', 'score', 'round', 'canonical')


def make_game(variant):
    import test_gpu_abalone_variants
    import test_gpu_env
    return test_gpu_env.make_game(variant) if variant in test_gpu_env.VARIANTS else test_gpu_abalone_variants.make(variant)


def kernel_outputs(g, d, n=None):
    """the four env kernels on the first n rows of d: valid_moves and next_state on (state, player[, action, seed]); game_ended and
    canonical on the RECORDED (next_state, next_player), so that one wrong step does not show up three times -> arrays typed like d's"""
    import torch
    dev = g.device
    n = len(d['action']) if n is None else n

    def t(k, dt):
        return torch.from_numpy(np.ascontiguousarray(d[k][:n].astype(dt))).to(dev)
    st, pl, act, seeds = t('state', np.int8), t('player', np.int32), t('action', np.int32), t('seed', np.int64)
    ns, npl = t('next_state', np.int8), t('next_player', np.int32)
    valid = g.valid_moves_batch(st, pl)
    nxt, nxt_pl = g.next_state_batch(st, pl, act, seeds)
    ended, score, rnd = g.game_ended_batch(ns, npl)
    canon = g.canonical_batch(ns, npl)
    torch.cuda.synchronize()
    return dict(valid=np.packbits(valid.cpu().numpy(), axis=1), next_state=nxt.cpu().numpy(), next_player=nxt_pl.cpu().numpy().astype(np.int8),
                ended=ended.cpu().numpy(), score=score.cpu().numpy().astype(np.int16), round=rnd.cpu().numpy().astype(np.int16),
                canonical=canon.cpu().numpy())


def compare(variant, what, got, exp, actions, rows_idx):
    """got == the first len(got) rows of exp, field by field; a failure names variant, row, action id and first differing byte"""
    for k in OUTPUTS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k][:len(got[k])].shape, (variant, what, k, got[k].dtype, got[k].shape)
        E.check_equal(variant, '%s, %s' % (what, k), got[k], exp[k][:len(got[k])], actions, rows_idx)


def true_random_steps(variant, g, og, d):
    """random_seed == 0 on the rows of d: the step draws from stream (rng_seed, stream0 + row) at the row's counter, like the oracle"""
    import torch
    n, dev = len(d['action']), g.device
    g.rng_seed = 1234
    counters = torch.arange(n, dtype=torch.int64, device=dev) * 3
    out, nxt = g.next_state_batch(torch.from_numpy(d['state']).to(dev), torch.from_numpy(d['player'].astype(np.int32)).to(dev),
                                  torch.from_numpy(d['action'].astype(np.int32)).to(dev), torch.zeros(n, dtype=torch.int64, device=dev),
                                  stream0=77, counters=counters)
    out, nxt, cnt = out.cpu().numpy(), nxt.cpu().numpy(), counters.cpu().numpy()
    exp, exp_pl, exp_cnt = np.empty_like(out), np.empty_like(nxt), np.empty_like(cnt)
    for i in range(n):
        rng = og.rng(seed=1234, stream=77 + i)
        rng.counter = 3 * i
        b, exp_pl[i] = og.getNextState(d['state'][i], int(d['player'][i]), int(d['action'][i]), 0, rng)
        exp[i], exp_cnt[i] = b.reshape(-1), rng.counter
    E.check_equal(variant, 'random_seed == 0, next state', out, exp, d['action'], d['row'])
    E.check_equal(variant, 'random_seed == 0, next player', nxt, exp_pl, d['action'], d['row'])
    E.check_equal(variant, 'random_seed == 0, counter after the step', cnt, exp_cnt, d['action'], d['row'])
    return int((exp_cnt - 3 * np.arange(n)).sum())


def symmetries(variant, g, og, r, head):
    """symmetries_batch vs og.getSymmetries on 256 positions in canonical form: 128 spread over the cover rows, and the last position
    before the end of 128 games.  pi has the support MCTS gives it where the reference maps only the entries of valid actions (Abalone,
    Akropolis: test_gpu_env.test_symmetries_vs_golden_and_oracle)."""
    import torch
    last = np.flatnonzero(r['ended'].any(axis=1))            # (the state of a game's last transition is its last open position)
    pos = np.concatenate([head[np.linspace(0, len(head) - 1, 128).astype(np.int64)], last[np.linspace(0, len(last) - 1, 128).astype(np.int64)]])
    rng = np.random.default_rng(3)
    K, on_valid = g.max_symmetries(), E.VARIANTS[variant][0] in ('ABALONE', 'AKROPOLIS')
    states = np.stack([og.getCanonicalForm(r['state'][i].reshape(og.shape), int(r['player'][i])).reshape(-1) for i in pos])
    vas = np.stack([og.getValidMoves(s.reshape(og.shape), 0) for s in states]).astype(np.uint8)
    pis = rng.random(vas.shape).astype(np.float32) * (vas if on_valid else 1)
    ob, op, ov, cnt = g.symmetries_batch(torch.from_numpy(states).to(g.device), torch.from_numpy(pis).to(g.device), torch.from_numpy(vas).to(g.device))
    ob, op, ov, cnt = ob.cpu().numpy(), op.cpu().numpy(), ov.cpu().numpy(), cnt.cpu().numpy()
    for j, i in enumerate(pos):
        syms = og.getSymmetries(states[j].reshape(og.shape), pis[j], vas[j], max_sym=K)
        where = '%s symmetries: position %d (row %d of rows(), action %d)' % (variant, j, i, r['action'][i])
        assert len(syms) == int(cnt[j]), (where, len(syms), int(cnt[j]))
        for k, (s, p_, v_) in enumerate(syms):
            for what, got, exp in (('board', ob[j, k], s.reshape(-1)), ('pi', op[j, k], p_), ('valids', ov[j, k], v_.astype(np.uint8))):
                if not np.array_equal(got, exp):
                    b = int(np.flatnonzero(got != exp)[0])
                    raise AssertionError('%s, form %d, %s: first differing element %d: got %r, expected %r' % (where, k, what, b, got[b], exp[b]))
    return len(pos)


@pytest.mark.parametrize('variant', list(E.VARIANTS))
def test_env_kernels_on_every_reachable_action_id(golden_dir, variant):
    g, og = make_game(variant), E.oracle_game(variant)
    assert (g.S, g.A, g.P) == (og.S, og.A, og.P)
    r = E.rows(variant)
    idx, group = E.select(r)
    sel = E.take(r, idx)
    sel['row'] = idx
    # 1. the whole selection against the oracle
    full = kernel_outputs(g, sel)
    compare(variant, 'kernels vs oracle rows', full, sel, sel['action'], idx)
    # 2. the launch tail: the first n rows alone give what they gave inside the full batch
    for n in TAILS:
        few = kernel_outputs(g, sel, n)
        compare(variant, 'first %d rows alone vs the same rows of the full batch' % n, few, full, sel['action'], idx)
    # 3. the reference's own answers on the committed head of the selection
    d = dict(np.load(os.path.join(golden_dir, 'envcover_%s.npz' % variant)))
    assert len(d['action']) > 0 and np.array_equal(d['row'], idx[:len(d['row'])]) and np.array_equal(d['state'], sel['state'][:len(d['row'])])
    compare(variant, 'kernels vs envcover_%s.npz' % variant, kernel_outputs(g, d), d, d['action'], d['row'])
    # 4. random_seed == 0 on every covering row of the games that draw
    head = idx[group <= 2]
    if E.VARIANTS[variant][0].lower() in E.STOCHASTIC:
        cover = {k: (v[group <= 2] if isinstance(v, np.ndarray) else v) for k, v in sel.items()}
        drawn = true_random_steps(variant, g, og, cover)
        assert drawn > 0, variant                            # the counter stream really was consumed somewhere
    # 5. symmetries of cover and last-ply positions
    if variant in SYMMETRIES:
        assert symmetries(variant, g, og, r, head) == 256
