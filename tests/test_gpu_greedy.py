"""GPU: the greedy players -- azg_greedy_candidates (csrc/lookahead.hip.h) and arena.GreedyContestant -- against the NumPy restatement of
tests/greedyref.py, which tests/test_greedy_reference.py holds to the live reference's <G>Players.GreedyPlayer on the same positions.
Candidate masks: the kernel fed with the ORACLE's valid moves and scores equals the restatement on the canonicalised envcover rows of
greedyref.positions -- rule 'reference' on Splendor with 2 and 3 players, Azul and Abalone, rule 'lead' on Santorini without gods and
Minivilles -- and so does the kernel fed by lookahead_batch, i.e. what GreedyContestant runs.  The Splendor rows reach the branches
M != init, buy and gem (counted here); they never reach the last fallback (every valid id), which only a hand-made valid row reaches:
test_splendor_last_fallback.  The Abalone rows hold positions where a push changes a score and positions where every d_a ties; the Azul
rows positions where move 0 is valid (the `not best_move` quirk).
Arena: 8 games of GreedyContestant against RandomContestant in Splendor-2p and Abalone, recorded and replayed on the oracle ply for ply:
every greedy move is the floor(u |C|)-th restated candidate for u = the draw (rng_seed, stream0 + (c + 1) << 30 + i, counter = the
contestant's k-th move of game i), and n_parallel = 8 and 3 play the same games."""
import numpy as np
import pytest

import envcover as E
import greedyref as R

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1
CASES = (('splendor2', 'reference'), ('splendor3', 'reference'), ('azul', 'reference'), ('abalone', 'reference'), ('santorini1', 'lead'),
         ('minivilles2', 'lead'))


def mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def u01(seed, stream, counter):
    """the RNG contract of include/azg.h"""
    raw = mix64((mix64((mix64((seed ^ 0x9E3779B97F4A7C15) & M64) + stream) & M64) + counter) & M64)
    return (raw >> 11) * 2.0 ** -53


def make_game(variant):
    import test_gpu_lookahead
    return test_gpu_lookahead.make_game(variant)


def family(variant):
    return (E.VARIANTS[variant] if variant in E.VARIANTS else E.DRAWING[variant])[0]


@pytest.mark.parametrize('variant,rule', CASES)
def test_candidate_masks_equal_the_restatement(variant, rule):
    import torch
    from azg_amd.games import greedy_candidates
    g, og, name = make_game(variant), E.oracle_game(variant), family(variant)
    boards = R.positions(variant)
    n, dev = len(boards), g.device
    valid, scores, exp, count = np.zeros((n, g.A), np.uint8), np.zeros((n, g.A, g.P), np.int64), np.zeros((n, g.A), np.uint8), {}
    for t, b in enumerate(boards):
        valid[t], scores[t] = R.oracle_scores(og, b, seed=g.rng_seed, stream=40 + t)
        exp[t] = R.mask(R.candidates(rule, name, og, b) if name == 'AZUL' else R.from_scores(rule, name, og, b, valid[t], scores[t]), g.A)
        v = valid[t].astype(bool)
        if name == 'SPLENDOR':
            what = R.splendor(v, scores[t], og.getScore(b.reshape(og.shape), 0))[1]
        elif name == 'ABALONE':
            d = scores[t][v, 1] - scores[t][v, 0]
            what = 'push' if d.max() != d.min() else 'tie'
        elif name == 'AZUL':
            what = 'zero' if v[0] else 'other'
        else:
            what = 'fewer' if exp[t].sum() < v.sum() else 'every'            # the rule narrows the valid moves / every move ties
        count[what] = count.get(what, 0) + 1
    print(variant, rule, n, 'positions', count, 'candidates per position: mean %.1f' % exp.sum(axis=1).mean())
    need = {'SPLENDOR': ('max', 'buy', 'gem'), 'ABALONE': ('push', 'tie'), 'AZUL': ('zero', 'other')}.get(name, ('fewer', 'every'))
    assert all(count.get(k, 0) > 0 for k in need) and count.get('none', 0) == 0, count
    assert (exp.sum(axis=1) >= 1).all() and (exp <= valid).all()
    cb, cv = torch.from_numpy(boards).to(dev), torch.from_numpy(valid).to(dev)
    cs = torch.from_numpy(scores.astype(np.int32)).to(dev)
    # 1. the rule kernel on the oracle's scores
    got = greedy_candidates(g, rule, cb, cv, cs).cpu().numpy()
    E.check_equal(variant, 'candidates (%s) from the oracle scores' % rule, got, exp, exp.argmax(axis=1))
    if name == 'AZUL':                                                    # the board alone: no scores
        assert np.array_equal(greedy_candidates(g, rule, cb, cv, None).cpu().numpy(), exp) and (exp.sum(axis=1) == 1).all()
    # 2. fed by the lookahead on the same streams: what GreedyContestant launches
    ahead = g.lookahead_batch(cb, stream0=40)
    assert np.array_equal(ahead.valid.cpu().numpy(), valid) and np.array_equal(ahead.scores.cpu().numpy(), scores)
    assert np.array_equal(greedy_candidates(g, rule, cb, ahead.valid, ahead.scores).cpu().numpy(), exp)
    # 3. rows with active == 0 keep what the buffer held; a position without a valid move gives an all-zero row
    active = torch.arange(n, device=dev) % 2 == 0
    out = torch.full((n, g.A), 7, dtype=torch.uint8, device=dev)
    greedy_candidates(g, rule, cb, cv, cs, active=active, out=out)
    a = active.cpu().numpy()
    assert np.array_equal(out.cpu().numpy()[a], exp[a]) and (out.cpu().numpy()[~a] == 7).all()
    none = torch.full((n, g.A), 7, dtype=torch.uint8, device=dev)
    greedy_candidates(g, rule, cb, torch.zeros_like(cv), cs, out=none)
    assert int(none.sum()) == 0
    # 4. the move: azg_pick_actions mode 0 on the candidates, one draw per move
    from azg_amd.arena import PICK_UNIFORM, pick_actions
    counters = torch.full((n,), 9, dtype=torch.int64, device=dev)
    moves = pick_actions(PICK_UNIFORM, None, torch.from_numpy(exp).to(dev), rng_seed=g.rng_seed, stream0=1000, counters=counters).cpu().numpy()
    for t in range(n):
        c = np.flatnonzero(exp[t])
        assert moves[t] == c[min(int(u01(g.rng_seed, 1000 + t, 9) * len(c)), len(c) - 1)], (variant, t)
    assert (counters.cpu().numpy() == 10).all()


def test_splendor_last_fallback():
    """nothing affordable on the table and no gem move valid: every valid id.  No steered position is like that, so the valid row is
    made by hand (reserve moves 12..26 and buy-reserved 27..29 only) on a real position whose scores all tie with init"""
    import torch
    from azg_amd.games import greedy_candidates
    g, og = make_game('splendor2'), E.oracle_game('splendor2')
    b = R.positions('splendor2')[0]
    init = og.getScore(b.reshape(og.shape), 0)
    valid = np.zeros(g.A, np.uint8)
    valid[[13, 20, 28]] = 1
    scores = np.full((g.A, g.P), init, np.int32)
    exp, what = R.splendor(valid.astype(bool), scores.astype(np.int64), init)
    assert what == 'all'
    got = greedy_candidates(g, 'reference', torch.from_numpy(b[None]).to(g.device), torch.from_numpy(valid[None]).to(g.device),
                            torch.from_numpy(scores[None]).to(g.device)).cpu().numpy()[0]
    assert np.array_equal(got, R.mask(exp, g.A)) and got.sum() == 3


def test_the_reference_rule_of_a_game_without_one_is_an_error():
    import torch
    from azg_amd import _lib, games
    from azg_amd.arena import BatchedArena, GreedyContestant, RandomContestant
    g = games.SantoriniGame(1)
    b = torch.from_numpy(R.positions('santorini1')[:2]).to(g.device)
    ahead = g.lookahead_batch(b)
    with pytest.raises(_lib.AzgError, match='the reference defines no greedy player for this game'):
        games.greedy_candidates(g, 'reference', b, ahead.valid, ahead.scores)
    with pytest.raises(_lib.AzgError, match='the reference defines no greedy player for this game'):
        BatchedArena(g, GreedyContestant('reference'), RandomContestant(), None, n_parallel=2).play_wave(0, 2)
    assert games.greedy_candidates(g, 'lead', b, ahead.valid, ahead.scores).sum() >= 2


def play(g, n_parallel, waves, stream0=500):
    """GreedyContestant (contestant 0) against RandomContestant over the waves [(first, n), ...] -> per game (result, [(board, player,
    action), ...]) from play_wave's record"""
    from azg_amd.arena import BatchedArena, GreedyContestant, RandomContestant
    arena = BatchedArena(g, GreedyContestant(), RandomContestant(), None, n_parallel=n_parallel, stream0=stream0)
    assert arena.mcts == []
    games_ = []
    for first, n in waves:
        rec = []
        res, _ = arena.play_wave(first, n, record=rec)
        assert len(rec) < arena.max_plies, 'a game did not end'
        res = res.cpu().numpy()
        plies = [[] for _ in range(n)]
        for boards, cur, actions, done in rec:
            bo, cu, ac, do = boards.cpu().numpy(), cur.cpu().numpy(), actions.cpu().numpy(), done.cpu().numpy()
            for i in range(n):
                if not do[i]:
                    plies[i].append((bo[i], int(cu[i]), int(ac[i])))
        games_ += [(float(res[i]), plies[i]) for i in range(n)]
    return games_


@pytest.mark.parametrize('variant', ['splendor2', 'abalone'])
def test_arena_games_replayed_on_the_oracle(variant):
    g, og, name = make_game(variant), E.oracle_game(variant), family(variant)
    stream0 = 500
    full = play(g, 8, [(0, 8)])
    greedy_moves = sizes = 0
    for i, (result, plies) in enumerate(full):
        rng = og.rng(seed=g.rng_seed, stream=stream0 + i)                # the arena's env stream of game i, from Board.init_game on
        board, cur, k = og.getInitBoard(rng), 0, [0, 0]
        greedy_seat0 = i % 4 in (0, 3)                                    # "one vs two": seat 0 belongs to contestant 0
        for b, p, a in plies:
            assert np.array_equal(b, board.reshape(-1)) and p == cur, (variant, i)
            c = 0 if (cur == 0) == greedy_seat0 else 1
            canonical = og.getCanonicalForm(board, cur)
            cand = R.candidates('reference', name, og, canonical) if c == 0 else np.flatnonzero(og.getValidMoves(canonical, 0))
            u = u01(g.rng_seed, stream0 + (c + 1) * (1 << 30) + i, k[c])
            assert a == cand[min(int(u * len(cand)), len(cand) - 1)], (variant, 'game', i, 'contestant', c, 'move', k[c], a, cand.tolist())
            greedy_moves += c == 0
            sizes += len(cand) if c == 0 else 0
            k[c] += 1
            board, cur = og.getNextState(board, cur, a, 0, rng)
        ended = og.getGameEnded(board, cur)
        assert ended.any() and ended[0] == np.float32(result), (variant, i, ended, result)
    print(variant, 'greedy moves', greedy_moves, 'mean candidates %.2f' % (sizes / greedy_moves), 'results', [r for r, _ in full])
    assert greedy_moves >= 8 * 4
    # the same games whatever n_parallel: three waves of at most 3
    small = play(g, 3, [(0, 3), (3, 3), (6, 2)])
    assert [r for r, _ in small] == [r for r, _ in full]
    assert [[a for _, _, a in p] for _, p in small] == [[a for _, _, a in p] for _, p in full]
