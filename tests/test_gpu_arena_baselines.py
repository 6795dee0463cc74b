"""GPU: the baseline contestants of BatchedArena (arena.RandomContestant, arena.PolicyContestant, arena.vs_random): the reference's
<G>Players.RandomPlayer and pit.py's raw-policy players.  What is checked is what the contestants promise -- legal moves, finished games,
results that are a function of the game index, the policy contestant's move being the argmax of its net -- never a win rate."""
import numpy as np
import pytest

from tools_args import MCTS_ARGS

pytestmark = pytest.mark.gpu


class Args(dict):
    __getattr__ = dict.get


def sequences(rec, n):
    """per game: the list of its moves, from play_wave's record"""
    seq = [[] for _ in range(n)]
    for _, _, actions, done in rec:
        d, a = done.cpu().numpy(), actions.cpu().numpy()
        for i in range(n):
            if not d[i]:
                seq[i].append(int(a[i]))
    return seq


def random_match(g, n_parallel, first, n, ctor_first=0):
    from azg_amd.arena import BatchedArena, RandomContestant
    arena = BatchedArena(g, RandomContestant(), RandomContestant(), None, n_parallel=n_parallel, stream0=700, first_game_index=ctor_first)
    assert arena.mcts == []
    rec = []
    res, ovt = arena.play_wave(first, n, record=rec)
    assert len(rec) < arena.max_plies, 'a game did not end'
    return res.cpu().numpy(), ovt.cpu().numpy(), rec, arena


def test_random_vs_random_is_legal_and_a_function_of_the_game_index():
    import torch
    from azg_amd import games
    g = games.MinivillesGame(2)
    res, ovt, rec, arena = random_match(g, 8, 0, 8)
    ok = torch.ones(8, dtype=torch.bool, device=g.device)
    for boards, cur, actions, done in rec:                    # every move is valid in the board it was played on, for the player to move
        valid = g.valid_moves_batch(boards, cur)
        ok &= done | (valid.gather(1, actions.long()[:, None])[:, 0] != 0)
    assert bool(ok.all().item())
    seq = sequences(rec, 8)
    one, two, draws = arena.playGames(8)
    assert one + two + draws == 8
    exp_one = int(((ovt & (res == 1.0)) | (~ovt & (res == -1.0))).sum())
    exp_two = int(((ovt & (res == -1.0)) | (~ovt & (res == 1.0))).sum())
    assert (one, two, draws) == (exp_one, exp_two, 8 - exp_one - exp_two)
    # n_parallel = 4, two waves
    r0, o0, rec0, _ = random_match(g, 4, 0, 4)
    r1, o1, rec1, _ = random_match(g, 4, 4, 4)
    assert np.array_equal(np.concatenate([r0, r1]), res) and np.array_equal(np.concatenate([o0, o1]), ovt)
    assert sequences(rec0, 4) + sequences(rec1, 4) == seq
    # dealt out over two ranks: arenas built for games 0..3 and 4..7
    r0, o0, rec0, _ = random_match(g, 4, 0, 4, ctor_first=0)
    r1, o1, rec1, _ = random_match(g, 4, 4, 4, ctor_first=4)
    assert np.array_equal(np.concatenate([r0, r1]), res) and np.array_equal(np.concatenate([o0, o1]), ovt)
    assert sequences(rec0, 4) + sequences(rec1, 4) == seq


def test_policy_contestant_plays_the_argmax_of_its_net():
    from azg_amd import games
    from azg_amd.arena import BatchedArena, PolicyContestant, RandomContestant
    from hashnet import HashNetTorch
    g = games.SplendorGame(2)
    net = HashNetTorch(2)
    arena = BatchedArena(g, PolicyContestant(net), RandomContestant(), None, n_parallel=4, stream0=900)
    assert arena.mcts == []
    rec = []
    res, ovt = arena.play_wave(0, 4, record=rec)
    assert len(rec) < arena.max_plies, 'a game did not end'
    ovt = ovt.cpu().numpy()
    n_policy = n_random = 0
    for boards, cur, actions, done in rec:
        canonical = g.canonical_batch(boards, cur)
        valid = g.valid_moves_batch(canonical, None)
        pi, _ = net.predict_batch(canonical.view((4,) + tuple(g.getBoardSize())), valid.bool())
        pi, va, c, a, d = pi.cpu().numpy(), valid.cpu().numpy().astype(bool), cur.cpu().numpy(), actions.cpu().numpy(), done.cpu().numpy()
        for i in range(4):
            if d[i]:
                continue
            assert va[i, a[i]], (i, a[i])
            if (c[i] == 0) == ovt[i]:                          # the policy contestant's seat
                cand = np.flatnonzero(va[i])
                assert a[i] == cand[np.argmax(pi[i][cand])], (i, a[i])
                n_policy += 1
            else:
                n_random += 1
    assert n_policy > 0 and n_random > 0


def test_search_vs_random_allocates_one_forest():
    from azg_amd import games
    from azg_amd.arena import BatchedArena, RandomContestant
    from azg_amd.mcts import BatchedMCTS
    from hashnet import HashNetTorch
    g = games.SplendorGame(2)
    a = Args(numMCTSSims=16, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0, temperature=[1, 1, 1], **dict(MCTS_ARGS['splendor2']))
    arena = BatchedArena(g, HashNetTorch(2), RandomContestant(), a, n_parallel=4, node_capacity=1024)
    assert len(arena.mcts) == 1 and isinstance(arena.contestants[0], BatchedMCTS) and isinstance(arena.contestants[1], RandomContestant)
    one, two, draws = arena.playGames(4)
    assert one + two + draws == 4


def test_vs_random_returns_the_tally():
    from azg_amd import games
    from azg_amd.arena import vs_random
    from hashnet import HashNetTorch
    g = games.SplendorGame(2)
    a = Args(numMCTSSims=8, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0, temperature=[1, 1, 1], **dict(MCTS_ARGS['splendor2']))
    out = vs_random(g, HashNetTorch(2), a, 3, node_capacity=1024)
    assert len(out) == 3 and all(type(x) is int for x in out) and sum(out) == 3
