"""GPU: nnet.RolloutEvaluator -- uniform prior, mean of random playouts as the leaf value -- by itself and in the place of an nnet in
BatchedMCTS, BatchedArena and SelfPlayEngine; arena.random_games.  What is checked is the contract: the values are the playouts' mean on
the evaluator's own streams, the searches are structurally sound and repeat with their seeds -- never a win rate."""
import numpy as np
import pytest

from tools_args import MCTS_ARGS

pytestmark = pytest.mark.gpu


class Args(dict):
    __getattr__ = dict.get


def args(**kw):
    # forced_playouts off: with it the reference's policy-target pruning zeroes every root count <= 1 (MCTS.py:78-79), the best one too, and
    # eight simulations spread by a uniform prior over an opening's moves leave no count above 1 -- 0 / 0 there, error bit 64 here
    return Args(dict(dict(MCTS_ARGS['minivilles2']), prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0, temperature=[1, 1, 1], forced_playouts=False), **kw)


def test_predict_batch_is_the_mean_of_its_playouts():
    import torch
    from azg_amd import games
    from azg_amd.nnet import RolloutEvaluator
    g = games.SplendorGame(2, rng_seed=3)
    B, k = 3, 4
    boards = g.init_boards_batch(B, 100)
    valids = g.valid_moves_batch(boards, None)
    ev = RolloutEvaluator(g, k, max_batch=B)
    assert ev.counters.shape == (B * k,) and ev.counters.dtype == torch.int64 and tuple(ev.pi.shape) == (B, g.A) and tuple(ev.v.shape) == (B, g.P)

    def expected(counters):
        c = counters.clone()
        return g.playouts_batch(boards, k=k, max_plies=ev.max_plies, stream0=ev.stream0, counters=c).ended.mean(1), c

    want1, c1 = expected(ev.counters)
    pi, v = ev.predict_batch(boards.view((B,) + tuple(g.getBoardSize())), valids.bool())
    assert torch.equal(pi, valids.float() / valids.float().sum(dim=1, keepdim=True))
    assert torch.equal(v, want1) and torch.equal(ev.counters, c1) and bool((c1 > 0).all().item())
    v1 = v.clone()
    want2, c2 = expected(ev.counters)
    pi, v = ev.predict_batch(boards, valids)
    assert torch.equal(v, want2) and torch.equal(ev.counters, c2) and bool((c2 > c1).all().item())
    print('v of two calls', v1.tolist(), v.tolist())
    # a row without a valid action: nothing runs for it
    valids[1] = 0
    c_before = ev.counters.clone()
    pi, v = ev.predict_batch(boards, valids)
    assert bool((pi[1] == 0).all().item()) and bool((v[1] == 0).all().item())
    assert torch.equal(ev.counters[k:2 * k], c_before[k:2 * k]) and bool((ev.counters[:k] > c_before[:k]).all().item())
    assert torch.equal(pi[0], valids[0].float() / valids[0].sum())
    # the single-board form, and a clone on streams of its own
    p1, v1 = ev.predict(boards[0].cpu().numpy().reshape(g.getBoardSize()), valids[0].cpu().numpy())
    assert p1.shape == (g.A,) and v1.shape == (g.P,) and abs(float(p1.sum()) - 1.0) < 1e-6
    other = ev.clone_buffers()
    assert other.stream0 >= ev.stream0 + ev.maxB * k and other.counters.data_ptr() != ev.counters.data_ptr() and other.pi.data_ptr() != ev.pi.data_ptr()
    assert bool((other.counters == 0).all().item()) and ev.clone_buffers().stream0 != other.stream0


def test_search_with_rollouts():
    import torch
    from azg_amd import games
    from azg_amd.mcts import BatchedMCTS
    from azg_amd.nnet import RolloutEvaluator
    g = games.MinivillesGame(2, rng_seed=5)
    roots = g.init_boards_batch(4, 200)
    m = BatchedMCTS(g, RolloutEvaluator(g, 2, max_batch=4), args(numMCTSSims=8), 4)
    probs, _, _ = m.getActionProb(roots, temp=1, force_full_search=True)
    valid = g.valid_moves_batch(roots, None)
    probs = probs.cpu().numpy()
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-9) and np.all(probs[valid.cpu().numpy() == 0] == 0)
    assert m.forest.validate() == 0
    m.forest.close()


def rollout_match(n_games):
    from azg_amd import games
    from azg_amd.arena import BatchedArena, RandomContestant
    from azg_amd.nnet import RolloutEvaluator
    g = games.MinivillesGame(2, rng_seed=11)
    arena = BatchedArena(g, RolloutEvaluator(g, 2, max_batch=4), RandomContestant(), args(numMCTSSims=8), n_parallel=4, stream0=300)
    rec = []
    res, ovt = arena.play_wave(0, n_games, record=rec)
    assert len(rec) < arena.max_plies, 'a game did not end'
    moves = [(a.cpu().numpy().copy(), d.cpu().numpy().copy()) for _, _, a, d in rec]
    return arena, res.cpu().numpy(), moves


def test_arena_with_rollouts_and_random_games():
    import torch
    from azg_amd import games
    from azg_amd.arena import random_games
    arena, res, moves = rollout_match(4)
    arena2, res2, moves2 = rollout_match(4)
    assert np.array_equal(res, res2) and len(moves) == len(moves2)
    assert all(np.array_equal(a[~d], a2[~d2]) and np.array_equal(d, d2) for (a, d), (a2, d2) in zip(moves, moves2))
    one, two, draws = arena2.playGames(4)
    assert one + two + draws == 4
    for m in arena.mcts + arena2.mcts:
        m.forest.close()
    # whole random games in one launch: game i is a function of its index
    g = games.MinivillesGame(2, rng_seed=11)
    e6, p6, s6 = random_games(g, 6)
    e3, p3, s3 = random_games(g, 3)
    assert torch.equal(e6[:3], e3) and torch.equal(p6[:3], p3) and torch.equal(s6[:3], s3)
    assert tuple(e6.shape) == (6, 2) and bool((p6 > 0).all().item()) and bool(((s6 == 0) == (e6 != 0).any(dim=1)).all().item())


def test_selfplay_with_rollouts():
    import torch
    from azg_amd import games
    from azg_amd.nnet import RolloutEvaluator
    from azg_amd.selfplay import SelfPlayEngine
    g = games.MinivillesGame(2, rng_seed=7)
    eng = SelfPlayEngine(g, RolloutEvaluator(g, 2, max_batch=8), args(numMCTSSims=8, temperature=[1.25, 0.8, 1.0], tempThreshold=6), n_games=8)
    assert not eng.async_pipe
    with pytest.raises(ValueError):
        SelfPlayEngine(g, RolloutEvaluator(g, 2, max_batch=8), args(numMCTSSims=8), n_games=8, async_pipe=True)
    eng.start()
    for _ in range(100):
        eng.run(128)
        st = eng.stats()
        assert st['errors'] == 0, st
        if st['games'] >= 1:
            break
    assert st['games'] >= 1 and sum(grp.f.validate() for grp in eng.groups) == 0
    boards, pi, z, valids, q, meta = eng.drain_examples()
    pi, valids = pi.cpu().numpy(), valids.cpu().numpy()
    assert pi.shape[0] > 0 and np.all(np.isfinite(pi)) and np.all(pi[valids == 0] == 0) and np.allclose(pi.sum(axis=1), 1.0, atol=1e-5)
    assert bool((eng.nnet.counters > 0).any().item())
    eng.close()
