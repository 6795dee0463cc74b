"""Smallworld 2 / 3 / 4 players on the asynchronous tree pipeline (csrc/azg_async.hip.h: k_async_select<SmallworldDev<P>> + the V62
transformer as the persistent net kernel's body, k_async_net<NetSw62<P>>; include/azg.h azg_forest_async_rounds_sw62): the pipeline itself
plays the oracle's episodes, it equals the two-kernel rounds record for record, the work-sharing budget plays the same games, and the
engine refuses what the pipeline cannot run -- opt-in only, the default stays the two-kernel rounds."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_selfplay import _first_games_vs_oracle
from tools_args import MCTS_ARGS

pytestmark = pytest.mark.gpu

_VARIANT = {2: 'smallworld', 3: 'smallworld3', 4: 'smallworld4'}


class Args(dict):
    __getattr__ = dict.get


def _v62(golden_dir, P, T):
    from azg_amd import nnet
    w = os.path.join(golden_dir, 'weights_%s_v62.npz' % _VARIANT[P])
    return nnet.SmallworldV62Hip(nnet.SmallworldV62.from_npz(w, num_players=P, device='cuda:0'), max_batch=T)


def _args(P, sims, forced=False):
    # (forced playouts prune the policy target: with a few dozen simulations and Smallworld's many valid moves a pruned target can be empty,
    # error bit 64 on either side -- only the configuration with the most simulations keeps them on)
    return Args(numMCTSSims=sims, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0.3, temperature=[1.25, 0.8, 1.0], tempThreshold=6,
                **{**MCTS_ARGS[_VARIANT[P]], 'forced_playouts': forced})


@pytest.mark.parametrize('variant', ['smallworld', 'smallworld3', 'smallworld4'])
def test_async_pipeline_smallworld_first_games_vs_oracle(variant):
    """the PIPELINE itself (persistent Smallworld descent kernel, the hash-net evaluated inside the persistent evaluator kernel, moves /
    examples / restarts in-kernel) plays the oracle's episodes (Coach.py:37-84,117-144)"""
    _first_games_vs_oracle(variant, 1.0, 'async')


@pytest.mark.parametrize('P,T,sims,K,budget,cfg,forced', [(2, 48, 32, 16, 20, {}, True), (2, 32, 24, 8, 0, dict(n_net=2, n_sel=3), False),
                                                          (3, 40, 24, 8, 20, dict(n_net=5, n_sel=4), False), (4, 32, 24, 16, 20, {}, False)])
def test_async_pipeline_sw62_equals_two_kernel_rounds(golden_dir, P, T, sims, K, budget, cfg, forced):
    """azg_forest_async_rounds_sw62 with per-tree budgets against the two-kernel rounds (azg_forest_select_fused + azg_selfplay_advance +
    azg_nn_sw62_forward) on the shipped V62 weights: the same games move for move -- every statistics counter, every drained example record
    and every root statistic EQUAL.  This ties the pipeline's NetSw62 forward bit for bit to k_sw62_net (partly filled batches included:
    n_net = 2 / n_sel = 3 leaves most forwards short of their 4 samples)."""
    from azg_amd import games
    from azg_amd.selfplay import SelfPlayEngine
    g = games.SmallworldGame(P)
    args = _args(P, sims, forced)
    out = []
    for pipe in (False, True):
        e = SelfPlayEngine(g, _v62(golden_dir, P, T), args, T, node_capacity=4096, max_examples=T * 400, rng_seed=17, use_graph=False,
                           advance_every=1, work_budget=budget, async_pipe=pipe, async_cfg=dict(cfg, shared_budget=False))
        assert e.async_pipe == pipe
        e.start()
        n_rounds = (110 if P == 2 else 220) * (sims + 2)
        if pipe:
            for _ in range(n_rounds // K):
                e.run(K)
            e.run(n_rounds % K)
        else:
            for _ in range(n_rounds):
                e.groups[0].round(e.fused, advance=True)
        torch.cuda.synchronize()
        st = e.stats()
        assert st['errors'] == 0 and st['plies'] > 10 * T, (st['errors'], e.forest.async_profile()['ctl'] if pipe else None)
        assert e.forest.validate(verbose=False) == 0
        ex = [x.cpu() for x in e.drain_examples(symmetries=False)]
        m = ex[5].to(torch.int64)
        order = torch.argsort((m[:, 0] * 100000 + m[:, 1]) * 1000 + m[:, 2])
        ex = [x[order] for x in ex]
        rs = {k: v.cpu() for k, v in e.forest.root_stats().items()}
        out.append((st, ex, rs))
        e.close()
    (s0, e0, r0), (s1, e1, r1) = out
    for k in ('plies', 'games', 'sims', 'levels', 'expansions', 'terminal_hits', 'examples', 'sum_valid_visited', 'sum_depth_at_expand', 'errors'):
        assert s0[k] == s1[k], (k, s0[k], s1[k])
    assert s0['games'] > 0 and len(e0[0]) == len(e1[0]) > 0
    for a, b in zip(e0, e1):
        assert torch.equal(a, b)
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


def test_async_pipeline_sw62_shared_budget_plays_the_same_games(golden_dir):
    """the work-sharing budget (SelfPlayEngine's default for the pipeline) over launches of odd lengths plays the games the per-tree budget
    plays: one whole game per tree, then every drained record, keyed (stream, game, ply), equal"""
    from azg_amd import games
    from azg_amd.selfplay import SelfPlayEngine
    P, T = 2, 32
    g = games.SmallworldGame(P)
    args = _args(P, 16)
    res = []
    for shared, lengths in ((True, (37, 91, 13, 255, 64, 7)), (False, (64,))):
        e = SelfPlayEngine(g, _v62(golden_dir, P, T), args, T, node_capacity=2048, max_examples=T * 400, rng_seed=5, stream0=40,
                           async_pipe=True, async_cfg=dict(shared_budget=shared))
        assert e.async_pipe and e.groups[0].async_cfg['shared_budget'] is shared
        e.start(episode_quota=T)
        for k in range(4000):
            e.run(lengths[k % len(lengths)])
            st = e.stats()
            assert st['errors'] == 0, st
            if st['active'] == 0:
                break
        assert st['games'] == T and st['active'] == 0
        assert e.forest.validate() == 0
        ex = [x.cpu().numpy() for x in e.drain_examples(symmetries=False)]
        meta = ex[5]
        order = np.lexsort((meta[:, 2], meta[:, 1], meta[:, 0]))
        res.append([x[order] for x in ex])
        e.close()
    assert len(res[0][0]) > T
    for a, b in zip(res[0], res[1]):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_async_pipeline_sw62_refusals(golden_dir):
    """async_pipe=True is refused (ValueError, before anything is made or launched) for the torch net, for two groups and for a kernel net
    whose static buffers are not (n_games, A); the C entry point refuses another game's forest and null arguments and launches nothing"""
    from azg_amd import _lib, games, nnet
    from azg_amd.forest import Forest
    from azg_amd.selfplay import SelfPlayEngine
    T = 8
    g = games.SmallworldGame(2)
    args = _args(2, 8)
    base = nnet.SmallworldV62.from_npz(os.path.join(golden_dir, 'weights_smallworld_v62.npz'), num_players=2, device='cuda:0')
    with pytest.raises(ValueError):
        SelfPlayEngine(g, base, args, T, async_pipe=True)
    with pytest.raises(ValueError):
        SelfPlayEngine(g, nnet.SmallworldV62Hip(base, max_batch=T // 2), args, T, groups=2, async_pipe=True)
    with pytest.raises(ValueError):
        SelfPlayEngine(g, nnet.SmallworldV62Hip(base, max_batch=2 * T), args, T, async_pipe=True)

    hip = nnet.SmallworldV62Hip(base, max_batch=T)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sp = Forest(_lib.SPLENDOR, 2, T, args, node_capacity=256)
    spi, sv = torch.zeros((T, sp.A), device='cuda'), torch.zeros((T, sp.P), device='cuda')
    assert L.azg_forest_async_rounds_sw62(sp.h, p(sp.leaf_valid), p(sp.needs_eval), p(spi), p(sv), 0, hip.ptrs, 4, 0, 0, -1, 0, st) < 0
    assert 'Smallworld' in L.azg_last_error().decode()
    f = Forest(g.GAME_ID, g.variant, T, args, node_capacity=256)
    pi, v = torch.zeros((T, f.A), device='cuda'), torch.zeros((T, f.P), device='cuda')
    assert L.azg_forest_async_rounds_sw62(None, p(f.leaf_valid), p(f.needs_eval), p(pi), p(v), 0, hip.ptrs, 4, 0, 0, -1, 0, st) < 0
    assert L.azg_forest_async_rounds_sw62(f.h, None, p(f.needs_eval), p(pi), p(v), 0, hip.ptrs, 4, 0, 0, -1, 0, st) < 0
    assert L.azg_forest_async_rounds_sw62(f.h, p(f.leaf_valid), p(f.needs_eval), None, p(v), 0, hip.ptrs, 4, 0, 0, -1, 0, st) < 0
    assert L.azg_forest_async_rounds_sw62(f.h, p(f.leaf_valid), p(f.needs_eval), p(pi), p(v), 0, None, 4, 0, 0, -1, 0, st) < 0
    holes = (C.c_void_p * 25)(*list(hip.ptrs))
    holes[13] = None
    assert L.azg_forest_async_rounds_sw62(f.h, p(f.leaf_valid), p(f.needs_eval), p(pi), p(v), 0, holes, 4, 0, 0, -1, 0, st) < 0
    assert 'null' in L.azg_last_error().decode()
    torch.cuda.synchronize()
    for fo in (sp, f):
        prof = fo.async_profile()
        assert prof['launches'] == 0 and prof['descents'] == 0 and prof['batches'] == 0
        assert fo.stats()['errors'] == 0
        fo.close()


def test_smallworld_default_stays_on_the_two_kernel_rounds(golden_dir):
    """without async_pipe the engine keeps Smallworld on the two-kernel rounds (the pipeline is opt-in)"""
    from azg_amd import games
    from azg_amd.selfplay import SelfPlayEngine
    T = 8
    e = SelfPlayEngine(games.SmallworldGame(2), _v62(golden_dir, 2, T), _args(2, 8), T, node_capacity=1024)
    assert e.async_pipe is False and e.percu != 'async'
    e.close()
