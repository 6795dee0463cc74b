"""Minivilles 2 / 3 / 4 players and The Little Prince 3 / 4 / 5 players on the asynchronous tree pipeline (csrc/azg_async.hip.h:
k_async_select<MinivillesDev<P>> / k_async_select<TLPDev<P>> + the MobileNet-1d forward as the persistent net kernel's body,
k_async_net<NetMb1d<Cfg..>>; include/azg.h azg_forest_async_rounds_mb1d_h2).  These are the first STOCHASTIC games on the pipeline: the
env step draws the dice / market refills from the tree's own counter stream, inside the search and between moves.  The pipeline itself
plays the oracle's episodes, it equals the two-kernel rounds record for record on the shipped nets, the work-sharing budget plays the
same games, and the engine refuses what the pipeline cannot run -- opt-in only, the default stays the two-kernel rounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_selfplay import _play_until

pytestmark = pytest.mark.gpu

KW = dict(cpuct=1.0, fpu=0.0, universes=1, forced_playouts=True)
# variant -> (game name, players, fixture tag of the shipped net (Minivilles 4p: the stand-in of weightstats_minivilles4_v82.npz))
VARIANTS = {'minivilles2': ('minivilles', 2, 'minivilles2_v82'), 'minivilles3': ('minivilles', 3, 'minivilles3_v82'),
            'minivilles4': ('minivilles', 4, 'minivilles4_v82'), 'tlp3': ('tlp', 3, 'tlp3_v83'), 'tlp4': ('tlp', 4, 'tlp4_v83'),
            'tlp5': ('tlp', 5, 'tlp5_v83')}


class Args(dict):
    __getattr__ = dict.get


def _game(variant):
    from azg_amd import games
    name, P, _ = VARIANTS[variant]
    return games.MinivillesGame(P) if name == 'minivilles' else games.TLPGame(P)


def _base(golden_dir, variant):
    from azg_amd import formats, nnet
    sd, _ = formats.fixture_state_dict(golden_dir, VARIANTS[variant][2])
    return nnet.MobileNet1d({k: torch.from_numpy(v) for k, v in sd.items()}, device='cuda:0')


def _hip(golden_dir, variant, T):
    from azg_amd import nnet
    return nnet.MobileNet1dHip(_base(golden_dir, variant), max_batch=T)


def _net_args(golden_dir, variant, sims, forced, alpha=0.3):
    """the MCTS arguments stored with the checkpoint (the 3 / 4 / 5-player ones store no `universes`: one)"""
    from azg_amd import formats
    a = formats.fixture_state_dict(golden_dir, VARIANTS[variant][2])[1]
    return Args(numMCTSSims=sims, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=alpha, temperature=[1.25, 0.8, 1.0], tempThreshold=6,
                cpuct=float(a['cpuct']), fpu=float(a['fpu']), universes=int(a.get('universes', 1)), forced_playouts=forced)


def _sorted_examples(ex):
    meta = ex[5]
    order = np.lexsort((meta[:, 2], meta[:, 1], meta[:, 0]))
    return [x[order] for x in ex]


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_stochastic_pipeline_plays_the_oracles_episodes(variant):
    """the PIPELINE itself (persistent descent kernel of the game, the hash-net evaluated inside the persistent evaluator kernel, moves /
    examples / restarts in-kernel) plays Coach.executeEpisode's episodes of the oracle: search dice, move picks and real dice interleave
    on one stream per game exactly as in the two-kernel rounds, so every canonical board, pi, q, z and player is the oracle's"""
    import azg_oracle as O
    from azg_amd.forest import Forest
    name, P, _ = VARIANTS[variant]
    g = _game(variant)
    og = O.OracleGame(O.MINIVILLES if name == 'minivilles' else O.TLP, P)
    sims, T, seed, stream0, temp = (30 if name == 'minivilles' else 40), 16, 4242, 1000, [1.25, 0.8, 1.0]
    args = Args(numMCTSSims=sims, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0, temperature=temp, tempThreshold=6, **KW)
    f = Forest(g.GAME_ID, g.variant, T, args, node_capacity=4096, max_examples=T * 1200, rng_seed=seed, stream0=stream0)
    f.selfplay_start()
    st = _play_until(f, T, 2 * T, 'async')
    assert st['games'] >= 2 * T and f.async_profile(reset=False)['launches'] > 0
    assert f.validate() == 0
    boards, pis, zs, valids, qs, meta = [x.cpu().numpy() for x in f.drain_examples()]
    for t in range(T):
        o = O.run_episode(og, O.make_args(numMCTSSims=sims, **KW), None, seed=seed, stream=stream0 + t, temp=(temp[0], temp[1]),
                          tempThreshold=6.0)
        sel = np.flatnonzero((meta[:, 0] == stream0 + t) & (meta[:, 1] == 0))
        sel = sel[np.argsort(meta[sel, 2])]
        assert len(sel) == o['plies'], (t, len(sel), o['plies'])
        for k, ply in zip(sel, range(o['plies'])):
            assert meta[k, 2] == ply and meta[k, 3] == o['player'][ply], (t, ply)
            assert np.array_equal(boards[k], o['canonical'][ply]), (t, ply)
            assert np.array_equal(pis[k], o['pi'][ply].astype(np.float32)), (t, ply)
            assert np.array_equal(qs[k], o['q'][ply]), (t, ply)
            assert np.array_equal(zs[k], np.roll(o['result'], -int(o['player'][ply]))), (t, ply)
            assert np.array_equal(valids[k].astype(bool), og.getValidMoves(o['canonical'][ply], 0)), (t, ply)
    f.close()


# (variant, trees, simulations, launch length K, work budget, split, forced playouts, rounds / (simulations + 2): about the plies a tree plays)
@pytest.mark.parametrize('variant,T,sims,K,budget,cfg,forced,mult', [
    ('minivilles2', 48, 24, 8, 20, dict(n_net=2, n_sel=3), False, 120),        # most forwards short of their 16 samples
    ('minivilles3', 32, 24, 16, 0, {}, False, 120),                             # no work budget
    ('minivilles4', 32, 24, 8, 20, {}, True, 120),                              # forced playouts
    ('tlp3', 40, 24, 8, 20, dict(n_net=3, n_sel=2), False, 100),                 # most forwards short of their 8 samples
    ('tlp4', 32, 24, 16, 0, {}, True, 100),
    ('tlp5', 30, 24, 8, 20, {}, False, 100)])
def test_stochastic_pipeline_equals_two_kernel_rounds(golden_dir, variant, T, sims, K, budget, cfg, forced, mult):
    """azg_forest_async_rounds_mb1d_h2 with per-tree budgets against the two-kernel rounds (azg_forest_select_fused + azg_selfplay_advance +
    azg_nn_mb1d_forward_h2) on the shipped V82 / V83 nets: the same games move for move -- every statistics counter, every drained example
    record and every root statistic EQUAL.  A tree's stream is drawn from in the same order by both (the search's env steps, the move
    pick, the real dice / refills, the next root), and NetMb1d is bit for bit the stand-alone forward, partly filled batches included."""
    from azg_amd.selfplay import SelfPlayEngine
    g = _game(variant)
    args = _net_args(golden_dir, variant, sims, forced)
    out = []
    for pipe in (False, True):
        e = SelfPlayEngine(g, _hip(golden_dir, variant, T), args, T, node_capacity=4096, max_examples=T * 600, rng_seed=13, use_graph=False,
                           advance_every=1, work_budget=budget, async_pipe=pipe, async_cfg=dict(cfg, shared_budget=False))
        assert e.async_pipe == pipe
        e.start()
        n_rounds = mult * (sims + 2)
        if pipe:
            for _ in range(n_rounds // K):
                e.run(K)
            e.run(n_rounds % K)
        else:
            for _ in range(n_rounds):
                e.groups[0].round(e.fused, advance=True)
        torch.cuda.synchronize()
        st = e.stats()
        assert st['errors'] == 0 and st['plies'] > 10 * T, (st, e.forest.async_profile()['ctl'] if pipe else None)
        assert e.forest.validate(verbose=False) == 0
        ex = _sorted_examples([x.cpu().numpy() for x in e.drain_examples(symmetries=False)])
        rs = {k: v.cpu() for k, v in e.forest.root_stats().items()}
        out.append((st, ex, rs))
        e.close()
    (s0, e0, r0), (s1, e1, r1) = out
    for k in ('plies', 'games', 'sims', 'levels', 'expansions', 'terminal_hits', 'examples', 'sum_valid_visited', 'sum_depth_at_expand', 'errors'):
        assert s0[k] == s1[k], (k, s0[k], s1[k])
    assert s0['games'] > 0 and len(e0[0]) == len(e1[0]) > 0
    for a, b in zip(e0, e1):
        assert a.shape == b.shape and np.array_equal(a, b)
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


@pytest.mark.parametrize('variant', ['minivilles2', 'tlp3'])
def test_stochastic_pipeline_shared_budget_plays_the_same_games(golden_dir, variant):
    """the work-sharing budget (SelfPlayEngine's default for the pipeline) over launches of odd lengths, and deterministic=True, play the
    games of the per-tree budget: one whole game per tree (an episode quota played to the end), every drained record keyed (stream, game,
    ply) equal"""
    from azg_amd.selfplay import SelfPlayEngine
    T = 32
    g = _game(variant)
    args = _net_args(golden_dir, variant, 16, True)
    res = []
    for kw, lengths in ((dict(async_cfg=dict(shared_budget=True)), (37, 91, 13, 255, 64, 7)), (dict(deterministic=True), (50,)),
                        (dict(async_cfg=dict(shared_budget=False)), (64,))):
        e = SelfPlayEngine(g, _hip(golden_dir, variant, T), args, T, node_capacity=2048, max_examples=T * 600, rng_seed=5, stream0=40,
                           async_pipe=True, **kw)
        assert e.async_pipe and e.groups[0].async_cfg['shared_budget'] is kw.get('async_cfg', {}).get('shared_budget', False)
        e.start(episode_quota=T)
        for k in range(20000):
            e.run(lengths[k % len(lengths)])
            st = e.stats()
            assert st['errors'] == 0, st
            if st['active'] == 0:
                break
        assert st['games'] == T and st['active'] == 0
        assert e.forest.validate() == 0
        res.append(_sorted_examples([x.cpu().numpy() for x in e.drain_examples(symmetries=False)]))
        e.close()
    assert len(res[0][0]) > T
    for other in res[:2]:
        for a, b in zip(other, res[2]):
            assert a.shape == b.shape and np.array_equal(a, b)


def test_stochastic_pipeline_refusals(golden_dir):
    """async_pipe=True is refused (ValueError, before anything is made or launched) for the torch net, for two groups and for a kernel net
    whose static buffers are not (n_games, A); the C entry point refuses a geometry of another game -- naming both -- and null arguments,
    and launches nothing"""
    from azg_amd import _lib, nnet
    from azg_amd.forest import Forest
    from azg_amd.selfplay import SelfPlayEngine
    T = 8
    g = _game('minivilles2')
    args = _net_args(golden_dir, 'minivilles2', 8, False)
    base = _base(golden_dir, 'minivilles2')
    with pytest.raises(ValueError):
        SelfPlayEngine(g, base, args, T, async_pipe=True)
    with pytest.raises(ValueError):
        SelfPlayEngine(g, nnet.MobileNet1dHip(base, max_batch=T // 2), args, T, groups=2, async_pipe=True)
    with pytest.raises(ValueError):
        SelfPlayEngine(g, nnet.MobileNet1dHip(base, max_batch=2 * T), args, T, async_pipe=True)
    with pytest.raises(ValueError):          # a TLP net on a Minivilles engine
        SelfPlayEngine(g, _hip(golden_dir, 'tlp3', T), args, T, async_pipe=True)

    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    mv = _hip(golden_dir, 'minivilles2', T)
    sp3 = nnet.MobileNet1dHip(nnet.SplendorV80.random_init(num_players=3, seed=5, device='cuda:0'), max_batch=T)
    forests = []

    def forest(game):
        f = Forest(game.GAME_ID, game.variant, T, args, node_capacity=256)
        forests.append(f)
        return f, torch.zeros((f.T, f.A), device='cuda'), torch.zeros((f.T, f.P), device='cuda')

    def call(fo, net, pi_t, v_t, **kw):
        a = dict(f=fo.h, geo=net.geometry, lv=p(fo.leaf_valid), ne=p(fo.needs_eval), pi=p(pi_t), v=p(v_t), w=net.fused_ptrs_h2, d=net.descale_h2)
        a.update(kw)
        return L.azg_forest_async_rounds_mb1d_h2(a['f'], a['geo'], a['lv'], a['ne'], a['pi'], a['v'], 0, a['w'], a['d'], 4, 0, 0, -1, 0, st)

    tf, tpi, tv = forest(_game('tlp3'))
    assert call(tf, mv, tpi, tv) < 0                 # a Minivilles geometry on a TLP forest
    msg = L.azg_last_error().decode()
    assert 'does not match' in msg and 'Minivilles 2 players' in msg and 'The Little Prince' in msg, msg
    mf, mpi, mv_ = forest(g)
    assert call(mf, sp3, mpi, mv_) < 0               # a Splendor geometry on a Minivilles forest
    msg = L.azg_last_error().decode()
    assert 'does not match' in msg and 'Splendor 3 players' in msg and 'Minivilles' in msg, msg
    assert call(mf, mv, mpi, mv_, geo=99) < 0
    assert 'geometry must be' in L.azg_last_error().decode()
    for bad in (dict(f=None), dict(lv=None), dict(ne=None), dict(pi=None), dict(v=None), dict(w=None), dict(d=None)):
        assert call(mf, mv, mpi, mv_, **bad) < 0, bad
        assert 'null' in L.azg_last_error().decode(), bad
    torch.cuda.synchronize()
    for fo in forests:
        prof = fo.async_profile()
        assert prof['launches'] == 0 and prof['descents'] == 0 and prof['batches'] == 0
        assert fo.stats()['errors'] == 0
        fo.close()


@pytest.mark.parametrize('variant', ['minivilles2', 'tlp3'])
def test_stochastic_games_default_stays_on_the_two_kernel_rounds(golden_dir, variant):
    """without async_pipe the engine keeps Minivilles and The Little Prince on the two-kernel rounds (the pipeline is opt-in)"""
    from azg_amd.selfplay import SelfPlayEngine
    T = 8
    e = SelfPlayEngine(_game(variant), _hip(golden_dir, variant, T), _net_args(golden_dir, variant, 8, False), T, node_capacity=1024)
    assert e.async_pipe is False and e.percu != 'async'
    e.close()
