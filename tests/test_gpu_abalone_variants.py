"""GPU: Abalone from the classic and German-Daisy openings and with dynamic komi (games.AbaloneGame(layout, dynamic_komi); csrc/game_abalone.hip.h)
against the reference's own outputs with its two module constants patched (tools/gen_golden_abalone_variants.py): env step, init boards,
symmetries and MCTS traces bit-exact; playouts and self-play on the komi rules; the two other shipped nets on the engine kernel."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# fixture name -> (layout, dynamic_komi)
CONFIGS = {'abalone_classic': ('classic', False), 'abalone_german': ('german', False), 'abalone_classic_komi': ('classic', True),
           'abalone_belgian_komi': ('belgian', True)}
KOMI_BYTE = (0 * 9 + 3) * 4 + 3          # misc[0][3]


class Args(dict):
    __getattr__ = dict.get


def make(config, **kw):
    from azg_amd import games
    layout, komi = CONFIGS[config]
    return games.AbaloneGame(layout=layout, dynamic_komi=komi, **kw)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_env_vs_golden(golden_dir, config):
    import torch
    d = np.load(os.path.join(golden_dir, 'env_%s.npz' % config))
    g = make(config)
    dev = g.device
    st = torch.from_numpy(d['state']).to(dev)
    pl = torch.from_numpy(d['player'].astype(np.int32)).to(dev)
    assert len(d['state']) >= 300
    assert np.array_equal(g.valid_moves_batch(st, pl).cpu().numpy(), np.unpackbits(d['valid'], axis=1)[:, :g.A])
    seeds = torch.from_numpy(d['seed'].astype(np.int64)).to(dev)
    act = torch.from_numpy(d['action'].astype(np.int32)).to(dev)
    nxt_state, nxt_pl = g.next_state_batch(st, pl, act, seeds)
    assert np.array_equal(nxt_state.cpu().numpy(), d['next_state'])           # (the env step is deterministic for every seed)
    assert np.array_equal(nxt_pl.cpu().numpy(), d['next_player'].astype(np.int32))
    ns = torch.from_numpy(d['next_state']).to(dev)
    npl = torch.from_numpy(d['next_player'].astype(np.int32)).to(dev)
    ended, scores, rnd = g.game_ended_batch(ns, npl)
    assert np.array_equal(ended.cpu().numpy(), d['ended'])
    assert np.array_equal(scores.cpu().numpy(), d['score'].astype(np.int32))
    assert np.array_equal(rnd.cpu().numpy(), d['round'].astype(np.int32))
    canon = g.canonical_batch(ns, npl).cpu().numpy()
    assert np.array_equal(canon, d['canonical'])
    if CONFIGS[config][1]:                # the flipped komi bit is in what was just compared
        assert (d['canonical'][:, KOMI_BYTE] != d['next_state'][:, KOMI_BYTE]).any()


@pytest.mark.parametrize('config', list(CONFIGS))
def test_init_boards(golden_dir, config):
    import torch
    import azg_oracle as O
    d = np.load(os.path.join(golden_dir, 'env_%s.npz' % config))
    want = d['init_boards'][0].reshape(81, 4)
    g = make(config, rng_seed=1234)
    n, s0 = 64, 5
    counters = torch.zeros(n, dtype=torch.int64, device=g.device)
    boards = g.init_boards_batch(n, stream0=s0, counters=counters).cpu().numpy().reshape(n, 81, 4)
    assert (boards[:, :, :3] == want[None, :, :3]).all()
    misc = boards[:, :, 3].copy()
    bits = misc[:, 3].copy()
    misc[:, 3] = 0
    assert not misc.any()
    if not CONFIGS[config][1]:
        assert not bits.any() and not counters.any().item()
        return
    og = O.OracleGame(O.ABALONE, 0)
    O.lib().azo_rng_u01.restype = C.c_double
    exp = []
    for i in range(n):
        rng = og.rng(seed=1234, stream=s0 + i)
        exp.append(int(np.floor(2.0 * O.lib().azo_rng_u01(C.byref(rng)))))
    assert bits.tolist() == exp
    assert counters.cpu().tolist() == [1] * n
    assert set(exp) == {0, 1}
    # the Game.py surface draws a fresh stream per call and hands the same position back
    b = g.getInitBoard()
    assert b.shape == (9, 9, 4) and np.array_equal(b.reshape(81, 4)[:, :3], want[:, :3])


@pytest.mark.parametrize('config', list(CONFIGS))
def test_symmetries_vs_golden(golden_dir, config):
    import torch
    d = np.load(os.path.join(golden_dir, 'sym_%s.npz' % config))
    g = make(config)
    n = len(d['state'])
    ob, op, ov, cnt = g.symmetries_batch(torch.from_numpy(d['state'].reshape(n, -1)).to(g.device), torch.from_numpy(d['pi']).to(g.device),
                                         torch.from_numpy(d['valid'].astype(np.uint8)).to(g.device))
    ob, op, ov, cnt = ob.cpu().numpy(), op.cpu().numpy(), ov.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt, d['count']) and (cnt == 12).all()
    for i in range(n):
        assert np.array_equal(ob[i], d['out_state'][i][:12].reshape(12, -1)), (config, i)
        assert np.array_equal(op[i], d['out_pi'][i][:12]), (config, i)
        assert np.array_equal(ov[i], d['out_valid'][i][:12]), (config, i)
        assert (ob[i].reshape(12, 81, 4)[:, :, 3] == d['state'][i].reshape(81, 4)[None, :, 3]).all()      # the misc plane is carried over


@pytest.mark.parametrize('config', list(CONFIGS))
def test_mcts_traces_vs_golden(golden_dir, config):
    """the assertions of test_gpu_mcts.test_mcts_traces_vs_golden (25 and 200 simulations, hash-net); the komi files hold roots at rounds
    125 and 126 with level scores, whose trees end in terminals that the bit decides"""
    import torch
    from azg_amd.mcts import BatchedMCTS
    from hashnet import HashNetTorch
    d = np.load(os.path.join(golden_dir, 'mcts_%s_numba.npz' % config))
    g = make(config)
    assert set(d['case_sims'].tolist()) == {25, 200}
    if CONFIGS[config][1]:
        late = d['case_round'] >= 124
        assert late.any() and (d['case_tied_terminals'][late] > 0).all()
    keys = {}
    for i in range(len(d['case_sims'])):
        k = (int(d['case_sims'][i]), float(d['case_cpuct'][i]), float(d['case_fpu'][i]), int(d['case_universes'][i]), int(d['case_forced'][i]))
        keys.setdefault(k, []).append(i)
    for (sims, cpuct, fpu, uni, forced), idxs in keys.items():
        args = Args(numMCTSSims=sims, cpuct=cpuct, fpu=fpu, universes=uni, forced_playouts=bool(forced), prob_fullMCTS=1.0, ratio_fullMCTS=5,
                    dirichletAlpha=0, temperature=[1, 1, 1])
        m = BatchedMCTS(g, HashNetTorch(g.P), args, len(idxs), node_capacity=sims + 64)
        probs, q, full = m.getActionProb(torch.from_numpy(d['case_root'][idxs]).to(g.device), temp=1, force_full_search=True)
        rs = m.forest.root_stats()
        for k, i in enumerate(idxs):
            assert int(rs['Ns'][k]) == int(d['case_Ns'][i]), (config, i)
            assert np.array_equal(rs['Nsa'][k].cpu().numpy(), d['case_Nsa'][i].astype(np.int32)), (config, i)
            assert np.array_equal(rs['Qsa'][k].cpu().numpy(), d['case_Qsa'][i]), (config, i)
            assert float(rs['Qs'][k]) == float(d['case_Qs'][i]), (config, i)
            assert int(rs['n_nodes'][k]) == int(d['case_nodes'][i]), (config, i)
            assert np.array_equal(probs[k].cpu().numpy(), d['case_probs'][i]), (config, i)
            assert np.array_equal(q[k].cpu().numpy(), d['case_q'][i]), (config, i)
            va = d['case_Ps'][i] > 0
            assert np.array_equal(rs['Ps'][k].cpu().numpy()[va], d['case_Ps'][i][va]), (config, i)
        m.forest.close()


def test_playouts_classic_komi():
    """arena.random_games on the komi rules: every result is a win, and the games are the ply-by-ply loop's on the same streams"""
    import torch
    from azg_amd import arena
    from test_gpu_playouts import loop
    g = make('abalone_classic_komi', rng_seed=77)
    n, s0 = 256, 5000
    ended, plies, status = arena.random_games(g, n, stream0=s0)
    assert bool((status <= 1).all().item())
    fin = status == 0
    assert bool(fin.any().item())
    e = ended[fin]
    assert bool(((e.abs() == 1).all() & (e.sum(dim=1) == 0).all()).item())
    assert bool((ended[~fin] == 0).all().item())
    m = 16                                     # the loop costs four launches a ply: the first 16 games
    counters = torch.zeros(m, dtype=torch.int64, device=g.device)
    boards = g.init_boards_batch(m, s0, counters)
    assert bool((counters == 1).all().item())
    ref = loop(g, boards, torch.zeros(m, dtype=torch.int32, device=g.device), counters, s0, 4096)
    assert torch.equal(ended[:m], ref['ended']) and torch.equal(plies[:m], ref['plies']) and torch.equal(status[:m], ref['status'])
    # among the 256 some games reach the round limit with level scores, and the bit decides them both ways
    c = torch.zeros(n, dtype=torch.int64, device=g.device)
    b0 = g.init_boards_batch(n, s0, c)
    out = g.playouts_batch(b0, k=1, stream0=s0, counters=c, final_boards=True)
    assert torch.equal(out.ended[:, 0], ended)
    fb = out.boards[:, 0].reshape(n, 81, 4)
    tie = (fb[:, 2, 3] >= 127) & (fb[:, 0, 3] == fb[:, 1, 3]) & fin
    assert bool(tie.any().item())
    # (the final board is in the seats of the input board: misc[0][3] = 1 gives the tie to seat 0)
    assert torch.equal(ended[tie][:, 0], torch.where(fb[tie][:, 3, 3] == 1, 1.0, -1.0).to(ended.dtype))
    assert len(set(ended[tie][:, 0].tolist())) == 2


def test_selfplay_classic_komi_with_the_classic_net(golden_dir):
    import torch
    from azg_amd import nnet
    from azg_amd.selfplay import SelfPlayEngine
    w = os.path.join(golden_dir, 'weights_abalone_v21_classic.npz')
    z = np.load(w)
    a = Args(numMCTSSims=16, cpuct=float(z['arg/cpuct']), fpu=float(z['arg/fpu']), universes=int(z['arg/universes']), forced_playouts=True,
             prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0.0, temperature=[1.25, 0.8, 1.0], tempThreshold=4)
    g = make('abalone_classic_komi')
    T = 16
    eng = SelfPlayEngine(g, nnet.AbaloneV21Hip(nnet.AbaloneV21.from_npz(w, device='cuda:0'), max_batch=T), a, n_games=T, node_capacity=1024,
                         max_examples=T * 512)
    eng.start()
    for _ in range(40):
        eng.run(128)
        torch.cuda.synchronize()
        if eng.stats()['games'] >= 4:
            break
    st = eng.stats()
    assert st['errors'] == 0 and st['games'] >= 4, st
    boards, pi, zz, valids, q, meta = eng.drain_examples(symmetries=False)
    zz, meta = torch.as_tensor(zz).cpu().numpy(), torch.as_tensor(meta).cpu().numpy()
    boards = torch.as_tensor(boards).cpu().numpy().reshape(-1, 81, 4)
    assert len(zz) > 0 and np.all(np.abs(zz) == 1) and np.all(zz.sum(axis=1) == 0)
    first = meta[:, 2] == 0
    n_games = len({(int(s), int(i)) for s, i in meta[:, :2]})
    assert n_games >= 4 and int(first.sum()) == n_games
    want = np.load(os.path.join(golden_dir, 'env_abalone_classic_komi.npz'))['init_boards'][0].reshape(81, 4)
    assert (boards[first][:, :, :3] == want[None, :, :3]).all()
    assert set(np.unique(boards[:, 3, 3])) <= {0, 1}
    eng.close()


@pytest.mark.parametrize('tag', ['abalone_v21_german', 'abalone_v21_classic'])
@pytest.mark.parametrize('B', [1, 5, 128])
def test_net_parity(golden_dir, tag, B):
    """AbaloneV21Hip on the two other shipped checkpoints, launched B boards at a time over the 128 golden boards (the classic net's carry
    the komi bit), against the reference module's outputs with the tolerances of tag abalone_v21"""
    import torch
    from azg_amd import nnet
    from test_nnet import assert_net_close
    d = np.load(os.path.join(golden_dir, 'netfwd_%s.npz' % tag))
    n = len(d['boards'])
    assert n == 128 and (tag != 'abalone_v21_classic' or d['boards'].reshape(n, 81, 4)[:, 3, 3].any())
    net = nnet.AbaloneV21Hip(nnet.AbaloneV21.from_npz(os.path.join(golden_dir, 'weights_%s.npz' % tag), device='cuda:0'), max_batch=max(B, 8))
    boards = torch.from_numpy(d['boards'].reshape(n, -1)).to('cuda:0')
    masks = torch.from_numpy(d['masks']).to('cuda:0')
    pis, vs = [], []
    for lo in range(0, n, B):
        pi, v = net.predict_batch(boards[lo:lo + B].contiguous(), masks[lo:lo + B].contiguous())
        pis.append(pi.clone())
        vs.append(v.clone())
    assert_net_close(torch.cat(pis), torch.cat(vs), tag, d)
