"""GPU parity of the Abalone engine net (AbaloneV21Hip: azg_nn_aba21_forward, csrc/nn_abalone.hip.h) against the reference model's
rounding-free forward (netfwd64_abalone_v21.npz) and the plain-torch net, on golden and on engine-made boards; self-play on the shipped
net (pretrained_BelgianDaisy.pt, its stored MCTS arguments); the wrapper's (Abalone, nn_version 21) path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAG = 'abalone_v21'


class Args(dict):
    __getattr__ = dict.get


def _paths(golden_dir):
    return (os.path.join(golden_dir, 'weights_%s.npz' % TAG), np.load(os.path.join(golden_dir, 'netfwd_%s.npz' % TAG)),
            np.load(os.path.join(golden_dir, 'netfwd64_%s.npz' % TAG)))


def _hip(golden_dir, max_batch):
    from azg_amd import nnet
    return nnet.AbaloneV21Hip(nnet.AbaloneV21.from_npz(_paths(golden_dir)[0], device='cuda:0'), max_batch=max_batch)


@pytest.mark.parametrize('B', [1, 7, 203, 4096])
def test_abalone_kernel_matches_reference(golden_dir, B):
    """pi, v within 1e-5 (+ the reference's own f32 - f64 distance) of the f64 forward; invalid actions exactly 0, rows sum to 1; batch
    sizes that are not a multiple of the workgroup's 4 samples"""
    _, d, d64 = _paths(golden_dir)
    n = len(d['boards'])
    idx = np.arange(B) % n
    net = _hip(golden_dir, max_batch=max(B, 8))
    boards = torch.from_numpy(d['boards'][idx].reshape(B, -1)).to('cuda:0')
    masks = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    pi, v = net.predict_batch(boards, masks)
    torch.cuda.synchronize()
    pi, v = pi.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    tol_pi = 1e-5 + np.abs(d['pi'] - d64['pi64']).max()
    tol_v = 1e-5 + np.abs(d['v'] - d64['v64']).max()
    assert np.abs(pi - d64['pi64'][idx]).max() <= tol_pi, np.abs(pi - d64['pi64'][idx]).max()
    assert np.abs(v - d64['v64'][idx]).max() <= tol_v, np.abs(v - d64['v64'][idx]).max()
    assert np.all(pi[d['masks'][idx] == 0] == 0)
    assert np.abs(pi.sum(axis=1) - 1.0).max() <= 1e-5


def test_abalone_kernel_does_not_depend_on_stale_onchip_memory(golden_dir):
    from conftest import poison_onchip
    _, d, _ = _paths(golden_dir)
    net = _hip(golden_dir, max_batch=256)
    reps = -(-203 // len(d['boards']))
    boards = torch.from_numpy(np.concatenate([d['boards']] * reps)[:203].reshape(203, -1)).to('cuda:0')
    masks = torch.from_numpy(np.concatenate([d['masks']] * reps)[:203]).to('cuda:0')
    outs = []
    for pattern in (0x0, 0xFFFFFFFF, 0x7FC00000, 0xA5A5A5A5):
        poison_onchip(pattern)
        pi, v = net.predict_batch(boards, masks)
        outs.append((pi.clone(), v.clone()))
    for pi, v in outs[1:]:
        assert torch.equal(pi, outs[0][0]) and torch.equal(v, outs[0][1])


def _args(golden_dir):
    z = np.load(_paths(golden_dir)[0])
    return Args(numMCTSSims=50, cpuct=float(z['arg/cpuct']), fpu=float(z['arg/fpu']), universes=int(z['arg/universes']), forced_playouts=True,
                prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0.0, temperature=[1.25, 0.8, 1.0], tempThreshold=4)


def _late_boards(golden_dir, T):
    """T canonical boards of the golden env trajectories in their last rounds (round 112..126 of the 127-round limit, nobody at 6 yet):
    games that end within 15 plies, with late-game metadata"""
    c = np.load(os.path.join(golden_dir, 'env_abalone.npz'))['canonical']
    c = c.reshape(len(c), 81, 4)
    sel = np.nonzero((c[:, 2, 3] >= 112) & (c[:, 2, 3] < 127) & (c[:, 0, 3] < 6) & (c[:, 1, 3] < 6))[0]
    assert len(sel) >= 8
    return torch.from_numpy(np.ascontiguousarray(c[np.resize(sel, T)].reshape(T, -1))).to('cuda:0').to(torch.int8)


def test_selfplay_with_the_shipped_abalone_net(golden_dir):
    """SelfPlayEngine on the one-launch kernel (HIP graph on and off) and on the same weights as torch ops, from late-game boards: no
    engine errors, valid trees, finished games whose examples carry finite masked normalised pi, the same pace of play; on the boards
    the engine made (its last leaf batch and the drained examples) the kernel agrees with the torch net within 1e-5"""
    from azg_amd import games, nnet
    from azg_amd.selfplay import SelfPlayEngine
    a = _args(golden_dir)
    T = 64
    init = _late_boards(golden_dir, T)
    plies = []
    made = None
    for kind in ('hip_graph', 'hip', 'torch'):
        g = games.AbaloneGame()
        base = nnet.AbaloneV21.from_npz(_paths(golden_dir)[0], device='cuda:0')
        net = base if kind == 'torch' else nnet.AbaloneV21Hip(base, max_batch=T)
        eng = SelfPlayEngine(g, net, a, n_games=T, node_capacity=2048, max_examples=T * 256, use_graph=(kind == 'hip_graph'))
        eng.start(init_boards=init.clone())
        eng.run(16 * 50)
        torch.cuda.synchronize()
        st = eng.stats()
        assert st['errors'] == 0 and st['plies'] >= 3 * T and st['games'] >= 1, st
        assert sum(grp.f.validate() for grp in eng.groups) == 0
        boards, pi, zz, valids, q, meta = eng.drain_examples(symmetries=False)
        pi_np, va_np = torch.as_tensor(pi).cpu().numpy(), torch.as_tensor(valids).cpu().numpy()
        assert len(pi_np) > 0
        assert np.all(np.isfinite(pi_np)) and np.all(pi_np[va_np == 0] == 0) and np.allclose(pi_np.sum(axis=1), 1.0, atol=1e-5)
        if kind == 'hip':
            f = eng.groups[0].f
            made = (torch.cat([f.leaf_states.clone(), torch.as_tensor(boards).to('cuda:0').to(torch.int8).reshape(-1, f.leaf_states.shape[1])]),
                    torch.cat([f.leaf_valid.clone(), torch.as_tensor(valids).to('cuda:0').to(torch.uint8)]))
        plies.append(st['plies'])
        for grp in eng.groups:
            grp.f.close()
    assert abs(plies[0] - plies[2]) <= T and abs(plies[1] - plies[2]) <= T, plies
    boards, valids = made
    B = min(len(boards), 2048)
    boards, valids = boards[:B].contiguous(), valids[:B].contiguous()
    assert int(boards.reshape(B, 81, 4)[:, 2, 3].max()) >= 112
    base = nnet.AbaloneV21.from_npz(_paths(golden_dir)[0], device='cuda:0')
    p1, v1 = nnet.AbaloneV21Hip(base, max_batch=B).predict_batch(boards, valids)
    p2, v2 = base.predict_batch(boards, valids)
    assert float((p1 - p2).abs().max()) <= 1e-5 and float((v1 - v2).abs().max()) <= 1e-5


def test_wrapper_runs_abalone_v21_on_the_engine_kernel(golden_dir, tmp_path):
    """NNetWrapper(AbaloneGame(), nn_version=21): load_checkpoint of a checkpoint in the reference's layout (state_dict + embedded args),
    predict on the golden vectors, evaluator() is the one-launch kernel; Coach builds on the bare trainable module"""
    from azg_amd import games, nnet, train
    from azg_amd.coach import Coach
    from azg_amd.nnet_wrapper import NNetWrapper
    w_path, d, d64 = _paths(golden_dir)
    z = np.load(w_path)
    ck = {'state_dict': {k[3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith('sd/')}}
    ck.update({k[4:]: z[k].item() for k in z.files if k.startswith('arg/') and z[k].ndim == 0})
    torch.save(ck, str(tmp_path / 'belgian.pt'))
    g = games.AbaloneGame()
    w = NNetWrapper(g, dict(nn_version=21, learn_rate=1e-3, batch_size=64, epochs=1, dropout=0.0))
    assert isinstance(w.nnet, train.AbaloneV21Module)
    assert w.load_checkpoint(str(tmp_path), 'belgian.pt') is not None and not getattr(w, 'requestKnowledgeTransfer', False)
    assert isinstance(w.evaluator(8), nnet.AbaloneV21Hip)
    for i in (0, 5, 77):
        pi, v = w.predict(d['boards'][i], d['masks'][i])
        assert np.abs(pi - d64['pi64'][i]).max() <= 1e-5 + np.abs(d['pi'] - d64['pi64']).max()
        assert np.abs(v - d64['v64'][i]).max() <= 1e-5 + np.abs(d['v'] - d64['v64']).max()
    args = Args(numMCTSSims=8, cpuct=1.5, fpu=0.1, universes=1, forced_playouts=False, dirichletAlpha=0.0, prob_fullMCTS=1.0, ratio_fullMCTS=5,
                temperature=[1.25, 0.8, 1.0], tempThreshold=6, numIters=1, numEps=8, numItersHistory=2, maxlenOfQueue=100000, learn_rate=1e-3,
                batch_size=64, epochs=1, q_weight=0.5, arenaCompare=8, updateThreshold=0.6, checkpoint=str(tmp_path))
    c = Coach(g, train.AbaloneV21Module(), args, n_games=8, node_capacity=1024, log=lambda s: None)
    assert isinstance(c.nnet, NNetWrapper) and isinstance(c.nnet.evaluator(8), nnet.AbaloneV21Hip)
