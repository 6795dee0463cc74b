"""GPU parity of the Akropolis engine net (AkropolisV31Hip: azg_nn_akr31_forward, csrc/nn_akropolis.hip.h) for 2, 3 and 4 players
against the reference model's rounding-free forward (netfwd64_akropolis*_v31.npz, netfwdrand_akropolis*_v31.npz) and the plain-torch
net, on golden, random and engine-made boards; self-play on the shipped nets (pretrained_{2,3,4}pl.pt, their stored MCTS arguments);
the wrapper's (Akropolis, nn_version 31) path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAGS = {2: 'akropolis_v31', 3: 'akropolis3_v31', 4: 'akropolis4_v31'}


class Args(dict):
    __getattr__ = dict.get


def _paths(golden_dir, P):
    return (os.path.join(golden_dir, 'weights_%s.npz' % TAGS[P]), np.load(os.path.join(golden_dir, 'netfwd_%s.npz' % TAGS[P])),
            np.load(os.path.join(golden_dir, 'netfwd64_%s.npz' % TAGS[P])))


def _base(golden_dir, P):
    from azg_amd import nnet
    return nnet.AkropolisV31.from_npz(_paths(golden_dir, P)[0], num_players=P, device='cuda:0')


@pytest.mark.parametrize('P', [2, 3, 4])
@pytest.mark.parametrize('B', [1, 7, 203, 4096, 4097])
def test_akropolis_kernel_matches_reference(golden_dir, P, B):
    """pi, v within 1e-5 (+ the reference's own f32 - f64 distance) of the f64 forward; invalid actions exactly 0, rows sum to 1"""
    from azg_amd import nnet
    _, d, d64 = _paths(golden_dir, P)
    idx = np.arange(B) % len(d['boards'])
    net = nnet.AkropolisV31Hip(_base(golden_dir, P), max_batch=max(B, 8))
    boards = torch.from_numpy(d['boards'][idx].reshape(B, -1)).to('cuda:0')
    masks = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    pi, v = net.predict_batch(boards, masks)
    torch.cuda.synchronize()
    _check(pi, v, d['masks'][idx], d['pi'], d['v'], d64['pi64'], d64['v64'], idx)


def _check(pi, v, masks, p32, v32, p64, v64, idx, k=1):
    pi, v = pi.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    tol_pi = 1e-5 + k * np.abs(p32 - p64).max()
    tol_v = 1e-5 + k * np.abs(v32 - v64).max()
    assert np.abs(pi - p64[idx]).max() <= tol_pi, np.abs(pi - p64[idx]).max()
    assert np.abs(v - v64[idx]).max() <= tol_v, np.abs(v - v64[idx]).max()
    assert np.all(pi[masks == 0] == 0)
    assert np.abs(pi.sum(axis=1) - 1.0).max() <= 1e-5


@pytest.mark.parametrize('P', [2, 3, 4])
def test_akropolis_kernel_matches_reference_on_random_boards(golden_dir, P):
    """random int8 boards (codes outside 0..11, negative heights and scores), all actions valid.  Scores of +-128 make W_c ~1000x larger
    than on game boards (|W_c| ~5e3 against ~5), so the logits reach the thousands and any f32 evaluation of them is ~1e-4 from their
    exact values: the reference's own f32 pi sits up to 2e-5 from its f64 forward (P = 3, 4).  The kernel's f32 rounding is of the same
    size in another order, so the bound here is 1e-5 plus twice the reference's distance (game boards: once, above)."""
    from azg_amd import nnet
    r = np.load(os.path.join(golden_dir, 'netfwdrand_%s.npz' % TAGS[P]))
    B = len(r['boards'])
    net = nnet.AkropolisV31Hip(_base(golden_dir, P), max_batch=B)
    pi, v = net.predict_batch(torch.from_numpy(r['boards'].reshape(B, -1)).to('cuda:0'), torch.from_numpy(r['masks']).to('cuda:0'))
    torch.cuda.synchronize()
    _check(pi, v, r['masks'], r['pi'], r['v'], r['pi64'], r['v64'], np.arange(B), k=2)


def test_akropolis_kernel_rejects_other_shapes():
    """anything but (P, A) in {(2, 4056), (3, 5070), (4, 6084)}, B <= 0 or a null argument is an error before any launch"""
    import ctypes as C
    from azg_amd import _lib
    net = _lib.lib()
    z = torch.zeros(8, dtype=torch.int64, device='cuda:0')
    p = C.c_void_p(z.data_ptr())
    ptrs = (C.c_void_p * 3)(*([z.data_ptr()] * 3))
    for P, A, B in ((2, 5070, 1), (3, 4056, 1), (5, 7098, 1), (1, 3042, 1), (2, 4056, 0), (4, 6084, -1)):
        assert net.azg_nn_akr31_forward(p, p, ptrs, P, A, B, p, p, None) != 0
    assert net.azg_nn_akr31_forward(None, p, ptrs, 2, 4056, 1, p, p, None) != 0
    assert net.azg_nn_akr31_forward(p, p, (C.c_void_p * 3)(z.data_ptr(), None, z.data_ptr()), 2, 4056, 1, p, p, None) != 0


@pytest.mark.parametrize('P', [2, 4])
def test_akropolis_kernel_does_not_depend_on_stale_onchip_memory(golden_dir, P):
    from conftest import poison_onchip
    from azg_amd import nnet
    _, d, _ = _paths(golden_dir, P)
    net = nnet.AkropolisV31Hip(_base(golden_dir, P), max_batch=256)
    idx = np.arange(203) % len(d['boards'])
    boards = torch.from_numpy(d['boards'][idx].reshape(203, -1)).to('cuda:0')
    masks = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    outs = []
    for pattern in (0x0, 0xFFFFFFFF, 0x7FC00000, 0xA5A5A5A5):
        poison_onchip(pattern)
        pi, v = net.predict_batch(boards, masks)
        outs.append((pi.clone(), v.clone()))
    for pi, v in outs[1:]:
        assert torch.equal(pi, outs[0][0]) and torch.equal(v, outs[0][1])


def _args(golden_dir, P):
    z = np.load(_paths(golden_dir, P)[0])
    return Args(numMCTSSims=16, cpuct=float(z['arg/cpuct']), fpu=float(z['arg/fpu']), universes=int(z['arg/universes']), forced_playouts=False,
                prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0.0, temperature=[1.25, 0.8, 1.0], tempThreshold=6)


@pytest.mark.parametrize('P', [2, 3, 4])
def test_selfplay_with_the_shipped_akropolis_net(golden_dir, P):
    """SelfPlayEngine on the one-launch kernel (HIP graph on and off) and on the same weights as torch ops: no engine errors, valid trees,
    plies played, finished games whose examples carry finite masked normalised pi; on the boards the engine made (its last leaf batch
    and the drained examples) the kernel agrees with the torch net within 1e-5"""
    from azg_amd import games, nnet
    from azg_amd.selfplay import SelfPlayEngine
    a = _args(golden_dir, P)
    T = 32
    made = None
    for kind in ('hip_graph', 'hip', 'torch'):
        g = games.AkropolisGame(P)
        base = _base(golden_dir, P)
        net = base if kind == 'torch' else nnet.AkropolisV31Hip(base, max_batch=T)
        eng = SelfPlayEngine(g, net, a, n_games=T, node_capacity=max(2048, 80 * a.numMCTSSims), max_examples=T * 512,
                             use_graph=(kind == 'hip_graph'))
        eng.start()
        eng.run(16 * 160)
        torch.cuda.synchronize()
        st = eng.stats()
        assert st['errors'] == 0 and st['plies'] > 0 and st['games'] >= 1, st
        assert sum(grp.f.validate() for grp in eng.groups) == 0
        boards, pi, zz, valids, q, meta = eng.drain_examples(symmetries=False)
        pi_np, va_np = torch.as_tensor(pi).cpu().numpy(), torch.as_tensor(valids).cpu().numpy()
        assert len(pi_np) > 0
        assert np.all(np.isfinite(pi_np)) and np.all(pi_np[va_np == 0] == 0) and np.allclose(pi_np.sum(axis=1), 1.0, atol=1e-5)
        if kind == 'hip':
            f = eng.groups[0].f
            made = (torch.cat([f.leaf_states.clone(), torch.as_tensor(boards).to('cuda:0').to(torch.int8).reshape(-1, f.leaf_states.shape[1])]),
                    torch.cat([f.leaf_valid.clone(), torch.as_tensor(valids).to('cuda:0').to(torch.uint8)]))
        for grp in eng.groups:
            grp.f.close()
    boards, valids = made
    B = min(len(boards), 2048)
    boards, valids = boards[:B].contiguous(), valids[:B].contiguous()
    base = _base(golden_dir, P)
    p1, v1 = nnet.AkropolisV31Hip(base, max_batch=B).predict_batch(boards, valids)
    p2, v2 = base.predict_batch(boards, valids)
    assert float((p1 - p2).abs().max()) <= 1e-5 and float((v1 - v2).abs().max()) <= 1e-5


@pytest.mark.parametrize('P', [2, 3, 4])
def test_wrapper_runs_akropolis_v31_on_the_engine_kernel(golden_dir, tmp_path, P):
    """NNetWrapper(AkropolisGame(P), nn_version=31): load_checkpoint of a checkpoint in the reference's layout (state_dict + embedded
    args), predict on the golden vectors, evaluator() is the one-launch kernel; Coach builds on the bare trainable module"""
    from azg_amd import games, nnet, train
    from azg_amd.coach import Coach
    from azg_amd.nnet_wrapper import NNetWrapper
    w_path, d, d64 = _paths(golden_dir, P)
    z = np.load(w_path)
    ck = {'state_dict': {k[3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith('sd/')}}
    ck.update({k[4:]: z[k].item() for k in z.files if k.startswith('arg/') and z[k].ndim == 0})
    torch.save(ck, str(tmp_path / 'akr.pt'))
    g = games.AkropolisGame(P)
    w = NNetWrapper(g, dict(nn_version=31, learn_rate=1e-3, batch_size=64, epochs=1, dropout=0.0))
    assert isinstance(w.nnet, train.AkropolisV31Module)
    assert w.load_checkpoint(str(tmp_path), 'akr.pt') is not None and not getattr(w, 'requestKnowledgeTransfer', False)
    assert isinstance(w.evaluator(8), nnet.AkropolisV31Hip)
    for i in (0, 5, 77):
        pi, v = w.predict(d['boards'][i], d['masks'][i])
        assert np.abs(pi - d64['pi64'][i]).max() <= 1e-5 + np.abs(d['pi'] - d64['pi64']).max()
        assert np.abs(v - d64['v64'][i]).max() <= 1e-5 + np.abs(d['v'] - d64['v64']).max()
    args = Args(numMCTSSims=8, cpuct=1.0, fpu=0.1, universes=1, forced_playouts=False, dirichletAlpha=0.0, prob_fullMCTS=1.0, ratio_fullMCTS=5,
                temperature=[1.25, 0.8, 1.0], tempThreshold=6, numIters=1, numEps=8, numItersHistory=2, maxlenOfQueue=100000, learn_rate=1e-3,
                batch_size=64, epochs=1, q_weight=0.5, arenaCompare=8, updateThreshold=0.6, checkpoint=str(tmp_path))
    c = Coach(g, train.AkropolisV31Module(P, g.A), args, n_games=8, node_capacity=2048, log=lambda s: None)
    assert isinstance(c.nnet, NNetWrapper) and isinstance(c.nnet.evaluator(8), nnet.AkropolisV31Hip)
