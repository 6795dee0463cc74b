"""GPU parity of the Botanik engine nets (BotanikV1xHip: azg_nn_bot_forward, csrc/nn_botanik.hip.h) for nn_version 10 and 11 against the
reference model's rounding-free forward on the stand-in weights (netfwd64_botanik_v1x.npz, netfwdrand_botanik_v1x.npz) and the
plain-torch net, on golden, random and engine-made boards; self-play on BotanikGame; the wrapper's (Botanik, 10 | 11) path and Coach."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
VERSIONS = (10, 11)
NS = 8   # samples per workgroup (BOT_NS, nn_botanik.hip.h)


class Args(dict):
    __getattr__ = dict.get


def _sd(golden_dir, version):
    from azg_amd import formats
    sd, _ = formats.fixture_state_dict(golden_dir, 'botanik_v%d' % version)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _data(golden_dir, version):
    tag = 'botanik_v%d' % version
    return tuple(np.load(os.path.join(golden_dir, '%s_%s.npz' % (n, tag))) for n in ('netfwd', 'netfwd64', 'netfwdrand'))


def _base(golden_dir, version):
    from azg_amd import nnet
    return nnet.BotanikV1x(_sd(golden_dir, version), device='cuda:0')


def _check(pi, v, masks, p32, v32, p64, v64, idx):
    pi, v = pi.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    assert np.abs(pi - p64[idx]).max() <= 1e-5 + np.abs(p32 - p64).max(), np.abs(pi - p64[idx]).max()
    assert np.abs(v - v64[idx]).max() <= 1e-5 + np.abs(v32 - v64).max(), np.abs(v - v64[idx]).max()
    some = masks.any(axis=1)        # (a board without a valid move, as some of the golden ones: every logit is -1e8, pi uniform, as the reference's)
    assert np.all(pi[some][masks[some] == 0] == 0)
    assert np.abs(pi.sum(axis=1) - 1.0).max() <= 1e-5


def _inputs(d, idx):
    return (torch.from_numpy(d['boards'][idx].reshape(len(idx), -1)).to('cuda:0'), torch.from_numpy(d['masks'][idx]).to('cuda:0'))


@pytest.mark.parametrize('version', VERSIONS)
@pytest.mark.parametrize('B', [1, NS - 1, NS, NS + 1, 128, 4096])
def test_botanik_kernel_matches_reference(golden_dir, version, B):
    """pi, v within 1e-5 (+ the reference's own f32 - f64 distance) of the f64 forward; invalid actions exactly 0, rows sum to 1"""
    from azg_amd import nnet
    d, d64, _ = _data(golden_dir, version)
    idx = np.arange(B) % len(d['boards'])
    net = nnet.BotanikV1xHip(_base(golden_dir, version), max_batch=B)
    assert net.n_mach == version - 9
    pi, v = net.predict_batch(*_inputs(d, idx))
    torch.cuda.synchronize()
    _check(pi, v, d['masks'][idx], d['pi'], d['v'], d64['pi64'], d64['v64'], idx)


@pytest.mark.parametrize('version', VERSIONS)
def test_botanik_kernel_matches_reference_on_random_boards(golden_dir, version):
    from azg_amd import nnet
    _, _, r = _data(golden_dir, version)
    B = len(r['boards'])
    net = nnet.BotanikV1xHip(_base(golden_dir, version), max_batch=B)
    pi, v = net.predict_batch(*_inputs(r, np.arange(B)))
    torch.cuda.synchronize()
    _check(pi, v, r['masks'], r['pi'], r['v'], r['pi64'], r['v64'], np.arange(B))


def test_botanik_kernel_does_not_depend_on_stale_onchip_memory(golden_dir):
    """the same outputs, bit for bit, after a forward of the other version, after a larger batch, and under the four poison patterns"""
    from conftest import poison_onchip
    from azg_amd import nnet
    nets = {ver: nnet.BotanikV1xHip(_base(golden_dir, ver), max_batch=4096) for ver in VERSIONS}
    d = {ver: _data(golden_dir, ver)[0] for ver in VERSIONS}
    idx = np.arange(203) % 128
    big = np.arange(4096) % 128
    for ver in VERSIONS:
        other = 21 - ver
        inp = _inputs(d[ver], idx)
        outs = []
        for prior in ('none', 'other', 'big', 0x0, 0xFFFFFFFF, 0x7FC00000, 0xA5A5A5A5):
            if prior == 'other':
                nets[other].predict_batch(*_inputs(d[other], big))
            elif prior == 'big':
                nets[ver].predict_batch(*_inputs(d[ver], big[::-1].copy()))
            elif prior != 'none':
                poison_onchip(prior)
            pi, v = nets[ver].predict_batch(*inp)
            outs.append((pi.clone(), v.clone()))
        for pi, v in outs[1:]:
            assert torch.equal(pi, outs[0][0]) and torch.equal(v, outs[0][1])


def test_botanik_kernel_rejects_bad_arguments():
    """n_mach outside {1, 2}, (P, A) other than (2, 428), B <= 0 or a null pointer is an error before any launch; nothing is written"""
    import ctypes as C
    from azg_amd import _lib
    L = _lib.lib()
    z = torch.zeros(4096, dtype=torch.float32, device='cuda:0')
    out = torch.full((64,), 7.0, dtype=torch.float32, device='cuda:0')
    p, po = C.c_void_p(z.data_ptr()), C.c_void_p(out.data_ptr())
    ptrs = (C.c_void_p * 10)(*([z.data_ptr()] * 10))
    for n_mach, P, A, B in ((0, 2, 428, 1), (3, 2, 428, 1), (1, 3, 428, 1), (2, 2, 427, 1), (1, 2, 428, 0), (2, 2, 428, -1)):
        assert L.azg_nn_bot_forward(p, p, ptrs, n_mach, P, A, B, po, po, None) != 0
    assert L.azg_nn_bot_forward(None, p, ptrs, 1, 2, 428, 1, po, po, None) != 0
    assert L.azg_nn_bot_forward(p, p, None, 1, 2, 428, 1, po, po, None) != 0
    assert L.azg_nn_bot_forward(p, p, ptrs, 1, 2, 428, 1, None, po, None) != 0
    bad = (C.c_void_p * 10)(*([z.data_ptr()] * 9 + [None]))
    assert L.azg_nn_bot_forward(p, p, bad, 2, 2, 428, 1, po, po, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize('version', VERSIONS)
def test_selfplay_with_the_botanik_net(golden_dir, version):
    """SelfPlayEngine on BotanikGame with the one-launch kernel (HIP graph on and off) and with the same weights as torch ops: no engine
    errors, valid trees, finite masked normalised pi; on the boards the engine made (its last leaf batch and the drained examples) the
    kernel agrees with the torch net within 1e-5"""
    from azg_amd import games, nnet
    from azg_amd.selfplay import SelfPlayEngine
    a = Args(numMCTSSims=16, cpuct=1.0, fpu=0.0, universes=1, forced_playouts=False, prob_fullMCTS=1.0, ratio_fullMCTS=5,
             dirichletAlpha=0.0, temperature=[1.25, 0.8, 1.0], tempThreshold=6)
    T = 32
    made = None
    for kind in ('hip_graph', 'hip', 'torch'):
        g = games.BotanikGame()
        base = _base(golden_dir, version)
        net = base if kind == 'torch' else nnet.BotanikV1xHip(base, max_batch=T)
        eng = SelfPlayEngine(g, net, a, n_games=T, node_capacity=2048, max_examples=T * 512, use_graph=(kind == 'hip_graph'))
        eng.start()
        eng.run(16 * 40)
        torch.cuda.synchronize()
        st = eng.stats()
        assert st['errors'] == 0 and st['plies'] > 0, st
        assert sum(grp.f.validate() for grp in eng.groups) == 0
        boards, pi, zz, valids, q, meta = eng.drain_examples(symmetries=False)
        pi_np, va_np = torch.as_tensor(pi).cpu().numpy(), torch.as_tensor(valids).cpu().numpy()
        if len(pi_np):
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
    base = _base(golden_dir, version)
    p1, v1 = nnet.BotanikV1xHip(base, max_batch=B).predict_batch(boards, valids)
    p2, v2 = base.predict_batch(boards, valids)
    assert float((p1 - p2).abs().max()) <= 1e-5 and float((v1 - v2).abs().max()) <= 1e-5


@pytest.mark.parametrize('version', VERSIONS)
def test_wrapper_loads_trains_and_evaluates_botanik(golden_dir, tmp_path, version):
    """NNetWrapper(BotanikGame(), nn_version=10 | 11): load_checkpoint of a checkpoint in the reference's layout predicts within 1e-5 of the
    module; after a training step the evaluator is the one-launch kernel on the new weights"""
    from azg_amd import games, nnet, train
    from azg_amd.nnet_wrapper import NNetWrapper, evaluator_for
    d = _data(golden_dir, version)[0]
    torch.save({'state_dict': _sd(golden_dir, version), 'nn_version': version}, str(tmp_path / 'ref.pt'))
    g = games.BotanikGame()
    w = NNetWrapper(g, dict(nn_version=version, learn_rate=1e-3, batch_size=64, epochs=1, dropout=0.1))
    assert type(w.nnet) is (train.BotanikV10Module if version == 10 else train.BotanikV11Module)
    assert w.load_checkpoint(str(tmp_path), 'ref.pt') is not None and not w.requestKnowledgeTransfer
    assert isinstance(w.evaluator(8), nnet.BotanikV1xHip)
    n = len(d['boards'])
    boards = torch.from_numpy(d['boards']).reshape(n, -1).cuda()
    masks = torch.from_numpy(d['masks']).cuda()

    def module_out():
        m = w.nnet.eval()
        with torch.no_grad():
            lp, v = m.to('cuda:0')(boards, masks)
        return torch.exp(lp), v
    pm, vm = module_out()
    pi, v = w.predict_batch(boards, masks)
    assert float((pi - pm).abs().max()) <= 1e-5 and float((v - vm).abs().max()) <= 1e-5
    rng = np.random.default_rng(0)
    ex = (d['boards'].reshape(n, -1), pm.cpu().numpy(), rng.uniform(-1, 1, (n, 2)).astype(np.float32), d['masks'],
          rng.uniform(-1, 1, (n, 2)).astype(np.float32))
    before = {k: t.detach().clone().cpu() for k, t in w.nnet.state_dict().items()}
    hist = w.train(ex)
    assert len(hist) >= 1 and np.all(np.isfinite(np.asarray(hist, dtype=np.float64)))
    assert any(not torch.equal(before[k], t.cpu()) for k, t in w.nnet.state_dict().items() if k.endswith('weight'))
    ev = evaluator_for(w.nnet, g, n)
    assert isinstance(ev, nnet.BotanikV1xHip)
    pm, vm = module_out()
    pi, v = ev.predict_batch(boards, masks)
    assert float((pi - pm).abs().max()) <= 1e-5 and float((v - vm).abs().max()) <= 1e-5


def test_coach_learn_botanik_v10_one_iteration(golden_dir, tmp_path):
    """Coach.learn on Botanik from the bare V10 module with the stand-in weights: engine self-play on the one-launch net, training, arena
    gate -- one iteration end to end"""
    from azg_amd import games, nnet, train
    from azg_amd.coach import Coach
    g = games.BotanikGame()
    m = train.BotanikV10Module(2, g.A)
    m.load_state_dict(_sd(golden_dir, 10), strict=True)
    args = Args(numMCTSSims=8, cpuct=1.0, fpu=0.1, universes=1, forced_playouts=False, dirichletAlpha=-1, prob_fullMCTS=1.0,
                ratio_fullMCTS=5, temperature=[1.25, 0.8, 1.0], tempThreshold=4, numIters=1, numEps=8, numItersHistory=2,
                maxlenOfQueue=100000, learn_rate=1e-3, batch_size=64, epochs=1, q_weight=0.5, arenaCompare=4,
                updateThreshold=0.6, checkpoint=str(tmp_path))
    c = Coach(g, m, args, n_games=16, node_capacity=2048, log=lambda s: None)
    assert isinstance(c.nnet.evaluator(8), nnet.BotanikV1xHip)
    res = c.learn()
    assert len(res) == 1 and res[0]["nwins"] + res[0]["pwins"] + res[0]["draws"] == 4 and res[0]["examples"] > 0
    ck = torch.load(os.path.join(tmp_path, 'temp.pt'), map_location='cpu', weights_only=False)
    assert ck['full_model'].version == 10 and set(ck['state_dict'].keys()) == set(m.state_dict().keys())
