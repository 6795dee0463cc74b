"""GPU: the one-launch MobileNet-1d kernel (k_mb1d_net, csrc/nn_mb1d.hip.h) on the shipped checkpoints it gained -- Minivilles 3 / 4p,
The Little Prince 4 / 5p -- and on the Splendor 3p weights: parity with the reference model's f64 forward at batch sizes around the
per-workgroup sample count NS and at 4096 leaves, independence from a previous geometry's LDS contents, the unknown-geometry error,
self-play on the shipped nets, and NNetWrapper / Coach on the V82 / V83 modules."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tag -> (samples per workgroup NS of its Mb1dCfg, AZG_NET_* id)
GEOM = {'splendor3_v80': (8, 1), 'minivilles3_v82': (16, 6), 'minivilles4_v82': (16, 7), 'tlp4_v83': (6, 8), 'tlp5_v83': (6, 9)}


class Args(dict):
    __getattr__ = dict.get


def _paths(golden_dir, tag):
    """(weights, forward vectors, their f64 values); the Minivilles 4p weights are the stand-in of weightstats_minivilles4_v82.npz
    (azg_amd.formats.fixture_state_dict): the shipped tensors are too large to keep, the forward vectors are the reference module's on
    the stand-in"""
    return tuple(os.path.join(golden_dir, '%s_%s.npz' % (k, tag)) for k in ('weights', 'netfwd', 'netfwd64'))


def _sd(golden_dir, tag):
    from azg_amd import formats
    return {k: torch.from_numpy(v) for k, v in formats.fixture_state_dict(golden_dir, tag)[0].items()}


def _args(golden_dir, tag):
    from azg_amd import formats
    return formats.fixture_state_dict(golden_dir, tag)[1]


def _hip(golden_dir, tag, h2=True, max_batch=4096):
    from azg_amd import nnet
    return nnet.MobileNet1dHip(nnet.MobileNet1d(_sd(golden_dir, tag), device='cuda:0'), max_batch=max_batch, h2=h2)


def _check_rows(pi, v, rows, masks, pi64, v64):
    """rows[i] = the fixture row that output row i evaluated: <= 1e-5 of the reference's f64 forward, masked entries exactly 0"""
    pi, v = pi.double().cpu().numpy(), v.double().cpu().numpy()
    assert np.abs(pi - pi64[rows]).max() <= 1e-5, np.abs(pi - pi64[rows]).max()
    assert np.abs(v - v64[rows]).max() <= 1e-5, np.abs(v - v64[rows]).max()
    m = masks[rows]
    some = m.any(axis=1)                 # (finished TLP games have no valid move: pi is uniform there, as the reference's)
    assert np.all(pi[some][m[some] == 0] == 0)


@pytest.mark.parametrize('h2', [True, False], ids=['h2', 'f32'])
@pytest.mark.parametrize('tag', list(GEOM))
def test_kernel_matches_reference_f64(golden_dir, tag, h2):
    _, d_path, d64_path = _paths(golden_dir, tag)
    d, d64 = np.load(d_path), np.load(d64_path)
    NS, gid = GEOM[tag]
    net = _hip(golden_dir, tag, h2=h2)
    assert net.fused and net.geometry == gid
    boards, masks = torch.from_numpy(d['boards']).reshape(len(d['boards']), -1).cuda(), torch.from_numpy(d['masks']).cuda()
    n = len(boards)
    for B in sorted({1, NS - 1, NS, NS + 1, 128}):
        rows = np.arange(B) % n
        pi, v = net.predict_batch(boards[rows].contiguous(), masks[rows].contiguous())
        _check_rows(pi, v, rows, d['masks'], d64['pi64'], d64['v64'])
    rows = np.random.default_rng(1).integers(0, n, size=4096)             # 4096 leaves: the fixture rows tiled in a random order
    pi, v = net.predict_batch(boards[rows].contiguous(), masks[rows].contiguous())
    torch.cuda.synchronize()
    _check_rows(pi, v, rows, d['masks'], d64['pi64'], d64['v64'])


@pytest.mark.parametrize('h2', [True, False], ids=['h2', 'f32'])
def test_outputs_do_not_depend_on_the_previous_geometry(golden_dir, h2):
    """each new geometry right after a forward of a different one (a different LDS layout in the previous workgroups of every CU) gives
    the bits of its first run"""
    d_other = np.load(_paths(golden_dir, 'tlp3_v83')[1])
    other = _hip(golden_dir, 'tlp3_v83', h2=h2, max_batch=512)
    ob = torch.from_numpy(d_other['boards']).reshape(len(d_other['boards']), -1).cuda()
    om = torch.from_numpy(d_other['masks']).cuda()
    oi = np.arange(512) % len(ob)
    for tag in ('minivilles3_v82', 'minivilles4_v82', 'tlp4_v83', 'tlp5_v83'):
        d = np.load(_paths(golden_dir, tag)[1])
        net = _hip(golden_dir, tag, h2=h2, max_batch=512)
        rows = np.arange(512) % len(d['boards'])
        b = torch.from_numpy(d['boards']).reshape(len(d['boards']), -1)[rows].contiguous().cuda()
        m = torch.from_numpy(d['masks'])[rows].contiguous().cuda()
        cold = [t.clone() for t in net.predict_batch(b, m)]
        other.predict_batch(ob[oi].contiguous(), om[oi].contiguous())
        warm = net.predict_batch(b, m)
        torch.cuda.synchronize()
        assert torch.equal(cold[0], warm[0]) and torch.equal(cold[1], warm[1]), tag


def test_unknown_geometry_is_an_error_and_launches_nothing(golden_dir):
    from azg_amd import _lib
    net = _hip(golden_dir, 'tlp5_v83', max_batch=16)
    d = np.load(_paths(golden_dir, 'tlp5_v83')[1])
    b = torch.from_numpy(d['boards'][:16]).reshape(16, -1).contiguous().cuda()
    m = torch.from_numpy(d['masks'][:16]).contiguous().cuda()
    pi = torch.full((16, 25), 7.0, device='cuda:0')
    v = torch.full((16, 5), 7.0, device='cuda:0')
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.azg_nn_mb1d_forward(10, p(b), p(m), net.fused_ptrs, 16, p(pi), p(v), st) != 0
    assert L.azg_nn_mb1d_forward_h2(10, p(b), p(m), net.fused_ptrs_h2, net.descale_h2, 16, p(pi), p(v), st) != 0
    torch.cuda.synchronize()
    assert bool((pi == 7.0).all()) and bool((v == 7.0).all())


@pytest.mark.parametrize('game,P,tag', [('minivilles', 3, 'minivilles3_v82'), ('minivilles', 4, 'minivilles4_v82'), ('tlp', 4, 'tlp4_v83'),
                                        ('tlp', 5, 'tlp5_v83')])
def test_selfplay_with_the_shipped_net(golden_dir, game, P, tag):
    """SelfPlayEngine with the one-launch kernel and with the same weights as torch ops: no engine errors, valid trees, finite masked
    normalised pi, the same pace of play.  (The shipped args of these checkpoints store no `universes`: the reference's default, 1.)"""
    from azg_amd import games, nnet
    from azg_amd.selfplay import SelfPlayEngine
    z = _args(golden_dir, tag)
    universes = int(z['universes']) if 'universes' in z else 1
    a = Args(numMCTSSims=50, cpuct=float(z['cpuct']), fpu=float(z['fpu']), universes=universes, forced_playouts=True,
             prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0.0, temperature=[1.25, 0.8, 1.0], tempThreshold=4)
    T = 64
    out = []
    for engine_net in (True, False):
        g = games.MinivillesGame(P) if game == 'minivilles' else games.TLPGame(P)
        base = nnet.MobileNet1d(_sd(golden_dir, tag), device='cuda:0')
        assert (base.nb_vect * base.L, base.A, base.P) == (g.S, g.A, g.P)
        net = nnet.MobileNet1dHip(base, max_batch=T) if engine_net else base
        eng = SelfPlayEngine(g, net, a, n_games=T, node_capacity=2048, max_examples=T * 256, use_graph=False)
        eng.start()
        eng.run(6 * 50)
        torch.cuda.synchronize()
        st = eng.stats()
        assert st['errors'] == 0 and st['plies'] >= 3 * T, st
        assert sum(grp.f.validate() for grp in eng.groups) == 0
        boards, pi, zz, valids, q, meta = eng.drain_examples(symmetries=False)
        pi, valids = torch.as_tensor(pi).cpu().numpy(), torch.as_tensor(valids).cpu().numpy()
        assert np.all(np.isfinite(pi)) and np.all(pi[valids == 0] == 0) and np.allclose(pi.sum(axis=1), 1.0, atol=1e-5)
        out.append(st['plies'])
        for grp in eng.groups:
            grp.f.close()
    assert abs(out[0] - out[1]) <= T        # the same pace of play with either evaluator


@pytest.mark.parametrize('game,P,tag', [('minivilles', 2, 'minivilles2_v82'), ('minivilles', 3, 'minivilles3_v82'),
                                        ('minivilles', 4, 'minivilles4_v82'), ('tlp', 3, 'tlp3_v83'), ('tlp', 4, 'tlp4_v83'),
                                        ('tlp', 5, 'tlp5_v83')])
def test_wrapper_loads_trains_and_evaluates_v82_v83(golden_dir, tmp_path, game, P, tag):
    """NNetWrapper(game, nn_version=82 | 83): load_checkpoint of a checkpoint in the reference's layout (state_dict + embedded args)
    predicts within 1e-5 of the module; after a training step the evaluator is the one-launch kernel on the new weights"""
    from azg_amd import formats, games, nnet, train
    from azg_amd.nnet_wrapper import NNetWrapper, evaluator_for
    d = np.load(_paths(golden_dir, tag)[1])
    ck = {'state_dict': _sd(golden_dir, tag)}
    ck.update({k: v.item() for k, v in _args(golden_dir, tag).items() if v.ndim == 0})
    torch.save(ck, str(tmp_path / 'ref.pt'))
    sd_read, args_read = formats.load_reference_checkpoint(str(tmp_path / 'ref.pt'))
    assert set(sd_read) == set(ck['state_dict']) and args_read['nn_version'] == (82 if game == 'minivilles' else 83)
    g = games.MinivillesGame(P) if game == 'minivilles' else games.TLPGame(P)
    ver, cls = (82, train.MinivillesV82Module) if game == 'minivilles' else (83, train.TLPV83Module)
    w = NNetWrapper(g, dict(nn_version=ver, learn_rate=1e-3, batch_size=64, epochs=1, dropout=0.1))
    assert type(w.nnet) is cls
    assert w.load_checkpoint(str(tmp_path), 'ref.pt') is not None and not w.requestKnowledgeTransfer
    assert isinstance(w.evaluator(8), nnet.MobileNet1dHip)
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
    for i in (0, 7):
        p1, v1 = w.predict(d['boards'][i], d['masks'][i])
        assert np.abs(p1 - pm[i].cpu().numpy()).max() <= 1e-5 and np.abs(v1 - vm[i].cpu().numpy()).max() <= 1e-5
    rng = np.random.default_rng(0)
    ex = (d['boards'].reshape(n, -1), pm.cpu().numpy(), rng.uniform(-1, 1, (n, P)).astype(np.float32), d['masks'],
          rng.uniform(-1, 1, (n, P)).astype(np.float32))
    before = {k: t.detach().clone().cpu() for k, t in w.nnet.state_dict().items()}
    hist = w.train(ex)
    assert len(hist) >= 1 and np.all(np.isfinite(np.asarray(hist, dtype=np.float64)))
    assert any(not torch.equal(before[k], t.cpu()) for k, t in w.nnet.state_dict().items() if k.endswith('weight'))
    ev = evaluator_for(w.nnet, g, n)
    assert isinstance(ev, nnet.MobileNet1dHip) and ev.fused
    pm, vm = module_out()
    pi, v = ev.predict_batch(boards, masks)
    assert float((pi - pm).abs().max()) <= 1e-5 and float((v - vm).abs().max()) <= 1e-5


def test_coach_learn_minivilles3_one_iteration(golden_dir, tmp_path):
    """Coach.learn on Minivilles 3p from the bare V82 module with the shipped weights: engine self-play on the one-launch net, training,
    arena gate -- one iteration end to end"""
    from azg_amd import games, nnet, train
    from azg_amd.coach import Coach
    g = games.MinivillesGame(3)
    m = train.MinivillesV82Module(3, g.A)
    m.load_state_dict(_sd(golden_dir, 'minivilles3_v82'), strict=True)
    args = Args(numMCTSSims=8, cpuct=1.0, fpu=0.1, universes=1, forced_playouts=False, dirichletAlpha=-1, prob_fullMCTS=1.0,
                ratio_fullMCTS=5, temperature=[1.25, 0.8, 1.0], tempThreshold=4, numIters=1, numEps=8, numItersHistory=2,
                maxlenOfQueue=100000, learn_rate=1e-3, batch_size=64, epochs=1, q_weight=0.5, arenaCompare=4,
                updateThreshold=0.6, checkpoint=str(tmp_path))
    c = Coach(g, m, args, n_games=16, node_capacity=2048, log=lambda s: None)
    assert isinstance(c.nnet.evaluator(8), nnet.MobileNet1dHip)
    res = c.learn()
    assert len(res) == 1 and res[0]["nwins"] + res[0]["pwins"] + res[0]["draws"] == 4 and res[0]["examples"] > 0
    ck = torch.load(os.path.join(tmp_path, 'temp.pt'), map_location='cpu', weights_only=False)
    assert ck['full_model'].version == 82 and set(ck['state_dict'].keys()) == set(m.state_dict().keys())
