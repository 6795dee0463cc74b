"""The shipped MobileNet-1d checkpoints of every player count on the CPU: Splendor 3p (V80), Minivilles 3 / 4p (V82) and The Little
Prince 4 / 5p (V83).  The plain-torch net and the trainable modules against the reference model's f64 forward (netfwd64_<tag>.npz on
the boards of netfwd_<tag>.npz, tools/convert_ckpt.py), dropout and one training step of the modules, the wrapper's game/version
mapping, the geometry table against include/azg.h, and the resources of the new k_mb1d_net instantiations in the built library."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB, LLVM, kernel_notes

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
HEADER = os.path.join(os.path.dirname(__file__), '..', 'include', 'azg.h')
NEW_TAGS = ['splendor3_v80', 'minivilles3_v82', 'minivilles4_v82', 'tlp4_v83', 'tlp5_v83']
# (module class name, players, fixture tag) of every shipped V82 / V83 checkpoint
MODULES = [('MinivillesV82Module', 2, 'minivilles2_v82'), ('MinivillesV82Module', 3, 'minivilles3_v82'),
           ('MinivillesV82Module', 4, 'minivilles4_v82'), ('TLPV83Module', 3, 'tlp3_v83'), ('TLPV83Module', 4, 'tlp4_v83'),
           ('TLPV83Module', 5, 'tlp5_v83')]
# the geometries this family's kernel gained, and their AZG_NET_* names
NEW_GEOMETRY = {(2, 78): 'AZG_NET_MINIVILLES3', (2, 98): 'AZG_NET_MINIVILLES4', (15, 73): 'AZG_NET_TLP4', (15, 91): 'AZG_NET_TLP5'}
OLD_GEOMETRY = {(7, 56): 0, (7, 71): 1, (7, 88): 2, (6, 23): 3, (2, 58): 4, (15, 55): 5}
# VGPR budget of the new instantiations: at most 168 keeps 3 waves of the 768-thread workgroup on every SIMD
VGPR_BUDGET = 168


def _sd(tag):
    """the shipped state_dict; for Minivilles 4p, whose weights are too large to keep, the stand-in weights of the same shapes
    (weightstats_minivilles4_v82.npz) that its forward vectors were computed with by the reference's module"""
    from azg_amd import formats
    return {k: torch.from_numpy(v) for k, v in formats.fixture_state_dict(ROOT, tag)[0].items()}


def _ref(tag):
    d, d64 = np.load(os.path.join(ROOT, 'netfwd_%s.npz' % tag)), np.load(os.path.join(ROOT, 'netfwd64_%s.npz' % tag))
    return d['boards'], d['masks'], d64['pi64'], d64['v64']


def assert_matches_f64(pi, v, masks, pi64, v64):
    pi, v = np.asarray(pi, dtype=np.float64), np.asarray(v, dtype=np.float64)
    assert np.abs(pi - pi64).max() <= 1e-5, np.abs(pi - pi64).max()
    assert np.abs(v - v64).max() <= 1e-5, np.abs(v - v64).max()
    some = masks.any(axis=1)            # (finished TLP games have no valid move: every logit is -1e8 and pi is uniform, as the reference's)
    assert np.all(pi[some][masks[some] == 0] == 0)


def _module(name, P, tag, dropout=0.0):
    from azg_amd import train
    A = _ref(tag)[1].shape[1]
    m = getattr(train, name)(P, A, dropout)
    m.load_state_dict(_sd(tag), strict=True)
    return m


@pytest.mark.parametrize('tag', NEW_TAGS)
def test_mobilenet1d_torch_matches_reference_f64(tag):
    from azg_amd import nnet
    boards, masks, pi64, v64 = _ref(tag)
    net = nnet.MobileNet1d(_sd(tag), device='cpu')
    assert (net.nb_vect * net.L, net.A) == (boards[0].size, masks.shape[1])
    pi, v = net.predict_batch(torch.from_numpy(boards).reshape(len(boards), -1), torch.from_numpy(masks))
    assert_matches_f64(pi.numpy(), v.numpy(), masks, pi64, v64)


@pytest.mark.parametrize('name,P,tag', MODULES, ids=[t for _, _, t in MODULES])
def test_module_loads_shipped_checkpoint_and_matches_reference(name, P, tag):
    boards, masks, pi64, v64 = _ref(tag)
    m = _module(name, P, tag).eval()
    assert m.version == (82 if name.startswith('Minivilles') else 83) and (m.P, m.C) == (P, boards[0].shape[0])
    with torch.no_grad():
        lp, v = m(torch.from_numpy(boards).reshape(len(boards), -1), torch.from_numpy(masks))
    assert_matches_f64(torch.exp(lp).numpy(), v.numpy(), masks, pi64, v64)


@pytest.mark.parametrize('name,P,tag', MODULES, ids=[t for _, _, t in MODULES])
def test_module_dropout_acts_in_training_mode_only(name, P, tag):
    boards, masks, _, _ = _ref(tag)
    x, va = torch.from_numpy(boards[:16]).reshape(16, -1), torch.from_numpy(masks[:16])
    with torch.no_grad():
        ref = _module(name, P, tag).eval()(x, va)
        torch.manual_seed(0)
        m = _module(name, P, tag, dropout=0.3).train()
        # (BatchNorm in training mode normalises with the batch statistics: compare against the same module's dropout-free pass)
        m.dropout = 0.0
        no_drop = m(x, va)
        m.dropout = 0.3
        drop = m(x, va)
        ev = _module(name, P, tag, dropout=0.3).eval()(x, va)
    assert not torch.allclose(drop[1], no_drop[1]) and not torch.allclose(drop[0], no_drop[0])
    assert torch.equal(ev[0], ref[0]) and torch.equal(ev[1], ref[1])
    m0 = _module(name, P, tag, dropout=0.0).train()
    with torch.no_grad():
        a, b = m0(x, va), m0(x, va)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('name,P,tag', MODULES, ids=[t for _, _, t in MODULES])
def test_module_train_step(name, P, tag):
    from azg_amd import train
    boards, masks, pi64, _ = _ref(tag)
    n = 64
    rng = np.random.default_rng(P)
    m = _module(name, P, tag, dropout=0.1)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    z = rng.uniform(-1, 1, size=(n, P)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(n, P)).astype(np.float32)
    pi = pi64[:n].astype(np.float32)
    hist = train.train(m, (boards[:n].reshape(n, -1), pi, z, masks[:n], q), batch_size=32, epochs=1, device='cpu', seed=0)
    assert len(hist) == 2 and np.all(np.isfinite(np.asarray(hist, dtype=np.float64)))
    after = m.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k.endswith('weight'))


def test_wrapper_maps_v82_v83_to_their_modules():
    """(Minivilles, 82) for 2-4 players and (The Little Prince, 83) for 3-5 players -> the trainable modules; the games' other versions
    stay unbuilt, and neither game has a default version"""
    from azg_amd import _lib, nnet_wrapper, train
    for name, P, tag in MODULES:
        gid, ver = (_lib.MINIVILLES, 82) if name.startswith('Minivilles') else (_lib.TLP, 83)
        A = _ref(tag)[1].shape[1]
        g = SimpleNamespace(GAME_ID=gid, P=P, A=A, variant=P, device=torch.device('cpu'))
        m = nnet_wrapper._module_for(g, ver, 0.0)
        assert type(m) is getattr(train, name) and m.version == ver and (m.P, m.A) == (P, A)
        m.load_state_dict(_sd(tag), strict=True)
        for other in ((80, 81, 83) if gid == _lib.MINIVILLES else (80, 81, 82)):
            with pytest.raises(ValueError):
                nnet_wrapper._module_for(g, other, 0.0)
        assert (gid, P) not in nnet_wrapper._DEFAULT_VERSION


def _header_enum():
    src = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r'\b(AZG_NET_\w+)\s*=\s*(\d+)', src)}


def test_geometry_table_matches_header():
    from azg_amd import nnet
    enum = _header_enum()
    for lc, name in NEW_GEOMETRY.items():
        assert nnet.MB1D_GEOMETRY[lc] == enum[name], (lc, name)
    for lc, gid in OLD_GEOMETRY.items():
        assert nnet.MB1D_GEOMETRY[lc] == gid
    assert len(nnet.MB1D_GEOMETRY) == len(set(nnet.MB1D_GEOMETRY.values())) == 10
    for tag in NEW_TAGS:
        sd = _sd(tag)
        lc = (int(sd['trunk.0.depthwise.linear.weight'].shape[0]), int(sd['first_layer.linear.weight'].shape[0]))
        assert lc in nnet.MB1D_GEOMETRY, (tag, lc)


def _mb1d_lds(args):
    """Mb1dCfg<...>::LDS_FLOATS * 4 (csrc/nn_mb1d.hip.h) from the template arguments"""
    L, C, NS, A, P, E0, E1, E2, Q0, Q1, Q2, CO1 = args[:12]
    r16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
    ROWSP = r16(NS * L)
    XS, OS, HS, QS, AS = r16(C) + 4, r16(max(CO1, C)) + 4, r16(max(E0, E1, E2)) + 28, r16(max(Q0, Q1, Q2)) + 4, r16(A) + 4
    sc_rows = ROWSP // L + 1
    pl_rows = max(NS, 16 - sc_rows)
    ks_pi = 1 if r16(A) // 16 >= 12 else 12 // (r16(A) // 16)
    head = max((ks_pi + 1) * 16 * AS, 12 * 16 * 20)
    wd = 64 if L * L <= 64 else L * ((L + 3) // 4 * 4)
    return 4 * (ROWSP * max(XS, OS) + ROWSP * XS + max(ROWSP * HS, head) + pl_rows * HS + sc_rows * HS + 16 * QS + wd)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)), reason='needs the ROCm LLVM tools and the built library')
def test_new_mb1d_instantiations_have_no_spills_and_fit():
    k = kernel_notes(LIB)
    found = {}
    for n, r in k.items():
        m = re.search(r'k_mb1d_net<azg::Mb1dCfg<([-\d, ]+)>, (true|false)>', n)
        if not m:
            continue
        args = [int(a) for a in m.group(1).split(',')]
        if (args[0], args[1]) in NEW_GEOMETRY:
            found[(args[0], args[1], m.group(2))] = (args, r)
    assert len(found) == 8, sorted(found)
    for key, (args, r) in found.items():
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, (key, r)
        assert 0 < r['vgpr'] <= VGPR_BUDGET, (key, r)
        assert _mb1d_lds(args) <= 160 * 1024, (key, _mb1d_lds(args))
