"""Akropolis net V31 on the CPU: the plain-torch re-expression and the trainable module against the reference model's own outputs
(netfwd_akropolis*_v31.npz with their f64 values netfwd64_akropolis*_v31.npz, and 16 random int8 boards per player count,
netfwdrand_akropolis*_v31.npz: pretrained_{2,3,4}pl.pt, tools/convert_ckpt.py), the kernel's packed operands, the wrapper's game/version
mapping, and the resources of the engine kernel (k_akr31_net, csrc/nn_akropolis.hip.h) read from the library's code-object notes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_kernel_resources import LIB, LLVM, kernel_notes

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
TAGS = {2: 'akropolis_v31', 3: 'akropolis3_v31', 4: 'akropolis4_v31'}


def _w(P):
    return os.path.join(ROOT, 'weights_%s.npz' % TAGS[P])


def _sd(P):
    z = np.load(_w(P))
    return {k[3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith('sd/')}


def _sets(P):
    """(boards, masks, ref f32 pi, ref f32 v, ref f64 pi, ref f64 v) of the env boards and of the random boards"""
    d, d64 = np.load(os.path.join(ROOT, 'netfwd_%s.npz' % TAGS[P])), np.load(os.path.join(ROOT, 'netfwd64_%s.npz' % TAGS[P]))
    r = np.load(os.path.join(ROOT, 'netfwdrand_%s.npz' % TAGS[P]))
    return {'env': (d['boards'], d['masks'], d['pi'], d['v'], d64['pi64'], d64['v64']),
            'random': (r['boards'], r['masks'], r['pi'], r['v'], r['pi64'], r['v64'])}


def assert_close(pi, v, ref):
    """within 1e-5 plus the reference's own f32 - f64 distance of its f64 forward; invalid actions exactly 0"""
    _, masks, p32, v32, p64, v64 = ref
    pi, v = pi.detach().cpu().numpy().astype(np.float64), v.detach().cpu().numpy().astype(np.float64)
    assert np.abs(pi - p64).max() <= 1e-5 + np.abs(p32 - p64).max(), np.abs(pi - p64).max()
    assert np.abs(v - v64).max() <= 1e-5 + np.abs(v32 - v64).max(), np.abs(v - v64).max()
    assert np.all(pi[masks == 0] == 0)


@pytest.mark.parametrize('P', [2, 3, 4])
@pytest.mark.parametrize('kind', ['env', 'random'])
def test_akropolis_v31_torch_matches_reference(P, kind):
    from azg_amd import nnet
    ref = _sets(P)[kind]
    net = nnet.AkropolisV31.from_npz(_w(P), num_players=P, device='cpu')
    assert (net.S, net.A, net.CS) == (169 * (3 * P + 2), 1014 * (P + 2), P + 2)
    boards = ref[0]
    if kind == 'random':       # codes outside 0..11, negative heights and scores: the clamp and the int8 handling
        assert boards.min() < 0 and boards.max() > 11
    pi, v = net.predict_batch(torch.from_numpy(boards).reshape(len(boards), -1), torch.from_numpy(ref[1]))
    assert_close(pi, v, ref)
    p1, v1 = net.predict(boards[3], ref[1][3])
    assert np.abs(p1 - ref[4][3]).max() <= 1e-5 + np.abs(ref[2] - ref[4]).max() and np.abs(v1 - ref[5][3]).max() <= 1e-5


@pytest.mark.parametrize('P', [2, 3, 4])
def test_akropolis_v31_module_loads_the_shipped_state_dict(P):
    from azg_amd import train
    m = train.AkropolisV31Module(P, 1014 * (P + 2))
    m.load_state_dict(_sd(P), strict=True)
    m.eval()
    for ref in _sets(P).values():
        with torch.no_grad():
            lp, v = m(torch.from_numpy(ref[0]), torch.from_numpy(ref[1]).bool())
        assert_close(torch.exp(lp), v, ref)


@pytest.mark.parametrize('P', [2, 4])
def test_akropolis_v31_module_applies_dropout_in_training(P):
    from azg_amd import train
    ref = _sets(P)['env']
    m = train.AkropolisV31Module(P, 1014 * (P + 2), dropout=0.3)
    m.load_state_dict(_sd(P), strict=True)
    b, va = torch.from_numpy(ref[0][:8]), torch.from_numpy(ref[1][:8]).bool()
    m.train()
    torch.manual_seed(0)
    a = m(b, va)[0]
    torch.manual_seed(1)
    assert not torch.equal(a, m(b, va)[0])
    m.eval()
    assert torch.equal(m(b, va)[0], m(b, va)[0])


def _emulate_kernel(blocks, boards, valids, P):
    """the kernel's arithmetic written out in torch (f64) from the three packed blocks: conv1 from the per-tap code tables and the
    height / tileID columns, conv2 per tap, proj_p's first 1x1 as the per-player board products plus the per-sample constant c0, the SE
    over the cells, the policy as p . W_c with W_c[o][r] = a[r] h[16 o + r], and the value head"""
    from azg_amd import nnet
    w = {k: t.double() for k, t in nnet.AkropolisV31Hip.unpack(blocks, P).items()}
    CS, C = P + 2, 3 * P + 2
    B = boards.shape[0]
    x = boards.reshape(B, 13, 13, C).long()
    hs = F.hardswish
    code = lambda t: t.clamp(0, 11)  # noqa: E731
    s1 = x[:, 0:3 * P, 0:5, 3 * P].reshape(B, 15 * P).double() @ w['ws'] + w['bs']
    g1 = hs(x[:, CS + 1, 0:2, 3 * P + 1].double() @ w['wg'] + w['bg'])
    cc = code(x[:, 0:CS, 0:3, 3 * P + 1])                                                   # [B][CS][3]
    t = hs(sum(w['tc'][k][cc[..., k]] for k in range(3)) + w['bc'])                         # [B][CS][32]
    f3 = torch.cat([t, s1[:, None].expand(B, CS, 16), g1[:, None].expand(B, CS, 8)], dim=2)
    a = hs(f3 @ w['wi'] + w['bi'])
    h = f3 @ w['wo'] + w['bo']
    wc = (a.repeat(1, 1, 6) * h).view(B, CS, 6, 16)                                         # W_c [c][o][r]
    c0 = torch.cat([s1, g1], dim=1) @ w['wec'] + w['be']
    e = c0[:, None, None, :].expand(B, 13, 13, 32).clone()
    for i in range(P):
        pad = lambda z: F.pad(z, (0, 0, 1, 1, 1, 1))  # noqa: E731             # zero border of the [B][15][15][...] image
        cp, hp, tp = pad(code(x[..., i])[..., None])[..., 0], pad(x[..., P + i, None].double()), pad(x[..., 2 * P + i, None].double())
        inside = pad(torch.ones(B, 13, 13, 1, dtype=torch.float64))
        img = w['b1'].expand(B, 13, 13, 8).clone()
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            sl = (slice(None), slice(ky, ky + 13), slice(kx, kx + 13))
            img = img + inside[sl] * (w['t1'][tap][cp[sl]] + hp[sl] * w['w1x'][tap, 0] + tp[sl] * w['w1x'][tap, 1])
        img = pad(hs(img))
        out = w['b2'].expand(B, 13, 13, 8).clone()
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            out = out + img[:, ky:ky + 13, kx:kx + 13] @ w['w2'][tap]
        e = e + hs(out) @ w['we'][8 * i:8 * i + 8]
    d = hs(hs(e) * w['dws'] + w['dwb']).reshape(B, 169, 32)
    se = F.hardsigmoid(F.relu(d.mean(dim=1) @ w['fc1'] + w['fc1b']) @ w['fc2'] + w['fc2b'])
    p = (d * se[:, None]) @ w['wp'] + w['bp']                                               # [B][169][16]
    lg = torch.einsum('bnr,bcor->bcno', p, wc).reshape(B, 1014 * CS)
    lg = torch.where(valids.bool(), lg, torch.full_like(lg, -1e8))
    v = hs(hs(f3.reshape(B, CS * 56) @ w['wv1'] + w['bv1']) @ w['wv2'] + w['bv2']) @ w['wv3'] + w['bv3']
    return torch.softmax(lg, dim=1), torch.tanh(v)


@pytest.mark.parametrize('P', [2, 3, 4])
def test_akropolis_v31_packed_operands_reproduce_the_net(P):
    from azg_amd import nnet
    base = nnet.AkropolisV31.from_npz(_w(P), num_players=P, device='cpu')
    blocks = nnet.AkropolisV31Hip.pack(base)
    # sizes of the three blocks as the kernel's offsets (Akr31<P>::N_CTX, N_BOARDS, N_PROJ) count them
    CS = P + 2
    assert [b.numel() for b in blocks] == [240 * P + 16 + 16 + 8 + 1152 + 32 + 896 + 16 + 5376 + 96 + 768 + 32 + 896 * CS + 16 + 256 + 16 +
                                           16 * P + P, 864 + 144 + 8 + 576 + 8 + 256 * P, 32 + 32 + 256 + 8 + 256 + 32 + 512 + 16]
    assert all(b.dtype == torch.float32 for b in blocks)
    for ref in _sets(P).values():
        pi, v = _emulate_kernel(blocks, torch.from_numpy(ref[0]), torch.from_numpy(ref[1]), P)
        assert_close(pi, v, ref)


def test_wrapper_maps_akropolis_v31_to_its_module():
    """(Akropolis, nn_version 31) -> train.AkropolisV31Module for 2, 3 and 4 players (an engine net: evaluator_for gives it the one-launch
    kernel); the game's other versions stay unbuilt, and Akropolis has no default version"""
    from types import SimpleNamespace
    from azg_amd import _lib, nnet_wrapper, train
    for P in (2, 3, 4):
        A = 1014 * (P + 2)
        g = SimpleNamespace(GAME_ID=_lib.AKROPOLIS, P=P, A=A, variant=P, device=torch.device('cpu'))
        m = nnet_wrapper._module_for(g, 31, 0.0)
        assert type(m) is train.AkropolisV31Module and m.version == 31 and (m.P, m.A) == (P, A)
        m.load_state_dict(_sd(P), strict=True)
        for ver in (1, 30, 32, 40, 62):
            with pytest.raises(ValueError):
                nnet_wrapper._module_for(g, ver, 0.0)
        assert (_lib.AKROPOLIS, P) not in nnet_wrapper._DEFAULT_VERSION


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)), reason='needs the ROCm LLVM tools and the built library')
def test_akropolis_kernel_has_no_spills_and_fits_lds():
    k = kernel_notes(LIB)
    m = {n: v for n, v in k.items() if 'k_akr31_net<' in n}
    assert len(m) == 3, [n for n in k if 'akr31' in n]
    for n, r in m.items():
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, (n, r)
        assert 0 < r['lds'] <= 160 * 1024, (n, r)              # all of the kernel's LDS is static
