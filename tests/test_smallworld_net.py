"""Smallworld net V62 on the CPU: the plain-torch re-expression and the trainable module against the reference model's own outputs
(netfwd_smallworld*_v62.npz, netfwd64_smallworld*_v62.npz: pretrained_{2,3,4}pl.pt, tools/convert_ckpt.py), the wrapper's game/version
mapping, the kernel's packed operand order, and the resources of the engine kernel (k_sw62_net, csrc/nn_smallworld.hip.h) read from the
library's code-object notes."""
import os

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB, LLVM, kernel_notes
from test_nnet import assert_net_close

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
TAGS = {2: 'smallworld_v62', 3: 'smallworld3_v62', 4: 'smallworld4_v62'}
SHAPES = {2: (40, 131), 3: (52, 166), 4: (66, 211)}


def _w(P):
    return os.path.join(ROOT, 'weights_%s.npz' % TAGS[P])


def _sd(P):
    z = np.load(_w(P))
    return {k[3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith('sd/')}


def _d(P):
    return np.load(os.path.join(ROOT, 'netfwd_%s.npz' % TAGS[P]))


@pytest.mark.parametrize('P', [2, 3, 4])
def test_smallworld_v62_torch_matches_reference(P):
    from azg_amd import nnet
    d = _d(P)
    net = nnet.SmallworldV62.from_npz(_w(P), num_players=P, device='cpu')
    assert (net.N, net.A, net.P) == SHAPES[P] + (P,)
    assert d['boards'].min() < 0                        # negative bitfields are exercised
    pi, v = net.predict_batch(torch.from_numpy(d['boards']).reshape(len(d['boards']), -1), torch.from_numpy(d['masks']))
    assert_net_close(pi, v, TAGS[P], d)
    p1, v1 = net.predict(d['boards'][3], d['masks'][3])
    assert np.abs(p1 - d['pi'][3]).max() <= 1e-5 and np.abs(v1 - d['v'][3]).max() <= 1e-5


@pytest.mark.parametrize('P', [2, 3, 4])
def test_smallworld_v62_module_loads_the_shipped_state_dict(P):
    from azg_amd import train
    d = _d(P)
    m = train.SmallworldV62Module(P, SHAPES[P][1])
    m.load_state_dict(_sd(P), strict=True)
    m.eval()
    with torch.no_grad():
        lp, v = m(torch.from_numpy(d['boards']), torch.from_numpy(d['masks']).bool())
    assert_net_close(torch.exp(lp), v, TAGS[P], d)


def test_smallworld_v62_module_applies_dropout_in_training():
    from azg_amd import train
    d = _d(2)
    m = train.SmallworldV62Module(2, 131, dropout=0.3)
    m.load_state_dict(_sd(2), strict=True)
    b, va = torch.from_numpy(d['boards'][:8]), torch.from_numpy(d['masks'][:8]).bool()
    m.train()
    torch.manual_seed(0)
    a = m(b, va)[0]
    torch.manual_seed(1)
    assert not torch.equal(a, m(b, va)[0])
    m.eval()
    assert torch.equal(m(b, va)[0], m(b, va)[0])


def _emulate_kernel(keep, boards, valids, P):
    """the kernel's arithmetic order written out in torch (f64) from the packed operands: a check of the fragment layout of pack() and of
    the k order the header documents (k = 16 (m >> 2) + 4 g + (m & 3) in MFMA m for the lanes of group g)"""
    N, A = SHAPES[P]
    nA = (A - 16) // 5
    w = [t.double() for t in keep]

    def unfrag(fr, K, nct):                              # [nct][K / 4][64] -> W^T [K][16 nct]
        z = fr.view(nct, K // 16, 4, 4, 16)              # (ct, a, j, g, i)
        return z.permute(1, 3, 2, 0, 4).reshape(K, 16 * nct)
    B = boards.shape[0]
    c = boards.reshape(B, N, 8).long()
    f = torch.cat([c[..., [0, 3, 4, 5, 6]].double() / 10.0] + [((c[..., j:j + 1] >> torch.arange(8)) & 1).double() for j in (3, 4)], dim=-1)
    x = w[0][(c[..., 1] + 15).clamp(0, 30)] + w[1][(c[..., 2] + 20).clamp(0, 40)] + w[2][(c[..., 7] + 1).clamp(0, 5)] + f @ w[3] + w[4]
    x = torch.nn.functional.layer_norm(x, (48,), w[5], w[6])
    for l in range(3):
        wqkv = unfrag(w[7].view(3, -1)[l], 48, 9)
        qkv = x @ wqkv + w[8].view(3, 144)[l]
        q, k, v = (qkv[..., 48 * j:48 * (j + 1)].view(B, N, 3, 16).transpose(1, 2) for j in range(3))
        o = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).transpose(1, 2).reshape(B, N, 48)
        x = torch.nn.functional.layer_norm(x + o @ unfrag(w[9].view(3, -1)[l], 48, 3) + w[10].view(3, 48)[l], (48,), w[11].view(3, 48)[l],
                                           w[12].view(3, 48)[l])
        h = torch.relu(x @ unfrag(w[13].view(3, -1)[l], 48, 12) + w[14].view(3, 192)[l])
        x = torch.nn.functional.layer_norm(x + h @ unfrag(w[15].view(3, -1)[l], 192, 3) + w[16].view(3, 48)[l], (48,), w[17].view(3, 48)[l],
                                           w[18].view(3, 48)[l])
    loc = x[:, :nA] @ w[19] + w[20]
    g = x[:, nA:].mean(dim=1)
    gl = g @ w[21] + w[22]
    lg = torch.cat([loc[..., 0], loc[..., 1], loc[..., 2], loc[..., 3], gl[:, :8], loc[..., 4], gl[:, 8:]], dim=1)
    lg = torch.where(valids.bool(), lg, torch.full_like(lg, -1e8))
    return torch.softmax(lg, dim=1), torch.tanh(g @ w[23] + w[24])


@pytest.mark.parametrize('P', [2, 4])
def test_smallworld_v62_packed_operands_reproduce_the_net(P):
    from azg_amd import nnet
    d = _d(P)
    base = nnet.SmallworldV62.from_npz(_w(P), num_players=P, device='cpu')
    keep = nnet.SmallworldV62Hip.pack(base)
    assert len(keep) == 25
    pi, v = _emulate_kernel(keep, torch.from_numpy(d['boards']), torch.from_numpy(d['masks']), P)
    assert_net_close(pi, v, TAGS[P], d)


def test_wrapper_maps_smallworld_v62_to_its_module():
    """(Smallworld, nn_version 62) -> train.SmallworldV62Module for 2, 3 and 4 players (an engine net: evaluator_for gives it the one-launch
    kernel); the game's other versions stay unbuilt"""
    from types import SimpleNamespace
    from azg_amd import _lib, nnet_wrapper, train
    for P in (2, 3, 4):
        g = SimpleNamespace(GAME_ID=_lib.SMALLWORLD, P=P, A=SHAPES[P][1], variant=P, device=torch.device('cpu'))
        m = nnet_wrapper._module_for(g, 62, 0.0)
        assert type(m) is train.SmallworldV62Module and m.version == 62 and (m.P, m.A) == (P, SHAPES[P][1])
        m.load_state_dict(_sd(P), strict=True)
        for ver in (31, 42, 80):
            with pytest.raises(ValueError):
                nnet_wrapper._module_for(g, ver, 0.0)
    assert (_lib.SMALLWORLD, 2) not in nnet_wrapper._DEFAULT_VERSION


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)), reason='needs the ROCm LLVM tools and the built library')
def test_smallworld_kernel_has_no_spills_and_fits_lds():
    k = kernel_notes(LIB)
    m = {n: v for n, v in k.items() if 'k_sw62_net<' in n}
    assert len(m) == 3, [n for n in k if 'sw62' in n]
    for n, r in m.items():
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, (n, r)
        assert 0 < r['lds'] <= 160 * 1024, (n, r)              # all of the kernel's LDS is static
