"""Botanik nets V10 / V11 on the CPU: the plain-torch re-expression and the trainable modules against the reference model's own outputs on
the stand-in weights of weightstats_botanik_v1x.npz (netfwd*_botanik_v1x.npz, tools/convert_ckpt.py --botanik), dropout placement, a
torch emulation of the kernel's packed operands (offsets read from csrc/nn_botanik.hip.h), the wrapper's game/version mapping, and the
resources of the engine kernel (k_bot_net, csrc/nn_botanik.hip.h) read from the library's code-object notes."""
import os
import re

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB, LLVM, kernel_notes
from test_nnet import assert_net_close

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
HDR = os.path.join(os.path.dirname(__file__), '..', 'alpha-zero-general_amd', 'csrc', 'nn_botanik.hip.h')
VERSIONS = (10, 11)


def _sd(version):
    from azg_amd import formats
    sd, _ = formats.fixture_state_dict(ROOT, 'botanik_v%d' % version)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _data(version):
    tag = 'botanik_v%d' % version
    return (np.load(os.path.join(ROOT, 'netfwd_%s.npz' % tag)), np.load(os.path.join(ROOT, 'netfwd64_%s.npz' % tag)),
            np.load(os.path.join(ROOT, 'netfwdrand_%s.npz' % tag)))


def _close_random(pi, v, r):
    """random int8 boards: within 1e-5 of the f64 forward plus the reference's own f32 - f64 distance, element by element"""
    pi, v = pi.detach().double().numpy(), v.detach().double().numpy()
    assert np.all(np.abs(pi - r['pi64']) <= 1e-5 + np.abs(r['pi'] - r['pi64'])), np.abs(pi - r['pi64']).max()
    assert np.all(np.abs(v - r['v64']) <= 1e-5 + np.abs(r['v'] - r['v64'])), np.abs(v - r['v64']).max()


@pytest.mark.parametrize('version', VERSIONS)
def test_botanik_torch_net_matches_reference(version):
    from azg_amd import nnet
    d, _, r = _data(version)
    net = nnet.BotanikV1x(_sd(version), device='cpu')
    assert (net.version, net.n_mach, net.A, net.P) == (version, version - 9, 428, 2)
    pi, v = net.predict_batch(torch.from_numpy(d['boards']).reshape(len(d['boards']), -1), torch.from_numpy(d['masks']))
    assert_net_close(pi, v, 'botanik_v%d' % version, d)
    pi, v = net.predict_batch(torch.from_numpy(r['boards']).reshape(len(r['boards']), -1), torch.from_numpy(r['masks']))
    _close_random(pi, v, r)
    p1, v1 = net.predict(d['boards'][3], d['masks'][3])
    assert np.abs(p1 - d['pi'][3]).max() <= 1e-5 and np.abs(v1 - d['v'][3]).max() <= 1e-5


@pytest.mark.parametrize('version', VERSIONS)
def test_botanik_module_loads_the_standin_state_dict(version):
    from azg_amd import train
    d, _, r = _data(version)
    m = (train.BotanikV10Module if version == 10 else train.BotanikV11Module)()
    m.load_state_dict(_sd(version), strict=True)
    m.eval()
    with torch.no_grad():
        lp, v = m(torch.from_numpy(d['boards']), torch.from_numpy(d['masks']).bool())
        assert_net_close(torch.exp(lp), v, 'botanik_v%d' % version, d)
        lp, v = m(torch.from_numpy(r['boards']), torch.from_numpy(r['masks']).bool())
        _close_random(torch.exp(lp), v, r)


@pytest.mark.parametrize('version', VERSIONS)
def test_botanik_module_dropout_only_after_trunk_1d(version, monkeypatch):
    """training mode: one dropout call, on the trunk_1d output (B, 7, 30), with the module's p (BotanikNNet.py:256 / :276)"""
    from azg_amd import train
    import torch.nn.functional as F
    calls = []
    orig = F.dropout

    def spy(x, p=0.5, training=True, inplace=False):
        calls.append((tuple(x.shape), p, training))
        return orig(x, p, training, inplace)
    monkeypatch.setattr(F, 'dropout', spy)
    d, _, _ = _data(version)
    m = (train.BotanikV10Module if version == 10 else train.BotanikV11Module)(dropout=0.3)
    m.load_state_dict(_sd(version), strict=True)
    b, k = torch.from_numpy(d['boards'][:4]), torch.from_numpy(d['masks'][:4]).bool()
    m.train()
    torch.manual_seed(0)
    lp_t, _ = m(b, k)
    assert calls == [((4, 7, 30), 0.3, True)]
    calls.clear()
    m.eval()
    with torch.no_grad():
        lp_e, _ = m(b, k)
    assert calls == [((4, 7, 30), 0.3, False)]
    assert not torch.allclose(lp_t, lp_e)


def _consts():
    src = open(HDR).read()
    return dict((a, int(b)) for a, b in re.findall(r'(BOT1?M?_\w+) = (\d+)', src))


def _unfrag(z, G, nct, K, N):
    return z.view(nct, G, 4, 16).permute(2, 1, 0, 3).reshape(4 * G, 16 * nct)[:K, :N]


def _unsfrag(z, KQ, K, N):
    return z.view(27, KQ, 4, 16).permute(1, 2, 0, 3).reshape(4 * KQ, 432)[:K, :N]


@pytest.mark.parametrize('version', VERSIONS)
def test_botanik_packed_operands_reproduce_the_net(version):
    """unpack the 10 kernel operands at the header's offsets back into the net's folded tensors: the net rebuilt from them gives the same
    outputs within 1e-6, the bias sums being re-associated (every tensor lands where the kernel reads it)"""
    from azg_amd import nnet
    c = _consts()
    base = nnet.BotanikV1x(_sd(version), device='cpu')
    w = nnet.BotanikV1xHip.pack(base)
    t = {}
    w1d = w[0]
    t['1d.W0'], t['1d.b0'] = w1d[:49].view(7, 7), w1d[49:56]
    shapes = [('We', (21, 7), 'BOT1_WE'), ('be', (21,), 'BOT1_BE'), ('Wt', (30, 30), 'BOT1_WT'), ('sd', (21,), 'BOT1_SD'), ('bd', (21,), 'BOT1_BD'),
              ('W1', (8, 21), 'BOT1_W1'), ('b1', (8,), 'BOT1_B1'), ('W2', (21, 8), 'BOT1_W2'), ('b2', (21,), 'BOT1_B2'), ('Wp', (7, 21), 'BOT1_WP'),
              ('bp', (7,), 'BOT1_BP')]
    for j in range(3):
        o = c['BOT1_BLK0'] + j * c['BOT1_BLK']
        for n, sh, key in shapes:
            t['1d.%d.%s' % (j, n)] = w1d[o + c.get(key, 0):o + c.get(key, 0) + int(np.prod(sh))].view(sh)
    mb = c['BOTM_H'] + 6 * c['BOTM_HB']
    assert w[1].numel() == mb * base.n_mach
    for m in range(base.n_mach):
        k, wm = 'm%d.' % m, w[1][m * mb:(m + 1) * mb]
        t[k + 'c0'] = _unfrag(wm[:1024], 16, 1, 63, 16).reshape(3, 3, 7, 16).permute(3, 2, 0, 1)
        o = c['BOTM_T']
        t[k + 't.we'] = _unfrag(wm[o:o + 512], 4, 2, 16, 32).t().reshape(32, 16, 1, 1)
        t[k + 't.be'] = wm[o + c['BOTM_T_BE']:o + c['BOTM_T_BE'] + 32]
        t[k + 't.wd'] = wm[o + c['BOTM_T_WD']:o + c['BOTM_T_WD'] + 288].view(9, 32).t().reshape(32, 1, 3, 3)
        t[k + 't.bd'] = wm[o + c['BOTM_T_BD']:o + c['BOTM_T_BD'] + 32]
        t[k + 't.wp'] = _unfrag(wm[o + c['BOTM_T_WP']:o + c['BOTM_T_WP'] + 512], 8, 1, 32, 16).t().reshape(16, 32, 1, 1)
        t[k + 't.bp'] = wm[o + c['BOTM_T_BP']:o + c['BOTM_T_BP'] + 16]
        for b in range(6):
            q, o = k + 'h%d.' % b, c['BOTM_H'] + b * c['BOTM_HB']
            sl = lambda key, n: wm[o + c[key]:o + c[key] + n]  # noqa: E731
            t[q + 'we'] = _unfrag(wm[o:o + 768], 4, 3, 16, 48).t().reshape(48, 16, 1, 1)
            t[q + 'be'], t[q + 'bd'], t[q + 'b1'], t[q + 'b2'], t[q + 'bp'] = (sl('BOTM_BE', 48), sl('BOTM_BD', 48), sl('BOTM_B1', 16),
                                                                                 sl('BOTM_B2', 48), sl('BOTM_BP', 16))
            t[q + 'wd'] = sl('BOTM_WD', 432).view(9, 48).t().reshape(48, 1, 3, 3)
            t[q + 'w1'] = sl('BOTM_W1', 768).view(16, 48, 1, 1)
            t[q + 'w2'] = sl('BOTM_W2', 768).view(48, 16, 1, 1)
            t[q + 'wp'] = _unfrag(sl('BOTM_WP', 768), 12, 1, 48, 16).t().reshape(16, 48, 1, 1)
    n1, nm = 27 * c['BOT_KQ1'] * 64, 27 * c['BOT_KQM'] * 64
    assert w[2].numel() == n1 + base.n_mach * nm
    t['pi1d.W'] = _unsfrag(w[2][:n1], c['BOT_KQ1'], 210, 428).t()
    t['v1d.W'] = w[4][:420].view(2, 210)
    for m in range(base.n_mach):
        t['pim%d.W' % m] = _unsfrag(w[2][n1 + m * nm:n1 + (m + 1) * nm], c['BOT_KQM'], 784, 428).t()
        t['vm%d.W' % m] = w[4][420 + m * 1568:420 + (m + 1) * 1568].view(2, 784)
        t['pim%d.b' % m], t['vm%d.b' % m] = torch.zeros(428), torch.zeros(2)
    assert torch.all(w[3][428:] == 0) and torch.all(w[6][428:] == 0) and torch.all(w[8][428:] == 0)
    t['pi1d.b'], t['v1d.b'] = w[3][:428], w[9][:2]
    t['f1.W'], t['f1.b'] = _unsfrag(w[5], c['BOT_KQF'], 428, 428).t(), w[6][:428]
    t['f2.W'], t['f2.b'] = _unsfrag(w[7], c['BOT_KQF'], 428, 428).t(), w[8][:428]
    t['fv1.W'], t['fv1.b'], t['fv2.W'], t['fv2.b'] = w[9][2:6].view(2, 2), w[9][6:8], w[9][8:12].view(2, 2), w[9][12:14]
    for key in base.t:
        if not key.endswith('.b') or key.startswith('f'):
            assert torch.equal(t[key].reshape(base.t[key].shape), base.t[key]), key
    emu = nnet.BotanikV1x(_sd(version), device='cpu')
    emu.t = {k: v.reshape(base.t[k].shape).contiguous() for k, v in t.items()}
    d, _, _ = _data(version)
    b, k = torch.from_numpy(d['boards']).reshape(len(d['boards']), -1), torch.from_numpy(d['masks'])
    p0, v0 = base.predict_batch(b, k)
    p1, v1 = emu.predict_batch(b, k)
    assert float((p0 - p1).abs().max()) <= 1e-6 and float((v0 - v1).abs().max()) <= 1e-6   # the bias sums are re-associated


def test_wrapper_maps_botanik_versions_to_their_modules():
    """(Botanik, 10) -> BotanikV10Module, (Botanik, 11) -> BotanikV11Module (engine nets); versions the reference does not define raise"""
    from types import SimpleNamespace
    from azg_amd import _lib, nnet_wrapper, train
    g = SimpleNamespace(GAME_ID=_lib.BOTANIK, P=2, A=428, variant=0, device=torch.device('cpu'))
    for version, cls in ((10, train.BotanikV10Module), (11, train.BotanikV11Module)):
        m = nnet_wrapper._module_for(g, version, 0.0)
        assert type(m) is cls and m.version == version
        m.load_state_dict(_sd(version), strict=True)
    for version in (1, 12):
        with pytest.raises(ValueError):
            nnet_wrapper._module_for(g, version, 0.0)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)), reason='needs the ROCm LLVM tools and the built library')
def test_botanik_kernel_has_no_spills_and_fits_lds():
    k = kernel_notes(LIB)
    m = [v for n, v in k.items() if 'k_bot_net<' in n]
    assert len(m) == 2, [n for n in k if 'bot_net' in n]
    c = _consts()
    dyn = (2 * c['BOT_RT'] * 16 * c['BOT_XS'] + c['BOT_RT'] * 16 * c['BOT_HS'] + c['BOT_NS'] * (48 + 16 + 48 + 2)) * 4
    for r in m:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r
        assert r['lds'] + dyn <= 160 * 1024, (r['lds'], dyn)
