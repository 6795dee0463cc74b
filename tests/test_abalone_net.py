"""Abalone net V21 on the CPU: the plain-torch re-expression and the trainable module against the reference model's own outputs
(netfwd_abalone_v21.npz, netfwd64_abalone_v21.npz: pretrained_BelgianDaisy.pt, tools/convert_ckpt.py), the wrapper's game/version
mapping, and the resources of the engine kernel (k_aba21_net, csrc/nn_abalone.hip.h) read from the library's code-object notes."""
import os

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB, LLVM, kernel_notes
from test_nnet import assert_net_close

ROOT = os.path.join(os.path.dirname(__file__), 'golden')
W = os.path.join(ROOT, 'weights_abalone_v21.npz')


def _sd():
    z = np.load(W)
    return {k[3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith('sd/')}


def test_abalone_v21_torch_matches_reference():
    from azg_amd import nnet
    d = np.load(os.path.join(ROOT, 'netfwd_abalone_v21.npz'))
    net = nnet.AbaloneV21.from_npz(W, device='cpu')
    assert (net.A, net.P) == (3402, 2)
    pi, v = net.predict_batch(torch.from_numpy(d['boards']).reshape(len(d['boards']), -1), torch.from_numpy(d['masks']))
    assert_net_close(pi, v, 'abalone_v21', d)
    p1, v1 = net.predict(d['boards'][3], d['masks'][3])
    assert np.abs(p1 - d['pi'][3]).max() <= 1e-5 and np.abs(v1 - d['v'][3]).max() <= 1e-5


def test_abalone_v21_module_loads_the_shipped_state_dict():
    from azg_amd import train
    d = np.load(os.path.join(ROOT, 'netfwd_abalone_v21.npz'))
    m = train.AbaloneV21Module()
    m.load_state_dict(_sd(), strict=True)
    m.eval()
    with torch.no_grad():
        lp, v = m(torch.from_numpy(d['boards']), torch.from_numpy(d['masks']).bool())
    assert_net_close(torch.exp(lp), v, 'abalone_v21', d)


def test_wrapper_maps_abalone_v21_to_its_module():
    """(Abalone, nn_version 21) -> train.AbaloneV21Module (an engine net: evaluator_for gives it the one-launch kernel); other versions
    of the game stay unbuilt"""
    from types import SimpleNamespace
    from azg_amd import _lib, nnet_wrapper, train
    g = SimpleNamespace(GAME_ID=_lib.ABALONE, P=2, A=3402, variant=1, device=torch.device('cpu'))
    m = nnet_wrapper._module_for(g, 21, 0.0)
    assert type(m) is train.AbaloneV21Module and m.version == 21
    m.load_state_dict(_sd(), strict=True)
    for ver in (10, 20, 80):
        with pytest.raises(ValueError):
            nnet_wrapper._module_for(g, ver, 0.0)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)), reason='needs the ROCm LLVM tools and the built library')
def test_abalone_kernel_has_no_spills_and_fits_lds():
    import re
    k = kernel_notes(LIB)
    m = [v for n, v in k.items() if 'k_aba21_net<' in n]
    assert len(m) == 1, [n for n in k if 'aba21' in n]
    r = m[0]
    assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r
    # static + dynamic LDS: the launch's dynamic size is ABA_LDS of the header
    src = open(os.path.join(os.path.dirname(LIB), 'csrc', 'nn_abalone.hip.h')).read()
    c = dict((a, int(b)) for a, b in re.findall(r'ABA_(\w+) = (\d+)', src))
    dyn = (c['RT'] * 16 * (c['XS'] + c['HS']) + c['NS'] * (16 + 64)) * 4
    assert r['lds'] + dyn <= 160 * 1024, (r['lds'], dyn)
