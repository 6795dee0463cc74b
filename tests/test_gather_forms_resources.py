"""CPU: code-object notes of the k_gather_forms* kernels (csrc/examples.hip.h; azg_train_gather_forms), read as
tests/test_train_adamw_resources.py reads them: no scratch, no spilled register, LDS no larger than the k_env_symmetries* kernel of the
same game, VGPRs within the next multiple of 16 above the measured build.

Measured build (VGPRs; bound): k_gather_forms -- Splendor 2 / 3 / 4: 27 / 18 / 27 (32), Santorini 1 / 11: 16 / 16 (32), Azul 10 (16),
Abalone 16 (32), Minivilles 8 (16); k_gather_forms_built -- The Little Prince 3 / 4 / 5: 93 / 91 / 95 (96), Botanik 53 (64), Akropolis
2 / 3 / 4: 20 / 28 / 34 (32 / 32 / 48), Smallworld 12 (16).  LDS equals that of the k_env_symmetries* kernel of the same game in every
case (Splendor-2p 400 B, Azul 144 B, The Little Prince 3p 6680 B, Akropolis 4p 16912 B).
(The kernels are named k_gather_forms*, neither k_examples_* nor k_train_*: tests/test_device_history_surface.py and
tests/test_train_batches_surface.py count the kernels with those names.)"""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)

# kernel fragment -> VGPR bound (the next multiple of 16 above the measured build, module docstring)
VGPR_BOUNDS = {
    'k_gather_forms<azg::SplendorDev<2> >': 32, 'k_gather_forms<azg::SplendorDev<3> >': 32, 'k_gather_forms<azg::SplendorDev<4> >': 32,
    'k_gather_forms<azg::SantoriniDev<1> >': 32, 'k_gather_forms<azg::SantoriniDev<11> >': 32, 'k_gather_forms<azg::AzulDev>': 16,
    'k_gather_forms<azg::AbaloneDevT<false> >': 32, 'k_gather_forms<azg::AbaloneDevT<true> >': 32,
    'k_gather_forms<azg::MinivillesDev<2> >': 16, 'k_gather_forms<azg::MinivillesDev<3> >': 16, 'k_gather_forms<azg::MinivillesDev<4> >': 16,
    'k_gather_forms_built<azg::TLPDev<3> >': 96, 'k_gather_forms_built<azg::TLPDev<4> >': 96, 'k_gather_forms_built<azg::TLPDev<5> >': 96,
    'k_gather_forms_built<azg::BotanikDev>': 64,
    'k_gather_forms_built<azg::AkropolisDev<2> >': 32, 'k_gather_forms_built<azg::AkropolisDev<3> >': 32, 'k_gather_forms_built<azg::AkropolisDev<4> >': 48,
    'k_gather_forms_built<azg::SmallworldDev<2> >': 16, 'k_gather_forms_built<azg::SmallworldDev<3> >': 16, 'k_gather_forms_built<azg::SmallworldDev<4> >': 16,
}


@pytest.fixture(scope='module')
def notes():
    return kernel_notes(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_there_is_one_gather_forms_kernel_per_game_and_no_other(notes):
    ks = sorted(n.split('(')[0].replace('void azg::', '') for n in notes if 'k_gather_forms' in n)
    assert ks == sorted(VGPR_BOUNDS)
    assert not [n for n in ks if 'k_examples_' in n or 'k_train_' in n]


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
@pytest.mark.parametrize('frag', sorted(VGPR_BOUNDS))
def test_gather_forms_kernel_resources(notes, frag):
    k = [(n, v) for n, v in notes.items() if ('azg::' + frag + '(') in n]
    assert len(k) == 1, (frag, sorted(n for n in notes if 'k_gather_forms' in n))
    n, v = k[0]
    twin_name = frag.replace('k_gather_forms_built', 'k_env_symmetries_built').replace('k_gather_forms<', 'k_env_symmetries<')
    twin = [(m, w) for m, w in notes.items() if ('azg::' + twin_name + '(') in m]
    assert len(twin) == 1, frag
    print(frag, v, 'symmetry kernel:', twin[0][1])
    assert v['lds'] <= twin[0][1]['lds'], (n, v, twin[0][1])
    assert v['vgpr'] <= VGPR_BOUNDS[frag], (n, v)
    assert v['vgpr_spill'] == 0 and v.get('sgpr_spill', 0) == 0, (n, v)
    assert v['scratch'] == 0, (n, v)
