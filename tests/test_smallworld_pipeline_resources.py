"""Code-generation guard for the Smallworld kernels of the asynchronous tree pipeline (CPU-only: the metadata notes of the code objects
inside libazg_hip.so, read as tests/test_kernel_resources.py reads them) and the C-ABI symbol of its entry point.

Descent (k_async_select<SmallworldDev<P>>): 16 waves per CU -> at most 128 VGPRs.  The game's make_move / valid_mask stay out of line
 and need 148 / 152 / 212 VGPRs where the register file allows it (k_select, k_selfplay_advance); under the pipeline's cap
they are compiled to 128 and spill -- those spills, in cold rules code run by one lane, are most of the counts below (measured build:
150 / 201 / 254 spilled vector registers, 784 / 896 / 1084 B of scratch).  Net (k_async_net<NetSw62<P>>): 12 waves per CU -> at most 168
VGPRs; the V62 forward inside the persistent loop runs without scratch memory (measured: 110 / 110 / 122 VGPRs)."""
import ctypes
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_smallworld_pipeline_kernels_stay_within_their_register_budgets():
    k = kernel_notes(LIB)

    def one(frag):
        m = [v for n, v in k.items() if frag in n]
        assert len(m) == 1, (frag, [n for n in k if frag in n])
        return m[0]

    for P, spill_max, scratch_max in ((2, 164, 832), (3, 216, 960), (4, 272, 1152)):
        v = one('k_async_select<azg::SmallworldDev<%d> >' % P)
        assert v['vgpr'] <= 128, (P, v)
        assert v['vgpr_spill'] <= spill_max and v['scratch'] <= scratch_max, (P, v)
    for P in (2, 3, 4):
        v = one('k_async_net<azg::NetSw62<%d> >' % P)
        assert v['vgpr'] <= 168 and v['vgpr_spill'] == 0 and v['scratch'] == 0, (P, v)
        v = one('k_async_net<azg::NetHash<azg::SmallworldDev<%d> > >' % P)
        assert v['vgpr'] <= 168 and v['scratch'] == 0, (P, v)


@pytest.mark.skipif(not os.path.exists(LIB), reason='needs the built library')
def test_smallworld_pipeline_entry_point_is_exported():
    from azg_amd import _lib
    assert 'azg_forest_async_rounds_sw62' in _lib.EXPORTS
    L = ctypes.CDLL(LIB)
    assert hasattr(L, 'azg_forest_async_rounds_sw62')
