"""CPU: code-object notes of the optimiser's two kernels (csrc/train.hip.h), read as tests/test_train_batches_surface.py reads them: no
scratch, no spilled register, no LDS.  Measured build: k_adamw_onecycle 52 VGPRs (two 16-byte loads of p, g, m and v per lane in flight),
k_adamw_step_advance 4 -- each bounded at the next multiple of 16 above (64 / 16).
(The kernels are named k_adamw_*, not k_train_*: tests/test_train_batches_surface.py counts the k_train_ kernels of the library.)"""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_optimiser_kernels_need_no_scratch_no_lds_and_stay_within_their_registers():
    notes = kernel_notes(LIB)
    bounds = {'k_adamw_onecycle(': 64, 'k_adamw_step_advance(': 16}
    for frag, vgpr_max in bounds.items():
        k = [(n, v) for n, v in notes.items() if frag in n]
        assert len(k) == 1, (frag, sorted(n for n in notes if 'adamw' in n))
        n, v = k[0]
        assert v['scratch'] == 0 and v['vgpr_spill'] == 0 and v.get('sgpr_spill', 0) == 0, (n, v)
        assert v['lds'] == 0, (n, v)
        assert v['vgpr'] <= vgpr_max, (n, v)
    assert len([n for n in notes if 'k_adamw_' in n]) == 2
