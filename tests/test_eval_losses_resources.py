"""Code-generation guard for the validation-loss kernels (csrc/loss.hip.h; CPU-only: the metadata notes of the code objects inside
libazg_hip.so, read as tests/test_kernel_resources.py reads them).  One wave per example row / one wave for the totals, rows streamed
through a handful of registers with the f64 log inlined: both kernels need no scratch memory, no LDS, no spilled register and at most
64 VGPRs, the bound the pick kernels are held to (measured build: 40 / 48)."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_loss_kernels_need_no_scratch_and_few_registers():
    notes = kernel_notes(LIB)
    k = {n: v for n, v in notes.items() if 'k_eval_losses(' in n or 'k_eval_totals(' in n}
    assert len(k) == 2, sorted(n for n in notes if 'k_eval' in n)
    for n, v in k.items():
        assert v['scratch'] == 0 and v['vgpr_spill'] == 0 and v.get('sgpr_spill', 0) == 0 and v['lds'] == 0, (n, v)
        assert v['vgpr'] <= 64, (n, v)
