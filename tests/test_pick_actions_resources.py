"""Code-generation guard for the move-picking kernels (csrc/pick.hip.h; CPU-only: the metadata notes of the code objects inside
libazg_hip.so, read as tests/test_kernel_resources.py reads them).  One wave per game, rows streamed through a handful of registers: the
three kernels (one per mode) need no scratch memory, no LDS and at most 64 VGPRs (measured build: 9 / 10 / 24)."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_pick_kernels_need_no_scratch_and_few_registers():
    k = {n: v for n, v in kernel_notes(LIB).items() if 'k_pick_actions<' in n}
    assert len(k) == 3, sorted(k)
    for n, v in k.items():
        assert v['scratch'] == 0 and v['vgpr_spill'] == 0 and v['lds'] == 0, (n, v)
        assert v['vgpr'] <= 64, (n, v)
