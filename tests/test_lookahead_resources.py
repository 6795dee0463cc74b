"""Code-generation guard for the lookahead kernels (csrc/lookahead.hip.h; CPU-only: the metadata notes of the code objects inside
libazg_hip.so, read as tests/test_kernel_resources.py reads them).  k_env_lookahead<G> runs G::valid_mask, G::wave_make_move, G::game_ended
and G::get_score one after another on LDS states, so -- the argument of tests/test_playouts_resources.py -- it needs no more private
memory than the neediest of the three env kernels that each run one of them: its scratch size and its spilled vector registers are
bounded by the largest among k_env_valid_moves<G>, k_env_next_state<G> and k_env_game_ended<G> of the same game in the same build."""
import os
import re

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_lookahead_kernels_need_no_more_private_memory_than_the_env_kernels():
    notes = kernel_notes(LIB)

    def by_game(kernel):
        out = {}
        for n, v in notes.items():
            m = re.search(r'\b%s<(.*)>\(' % kernel, n)
            if m:
                out[m.group(1)] = v
        return out

    look, step, valid, ended = (by_game(k) for k in ('k_env_lookahead', 'k_env_next_state', 'k_env_valid_moves', 'k_env_game_ended'))
    assert len(look) > 0 and sorted(look) == sorted(step) == sorted(valid) == sorted(ended), (sorted(look), sorted(step))
    for g, v in sorted(look.items()):
        others = (step[g], valid[g], ended[g])
        print(g, 'lookahead', v, 'scratch of the env kernels', [o['scratch'] for o in others], 'spills', [o['vgpr_spill'] for o in others])
        assert v['scratch'] <= max(o['scratch'] for o in others), (g, v, others)
        assert v['vgpr_spill'] <= max(o['vgpr_spill'] for o in others), (g, v, others)
