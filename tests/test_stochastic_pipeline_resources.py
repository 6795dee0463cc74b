"""Code-generation guard for the Minivilles / The Little Prince kernels of the asynchronous tree pipeline (CPU-only: the metadata notes of the
code objects inside libazg_hip.so, read as tests/test_kernel_resources.py reads them) and the C-ABI symbol of their entry point.

Descent (k_async_select<MinivillesDev<P>> / k_async_select<TLPDev<P>>): 16 waves per CU -> at most 128 VGPRs.  The games' make_move
(dice, market refills) and valid_mask stay out of line and are compiled to the cap; the spills are mostly in that cold rules code
(measured build: 6 / 8 / 20 spilled vector registers and 448 / 472 / 468 B of scratch for Minivilles 2 / 3 / 4 players, 30 / 22 / 22 and
532 / 584 / 568 B for TLP 3 / 4 / 5 players).  Bounds: the measured spills + 8, the measured scratch + 64 B.

Net (k_async_net<NetMb1d<Cfg..>>): 12 waves per CU -> at most 168 VGPRs (measured: 145 / 162 / 168 for Minivilles 2 / 3 / 4, 140 / 168 / 168
for TLP 3 / 4 / 5).  Four of the six forwards run without scratch memory.  The two widest nets, Minivilles 4 players (C = 98) and TLP
5 players (C = 91), sit at the cap and keep 6 / 7 thread-derived LDS addresses that the compiler hoisted out of the persistent loop in
scratch (28 / 32 B: five scratch loads per forward, outside the GEMM loops) -- as the existing Splendor 4 players / Azul net kernels of the
same family do (60 / 24 B).  The hoisting comes from the raw threadIdx.x reads inside nn_mb1d.hip.h; bounds: 8 spilled registers and 40 B.
The hash-net evaluator (k_async_net<NetHash<..>>) needs ~40 VGPRs and no scratch."""
import ctypes
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)

# (game of the descent, its spill / scratch bounds, the net's Mb1dCfg prefix, its spill / scratch bounds)
_KINDS = (('MinivillesDev<2>', 14, 512, 'Mb1dCfg<2, 58, 16, 21, 2,', 0, 0),
          ('MinivillesDev<3>', 16, 536, 'Mb1dCfg<2, 78, 16, 21, 3,', 0, 0),
          ('MinivillesDev<4>', 28, 532, 'Mb1dCfg<2, 98, 16, 21, 4,', 8, 40),
          ('TLPDev<3>', 38, 596, 'Mb1dCfg<15, 55, 8, 9, 3,', 0, 0),
          ('TLPDev<4>', 30, 648, 'Mb1dCfg<15, 73, 6, 16, 4,', 0, 0),
          ('TLPDev<5>', 30, 632, 'Mb1dCfg<15, 91, 6, 25, 5,', 8, 40))


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_stochastic_pipeline_kernels_stay_within_their_register_budgets():
    k = kernel_notes(LIB)

    def one(*frags):
        m = [v for n, v in k.items() if all(f in n for f in frags)]
        assert len(m) == 1, (frags, [n for n in k if all(f in n for f in frags)])
        return m[0]

    for game, sel_spill, sel_scratch, cfg, net_spill, net_scratch in _KINDS:
        v = one('k_async_select<azg::%s >' % game)
        assert v['vgpr'] <= 128, (game, v)
        assert v['vgpr_spill'] <= sel_spill and v['scratch'] <= sel_scratch, (game, v)
        v = one('k_async_net<azg::NetMb1d<azg::%s' % cfg, 'azg::%s >' % game)
        assert v['vgpr'] <= 168 and v['vgpr_spill'] <= net_spill and v['scratch'] <= net_scratch, (game, v)
        v = one('k_async_net<azg::NetHash<azg::%s > >' % game)
        assert v['vgpr'] <= 168 and v['scratch'] == 0, (game, v)


@pytest.mark.skipif(not os.path.exists(LIB), reason='needs the built library')
def test_stochastic_pipeline_entry_points_are_exported():
    from azg_amd import _lib
    for sym in ('azg_forest_async_rounds_mb1d_h2', 'azg_forest_async_rounds_hashnet'):
        assert sym in _lib.EXPORTS or hasattr(_lib.lib(), sym)
        assert hasattr(ctypes.CDLL(LIB), sym)
