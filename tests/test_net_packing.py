"""The weight packers of the engine nets (nnet._split_frag with nnet._pow2_scale, and the f32 packer nnet._frag) against their definitions, on
the CPU: the fragment layouts element by element, the precision of the f16 x 2 and bf16 x 3 planes, and the scale of an all-zero matrix."""
import math

import pytest
import torch

from azg_amd import nnet

SHAPES = [(32, 16), (64, 48), (160, 32)]        # one tile; several tiles and chunks; the five chunks of the V78 policy FC


def _matrix(K, N):
    g = torch.Generator().manual_seed(1000 * K + N)
    m = 0.3 * torch.randn((K, N), generator=g)
    m[K // 2, N // 3] = 0.0
    m[K - 1, N - 1] = 1e-7
    return m


def _planes(out, K, N, planes):
    """the [planes][K][N] matrices a flat fragment tensor holds, by the layout's definition:
    o[ct, c, p, lane, j] = plane_p[32c + 8(lane>>4) + j, 16ct + (lane&15)]"""
    o = out.view(N // 16, K // 32, planes, 64, 8)
    ct, c, p, lane, j = torch.meshgrid(torch.arange(N // 16), torch.arange(K // 32), torch.arange(planes), torch.arange(64), torch.arange(8),
                                       indexing='ij')
    pl = torch.zeros((planes, K, N), dtype=out.dtype)
    seen = torch.zeros((planes, K, N), dtype=torch.int32)
    rows, cols = 32 * c + 8 * (lane >> 4) + j, 16 * ct + (lane & 15)
    pl[p, rows, cols] = o
    seen.index_put_((p, rows, cols), torch.ones_like(rows, dtype=torch.int32), accumulate=True)
    assert bool((seen == 1).all())              # the layout is a bijection: every element of every plane exactly once
    return pl


@pytest.mark.parametrize('K,N', SHAPES)
def test_h2_fragments(K, N):
    m = _matrix(K, N)
    k = nnet._pow2_scale(m.abs().max())
    out = nnet._split_frag(m, 'h2', k)
    assert out.dtype == torch.float16 and out.shape == (2 * K * N,)
    ms = m * (2.0 ** k)
    assert 2.0 ** 11 < float(ms.abs().max()) <= 2.0 ** 12
    hi = ms.to(torch.float16)
    lo = (ms - hi.float()).to(torch.float16)
    pl = _planes(out, K, N, 2)
    assert torch.equal(pl[0], hi) and torch.equal(pl[1], lo)
    # 11 + 11 significand bits, and the f16 subnormal floor
    err = (pl[0].double() + pl[1].double() - ms.double()).abs()
    assert bool((err <= 2.0 ** -22 * ms.double().abs() + 2.0 ** -25).all())
    assert nnet._descale(k) == 2.0 ** -k / 64.0


@pytest.mark.parametrize('K,N', SHAPES)
def test_bf16x3_fragments(K, N):
    m = _matrix(K, N)
    out = nnet._split_frag(m, 'bf16x3')
    assert out.dtype == torch.bfloat16 and out.shape == (3 * K * N,)
    hi = m.to(torch.bfloat16)
    mid = (m - hi.float()).to(torch.bfloat16)
    lo = (m - hi.float() - mid.float()).to(torch.bfloat16)
    pl = _planes(out, K, N, 3)
    assert torch.equal(pl[0], hi) and torch.equal(pl[1], mid) and torch.equal(pl[2], lo)
    assert torch.equal(pl[0].double() + pl[1].double() + pl[2].double(), m.double())


def test_all_zero_matrix():
    m = torch.zeros((64, 48))
    k = nnet._pow2_scale(m.abs().max())
    ds = nnet._descale(k)
    assert math.isfinite(ds) and math.isfinite(float(torch.tensor(ds, dtype=torch.float32))) and ds > 0.0
    out = nnet._split_frag(m, 'h2', k)
    assert out.shape == (2 * 64 * 48,) and float(out.float().abs().max()) == 0.0
    assert float(nnet._split_frag(m, 'bf16x3').float().abs().max()) == 0.0


def test_rejects_unpadded_shapes_and_overflow():
    with pytest.raises(AssertionError):
        nnet._split_frag(torch.zeros((48, 16)), 'h2', 0)
    with pytest.raises(AssertionError):
        nnet._split_frag(torch.zeros((32, 24)), 'bf16x3')
    with pytest.raises(AssertionError):
        nnet._split_frag(torch.full((32, 16), 1.0), 'h2', 17)          # 2^17 does not fit f16: the scale must come from _pow2_scale


F32_SHAPES = [(16, 16), (64, 48), (176, 64)]    # one tile; several tiles and chunks; the 11 chunks of the V80 project matrix


def _f32_matrix(out, K, N):
    """the [K][N] matrix a flat f32 fragment tensor holds, by the layout's definition: o[nt, c, lane, j] = W[16c + 4(lane>>4) + j, 16nt + (lane&15)]"""
    o = out.view(N // 16, K // 16, 64, 4)
    nt, c, lane, j = torch.meshgrid(torch.arange(N // 16), torch.arange(K // 16), torch.arange(64), torch.arange(4), indexing='ij')
    w = torch.zeros((K, N), dtype=out.dtype)
    seen = torch.zeros((K, N), dtype=torch.int32)
    rows, cols = 16 * c + 4 * (lane >> 4) + j, 16 * nt + (lane & 15)
    w[rows, cols] = o
    seen.index_put_((rows, cols), torch.ones_like(rows, dtype=torch.int32), accumulate=True)
    assert bool((seen == 1).all())              # every element exactly once
    return w


@pytest.mark.parametrize('K,N', F32_SHAPES)
def test_f32_fragments(K, N):
    m = _matrix(K, N)
    out = nnet._frag(m)
    assert out.dtype == torch.float32 and out.shape == (K * N,) and out.is_contiguous()
    assert torch.equal(_f32_matrix(out, K, N), m)


def test_f32_fragments_half_last_chunk():
    """K = 8 mod 16 (zero padded to [64][176], rows 56..63 zero): lane group g of the last chunk holds rows 16c + 2g + {0, 1} in j = 0, 1"""
    m = _matrix(64, 176)
    m[56:] = 0.0
    keep = m.clone()
    o = nnet._frag(m, True).view(11, 4, 64, 4)
    assert torch.equal(m, keep)                                                    # the argument is left alone
    assert torch.equal(o[:, :3], nnet._frag(m[:48].contiguous()).view(11, 3, 64, 4))   # the whole chunks as without half_last
    for nt in range(11):
        for lane in range(64):
            g, col = lane >> 4, 16 * nt + (lane & 15)
            assert torch.equal(o[nt, 3, lane, :2], m[48 + 2 * g: 48 + 2 * g + 2, col])
            assert float(o[nt, 3, lane, 2:].abs().max()) == 0.0
    with pytest.raises(AssertionError):
        bad = m.clone()
        bad[59, 3] = 1.0                        # a non-zero row among the last 8
        nnet._frag(bad, True)


def test_f32_fragments_reject_unpadded_shapes():
    with pytest.raises(AssertionError):
        nnet._frag(torch.zeros((24, 16)))
    with pytest.raises(AssertionError):
        nnet._frag(torch.zeros((16, 24)))
