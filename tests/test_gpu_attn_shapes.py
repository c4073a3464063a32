"""Spatial attention at the sequence lengths where the kernel leaves work out or changes lane ownership.

The kernel (csrc/vda_attn.hip) walks 64-key tiles in two 32-key halves, four waves of 32 queries per 128-query
block.  A half of the masked tail tile whose keys are all >= N is skipped whole, a wave whose queries are all
>= N only moves its share of the K / V tiles and takes the barriers, and the MFMA layouts own queries and keys
in groups of 16.  tests/test_gpu_fp16_edges.py covers the 32 / 64 / 128 edges; here are the lengths that put a
fully masked half, a single real key in the second half, dead waves next to live or partly filled ones, and
the 16-query tile edges into play.  Same assertions as there: every element inside the derived bound of
fp16_bounds.spatial_attn_ref_bound, the whole-tensor rel-L1 bar against the float64 reference on the unrounded
q, sentinel guards around the output intact, and batch 1 (batch 0 all NaN) bit-identical to the call on batch 1
alone.  The product route (ops.spatial_attention) must give the same bits as the guarded C-ABI call.
"""
import math

import pytest
import torch

from vda_amd import ops
import fp16_bounds as fb
from helpers import assert_elementwise
from tunelib import tune_lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7776.0  # exactly representable in fp16
GUARD = 1024    # halfs of sentinel before and after the output
BAR_ATTN = 3e-3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def h(t):
    return t.to(DEV, torch.float16).contiguous()


def guarded(shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=torch.float16)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def check_lengths(N):
    T = tune_lib()
    worst = 0.0
    for H in (1, 3):
        one = fb.rnd16(N, 3 * H * 64, seed=N + H)
        both = torch.cat([torch.full_like(one, float("nan")), one])
        ref, bound = fb.spatial_attn_ref_bound(one, 1, N, H)
        t = one.reshape(1, N, 3, H, 64).permute(2, 0, 3, 1, 4).double()
        ref_q = (torch.softmax(t[0] @ t[1].transpose(-1, -2) * 0.125, -1) @ t[2]).transpose(1, 2).reshape(N, H * 64)
        buf2, y2 = guarded((2 * N, H * 64))
        buf1, y1 = guarded((N, H * 64))
        T.spatial_attention(h(both), 2, N, H, out=y2)
        T.spatial_attention(h(one), 1, N, H, out=y1)
        assert guard_ok(buf2) and guard_ok(buf1), "a store outside the output"
        p2 = ops.spatial_attention(h(both), 2, N, H, 64)
        assert torch.equal(p2[N:], y2[N:]) and torch.equal(ops.spatial_attention(h(one), 1, N, H, 64), y1)
        worst = max(worst, assert_elementwise(p2[N:], ref, bound, f"spatial attention N={N} H={H}"))
        assert rel(p2[N:], ref_q) < BAR_ATTN
        assert torch.equal(p2[N:], y1), "batch 1 depends on batch 0"
    print(f"spatial attention N={N}: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("N", [32, 96, 97, 160, 161, 200])
def test_spatial_attention_dead_half_and_wave(N):
    """N = 32: one tile whose second half is all mask (the first half does the unconditional re-base).  96, 160:
    the tail tile's second half is all mask after whole tiles; 97, 161: it holds one real key.  160 / 161 leave
    three / two waves of the second query block without a query, 200 one such wave next to a partly filled one."""
    check_lengths(N)


@pytest.mark.parametrize("N", [15, 16, 17, 47, 48, 49, 143, 144, 145])
def test_spatial_attention_16_query_tile_edges(N):
    """Sequence lengths on both sides of a multiple of 16 that is no multiple of 32: the edges of a 16 x 16 MFMA
    tile of queries and of keys, in the first wave, a later wave and the second query block."""
    check_lengths(N)


@pytest.mark.parametrize("N", [160, 161])
@pytest.mark.parametrize("ramp", ["up", "spike", "down"])
def test_spatial_attention_rebase_with_skipped_half(ramp, N):
    """Climbing scores, one late spike and falling scores (the deferred re-base of the online softmax) where the
    last tile's second half is skipped (N = 160) or holds one key (N = 161), under the per-element bound."""
    T = tune_lib()
    B, H = 2, 2
    qkv = fb.attn_ramp_qkv(ramp, B, N, H)
    ref, bound = fb.spatial_attn_ref_bound(qkv, B, N, H)
    buf, y = guarded((B * N, H * 64))
    T.spatial_attention(h(qkv), B, N, H, out=y)
    assert guard_ok(buf), "a store outside the output"
    p = ops.spatial_attention(h(qkv), B, N, H, 64)
    assert torch.equal(p, y)
    worst = assert_elementwise(p, ref, bound, f"spatial attention ramp {ramp} N={N}")
    assert rel(p, ref) < BAR_ATTN
    print(f"spatial attention ramp {ramp} N={N}: worst |y - ref| / bound = {worst:.3f}")
