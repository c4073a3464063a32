"""CPU proof that the per-element bounds of tests/fp16_bounds.py are not too tight.

For every case family of tests/test_gpu_fp16_edges.py, a CPU emulation of the kernel's arithmetic (fp32
accumulation in torch's own order, .half() exactly at the kernel's rounding points) must lie inside the
bound of the float64 reference at EVERY element.  The bounds are derived (fp16_bounds.py), so an emulation
outside one means the derivation is wrong, not that a factor needs widening.  The worst ratio of each family
is printed (pytest -s).  assert_elementwise itself is checked on a planted error.
"""
import pytest
import torch

import fp16_bounds as fb
from helpers import assert_elementwise


def test_assert_elementwise_reports_the_element():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    y = ref.clone().half()
    assert assert_elementwise(y, ref, bound, "clean") == 0.0
    y[1, 2, 0, 3] = 0.01
    y[0, 1, 1, 1] = 0.002
    with pytest.raises(AssertionError, match=r"2 of 120 elements.*index \(1, 2, 0, 3\).*first violation at \(0, 1, 1, 1\)"):
        assert_elementwise(y, ref, bound, "planted")
    y[0, 0, 0, 0] = float("nan")  # a NaN is the worst violation, not a pass
    with pytest.raises(AssertionError, match=r"3 of 120.*index \(0, 0, 0, 0\)"):
        assert_elementwise(y, ref, bound, "nan")


@pytest.mark.parametrize("staged", [False, True], ids=["tile", "phased"])
@pytest.mark.parametrize("epi", fb.GEMM_EPIS)
def test_gemm_emulation_within_bound(epi, staged):
    """phased: the staged residual adds and, for GELU / GEGLU, the Phi table of the 256x256 kernels (the emulation
    evaluates the very table of csrc/phi_table.h)."""
    worst = 0.0
    for M, N, K in [(1, 32, 8), (127, 56, 24), (129, 136, 40), (257, 264, 160), (65, 128, 96)]:
        c = fb.gemm_case(M, N, K, epi, seed=M)
        ref, bound = fb.gemm_ref_bound(c["x"], c["w"], staged=staged, phi_table=staged, **c["kw"])
        worst = max(worst, assert_elementwise(fb.emulate_gemm(c["x"], c["w"], staged=staged, phi_table=staged, **c["kw"]),
                                              ref, bound, f"gemm {epi} {M}x{N}x{K}"))
    print(f"gemm {epi} staged={staged}: worst emulation |y - ref| / bound = {worst:.3f}")
    assert worst > 0.05  # the bound is within a small factor of what fp16 arithmetic really does


@pytest.mark.parametrize("kind", fb.LN_KINDS)
def test_gemm_ln_fold_emulation_within_bound(kind):
    c = fb.gemm_ln_case(257, 256, 192, kind, seed=3)
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], phi_table=True, **c["kw"])
    worst = assert_elementwise(fb.emulate_gemm(c["x"], c["w"], phi_table=True, **c["kw"]), ref, bound, f"gemm {kind}")
    print(f"gemm {kind}: worst emulation |y - ref| / bound = {worst:.3f}")
    assert worst > 0.05


def test_phi_table_within_its_documented_error():
    """The table the emulation reads is the one the bound's 1.27e-6 speaks of."""
    x = torch.linspace(-8, 8, 200001, dtype=torch.float64)
    tab = fb.phi_table().double()
    idx = (torch.round(x * 128) + 1024).clamp(0, 2047).long()
    phi = 0.5 * torch.erfc(-x * 0.5 ** 0.5)
    assert float((tab[idx, 0] + tab[idx, 1] * x - phi).abs().max()) <= 1.27e-6


def test_row_stats_emulation_within_bound():
    y = (fb.rnd16(257, 512, seed=4) * 3 + 0.5).half()
    ref, bound = fb.row_stats_ref_bound(y)
    worst = assert_elementwise(fb.emulate_row_stats(y), ref, bound, "stats_out partials")
    print(f"stats_out partials: worst emulation ratio {worst:.3f}")


CONV_CASES = [
    ("hconv/strip plain", dict(BT=2, Cin=64, Cout=256, H=9, W=33, mode="plain"), True),
    ("hconv/strip rcu1", dict(BT=2, Cin=64, Cout=256, H=9, W=33, mode="rcu1"), True),
    ("hconv/strip rcu2", dict(BT=2, Cin=128, Cout=256, H=17, W=19, mode="rcu2"), True),
    ("hconv res2 upsampled", dict(BT=1, Cin=64, Cout=256, H=17, W=23, mode="rcu2", res2_src=(9, 12)), True),
    ("hconv res2 from 1x1", dict(BT=1, Cin=64, Cout=256, H=9, W=11, mode="rcu2", res2_src=(1, 1)), True),
    ("implicit gemm rcu2", dict(BT=2, Cin=8, Cout=32, H=9, W=11, mode="rcu2"), False),
    ("implicit gemm s2", dict(BT=2, Cin=64, Cout=128, H=9, W=11, mode="rcu1", stride=2), False),
    ("implicit gemm 1x1", dict(BT=2, Cin=64, Cout=128, H=2, W=3, mode="rcu2", ks=1), False),
    ("phased conv rcu2", dict(BT=1, Cin=64, Cout=256, H=12, W=13, mode="rcu2"), True),
    ("resize + conv", dict(BT=2, Cin=64, Cout=128, H=8, W=20, mode="rcu1", up=(33, 47)), False),
]


@pytest.mark.parametrize("name,shape,staged", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_emulation_within_bound(name, shape, staged):
    c = fb.conv_case(**shape)
    if shape.get("up"):
        c["kw"]["pre_relu"] = False  # the resize routes take no pre-ReLU
    if "1x1" in name:
        c["kw"]["framebias"] = fb.rnd32(3, shape["Cout"], seed=9)
    ref, bound = fb.conv_ref_bound(c["x"], c["w"], staged=staged, **c["kw"])
    worst = assert_elementwise(fb.emulate_conv(c["x"], c["w"], staged=staged, **c["kw"]), ref, bound, name)
    print(f"conv {name}: worst emulation |y - ref| / bound = {worst:.3f}")
    assert worst > 0.05


@pytest.mark.parametrize("round1", [False, True], ids=["mfma32", "round1"])
@pytest.mark.parametrize("N", [1, 31, 33, 65, 129, 257])
def test_spatial_attention_emulation_within_bound(N, round1):
    B, H = 2, 3
    qkv = fb.rnd16(B * N, 3 * H * 64, seed=N)
    ref, bound = fb.spatial_attn_ref_bound(qkv, B, N, H)
    worst = assert_elementwise(fb.emulate_spatial_attn(qkv, B, N, H, round1=round1), ref, bound, f"spatial attention N={N}")
    print(f"spatial attention N={N} round1={round1}: worst emulation ratio {worst:.3f}")
    assert N == 1 or worst > 0.05  # N = 1: softmax of one key, the output is v exactly


@pytest.mark.parametrize("ramp", ["up", "spike", "down"])
def test_spatial_attention_ramps_emulation_within_bound(ramp):
    B, N, H = 2, 129, 2
    qkv = fb.attn_ramp_qkv(ramp, B, N, H)
    ref, bound = fb.spatial_attn_ref_bound(qkv, B, N, H)
    worst = 0.0
    for round1 in (False, True):
        worst = max(worst, assert_elementwise(fb.emulate_spatial_attn(qkv, B, N, H, round1=round1), ref, bound,
                                              f"spatial attention {ramp}"))
    print(f"spatial attention ramp {ramp}: worst emulation ratio {worst:.3f}")
    assert worst > 0.05


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("T,D", [(1, 32), (2, 8), (31, 64), (32, 128), (32, 24)])
def test_temporal_attention_emulation_within_bound(T, D, rope):
    B, S, H = 1, 3, 3
    qkv = fb.rnd16(B * T * S, 3 * H * D, seed=T + D) * 2
    ref, bound = fb.temporal_attn_ref_bound(qkv, B, T, S, H, D, rope)
    worst = assert_elementwise(fb.emulate_temporal_attn(qkv, B, T, S, H, D, rope), ref, bound, f"temporal T={T} D={D}")
    print(f"temporal attention T={T} D={D} rope={rope}: worst emulation ratio {worst:.3f}")
    # T = 1: the output is v exactly.  With RoPE the fp16 rounding of the rotated q and k can only be carried as
    # a worst case through the softmax (fp16_bounds.temporal_attn_ref_bound): that bound is ~10x looser
    assert T == 1 or worst > (0.02 if rope else 0.05)
