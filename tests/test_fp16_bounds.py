"""CPU proof that the per-element bounds of tests/fp16_bounds.py are not too tight.

For every case family of tests/test_gpu_fp16_edges.py and tests/test_gpu_fp16_small_ops.py, a CPU emulation of the kernel's arithmetic (fp32
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


@pytest.mark.parametrize("epi", ["gelu", "gamma_res", "res_res2"])
def test_gemm_phased_512x128_emulation_within_bound(epi):
    """The phased 512x128 kernel (XR = 4, ViT-B's N = 128 GEMMs) runs the staged epilogue (t rounded to fp16, then
    packed fp16 residual adds) but has no Phi table (TAB is XR == 2 only): its GELU is gelu_erf.  That pair of
    forms, staged=True with phi_table=False, at N = 128."""
    worst = 0.0
    for M, K in [(1, 8), (129, 40), (257, 512)]:
        c = fb.gemm_case(M, 128, K, epi, seed=M)
        ref, bound = fb.gemm_ref_bound(c["x"], c["w"], staged=True, phi_table=False, **c["kw"])
        worst = max(worst, assert_elementwise(fb.emulate_gemm(c["x"], c["w"], staged=True, phi_table=False, **c["kw"]),
                                              ref, bound, f"gemm 512x128 {epi} {M}x128x{K}"))
    print(f"gemm 512x128 staged {epi}: worst emulation |y - ref| / bound = {worst:.3f}")
    assert worst > 0.05


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
    y = (fb.rnd16(257, 128, seed=5) * 3 + 0.5).half()  # a row narrower than a part (N = 128): one 128-term part
    ref, bound = fb.row_stats_ref_bound(y, part=128)
    assert ref.shape == (257, 1, 2)
    emu = y.float()
    assert_elementwise(torch.stack([emu.sum(-1), (emu * emu).sum(-1)], -1)[:, None], ref, bound, "stats_out partials N=128")


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
    ("phased conv 512x128 Cin 96 rcu2", dict(BT=2, Cin=96, Cout=128, H=12, W=13, mode="rcu2"), True),
    ("phased conv 512x128 Cin 8 rcu1", dict(BT=2, Cin=8, Cout=128, H=12, W=13, mode="rcu1"), True),
    ("phased conv 256x256 Cin 96 rcu2", dict(BT=1, Cin=96, Cout=256, H=12, W=13, mode="rcu2"), True),
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
@pytest.mark.parametrize("T,D", [(1, 32), (2, 8), (31, 64), (32, 128), (32, 24), (2, 16), (32, 16), (31, 96), (32, 96), (32, 48)])
def test_temporal_attention_emulation_within_bound(T, D, rope):
    B, S, H = 1, 3, 3
    qkv = fb.rnd16(B * T * S, 3 * H * D, seed=T + D) * 2
    ref, bound = fb.temporal_attn_ref_bound(qkv, B, T, S, H, D, rope)
    worst = assert_elementwise(fb.emulate_temporal_attn(qkv, B, T, S, H, D, rope), ref, bound, f"temporal T={T} D={D}")
    print(f"temporal attention T={T} D={D} rope={rope}: worst emulation ratio {worst:.3f}")
    # T = 1: the output is v exactly.  With RoPE the fp16 rounding of the rotated q and k can only be carried as
    # a worst case through the softmax (fp16_bounds.temporal_attn_ref_bound): that bound is ~10x looser
    assert T == 1 or worst > (0.02 if rope else 0.05)


# =====================================================================================================
# LayerNorm, GroupNorm, GroupNorm -> Linear, resize, depth tail: the cases of tests/test_gpu_fp16_small_ops.py.
# Every emulation inside its bound; for every bound one deliberately wrong emulation (a MUTANT: these exist
# only here, as CPU arithmetic) outside it on the same inputs.
# =====================================================================================================
def outside(y, ref, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_elementwise(y, ref, bound, what)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("C", fb.LN_CS)
def test_layernorm_emulation_within_bound(C, eps):
    x = fb.ln_rows(33, C)
    g, b = fb.gn_affine(C, seed=C)
    ref, bound = fb.layernorm_ref_bound(x, g, b, eps)
    worst = assert_elementwise(fb.emulate_layernorm(x, g, b, eps), ref, bound, f"layernorm C={C}")
    sref, sbound = fb.ln_stats_ref_bound(x, eps)
    ws = assert_elementwise(fb.emulate_layernorm(x, g, b, eps, stats_only=True), sref, sbound, f"row_stats C={C}")
    print(f"layernorm C={C} eps={eps}: worst emulation ratio {worst:.3f}, statistics {ws:.3f}")
    assert worst > 0.05
    # MUTANT: the last lane of the row left out of both reductions (a narrow row's shuffle one level short)
    lane = min(C // 8, 64) - 1
    outside(fb.emulate_layernorm(x, g, b, eps, drop_lane=lane), ref, bound, "layernorm, a lane dropped")
    outside(fb.emulate_layernorm(x, g, b, eps, stats_only=True, drop_lane=lane), sref, sbound, "row_stats, a lane dropped")


@pytest.mark.parametrize("Fr", fb.GN_FRAMES)
@pytest.mark.parametrize("C,groups", fb.GN_SHAPES)
def test_groupnorm_emulations_within_bound(C, groups, Fr):
    g, b = fb.gn_affine(C, seed=C)
    worst = wstat = 0.0
    for S in fb.GN_S:
        x = fb.gn_case(Fr, S, C)
        ref, bound = fb.groupnorm_ref_bound(x, g, b, groups, 1e-6)
        sref, sbound = fb.gn_stats_ref_bound(x, groups, 1e-6)
        what = f"groupnorm C={C} S={S} F={Fr}"
        worst = max(worst, assert_elementwise(fb.emulate_groupnorm_two_pass(x, g, b, groups, 1e-6), ref, bound, what + " two-pass"),
                    assert_elementwise(fb.emulate_groupnorm_ws(x, g, b, groups, 1e-6), ref, bound, what + " workspace"))
        wstat = max(wstat, assert_elementwise(fb.emulate_groupnorm_ws(x, g, b, groups, 1e-6, stats_only=True), sref, sbound,
                                              what + " statistics"))
    print(f"groupnorm C={C} groups={groups} F={Fr}: worst emulation ratio {worst:.3f}, statistics {wstat:.3f}")
    assert worst > 0.05


def test_groupnorm_apply_mutant_outside_bound():
    """MUTANT: gn_apply reading the statistics of its chunk's first channel's group for all eight channels, wrong
    for the groups that share a 16-byte chunk (cg = 6: C = 24, 4 groups; cg = 12: C = 48).  (gn_apply's `of`
    formed without its fma is one more fp32 rounding of the same size as those the bound already counts: a derived
    bound does not tell the two apart, and torch.equal between the fused GroupNorm -> Linear and the composition
    is what pins those bits.)"""
    for C in (24, 48):
        x = fb.gn_case(3, 33, C)
        x[:, :, C // 2:] *= 3.0  # groups of different spread
        g, b = fb.gn_affine(C, seed=1)
        ref, bound = fb.groupnorm_ref_bound(x, g, b, 4, 1e-6)
        assert_elementwise(fb.emulate_groupnorm_ws(x, g, b, 4, 1e-6), ref, bound, f"C={C}")
        outside(fb.emulate_groupnorm_ws(x, g, b, 4, 1e-6, chunk_group=True), ref, bound, f"C={C}, the chunk's group")


@pytest.mark.parametrize("kind", fb.GN_OUTLIER_KINDS)
@pytest.mark.parametrize("S,C,v0", fb.GN_OUTLIER_SIZES)
def test_groupnorm_outlier_first_value_shift_is_outside_bound(S, C, v0, kind):
    """The finding.  On a frame with a massive activation both two-pass orders (groupnorm_kernel's, and the
    chunk-local two-pass + merge the workspace route now runs) stay inside groupnorm_ref_bound, output and
    statistics.  The first-value shift the workspace route used before does not, whenever the outlier sits AT
    the shift position: that is what the GPU test would have shown against the parent library."""
    x, fo = fb.gn_outlier_case(S, C, v0, kind)
    g, b = fb.gn_affine(C, seed=C)
    ref, bound = fb.groupnorm_ref_bound(x, g, b, 32, 1e-6)
    sref, sbound = fb.gn_stats_ref_bound(x, 32, 1e-6)
    what = f"groupnorm outlier S={S} C={C} v0={v0} {kind}"
    assert float(ref.abs().max()) < 1000 and float(ref.abs().max()) > 30
    w2 = assert_elementwise(fb.emulate_groupnorm_two_pass(x, g, b, 32, 1e-6), ref, bound, what + " two-pass")
    ww = assert_elementwise(fb.emulate_groupnorm_ws(x, g, b, 32, 1e-6), ref, bound, what + " workspace")
    st = fb.emulate_groupnorm_ws(x, g, b, 32, 1e-6, stats_only=True)
    wstat = assert_elementwise(st, sref, sbound, what + " workspace statistics")
    old = fb.emulate_groupnorm_ws_first_value_shift(x, g, b, 32, 1e-6, stats_only=True)
    err = lambda s: float(((s[fo, 0, 1].double() - sref[fo, 0, 1]) / sref[fo, 0, 1]).abs())  # noqa: E731
    print(f"{what}: two-pass {w2:.3f}, workspace {ww:.3f} (statistics {wstat:.3f}); relative rstd error of group 0: "
          f"workspace {err(st):.1e}, first-value shift {err(old):.1e}")
    yold = fb.emulate_groupnorm_ws_first_value_shift(x, g, b, 32, 1e-6)
    if kind == "middle":  # the shift is an ordinary value: the old route was right here too
        assert_elementwise(yold, ref, bound, what + " first-value shift")
    else:
        outside(yold, ref, bound, what + " first-value shift")
        outside(old, sref, sbound, what + " first-value shift statistics")


@pytest.mark.parametrize("C,S,Fr", fb.GNL_CASES)
def test_groupnorm_linear_emulation_within_bound(C, S, Fr):
    x = fb.gn_case(Fr, S, C, seed=3)
    g, b = fb.gn_affine(C, seed=C)
    w, bias = fb.rnd16(C, C, scale=C ** -0.5, seed=C + 1), fb.rnd32(C, scale=0.1, seed=C + 2)
    ref, bound = fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, bias)
    worst = assert_elementwise(fb.emulate_groupnorm_linear(x, g, b, 32, 1e-6, w, bias), ref, bound, f"gn_linear C={C} S={S} F={Fr}")
    print(f"groupnorm_linear C={C} S={S} F={Fr}: worst emulation ratio {worst:.3f}")
    if Fr * S > 5:  # MUTANT: one 8-channel chunk (a lane group's share of a k-step) left out of rows m % 16 == 5
        outside(fb.emulate_groupnorm_linear(x, g, b, 32, 1e-6, w, bias, drop=(32, 40)), ref, bound, "gn_linear, a chunk dropped")


def test_groupnorm_linear_outlier_emulation_within_bound():
    S, C, v0 = fb.GN_OUTLIER_SIZES[0]
    x, _ = fb.gn_outlier_case(S, C, v0, "first_frame1of3")
    x = x[:2]
    g, b = fb.gn_affine(C, seed=C)
    w, bias = fb.rnd16(C, C, scale=C ** -0.5, seed=C + 1), fb.rnd32(C, scale=0.1, seed=C + 2)
    ref, bound = fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, bias)
    assert_elementwise(fb.emulate_groupnorm_linear(x, g, b, 32, 1e-6, w, bias), ref, bound, "gn_linear outlier frame")


@pytest.mark.parametrize("kind", ["rand", "checker"])
@pytest.mark.parametrize("BT,H,W,C,Ho,Wo", fb.UPSAMPLE_CASES)
def test_upsample_emulation_within_bound(BT, H, W, C, Ho, Wo, kind):
    x = fb.upsample_input(BT, H, W, C, kind)
    ref, bound = fb.upsample_ref_bound(x, Ho, Wo)
    worst = assert_elementwise(fb.emulate_upsample(x, Ho, Wo), ref, bound, f"resize {H}x{W}->{Ho}x{Wo} C={C} {kind}")
    print(f"resize {BT}x{H}x{W}x{C} -> {Ho}x{Wo} {kind}: worst emulation ratio {worst:.3f}")
    # MUTANT: the second row of a pair keeps the first row's source rows.  It shows wherever some pair does not
    # share them (and the source has more than one distinct row)
    if H > 1 and Ho > 1 and (Ho < 2 * H or BT * Ho > Ho):
        y = fb.emulate_upsample(x, Ho, Wo, stale_pair=True)
        if not torch.equal(y, fb.emulate_upsample(x, Ho, Wo)):
            outside(y, ref, bound, "resize, a stale row pair")


def test_upsample_stale_pair_mutant_is_caught_where_it_matters():
    for BT, H, W, C, Ho, Wo in [(2, 37, 37, 8, 19, 19), (3, 4, 5, 40, 9, 6), (2, 19, 19, 32, 37, 37)]:
        x = fb.upsample_input(BT, H, W, C)
        ref, bound = fb.upsample_ref_bound(x, Ho, Wo)
        outside(fb.emulate_upsample(x, Ho, Wo, stale_pair=True), ref, bound, "resize, a stale row pair")


def test_im2col_references():
    """The exact references against torch's own unfold (they are index gathers: any disagreement is a bug here)."""
    import torch.nn.functional as F
    img = fb.rnd32(2, 3, 28, 42, seed=1)
    a = fb.patch_im2col_ref(img, 592).view(2, 7, 592)
    u = F.unfold(img, 14, stride=14).transpose(1, 2).half()  # [BT, np, 588], k = (ci, ky, kx)
    assert torch.equal(a[:, 1:, :588], u) and float(a[:, 0].abs().max()) == 0 and float(a[:, :, 588:].abs().max()) == 0
    x = fb.rnd16(2, 5, 6, 8, seed=2)
    for ks, stride, pad in [(3, 2, 1), (3, 1, 1), (1, 1, 0), (3, 2, 0)]:
        a = fb.conv_im2col_ref(x, ks, stride, pad)
        u = F.unfold(x.permute(0, 3, 1, 2), ks, padding=pad, stride=stride)  # [BT, C ks ks, L], k = (ci, ky, kx)
        u = u.view(2, 8, ks * ks, -1).permute(0, 3, 2, 1).reshape(a.shape)
        assert torch.equal(a, u)


@pytest.mark.parametrize("C,Hin,Win,Ho,Wo", fb.DEPTH_CASES)
def test_depth_head_emulation_within_bound(C, Hin, Win, Ho, Wo):
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hin, Win, 2, seed=C)
    ref, bound = fb.depth_head_ref_bound(x, w1, b1, w2, b2, Ho, Wo)
    worst = assert_elementwise(fb.emulate_depth_head(x, w1, b1, w2, b2, Ho, Wo), ref, bound, f"depth tail C={C} {Hin}x{Win}->{Ho}x{Wo}")
    print(f"depth tail C={C} {Hin}x{Win} -> {Ho}x{Wo}: worst emulation ratio {worst:.3f}")
    # MUTANT: the ReLU between the two convs left out.  (The bound is gamma(9 C + 3) of the absolute image, the
    # any-order fp32 bound at K = 9 C up to 1,152: ~1e-3 of the output, far above what the MFMA chain really loses,
    # so it cannot see a dropped lo half of the weights; the rel-L1 1e-5 bar the GPU test keeps beside it does.)
    outside(fb.emulate_depth_head(x, w1, b1, w2, b2, Ho, Wo, no_relu=True), ref, bound, "depth tail without the inner ReLU")
