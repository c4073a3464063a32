"""ViT-B on the device: the reference golden, every stage against the oracle, and the kernel routes only it takes.

ViT-B (embed 768, 12 heads, features 128, out_channels [96, 192, 384, 768]; motion modules at C = 384, 768, 128, 128,
head dims 48, 96, 16, 16) is the one encoder whose 3x3 convs have 128 outputs outside the fused-resize path and whose
motion modules have N = 128 GEMMs, so it alone reaches, on the automatic route (vda_gemm.hip gemm_route):

  route                                                     held by
  phased conv 512x128 (cfg 5, launch_phased<4, 1, CONV>)     test_phased_conv_512x128, Clip B fus1 / fus2 / head
    per-lane tap decode (Cin % 64 != 0, vda_gemm_phased.h)   test_phased_conv_512x128[96-*], Clip B head (layer1_rn)
    the same decode in the 256x256 phased conv (cfg 4)       test_phased_conv_256x256_per_lane_taps
  implicit-GEMM conv 256x128 (cfg 1, 4096 <= M < 8192)       test_implicit_conv_256x128_automatic (+ cfg 1 in the lists
                                                             of test_gpu_fp16_edges.py)
  dense 512x128 (cfg 5) with every staged epilogue           test_gemm_512x128_epilogues, test_gemm_512x128_res_stats_out,
                                                             Clip B mm3, test_vitb_motion_module_routes[*-32]
  direct-load temporal attention at H = 8, D = 16 / 48 / 96  TEMPORAL in test_gpu_fp16_edges.py, mm0..3 here
  GroupNorm(32) at C = 384 / 768, unfused GroupNorm->Linear  GN_SHAPES, test_groupnorm_linear_unfused_vitb_widths
  the glue at these widths (no tap / head / oc1 fold, the    Clip A (all stages, fp16 and fp32 mode); the decisions
    q/k/v fold at C = 768 only, ps_cout = 96, C = 64 tail)   themselves: tests/test_vitb.py

Every kernel-level case is compared element by element with the float64 reference and bound of tests/fp16_bounds.py in
a sentinel-guarded output (test_gpu_fp16_edges.run_conv / run_gemm), and the automatic route's output is bit-identical
to the same call with that kernel forced (force_tile): the proof of which kernel the automatic route ran.  The phased
512x128 kernel runs the staged epilogue (t rounded to fp16, residuals added as packed fp16 vectors: staged=True) but
has no Phi table (TAB is XR == 2 only), so its GELU is gelu_erf: staged=True with phi_table=False
(test_gemm_phased_512x128_emulation_within_bound).

One premise of the case list did not survive reading gemm_route: the Cin = 8 conv (K = 72) does NOT take cfg 5 on the
automatic route, `K <= 256 && N < 256` gives it to the 128x64 tile (cfg 2) first.  The case stays: cfg 5 forced under
the staged bound, and the automatic route under the one-rounding bound, bit-identical to cfg 2 forced.

The stage tests reuse tests/test_gpu_stages.py's gpu_stage / hold and tests/stagelib.py unchanged: every slice within
4 x O16(all), fp32 mode within 1e-5; weights through round_weights(recipe_state_dict('vitb')).
* Clip A: B = 2, T = 3, 42 x 70 (3 x 5 patches): all of L.STAGES, fp16 and fp32 mode.
* Clip B: B = 1, T = 16, 154 x 196 (11 x 14 patches): fus1 (RCU convs at 16 x 44 x 56 = 39,424 rows: cfg 5 conv),
  fus2 (16 x 22 x 28 = 9,856 rows: cfg 5 conv), mm2 (2,464 rows), mm3 (9,856 rows: ff2 is dense cfg 5 with the in-place
  residual), head (layer1_rn 96 -> 128 at 39,424 rows: cfg 5 with the per-lane tap decode).
* The four motion modules alone at S = 16 x 16, B = 1, T = 16 (M = 4096): the LN-folded q/k/v route asserted taken at
  C = 768 and declined at C = 384 / 128; C = 128 also at T = 32 (M = 8192: ff2 reaches cfg 5 on its own).

CPU oracle time, measured on the MI355X machine at 16 threads: Clip B 3.4 .. 3.7 s in all over two runs (the clip's chain of stage inputs
1.5 s, then r and O16(all) of fus1 1.2 s, head 0.6 s, fus2 0.3 s, mm3 0.1 s, mm2 < 0.1 s), so T stays 16 and fus2 stays
on cfg 5; Clip A 0.5 s; the six motion-module references 0.8 s.  GPU time per test: 0.01 .. 0.6 s after the first
call of the model (Clip B fus1, the first to ask for the clip, 3.3 s with its oracle share); the golden test 2.6 s
(it builds the model); the kernel-level cases 0.02 .. 0.26 s each.  The whole file ran in 12 s.

Measured on MI355X (first run of these tests; nothing failed and no kernel changed).  Golden 1x4x70x98: fp16 3.6e-4,
fp32 mode 5.9e-7 rel-L1 against the reference; skip_tmp_block against the oracle 3.8e-4 / 5.8e-7.  Stages, worst over
outputs and slices, in test_gpu_stages.py's format:

    case                          stage                       E/bar        max/bar      fp32 E/1e-5
    ViT-B 2x3x42x70               encode                      0.25         0.27         0.12
                                  reassemble                  0.26         0.25         0.13
                                  mm0..3                      0.29..0.35   0.23..0.35   0.02..0.10
                                  fus4..1                     0.27..0.31   0.28..0.36   0.02..0.03
                                  head                        0.13         0.22         0.06
    ViT-B 1x16x154x196            fus1 / fus2 (cfg 5 conv)    0.30 / 0.32  0.32 / 0.36
                                  mm2 / mm3 (ff2 cfg 5)       0.35 / 0.36  0.34 / 0.45
                                  head (per-lane taps)        0.26         0.24
    ViT-B mm0..3, M=4096, S=256   C = 768 LN-folded q/k/v     0.35         0.36
                                  C = 384 / 128 LayerNorm     0.30..0.34   0.29..0.38
    ViT-B mm2 / mm3, M=8192       ff2 on cfg 5                0.32         0.30..0.35

Kernel-level cases, worst |y - ref| / bound: phased conv 512x128 0.75 (Cin 96), 0.68 .. 0.74 (Cin 128), 0.99 (Cin 8, cfg 5
forced and the automatic cfg 2); phased conv 256x256 with per-lane taps 0.75; implicit conv 256x128 0.75; dense 512x128
epilogues bias 0.75, gelu 0.72, gamma_res 0.93, res_res2 0.84, rowbias 0.80, strided_x 0.78; res + stats_out 0.84
(statistics 0.02).
"""
import functools
import os
import time

import pytest
import torch

import stagelib as L
import test_gpu_fp16_edges as E
import test_gpu_stages as GS
import vda_amd
import fp16_bounds as fb
from helpers import assert_elementwise, load_golden, recipe_state_dict, rel_l1, vda_oracle
from vda_amd import ops
from tunelib import tune_lib

pytestmark = pytest.mark.gpu
NAME = "vitb_t4_70x98"
ORACLE_SECONDS = {}
_NESTED = [0.0]


def timed(fn):
    """lru_cache'd oracle work; its own CPU time (without that of timed calls inside it) is kept per call in
    ORACLE_SECONDS and printed."""
    @functools.lru_cache(maxsize=None)
    def wrapper(*a):
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        outer, _NESTED[0] = _NESTED[0], 0.0
        t0 = time.perf_counter()
        out = fn(*a)
        whole = time.perf_counter() - t0
        own = ORACLE_SECONDS[(fn.__name__,) + a] = whole - _NESTED[0]
        _NESTED[0] = outer + whole
        print(f"oracle {fn.__name__}{a}: {own:.1f} s (file total {sum(ORACLE_SECONDS.values()):.1f} s)")
        return out
    return wrapper


# ---------------------------------------------------------------------------------------------
# the reference golden
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recipe_model():
    return vda_amd.build_model("vitb", recipe_state_dict("vitb"), device="cuda")


def test_vitb_forward_matches_reference_golden():
    """fp16 <= 1e-3 and fp32 <= 1e-5 rel-L1 against the reference's own forward (test_gpu_model.py's bars)."""
    x, depth, _, meta = load_golden(NAME)
    m = recipe_model()
    d16 = m(x.cuda()).float().cpu()
    d32 = m(x.cuda(), fp32=True).float().cpu()
    e16, e32 = rel_l1(d16, depth), rel_l1(d32, depth)
    print(f"{NAME}: rel-L1 vs reference fp16 {e16:.3e}, fp32 {e32:.3e}")
    assert d16.shape == depth.shape and bool(torch.isfinite(d16).all()) and bool(torch.isfinite(d32).all())
    assert e32 <= 1e-5
    assert e16 <= 1e-3


def test_vitb_forward_skip_tmp_block_matches_oracle():
    """skip_tmp_block=True (motion module 2 left out) against the oracle on the golden's clip, same bars."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x, _, _, _ = load_golden(NAME)
    ref = vda_oracle.forward(recipe_state_dict("vitb"), "vitb", x, skip_tmp_block=True)
    m = recipe_model()
    d16 = m(x.cuda(), skip_tmp_block=True).float().cpu()
    d32 = m(x.cuda(), skip_tmp_block=True, fp32=True).float().cpu()
    e16, e32 = rel_l1(d16, ref), rel_l1(d32, ref)
    print(f"{NAME} skip_tmp_block: rel-L1 vs oracle fp16 {e16:.3e}, fp32 {e32:.3e}")
    assert rel_l1(ref, vda_oracle.forward(recipe_state_dict("vitb"), "vitb", x)) > 1e-3  # the switch does something
    assert e32 <= 1e-5
    assert e16 <= 1e-3


# ---------------------------------------------------------------------------------------------
# every stage against the oracle
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    return L.round_weights(recipe_state_dict("vitb"))


@functools.lru_cache(maxsize=None)
def model():
    return vda_amd.build_model("vitb", weights(), device="cuda")


CLIPS = {"A": (2, 3, 42, 70, 61), "B": (1, 16, 154, 196, 62)}


@timed
def clip(name):
    B, T, H, W, seed = CLIPS[name]
    g = torch.Generator().manual_seed(seed)
    return L.Clip(weights(), "vitb", torch.randn(B, T, 3, H, W, generator=g))


@timed
def reference(name, stage):
    """(r, bars) of a stage of a clip: computed once, shared by the fp16 and fp32 tests, never modified."""
    return clip(name).bars(stage)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("stage", L.STAGES)
def test_vitb_every_stage(stage, fp32):
    """Clip A: the glue at ViT-B widths (projects to 96 / 192 / 384 / 768, ps_cout = 96, no tap / head / oc1 fold,
    unfused GroupNorm -> Linear at C = 384 / 768, the C = 64 depth tail), D = 48 / 96 / 16 attention inside mm0..3."""
    t0 = time.perf_counter()
    r, bars = reference("A", stage)
    t1 = time.perf_counter()
    GS.hold(f"vitb 2x3x42x70 {stage}", GS.gpu_stage(model(), clip("A"), stage, fp32), r, bars, fp32)
    print(f"vitb A {stage}: GPU stage + comparison {time.perf_counter() - t1:.2f} s (reference lookup {t1 - t0:.2f} s)")


@pytest.mark.parametrize("stage", ["fus1", "fus2", "mm2", "mm3", "head"])
def test_vitb_clip_b_large_routes(stage):
    """Clip B: the stages whose kernels are the cfg 5 conv (fus1, fus2; head: + the per-lane tap decode of layer1_rn)
    and the dense cfg 5 GEMM with the in-place residual (mm3's ff2), on the automatic route at rows >= 8192."""
    t0 = time.perf_counter()
    r, bars = reference("B", stage)
    t1 = time.perf_counter()
    GS.hold(f"vitb 1x16x154x196 {stage}", GS.gpu_stage(model(), clip("B"), stage), r, bars)
    print(f"vitb B {stage}: GPU stage + comparison {time.perf_counter() - t1:.2f} s (reference lookup {t1 - t0:.2f} s)")


@timed
def mm_reference(k, B, T):
    sd = weights()
    C = sd[f"head.motion_modules.{k}.temporal_transformer.proj_in.weight"].shape[0]
    g = torch.Generator().manual_seed(70 + k)
    x = L.r16(torch.randn(B * T, C, 16, 16, generator=g, dtype=torch.float64))
    pre = f"head.motion_modules.{k}."
    keys = {n: v for n, v in sd.items() if n.startswith(pre)}
    sd64 = L.cast(keys, torch.float64)
    r = L.run(lambda: L.O.temporal_module(sd64, pre, x, T))
    o = L.run(lambda: L.O.temporal_module(keys, pre, x.float(), T), "all")
    return x, r, L.Bars(o, r)


@pytest.mark.parametrize("k,T", [(0, 16), (1, 16), (2, 16), (3, 16), (2, 32), (3, 32)])
def test_vitb_motion_module_routes(k, T):
    """The four ViT-B motion modules alone on fp16 normal deviates at S = 16 x 16, B = 1: T = 16 (M = 4096: the
    LN-folded q/k/v GEMM, N = 2304 with three statistics parts, asserted taken at C = 768 and declined at C = 384 /
    128, which take LayerNorm + the row-bias GEMM), and C = 128 at T = 32 (M = 8192: ff2, N = 128, K = 512 with the
    in-place residual, is the dense phased 512x128 kernel; the last row of the PE table)."""
    m = model()
    P = m._pack(GS.dev(), False)
    q, S, B = P.mm[k], 256, 1
    assert q.C == (384, 768, 128, 128)[k]
    assert m._qkv_fold(q, B * T * S, S, T) == ([True, True] if k == 1 else [False, False])
    x, r, bars = mm_reference(k, B, T)
    y = m._temporal(q, L.map_to_rows(x), B, T, S)
    GS.hold(f"vitb mm{k} {B}x{T}x16x16", {"mm": L.map_from_rows(y, B * T, 16, 16)}, {"mm": r}, {"mm": bars})


# ---------------------------------------------------------------------------------------------
# kernel-level cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("BT,H,W", fb.VITB_CONV_SIZES)
@pytest.mark.parametrize("Cin", fb.VITB_CONV_CINS)
def test_phased_conv_512x128(Cin, BT, H, W):
    """The phased 512x128 implicit-GEMM conv (cfg 5, launch_phased<4, 1, CONV>), Cout = 128, plain / rcu1 / rcu2:
    Cin = 96 (K = 864: tap_uniform == false, the per-lane k / Cin decode, K tiles straddling taps, a last K tile of 32),
    128 (wave-uniform taps) and 8 (K = 72: two K tiles, both straddling taps); 1 x 91 x 91 (M = 8,281 = 16 x 512 + 89)
    and 2 x 64 x 64 (M = 8,192: whole tiles, the frame change on a tile edge).  cfg 5 forced under the staged bound;
    the automatic route (the tuning build at rest, and ops.conv2d with the same bits) is bit-identical to it for
    Cin = 96 / 128.  Cin = 8 has K <= 256, which gemm_route gives to the 128x64 tile before it looks at cfg 5: there
    the automatic route is held to the one-rounding bound and is bit-identical to cfg 2 forced."""
    worst = 0.0
    for mode in E.MODES:
        c = fb.vitb_conv_case(BT, Cin, H, W, mode)
        what = f"phased conv 512x128 {BT}x{H}x{W} Cin {Cin} {mode}"
        rb = E.conv_rb(c, True)
        out5, r5 = E.run_conv(c, dict(force_tile=5), True, what + " forced", rb=rb)
        if Cin == 8:
            auto, ra = E.run_conv(c, {}, False, what + " auto (cfg 2)", product=True)
            out2, _ = E.run_conv(c, dict(force_tile=2), False, what + " cfg 2 forced")
            assert torch.equal(auto, out2), f"{what}: K <= 256 no longer goes to the 128x64 tile"
        else:
            auto, ra = E.run_conv(c, {}, True, what + " auto", product=True, rb=rb)
            assert torch.equal(auto, out5), f"{what}: the automatic route is not the phased 512x128 conv"
        worst = max(worst, r5, ra)
    E.note(f"phased conv 512x128 {BT}x{H}x{W} Cin {Cin}", worst)


def test_phased_conv_256x256_per_lane_taps():
    """test_phased_conv_edge with the loader branch it does not reach: Cin = 96 -> 256 at 64 x 65 (M = 4160), rcu2,
    halo and strip routes off: the phased 256x256 conv (cfg 4) with tap_uniform == false.  Bit-identical to cfg 4
    forced."""
    c = fb.conv_case(1, 96, 256, 64, 65, "rcu2", seed=6)
    rb = E.conv_rb(c, True)
    out, worst = E.run_conv(c, dict(hconv=0, force_tile=-2), True, "phased conv 64x65 Cin 96", rb=rb)
    out4, _ = E.run_conv(c, dict(hconv=0, force_tile=4), True, "phased conv 64x65 Cin 96 cfg 4", rb=rb)
    assert torch.equal(out, out4), "force_tile = -2 did not take the phased 256x256 conv"
    E.note("phased conv 256x256 64x65 Cin 96", worst)


def test_implicit_conv_256x128_automatic():
    """The implicit-GEMM conv at 256x128 (cfg 1): N = 128 with 4096 <= M < 8192, ViT-B streaming one frame at 74 x 74
    (M = 5,476 = 21 x 256 + 100), Cin = 96 -> 128, plain / rcu1 / rcu2.  One rounding at the store; the automatic
    route (and ops.conv2d) is bit-identical to cfg 1 forced."""
    worst = 0.0
    for mode in E.MODES:
        c = fb.conv_case(1, 96, 128, 74, 74, mode, seed=74)
        rb = E.conv_rb(c, False)
        auto, r = E.run_conv(c, {}, False, f"implicit conv 256x128 74x74 {mode} auto", product=True, rb=rb)
        out1, _ = E.run_conv(c, dict(force_tile=1), False, f"implicit conv 256x128 74x74 {mode} forced", rb=rb)
        assert torch.equal(auto, out1), f"{mode}: the automatic route is not the 256x128 implicit-GEMM conv"
        worst = max(worst, r)
    E.note("implicit-GEMM conv 256x128 74x74 Cin 96", worst)


@pytest.mark.parametrize("epi", ["bias", "gelu", "gamma_res", "res_res2", "rowbias", "strided_x"])
def test_gemm_512x128_epilogues(epi):
    """The dense phased 512x128 kernel (cfg 5) on the AUTOMATIC route (N = 128, K = 512 > 256, M >= 8192: ViT-B's ff2)
    at M = 8,193 (a one-row last M tile), on 3 persistent blocks.  Register epilogues are 256x256-only, so every
    epilogue here is the staged code at XR = 4: bias, bias + GELU (gelu_erf: no Phi table at XR = 4), gamma + the
    in-place residual, two residuals in wider buffers, the per-frame row bias (frames of 300 rows: every tile spans
    frame changes), x as the middle third of a [M, 3K] buffer.  Staged bound; bit-identical to cfg 5 forced."""
    T = tune_lib()
    M, N, K = 8193, 128, 512
    c = fb.gemm_case(M, N, K, epi, seed=N + len(epi))
    if epi == "rowbias":
        c["kw"].update(rdiv=300)
    rb = fb.gemm_ref_bound(c["x"], c["w"], staged=True, phi_table=False, **c["kw"])
    with T.route(gemm_sched=3):
        worst = E.run_gemm(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk), f"gemm 512x128 {epi}", ref_bound=rb,
                           align16=True, staged=True, same_as=E.forced(T, 5, gemm_sched=3))
    E.note(f"gemm phased 512x128 epilogue {epi}", worst)


def test_gemm_512x128_res_stats_out():
    """res (in place, as the motion module's residual stream) + stats_out at M = 8,193, N = 128, K = 512: cfg 5's staged
    epilogue does not form row statistics (store_with_stats is 256x256-only), the separate partial-sum kernel does:
    [M, 1, 2] (sum, sum of squares) over the 128 stored columns against float64 sums of the kernel's own output
    (fp16_bounds.row_stats_ref_bound, part = 128), the NaN spare row after row M - 1 untouched.  Output and
    statistics bit-identical to cfg 5 forced, and so is ops.gemm (the product library) on the same call."""
    T = tune_lib()
    M, N, K = 8193, 128, 512
    c = fb.gemm_case(M, N, K, "gamma_res", seed=N)
    del c["kw"]["gamma"]
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], staged=True, **c["kw"])
    x, w, bias = E.h(c["x"]), E.h(c["w"]), E.f32(c["kw"]["bias"])
    outs = []
    for knobs in (dict(gemm_sched=3), dict(gemm_sched=3, force_tile=5)):
        buf, out = E.framed2d(M, N)
        out.copy_(E.h(c["kw"]["res"]))
        stats = torch.full((M + 1, 1, 2), float("nan"), device=E.DEV, dtype=torch.float32)
        with T.route(**knobs):
            T.gemm_kw(x, w, out, bias=bias, res=out, stats_out=stats)
        assert E.frame2d_ok(buf, M, N), "a store outside the output"
        outs.append((out, stats))
    (out, stats), (out5, stats5) = outs
    worst = assert_elementwise(out, ref, bound, "gemm 512x128 res+stats")
    assert E.rel(out, ref) < E.BAR_GEMM
    assert torch.equal(out, out5) and torch.equal(stats[:M], stats5[:M]), "the automatic route is not the phased 512x128 kernel"
    prod = E.h(c["kw"]["res"])  # the product library, as _temporal calls ff2: res aliasing out
    ops.gemm(x, w, bias=bias, res=prod, out=prod)
    assert torch.equal(prod, out5), "ops.gemm is not the phased 512x128 kernel"
    sref, sbound = fb.row_stats_ref_bound(out, part=128)
    assert bool(torch.isnan(stats[M]).all()), "the spare statistics row was written"
    ws = assert_elementwise(stats[:M], sref, sbound, "stats_out N=128")
    E.note(f"gemm phased 512x128 res+stats (stats {ws:.3f})", worst)
