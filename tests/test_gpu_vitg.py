"""ViT-g on the device: the SwiGLU GEMM epilogue, temporal attention at head dims up to 192, the reduced-depth model.

  * SwiGLU GEMM (VDA_ACT_SWIGLU), every element against the derived bound of tests/swiglu_bounds.py, on the (M, N, K)
    grid tests/test_gpu_fp16_edges.py runs for GEGLU: every one-tile-per-block configuration and the automatic
    choice, the phased 256x256 kernel's staged epilogue with and without the LayerNorm fold at M = 4097, K = 192, the
    model's depth (300, 8192, 1536), and gate pre-activations planted at +-30 / +-100.  The output is a view inside a
    NaN-filled buffer whose frame (canary rows after the output included) must stay NaN.
  * vda_gemm_f32's SwiGLU branch with the comparison tests/test_gpu_fp32_ops.py uses for GEGLU.
  * Temporal attention at D = 136 .. 192 against fp16_bounds.temporal_attn_ref_bound, each route forced through the
    tuning build; the fp32 entry point at D = 192 and 130.
  * The d4 model (4 blocks, taps [0, 1, 2, 3]) against the reference-generated golden, fp16 and fp32.

Measured on an MI355X (pytest -s prints them): worst |y - ref| / bound 0.98 over the tile grid, 0.76 .. 0.81 on the
phased kernel, 0.98 / 0.97 with the planted gate values, 0.05 .. 0.34 for temporal attention; the d4 model 3.8e-4
(fp16) and 9.0e-7 (fp32) rel-L1 against the reference.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vda_amd
from vda_amd import ops
from vda_amd import model as vm
from vda_amd._lib import ACT_SWIGLU
from vda_amd.model import _geglu_interleave
from vda_amd.weights import synthetic_state_dict
import fp16_bounds as fb
import swiglu_bounds as sb
from helpers import GOLDEN, assert_elementwise, load_golden, recipe_state_dict, rel_l1
from tunelib import tune_lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_GEMM, BAR_ATTN = 2e-3, 3e-3
TILES = {0: (128, 128), 1: (256, 128), 2: (128, 64), 3: (256, 256), 6: (64, 64), 7: (64, 128)}
SENT = -7776.0
GUARD = 1024


def h(t):
    return t.to(DEV, torch.float16).contiguous()


def f32(t):
    return t.to(DEV, torch.float32).contiguous()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def nan_framed(M, N):
    """An [M, N] view with 4 NaN canary rows above / below and 8 NaN columns left / right (16-byte aligned rows)."""
    buf = torch.full((M + 8, N + 16), float("nan"), device=DEV, dtype=torch.float16)
    return buf, buf[4:4 + M, 8:8 + N]


def frame_is_nan(buf, M, N):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[4:4 + M, 8:8 + N] = False
    return bool(torch.isnan(buf[mask]).all())


def legal_ns(BN):  # test_gpu_fp16_edges.legal_ns for the gated epilogues: N % 32 == 0
    return sorted({32, max(BN - 32, 32), BN, BN + 32})


def il(a, b):
    return _geglu_interleave(torch.cat([a, b]))


def run_swiglu(c, launch, what, staged=False, same_as=None):
    """One SwiGLU case (swiglu_bounds.swiglu_case / swiglu_ln_case / planted_case) through `launch(x, w, out, gk)`."""
    M, N, kw = c["M"], c["N"], c["kw"]
    ln = kw.get("ln")
    ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], staged=staged, **kw)
    x, w = h(c["x"]), h(il(c["w"], kw["wg"]))
    gk = dict(bias=f32(il(kw["bias"], kw["bg"])), act=ACT_SWIGLU)
    if ln is not None:
        parts = ln["parts"].shape[1] if "parts" in ln else 0
        gk.update(ln_stats=f32(ln["parts"] if parts else torch.stack([ln["mean"], ln["rstd"]], -1)),
                  ln_colsum=f32(il(ln["colsum"], ln["colsum_g"])), ln_parts=parts, ln_eps=1e-6)
    buf, out = nan_framed(M, N // 2)
    launch(x, w, out, gk)
    worst = assert_elementwise(out, ref, bound, what)
    assert rel(out, ref) < BAR_GEMM, what
    assert frame_is_nan(buf, M, N // 2), f"{what}: a store outside the output"
    if same_as is not None:
        buf2, out2 = nan_framed(M, N // 2)
        same_as(x, w, out2, gk)
        assert torch.equal(out, out2), f"{what}: the automatic route is not the kernel this case is about"
    return worst


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 6, 7, "auto"])
def test_swiglu_tile_edges(cfg):
    """test_gemm_tile_edges' grid for the gated epilogue: M in {1, BM - 1, BM, BM + 1}, N in {32, BN - 32, BN, BN + 32}
    (N tails inside a 16-row [h | g] block pair), K in {8, 24, 32, 40, 96, 160}."""
    T = tune_lib()
    BM, BN = TILES.get(cfg, (128, 128))
    worst = 0.0
    for M in (1, BM - 1, BM, BM + 1):
        for N in legal_ns(BN):
            for K in (8, 24, 32, 40, 96, 160):
                c = sb.swiglu_case(M, N, K, seed=M + N + K)
                if cfg == "auto":
                    worst = max(worst, run_swiglu(c, lambda x, w, out, gk: ops.gemm(x, w, out=out, **gk),
                                                  f"swiglu auto {M}x{N}x{K}"))
                else:
                    with T.route(force_tile=cfg):
                        worst = max(worst, run_swiglu(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk),
                                                      f"swiglu cfg {cfg} {M}x{N}x{K}"))
    print(f"swiglu tile cfg {cfg}: worst |y - ref| / bound = {worst:.3f}")


def forced(T, cfg, **knobs):
    def launch(x, w, out, gk):
        with T.route(force_tile=cfg, **knobs):
            T.gemm_kw(x, w, out, **gk)
    return launch


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("kind", ["plain", "ln", "ln_parts"])
def test_swiglu_phased(kind, N):
    """The phased 256x256 kernel's staged epilogue (test_gemm_phased_epilogues / test_gemm_phased_ln_fold's geglu and
    ln_geglu cases): M = 4097 (a one-row last M tile), K = 192 (every prologue case), 3 persistent blocks; without the
    LayerNorm fold, with [M, 2] (mean, rstd) statistics and with three-part (sum, sum of squares) statistics.
    Bit-identical to cfg 4 forced: the automatic route took the phased kernel."""
    T = tune_lib()
    M, K = 4097, 192
    c = sb.swiglu_case(M, N, K, seed=N) if kind == "plain" else sb.swiglu_ln_case(M, N, K, seed=N, parts=kind == "ln_parts")
    c.update(M=M, N=N)
    with T.route(gemm_sched=3):
        worst = run_swiglu(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk), f"swiglu phased {kind} N={N}", staged=True,
                           same_as=forced(T, 4, gemm_sched=3))
    print(f"swiglu phased {kind} N={N}: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("cfg", [0, 3, "auto"])
def test_swiglu_tile_ln_fold(cfg):
    """The LayerNorm fold on the one-tile-per-block kernels (epi_geglu4's sibling): M = 257 < 4096 rows."""
    T = tune_lib()
    worst = 0.0
    for parts in (False, True):
        c = sb.swiglu_ln_case(257, 288, 192, seed=7, parts=parts)
        c.update(M=257, N=288)
        if cfg == "auto":
            worst = max(worst, run_swiglu(c, lambda x, w, out, gk: ops.gemm(x, w, out=out, **gk), f"swiglu LN auto parts={parts}"))
        else:
            with T.route(force_tile=cfg):
                worst = max(worst, run_swiglu(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk),
                                              f"swiglu LN cfg {cfg} parts={parts}"))
    print(f"swiglu tile LN fold cfg {cfg}: worst |y - ref| / bound = {worst:.3f}")


def test_swiglu_model_depth():
    """ViT-g's w12 GEMM at the model's depth, (M, N, K) = (300, 8192, 1536), norm2 folded in, automatic route."""
    c = sb.swiglu_ln_case(300, 8192, 1536, seed=11)
    c.update(M=300, N=8192)
    worst = run_swiglu(c, lambda x, w, out, gk: ops.gemm(x, w, out=out, **gk), "swiglu 300x8192x1536")
    print(f"swiglu 300x8192x1536 LN fold: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("route", ["tile", "phased"])
def test_swiglu_planted_gate(route):
    """Gate pre-activations planted at +-30, +-100 and +-88 / +-89: finite and inside the bound on both routes (the
    exp(v) / (1 + exp(v)) form is NaN at +100)."""
    T = tune_lib()
    c = sb.planted_case(96, 64, 48, seed=2) if route == "tile" else sb.planted_case(4097, 128, 64, seed=3)
    if route == "tile":
        worst = run_swiglu(c, lambda x, w, out, gk: ops.gemm(x, w, out=out, **gk), "swiglu planted tile")
    else:
        worst = run_swiglu(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk), "swiglu planted phased", staged=True,
                           same_as=forced(T, 4))
    print(f"swiglu planted {route}: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("I", [48, 80, 96])
def test_gemm_f32_swiglu_tails(I):
    """vda_gemm_f32's SwiGLU branch as test_gemm_f32_geglu_tails holds GEGLU: N = 2 I = 96, 160, 192, gamma and a
    residual of the output's width, rel-L1 < 2e-6 against float64; one row of gate values planted at +-100."""
    g = torch.Generator().manual_seed(14 + I)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g, dtype=torch.float64).float() * scale  # noqa: E731
    M, K = 150, 24
    x, w, b = rnd(M, K), rnd(2 * I, K, scale=K ** -0.5), rnd(2 * I, scale=0.1)
    b[I:I + 4] = torch.tensor([100.0, -100.0, 30.0, -30.0])  # rows [h; g] before the interleave: gate biases
    w[I:I + 4] = 0
    gam, res = rnd(I).abs() + 0.1, rnd(M, I)
    hg = x.double() @ w.double().t() + b.double()
    ref = gam.double() * (hg[:, :I] * F.silu(hg[:, I:])) + res.double()
    buf = torch.full((M + 8, I + 8), float("nan"), device=DEV, dtype=torch.float32)
    out = buf[:M, :I]
    c = lambda t: t.to(DEV, torch.float32).contiguous()  # noqa: E731
    ops.gemm(c(x), c(_geglu_interleave(w)), bias=c(_geglu_interleave(b)), gamma=c(gam), res=c(res), act=ACT_SWIGLU, out=out)
    assert bool(torch.isfinite(out).all())
    assert rel(out, ref) < 2e-6
    assert bool(torch.isnan(buf[M:]).all()) and bool(torch.isnan(buf[:, I:]).all())


# ---- temporal attention, D <= 192 -------------------------------------------------------------------------------
def guarded(shape):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=torch.float16)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


BTS = [(1, 32, 37), (2, 5, 19), (1, 1, 8), (3, 17, 1)]
# (D, H, knob): the direct-load kernel by the attn knob, the staged D = 192 kernel on the automatic route; H = 3 leaves
# idle waves in the direct kernel's last block of four (B S H = 3 .. 111 items) and routes to it on its own
TEMPORAL = [(136, 8, 1), (152, 8, 1), (168, 8, 1), (184, 8, 1), (192, 8, 1), (192, 8, 0), (192, 3, 0), (136, 3, 1)]


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("D,H,knob", TEMPORAL)
def test_temporal_attention_d192(D, H, knob, rope):
    T = tune_lib()
    C = H * D
    worst = 0.0
    for B, Tn, S in BTS:
        qkv = fb.rnd16(B * Tn * S, 3 * C, seed=D + Tn + S) * 2
        ref, bound = fb.temporal_attn_ref_bound(qkv, B, Tn, S, H, D, rope)
        buf, y = guarded((B * Tn * S, C))
        with T.route(attn=knob):
            T.temporal_attention(h(qkv), B, Tn, S, H, D, rope, out=y)
        assert guard_ok(buf), "a store outside the output"
        what = f"temporal attention D={D} H={H} knob={knob} rope={rope} B={B} T={Tn} S={S}"
        worst = max(worst, assert_elementwise(y, ref, bound, what))
        assert rel(y, ref) < BAR_ATTN, what
        if knob == 0:  # the product library's automatic route is the tuning build's
            assert torch.equal(ops.temporal_attention(h(qkv), B, Tn, S, H, D, rope), y)
    print(f"temporal attention D={D} H={H} knob={knob} rope={rope}: worst |y - ref| / bound = {worst:.3f}")


def test_temporal_attention_d192_routes_differ_only_in_rounding():
    """Staged and direct-load kernels at D = 192 compute the same sums in the same MFMA order: bit-identical."""
    T = tune_lib()
    B, Tn, S, H, D = 1, 32, 37, 8, 192
    qkv = h(fb.rnd16(B * Tn * S, 3 * H * D, seed=5) * 2)
    with T.route(attn=1):
        a = T.temporal_attention(qkv, B, Tn, S, H, D)
    b = T.temporal_attention(qkv, B, Tn, S, H, D)
    assert torch.equal(a, b)


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("D", [192, 130])
def test_temporal_attention_f32_d192(D, rope):
    """The fp32 entry point beyond D = 128 (even D <= 192) with test_gpu_fp32_ops.py's comparisons: rel-L1 < 2e-6
    against float64 without RoPE; with it, where the fp32 angle carries the error, stress_bar (at most twice the error
    of torch's own fp32 evaluation)."""
    from test_gpu_fp32_ops import TOL_OP, _temporal_ref, stress_bar
    g = torch.Generator().manual_seed(60 + D)
    for B, Tn, S, H in [(2, 32, 5, 8), (1, 3, 7, 3)]:
        qkv = torch.randn(B * Tn * S, 3 * H * D, generator=g, dtype=torch.float64).float()
        y = ops.temporal_attention(qkv.to(DEV), B, Tn, S, H, D, rope_theta=rope)
        ref = _temporal_ref(qkv, B, Tn, S, H, D, rope)
        if rope:
            stress_bar(f"fp32 temporal attention rope D={D} T={Tn}", y, _temporal_ref(qkv, B, Tn, S, H, D, rope, torch.float32), ref)
        else:
            err = rel(y, ref)
            print(f"fp32 temporal attention D={D} T={Tn}: rel-L1 {err:.2e}")
            assert err < TOL_OP


# ---- the reduced-depth model --------------------------------------------------------------------------------------
D4 = dict(embed_dim=1536, depth=4, heads=24, taps=[0, 1, 2, 3], ffn="swiglu")


@pytest.fixture(scope="module")
def vitg_d4():
    """The d4 model on the recipe weights (348 M parameters; built once for the module)."""
    mp = pytest.MonkeyPatch()
    mp.setitem(vm.ENCODER_CFG, "vitg", D4)
    try:
        meta = vm.VideoDepthAnything.from_config("vitg", device="meta")
        sd = synthetic_state_dict((k, tuple(v.shape)) for k, v in meta.state_dict().items())
        m = vda_amd.build_model("vitg", sd, device="cuda")
    finally:
        mp.undo()
    assert len(m.pretrained.blocks) == 4 and m.intermediate_layer_idx["vitg"] == [0, 1, 2, 3]
    return m


def test_vitg_d4_matches_reference_golden(vitg_d4):
    """fp16 <= 1e-3 and fp32 <= 1e-5 rel-L1 against the reference's own forward (test_gpu_model.py's bars)."""
    x, depth, meta = _golden()
    d16 = vitg_d4(x.cuda()).float().cpu()
    d32 = vitg_d4(x.cuda(), fp32=True).float().cpu()
    e16, e32 = rel_l1(d16, depth), rel_l1(d32, depth)
    print(f"vitg d4 1x4x70x98: rel-L1 vs reference fp16 {e16:.3e}, fp32 {e32:.3e}")
    assert d16.shape == depth.shape and bool(torch.isfinite(d16).all())
    assert e32 <= 1e-5
    assert e16 <= 1e-3


def _golden():
    import numpy as np
    z = np.load(os.path.join(GOLDEN, "vitg_d4_t4_70x98.npz"), allow_pickle=False)
    return torch.from_numpy(z["x"].astype(np.float32)), torch.from_numpy(z["depth"]), json.loads(str(z["meta"]))


def test_vitg_d4_deterministic_and_other_encoders_unmoved(vitg_d4):
    """Two forwards are bit-equal; vits and vitl goldens run in the same process, before and after a ViT-g forward,
    give the same bits and stay inside the bar (packing is keyed per model)."""
    x, _, _ = _golden()
    xs = x.cuda()
    small = {}
    for name in ("vits_t4_70x126", "vitl_t4_70"):
        gx, gd, _, meta = load_golden(name)
        m = vda_amd.build_model(meta["encoder"], recipe_state_dict(meta["encoder"]), device="cuda")
        small[name] = (m, gx.cuda(), gd, m(gx.cuda()))
    a = vitg_d4(xs)
    assert torch.equal(a, vitg_d4(xs))
    for name, (m, gx, gd, before) in small.items():
        after = m(gx)
        assert torch.equal(before, after), name
        err = rel_l1(after.float().cpu(), gd)
        print(f"{name} beside vitg: rel-L1 vs reference = {err:.3e}")
        assert err <= 1e-3
