"""The fp16 GEMM, conv and attention kernels at their tile edges, under a per-element bound.

tests/test_gpu_ops.py reduces every comparison to one whole-tensor rel-L1 number at 2e-3 / 3e-3, which a
wrong tile edge row, MFMA fragment or K step of a large tensor passes.  Here every kernel route runs at the
smallest shapes that reach it (the tuning build's knobs, tests/tunelib.py, force the routes the product only
takes at large shapes), where one tile edge is a large share of the tensor, and EVERY element is held to
|y - ref| <= bound (helpers.assert_elementwise) with the float64 references and derived bounds of
tests/fp16_bounds.py (proved not too tight on the CPU by tests/test_fp16_bounds.py).  On top of it:

  * the old whole-tensor rel-L1 bar of test_gpu_ops.py (2e-3 GEMM / conv, 3e-3 attention);
  * every output that the C ABI lets the caller place is a view inside a sentinel-filled buffer, which must
    be untouched around the view afterwards (no store outside the output);
  * isolation: NaN neighbour frames / batches / sites must not reach the case's output, which is compared
    bit for bit with the call on the case alone.

`ops.*` runs the product's automatic route; `TuneLib` the forced ones and the calls that need `out=`.
The worst ratio |y - ref| / bound of every test is printed (pytest -s) and recorded in DESIGN.md.
"""
import math

import pytest
import torch

from vda_amd import ops
from vda_amd._lib import ACT_GEGLU, ACT_RELU
from vda_amd.model import _geglu_interleave
import fp16_bounds as fb
from helpers import assert_elementwise
from tunelib import tune_lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7776.0  # exactly representable in fp16
GUARD = 1024    # halfs of sentinel before and after a contiguous output (keeps it 16-byte aligned)
BAR_GEMM, BAR_ATTN = 2e-3, 3e-3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def h(t):
    return t.to(DEV, torch.float16).contiguous()


def f32(t):
    return t.to(DEV, torch.float32).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def framed2d(M, N):
    """An [M, N] view with 4 sentinel rows above / below and 8 sentinel columns left / right (row stride
    N + 16: 16-byte aligned rows whenever N % 8 == 0, N % 4 == 0 keeps the 8-byte contract of vda_gemm)."""
    buf = torch.full((M + 8, N + 16), SENT, device=DEV, dtype=torch.float16)
    return buf, buf[4:4 + M, 8:8 + N]


def frame2d_ok(buf, M, N):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[4:4 + M, 8:8 + N] = False
    return bool((buf[mask] == SENT).all())


def guarded(shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=torch.float16)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def note(what, worst):
    print(f"{what}: worst |y - ref| / bound = {worst:.3f}")


# =====================================================================================================
# Dense GEMM, one-tile-per-block kernels (vda_gemm_tile.h gemm_kernel through launch_tile)
# =====================================================================================================
TILES = {0: (128, 128), 1: (256, 128), 2: (128, 64), 3: (256, 256), 6: (64, 64), 7: (64, 128)}


def legal_ns(epi, BN):
    """The smallest legal N, BN - 8, BN, BN + 8 - in the epilogue's own granularity where 8 is not legal:
    GEGLU needs N % 32 == 0 (its output has N / 2 columns), the pixel-shuffle store N = k * k * cout with
    cout % 4 == 0, i.e. N % 16 (k = 2) or N % 64 (k = 4)."""
    g = {"geglu": 32, "ps2": 16, "ps4": 64}.get(epi, 8)
    small = {"geglu": 32, "ps2": 16, "ps4": 64}.get(epi, 4)
    return sorted({small, max(BN - g, small), BN, BN + g})


def ps_shuffle(t, BT, hin, win, k, cout):
    """[M, k*k*cout] GEMM matrix -> the [BT, hin*k, win*k, cout] NHWC map of the pixel-shuffle store."""
    return t.reshape(BT, hin, win, k, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(BT, hin * k, win * k, cout)


def run_gemm(c, launch, what, ref_bound=None, align16=False, staged=False, same_as=None):
    """One dense-GEMM case.  `launch(x, w, out, gk)` runs it (TuneLib.gemm_kw keywords); returns the worst ratio.
    align16: res / res2 rows 16-byte aligned (the phased route's contract) instead of 8-byte.  staged: the
    phased kernels' rounding points (fp16 residual adds, the Phi-table GELU).  same_as: a second launch function
    whose output must be bit-identical (the automatic route against the same kernel forced)."""
    M, N, K, epi, kw = c["M"], c["N"], c["K"], c["epi"], c["kw"]
    ref, bound = ref_bound if ref_bound is not None else fb.gemm_ref_bound(c["x"], c["w"], staged=staged,
                                                                           phi_table=staged, **kw)
    x = h(c["x"])
    if epi == "strided_x":  # the middle third of a [M, 3K] buffer: ldx = 3K
        x = torch.cat([h(fb.rnd16(M, K, seed=98)), x, h(fb.rnd16(M, K, seed=99))], 1)[:, K:2 * K]
    keep = []
    if epi == "geglu":
        w = h(_geglu_interleave(torch.cat([c["w"], kw["wg"]])))
        gk = dict(bias=f32(_geglu_interleave(torch.cat([kw["bias"], kw["bg"]]))), act=ACT_GEGLU)
        n_out = N // 2
    else:
        w, n_out = h(c["w"]), N
        gk = {k: f32(kw[k]) for k in ("bias", "rowbias", "gamma") if k in kw}
        gk.update({k: kw[k] for k in ("rdiv", "rmod", "act") if k in kw})
    if epi in ("ps2", "ps4"):
        k = int(epi[2])
        cout = N // (k * k)
        BT, hin, win = c.get("ps_geom") or fb.ps_geometry(M)
        buf, out = guarded((BT, hin * k, win * k, cout))
        launch(x, w, out, dict(gk, ps=(k, cout, hin, win)))
        ref, bound = ps_shuffle(ref, BT, hin, win, k, cout), ps_shuffle(bound, BT, hin, win, k, cout)
        intact = guard_ok(buf)
        if same_as is not None:
            buf2, out2 = guarded(tuple(out.shape))
            same_as(x, w, out2, dict(gk, ps=(k, cout, hin, win)))
    else:
        buf, out = framed2d(M, n_out)
        if epi == "gamma_res":  # in place, as the encoder's residual stream: res is the output
            out.copy_(h(kw["res"]))
            gk["res"] = out
        elif epi == "res_res2":  # column slices of wider buffers: row strides that are not N
            for name, off in (("res", 8), ("res2", 16)) if align16 else (("res", 4), ("res2", 8)):
                wide = torch.zeros(M, n_out + (24 if align16 else 12), device=DEV, dtype=torch.float16)
                wide[:, off:off + n_out] = h(kw[name])
                keep.append(wide)
                gk[name] = wide[:, off:off + n_out]
        launch(x, w, out, gk)
        intact = frame2d_ok(buf, M, n_out)
        if same_as is not None:
            buf2, out2 = framed2d(M, n_out)
            if epi == "gamma_res":
                out2.copy_(h(kw["res"]))
                gk = dict(gk, res=out2)
            same_as(x, w, out2, gk)
    worst = assert_elementwise(out, ref, bound, what)
    assert rel(out, ref) < BAR_GEMM, what
    assert intact, f"{what}: a store outside the output"
    if same_as is not None:
        assert torch.equal(out, out2), f"{what}: the automatic route is not the kernel this case is about"
    return worst


@pytest.mark.parametrize("epi", fb.GEMM_EPIS)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 6, 7, "auto"])
def test_gemm_tile_edges(cfg, epi):
    """BM x BN = 128x128, 256x128, 128x64, 256x256, 64x64, 64x128 (force_tile 0, 1, 2, 3, 6, 7), KB = 32, 4
    stages, and the automatic choice (ops.gemm; TuneLib with its knobs at rest for the pixel-shuffle store,
    which ops only exposes without out=).  M in {1, BM - 1, BM, BM + 1}; N in {smallest legal, BN - 8, BN,
    BN + 8} (legal_ns); K in {8, 24, 32, 40, 96, 160}: fewer K steps than stages, and K tails that are no
    multiple of 32.  Every epilogue runs the whole M x N x K grid.  drop_period is not in this list: vda_gemm serves it on the phased route only
    and rejects it with a tile forced (vda.h), see test_gemm_phased_ln_fold."""
    T = tune_lib()
    BM, BN = TILES.get(cfg, (128, 128))
    Ms, Ks = [1, BM - 1, BM, BM + 1], [8, 24, 32, 40, 96, 160]
    worst = 0.0
    for M in Ms:
        for N in legal_ns(epi, BN):
            for K in Ks:
                c = fb.gemm_case(M, N, K, epi, seed=M + N + K)
                if cfg == "auto" and not epi.startswith("ps"):
                    def launch(x, w, out, gk):
                        ops.gemm(x, w, out=out, **gk)
                    worst = max(worst, run_gemm(c, launch, f"gemm auto {epi} {M}x{N}x{K}"))
                else:
                    with T.route(**({} if cfg == "auto" else dict(force_tile=cfg))):
                        worst = max(worst, run_gemm(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk),
                                                    f"gemm cfg {cfg} {epi} {M}x{N}x{K}"))
    note(f"gemm tile cfg {cfg} {epi}", worst)


# =====================================================================================================
# Dense GEMM, phased kernels (vda_gemm_phased.h): cfg 4 = 256x256, cfg 5 = 512x128
# =====================================================================================================
def forced(T, cfg, **knobs):
    """A launch function for run_gemm(same_as=): the same GEMM with the phased kernel `cfg` forced.  gemm_route
    only takes the phased 256x256 kernel on its own when M, N, K and every alignment allow it and otherwise
    falls back to a tile kernel with other rounding points, which the (looser) staged bound would not notice;
    bit-identity with the forced kernel over a million outputs shows which kernel the automatic route ran."""
    def launch(x, w, out, gk):
        with T.route(force_tile=cfg, **knobs):
            T.gemm_kw(x, w, out, **gk)
    return launch


@pytest.mark.parametrize("M,N", [(M, N) for M in (4096, 4097, 4351) for N in (256, 264, 504, 512)] +
                         [(8192, 128), (8193, 128), (8703, 128)])
def test_gemm_phased_edges(M, N):
    """cfg 4 (256x256; M >= 4096, N >= 256, K % 64 == 0) and cfg 5 (512x128; N = 128, M >= 8192) on the
    automatic route (cfg 5 by force_tile = 5: the automatic table gives N = 128 with K <= 256 to the 128x64
    tile), at K = 64, 128, 192, 320 (nk = 1, 2, 3, 5: every prologue case of the 4-phase loop), on
    the automatic schedule and with gemm_sched = 1, 3, 5 persistent blocks: a block then walks several tiles
    with a short last round at 17 .. 36 tiles instead of more than 256.  Bias epilogue (EK 1).  The automatic
    route's output is bit-identical to cfg 4 forced (see forced())."""
    T = tune_lib()
    worst = 0.0
    for K in (64, 128, 192, 320):
        c = fb.gemm_case(M, N, K, "bias", seed=M + N + K)
        rb = fb.gemm_ref_bound(c["x"], c["w"], **c["kw"])
        for sched in (-1, 1, 3, 5):
            with T.route(gemm_sched=sched, **(dict(force_tile=5) if N == 128 else {})):
                worst = max(worst, run_gemm(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk),
                                            f"gemm phased {M}x{N}x{K} sched {sched}", ref_bound=rb,
                                            same_as=forced(T, 4, gemm_sched=sched) if N != 128 and sched == -1 else None))
    note(f"gemm phased {M}x{N}", worst)


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("epi", ["bias", "gelu", "gamma_res", "res_res2", "rowbias", "geglu", "ps2", "ps4", "strided_x"])
def test_gemm_phased_epilogues(epi, N):
    """The register and staged epilogues gemm_route picks without the LayerNorm fold, at M = 4097 (a one-row
    last M tile), K = 192, on 3 persistent blocks: bias and bias + GELU (EK 1), the general staged epilogue
    (GEGLU; gamma / res / res2: t = gamma * act(..) rounded to fp16, then the residuals added as packed fp16 vectors,
    fp16_bounds.gemm_ref_bound staged=True; GELU and GEGLU through the Phi table; pixel-shuffle store), the
    row-bias instantiation.  Bit-identical to cfg 4 forced: the automatic route took the phased kernel.  The LayerNorm-fold
    epilogues, drop_period and stats_out: test_gemm_phased_ln_fold, test_gemm_phased_res_stats_out."""
    T = tune_lib()
    M, K = 4097, 192
    c = fb.gemm_case(M, N, K, epi, seed=N + len(epi))
    if epi == "rowbias":
        c["kw"].update(rdiv=300)  # frames of 300 rows: every 256-row tile spans a frame change
    with T.route(gemm_sched=3):
        worst = run_gemm(c, lambda x, w, out, gk: T.gemm_kw(x, w, out, **gk), f"gemm phased {epi} N={N}", align16=True,
                         staged=True, same_as=forced(T, 4, gemm_sched=3))
    note(f"gemm phased epilogue {epi} N={N}", worst)


def check_stats(stats, out, M, parts, what):
    """stats [M + 1, parts, 2] against float64 sums of the stored fp16 rows per 256-column part; row M stays NaN."""
    assert parts * 256 == out.shape[1]
    sref, sbound = fb.row_stats_ref_bound(out)
    assert bool(torch.isnan(stats[M]).all()), f"{what}: the spare statistics row was written"
    return assert_elementwise(stats[:M], sref, sbound, what)


DROPS = {"ln_drop": 300, "ln_drop256": 256, "ln_drop511": 511, "ln_drop4096": 4096}


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("kind", fb.LN_KINDS + ("ln_drop256", "ln_drop511", "ln_drop4096"))
def test_gemm_phased_ln_fold(kind, N):
    """The LayerNorm-fold epilogues gemm_route picks at M = 4097, K = 192, 3 persistent blocks: plain with [M, 2]
    (mean, rstd) statistics (register epilogue EK 1) and with three-part (sum, sum of squares) statistics, + GELU,
    + GEGLU (staged), + the per-frame row bias (EK 3, frames of 300 rows), + stats_out (the staged epilogue and
    the separate partial-sum pass), and drop_period (served by this route's EK 1 epilogue only; the dropped row
    first, last and on a tile boundary as that epilogue meets them): 300 (the dropped row first in tile 0, then
    inside tiles), 256 (every tile starts on a dropped row), 511 (the frame boundary on tile row 255) and 4096
    (row 4096 is the last row, dropped, and alone in the last tile, which stores nothing).  The statistics
    buffer holds exactly M entries.  Bound: fp16_bounds.gemm_ref_bound's folded form, GELU / GEGLU through the
    Phi table.  Where vda_gemm accepts a forced tile (not with a row bias or drop_period, which only this route
    serves at all), the output is bit-identical to cfg 4 forced."""
    T = tune_lib()
    M, K = 4097, 192
    c = fb.gemm_ln_case(M, N, K, kind, seed=N)
    kw = c["kw"]
    ln = kw["ln"]
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], phi_table=True, **kw)
    parts = 3 if "parts" in ln else 0
    st = f32(ln["parts"] if parts else torch.stack([ln["mean"], ln["rstd"]], -1))
    n_out, gk = N, {}
    if kind == "ln_geglu":
        il = lambda a, b: _geglu_interleave(torch.cat([a, b]))  # noqa: E731
        w, bias, cs = h(il(c["w"], kw["wg"])), f32(il(kw["bias"], kw["bg"])), f32(il(ln["colsum"], ln["colsum_g"]))
        n_out, gk = N // 2, dict(act=ACT_GEGLU)
    else:
        w, bias, cs = h(c["w"]), f32(kw["bias"]), f32(ln["colsum"])
    gk.update(bias=bias, ln_stats=st, ln_colsum=cs, ln_parts=parts, ln_eps=1e-6, act=kw.get("act", gk.get("act", 0)))
    rows = M
    if kind in DROPS:
        keep = torch.arange(M) % DROPS[kind] != 0
        ref, bound, rows = ref[keep], bound[keep], int(keep.sum())
        gk["drop_period"] = DROPS[kind]
    elif kind == "ln_rowbias":
        gk.update(rowbias=f32(kw["rowbias"]), rdiv=kw["rdiv"], rmod=kw["rmod"])
    elif kind == "ln_stats_out":
        stats = torch.full((M + 1, N // 256, 2), float("nan"), device=DEV, dtype=torch.float32)
        gk["stats_out"] = stats
    buf, out = framed2d(rows, n_out)
    x = h(c["x"])
    with T.route(gemm_sched=3):
        T.gemm_kw(x, w, out, **gk)
    worst = assert_elementwise(out, ref, bound, f"gemm phased {kind} N={N}")
    assert rel(out, ref) < BAR_GEMM and frame2d_ok(buf, rows, n_out)
    if kind not in DROPS and kind != "ln_rowbias":
        buf2, out2 = framed2d(rows, n_out)
        forced(T, 4, gemm_sched=3)(x, w, out2, dict(gk, stats_out=None))
        assert torch.equal(out, out2), "the automatic route is not the phased kernel"
    if kind == "ln_stats_out":
        check_stats(stats, out, M, N // 256, f"LN fold stats_out N={N}")
    note(f"gemm phased {kind} N={N}", worst)


@pytest.mark.parametrize("N", [256, 512])
def test_gemm_phased_res_stats_out(N):
    """res + stats_out through the staged epilogue, M = 4097: the output under the per-element bound, and the
    [M, N / 256, 2] partial (sum, sum of squares) of the STORED
    fp16 row against float64 sums of the kernel's own output per 256-column part (fp32 accumulation of 256
    terms: fp16_bounds.row_stats_ref_bound), with a NaN spare row after row M - 1 that must stay NaN.  Output
    and statistics are bit-identical to cfg 4 forced (the in-epilogue statistics, not the separate pass)."""
    T = tune_lib()
    M, K = 4097, 128
    parts = N // 256
    c = fb.gemm_case(M, N, K, "gamma_res", seed=N)
    del c["kw"]["gamma"]
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], staged=True, **c["kw"])
    buf, out = framed2d(M, N)
    res = h(c["kw"]["res"])
    stats = torch.full((M + 1, parts, 2), float("nan"), device=DEV, dtype=torch.float32)
    with T.route(gemm_sched=3):
        T.gemm_kw(h(c["x"]), h(c["w"]), out, bias=f32(c["kw"]["bias"]), res=res, stats_out=stats)
    worst = assert_elementwise(out, ref, bound, f"gemm res+stats N={N}")
    assert rel(out, ref) < BAR_GEMM and frame2d_ok(buf, M, N)
    buf2, out2 = framed2d(M, N)
    stats2 = torch.full_like(stats, float("nan"))
    forced(T, 4, gemm_sched=3)(h(c["x"]), h(c["w"]), out2, dict(bias=f32(c["kw"]["bias"]), res=res, stats_out=stats2))
    assert torch.equal(out, out2) and torch.equal(stats[:M], stats2[:M]), "the automatic route is not the phased kernel"
    ws = check_stats(stats, out, M, parts, f"stats_out N={N}")
    note(f"gemm phased res+stats N={N} (stats {ws:.3f})", worst)


# =====================================================================================================
# Convolutions (vda_conv2d)
# =====================================================================================================
def conv_launch_kw(c):
    kw = c["kw"]
    gk = dict(ks=c["w"].shape[2], stride=kw["stride"], pad=kw["pad"], pre_relu=kw.get("pre_relu", False),
              act=ACT_RELU if kw.get("relu_out") else 0)
    if "bias" in kw:
        gk["bias"] = f32(kw["bias"])
    for name in ("res", "res2"):
        if name in kw:
            gk[name] = h(nhwc(kw[name]))
    if "up" in kw:
        gk["up"] = kw["up"]
    if "framebias" in kw:
        gk.update(rowbias=f32(kw["framebias"]), rdiv=c["Ho"] * c["Wo"], rmod=kw["framebias"].shape[0])
    return gk


def conv_rb(c, staged):
    ref, bound = fb.conv_ref_bound(c["x"], c["w"], staged=staged, **c["kw"])
    return nhwc(ref), nhwc(bound)


def run_conv(c, knobs, staged, what, product=False, rb=None):
    """One conv case on the route `knobs` select, into a sentinel-guarded output; returns (out, worst ratio).
    product=True also runs ops.conv2d (the product library's automatic route): same bits."""
    T = tune_lib()
    kw = c["kw"]
    x, w = h(nhwc(c["x"])), h(nhwc(c["w"]))
    gk = conv_launch_kw(c)
    ref, bound = rb if rb is not None else conv_rb(c, staged)
    buf, out = guarded(tuple(ref.shape))
    with T.route(**knobs):
        T.conv2d(x, w, out=out, res2_up=kw.get("res2_up", False), **gk)
    worst = assert_elementwise(out, ref, bound, what)
    assert rel(out, ref) < BAR_GEMM, what
    assert guard_ok(buf), f"{what}: a store outside the output"
    if product:
        assert torch.equal(ops.conv2d(x, w, **gk), out), f"{what}: ops.conv2d differs from the tuning build at rest"
    return out, worst


MODES = ("plain", "rcu1", "rcu2")


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 32), (9, 33), (7, 31), (16, 64), (17, 95)])
def test_hconv_forced_edges(H, W, Cin):
    """vda_hconv.hip (8 x 32 output tiles, 64-channel slabs; Cin = 64 is the smallest it accepts) forced on
    maps of less than one tile, exactly one, one plus a row and a column, one less, 2 x 2 tiles and 3 x 3
    ragged tiles; BT = 2; plain / rcu1 / rcu2.  Staged epilogue: conv + bias rounded to fp16, then res and
    res2 added as fp16 vectors."""
    worst = 0.0
    for mode in MODES:
        c = fb.conv_case(2, Cin, 256, H, W, mode, seed=H * W + Cin)
        worst = max(worst, run_conv(c, dict(hconv=1), True, f"hconv {H}x{W} Cin {Cin} {mode}")[1])
    note(f"hconv forced {H}x{W} Cin {Cin}", worst)


@pytest.mark.parametrize("H,W,mode", [(64, 64, "rcu2"), (65, 67, "rcu1"), (71, 95, "rcu2"), (4, 1024, "rcu2"),
                                      (1030, 4, "rcu1"), (4, 1024, "plain")])
def test_hconv_product_route(H, W, mode):
    """The product's automatic route (H * W >= 4096 -> the halo conv) through ops.conv2d, BT = 2, Cin = 64: whole
    tiles, ragged tiles in both directions, and the thin maps 4 x 1024 (H < 8: every tile has 4 rows past the
    map) and 1030 x 4 (W < 32: 28 columns past it; 129 tile rows).  Both are addressable: the patch staging
    tests every pixel against H and W (poff = -1 reads the zero page), voff() gives pixels past the map the
    out-of-range buffer offset, and all epilogue accesses go through per-frame buffer descriptors."""
    c = fb.conv_case(2, 64, 256, H, W, mode, seed=H + W)
    _, worst = run_conv(c, {}, True, f"hconv auto {H}x{W} {mode}", product=True)
    note(f"hconv product route {H}x{W} {mode}", worst)


@pytest.mark.parametrize("src", [(1, 1), (65, 67), (33, 34)])
def test_hconv_res2_upsample_edges(src):
    """res2 read through the bilinear align_corners=True upsample in the halo conv's epilogue at 65 x 67 from a
    1 x 1 source, a source of the output's own size and the half-size (ceil) one: against the float64 resize,
    and bit for bit against ops.upsample_bilinear + the same-grid res2."""
    T = tune_lib()
    H, W = 65, 67
    c = fb.conv_case(2, 64, 256, H, W, "rcu2", seed=src[0], res2_src=src)
    out, worst = run_conv(c, {}, True, f"hconv res2 upsampled from {src}")
    gk = conv_launch_kw(c)
    gk["res2"] = ops.upsample_bilinear(gk["res2"], H, W)
    y_mat = T.conv2d(h(nhwc(c["x"])), h(nhwc(c["w"])), **gk)
    assert torch.equal(out, y_mat)
    note(f"hconv res2 upsample {src}", worst)


@pytest.mark.parametrize("H,W", [(1, 8), (1, 16), (2, 127), (2, 128), (3, 129), (5, 160), (19, 19)])
def test_strip_edges(H, W):
    """vda_strip.hip (256-pixel strips of 32-channel slabs, 16 <= W <= 160) by force_tile = -3, BT = 2, Cin in
    {32 (the smallest), 64, 96}, strip_split in {1, 2, 3, 0}: a split that does not divide Cin / 32 (2 at Cin
    = 32 / 96, 3 at 32 / 64) falls back to the automatic count, 3 is no power of two and never taken.  A
    strip of less than one tile, exactly 256 pixels, 256 + 2, three ragged tiles spanning rows.  1 x 8: the
    strip kernel declines W < 16 (vda_conv_strip_serves), so that shape checks the fall-through to the
    implicit GEMM (one rounding).  Split results are bit-identical across two runs."""
    T = tune_lib()
    staged = W >= 16
    worst = 0.0
    for i, Cin in enumerate((32, 64, 96)):
        for j, mode in enumerate(MODES):
            c = fb.conv_case(2, Cin, 256, H, W, mode, seed=H * W + Cin)
            rb = conv_rb(c, staged)
            for split in ((1, 2, 3, 0) if (i + j) % 3 == 0 else (0, 2)):
                out, r = run_conv(c, dict(force_tile=-3, strip_split=split), staged, f"strip {H}x{W} Cin {Cin} {mode} split {split}", rb=rb)
                again, _ = run_conv(c, dict(force_tile=-3, strip_split=split), staged, "strip again", rb=rb)
                assert torch.equal(out, again)
                worst = max(worst, r)
    note(f"strip {H}x{W}", worst)


def bias_case(BT, Cin, Cout, H, W, relu, seed, up=None):
    c = fb.conv_case(BT, Cin, Cout, H, W, "rcu1", seed=seed, up=up)
    c["kw"].update(pre_relu=False, relu_out=relu)
    return c


@pytest.mark.parametrize("H,W,relu", [(129, 128, False), (143, 115, True)])
def test_halo_cout128_product_route(H, W, relu):
    """The 128-output halo conv (vda_oc1.hip, 16 x 16 tiles) on the automatic route (H * W >= 128^2): one
    row more than 8 whole tiles, and ragged tiles both ways.  Bias [+ ReLU], one rounding."""
    _, worst = run_conv(bias_case(1, 64, 128, H, W, relu, H), {}, False, f"halo128 {H}x{W}", product=True)
    note(f"halo Cout 128 {H}x{W}", worst)


@pytest.mark.parametrize("Hs,Ws,H,W", [(1, 1, 16, 16), (9, 9, 17, 17), (8, 20, 33, 47), (16, 16, 16, 16),
                                       (22, 21, 33, 33), (21, 22, 33, 33), (22, 22, 33, 33)])
def test_halo_fused_resize_edges(Hs, Ws, H, W):
    """3x3 conv (Cout = 128) on a bilinear resize fused into the halo conv's patch staging: from one pixel, x2
    with a ragged tile, a ragged non-integer ratio.  The identity 16 x 16 -> 16 x 16 is the case
    vda_conv_halo_fused DECLINES (a tile's source window of 20 x 20 pixels exceeds its 192-pixel staging), so
    it runs on vda_launch_conv_reg and must still be correct.  To 33 x 33 (scale (Hs - 1) / 32, exact) the
    staging boundary itself: 22 x 21 and 21 x 22 need 14 x 13 = 182 pixels (served), 22 x 22 needs 196
    (declined).  The resized operand is an fp16 rounding."""
    c = bias_case(2, 64, 128, Hs, Ws, True, Hs + W, up=(H, W))
    _, worst = run_conv(c, {}, False, f"fused resize {Hs}x{Ws}->{H}x{W}", product=True)
    note(f"halo fused resize {Hs}x{Ws}->{H}x{W}", worst)


@pytest.mark.parametrize("cfg", [-2, 0, 1, 2, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (9, 11), (16, 16)])
def test_implicit_gemm_conv_edges(H, W, cfg):
    """The implicit-GEMM conv (gemm_kernel<CONV>) by force_tile = -2 (automatic tile) and cfg 0 / 1 / 2 / 3 (1: the
    256x128 tile the automatic route gives N = 128 convs of 4096 <= M < 8192 rows, ViT-B streaming): stride 1
    and 2, ks 1 and 3, Cin = 8 (the smallest: K = 8 or 72, a K tail) and 64, Cout = 32 and 128, BT = 2,
    plain / rcu1 / rcu2.  One rounding at the store."""
    worst = 0.0
    for stride in (1, 2):
        for ks in (1, 3):
            for n, (Cin, Cout) in enumerate(((8, 32), (64, 128))):
                mode = MODES[(stride + ks + n) % 3]
                c = fb.conv_case(2, Cin, Cout, H, W, mode, ks=ks, stride=stride, seed=H * W + ks)
                worst = max(worst, run_conv(c, dict(force_tile=cfg), False,
                                            f"implicit gemm cfg {cfg} {H}x{W} s{stride} k{ks} {Cin}->{Cout} {mode}")[1])
    note(f"implicit-GEMM conv cfg {cfg} {H}x{W}", worst)


@pytest.mark.parametrize("cfg", [-2, 0, 1, 2])
def test_implicit_gemm_conv_rowbias(cfg):
    """rowbias with rdiv = Ho * Wo (one bias row per frame, rmod = 3 over BT = 5 frames) on the implicit-GEMM
    conv at 9 x 11, stride 1 and 2: 128-row tiles span frame changes at rows that are no multiple of 16."""
    worst = 0.0
    for stride in (1, 2):
        c = fb.conv_case(5, 64, 128, 9, 11, "rcu2", stride=stride, seed=stride)
        c["kw"]["framebias"] = fb.rnd32(3, 128, seed=7)
        worst = max(worst, run_conv(c, dict(force_tile=cfg), False, f"implicit gemm rowbias cfg {cfg} s{stride}")[1])
    note(f"implicit-GEMM conv rowbias cfg {cfg}", worst)


@pytest.mark.parametrize("Cout", [32, 128])
def test_conv_reg_resize_edges(Cout):
    """up= through the register-staged conv (vda_launch_conv_reg, 128x64 and 128x128 tiles), reached with a tile
    forced: (8, 20) -> (33, 47), BT = 2."""
    c = bias_case(2, 64, Cout, 8, 20, True, Cout, up=(33, 47))
    _, worst = run_conv(c, dict(force_tile=0), False, f"conv_reg resize Cout {Cout}")
    note(f"register-staged resize conv Cout {Cout}", worst)


def test_phased_conv_edge():
    """The phased 256x256 implicit-GEMM conv needs M >= 4096: BT = 1 at 64 x 65 (M = 4160, a ragged second M
    tile), Cin = 64, Cout = 256, with the halo and strip routes off.  Its staged epilogue adds res and res2 as
    packed fp16 vectors after rounding conv + bias (the bound's staged form)."""
    c = fb.conv_case(1, 64, 256, 64, 65, "rcu2", seed=5)
    _, worst = run_conv(c, dict(hconv=0, force_tile=-2), True, "phased conv 64x65")
    note("phased conv 64x65", worst)


@pytest.mark.parametrize("H,W", [(128, 128), (127, 131)])
def test_im2col_route_edges(H, W):
    """Stride-2 3x3 convs with M >= 4096, Cin % 64 == 0, Cout % 256 == 0 take explicit im2col + the dense phased
    GEMM: BT = 1, Cin = 64, Cout = 256 (M = 4096 and 64 x 66 = 4224).  Bit-identical to the implicit GEMM
    (force_tile = -2: the same K order)."""
    c = fb.conv_case(1, 64, 256, H, W, "rcu1", stride=2, seed=H)
    out, worst = run_conv(c, {}, False, f"im2col {H}x{W}", product=True)
    out2, _ = run_conv(c, dict(force_tile=-2), False, f"im2col vs implicit {H}x{W}", rb=conv_rb(c, False))
    assert torch.equal(out, out2)
    note(f"im2col route {H}x{W}", worst)


ISOLATION = [
    ("hconv", dict(hconv=1), dict(Cin=64, Cout=256, H=9, W=33, mode="rcu2"), {}),
    ("strip", dict(force_tile=-3), dict(Cin=64, Cout=256, H=3, W=129, mode="rcu2"), {}),
    ("strip split", dict(force_tile=-3, strip_split=2), dict(Cin=64, Cout=256, H=3, W=129, mode="rcu1"), {}),
    ("halo128", {}, dict(Cin=64, Cout=128, H=129, W=130, mode="rcu1"), dict(pre_relu=False)),
    ("halo fused resize", {}, dict(Cin=64, Cout=128, H=8, W=20, mode="rcu1", up=(33, 47)), dict(pre_relu=False)),
    ("conv_reg resize", dict(force_tile=0), dict(Cin=64, Cout=128, H=8, W=20, mode="rcu1", up=(33, 47)), dict(pre_relu=False)),
    ("implicit gemm", dict(force_tile=-2), dict(Cin=8, Cout=32, H=9, W=11, mode="rcu2"), {}),
    ("implicit gemm s2", dict(force_tile=2), dict(Cin=64, Cout=128, H=9, W=11, mode="rcu1", stride=2), {}),
    ("im2col", {}, dict(Cin=64, Cout=256, H=127, W=131, mode="rcu1", stride=2), {}),
    ("phased conv", dict(hconv=0, force_tile=-2), dict(Cin=64, Cout=256, H=64, W=65, mode="rcu2"), {}),
    ("phased conv 512x128", {}, dict(Cin=96, Cout=128, H=91, W=91, mode="rcu2"), {}),
]


@pytest.mark.parametrize("name,knobs,shape,over", ISOLATION, ids=[i[0] for i in ISOLATION])
def test_conv_frame_isolation(name, knobs, shape, over):
    """A batch of three frames whose middle frame is the case and whose outer frames (input and residuals) are
    NaN: the middle output is finite and bit-identical to the single-frame call, on every conv route at one
    ragged shape each (a neighbouring frame cannot leak in through a halo or a tile that spans frames)."""
    T = tune_lib()
    c = fb.conv_case(1, seed=3, **shape)
    c["kw"].update(over)
    gk = conv_launch_kw(c)
    x, w = h(nhwc(c["x"])), h(nhwc(c["w"]))

    def tripled(t):
        out = torch.full((3,) + tuple(t.shape[1:]), float("nan"), device=DEV, dtype=torch.float16)
        out[1] = t[0]
        return out
    gk3 = dict(gk, **{k: tripled(gk[k]) for k in ("res", "res2") if k in gk})
    with T.route(**knobs):
        single = T.conv2d(x, w, **gk)
        triple = T.conv2d(tripled(x), w, **gk3)
    assert bool(torch.isfinite(triple[1]).all()), f"{name}: a NaN neighbour frame reached the middle frame"
    assert torch.equal(triple[1], single[0]), f"{name}: the middle frame depends on its neighbours"


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("BT,hh,ww,cout", [(1, 1, 1, 32), (2, 3, 5, 32), (1, 16, 16, 64), (2, 17, 23, 32), (4, 33, 32, 256)])
def test_conv_transpose_pixel_shuffle_edges(BT, hh, ww, cout, k):
    """ConvTranspose2d(kernel = stride = k) as a GEMM with the pixel-shuffle store on the automatic route: one
    pixel, a ragged small map, 16 x 16, 17 x 23, and (4, 33, 32) with cout = 256 (M = 4224: the phased kernel's
    staged whole-pixel store, bit-identical to cfg 4 forced).  Cin = 64.  Through the C ABI into a
    sentinel-guarded output, and bit-identical through ops.conv_transpose_ks (the product)."""
    T = tune_lib()
    Cin, M, N = 64, BT * hh * ww, k * k * cout
    c = fb.gemm_case(M, N, Cin, "ps%d" % k, seed=M + k)
    c["ps_geom"] = (BT, hh, ww)
    got = []

    def launch(x, w, out, gk):
        T.gemm_kw(x, w, out, **gk)
        got.append(out)
    worst = run_gemm(c, launch, f"conv transpose k{k} {BT}x{hh}x{ww}",
                     same_as=forced(T, 4) if M >= 4096 and cout % 256 == 0 else None)
    y = ops.conv_transpose_ks(h(c["x"]), h(c["w"]), f32(c["kw"]["bias"]), BT, hh, ww, k)
    assert torch.equal(y, got[0])
    note(f"conv transpose k{k} {BT}x{hh}x{ww} cout {cout}", worst)


# =====================================================================================================
# Attention
# =====================================================================================================
@pytest.mark.parametrize("old", [0], ids=["mfma32"])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
def test_spatial_attention_edges(N, old):
    """Spatial attention (128-query blocks, 64-key tiles, 32-key softmax halves) with sequence lengths on both
    sides of every one of those sizes, H in {1, 3}, B = 2 with batch 0 all NaN: batch 1 is finite, inside the
    bound (fp16_bounds.spatial_attn_ref_bound: P rounded to fp16 before the PV MFMA, the output to fp16, q *
    scale * log2e to fp16) and bit-identical to the call on batch 1 alone; every output sits between sentinel
    guards that must stay intact (no store past the last query row).  The single-valued `old` axis keeps the
    test ids of the time when a second spatial kernel ran here."""
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
        assert torch.equal(ops.spatial_attention(h(one), 1, N, H, 64), y1)
        worst = max(worst, assert_elementwise(y2[N:], ref, bound, f"spatial attention N={N} H={H}"))
        assert rel(y2[N:], ref_q) < BAR_ATTN
        assert torch.equal(y2[N:], y1), "batch 1 depends on batch 0"
    note(f"spatial attention N={N}", worst)


@pytest.mark.parametrize("old", [0], ids=["mfma32"])
@pytest.mark.parametrize("ramp", ["up", "spike", "down"])
def test_spatial_attention_ramps_elementwise(ramp, old):
    """The three score profiles of test_spatial_attention_rebase (climbing, one late spike, falling: the deferred
    re-base of the online softmax) at N = 129 (two whole key tiles and one key) under the per-element bound."""
    T = tune_lib()
    B, N, H = 2, 129, 2
    qkv = fb.attn_ramp_qkv(ramp, B, N, H)
    ref, bound = fb.spatial_attn_ref_bound(qkv, B, N, H)
    buf, y = guarded((B * N, H * 64))
    T.spatial_attention(h(qkv), B, N, H, out=y)
    assert guard_ok(buf), "a store outside the output"
    worst = assert_elementwise(y, ref, bound, f"spatial attention ramp {ramp}")
    assert rel(y, ref) < BAR_ATTN
    note(f"spatial attention ramp {ramp}", worst)


TEMPORAL = [(32, 4, 0), (64, 4, 0), (128, 4, 0),                 # the LDS-staged kernel (H % waves-per-block == 0)
            (8, 3, 0), (24, 3, 0), (48, 3, 0), (120, 3, 0),      # the direct-load kernel's own head dims
            (64, 3, 0), (64, 4, 1), (32, 3, 1),                  # direct-load: by H % 4 != 0 and by the attn knob
            (16, 8, 0), (96, 8, 0), (48, 8, 0)]                  # direct-load at H = 8: ViT-B's motion modules 2 / 3, 1, 0


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("D,H,old", TEMPORAL)
def test_temporal_attention_edges(D, H, old, rope):
    """Both temporal kernels at T in {1, 2, 31, 32}, S = 3, RoPE on and off, site 1 the case with sites 0 and 2
    all NaN: site 1 is finite, inside the bound and bit-identical to the S = 1 call; the outputs sit between
    sentinel guards (no store for frames >= T or past the last site).  The LDS-staged kernel
    (D in {32, 64, 128}) only runs when H is a multiple of its waves per block, so it never has an idle wave:
    it gets H = 4 (S * H = 12 items); the direct-load kernel gets H = 3 (S * H = 9: one idle wave in the
    last block of 4) at D in {8, 24, 48, 120}, at D = 64 (where H = 3 itself routes to it) and by the attn knob;
    and at H = 8 (the motion modules' head count: S * H = 24 items, no idle wave) with D = 16, 96 and 48, ViT-B's
    modules 2 / 3, 1 and 0, which no other encoder's head dims reach."""
    T = tune_lib()
    S, C = 3, H * D
    worst = 0.0
    for Tn in (1, 2, 31, 32):
        one = fb.rnd16(Tn, 3 * C, seed=Tn + D) * 2           # [T * 1, 3C]: the case as a single site
        three = torch.full((Tn, S, 3 * C), float("nan"))
        three[:, 1] = one
        ref, bound = fb.temporal_attn_ref_bound(one, 1, Tn, 1, H, D, rope)
        buf3, y3 = guarded((Tn * S, C))
        buf1, y1 = guarded((Tn, C))
        with T.route(attn=old):
            T.temporal_attention(h(three.reshape(Tn * S, 3 * C)), 1, Tn, S, H, D, rope, out=y3)
            T.temporal_attention(h(one), 1, Tn, 1, H, D, rope, out=y1)
        assert guard_ok(buf3) and guard_ok(buf1), "a store outside the output"
        y3 = y3.reshape(Tn, S, C)
        if not old:
            assert torch.equal(ops.temporal_attention(h(one), 1, Tn, 1, H, D, rope), y1)
        worst = max(worst, assert_elementwise(y3[:, 1], ref, bound, f"temporal attention T={Tn} D={D} H={H} old={old} rope={rope}"))
        assert rel(y3[:, 1], ref) < BAR_ATTN
        assert torch.equal(y3[:, 1], y1), "site 1 depends on its neighbour sites"
    note(f"temporal attention D={D} H={H} old={old} rope={rope}", worst)


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("D,H", [(32, 4), (128, 2), (24, 3), (16, 8), (96, 8)])
def test_temporal_attention_batch_decode(D, H, rope):
    """The (item -> batch, site, head) decode both temporal kernels share, at B = 2 (the edges test has B = 1
    only), T = 5, S = 2: both block shapes of the LDS-staged kernel (4 waves at D = 32, 2 at D = 128) and the
    direct-load kernel (D = 24, H = 3: 6 items in the B = 1 call, so two idle waves in its last block; D = 16 and 96
    at H = 8, ViT-B's motion modules).  Batch 0
    is all NaN: batch 1 is finite, inside the bound and bit-identical to the B = 1 call on batch 1 alone; both
    outputs sit between sentinel guards."""
    T = tune_lib()
    B, Tn, S, C = 2, 5, 2, H * D
    one = fb.rnd16(Tn * S, 3 * C, seed=D + H) * 2            # [(1 * T) * S, 3C]: batch 1 alone
    both = torch.cat([torch.full_like(one, float("nan")), one])
    ref, bound = fb.temporal_attn_ref_bound(one, 1, Tn, S, H, D, rope)
    buf2, y2 = guarded((B * Tn * S, C))
    buf1, y1 = guarded((Tn * S, C))
    T.temporal_attention(h(both), B, Tn, S, H, D, rope, out=y2)
    T.temporal_attention(h(one), 1, Tn, S, H, D, rope, out=y1)
    assert guard_ok(buf2) and guard_ok(buf1), "a store outside the output"
    got = y2[Tn * S:]
    assert bool(torch.isfinite(got).all()), "NaN batch 0 reached batch 1"
    worst = assert_elementwise(got, ref, bound, f"temporal attention B=2 D={D} H={H} rope={rope}")
    assert torch.equal(got, y1), "batch 1 depends on batch 0"
    note(f"temporal attention batch decode D={D} H={H} rope={rope}", worst)
