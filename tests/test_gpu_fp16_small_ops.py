"""The fp16 LayerNorm, GroupNorm, GroupNorm -> Linear, resize, im2col and depth-tail kernels at their edges, under
per-element bounds.

tests/test_gpu_ops.py holds these kernels to one whole-tensor rel-L1 number at a few mid-sized contiguous
shapes.  Here they run at the smallest shapes that reach every path (rows-per-wave edges, chunk and block edges,
idle threads, row pairs, stride loops), with strided inputs and stress values, and EVERY element is held to
|y - ref| <= bound (helpers.assert_elementwise) with the float64 references and derived bounds of
tests/fp16_bounds.py (proved not too tight, and shown to reject wrong arithmetic, on the CPU by
tests/test_fp16_bounds.py).  On top of it, as in tests/test_gpu_fp16_edges.py:

  * the old whole-tensor rel-L1 bars of test_gpu_ops.py;
  * every output the C ABI lets the caller place is a view inside a sentinel-filled buffer that must be
    untouched around the view afterwards; `ops.*` (which allocates) must return the same bits;
  * isolation (a NaN row / frame must not reach its neighbours) and determinism.

The worst ratio |y - ref| / bound of every test is printed (pytest -s) and recorded in DESIGN.md.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import vda_amd
from vda_amd import ops
import fp16_bounds as fb
from helpers import assert_elementwise
from tunelib import tune_lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7776.0  # exactly representable in fp16
GUARD = 1024    # elements of sentinel before and after a contiguous output (keeps it 16-byte aligned)
BAR = 2e-3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def h(t):
    return t.to(DEV, torch.float16).contiguous()


def f32(t):
    return t.to(DEV, torch.float32).contiguous()


def guarded(shape, dtype=torch.float16):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def note(what, worst):
    print(f"{what}: worst |y - ref| / bound = {worst:.3f}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vda_amd._libvda()


def strided(x16, ld):
    """x16 [R, C] on the device as a row-strided view (row stride ld >= C) of a NaN-filled buffer."""
    R, C = x16.shape
    buf = torch.full((R, ld), float("nan"), device=DEV, dtype=torch.float16)
    buf[:, :C] = x16
    return buf[:, :C]


# =====================================================================================================
# LayerNorm and row_stats (vda_norm.hip: layernorm_kernel, layernorm_narrow_kernel<16|32|64>, row_stats_kernel)
# =====================================================================================================
LN_ROWS = [1, 3, 4, 5, 15, 16, 17, 33]


def c_layernorm(x, g, b, rows, eps, skip=0):
    """vda_layernorm through the C ABI into a sentinel-guarded output."""
    C = x.shape[1]
    buf, out = guarded((rows, C))
    rc = lib().vda_layernorm(x.data_ptr(), x.stride(0), out.data_ptr(), g.data_ptr(), b.data_ptr(), rows, C, eps, skip, stream())
    assert rc == 0, lib().vda_last_error().decode()
    return buf, out


@pytest.mark.parametrize("C", fb.LN_CS)
def test_layernorm_edges(C):
    """C = 128 / 256 / 512: the narrow kernels (16 / 32 / 64 lanes per row, 4 / 2 / 1 rows per wave); the others
    the one-wave-per-row kernel with 1 (C = 8, 64, 384: part of a wave), 2 (520: one lane of the second chunk),
    3, 4 (2040: a ragged last chunk; 2048) chunks per lane.  rows around the rows-per-wave and 4-waves-per-block
    edges; contiguous, ldx = C + 8 and ldx = 2 C inputs with NaN between the rows; eps 1e-6 and 1e-5; the last
    four rows of every case are the stress rows of fp16_bounds.ln_rows."""
    X = fb.ln_rows(33, C)
    g, b = fb.gn_affine(C, seed=C)
    gd, bd = f32(g), f32(b)
    worst = wstat = 0.0
    for eps in (1e-6, 1e-5):
        ref, bound = fb.layernorm_ref_bound(X, g, b, eps)
        sref, sbound = fb.ln_stats_ref_bound(X, eps)
        for R in LN_ROWS:
            lo = X.shape[0] - R  # the stress rows first: every R has the all-zero row, R >= 4 all four
            for ld in (C, C + 8, 2 * C):
                if eps == 1e-5 and (ld != C + 8 or R not in (5, 33)):
                    continue
                x = strided(h(X[lo:]), ld)
                what = f"layernorm C={C} rows={R} ldx={ld} eps={eps}"
                buf, y = c_layernorm(x, gd, bd, R, eps)
                worst = max(worst, assert_elementwise(y, ref[lo:], bound[lo:], what))
                assert rel(y, ref[lo:]) < BAR, what
                assert guard_ok(buf), f"{what}: a store outside the output"
                assert torch.equal(y, ops.layernorm(x, gd, bd, eps)), f"{what}: ops.layernorm differs from the C ABI"
                st = torch.full((R + 3, 2), float("nan"), device=DEV)
                rc = lib().vda_row_stats(x.data_ptr(), x.stride(0), st.data_ptr(), R, C, eps, stream())
                assert rc == 0
                wstat = max(wstat, assert_elementwise(st[:R], sref[lo:], sbound[lo:], what + " row_stats"))
                assert bool(torch.isnan(st[R:]).all()), f"{what}: row_stats wrote past row {R - 1}"
                assert torch.equal(ops.row_stats(x, eps)[:R], st[:R])
    note(f"layernorm C={C} (row_stats {wstat:.3f})", worst)


@pytest.mark.parametrize("np_,BT", [(1, 5), (2, 3), (10, 3)])
@pytest.mark.parametrize("C", [256, 384, 512])
def test_layernorm_skip_period_edges(C, np_, BT):
    """skip_period (each frame's first row dropped): frames of 1, 2 and 10 kept rows, BT such that the last frame
    ends part-way into a block (5, 6 and 30 output rows), on a narrow and the general kernel, from a strided input."""
    X = (fb.rnd16(BT * (np_ + 1), C, seed=C + np_) * 2 + 0.5).half().float()
    X[::np_ + 1] = 777.0  # the dropped rows: they must not be read into any output
    g, b = fb.gn_affine(C, seed=C)
    keep = torch.arange(X.shape[0]) % (np_ + 1) != 0
    ref, bound = fb.layernorm_ref_bound(X[keep], g, b, 1e-6)
    x = strided(h(X), C + 8)
    buf, y = c_layernorm(x, f32(g), f32(b), BT * np_, 1e-6, skip=np_)
    worst = assert_elementwise(y, ref, bound, f"layernorm skip {np_} C={C}")
    assert rel(y, ref) < BAR and guard_ok(buf)
    assert torch.equal(y, ops.layernorm(x, f32(g), f32(b), 1e-6, skip_period=np_))
    note(f"layernorm skip_period={np_} C={C}", worst)


@pytest.mark.parametrize("C", [128, 256, 512, 1024])
def test_layernorm_nan_row_isolation_and_determinism(C):
    """One NaN row leaves every other row bit-identical to the run without it (the narrow kernels share a wave
    between 4 / 2 rows: a shuffle one level too wide would mix them); two runs give the same bits."""
    X = fb.ln_rows(13, C)
    g, b = f32(fb.gn_affine(C)[0]), f32(fb.gn_affine(C)[1])
    x = h(X)
    y = ops.layernorm(x, g, b, 1e-6)
    assert torch.equal(y, ops.layernorm(x, g, b, 1e-6))
    st = ops.row_stats(x, 1e-6)
    for bad in (0, 6, 7, 16):
        xn = x.clone()
        xn[bad] = float("nan")
        yn, sn = ops.layernorm(xn, g, b, 1e-6), ops.row_stats(xn, 1e-6)
        others = torch.arange(x.shape[0], device=DEV) != bad
        assert torch.equal(yn[others], y[others]) and bool(torch.isnan(yn[bad]).all()), f"C={C}: NaN row {bad} leaked"
        assert torch.equal(sn[:x.shape[0]][others], st[:x.shape[0]][others])


# =====================================================================================================
# row_partials_kernel: stats_out of a GEMM on the one-tile-per-block route
# =====================================================================================================
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("N", [8, 248, 256, 264, 504, 512])
def test_row_partials_edges(N, M):
    """stats_out behind a tile GEMM (force_tile = 0, as test_gemm_phased_res_stats_out forces its route) is the
    separate row_partials pass over the stored output: N below / at / above one and two 256-column blocks (a
    ragged last block), the output a view with ldy = N + 16 inside a sentinel frame, a NaN spare statistics row.
    Held to fp16_bounds.row_stats_ref_bound on the kernel's own stored rows, zero-padded to whole blocks."""
    T = tune_lib()
    K, P = 64, (N + 255) // 256
    c = fb.gemm_case(M, N, K, "bias", seed=N + M)
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], **c["kw"])
    buf = torch.full((M + 8, N + 16), SENT, device=DEV, dtype=torch.float16)
    out = buf[4:4 + M, 8:8 + N]
    stats = torch.full((M + 1, P, 2), float("nan"), device=DEV)
    with T.route(force_tile=0):
        T.gemm_kw(h(c["x"]), h(c["w"]), out, bias=f32(c["kw"]["bias"]), stats_out=stats)
    assert_elementwise(out, ref, bound, f"gemm {M}x{N}")
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[4:4 + M, 8:8 + N] = False
    assert bool((buf[mask] == SENT).all())
    ypad = torch.zeros(M, P * 256, dtype=torch.float16)
    ypad[:, :N] = out.cpu()
    sref, sbound = fb.row_stats_ref_bound(ypad)
    worst = assert_elementwise(stats[:M], sref, sbound, f"row_partials N={N} M={M}")
    assert bool(torch.isnan(stats[M]).all()), "the spare statistics row was written"
    note(f"row_partials N={N} M={M}", worst)


# =====================================================================================================
# GroupNorm, both routes (gn_partial / gn_finalize / gn_apply with a workspace; groupnorm_kernel<8|4|2> without)
# =====================================================================================================
def c_groupnorm(x, g, b, Fr, S, C, groups, eps, with_ws):
    """vda_groupnorm through the C ABI into a sentinel-guarded output; the workspace (the route ops.groupnorm
    takes) is NaN-filled first: every partial that gn_finalize reads must have been written by gn_partial."""
    buf, out = guarded((Fr * S, C))
    ws = None
    if with_ws:
        ws = torch.full((max(int(lib().vda_groupnorm_workspace(Fr, S, C, groups)), 1),), float("nan"), device=DEV)
    rc = lib().vda_groupnorm(x.data_ptr(), out.data_ptr(), g.data_ptr(), b.data_ptr(), Fr, S, C, groups, eps,
                             ws.data_ptr() if with_ws else None, stream())
    assert rc == 0, lib().vda_last_error().decode()
    return buf, out


def run_groupnorm(x, g, b, groups, eps, what):
    """x [F, S, C] on both routes against groupnorm_ref_bound; returns the worst ratio of (workspace, two-pass)."""
    Fr, S, C = x.shape
    ref, bound = fb.groupnorm_ref_bound(x, g, b, groups, eps)
    ref, bound = ref.view(-1, C), bound.view(-1, C)
    xh, gd, bd = h(x.view(-1, C)), f32(g), f32(b)
    worst = []
    for with_ws in (True, False):
        route = "workspace" if with_ws else "two-pass"
        buf, y = c_groupnorm(xh, gd, bd, Fr, S, C, groups, eps, with_ws)
        worst.append(assert_elementwise(y, ref, bound, f"{what} {route}"))
        assert rel(y, ref) < BAR, f"{what} {route}"
        assert guard_ok(buf), f"{what} {route}: a store outside the output"
        if with_ws:
            yo = ops.groupnorm(xh, gd, bd, Fr, groups, eps)
            assert torch.equal(y, yo), f"{what}: ops.groupnorm differs from the C ABI with a workspace"
            assert torch.equal(yo, ops.groupnorm(xh, gd, bd, Fr, groups, eps)), f"{what}: not deterministic"
    return worst


@pytest.mark.parametrize("Fr", fb.GN_FRAMES)
@pytest.mark.parametrize("C,groups", fb.GN_SHAPES)
def test_groupnorm_edges(C, groups, Fr):
    """Channels per group 2, 4, 6, 8, 12, 32, 64 (a group inside, equal to and spanning 16-byte chunks; 3 and 6
    chunks per row leave idle threads; C = 2048 has one row-lane), S around both chunk heights (128 rows below
    C = 512, 32 from there: one row, one short chunk, a full one, a ragged second and third), one and three
    frames (the middle one offset by +40)."""
    g, b = fb.gn_affine(C, seed=C)
    worst = [0.0, 0.0]
    for S in fb.GN_S:
        w = run_groupnorm(fb.gn_case(Fr, S, C), g, b, groups, 1e-6, f"groupnorm C={C} groups={groups} S={S} F={Fr}")
        worst = [max(a, c) for a, c in zip(worst, w)]
    note(f"groupnorm C={C} groups={groups} F={Fr} (two-pass {worst[1]:.3f})", worst[0])


@pytest.mark.parametrize("kind", fb.GN_OUTLIER_KINDS)
@pytest.mark.parametrize("S,C,v0", fb.GN_OUTLIER_SIZES)
def test_groupnorm_outlier(S, C, v0, kind):
    """One massive activation per frame, at the group's first value of the frame (where the workspace route used
    to take its shift: test_fp16_bounds.py shows that arithmetic 3 .. 50 bounds out, up to rstd = 1 / sqrt(eps)), in
    the middle of the map, with the rest of the group at sigma 0.01, and in frame 1 of 3.  Both routes inside the
    same bound, every output finite."""
    x, _ = fb.gn_outlier_case(S, C, v0, kind)
    g, b = fb.gn_affine(C, seed=C)
    worst = run_groupnorm(x, g, b, 32, 1e-6, f"groupnorm outlier S={S} C={C} v0={v0} {kind}")
    note(f"groupnorm outlier S={S} C={C} v0={v0} {kind} (two-pass {worst[1]:.3f})", worst[0])


def test_groupnorm_nan_frame_isolation():
    """A NaN frame between two others: their outputs are bit-identical to the calls on each alone."""
    S, C = 129, 256
    x = h(fb.gn_case(3, S, C).view(-1, C))
    g, b = f32(fb.gn_affine(C)[0]), f32(fb.gn_affine(C)[1])
    xn = x.clone()
    xn[S:2 * S] = float("nan")
    y = ops.groupnorm(xn, g, b, 3, 32, 1e-6)
    for f in (0, 2):
        assert torch.equal(y[f * S:(f + 1) * S], ops.groupnorm(x[f * S:(f + 1) * S].contiguous(), g, b, 1, 32, 1e-6))
    assert bool(torch.isnan(y[S:2 * S]).all())


# =====================================================================================================
# GroupNorm -> Linear, fused (gn_linear_kernel<64|128|256>)
# =====================================================================================================
def run_gnl(x, C, what, equal_composition=False):
    Fr, S, _ = x.shape
    M = Fr * S
    g, b = fb.gn_affine(C, seed=C)
    w, bias = fb.rnd16(C, C, scale=C ** -0.5, seed=C + 1), fb.rnd32(C, scale=0.1, seed=C + 2)
    assert lib().vda_groupnorm_linear_fused(C, 32, C) == 1
    ref, bound = fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, bias)
    xh, gd, bd, wd, biasd = h(x.view(-1, C)), f32(g), f32(b), h(w), f32(bias)
    # through the C ABI: the output in a sentinel frame, the workspace NaN-filled, a NaN guard row after the statistics
    buf, y = guarded((M, C))
    st = torch.full((M + 1, 1, 2), float("nan"), device=DEV)
    wsb = int(lib().vda_groupnorm_linear_workspace(Fr, S, C, 32, C))
    ws = torch.full((wsb // 4 + 4,), float("nan"), device=DEV)
    rc = lib().vda_groupnorm_linear(xh.data_ptr(), gd.data_ptr(), bd.data_ptr(), Fr, S, C, 32, 1e-6, wd.data_ptr(),
                                    biasd.data_ptr(), y.data_ptr(), C, st.data_ptr(), ws.data_ptr(), wsb, stream())
    assert rc == 0, lib().vda_last_error().decode()
    worst = assert_elementwise(y, ref, bound, what)
    assert rel(y, ref) < BAR, what
    assert guard_ok(buf), f"{what}: a store outside the output"
    sref, sbound = fb.sums_ref_bound(y)
    assert_elementwise(st[:M, 0], sref, sbound, what + " stats_out")
    assert bool(torch.isnan(st[M]).all()), f"{what}: stats_out written past row M - 1"
    yo = ops.groupnorm_linear(xh, gd, bd, Fr, 32, 1e-6, wd, bias=biasd)
    assert torch.equal(y, yo), f"{what}: ops.groupnorm_linear differs from the C ABI"
    assert torch.equal(yo, ops.groupnorm_linear(xh, gd, bd, Fr, 32, 1e-6, wd, bias=biasd)), f"{what}: not deterministic"
    unf = ops.gemm(ops.groupnorm(xh, gd, bd, Fr, 32, 1e-6), wd, bias=biasd)  # this library's own composition
    assert rel(y, unf) < 2e-4, what
    if equal_composition:  # against the phased GEMM: the same operand bits and the same K order
        assert torch.equal(y, unf), f"{what}: the fused kernel and GroupNorm + GEMM differ"
    yn = ops.groupnorm_linear(xh, gd, bd, Fr, 32, 1e-6, wd)  # without the bias
    assert_elementwise(yn, *fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, None), what + " no bias")
    return worst


@pytest.mark.parametrize("C,S,Fr", fb.GNL_CASES)
def test_groupnorm_linear_edges(C, S, Fr):
    """M = F S in {1, 15, 16, 17, 128 k +- 1} rows (a ragged last 16-row tile, one row more or less than whole blocks
    of 8 waves), frames of 1, 5, 7, 15, 16, 17, 37 rows (a tile spans up to four frames: each lane looks up its own
    row's frame), 900 x 37 rows at C = 64 (2,082 tiles > 8 waves x 256 CUs: both register sets of the tile loop);
    with and without bias, stats_out with a NaN guard row."""
    worst = run_gnl(fb.gn_case(Fr, S, C, seed=3), C, f"groupnorm_linear C={C} S={S} F={Fr}")
    note(f"groupnorm_linear C={C} S={S} F={Fr}", worst)


@pytest.mark.parametrize("C,S,Fr", [(384, 37, 3), (768, 19, 5)])
def test_groupnorm_linear_unfused_vitb_widths(C, S, Fr):
    """ViT-B's motion modules 0 and 1 (C = N = 384 and 768, 12 and 24 channels per group): no fused kernel
    (vda_groupnorm_linear_fused says 0), so ops.groupnorm_linear is GroupNorm into a workspace + vda_gemm on the same
    fp16 operand.  The output under groupnorm_linear_ref_bound and bit-identical to ops.groupnorm + ops.gemm;
    stats_out ([M, ceil(N / 256), 2], the last part of C = 384 is 128 columns wide) against float64 sums of the stored
    rows, with a NaN guard row after row M - 1; the middle frame carries the +40 offset."""
    assert lib().vda_groupnorm_linear_fused(C, 32, C) == 0
    x = fb.gn_case(Fr, S, C, seed=3)
    M, P = Fr * S, (C + 255) // 256
    g, b = fb.gn_affine(C, seed=C)
    w, bias = fb.rnd16(C, C, scale=C ** -0.5, seed=C + 1), fb.rnd32(C, scale=0.1, seed=C + 2)
    ref, bound = fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, bias)
    xh, gd, bd, wd, biasd = h(x.view(-1, C)), f32(g), f32(b), h(w), f32(bias)
    st = torch.full((M + 1, P, 2), float("nan"), device=DEV)
    y = ops.groupnorm_linear(xh, gd, bd, Fr, 32, 1e-6, wd, bias=biasd, stats_out=st)
    what = f"groupnorm_linear unfused C={C} S={S} F={Fr}"
    worst = assert_elementwise(y, ref, bound, what)
    assert rel(y, ref) < BAR, what
    assert torch.equal(y, ops.gemm(ops.groupnorm(xh, gd, bd, Fr, 32, 1e-6), wd, bias=biasd)), f"{what}: not the composition"
    assert torch.equal(y, ops.groupnorm_linear(xh, gd, bd, Fr, 32, 1e-6, wd, bias=biasd)), f"{what}: not deterministic"
    ypad = torch.zeros(M, P * 256, dtype=torch.float16)  # zero columns add nothing to a part's sums
    ypad[:, :C] = y.cpu()
    sref, sbound = fb.row_stats_ref_bound(ypad)
    ws = assert_elementwise(st[:M], sref, sbound, what + " stats_out")
    assert bool(torch.isnan(st[M]).all()), f"{what}: stats_out written past row M - 1"
    note(f"{what} (stats {ws:.3f})", worst)


def test_groupnorm_linear_outlier_frame():
    """The fused operand built from the repaired statistics: frame 1 of 2 carries the first-position outlier at
    74 x 74 x 256; M = 10,952 rows, where the composition's GEMM is the phased kernel: bit-identical."""
    S, C, v0 = fb.GN_OUTLIER_SIZES[0]
    x, _ = fb.gn_outlier_case(S, C, v0, "first_frame1of3")
    worst = run_gnl(x[:2].contiguous(), C, "groupnorm_linear outlier frame", equal_composition=True)
    note("groupnorm_linear outlier frame", worst)


# =====================================================================================================
# Bilinear resize (upsample_kernel)
# =====================================================================================================
@pytest.mark.parametrize("kind", ["rand", "checker"])
@pytest.mark.parametrize("BT,H,W,C,Ho,Wo", fb.UPSAMPLE_CASES)
def test_upsample_edges(BT, H, W, C, Ho, Wo, kind):
    """From and to 1 x 1 (scale 0), identity, x2 exactly (every pair shares its source rows) and x2 - 1, downscales
    (no pair shares), odd Ho with 2 and 3 frames (a pair straddles two frames) and an odd total row count (the last
    row has no partner), W = 1, C = 8 .. 256 with Wo C / 8 below, at and above one block's 512 items, and
    131,075 output rows (the gridDim.y stride loop).  Random values and a +-60000 checkerboard (the largest fp16
    corner differences; the weights' fp32 error times them is in the bound)."""
    x = fb.upsample_input(BT, H, W, C, kind)
    ref, bound = fb.upsample_ref_bound(x, Ho, Wo)
    xh = h(x)
    buf, y = guarded((BT, Ho, Wo, C))
    rc = lib().vda_upsample_bilinear(xh.data_ptr(), y.data_ptr(), BT, H, W, C, Ho, Wo, stream())
    assert rc == 0, lib().vda_last_error().decode()
    what = f"resize {BT}x{H}x{W}x{C} -> {Ho}x{Wo} {kind}"
    worst = assert_elementwise(y, ref, bound, what)
    assert rel(y, ref) < BAR, what
    assert guard_ok(buf), f"{what}: a store outside the output"
    assert torch.equal(y, ops.upsample_bilinear(xh, Ho, Wo)), f"{what}: ops differs from the C ABI / not deterministic"
    note(what, worst)


def test_upsample_nan_frame_isolation():
    x = h(fb.upsample_input(3, 4, 5, 40))
    xn = x.clone()
    xn[1] = float("nan")
    y = ops.upsample_bilinear(xn, 9, 6)  # 27 rows: the pairs (8, 9) and (17, 18) straddle the NaN frame's edges
    for f in (0, 2):
        assert torch.equal(y[f], ops.upsample_bilinear(x[f:f + 1].contiguous(), 9, 6)[0])


# =====================================================================================================
# im2col (exact)
# =====================================================================================================
@pytest.mark.parametrize("Kp", [592, 640])
@pytest.mark.parametrize("BT", [1, 3])
@pytest.mark.parametrize("W", [14, 14 * 13, 14 * 14, 14 * 40])
def test_patch_im2col_exact(W, BT, Kp):
    """One patch, 13 patches (one whole group), 14 (a ragged second group) and 40 per row (where the halving of
    the group size for small grids ends at 3), H = 14; Kp = 592 and 640 (zero padding beyond 588): bit for bit
    the index gather of the fp16-rounded image, the cls rows zero, nothing written around the output."""
    img = fb.rnd32(BT, 3, 14, W, seed=W + BT)
    ref = fb.patch_im2col_ref(img, Kp)
    imgd = img.to(DEV).contiguous()
    buf, a = guarded(tuple(ref.shape))
    rc = lib().vda_patch_im2col(imgd.data_ptr(), a.data_ptr(), BT, 14, W, Kp, stream())
    assert rc == 0, lib().vda_last_error().decode()
    assert torch.equal(a.cpu(), ref)
    assert guard_ok(buf)
    assert torch.equal(ops.patch_im2col(imgd, Kp), a)


def test_patch_im2col_rejects_unpadded_k():
    img = torch.zeros(1, 3, 14, 14, device=DEV)
    with pytest.raises(RuntimeError, match="Kp"):
        ops.patch_im2col(img, 588)  # 588 % 8 != 0


@pytest.mark.parametrize("BT,Cin,H,W", [(1, 64, 127, 127), (1, 256, 127, 131), (1, 1024, 127, 127), (3, 64, 74, 74),
                                        (1, 64, 513, 513)])
def test_conv_im2col_exact(BT, Cin, H, W):
    """conv_im2col_kernel is reached through vda_conv2d only (3x3, stride 2, pad 1, Cin % 64 == 0, Cout % 256 == 0,
    M >= 4096, no pre-ReLU: the router's conv_takes_im2col): Cin = 64 / 256 / 1024 (72, 288 and 1,152 chunks per row
    of A: one, two and five x-blocks), odd maps (the padding column and row on both sides), three frames, and
    M = 66,049 > 65,535 rows (the y stride loop).  The gather itself is exact, so the route's output must equal the
    implicit-GEMM conv's (force_tile = -2: the same K order) bit for bit, in a sentinel frame; the smaller cases
    are also held to the conv bound."""
    T = tune_lib()
    c = fb.conv_case(BT, Cin, 256, H, W, "rcu2", stride=2, seed=H + Cin)
    nh = lambda t: h(t.permute(0, 2, 3, 1))  # noqa: E731
    x, w = nh(c["x"]), nh(c["w"])
    gk = dict(stride=2, pad=1, bias=f32(c["kw"]["bias"]), res=nh(c["kw"]["res"]), res2=nh(c["kw"]["res2"]))
    assert lib().vda_conv2d_workspace(BT, H, W, Cin, 256, 3, 2, 1) == BT * c["Ho"] * c["Wo"] * 9 * Cin * 2  # the route is taken
    buf, out = guarded((BT, c["Ho"], c["Wo"], 256))
    T.conv2d(x, w, out=out, **gk)
    assert guard_ok(buf)
    with T.route(force_tile=-2):
        out2 = T.conv2d(x, w, **gk)
    assert torch.equal(out, out2)
    assert torch.equal(out, ops.conv2d(x, w, **gk))
    if BT * c["Ho"] * c["Wo"] * Cin <= 4096 * 256:
        ref, bound = fb.conv_ref_bound(c["x"], c["w"], staged=True, **c["kw"])
        worst = assert_elementwise(out, ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1), f"im2col conv Cin={Cin} {H}x{W}")
        note(f"im2col conv Cin={Cin} {H}x{W}", worst)


# =====================================================================================================
# Depth tail (vda_depth_head: vda_dconv.hip fused / unfused, the implicit-GEMM depth kernel)
# =====================================================================================================
def c_depth_head(L, xh, split, b1, w2, b2, Ho, Wo):
    """vda_depth_head of library L (ctypes) into a sentinel-guarded fp32 output."""
    BT, H, W, C = xh.shape
    buf, dep = guarded((BT, Ho, Wo), torch.float32)
    wsb = int(L.vda_depth_head_workspace(BT, H, W, C, Ho, Wo))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    rc = L.vda_depth_head(xh.data_ptr(), split.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dep.data_ptr(),
                          ws.data_ptr() if wsb > 0 else None, BT, H, W, C, Ho, Wo, stream())
    assert rc == 0, L.vda_last_error().decode()
    return buf, dep


@pytest.mark.parametrize("BT", [1, 2])
@pytest.mark.parametrize("C,Hin,Win,Ho,Wo", fb.DEPTH_CASES)
def test_depth_head_edges(C, Hin, Win, Ho, Wo, BT):
    """C = 32 / 64 / 128 (the depth conv of vda_dconv.hip, the resize fused into its patches for upscales, through
    the materialised resize for the downscale) and C = 40 (the implicit-GEMM depth kernel); 1 x 1 -> 1 x 1, a 1 x 1
    source, partial 16 x 16 tiles, an identity resize, a downscale; the fp32 output in a sentinel frame.  Also the
    implicit-GEMM depth kernel forced (tuning build, force_tile = 13) under the same bound, and the old 1e-5 bar."""
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hin, Win, BT, seed=C)
    ref, bound = fb.depth_head_ref_bound(x, w1, b1, w2, b2, Ho, Wo)
    hi, lo = fb.split_hi_lo(w1.permute(0, 2, 3, 1).contiguous())
    args = (torch.cat([hi, lo], 0).to(DEV).contiguous(), f32(b1), f32(w2), f32(b2), Ho, Wo)
    xh = h(x.permute(0, 2, 3, 1))
    what = f"depth tail C={C} {Hin}x{Win}->{Ho}x{Wo} BT={BT}"
    # the old bar's own reference (test_depth_head_fp32): torch's fp32 resize rounded to fp16, the fp32 weights
    up = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True).half().float()
    ref32 = F.relu(F.conv2d(F.relu(F.conv2d(up, w1, b1, padding=1)), w2.view(1, -1, 1, 1), b2))[:, 0]
    buf, y = c_depth_head(lib(), xh, *args)
    worst = assert_elementwise(y, ref, bound, what)
    assert rel(y, ref32) < 1e-5, what
    assert guard_ok(buf), f"{what}: a store outside the output"
    assert torch.equal(y, ops.depth_head(xh, *args)), f"{what}: ops.depth_head differs from the C ABI"
    T = tune_lib()
    with T.route(force_tile=13):
        buf2, y2 = c_depth_head(T.lib, xh, *args)
    w13 = assert_elementwise(y2, ref, bound, what + " implicit GEMM")
    assert rel(y2, ref32) < 1e-5 and guard_ok(buf2)
    note(what + f" (implicit GEMM forced {w13:.3f})", worst)


# To 33 x 33 the scale is (Hs - 1) / 32, exact in fp32.  A 16 x 16 tile stages a source window of at most
# (int)(17 sy) + 3 rows x (int)(17 sx) + 3 columns in a 192-pixel slot: 22 x 21 and 21 x 22 give 14 x 13 = 182
# pixels (served), 22 x 22 gives 14 x 14 = 196 (declined).  The served shapes put a 13 x 12 = 156-pixel window in
# the second tile (y0 = 16: source rows 9..21).
STAGING_OUT = 33
STAGING_CASES = [(22, 21, True), (21, 22, True), (22, 22, False)]


def staging_case(C, Hs, Ws, BT):
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hs, Ws, BT, seed=C + Hs * Ws)
    hi, lo = fb.split_hi_lo(w1.permute(0, 2, 3, 1).contiguous())
    args = (torch.cat([hi, lo], 0).to(DEV).contiguous(), f32(b1), f32(w2), f32(b2), STAGING_OUT, STAGING_OUT)
    return (x, w1, b1, w2, b2), h(x.permute(0, 2, 3, 1)), args


# C = 32 keeps the ids it had before C = 64 joined it
STAGING_C = [pytest.param(C, *case, id=("" if C == 32 else f"C{C}-") + "-".join(str(v) for v in case))
             for C in (32, 64) for case in STAGING_CASES]


@pytest.mark.parametrize("BT", [1, 2])
@pytest.mark.parametrize("C,Hs,Ws,served", STAGING_C)
def test_depth_head_staging_boundary(C, Hs, Ws, served, BT):
    """Both sides of the one predicate (halo_fused_fits) that decides whether the depth conv builds its patches
    from a staged source window, and with it the depth head's workspace: C = 32 and 64 (one and two 32-channel
    slabs), no workspace where served and the resized map where declined; the output within the bound, bit for
    bit the materialised resize + the same conv (tuning build, dconv = 2), and nothing stored outside it."""
    S = STAGING_OUT
    case, xh, args = staging_case(C, Hs, Ws, BT)
    ref, bound = fb.depth_head_ref_bound(*case, S, S)
    what = f"depth tail staging C={C} {Hs}x{Ws}->{S}x{S} BT={BT}"
    assert lib().vda_depth_head_workspace(BT, Hs, Ws, C, S, S) == (0 if served else BT * S * S * C * 2), what
    buf, y = c_depth_head(lib(), xh, *args)
    worst = assert_elementwise(y, ref, bound, what)
    assert guard_ok(buf), f"{what}: a store outside the output"
    T = tune_lib()
    with T.route(dconv=2):
        buf2, y2 = c_depth_head(T.lib, xh, *args)
    assert torch.equal(y, y2), f"{what}: differs from resize + conv"
    assert guard_ok(buf2)
    note(what, worst)


@pytest.mark.parametrize("C,Hin,Win,Ho,Wo", [(64, 8, 20, 33, 47), (64, 37, 37, 19, 19), (40, 9, 9, 15, 17)])
def test_depth_head_nan_frame_isolation(C, Hin, Win, Ho, Wo):
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hin, Win, 1, seed=C)
    hi, lo = fb.split_hi_lo(w1.permute(0, 2, 3, 1).contiguous())
    args = (torch.cat([hi, lo], 0).to(DEV).contiguous(), f32(b1), f32(w2), f32(b2), Ho, Wo)
    xh = h(x.permute(0, 2, 3, 1))
    x3 = torch.full((3,) + tuple(xh.shape[1:]), float("nan"), device=DEV, dtype=torch.float16)
    x3[1] = xh[0]
    single, triple = ops.depth_head(xh, *args), ops.depth_head(x3, *args)
    assert bool(torch.isfinite(triple[1]).all()) and torch.equal(triple[1], single[0])
