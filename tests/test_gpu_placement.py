"""Every fp16 and fp32 kernel route with its operands surrounded by poison and its workspaces exact and guarded.

tests/test_gpu_fp16_edges.py and its siblings hold what a kernel WRITES to sentinel frames and per-element
bounds; their operands are fresh tensors, whose surroundings are whatever the caching allocator left (finite,
mostly zero), and garbage times a zero-padded partner is zero.  Here every pointer that crosses the C ABI is
placed by tests/placement.py: exactly at the alignment include/vda.h promises, with zeros, quiet NaN or +Inf
before it, after it and between strided rows; every workspace has exactly the `*_workspace()` size inside a
guard and runs prefilled with 0x00 and 0xFF bytes.  run_placed asserts bit identity of every output across the
fills, the op's own bound (fp16_bounds / swiglu_bounds / stagelib bars, the fp32 tests' 2e-6) on the zero-fill
run, intact output frames, bitwise unchanged input buffers and intact workspace guards.  One case per route at
its smallest tailed shape (an M or pixel tail, an N or channel tail, a K that is no multiple of the K step), two
frames for the convs so that row -1 of the first and row H of the last frame are poison.

pytest -s prints per family the number of (route, shape, fill) runs and the worst zero-fill |y - ref| / bound
(DESIGN.md records them).  tests/test_placement.py shows on the CPU that each check catches its leak.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fp16_bounds as fb
import stagelib as SL
import swiglu_bounds as sb
import vda_amd
from head_linear_ref import CHAINS, Case, Case3
from helpers import assert_elementwise
from placement import In, Out, report, run_placed, same_bits
from tunelib import _attn_scale, tune_lib
from vda_amd import _lib, weights
from vda_amd._lib import ACT_GEGLU, ACT_RELU, ACT_SWIGLU
from vda_amd.model import _geglu_interleave

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_GEMM, BAR_ATTN, BAR_OP, TOL_F32 = 2e-3, 3e-3, 2e-3, 2e-6
TILES = {0: (128, 128), 1: (256, 128), 2: (128, 64), 3: (256, 256), 6: (64, 64), 7: (64, 128)}
TALLY = {}


def placed(family, call, ins, outs, ws=None, check=None, what=""):
    return run_placed(call, ins, outs, ws, check=check, what=what, device=DEV, tally=TALLY.setdefault(family, [0, 0.0]))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def H16(t, **kw):
    return In(t.to(torch.float16), **kw)


def F32(t, **kw):
    return In(t.to(torch.float32), **kw)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vda_amd._libvda()


def ok(L, rc, what):
    assert rc == 0, f"{what}: {L.vda_last_error().decode()}"


def il(a, b):
    return _geglu_interleave(torch.cat([a, b]))


def bounded(name, ref, bound, what, bar=None):
    """check(outs): output `name` inside the per-element bound (and the whole-tensor rel-L1 bar of its own test)."""
    def check(outs):
        worst = assert_elementwise(outs[name], ref, bound, what)
        if bar is not None:
            assert rel(outs[name], ref) < bar, what
        return worst
    return check


def test_harness_catches_a_leak_on_the_device():
    """tests/test_placement.py's first leak with torch's own device kernels in the kernel's place: the K loop runs to
    64 over a zero-padded W and an X read past its 40 columns.  The faithful product passes on the device, the
    leaky one is reported under the NaN fill and named, and a stale workspace by the 0xFF prefill."""
    x, w = fb.rnd16(5, 40, seed=1), fb.rnd16(12, 40, seed=2)
    ref = x.double() @ w.double().t()

    def mm(a, b):  # [M, K] x [N, K]^T without a BLAS call
        return (a.float()[:, None, :] * b.float()[None, :, :]).sum(-1)

    def faithful(i, o, ws):
        o["out"].copy_(mm(i["x"], i["w"]))

    def leaky(i, o, ws):
        xe = i["x"].as_strided((5, 64), (i["x"].stride(0), 1), i["x"].storage_offset())
        o["out"].copy_(mm(xe, torch.cat([i["w"], torch.zeros(12, 24, device=DEV, dtype=torch.float16)], 1)))

    def stale(i, o, ws):
        acc = ws["acc"].view(torch.float32).view(5, 12)
        acc += mm(i["x"], i["w"])
        o["out"].copy_(acc)

    def check(o):
        err = float((o["out"].double() - ref).abs().max())
        assert err < 1e-4
        return err / 1e-4
    ins, outs = dict(x=F32(x, ld=48), w=F32(w)), dict(out=Out((5, 12), torch.float32, ld=16))
    ins16 = dict(x=H16(x, ld=48), w=H16(w))
    assert run_placed(faithful, ins, outs, check=check, device=DEV)["runs"] == 3
    with pytest.raises(AssertionError, match=r"\(a\) bit identity.*nan fill.*\['x'\]"):
        run_placed(leaky, ins16, outs, check=check, device=DEV)
    with pytest.raises(AssertionError, match=r"\(e\) workspace prefill"):
        run_placed(stale, ins, outs, {"acc": 5 * 12 * 4}, check=check, device=DEV)


# =====================================================================================================
# vda_gemm
# =====================================================================================================
def ps_shuffle(t, BT, hin, win, k, cout):
    return t.reshape(BT, hin, win, k, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(BT, hin * k, win * k, cout)


def gemm_placed(c, launch, what, staged=False, align16=False, extra_out=None, extra_check=None, rows=None, ref_bound=None,
                align8=False, same_as=None, same_as_drop=()):
    """One dense-GEMM case of fp16_bounds.gemm_case / gemm_ln_case / swiglu_bounds.swiglu_case, every operand
    placed.  launch(x, w, out, gk) runs it (TuneLib.gemm_kw keywords).  align16: res / res2 rows 16-byte aligned
    (the phased route's contract) instead of 8.  staged: the phased kernels' rounding points.  extra_out: further
    outputs (name -> Out) handed to launch through gk; rows: the output's row count when it is not M.
    align8: y, res and res2 START 8 bytes past a 256-byte boundary, the weakest base vda.h gives vda_gemm's row
    store (the one-tile kernels).  c["inplace"] = False runs gamma_res with res a placed input of its own (in place,
    res is the output and its surroundings the finite sentinel: only the separate operand has poison after row M).
    same_as: a second launch function (the kernel this case is about, forced) whose zero-fill outputs must have the
    same bits, so that a routing change cannot turn the case into a test of another kernel unnoticed;
    same_as_drop: outputs that launch does not get."""
    M, N, K, epi, kw = c["M"], c["N"], c["K"], c["epi"], c["kw"]
    ln = kw.get("ln")
    gated = "wg" in kw
    if ref_bound is not None:
        ref, bound = ref_bound
    elif epi == "swiglu":
        ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], staged=staged, **kw)
    else:
        ref, bound = fb.gemm_ref_bound(c["x"], c["w"], staged=staged, phi_table=staged, **kw)
    ins = dict(x=H16(c["x"], ld=3 * K if epi == "strided_x" else None))
    static = {}
    if gated:
        ins["w"], ins["bias"] = H16(il(c["w"], kw["wg"])), F32(il(kw["bias"], kw["bg"]))
        static["act"] = ACT_SWIGLU if epi == "swiglu" else ACT_GEGLU
        n_out = N // 2
    else:
        ins["w"], n_out = H16(c["w"]), N
        for k in ("bias", "rowbias", "gamma"):
            if k in kw:
                ins[k] = F32(kw[k])
        static.update({k: kw[k] for k in ("rdiv", "rmod", "act") if k in kw})
    if ln is not None:
        parts = ln["parts"].shape[1] if "parts" in ln else 0
        ins["ln_stats"] = F32(ln["parts"] if parts else torch.stack([ln["mean"], ln["rstd"]], -1))
        ins["ln_colsum"] = F32(il(ln["colsum"], ln["colsum_g"]) if gated else ln["colsum"])
        static.update(ln_parts=parts, ln_eps=1e-6)
    outs = dict(extra_out or {})
    oa = 8 if align8 else 16
    inplace = epi == "gamma_res" and c.get("inplace", True)
    if epi in ("ps2", "ps4"):
        k = int(epi[2])
        cout = N // (k * k)
        BT, hin, win = fb.ps_geometry(M)
        outs["out"] = Out((BT, hin * k, win * k, cout))
        static["ps"] = (k, cout, hin, win)
        ref, bound = ps_shuffle(ref, BT, hin, win, k, cout), ps_shuffle(bound, BT, hin, win, k, cout)
    elif inplace:  # as the encoder's residual stream: res is the output
        outs["out"] = Out((M, n_out), ld=n_out + 16, init=kw["res"].half(), align=oa)
    else:
        outs["out"] = Out((M if rows is None else rows, n_out), ld=n_out + 16, align=oa)
        pad = 24 if align16 else 12  # column slices of wider buffers: row strides that are not N, the gaps poisoned
        for name in ("res", "res2"):
            if name in kw and not gated:
                ins[name] = H16(kw[name], ld=n_out + pad, align=oa)
            elif name in kw:
                ins[name] = H16(kw[name])

    def caller(fn):
        def call(i, o, ws):
            gk = dict(static, **{k: v for k, v in i.items() if k not in ("x", "w")})
            gk.update({k: v for k, v in o.items() if k != "out"})
            if inplace:
                gk["res"] = o["out"]
            fn(i["x"], i["w"], o["out"], gk)
        return call

    def check(o):
        worst = assert_elementwise(o["out"], ref, bound, what)
        assert rel(o["out"], ref) < BAR_GEMM, what
        if extra_check is not None:
            extra_check(o)
        return worst
    r = placed("gemm", caller(launch), ins, outs, check=check, what=what)
    if same_as is not None:
        outs2 = {k: v for k, v in outs.items() if k not in same_as_drop}
        r2 = run_placed(caller(same_as), ins, outs2, what=what + " (forced)", device=DEV, fills=("zero",))
        for k in outs2:
            assert same_bits(r["outputs"][k], r2["outputs"][k]), f"{what}: '{k}' is not what the kernel this case is about gives"
    return r


def tile_launch(T, cfg):
    def launch(x, w, out, gk):
        with T.route(**({} if cfg == "auto" else dict(force_tile=cfg))):
            T.gemm_kw(x, w, out, **gk)
    return launch


TILE_EPIS = ("bias", "gamma_res", "res_res2", "rowbias", "geglu", "swiglu", "ps2", "strided_x")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 6, 7, "auto"])
def test_gemm_tile_placed(cfg):
    """The one-tile-per-block kernels at (BM + 1, BN + 8, 40) (an M, an N and a K tail; BN + 32 / + 16 where the
    gated epilogues / the pixel-shuffle store need that granularity) and (1, smallest legal N, 8): bias, gamma +
    res in place and with res an operand of its own, res + res2 as strided slices with poisoned gaps, rowbias, GEGLU, SwiGLU, the x2 pixel-shuffle
    store, x as the middle third of a [M, 3 K] buffer; and the LayerNorm fold with [M, 2] (mean, rstd) and with
    three-part (sum, sum of squares) statistics at K = 72.  y, res and res2 of the row stores start 8 bytes past a
    256-byte boundary at one of the two shapes (vda.h: the one-tile kernels take them there) and 16 at the other."""
    T = tune_lib()
    BM, BN = TILES.get(cfg, (128, 128))
    launch = tile_launch(T, cfg)
    for epi in TILE_EPIS:
        g, small = {"geglu": (32, 32), "swiglu": (32, 32), "ps2": (16, 16)}.get(epi, (8, 4))
        for M, N, K in ((BM + 1, BN + g, 40), (1, small, 8)):
            c = sb.swiglu_case(M, N, K, seed=M + N + K) if epi == "swiglu" else fb.gemm_case(M, N, K, epi, seed=M + N + K)
            c.update(M=M, N=N, K=K)
            # row stores: y, res and res2 at an 8-byte base on the large shape, a 16-byte one on the small
            gemm_placed(c, launch, f"gemm cfg {cfg} {epi} {M}x{N}x{K}", align8=M > 1 and epi != "ps2")
            if epi == "gamma_res":
                gemm_placed(dict(c, inplace=False), launch, f"gemm cfg {cfg} gamma + separate res {M}x{N}x{K}", align8=M == 1)
    for kind in ("ln", "ln_parts"):
        c = fb.gemm_ln_case(BM + 1, BN + 8, 72, kind, seed=BN)
        gemm_placed(c, launch, f"gemm cfg {cfg} {kind} {BM + 1}x{BN + 8}x72")
    report("gemm", TALLY["gemm"])


def phased_launch(T, sched=3, drop=(), **knobs):
    """The automatic route on `sched` persistent blocks; with force_tile=4 the launch for gemm_placed(same_as=)."""
    def launch(x, w, out, gk):
        with T.route(gemm_sched=sched, **knobs):
            T.gemm_kw(x, w, out, **{k: v for k, v in gk.items() if k not in drop})
    return launch


@pytest.mark.parametrize("N", [264, 512])
@pytest.mark.parametrize("epi", ["bias", "gamma_res", "res_res2", "rowbias", "strided_x", "geglu", "swiglu", "ps2"])
def test_gemm_phased_placed(epi, N):
    """The phased 256x256 kernel (cfg 4, the automatic route) at M = 4097 (a one-row last M tile), K = 192, on 3
    persistent blocks: the register epilogue (bias), the staged one (gamma + res in place, res + res2 strided,
    GEGLU, SwiGLU, pixel shuffle), the row-bias instantiation; every output bit-identical to cfg 4 forced (the
    placed strides and bases still reach the phased kernel); N = 264 (an 8-column last N tile; the gated and
    pixel-shuffle epilogues need N % 32 / N % 16, so they run at N = 288) and 512."""
    T = tune_lib()
    M, K = 4097, 192
    if N == 264 and epi in ("geglu", "swiglu", "ps2"):
        N = 288
    c = sb.swiglu_case(M, N, K, seed=N) if epi == "swiglu" else fb.gemm_case(M, N, K, epi, seed=N + len(epi))
    c.update(M=M, N=N, K=K)
    if epi == "rowbias":
        c["kw"].update(rdiv=300)
    gemm_placed(c, phased_launch(T), f"gemm phased {epi} N={N}", staged=True, align16=True,
                same_as=phased_launch(T, force_tile=4))
    if epi == "gamma_res":
        gemm_placed(dict(c, inplace=False), phased_launch(T), f"gemm phased gamma + separate res N={N}", staged=True,
                    align16=True, same_as=phased_launch(T, force_tile=4))
    report("gemm", TALLY["gemm"])


def stats_check(M, parts):
    def check(o):
        sref, sbound = fb.row_stats_ref_bound(o["out"])
        assert_elementwise(o["stats_out"], sref, sbound, "stats_out")
    return check


@pytest.mark.parametrize("kind", ["ln", "ln_parts", "ln_geglu", "ln_rowbias", "ln_stats_out", "ln_drop"])
def test_gemm_phased_ln_fold_placed(kind):
    """The LayerNorm-fold epilogues of the phased kernel at (4097, 256, 192): [M, 2] and three-part statistics
    (exactly M entries: the last 16-byte piece ends at the poison), GEGLU, the EK 3 per-frame row bias, stats_out
    as a guarded output, drop_period = 300 (the output holds M - ceil(M / 300) rows)."""
    T = tune_lib()
    M, N, K = 4097, 256, 192
    c = fb.gemm_ln_case(M, N, K, kind, seed=N)
    ref, bound = fb.gemm_ref_bound(c["x"], c["w"], phi_table=True, **c["kw"])
    kwargs = {}
    if kind == "ln_drop":
        keep = torch.arange(M) % 300 != 0
        ref, bound = ref[keep], bound[keep]
        kwargs["rows"] = int(keep.sum())
        c["kw"]["drop_period"] = 300
    elif kind == "ln_stats_out":
        kwargs.update(extra_out=dict(stats_out=Out((M, N // 256, 2), torch.float32)), extra_check=stats_check(M, N // 256))
    drop = c["kw"].pop("drop_period", 0)

    def launch(x, w, out, gk):
        with T.route(gemm_sched=3):
            T.gemm_kw(x, w, out, drop_period=drop, **gk)
    if kind not in ("ln_drop", "ln_rowbias"):  # vda_gemm serves those two on this route alone, -22 anywhere else
        kwargs.update(same_as=phased_launch(T, force_tile=4, drop=("stats_out",)), same_as_drop=("stats_out",))
    gemm_placed(c, launch, f"gemm phased {kind}", ref_bound=(ref, bound), **kwargs)
    report("gemm", TALLY["gemm"])


def test_gemm_phased_res_stats_out_placed():
    """res + stats_out through the staged epilogue's own statistics (4097, 512, 128), the statistics a guarded
    output."""
    T = tune_lib()
    M, N, K = 4097, 512, 128
    c = fb.gemm_case(M, N, K, "gamma_res", seed=N)
    del c["kw"]["gamma"]
    c["epi"] = "res"
    gemm_placed(c, phased_launch(T), "gemm phased res + stats_out", staged=True, align16=True,
                extra_out=dict(stats_out=Out((M, N // 256, 2), torch.float32)), extra_check=stats_check(M, N // 256),
                same_as=phased_launch(T, force_tile=4))
    report("gemm", TALLY["gemm"])


def test_gemm_phased_512x128_placed():
    """cfg 5 (512x128, N = 128, M >= 8192) forced at M = 8193 (a one-row last tile), K = 64."""
    T = tune_lib()
    c = fb.gemm_case(8193, 128, 64, "bias", seed=3)
    gemm_placed(c, phased_launch(T, force_tile=5), "gemm cfg 5 8193x128x64")
    report("gemm", TALLY["gemm"])


def test_gemm_dynamic_schedule_placed():
    """ops.sched_counters' protocol with the counters placed.  gemm256_kernel draws tickets only when there are more
    tiles than blocks and the block count is a multiple of 8: (4097, 512, 192) is 17 x 2 = 34 tiles, run on
    gemm_sched = 8 persistent blocks, so every block takes its tiles beyond the first by ticket.  The output is inside
    the bound and bit-identical to the fixed-stride schedule of cfg 4 forced on the same 8 blocks without counters;
    the 16 counters are zero again afterwards and nothing around them is written."""
    T = tune_lib()
    M, N, K, blocks = 4097, 512, 192, 8
    ntiles = -(-M // 256) * -(-N // 256)
    assert ntiles > blocks and blocks % 8 == 0, "the launch would not take the ticket path"
    c = fb.gemm_case(M, N, K, "bias", seed=9)

    def counters_zero(o):
        assert int(o["sched"].abs().sum()) == 0, "the last block must leave the counters zero"
    gemm_placed(c, phased_launch(T, sched=blocks), "gemm phased dynamic schedule",
                extra_out=dict(sched=Out((16,), torch.int32, init=torch.zeros(16, dtype=torch.int32), sentinel=-7776)),
                extra_check=counters_zero, same_as=phased_launch(T, sched=blocks, force_tile=4, drop=("sched",)),
                same_as_drop=("sched",))
    report("gemm", TALLY["gemm"])


# =====================================================================================================
# vda_conv2d
# =====================================================================================================
def c_conv2d(L, x, w, out, ws, *, ks=3, stride=1, pad=1, pre_relu=False, act=0, bias=None, bias9=None, rowbias=None, rdiv=1,
             rmod=1, res=None, res2=None, res2_up=False, up=None):
    BT, H, W, Cin = x.shape
    Cout = w.shape[0]
    e = _lib.Epilogue(rdiv=rdiv, rmod=rmod, act=act)
    for name, t in (("bias", bias), ("bias9", bias9), ("rowbias", rowbias)):
        if t is not None:
            setattr(e, name, t.data_ptr())
    if res is not None:
        e.res, e.ldres = res.data_ptr(), Cout
    if res2 is not None:
        e.res2, e.ldres2 = res2.data_ptr(), Cout
        if res2_up:
            e.res2_h, e.res2_w = res2.shape[1], res2.shape[2]
    uh, uw = (0, 0) if up is None else up
    ok(L, L.vda_conv2d(x.data_ptr(), w.data_ptr(), out.data_ptr(), BT, H, W, Cin, Cout, ks, stride, pad, int(pre_relu), uh, uw,
                       ctypes.byref(e), ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                       stream()), "vda_conv2d")


def conv_placed(c, knobs, staged, what, want_ws=None, differs_from=None):
    """One fp16_bounds.conv_case on the route `knobs` select (tuning library), x / w / bias / res / res2 / rowbias
    placed, the workspace exactly vda_conv2d_workspace() bytes under those knobs.  want_ws: whether the route must
    ask for one (the test is then about it).  differs_from: knobs of ANOTHER kernel for the same conv (another
    accumulation order or other rounding points), whose zero-fill output must not have the same bits: where no
    predicate says which kernel the automatic route took, this is how the case knows it is not that fallback."""
    T = tune_lib()
    kw = c["kw"]
    ref, bound = fb.conv_ref_bound(c["x"], c["w"], staged=staged, **kw)
    ref, bound = nhwc(ref), nhwc(bound)
    x, w = nhwc(c["x"]), nhwc(c["w"])
    BT, Hh, Ww, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[1]
    ins = dict(x=H16(x), w=H16(w))
    static = dict(ks=ks, stride=kw["stride"], pad=kw["pad"], pre_relu=kw.get("pre_relu", False),
                  act=ACT_RELU if kw.get("relu_out") else 0, up=kw.get("up"), res2_up=kw.get("res2_up", False))
    if "bias" in kw:
        ins["bias"] = F32(kw["bias"])
    for name in ("res", "res2"):
        if name in kw:
            ins[name] = H16(nhwc(kw[name]))
    if "framebias" in kw:
        ins["rowbias"] = F32(kw["framebias"])
        static.update(rdiv=c["Ho"] * c["Wo"], rmod=kw["framebias"].shape[0])
    def ws_bytes(kn):
        with T.route(**kn):
            return int(T.lib.vda_conv2d_workspace(BT, Hh, Ww, Cin, Cout, ks, kw["stride"], kw["pad"]))
    wsb = ws_bytes(knobs)
    if want_ws is not None:
        assert (wsb > 0) == want_ws, f"{what}: vda_conv2d_workspace = {wsb}"

    def caller(kn):
        def call(i, o, ws):
            with T.route(**kn):
                c_conv2d(T.lib, i["x"], i["w"], o["out"], ws.get("ws"), **static, **{k: v for k, v in i.items() if k not in ("x", "w")})
        return call
    outs = dict(out=Out(tuple(ref.shape)))
    r = placed("conv", caller(knobs), ins, outs, {"ws": wsb} if wsb > 0 else None,
               check=bounded("out", ref, bound, what, BAR_GEMM), what=what)
    if differs_from is not None:
        wsb2 = ws_bytes(differs_from)
        r2 = run_placed(caller(differs_from), ins, outs, {"ws": wsb2} if wsb2 > 0 else None, what=what + " (other kernel)",
                        device=DEV, fills=("zero",))
        assert not same_bits(r["outputs"]["out"], r2["outputs"]["out"]), f"{what}: the bits of {differs_from}: not the route meant"
    return r


def bias_case(BT, Cin, Cout, Hh, Ww, relu, seed, up=None):
    c = fb.conv_case(BT, Cin, Cout, Hh, Ww, "rcu1", seed=seed, up=up)
    c["kw"].update(pre_relu=False, relu_out=relu)
    return c


@pytest.mark.parametrize("Hh,Ww", [(9, 33), (17, 95)])
def test_hconv_placed(Hh, Ww):
    """vda_hconv.hip forced, Cin = 64, two frames: one tile plus a row and a column, 3 x 3 ragged tiles; the
    pre-ReLU / ReLU pair (rcu1: a NaN halo would be squashed, +Inf is not) and bias + res + res2 (rcu2)."""
    for mode in ("rcu1", "rcu2"):
        conv_placed(fb.conv_case(2, 64, 256, Hh, Ww, mode, seed=Hh * Ww), dict(hconv=1), True, f"hconv {Hh}x{Ww} {mode}")
    report("conv", TALLY["conv"])


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("Hh,Ww", [(3, 129), (19, 19)])
def test_strip_placed(Hh, Ww, split):
    """vda_strip.hip (force_tile = -3), Cin = 128 (four 32-channel slabs), unsplit and with the input channels
    split over 2 and 4 work items: the fp32 slices live in a workspace of exactly vda_conv2d_workspace() bytes."""
    for mode in ("rcu1", "rcu2"):
        conv_placed(fb.conv_case(2, 128, 256, Hh, Ww, mode, seed=Hh * Ww), dict(force_tile=-3, strip_split=split), True,
                    f"strip {Hh}x{Ww} {mode} split {split}", want_ws=split > 1)
    report("conv", TALLY["conv"])


def test_halo_cout128_placed():
    """The 128-output halo conv (vda_oc1.hip) on the automatic route at 129 x 128 (a one-row last tile row), and
    with the bilinear resize fused into its patch staging, (8, 20) -> (33, 47).  The fused resize is asserted by the library's own predicate."""
    # no predicate is exported for the plain halo route and its bits equal the implicit GEMM's (the same K order,
    # measured), so neither can say which kernel ran; the shape restates vda_conv2d's own conditions for it
    BT, Cin, Cout, Hh, Ww = 2, 64, 128, 129, 128
    assert Cout == 128 and Cin % 64 == 0 and Hh * Ww >= 128 * 128
    conv_placed(bias_case(BT, Cin, Cout, Hh, Ww, True, 129), {}, False, "halo128 129x128")
    assert tune_lib().lib.vda_conv2d_bias9_ok(2, 8, 20, 64, 128, 33, 47) == 1  # vda_conv_halo_fused_serves
    conv_placed(bias_case(2, 64, 128, 8, 20, True, 55, up=(33, 47)), {}, False, "halo128 fused resize 8x20->33x47")
    report("conv", TALLY["conv"])


def test_implicit_gemm_conv_placed():
    """The implicit-GEMM conv (force_tile = -2) at 9 x 11: Cin = 8 (K = 72, a K tail) stride 1 with res + res2,
    Cin = 64 stride 2 with the pre-ReLU, and the per-frame rowbias (rmod = 3 over five frames)."""
    conv_placed(fb.conv_case(2, 8, 32, 9, 11, "rcu2", seed=1), dict(force_tile=-2), False, "implicit gemm 8->32")
    conv_placed(fb.conv_case(2, 64, 128, 9, 11, "rcu1", stride=2, seed=2), dict(force_tile=-2), False, "implicit gemm s2 64->128")
    c = fb.conv_case(5, 64, 128, 9, 11, "rcu2", seed=3)
    c["kw"]["framebias"] = fb.rnd32(3, 128, seed=7)
    conv_placed(c, dict(force_tile=-2), False, "implicit gemm rowbias")
    report("conv", TALLY["conv"])


def test_conv_reg_resize_placed():
    """up= through the register-staged conv (a tile forced), (8, 20) -> (33, 47), Cout = 32."""
    conv_placed(bias_case(2, 64, 32, 8, 20, True, 32, up=(33, 47)), dict(force_tile=0), False, "conv_reg resize")
    report("conv", TALLY["conv"])


def test_phased_conv_placed():
    """The phased 256x256 implicit-GEMM conv (M >= 4096) with the halo and strip routes off: two frames of 32 x 65
    (M = 4160, a ragged second M tile that ends at the last frame's row H)."""
    conv_placed(fb.conv_case(2, 64, 256, 32, 65, "rcu2", seed=5), dict(hconv=0, force_tile=-2), True, "phased conv 2x32x65",
                differs_from=dict(hconv=0, force_tile=3))  # the 256x256 one-tile kernel adds res and res2 in fp32
    report("conv", TALLY["conv"])


def test_im2col_route_placed():
    """The stride-2 explicit-im2col route (automatic), two frames of 91 x 93 -> 46 x 47 (M = 4324): the im2col
    matrix is a workspace of exactly vda_conv2d_workspace() bytes, every byte of which the gather must write."""
    c = fb.conv_case(2, 64, 256, 91, 93, "rcu2", stride=2, seed=91)
    conv_placed(c, {}, True, "im2col route 2x91x93", want_ws=True)  # the dense phased GEMM's staged residual adds
    report("conv", TALLY["conv"])


def test_hconv_res2_upsample_placed():
    """res2 read through the epilogue's bilinear upsample from (33, 34) to 65 x 67 on the automatic halo route."""
    c = fb.conv_case(2, 64, 256, 65, 67, "rcu2", seed=33, res2_src=(33, 34))
    assert tune_lib().lib.vda_conv2d_res2_upsample_ok(2, 65, 67, 64, 256, 3, 1, 1) == 1  # else vda_conv2d refuses the call
    conv_placed(c, {}, True, "hconv res2 upsampled from (33, 34)")
    report("conv", TALLY["conv"])


def stage_check(name, r, bars, what):
    def check(o):
        rE, where, rmax, lines = SL.evaluate(SL.map_from_nhwc(o[name]), r, bars.E, bars.max)
        assert not lines, f"{what}: {lines}"
        return max(rE, rmax)
    return check


@pytest.mark.parametrize("route", [2, 0], ids=["source", "parent"])
@pytest.mark.parametrize("BT,hh,ww", [(1, 17, 9), (2, 1, 2)])
def test_oc1_src_placed(BT, hh, ww, route):
    """output_conv1 at the source resolution of its x2 resize (vda_oc1_src.hip, vda_debug_oc1_src(2)) and on the
    parent route (0: the halo conv with the fused resize), both with the 9-class bias table: x, the composed weights
    and bias9 placed, the output framed; the stage bar of test_gpu_oc1_src.py."""
    T = tune_lib()
    c = Case3(BT, hh, ww)
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    wq, b9 = weights.compose_pointwise_conv3(c.w0, c.b0, c.w1, c.b1)
    what = f"oc1_src bias9 {BT}x{hh}x{ww} route {route}"

    def call(i, o, ws):
        assert T.lib.vda_debug_oc1_src(route) == 0
        try:
            c_conv2d(T.lib, i["x"], i["w"], o["out"], None, bias9=i["bias9"], up=(2 * hh, 2 * ww))
        finally:
            assert T.lib.vda_debug_oc1_src(1) == 0
    placed("conv", call, dict(x=H16(nhwc(c.x)), w=H16(wq), bias9=F32(b9)), dict(out=Out((BT, 2 * hh, 2 * ww, 128))),
           check=stage_check("out", r, bars, what), what=what)
    report("conv", TALLY["conv"])


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("BT,hh,ww", [(2, 1, 2), (3, 5, 7)])
def test_subpixel_conv_placed(BT, hh, ww, s):
    """vda_subpixel_conv: x, the phase-group weights and bias9 placed, the output framed, the corner im2col a
    workspace of exactly vda_subpixel_conv_workspace() bytes; the stage bar of test_gpu_head_linear.py."""
    L = lib()
    c = Case(s, BT, hh, ww)
    Cin, _, Cout = CHAINS[s]
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    wq, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, s)
    wsb = int(L.vda_subpixel_conv_workspace(BT, hh, ww, Cin, s))
    assert wsb > 0 and L.vda_subpixel_conv_check(BT, hh, ww, Cin, Cout, s) == 0
    what = f"subpixel s={s} {BT}x{hh}x{ww}"

    def call(i, o, ws):
        ok(L, L.vda_subpixel_conv(i["x"].data_ptr(), i["w"].data_ptr(), i["bias9"].data_ptr(), o["out"].data_ptr(), BT, hh, ww,
                                  Cin, Cout, s, ws["ws"].data_ptr(), wsb, stream()), what)
    placed("subpixel", call, dict(x=H16(nhwc(c.x).reshape(-1, Cin)), w=H16(wq.reshape(-1)), bias9=F32(b9)),
           dict(out=Out((BT, s * hh, s * ww, Cout))), {"ws": wsb}, check=stage_check("out", r, bars, what), what=what)
    report("subpixel", TALLY["subpixel"])


# =====================================================================================================
# Attention
# =====================================================================================================
@pytest.mark.parametrize("N", [1, 33, 129])
def test_spatial_attention_placed(N):
    """B = 2, H = 2: the last batch's last head's K / V record range ends at the poison; the first batch's
    query rows start after it."""
    T = tune_lib()
    B, Hd = 2, 2
    qkv = fb.rnd16(B * N, 3 * Hd * 64, seed=N)
    ref, bound = fb.spatial_attn_ref_bound(qkv, B, N, Hd)
    what = f"spatial attention N={N}"
    placed("attention", lambda i, o, ws: T.spatial_attention(i["qkv"], B, N, Hd, out=o["out"]), dict(qkv=H16(qkv)),
           dict(out=Out((B * N, Hd * 64))), check=bounded("out", ref, bound, what, BAR_ATTN), what=what)
    report("attention", TALLY["attention"])


BTS = [(1, 32, 37), (2, 5, 19), (1, 1, 8), (3, 17, 1)]  # test_gpu_vitg.py
# (D, H, attn knob): direct-load (D = 24; D = 64 / 136 / 192 by the knob), staged (D = 64), staged-192
TEMPORAL = [(24, 3, 0), (64, 4, 0), (64, 4, 1), (136, 2, 1), (192, 2, 0), (192, 2, 1)]


@pytest.mark.parametrize("rope", [0.0, 10000.0])
@pytest.mark.parametrize("D,Hd,knob", TEMPORAL)
def test_temporal_attention_placed(D, Hd, knob, rope):
    T = tune_lib()
    C = Hd * D
    for B, Tn, S in BTS:
        qkv = fb.rnd16(B * Tn * S, 3 * C, seed=D + Tn + S) * 2
        ref, bound = fb.temporal_attn_ref_bound(qkv, B, Tn, S, Hd, D, rope)
        what = f"temporal attention D={D} H={Hd} knob={knob} rope={rope} B={B} T={Tn} S={S}"

        def call(i, o, ws):
            with T.route(attn=knob):
                T.temporal_attention(i["qkv"], B, Tn, S, Hd, D, rope, out=o["out"])
        placed("attention", call, dict(qkv=H16(qkv)), dict(out=Out((B * Tn * S, C))),
               check=bounded("out", ref, bound, what, BAR_ATTN), what=what)
    report("attention", TALLY["attention"])


# =====================================================================================================
# Small ops
# =====================================================================================================
@pytest.mark.parametrize("C", [128, 520])
def test_layernorm_row_stats_placed(C):
    """The narrow (C = 128: four rows per wave) and the general kernel (C = 520: one lane of the second chunk) on
    five rows (the four stress rows among them) with ldx = C + 8: the gaps between rows are poison; row_stats on
    the same operand writes exactly [rows, 2]."""
    L = lib()
    X = fb.ln_rows(1, C)
    R = X.shape[0]
    g, b = fb.gn_affine(C, seed=C)
    ref, bound = fb.layernorm_ref_bound(X, g, b, 1e-6)
    sref, sbound = fb.ln_stats_ref_bound(X, 1e-6)
    ins = dict(x=H16(X, ld=C + 8), g=F32(g), b=F32(b))
    placed("small ops", lambda i, o, ws: ok(L, L.vda_layernorm(i["x"].data_ptr(), i["x"].stride(0), o["out"].data_ptr(),
                                                               i["g"].data_ptr(), i["b"].data_ptr(), R, C, 1e-6, 0, stream()), "ln"),
           ins, dict(out=Out((R, C))), check=bounded("out", ref, bound, f"layernorm C={C}", BAR_OP), what=f"layernorm C={C}")
    placed("small ops", lambda i, o, ws: ok(L, L.vda_row_stats(i["x"].data_ptr(), i["x"].stride(0), o["st"].data_ptr(), R, C, 1e-6,
                                                               stream()), "row_stats"),
           dict(x=H16(X, ld=C + 8)), dict(st=Out((R, 2), torch.float32)), check=bounded("st", sref, sbound, f"row_stats C={C}"),
           what=f"row_stats C={C}")
    report("small ops", TALLY["small ops"])


def test_layernorm_skip_period_placed():
    """skip_period = 2 over three frames (C = 256): the dropped rows hold 777, the last kept row is the operand's last."""
    L = lib()
    C, np_, BT = 256, 2, 3
    X = (fb.rnd16(BT * (np_ + 1), C, seed=C + np_) * 2 + 0.5).half().float()
    X[::np_ + 1] = 777.0
    g, b = fb.gn_affine(C, seed=C)
    keep = torch.arange(X.shape[0]) % (np_ + 1) != 0
    ref, bound = fb.layernorm_ref_bound(X[keep], g, b, 1e-6)
    placed("small ops", lambda i, o, ws: ok(L, L.vda_layernorm(i["x"].data_ptr(), i["x"].stride(0), o["out"].data_ptr(),
                                                               i["g"].data_ptr(), i["b"].data_ptr(), BT * np_, C, 1e-6, np_,
                                                               stream()), "ln skip"),
           dict(x=H16(X, ld=C + 8), g=F32(g), b=F32(b)), dict(out=Out((BT * np_, C))),
           check=bounded("out", ref, bound, "layernorm skip_period", BAR_OP), what="layernorm skip_period")
    report("small ops", TALLY["small ops"])


@pytest.mark.parametrize("with_ws", [True, False], ids=["workspace", "two-pass"])
@pytest.mark.parametrize("C,groups,S", [(64, 32, 129), (1024, 32, 33), (24, 4, 33)])
def test_groupnorm_placed(C, groups, S, with_ws):
    """Both routes, three frames (the middle one offset by +40): 2, 32 and 6 channels per group, a ragged second
    row chunk.  The workspace is exactly vda_groupnorm_workspace() floats."""
    L = lib()
    Fr = 3
    x = fb.gn_case(Fr, S, C)
    g, b = fb.gn_affine(C, seed=C)
    ref, bound = fb.groupnorm_ref_bound(x, g, b, groups, 1e-6)
    wsb = 4 * int(L.vda_groupnorm_workspace(Fr, S, C, groups))
    assert wsb > 0
    what = f"groupnorm C={C} groups={groups} S={S} {'workspace' if with_ws else 'two-pass'}"

    def call(i, o, ws):
        ok(L, L.vda_groupnorm(i["x"].data_ptr(), o["out"].data_ptr(), i["g"].data_ptr(), i["b"].data_ptr(), Fr, S, C, groups, 1e-6,
                              ws["ws"].data_ptr() if with_ws else None, stream()), what)
    placed("small ops", call, dict(x=H16(x.view(-1, C)), g=F32(g), b=F32(b)), dict(out=Out((Fr * S, C))),
           {"ws": wsb} if with_ws else None, check=bounded("out", ref.view(-1, C), bound.view(-1, C), what, BAR_OP), what=what)
    report("small ops", TALLY["small ops"])


@pytest.mark.parametrize("C,S,Fr", [(64, 5, 7), (256, 17, 15), (1024, 5, 7)])
def test_groupnorm_linear_placed(C, S, Fr):
    """The fused kernel (C = 64, 256: ragged 16-row tiles, a tile spans frames) and the GroupNorm + GEMM
    composition through the workspace (C = 1024, which then holds GN(x)); stats_out a guarded output."""
    L = lib()
    M = Fr * S
    x = fb.gn_case(Fr, S, C, seed=3)
    g, b = fb.gn_affine(C, seed=C)
    w, bias = fb.rnd16(C, C, scale=C ** -0.5, seed=C + 1), fb.rnd32(C, scale=0.1, seed=C + 2)
    fused = L.vda_groupnorm_linear_fused(C, 32, C) == 1
    assert fused == (C != 1024)
    ref, bound = fb.groupnorm_linear_ref_bound(x, g, b, 32, 1e-6, w, bias)
    wsb = int(L.vda_groupnorm_linear_workspace(Fr, S, C, 32, C))
    assert wsb > 0  # both routes keep the GroupNorm statistics there (the entry point refuses a NULL workspace)
    P = (C + 255) // 256
    what = f"groupnorm_linear C={C} S={S} F={Fr}"

    def call(i, o, ws):
        ok(L, L.vda_groupnorm_linear(i["x"].data_ptr(), i["g"].data_ptr(), i["b"].data_ptr(), Fr, S, C, 32, 1e-6, i["w"].data_ptr(),
                                     i["bias"].data_ptr(), o["out"].data_ptr(), C, o["st"].data_ptr(), ws["ws"].data_ptr(), wsb,
                                     stream()), what)

    def check(o):
        if fused:
            worst = assert_elementwise(o["out"], ref, bound, what)
            sref, sbound = fb.sums_ref_bound(o["out"])
            assert_elementwise(o["st"][:, 0], sref, sbound, what + " stats_out")
        else:  # the composition's own bar (test_gpu_ops.py test_groupnorm_linear)
            worst = rel(o["out"], ref) / BAR_OP
            assert worst < 1, what
            sref, sbound = fb.row_stats_ref_bound(o["out"])
            assert_elementwise(o["st"], sref, sbound, what + " stats_out")
        return worst
    placed("small ops", call, dict(x=H16(x.view(-1, C)), g=F32(g), b=F32(b), w=H16(w), bias=F32(bias)),
           dict(out=Out((M, C)), st=Out((M, P, 2), torch.float32)), {"ws": wsb}, check=check, what=what)
    report("small ops", TALLY["small ops"])


@pytest.mark.parametrize("BT,Hh,Ww,C,Ho,Wo", [(2, 4, 5, 8, 9, 11), (2, 19, 19, 32, 38, 38), (3, 3, 3, 8, 7, 5)])
def test_upsample_placed(BT, Hh, Ww, C, Ho, Wo):
    """A pair that straddles two frames, the exact x2 (every row pair shares its source rows) and an odd total row
    count (the last row has no partner: its would-be second source row is the poison after the operand)."""
    L = lib()
    x = fb.upsample_input(BT, Hh, Ww, C)
    ref, bound = fb.upsample_ref_bound(x, Ho, Wo)
    what = f"resize {BT}x{Hh}x{Ww}x{C} -> {Ho}x{Wo}"
    placed("small ops", lambda i, o, ws: ok(L, L.vda_upsample_bilinear(i["x"].data_ptr(), o["out"].data_ptr(), BT, Hh, Ww, C, Ho, Wo,
                                                                       stream()), what),
           dict(x=H16(x)), dict(out=Out((BT, Ho, Wo, C))), check=bounded("out", ref, bound, what, BAR_OP), what=what)
    report("small ops", TALLY["small ops"])


@pytest.mark.parametrize("W", [14, 14 * 14])
def test_patch_im2col_placed(W):
    """img at the 8-byte alignment vda.h gives it (not 16), three frames, Kp = 592: exact."""
    L = lib()
    BT, Kp = 3, 592
    img = fb.rnd32(BT, 3, 14, W, seed=W)
    ref = fb.patch_im2col_ref(img, Kp)

    def check(o):
        assert torch.equal(o["a"], ref), "patch_im2col is not the exact gather"
        return 0.0
    placed("small ops", lambda i, o, ws: ok(L, L.vda_patch_im2col(i["img"].data_ptr(), o["a"].data_ptr(), BT, 14, W, Kp, stream()),
                                            "patch_im2col"),
           dict(img=F32(img, align=8)), dict(a=Out(tuple(ref.shape))), check=check, what=f"patch_im2col W={W}")
    report("small ops", TALLY["small ops"])


# (C, Hin, Win, Ho, Wo, knobs, workspace expected): the fused depth conv, both sides of its staging boundary, the
# implicit-GEMM tail forced, the materialised resize (a downscale)
DEPTH = [(64, 8, 20, 33, 47, {}, False), (32, 22, 21, 33, 33, {}, False), (32, 22, 22, 33, 33, {}, True),
         (40, 9, 9, 15, 17, dict(force_tile=13), None), (64, 37, 37, 19, 19, {}, True)]


@pytest.mark.parametrize("C,Hin,Win,Ho,Wo,knobs,want_ws", DEPTH)
def test_depth_head_placed(C, Hin, Win, Ho, Wo, knobs, want_ws):
    T = tune_lib()
    BT = 2
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hin, Win, BT, seed=C)
    ref, bound = fb.depth_head_ref_bound(x, w1, b1, w2, b2, Ho, Wo)
    hi, lo = fb.split_hi_lo(w1.permute(0, 2, 3, 1).contiguous())
    with T.route(**knobs):
        wsb = int(T.lib.vda_depth_head_workspace(BT, Hin, Win, C, Ho, Wo))
    if want_ws is not None:
        assert (wsb > 0) == want_ws
    what = f"depth tail C={C} {Hin}x{Win}->{Ho}x{Wo} {knobs}"

    def call(i, o, ws):
        with T.route(**knobs):
            ok(T.lib, T.lib.vda_depth_head(i["x"].data_ptr(), i["w1"].data_ptr(), i["b1"].data_ptr(), i["w2"].data_ptr(),
                                           i["b2"].data_ptr(), o["out"].data_ptr(), ws["ws"].data_ptr() if wsb > 0 else None,
                                           BT, Hin, Win, C, Ho, Wo, stream()), what)
    placed("small ops", call, dict(x=H16(nhwc(x)), w1=H16(torch.cat([hi, lo], 0)), b1=F32(b1), w2=F32(w2), b2=F32(b2)),
           dict(out=Out((BT, Ho, Wo), torch.float32)), {"ws": wsb} if wsb > 0 else None,
           check=bounded("out", ref, bound, what), what=what)
    report("small ops", TALLY["small ops"])


# =====================================================================================================
# fp32 kernels (vda_f32.hip): float4 loads at N tails
# =====================================================================================================
def rnd(*s, scale=1.0, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float() * scale


def f32_check(name, ref, what):
    def check(o):
        r = rel(o[name], ref) / TOL_F32
        assert r < 1, f"{what}: rel-L1 {r * TOL_F32:.3e}"
        return r
    return check


def test_gemm_f32_placed():
    """M = 150, K = 24, I = 80 (N = 160 interleaved GEGLU rows; the output's 80 columns end inside a float4 group
    of a 64-column tile): strided x (ldx = 3 K) and out, gamma and a strided res."""
    L = lib()
    M, K, I = 150, 24, 80
    x, w, b = rnd(M, K, seed=1), rnd(2 * I, K, scale=K ** -0.5, seed=2), rnd(2 * I, scale=0.1, seed=3)
    gam, res = rnd(I, seed=4).abs() + 0.1, rnd(M, I, seed=5)
    hg = x.double() @ w.double().t() + b.double()
    ref = gam.double() * (hg[:, :I] * F.gelu(hg[:, I:])) + res.double()

    def call(i, o, ws):
        e = _lib.Epilogue(rdiv=1, rmod=1, act=ACT_GEGLU, bias=i["bias"].data_ptr(), gamma=i["gamma"].data_ptr(),
                          res=i["res"].data_ptr(), ldres=i["res"].stride(0))
        ok(L, L.vda_gemm_f32(i["x"].data_ptr(), i["x"].stride(0), i["w"].data_ptr(), o["out"].data_ptr(), o["out"].stride(0), M,
                             2 * I, K, ctypes.byref(e), stream()), "gemm_f32")
    placed("fp32", call, dict(x=F32(x, ld=3 * K), w=F32(_geglu_interleave(w)), bias=F32(_geglu_interleave(b)), gamma=F32(gam),
                              res=F32(res, ld=I + 8)), dict(out=Out((M, I), torch.float32, ld=I + 8)),
           check=f32_check("out", ref, "gemm_f32"), what="gemm_f32 GEGLU")
    report("fp32", TALLY["fp32"])


def test_conv_f32_placed():
    """3x3 conv, two frames of 9 x 11, Cin = 32, Cout = 48 (an N tail), bias + res + res2."""
    L = lib()
    BT, Cin, Hh, Ww, Cout = 2, 32, 9, 11, 48
    x, w, b = rnd(BT, Cin, Hh, Ww, seed=30), rnd(Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5, seed=31), rnd(Cout, scale=0.1, seed=32)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    r1, r2 = rnd(*ref.shape, seed=33), rnd(*ref.shape, seed=34)
    ref = ref + r1.double() + r2.double()

    def call(i, o, ws):
        e = _lib.Epilogue(rdiv=1, rmod=1, bias=i["bias"].data_ptr(), res=i["res"].data_ptr(), ldres=Cout, res2=i["res2"].data_ptr(),
                          ldres2=Cout)
        ok(L, L.vda_conv2d_f32(i["x"].data_ptr(), i["w"].data_ptr(), o["out"].data_ptr(), BT, Hh, Ww, Cin, Cout, 3, 1, 1, 0,
                               ctypes.byref(e), stream()), "conv_f32")
    placed("fp32", call, dict(x=F32(nhwc(x)), w=F32(nhwc(w)), bias=F32(b), res=F32(r1), res2=F32(r2)),
           dict(out=Out(tuple(ref.shape), torch.float32)), check=f32_check("out", ref, "conv_f32"), what="conv_f32")
    report("fp32", TALLY["fp32"])


def test_attention_f32_placed():
    """Spatial attention at N = 65 (one key past a 64-key block: the last batch's padding keys are the poison) and
    temporal attention at T = 3, S = 5, D = 24, H = 3 with RoPE."""
    L = lib()
    B, N, Hd, D = 2, 65, 2, 64
    qkv = rnd(B * N, 3 * Hd * D, seed=40)
    q, k, v = qkv.double().view(B, N, 3, Hd, D).permute(2, 0, 3, 1, 4)
    ref = (((q * D ** -0.5) @ k.transpose(-1, -2)).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * N, Hd * D)
    placed("fp32", lambda i, o, ws: ok(L, L.vda_spatial_attention_f32(i["qkv"].data_ptr(), o["out"].data_ptr(), B, N, Hd, D,
                                                                      _attn_scale(D), stream()), "spatial f32"),
           dict(qkv=F32(qkv)), dict(out=Out((B * N, Hd * D), torch.float32)), check=f32_check("out", ref, "spatial_attention_f32"),
           what="spatial_attention_f32")
    B, Tn, S, Hd, D = 2, 3, 5, 3, 24
    qkv = rnd(B * Tn * S, 3 * Hd * D, seed=61)
    ref, _ = fb.temporal_attn_ref_bound(qkv, B, Tn, S, Hd, D, 10000.0)
    placed("fp32", lambda i, o, ws: ok(L, L.vda_temporal_attention_f32(i["qkv"].data_ptr(), o["out"].data_ptr(), B, Tn, S, Hd, D,
                                                                       _attn_scale(D), 10000.0, stream()), "temporal f32"),
           dict(qkv=F32(qkv)), dict(out=Out((B * Tn * S, Hd * D), torch.float32)),
           check=f32_check("out", ref, "temporal_attention_f32"), what="temporal_attention_f32")
    report("fp32", TALLY["fp32"])


def test_norms_f32_placed():
    """LayerNorm at C = 72 on 3 rows with ldx = C + 8, GroupNorm on 2 frames of 7 sites at C = 64."""
    L = lib()
    C, R = 72, 3
    x, g, b = rnd(R, C, seed=80) * 2 + 0.5, rnd(C, seed=81) * 0.2 + 1, rnd(C, seed=82) * 0.2
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), eps=1e-6)
    placed("fp32", lambda i, o, ws: ok(L, L.vda_layernorm_f32(i["x"].data_ptr(), i["x"].stride(0), o["out"].data_ptr(),
                                                              i["g"].data_ptr(), i["b"].data_ptr(), R, C, 1e-6, 0, stream()), "ln f32"),
           dict(x=F32(x, ld=C + 8), g=F32(g), b=F32(b)), dict(out=Out((R, C), torch.float32)), check=f32_check("out", ref, "layernorm_f32"),
           what="layernorm_f32")
    Fr, S, C = 2, 7, 64
    x, g, b = rnd(Fr, S, C, seed=90) + 0.3, rnd(C, seed=91) * 0.2 + 1, rnd(C, seed=92) * 0.2
    ref = F.group_norm(x.double().permute(0, 2, 1), 32, g.double(), b.double(), eps=1e-6).permute(0, 2, 1).reshape(-1, C)
    placed("fp32", lambda i, o, ws: ok(L, L.vda_groupnorm_f32(i["x"].data_ptr(), o["out"].data_ptr(), i["g"].data_ptr(),
                                                              i["b"].data_ptr(), Fr, S, C, 32, 1e-6, stream()), "gn f32"),
           dict(x=F32(x.view(-1, C)), g=F32(g), b=F32(b)), dict(out=Out((Fr * S, C), torch.float32)),
           check=f32_check("out", ref, "groupnorm_f32"), what="groupnorm_f32")
    report("fp32", TALLY["fp32"])


def test_depth_head_f32_placed():
    """C = 64, (5, 40) -> (33, 47), two frames: the resized map and the 32-channel hidden map are workspaces of
    exactly [BT, Ho, Wo, C] and [BT Ho Wo, 32] floats."""
    L = lib()
    C, Hin, Win, Ho, Wo, BT = 64, 5, 40, 33, 47, 2
    x, w1, b1, w2, b2 = fb.depth_head_case(C, Hin, Win, BT, seed=C)
    x = rnd(BT, C, Hin, Win, seed=7)
    up = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    ref = F.relu(F.conv2d(F.relu(F.conv2d(up, w1.double(), b1.double(), padding=1)), w2.double().view(1, -1, 1, 1), b2.double()))[:, 0]

    def call(i, o, ws):
        ok(L, L.vda_depth_head_f32(i["x"].data_ptr(), i["w1"].data_ptr(), i["b1"].data_ptr(), i["w2"].data_ptr(), i["b2"].data_ptr(),
                                   o["out"].data_ptr(), ws["up"].data_ptr(), ws["mid"].data_ptr(), BT, Hin, Win, C, Ho, Wo, stream()),
           "depth_head_f32")
    placed("fp32", call, dict(x=F32(nhwc(x)), w1=F32(nhwc(w1)), b1=F32(b1), w2=F32(w2), b2=F32(b2)),
           dict(out=Out((BT, Ho, Wo), torch.float32)), dict(up=BT * Ho * Wo * C * 4, mid=BT * Ho * Wo * 32 * 4),
           check=f32_check("out", ref, "depth_head_f32"), what="depth_head_f32")
    report("fp32", TALLY["fp32"])
