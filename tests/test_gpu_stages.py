"""Each stage of the clip forward on the GPU against the oracle's stage, slice by slice (tests/stagelib.py).

Every test feeds ONE stage of ``VideoDepthAnything`` (``_encode``, ``_reassemble``, ``_temporal``,
``_fusion`` + ``ops.upsample_bilinear``, ``_head``) the oracle's input of that stage rounded to fp16, and
holds every slice of every output -- each (frame, ring class) of a map, each (frame, first / last / other
tokens) of a token matrix, each (frame, 64-channel block) -- to ``E <= 4 x max_s E(O16(all), s)`` and the
whole output to ``max|y - r| <= 4 x max|O16(all) - r|``; fp32 mode to ``E <= 1e-5`` per slice.  The bars
come from the reference alone (stagelib.Bars).  The model is built from ``stagelib.round_weights`` weights,
so kernels and reference multiply by the same numbers.

Shapes: the smallest at which the glue can still be wrong.
* ViT-S, B = 2, T = 3, 42 x 70 (3 x 5 patches, ntok 16, layer_4 2 x 3): every stage, fp16 and fp32 mode;
  the head also with skip_tmp_block and with ``sel``.
* ViT-S, B = 1, T = 32, 28 x 42: the motion modules and the head at the last row of the PE table.
* ViT-S use_bn + use_clstoken, B = 2, T = 2, 42 x 70: encoder with cls rows, readout row bias, folded BatchNorm.
* ViT-S pe='rope', B = 2, T = 5, 42 x 70: the four motion modules.
* Streaming, T = 8, 42 x 70: ``forward_single_image``'s index glue + ``_head`` on the oracle's maps (the
  new frame's ``_reassemble`` is replaced by the oracle's maps, so nothing compounds), pred_depth_idx
  [0, 5, 2] and [0, -3, 2] against ``head_from_layers(sel=...)`` as ``StreamEngine.predict`` calls it.
* Fold routes, ViT-L motion modules (C = 1024, 1024, 256, 256) at B = 1, T = 16 and B = 2, T = 8 with
  S = 16 x 16 (M = 4096 in frames of 256 rows; inputs: fp16 normal deviates, the modules normalise them):
  the LN-folded q/k/v route (asserted taken), LayerNorm + GEMM (``ops.gemm_accepts`` refusing), and
  ``fold_ff_norm``.
* Fold routes, ViT-L encoder at 11 x 210 x 350 (15 x 25 patches, 4,136 rows, the smallest odd non-square
  clip ``_tap_fold`` accepts, asserted): ``fold_tap_norm`` on (output = projects(norm(tap)), against the
  oracle's projects.i conv on its tap) and off.

CPU oracle time of the whole file, measured on the MI355X machine at 16 threads: 17.9 s, of which the ViT-L
encoder reference is 13.4 s (r in float64 and O16(all) in fp32 each run once through all 24 blocks at 4,136
rows and are shared by both routes), the eight ViT-L motion-module references 3.0 s, everything ViT-S 1.5 s.
GPU time per test: 0.1 .. 0.3 s after the first call of a model (the whole file ran in 26 s).  The ViT-L
encoder case is much longer than test_forward_matches_oracle's ViT-L case (< 1 s: 846 rows, fp32 only), but
O16 cannot be cut down to the tap outputs for it: the first GPU run showed that the rounding which matters
there is the fp16 residual stream, which has to be followed through all blocks (below).

Measured on MI355X (first run of these tests), worst over the outputs and slices of each stage:
``E / bar`` and ``max|y - r| / bar`` for fp16 (0.25 would be O16(all) itself), ``E / 1e-5`` for fp32 mode.

    case                          stage                       E/bar        max/bar      fp32 E/1e-5
    ViT-S 2x3x42x70               encode                      0.25         0.25         0.09
                                  reassemble                  0.25         0.25         0.09
                                  mm0..3                      0.30..0.34   0.30..0.35   0.02..0.08
                                  fus4..1                     0.27..0.30   0.26..0.40   0.02
                                  head (+ skip, sel)          0.14..0.29   0.20..0.40   0.06..0.09
    ViT-S 1x32x28x42              mm0..3, head                0.23..0.35   0.27..0.41
    ViT-S bn+cls 2x2x42x70        encode (cls rows)           0.30         0.26         0.19
                                  reassemble (readout)        0.21         0.25         0.10
                                  fus4..1 (folded BN)         0.26..0.29   0.24..0.30   0.02
    ViT-S rope 2x5x42x70          mm0..3                      0.30..0.32   0.29..0.37   0.02..0.08
    streaming T=8                 index glue + head           0.20         0.19
    ViT-L mm0..3, M=4096, S=256   LN-folded q/k/v             0.34..0.36   0.35..0.42
                                  LayerNorm + GEMM            0.33..0.36   0.35..0.40
                                  fold_ff_norm                0.34..0.36   0.35..0.42
    ViT-L encoder 11x210x350      tap-norm fold (projected)   0.25         0.26
                                  LayerNorm taps              0.26         0.28

One healthy stage exceeded its bar on that run: the ViT-L encoder's LayerNorm taps passed every slice E
(0.50 .. 0.69 of the bar) but max|y - r| was 1.14x / 1.05x / 1.24x the bar on taps 1..3, growing with depth.
The kernels keep the residual stream in fp16 (documented: DESIGN.md, test_forward_massive_residual_channels);
O16 as first written did not.  With every tensor add of ``encoder_taps`` rounded as well (stagelib
``_RoundedAdds``, used for the encoder stage's O16(all) only) O16 gives E 1.48e-3 and max 1.66e-2 on the last
tap, against the GPU's 1.52e-3 and 1.69e-2: that rounding is the whole difference.  The factor 4 and the
slices are unchanged.

The negative streaming index exposed a fault in ``forward_single_image`` (a negative index handed to
``index_select`` on the context maps); it is fixed and test_streaming_head[idx0,-3,2] is its regression.
"""
import functools
import json
import os
import time

import pytest
import torch

import stagelib as L
import vda_amd
from helpers import GOLDEN, recipe_state_dict
from vda_amd import ops
from vda_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
ORACLE_SECONDS = [0.0]


def timed(fn):
    """lru_cache'd oracle work, its CPU time added to ORACLE_SECONDS."""
    @functools.lru_cache(maxsize=None)
    def wrapper(*a):
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        t0 = time.perf_counter()
        out = fn(*a)
        ORACLE_SECONDS[0] += time.perf_counter() - t0
        print(f"oracle {fn.__name__}{a}: {time.perf_counter() - t0:.1f} s (file total {ORACLE_SECONDS[0]:.1f} s)")
        return out
    return wrapper


VARIANTS = {"vits": {}, "vitl": {}, "bn_cls": dict(use_bn=True, use_clstoken=True), "rope": dict(pe="rope")}


@functools.lru_cache(maxsize=None)
def weights(variant):
    if variant in ("vits", "vitl"):
        return L.round_weights(recipe_state_dict(variant))
    with open(os.path.join(GOLDEN, f"state_dict_keys_vits_{variant}.json")) as f:
        return L.round_weights(synthetic_state_dict([(k, tuple(s)) for k, s in json.load(f)]))


@functools.lru_cache(maxsize=None)
def model(variant):
    enc = variant if variant in ("vits", "vitl") else "vits"
    return vda_amd.build_model(enc, weights(variant), device="cuda", **VARIANTS[variant])


CLIPS = {"A": ("vits", 2, 3, 42, 70, 31), "T32": ("vits", 1, 32, 28, 42, 32), "bn_cls": ("bn_cls", 2, 2, 42, 70, 33),
         "rope": ("rope", 2, 5, 42, 70, 34), "stream": ("vits", 1, 8, 42, 70, 35)}


@timed
def clip(name):
    variant, B, T, H, W, seed = CLIPS[name]
    g = torch.Generator().manual_seed(seed)
    return L.Clip(weights(variant), "vits", torch.randn(B, T, 3, H, W, generator=g))


@timed
def reference(name, stage, skip=False, sel=None, sel12=None):
    """(r, bars) of a stage of a clip: computed once, shared by the fp16 and fp32 tests, never modified."""
    return clip(name).bars(stage, skip_tmp_block=skip, sel=None if sel is None else list(sel),
                           sel12=None if sel12 is None else list(sel12))


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gpu_stage(m, c, stage, fp32=False, skip=False, sel=None):
    """One stage of the model on the clip's oracle input of that stage -> {output name: oracle layout, CPU}."""
    P = m._pack(dev(), fp32)
    dt = P.dt
    if stage == "encode":
        feats, cls, projected = m._encode(P, c.x.float().cuda())
        assert not projected
        out = {f"tap{i}": L.tokens_from_rows(f, c.BT) for i, f in enumerate(feats)}
        if c.readout:
            out.update({f"cls{i}": L.tokens_from_rows(t, c.BT) for i, t in enumerate(cls)})
        return out
    if stage == "reassemble":
        feats = [L.tokens_to_rows(f, dt) for f in c.feats]
        cls = [t.to(dt).cuda() for t in c.cls] if c.readout else None
        lay = m._reassemble(P, (feats, cls, False), c.BT, c.ph, c.pw)
        return {f"layer{i + 1}": L.map_from_nhwc(l) for i, l in enumerate(lay)}
    if stage.startswith("mm"):
        x = c.inner[stage]
        h, w = x.shape[2:]
        y = m._temporal(P.mm[int(stage[2:])], L.map_to_rows(x, dt), c.B, c.T, h * w)
        return {stage: L.map_from_rows(y, c.BT, h, w)}
    if stage.startswith("fus"):
        xs, size = c.inner[stage]
        x0 = L.map_to_nhwc(xs[0], dt)
        x1 = L.map_to_nhwc(xs[1], dt) if len(xs) == 2 else None
        y, _ = m._fusion(P.ref[int(stage[3:])], x0, x1, None)
        Ho, Wo = size if size is not None else (2 * y.shape[1], 2 * y.shape[2])
        return {stage: L.map_from_nhwc(ops.upsample_bilinear(y, Ho, Wo))}
    if stage == "head":
        l1, l2, l3, l4 = (L.map_to_nhwc(l, dt) for l in c.layers)
        if sel is not None:
            it = torch.tensor(list(sel), device=l1.device)
            l1, l2 = l1.index_select(0, it), l2.index_select(0, it)
        d = m._head(P, l1, l2, l3, l4, c.B, c.T, c.ph, c.pw, skip, sel=None if sel is None else list(sel))
        return {"depth": d.detach().to("cpu", torch.float64).reshape(-1, 1, 14 * c.ph, 14 * c.pw)}
    raise KeyError(stage)


def hold(what, y, r, bars, fp32=False):
    assert set(y) == set(r)
    fails = []
    for k in sorted(r):
        try:
            if fp32:
                L.check_fp32(f"{what}/{k}", y[k], r[k])
            else:
                L.check_fp16(f"{what}/{k}", y[k], r[k], bars[k])
        except L.StageFailure as e:
            fails.append(str(e))
    if fails:
        raise L.StageFailure("\n".join(fails))


@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("stage", L.STAGES)
def test_vits_every_stage(stage, fp32):
    """ViT-S, B = 2, T = 3, 42 x 70: both patch counts odd, every resize off the 2x grid, two batches."""
    r, bars = reference("A", stage)
    hold(f"vits 2x3x42x70 {stage}", gpu_stage(model("vits"), clip("A"), stage, fp32), r, bars, fp32)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("skip,sel", [(True, None), (False, (1, 3, 5)), (True, (0, 5))], ids=["skip", "sel", "skip+sel"])
def test_vits_head_variants(skip, sel, fp32):
    r, bars = reference("A", "head", skip, sel)
    hold(f"vits 2x3x42x70 head skip={skip} sel={sel}", gpu_stage(model("vits"), clip("A"), "head", fp32, skip, sel),
         r, bars, fp32)


@pytest.mark.parametrize("stage", ["mm0", "mm1", "mm2", "mm3", "head"])
def test_vits_t32_last_pe_row(stage):
    r, bars = reference("T32", stage)
    hold(f"vits 1x32x28x42 {stage}", gpu_stage(model("vits"), clip("T32"), stage), r, bars)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("stage", ["encode", "reassemble", "fus4", "fus3", "fus2", "fus1"])
def test_bn_clstoken_stages(stage, fp32):
    r, bars = reference("bn_cls", stage)
    hold(f"vits bn+cls 2x2x42x70 {stage}", gpu_stage(model("bn_cls"), clip("bn_cls"), stage, fp32), r, bars, fp32)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("stage", ["mm0", "mm1", "mm2", "mm3"])
def test_rope_motion_modules(stage, fp32):
    r, bars = reference("rope", stage)
    hold(f"vits rope 2x5x42x70 {stage}", gpu_stage(model("rope"), clip("rope"), stage, fp32), r, bars, fp32)


@pytest.mark.parametrize("pred", [(0, 5, 2), (0, -3, 2)], ids=["idx0,5,2", "idx0,-3,2"])
def test_streaming_head(pred, monkeypatch):
    """forward_single_image's glue (context index_select, cat with the new frame, ``sel``) + ``_head`` on the
    oracle's maps.  A negative index names frame i + (T - 1) of the context but frame i + T of path_3, as
    in the reference and in ``StreamEngine.predict``."""
    c, m, T = clip("stream"), model("vits"), 8
    sel = [i % T for i in pred] + [T - 1]
    sel12 = [i % (T - 1) for i in pred] + [T - 1]
    r, bars = reference("stream", "head", False, tuple(sel), tuple(sel12))
    lay = [L.map_to_nhwc(l) for l in c.layers]
    monkeypatch.setattr(m, "_reassemble", lambda P, enc, BT, ph, pw: [l[T - 1:] for l in lay])
    d, new = m.forward_single_image(c.x[T - 1:].float().cuda()[None], tuple(l[:T - 1] for l in lay), list(pred), T)
    assert d.shape == (1, 4, 42, 70) and all(torch.equal(a, b[T - 1:]) for a, b in zip(new, lay))
    hold(f"vits stream T=8 pred={pred} head", {"depth": d.detach().to("cpu", torch.float64).reshape(-1, 1, 42, 70)}, r, bars)


# ---------------------------------------------------------------------------------------------
# fold routes (ViT-L widths)
# ---------------------------------------------------------------------------------------------
@timed
def vitl_mm_reference(k, B, T):
    sd = weights("vitl")
    C = sd[f"head.motion_modules.{k}.temporal_transformer.proj_in.weight"].shape[0]
    g = torch.Generator().manual_seed(40 + k)
    x = L.r16(torch.randn(B * T, C, 16, 16, generator=g, dtype=torch.float64))
    pre = f"head.motion_modules.{k}."
    keys = {n: v for n, v in sd.items() if n.startswith(pre)}
    sd64 = L.cast(keys, torch.float64)
    r = L.run(lambda: L.O.temporal_module(sd64, pre, x, T))
    o = L.run(lambda: L.O.temporal_module(keys, pre, x.float(), T), "all")
    return x, r, L.Bars(o, r)


@pytest.mark.parametrize("route", ["qkv_fold", "layernorm_gemm", "ff_fold"])
@pytest.mark.parametrize("B,T", [(1, 16), (2, 8)])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_vitl_motion_module_fold_routes(k, B, T, route, monkeypatch):
    m = model("vitl")
    P = m._pack(dev(), False)
    q, S = P.mm[k], 256
    assert q.C == (1024, 1024, 256, 256)[k]
    assert m._qkv_fold(q, B * T * S, S, T) == [True, True]
    if route == "layernorm_gemm":
        monkeypatch.setattr(ops, "gemm_accepts", lambda *a, **kw: False)
        assert m._qkv_fold(q, B * T * S, S, T) == [False, False]
    x, r, bars = vitl_mm_reference(k, B, T)
    m.fold_ff_norm = route == "ff_fold"
    try:
        assert not m.fold_ff_norm or q.fffold
        y = m._temporal(q, L.map_to_rows(x), B, T, S)
    finally:
        m.fold_ff_norm = False
    hold(f"vitl mm{k} {B}x{T}x16x16 {route}", {"mm": L.map_from_rows(y, B * T, 16, 16)}, {"mm": r}, {"mm": bars})


VITL_ENC = (11, 210, 350)


@timed
def vitl_encoder_reference():
    BT, H, W = VITL_ENC
    sd = {k: v for k, v in weights("vitl").items() if k.startswith("pretrained.") or k.startswith("head.projects.")}
    sd64 = L.cast(sd, torch.float64)
    g = torch.Generator().manual_seed(50)
    x = L.r16(torch.randn(BT, 3, H, W, generator=g, dtype=torch.float64))
    ph, pw = H // 14, W // 14

    def both(s, xx):
        taps = L.O.encoder_taps(s, "vitl", xx)
        return taps, L.project_taps(s, taps, ph, pw)
    r_taps, r_proj = L.run(lambda: both(sd64, x))
    o_taps, o_proj = L.run(lambda: both(sd, x.float()), "all", True)  # with the fp16 residual stream
    return (x, {f"tap{i}": t for i, t in enumerate(r_taps)}, {f"tap{i}": L.Bars(o, t) for i, (o, t) in enumerate(zip(o_taps, r_taps))},
            {f"tap{i}": t for i, t in enumerate(r_proj)}, {f"tap{i}": L.Bars(o, t) for i, (o, t) in enumerate(zip(o_proj, r_proj))})


@pytest.mark.parametrize("fold", [True, False], ids=["tap_fold", "layernorm"])
def test_vitl_encoder_tap_fold_routes(fold):
    m = model("vitl")
    P = m._pack(dev(), False)
    BT, H, W = VITL_ENC
    ntok = (H // 14) * (W // 14) + 1
    assert m._tap_fold(P, BT, ntok) and not m._tap_fold(P, BT - 1, ntok)
    x, r_taps, b_taps, r_proj, b_proj = vitl_encoder_reference()
    m.fold_tap_norm = fold
    try:
        feats, cls, projected = m._encode(P, x.float().cuda())
    finally:
        m.fold_tap_norm = True
    assert projected == fold and cls is None
    y = {f"tap{i}": L.tokens_from_rows(f, BT) for i, f in enumerate(feats)}
    if fold:
        hold(f"vitl encode {BT}x{H}x{W} tap fold (projected)", y, r_proj, b_proj)
    else:
        hold(f"vitl encode {BT}x{H}x{W} LayerNorm taps", y, r_taps, b_taps)
