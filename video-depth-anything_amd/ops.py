"""Tensor-level API of the libvda kernels: thin keyword wrappers over ``torch.ops.vda.*``.

The operators are native: ``csrc/vda_torch.cpp`` registers them with ``TORCH_LIBRARY(vda, m)``
(CUDA = HIP and Meta keys) in ``libvda_torch.so``, which validates device / dtype / layout,
allocates outputs and workspaces through the PyTorch caching allocator and launches through the C
ABI of ``include/vda.h`` on the current HIP stream (so whole forwards can be captured in a HIP
graph).  Activations are fp16 NHWC / token-major; biases, scales and norm affines fp32.  There is
deliberately no CPU path: an op on a CPU tensor, or without the native libraries, raises.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_GELU, ACT_GEGLU, ACT_RELU, ACT_SWIGLU, STORE_ROWS, STORE_PIXEL_SHUFFLE  # noqa: F401

Tensor = torch.Tensor


# Optional per-launch timing of tagged launches (bench.py's roofline leg).  When a tag is enabled,
# the launch is bracketed by two events on the launch stream; nothing else changes.
_PROBE: Optional[dict] = None


def enable_probe(tags):
    global _PROBE
    _PROBE = {t: [] for t in tags}


def take_probe():
    """Return {tag: [(ms, flop) per launch]} for the probed launches (synchronises) and disable
    probing; flop = 2*M*N*K of that launch."""
    global _PROBE
    out = {}
    if _PROBE:
        torch.cuda.synchronize()
        out = {t: [(a.elapsed_time(b), fl) for a, b, fl in ev] for t, ev in _PROBE.items()}
    _PROBE = None
    return out


def _vda():
    """torch.ops.vda, loading libvda_torch.so (TORCH_LIBRARY over libvda's C ABI) on first use.
    Raises VDAUnavailable when the native libraries are missing: there is no fallback."""
    return _lib.torch_ops()


def _need(t: Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"vda op: {name} must be a GPU tensor (no CPU path in the product)")
    if t.dtype != dtype:
        raise RuntimeError(f"vda op: {name} must be {dtype}, got {t.dtype}")


def gemm(x: Tensor, w: Tensor, *, bias=None, rowbias=None, rdiv=1, rmod=1, gamma=None, res=None,
         res2=None, act=ACT_NONE, ln_stats=None, ln_colsum=None, ln_parts=0, ln_eps=1e-6, stats_out=None,
         sched=None, drop_period=0, out: Optional[Tensor] = None, tag: Optional[str] = None) -> Tensor:
    """out[M, N'] = epi(x[M, K] @ w[N, K]^T); N' = N (N/2 for GEGLU / SwiGLU). x may be a row-strided view.
    fp16 x/w -> vda_gemm; fp32 x/w -> vda_gemm_f32 (fp32 mode).  torch.ops.vda.gemm[.out].
    ``ln_stats`` + ``ln_colsum`` fold a LayerNorm of x into the GEMM (vda.h): ln_stats is either
    ``row_stats(x)`` ([M, 2] (mean, rstd), ln_parts=0) or the [M, P, 2] partial sums another GEMM wrote
    through ``stats_out`` while producing x (ln_parts=P, ln_eps the LayerNorm eps).  ``stats_out``
    ([M, ceil(N/256), 2] fp32) receives this GEMM's per-row partial (sum, sumsq) of its output.
    ``sched`` (int32 [>= 9], zeroed once; see ``sched_counters``) lets the persistent 256x256 GEMM take its
    tiles by atomic ticket; one counter set per stream (vda.h vda_epilogue.sched).  ``drop_period`` = P > 0:
    x is frames of P token rows, the first the cls token; the output leaves those rows out
    ([M - ceil(M / P), N'], the LN-folded projects GEMM on an encoder tap, vda.h drop_period)."""
    _need(x, x.dtype, "x")
    probe = _PROBE is not None and tag in _PROBE
    if probe:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    v = _vda()
    if out is None:
        out = v.gemm(x, w, bias, rowbias, int(rdiv), int(rmod), gamma, res, res2, int(act), ln_stats, ln_colsum,
                     int(ln_parts), float(ln_eps), stats_out, sched, int(drop_period))
    else:
        v.gemm.out(x, w, bias, rowbias, int(rdiv), int(rmod), gamma, res, res2, int(act), ln_stats, ln_colsum,
                   int(ln_parts), float(ln_eps), stats_out, sched, int(drop_period), out=out)
    if probe:
        ev1.record()
        _PROBE[tag].append((ev0, ev1, 2.0 * x.shape[0] * w.shape[0] * x.shape[1]))
    return out


@functools.lru_cache(maxsize=None)
def gemm_accepts(M: int, N: int, K: int, *, bias=True, ln_fold=False, ln_parts=0, rowbias=False, rdiv=1, rmod=1,
                 drop_period=0, act=ACT_NONE, res=False, stats_out=False, ldx=None, ldy=None) -> bool:
    """Whether ``gemm`` of contiguous, 16-byte aligned fp16 x [M, K] (row stride ``ldx``, default K) and
    w [N, K] with these epilogue features is accepted: the library's own argument and route checks
    (vda.h vda_gemm_check), no launch.  ``bias`` / ``ln_fold`` / ``rowbias`` / ``res`` / ``stats_out`` say
    which tensors the call would pass.  For callers that choose between a fused epilogue (``drop_period``,
    LN fold + ``rowbias``) and separate ops.  Memoised per argument tuple: a steady-state forward asks the
    library nothing."""
    ptr = lambda on: 0x1000 if on else None  # noqa: E731  (only null-ness and alignment are looked at)
    ny = N // 2 if act in (ACT_GEGLU, ACT_SWIGLU) else N
    e = _lib.Epilogue(bias=ptr(bias), rowbias=ptr(rowbias), rdiv=int(rdiv), rmod=int(rmod), res=ptr(res), ldres=ny,
                      act=int(act), ln_stats=ptr(ln_fold), ln_colsum=ptr(ln_fold), ln_parts=int(ln_parts),
                      stats_out=ptr(stats_out), drop_period=int(drop_period))
    return _lib.lib().vda_gemm_check(int(K if ldx is None else ldx), int(ny if ldy is None else ldy), int(M), int(N),
                                     int(K), e) == 0


_SCHED = {}


def sched_counters(device=None) -> Tensor:
    """The tile-scheduler counters (int32 [16], zero) of the current stream on `device`: one set per
    stream, so that GEMMs on different streams never share one (vda_epilogue.sched).  The kernels leave
    them zero after every launch."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = torch.cuda.current_stream(dev)
    key = (dev.index, st.cuda_stream)
    t = _SCHED.get(key)
    if t is None:
        t = torch.zeros(16, dtype=torch.int32, device=dev)
        _SCHED[key] = t
    return t


def conv_transpose_ks(x: Tensor, w: Tensor, bias: Tensor, BT: int, h: int, w_: int, k: int) -> Tensor:
    """ConvTranspose2d(kernel = stride = k) as one GEMM with a pixel-shuffle store.
    x [BT*h*w, Cin]; w [k*k*Cout, Cin] packed (i, j, co); bias [k*k*Cout] fp32 -> [BT, h*k, w*k, Cout]."""
    _need(x, x.dtype, "x")
    return _vda().conv_transpose_ks(x, w, bias, int(BT), int(h), int(w_), int(k))


def subpixel_conv(x: Tensor, w: Tensor, bias9: Tensor, BT: int, h: int, w_: int, s: int) -> Tensor:
    """ConvTranspose2d(kernel = stride = s) then a zero-padded 3x3 conv as ONE sub-pixel conv of the low-resolution
    map (vda.h vda_subpixel_conv): x [BT*h*w, Cin] fp16; w the composed phase-group weights and bias9 [9, Cout]
    fp32 of ``weights.compose_subpixel`` -> [BT, s*h, s*w, Cout].  The map between the two convs is never written."""
    _need(x, torch.float16, "x")
    return _vda().subpixel_conv(x, w, bias9, int(BT), int(h), int(w_), int(s))


@functools.lru_cache(maxsize=None)
def subpixel_conv_accepts(BT: int, h: int, w_: int, Cin: int, Cout: int, s: int) -> bool:
    """Whether ``subpixel_conv`` serves this shape (vda.h vda_subpixel_conv_check: Cout 256, Cin % 64 == 0, s in
    {2, 4}, buffers below 2 GiB), no launch.  Memoised per shape."""
    return _lib.lib().vda_subpixel_conv_check(int(BT), int(h), int(w_), int(Cin), int(Cout), int(s)) == 0


@functools.lru_cache(maxsize=None)
def conv2d_bias9_accepts(BT: int, H: int, W: int, Cin: int, Cout: int, up) -> bool:
    """Whether the 3x3 ``conv2d`` of [BT, H, W, Cin] through ``up=(Hu, Wu)`` takes a ``bias9`` table
    (vda.h vda_conv2d_bias9_ok), no launch.  Memoised per shape."""
    return _lib.lib().vda_conv2d_bias9_ok(int(BT), int(H), int(W), int(Cin), int(Cout), int(up[0]), int(up[1])) == 1


def conv2d(x: Tensor, w: Tensor, *, ks=3, stride=1, pad=1, bias=None, pre_relu=False, act=ACT_NONE,
           res=None, res2=None, up=None, bias9=None) -> Tensor:
    """NHWC conv.  x [BT, H, W, Cin] fp16; w [Cout, ks, ks, Cin] fp16 -> [BT, Ho, Wo, Cout].
    `up=(Hu, Wu)` reads x through a bilinear align_corners=True resize to (Hu, Wu) first.
    `bias9` [9, Cout] fp32 replaces `bias` by a per-class table over the output map's outer ring (the bias of
    a 1x1 conv composed into this one, vda.h vda_epilogue.bias9; where ``conv2d_bias9_accepts``).
    The strip conv's split workspace comes from the caching allocator per call (no shared state)."""
    _need(x, x.dtype, "x")
    return _vda().conv2d(x, w, int(ks), int(stride), int(pad), bias, bool(pre_relu), int(act), res, res2,
                         None if up is None else [int(up[0]), int(up[1])], bias9)


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, *, skip_period: int = 0,
              rows: Optional[int] = None) -> Tensor:
    """Row LayerNorm of x [R, C] (row-strided ok).  skip_period=np drops each frame's cls row."""
    _need(x, x.dtype, "x")
    return _vda().layernorm(x, gamma, beta, float(eps), int(skip_period), rows)


def row_stats(x: Tensor, eps: float) -> Tensor:
    """Per-row LayerNorm statistics of x [R, C] fp16: [round_up(R, 2), 2] fp32 (mean, rstd)."""
    _need(x, torch.float16, "x")
    return _vda().row_stats(x, float(eps))


def groupnorm(x: Tensor, gamma: Tensor, beta: Tensor, frames: int, groups: int, eps: float) -> Tensor:
    """GroupNorm on NHWC frames: x [F*S, C] -> same."""
    _need(x, x.dtype, "x")
    return _vda().groupnorm(x, gamma, beta, int(frames), int(groups), float(eps))


def groupnorm_linear(x: Tensor, gamma: Tensor, beta: Tensor, frames: int, groups: int, eps: float, w: Tensor, *,
                     bias=None, stats_out=None) -> Tensor:
    """GroupNorm on NHWC frames then Linear: x [F*S, C] -> GN(x) @ w[N, C]^T + bias, [F*S, N]
    (motion_module.py:116-119, norm + proj_in).  fp16: one fused kernel for groups 32, N = C in
    {64, 128, 256} (vda.h vda_groupnorm_linear), else GroupNorm + GEMM through a workspace; ``stats_out``
    ([F*S, 1, 2] fp32) receives the per-row (sum, sumsq) of the output for a following LN-folded GEMM."""
    _need(x, x.dtype, "x")
    return _vda().groupnorm_linear(x, gamma, beta, int(frames), int(groups), float(eps), w, bias, stats_out)


def spatial_attention(qkv: Tensor, B: int, N: int, H: int, D: int = 64) -> Tensor:
    _need(qkv, qkv.dtype, "qkv")
    return _vda().spatial_attention(qkv, int(B), int(N), int(H), int(D))


def temporal_attention(qkv: Tensor, B: int, T: int, S: int, H: int, D: int, rope_theta: float = 0.0) -> Tensor:
    """Softmax attention over the T frames of every site; ``rope_theta`` > 0 rotates q and k first
    (pe='rope', attention.py:403-429: pairs (2i, 2i+1) of all H*D channels, angle t * theta^(-2i/C))."""
    _need(qkv, qkv.dtype, "qkv")
    return _vda().temporal_attention(qkv, int(B), int(T), int(S), int(H), int(D), float(rope_theta))


def upsample_bilinear(x: Tensor, Ho: int, Wo: int) -> Tensor:
    _need(x, x.dtype, "x")
    return _vda().upsample_bilinear(x, int(Ho), int(Wo))


def patch_im2col(img: Tensor, Kp: int, dtype=torch.float16) -> Tensor:
    """images [BT, 3, H, W] fp32 -> im2col rows [BT*(1+np), Kp] of ``dtype`` (fp16, or fp32 for fp32 mode)."""
    _need(img, torch.float32, "img")
    return _vda().patch_im2col(img, int(Kp), dtype)


def depth_head(x: Tensor, w1_split: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, Ho: int, Wo: int) -> Tensor:
    """Depth tail: bilinear resize to (Ho, Wo), 3x3 conv (split-fp16 fp32 weights) -> ReLU -> 1x1 -> ReLU.
    x [BT, H, W, C] fp16; w1_split [64, 3, 3, C] fp16 (hi rows 0..31, lo rows 32..63) -> depth [BT, Ho, Wo] fp32.
    The resize workspace is allocated only for shapes the fused depth conv does not serve."""
    _need(x, torch.float16, "x")
    return _vda().depth_head(x, w1_split, b1, w2, b2, int(Ho), int(Wo))


def depth_head_f32(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, Ho: int, Wo: int) -> Tensor:
    """fp32-mode depth tail: x [BT, H, W, C] fp32; w1 [32, 3, 3, C] fp32 -> depth [BT, Ho, Wo] fp32."""
    _need(x, torch.float32, "x")
    return _vda().depth_head(x, w1, b1, w2, b2, int(Ho), int(Wo))


def preprocess_frames(frames: Tensor, H: int, W: int, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)) -> Tensor:
    """uint8 frames [N, h, w, 3] (GPU) -> normalised network input [N, 3, H, W] fp32 (bicubic resize)."""
    _need(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be [N, h, w, 3] uint8, got {tuple(frames.shape)}")
    return _vda().preprocess_frames(frames, int(H), int(W), [float(v) for v in mean], [float(v) for v in std])


def depth_resize(depth: Tensor, ho: int, wo: int) -> Tensor:
    """depth [N, H, W] fp32 (GPU) -> [N, ho, wo] fp32, bilinear align_corners=True."""
    _need(depth, torch.float32, "depth")
    return _vda().depth_resize(depth, int(ho), int(wo))


def scale_shift(pred: Tensor, target: Tensor, *, mask: Optional[Tensor] = None):
    """Least-squares (scale, shift) of pred onto target (same number of elements, fp32, GPU; ``mask``
    uint8 or None = all ones) -> (ss [2] fp32, sums [5] fp64 = a_00, a_01, a_11, b_0, b_1), both on the
    device.  fp64 sums in a fixed order: deterministic, no host sync (vda.h vda_scale_shift)."""
    _need(pred, torch.float32, "pred")
    _need(target, torch.float32, "target")
    if pred.numel() != target.numel() or pred.numel() < 1:
        raise ValueError(f"pred and target need the same, non-zero number of elements, got {pred.numel()} and {target.numel()}")
    if mask is not None:
        _need(mask, torch.uint8, "mask")
        if mask.numel() != pred.numel():
            raise ValueError(f"mask has {mask.numel()} elements, pred {pred.numel()}")
    return _vda().scale_shift(pred, target, mask)


def depth_align(src: Tensor, ho: int, wo: int, *, ss: Optional[Tensor] = None, clip: bool = True,
                pre: Optional[Tensor] = None, w_pre=None, w_post=None, out: Optional[Tensor] = None) -> Tensor:
    """src [F, H, W] fp32 (GPU, F <= 32) -> [F, ho, wo]: bilinear align_corners=True resize (the bits
    of ``depth_resize``), then ``* ss[0] + ss[1]`` (``ss`` a device [2] tensor, two roundings; None =
    identity), then clip at 0, then with ``pre`` [F, ho, wo] the blend ``pre * w_pre[f] + v * w_post[f]``
    (F Python floats each).  ``out`` may be ``pre`` (in place).  One pass (vda.h vda_depth_align)."""
    _need(src, torch.float32, "src")
    if src.dim() != 3 or not 1 <= src.shape[0] <= 32:
        raise ValueError(f"src must be [F, H, W] with 1 <= F <= 32, got {tuple(src.shape)}")
    if ss is not None:
        _need(ss, torch.float32, "ss")
    if pre is not None:
        _need(pre, torch.float32, "pre")
        if w_pre is None or w_post is None or len(w_pre) != src.shape[0] or len(w_post) != src.shape[0]:
            raise ValueError("a blend (pre) needs one weight per frame in w_pre and in w_post")
        w_pre, w_post = [float(v) for v in w_pre], [float(v) for v in w_post]
    else:
        w_pre = w_post = None
    if out is not None:
        _need(out, torch.float32, "out")
    return _vda().depth_align(src, int(ho), int(wo), ss, bool(clip), pre, w_pre, w_post, out)


def _eval_inputs(pred: Tensor, gt: Tensor, valid: Optional[Tensor]):
    """Checks shared by the evaluation ops; returns ``valid`` as uint8 (a bool mask is viewed, not copied)."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 GPU tensor (no CPU path in the product)")
    if pred.dim() < 1 or pred.numel() < 1 or not 1 <= pred.shape[0] <= 65535:
        raise ValueError(f"pred must be a non-empty [F, ...] tensor with 1 <= F <= 65535, got {tuple(pred.shape)}")
    if gt.shape != pred.shape or gt.device != pred.device:
        raise ValueError(f"gt must have pred's shape and device, got {tuple(gt.shape)} on {gt.device}")
    if not pred.is_contiguous() or not gt.is_contiguous():
        raise ValueError("pred and gt must be contiguous")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError("valid must be a bool or uint8 tensor")
        if valid.shape != pred.shape or valid.device != pred.device or not valid.is_contiguous():
            raise ValueError(f"valid must be contiguous with pred's shape and device, got {tuple(valid.shape)} on {valid.device}")
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
    return valid


def depth_eval_fit(pred: Tensor, gt: Tensor, valid: Optional[Tensor] = None, *, per_frame: bool = False):
    """Masked least squares in inverse depth (the fit of the reference's ``align_prediction``): pred / gt
    [F, ...] fp32 on the GPU, ``valid`` bool / uint8 of the same shape or None (all valid) -> (ss [G, 2] fp32
    = (scale, shift), sums [G, 5] fp64), G = F with ``per_frame`` and 1 otherwise, both on the device.  A fit
    without a solution gives (inf, 0).  fp64 sums in a fixed order, no host sync (vda.h vda_depth_eval_fit)."""
    valid = _eval_inputs(pred, gt, valid)
    return _vda().depth_eval_fit(pred, gt, valid, bool(per_frame))


def depth_eval_metrics(pred: Tensor, gt: Tensor, valid: Optional[Tensor], ss: Tensor, *, max_depth: float = 80.,
                       want_aligned: bool = False):
    """Align with ``ss`` ([2] / [1, 2], or [F, 2] per frame; fp32 on the device), clip, invert and clip at
    ``max_depth`` as ``align_prediction`` does, and sum the metric terms over the valid pixels in the same
    pass -> (frame_sums [F, 8] fp64, total [8] fp64, aligned metric depth with pred's shape or None).  The
    sums: count, outliers at 1.25 / 1.25^2 / 1.25^3, S d/g, S |d|, S |d|/g, S d^2
    (vda.h vda_depth_eval_metrics)."""
    valid = _eval_inputs(pred, gt, valid)
    if not isinstance(ss, torch.Tensor) or ss.dtype != torch.float32 or ss.device != pred.device:
        raise ValueError("ss must be a float32 tensor on pred's device")
    F = pred.shape[0]
    if not (ss.numel() == 2 or tuple(ss.shape) == (F, 2)) or not ss.is_contiguous():
        raise ValueError(f"ss must be contiguous [2], [1, 2] or [F, 2] = (scale, shift), got {tuple(ss.shape)}")
    if not float(max_depth) > 0.:
        raise ValueError(f"max_depth must be greater than 0, got {max_depth}")
    return _vda().depth_eval_metrics(pred, gt, valid, ss, float(max_depth), bool(want_aligned))


CLOUD_LAYOUTS = {"split": _lib.CLOUD_SPLIT, "packed": _lib.CLOUD_PACKED}


def _cloud_inputs(depth: Tensor, valid: Optional[Tensor], step: int, trunc: float):
    """Checks shared by the point-cloud ops; returns ``valid`` as uint8 (a bool mask is viewed, not copied)."""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype != torch.float32:
        raise ValueError("depth must be a float32 GPU tensor (no CPU path in the product)")
    if depth.dim() != 3 or depth.numel() < 1 or not depth.is_contiguous() or depth.shape[0] > 65535:
        raise ValueError(f"depth must be contiguous, non-empty [F, H, W] with F <= 65535, got {tuple(depth.shape)}")
    if int(step) != step or int(step) < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    if float(trunc) != float(torch.tensor(float(trunc), dtype=torch.float32)):
        raise ValueError(f"trunc must be exactly representable in float32, got {trunc!r}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError("valid must be a bool or uint8 tensor")
        if valid.shape != depth.shape or valid.device != depth.device or not valid.is_contiguous():
            raise ValueError(f"valid must be contiguous with depth's shape and device, got {tuple(valid.shape)} on {valid.device}")
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
    return valid


def cloud_count(depth: Tensor, valid: Optional[Tensor] = None, *, step: int = 1, trunc: float):
    """Count the points ``cloud_write`` will produce: depth [F, H, W] fp32 on the GPU, ``valid`` bool / uint8 of
    the same shape or None -> (frame_offsets [F + 1] int64 on the device, the exclusive prefix of the frames'
    counts with the total last, and ws, the workspace that carries the block offsets to ``cloud_write``).  A
    candidate (every ``step``-th row and column) is kept when it is valid and ``0 < depth < trunc``.  No host
    sync (vda.h vda_cloud_count)."""
    valid = _cloud_inputs(depth, valid, step, trunc)
    return _vda().cloud_count(depth, valid, int(step), float(trunc))


def cloud_write(depth: Tensor, valid: Optional[Tensor], rgb: Optional[Tensor], K: Tensor, M: Optional[Tensor], *,
                step: int = 1, trunc: float, ws: Tensor, n: int, layout="split"):
    """Unproject and compact the kept candidates of ``cloud_count``'s operands (the same depth, valid, step and
    trunc, and its ws) in candidate order: ``K`` [F, 4] fp32 = (fx, fy, cx, cy), ``M`` [F, 3, 4] fp32
    camera-to-output or None, ``rgb`` [F, H, W, 3] uint8 or None, ``n`` the number of points to store (the total
    ``frame_offsets[-1]``, or fewer: only the first ``n`` are written).  ``layout="split"`` -> (points [n, 3]
    fp32, colors [n, 3] uint8 or None); ``"packed"`` -> (the records of a binary PLY body, [n * 12] or [n * 15]
    uint8, None) (vda.h vda_cloud_write)."""
    valid = _cloud_inputs(depth, valid, step, trunc)
    F, H, W = depth.shape
    if rgb is not None:
        if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.device != depth.device \
                or tuple(rgb.shape) != (F, H, W, 3) or not rgb.is_contiguous():
            raise ValueError("rgb must be a contiguous uint8 [F, H, W, 3] tensor on depth's device")
    for name, t, shape in (("K", K, (F, 4)), ("M", M, (F, 3, 4))):
        if t is None and name == "M":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != depth.device \
                or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor on depth's device")
    code = CLOUD_LAYOUTS.get(layout, layout) if isinstance(layout, str) else int(layout)
    if code not in CLOUD_LAYOUTS.values():
        raise ValueError(f"layout must be one of {sorted(CLOUD_LAYOUTS)}, got {layout!r}")
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or ws.device != depth.device:
        raise ValueError("ws must be the uint8 workspace cloud_count returned")
    if int(n) != n or int(n) < 0:
        raise ValueError(f"n must be a non-negative integer, got {n!r}")
    return _vda().cloud_write(depth, valid, rgb, K, M, int(step), float(trunc), code, ws, int(n))


VIS_LAYOUTS = {"index": _lib.VIS_INDEX, "hwc": _lib.VIS_HWC, "planar444": _lib.VIS_PLANAR444,
               "planar420": _lib.VIS_PLANAR420}


def depth_range(depth: Tensor) -> Tensor:
    """(min, max) of a contiguous fp32 GPU tensor -> [2] fp32 on the device, NaNs skipped, no host sync
    (vda.h vda_depth_range)."""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype != torch.float32:
        raise ValueError("depth must be a float32 GPU tensor (no CPU path in the product)")
    if depth.numel() < 1 or not depth.is_contiguous():
        raise ValueError(f"depth must be contiguous and non-empty, got {tuple(depth.shape)}")
    return _vda().depth_range(depth)


def depth_colorize(depth: Tensor, range: Tensor, *, lut: Optional[Tensor] = None, layout="hwc") -> Tensor:
    """depth [F, H, W] fp32 (GPU) -> uint8: the index ``uint8((d - range[0]) / (range[1] - range[0]) * 255)``
    of every pixel in fp32, then ``lut[index]`` (``lut`` [256, 3] uint8 on the device) in ``layout``:
    ``"index"`` [F, H, W] (no lut), ``"hwc"`` [F, H, W, 3], ``"planar444"`` [F, 3, H, W] or ``"planar420"``
    [F, H*W + 2*ch*cw] (a name or the VDA_VIS_* code).  ``range`` is a device [2] tensor, e.g. ``depth_range``
    of the whole video (vda.h vda_depth_colorize)."""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype != torch.float32:
        raise ValueError("depth must be a float32 GPU tensor (no CPU path in the product)")
    if depth.dim() != 3 or depth.numel() < 1 or not depth.is_contiguous() or depth.shape[0] > 65535:
        raise ValueError(f"depth must be contiguous, non-empty [F, H, W] with F <= 65535, got {tuple(depth.shape)}")
    if not isinstance(range, torch.Tensor) or range.dtype != torch.float32 or range.device != depth.device \
            or range.numel() != 2 or not range.is_contiguous():
        raise ValueError("range must be a contiguous float32 [2] tensor (min, max) on depth's device")
    code = VIS_LAYOUTS.get(layout, layout) if isinstance(layout, str) else int(layout)
    if code not in VIS_LAYOUTS.values():
        raise ValueError(f"layout must be one of {sorted(VIS_LAYOUTS)}, got {layout!r}")
    if lut is None:
        if code != _lib.VIS_INDEX:
            raise ValueError("every layout but 'index' needs a lut")
    else:
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.device != depth.device \
                or tuple(lut.shape) != (256, 3) or not lut.is_contiguous():
            raise ValueError("lut must be a contiguous uint8 [256, 3] tensor on depth's device")
    return _vda().depth_colorize(depth, range, lut, code)


TILE_KINDS = {"rgb": _lib.TILE_RGB, "depth": _lib.TILE_DEPTH, "error": _lib.TILE_ERROR, "xt": _lib.TILE_XT}


def depth_absdiff_range(a: Tensor, b: Tensor, valid: Optional[Tensor] = None) -> Tensor:
    """(min, max) of ``valid ? |b - a| : 0`` over two contiguous fp32 GPU tensors of one shape (a = pred,
    b = gt; ``valid`` bool / uint8 or None) -> [2] fp32 on the device, NaNs skipped, no host sync
    (vda.h vda_depth_absdiff_range)."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 GPU tensor (no CPU path in the product)")
    if a.numel() < 1 or not a.is_contiguous() or not b.is_contiguous() or b.shape != a.shape or b.device != a.device:
        raise ValueError(f"a and b must be contiguous, non-empty, of one shape and device, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError("valid must be a bool or uint8 tensor")
        if valid.shape != a.shape or valid.device != a.device or not valid.is_contiguous():
            raise ValueError(f"valid must be contiguous with a's shape and device, got {tuple(valid.shape)} on {valid.device}")
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
    return _vda().depth_absdiff_range(a, b, valid)


def panel_compose(tiles, rows: int, cols: int, F: int, t0: int, N: int, xstar: int, *, lut0: Optional[Tensor] = None,
                  lut1: Optional[Tensor] = None, layout="hwc") -> Tensor:
    """The canvas frames t0 .. t0 + F - 1 of a comparison video of N frames: ``rows x cols`` tiles of H x W
    pixels -> uint8 ``"hwc"`` [F, rows*H, cols*W, 3], ``"planar444"`` [F, 3, rows*H, cols*W] or ``"planar420"``
    [F, CH*CW + 2*ch*cw].  ``tiles``: up to 12 dicts ``kind`` ("rgb" / "depth" / "error" / "xt" or the
    VDA_TILE_* code), ``row``, ``col``, ``a`` (uint8 [n, H, W, 3] for "rgb", float32 [n, H, W] otherwise) and,
    optional, ``offset`` (canvas frame t shows source frame t - offset), ``lut`` (0 / 1), ``b`` and ``valid``
    (an error tile's gt and mask), ``range`` (device [2]; every kind but "rgb").  GPU tensors only
    (vda.h vda_panel_compose)."""
    if not isinstance(tiles, (list, tuple)) or not 1 <= len(tiles) <= 12:
        raise ValueError("tiles must be a list of 1 to 12 tile dicts")
    code = VIS_LAYOUTS.get(layout, layout) if isinstance(layout, str) else int(layout)
    if code not in (_lib.VIS_HWC, _lib.VIS_PLANAR444, _lib.VIS_PLANAR420):
        raise ValueError(f"layout must be one of ['hwc', 'planar420', 'planar444'], got {layout!r}")
    rows, cols, F, t0, N, xstar = int(rows), int(cols), int(F), int(t0), int(N), int(xstar)
    if not (1 <= rows <= 4 and 1 <= cols <= 3):
        raise ValueError(f"the grid must be 1..4 rows by 1..3 columns, got {rows} x {cols}")
    if not (1 <= F <= 65535 and t0 >= 0 and t0 + F <= N):
        raise ValueError(f"need 1 <= F <= 65535 and 0 <= t0, t0 + F <= N, got F={F}, t0={t0}, N={N}")
    dev, H, W, cells = None, None, None, set()
    a, b, valid, rng, kind, row, col, offset, lut = [], [], [], [], [], [], [], [], []
    for t in tiles:
        k = TILE_KINDS.get(t["kind"], t["kind"]) if isinstance(t["kind"], str) else int(t["kind"])
        if k not in TILE_KINDS.values():
            raise ValueError(f"tile kind must be one of {sorted(TILE_KINDS)}, got {t['kind']!r}")
        src = t["a"]
        want = torch.uint8 if k == _lib.TILE_RGB else torch.float32
        if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != want or not src.is_contiguous():
            raise ValueError(f"a tile source must be a contiguous {want} GPU tensor (no CPU path in the product)")
        if src.dim() != (4 if k == _lib.TILE_RGB else 3) or src.numel() < 1 or (k == _lib.TILE_RGB and src.shape[3] != 3):
            raise ValueError(f"a tile source must be [n, H, W] ([n, H, W, 3] for rgb), got {tuple(src.shape)}")
        if dev is None:
            dev, H, W = src.device, int(src.shape[1]), int(src.shape[2])
        if src.device != dev or tuple(src.shape[1:3]) != (H, W):
            raise ValueError(f"every tile must be {H} x {W} on {dev}, got {tuple(src.shape)} on {src.device}")
        r, c = int(t["row"]), int(t["col"])
        if not (0 <= r < rows and 0 <= c < cols) or (r, c) in cells:
            raise ValueError(f"tile cell ({r}, {c}) lies outside the {rows} x {cols} grid or is taken")
        cells.add((r, c))
        o, l = int(t.get("offset", 0)), int(t.get("lut", 0))
        if o < 0 or l not in (0, 1):
            raise ValueError(f"a tile needs offset >= 0 and lut 0 or 1, got {o} and {l}")
        tb, tv, tr = t.get("b"), t.get("valid"), t.get("range")
        if k == _lib.TILE_ERROR:
            tv = _eval_inputs(src, tb, tv)
        else:
            tb = tv = None
        if k != _lib.TILE_RGB:
            if not isinstance(tr, torch.Tensor) or tr.dtype != torch.float32 or tr.device != dev or tr.numel() != 2 \
                    or not tr.is_contiguous():
                raise ValueError("a tile's range must be a contiguous float32 [2] tensor (min, max) on its device")
            if (lut0 if l == 0 else lut1) is None:
                raise ValueError(f"a tile names lut{l}, which is missing")
        else:
            tr = None
        for lst, v in zip((a, b, valid, rng, kind, row, col, offset, lut), (src, tb, tv, tr, k, r, c, o, l)):
            lst.append(v)
    if not 0 <= xstar < W:
        raise ValueError(f"xstar must lie in 0..{W - 1}, got {xstar}")
    for l in (lut0, lut1):
        if l is not None and (not isinstance(l, torch.Tensor) or l.dtype != torch.uint8 or l.device != dev
                              or tuple(l.shape) != (256, 3) or not l.is_contiguous()):
            raise ValueError("a lut must be a contiguous uint8 [256, 3] tensor on the tiles' device")
    return _vda().panel_compose(a, b, valid, rng, kind, row, col, offset, lut, rows, cols, H, W, F, t0, N, xstar,
                                lut0, lut1, code)


YUV_CHROMA = {"420": _lib.YUV_420, "422": _lib.YUV_422, "444": _lib.YUV_444, "mono": _lib.YUV_MONO}


def _yuv_inputs(payload: Tensor, h: int, w: int, chroma):
    if not isinstance(payload, torch.Tensor) or not payload.is_cuda or payload.dtype != torch.uint8:
        raise ValueError("payload must be a uint8 GPU tensor (no CPU path in the product)")
    code = YUV_CHROMA.get(chroma, chroma) if isinstance(chroma, str) else int(chroma)
    if code not in YUV_CHROMA.values():
        raise ValueError(f"chroma must be one of {sorted(YUV_CHROMA)}, got {chroma!r}")
    if payload.dim() != 2 or (payload.shape[1] > 1 and payload.stride(1) != 1) or payload.shape[0] > 65535:
        raise ValueError(f"payload must be [N, frame_stride] with unit-stride rows and N <= 65535, got "
                         f"{tuple(payload.shape)}")
    return int(h), int(w), code


def yuv_to_rgb(payload: Tensor, h: int, w: int, chroma) -> Tensor:
    """Planar YUV frames ``payload`` [N, frame_stride] uint8 (GPU; Y, U, V planes of an h x w frame per row, as a
    .y4m file holds them, any base alignment) -> RGB uint8 [N, h, w, 3], the bits of ``video_io.read_y4m``.
    ``chroma``: "420", "422", "444", "mono" or the VDA_YUV_* code (vda.h vda_yuv_to_rgb)."""
    h, w, code = _yuv_inputs(payload, h, w, chroma)
    return _vda().yuv_to_rgb(payload, h, w, code)


@functools.lru_cache(maxsize=None)
def yuv_downscale_accepts(h: int, w: int, h2: int, w2: int) -> bool:
    """Whether ``yuv_downscale`` serves h x w -> h2 x w2 (vda.h vda_yuv_downscale_ok: at most 29 coefficients
    per axis, a ratio up to 7).  Memoised per shape."""
    return _lib.lib().vda_yuv_downscale_ok(int(h), int(w), int(h2), int(w2)) == 1


@functools.lru_cache(maxsize=None)
def _downscale_tables(h: int, w: int, h2: int, w2: int, device: str):
    """(kx, bx, ky, by) of ``decode.resample_tables`` on ``device``: built and uploaded once per shape and device."""
    from .decode import resample_tables
    tables = tuple(t.to(device) for t in resample_tables(w, w2) + resample_tables(h, h2))
    torch.cuda.current_stream(device).synchronize()  # later calls may run on other streams: the upload has landed
    return tables


def yuv_downscale(payload: Tensor, h: int, w: int, chroma, h2: int, w2: int) -> Tensor:
    """Planar YUV frames (as ``yuv_to_rgb`` takes them) -> RGB uint8 [N, h2, w2, 3]: the decoded frames resized as
    Pillow's ``Image.resize((w2, h2), Image.BICUBIC)`` does (``video_io._resize_rgb``, the ``--max_res`` step),
    bit for bit, without the full-size RGB frames in memory (vda.h vda_yuv_downscale).  Raises for a ratio
    ``yuv_downscale_accepts`` refuses."""
    h, w, code = _yuv_inputs(payload, h, w, chroma)
    kx, bx, ky, by = _downscale_tables(h, w, int(h2), int(w2), str(payload.device))
    return _vda().yuv_downscale(payload, h, w, code, int(h2), int(w2), kx, bx, ky, by)


def preprocess_yuv(payload: Tensor, h: int, w: int, chroma, H: int, W: int, mean=(0.485, 0.456, 0.406),
                   std=(0.229, 0.224, 0.225)) -> Tensor:
    """Planar YUV frames (as ``yuv_to_rgb`` takes them) -> normalised network input [N, 3, H, W] fp32:
    ``preprocess_frames(yuv_to_rgb(payload, ...), H, W)`` bit for bit, without the RGB frames in memory unless
    the downscale is too strong for the tile kernel (vda.h vda_preprocess_yuv)."""
    h, w, code = _yuv_inputs(payload, h, w, chroma)
    return _vda().preprocess_yuv(payload, h, w, code, int(H), int(W), [float(v) for v in mean], [float(v) for v in std])
