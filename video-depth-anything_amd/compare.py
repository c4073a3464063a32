"""Ground-truth comparison video of one scene: the reference's ``calculate_metrics.py:174-258`` with
``utils/vis_util.py: visualise_data``, without the matplotlib figure.

The reference compares the temporal stability of several predictions of one scene (the batch run, the streaming
``--process_single_image`` run) against ground truth: it aligns each method on its first frame, logs an
absolute and a squared error per method and draws, per frame, a 4000 x 3000 matplotlib figure of the RGB frame,
the GT depth and, per method, an error map ``|gt - pred|``, the prediction and a "stability" image (the x-t
slice of the depth at one image column, filled in frame by frame), at seconds per frame.  Everything under the
figure is per-pixel lookup work on tensors the evaluation already leaves on the device; here the panels go
from those tensors straight to the bytes of the output file (``vda_depth_absdiff_range`` /
``vda_panel_compose``, csrc/vda_compare.hip), bit for bit what a plain host composition of the same panels
gives.  include/vda.h states the arithmetic and the three deviations from the figure (the colour index rule is
the project's ``save_video`` rule, a warmed-up method is paired with the GT frame its numbers are computed
against, no axes / text / line plot: the per-frame MSE series is returned, and written as CSV by the CLI).

* ``LibCompare`` / ``TorchCompare`` - the two backends: libvda kernels, and the same arithmetic in plain torch
  on any device (the orchestration and the CPU tests run on it; it is not a fallback of the product path).
* ``compare_depths`` - gt + raw predictions -> ``CompareResult`` (alignment, numbers, ranges, aligned tensors).
* ``compose_frames`` - ``CompareResult`` -> chunks of uint8 canvas frames in a file-ready layout.
* ``save_compare_video`` - the canvas as ``.y4m`` (4:4:4 or 4:2:0), gif, png or webp.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from .evaluate import ALIGN_MODES, LibEval, TorchEval, _as_tensor
from .ops import TILE_KINDS  # VDA_TILE_* (include/vda.h)
from .visualize import LAYOUTS, LibVis, TorchVis, _layout_code, named_color_table

MAX_METHODS = 3
DEPTH_MAP, ERROR_MAP = "Spectral", "RdYlGn"  # vis_util.py:131, :178


class LibCompare:
    """The comparison arithmetic on libvda kernels (GPU tensors only): ``range`` / ``absdiff_range`` -> [2]
    fp32 (min, max) on the device, ``compose(tiles, ...)`` -> uint8 canvas frames on the device
    (``ops.panel_compose``)."""
    eval = LibEval

    @staticmethod
    def range(depth):
        return LibVis.range(depth)

    @staticmethod
    def absdiff_range(pred, gt, valid=None):
        from . import ops
        return ops.depth_absdiff_range(pred, gt, valid)

    @staticmethod
    def compose(tiles, rows, cols, F, t0, N, xstar, lut0=None, lut1=None, layout="hwc"):
        from . import ops
        return ops.panel_compose(tiles, rows, cols, F, t0, N, xstar, lut0=lut0, lut1=lut1, layout=_layout_code(layout))


class TorchCompare:
    """``LibCompare``'s contract in plain torch on any device: every per-pixel operation a separate, separately
    rounded fp32 op (constants as fp32 tensors, divisions by tensors), then integer work."""
    eval = TorchEval

    @staticmethod
    def range(depth):
        return TorchVis.range(depth)

    @staticmethod
    def absdiff(pred, gt, valid=None):
        """The error map as displayed: ``valid ? |gt - pred| : 0`` (utils/metrics.py:92-98)."""
        e = (gt - pred).abs()
        if valid is not None:
            e = torch.where(valid != 0, e, torch.zeros((), dtype=e.dtype, device=e.device))
        return e

    @staticmethod
    def absdiff_range(pred, gt, valid=None):
        return TorchVis.range(TorchCompare.absdiff(pred, gt, valid))

    @staticmethod
    def rgb_to_yuv(rgb):
        """uint8 [..., 3] RGB -> uint8 [..., 3] YUV: ``video_io._rgb_to_yuv`` operation for operation."""
        def c(v):
            return torch.tensor(v, dtype=torch.float32, device=rgb.device)

        def q(a):
            return torch.clamp(torch.round(a), 0., 255.).to(torch.uint8)

        r, g, b = rgb.to(torch.float32).unbind(-1)
        y = (c(0.299) * r + c(0.587) * g) + c(0.114) * b
        u = (b - y) / c(1.772)
        v = (r - y) / c(1.402)
        return torch.stack([q(y * c(219.0 / 255.0) + c(16.0)), q(u * c(224.0 / 255.0) + c(128.0)),
                            q(v * c(224.0 / 255.0) + c(128.0))], -1)

    @staticmethod
    def _frames(src, s, zero):
        """src[s] per canvas frame, ``zero`` where s lies outside the source."""
        live = (s >= 0) & (s < src.shape[0])
        got = src[s.clamp(0, src.shape[0] - 1)]
        return torch.where(live.reshape((-1,) + (1,) * (src.dim() - 1)), got, zero)

    @staticmethod
    def compose(tiles, rows, cols, F, t0, N, xstar, lut0=None, lut1=None, layout="hwc"):
        code = _layout_code(layout)
        if code == LAYOUTS["index"]:
            raise ValueError("the canvas has no 'index' layout")
        src0 = tiles[0]["a"]
        dev, H, W = src0.device, int(src0.shape[1]), int(src0.shape[2])
        yuv = code != LAYOUTS["hwc"]
        canvas = torch.zeros(F, rows * H, cols * W, 3, dtype=torch.uint8, device=dev)
        if yuv:
            canvas[...] = torch.tensor([16, 128, 128], dtype=torch.uint8, device=dev)
        t = torch.arange(t0, t0 + F, device=dev)
        f0 = torch.zeros((), dtype=torch.float32, device=dev)
        for tile in tiles:
            kind = TILE_KINDS.get(tile["kind"], tile["kind"])
            a, o = tile["a"], int(tile.get("offset", 0))
            s = t - o
            if kind == TILE_KINDS["rgb"]:
                px = TorchCompare._frames(a, s, canvas.new_zeros(()))  # black outside the source
                px = TorchCompare.rgb_to_yuv(px) if yuv else px
            else:
                if kind == TILE_KINDS["depth"]:
                    v = TorchCompare._frames(a, s, f0)
                elif kind == TILE_KINDS["error"]:
                    m = tile.get("valid")  # outside the source pred = gt = 0: the error is 0
                    v = TorchCompare.absdiff(TorchCompare._frames(a, s, f0), TorchCompare._frames(tile["b"], s, f0),
                                             None if m is None else TorchCompare._frames(m, s, m.new_zeros(())))
                else:  # the [H, N] stability image, stretched to W columns and filled in up to column t
                    c = (torch.arange(W, device=dev, dtype=torch.int64) * N) // W
                    sc = c - o
                    img = a[sc.clamp(0, a.shape[0] - 1), :, xstar].transpose(0, 1)  # [H, W]
                    ok = (c[None] <= t[:, None]) & ((sc >= 0) & (sc < a.shape[0]))[None]  # [F, W]
                    v = torch.where(ok[:, None, :], img[None], f0)
                lut = lut1 if int(tile.get("lut", 0)) else lut0
                px = lut[TorchVis.index(v, tile["range"]).long()]
            r, cc = int(tile["row"]), int(tile["col"])
            canvas[:, r * H:(r + 1) * H, cc * W:(cc + 1) * W] = px
        if code == LAYOUTS["hwc"]:
            return canvas
        planes = canvas.permute(0, 3, 1, 2)
        if code == LAYOUTS["planar444"]:
            return planes.contiguous()
        return torch.cat([planes[:, 0].reshape(F, -1), TorchVis.subsample(planes[:, 1]).reshape(F, -1),
                          TorchVis.subsample(planes[:, 2]).reshape(F, -1)], 1).contiguous()


@dataclass
class MethodResult:
    """One method of a ``CompareResult``.  ``scale`` / ``shift``: floats ([N_m] arrays with
    ``align="per_frame"``).  ``abs_error`` = S |gt[o:] - pred| / gt.size: divided by the size of the WHOLE gt
    also for a warmed-up method (o > 0), as calculate_metrics.py:226 does.  ``mse`` = mean((pred - gt[o:])^2)
    (:224), ``frame_mse`` [N_m] the same per frame (vis_util.py:96-100), all unmasked.  ``aligned`` [N_m, H, W]:
    the aligned metric depth on the compute device; ``offset`` = o = N - N_m, the warm-up."""
    scale: object
    shift: object
    abs_error: float
    mse: float
    frame_mse: np.ndarray
    offset: int
    aligned: torch.Tensor


@dataclass
class CompareResult:
    """``methods`` in panel order (row 1 + i).  ``depth_range`` / ``error_range``: [2] fp32 tensors on the
    compute device (the ranges of the colour maps).  ``gt`` [N, H, W], ``rgb`` [N, H, W, 3] uint8 or None and
    ``valid`` (uint8 or None) lie there too."""
    methods: Dict[str, MethodResult]
    depth_range: torch.Tensor
    error_range: torch.Tensor
    gt: torch.Tensor
    rgb: Optional[torch.Tensor]
    valid: Optional[torch.Tensor]
    stability_line: float
    backend: type = field(repr=False, default=TorchCompare)

    @property
    def xstar(self) -> int:
        return int(self.gt.shape[2] * self.stability_line)  # vis_util.py:31

    @property
    def canvas_size(self):
        """(height, width) of a canvas frame."""
        return (1 + len(self.methods)) * int(self.gt.shape[1]), 3 * int(self.gt.shape[2])


def _range_tensor(r, device, name):
    r = torch.as_tensor(r, dtype=torch.float32).reshape(-1).to(device).contiguous()
    if r.numel() != 2:
        raise ValueError(f"{name} must hold (min, max), got {r.numel()} values")
    return r


def compare_depths(gt, preds, rgb=None, valid=None, max_depth: float = 80., align: str = "first",
                   stability_line: float = 0.5, depth_range=None, error_range=None, device=None,
                   backend=None) -> CompareResult:
    """Align up to three predictions of one scene to ``gt`` and collect what the comparison video shows.

    ``gt`` [N, H, W] metres; ``preds`` maps method names to raw inverse depth [N_m, H, W], N_m <= N: a method with
    fewer frames is a streaming run whose first o = N - N_m frames were warm-up, its frame k pairs with
    gt[o + k] (calculate_metrics.py:179-182, :223-226).  ``rgb`` [N, H, W, 3] uint8 and ``valid`` [N, H, W] (masks
    the error maps, utils/metrics.py:92-98) are optional.  Numpy arrays or tensors; tensors are used where they
    lie.  The computation runs on ``device`` (default: the device of the first prediction given as a tensor, else
    the CPU): ``LibCompare`` on a GPU, ``TorchCompare`` elsewhere.

    Each method is fitted in inverse depth over ``gt < max_depth`` (and ``valid``), with ``align="first"`` on its
    first frame as the reference does (calculate_metrics.py:176-204), ``"all"`` / ``"per_frame"`` as
    ``evaluate_depth``; the numbers are unmasked sums of ``vda_depth_eval_metrics``.  The depth range is the
    (min, max) over all aligned predictions, not the GT (vis_util.py:75-82), the error range that of the error
    maps as displayed (:84-94); ``depth_range`` / ``error_range`` override them, so that several scenes can share
    one scale."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align must be one of {ALIGN_MODES}, got {align!r}")
    if not float(max_depth) > 0:
        raise ValueError(f"max_depth must be greater than 0, got {max_depth}")
    if not 0. <= float(stability_line) < 1.:
        raise ValueError(f"stability_line must lie in [0, 1), got {stability_line}")
    if not isinstance(preds, dict) or not 1 <= len(preds) <= MAX_METHODS:
        raise ValueError(f"preds must map 1 to {MAX_METHODS} method names to predictions")
    if device is None:
        device = next((p.device for p in preds.values() if isinstance(p, torch.Tensor)), torch.device("cpu"))
    device = torch.device(device)
    if backend is None:
        backend = LibCompare if device.type == "cuda" else TorchCompare
    gt = _as_tensor(gt, torch.float32, device, "gt")
    if gt.dim() != 3 or gt.numel() < 1:
        raise ValueError(f"gt must be a non-empty [N, H, W], got {tuple(gt.shape)}")
    N, H, W = (int(v) for v in gt.shape)
    if valid is not None:
        valid = _as_tensor(valid, None, device, "valid")
        if valid.dtype not in (torch.bool, torch.uint8) or valid.shape != gt.shape:
            raise ValueError(f"valid must be bool / uint8 with gt's shape, got {valid.dtype} {tuple(valid.shape)}")
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    if rgb is not None:
        rgb = _as_tensor(rgb, None, device, "rgb")
        if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (N, H, W, 3):
            raise ValueError(f"rgb must be uint8 [{N}, {H}, {W}, 3], got {rgb.dtype} {tuple(rgb.shape)}")
    fit_mask = gt < float(max_depth)
    if valid is not None:
        fit_mask = fit_mask & (valid != 0)
    fit_mask = fit_mask.view(torch.uint8)
    methods, dranges, eranges = {}, [], []
    for name, pred in preds.items():
        pred = _as_tensor(pred, torch.float32, device, f"preds[{name!r}]")
        if pred.dim() != 3 or tuple(pred.shape[1:]) != (H, W) or not 1 <= pred.shape[0] <= N:
            raise ValueError(f"preds[{name!r}] must be [N_m <= {N}, {H}, {W}], got {tuple(pred.shape)}")
        o = N - int(pred.shape[0])
        g, m = gt[o:], fit_mask[o:]
        if align == "first":
            ss, _ = backend.eval.fit(pred[:1], g[:1], m[:1], False)
        else:
            ss, _ = backend.eval.fit(pred, g, m, align == "per_frame")
        fs, _, aligned = backend.eval.metrics(pred, g, None, ss, float(max_depth), True)
        dranges.append(backend.range(aligned))
        eranges.append(backend.absdiff_range(aligned, g, None if valid is None else valid[o:]))
        fs_h, ss_h = fs.cpu().numpy(), ss.reshape(-1, 2).cpu().numpy()
        if align == "per_frame":
            scale, shift = ss_h[:, 0].copy(), ss_h[:, 1].copy()
        else:
            scale, shift = float(ss_h[0, 0]), float(ss_h[0, 1])
        methods[str(name)] = MethodResult(scale=scale, shift=shift, abs_error=float(fs_h[:, 5].sum() / gt.numel()),
                                          mse=float(fs_h[:, 7].sum() / pred.numel()), frame_mse=fs_h[:, 7] / fs_h[:, 0],
                                          offset=o, aligned=aligned)

    def union(rs):
        r = torch.stack(rs)
        return torch.stack([r[:, 0].min(), r[:, 1].max()])

    drange = union(dranges) if depth_range is None else _range_tensor(depth_range, device, "depth_range")
    erange = union(eranges) if error_range is None else _range_tensor(error_range, device, "error_range")
    return CompareResult(methods=methods, depth_range=drange, error_range=erange, gt=gt, rgb=rgb, valid=valid,
                         stability_line=float(stability_line), backend=backend)


def panel_tiles(result: CompareResult) -> list:
    """The tile list of ``result``'s canvas: row 0 RGB | GT depth | GT stability, row 1 + i error map |
    prediction | stability of method i (vis_util.py:123-194; the reference's third cell of row 0 is the line
    plot and its GT stability image a separate file)."""
    gt, dr, er = result.gt, result.depth_range, result.error_range
    tiles = []
    if result.rgb is not None:
        tiles.append(dict(kind="rgb", row=0, col=0, a=result.rgb))
    tiles.append(dict(kind="depth", row=0, col=1, a=gt, range=dr, lut=0))
    tiles.append(dict(kind="xt", row=0, col=2, a=gt, range=dr, lut=0))
    for i, m in enumerate(result.methods.values()):
        o = m.offset
        tiles.append(dict(kind="error", row=1 + i, col=0, a=m.aligned, b=gt[o:], offset=o, range=er, lut=1,
                          valid=None if result.valid is None else result.valid[o:]))
        tiles.append(dict(kind="depth", row=1 + i, col=1, a=m.aligned, offset=o, range=dr, lut=0))
        tiles.append(dict(kind="xt", row=1 + i, col=2, a=m.aligned, offset=o, range=dr, lut=0))
    return tiles


def compose_frames(result: CompareResult, layout: str = "hwc", chunk: int = 32, backend=None) -> Iterator[np.ndarray]:
    """The canvas frames of ``result`` in chunks of at most ``chunk`` frames as uint8 numpy arrays in ``layout``
    ("hwc" [F, CH, CW, 3] RGB; "planar444" [F, 3, CH, CW] / "planar420" [F, CH*CW + 2*ch*cw] YUV, the payloads
    of y4m frames).  On a GPU the chunks pass through two pinned staging buffers with non-blocking copies, as in
    ``colorize_depths_device``: a yielded array is a view of a staging buffer, valid until the generator is
    advanced."""
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    code = _layout_code(layout)
    if code == LAYOUTS["index"]:
        raise ValueError("the canvas has no 'index' layout")
    backend = result.backend if backend is None else backend
    dev = result.gt.device
    yuv = code != LAYOUTS["hwc"]
    lut0 = torch.from_numpy(named_color_table(DEPTH_MAP, yuv)).to(dev)
    lut1 = torch.from_numpy(named_color_table(ERROR_MAP, yuv)).to(dev)
    tiles, rows, N, chunk = panel_tiles(result), 1 + len(result.methods), int(result.gt.shape[0]), int(chunk)

    def compose(a):
        return backend.compose(tiles, rows, 3, min(chunk, N - a), a, N, result.xstar, lut0, lut1, code)

    if dev.type != "cuda":
        for a in range(0, N, chunk):
            yield compose(a).numpy()
        return
    ring, pending = [None, None], None
    for k, a in enumerate(range(0, N, chunk)):
        out = compose(a)
        if ring[k % 2] is None:  # the first chunk is the largest
            ring[k % 2] = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
        host = ring[k % 2][:out.numel()].view(out.shape)
        host.copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        if pending is not None:
            pending[1].synchronize()
            yield pending[0].numpy()
        pending = (host, ev)
    pending[1].synchronize()
    yield pending[0].numpy()


def save_compare_video(path: str, result: CompareResult, fps: float = 10., chroma: str = "444", chunk: int = 32,
                       backend=None):
    """Write ``result``'s canvas video: ``.y4m`` (``chroma`` "444" or "420", the frames arrive as payloads and are
    written as they arrive), or gif / png / webp through Pillow."""
    from . import video_io
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        ch, cw = result.canvas_size
        head = video_io._y4m_header(cw, ch, fps, chroma)
        with open(path, "wb") as f:
            f.write(head)
            for block in compose_frames(result, "planar" + chroma, chunk, backend):
                for payload in block:
                    f.write(b"FRAME\n")
                    f.write(payload.tobytes())
        return
    if ext not in (".gif", ".png", ".webp", ".apng"):
        raise ValueError(f"{path}: the comparison video is written as .y4m, .gif, .png or .webp")
    from PIL import Image
    ims = [Image.fromarray(f.copy()) for block in compose_frames(result, "hwc", chunk, backend) for f in block]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=int(round(1000 / fps)), loop=0)


def stability_image(result: CompareResult, lut: Optional[np.ndarray] = None) -> np.ndarray:
    """The GT stability image [H, N, 3] uint8 (vis_util.py:138, :203-208): column t is gt[t, :, x*], coloured with
    the depth map over the depth range by the panels' index rule."""
    lut = named_color_table(DEPTH_MAP) if lut is None else lut
    sl = result.gt[:, :, result.xstar].transpose(0, 1).contiguous()  # [H, N]
    idx = TorchVis.index(sl, result.depth_range).cpu().numpy()
    return lut[idx]
