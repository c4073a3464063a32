"""Depth visualisation without the host passes: the reference's ``save_video`` colouring (utils/dc_utils.py:74-85).

The reference normalises the whole clip to uint8 with its min / max and maps the result through matplotlib's
inferno (or Spectral) table; ``video_io.colorize_depths`` restates that in numpy (about eight full-size passes,
one of them a float64 ``[F, H, W, 3]`` gather) and ``video_io.write_y4m`` converts every frame to BT.601 YUV
(six more float passes).  All of it is a lookup: the normalised depth is a uint8 index, and inferno, Spectral
and their YUV conversions are 256-row tables, bit-identical to what the host path computes per pixel.  Here
the depth that already lies on the device (``infer_video_depth(stitch="device", return_device=True)``) becomes
the bytes of the output file in two kernels (``vda_depth_range`` / ``vda_depth_colorize``, csrc/vda_vis.hip),
and 1 to 3 bytes per pixel cross to the host instead of 4; see include/vda.h for the arithmetic, the layouts
and the stated deviation (NaN / out-of-range indices clamp, numpy's cast is undefined there).

* ``color_table`` - the 256-row RGB or YUV table of a colour map, from ``colorize_depths``' own expressions.
* ``named_color_table`` - the same for any matplotlib map by name (the comparison video's RdYlGn).
* ``LibVis`` / ``TorchVis`` - the two backends: libvda kernels, and the same arithmetic in plain torch on any
  device (the orchestration and the CPU tests run on it; it is not a fallback of the product path).
* ``colorize_depths_device`` - depth tensor -> chunks of uint8 numpy arrays in a file-ready layout.
"""
from __future__ import annotations

from typing import Iterator, Optional

import numpy as np
import torch

LAYOUTS = {"index": 0, "hwc": 1, "planar444": 2, "planar420": 3}  # VDA_VIS_* (include/vda.h)


def color_table(grayscale: bool = False, spectral: bool = False, yuv: bool = False) -> np.ndarray:
    """uint8 [256, 3]: row i is what ``video_io.colorize_depths`` gives a pixel of index i (grey: (i, i, i)),
    with ``yuv`` pushed through ``video_io._rgb_to_yuv`` (what ``write_y4m`` stores for that pixel)."""
    from . import video_io
    idx = np.arange(256, dtype=np.uint8)
    if grayscale:
        table = np.stack([idx, idx, idx], -1)
    else:
        import matplotlib
        if spectral:
            table = (matplotlib.colormaps["Spectral"](idx)[..., :3] * 255).astype(np.uint8)
        else:
            table = (np.array(matplotlib.colormaps["inferno"].colors)[idx] * 255).astype(np.uint8)
    if yuv:
        table = np.stack(video_io._rgb_to_yuv(table), -1)
    return np.ascontiguousarray(table, dtype=np.uint8)


def named_color_table(name: str, yuv: bool = False) -> np.ndarray:
    """uint8 [256, 3]: matplotlib's colour map ``name`` (e.g. "RdYlGn") sampled with the expression
    ``color_table`` uses for Spectral, so ``named_color_table("Spectral")`` is ``color_table(spectral=True)``;
    ``yuv`` as there."""
    from . import video_io
    import matplotlib
    idx = np.arange(256, dtype=np.uint8)
    table = (matplotlib.colormaps[name](idx)[..., :3] * 255).astype(np.uint8)
    if yuv:
        table = np.stack(video_io._rgb_to_yuv(table), -1)
    return np.ascontiguousarray(table, dtype=np.uint8)


def _layout_code(layout) -> int:
    code = LAYOUTS.get(layout) if isinstance(layout, str) else int(layout)
    if code not in LAYOUTS.values():
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return code


class LibVis:
    """The visualisation arithmetic on libvda kernels (GPU tensors only): ``range(depth)`` -> [2] fp32
    (min, max) on the device, and ``colorize(depth [F, H, W], range, lut [256, 3] uint8 or None, layout)`` ->
    uint8 on the device, [F, H, W] / [F, H, W, 3] / [F, 3, H, W] / [F, H*W + 2*ch*cw]."""

    @staticmethod
    def range(depth):
        from . import ops
        return ops.depth_range(depth)

    @staticmethod
    def colorize(depth, range, lut, layout):
        from . import ops
        return ops.depth_colorize(depth, range, lut=lut, layout=_layout_code(layout))


class TorchVis:
    """``LibVis``'s contract in plain torch on any device: the same fp32 operations, each rounded on its own
    (the division is by a tensor, never by a Python scalar, which torch may turn into a multiplication by
    the reciprocal), the same clamp before the cast, the same integer 2x2 average."""

    @staticmethod
    def range(depth):
        nan = torch.isnan(depth)
        inf = torch.full((), float("inf"), dtype=depth.dtype, device=depth.device)
        return torch.stack([torch.where(nan, inf, depth).min(), torch.where(nan, -inf, depth).max()]).float()

    @staticmethod
    def index(depth, range):
        x = (depth - range[0]) / (range[1] - range[0]) * 255
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        x = torch.where(x >= 255, torch.full_like(zero, 255.), torch.where(x > 0, x, zero))  # NaN -> 0
        return x.to(torch.uint8)

    @staticmethod
    def subsample(plane):
        """[F, H, W] uint8 -> [F, ch, cw]: (a + b + c + d + 2) >> 2 over 2x2 blocks, edges repeated."""
        p = plane.to(torch.int32)
        if p.shape[1] % 2:
            p = torch.cat([p, p[:, -1:]], 1)
        if p.shape[2] % 2:
            p = torch.cat([p, p[:, :, -1:]], 2)
        s = p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2
        return (s >> 2).to(torch.uint8)

    @staticmethod
    def colorize(depth, range, lut, layout):
        code = _layout_code(layout)
        idx = TorchVis.index(depth, range)
        if code == LAYOUTS["index"]:
            return idx
        if lut is None:
            raise ValueError("every layout but 'index' needs a lut")
        col = lut[idx.long()]  # [F, H, W, 3]
        if code == LAYOUTS["hwc"]:
            return col.contiguous()
        planes = col.permute(0, 3, 1, 2)
        if code == LAYOUTS["planar444"]:
            return planes.contiguous()
        F = depth.shape[0]
        return torch.cat([planes[:, 0].reshape(F, -1), TorchVis.subsample(planes[:, 1]).reshape(F, -1),
                          TorchVis.subsample(planes[:, 2]).reshape(F, -1)], 1).contiguous()


def colorize_depths_device(depth, grayscale: bool = False, spectral: bool = False, layout: str = "hwc",
                           chunk: int = 32, backend=None, yuv: Optional[bool] = None) -> Iterator[np.ndarray]:
    """Colour ``depth`` [F, H, W] (a float32 tensor, used where it lies) as ``video_io.colorize_depths`` does
    and yield it in chunks of at most ``chunk`` frames as uint8 numpy arrays in ``layout``.

    The range is computed once over the whole tensor, the colouring runs per chunk.  ``yuv`` selects the YUV
    table (default: for the two planar layouts, which are y4m payloads).  On a GPU the chunks pass through two
    pinned staging buffers with non-blocking copies: chunk k + 1 is colourised and copied while the caller
    works on chunk k, and host memory stays flat in the video length.  A yielded array is a view of a staging
    buffer then: it is valid until the generator is advanced, copy it to keep it."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 3 or depth.numel() < 1:
        raise ValueError("depth must be a non-empty float32 [F, H, W] tensor")
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    code = _layout_code(layout)
    if backend is None:
        backend = LibVis if depth.is_cuda else TorchVis
    depth = depth.contiguous()
    lut = None
    if code != LAYOUTS["index"]:
        use_yuv = code in (LAYOUTS["planar444"], LAYOUTS["planar420"]) if yuv is None else bool(yuv)
        lut = torch.from_numpy(color_table(grayscale, spectral, use_yuv)).to(depth.device)
    rng = backend.range(depth)
    F, chunk = depth.shape[0], int(chunk)
    if not depth.is_cuda:
        for a in range(0, F, chunk):
            yield backend.colorize(depth[a:a + chunk], rng, lut, code).numpy()
        return
    ring, pending = [None, None], None
    for k, a in enumerate(range(0, F, chunk)):
        out = backend.colorize(depth[a:a + chunk], rng, lut, code)
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
