"""Video frames from the bytes of a .y4m file to the network input, without the host decode.

``video_io.read_y4m`` reads the whole file, repeats the chroma planes to luma size, converts every pixel in
numpy fp32 and stacks a 3-bytes-per-pixel copy of the video in host memory.  The device needs only the bytes the
file already holds: ``video_io.open_y4m`` indexes the file (``Y4MFrames``), each window batch uploads the planar
YUV payload of the frames it needs (1.5 bytes per pixel at 4:2:0), and ``vda_preprocess_yuv`` (csrc/vda_decode.hip)
turns them into the normalised, resized input: bit for bit what ``vda_preprocess_frames`` makes of the frames
``read_y4m`` decodes.  See include/vda.h for the plane layout and the arithmetic.

Frames that ``read_video_frames`` would downscale for ``max_res`` (``open_y4m(path, max_res=M)``) are downscaled
on the device as well: ``vda_yuv_downscale`` restates Pillow's antialiased bicubic ``Image.resize``, which runs in
integer fixed point for 8-bit images, from the coefficient tables of ``resample_tables`` and gives the same RGB
frames bit for bit; ``vda_preprocess_frames`` then takes them as it takes host frames.

* ``LibDecode`` - the kernels (GPU tensors only).
* ``TorchDecode`` - the same YUV -> RGB arithmetic in plain torch, one rounding per operation, and the downscale in
  int32 torch; it runs on the CPU and is what the tests compare with where there is no GPU.  It is not a fallback
  of the product path.
* ``resample_tables`` - the resampling coefficients of one axis in Python floats (``vda_resample_tables`` in C).
"""
from __future__ import annotations

import torch

CHROMA = {"420": 0, "422": 1, "444": 2, "mono": 3}  # VDA_YUV_* (include/vda.h)


def chroma_code(chroma) -> int:
    code = CHROMA.get(chroma) if isinstance(chroma, str) else int(chroma)
    if code not in CHROMA.values():
        raise ValueError(f"chroma must be one of {sorted(CHROMA)}, got {chroma!r}")
    return code


def plane_sizes(h: int, w: int, chroma) -> tuple:
    """(cw, ch, sx, sy): the chroma plane size and the chroma shifts of an h x w frame (mono: no planes)."""
    code = chroma_code(chroma)
    sx = 1 if code in (CHROMA["420"], CHROMA["422"]) else 0
    sy = 1 if code == CHROMA["420"] else 0
    if code == CHROMA["mono"]:
        return 0, 0, 0, 0
    return (w + sx) >> sx, (h + sy) >> sy, sx, sy


def payload_bytes(h: int, w: int, chroma) -> int:
    cw, ch, _, _ = plane_sizes(h, w, chroma)
    return h * w + 2 * cw * ch


RESAMPLE_BITS = 22  # fractional bits of a resampling coefficient (Pillow's PRECISION_BITS for 8-bit images)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def resample_taps(n_in: int, n_out: int) -> int:
    """Coefficients per output position of ``resample_tables(n_in, n_out)``."""
    import math
    support = 2.0 * max(n_in / n_out, 1.0)
    return int(math.ceil(support)) * 2 + 1


def resample_tables(n_in: int, n_out: int):
    """The fixed-point coefficients of Pillow's antialiased bicubic resampling of one axis from ``n_in`` to
    ``n_out`` samples (``Image.resize(..., Image.BICUBIC)`` on an 8-bit image): ``(k int32 [n_out, ksize],
    bounds int32 [n_out, 2])``.  Output ``xx`` is ``clamp((2^21 + sum_x src[xmin + x] * k[xx, x]) >> 22, 0, 255)``
    over ``x < n`` with ``bounds[xx] = (xmin, n)``; ``k[xx, n:]`` is 0.  Python floats are IEEE doubles, every
    operation rounded once, as ``vda_resample_tables`` (include/vda.h) computes them."""
    import math
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample_tables needs positive sizes, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    one = float(1 << RESAMPLE_BITS)
    k = [[0] * ksize for _ in range(n_out)]
    bounds = [[0, 0] for _ in range(n_out)]
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * inv) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        row = k[xx]
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            row[x] = int(v * one + (-0.5 if v < 0 else 0.5))
        bounds[xx] = [xmin, n]
    return (torch.tensor(k, dtype=torch.int32).reshape(n_out, ksize),
            torch.tensor(bounds, dtype=torch.int32).reshape(n_out, 2))


class LibDecode:
    """Planar YUV frames on libvda kernels: ``payload`` [N, frame_stride] uint8 on the GPU, one frame's Y, U and
    V planes per row (any base alignment, rows may be padded)."""

    @staticmethod
    def yuv_to_rgb(payload, h, w, chroma):
        from . import ops
        return ops.yuv_to_rgb(payload, h, w, chroma_code(chroma))

    @staticmethod
    def preprocess(payload, h, w, chroma, size, mean, std):
        from . import ops
        return ops.preprocess_yuv(payload, h, w, chroma_code(chroma), int(size[0]), int(size[1]), mean, std)

    @staticmethod
    def downscale(payload, h, w, chroma, size):
        """RGB uint8 [N, size[0], size[1], 3]: the decoded frames resized as ``video_io._resize_rgb`` (Pillow's
        antialiased bicubic) resizes them, bit for bit (vda_yuv_downscale)."""
        from . import ops
        return ops.yuv_downscale(payload, h, w, chroma_code(chroma), int(size[0]), int(size[1]))


class TorchDecode:
    """``LibDecode``'s contract in plain torch on any device.  ``yuv_to_rgb`` restates ``video_io._yuv_to_rgb``
    operation by operation in float32 (constants rounded to float32 first, g = (yf - cu * uf) - cv * vf in that
    order, ``torch.round`` = ties to even, clamp, cast) and equals it bit for bit; ``preprocess`` resizes with
    torch's bicubic, which agrees with the kernel to rounding only."""

    @staticmethod
    def convert(y, u, v):
        """uint8 tensors of one shape -> uint8 [..., 3]."""
        f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=y.device)  # noqa: E731
        yf = (y.float() - 16.0) * f32(255.0 / 219.0)
        uf = (u.float() - 128.0) * f32(255.0 / 224.0)
        vf = (v.float() - 128.0) * f32(255.0 / 224.0)
        r = yf + f32(1.402) * vf
        g = (yf - f32(0.344136) * uf) - f32(0.714136) * vf
        b = yf + f32(1.772) * uf
        return torch.clamp(torch.round(torch.stack([r, g, b], -1)), 0, 255).to(torch.uint8)

    @staticmethod
    def yuv_to_rgb(payload, h, w, chroma):
        cw, ch, sx, sy = plane_sizes(h, w, chroma)
        N = payload.shape[0]
        y = payload[:, :h * w].reshape(N, h, w)
        if cw == 0:
            u = v = torch.full_like(y, 128)
        else:
            yy = (torch.arange(h, device=payload.device) >> sy).view(h, 1)
            xx = (torch.arange(w, device=payload.device) >> sx).view(1, w)
            u = payload[:, h * w:h * w + cw * ch].reshape(N, ch, cw)[:, yy, xx]
            v = payload[:, h * w + cw * ch:h * w + 2 * cw * ch].reshape(N, ch, cw)[:, yy, xx]
        return TorchDecode.convert(y, u, v).contiguous()

    @staticmethod
    def resample(x, dim, n_out):
        """One pass of Pillow's 8-bit resampling along ``dim`` of a uint8 tensor, in int32 from
        ``resample_tables``: one gather and one multiply-add per coefficient column."""
        n_in = int(x.shape[dim])
        k, bounds = resample_tables(n_in, n_out)
        k, xmin = k.to(x.device), bounds[:, 0].to(x.device).long()
        view = [1] * x.dim()
        view[dim] = n_out
        acc = torch.full([n_out if d == dim else s for d, s in enumerate(x.shape)], 1 << (RESAMPLE_BITS - 1),
                         dtype=torch.int32, device=x.device)
        for t in range(k.shape[1]):  # k is 0 past a row's n taps, so the clamped index is never weighted
            acc += x.index_select(dim, torch.clamp(xmin + t, max=n_in - 1)).int() * k[:, t].view(view)
        return torch.clamp(acc >> RESAMPLE_BITS, 0, 255).to(torch.uint8)

    @staticmethod
    def downscale(payload, h, w, chroma, size):
        """``LibDecode.downscale`` in integer torch arithmetic: the horizontal pass over the decoded frames,
        rounded to uint8, then the vertical pass; a pass whose size does not change is skipped."""
        h2, w2 = int(size[0]), int(size[1])
        x = TorchDecode.yuv_to_rgb(payload, h, w, chroma)
        if w2 != w:
            x = TorchDecode.resample(x, 2, w2)
        if h2 != h:
            x = TorchDecode.resample(x, 1, h2)
        return x.contiguous()

    @staticmethod
    def preprocess(payload, h, w, chroma, size, mean, std):
        import torch.nn.functional as F
        x = TorchDecode.yuv_to_rgb(payload, h, w, chroma).permute(0, 3, 1, 2).float() / 255.0
        x = F.interpolate(x, size=(int(size[0]), int(size[1])), mode="bicubic", align_corners=False)
        m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        return (x - m) / s
