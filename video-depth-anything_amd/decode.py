"""Video frames from the bytes of a .y4m file to the network input, without the host decode.

``video_io.read_y4m`` reads the whole file, repeats the chroma planes to luma size, converts every pixel in
numpy fp32 and stacks a 3-bytes-per-pixel copy of the video in host memory.  The device needs only the bytes the
file already holds: ``video_io.open_y4m`` indexes the file (``Y4MFrames``), each window batch uploads the planar
YUV payload of the frames it needs (1.5 bytes per pixel at 4:2:0), and ``vda_preprocess_yuv`` (csrc/vda_decode.hip)
turns them into the normalised, resized input: bit for bit what ``vda_preprocess_frames`` makes of the frames
``read_y4m`` decodes.  See include/vda.h for the plane layout and the arithmetic.

* ``LibDecode`` - the kernels (GPU tensors only).
* ``TorchDecode`` - the same YUV -> RGB arithmetic in plain torch, one rounding per operation; it runs on the CPU
  and is what the tests compare with where there is no GPU.  It is not a fallback of the product path.
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
    def preprocess(payload, h, w, chroma, size, mean, std):
        import torch.nn.functional as F
        x = TorchDecode.yuv_to_rgb(payload, h, w, chroma).permute(0, 3, 1, 2).float() / 255.0
        x = F.interpolate(x, size=(int(size[0]), int(size[1])), mode="bicubic", align_corners=False)
        m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        return (x - m) / s
