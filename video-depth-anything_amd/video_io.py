"""Video I/O and output formats around the depth path (utils/dc_utils.py:19-89, run.py:150-166).

The reference decodes with decord (or cv2) and encodes mp4 with imageio/ffmpeg; none of those is
installed in this image, so this module keeps the reference's *semantics* and supplies decoders
and encoders that need only numpy / Pillow:

* ``read_video_frames(path, process_length, target_fps=-1, max_res=-1) -> (frames uint8 [N,h,w,3], fps)``
  (dc_utils.py:19-69).  Containers: YUV4MPEG2 ``.y4m`` (uncompressed 4:2:0 / 4:2:2 / 4:4:4 / mono,
  the format ffmpeg emits with ``-f yuv4mpegpipe``), ``.npy`` / ``.npz`` frame stacks, animated
  GIF / PNG / WebP / multi-page TIFF and directories of images via Pillow; compressed containers
  (.mp4 ...) go through decord when it is importable.  Frame stride = max(round(source_fps / target_fps), 1); at most
  ``process_length`` frames; ``max_res`` scales the longer side down (decord branch: sizes rounded
  and made even, dc_utils.py:22-29).
* ``open_y4m(path, process_length, target_fps, max_res=-1) -> (Y4MFrames, fps)``: a ``.y4m`` file indexed and
  memory-mapped but not decoded, with the same frame selection.  ``Y4MFrames.payload`` hands out the planar YUV bytes
  of frames (what ``infer_video_depth`` uploads on a GPU, vda_amd.decode), ``rgb`` / ``np.asarray`` decode as
  ``read_y4m``; with a ``max_res`` below the longer side its RGB frames are the downscaled ones of
  ``read_video_frames`` (on a GPU made from the same payload by vda_yuv_downscale).
* ``save_video(frames, path, fps, is_depths, grayscale, spectral)`` (dc_utils.py:72-89): depth is
  min/max-normalised to uint8 over the whole clip and mapped through matplotlib's inferno (or
  Spectral) table; written as ``.y4m`` (4:4:4), or animated GIF / PNG / WebP via Pillow; ``.mp4``
  needs imageio + ffmpeg and raises a clear error without them.  ``chroma="420"`` writes a 4:2:0 ``.y4m``;
  depth given as a CUDA tensor is coloured on the device (vda_amd.visualize) and gives the same files.
* ``save_npz`` (``depths`` key, run.py:162-164) and ``save_tiff`` (float32 multi-page, :165-166).

YUV <-> RGB uses BT.601 limited range (ffmpeg's default for SD/unknown-matrix y4m); decoded frames
of the reference's decord path are therefore parity-unpinned here (no decoder to compare with).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np

_IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")


def ensure_even(v: int) -> int:
    return v if v % 2 == 0 else v + 1


# ---- YUV4MPEG2 -------------------------------------------------------------------------------
def _yuv_to_rgb(y: np.ndarray, u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """BT.601 limited range -> RGB uint8 (planes already at luma resolution)."""
    yf = (y.astype(np.float32) - 16.0) * (255.0 / 219.0)
    uf = (u.astype(np.float32) - 128.0) * (255.0 / 224.0)
    vf = (v.astype(np.float32) - 128.0) * (255.0 / 224.0)
    r = yf + 1.402 * vf
    g = yf - 0.344136 * uf - 0.714136 * vf
    b = yf + 1.772 * uf
    return np.clip(np.rint(np.stack([r, g, b], -1)), 0, 255).astype(np.uint8)


def _rgb_to_yuv(rgb: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    f = rgb.astype(np.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = (b - y) / 1.772
    v = (r - y) / 1.402
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)  # noqa: E731
    return q(y * (219.0 / 255.0) + 16.0), q(u * (224.0 / 255.0) + 128.0), q(v * (224.0 / 255.0) + 128.0)


def _parse_ratio(s: str) -> float:
    a, b = s.split(":")
    return float(a) / float(b) if float(b) else 0.0


def _decode_payload(buf: np.ndarray, w: int, h: int, cw: int, ch: int) -> np.ndarray:
    """One frame's planar payload (Y, then U and V of ch x cw) -> RGB uint8 [h, w, 3], chroma taken nearest."""
    y = buf[:w * h].reshape(h, w)
    if cw == 0:
        u = v = np.full((h, w), 128, np.uint8)
    else:
        u = buf[w * h:w * h + cw * ch].reshape(ch, cw)
        v = buf[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
        ry, rx = (2 if ch != h else 1), (2 if cw != w else 1)  # nearest chroma upsampling
        u = np.repeat(np.repeat(u, ry, 0), rx, 1)[:h, :w]
        v = np.repeat(np.repeat(v, ry, 0), rx, 1)[:h, :w]
    return _yuv_to_rgb(y, u, v)


def _y4m_stream_header(data, path: str, refuse_depth_suffix: bool = False):
    """The stream header of a YUV4MPEG2 file (bytes or a memory map) -> (w, h, fps, cw, ch, "420" / "422" /
    "444" / "mono", offset of the first frame header); 8-bit 420 / 422 / 444 / mono only.  ``read_y4m`` takes
    a ``p<bits>`` suffix (C420p10) for a siting tag (C420paldv) and fails at the first frame header instead;
    ``refuse_depth_suffix`` refuses it here."""
    nl = data.find(b"\n")
    if nl < 0:
        raise ValueError(f"{path}: not a YUV4MPEG2 stream")
    head = bytes(data[:nl]).decode("ascii").split()
    if not head or head[0] != "YUV4MPEG2":
        raise ValueError(f"{path}: not a YUV4MPEG2 stream")
    w = h = None
    fps, cs = 25.0, "420"
    for tok in head[1:]:
        k, val = tok[0], tok[1:]
        if k == "W":
            w = int(val)
        elif k == "H":
            h = int(val)
        elif k == "F":
            fps = _parse_ratio(val)
        elif k == "C":
            cs = val
    if w is None or h is None:
        raise ValueError(f"{path}: y4m header lacks W/H")
    base = cs.split("p")[0]
    if refuse_depth_suffix and cs[len(base):].startswith("p") and cs[len(base) + 1:].isdigit():
        base = ""  # a bit depth, not a siting tag: refused below
    if base.startswith("420"):
        cw, ch = (w + 1) // 2, (h + 1) // 2
    elif base == "422":
        cw, ch = (w + 1) // 2, h
    elif base == "444":
        cw, ch = w, h
    elif base == "mono":
        cw = ch = 0
    else:
        raise ValueError(f"{path}: unsupported y4m colourspace C{cs} (8-bit 420/422/444/mono only)")
    return w, h, fps, cw, ch, ("420" if base.startswith("420") else base), nl + 1


def read_y4m(path: str) -> Tuple[np.ndarray, float]:
    """All frames of a YUV4MPEG2 file as RGB uint8 [N, h, w, 3], plus its frame rate."""
    with open(path, "rb") as f:
        data = f.read()
    w, h, fps, cw, ch, _, pos = _y4m_stream_header(data, path)
    fsz = w * h + 2 * cw * ch
    frames = []
    while pos < len(data):
        e = data.index(b"\n", pos)
        if not data[pos:e].startswith(b"FRAME"):
            raise ValueError(f"{path}: corrupt frame header at byte {pos}")
        pos = e + 1
        buf = np.frombuffer(data, np.uint8, fsz, pos)
        pos += fsz
        frames.append(_decode_payload(buf, w, h, cw, ch))
    if not frames:
        return np.zeros((0, h, w, 3), np.uint8), fps
    return np.stack(frames), fps


class Y4MFrames:
    """The frames of a YUV4MPEG2 file, indexed but not decoded (``open_y4m``).  The file is memory-mapped;
    ``payload`` hands out the planar YUV bytes of frames as they lie in the file (what vda_amd.decode's
    kernels take), ``rgb`` / ``np.asarray`` decode on the host as ``read_y4m`` does, so anything that wants
    RGB frames takes this object too.  ``shape`` is that of the RGB frames, ``(N, out_h, out_w, 3)``.

    ``out_h`` / ``out_w`` are the file's ``h`` / ``w`` unless ``open_y4m`` was given a ``max_res`` below the
    frame's longer side: then they are the size ``read_video_frames`` downscales to, ``rgb`` resizes the
    decoded frames as it does (``_resize_rgb``), and ``payload`` still hands out the file's full-size planes
    (vda_yuv_downscale makes the same RGB frames of them on the device)."""

    def __init__(self, path: str, data, offsets, w: int, h: int, cw: int, ch: int, chroma: str,
                 out_h: Optional[int] = None, out_w: Optional[int] = None):
        self.path = path
        self.data = data                              # uint8 view of the whole file
        self.offsets = np.asarray(offsets, np.int64)  # byte offset of each selected frame's payload
        self.w, self.h, self.cw, self.ch = int(w), int(h), int(cw), int(ch)
        self.chroma = chroma                          # "420", "422", "444" or "mono"
        self.payload_bytes = self.w * self.h + 2 * self.cw * self.ch
        self.frame_stride = (self.payload_bytes + 15) // 16 * 16  # frames of a payload block are padded to this
        self.out_h = self.h if out_h is None else int(out_h)  # the size of the RGB frames (max_res)
        self.out_w = self.w if out_w is None else int(out_w)

    @property
    def downscaled(self) -> bool:
        return (self.out_h, self.out_w) != (self.h, self.w)

    @property
    def shape(self) -> tuple:
        return (len(self.offsets), self.out_h, self.out_w, 3)

    def __len__(self) -> int:
        return len(self.offsets)

    def payload(self, indices, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The planar bytes of frames ``indices`` as uint8 [n, frame_stride] (into ``out`` when given); the
        padding bytes of a row are not written."""
        idx = [int(i) for i in indices]
        if out is None:
            out = np.zeros((len(idx), self.frame_stride), np.uint8)
        if out.shape != (len(idx), self.frame_stride) or out.dtype != np.uint8:
            raise ValueError(f"out must be uint8 {(len(idx), self.frame_stride)}, got {out.dtype} {out.shape}")
        n = self.payload_bytes
        for j, i in enumerate(idx):
            o = int(self.offsets[i])
            out[j, :n] = self.data[o:o + n]
        return out

    def rgb(self, indices=None) -> np.ndarray:
        """Frames ``indices`` (default: all) decoded on the host: uint8 [n, out_h, out_w, 3], equal to
        ``read_y4m`` (then ``_resize_rgb`` when the object downscales)."""
        idx = range(len(self)) if indices is None else [int(i) for i in indices]
        out = np.zeros((len(idx), self.out_h, self.out_w, 3), np.uint8)
        for j, i in enumerate(idx):
            o = int(self.offsets[i])
            f = _decode_payload(self.data[o:o + self.payload_bytes], self.w, self.h, self.cw, self.ch)
            out[j] = _resize_rgb(f[None], self.out_h, self.out_w)[0] if self.downscaled else f
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.rgb()
        return a if dtype is None else a.astype(dtype, copy=False)


def open_y4m(path: str, process_length: int = -1, target_fps: float = -1, max_res: int = -1) -> Tuple[Y4MFrames, float]:
    """Index a YUV4MPEG2 file without decoding it: ``(Y4MFrames, fps)`` with ``read_video_frames``' frame
    selection (stride = max(round(source_fps / target_fps), 1), at most ``process_length`` frames).  The
    stream header is parsed and refused as ``read_y4m`` does; the FRAME headers are walked once, since they
    may carry parameters and the payloads are therefore not a fixed stride apart.  With ``max_res`` > 0 and
    a longer side above it, the object's RGB frames have ``read_video_frames``' downscaled size
    (``Y4MFrames.out_h`` / ``out_w``); the payload stays the file's."""
    import mmap
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    w, h, src_fps, cw, ch, chroma, pos = _y4m_stream_header(mm, path, refuse_depth_suffix=True)
    fsz = w * h + 2 * cw * ch
    offsets = []
    size = len(mm)
    while pos < size:
        e = mm.find(b"\n", pos)
        if e < 0 or mm[pos:pos + 5] != b"FRAME":
            raise ValueError(f"{path}: corrupt frame header at byte {pos}")
        pos = e + 1
        if pos + fsz > size:
            raise ValueError(f"{path}: truncated frame at byte {pos} ({size - pos} of {fsz} bytes)")
        offsets.append(pos)
        pos += fsz
    fps = src_fps if target_fps == -1 else target_fps
    idx = list(range(0, len(offsets), max(round(src_fps / fps), 1)))
    if process_length != -1 and process_length < len(idx):
        idx = idx[:process_length]
    data = np.frombuffer(mm, np.uint8)
    out_h, out_w = h, w
    if max_res > 0 and max(h, w) > max_res:
        s = max_res / max(h, w)
        out_h, out_w = ensure_even(round(h * s)), ensure_even(round(w * s))
    return Y4MFrames(path, data, [offsets[i] for i in idx], w, h, cw, ch, chroma, out_h, out_w), fps


def _subsample_420(p: np.ndarray) -> np.ndarray:
    """uint8 [h, w] -> [(h+1)//2, (w+1)//2]: (a + b + c + d + 2) >> 2 over 2x2 blocks (an exact integer
    average, sited between the four samples as C420jpeg is), the last row / column repeated at odd sizes."""
    p = np.pad(p.astype(np.int32), ((0, p.shape[0] % 2), (0, p.shape[1] % 2)), mode="edge")
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _y4m_header(w: int, h: int, fps: float, chroma: str) -> bytes:
    if chroma not in ("444", "420"):
        raise ValueError(f"chroma must be '444' or '420', got {chroma!r}")
    num, den = (int(round(fps * 1001)), 1001) if abs(fps * 1001 - round(fps * 1001)) < 1e-6 else (int(round(fps * 1000)), 1000)
    cs = "C444" if chroma == "444" else "C420jpeg"
    return f"YUV4MPEG2 W{w} H{h} F{num}:{den} Ip A1:1 {cs}\n".encode("ascii")


def write_y4m(path: str, frames: np.ndarray, fps: float, chroma: str = "444"):
    """RGB (or grey) uint8 frames -> YUV4MPEG2, BT.601 limited range: 4:4:4 (C444), or with ``chroma="420"``
    4:2:0 (C420jpeg), the chroma planes averaged over 2x2 blocks (``_subsample_420``)."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = np.repeat(frames[..., None], 3, -1)
    n, h, w, _ = frames.shape
    head = _y4m_header(w, h, fps, chroma)
    with open(path, "wb") as f:
        f.write(head)
        for i in range(n):
            y, u, v = _rgb_to_yuv(frames[i])
            if chroma == "420":
                u, v = _subsample_420(u), _subsample_420(v)
            f.write(b"FRAME\n")
            f.write(y.tobytes())
            f.write(u.tobytes())
            f.write(v.tobytes())


# ---- readers ---------------------------------------------------------------------------------
def _read_pillow(path: str) -> Tuple[np.ndarray, float]:
    from PIL import Image, ImageSequence
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(_IMG_EXT))
        frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names]
        return np.stack(frames), 30.0
    im = Image.open(path)
    frames, dur = [], []
    for fr in ImageSequence.Iterator(im):
        frames.append(np.asarray(fr.convert("RGB")))
        dur.append(fr.info.get("duration", 0) or 0)
    d = float(np.mean(dur)) if dur and np.mean(dur) > 0 else 0.0
    return np.stack(frames), (1000.0 / d if d > 0 else 30.0)


def _resize_rgb(frames: np.ndarray, height: int, width: int) -> np.ndarray:
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(f).resize((width, height), Image.BICUBIC)) for f in frames])


def _read_all(path: str) -> Tuple[np.ndarray, float]:
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        return read_y4m(path)
    if ext == ".npy":
        return np.load(path, allow_pickle=False), 30.0
    if ext == ".npz":
        z = np.load(path, allow_pickle=False)
        fps = float(z["fps"]) if "fps" in z.files else 30.0
        return z["frames"], fps
    return _read_pillow(path)


def read_video_frames(video_path: str, process_length: int, target_fps: float = -1, max_res: int = -1):
    """dc_utils.py:19-69 semantics on the decoders available (module docstring)."""
    ext = os.path.splitext(video_path)[1].lower()
    if ext in (".mp4", ".mov", ".avi", ".mkv", ".webm"):
        try:
            import decord  # noqa: F401
        except ImportError:
            decord = None
        if decord is None:
            raise RuntimeError(f"{video_path}: compressed video needs decord or cv2, neither is installed; "
                               "convert it to .y4m (ffmpeg -i in.mp4 -f yuv4mpegpipe out.y4m) or a frame stack")
        vr = decord.VideoReader(video_path, ctx=decord.cpu(0))
        oh, ow = vr.get_batch([0]).shape[1:3]
        h, w = oh, ow
        if max_res > 0 and max(h, w) > max_res:
            s = max_res / max(oh, ow)
            h, w = ensure_even(round(oh * s)), ensure_even(round(ow * s))
        vr = decord.VideoReader(video_path, ctx=decord.cpu(0), width=w, height=h)
        src_fps = vr.get_avg_fps()
        fps = src_fps if target_fps == -1 else target_fps
        idx = list(range(0, len(vr), max(round(src_fps / fps), 1)))
        if process_length != -1 and process_length < len(idx):
            idx = idx[:process_length]
        return vr.get_batch(idx).asnumpy(), fps
    frames, src_fps = _read_all(video_path)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError(f"{video_path}: expected uint8 frames [N, h, w, 3], got {frames.dtype} {frames.shape}")
    fps = src_fps if target_fps == -1 else target_fps
    idx = list(range(0, len(frames), max(round(src_fps / fps), 1)))
    if process_length != -1 and process_length < len(idx):
        idx = idx[:process_length]
    frames = frames[idx]
    oh, ow = frames.shape[1:3]
    if max_res > 0 and max(oh, ow) > max_res:
        s = max_res / max(oh, ow)
        frames = _resize_rgb(frames, ensure_even(round(oh * s)), ensure_even(round(ow * s)))
    return np.ascontiguousarray(frames), fps


# ---- writers ---------------------------------------------------------------------------------
def colorize_depths(depths: np.ndarray, grayscale: bool = False, spectral: bool = False) -> np.ndarray:
    """dc_utils.py:74-85: clip-wide min/max normalisation to uint8, then inferno / Spectral / grey."""
    d_min, d_max = depths.min(), depths.max()
    norm = ((depths - d_min) / (d_max - d_min) * 255).astype(np.uint8)
    if grayscale:
        return norm
    import matplotlib
    if spectral:
        return (matplotlib.colormaps["Spectral"](norm)[..., :3] * 255).astype(np.uint8)
    table = np.array(matplotlib.colormaps["inferno"].colors)
    return (table[norm] * 255).astype(np.uint8)


def _is_cuda_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and bool(getattr(x, "is_cuda", False))


def _save_depth_video_device(depth, output_video_path: str, fps: float, grayscale: bool, spectral: bool, chroma: str):
    """``save_video`` for depth that lies on the device (vda_amd.visualize): the frames arrive from the
    device as y4m payloads (planar YUV, 4:4:4 or 4:2:0) and are written as they arrive, or as RGB / grey
    frames for Pillow and imageio.  The same bytes as the host path writes for the same depth."""
    from .visualize import colorize_depths_device
    ext = os.path.splitext(output_video_path)[1].lower()
    if ext == ".y4m":
        _, h, w = depth.shape
        head = _y4m_header(w, h, fps, chroma)
        with open(output_video_path, "wb") as f:
            f.write(head)
            for block in colorize_depths_device(depth, grayscale, spectral, layout="planar" + chroma):
                for payload in block:
                    f.write(b"FRAME\n")
                    f.write(payload.tobytes())
        return
    chunks = colorize_depths_device(depth, grayscale, spectral, layout="index" if grayscale else "hwc")
    if ext in (".gif", ".png", ".webp", ".apng"):
        from PIL import Image
        ims = [Image.fromarray(f.copy()) for block in chunks for f in block]
        ims[0].save(output_video_path, save_all=True, append_images=ims[1:], duration=int(round(1000 / fps)), loop=0)
        return
    try:
        import imageio
    except ImportError as e:
        raise RuntimeError(f"{output_video_path}: mp4 output needs imageio + ffmpeg (not installed); use .y4m, .gif, "
                           ".png or .webp") from e
    writer = imageio.get_writer(output_video_path, fps=fps, macro_block_size=1, codec="libx264",
                                ffmpeg_params=["-crf", "18"])
    for block in chunks:
        for f in block:
            writer.append_data(f)
    writer.close()


def save_video(frames: np.ndarray, output_video_path: str, fps: float = 10, is_depths: bool = False,
               grayscale: bool = False, spectral: bool = False, chroma: str = "444"):
    """``frames``: uint8 frames, or with ``is_depths`` float depth [N, h, w]; depth given as a CUDA tensor is
    coloured on the device (``_save_depth_video_device``), numpy input on the host.  ``chroma``: the chroma
    format of a ``.y4m`` output, "444" or "420"."""
    if is_depths and _is_cuda_tensor(frames):
        _save_depth_video_device(frames, output_video_path, fps, grayscale, spectral, chroma)
        return
    vis = colorize_depths(frames, grayscale, spectral) if is_depths else np.asarray(frames)
    ext = os.path.splitext(output_video_path)[1].lower()
    if ext == ".y4m":
        write_y4m(output_video_path, vis, fps, chroma)
        return
    if ext in (".gif", ".png", ".webp", ".apng"):
        from PIL import Image
        ims = [Image.fromarray(f) for f in vis]
        ims[0].save(output_video_path, save_all=True, append_images=ims[1:], duration=int(round(1000 / fps)), loop=0)
        return
    try:
        import imageio
    except ImportError as e:
        raise RuntimeError(f"{output_video_path}: mp4 output needs imageio + ffmpeg (not installed); use .y4m, .gif, "
                           ".png or .webp") from e
    writer = imageio.get_writer(output_video_path, fps=fps, macro_block_size=1, codec="libx264",
                                ffmpeg_params=["-crf", "18"])
    for f in vis:
        writer.append_data(f)
    writer.close()


def save_npz(path: str, depths: np.ndarray):
    np.savez_compressed(path, depths=depths)


def save_tiff(path: str, depths: np.ndarray):
    """float32 multi-page TIFF, one page per frame (run.py:165-166 writes one tifffile stack)."""
    from PIL import Image
    pages = [Image.fromarray(np.ascontiguousarray(d, dtype=np.float32), mode="F") for d in depths]
    pages[0].save(path, save_all=True, append_images=pages[1:])


def load_tiff(path: str) -> np.ndarray:
    from PIL import Image, ImageSequence
    return np.stack([np.asarray(p, dtype=np.float32) for p in ImageSequence.Iterator(Image.open(path))])

