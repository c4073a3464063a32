"""Long-video inference: 32-frame windows, clip-parallel sharding, host scale/shift stitching.

Mirrors ``VideoDepthAnything.infer_video_depth`` (video_depth.py:329-417) and its helpers
(utils/util.py:16-73, util/transform.py:5-157):

* frames are resized (lower-bound, keep aspect, multiple of 14, bicubic) and ImageNet-normalised;
* the frame list is padded with copies of the last frame to a multiple of the 22-frame stride
  plus the 10 overlap slots (:351-354);
* window k feeds frames [k*22 .. k*22+31] with slots 0..9 overwritten by the previous window's
  slots KEYFRAMES (:363-364).  That overwrite copies *input frames*, so each window has a closed
  form (``window_frame_indices``) and windows are independent: ``infer_video_depth`` may shard
  them over ranks (one process per GPU, RCCL) with no data-path collective but the final depth
  gather to rank 0;
* rank 0 stitches: least-squares scale/shift on keyframe slots {0, 12}, 8-frame linear blend,
  clip at 0 (:379-413): on the host in the reference's numpy arithmetic (``Stitcher``, the default),
  or with ``stitch="device"`` on the device (``DeviceStitcher`` on vda_scale_shift /
  vda_depth_align), where the windows stay at network resolution until they are aligned.

Preprocessing (bicubic resize + normalise) and the final depth resize run as libvda kernels
(``DeviceIO``).  cv2 is not available here, so the bicubic resize is pinned against torch bicubic
(a=-0.75, the same kernel as cv2.INTER_CUBIC), not cv2 itself.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .video_io import Y4MFrames

INFER_LEN = 32
OVERLAP = 10
KEYFRAMES = [0, 12, 24, 25, 26, 27, 28, 29, 30, 31]
INTERP_LEN = 8
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ---- windowing ------------------------------------------------------------------------------
def padded_length(n_frames: int) -> int:
    """video_depth.py:350-354: pad to a multiple of the stride plus the overlap."""
    step = INFER_LEN - OVERLAP
    return n_frames + (step - (n_frames % step)) % step + (INFER_LEN - step)


def window_starts(n_frames: int) -> List[int]:
    return list(range(0, n_frames, INFER_LEN - OVERLAP))


def window_frame_indices(k: int, n_frames: int) -> List[int]:
    """Original frame index of every slot of window k (closed form of :358-364), clamped to the
    padded list (padding repeats the last frame)."""
    step = INFER_LEN - OVERLAP
    if k == 0:
        idx = list(range(INFER_LEN))
    else:
        prev = window_frame_indices(k - 1, n_frames)
        idx = [prev[j] for j in KEYFRAMES] + [k * step + i for i in range(OVERLAP, INFER_LEN)]
    return [min(i, n_frames - 1) for i in idx]


# ---- preprocessing (util/transform.py:5-157, video_depth.py:330-348) ------------------------
def _constrain(x, multiple, min_val=0, max_val=None):
    y = int(np.round(x / multiple) * multiple)
    if max_val is not None and y > max_val:
        y = int(np.floor(x / multiple) * multiple)
    if y < min_val:
        y = int(np.ceil(x / multiple) * multiple)
    return y


def net_input_size(height: int, width: int, input_size: int = 518) -> tuple:
    """(H, W) the network sees: aspect > 1.78 shrinks input_size (:330-334); Resize lower_bound,
    keep_aspect_ratio, ensure_multiple_of=14 (transform.py:57-110)."""
    ratio = max(height, width) / min(height, width)
    if ratio > 1.78:
        input_size = int(input_size * 1.777 / ratio)
        input_size = round(input_size / 14) * 14
    sh, sw = input_size / height, input_size / width
    if sw > sh:
        sh = sw
    else:
        sw = sh
    return (_constrain(sh * height, 14, min_val=input_size), _constrain(sw * width, 14, min_val=input_size))


class DeviceIO:
    """The per-frame data formats either side of the forward, on libvda kernels:
    ``preprocess`` uint8 frames [N, h, w, 3] (on the device) -> normalised input [N, 3, H, W] fp32
    (bicubic resize + ImageNet normalise, vda_preprocess_frames); ``resize_depth`` depth [N, H, W]
    -> [N, h, w] fp32 (bilinear align_corners=True, vda_depth_resize).  The drivers take any object
    with these two methods (the tests pass the oracle's torch-CPU restatement, ``TorchIO``)."""

    @staticmethod
    def preprocess(frames: torch.Tensor, size: tuple) -> torch.Tensor:
        from . import ops
        return ops.preprocess_frames(frames, int(size[0]), int(size[1]), MEAN, STD)

    @staticmethod
    def preprocess_planar(payload: torch.Tensor, frames, size: tuple) -> torch.Tensor:
        """``preprocess`` from the planar YUV bytes of the frames (``payload`` [N, frame_stride] uint8 on the
        device, rows as ``frames``, a ``video_io.Y4MFrames``, hands them out): vda_preprocess_yuv, the bits
        ``preprocess`` gives for the host-decoded frames.  Frames opened with a ``max_res`` that downscales them
        go through vda_yuv_downscale first (the RGB frames ``frames.rgb()`` gives, on the device), then
        ``preprocess``."""
        from . import ops
        if (frames.out_h, frames.out_w) == (frames.h, frames.w):
            return ops.preprocess_yuv(payload, frames.h, frames.w, frames.chroma, int(size[0]), int(size[1]), MEAN, STD)
        rgb = ops.yuv_downscale(payload, frames.h, frames.w, frames.chroma, frames.out_h, frames.out_w)
        return ops.preprocess_frames(rgb, int(size[0]), int(size[1]), MEAN, STD)

    @staticmethod
    def resize_depth(depth: torch.Tensor, size: tuple) -> torch.Tensor:
        from . import ops
        return ops.depth_resize(depth.float().contiguous(), int(size[0]), int(size[1]))


class DeviceAlign:
    """The alignment arithmetic of the device stitcher (``stitch="device"``) on libvda kernels:
    ``scale_shift(pred, target, mask=None)`` -> ss [2] fp32 on the device (least squares with fp64
    sums, vda_scale_shift) and ``depth_align(src[F, H, W], size, ss=None, clip=True, pre=None,
    w_pre=None, w_post=None, out=None)`` -> [F, h, w] (resize, ``* scale + shift``, clip at 0, blend
    into ``pre``; vda_depth_align).  Neither reads a value back to the host.  The drivers take any
    object with these two methods, as they take ``io=`` (``TorchAlign`` runs on any device)."""

    @staticmethod
    def scale_shift(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        from . import ops
        return ops.scale_shift(pred, target, mask=mask)[0]

    @staticmethod
    def depth_align(src: torch.Tensor, size: tuple, ss=None, clip: bool = True, pre=None, w_pre=None, w_post=None,
                    out=None) -> torch.Tensor:
        from . import ops
        return ops.depth_align(src.float().contiguous(), int(size[0]), int(size[1]), ss=ss, clip=clip, pre=pre,
                               w_pre=w_pre, w_post=w_post, out=out)


class TorchAlign:
    """``DeviceAlign``'s contract in plain torch on any device: fp64 sums, ``F.interpolate(...,
    align_corners=True)``, multiply and add as separate (separately rounded) ops.  It lets the device
    stitcher's orchestration run on the CPU; it is not a fallback of the product path."""

    @staticmethod
    def scale_shift(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        p, t = pred.reshape(-1).double(), target.reshape(-1).double()
        m = torch.ones_like(p) if mask is None else mask.reshape(-1).double()
        a00, a01, a11 = (m * p * p).sum(), (m * p).sum(), m.sum()
        b0, b1 = (m * p * t).sum(), (m * t).sum()
        det = a00 * a11 - a01 * a01
        ok = det != 0
        den = torch.where(ok, det, torch.ones_like(det))
        x0 = torch.where(ok, (a11 * b0 - a01 * b1) / den, torch.ones_like(det))
        x1 = torch.where(ok, (-a01 * b0 + a00 * b1) / den, torch.zeros_like(det))
        return torch.stack([x0, x1]).float()

    @staticmethod
    def depth_align(src: torch.Tensor, size: tuple, ss=None, clip: bool = True, pre=None, w_pre=None, w_post=None,
                    out=None) -> torch.Tensor:
        import torch.nn.functional as F
        v = F.interpolate(src.float().unsqueeze(1), size=(int(size[0]), int(size[1])), mode="bilinear",
                          align_corners=True)[:, 0]
        if ss is not None:
            v = v * ss[0]
            v = v + ss[1]
        if clip:
            v = torch.where(v < 0, torch.zeros_like(v), v)
        if pre is not None:
            w0 = torch.tensor([float(x) for x in w_pre], dtype=torch.float32, device=v.device).view(-1, 1, 1)
            w1 = torch.tensor([float(x) for x in w_post], dtype=torch.float32, device=v.device).view(-1, 1, 1)
            a = pre * w0
            b = v * w1
            v = a + b
        if out is None:
            return v
        out.copy_(v)
        return out


# ---- stitching (video_depth.py:375-413, utils/util.py:40-73) --------------------------------
def compute_scale_and_shift(prediction, target, mask):
    prediction = prediction.astype(np.float32)
    target = target.astype(np.float32)
    mask = mask.astype(np.float32)
    a_00 = np.sum(mask * prediction * prediction)
    a_01 = np.sum(mask * prediction)
    a_11 = np.sum(mask)
    b_0 = np.sum(mask * prediction * target)
    b_1 = np.sum(mask * target)
    x_0, x_1 = 1, 0
    det = a_00 * a_11 - a_01 * a_01
    if det != 0:
        x_0 = (a_11 * b_0 - a_01 * b_1) / det
        x_1 = (-a_01 * b_0 + a_00 * b_1) / det
    return x_0, x_1


def blend_weights(n: int) -> List[float]:
    """get_interpolate_frames' weight of the post frame (utils/util.py:65-73), as Python floats."""
    step = 1.0 / (n - 1)
    return [0.0] + [i * step for i in range(1, n - 1)] + [1.0]


def interpolate_frames(pre: Sequence[np.ndarray], post: Sequence[np.ndarray]) -> List[np.ndarray]:
    n = len(pre)
    w = blend_weights(n)
    return [pre[i] * (1 - w[i]) + post[i] * w[i] for i in range(n)]


class Stitcher:
    """The reference's stitch loop (video_depth.py:379-413) taken one window at a time, so the host
    aligns window k while the GPU computes window k + 1.  ``add`` takes the windows in order.  Only
    the last INTERP_LEN aligned frames can still change (the next window blends into them), so every
    earlier one is written straight into the preallocated [n_frames, h, w] result as it settles."""

    def __init__(self, n_frames: int):
        self.n = int(n_frames)
        self.out: Optional[np.ndarray] = None
        self.done = 0
        self.aligned: List[np.ndarray] = []
        self.ref_align: List[np.ndarray] = []

    def _flush(self, keep: int):
        if self.out is None:
            self.out = np.empty((self.n,) + self.aligned[0].shape, dtype=self.aligned[0].dtype)
        while len(self.aligned) > keep and self.done < self.n:
            self.out[self.done] = self.aligned.pop(0)
            self.done += 1

    def add(self, win: Sequence[np.ndarray]):
        align_len = OVERLAP - INTERP_LEN
        kf_align = KEYFRAMES[:align_len]
        if not self.aligned:
            self.aligned += list(win[:INFER_LEN])
            for kf in kf_align:
                self.ref_align.append(win[kf])
            self._flush(INTERP_LEN)
            return
        cur = [win[i] for i in range(len(kf_align))]
        scale, shift = compute_scale_and_shift(np.concatenate(cur), np.concatenate(self.ref_align),
                                               np.concatenate(np.ones_like(self.ref_align) == 1))
        pre = self.aligned[-INTERP_LEN:]
        post = list(win[align_len:OVERLAP])
        for i in range(len(post)):
            post[i] = post[i] * scale + shift
            post[i][post[i] < 0] = 0
        self.aligned[-INTERP_LEN:] = interpolate_frames(pre, post)
        for i in range(OVERLAP, INFER_LEN):
            d = win[i] * scale + shift
            d[d < 0] = 0
            self.aligned.append(d)
        self.ref_align = self.ref_align[:1]
        for kf in kf_align[1:]:
            d = win[kf] * scale + shift
            d[d < 0] = 0
            self.ref_align.append(d)
        self._flush(INTERP_LEN)

    def result(self) -> np.ndarray:
        self._flush(0)
        return self.out[:self.done]


def stitch(depth_list: List[np.ndarray], n_frames: int) -> np.ndarray:
    """depth_list: per-window depth frames concatenated (32 per window) -> [n_frames, h, w]."""
    st = Stitcher(n_frames)
    for fid in range(0, len(depth_list), INFER_LEN):
        st.add(depth_list[fid:fid + INFER_LEN])
    return st.result()


class DeviceStitcher:
    """``Stitcher`` restated on tensors that stay where the windows are (``stitch="device"``).  ``add``
    takes each window at NETWORK resolution [32, H, W], in order, and returns the frames that have
    settled as a tuple of [m, h, w] blocks; ``size`` = (h, w) is the output size (None: the windows'
    own).  State: ``ref_align`` [2, h, w] and the INTERP_LEN still-blendable tail frames.  A window
    k >= 1 costs two small launches (resize slots 0-1, their scale/shift against ``ref_align``) and two
    passes that resize, align, clip and blend (slots 2-9 into the tail in place, slots 10-31); the
    resized, unaligned window never exists in memory, no scalar is read back and nothing waits on the
    host.  The scale/shift sums are fp64 here and fp32 on the host path."""

    def __init__(self, n_frames: int, align=DeviceAlign, size: Optional[tuple] = None):
        self.n = int(n_frames)
        self.align = align
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.ref_align: Optional[torch.Tensor] = None
        self.tail: Optional[torch.Tensor] = None
        w = blend_weights(INTERP_LEN)  # the Python floats interpolate_frames multiplies float32 frames by
        self.w_pre = [float(np.float32(1 - x)) for x in w]
        self.w_post = [float(np.float32(x)) for x in w]

    def state(self) -> tuple:
        return tuple(t for t in (self.ref_align, self.tail) if t is not None)

    def add(self, win: torch.Tensor) -> tuple:
        size = self.size or (int(win.shape[-2]), int(win.shape[-1]))
        align_len = OVERLAP - INTERP_LEN
        kf_align = KEYFRAMES[:align_len]
        al = self.align
        if self.tail is None:
            r = al.depth_align(win[:INFER_LEN], size, clip=False)
            self.ref_align = torch.stack([r[kf] for kf in kf_align], 0)
            self.tail = r[INFER_LEN - INTERP_LEN:]
            return (r[:INFER_LEN - INTERP_LEN],)
        cur = al.depth_align(win[:align_len], size, clip=False)
        ss = al.scale_shift(cur, self.ref_align)
        settled = al.depth_align(win[align_len:OVERLAP], size, ss=ss, clip=True, pre=self.tail, w_pre=self.w_pre,
                                 w_post=self.w_post, out=self.tail)
        new = al.depth_align(win[OVERLAP:INFER_LEN], size, ss=ss, clip=True)
        for j, kf in enumerate(kf_align):
            if j >= 1:  # slot 0's reference stays window 0's (video_depth.py:409-413)
                self.ref_align[j].copy_(new[kf - OVERLAP])
        self.tail = new[new.shape[0] - INTERP_LEN:]
        return (settled, new[:new.shape[0] - INTERP_LEN])

    def finish(self) -> tuple:
        tail, self.tail = self.tail, None
        return () if tail is None else (tail,)


# ---- driver ---------------------------------------------------------------------------------
class _DeviceSink:
    """``_HostSink``'s contract (``put`` windows in any order, ``result`` raises on a missing one) for
    ``stitch="device"``: the windows arrive at network resolution and are stitched where they are
    (``DeviceStitcher``).  The settled frames go either into a preallocated device [n, h, w] tensor
    (``return_device``) or to the host through a ring of two pinned staging buffers with non-blocking
    copies, 22 frames per window (the host path moves all 32), so device memory stays flat in the
    video length.  Windows may be put under different streams: a step waits for the event of the
    previous one, and every buffer that outlives a step is ``record_stream``-ed on the stream that
    uses it (the discipline ``land`` in ``infer_video_depth`` documents for side-stream buffers)."""

    def __init__(self, device: torch.device, n_frames: int, size: Optional[tuple] = None, align=DeviceAlign,
                 return_device: bool = False):
        self.dev = device
        self.gpu = device.type == "cuda"
        self.n = int(n_frames)
        self.return_device = bool(return_device)
        self.stitcher = DeviceStitcher(n_frames, align, size)
        self.ready = {}          # window id -> (window, event or None): landed, not yet stitchable
        self.next = 0
        self.done = 0
        self.out: Optional[torch.Tensor] = None    # device result (return_device, or a CPU run)
        self.host: Optional[np.ndarray] = None     # host result (GPU run with host output)
        self.ring: list = []
        self.pending: list = []  # (first frame, frame count, staging slot, event)
        self.last = None         # event after the latest stitch step

    def _drain(self, keep: int):
        while len(self.pending) > keep:
            pos, m, slot, ev = self.pending.pop(0)
            ev.synchronize()
            self.host[pos:pos + m] = slot[:m].numpy()

    def _emit(self, blocks: Sequence[torch.Tensor]):
        m = min(sum(int(b.shape[0]) for b in blocks), self.n - self.done)
        if m <= 0:
            return
        shape = tuple(blocks[0].shape[1:])
        if self.return_device or not self.gpu:
            if self.out is None:
                self.out = torch.empty((self.n,) + shape, dtype=torch.float32, device=self.dev)
            dst = self.out[self.done:self.done + m]
            if self.gpu:
                self.out.record_stream(torch.cuda.current_stream(self.dev))
        else:
            if self.host is None:
                self.host = np.empty((self.n,) + shape, dtype=np.float32)
            self._drain(1)
            busy = {id(s) for _, _, s, _ in self.pending}
            cap = (INFER_LEN - INTERP_LEN,) + shape
            dst = next((s for s in self.ring if id(s) not in busy and tuple(s.shape) == cap), None)
            if dst is None:
                dst = torch.empty(cap, dtype=torch.float32, pin_memory=True)
                self.ring.append(dst)
                self.ring = self.ring[-2:]
        at = 0
        for b in blocks:
            c = min(int(b.shape[0]), m - at)
            if c > 0:
                dst[at:at + c].copy_(b[:c], non_blocking=True)
            at += c
        if self.gpu and not self.return_device:
            ev = torch.cuda.Event()
            ev.record()
            self.pending.append((self.done, m, dst, ev))
        self.done += m

    def _on_current_stream(self, extra=()):
        """Order the current stream behind the previous stitch step and tell the caching allocator that
        it uses the buffers that step left (they may have been allocated under another stream)."""
        if not self.gpu:
            return
        cur = torch.cuda.current_stream(self.dev)
        if self.last is not None:
            cur.wait_event(self.last)
        for t in self.stitcher.state() + tuple(extra):
            if t.is_cuda:
                t.record_stream(cur)

    def _stitch(self, d: torch.Tensor, ev):
        if self.gpu and ev is not None:
            torch.cuda.current_stream(self.dev).wait_event(ev)
        self._on_current_stream((d,))
        self._emit(self.stitcher.add(d))
        if self.gpu:
            self.last = torch.cuda.Event()
            self.last.record()

    def put(self, k: int, d: torch.Tensor):
        d = d.detach()
        if d.dtype != torch.float32 or not d.is_contiguous():
            d = d.float().contiguous()
        ev = None
        if self.gpu:
            ev = torch.cuda.Event()
            ev.record()  # d is complete once the stream it was produced (or received) on reaches this
        self.ready[k] = (d, ev)
        while self.next in self.ready:
            self._stitch(*self.ready.pop(self.next))
            self.next += 1

    def result(self):
        if self.ready:
            raise RuntimeError(f"windows {sorted(self.ready)} never became stitchable (missing {self.next})")
        self._on_current_stream()
        self._emit(self.stitcher.finish())
        if self.return_device:
            return self.out[:self.done]
        if not self.gpu:
            return self.out[:self.done].numpy()
        self._drain(0)
        return self.host[:self.done]


class _HostSink:
    """Moves each window's resized depth [32, h, w] off the device as soon as it exists (as the
    reference does, video_depth.py:372-373), so device memory stays flat in the video length, and
    stitches the windows in order as they land.  On a GPU the copies go through a ring of two
    pinned staging buffers with non-blocking D2H copies: window k is copied out and stitched on the
    host while the device runs window k + 1's forward."""

    def __init__(self, device: torch.device, n_frames: int):
        self.gpu = device.type == "cuda"
        self.ring: list = []
        self.pending: list = []  # (window id, staging slot, event)
        self.ready = {}          # landed windows not yet stitched (multi-rank rounds arrive out of order)
        self.next = 0
        self.stitcher = Stitcher(n_frames)

    def _land(self, k: int, a: np.ndarray):
        self.ready[k] = a
        while self.next in self.ready:
            self.stitcher.add(list(self.ready.pop(self.next)))
            self.next += 1

    def _drain(self, keep: int):
        while len(self.pending) > keep:
            k, slot, ev = self.pending.pop(0)
            ev.synchronize()
            self._land(k, slot.numpy().copy())

    def put(self, k: int, d: torch.Tensor):
        if not self.gpu:
            self._land(k, d.detach().to("cpu", torch.float32).numpy().copy())
            return
        self._drain(1)  # slot (len(pending) % 2) is free after this
        busy = {id(s) for _, s, _ in self.pending}
        slot = next((s for s in self.ring if id(s) not in busy and s.shape == d.shape), None)
        if slot is None:
            slot = torch.empty(d.shape, dtype=torch.float32, pin_memory=True)
            self.ring.append(slot)
            self.ring = self.ring[-2:]
        slot.copy_(d, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((k, slot, ev))

    def result(self) -> np.ndarray:
        self._drain(0)
        if self.ready:
            raise RuntimeError(f"windows {sorted(self.ready)} never became stitchable (missing {self.next})")
        return self.stitcher.result()


class _HostSource:
    """Uploads a window batch's frames: gathered on the host into one of two pinned staging
    buffers, then copied with a non-blocking H2D (a pageable copy would hold the host until the
    device had drained the previous window, leaving the GPU idle while the next forward is
    launched).  A slot is reused only after its previous copy has completed."""

    def __init__(self, frames: torch.Tensor, device: torch.device):
        self.frames, self.dev = frames, device
        self.gpu = device.type == "cuda"
        self.slots: list = []  # [pinned tensor, event or None]
        self.row = tuple(frames.shape[1:])
        self.dtype = frames.dtype

    def _gather(self, idx: List[int], out: torch.Tensor):
        torch.index_select(self.frames, 0, torch.as_tensor(idx, dtype=torch.long), out=out)

    def get(self, idx: List[int]) -> torch.Tensor:
        if not self.gpu or self.frames.device.type != "cpu":  # CPU run, or frames already on a device
            ix = torch.as_tensor(idx, dtype=torch.long)
            return self.frames[ix.to(self.frames.device)].to(self.dev)
        return self._upload(idx)

    def _upload(self, idx: List[int]) -> torch.Tensor:
        shape = (len(idx),) + self.row
        slot = next((s for s in self.slots if tuple(s[0].shape) == shape and (s[1] is None or s[1].query())), None)
        if slot is None:
            if len(self.slots) >= 2:
                slot = self.slots.pop(0)
                slot[1].synchronize()
                if tuple(slot[0].shape) != shape:
                    slot[0] = torch.empty(shape, dtype=self.dtype, pin_memory=True)
            else:
                slot = [torch.empty(shape, dtype=self.dtype, pin_memory=True), None]
            self.slots.append(slot)
        self._gather(idx, slot[0])
        x = slot[0].to(self.dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return x


class _PlanarSource(_HostSource):
    """``_HostSource`` for a ``video_io.Y4MFrames`` on a GPU run: a window batch's frames are copied out of the
    memory-mapped file as planar YUV rows [n, frame_stride] (1.5 bytes per pixel at 4:2:0, never decoded on the
    host) into the pinned staging buffers and uploaded non-blocking."""

    def __init__(self, frames, device: torch.device):
        self.frames, self.dev = frames, device
        self.gpu = True
        self.slots = []
        self.row = (int(frames.frame_stride),)
        self.dtype = torch.uint8

    def _gather(self, idx: List[int], out: torch.Tensor):
        self.frames.payload(idx, out=out.numpy())

    def get(self, idx: List[int]) -> torch.Tensor:
        return self._upload(idx)


def _gather_round(buf: torch.Tensor, rank: int, world: int, group):
    """Start gathering one round's per-rank window buffers [n, 32, h, w] to rank 0 (RCCL on GPU
    tensors, issued on the current stream; gloo takes host copies).  Returns (the list of world
    receive buffers on rank 0 or None, the async work, the send buffer to keep alive)."""
    import torch.distributed as dist
    cpu = dist.get_backend(group) == "gloo"
    src = buf.cpu() if cpu else buf
    bufs = [torch.empty_like(src) for _ in range(world)] if rank == 0 else None
    work = dist.gather(src, bufs, dst=0, group=group, async_op=True)
    return bufs, work, src


def infer_video_depth(forward: Callable[[torch.Tensor], torch.Tensor], frames, target_fps, input_size: int = 518,
                      device="cuda", windows_per_batch: int = 1, rank: int = 0, world: int = 1, group=None,
                      io=DeviceIO, streams: int = 2, prepare: Optional[Callable[[tuple], None]] = None,
                      stitch: str = "host", return_device: bool = False, align=DeviceAlign):
    """Depth for every frame of ``frames`` (uint8 [N, h, w, 3] numpy or tensor, or a ``video_io.Y4MFrames``:
    on a GPU with an ``io`` that has ``preprocess_planar`` its frames are uploaded as the planar YUV bytes of the
    file and decoded by the preprocessing kernel, otherwise they are decoded on the host first; the depth is the
    same bit for bit.  Frames opened with a ``max_res`` that downscales them are downscaled on the device too,
    unless ``ops.yuv_downscale_accepts`` refuses the ratio: then they are decoded and resized on the host).

    ``forward(x[B, 32, 3, H, W]) -> depth[B, 32, H, W]`` is the clip forward (the model, or any
    callable); ``prepare((H, W))``, when given, builds whatever state the forward creates lazily
    (packed weights, the resolution's token bias) on the current stream before any side stream runs
    a forward.  With world > 1, window k runs on rank k % world: round r is windows
    r*world .. r*world + world - 1, one per rank, and each round's (or each ``windows_per_batch``
    rounds') depth maps are gathered to rank 0 by an asynchronous collective, so no rank ever holds
    more than two batches of windows on the device.  Rank 0 hands round r's windows to the host
    stitcher only after round r + 1's forward and gather are enqueued, so the host work never sits
    between two collectives; rank 0 returns (depth, fps), others (None, fps).

    ``streams`` > 1 (GPU): consecutive window batches go round-robin onto that many HIP streams, so
    one window's forward can start while the previous one's tail kernels run (one GPU, two streams:
    the 176-frame ViT-L job in 414-420 ms against 442 ms on one stream and 413 ms for its 8 forwards
    back to back; ``tools/archive/video_probe.py``).  Each rank of a multi-GPU job does the same.

    ``stitch="device"`` keeps the windows on the device: the per-window ``io.resize_depth`` is skipped,
    the multi-rank gather carries network-resolution windows, and rank 0 resizes while it aligns
    (``DeviceStitcher`` on the ``align`` backend; fp64 scale/shift sums where the host path sums in
    fp32, so the two modes agree to the fp32 tier, not bit for bit).  ``return_device=True`` (device
    mode only) returns the depth as a [N, h, w] fp32 tensor on ``device`` instead of a numpy array.
    """
    if stitch not in ("host", "device"):
        raise ValueError(f"stitch must be 'host' or 'device', got {stitch!r}")
    if return_device and stitch != "device":
        raise ValueError("return_device=True needs stitch='device' (the host stitcher returns numpy)")
    dev = torch.device(device)
    planar = None
    if isinstance(frames, Y4MFrames):
        use_planar = dev.type == "cuda" and callable(getattr(io, "preprocess_planar", None))
        if use_planar and frames.downscaled:
            from . import ops
            use_planar = ops.yuv_downscale_accepts(frames.h, frames.w, frames.out_h, frames.out_w)
        if use_planar:
            planar = frames          # the window batches upload the file's YUV bytes
        else:                        # a CPU run, an io without the planar kernel, or a ratio beyond the downscale
            frames = frames.rgb()    # kernel: decode (and downscale) on the host
    if planar is None and not isinstance(frames, torch.Tensor):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    n = frames.shape[0]
    h, w = int(frames.shape[1]), int(frames.shape[2])
    size = net_input_size(h, w, input_size)
    nwin = len(window_starts(n))
    rounds = (nwin + world - 1) // world
    on_device = stitch == "device"
    out_hw = size if on_device else (h, w)  # the size a window has when it reaches the sink / the gather
    sink = None
    if rank == 0:
        sink = _DeviceSink(dev, n, (h, w), align, return_device) if on_device else _HostSink(dev, n)
    source = _HostSource(frames, dev) if planar is None else _PlanarSource(planar, dev)
    wpb = max(1, int(windows_per_batch))
    if prepare is None and callable(getattr(forward, "prepare", None)):  # the model itself as the forward
        prepare = lambda hw: forward.prepare(dev, hw)  # noqa: E731
    if prepare is not None:
        prepare(size)
    strs = []
    if dev.type == "cuda" and int(streams) > 1:
        strs = [torch.cuda.Stream(device=dev) for _ in range(int(streams))]
        for st in strs:  # after prepare(): the side streams see the packed weights / token bias
            st.wait_stream(torch.cuda.current_stream(dev))
    pending = None  # previous round's (receive buffers, rounds, work, send buffer)

    def land(pend):
        bufs, rr_, work, _ = pend
        work.wait()  # the current stream (or, on gloo, the host) waits for the gather
        if rank == 0:
            if strs:
                # the receive buffers were allocated on a side stream, but the sink's D2H copies run on
                # the current one: without this the caching allocator could hand their blocks to that
                # side stream's next forward while the copies are still queued
                cur_st = torch.cuda.current_stream(dev)
                for b in bufs:
                    if b.is_cuda:
                        b.record_stream(cur_st)
            for src in range(world):
                for j, r in enumerate(rr_):
                    k = r * world + src
                    if k < nwin:
                        sink.put(k, bufs[src][j])

    for bi, r0 in enumerate(range(0, rounds, wpb)):
        rr = list(range(r0, min(rounds, r0 + wpb)))
        ks = [r * world + rank for r in rr if r * world + rank < nwin]
        d = None
        with (torch.cuda.stream(strs[bi % len(strs)]) if strs else contextlib.nullcontext()):
            if ks:
                idx = [window_frame_indices(k, n) for k in ks]
                uniq = sorted(set(i for row in idx for i in row))
                pre = (io.preprocess(source.get(uniq), size) if planar is None
                       else io.preprocess_planar(source.get(uniq), planar, size))
                pos = {f: j for j, f in enumerate(uniq)}
                x = torch.stack([pre[[pos[i] for i in row]] for row in idx], 0)
                del pre
                with torch.no_grad():
                    d = forward(x).float()  # [B, 32, H, W]
                del x
                if on_device:
                    d = d.contiguous()
                else:
                    d = io.resize_depth(d.flatten(0, 1), (h, w)).view(len(ks), INFER_LEN, h, w)
            if world == 1:
                for j, k in enumerate(ks):
                    sink.put(k, d[j])
                continue
            # every rank takes part in every round's gather (a rank without a window sends zeros),
            # enqueued behind this round's forward on its stream
            buf = torch.zeros(len(rr), INFER_LEN, out_hw[0], out_hw[1], dtype=torch.float32, device=dev)
            if d is not None:
                buf[:len(ks)] = d
            cur = _gather_round(buf, rank, world, group) + (rr,)
        if pending is not None:
            land(pending)
        pending = (cur[0], cur[3], cur[1], cur[2])
    if pending is not None:
        land(pending)
    if rank != 0:
        return None, target_fps
    return sink.result(), target_fps
