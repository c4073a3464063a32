"""Device-side scale/shift alignment and window stitching, on the CPU (``stitch="device"``).

The orchestration (``DeviceStitcher``, ``_DeviceSink``, the streaming device mode) runs here on the
plain-torch ``TorchAlign`` backend and is compared with the host path (``V.stitch`` /
``stitch="host"``), whose only arithmetic difference is fp32 against fp64 scale/shift sums.  The
libvda entry points are exercised as far as they go without a GPU: argument validation through
ctypes and the Meta shapes of the two torch operators.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, recipe_state_dict, vda_oracle
from vda_amd import _lib
from vda_amd import stream as S
from vda_amd import video as V


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).sum() / np.abs(b).sum())


def random_windows(shape, amp, nwin=5, seed=0):
    """Windows the way a video makes them: one true depth per frame (base * amp), every window sees its
    frames (``window_frame_indices``) through its own scale in [0.5, 1.5] and shift, plus noise."""
    g = np.random.default_rng(seed)
    n = nwin * (V.INFER_LEN - V.OVERLAP) - 10
    assert len(V.window_starts(n)) == nwin
    base = (g.random((n,) + shape, dtype=np.float32) + 0.5) * np.float32(amp)
    wins = []
    for k in range(nwin):
        idx = V.window_frame_indices(k, n)
        scale = np.float32(g.uniform(0.5, 1.5))
        shift = np.float32(g.uniform(-0.2, 0.2) * amp)
        noise = g.standard_normal((V.INFER_LEN,) + shape).astype(np.float32) * np.float32(0.01 * amp)
        wins.append(np.ascontiguousarray(base[idx] * scale + shift + noise))
    return wins, n


def device_stitch(wins, n, order=None, align=V.TorchAlign):
    sink = V._DeviceSink(torch.device("cpu"), n, None, align)
    for k in (order if order is not None else range(len(wins))):
        sink.put(k, torch.from_numpy(wins[k]))
    return sink.result()


@pytest.mark.parametrize("amp", [10, 2000])
@pytest.mark.parametrize("shape", [(6, 7), (48, 64)])
def test_device_stitcher_matches_host_stitch(shape, amp):
    """fp64 sums (device) against fp32 sums (host) is the only difference: emulated on the CPU it
    measured 1.7e-7 .. 9.6e-7 rel-L1 over 6x7 .. 720x1280 and up to 8 windows, so the project's fp32
    tier (1e-5) holds with 10x margin."""
    wins, n = random_windows(shape, amp, seed=shape[0] + amp)
    ref = V.stitch([f for w in wins for f in w], n)
    out = device_stitch(wins, n)
    assert out.shape == ref.shape == (n,) + shape and out.dtype == np.float32
    err = rel(out, ref)
    print(f"device stitch {shape} amp {amp}: rel-L1 vs host {err:.3e}")
    assert err <= 1e-5, err


def test_device_sink_out_of_order_and_missing_window():
    wins, n = random_windows((6, 7), 10, seed=3)
    ref = device_stitch(wins, n)
    out = device_stitch(wins, n, order=(2, 0, 4, 1, 3))
    assert out.shape == ref.shape and np.array_equal(out, ref)
    sink = V._DeviceSink(torch.device("cpu"), n, None, V.TorchAlign)
    for k in (0, 1, 3, 4):
        sink.put(k, torch.from_numpy(wins[k]))
    with pytest.raises(RuntimeError):
        sink.result()


class _UnitAlign(V.TorchAlign):
    """TorchAlign with the scale/shift forced to (1, 0)."""

    @staticmethod
    def scale_shift(pred, target, mask=None):
        return torch.tensor([1.0, 0.0], dtype=torch.float32, device=pred.device)


def test_blend_weights_reproduce_interpolate_frames():
    """With scale = 1, shift = 0 the blended frames are interpolate_frames' bytes: the weights are
    np.float32(1 - w) and np.float32(w) of the same Python floats, three roundings per pixel."""
    g = np.random.default_rng(8)
    n = 40
    wins = [g.random((V.INFER_LEN, 6, 7), dtype=np.float32) * 10 + 1 for _ in range(2)]
    out = device_stitch(wins, n, align=_UnitAlign)
    lo = V.INFER_LEN - V.INTERP_LEN
    pre = list(wins[0][lo:])
    post = list(wins[1][V.OVERLAP - V.INTERP_LEN:V.OVERLAP])
    ref = np.stack(V.interpolate_frames(pre, post))
    assert np.array_equal(out[lo:V.INFER_LEN], ref)
    assert np.array_equal(out[:lo], wins[0][:lo])
    assert np.array_equal(out[V.INFER_LEN:], wins[1][V.OVERLAP:V.OVERLAP + n - V.INFER_LEN])


def test_torch_align_resizes_like_torch_io():
    g = torch.Generator().manual_seed(2)
    d = torch.rand(3, 14, 21, generator=g) * 20 - 5
    r = V.TorchAlign.depth_align(d, (9, 30), clip=False)
    assert torch.equal(r, vda_oracle.TorchIO.resize_depth(d, (9, 30)))
    ss = torch.tensor([1.5, -2.0])
    v = V.TorchAlign.depth_align(d, (9, 30), ss=ss)
    assert torch.equal(v, (r * 1.5 - 2.0).clamp_min(0))
    # degenerate systems return (1, 0) exactly
    ones = torch.ones(50)
    assert V.TorchAlign.scale_shift(ones, torch.rand(50, generator=g)).tolist() == [1.0, 0.0]
    assert V.TorchAlign.scale_shift(d, d, mask=torch.zeros_like(d, dtype=torch.uint8)).tolist() == [1.0, 0.0]


# ---- golden video ---------------------------------------------------------------------------
_FWD = {}


def _memo_forward(sd):
    """The oracle clip forward, each distinct window computed once for all tests of this file."""
    def fwd(x):
        key = hash(x.cpu().numpy().tobytes())
        if key not in _FWD:
            _FWD[key] = vda_oracle.forward(sd, "vits", x.cpu())
        return _FWD[key]
    return fwd


def test_golden_video_device_stitch():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    z = np.load(os.path.join(GOLDEN, "video_vits_57f.npz"), allow_pickle=False)
    frames, depth_ref, meta = z["frames"], z["depth"], json.loads(str(z["meta"]))
    fwd = _memo_forward(recipe_state_dict("vits"))
    kw = dict(input_size=meta["input_size"], device="cpu", io=vda_oracle.TorchIO)
    host, _ = V.infer_video_depth(fwd, frames, meta["fps"], **kw)
    dev, fps = V.infer_video_depth(fwd, frames, meta["fps"], stitch="device", align=V.TorchAlign, **kw)
    assert fps == meta["fps"] and dev.shape == depth_ref.shape and dev.dtype == np.float32
    e_host, e_ref = rel(dev, host), rel(dev, depth_ref)
    print(f"golden video, device stitch: rel-L1 vs host {e_host:.3e}, vs reference {e_ref:.3e}")
    assert e_host <= 1e-5, e_host
    assert e_ref <= 2e-5, e_ref
    t, _ = V.infer_video_depth(fwd, frames, meta["fps"], stitch="device", align=V.TorchAlign, return_device=True, **kw)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), dev)
    with pytest.raises(ValueError):
        V.infer_video_depth(fwd, frames, meta["fps"], return_device=True, **kw)
    with pytest.raises(ValueError):
        V.infer_video_depth(fwd, frames, meta["fps"], stitch="gpu", **kw)


# ---- golden streaming -----------------------------------------------------------------------
class _MemoEngine:
    """Records the engine's answers on the first run and replays them, in call order, on the next:
    host and device mode make the same calls with the same inputs."""

    def __init__(self, eng):
        self.eng, self.log, self.pos = eng, [], None

    def replay(self):
        self.pos = 0

    def _call(self, fn, *a):
        if self.pos is None:
            self.log.append(fn(*a))
            return self.log[-1]
        self.pos += 1
        return self.log[self.pos - 1]

    def motion_features(self, x):
        return self._call(self.eng.motion_features, x)

    def predict(self, *a):
        return self._call(self.eng.predict, *a)


def _stream_golden():
    z = np.load(os.path.join(GOLDEN, "stream_vits_50f.npz"), allow_pickle=False)
    return z["frames"], {k[6:]: z[k] for k in z.files if k.startswith("depth_")}, json.loads(str(z["meta"]))


@pytest.mark.parametrize("case", ["noalign", "kf2_12", "kf4_12_skip", "kf2_12_len16"])
def test_golden_stream_device_mode(case):
    """Device mode against host mode on the streaming goldens (oracle engine, TorchAlign): <= 1e-5;
    without alignment there is nothing to align and the two are the same bytes."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    frames, depths, meta = _stream_golden()
    eng = _MemoEngine(vda_oracle.StreamEngine(recipe_state_dict("vits"), "vits"))
    kw = dict(input_size=meta["input_size"], device="cpu", io=vda_oracle.TorchIO, **meta["cases"][case])
    host, _ = S.infere_single_image(eng, frames, 24, **kw)
    eng.replay()
    dev, fps = S.infere_single_image(eng, frames, 24, stitch="device", align=V.TorchAlign, **kw)
    assert fps == 24 and dev.shape == host.shape == depths[case].shape and dev.dtype == np.float32
    if case == "noalign":
        assert np.array_equal(dev, host)
        return
    err = rel(dev, host)
    print(f"stream {case}, device mode: rel-L1 vs host {err:.3e}, vs reference {rel(dev, depths[case]):.3e}")
    assert err <= 1e-5, err


def test_stream_device_mode_keeps_reference_errors():
    frames, _, meta = _stream_golden()
    eng = vda_oracle.StreamEngine(recipe_state_dict("vits"), "vits")
    kw = dict(input_size=56, device="cpu", io=vda_oracle.TorchIO, stitch="device", align=V.TorchAlign)
    with pytest.raises(IndexError):
        S.infere_single_image(eng, frames[:33], 24, **kw)
    with pytest.raises(NotImplementedError):
        S.infere_single_image(eng, frames[:2], 24, warmup=False, **kw)
    with pytest.raises(ValueError):
        S.infere_single_image(eng, frames[:2], 24, input_size=56, device="cpu", stitch="gpu")


# ---- libvda without a GPU -------------------------------------------------------------------
def test_align_argument_validation():
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    n = 4099
    ws = lib.vda_scale_shift_workspace(n)
    assert ws >= 5 * 8 and lib.vda_scale_shift_workspace(0) == 0
    ok = [fake, fake, None, n, fake, fake, fake, ws, None]
    for null in (0, 1, 5, 6):  # pred, target, ss, ws
        bad = list(ok)
        bad[null] = None
        assert lib.vda_scale_shift(*bad) == -22
        assert b"null pointer" in lib.vda_last_error()
    bad = list(ok)
    bad[3] = 0
    assert lib.vda_scale_shift(*bad) == -22
    assert b"n >= 1" in lib.vda_last_error()
    bad = list(ok)
    bad[7] = ws - 8
    assert lib.vda_scale_shift(*bad) == -22
    assert b"workspace" in lib.vda_last_error()
    w8 = (ctypes.c_float * 33)(*([0.5] * 33))
    ok = [fake, 8, 14, 14, 7, 7, None, 1, None, None, None, fake, None]
    for null in (0, 11):  # src, out
        bad = list(ok)
        bad[null] = None
        assert lib.vda_depth_align(*bad) == -22
        assert b"null pointer" in lib.vda_last_error()
    bad = list(ok)
    bad[1] = 33
    bad[8], bad[9], bad[10] = fake, w8, w8
    assert lib.vda_depth_align(*bad) == -22
    assert b"F <= 32" in lib.vda_last_error()
    bad = list(ok)
    bad[8] = fake  # a blend without its weights
    assert lib.vda_depth_align(*bad) == -22
    bad = list(ok)
    bad[4] = 70000  # output height past the launch grid, as vda_depth_resize
    assert lib.vda_depth_align(*bad) == -22


def test_align_ops_meta_shapes():
    import vda_amd.torch_ops  # noqa: F401
    p = torch.empty(2, 48, 64, device="meta")
    ss, sums = torch.ops.vda.scale_shift(p, p)
    assert ss.shape == (2,) and ss.dtype == torch.float32
    assert sums.shape == (5,) and sums.dtype == torch.float64
    ss, _ = torch.ops.vda.scale_shift(p, p, torch.empty(2, 48, 64, device="meta", dtype=torch.uint8))
    assert ss.shape == (2,)
    src = torch.empty(8, 56, 70, device="meta")
    out = torch.ops.vda.depth_align(src, 48, 64)
    assert out.shape == (8, 48, 64) and out.dtype == torch.float32
    pre = torch.empty(8, 48, 64, device="meta")
    out = torch.ops.vda.depth_align(src, 48, 64, ss, True, pre, [0.5] * 8, [0.5] * 8, pre)
    assert out.shape == (8, 48, 64)
    with pytest.raises(RuntimeError):
        torch.ops.vda.depth_align(torch.empty(33, 56, 70, device="meta"), 48, 64)
    with pytest.raises(NotImplementedError):
        torch.ops.vda.scale_shift(torch.zeros(4), torch.zeros(4))
