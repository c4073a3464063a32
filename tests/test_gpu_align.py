"""vda_scale_shift / vda_depth_align and the device stitch mode on the GPU (``stitch="device"``).

The kernels are pinned exactly where that is possible: the fp64 sums against numpy fp64, the fp32
(scale, shift) against the fp32 rounding of the fp64 closed form, the fused resize + affine + clip +
blend bit for bit against ``ops.depth_resize`` followed by separate torch ops.  The drivers run the
golden videos in device mode against the reference goldens and against host mode.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, device_at_offset as offset_by_one, recipe_state_dict
from vda_amd import _lib
from vda_amd import video as V

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).sum() / np.abs(b).sum())


def closed_form(sums):
    a00, a01, a11, b0, b1 = (float(v) for v in sums)
    det = a00 * a11 - a01 * a01
    if det == 0:
        return np.float32(1), np.float32(0)
    return np.float32((a11 * b0 - a01 * b1) / det), np.float32((-a01 * b0 + a00 * b1) / det)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def raw_scale_shift(pred, target, mask, n):
    """vda_scale_shift through the C ABI with NaN canaries behind ss and sums."""
    lib = _lib.lib()
    ss = torch.full((6,), float("nan"), dtype=torch.float32, device="cuda")
    sums = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    wsb = lib.vda_scale_shift_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = lib.vda_scale_shift(pred.data_ptr(), target.data_ptr(), None if mask is None else mask.data_ptr(), n,
                             sums.data_ptr(), ss.data_ptr(), ws.data_ptr(), wsb,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.vda_last_error()
    torch.cuda.synchronize()
    return ss.cpu(), sums.cpu()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 257, 4099, 2 * 48 * 64, 2 * 270 * 480])
def test_scale_shift_kernel(n, masked):
    from vda_amd import ops
    g = np.random.default_rng(n + masked)
    p = (g.random(n) * 10 + 1).astype(np.float32)
    t = (p * 1.3 - 0.7 + g.standard_normal(n) * 0.05).astype(np.float32)
    m = g.integers(0, 2, n).astype(np.uint8) if masked else None
    dp, dt = offset_by_one(p), offset_by_one(t)
    dm = offset_by_one(m) if masked else None
    assert dp.data_ptr() % 16 == 4
    ss, sums = ops.scale_shift(dp, dt, mask=dm)
    ss2, sums2 = ops.scale_shift(dp, dt, mask=dm)
    assert ss.shape == (2,) and ss.dtype == torch.float32 and sums.shape == (5,) and sums.dtype == torch.float64
    assert torch.equal(ss.view(torch.int32), ss2.view(torch.int32))      # deterministic: the same bits
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    P, T = p.astype(np.float64), t.astype(np.float64)
    M = np.ones(n) if m is None else m.astype(np.float64)
    ref = np.array([np.sum(M * P * P), np.sum(M * P), np.sum(M), np.sum(M * P * T), np.sum(M * T)])
    np.testing.assert_allclose(sums.cpu().numpy(), ref, rtol=1e-12, atol=0)
    x0, x1 = closed_form(ref)
    got = ss.cpu().numpy()
    print(f"n {n} masked {masked}: ss {got}, closed form ({x0}, {x1})")
    assert ulps(got[0], x0) <= 1 and ulps(got[1], x1) <= 1
    # the C ABI writes ss [2] and sums [5] and nothing behind them
    rss, rsums = raw_scale_shift(dp, dt, dm, n)
    assert torch.equal(rss[:2].view(torch.int32), ss.cpu().view(torch.int32))
    assert torch.equal(rsums[:5].view(torch.int64), sums.cpu().view(torch.int64))
    assert torch.isnan(rss[2:]).all() and torch.isnan(rsums[5:]).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_scale_shift_every_head_and_tail(off, masked):
    """pred starts ``off`` elements past a 16-byte boundary (heads of 0, 3, 2, 1 elements), with runs shorter
    than a head, shorter than one 16-byte group, and with every tail length."""
    from vda_amd import ops
    for n in (1, 2, 3, 4, 5, 7, 8, 1030):
        g = np.random.default_rng(100 * n + 2 * off + masked)
        p = (g.random(n) * 10 + 1).astype(np.float32)
        t = (p * 1.3 - 0.7 + g.standard_normal(n) * 0.05).astype(np.float32)
        m = g.integers(0, 2, n).astype(np.uint8) if masked else None
        dp, dt = offset_by_one(p, off), offset_by_one(t, off)
        dm = offset_by_one(m, off) if masked else None
        assert dp.data_ptr() % 16 == 4 * off
        _, sums = ops.scale_shift(dp, dt, mask=dm)
        P, T = p.astype(np.float64), t.astype(np.float64)
        M = np.ones(n) if m is None else m.astype(np.float64)
        ref = np.array([np.sum(M * P * P), np.sum(M * P), np.sum(M), np.sum(M * P * T), np.sum(M * T)])
        got = sums.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=f"n {n}")
        assert got[2] == ref[2], (n, got[2], ref[2])  # the count: exact


def test_scale_shift_degenerate_systems_return_identity():
    from vda_amd import ops
    g = np.random.default_rng(1)
    n = 4099
    t = offset_by_one(g.random(n).astype(np.float32))
    ss, sums = ops.scale_shift(offset_by_one(np.ones(n, dtype=np.float32)), t)
    assert ss.tolist() == [1.0, 0.0] and sums[:3].tolist() == [n, n, n]
    p = offset_by_one((g.random(n) * 10).astype(np.float32))
    ss, sums = ops.scale_shift(p, t, mask=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    assert ss.tolist() == [1.0, 0.0] and sums.tolist() == [0.0] * 5
    with pytest.raises(ValueError):
        ops.scale_shift(p, t[:-1])


@pytest.mark.parametrize("F", [1, 8, 22, 32])
@pytest.mark.parametrize("src,dst", [((56, 70), (48, 64)), ((14, 14), (1, 1)), ((1, 7), (3, 9)), ((48, 64), (48, 64))])
def test_depth_align_kernel(src, dst, F):
    """Bit for bit ops.depth_resize followed by separate torch mul, add, clamp_min and
    pre * w0 + v * w1 (three roundings), with and without clip / pre, and in place."""
    from vda_amd import ops
    g = torch.Generator().manual_seed(F * 100 + src[1] + dst[0])
    d = (torch.rand(F, *src, generator=g) * 50 - 10).cuda()     # negative values: the clip fires
    ss = torch.tensor([1.37, -3.25], device="cuda")
    pre0 = (torch.rand(F, *dst, generator=g) * 40).cuda()
    w = V.blend_weights(F) if F >= 2 else [0.3]
    w0 = [float(np.float32(1 - x)) for x in w]
    w1 = [float(np.float32(x)) for x in w]
    tw0 = torch.tensor(w0, device="cuda").view(-1, 1, 1)
    tw1 = torch.tensor(w1, device="cuda").view(-1, 1, 1)
    r = ops.depth_resize(d, *dst)
    assert torch.equal(ops.depth_align(d, *dst, clip=False), r)      # ss=None: the resize itself
    if dst == src:
        assert torch.equal(r, d)
    for clip in (False, True):
        v = torch.add(torch.mul(r, ss[0]), ss[1])
        if clip:
            assert v.numel() < 64 or (v < 0).any()
            v = v.clamp_min(0)
        assert torch.equal(ops.depth_align(d, *dst, ss=ss, clip=clip), v)
        blend = torch.add(torch.mul(pre0, tw0), torch.mul(v, tw1))
        assert torch.equal(ops.depth_align(d, *dst, ss=ss, clip=clip, pre=pre0, w_pre=w0, w_post=w1), blend)
        # out aliasing pre, with canary rows behind it
        big = torch.full((F + 2,) + dst, float("nan"), device="cuda")
        big[:F].copy_(pre0)
        out = ops.depth_align(d, *dst, ss=ss, clip=clip, pre=big[:F], w_pre=w0, w_post=w1, out=big[:F])
        assert out.data_ptr() == big.data_ptr()
        assert torch.equal(big[:F], blend) and torch.isnan(big[F:]).all()
    with pytest.raises(ValueError):
        ops.depth_align(d, *dst, pre=pre0)                          # a blend without weights
    with pytest.raises(ValueError):
        ops.depth_align(torch.zeros(33, 4, 4, device="cuda"), 4, 4)


# ---- drivers --------------------------------------------------------------------------------
_M = {}


def model():
    if "vits" not in _M:
        import vda_amd
        _M["vits"] = vda_amd.build_model("vits", state_dict=recipe_state_dict("vits"), device="cuda")
    return _M["vits"]


def test_golden_video_device_stitch_on_gpu():
    z = np.load(os.path.join(GOLDEN, "video_vits_57f.npz"), allow_pickle=False)
    frames, depth_ref, meta = z["frames"], z["depth"], json.loads(str(z["meta"]))
    m = model()
    kw = dict(input_size=meta["input_size"], device="cuda")
    host, _ = m.infer_video_depth(frames, meta["fps"], streams=2, **kw)
    d1, _ = m.infer_video_depth(frames, meta["fps"], streams=1, stitch="device", **kw)
    d2, _ = m.infer_video_depth(frames, meta["fps"], streams=2, stitch="device", **kw)
    e_ref, e_host = rel(d2, depth_ref), rel(d2, host)
    print(f"video 57 frames, device stitch: rel-L1 vs reference {e_ref:.3e}, vs host mode {e_host:.3e}")
    assert d2.shape == depth_ref.shape and d2.dtype == np.float32
    assert e_ref <= 1e-3, e_ref
    assert e_host <= 1e-5, e_host
    assert np.array_equal(d1, d2)
    t, _ = m.infer_video_depth(frames, meta["fps"], streams=2, stitch="device", return_device=True, **kw)
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == depth_ref.shape
    assert np.array_equal(t.cpu().numpy(), d2)


def test_video_device_stitch_memory_flat_in_video_length():
    """stitch="device" with host output: the stitcher keeps ref_align and one window's tail, the ring
    moves the settled frames out, so a 4x longer video has the same peak device memory."""
    def fwd(x):
        return x[:, :, 0].contiguous()
    peaks = []
    for n in (60, 240):
        frames = np.random.default_rng(n).integers(0, 256, (n, 48, 64, 3), dtype=np.uint8)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        d, _ = V.infer_video_depth(fwd, frames, 24, input_size=56, device="cuda", stitch="device")
        assert d.shape == (n, 48, 64)
        peaks.append(torch.cuda.max_memory_allocated() - base)
    assert peaks[1] <= peaks[0] * 1.1 + (1 << 20), peaks


def test_multirank_device_stitch_survives_side_stream_reuse(monkeypatch):
    """world=2 stand-in gather (side-stream receive buffers, a wait() that delays the current stream)
    with stitch="device": the network-resolution windows are stitched on the current stream while the
    side streams' next forwards scribble over same-size blocks; streams=2 must equal streams=1."""
    class _Work:
        def wait(self):
            torch.cuda._sleep(20_000_000)

    def fake_gather(buf, rank, world, group):
        bufs = [(buf * (1.0 + src)).contiguous() for src in range(world)]
        return bufs, _Work(), buf

    def fwd(x):
        for _ in range(3):
            torch.full((x.shape[0], x.shape[1], x.shape[3], x.shape[4]), -7.0, device=x.device)
        return (x[:, :, 0] * 3.0 + 1.0).contiguous()

    monkeypatch.setattr(V, "_gather_round", fake_gather)
    frames = np.random.default_rng(11).integers(0, 256, (150, 48, 64, 3), dtype=np.uint8)
    out = []
    for streams in (1, 2):
        d, _ = V.infer_video_depth(fwd, frames, 24, input_size=56, device="cuda", rank=0, world=2,
                                   streams=streams, stitch="device")
        torch.cuda.synchronize()
        out.append(d)
    assert out[0].shape == (150, 48, 64) and np.isfinite(out[0]).all()
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("case", ["kf2_12", "kf4_12_skip", "kf2_12_len16"])
def test_golden_stream_device_mode_on_gpu(case):
    z = np.load(os.path.join(GOLDEN, "stream_vits_50f.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    frames, ref = z["frames"], z["depth_" + case]
    m = model()
    kw = dict(input_size=meta["input_size"], device="cuda", **meta["cases"][case])
    host, _ = m.infere_single_image(frames, 24, **kw)
    dev, _ = m.infere_single_image(frames, 24, stitch="device", **kw)
    e_ref, e_host = rel(dev, ref), rel(dev, host)
    print(f"stream {case}, device mode: rel-L1 vs reference {e_ref:.3e}, vs host mode {e_host:.3e}")
    assert dev.shape == ref.shape and dev.dtype == np.float32 and np.isfinite(dev).all()
    assert e_ref <= 1e-3, e_ref
    assert e_host <= 1e-5, e_host
