"""vda_depth_absdiff_range / vda_panel_compose on the GPU against ``TorchCompare`` and the plain numpy
composition of the panels (tests/compare_ref.py).

Every per-pixel operation is one correctly rounded fp32 operation followed by integer work on both sides, so
the bar is equality.  Shapes are the smallest at which the kernels take another path: one pixel, odd H x W
(every frame and plane misaligned, 4:2:0 blocks that straddle two tiles, groups of 4 across a tile seam), aligned,
a row longer than a block's pass, a warmed-up second method, a chunk that starts at t0 > 0, an output whose
base is odd, a source one float past 16-byte alignment.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import device_at_offset
import vda_amd  # noqa: F401
from vda_amd import _lib
from vda_amd import compare as CMP
from vda_amd import video_io as VIO
from vda_amd import visualize as VIS

import compare_ref as R

pytestmark = pytest.mark.gpu
LAYOUTS = ["hwc", "planar444", "planar420"]
RANGE_SHAPES = [(1, 1, 1), (3, 37, 53), (2, 3, 1030), (1023,), (4095,), (4096,), (4097,), (4 * 4096 + 5,)]


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_absdiff_range(shape, masked):
    """The extremes in the last elements (the tail), NaNs present, the bases one float past 16-byte alignment."""
    g = np.random.default_rng(sum(shape))
    n = int(np.prod(shape))
    gt = g.uniform(1., 60., shape).astype(np.float32)
    pred = (gt + g.uniform(0.5, 5., shape)).astype(np.float32)
    valid = np.ones(shape, dtype=bool)
    if n >= 4:
        pred.reshape(-1)[0] = np.nan
        pred.reshape(-1)[-2] = gt.reshape(-1)[-2] + np.float32(0.125)  # the minimum, unless masked out
        valid.reshape(-1)[n // 2] = False
    pred.reshape(-1)[-1] = gt.reshape(-1)[-1] - np.float32(70.)  # the maximum
    m = valid if masked else None
    e = R.error_map(gt, pred, m)
    want = [float(np.nanmin(e)), float(np.nanmax(e))]
    assert np.nanargmax(e.reshape(-1)) == n - 1 and (n < 4 or np.nanargmin(e.reshape(-1)) == (n // 2 if masked else n - 2))
    dp, dg = device_at_offset(pred, 1), device_at_offset(gt, 1)
    dv = None if m is None else device_at_offset(m.view(np.uint8), 1)
    got = CMP.LibCompare.absdiff_range(dp, dg, dv).cpu()
    assert got.tolist() == want
    mirror = CMP.TorchCompare.absdiff_range(torch.from_numpy(pred), torch.from_numpy(gt), None if m is None else torch.from_numpy(m))
    assert got.tolist() == mirror.tolist()


@functools.lru_cache(maxsize=None)
def host_scene(N, H, W, offsets, with_rgb=True, with_valid=True, line=0.5):
    """A scene and its numpy canvas (computed once, read-only)."""
    gt, preds, rgb, valid = R.scene(N, H, W, offsets, seed=N * H + W, with_rgb=with_rgb, with_valid=with_valid)
    dr, er = R.ranges(gt, preds, valid)
    canvas = R.canvas_rgb(gt, preds, rgb, valid, dr, er, int(W * line))
    canvas.setflags(write=False)
    return dict(gt=gt, preds=preds, rgb=rgb, valid=valid, dr=dr, er=er, line=line, canvas=canvas)


def device_result(s):
    return R.result_of(s["gt"], s["preds"], s["rgb"], s["valid"], s["dr"], s["er"], s["line"], "cuda", CMP.LibCompare)


SHAPES = [(1, 1, 1), (2, 2, 2), (3, 37, 53), (5, 48, 64), (2, 3, 1030)]  # the last: a row longer than a block's pass


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_panel_compose_one_method(shape, layout):
    s = host_scene(*shape, (0,))
    got = R.frames_of(device_result(s), layout)
    assert np.array_equal(got, R.to_layout(s["canvas"], layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_panel_compose_two_methods_warmup(layout):
    """M = 2, the second method one frame short (o = 1), no RGB (a black cell), stability line at the last column;
    also against the torch mirror."""
    s = host_scene(3, 37, 53, (0, 1), False, False, 0.999)
    got = R.frames_of(device_result(s), layout)
    assert np.array_equal(got, R.to_layout(s["canvas"], layout))
    cpu = R.result_of(s["gt"], s["preds"], s["rgb"], s["valid"], s["dr"], s["er"], s["line"], "cpu", CMP.TorchCompare)
    assert np.array_equal(got, R.frames_of(cpu, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_panel_compose_chunks_equal_whole_video(layout):
    """The composer called chunk-wise (t0 = 0, 2, 4) against one call over the whole video; N > W."""
    s = host_scene(5, 9, 4, (0, 2))
    res = device_result(s)
    whole = R.frames_of(res, layout, chunk=32)
    assert np.array_equal(R.frames_of(res, layout, chunk=2), whole)
    assert np.array_equal(whole, R.to_layout(s["canvas"], layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_panel_compose_odd_output_base_and_offset_sources(layout):
    """The C ABI directly: out starts at an odd address inside a guarded buffer, the float sources one float
    past 16-byte alignment; nothing is written outside vda_panel_compose_bytes."""
    s = host_scene(3, 37, 53, (0, 1))
    N, H, W = s["gt"].shape
    lib = _lib.lib()
    code = VIS.LAYOUTS[layout]
    yuv = layout != "hwc"
    keep = [device_at_offset(s["gt"], 1), torch.from_numpy(s["rgb"]).cuda(),
            device_at_offset(s["valid"].view(np.uint8), 1), torch.from_numpy(s["dr"]).cuda(),
            torch.from_numpy(s["er"]).cuda(), torch.from_numpy(VIS.named_color_table("Spectral", yuv)).cuda(),
            torch.from_numpy(VIS.named_color_table("RdYlGn", yuv)).cuda()]
    gt, rgb, valid, dr, er, lut0, lut1 = keep
    S = H * W
    tiles = [_lib.Tile(kind=_lib.TILE_RGB, row=0, col=0, frames=N, a=rgb.data_ptr()),
             _lib.Tile(kind=_lib.TILE_DEPTH, row=0, col=1, frames=N, a=gt.data_ptr(), range=dr.data_ptr()),
             _lib.Tile(kind=_lib.TILE_XT, row=0, col=2, frames=N, a=gt.data_ptr(), range=dr.data_ptr())]
    for i, p in enumerate(s["preds"]):
        o = N - len(p)
        dp = device_at_offset(p, 1)
        keep.append(dp)
        common = dict(row=1 + i, offset=o, frames=len(p), a=dp.data_ptr())
        tiles += [_lib.Tile(kind=_lib.TILE_ERROR, col=0, b=gt.data_ptr() + 4 * o * S, valid=valid.data_ptr() + o * S,
                            range=er.data_ptr(), lut=1, **common),
                  _lib.Tile(kind=_lib.TILE_DEPTH, col=1, range=dr.data_ptr(), **common),
                  _lib.Tile(kind=_lib.TILE_XT, col=2, range=dr.data_ptr(), **common)]
    rows = 1 + len(s["preds"])
    nbytes = lib.vda_panel_compose_bytes(N, rows, 3, H, W, code)
    want = R.to_layout(s["canvas"], layout)
    assert nbytes == want.size
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = 17
    assert (buf.data_ptr() + base) % 2 == 1
    arr = (_lib.Tile * len(tiles))(*tiles)
    rc = lib.vda_panel_compose(arr, len(tiles), rows, 3, N, 0, N, H, W, W // 2, ctypes.c_void_p(lut0.data_ptr()),
                               ctypes.c_void_p(lut1.data_ptr()), code, ctypes.c_void_p(buf.data_ptr() + base),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "vda_panel_compose")
    host = buf.cpu().numpy()
    assert np.array_equal(host[base:base + nbytes], want.reshape(-1))
    assert (host[:base] == 0xA5).all() and (host[base + nbytes:] == 0xA5).all()


def test_rgb_tile_converts_every_triple():
    """All 2^24 RGB triples as one 4096 x 4096 frame through the RGB tile in planar444."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    from vda_amd import ops
    out = ops.panel_compose([dict(kind="rgb", row=0, col=0, a=torch.from_numpy(rgb).cuda())], 1, 1, 1, 0, 1, 0,
                            layout="planar444").cpu().numpy()
    for c, plane in enumerate(VIO._rgb_to_yuv(rgb[0])):
        assert np.array_equal(out[0, c], plane), "YUV"[c]


def test_single_720p_frame_420():
    """One 720 x 1280 frame, M = 1, 4:2:0: many blocks per frame (the grid stride)."""
    s = host_scene(1, 720, 1280, (0,))
    got = R.frames_of(device_result(s), "planar420")
    assert np.array_equal(got, R.to_layout(s["canvas"], "planar420"))


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_end_to_end_file_equals_cpu_mirror(tmp_path, chroma):
    """compare_depths + save_compare_video on device tensors against the same calls on the CPU mirror."""
    g = np.random.default_rng(11)
    N, H, W = 5, 37, 53
    gt = g.uniform(2., 90., (N, H, W)).astype(np.float32)
    valid = g.random((N, H, W)) < 0.8
    rgb = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    noise = lambda n: np.float32(0.02) * g.standard_normal((n, H, W)).astype(np.float32)  # noqa: E731
    preds = {"VDA": (np.float32(37.) / gt + np.float32(2.5) + noise(N)).astype(np.float32),
             "VDA_s": (np.float32(21.) / gt[2:] + np.float32(1.25) + noise(N - 2)).astype(np.float32)}
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dev = CMP.compare_depths(t(gt), {k: t(v) for k, v in preds.items()}, rgb=t(rgb), valid=t(valid))
    cpu = CMP.compare_depths(gt, preds, rgb=rgb, valid=valid)
    assert dev.backend is CMP.LibCompare and cpu.backend is CMP.TorchCompare
    assert dev.depth_range.tolist() == cpu.depth_range.tolist()
    assert dev.error_range.tolist() == cpu.error_range.tolist()
    for k in preds:
        assert dev.methods[k].scale == cpu.methods[k].scale and dev.methods[k].shift == cpu.methods[k].shift
        assert dev.methods[k].offset == cpu.methods[k].offset
        assert np.allclose(dev.methods[k].frame_mse, cpu.methods[k].frame_mse, rtol=1e-12)
    CMP.save_compare_video(str(tmp_path / "dev.y4m"), dev, fps=24, chroma=chroma, chunk=2)
    CMP.save_compare_video(str(tmp_path / "cpu.y4m"), cpu, fps=24, chroma=chroma)
    assert open(tmp_path / "dev.y4m", "rb").read() == open(tmp_path / "cpu.y4m", "rb").read()
