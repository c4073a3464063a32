"""Depth visualisation off the host passes (vda_amd.visualize, video_io's 4:2:0 writer, run.py --vis): what
runs without a GPU.  The colour tables and the ``TorchVis`` restatement of the kernels' arithmetic are held to
``video_io.colorize_depths`` / ``write_y4m`` bit for bit; the C ABI's argument checks run before any launch.
"""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import vda_amd  # noqa: F401
from vda_amd import _lib
from vda_amd import video_io as VIO
from vda_amd import visualize as VIS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [dict(), dict(spectral=True), dict(grayscale=True)]  # inferno, Spectral, grey


def clip(shape=(3, 37, 53), seed=0):
    return np.random.default_rng(seed).uniform(0.2, 7.5, shape).astype(np.float32)


def payloads(path, nbytes):
    """The frame payloads of a y4m file written by ``write_y4m``: [n, nbytes] uint8."""
    data = open(path, "rb").read()
    body = data[data.index(b"\n") + 1:]
    rec = len(b"FRAME\n") + nbytes
    assert len(body) % rec == 0
    out = []
    for i in range(len(body) // rec):
        assert body[i * rec:i * rec + 6] == b"FRAME\n"
        out.append(np.frombuffer(body, np.uint8, nbytes, i * rec + 6))
    return np.stack(out)


def host_rgb(vis):
    """colorize_depths' result as the [F, H, W, 3] frames write_y4m makes of it (grey is repeated)."""
    return np.repeat(vis[..., None], 3, -1) if vis.ndim == 3 else vis


@pytest.mark.parametrize("kw", MAPS)
def test_tables_reproduce_colorize_depths(kw):
    d = clip()
    idx = VIO.colorize_depths(d, grayscale=True)
    vis = host_rgb(VIO.colorize_depths(d, **kw))
    assert np.array_equal(VIS.color_table(**kw)[idx], vis)
    tab = VIS.color_table(yuv=True, **kw)
    assert tab.shape == (256, 3) and tab.dtype == np.uint8
    for f in range(d.shape[0]):
        for c, plane in enumerate(VIO._rgb_to_yuv(vis[f])):
            assert np.array_equal(tab[idx[f]][..., c], plane)
    i = np.arange(256, dtype=np.uint8)
    assert np.array_equal(VIS.color_table(grayscale=True), np.stack([i, i, i], -1))


@pytest.mark.parametrize("kw", MAPS)
def test_torchvis_reproduces_host_path(kw, tmp_path):
    d = clip()
    t = torch.from_numpy(d)
    rng = VIS.TorchVis.range(t)
    assert rng.dtype == torch.float32 and rng[0].item() == d.min() and rng[1].item() == d.max()
    idx = VIO.colorize_depths(d, grayscale=True)
    vis = host_rgb(VIO.colorize_depths(d, **kw))
    assert np.array_equal(VIS.TorchVis.colorize(t, rng, None, "index").numpy(), idx)
    rgb = torch.from_numpy(VIS.color_table(**kw))
    assert np.array_equal(VIS.TorchVis.colorize(t, rng, rgb, "hwc").numpy(), vis)
    yuv = torch.from_numpy(VIS.color_table(yuv=True, **kw))
    p444 = VIS.TorchVis.colorize(t, rng, yuv, "planar444").numpy()
    assert p444.shape == (3, 3, 37, 53)
    VIO.write_y4m(str(tmp_path / "a.y4m"), vis, 10)
    assert np.array_equal(p444.reshape(3, -1), payloads(str(tmp_path / "a.y4m"), 3 * 37 * 53))


@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 2, 2), (2, 1, 1)])
def test_torchvis_420_is_the_420_file(shape, tmp_path):
    d = clip(shape, seed=1)
    t = torch.from_numpy(d)
    F, H, W = shape
    nbytes = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    yuv = torch.from_numpy(VIS.color_table(spectral=True, yuv=True))
    p420 = VIS.TorchVis.colorize(t, VIS.TorchVis.range(t), yuv, "planar420").numpy()
    assert p420.shape == (F, nbytes)
    VIO.write_y4m(str(tmp_path / "a.y4m"), VIO.colorize_depths(d, spectral=True), 10, chroma="420")
    assert np.array_equal(p420, payloads(str(tmp_path / "a.y4m"), nbytes))


def test_420_round_trip_and_default_unchanged(tmp_path):
    vis = VIO.colorize_depths(clip(), spectral=True)
    p444, p420, pdef = (str(tmp_path / n) for n in ("a444.y4m", "a420.y4m", "adef.y4m"))
    VIO.write_y4m(p444, vis, 24, chroma="444")
    VIO.write_y4m(p420, vis, 24, chroma="420")
    VIO.write_y4m(pdef, vis, 24)
    assert open(pdef, "rb").read() == open(p444, "rb").read()
    # the file as the code before the keyword wrote it: the C444 header, then y, u, v of every frame
    old = b"YUV4MPEG2 W53 H37 F24024:1001 Ip A1:1 C444\n"
    for f in vis:
        old += b"FRAME\n" + b"".join(p.tobytes() for p in VIO._rgb_to_yuv(f))
    assert open(pdef, "rb").read() == old
    VIO.save_video(vis, str(tmp_path / "sv.y4m"), fps=24)  # the existing caller, which passes no keyword
    assert open(str(tmp_path / "sv.y4m"), "rb").read() == old
    back, fps = VIO.read_y4m(p420)
    assert back.shape == (3, 37, 53, 3) and fps == 24
    assert b"C420jpeg" in open(p420, "rb").read(64)
    y444 = payloads(p444, 3 * 37 * 53)[:, :37 * 53]
    y420 = payloads(p420, 37 * 53 + 2 * 19 * 27)[:, :37 * 53]
    assert np.array_equal(y444, y420)
    with pytest.raises(ValueError):
        VIO.write_y4m(p420, vis, 24, chroma="422")


def test_constant_depth_gives_index_zero():
    t = torch.full((2, 5, 7), 3.25)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rng = VIS.TorchVis.range(t)
        idx = VIS.TorchVis.colorize(t, rng, None, "index")
        chunks = [c.copy() for c in VIS.colorize_depths_device(t, grayscale=True, layout="index")]
    assert idx.dtype == torch.uint8 and not idx.any()
    assert not np.concatenate(chunks).any()


def test_nan_pixels_are_skipped_by_the_range_and_get_index_zero():
    d = clip()
    d[0, 3, 5] = d[2, 36, 52] = d[1, 0, 0] = np.nan
    t = torch.from_numpy(d)
    rng = VIS.TorchVis.range(t)
    assert rng[0].item() == np.nanmin(d) and rng[1].item() == np.nanmax(d)
    idx = VIS.TorchVis.colorize(t, rng, None, "index").numpy()
    assert idx[0, 3, 5] == 0 and idx[2, 36, 52] == 0 and idx[1, 0, 0] == 0
    fin = ~np.isnan(d)
    ref = ((d - np.nanmin(d)) / (np.nanmax(d) - np.nanmin(d)) * 255)[fin].astype(np.uint8)
    assert np.array_equal(idx[fin], ref)
    allnan = VIS.TorchVis.range(torch.full((4,), float("nan")))
    assert allnan[0].item() == float("inf") and allnan[1].item() == float("-inf")


@pytest.mark.parametrize("layout", ["index", "hwc", "planar444", "planar420"])
def test_chunks(layout):
    t = torch.from_numpy(clip((5, 6, 10), seed=2))
    got = [c.copy() for c in VIS.colorize_depths_device(t, spectral=True, layout=layout, chunk=2, backend=VIS.TorchVis)]
    assert [len(c) for c in got] == [2, 2, 1]
    whole = list(VIS.colorize_depths_device(t, spectral=True, layout=layout, chunk=32, backend=VIS.TorchVis))
    assert len(whole) == 1 and whole[0].dtype == np.uint8
    assert np.array_equal(np.concatenate(got), whole[0])
    if layout == "hwc":
        assert np.array_equal(whole[0], VIO.colorize_depths(t.numpy(), spectral=True))
    with pytest.raises(ValueError):
        next(VIS.colorize_depths_device(t, layout="nv12"))


def _rejected(rc, msg):
    assert rc == -22
    err = _lib.lib().vda_last_error()
    assert msg in err, err


def test_c_abi_rejects_bad_arguments():
    """Fake pointers: a launch would fault, so every case must be refused before it."""
    lib = _lib.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
    ws = lib.vda_depth_range_workspace(5000)
    assert ws > 0 and lib.vda_depth_range_workspace(0) == 0
    _rejected(lib.vda_depth_range(None, 5000, fake, fake, ws, None), b"null pointer")
    _rejected(lib.vda_depth_range(fake, 5000, None, fake, ws, None), b"null pointer")
    _rejected(lib.vda_depth_range(fake, 5000, fake, None, ws, None), b"null pointer")
    _rejected(lib.vda_depth_range(fake, 0, fake, fake, ws, None), b"n >= 1")
    _rejected(lib.vda_depth_range(odd, 5000, fake, fake, ws, None), b"4-byte aligned")
    _rejected(lib.vda_depth_range(fake, 5000, fake, fake, ws - 1, None), b"workspace")
    col = lambda *a: lib.vda_depth_colorize(*a, None)  # noqa: E731
    _rejected(col(None, 2, 3, 4, fake, fake, _lib.VIS_HWC, fake), b"null pointer")
    _rejected(col(fake, 2, 3, 4, None, fake, _lib.VIS_HWC, fake), b"null pointer")
    _rejected(col(fake, 2, 3, 4, fake, fake, _lib.VIS_HWC, None), b"null pointer")
    _rejected(col(fake, 0, 3, 4, fake, fake, _lib.VIS_HWC, fake), b"F >= 1")
    _rejected(col(fake, 2, 0, 4, fake, fake, _lib.VIS_HWC, fake), b"H >= 1")
    _rejected(col(fake, 2, 3, -1, fake, fake, _lib.VIS_HWC, fake), b"W >= 1")
    _rejected(col(fake, 65536, 3, 4, fake, fake, _lib.VIS_HWC, fake), b"65535")
    _rejected(col(fake, 2, 3, 4, fake, fake, 4, fake), b"unknown layout")
    _rejected(col(fake, 2, 3, 4, fake, fake, -1, fake), b"unknown layout")
    for layout in (_lib.VIS_HWC, _lib.VIS_PLANAR444, _lib.VIS_PLANAR420):
        _rejected(col(fake, 2, 3, 4, fake, None, layout, fake), b"needs a lut")
    _rejected(col(odd, 2, 3, 4, fake, fake, _lib.VIS_HWC, fake), b"4-byte aligned")


def test_byte_counts():
    n = _lib.lib().vda_depth_colorize_bytes
    for F, H, W in [(1, 1, 1), (2, 2, 2), (3, 37, 53), (5, 48, 64), (2, 3, 1030), (64, 720, 1280)]:
        assert n(F, H, W, _lib.VIS_INDEX) == F * H * W
        assert n(F, H, W, _lib.VIS_HWC) == 3 * F * H * W
        assert n(F, H, W, _lib.VIS_PLANAR444) == 3 * F * H * W
        assert n(F, H, W, _lib.VIS_PLANAR420) == F * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
    assert n(40000, 720, 1280, _lib.VIS_HWC) == 3 * 40000 * 720 * 1280  # past 2^31
    assert n(0, 4, 4, _lib.VIS_HWC) == 0 and n(1, 4, 4, 7) == 0
    assert (VIS.LAYOUTS["index"], VIS.LAYOUTS["hwc"], VIS.LAYOUTS["planar444"], VIS.LAYOUTS["planar420"]) == \
        (_lib.VIS_INDEX, _lib.VIS_HWC, _lib.VIS_PLANAR444, _lib.VIS_PLANAR420)


def test_meta_shapes_and_no_cpu_kernel():
    import vda_amd.torch_ops  # noqa: F401
    d = torch.empty(3, 37, 53, device="meta")
    rng = torch.ops.vda.depth_range(d)
    assert rng.shape == (2,) and rng.dtype == torch.float32
    lut = torch.empty(256, 3, device="meta", dtype=torch.uint8)
    shapes = {_lib.VIS_INDEX: (3, 37, 53), _lib.VIS_HWC: (3, 37, 53, 3), _lib.VIS_PLANAR444: (3, 3, 37, 53),
              _lib.VIS_PLANAR420: (3, 37 * 53 + 2 * 19 * 27)}
    for layout, shape in shapes.items():
        o = torch.ops.vda.depth_colorize(d, rng, lut, layout)
        assert o.shape == shape and o.dtype == torch.uint8
    assert torch.ops.vda.depth_colorize(d, rng, None, _lib.VIS_INDEX).shape == (3, 37, 53)
    with pytest.raises(RuntimeError):
        torch.ops.vda.depth_colorize(d, rng, None, _lib.VIS_HWC)
    with pytest.raises(NotImplementedError):
        torch.ops.vda.depth_range(torch.zeros(4))
    from vda_amd import ops
    with pytest.raises(ValueError):
        ops.depth_range(torch.zeros(4))
    with pytest.raises(ValueError):
        ops.depth_colorize(torch.zeros(1, 2, 2), torch.zeros(2))


def test_cli_flags():
    run = [sys.executable, os.path.join(REPO, "run.py")]
    r = subprocess.run(run + ["--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--vis " in r.stdout and "--vis_chroma" in r.stdout
    r = subprocess.run(run + ["--input_video", "x.y4m", "--save_vis", "--vis", "device"], capture_output=True, text=True)
    assert r.returncode != 0 and "--stitch device" in r.stderr
