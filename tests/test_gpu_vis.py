"""vda_depth_range / vda_depth_colorize on the GPU against the host path they replace.

Both sides round every fp32 operation once (numpy float32 on the host, IEEE operations without contraction in
the kernel), so the bar is equality: the index and the RGB frames equal ``video_io.colorize_depths``, the
planar layouts equal the payloads ``write_y4m`` puts into the file.  Shapes are the smallest at which the
kernels take another path: one pixel, odd H * W (every frame and plane misaligned, odd chroma edges), aligned,
a row longer than a block's pass, many blocks per frame (grid stride), a base that is 4- but not 16-byte aligned.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from helpers import device_at_offset
import vda_amd  # noqa: F401
from vda_amd import _lib
from vda_amd import video_io as VIO
from vda_amd import visualize as VIS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 37, 53), (5, 48, 64), (2, 3, 1030), (1, 720, 1280)]
CASES = [(s, False) for s in SHAPES] + [((3, 37, 53), True)]  # True: a view one float into a larger buffer
IDS = ["x".join(map(str, s)) + ("+4B" if off else "") for s, off in CASES]
LAYOUTS = ["index", "hwc", "planar444", "planar420"]


@functools.lru_cache(maxsize=None)
def host_clip(shape):
    """Random fp32 depth in [0.2, 7.5] and what the host path makes of it (computed once, read-only)."""
    d = np.random.default_rng(sum(shape)).uniform(0.2, 7.5, shape).astype(np.float32)
    with np.errstate(invalid="ignore"):  # one pixel is a constant clip: 0 / 0 on the host
        ref = {"d": d, "index": VIO.colorize_depths(d, grayscale=True), "inferno": VIO.colorize_depths(d),
               "spectral": VIO.colorize_depths(d, spectral=True)}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def as_tensor(a):
    return torch.from_numpy(np.array(a))  # a copy: the shared references are read-only


def on_device(d, offset):
    if not offset:
        return as_tensor(d).cuda()
    v = device_at_offset(d, 1)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def table(yuv=False, **kw):
    return as_tensor(VIS.color_table(yuv=yuv, **kw)).cuda()


def host_payloads(vis, chroma):
    """[F, bytes]: what write_y4m stores per frame for RGB frames ``vis``."""
    out = []
    for f in vis:
        y, u, v = VIO._rgb_to_yuv(f)
        if chroma == "420":
            u, v = VIO._subsample_420(u), VIO._subsample_420(v)
        out.append(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
    return np.stack(out)


@pytest.mark.parametrize("shape,offset", CASES, ids=IDS)
def test_range(shape, offset):
    d = host_clip(shape)["d"]
    r = VIS.LibVis.range(on_device(d, offset)).cpu().numpy()
    assert r.dtype == np.float32 and r[0] == d.min() and r[1] == d.max()


@pytest.mark.parametrize("n", [1023, 1025, 4095, 4096, 4097, 4 * 4096 + 5])
def test_range_around_one_block(n):
    """One block takes 4 x 1024 elements; the extremes sit in the last elements (the tail)."""
    d = np.random.default_rng(n).uniform(0.2, 7.5, n + 1).astype(np.float32)
    d[-1], d[-2] = 9.5, 0.1
    for off in (0, 1):  # a 16-byte-aligned base, and one float past it (three head elements)
        t = as_tensor(d).cuda()[off:]
        r = VIS.LibVis.range(t).cpu().numpy()
        assert r[0] == np.float32(0.1) and r[1] == np.float32(9.5)
    d[5], d[-1] = np.nan, np.nan
    r = VIS.LibVis.range(as_tensor(d).cuda()).cpu().numpy()
    assert r[0] == np.float32(0.1) and r[1] == np.nanmax(d)
    r = VIS.LibVis.range(torch.full((n,), float("nan"), device="cuda")).cpu().numpy()
    assert r[0] == np.inf and r[1] == -np.inf


@pytest.mark.parametrize("shape,offset", CASES, ids=IDS)
def test_colorize_equals_host_path(shape, offset):
    ref = host_clip(shape)
    t = on_device(ref["d"], offset)
    rng = VIS.LibVis.range(t)
    idx = VIS.LibVis.colorize(t, rng, None, "index")
    assert torch.equal(idx.cpu(), as_tensor(ref["index"]))
    tc, rc = t.cpu(), rng.cpu()
    for name, kw in (("inferno", {}), ("spectral", dict(spectral=True))):
        hwc = VIS.LibVis.colorize(t, rng, table(**kw), "hwc")
        assert torch.equal(hwc.cpu(), as_tensor(ref[name]))
        yuv = table(yuv=True, **kw)
        for layout, chroma in (("planar444", "444"), ("planar420", "420")):
            got = VIS.LibVis.colorize(t, rng, yuv, layout).cpu()
            assert torch.equal(got, VIS.TorchVis.colorize(tc, rc, yuv.cpu(), layout))
            assert np.array_equal(got.reshape(shape[0], -1).numpy(), host_payloads(ref[name], chroma))


def test_index_boundaries():
    """d = min + k (max - min) / 255 for every k: x lands on, or an ulp beside, every integer."""
    lo, hi = np.float32(0.3), np.float32(6.9)
    k = np.arange(256, dtype=np.float32)
    d = np.stack([lo + k * (hi - lo) / np.float32(255), np.nextafter(lo + k * (hi - lo) / np.float32(255), hi),
                  np.nextafter(lo + k * (hi - lo) / np.float32(255), lo)]).astype(np.float32).reshape(3, 16, 16)
    d = np.clip(d, lo, hi)
    ref = VIO.colorize_depths(d, grayscale=True)
    t = as_tensor(d).cuda()
    got = VIS.LibVis.colorize(t, VIS.LibVis.range(t), None, "index")
    assert torch.equal(got.cpu(), as_tensor(ref))
    assert len(np.unique(ref)) == 256


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 3, 1030), (5, 48, 64)], ids=["3x37x53", "2x3x1030", "5x48x64"])
def test_nothing_written_outside_the_output(shape, layout):
    """The C ABI on an output inside a larger buffer of canary bytes, at an odd and at an aligned address."""
    lib = _lib.lib()
    F, H, W = shape
    code = VIS.LAYOUTS[layout]
    t = as_tensor(host_clip(shape)["d"]).cuda()
    rng = VIS.LibVis.range(t)
    lut = table(yuv=True, spectral=True)
    want = VIS.LibVis.colorize(t, rng, lut, layout).reshape(-1)
    n = lib.vda_depth_colorize_bytes(F, H, W, code)
    assert n == want.numel()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lead in (61, 64):
        buf = torch.full((lead + n + 67,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.vda_depth_colorize(ctypes.c_void_p(t.data_ptr()), F, H, W, ctypes.c_void_p(rng.data_ptr()),
                                    ctypes.c_void_p(lut.data_ptr()), code, ctypes.c_void_p(buf.data_ptr() + lead), stream)
        assert rc == 0, lib.vda_last_error()
        torch.cuda.synchronize()
        assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + n:] == 0xA5).all())
        assert torch.equal(buf[lead:lead + n], want)


EDGE_RUNS = (1, 2, 3, 4, 5, 7, 8, 1030)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_range_every_head_and_tail(off):
    """depth starts ``off`` elements past a 16-byte boundary (heads of 0, 3, 2, 1 elements), with runs shorter
    than a head, shorter than one 16-byte group, and with every tail length; each element in turn holds the
    extremes, so one that is skipped shows."""
    for n in EDGE_RUNS:
        d = np.random.default_rng(10 * n + off).uniform(0.2, 7.5, n).astype(np.float32)
        for k in sorted({0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1} & set(range(n))):
            for v in (np.float32(0.1), np.float32(9.5)):
                e = d.copy()
                e[k] = v
                r = VIS.LibVis.range(device_at_offset(e, off)).cpu().numpy()
                assert r[0] == e.min() and r[1] == e.max(), (n, k, v, r)


@pytest.mark.parametrize("layout", ["index", "hwc"])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_colorize_every_head_and_tail(off, layout):
    """Two frames of S pixels, depth ``off`` elements past a 16-byte boundary, the output at byte offsets 0..3
    inside a buffer of canary bytes: the host path's bytes, and nothing around them."""
    lib = _lib.lib()
    code = VIS.LAYOUTS[layout]
    lut = None if layout == "index" else table()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for S in EDGE_RUNS:
        d = np.random.default_rng(10 * S + off).uniform(0.2, 7.5, (2, 1, S)).astype(np.float32)
        want = as_tensor(VIO.colorize_depths(d, grayscale=True) if layout == "index" else VIO.colorize_depths(d))
        t = device_at_offset(d, off)
        rng = VIS.LibVis.range(t)
        n = lib.vda_depth_colorize_bytes(2, 1, S, code)
        assert n == want.numel()
        for lead in (64, 61, 62, 63):
            buf = torch.full((lead + n + 67,), 0xA5, dtype=torch.uint8, device="cuda")
            assert (buf.data_ptr() + lead) % 4 == lead % 4
            rc = lib.vda_depth_colorize(ctypes.c_void_p(t.data_ptr()), 2, 1, S, ctypes.c_void_p(rng.data_ptr()),
                                        None if lut is None else ctypes.c_void_p(lut.data_ptr()), code,
                                        ctypes.c_void_p(buf.data_ptr() + lead), stream)
            assert rc == 0, lib.vda_last_error()
            torch.cuda.synchronize()
            assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + n:] == 0xA5).all()), (S, lead)
            assert torch.equal(buf[lead:lead + n].cpu(), want.reshape(-1)), (S, lead)


def test_range_from_the_whole_clip():
    t = as_tensor(host_clip((5, 48, 64))["d"]).cuda()
    rng = VIS.LibVis.range(t)
    lut = table(spectral=True)
    for layout in LAYOUTS:
        whole = VIS.LibVis.colorize(t, rng, lut, layout)
        assert torch.equal(VIS.LibVis.colorize(t[2:4], rng, lut, layout), whole[2:4])


def test_deterministic_and_constant_clip():
    t = as_tensor(host_clip((3, 37, 53))["d"]).cuda()
    lut = table()
    for layout in LAYOUTS:
        a = VIS.LibVis.colorize(t, VIS.LibVis.range(t), lut, layout)
        b = VIS.LibVis.colorize(t, VIS.LibVis.range(t), lut, layout)
        assert torch.equal(a, b)
    c = torch.full((2, 37, 53), 3.25, device="cuda")
    rng = VIS.LibVis.range(c)
    assert rng.cpu().tolist() == [3.25, 3.25]
    assert not VIS.LibVis.colorize(c, rng, None, "index").any()
    grey = table(grayscale=True)
    assert not VIS.LibVis.colorize(c, rng, grey, "hwc").any()


def test_chunked_device_path_and_save_video(tmp_path):
    """colorize_depths_device through the pinned ring (chunks of 2, 2, 1), and save_video on a CUDA tensor
    against save_video on the same depth in numpy: the same files."""
    ref = host_clip((5, 48, 64))
    t = as_tensor(ref["d"]).cuda()
    got = [c.copy() for c in VIS.colorize_depths_device(t, spectral=True, chunk=2)]
    assert [len(c) for c in got] == [2, 2, 1]
    assert np.array_equal(np.concatenate(got), ref["spectral"])
    for name, kw in (("a.y4m", dict(spectral=True)), ("b.y4m", dict(grayscale=True)), ("c.y4m", dict(chroma="420")),
                     ("d.png", dict()), ("e.png", dict(grayscale=True))):
        host, dev = str(tmp_path / ("host_" + name)), str(tmp_path / ("dev_" + name))
        VIO.save_video(ref["d"], host, fps=12, is_depths=True, **kw)
        VIO.save_video(t, dev, fps=12, is_depths=True, **kw)
        assert open(host, "rb").read() == open(dev, "rb").read(), name


def test_cli_device_vis_writes_the_host_file(tmp_path):
    """run.py --save_vis with --vis host and --vis device on the same device-stitched depth: the same bytes;
    --vis_chroma 420: the 4:2:0 file the host writer makes of that depth, its luma the 4:4:4 file's."""
    sys.path.insert(0, REPO)
    import run as cli
    fr = np.random.default_rng(0).integers(0, 256, (40, 42, 56, 3), dtype=np.uint8)
    clip = str(tmp_path / "clip.y4m")
    VIO.write_y4m(clip, fr, 24)
    base = ["--input_video", clip, "--encoder", "vits", "--input_size", "56", "--synthetic_weights", "--stitch", "device",
            "--save_vis"]
    name = "VideoDepthAny_vits_clip_vis.y4m"
    dh = cli.main(base + ["--output_dir", str(tmp_path / "h"), "--vis", "host"])
    dd = cli.main(base + ["--output_dir", str(tmp_path / "d"), "--vis", "device"])
    d4 = cli.main(base + ["--output_dir", str(tmp_path / "c"), "--vis", "device", "--vis_chroma", "420"])
    assert isinstance(dd, np.ndarray) and dd.shape == (40, 42, 56)
    assert np.array_equal(dh, dd) and np.array_equal(dh, d4)
    f444 = open(str(tmp_path / "h" / name), "rb").read()
    assert f444 == open(str(tmp_path / "d" / name), "rb").read()
    VIO.write_y4m(str(tmp_path / "ref420.y4m"), VIO.colorize_depths(dh, spectral=True), 24, chroma="420")
    f420 = open(str(tmp_path / "c" / name), "rb").read()
    assert f420 == open(str(tmp_path / "ref420.y4m"), "rb").read()
    back, fps = VIO.read_y4m(str(tmp_path / "c" / name))
    assert back.shape == (40, 42, 56, 3) and abs(fps - 24) < 1e-9
    S, rec444, rec420 = 42 * 56, 6 + 3 * 42 * 56, 6 + 42 * 56 + 2 * 21 * 28
    b444, b420 = f444[f444.index(b"\n") + 1:], f420[f420.index(b"\n") + 1:]
    for i in range(40):
        assert b444[i * rec444 + 6:i * rec444 + 6 + S] == b420[i * rec420 + 6:i * rec420 + 6 + S]
