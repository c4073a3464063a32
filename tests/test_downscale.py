"""The device downscale of .y4m frames, as far as it runs without a GPU: the resampling tables and their torch
restatement against Pillow itself, the C tables against the Python ones, ``open_y4m(max_res=...)`` against
``read_video_frames`` and the command line.

Every comparison is equality: Pillow resamples 8-bit images in integer fixed point, and the tables are computed in
IEEE doubles with one rounding per operation on every side.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vda_amd import _lib
from vda_amd import decode as D
from vda_amd import video_io as VIO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w) -> (h2, w2): the 4K and 1080p product ratios, a ratio that is no integer, small even and odd frames, one
# axis unchanged, one axis growing by a pixel
SHAPES = [((2160, 3840), (720, 1280)), ((1080, 1920), (720, 1280)), ((1442, 2562), (720, 1280)),
          ((90, 160), (36, 64)), ((161, 90), (64, 36)), ((33, 65), (16, 32)), ((50, 131), (50, 64)),
          ((37, 1300), (38, 1280))]
AXES = sorted({(a, b) for (h, w), (h2, w2) in SHAPES for a, b in ((h, h2), (w, w2))} | {(10240, 1280), (5, 6)})


def frames_444(n, h, w, kind):
    """4:4:4 payloads [n, 3 * h * w] whose decoded frames exercise the resampler: random bytes, or
    Y in {16, 235} with grey chroma, which decodes to 0 / 255 images (both clamps through the negative lobes)."""
    g = np.random.default_rng(h * 7 + w)
    if kind == "random":
        return g.integers(0, 256, (n, 3 * h * w), dtype=np.uint8)
    y = np.where(g.integers(0, 2, (n, h * w)) == 1, 235, 16).astype(np.uint8)
    return np.concatenate([y, np.full((n, 2 * h * w), 128, np.uint8)], 1)


@pytest.mark.parametrize("kind", ["random", "binary"])
@pytest.mark.parametrize("hw,hw2", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES])
def test_torch_downscale_equals_pillow(hw, hw2, kind):
    (h, w), (h2, w2) = hw, hw2
    n = 1 if h * w > 1000000 else 2
    pay = frames_444(n, h, w, kind)
    rgb = np.stack([VIO._decode_payload(p, w, h, w, h) for p in pay])
    if kind == "binary":
        assert set(np.unique(rgb)) == {0, 255}
    ref = VIO._resize_rgb(rgb, h2, w2)
    out = D.TorchDecode.downscale(torch.from_numpy(pay), h, w, "444", (h2, w2))
    assert out.shape == (n, h2, w2, 3) and out.dtype == torch.uint8
    assert np.array_equal(out.numpy(), ref)


def test_torch_downscale_takes_subsampled_chroma():
    pay = np.random.default_rng(3).integers(0, 256, (2, D.payload_bytes(37, 53, "420")), dtype=np.uint8)
    rgb = np.stack([VIO._decode_payload(p, 53, 37, 27, 19) for p in pay])
    out = D.TorchDecode.downscale(torch.from_numpy(pay), 37, 53, "420", (16, 22))
    assert np.array_equal(out.numpy(), VIO._resize_rgb(rgb, 16, 22))


@pytest.mark.parametrize("n_in,n_out", AXES, ids=[f"{a}-{b}" for a, b in AXES])
def test_c_tables_equal_python_tables(n_in, n_out):
    lib = _lib.lib()
    k, b = D.resample_tables(n_in, n_out)
    taps = lib.vda_resample_taps(n_in, n_out)
    assert taps == k.shape[1] == D.resample_taps(n_in, n_out) and k.shape[0] == b.shape[0] == n_out
    ck = np.full((n_out, taps), -7, np.int32)
    cb = np.full((n_out, 2), -7, np.int32)
    assert lib.vda_resample_tables(n_in, n_out, ck.ctypes.data_as(ctypes.c_void_p), cb.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(ck, k.numpy()) and np.array_equal(cb, b.numpy())
    # every row reads inside the axis, and its coefficients sum to one within the rounding of its taps
    assert (cb[:, 0] >= 0).all() and (cb[:, 1] >= 1).all() and (cb[:, 0] + cb[:, 1] <= n_in).all()
    assert (np.abs(ck.sum(1) - (1 << 22)) <= taps).all()
    # the kernel multiplies with 24-bit multiplies and accumulates in int32 (include/vda.h)
    pos = np.where(ck > 0, ck, 0).astype(np.int64).sum(1).max()
    assert np.abs(ck).max() < (1 << 23) and 255 * pos + (1 << 21) < (1 << 31)


def test_c_tables_refuse_bad_arguments():
    lib = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    assert lib.vda_resample_taps(0, 4) == 0 and lib.vda_resample_taps(4, 0) == 0
    assert lib.vda_resample_tables(4, 2, None, buf) == -22
    assert lib.vda_resample_tables(0, 2, buf, buf) == -22


def test_downscale_route_queries_and_refusals():
    """The compiled cap is 29 coefficients per axis (a ratio of 7); beyond it the entry point refuses before any
    launch (fake pointers: a launch would fault).  No shape needs a workspace."""
    lib = _lib.lib()
    ok = lib.vda_yuv_downscale_ok
    assert ok(2160, 3840, 720, 1280) == 1 and ok(1080, 1920, 720, 1280) == 1 and ok(4320, 7680, 720, 1280) == 1
    assert ok(720, 8960, 720, 1280) == 1 and ok(720, 8961, 720, 1280) == 0
    assert ok(8961, 64, 1280, 64) == 0 and ok(0, 4, 2, 2) == 0
    assert ok(5, 64, 6, 32) == 1 and ok(64, 64, 64, 64) == 1
    assert lib.vda_resample_taps(7680, 1280) == 25 and lib.vda_resample_taps(8960, 1280) == 29
    assert lib.vda_yuv_downscale_workspace(32, 2160, 3840, 720, 1280) == 0
    fake = ctypes.c_void_p(0x1000)

    def call(src=fake, N=2, h=36, w=104, stride=D.payload_bytes(36, 104, "420"), chroma=_lib.YUV_420, out=fake,
             h2=12, w2=34, tables=(fake, fake, fake, fake)):
        return lib.vda_yuv_downscale(src, N, h, w, stride, chroma, *tables, out, h2, w2, None, 0, None)

    def rejected(rc, msg):
        assert rc == -22 and msg in lib.vda_last_error(), lib.vda_last_error()

    rejected(call(src=None), b"null pointer")
    rejected(call(out=None), b"null pointer")
    rejected(call(N=0), b"empty frame geometry")
    rejected(call(w2=0), b"empty frame geometry")
    rejected(call(chroma=5), b"unknown chroma code")
    rejected(call(stride=100), b"frame_stride")
    rejected(call(N=65536), b"exceed the launch grid")
    rejected(call(tables=(None, fake, fake, fake)), b"null coefficient table")
    rejected(call(tables=(fake, fake, fake, None)), b"null coefficient table")
    rejected(call(h=8, w=8961, stride=D.payload_bytes(8, 8961, "420"), h2=8, w2=1280), b"tap capacity")


def test_ops_refuse_cpu_tensors_and_meta_shapes():
    import vda_amd.torch_ops  # noqa: F401
    from vda_amd import ops
    with pytest.raises(ValueError):
        ops.yuv_downscale(torch.zeros(1, 64, dtype=torch.uint8), 4, 4, "444", 2, 2)
    assert ops.yuv_downscale_accepts(2160, 3840, 720, 1280) and not ops.yuv_downscale_accepts(720, 8961, 720, 1280)
    meta = lambda *s: torch.empty(*s, device="meta", dtype=torch.int32)  # noqa: E731
    pay = torch.empty(3, D.payload_bytes(36, 104, "420"), device="meta", dtype=torch.uint8)
    tables = (meta(34, 15), meta(34, 2), meta(12, 13), meta(12, 2))  # 104 / 34 > 3: 15 taps; 36 / 12 = 3: 13
    o = torch.ops.vda.yuv_downscale(pay, 36, 104, _lib.YUV_420, 12, 34, *tables)
    assert o.shape == (3, 12, 34, 3) and o.dtype == torch.uint8
    with pytest.raises(RuntimeError):  # the horizontal table of another ratio
        torch.ops.vda.yuv_downscale(pay, 36, 104, _lib.YUV_420, 12, 34, meta(34, 13), *tables[1:])
    with pytest.raises(RuntimeError):  # float tables
        torch.ops.vda.yuv_downscale(pay, 36, 104, _lib.YUV_420, 12, 34, tables[0].float(), *tables[1:])
    with pytest.raises(NotImplementedError):
        cpu = [torch.zeros(t.shape, dtype=torch.int32) for t in tables]
        torch.ops.vda.yuv_downscale(torch.zeros(3, pay.shape[1], dtype=torch.uint8), 36, 104, _lib.YUV_420, 12, 34, *cpu)


def rgb_clip(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("hw,max_res", [((36, 104), 34), ((45, 28), 30), ((37, 53), 40)],
                         ids=["wide", "tall", "odd"])
def test_open_y4m_max_res_matches_read_video_frames(tmp_path, hw, max_res):
    h, w = hw
    p = str(tmp_path / "clip.y4m")
    VIO.write_y4m(p, rgb_clip(5, h, w, seed=h), 24, chroma="420")
    ref, fps_ref = VIO.read_video_frames(p, -1, -1, max_res)
    fr, fps = VIO.open_y4m(p, -1, -1, max_res)
    plain, _ = VIO.open_y4m(p)
    assert fps == fps_ref and fr.shape == ref.shape and len(fr) == len(ref) == 5
    assert (fr.out_h, fr.out_w) == ref.shape[1:3] and (fr.h, fr.w) == (h, w) and fr.downscaled
    assert fr.out_h % 2 == 0 and fr.out_w % 2 == 0 and max(fr.out_h, fr.out_w) <= max_res + 1
    assert np.array_equal(fr.rgb(), ref) and np.array_equal(np.asarray(fr), ref)
    assert np.array_equal(fr.rgb([3, 1]), ref[[3, 1]])
    assert fr.frame_stride == plain.frame_stride and np.array_equal(fr.payload(range(5)), plain.payload(range(5)))
    ref2, _ = VIO.read_video_frames(p, 3, 12, max_res)
    fr2, _ = VIO.open_y4m(p, 3, 12, max_res)
    assert fr2.shape == ref2.shape and np.array_equal(fr2.rgb(), ref2)


@pytest.mark.parametrize("max_res", [-1, 104, 1280])
def test_open_y4m_without_a_downscale_is_unchanged(tmp_path, max_res):
    p = str(tmp_path / "clip.y4m")
    VIO.write_y4m(p, rgb_clip(3, 36, 104), 24, chroma="420")
    fr, _ = VIO.open_y4m(p, -1, -1, max_res)
    plain, _ = VIO.open_y4m(p)
    assert fr.shape == plain.shape == (3, 36, 104, 3) and (fr.out_h, fr.out_w) == (36, 104) and not fr.downscaled
    assert np.array_equal(fr.rgb(), VIO.read_y4m(p)[0])


def fake_forward(x):
    return x[:, :, 0] * 0.5 + x[:, :, 1].abs() + x[:, :, 2] * x[:, :, 2] + 2.0


def test_infer_video_depth_takes_downscaling_frames_on_the_cpu(tmp_path):
    from helpers import vda_oracle
    from vda_amd import video as V
    p = str(tmp_path / "clip.y4m")
    VIO.write_y4m(p, rgb_clip(40, 72, 104, seed=2), 24, chroma="420")
    rgb, fps = VIO.read_video_frames(p, -1, -1, 52)
    fr, _ = VIO.open_y4m(p, -1, -1, 52)
    kw = dict(input_size=56, device="cpu", io=vda_oracle.TorchIO, align=V.TorchAlign)
    ref, _ = V.infer_video_depth(fake_forward, rgb, fps, **kw)
    out, _ = V.infer_video_depth(fake_forward, fr, fps, **kw)
    assert out.shape == ref.shape == (40, 36, 52) and np.array_equal(out, ref)


def test_cli_downscale_flag(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import run as cli
    r = subprocess.run([sys.executable, os.path.join(REPO, "run.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--downscale" in r.stdout
    p = str(tmp_path / "wide.y4m")
    VIO.write_y4m(p, rgb_clip(2, 8, 40), 24, chroma="420")
    with pytest.raises(SystemExit) as e:  # the default stays the refusal, with its message
        cli.main(["--input_video", p, "--decode", "device", "--max_res", "32"])
    assert "does not downscale" in str(e.value.code) and "--max_res -1" in str(e.value.code)
    assert "--decode host" in str(e.value.code) and "--downscale device" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cli.parse(["--input_video", p, "--downscale", "device"])
    assert e.value.code not in (0, None) and "--downscale device needs --decode device" in capsys.readouterr().err
    a = cli.parse(["--input_video", p, "--decode", "device", "--downscale", "device", "--max_res", "32"])
    frames, fps = cli.open_input(a)
    assert frames.shape == (2, 6, 32, 3) and (frames.h, frames.w) == (8, 40) and fps == 24
