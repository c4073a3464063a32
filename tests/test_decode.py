"""The undecoded .y4m input path on the CPU: ``open_y4m`` / ``Y4MFrames`` against ``read_video_frames``, the torch
restatement of the YUV -> RGB arithmetic (``TorchDecode``) against numpy's, the driver taking a ``Y4MFrames`` where
it took RGB frames, the C ABI's argument checks (fake pointers: nothing is launched) and the command line.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import vda_oracle
from vda_amd import _lib
from vda_amd import decode as D
from vda_amd import video as V
from vda_amd import video_io as VIO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = {"420": "C420jpeg", "422": "C422", "444": "C444", "mono": "Cmono"}


def write_stream(path, h, w, chroma, n, seed=0, fps="30000:1001", frame_params=False, cs=None):
    """A hand-assembled YUV4MPEG2 stream of random planes (every byte value, so the clamps are hit); returns the
    payloads uint8 [n, payload bytes]."""
    g = np.random.default_rng(seed)
    planes = g.integers(0, 256, (n, D.payload_bytes(h, w, chroma)), dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{fps} Ip A1:1 {cs or CS[chroma]}\n".encode())
        for i in range(n):
            f.write(b"FRAME Ip Xframe=%d\n" % (10 ** (i % 4)) if frame_params else b"FRAME\n")
            f.write(planes[i].tobytes())
    return planes


def rgb_clip(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_open_y4m_matches_read_video_frames_on_written_files(tmp_path, chroma):
    p = str(tmp_path / "clip.y4m")
    VIO.write_y4m(p, rgb_clip(9, 37, 53), 24, chroma=chroma)
    ref, fps_ref = VIO.read_video_frames(p, -1)
    fr, fps = VIO.open_y4m(p)
    assert isinstance(fr, VIO.Y4MFrames) and fr.chroma == chroma
    assert fps == fps_ref and fr.shape == ref.shape == (9, 37, 53, 3) and len(fr) == 9
    assert np.array_equal(fr.rgb(), ref) and np.array_equal(np.asarray(fr), ref)
    assert np.array_equal(fr.rgb([7, 0, 7]), ref[[7, 0, 7]])
    for length, target in [(4, -1), (-1, 12), (2, 8), (100, 24), (-1, 7)]:  # process_length and frame stride
        ref, fps_ref = VIO.read_video_frames(p, length, target)
        fr, fps = VIO.open_y4m(p, length, target)
        assert fps == fps_ref and fr.shape == ref.shape and np.array_equal(fr.rgb(), ref), (length, target)


@pytest.mark.parametrize("chroma", ["422", "mono", "420", "444"])
@pytest.mark.parametrize("frame_params", [False, True])
def test_open_y4m_on_hand_assembled_streams(tmp_path, chroma, frame_params):
    """Odd sizes (odd chroma edges), frame headers with parameters (payloads not a fixed stride apart)."""
    p = str(tmp_path / "clip.y4m")
    planes = write_stream(p, 37, 53, chroma, 5, seed=3, frame_params=frame_params)
    ref, fps_ref = VIO.read_y4m(p)
    fr, fps = VIO.open_y4m(p)
    assert fps == fps_ref == 30000 / 1001 and fr.shape == ref.shape == (5, 37, 53, 3)
    assert np.array_equal(fr.rgb(), ref)
    pay = fr.payload([4, 1])
    assert pay.shape == (2, fr.frame_stride) and fr.frame_stride % 16 == 0 and fr.frame_stride >= fr.payload_bytes
    assert np.array_equal(pay[:, :fr.payload_bytes], planes[[4, 1]])
    out = np.full((1, fr.frame_stride), 7, np.uint8)
    assert fr.payload([2], out=out) is out and np.array_equal(out[0, :fr.payload_bytes], planes[2])
    with pytest.raises(ValueError):
        fr.payload([0], out=np.zeros((2, fr.frame_stride), np.uint8))


def test_open_y4m_refusals(tmp_path):
    p = str(tmp_path / "deep.y4m")
    write_stream(p, 8, 8, "420", 1, cs="C420p10")
    with pytest.raises(ValueError, match="unsupported y4m colourspace"):
        VIO.open_y4m(p)
    write_stream(p, 8, 8, "mono", 1, cs="Cmono16")
    with pytest.raises(ValueError, match="unsupported y4m colourspace"):
        VIO.open_y4m(p)
    p = str(tmp_path / "cut.y4m")
    write_stream(p, 8, 8, "420", 3)
    data = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(data[:-5])
    with pytest.raises(ValueError, match="truncated"):
        VIO.open_y4m(p)
    with pytest.raises(ValueError):
        VIO.read_y4m(p)
    with open(p, "wb") as f:
        f.write(b"RIFF....AVI \n" + data)
    with pytest.raises(ValueError, match="not a YUV4MPEG2"):
        VIO.open_y4m(p)


def test_torch_decode_equals_numpy_on_every_triple():
    """All 2^24 (y, u, v): the per-operation float32 restatement the kernel follows equals ``_yuv_to_rgb``."""
    a = np.arange(256, dtype=np.uint8)
    y = np.ascontiguousarray(np.broadcast_to(a.reshape(256, 1, 1), (256, 256, 256))).reshape(4096, 4096)
    u = np.ascontiguousarray(np.broadcast_to(a.reshape(1, 256, 1), (256, 256, 256))).reshape(4096, 4096)
    v = np.ascontiguousarray(np.broadcast_to(a.reshape(1, 1, 256), (256, 256, 256))).reshape(4096, 4096)
    ref = VIO._yuv_to_rgb(y, u, v)
    out = D.TorchDecode.convert(torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(v)).numpy()
    assert np.array_equal(out, ref)
    assert ref.min() == 0 and ref.max() == 255  # both clamps are reached


@pytest.mark.parametrize("chroma", ["420", "422", "444", "mono"])
def test_torch_decode_equals_read_y4m(tmp_path, chroma):
    p = str(tmp_path / "clip.y4m")
    write_stream(p, 37, 53, chroma, 3, seed=5)
    ref, _ = VIO.read_y4m(p)
    fr, _ = VIO.open_y4m(p)
    pay = torch.from_numpy(fr.payload(range(3)))
    assert np.array_equal(D.TorchDecode.yuv_to_rgb(pay, 37, 53, chroma).numpy(), ref)
    assert D.payload_bytes(37, 53, chroma) == fr.payload_bytes
    x = D.TorchDecode.preprocess(pay, 37, 53, chroma, (56, 84), V.MEAN, V.STD)
    assert torch.equal(x, vda_oracle.TorchIO.preprocess(torch.from_numpy(ref), (56, 84)))


def fake_forward(x):
    return x[:, :, 0] * 0.5 + x[:, :, 1].abs() + x[:, :, 2] * x[:, :, 2] + 2.0


@pytest.mark.parametrize("stitch", ["host", "device"])
def test_infer_video_depth_takes_y4m_frames_on_the_cpu(tmp_path, stitch):
    """No GPU, or an io without the planar kernel (the oracle's TorchIO): the frames are decoded on the host and
    the result is that of the RGB array."""
    p = str(tmp_path / "clip.y4m")
    VIO.write_y4m(p, rgb_clip(40, 36, 52, seed=2), 24, chroma="420")
    rgb, fps = VIO.read_video_frames(p, -1)
    fr, _ = VIO.open_y4m(p)
    kw = dict(input_size=56, device="cpu", io=vda_oracle.TorchIO, stitch=stitch, align=V.TorchAlign)
    ref, _ = V.infer_video_depth(fake_forward, rgb, fps, **kw)
    out, f = V.infer_video_depth(fake_forward, fr, fps, **kw)
    assert f == fps and out.shape == ref.shape == (40, 36, 52) and np.array_equal(out, ref)


def _rejected(rc, msg):
    assert rc == -22
    err = _lib.lib().vda_last_error()
    assert msg in err, err


def test_c_abi_rejects_bad_arguments():
    """Fake pointers: a launch would fault, so every case must be refused before it."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    mean = (ctypes.c_float * 3)(*V.MEAN)
    std = (ctypes.c_float * 3)(*V.STD)
    h, w = 37, 53
    fsz = D.payload_bytes(h, w, "420")
    rgb = lambda src, N, h, w, stride, chroma, out: lib.vda_yuv_to_rgb(src, N, h, w, stride, chroma, out, None)  # noqa: E731
    _rejected(rgb(None, 2, h, w, fsz, _lib.YUV_420, fake), b"null pointer")
    _rejected(rgb(fake, 2, h, w, fsz, _lib.YUV_420, None), b"null pointer")
    _rejected(rgb(fake, 0, h, w, fsz, _lib.YUV_420, fake), b"empty frame geometry")
    _rejected(rgb(fake, 2, h, w, fsz, 4, fake), b"unknown chroma code")
    _rejected(rgb(fake, 2, h, w, fsz, -1, fake), b"unknown chroma code")
    _rejected(rgb(fake, 2, h, w, fsz - 1, _lib.YUV_420, fake), b"frame_stride")
    _rejected(rgb(fake, 2, h, w, D.payload_bytes(h, w, "420"), _lib.YUV_444, fake), b"frame_stride")
    _rejected(rgb(fake, 65536, h, w, fsz, _lib.YUV_420, fake), b"exceed the launch grid")
    _rejected(rgb(fake, 2, 65536, 2, 4 * 65536, _lib.YUV_MONO, fake), b"exceed the launch grid")

    def pre(src=fake, N=2, h=h, w=w, stride=fsz, chroma=_lib.YUV_420, out=fake, H=56, W=84, mean=mean, std=std,
            ws=None, ws_bytes=0):
        return lib.vda_preprocess_yuv(src, N, h, w, stride, chroma, out, H, W, mean, std, ws, ws_bytes, None)

    _rejected(pre(src=None), b"null pointer")
    _rejected(pre(out=None), b"null pointer")
    _rejected(pre(mean=None), b"null pointer")
    _rejected(pre(std=None), b"null pointer")
    _rejected(pre(W=0), b"empty frame geometry")
    _rejected(pre(chroma=7), b"unknown chroma code")
    _rejected(pre(stride=fsz - 1), b"frame_stride")
    _rejected(pre(N=65536), b"exceed the launch grid")
    _rejected(pre(H=65536), b"exceed the launch grid")
    _rejected(pre(std=(ctypes.c_float * 3)(0.2, 0.0, 0.2)), b"std must be non-zero")
    # 720x1280 -> 56x98 is a composition-route shape: it needs the workspace
    big = D.payload_bytes(720, 1280, "420")
    need = lib.vda_preprocess_yuv_workspace(2, 720, 1280, 56, 98)
    assert need >= 2 * 720 * 1280 * 3
    _rejected(pre(h=720, w=1280, stride=big, H=56, W=98), b"workspace")
    _rejected(pre(h=720, w=1280, stride=big, H=56, W=98, ws=fake, ws_bytes=need - 1), b"workspace")


def test_workspace_query_and_codes():
    ws = _lib.lib().vda_preprocess_yuv_workspace
    assert ws(32, 720, 1280, 518, 924) == 0      # the product ratio: the tile route
    assert ws(1, 1, 1, 14, 14) == 0 and ws(2, 37, 53, 56, 84) == 0 and ws(2, 37, 53, 28, 42) == 0
    assert ws(1, 720, 1280, 56, 98) == (720 * 1280 * 3 + 255) // 256 * 256
    assert ws(0, 720, 1280, 56, 98) == 0
    assert ws(3, 720, 1280, 56, 98) >= 3 * 720 * 1280 * 3
    assert (D.CHROMA["420"], D.CHROMA["422"], D.CHROMA["444"], D.CHROMA["mono"]) == \
        (_lib.YUV_420, _lib.YUV_422, _lib.YUV_444, _lib.YUV_MONO)
    with pytest.raises(ValueError):
        D.chroma_code("411")


def test_meta_shapes_and_no_cpu_kernel():
    import vda_amd.torch_ops  # noqa: F401
    from vda_amd import ops
    pay = torch.empty(3, D.payload_bytes(37, 53, "420") + 9, device="meta", dtype=torch.uint8)
    o = torch.ops.vda.yuv_to_rgb(pay, 37, 53, _lib.YUV_420)
    assert o.shape == (3, 37, 53, 3) and o.dtype == torch.uint8
    x = torch.ops.vda.preprocess_yuv(pay, 37, 53, _lib.YUV_420, 56, 84, list(V.MEAN), list(V.STD))
    assert x.shape == (3, 3, 56, 84) and x.dtype == torch.float32
    with pytest.raises(RuntimeError):  # 4:4:4 needs more bytes than a frame of this payload holds
        torch.ops.vda.yuv_to_rgb(pay, 37, 53, _lib.YUV_444)
    with pytest.raises(NotImplementedError):
        torch.ops.vda.yuv_to_rgb(torch.zeros(1, 64, dtype=torch.uint8), 4, 4, _lib.YUV_444)
    with pytest.raises(ValueError):
        ops.yuv_to_rgb(torch.zeros(1, 64, dtype=torch.uint8), 4, 4, "444")
    with pytest.raises(ValueError):
        ops.preprocess_yuv(torch.zeros(1, 64, dtype=torch.uint8), 4, 4, "444", 14, 14)


def test_cli_help_lists_decode():
    r = subprocess.run([sys.executable, os.path.join(REPO, "run.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--decode" in r.stdout


def test_cli_refuses_what_device_decode_does_not_do(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import run as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--input_video", str(tmp_path / "clip.npz"), "--decode", "device"])
    assert e.value.code not in (0, None) and "needs a .y4m input" in capsys.readouterr().err
    p = str(tmp_path / "wide.y4m")
    VIO.write_y4m(p, rgb_clip(2, 8, 40), 24, chroma="420")
    with pytest.raises(SystemExit) as e:
        cli.main(["--input_video", p, "--decode", "device", "--max_res", "32"])
    assert e.value.code not in (0, None)
    assert "--max_res -1" in str(e.value.code) and "--decode host" in str(e.value.code)
    with pytest.raises(SystemExit):
        cli.main(["--input_video", p, "--decode", "device", "--device", "cpu"])
    assert "CUDA device" in capsys.readouterr().err
