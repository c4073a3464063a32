"""vda_yuv_downscale on the GPU against the host steps it replaces: ``read_y4m``'s decode, then Pillow's antialiased
bicubic resize (``video_io._resize_rgb``, what ``read_video_frames`` runs for ``max_res``).

Every comparison is equality: Pillow resamples 8-bit images in integer fixed point and the kernel restates that
arithmetic from the same tables.  Shapes are the smallest at which the kernel takes another path: tables clipped
at both edges at once, odd frames in every chroma mode with padded and misaligned payloads, the 4K product ratio,
several tiles each way (tile seams inside the image), a row longer than one pass of a block, either pass skipped,
an axis that grows, the two widths either side of the compiled tap cap, and one frame of each product shape.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import vda_amd
from vda_amd import _lib
from vda_amd import decode as D
from vda_amd import ops
from vda_amd import video_io as VIO
from helpers import device_at_offset

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMAS = ["420", "422", "444", "mono"]
VARIANTS = [dict(), dict(padded=True), dict(offset=1)]  # the payload layouts of test_gpu_decode.py


def on_device(pay, padded=False, offset=0):
    """[n, frame_stride] uint8 on the GPU holding ``pay``: frames padded to a multiple of 16 bytes (the padding
    filled with 0xAA) or back to back, the base ``offset`` bytes into a larger buffer."""
    n, fsz = pay.shape
    stride = (fsz + 15) // 16 * 16 if padded else fsz
    host = np.full((n, stride), 0xAA, np.uint8)
    host[:, :fsz] = pay
    return device_at_offset(host, offset, fill=0x55)


@functools.lru_cache(maxsize=None)
def clip(n, h, w, chroma, kind="random"):
    """Planar frames uint8 [n, payload bytes] and the RGB frames ``read_y4m`` makes of them (read-only).
    ``kind`` "random": every byte value; "binary": Y in {16, 235} and grey chroma, which decodes to 0 / 255."""
    cw, ch, _, _ = D.plane_sizes(h, w, chroma)
    g = np.random.default_rng(n + 3 * h + 7 * w + len(chroma))
    pay = g.integers(0, 256, (n, D.payload_bytes(h, w, chroma)), dtype=np.uint8)
    if kind == "binary":
        pay[:] = 128
        pay[:, :h * w] = np.where(g.integers(0, 2, (n, h * w)) == 1, 235, 16)
    rgb = np.stack([VIO._decode_payload(p, w, h, cw, ch) for p in pay])
    pay.setflags(write=False)
    rgb.setflags(write=False)
    return pay, rgb


def check(n, hw, hw2, chroma="420", variants=({},), kind="random"):
    (h, w), (h2, w2) = hw, hw2
    pay, rgb = clip(n, h, w, chroma, kind)
    ref = torch.from_numpy(VIO._resize_rgb(rgb, h2, w2))
    assert ops.yuv_downscale_accepts(h, w, h2, w2)
    assert _lib.lib().vda_yuv_downscale_workspace(n, h, w, h2, w2) == 0
    for kw in variants:
        out = D.LibDecode.downscale(on_device(pay, **kw), h, w, chroma, (h2, w2))
        assert out.shape == (n, h2, w2, 3) and out.dtype == torch.uint8
        diff = (out.cpu().int() - ref.int()).abs()
        assert torch.equal(out.cpu(), ref), (kw, int(diff.max()), int((diff != 0).sum()))


CASES = [
    (2, (2, 2), (1, 1)),          # one output pixel: tables clipped at both edges
    (2, (3, 5), (2, 2)),
    (2, (36, 104), (12, 34)),     # ratio 3, the 4K product ratio: 13 and 15 taps
    (2, (75, 300), (50, 200)),    # ratio 1.5: four tiles each way, seams inside the image
    (1, (24, 2600), (12, 1280)),  # a row longer than one pass of a block, 21 tiles
    (2, (64, 64), (64, 32)),      # the vertical pass skipped
    (2, (64, 64), (32, 64)),      # the horizontal pass skipped
    (2, (5, 64), (6, 32)),        # an axis growing
]


@pytest.mark.parametrize("n,hw,hw2", CASES, ids=[f"{c[1][0]}x{c[1][1]}-{c[2][0]}x{c[2][1]}" for c in CASES])
def test_downscale_equals_pillow(n, hw, hw2):
    check(n, hw, hw2)


@pytest.mark.parametrize("chroma", CHROMAS)
def test_downscale_odd_frame_all_modes(chroma):
    """37 x 53: odd chroma edges, every plane and row misaligned; also padded frames and a base one byte in."""
    check(3, (37, 53), (16, 22), chroma, VARIANTS)


@pytest.mark.parametrize("chroma", CHROMAS)
def test_downscale_dword_aligned_frames_all_modes(chroma):
    """18 x 40: the width a multiple of 4, so padded frames (and unpadded ones whose payload is a multiple of 4
    bytes) take the kernel's branch-free wide loads; the base one byte in takes the bytewise ones."""
    check(3, (18, 40), (8, 18), chroma, VARIANTS)


def test_downscale_black_and_white_frames():
    """0 / 255 images drive the negative lobes past both clamps, in both passes."""
    pay, rgb = clip(2, 37, 53, "420", "binary")
    assert set(np.unique(rgb)) == {0, 255}
    check(2, (37, 53), (16, 22), "420", VARIANTS, kind="binary")


def test_downscale_either_side_of_the_tap_cap():
    """The widest source the kernel serves for 40 output columns (29 taps) and the next one (31 taps), which
    vda_yuv_downscale_ok, the C entry point and the operator refuse; ``infer_video_depth`` resizes such frames on
    the host."""
    lib = _lib.lib()
    h, w2 = 6, 40
    w = next(w for w in range(w2, 20 * w2) if not lib.vda_yuv_downscale_ok(h, w + 1, h, w2))
    assert w == 7 * w2 and lib.vda_resample_taps(w, w2) == 29 and lib.vda_resample_taps(w + 1, w2) == 31
    check(2, (h, w), (h, w2))
    check(2, (w, h), (w2, h))  # the cap on the vertical axis
    pay, _ = clip(2, h, w + 1, "420")
    assert not ops.yuv_downscale_accepts(h, w + 1, h, w2)
    with pytest.raises(RuntimeError, match="beyond the kernel's ratio"):
        ops.yuv_downscale(on_device(pay), h, w + 1, "420", h, w2)
    kx, bx = (t.cuda() for t in D.resample_tables(w + 1, w2))
    out = torch.zeros(2, h, w2, 3, dtype=torch.uint8, device="cuda")
    dev = on_device(pay)
    rc = lib.vda_yuv_downscale(dev.data_ptr(), 2, h, w + 1, dev.stride(0), _lib.YUV_420, kx.data_ptr(), bx.data_ptr(),
                               None, None, out.data_ptr(), h, w2, None, 0, None)
    assert rc == -22 and b"tap capacity" in lib.vda_last_error()
    torch.cuda.synchronize()
    assert int(out.max()) == 0  # nothing was launched


@pytest.mark.parametrize("hw", [(1080, 1920), (2160, 3840)], ids=["1080p", "4k"])
def test_downscale_product_shapes(hw):
    check(1, hw, (720, 1280))


def test_downscale_is_capturable_and_repeatable():
    """No allocation or synchronisation inside the op once its tables exist: captured in a graph and replayed, it
    gives the same bytes."""
    h, w, h2, w2 = 36, 104, 12, 34
    pay, rgb = clip(2, h, w, "420")
    dev = on_device(pay)
    ref = ops.yuv_downscale(dev, h, w, "420", h2, w2).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ops.yuv_downscale(dev, h, w, "420", h2, w2)
        out.zero_()
        g.replay()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@functools.lru_cache(maxsize=None)
def small_model():
    return vda_amd.build_model("vits", device="cuda")


def write_clip(path):
    fr = np.random.default_rng(11).integers(0, 256, (40, 72, 104, 3), dtype=np.uint8)
    VIO.write_y4m(path, fr, 24, chroma="420")


@pytest.mark.parametrize("stitch", ["host", "device"])
def test_infer_video_depth_on_downscaling_y4m_frames(tmp_path, stitch):
    """ViT-S, synthetic weights, two windows of 72 x 104 frames at max_res 52: the planar upload and the device
    downscale give the depth of the frames the host decodes and resizes."""
    p = str(tmp_path / "clip.y4m")
    write_clip(p)
    rgb, fps = VIO.read_video_frames(p, -1, -1, 52)
    fr, fps2 = VIO.open_y4m(p, -1, -1, 52)
    assert fps == fps2 and fr.shape == rgb.shape == (40, 36, 52, 3) and (fr.h, fr.w) == (72, 104)
    m = small_model()
    ref, _ = m.infer_video_depth(rgb, fps, input_size=56, stitch=stitch)
    out, _ = m.infer_video_depth(fr, fps, input_size=56, stitch=stitch)
    assert out.shape == ref.shape == (40, 36, 52) and np.array_equal(out, ref)


def test_cli_downscale_device_writes_the_same_npz(tmp_path):
    sys.path.insert(0, REPO)
    import run as cli
    p = str(tmp_path / "clip.y4m")
    write_clip(p)
    base = ["--input_video", p, "--encoder", "vits", "--input_size", "56", "--synthetic_weights", "--save_npz",
            "--max_res", "52"]
    cli.main(base + ["--output_dir", str(tmp_path / "host")])
    cli.main(base + ["--output_dir", str(tmp_path / "dev"), "--decode", "device", "--downscale", "device"])
    a = np.load(str(tmp_path / "host" / "VideoDepthAny_vits_clip_depths.npz"))["depths"]
    b = np.load(str(tmp_path / "dev" / "VideoDepthAny_vits_clip_depths.npz"))["depths"]
    assert a.shape == (40, 36, 52) and np.array_equal(a, b)
