"""vda_yuv_to_rgb / vda_preprocess_yuv on the GPU against the host decode they replace.

Every comparison is equality.  The YUV -> RGB arithmetic rounds every fp32 operation once on both sides (numpy
float32 on the host, IEEE operations without contraction in the kernel), and vda_preprocess_yuv instantiates the
device function vda_preprocess_frames is made of, so its output is that kernel's on the host-decoded frames.
Shapes are the smallest at which the kernels take another path: one pixel, odd sizes (odd chroma edges, every
plane and row misaligned), even sizes, a row longer than a block's pass, several tiles each way at the product's
ratio, up- and downscales, the identity, the product shape, a downscale beyond the tile kernel's footprint and the
two output widths either side of that threshold; a base one byte into its buffer; padded and unpadded frames.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from helpers import device_at_offset
import vda_amd
from vda_amd import _lib
from vda_amd import decode as D
from vda_amd import ops
from vda_amd import video as V
from vda_amd import video_io as VIO

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROMAS = ["420", "422", "444", "mono"]


@functools.lru_cache(maxsize=None)
def clip(n, h, w, chroma):
    """Random planar frames uint8 [n, payload bytes] (every byte value, so both clamps are hit) and the RGB frames
    ``read_y4m`` makes of them (computed once, read-only)."""
    cw, ch, _, _ = D.plane_sizes(h, w, chroma)
    pay = np.random.default_rng(n + 3 * h + 7 * w + len(chroma)).integers(0, 256, (n, D.payload_bytes(h, w, chroma)),
                                                                        dtype=np.uint8)
    rgb = np.stack([VIO._decode_payload(p, w, h, cw, ch) for p in pay])
    pay.setflags(write=False)
    rgb.setflags(write=False)
    return pay, rgb


def on_device(pay, padded=False, offset=0):
    """[n, frame_stride] uint8 on the GPU holding ``pay``: frames padded to a multiple of 16 bytes (the padding
    filled with 0xAA) or back to back, the base ``offset`` bytes into a larger buffer."""
    n, fsz = pay.shape
    stride = (fsz + 15) // 16 * 16 if padded else fsz
    host = np.full((n, stride), 0xAA, np.uint8)
    host[:, :fsz] = pay
    return device_at_offset(host, offset, fill=0x55)


VARIANTS = [dict(), dict(padded=True), dict(offset=1)]


def test_yuv_to_rgb_every_triple():
    """All 2^24 (y, u, v) as one 4096 x 4096 4:4:4 frame: exact .5 ties occur, so the rounding mode matters."""
    a = np.arange(256, dtype=np.uint8)
    y, u, v = (np.ascontiguousarray(np.broadcast_to(a.reshape(s), (256, 256, 256))).reshape(4096, 4096)
               for s in [(256, 1, 1), (1, 256, 1), (1, 1, 256)])
    ref = torch.from_numpy(VIO._yuv_to_rgb(y, u, v))
    pay = torch.from_numpy(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])[None]).cuda()
    out = ops.yuv_to_rgb(pay, 4096, 4096, "444").cpu()
    assert out.shape == (1, 4096, 4096, 3) and torch.equal(out[0], ref)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (37, 53), (36, 52), (3, 1030)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_yuv_to_rgb_equals_read_y4m(hw, chroma):
    h, w = hw
    pay, rgb = clip(3, h, w, chroma)
    ref = torch.from_numpy(np.array(rgb))
    for kw in VARIANTS:
        out = D.LibDecode.yuv_to_rgb(on_device(pay, **kw), h, w, chroma)
        assert out.shape == (3, h, w, 3) and out.dtype == torch.uint8
        assert torch.equal(out.cpu(), ref), kw


def check_preprocess(n, hw, HW, chroma, route, variants=({},)):
    (h, w), (H, W) = hw, HW
    pay, rgb = clip(n, h, w, chroma)
    ws = _lib.lib().vda_preprocess_yuv_workspace(n, h, w, H, W)
    assert (ws > 0) == (route == "composition"), (ws, route)
    ref = ops.preprocess_frames(torch.from_numpy(np.array(rgb)).cuda(), H, W, V.MEAN, V.STD)
    for kw in variants:
        out = ops.preprocess_yuv(on_device(pay, **kw), h, w, chroma, H, W, V.MEAN, V.STD)
        assert out.shape == (n, 3, H, W) and out.dtype == torch.float32
        assert torch.equal(out, ref), (kw, float((out - ref).abs().max()))


PRE_CASES = [
    (2, (1, 1), (14, 14), "tile"),
    (2, (2, 2), (14, 28), "tile"),
    (2, (28, 42), (28, 42), "tile"),           # identity
    (2, (3, 1030), (5, 700), "tile"),          # a row of many tiles, three source rows
    (2, (100, 178), (70, 126), "tile"),        # the product's ratio, several tiles each way
    (2, (720, 1280), (518, 924), "tile"),      # the product shape
    (1, (720, 1280), (56, 98), "composition"),
]


@pytest.mark.parametrize("chroma", ["420", "444"])
@pytest.mark.parametrize("n,hw,HW,route", PRE_CASES, ids=[f"{c[1][0]}x{c[1][1]}-{c[2][0]}x{c[2][1]}" for c in PRE_CASES])
def test_preprocess_yuv_equals_preprocess_frames(n, hw, HW, route, chroma):
    check_preprocess(n, hw, HW, chroma, route)


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("HW", [(56, 84), (28, 42)], ids=["up", "down"])
def test_preprocess_yuv_odd_frame_all_modes(HW, chroma):
    """37 x 53: odd chroma edges, every plane and row misaligned; also padded frames and a base one byte in."""
    check_preprocess(3, (37, 53), HW, chroma, "tile", VARIANTS)


@pytest.mark.parametrize("chroma", ["420", "444"])
def test_preprocess_yuv_either_side_of_the_route_threshold(chroma):
    """For a 100 x 178 source and 70 output rows, the widest output that takes the workspace route and the
    narrowest that takes the tile route, found by asking the library."""
    ws = _lib.lib().vda_preprocess_yuv_workspace
    h, w, H = 100, 178, 70
    assert ws(2, h, w, H, 126) == 0 and ws(2, h, w, H, 14) > 0
    W = next(W for W in range(126, 13, -1) if ws(2, h, w, H, W) > 0)
    assert ws(2, h, w, H, W + 1) == 0
    check_preprocess(2, (h, w), (H, W + 1), chroma, "tile")
    check_preprocess(2, (h, w), (H, W), chroma, "composition")


@functools.lru_cache(maxsize=None)
def small_model():
    return vda_amd.build_model("vits", device="cuda")


def write_clip(path):
    fr = np.random.default_rng(11).integers(0, 256, (40, 36, 52, 3), dtype=np.uint8)
    VIO.write_y4m(path, fr, 24, chroma="420")


@pytest.mark.parametrize("stitch", ["host", "device"])
def test_infer_video_depth_on_y4m_frames(tmp_path, stitch):
    """ViT-S, synthetic weights, two windows: the planar upload gives the depth of the host-decoded frames."""
    p = str(tmp_path / "clip.y4m")
    write_clip(p)
    rgb, fps = VIO.read_y4m(p)
    fr, fps2 = VIO.open_y4m(p)
    assert fps == fps2 and fr.chroma == "420"
    m = small_model()
    ref, _ = m.infer_video_depth(rgb, fps, input_size=56, stitch=stitch)
    out, _ = m.infer_video_depth(fr, fps, input_size=56, stitch=stitch)
    assert out.shape == ref.shape == (40, 36, 52) and np.array_equal(out, ref)


def test_cli_decode_device_writes_the_same_npz(tmp_path):
    sys.path.insert(0, REPO)
    import run as cli
    p = str(tmp_path / "clip.y4m")
    write_clip(p)
    base = ["--input_video", p, "--encoder", "vits", "--input_size", "56", "--synthetic_weights", "--save_npz"]
    cli.main(base + ["--output_dir", str(tmp_path / "host")])
    cli.main(base + ["--output_dir", str(tmp_path / "dev"), "--decode", "device"])
    a = np.load(str(tmp_path / "host" / "VideoDepthAny_vits_clip_depths.npz"))["depths"]
    b = np.load(str(tmp_path / "dev" / "VideoDepthAny_vits_clip_depths.npz"))["depths"]
    assert a.shape == (40, 36, 52) and np.array_equal(a, b)
