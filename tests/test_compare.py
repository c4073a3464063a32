"""The ground-truth comparison video (vda_amd.compare, compare.py): what runs without a GPU.  ``TorchCompare``
is held to the reference's own numbers (tests/golden/compare_ref.npz) and, bit for bit, to a plain numpy
composition of the panels (tests/compare_ref.py); the C ABI's argument checks run before any launch.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import vda_amd  # noqa: F401
from vda_amd import _lib
from vda_amd import compare as CMP
from vda_amd import video_io as VIO
from vda_amd import visualize as VIS

import compare_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_BAR = 1e-5  # tests/test_eval.py: fp32 per-pixel arithmetic against the reference's float64
LAYOUTS = ("hwc", "planar444", "planar420")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "compare_ref.npz"), allow_pickle=False)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


def test_numbers_match_reference(golden):
    z = golden
    names = [str(n) for n in z["methods"]]
    res = CMP.compare_depths(z["gt"], {n: z[f"{n}_raw"] for n in names}, max_depth=float(z["max_depth"]), align="first")
    assert list(res.methods) == names and res.backend is CMP.TorchCompare
    assert [m.offset for m in res.methods.values()] == [0, 1]
    for n, m in res.methods.items():
        for key, got in (("scale", m.scale), ("shift", m.shift), ("abs_error", m.abs_error), ("mse", m.mse),
                         ("frame_mse", m.frame_mse)):
            r = rel(got, z[f"{n}_{key}"])
            print(f"{n} {key}: relative deviation {r:.3e}")
            assert r <= REL_BAR, (n, key, r)
        assert m.frame_mse.shape == (z["gt"].shape[0] - m.offset,)
    # the depth range is over the predictions, not the GT; the error range over the maps as displayed
    al = [m.aligned.numpy() for m in res.methods.values()]
    assert res.depth_range.tolist() == [min(a.min() for a in al), max(a.max() for a in al)]
    er = [np.abs(z["gt"][m.offset:] - m.aligned.numpy()) for m in res.methods.values()]
    assert res.error_range.tolist() == [min(e.min() for e in er), max(e.max() for e in er)]
    fixed = CMP.compare_depths(z["gt"], {"VDA": z["VDA_raw"]}, depth_range=(0., 80.), error_range=[0., 10.])
    assert fixed.depth_range.tolist() == [0., 80.] and fixed.error_range.tolist() == [0., 10.]


def test_error_maps_equal_reference(golden):
    z = golden
    for n in (str(n) for n in z["methods"]):
        p = torch.from_numpy(z[f"{n}_aligned"])
        o = z["gt"].shape[0] - p.shape[0]
        g, v = torch.from_numpy(z["gt"][o:]), torch.from_numpy(z["valid"][o:])
        assert np.array_equal(CMP.TorchCompare.absdiff(p, g).numpy(), z[f"{n}_err"].astype(np.float32))
        masked = CMP.TorchCompare.absdiff(p, g, v).numpy()
        assert np.array_equal(masked, z[f"{n}_err_masked"].astype(np.float32))
        assert CMP.TorchCompare.absdiff_range(p, g, v).tolist() == [masked.min(), masked.max()]


COMPOSE_CASES = [
    # N, H, W, offsets, rgb, valid, stability_line
    (3, 6, 10, (0,), True, False, 0.5),
    (3, 6, 10, (0, 1), True, True, 0.5),
    (3, 37, 53, (0,), True, True, 0.5),      # odd H x W: a 4:2:0 block straddles two tiles
    (3, 37, 53, (0, 1), False, False, 0.999),
    (7, 5, 4, (0, 2), True, False, 0.0),     # N > W: the stability tile skips columns
    (2, 3, 9, (0,), False, True, 0.999),     # N < W: it repeats them
    (1, 1, 1, (0,), True, False, 0.0),
]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", COMPOSE_CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"-M{len(c[3])}")
def test_torch_compose_equals_numpy_composition(case, layout):
    N, H, W, offsets, with_rgb, with_valid, line = case
    gt, preds, rgb, valid = R.scene(N, H, W, offsets, seed=N + H, with_rgb=with_rgb, with_valid=with_valid)
    dr, er = R.ranges(gt, preds, valid)
    res = R.result_of(gt, preds, rgb, valid, dr, er, line, "cpu", CMP.TorchCompare)
    assert res.xstar == int(W * line)
    want = R.to_layout(R.canvas_rgb(gt, preds, rgb, valid, dr, er, res.xstar), layout)
    got = R.frames_of(res, layout, chunk=2)  # chunks: t0 > 0
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)


def test_ranges_of_compare_depths_feed_the_canvas():
    """compare_depths' own ranges (NaNs skipped, mask applied) are the numpy ones."""
    gt, preds, rgb, valid = R.scene(3, 6, 10, (0, 1), seed=5, with_valid=True)
    dr, er = R.ranges(gt, preds, valid)
    T = CMP.TorchCompare
    t = torch.from_numpy
    d = torch.stack([T.range(t(p)) for p in preds])
    assert [float(d[:, 0].min()), float(d[:, 1].max())] == dr.tolist()
    e = torch.stack([T.absdiff_range(t(p), t(gt[3 - len(p):]), t(valid[3 - len(p):])) for p in preds])
    assert [float(e[:, 0].min()), float(e[:, 1].max())] == er.tolist()


def test_rgb_to_yuv_restatement_on_all_triples():
    """Every RGB triple, as one 4096 x 4096 frame, against video_io._rgb_to_yuv."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    got = CMP.TorchCompare.rgb_to_yuv(torch.from_numpy(rgb)).numpy()
    for c, plane in enumerate(VIO._rgb_to_yuv(rgb)):
        assert np.array_equal(got[..., c], plane), "YUV"[c]


def test_named_color_table():
    assert np.array_equal(VIS.named_color_table("Spectral"), VIS.color_table(spectral=True))
    assert np.array_equal(VIS.named_color_table("Spectral", yuv=True), VIS.color_table(spectral=True, yuv=True))
    rd = VIS.named_color_table("RdYlGn")
    assert rd.shape == (256, 3) and rd.dtype == np.uint8 and np.array_equal(rd, R.table("RdYlGn"))
    assert np.array_equal(VIS.named_color_table("RdYlGn", yuv=True), np.stack(VIO._rgb_to_yuv(rd), -1))


def test_symbols_declared_and_exported():
    src = open(os.path.join(REPO, "include", "vda.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in ("vda_tile_size", "vda_depth_absdiff_range_workspace", "vda_depth_absdiff_range",
                "vda_panel_compose_bytes", "vda_panel_compose"):
        assert re.search(rf"\b{sym}\s*\(", code), sym
        assert sym in _lib.EXPORTED
        getattr(_lib.lib(), sym)
    assert _lib.lib().vda_tile_size() == ctypes.sizeof(_lib.Tile)
    for word in ("min(int(x * 256), 255)", "The panels follow the numbers", "no axes, titles, legend or line plot"):
        assert word in src  # the three stated deviations


def _rejected(rc, msg):
    assert rc == -22
    err = _lib.lib().vda_last_error()
    assert msg in err, err


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Fake pointers: a launch would fault."""
    lib = _lib.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001)
    ws = lib.vda_depth_absdiff_range_workspace(5000)
    assert ws > 0 and lib.vda_depth_absdiff_range_workspace(0) == 0
    rng = lib.vda_depth_absdiff_range
    _rejected(rng(None, fake, None, 5000, fake, fake, ws, None), b"null pointer")
    _rejected(rng(fake, None, None, 5000, fake, fake, ws, None), b"null pointer")
    _rejected(rng(fake, fake, None, 5000, None, fake, ws, None), b"null pointer")
    _rejected(rng(fake, fake, None, 5000, fake, None, ws, None), b"null pointer")
    _rejected(rng(fake, fake, None, 0, fake, fake, ws, None), b"n >= 1")
    _rejected(rng(fake, odd, None, 5000, fake, fake, ws, None), b"4-byte aligned")
    _rejected(rng(fake, fake, None, 5000, fake, fake, ws - 1, None), b"workspace")

    nbytes = lib.vda_panel_compose_bytes
    assert nbytes(2, 2, 3, 37, 53, _lib.VIS_HWC) == nbytes(2, 2, 3, 37, 53, _lib.VIS_PLANAR444) == 2 * 3 * 74 * 159
    assert nbytes(2, 2, 3, 37, 53, _lib.VIS_PLANAR420) == 2 * (74 * 159 + 2 * 37 * 80)
    assert nbytes(2, 2, 3, 37, 53, _lib.VIS_INDEX) == 0 and nbytes(0, 2, 3, 37, 53, _lib.VIS_HWC) == 0

    def tile(**kw):
        d = dict(kind=_lib.TILE_DEPTH, row=0, col=0, offset=0, frames=4, lut=0, a=0x1000, range=0x2000)
        d.update(kw)
        return _lib.Tile(**d)

    def compose(tiles, ntiles=None, rows=2, cols=3, F=2, t0=0, N=4, H=6, W=10, xstar=5, lut0=fake, lut1=fake,
                layout=_lib.VIS_HWC, out=fake):
        arr = (_lib.Tile * max(len(tiles), 1))(*tiles)
        return lib.vda_panel_compose(arr, len(tiles) if ntiles is None else ntiles, rows, cols, F, t0, N, H, W, xstar,
                                     lut0, lut1, layout, out, None)

    _rejected(lib.vda_panel_compose(None, 1, 2, 3, 2, 0, 4, 6, 10, 5, fake, fake, _lib.VIS_HWC, fake, None), b"null pointer")
    _rejected(compose([tile()], out=None), b"null pointer")
    _rejected(compose([tile()], ntiles=0), b"1 to 12 tiles")
    _rejected(compose([tile()], ntiles=13), b"1 to 12 tiles")
    _rejected(compose([tile()], rows=5), b"1..4 rows by 1..3 columns")
    _rejected(compose([tile()], cols=4), b"1..4 rows by 1..3 columns")
    _rejected(compose([tile()], F=0), b"F >= 1")
    _rejected(compose([tile()], F=65536, N=70000), b"F <= 65535")
    _rejected(compose([tile()], t0=3), b"t0 + F <= N")
    _rejected(compose([tile()], t0=-1), b"t0 + F <= N")
    _rejected(compose([tile()], xstar=10), b"xstar < W")
    _rejected(compose([tile()], layout=_lib.VIS_INDEX), b"unknown layout")
    _rejected(compose([tile()], rows=4, H=1 << 20, W=1 << 10), b"2^31 pixels")
    _rejected(compose([tile(kind=4)]), b"unknown tile kind")
    _rejected(compose([tile(row=2)]), b"outside the grid")
    _rejected(compose([tile(col=3)]), b"outside the grid")
    _rejected(compose([tile(), tile()]), b"share a grid cell")
    _rejected(compose([tile(a=None)]), b"without a source")
    _rejected(compose([tile(frames=0)]), b"frames >= 1")
    _rejected(compose([tile(offset=-1)]), b"offset >= 0")
    _rejected(compose([tile(range=None)]), b"needs a range")
    _rejected(compose([tile(lut=2)]), b"lut must be 0 or 1")
    _rejected(compose([tile(lut=1)], lut1=None), b"lut that is NULL")
    _rejected(compose([tile()], lut0=None), b"lut that is NULL")
    _rejected(compose([tile(a=0x1002)]), b"4-byte aligned")
    _rejected(compose([tile(kind=_lib.TILE_ERROR)]), b"second operand")
    _rejected(compose([tile(kind=_lib.TILE_ERROR, b=0x3001)]), b"second operand")


def test_op_wrappers_validate_and_meta_shapes():
    import vda_amd.torch_ops  # noqa: F401
    from vda_amd import ops
    meta = dict(device="meta")
    a = torch.empty(3, 37, 53, **meta)
    assert torch.ops.vda.depth_absdiff_range(a, a, None).shape == (2,)
    rgb = torch.empty(3, 37, 53, 3, dtype=torch.uint8, **meta)
    rng, lut = torch.empty(2, **meta), torch.empty(256, 3, dtype=torch.uint8, **meta)
    v = torch.empty(3, 37, 53, dtype=torch.uint8, **meta)

    def op(layout, F=2):
        return torch.ops.vda.panel_compose([rgb, a, a], [None, None, a], [None, None, v], [None, rng, rng], [0, 1, 2],
                                           [0, 0, 1], [0, 1, 0], [0, 0, 0], [0, 0, 1], 2, 3, 37, 53, F, 1, 3, 26, lut, lut,
                                           layout)
    assert op(_lib.VIS_HWC).shape == (2, 74, 159, 3)
    assert op(_lib.VIS_PLANAR444).shape == (2, 3, 74, 159)
    assert op(_lib.VIS_PLANAR420).shape == (2, 74 * 159 + 2 * 37 * 80)
    with pytest.raises(RuntimeError, match="t0 \\+ F <= N"):
        op(_lib.VIS_HWC, F=3)
    with pytest.raises(RuntimeError, match="unknown layout"):
        op(_lib.VIS_INDEX)
    with pytest.raises(NotImplementedError):  # no CPU kernel: no fallback
        torch.ops.vda.depth_absdiff_range(torch.zeros(4), torch.zeros(4), None)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.depth_absdiff_range(torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.panel_compose([dict(kind="depth", row=0, col=0, a=torch.zeros(1, 2, 2), range=torch.zeros(2))], 1, 1, 1, 0, 1, 0)
    with pytest.raises(ValueError, match="1 to 12"):
        ops.panel_compose([], 1, 1, 1, 0, 1, 0)
    with pytest.raises(ValueError, match="layout"):
        ops.panel_compose([dict(kind="depth", row=0, col=0, a=torch.zeros(1, 2, 2))], 1, 1, 1, 0, 1, 0, layout="index")
    with pytest.raises(ValueError, match="t0 \\+ F <= N"):
        ops.panel_compose([dict(kind="depth", row=0, col=0, a=torch.zeros(1, 2, 2))], 1, 1, 2, 0, 1, 0)


def test_compare_depths_validates():
    gt = np.ones((2, 3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="align"):
        CMP.compare_depths(gt, {"a": gt}, align="last")
    with pytest.raises(ValueError, match="1 to 3"):
        CMP.compare_depths(gt, {})
    with pytest.raises(ValueError, match="1 to 3"):
        CMP.compare_depths(gt, {str(i): gt for i in range(4)})
    with pytest.raises(ValueError, match="N_m <= 2"):
        CMP.compare_depths(gt, {"a": np.ones((3, 3, 4), dtype=np.float32)})
    with pytest.raises(ValueError, match="stability_line"):
        CMP.compare_depths(gt, {"a": gt}, stability_line=1.0)
    with pytest.raises(ValueError, match="rgb"):
        CMP.compare_depths(gt, {"a": gt}, rgb=np.zeros((2, 3, 4), dtype=np.uint8))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "compare.py"), *args], capture_output=True, text=True,
                          cwd=REPO)


def test_cli_help():
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for flag in ("--gt", "--pred", "--rgb", "--align", "--max_depth", "--stability_line", "--output_dir", "--vis_format",
                 "--vis_chroma", "--frame_csv", "--save_gt_stability", "--device"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_cli_on_cpu_writes_the_numpy_canvas(tmp_path, golden, chroma):
    """A batch and a streaming prediction as run.py saves them -> the panel .y4m (payloads equal to write_y4m of
    the numpy canvas), the log block, the frame CSV and the GT stability image."""
    z = golden
    gt, valid = z["gt"], z["valid"]
    N, H, W = gt.shape
    g = np.random.default_rng(3)
    rgb = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    np.savez(tmp_path / "scene7.npz", depth=gt, valid_depth=valid)
    VIO.save_npz(str(tmp_path / "batch_depths.npz"), z["VDA_raw"])
    VIO.save_tiff(str(tmp_path / "single_depths.tiff"), z["VDA_s_raw"])
    np.save(tmp_path / "rgb.npy", rgb)
    out = tmp_path / "out"
    r = _cli("--gt", str(tmp_path / "scene7.npz"), "--pred", f"VDA={tmp_path / 'batch_depths.npz'}",
             "--pred", f"VDA_s={tmp_path / 'single_depths.tiff'}", "--rgb", str(tmp_path / "rgb.npy"),
             "--output_dir", str(out), "--vis_chroma", chroma, "--frame_csv", "--save_gt_stability", "--device", "cpu")
    assert r.returncode == 0, r.stderr
    res = CMP.compare_depths(gt, {"VDA": z["VDA_raw"], "VDA_s": z["VDA_s_raw"]}, rgb=rgb, valid=valid)
    preds = [m.aligned.numpy() for m in res.methods.values()]
    canvas = R.canvas_rgb(gt, preds, rgb, valid, res.depth_range.numpy(), res.error_range.numpy(), W // 2)
    VIO.write_y4m(str(tmp_path / "want.y4m"), canvas, 30., chroma)
    vis = out / "scene7_VDA_VDA_s_Vis.y4m"
    assert open(vis, "rb").read() == open(tmp_path / "want.y4m", "rb").read()
    log = open(out / "inference_log.txt").read().splitlines()
    m0, m1 = res.methods["VDA"], res.methods["VDA_s"]
    assert log[:11] == ["scene7 VDA: ", "-----------------------", f"Abs. Error: {m0.abs_error:.3f}",
                        f"MSE Error: {m0.mse:.3f}", "", "Assuming wamup length of 1", "scene7 VDA_s: ",
                        "-----------------------", f"Abs. Error: {m1.abs_error:.3f}", f"MSE Error: {m1.mse:.3f}", ""]
    assert log[11] == "Overall VDA: " and log[16] == "Overall VDA_s: "
    rows = [l.split(",") for l in open(out / "scene7_frame_mse.csv").read().split()]
    assert rows[0] == ["frame", "VDA", "VDA_s"] and len(rows) == 1 + N and rows[1][2] == ""
    assert [float(r[1]) for r in rows[1:]] == m0.frame_mse.tolist()  # fitted over gt < max_depth and valid
    assert [float(r[2]) for r in rows[2:]] == m1.frame_mse.tolist()
    from PIL import Image
    st = np.asarray(Image.open(out / "scene7_GT_tmpc_Vis.png"))
    assert np.array_equal(st, R.table("Spectral")[R.index(gt[:, :, W // 2].T, res.depth_range.numpy())])
