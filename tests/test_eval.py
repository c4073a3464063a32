"""Ground-truth evaluation (vda_amd.evaluate) on the CPU: the plain-torch ``TorchEval`` backend against the
reference golden (tests/golden/eval_ref.npz, made by make_eval_golden.py from the reference's
``align_prediction`` and utils/metrics.py), the alignment modes, the CSV writer, the driver with a stand-in
forward, and libvda's new entry points as far as they go without a GPU (argument validation through
ctypes, the Meta shapes of the two torch operators).

Bars against the reference (numpy 2.2.6: its aligned map and metrics are float64, ours fp32 per pixel with
fp64 sums): scale, shift, AbsoluteError, AbsoluteRelative, MeanSquaredError to the project's fp32 tier, 1e-5
relative; SignedRelative, a cancelling mean, to 1e-5 * AbsoluteRelative absolute; Delta1/2/3 equal (the golden
keeps every valid pixel a relative 1e-4 away from the thresholds).  Measured here, all / first-frame
alignment: scale 2.8e-8 / 3.1e-8, shift 4.2e-8 / 2.5e-8, AbsoluteError 2.2e-8 / 5.2e-8, AbsoluteRelative
2.9e-8 / 4.1e-10, MeanSquaredError 4.8e-8 / 1.0e-7 relative, SignedRelative 6.8e-8 / 7.9e-8 absolute
(bar 1.1e-6).
"""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, REPO, vda_oracle
from vda_amd import _lib
from vda_amd import evaluate as E
from vda_amd import video as V

REL_BAR = 1e-5
REL_KEYS = ("AbsoluteError", "AbsoluteRelative", "MeanSquaredError")
DELTAS = ("Delta1", "Delta2", "Delta3")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "eval_ref.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def check_against_reference(res, z, mode, what):
    """The bars of the module docstring; prints every figure before it asserts."""
    ref = dict(zip((str(s) for s in z["metric_names"]), (float(v) for v in z["metrics_" + mode])))
    rs, rh = float(z["scale_" + mode]), float(z["shift_" + mode])
    figs = {"scale": abs(res.scale / rs - 1), "shift": abs(res.shift / rh - 1)}
    figs.update({k: abs(res.metrics[k] / ref[k] - 1) for k in REL_KEYS})
    signed = abs(res.metrics["SignedRelative"] - ref["SignedRelative"])
    print(f"{what}, align={mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()) +
          f", SignedRelative abs {signed:.2e} (bar {REL_BAR * ref['AbsoluteRelative']:.2e}), Delta " +
          " ".join(f"{res.metrics[k]!r}" for k in DELTAS))
    for k, v in figs.items():
        assert v <= REL_BAR, (k, v)
    assert signed <= REL_BAR * ref["AbsoluteRelative"], signed
    for k in DELTAS:
        assert res.metrics[k] == ref[k], (k, res.metrics[k], ref[k])


@pytest.mark.parametrize("mode", ["all", "first"])
def test_torch_eval_matches_reference_golden(golden, mode):
    z = golden
    res = E.evaluate_depth(z["pred"], z["gt"], z["valid"], max_depth=float(z["max_depth"]), align=mode,
                           backend=E.TorchEval)
    assert res.frames == 5 and isinstance(res.scale, float) and set(res.metrics) == set(E.METRICS)
    assert all(v.shape == (5,) for v in res.frame_metrics.values()) and res.frame_sums.shape == (5, 8)
    check_against_reference(res, z, mode, "TorchEval")
    # the whole video's sums are the frames' sums added in frame order
    tot = np.zeros(8)
    for f in range(5):
        tot = tot + res.frame_sums[f]
    assert np.array_equal(tot, res.sums)
    assert res.sums[0] == z["valid"].sum()


def test_per_frame_equals_single_frame_evaluations(golden):
    z = golden
    res = E.evaluate_depth(z["pred"], z["gt"], z["valid"], align="per_frame", return_aligned=True)
    assert res.scale.shape == res.shift.shape == (5,) and isinstance(res.aligned, np.ndarray)
    for f in range(5):
        one = E.evaluate_depth(z["pred"][f:f + 1], z["gt"][f:f + 1], z["valid"][f:f + 1], align="all", return_aligned=True)
        assert one.scale == res.scale[f] and one.shift == res.shift[f]
        assert np.array_equal(one.frame_sums[0], res.frame_sums[f])
        assert np.array_equal(one.aligned[0], res.aligned[f])
        for k in E.METRICS:
            assert one.metrics[k] == res.frame_metrics[k][f]


def test_aligned_map_is_the_reference_formula_in_fp32(golden):
    z = golden
    t = torch.from_numpy(z["pred"])
    res = E.evaluate_depth(t, z["gt"], z["valid"], return_aligned=True)
    assert isinstance(res.aligned, torch.Tensor) and res.aligned.dtype == torch.float32
    scale, shift = np.float32(res.scale), np.float32(res.shift)
    a = np.clip((z["pred"] - shift) / scale, np.float32(0), np.float32(1))
    a = np.where(a == 0, np.float32(1e-4), a)
    p = np.clip(np.float32(1) / a, np.float32(0), np.float32(z["max_depth"]))
    assert p.dtype == np.float32 and np.array_equal(res.aligned.numpy(), p)


def test_frame_without_valid_pixel_and_degenerate_fits(golden):
    z = golden
    valid = z["valid"].copy()
    valid[2] = False
    res = E.evaluate_depth(z["pred"], z["gt"], valid, align="per_frame")
    assert np.isinf(res.scale[2]) and res.shift[2] == 0 and np.isfinite(np.delete(res.scale, 2)).all()
    for k in E.METRICS:
        assert np.isnan(res.frame_metrics[k][2]) and np.isfinite(np.delete(res.frame_metrics[k], 2)).all()
        assert np.isfinite(res.metrics[k])
    res = E.evaluate_depth(z["pred"], z["gt"], np.zeros_like(valid))
    assert np.isinf(res.scale) and res.shift == 0 and all(np.isnan(v) for v in res.metrics.values())
    res = E.evaluate_depth(np.full_like(z["pred"], 3.), z["gt"], z["valid"], return_aligned=True)  # det == 0
    assert np.isinf(res.scale) and res.shift == 0 and (res.aligned == np.float32(z["max_depth"])).all()
    assert all(np.isfinite(v) for v in res.metrics.values())
    with pytest.raises(ValueError):
        E.evaluate_depth(z["pred"], z["gt"], z["valid"], align="last")
    with pytest.raises(ValueError):
        E.evaluate_depth(z["pred"], z["gt"][:4], z["valid"])
    with pytest.raises(ValueError):
        E.evaluate_depth(z["pred"], z["gt"], z["valid"], max_depth=0.)


@pytest.mark.parametrize("mode", ["all", "first", "per_frame"])
def test_gt_at_invalid_pixels_reaches_no_output(golden, mode):
    z = golden
    base = E.evaluate_depth(z["pred"], z["gt"], z["valid"], align=mode, return_aligned=True)
    for poison in (0., np.nan, 1e30):
        gt = np.where(z["valid"], z["gt"], np.float32(poison)).astype(np.float32)
        res = E.evaluate_depth(z["pred"], gt, z["valid"], align=mode, return_aligned=True)
        assert np.array_equal(np.asarray(res.scale), np.asarray(base.scale))
        assert np.array_equal(np.asarray(res.shift), np.asarray(base.shift))
        assert np.array_equal(res.sums, base.sums) and np.array_equal(res.frame_sums, base.frame_sums)
        assert np.array_equal(res.aligned, base.aligned)


def test_uint8_valid_and_none_valid(golden):
    z = golden
    a = E.evaluate_depth(z["pred"], z["gt"], z["valid"])
    b = E.evaluate_depth(z["pred"], z["gt"], z["valid"].astype(np.uint8) * 7)
    assert np.array_equal(a.sums, b.sums) and a.scale == b.scale
    gt = np.where(z["valid"], z["gt"], np.float32(10.)).astype(np.float32)
    c = E.evaluate_depth(z["pred"], gt, None)
    d = E.evaluate_depth(z["pred"], gt, np.ones_like(z["valid"]))
    assert np.array_equal(c.sums, d.sums) and c.sums[0] == z["pred"].size


# ---- CSV --------------------------------------------------------------------------------------
def test_metrics_csv_format(golden, tmp_path):
    z = golden
    assert E.MetricsCSV.HEADER == ["Scene", "#frames", "scale", "shift", "Delta1", "Delta2", "Delta3", "SignedRelative",
                                   "AbsoluteError", "AbsoluteRelative", "MeanSquaredError"]  # utils/metrics.py:10
    path = str(tmp_path / "m.csv")
    log = E.MetricsCSV(path)
    rows = []
    for i, mode in enumerate(("all", "first", "per_frame")):
        res = E.evaluate_depth(z["pred"], z["gt"], z["valid"], align=mode)
        log.add(res, f"scene{i}", frames=5 + i)
        rows.append(res.row(f"scene{i}", 5 + i))
    with pytest.raises(FileExistsError):
        E.MetricsCSV(path).add(res, "again")
    log.summarize(extra_header=["Mean FPS", "Var FPS"], extra_data=[12.5, 0.25])
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == E.MetricsCSV.HEADER and len(lines) == 10
    for got, want in zip(lines[1:4], rows):
        assert got[0] == want[0] and [float(v) for v in got[1:]] == [float(v) for v in want[1:]]
    assert lines[4] == [] and lines[5][0] == "Overall Mean" and lines[6][0] == "Overall Variance"
    cols = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.allclose([float(v) for v in lines[5][1:]], cols.mean(0), rtol=1e-12)  # every row, the first included
    assert np.allclose([float(v) for v in lines[6][1:]], cols.var(0), rtol=1e-9, atol=1e-300)
    assert lines[7] == [] and lines[8] == ["Mean FPS", "Var FPS"] and lines[9] == ["12.5", "0.25"]
    # '#frames' unknown: '--' as the reference writes it; resume() continues an existing file
    path2 = str(tmp_path / "n.csv")
    E.MetricsCSV(path2).add(res, "a")
    E.MetricsCSV(path2).resume().add(res, "b")
    E.MetricsCSV(path2).resume().summarize()
    with open(path2, newline="") as f:
        lines = list(csv.reader(f))
    assert len(lines) == 6 and lines[1][1] == "NotSaved" and lines[4][1] == lines[5][1] == "--"


# ---- driver -----------------------------------------------------------------------------------
class _StandInModel:
    """``infer_video_depth`` / ``infere_single_image`` of the model with a stand-in forward on the CPU."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def fwd(x):  # [B, T, 3, H, W] -> [B, T, H, W]: positive, frame-dependent
        return x.float().abs().mean(2) + 0.5

    def infer_video_depth(self, frames, fps, **kw):
        self.calls.append(("video", dict(kw)))
        return V.infer_video_depth(self.fwd, frames, fps, io=vda_oracle.TorchIO, align=V.TorchAlign, **kw)

    def infere_single_image(self, frames, fps, **kw):
        self.calls.append(("stream", dict(kw)))
        pred, fps = V.infer_video_depth(self.fwd, frames, fps, io=vda_oracle.TorchIO, align=V.TorchAlign,
                                        device=kw["device"], input_size=kw["input_size"], stitch=kw["stitch"])
        return pred[3:], fps  # the streaming driver returns numpy and drops its warm-up frames


def test_evaluate_video_depth_with_stand_in_forward(tmp_path):
    import vda_amd
    g = np.random.default_rng(5)
    n, h, w = 40, 28, 42
    frames = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    gt = g.uniform(2., 60., (n, h, w)).astype(np.float32)
    valid = g.random((n, h, w)) < 0.7
    m = _StandInModel()
    kw = dict(input_size=28, device="cpu")
    res, fps = vda_amd.VideoDepthAnything.evaluate_video_depth(m, frames, 24, gt, valid, max_depth=70., align="first", **kw)
    assert fps == 24 and res.frames == n and m.calls[0][0] == "video"
    assert m.calls[0][1]["stitch"] == "device" and m.calls[0][1]["return_device"] is True
    pred, _ = V.infer_video_depth(m.fwd, frames, 24, io=vda_oracle.TorchIO, align=V.TorchAlign, stitch="device",
                                  return_device=True, **kw)
    want = E.evaluate_depth(pred, gt, valid, max_depth=70., align="first")
    assert res.metrics == want.metrics and res.scale == want.scale and all(np.isfinite(v) for v in res.metrics.values())
    # streaming: fewer predicted frames, the first ground-truth frames are dropped (eval.py:154-159)
    res_s, _ = vda_amd.VideoDepthAnything.evaluate_video_depth(m, frames, 24, gt, valid, max_depth=70., streaming=True, **kw)
    assert m.calls[-1][0] == "stream" and res_s.frames == n - 3
    want = E.evaluate_depth(pred[3:], gt[3:], valid[3:], max_depth=70.)
    assert res_s.metrics == want.metrics
    path = str(tmp_path / "scene.csv")
    E.MetricsCSV(path).add(res, "stand-in", frames=n)
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == E.HEADER and lines[1][0] == "stand-in" and float(lines[1][4]) == res.metrics["Delta1"]


def test_eval_cli_help():
    r = subprocess.run([sys.executable, os.path.join(REPO, "eval.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--gt", "--align", "--max_depth", "--csv", "--scene_name", "--summarize", "--synthetic_weights",
                 "--process_single_image", "--encoder"):
        assert flag in r.stdout, flag


# ---- libvda without a GPU ---------------------------------------------------------------------
def test_eval_symbols_exported():
    lib = _lib.lib()
    for sym in ("vda_depth_eval_workspace", "vda_depth_eval_fit", "vda_depth_eval_metrics"):
        assert sym in _lib.EXPORTED and getattr(lib, sym)


def test_eval_workspace_positive_and_monotone():
    lib = _lib.lib()
    for S in (1, 3, 63, 4099, 48 * 64, 270 * 480, 720 * 1280, 1 << 33):
        prev = 0
        for F in (1, 2, 3, 33, 64, 65535):
            ws = lib.vda_depth_eval_workspace(F, S)
            assert ws > 0 and ws >= prev and ws % 8 == 0, (F, S, ws)  # rounded up to 256 bytes
            assert ws >= F * 13 * 8  # at least one block partial (8) and one frame sum (5) per frame
            prev = ws
    assert lib.vda_depth_eval_workspace(0, 10) == 0 and lib.vda_depth_eval_workspace(1, 0) == 0


def test_eval_argument_validation():
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    F, S = 3, 4099
    ws = lib.vda_depth_eval_workspace(F, S)

    def rejected(fn, args, msg):
        assert fn(*args) == -22
        assert msg in lib.vda_last_error(), lib.vda_last_error()

    # pred, gt, valid, F, S, per_frame, sums, ss, ws, ws_bytes, stream
    ok = [fake, fake, None, F, S, 0, None, fake, fake, ws, None]
    for i in (0, 1, 7, 8):  # pred, gt, ss, ws
        rejected(lib.vda_depth_eval_fit, ok[:i] + [None] + ok[i + 1:], b"null pointer")
    rejected(lib.vda_depth_eval_fit, ok[:3] + [0] + ok[4:], b"F >= 1")
    rejected(lib.vda_depth_eval_fit, ok[:4] + [0] + ok[5:], b"S >= 1")
    rejected(lib.vda_depth_eval_fit, ok[:3] + [65536] + ok[4:], b"65535")
    rejected(lib.vda_depth_eval_fit, ok[:9] + [ws - 8] + ok[10:], b"workspace")
    for i, addr in ((0, 0x1002), (1, 0x1001), (7, 0x1002), (6, 0x1004), (8, 0x1004)):  # pred, gt, ss, sums, ws
        rejected(lib.vda_depth_eval_fit, ok[:i] + [ctypes.c_void_p(addr)] + ok[i + 1:], b"aligned")
    # pred, gt, valid, F, S, ss, ss_per_frame, max_depth, aligned, frame_sums, total, ws, ws_bytes, stream
    ok = [fake, fake, fake, F, S, fake, 0, 80., None, fake, None, fake, ws, None]
    for i in (0, 1, 5, 9, 11):  # pred, gt, ss, frame_sums, ws
        rejected(lib.vda_depth_eval_metrics, ok[:i] + [None] + ok[i + 1:], b"null pointer")
    rejected(lib.vda_depth_eval_metrics, ok[:3] + [0] + ok[4:], b"F >= 1")
    rejected(lib.vda_depth_eval_metrics, ok[:4] + [-1] + ok[5:], b"S >= 1")
    rejected(lib.vda_depth_eval_metrics, ok[:3] + [70000] + ok[4:], b"65535")
    rejected(lib.vda_depth_eval_metrics, ok[:12] + [ws - 8] + ok[13:], b"workspace")
    for bad in (0., -1., float("nan")):
        rejected(lib.vda_depth_eval_metrics, ok[:7] + [bad] + ok[8:], b"max_depth")
    for i, addr in ((0, 0x1002), (1, 0x1003), (5, 0x1001), (8, 0x1002), (9, 0x1004), (10, 0x1004), (11, 0x1004)):
        rejected(lib.vda_depth_eval_metrics, ok[:i] + [ctypes.c_void_p(addr)] + ok[i + 1:], b"aligned")


def test_eval_ops_meta_shapes():
    import vda_amd.torch_ops  # noqa: F401
    p = torch.empty(7, 48, 64, device="meta")
    v = torch.empty(7, 48, 64, device="meta", dtype=torch.uint8)
    ss, sums = torch.ops.vda.depth_eval_fit(p, p, v, False)
    assert ss.shape == (1, 2) and ss.dtype == torch.float32 and sums.shape == (1, 5) and sums.dtype == torch.float64
    ss, sums = torch.ops.vda.depth_eval_fit(p, p, None, True)
    assert ss.shape == (7, 2) and sums.shape == (7, 5)
    fs, tot, al = torch.ops.vda.depth_eval_metrics(p, p, v, ss, 80., True)
    assert fs.shape == (7, 8) and fs.dtype == torch.float64 and tot.shape == (8,) and tot.dtype == torch.float64
    assert al.shape == (7, 48, 64) and al.dtype == torch.float32
    fs, tot, al = torch.ops.vda.depth_eval_metrics(p, p, None, torch.empty(2, device="meta"), 80., False)
    assert fs.shape == (7, 8) and al is None
    with pytest.raises(RuntimeError):
        torch.ops.vda.depth_eval_metrics(p, p, None, torch.empty(3, 2, device="meta"), 80., False)
    with pytest.raises(RuntimeError):
        torch.ops.vda.depth_eval_metrics(p, p, None, ss, 0., False)
    with pytest.raises(RuntimeError):
        torch.ops.vda.depth_eval_fit(p, torch.empty(7, 48, 63, device="meta"), None, False)
    with pytest.raises(NotImplementedError):
        torch.ops.vda.depth_eval_fit(torch.zeros(1, 4), torch.zeros(1, 4), None, False)


def test_eval_op_wrappers_reject_bad_inputs():
    from vda_amd import ops
    p = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError):
        ops.depth_eval_fit(p, p)  # not on the GPU
    with pytest.raises(ValueError):
        ops.depth_eval_metrics(p, p, None, torch.zeros(2))
    with pytest.raises(ValueError):
        E.LibEval.fit(p.double(), p, None)
