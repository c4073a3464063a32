"""vda_depth_eval_fit / vda_depth_eval_metrics and the evaluation driver on the GPU.

The kernels are pinned exactly where that is possible: the fp64 sums against numpy fp64 sums of the same
fp32 terms (rtol 1e-12, the tolerance of vda_scale_shift's test), the fp32 (scale, shift) against the fp32
rounding of the fp64 closed form (1 ulp), the aligned metric depth bit for bit against separate torch fp32
ops on the GPU, the outlier counts exactly, per-frame results bit for bit against single-frame calls, totals
bit for bit against the frames added in order.  Shapes: the smallest at which head, tail, per-frame and
grid handling can each go wrong; every array starts one element past an allocation boundary, so with S not
a multiple of 4 every frame has another head.  The golden and the driver run through ``LibEval``.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, device_at_offset as offset_by_one, recipe_state_dict
from test_eval import check_against_reference
from vda_amd import _lib
from vda_amd import evaluate as E

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (3, 63), (2, 64), (3, 257), (1, 4099), (33, 48 * 64), (2, 270 * 480)]
MAX_DEPTH = 80.0


def scene(F, S, masked, seed=0):
    """The golden's recipe: gt 2..80 m (5 % of it x 1.5), pred = 37 / gt + 2.5 + 0.15 N(0, 1), 60 % valid,
    gt = 0 at invalid pixels."""
    g = np.random.default_rng(1000 * F + S + seed)
    gt = g.uniform(2., 80., (F, S)).astype(np.float32)
    gt = np.where(g.random((F, S)) < 0.05, gt * np.float32(1.5), gt).astype(np.float32)
    pred = (np.float32(37.) / gt + np.float32(2.5) + np.float32(0.15) * g.standard_normal((F, S)).astype(np.float32))
    pred = pred.astype(np.float32)
    valid = None
    if masked:
        valid = g.random((F, S)) < 0.6
        gt = np.where(valid, gt, np.float32(0.)).astype(np.float32)
    return pred, gt, valid


def on_device(pred, gt, valid):
    dp, dg = offset_by_one(pred), offset_by_one(gt)
    dv = None if valid is None else offset_by_one(valid.astype(np.uint8))
    assert dp.data_ptr() % 16 == 4 and dg.data_ptr() % 16 == 4
    return dp, dg, dv


def fit_sums_ref(pred, gt, valid):
    """numpy fp64 sums of the fp32 inputs (t = 1 / gt is an fp32 division), one frame or many."""
    m = np.ones(pred.shape, dtype=bool) if valid is None else valid.astype(bool)
    with np.errstate(divide="ignore"):
        t = (np.float32(1.) / gt).astype(np.float32)
    P, T = pred[m].astype(np.float64), t[m].astype(np.float64)
    return np.array([np.sum(P * P), np.sum(P), float(m.sum()), np.sum(P * T), np.sum(T)])


def closed_form(sums):
    a00, a01, a11, b0, b1 = (float(v) for v in sums)
    det = a00 * a11 - a01 * a01
    if det == 0:
        return np.float32(np.inf), np.float32(0)
    c0 = (a11 * b0 - a01 * b1) / det
    c1 = (-a01 * b0 + a00 * b1) / det
    if c0 == 0:
        return np.float32(np.inf), np.float32(0)
    return np.float32(1. / c0), np.float32(-c1 / c0)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_fit(dp, dg, dv, F, S, per_frame):
    """vda_depth_eval_fit through the C ABI with NaN canaries behind ss and sums."""
    lib = _lib.lib()
    G = F if per_frame else 1
    ss = torch.full((G * 2 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    sums = torch.full((G * 5 + 3,), float("nan"), dtype=torch.float64, device="cuda")
    wsb = lib.vda_depth_eval_workspace(F, S)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = lib.vda_depth_eval_fit(dp.data_ptr(), dg.data_ptr(), None if dv is None else dv.data_ptr(), F, S,
                                1 if per_frame else 0, sums.data_ptr(), ss.data_ptr(), ws.data_ptr(), wsb, stream_ptr())
    assert rc == 0, lib.vda_last_error()
    torch.cuda.synchronize()
    return ss, sums


def raw_metrics(dp, dg, dv, F, S, ss, with_total=True):
    """vda_depth_eval_metrics through the C ABI with a NaN canary frame behind aligned and frame_sums."""
    lib = _lib.lib()
    aligned = torch.full((F * S + S + 5,), float("nan"), dtype=torch.float32, device="cuda")
    fsum = torch.full((F + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
    total = torch.full((11,), float("nan"), dtype=torch.float64, device="cuda")
    wsb = lib.vda_depth_eval_workspace(F, S)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = lib.vda_depth_eval_metrics(dp.data_ptr(), dg.data_ptr(), None if dv is None else dv.data_ptr(), F, S,
                                    ss.data_ptr(), 1 if ss.numel() == 2 * F and F > 1 else 0, MAX_DEPTH,
                                    aligned.data_ptr(), fsum.data_ptr(), total.data_ptr() if with_total else None,
                                    ws.data_ptr(), wsb, stream_ptr())
    assert rc == 0, lib.vda_last_error()
    torch.cuda.synchronize()
    return aligned, fsum, total


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("F,S", SHAPES)
def test_depth_eval_fit_kernel(F, S, masked):
    from vda_amd import ops
    pred, gt, valid = scene(F, S, masked)
    dp, dg, dv = on_device(pred, gt, valid)
    ss, sums = ops.depth_eval_fit(dp, dg, dv)
    ss2, sums2 = ops.depth_eval_fit(dp, dg, None if dv is None else dv.view(torch.bool))  # bool is viewed as uint8
    assert ss.shape == (1, 2) and ss.dtype == torch.float32 and sums.shape == (1, 5) and sums.dtype == torch.float64
    assert same_bits(ss, ss2) and same_bits(sums, sums2)  # deterministic: the same bits
    ref = fit_sums_ref(pred, gt, valid)
    np.testing.assert_allclose(sums[0].cpu().numpy(), ref, rtol=1e-12, atol=0)
    x0, x1 = closed_form(ref)
    got = ss[0].cpu().numpy()
    print(f"F {F} S {S} masked {masked}: ss {got}, closed form ({x0}, {x1})")
    assert ulps(got[0], x0) <= 1 and ulps(got[1], x1) <= 1
    # per frame: bit for bit F single-frame calls, and near each frame's own numpy sums
    pss, psums = ops.depth_eval_fit(dp, dg, dv, per_frame=True)
    assert pss.shape == (F, 2) and psums.shape == (F, 5)
    for f in range(F):
        one_ss, one_sums = ops.depth_eval_fit(dp[f:f + 1], dg[f:f + 1], None if dv is None else dv[f:f + 1])
        assert same_bits(one_ss[0], pss[f]) and same_bits(one_sums[0], psums[f]), f
    hs = psums.cpu().numpy()
    for f in range(F):
        np.testing.assert_allclose(hs[f], fit_sums_ref(pred[f], gt[f], None if valid is None else valid[f]), rtol=1e-12,
                                   atol=0)
    tot = np.zeros(5)
    for f in range(F):
        tot = tot + hs[f]
    assert np.array_equal(tot, sums[0].cpu().numpy())  # all frames = the frames' sums added in frame order
    # the C ABI writes ss [G, 2] and sums [G, 5] and nothing behind them
    for per_frame, want_ss, want_sums in ((False, ss, sums), (True, pss, psums)):
        G = F if per_frame else 1
        rss, rsums = raw_fit(dp, dg, dv, F, S, per_frame)
        assert same_bits(rss[:2 * G], want_ss.reshape(-1)) and same_bits(rsums[:5 * G], want_sums.reshape(-1))
        assert torch.isnan(rss[2 * G:]).all() and torch.isnan(rsums[5 * G:]).all()


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_depth_eval_fit_every_head_and_tail(off, masked):
    """pred starts ``off`` elements past a 16-byte boundary and frame 1 another S elements on, with frames
    shorter than a head, shorter than one 16-byte group, and with every tail length."""
    from vda_amd import ops
    F = 2
    for S in (1, 2, 3, 4, 5, 7, 8, 1030):
        pred, gt, valid = scene(F, S, masked, seed=off)
        dp, dg = offset_by_one(pred, off), offset_by_one(gt, off)
        dv = None if valid is None else offset_by_one(valid.astype(np.uint8), off)
        assert dp.data_ptr() % 16 == 4 * off
        _, psums = ops.depth_eval_fit(dp, dg, dv, per_frame=True)
        hs = psums.cpu().numpy()
        for f in range(F):
            ref = fit_sums_ref(pred[f], gt[f], None if valid is None else valid[f])
            np.testing.assert_allclose(hs[f], ref, rtol=1e-12, atol=0, err_msg=f"S {S} frame {f}")
            assert hs[f, 2] == ref[2], (S, f, hs[f, 2], ref[2])  # the count: exact


def torch_aligned(dp, ss, F):
    """utils/align.py:210-216 as separate torch fp32 ops on the GPU; ss [1, 2] or [F, 2] on the device."""
    scale, shift = ss[:, 0:1], ss[:, 1:2]
    one = torch.ones((), dtype=torch.float32, device="cuda")
    a = torch.clamp(torch.div(torch.sub(dp, shift), scale), 0., 1.)
    a = torch.where(a == 0, torch.tensor(1e-4, dtype=torch.float32, device="cuda"), a)
    return torch.clamp(torch.div(one, a), 0., MAX_DEPTH)


def metric_sums_ref(p, gt, valid):
    """numpy fp64 sums of the fp32 terms over one frame's valid pixels, from the aligned map p."""
    m = np.ones(p.shape, dtype=bool) if valid is None else valid.astype(bool)
    pv, gv = p[m], gt[m]
    d = (pv - gv).astype(np.float32)
    terms = [(d / gv).astype(np.float32), np.abs(d), (np.abs(d) / gv).astype(np.float32), (d * d).astype(np.float32)]
    return [float(np.sum(t.astype(np.float64))) for t in terms]


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("F,S", SHAPES)
def test_depth_eval_metrics_kernel(F, S, masked):
    from vda_amd import ops
    pred, gt, valid = scene(F, S, masked)
    dp, dg, dv = on_device(pred, gt, valid)
    ss_all, _ = ops.depth_eval_fit(dp, dg, dv)
    ss_pf, _ = ops.depth_eval_fit(dp, dg, dv, per_frame=True)
    if S < 8:  # too few pixels for a fit: a fixed, sensible alignment instead of (inf, 0)
        ss_all = torch.tensor([[37., 2.5]], device="cuda")
        ss_pf = ss_all.repeat(F, 1) * torch.linspace(1., 1.1, F, device="cuda")[:, None]
    for ss in (ss_all, ss_pf):
        fs, tot, al = ops.depth_eval_metrics(dp, dg, dv, ss, max_depth=MAX_DEPTH, want_aligned=True)
        assert fs.shape == (F, 8) and fs.dtype == torch.float64 and tot.shape == (8,) and al.shape == (F, S)
        want = torch_aligned(dp, ss, F)
        assert same_bits(al, want)
        m = torch.ones_like(dp, dtype=torch.bool) if dv is None else dv != 0
        mx = torch.maximum(torch.div(want, dg), torch.div(dg, want))
        counts = torch.stack([m.sum(1)] + [((mx > t) & m).sum(1) for t in (1.25, 1.5625, 1.953125)], 1)
        assert torch.equal(fs[:, :4], counts.double())
        hp, hfs = want.cpu().numpy(), fs.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            for f in range(F):
                ref = metric_sums_ref(hp[f], gt[f], None if valid is None else valid[f])
                np.testing.assert_allclose(hfs[f, 5:], ref[1:], rtol=1e-12, atol=0)
                assert abs(hfs[f, 4] - ref[0]) <= 1e-12 * ref[2], (f, hfs[f, 4], ref[0])  # a cancelling sum
        t = np.zeros(8)
        for f in range(F):
            t = t + hfs[f]
        assert np.array_equal(t, tot.cpu().numpy())  # frames added in frame order, bit for bit
        fs2, tot2, none = ops.depth_eval_metrics(dp, dg, dv, ss, max_depth=MAX_DEPTH)  # aligned = NULL
        assert none is None and same_bits(fs, fs2) and same_bits(tot, tot2)
        # the C ABI writes aligned [F, S], frame_sums [F, 8], total [8] and nothing behind them
        ral, rfs, rtot = raw_metrics(dp, dg, dv, F, S, ss)
        assert same_bits(ral[:F * S], al.reshape(-1)) and torch.isnan(ral[F * S:]).all()
        assert same_bits(rfs[:F], fs) and torch.isnan(rfs[F:]).all()
        assert same_bits(rtot[:8], tot) and torch.isnan(rtot[8:]).all()
        _, rfs, rtot = raw_metrics(dp, dg, dv, F, S, ss, with_total=False)
        assert same_bits(rfs[:F], fs) and torch.isnan(rtot).all()
    # per-frame alignment: frame f as a single-frame call with its own (scale, shift)
    fs, _, al = ops.depth_eval_metrics(dp, dg, dv, ss_pf, max_depth=MAX_DEPTH, want_aligned=True)
    for f in range(F):
        one_fs, one_tot, one_al = ops.depth_eval_metrics(dp[f:f + 1], dg[f:f + 1], None if dv is None else dv[f:f + 1],
                                                         ss_pf[f:f + 1].contiguous(), max_depth=MAX_DEPTH,
                                                         want_aligned=True)
        assert same_bits(one_fs[0], fs[f]) and same_bits(one_tot, fs[f]) and same_bits(one_al[0], al[f])


def test_many_frames_are_added_in_frame_order():
    """More frames than the finalize kernels stage at a time (64), and not a multiple of it."""
    from vda_amd import ops
    F, S = 131, 7
    pred, gt, valid = scene(F, S, True)
    dp, dg, dv = on_device(pred, gt, valid)
    ss, sums = ops.depth_eval_fit(dp, dg, dv)
    pss, psums = ops.depth_eval_fit(dp, dg, dv, per_frame=True)
    hs, tot = psums.cpu().numpy(), np.zeros(5)
    for f in range(F):
        tot = tot + hs[f]
    assert np.array_equal(tot, sums[0].cpu().numpy())
    x0, x1 = closed_form(fit_sums_ref(pred, gt, valid))
    assert ulps(ss[0, 0].item(), x0) <= 1 and ulps(ss[0, 1].item(), x1) <= 1
    fs, total, _ = ops.depth_eval_metrics(dp, dg, dv, ss, max_depth=MAX_DEPTH)
    hfs, tot = fs.cpu().numpy(), np.zeros(8)
    for f in range(F):
        tot = tot + hfs[f]
    assert np.array_equal(tot, total.cpu().numpy()) and total[0].item() == valid.sum()
    one_fs, _, _ = ops.depth_eval_metrics(dp[130:131], dg[130:131], dv[130:131], ss, max_depth=MAX_DEPTH)
    assert same_bits(one_fs[0], fs[130])


@pytest.mark.parametrize("F,S", [(3, 257), (2, 270 * 480)])
def test_poisoned_invalid_pixels_change_no_bit(F, S):
    from vda_amd import ops
    pred, gt, valid = scene(F, S, True)
    dp, dg, dv = on_device(pred, gt, valid)
    ss, sums = ops.depth_eval_fit(dp, dg, dv)
    pss, psums = ops.depth_eval_fit(dp, dg, dv, per_frame=True)
    fs, tot, _ = ops.depth_eval_metrics(dp, dg, dv, ss, max_depth=MAX_DEPTH)
    for gt_poison, pred_poison in ((0., None), (np.nan, None), (np.nan, np.nan), (-1., np.inf)):
        g2 = np.where(valid, gt, np.float32(gt_poison)).astype(np.float32)
        p2 = pred if pred_poison is None else np.where(valid, pred, np.float32(pred_poison)).astype(np.float32)
        dp2, dg2, _ = on_device(p2, g2, valid)
        ss2, sums2 = ops.depth_eval_fit(dp2, dg2, dv)
        pss2, psums2 = ops.depth_eval_fit(dp2, dg2, dv, per_frame=True)
        fs2, tot2, _ = ops.depth_eval_metrics(dp2, dg2, dv, ss2, max_depth=MAX_DEPTH)
        assert same_bits(ss, ss2) and same_bits(sums, sums2) and same_bits(pss, pss2) and same_bits(psums, psums2)
        assert same_bits(fs, fs2) and same_bits(tot, tot2)
        assert torch.isfinite(tot2).all()


def test_degenerate_fits_and_empty_frames():
    from vda_amd import ops
    F, S = 3, 4099
    pred, gt, valid = scene(F, S, True)
    dp, dg, dv = on_device(pred, gt, valid)
    inf0 = [float("inf"), 0.0]
    # no valid pixel at all
    none = torch.zeros(F, S, dtype=torch.uint8, device="cuda")
    ss, sums = ops.depth_eval_fit(dp, dg, none)
    assert ss[0].tolist() == inf0 and sums[0].tolist() == [0.0] * 5
    fs, tot, al = ops.depth_eval_metrics(dp, dg, none, ss, max_depth=MAX_DEPTH, want_aligned=True)
    assert (fs == 0).all() and (tot == 0).all() and (al == MAX_DEPTH).all()
    # a constant prediction: det == 0
    const = offset_by_one(np.full((F, S), 3., dtype=np.float32))
    ss, sums = ops.depth_eval_fit(const, dg, dv)
    assert ss[0].tolist() == inf0 and sums[0, 2].item() == valid.sum()
    fs, tot, al = ops.depth_eval_metrics(const, dg, dv, ss, max_depth=MAX_DEPTH, want_aligned=True)
    assert (al == MAX_DEPTH).all() and torch.isfinite(tot).all() and tot[0].item() == valid.sum()
    # one frame without a valid pixel (and NaN ground truth) among valid ones
    v2, g2 = valid.copy(), gt.copy()
    v2[1] = False
    g2[1] = np.nan
    dp, dg2, dv2 = on_device(pred, g2, v2)
    pss, psums = ops.depth_eval_fit(dp, dg2, dv2, per_frame=True)
    assert pss[1].tolist() == inf0 and psums[1].tolist() == [0.0] * 5
    assert torch.isfinite(pss[0]).all() and torch.isfinite(pss[2]).all()
    ss, sums = ops.depth_eval_fit(dp, dg2, dv2)
    assert torch.isfinite(ss).all() and torch.isfinite(sums).all()
    for s_ in (ss, pss):
        fs, tot, _ = ops.depth_eval_metrics(dp, dg2, dv2, s_, max_depth=MAX_DEPTH)
        assert (fs[1] == 0).all() and torch.isfinite(fs).all() and torch.isfinite(tot).all()
        assert tot[0].item() == v2.sum() and (fs[0, 4:].abs() > 0).all() and (fs[2, 4:].abs() > 0).all()
    res = E.evaluate_depth(dp, dg2, dv2, align="per_frame")
    assert np.isinf(res.scale[1]) and all(np.isnan(v[1]) for v in res.frame_metrics.values())
    assert all(np.isfinite(v) for v in res.metrics.values())
    with pytest.raises(ValueError):
        ops.depth_eval_fit(dp, dg2[:2], dv2)
    with pytest.raises(ValueError):
        ops.depth_eval_metrics(dp, dg2, dv2, ss.cpu())
    with pytest.raises(ValueError):
        ops.depth_eval_metrics(dp, dg2, dv2, ss, max_depth=0.)


@pytest.mark.parametrize("mode", ["all", "first"])
def test_lib_eval_matches_reference_golden(mode):
    z = np.load(os.path.join(GOLDEN, "eval_ref.npz"), allow_pickle=False)
    pred, gt, valid = (torch.from_numpy(z[k]).cuda() for k in ("pred", "gt", "valid"))
    res = E.evaluate_depth(pred, gt, valid, max_depth=float(z["max_depth"]), align=mode, return_aligned=True)
    assert isinstance(res.aligned, torch.Tensor) and res.aligned.is_cuda
    check_against_reference(res, z, mode, "LibEval")
    tor = E.evaluate_depth(pred, gt, valid, max_depth=float(z["max_depth"]), align=mode, return_aligned=True,
                           backend=E.TorchEval)
    assert res.scale == tor.scale and res.shift == tor.shift
    assert torch.equal(res.aligned, tor.aligned)
    assert np.array_equal(res.frame_sums[:, :4], tor.frame_sums[:, :4]) and np.array_equal(res.sums[:4], tor.sums[:4])
    np.testing.assert_allclose(res.frame_sums[:, 5:], tor.frame_sums[:, 5:], rtol=1e-12, atol=0)
    np.testing.assert_allclose(res.sums[5:], tor.sums[5:], rtol=1e-12, atol=0)
    assert (np.abs(res.frame_sums[:, 4] - tor.frame_sums[:, 4]) <= 1e-12 * tor.frame_sums[:, 6]).all()
    assert abs(res.sums[4] - tor.sums[4]) <= 1e-12 * tor.sums[6]


def test_evaluate_video_depth_on_gpu():
    import vda_amd
    z = np.load(os.path.join(GOLDEN, "video_vits_57f.npz"), allow_pickle=False)
    frames, depth_ref, meta = z["frames"], z["depth"], json.loads(str(z["meta"]))
    m = vda_amd.build_model("vits", state_dict=recipe_state_dict("vits"), device="cuda")
    g = np.random.default_rng(57)
    lo, hi = float(depth_ref.min()), float(depth_ref.max())
    inv = (depth_ref - lo) / max(hi - lo, 1e-12) * (0.5 - 1. / 60.) + 1. / 60.   # inverse depth of 2 .. 60 m
    gt = (1. / inv * (1. + 0.05 * g.standard_normal(depth_ref.shape))).astype(np.float32)
    valid = g.random(depth_ref.shape) < 0.6
    gt = np.where(valid, gt, np.float32(0.)).astype(np.float32)
    kw = dict(input_size=meta["input_size"], device="cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pred, _ = m.infer_video_depth(frames, meta["fps"], stitch="device", return_device=True, **kw)
    torch.cuda.synchronize()
    peak_infer = torch.cuda.max_memory_allocated() - base
    want = E.evaluate_depth(pred, gt, valid, max_depth=MAX_DEPTH)
    del pred
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    res, fps = m.evaluate_video_depth(frames, meta["fps"], gt, valid, max_depth=MAX_DEPTH, **kw)
    torch.cuda.synchronize()
    peak_eval = torch.cuda.max_memory_allocated() - base
    print(f"evaluate_video_depth 57 frames: scale {res.scale:.5g} shift {res.shift:.5g} {res.metrics}; "
          f"peak {peak_eval} B against inference alone {peak_infer} B + gt {gt.nbytes} B + valid {valid.nbytes} B")
    assert fps == meta["fps"] and res.frames == len(frames)
    assert all(np.isfinite(v) for v in res.metrics.values()) and np.isfinite(res.scale) and np.isfinite(res.shift)
    assert 0.5 < res.metrics["Delta1"] <= 1.0  # gt is the golden depth up to scale, shift and 5 % noise
    assert res.metrics == want.metrics and res.scale == want.scale and res.shift == want.shift
    assert np.array_equal(res.frame_sums, want.frame_sums)
    assert peak_eval <= peak_infer + gt.nbytes + valid.nbytes, (peak_eval, peak_infer)


def test_eval_cli_end_to_end(tmp_path):
    """eval.py with synthetic weights: a long-video scene and a streaming scene (39 of 40 frames: the first
    ground-truth frame is dropped) appended to one CSV, the second invocation closing it."""
    import csv
    import importlib
    import vda_amd
    from vda_amd import video_io as VIO
    cli = importlib.import_module("eval")
    g = np.random.default_rng(40)
    n, h, w = 40, 42, 56
    frames = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    clip, gtp, out = str(tmp_path / "clip.y4m"), str(tmp_path / "scene.npz"), str(tmp_path / "metrics.csv")
    VIO.write_y4m(clip, frames, 24)
    gt = g.uniform(2., 90., (n, h, w)).astype(np.float32)
    valid = g.random((n, h, w)) < 0.6
    np.savez(gtp, depth=gt, valid_depth=valid, max_depth=np.float64(70.))
    base = ["--input_video", clip, "--gt", gtp, "--encoder", "vits", "--input_size", "56", "--synthetic_weights",
            "--csv", out]
    stream = ["--process_single_image", "--keyframe_list", "2", "12", "--align_each_new_frame"]
    r1 = cli.main(base + ["--scene_name", "long", "--align", "first"])
    r2 = cli.main(base + stream + ["--scene_name", "stream", "--summarize"])
    assert r1.frames == n and r2.frames == n - 1
    decoded, fps = VIO.read_video_frames(clip, -1, -1, 1280)
    m = vda_amd.build_model("vits", device="cuda")
    w1, _ = m.evaluate_video_depth(decoded, fps, gt, valid, max_depth=70., align="first", input_size=56)
    w2, _ = m.evaluate_video_depth(decoded, fps, gt, valid, max_depth=70., streaming=True, input_size=56,
                                   keyframe_list=[2, 12], align_each_new_frame=True)
    assert r1.metrics == w1.metrics and r1.scale == w1.scale and r2.metrics == w2.metrics and r2.scale == w2.scale
    assert all(np.isfinite(v) for v in r1.metrics.values()) and all(np.isfinite(v) for v in r2.metrics.values())
    assert r2.sums[0] == valid[1:].sum()
    with open(out, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == E.HEADER and len(lines) == 6 and lines[3] == []
    assert lines[1][:2] == ["long", str(n)] and lines[2][:2] == ["stream", str(n)]
    assert [float(v) for v in lines[1][2:]] == [float(v) for v in r1.row("long")[2:]]
    assert lines[4][0] == "Overall Mean" and lines[5][0] == "Overall Variance"
    assert float(lines[4][4]) == np.mean([r1.metrics["Delta1"], r2.metrics["Delta1"]])
