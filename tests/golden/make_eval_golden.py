"""Golden fixture for the ground-truth evaluation, generated from the REFERENCE (container only).

Runs the reference's own evaluation arithmetic, ``align_prediction`` (utils/align.py:192-218) and the seven
metric functions of utils/metrics.py as ``csv_saver.save_metrics_csv`` (:24-31) calls them, on a synthetic
5 x 48 x 64 scene, once aligned on all frames (eval.py:163) and once on the first frame (eval.py:168-181).
Writes ``eval_ref.npz``: pred, gt, valid, max_depth, and per alignment mode scale, shift and the metrics.

Scene: gt uniform in 2..80 m with about 5 % of the pixels multiplied by 1.5 (beyond max_depth),
pred = 37 / gt + 2.5 + 0.15 N(0, 1), about 60 % of the pixels valid, gt = 0 at the invalid ones.

The seed is searched until, in the reference's own aligned maps (both modes), no valid pixel's
max(p/g, g/p) lies within a relative 1e-4 of 1.25, 1.25^2 or 1.25^3: the Delta counts of an fp32
evaluation then have to match the reference's exactly.

    python tests/golden/make_eval_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPE = (5, 48, 64)
MAX_DEPTH = 80.0
NAMES = ["Delta1", "Delta2", "Delta3", "SignedRelative", "AbsoluteError", "AbsoluteRelative", "MeanSquaredError"]
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
MARGIN = 1e-4


def scene(seed):
    g = np.random.default_rng(seed)
    gt = g.uniform(2., 80., SHAPE).astype(np.float32)
    gt = np.where(g.random(SHAPE) < 0.05, gt * np.float32(1.5), gt).astype(np.float32)
    pred = (np.float32(37.) / gt + np.float32(2.5) + np.float32(0.15) * g.standard_normal(SHAPE).astype(np.float32))
    pred = pred.astype(np.float32)
    valid = g.random(SHAPE) < 0.6
    gt = np.where(valid, gt, np.float32(0.)).astype(np.float32)
    return pred, gt, valid


def threshold_margin(p, gt, valid):
    """Smallest relative distance of a valid pixel's max(p/g, g/p) to a Delta threshold."""
    pv, gv = p[valid].astype(np.float64), gt[valid].astype(np.float64)
    r = np.maximum(pv / gv, gv / pv)
    return min(float(np.min(np.abs(r / t - 1.))) for t in THRESHOLDS)


def main():
    sys.path.insert(0, REF)
    from utils import metrics as M
    from utils.align import align_prediction

    def metrics(p, gt, valid):
        return [1. - M.OutlierRatio(p, gt, threshold=1.25, valid_depth=valid),
                1. - M.OutlierRatio(p, gt, threshold=1.25 ** 2, valid_depth=valid),
                1. - M.OutlierRatio(p, gt, threshold=1.25 ** 3, valid_depth=valid),
                M.SignedRelativeDifference_Error(p, gt, valid_depth=valid),
                M.AbsoluteDifference_Error(p, gt, valid_depth=valid),
                M.AbsoluteRelativeDifference_Error(p, gt, valid_depth=valid),
                M.MeanSquared_Error(p, gt, valid_depth=valid)]

    for seed in range(1, 1000):
        pred, gt, valid = scene(seed)
        with np.errstate(divide="ignore", invalid="ignore"):
            p_all, scale, shift = align_prediction(pred, gt, valid, max_depth=MAX_DEPTH)
            _, scale1, shift1 = align_prediction(pred[0], gt[0], valid[0], max_depth=MAX_DEPTH)
            a = np.clip((pred - shift1) / scale1, 0., 1.)  # eval.py:173-178
            a = np.where(a == 0., 1e-4, a)
            p_first = np.clip(1. / a, 0., MAX_DEPTH)
            margins = threshold_margin(p_all, gt, valid), threshold_margin(p_first, gt, valid)
            print(f"seed {seed}: threshold margins {margins[0]:.2e} (all) {margins[1]:.2e} (first)")
            if min(margins) <= MARGIN:
                continue
            m_all, m_first = metrics(p_all, gt, valid), metrics(p_first, gt, valid)
        break
    else:
        raise RuntimeError("no seed keeps the valid pixels away from the Delta thresholds")
    assert min(margins) > MARGIN
    out = dict(pred=pred, gt=gt, valid=valid, max_depth=np.float64(MAX_DEPTH), seed=np.int64(seed),
               margin=np.float64(min(margins)), numpy_version=np.array(np.__version__),
               scale_all=np.float64(scale), shift_all=np.float64(shift), metrics_all=np.asarray(m_all, dtype=np.float64),
               scale_first=np.float64(scale1), shift_first=np.float64(shift1),
               metrics_first=np.asarray(m_first, dtype=np.float64), metric_names=np.array(NAMES))
    path = os.path.join(HERE, "eval_ref.npz")
    np.savez_compressed(path, **out)
    print(f"eval_ref.npz: seed {seed}, numpy {np.__version__}, {os.path.getsize(path)} bytes")
    print("all:  ", float(scale), float(shift), dict(zip(NAMES, (float(v) for v in m_all))))
    print("first:", float(scale1), float(shift1), dict(zip(NAMES, (float(v) for v in m_first))))


if __name__ == "__main__":
    main()
