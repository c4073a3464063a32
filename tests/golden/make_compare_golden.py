"""Golden fixture for the ground-truth comparison video, generated from the REFERENCE (container only).

Runs the reference's own functions on a synthetic 3 x 6 x 10 scene with two methods, "VDA" (3 frames) and
"VDA_s" (2 frames: a streaming run with one warm-up frame, o = 1):

* scale / shift: ``utils/align.py: frame_align_lstsq`` on the first frame over ``gt < 80``, set up as
  calculate_metrics.py:176-195 sets it up (``calculate_metrics.py`` runs at import and cannot be imported);
* the aligned metric depth: calculate_metrics.py:198-204, restated;
* ``Abs. Error`` / ``MSE``: calculate_metrics.py:219-226, restated (the absolute error of the warmed-up
  method is divided by the size of the whole gt, as there); the per-frame MSE: vis_util.py:96-100, restated;
* the error maps: ``utils/metrics.py: AbsoluteDifference`` of the aligned depth rounded to float32, unmasked and
  with the validity mask.

Writes ``compare_ref.npz``: gt, valid, the raw predictions, and per method scale, shift, aligned (float32),
abs_error, mse, frame_mse, err, err_masked.  Data only.

    python tests/golden/make_compare_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPE = (3, 6, 10)
MAX_DEPTH = 80.0


def scene():
    g = np.random.default_rng(7)
    gt = g.uniform(2., 70., SHAPE).astype(np.float32)
    gt = np.where(g.random(SHAPE) < 0.1, gt * np.float32(1.5), gt).astype(np.float32)  # some beyond max_depth
    valid = g.random(SHAPE) < 0.7
    noise = lambda s: np.float32(0.01) * g.standard_normal(s).astype(np.float32)  # noqa: E731
    vda = (np.float32(37.) / gt + np.float32(2.5) + noise(SHAPE)).astype(np.float32)
    vda_s = (np.float32(21.) / gt[1:] + np.float32(1.25) + noise((SHAPE[0] - 1,) + SHAPE[1:])).astype(np.float32)
    return gt, valid, {"VDA": vda, "VDA_s": vda_s}


def main():
    sys.path.insert(0, REF)
    from utils import metrics as M
    from utils.align import DepthMap, frame_align_lstsq

    gt, valid, preds = scene()
    out = dict(gt=gt, valid=valid, max_depth=np.float64(MAX_DEPTH), numpy_version=np.array(np.__version__),
               methods=np.array(list(preds)))
    for name, raw in preds.items():
        warm = len(gt) - len(raw)
        prediction, ground_truth = raw[0], gt[warm]  # calculate_metrics.py:179-185
        valid_depth = ground_truth < 80.
        gt_mask = np.ma.array(ground_truth, mask=~valid_depth)
        prediction_tmp = DepthMap(np.ma.array(prediction), inverse=True, range=None, scale=None, shift=None)
        gt_depth_tmp = DepthMap(gt_mask, inverse=False, range=None, scale=1, shift=0)
        alignment = frame_align_lstsq(prediction_tmp, gt_depth_tmp)
        scale, shift = alignment.scale, alignment.shift
        a = np.clip((raw - shift) / scale, 0., 1.)  # :198-204
        a = np.where(a == 0., 1e-4, a)
        method_pred = np.clip(1. / a, 0., 80.)
        g = gt[warm:]
        mse = np.mean((method_pred - g) ** 2)  # :221 / :224
        error = np.abs(g - method_pred).sum() / gt.size  # :220 / :226: the size of the whole gt
        frame_mse = np.mean((method_pred - g) ** 2, axis=(1, 2))  # vis_util.py:98-100
        p32 = method_pred.astype(np.float32)
        out.update({f"{name}_raw": raw, f"{name}_scale": np.float64(scale), f"{name}_shift": np.float64(shift),
                    f"{name}_aligned": p32, f"{name}_abs_error": np.float64(error), f"{name}_mse": np.float64(mse),
                    f"{name}_frame_mse": np.asarray(frame_mse, dtype=np.float64),
                    f"{name}_err": np.asarray(M.AbsoluteDifference(p32, g)),
                    f"{name}_err_masked": np.asarray(M.AbsoluteDifference(p32, g, valid_depth=valid[warm:]))})
        print(name, float(scale), float(shift), float(error), float(mse), frame_mse)
    path = os.path.join(HERE, "compare_ref.npz")
    np.savez_compressed(path, **out)
    print(f"compare_ref.npz: numpy {np.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
