"""Ground-truth evaluation of a predicted video: the reference's ``eval.py:149-181`` without its host passes.

The reference scores a scene in three steps: ``align_prediction`` (utils/align.py:192-218) fits scale and
shift in inverse depth over the valid pixels, converts the aligned prediction to clipped metric depth, and
``csv_saver`` (utils/metrics.py:7-78) computes seven numbers over the valid pixels and appends them to a
CSV: Delta1/2/3, SignedRelative, AbsoluteError, AbsoluteRelative, MeanSquaredError.  It does that in numpy
on the host: masked arrays, an SVD ``lstsq`` on an ``[n_valid, 2]`` matrix and ten full-size passes.

Here the evaluation is two streaming reductions over data that already lies on the device
(``vda_depth_eval_fit`` / ``vda_depth_eval_metrics``, csrc/vda_eval.hip); only ``2 G + 8 F + 8`` numbers come
back to the host.  Per pixel everything is fp32 (one rounding per operation), every sum is fp64 in a fixed
order; see include/vda.h for the arithmetic and where it deviates from the reference (float64 promotion
under numpy >= 2, (inf, 0) for every fit without a solution).

* ``LibEval`` / ``TorchEval`` - the two backends: libvda kernels, and the same arithmetic in plain torch on
  any device (the orchestration and the CPU tests run on it; it is not a fallback of the product path).
* ``evaluate_depth`` - pred / gt / valid -> ``EvalResult`` (scale, shift, the seven metrics, per frame too).
* ``MetricsCSV`` - the reference's CSV format.
* ``evaluate_video_depth`` - inference with the device stitcher, then ``evaluate_depth`` on the device tensor
  (bound to the model as ``VideoDepthAnything.evaluate_video_depth``).
"""
from __future__ import annotations

import csv
import os
from dataclasses import dataclass
from typing import Dict

import numpy as np
import torch

# The reference's CSV header (utils/metrics.py:10) and, from column 4 on, the metric names.
HEADER = ["Scene", "#frames", "scale", "shift", "Delta1", "Delta2", "Delta3", "SignedRelative", "AbsoluteError",
          "AbsoluteRelative", "MeanSquaredError"]
METRICS = tuple(HEADER[4:])
ALIGN_MODES = ("all", "first", "per_frame")


class LibEval:
    """The evaluation arithmetic on libvda kernels (GPU tensors only):
    ``fit(pred, gt, valid, per_frame)`` -> (ss [G, 2] fp32, sums [G, 5] fp64) and
    ``metrics(pred, gt, valid, ss, max_depth, want_aligned)`` -> (frame_sums [F, 8] fp64, total [8] fp64,
    aligned or None), all on the device.  pred / gt [F, ...] fp32, valid bool / uint8 or None."""

    @staticmethod
    def fit(pred, gt, valid, per_frame: bool = False):
        from . import ops
        return ops.depth_eval_fit(pred, gt, valid, per_frame=per_frame)

    @staticmethod
    def metrics(pred, gt, valid, ss, max_depth: float = 80., want_aligned: bool = False):
        from . import ops
        return ops.depth_eval_metrics(pred, gt, valid, ss, max_depth=max_depth, want_aligned=want_aligned)


class TorchEval:
    """``LibEval``'s contract in plain torch on any device: the same fp32 per-pixel operations (every one a
    separate, separately rounded op; divisions by tensors, never by Python scalars, which torch may turn
    into a multiplication by the reciprocal), fp64 sums, frames added in frame order."""

    @staticmethod
    def _valid(pred, valid):
        if valid is None:
            return torch.ones(pred.shape, dtype=torch.bool, device=pred.device)
        return valid != 0

    @staticmethod
    def solve(sums: torch.Tensor) -> torch.Tensor:
        """sums [G, 5] fp64 -> ss [G, 2] fp32; (inf, 0) where the 2x2 system has no solution or c0 == 0."""
        a00, a01, a11, b0, b1 = sums.unbind(-1)
        det = a00 * a11 - a01 * a01
        ok = det != 0
        den = torch.where(ok, det, torch.ones_like(det))
        c0 = (a11 * b0 - a01 * b1) / den
        c1 = (-a01 * b0 + a00 * b1) / den
        ok = ok & (c0 != 0)
        c0s = torch.where(ok, c0, torch.ones_like(c0))
        scale = torch.where(ok, 1. / c0s, torch.full_like(c0, float("inf")))
        shift = torch.where(ok, -c1 / c0s, torch.zeros_like(c0))
        return torch.stack([scale, shift], -1).float()

    @staticmethod
    def fit(pred, gt, valid, per_frame: bool = False):
        F = pred.shape[0]
        p, g = pred.reshape(F, -1), gt.reshape(F, -1)
        m = TorchEval._valid(pred, valid).reshape(F, -1)
        t = torch.ones((), dtype=torch.float32, device=p.device) / g
        zero = torch.zeros((), dtype=torch.float64, device=p.device)
        pd = torch.where(m, p.double(), zero)
        td = torch.where(m, t.double(), zero)
        fs = torch.stack([(pd * pd).sum(1), pd.sum(1), m.double().sum(1), (pd * td).sum(1), td.sum(1)], 1)
        sums = fs if per_frame else _frame_order_sum(fs)[None]
        return TorchEval.solve(sums), sums

    @staticmethod
    def align(pred, ss, max_depth: float):
        """utils/align.py:210-216 in fp32; ss [2] or [F, 2] (per frame) on pred's device."""
        ss = ss.reshape(-1, 2)
        if ss.shape[0] not in (1, pred.shape[0]):
            raise ValueError(f"ss must hold one (scale, shift) or one per frame, got {tuple(ss.shape)}")
        bshape = (-1,) + (1,) * (pred.dim() - 1)
        scale, shift = ss[:, 0].reshape(bshape), ss[:, 1].reshape(bshape)
        f32 = dict(dtype=torch.float32, device=pred.device)
        a = torch.clamp((pred - shift) / scale, 0., 1.)
        a = torch.where(a == 0, torch.tensor(1e-4, **f32), a)
        return torch.clamp(torch.ones((), **f32) / a, 0., float(max_depth))

    @staticmethod
    def metrics(pred, gt, valid, ss, max_depth: float = 80., want_aligned: bool = False):
        F = pred.shape[0]
        p = TorchEval.align(pred, ss, max_depth)
        m = TorchEval._valid(pred, valid).reshape(F, -1)
        pf, g = p.reshape(F, -1), gt.reshape(F, -1)
        d = pf - g
        mx = torch.maximum(pf / g, g / pf)
        rel = d / g
        zero = torch.zeros((), dtype=torch.float64, device=p.device)

        def msum(x):
            return torch.where(m, x.double(), zero).sum(1)

        frame_sums = torch.stack([m.double().sum(1), msum(mx > 1.25), msum(mx > 1.5625), msum(mx > 1.953125),
                                  msum(rel), msum(d.abs()), msum(rel.abs()), msum(d * d)], 1)
        return frame_sums, _frame_order_sum(frame_sums), (p if want_aligned else None)


def _frame_order_sum(fs: torch.Tensor) -> torch.Tensor:
    """[F, K] -> [K]: the rows added one after the other, as the kernels' finalize step adds them."""
    tot = torch.zeros_like(fs[0])
    for f in range(fs.shape[0]):
        tot = tot + fs[f]
    return tot


def metrics_from_sums(sums) -> Dict[str, np.ndarray]:
    """The seven metrics from [..., 8] sums (count, three outlier counts, S d/g, S |d|, S |d|/g, S d^2).
    A count of 0 gives NaN, as the reference's mean of an empty array does."""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = s[..., 0]
        vals = [1. - s[..., 1] / n, 1. - s[..., 2] / n, 1. - s[..., 3] / n, s[..., 4] / n, s[..., 5] / n, s[..., 6] / n,
                s[..., 7] / n]
    return dict(zip(METRICS, vals))


@dataclass
class EvalResult:
    """``scale`` / ``shift``: floats, or [F] arrays with ``align="per_frame"``.  ``metrics``: the seven numbers
    of the whole video keyed by the reference's CSV names; ``frame_metrics``: the same as [F] arrays.
    ``sums`` [8] / ``frame_sums`` [F, 8]: the fp64 sums they come from.  ``aligned``: the aligned metric depth
    (``return_aligned``), a tensor on the input's device when the input was a tensor, else numpy."""
    scale: object
    shift: object
    metrics: Dict[str, float]
    frame_metrics: Dict[str, np.ndarray]
    sums: np.ndarray
    frame_sums: np.ndarray
    frames: int
    aligned: object = None

    def row(self, scene_name: str, frames=None) -> list:
        """One CSV row in ``HEADER`` order (a per-frame scale / shift is written as its mean)."""
        return [scene_name, self.frames if frames is None else frames, float(np.mean(self.scale)),
                float(np.mean(self.shift))] + [self.metrics[k] for k in METRICS]


def _as_tensor(x, dtype, device, name):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a numpy array or a tensor, got {type(x).__name__}")
    if device is not None and x.device != device:
        x = x.to(device)
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.contiguous()


def evaluate_depth(pred, gt, valid=None, max_depth: float = 80., align: str = "all", return_aligned: bool = False,
                   backend=None) -> EvalResult:
    """Score ``pred`` [F, h, w] (relative inverse depth) against ``gt`` [F, h, w] (metres) over ``valid``
    [F, h, w] (bool / uint8, None = all valid) as the reference's eval.py does.

    ``align="all"`` fits one (scale, shift) over the whole video (eval.py:163), ``"first"`` fits frame 0 and
    applies it to every frame (eval.py:168-181), ``"per_frame"`` fits every frame on its own.  A fit without
    a solution reports ``scale = inf``; a frame or video without a valid pixel reports NaN metrics.

    Inputs are numpy arrays or tensors.  A tensor is used where it lies (``pred`` on a GPU: ``LibEval``, no
    copy to the host; anywhere else ``TorchEval``) and ``gt`` / ``valid`` are moved to ``pred``'s device when
    they are not there; the only transfer to the host is the final ss, frame_sums and total."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align must be one of {ALIGN_MODES}, got {align!r}")
    if not float(max_depth) > 0:
        raise ValueError(f"max_depth must be greater than 0, got {max_depth}")
    was_numpy = isinstance(pred, np.ndarray)
    pred = _as_tensor(pred, torch.float32, None, "pred")
    if pred.dim() < 2 or pred.shape[0] < 1 or pred.numel() < 1:
        raise ValueError(f"pred must be [F, h, w] with at least one frame and pixel, got {tuple(pred.shape)}")
    gt = _as_tensor(gt, torch.float32, pred.device, "gt")
    if gt.shape != pred.shape:
        raise ValueError(f"gt has shape {tuple(gt.shape)}, pred {tuple(pred.shape)}")
    if valid is not None:
        valid = _as_tensor(valid, None, pred.device, "valid")
        if valid.dtype not in (torch.bool, torch.uint8) or valid.shape != pred.shape:
            raise ValueError(f"valid must be bool / uint8 with pred's shape, got {valid.dtype} {tuple(valid.shape)}")
    if backend is None:
        backend = LibEval if pred.is_cuda else TorchEval
    if align == "first":
        ss, _ = backend.fit(pred[:1], gt[:1], None if valid is None else valid[:1], False)
    else:
        ss, _ = backend.fit(pred, gt, valid, align == "per_frame")
    frame_sums, total, aligned = backend.metrics(pred, gt, valid, ss, float(max_depth), bool(return_aligned))
    ss_h = ss.reshape(-1, 2).cpu().numpy()
    frame_sums_h, total_h = frame_sums.cpu().numpy(), total.cpu().numpy()
    if align == "per_frame":
        scale, shift = ss_h[:, 0].copy(), ss_h[:, 1].copy()
    else:
        scale, shift = float(ss_h[0, 0]), float(ss_h[0, 1])
    if aligned is not None and was_numpy:
        aligned = aligned.cpu().numpy()
    return EvalResult(scale=scale, shift=shift, metrics={k: float(v) for k, v in metrics_from_sums(total_h).items()},
                      frame_metrics=metrics_from_sums(frame_sums_h), sums=total_h, frame_sums=frame_sums_h,
                      frames=int(pred.shape[0]), aligned=aligned)


class MetricsCSV:
    """The reference's metrics file (``csv_saver``, utils/metrics.py:7-78): the same header row, one row per
    scene, and ``summarize()`` appends a blank line, the 'Overall Mean' row and the 'Overall Variance' row,
    then optionally a blank line, an extra header row and an extra data row.  The file is created with the
    first row; an existing file raises ``FileExistsError`` rather than being overwritten.

    Deviation: the reference's summary skips the first data row (metrics.py:41-50 uses row 0 only to create
    the columns); this one includes every row."""

    HEADER = HEADER

    def __init__(self, path: str):
        self.path = path
        self.initialised = False

    def _init(self):
        if not self.initialised:
            if os.path.isfile(self.path):
                raise FileExistsError(f"csv file does already exist, not overwriting: {self.path}")
            with open(self.path, mode="w", newline="") as f:
                csv.writer(f).writerow(self.HEADER)
            self.initialised = True

    def add(self, result: EvalResult, scene_name: str, frames="NotSaved"):
        """Append the row of one scene; ``frames`` as the reference's ``frames=`` (its eval.py passes the
        number of input frames)."""
        self._init()
        with open(self.path, mode="a", newline="") as f:
            csv.writer(f).writerow(result.row(scene_name, frames))

    def resume(self):
        """Continue a file this class wrote earlier (one command-line invocation per scene)."""
        with open(self.path, mode="r", newline="") as f:
            if next(csv.reader(f), None) != self.HEADER:
                raise ValueError(f"{self.path} does not start with the metrics header")
        self.initialised = True
        return self

    def summarize(self, extra_header=None, extra_data=None):
        data = {k: [] for k in self.HEADER}
        with open(self.path, mode="r", newline="") as f:
            for row in csv.DictReader(f):
                for k in self.HEADER:
                    data[k].append(row[k] if k in ("Scene", "#frames") else float(row[k]))
        mean, var = [], []
        for k in self.HEADER:
            if k == "Scene":
                mean.append("Overall Mean")
                var.append("Overall Variance")
            elif k == "#frames" and "NotSaved" in data[k]:
                mean.append("--")
                var.append("--")
            else:
                col = [float(v) for v in data[k]]
                mean.append(np.mean(col))
                var.append(np.var(col))
        with open(self.path, mode="a", newline="") as f:
            w = csv.writer(f)
            w.writerow([])
            w.writerow(mean)
            w.writerow(var)
            if extra_header is not None and extra_data is not None:
                w.writerow([])
                w.writerow(extra_header)
                w.writerow(extra_data)


def evaluate_video_depth(model, frames, fps, gt, valid=None, *, max_depth: float = 80., align: str = "all",
                         streaming: bool = False, return_aligned: bool = False, backend=None, **infer_kwargs):
    """Predict ``frames`` and score the prediction against ``gt`` / ``valid`` -> (EvalResult, fps).

    Runs ``model.infer_video_depth(frames, fps, stitch="device", return_device=True, **infer_kwargs)`` and
    hands the device tensor to ``evaluate_depth``: the predicted pixels never leave the device.  With
    ``streaming=True`` the prediction comes from ``model.infere_single_image(..., stitch="device")``, which
    returns fewer frames than it was given (its warm-up); the first ``len(gt) - len(pred)`` ground-truth
    frames are dropped then, as eval.py:154-159 does."""
    if streaming:
        pred, fps = model.infere_single_image(frames, fps, stitch="device", **infer_kwargs)
    else:
        pred, fps = model.infer_video_depth(frames, fps, stitch="device", return_device=True, **infer_kwargs)
    skip = len(gt) - len(pred)
    if skip < 0:
        raise ValueError(f"{len(pred)} predicted frames but only {len(gt)} ground-truth frames")
    if skip:
        gt = gt[skip:]
        valid = None if valid is None else valid[skip:]
    if isinstance(pred, np.ndarray):  # the streaming driver returns numpy: score it where the model runs
        pred = torch.from_numpy(pred).to(infer_kwargs.get("device", "cuda"))
    res = evaluate_depth(pred, gt, valid, max_depth=max_depth, align=align, return_aligned=return_aligned,
                         backend=backend)
    return res, fps
