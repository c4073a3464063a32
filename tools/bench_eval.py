"""Time the evaluation kernels against masked vda_scale_shift on the same number of elements.

    python tools/bench_eval.py [--frames 64] [--height 720] [--width 1280] [--reps 30] [--out FILE]
    python tools/bench_eval.py --host_reference /path/to/reference [--frames 64 ...]     # CPU, no GPU needed

GPU mode: pred / gt [F, h*w] fp32 and valid uint8 on the device (the recipe of tests/golden/make_eval_golden.py),
then depth_eval_fit, depth_eval_metrics (without and with the aligned map) and masked scale_shift over
n = F*h*w, interleaved, each call between two device events; warm-up calls first; median, min and max of
the repeats, and the achieved GB/s from the bytes the algorithm needs (9 B per element read: two floats and
a mask byte; + 4 B written with the aligned map).  The event interval of the two-to-three-launch entry
points includes their small finalize kernels.

``--host_reference DIR``: wall time of the reference's own host path (``align_prediction`` plus the seven
metric calls of utils/metrics.py, imported from DIR) on arrays of the same size, for context.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scene(F, S, seed=0):
    g = np.random.default_rng(seed)
    gt = g.uniform(2., 80., (F, S)).astype(np.float32)
    gt *= np.where(g.random((F, S), dtype=np.float32) < 0.05, np.float32(1.5), np.float32(1.))
    pred = np.float32(37.) / gt + np.float32(2.5) + np.float32(0.15) * g.standard_normal((F, S), dtype=np.float32)
    valid = g.random((F, S), dtype=np.float32) < 0.6
    gt[~valid] = 0.
    return pred, gt, valid


def host_reference(ref_dir, pred, gt, valid, say):
    sys.path.insert(0, ref_dir)
    from utils import metrics as M
    from utils.align import align_prediction
    t0 = time.perf_counter()
    with np.errstate(divide="ignore", invalid="ignore"):
        p, scale, shift = align_prediction(pred, gt, valid, max_depth=80.)
        t1 = time.perf_counter()
        vals = [1. - M.OutlierRatio(p, gt, threshold=t, valid_depth=valid) for t in (1.25, 1.25 ** 2, 1.25 ** 3)]
        vals += [f(p, gt, valid_depth=valid) for f in (M.SignedRelativeDifference_Error, M.AbsoluteDifference_Error,
                                                       M.AbsoluteRelativeDifference_Error, M.MeanSquared_Error)]
    t2 = time.perf_counter()
    say(f"reference host path (numpy {np.__version__}, {os.cpu_count()} CPUs): align_prediction {t1 - t0:.2f} s, "
        f"seven metric calls {t2 - t1:.2f} s, total {t2 - t0:.2f} s; scale {float(scale):.6g} shift {float(shift):.6g} "
        f"Delta1 {float(vals[0]):.6g} AbsoluteRelative {float(vals[5]):.6g}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    ap.add_argument("--host_reference", type=str, default=None, help="time the reference's numpy path from this checkout")
    a = ap.parse_args(argv)
    F, S = a.frames, a.height * a.width
    n = F * S
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"evaluation kernels at F={F}, S={a.height}x{a.width} (n = {n} elements)")
    pred, gt, valid = scene(F, S)
    if a.host_reference:
        host_reference(a.host_reference, pred.reshape(F, a.height, a.width), gt.reshape(F, a.height, a.width),
                       valid.reshape(F, a.height, a.width), say)
    else:
        import torch
        from vda_amd import ops
        if not torch.cuda.is_available():
            raise RuntimeError("timing needs the GPU (use --host_reference for the CPU context figure)")
        dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        dv = torch.from_numpy(valid.view(np.uint8)).cuda()
        ss, _ = ops.depth_eval_fit(dp, dg, dv)
        cases = {
            "scale_shift (masked)": (9, lambda: ops.scale_shift(dp.view(-1), dg.view(-1), mask=dv.view(-1))),
            "depth_eval_fit": (9, lambda: ops.depth_eval_fit(dp, dg, dv)),
            "depth_eval_fit per_frame": (9, lambda: ops.depth_eval_fit(dp, dg, dv, per_frame=True)),
            "depth_eval_metrics": (9, lambda: ops.depth_eval_metrics(dp, dg, dv, ss)),
            "depth_eval_metrics + aligned": (13, lambda: ops.depth_eval_metrics(dp, dg, dv, ss, want_aligned=True)),
        }
        for _ in range(a.warmup):
            for _, fn in cases.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(a.reps):  # interleaved, so that drift hits every case alike
            for k, (_, fn) in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        say(f"{torch.cuda.get_device_name(0)}; {a.reps} repeats after {a.warmup} warm-up calls, device events, us")
        for k, (bpe, _) in cases.items():
            t = times[k]
            med = statistics.median(t)
            say(f"  {k:30s} median {med:9.1f}  min {min(t):9.1f}  max {max(t):9.1f}   "
                f"{bpe} B/element -> {n * bpe / med / 1e3:7.1f} GB/s at the median")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
