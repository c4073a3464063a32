"""Score a predicted video against ground truth, with the reference's metrics and CSV (eval.py), on the device.

    python eval.py --input_video clip.y4m --gt scene.npz --csv metrics.csv --scene_name scene --encoder vitl
    python eval.py ... --csv metrics.csv --summarize          # last scene: also append mean / variance rows

Mirrors FriedFeid/Video-Depth-Anything eval.py:119-188 for one scene per invocation: the model and inference
flags are run.py's (``--process_single_image`` scores the streaming path, whose warm-up frames are dropped
from the ground truth as eval.py:154-159 does).  ``--gt FILE.npz`` stands in for the reference's dataset
loaders: arrays ``depth`` [N, h, w] float (metres) and ``valid_depth`` [N, h, w] bool, optionally
``max_depth``.  The prediction is stitched on the device and scored there (vda_amd.evaluate: vda_depth_eval_fit
/ vda_depth_eval_metrics); only the fit and the metric sums come back to the host.  One row is appended to
``--csv`` (created with the reference's header when it does not exist); ``--summarize`` closes the file with
the mean and variance rows.  ``--align first`` is the reference's ``--align_only_first_frame``.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import run as cli  # noqa: E402  (the shared flags and model construction)


def parse(argv=None):
    p = cli.add_model_arguments(argparse.ArgumentParser(description="Video Depth Anything evaluation (MI355X)"))
    p.add_argument("--gt", type=str, required=True, help=".npz with depth [N, h, w], valid_depth [N, h, w] and optionally max_depth")
    p.add_argument("--align", type=str, default="all", choices=["all", "first", "per_frame"],
                   help="fit scale / shift on all frames, on the first frame only, or on every frame separately")
    p.add_argument("--max_depth", type=float, default=None, help="clip of the metric depth (default: the npz's, else 80)")
    p.add_argument("--csv", type=str, default=None, help="metrics file to append this scene's row to")
    p.add_argument("--scene_name", type=str, default=None)
    p.add_argument("--summarize", action="store_true", help="append the mean / variance rows after this scene's row")
    return cli.check_args(p.parse_args(argv))


def load_gt(path, max_depth=None):
    z = np.load(path, allow_pickle=False)
    gt = np.ascontiguousarray(z["depth"], dtype=np.float32)
    valid = np.ascontiguousarray(z["valid_depth"]).astype(bool)
    if max_depth is None:
        max_depth = float(z["max_depth"]) if "max_depth" in z.files else 80.
    if gt.ndim != 3 or valid.shape != gt.shape:
        raise ValueError(f"{path}: depth must be [N, h, w] and valid_depth the same shape, got {gt.shape} and {valid.shape}")
    return gt, valid, float(max_depth)


def main(argv=None):
    args = parse(argv)
    from vda_amd import video_io as VIO
    from vda_amd.evaluate import MetricsCSV
    model = cli.load_model(args)
    frames, target_fps = VIO.read_video_frames(args.input_video, args.max_len, args.target_fps, args.max_res)
    gt, valid, max_depth = load_gt(args.gt, args.max_depth)
    kw = dict(input_size=args.input_size, device=args.device, fp32=args.fp32)
    if args.process_single_image:
        kw.update(streaming=True, inference_length=args.inference_length, keyframe_list=args.keyframe_list,
                  align_each_new_frame=args.align_each_new_frame, warmup=True, skip_tmp_block=args.skip_tmp_block)
    else:
        kw.update(skip_tmp_block=args.skip_tmp_block and not args.original,
                  windows_per_batch=max(1, args.windows_per_batch))
    t0 = time.time()
    res, _ = model.evaluate_video_depth(frames, target_fps, gt, valid, max_depth=max_depth, align=args.align, **kw)
    dur = time.time() - t0
    scene = args.scene_name or os.path.splitext(os.path.basename(args.input_video))[0]
    print(f"{scene}: {res.frames} of {len(frames)} frames scored in {dur:.2f} s, align={args.align}, "
          f"scale {np.mean(res.scale):.6g} shift {np.mean(res.shift):.6g}")
    for k, v in res.metrics.items():
        print(f"  {k}: {v:.6g}")
    if args.csv:
        log = MetricsCSV(args.csv)
        if os.path.isfile(args.csv):
            log.resume()
        log.add(res, scene, frames=len(frames))
        if args.summarize:
            log.summarize()
    return res


if __name__ == "__main__":
    main()
