"""Ground-truth comparison video of one scene (the reference's calculate_metrics.py for one scene):

    python compare.py --gt scene.npz --pred VDA=out/clip_depths.npz --pred VDA_s=out/clip_single_depths.npz \\
        [--rgb clip.y4m] --output_dir out

Aligns every prediction (the raw inverse depth ``run.py --save_npz`` / ``--save_tiff`` wrote) to the ground
truth on its first frame, appends the reference's log block (Abs. Error / MSE per method,
calculate_metrics.py:228-245) to ``inference_log.txt`` and writes the panel video ``<scene>_<methods>_Vis``:
per frame the RGB frame, the GT depth and its stability image, and per method the error map, the prediction
and its stability image (vda_amd/compare.py; include/vda.h states the deviations from the reference's
matplotlib figure).  A prediction with fewer frames than the ground truth is a streaming run after its
warm-up.  ``--frame_csv`` writes the per-frame MSE series the reference plots as lines, ``--save_gt_stability``
the GT stability image as PNG.  No model is loaded.  On a CUDA device the panels are composed by the libvda
kernels, on ``--device cpu`` by their torch mirror.
"""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    p = argparse.ArgumentParser(description="Ground-truth comparison video of one scene")
    p.add_argument("--gt", type=str, required=True, help=".npz with depth [N, h, w] (metres) and optionally valid_depth")
    p.add_argument("--pred", type=str, action="append", required=True, metavar="NAME=FILE",
                   help="a method's raw inverse depth: the _depths.npz or _depths.tiff of run.py (repeatable, up to 3)")
    p.add_argument("--rgb", type=str, default=None, help="the input video (.y4m, frame stack, gif ...)")
    p.add_argument("--align", type=str, default="first", choices=["all", "first", "per_frame"])
    p.add_argument("--max_depth", type=float, default=80.)
    p.add_argument("--stability_line", type=float, default=0.5, help="image column of the x-t slice, as a fraction of the width")
    p.add_argument("--output_dir", type=str, default="./outputs")
    p.add_argument("--scene_name", type=str, default=None, help="default: the stem of --gt")
    p.add_argument("--fps", type=float, default=None, help="default: the frame rate of --rgb, else 10")
    p.add_argument("--vis_format", type=str, default="y4m", choices=["y4m", "gif", "png", "webp"])
    p.add_argument("--vis_chroma", type=str, default="444", choices=["444", "420"], help="chroma format of a .y4m output")
    p.add_argument("--frame_csv", action="store_true", help="write <scene>_frame_mse.csv: the per-frame MSE per method")
    p.add_argument("--save_gt_stability", action="store_true", help="write <scene>_GT_tmpc_Vis.png")
    p.add_argument("--device", type=str, default="cuda:0")
    return p.parse_args(argv)


def load_pred(path):
    from vda_amd import video_io as VIO
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        return np.ascontiguousarray(np.load(path, allow_pickle=False)["depths"], dtype=np.float32)
    if ext in (".tif", ".tiff"):
        return VIO.load_tiff(path)
    raise ValueError(f"{path}: a prediction is a _depths.npz or _depths.tiff of run.py")


def log_block(scene, result):
    """calculate_metrics.py:223-245 for one scene."""
    lines = []
    for name, m in result.methods.items():
        if m.offset:
            lines.append(f"Assuming wamup length of {m.offset}")
        lines += [f"{scene} {name}: ", "-----------------------", f"Abs. Error: {m.abs_error:.3f}",
                  f"MSE Error: {m.mse:.3f}", ""]
    for name, m in result.methods.items():
        lines += [f"Overall {name}: ", "-----------------------", f"Abs. Error: {m.abs_error:.3f}",
                  f"MSE Error: {m.mse:.3f}", ""]
    return lines


def main(argv=None):
    args = parse(argv)
    from vda_amd import video_io as VIO
    from vda_amd.compare import compare_depths, save_compare_video, stability_image
    preds = {}
    for item in args.pred:
        name, sep, path = item.partition("=")
        if not sep or not name or name in preds:
            raise SystemExit(f"--pred takes NAME=FILE with distinct names, got {item!r}")
        preds[name] = load_pred(path)
    z = np.load(args.gt, allow_pickle=False)
    gt = np.ascontiguousarray(z["depth"], dtype=np.float32)
    valid = np.ascontiguousarray(z["valid_depth"]).astype(bool) if "valid_depth" in z.files else None
    rgb, fps = None, 10.
    if args.rgb:
        rgb, fps = VIO.read_video_frames(args.rgb, -1)
    fps = fps if args.fps is None else args.fps
    scene = args.scene_name or os.path.splitext(os.path.basename(args.gt))[0]
    os.makedirs(args.output_dir, exist_ok=True)
    result = compare_depths(gt, preds, rgb=rgb, valid=valid, max_depth=args.max_depth, align=args.align,
                            stability_line=args.stability_line, device=args.device)
    lines = log_block(scene, result)
    with open(os.path.join(args.output_dir, "inference_log.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    vis = os.path.join(args.output_dir, f"{scene}_{'_'.join(result.methods)}_Vis.{args.vis_format}")
    save_compare_video(vis, result, fps=fps, chroma=args.vis_chroma)
    print(f"wrote {vis}")
    if args.frame_csv:
        path = os.path.join(args.output_dir, f"{scene}_frame_mse.csv")
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["frame"] + list(result.methods))
            for t in range(gt.shape[0]):  # a warmed-up method has no value before its first frame
                w.writerow([t] + [m.frame_mse[t - m.offset] if t >= m.offset else "" for m in result.methods.values()])
        print(f"wrote {path}")
    if args.save_gt_stability:
        from PIL import Image
        path = os.path.join(args.output_dir, f"{scene}_GT_tmpc_Vis.png")
        Image.fromarray(stability_image(result)).save(path)
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
