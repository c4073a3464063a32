"""Turn a depth video into one merged, coloured world-space point cloud (.ply), on the device.

    python cloud.py --depth out/clip_depths.npz --gt scene.npz --camera cams.npz --rgb clip.y4m --every 8 --out scene.ply
    python cloud.py --depth scene.npz --intrinsics 725 725 620.5 187 --step 2 --out gt.ply      # metric depth as it is

Mirrors FriedFeid/Video-Depth-Anything datasets/visualisation_utils.py:135-187 (``project_scene_to_3d``) for one
scene: every chosen frame is unprojected through its pinhole intrinsics, moved to world space with its
extrinsics and the clouds are merged in frame order.  With ``--gt`` the prediction (the raw inverse depth
``run.py --save_npz`` wrote) is aligned to the ground truth with ``evaluate_depth(return_aligned=True)`` and the
aligned metric depth is unprojected where it lies: it never leaves the device.  Without ``--gt``, ``--depth`` is
taken as metric depth (key ``depths``, or ``depth`` as in a ground-truth file), which is how to make a cloud of
the ground truth itself.  ``--camera FILE.npz`` holds ``intrinsics`` [N, 3, 3] or [3, 3] and optionally
``extrinsics`` [N, 4, 4] (world to camera unless ``--cam_to_world``); ``--intrinsics fx fy cx cy`` is one pinhole
for all frames and no pose.  Depths of ``max_depth - 1e-4`` and more (the clip of the aligned depth: sky) drop
out, as do zero, negative and non-finite ones.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def parse(argv=None):
    p = argparse.ArgumentParser(description="Point cloud of a depth video (MI355X)")
    p.add_argument("--depth", type=str, required=True, help=".npz with depths [N, h, w]: run.py's output with --gt, else metric depth")
    p.add_argument("--gt", type=str, default=None, help=".npz with depth [N, h, w] (metres), valid_depth and optionally max_depth")
    p.add_argument("--align", type=str, default="all", choices=["all", "first", "per_frame"])
    p.add_argument("--max_depth", type=float, default=None, help="default: the ground truth's, else 80 with --gt and 1000 without")
    cam = p.add_mutually_exclusive_group(required=True)
    cam.add_argument("--camera", type=str, help=".npz with intrinsics [N, 3, 3] or [3, 3] and optionally extrinsics [N, 4, 4]")
    cam.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    p.add_argument("--cam_to_world", action="store_true", help="the extrinsics are camera-to-world (default: world-to-camera)")
    p.add_argument("--rgb", type=str, default=None, help="the input video (.y4m, frame stack, gif ...): colours of the points")
    sel = p.add_mutually_exclusive_group()
    sel.add_argument("--frames", type=int, nargs="+", default=None, help="frame indices, in the order to merge them")
    sel.add_argument("--every", type=int, default=None, help="every K-th frame")
    p.add_argument("--step", type=int, default=1, help="every S-th row and column")
    p.add_argument("--out", type=str, required=True, help="the .ply to write")
    p.add_argument("--device", type=str, default="cuda:0")
    return p.parse_args(argv)


def load_depth(path):
    z = np.load(path, allow_pickle=False)
    key = "depths" if "depths" in z.files else "depth"
    d = np.ascontiguousarray(z[key], dtype=np.float32)
    if d.ndim != 3:
        raise SystemExit(f"{path}: {key} must be [N, h, w], got {d.shape}")
    return d


def main(argv=None):
    args = parse(argv)
    import torch
    from vda_amd import pointcloud as PC
    from vda_amd.evaluate import evaluate_depth
    dev = torch.device(args.device)
    depth = torch.from_numpy(load_depth(args.depth)).to(dev)
    max_depth = args.max_depth
    t0 = time.time()
    if args.gt:
        z = np.load(args.gt, allow_pickle=False)
        gt = np.ascontiguousarray(z["depth"], dtype=np.float32)
        valid = np.ascontiguousarray(z["valid_depth"]).astype(bool) if "valid_depth" in z.files else None
        if max_depth is None:
            max_depth = float(z["max_depth"]) if "max_depth" in z.files else 80.
        skip = gt.shape[0] - depth.shape[0]  # a streaming prediction lacks its warm-up frames (eval.py:154-159)
        if skip < 0:
            raise SystemExit(f"{depth.shape[0]} predicted frames but only {gt.shape[0]} ground-truth frames")
        res = evaluate_depth(depth, gt[skip:], None if valid is None else valid[skip:], max_depth=max_depth,
                             align=args.align, return_aligned=True)
        depth = res.aligned  # metric depth, on the device
        print(f"aligned {res.frames} frames ({args.align}): scale {np.mean(res.scale):.6g} shift {np.mean(res.shift):.6g}, "
              f"AbsoluteRelative {res.metrics['AbsoluteRelative']:.6g}")
    elif max_depth is None:
        max_depth = 1000.
    N = depth.shape[0]
    if args.camera:
        z = np.load(args.camera, allow_pickle=False)
        intr = np.asarray(z["intrinsics"], dtype=np.float32)
        ext = np.asarray(z["extrinsics"], dtype=np.float64) if "extrinsics" in z.files else None
        if intr.ndim == 3 and intr.shape[0] > N:  # the warm-up frames again
            intr = intr[intr.shape[0] - N:]
        if ext is not None and ext.shape[0] > N:
            ext = ext[ext.shape[0] - N:]
    else:
        fx, fy, cx, cy = args.intrinsics
        intr = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
        ext = None
    rgb = None
    if args.rgb:
        from vda_amd import video_io as VIO
        frames, _ = VIO.read_video_frames(args.rgb, -1)
        rgb = np.ascontiguousarray(np.asarray(frames)[-N:], dtype=np.uint8)
        if rgb.shape != tuple(depth.shape) + (3,):
            raise SystemExit(f"--rgb holds frames of shape {rgb.shape}, the depth is {tuple(depth.shape)}")
    frames = args.frames
    if args.every is not None:
        if args.every < 1:
            raise SystemExit("--every takes a positive number")
        frames = list(range(0, N, args.every))
    body = PC.unproject_to_ply_bytes(depth, intr, ext, rgb=rgb, max_depth=max_depth, cam_to_world=args.cam_to_world,
                                     step=args.step, frames=frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    n = PC.write_ply(args.out, body, colors=rgb is not None)
    print(f"wrote {args.out}: {n} points from {len(frames) if frames is not None else N} frames in {time.time() - t0:.2f} s")
    return n


if __name__ == "__main__":
    main()
