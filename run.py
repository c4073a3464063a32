"""Command-line driver with the reference's flags (run.py), on the MI355X path.

    python run.py --input_video clip.y4m --output_dir out --encoder vitl [--process_single_image ...]

Mirrors FriedFeid/Video-Depth-Anything run.py:27-166: loads ``checkpoints/video_depth_anything_<enc>.pth``
(``torch.load(weights_only=True)``, strict), reads the video (vda_amd.video_io: .y4m / frame stacks /
Pillow formats; decord when installed), runs ``infer_video_depth`` (or ``infere_single_image`` with
``--process_single_image``), and writes the requested outputs (npz ``depths``, float32 TIFF stack,
source / visualisation videos as .y4m, or .gif/.png/.webp via ``--vis_format``).  ``--synthetic_weights``
uses the deterministic recipe of vda_amd.weights when no checkpoint is available (this image has none).
``--fp32`` selects the fp32 kernels (the reference's autocast-off path); the default is fp16 compute.
``--stitch device`` aligns and stitches on the device (vda_scale_shift / vda_depth_align); the default is the host.
``--vis device`` (with ``--stitch device``) colours the ``--save_vis`` video on the device (vda_depth_range /
vda_depth_colorize) and writes the same file as the host path; ``--vis_chroma 420`` writes a 4:2:0 .y4m.
``--decode device`` (a .y4m input) indexes the file instead of decoding it: every window batch uploads the planar
YUV bytes of its frames and vda_preprocess_yuv decodes them into the network input; the depth is the same.
``--downscale device`` (with ``--decode device``) also makes the ``--max_res`` downscale on the device
(vda_yuv_downscale, Pillow's antialiased bicubic in its own integer arithmetic): 1080p and 4K files take that path too.
"""
import argparse
import os
import sys
import time
from datetime import datetime

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def add_model_arguments(p):
    """The model, input and inference flags (eval.py takes the same ones)."""
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--input_video", type=str, required=True)
    p.add_argument("--process_single_image", action="store_true")
    p.add_argument("--inference_length", type=int, default=32)
    p.add_argument("--keyframe_list", type=int, nargs="+", default=[20])
    p.add_argument("--align_each_new_frame", action="store_true")
    p.add_argument("--original", action="store_true")
    p.add_argument("--skip_tmp_block", action="store_true")
    p.add_argument("--input_size", type=int, default=518)
    p.add_argument("--max_res", type=int, default=1280)
    p.add_argument("--encoder", type=str, default="vitl", choices=["vits", "vitb", "vitl", "vitg"])
    p.add_argument("--max_len", type=int, default=-1)
    p.add_argument("--target_fps", type=int, default=-1)
    p.add_argument("--fp32", action="store_true")
    p.add_argument("--checkpoint", type=str, default=None)
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--windows_per_batch", type=int, default=1,
                   help="windows per forward in the long-video path (2: ~3%% more frames/s on MI355X)")
    return p


def add_arguments(p):
    """Every flag of this tool: the model / inference flags and the output flags."""
    add_model_arguments(p)
    p.add_argument("--output_dir", type=str, default="./outputs")
    p.add_argument("--grayscale", action="store_true")
    p.add_argument("--save_npz", action="store_true")
    p.add_argument("--save_tiff", action="store_true")
    p.add_argument("--save_orig", action="store_true")
    p.add_argument("--save_vis", action="store_true")
    p.add_argument("--save_stats", action="store_true")
    p.add_argument("--vis_format", type=str, default="y4m", choices=["y4m", "gif", "png", "webp", "mp4"])
    p.add_argument("--stitch", type=str, default="host", choices=["host", "device"],
                   help="where windows (or, with --process_single_image --align_each_new_frame, new frames) are "
                        "aligned and stitched: on the host as the reference does, or on the device")
    p.add_argument("--vis", type=str, default="host", choices=["host", "device"],
                   help="where --save_vis colours the depth: in numpy on the host as the reference does, or on the "
                        "device (needs --stitch device; the same file, without the host passes)")
    p.add_argument("--vis_chroma", type=str, default="444", choices=["444", "420"],
                   help="chroma format of a .y4m visualisation: 4:4:4 (3 B per pixel) or 4:2:0 (1.5 B per pixel)")
    p.add_argument("--decode", type=str, default="host", choices=["host", "device"],
                   help="where a .y4m input is decoded: on the host (numpy, the whole file up front), or on the "
                        "device, from the file's YUV bytes as each window needs them (the same depth; needs a "
                        ".y4m input, a CUDA device and, without --downscale device, no --max_res downscale)")
    p.add_argument("--downscale", type=str, default="host", choices=["host", "device"],
                   help="where frames larger than --max_res are downscaled: on the host (Pillow's antialiased bicubic, "
                        "as the reference does), or with --decode device on the device from the file's YUV bytes "
                        "(vda_yuv_downscale: the same frames bit for bit, so the same depth)")
    return p


def check_args(a):
    assert a.inference_length > len(a.keyframe_list) + 2, "Inference length to small for the number of geiven keyframes"
    return a


def parse(argv=None):
    p = add_arguments(argparse.ArgumentParser(description="Video Depth Anything (MI355X)"))
    a = p.parse_args(argv)
    if a.vis == "device" and a.stitch != "device":
        p.error("--vis device needs --stitch device (it colours the depth where the device stitcher leaves it)")
    if a.downscale == "device" and a.decode != "device":
        p.error("--downscale device needs --decode device (it downscales the planar YUV frames that path uploads)")
    if a.decode == "device":
        if os.path.splitext(a.input_video)[1].lower() != ".y4m":
            p.error("--decode device needs a .y4m input (it uploads the file's planar YUV frames); convert the video "
                    "(ffmpeg -i in.mp4 -f yuv4mpegpipe out.y4m) or pass --decode host")
        if torch.device(a.device).type != "cuda":
            p.error("--decode device needs a CUDA device")
    return check_args(a)


def open_input(args):
    """The input frames and their rate: decoded on the host (``--decode host``), or with ``--decode device`` the
    indexed .y4m file (``video_io.Y4MFrames``).  A ``--max_res`` that would downscale it is refused unless
    ``--downscale device`` asks for that step on the device: then the object carries the downscaled size."""
    from vda_amd import video_io as VIO
    if args.decode != "device":
        return VIO.read_video_frames(args.input_video, args.max_len, args.target_fps, args.max_res)
    if args.downscale == "device":
        return VIO.open_y4m(args.input_video, args.max_len, args.target_fps, args.max_res)
    frames, fps = VIO.open_y4m(args.input_video, args.max_len, args.target_fps)
    if args.max_res > 0 and max(frames.h, frames.w) > args.max_res:
        sys.exit(f"{args.input_video}: --decode device does not downscale ({frames.w}x{frames.h} exceeds --max_res "
                 f"{args.max_res}; the host path does that step with Pillow's antialiased bicubic): pass --max_res -1 "
                 "or --decode host, or --downscale device for the same step on the device")
    return frames, fps


def load_model(args):
    """The model of ``--encoder`` on ``--device``: the checkpoint, or the synthetic recipe weights."""
    import vda_amd
    if not torch.cuda.is_available():
        raise RuntimeError("the MI355X path needs a GPU (there is no CPU mode)")
    if args.synthetic_weights:
        return vda_amd.build_model(args.encoder, device=args.device)
    ck = args.checkpoint or os.path.join("checkpoints", f"video_depth_anything_{args.encoder}.pth")
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    return vda_amd.build_model(args.encoder, state_dict=sd, device=args.device)


def main(argv=None):
    args = parse(argv)
    from vda_amd import video_io as VIO
    if args.decode == "device":  # index the file first: a refused input should not cost a model load
        frames, target_fps = open_input(args)
    model = load_model(args)
    dev = args.device
    if args.save_stats:
        torch.cuda.reset_peak_memory_stats(dev)
    if args.decode != "device":
        frames, target_fps = open_input(args)
    total = len(frames)
    t0 = time.time()
    if args.process_single_image:  # checked before --original, as in the reference (run.py:93-100)
        if args.decode == "device":  # the streaming driver takes RGB frames: decoded on the host
            frames = frames.rgb()
        depths, fps = model.infere_single_image(frames, target_fps, device=dev, fp32=args.fp32, input_size=args.input_size,
                                                inference_length=args.inference_length, keyframe_list=args.keyframe_list,
                                                align_each_new_frame=args.align_each_new_frame, warmup=True,
                                                skip_tmp_block=args.skip_tmp_block, stitch=args.stitch)
    else:
        depths, fps = model.infer_video_depth(frames, target_fps, input_size=args.input_size, device=dev, fp32=args.fp32,
                                              skip_tmp_block=args.skip_tmp_block and not args.original,
                                              windows_per_batch=max(1, args.windows_per_batch), stitch=args.stitch,
                                              **({"return_device": True} if args.vis == "device" else {}))
    dur = time.time() - t0
    os.makedirs(args.output_dir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(args.input_video))[0]
    name = ("Single_" if args.process_single_image else "") + f"VideoDepthAny_{args.encoder}_{stem}"
    if args.save_stats:
        lines = [f"Run: {args.encoder} {args.inference_length} {'Single Image' if args.process_single_image else ''} "
                 f"{'Align each frame' if args.align_each_new_frame else ''} keyframes {args.keyframe_list} "
                 f"{datetime.now():%Y-%m-%d %H:%M:%S}", "", "Times", "___________________________",
                 f"Runtime: {dur}", f"Processed Frames: {len(depths)}", f"Total Frames: {total}",
                 f"FPS (Processed): {len(depths) / dur}", f"Raw FPS: {total / dur}", "", "Memory",
                 "___________________________", f"GPU Memory (mb): {torch.cuda.max_memory_reserved(dev) / 2**20}", "", ""]
        with open(os.path.join(args.output_dir, "inference_log.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
    ext = "." + args.vis_format
    if args.save_orig:
        VIO.save_video(frames, os.path.join(args.output_dir, name + "_src" + ext), fps=fps)
    if args.save_vis:
        vis_in = depths
        if args.vis == "device" and not torch.is_tensor(depths):  # the streaming driver returns numpy
            vis_in = torch.from_numpy(np.ascontiguousarray(depths, dtype=np.float32)).to(dev)
        VIO.save_video(vis_in, os.path.join(args.output_dir, name + "_vis" + ext), fps=fps, is_depths=True,
                       grayscale=args.grayscale, spectral=not args.grayscale, chroma=args.vis_chroma)
        del vis_in
    if torch.is_tensor(depths):  # --vis device: the float depth leaves the device after the visualisation is written
        depths = depths.cpu().numpy()
    if args.save_npz:
        VIO.save_npz(os.path.join(args.output_dir, name + "_depths.npz"), depths)
    if args.save_tiff:
        VIO.save_tiff(os.path.join(args.output_dir, name + "_depths.tiff"), depths)
    print(f"{name}: {len(depths)} depth frames from {total} input frames in {dur:.2f} s")
    return depths


if __name__ == "__main__":
    main()
