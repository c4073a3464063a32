"""Time the visualisation kernels against vda_scale_shift on the same number of elements, and the whole
visualisation stage on the host against the device path.

    python tools/bench_vis.py [--frames 64] [--height 720] [--width 1280] [--reps 30] [--out FILE]

Kernels: depth [F, h, w] fp32 on the device, then depth_range, depth_colorize in its four layouts and unmasked
scale_shift over n = F*h*w (the yardstick: a streaming reduction that reads 8 B per element), interleaved,
each call between two device events; warm-up calls first; median [min .. max] of the repeats, and the achieved
GB/s from the bytes the algorithm needs (4 B read per element, + 1 / 3 / 3 / 1.5 B written).  The event
interval of depth_range and scale_shift includes their small second kernel.

End to end (``--e2e_frames``, 0 = skip): the same depth written as a Spectral .y4m by the host path (the copy
of the float depth to the host, ``colorize_depths``, ``write_y4m``) and by ``save_video`` on the device tensor,
both into ``--tmp`` on this machine; wall time per frame, best of ``--e2e_reps``.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e_frames", type=int, default=16, help="frames of the end-to-end comparison (0: skip it)")
    ap.add_argument("--e2e_reps", type=int, default=3)
    ap.add_argument("--tmp", type=str, default=None, help="directory for the end-to-end files (default: a temp dir)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args(argv)
    import torch
    from vda_amd import ops, video_io as VIO, visualize as VIS
    if not torch.cuda.is_available():
        raise RuntimeError("timing needs the GPU")
    F, H, W = a.frames, a.height, a.width
    n = F * H * W
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"visualisation kernels at F={F}, {H}x{W} (n = {n} elements)")
    g = torch.Generator(device="cuda").manual_seed(0)
    depth = torch.empty(F, H, W, device="cuda").uniform_(0.2, 7.5, generator=g)
    target = torch.empty(F, H, W, device="cuda").uniform_(0.2, 7.5, generator=g)
    rng = ops.depth_range(depth)
    rgb = torch.from_numpy(VIS.color_table(spectral=True)).cuda()
    yuv = torch.from_numpy(VIS.color_table(spectral=True, yuv=True)).cuda()
    cases = {
        "scale_shift (unmasked)": (8, lambda: ops.scale_shift(depth.view(-1), target.view(-1))),
        "depth_range": (4, lambda: ops.depth_range(depth)),
        "depth_colorize index": (5, lambda: ops.depth_colorize(depth, rng, layout="index")),
        "depth_colorize hwc": (7, lambda: ops.depth_colorize(depth, rng, lut=rgb, layout="hwc")),
        "depth_colorize planar444": (7, lambda: ops.depth_colorize(depth, rng, lut=yuv, layout="planar444")),
        "depth_colorize planar420": (5.5, lambda: ops.depth_colorize(depth, rng, lut=yuv, layout="planar420")),
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
    base = statistics.median(times["scale_shift (unmasked)"])
    for k, (bpe, _) in cases.items():
        t = times[k]
        med = statistics.median(t)
        say(f"  {k:26s} median {med:8.1f} [{min(t):8.1f} .. {max(t):8.1f}]   {bpe} B/element -> "
            f"{n * bpe / med / 1e3:7.1f} GB/s at the median, {med / base:5.2f} x scale_shift")

    if a.e2e_frames > 0:
        E = min(a.e2e_frames, F)
        d = depth[:E].contiguous()
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            hp, dp, d4 = (os.path.join(tmp, x) for x in ("host.y4m", "dev.y4m", "dev420.y4m"))

            def host():
                h = d.cpu().numpy()
                VIO.write_y4m(hp, VIO.colorize_depths(h, spectral=True), 24)

            def dev():
                VIO.save_video(d, dp, fps=24, is_depths=True, spectral=True)

            def dev420():
                VIO.save_video(d, d4, fps=24, is_depths=True, spectral=True, chroma="420")

            best = {}
            for name, fn in (("host: .cpu() + colorize_depths + write_y4m", host), ("device: save_video 4:4:4", dev),
                             ("device: save_video 4:2:0", dev420)):
                fn()  # warm-up (page cache, pinned buffers, matplotlib import)
                ts = []
                for _ in range(a.e2e_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                best[name] = min(ts)
            same = open(hp, "rb").read() == open(dp, "rb").read()
        say(f"end to end, {E} frames of {H}x{W} to a Spectral .y4m (numpy {np.__version__}, best of {a.e2e_reps}, "
            f"files identical: {same})")
        hb = best["host: .cpu() + colorize_depths + write_y4m"]
        for name, t in best.items():
            say(f"  {name:46s} {t / E * 1e3:8.2f} ms per frame ({E / t:7.1f} frames/s), {hb / t:5.1f} x the host path")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
