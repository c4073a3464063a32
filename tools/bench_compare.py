"""Time the comparison-video kernels against vda_depth_colorize over the same number of output pixels, and the
whole panel stage on the host against the device path.

    python tools/bench_compare.py [--frames 32] [--height 720] [--width 1280] [--methods 1] [--reps 30] [--out FILE]

Kernels: a scene of F frames of h x w with M methods on the device (gt, aligned predictions, RGB, a validity
mask), then depth_absdiff_range over one method (n = F*h*w) and panel_compose of all F frames in its three
layouts (a canvas of (1 + M) x 3 tiles: P = F * (1 + M) * 3 * h * w output pixels); the yardstick is
depth_colorize in the same layout over a depth tensor of P pixels, and depth_range over n elements for the
reduction.  Interleaved, each call between two device events; warm-up calls first; median [min .. max] of the
repeats, and the achieved GB/s from the bytes the algorithm needs: per pixel of a tile column 3 + 9 B (RGB over
masked error map), 4 + 4 B (GT over prediction) and 2 x 4 B (the two x-t slices) read, 3 B (1.5 B at 4:2:0)
written per pixel.  The event interval of the two reductions includes their small second kernel.

End to end (``--e2e_frames``, 0 = skip): the panel .y4m of the same scene by the plain numpy composition of the
tests (tests/compare_ref.py: ``canvas_rgb`` + ``write_y4m``, after the copy of the aligned depth to the host)
and by ``save_compare_video`` on the device tensors, both into ``--tmp`` on this machine; wall time per frame,
best of ``--e2e_reps``.
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--methods", type=int, default=1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e_frames", type=int, default=4, help="frames of the end-to-end comparison (0: skip it)")
    ap.add_argument("--e2e_reps", type=int, default=2)
    ap.add_argument("--tmp", type=str, default=None, help="directory for the end-to-end files (default: a temp dir)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args(argv)
    import torch
    from vda_amd import compare as CMP, ops, video_io as VIO, visualize as VIS
    if not torch.cuda.is_available():
        raise RuntimeError("timing needs the GPU")
    F, H, W, M = a.frames, a.height, a.width, a.methods
    n = F * H * W
    P = n * (1 + M) * 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"comparison-video kernels at F={F}, {H}x{W}, M={M} (n = {n} elements per video, canvas {(1 + M) * H}x{3 * W}, "
        f"P = {P} output pixels)")
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.empty(F, H, W, device="cuda").uniform_(1., 60., generator=g)
    preds = [(gt * torch.empty(F, H, W, device="cuda").uniform_(0.7, 1.4, generator=g)).contiguous() for _ in range(M)]
    rgb = torch.randint(0, 256, (F, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    valid = (torch.rand(F, H, W, device="cuda", generator=g) < 0.7).view(torch.uint8)
    dr = torch.stack([torch.stack([ops.depth_range(p) for p in preds])[:, 0].min(),
                      torch.stack([ops.depth_range(p) for p in preds])[:, 1].max()])
    er = ops.depth_absdiff_range(preds[0], gt, valid)
    methods = {f"m{i}": CMP.MethodResult(1., 0., 0., 0., np.zeros(F), 0, p) for i, p in enumerate(preds)}
    res = CMP.CompareResult(methods=methods, depth_range=dr, error_range=er, gt=gt, rgb=rgb, valid=valid,
                            stability_line=0.5, backend=CMP.LibCompare)
    tiles = CMP.panel_tiles(res)
    big = torch.empty(F, (1 + M) * H, 3 * W, device="cuda").uniform_(1., 60., generator=g)  # P pixels for the yardstick
    brng = ops.depth_range(big)
    lut = {yuv: (torch.from_numpy(VIS.named_color_table("Spectral", yuv)).cuda(),
                 torch.from_numpy(VIS.named_color_table("RdYlGn", yuv)).cuda()) for yuv in (False, True)}
    # bytes read per canvas pixel, averaged over the three tile columns of a canvas with M method rows
    read = ((3 + 9 * M) + (4 + 4 * M) + (4 + 4 * M)) / (3 * (1 + M))

    def compose(layout):
        l0, l1 = lut[layout != "hwc"]
        return lambda: ops.panel_compose(tiles, 1 + M, 3, F, 0, F, res.xstar, lut0=l0, lut1=l1, layout=layout)

    def colorize(layout):
        return lambda: ops.depth_colorize(big, brng, lut=lut[layout != "hwc"][0], layout=layout)

    # name -> (bytes per element, elements, call, the case it is set against)
    cases = {
        "depth_range (n)": (4, n, lambda: ops.depth_range(gt), "depth_range (n)"),
        "depth_absdiff_range masked (n)": (9, n, lambda: ops.depth_absdiff_range(preds[0], gt, valid), "depth_range (n)"),
        "depth_absdiff_range (n)": (8, n, lambda: ops.depth_absdiff_range(preds[0], gt), "depth_range (n)"),
    }
    for layout, wr in (("hwc", 3), ("planar444", 3), ("planar420", 1.5)):
        yard = f"depth_colorize {layout} (P)"
        cases[yard] = (4 + wr, P, colorize(layout), yard)
        cases[f"panel_compose {layout} (P)"] = (read + wr, P, compose(layout), yard)
    for _ in range(a.warmup):
        for _, _, fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.reps):  # interleaved, so that drift hits every case alike
        for k, (_, _, fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    say(f"{torch.cuda.get_device_name(0)}; {a.reps} repeats after {a.warmup} warm-up calls, device events, us")
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, (bpe, cnt, _, yard) in cases.items():
        t = times[k]
        say(f"  {k:32s} median {med[k]:8.1f} [{min(t):8.1f} .. {max(t):8.1f}]   {bpe:5.2f} B/element -> "
            f"{cnt * bpe / med[k] / 1e3:7.1f} GB/s at the median, {med[k] / med[yard]:5.2f} x {yard.split()[0]}")

    if a.e2e_frames > 0:
        import compare_ref as R
        E = min(a.e2e_frames, F)
        sub = CMP.CompareResult(
            methods={k: CMP.MethodResult(1., 0., 0., 0., np.zeros(E), 0, m.aligned[:E].contiguous()) for k, m in methods.items()},
            depth_range=dr, error_range=er, gt=gt[:E].contiguous(), rgb=rgb[:E].contiguous(), valid=valid[:E].contiguous(),
            stability_line=0.5, backend=CMP.LibCompare)
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            hp, dp, d4 = (os.path.join(tmp, x) for x in ("host.y4m", "dev.y4m", "dev420.y4m"))

            def host():
                h = [m.aligned.cpu().numpy() for m in sub.methods.values()]
                canvas = R.canvas_rgb(sub.gt.cpu().numpy(), h, sub.rgb.cpu().numpy(), sub.valid.cpu().numpy().astype(bool),
                                      dr.cpu().numpy(), er.cpu().numpy(), sub.xstar)
                VIO.write_y4m(hp, canvas, 24)

            def dev():
                CMP.save_compare_video(dp, sub, fps=24)

            def dev420():
                CMP.save_compare_video(d4, sub, fps=24, chroma="420")

            best = {}
            for name, fn in (("host: .cpu() + numpy composition + write_y4m", host), ("device: save_compare_video 4:4:4", dev),
                             ("device: save_compare_video 4:2:0", dev420)):
                fn()  # warm-up (page cache, pinned buffers, matplotlib import)
                ts = []
                for _ in range(a.e2e_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                best[name] = min(ts)
            same = open(hp, "rb").read() == open(dp, "rb").read()
        say(f"end to end, {E} frames of {H}x{W}, M={M}, to a panel .y4m (numpy {np.__version__}, best of {a.e2e_reps}, "
            f"files identical: {same})")
        hb = best["host: .cpu() + numpy composition + write_y4m"]
        for name, t in best.items():
            say(f"  {name:46s} {t / E * 1e3:8.2f} ms per frame ({E / t:7.1f} frames/s), {hb / t:5.1f} x the host path")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
