"""Time the point-cloud kernels against vda_depth_colorize over the same pixels, and the host path.

    python tools/bench_cloud.py [--frames 64] [--height 720] [--width 1280] [--reps 30] [--out FILE]

Kernels: depth [F, h, w] fp32, valid, rgb, K and M on the device, at keep ratios of about 0.7 (a random mask)
and 1.0 (no mask): cloud_count, cloud_write in both layouts, and depth_colorize (HWC) over the same pixels as the
bandwidth yardstick (4 B read, 3 B written per pixel), interleaved, each call between two device events; warm-up
calls first; median [min .. max] of the repeats and the achieved GB/s on the bytes the algorithm needs: count
reads 4 (+ 1 with a mask) B per candidate, write reads 4 (+ 1) B per candidate and 3 B per kept point and stores
15 B per kept point.  The event interval of cloud_count includes its two small scan kernels, that of the
cloud_write cases the allocation of the output by the caching allocator.

Host path (``--host_frames``, 0 = skip): the copy of depth to the host, the numpy restatement of the tests
(tests/cloud_ref.py: about a dozen full-size passes and a boolean gather) and ``tofile`` of the packed body,
wall time, against ``unproject_to_ply_bytes`` + ``write_ply`` on the device tensor, both into ``--tmp``.
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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_frames", type=int, default=8, help="frames of the host-path comparison (0: skip it)")
    ap.add_argument("--tmp", type=str, default=None, help="directory for the host-path files (default: a temp dir)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args(argv)
    import torch
    import cloud_ref
    from vda_amd import ops, pointcloud as PC, visualize as VIS
    if not torch.cuda.is_available():
        raise RuntimeError("timing needs the GPU")
    F, H, W = a.frames, a.height, a.width
    n = F * H * W
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"point-cloud kernels at F={F}, {H}x{W} (n = {n} candidates), with colour and a pose per frame")
    g = torch.Generator(device="cuda").manual_seed(0)
    depth = torch.empty(F, H, W, device="cuda").uniform_(0.5, 70., generator=g)
    rgb = torch.randint(0, 256, (F, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    mask = (torch.rand(F, H, W, device="cuda", generator=g) < 0.7).to(torch.uint8)
    K = torch.tensor([[1000., 1000., W / 2, H / 2]], device="cuda").repeat(F, 1).contiguous()
    M = torch.eye(4, device="cuda")[:3].repeat(F, 1, 1).contiguous()
    M[:, :, 3] = torch.arange(F, device="cuda", dtype=torch.float32)[:, None]
    trunc = PC.depth_trunc(80.)
    rng = ops.depth_range(depth)
    lut = torch.from_numpy(VIS.color_table(spectral=True)).cuda()

    cases = {"depth_colorize hwc": (7 * n, lambda: ops.depth_colorize(depth, rng, lut=lut, layout="hwc"))}
    for name, valid in (("keep 0.7", mask), ("keep 1.0", None)):
        offs, ws = ops.cloud_count(depth, valid, trunc=trunc)
        kept = int(offs[-1])
        per = 4 + (valid is not None)
        say(f"  {name}: {kept} of {n} candidates kept ({kept / n:.3f})")
        cases[f"cloud_count {name}"] = (per * n, lambda valid=valid: ops.cloud_count(depth, valid, trunc=trunc))
        for layout in ("split", "packed"):
            cases[f"cloud_write {layout} {name}"] = (
                per * n + (3 + 15) * kept,
                lambda valid=valid, ws=ws, kept=kept, layout=layout: ops.cloud_write(depth, valid, rgb, K, M, trunc=trunc, ws=ws,
                                                                                      n=kept, layout=layout))
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
    base = cases["depth_colorize hwc"][0] / statistics.median(times["depth_colorize hwc"])
    for k, (nbytes, _) in cases.items():
        t = times[k]
        med = statistics.median(t)
        say(f"  {k:30s} median {med:8.1f} [{min(t):8.1f} .. {max(t):8.1f}]   {nbytes / 1e6:7.1f} MB -> "
            f"{nbytes / med / 1e3:7.1f} GB/s at the median, {nbytes / med / base:5.2f} x depth_colorize's")

    if a.host_frames > 0:
        E = min(a.host_frames, F)
        d, v, c, k, m = depth[:E].contiguous(), mask[:E].contiguous(), rgb[:E].contiguous(), K[:E].contiguous(), M[:E].contiguous()
        intr = np.array([[1000., 0., W / 2], [0., 1000., H / 2], [0., 0., 1.]], np.float32)
        ext = np.tile(np.eye(4), (E, 1, 1))
        ext[:, :3, 3] = np.arange(E)[:, None]
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            hp, dp = os.path.join(tmp, "host.ply"), os.path.join(tmp, "dev.ply")

            def host():
                pts, col, _ = cloud_ref.cloud_f32(d.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy(),
                                                  m.cpu().numpy(), 1, trunc)
                with open(hp, "wb") as f:
                    f.write(PC.ply_header(len(pts), True))
                    cloud_ref.packed(pts, col).tofile(f)

            def dev():
                body = PC.unproject_to_ply_bytes(d, intr, ext, rgb=c, valid=v, max_depth=80., cam_to_world=True)
                PC.write_ply(dp, body, colors=True)

            best = {}
            for name, fn in (("host: .cpu() + numpy restatement + tofile", host), ("device: unproject_to_ply_bytes + write_ply", dev)):
                fn()  # warm-up
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                best[name] = min(ts)
            same = open(hp, "rb").read() == open(dp, "rb").read()
            size = os.path.getsize(dp)
        say(f"end to end, {E} frames of {H}x{W} to a coloured .ply of {size / 1e6:.0f} MB (numpy {np.__version__}, "
            f"{os.cpu_count()} CPUs, best of 3, files identical: {same})")
        hb = best["host: .cpu() + numpy restatement + tofile"]
        for name, t in best.items():
            say(f"  {name:46s} {t * 1e3:9.1f} ms, {hb / t:5.1f} x the host path")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
