"""Time the .y4m input path: the preprocessing kernels from planar YUV against the RGB kernel, and a whole video
job with the file decoded on the host against the file decoded on the device.

    python tools/bench_decode.py [--frames 32] [--height 720] [--width 1280] [--rounds 20] [--out FILE]

Kernels: ``--frames`` frames of 4:2:0 at ``--height`` x ``--width`` to the network size of ``--input_size``, three
candidates in one process after warm-up, taken in turn every round, each call between two device events:
  (a) preprocess_yuv              the product's route for the shape (the tile kernel at the product ratio)
  (b) yuv_to_rgb + preprocess_frames   the composition, made here of the two operators (the library picks its
                                  route from the geometry alone, it has no knob)
  (c) preprocess_frames           alone, on frames that are RGB already: what the host-decode path runs
Medians over all rounds, and per candidate the medians of the first and of the second half of its rounds: their
difference is the spread a difference between candidates has to beat.  The outputs are compared for equality.

End to end (``--e2e_frames``, 0 = skip): a synthetic 4:2:0 .y4m of that many frames through the calls run.py makes,
``read_video_frames`` + ``infer_video_depth`` (``--decode host``) against ``open_y4m`` + ``infer_video_depth``
(``--decode device``), ``--encoder`` with synthetic weights; wall time from before the file is opened to the depth on
the host, in turn, ``--e2e_reps`` times after one warm-up each; the host decode alone is timed too.  The file was
written just before, so it is read from the page cache.

``--max_res M`` below the frame's longer side times the ``--max_res`` downscale instead: vda_yuv_downscale (planar
YUV -> the downscaled RGB frames) with the bytes it must move and that figure over its time, ``yuv_to_rgb`` on the
same frames for scale, and end to end ``read_video_frames(max_res=M)`` (numpy decode + Pillow resize on the host)
against ``open_y4m(max_res=M)`` (``run.py --decode device --downscale device``).
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


def write_synthetic_y4m(path, n, h, w, fps=30):
    """Random 4:2:0 planes: the content does not matter to the timing, only the bytes per frame."""
    g = np.random.default_rng(0)
    fsz = h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{fps}:1 Ip A1:1 C420jpeg\n".encode())
        for _ in range(n):
            f.write(b"FRAME\n")
            f.write(g.integers(16, 236, fsz, dtype=np.uint8).tobytes())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--input_size", type=int, default=518)
    ap.add_argument("--max_res", type=int, default=-1,
                    help="downscale frames whose longer side exceeds this, as run.py does: times vda_yuv_downscale and "
                         "the job with the downscale on the host against --downscale device")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e_frames", type=int, default=176, help="frames of the end-to-end video (0: skip it)")
    ap.add_argument("--e2e_reps", type=int, default=3)
    ap.add_argument("--encoder", type=str, default="vitl", choices=["vits", "vitl"])
    ap.add_argument("--tmp", type=str, default=None, help="directory for the end-to-end file (default: a temp dir)")
    ap.add_argument("--out", type=str, default=None, help="also append the report to this file")
    a = ap.parse_args(argv)
    import torch
    import vda_amd
    from vda_amd import _lib, decode as D, ops, video as V, video_io as VIO
    if not torch.cuda.is_available():
        raise RuntimeError("timing needs the GPU")
    N, h, w = a.frames, a.height, a.width
    H, W = V.net_input_size(h, w, a.input_size)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.max_res > 0 and max(h, w) > a.max_res:
        return bench_downscale(a, say, lines)
    fsz = D.payload_bytes(h, w, "420")
    ws = _lib.lib().vda_preprocess_yuv_workspace(N, h, w, H, W)
    say(f"preprocessing {N} frames of {h}x{w} 4:2:0 -> {H}x{W} ({torch.cuda.get_device_name(0)}); preprocess_yuv takes "
        f"the {'composition (workspace ' + str(ws) + ' B)' if ws else 'tile'} route for this shape")
    pay = torch.randint(0, 256, (N, (fsz + 15) // 16 * 16), dtype=torch.uint8, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(0))
    rgb = ops.yuv_to_rgb(pay, h, w, "420")
    cases = {
        "(a) preprocess_yuv": lambda: ops.preprocess_yuv(pay, h, w, "420", H, W),
        "(b) yuv_to_rgb + preprocess_frames": lambda: ops.preprocess_frames(ops.yuv_to_rgb(pay, h, w, "420"), H, W),
        "(c) preprocess_frames on RGB": lambda: ops.preprocess_frames(rgb, H, W),
    }
    outs = [fn() for fn in cases.values()]
    say(f"  outputs equal bit for bit: {all(torch.equal(outs[0], o) for o in outs[1:])}")
    del outs
    for _ in range(a.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.rounds):  # in turn, so that drift hits every candidate alike
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    say(f"  {a.rounds} rounds after {a.warmup} warm-up rounds, device events, us")
    med, spread = {}, {}
    for k, t in times.items():
        half = len(t) // 2
        m0, m1 = statistics.median(t[:half]), statistics.median(t[half:])
        med[k], spread[k] = statistics.median(t), abs(m0 - m1)
        say(f"  {k:36s} median {med[k]:8.1f} [{min(t):8.1f} .. {max(t):8.1f}]   first half {m0:8.1f}, second half "
            f"{m1:8.1f}, spread {spread[k]:6.1f}")
    ka, kb, kc = list(cases)
    gain, bar = med[kb] - med[ka], max(spread[ka], spread[kb])
    say(f"  (a) against (b): {gain:+.1f} us ({med[kb] / med[ka]:.2f} x), the larger spread of the two is {bar:.1f} us; "
        f"(a) against (c): {med[ka] - med[kc]:+.1f} us for decoding {N} frames inside the kernel")

    if a.e2e_frames > 0:
        E = a.e2e_frames
        model = vda_amd.build_model(a.encoder, device="cuda")
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            p = os.path.join(tmp, "clip.y4m")
            write_synthetic_y4m(p, E, h, w)

            def host():
                frames, fps = VIO.read_video_frames(p, -1, -1, -1)
                return model.infer_video_depth(frames, fps, input_size=a.input_size, device="cuda")[0]

            def device():
                frames, fps = VIO.open_y4m(p, -1, -1)
                return model.infer_video_depth(frames, fps, input_size=a.input_size, device="cuda")[0]

            def decode_only():
                return VIO.read_video_frames(p, -1, -1, -1)[0]

            legs = {"--decode host: read_video_frames + infer_video_depth": host,
                    "--decode device: open_y4m + infer_video_depth": device,
                    "host decode alone (read_video_frames)": decode_only}
            ref = host()  # warm-up: page cache, pinned buffers, packed weights
            same = np.array_equal(ref, device())
            del ref
            wall = {k: [] for k in legs}
            for _ in range(a.e2e_reps):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall[k].append(time.perf_counter() - t0)
        say(f"end to end, {E} frames of {h}x{w} 4:2:0 from a .y4m, {a.encoder} with synthetic weights, file open to depth "
            f"on the host (numpy {np.__version__}; {a.e2e_reps} runs each in turn after a warm-up; depth equal: {same})")
        hb = statistics.median(wall["--decode host: read_video_frames + infer_video_depth"])
        for k, t in wall.items():
            m = statistics.median(t)
            say(f"  {k:58s} median {m:7.3f} s [{min(t):7.3f} .. {max(t):7.3f}]  {m / E * 1e3:7.2f} ms per frame, "
                f"{E / m:7.1f} frames/s, {hb / m:5.2f} x")
    write_report(a, lines)


def write_report(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def bench_downscale(a, say, lines):
    """``--max_res`` below the frame's longer side: the downscale kernel against the bytes it must move, and the
    whole job with the downscale on the host (``read_video_frames``) against the device (``open_y4m(max_res=)``)."""
    import torch
    import vda_amd
    from vda_amd import decode as D, ops, video as V, video_io as VIO
    N, h, w = a.frames, a.height, a.width
    s = a.max_res / max(h, w)
    h2, w2 = VIO.ensure_even(round(h * s)), VIO.ensure_even(round(w * s))
    H, W = V.net_input_size(h2, w2, a.input_size)
    fsz = D.payload_bytes(h, w, "420")
    say(f"downscaling {N} frames of {h}x{w} 4:2:0 -> {h2}x{w2} RGB (--max_res {a.max_res}; "
        f"{torch.cuda.get_device_name(0)}); {D.resample_taps(w, w2)} x {D.resample_taps(h, h2)} taps, served by the "
        f"kernel: {ops.yuv_downscale_accepts(h, w, h2, w2)}")
    pay = torch.randint(0, 256, (N, (fsz + 15) // 16 * 16), dtype=torch.uint8, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(0))
    small = ops.yuv_downscale(pay, h, w, "420", h2, w2)
    ref = torch.from_numpy(VIO._resize_rgb(ops.yuv_to_rgb(pay[:1], h, w, "420").cpu().numpy(), h2, w2))
    say(f"  frame 0 equals Pillow's resize of the decoded frame bit for bit: {torch.equal(small[:1].cpu(), ref)}")
    cases = {
        "(a) yuv_downscale": (lambda: ops.yuv_downscale(pay, h, w, "420", h2, w2), N * (fsz + 3 * h2 * w2)),
        "(b) yuv_to_rgb (full size, for scale)": (lambda: ops.yuv_to_rgb(pay, h, w, "420"), N * (fsz + 3 * h * w)),
        "(c) preprocess_frames on the small RGB": (lambda: ops.preprocess_frames(small, H, W), N * (3 * h2 * w2 + 12 * H * W)),
    }
    for _ in range(a.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, (fn, _b) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    say(f"  {a.rounds} rounds after {a.warmup} warm-up rounds, device events, us; bytes = what the op must read and write")
    for k, t in times.items():
        half = len(t) // 2
        m, m0, m1 = statistics.median(t), statistics.median(t[:half]), statistics.median(t[half:])
        nbytes = cases[k][1]
        say(f"  {k:40s} median {m:8.1f} [{min(t):8.1f} .. {max(t):8.1f}]   first half {m0:8.1f}, second half {m1:8.1f}; "
            f"{nbytes / 1e6:8.1f} MB, {nbytes / m / 1e6:6.2f} TB/s")
    del small, pay
    if a.e2e_frames > 0:
        E = a.e2e_frames
        model = vda_amd.build_model(a.encoder, device="cuda")
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            p = os.path.join(tmp, "clip.y4m")
            write_synthetic_y4m(p, E, h, w)

            def host():
                frames, fps = VIO.read_video_frames(p, -1, -1, a.max_res)
                return model.infer_video_depth(frames, fps, input_size=a.input_size, device="cuda")[0]

            def device():
                frames, fps = VIO.open_y4m(p, -1, -1, a.max_res)
                return model.infer_video_depth(frames, fps, input_size=a.input_size, device="cuda")[0]

            def decode_only():
                return VIO.read_video_frames(p, -1, -1, a.max_res)[0]

            legs = {"--decode host: read_video_frames(max_res) + infer_video_depth": host,
                    "--decode device --downscale device: open_y4m(max_res) + infer_video_depth": device,
                    "host decode + Pillow resize alone (read_video_frames)": decode_only}
            ref = host()  # warm-up: page cache, pinned buffers, packed weights
            same = np.array_equal(ref, device())
            del ref
            wall = {k: [] for k in legs}
            for _ in range(a.e2e_reps):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall[k].append(time.perf_counter() - t0)
        say(f"end to end, {E} frames of {h}x{w} 4:2:0 from a .y4m at --max_res {a.max_res}, {a.encoder} with synthetic "
            f"weights, file open to depth on the host ({a.e2e_reps} runs each in turn after a warm-up; depth equal: {same})")
        hb = statistics.median(next(iter(wall.values())))
        for k, t in wall.items():
            m = statistics.median(t)
            say(f"  {k:74s} median {m:7.3f} s [{min(t):7.3f} .. {max(t):7.3f}]  {m / E * 1e3:7.2f} ms per frame, "
                f"{E / m:7.1f} frames/s, {hb / m:5.2f} x")
    write_report(a, lines)


if __name__ == "__main__":
    main()
