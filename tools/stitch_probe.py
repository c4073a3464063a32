"""Host against device stitching on one GPU (tuning tool): ``stitch="host"`` and ``stitch="device"``
alternated in one process, synthetic ViT-L weights, on

  * the 176-frame 518x518 long-video job (8 windows),
  * a 66-frame 720x1280 job (3 windows at 518x924, 118 MB of fp32 per resized window),
  * 64 frames of 518x518 streaming with alignment (keyframes 2 12): wall time per frame.

Every leg is warmed up in both modes, then timed ``--rounds`` times per mode, host and device in
turn, with a host clock around work that ends in a device synchronise.  Reports every round, the
median and the min..max spread per mode, and the rel-L1 between the two modes' outputs at the timed
size.  Writes the report to ``--out`` (default profiles/stitch_device_ab.log) as well as stdout.

    python tools/stitch_probe.py [--rounds 4] [--encoder vitl] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--encoder", default="vitl")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "stitch_device_ab.log"))
    ap.add_argument("--legs", nargs="+", default=["video518", "video720", "stream"])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("stitch_probe measures on the GPU; there is nothing to time without one")
    import vda_amd
    dev = torch.device("cuda", 0)
    model = vda_amd.build_model(args.encoder, device=dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rel(a, b):
        return float(np.abs(a.astype(np.float64) - b).sum() / np.abs(b).sum())

    def leg(name, run, per):
        """run(mode) -> depth; per = frames the time is divided by."""
        out = {}
        for mode in ("host", "device"):  # warm-up: code objects, packed weights, pinned rings
            out[mode] = run(mode)
        torch.cuda.synchronize(dev)
        ts = {"host": [], "device": []}
        for _ in range(max(4, args.rounds)):
            for mode in ("host", "device"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(mode)
                torch.cuda.synchronize(dev)
                ts[mode].append((time.perf_counter() - t0) * 1e3)
        say(f"{name}: device vs host output rel-L1 {rel(out['device'], out['host']):.3e}")
        for mode in ("host", "device"):
            t = ts[mode]
            say(f"  {mode:6s} rounds {' '.join(f'{v:.1f}' for v in t)} ms | median {statistics.median(t):.1f} ms "
                f"(min {min(t):.1f}, max {max(t):.1f}) | {statistics.median(t) / per:.2f} ms/frame")
        mh, md = statistics.median(ts["host"]), statistics.median(ts["device"])
        say(f"  device/host median {md / mh:.3f}")

    say(f"stitch_probe: {args.encoder}, synthetic weights, {torch.cuda.get_device_name(dev)}, rounds {max(4, args.rounds)} per mode, "
        f"alternating host/device")
    g = np.random.default_rng(0)
    if "video518" in args.legs:
        fr = g.integers(0, 256, (176, 518, 518, 3), dtype=np.uint8)
        leg("long video 176 x 518x518", lambda mode: model.infer_video_depth(fr, 30, input_size=518, device=dev,
                                                                            stitch=mode)[0], 176)
    if "video720" in args.legs:
        fr = g.integers(0, 256, (66, 720, 1280, 3), dtype=np.uint8)
        leg("long video 66 x 720x1280", lambda mode: model.infer_video_depth(fr, 30, input_size=518, device=dev,
                                                                            stitch=mode)[0], 66)
    if "stream" in args.legs:
        fr = g.integers(0, 256, (64, 518, 518, 3), dtype=np.uint8)
        leg("streaming 64 x 518x518, align_each_new_frame, keyframes 2 12",
            lambda mode: model.infere_single_image(fr, 30, input_size=518, device=dev, keyframe_list=[2, 12],
                                                   align_each_new_frame=True, stitch=mode)[0], 64)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
