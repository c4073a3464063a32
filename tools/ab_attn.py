"""In-process A/B of the attention kernels across libvda builds (tuning tool, not product code).

usage: python tools/ab_attn.py [spatial|temporal|bits] LIB_A.so [LIB_B.so ...] [--rounds R] [--calls C]
Every case goes through the C ABI on the current torch stream; outputs are compared bit-for-bit against
the first library's; timing rounds alternate the libraries (median / min / max us per call over the rounds).
--calls C: calls per timed window (default: 10, temporal 20).  A 10-call window is a few ms, which times the clock
ramp as much as the kernel; with --calls every library also runs C untimed calls of the case first, so a few
hundred give windows of ~0.1 s at the clock the kernel holds under its own load.
  spatial   ViT-L clip shape (32 frames x 1370 tokens x 16 heads x 64), also against torch SDPA in fp32
            (first 2 frames), and the 518 x 924 shape (N = 2443)
  temporal  the four motion-module shapes (T = 32, H = 8, C in {1024, 256}), rope_theta 0 and 10000
  bits      no timing: the small shapes of tests/test_gpu_fp16_edges.py (spatial N x H and the three ramps,
            temporal (D, H) x T x S = 3, RoPE off and on) and the shapes above
"""
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch
import torch.nn.functional as F
from vda_amd import _lib

MODEL_TEMPORAL = [("mm0 37^2 C=1024", 37 * 37, 1024), ("mm1 19^2 C=1024", 19 * 19, 1024),
                  ("mm2 37^2 C=256", 37 * 37, 256), ("mm3 74^2 C=256", 74 * 74, 256)]
SMALL_TEMPORAL = [(32, 4), (64, 4), (128, 4), (8, 3), (24, 3), (48, 3), (120, 3), (64, 3), (32, 3)]  # (D, H)

args = sys.argv[1:]
mode = args.pop(0) if args and args[0] in ("spatial", "temporal", "bits") else "spatial"
rounds = 7
calls = 0
libs = []
i = 0
while i < len(args):
    if args[i] == "--rounds":
        rounds = int(args[i + 1]); i += 2
    elif args[i] == "--calls":
        calls = int(args[i + 1]); i += 2
    else:
        libs.append(args[i]); i += 1
L = []
for p in libs:
    l = ctypes.CDLL(os.path.abspath(p))
    _lib._declare(l)
    L.append(l)
st = torch.cuda.current_stream().cuda_stream


def spatial(qkv, B, N, H):
    def call(l, y):
        assert l.vda_spatial_attention(qkv.data_ptr(), y.data_ptr(), B, N, H, 64, 64 ** -0.5, st) == 0, l.vda_last_error()
    return call, (B * N, H * 64)


def temporal(qkv, B, T, S, H, D, rope):
    def call(l, y):
        assert l.vda_temporal_attention(qkv.data_ptr(), y.data_ptr(), B, T, S, H, D, D ** -0.5, rope, st) == 0, l.vda_last_error()
    return call, (B * T * S, H * D)


def run(name, case, timed, n=10):
    """One case on every library: bit-for-bit against the first, then (timed) alternating rounds."""
    call, shape = case
    outs = []
    for l in L:
        y = torch.full(shape, float("nan"), device="cuda", dtype=torch.float16)
        call(l, y)
        torch.cuda.synchronize()
        outs.append(y)
    same = [bool(torch.equal(outs[0], o)) for o in outs[1:]]
    finite = bool(torch.isfinite(outs[0]).all())
    if timed:
        if calls:
            n = calls
            for li, l in enumerate(L):
                for _ in range(n):
                    call(l, outs[li])
            torch.cuda.synchronize()
        times = [[] for _ in L]
        for r in range(rounds):
            for li, l in enumerate(L):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    call(l, outs[li])
                e1.record()
                torch.cuda.synchronize()
                times[li].append(e0.elapsed_time(e1) / n * 1e3)
        for p, t in zip(libs, times):
            print(f"{name}: {p}: med {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}", flush=True)
    print(f"{name}: finite {finite}, bit-identical to the first: {same}", flush=True)
    return outs, all(same) and finite


ok = True
if mode in ("spatial", "bits"):
    B, N, H = 32, 1370, 16
    torch.manual_seed(0)
    qkv = (torch.randn(B * N, 3 * H * 64, device="cuda") * 1.5).half()
    outs, good = run(f"spatial ViT-L {B}x{N}x{H}x64", spatial(qkv, B, N, H), mode == "spatial")
    ok &= good
    q, k, v = qkv.view(B, N, 3, H, 64)[:2].float().permute(2, 0, 3, 1, 4)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(2 * N, H * 64)
    print("rel-L1 vs SDPA:", ["%.2e" % float((o[:2 * N].float() - ref).abs().sum() / ref.abs().sum()) for o in outs], flush=True)
if mode == "spatial":
    B, N, H = 32, 2443, 16
    torch.manual_seed(1)
    qkv = (torch.randn(B * N, 3 * H * 64, device="cuda") * 1.5).half()
    ok &= run(f"spatial 518x924 {B}x{N}x{H}x64", spatial(qkv, B, N, H), True)[1]
if mode in ("temporal", "bits"):
    for name, S, C in MODEL_TEMPORAL:
        for rope in (0.0, 10000.0):
            torch.manual_seed(S + C)
            qkv = torch.randn(32 * S, 3 * C, device="cuda", dtype=torch.float16)
            ok &= run(f"temporal {name} rope={rope:g}", temporal(qkv, 1, 32, S, 8, C // 8, rope), mode == "temporal", n=20)[1]
if mode == "bits":
    import fp16_bounds as fb
    for N in (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 161, 200, 257):
        for H in (1, 3):
            qkv = fb.rnd16(2 * N, 3 * H * 64, seed=N + H).to("cuda", torch.float16)
            ok &= run(f"spatial N={N} H={H}", spatial(qkv, 2, N, H), False)[1]
    for ramp in ("up", "spike", "down"):
        qkv = fb.attn_ramp_qkv(ramp, 2, 129, 2).to("cuda", torch.float16)
        ok &= run(f"spatial ramp {ramp}", spatial(qkv, 2, 129, 2), False)[1]
    for D, H in SMALL_TEMPORAL:
        for T in (1, 2, 31, 32):
            for rope in (0.0, 10000.0):
                qkv = (fb.rnd16(T * 3, 3 * H * D, seed=T + D) * 2).to("cuda", torch.float16)
                ok &= run(f"temporal D={D} H={H} T={T} S=3 rope={rope:g}", temporal(qkv, 1, T, 3, H, D, rope), False)[1]
print("ALL BIT-IDENTICAL AND FINITE" if ok else "DIFFERENCES (see above)", flush=True)
sys.exit(0 if ok else 1)
