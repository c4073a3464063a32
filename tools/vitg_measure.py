"""ViT-g measurements on the device (measuring tool, not product code; see profiles/vitg_*.log).

usage: python tools/vitg_measure.py gemm [--rounds R]     w12 SwiGLU + LN fold against GEGLU + LN fold, same shape
       python tools/vitg_measure.py attn [--rounds R]     temporal attention D = 192, staged against direct-load
       python tools/vitg_measure.py model [--cache F]     1 x 32 x 518^2 frames/s, fp16 against fp32 on 4 frames
       python tools/vitg_measure.py forward N [--cache F] N forwards and nothing else (under rocprofv3 --kernel-trace)

Every comparison alternates its two sides round by round in one process on one device; a round is `reps` launches
between two device events after a warm-up round; the median over rounds and the spread (min .. max) are printed.
`--cache F`: keep the synthetic state dict in file F (built on first use: 1.37 G parameters take a minute).
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import vda_amd  # noqa: E402
from vda_amd import _lib, ops, weights  # noqa: E402
from vda_amd.model import _geglu_interleave  # noqa: E402

DEV = "cuda"


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per launch


def alternate(sides, rounds, reps):
    """{name: fn} -> {name: [us per round]}, the sides taking turns within every round."""
    for fn in sides.values():
        timed(fn, reps)  # warm-up
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(timed(fn, reps))
    return out


def show(name, us, work, unit):
    med = statistics.median(us)
    print(f"{name:28s} median {med:9.1f} us  (min {min(us):.1f} .. max {max(us):.1f} over {len(us)} rounds)  "
          f"{work / med / 1e6:7.2f} {unit}")
    return med


def gemm():
    rounds = int(opt("--rounds", 9))
    M, N, K = 43840, 8192, 1536
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(M, K, generator=g) * (1 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).half().to(DEV)
    w = _geglu_interleave((torch.randn(N, K, generator=g) * K ** -0.5)).half().to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    cs = w.float().sum(1).contiguous()
    st = ops.row_stats(x, 1e-6)
    out = torch.empty(M, N // 2, dtype=torch.float16, device=DEV)
    kw = dict(bias=bias, ln_stats=st, ln_parts=0, ln_eps=1e-6, ln_colsum=cs, out=out)
    sides = {"GEGLU + LN fold": lambda: ops.gemm(x, w, act=ops.ACT_GEGLU, **kw),
             "SwiGLU + LN fold": lambda: ops.gemm(x, w, act=ops.ACT_SWIGLU, **kw)}
    print(f"w12 GEMM M={M} N={N} K={K} (output [M, {N // 2}]), fp16, [M, 2] LN statistics, {torch.cuda.get_device_name()}")
    r = alternate(sides, rounds, 10)
    flop = 2.0 * M * N * K
    a = show("GEGLU + LN fold", r["GEGLU + LN fold"], flop, "TFLOP/s")
    b = show("SwiGLU + LN fold", r["SwiGLU + LN fold"], flop, "TFLOP/s")
    print(f"SwiGLU / GEGLU = {b / a:.4f}; per-round ratios "
          + " ".join(f"{s / t:.4f}" for s, t in zip(r["SwiGLU + LN fold"], r["GEGLU + LN fold"])))


def attn():
    import ctypes
    rounds = int(opt("--rounds", 9))
    B, T, S, H, D = 1, 32, 1369, 8, 192
    C = H * D
    tune = ctypes.CDLL(_lib.TUNE_LIB_PATH)
    _lib._declare(tune)
    qkv = (torch.randn(B * T * S, 3 * C, device=DEV) * 2).half()
    out = torch.empty(B * T * S, C, dtype=torch.float16, device=DEV)
    scale = float(torch.ones(()) / torch.sqrt(torch.tensor(float(D))))

    def run(knob):
        def fn():
            tune.vda_debug_attn(knob)
            rc = tune.vda_temporal_attention(qkv.data_ptr(), out.data_ptr(), B, T, S, H, D, scale, 0.0,
                                             torch.cuda.current_stream().cuda_stream)
            tune.vda_debug_attn(0)
            assert rc == 0
        return fn
    print(f"temporal attention B*T={B * T} S={S} H={H} D={D}, fp16, {torch.cuda.get_device_name()}")
    run(0)()
    a = out.clone()
    run(1)()
    print("staged and direct-load outputs bit-identical:", bool(torch.equal(a, out)))
    r = alternate({"staged (LDS, D = 192)": run(0), "direct-load": run(1)}, rounds, 20)
    nbytes = 4.0 * T * C * 2 * S * B  # q, k, v read and the output written, per site
    a = show("staged (LDS, D = 192)", r["staged (LDS, D = 192)"], nbytes, "TB/s")
    b = show("direct-load", r["direct-load"], nbytes, "TB/s")
    print(f"staged / direct = {a / b:.4f}")


def build():
    cache = opt("--cache")
    t0 = time.time()
    if cache and os.path.exists(cache):
        sd = torch.load(cache)
    else:
        meta = vda_amd.VideoDepthAnything.from_config("vitg", device="meta")
        sd = weights.synthetic_state_dict((k, tuple(v.shape)) for k, v in meta.state_dict().items())
        if cache:
            torch.save(sd, cache)
    m = vda_amd.build_model("vitg", sd, device=DEV)
    print(f"ViT-g: {sum(p.numel() for p in m.parameters()) / 1e9:.3f} G parameters, weights + build {time.time() - t0:.0f} s",
          flush=True)
    return m


def clip(T, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, T, 3, 518, 518, generator=g).to(DEV)


def model():
    m = build()
    x = clip(32)
    for _ in range(2):
        d = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d).all())
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(3):
            m(x)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / 3)
    med = statistics.median(times)
    print(f"ViT-g 1x32x518x518 fp16, one clip in flight, {torch.cuda.get_device_name()}: {med * 1e3:.1f} ms per forward "
          f"(min {min(times) * 1e3:.1f} .. max {max(times) * 1e3:.1f} over 5 rounds of 3) = {32 / med:.1f} frames/s")
    x4 = clip(4, seed=2)
    d16, d32 = m(x4).double(), m(x4, fp32=True).double()
    err = float((d16 - d32).abs().sum() / d32.abs().sum())
    print(f"full depth (40 blocks), 1x4x518x518: fp16 against fp32=True rel-L1 {err:.3e} (bar 1e-3); "
          f"depth mean {float(d32.mean()):.3f} min {float(d32.min()):.3f}")
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def forward():
    n = int(sys.argv[2])
    m = build()
    x = clip(32)
    for _ in range(n):
        m(x)
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"gemm": gemm, "attn": attn, "model": model, "forward": forward}[sys.argv[1]]()
