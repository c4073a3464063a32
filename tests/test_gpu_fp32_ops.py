"""Per-kernel parity of the fp32 mode (csrc/vda_f32.hip) at the shapes where its kernels can go wrong.

The fp32 mode is parity tier (i) of SURVEY.md §8(d) and the yardstick the fp16 path is judged against at
config 5's frame size, so each *_f32 kernel is held here in isolation: ragged and multiple
tiles, strided rows, every epilogue term, the grid-stride loops past the 65,536-block launch cap, NaN
neighbours (a frame / batch / site that must not leak into another) and run-to-run determinism.

Reference: the same operation in float64 torch on the CPU, on the same fp32 inputs.  Metric: rel-L1.  Bar:
TOL_OP = 2e-6 (exact-f32 products, fp32 accumulation in another order).  The stress inputs (attention
ramps and spike, RoPE, large common offsets in the norms) are limited by their conditioning, not by the
kernel: there the bar is max(TOL_OP, 2 * err0), err0 the rel-L1 of torch's own fp32 CPU op on the same
inputs (the factor 2 as in test_gemm_layernorm_fold: another summation order, nothing more).
"""
import pytest
import torch
import torch.nn.functional as F

from vda_amd import ops
from vda_amd._lib import ACT_GELU, ACT_GEGLU, ACT_RELU
from vda_amd.model import _geglu_interleave
from helpers import rel_l1

pytestmark = pytest.mark.gpu
TOL_OP = 2e-6
DEV = "cuda"


def c(t):
    return t.to(DEV, torch.float32).contiguous()


def rnd(*s, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*s, generator=g, dtype=torch.float64).float() * scale


def rel(a, b):
    return rel_l1(a.cpu(), b.cpu())


def stress_bar(name, y, y0, ref):
    """err < max(TOL_OP, 2 * err0): y the kernel's result, y0 torch's fp32 CPU op, ref float64."""
    err, err0 = rel(y, ref), rel(y0, ref)
    print(f"{name}: rel-L1 {err:.2e} (torch fp32 CPU {err0:.2e})")
    assert err < max(TOL_OP, 2 * err0)


# ---- GEMM (gemm_f32_kernel, dense) ------------------------------------------------------------------
def test_gemm_f32_refuses_drop_period():
    """drop_period is vda_gemm's (vda.h): the fp32 kernel stores all M rows, so the op refuses it before
    the launch instead of writing M rows into the [M - ceil(M / P), N] output."""
    x, w = c(rnd(600, 64, seed=1)), c(rnd(64, 64, seed=2))
    with pytest.raises(RuntimeError, match="drop_period"):
        ops.gemm(x, w, drop_period=300)


def test_gemm_f32_strided_rows():
    M, N, K = 200, 128, 64
    big, w = rnd(M, 3 * K, seed=3), rnd(N, K, scale=K ** -0.5, seed=4)
    y = ops.gemm(c(big)[:, K:2 * K], c(w))  # ldx = 3K
    assert rel(y, big[:, K:2 * K].double() @ w.double().t()) < TOL_OP


SENTINEL = -7777.0


def _framed(M, N):
    """An [M, N] view of an [M + 8, N + 8] sentinel buffer (row stride N + 8) and the buffer."""
    buf = torch.full((M + 8, N + 8), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[:M, :N]


def _frame_untouched(buf, M, N):
    return bool((buf[M:] == SENTINEL).all()) and bool((buf[:, N:] == SENTINEL).all())


def test_gemm_f32_strided_out_and_residuals():
    """out=, res and res2 as column slices of wider buffers (row strides that are multiples of 4, not N),
    res aliasing out, and no store past M or N: the sentinel frame around the output view stays."""
    M, N, K = 130, 132, 40
    x, w, b = rnd(M, K, seed=5), rnd(N, K, scale=K ** -0.5, seed=6), rnd(N, scale=0.1, seed=7)
    gam = rnd(N, seed=8).abs() + 0.1
    rw, r2w = rnd(M, N + 12, seed=9), rnd(M, N + 20, seed=10)
    res, res2 = rw[:, 4:4 + N], r2w[:, 8:8 + N]
    lin = x.double() @ w.double().t() + b.double()
    ref = gam.double() * lin + res.double() + res2.double()
    buf, out = _framed(M, N)
    ret = ops.gemm(c(x), c(w), bias=c(b), gamma=c(gam), res=c(rw)[:, 4:4 + N], res2=c(r2w)[:, 8:8 + N], out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert rel(out, ref) < TOL_OP
    assert _frame_untouched(buf, M, N)
    # in place: res is out (block.py:84-87, the residual stream)
    buf, out = _framed(M, N)
    out.copy_(res)
    ops.gemm(c(x), c(w), bias=c(b), gamma=c(gam), res=out, res2=c(r2w)[:, 8:8 + N], out=out)
    assert rel(out, ref) < TOL_OP
    assert _frame_untouched(buf, M, N)


@pytest.mark.parametrize("K", [16, 32, 48])
def test_gemm_f32_k_steps(K):
    """nk = 1, 2, 3 K steps of the double-buffered loop; two ragged M tiles and two ragged N tiles."""
    M, N = 130, 132
    x, w, b = rnd(M, K, seed=11), rnd(N, K, scale=K ** -0.5, seed=12), rnd(N, scale=0.1, seed=13)
    assert rel(ops.gemm(c(x), c(w), bias=c(b)), x.double() @ w.double().t() + b.double()) < TOL_OP


@pytest.mark.parametrize("I", [48, 80, 96])
def test_gemm_f32_geglu_tails(I):
    """GEGLU with N = 2 I = 96, 160, 192: the last 128-tile ends inside a wave's 64 rows (the nh >= N skip at
    32-row granularity); gamma and a residual of the output's width I."""
    M, K = 150, 24
    x, w, b = rnd(M, K, seed=14), rnd(2 * I, K, scale=K ** -0.5, seed=15), rnd(2 * I, scale=0.1, seed=16)
    gam, res = rnd(I, seed=17).abs() + 0.1, rnd(M, I, seed=18)
    hg = x.double() @ w.double().t() + b.double()
    ref = gam.double() * (hg[:, :I] * F.gelu(hg[:, I:])) + res.double()
    buf, out = _framed(M, I)
    ops.gemm(c(x), c(_geglu_interleave(w)), bias=c(_geglu_interleave(b)), gamma=c(gam), res=c(res), act=ACT_GEGLU,
             out=out)
    assert rel(out, ref) < TOL_OP
    assert _frame_untouched(buf, M, I)


def test_gemm_f32_epilogue_order():
    """gamma * gelu(x W^T + bias + rowbias) + res + res2, every term at once."""
    M, N, K, T, S = 257, 136, 40, 7, 11
    x, w, b = rnd(M, K, seed=19), rnd(N, K, scale=K ** -0.5, seed=20), rnd(N, scale=0.1, seed=21)
    rb, gam = rnd(T, N, seed=22), rnd(N, seed=23).abs() + 0.1
    res, res2 = rnd(M, N, seed=24), rnd(M, N, seed=25)
    pre = x.double() @ w.double().t() + b.double() + rb.double()[(torch.arange(M) // S) % T]
    ref = gam.double() * F.gelu(pre) + res.double() + res2.double()
    y = ops.gemm(c(x), c(w), bias=c(b), rowbias=c(rb), rdiv=S, rmod=T, gamma=c(gam), res=c(res), res2=c(res2),
                 act=ACT_GELU)
    assert rel(y, ref) < TOL_OP


@pytest.mark.parametrize("k,Cout", [(2, 24), (4, 24), (2, 40), (4, 40)])
def test_gemm_f32_pixel_shuffle(k, Cout):
    """ConvTranspose2d(kernel = stride = k) through the pixel-shuffle store: M = 189 (a ragged second M tile)."""
    BT, hh, ww, Cin = 3, 9, 7, 16
    xi = rnd(BT, Cin, hh, ww, seed=26)
    wt, bt = rnd(Cin, Cout, k, k, scale=0.2, seed=27), rnd(Cout, seed=28)
    ref = F.conv_transpose2d(xi.double(), wt.double(), bt.double(), stride=k).permute(0, 2, 3, 1)
    wp = wt.permute(2, 3, 1, 0).reshape(k * k * Cout, Cin)
    y = ops.conv_transpose_ks(c(xi.permute(0, 2, 3, 1).reshape(-1, Cin)), c(wp), c(bt.repeat(k * k)), BT, hh, ww, k)
    assert y.shape == ref.shape
    assert rel(y, ref) < TOL_OP


# ---- conv (gemm_f32_kernel<CONV>) -------------------------------------------------------------------
def nhwc(t):
    return c(t.permute(0, 2, 3, 1))


CONV_CASES = {
    # name: (BT, Cin, H, W, Cout, ks, stride, pad, bias, nres)
    "two_n_tiles": (2, 32, 9, 11, 256, 3, 1, 1, True, 0),
    "layer4_rn": (2, 1024, 5, 5, 256, 3, 1, 1, False, 0),
    "no_bias": (2, 32, 9, 11, 48, 3, 1, 1, False, 0),
    "res_res2": (2, 32, 9, 11, 48, 3, 1, 1, True, 2),
    "s2_20x23": (2, 32, 20, 23, 48, 3, 2, 1, True, 0),
    "s2_19x24": (2, 32, 19, 24, 48, 3, 2, 1, True, 0),
    "s2_2x2": (2, 32, 2, 2, 48, 3, 2, 1, True, 0),
    "s2_1x5": (2, 32, 1, 5, 48, 3, 2, 1, True, 0),
    "k1_p0": (2, 32, 9, 11, 48, 1, 1, 0, True, 0),
    "k3_p0": (2, 32, 9, 11, 48, 3, 1, 0, True, 0),
    "k5_p2": (2, 32, 9, 11, 48, 5, 1, 2, True, 0),
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_f32_geometries(name):
    BT, Cin, H, W, Cout, ks, stride, pad, bias, nres = CONV_CASES[name]
    x = rnd(BT, Cin, H, W, seed=30)
    w = rnd(Cout, Cin, ks, ks, scale=(ks * ks * Cin) ** -0.5, seed=31)
    b = rnd(Cout, scale=0.1, seed=32) if bias else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=pad)
    ref = ref.permute(0, 2, 3, 1)
    kw = {}
    if nres:  # the RCU's second conv: its own skip add and the fusion block's (blocks.py:78-91, :146-150)
        r1, r2 = rnd(*ref.shape, seed=33), rnd(*ref.shape, seed=34)
        kw = dict(res=c(r1), res2=c(r2))
        ref = ref + r1.double() + r2.double()
    y = ops.conv2d(nhwc(x), nhwc(w), ks=ks, stride=stride, pad=pad, bias=None if b is None else c(b), **kw)
    assert y.shape == ref.shape
    assert rel(y, ref) < TOL_OP


def test_conv_f32_frame_isolation():
    """13 x 11 = 143 rows per frame: the second 128-row M tile straddles the frame boundary.  Frame 1 all
    NaN must leave frame 0 finite and equal to the conv of frame 0 alone (no tap crosses a frame edge)."""
    Cin, Cout, H, W = 32, 48, 13, 11
    x = rnd(2, Cin, H, W, seed=35)
    x[1] = float("nan")
    w, b = rnd(Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5, seed=36), rnd(Cout, scale=0.1, seed=37)
    y = ops.conv2d(nhwc(x), nhwc(w), bias=c(b)).cpu()
    ref = F.conv2d(x[:1].double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert torch.isfinite(y[0]).all()
    assert rel(y[:1], ref) < TOL_OP
    assert torch.isnan(y[1]).all()


# ---- spatial attention (spatial_attn_f32_kernel) ----------------------------------------------------
def _spatial_ref(qkv, B, N, H, D, dtype=torch.float64):
    q, k, v = qkv.to(dtype).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    o = ((q * D ** -0.5) @ k.transpose(-1, -2)).softmax(-1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * N, H * D)


@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 128, 257])
def test_spatial_attention_f32_sizes(N):
    """One key, less than / exactly / just over one 64-key block, two full blocks, five with a ragged last."""
    B, H, D = 2, 3, 64
    qkv = rnd(B * N, 3 * H * D, seed=40 + N)
    assert rel(ops.spatial_attention(c(qkv), B, N, H, D), _spatial_ref(qkv, B, N, H, D)) < TOL_OP


def test_spatial_attention_f32_batch_isolation():
    """N = 70: the 58 padding keys of batch 0's last key block are batch 1's rows in memory.  Batch 1 all
    NaN must not reach batch 0."""
    B, N, H, D = 2, 70, 2, 64
    qkv = rnd(B * N, 3 * H * D, seed=50)
    qkv[N:] = float("nan")
    y = ops.spatial_attention(c(qkv), B, N, H, D).cpu()
    assert torch.isfinite(y[:N]).all()
    assert rel(y[:N], _spatial_ref(qkv[:N], 1, N, H, D)) < TOL_OP


@pytest.mark.parametrize("ramp", ["up", "spike", "down"])
def test_spatial_attention_f32_online_softmax(ramp):
    """The running-max correction of the online softmax, on the inputs of test_gpu_ops.py's
    test_spatial_attention_rebase without the fp16 rounding: scores that climb block after block ("up":
    every block re-bases), one huge score late in the sequence ("spike"), falling scores ("down")."""
    B, N, H, D = 2, 600, 2, 64
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, N, H, D, generator=g)
    k = torch.randn(B, N, H, D, generator=g)
    v = torch.randn(B, N, H, D, generator=g)
    pos = torch.arange(N, dtype=torch.float32)[None, :, None, None]
    q = q + 1.0
    if ramp == "up":
        k = k + pos / N * 3.5
    elif ramp == "spike":
        k[:, 500] = 4.0
    else:
        k = k + (N - pos) / N * 3.5
    qkv = torch.stack([q, k, v], 2).reshape(B * N, 3 * H * D)
    y = ops.spatial_attention(c(qkv), B, N, H, D)
    assert torch.isfinite(y).all()
    stress_bar(f"fp32 spatial attention {ramp}", y, _spatial_ref(qkv, B, N, H, D, torch.float32),
               _spatial_ref(qkv, B, N, H, D))


# ---- temporal attention (temporal_attn_f32_kernel) --------------------------------------------------
def _rotate(t, theta, dtype):
    """pe='rope' on t [..., T, C] (T the second-last axis): pairs (2i, 2i+1) of all C channels of frame t
    rotate by t * theta^(-2i/C), every step in `dtype`."""
    T, C = t.shape[-2], t.shape[-1]
    i = torch.arange(C // 2, dtype=dtype)
    freq = torch.tensor(theta, dtype=dtype) ** (-2 * i / C)
    ang = torch.arange(T, dtype=dtype)[:, None] * freq[None, :]  # [T, C/2]
    cs, sn = torch.cos(ang), torch.sin(ang)
    a, b = t.to(dtype)[..., 0::2], t.to(dtype)[..., 1::2]
    return torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(t.shape)


def _temporal_ref(qkv, B, T, S, H, D, theta=0.0, dtype=torch.float64):
    C = H * D
    t = qkv.to(dtype).view(B, T, S, 3, C).permute(3, 0, 2, 1, 4)  # [3, B, S, T, C]
    q, k, v = t[0], t[1], t[2]
    if theta > 0:
        q, k = _rotate(q, theta, dtype), _rotate(k, theta, dtype)
    sp = lambda z: z.reshape(B, S, T, H, D).permute(0, 1, 3, 2, 4)  # noqa: E731  [B, S, H, T, D]
    o = ((sp(q) @ sp(k).transpose(-1, -2)) * D ** -0.5).softmax(-1) @ sp(v)
    return o.permute(0, 3, 1, 2, 4).reshape(B * T * S, C)


@pytest.mark.parametrize("T,D,H", [(T, D, 8) for T in (1, 3, 32) for D in (2, 8, 24, 128)] + [(3, 24, 3)])
def test_temporal_attention_f32_shapes(T, D, H):
    B, S = 2, 5
    qkv = rnd(B * T * S, 3 * H * D, seed=60 + T + D)
    y = ops.temporal_attention(c(qkv), B, T, S, H, D)
    assert rel(y, _temporal_ref(qkv, B, T, S, H, D)) < TOL_OP


@pytest.mark.parametrize("T,S,H,D", [(32, 9, 8, 32), (7, 5, 8, 24), (32, 3, 8, 128)])
def test_temporal_attention_f32_rope(T, S, H, D):
    """rope_theta = 10000 against a float64 rotation; the kernel forms the angle in fp32, as torch fp32 does."""
    qkv = rnd(T * S, 3 * H * D, seed=70 + D)
    y = ops.temporal_attention(c(qkv), 1, T, S, H, D, rope_theta=10000.0)
    stress_bar(f"fp32 temporal attention rope T={T} S={S} D={D}", y,
               _temporal_ref(qkv, 1, T, S, H, D, 10000.0, torch.float32), _temporal_ref(qkv, 1, T, S, H, D, 10000.0))


def test_temporal_attention_f32_site_isolation():
    """One site's rows (all frames) NaN: every other site stays finite and correct."""
    B, T, S, H, D = 2, 5, 5, 8, 8
    qkv = rnd(B * T * S, 3 * H * D, seed=75)
    bad = torch.zeros(B, T, S, dtype=torch.bool)
    bad[1, :, 2] = True
    bad = bad.reshape(-1)
    qkv[bad] = float("nan")
    y = ops.temporal_attention(c(qkv), B, T, S, H, D).cpu()
    assert torch.isfinite(y[~bad]).all()
    ref = _temporal_ref(torch.nan_to_num(qkv), B, T, S, H, D)
    assert rel(y[~bad], ref[~bad]) < TOL_OP
    assert torch.isnan(y[bad]).all()


# ---- LayerNorm / GroupNorm --------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 72, 384, 1024, 2048])
@pytest.mark.parametrize("rows", [50, 3])
def test_layernorm_f32_shapes(C, rows):
    """C = 72 is no multiple of the wave width; rows = 50 and 3 leave waves of the last block without a
    row; x contiguous and as a column slice of a wider matrix (row stride C + 24)."""
    big = rnd(rows, C + 24, seed=80 + C) * 3 + 1
    g, b = rnd(C, seed=81), rnd(C, seed=82)
    x = big[:, 8:8 + C]
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)
    assert rel(ops.layernorm(c(x), c(g), c(b), 1e-6), ref) < TOL_OP
    assert rel(ops.layernorm(c(big)[:, 8:8 + C], c(g), c(b), 1e-6), ref) < TOL_OP


def test_layernorm_f32_skip_period_never_reads_cls():
    """skip_period drops each frame's cls row: with those rows NaN, no NaN reaches the output."""
    C, frames, npt = 384, 5, 9
    x = rnd(frames * (npt + 1), C, seed=83) * 2 - 0.5
    x.view(frames, npt + 1, C)[:, 0] = float("nan")
    g, b = rnd(C, seed=84), rnd(C, seed=85)
    y = ops.layernorm(c(x), c(g), c(b), 1e-6, skip_period=npt)
    assert y.shape == (frames * npt, C)
    assert torch.isfinite(y).all()
    ref = F.layer_norm(x.view(frames, npt + 1, C)[:, 1:].reshape(-1, C).double(), (C,), g.double(), b.double(), 1e-6)
    assert rel(y, ref) < TOL_OP


def test_layernorm_f32_large_offset():
    """+1000 on some rows: the two-pass variance must not cancel; bar from torch's fp32 LayerNorm."""
    C = 1024
    x = rnd(50, C, seed=86)
    x[::3] += 1000.0
    g, b = rnd(C, seed=87), rnd(C, seed=88)
    y = ops.layernorm(c(x), c(g), c(b), 1e-6)
    stress_bar("fp32 LayerNorm +1000", y, F.layer_norm(x, (C,), g, b, 1e-6),
               F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6))


def _gn_ref(x, g, b, F_, S, C):
    """GroupNorm(32, eps 1e-6) of NHWC frames in float64, written out (F.group_norm refuses a group of one
    value, which (F, S, C) = (1, 1, 32) has): biased variance over a frame's (S x C/32) slab."""
    v = x.double().view(F_, S, 32, C // 32)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    return ((v - mean) / torch.sqrt(var + 1e-6)).reshape(F_ * S, C) * g.double() + b.double()


def _gn_torch_f32(x, g, b, F_, S, C):
    """torch's own fp32 GroupNorm on the CPU."""
    r = F.group_norm(x.view(F_, S, C).permute(0, 2, 1), 32, g, b, 1e-6)
    return r.permute(0, 2, 1).reshape(F_ * S, C)


@pytest.mark.parametrize("F_,S,C", [(3, 37, 256), (2, 7, 64), (1, 1, 32), (2, 300, 1024)])
def test_groupnorm_f32_shapes(F_, S, C):
    x = rnd(F_ * S, C, seed=90 + S) * 2 + 0.5
    g, b = rnd(C, seed=91), rnd(C, seed=92)
    assert rel(ops.groupnorm(c(x), c(g), c(b), F_, 32, 1e-6), _gn_ref(x, g, b, F_, S, C)) < TOL_OP


def test_groupnorm_f32_frame_isolation():
    F_, S, C = 3, 37, 256
    x = rnd(F_ * S, C, seed=93)
    x[S:2 * S] = float("nan")
    g, b = rnd(C, seed=94), rnd(C, seed=95)
    y = ops.groupnorm(c(x), c(g), c(b), F_, 32, 1e-6).cpu()
    keep = torch.ones(F_ * S, dtype=torch.bool)
    keep[S:2 * S] = False
    assert torch.isfinite(y[keep]).all()
    ref = _gn_ref(torch.nan_to_num(x), g, b, F_, S, C)
    assert rel(y[keep], ref[keep]) < TOL_OP


def test_groupnorm_f32_large_offset():
    """+40 on one frame; bar from torch's fp32 GroupNorm."""
    F_, S, C = 3, 37, 256
    x = rnd(F_ * S, C, seed=96)
    x[S:2 * S] += 40.0
    g, b = rnd(C, seed=97), rnd(C, seed=98)
    y = ops.groupnorm(c(x), c(g), c(b), F_, 32, 1e-6)
    stress_bar("fp32 GroupNorm +40", y, _gn_torch_f32(x, g, b, F_, S, C), _gn_ref(x, g, b, F_, S, C))


@pytest.mark.parametrize("bias", [True, False])
def test_groupnorm_linear_f32_is_the_composition(bias):
    """fp32 groupnorm_linear is vda_groupnorm_f32 + vda_gemm_f32: the bits of the two ops, and parity."""
    F_, S, C, N = 3, 37, 256, 136
    x = rnd(F_ * S, C, seed=100)
    g, b = rnd(C, seed=101), rnd(C, seed=102)
    w, lb = rnd(N, C, scale=C ** -0.5, seed=103), (rnd(N, scale=0.1, seed=104) if bias else None)
    cb = None if lb is None else c(lb)
    y = ops.groupnorm_linear(c(x), c(g), c(b), F_, 32, 1e-6, c(w), bias=cb)
    assert torch.equal(y, ops.gemm(ops.groupnorm(c(x), c(g), c(b), F_, 32, 1e-6), c(w), bias=cb))
    ref = _gn_ref(x, g, b, F_, S, C) @ w.double().t() + (0 if lb is None else lb.double())
    assert rel(y, ref) < TOL_OP


def test_groupnorm_linear_f32_refuses_stats_out():
    F_, S, C = 2, 7, 64
    x, g, w = c(rnd(F_ * S, C, seed=105)), c(rnd(C, seed=106)), c(rnd(C, C, seed=107))
    st = torch.zeros(F_ * S, 1, 2, device=DEV, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="stats_out"):
        ops.groupnorm_linear(x, g, g, F_, 32, 1e-6, w, stats_out=st)


# ---- resize, im2col, depth tail ---------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 8, 128])
@pytest.mark.parametrize("src,dst", [((13, 12), (29, 31)), ((12, 12), (12, 12)), ((20, 24), (7, 9)), ((9, 9), (1, 1)),
                                     ((9, 9), (1, 17)), ((1, 7), (3, 9))])
def test_upsample_bilinear_f32_sizes(C, src, dst):
    """Upscale, identity, downscale, one output row / pixel (the Ho > 1 / Wo > 1 branches), one input row."""
    x = rnd(2, C, *src, seed=110 + C)
    ref = F.interpolate(x.double(), size=dst, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    y = ops.upsample_bilinear(nhwc(x), *dst)
    assert y.shape == ref.shape
    assert rel(y, ref) < TOL_OP
    if src == dst:
        assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1))


def test_upsample_bilinear_f32_past_grid_cap():
    """16.9 M float4 items on a launch capped at 65,536 blocks of 256: every thread strides (the model's
    296^2 resize does); the float64 reference in channel chunks."""
    C, Ho, Wo = 256, 520, 512
    x = rnd(1, C, 9, 9, seed=115)
    y = ops.upsample_bilinear(nhwc(x), Ho, Wo).cpu()
    assert y.shape == (1, Ho, Wo, C)
    num = den = 0.0
    for c0 in range(0, C, 32):
        ref = F.interpolate(x[:, c0:c0 + 32].double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
        ref = ref.permute(0, 2, 3, 1)
        num += float((y[..., c0:c0 + 32].double() - ref).abs().sum())
        den += float(ref.abs().sum())
    assert num / den < TOL_OP


def _im2col_ref(img, Kp):
    BT, _, H, W = img.shape
    np_ = (H // 14) * (W // 14)
    ref = torch.zeros(BT, np_ + 1, Kp)
    ref[:, 1:, :588] = F.unfold(img, 14, stride=14).transpose(1, 2)
    return ref.view(BT * (np_ + 1), Kp)


@pytest.mark.parametrize("BT,H,W,Kp", [(2, 28, 42, 588), (1, 14, 70, 588), (1, 28, 42, 592), (24, 518, 518, 588)])
def test_patch_im2col_f32_exact(BT, H, W, Kp):
    """The fp32 patch matrix is the image's 14 x 14 patches bit for bit, with zero cls rows and zero K
    padding; BT = 24 at 518^2 is 19.3 M elements, past the launch's 65,536-block cap."""
    img = torch.randn(BT, 3, H, W, generator=torch.Generator().manual_seed(120))
    a = ops.patch_im2col(img.to(DEV), Kp, dtype=torch.float32)
    assert a.dtype == torch.float32
    assert torch.equal(a.cpu(), _im2col_ref(img, Kp))


def _depth_head_inputs(C, Hin, Win, BT):
    x = rnd(BT, C, Hin, Win, seed=45)
    w1 = rnd(32, C, 3, 3, scale=(9 * C) ** -0.5, seed=46)
    b1 = rnd(32, scale=0.1, seed=47)
    w2, b2 = rnd(1, 32, 1, 1, seed=48).abs() * 0.2, torch.tensor([0.05])
    return x, w1, b1, w2, b2


@pytest.mark.parametrize("C,Hin,Win,Ho,Wo,BT", [(32, 9, 9, 16, 16, 1), (64, 5, 40, 33, 47, 2), (128, 12, 12, 12, 12, 1),
                                                 (128, 20, 24, 37, 51, 3)])
def test_depth_head_f32(C, Hin, Win, Ho, Wo, BT):
    """vda_depth_head_f32 (resize -> 3x3 conv -> ReLU -> 1x1 -> ReLU) against the same chain in float64."""
    x, w1, b1, w2, b2 = _depth_head_inputs(C, Hin, Win, BT)
    up = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    ref = F.relu(F.conv2d(F.relu(F.conv2d(up, w1.double(), b1.double(), padding=1)), w2.double(), b2.double()))[:, 0]
    y = ops.depth_head_f32(nhwc(x), nhwc(w1), c(b1), c(w2.reshape(-1)), c(b2), Ho, Wo)
    assert y.shape == ref.shape and y.dtype == torch.float32
    assert rel(y, ref) < TOL_OP


# ---- determinism ------------------------------------------------------------------------------------
def _det_cases():
    x, w, b = c(rnd(257, 40, seed=130)), c(rnd(136, 40, seed=131)), c(rnd(136, seed=132))
    res = c(rnd(257, 136, seed=133))
    yield "gemm", lambda: ops.gemm(x, w, bias=b, res=res, act=ACT_GELU)
    xc, wc = nhwc(rnd(2, 32, 13, 11, seed=134)), nhwc(rnd(48, 32, 3, 3, scale=0.1, seed=135))
    yield "conv2d", lambda: ops.conv2d(xc, wc, act=ACT_RELU)
    qs = c(rnd(2 * 150, 3 * 2 * 64, seed=136))
    yield "spatial_attention", lambda: ops.spatial_attention(qs, 2, 150, 2, 64)
    qt = c(rnd(7 * 5, 3 * 8 * 24, seed=137))
    yield "temporal_attention", lambda: ops.temporal_attention(qt, 1, 7, 5, 8, 24, rope_theta=10000.0)
    xl, g = c(rnd(111, 256, seed=138)), c(rnd(256, seed=139))
    yield "layernorm", lambda: ops.layernorm(xl, g, g, 1e-6)
    yield "groupnorm", lambda: ops.groupnorm(xl, g, g, 3, 32, 1e-6)
    xu = nhwc(rnd(2, 8, 13, 12, seed=140))
    yield "upsample_bilinear", lambda: ops.upsample_bilinear(xu, 29, 31)
    img = c(rnd(2, 3, 28, 42, seed=141))
    yield "patch_im2col", lambda: ops.patch_im2col(img, 588, dtype=torch.float32)
    xd, w1, b1, w2, b2 = _depth_head_inputs(64, 5, 40, 2)
    xd, w1, b1, w2, b2 = nhwc(xd), nhwc(w1), c(b1), c(w2.reshape(-1)), c(b2)
    yield "depth_head_f32", lambda: ops.depth_head_f32(xd, w1, b1, w2, b2, 33, 47)


def test_f32_kernels_are_deterministic():
    """No kernel of the fp32 mode uses atomics: the same input gives the same bits on every run."""
    for name, run in _det_cases():
        assert torch.equal(run(), run()), name
