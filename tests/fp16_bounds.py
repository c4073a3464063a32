"""Float64 references, derived per-element error bounds and CPU emulations for the fp16 kernels.

Shared by tests/test_fp16_bounds.py (CPU: every emulation lies inside its bound) and
tests/test_gpu_fp16_edges.py / tests/test_gpu_fp16_small_ops.py (GPU: every kernel output lies inside the same bound); DESIGN.md
"Per-element bounds of the fp16 kernels" has the derivation in prose.

Every `*_ref_bound` takes tensors whose VALUES are already fp16-representable (fp32 for bias / gamma /
rowbias), evaluates the operation in float64 as the same sequence of terms as the kernel, and returns
(ref, bound), both float64, with

    bound = u16 (|ref| + sum_i |v_i|) + gamma(K + c) A + f_act + 2^-24

u16 = 2^-11 (fp16 round to nearest), u32 = 2^-24, gamma(n) = n u32 / (1 - n u32) (the standard bound of an
n-term fp32 sum in ANY order), v_i the float64 value of every intermediate the kernel rounds to fp16
before the final store, A the absolute-value image of the accumulated expression, c the number of fp32
epilogue operations, f_act the activation's own error, 2^-24 the fp16 subnormal spacing.  No factor is
fitted to a kernel's output; each `emulate_*` is the kernel's arithmetic in torch on the CPU (fp32
accumulation in torch's order, .half() exactly at the kernel's rounding points).
"""
import math

import torch
import torch.nn.functional as F

U16 = 2.0 ** -11
U32 = 2.0 ** -24
SUB16 = 2.0 ** -24  # spacing of the fp16 subnormals: the absolute rounding error below 2^-14 is <= 2^-25
ACT_NONE, ACT_GELU, ACT_GEGLU, ACT_RELU = 0, 1, 2, 3


def gam(n):
    return n * U32 / (1.0 - n * U32)


def d(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_err(v, dv, phi_table=False):
    """Error of the kernel's GELU of v~ against gelu64(v) when |v~ - v| <= dv; |gelu'| <= 1.13 carries dv over.
    gelu_erf (vda_common.h; the tile kernels, the 512x128 phased kernel, the convs): erf_fast is Abramowitz &
    Stegun 7.1.26 (|error| <= 1.5e-7) plus two fp32 ulps (2^-23 each) for its v_rcp and v_exp, and enters as
    0.5 |v| erf; the three fp32 products / sums of 0.5 * v * (1 + erf) add 4 u32 |gelu|.
    phi_table (the phased 256x256 kernels, TAB in vda_gemm_phased.h): v * fma(v, B_i, A_i) with the line {A_i, B_i}
    of phi_table.h at the node nearest to v, max |A_i + B_i x - Phi(x)| = 1.27e-6 on [-8, 8] as the table's
    header documents (|v| <= 8 in every test): |v| * 1.27e-6, plus the fma's and the product's roundings,
    3 u32 |gelu| (Phi <= 1)."""
    if phi_table:
        return 1.13 * dv + v.abs() * (1.27e-6 + U32) + 3 * U32 * gelu64(v).abs()
    return 1.13 * dv + 0.5 * v.abs() * (1.5e-7 + 2 * 2.0 ** -23) + 4 * U32 * gelu64(v).abs()


_PHI_TAB = None


def phi_table():
    """The {A_i, B_i} lines of csrc/phi_table.h as a [2048, 2] fp32 tensor (for the CPU emulation)."""
    global _PHI_TAB
    if _PHI_TAB is None:
        import os
        import re
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-depth-anything_amd", "csrc",
                            "phi_table.h")
        vals = [float.fromhex(m) for m in re.findall(r"(-?0x[0-9a-f.]+p[+-]\d+)f", open(path).read())]
        assert len(vals) == 4096
        _PHI_TAB = torch.tensor(vals, dtype=torch.float64).float().view(2048, 2)
    return _PHI_TAB


def gelu_phi_table32(v):
    """The phased 256x256 kernels' GELU in fp32: node round(128 v) + 1024 clamped to 0 .. 2047 (phi_line)."""
    tab = phi_table()
    idx = (torch.round(v * 128.0) + 1024).clamp(0, 2047).long()
    ab = tab[idx]
    return v * (v * ab[..., 1] + ab[..., 0])


# ---- GEMM (vda_gemm_tile.h epi_store4 / epi_geglu4; the phased register epilogues are the same terms) ----
def gemm_ref_bound(x, w, *, bias=None, rowbias=None, rdiv=1, rmod=1, gamma=None, res=None, res2=None, act=ACT_NONE,
                   wg=None, bg=None, staged=False, ln=None, phi_table=False):
    """y = res + res2 + gamma * act(x w^T + bias + rowbias[(m / rdiv) % rmod]).  GEGLU: w / bias are the value
    half, wg / bg the gate half, v = (x w^T + bias) * gelu(x wg^T + bg).

    staged=False, the one-tile-per-block kernels (vda_gemm_tile.h epi_store4 / epi_geglu4): the accumulator and
    the whole epilogue including the residual adds are fp32 and the store is the ONLY fp16 rounding: no v_i.
    staged=True, the phased kernels (vda_gemm_phased.h: the LDS-staged epilogue's phase 1 / phase 2): t = gamma *
    act(...) is rounded to fp16, then res and res2 are added as packed fp16 vectors, one rounding per add, so t
    and (with both residuals) t + res are intermediates v_i.
    phi_table=True: GELU / GEGLU through the Phi table of the phased 256x256 kernels (gelu_err).

    ln: the LayerNorm fold, bounded for the folded form the kernel evaluates, rstd * (sum x w' - mean * colsum) +
    b' (one fma and one product after the K-term sum): A carries |rstd| (sum |x| |w'| + |mean| |colsum|).
    ln = dict(mean=, rstd=) ([M] fp32 VALUES, the ln_parts = 0 layout: the kernel reads them as they are, so the
    reference uses those very values and they add no error) or dict(parts= [M, P, 2] fp32 (sum, sum of squares),
    eps=): the kernel forms mean = sum / K, var = max(sumsq / K - mean^2, 0), rstd = rsqrt(var + eps) in fp32;
    their own error: dmean = gamma(P + 1) sum|part sums| / K, dvar = gamma(P + 3) (sumsq / K + mean^2) + 2 |mean|
    dmean, drstd / rstd = dvar / (2 (var + eps)) + 4 u32 (rsqrt and the add), which reach the output as
    |rstd colsum| dmean + (drstd / rstd) |rstd (acc - mean colsum)|.  colsum / colsum_g are [N] fp32 values."""
    x, w, bias, rowbias, gamma, res, res2, wg, bg = map(d, (x, w, bias, rowbias, gamma, res, res2, wg, bg))
    M, K = x.shape
    if ln is not None:
        if "parts" in ln:
            pt = d(ln["parts"])
            P = pt.shape[1]
            sm, sq = pt[..., 0].sum(1), pt[..., 1].sum(1)
            mean = sm / K
            var = (sq / K - mean * mean).clamp_min(0)
            rstd = (var + ln["eps"]) ** -0.5
            dmean = gam(P + 1) * pt[..., 0].abs().sum(1) / K
            dvar = gam(P + 3) * (sq / K + mean * mean) + 2 * mean.abs() * dmean
            drel = 0.5 * dvar / (var + ln["eps"]) + 4 * U32
        else:
            mean, rstd = d(ln["mean"]), d(ln["rstd"])
            dmean, drel = torch.zeros_like(mean), torch.zeros_like(mean)
        mean, rstd, dmean, drel = (t[:, None] for t in (mean, rstd, dmean, drel))

    def lin(wt, b, colsum=None):
        pre, A = x @ wt.t(), x.abs() @ wt.abs().t()
        c = 0
        dstat = 0.0
        if ln is not None:
            cs = d(colsum)[None, :]
            A = rstd * (A + (mean * cs).abs())
            pre = rstd * (pre - mean * cs)
            dstat = (rstd * cs.abs() * dmean + drel * pre.abs()) * (1 + drel)
            c = 2
        if b is not None:
            pre, A, c = pre + b, A + b.abs(), c + 1
        if rowbias is not None:
            rb = rowbias[(torch.arange(M) // rdiv) % rmod]
            pre, A, c = pre + rb, A + rb.abs(), c + 1
        return pre, gam(K + c) * A + dstat

    pre, dpre = lin(w, bias, None if ln is None else ln["colsum"])
    if act == ACT_GEGLU:
        g, dg = lin(wg, bg, None if ln is None else ln["colsum_g"])
        gg, dgg = gelu64(g), gelu_err(g, dg, phi_table)
        v = pre * gg
        dv = gg.abs() * dpre + pre.abs() * dgg + dpre * dgg + U32 * v.abs()
    elif act == ACT_GELU:
        v, dv = gelu64(pre), gelu_err(pre, dpre, phi_table)
    elif act == ACT_RELU:
        v, dv = pre.clamp_min(0), dpre
    else:
        v, dv = pre, dpre
    if gamma is not None:
        v, dv = gamma * v, gamma.abs() * dv + U32 * (gamma * v).abs()
    if staged:
        inter = 0.0
        for r in (res, res2):
            if r is not None:  # an fp16 add of two fp16 values: one rounding of the exact sum
                inter = inter + v.abs()
                v = v + r
        return v, U16 * (v.abs() + inter) + dv + SUB16
    for r in (res, res2):
        if r is not None:  # one fp32 add each: its rounding is relative to the running sum
            dv = dv * (1 + U32) + U32 * (v.abs() + r.abs())
            v = v + r
    return v, U16 * v.abs() + dv + SUB16


def emulate_gemm(x, w, *, bias=None, rowbias=None, rdiv=1, rmod=1, gamma=None, res=None, res2=None, act=ACT_NONE,
                 wg=None, bg=None, staged=False, ln=None, phi_table=False):
    gelu = gelu_phi_table32 if phi_table else F.gelu
    f = lambda t: None if t is None else t.detach().to("cpu", torch.float32)  # noqa: E731
    x, w, bias, rowbias, gamma, res, res2, wg, bg = map(f, (x, w, bias, rowbias, gamma, res, res2, wg, bg))

    if ln is not None:
        K = x.shape[1]
        if "parts" in ln:
            pt = f(ln["parts"])
            mean = pt[..., 0].sum(1) / K
            rstd = torch.rsqrt((pt[..., 1].sum(1) / K - mean * mean).clamp_min(0) + ln["eps"])
        else:
            mean, rstd = f(ln["mean"]), f(ln["rstd"])

    def lin(wt, b, colsum=None):
        v = x @ wt.t()
        if ln is not None:
            v = rstd[:, None] * (v - mean[:, None] * f(colsum)[None, :])
        if b is not None:
            v = v + b
        if rowbias is not None:
            v = v + rowbias[(torch.arange(x.shape[0]) // rdiv) % rmod]
        return v

    v = lin(w, bias, None if ln is None else ln["colsum"])
    if act == ACT_GEGLU:
        v = v * gelu(lin(wg, bg, None if ln is None else ln["colsum_g"]))
    elif act == ACT_GELU:
        v = gelu(v)
    elif act == ACT_RELU:
        v = F.relu(v)
    if gamma is not None:
        v = v * gamma
    if staged:
        v = v.half().float()
        if res is not None and res2 is not None:
            v = (v + res).half().float()
            res = None
    if res is not None:
        v = v + res
    if res2 is not None:
        v = v + res2
    return v.half()


def row_stats_ref_bound(y16, part=256):
    """The stats_out partials of stored fp16 rows y16 [M, parts * 256]: (sum, sum of squares) per 256-column part
    in float64 [M, parts, 2] and their bound: a 256-term fp32 sum in any order (per lane, across lanes, across
    the four waves of a block) with the squares' own roundings, gamma(256 + 8) of the absolute sums.
    part: the width of a part where the row is narrower than 256 columns (N = 128: one part of 128 terms,
    gamma(128 + 8))."""
    y = d(y16).reshape(y16.shape[0], -1, part)
    ref = torch.stack([y.sum(-1), (y * y).sum(-1)], -1)
    A = torch.stack([y.abs().sum(-1), (y * y).sum(-1)], -1)
    return ref, gam(part + 8) * A + 2.0 ** -100


def emulate_row_stats(y16):
    y = y16.detach().to("cpu", torch.float32).reshape(y16.shape[0], -1, 256)
    return torch.stack([y.sum(-1), (y * y).sum(-1)], -1)


# ---- 3x3 / 1x1 convolutions (NCHW here; the tests permute to the kernels' NHWC) ----
def bilinear64(x, Ho, Wo):
    """align_corners=True bilinear resize of NCHW float64."""
    return F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)


def conv_ref_bound(x, w, *, bias=None, stride=1, pad=1, pre_relu=False, relu_out=False, res=None, res2=None,
                   staged=False, up=None, res2_up=False, framebias=None):
    """y = [relu](conv(pre_relu ? relu(x) : x) + bias) + res + res2, x [BT, Cin, H, W], w [Cout, Cin, ks, ks].

    staged=False (implicit-GEMM tile kernels, the register-staged conv, the 128-channel halo conv): fp32 up
    to the store, one rounding.  staged=True (vda_hconv.hip, vda_strip.hip and its split finish kernel): the
    kernel rounds v0 = [relu](conv + bias) to fp16, then adds res and res2 as fp16 vectors, one rounding per
    add, so v0 and (with both residuals) v0 + res are the intermediates v_i.  res2_up (hconv only): res2 is a
    smaller map read through the bilinear upsample: bilerp8 rounds the interpolated value to fp16 (a further
    v_i); its fp32 blend and its fp32 weights fma(scale, o, -i0) (error <= 2 u32 * source coordinate) are
    bounded with 4 max|res2| for the four corners.  up=(Hu, Wu): x is read through the bilinear resize,
    rounded to fp16 (the register-staged loader and the fused halo conv both build an fp16 patch).
    framebias [rmod, Cout]: the epilogue's rowbias with rdiv = Ho * Wo, i.e. frame bt adds row bt % rmod."""
    x, w, bias, res, res2, framebias = map(d, (x, w, bias, res, res2, framebias))
    extra = 0.0
    if up is not None:
        # the resized operand is an fp16 rounding of a float64-exact blend: |dx| <= u16 |x_up| + its fp32 terms
        xu = bilinear64(x, *up)
        n_src = max(x.shape[2], x.shape[3])
        dx = U16 * xu.abs() + (8 + 4 * n_src) * U32 * 4 * float(x.abs().max()) + SUB16
        extra = F.conv2d(dx, w.abs(), None, stride, pad)
        x = xu
    xin = x.clamp_min(0) if pre_relu else x
    K = w.shape[1] * w.shape[2] * w.shape[3]
    v = F.conv2d(xin, w, None, stride, pad)
    A = F.conv2d(xin.abs(), w.abs(), None, stride, pad)
    c = 0
    if bias is not None:
        v, A, c = v + bias.view(1, -1, 1, 1), A + bias.abs().view(1, -1, 1, 1), 1
    if framebias is not None:
        fbv = framebias[torch.arange(v.shape[0]) % framebias.shape[0]][:, :, None, None]
        v, A, c = v + fbv, A + fbv.abs(), c + 1
    dv = gam(K + c) * A + extra
    if relu_out:
        v = v.clamp_min(0)
    if not staged:
        for r in (res, res2):
            if r is not None:
                dv = dv * (1 + U32) + U32 * (v.abs() + r.abs())
                v = v + r
        return v, U16 * v.abs() + dv + SUB16
    inter = 0.0  # sum of |v_i|
    ref = v
    if res is not None:
        inter = inter + ref.abs()
        ref = ref + res
    if res2 is not None:
        inter = inter + ref.abs()
        if res2_up:
            upv = bilinear64(res2, v.shape[2], v.shape[3])
            n_src = max(res2.shape[2], res2.shape[3])
            inter = inter + upv.abs()
            dv = dv + (8 + 4 * n_src) * U32 * 4 * float(res2.abs().max()) + SUB16
            ref = ref + upv
        else:
            ref = ref + res2
    return ref, U16 * (ref.abs() + inter) + dv + SUB16


def emulate_conv(x, w, *, bias=None, stride=1, pad=1, pre_relu=False, relu_out=False, res=None, res2=None,
                 staged=False, up=None, res2_up=False, framebias=None):
    f = lambda t: None if t is None else t.detach().to("cpu", torch.float32)  # noqa: E731
    x, w, bias, res, res2, framebias = map(f, (x, w, bias, res, res2, framebias))
    if up is not None:
        x = F.interpolate(x, size=up, mode="bilinear", align_corners=True).half().float()
    if pre_relu:
        x = F.relu(x)
    v = F.conv2d(x, w, bias, stride, pad)
    if framebias is not None:
        v = v + framebias[torch.arange(v.shape[0]) % framebias.shape[0]][:, :, None, None]
    if relu_out:
        v = F.relu(v)
    if not staged:
        if res is not None:
            v = v + res
        if res2 is not None:
            v = v + res2
        return v.half()
    o = v.half()
    if res is not None:
        o = (o.float() + res).half()  # an fp16 add is the correctly rounded sum of two fp16 values
    if res2 is not None:
        r2 = F.interpolate(res2, size=v.shape[2:], mode="bilinear", align_corners=True).half().float() if res2_up else res2
        o = (o.float() + r2).half()
    return o


# ---- attention ----
def _softmax_pv_bound(s, eps, v, nk, D):
    """Output bound of softmax(s) v when every score carries an absolute error <= eps (per query row).

    With s~_j = s_j + d_j, |d_j| <= eps, p~_j / p_j = e^{d_j} / sum_i p_i e^{d_i} lies in [e^{-2 eps}, e^{2 eps}]
    (the softmax's Lipschitz factor).  P is rounded to fp16 before the PV MFMA (numerator) and, in the round-1
    spatial kernel, also before the row sum (denominator): (1 + u16)^2.  exp2 is within one fp32 ulp (2 u32)
    in numerator and denominator, the row sum and the PV accumulation are nk-term fp32 sums, the rescales of O
    and the final O * (1 / l) a handful of fp32 operations: (1 + u32)^(2 nk + 16).  The product form keeps the
    second-order terms.  P is relative to a reference under which the largest P of the row is >= 1 when it is
    taken (so l >= 1): a P below 2^-14 is an fp16 subnormal with absolute error <= 2^-25, i.e. <= 2^-25 |v_j|
    per key in the normalised output.  Then the output's own fp16 rounding."""
    p = torch.softmax(s, -1)
    ref = p @ v
    Apv = p @ v.abs()
    factor = torch.exp(2 * eps) * (1 + U16) ** 2 * (1 + U32) ** (2 * nk + 16) - 1
    dO = factor * Apv + 2.0 ** -25 * v.abs().sum(-2, keepdim=True)
    return ref, U16 * ref.abs() + dO + SUB16


def spatial_q_scaled(q32):
    """The spatial kernels' B operand q' = fp16(q * scale * log2(e)), scale * log2(e) as the host forms it in
    fp32 (D = 64: 0.125f * 1.44269504f): one IEEE fp32 product and one round-to-nearest fp16 conversion, so
    torch on the CPU reproduces it bit for bit."""
    sl2 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (q32.to(torch.float32) * sl2).half()


def spatial_attn_ref_bound(qkv, B, N, H, D=64):
    """softmax(q k^T / sqrt(D)) v on qkv [B*N, 3*H*D] -> (ref, bound) [B*N, H*D].

    Both spatial kernels round q' = q * scale * log2(e) to fp16 before the QK MFMA.  That rounding is
    reproduced exactly (spatial_q_scaled) and the float64 reference is evaluated on q', the operand the kernel
    really multiplies: carried through the softmax as a worst-case u16 sum |q'| |k| term instead it would make
    the bound ~20x looser than the arithmetic (the test also keeps the rel-L1 bar against the reference on the
    unrounded q).  What remains on a score: a D-term fp32 accumulation that starts from C = -m (the running
    reference, |m| <= the largest |score| of the row) and a few fp32 re-base subtractions; in natural units
    eps = 2 gamma(D + 4) max_j ln2 sum_d |q'_d| |k_d|."""
    assert D == 64
    t = d(qkv).reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    q = spatial_q_scaled(q).to(torch.float64) * math.log(2.0)
    s = q @ k.transpose(-1, -2)
    As = q.abs() @ k.abs().transpose(-1, -2)
    eps = 2 * gam(D + 4) * As.max(-1, keepdim=True).values
    ref, bound = _softmax_pv_bound(s, eps, v, N, D)
    back = lambda z: z.transpose(1, 2).reshape(B * N, H * D)  # noqa: E731
    return back(ref), back(bound)


def emulate_spatial_attn(qkv, B, N, H, D=64, round1=False):
    """round1: the round-1 kernel's row sum rides on the PV MFMA, i.e. it sums the fp16-rounded P."""
    t = qkv.detach().to("cpu", torch.float32).reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    s = spatial_q_scaled(q).float() @ k.transpose(-1, -2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    ph = p.half().float()
    o = (ph @ v) / (ph if round1 else p).sum(-1, keepdim=True)
    return o.half().transpose(1, 2).reshape(B * N, H * D)


def _rope64(z, theta):
    """z [..., T, C] float64 -> (rotated, |a| + |b| per channel, angle per channel): pairs (2i, 2i + 1) of all C
    channels of frame t rotate by t * theta^(-2i / C)."""
    T, C = z.shape[-2], z.shape[-1]
    i = torch.arange(C // 2, dtype=torch.float64)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * theta ** (-2 * i / C)[None, :]  # [T, C/2]
    cs, sn = torch.cos(ang), torch.sin(ang)
    a, b = z[..., 0::2], z[..., 1::2]
    out = torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(z.shape)
    mag = (a.abs() + b.abs()).repeat_interleave(2, -1)
    return out, mag, ang.repeat_interleave(2, -1)


def temporal_attn_ref_bound(qkv, B, T, S, H, D, rope_theta=0.0):
    """Attention over the T frames of every (site, head) on qkv [(B*T)*S, 3*H*D] -> (ref, bound) [(B*T)*S, H*D].

    Both temporal kernels accumulate q.k in fp32 from zero, scale by scale * log2(e) in fp32 and subtract the
    row maximum: eps = 2 gamma(D + 5) max_j scale sum_d |q_d| |k_d|.  With RoPE, q and k are rotated in fp32 from
    the fp16 values and rounded BACK TO fp16: per channel |dq'| <= u16 |q'| + (|a| + |b|) (17 u32 angle + 4 u32) +
    2^-25, where 17 u32 angle covers the fp32 frequency 1 / powf(theta, 2i / C) (ln(theta) <= 9.3 times the
    exponent's rounding, the powf / division / product roundings: 17 u32 relative) and 4 u32 sincosf and the two
    products; those enter the score through scale (dq |k'| + |q'| dk + dq dk)."""
    C = H * D
    t = d(qkv).reshape(B, T, S, 3, C)
    q, k, v = t[..., 0, :].transpose(1, 2), t[..., 1, :].transpose(1, 2), t[..., 2, :].transpose(1, 2)  # [B, S, T, C]
    dq = dk = None
    if rope_theta > 0:
        q, mq, ang = _rope64(q, rope_theta)
        k, mk, _ = _rope64(k, rope_theta)
        dq = U16 * q.abs() + mq * (17 * U32 * ang + 4 * U32) + 2.0 ** -25
        dk = U16 * k.abs() + mk * (17 * U32 * ang + 4 * U32) + 2.0 ** -25
    sp = lambda z: z.reshape(B, S, T, H, D).permute(0, 1, 3, 2, 4)  # noqa: E731  [B, S, H, T, D]
    q, k, v = sp(q), sp(k), sp(v)
    scale = D ** -0.5
    s = scale * (q @ k.transpose(-1, -2))
    As = scale * (q.abs() @ k.abs().transpose(-1, -2))
    eps = 2 * gam(D + 5) * As.max(-1, keepdim=True).values
    if dq is not None:
        dq, dk = sp(dq), sp(dk)
        E = scale * (dq @ k.abs().transpose(-1, -2) + q.abs() @ dk.transpose(-1, -2) + dq @ dk.transpose(-1, -2))
        eps = eps + E.max(-1, keepdim=True).values
    ref, bound = _softmax_pv_bound(s, eps, v, T, D)
    back = lambda z: z.permute(0, 3, 1, 2, 4).reshape(B * T * S, C)  # noqa: E731
    return back(ref), back(bound)


def emulate_temporal_attn(qkv, B, T, S, H, D, rope_theta=0.0):
    C = H * D
    t = qkv.detach().to("cpu", torch.float32).reshape(B, T, S, 3, C)
    q, k, v = t[..., 0, :].transpose(1, 2), t[..., 1, :].transpose(1, 2), t[..., 2, :].transpose(1, 2)
    if rope_theta > 0:
        i = torch.arange(C // 2, dtype=torch.float32)
        freq = 1.0 / torch.pow(torch.tensor(rope_theta, dtype=torch.float32), (2 * i) / C)
        ang = torch.arange(T, dtype=torch.float32)[:, None] * freq[None, :]
        cs, sn = torch.cos(ang), torch.sin(ang)

        def rot(z):
            a, b = z[..., 0::2], z[..., 1::2]
            return torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(z.shape).half().float()
        q, k = rot(q), rot(k)
    sp = lambda z: z.reshape(B, S, T, H, D).permute(0, 1, 3, 2, 4)  # noqa: E731
    q, k, v = sp(q), sp(k), sp(v)
    sl2 = torch.tensor(D ** -0.5, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)) * sl2
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = (p.half().float() @ v) / p.sum(-1, keepdim=True)
    return o.half().permute(0, 3, 1, 2, 4).reshape(B * T * S, C)


# ---- case families (shared inputs of the CPU proof and the GPU tests; values fp16-representable) ----
def rnd16(*s, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*s, generator=g) * scale).half().float()


def rnd32(*s, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*s, generator=g) * scale


GEMM_EPIS = ("bias", "gelu", "gamma_res", "res_res2", "rowbias", "geglu", "ps2", "ps4", "strided_x")


def ps_geometry(M):
    """(BT, hin, win) with BT * hin * win == M and as many factors > 1 as M has among 2, 3, 5, 7."""
    dims = []
    for _ in range(2):
        f = next((f for f in (7, 5, 3, 2) if M % f == 0 and M > f), 1)
        dims.append(f)
        M //= f
    return M, dims[1], dims[0]


def gemm_case(M, N, K, epi, seed=0):
    """Inputs and the reference keywords of one dense-GEMM epilogue family.  N counts the GEMM's weight rows
    (GEGLU: 2 I interleaved rows, output I = N / 2 columns; pixel shuffle: N = k * k * cout)."""
    c = dict(M=M, N=N, K=K, epi=epi, x=rnd16(M, K, seed=seed + 1), kw={})
    wscale = K ** -0.5
    if epi == "geglu":
        I = N // 2
        c["w"], c["kw"] = rnd16(I, K, scale=wscale, seed=seed + 2), dict(
            act=ACT_GEGLU, wg=rnd16(I, K, scale=wscale, seed=seed + 3), bias=rnd32(I, scale=0.1, seed=seed + 4),
            bg=rnd32(I, scale=0.1, seed=seed + 5))
        return c
    c["w"] = rnd16(N, K, scale=wscale, seed=seed + 2)
    b = rnd32(N, scale=0.1, seed=seed + 4)
    if epi in ("bias", "strided_x", "ps2", "ps4"):
        c["kw"] = dict(bias=b)
    elif epi == "gelu":
        c["kw"] = dict(bias=b, act=ACT_GELU)
    elif epi == "gamma_res":
        c["kw"] = dict(bias=b, gamma=rnd32(N, seed=seed + 5).abs() + 0.1, res=rnd16(M, N, seed=seed + 6))
    elif epi == "res_res2":
        c["kw"] = dict(bias=b, res=rnd16(M, N, seed=seed + 6), res2=rnd16(M, N, seed=seed + 7))
    elif epi == "rowbias":  # frames of rdiv rows: with rdiv no divisor of the tile height a tile spans a frame change
        rdiv = max(1, min(M // 2, 50))
        rmod = 3
        c["kw"] = dict(rowbias=rnd32(rmod, N, seed=seed + 8), rdiv=rdiv, rmod=rmod)
    else:
        raise ValueError(epi)
    return c


def conv_case(BT, Cin, Cout, H, W, mode, *, ks=3, stride=1, seed=0, res2_src=None, up=None):
    """mode plain / rcu1 (pre-ReLU, bias, ReLU) / rcu2 (bias + res + res2); res2_src=(h, w): res2 is that smaller
    map; up=(Hu, Wu): x is read through the resize."""
    pad = ks // 2
    Hi, Wi = (H, W) if up is None else up
    Ho, Wo = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
    c = dict(x=rnd16(BT, Cin, H, W, seed=seed + 1), w=rnd16(Cout, Cin, ks, ks, scale=(ks * ks * Cin) ** -0.5, seed=seed + 2),
             kw=dict(stride=stride, pad=pad), Ho=Ho, Wo=Wo)
    if up is not None:
        c["kw"]["up"] = up
    if mode != "plain":
        c["kw"]["bias"] = rnd32(Cout, scale=0.1, seed=seed + 3)
    if mode == "rcu1":
        c["kw"].update(pre_relu=True, relu_out=True)
    elif mode == "rcu2":
        c["kw"]["res"] = rnd16(BT, Cout, Ho, Wo, seed=seed + 4)
        if res2_src is None:
            c["kw"]["res2"] = rnd16(BT, Cout, Ho, Wo, seed=seed + 5)
        else:
            c["kw"].update(res2=rnd16(BT, Cout, *res2_src, seed=seed + 5), res2_up=True)
    elif mode != "plain":
        raise ValueError(mode)
    return c


# ViT-B's 3x3 convs with 128 outputs (layer1..4_rn, the refinenets' RCU convs) on the phased 512x128 kernel:
# (BT, H, W) with M = 8,281 = 16 x 512 + 89 (a ragged last tile) and M = 8,192 (whole tiles, the frame change on a
# tile edge); Cin = 96 (K = 864: per-lane tap decode, a K tail of 32), 128 (wave-uniform taps), 8 (K = 72: two K
# tiles, both straddling taps).  Shared by tests/test_gpu_vitb.py and the negative control of tests/test_vitb.py.
VITB_CONV_SIZES = [(1, 91, 91), (2, 64, 64)]
VITB_CONV_CINS = [96, 128, 8]


def vitb_conv_case(BT, Cin, H, W, mode):
    return conv_case(BT, Cin, 128, H, W, mode, seed=Cin + H)


def attn_ramp_qkv(ramp, B, N, H, D=64, seed=7):
    """The three score profiles of test_spatial_attention_rebase, scaled to any N: keys whose scores climb
    through the sequence, one huge-score key late in it, and falling scores."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, N, H, D, generator=g) + 1.0
    k = torch.randn(B, N, H, D, generator=g)
    v = torch.randn(B, N, H, D, generator=g)
    pos = torch.arange(N, dtype=torch.float32)[None, :, None, None]
    if ramp == "up":
        k = k + pos / N * 3.5
    elif ramp == "spike":
        k[:, (N * 5) // 6] = 4.0
    else:
        k = k + (N - pos) / N * 3.5
    return torch.stack([q, k, v], 2).reshape(B * N, 3 * H * D).half().float()


LN_KINDS = ("ln", "ln_parts", "ln_gelu", "ln_geglu", "ln_rowbias", "ln_stats_out", "ln_drop")


def gemm_ln_case(M, N, K, kind, seed=0, eps=1e-6):
    """A LayerNorm-folded GEMM: x rows with their own offset and scale, w' = fp16(w diag(gamma)), b' = w beta + b,
    colsum = sum_k w' in fp32, the statistics in float64 rounded to fp32 ([M, 2] (mean, rstd), or for ln_parts
    three column parts of (sum, sum of squares))."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * (1 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).half().float()
    gam_, bet = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)

    def fold(n):
        w = torch.randn(n, K, generator=g) * K ** -0.5
        wf = (w * gam_[None, :]).half().float()
        return wf, (w @ bet + 0.1 * torch.randn(n, generator=g)), wf.double().sum(1).float()
    c = dict(M=M, N=N, K=K, epi=kind, x=x)
    x64 = x.double()
    if kind == "ln_parts":
        P = 3
        xp = x64.view(M, P, K // P)
        ln = dict(parts=torch.stack([xp.sum(-1), (xp * xp).sum(-1)], -1).float(), eps=eps)
    else:
        mean, var = x64.mean(1), x64.var(1, unbiased=False)
        ln = dict(mean=mean.float(), rstd=((var + eps) ** -0.5).float())
    if kind == "ln_geglu":
        c["w"], b, ln["colsum"] = fold(N // 2)
        wg, bg, ln["colsum_g"] = fold(N // 2)
        c["kw"] = dict(bias=b, act=ACT_GEGLU, wg=wg, bg=bg, ln=ln)
        return c
    c["w"], b, ln["colsum"] = fold(N)
    c["kw"] = dict(bias=b, ln=ln)
    if kind == "ln_gelu":
        c["kw"]["act"] = ACT_GELU
    elif kind == "ln_rowbias":  # the motion modules' per-frame PE row bias (EK 3): rdiv >= 256
        c["kw"].update(rowbias=torch.randn(3, N, generator=g), rdiv=300, rmod=3)
    return c


# =====================================================================================================
# LayerNorm, GroupNorm, GroupNorm -> Linear (csrc/vda_norm.hip)
# =====================================================================================================
def fma32(a, b, c):
    """fp32 fma(a, b, c) on fp32 tensors: the product is exact in float64 (24 + 24 bits), the sum rounds to
    float64 and then to fp32 (a double rounding differs from the fused one only on a 2^-29 tie window)."""
    return (a.double() * b.double() + c.double()).float()


def wave_tree(v):
    """wave_sum (vda_common.h:140): the xor butterfly 32, 16, .. 1 over the last dim (any power of two <= 64);
    every lane ends with the same bits, lane 0 is returned."""
    n = v.shape[-1]
    idx = torch.arange(n)
    o = n // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def _norm_out(x, mean, rstd, g, b, dmean, dvar, eps):
    """y = (x - mean) * rstd * g + b in float64 and its bound when the kernel's mean is within dmean and its
    variance within dvar: rstd~ / rstd - 1 is within drel = r / (2 (1 - r)) + 4 u32, r = dvar / (var + eps) (the
    add of eps, the division by n, v_rsq_f32 at 1 ulp); (x - mean~) sc~ = ((x - mean) + (mean - mean~)) sc
    (1 + drel); the kernels evaluate either ((x - mean) * rstd) * g + b or fma(x, sc, fma(-mean, sc, b)): at most
    four fp32 roundings, each relative to a partial result <= A = |sc| (|x| + |mean|) + |b|; one fp16 store."""
    var_eps = rstd ** -2
    r = (dvar / var_eps).clamp_max(0.5)
    drel = 0.5 * r / (1 - r) + 4 * U32
    sc = rstd * g
    v = (x - mean) * sc
    ref = v + b
    A = sc.abs() * (x.abs() + mean.abs()) + b.abs()
    bound = U16 * ref.abs() + sc.abs() * dmean * (1 + drel) + drel * v.abs() + 4 * U32 * A + SUB16
    return ref, bound, drel


def ln_depth(C):
    """Summation depth of the LayerNorm kernels' statistics: 8 values per 16-byte chunk, ceil(C / 512) chunks per
    lane in sequence (layernorm_kernel, vda_norm.hip:21-31; one in layernorm_narrow_kernel :136), then the
    6-level wave tree (:32, log2(LPR) levels in the narrow kernel :138)."""
    return 8 * ((C // 8 + 63) // 64) + 6


def _ln_stats(x, eps):
    C = x.shape[1]
    D = ln_depth(C)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    dmean = gam(D + 1) * x.abs().mean(1, keepdim=True)  # D adds and the division by C
    # sum (x - mean~)^2 = sum (x - mean)^2 + C (mean~ - mean)^2 exactly; each term rounds d and d * d, the sum D
    # times, the division once
    dvar = gam(D + 4) * (var + dmean ** 2) + dmean ** 2
    return mean, var, dmean, dvar


def layernorm_ref_bound(x, g, b, eps):
    """layernorm_kernel / layernorm_narrow_kernel<16|32|64> (vda_norm.hip:8-59, :122-155): two-pass fp32
    statistics from registers over the fp16 row, then fp16((v - mean) * rstd * g + b) (:53, :151), the ONLY fp16
    rounding.  x [R, C] (fp16 values), g / b [C] fp32.  Bound: half an fp16 ulp of the reference + the fp32
    terms of _norm_out + the statistics term of _ln_stats at the kernel's summation depth ln_depth(C)."""
    x, g, b = map(d, (x, g, b))
    mean, var, dmean, dvar = _ln_stats(x, eps)
    ref, bound, _ = _norm_out(x, mean, (var + eps) ** -0.5, g[None], b[None], dmean, dvar, eps)
    return ref, bound


def ln_stats_ref_bound(x, eps):
    """row_stats_kernel (vda_norm.hip:63-96): (mean, rstd) per row [R, 2] fp32 from the same two passes: mean
    within dmean + u32 |mean|, rstd within rstd * drel (_norm_out)."""
    x = d(x)
    mean, var, dmean, dvar = _ln_stats(x, eps)
    rstd = (var + eps) ** -0.5
    one = torch.ones_like(mean)
    _, _, drel = _norm_out(x[:, :1], mean, rstd, one, one, dmean, dvar, eps)
    ref = torch.cat([mean, rstd], 1)
    return ref, torch.cat([dmean + U32 * mean.abs() + 2.0 ** -140, rstd * drel], 1)


def emulate_layernorm(x, g, b, eps, stats_only=False, drop_lane=None):
    """The kernels' order: lane l sums chunks l, l + 64, .. (8 values each, in order), the wave tree, mean = s / C;
    q = fma(d, d, q) in the same order (hipcc contracts q += d * d), rstd = rsqrt(q / C + eps);
    y = fp16(fma((v - mean) * rstd, g, b)).  A narrow row (C / 8 lanes) is the same sums with the other lanes at
    zero.  drop_lane: a MUTANT that leaves one lane out of both reductions (test_fp16_bounds.py only)."""
    x, g, b = (t.detach().to("cpu", torch.float32) for t in (x, g, b))
    R, C = x.shape
    xp = F.pad(x, (0, 2048 - C)).view(R, 4, 64, 8)
    live = (torch.arange(2048) < C).view(4, 64, 8)
    if drop_lane is not None:
        live = live.clone()
        live[:, drop_lane] = False
    s = torch.zeros(R, 64)
    for i in range(4):
        for j in range(8):
            s = torch.where(live[i, :, j], s + xp[:, i, :, j], s)
    mean = wave_tree(s) / float(C)
    q = torch.zeros(R, 64)
    for i in range(4):
        for j in range(8):
            dd = xp[:, i, :, j] - mean[:, None]
            q = torch.where(live[i, :, j], fma32(dd, dd, q), q)
    rstd = torch.rsqrt(wave_tree(q) / float(C) + torch.tensor(eps, dtype=torch.float32))
    if stats_only:
        return torch.stack([mean, rstd], 1)
    return fma32((x - mean[:, None]) * rstd[:, None], g[None].expand_as(x), b[None].expand_as(x)).half()


LN_CS = [8, 64, 128, 256, 384, 512, 520, 1024, 2040, 2048]


def ln_rows(R, C, seed=0):
    """R random rows, then the stress rows: a +1000 offset, one 60000 outlier, a constant row, an all-zero row."""
    x = rnd16(R + 4, C, seed=seed + R + C) * 2 + 0.5
    x[R] += 1000.0
    x[R + 1, C // 3] = 60000.0
    x[R + 2] = 3.0
    x[R + 3] = 0.0
    return x.half().float()


def gn_rows(C):
    return 32 if C >= 512 else 128


def gn_layout(C):
    """(cpr, rpi, nr) of gn_partial / gn_apply (vda_norm.hip gn_layout, gn_stats_launch): 16-byte chunks per row,
    row-lanes of a 256-thread block, rows per thread."""
    cpr = C // 8
    rpi = 256 // cpr
    return cpr, rpi, (gn_rows(C) + rpi - 1) // rpi


def gn_depth(S, C, groups):
    """The deeper of the two routes' summation depths.  groupnorm_kernel<VW> (vda_norm.hip:181-196): ceil(S cg /
    (256 VW)) vectors of VW values per thread in sequence, the wave tree (6) and the four waves (3).  Workspace
    route: nr rows per thread, the rpi row-lanes folded in sequence (gn_partial_kernel), then ceil(nchunk cg / 64)
    pairs per lane in sequence and the wave tree, with the merge's own products (gn_finalize_kernel)."""
    cg = C // groups
    vw = 8 if cg % 8 == 0 else 4 if cg % 4 == 0 else 2
    two_pass = -(-(S * cg // vw) // 256) * vw + 9
    if C % 8 or C > 2048:
        return two_pass
    _, rpi, nr = gn_layout(C)
    nchunk = -(-S // gn_rows(C))
    return max(two_pass, nr + rpi + -(-nchunk * cg // 64) + 6 + 4)


def _gn_stats(x, groups, eps):
    """x [F, S, C] float64 -> per (frame, group) mean, var, dmean, dvar [F, 1, groups, 1].

    The statistics term is that of a two-pass fp32 variance, in a form that also covers the merge of chunk-local
    two-pass moments: with D = gn_depth and rms^2 = var + mean^2 (the data's spread about zero),
        dmean = gamma(D) rms                     (a D-deep fp32 sum of n values: gamma(D) mean|x| <= gamma(D) rms)
        dvar  = gamma(D) (var + dmean^2) + dmean^2 + 2 sqrt(var) dmean
    The first two terms are the two-pass kernel's (sum (x - m~)^2 = n var + n (m~ - m)^2 exactly).  The last is
    the merged form's: n var = sum_i M2_i + n_i (m_i - m)^2 over chunks i, whose computed chunk means m~_i = m_i +
    e_i, |e_i| <= gamma(D) rms_i, enter the between-chunk term to first order, 2 sum n_i (m_i - m) e_i <= 2 n
    sqrt(var) gamma(D) rms (Cauchy-Schwarz, sum n_i rms_i^2 = n rms^2).  It depends on n = S cg (through D) and on
    var and mean only: NOT on where in the frame any value lies, so it cannot absorb a cancellation that comes
    from a value's position (the first-value shift of the one-pass variance this route used before)."""
    Fr, S, C = x.shape
    xg = x.view(Fr, S, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    D = gn_depth(S, C, groups)
    dmean = gam(D) * (var + mean ** 2).sqrt()
    dvar = gam(D) * (var + dmean ** 2) + dmean ** 2 + 2 * var.sqrt() * dmean
    return xg, mean, var, dmean, dvar


def groupnorm_ref_bound(x, g, b, groups, eps):
    """GroupNorm of x [F, S, C] (fp16 values) over (S, C / groups) per frame and group -> (ref, bound) [F, S, C].
    Both routes (groupnorm_kernel<8|4|2>, vda_norm.hip:160-208; gn_partial / gn_finalize / gn_apply) keep fp32 up
    to the one fp16 store (:204; gn_apply's fp16(fma(x, sc, of))): half an fp16 ulp + the fp32 terms of _norm_out
    + the statistics term of _gn_stats."""
    x, g, b = map(d, (x, g, b))
    Fr, S, C = x.shape
    xg, mean, var, dmean, dvar = _gn_stats(x, groups, eps)
    gg, bb = g.view(1, 1, groups, -1), b.view(1, 1, groups, -1)
    ref, bound, _ = _norm_out(xg, mean, (var + eps) ** -0.5, gg, bb, dmean, dvar, eps)
    return ref.reshape(Fr, S, C), bound.reshape(Fr, S, C)


def gn_stats_ref_bound(x, groups, eps):
    """(mean, rstd) per (frame, group) [F, groups, 2] and their bound (for the emulations' statistics)."""
    x = d(x)
    xg, mean, var, dmean, dvar = _gn_stats(x, groups, eps)
    rstd = (var + eps) ** -0.5
    one = torch.ones_like(mean)
    _, _, drel = _norm_out(mean, mean, rstd, one, one, dmean, dvar, eps)
    f = lambda t: t.reshape(x.shape[0], groups)  # noqa: E731
    return torch.stack([f(mean), f(rstd)], -1), torch.stack([f(dmean + U32 * mean.abs()) + 2.0 ** -140, f(rstd * drel)], -1)


def emulate_groupnorm_two_pass(x, g, b, groups, eps):
    """groupnorm_kernel<VW>: thread t of the (frame, group) block sums vectors t, t + 256, .. of the [S, cg] slab
    (VW values each, in order), wave tree, red[0] + red[1] + red[2] + red[3]; mean = s / n; the same order for
    q += d * d (contracted to an fma); y = fp16(fma((v - mean) * rstd, g, b))."""
    x, g, b = (t.detach().to("cpu", torch.float32) for t in (x, g, b))
    Fr, S, C = x.shape
    cg = C // groups
    vw = 8 if cg % 8 == 0 else 4 if cg % 4 == 0 else 2
    n = S * cg
    it = -(-n // (256 * vw))
    flat = x.view(Fr, S, groups, cg).permute(0, 2, 1, 3).reshape(Fr * groups, n)
    xp = F.pad(flat, (0, it * 256 * vw - n)).view(-1, it, 256, vw)
    live = (torch.arange(it * 256 * vw) < n).view(it, 256, vw)

    def block_sum(term):
        s = torch.zeros(xp.shape[0], 256)
        for i in range(it):
            for j in range(vw):
                s = torch.where(live[i, :, j], term(s, xp[:, i, :, j]), s)
        w = wave_tree(s.view(-1, 4, 64))
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    cnt = float(S) * float(cg)
    mean = block_sum(lambda s, v: s + v) / cnt
    q = block_sum(lambda s, v: fma32(v - mean[:, None], v - mean[:, None], s))
    rstd = torch.rsqrt(q / cnt + torch.tensor(eps, dtype=torch.float32))
    mean, rstd = mean.view(Fr, 1, groups, 1), rstd.view(Fr, 1, groups, 1)
    xg = x.view(Fr, S, groups, cg)
    gg, bb = g.view(1, 1, groups, cg).expand_as(xg), b.view(1, 1, groups, cg).expand_as(xg)
    return fma32((xg - mean) * rstd, gg, bb).half().view(Fr, S, C)


def _gn_chunks(x):
    """x [F, S, C] fp32 -> (xc [F, nchunk, nr, rpi, C] zero-padded, live [nchunk, nr, rpi] bool, rows [nchunk]):
    thread (row-lane q, chunk column) of block (frame, chunk) owns rows chunk * gn_rows + q + i * rpi, i < nr."""
    Fr, S, C = x.shape
    _, rpi, nr = gn_layout(C)
    R = gn_rows(C)
    nchunk = -(-S // R)
    xs = F.pad(x, (0, 0, 0, nchunk * R - S)).view(Fr, nchunk, R, C)
    xc = F.pad(xs, (0, 0, 0, nr * rpi - R)).view(Fr, nchunk, nr, rpi, C)
    local = torch.arange(nr * rpi).view(1, nr, rpi)
    rows = (S - torch.arange(nchunk) * R).clamp_max(R)
    live = local < rows.view(-1, 1, 1)
    return xc, live, rows


def _gn_apply(x, mean, rstd, g, b, groups, chunk_group=False):
    """gn_apply_kernel (vda_norm.hip): sc = rstd * g, of = fma(-mean, sc, b), y = fp16(fma(x, sc, of)), the group
    looked up per CHANNEL.  chunk_group=True: a MUTANT that takes the group of its 8-channel chunk's first channel
    for all eight (wrong wherever a chunk spans two groups, cg = 2, 4, 6, 12; test_fp16_bounds.py only)."""
    Fr, S, C = x.shape
    cg = C // groups
    ch = torch.arange(C)
    grp = (ch // 8 * 8 if chunk_group else ch) // cg
    mc, rc = mean[:, grp].view(Fr, 1, C), rstd[:, grp].view(Fr, 1, C)
    sc = rc * g.view(1, 1, C)
    of = fma32(-mc, sc, b.view(1, 1, C).expand_as(sc))
    return fma32(x, sc.expand_as(x), of.expand_as(x)).half()


def _gn_finalize_lanes(vals, groups):
    """[F, nchunk, C] -> [F, groups, 64 lanes, per-lane sequence]: entry i = chunk * cg + channel of the group goes
    to lane i % 64, step i / 64 (gn_finalize_kernel's loop); also returns the live mask of the padded steps."""
    Fr, nchunk, C = vals.shape
    cg = C // groups
    n = nchunk * cg
    steps = -(-n // 64)
    v = vals.view(Fr, nchunk, groups, cg).permute(0, 2, 1, 3).reshape(Fr, groups, n)
    v = F.pad(v, (0, steps * 64 - n)).view(Fr, groups, steps, 64)
    return v, (torch.arange(steps * 64) < n).view(steps, 64)


def emulate_groupnorm_ws(x, g, b, groups, eps, stats_only=False, chunk_group=False):
    """gn_partial_kernel / gn_finalize_kernel / gn_apply_kernel as they stand: per (frame, chunk) block each
    thread sums its nr rows per channel, the rpi row-lanes are folded in order, chunk mean = sum * (1 / rows);
    M2 = fma(d, d, M2) with d = x - chunk mean in the same order and fold; gn_finalize: lane i % 64 takes pair i,
    a1 = fma(rows, mean_i, a1), wave tree, mean = a1 / n; a2 += fma(rows * d, d, M2_i), wave tree,
    rstd = rsqrt(a2 / n + eps)."""
    x, g, b = (t.detach().to("cpu", torch.float32) for t in (x, g, b))
    Fr, S, C = x.shape
    cg = C // groups
    xc, live, rows = _gn_chunks(x)
    nchunk, nr, rpi = live.shape

    def fold(term):
        s = torch.zeros(Fr, nchunk, rpi, C)
        for i in range(nr):
            s = torch.where(live[None, :, i, :, None], term(s, xc[:, :, i]), s)
        a = torch.zeros(Fr, nchunk, C)
        for q in range(rpi):
            a = a + s[:, :, q]
        return a
    rowsf = rows.float()
    cm = fold(lambda s, v: s + v) * (1.0 / rowsf).view(1, -1, 1)
    m2 = fold(lambda s, v: fma32(v - cm[:, :, None], v - cm[:, :, None], s))
    cnt = float(S) * float(cg)
    rw = rowsf.view(1, -1, 1).expand(Fr, nchunk, C).contiguous()
    mv, lv = _gn_finalize_lanes(cm, groups)
    rv, _ = _gn_finalize_lanes(rw, groups)
    m2v, _ = _gn_finalize_lanes(m2, groups)
    a1 = torch.zeros(Fr, groups, 64)
    for s_ in range(mv.shape[2]):
        a1 = torch.where(lv[s_], fma32(rv[:, :, s_], mv[:, :, s_], a1), a1)
    mean = wave_tree(a1) / cnt
    a2 = torch.zeros(Fr, groups, 64)
    for s_ in range(mv.shape[2]):
        dd = mv[:, :, s_] - mean[..., None]
        a2 = torch.where(lv[s_], a2 + fma32(rv[:, :, s_] * dd, dd, m2v[:, :, s_]), a2)
    rstd = torch.rsqrt(wave_tree(a2) / cnt + torch.tensor(eps, dtype=torch.float32))
    if stats_only:
        return torch.stack([mean, rstd], -1)
    return _gn_apply(x, mean, rstd, g, b, groups, chunk_group)


def emulate_groupnorm_ws_first_value_shift(x, g, b, groups, eps, stats_only=False):
    """The workspace route AS IT WAS before its repair (kept as the evidence that groupnorm_ref_bound has teeth):
    gn_partial summed d and fma(d, d, .) with d = x - shift, shift = x[f, 0, group's first channel], in the same
    thread / fold order; gn_finalize summed the pairs per lane and the wave tree, md = a1 / n,
    var = max(a2 / n - md * md, 0), mean = shift + md.  An outlier AT the shift position makes a2 / n and md^2 both
    ~ v0^2 and the variance their difference."""
    x, g, b = (t.detach().to("cpu", torch.float32) for t in (x, g, b))
    Fr, S, C = x.shape
    cg = C // groups
    xc, live, rows = _gn_chunks(x)
    nchunk, nr, rpi = live.shape
    sh = x[:, 0].view(Fr, groups, cg)[:, :, :1].expand(Fr, groups, cg).reshape(Fr, 1, 1, C)

    def fold(term):
        s = torch.zeros(Fr, nchunk, rpi, C)
        for i in range(nr):
            s = torch.where(live[None, :, i, :, None], term(s, xc[:, :, i] - sh), s)
        a = torch.zeros(Fr, nchunk, C)
        for q in range(rpi):
            a = a + s[:, :, q]
        return a
    p1, lv = _gn_finalize_lanes(fold(lambda s, dd: s + dd), groups)
    p2, _ = _gn_finalize_lanes(fold(lambda s, dd: fma32(dd, dd, s)), groups)
    a1, a2 = torch.zeros(Fr, groups, 64), torch.zeros(Fr, groups, 64)
    for s_ in range(p1.shape[2]):
        a1 = torch.where(lv[s_], a1 + p1[:, :, s_], a1)
        a2 = torch.where(lv[s_], a2 + p2[:, :, s_], a2)
    cnt = float(S) * float(cg)
    md = wave_tree(a1) / cnt
    var = fma32(-md, md, wave_tree(a2) / cnt).clamp_min(0)
    mean = sh.view(Fr, groups, cg)[:, :, 0] + md
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    if stats_only:
        return torch.stack([mean, rstd], -1)
    return _gn_apply(x, mean, rstd, g, b, groups)


def groupnorm_linear_ref_bound(x, g, b, groups, eps, w, bias=None):
    """GroupNorm -> Linear, y = GN(x) w^T + bias on x [F, S, C], w [N, C] (fp16 values) -> (ref, bound) [F S, N].
    gn_linear_kernel<64|128|256> (vda_norm.hip) multiplies gn_apply's fp16 operand z (the kernel forms the very
    bits of fp16(fma(x, sc, of))), accumulates the K = C products in fp32 MFMAs, adds the bias in fp32 and
    rounds once to fp16; the unfused route is the same operand through vda_gemm.  |z - GN64(x)| <= bz, the
    GroupNorm bound, reaches the output through |w| in the worst case (every operand error with the sign of its
    weight): bound = u16 |ref| + bz |w|^T + gamma(K + 1) ((|GN64| + bz) |w|^T + |bias|) + 2^-24."""
    zr, bz = groupnorm_ref_bound(x, g, b, groups, eps)
    w, bias = d(w), d(bias)
    K = w.shape[1]
    zr, bz = zr.reshape(-1, K), bz.reshape(-1, K)
    ref, A, dz = zr @ w.t(), (zr.abs() + bz) @ w.abs().t(), bz @ w.abs().t()
    if bias is not None:
        ref, A = ref + bias, A + bias.abs()
    return ref, U16 * ref.abs() + dz + gam(K + 1) * A + SUB16


def emulate_groupnorm_linear(x, g, b, groups, eps, w, bias=None, drop=None):
    """drop=(k0, k1): a MUTANT that leaves the K range [k0, k1) out of rows m % 16 == 5 (one lane group's k-step)."""
    z = emulate_groupnorm_ws(x, g, b, groups, eps).float().view(-1, x.shape[-1])
    w = w.detach().to("cpu", torch.float32)
    v = z @ w.t()
    if drop is not None:
        rows = torch.arange(z.shape[0]) % 16 == 5
        v[rows] -= z[rows, drop[0]:drop[1]] @ w[:, drop[0]:drop[1]].t()
    if bias is not None:
        v = v + bias.detach().to("cpu", torch.float32)
    return v.half()


def sums_ref_bound(y16):
    """(sum, sum of squares) of each stored fp16 row [M, N] -> [M, 2] float64 and the bound of an N-term fp32 sum
    in any order with the squares' roundings (gn_linear_kernel's stats_out: N / 4 per lane, then the lane groups)."""
    y = d(y16)
    n = y.shape[1]
    ref = torch.stack([y.sum(-1), (y * y).sum(-1)], -1)
    return ref, gam(n + 8) * torch.stack([y.abs().sum(-1), (y * y).sum(-1)], -1) + 2.0 ** -100


def gn_input(Fr, S, C, seed=0, sigma=1.0, mu=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Fr, S, C, generator=g) * sigma + mu).half().float()


def gn_affine(C, seed=0):
    return rnd32(C, scale=0.1, seed=seed + 11) + 1, rnd32(C, scale=0.1, seed=seed + 12)


# (C, groups): cg = 2, 4, 6, 8, 12, 32, 64, and ViT-B's 12 / 24 of 32 groups (C = 384 / 768); C = 24 / 48: 3 / 6 chunks per row leave idle threads in gn_layout;
# C = 2048: one row-lane (rpi = 1).  S around both gn_rows values (128 below C = 512, 32 from there).
GN_SHAPES = [(64, 32), (128, 32), (24, 4), (256, 32), (48, 4), (1024, 32), (2048, 32), (384, 32), (768, 32)]
GN_S = [1, 2, 31, 32, 33, 127, 128, 129, 257]
GN_FRAMES = [1, 3]


def gn_case(Fr, S, C, seed=0):
    """Random frames; with three frames the middle one carries a +40 offset (the old test's stress)."""
    x = gn_input(Fr, S, C, seed=seed + S + C)
    if Fr == 3:
        x[1] += 40.0
        x = x.half().float()
    return x


# (S, C, v0): the sizes at which an outlier at the group's first position broke the first-value shift
GN_OUTLIER_SIZES = [(5476, 256, 1000.0), (1369, 1024, 2000.0), (21904, 256, 60000.0)]
GN_OUTLIER_KINDS = ("first", "first_sigma0.01", "middle", "first_frame1of3")


def gn_outlier_case(S, C, v0, kind, groups=32):
    """One massive activation v0 per frame in groups 0 and 5: at the group's first value of the frame (row 0, the
    group's first channel), or in the middle of the map; the rest N(0.3, sigma).  Returns (x [F, S, C], frame that
    carries the outlier).  |z| <= sqrt(S cg) ~ 420 at most, finite in fp16."""
    Fr, fo = (3, 1) if kind == "first_frame1of3" else (1, 0)
    x = gn_input(Fr, S, C, seed=S + C, sigma=0.01 if "sigma" in kind else 1.0)
    cg = C // groups
    row = S // 2 + 3 if kind == "middle" else 0
    off = cg // 2 if kind == "middle" else 0
    for grp in (0, 5):
        x[fo, row, grp * cg + off] = v0
    return x, fo


# (C, S, F): M = F S in {1, 15, 16, 17, 128 k +- 1}; S = 5: a 16-row tile spans up to four frames; the last one has
# more 16-row tiles than 8 waves x 256 CUs, so both register sets of the tile loop run
GNL_CASES = [(64, 1, 1), (128, 15, 1), (256, 16, 1), (64, 17, 1), (128, 7, 55), (256, 7, 73), (64, 37, 83), (128, 15, 17),
             (256, 17, 15), (64, 5, 7), (256, 5, 7), (128, 16, 3), (64, 37, 900)]


# =====================================================================================================
# Bilinear resize (csrc/vda_misc.hip upsample_kernel), NHWC
# =====================================================================================================
def _resize_err(x, Ho, Wo):
    """x [BT, H, W, C] float64 -> (ref, A, epos) NHWC: the float64 resize, the resize of |x| and the value error of
    the kernel's fp32 coordinates.  ac_coord / the kernel's x loop (vda_misc.hip:37-43, :81-83): sc = fl((in - 1) /
    (out - 1)), i0 = (int)fl(sc * o), w = fma(sc, o, -i0): the blend is evaluated at p~ = i0 + w with |p~ - p| <=
    u32 (p + |w|) <= u32 in.  When p is an integer, (int) may fall one cell short (w ~ 1) or land on it (w ~ 0):
    bilinear interpolation is continuous across cells, so either way the value moves by at most |p~ - p| times the
    largest difference of horizontally (vertically) adjacent source values of that frame and channel."""
    BT, H, W, C = x.shape
    xc = x.permute(0, 3, 1, 2)
    ref, A = bilinear64(xc, Ho, Wo).permute(0, 2, 3, 1), bilinear64(xc.abs(), Ho, Wo).permute(0, 2, 3, 1)
    z = torch.zeros(BT, 1, 1, C, dtype=torch.float64)
    Dx = (x[:, :, 1:] - x[:, :, :-1]).abs().amax((1, 2), keepdim=True) if W > 1 else z
    Dy = (x[:, 1:] - x[:, :-1]).abs().amax((1, 2), keepdim=True) if H > 1 else z
    return ref, A, U32 * (W * Dx + H * Dy)


def upsample_ref_bound(x, Ho, Wo):
    """vda_upsample_bilinear on x [BT, H, W, C] (fp16 values) -> (ref, bound) [BT, Ho, Wo, C]: bilinear64 as the
    reference; bilerp8 (vda_common.h:68-78) forms ux = 1 - wx, top = fma(wx, b, ux * a), bot likewise, o =
    fp16(fma(wy, bot, (1 - wy) * top)): six fp32 roundings, each relative to a partial blend of |corners| (<= the
    resize A of |x|), 8 u32 A with the second-order terms; the coordinates' error _resize_err; one fp16 rounding."""
    ref, A, epos = _resize_err(d(x), Ho, Wo)
    return ref, U16 * ref.abs() + 8 * U32 * A + epos + SUB16


def emulate_upsample(x, Ho, Wo, stale_pair=False):
    """The kernel's fp32 arithmetic per output.  stale_pair: a MUTANT whose second row of every row pair blends the
    FIRST row's two source rows (with its own wy) even when it may not share them (test_fp16_bounds.py only)."""
    x = x.detach().to("cpu", torch.float32)
    BT, H, W, C = x.shape

    def coord(n_in, n_out):
        o = torch.arange(n_out, dtype=torch.float32)
        sc = torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32) \
            if n_out > 1 else torch.zeros((), dtype=torch.float32)
        i0 = (sc * o).to(torch.int64)
        return i0, (i0 + 1).clamp_max(n_in - 1), fma32(sc.expand_as(o), o, -i0.float())
    y0, y1, wy = coord(H, Ho)
    x0, x1, wx = coord(W, Wo)
    r = torch.arange(BT * Ho)
    bt, oy = r // Ho, r % Ho
    ya, yb, wyr = y0[oy], y1[oy], wy[oy]
    if stale_pair:
        first = r - (r % 2)
        ya, yb, bt = ya[first], yb[first], bt[first]
    wxv, wyv = wx.view(1, Wo, 1), wyr.view(-1, 1, 1)
    ux, uy = 1.0 - wxv, 1.0 - wyv
    xf = x.reshape(BT * H, W, C)
    ra, rb = xf[bt * H + ya], xf[bt * H + yb]  # [rows, W, C]
    e = lambda t: t.expand(BT * Ho, Wo, C)  # noqa: E731
    top = fma32(e(wxv), ra[:, x1], e(ux) * ra[:, x0])
    bot = fma32(e(wxv), rb[:, x1], e(ux) * rb[:, x0])
    return fma32(e(wyv), bot, e(uy) * top).half().view(BT, Ho, Wo, C)


# (BT, H, W, C, Ho, Wo)
UPSAMPLE_CASES = [
    (2, 1, 1, 8, 5, 7), (2, 5, 7, 8, 1, 1), (1, 5, 7, 32, 1, 9), (2, 9, 11, 40, 9, 11),    # from 1x1, to 1x1, 1 x Wo, identity
    (2, 19, 19, 32, 38, 38), (2, 19, 19, 32, 37, 37),                                      # x2 exactly, x2 - 1
    (2, 37, 37, 8, 19, 19), (1, 37, 37, 32, 5, 5),                                         # downscales: pairs never share
    (2, 4, 5, 8, 9, 11), (3, 4, 5, 40, 9, 6), (3, 3, 3, 8, 7, 5),                          # Ho odd: a pair straddles frames; BT Ho odd
    (2, 6, 1, 8, 13, 1), (1, 3, 1, 32, 7, 5),                                              # W = 1
    (1, 5, 8, 256, 9, 15), (1, 5, 8, 256, 9, 16), (1, 5, 8, 256, 9, 17), (1, 5, 8, 256, 9, 33),  # Wo C / 8 = 480, 512, 544, 1056
    (5, 2, 1, 8, 26215, 2),                                                                # 131,075 rows: the gridDim.y stride loop
]


def upsample_input(BT, H, W, C, kind="rand", seed=0):
    if kind == "rand":
        return rnd16(BT, H, W, C, seed=seed + H + W + C)
    i = torch.arange(H).view(1, H, 1, 1) + torch.arange(W).view(1, 1, W, 1) + torch.arange(C).view(1, 1, 1, C)
    return ((i % 2) * 2.0 - 1.0).expand(BT, H, W, C).contiguous() * 60000.0  # checkerboard: corner differences 120,000


# =====================================================================================================
# im2col (exact): index gathers
# =====================================================================================================
def patch_im2col_ref(img, Kp):
    """A [BT (1 + np), Kp] fp16 of img [BT, 3, H, W] fp32: row 0 of each frame zero, then the 14 x 14 patches in
    row-major order with k = ci * 196 + ky * 14 + kx, zero beyond 588; the one rounding is fp16(float)."""
    BT, _, H, W = img.shape
    ph, pw = H // 14, W // 14
    p = img.cpu().view(BT, 3, ph, 14, pw, 14).permute(0, 2, 4, 1, 3, 5).reshape(BT, ph * pw, 588)
    a = torch.zeros(BT, 1 + ph * pw, Kp)
    a[:, 1:, :588] = p
    return a.half().view(-1, Kp)


def conv_im2col_ref(x, ks, stride, pad):
    """A [BT Ho Wo, ks ks Cin] of NHWC x: k = (ky, kx, ci), zeros outside the image."""
    BT, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    oy, ox = torch.arange(Ho) * stride, torch.arange(Wo) * stride
    taps = [xp[:, oy + ky][:, :, ox + kx] for ky in range(ks) for kx in range(ks)]
    return torch.stack(taps, 3).reshape(BT * Ho * Wo, ks * ks * C)


# =====================================================================================================
# Depth tail (csrc/vda_depth_head.hip -> vda_dconv.hip / the implicit-GEMM depth kernel)
# =====================================================================================================
def split_hi_lo(w1):
    """The fp32 3x3 weights [32, C, 3, 3] as the fp16 pair the kernels multiply: hi = fp16(w), lo = fp16(w - hi)."""
    hi = w1.half()
    return hi, (w1 - hi.float()).half()


def depth_head_ref_bound(x, w1, b1, w2, b2, Ho, Wo):
    """depth = relu(b2 + sum_j w2[j] relu(b1[j] + conv3x3_j(U))), U = fp16(resize(x)), x [BT, C, H, W] (fp16
    values), w1 [32, C, 3, 3] fp32, w2 [32] -> (ref, bound) [BT, Ho, Wo], fp32 output (no fp16 store).

    Reference: float64 resize, rounded to fp16, then the conv with the weights hi + lo the kernels really
    multiply (split_hi_lo), everything else float64.  Kernel (vda_dconv.hip:1-11, :392-396; the
    implicit-GEMM depth tail keeps the same terms): 64 MFMA rows, hi and lo accumulated
    separately in fp32 over K = 9 C products each, h_j = relu(acc_hi + acc_lo + b1): gamma(K + 3) of the absolute
    image; then 4 products per lane, two lane-group shuffles and b2: gamma(32 + 2) of sum |w2 h| + |b2|.
    The resized map: the kernels blend in fp32 (bilerp8, _resize_err) and round to fp16, so an element whose
    float64 value lies within that fp32 error e32 of an fp16 rounding boundary may round the other way, a whole
    fp16 ulp; only those elements are budgeted (dU = ulp where the distance to the boundary is <= e32, else 0),
    carried through |hi + lo| as conv_ref_bound(up=...) carries its dx."""
    x, w1, b1, w2, b2 = map(d, (x, w1, b1, w2, b2))
    hi, lo = split_hi_lo(w1.float())
    hi, lo = hi.double(), lo.double()
    xn = x.permute(0, 2, 3, 1)
    u64, A, epos = _resize_err(xn, Ho, Wo)
    e32 = 8 * U32 * A + epos
    U = u64.half().double()
    ulp = torch.where(u64.abs() >= 2.0 ** -14, 2.0 ** (torch.floor(torch.log2(u64.abs().clamp_min(2.0 ** -14))) - 10),
                      torch.full_like(u64, 2.0 ** -24))
    dU = torch.where(0.5 * ulp - (u64 - U).abs() <= e32, 2 * ulp, torch.zeros_like(ulp))  # 2 ulp: a binade edge
    U, dU = U.permute(0, 3, 1, 2), dU.permute(0, 3, 1, 2)
    K = 9 * x.shape[1]
    pre = F.conv2d(U, hi + lo, b1, padding=1)
    Ah = F.conv2d(U.abs(), hi.abs() + lo.abs(), b1.abs(), padding=1)
    dh = gam(K + 3) * Ah + F.conv2d(dU, (hi + lo).abs(), None, padding=1)
    hj = pre.clamp_min(0)
    w2v = w2.view(1, -1, 1, 1)
    out = (hj * w2v).sum(1) + b2
    dout = (dh * w2v.abs()).sum(1) * (1 + gam(34)) + gam(32 + 2) * ((hj * w2v).abs().sum(1) + b2.abs())
    return out.clamp_min(0), dout + 2.0 ** -60


def emulate_depth_head(x, w1, b1, w2, b2, Ho, Wo, no_relu=False):
    """fp32: the emulated resize rounded to fp16, the hi and lo convs accumulated separately, the fp32 tail.
    no_relu: a MUTANT without the ReLU between the 3x3 and the 1x1 conv (test_fp16_bounds.py only)."""
    x, w1, b1, w2, b2 = (t.detach().to("cpu", torch.float32) for t in (x, w1, b1, w2, b2))
    U = emulate_upsample(x.permute(0, 2, 3, 1), Ho, Wo).float().permute(0, 3, 1, 2)
    hi, lo = split_hi_lo(w1)
    hj = F.conv2d(U, hi.float(), None, padding=1) + F.conv2d(U, lo.float(), None, padding=1) + b1.view(1, -1, 1, 1)
    if not no_relu:
        hj = F.relu(hj)
    return F.relu((hj * w2.view(1, -1, 1, 1)).sum(1) + b2)


def depth_head_case(C, Hin, Win, BT, seed=0):
    x = rnd16(BT, C, Hin, Win, seed=seed + 45)
    w1 = torch.randn(32, C, 3, 3, generator=torch.Generator().manual_seed(seed + 46)) * (9 * C) ** -0.5
    return x, w1, rnd32(32, scale=0.1, seed=seed + 47), rnd32(32, seed=seed + 48).abs() * 0.2, torch.tensor([0.05])


# (C, Hin, Win, Ho, Wo): C = 40 takes the implicit-GEMM depth kernel (C % 32 != 0); 37 -> 19 is the downscale
DEPTH_CASES = [(32, 1, 1, 1, 1), (64, 1, 1, 16, 16), (128, 9, 9, 15, 17), (64, 8, 20, 33, 47), (32, 16, 16, 16, 16),
               (64, 37, 37, 19, 19), (40, 9, 9, 15, 17)]
