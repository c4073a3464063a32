"""Float64 references, derived per-element error bounds and CPU emulations for the fp16 kernels.

Shared by tests/test_fp16_bounds.py (CPU: every emulation lies inside its bound) and
tests/test_gpu_fp16_edges.py (GPU: every kernel output lies inside the same bound); DESIGN.md
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
    staged=True, the phased kernels (vda_gemm_phased.h: the LDS-staged epilogue's phase 1 / phase 2 and the
    register epilogue EK 2): t = gamma * act(...) is rounded to fp16, then res and res2 are added as packed
    fp16 vectors, one rounding per add, so t and (with both residuals) t + res are intermediates v_i.
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


def row_stats_ref_bound(y16):
    """The stats_out partials of stored fp16 rows y16 [M, parts * 256]: (sum, sum of squares) per 256-column part
    in float64 [M, parts, 2] and their bound: a 256-term fp32 sum in any order (per lane, across lanes, across
    the four waves of a block) with the squares' own roundings, gamma(256 + 8) of the absolute sums."""
    y = d(y16).reshape(y16.shape[0], -1, 256)
    ref = torch.stack([y.sum(-1), (y * y).sum(-1)], -1)
    A = torch.stack([y.abs().sum(-1), (y * y).sum(-1)], -1)
    return ref, gam(256 + 8) * A + 2.0 ** -100


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
