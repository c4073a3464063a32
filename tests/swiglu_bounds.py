"""Float64 reference, derived per-element bound and CPU emulation of the SwiGLU GEMM (VDA_ACT_SWIGLU).

In the manner of tests/fp16_bounds.py (gemm_ref_bound / emulate_gemm), whose linear part, LayerNorm-fold terms and
rounding model this file takes over unchanged; only the gate differs.  The kernel computes, on the fp32 accumulators
h~ = x w^T + b and g~ = x wg^T + bg (each within d_h, d_g of its float64 value, the gamma(K + c) A terms of
fp16_bounds),

    y = fp16( h~ * silu(g~) ),   silu(v) = v * rcp(1 + exp2(v * -log2(e)))        (vda_common.h silu_f32)

Gate error, |silu~(g~) - silu(g)| <= silu_err(g, d_g), term by term:
  * |silu'| <= 1.0999 everywhere (its maximum, at v = 2.3994): the argument's error carries over as 1.1 d_g;
  * t = v * c, c = fp32(-log2 e): the product's rounding and the constant's own are each relative u32 of t, and a
    relative error r of an exponent t moves exp2(t) by |t| ln2 r = |v| r: 2 |v| u32; v_exp_f32 itself is within one
    fp32 ulp (2^-23): e~ = e (1 + eps_e), |eps_e| <= 2 |v| u32 + 2 u32, e = exp(-v);
  * s = 1 / (1 + e): d s / s = (e / (1 + e)) eps_e = (1 - s) eps_e, plus the add's rounding (u32) and v_rcp_f32's
    one ulp (2 u32);
  * the product v * s rounds once more (u32).
  So d silu = |silu(v)| ((1 - s) (2 |v| + 2) u32 + 4 u32).  Where e overflows to +inf (v < -88.7) the kernel gives
  v * 0 = -0 against |v| e^v < 1e-36, and where it underflows s = 1 against 1 - e: both far inside the 2^-24 term.
Then v = h * silu(g): d v = |silu| d_h + |h| d silu + d_h d silu + u32 |v| (the product), an optional gamma and
residuals exactly as gemm_ref_bound treats them, and the one fp16 rounding of the store, u16 |v| + 2^-24.
No factor is fitted to a kernel's output.
"""
import torch
import torch.nn.functional as F

import fp16_bounds as fb
from fp16_bounds import U16, U32, SUB16, d, gam

LOG2E_F32 = 1.4426950408889634  # rounded to fp32 where it is used


def silu64(v):
    return v * torch.sigmoid(v)


def silu_err(v, dv):
    s = torch.sigmoid(v)
    return 1.1 * dv + silu64(v).abs() * ((1 - s) * (2 * v.abs() + 2) * U32 + 4 * U32)


def _ln_terms(x, ln):
    """(mean, rstd, dmean, drel) [M, 1] float64 of fp16_bounds.gemm_ref_bound's LayerNorm fold (same derivation)."""
    K = x.shape[1]
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
    return tuple(t[:, None] for t in (mean, rstd, dmean, drel))


def swiglu_ref_bound(x, w, wg, *, bias=None, bg=None, gamma=None, res=None, staged=False, ln=None):
    """y = res + gamma * ((x w^T + bias) * silu(x wg^T + bg)): w / bias the value half (the reference's x2 rows), wg /
    bg the gate half (x1).  staged: the phased kernel (t = gamma * v rounded to fp16, then res added in fp16); else
    the tile kernels (fp32 up to the one store).  ln: as fp16_bounds.gemm_ref_bound (colsum / colsum_g)."""
    x, w, wg, bias, bg, gamma, res = map(d, (x, w, wg, bias, bg, gamma, res))
    K = x.shape[1]
    if ln is not None:
        mean, rstd, dmean, drel = _ln_terms(x, ln)

    def lin(wt, b, colsum):
        pre, A = x @ wt.t(), x.abs() @ wt.abs().t()
        c, dstat = 0, 0.0
        if ln is not None:
            cs = d(colsum)[None, :]
            A = rstd * (A + (mean * cs).abs())
            pre = rstd * (pre - mean * cs)
            dstat = (rstd * cs.abs() * dmean + drel * pre.abs()) * (1 + drel)
            c = 2
        if b is not None:
            pre, A, c = pre + b, A + b.abs(), c + 1
        return pre, gam(K + c) * A + dstat

    hv, dh = lin(w, bias, None if ln is None else ln["colsum"])
    g, dg = lin(wg, bg, None if ln is None else ln["colsum_g"])
    sg, dsg = silu64(g), silu_err(g, dg)
    v = hv * sg
    dv = sg.abs() * dh + hv.abs() * dsg + dh * dsg + U32 * v.abs()
    if gamma is not None:
        v, dv = gamma * v, gamma.abs() * dv + U32 * (gamma * v).abs()
    if staged:
        inter = 0.0
        if res is not None:
            inter = v.abs()
            v = v + res
        return v, U16 * (v.abs() + inter) + dv + SUB16
    if res is not None:
        dv = dv * (1 + U32) + U32 * (v.abs() + res.abs())
        v = v + res
    return v, U16 * v.abs() + dv + SUB16


def silu_kernel32(v):
    """silu_f32 in fp32 torch: v * (1 / (1 + exp2(v * -log2e)))."""
    c = torch.tensor(-LOG2E_F32, dtype=torch.float32)
    return v * (1.0 / (1.0 + torch.exp2(v * c)))


def emulate_swiglu(x, w, wg, *, bias=None, bg=None, gamma=None, res=None, staged=False, ln=None, mutant=None):
    """The kernel's arithmetic in fp32 torch, .half() at its rounding points.  mutant: None (faithful), "swap" (the
    gate applied to the value half: silu(h) * g), "gelu" (GELU in place of SiLU), "expform" (v * exp(v) / (1 + exp(v)),
    inf / inf beyond v = 88.7)."""
    f = lambda t: None if t is None else t.detach().to("cpu", torch.float32)  # noqa: E731
    x, w, wg, bias, bg, gamma, res = map(f, (x, w, wg, bias, bg, gamma, res))
    if ln is not None:
        K = x.shape[1]
        if "parts" in ln:
            pt = f(ln["parts"])
            mean = pt[..., 0].sum(1) / K
            rstd = torch.rsqrt((pt[..., 1].sum(1) / K - mean * mean).clamp_min(0) + ln["eps"])
        else:
            mean, rstd = f(ln["mean"]), f(ln["rstd"])

    def lin(wt, b, colsum):
        v = x @ wt.t()
        if ln is not None:
            v = rstd[:, None] * (v - mean[:, None] * f(colsum)[None, :])
        return v if b is None else v + b

    hv = lin(w, bias, None if ln is None else ln["colsum"])
    g = lin(wg, bg, None if ln is None else ln["colsum_g"])
    if mutant == "swap":
        v = g * silu_kernel32(hv)
    elif mutant == "gelu":
        v = hv * F.gelu(g)
    elif mutant == "expform":
        e = torch.exp(g)
        v = hv * (g * (e / (1.0 + e)))
    else:
        assert mutant is None
        v = hv * silu_kernel32(g)
    if gamma is not None:
        v = v * gamma
    if staged:
        v = v.half().float()
    if res is not None:
        v = v + res
    return v.half()


def swiglu_case(M, N, K, seed=0):
    """fp16_bounds.gemm_case's GEGLU family (N = 2 I interleaved rows) for SwiGLU: the same inputs."""
    c = fb.gemm_case(M, N, K, "geglu", seed=seed)
    c["epi"] = "swiglu"
    c["kw"] = {k: v for k, v in c["kw"].items() if k != "act"}
    return c


def swiglu_ln_case(M, N, K, seed=0, parts=False):
    """fp16_bounds.gemm_ln_case's ln_geglu family for SwiGLU; parts: three-part (sum, sum of squares) statistics."""
    c = fb.gemm_ln_case(M, N, K, "ln_geglu", seed=seed)
    c["kw"] = {k: v for k, v in c["kw"].items() if k != "act"}
    if parts:
        x64 = c["x"].double().view(M, 3, K // 3)
        ln = c["kw"]["ln"]
        c["kw"]["ln"] = dict(parts=torch.stack([x64.sum(-1), (x64 * x64).sum(-1)], -1).float(), eps=1e-6,
                             colsum=ln["colsum"], colsum_g=ln["colsum_g"])
    return c


def planted_case(M, I, K, seed=0):
    """Gate pre-activations planted at +-30 and +-100 (exactly: x rows are one-hot selectors of K gate-weight columns
    holding those values and the edges of exp's fp32 range, +-88 / +-89; the gate bias zero), value pre-activations
    ordinary: the product must be finite and correct."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0, 11.0, -11.0, 88.0, -88.0, 89.0, -89.0])
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    wg = vals[torch.randint(0, len(vals), (I, K), generator=g)]
    w = (torch.randn(I, K, generator=g)).half().float()
    return dict(M=M, N=2 * I, K=K, x=x, w=w, kw=dict(wg=wg, bias=fb.rnd32(I, scale=0.1, seed=seed + 1), bg=torch.zeros(I)))
