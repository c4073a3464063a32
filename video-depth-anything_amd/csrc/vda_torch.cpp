// torch.ops.vda.* — the libvda kernels registered as native PyTorch operators (TORCH_LIBRARY).
//
// The reference's op-level boundary is xformers.ops.memory_efficient_attention plus plain
// nn.Linear / nn.Conv2d / F.layer_norm / F.group_norm / F.interpolate calls inside its modules
// (dinov2_layers/attention.py:72-76, motion_module.py:309-313); here every hot op
// is one operator of the `vda` library.  Each kernel:
//   * checks device / dtype / layout with TORCH_CHECK (-> RuntimeError in Python);
//   * allocates its output (and any workspace) through the PyTorch caching allocator on the
//     input's device;
//   * launches on the current HIP stream of that device through the C ABI of include/vda.h
//     (libvda.so), and turns a non-zero return code into a c10::Error carrying vda_last_error().
// The same function serves the CUDA (HIP) key and the Meta key (shape / dtype only, no launch), so
// the ops trace under fake tensors.  There is deliberately no CPU kernel: a CPU tensor reaches the
// dispatcher's "no kernel" error (NotImplementedError), never a silent fallback.
// Activation dtype follows the input: fp16 (the shipped mode) or fp32 (fp32 mode, the *_f32 entry
// points).  Inference only: the ops are registered without autograd formulas.
#include <ATen/ATen.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <array>
#include <cstring>

#include "vda.h"

namespace {

using at::Tensor;
using c10::optional;
using OptT = const optional<Tensor>&;

void* stream_of(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed (rc=", rc, "): ", vda_last_error());
}

void need(const Tensor& t, at::ScalarType dt, const char* name, const Tensor& like) {
  TORCH_CHECK(t.device() == like.device(), "vda op: ", name, " must be on ", like.device(), " (got ", t.device(),
              "; there is no CPU path in the product)");
  TORCH_CHECK(t.scalar_type() == dt, "vda op: ", name, " must be ", dt, ", got ", t.scalar_type());
}

void need_contig(const Tensor& t, at::ScalarType dt, const char* name, const Tensor& like) {
  need(t, dt, name, like);
  TORCH_CHECK(t.is_contiguous(), "vda op: ", name, " must be contiguous");
}

at::ScalarType act_dtype(const Tensor& x) {
  TORCH_CHECK(x.scalar_type() == at::kHalf || x.scalar_type() == at::kFloat,
              "vda op: activations must be float16 or float32, got ", x.scalar_type());
  return x.scalar_type();
}

const void* ptr(OptT t) { return t.has_value() ? t->data_ptr() : nullptr; }

// vda_epilogue from the optional per-channel / per-row / residual operands (include/vda.h).
vda_epilogue make_epi(const Tensor& x, OptT bias, OptT rowbias, int64_t rdiv, int64_t rmod, OptT gamma, OptT res,
                      OptT res2, int64_t act, at::ScalarType dt, OptT ln_stats = c10::nullopt,
                      OptT ln_colsum = c10::nullopt, int64_t ln_parts = 0, double ln_eps = 1e-6,
                      OptT stats_out = c10::nullopt) {
  vda_epilogue e;
  std::memset(&e, 0, sizeof(e));
  if (bias) need_contig(*bias, at::kFloat, "bias", x);
  if (rowbias) need_contig(*rowbias, at::kFloat, "rowbias", x);
  if (gamma) need_contig(*gamma, at::kFloat, "gamma", x);
  e.bias = (const float*)ptr(bias);
  e.rowbias = (const float*)ptr(rowbias);
  e.gamma = (const float*)ptr(gamma);
  e.rdiv = (int32_t)rdiv;
  e.rmod = (int32_t)rmod;
  if (res) {
    need(*res, dt, "res", x);
    TORCH_CHECK(res->stride(-1) == 1, "vda op: res must have unit column stride");
    e.res = res->data_ptr();
    e.ldres = res->dim() >= 2 ? res->stride(-2) : res->size(-1);
  }
  if (res2) {
    need(*res2, dt, "res2", x);
    TORCH_CHECK(res2->stride(-1) == 1, "vda op: res2 must have unit column stride");
    e.res2 = res2->data_ptr();
    e.ldres2 = res2->dim() >= 2 ? res2->stride(-2) : res2->size(-1);
  }
  e.act = (int32_t)act;
  e.store = VDA_STORE_ROWS;
  if (ln_stats) {
    TORCH_CHECK(ln_colsum.has_value(), "vda gemm: ln_stats needs ln_colsum");
    need_contig(*ln_stats, at::kFloat, "ln_stats", x);
    need_contig(*ln_colsum, at::kFloat, "ln_colsum", x);
    if (ln_parts > 0) {
      TORCH_CHECK(ln_parts <= 4 && ln_stats->dim() == 3 && ln_stats->size(0) >= x.size(0) &&
                      ln_stats->size(1) == ln_parts && ln_stats->size(2) == 2,
                  "vda gemm: with ln_parts = P, ln_stats must be [M, P, 2] partial sums (a GEMM's stats_out), P <= 4");
    } else {
      TORCH_CHECK(ln_stats->dim() == 2 && ln_stats->size(1) == 2 && ln_stats->size(0) >= x.size(0),
                  "vda gemm: ln_stats must be [M, 2] (from vda.row_stats)");
    }
    e.ln_stats = (const float*)ln_stats->data_ptr();
    e.ln_colsum = (const float*)ln_colsum->data_ptr();
    e.ln_parts = (int32_t)ln_parts;
    e.ln_eps = (float)ln_eps;
  }
  if (stats_out) {
    need_contig(*stats_out, at::kFloat, "stats_out", x);
    e.stats_out = (float*)stats_out->data_ptr();
  }
  return e;
}

// ---- linear / 1x1 conv / ConvTranspose(k=s) ------------------------------------------------------
// rows of the GEMM output: M, or M - ceil(M / drop_period) with the cls rows dropped (vda.h drop_period)
int64_t gemm_out_rows(int64_t M, int64_t drop_period) { return drop_period > 0 ? M - (M + drop_period - 1) / drop_period : M; }

Tensor gemm_into(const Tensor& x, const Tensor& w, OptT bias, OptT rowbias, int64_t rdiv, int64_t rmod, OptT gamma,
                 OptT res, OptT res2, int64_t act, OptT ln_stats, OptT ln_colsum, int64_t ln_parts, double ln_eps,
                 OptT stats_out, OptT sched, int64_t drop_period, Tensor out) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "vda gemm: x must be a 2-D row-major (possibly row-strided) matrix");
  need_contig(w, dt, "w", x);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == x.size(1), "vda gemm: K mismatch ", w.sizes(), " vs ", x.sizes());
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  const int64_t nout = (act == VDA_ACT_GEGLU || act == VDA_ACT_SWIGLU) ? N / 2 : N;
  TORCH_CHECK(drop_period >= 0, "vda gemm: drop_period >= 0");
  const int64_t Mo = gemm_out_rows(M, drop_period);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == Mo && out.size(1) == nout && out.stride(1) == 1 &&
                  out.scalar_type() == dt && out.device() == x.device(),
              "vda gemm: out must be [", Mo, ", ", nout, "] ", dt, " with unit column stride");
  if (stats_out)
    TORCH_CHECK(stats_out->dim() == 3 && stats_out->size(0) >= M && stats_out->size(1) == (nout + 255) / 256 &&
                    stats_out->size(2) == 2 && stats_out->scalar_type() == at::kFloat && stats_out->is_contiguous(),
                "vda gemm: stats_out must be a contiguous float [M, ceil(N / 256), 2]");
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  vda_epilogue e = make_epi(x, bias, rowbias, rdiv, rmod, gamma, res, res2, act, dt, ln_stats, ln_colsum, ln_parts,
                            ln_eps, stats_out);
  if (sched) {  // the caller's per-stream tile-scheduler counters (vda.h vda_epilogue.sched)
    need_contig(*sched, at::kInt, "sched", x);
    TORCH_CHECK(sched->numel() >= 9, "vda gemm: sched must hold >= 9 int32 counters");
    e.sched = (int32_t*)sched->data_ptr();
  }
  e.drop_period = (int32_t)drop_period;
  const int rc = dt == at::kHalf
                     ? vda_gemm(x.data_ptr(), x.stride(0), w.data_ptr(), out.data_ptr(), out.stride(0), (int32_t)M,
                                (int32_t)N, (int32_t)K, &e, stream_of(x))
                     : vda_gemm_f32((const float*)x.data_ptr(), x.stride(0), (const float*)w.data_ptr(),
                                    (float*)out.data_ptr(), out.stride(0), (int32_t)M, (int32_t)N, (int32_t)K, &e,
                                    stream_of(x));
  check_rc(rc, "vda_gemm");
  return out;
}

Tensor gemm(const Tensor& x, const Tensor& w, OptT bias, OptT rowbias, int64_t rdiv, int64_t rmod, OptT gamma,
            OptT res, OptT res2, int64_t act, OptT ln_stats, OptT ln_colsum, int64_t ln_parts, double ln_eps,
            OptT stats_out, OptT sched, int64_t drop_period) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "vda gemm: x and w must be 2-D");
  const int64_t nout = (act == VDA_ACT_GEGLU || act == VDA_ACT_SWIGLU) ? w.size(0) / 2 : w.size(0);
  Tensor out = at::empty({gemm_out_rows(x.size(0), drop_period), nout}, x.options().dtype(dt));
  return gemm_into(x, w, bias, rowbias, rdiv, rmod, gamma, res, res2, act, ln_stats, ln_colsum, ln_parts, ln_eps,
                   stats_out, sched, drop_period, out);
}

Tensor& gemm_out(const Tensor& x, const Tensor& w, OptT bias, OptT rowbias, int64_t rdiv, int64_t rmod, OptT gamma,
                 OptT res, OptT res2, int64_t act, OptT ln_stats, OptT ln_colsum, int64_t ln_parts, double ln_eps,
                 OptT stats_out, OptT sched, int64_t drop_period, Tensor& out) {
  gemm_into(x, w, bias, rowbias, rdiv, rmod, gamma, res, res2, act, ln_stats, ln_colsum, ln_parts, ln_eps, stats_out,
            sched, drop_period, out);
  return out;
}

Tensor conv_transpose_ks(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t BT, int64_t h, int64_t w_,
                         int64_t k) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "vda conv_transpose_ks: x must be a contiguous [BT*h*w, Cin] matrix");
  need_contig(w, dt, "w", x);
  need_contig(bias, at::kFloat, "bias", x);
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(k > 0 && N % (k * k) == 0 && w.size(1) == K && M == BT * h * w_, "vda conv_transpose_ks: bad geometry");
  const int64_t cout = N / (k * k);
  Tensor out = at::empty({BT, h * k, w_ * k, cout}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  vda_epilogue e;
  std::memset(&e, 0, sizeof(e));
  e.bias = (const float*)bias.data_ptr();
  e.rdiv = e.rmod = 1;
  e.store = VDA_STORE_PIXEL_SHUFFLE;
  e.ps_k = (int32_t)k; e.ps_cout = (int32_t)cout; e.ps_hin = (int32_t)h; e.ps_win = (int32_t)w_;
  const int rc = dt == at::kHalf
                     ? vda_gemm(x.data_ptr(), K, w.data_ptr(), out.data_ptr(), N, (int32_t)M, (int32_t)N, (int32_t)K,
                                &e, stream_of(x))
                     : vda_gemm_f32((const float*)x.data_ptr(), K, (const float*)w.data_ptr(), (float*)out.data_ptr(),
                                    N, (int32_t)M, (int32_t)N, (int32_t)K, &e, stream_of(x));
  check_rc(rc, "vda_gemm(pixel-shuffle)");
  return out;
}

// ConvTranspose(k = s) + 3x3 conv composed into one sub-pixel conv (vda.h vda_subpixel_conv): x [BT*h*w, Cin]
// half, w the packed phase groups (flat), bias9 [9, Cout] fp32 -> [BT, s h, s w, Cout]
Tensor subpixel_conv(const Tensor& x, const Tensor& w, const Tensor& bias9, int64_t BT, int64_t h, int64_t w_,
                     int64_t s) {
  TORCH_CHECK(x.scalar_type() == at::kHalf, "vda subpixel_conv: fp16 only");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && x.size(0) == BT * h * w_,
              "vda subpixel_conv: x must be a contiguous [BT*h*w, Cin] matrix");
  need_contig(w, at::kHalf, "w", x);
  need_contig(bias9, at::kFloat, "bias9", x);
  TORCH_CHECK(bias9.dim() == 2 && bias9.size(0) == 9, "vda subpixel_conv: bias9 must be [9, Cout]");
  const int64_t Cin = x.size(1), Cout = bias9.size(1);
  // s = 2: one 2x2 group; s = 4: 2x2 + 1x2 + 2x1 + 1x1 groups of four phases each
  TORCH_CHECK((s == 2 || s == 4) && w.numel() == 4 * Cout * Cin * (s == 2 ? 4 : 9),
              "vda subpixel_conv: w must hold the packed phase groups of s = ", s);
  Tensor out = at::empty({BT, h * s, w_ * s, Cout}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  check_rc(vda_subpixel_conv_check((int32_t)BT, (int32_t)h, (int32_t)w_, (int32_t)Cin, (int32_t)Cout, (int32_t)s),
           "vda_subpixel_conv_check");
  const int64_t wsb = vda_subpixel_conv_workspace((int32_t)BT, (int32_t)h, (int32_t)w_, (int32_t)Cin, (int32_t)s);
  Tensor ws = at::empty({wsb}, x.options().dtype(at::kByte));
  check_rc(vda_subpixel_conv(x.data_ptr(), w.data_ptr(), (const float*)bias9.data_ptr(), out.data_ptr(), (int32_t)BT,
                             (int32_t)h, (int32_t)w_, (int32_t)Cin, (int32_t)Cout, (int32_t)s, ws.data_ptr(), wsb,
                             stream_of(x)),
           "vda_subpixel_conv");
  return out;
}

// ---- NHWC conv ---------------------------------------------------------------------------------
Tensor upsample_bilinear(const Tensor& x, int64_t Ho, int64_t Wo);
Tensor conv2d(const Tensor& x, const Tensor& w, int64_t ks, int64_t stride, int64_t pad, OptT bias, bool pre_relu,
              int64_t act, OptT res, OptT res2, at::OptionalIntArrayRef up, OptT bias9) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous(), "vda conv2d: x must be a contiguous NHWC [BT, H, W, Cin] map");
  need_contig(w, dt, "w", x);
  const int64_t BT = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3), Cout = w.size(0);
  TORCH_CHECK(w.dim() == 4 && w.size(1) == ks && w.size(2) == ks && w.size(3) == Cin, "vda conv2d: weight ",
              w.sizes(), " vs Cin=", Cin, " ks=", ks);
  int64_t uh = 0, uw = 0;
  if (up.has_value()) {
    TORCH_CHECK(up->size() == 2, "vda conv2d: up must be (Hu, Wu)");
    uh = (*up)[0];
    uw = (*up)[1];
  }
  const int64_t Hi = uh > 0 ? uh : H, Wi = uw > 0 ? uw : W;
  const int64_t Ho = (Hi + 2 * pad - ks) / stride + 1, Wo = (Wi + 2 * pad - ks) / stride + 1;
  Tensor out = at::empty({BT, Ho, Wo, Cout}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  optional<Tensor> r, r2;
  if (res) r = res->reshape({-1, Cout});
  int32_t r2h = 0, r2w = 0;
  if (res2) {
    Tensor s2 = *res2;
    if (s2.dim() == 4 && (s2.size(1) != Ho || s2.size(2) != Wo)) {
      // a lower-resolution skip input (the previous fusion block's output, blocks.py:156-158): read
      // through the bilinear upsample in the conv epilogue where the route has it, else materialised
      TORCH_CHECK(s2.size(0) == BT && s2.size(3) == Cout && s2.size(1) <= Ho && s2.size(2) <= Wo && s2.is_contiguous(),
                  "vda conv2d: a res2 of another grid must be a contiguous [BT, h <= Ho, w <= Wo, Cout] map, got ",
                  s2.sizes());
      if (dt != at::kFloat && uh == 0 && vda_conv2d_res2_upsample_ok(BT, H, W, Cin, Cout, ks, stride, pad)) {
        r2h = (int32_t)s2.size(1);
        r2w = (int32_t)s2.size(2);
      } else {
        s2 = upsample_bilinear(s2, Ho, Wo);
      }
    }
    r2 = s2.reshape({-1, Cout});
  }
  vda_epilogue e = make_epi(x, bias, c10::nullopt, 1, 1, c10::nullopt, r, r2, act, dt);
  e.res2_h = r2h;
  e.res2_w = r2w;
  if (bias9) {  // the 9-class table in place of bias (vda.h vda_epilogue.bias9)
    need_contig(*bias9, at::kFloat, "bias9", x);
    TORCH_CHECK(!bias && bias9->dim() == 2 && bias9->size(0) == 9 && bias9->size(1) == Cout,
                "vda conv2d: bias9 must be [9, Cout] and replaces bias");
    e.bias9 = (const float*)bias9->data_ptr();
  }
  int rc;
  if (dt == at::kFloat) {
    TORCH_CHECK(uh == 0, "vda conv2d: the fused-upsample loader is fp16-only");
    rc = vda_conv2d_f32((const float*)x.data_ptr(), (const float*)w.data_ptr(), (float*)out.data_ptr(), BT, H, W,
                        Cin, Cout, ks, stride, pad, pre_relu ? 1 : 0, &e, stream_of(x));
  } else {
    // split workspace of the strip-tiled conv (small maps): per call, from the caching allocator on
    // this stream, so concurrent convs on different streams never share it
    const int64_t wsb = uh > 0 ? 0 : vda_conv2d_workspace(BT, H, W, Cin, Cout, ks, stride, pad);
    Tensor ws;
    if (wsb > 0) ws = at::empty({wsb}, x.options().dtype(at::kByte));
    rc = vda_conv2d(x.data_ptr(), w.data_ptr(), out.data_ptr(), BT, H, W, Cin, Cout, ks, stride, pad,
                    pre_relu ? 1 : 0, uh, uw, &e, wsb > 0 ? ws.data_ptr() : nullptr, wsb, stream_of(x));
  }
  check_rc(rc, "vda_conv2d");
  return out;
}

// ---- norms -------------------------------------------------------------------------------------
Tensor layernorm(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps, int64_t skip_period,
                 optional<int64_t> rows) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "vda layernorm: x must be a 2-D row-major (possibly row-strided) matrix");
  const int64_t R = x.size(0), C = x.size(1);
  const int64_t nr = rows.has_value() ? *rows : (skip_period == 0 ? R : (R / (skip_period + 1)) * skip_period);
  Tensor out = at::empty({nr, C}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  need_contig(gamma, at::kFloat, "gamma", x);
  need_contig(beta, at::kFloat, "beta", x);
  const int rc = dt == at::kHalf
                     ? vda_layernorm(x.data_ptr(), x.stride(0), out.data_ptr(), (const float*)gamma.data_ptr(),
                                     (const float*)beta.data_ptr(), (int32_t)nr, (int32_t)C, (float)eps,
                                     (int32_t)skip_period, stream_of(x))
                     : vda_layernorm_f32((const float*)x.data_ptr(), x.stride(0), (float*)out.data_ptr(),
                                         (const float*)gamma.data_ptr(), (const float*)beta.data_ptr(), (int32_t)nr,
                                         (int32_t)C, (float)eps, (int32_t)skip_period, stream_of(x));
  check_rc(rc, "vda_layernorm");
  return out;
}

// [round_up(R, 2), 2] fp32 (mean, rstd) per row: the statistics half of a LayerNorm, for the LN-folded GEMM
Tensor row_stats(const Tensor& x, double eps) {
  TORCH_CHECK(x.scalar_type() == at::kHalf && x.dim() == 2 && x.stride(1) == 1,
              "vda row_stats: x must be a 2-D row-major fp16 matrix");
  const int64_t R = x.size(0), C = x.size(1);
  Tensor out = at::empty({(R + 1) / 2 * 2, 2}, x.options().dtype(at::kFloat));
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  check_rc(vda_row_stats(x.data_ptr(), x.stride(0), (float*)out.data_ptr(), (int32_t)R, (int32_t)C, (float)eps,
                         stream_of(x)),
           "vda_row_stats");
  return out;
}

Tensor groupnorm(const Tensor& x, const Tensor& gamma, const Tensor& beta, int64_t frames, int64_t groups, double eps) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "vda groupnorm: x must be a contiguous [F*S, C] matrix");
  TORCH_CHECK(frames > 0 && x.size(0) % frames == 0, "vda groupnorm: rows must be a multiple of frames");
  Tensor out = at::empty_like(x);
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  need_contig(gamma, at::kFloat, "gamma", x);
  need_contig(beta, at::kFloat, "beta", x);
  const int64_t C = x.size(1), S = x.size(0) / frames;
  int rc;
  if (dt == at::kFloat) {
    rc = vda_groupnorm_f32((const float*)x.data_ptr(), (float*)out.data_ptr(), (const float*)gamma.data_ptr(),
                           (const float*)beta.data_ptr(), frames, S, C, groups, (float)eps, stream_of(x));
  } else {
    const int64_t nws = vda_groupnorm_workspace(frames, S, C, groups);
    Tensor ws = at::empty({std::max<int64_t>(nws, 1)}, x.options().dtype(at::kFloat));
    rc = vda_groupnorm(x.data_ptr(), out.data_ptr(), (const float*)gamma.data_ptr(), (const float*)beta.data_ptr(),
                       frames, S, C, groups, (float)eps, (float*)ws.data_ptr(), stream_of(x));
  }
  check_rc(rc, "vda_groupnorm");
  return out;
}

// GroupNorm -> Linear (motion_module.py:116-119): fp16 through vda_groupnorm_linear (fused where
// vda_groupnorm_linear_fused says so), fp32 mode as vda_groupnorm_f32 + vda_gemm_f32.
Tensor groupnorm_linear(const Tensor& x, const Tensor& gamma, const Tensor& beta, int64_t frames, int64_t groups,
                        double eps, const Tensor& w, OptT bias, OptT stats_out) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "vda groupnorm_linear: x must be a contiguous [F*S, C] matrix");
  TORCH_CHECK(frames > 0 && x.size(0) % frames == 0, "vda groupnorm_linear: rows must be a multiple of frames");
  TORCH_CHECK(w.dim() == 2 && w.size(1) == x.size(1), "vda groupnorm_linear: w must be [N, C], got ", w.sizes());
  const int64_t M = x.size(0), C = x.size(1), N = w.size(0), S = M / frames;
  if (stats_out)
    TORCH_CHECK(dt == at::kHalf && stats_out->dim() == 3 && stats_out->size(0) >= M &&
                    stats_out->size(1) == (N + 255) / 256 && stats_out->size(2) == 2 &&
                    stats_out->scalar_type() == at::kFloat && stats_out->is_contiguous(),
                "vda groupnorm_linear: stats_out must be a contiguous float [M, ceil(N / 256), 2] (fp16 mode)");
  Tensor out = at::empty({M, N}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  need_contig(gamma, at::kFloat, "gamma", x);
  need_contig(beta, at::kFloat, "beta", x);
  need_contig(w, dt, "w", x);
  if (bias) need_contig(*bias, at::kFloat, "bias", x);
  if (stats_out) need_contig(*stats_out, at::kFloat, "stats_out", x);
  if (dt == at::kFloat) {
    Tensor xn = at::empty_like(x);
    check_rc(vda_groupnorm_f32((const float*)x.data_ptr(), (float*)xn.data_ptr(), (const float*)gamma.data_ptr(),
                               (const float*)beta.data_ptr(), frames, S, C, groups, (float)eps, stream_of(x)),
             "vda_groupnorm_f32");
    vda_epilogue e;
    std::memset(&e, 0, sizeof(e));
    e.bias = (const float*)ptr(bias);
    e.rdiv = e.rmod = 1;
    check_rc(vda_gemm_f32((const float*)xn.data_ptr(), C, (const float*)w.data_ptr(), (float*)out.data_ptr(), N,
                          (int32_t)M, (int32_t)N, (int32_t)C, &e, stream_of(x)),
             "vda_gemm_f32");
    return out;
  }
  const int64_t wsb = vda_groupnorm_linear_workspace(frames, S, C, groups, N);
  Tensor ws = at::empty({std::max<int64_t>(wsb, 16)}, x.options().dtype(at::kByte));
  check_rc(vda_groupnorm_linear(x.data_ptr(), (const float*)gamma.data_ptr(), (const float*)beta.data_ptr(), frames,
                                S, C, groups, (float)eps, w.data_ptr(), (const float*)ptr(bias), out.data_ptr(), N,
                                stats_out ? (float*)stats_out->data_ptr() : nullptr, ws.data_ptr(), wsb,
                                stream_of(x)),
           "vda_groupnorm_linear");
  return out;
}

// ---- attention ---------------------------------------------------------------------------------
Tensor spatial_attention(const Tensor& qkv, int64_t B, int64_t N, int64_t H, int64_t D) {
  const auto dt = act_dtype(qkv);
  TORCH_CHECK(qkv.is_contiguous() && qkv.dim() == 2 && qkv.size(0) == B * N && qkv.size(1) == 3 * H * D,
              "vda spatial_attention: qkv must be a contiguous [B*N, 3*H*D] matrix");
  Tensor out = at::empty({B * N, H * D}, qkv.options());
  if (qkv.is_meta()) return out;
  const at::OptionalDeviceGuard g(qkv.device());
  const float scale = 1.0f / std::sqrt((float)D);
  const int rc = dt == at::kHalf
                     ? vda_spatial_attention(qkv.data_ptr(), out.data_ptr(), B, N, H, D, scale, stream_of(qkv))
                     : vda_spatial_attention_f32((const float*)qkv.data_ptr(), (float*)out.data_ptr(), B, N, H, D,
                                                 scale, stream_of(qkv));
  check_rc(rc, "vda_spatial_attention");
  return out;
}

Tensor temporal_attention(const Tensor& qkv, int64_t B, int64_t T, int64_t S, int64_t H, int64_t D, double rope_theta) {
  const auto dt = act_dtype(qkv);
  TORCH_CHECK(qkv.is_contiguous() && qkv.dim() == 2 && qkv.size(0) == B * T * S && qkv.size(1) == 3 * H * D,
              "vda temporal_attention: qkv must be a contiguous [B*T*S, 3*H*D] matrix");
  Tensor out = at::empty({B * T * S, H * D}, qkv.options());
  if (qkv.is_meta()) return out;
  const at::OptionalDeviceGuard g(qkv.device());
  const float scale = 1.0f / std::sqrt((float)D);
  const int rc = dt == at::kHalf
                     ? vda_temporal_attention(qkv.data_ptr(), out.data_ptr(), B, T, S, H, D, scale, (float)rope_theta,
                                              stream_of(qkv))
                     : vda_temporal_attention_f32((const float*)qkv.data_ptr(), (float*)out.data_ptr(), B, T, S, H, D,
                                                  scale, (float)rope_theta, stream_of(qkv));
  check_rc(rc, "vda_temporal_attention");
  return out;
}

// ---- resampling / layout -----------------------------------------------------------------------
Tensor upsample_bilinear(const Tensor& x, int64_t Ho, int64_t Wo) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous(), "vda upsample_bilinear: x must be a contiguous NHWC map");
  const int64_t BT = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  Tensor out = at::empty({BT, Ho, Wo, C}, x.options());
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  const int rc = dt == at::kHalf
                     ? vda_upsample_bilinear(x.data_ptr(), out.data_ptr(), BT, H, W, C, Ho, Wo, stream_of(x))
                     : vda_upsample_bilinear_f32((const float*)x.data_ptr(), (float*)out.data_ptr(), BT, H, W, C, Ho,
                                                 Wo, stream_of(x));
  check_rc(rc, "vda_upsample_bilinear");
  return out;
}

Tensor patch_im2col(const Tensor& img, int64_t Kp, at::ScalarType dtype) {
  TORCH_CHECK(img.scalar_type() == at::kFloat && img.dim() == 4 && img.is_contiguous(),
              "vda patch_im2col: img must be a contiguous float [BT, 3, H, W] tensor");
  TORCH_CHECK(dtype == at::kHalf || dtype == at::kFloat, "vda patch_im2col: dtype must be float16 or float32");
  const int64_t BT = img.size(0), H = img.size(2), W = img.size(3);
  const int64_t np = (H / 14) * (W / 14);
  Tensor out = at::empty({BT * (1 + np), Kp}, img.options().dtype(dtype));
  if (img.is_meta()) return out;
  const at::OptionalDeviceGuard g(img.device());
  const int rc = dtype == at::kHalf
                     ? vda_patch_im2col((const float*)img.data_ptr(), out.data_ptr(), BT, H, W, Kp, stream_of(img))
                     : vda_patch_im2col_f32((const float*)img.data_ptr(), (float*)out.data_ptr(), BT, H, W, Kp,
                                            stream_of(img));
  check_rc(rc, "vda_patch_im2col");
  return out;
}

Tensor depth_head(const Tensor& x, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2, int64_t Ho,
                  int64_t Wo) {
  const auto dt = act_dtype(x);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous(), "vda depth_head: x must be a contiguous NHWC map");
  const int64_t BT = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  Tensor out = at::empty({BT, Ho, Wo}, x.options().dtype(at::kFloat));
  if (x.is_meta()) return out;
  const at::OptionalDeviceGuard g(x.device());
  need_contig(w1, dt, "w1", x);
  need_contig(b1, at::kFloat, "b1", x);
  need_contig(w2, at::kFloat, "w2", x);
  need_contig(b2, at::kFloat, "b2", x);
  int rc;
  if (dt == at::kHalf) {
    TORCH_CHECK(w1.dim() == 4 && w1.size(0) == 64 && w1.size(1) == 3 && w1.size(2) == 3 && w1.size(3) == C,
                "vda depth_head: w1 must be the [64, 3, 3, C] hi/lo split");
    // the resize is fused into the conv's patch staging for every shipped shape: the materialised
    // resize workspace is allocated only when the library asks for it
    const int64_t wsb = vda_depth_head_workspace(BT, H, W, C, Ho, Wo);
    Tensor ws;
    if (wsb > 0) ws = at::empty({wsb}, x.options().dtype(at::kByte));
    rc = vda_depth_head(x.data_ptr(), w1.data_ptr(), (const float*)b1.data_ptr(), (const float*)w2.data_ptr(),
                        (const float*)b2.data_ptr(), (float*)out.data_ptr(), wsb > 0 ? ws.data_ptr() : nullptr, BT, H,
                        W, C, Ho, Wo, stream_of(x));
  } else {
    TORCH_CHECK(w1.dim() == 4 && w1.size(0) == 32 && w1.size(3) == C, "vda depth_head: w1 must be [32, 3, 3, C]");
    Tensor up = at::empty({BT, Ho, Wo, C}, x.options());
    Tensor mid = at::empty({BT * Ho * Wo, 32}, x.options());
    rc = vda_depth_head_f32((const float*)x.data_ptr(), (const float*)w1.data_ptr(), (const float*)b1.data_ptr(),
                            (const float*)w2.data_ptr(), (const float*)b2.data_ptr(), (float*)out.data_ptr(),
                            (float*)up.data_ptr(), (float*)mid.data_ptr(), BT, H, W, C, Ho, Wo, stream_of(x));
  }
  check_rc(rc, "vda_depth_head");
  return out;
}

Tensor preprocess_frames(const Tensor& frames, int64_t H, int64_t W, at::ArrayRef<double> mean,
                         at::ArrayRef<double> std) {
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3,
              "vda preprocess_frames: frames must be uint8 [N, h, w, 3]");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "vda preprocess_frames: mean / std need 3 values");
  const Tensor fr = frames.contiguous();
  const int64_t N = fr.size(0), h = fr.size(1), w = fr.size(2);
  Tensor out = at::empty({N, 3, H, W}, fr.options().dtype(at::kFloat));
  if (fr.is_meta() || N == 0) return out;
  const at::OptionalDeviceGuard g(fr.device());
  const float m3[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  const float s3[3] = {(float)std[0], (float)std[1], (float)std[2]};
  check_rc(vda_preprocess_frames(fr.data_ptr(), (float*)out.data_ptr(), N, h, w, H, W, m3, s3, stream_of(fr)),
           "vda_preprocess_frames");
  return out;
}

Tensor depth_resize(const Tensor& depth, int64_t ho, int64_t wo) {
  TORCH_CHECK(depth.scalar_type() == at::kFloat && depth.dim() == 3 && depth.is_contiguous(),
              "vda depth_resize: depth must be a contiguous float [N, H, W] tensor");
  const int64_t N = depth.size(0), H = depth.size(1), W = depth.size(2);
  Tensor out = at::empty({N, ho, wo}, depth.options());
  if (depth.is_meta() || N == 0) return out;
  const at::OptionalDeviceGuard g(depth.device());
  check_rc(vda_depth_resize((const float*)depth.data_ptr(), (float*)out.data_ptr(), N, H, W, ho, wo,
                            stream_of(depth)),
           "vda_depth_resize");
  return out;
}

// ---- scale/shift alignment ---------------------------------------------------------------------
std::tuple<Tensor, Tensor> scale_shift(const Tensor& pred, const Tensor& target, OptT mask) {
  TORCH_CHECK(pred.scalar_type() == at::kFloat && pred.is_contiguous() && pred.numel() >= 1,
              "vda scale_shift: pred must be a contiguous, non-empty float tensor");
  need_contig(target, at::kFloat, "target", pred);
  TORCH_CHECK(target.numel() == pred.numel(), "vda scale_shift: pred and target must have the same number of elements");
  if (mask) {
    need_contig(*mask, at::kByte, "mask", pred);
    TORCH_CHECK(mask->numel() == pred.numel(), "vda scale_shift: mask must have pred's number of elements");
  }
  Tensor ss = at::empty({2}, pred.options());
  Tensor sums = at::empty({5}, pred.options().dtype(at::kDouble));
  if (pred.is_meta()) return {ss, sums};
  const at::OptionalDeviceGuard g(pred.device());
  const int64_t n = pred.numel();
  const int64_t wsb = vda_scale_shift_workspace(n);
  Tensor ws = at::empty({wsb}, pred.options().dtype(at::kByte));
  check_rc(vda_scale_shift((const float*)pred.data_ptr(), (const float*)target.data_ptr(), (const uint8_t*)ptr(mask), n,
                           (double*)sums.data_ptr(), (float*)ss.data_ptr(), ws.data_ptr(), wsb, stream_of(pred)),
           "vda_scale_shift");
  return {ss, sums};
}

Tensor depth_align(const Tensor& src, int64_t ho, int64_t wo, OptT ss, bool clip, OptT pre,
                   optional<at::ArrayRef<double>> w_pre, optional<at::ArrayRef<double>> w_post, OptT out_) {
  TORCH_CHECK(src.scalar_type() == at::kFloat && src.dim() == 3 && src.is_contiguous(),
              "vda depth_align: src must be a contiguous float [F, H, W] tensor");
  const int64_t F = src.size(0), H = src.size(1), W = src.size(2);
  TORCH_CHECK(F >= 1 && F <= 32, "vda depth_align: 1 <= F <= 32 frames per call, got ", F);
  TORCH_CHECK(ho >= 1 && wo >= 1, "vda depth_align: empty output size");
  if (ss) {
    need_contig(*ss, at::kFloat, "ss", src);
    TORCH_CHECK(ss->numel() == 2, "vda depth_align: ss must hold (scale, shift)");
  }
  float wp[32], wq[32];
  if (pre) {
    need_contig(*pre, at::kFloat, "pre", src);
    TORCH_CHECK(pre->dim() == 3 && pre->size(0) == F && pre->size(1) == ho && pre->size(2) == wo,
                "vda depth_align: pre must be [F, ho, wo]");
    TORCH_CHECK(w_pre.has_value() && w_post.has_value() && (int64_t)w_pre->size() == F && (int64_t)w_post->size() == F,
                "vda depth_align: a blend needs F weights in w_pre and in w_post");
    for (int64_t f = 0; f < F; ++f) {
      wp[f] = (float)(*w_pre)[f];
      wq[f] = (float)(*w_post)[f];
    }
  }
  Tensor out;
  if (out_) {
    need_contig(*out_, at::kFloat, "out", src);
    TORCH_CHECK(out_->dim() == 3 && out_->size(0) == F && out_->size(1) == ho && out_->size(2) == wo,
                "vda depth_align: out must be [F, ho, wo]");
    out = *out_;
  } else {
    out = at::empty({F, ho, wo}, src.options());
  }
  if (src.is_meta()) return out;
  const at::OptionalDeviceGuard g(src.device());
  check_rc(vda_depth_align((const float*)src.data_ptr(), F, H, W, ho, wo, (const float*)ptr(ss), clip ? 1 : 0,
                           (const float*)ptr(pre), pre ? wp : nullptr, pre ? wq : nullptr, (float*)out.data_ptr(),
                           stream_of(src)),
           "vda_depth_align");
  return out;
}

// ---- ground-truth evaluation -------------------------------------------------------------------
// pred / gt [F, ...] float and valid [F, ...] uint8 with the same number of elements per frame.
int64_t eval_inputs(const char* op, const Tensor& pred, const Tensor& gt, OptT valid) {
  TORCH_CHECK(pred.scalar_type() == at::kFloat && pred.is_contiguous() && pred.dim() >= 1 && pred.numel() >= 1,
              "vda ", op, ": pred must be a contiguous, non-empty float [F, ...] tensor");
  TORCH_CHECK(pred.size(0) <= 65535, "vda ", op, ": F <= 65535 frames per call, got ", pred.size(0));
  need_contig(gt, at::kFloat, "gt", pred);
  TORCH_CHECK(gt.sizes() == pred.sizes(), "vda ", op, ": gt must have pred's shape");
  if (valid) {
    need_contig(*valid, at::kByte, "valid", pred);
    TORCH_CHECK(valid->sizes() == pred.sizes(), "vda ", op, ": valid must have pred's shape");
  }
  return pred.numel() / pred.size(0);
}

std::tuple<Tensor, Tensor> depth_eval_fit(const Tensor& pred, const Tensor& gt, OptT valid, bool per_frame) {
  const int64_t S = eval_inputs("depth_eval_fit", pred, gt, valid);
  const int64_t F = pred.size(0), G = per_frame ? F : 1;
  Tensor ss = at::empty({G, 2}, pred.options());
  Tensor sums = at::empty({G, 5}, pred.options().dtype(at::kDouble));
  if (pred.is_meta()) return {ss, sums};
  const at::OptionalDeviceGuard g(pred.device());
  const int64_t wsb = vda_depth_eval_workspace((int32_t)F, S);
  Tensor ws = at::empty({wsb}, pred.options().dtype(at::kByte));
  check_rc(vda_depth_eval_fit((const float*)pred.data_ptr(), (const float*)gt.data_ptr(), (const uint8_t*)ptr(valid),
                              (int32_t)F, S, per_frame ? 1 : 0, (double*)sums.data_ptr(), (float*)ss.data_ptr(),
                              ws.data_ptr(), wsb, stream_of(pred)),
           "vda_depth_eval_fit");
  return {ss, sums};
}

std::tuple<Tensor, Tensor, optional<Tensor>> depth_eval_metrics(const Tensor& pred, const Tensor& gt, OptT valid,
                                                                const Tensor& ss, double max_depth,
                                                                bool want_aligned) {
  const int64_t S = eval_inputs("depth_eval_metrics", pred, gt, valid);
  const int64_t F = pred.size(0);
  need_contig(ss, at::kFloat, "ss", pred);
  TORCH_CHECK(ss.numel() == 2 || (ss.numel() == 2 * F && ss.dim() == 2),
              "vda depth_eval_metrics: ss must hold (scale, shift) once ([2] or [1, 2]) or per frame ([F, 2])");
  TORCH_CHECK(max_depth > 0., "vda depth_eval_metrics: max_depth must be greater than 0");
  const bool ss_per_frame = ss.dim() == 2 && ss.size(0) == F && F > 1;
  Tensor frame_sums = at::empty({F, 8}, pred.options().dtype(at::kDouble));
  Tensor total = at::empty({8}, pred.options().dtype(at::kDouble));
  optional<Tensor> aligned;
  if (want_aligned) aligned = at::empty(pred.sizes(), pred.options());
  if (pred.is_meta()) return {frame_sums, total, aligned};
  const at::OptionalDeviceGuard g(pred.device());
  const int64_t wsb = vda_depth_eval_workspace((int32_t)F, S);
  Tensor ws = at::empty({wsb}, pred.options().dtype(at::kByte));
  check_rc(vda_depth_eval_metrics((const float*)pred.data_ptr(), (const float*)gt.data_ptr(),
                                  (const uint8_t*)ptr(valid), (int32_t)F, S, (const float*)ss.data_ptr(),
                                  ss_per_frame ? 1 : 0, (float)max_depth, aligned ? (float*)aligned->data_ptr() : nullptr,
                                  (double*)frame_sums.data_ptr(), (double*)total.data_ptr(), ws.data_ptr(), wsb,
                                  stream_of(pred)),
           "vda_depth_eval_metrics");
  return {frame_sums, total, aligned};
}

// ---- depth visualisation -----------------------------------------------------------------------
Tensor depth_range(const Tensor& depth) {
  TORCH_CHECK(depth.scalar_type() == at::kFloat && depth.is_contiguous() && depth.numel() >= 1,
              "vda depth_range: depth must be a contiguous, non-empty float tensor");
  Tensor range = at::empty({2}, depth.options());
  if (depth.is_meta()) return range;
  const at::OptionalDeviceGuard g(depth.device());
  const int64_t n = depth.numel();
  const int64_t wsb = vda_depth_range_workspace(n);
  Tensor ws = at::empty({wsb}, depth.options().dtype(at::kByte));
  check_rc(vda_depth_range((const float*)depth.data_ptr(), n, (float*)range.data_ptr(), ws.data_ptr(), wsb,
                           stream_of(depth)),
           "vda_depth_range");
  return range;
}

Tensor depth_colorize(const Tensor& depth, const Tensor& range, OptT lut, int64_t layout) {
  TORCH_CHECK(depth.scalar_type() == at::kFloat && depth.dim() == 3 && depth.is_contiguous() && depth.numel() >= 1,
              "vda depth_colorize: depth must be a contiguous, non-empty float [F, H, W] tensor");
  const int64_t F = depth.size(0), H = depth.size(1), W = depth.size(2);
  TORCH_CHECK(F <= 65535, "vda depth_colorize: F <= 65535 frames per call, got ", F);
  TORCH_CHECK(H <= INT32_MAX && W <= INT32_MAX, "vda depth_colorize: H and W must fit 32 bits");
  need_contig(range, at::kFloat, "range", depth);
  TORCH_CHECK(range.numel() == 2, "vda depth_colorize: range must hold (min, max)");
  TORCH_CHECK(layout >= VDA_VIS_INDEX && layout <= VDA_VIS_PLANAR420, "vda depth_colorize: unknown layout ", layout);
  TORCH_CHECK(lut.has_value() || layout == VDA_VIS_INDEX, "vda depth_colorize: this layout needs a lut");
  if (lut) {
    need_contig(*lut, at::kByte, "lut", depth);
    TORCH_CHECK(lut->dim() == 2 && lut->size(0) == 256 && lut->size(1) == 3, "vda depth_colorize: lut must be [256, 3]");
  }
  const int64_t ch = (H + 1) / 2, cw = (W + 1) / 2;
  Tensor out;
  const auto opt = depth.options().dtype(at::kByte);
  switch (layout) {
    case VDA_VIS_INDEX: out = at::empty({F, H, W}, opt); break;
    case VDA_VIS_HWC: out = at::empty({F, H, W, 3}, opt); break;
    case VDA_VIS_PLANAR444: out = at::empty({F, 3, H, W}, opt); break;
    default: out = at::empty({F, H * W + 2 * ch * cw}, opt); break;
  }
  if (depth.is_meta()) return out;
  const at::OptionalDeviceGuard g(depth.device());
  TORCH_CHECK(out.numel() == vda_depth_colorize_bytes((int32_t)F, (int32_t)H, (int32_t)W, (int32_t)layout),
              "vda depth_colorize: output size disagrees with vda_depth_colorize_bytes");
  check_rc(vda_depth_colorize((const float*)depth.data_ptr(), (int32_t)F, (int32_t)H, (int32_t)W,
                              (const float*)range.data_ptr(), (const uint8_t*)ptr(lut), (int32_t)layout,
                              (uint8_t*)out.data_ptr(), stream_of(depth)),
           "vda_depth_colorize");
  return out;
}

// ---- point clouds ----------------------------------------------------------------------------------
// depth [F, H, W] float, valid [F, H, W] uint8 and rgb [F, H, W, 3] uint8 on depth's device.
void cloud_inputs(const char* op, const Tensor& depth, OptT valid, int64_t step) {
  TORCH_CHECK(depth.scalar_type() == at::kFloat && depth.dim() == 3 && depth.is_contiguous() && depth.numel() >= 1,
              "vda ", op, ": depth must be a contiguous, non-empty float [F, H, W] tensor");
  TORCH_CHECK(depth.size(0) <= 65535, "vda ", op, ": F <= 65535 frames per call, got ", depth.size(0));
  TORCH_CHECK(depth.size(1) <= INT32_MAX && depth.size(2) <= INT32_MAX, "vda ", op, ": H and W must fit 32 bits");
  TORCH_CHECK(step >= 1 && step <= INT32_MAX, "vda ", op, ": step must be at least 1, got ", step);
  if (valid) {
    need_contig(*valid, at::kByte, "valid", depth);
    TORCH_CHECK(valid->sizes() == depth.sizes(), "vda ", op, ": valid must have depth's shape");
  }
}

// -> (frame_offsets [F + 1] int64, ws): ws carries the block offsets to cloud_write.
std::tuple<Tensor, Tensor> cloud_count(const Tensor& depth, OptT valid, int64_t step, double trunc) {
  cloud_inputs("cloud_count", depth, valid, step);
  const int64_t F = depth.size(0), H = depth.size(1), W = depth.size(2);
  const int64_t wsb = vda_cloud_workspace((int32_t)F, (int32_t)H, (int32_t)W, (int32_t)step);
  Tensor offs = at::empty({F + 1}, depth.options().dtype(at::kLong));
  Tensor ws = at::empty({wsb}, depth.options().dtype(at::kByte));
  if (depth.is_meta()) return {offs, ws};
  const at::OptionalDeviceGuard g(depth.device());
  check_rc(vda_cloud_count((const float*)depth.data_ptr(), (const uint8_t*)ptr(valid), (int32_t)F, (int32_t)H,
                           (int32_t)W, (int32_t)step, (float)trunc, (int64_t*)offs.data_ptr(), ws.data_ptr(), wsb,
                           stream_of(depth)),
           "vda_cloud_count");
  return {offs, ws};
}

// n: the number of points (frame_offsets[F] of cloud_count, read by the caller), which sizes the output.
// VDA_CLOUD_SPLIT -> (points [n, 3] float, colors [n, 3] uint8 or None); VDA_CLOUD_PACKED -> (the n records as
// [n * 12] or [n * 15] uint8, None).
std::tuple<Tensor, optional<Tensor>> cloud_write(const Tensor& depth, OptT valid, OptT rgb, const Tensor& K, OptT M,
                                                 int64_t step, double trunc, int64_t layout, const Tensor& ws,
                                                 int64_t n) {
  cloud_inputs("cloud_write", depth, valid, step);
  const int64_t F = depth.size(0), H = depth.size(1), W = depth.size(2);
  if (rgb) {
    need_contig(*rgb, at::kByte, "rgb", depth);
    TORCH_CHECK(rgb->dim() == 4 && rgb->size(0) == F && rgb->size(1) == H && rgb->size(2) == W && rgb->size(3) == 3,
                "vda cloud_write: rgb must be [F, H, W, 3]");
  }
  need_contig(K, at::kFloat, "K", depth);
  TORCH_CHECK(K.dim() == 2 && K.size(0) == F && K.size(1) == 4, "vda cloud_write: K must be [F, 4] = (fx, fy, cx, cy)");
  if (M) {
    need_contig(*M, at::kFloat, "M", depth);
    TORCH_CHECK(M->dim() == 3 && M->size(0) == F && M->size(1) == 3 && M->size(2) == 4,
                "vda cloud_write: M must be [F, 3, 4]");
  }
  TORCH_CHECK(layout == VDA_CLOUD_SPLIT || layout == VDA_CLOUD_PACKED, "vda cloud_write: unknown layout ", layout);
  TORCH_CHECK(n >= 0, "vda cloud_write: n must not be negative, got ", n);
  need_contig(ws, at::kByte, "ws", depth);
  const int64_t wsb = vda_cloud_workspace((int32_t)F, (int32_t)H, (int32_t)W, (int32_t)step);
  TORCH_CHECK(ws.numel() == wsb, "vda cloud_write: ws must be the workspace cloud_count returned for this shape");
  Tensor out;
  optional<Tensor> colors;
  if (layout == VDA_CLOUD_PACKED) {
    out = at::empty({n * (rgb ? 15 : 12)}, depth.options().dtype(at::kByte));
  } else {
    out = at::empty({n, 3}, depth.options());
    if (rgb) colors = at::empty({n, 3}, depth.options().dtype(at::kByte));
  }
  if (depth.is_meta() || n == 0) return {out, colors};
  const at::OptionalDeviceGuard g(depth.device());
  check_rc(vda_cloud_write((const float*)depth.data_ptr(), (const uint8_t*)ptr(valid), (const uint8_t*)ptr(rgb),
                           (int32_t)F, (int32_t)H, (int32_t)W, (int32_t)step, (float)trunc, (const float*)K.data_ptr(),
                           (const float*)ptr(M), (int32_t)layout, out.data_ptr(),
                           colors ? (uint8_t*)colors->data_ptr() : nullptr, n, ws.data_ptr(), wsb, stream_of(depth)),
           "vda_cloud_write");
  return {out, colors};
}

// ---- ground-truth comparison video ---------------------------------------------------------------
Tensor depth_absdiff_range(const Tensor& a, const Tensor& b, OptT valid) {
  TORCH_CHECK(a.scalar_type() == at::kFloat && a.is_contiguous() && a.numel() >= 1,
              "vda depth_absdiff_range: a must be a contiguous, non-empty float tensor");
  need_contig(b, at::kFloat, "b", a);
  TORCH_CHECK(b.numel() == a.numel(), "vda depth_absdiff_range: b must have a's number of elements");
  if (valid) {
    need_contig(*valid, at::kByte, "valid", a);
    TORCH_CHECK(valid->numel() == a.numel(), "vda depth_absdiff_range: valid must have a's number of elements");
  }
  Tensor range = at::empty({2}, a.options());
  if (a.is_meta()) return range;
  const at::OptionalDeviceGuard g(a.device());
  const int64_t n = a.numel();
  const int64_t wsb = vda_depth_absdiff_range_workspace(n);
  Tensor ws = at::empty({wsb}, a.options().dtype(at::kByte));
  check_rc(vda_depth_absdiff_range((const float*)a.data_ptr(), (const float*)b.data_ptr(), (const uint8_t*)ptr(valid), n,
                                   (float*)range.data_ptr(), ws.data_ptr(), wsb, stream_of(a)),
           "vda_depth_absdiff_range");
  return range;
}

// Tile i: kind[i] in cell (row[i], col[i]) with frame offset offset[i] and table lut[i]; a[i] its source
// ([n, H, W, 3] uint8 for VDA_TILE_RGB, [n, H, W] float otherwise), b[i] / valid[i] the second operand and the
// mask of an error tile, range[i] the [2] range of every tile but RGB.
Tensor panel_compose(at::TensorList a, const c10::List<optional<Tensor>>& b, const c10::List<optional<Tensor>>& valid,
                     const c10::List<optional<Tensor>>& range, at::IntArrayRef kind, at::IntArrayRef row,
                     at::IntArrayRef col, at::IntArrayRef offset, at::IntArrayRef lut, int64_t rows, int64_t cols,
                     int64_t H, int64_t W, int64_t F, int64_t t0, int64_t N, int64_t xstar, OptT lut0, OptT lut1,
                     int64_t layout) {
  const size_t n = a.size();
  TORCH_CHECK(n >= 1 && n <= 12, "vda panel_compose: 1 to 12 tiles, got ", n);
  TORCH_CHECK(b.size() == n && valid.size() == n && range.size() == n && kind.size() == n && row.size() == n &&
                  col.size() == n && offset.size() == n && lut.size() == n,
              "vda panel_compose: every per-tile list needs one entry per tile");
  TORCH_CHECK(rows >= 1 && rows <= 4 && cols >= 1 && cols <= 3, "vda panel_compose: a grid of 1..4 rows by 1..3 columns");
  TORCH_CHECK(H >= 1 && W >= 1 && rows * H * cols * W < (int64_t(1) << 31),
              "vda panel_compose: the canvas must hold 1 to 2^31 - 1 pixels");
  TORCH_CHECK(F >= 1 && F <= 65535, "vda panel_compose: 1 <= F <= 65535 frames per call, got ", F);
  TORCH_CHECK(N >= 1 && N <= INT32_MAX && t0 >= 0 && t0 + F <= N, "vda panel_compose: 0 <= t0 and t0 + F <= N");
  TORCH_CHECK(xstar >= 0 && xstar < W, "vda panel_compose: 0 <= xstar < W");
  TORCH_CHECK(layout >= VDA_VIS_HWC && layout <= VDA_VIS_PLANAR420, "vda panel_compose: unknown layout ", layout);
  const Tensor& like = a[0];
  vda_tile tiles[12];
  for (size_t i = 0; i < n; ++i) {
    const Tensor& s = a[i];
    const bool rgb = kind[i] == VDA_TILE_RGB;
    TORCH_CHECK(kind[i] >= VDA_TILE_RGB && kind[i] <= VDA_TILE_XT, "vda panel_compose: unknown tile kind ", kind[i]);
    need_contig(s, rgb ? at::kByte : at::kFloat, "a tile source", like);
    TORCH_CHECK(s.dim() == (rgb ? 4 : 3) && s.size(0) >= 1 && s.size(0) <= INT32_MAX && s.size(1) == H &&
                    s.size(2) == W && (!rgb || s.size(3) == 3),
                "vda panel_compose: a tile source must be [n, H, W] float ([n, H, W, 3] uint8 for RGB), got ", s.sizes());
    TORCH_CHECK(offset[i] >= 0 && offset[i] <= INT32_MAX, "vda panel_compose: a frame offset must be >= 0");
    vda_tile& t = tiles[i];
    t = vda_tile{};
    t.kind = (int32_t)kind[i], t.row = (int32_t)row[i], t.col = (int32_t)col[i];
    t.offset = (int32_t)offset[i], t.frames = (int32_t)s.size(0), t.lut = (int32_t)lut[i];
    t.a = s.is_meta() ? nullptr : s.data_ptr();
    const optional<Tensor> bi = b.get(i), vi = valid.get(i), ri = range.get(i);
    if (kind[i] == VDA_TILE_ERROR) {
      TORCH_CHECK(bi.has_value(), "vda panel_compose: an error tile needs its second operand");
      need_contig(*bi, at::kFloat, "b", like);
      TORCH_CHECK(bi->sizes() == s.sizes(), "vda panel_compose: b must have a's shape");
      if (vi) {
        need_contig(*vi, at::kByte, "valid", like);
        TORCH_CHECK(vi->sizes() == s.sizes(), "vda panel_compose: valid must have a's shape");
      }
      if (!s.is_meta()) {
        t.b = (const float*)bi->data_ptr();
        t.valid = vi ? (const uint8_t*)vi->data_ptr() : nullptr;
      }
    }
    if (!rgb) {
      TORCH_CHECK(ri.has_value(), "vda panel_compose: every tile but RGB needs a range");
      need_contig(*ri, at::kFloat, "range", like);
      TORCH_CHECK(ri->numel() == 2, "vda panel_compose: a range must hold (min, max)");
      TORCH_CHECK(lut[i] == 0 ? lut0.has_value() : (lut[i] == 1 && lut1.has_value()),
                  "vda panel_compose: a tile names a lut that is missing");
      if (!s.is_meta()) t.range = (const float*)ri->data_ptr();
    }
  }
  for (const optional<Tensor>* l : {&lut0, &lut1}) {
    if (!l->has_value()) continue;
    need_contig(**l, at::kByte, "lut", like);
    TORCH_CHECK((*l)->dim() == 2 && (*l)->size(0) == 256 && (*l)->size(1) == 3,
                "vda panel_compose: a lut must be [256, 3]");
  }
  const int64_t CH = rows * H, CW = cols * W;
  const auto opt = like.options().dtype(at::kByte);
  Tensor out;
  switch (layout) {
    case VDA_VIS_HWC: out = at::empty({F, CH, CW, 3}, opt); break;
    case VDA_VIS_PLANAR444: out = at::empty({F, 3, CH, CW}, opt); break;
    default: out = at::empty({F, CH * CW + 2 * ((CH + 1) / 2) * ((CW + 1) / 2)}, opt); break;
  }
  if (like.is_meta()) return out;
  const at::OptionalDeviceGuard g(like.device());
  TORCH_CHECK(out.numel() == vda_panel_compose_bytes((int32_t)F, (int32_t)rows, (int32_t)cols, (int32_t)H, (int32_t)W,
                                                     (int32_t)layout),
              "vda panel_compose: output size disagrees with vda_panel_compose_bytes");
  check_rc(vda_panel_compose(tiles, (int32_t)n, (int32_t)rows, (int32_t)cols, (int32_t)F, (int32_t)t0, (int32_t)N,
                             (int32_t)H, (int32_t)W, (int32_t)xstar, (const uint8_t*)ptr(lut0),
                             (const uint8_t*)ptr(lut1), (int32_t)layout, (uint8_t*)out.data_ptr(), stream_of(like)),
           "vda_panel_compose");
  return out;
}

// ---- planar YUV frames -------------------------------------------------------------------------
// payload [N, frame_stride] uint8 with unit stride along a frame (any base address): the frames' planar bytes.
int64_t yuv_frame_stride(const Tensor& payload, int64_t h, int64_t w, int64_t chroma, const char* what) {
  TORCH_CHECK(payload.scalar_type() == at::kByte && payload.dim() == 2, what, ": payload must be uint8 [N, frame_stride]");
  TORCH_CHECK(payload.size(1) <= 1 || payload.stride(1) == 1, what, ": payload rows must have unit stride");
  TORCH_CHECK(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, what, ": h and w must be positive and fit 32 bits");
  TORCH_CHECK(chroma >= VDA_YUV_420 && chroma <= VDA_YUV_MONO, what, ": unknown chroma code ", chroma);
  const int64_t sx = (chroma == VDA_YUV_420 || chroma == VDA_YUV_422) ? 1 : 0, sy = chroma == VDA_YUV_420 ? 1 : 0;
  const int64_t fsz = h * w + (chroma == VDA_YUV_MONO ? 0 : 2 * ((w + sx) >> sx) * ((h + sy) >> sy));
  TORCH_CHECK(payload.size(1) >= fsz, what, ": a frame holds ", payload.size(1), " bytes, its payload needs ", fsz);
  const int64_t stride = payload.size(0) > 1 ? payload.stride(0) : payload.size(1);
  TORCH_CHECK(stride >= payload.size(1), what, ": payload frames overlap");
  return stride;
}

Tensor yuv_to_rgb(const Tensor& payload, int64_t h, int64_t w, int64_t chroma) {
  const int64_t stride = yuv_frame_stride(payload, h, w, chroma, "vda yuv_to_rgb");
  const int64_t N = payload.size(0);
  TORCH_CHECK(N <= 65535 && h <= 65535, "vda yuv_to_rgb: N and h <= 65535 per call");
  Tensor out = at::empty({N, h, w, 3}, payload.options());
  if (payload.is_meta() || N == 0) return out;
  const at::OptionalDeviceGuard g(payload.device());
  check_rc(vda_yuv_to_rgb((const uint8_t*)payload.data_ptr(), (int32_t)N, (int32_t)h, (int32_t)w, stride,
                          (int32_t)chroma, (uint8_t*)out.data_ptr(), stream_of(payload)),
           "vda_yuv_to_rgb");
  return out;
}

Tensor preprocess_yuv(const Tensor& payload, int64_t h, int64_t w, int64_t chroma, int64_t H, int64_t W,
                      at::ArrayRef<double> mean, at::ArrayRef<double> std) {
  const int64_t stride = yuv_frame_stride(payload, h, w, chroma, "vda preprocess_yuv");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "vda preprocess_yuv: mean / std need 3 values");
  TORCH_CHECK(H >= 1 && W >= 1 && H <= INT32_MAX && W <= INT32_MAX, "vda preprocess_yuv: H and W must be positive");
  const int64_t N = payload.size(0);
  TORCH_CHECK(N <= 65535, "vda preprocess_yuv: N <= 65535 frames per call");
  Tensor out = at::empty({N, 3, H, W}, payload.options().dtype(at::kFloat));
  if (payload.is_meta() || N == 0) return out;
  const at::OptionalDeviceGuard g(payload.device());
  const float m3[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  const float s3[3] = {(float)std[0], (float)std[1], (float)std[2]};
  const int64_t wsb = vda_preprocess_yuv_workspace((int32_t)N, (int32_t)h, (int32_t)w, (int32_t)H, (int32_t)W);
  Tensor ws;
  if (wsb > 0) ws = at::empty({wsb}, payload.options());
  check_rc(vda_preprocess_yuv((const uint8_t*)payload.data_ptr(), (int32_t)N, (int32_t)h, (int32_t)w, stride,
                              (int32_t)chroma, (float*)out.data_ptr(), (int32_t)H, (int32_t)W, m3, s3,
                              wsb > 0 ? ws.data_ptr() : nullptr, wsb, stream_of(payload)),
           "vda_preprocess_yuv");
  return out;
}

// The resampling tables of one axis (vda_resample_tables): k int32 [out, vda_resample_taps(in, out)], b int32 [out, 2].
void need_tables(const Tensor& k, const Tensor& b, int64_t in, int64_t out, const char* axis, const Tensor& like) {
  need_contig(k, at::kInt, axis, like);
  need_contig(b, at::kInt, axis, like);
  const int64_t taps = vda_resample_taps((int32_t)in, (int32_t)out);
  TORCH_CHECK(k.dim() == 2 && k.size(0) == out && k.size(1) == taps, "vda yuv_downscale: the ", axis,
              " coefficients must be [", out, ", ", taps, "] for ", in, " -> ", out, ", got ", k.sizes());
  TORCH_CHECK(b.dim() == 2 && b.size(0) == out && b.size(1) == 2, "vda yuv_downscale: the ", axis,
              " bounds must be [", out, ", 2], got ", b.sizes());
}

Tensor yuv_downscale(const Tensor& payload, int64_t h, int64_t w, int64_t chroma, int64_t h2, int64_t w2,
                     const Tensor& kx, const Tensor& bx, const Tensor& ky, const Tensor& by) {
  const int64_t stride = yuv_frame_stride(payload, h, w, chroma, "vda yuv_downscale");
  TORCH_CHECK(h2 >= 1 && w2 >= 1 && w2 <= INT32_MAX, "vda yuv_downscale: h2 and w2 must be positive");
  const int64_t N = payload.size(0);
  TORCH_CHECK(N <= 65535 && h2 <= 65535, "vda yuv_downscale: N and h2 <= 65535 per call");
  need_tables(kx, bx, w, w2, "horizontal", payload);
  need_tables(ky, by, h, h2, "vertical", payload);
  TORCH_CHECK(vda_yuv_downscale_ok((int32_t)h, (int32_t)w, (int32_t)h2, (int32_t)w2) == 1, "vda yuv_downscale: ", h, "x", w,
              " -> ", h2, "x", w2, " is beyond the kernel's ratio (vda_yuv_downscale_ok)");
  Tensor out = at::empty({N, h2, w2, 3}, payload.options());
  if (payload.is_meta() || N == 0) return out;
  const at::OptionalDeviceGuard g(payload.device());
  const int64_t wsb = vda_yuv_downscale_workspace((int32_t)N, (int32_t)h, (int32_t)w, (int32_t)h2, (int32_t)w2);
  Tensor ws;
  if (wsb > 0) ws = at::empty({wsb}, payload.options());
  check_rc(vda_yuv_downscale((const uint8_t*)payload.data_ptr(), (int32_t)N, (int32_t)h, (int32_t)w, stride,
                             (int32_t)chroma, (const int32_t*)kx.data_ptr(), (const int32_t*)bx.data_ptr(),
                             (const int32_t*)ky.data_ptr(), (const int32_t*)by.data_ptr(), (uint8_t*)out.data_ptr(),
                             (int32_t)h2, (int32_t)w2, wsb > 0 ? ws.data_ptr() : nullptr, wsb, stream_of(payload)),
           "vda_yuv_downscale");
  return out;
}

}  // namespace

TORCH_LIBRARY(vda, m) {
  m.def("yuv_to_rgb(Tensor payload, int h, int w, int chroma) -> Tensor");
  m.def("yuv_downscale(Tensor payload, int h, int w, int chroma, int h2, int w2, Tensor kx, Tensor bx, Tensor ky, "
        "Tensor by) -> Tensor");
  m.def("preprocess_yuv(Tensor payload, int h, int w, int chroma, int H, int W, float[] mean, float[] std) -> Tensor");
  m.def("depth_range(Tensor depth) -> Tensor");
  m.def("depth_colorize(Tensor depth, Tensor range, Tensor? lut, int layout) -> Tensor");
  m.def("depth_absdiff_range(Tensor a, Tensor b, Tensor? valid=None) -> Tensor");
  m.def("panel_compose(Tensor[] a, Tensor?[] b, Tensor?[] valid, Tensor?[] range, int[] kind, int[] row, int[] col, "
        "int[] offset, int[] lut, int rows, int cols, int H, int W, int F, int t0, int N, int xstar, Tensor? lut0, "
        "Tensor? lut1, int layout) -> Tensor");
  m.def("gemm(Tensor x, Tensor w, Tensor? bias=None, Tensor? rowbias=None, int rdiv=1, int rmod=1, "
        "Tensor? gamma=None, Tensor? res=None, Tensor? res2=None, int act=0, Tensor? ln_stats=None, "
        "Tensor? ln_colsum=None, int ln_parts=0, float ln_eps=1e-6, Tensor(b!)? stats_out=None, "
        "Tensor(c!)? sched=None, int drop_period=0) -> Tensor");
  m.def("gemm.out(Tensor x, Tensor w, Tensor? bias=None, Tensor? rowbias=None, int rdiv=1, int rmod=1, "
        "Tensor? gamma=None, Tensor? res=None, Tensor? res2=None, int act=0, Tensor? ln_stats=None, "
        "Tensor? ln_colsum=None, int ln_parts=0, float ln_eps=1e-6, Tensor(b!)? stats_out=None, "
        "Tensor(c!)? sched=None, int drop_period=0, *, Tensor(a!) out) -> Tensor(a!)");
  m.def("row_stats(Tensor x, float eps) -> Tensor");
  m.def("conv_transpose_ks(Tensor x, Tensor w, Tensor bias, int BT, int h, int w_, int k) -> Tensor");
  m.def("subpixel_conv(Tensor x, Tensor w, Tensor bias9, int BT, int h, int w_, int s) -> Tensor");
  m.def("conv2d(Tensor x, Tensor w, int ks=3, int stride=1, int pad=1, Tensor? bias=None, bool pre_relu=False, "
        "int act=0, Tensor? res=None, Tensor? res2=None, int[]? up=None, Tensor? bias9=None) -> Tensor");
  m.def("layernorm(Tensor x, Tensor gamma, Tensor beta, float eps, int skip_period=0, int? rows=None) -> Tensor");
  m.def("groupnorm(Tensor x, Tensor gamma, Tensor beta, int frames, int groups, float eps) -> Tensor");
  m.def("groupnorm_linear(Tensor x, Tensor gamma, Tensor beta, int frames, int groups, float eps, Tensor w, "
        "Tensor? bias=None, Tensor(b!)? stats_out=None) -> Tensor");
  m.def("spatial_attention(Tensor qkv, int B, int N, int H, int D=64) -> Tensor");
  m.def("temporal_attention(Tensor qkv, int B, int T, int S, int H, int D, float rope_theta=0.) -> Tensor");
  m.def("upsample_bilinear(Tensor x, int Ho, int Wo) -> Tensor");
  m.def("patch_im2col(Tensor img, int Kp, ScalarType dtype=float16) -> Tensor");
  m.def("depth_head(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, int Ho, int Wo) -> Tensor");
  m.def("preprocess_frames(Tensor frames, int H, int W, float[] mean, float[] std) -> Tensor");
  m.def("depth_resize(Tensor depth, int ho, int wo) -> Tensor");
  m.def("scale_shift(Tensor pred, Tensor target, Tensor? mask=None) -> (Tensor ss, Tensor sums)");
  m.def("depth_align(Tensor src, int ho, int wo, Tensor? ss=None, bool clip=True, Tensor? pre=None, "
        "float[]? w_pre=None, float[]? w_post=None, Tensor(a!)? out=None) -> Tensor");
  m.def("depth_eval_fit(Tensor pred, Tensor gt, Tensor? valid=None, bool per_frame=False) -> (Tensor ss, Tensor sums)");
  m.def("depth_eval_metrics(Tensor pred, Tensor gt, Tensor? valid, Tensor ss, float max_depth=80., "
        "bool want_aligned=False) -> (Tensor frame_sums, Tensor total, Tensor? aligned)");
  m.def("cloud_count(Tensor depth, Tensor? valid, int step, float trunc) -> (Tensor frame_offsets, Tensor ws)");
  m.def("cloud_write(Tensor depth, Tensor? valid, Tensor? rgb, Tensor K, Tensor? M, int step, float trunc, int layout, "
        "Tensor ws, int n) -> (Tensor out, Tensor? colors)");
}

#define VDA_IMPL(KEY)                                         \
  TORCH_LIBRARY_IMPL(vda, KEY, m) {                           \
    m.impl("gemm", &gemm);                                    \
    m.impl("gemm.out", &gemm_out);                            \
    m.impl("conv_transpose_ks", &conv_transpose_ks);          \
    m.impl("subpixel_conv", &subpixel_conv);                  \
    m.impl("conv2d", &conv2d);                                \
    m.impl("layernorm", &layernorm);                          \
    m.impl("row_stats", &row_stats);                          \
    m.impl("groupnorm", &groupnorm);                          \
    m.impl("groupnorm_linear", &groupnorm_linear);            \
    m.impl("spatial_attention", &spatial_attention);          \
    m.impl("temporal_attention", &temporal_attention);        \
    m.impl("upsample_bilinear", &upsample_bilinear);          \
    m.impl("patch_im2col", &patch_im2col);                    \
    m.impl("depth_head", &depth_head);                        \
    m.impl("preprocess_frames", &preprocess_frames);          \
    m.impl("depth_resize", &depth_resize);                    \
    m.impl("scale_shift", &scale_shift);                      \
    m.impl("depth_align", &depth_align);                      \
    m.impl("depth_eval_fit", &depth_eval_fit);                \
    m.impl("depth_eval_metrics", &depth_eval_metrics);        \
    m.impl("cloud_count", &cloud_count);                      \
    m.impl("cloud_write", &cloud_write);                      \
    m.impl("depth_range", &depth_range);                      \
    m.impl("depth_colorize", &depth_colorize);                \
    m.impl("depth_absdiff_range", &depth_absdiff_range);      \
    m.impl("panel_compose", &panel_compose);                  \
    m.impl("yuv_to_rgb", &yuv_to_rgb);                        \
    m.impl("preprocess_yuv", &preprocess_yuv);                \
    m.impl("yuv_downscale", &yuv_downscale);                  \
  }

VDA_IMPL(CUDA)
VDA_IMPL(Meta)
