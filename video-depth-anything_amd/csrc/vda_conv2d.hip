// Conv router: vda_conv2d picks, per shape, the halo-tiled phased conv (vda_hconv.hip), the strip-tiled
// conv (vda_strip.hip), the 128-channel halo conv (vda_depth.hip), explicit im2col + the dense GEMM, or
// the implicit-GEMM conv of vda_gemm.hip; vda_conv2d_workspace / vda_conv2d_res2_upsample_ok answer for
// the same choice.  Host code only.
#include "vda_internal.h"

// The strip-tiled 3x3 conv (vda_strip.hip) serves 3x3 / s1 / p1 convs with 256 output channels and
// Cin >= 512 on maps up to 160 wide (layer2..4_rn; measured 10-14% faster there, 1-4% slower than the
// implicit GEMM at Cin = 256), and any Cout = 256 3x3 conv whose 256-pixel strip tiles would fill at
// most half the CUs (19^2 maps: the strip kernel then splits the input channels over several work
// items).  vda_debug_force_tile(-3) routes every Cout = 256 conv to it, (-2) none.
static bool conv_takes_strip(int BT, int H, int W, int Cin, int Cout, int ks, int stride, int pad, int up_h) {
  if (up_h > 0 || ks != 3 || stride != 1 || pad != 1 || !vda_conv_strip_serves(W, Cin, Cout)) return false;
  const long strip_tiles = (long)BT * ((H * W + 255) / 256);
  return g_force_tile == -3 || (g_force_tile == -1 && (Cin >= 512 || strip_tiles * 2 <= vda_cu_count()));
}

// Stride-2 3x3 convs (the DPT reassemble's resize_layers[3], dpt.py:77-82: 1024 -> 1024 at 37^2 -> 19^2):
// explicit im2col into the workspace + the dense phased GEMM.  The implicit-GEMM conv runs its K steps at
// about half the dense rate, and at 184 tiles x 144 K steps (32 frames) the copy costs far less than that
// (410 -> 210 us of GEMM for ~70 us of copy, tools/archive/s2conv_probe.py); bit-identical (same K order).
static long conv_im2col_bytes(int BT, int H, int W, int Cin, int ks, int stride, int pad) {
  const long Ho = (H + 2L * pad - ks) / stride + 1, Wo = (W + 2L * pad - ks) / stride + 1;
  return (long)BT * Ho * Wo * ks * ks * Cin * 2;
}
static bool conv_takes_im2col(int BT, int H, int W, int Cin, int Cout, int ks, int stride, int pad, int up_h) {
  if (up_h > 0 || ks != 3 || stride != 2 || Cout % 256 != 0 || g_force_tile != -1) return false;
  const long Ho = (H + 2L * pad - ks) / stride + 1, Wo = (W + 2L * pad - ks) / stride + 1;
  // worth the copy only where the GEMM route gives the [M, 9 Cin] matrix to the phased 256x256 dense kernel
  return Ho > 0 && Wo > 0 && vda_gemm_phased256_serves((long)BT * Ho * Wo, Cout, 9L * Cin, 9L * Cin);
}

// the halo-tiled 256-channel conv route (the only one whose epilogue reads an upsampled res2)
static bool conv_takes_hconv(int BT, int H, int W, int Cin, int Cout, int ks, int stride, int pad) {
  return ks == 3 && stride == 1 && pad == 1 && g_force_tile == -1 && vda_conv_hconv_serves(BT, H, W, Cin, Cout);
}

extern "C" int64_t vda_conv2d_workspace(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks,
                                        int32_t stride, int32_t pad) {
  if (BT <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (conv_takes_hconv(BT, H, W, Cin, Cout, ks, stride, pad)) return 0;
  if (conv_takes_im2col(BT, H, W, Cin, Cout, ks, stride, pad, 0)) return conv_im2col_bytes(BT, H, W, Cin, ks, stride, pad);
  if (!conv_takes_strip(BT, H, W, Cin, Cout, ks, stride, pad, 0)) return 0;
  return vda_conv_strip_ws_bytes(BT, H, W, Cin, Cout);
}

extern "C" int vda_conv2d_res2_upsample_ok(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks,
                                           int32_t stride, int32_t pad) {
  if (BT <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return conv_takes_hconv(BT, H, W, Cin, Cout, ks, stride, pad) ? 1 : 0;
}

extern "C" int vda_conv2d_bias9_ok(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t up_h,
                                   int32_t up_w) {
  if (BT <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || up_h <= 0 || up_w <= 0 || g_force_tile >= 0) return 0;
  return vda_conv_halo_fused_serves(BT, H, W, up_h, up_w, Cin, Cout) ? 1 : 0;
}

extern "C" int vda_conv2d(const void* x, const void* w, void* y, int32_t BT, int32_t H, int32_t W,
                          int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad,
                          int32_t pre_relu, int32_t up_h, int32_t up_w, const vda_epilogue* epi,
                          void* ws, int64_t ws_bytes, void* stream) {
  VDA_CHECK_ARG(x && w && y, "null pointer");
  VDA_CHECK_ARG(BT > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ks > 0 && stride > 0 && pad >= 0,
                "bad conv geometry");
  VDA_CHECK_ARG(Cin % 8 == 0 && Cout % 4 == 0, "Cin % 8 and Cout % 4 required");
  const int Hi = up_h > 0 ? up_h : H, Wi = up_w > 0 ? up_w : W;
  GemmParams p{};
  p.x = (const h16*)x; p.w = (const h16*)w; p.y = (h16*)y;
  p.H = H; p.W = W; p.Cin = Cin; p.ks = ks; p.stride = stride; p.pad = pad; p.pre_relu = pre_relu;
  p.up_h = up_h > 0 ? up_h : 0; p.up_w = up_w > 0 ? up_w : 0;
  p.Ho = (Hi + 2 * pad - ks) / stride + 1;
  p.Wo = (Wi + 2 * pad - ks) / stride + 1;
  VDA_CHECK_ARG(p.Ho > 0 && p.Wo > 0, "empty conv output");
  p.M = BT * p.Ho * p.Wo; p.N = Cout; p.K = ks * ks * Cin;
  p.ldy = Cout; p.ldx = 0;
  p.epi = epi ? *epi : vda_default_epi();
  if (p.epi.rdiv <= 0) p.epi.rdiv = 1;
  if (p.epi.rmod <= 0) p.epi.rmod = 1;
  VDA_CHECK_ARG(p.epi.store == VDA_STORE_ROWS && (p.epi.act == VDA_ACT_NONE || p.epi.act == VDA_ACT_RELU),
                "conv: row store, activation none/relu");
  VDA_CHECK_ARG(!p.epi.stats_out && !p.epi.ln_stats, "conv: no LayerNorm fold / row statistics");
  int rc = vda_check_epi(p.epi, p.M, Cout);
  if (rc) return rc;
  const bool res2_up = p.epi.res2_h > 0 || p.epi.res2_w > 0;
  if (res2_up) {  // refinenet1's skip add on the previous block's output, upsampled in the epilogue
    VDA_CHECK_ARG(p.epi.res2 && p.epi.res2_h > 0 && p.epi.res2_w > 0 && p.epi.ldres2 == Cout && p.up_h == 0 &&
                      !p.epi.gamma && !p.epi.rowbias && (!p.epi.res || p.epi.ldres == Cout) &&
                      p.epi.res2_h <= p.Ho && p.epi.res2_w <= p.Wo &&
                      (long)p.epi.res2_h * p.epi.res2_w * Cout * 2 < (1L << 31) &&
                      conv_takes_hconv(BT, H, W, Cin, Cout, ks, stride, pad),
                  "upsampled res2 needs the halo conv route (vda_conv2d_res2_upsample_ok), a [BT, h <= Ho, w <= Wo, "
                  "Cout] source, no gamma / rowbias / input upsample");
    return vda_conv_hconv(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, pre_relu, p.epi.res, p.epi.res2,
                          p.epi.res2_h, p.epi.res2_w, BT, H, W, Cin, Cout, (hipStream_t)stream);
  }
  // a 9-class bias table exists in the halo conv with the fused resize only
  VDA_CHECK_ARG(!p.epi.bias9 || (!p.epi.bias && (uintptr_t)p.epi.bias9 % 16 == 0 && ks == 3 && stride == 1 && pad == 1 &&
                                 !pre_relu && !p.epi.res && !p.epi.res2 && !p.epi.gamma && !p.epi.rowbias &&
                                 vda_conv2d_bias9_ok(BT, H, W, Cin, Cout, p.up_h, p.up_w)),
                "bias9: the 3x3 conv through a fused resize only (vda_conv2d_bias9_ok), 16-byte aligned, in place "
                "of bias, no residual / gamma / rowbias / pre-ReLU");
  if (p.up_h > 0) {
    // 3x3 conv on a bilinear resize with 128 outputs (output_conv1 on refinenet1's x2 resize): the
    // halo conv with the resize fused into its patch staging (bit-identical to resize + conv)
    if (g_force_tile < 0 && ks == 3 && stride == 1 && pad == 1 && !pre_relu && !p.epi.res && !p.epi.res2 &&
        !p.epi.gamma && !p.epi.rowbias) {
      // an exact x2 resize with a bias9 table: the channel mixing at the source resolution, a quarter of the
      // matrix work (vda_oc1_src.hip; same linear map, not the same bits, so a plain-bias call is not routed there)
      rc = vda_conv_oc1_src(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, BT, H, W, p.up_h, p.up_w, Cin, Cout,
                            (hipStream_t)stream, p.epi.bias9);
      if (rc != 1) return rc;
      rc = vda_conv_halo_fused(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, BT, H, W, p.up_h, p.up_w, Cin, Cout,
                               (hipStream_t)stream, p.epi.bias9);
      if (rc != 1) return rc;
    }
    return vda_launch_conv_reg(p, (hipStream_t)stream);
  }
  // large maps with 256 output channels (the refinenet RCU convs and layer1_rn at 148^2): the
  // halo-tiled phased conv stages each input patch once per 64-channel slab instead of 9 times
  if (!p.epi.gamma && !p.epi.rowbias && (!p.epi.res || p.epi.ldres == Cout) && (!p.epi.res2 || p.epi.ldres2 == Cout) &&
      conv_takes_hconv(BT, H, W, Cin, Cout, ks, stride, pad)) {
    rc = vda_conv_hconv(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, pre_relu, p.epi.res, p.epi.res2, 0, 0, BT, H,
                        W, Cin, Cout, (hipStream_t)stream);
    if (rc != 1) return rc;
  }
  if (conv_takes_strip(BT, H, W, Cin, Cout, ks, stride, pad, 0) && !p.epi.gamma && !p.epi.rowbias &&
      (!p.epi.res || p.epi.ldres == Cout) && (!p.epi.res2 || p.epi.ldres2 == Cout)) {
    rc = vda_conv_strip(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, pre_relu, p.epi.res, p.epi.res2, BT, H, W,
                        Cin, Cout, ws, ws ? ws_bytes : 0, (hipStream_t)stream);
    if (rc != 1) return rc;
  }
  // large 3x3 maps with 128 output channels (output_conv1 at 296^2): halo-tiled kernel (vda_depth.hip)
  if (g_force_tile < 0 && ks == 3 && stride == 1 && pad == 1 && !pre_relu && !p.epi.res && !p.epi.res2 &&
      !p.epi.gamma && !p.epi.rowbias && (long)H * W >= 128L * 128L) {
    rc = vda_conv_halo(x, w, y, p.epi.bias, p.epi.act == VDA_ACT_RELU, BT, H, W, Cin, Cout, (hipStream_t)stream);
    if (rc != 1) return rc;
  }
  if (conv_takes_im2col(BT, H, W, Cin, Cout, ks, stride, pad, 0) && !pre_relu && ws &&
      ws_bytes >= conv_im2col_bytes(BT, H, W, Cin, ks, stride, pad) && (uintptr_t)ws % 16 == 0 &&
      (uintptr_t)x % 16 == 0) {
    rc = vda_conv_im2col(x, ws, BT, H, W, Cin, p.Ho, p.Wo, ks, stride, pad, (hipStream_t)stream);
    if (rc) return rc;
    p.x = (const h16*)ws;
    p.ldx = p.K;
    return vda_launch_gemm(p, (hipStream_t)stream);
  }
  return vda_launch_conv_gemm(p, (hipStream_t)stream);
}
