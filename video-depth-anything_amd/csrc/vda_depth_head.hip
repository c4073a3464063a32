// Depth-head router: the DPT head's tail (bilinear resize to (Ho, Wo), 3x3 conv C -> 32, ReLU, 1x1 conv
// 32 -> 1, ReLU; fp32 depth) through the depth conv of vda_dconv.hip or, for the channel counts it does
// not serve, the implicit-GEMM tail of vda_gemm.hip.  Host code only.
#include "vda_internal.h"

extern "C" int vda_depth_head(const void* x, const void* w1, const float* b1, const float* w2, const float* b2,
                              float* depth, void* ws, int32_t BT, int32_t Hin, int32_t Win, int32_t C, int32_t Ho,
                              int32_t Wo, void* stream) {
  VDA_CHECK_ARG(x && w1 && b1 && w2 && b2 && depth, "null pointer");
  VDA_CHECK_ARG(BT > 0 && Hin > 0 && Win > 0 && Ho > 0 && Wo > 0, "bad depth-head geometry");
  VDA_CHECK_ARG(C % 8 == 0, "depth head needs C % 8 == 0");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  // vda_debug_force_tile(13) (tuning build; any value >= 10): the implicit-GEMM tail for every shape; lower
  // values are the GEMM's and the conv's and do not move the depth tail
  const bool gemm_tail = g_force_tile >= 10;
  // 1) the depth conv of vda_dconv.hip (two 4-wave blocks per CU, 64 pixels x all 64 hi/lo rows per wave)
  //    with the bilinear resize fused into its patch building: the resized map is never written
  if (!gemm_tail) {
    rc = vda_depth_conv_fused(x, w1, b1, w2, b2, depth, BT, Hin, Win, Ho, Wo, C, st);
    if (rc != 1) return rc;
  }
  // 2) bilinear (align_corners=True) resize of the output_conv1 map into ws, fp16 like the reference's
  //    autocast interpolate (dpt_temporal.py:92-94), and the same conv on the materialised map
  //    (bit-identical to 1; also vda_debug_dconv(2))
  VDA_CHECK_ARG(ws, "depth head: needs the resize workspace (vda_depth_head_workspace)");
  rc = vda_upsample_bilinear(x, ws, BT, Hin, Win, C, Ho, Wo, stream);
  if (rc) return rc;
  if (!gemm_tail) {
    rc = vda_depth_conv(ws, w1, b1, w2, b2, depth, BT, Ho, Wo, C, st);
    if (rc != 1) return rc;
  }
  // 3) C % 32 != 0: the implicit-GEMM conv with split-fp16 weights + fused ReLU / 1x1 / ReLU epilogue
  GemmParams p{};
  p.x = (const h16*)ws; p.w = (const h16*)w1; p.y = (h16*)depth;
  p.H = Ho; p.W = Wo; p.Cin = C; p.ks = 3; p.stride = 1; p.pad = 1; p.pre_relu = 0;
  p.Ho = Ho; p.Wo = Wo;
  p.M = BT * Ho * Wo; p.N = 64; p.K = 9 * C; p.ldy = 1;
  p.epi = vda_default_epi();
  p.epi.bias = b1; p.epi.gamma = w2; p.epi.rowbias = b2;
  return vda_launch_depth_gemm(p, st);
}

extern "C" int64_t vda_depth_head_workspace(int32_t BT, int32_t Hin, int32_t Win, int32_t C, int32_t Ho, int32_t Wo) {
  if (BT <= 0 || Hin <= 0 || Win <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return 0;
  if (g_force_tile < 10 && vda_depth_conv_fused_serves(Hin, Win, Ho, Wo, C)) return 0;  // fused: no resized map
  return (int64_t)BT * Ho * Wo * C * 2;
}
