// 3x3 / stride 1 / same-padding convolution with the weights streamed through LDS (conv3_x ..
// conv5_x: cin % 32 == 0, kout % 128 == 0, up to 1024): the C entry points (scl_convg*,
// include/scl_hip.h), the argument checks and the choice of kernel.  Kernels and launchers: convh.hip
// (16x16x32 MFMA; 32-channel chunks in pairs — every VGG layer) and convg.hip (32x32x16; the odd
// chunk counts).  A launcher trusts the LdsConvCall it gets (conv_lds.h).
#include "conv_lds.h"

extern "C" size_t scl_convg_workspace_bytes(int cin, int kout) {
  if (cin < 32 || kout < 128 || cin % 32 || kout % 128 || cin > 1024 || kout > 1024) return 0;
  return scl_round256((size_t)9 * (cin / 32) * kout * LDS_CONV_ROW * sizeof(unsigned short));
}

// The contract of scl_conv3x3_fused / scl_conv3x3_masked (include/scl_hip.h), no pooled output.
static int lds_conv(LdsConvCall c, size_t workspace_bytes) {
  if (!c.x || !c.w || !c.out || !c.workspace) return SCL_E_NULL;
  if (c.pidx && (!c.bias || c.mask)) return SCL_E_NULL;
  if (c.mask && (c.bias || ((uintptr_t)c.mask % 16))) return SCL_E_NULL;
  const size_t need = scl_convg_workspace_bytes(c.cin, c.kout);
  const int64_t pixels = (int64_t)c.B * c.H * c.W;
  if (need == 0 || c.B < 1 || c.H < 1 || c.W < 1 || pixels > (int64_t)1 << 30) return SCL_E_SHAPE;
  if (((uintptr_t)c.x % 16) || ((uintptr_t)c.out % 16)) return SCL_E_SHAPE;
  if (pixels * c.cin >= (int64_t)1 << 31) return SCL_E_SHAPE;             // 32-bit offsets
  if (!scl_aligned256(c.workspace) || workspace_bytes < need) return SCL_E_WORKSPACE;
  // scl_debug_set_variant(40000 + v) pins the 32x32x16 kernel, 50000 + v the 16x16x32 one, each
  // with the diagnostic variant v of its launcher; plain v goes to the kernel chosen here
  c.dv = scl_variant();
  const bool pin_g = c.dv >= 40000 && c.dv < 50000, pin_h = c.dv >= 50000 && c.dv < 60000;
  if (pin_g || pin_h) c.dv -= pin_g ? 40000 : 50000;
  const bool use_h = !pin_g && c.cin % 64 == 0;      // convh.hip walks the 32-channel chunks in pairs
  if ((c.flags & SCL_W_PACKED) && !use_h) return SCL_E_KIND;   // packed images: convh.hip's layout only
  return use_h ? convh_launch(c) : convg_launch(c);
}

extern "C" int scl_convg(const void* x, const void* w, int64_t w_stride_k, int64_t w_stride_c,
                         int64_t w_stride_h, int64_t w_stride_w, int transposed, int B, int H,
                         int W, int cin, int kout, void* out, const float* bias, int relu,
                         void* workspace, size_t workspace_bytes, void* stream) {
  LdsConvCall c{x, w, w_stride_k, w_stride_c, w_stride_h, w_stride_w, transposed, B, H, W, cin, kout};
  c.out = out, c.bias = bias, c.relu = relu, c.workspace = workspace, c.stream = (hipStream_t)stream;
  return lds_conv(c, workspace_bytes);
}

extern "C" int scl_convg_pool_idx(const void* x, const void* w, int64_t w_stride_k,
                                  int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w,
                                  int flags, int B, int H, int W, int cin, int kout,
                                  const float* bias, void* pooled, void* pool_idx, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!pool_idx || !pooled || !bias) return SCL_E_NULL;
  LdsConvCall c{x, w, w_stride_k, w_stride_c, w_stride_h, w_stride_w, flags & 6, B, H, W, cin, kout};
  c.out = pooled, c.bias = bias, c.pidx = pool_idx, c.workspace = workspace, c.stream = (hipStream_t)stream;
  return lds_conv(c, workspace_bytes);
}

extern "C" int scl_convg_masked(const void* x, const void* w, int64_t w_stride_k,
                                int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w,
                                int transposed, int B, int H, int W, int cin, int kout, void* out,
                                const void* mask, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!mask) return SCL_E_NULL;
  LdsConvCall c{x, w, w_stride_k, w_stride_c, w_stride_h, w_stride_w, transposed, B, H, W, cin, kout};
  c.out = out, c.mask = mask, c.workspace = workspace, c.stream = (hipStream_t)stream;
  return lds_conv(c, workspace_bytes);
}
