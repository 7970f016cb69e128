// UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models";
// data prediction, multistep, orders 1 - 3) as one launch per model evaluation: the corrector of the step that led here
// and the predictor of the step that leaves.  See include/upk.h, upk_unipc_step_f32, for the coefficient row.
#include "common.h"

namespace {

// The thread layout of dpm.hip: one thread owns one (sample, pixel) and walks its C channels, so the fp32 NCHW loads and
// stores of a channel are stride-1 across the wave and the pixel's fp16 NHWC stem-input row leaves as ONE 8-byte store
// per lane for C = 4 (CT = 4); CT = 0: any channel count, the row element by element.
// The row says which operands exist: x_corr and the ring slots are uninitialised memory at a chain's start, so a term
// whose weight is zero is not loaded (0 * NaN is NaN).  The weights are wave-uniform: the branches do not diverge.
template <int CT>
__global__ void unipc_step_kernel(float* x, const float* eps, const float* coefs, const int* step, float* hist,
                                  float* x_corr, float* pred_x0, f16* xin, int ld_xin, int c_rt, int hw, long npix,
                                  int cfg_rows, float scale, int* done) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;  // b * hw + p
  const int st = step ? *step : 0;
  if (pix < npix) {
    const int c = CT ? CT : c_rt;
    const float* cf = coefs + 12 * (long)st;
    const float sig = cf[0], ralpha = cf[1];
    const float c_x = cf[2], c_h = cf[3], c_d0 = cf[4], c_d1 = cf[5], c_d2 = cf[6];
    const float p_x = cf[7], p_m = cf[8], p_d0 = cf[9], p_d1 = cf[10];
    const bool corr = cf[11] != 0.f;
    const bool need_h0 = corr || p_d0 != 0.f;
    const bool need_h1 = (corr && c_d1 != 0.f) || p_d1 != 0.f;
    const bool need_h2 = corr && c_d2 != 0.f;
    const long b = pix / hw;
    const long base = b * c * hw + (pix - b * hw);
    const long n = npix * c;
    // ring slots: m_k goes to slot k mod 3 (the slot of evaluation k - 3), evaluation k - j sits in slot (k - j) mod 3
    const int s0 = (st + 2) % 3, s1 = (st + 1) % 3, s2 = st % 3;
    const float* h0p = hist + s0 * n;
    const float* h1p = hist + s1 * n;
    float* h2p = hist + s2 * n;
    f16* row = xin ? xin + pix * ld_xin : nullptr;
    f16* row2 = (xin && cfg_rows == 2) ? xin + (npix + pix) * ld_xin : nullptr;  // the conditional half
    f16 h[CT ? CT : 1];
#pragma unroll
    for (int ch = 0; ch < c; ++ch) {
      const long idx = base + (long)ch * hw;
      float e = eps[idx];
      if (cfg_rows == 2) e = e + scale * (eps[n + idx] - e);
      const float xv = x[idx];
      const float m = (xv - sig * e) * ralpha;
      float h0 = 0.f, h1 = 0.f;
      if (need_h0) h0 = h0p[idx];
      if (need_h1) h1 = h1p[idx];
      float xc = xv;
      if (corr) {
        xc = c_x * x_corr[idx] + c_h * h0 + c_d0 * (m - h0);
        if (c_d1 != 0.f) xc += c_d1 * (h1 - h0);
        if (need_h2) xc += c_d2 * (h2p[idx] - h0);
      }
      float xn = p_x * xc + p_m * m;
      if (p_d0 != 0.f) xn += p_d0 * (h0 - m);
      if (p_d1 != 0.f) xn += p_d1 * (h1 - m);
      x_corr[idx] = xc;
      x[idx] = xn;
      h2p[idx] = m;
      if (pred_x0) pred_x0[idx] = m;
      if (CT) {
        h[ch] = (f16)xn;
      } else if (row) {
        row[ch] = (f16)xn;
        if (row2) row2[ch] = (f16)xn;
      }
    }
    if (CT == 4 && row) {
      const f16x4 v = {h[0], h[1], h[2], h[3]};
      upk_stem_row_store4(row, v);
      if (row2) upk_stem_row_store4(row2, v);
    }
  }
  if (step) step_advance(step, done);
}

inline bool misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

}  // namespace

extern "C" int upk_unipc_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const int32_t* step,
                                  float* hist, float* x_corr, float* pred_x0, void* xin, int ld_xin, int batch, int c,
                                  int hw, float cfg_scale, int cfg, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !eps || !coefs || !hist || !x_corr || batch <= 0 || c <= 0 || hw <= 0)
    return upk_fail(ctx, UPK_EINVAL, "unipc_step: bad args");
  if (xin && ld_xin < c) return upk_fail(ctx, UPK_EINVAL, "unipc_step: ld_xin < c");
  if (misaligned(x, 4) || misaligned(eps, 4) || misaligned(coefs, 4) || misaligned(step, 4) || misaligned(hist, 4) ||
      misaligned(x_corr, 4) || misaligned(pred_x0, 4) || misaligned(xin, 2))
    return upk_fail(ctx, UPK_EINVAL, "unipc_step: misaligned pointer");
  const long npix = (long)batch * hw;
  const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  if (c == 4)
    hipLaunchKernelGGL(unipc_step_kernel<4>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, step, hist, x_corr,
                       pred_x0, (f16*)xin, ld_xin, c, hw, npix, cfg ? 2 : 1, cfg_scale, ctx->step_done);
  else
    hipLaunchKernelGGL(unipc_step_kernel<0>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, step, hist, x_corr,
                       pred_x0, (f16*)xin, ld_xin, c, hw, npix, cfg ? 2 : 1, cfg_scale, ctx->step_done);
  return upk_check_launch(ctx, "unipc_step");
}
