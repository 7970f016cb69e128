// SDE-DPM-Solver++(2M) update (Lu et al. 2022, "DPM-Solver++", the sde-dpmsolver++ multistep form; data prediction, eta
// interpolating between the ODE and the SDE) as one launch per model evaluation, with the editing chains' blend for the
// next step: see include/upk.h, upk_dpmpp_2m_sde_step_f32, for the coefficient row.
#include "common.h"

namespace {

// The thread layout of dpm.hip / unipc.hip: one thread owns one (sample, pixel) and walks its C channels, so the fp32
// NCHW loads and stores of a channel are stride-1 across the wave and the pixel's fp16 NHWC stem-input row leaves as ONE
// 8-byte store per lane for C = 4 (CT = 4) where its address allows; CT = 0: any channel count, element by element.
// The row says whether m_old exists: on a first-order row (w = 0: a chain's first row, order 1, a lower-order final row)
// it is uninitialised memory and is not loaded.  w, the noise / mask pointers and the last-row test are wave-uniform.
template <int CT>
__global__ void dpmpp_2m_sde_step_kernel(float* x, const float* eps, const float* coefs, const float* noise,
                                         const float* keep, const float* mask, int n_rows, const int* step, float* m_old,
                                         float* pred_x0, float* x_plain, f16* xin, int ld_xin, int c_rt, int hw, long npix,
                                         int cfg_rows, float scale, int* done) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;  // b * hw + p
  const int st = step ? *step : 0;
  if (pix < npix) {
    const int c = CT ? CT : c_rt;
    const float* cf = coefs + 8 * (long)st;
    const float sig = cf[0], ralpha = cf[1], kx = cf[2], kd = cf[3], w = cf[4];
    const bool second = w != 0.f;
    const long b = pix / hw;
    const long base = b * c * hw + (pix - b * hw);
    const long n = npix * c;
    const float* nz = noise ? noise + (long)st * n : nullptr;
    // the reference blends in front of the NEXT evaluation (ddim.py:144-147); the last row's result is never blended
    const float* kp = (mask && st + 1 < n_rows) ? keep + (long)(st + 1) * n : nullptr;
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
      float d = m;
      if (second) d = m + w * (m - m_old[idx]);
      float xn = kx * xv + kd * d;
      if (nz) xn += nz[idx];
      if (x_plain) x_plain[idx] = xn;
      if (kp) {
        const float mk = mask[idx];
        xn = mk * kp[idx] + (1.f - mk) * xn;
      }
      x[idx] = xn;
      m_old[idx] = m;
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

extern "C" int upk_dpmpp_2m_sde_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const float* noise,
                                         const float* keep, const float* mask, int n_rows, const int32_t* step,
                                         float* m_old, float* pred_x0, float* x_plain, void* xin, int ld_xin, int batch,
                                         int c, int hw, float cfg_scale, int cfg, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !eps || !coefs || !m_old || batch <= 0 || c <= 0 || hw <= 0)
    return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_sde_step: bad args");
  if (mask && (!keep || n_rows <= 0)) return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_sde_step: mask without keep rows");
  if (xin && ld_xin < c) return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_sde_step: ld_xin < c");
  if (misaligned(x, 4) || misaligned(eps, 4) || misaligned(coefs, 4) || misaligned(noise, 4) || misaligned(keep, 4) ||
      misaligned(mask, 4) || misaligned(step, 4) || misaligned(m_old, 4) || misaligned(pred_x0, 4) ||
      misaligned(x_plain, 4) || misaligned(xin, 2))
    return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_sde_step: misaligned pointer");
  const long npix = (long)batch * hw;
  const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  if (c == 4)
    hipLaunchKernelGGL(dpmpp_2m_sde_step_kernel<4>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, noise, keep,
                       mask, n_rows, step, m_old, pred_x0, x_plain, (f16*)xin, ld_xin, c, hw, npix, cfg ? 2 : 1, cfg_scale,
                       ctx->step_done);
  else
    hipLaunchKernelGGL(dpmpp_2m_sde_step_kernel<0>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, noise, keep,
                       mask, n_rows, step, m_old, pred_x0, x_plain, (f16*)xin, ld_xin, c, hw, npix, cfg ? 2 : 1, cfg_scale,
                       ctx->step_done);
  return upk_check_launch(ctx, "dpmpp_2m_sde_step");
}
