// DPM-Solver++(2M) update (Lu et al. 2022, "DPM-Solver++", algorithm 2; data prediction, multistep, eta = 0) as one
// launch per model evaluation: see include/upk.h, upk_dpmpp_2m_step_f32, for the coefficient row.
#include "common.h"

namespace {

// One thread owns one (sample, pixel) and walks its C channels: the fp32 NCHW loads and stores of a channel are
// stride-1 across the wave (256 B per wave instruction), and the pixel's fp16 NHWC stem-input row — C contiguous
// halves — leaves as ONE 8-byte store per lane for C = 4 (CT = 4) instead of four 2-byte stores from four different
// waves.  CT = 0: any channel count, the row element by element (the upscale model's C = 3 rows are 6 bytes).
// x0_old is read only on a second-order row: on the first row of a chain it is uninitialised memory.
template <int CT>
__global__ void dpmpp_2m_step_kernel(float* x, const float* eps, const float* coefs, const int* step, float* x0_old,
                                     float* pred_x0, f16* xin, int ld_xin, int c_rt, int hw, long npix, int first_row,
                                     int cfg_rows, float scale, int* done) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;  // b * hw + p
  const int st = step ? *step : 0;
  if (pix < npix) {
    const int c = CT ? CT : c_rt;
    const float* cf = coefs + 8 * (long)st;
    const float sig_t = cf[0], ralpha_t = cf[1], kx = cf[2], kd = cf[3], w = cf[4];
    const bool second = w != 0.f && st != first_row;
    const long b = pix / hw;
    const long base = b * c * hw + (pix - b * hw);
    const long n = npix * c;
    f16* row = xin ? xin + pix * ld_xin : nullptr;
    f16* row2 = (xin && cfg_rows == 2) ? xin + (npix + pix) * ld_xin : nullptr;  // the conditional half
    f16 h[CT ? CT : 1];
#pragma unroll
    for (int ch = 0; ch < c; ++ch) {
      const long idx = base + (long)ch * hw;
      float e = eps[idx];
      if (cfg_rows == 2) e = e + scale * (eps[n + idx] - e);
      const float xv = x[idx];
      const float p0 = (xv - sig_t * e) * ralpha_t;
      float d = p0;
      if (second) d = p0 + w * (p0 - x0_old[idx]);
      const float xp = kx * xv + kd * d;
      x[idx] = xp;
      x0_old[idx] = p0;
      if (pred_x0) pred_x0[idx] = p0;
      if (CT) {
        h[ch] = (f16)xp;
      } else if (row) {
        row[ch] = (f16)xp;
        if (row2) row2[ch] = (f16)xp;
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

}  // namespace

extern "C" int upk_dpmpp_2m_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const int32_t* step,
                                     float* x0_old, float* pred_x0, void* xin, int ld_xin, int batch, int c, int hw,
                                     int first_row, float cfg_scale, int cfg, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !eps || !coefs || !x0_old || batch <= 0 || c <= 0 || hw <= 0 || first_row < 0)
    return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_step: bad args");
  if (xin && ld_xin < c) return upk_fail(ctx, UPK_EINVAL, "dpmpp_2m_step: ld_xin < c");
  const long npix = (long)batch * hw;
  const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  if (c == 4)
    hipLaunchKernelGGL(dpmpp_2m_step_kernel<4>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, step, x0_old,
                       pred_x0, (f16*)xin, ld_xin, c, hw, npix, first_row, cfg ? 2 : 1, cfg_scale, ctx->step_done);
  else
    hipLaunchKernelGGL(dpmpp_2m_step_kernel<0>, grid, block, 0, (hipStream_t)stream_, x, eps, coefs, step, x0_old,
                       pred_x0, (f16*)xin, ld_xin, c, hw, npix, first_row, cfg ? 2 : 1, cfg_scale, ctx->step_done);
  return upk_check_launch(ctx, "dpmpp_2m_step");
}
