// upk_image_finish_u8: fp32 images -> a window of a uint8 HWC picture, the tail of LatentDiffusion.test_step
// (ddpm.py:1352-1357, 1371-1376): centre crop, clamp / rescale / CLIP de-normalisation, the width concat (through the
// destination window) and ToPILImage's mul(255).byte(), in one launch per component.
//
// The result is TRUNCATED to a byte, so the last bit of every fp32 operation decides bytes: each operation below is one
// correctly rounded IEEE fp32 operation in the order include/upk.h states, nothing is contracted into an FMA and
// nothing is reassociated.  The library is built with -ffp-contract=fast; this file gets -ffp-contract=off from
// build.py's FILE_FLAGS, and says so itself for whoever compiles it another way:
#pragma clang fp contract(off)
//
// Memory- and launch-bound (a few MB per batch).  Fast path: one thread = 4 horizontally adjacent pixels, 16-byte loads
// (one per channel plane for NCHW, three consecutive ones for NHWC), 12 packed bytes out as three dword stores; taken
// when the source window, the crop width and the destination offset are multiples of 4 pixels and the bases / strides
// keep the vectors aligned.  Everything else (odd widths, odd offsets) takes one thread per pixel and byte stores.
#include "common.h"

namespace {

struct FinishArgs {
  const float* src;
  uint8_t* dst;
  long src_bs;   // floats between source samples
  long dst_bs;   // bytes between destination samples
  long pitch;    // bytes between destination rows
  long total;    // work items: batch * crop_h * (fast ? crop_w / 4 : crop_w)
  int src_h, src_w, top, left, crop_h, crop_w, dst_x, nhwc, mode;
  float d[3], m[3];
};

// value -> byte.  SAMPLE: (clamp(v, -1, 1) + 1) / 2; INPUT: (v + 1) / 2; DENORM: v / d - m; then trunc(t * 255),
// saturated, NaN -> 0 (fmaxf returns the other operand for a NaN).
__device__ __forceinline__ uint32_t finish_byte(float v, int mode, float d, float m) {
  float t;
  if (mode == UPK_FINISH_SAMPLE) {
    t = (fminf(fmaxf(v, -1.0f), 1.0f) + 1.0f) / 2.0f;
  } else if (mode == UPK_FINISH_INPUT) {
    t = (v + 1.0f) / 2.0f;
  } else {
    t = __fdiv_rn(v, d) - m;
  }
  float p = t * 255.0f;
  p = fminf(fmaxf(p, 0.0f), 255.0f);
  return (uint32_t)(int)p;
}

__global__ __launch_bounds__(256) void image_finish_vec4_kernel(const FinishArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int wq = a.crop_w >> 2;
  const int xq = (int)(idx % wq);
  const long r = idx / wq;
  const int y = (int)(r % a.crop_h);
  const long b = r / a.crop_h;
  const int sy = a.top + y, sx = a.left + 4 * xq;
  const float* s = a.src + b * a.src_bs;
  float v[12];  // pixel-major, channel-minor: the byte order of the destination
  if (a.nhwc) {
    const f32x4* p = (const f32x4*)(s + ((long)sy * a.src_w + sx) * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const f32x4 q = p[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = q[j];
    }
  } else {
    const long plane = (long)a.src_h * a.src_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 q = *(const f32x4*)(s + c * plane + (long)sy * a.src_w + sx);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[3 * j + c] = q[j];
    }
  }
  uint32_t w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * k + j, c = i % 3;
      acc |= finish_byte(v[i], a.mode, a.d[c], a.m[c]) << (8 * j);
    }
    w[k] = acc;
  }
  uint32_t* o = (uint32_t*)(a.dst + b * a.dst_bs + (long)y * a.pitch + (long)(a.dst_x + 4 * xq) * 3);
  o[0] = w[0];
  o[1] = w[1];
  o[2] = w[2];
}

__global__ __launch_bounds__(256) void image_finish_pixel_kernel(const FinishArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int x = (int)(idx % a.crop_w);
  const long r = idx / a.crop_w;
  const int y = (int)(r % a.crop_h);
  const long b = r / a.crop_h;
  const int sy = a.top + y, sx = a.left + x;
  const float* s = a.src + b * a.src_bs;
  const long pix = (long)sy * a.src_w + sx;
  const long plane = (long)a.src_h * a.src_w;
  uint8_t* o = a.dst + b * a.dst_bs + (long)y * a.pitch + (long)(a.dst_x + x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = a.nhwc ? s[pix * 3 + c] : s[c * plane + pix];
    o[c] = (uint8_t)finish_byte(v, a.mode, a.d[c], a.m[c]);
  }
}

}  // namespace

extern "C" int upk_image_finish_u8(upk_ctx* ctx, const float* src, int layout, int batch, int src_h, int src_w,
                                   long long src_batch_stride, int top, int left, int crop_h, int crop_w, uint8_t* dst,
                                   long long dst_pitch, int dst_x, long long dst_sample_stride, int mode,
                                   const float* denorm_host, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!src || !dst) return upk_fail(ctx, UPK_EINVAL, "image_finish: null pointer");
  if ((uintptr_t)src & 3) return upk_fail(ctx, UPK_EINVAL, "image_finish: src is not 4-byte aligned");
  if (layout != UPK_LAYOUT_NCHW && layout != UPK_LAYOUT_NHWC) return upk_fail(ctx, UPK_EINVAL, "image_finish: unknown layout %d", layout);
  if (mode != UPK_FINISH_SAMPLE && mode != UPK_FINISH_INPUT && mode != UPK_FINISH_DENORM)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: unknown mode %d", mode);
  if (batch <= 0 || src_h <= 0 || src_w <= 0 || crop_h <= 0 || crop_w <= 0)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: sizes must be positive");
  if (top < 0 || left < 0 || (long)top + crop_h > src_h || (long)left + crop_w > src_w)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: window (%d, %d, %d, %d) outside the %d x %d source", top, left, crop_h,
                    crop_w, src_h, src_w);
  if (batch > 1 && src_batch_stride < 3LL * src_h * src_w)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: source samples overlap (batch stride %lld)", src_batch_stride);
  if (dst_x < 0 || ((long long)dst_x + crop_w) * 3 > dst_pitch)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: destination window [%d, %d) outside the row pitch of %lld bytes", dst_x,
                    dst_x + crop_w, dst_pitch);
  if (batch > 1 && dst_sample_stride < (long long)crop_h * dst_pitch)
    return upk_fail(ctx, UPK_EINVAL, "image_finish: destination samples overlap (sample stride %lld)", dst_sample_stride);
  FinishArgs a;
  memset(&a, 0, sizeof(a));
  if (mode == UPK_FINISH_DENORM) {
    if (!denorm_host) return upk_fail(ctx, UPK_EINVAL, "image_finish: DENORM needs denorm_host");
    for (int c = 0; c < 3; ++c) {
      a.d[c] = denorm_host[c];
      a.m[c] = denorm_host[3 + c];
      if (!(a.d[c] != 0.0f) || a.d[c] - a.d[c] != 0.0f || a.m[c] - a.m[c] != 0.0f)
        return upk_fail(ctx, UPK_EINVAL, "image_finish: denorm_host[%d] must be finite and d non-zero", c);
    }
  }
  a.src = src, a.dst = dst, a.src_bs = batch > 1 ? src_batch_stride : 0, a.dst_bs = batch > 1 ? dst_sample_stride : 0;
  a.pitch = dst_pitch;
  a.src_h = src_h, a.src_w = src_w, a.top = top, a.left = left, a.crop_h = crop_h, a.crop_w = crop_w, a.dst_x = dst_x;
  a.nhwc = layout == UPK_LAYOUT_NHWC, a.mode = mode;
  // 16-byte loads: every (sample, row, 4-pixel group) of the window starts on a 16-byte boundary in both layouts;
  // dword stores: every group's 12 bytes start on a 4-byte boundary
  const bool vec = !((uintptr_t)src & 15) && !(a.src_bs & 3) && !(src_w & 3) && !(left & 3) && !(crop_w & 3) &&
                   !((uintptr_t)dst & 3) && !(a.dst_bs & 3) && !(dst_pitch & 3) && !(dst_x & 3);
  a.total = (long)batch * crop_h * (vec ? crop_w >> 2 : crop_w);
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_EINVAL, "image_finish: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  if (vec) {
    hipLaunchKernelGGL(image_finish_vec4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  } else {
    hipLaunchKernelGGL(image_finish_pixel_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  }
  return upk_check_launch(ctx, "image_finish");
}
