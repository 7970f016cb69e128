// LPIPS (VGG16) around upk_conv2d_nhwc_f16: what scripts/eval_metrics.py:112 gets from lpips.LPIPS(net='vgg') needs, next
// to the 13 convolutions, three memory-bound passes (the algorithm is stated in include/upk.h):
//   upk_lpips_input_f16     pictures (uint8 HWC windows or fp32 NCHW) -> the scaling layer's output as fp16 NHWC, 32 channels
//   upk_relu_pool_nhwc_f16  ReLU in place and, for the last conv of a slice, the 2x2 floor max-pool behind it
//   upk_lpips_layer_f16     one tap: per-pixel channel normalisation, weighted squared distance, mean over pixels
//
// The input values are specified operation by operation (bit for bit torch's fp32 expression followed by .half()): no
// mul + sub may be contracted into an FMA.  build.py's FILE_FLAGS gives this file -ffp-contract=off; it says so itself for
// whoever compiles it another way (the layer kernel's result does not depend on it beyond its error bound):
#pragma clang fp contract(off)
#include "common.h"

namespace {

// ---------------------------------------------------------------- input
struct InputArgs {
  const void* src;
  f16* y;
  long pitch, ss;  // u8: bytes between rows / samples; f32: ss = floats between samples
  long ys;         // elements between the outputs of consecutive samples
  long total;      // batch * h * w * 4 (four 16-byte pieces per pixel)
  int h, w, f32, normalize;
  float shift[3], scale[3];
};

// one thread per 16-byte piece of an output pixel: piece 0 holds the three channels, pieces 1..3 are zero
__global__ __launch_bounds__(256) void lpips_input_kernel(const InputArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int q = (int)(idx & 3);
  const long pix = idx >> 2;
  f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  const int x = (int)(pix % a.w);
  const long r = pix / a.w;
  const int y = (int)(r % a.h);
  const long n = r / a.h;
  if (q == 0) {
    float v[3];
    if (a.f32) {
      const float* s = (const float*)a.src + n * a.ss + (long)y * a.w + x;
      const long plane = (long)a.h * a.w;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = s[c * plane];
    } else {
      const uint8_t* s = (const uint8_t*)a.src + n * a.ss + (long)y * a.pitch + 3L * x;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)s[c], 255.0f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t = v[c];
      if (a.normalize) t = __fsub_rn(__fmul_rn(2.0f, t), 1.0f);
      o[c] = (f16)__fdiv_rn(__fsub_rn(t, a.shift[c]), a.scale[c]);
    }
  }
  *(f16x8*)(a.y + n * a.ys + ((long)y * a.w + x) * 32 + 8 * q) = o;
}

// ---------------------------------------------------------------- ReLU (+ 2x2 floor max-pool)
struct ReluArgs {
  f16* x;
  f16* pooled;
  long total;  // batch * ceil(h / 2) * ceil(w / 2) * (c / 8)
  int h, w, h2c, w2c, c8, ld, ld_p;
};

// one thread per (2x2 pixel block, 8 channels): up to four 16-byte loads, the same stores, one pooled store.  The blocks
// of an odd last row / column hold one or two pixels and write no pooled value (floor).
__global__ __launch_bounds__(256) void relu_pool_kernel(const ReluArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int cg = (int)(idx % a.c8);
  long r = idx / a.c8;
  const int bx = (int)(r % a.w2c);
  r /= a.w2c;
  const int by = (int)(r % a.h2c);
  const long n = r / a.h2c;
  const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 m = zero;
  const int y0 = 2 * by, x0 = 2 * bx;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      if (y0 + dy < a.h && x0 + dx < a.w) {
        f16x8* p = (f16x8*)(a.x + ((n * a.h + y0 + dy) * a.w + x0 + dx) * a.ld + 8 * cg);
        f16x8 v = *p;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] > (f16)0 ? v[j] : (f16)0;
        *p = v;
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
      }
    }
  const int h2 = a.h >> 1, w2 = a.w >> 1;
  if (a.pooled && by < h2 && bx < w2) *(f16x8*)(a.pooled + ((n * h2 + by) * w2 + bx) * a.ld_p + 8 * cg) = m;
}

// ---------------------------------------------------------------- one tap
constexpr int LW = 4;       // waves per workgroup
constexpr int LITER = 8;    // loads per wave and picture
constexpr float LEPS = 1e-10f;

struct LayerArgs {
  const f16* f0;
  const f16* f1;
  const float* w;
  float* part;  // [n][slots]
  long bs;  // elements between consecutive pairs of f0 (and of f1)
  int hw, c, ld, slots;
};

static inline int layer_pix_per_wg(int c) { return LW * LITER * (512 / c); }

// A wave covers 512 channels with one 16-byte load per lane: 512 / c pixels side by side, c / 8 lanes per pixel.  A lane
// keeps its eight weights in registers; the two squared norms of a pixel are summed over its lanes with xor shuffles
// (every lane of the pixel gets them), the lane then adds w (f0 / (n0 + eps) - f1 / (n1 + eps))^2 of its eight channels to
// its own accumulator.  The accumulators are summed over the wave, then over the four waves in a fixed order, into the
// workgroup's OWN slot: no atomics.  Pixels past hw load nothing and add exactly 0 (0 / (0 + eps) = 0).
__global__ __launch_bounds__(LW * 64) void lpips_layer_kernel(const LayerArgs a) {
  __shared__ float s_red[LW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n = blockIdx.x / a.slots;
  const int slot = blockIdx.x % a.slots;
  const int lpp = a.c >> 3, ppw = 64 / lpp;  // lanes per pixel, pixels per wave and load
  const int g = lane / lpp, coff = (lane % lpp) * 8;
  float wt[8];
  {
    const f32x4 w0 = *(const f32x4*)(a.w + coff), w1 = *(const f32x4*)(a.w + coff + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) wt[j] = w0[j], wt[4 + j] = w1[j];
  }
  const f16* b0 = a.f0 + n * a.bs + coff;
  const f16* b1 = a.f1 + n * a.bs + coff;
  const long base = (long)slot * (LW * LITER * ppw);
  float acc = 0.0f;
#pragma unroll 2
  for (int it = 0; it < LITER; ++it) {
    const long p = base + (long)(it * LW + wave) * ppw + g;
    float x0[8], x1[8];
    if (p < a.hw) {
      const f16x8 v0 = *(const f16x8*)(b0 + p * a.ld), v1 = *(const f16x8*)(b1 + p * a.ld);
#pragma unroll
      for (int j = 0; j < 8; ++j) x0[j] = (float)v0[j], x1[j] = (float)v1[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x0[j] = 0.0f, x1[j] = 0.0f;
    }
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s0 += x0[j] * x0[j], s1 += x1[j] * x1[j];
    for (int off = lpp >> 1; off >= 1; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
    }
    const float n0 = __fsqrt_rn(s0) + LEPS, n1 = __fsqrt_rn(s1) + LEPS;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = __fdiv_rn(x0[j], n0) - __fdiv_rn(x1[j], n1);
      acc += wt[j] * (d * d);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) s_red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[n * a.slots + slot] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

struct LayerFinalArgs {
  const float* part;
  float* out;
  double inv_hw;
  int slots, out_stride, layer;
};

// one wave per sample: lane i sums slots i, i + 64, ... in fp64, then a shuffle tree; always the same order
__global__ __launch_bounds__(64) void lpips_final_kernel(const LayerFinalArgs a) {
  const long n = blockIdx.x;
  const float* part = a.part + n * a.slots;
  double s = 0.0;
  for (int i = threadIdx.x; i < a.slots; i += 64) s += (double)part[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) a.out[n * a.out_stride + a.layer] = (float)(s * a.inv_hw);
}

bool layer_c_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

}  // namespace

extern "C" int upk_lpips_input_f16(upk_ctx* ctx, const void* src, int src_f32, long long pitch, long long sample_stride,
                                   int batch, int h, int w, int normalize, const float* shift_scale_host, void* y,
                                   long long y_sample_stride, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!src || !y || !shift_scale_host) return upk_fail(ctx, UPK_EINVAL, "lpips_input: null pointer");
  if (batch <= 0 || h <= 0 || w <= 0) return upk_fail(ctx, UPK_EINVAL, "lpips_input: sizes must be positive");
  if (((uintptr_t)y & 15) || (y_sample_stride & 7)) return upk_fail(ctx, UPK_EINVAL, "lpips_input: y is not 16-byte aligned");
  if (batch > 1 && y_sample_stride < 32LL * h * w)
    return upk_fail(ctx, UPK_EINVAL, "lpips_input: outputs overlap (y sample stride %lld elements)", y_sample_stride);
  if (src_f32) {
    if ((uintptr_t)src & 3) return upk_fail(ctx, UPK_EINVAL, "lpips_input: fp32 src is not 4-byte aligned");
    if (batch > 1 && sample_stride < 3LL * h * w)
      return upk_fail(ctx, UPK_EINVAL, "lpips_input: samples overlap (sample stride %lld floats)", sample_stride);
  } else {
    if (pitch < 3LL * w) return upk_fail(ctx, UPK_EINVAL, "lpips_input: row pitch %lld below 3 * w = %lld bytes", pitch, 3LL * w);
    if (batch > 1 && sample_stride < (h - 1) * pitch + 3LL * w)
      return upk_fail(ctx, UPK_EINVAL, "lpips_input: samples overlap (sample stride %lld)", sample_stride);
  }
  InputArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < 3; ++c) {
    a.shift[c] = shift_scale_host[c];
    a.scale[c] = shift_scale_host[3 + c];
    if (!(a.scale[c] != 0.0f) || a.scale[c] - a.scale[c] != 0.0f || a.shift[c] - a.shift[c] != 0.0f)
      return upk_fail(ctx, UPK_EINVAL, "lpips_input: shift / scale of channel %d must be finite and scale non-zero", c);
  }
  a.src = src, a.y = (f16*)y, a.pitch = pitch, a.ss = batch > 1 ? sample_stride : 0;
  a.ys = batch > 1 ? y_sample_stride : 0;
  a.h = h, a.w = w, a.f32 = src_f32 != 0, a.normalize = normalize != 0;
  a.total = (long)batch * h * w * 4;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "lpips_input: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "lpips_input");
}

extern "C" int upk_relu_pool_nhwc_f16(upk_ctx* ctx, void* x, int ld, int batch, int h, int w, int c, void* pooled, int ld_p,
                                      upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x) return upk_fail(ctx, UPK_EINVAL, "relu_pool: null pointer");
  if (batch <= 0 || h <= 0 || w <= 0 || c <= 0) return upk_fail(ctx, UPK_EINVAL, "relu_pool: sizes must be positive");
  if (c % 8) return upk_fail(ctx, UPK_ESHAPE, "relu_pool: c = %d is not a multiple of 8", c);
  if (ld < c || ld % 8 || ((uintptr_t)x & 15))
    return upk_fail(ctx, UPK_EINVAL, "relu_pool: x needs 16-byte aligned rows of at least c elements (ld = %d)", ld);
  if (pooled) {
    if (h < 2 || w < 2) return upk_fail(ctx, UPK_ESHAPE, "relu_pool: a %d x %d map has no 2x2 pooled output", h, w);
    if (ld_p < c || ld_p % 8 || ((uintptr_t)pooled & 15))
      return upk_fail(ctx, UPK_EINVAL, "relu_pool: pooled needs 16-byte aligned rows of at least c elements (ld_p = %d)", ld_p);
  }
  ReluArgs a;
  a.x = (f16*)x, a.pooled = (f16*)pooled;
  a.h = h, a.w = w, a.h2c = (h + 1) / 2, a.w2c = (w + 1) / 2, a.c8 = c / 8, a.ld = ld, a.ld_p = ld_p;
  a.total = (long)batch * a.h2c * a.w2c * a.c8;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "relu_pool: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(relu_pool_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "relu_pool");
}

extern "C" size_t upk_lpips_ws_bytes(int n, int hw, int c) {
  if (n <= 0 || hw <= 0 || !layer_c_ok(c)) return 0;
  const long slots = ((long)hw + layer_pix_per_wg(c) - 1) / layer_pix_per_wg(c);
  if (slots * n > 0x7fffffffL) return 0;
  return ((size_t)n * slots * sizeof(float) + 15) / 16 * 16;
}

extern "C" int upk_lpips_layer_f16(upk_ctx* ctx, const void* f0, const void* f1, int ld, long long batch_stride, int n, int hw, int c,
                                   const float* w, int layer, float* out, void* ws, size_t ws_bytes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!f0 || !f1 || !w || !out || !ws) return upk_fail(ctx, UPK_EINVAL, "lpips_layer: null pointer");
  if (n <= 0 || hw <= 0) return upk_fail(ctx, UPK_EINVAL, "lpips_layer: sizes must be positive");
  if (layer < 0 || layer > 4) return upk_fail(ctx, UPK_EINVAL, "lpips_layer: layer = %d, must be 0 .. 4", layer);
  if (!layer_c_ok(c)) return upk_fail(ctx, UPK_ESHAPE, "lpips_layer: c = %d, must be 64, 128, 256 or 512", c);
  if (ld < c || ld % 8 || ((uintptr_t)f0 & 15) || ((uintptr_t)f1 & 15))
    return upk_fail(ctx, UPK_EINVAL, "lpips_layer: features need 16-byte aligned rows of at least c elements (ld = %d)", ld);
  if (n > 1 && (batch_stride < (long long)hw * ld || (batch_stride & 7)))
    return upk_fail(ctx, UPK_EINVAL, "lpips_layer: batch stride %lld below hw * ld or not a multiple of 8", batch_stride);
  if (((uintptr_t)w & 15) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 15))
    return upk_fail(ctx, UPK_EINVAL, "lpips_layer: w / ws must be 16-byte and out 4-byte aligned");
  const size_t need = upk_lpips_ws_bytes(n, hw, c);
  if (!need) return upk_fail(ctx, UPK_ESHAPE, "lpips_layer: %d samples of %d pixels are too many workgroups", n, hw);
  if (ws_bytes < need) return upk_fail(ctx, UPK_EWORKSPACE, "lpips_layer: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  LayerArgs a;
  a.f0 = (const f16*)f0, a.f1 = (const f16*)f1, a.w = w, a.part = (float*)ws;
  a.hw = hw, a.c = c, a.ld = ld, a.bs = n > 1 ? batch_stride : 0;
  a.slots = (hw + layer_pix_per_wg(c) - 1) / layer_pix_per_wg(c);
  hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)((long)n * a.slots)), dim3(LW * 64), 0, stream, a);
  int e = upk_check_launch(ctx, "lpips_layer");
  if (e != UPK_OK) return e;
  LayerFinalArgs fa;
  fa.part = a.part, fa.out = out, fa.inv_hw = 1.0 / (double)hw, fa.slots = a.slots, fa.out_stride = 5, fa.layer = layer;
  hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)n), dim3(64), 0, stream, fa);
  return upk_check_launch(ctx, "lpips_final");
}
