// The per-pixel work of the test split's loader (DeepFashionPair.__getitem__, deepfashion_inshop.py:173-272) on the bytes PIL
// decoded: batch['person_mask'], batch['loss_w'] and batch['styles'] from uint8 maps and stored crops.
//
//   upk_cond_bbox_u8      get_bbox + mask_transform: the bounding box of the non-zero bytes of a map, then Pillow's NEAREST
//                         resize of the box picture and t = fl(fl(u / 255) * 2 - 1) with u = 1 inside, 0 outside
//   upk_cond_gather_u8    mask_transform / loss_w_transform: out = lut[map[ytab[y]][xtab[x]]], a 256-entry fp32 table
//   upk_cond_smpl_u8      the `smpl` mask_transform after the bilinear resize: torch.mean(x, 0) * 2. - 1.
//   upk_clip_normalize_u8 clip_transform of a stored 224 x 224 crop: HWC bytes -> CHW fp32, (u / 255 - mean) / std
//
// Every fp32 result is specified one correctly rounded IEEE operation at a time (include/upk.h), hence the explicit
// __f*_rn calls, the pragma below and -ffp-contract=off (build.py FILE_FLAGS): no FMA, no reciprocal multiply.
#pragma clang fp contract(off)
// All four are launch- or memory-bound.  Only upk_clip_normalize_u8 moves real bytes (72 crops: 10.8 MB in, 43 MB out):
// a workgroup stages 8 rows of a crop in LDS with 16-byte loads of the interleaved bytes, then every lane takes 4 adjacent
// pixels = 3 aligned LDS dwords (lane stride 3 dwords: odd, so the 64 banks are hit once each) and writes one 16-byte
// float4 into each of the three planes; adjacent lanes write adjacent float4s, 1 KB per wave and plane.
#include "common.h"

namespace {

constexpr int BB_THREADS = 512;
constexpr int CM_THREADS = 256;
constexpr int CN_THREADS = 256;
constexpr int CN_ROWS = 8;                // rows of a crop per workgroup (224 = 28 tiles)
constexpr int CN_LDS_BYTES = 64 * 1024;   // staging budget of the vector path

// ToTensor and x * 2. - 1. of a byte
__device__ __forceinline__ float mask_value(uint32_t u) {
  return __fsub_rn(__fmul_rn(__fdiv_rn((float)u, 255.0f), 2.0f), 1.0f);
}

struct BoxMapArgs {
  const uint8_t* src;
  const int32_t *ytab, *xtab;
  float* dst;
  int32_t* boxes;
  long pitch, ss;
  int h, w, oh, ow, vec;
};

// one workgroup per map: rows / columns holding a non-zero byte -> LDS minima and maxima (integers: no order to depend
// on), a barrier, then the map's oh x ow outputs
__global__ __launch_bounds__(BB_THREADS) void cond_bbox_kernel(const BoxMapArgs a) {
  __shared__ int red[4];  // r0, r1, c0, c1
  const int b = blockIdx.x;
  if (threadIdx.x < 4) red[threadIdx.x] = (threadIdx.x & 1) ? -1 : 0x7fffffff;
  __syncthreads();
  const uint8_t* s = a.src + (long)b * a.ss;
  int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
  if (a.vec) {  // 16 bytes per lane and trip (w, pitch, sample stride and base multiples of 16)
    const int cpr = a.w >> 4;
    for (int i = threadIdx.x; i < a.h * cpr; i += BB_THREADS) {
      const int y = i / cpr, cx = i - y * cpr;
      const uint4 v = *(const uint4*)(s + (long)y * a.pitch + 16L * cx);
      if (!(v.x | v.y | v.z | v.w)) continue;
      r0 = min(r0, y), r1 = max(r1, y);
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if ((d[j >> 2] >> (8 * (j & 3))) & 0xffu) c0 = min(c0, 16 * cx + j), c1 = max(c1, 16 * cx + j);
    }
  } else {
    for (int i = threadIdx.x; i < a.h * a.w; i += BB_THREADS) {
      const int y = i / a.w, x = i - y * a.w;
      if (!s[(long)y * a.pitch + x]) continue;
      r0 = min(r0, y), r1 = max(r1, y), c0 = min(c0, x), c1 = max(c1, x);
    }
  }
  if (r1 >= 0) atomicMin(&red[0], r0), atomicMax(&red[1], r1), atomicMin(&red[2], c0), atomicMax(&red[3], c1);
  __syncthreads();
  const int R0 = red[0], R1 = red[1], C0 = red[2], C1 = red[3];
  const bool any = R1 >= 0;
  if (threadIdx.x < 4) a.boxes[4L * b + threadIdx.x] = any ? red[threadIdx.x] : -1;
  float* out = a.dst + (long)b * a.oh * a.ow;
  for (int i = threadIdx.x; i < a.oh * a.ow; i += BB_THREADS) {
    const int y = i / a.ow, x = i - y * a.ow;
    const int sy = a.ytab[y], sx = a.xtab[x];  // (compared only, never an address)
    const bool inside = any && sy >= R0 && sy <= R1 && sx >= C0 && sx <= C1;
    out[i] = mask_value(inside ? 1u : 0u);
  }
}

struct GatherArgs {
  const uint8_t* src;
  const int32_t *ytab, *xtab;
  float* dst;
  long pitch, ss;
  int h, w, oh, ow;
  float lut[256];
};

__global__ __launch_bounds__(CM_THREADS) void cond_gather_kernel(const GatherArgs a) {
  __shared__ float lut[256];
  const float* l = a.lut;
  lut[threadIdx.x] = l[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y;
  const uint8_t* s = a.src + (long)b * a.ss;
  float* out = a.dst + (long)b * a.oh * a.ow;
  for (int i = blockIdx.x * CM_THREADS + threadIdx.x; i < a.oh * a.ow; i += gridDim.x * CM_THREADS) {
    const int y = i / a.ow, x = i - y * a.ow;
    const int sy = min(max(a.ytab[y], 0), a.h - 1), sx = min(max(a.xtab[x], 0), a.w - 1);  // (validated by the caller)
    out[i] = lut[s[(long)sy * a.pitch + sx]];
  }
}

struct SmplArgs {
  const uint8_t* src;
  float* dst;
  long pitch, ss;
  int h, w;
};

// torch.mean(x, 0, keepdim=True) * 2. - 1. of x = ToTensor(picture): fl(fl(fl(fl(r + g) + b) / 3) * 2 - 1)
__global__ __launch_bounds__(CM_THREADS) void cond_smpl_kernel(const SmplArgs a) {
  const int b = blockIdx.y;
  const uint8_t* s = a.src + (long)b * a.ss;
  float* out = a.dst + (long)b * a.h * a.w;
  for (int i = blockIdx.x * CM_THREADS + threadIdx.x; i < a.h * a.w; i += gridDim.x * CM_THREADS) {
    const int y = i / a.w, x = i - y * a.w;
    const uint8_t* p = s + (long)y * a.pitch + 3L * x;
    const float r = __fdiv_rn((float)p[0], 255.0f), g = __fdiv_rn((float)p[1], 255.0f), bl = __fdiv_rn((float)p[2], 255.0f);
    const float m = __fdiv_rn(__fadd_rn(__fadd_rn(r, g), bl), 3.0f);
    out[i] = __fsub_rn(__fmul_rn(m, 2.0f), 1.0f);
  }
}

struct NormArgs {
  const uint8_t* src;
  const int32_t* valid;
  float* dst;
  long pitch, ss;
  int h, w, vec;
  float mean[3], std[3];
};

__device__ __forceinline__ float clip_value(const NormArgs& a, uint32_t u, int c) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), a.mean[c]), a.std[c]);
}

__global__ __launch_bounds__(CN_THREADS) void clip_norm_kernel(const NormArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  const int n = blockIdx.y;
  const int y0 = blockIdx.x * CN_ROWS;
  const int rows = min(CN_ROWS, a.h - y0);
  const bool ok = !a.valid || a.valid[n] != 0;  // uniform over the workgroup; an invalid crop's bytes are never read
  const uint8_t* s = a.src + (long)n * a.ss;
  float* out = a.dst + (long)n * 3 * a.h * a.w;
  if (a.vec) {
    const int row_bytes = 3 * a.w, cpr = row_bytes >> 4, wq = a.w >> 2;
    if (ok) {
      for (int i = threadIdx.x; i < rows * cpr; i += CN_THREADS) {
        const int r = i / cpr, c = i - r * cpr;
        *(uint4*)(stage + r * row_bytes + 16 * c) = *(const uint4*)(s + (long)(y0 + r) * a.pitch + 16L * c);
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < rows * wq; i += CN_THREADS) {
      const int r = i / wq, xq = i - r * wq;
      uint32_t u[12];  // pixel-major, channel-minor
#pragma unroll
      for (int j = 0; j < 12; ++j) u[j] = 0;
      if (ok) {
        const uint32_t* p = (const uint32_t*)(stage + r * row_bytes + 12 * xq);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint32_t v = p[q];
#pragma unroll
          for (int j = 0; j < 4; ++j) u[4 * q + j] = (v >> (8 * j)) & 0xffu;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = clip_value(a, u[3 * j + c], c);
        *(f32x4*)(out + ((long)c * a.h + y0 + r) * a.w + 4 * xq) = v;
      }
    }
  } else {
    for (int i = threadIdx.x; i < rows * a.w; i += CN_THREADS) {
      const int r = i / a.w, x = i - r * a.w;
      const uint8_t* p = s + (long)(y0 + r) * a.pitch + 3L * x;
#pragma unroll
      for (int c = 0; c < 3; ++c) out[((long)c * a.h + y0 + r) * a.w + x] = clip_value(a, ok ? p[c] : 0u, c);
    }
  }
}

int check_map(upk_ctx* ctx, const char* who, const uint8_t* src, long long pitch, long long row_bytes, int batch, int h, int w,
              int out_h, int out_w, const float* dst) {
  if (!src || !dst) return upk_fail(ctx, UPK_EINVAL, "%s: null source or destination", who);
  if (batch <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return upk_fail(ctx, UPK_EINVAL, "%s: sizes must be positive", who);
  if (pitch < row_bytes) return upk_fail(ctx, UPK_EINVAL, "%s: pitch %lld below the %lld bytes of a row", who, pitch, row_bytes);
  if ((uintptr_t)dst & 3) return upk_fail(ctx, UPK_EINVAL, "%s: the fp32 destination must be 4-byte aligned", who);
  if ((long long)h * w > 0x7fffffffLL || (long long)out_h * out_w > 0x7fffffffLL)
    return upk_fail(ctx, UPK_ESHAPE, "%s: a map of more than 2^31 - 1 pixels", who);
  if (batch > 65535) return upk_fail(ctx, UPK_ESHAPE, "%s: batch %d above 65535", who, batch);
  return UPK_OK;
}

unsigned blocks_for(long n, int threads) {
  const long b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : b > 64 ? 64 : b);
}

}  // namespace

extern "C" int upk_cond_bbox_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h,
                                int w, const int32_t* ytab, const int32_t* xtab, int out_h, int out_w, float* dst,
                                int32_t* boxes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_map(ctx, "cond_bbox", src, pitch, w, batch, h, w, out_h, out_w, dst);
  if (rc != UPK_OK) return rc;
  if (!ytab || !xtab || !boxes) return upk_fail(ctx, UPK_EINVAL, "cond_bbox: null index tables or boxes");
  if (((uintptr_t)ytab | (uintptr_t)xtab | (uintptr_t)boxes) & 3)
    return upk_fail(ctx, UPK_EINVAL, "cond_bbox: index tables and boxes must be 4-byte aligned");
  BoxMapArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src, a.ytab = ytab, a.xtab = xtab, a.dst = dst, a.boxes = boxes;
  a.pitch = pitch, a.ss = batch > 1 ? sample_stride : 0;
  a.h = h, a.w = w, a.oh = out_h, a.ow = out_w;
  a.vec = !(w & 15) && !(((uintptr_t)src | (uintptr_t)a.ss | (uintptr_t)pitch) & 15);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(cond_bbox_kernel, dim3((unsigned)batch), dim3(BB_THREADS), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "cond_bbox");
}

extern "C" int upk_cond_gather_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h,
                                  int w, const int32_t* ytab, const int32_t* xtab, int out_h, int out_w,
                                  const float* lut_host, float* dst, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_map(ctx, "cond_gather", src, pitch, w, batch, h, w, out_h, out_w, dst);
  if (rc != UPK_OK) return rc;
  if (!ytab || !xtab || !lut_host) return upk_fail(ctx, UPK_EINVAL, "cond_gather: null index tables or look-up table");
  if (((uintptr_t)ytab | (uintptr_t)xtab) & 3) return upk_fail(ctx, UPK_EINVAL, "cond_gather: index tables must be 4-byte aligned");
  GatherArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src, a.ytab = ytab, a.xtab = xtab, a.dst = dst;
  a.pitch = pitch, a.ss = batch > 1 ? sample_stride : 0;
  a.h = h, a.w = w, a.oh = out_h, a.ow = out_w;
  memcpy(a.lut, lut_host, sizeof(a.lut));
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(cond_gather_kernel, dim3(blocks_for((long)out_h * out_w, CM_THREADS), (unsigned)batch), dim3(CM_THREADS), 0,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "cond_gather");
}

extern "C" int upk_cond_smpl_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h,
                                int w, float* dst, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_map(ctx, "cond_smpl", src, pitch, 3LL * w, batch, h, w, h, w, dst);
  if (rc != UPK_OK) return rc;
  SmplArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src, a.dst = dst, a.pitch = pitch, a.ss = batch > 1 ? sample_stride : 0, a.h = h, a.w = w;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(cond_smpl_kernel, dim3(blocks_for((long)h * w, CM_THREADS), (unsigned)batch), dim3(CM_THREADS), 0,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "cond_smpl");
}

extern "C" int upk_clip_normalize_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride,
                                     const int32_t* valid, int n, int h, int w, const float* mean_std_host, float* dst,
                                     upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_map(ctx, "clip_normalize", src, pitch, 3LL * w, n, h, w, h, w, dst);
  if (rc != UPK_OK) return rc;
  if (!mean_std_host) return upk_fail(ctx, UPK_EINVAL, "clip_normalize: null constants");
  if ((uintptr_t)valid & 3) return upk_fail(ctx, UPK_EINVAL, "clip_normalize: valid must be 4-byte aligned");
  for (int c = 0; c < 3; ++c)
    if (!(mean_std_host[3 + c] > 0.0f)) return upk_fail(ctx, UPK_EINVAL, "clip_normalize: std[%d] must be positive", c);
  NormArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src, a.valid = valid, a.dst = dst, a.pitch = pitch, a.ss = n > 1 ? sample_stride : 0, a.h = h, a.w = w;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean_std_host[c], a.std[c] = mean_std_host[3 + c];
  // 16-byte loads of whole rows and 16-byte stores of 4 floats per plane: every row, sample and plane stays aligned
  const long stage = (long)CN_ROWS * 3 * w;
  a.vec = !(w & 15) && stage <= CN_LDS_BYTES && !(((uintptr_t)src | (uintptr_t)a.ss | (uintptr_t)pitch | (uintptr_t)dst) & 15);
  const size_t lds = a.vec ? (size_t)stage : 0;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(clip_norm_kernel, dim3((unsigned)((h + CN_ROWS - 1) / CN_ROWS), (unsigned)n), dim3(CN_THREADS), lds,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "clip_normalize");
}
