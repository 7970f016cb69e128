// Pose interpolation (app.py:280-308, "Interpolate"): the conditioning of all n frames of a sequence in one launch.
//
//   upk_pose_interp_f32   smpl_i = alpha_i * smpl_src + (1 - alpha_i) * smpl_dst and person_mask_i = the box picture of
//                         trunc(alpha_i * box(src) + (1 - alpha_i) * box(dst)), for every alpha of a DEVICE array
//
// The results are specified one correctly rounded IEEE operation at a time (include/upk.h): the box blend in
// fp64 and the SMPL blend in fp32, neither with a fused multiply-add, 1 - alpha in fp64 for both.  The truncation of the
// box blend is sensitive to exactly that (0.05 * 3 + 0.95 * 3 = 2.9999999999999996 -> row 2), hence the explicit
// __d*_rn / __f*_rn calls, the pragma below and -ffp-contract=off (build.py FILE_FLAGS).
#pragma clang fp contract(off)
// Launch-bound: a 32 x 24 map is 3 KB, so every workgroup (one per frame) finds the boxes of both maps again rather
// than wait for a second launch; the reduction is integer minima and maxima in LDS, as in cond_bbox_kernel (batch.hip).
#include "common.h"

namespace {

constexpr int PI_THREADS = 256;
constexpr float PI_BG = -1.0f, PI_FG = -0.99215686f;  // t(0), t(1) with t(u) = fl(fl(u / 255) * 2 - 1)

struct PoseArgs {
  const float *src_mask, *dst_mask, *src_smpl, *dst_smpl;
  const double* alphas;
  float *mask_out, *smpl_out;
  int32_t* boxes;
  int h, w, d;
};

__device__ __forceinline__ bool occupied(float v) { return v != -1.0f && v != 0.0f; }

__device__ __forceinline__ int blend(double a, double b, int s, int d) {
  return (int)__dadd_rn(__dmul_rn(a, (double)s), __dmul_rn(b, (double)d));
}

// one workgroup per frame
__global__ __launch_bounds__(PI_THREADS) void pose_interp_kernel(const PoseArgs a) {
  __shared__ int red[8];  // r0, r1, c0, c1 of src, then of dst
  const int f = blockIdx.x;
  if (threadIdx.x < 8) red[threadIdx.x] = (threadIdx.x & 1) ? -1 : 0x7fffffff;
  __syncthreads();
  const int hw = a.h * a.w;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float* s = m ? a.dst_mask : a.src_mask;
    int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
    for (int i = threadIdx.x; i < hw; i += PI_THREADS) {
      if (!occupied(s[i])) continue;
      const int y = i / a.w, x = i - y * a.w;
      r0 = min(r0, y), r1 = max(r1, y), c0 = min(c0, x), c1 = max(c1, x);
    }
    if (r1 >= 0)
      atomicMin(&red[4 * m], r0), atomicMax(&red[4 * m + 1], r1), atomicMin(&red[4 * m + 2], c0), atomicMax(&red[4 * m + 3], c1);
  }
  __syncthreads();
  const bool any = red[1] >= 0 && red[5] >= 0;  // a map without an occupied element: every frame is background
  if (a.boxes && f == 0 && threadIdx.x < 8) a.boxes[threadIdx.x] = red[(threadIdx.x & 4) + 1] >= 0 ? red[threadIdx.x] : -1;
  const double alpha = a.alphas[f];
  const double beta = __dsub_rn(1.0, alpha);
  int R0 = -1, R1 = -1, C0 = -1, C1 = -1;
  if (any) {  // lower bounds clamped to [0, size], upper bounds to [-1, size - 1]: a box outside the map stays empty
    R0 = min(max(blend(alpha, beta, red[0], red[4]), 0), a.h), R1 = min(max(blend(alpha, beta, red[1], red[5]), -1), a.h - 1);
    C0 = min(max(blend(alpha, beta, red[2], red[6]), 0), a.w), C1 = min(max(blend(alpha, beta, red[3], red[7]), -1), a.w - 1);
  }
  if (a.boxes && threadIdx.x < 4) a.boxes[8 + 4L * f + threadIdx.x] = threadIdx.x == 0 ? R0 : threadIdx.x == 1 ? R1 : threadIdx.x == 2 ? C0 : C1;
  float* out = a.mask_out + (long)f * hw;
  for (int i = threadIdx.x; i < hw; i += PI_THREADS) {
    const int y = i / a.w, x = i - y * a.w;
    out[i] = (any && y >= R0 && y <= R1 && x >= C0 && x <= C1) ? PI_FG : PI_BG;
  }
  const float a32 = (float)alpha, b32 = (float)beta;
  float* so = a.smpl_out + (long)f * a.d;
  for (int i = threadIdx.x; i < a.d; i += PI_THREADS)
    so[i] = __fadd_rn(__fmul_rn(a32, a.src_smpl[i]), __fmul_rn(b32, a.dst_smpl[i]));
}

inline bool overlap(const void* p, long long pb, const void* q, long long qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

}  // namespace

extern "C" int upk_pose_interp_f32(upk_ctx* ctx, const float* src_mask, const float* dst_mask, int h, int w,
                                   const float* src_smpl, const float* dst_smpl, int d, const double* alphas, int n,
                                   float* mask_out, float* smpl_out, int32_t* boxes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!src_mask || !dst_mask || !src_smpl || !dst_smpl || !alphas || !mask_out || !smpl_out)
    return upk_fail(ctx, UPK_EINVAL, "pose_interp: null pointer");
  if (h <= 0 || w <= 0 || d <= 0 || n <= 0) return upk_fail(ctx, UPK_EINVAL, "pose_interp: sizes must be positive");
  if ((((uintptr_t)src_mask | (uintptr_t)dst_mask | (uintptr_t)src_smpl | (uintptr_t)dst_smpl | (uintptr_t)mask_out |
        (uintptr_t)smpl_out | (uintptr_t)boxes) & 3) || ((uintptr_t)alphas & 7))
    return upk_fail(ctx, UPK_EINVAL, "pose_interp: fp32 / int32 pointers must be 4-byte aligned, alphas 8-byte aligned");
  if ((long long)h * w > 0x7fffffffLL) return upk_fail(ctx, UPK_ESHAPE, "pose_interp: a map of more than 2^31 - 1 elements");
  if (n > 65535) return upk_fail(ctx, UPK_ESHAPE, "pose_interp: %d frames above 65535", n);
  const long long hw = (long long)h * w;
  const void* in[5] = {src_mask, dst_mask, src_smpl, dst_smpl, alphas};
  const long long in_b[5] = {4 * hw, 4 * hw, 4LL * d, 4LL * d, 8LL * n};
  const void* out[3] = {mask_out, smpl_out, boxes};
  const long long out_b[3] = {4 * hw * n, 4LL * d * n, boxes ? 16LL * (n + 2) : 0};
  for (int o = 0; o < 3; ++o) {
    if (!out[o]) continue;
    for (int i = 0; i < 5; ++i)
      if (overlap(out[o], out_b[o], in[i], in_b[i])) return upk_fail(ctx, UPK_EINVAL, "pose_interp: an output aliases an input");
    for (int p = o + 1; p < 3; ++p)
      if (out[p] && overlap(out[o], out_b[o], out[p], out_b[p])) return upk_fail(ctx, UPK_EINVAL, "pose_interp: two outputs overlap");
  }
  PoseArgs a;
  memset(&a, 0, sizeof(a));
  a.src_mask = src_mask, a.dst_mask = dst_mask, a.src_smpl = src_smpl, a.dst_smpl = dst_smpl, a.alphas = alphas;
  a.mask_out = mask_out, a.smpl_out = smpl_out, a.boxes = boxes;
  a.h = h, a.w = w, a.d = d;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(pose_interp_kernel, dim3((unsigned)n), dim3(PI_THREADS), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "pose_interp");
}
