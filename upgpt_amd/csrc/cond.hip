// Kernels of the CLIPTextImageCrossAtten conditioning stage (include/upk.h):
//   upk_attention_fewkeys_f16   softmax(Q K^T * scale) V over 1 .. 16 keys, any head dim that is a multiple of 8
//   upk_gelu_f16                exact (erf) GELU in place, the activation of a CLIP MLP with hidden_act "gelu"
// Both run once per batch (not once per sampler step) and are VALU kernels: with 9 keys an MFMA tile of 32 keys would
// be 72 % padding, and the whole K | V of a head (at most 2 x 16 x 128 fp16 = 8 KB) fits a corner of the LDS.
#include "common.h"

namespace {

constexpr int FK_MAX_KV = 16;
constexpr int FK_MAX_D = 128;
constexpr int FK_ROWS = 64;  // queries per workgroup = one wave, one lane per query

// grid (query tiles, heads, batch), 64 threads.  K and V of (sample, head) are staged once in LDS, rows d apart; every
// lane then reads the SAME 16-byte chunk of a key row at a time (identical addresses broadcast: no bank conflict),
// against its own q row, which it reads from memory 16 bytes at a time.  Scores, softmax and the P V sums are fp32;
// P V goes 8 channels at a time so that the accumulators stay at 8 registers whatever d is.
__global__ __launch_bounds__(FK_ROWS) void attention_fewkeys_kernel(
    const f16* __restrict__ q, int ldq, long qbs, const f16* __restrict__ k, int ldk, long kbs,
    const f16* __restrict__ v, int ldv, long vbs, f16* __restrict__ out, int ldo, long obs, int n_q, int n_kv, int d,
    float scale) {
  __shared__ __attribute__((aligned(16))) f16 ks[FK_MAX_KV * FK_MAX_D];
  __shared__ __attribute__((aligned(16))) f16 vs[FK_MAX_KV * FK_MAX_D];
  const int h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x;
  const int cpr = d >> 3;  // 16-byte chunks per row
  const f16* kb = k + (long)b * kbs + (long)h * d;
  const f16* vb = v + (long)b * vbs + (long)h * d;
  for (int c = lane; c < n_kv * cpr; c += FK_ROWS) {
    const int j = c / cpr, cc = c - j * cpr;
    *(f16x8*)(ks + j * d + cc * 8) = *(const f16x8*)(kb + (long)j * ldk + cc * 8);
    *(f16x8*)(vs + j * d + cc * 8) = *(const f16x8*)(vb + (long)j * ldv + cc * 8);
  }
  __syncthreads();
  const int row = blockIdx.x * FK_ROWS + lane;
  if (row >= n_q) return;  // (after the only barrier)
  const f16* qr = q + (long)b * qbs + (long)row * ldq + (long)h * d;
  float s[FK_MAX_KV];
#pragma unroll
  for (int j = 0; j < FK_MAX_KV; ++j) s[j] = 0.0f;
  for (int cc = 0; cc < cpr; ++cc) {
    const f16x8 qv = *(const f16x8*)(qr + cc * 8);
    float qf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = (float)qv[e];
#pragma unroll
    for (int j = 0; j < FK_MAX_KV; ++j) {
      if (j < n_kv) {  // (uniform)
        const f16x8 kv = *(const f16x8*)(ks + j * d + cc * 8);
        float a = s[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(qf[e], (float)kv[e], a);
        s[j] = a;
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < FK_MAX_KV; ++j) {
    s[j] *= scale;
    if (j < n_kv) m = fmaxf(m, s[j]);
  }
  float sum = 0.0f;
#pragma unroll
  for (int j = 0; j < FK_MAX_KV; ++j) {
    s[j] = j < n_kv ? __expf(s[j] - m) : 0.0f;  // (the maximum's own term is exp(0) = 1: sum >= 1)
    sum += s[j];
  }
  const float inv = 1.0f / sum;
  f16* orow = out + (long)b * obs + (long)row * ldo + (long)h * d;
  for (int cc = 0; cc < cpr; ++cc) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < FK_MAX_KV; ++j) {
      if (j < n_kv) {
        const f16x8 vv = *(const f16x8*)(vs + j * d + cc * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(s[j], (float)vv[e], acc[e]);
      }
    }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)(acc[e] * inv);
    *(f16x8*)(orow + cc * 8) = o;
  }
}

// in place over [rows, cols] fp16, rows ld apart: one thread per 8 channels, grid-stride.  upk_geglu_mul(1, x) is the
// GELU of the GEGLU epilogues (common.h) with a value of one: the two activations agree bit for bit.
__global__ void gelu_kernel(f16* x, int ld, int vpr, long total) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const long r = i / vpr;
    const int c = (int)(i - r * vpr);
    f16x8* p = (f16x8*)(x + r * ld + c * 8);
    const f16x8 a = *p;
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)upk_geglu_mul(1.0f, (float)a[e]);
    *p = o;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int upk_attention_fewkeys_f16(upk_ctx* ctx, const void* q, int ldq, long long qbs, const void* k, int ldk,
                                         long long kbs, const void* v, int ldv, long long vbs, void* out, int ldo,
                                         long long obs, int batch, int heads, int n_q, int n_kv, int d, float scale,
                                         upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!q || !k || !v || !out) return upk_fail(ctx, UPK_EINVAL, "attention_fewkeys: null pointer");
  if (n_kv < 1 || n_kv > FK_MAX_KV || d < 8 || d > FK_MAX_D || (d & 7) || n_q < 1 || batch < 1 || heads < 1 ||
      heads > 65535 || batch > 65535)
    return upk_fail(ctx, UPK_ESHAPE, "attention_fewkeys: needs 1 <= n_kv <= %d, 8 <= d <= %d with d %% 8 == 0, n_q >= 1 "
                    "(got n_kv %d, d %d, n_q %d, heads %d, batch %d)", FK_MAX_KV, FK_MAX_D, n_kv, d, n_q, heads, batch);
  const long hd = (long)heads * d;
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 7) || ldq < hd || ldk < hd || ldv < hd || ldo < hd)
    return upk_fail(ctx, UPK_ESHAPE, "attention_fewkeys: leading dimensions must be multiples of 8 and >= heads * d = %ld "
                    "(got q %d, k %d, v %d, out %d)", hd, ldq, ldk, ldv, ldo);
  if ((qbs & 7) || (kbs & 7) || (vbs & 7) || (obs & 7) || !al16(q) || !al16(k) || !al16(v) || !al16(out))
    return upk_fail(ctx, UPK_ESHAPE, "attention_fewkeys: pointers and batch strides must be 16-byte aligned");
  upk_prof_scope prof(ctx, UPK_CLS_ATTN, (hipStream_t)stream_);
  hipLaunchKernelGGL(attention_fewkeys_kernel, dim3((unsigned)((n_q + FK_ROWS - 1) / FK_ROWS), heads, batch), dim3(FK_ROWS),
                     0, (hipStream_t)stream_, (const f16*)q, ldq, (long)qbs, (const f16*)k, ldk, (long)kbs, (const f16*)v,
                     ldv, (long)vbs, (f16*)out, ldo, (long)obs, n_q, n_kv, d, scale);
  return upk_check_launch(ctx, "attention_fewkeys");
}

extern "C" int upk_gelu_f16(upk_ctx* ctx, void* x, int ld, int rows, int cols, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x) return upk_fail(ctx, UPK_EINVAL, "gelu: null pointer");
  if (rows < 1 || cols < 8 || (cols & 7) || (ld & 7) || ld < cols || !al16(x))
    return upk_fail(ctx, UPK_ESHAPE, "gelu: cols and ld must be multiples of 8 with ld >= cols, x 16-byte aligned "
                    "(got rows %d, cols %d, ld %d)", rows, cols, ld);
  const int vpr = cols >> 3;
  const long total = (long)rows * vpr;
  long blocks = (total + 255) / 256;
  const long cap = (long)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
  if (blocks > cap) blocks = cap;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, (f16*)x, ld, vpr, total);
  return upk_check_launch(ctx, "gelu");
}
