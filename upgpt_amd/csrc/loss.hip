// The denoising loss around one UNet forward (ddpm.py:1083-1123 of the reference): upk_q_sample_f32 noises the batch with
// one timestep per sample and writes the UNet stem input; upk_p_losses_f32 turns model output and target into the per-sample
// and batch loss values.  Arithmetic, layouts and error codes are stated in include/upk.h.  This file is compiled with
// -ffp-contract=off: every fp32 operation below is one IEEE operation, as torch evaluates the reference's expressions.
//
// q_sample_kernel   one thread per 4 consecutive elements of the flat [B * C * HW] tensors (16-byte loads and stores) plus
//                   one thread per element of the n % 4 tail; without 16-byte aligned pointers every element is a tail
//                   element.  A group may cross a channel or a sample: (sample, channel, pixel) walk along with it.
// q_sample_keyed_kernel  upk_q_sample_keyed_f32: a workgroup takes KTILE = 1024 consecutive elements of ONE sample per turn
//                   and walks the (sample, tile) pairs grid-stride; thread t owns quad e / 4 = tile * 256 + t of the sample,
//                   makes its Philox call and the two Box-Muller pairs (philox.h: the device functions of rng.hip) and
//                   noises its four elements.  Nothing of the launch, the batch or the addresses enters a value.  The
//                   sample is uniform over the workgroup, so its key, its timestep (the Philox call of STREAM_TIMESTEP, or
//                   t_in) and the two table entries are wave-uniform loads.  A quad moves with one 16-byte load / store
//                   per tensor where that tensor's address of the quad is 16-byte aligned (a sample starts at base + b * c
//                   * hw: aligned only by luck when c * hw % 4 != 0 or the base is offset) and element by element
//                   otherwise, as does the sample's tail of c * hw % 4 elements.  No LDS, no barrier.
// p_losses_partial  one workgroup (256 threads) per (sample, chunk of 4096 elements of its C * HW): the fp32 terms e and
//                   w * e are widened to fp64 as they are made and summed per thread, per wave (shuffles), then over the
//                   four waves in a fixed order into the workgroup's OWN slot of ws (no atomics).  The element -> (thread,
//                   turn) map is the same with 16-byte loads (HW % 4 == 0, aligned pointers) and without, so the order of
//                   the additions, and with it every bit of the result, does not depend on which loads were used.
// p_losses_final    one workgroup: wave w sums the slots of samples w, w + 4, ... (lane i the slots i, i + 64, ..., then a
//                   shuffle tree: an order that depends on C * HW alone), forms the sample's terms in fp64 and adds them
//                   to the wave's batch sums; thread 0 adds the four waves' sums in order and writes the batch scalars.
#include "common.h"
#include "philox.h"

namespace {

constexpr int NT = 256;
constexpr int GROUPS = 4;                 // 4-element groups per thread of the partial kernel
constexpr int CHUNK = NT * GROUPS * 4;    // elements of one sample per workgroup
constexpr long MAX_CHW = 0x7fffffffL - 2 * CHUNK;

struct QArgs {
  const float* x0;
  const float* noise;
  const int32_t* t;
  const float* ta;  // sqrt_alphas_cumprod
  const float* ts;  // sqrt_one_minus_alphas_cumprod
  float* xn;
  f16* xin;
  long n, nvec;
  int n_t, c, hw, chw, ld;
};

__global__ __launch_bounds__(NT) void q_sample_kernel(const QArgs p) {
  const long g = (long)blockIdx.x * NT + threadIdx.x;
  const bool vec = g < p.nvec;
  const long i = vec ? 4 * g : 4 * p.nvec + (g - p.nvec);
  if (i >= p.n) return;
  const int cnt = vec ? 4 : 1;
  long b = i / p.chw;
  const int r = (int)(i - b * p.chw);
  int c = r / p.hw, px = r - c * p.hw;
  float x0[4], nz[4], v[4];
  if (vec) {
    const f32x4 a = *(const f32x4*)(p.x0 + i), m = *(const f32x4*)(p.noise + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) x0[j] = a[j], nz[j] = m[j];
  } else {
    x0[0] = p.x0[i], nz[0] = p.noise[i];
  }
  long cur = -1;
  float a = 0.0f, s = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < cnt) {
      if (b != cur) {  // (a table entry per sample; a timestep outside the tables is never used as an index)
        const int tb = p.t[b];
        const bool ok = (unsigned)tb < (unsigned)p.n_t;
        a = ok ? p.ta[tb] : __builtin_nanf("");
        s = ok ? p.ts[tb] : __builtin_nanf("");
        cur = b;
      }
      const float lhs = a * x0[j], rhs = s * nz[j];
      v[j] = lhs + rhs;
      if (p.xin) p.xin[(b * p.hw + px) * p.ld + c] = (f16)v[j];
      if (++px == p.hw) {
        px = 0;
        if (++c == p.c) c = 0, ++b;
      }
    }
  }
  if (p.xn) {
    if (vec) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = v[j];
      *(f32x4*)(p.xn + i) = o;
    } else {
      p.xn[i] = v[0];
    }
  }
}

struct KArgs {
  const uint32_t* keys;  // [batch, 2]
  const float* x0;
  const int32_t* t_in;   // or nullptr: the keyed timestep
  const float* ta;
  const float* ts;
  int32_t* t_out;
  float* nz;
  float* xn;
  f16* xin;
  long total_tiles;
  int tiles_per_seg, n_t, c, hw, chw, ld;
  uint32_t draw;
};

constexpr int KTILE = NT * 4;

__global__ __launch_bounds__(NT) void q_sample_keyed_kernel(const KArgs p) {
  const int tid = threadIdx.x;
  for (long w = blockIdx.x; w < p.total_tiles; w += gridDim.x) {
    const long b = w / p.tiles_per_seg;
    const int tile = (int)(w - b * p.tiles_per_seg);
    const uint32_t k0 = p.keys[2 * b], k1 = p.keys[2 * b + 1];
    int tb;
    if (p.t_in) {
      tb = p.t_in[b];
    } else {
      uint32_t tw[4];
      philox4x32_10(0u, 0u, (uint32_t)UPK_STREAM_TIMESTEP, p.draw, k0, k1, tw);
      tb = (int)(((uint64_t)tw[0] * (uint64_t)(uint32_t)p.n_t) >> 32);
    }
    if (tile == 0 && tid == 0) p.t_out[b] = tb;
    const bool ok = (unsigned)tb < (unsigned)p.n_t;  // (a timestep outside the tables is never used as an index)
    const float a = ok ? p.ta[tb] : __builtin_nanf(""), s = ok ? p.ts[tb] : __builtin_nanf("");
    const int e = tile * KTILE + 4 * tid;
    if (e >= p.chw) continue;
    const int cnt = min(4, p.chw - e);
    uint32_t q[4];
    philox4x32_10((uint32_t)(e >> 2), 0u, (uint32_t)UPK_STREAM_LOSS_NOISE, p.draw, k0, k1, q);
    float z[4], x0[4], v[4];
    box_muller(q[0], q[1], z[0], z[1]);
    box_muller(q[2], q[3], z[2], z[3]);
    const long i = b * p.chw + e;
    const float* px0 = p.x0 + i;
    if (cnt == 4 && !((uintptr_t)px0 & 15)) {
      const f32x4 m = *(const f32x4*)px0;
#pragma unroll
      for (int j = 0; j < 4; ++j) x0[j] = m[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x0[j] = j < cnt ? px0[j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lhs = a * x0[j], rhs = s * z[j];
      v[j] = lhs + rhs;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float* dst = k == 0 ? p.nz : p.xn;
      const float* src = k == 0 ? z : v;
      if (!dst) continue;
      dst += i;
      if (cnt == 4 && !((uintptr_t)dst & 15)) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = src[j];
        *(f32x4*)dst = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) dst[j] = src[j];
      }
    }
    if (p.xin) {
      int c = e / p.hw, px = e - c * p.hw;
      f16* row = p.xin + b * p.hw * p.ld;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          row[(long)px * p.ld + c] = (f16)v[j];
          if (++px == p.hw) px = 0, ++c;
        }
      }
    }
  }
}

struct PArgs {
  const float* pred;
  const float* tgt;
  const float* w;  // [B, C or 1, HW], or nullptr
  double* part;    // [B][nblk][2]
  int chw, hw, w_full, nblk, l1;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void p_losses_partial_kernel(const PArgs p) {
  __shared__ double s_red[NT / 64][2];
  const int tid = threadIdx.x;
  const long b = blockIdx.x / (unsigned)p.nblk;
  const int blk = (int)(blockIdx.x - (unsigned)(b * p.nblk));
  const float* pred = p.pred + b * p.chw;
  const float* tgt = p.tgt + b * p.chw;
  const float* w = p.w ? p.w + b * (p.w_full ? p.chw : p.hw) : nullptr;
  double sw = 0.0, se = 0.0;
#pragma unroll
  for (int k = 0; k < GROUPS; ++k) {
    const int r = blk * CHUNK + 4 * (tid + NT * k);
    if (r >= p.chw) break;
    float pv[4], tv[4], wv[4];
    int cnt = 4;
    if (VEC) {  // (HW % 4 == 0: a group neither leaves the sample nor crosses a channel)
      const f32x4 a = *(const f32x4*)(pred + r), m = *(const f32x4*)(tgt + r);
      f32x4 q = {1.0f, 1.0f, 1.0f, 1.0f};
      if (w) q = *(const f32x4*)(w + (p.w_full ? r : r % p.hw));
#pragma unroll
      for (int j = 0; j < 4; ++j) pv[j] = a[j], tv[j] = m[j], wv[j] = q[j];
    } else {
      cnt = min(4, p.chw - r);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = j < cnt;
        pv[j] = ok ? pred[r + j] : 0.0f;
        tv[j] = ok ? tgt[r + j] : 0.0f;
        wv[j] = ok && w ? w[p.w_full ? r + j : (r + j) % p.hw] : 1.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        const float d = tv[j] - pv[j];
        const float e = p.l1 ? fabsf(d) : d * d;
        const float we = w ? wv[j] * e : e;
        sw += (double)we;
        se += (double)e;
      }
    }
  }
  sw = wave_sum(sw);
  se = wave_sum(se);
  if ((tid & 63) == 0) s_red[tid >> 6][0] = sw, s_red[tid >> 6][1] = se;
  __syncthreads();
  if (tid < 2) p.part[((long)blockIdx.x) * 2 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

struct FArgs {
  const double* part;
  const int32_t* t;
  const float* logvar;
  const float* lvlb;
  float* out;  // {loss, loss_simple, loss_gamma, loss_vlb}, then {simple, plain} per sample
  int batch, nblk, n_t, chw;
  float l_simple_weight, original_elbo_weight;
};

__global__ __launch_bounds__(NT) void p_losses_final_kernel(const FArgs p) {
  __shared__ double s_acc[NT / 64][3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double a_simple = 0.0, a_gamma = 0.0, a_vlb = 0.0;
  for (int b = wave; b < p.batch; b += NT / 64) {
    const double* pp = p.part + (long)b * p.nblk * 2;
    double sw = 0.0, se = 0.0;
    for (int i = lane; i < p.nblk; i += 64) sw += pp[2 * i], se += pp[2 * i + 1];
    sw = wave_sum(sw);
    se = wave_sum(se);
    const int tb = p.t[b];
    const bool ok = (unsigned)tb < (unsigned)p.n_t;
    const double nan = __builtin_nan("");
    const double simple = ok ? sw / (double)p.chw : nan, plain = ok ? se / (double)p.chw : nan;
    const double lv = ok ? (double)p.logvar[tb] : nan, lw = ok ? (double)p.lvlb[tb] : nan;
    a_simple += simple;
    a_gamma += simple / exp(lv) + lv;
    a_vlb += lw * plain;
    if (lane == 0) p.out[4 + 2 * (long)b] = (float)simple, p.out[5 + 2 * (long)b] = (float)plain;
  }
  if (lane == 0) s_acc[wave][0] = a_simple, s_acc[wave][1] = a_gamma, s_acc[wave][2] = a_vlb;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = (((s_acc[0][q] + s_acc[1][q]) + s_acc[2][q]) + s_acc[3][q]) / (double)p.batch;
    p.out[0] = (float)((double)p.l_simple_weight * v[1] + (double)p.original_elbo_weight * v[2]);
    p.out[1] = (float)v[0];
    p.out[2] = (float)v[1];
    p.out[3] = (float)v[2];
  }
}

// workgroups per sample of the partial kernel; 0: C * HW is refused
long blocks_per_sample(int c, int hw) {
  if (c <= 0 || hw <= 0) return 0;
  const long chw = (long)c * hw;
  return chw > MAX_CHW ? 0 : (chw + CHUNK - 1) / CHUNK;
}

}  // namespace

extern "C" int upk_q_sample_f32(upk_ctx* ctx, const float* x_start, const float* noise, const int32_t* t,
                                const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, int n_t,
                                float* x_noisy, void* xin, int ld_xin, int batch, int c, int hw, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x_start || !noise || !t || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod)
    return upk_fail(ctx, UPK_EINVAL, "q_sample: null pointer");
  if (!x_noisy && !xin) return upk_fail(ctx, UPK_EINVAL, "q_sample: x_noisy and xin are both null");
  if (batch <= 0 || c <= 0 || hw <= 0 || n_t <= 0) return upk_fail(ctx, UPK_EINVAL, "q_sample: sizes must be positive");
  if (xin && ld_xin < c) return upk_fail(ctx, UPK_EINVAL, "q_sample: ld_xin = %d below c = %d", ld_xin, c);
  if (((uintptr_t)x_start | (uintptr_t)noise | (uintptr_t)t | (uintptr_t)sqrt_alphas_cumprod |
       (uintptr_t)sqrt_one_minus_alphas_cumprod | (uintptr_t)x_noisy) & 3)
    return upk_fail(ctx, UPK_EINVAL, "q_sample: an fp32 / int32 pointer is not 4-byte aligned");
  if ((uintptr_t)xin & 1) return upk_fail(ctx, UPK_EINVAL, "q_sample: xin is not 2-byte aligned");
  if (!blocks_per_sample(c, hw)) return upk_fail(ctx, UPK_ESHAPE, "q_sample: c * hw = %ld too large", (long)c * hw);
  QArgs qa;
  qa.x0 = x_start, qa.noise = noise, qa.t = t, qa.ta = sqrt_alphas_cumprod, qa.ts = sqrt_one_minus_alphas_cumprod;
  qa.xn = x_noisy, qa.xin = (f16*)xin, qa.n_t = n_t, qa.c = c, qa.hw = hw, qa.chw = c * hw, qa.ld = ld_xin;
  qa.n = (long)batch * c * hw;
  const bool aligned = !(((uintptr_t)x_start | (uintptr_t)noise | (uintptr_t)x_noisy) & 15);
  qa.nvec = aligned ? qa.n / 4 : 0;
  const long threads = qa.nvec + (qa.n - 4 * qa.nvec);
  const long blocks = (threads + NT - 1) / NT;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "q_sample: %ld workgroups", blocks);
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, qa);
  return upk_check_launch(ctx, "q_sample");
}

extern "C" int upk_q_sample_keyed_f32(upk_ctx* ctx, const uint32_t* keys, uint32_t draw, const float* x_start,
                                      const int32_t* t_in, const float* sqrt_alphas_cumprod,
                                      const float* sqrt_one_minus_alphas_cumprod, int n_t, int32_t* t_out, float* noise_out,
                                      float* x_noisy, void* xin, int ld_xin, int batch, int c, int hw, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!keys || !x_start || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || !t_out)
    return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: null pointer");
  if (!noise_out && !x_noisy && !xin) return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: noise_out, x_noisy and xin are all null");
  if (batch <= 0 || c <= 0 || hw <= 0 || n_t <= 0) return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: sizes must be positive");
  if (xin && ld_xin < c) return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: ld_xin = %d below c = %d", ld_xin, c);
  if (((uintptr_t)keys | (uintptr_t)x_start | (uintptr_t)t_in | (uintptr_t)sqrt_alphas_cumprod |
       (uintptr_t)sqrt_one_minus_alphas_cumprod | (uintptr_t)t_out | (uintptr_t)noise_out | (uintptr_t)x_noisy) & 3)
    return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: an fp32 / int32 pointer is not 4-byte aligned");
  if ((uintptr_t)xin & 1) return upk_fail(ctx, UPK_EINVAL, "q_sample_keyed: xin is not 2-byte aligned");
  if (!blocks_per_sample(c, hw)) return upk_fail(ctx, UPK_ESHAPE, "q_sample_keyed: c * hw = %ld too large", (long)c * hw);
  KArgs ka;
  ka.keys = keys, ka.x0 = x_start, ka.t_in = t_in, ka.ta = sqrt_alphas_cumprod, ka.ts = sqrt_one_minus_alphas_cumprod;
  ka.t_out = t_out, ka.nz = noise_out, ka.xn = x_noisy, ka.xin = (f16*)xin;
  ka.n_t = n_t, ka.c = c, ka.hw = hw, ka.chw = c * hw, ka.ld = ld_xin, ka.draw = draw;
  ka.tiles_per_seg = (ka.chw + KTILE - 1) / KTILE;
  ka.total_tiles = (long)batch * ka.tiles_per_seg;
  const unsigned grid = (unsigned)(ka.total_tiles < 65536L ? ka.total_tiles : 65536L);  // (the tiles beyond go grid-stride)
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  hipLaunchKernelGGL(q_sample_keyed_kernel, dim3(grid), dim3(NT), 0, stream, ka);
  return upk_check_launch(ctx, "q_sample_keyed");
}

extern "C" size_t upk_p_losses_ws_bytes(int batch, int c, int hw) {
  const long nblk = blocks_per_sample(c, hw);
  if (batch <= 0 || !nblk || nblk * batch > 0x7fffffffL) return 0;
  return (size_t)batch * nblk * 2 * sizeof(double);
}

extern "C" int upk_p_losses_f32(upk_ctx* ctx, const float* model_out, const float* target, const float* loss_w,
                                int loss_w_channels, const int32_t* t, const float* logvar, const float* lvlb_weights,
                                int n_t, int loss_type, float l_simple_weight, float original_elbo_weight, float* out,
                                int batch, int c, int hw, void* ws, size_t ws_bytes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!model_out || !target || !t || !logvar || !lvlb_weights || !out || !ws)
    return upk_fail(ctx, UPK_EINVAL, "p_losses: null pointer");
  if (batch <= 0 || c <= 0 || hw <= 0 || n_t <= 0) return upk_fail(ctx, UPK_EINVAL, "p_losses: sizes must be positive");
  if (loss_type != UPK_LOSS_L2 && loss_type != UPK_LOSS_L1)
    return upk_fail(ctx, UPK_EINVAL, "p_losses: loss_type = %d, must be UPK_LOSS_L2 or UPK_LOSS_L1", loss_type);
  if (loss_w && loss_w_channels != 1 && loss_w_channels != c)
    return upk_fail(ctx, UPK_EINVAL, "p_losses: loss_w with %d channels, must be 1 or c = %d", loss_w_channels, c);
  if (((uintptr_t)model_out | (uintptr_t)target | (uintptr_t)loss_w | (uintptr_t)t | (uintptr_t)logvar |
       (uintptr_t)lvlb_weights | (uintptr_t)out) & 3)
    return upk_fail(ctx, UPK_EINVAL, "p_losses: an fp32 / int32 pointer is not 4-byte aligned");
  if ((uintptr_t)ws & 15) return upk_fail(ctx, UPK_EINVAL, "p_losses: ws is not 16-byte aligned");
  const long nblk = blocks_per_sample(c, hw);
  if (!nblk) return upk_fail(ctx, UPK_ESHAPE, "p_losses: c * hw = %ld too large", (long)c * hw);
  if (nblk * batch > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "p_losses: %ld workgroups", nblk * batch);
  const size_t need = (size_t)batch * nblk * 2 * sizeof(double);
  if (ws_bytes < need) return upk_fail(ctx, UPK_EWORKSPACE, "p_losses: workspace of %zu bytes, %zu needed", ws_bytes, need);

  PArgs pa;
  pa.pred = model_out, pa.tgt = target, pa.w = loss_w, pa.part = (double*)ws;
  pa.chw = c * hw, pa.hw = hw, pa.w_full = loss_w_channels == c, pa.nblk = (int)nblk, pa.l1 = loss_type == UPK_LOSS_L1;
  const bool vec = hw % 4 == 0 && !(((uintptr_t)model_out | (uintptr_t)target | (uintptr_t)loss_w) & 15);
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  const dim3 grid((unsigned)(nblk * batch));
  if (vec) {
    hipLaunchKernelGGL(p_losses_partial_kernel<true>, grid, dim3(NT), 0, stream, pa);
  } else {
    hipLaunchKernelGGL(p_losses_partial_kernel<false>, grid, dim3(NT), 0, stream, pa);
  }
  const int e = upk_check_launch(ctx, "p_losses_partial");
  if (e != UPK_OK) return e;
  FArgs fa;
  fa.part = pa.part, fa.t = t, fa.logvar = logvar, fa.lvlb = lvlb_weights, fa.out = out;
  fa.batch = batch, fa.nblk = (int)nblk, fa.n_t = n_t, fa.chw = pa.chw;
  fa.l_simple_weight = l_simple_weight, fa.original_elbo_weight = original_elbo_weight;
  hipLaunchKernelGGL(p_losses_final_kernel, dim3(1), dim3(NT), 0, stream, fa);
  return upk_check_launch(ctx, "p_losses_final");
}
