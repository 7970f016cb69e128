// Fused feed-forward tail of a SpatialTransformer block (attention.py:42-64, 215, 259-261), one launch:
//
//     h   = GEGLU(LayerNorm(t2))                      [M, 4C]    norm3 -> ff.net.0 (value | gate, erf GELU)
//     out = x_in + (P F2) h + P t2 + (P b2 + bp)      [M, C]     ff.net.2, + t2, proj_out, + x_in  (one GEMM over [h | t2])
//
// A workgroup owns BM rows.  t2's tile is staged once in LDS (LDS-DMA), the 4C-wide hidden activation h is produced
// pass by pass (8 waves x 2 fragments of 16 columns, astat.hip's scheme: weights straight from L2 into a register
// ring, no barrier in the K loops) and written to LDS as the A operand of the second GEMM — it never exists in HBM:
// 14.7 MB written and read back per block at the 32x32 level, and one launch less.  The weight stream runs on across
// the seam (the ring's refills go from the last GEGLU pass straight into the second GEMM's first chunks); the only
// workgroup barriers are the one behind the tile DMA and the one between the two GEMMs.
//
// The price is the weight traffic per CU: every workgroup streams BOTH weights in full ((8 + 5) C^2 fp16), where the
// two-launch form tiles N.  It pays where M / BM covers the chip (the 32x32 level: M = 8192), not at the deeper levels.
//
// Two forms.  mlp_kernel<2 | 4, 7> (32 / 64 rows) is the RESIDENT form above: the whole h tile in LDS ((4C + C) / 32
// chunks x BM x 64 B: 140 KB at 64 rows, so no taller tile), one launch that has the chip to itself — 256 workgroups at
// M = 8192.  mlp_stream_kernel<4, 7 | 8, 4> (64 / 128 rows, C = 224) is the STREAMING form further down: h exists only as
// two 128-column slices (t2 tile + 2 x 4 chunks: 15 x BM x 64 B = 120 KB at 128 rows), the second GEMM's accumulators stay
// in registers across the GEGLU passes.  At 128 rows a launch is 64 workgroups that stream the weights a quarter as often:
// the form for launches that share the chip with other batches.  Same K order per row: equal BM, equal bits.
#include "igemm_common.h"

namespace upkd {
namespace {

constexpr int ML_NW = 8;
constexpr int ML_SLICES = 2;  // h slices in LDS (one slice and a second barrier per pass lost the A/B of DESIGN.md 26)

struct MlpArgs {
  const f16* x;      // t2 [M, ldx] (un-normalised residual stream)
  const f16* w1;     // packed GEGLU weight [nch1][n1][32], LayerNorm affine folded in (W * gamma)
  const f16* w2;     // packed [nh + nch1][n2pad][32]: K order [h | t2]
  const f16* zero;
  const float* b1;   // [n1] packed order (b + W beta)
  const float* u1;   // [n1] column sums of the fp16-rounded W * gamma
  const float* b2;   // [n2pad]
  const f16* res;    // x_in [M, ldr]
  f16* y;            // out [M, ldy]
  float* gn_cp;      // per-(M tile, channel) partials [B][nblk][2][n2pad] for the GroupNorm that reads `out`, or nullptr
  int ldx, ldr, ldy, M, nch1, n1, n2, n2pad, nh;
  int gn_nblk, gn_hw;
  float ln_inv_dim, ln_eps;
  unsigned long long* dbg;  // dev: s_memtime stamps (UPK_TIMELINE builds)
};
#define ML_PIN(v) asm volatile("" ::"s"(v))

template <int MI, int PF>
__global__ __launch_bounds__(512) void mlp_kernel(const MlpArgs s) {
  constexpr int NW = ML_NW, NI = 2;
  constexpr int BM = MI * 16;
  constexpr int PW = NW * NI * 16;  // packed GEGLU columns per pass (= 128 hidden columns)
  extern __shared__ __attribute__((aligned(16))) f16 smem[];
  ML_PIN(s.x); ML_PIN(s.w1); ML_PIN(s.w2); ML_PIN(s.zero); ML_PIN(s.b1); ML_PIN(s.u1); ML_PIN(s.b2); ML_PIN(s.res);
  ML_PIN(s.y); ML_PIN(s.gn_cp); ML_PIN(s.ldx); ML_PIN(s.ldr); ML_PIN(s.ldy); ML_PIN(s.M); ML_PIN(s.nch1); ML_PIN(s.n1);
  ML_PIN(s.n2); ML_PIN(s.n2pad); ML_PIN(s.nh);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
#ifdef UPK_TIMELINE
  const bool tl = s.dbg && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && (wave == 0 || wave == 4);
  unsigned long long* tlp = s.dbg + (blockIdx.x == 0 ? 0 : 64) + (wave == 0 ? 0 : 32);
#define STAMP(i) do { if (tl && lane == 0 && (i) < 32) tlp[i] = __builtin_readcyclecounter(); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif
  STAMP(0);
  const int m0 = upk_xcd_tile(blockIdx.x, gridDim.x) * BM;
  const int nch1 = s.nch1, nh = s.nh, nch2 = nh + nch1;
  // LDS: chunks [0, nh) = h, chunks [nh, nh + nch1) = t2  (the second GEMM's K order), then the row statistics
  f16* const hT = smem;
  f16* const xT = smem + nh * BM * 32;
  float* const st = (float*)(smem + nch2 * BM * 32);  // [BM][2]
  float* const bl = st + BM * 2;                      // [2][n1]: GEGLU bias, LayerNorm column sums (packed order)

  // ---- 1. t2 tile
  {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;
    const int r16 = lane >> 2;
    const int chd = (lane & 3) ^ ((-(lane >> 4)) & 3);
    const f16* zsrc = s.zero + (lane & 3) * 8;
    for (int idx = wave; idx < nch1 * MI; idx += NW) {
      const int kc = idx / MI, rg = idx - kc * MI;
      const int m = m0 + rg * 16 + r16;
      const f16* src = m < s.M ? s.x + (long)m * s.ldx + kc * 32 + chd * 8 : zsrc;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(xT + (kc * BM + rg * 16) * 32), 16, 0, 0);
    }
    // the GEGLU epilogue's operands for every pass, into LDS with the tile: read from global memory per pass they put a
    // vmcnt(0) in front of each epilogue (the compiler cannot count across the K loop) — a drain of the 14 weight
    // fragments just requested for the next pass, ~2k cycles per pass in the in-kernel stamps
    const int nkb = s.n1 >> 8;  // 1 KiB pieces per array (n1 % 256 == 0)
    for (int idx = wave; idx < 2 * nkb; idx += NW) {
      const float* src = (idx < nkb ? s.b1 + idx * 256 : s.u1 + (idx - nkb) * 256) + lane * 4;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(bl + idx * 256), 16, 0, 0);
    }
  }

  // ---- 2. weight streams.  GEGLU: wave w owns, per pass, value columns blk*64 + q*16 .. +15 and their gates 32
  // columns on (blk = pass * 4 + w / 2, q = w & 1).  Second GEMM: waves 0 .. n2pad / 32 - 1 own 32 columns each.
  const int col1 = (wave >> 1) * 64 + (wave & 1) * 16;
  const int npass = (s.n1 + PW - 1) / PW;
  const int p1w = min(npass, (s.n1 - col1 + PW - 1) / PW);  // passes with columns for this wave
  const int col2 = wave * 32;
  const bool act2 = col2 < s.n2pad;
  const unsigned ks1 = (unsigned)s.n1 * 64u, ks2 = (unsigned)s.n2pad * 64u;
  const unsigned loff = (unsigned)(lc * 32 + lg * 8) * 2u;
  unsigned voff1[PF], voff2[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) voff1[u] = loff + (unsigned)u * ks1, voff2[u] = loff + (unsigned)u * ks2;
  const char* wb1 = (const char*)s.w1;
  const char* wb2 = (const char*)s.w2 + (size_t)col2 * 64;
  auto base1 = [&](int p, int kc) -> const char* {
    return wb1 + (size_t)(((unsigned)kc * (unsigned)s.n1 + (unsigned)(col1 + p * PW)) * 64u);
  };
  f16x8 ring[PF][NI];
  if (p1w > 0) {
    const char* b0 = base1(0, 0);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      ring[u][0] = *(const f16x8*)(b0 + voff1[u]);
      ring[u][1] = *(const f16x8*)(b0 + 2048 + voff1[u]);
    }
  } else if (act2) {  // (no GEGLU columns for this wave: its ring starts in the second GEMM)
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      ring[u][0] = *(const f16x8*)(wb2 + voff2[u]);
      ring[u][1] = *(const f16x8*)(wb2 + 1024 + voff2[u]);
    }
  }
  // operands of the second GEMM's epilogue (requested with the ring: one round trip)
  f32x4 b2v[NI];
  f16x4 rr[MI][NI];
  if (act2) {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col2 + j * 16 + lg * 4;
      b2v[j] = *(const f32x4*)(s.b2 + (n < s.n2pad ? n : 0));
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const unsigned m = (unsigned)min(m0 + i * 16 + lc, s.M - 1);
        rr[i][j] = *(const f16x4*)(s.res + m * (unsigned)s.ldr + (unsigned)(n < s.n2 ? n : 0));
      }
    }
  }
  STAMP(1);
  __syncthreads();  // (t2 tile landed)
  STAMP(2);

  // ---- 3. LayerNorm statistics of the tile's rows (from the resident tile)
  {
    constexpr int LPR = 512 / BM;
    const int row = tid / LPR, part = tid - row * LPR;
    float s1 = 0.f, s2 = 0.f;
    const f16x2 one2 = {(f16)1.f, (f16)1.f};
    for (int q = part; q < nch1 * 4; q += LPR) {
      const f16x8 v = *(const f16x8*)(xT + ((q >> 2) * BM + row) * 32 + (q & 3) * 8);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const f16x2 xx = {v[2 * h], v[2 * h + 1]};
        s1 = __builtin_amdgcn_fdot2(xx, one2, s1, false);
        s2 = __builtin_amdgcn_fdot2(xx, xx, s2, false);
      }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (part == 0) {
      const float mu = s1 * s.ln_inv_dim;
      st[2 * row] = mu;
      st[2 * row + 1] = rsqrtf(fmaxf(s2 * s.ln_inv_dim - mu * mu, 0.f) + s.ln_eps);
    }
  }
  __syncthreads();

  STAMP(3);
  const unsigned la = (unsigned)(lc * 32 + lds_swz(lc, lg) * 8) * 2u;
  const char* const xs = (const char*)xT;
  const char* const hs = (const char*)hT;

  // ---- 4. GEGLU passes -> h tile in LDS
  for (int p = 0; p < p1w; ++p) {
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kc0 = 0; kc0 < nch1; kc0 += PF) {
      const bool wrap = kc0 + PF >= nch1;       // the refills of this block belong to the next pass ...
      const bool seam = wrap && p + 1 >= p1w;   // ... or, behind the last pass, to the second GEMM's first chunks
      const char* sb0 = seam ? (act2 ? wb2 : wb1) : base1(wrap ? p + 1 : p, wrap ? 0 : kc0 + PF);
      const char* sb1 = seam ? (act2 ? wb2 + 1024 : wb1) : sb0 + 2048;
      const char* ldsA = xs + la + (unsigned)(kc0 * BM) * 64u;
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        f16x8 fc[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) fc[i] = *(const f16x8*)(ldsA + (u * BM + i * 16) * 64);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[u][j], fc[i], acc[i][j], 0, 0, 0);
        const unsigned vo = seam ? (act2 ? voff2[u] : loff) : voff1[u];
        ring[u][0] = *(const f16x8*)(sb0 + vo);
        ring[u][1] = *(const f16x8*)(sb1 + vo);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    STAMP(4 + 2 * p);
    // epilogue: folded LayerNorm, bias, v * gelu(g) -> fp16 -> h tile (chunk = hidden column / 32, XOR-swizzled 16-byte
    // pieces like every A tile: this lane's 4 columns are half a piece)
    const int n = col1 + p * PW + lg * 4;            // packed value column
    const f32x4 bv0 = *(const f32x4*)(bl + n), bv1 = *(const f32x4*)(bl + n + 32);
    const f32x4 lu0 = *(const f32x4*)(bl + s.n1 + n), lu1 = *(const f32x4*)(bl + s.n1 + n + 32);
    const int oc = (n >> 6) * 32 + (n & 31);         // hidden column
    const int hk = oc >> 5, hq = (oc & 31) >> 3, hh = oc & 7;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x2 mr = *(const f32x2*)(st + 2 * (i * 16 + lc));
      const f32x4 v = (acc[i][0] - mr[0] * lu0) * mr[1] + bv0;
      const f32x4 g = (acc[i][1] - mr[0] * lu1) * mr[1] + bv1;
      f16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (f16)upk_geglu_mul(v[k], g[k]);
      const int row = i * 16 + lc;
      *(f16x4*)(hT + (hk * BM + row) * 32 + lds_swz(lc, hq) * 8 + hh) = o;
    }
    STAMP(5 + 2 * p);
  }
  STAMP(20);
  __syncthreads();  // (h complete)
  STAMP(21);

  // ---- 5. second GEMM over [h | t2] (LDS chunk order = its K order), epilogue: bias, residual, GroupNorm partials
  if (!act2) return;
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int kc0 = 0; kc0 < nch2; kc0 += PF) {
    const bool dead = kc0 + PF >= nch2;
    const char* sb0 = dead ? wb2 : wb2 + (size_t)((unsigned)(kc0 + PF) * ks2);
    const char* ldsA = hs + la + (unsigned)(kc0 * BM) * 64u;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      f16x8 fc[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fc[i] = *(const f16x8*)(ldsA + (u * BM + i * 16) * 64);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[u][j], fc[i], acc[i][j], 0, 0, 0);
      const unsigned vo = dead ? loff : voff2[u];
      ring[u][0] = *(const f16x8*)(sb0 + vo);
      ring[u][1] = *(const f16x8*)(sb0 + (dead ? 0 : 1024) + vo);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  STAMP(22);
  f32x4 cs[NI], cq[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) cs[j] = cq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + i * 16 + lc;
    const bool ok = m < s.M;
    f16* yrow = s.y + (unsigned)(ok ? m : 0) * (unsigned)s.ldy;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col2 + j * 16 + lg * 4;
      const f32x4 v = acc[i][j] + b2v[j];
      f16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (f16)(v[k] + (float)rr[i][j][k]);
      if (ok && n < s.n2) *(f16x4*)(yrow + n) = o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = ok ? (float)o[k] : 0.f;
        cs[j][k] += f;
        cq[j][k] += f * f;
      }
    }
  }
  if (s.gn_cp) {  // (a wave owns its columns for all BM rows: the 16 rows of a fragment by rotate-add, no LDS)
    const int b = m0 / s.gn_hw;
    const int blk = (m0 - b * s.gn_hw) / BM;
    float* dst = s.gn_cp + (long)((b * s.gn_nblk + blk) * 2) * s.n2pad;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col2 + j * 16 + lg * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cs[j][k] = Epi::row_sum16(cs[j][k]);
        cq[j][k] = Epi::row_sum16(cq[j][k]);
      }
      if (lc == 0 && n < s.n2pad) {
        *(f32x4*)(dst + n) = cs[j];
        *(f32x4*)(dst + s.n2pad + n) = cq[j];
      }
    }
  }
#ifdef UPK_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  STAMP(23);
#endif
#undef STAMP
}

template <int I>
struct ml_ic {
  static constexpr int value = I;
};
template <int B, int E, class F>
__device__ __forceinline__ void ml_static_for(F&& f) {  // f(ml_ic<B>) .. f(ml_ic<E - 1>): a loop whose index is a constant
  if constexpr (B < E) {
    f(ml_ic<B>{});
    ml_static_for<B + 1, E>(f);
  }
}

// The streaming form: the same computation with the same operands, but h never exists as a whole tile.  The second
// GEMM's accumulators (wave w: its 32 output columns, MI x 2 fragments) live in registers for the whole kernel; each
// GEGLU pass writes its 128 hidden columns — 4 K chunks of the second GEMM — into one of two LDS slices, and behind ONE
// workgroup barrier every wave feeds those 4 chunks to its accumulators while the other slice is free for the next pass
// (a wave that writes slice p & 1 again in pass p + 2 has passed the barrier of pass p + 1, which no wave reaches before
// it has consumed pass p).  After the last pass the t2 chunks are consumed from the resident tile: the K order of a row
// is the resident kernel's (hidden chunks ascending, then t2), so at equal BM the results are bit-identical.
// One weight ring of RD slots carries both streams.  A pass is NK1 + 4 steps (7 chunks of w1, 4 of w2), unrolled; step t
// consumes slot t % RD and refills it with step t + RD of the pass or, in its last RD steps, with step t % RD of the
// next pass (behind the last pass: of the t2 chunks of w2) — every fragment is requested >= min(RD, 3) steps before its
// use, and a pass starts with its steps 0 .. RD - 1 in slots 0 .. RD - 1 whatever (NK1 + 4) % RD is.
template <int MI, int RD>
__global__ __launch_bounds__(512) void mlp_stream_kernel(const MlpArgs s) {
  constexpr int NW = ML_NW, NI = 2;
  constexpr int BM = MI * 16;
  constexpr int PW = NW * NI * 16;  // packed GEGLU columns per pass (= 128 hidden columns)
  constexpr int NK1 = 7;            // K chunks of a GEGLU pass (c = 224: n_pad <= 256 leaves no other member of the family)
  constexpr int NS = PW / 64;       // hidden chunks per pass = K chunks of the second GEMM per slice
  constexpr int S = NK1 + NS;
  constexpr int NSL = ML_SLICES;
  static_assert(RD >= 1 && RD <= NK1, "the first RD steps of a pass are w1 chunks (t2 chunks behind the last pass)");
  extern __shared__ __attribute__((aligned(16))) f16 smem[];
  ML_PIN(s.x); ML_PIN(s.w1); ML_PIN(s.w2); ML_PIN(s.zero); ML_PIN(s.b1); ML_PIN(s.u1); ML_PIN(s.b2); ML_PIN(s.res);
  ML_PIN(s.y); ML_PIN(s.gn_cp); ML_PIN(s.ldx); ML_PIN(s.ldr); ML_PIN(s.ldy); ML_PIN(s.M); ML_PIN(s.nch1); ML_PIN(s.n1);
  ML_PIN(s.n2); ML_PIN(s.n2pad); ML_PIN(s.nh);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int m0 = upk_xcd_tile(blockIdx.x, gridDim.x) * BM;
  const int nh = s.nh;
  // LDS: the t2 tile (NK1 chunks), two slices of NS chunks of h, the row statistics, the GEGLU vectors
  f16* const xT = smem;
  f16* const hS = smem + NK1 * BM * 32;
  float* const st = (float*)(smem + (NK1 + NSL * NS) * BM * 32);  // [BM][2]
  float* const bl = st + BM * 2;                                // [2][n1]: GEGLU bias, LayerNorm column sums (packed order)

  // ---- 1. t2 tile and the GEGLU epilogue's vectors (as mlp_kernel)
  {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;
    const int r16 = lane >> 2;
    const int chd = (lane & 3) ^ ((-(lane >> 4)) & 3);
    const f16* zsrc = s.zero + (lane & 3) * 8;
    for (int idx = wave; idx < NK1 * MI; idx += NW) {
      const int kc = idx / MI, rg = idx - kc * MI;
      const int m = m0 + rg * 16 + r16;
      const f16* src = m < s.M ? s.x + (long)m * s.ldx + kc * 32 + chd * 8 : zsrc;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(xT + (kc * BM + rg * 16) * 32), 16, 0, 0);
    }
    const int nkb = s.n1 >> 8;  // 1 KiB pieces per array (n1 % 256 == 0)
    for (int idx = wave; idx < 2 * nkb; idx += NW) {
      const float* src = (idx < nkb ? s.b1 + idx * 256 : s.u1 + (idx - nkb) * 256) + lane * 4;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(bl + idx * 256), 16, 0, 0);
    }
  }

  // ---- 2. weight streams: the column ownership of mlp_kernel.  n1 % PW == 0, so every wave has columns in every pass.
  // A wave without columns in the second GEMM (act2 false) runs its steps all the same, on the first 2 KiB of w2 over and
  // over (chunk stride 0: hits in its L1) and into accumulators nobody reads: a branch around them would cost every wave
  // the compiler's vmcnt count (it drains the ring at each join), and that wave's SIMD is no busier than the other three.
  const int col1 = (wave >> 1) * 64 + (wave & 1) * 16;
  const int npass = s.n1 / PW;
  const int col2 = wave * 32;
  const bool act2 = col2 < s.n2pad;
  const unsigned ks1 = (unsigned)s.n1 * 64u, ks2 = act2 ? (unsigned)s.n2pad * 64u : 0u;
  const unsigned loff = (unsigned)(lc * 32 + lg * 8) * 2u;
  const char* wb1 = (const char*)s.w1 + (size_t)col1 * 64;
  const char* wb2 = (const char*)s.w2 + (size_t)(act2 ? col2 : 0) * 64;
  const char* const wt2 = wb2 + (size_t)((unsigned)nh * ks2);  // w2's t2 chunks
  f16x8 ring[RD][NI];
#pragma unroll
  for (int u = 0; u < RD; ++u) {
    ring[u][0] = *(const f16x8*)(wb1 + (unsigned)u * ks1 + loff);
    ring[u][1] = *(const f16x8*)(wb1 + (unsigned)u * ks1 + 2048 + loff);
  }
  __syncthreads();  // (t2 tile landed)

  // ---- 3. LayerNorm statistics of the tile's rows (from the resident tile)
  {
    constexpr int LPR = 512 / BM;
    const int row = tid / LPR, part = tid - row * LPR;
    float s1 = 0.f, s2 = 0.f;
    const f16x2 one2 = {(f16)1.f, (f16)1.f};
    for (int q = part; q < NK1 * 4; q += LPR) {
      const f16x8 v = *(const f16x8*)(xT + ((q >> 2) * BM + row) * 32 + (q & 3) * 8);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const f16x2 xx = {v[2 * h], v[2 * h + 1]};
        s1 = __builtin_amdgcn_fdot2(xx, one2, s1, false);
        s2 = __builtin_amdgcn_fdot2(xx, xx, s2, false);
      }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (part == 0) {
      const float mu = s1 * s.ln_inv_dim;
      st[2 * row] = mu;
      st[2 * row + 1] = rsqrtf(fmaxf(s2 * s.ln_inv_dim - mu * mu, 0.f) + s.ln_eps);
    }
  }
  __syncthreads();

  const unsigned la = (unsigned)(lc * 32 + lds_swz(lc, lg) * 8) * 2u;
  const char* const xs = (const char*)xT + la;
  f32x4 acc[MI][NI];  // the second GEMM's
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- 4. passes: GEGLU over the t2 tile -> slice p & 1 -> barrier -> the slice's 4 chunks into the second GEMM
#pragma unroll 1
  for (int p = 0; p < npass; ++p) {
    const bool last = p + 1 >= npass;
    const char* const g1 = wb1 + (size_t)((unsigned)(p * PW) * 64u);         // this pass's w1 columns
    const char* const g2 = wb2 + (size_t)((unsigned)(p * NS) * ks2);         // this pass's w2 chunks
    const char* const nx = last ? wt2 : g1 + PW * 64;                        // the first RD steps of what follows
    const unsigned ksn = last ? ks2 : ks1, fn = last ? 1024u : 2048u;
    f16* const hT = hS + (p % NSL) * (NS * BM * 32);
    auto refill = [&](auto tc) {
      constexpr int t = decltype(tc)::value, q = t + RD, sl = t % RD;
      if constexpr (q < NK1) {
        ring[sl][0] = *(const f16x8*)(g1 + (unsigned)q * ks1 + loff);
        ring[sl][1] = *(const f16x8*)(g1 + (unsigned)q * ks1 + 2048 + loff);
      } else if constexpr (q < S) {
        ring[sl][0] = *(const f16x8*)(g2 + (unsigned)(q - NK1) * ks2 + loff);
        ring[sl][1] = *(const f16x8*)(g2 + (unsigned)(q - NK1) * ks2 + 1024 + loff);
      } else {
        ring[sl][0] = *(const f16x8*)(nx + (unsigned)sl * ksn + loff);
        ring[sl][1] = *(const f16x8*)(nx + (unsigned)sl * ksn + fn + loff);
      }
    };
    f32x4 ag[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) ag[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ml_static_for<0, NK1>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      f16x8 fc[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fc[i] = *(const f16x8*)(xs + (t * BM + i * 16) * 64);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          ag[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[t % RD][j], fc[i], ag[i][j], 0, 0, 0);
      refill(tc);
      __builtin_amdgcn_sched_barrier(0);
    });
    {  // epilogue: folded LayerNorm, bias, v * gelu(g) -> fp16 -> slice (chunk = wave / 2; layout as mlp_kernel's h tile)
      const int n = col1 + p * PW + lg * 4;  // packed value column
      const f32x4 bv0 = *(const f32x4*)(bl + n), bv1 = *(const f32x4*)(bl + n + 32);
      const f32x4 lu0 = *(const f32x4*)(bl + s.n1 + n), lu1 = *(const f32x4*)(bl + s.n1 + n + 32);
      const int oc = n & 31;  // hidden column inside its chunk
      const int hk = wave >> 1, hq = oc >> 3, hh = oc & 7;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const f32x2 mr = *(const f32x2*)(st + 2 * (i * 16 + lc));
        const f32x4 v = (ag[i][0] - mr[0] * lu0) * mr[1] + bv0;
        const f32x4 g = (ag[i][1] - mr[0] * lu1) * mr[1] + bv1;
        f16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (f16)upk_geglu_mul(v[k], g[k]);
        const int row = i * 16 + lc;
        *(f16x4*)(hT + (hk * BM + row) * 32 + lds_swz(lc, hq) * 8 + hh) = o;
      }
    }
    __syncthreads();  // (slice p & 1 complete)
    const char* const hs = (const char*)hT + la;
    ml_static_for<NK1, S>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      f16x8 fc[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fc[i] = *(const f16x8*)(hs + ((t - NK1) * BM + i * 16) * 64);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[t % RD][j], fc[i], acc[i][j], 0, 0, 0);
      refill(tc);
      __builtin_amdgcn_sched_barrier(0);
    });
  }

  // ---- 5. the t2 chunks of the second GEMM from the resident tile; epilogue: bias, residual, GroupNorm partials
  if (!act2) return;
  f32x4 b2v[NI];
  f16x4 rr[MI][NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int n = col2 + j * 16 + lg * 4;
    b2v[j] = *(const f32x4*)(s.b2 + n);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const unsigned m = (unsigned)min(m0 + i * 16 + lc, s.M - 1);
      rr[i][j] = *(const f16x4*)(s.res + m * (unsigned)s.ldr + (unsigned)(n < s.n2 ? n : 0));
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  ml_static_for<0, NK1>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    f16x8 fc[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) fc[i] = *(const f16x8*)(xs + (t * BM + i * 16) * 64);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[t % RD][j], fc[i], acc[i][j], 0, 0, 0);
    if constexpr (t + RD < NK1) {
      ring[t % RD][0] = *(const f16x8*)(wt2 + (unsigned)(t + RD) * ks2 + loff);
      ring[t % RD][1] = *(const f16x8*)(wt2 + (unsigned)(t + RD) * ks2 + 1024 + loff);
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  f32x4 cs[NI], cq[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) cs[j] = cq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + i * 16 + lc;
    const bool ok = m < s.M;
    f16* yrow = s.y + (unsigned)(ok ? m : 0) * (unsigned)s.ldy;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col2 + j * 16 + lg * 4;
      const f32x4 v = acc[i][j] + b2v[j];
      f16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (f16)(v[k] + (float)rr[i][j][k]);
      if (ok && n < s.n2) *(f16x4*)(yrow + n) = o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = ok ? (float)o[k] : 0.f;
        cs[j][k] += f;
        cq[j][k] += f * f;
      }
    }
  }
  if (s.gn_cp) {
    const int b = m0 / s.gn_hw;
    const int blk = (m0 - b * s.gn_hw) / BM;
    float* dst = s.gn_cp + (long)((b * s.gn_nblk + blk) * 2) * s.n2pad;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col2 + j * 16 + lg * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cs[j][k] = Epi::row_sum16(cs[j][k]);
        cq[j][k] = Epi::row_sum16(cq[j][k]);
      }
      if (lc == 0) {
        *(f32x4*)(dst + n) = cs[j];
        *(f32x4*)(dst + s.n2pad + n) = cq[j];
      }
    }
  }
}

}  // namespace
}  // namespace upkd

using namespace upkd;

// rows_per_wg -> (rows, form): 32 / 64 the resident kernels, 128 and 64 | UPK_MLP_STREAM the streaming ones (0 = 64 resident)
static int mlp_form(const upk_mlp_desc* d, int* stream) {
  const int raw = d->rows_per_wg > 0 ? d->rows_per_wg : 64;
  const int bm = (raw & ~UPK_MLP_STREAM) ? (raw & ~UPK_MLP_STREAM) : 64;
  *stream = (raw & UPK_MLP_STREAM) != 0 || bm == 128;
  return bm;
}

// LDS of a launch: the resident form keeps [h | t2] (nh + nch1 chunks), the streaming form t2 and two 4-chunk slices of h
static size_t mlp_lds_bytes(int nch1, int nh, int n1, int bm, int stream) {
  return (size_t)(stream ? nch1 + 4 * ML_SLICES : nch1 + nh) * bm * 64 + (size_t)bm * 8 + (size_t)n1 * 8;
}

extern "C" int upk_geglu_mlp_supported(upk_ctx* ctx, const upk_mlp_desc* d) {
  if (!ctx || !d) return 0;
  if (d->c <= 0 || (d->c & 31) || d->inner != 4 * d->c || (d->inner & 31)) return 0;
  const int nch1 = d->c / 32, nh = d->inner / 32;
  if (nch1 % 7 || (nch1 + nh) % 7) return 0;   // (ring depth 7: the 7 * 32 channel family)
  if (d->n_pad > ML_NW * 32 || (d->n_pad & 31)) return 0;
  if ((d->ldx & 7) || (d->ld_res & 3) || (d->ldy & 3) || (d->n_out & 3)) return 0;
  int stream;
  const int bm = mlp_form(d, &stream);
  if (stream ? (bm != 64 && bm != 128) : (bm != 32 && bm != 64)) return 0;
  if ((2 * d->inner) & 255) return 0;
  if (mlp_lds_bytes(nch1, nh, 2 * d->inner, bm, stream) > 160 * 1024) return 0;  // (c = 448 at 128 rows: 114 + 64 KB)
  if (stream && nch1 != 7) return 0;  // (a pass of the streaming form is unrolled over its 7 K chunks)
  if (d->gn_stats_ws && (d->hw <= 0 || d->hw % bm || d->hw / bm > UPK_GN_MAX_CHUNKS)) return 0;
  return 1;
}

extern "C" int upk_geglu_mlp_f16(upk_ctx* ctx, const upk_mlp_desc* d, upk_stream stream_) {
  if (!ctx || !d) return UPK_EINVAL;
  if (!d->x || !d->w1 || !d->w2 || !d->b1 || !d->u1 || !d->b2 || !d->residual || !d->y)
    return upk_fail(ctx, UPK_EINVAL, "geglu_mlp: null operand");
  if (!upk_geglu_mlp_supported(ctx, d))
    return upk_fail(ctx, UPK_ESHAPE, "geglu_mlp: shape outside the fused kernel's domain (c=%d inner=%d n_pad=%d)", d->c,
                    d->inner, d->n_pad);
  hipStream_t stream = (hipStream_t)stream_;
  MlpArgs s;
  memset(&s, 0, sizeof(s));
  s.x = (const f16*)d->x, s.w1 = (const f16*)d->w1, s.w2 = (const f16*)d->w2, s.zero = (const f16*)ctx->zero_page;
  s.b1 = d->b1, s.u1 = d->u1, s.b2 = d->b2, s.res = (const f16*)d->residual, s.y = (f16*)d->y;
  s.gn_cp = d->gn_stats_ws;
  s.ldx = d->ldx, s.ldr = d->ld_res, s.ldy = d->ldy, s.M = d->m;
  s.nch1 = d->c / 32, s.n1 = 2 * d->inner, s.n2 = d->n_out, s.n2pad = d->n_pad, s.nh = d->inner / 32;
  int strm;
  const int bm = mlp_form(d, &strm);
  s.gn_hw = d->hw > 0 ? d->hw : 1;
  s.gn_nblk = d->hw > 0 ? d->hw / bm : 1;
  s.ln_inv_dim = 1.0f / (float)(d->ln_dim > 0 ? d->ln_dim : d->c);
  s.ln_eps = d->ln_eps;
#ifdef UPK_TIMELINE
  s.dbg = getenv("UPK_MLP_TL") ? (unsigned long long*)((char*)ctx->ws + ctx->ws_bytes - 4096) : nullptr;
#endif
  const size_t lds = mlp_lds_bytes(s.nch1, s.nh, s.n1, bm, strm);
  void (*fn)(const MlpArgs) = strm ? (bm == 64 ? mlp_stream_kernel<4, 7> : mlp_stream_kernel<8, 4>)
                                     : (bm == 32 ? mlp_kernel<2, 7> : mlp_kernel<4, 7>);
  static unsigned long long attr[4] = {0, 0, 0, 0};
  if (int rc = upk_lds_attr_once(ctx, (const void*)fn, &attr[strm * 2 + (bm > (strm ? 64 : 32))])) return rc;
  upk_prof_scope prof(ctx, UPK_CLS_IGEMM, stream);
  hipLaunchKernelGGL(fn, dim3((s.M + bm - 1) / bm), dim3(512), lds, stream, s);
  return upk_check_launch(ctx, "geglu_mlp");
}
