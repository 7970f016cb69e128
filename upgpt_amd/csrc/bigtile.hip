// Big-tile implicit-GEMM convolution for gfx950: the long-M launches (the VAE decoder's 3x3 convs, M = 32768 ..
// 524288 output pixels, model.py:535-568; any launch with >= one tile per CU can ask for it).
//
// Why a second family next to igemm_ws_kernel: a 128x128 block tile needs 16 KB of LDS fill per 1.05 MFLOP, i.e.
// 63 B/clk/CU at the MFMA peak — the CU's whole L2 -> LDS path — and the wave-specialised kernel sits at 25-33 % of
// the peak on those convs (profiles/r02_optrace_vae_final_32x32.txt).  Larger tiles did not fit there: with 4 loader
// and 4 MFMA waves (256 registers each) a wave's accumulator tile is a quarter of the block tile.
//   * two waves per SIMD, EVERY wave both loader and MFMA wave: 4 waves per workgroup and two workgroups per CU
//     (256x128 / 128x256 tiles) or 8 waves and one workgroup (256x256 / 512x128: 32 KB of fill per 4.2 MFLOP =
//     32 B/clk/CU at the MFMA peak); 64x128 or 128x64 accumulators per wave (128 registers), 256 registers per wave;
//   * no loader waves: every wave issues its share of the stage's LDS-DMAs (global_load_lds_dwordx4, 1 KB each: one
//     16-row group of a [rows][32 fp16] tile, XOR swizzle applied to the source chunk) and then runs its MFMAs; an
//     LDS-DMA costs its wave 60-185 issue cycles (MI355X_MICROARCH.md), which the sibling wave on the SIMD fills
//     with its own MFMAs — a one-wave-per-SIMD variant (256x256 tile, 128x128 per wave in AGPRs) was built first and
//     lost to these for exactly that reason (512 -> 512 conv at 64x64: 170 us vs 148 us);
//   * ring of NBUF stage slots (one 32-wide K chunk each), ONE s_barrier per stage: at the barrier of stage t every
//     wave has consumed stage t-1, so its slot takes stage t+NBUF-1;  waits are COUNTED (vmcnt(k P)): the younger
//     stages stay in flight across the barrier;
//   * LA (the 8-wave variants): the barrier of stage t also guarantees stage t+1, whose fragments are requested while
//     the MFMAs of stage t issue (column-major MFMA order, counted lgkmcnt) — no exposed LDS round trip;
//   * the fragment reads are inline-asm ds_read_b128 with hand-placed s_waitcnt lgkmcnt: to the compiler's counter
//     model an LDS-DMA is a FLAT access pending on both counters, and any wait it inserts itself while one is pending
//     is vmcnt(0) lgkmcnt(0) — the whole ring drained at every fragment read.
// What it reaches: 142-148 us for 154.6 GF with EVERY tile shape / ring depth on random operands and
// 115-130 us on all-zero ones — an MFMA-bound launch runs at the clock the chip sustains under its operands' switching
// power, ~1.05 PFLOP/s here.
// Same operand layout, weight packing ([K/32][n_pad][32]), tile order (tile_map), split-K slabs and epilogues
// (Epi) as igemm.hip: plain epilogues in every configuration, all others in the 4-wave ones (own instantiations) or
// through the reduce pass when K is split; no appended K segment, no fragment-side LayerNorm fold (row statistics from
// the producer are taken: IgemmArgs::lnr_in); results are bit-identical to the other families' for the same split.
#include <type_traits>

#include "igemm_common.h"

namespace upkd {
namespace {

template <int N>
__device__ __forceinline__ void bt_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int OFF>
__device__ __forceinline__ f16x8 bt_ldsr(unsigned addr) {
  f16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// wait until at most n of this wave's LDS reads are outstanding (n is a constant after unrolling)
__device__ __forceinline__ void bt_wait_lgkm(int n) {
  switch (n) {
#define BT_W(k) case k: asm volatile("s_waitcnt lgkmcnt(" #k ")" ::: "memory"); break;
    BT_W(0) BT_W(1) BT_W(2) BT_W(3) BT_W(4) BT_W(5) BT_W(6) BT_W(7) BT_W(8) BT_W(9) BT_W(10) BT_W(11) BT_W(12) BT_W(13) BT_W(14)
#undef BT_W
    default: asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory"); break;
  }
}
// the value is used only after the preceding (volatile) wait: volatile asm statements keep their order
__device__ __forceinline__ void bt_tie(f16x8& v) { asm volatile("" : "+v"(v)); }

template <int MI, int NI, int WM, int WN, int NBUF, bool LA, bool FE = false>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void igemm_bt_kernel(const IgemmArgs a) {
  constexpr int NW = WM * WN;  // waves: 4 (two workgroups per CU) or 8 (one)
  static_assert(NW == 4 || NW == 8, "two waves per SIMD");
  constexpr int BM = MI * 16 * WM, BN = NI * 16 * WN;
  constexpr int AG = BM / 16, BG = BN / 16;
  // the 16-row groups of the A and the B tile are dealt to the waves round robin.  The 7 * 32-channel family (N tiles of
  // 112 / 224 columns: 7 / 14 groups) does not divide by the wave count: every wave still issues P DMAs per stage — the
  // waits are COUNTED — and the surplus ones of the waves with fewer groups fetch the zero page into a 1 KiB dump row group
  // behind the ring (as the wave-specialised loaders of igemm.hip do)
  constexpr int AGW = (AG + NW - 1) / NW, BGW = (BG + NW - 1) / NW, P = AGW + BGW;  // DMAs per wave per stage
  constexpr bool UNEVEN = (AG % NW != 0) || (BG % NW != 0);
  constexpr int DUMP = UNEVEN ? 512 : 0;
  constexpr int ROWS = BM + BN;
  constexpr int STAGE = ROWS * 32;    // halfs per ring slot (one K chunk)
  constexpr int L = LA ? 1 : 0;         // look-ahead: the barrier of stage t also guarantees stage t + 1
  constexpr int KEEP = NBUF - 2 - L;    // stages that may stay in flight across a barrier
  static_assert(KEEP >= 1 && KEEP <= 2 && (KEEP + 1) * P <= 63, "vmcnt range");
  static_assert(MI + NI - 1 <= 15, "lgkmcnt range");
  static_assert(BM * 64 + (NI - 1) * 1024 < 65536, "ds_read offsets");
  static_assert((NBUF * STAGE + DUMP) * 2 <= 160 * 1024, "LDS");
  static_assert(WM * WN * NI * 32 * 4 <= NBUF * STAGE * 2, "tile_plain_cp scratch");
  __shared__ __attribute__((aligned(16))) f16 smem[NBUF * STAGE + DUMP];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tm, tn, zs;
  if (!tile_map(a, tm, tn, zs)) return;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kc0 = zs * a.chunks_per_split;
  const int kc1 = min(a.nchunks, kc0 + a.chunks_per_split);
  const int nstages = kc1 - kc0;
  const int ph = ph_id(a);

  // ---------------- loader state: this wave's 16-row groups rg = wave + NW i of the A and of the B tile ----------------
  const int r16 = lane >> 2;
  const int chd = (lane & 3) ^ ((-(lane >> 4)) & 3);  // source chunk of this lane (LDS-DMA writes lane-linear)
  const f16* const zsrc = a.zero + (lane & 3) * 8;
  int a_oy[AGW], a_ox[AGW], a_b[AGW];
  const int HoWo = a.Ho * a.Wo;
#pragma unroll
  for (int i = 0; i < AGW; ++i) {
    const int m = m0 + (wave + NW * i) * 16 + r16;
    const bool ok = m < a.M && (!UNEVEN || wave + NW * i < AG);
    const int mm = ok ? m : 0;
    if (a.linear) {
      a_b[i] = 0;
      a_oy[i] = ok ? 0 : -(1 << 20);  // (rows past M: never a valid pixel)
      a_ox[i] = mm;
    } else {
      const int b = div_hw(a, mm, HoWo);
      const int p = mm - b * HoWo;
      const int oy = div_w(a, p);
      a_b[i] = b;
      a_oy[i] = ok ? oy * a.stride - (a.ph_on ? 1 - (ph >> 1) : a.pad_lo) : -(1 << 20);
      a_ox[i] = (p - oy * a.Wo) * a.stride - (a.ph_on ? 1 - (ph & 1) : a.pad_lo);
    }
  }
  // source rows of the current tap in both sources of the channel concat; nullptr: out of the image / past M (the
  // zero page is fetched instead)
  const f16* ap1[AGW];
  const f16* ap2[AGW];
  const int sc1 = a.c1, ctot = a.c1 + a.c2;
  auto set_tap = [&](int ky, int kx) {
#pragma unroll
    for (int i = 0; i < AGW; ++i) {
      int iy = a_oy[i] + ky;
      int ix = a_ox[i] + kx;
      const bool ok = a.linear ? (iy >= 0) : (iy >= 0 && iy < a.HL && ix >= 0 && ix < a.WL);
      if (a.ups) {
        iy >>= 1;
        ix >>= 1;
      }
      const long pix = ((long)a_b[i] * a.HS + iy) * a.WS + ix;
      ap1[i] = ok ? a.x1 + pix * a.ld1 + chd * 8 : nullptr;
      ap2[i] = ok ? (a.x2 ? a.x2 + pix * a.ld2 + chd * 8 - sc1 : a.x1) : nullptr;
    }
  };
  int cur_kc = kc0, cur_c0, cur_ky, cur_kx;
  {
    const int tap = kc0 / a.cpt;
    cur_c0 = (kc0 - tap * a.cpt) * 32;
    cur_ky = tap / a.ks;
    cur_kx = tap - cur_ky * a.ks;
    set_tap(cur_ky, cur_kx);
  }
  const f16* bp[BGW];
#pragma unroll
  for (int i = 0; i < BGW; ++i) {
    const int row = (wave + NW * i) * 16 + r16;
    const bool ok = n0 + row < a.npad && (!UNEVEN || wave + NW * i < BG);
    bp[i] = ok ? a.w + (long)ph * a.ph_wstride + ((long)kc0 * a.npad + n0 + row) * 32 + chd * 8 : nullptr;
  }
  const long wstep = (long)a.npad * 32;

  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* glb_ptr;
  auto issue_stage = [&](int slot) {
    f16* base = smem + slot * STAGE;
    const bool second = cur_c0 >= sc1;
#pragma unroll
    for (int i = 0; i < AGW; ++i) {
      const f16* p = second ? ap2[i] : ap1[i];
      const f16* src = p ? p + cur_c0 : zsrc;
      f16* dst = base + (wave + NW * i) * 16 * 32;
      if constexpr (UNEVEN) dst = (wave + NW * i < AG) ? dst : smem + NBUF * STAGE;  // (wave-uniform)
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)dst, 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BGW; ++i) {
      const f16* src = bp[i] ? bp[i] : zsrc;
      f16* dst = base + (BM + (wave + NW * i) * 16) * 32;
      if constexpr (UNEVEN) dst = (wave + NW * i < BG) ? dst : smem + NBUF * STAGE;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)dst, 16, 0, 0);
      if (bp[i]) bp[i] += wstep;
    }
    ++cur_kc;
    cur_c0 += 32;
    if (cur_c0 == ctot) {
      cur_c0 = 0;
      if (++cur_kx == a.ks) {
        cur_kx = 0;
        ++cur_ky;
      }
      if (cur_kc < kc1) set_tap(cur_ky, cur_kx);
    }
  };

  // ---------------- MFMA state ----------------
  const int wm = wave / WN, wn = wave - wm * WN;
  const int lg = lane >> 4, lc = lane & 15;
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  typedef __attribute__((address_space(3))) f16* lds_f16p;
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_f16p)smem;
  const unsigned frag_b = (unsigned)(lc * 32 + lds_swz(lc, lg) * 8) * 2u;
  const unsigned a_addr = lds0 + (unsigned)(wm * MI * 16) * 64u + frag_b;
  const unsigned b_addr = lds0 + (unsigned)(BM + wn * NI * 16) * 64u + frag_b;
  f16x8 fa[LA ? 2 : 1][MI], fb[NI];
#if defined(UPK_DEV)
#pragma unroll
  for (int i = 0; i < MI; ++i) fa[0][i] = fa[LA ? 1 : 0][i] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NI; ++j) fb[j] = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
#endif
  typedef std::integral_constant<int, 0> I0;
  typedef std::integral_constant<int, 1> I1;
#define BT_RD(dst, n, base, k) \
  if constexpr (k < n) dst[k < n ? k : 0] = bt_ldsr<k * 1024>(base)
  auto read_a = [&](auto SET, int t) {  // the MI A-row fragments of stage t
    constexpr int s = decltype(SET)::value;
    const unsigned aa = a_addr + (unsigned)(t % NBUF) * (unsigned)(STAGE * 2);
    BT_RD(fa[s], MI, aa, 0); BT_RD(fa[s], MI, aa, 1); BT_RD(fa[s], MI, aa, 2); BT_RD(fa[s], MI, aa, 3);
    BT_RD(fa[s], MI, aa, 4); BT_RD(fa[s], MI, aa, 5); BT_RD(fa[s], MI, aa, 6); BT_RD(fa[s], MI, aa, 7);
  };
  auto read_b_all = [&](int t) {  // the NI B-column fragments of stage t
    const unsigned ba = b_addr + (unsigned)(t % NBUF) * (unsigned)(STAGE * 2);
    BT_RD(fb, NI, ba, 0); BT_RD(fb, NI, ba, 1); BT_RD(fb, NI, ba, 2); BT_RD(fb, NI, ba, 3);
    BT_RD(fb, NI, ba, 4); BT_RD(fb, NI, ba, 5); BT_RD(fb, NI, ba, 6); BT_RD(fb, NI, ba, 7);
  };
#undef BT_RD
  auto read_b = [&](int j, unsigned ba) {  // (j is a constant after unrolling)
    switch (j) {
#define BT_RB(k) case k: fb[k < NI ? k : 0] = bt_ldsr<k * 1024>(ba); break;
      BT_RB(0) BT_RB(1) BT_RB(2) BT_RB(3) BT_RB(4) BT_RB(5) BT_RB(6) BT_RB(7)
#undef BT_RB
    }
  };

  // one stage: barrier (stage t landed everywhere, stage t-1 consumed everywhere), refill of that slot, matrix work.
  // An LDS-DMA holds its wave at issue while the CU's fill path is busy (the K loop moves 24-40 KB per stage at the
  // CU's 40-50 B/clk), and a wave issues in order: its MFMAs wait behind its DMAs.  With 8 waves, waves w and w + 4
  // share a SIMD (waves are dealt to the SIMDs cyclically): the first four refill BEFORE their MFMAs, the last four
  // AFTER, so that on every SIMD one wave's DMA issue runs under the other's matrix work.
  const bool early = NW == 4 || wave < NW / 2;
  int issued = 0;
  for (; issued < NBUF - 1 && issued < nstages; ++issued) issue_stage(issued);
  auto top = [&](int t) {  // counted wait + barrier in front of stage t
    const int last = min(t + L, nstages - 1);  // youngest stage that must have landed
    const int keep = issued - 1 - last;        // younger stages of this wave still allowed in flight
    if (keep >= 2 && KEEP >= 2) bt_wait_vm<(KEEP >= 2 ? 2 : 0) * P>();
    else if (keep == 1) bt_wait_vm<P>();
    else bt_wait_vm<0>();
    __builtin_amdgcn_s_barrier();
  };
  auto refill = [&]() {
    if (issued < nstages) {
      if (!ABL_ON(ABL_NOGLOAD)) issue_stage(issued % NBUF);
      ++issued;
    }
  };
  if constexpr (LA) {
    // Look-ahead: the fragments of stage t+1 are requested while the MFMAs of stage t issue, so that no wave ever
    // waits for an LDS round trip with an idle MFMA pipe (phase ablation, v512: MFMA + LDS reads without look-ahead
    // 137 us, MFMA alone 90 us, reads alone 54 us).  Column-major MFMA order: the MI A fragments live for the whole
    // stage (two register sets), B column j is dead after its MI MFMAs and is re-requested for stage t+1 at once.
    // LDS reads return in order, so "fragment landed" is a COUNT: behind B column j of stage t there are always the
    // NI-1-j later columns of stage t, the MI A fragments and the first j columns of stage t+1 = MI + NI - 1 reads.
    {
      const int keep = issued - 1;  // stage 0 landed
      if (keep >= 2) bt_wait_vm<2 * P>();
      else if (keep == 1) bt_wait_vm<P>();
      else bt_wait_vm<0>();
      __builtin_amdgcn_s_barrier();
      if (!ABL_ON(ABL_NOLDSW)) {
        read_a(I0(), 0);
        read_b_all(0);
      }
    }
    // (the last stage requests "stage nstages" too — stale bytes of a ring slot, never used: one wait count for every
    // stage instead of a peeled tail; the requests are drained behind the loop)
    auto stage = [&](auto CUR, int t) {
      constexpr int c = decltype(CUR)::value;
      typedef std::integral_constant<int, c ^ 1> NXT;
      top(t);
      if (early) refill();
      const unsigned ba = b_addr + (unsigned)((t + 1) % NBUF) * (unsigned)(STAGE * 2);
      if (!ABL_ON(ABL_NOLDSW)) read_a(NXT(), t + 1);
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        bt_wait_lgkm(MI + NI - 1);
        if (j == 0) {
#pragma unroll
          for (int i = 0; i < MI; ++i) bt_tie(fa[c][i]);
        }
        bt_tie(fb[j]);
        if (!ABL_ON(ABL_NOMFMA)) {
#pragma unroll
          for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[c][i], acc[i][j], 0, 0, 0);
        }
        if (!ABL_ON(ABL_NOLDSW)) {
          __builtin_amdgcn_sched_barrier(0);  // (the request follows the MFMAs that read the old column)
          read_b(j, ba);
        }
      }
      if (!early) {
        __builtin_amdgcn_sched_barrier(0);
        refill();
      }
    };
    for (int t = 0; t < nstages; t += 2) {
      stage(I0(), t);
      if (t + 1 < nstages) stage(I1(), t + 1);
    }
    bt_wait_lgkm(0);
  } else {
    for (int t = 0; t < nstages; ++t) {
      top(t);
      if (early) refill();
      if (!ABL_ON(ABL_NOLDSW)) {
        read_b_all(t);
        read_a(I0(), t);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        bt_wait_lgkm(MI - 1 - i);
        if (i == 0) {
#pragma unroll
          for (int j = 0; j < NI; ++j) bt_tie(fb[j]);
        }
        bt_tie(fa[0][i]);
        if (!ABL_ON(ABL_NOMFMA)) {
#pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[0][i], acc[i][j], 0, 0, 0);
        }
      }
      if (!early) {
        __builtin_amdgcn_sched_barrier(0);
        refill();
      }
    }
  }
  __builtin_amdgcn_s_barrier();  // (the epilogue may reuse the ring)
  if ABL_ON(ABL_NOEPI) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (t == 123.456f) ((float*)a.y)[0] = t;
    return;
  }

  const int mw = m0 + wm * (MI * 16);
  const int nw = n0 + wn * (NI * 16);
  if (a.lnr_in) Epi::lnr_fix<MI, NI>(a, mw, nw, lc, lg, acc);
  if (a.partial) {
    slab_t* slab = (slab_t*)a.partial + ((long)zs * (a.ph_on ? 4 : 1) + ph) * a.M * a.npad;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = mw + i * 16 + lc;
      if (m >= a.M) continue;
      const unsigned roff = (unsigned)m * (unsigned)a.npad;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = nw + j * 16 + lg * 4;
        if (n < a.npad) slab_store(slab + roff + n, acc[i][j]);
      }
    }
    return;
  }
  if constexpr (FE) {
    // every epilogue of the shared Epi::tile (SiLU / quick-GELU, fp32 / NCHW output, transposed V tail, GEGLU): its
    // own instantiation — compiled into the kernels above, the general per-fragment path costs their K loops 5-50 %
    // (registers live across the loop; 512 -> 512 at 64x64: 144 -> 152 us on the 4-wave, -> 219 us on the 8-wave tiles)
    Epi::tile<MI, NI, WM, WN>(a, m0, mw, nw, lc, lg, acc, wm, wn, (float*)smem, a.M);
  } else {
    // plain epilogues (bias + timestep row vector + residual -> fp16 NHWC, optionally with the GroupNorm channel
    // partials or the LayerNorm row sums of what is stored); anything else goes to the FE instantiation of the
    // configuration, or — when K is split — to the reduce pass
    if (a.gn_cp) Epi::tile_plain_cp<MI, NI, WM, WN>(a, m0, mw, nw, lc, lg, acc, wm, wn, (float*)smem, a.M);
    else if (a.lnr_out) Epi::tile_plain_lnr<MI, NI>(a, mw, nw, lc, lg, acc, a.M);
    else Epi::tile_plain<MI, NI>(a, mw, nw, lc, lg, acc, a.M);
  }
}

struct BtCfg {
  int mi, ni, wm, wn, nbuf;
  const char* name;
  void (*fn)(const IgemmArgs);
  void (*fn_fe)(const IgemmArgs);  // instantiation with every epilogue, or nullptr
};
#define BTC(MI, NI, WM, WN, NB, LA) \
  {MI, NI, WM, WN, NB, "bt" #MI "x" #NI "x" #WM "x" #WN "n" #NB, igemm_bt_kernel<MI, NI, WM, WN, NB, LA>, nullptr}
#define BTCF(MI, NI, WM, WN, NB, LA) \
  {MI, NI, WM, WN, NB, "bt" #MI "x" #NI "x" #WM "x" #WN "n" #NB, igemm_bt_kernel<MI, NI, WM, WN, NB, LA>, \
   igemm_bt_kernel<MI, NI, WM, WN, NB, LA, true>}
const BtCfg kBt[] = {
    // 4 waves, two workgroups per CU (72 KB rings); also instantiated with the general epilogue
    BTCF(8, 4, 2, 2, 3, false),  // 256x128
    BTCF(4, 8, 2, 2, 3, false),  // 128x256
    BTCF(4, 8, 4, 1, 3, false),  // 256x128 (wave 64x128: A rows private, B shared)
    // 8 waves, one workgroup per CU, fragments of the next stage read ahead
    BTC(4, 8, 4, 2, 4, true),  // 256x256, 128 KB ring
    BTC(8, 4, 2, 4, 4, true),  // 256x256 (wave 128x64)
    BTC(4, 8, 8, 1, 4, true),  // 512x128, 160 KB ring (N = 128 layers)
    BTC(4, 4, 4, 2, 4, true),  // 256x128,  96 KB ring (wave 64x64)
    // (224 / 112-column tiles for the UNet's 7 * 32-channel family were tried and were slower by chip time on every UNet
    // shape, DESIGN.md 14b: with 64-workgroup launches on four lanes there is one workgroup per CU; not kept)
};
constexpr int kNumBt = sizeof(kBt) / sizeof(kBt[0]);

}  // namespace

int bt_num_configs() { return kNumBt; }
const char* bt_config_name(int c) { return (c >= 0 && c < kNumBt) ? kBt[c].name : "?"; }

// Geometry of configuration `c`; false = the launch in `a` (filled by conv_plan) at split-K factor `splitk` is outside the
// family's domain: an appended K segment, a fragment-side LayerNorm fold, an epilogue that is not plain where K is not
// split and the configuration has no general-epilogue instantiation, GEGLU on waves narrower than 64 columns
bool bt_plan(const upk_ctx* ctx, const IgemmArgs& a, int c, int splitk, BtPlan* pl) {
  if (c < 0 || c >= kNumBt) return false;
  const BtCfg& k = kBt[c];
  *pl = {k.mi * 16 * k.wm, k.ni * 16 * k.wn, k.wm * k.wn == 4 ? 2 : 1, k.mi, k.ni, k.wn, k.wm * k.wn * 64};
  if (a.x3 || (a.ln_u && !a.lnr_in) || !splitk_fits(ctx, a, splitk)) return false;
  if (splitk == 1 && !Epi::plain(a) && !k.fn_fe) return false;
  return !(a.flags & UPK_F_GEGLU) || (k.ni * 16) % 64 == 0;
}
int bt_launch(upk_ctx* ctx, const IgemmArgs& a, int c, dim3 grid, dim3 block, hipStream_t stream) {
  // (split launches write partial slabs: no epilogue in the kernel)
  const bool fe = !a.partial && !Epi::plain(a);
  if (fe && !kBt[c].fn_fe) return upk_fail(ctx, UPK_ESHAPE, "conv: %s has no general-epilogue instantiation", kBt[c].name);
  hipLaunchKernelGGL(fe ? kBt[c].fn_fe : kBt[c].fn, grid, block, 0, stream, a);
  return upk_check_launch(ctx, "igemm_bt");
}

}  // namespace upkd
