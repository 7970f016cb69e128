// upk_region_mask_u8 + upk_composite_u8: the two per-pixel passes of a region-locked edit.
//
// upk_region_mask_u8: a human-parsing label map and a set of labels -> the picture-resolution edit mask (the selected
// pixels dilated by a Chebyshev window of radius `dilate`), the latent-resolution keep-mask the sampler takes
// (1 keeps x0) and the number of cells that are edited.
// upk_composite_u8: the generated picture blended into the original under the box-feathered mask, on the bytes.
//
// Integers only in both: no result depends on an order of evaluation.  Both work on BIT ROWS.  A wave reads 64 adjacent
// bytes of a row and one ballot turns the 64 predicates (label selected / mask byte non-zero) into one 64-bit word in
// LDS (stage_bits; stage_bits16 for maps that allow 16-byte loads); a window then is a handful of word operations
// instead of (2 r + 1)^2 byte reads:
//   dilation      V[y] = OR of the bit rows y - r .. y + r (word-wise), M(y, x) = any bit of V[y] in [x - r, x + r]
//   box count     Hs(y, x) = popcount of the bit row in [x - fr, x + fr] (edge replication: the columns beyond an end
//                 count as that end's bit), kept as a byte (<= 33); s(y, x) = sum of 2 fr + 1 such bytes down a column,
//                 four columns per LDS dword, summed in two 2 x 16-bit accumulators (<= 1089 each)
// One workgroup = a band of RG_BAND = 16 rows of one picture: the bit rows its window covers, a barrier, the vertical
// pass, a barrier, the band's bytes (and the band's cells: 16 is a multiple of every factor, a cell never straddles two
// workgroups).  Rows outside the picture are zero rows for the dilation and the clamped row for the composite.
//
// cells[b] is WRITTEN, so no workgroup may accumulate into it: the workgroup after the last band of a sample counts that
// sample's cells on its own, from the bit rows of the whole map (a cell is edited when a selected pixel lies in its block
// grown by r on every side), in parallel with the bands.  It exists only when `cells` is asked for.
#include "common.h"

namespace {

constexpr int RG_THREADS = 1024;
constexpr int RG_BAND = 16;             // rows per workgroup: a multiple of every factor
constexpr int RG_LDS_BYTES = 64 * 1024;  // staging budget
constexpr int RG_MAX_DILATE = 32;
constexpr int RG_MAX_FEATHER = 16;
constexpr int RG_UNROLL = 4;            // rows of bytes in flight per wave while staging

typedef unsigned long long u64;

// bits[t], t = j * words + q: bit i = test(byte (64 q + i) of row j); row(j) == nullptr is a row of zeros
template <class Row, class Test>
__device__ __forceinline__ void stage_bits(u64* bits, int nrows, int words, int w, Row row, Test test) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int n = nrows * words;
  for (int t0 = wave; t0 < n; t0 += RG_UNROLL * nw) {  // (uniform per wave: every lane meets every ballot)
    uint32_t v[RG_UNROLL];
    bool ok[RG_UNROLL];
#pragma unroll
    for (int u = 0; u < RG_UNROLL; ++u) {
      const int t = t0 + u * nw;
      v[u] = 0, ok[u] = false;
      if (t < n) {
        const int j = t / words, x = 64 * (t - j * words) + lane;
        const uint8_t* p = row(j);
        if (p && x < w) v[u] = p[x], ok[u] = true;
      }
    }
#pragma unroll
    for (int u = 0; u < RG_UNROLL; ++u) {
      const int t = t0 + u * nw;
      const u64 m = __ballot(ok[u] && test(v[u]));
      if (t < n && lane == 0) bits[t] = m;
    }
  }
}

// The same from 16-byte loads, for maps whose rows allow them (w, the base address, the pitch and the sample stride
// multiples of 16): a lane tests its 16 bytes and ORs the 16 bits into their word, an LDS atomic on zeroed words (an
// integer OR: its order changes nothing).  A quarter of the instructions of the ballot form per byte, and lanes whose
// bytes are all outside the set, most of a label map, write nothing.  Every thread of the workgroup calls it (barrier).
template <class Row, class Test>
__device__ __forceinline__ void stage_bits16(u64* bits, int nrows, int words, int w, Row row, Test test) {
  for (int i = threadIdx.x; i < nrows * words; i += blockDim.x) bits[i] = 0;
  __syncthreads();
  const int per_row = w >> 4;
  for (int i = threadIdx.x; i < nrows * per_row; i += blockDim.x) {
    const int j = i / per_row, x = 16 * (i - j * per_row);
    const uint8_t* p = row(j);
    if (!p) continue;
    const uint4 v = *(const uint4*)(p + x);
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) m |= (uint32_t)test((d[q] >> (8 * k)) & 0xffu) << (4 * q + k);
    if (m) atomicOr(&bits[j * words + (x >> 6)], (u64)m << (x & 63));
  }
}
template <class Row, class Test>
__device__ __forceinline__ void stage(bool vec16, u64* bits, int nrows, int words, int w, Row row, Test test) {
  if (vec16) stage_bits16(bits, nrows, words, w, row, test);
  else stage_bits(bits, nrows, words, w, row, test);
}

// the bits of word k that lie in columns [lo, hi] (the caller passes a k with 64 k <= hi and 64 k + 63 >= lo)
__device__ __forceinline__ u64 word_range(int lo, int hi, int k) {
  const int a = max(lo - 64 * k, 0), b = min(hi - 64 * k, 63);
  return (~0ull >> (63 - b)) & (~0ull << a);
}
__device__ __forceinline__ bool any_bits(const u64* row, int lo, int hi) {  // 0 <= lo <= hi < w
  u64 acc = 0;
  for (int k = lo >> 6; k <= hi >> 6; ++k) acc |= row[k] & word_range(lo, hi, k);
  return acc != 0;
}
__device__ __forceinline__ int count_bits(const u64* row, int lo, int hi) {
  int n = 0;
  for (int k = lo >> 6; k <= hi >> 6; ++k) n += __popcll(row[k] & word_range(lo, hi, k));
  return n;
}

struct RegionArgs {
  const uint8_t* segm;
  uint8_t* mask;
  float* keep;
  int32_t* cells;
  long segm_pitch, segm_ss, mask_pitch, mask_ss;
  int h, w, r, f, words, bands, vec, vec16;
  uint32_t sel[8];
};

__global__ __launch_bounds__(RG_THREADS) void region_mask_kernel(const RegionArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds64[];
  __shared__ uint32_t sel[8];
  __shared__ int n_cells;
  const int b = blockIdx.y, words = a.words, r = a.r, f = a.f;
  if (threadIdx.x < 8) {
    const uint32_t* s = a.sel;
    sel[threadIdx.x] = s[threadIdx.x];
  }
  if (threadIdx.x == 0) n_cells = 0;
  __syncthreads();
  const uint8_t* sg = a.segm + (long)b * a.segm_ss;
  auto selected = [&](uint32_t l) { return ((sel[l >> 5] >> (l & 31)) & 1u) != 0; };
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cw = a.w / f;

  if ((int)blockIdx.x == a.bands) {  // the sample's cell count
    u64* bits = lds64;                      // [h][words]
    u64* grown = lds64 + (long)a.h * words;  // [h / f][words]: OR of the rows a cell row's blocks reach
    const int ch = a.h / f;
    stage(a.vec16, bits, a.h, words, a.w, [&](int j) { return sg + (long)j * a.segm_pitch; }, selected);
    __syncthreads();
    for (int i = threadIdx.x; i < ch * words; i += RG_THREADS) {
      const int cy = i / words, q = i - cy * words;
      const int lo = max(cy * f - r, 0), hi = min(cy * f + f - 1 + r, a.h - 1);
      u64 acc = 0;
      for (int y = lo; y <= hi; ++y) acc |= bits[y * words + q];
      grown[i] = acc;
    }
    __syncthreads();
    int n = 0;
    for (int i = threadIdx.x; i < ch * cw; i += RG_THREADS) {
      const int cy = i / cw, cx = i - cy * cw;
      n += any_bits(grown + cy * words, max(cx * f - r, 0), min(cx * f + f - 1 + r, a.w - 1));
    }
    if (n) atomicAdd(&n_cells, n);  // (an integer sum in LDS: its order changes nothing)
    __syncthreads();
    if (threadIdx.x == 0) a.cells[b] = n_cells;
    return;
  }

  const int y0 = blockIdx.x * RG_BAND, rows = min(RG_BAND, a.h - y0);
  u64* bits = lds64;                                      // [rows + 2 r][words]: picture rows y0 - r ..
  u64* vert = lds64 + (long)(RG_BAND + 2 * r) * words;  // [rows][words]: V
  u64* dil = vert + RG_BAND * words;                      // [rows][words]: M
  stage(a.vec16, bits, rows + 2 * r, words, a.w,
        [&](int j) {
          const int y = y0 - r + j;
          return (y >= 0 && y < a.h) ? sg + (long)y * a.segm_pitch : (const uint8_t*)nullptr;
        },
        selected);
  __syncthreads();
  for (int i = threadIdx.x; i < rows * words; i += RG_THREADS) {
    const int ry = i / words, q = i - ry * words;
    u64 acc = 0;
    for (int j = ry; j <= ry + 2 * r; ++j) acc |= bits[j * words + q];
    vert[i] = acc;
  }
  __syncthreads();
  for (int t = wave; t < rows * words; t += RG_THREADS / 64) {  // (uniform per wave)
    const int ry = t / words, x = 64 * (t - ry * words) + lane;
    const bool m = x < a.w && any_bits(vert + ry * words, max(x - r, 0), min(x + r, a.w - 1));
    const u64 word = __ballot(m);
    if (lane == 0) dil[t] = word;
  }
  __syncthreads();

  if (a.mask) {
    uint8_t* mk = a.mask + (long)b * a.mask_ss;
    const int wq = (a.w + 3) >> 2;
    for (int i = threadIdx.x; i < rows * wq; i += RG_THREADS) {
      const int ry = i / wq, x = 4 * (i - ry * wq);
      const uint32_t four = (uint32_t)(dil[ry * words + (x >> 6)] >> (x & 63)) & 0xfu;  // (x is a multiple of 4)
      uint8_t* o = mk + (long)(y0 + ry) * a.mask_pitch + x;
      if (a.vec && x + 3 < a.w) {
        *(uint32_t*)o = (four & 1u ? 0xffu : 0u) | (four & 2u ? 0xff00u : 0u) | (four & 4u ? 0xff0000u : 0u) |
                        (four & 8u ? 0xff000000u : 0u);
      } else {
        for (int j = 0; j < 4 && x + j < a.w; ++j) o[j] = (four >> j) & 1u ? 255 : 0;
      }
    }
  }
  if (a.keep) {
    float* kp = a.keep + (long)b * (a.h / f) * cw;
    const u64 ones = f == 64 ? ~0ull : (1ull << f) - 1;
    for (int i = threadIdx.x; i < (rows / f) * cw; i += RG_THREADS) {
      const int cr = i / cw, cx = i - cr * cw;
      const int x = cx * f;  // (f divides 64: a cell's columns lie in one word)
      u64 acc = 0;
      for (int ry = cr * f; ry < cr * f + f; ++ry) acc |= (dil[ry * words + (x >> 6)] >> (x & 63)) & ones;
      kp[(long)(y0 / f + cr) * cw + cx] = acc ? 0.0f : 1.0f;
    }
  }
}

struct CompArgs {
  const uint8_t *orig, *gen, *mask;
  uint8_t *out, *alpha;
  long orig_pitch, orig_ss, gen_pitch, gen_ss, mask_pitch, mask_ss, out_pitch, out_ss, alpha_pitch, alpha_ss;
  int h, w, fr, words, w4, vec, vec16;
};

__device__ __forceinline__ uint32_t blend8(uint32_t a, uint32_t g, uint32_t o) { return (a * g + (255u - a) * o + 127u) / 255u; }

__global__ __launch_bounds__(RG_THREADS) void composite_kernel(const CompArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 lds64[];
  const int b = blockIdx.y, words = a.words, fr = a.fr, w4 = a.w4;
  const int y0 = blockIdx.x * RG_BAND, rows = min(RG_BAND, a.h - y0);
  const int nst = rows + 2 * fr;  // staged row j = picture row clamp(y0 - fr + j): the window of output row ry is j = ry .. ry + 2 fr
  u64* bits = lds64;                                                       // [nst][words]
  uint8_t* hs = (uint8_t*)(lds64 + (long)(RG_BAND + 2 * fr) * words);  // [nst][w4]: horizontal counts
  const uint8_t* mk = a.mask + (long)b * a.mask_ss;
  stage(a.vec16, bits, nst, words, a.w, [&](int j) { return mk + (long)min(max(y0 - fr + j, 0), a.h - 1) * a.mask_pitch; },
        [](uint32_t v) { return v != 0; });
  __syncthreads();
  for (int i = threadIdx.x; i < nst * w4; i += RG_THREADS) {
    const int j = i / w4, x = i - j * w4;
    int n = 0;
    if (x < a.w) {
      const u64* row = bits + j * words;
      const int lo = x - fr, hi = x + fr;
      n = count_bits(row, max(lo, 0), min(hi, a.w - 1));
      if (lo < 0) n += -lo * (int)(row[0] & 1u);
      if (hi > a.w - 1) n += (hi - (a.w - 1)) * (int)((row[(a.w - 1) >> 6] >> ((a.w - 1) & 63)) & 1u);
    }
    hs[i] = (uint8_t)n;
  }
  __syncthreads();

  const uint32_t side = 2u * fr + 1u, area = side * side;
  const uint8_t* og = a.orig + (long)b * a.orig_ss;
  const uint8_t* gn = a.gen + (long)b * a.gen_ss;
  uint8_t* out = a.out + (long)b * a.out_ss;
  uint8_t* al = a.alpha ? a.alpha + (long)b * a.alpha_ss : nullptr;
  const int wq = w4 >> 2;
  for (int i = threadIdx.x; i < rows * wq; i += RG_THREADS) {
    const int ry = i / wq, x = 4 * (i - ry * wq);
    uint32_t even = 0, odd = 0;  // columns x, x + 2 | x + 1, x + 3 as 2 x 16 bits
    for (int j = ry; j <= ry + 2 * fr; ++j) {
      const uint32_t v = *(const uint32_t*)(hs + j * w4 + x);
      even += v & 0x00ff00ffu, odd += (v >> 8) & 0x00ff00ffu;
    }
    const uint32_t s[4] = {even & 0xffffu, odd & 0xffffu, even >> 16, odd >> 16};
    uint32_t A[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) A[j] = (255u * s[j] + area / 2u) / area;
    const long y = y0 + ry;
    const uint8_t* po = og + y * a.orig_pitch + 3L * x;
    const uint8_t* pg = gn + y * a.gen_pitch + 3L * x;
    uint8_t* pd = out + y * a.out_pitch + 3L * x;
    if (a.vec && x + 3 < a.w) {
      uint32_t d[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint32_t vo = ((const uint32_t*)po)[q], vg = ((const uint32_t*)pg)[q];
        d[q] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int byte = 4 * q + k;  // pixel byte / 3 of the group
          d[q] |= blend8(A[byte / 3], (vg >> (8 * k)) & 0xffu, (vo >> (8 * k)) & 0xffu) << (8 * k);
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) ((uint32_t*)pd)[q] = d[q];
      if (al) *(uint32_t*)(al + y * a.alpha_pitch + x) = A[0] | A[1] << 8 | A[2] << 16 | A[3] << 24;
    } else {
      for (int j = 0; j < 4 && x + j < a.w; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pd[3 * j + c] = (uint8_t)blend8(A[j], pg[3 * j + c], po[3 * j + c]);
        if (al) al[y * a.alpha_pitch + x + j] = (uint8_t)A[j];
      }
    }
  }
}

// the bytes [lo, hi) a pitched batch touches (sample stride of any sign)
struct Extent {
  uintptr_t lo, hi;
};
Extent extent_of(const void* p, long long pitch, long long ss, int batch, int h, long long row_bytes) {
  const long long span = (long long)(batch - 1) * ss;
  const uintptr_t base = (uintptr_t)p;
  Extent e;
  e.lo = base + (uintptr_t)(span < 0 ? span : 0);
  e.hi = base + (uintptr_t)((span > 0 ? span : 0) + (long long)(h - 1) * pitch + row_bytes);
  return e;
}
bool overlap(const Extent& x, const Extent& y) { return x.lo < y.hi && y.lo < x.hi; }

}  // namespace

extern "C" int upk_region_mask_u8(upk_ctx* ctx, const uint8_t* segm, long long segm_pitch, long long segm_sample_stride,
                                  int batch, int h, int w, const uint32_t* label_sel_host, int dilate, int factor,
                                  uint8_t* mask_u8, long long mask_pitch, long long mask_sample_stride, float* keep,
                                  int32_t* cells, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!segm || !label_sel_host) return upk_fail(ctx, UPK_EINVAL, "region_mask: null label map or label set");
  if (!mask_u8 && !keep && !cells) return upk_fail(ctx, UPK_EINVAL, "region_mask: no output");
  if (batch <= 0 || h <= 0 || w <= 0) return upk_fail(ctx, UPK_EINVAL, "region_mask: sizes must be positive");
  if (dilate < 0 || dilate > RG_MAX_DILATE)
    return upk_fail(ctx, UPK_EINVAL, "region_mask: dilate %d, 0 .. %d are supported", dilate, RG_MAX_DILATE);
  if (factor != 1 && factor != 2 && factor != 4 && factor != 8 && factor != 16)
    return upk_fail(ctx, UPK_EINVAL, "region_mask: factor %d, one of 1, 2, 4, 8, 16", factor);
  if (h % factor || w % factor)
    return upk_fail(ctx, UPK_EINVAL, "region_mask: %d x %d is not a multiple of factor %d", h, w, factor);
  if (segm_pitch < (long long)w) return upk_fail(ctx, UPK_EINVAL, "region_mask: label map pitch %lld below w = %d", segm_pitch, w);
  if (mask_u8 && mask_pitch < (long long)w) return upk_fail(ctx, UPK_EINVAL, "region_mask: mask pitch %lld below w = %d", mask_pitch, w);
  if (((uintptr_t)keep | (uintptr_t)cells) & 3) return upk_fail(ctx, UPK_EINVAL, "region_mask: keep and cells must be 4-byte aligned");
  if (batch > 65535) return upk_fail(ctx, UPK_ESHAPE, "region_mask: batch %d above 65535", batch);
  const long long segm_ss = batch > 1 ? segm_sample_stride : 0, mask_ss = batch > 1 ? mask_sample_stride : 0;
  if (mask_u8 && batch > 1 && mask_ss < (long long)(h - 1) * mask_pitch + w)
    return upk_fail(ctx, UPK_EINVAL, "region_mask: mask samples overlap (sample stride %lld)", mask_ss);
  if (mask_u8 && overlap(extent_of(mask_u8, mask_pitch, mask_ss, batch, h, w), extent_of(segm, segm_pitch, segm_ss, batch, h, w)))
    return upk_fail(ctx, UPK_EINVAL, "region_mask: the mask overlaps the label map");
  const long long words = ((long long)w + 63) / 64;
  const long long band_lds = (RG_BAND + 2LL * dilate + 2LL * RG_BAND) * words * 8;
  const long long count_lds = cells ? ((long long)h + h / factor) * words * 8 : 0;
  if (band_lds > RG_LDS_BYTES || count_lds > RG_LDS_BYTES)
    return upk_fail(ctx, UPK_ESHAPE, "region_mask: the bit rows of a %d x %d map (%lld and %lld bytes) do not fit %d bytes of LDS", h, w,
                    band_lds, count_lds, RG_LDS_BYTES);
  RegionArgs a;
  memset(&a, 0, sizeof(a));
  a.segm = segm, a.mask = mask_u8, a.keep = keep, a.cells = cells;
  a.segm_pitch = segm_pitch, a.segm_ss = segm_ss, a.mask_pitch = mask_pitch, a.mask_ss = mask_ss;
  a.h = h, a.w = w, a.r = dilate, a.f = factor, a.words = (int)words, a.bands = (h + RG_BAND - 1) / RG_BAND;
  a.vec = mask_u8 && !(((uintptr_t)mask_u8 | (uintptr_t)mask_pitch | (uintptr_t)mask_ss) & 3);
  a.vec16 = !(w & 15) && !(((uintptr_t)segm | (uintptr_t)segm_pitch | (uintptr_t)segm_ss) & 15);
  memcpy(a.sel, label_sel_host, sizeof(a.sel));
  const size_t lds = (size_t)(band_lds > count_lds ? band_lds : count_lds);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(region_mask_kernel, dim3((unsigned)(a.bands + (cells ? 1 : 0)), (unsigned)batch), dim3(RG_THREADS), lds,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "region_mask");
}

extern "C" int upk_composite_u8(upk_ctx* ctx, const uint8_t* orig, long long orig_pitch, long long orig_ss, const uint8_t* gen,
                                long long gen_pitch, long long gen_ss, const uint8_t* mask_u8, long long mask_pitch,
                                long long mask_ss, int batch, int h, int w, int feather, uint8_t* out, long long out_pitch,
                                long long out_ss, uint8_t* alpha_out, long long alpha_pitch, long long alpha_ss,
                                upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!orig || !gen || !mask_u8 || !out) return upk_fail(ctx, UPK_EINVAL, "composite: null original, generated picture, mask or output");
  if (batch <= 0 || h <= 0 || w <= 0) return upk_fail(ctx, UPK_EINVAL, "composite: sizes must be positive");
  if (feather < 0 || feather > RG_MAX_FEATHER)
    return upk_fail(ctx, UPK_EINVAL, "composite: feather %d, 0 .. %d are supported", feather, RG_MAX_FEATHER);
  if (orig_pitch < 3LL * w || gen_pitch < 3LL * w || out_pitch < 3LL * w)
    return upk_fail(ctx, UPK_EINVAL, "composite: a picture pitch (%lld, %lld, %lld) below 3 * w = %lld", orig_pitch, gen_pitch, out_pitch,
                    3LL * w);
  if (mask_pitch < (long long)w || (alpha_out && alpha_pitch < (long long)w))
    return upk_fail(ctx, UPK_EINVAL, "composite: a mask / alpha pitch (%lld, %lld) below w = %d", mask_pitch, alpha_pitch, w);
  if (batch > 65535) return upk_fail(ctx, UPK_ESHAPE, "composite: batch %d above 65535", batch);
  if (batch == 1) orig_ss = gen_ss = mask_ss = out_ss = alpha_ss = 0;
  if (batch > 1 && (out_ss < (long long)(h - 1) * out_pitch + 3LL * w || (alpha_out && alpha_ss < (long long)(h - 1) * alpha_pitch + w)))
    return upk_fail(ctx, UPK_EINVAL, "composite: output samples overlap (sample strides %lld, %lld)", out_ss, alpha_ss);
  const Extent e_out = extent_of(out, out_pitch, out_ss, batch, h, 3LL * w);
  const Extent e_in[3] = {extent_of(orig, orig_pitch, orig_ss, batch, h, 3LL * w), extent_of(gen, gen_pitch, gen_ss, batch, h, 3LL * w),
                          extent_of(mask_u8, mask_pitch, mask_ss, batch, h, w)};
  for (int i = 0; i < 3; ++i)
    if (overlap(e_out, e_in[i])) return upk_fail(ctx, UPK_EINVAL, "composite: out overlaps an input");
  if (alpha_out) {
    const Extent e_al = extent_of(alpha_out, alpha_pitch, alpha_ss, batch, h, w);
    for (int i = 0; i < 3; ++i)
      if (overlap(e_al, e_in[i])) return upk_fail(ctx, UPK_EINVAL, "composite: alpha_out overlaps an input");
    if (overlap(e_al, e_out)) return upk_fail(ctx, UPK_EINVAL, "composite: alpha_out overlaps out");
  }
  const long long words = ((long long)w + 63) / 64, w4 = ((long long)w + 3) / 4 * 4;
  const long long nst = RG_BAND + 2LL * feather;
  const long long lds = nst * words * 8 + nst * w4;
  if (lds > RG_LDS_BYTES)
    return upk_fail(ctx, UPK_ESHAPE, "composite: %lld staged rows of a %d-pixel row (%lld bytes) do not fit %d bytes of LDS", nst, w, lds,
                    RG_LDS_BYTES);
  CompArgs a;
  memset(&a, 0, sizeof(a));
  a.orig = orig, a.gen = gen, a.mask = mask_u8, a.out = out, a.alpha = alpha_out;
  a.orig_pitch = orig_pitch, a.orig_ss = orig_ss, a.gen_pitch = gen_pitch, a.gen_ss = gen_ss;
  a.mask_pitch = mask_pitch, a.mask_ss = mask_ss, a.out_pitch = out_pitch, a.out_ss = out_ss;
  a.alpha_pitch = alpha_pitch, a.alpha_ss = alpha_ss;
  a.h = h, a.w = w, a.fr = feather, a.words = (int)words, a.w4 = (int)w4;
  // dword accesses of 12 picture bytes / 4 alpha bytes: every group of 4 pixels stays aligned
  a.vec = !(((uintptr_t)orig | (uintptr_t)gen | (uintptr_t)out | (uintptr_t)alpha_out | (uintptr_t)orig_pitch | (uintptr_t)gen_pitch |
             (uintptr_t)out_pitch | (uintptr_t)(alpha_out ? alpha_pitch : 0) | (uintptr_t)orig_ss | (uintptr_t)gen_ss | (uintptr_t)out_ss |
             (uintptr_t)(alpha_out ? alpha_ss : 0)) & 3);
  a.vec16 = !(w & 15) && !(((uintptr_t)mask_u8 | (uintptr_t)mask_pitch | (uintptr_t)mask_ss) & 15);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((h + RG_BAND - 1) / RG_BAND), (unsigned)batch), dim3(RG_THREADS), (size_t)lds,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "composite");
}
