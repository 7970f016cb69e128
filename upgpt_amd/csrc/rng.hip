// Keyed (counter-based) device noise: upk_randn_keyed_f32 fills a [rows, batch, n] table of scaled standard normals,
// upk_philox_u32 the raw Philox words of the same elements.  Generator, counter layout, transform and error codes are
// stated in include/upk.h.  This file is compiled with -ffp-contract=off: the transform below is one fp32 operation
// at a time around logf / sqrtf / sincospif (philox.h: the generator and the transform, shared with loss.hip).
//
// fill_kernel<NORMAL>  a workgroup (256 threads) takes TILE = 1024 consecutive elements of one (row, sample) segment per
//                      turn and walks the tiles of the whole table grid-stride, so a value is a function of (key, element,
//                      row, stream, draw) alone: nothing of the launch enters it.  Thread t makes the Philox call of quad
//                      e0 / 4 + t and leaves its four values in LDS at s + 4 t .. s + 4 t + 3, s = the position of the tile's
//                      first element inside its 16-byte group of `out` (a segment starts at out + seg * n, 16-byte aligned
//                      only by luck when n % 4 != 0 or out is offset).  After the barrier thread g stores LDS group
//                      [4 g, 4 g + 4) with one 16-byte store when all four positions belong to the tile and element by
//                      element otherwise (the head in front of s, the tail behind s + cnt); 257 groups cover s + 1024.
//                      VALU (10 Philox rounds, two log / sqrt / sincospi per quad) and stores only; no global load but the
//                      wave-uniform key and scale.
#include "common.h"
#include "philox.h"

namespace {

constexpr int NT = 256;
constexpr int TILE = NT * 4;
constexpr long MAX_N = 1L << 34;       // q = e >> 2 is a 32-bit counter word
constexpr unsigned MAX_WG = 1u << 16;  // workgroups of a launch (the tiles beyond go grid-stride)

struct RArgs {
  const uint32_t* keys;  // [batch, 2]
  const float* scale;    // indexed by absolute row, or nullptr
  uint32_t* out;
  long n, tiles_per_seg, total_tiles;
  int batch, row0;
  uint32_t stream, draw;
};

template <bool NORMAL>
__global__ __launch_bounds__(NT) void fill_kernel(const RArgs p) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[TILE + 4];
  const int tid = threadIdx.x;
  for (long w = blockIdx.x; w < p.total_tiles; w += gridDim.x) {
    const long seg = w / p.tiles_per_seg;  // (row - row0) * batch + sample
    const long e0 = (w - seg * p.tiles_per_seg) * TILE;
    const long rr = seg / p.batch;
    const int b = (int)(seg - rr * p.batch);
    const uint32_t row = (uint32_t)p.row0 + (uint32_t)rr;
    const int cnt = (int)(p.n - e0 < TILE ? p.n - e0 : TILE);
    uint32_t* dst = p.out + seg * p.n + e0;
    const int s = (int)(((uintptr_t)dst >> 2) & 3);
    if (4 * tid < cnt) {
      uint32_t v[4];
      philox4x32_10((uint32_t)(e0 >> 2) + tid, row, p.stream, p.draw, p.keys[2 * b], p.keys[2 * b + 1], v);
      if (NORMAL) {
        const float sc = p.scale ? p.scale[row] : 1.0f;
        float z[4];
        box_muller(v[0], v[1], z[0], z[1]);
        box_muller(v[2], v[3], z[2], z[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sc == 0.0f ? 0u : __float_as_uint(z[j] * sc);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) s_v[s + 4 * tid + j] = v[j];
    }
    __syncthreads();
    for (int g = tid; g <= NT; g += NT) {
      const int lo = 4 * g;
      if (lo >= s && lo + 4 <= s + cnt) {
        *(uint4*)(dst - s + lo) = *(const uint4*)&s_v[lo];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (lo + j >= s && lo + j < s + cnt) dst[lo + j - s] = s_v[lo + j];
      }
    }
    __syncthreads();  // (the next turn overwrites s_v)
  }
}

int launch(upk_ctx* ctx, const char* what, bool normal, const uint32_t* keys, int batch, long long n, int row0, int rows,
           uint32_t stream_id, uint32_t draw, const float* row_scale, void* out, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!keys || !out) return upk_fail(ctx, UPK_EINVAL, "%s: null pointer", what);
  if (batch <= 0 || n <= 0 || rows <= 0) return upk_fail(ctx, UPK_EINVAL, "%s: batch, n and rows must be positive", what);
  if (row0 < 0 || row0 > 0x7fffffff - rows) return upk_fail(ctx, UPK_EINVAL, "%s: rows [%d, %d + %d) out of range", what, row0, row0, rows);
  if (n > MAX_N) return upk_fail(ctx, UPK_EINVAL, "%s: n = %lld above 2^34", what, n);
  if (((uintptr_t)keys | (uintptr_t)out | (uintptr_t)row_scale) & 3)
    return upk_fail(ctx, UPK_EINVAL, "%s: a pointer is not 4-byte aligned", what);
  RArgs a;
  a.keys = keys, a.scale = row_scale, a.out = (uint32_t*)out, a.n = (long)n, a.batch = batch, a.row0 = row0;
  a.stream = stream_id, a.draw = draw;
  a.tiles_per_seg = ((long)n + TILE - 1) / TILE;
  const long segs = (long)batch * rows;
  if (segs > (1L << 62) / a.tiles_per_seg || segs > (1L << 62) / (long)n)
    return upk_fail(ctx, UPK_ESHAPE, "%s: a table of %d x %d x %lld elements", what, rows, batch, n);
  a.total_tiles = segs * a.tiles_per_seg;
  const unsigned grid = (unsigned)(a.total_tiles < (long)MAX_WG ? a.total_tiles : (long)MAX_WG);
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  if (normal)
    hipLaunchKernelGGL(fill_kernel<true>, dim3(grid), dim3(NT), 0, stream, a);
  else
    hipLaunchKernelGGL(fill_kernel<false>, dim3(grid), dim3(NT), 0, stream, a);
  return upk_check_launch(ctx, what);
}

}  // namespace

extern "C" int upk_randn_keyed_f32(upk_ctx* ctx, const uint32_t* keys, int batch, long long n, int row0, int rows,
                                   uint32_t stream_id, uint32_t draw, const float* row_scale, float* out,
                                   upk_stream stream) {
  return launch(ctx, "randn_keyed", true, keys, batch, n, row0, rows, stream_id, draw, row_scale, out, stream);
}

extern "C" int upk_philox_u32(upk_ctx* ctx, const uint32_t* keys, int batch, long long n, int row0, int rows,
                              uint32_t stream_id, uint32_t draw, uint32_t* out, upk_stream stream) {
  return launch(ctx, "philox_u32", false, keys, batch, n, row0, rows, stream_id, draw, nullptr, out, stream);
}
