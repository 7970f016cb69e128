// upk_ssim_u8: per-level, per-channel means of the SSIM and contrast-structure maps of uint8 HWC picture pairs, what
// scripts/eval_metrics.py:110-111 gets from pytorch_msssim.ssim / ms_ssim (the algorithm is stated in include/upk.h).
//
// An HWC row of w pixels is a dense run of 3 w elements whose channel is (index % 3): the horizontal 11-tap pass is a
// 1-d filter with a tap distance of 3 ELEMENTS, so the three channels need no de-interleaving, every global and LDS
// access is dense, and a thread's channel is fixed by its column (tile widths are multiples of 3).
//
// ssim_level_kernel, one workgroup (192 threads) per (sample, 16 row x 96 element tile of the OUTPUT map):
//   stage    the tile plus its halo (26 rows x 126 elements) of both images into LDS as the integers they are
//   h-pass   thread (column j, row parity) -> the five moment planes G*x, G*y, G*xx, G*yy, G*xy of 13 rows into LDS
//   v-pass   thread (column j, row group of 8): 18 rows of the five planes slide through 8 x 5 register accumulators
//   maps     cs and ssim per output pixel, summed per thread, reduced per channel with wave shuffles, then over the
//            three waves in a fixed order into the workgroup's OWN slot of ws (no atomics)
// ssim_pool_kernel writes the next level's planes into ws, ssim_final_kernel sums the slots of every (sample, level)
// in a fixed order in fp64 and divides by the map size.
//
// Arithmetic.  A level-l plane is an exact integer sum P over 255 * 4^l (P <= 65280 at level 4: uint16).  sigma^2 =
// G*xx - (G*x)^2 is pure cancellation on flat pictures, and it is shift-invariant, so the tile works on x = (P - c) *
// scale with c the integer at the middle of the tile's input region (per image and channel): P - c is exact, flat
// regions give x = 0, and only mu needs c back (mu = G*x + c * scale; the weights sum to 1).
#include "common.h"

namespace {

constexpr int TH = 16;                   // output rows per tile
constexpr int TWE = 96;                  // output elements per tile row (32 pixels x 3 channels)
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int IN_ROWS = TH + HALO;       // 26
constexpr int IN_COLS = TWE + 3 * HALO;  // 126
constexpr int NT = 2 * TWE;              // 192 threads: (column, row parity) / (column, row group)
constexpr int RPT = TH / 2;              // output rows per thread
constexpr int MAX_LEVELS = 5;
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct LevelArgs {
  const void* a;
  const void* b;
  long a_pitch, a_ss, b_pitch, b_ss;  // in elements of the plane type
  float* part;                        // [batch][tiles][6]
  int h, w3, oh, ow3, tiles_x, tiles;
  float scale;  // 1 / (255 * 4^level)
  float g[TAPS];
};

template <typename T>
__global__ __launch_bounds__(NT) void ssim_level_kernel(const LevelArgs p) {
  __shared__ uint16_t s_in[2][IN_ROWS][IN_COLS];
  __shared__ float s_h[5][IN_ROWS][TWE];
  __shared__ float s_red[NT / 64][6];
  const int t = threadIdx.x;
  const long n = blockIdx.x / p.tiles;
  const int tile = blockIdx.x % p.tiles;
  const int y0 = (tile / p.tiles_x) * TH, x0 = (tile % p.tiles_x) * TWE;
  const T* pa = (const T*)p.a + n * p.a_ss + (long)y0 * p.a_pitch + x0;
  const T* pb = (const T*)p.b + n * p.b_ss + (long)y0 * p.b_pitch + x0;
  const int vr = min(IN_ROWS, p.h - y0), vc = min(IN_COLS, p.w3 - x0);  // (>= 11 rows, >= 33 elements)
  // (one element per thread and load, any pitch / alignment; dword loads unpacked into LDS would issue a quarter of the
  //  load instructions at level 0 where the row start allows it: not measured to matter at 0.6 ms per 100 pictures)
  for (int i = t; i < IN_ROWS * IN_COLS; i += NT) {
    const int r = i / IN_COLS, c = i % IN_COLS;
    const bool ok = r < vr && c < vc;
    s_in[0][r][c] = ok ? (uint16_t)pa[(long)r * p.a_pitch + c] : (uint16_t)0;
    s_in[1][r][c] = ok ? (uint16_t)pb[(long)r * p.b_pitch + c] : (uint16_t)0;
  }
  __syncthreads();

  const int j = t % TWE, rg = t / TWE, ch = j % 3;
  const int cr = vr / 2, cc = (vc / 2) / 3 * 3 + ch;
  const int ca = s_in[0][cr][cc], cb = s_in[1][cr][cc];
  // horizontal pass: rows rg, rg + 2, ...; taps 3 elements apart; g[k] == g[10 - k], so the pairs are added first
  for (int r = rg; r < IN_ROWS; r += 2) {
    float xa[TAPS], xb[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      xa[k] = (float)((int)s_in[0][r][j + 3 * k] - ca) * p.scale;
      xb[k] = (float)((int)s_in[1][r][j + 3 * k] - cb) * p.scale;
    }
    float m[5] = {p.g[5] * xa[5], p.g[5] * xb[5], p.g[5] * (xa[5] * xa[5]), p.g[5] * (xb[5] * xb[5]), p.g[5] * (xa[5] * xb[5])};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float a0 = xa[k], a1 = xa[HALO - k], b0 = xb[k], b1 = xb[HALO - k], gk = p.g[k];
      m[0] += gk * (a0 + a1);
      m[1] += gk * (b0 + b1);
      m[2] += gk * (a0 * a0 + a1 * a1);
      m[3] += gk * (b0 * b0 + b1 * b1);
      m[4] += gk * (a0 * b0 + a1 * b1);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) s_h[q][r][j] = m[q];
  }
  __syncthreads();

  // vertical pass: output rows rg * 8 + i, input rows rg * 8 + [0, 18)
  float acc[5][RPT];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int i = 0; i < RPT; ++i) acc[q][i] = 0.0f;
#pragma unroll
  for (int rr = 0; rr < RPT + HALO; ++rr) {
    float v[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = s_h[q][rg * RPT + rr][j];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int k = rr - i;
      if (k >= 0 && k < TAPS) {
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q][i] += p.g[k] * v[q];
      }
    }
  }
  const float sa = (float)ca * p.scale, sb = (float)cb * p.scale;
  float ssim = 0.0f, cs = 0.0f;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    if (y0 + rg * RPT + i < p.oh && x0 + j < p.ow3) {
      const float u1 = acc[0][i], u2 = acc[1][i];
      const float s11 = acc[2][i] - u1 * u1, s22 = acc[3][i] - u2 * u2, s12 = acc[4][i] - u1 * u2;
      const float m1 = u1 + sa, m2 = u2 + sb;
      const float c = (2.0f * s12 + C2) / (s11 + s22 + C2);
      const float l = (2.0f * (m1 * m2) + C1) / (m1 * m1 + m2 * m2 + C1);
      cs += c;
      ssim += l * c;
    }
  }
  float v[6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[2 * c] = ch == c ? ssim : 0.0f;
    v[2 * c + 1] = ch == c ? cs : 0.0f;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] += __shfl_xor(v[q], off, 64);
  if ((t & 63) == 0)
#pragma unroll
    for (int q = 0; q < 6; ++q) s_red[t >> 6][q] = v[q];
  __syncthreads();
  if (t < 6) p.part[(n * p.tiles + tile) * 6 + t] = (s_red[0][t] + s_red[1][t]) + s_red[2][t];
}

struct PoolArgs {
  const void* a;
  const void* b;
  long a_pitch, a_ss, b_pitch, b_ss;
  uint16_t* dst;  // [batch][2][h2][3 w2]
  long total;
  int h2, w2e, ph, pw;
};

// avg_pool2d(2, 2, padding = size % 2, count_include_pad=True) without its division: output i sums inputs 2 i - pad and
// 2 i - pad + 1, index -1 reads zero
template <typename T>
__global__ __launch_bounds__(256) void ssim_pool_kernel(const PoolArgs p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.total) return;
  const int e = (int)(idx % p.w2e);
  long r = idx / p.w2e;
  const int y = (int)(r % p.h2);
  r /= p.h2;
  const int img = (int)(r & 1);
  const long n = r >> 1;
  const int x = e / 3, ch = e - 3 * x;
  const T* s = img ? (const T*)p.b + n * p.b_ss : (const T*)p.a + n * p.a_ss;
  const long pitch = img ? p.b_pitch : p.a_pitch;
  uint32_t sum = 0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int iy = 2 * y - p.ph + dy;
    if (iy < 0) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int ix = 2 * x - p.pw + dx;
      if (ix < 0) continue;
      sum += s[(long)iy * pitch + 3 * ix + ch];
    }
  }
  p.dst[idx] = (uint16_t)sum;
}

struct FinalArgs {
  const float* part[MAX_LEVELS];
  int tiles[MAX_LEVELS];
  double inv_n[MAX_LEVELS];  // 1 / (map rows * map columns)
  float* out;                // [batch][levels][3][2]
  int levels;
};

// one wave per (sample, level): lane i sums slots i, i + 64, ... in fp64, then a shuffle tree; always the same order
__global__ __launch_bounds__(64) void ssim_final_kernel(const FinalArgs p) {
  const long n = blockIdx.x / p.levels;
  const int l = blockIdx.x % p.levels;
  const int tiles = p.tiles[l];
  const float* part = p.part[l] + n * tiles * 6;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < tiles; i += 64)
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] += (double)part[(long)i * 6 + q];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] += __shfl_xor(s[q], off, 64);
  if (threadIdx.x < 6) {
    double v = s[0];
#pragma unroll
    for (int q = 1; q < 6; ++q) v = threadIdx.x == q ? s[q] : v;
    p.out[(n * p.levels + l) * 6 + threadIdx.x] = (float)(v * p.inv_n[l]);
  }
}

struct Layout {
  int h[MAX_LEVELS], w[MAX_LEVELS], tiles_x[MAX_LEVELS], tiles[MAX_LEVELS];
  size_t part_off[MAX_LEVELS], plane_off[MAX_LEVELS];  // (plane_off[0] unused: level 0 is the caller's pictures)
  size_t total;
};

// 0: fine; UPK_EINVAL / UPK_ESHAPE otherwise
int make_layout(int batch, int h, int w, int levels, Layout* L) {
  if (batch <= 0 || h <= 0 || w <= 0 || levels < 1 || levels > MAX_LEVELS) return UPK_EINVAL;
  if (h > (1 << 24) || w > (1 << 24)) return UPK_ESHAPE;
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    L->h[l] = h, L->w[l] = w;
    if (h < TAPS || w < TAPS) return UPK_ESHAPE;
    L->tiles_x[l] = (3 * (w - HALO) + TWE - 1) / TWE;
    const long tiles = (long)L->tiles_x[l] * ((h - HALO + TH - 1) / TH);
    if (tiles * batch > 0x7fffffffL) return UPK_ESHAPE;
    L->tiles[l] = (int)tiles;
    L->part_off[l] = off;
    off += ((size_t)batch * tiles * 6 * sizeof(float) + 15) / 16 * 16;
    h = (h + 1) / 2, w = (w + 1) / 2;
  }
  for (int l = 1; l < levels; ++l) {
    L->plane_off[l] = off;
    off += ((size_t)batch * 2 * L->h[l] * 3 * L->w[l] * sizeof(uint16_t) + 15) / 16 * 16;
  }
  L->total = off;
  return UPK_OK;
}

}  // namespace

extern "C" size_t upk_ssim_ws_bytes(int batch, int h, int w, int levels) {
  Layout L;
  return make_layout(batch, h, w, levels, &L) == UPK_OK ? L.total : 0;
}

extern "C" int upk_ssim_u8(upk_ctx* ctx, const uint8_t* a, long long a_pitch, long long a_sample_stride, const uint8_t* b,
                           long long b_pitch, long long b_sample_stride, int batch, int h, int w, int levels, float* out,
                           void* ws, size_t ws_bytes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!a || !b || !out || !ws) return upk_fail(ctx, UPK_EINVAL, "ssim: null pointer");
  if (batch <= 0 || h <= 0 || w <= 0) return upk_fail(ctx, UPK_EINVAL, "ssim: sizes must be positive");
  if (levels < 1 || levels > MAX_LEVELS) return upk_fail(ctx, UPK_EINVAL, "ssim: levels = %d, must be 1 .. %d", levels, MAX_LEVELS);
  if (a_pitch < 3LL * w || b_pitch < 3LL * w)
    return upk_fail(ctx, UPK_EINVAL, "ssim: row pitch (%lld, %lld) below 3 * w = %lld bytes", a_pitch, b_pitch, 3LL * w);
  if (batch > 1 && (a_sample_stride < (h - 1) * a_pitch + 3LL * w || b_sample_stride < (h - 1) * b_pitch + 3LL * w))
    return upk_fail(ctx, UPK_EINVAL, "ssim: samples overlap (sample strides %lld, %lld)", a_sample_stride, b_sample_stride);
  if ((uintptr_t)out & 3) return upk_fail(ctx, UPK_EINVAL, "ssim: out is not 4-byte aligned");
  if ((uintptr_t)ws & 15) return upk_fail(ctx, UPK_EINVAL, "ssim: ws is not 16-byte aligned");
  Layout L;
  const int rc = make_layout(batch, h, w, levels, &L);
  if (rc != UPK_OK)
    return upk_fail(ctx, rc, "ssim: %d level(s) of a %d x %d picture: every level needs both sides in [%d, 2^24]", levels, h, w, TAPS);
  if (ws_bytes < L.total) return upk_fail(ctx, UPK_EWORKSPACE, "ssim: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  for (int l = 1; l < levels; ++l)
    if (((long)batch * 2 * L.h[l] * 3 * L.w[l] + 255) / 256 > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "ssim: level %d too large", l);

  float g[TAPS];
  {  // exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 (in double, rounded once)
    double e[TAPS], sum = 0.0;
    for (int i = 0; i < TAPS; ++i) sum += e[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < TAPS; ++i) g[i] = (float)(e[i] / sum);
  }
  hipStream_t stream = (hipStream_t)stream_;
  char* wsb = (char*)ws;
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, stream);
  FinalArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.out = out, fa.levels = levels;
  // the planes of the level at hand: the caller's pictures (bytes), then dense uint16 planes in ws
  const void *pa = a, *pb = b;
  long pa_pitch = a_pitch, pa_ss = batch > 1 ? a_sample_stride : 0, pb_pitch = b_pitch, pb_ss = batch > 1 ? b_sample_stride : 0;
  double denom = 255.0;
  for (int l = 0; l < levels; ++l) {
    LevelArgs la;
    la.a = pa, la.b = pb, la.a_pitch = pa_pitch, la.a_ss = pa_ss, la.b_pitch = pb_pitch, la.b_ss = pb_ss;
    la.part = (float*)(wsb + L.part_off[l]);
    la.h = L.h[l], la.w3 = 3 * L.w[l], la.oh = L.h[l] - HALO, la.ow3 = 3 * (L.w[l] - HALO);
    la.tiles_x = L.tiles_x[l], la.tiles = L.tiles[l];
    la.scale = (float)(1.0 / denom);
    memcpy(la.g, g, sizeof(g));
    const dim3 grid((unsigned)((long)batch * L.tiles[l]));
    if (l == 0) {
      hipLaunchKernelGGL(ssim_level_kernel<uint8_t>, grid, dim3(NT), 0, stream, la);
    } else {
      hipLaunchKernelGGL(ssim_level_kernel<uint16_t>, grid, dim3(NT), 0, stream, la);
    }
    int e = upk_check_launch(ctx, "ssim_level");
    if (e != UPK_OK) return e;
    fa.part[l] = la.part, fa.tiles[l] = L.tiles[l];
    fa.inv_n[l] = 1.0 / ((double)(L.h[l] - HALO) * (double)(L.w[l] - HALO));
    if (l + 1 == levels) break;
    PoolArgs po;
    po.a = pa, po.b = pb, po.a_pitch = pa_pitch, po.a_ss = pa_ss, po.b_pitch = pb_pitch, po.b_ss = pb_ss;
    po.dst = (uint16_t*)(wsb + L.plane_off[l + 1]);
    po.h2 = L.h[l + 1], po.w2e = 3 * L.w[l + 1], po.ph = L.h[l] & 1, po.pw = L.w[l] & 1;
    po.total = (long)batch * 2 * po.h2 * po.w2e;
    const dim3 pgrid((unsigned)((po.total + 255) / 256));
    if (l == 0) {
      hipLaunchKernelGGL(ssim_pool_kernel<uint8_t>, pgrid, dim3(256), 0, stream, po);
    } else {
      hipLaunchKernelGGL(ssim_pool_kernel<uint16_t>, pgrid, dim3(256), 0, stream, po);
    }
    e = upk_check_launch(ctx, "ssim_pool");
    if (e != UPK_OK) return e;
    const long plane = (long)po.h2 * po.w2e;
    pa = po.dst, pb = po.dst + plane;
    pa_pitch = pb_pitch = po.w2e, pa_ss = pb_ss = 2 * plane;
    denom *= 4.0;
  }
  hipLaunchKernelGGL(ssim_final_kernel, dim3((unsigned)((long)batch * levels)), dim3(64), 0, stream, fa);
  return upk_check_launch(ctx, "ssim_final");
}
