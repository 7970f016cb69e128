// upk_resize_bilinear_u8: uint8 HWC pictures -> the `lr` conditioning of the upscale model (app.py:93-97,
// deepfashion_inshop.py:427-431): T.Pad(edge), T.Resize(BILINEAR) on the PIL picture, T.ToTensor(), x * 2 - 1, in one launch.
//
// T.Resize on a PIL picture is Pillow's two-pass resampling in 22-bit fixed point: integer arithmetic, so the bytes are
// reproducible bit for bit.  The coefficient tables come from the host (upgpt_amd/prepare.py builds them in double);
// per pass   acc = 2^21 + sum_t pix[xmin + t] * k[t],   out = clip8(acc >> 22)   (acc < 2^31: sum k <= 2^22 + n).
// The horizontal pass runs first and is rounded to a byte; the vertical pass runs on those bytes.
//
// One workgroup = one band of output rows of one picture: it runs the horizontal pass for the (padded) input rows the
// band's taps cover into LDS as bytes, passes a barrier, and runs the vertical pass from LDS.  A skipped pass is the
// same code with the single tap (x, 2^22), which returns the byte itself.  The edge pad is index clamping on the read.
// The fp32 finishing t = fl(fl(u / 255) * 2 - 1) is specified operation by operation, hence (build.py FILE_FLAGS too):
#pragma clang fp contract(off)
//
// Launch-bound (8 pictures of 256 x 192 are 1.2 MB in, 0.3 MB of bytes out).  Fast path of the vertical pass: one thread
// = 4 adjacent output pixels, three LDS dwords per tap, 12 packed bytes as three dword stores / 16-byte fp32 stores;
// taken when out_w is a multiple of 4 and the destinations keep the vectors aligned.  Everything else goes per pixel.
// The source is always read bytewise: any pitch, any sample stride, any alignment.
#include "common.h"

namespace {

constexpr int RS_LDS_BYTES = 64 * 1024;  // staging budget: two workgroups per CU
constexpr int RS_BAND = 8;               // output rows per workgroup (fewer when the staged rows would not fit)
constexpr int RS_THREADS = 256;
constexpr int RS_BITS = 22;

struct ResizeArgs {
  const uint8_t* src;
  const int32_t *xb, *xk, *yb, *yk;
  uint8_t* dst;
  float *nchw, *nhwc;
  long src_pitch, src_ss, dst_pitch, dst_ss;
  int src_h, src_w, pad_x, pad_y, out_h, out_w, xks, yks, band, cap_rows, vec;
};

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
  const int v = (int)acc >> RS_BITS;
  return (uint32_t)min(max(v, 0), 255);
}

__device__ __forceinline__ float lr_value(uint32_t u) { return __fdiv_rn((float)u, 255.0f) * 2.0f - 1.0f; }

// (first tap, taps) of output row y; a skipped pass has the one tap y
__device__ __forceinline__ void row_taps(const ResizeArgs& a, int y, int& lo, int& n) {
  if (a.yb) {
    lo = a.yb[2 * y];
    n = max(min(a.yb[2 * y + 1], a.yks), 0);
  } else {
    lo = y;
    n = 1;
  }
}

// padded input rows [lo, hi) the output rows [y0, y1) read
__device__ __forceinline__ void band_span(const ResizeArgs& a, int y0, int y1, int& lo, int& hi) {
  lo = 0x7fffffff, hi = 0;
  for (int y = y0; y < y1; ++y) {
    int l, n;
    row_taps(a, y, l, n);
    lo = min(lo, l);
    hi = max(hi, l + n);
  }
  if (hi < lo) hi = lo;
}

__global__ __launch_bounds__(RS_THREADS) void resize_band_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  const int b = blockIdx.y;
  const int y0 = blockIdx.x * a.band;
  const int y1 = min(y0 + a.band, a.out_h);
  const int row_bytes = 3 * a.out_w;
  const uint8_t* s = a.src + (long)b * a.src_ss;
  int lo, hi;
  band_span(a, y0, y1, lo, hi);
  // the host sizes the band for tables of the resampling geometry; any other table is taken one output row at a time
  // (yks <= cap_rows is checked before the launch), so the staged rows never leave the LDS allocation
  const bool whole = (long)hi - lo <= a.cap_rows;
  for (int ya = y0; ya < y1;) {
    const int ye = whole ? y1 : ya + 1;
    if (!whole) band_span(a, ya, ye, lo, hi);
    const int nrows = hi - lo;
    // horizontal pass: padded input rows [lo, hi) -> bytes in LDS
    for (int i = threadIdx.x; i < nrows * a.out_w; i += RS_THREADS) {
      const int r = i / a.out_w, x = i - r * a.out_w;
      const int sy = min(max(lo + r - a.pad_y, 0), a.src_h - 1);
      const uint8_t* row = s + (long)sy * a.src_pitch;
      int xmin = x, n = 1;
      if (a.xb) {
        xmin = a.xb[2 * x];
        n = min(a.xb[2 * x + 1], a.xks);
      }
      const int32_t* k = a.xk + (long)x * a.xks;
      uint32_t c0 = 1u << (RS_BITS - 1), c1 = c0, c2 = c0;
      for (int t = 0; t < n; ++t) {
        const int sx = min(max(xmin + t - a.pad_x, 0), a.src_w - 1);
        const uint8_t* p = row + 3L * sx;
        const uint32_t kk = a.xb ? (uint32_t)k[t] : 1u << RS_BITS;
        c0 += p[0] * kk;
        c1 += p[1] * kk;
        c2 += p[2] * kk;
      }
      uint8_t* o = stage + r * row_bytes + 3 * x;
      o[0] = (uint8_t)clip8(c0);
      o[1] = (uint8_t)clip8(c1);
      o[2] = (uint8_t)clip8(c2);
    }
    __syncthreads();
    // vertical pass from LDS, and the three destinations
    if (a.vec) {
      const int wq = a.out_w >> 2;
      for (int i = threadIdx.x; i < (ye - ya) * wq; i += RS_THREADS) {
        const int r = i / wq, xq = i - r * wq;
        const int y = ya + r;
        int ymin, n;
        row_taps(a, y, ymin, n);
        const int32_t* k = a.yk + (long)y * a.yks;
        uint32_t acc[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] = 1u << (RS_BITS - 1);
        for (int t = 0; t < n; ++t) {
          const uint32_t* p = (const uint32_t*)(stage + (ymin + t - lo) * row_bytes + 12 * xq);
          const uint32_t kk = a.yb ? (uint32_t)k[t] : 1u << RS_BITS;
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const uint32_t v = p[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * q + j] += ((v >> (8 * j)) & 0xffu) * kk;
          }
        }
        uint32_t u[12];  // pixel-major, channel-minor
#pragma unroll
        for (int j = 0; j < 12; ++j) u[j] = clip8(acc[j]);
        if (a.dst) {
          uint32_t* o = (uint32_t*)(a.dst + b * a.dst_ss + (long)y * a.dst_pitch + 12L * xq);
#pragma unroll
          for (int q = 0; q < 3; ++q) o[q] = u[4 * q] | u[4 * q + 1] << 8 | u[4 * q + 2] << 16 | u[4 * q + 3] << 24;
        }
        if (a.nhwc) {
          f32x4* o = (f32x4*)(a.nhwc + (((long)b * a.out_h + y) * a.out_w + 4 * xq) * 3);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lr_value(u[4 * q + j]);
            o[q] = v;
          }
        }
        if (a.nchw) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lr_value(u[3 * j + c]);
            *(f32x4*)(a.nchw + (((long)b * 3 + c) * a.out_h + y) * a.out_w + 4 * xq) = v;
          }
        }
      }
    } else {
      for (int i = threadIdx.x; i < (ye - ya) * a.out_w; i += RS_THREADS) {
        const int r = i / a.out_w, x = i - r * a.out_w;
        const int y = ya + r;
        int ymin, n;
        row_taps(a, y, ymin, n);
        const int32_t* k = a.yk + (long)y * a.yks;
        uint32_t acc[3] = {1u << (RS_BITS - 1), 1u << (RS_BITS - 1), 1u << (RS_BITS - 1)};
        for (int t = 0; t < n; ++t) {
          const uint8_t* p = stage + (ymin + t - lo) * row_bytes + 3 * x;
          const uint32_t kk = a.yb ? (uint32_t)k[t] : 1u << RS_BITS;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += p[c] * kk;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t u = clip8(acc[c]);
          if (a.dst) a.dst[b * a.dst_ss + (long)y * a.dst_pitch + 3L * x + c] = (uint8_t)u;
          const float t = lr_value(u);
          if (a.nhwc) a.nhwc[(((long)b * a.out_h + y) * a.out_w + x) * 3 + c] = t;
          if (a.nchw) a.nchw[(((long)b * 3 + c) * a.out_h + y) * a.out_w + x] = t;
        }
      }
    }
    ya = ye;
    if (ya < y1) __syncthreads();  // (the next row's staging overwrites what this row's vertical pass reads)
  }
}

}  // namespace

extern "C" int upk_resize_bilinear_u8(upk_ctx* ctx, const uint8_t* src, int batch, int src_h, int src_w, long long src_pitch,
                                      long long src_sample_stride, int pad_x, int pad_y, int out_h, int out_w,
                                      const int32_t* xbounds, const int32_t* xk, int xksize, const int32_t* ybounds,
                                      const int32_t* yk, int yksize, uint8_t* dst_u8, long long dst_pitch,
                                      long long dst_sample_stride, float* dst_nchw, float* dst_nhwc, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!src) return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: null src");
  if (!dst_u8 && !dst_nchw && !dst_nhwc) return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: no destination");
  if (batch <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0)
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: sizes must be positive");
  if (pad_x < 0 || pad_y < 0) return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: negative pad (%d, %d)", pad_x, pad_y);
  const long in_w = (long)src_w + 2L * pad_x, in_h = (long)src_h + 2L * pad_y;
  if (in_w > 0x7fffffffL || in_h > 0x7fffffffL) return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: padded size overflows");
  const bool xpass = xbounds || xk, ypass = ybounds || yk;
  if ((in_w != out_w || xpass) && (!xbounds || !xk))
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: the horizontal pass %ld -> %d needs xbounds and xk", in_w, out_w);
  if ((in_h != out_h || ypass) && (!ybounds || !yk))
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: the vertical pass %ld -> %d needs ybounds and yk", in_h, out_h);
  if ((xpass && xksize < 1) || (ypass && yksize < 1))
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: ksize must be >= 1 (%d, %d)", xksize, yksize);
  if (((uintptr_t)xbounds | (uintptr_t)xk | (uintptr_t)ybounds | (uintptr_t)yk | (uintptr_t)dst_nchw | (uintptr_t)dst_nhwc) & 3)
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: tables and fp32 destinations must be 4-byte aligned");
  if (dst_u8 && dst_pitch < 3LL * out_w)
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: dst_pitch %lld below 3 * out_w = %lld", dst_pitch, 3LL * out_w);
  if (dst_u8 && batch > 1 && dst_sample_stride < (long long)(out_h - 1) * dst_pitch + 3LL * out_w)
    return upk_fail(ctx, UPK_EINVAL, "resize_bilinear: destination samples overlap (sample stride %lld)", dst_sample_stride);
  // band geometry: cap_rows staged rows of 3 * out_w bytes fit the budget; one output row needs yksize of them
  const long row_bytes = 3L * out_w;
  const long cap = RS_LDS_BYTES / row_bytes;
  const long need = ypass ? yksize : 1;
  if (cap < need)
    return upk_fail(ctx, UPK_ESHAPE, "resize_bilinear: %ld staged rows of %ld bytes do not fit %d bytes of LDS", need, row_bytes,
                    RS_LDS_BYTES);
  if (batch > 65535) return upk_fail(ctx, UPK_ESHAPE, "resize_bilinear: batch %d above 65535", batch);
  // rows a band of bh output rows reads: its first and last row are (bh - 1) * in / out apart, each reads <= yksize
  auto span = [&](long bh) { return ypass ? (((bh - 1) * in_h + out_h - 1) / out_h + yksize) : bh; };
  long bh = RS_BAND < out_h ? RS_BAND : out_h;
  while (bh > 1 && span(bh) > cap) --bh;
  long rows = span(bh);
  if (rows > cap) rows = cap;
  if (rows < need) rows = need;
  ResizeArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src, a.xb = xbounds, a.xk = xk, a.yb = ybounds, a.yk = yk, a.dst = dst_u8, a.nchw = dst_nchw, a.nhwc = dst_nhwc;
  a.src_pitch = src_pitch, a.src_ss = batch > 1 ? src_sample_stride : 0;
  a.dst_pitch = dst_pitch, a.dst_ss = batch > 1 ? dst_sample_stride : 0;
  a.src_h = src_h, a.src_w = src_w, a.pad_x = pad_x, a.pad_y = pad_y, a.out_h = out_h, a.out_w = out_w;
  a.xks = xksize, a.yks = yksize, a.band = (int)bh, a.cap_rows = (int)rows;
  // dword stores of 12 packed bytes, 16-byte stores of 4 floats: every group of 4 pixels stays aligned
  a.vec = !(out_w & 3) && !(dst_u8 && (((uintptr_t)dst_u8 | a.dst_ss | dst_pitch) & 3)) && !((uintptr_t)dst_nchw & 15) &&
          !((uintptr_t)dst_nhwc & 15);
  const size_t lds = (size_t)((rows * row_bytes + 15) / 16 * 16);
  const unsigned bands = (unsigned)((out_h + bh - 1) / bh);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(resize_band_kernel, dim3(bands, (unsigned)batch), dim3(RS_THREADS), lds, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "resize_bilinear");
}
