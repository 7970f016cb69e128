// FID's InceptionV3 (pytorch_fid 0.3.0, dims = 2048; the algorithm is stated in include/upk.h).  upk_conv2d_nhwc_f16 takes
// ksize 1 or 3 with "same" padding only; the network needs unpadded 3x3 (stride 1 and 2), 5x5, 1x7 / 7x1, 1x3 / 3x1 and 3x3
// pools.  Four entry points:
//   upk_conv2d_rect_f16     MFMA implicit-GEMM convolution, independent kh / kw / pad_h / pad_w, bias + ReLU epilogue, output
//                           row stride (a branch writes its channel slice of the block's concatenation)
//   upk_pool3_nhwc_f16      3x3 max / average (in-picture divisor) pooling, stride 1 pad 1 or stride 2 pad 0
//   upk_fid_input_f16       pictures (uint8 HWC windows or fp32 NCHW) -> bilinear resize -> 2 x - 1 -> fp16 NHWC, 32 channels
//   upk_avgpool_global_f32  fp16 NHWC [n, hw, C] -> fp32 [n, C] means
//
// The input values are specified operation by operation (include/upk.h): build.py's FILE_FLAGS gives this file
// -ffp-contract=off; it says so itself for whoever compiles it another way:
#pragma clang fp contract(off)
#include "common.h"

namespace {

// ---------------------------------------------------------------- convolution
// Output tile of a workgroup: 128 pixels x (16 NI) channels; wave v owns pixels 32 v .. 32 v + 31 (two 16-pixel MFMA
// columns) and all 16 NI channels.  D = W x X^T with v_mfma_f32_16x16x32_f16: operand A is the weight fragment (lane l:
// packed row n0 + 16 j + (l & 15), k = 8 (l >> 4) .. + 7, one 16-byte load from the [K / 32][n_pad][32] layout), operand B
// the activation fragment (lane l: pixel m0 + 16 i + (l & 15), the same eight channels, one 16-byte load from NHWC or
// zeros outside the picture), and lane l ends with channels n0 + 16 j + 4 (l >> 4) .. + 3 of that pixel: one 8-byte store.
// No LDS and no split-K: the four waves of a workgroup read the same weight lines (L1 / L2 hits), and an output element
// is ONE fp32 accumulation chain over k = (ky, kx, ci) in ascending order, whatever the batch and wherever the picture
// sits in it.
struct RectArgs {
  const f16* x;
  const f16* w;
  const float* bias;
  const f16* zeros;  // the context's zero page: what a tap outside the picture (or a pixel past M) loads, with step 0
  f16* y;
  int M;  // batch * ho * wo
  int h, w_in, ho, wo, cchunks, ldx, kh, kw, stride, ph, pw, n_out, n_pad, ldy, relu;
};

template <int NI>
__global__ __launch_bounds__(256) void conv_rect_kernel(const RectArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & 15, lg = lane >> 4;
  const int m0 = ((int)blockIdx.x * 4 + wave) * 32;
  const int n0 = (int)blockIdx.y * (16 * NI);
  if (m0 >= a.M) return;  // (wave-uniform; the kernel has no barrier)
  const int hw = a.ho * a.wo;
  bool live[2];
  int iy0[2], ix0[2];
  long pb[2];  // element offset of pixel (0, 0) of the lane's picture
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + 16 * i + lc;
    live[i] = m < a.M;
    const int mm = live[i] ? m : 0;
    const int b = mm / hw, p = mm - b * hw;
    const int oy = p / a.wo, ox = p - oy * a.wo;
    iy0[i] = oy * a.stride - a.ph;
    ix0[i] = ox * a.stride - a.pw;
    pb[i] = (long)b * a.h * a.w_in;
  }
  bool nlive[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) nlive[j] = n0 + 16 * j < a.n_pad;
  const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const long wrow = (long)(n0 + lc) * 32 + 8 * lg;     // the lane's place inside a K chunk of the packed weight
  const long wchunk = (long)a.n_pad * 32;
  for (int ky = 0; ky < a.kh; ++ky)
    for (int kx = 0; kx < a.kw; ++kx) {
      const f16* px[2];
      int step[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int iy = iy0[i] + ky, ix = ix0[i] + kx;
        const bool ok = live[i] && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w_in;
        px[i] = ok ? a.x + (pb[i] + (long)iy * a.w_in + ix) * a.ldx + 8 * lg : a.zeros + 8 * lg;
        step[i] = ok ? 32 : 0;
      }
      const f16* wt = a.w + (long)(ky * a.kw + kx) * a.cchunks * wchunk + wrow;
      for (int cc = 0; cc < a.cchunks; ++cc) {
        f16x8 fa[2], fb[NI];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *(const f16x8*)(px[i] + cc * step[i]);
#pragma unroll
        for (int j = 0; j < NI; ++j) fb[j] = nlive[j] ? *(const f16x8*)(wt + cc * wchunk + j * 512) : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
      }
    }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int n = n0 + 16 * j + 4 * lg;
    if (!nlive[j] || n >= a.n_out) continue;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *(const f32x4*)(a.bias + n);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (!live[i]) continue;
      const int m = m0 + 16 * i + lc;
      f16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r] + bv[r];
        if (a.relu) v = v > 0.0f ? v : 0.0f;
        o[r] = (f16)v;
      }
      f16* yp = a.y + (long)m * a.ldy + n;
      if (n + 3 < a.n_out) {
        *(f16x4*)yp = o;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.n_out) yp[r] = o[r];
      }
    }
  }
}

// ---------------------------------------------------------------- 3x3 pooling
struct PoolArgs {
  const f16* x;
  f16* y;
  long total;  // batch * ho * wo * (c / 8)
  int h, w, ho, wo, c8, ldx, ldy, stride, pad, avg;
};

// one thread per (output pixel, 8 channels): up to nine 16-byte loads, one 16-byte store.  Taps outside the picture take no
// part: the maximum ignores them, the average sums the in-picture taps in (ky, kx) order in fp32 and divides ONCE by their
// number.
__global__ __launch_bounds__(256) void pool3_kernel(const PoolArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int cg = (int)(idx % a.c8);
  long r = idx / a.c8;
  const int ox = (int)(r % a.wo);
  r /= a.wo;
  const int oy = (int)(r % a.ho);
  const long n = r / a.ho;
  float s[8];
  f16x8 m;
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.0f, m[j] = (f16)(-__builtin_huge_valf());
  int cnt = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
      if (iy < 0 || iy >= a.h || ix < 0 || ix >= a.w) continue;
      const f16x8 v = *(const f16x8*)(a.x + ((n * a.h + iy) * a.w + ix) * a.ldx + 8 * cg);
      ++cnt;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[j] += (float)v[j];
        m[j] = v[j] > m[j] ? v[j] : m[j];
      }
    }
  if (a.avg) {
    const float d = (float)cnt;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = (f16)__fdiv_rn(s[j], d);
  }
  *(f16x8*)(a.y + ((n * a.ho + oy) * a.wo + ox) * a.ldy + 8 * cg) = m;
}

// ---------------------------------------------------------------- input
struct FidInputArgs {
  const void* src;
  f16* y;
  long pitch, ss, ys, total;  // total = batch * oh * ow * 4 (four 16-byte pieces per output pixel)
  double sh, sw;              // h / oh, w / ow
  int h, w, oh, ow, f32, normalize;
};

__device__ __forceinline__ void fid_axis(int d, double scale, int n, int& i0, int& i1, float& lam) {
  double s = ((double)d + 0.5) * scale - 0.5;
  if (s < 0.0) s = 0.0;
  int i = (int)s;  // (s >= 0: truncation is the floor)
  if (i > n - 1) i = n - 1;
  i0 = i;
  i1 = i + 1 < n ? i + 1 : n - 1;
  lam = (float)(s - (double)i);
}

// one thread per 16-byte piece of an output pixel: piece 0 holds the three channels, pieces 1..3 are zero.  The source
// coordinate is formed in fp64 (so the interpolation weight is the exact one rounded once); the pixel arithmetic is fp32,
// one rounding per operation: v = u / 255; top = (1 - lx) v00 + lx v01, bottom likewise; (1 - ly) top + ly bottom; 2 x - 1.
__global__ __launch_bounds__(256) void fid_input_kernel(const FidInputArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int q = (int)(idx & 3);
  const long pix = idx >> 2;
  const int ox = (int)(pix % a.ow);
  const long r = pix / a.ow;
  const int oy = (int)(r % a.oh);
  const long n = r / a.oh;
  f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (q == 0) {
    int y0, y1, x0, x1;
    float ly, lx;
    fid_axis(oy, a.sh, a.h, y0, y1, ly);
    fid_axis(ox, a.sw, a.w, x0, x1, lx);
    const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
    float v[2][2][3];
#pragma unroll
    for (int iy = 0; iy < 2; ++iy)
#pragma unroll
      for (int ix = 0; ix < 2; ++ix) {
        if (a.f32) {
          const float* s = (const float*)a.src + n * a.ss + (long)ys[iy] * a.w + xs[ix];
          const long plane = (long)a.h * a.w;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[iy][ix][c] = s[c * plane];
        } else {
          const uint8_t* s = (const uint8_t*)a.src + n * a.ss + (long)ys[iy] * a.pitch + 3L * xs[ix];
#pragma unroll
          for (int c = 0; c < 3; ++c) v[iy][ix][c] = __fdiv_rn((float)s[c], 255.0f);
        }
      }
    const float my = __fsub_rn(1.0f, ly), mx = __fsub_rn(1.0f, lx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = __fadd_rn(__fmul_rn(mx, v[0][0][c]), __fmul_rn(lx, v[0][1][c]));
      const float bot = __fadd_rn(__fmul_rn(mx, v[1][0][c]), __fmul_rn(lx, v[1][1][c]));
      float t = __fadd_rn(__fmul_rn(my, top), __fmul_rn(ly, bot));
      if (a.normalize) t = __fsub_rn(__fmul_rn(2.0f, t), 1.0f);
      o[c] = (f16)t;
    }
  }
  *(f16x8*)(a.y + n * a.ys + ((long)oy * a.ow + ox) * 32 + 8 * q) = o;
}

// ---------------------------------------------------------------- global average
struct GapArgs {
  const f16* x;
  float* out;
  long total;  // n * (c / 8)
  int hw, c8, ld;
};

// one thread per (sample, 8 channels): the hw values of a channel are added in pixel order in fp32, one division
__global__ __launch_bounds__(256) void gap_kernel(const GapArgs a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.total) return;
  const int cg = (int)(idx % a.c8);
  const long n = idx / a.c8;
  const f16* p = a.x + n * a.hw * a.ld + 8 * cg;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.0f;
  for (int i = 0; i < a.hw; ++i) {
    const f16x8 v = *(const f16x8*)(p + (long)i * a.ld);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += (float)v[j];
  }
  const float d = (float)a.hw;
  float* o = a.out + (n * a.c8 + cg) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = __fdiv_rn(s[j], d);
}

}  // namespace

extern "C" int upk_conv2d_rect_f16(upk_ctx* ctx, const void* x, int ldx, int batch, int in_h, int in_w, int cin_pad, int kh,
                                   int kw, int stride, int pad_h, int pad_w, const void* w_packed, int n_out, int n_pad,
                                   const float* bias, int relu, void* y, int ldy, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !w_packed || !y) return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: null pointer");
  if (batch <= 0 || in_h <= 0 || in_w <= 0) return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: sizes must be positive");
  if (kh < 1 || kh > 7 || kw < 1 || kw > 7 || (stride != 1 && stride != 2) || pad_h < 0 || pad_h > 3 || pad_w < 0 || pad_w > 3)
    return upk_fail(ctx, UPK_ESHAPE, "conv2d_rect: kernel %d x %d, stride %d, padding (%d, %d): kh, kw must be 1 .. 7, stride 1 or 2, "
                    "paddings 0 .. 3", kh, kw, stride, pad_h, pad_w);
  if (cin_pad <= 0 || cin_pad % 32 || n_out <= 0 || n_pad % 16 || n_out > n_pad)
    return upk_fail(ctx, UPK_ESHAPE, "conv2d_rect: cin_pad = %d must be a positive multiple of 32, n_pad = %d a multiple of 16 and "
                    "0 < n_out = %d <= n_pad", cin_pad, n_pad, n_out);
  if (ldy < n_out) return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: ldy = %d below n_out = %d", ldy, n_out);
  if (ldx < cin_pad || ldx % 8 || ((uintptr_t)x & 15))
    return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: x needs 16-byte aligned rows of at least cin_pad elements (ldx = %d)", ldx);
  if (ldy % 4 || ((uintptr_t)y & 7)) return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: y needs 8-byte aligned rows (ldy = %d)", ldy);
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)bias & 15))
    return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: w_packed / bias must be 16-byte aligned");
  const int eh = in_h + 2 * pad_h - kh, ew = in_w + 2 * pad_w - kw;
  if (eh < 0 || ew < 0)
    return upk_fail(ctx, UPK_EINVAL, "conv2d_rect: a %d x %d map has no output under a %d x %d kernel with padding (%d, %d)", in_h,
                    in_w, kh, kw, pad_h, pad_w);
  const int ho = eh / stride + 1, wo = ew / stride + 1;
  const long M = (long)batch * ho * wo;
  if (M > 0x7fffffffL - 256 || (long)batch * in_h * in_w > 0x7fffffffL)
    return upk_fail(ctx, UPK_ESHAPE, "conv2d_rect: %ld output pixels", M);
  RectArgs a;
  a.x = (const f16*)x, a.w = (const f16*)w_packed, a.bias = bias, a.zeros = (const f16*)ctx->zero_page, a.y = (f16*)y;
  a.M = (int)M, a.h = in_h, a.w_in = in_w, a.ho = ho, a.wo = wo, a.cchunks = cin_pad / 32, a.ldx = ldx;
  a.kh = kh, a.kw = kw, a.stride = stride, a.ph = pad_h, a.pw = pad_w;
  a.n_out = n_out, a.n_pad = n_pad, a.ldy = ldy, a.relu = relu != 0;
  // the tile is a function of n_pad alone (never of the batch): 64 channels per workgroup, 32 for a narrow layer
  const int ni = n_pad >= 64 ? 4 : 2;
  const dim3 grid((unsigned)((M + 127) / 128), (unsigned)((n_pad + 16 * ni - 1) / (16 * ni)));
  hipStream_t stream = (hipStream_t)stream_;
  upk_prof_scope prof(ctx, UPK_CLS_IGEMM, stream);
  if (ni == 4)
    hipLaunchKernelGGL(conv_rect_kernel<4>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(conv_rect_kernel<2>, grid, dim3(256), 0, stream, a);
  return upk_check_launch(ctx, "conv2d_rect");
}

extern "C" int upk_pool3_nhwc_f16(upk_ctx* ctx, const void* x, int ldx, int batch, int h, int w, int c, int mode, int stride,
                                  void* y, int ldy, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !y) return upk_fail(ctx, UPK_EINVAL, "pool3: null pointer");
  if (batch <= 0 || h <= 0 || w <= 0 || c <= 0) return upk_fail(ctx, UPK_EINVAL, "pool3: sizes must be positive");
  if (mode != UPK_POOL_MAX && mode != UPK_POOL_AVG) return upk_fail(ctx, UPK_EINVAL, "pool3: mode = %d", mode);
  if (stride != 1 && stride != 2) return upk_fail(ctx, UPK_ESHAPE, "pool3: stride = %d, must be 1 (pad 1) or 2 (pad 0)", stride);
  if (c % 8) return upk_fail(ctx, UPK_ESHAPE, "pool3: c = %d is not a multiple of 8", c);
  if (stride == 2 && (h < 3 || w < 3)) return upk_fail(ctx, UPK_ESHAPE, "pool3: a %d x %d map has no unpadded 3x3 window", h, w);
  if (ldx < c || ldx % 8 || ((uintptr_t)x & 15) || ldy < c || ldy % 8 || ((uintptr_t)y & 15))
    return upk_fail(ctx, UPK_EINVAL, "pool3: x / y need 16-byte aligned rows of at least c elements (ldx = %d, ldy = %d)", ldx, ldy);
  PoolArgs a;
  a.x = (const f16*)x, a.y = (f16*)y, a.h = h, a.w = w, a.c8 = c / 8, a.ldx = ldx, a.ldy = ldy;
  a.stride = stride, a.pad = stride == 1 ? 1 : 0, a.avg = mode == UPK_POOL_AVG;
  a.ho = stride == 1 ? h : (h - 3) / 2 + 1, a.wo = stride == 1 ? w : (w - 3) / 2 + 1;
  a.total = (long)batch * a.ho * a.wo * a.c8;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "pool3: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(pool3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "pool3");
}

extern "C" int upk_fid_input_f16(upk_ctx* ctx, const void* src, int src_f32, long long pitch, long long sample_stride, int batch,
                                 int h, int w, int out_h, int out_w, int normalize, void* y, long long y_sample_stride,
                                 upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!src || !y) return upk_fail(ctx, UPK_EINVAL, "fid_input: null pointer");
  if (batch <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0)
    return upk_fail(ctx, UPK_EINVAL, "fid_input: sizes must be positive");
  if (((uintptr_t)y & 15) || (y_sample_stride & 7)) return upk_fail(ctx, UPK_EINVAL, "fid_input: y is not 16-byte aligned");
  if (batch > 1 && y_sample_stride < 32LL * out_h * out_w)
    return upk_fail(ctx, UPK_EINVAL, "fid_input: outputs overlap (y sample stride %lld elements)", y_sample_stride);
  if (src_f32) {
    if ((uintptr_t)src & 3) return upk_fail(ctx, UPK_EINVAL, "fid_input: fp32 src is not 4-byte aligned");
    if (batch > 1 && sample_stride < 3LL * h * w)
      return upk_fail(ctx, UPK_EINVAL, "fid_input: samples overlap (sample stride %lld floats)", sample_stride);
  } else {
    if (pitch < 3LL * w) return upk_fail(ctx, UPK_EINVAL, "fid_input: row pitch %lld below 3 * w = %lld bytes", pitch, 3LL * w);
    if (batch > 1 && sample_stride < (h - 1) * pitch + 3LL * w)
      return upk_fail(ctx, UPK_EINVAL, "fid_input: samples overlap (sample stride %lld)", sample_stride);
  }
  FidInputArgs a;
  a.src = src, a.y = (f16*)y, a.pitch = pitch, a.ss = batch > 1 ? sample_stride : 0;
  a.ys = batch > 1 ? y_sample_stride : 0;
  a.h = h, a.w = w, a.oh = out_h, a.ow = out_w, a.f32 = src_f32 != 0, a.normalize = normalize != 0;
  a.sh = (double)h / (double)out_h, a.sw = (double)w / (double)out_w;
  a.total = (long)batch * out_h * out_w * 4;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "fid_input: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(fid_input_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "fid_input");
}

extern "C" int upk_avgpool_global_f32(upk_ctx* ctx, const void* x, int ld, int n, int hw, int c, float* out, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  if (!x || !out) return upk_fail(ctx, UPK_EINVAL, "avgpool_global: null pointer");
  if (n <= 0 || hw <= 0 || c <= 0) return upk_fail(ctx, UPK_EINVAL, "avgpool_global: sizes must be positive");
  if (c % 8) return upk_fail(ctx, UPK_ESHAPE, "avgpool_global: c = %d is not a multiple of 8", c);
  if (ld < c || ld % 8 || ((uintptr_t)x & 15) || ((uintptr_t)out & 3))
    return upk_fail(ctx, UPK_EINVAL, "avgpool_global: x needs 16-byte aligned rows of at least c elements (ld = %d), out 4-byte "
                    "alignment", ld);
  GapArgs a;
  a.x = (const f16*)x, a.out = out, a.hw = hw, a.c8 = c / 8, a.ld = ld;
  a.total = (long)n * a.c8;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return upk_fail(ctx, UPK_ESHAPE, "avgpool_global: %ld workgroups", blocks);
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(gap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "avgpool_global");
}
