// upk_segm_boxes_u8 + upk_style_crops_u8: a picture and its human-parsing label map -> the per-garment style crops
// batch['styles'] is made of (the reference's Segmenter.forward, segm_utils.py:42-150, and the consumer's clip_transform,
// deepfashion_inshop.py:128-133), in two launches with no device-to-host copy between them.
//
// Launch 1, one workgroup per (group, sample): scans the label map for the group's labels and leaves an int32 record
// (left, right, top, bottom, N, S_r, S_g, S_b).  Integer minima / maxima / sums only: no reduction order to depend on.
//
// Launch 2, one workgroup per (band of 8 output rows, slot, sample): reads its group's record FROM DEVICE MEMORY, derives
// cut, zero pad, T.Resize(224) size and T.CenterCrop(224) offsets, builds Pillow's triangle-filter coefficients of the
// 8 rows and 224 columns it produces in double (operation for operation prepare.resample_coeffs, hence no contraction:)
#pragma clang fp contract(off)
// and runs resize.hip's two 22-bit integer passes over the VIRTUAL source: zero outside the cut, `mask ? byte : 0` (or the
// byte itself, or `mask ? byte : fill` for the background group) inside it.  The horizontal pass of the band's input rows
// goes to LDS as bytes, then a barrier, then the vertical pass from LDS.  Only the central 224 of the long axis is made.
//
// Staging bound.  After the pad a cut is square to within one row, the background is the picture itself: every axis has
// scale = in / out <= max(H, W) / 224 <= 6 for the sides accepted here (ST_MAX_SIDE).  Output index xx reads
// [int(c - s + .5), int(c + s + .5)) with c = (xx + .5) scale, s = max(scale, 1): at most 2 s + 2 <= 14 taps (ST_TAPS = 16),
// and a band of 8 rows spans at most 7 scale + 2 s + 2 <= 56 input rows (ST_CAP = 64 staged rows of 672 bytes).
#include "common.h"

namespace {

constexpr int ST_OUT = 224;        // T.Resize(224), T.CenterCrop(224)
constexpr int ST_BAND = 8;         // output rows per workgroup (224 = 28 bands)
constexpr int ST_THREADS = 256;
constexpr int ST_CAP = 64;         // staged rows
constexpr int ST_TAPS = 16;        // taps per output index
constexpr int ST_REC = 2 + ST_TAPS;  // (first tap, taps, k[ST_TAPS])
constexpr int ST_ROW_BYTES = 3 * ST_OUT;
constexpr int ST_MAX_SIDE = 6 * ST_OUT;  // 1344
constexpr int ST_BITS = 22;
constexpr int BX_THREADS = 512;

struct BoxArgs {
  const uint8_t *segm, *pic;
  int32_t* boxes;
  long segm_pitch, segm_ss, pic_pitch, pic_ss;
  int h, w, n_groups;
  uint32_t label[256];
};

__global__ __launch_bounds__(BX_THREADS) void segm_boxes_kernel(const BoxArgs a) {
  __shared__ uint8_t in_group[256];
  __shared__ int red[8];
  const int g = blockIdx.x, b = blockIdx.y;
  const uint32_t* label = a.label;
  if (threadIdx.x < 256) in_group[threadIdx.x] = (uint8_t)((label[threadIdx.x] >> g) & 1u);
  if (threadIdx.x < 8) red[threadIdx.x] = (threadIdx.x == 0 || threadIdx.x == 2) ? 0x7fffffff : (threadIdx.x < 4 ? -1 : 0);
  __syncthreads();
  const uint8_t* sg = a.segm + (long)b * a.segm_ss;
  const uint8_t* pic = a.pic + (long)b * a.pic_ss;
  int left = 0x7fffffff, right = -1, top = 0x7fffffff, bottom = -1;
  uint32_t n = 0, s0 = 0, s1 = 0, s2 = 0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int y = wave; y < a.h; y += BX_THREADS / 64) {
    const uint8_t* srow = sg + (long)y * a.segm_pitch;
    const uint8_t* prow = pic + (long)y * a.pic_pitch;
    for (int x = lane; x < a.w; x += 64) {
      if (!in_group[srow[x]]) continue;
      left = min(left, x), right = max(right, x), top = min(top, y), bottom = max(bottom, y);
      const uint8_t* p = prow + 3L * x;
      ++n, s0 += p[0], s1 += p[1], s2 += p[2];
    }
  }
  if (n) {  // (integer atomics in LDS: the result does not depend on their order)
    atomicMin(&red[0], left), atomicMax(&red[1], right), atomicMin(&red[2], top), atomicMax(&red[3], bottom);
    atomicAdd(&red[4], (int)n), atomicAdd(&red[5], (int)s0), atomicAdd(&red[6], (int)s1), atomicAdd(&red[7], (int)s2);
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    int v = red[threadIdx.x];
    if (red[4] == 0) v = threadIdx.x == 1 ? a.w : threadIdx.x == 3 ? a.h : 0;  // no masked pixel: 0, W, 0, H
    a.boxes[((long)b * a.n_groups + g) * 8 + threadIdx.x] = v;
  }
}

struct StyleArgs {
  const uint8_t *pic, *segm;
  const int32_t* boxes;
  uint8_t* dst;
  float* f32;
  int32_t *valid, *coeff;
  long pic_pitch, pic_ss, segm_pitch, segm_ss;
  int h, w, n_groups, n_slots;
  float mean[3], std[3];
  uint32_t label[256];
  int32_t gflags[32];  // UPK_STYLE_FILL | UPK_STYLE_MASK | max_rows << 8
  int32_t slot[32];    // group of the slot, -1: empty
};

// int(round((n - 224) / 2.0)), Python's round-half-to-even (T.CenterCrop)
__device__ __forceinline__ int center_off(int n) {
  const int d = n - ST_OUT, k = d >> 1;
  return (d & 1) ? k + (k & 1) : k;
}

// prepare.resample_coeffs for ONE output index, every step in double in its order; in == out is the skipped pass, the
// single tap (xx, 2^22) that returns the byte itself
__device__ void make_coeff(int in, int out, int xx, int32_t* rec) {
  for (int t = 0; t < ST_REC; ++t) rec[t] = 0;
  if (in == out) {
    rec[0] = xx, rec[1] = 1, rec[2] = 1 << ST_BITS;
    return;
  }
  const double scale = (double)in / (double)out;
  const double fs = scale > 1.0 ? scale : 1.0;
  const double support = fs;
  const double center = ((double)xx + 0.5) * scale;
  const int xmin = max((int)(center - support + 0.5), 0);
  const int xmax = min((int)(center + support + 0.5), in);
  const int n = min(max(xmax - xmin, 0), ST_TAPS);
  auto weight = [&](int x) {
    const double v = 1.0 - fabs(((double)(x + xmin) - center + 0.5) / fs);
    return v > 0.0 ? v : 0.0;
  };
  double total = 0.0;
  for (int x = 0; x < n; ++x) total += weight(x);
  rec[0] = xmin, rec[1] = n;
  for (int x = 0; x < n; ++x) {
    double w = weight(x);
    if (total != 0.0) w = w / total;
    rec[2 + x] = (int)(w * (double)(1 << ST_BITS) + 0.5);
  }
}

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
  const int v = (int)acc >> ST_BITS;
  return (uint32_t)min(max(v, 0), 255);
}

__global__ __launch_bounds__(ST_THREADS) void style_crops_kernel(const StyleArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[ST_CAP * ST_ROW_BYTES];
  __shared__ int32_t xrec[ST_OUT * ST_REC];
  __shared__ int32_t yrec[ST_BAND * ST_REC];
  __shared__ uint8_t in_group[256];
  const int band = blockIdx.x, slot = blockIdx.y, b = blockIdx.z;
  const int y0 = band * ST_BAND;
  const int g = a.slot[slot];
  const long crop = (long)b * a.n_slots + slot;

  // geometry from the device record: uniform over the workgroup
  int valid = 0, x_org = 0, y_org = 0, cw = 0, ch = 0, pad_x = 0, pad_y = 0, fill_mode = 0, mask_content = 0;
  uint32_t fill[3] = {0, 0, 0};
  if (g >= 0) {
    const int32_t* rec = a.boxes + ((long)b * a.n_groups + g) * 8;
    const int flags = a.gflags[g];
    fill_mode = flags & UPK_STYLE_FILL, mask_content = flags & UPK_STYLE_MASK;
    const int max_rows = flags >> 8;
    if (fill_mode) {  // the background group: the whole picture, no cut, no pad
      const int n = rec[4];
      cw = a.w, ch = a.h;
      valid = n > 0;
      if (valid) fill[0] = (uint32_t)(rec[5] / n), fill[1] = (uint32_t)(rec[6] / n), fill[2] = (uint32_t)(rec[7] / n);
    } else {
      x_org = rec[0], y_org = rec[2];
      cw = rec[1] - rec[0], ch = rec[3] - rec[2];  // (the index of the last masked column / row as an exclusive end)
      valid = cw > 0 && ch > 0 && !(max_rows > 0 && ch > max_rows) && x_org >= 0 && y_org >= 0 && rec[1] <= a.w && rec[3] <= a.h;
      const int d = ch - cw, p = d >> 1;  // floor division
      if (p > 0) pad_x = p;
      if (p < 0) pad_y = -p;
    }
  }
  const int pw = cw + 2 * pad_x, ph = ch + 2 * pad_y;
  int ow = ST_OUT, oh = ST_OUT;
  if (valid) {
    if (pw <= ph) oh = (int)((long)ST_OUT * ph / pw);
    else ow = (int)((long)ST_OUT * pw / ph);
  }
  const int cx = center_off(ow), cy = center_off(oh);

  if (band == 0 && threadIdx.x == 0) a.valid[crop] = valid;
  if (!valid) {  // an empty slot or an invalid crop: bytes 0 and clip_norm(0)
    for (int i = threadIdx.x; i < ST_BAND * ST_OUT; i += ST_THREADS) {
      const int y = y0 + i / ST_OUT, x = i % ST_OUT;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (a.dst) a.dst[((crop * ST_OUT + y) * ST_OUT + x) * 3 + c] = 0;
        if (a.f32) a.f32[((crop * 3 + c) * ST_OUT + y) * ST_OUT + x] = __fdiv_rn(__fsub_rn(0.0f, a.mean[c]), a.std[c]);
      }
    }
    if (a.coeff) {
      int32_t* co = a.coeff + crop * 2 * ST_OUT * ST_REC;
      for (int i = threadIdx.x; i < ST_BAND * ST_REC; i += ST_THREADS) co[y0 * ST_REC + i] = 0;
      if (band == 0)
        for (int i = threadIdx.x; i < ST_OUT * ST_REC; i += ST_THREADS) co[ST_OUT * ST_REC + i] = 0;
    }
    return;
  }

  // coefficients of this band's rows and of the 224 produced columns, and the group's label bits
  {
    const uint32_t* label = a.label;
    in_group[threadIdx.x] = (uint8_t)((label[threadIdx.x] >> g) & 1u);
    if (threadIdx.x < ST_OUT) make_coeff(pw, ow, cx + threadIdx.x, xrec + threadIdx.x * ST_REC);
    if (threadIdx.x >= ST_THREADS - ST_BAND) {
      const int r = threadIdx.x - (ST_THREADS - ST_BAND);
      make_coeff(ph, oh, cy + y0 + r, yrec + r * ST_REC);
    }
  }
  __syncthreads();
  if (a.coeff) {
    int32_t* co = a.coeff + crop * 2 * ST_OUT * ST_REC;
    for (int i = threadIdx.x; i < ST_BAND * ST_REC; i += ST_THREADS) co[y0 * ST_REC + i] = yrec[i];
    if (band == 0)
      for (int i = threadIdx.x; i < ST_OUT * ST_REC; i += ST_THREADS) co[ST_OUT * ST_REC + i] = xrec[i];
  }
  int lo = 0x7fffffff, hi = 0;
  for (int r = 0; r < ST_BAND; ++r) {
    lo = min(lo, yrec[r * ST_REC]);
    hi = max(hi, yrec[r * ST_REC] + yrec[r * ST_REC + 1]);
  }
  const int nrows = min(max(hi - lo, 0), ST_CAP);  // (<= 56 by the bound above; the cut keeps LDS safe regardless)

  // horizontal pass: padded rows [lo, lo + nrows) of the virtual source -> bytes in LDS
  const uint8_t* pic = a.pic + (long)b * a.pic_ss;
  const uint8_t* sg = a.segm + (long)b * a.segm_ss;
  for (int i = threadIdx.x; i < nrows * ST_OUT; i += ST_THREADS) {
    const int r = i / ST_OUT, x = i - r * ST_OUT;
    const int32_t* rec = xrec + x * ST_REC;
    const int xmin = rec[0], n = rec[1];
    const int sy = lo + r - pad_y;  // row of the cut
    uint32_t c0 = 1u << (ST_BITS - 1), c1 = c0, c2 = c0;
    if (sy >= 0 && sy < ch) {  // (a zero-pad row adds nothing)
      const uint8_t* prow = pic + (long)(y_org + sy) * a.pic_pitch;
      const uint8_t* srow = sg + (long)(y_org + sy) * a.segm_pitch;
      for (int t = 0; t < n; ++t) {
        const int sx = xmin + t - pad_x;
        if (sx < 0 || sx >= cw) continue;
        const uint8_t* p = prow + 3L * (x_org + sx);
        uint32_t v0 = p[0], v1 = p[1], v2 = p[2];
        if ((mask_content || fill_mode) && !in_group[srow[x_org + sx]]) v0 = fill[0], v1 = fill[1], v2 = fill[2];
        const uint32_t kk = (uint32_t)rec[2 + t];
        c0 += v0 * kk, c1 += v1 * kk, c2 += v2 * kk;
      }
    }
    uint8_t* o = stage + r * ST_ROW_BYTES + 3 * x;
    o[0] = (uint8_t)clip8(c0), o[1] = (uint8_t)clip8(c1), o[2] = (uint8_t)clip8(c2);
  }
  __syncthreads();

  // vertical pass from LDS, the bytes and the CLIP normalisation t = fl(fl(fl(u / 255) - mean) / std)
  for (int i = threadIdx.x; i < ST_BAND * ST_OUT; i += ST_THREADS) {
    const int r = i / ST_OUT, x = i - r * ST_OUT;
    const int y = y0 + r;
    const int32_t* rec = yrec + r * ST_REC;
    const int ymin = rec[0], n = rec[1];
    uint32_t acc[3] = {1u << (ST_BITS - 1), 1u << (ST_BITS - 1), 1u << (ST_BITS - 1)};
    for (int t = 0; t < n; ++t) {
      const int sr = min(ymin + t - lo, ST_CAP - 1);
      const uint8_t* p = stage + sr * ST_ROW_BYTES + 3 * x;
      const uint32_t kk = (uint32_t)rec[2 + t];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += p[c] * kk;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t u = clip8(acc[c]);
      if (a.dst) a.dst[((crop * ST_OUT + y) * ST_OUT + x) * 3 + c] = (uint8_t)u;
      if (a.f32)
        a.f32[((crop * 3 + c) * ST_OUT + y) * ST_OUT + x] =
            __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), a.mean[c]), a.std[c]);
    }
  }
}

int check_maps(upk_ctx* ctx, const char* who, const uint8_t* pictures, long long pic_pitch, const uint8_t* segm,
               long long segm_pitch, int batch, int h, int w, const uint32_t* label_groups, int n_groups) {
  if (!pictures || !segm || !label_groups) return upk_fail(ctx, UPK_EINVAL, "%s: null pictures, label maps or group table", who);
  if (batch <= 0 || h <= 0 || w <= 0) return upk_fail(ctx, UPK_EINVAL, "%s: sizes must be positive", who);
  if (n_groups < 1 || n_groups > UPK_STYLE_MAX_GROUPS)
    return upk_fail(ctx, UPK_EINVAL, "%s: %d groups, 1 .. %d are supported", who, n_groups, UPK_STYLE_MAX_GROUPS);
  if (pic_pitch < 3LL * w) return upk_fail(ctx, UPK_EINVAL, "%s: picture pitch %lld below 3 * w = %lld", who, pic_pitch, 3LL * w);
  if (segm_pitch < (long long)w) return upk_fail(ctx, UPK_EINVAL, "%s: label map pitch %lld below w = %d", who, segm_pitch, w);
  if (h > ST_MAX_SIDE || w > ST_MAX_SIDE)
    return upk_fail(ctx, UPK_ESHAPE, "%s: a %d x %d picture, sides up to %d are supported", who, h, w, ST_MAX_SIDE);
  if (batch > 65535) return upk_fail(ctx, UPK_ESHAPE, "%s: batch %d above 65535", who, batch);
  return UPK_OK;
}

}  // namespace

extern "C" int upk_segm_boxes_u8(upk_ctx* ctx, const uint8_t* segm, long long segm_pitch, long long segm_sample_stride,
                                 const uint8_t* pictures, long long pic_pitch, long long pic_sample_stride, int batch, int h,
                                 int w, const uint32_t* label_groups_host, int n_groups, int32_t* boxes, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_maps(ctx, "segm_boxes", pictures, pic_pitch, segm, segm_pitch, batch, h, w, label_groups_host, n_groups);
  if (rc != UPK_OK) return rc;
  if (!boxes || ((uintptr_t)boxes & 3)) return upk_fail(ctx, UPK_EINVAL, "segm_boxes: boxes must be a 4-byte aligned device pointer");
  BoxArgs a;
  memset(&a, 0, sizeof(a));
  a.segm = segm, a.pic = pictures, a.boxes = boxes;
  a.segm_pitch = segm_pitch, a.segm_ss = batch > 1 ? segm_sample_stride : 0;
  a.pic_pitch = pic_pitch, a.pic_ss = batch > 1 ? pic_sample_stride : 0;
  a.h = h, a.w = w, a.n_groups = n_groups;
  memcpy(a.label, label_groups_host, sizeof(a.label));
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(segm_boxes_kernel, dim3((unsigned)n_groups, (unsigned)batch), dim3(BX_THREADS), 0, (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "segm_boxes");
}

extern "C" int upk_style_crops_u8(upk_ctx* ctx, const uint8_t* pictures, long long pic_pitch, long long pic_sample_stride,
                                  const uint8_t* segm, long long segm_pitch, long long segm_sample_stride, int batch, int h,
                                  int w, const uint32_t* label_groups_host, int n_groups, const int32_t* boxes,
                                  const int32_t* group_flags_host, const int32_t* slot_groups_host, int n_slots,
                                  const float* mean_std_host, uint8_t* dst_u8, float* dst_f32, int32_t* valid,
                                  int32_t* coeff_out, upk_stream stream_) {
  if (!ctx) return UPK_EINVAL;
  const int rc = check_maps(ctx, "style_crops", pictures, pic_pitch, segm, segm_pitch, batch, h, w, label_groups_host, n_groups);
  if (rc != UPK_OK) return rc;
  if (!boxes || !group_flags_host || !slot_groups_host || !mean_std_host || !valid)
    return upk_fail(ctx, UPK_EINVAL, "style_crops: null boxes, group flags, slot map, constants or valid");
  if (!dst_u8 && !dst_f32) return upk_fail(ctx, UPK_EINVAL, "style_crops: no destination");
  if (((uintptr_t)boxes | (uintptr_t)valid | (uintptr_t)coeff_out | (uintptr_t)dst_f32) & 3)
    return upk_fail(ctx, UPK_EINVAL, "style_crops: boxes, valid, coeff_out and the fp32 destination must be 4-byte aligned");
  if (n_slots < 1 || n_slots > UPK_STYLE_MAX_SLOTS)
    return upk_fail(ctx, UPK_EINVAL, "style_crops: %d slots, 1 .. %d are supported", n_slots, UPK_STYLE_MAX_SLOTS);
  for (int s = 0; s < n_slots; ++s)
    if (slot_groups_host[s] < -1 || slot_groups_host[s] >= n_groups)
      return upk_fail(ctx, UPK_EINVAL, "style_crops: slot %d names group %d of %d", s, slot_groups_host[s], n_groups);
  for (int g = 0; g < n_groups; ++g)
    if (group_flags_host[g] < 0) return upk_fail(ctx, UPK_EINVAL, "style_crops: negative flags of group %d", g);
  for (int c = 0; c < 3; ++c)
    if (!(mean_std_host[3 + c] > 0.0f)) return upk_fail(ctx, UPK_EINVAL, "style_crops: std[%d] must be positive", c);
  StyleArgs a;
  memset(&a, 0, sizeof(a));
  a.pic = pictures, a.segm = segm, a.boxes = boxes, a.dst = dst_u8, a.f32 = dst_f32, a.valid = valid, a.coeff = coeff_out;
  a.pic_pitch = pic_pitch, a.pic_ss = batch > 1 ? pic_sample_stride : 0;
  a.segm_pitch = segm_pitch, a.segm_ss = batch > 1 ? segm_sample_stride : 0;
  a.h = h, a.w = w, a.n_groups = n_groups, a.n_slots = n_slots;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean_std_host[c], a.std[c] = mean_std_host[3 + c];
  memcpy(a.label, label_groups_host, sizeof(a.label));
  memcpy(a.gflags, group_flags_host, sizeof(int32_t) * n_groups);
  for (int s = 0; s < n_slots; ++s) a.slot[s] = slot_groups_host[s];
  upk_prof_scope prof(ctx, UPK_CLS_OTHER, (hipStream_t)stream_);
  hipLaunchKernelGGL(style_crops_kernel, dim3(ST_OUT / ST_BAND, (unsigned)n_slots, (unsigned)batch), dim3(ST_THREADS), 0,
                     (hipStream_t)stream_, a);
  return upk_check_launch(ctx, "style_crops");
}
