/*
 * upk.h — C ABI of libupk.so, the MI355X (gfx950) kernel library under the
 * UPGPT denoising hot path (UNetModel.forward x DDIMSampler loop -> VAE decode).
 *
 * The reference (soon-yau/upgpt) has NO native boundary: below its Python
 * modules there is only torch.nn.functional.  Every entry
 * point here therefore cites the reference *Python* call site whose ATen
 * dispatch it replaces.  Bindings: upgpt_amd/_lib.py (ctypes); INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Rules of the ABI:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     unless the name says host;
 *   - every launcher enqueues on the given hipStream_t, never synchronises,
 *     never allocates (workspace is caller-provided through upk_set_workspace),
 *     is safe to capture in a HIP graph, and returns 0 or a negative UPK_E*;
 *   - no global mutable state outside upk_ctx.  A context is NOT thread-safe:
 *     one host thread per context at a time (one context per GPU process is
 *     the intended use); different contexts are independent;
 *   - the only entry points that synchronise or allocate are the offline
 *     tools: upk_conv_autotune (times launches; with UPK_TUNE_COLD it keeps a
 *     512 MB cache-flush buffer in the context until upk_destroy) and the
 *     upk_prof_* collectors.
 *
 * Activation layout: NHWC / token-major fp16 ([B, H*W, C] == [M, C] row major,
 * leading dimension given in elements).  NCHW fp32 only at the public boundary
 * (upk_nchw_f32_to_nhwc_f16, UPK_F_OUT_NCHW_F32).
 */
#ifndef UPK_H_
#define UPK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UPK_VERSION 100 /* 0.1.0 */

/* error codes */
#define UPK_OK 0
#define UPK_EINVAL (-1)     /* bad argument (null pointer, misaligned, negative size) */
#define UPK_ESHAPE (-2)     /* shape not supported by any compiled kernel variant */
#define UPK_EWORKSPACE (-3) /* split-K needs more workspace than was provided */
#define UPK_EHIP (-4)       /* a HIP runtime call failed; see upk_last_error */
#define UPK_ENODEV (-5)     /* no gfx950 device */

typedef struct upk_ctx upk_ctx;
typedef void* upk_stream; /* hipStream_t */

int upk_version(void);
/* Binds to HIP device `device` (hipSetDevice is NOT called by launchers; the
 * caller keeps the device current). */
int upk_create(upk_ctx** out, int device);
int upk_destroy(upk_ctx* ctx);
const char* upk_last_error(upk_ctx* ctx);
/* Caller-owned scratch for split-K partial sums (fp16 slabs [z][m][n_pad], accumulated in fp32 inside each slice and
 * summed in fp32 by the reduce pass; fixed slice order, so results are deterministic).  May be NULL/0. */
int upk_set_workspace(upk_ctx* ctx, void* dptr, size_t bytes);
/* Number of compute units of the bound device (256 on MI355X). */
int upk_num_cus(upk_ctx* ctx);

/* ------------------------------------------------------------------ */
/* Weight packing (done once at load).                                  */
/* ------------------------------------------------------------------ */
/* Packed layout consumed by upk_conv2d_nhwc_f16 / upk_gemm_f16:
 *   fp16 [K/32][n_pad][32], k = (ky*kw + kx) * cin_pad + ci,
 *   cin_pad = round_up(cin, 32), n_pad = round_up(n_rows, 16), zero filled.
 * `row_map` (device int32[n_rows_packed], may be NULL = identity) gives, for
 * each packed row, the source output channel or -1 for a zero row: this is how
 * head-dim padding (28->32 ...) and the GEGLU value/gate interleave are made.
 * `col_map` (device int32[cin_packed], may be NULL) likewise maps packed input
 * channels to source input channels (-1 = zero column).
 * Source: fp32 OIHW conv weight (openaimodel.py:204,230,519,685; model.py) or
 * fp32 [out,in] Linear weight (attention.py:161-168,40,60) with kh=kw=1. */
int upk_pack_weight_f16(upk_ctx* ctx, const float* w_oihw, int cout, int cin, int kh, int kw,
                        const int32_t* row_map, int n_rows_packed, const int32_t* col_map,
                        int cin_packed, void* w_packed, upk_stream stream);
/* bytes needed for the packed weight */
size_t upk_packed_weight_bytes(int n_rows_packed, int cin_packed, int kh, int kw);

/* ------------------------------------------------------------------ */
/* Implicit-GEMM convolution / Linear (MFMA).                           */
/* ------------------------------------------------------------------ */
/* flags */
#define UPK_F_SILU 0x1         /* y = silu(acc + bias ...) (openaimodel.py:509)            */
#define UPK_F_GEGLU 0x2        /* y[:, j] = v * gelu_erf(g) (attention.py:42-44); weight    */
                               /* rows packed as [32 value | 32 gate] per 64-row block       */
#define UPK_F_OUT_F32 0x4      /* y is fp32 [M, ldy]                                         */
#define UPK_F_OUT_NCHW_F32 0x8 /* y is fp32 NCHW [B, N, Ho, Wo] (public boundary)            */
#define UPK_F_UPSAMPLE2X 0x10  /* input is nearest-2x upsampled on the fly                   */
                               /* (openaimodel.py:116 + :107; model.py:53-56)                */
#define UPK_F_PAD_ASYM 0x20    /* stride-2 conv with (0,1,0,1) padding (model.py:72-76)      */
#define UPK_F_QUICKGELU 0x40   /* y = v * sigmoid(1.702 v) after bias (CLIP text MLP, hidden_act quick_gelu) */

typedef struct upk_conv_desc {
  /* input: up to two NHWC fp16 sources concatenated along C (openaimodel.py:736,
   * ddpm.py:1568).  c1, c2 multiples of 32 (pad with zero channels); x2 may be NULL. */
  const void* x1;
  const void* x2;
  int32_t c1, c2;
  int32_t ld1, ld2; /* pixel stride in elements */
  int32_t batch;
  int32_t in_h, in_w; /* STORED spatial dims of the sources (before 2x upsample) */
  int32_t ksize;      /* 1 or 3 */
  int32_t stride;     /* 1 or 2 */
  /* weights + epilogue */
  const void* w_packed; /* upk_pack_weight_f16 layout, K = ksize^2 * (c1+c2) */
  int32_t n_out;        /* valid output columns (GEGLU: packed rows = 2*n_out)     */
  int32_t n_pad;        /* packed rows (multiple of 16)                            */
  const float* bias;    /* [n_pad] fp32 in PACKED row order, or NULL               */
  const void* residual; /* fp16 [M, ld_res] added after bias/act, or NULL          */
  int32_t ld_res;
  /* per-sample broadcast add (ResBlock emb_out, openaimodel.py:273):
   * rowvec[(step * rv_step_stride) + b * rv_batch_stride + n], fp32. */
  const float* rowvec;
  int32_t rv_batch_stride;
  int32_t rv_step_stride;
  const int32_t* step; /* device scalar, NULL => 0 */
  void* y;
  int32_t ldy;
  /* optional transposed tail: packed columns >= vt_from are written to
   * vt[((b*vt_heads + h)*vt_dhead + d)*vt_ld + tok] (V^T for upk_attention_f16),
   * with m = b*vt_tokens + tok, col - vt_from = h*vt_dhead + d.  vt==NULL: off. */
  void* vt;
  int32_t vt_from, vt_heads, vt_dhead, vt_ld, vt_tokens;
  int32_t flags;
  /* tile configuration = tune_cfg - 1 and split-K factor chosen by upk_conv_autotune
   * (0 = let the built-in cost model decide). */
  int32_t tune_cfg, tune_splitk;
  /* LayerNorm folded into a Linear (BasicTransformerBlock norm1/2/3 -> to_q|k|v / to_q / GEGLU proj,
   * attention.py:203-215): with ln_colsum != NULL the rows of x1 are the UN-normalised residual stream
   * (ksize 1, c2 == 0), the packed weight must be W * gamma (column scaled), bias must be b + W @ beta,
   * ln_colsum[n] = sum_k fp16(W*gamma)[n, k] in PACKED row order (fp32 [n_pad]); the kernel takes each
   * row's mean / variance over its first ln_dim channels (fp32, from the fp16 tiles it stages anyway)
   * and finishes  y = rstd * (x @ W'^T - mean * colsum) + bias'  before the usual epilogue. */
  const float* ln_colsum;
  float ln_eps;
  int32_t ln_dim;
  /* GroupNorm statistics of the OUTPUT as a by-product of the launch, so that the following GroupNorm can run
   * upk_groupnorm_apply_nhwc_f16 only.  With gn_stats_ws != NULL and a plain fp16 NHWC epilogue
   *   mode 1: a split-K launch's reduce pass (it touches every output element anyway) writes the per-chunk
   *           per-group partials of upk_groupnorm_nhwc_f16 (n_out % 8 == 0, 16-byte aligned rows);
   *   mode 2: an unsplit launch whose M tiles lie inside one sample writes per-(M tile, channel) partials
   *           [batch][nblk][2][n_pad] from its epilogue.
   * gn_stats_ws must hold batch * 32 * 2 * max(n_pad, 32) floats.  upk_conv_gn_fused() returns the mode (0 = none:
   * the consumer has to run the full GroupNorm) and nblk for a descriptor; both depend on the tuned / overridden /
   * cost-model (tile, split-K) choice, the same decision procedure as the launch. */
  float* gn_stats_ws;
  int32_t gn_groups;
  /* Appended 1x1 K segment — the ResBlock skip projection folded into its second conv
   * (openaimodel.py:274-275: `skip_connection(x) + h` with skip_connection = conv1x1 when channels change):
   *   y = conv_ksize(x1 | x2) + conv1x1(x3 | x4) + bias ...
   * x3 (and optionally x4, concatenated along C like x1 | x2) are NHWC fp16 sources with the OUTPUT's spatial
   * dims (stride 1, no upsample); c3, c4 multiples of 32.  The packed weight is the main weight followed by the
   * 1x1 weight along K ((ksize^2 (c1+c2) + c3+c4) / 32 chunks of [n_pad][32]); bias = sum of both biases.
   * Wave-specialised tile configurations only (the classic kernels refuse).  x3 == NULL: off. */
  const void* x3;
  const void* x4;
  int32_t c3, c4;
  int32_t ld3, ld4;
  /* GroupNorm (+ SiLU) of the OUTPUT applied by the split-K reduce pass (gn_fused mode 3): when this launch splits
   * K (tuned / cost-model choice) and its epilogue is plain (bias + timestep row vector + residual -> fp16 NHWC),
   * the reduce pass runs one workgroup per (sample, group): it sums the slabs, writes y (unless gno_skip_y: nobody
   * but the GroupNorm reads it), takes the group's mean / variance from the fp16-rounded values it holds in
   * registers and writes SiLU?(GroupNorm(y)) * gamma + beta to gno_y (row stride gno_ld) — the GroupNorm launch
   * that would follow (ResBlock in_layers / out_layers, openaimodel.py:255-275; SpatialTransformer.norm,
   * attention.py:250) is not needed.  gn_groups gives the group count.  Launches that do not split K ignore these
   * fields (upk_conv_gn_fused reports what will happen). */
  const float* gno_gamma;
  const float* gno_beta;
  void* gno_y;
  float gno_eps;
  int32_t gno_silu, gno_ld, gno_skip_y;
  /* LayerNorm row statistics handed from the launch that PRODUCES a tensor to the folded-LayerNorm Linear that reads
   * it (BasicTransformerBlock: attn1/attn2 to_out -> norm2/norm3 -> to_q / GEGLU proj, proj_in -> norm1 -> q|k|v;
   * attention.py:203-215).  Producer: ln_rows_out = [8][M][2] floats; a plain-epilogue launch that does not split K
   * writes, per output row and per column slot, the sum and the sum of squares of the fp16 values it stores
   * (upk_conv_ln_rows reports the slot count, 0 = this launch cannot).  Consumer: ln_colsum / ln_eps / ln_dim as
   * for the in-kernel fold, plus ln_rows_in (the producer's buffer) and ln_rows_slots: the row statistics are read
   * instead of being taken from the operand tile, so every tile configuration can run the GEMM. */
  float* ln_rows_out;
  const float* ln_rows_in;
  int32_t ln_rows_slots;
  /* Upsample (openaimodel.py:109-119, model.py:41-56: F.interpolate(scale_factor=2, mode="nearest") -> conv3x3 p1) as
   * four 2x2 convolutions on the LOW-resolution grid, 4/9 of the multiply-adds: with UPK_F_UPSAMPLE2X, ksize 3,
   * stride 1 and w_phase != NULL the launch computes, for phase (py, px) in {0,1}^2, output pixel (2y + py, 2x + px)
   * from low-resolution rows {y + py - 1, y + py} x columns {x + px - 1, x + px}.  w_phase = the four phase
   * weights, each packed like a 2x2 conv weight [n_pad][2][2][c1 + c2] (upk_pack_weight_f16 with kh = kw = 2), phase
   * p = 2 py + px at w_phase + p * n_pad * 4 * (c1 + c2) halfs, where tap (ty, tx) of phase (py, px) is the sum of
   * the 3x3 taps (ky, kx) with (py + ky - 1) >> 1 == py + ty - 1 and likewise for x.  Plain epilogue only (bias ->
   * fp16 NHWC / fp32); w_packed stays the 3x3 weight (used when the launch cannot take the phase form). */
  const void* w_phase;
  /* Row-block capacity of gn_stats_ws for the per-(row block, channel) partials of an unsplit launch (mode 2): 0 = 32
   * (batch * 32 * 2 * max(n_pad, 32) floats); larger values (buffer: batch * cap * 2 * max(n_pad, 32) floats) let
   * launches with many M tiles per sample — the VAE decoder's 64x64 ... 256x256 feature maps — leave their partials
   * too; a consumer then folds them with upk_groupnorm_finalize_f32 before upk_groupnorm_apply_nhwc_f16 (mode 1). */
  int32_t gn_stats_cap;
  /* Weight prefetch for the NEXT weight-consuming launch of this stream (round 6).  Inside the sampler
   * loop every weight is cold when its launch starts: 0.85 GB of weights and ~2.7 GB of activations per forward pass
   * through a 32 MB L2 and a 256 MB memory-side cache between two uses (a launch on cold weights costs 9-32 % more than on
   * warm ones, profiles/r06_weight_temperature_4_lanes.txt).  Measured (profiles/r06_next_weight_prefetch.txt): one forward
   * alone 2.83 -> 2.76 ms, with four forwards in flight 1.461 -> 1.471 ms — the host arms it only for the former.  With
   * pf_next != NULL the wave-specialised kernels' MFMA waves, idle while the first ring stage is in flight, touch one
   * 16-byte piece of every 128-byte line of pf_next[0 .. pf_bytes) (direct-to-LDS loads into the dump row group: no
   * registers, nothing to wait for), each workgroup its share: the lines are in the memory-side cache when the next
   * launch — upk_conv_link_prefetch's caller passes the packed weight of the next conv / Linear — asks for them.  Other
   * kernel families ignore the fields.  Purely a performance hint: results never depend on it. */
  const void* pf_next;
  int64_t pf_bytes;
} upk_conv_desc;

/* Replaces F.conv2d (3x3 s1/s2 p1, 1x1) / F.linear call sites:
 * ResBlock (openaimodel.py:255-275), Downsample (:158-160), Upsample (:109-119),
 * SpatialTransformer.proj_in/out (attention.py:233-248), CrossAttention
 * to_q/k/v/out (attention.py:161-168), GEGLU/FeedForward (attention.py:40,60),
 * time_embed/emb_layers (openaimodel.py:506-511,220), VAE Decoder convs
 * (model.py:462-568).  A Linear is ksize=1, batch=1, in_h=M, in_w=1. */
int upk_conv2d_nhwc_f16(upk_ctx* ctx, const upk_conv_desc* d, upk_stream stream);

/* Which GroupNorm by-product upk_conv2d_nhwc_f16(d) will leave in d->gn_stats_ws (see upk_conv_desc): *mode in
 * {0, 1, 2, 3}, *nblk = row blocks per sample for mode 2; 3 = the reduce pass applies the GroupNorm itself (gno_*) and
 * leaves no statistics.  Nothing is enqueued. */
int upk_conv_gn_fused(upk_ctx* ctx, const upk_conv_desc* d, int* mode, int* nblk);
/* Folds per-(row block, channel) partials ([batch][nblk][2][ld], any nblk) into the per-(chunk, group) layout of
 * upk_groupnorm_nhwc_f16's workspace (everything in chunk 0, zeros elsewhere), so that
 * upk_groupnorm_apply_nhwc_f16(..., stats = ws, stats_mode = 1, ...) can follow: GroupNorm of a tensor whose producer
 * conv ran more than 32 M tiles per sample, without a statistics pass over the tensor.  c channels, hw pixels. */
int upk_groupnorm_finalize_f32(upk_ctx* ctx, const float* partials, int nblk, int ld, int batch, int hw, int c,
                               int groups, float* ws, upk_stream stream);
/* Number of column slots upk_conv2d_nhwc_f16(d) will fill in d->ln_rows_out (0: none — the launch splits K across workgroups or has no
 * plain epilogue).  Nothing is enqueued. */
int upk_conv_ln_rows(upk_ctx* ctx, const upk_conv_desc* d, int* slots);

/* Fused feed-forward tail of a SpatialTransformer block — BasicTransformerBlock.norm3 -> FeedForward (GEGLU, erf GELU)
 * -> + residual (attention.py:42-64, 215) followed by SpatialTransformer.proj_out -> + x_in (attention.py:259-261) —
 * as ONE launch; the 4c-wide hidden activation stays on the CU (the resident form keeps all of it in LDS, the streaming
 * form two 128-column slices of it):
 *     h   = (xn W1v^T + b1v) * gelu(xn W1g^T + b1g),  xn = LayerNorm(x)          [m, inner]
 *     y   = residual + [h | x] W2^T + b2                                          [m, n_out]
 * x: un-normalised rows [m, ldx] (c channels, c % 224 == 0); w1 / b1 / u1: the GEGLU Linear packed as for
 * upk_conv2d_nhwc_f16 with UPK_F_GEGLU and ln_colsum (W * gamma in [32 value | 32 gate] row blocks, b + W beta, column
 * sums of the fp16-rounded rows), inner = 4 c; w2: packed [n_pad rows][K = inner + c] weight whose K order is [h | x]
 * (Packer.append_1x1(P F2, P) for ff.net.2 / proj_out), b2 [n_pad]; n_pad <= 256.  rows_per_wg: 32 or 64 (0 = 64): the resident
 * form, for a launch that has the chip to itself; 128, or 64 | UPK_MLP_STREAM: the streaming form (c = 224 only), whose
 * m / 128 workgroups stream the weights a quarter as often, for launches that share the chip with other batches.  Same K order
 * per row in both forms: at equal rows the results are bit-identical.
 * gn_stats_ws != NULL: per-(row block, channel) GroupNorm partials [m / hw][hw / rows_per_wg][2][n_pad] of y, as
 * upk_conv_desc.gn_stats_ws mode 2 (hw = rows per sample, a multiple of rows_per_wg). */
#define UPK_MLP_STREAM 0x1000 /* or-ed into upk_mlp_desc.rows_per_wg: the streaming form at that tile height */
typedef struct upk_mlp_desc {
  const void* x;
  int32_t ldx, m, c, inner;
  const void* w1;
  const float* b1;
  const float* u1;
  float ln_eps;
  int32_t ln_dim;
  const void* w2;
  const float* b2;
  int32_t n_out, n_pad;
  const void* residual;
  int32_t ld_res;
  void* y;
  int32_t ldy;
  float* gn_stats_ws;
  int32_t hw, rows_per_wg;
} upk_mlp_desc;
int upk_geglu_mlp_f16(upk_ctx* ctx, const upk_mlp_desc* d, upk_stream stream);
/* 1 if upk_geglu_mlp_f16 takes the shape, else 0: the 7 * 32 channel family, n_pad <= 256, rows_per_wg one of the values above,
 * the LDS of the form within 160 KB — resident (5 c / 32) * rows * 64 B, i.e. c = 224 up to 64 rows; streaming (c / 32 + 8) * rows
 * * 64 B, i.e. c = 224 up to 128 rows and c = 448 refused at 128 — and, with gn_stats_ws, hw a multiple of rows with at most 32
 * row blocks per sample. */
int upk_geglu_mlp_supported(upk_ctx* ctx, const upk_mlp_desc* d);

/* The cross-attention half of a BasicTransformerBlock (attention.py:257-260 with the context K / V precomputed) as one
 * launch:  t1 = a1 W_out1^T + b_out1 + t0;  q = LayerNorm(t1) W_q^T;  a2 = softmax(q K^T scale) V per head;
 * y = a2 W_out2^T + b_out2 + t1.   a1 [m, lda]: self-attention output, heads side by side at the padded head width d;
 * w_out1 / w_out2: packed [c rows][K = heads * d] (upk_pack_weight with the head padding as column map); w_q: packed
 * [heads * d rows][K = c] with the LayerNorm affine folded in (as ln_colsum weights); vec = [b_out1 (c) | colsum_q
 * (heads * d) | bias_q (heads * d) | b_out2 (c)] fp32, zero padded to a multiple of 256 floats; k_ctx [batch * n_kv, ldk],
 * vt_ctx [batch, heads, d, vt_ld] as upk_attention_f16 takes them (n_kv <= 96 <= vt_ld).  Rows >= n_kv of a sample's
 * k_ctx are never read.  Columns [n_kv, 96) of vt_ctx ARE read, and multiplied by softmax weights that are exactly 0:
 * they must hold finite values (the engine zero-fills them; an inf or a NaN there reaches y).  hw = rows per sample (a
 * multiple of rows_per_wg: 16 or 32, 0 = 32; (c, d) = (224, 32) also 64 and 128 — m / 128 workgroups that stream the
 * weights a quarter as often, for launches that share the chip with other batches; the tile must fit 160 KB of LDS).
 * Shapes: heads = 8, (c, d) in {(224, 32), (448, 64)}. */
typedef struct upk_xblock_desc {
  const void* a1;
  int32_t lda, m, c, heads, d;
  const void* t0;
  int32_t ld_t0;
  const void* w_out1;
  const void* w_q;
  const void* w_out2;
  const float* vec;
  float ln_eps;
  int32_t ln_dim;
  const void* k_ctx;
  int32_t ldk, n_kv;
  const void* vt_ctx;
  int32_t vt_ld;
  float scale;
  void* y;
  int32_t ldy;
  int32_t hw, rows_per_wg;
} upk_xblock_desc;
int upk_cross_block_f16(upk_ctx* ctx, const upk_xblock_desc* d, upk_stream stream);
/* 1 if upk_cross_block_f16 takes the shape, else 0. */
int upk_cross_block_supported(upk_ctx* ctx, const upk_xblock_desc* d);

/* The head of a SpatialTransformer (attention.py:330-333, 257) as one launch: t0 = x W_in^T + b_in (x = the GroupNorm
 * output, proj_in a 1x1 conv), q | k | v = LayerNorm(t0) W_qkv^T.  w_in: packed [c rows][K = c]; w_qkv: packed
 * [3 heads d rows][K = c] in q | k | v order at the padded head width, LayerNorm affine folded in; vec = [b_in (c) |
 * colsum_qkv (3 heads d) | bias_qkv (3 heads d)] fp32, zero padded to a multiple of 256 floats.  t0 [m, ld_t0];
 * qk [m, ld_qk] = q | k; vt [m / hw, heads, d, vt_ld] = v transposed (vt_ld >= hw).  hw = rows per sample, a multiple of
 * rows_per_wg (16, 32, 64 or 128, 0 = 32; 64 and 128 as for upk_cross_block_f16).  Shapes: heads = 8, c = 224, d = 32. */
typedef struct upk_hblock_desc {
  const void* x;
  int32_t ldx, m, c, heads, d;
  const void* w_in;
  const void* w_qkv;
  const float* vec;
  float ln_eps;
  int32_t ln_dim;
  void* t0;
  int32_t ld_t0;
  void* qk;
  int32_t ld_qk;
  void* vt;
  int32_t vt_ld;
  int32_t hw, rows_per_wg;
  /* gn_part != NULL: x is the UN-normalised input of SpatialTransformer.norm (attention.py:330, GroupNorm without
   * SiLU) and the normalisation is applied to the tile inside the kernel, bit-identical to a upk_groupnorm_apply launch:
   * gn_part = the per-(row block, channel) partial sums [m / hw][gn_nblk][2][gn_ld] the producer of x left (gn_stats_ws
   * mode 2, gn_nblk <= 32), gn_gamma / gn_beta [c], gn_groups groups. */
  const float* gn_part;
  const float* gn_gamma;
  const float* gn_beta;
  int32_t gn_nblk, gn_ld, gn_groups;
  float gn_eps;
} upk_hblock_desc;
int upk_head_block_f16(upk_ctx* ctx, const upk_hblock_desc* d, upk_stream stream);
int upk_head_block_supported(upk_ctx* ctx, const upk_hblock_desc* d);

/* Convenience wrapper: y[M,N] = act(A[M,K] @ W^T + bias) + residual. */
int upk_gemm_f16(upk_ctx* ctx, const void* a, int lda, int m, int k, const void* w_packed,
                 int n_out, int n_pad, const float* bias, const void* residual, int ld_res,
                 void* y, int ldy, int flags, upk_stream stream);

/* Times every (tile configuration, split-K) candidate for this descriptor with HIP events on
 * `stream` (synchronises; call at plan-build time, never inside a captured region) and
 * returns the fastest pair (cfg is 0-based), its time, and the time of the cost model's
 * default choice.  The outputs of the descriptor are overwritten `reps` times per candidate. */
int upk_conv_autotune(upk_ctx* ctx, const upk_conv_desc* d, upk_stream stream, int reps, int* best_cfg,
                      int* best_splitk, float* best_us, float* default_us);

/* Forces a tile configuration / split-K factor for the next launches (tuning
 * and tests). cfg < 0 and splitk <= 0 restore the heuristic. */
int upk_conv_override(upk_ctx* ctx, int cfg, int splitk);
/* Number of compiled tile configurations, and a description of one.  Three families, in this order (tuning files
 * store indices: a family is only ever appended): the implicit-GEMM kernels ("4x4x2x2k2[wN]": classic and
 * wave-specialised), the A-stationary Linears ("as2x7p8": 1x1 only; the split-K slot means output-column passes per
 * workgroup) and the big-tile convs ("bt4x8x4x2n4": launches with at least one tile per CU, plain epilogues unless K
 * is split).  A configuration that cannot run a descriptor is refused (UPK_ESHAPE), never approximated. */
int upk_conv_num_configs(void);
const char* upk_conv_config_name(int cfg);

/* ------------------------------------------------------------------ */
/* Fused attention: softmax(Q K^T * scale) V, online softmax, no n^2 tensor. */
/* Replaces attention.py:178-192 (einsum/softmax/einsum) and model.py:180-196. */
/* ------------------------------------------------------------------ */
/* q  : fp16 [B, n_q , ldq ] head h at columns [h*d, (h+1)*d)
 * k  : fp16 [B, n_kv, ldk ] same head layout, batch stride = k_batch_stride elements
 * vt : fp16 [B, heads, d, vt_ld] (V transposed, vt_ld >= round_up(n_kv,32); the key columns
 *      [n_kv, round_up(n_kv,32)) of every row must hold zeros: a masked weight of 0 still
 *      multiplies them; columns at or beyond round_up(n_kv,32) are never read)
 * out: fp16 [B, n_q , ldo ]
 * d in {32, 64, 128, 256, 512} (head dims are padded to these by weight packing). */
int upk_attention_f16(upk_ctx* ctx, const void* q, int ldq, long long q_batch_stride,
                      const void* k, int ldk, long long k_batch_stride, const void* vt, int vt_ld,
                      void* out, int ldo, long long o_batch_stride, int batch, int heads, int n_q,
                      int n_kv, int d, float scale, upk_stream stream);

/* Causal self-attention (n_q == n_kv == n, key j visible to query i iff j <= i): the CLIP text transformer of the
 * conditioning stage (ldm/modules/encoders/modules.py:137-162 -> transformers CLIPTextModel). */
int upk_attention_causal_f16(upk_ctx* ctx, const void* q, int ldq, long long q_batch_stride,
                             const void* k, int ldk, long long k_batch_stride, const void* vt, int vt_ld,
                             void* out, int ldo, long long o_batch_stride, int batch, int heads, int n,
                             int d, float scale, upk_stream stream);

/* Cross-attention with the query projection inside: out = softmax(to_q(LayerNorm(x)) K^T * scale) V —
 * CrossAttention.forward (attention.py:170-196) behind BasicTransformerBlock.norm2 (attention.py:213), for the
 * attention whose K / V come from the (step-invariant) context.  x: [batch][n_q][ldx] fp16 un-normalised rows,
 * cq = 224 * n channels of which the first ln_dim are real.  wq: fp16 [heads][d][cq], W * gamma (LayerNorm affine
 * folded in), head dim zero-padded to d, the d rows of each head stored in the order
 *   row (32 kd + 16 t + m)  holds  d = 32 kd + 8 (m >> 2) + 4 t + (m & 3)      (t = 0,1; m = 0..15)
 * so that the projection's MFMA output is the score MFMA's operand fragment as it stands; wq_colsum / wq_bias:
 * [heads * d] fp32 in natural d order, column sums of the fp16-rounded wq rows and W beta (+ bias).  d in {32, 64}.
 * k / vt / out as upk_attention_f16. */
int upk_attention_qproj_f16(upk_ctx* ctx, const void* x, int ldx, long long xbs, int cq, int ln_dim, float ln_eps,
                            const void* wq, const float* wq_colsum, const float* wq_bias, const void* k, int ldk,
                            long long kbs, const void* vt, int vt_ld, void* out, int ldo, long long obs, int batch,
                            int heads, int n_q, int n_kv, int d, float scale, upk_stream stream);

/* Which kernel an attention launch runs.  The library compiles upk_attention_num_variants() instantiations:
 * "direct32q1" ... "direct128q2" (head dim 32 / 64 / 128, one or two 16-query groups per wave), "direct256",
 * "direct512", "lds32q1" ... "lds64q2" (K / V^T tiles of 64 keys staged in LDS), "wide512" (one head of 512 on
 * LDS-shared 32-key tiles), "qproj32q2", "qproj64q1" (upk_attention_qproj_f16).  Indices are only ever appended.  The
 * direct and qproj kernels run 1, 2 or 4 waves per workgroup, the lds and wide kernels 4.  A launch picks the variant
 * and the waves per workgroup from the CU count, batch * heads and n_q (and, for wide512, from the strides and the
 * alignment of the pointers); the queries below run the same decision procedure as the launch and enqueue nothing.
 *
 * upk_attention_plan: what upk_attention_f16 (causal = 0) / upk_attention_causal_f16 (causal = 1, n_q == n_kv) would
 * run with these arguments (the launch's argument list as it stands; the stream is not used); the same errors as the
 * launch.  upk_attention_qproj_plan: the same for
 * upk_attention_qproj_f16 (the pointers do not enter its choice).
 *
 * upk_attention_override forces the variant and / or the waves per workgroup of the next launches of this context
 * (tests and tuning): variant < 0 and wpb <= 0 restore the heuristic (variant 0 is a variant).  Precedence: the override,
 * then the heuristic.  An override never bypasses what a kernel needs: the lds
 * variants need n_kv % 64 == 0, n_kv >= 256, vt_ld % 8 == 0 and no causal mask; wide512 needs one head, n_kv % 32 == 0,
 * ldk >= 512, ldq / ldk / vt_ld / batch strides % 8 == 0, 16-byte aligned q / k / vt and no causal mask; a variant runs
 * only at its own head dim and through its own entry point; wpb is 1, 2 or 4, and 4 for the lds and wide variants.
 * Anything else is refused (UPK_ESHAPE) before anything is launched, never approximated. */
int upk_attention_num_variants(void);
const char* upk_attention_variant_name(int variant);
int upk_attention_override(upk_ctx* ctx, int variant, int wpb);
int upk_attention_plan(upk_ctx* ctx, const void* q, int ldq, long long q_batch_stride, const void* k, int ldk,
                       long long k_batch_stride, const void* vt, int vt_ld, const void* out, int ldo,
                       long long o_batch_stride, int batch, int heads, int n_q, int n_kv, int d, float scale,
                       upk_stream stream, int causal, int* variant, int* wpb);
int upk_attention_qproj_plan(upk_ctx* ctx, int ldx, int cq, int ln_dim, int ldk, int vt_ld, int ldo, int batch, int heads,
                             int n_q, int n_kv, int d, int* variant, int* wpb);

/* Attention over a HANDFUL of keys: out = softmax(Q K^T * scale) V with 1 <= n_kv <= 16 — the cross-attention of
 * CLIPTextImageCrossAtten (ldm/modules/encoders/modules.py:259-323: 77 text tokens over 9 style embeddings, 8 heads
 * of 96).  q / out as upk_attention_f16; k and v: fp16 [B, n_kv, ldk] / [B, n_kv, ldv] in the NATURAL layout (head h
 * at columns [h*d, (h+1)*d), not transposed, no key padding), so they may be two column slices of one k|v GEMM output.
 * 8 <= d <= 128 with d % 8 == 0 (no head padding), n_q >= 1; every leading dimension a multiple of 8 and
 * >= heads * d; pointers and batch strides 16-byte aligned.  Anything else: UPK_ESHAPE, nothing is launched.
 * VALU kernel, one lane per query: fp32 scores, max-subtracted fp32 softmax, fp32 P V, fp16 output; columns of out
 * beyond heads * d are not written. */
int upk_attention_fewkeys_f16(upk_ctx* ctx, const void* q, int ldq, long long q_batch_stride, const void* k, int ldk,
                              long long k_batch_stride, const void* v, int ldv, long long v_batch_stride, void* out,
                              int ldo, long long o_batch_stride, int batch, int heads, int n_q, int n_kv, int d,
                              float scale, upk_stream stream);

/* x <- 0.5 x (1 + erf(x / sqrt 2)) in place over fp16 [rows, cols], rows ld apart: the activation of a CLIP MLP whose
 * hidden_act is "gelu" (laion CLIP), behind a plain fc1 GEMM.  fp32 math by the device function of the GEGLU
 * epilogues (the two agree bit for bit).  cols and ld multiples of 8, ld >= cols, x 16-byte aligned; else UPK_ESHAPE. */
int upk_gelu_f16(upk_ctx* ctx, void* x, int ld, int rows, int cols, upk_stream stream);

/* out[r, :] = tok_emb[ids[r], :] + pos_emb[r % seq, :]  (fp16 tables [vocab, dim] / [seq, dim], fp16 out [rows, ld]):
 * CLIPTextEmbeddings.  ids outside [0, vocab) are an error the kernel cannot report: validate on the host. */
int upk_embed_tokens_f16(upk_ctx* ctx, const int32_t* ids, const void* tok_emb, const void* pos_emb, int rows,
                         int seq, int dim, int vocab, void* out, int ld_out, upk_stream stream);

/* y[i, :] = x[idx[i], :] for i < n (fp16 rows of `dim` channels, idx = device int32[n], clamped to [0, n_src)):
 * the end-of-text pooling of `clip.model.CLIP.encode_text` (x[arange, text.argmax(-1)]) behind
 * FrozenCLIPTextEmbedder (ldm/modules/encoders/modules.py:164-198); the argmax over the token ids is host logic. */
int upk_gather_rows_f16(upk_ctx* ctx, const void* x, int ldx, const int32_t* idx, int n, int n_src, int dim,
                        void* y, int ldy, upk_stream stream);

/* CLIP image tower (ldm/modules/encoders/modules.py:234-256 -> clip.model.VisionTransformer):
 * patch embedding = upk_patchify_nchw_f32_f16 (non-overlapping p x p patches of an fp32 NCHW image -> fp16 rows
 * [batch*(H/p)*(W/p), ld_out], k = c*p*p + py*p + px, zero padded) followed by a plain upk_gemm_f16 with the
 * Conv2d(3, width, p, stride p) weight flattened; upk_vit_assemble_f16 prepends the class token and adds the
 * positional embedding: out[n, 0] = class_emb + pos[0], out[n, 1 + j] = patch_emb[n, j] + pos[1 + j]. */
int upk_patchify_nchw_f32_f16(upk_ctx* ctx, const float* x, int batch, int c, int h, int w, int patch, void* out,
                              int ld_out, upk_stream stream);
int upk_vit_assemble_f16(upk_ctx* ctx, const void* patch_emb, int ld_patch, const float* class_emb,
                         const float* pos_emb, int batch, int npatch, int dim, void* out, int ld_out,
                         upk_stream stream);

/* ------------------------------------------------------------------ */
/* Normalisation (wavefront reductions, fp32 statistics).               */
/* ------------------------------------------------------------------ */
/* GroupNorm over NHWC fp16, optional fused SiLU, input may be a 2-source
 * channel concat; output is one [B*HW, c1+c2] fp16 tensor.
 * Replaces GroupNorm32 (util.py:214-216, eps 1e-5), Normalize (attention.py:76-77
 * and model.py:38-39, eps 1e-6) and the following SiLU/swish (openaimodel.py:203,227).
 * stats_ws: fp32 scratch, >= upk_groupnorm_ws_bytes(batch, hw) bytes (its contents after the call are unspecified:
 * feature maps of <= 64 pixels are normalised by ONE launch that keeps a (sample, group) in registers and never
 * touches it; larger ones by a statistics pass that fills it and an apply pass that reads it).
 * Reproducibility: every path sums in a fixed order (reruns are bit-identical).  ACROSS paths — this call, the apply pass
 * on a producer's partial statistics (upk_groupnorm_apply_nhwc_f16), a normalising split-K reduce (gno_*) — results are
 * bit-identical for feature maps of > 64 pixels only; at <= 64 pixels the one-launch kernel sums in another order and
 * agrees to fp16 rounding (so a tensor may normalise to different bits under different tuning files, never within one). */
int upk_groupnorm_nhwc_f16(upk_ctx* ctx, const void* x1, int c1, int ld1, const void* x2, int c2,
                           int ld2, int batch, int hw, int groups, const float* gamma,
                           const float* beta, float eps, int fuse_silu, void* y, int ldy,
                           float* stats_ws, upk_stream stream);
size_t upk_groupnorm_ws_bytes(int batch, int hw);
/* First half of upk_groupnorm_nhwc_f16 only: the per-(chunk, group) partial sums [batch][nchunks][groups][2]
 * (nchunks = *nchunks of upk_groupnorm_chunks(hw)). */
int upk_groupnorm_stats_nhwc_f16(upk_ctx* ctx, const void* x1, int c1, int ld1, const void* x2, int c2, int ld2,
                                 int batch, int hw, int groups, float* stats_ws, upk_stream stream);
int upk_groupnorm_chunks(int hw);
/* Second half of upk_groupnorm_nhwc_f16 only: stats_ws already holds the partial sums of x1, left by the conv
 * launch that produced it (upk_conv_desc.gn_stats_ws): stats_mode / stats_nblk as reported by upk_conv_gn_fused,
 * stats_ld = that launch's n_pad.  A two-source (concat) input needs mode 2 for BOTH sources: stats_ws2 /
 * stats_nblk2 / stats_ld2 describe x2's producer (NULL / 0 / 0 for a single source). */
int upk_groupnorm_apply_nhwc_f16(upk_ctx* ctx, const void* x1, int c1, int ld1, const void* x2, int c2,
                                 int ld2, int batch, int hw, int groups, const float* gamma,
                                 const float* beta, float eps, int fuse_silu, void* y, int ldy,
                                 const float* stats_ws, int stats_mode, int stats_nblk, int stats_ld,
                                 const float* stats_ws2, int stats_nblk2, int stats_ld2, upk_stream stream);
/* Which kernels a GroupNorm call runs.  upk_groupnorm_num_paths() paths, named by upk_groupnorm_path_name ("?" outside):
 * "onepass_v<V>n<NV>" = the one-launch kernel for feature maps of <= 64 pixels, a thread owning up to NV vectors of V
 * channels of one group (V = the largest of 8 / 4 / 2 that divides the group width; an odd width has none), and
 * "twopass" = the statistics pass and / or the apply pass.
 * upk_groupnorm_plan: what upk_groupnorm_nhwc_f16 (with_stats = with_apply = 1), upk_groupnorm_stats_nhwc_f16
 * (1, 0) or upk_groupnorm_apply_nhwc_f16 (0, 1) would run for these sizes: the launchers take their decision from the same
 * function.  *nchunks / *pix_per_chunk: the layout [batch][*nchunks][groups][2] of the statistics workspace, chunk k
 * holding the pixels [k, k + 1) * *pix_per_chunk (a one-pass path never touches the workspace); *apply_rows /
 * *apply_blocks: pixels per workgroup and workgroups per sample of the apply pass (0 where none is launched).
 * Nothing is enqueued; sizes the launch refuses are refused with the same code. */
int upk_groupnorm_num_paths(void);
const char* upk_groupnorm_path_name(int path);
int upk_groupnorm_plan(upk_ctx* ctx, int c1, int c2, int batch, int hw, int groups, int with_stats, int with_apply,
                       int* path, int* nchunks, int* pix_per_chunk, int* apply_rows, int* apply_blocks);

/* LayerNorm over the last dim of fp16 [rows, d] (attention.py:203-205, eps 1e-5). */
int upk_layernorm_f16(upk_ctx* ctx, const void* x, int ldx, int rows, int d, const float* gamma,
                      const float* beta, float eps, void* y, int ldy, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Small ops of the loop.                                               */
/* ------------------------------------------------------------------ */
/* timestep_embedding (util.py:151-171): out[i] = [cos(t_i f_j) | sin(t_i f_j)],
 * f_j = exp(-ln(max_period) j / half), written as fp16 [n, ld_out] (cols >= dim zero). */
int upk_timestep_embed_f16(upk_ctx* ctx, const float* t, int n, int dim, float max_period,
                           void* out, int ld_out, upk_stream stream);

/* NCHW fp32 -> NHWC fp16 with channel offset/padding: writes channels
 * [c_off, c_off+c) of y[B, HW, ldy]; if zero_pad_to > c_off+c also zeroes the
 * channels up to zero_pad_to (UNet stem input = cat[x, person_mask], ddpm.py:1568). */
int upk_nchw_f32_to_nhwc_f16(upk_ctx* ctx, const float* x, int batch, int c, int hw, void* y,
                             int ldy, int c_off, int zero_pad_to, float scale,
                             upk_stream stream);
int upk_nhwc_f16_to_nchw_f32(upk_ctx* ctx, const void* x, int ldx, int batch, int c, int hw,
                             float* y, upk_stream stream);
/* fp32 [rows, cols] -> fp16 [rows, ldy] (context tokens). */
int upk_f32_to_f16(upk_ctx* ctx, const float* x, int rows, int cols, void* y, int ldy,
                   upk_stream stream);

/* One DDIM update (ddim.py:189-203), fp32 NCHW, n = B*C*H*W elements:
 *   coef = coefs + 4 * (*step):  {sqrt(1-a_t), 1/sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2)}
 *   pred_x0 = (x - c0*e) * c1 ; x_prev = c2*pred_x0 + c3*e + noise_scaled
 *   noise (may be NULL) = sigma_t * temperature * randn, [n_steps, n] indexed by *step.
 * Also refreshes the UNet stem input: xin (fp16 NHWC [B, HW, ld_xin]) channels
 * [0, C) = x_prev (the concat channels after them are static).  x is updated in place. */
int upk_ddim_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs,
                      const float* noise, const int32_t* step, float* pred_x0, void* xin,
                      int ld_xin, int batch, int c, int hw, upk_stream stream);
/* The same update with classifier-free guidance folded in (ddim.py:173-178): the UNet ran on 2*batch rows,
 * [unconditional ; conditional]; eps2 is [2*batch, C, HW], e = e_u + scale * (e_c - e_u); x / pred_x0 / noise are
 * [batch, ...]; x_prev refreshes BOTH halves of xin (fp16 NHWC [2*batch, HW, ld_xin]). */
int upk_ddim_step_cfg_f32(upk_ctx* ctx, float* x, const float* eps2, const float* coefs,
                          const float* noise, const int32_t* step, float* pred_x0, void* xin,
                          int ld_xin, int batch, int c, int hw, float scale, upk_stream stream);
/* The DDIM update for the editing calls: inpainting (sample(mask=, x0=), ddim.py:144-147) and chains that start inside
 * the schedule (decode, ddim.py:222-241).  x / pred_x0 / noise / coefs / xin as for upk_ddim_step_f32, n = batch*C*HW;
 * cfg != 0: eps holds [uncond ; cond] (2*batch rows), e = e_u + scale * (e_c - e_u), and BOTH halves of xin
 * (2*batch*hw rows) are refreshed; cfg == 0: scale is ignored.
 *   x_prev = the update of upk_ddim_step_f32 at row *step
 *   mask != NULL and *step + 1 < n_rows:  x = mask * keep[*step + 1] + (1 - mask) * x_prev
 *   otherwise:                            x = x_prev
 * The reference blends BEFORE the model evaluation of a step; here that is the tail of the step before, so row r of
 * keep ([n_rows, n] fp32) is q_sample(x0, t) of loop position r (row 0 is never read: the caller blends the first latent),
 * and the last row's result is left unblended, as the reference returns it.  mask: [n], expanded to the latent's shape;
 * mask == NULL (keep and n_rows are then ignored) is the plain update.  x_plain (may be NULL) <- the unblended x_prev,
 * what the reference logs as x_inter; pred_x0, noise, xin, step may be NULL.  xin is refreshed from what went to x. */
int upk_ddim_step_edit_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const float* noise,
                           const float* keep, const float* mask, int n_rows, const int32_t* step, float* pred_x0,
                           float* x_plain, void* xin, int ld_xin, int batch, int c, int hw, float scale, int cfg,
                           upk_stream stream);
/* One DDPM ancestral step (ddpm.py:1125-1187; with a mask also the q_sample blend of ddpm.py:1282-1283), fp32 NCHW,
 * n = B*C*H*W elements; row = coefs + 8 * (*step):
 *   {sqrt(1/a_t), sqrt(1/a_t - 1), posterior_mean_coef1, posterior_mean_coef2,
 *    nonzero(t) * exp(0.5 * posterior_log_variance_clipped), sqrt(a_t), sqrt(1 - a_t), 0}
 *   x_recon = UPK_DDPM_X0 ? model_out : row[0]*x - row[1]*model_out; clamped to [-1, 1] with UPK_DDPM_CLIP
 *   x_prev = row[2]*x_recon + row[3]*x + row[4]*noise
 *   mask != NULL: x_prev = mask*(row[5]*x0 + row[6]*noise2) + (1 - mask)*x_prev   (the SAME t as the step)
 * noise / noise2: [n_steps, n] standard normals (temperature folded in by the caller) indexed by *step, may be NULL;
 * x0, mask: [n] (mask expanded to the latent's shape), may be NULL; pred_x0 (may be NULL) <- x_recon.  Refreshes
 * the UNet stem input xin like upk_ddim_step_f32.  x is updated in place. */
#define UPK_DDPM_X0 0x1
#define UPK_DDPM_CLIP 0x2
int upk_ddpm_step_f32(upk_ctx* ctx, float* x, const float* model_out, const float* coefs,
                      const float* noise, const float* noise2, const float* x0, const float* mask,
                      const int32_t* step, float* pred_x0, void* xin, int ld_xin, int batch, int c, int hw,
                      int flags, upk_stream stream);
/* One model evaluation of the PLMS sampler (ldm/models/diffusion/plms.py:177-236; eta = 0), *step = evaluation
 * counter k (S + 1 evaluations for S steps: the first step evaluates twice, pseudo improved Euler):
 *   k = 0: predictor x~ = ddim(x, e0, coef[0]) goes to xin only; k = 1: e' = (e0 + eps)/2, x <- ddim(x, e', coef[0]);
 *   k >= 2: e' = Adams-Bashforth of order min(k-1, 3)+1 over eps and the history; x <- ddim(x, e', coef[k-1]).
 * hist: fp32 [3, n] eps history ring (owned by the caller, no initialisation needed); coefs as for upk_ddim_step_f32
 * (one row per DDIM index); cfg != 0: eps holds [uncond ; cond] (2*batch) and e = e_u + cfg_scale*(e_c - e_u),
 * xin has 2*batch*hw rows. */
int upk_plms_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const int32_t* step,
                      float* hist, float* pred_x0, void* xin, int ld_xin, int batch, int c, int hw,
                      float cfg_scale, int cfg, upk_stream stream);
/* One step of DPM-Solver++(2M) (Lu et al. 2022, algorithm 2: second-order multistep on the data prediction, eta = 0), fp32
 * NCHW, n = B*C*H*W elements; row = coefs + 8 * (*step) for the step t -> p, lambda = log(alpha / sigma), h = lambda_p - lambda_t:
 *   {sigma_t, 1/alpha_t, sigma_p/sigma_t, -alpha_p * expm1(-h), w, 0, 0, 0},  w = h / (2 h_prev) on a second-order row, 0 on a
 *   first-order one (upgpt_amd/schedule.py dpm_coefficient_table)
 *   e = eps, or with cfg != 0 e_u + cfg_scale * (e_c - e_u) from eps = [uncond ; cond] (2*batch rows)
 *   p0 = (x - row[0]*e) * row[1];  second = row[4] != 0 && *step != first_row
 *   D = second ? p0 + row[4] * (p0 - x0_old) : p0;  x = row[2]*x + row[3]*D;  x0_old = p0;  pred_x0 = p0 (may be NULL)
 * x0_old: fp32 [n], the data prediction of the step before, owned by the caller.  It is READ ONLY when `second` holds — a
 * first-order row (row 0, the chain's first row first_row, a lower-order final row) never touches what it held, so it needs
 * no initialisation — and always written.  A first-order row is the DDIM eta = 0 update.  step == NULL: row 0.
 * Refreshes the UNet stem input xin like upk_ddim_step_f32 (with cfg both halves, 2*batch*hw rows); x is updated in
 * place; honours upk_step_autoadvance. */
int upk_dpmpp_2m_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const int32_t* step,
                          float* x0_old, float* pred_x0, void* xin, int ld_xin, int batch, int c, int hw,
                          int first_row, float cfg_scale, int cfg, upk_stream stream);
/* One model evaluation of UniPC (Zhao et al. 2023, arXiv:2302.04867: multistep predictor-corrector on the data prediction,
 * orders 1 - 3, eta = 0), fp32 NCHW, n = B*C*H*W elements.  Points are numbered k = 0 .. S along the chain (lambda =
 * log(alpha / sigma) ascends); evaluation k = *step sees the predicted latent x at point k, forms m_k, corrects the step
 * k-1 -> k with it and predicts the step k -> k+1 from the corrected latent.  row = coefs + 12 * (*step), h_c = lambda_k -
 * lambda_{k-1}, h_p = lambda_{k+1} - lambda_k (upgpt_amd/schedule.py unipc_coefficient_table):
 *   {sigma_k, 1/alpha_k,
 *    sigma_k/sigma_{k-1}, -alpha_k expm1(-h_c), weights of (m_k - m_{k-1}), (m_{k-2} - m_{k-1}), (m_{k-3} - m_{k-1}),
 *    sigma_{k+1}/sigma_k, -alpha_{k+1} expm1(-h_p), weights of (m_{k-1} - m_k), (m_{k-2} - m_k),
 *    1 if the corrector runs else 0}
 *   e  = eps, or with cfg != 0 e_u + cfg_scale * (e_c - e_u) from eps = [uncond ; cond] (2*batch rows)
 *   m  = (x - row[0]*e) * row[1]
 *   xc = row[11] != 0 ? row[2]*x_corr + row[3]*h0 + row[4]*(m - h0) [+ row[5]*(h1 - h0)] [+ row[6]*(h2 - h0)] : x
 *   xn = row[7]*xc + row[8]*m [+ row[9]*(h0 - m)] [+ row[10]*(h1 - m)]
 *   x_corr = xc;  x = xn;  pred_x0 = m (may be NULL)
 * hist: fp32 [3, n] ring owned by the caller; h0, h1, h2 = m of evaluations *step - 1, - 2, - 3 in slots (*step - j) mod 3,
 * and m goes to slot *step mod 3 (h2's, read before it is written).  x_corr: fp32 [n], the last corrected latent.  A
 * bracketed term runs only where its weight is non-zero, and neither it nor a corrector with row[11] = 0 loads its
 * operands: hist and x_corr need no initialisation, the rows of a chain say what exists.  step == NULL: row 0.
 * Refreshes the UNet stem input xin like upk_ddim_step_f32 (with cfg both halves, 2*batch*hw rows); x is updated in
 * place; honours upk_step_autoadvance.  UPK_EINVAL for a missing operand, a non-positive extent, ld_xin < c with xin,
 * or a pointer that is not aligned to its element. */
int upk_unipc_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const int32_t* step, float* hist,
                       float* x_corr, float* pred_x0, void* xin, int ld_xin, int batch, int c, int hw, float cfg_scale,
                       int cfg, upk_stream stream);
/* One step of SDE-DPM-Solver++(2M) (Lu et al. 2022: the stochastic form of the 2M update on the data prediction; eta = 0 is
 * upk_dpmpp_2m_step_f32's update term by term, eta = 1 the sde-dpmsolver++ midpoint form), fp32 NCHW, n = B*C*H*W elements;
 * row = coefs + 8 * (*step) for the step s -> t, lambda = log(alpha / sigma), h = lambda_t - lambda_s:
 *   {sigma_s, 1/alpha_s, (sigma_t/sigma_s) exp(-eta h), -alpha_t expm1(-(1 + eta) h), w, sigma_t sqrt(-expm1(-2 eta h)), 0, 0}
 *   w = h / (2 h_prev) on a second-order row, 0 on a first-order one; row[5] is the row's noise scale, which only the host
 *   reads (upgpt_amd/schedule.py dpm_sde_coefficient_table).  The rows describe themselves: there is no first_row.
 *   e  = eps, or with cfg != 0 e_u + cfg_scale * (e_c - e_u) from eps = [uncond ; cond] (2*batch rows)
 *   m  = (x - row[0]*e) * row[1]
 *   d  = row[4] != 0 ? m + row[4] * (m - m_old) : m
 *   xn = row[2]*x + row[3]*d [+ noise[*step * n + i]]
 *   x_plain = xn (may be NULL)
 *   mask != NULL and *step + 1 < n_rows:  xn = mask * keep[(*step + 1) * n + i] + (1 - mask) * xn
 *   x = xn;  m_old = m;  pred_x0 = m (may be NULL)
 * noise: [rows, n] fp32 indexed by *step, ALREADY scaled by row[5] * temperature, or NULL (eta = 0).  keep / mask / n_rows /
 * x_plain: as for upk_ddim_step_edit_f32 — the blend in front of the NEXT evaluation, the last row's result unblended; mask
 * == NULL ignores keep and n_rows.  m_old: fp32 [n], the data prediction of the step before, owned by the caller; READ ONLY
 * where row[4] != 0 (it needs no initialisation: a chain's first row is first-order) and always written.  step == NULL:
 * row 0.  Refreshes the UNet stem input xin from what went to x (with cfg both halves, 2*batch*hw rows); honours
 * upk_step_autoadvance.  UPK_EINVAL for a missing operand (x, eps, coefs, m_old), a mask without keep rows, a non-positive
 * extent, ld_xin < c with xin, or a pointer that is not aligned to its element. */
int upk_dpmpp_2m_sde_step_f32(upk_ctx* ctx, float* x, const float* eps, const float* coefs, const float* noise,
                              const float* keep, const float* mask, int n_rows, const int32_t* step, float* m_old,
                              float* pred_x0, float* x_plain, void* xin, int ld_xin, int batch, int c, int hw,
                              float cfg_scale, int cfg, upk_stream stream);
/* With done != NULL the sampler step kernels launched afterwards (upk_ddim_step_f32, upk_ddim_step_cfg_f32,
 * upk_ddim_step_edit_f32, upk_plms_step_f32, upk_ddpm_step_f32, upk_dpmpp_2m_step_f32, upk_unipc_step_f32,
 * upk_dpmpp_2m_sde_step_f32) add 1 to *step THEMSELVES once every workgroup has read it (done: a zero-initialised device
 * int32 they use as arrival counter and leave at zero) — one launch less per sampler step than upk_advance_step.
 * done == NULL restores the plain behaviour.  Host-side state of the context: set it around the calls. */
int upk_step_autoadvance(upk_ctx* ctx, int32_t* done);

/* Number of GPU kernels enqueued through this context since creation / the last reset (a split-K conv is two, a
 * GroupNorm with its own statistics pass is two): what bench.py reports as kernels per UNet forward. */
long long upk_kernel_launches(upk_ctx* ctx, int reset);

/* *step += 1 (end of a captured step graph). */
int upk_advance_step(upk_ctx* ctx, int32_t* step, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Image finishing: fp32 images -> uint8 HWC pictures (test_step).       */
/* ------------------------------------------------------------------ */
/* What LatentDiffusion.test_step does to every image before it is saved (ddpm.py:1352-1357 for the samples, the
 * reconstruction and the batch's images, ddpm.py:1371-1376 for the style crops; T.CenterCrop, torch.clamp, the
 * rescale, T.Normalize, torch.cat along the width and T.ToPILImage's pic.mul(255).byte()), one launch per component:
 * a window of `batch` fp32 3-channel source images is converted and written into a window of a uint8 HWC destination.
 *   src      [batch] images of src_h x src_w, UPK_LAYOUT_NCHW (3 planes) or UPK_LAYOUT_NHWC (3 interleaved floats),
 *            src_batch_stride floats apart (>= 3 * src_h * src_w; ignored for batch == 1); 4-byte aligned
 *   window   rows [top, top + crop_h), columns [left, left + crop_w) of every source image (the centre-crop offsets
 *            are the caller's: upgpt_amd/evaluate.py center_crop_window)
 *   dst      byte (c) of pixel (y, x) of sample b goes to dst[b * dst_sample_stride + y * dst_pitch + 3 * (dst_x + x) + c]
 *            (dst_pitch, dst_sample_stride in bytes, dst_x in pixels): launches with different dst_x lay components
 *            side by side in one strip, no concatenation pass.  Bytes outside the window are not touched.
 *   mode     the value t in front of the quantisation, per element v of channel c, every operation ONE correctly
 *            rounded IEEE fp32 operation in exactly this order (no FMA contraction, no reassociation):
 *              UPK_FINISH_SAMPLE  t = (min(max(v, -1), 1) + 1) / 2        log["samples"], log["reconstruction"]
 *              UPK_FINISH_INPUT   t = (v + 1) / 2                         batch["image" / "src_image" / "smpl_image"]
 *              UPK_FINISH_DENORM  t = (v / d[c]) - m[c]                   batch["styles"] crops (CLIP-normalised)
 *            denorm_host: HOST array {d[0], d[1], d[2], m[0], m[1], m[2]}, read before the call returns (DENORM only,
 *            else may be NULL); the reference's values are d = float32(1 / 0.226862954, 1 / 0.26130258,
 *            1 / 0.27577711) (quotients formed in double, then rounded, as T.Normalize does with its std list) and
 *            m = float32(-0.48145466, -0.4578275, -0.40821073).
 *   byte     u = (uint8) trunc(t * 255), saturated to [0, 255], NaN -> 0.
 * For inputs in the documented ranges ([-1, 1] for INPUT, CLIP-normalised [0, 1] images for DENORM, anything for
 * SAMPLE) these are bit for bit the bytes of the reference's torch expression followed by ToPILImage.  Outside them
 * t * 255 leaves [0, 256) and the reference's .byte() is undefined behaviour (it wraps on some hosts); this entry
 * point SATURATES instead.
 * Errors (UPK_EINVAL): null src / dst, src not 4-byte aligned, unknown layout / mode, non-positive sizes, a window
 * outside the source, (dst_x + crop_w) * 3 > dst_pitch, overlapping samples (a stride smaller than one sample's
 * extent), DENORM without denorm_host or with d = 0 / non-finite values.  Sources, offsets and strides that are
 * multiples of 4 pixels (16-byte aligned src, 4-byte aligned dst) take 16-byte loads and dword stores; everything else
 * is handled per pixel with the same results.  Never allocates, never synchronises, graph-capturable. */
#define UPK_LAYOUT_NCHW 0
#define UPK_LAYOUT_NHWC 1
#define UPK_FINISH_SAMPLE 0
#define UPK_FINISH_INPUT 1
#define UPK_FINISH_DENORM 2
int upk_image_finish_u8(upk_ctx* ctx, const float* src, int layout, int batch, int src_h, int src_w,
                        long long src_batch_stride, int top, int left, int crop_h, int crop_w, uint8_t* dst,
                        long long dst_pitch, int dst_x, long long dst_sample_stride, int mode,
                        const float* denorm_host, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Low-resolution conditioning: uint8 pictures -> `lr` (upscale stage).   */
/* ------------------------------------------------------------------ */
/* What the reference does to a generated picture before the upscale model sees it (app.py:93-97 with p = 4,
 * deepfashion_inshop.py:427-431 with p = 8): T.Pad((p, 0), padding_mode='edge'), T.Resize(size, BILINEAR) on the PIL
 * picture, T.ToTensor(), x * 2. - 1., in ONE launch.  T.Resize on a PIL picture is Pillow's two-pass resampling in
 * 22-bit fixed point, integer arithmetic, so the bytes are reproducible bit for bit.
 *   src      byte (c) of pixel (y, x) of sample b at src[b * src_sample_stride + y * src_pitch + 3 x + c] (strides in
 *            bytes, any value, no alignment: a window of a strip is read in place; the sample stride is ignored for
 *            batch == 1)
 *   pad      edge replication of pad_x columns left and right and pad_y rows above and below: padded column x reads
 *            source column min(max(x - pad_x, 0), src_w - 1), rows likewise.  Not a pass; the tables are built for the
 *            padded sizes in_w = src_w + 2 pad_x, in_h = src_h + 2 pad_y.
 *   tables   DEVICE int32, per axis: bounds [out][2] = (first tap xmin, taps n), k [out][ksize], built by the caller in
 *            double (upgpt_amd/prepare.py resample_coeffs): scale = in / out, fs = max(scale, 1), support = fs; for
 *            output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center +
 *            support + 0.5), in), n = xmax - xmin, w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fs|), divided by
 *            their sum, k[x] = (int)(w[x] * 2^22 + 0.5).  NULL for both pointers of an axis = that pass is skipped
 *            (only when in == out; the bytes go through unchanged).  The kernel relies on xmin >= 0, n >= 1 and
 *            xmin + n <= padded size (n above ksize is cut to ksize); the caller validates before the upload.
 *   pass     acc = 2^21 + sum_x pix[xmin + x] * k[x], out = min(max(acc >> 22, 0), 255); acc < 2^31 because
 *            sum k <= 2^22 + n.  The HORIZONTAL pass runs first and is ROUNDED TO uint8; the vertical pass runs on
 *            those bytes.
 *   dst_u8   may be NULL: byte (c) of pixel (y, x) of sample b at dst_u8[b * dst_sample_stride + y * dst_pitch + 3 x + c]
 *   dst_nchw, dst_nhwc   may be NULL: fp32 dense [batch, 3, out_h, out_w] / [batch, out_h, out_w, 3] of
 *            t = fl(fl(u / 255) * 2 - 1): one correctly rounded fp32 division, an exact doubling, one correctly rounded
 *            subtraction (the `lr` and `lr_image` entries of the reference's datasets)
 * A workgroup produces a band of output rows: the horizontal pass of the padded input rows the band's taps cover goes to
 * LDS as bytes, then a barrier, then the vertical pass from LDS.  The band height (8 rows at most) is chosen so that
 * the staged rows of 3 out_w bytes fit 64 KiB; a shape for which the yksize rows of ONE output row do not fit returns
 * UPK_ESHAPE (so does batch > 65535), it is never approximated.  out_w a multiple of 4 with 4-byte aligned dst_u8 /
 * pitch / sample stride and 16-byte aligned fp32 destinations takes dword / 16-byte stores; everything else is handled
 * per pixel with the same results.
 * Errors (UPK_EINVAL): null src, no destination at all, non-positive sizes, negative pads, a missing table pointer on an
 * axis with in != out (or one of the two given without the other), ksize < 1 on an axis with tables, tables or fp32
 * destinations not 4-byte aligned, dst_pitch < 3 out_w, overlapping destination samples.  Nothing is launched on an
 * error.  One launch, class "other".  Never allocates, never synchronises, graph-capturable. */
int upk_resize_bilinear_u8(upk_ctx* ctx, const uint8_t* src, int batch, int src_h, int src_w, long long src_pitch,
                           long long src_sample_stride, int pad_x, int pad_y, int out_h, int out_w,
                           const int32_t* xbounds, const int32_t* xk, int xksize, const int32_t* ybounds,
                           const int32_t* yk, int yksize, uint8_t* dst_u8, long long dst_pitch,
                           long long dst_sample_stride, float* dst_nchw, float* dst_nhwc, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Style crops: picture + human-parsing label map -> batch['styles'].    */
/* ------------------------------------------------------------------ */
/* The reference's Segmenter.forward (segm_utils.py:42-150) followed by the consumer's clip_transform
 * (deepfashion_inshop.py:128-133), in TWO launches with no device-to-host copy between them: the cut of every group is
 * found on the device and read from device memory by the second launch, so the pair is graph-capturable and a replay
 * on new label maps gives the new crops.
 *   pictures  uint8, byte (c) of pixel (y, x) of sample b at pictures[b * pic_sample_stride + y * pic_pitch + 3 x + c]
 *   segm      uint8 label maps, label of pixel (y, x) at segm[b * segm_sample_stride + y * segm_pitch + x]
 *             (strides in bytes, no alignment; pic_pitch >= 3 w, segm_pitch >= w; sample strides are ignored for
 *             batch == 1)
 *   label_groups_host   HOST uint32 [256], read during the call and handed to the kernel by value: bit g of entry l
 *             is set when label l belongs to group g (a label may belong to several groups); n_groups <= 32
 *
 * upk_segm_boxes_u8: boxes[b][g][8] (DEVICE int32) = left, right, top, bottom, N, S_r, S_g, S_b of mask = (label in
 * group g).  left / top are the first column / row holding a mask pixel, right / bottom the INDEX OF THE LAST one
 * (the reference's get_mask_range with margin 0; used below as exclusive ends, so the last masked column and row are
 * cut off, as in the reference).  N is the number of mask pixels and S_c the integer sum of channel c over them.  With
 * no mask pixel the record is 0, w, 0, h, 0, 0, 0, 0.  Integers only: the result does not depend on reduction order.
 *
 * upk_style_crops_u8: one crop of 224 x 224 per (sample, slot).
 *   slot_groups_host    HOST int32 [n_slots] (n_slots <= 32): the group a slot shows, -1 for an empty slot
 *   group_flags_host    HOST int32 [n_groups]: UPK_STYLE_FILL | UPK_STYLE_MASK | max_rows << 8
 *   mean_std_host       HOST float [6] = mean[3], std[3] of the normalisation (std > 0)
 *   per crop, from the group's record:
 *     UPK_STYLE_FILL (the reference's `background`): no cut and no pad; the content is the whole picture with every
 *       pixel outside the mask replaced, per channel, by floor(S_c / N).  Invalid when N == 0.
 *     otherwise: the content is the picture, with pixels outside the mask zeroed when UPK_STYLE_MASK is set (every
 *       group but `face`), cut to rows [top, bottom) and columns [left, right): ch x cw.  Invalid when ch <= 0 or
 *       cw <= 0, or when max_rows > 0 and ch > max_rows (`face`: 128).  p = floor((ch - cw) / 2): p > 0 adds p zero
 *       columns left and right, p < 0 adds -p zero rows above and below (ch - cw = -3 pads 2 and 2).
 *     T.Resize(224) of the padded ph x pw content: the short side becomes 224, the long one 224 * long / short (integer
 *       division; equal to Python's int(224 * long / short) for these sizes); nothing changes when short == 224.  The
 *       resize is upk_resize_bilinear_u8's: Pillow's tables, the horizontal pass first and rounded to uint8.  The
 *       tables of the produced rows and columns are built IN THE KERNEL in double, operation for operation as stated
 *       above for the caller of upk_resize_bilinear_u8, without contraction.
 *     T.CenterCrop(224): offset int(round((n - 224) / 2.0)) with round-half-to-even (227 -> 2, 225 -> 0).  Only the
 *       central 224 rows / columns are computed.
 *   dst_u8    may be NULL: dense uint8 [batch, n_slots, 224, 224, 3], the crop's bytes
 *   dst_f32   may be NULL: dense fp32 [batch, n_slots, 3, 224, 224] of t = fl(fl(fl(u / 255) - mean_c) / std_c),
 *             three correctly rounded fp32 operations (T.ToTensor, T.Normalize)
 *   valid     DEVICE int32 [batch, n_slots]: 1 for a crop made as above, 0 for an empty slot or an invalid crop; those
 *             get bytes 0 and t(0).  Validity is geometric: a valid cut that is black everywhere stays valid with the
 *             zero bytes the reference returns for it.
 *   coeff_out may be NULL: DEVICE int32 [batch, n_slots, 2, 224, 18], axis 0 = rows, 1 = columns, per produced index
 *             (first tap, taps, k[16]) as the kernel used them (a skipped pass is the single tap (index, 1, 2^22));
 *             zeros for an empty slot or an invalid crop.  For tests: it tells a wrong table from a wrong pass.
 * Two deliberate differences from the reference's file flow: the crop's bytes are handed on as they are (the reference
 * stores every crop as a JPEG and decodes it again), and the fill colour is the exact floor(S_c / N) where the reference
 * truncates a float32 mean of u / 255 values times 255 (equal except where rounding noise decides, e.g. a mean that is
 * an exact integer).
 * A workgroup makes 8 output rows of one crop: coefficients, then the horizontal pass of the input rows its taps cover
 * into LDS as bytes, a barrier, and the vertical pass from LDS.  Sides up to 1344 (scale <= 6: at most 14 taps and 56
 * staged rows of 672 bytes) are supported; a larger picture returns UPK_ESHAPE (so does batch > 65535).
 * Errors (UPK_EINVAL): a null pointer where none is allowed, no destination at all, non-positive sizes, n_groups
 * outside 1 .. 32, n_slots outside 1 .. 32, a slot naming a group outside -1 .. n_groups - 1, negative flags, std <= 0,
 * pic_pitch < 3 w, segm_pitch < w, boxes / valid / coeff_out / dst_f32 not 4-byte aligned.  Nothing is launched on an
 * error.  One launch each, class "other".  Never allocate, never synchronise, graph-capturable. */
#define UPK_STYLE_FILL 0x1
#define UPK_STYLE_MASK 0x2
#define UPK_STYLE_MAX_GROUPS 32
#define UPK_STYLE_MAX_SLOTS 32
int upk_segm_boxes_u8(upk_ctx* ctx, const uint8_t* segm, long long segm_pitch, long long segm_sample_stride,
                      const uint8_t* pictures, long long pic_pitch, long long pic_sample_stride, int batch, int h, int w,
                      const uint32_t* label_groups_host, int n_groups, int32_t* boxes, upk_stream stream);
int upk_style_crops_u8(upk_ctx* ctx, const uint8_t* pictures, long long pic_pitch, long long pic_sample_stride,
                       const uint8_t* segm, long long segm_pitch, long long segm_sample_stride, int batch, int h, int w,
                       const uint32_t* label_groups_host, int n_groups, const int32_t* boxes,
                       const int32_t* group_flags_host, const int32_t* slot_groups_host, int n_slots,
                       const float* mean_std_host, uint8_t* dst_u8, float* dst_f32, int32_t* valid, int32_t* coeff_out,
                       upk_stream stream);

/* ------------------------------------------------------------------ */
/* Region-locked editing: label map -> edit mask, pixel-space composite. */
/* ------------------------------------------------------------------ */
/* The two per-pixel passes around a masked sampling chain: which pixels may change, as a picture-
 * resolution mask and as the latent-resolution keep-mask the samplers take, and the blend of the generated picture into
 * the original ON THE BYTES, so that everything outside the feathered region is the input, byte for byte.  Integers
 * only: no result depends on an order of evaluation.
 *   strides   in bytes, any value with pitch >= the bytes of a row, no alignment; sample strides are ignored for
 *             batch == 1
 *
 * upk_region_mask_u8
 *   segm      uint8 label maps, label of pixel (y, x) of sample b at segm[b * segm_sample_stride + y * segm_pitch + x]
 *   label_sel_host   HOST uint32 [8], a 256-bit set read during the call and handed to the kernel by value: bit l % 32 of
 *             word l / 32 is set when label l is selected
 *   sel(y, x) = 1 when the label of the pixel is selected.  M(y, x) = 1 when some sel(y', x') = 1 with |y - y'| <= dilate
 *             and |x - x'| <= dilate (a Chebyshev window; pixels outside the picture count as unselected).
 *   mask_u8   may be NULL: byte (y, x) of sample b at mask_u8[b * mask_sample_stride + y * mask_pitch + x] = 255 where M,
 *             else 0.  Bytes of a row beyond w are not touched.
 *   keep      may be NULL: DEVICE fp32 dense [batch, 1, h / factor, w / factor]: exactly 0.0f when any pixel of the cell's
 *             factor x factor block has M = 1, else exactly 1.0f (the samplers' convention: 1 keeps x0)
 *   cells     may be NULL: DEVICE int32 [batch], the number of cells with keep = 0.  WRITTEN, not accumulated: the caller
 *             does not zero it.  (Counted by one extra workgroup per sample from the bit rows of the whole map; it exists
 *             only when cells is given.)
 * Errors (UPK_EINVAL): null segm or label_sel_host, no output at all, non-positive sizes, dilate outside 0 .. 32, factor not
 * one of 1, 2, 4, 8, 16, h % factor or w % factor not 0, segm_pitch < w, mask_pitch < w (with a mask), keep or cells not
 * 4-byte aligned, overlapping mask samples (a sample stride below one sample's extent), a mask that overlaps the label
 * maps.
 *
 * upk_composite_u8
 *   orig, gen   uint8 pictures, byte (c) of pixel (y, x) of sample b at p[b * ss + y * pitch + 3 x + c]
 *   mask_u8     uint8 [h][w] per sample (pitch, ss): m(y, x) = (byte != 0)
 *   n = (2 feather + 1)^2;  s(y, x) = the sum of m over the (2 feather + 1)^2 window with CLAMPED coordinates (edge
 *             replication);  A = (255 s + n / 2) / n, integer division, 0 .. 255
 *   out       out_c = (A gen_c + (255 - A) orig_c + 127) / 255, integer division, per channel: A = 0 gives the original
 *             byte exactly, A = 255 the generated byte exactly.  Layout as orig / gen.
 *   alpha_out may be NULL: uint8 [h][w] per sample (alpha_pitch, alpha_ss), receives A
 * Errors (UPK_EINVAL): null orig, gen, mask_u8 or out, non-positive sizes, feather outside 0 .. 16, a picture pitch below
 * 3 w, a mask / alpha pitch below w, out or alpha_out overlapping an input or each other, overlapping output samples.
 * orig, gen, out (and alpha_out) with 4-byte aligned pointers, pitches and sample strides take dword loads and stores
 * (12 bytes = 4 pixels); everything else, and the last w % 4 pixels of a row, go per pixel with the same results.
 *
 * Both work on bit rows: a wave turns 64 adjacent bytes of a row into one 64-bit word in LDS with one ballot (a label map
 * or mask whose width, address, pitch and sample stride are multiples of 16 is read by 16-byte loads instead, a lane ORs
 * its 16 bits into the word; same results), a window is then a few word operations (OR for the dilation, popcount for
 * the box sum).  A workgroup owns a band of 16 rows of one
 * picture: the bit rows its window covers, a barrier, the vertical pass, the band's bytes and cells (16 is a multiple of
 * every factor: a cell never straddles two workgroups).  UPK_ESHAPE: a size whose bit rows do not fit 64 KiB of LDS
 * (region_mask: (48 + 2 dilate) ceil(w / 64) 8 bytes, and with cells (h + h / factor) ceil(w / 64) 8 bytes; composite:
 * (16 + 2 feather) (ceil(w / 64) 8 + w rounded up to 4) bytes), or batch > 65535; never approximated.  Every picture up
 * to 512 x 384 fits at dilate 32 / feather 16.  Nothing is launched on an error.  One launch each, class "other".  Never
 * allocate, never synchronise, graph-capturable. */
int upk_region_mask_u8(upk_ctx* ctx, const uint8_t* segm, long long segm_pitch, long long segm_sample_stride, int batch,
                       int h, int w, const uint32_t* label_sel_host, int dilate, int factor, uint8_t* mask_u8,
                       long long mask_pitch, long long mask_sample_stride, float* keep, int32_t* cells, upk_stream stream);
int upk_composite_u8(upk_ctx* ctx, const uint8_t* orig, long long orig_pitch, long long orig_ss, const uint8_t* gen,
                     long long gen_pitch, long long gen_ss, const uint8_t* mask_u8, long long mask_pitch, long long mask_ss,
                     int batch, int h, int w, int feather, uint8_t* out, long long out_pitch, long long out_ss,
                     uint8_t* alpha_out, long long alpha_pitch, long long alpha_ss, upk_stream stream);

/* ------------------------------------------------------------------ */
/* The test split's loader: conditioning maps and stored style crops.    */
/* ------------------------------------------------------------------ */
/* The per-pixel work of DeepFashionPair.__getitem__ (deepfashion_inshop.py:173-272) on the bytes PIL decoded.  Every
 * fp32 result is one correctly rounded IEEE operation at a time in the reference's order: no FMA contraction, no
 * reciprocal multiply in place of a division.
 *   src       uint8 maps, byte of pixel (y, x) of sample b at src[b * sample_stride + y * pitch + x] (for the two
 *             entry points that read pictures: 3 interleaved bytes per pixel, + 3 x + c).  Strides in bytes, any value
 *             with pitch >= the bytes of a row, no alignment; the sample stride is ignored for batch == 1.
 *   ytab, xtab   DEVICE int32 [out_h], [out_w]: the source row / column Pillow's NEAREST resize reads for an output row /
 *             column, built by the caller in double as ImagingScaleAffine does (a = in / out, xo = a * 0.5, per output:
 *             idx = (int)xo, xo += a; NOT floor((i + 0.5) in / out), which differs at 256 -> 24).  The caller validates
 *             0 <= idx < in before the upload; upk_cond_gather_u8 clamps an index on the read regardless.
 *   dst       fp32 dense [batch, 1, out_h, out_w]
 *
 * upk_cond_bbox_u8 (input_mask_type 'bbox': get_bbox, then mask_transform): r0 / r1 = the first / last row of a map
 * holding a non-zero byte, c0 / c1 likewise for columns; boxes[b][4] (DEVICE int32) = r0, r1, c0, c1, or -1, -1, -1, -1
 * for a map without a non-zero byte.  dst[b][0][y][x] = t(1) when r0 <= ytab[y] <= r1 and c0 <= xtab[x] <= c1, else t(0),
 * t(u) = fl(fl(u / 255) * 2 - 1): the reference's kept bug of 1 / 255, -0.99215686 inside and -1 outside.  One workgroup
 * per map: the reduction runs in LDS (integer minima and maxima), then a barrier, then the map's outputs; one launch, no
 * workspace.  w, pitch, sample stride and src multiples of 16 take 16-byte loads; everything else is read bytewise.
 *
 * upk_cond_gather_u8 (input_mask_type 'mask' and loss_w): dst[b][0][y][x] = lut[src[b][ytab[y]][xtab[x]]].
 *   lut_host  HOST float [256], read during the call and handed to the kernel by value ('mask': lut[u] = t(u); loss_w:
 *             lut[label] = weight)
 *
 * upk_cond_smpl_u8 (input_mask_type 'smpl', after upk_resize_bilinear_u8 made the [h, w] bytes): pictures uint8 HWC ->
 * dst[b][0][y][x] = fl(fl(fl(fl(r + g) + b) / 3) * 2 - 1) with r, g, b = fl(u / 255): torch.mean(x, 0) * 2. - 1.
 *
 * upk_clip_normalize_u8 (clip_transform, deepfashion_inshop.py:128-133, 208-216): n crops uint8 [h][w][3] ->
 * dst fp32 dense [n, 3, h, w] of fl(fl(fl(u / 255) - mean_c) / std_c), the output stage of upk_style_crops_u8.
 *   valid     may be NULL: DEVICE int32 [n]; a crop with valid 0 gets the values of u = 0 and its bytes are NOT read (a
 *             missing style file, the reference's clip_norm(zeros))
 *   mean_std_host   HOST float [6] = mean[3], std[3] (std > 0)
 * A workgroup makes 8 rows of one crop.  With w a multiple of 16, 24 w <= 65536 and src, pitch, sample stride and dst
 * multiples of 16 the rows are staged in LDS by 16-byte loads and every lane writes one 16-byte float4 per plane;
 * everything else goes per pixel with the same results.
 * Errors (UPK_EINVAL): a null pointer where none is allowed, non-positive sizes, a pitch below the bytes of a row, std <=
 * 0, tables / boxes / valid / dst not 4-byte aligned; UPK_ESHAPE: batch (n) > 65535, a map of 2^31 pixels or more.
 * Nothing is launched on an error.  One launch each, class "other".  Never allocate, never synchronise, graph-capturable. */
int upk_cond_bbox_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h, int w,
                     const int32_t* ytab, const int32_t* xtab, int out_h, int out_w, float* dst, int32_t* boxes,
                     upk_stream stream);
int upk_cond_gather_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h, int w,
                       const int32_t* ytab, const int32_t* xtab, int out_h, int out_w, const float* lut_host, float* dst,
                       upk_stream stream);
int upk_cond_smpl_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, int batch, int h, int w,
                     float* dst, upk_stream stream);
int upk_clip_normalize_u8(upk_ctx* ctx, const uint8_t* src, long long pitch, long long sample_stride, const int32_t* valid,
                          int n, int h, int w, const float* mean_std_host, float* dst, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Pose interpolation: the conditioning of a frame sequence.             */
/* ------------------------------------------------------------------ */
/* The "Interpolate" loop of the reference's demo (app.py:280-308 with get_coord / get_mask / interp_mask, app.py:158-183)
 * for all n frames in ONE launch, one workgroup per frame.  DESIGN.md 31.
 *   src_mask, dst_mask   DEVICE fp32 dense [h, w]: the person_mask of the source and of the destination pose
 *   src_smpl, dst_smpl   DEVICE fp32 [d]
 *   alphas     DEVICE double [n]: frame i is alpha_i of the source and 1 - alpha_i of the destination.  Read by the
 *              kernel, so a captured launch follows a rewritten buffer.
 *   mask_out   DEVICE fp32 dense [n, 1, h, w];  smpl_out  DEVICE fp32 dense [n, d]
 *   boxes      may be NULL: DEVICE int32 [n + 2][4] = (r0, r1, c0, c1), inclusive; row 0 the source's box, row 1 the
 *              destination's, row 2 + i frame i's
 * Box of a map: r0 / r1 = the first / last row holding an OCCUPIED element, c0 / c1 likewise for columns; an element is
 * occupied when it is neither -1 nor 0.  PRECONDITION: the reference takes the rows and columns whose fp32 mean is
 * non-zero after -1 was replaced by 0; the two agree for every map whose other entries share one sign ({-1, -0.99215686},
 * {-1, 1}, and those after the reference's in-place zeroing: every mask this project or the demo makes).  numpy's
 * summation order is not emulated, so a map with entries of both signs that cancel in a row's mean is outside the contract.
 * Each workgroup reduces both maps in LDS with integer minima and maxima (no order to depend on), then writes its frame.
 * Arithmetic, one correctly rounded IEEE operation at a time, never a fused multiply-add:
 *   beta = 1.0 - alpha                                                     in fp64
 *   box_i[k] = (int)(fl64(fl64(alpha * src_box[k]) + fl64(beta * dst_box[k])))   truncation toward zero; numpy's
 *              (alpha * c1 + (1 - alpha) * c2).astype(np.int32).  NOT "fixed": alpha = 0.05 on rows 3 and 3 gives 2.
 *   smpl_out[i][j] = fl32(fl32((float)alpha * src_smpl[j]) + fl32((float)beta * dst_smpl[j]))   torch's alpha * x + (1 - alpha) * y
 *              with a float64 scalar alpha and fp32 tensors
 *   mask_out[i][0][y][x] = -0.99215686 (= fl(fl(1 / 255) * 2 - 1)) for r0 <= y <= r1 and c0 <= x <= c1 of box_i, else -1
 * A frame's box is clamped to the map (lower bounds to [0, size], upper bounds to [-1, size - 1]); a box with min > max
 * writes no foreground.  With alpha in [0, 1] the clamp never acts.  When either map has no occupied element its row of
 * `boxes` and every frame's row are -1, -1, -1, -1 and every frame is all background (the reference raises IndexError).
 * Inputs are not modified.  Errors (UPK_EINVAL): a null pointer other than boxes, non-positive sizes, fp32 / int32
 * pointers not 4-byte or alphas not 8-byte aligned, an output that overlaps an input or another output; UPK_ESHAPE:
 * n > 65535, a map of 2^31 elements or more.  Nothing is launched on an error.  One launch, class "other".  Never
 * allocates, never synchronises, graph-capturable. */
int upk_pose_interp_f32(upk_ctx* ctx, const float* src_mask, const float* dst_mask, int h, int w, const float* src_smpl,
                        const float* dst_smpl, int d, const double* alphas, int n, float* mask_out, float* smpl_out,
                        int32_t* boxes, upk_stream stream);

/* ------------------------------------------------------------------ */
/* SSIM / MS-SSIM moments of uint8 picture pairs (evaluation metrics).   */
/* ------------------------------------------------------------------ */
/* The per-image arithmetic of scripts/eval_metrics.py:110-111 (pytorch_msssim.ssim / ms_ssim with data_range=1,
 * size_average=False) up to the per-channel means.  Pictures are uint8 HWC, 3 interleaved bytes per pixel, X = u / 255
 * (T.ToTensor), every channel on its own:
 *   window     g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1; applied separably along H then W,
 *              "valid" (no padding): a level of h x w gives an (h - 10) x (w - 10) map
 *   moments    mu1 = G*X, mu2 = G*Y, s11 = G*(X X) - mu1^2, s22 = G*(Y Y) - mu2^2, s12 = G*(X Y) - mu1 mu2
 *   maps       cs_map = (2 s12 + C2) / (s11 + s22 + C2), ssim_map = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) cs_map,
 *              C1 = 0.01^2, C2 = 0.03^2
 *   means      ssim_c, cs_c = the means of ssim_map, cs_map per (sample, channel)
 *   next level both pictures through avg_pool2d(kernel 2, stride 2, padding = size % 2 per axis, count_include_pad=True):
 *              an odd axis s becomes (s + 1) / 2, output i averages inputs 2 i - 1 and 2 i with index -1 reading zero,
 *              the divisor is always 4 (so a level-l plane is an exact integer sum over 255 * 4^l)
 * out[((n * levels + l) * 3 + c) * 2 + {0, 1}] = {ssim_c, cs_c} of sample n, level l, channel c (fp32).  What is left
 * acts on these 6 * levels numbers per image and is the caller's (upgpt_amd/metrics.py): SSIM = the mean over c of ssim_c
 * at level 0 (no relu); MS-SSIM (levels = 5, needs min(h, w) > 160) = the mean over c of prod_{l<4} relu(cs_c[l])^wt[l] *
 * relu(ssim_c[4])^wt[4], wt = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).
 *   a, b       byte (c) of pixel (y, x) of sample n is at base[n * sample_stride + y * pitch + 3 x + c] (strides in bytes):
 *              a window of a wider strip or of a larger buffer is compared in place
 *   levels     1..5; every level must have both sides >= 11, else UPK_ESHAPE
 *   ws         upk_ssim_ws_bytes(batch, h, w, levels) bytes (0 for arguments upk_ssim_u8 would refuse), 16-byte aligned:
 *              the pooled planes of the deeper levels and one slot of partial sums per workgroup
 * Deterministic: no float atomics, every workgroup writes its own slot and a fixed-order pass sums them, so reruns are
 * bit-identical and a sample's result depends neither on its position in the batch nor on the batch size.
 * Errors: UPK_EINVAL for null pointers, non-positive sizes, levels outside 1..5, pitch < 3 w, overlapping samples
 * (batch > 1 and a sample stride below (h - 1) pitch + 3 w), out not 4-byte or ws not 16-byte aligned; UPK_ESHAPE as
 * above; UPK_EWORKSPACE for ws_bytes below upk_ssim_ws_bytes.  2 levels launches (levels level kernels, levels - 1
 * pooling kernels, one final pass), all counted in class "other".  Never allocates, never synchronises, graph-capturable. */
size_t upk_ssim_ws_bytes(int batch, int h, int w, int levels);
int upk_ssim_u8(upk_ctx* ctx, const uint8_t* a, long long a_pitch, long long a_sample_stride, const uint8_t* b,
                long long b_pitch, long long b_sample_stride, int batch, int h, int w, int levels, float* out, void* ws,
                size_t ws_bytes, upk_stream stream);

/* ------------------------------------------------------------------ */
/* LPIPS (VGG16) of picture pairs (evaluation metrics).                   */
/* ------------------------------------------------------------------ */
/* scripts/eval_metrics.py:112, lpips.LPIPS(net='vgg')(sample, gt) (lpips 0.1.4, version '0.1', lpips=True, spatial=False,
 * eval mode), for inputs in0, in1 [N, 3, H, W]:
 *   scaling    x' = (x - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale = (.458, .448, .450); with normalize
 *              x is 2 x - 1 first.  eval_metrics.py passes T.ToTensor() output, u / 255, with normalize=False.
 *   features   torchvision VGG16 `features`: 13 convolutions 3x3, stride 1, pad 1, with bias, each followed by a ReLU, in five
 *              slices of 2, 2, 3, 3, 3 convolutions (3->64->64 | ->128->128 | ->256->256->256 | ->512->512->512 | 512 x3);
 *              slices 2..5 start with MaxPool2d(2, 2) (floor: an odd side s becomes (s - 1) / 2, the last row / column is
 *              dropped).  Tap l = the output of the last ReLU of slice l (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3).
 *   distance   per tap and pixel f^ = f / (sqrt(sum_c f_c^2) + 1e-10); d_l = mean over pixels of sum_c w_l[c] (f^0_c - f^1_c)^2
 *              with w_l the 1x1 `lin` weight (no bias; dropout is the identity in eval mode); LPIPS = sum_l d_l.
 *   min(H, W) >= 16, so that the fifth tap has a pixel.
 * The convolutions are upk_conv2d_nhwc_f16 launches as they stand (plain epilogue, bias, fp16 NHWC output; relu(fp16(v)) ==
 * fp16(relu(v)), so a ReLU behind the rounding loses nothing); the three entry points below are what is left.  All of them
 * never allocate, never synchronise, are graph-capturable, and count their launches in class "other".
 *
 * upk_lpips_input_f16: pictures -> y fp16 NHWC [batch, h * w, 32]: channels 0..2 = ((x [* 2 - 1]) - shift[c]) / scale[c],
 * channels 3..31 zero (the first convolution reads 32-channel chunks).
 *   src_f32 == 0  src is uint8 HWC: byte (c) of pixel (y, x) of sample n at src[n * sample_stride + y * pitch + 3 x + c]
 *                 (strides in bytes: a window of a strip is read in place), x = u / 255
 *   src_f32 != 0  src is fp32 NCHW, every sample dense, sample_stride floats apart (pitch is ignored)
 *   shift_scale_host: HOST array {shift[0..2], scale[0..2]}, read before the call returns.
 * Every operation is ONE correctly rounded IEEE fp32 operation in the order written (u / 255; 2 * x, then - 1; - shift;
 * / scale; no FMA contraction), and the result is rounded once to fp16: bit for bit what torch's fp32 expression
 * followed by .half() gives.  sample_stride and y_sample_stride are ignored for batch == 1.
 * Errors: UPK_EINVAL for null pointers, non-positive sizes, y not 16-byte / fp32 src not 4-byte aligned, pitch < 3 w,
 * overlapping samples or outputs, a zero or non-finite scale / non-finite shift; UPK_ESHAPE for more than 2^31 - 1 workgroups. */
int upk_lpips_input_f16(upk_ctx* ctx, const void* src, int src_f32, long long pitch, long long sample_stride, int batch,
                        int h, int w, int normalize, const float* shift_scale_host, void* y, long long y_sample_stride,
                        upk_stream stream);
/* x [batch, h * w, ld] fp16 (c valid channels per row) becomes relu(x) IN PLACE; with pooled != NULL also pooled[batch,
 * (h / 2) * (w / 2), ld_p] = the 2x2 stride-2 floor max-pool of the ReLU'd values (an odd last row / column gets its ReLU
 * and takes no part in the pooling).  16-byte accesses, every input element is read once; channels >= c of a row (the
 * gap of ld > c) are neither read nor written.  Bit-exact by construction (relu(v) = v > 0 ? v : +0).
 * Errors: UPK_EINVAL for null x, non-positive sizes, ld / ld_p below c or not a multiple of 8, pointers not 16-byte
 * aligned; UPK_ESHAPE for c % 8 != 0, pooled with h < 2 or w < 2, more than 2^31 - 1 workgroups. */
int upk_relu_pool_nhwc_f16(upk_ctx* ctx, void* x, int ld, int batch, int h, int w, int c, void* pooled, int ld_p,
                           upk_stream stream);
/* One tap: out[i * 5 + layer] = d_layer of pair i (see above) for i < n, from f0, f1 [n, hw, ld] fp16, the post-ReLU
 * features of the two pictures, pair i at f0 + i * batch_stride and f1 + i * batch_stride elements (>= hw * ld, a multiple of
 * 8; ignored for n == 1: one buffer that holds the pictures interleaved is f1 = f0 + hw * ld with batch_stride = 2 hw ld,
 * two halves of one 2 n batch are f1 = f0 + n * hw * ld with batch_stride = hw ld), c channels, and w [c] fp32.
 * fp32 arithmetic, eps = 1e-10, IEEE divisions and square root (no approximate reciprocals); an all-zero pixel adds
 * exactly 0.  c in {64, 128, 256, 512}: a wave covers 512 channels with one 16-byte load per lane (512 / c pixels side by
 * side), every feature element is read once, the channel sums are shuffles inside the wave.
 * Deterministic like upk_ssim_u8: no float atomics; every workgroup (16384 / c pixels of one pair) writes its own slot
 * of ws and a fixed-order fp64 pass sums a pair's slots and divides by hw: reruns are bit-identical, and a pair's value
 * depends neither on its position in the batch nor on the batch size.  Every term is non-negative, so the result is
 * within relative (c * hw + 16) * 2^-23 of the exact value for the given fp16 features.
 *   ws   upk_lpips_ws_bytes(n, hw, c) bytes (0 for arguments upk_lpips_layer_f16 would refuse), 16-byte aligned
 * Errors: UPK_EINVAL for null pointers, non-positive sizes, layer outside 0..4, ld below c or not a multiple of 8, a batch stride
 * below hw * ld or not a multiple of 8, f0 / f1 / w / ws not 16-byte or out not 4-byte aligned; UPK_ESHAPE for another c or too many workgroups;
 * UPK_EWORKSPACE for ws_bytes below upk_lpips_ws_bytes.  Two launches (partial sums, final pass). */
size_t upk_lpips_ws_bytes(int n, int hw, int c);
int upk_lpips_layer_f16(upk_ctx* ctx, const void* f0, const void* f1, int ld, long long batch_stride, int n, int hw, int c,
                        const float* w, int layer, float* out, void* ws, size_t ws_bytes, upk_stream stream);

/* ------------------------------------------------------------------ */
/* FID features: InceptionV3 of pytorch_fid (evaluation metrics).         */
/* ------------------------------------------------------------------ */
/* scripts/eval_metrics.py:102, `python -m pytorch_fid gt_dir sample_dir` (pytorch_fid 0.3.0, dims = 2048): the [N, 2048]
 * pool3 features of its InceptionV3 (pt_inception-2015-12-05 weights, eval mode) for pictures x [N, 3, H, W] in [0, 1]:
 *   input      F.interpolate(x, size = (299, 299), mode = 'bilinear', align_corners = False), no antialias also when
 *              shrinking: source coordinate s = max(0, (d + 0.5) * in / 299 - 0.5), i0 = floor(s), i1 = min(i0 + 1, in - 1),
 *              weight lambda = s - i0, per axis; then 2 x - 1.
 *   conv unit  BasicConv2d = Conv2d(bias = False) -> BatchNorm2d(eps = 1e-3, eval) -> ReLU.  The BatchNorm is folded when the
 *              weights are packed (fp64, rounded once): w' = w g / sqrt(var + 1e-3) (fp16), b' = beta - mean g / sqrt(var +
 *              1e-3) (fp32).  All paddings 0 unless given; "avg" is avg_pool2d(3, stride 1, pad 1, count_include_pad = False):
 *              the divisor is the number of taps inside the picture.
 *   trunk      Conv2d_1a_3x3 3 -> 32 3x3 s2 (149) | Conv2d_2a_3x3 32 -> 32 3x3 (147) | Conv2d_2b_3x3 32 -> 64 3x3 p1 (147) |
 *              max pool 3x3 s2 (73) | Conv2d_3b_1x1 64 -> 80 1x1 | Conv2d_4a_3x3 80 -> 192 3x3 (71) | max pool 3x3 s2 (35) |
 *              Mixed_5b, 5c, 5d = A(192, 32), A(256, 64), A(288, 64) -> 256, 288, 288 (35) | Mixed_6a = B(288) -> 768 (17) |
 *              Mixed_6b .. 6e = C(768, c7 = 128, 160, 160, 192) -> 768 | Mixed_7a = D(768) -> 1280 (8) | Mixed_7b = E(1280,
 *              avg), Mixed_7c = E(2048, MAX) -> 2048 | mean over the pixels -> [N, 2048]
 *   blocks     (branches concatenated along C in this order)
 *     A(in, pf)  branch1x1 in -> 64 | branch5x5_1 in -> 48 1x1, branch5x5_2 48 -> 64 5x5 p2 | branch3x3dbl_1 in -> 64 1x1, _2
 *                64 -> 96 3x3 p1, _3 96 -> 96 3x3 p1 | avg, branch_pool in -> pf 1x1
 *     B(288)     branch3x3 288 -> 384 3x3 s2 | branch3x3dbl_1 288 -> 64 1x1, _2 64 -> 96 3x3 p1, _3 96 -> 96 3x3 s2 | max pool
 *                3x3 s2 of the input
 *     C(768, c7) branch1x1 -> 192 | branch7x7_1 -> c7 1x1, _2 c7 -> c7 (1,7) p(0,3), _3 c7 -> 192 (7,1) p(3,0) | branch7x7dbl_1
 *                -> c7 1x1, _2 (7,1) p(3,0), _3 (1,7) p(0,3), _4 (7,1) p(3,0) all c7 -> c7, _5 (1,7) p(0,3) c7 -> 192 | avg,
 *                branch_pool -> 192 1x1
 *     D(768)     branch3x3_1 -> 192 1x1, branch3x3_2 192 -> 320 3x3 s2 | branch7x7x3_1 -> 192 1x1, _2 (1,7) p(0,3), _3 (7,1)
 *                p(3,0), _4 3x3 s2, all 192 -> 192 | max pool 3x3 s2 of the input
 *     E(in)      branch1x1 -> 320 | branch3x3_1 -> 384 1x1, then branch3x3_2a (1,3) p(0,1) and branch3x3_2b (3,1) p(1,0), both
 *                384 -> 384 reading _1, concatenated | branch3x3dbl_1 -> 448 1x1, _2 448 -> 384 3x3 p1, then _3a (1,3) p(0,1)
 *                and _3b (3,1) p(1,0) both reading _2, concatenated | pool, branch_pool -> 192 1x1; the pool is avg in
 *                Mixed_7b and max_pool2d(3, stride 1, pad 1) in Mixed_7c
 * All four entry points never allocate, never synchronise and are graph-capturable.  The convolution counts in class
 * "igemm", the three others in class "other".
 *
 * upk_conv2d_rect_f16: y[m, 0 .. n_out) = act(conv(x, w)[m] + bias) for the batch * ho * wo output pixels m of an NHWC fp16
 * input x [batch, in_h * in_w, ldx] (cin_pad valid channels, a multiple of 32, zero-padded), ho = (in_h + 2 pad_h - kh) /
 * stride + 1 and wo likewise; kh, kw in 1 .. 7 independently, stride 1 or 2 (both axes), pad_h, pad_w in 0 .. 3 (zeros).
 *   w_packed  upk_pack_weight_f16 layout [kh * kw * cin_pad / 32][n_pad][32]
 *   bias      fp32 [n_pad] in packed row order, or NULL; relu != 0: max(v, +0) before the fp16 rounding
 *   y, ldy    row m at y + m * ldy, ldy >= n_out: a branch writes its channel slice of a concatenated output in place;
 *             columns >= n_out of a row are never touched
 * MFMA implicit GEMM, fp32 accumulation.  The tile (128 pixels x 64 channels, 32 for n_pad < 64) depends on n_pad alone and
 * K is never split: an output element is one accumulation chain over k = (ky, kx, ci) in ascending order, so its bits do
 * not depend on the batch size or on the picture's place in the batch, and reruns are bit-identical (no atomics).
 * Errors: UPK_ESHAPE for kh / kw / stride / paddings outside the above, cin_pad not a positive multiple of 32, n_pad not a
 * multiple of 16, n_out outside 1 .. n_pad, more than 2^31 - 1 pixels; UPK_EINVAL for null x / w_packed / y, non-positive sizes,
 * ldy < n_out, ldx < cin_pad, ldx % 8, ldy % 4, x / w_packed / bias not 16-byte or y not 8-byte aligned, an output extent that
 * is not positive (in + 2 pad < k). */
int upk_conv2d_rect_f16(upk_ctx* ctx, const void* x, int ldx, int batch, int in_h, int in_w, int cin_pad, int kh, int kw,
                        int stride, int pad_h, int pad_w, const void* w_packed, int n_out, int n_pad, const float* bias,
                        int relu, void* y, int ldy, upk_stream stream);
/* 3x3 pooling of x [batch, h * w, ldx] fp16 (c valid channels, a multiple of 8) into y [batch, ho * wo, ldy]: stride 1 with
 * padding 1 (ho = h, wo = w) or stride 2 without padding (ho = (h - 3) / 2 + 1).  Taps outside the picture take no part:
 * UPK_POOL_MAX is the maximum of the in-picture taps (bit-exact), UPK_POOL_AVG their fp32 sum in (ky, kx) order divided
 * once (IEEE) by their NUMBER (count_include_pad = False), rounded once to fp16.  Channels >= c of a row are neither read
 * nor written.
 * Errors: UPK_EINVAL for null pointers, non-positive sizes, another mode, ldx / ldy below c or not a multiple of 8, pointers
 * not 16-byte aligned; UPK_ESHAPE for another stride, c % 8 != 0, stride 2 with h < 3 or w < 3, too many workgroups. */
#define UPK_POOL_MAX 0
#define UPK_POOL_AVG 1
int upk_pool3_nhwc_f16(upk_ctx* ctx, const void* x, int ldx, int batch, int h, int w, int c, int mode, int stride, void* y,
                       int ldy, upk_stream stream);
/* pictures -> y fp16 NHWC [batch, out_h * out_w, 32]: the bilinear resize above from h x w to out_h x out_w (equal sizes:
 * a copy, lambda = 0), then 2 x - 1 when normalize != 0; channels 3 .. 31 are +0.  Sources as upk_lpips_input_f16 takes them:
 *   src_f32 == 0  uint8 HWC, byte (c) of pixel (y, x) of sample n at src[n * sample_stride + y * pitch + 3 x + c], x = u / 255
 *   src_f32 != 0  fp32 NCHW, every sample dense, sample_stride floats apart (pitch is ignored)
 * Sample n is written at y + n * y_sample_stride elements (>= 32 out_h out_w, a multiple of 8).  The source coordinate and
 * lambda are formed in fp64 and lambda rounded once; the pixel arithmetic is fp32, one IEEE operation at a time, no FMA: v = u /
 * 255; t = (1 - lx) v00 + lx v01 for both rows; (1 - ly) t0 + ly t1; 2 x, - 1; one rounding to fp16.  sample_stride and
 * y_sample_stride are ignored for batch == 1.
 * Errors: UPK_EINVAL for null pointers, non-positive sizes (a zero output size included), y not 16-byte / fp32 src not 4-byte
 * aligned, pitch < 3 w, overlapping samples or outputs; UPK_ESHAPE for more than 2^31 - 1 workgroups. */
int upk_fid_input_f16(upk_ctx* ctx, const void* src, int src_f32, long long pitch, long long sample_stride, int batch, int h,
                      int w, int out_h, int out_w, int normalize, void* y, long long y_sample_stride, upk_stream stream);
/* out[i, ch] = the mean over the hw pixels of x [n, hw, ld] fp16 (c valid channels, a multiple of 8; sample i at x + i * hw *
 * ld), fp32 [n, c] dense: an fp32 sum in pixel order, one IEEE division; reruns are bit-identical and a sample's value does not
 * depend on the batch.  Within (hw + 2) 2^-24 mean|x| of the exact mean.
 * Errors: UPK_EINVAL for null pointers, non-positive sizes, ld below c or not a multiple of 8, x not 16-byte or out not
 * 4-byte aligned; UPK_ESHAPE for c % 8 != 0, too many workgroups. */
int upk_avgpool_global_f32(upk_ctx* ctx, const void* x, int ld, int n, int hw, int c, float* out, upk_stream stream);

/* ------------------------------------------------------------------ */
/* The denoising loss: q_sample and p_losses (validation).                */
/* ------------------------------------------------------------------ */
/* What LatentDiffusion.p_losses (ddpm.py:1083-1123) does around its one UNet forward.  Both entry points never allocate,
 * never synchronise, are graph-capturable, and count their launches in class "other".
 *
 * upk_q_sample_f32: q_sample (ddpm.py:271-274) with one timestep per sample, one launch.
 *   x_start, noise   fp32 NCHW [batch, c, hw], dense
 *   t                int32 [batch]; a, s = sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod: fp32 tables of n_t entries
 *   x_noisy          fp32 NCHW [batch, c, hw], or NULL
 *   xin              the UNet stem input, fp16 NHWC [batch * hw, ld_xin], or NULL: channels [0, c) of every row are written,
 *                    as upk_ddim_step_f32 writes them; channels >= c of a row are left untouched
 * v = fl(fl(a[t_b] * x0) + fl(s[t_b] * n)): three correctly rounded IEEE fp32 operations, no FMA contraction, bit for bit
 * what torch's fp32 expression gives on the CPU; x_noisy = v, xin = v rounded once to fp16 (to nearest even).  A t_b outside
 * [0, n_t) is never used as an index: every output of that sample is NaN, the other samples are as without it.  With x_start,
 * noise and x_noisy 16-byte aligned a thread moves 4 consecutive elements with 16-byte loads and stores (a group may cross
 * a channel or a sample) and the batch * c * hw % 4 last elements go one per thread; otherwise every element goes alone.
 * Errors: UPK_EINVAL for null inputs, x_noisy and xin both NULL, non-positive sizes, ld_xin < c, an fp32 / int32 pointer not
 * 4-byte or xin not 2-byte aligned; UPK_ESHAPE for c * hw above 2^31 - 1 - 8192 or more than 2^31 - 1 workgroups. */
int upk_q_sample_f32(upk_ctx* ctx, const float* x_start, const float* noise, const int32_t* t,
                     const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, int n_t, float* x_noisy,
                     void* xin, int ld_xin, int batch, int c, int hw, upk_stream stream);
/* upk_p_losses_f32: the loss values of ddpm.py:1101-1121 from model_out and target, fp32 [batch, c, hw] dense.
 *   loss_w           fp32 [batch, loss_w_channels, hw] with loss_w_channels 1 (broadcast over c) or c; NULL: no weighting
 *   t                int32 [batch]; logvar, lvlb_weights: fp32 tables of n_t entries
 *   loss_type        UPK_LOSS_L2: e = (target - pred)^2; UPK_LOSS_L1: e = |target - pred|
 *   per element      d = fl(target - pred), e = fl(d * d) or |d|, we = fl(w * e) (we = e without loss_w): fp32, one IEEE
 *                    operation at a time, as the reference forms them
 *   per sample b     simple[b] = mean over (c, hw) of we, plain[b] = mean over (c, hw) of e
 *   batch            loss_simple = mean_b simple[b];  loss_gamma = mean_b (simple[b] / exp(logvar[t_b]) + logvar[t_b]);
 *                    loss_vlb = mean_b (lvlb_weights[t_b] * plain[b]);
 *                    loss = l_simple_weight * loss_gamma + original_elbo_weight * loss_vlb
 *   out              fp32 [4 + 2 batch]: {loss, loss_simple, loss_gamma, loss_vlb}, then {simple[b], plain[b]} per sample
 *   ws               upk_p_losses_ws_bytes(batch, c, hw) bytes (0 for sizes upk_p_losses_f32 would refuse), 16-byte aligned:
 *                    one slot of two fp64 partial sums per workgroup
 * Every fp32 term is widened to fp64 when it is made, and everything after it (the sums, the means, exp, the batch terms)
 * is fp64, rounded once to fp32 on output: simple, plain, loss_simple and loss_vlb are within relative 4 * 2^-24 of the exact
 * value for the given fp32 inputs (three roundings per non-negative term, one at the output), loss_gamma and loss within
 * 4 * 2^-24 of the sum of the magnitudes of their terms.  Deterministic like upk_ssim_u8: no float atomics; every workgroup
 * (one sample's chunk of 4096 elements) writes its own slot and a fixed-order pass sums them, so reruns are bit-identical
 * and simple[b], plain[b] depend neither on the sample's position in the batch nor on the batch size, nor on whether the
 * 16-byte loads were used (hw % 4 == 0 and model_out, target, loss_w 16-byte aligned; one element per load otherwise).
 * A t_b outside [0, n_t) is never used as an index: simple[b], plain[b] and with them the four batch values are NaN.
 * Errors: UPK_EINVAL for null pointers (loss_w excepted), non-positive sizes, another loss_type, loss_w with a channel count
 * other than 1 or c, an fp32 / int32 pointer not 4-byte or ws not 16-byte aligned; UPK_ESHAPE for c * hw above 2^31 - 1 -
 * 8192 or more than 2^31 - 1 workgroups; UPK_EWORKSPACE for ws_bytes below upk_p_losses_ws_bytes.  Two launches (partial
 * sums, final pass). */
#define UPK_LOSS_L2 0
#define UPK_LOSS_L1 1
size_t upk_p_losses_ws_bytes(int batch, int c, int hw);
int upk_p_losses_f32(upk_ctx* ctx, const float* model_out, const float* target, const float* loss_w, int loss_w_channels,
                     const int32_t* t, const float* logvar, const float* lvlb_weights, int n_t, int loss_type,
                     float l_simple_weight, float original_elbo_weight, float* out, int batch, int c, int hw, void* ws,
                     size_t ws_bytes, upk_stream stream);

/* ------------------------------------------------------------------ */
/* CU-partitioned streams (execution lanes on disjoint CU sets).         */
/* The reference has no counterpart: it runs one batch on `cuda:0`       */
/* (app.py:21); lanes are this build's serving mode. */
/* ------------------------------------------------------------------ */
/* Creates a stream whose kernels are only placed on the CUs whose bit is set in `mask` (nwords 32-bit words, bit b of
 * word w = CU-mask bit 32 w + b of the HSA queue; how bits map to XCDs is measured with upk_probe_placement, not
 * assumed).  The caller owns the stream (upk_stream_destroy).  Never synchronises. */
int upk_stream_create_cumask(upk_ctx* ctx, const uint32_t* mask, int nwords, upk_stream* out);
int upk_stream_destroy(upk_ctx* ctx, upk_stream stream);
/* Launches `nblocks` one-wave workgroups on `stream`; workgroup i writes {HW_REG_XCC_ID, HW_REG_HW_ID} to
 * out_dev[2 i], out_dev[2 i + 1] (device memory, 8 nblocks bytes) and holds its CU for ~spin_cycles shader clocks so that
 * the grid spreads over every CU the stream may use.  Graph-capturable. */
int upk_probe_placement(upk_ctx* ctx, uint32_t* out_dev, int nblocks, int spin_cycles, upk_stream stream);
/* One wave spins for ~spin_wall_ticks ticks of the constant 100 MHz wall clock and writes {shader-clock cycles elapsed,
 * wall ticks elapsed} to out_dev[0..1] (two uint64): shader MHz = 100 * out[0] / out[1] — the clock the chip sustains under
 * whatever else is running (bench.py reports it for the timed configuration). */
int upk_probe_clock(upk_ctx* ctx, unsigned long long* out_dev, long long spin_wall_ticks, upk_stream stream);

/* ------------------------------------------------------------------ */
/* Keyed device noise: Philox4x32-10 normals as a pure function of     */
/* (key, element, row, stream, draw).                                   */
/* ------------------------------------------------------------------ */
/* upk_randn_keyed_f32 fills the noise tables the sampler step kernels read (and x_T) without a generator state: one
 * launch, no allocation, no host state, no synchronisation; graph-capturable; counted in class "other".
 *
 * Generator: Philox4x32-10 (Salmon et al., SC'11) with the Random123 constants: multipliers M0 = 0xD2511F53, M1 =
 * 0xCD9E8D57, Weyl key increments 0x9E3779B9 (k0) and 0xBB67AE85 (k1).  One round: hi0:lo0 = M0 * c0, hi1:lo1 = M1 * c2
 * (32 x 32 -> 64 bit), c <- {hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0}, then k0 += 0x9E3779B9, k1 += 0xBB67AE85; ten rounds.
 *   key      (k0, k1) = keys[2 b], keys[2 b + 1] of sample b: uint32 [batch, 2] on the device
 *   counter  (c0, c1, c2, c3) = (q, row, stream_id, draw): q = e >> 2 for element e of the sample's n elements (n <= 2^34),
 *            row = the ABSOLUTE row of the table (row0 + r for the r-th row written), stream_id = the use the caller
 *            separates (x_T, step noise, q_sample noise, ...), draw = the sampling call among calls that share keys
 * The four output words (w0, w1, w2, w3) of that call belong to elements 4 q .. 4 q + 3; with n % 4 != 0 the words past
 * element n - 1 are discarded.  upk_philox_u32 writes word e & 3 for element e.
 * Normals (Box-Muller on the word pairs (w0, w1) -> elements 4 q, 4 q + 1 and (w2, w3) -> elements 4 q + 2, 4 q + 3):
 *   u1 = ((w_a >> 8) + 1) * 2^-24    in (0, 1], exact in fp32
 *   u2 = (w_b >> 8) * 2^-24          in [0, 1), exact in fp32
 *   r = sqrt(-2 ln u1);  z_a = r cos(2 pi u2),  z_b = r sin(2 pi u2)
 * evaluated in fp32 (log, one multiplication, a correctly rounded sqrt, cos / sin of pi * (2 u2) with 2 u2 exact, one
 * multiplication each; no FMA contraction): within 1e-5 of the fp64 value of the same formula, |z| <= sqrt(48 ln 2) < 5.77.
 * Layout: element e of sample b of row r (row0 <= r < row0 + rows) is
 *   out[(r - row0) * batch * n + b * n + e] = fl(z * row_scale[r])      (row_scale == NULL: z)
 * the layout of the [rows, batch * n] step-noise tables and, with rows == 1, of a dense [batch, C, H, W] latent.  row_scale
 * is a device fp32 table indexed by the absolute row (at least row0 + rows entries); a row whose scale is 0 is written
 * as +0.  A value depends on nothing but (key, e, row, stream_id, draw) and the row's scale: not on batch, on the sample's
 * position in the batch, on the [row0, row0 + rows) window, on the alignment of out or on the launch geometry.  Stores are
 * 16 bytes wide wherever four consecutive elements of a sample fill an aligned group of out (out + b * n need not be aligned:
 * heads and tails go element by element).
 * Errors: UPK_EINVAL for null keys / out, non-positive batch, n or rows, negative row0 (or row0 + rows above 2^31 - 1),
 * n above 2^34, a pointer not 4-byte aligned; UPK_ESHAPE for a table of 2^62 elements or more. */
int upk_randn_keyed_f32(upk_ctx* ctx, const uint32_t* keys, int batch, long long n, int row0, int rows, uint32_t stream_id,
                        uint32_t draw, const float* row_scale, float* out, upk_stream stream);
/* The raw Philox word of every element, same layout, same device function as the normals (the integer stage, exactly
 * testable): out[(r - row0) * batch * n + b * n + e] = w[e & 3] of the call with counter (e >> 2, r, stream_id, draw).
 * Errors as above. */
int upk_philox_u32(upk_ctx* ctx, const uint32_t* keys, int batch, long long n, int row0, int rows, uint32_t stream_id,
                   uint32_t draw, uint32_t* out, upk_stream stream);
/* The values of the counter's stream_id word the library itself uses (upgpt_amd/rng.py names 0 .. 3: x_T, the step noise,
 * the q_sample noise of a sampler, the first stage's posterior sample). */
#define UPK_STREAM_TIMESTEP 4   /* the timestep of a loss evaluation */
#define UPK_STREAM_LOSS_NOISE 5 /* its noise */
/* upk_q_sample_keyed_f32: upk_q_sample_f32 with the timestep and the noise drawn inside the kernel from the sample's key:
 * one launch for upk_randn_keyed_f32 (a noise table) + a host-made t + upk_q_sample_f32.  Never allocates, never
 * synchronises, graph-capturable, class "other".
 *   keys             uint32 [batch, 2] on the device; draw: the counter's draw word (both as in upk_randn_keyed_f32)
 *   x_start          fp32 NCHW [batch, c, hw], dense; a, s: the two fp32 schedule tables of n_t entries, as in upk_q_sample_f32
 *   t_in             int32 [batch], or NULL.  NULL: t_b = (w0 * n_t) >> 32 as a 64-bit product, w0 = word 0 of the Philox call
 *                    with counter (0, 0, UPK_STREAM_TIMESTEP, draw) and the key of sample b: uniform on [0, n_t), every value's
 *                    probability within n_t * 2^-32 relative of 1 / n_t.  Non-NULL: t_b = t_in[b] (t_in == t_out is allowed)
 *   t_out            int32 [batch], never NULL: t_b, what upk_p_losses_f32 and the forward plan's timestep rows read
 *   noise            element e of sample b is n = the normal of counter (e >> 2, 0, UPK_STREAM_LOSS_NOISE, draw), word pair
 *                    and transform as above: bit for bit what upk_randn_keyed_f32(rows = 1, row0 = 0, stream_id =
 *                    UPK_STREAM_LOSS_NOISE, draw, row_scale = NULL) writes
 *   noise_out        fp32 [batch, c, hw] <- n (the target of an eps model), or NULL
 *   x_noisy          fp32 [batch, c, hw] <- v, or NULL
 *   xin              fp16 NHWC [batch * hw, ld_xin] <- v rounded once to fp16 in channels [0, c), or NULL; channels >= c of a
 *                    row are left untouched
 * At least one of noise_out, x_noisy, xin must be given.  v = fl(fl(a[t_b] * x0) + fl(s[t_b] * n)), no FMA contraction: bit for
 * bit what upk_q_sample_f32 gives for that noise and t.  A t_in[b] outside [0, n_t) is never used as an index: x_noisy and
 * xin of that sample are NaN, its noise_out and the other samples are as without it.  A value depends on (key, draw, element)
 * and x_start alone: not on batch, on the sample's position, on the alignment of a pointer or on the launch geometry.  A
 * thread moves the four elements 4 q .. 4 q + 3 of a sample with one 16-byte load / store per tensor whose address of that
 * quad is 16-byte aligned, element by element otherwise (and for the sample's last c * hw % 4 elements).
 * Errors: UPK_EINVAL for null keys, x_start, tables or t_out, noise_out, x_noisy and xin all NULL, non-positive sizes,
 * ld_xin < c, an fp32 / int32 / uint32 pointer not 4-byte or xin not 2-byte aligned; UPK_ESHAPE for c * hw above
 * 2^31 - 1 - 8192. */
int upk_q_sample_keyed_f32(upk_ctx* ctx, const uint32_t* keys, uint32_t draw, const float* x_start, const int32_t* t_in,
                           const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod, int n_t,
                           int32_t* t_out, float* noise_out, float* x_noisy, void* xin, int ld_xin, int batch, int c, int hw,
                           upk_stream stream);

/* ------------------------------------------------------------------ */
/* HIP graph helpers (the 50-step loop replays one captured step).      */
/* ------------------------------------------------------------------ */
typedef struct upk_graph upk_graph;
int upk_graph_begin(upk_ctx* ctx, upk_stream stream);
int upk_graph_end(upk_ctx* ctx, upk_stream stream, upk_graph** out);
int upk_graph_launch(upk_ctx* ctx, upk_graph* g, upk_stream stream);
int upk_graph_destroy(upk_ctx* ctx, upk_graph* g);

/* ------------------------------------------------------------------ */
/* Per-kernel-class timing with HIP events on the launch stream          */
/* (bench.py roofline).  Classes: 0 igemm, 1 attention, 2 groupnorm,     */
/* 3 layernorm, 4 other.                                                  */
/* ------------------------------------------------------------------ */
#define UPK_NUM_CLASSES 5
int upk_prof_enable(upk_ctx* ctx, int on);
/* Synchronises the recorded events and returns accumulated ms / launches
 * per class since the last reset (host arrays of UPK_NUM_CLASSES). */
int upk_prof_collect(upk_ctx* ctx, double* ms_host, long long* launches_host);

#ifdef __cplusplus
}
#endif
#endif /* UPK_H_ */
