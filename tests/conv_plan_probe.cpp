// Prints what the conv launcher decides for a fixed list of descriptors, on a CPU-only machine: the planning half of
// upk_conv2d_nhwc_f16 needs no device, so a hand-made upk_ctx and dummy addresses are enough (nothing is dereferenced,
// nothing is launched).  tests/test_conv_plan_host.py compares the output with tests/golden/conv_plan.txt, recorded
// before the launcher was split into conv_plan / conv_launch: a difference is a behaviour change.
// Only public entry points are used, so the file compiles against any revision of the library.
//
// One line per (descriptor, context).  cm = the cost model's choice; sweep = every configuration index pinned with
// split-K slot 0, 1 and 4 through tune_cfg / tune_splitk, run-length packed; ovr = the same through upk_conv_override
// ("same" when equal).  A result is mode/nblk/slots (upk_conv_gn_fused, upk_conv_ln_rows) or !rc:eN for a failure, with
// the message texts listed under their numbers at the end.
#include <map>
#include <string>

#include "../upgpt_amd/csrc/common.h"

static std::vector<std::string> g_msgs;
static std::map<std::string, int> g_msg_id;

static std::string err_id(const upk_ctx& ctx) {
  auto it = g_msg_id.find(ctx.err);
  if (it == g_msg_id.end()) {
    it = g_msg_id.emplace(ctx.err, (int)g_msgs.size()).first;
    g_msgs.push_back(ctx.err);
  }
  return "e" + std::to_string(it->second);
}

static std::string query(upk_ctx& ctx, const upk_conv_desc& d) {
  int mode = -1, nblk = -1, slots = -1;
  ctx.err[0] = 0;
  const int rg = upk_conv_gn_fused(&ctx, &d, &mode, &nblk);
  const std::string eg = rg ? err_id(ctx) : "";
  ctx.err[0] = 0;
  const int rl = upk_conv_ln_rows(&ctx, &d, &slots);
  const std::string el = rl ? err_id(ctx) : "";
  const std::string out = std::to_string(mode) + "/" + std::to_string(nblk) + "/" + std::to_string(slots);
  if (!rg && !rl) return out;
  std::string s = "!" + std::to_string(rg) + ":" + eg;
  if (rl != rg || el != eg) s += "|" + std::to_string(rl) + ":" + el;
  if (out != "0/0/0") s += "?" + out;
  return s;
}

static const int kSks[] = {0, 1, 4};

static std::string sweep(upk_ctx& ctx, upk_conv_desc d, bool by_override) {
  std::string packed, prev;
  int run = 0;
  auto flush = [&]() {
    if (run) packed += (packed.empty() ? "" : " ") + prev + (run > 1 ? "*" + std::to_string(run) : "");
  };
  for (int c = 0; c < upk_conv_num_configs(); ++c)
    for (int sk : kSks) {
      if (by_override) upk_conv_override(&ctx, c, sk);
      else d.tune_cfg = c + 1, d.tune_splitk = sk;
      const std::string r = query(ctx, d);
      if (r == prev) ++run;
      else flush(), prev = r, run = 1;
    }
  flush();
  upk_conv_override(&ctx, -1, 0);
  return packed;
}

static void* ptr(int i) { return (void*)(uintptr_t)(0x10000 + 0x1000 * i); }

// conv / Linear with nothing optional: NHWC fp16 in and out, bias
static upk_conv_desc base(int b, int h, int w, int cin, int nout, int ks) {
  upk_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x1 = ptr(1), d.c1 = cin, d.ld1 = cin;
  d.batch = b, d.in_h = h, d.in_w = w, d.ksize = ks, d.stride = 1;
  d.w_packed = ptr(2), d.n_out = nout, d.n_pad = (nout + 15) / 16 * 16, d.bias = (const float*)ptr(3);
  d.y = ptr(4), d.ldy = nout;
  return d;
}

struct Case {
  std::string name;
  upk_conv_desc d;
  bool sweep;  // false: the cost model's answer only (descriptors that fail their checks)
  bool small_ws;  // also on the 1 MB context
};

int main() {
  upk_ctx big{}, small{};
  for (upk_ctx* c : {&big, &small}) {
    c->num_cus = 256;
    c->ws = ptr(100);
    c->zero_page = ptr(101);
    c->cfg_override = -1;
  }
  big.ws_bytes = (size_t)256 << 20;  // _lib.Context's default
  small.ws_bytes = (size_t)1 << 20;

  std::vector<Case> cases;
  auto add = [&](const char* name, upk_conv_desc d, bool sw = true, bool small_ws = false) {
    cases.push_back({name, d, sw, small_ws});
  };
  upk_conv_desc d;
  // ---- bases: the production levels, 3x3 and 1x1
  add("b8_32x24_224_3x3", base(8, 32, 24, 224, 224, 3), true, true);
  add("b2_16x12_448_3x3", base(2, 16, 12, 448, 448, 3));
  add("b8_8x6_896_3x3", base(8, 8, 6, 896, 896, 3), true, true);
  add("b2_4x3_896_3x3", base(2, 4, 3, 896, 896, 3));
  add("b8_16x12_448_1x1", base(8, 16, 12, 448, 448, 1));
  add("b2_32x24_224_1x1", base(2, 32, 24, 224, 224, 1));
  add("b2_32x32_256_3x3", base(2, 32, 32, 256, 256, 3));
  add("b8_32x32_256to512_1x1", base(8, 32, 32, 256, 512, 1));
  add("b2_8x6_1024_1x1", base(2, 8, 6, 1024, 1024, 1));
  add("b8_32x24_96_3x3", base(8, 32, 24, 96, 96, 3));
  add("b2_16x12_192_1x1", base(2, 16, 12, 192, 192, 1));
  add("b8_8x6_384_3x3", base(8, 8, 6, 384, 384, 3));
  add("b2_256x192_128_3x3_vae", base(2, 256, 192, 128, 128, 3));
  d = base(1, 8, 1, 224, 896, 1), d.flags = UPK_F_SILU;
  add("linear_m8_224to896_silu", d);
  d = base(1, 696, 1, 768, 448, 1), d.flags = UPK_F_OUT_F32;
  add("linear_m696_768to448_outf32", d);
  // ---- modifiers
  d = base(2, 16, 12, 448, 448, 3), d.residual = ptr(5), d.ld_res = 448;
  add("b2_16x12_448_3x3+res", d);
  d = base(8, 16, 12, 448, 448, 1), d.residual = ptr(5), d.ld_res = 448, d.ln_rows_out = (float*)ptr(6);
  add("b8_16x12_448_1x1+res+lnr_out", d);
  d = base(2, 16, 12, 192, 192, 1), d.ln_rows_out = (float*)ptr(6);
  add("b2_16x12_192_1x1+lnr_out", d);
  d = base(2, 8, 6, 1024, 1024, 1), d.ln_rows_out = (float*)ptr(6);
  add("b2_8x6_1024_1x1+lnr_out", d);
  d = base(8, 32, 24, 224, 224, 1), d.ln_rows_out = (float*)ptr(6), d.gn_stats_ws = (float*)ptr(7), d.gn_groups = 32;
  add("b8_32x24_224_1x1+lnr_out+gn_ws", d);
  d = base(8, 32, 24, 224, 224, 3), d.rowvec = (const float*)ptr(8), d.rv_batch_stride = 224, d.gn_stats_ws = (float*)ptr(7), d.gn_groups = 32;
  add("b8_32x24_224_3x3+rowvec+gn_ws", d);
  d = base(2, 32, 32, 256, 256, 3), d.gn_stats_ws = (float*)ptr(7), d.gn_groups = 32;
  add("b2_32x32_256_3x3+gn_ws", d);
  d = base(2, 256, 192, 128, 128, 3), d.gn_stats_ws = (float*)ptr(7), d.gn_groups = 32;
  add("b2_256x192_128_3x3_vae+gn_ws_cap0", d);
  d.gn_stats_cap = 512;
  add("b2_256x192_128_3x3_vae+gn_ws_cap512", d);
  d = base(8, 32, 24, 224, 224, 3), d.x2 = ptr(9), d.c2 = 224, d.ld2 = 224;
  add("b8_32x24_224+224_3x3_concat", d);
  d = base(2, 16, 12, 448, 448, 3), d.x3 = ptr(10), d.c3 = 224, d.ld3 = 224;
  add("b2_16x12_448_3x3+x3", d);
  d.x2 = ptr(9), d.c2 = 224, d.ld2 = 224, d.x4 = ptr(11), d.c4 = 448, d.ld4 = 448, d.gn_stats_ws = (float*)ptr(7), d.gn_groups = 32;
  add("b2_16x12_448+224_3x3+x3+x4+gn_ws", d);
  d = base(8, 16, 12, 448, 1344, 1), d.ln_colsum = (const float*)ptr(12), d.ln_eps = 1e-5f, d.ln_dim = 448;
  add("b8_16x12_448to1344_1x1+ln", d);
  d.ln_rows_in = (const float*)ptr(6), d.ln_rows_slots = 2;
  add("b8_16x12_448to1344_1x1+ln+lnr_in", d);
  d.vt = ptr(13), d.vt_from = 896, d.vt_heads = 8, d.vt_dhead = 56, d.vt_ld = 192, d.vt_tokens = 192;
  add("b8_16x12_448to1344_1x1+ln+lnr_in+vt", d);
  d = base(2, 32, 24, 224, 896, 1), d.n_pad = 1792, d.flags = UPK_F_GEGLU;
  add("b2_32x24_224to896_geglu", d);
  d.ln_colsum = (const float*)ptr(12), d.ln_eps = 1e-5f, d.ln_dim = 224;
  add("b2_32x24_224to896_geglu+ln", d);
  d = base(8, 8, 6, 896, 3584, 1), d.n_pad = 7168, d.flags = UPK_F_GEGLU, d.ln_colsum = (const float*)ptr(12), d.ln_dim = 896;
  d.ln_rows_in = (const float*)ptr(6), d.ln_rows_slots = 4;
  add("b8_8x6_896to3584_geglu+ln+lnr_in", d);
  d = base(2, 8, 6, 896, 896, 3), d.flags = UPK_F_UPSAMPLE2X;
  add("b2_8x6_896_3x3+ups", d);
  d.w_phase = ptr(14);
  add("b2_8x6_896_3x3+ups+w_phase", d);
  d = base(2, 128, 96, 256, 256, 3), d.flags = UPK_F_UPSAMPLE2X, d.w_phase = ptr(14);
  add("b2_128x96_256_3x3_vae+ups+w_phase", d);
  d = base(8, 32, 24, 224, 224, 3), d.stride = 2;
  add("b8_32x24_224_3x3_s2", d);
  d = base(2, 256, 192, 128, 128, 3), d.stride = 2, d.flags = UPK_F_PAD_ASYM;
  add("b2_256x192_128_3x3_s2_pad_asym", d);
  d = base(8, 32, 24, 224, 4, 3), d.ldy = 0, d.flags = UPK_F_OUT_NCHW_F32;
  add("b8_32x24_224to4_3x3_nchw", d);
  d = base(8, 8, 6, 896, 896, 3), d.rowvec = (const float*)ptr(8), d.rv_batch_stride = 896, d.gn_groups = 32;
  d.gno_gamma = (const float*)ptr(15), d.gno_beta = (const float*)ptr(16), d.gno_y = ptr(17), d.gno_eps = 1e-5f, d.gno_silu = 1, d.gno_ld = 896;
  d.gn_stats_ws = (float*)ptr(7);
  add("b8_8x6_896_3x3+rowvec+gno+gn_ws", d);
  d.batch = 2, d.in_h = 4, d.in_w = 3, d.gn_stats_ws = nullptr;
  add("b2_4x3_896_3x3+rowvec+gno", d);
  d = base(2, 16, 12, 448, 448, 3), d.gn_groups = 32, d.gn_stats_ws = (float*)ptr(7);
  d.gno_gamma = (const float*)ptr(15), d.gno_beta = (const float*)ptr(16), d.gno_y = ptr(17), d.gno_ld = 448;
  add("b2_16x12_448_3x3+gno+gn_ws", d);
  // ---- descriptors the checks refuse (one per message)
  d = base(2, 16, 12, 448, 448, 3), d.y = nullptr;
  add("bad_null_y", d, false);
  d = base(2, 16, 12, 440, 448, 3);
  add("bad_c1", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.c2 = 32;
  add("bad_x2_null", d, false);
  add("bad_ksize", base(2, 16, 12, 448, 448, 5), false);
  d = base(2, 16, 12, 448, 448, 3), d.stride = 3;
  add("bad_stride", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.n_pad = 450;
  add("bad_n_pad", d, false);
  d = base(2, 16, 12, 448, 896, 1), d.n_pad = 1776, d.flags = UPK_F_GEGLU;
  add("bad_geglu_n_pad", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.ldy = 450;
  add("bad_ldy", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.residual = ptr(5), d.ld_res = 450;
  add("bad_ld_res", d, false);
  d = base(2, 16, 12, 448, 1344, 1), d.vt = ptr(13), d.vt_from = 896, d.vt_heads = 8, d.vt_dhead = 0, d.vt_ld = 192, d.vt_tokens = 192;
  add("bad_vt", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.flags = UPK_F_PAD_ASYM;
  add("bad_pad_asym_s1", d, false);
  add("bad_empty", base(0, 16, 12, 448, 448, 3), false);
  d = base(2, 16, 12, 448, 448, 1), d.ln_colsum = (const float*)ptr(12), d.ln_dim = 448, d.ln_rows_in = (const float*)ptr(6), d.ln_rows_slots = 9;
  add("bad_ln_rows_slots", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.ln_colsum = (const float*)ptr(12), d.ln_dim = 448;
  add("bad_ln_3x3", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.x3 = ptr(10), d.c3 = 100, d.ld3 = 100;
  add("bad_c3", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.x3 = ptr(10), d.c3 = 224, d.ld3 = 224, d.stride = 2;
  add("bad_x3_s2", d, false);
  d = base(2, 16, 12, 448, 448, 3), d.tune_cfg = upk_conv_num_configs() + 1;
  add("bad_tune_cfg", d, false);

  for (const Case& c : cases)
    for (upk_ctx* ctx : {&big, &small}) {
      if (ctx == &small && !c.small_ws) continue;
      printf("%s ws=%zuMB cm=%s", c.name.c_str(), ctx->ws_bytes >> 20, query(*ctx, c.d).c_str());
      if (c.sweep) {
        const std::string s = sweep(*ctx, c.d, false), o = sweep(*ctx, c.d, true);
        printf(" sweep=[%s] ovr=[%s]", s.c_str(), o == s ? "same" : o.c_str());
      }
      printf("\n");
    }
  const int rc = upk_conv_override(&big, upk_conv_num_configs(), 0);
  printf("override_out_of_range rc=%d %s\n", rc, err_id(big).c_str());
  printf("configs=%d\n", upk_conv_num_configs());
  for (size_t i = 0; i < g_msgs.size(); ++i) printf("e%zu %s\n", i, g_msgs[i].c_str());
  return 0;
}
