"""tests/launch_ref.py against independent fp64 PyTorch formulations of the same launch, one upk_conv_desc feature at a
time and at tiny shapes, and its sensitivity: the reference passes itself and a correctly rounded output, and fails an
output with one element moved by 4 ulp, one K chunk or one split-K slice left out of a row, or the last 16 columns
missing.  tests/test_production_launches_gpu.py relies on both: it may not be shown to fail by breaking a kernel."""
import pytest
import torch
import torch.nn.functional as F

import launch_ref as LR
import range_ref as R
from upgpt_amd import _lib as L

F64 = torch.float64
d64 = lambda t: t.to(F64)
w16 = lambda w: R.q16(d64(w))
nchw = lambda x: d64(x).permute(0, 3, 1, 2)
rows = lambda y: y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])  # NCHW -> [M, N]


def operands(B, H, W, c1, N, ks=1, c2=0, seg=None, seed=0, Ho=None, Wo=None):
    """x1 / x2 / x3 / x4, w / w_app and a bias at unit scale; NHWC fp16 sources with 32 spare channels behind c1 that a
    correct reference never reads."""
    o = {"x1": R.activations((B, H, W, c1 + 32), seed), "w": R.weights((N, c1 + c2, ks, ks), ks * ks * (c1 + c2), seed + 1),
         "bias": R.vector(N, seed + 2)}
    if c2:
        o["x2"] = R.activations((B, H, W, c2), seed + 3)
    if seg:
        o["x3"] = R.activations((B, Ho or H, Wo or W, seg[0]), seed + 4)
        if seg[1]:
            o["x4"] = R.activations((B, Ho or H, Wo or W, seg[1]), seed + 5)
        o["w_app"] = R.weights((N, sum(seg), 1, 1), sum(seg), seed + 6)
    return o


def close(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------------- the sources
def test_concat_and_stride_2_against_conv2d():
    B, H, W, c1, c2, N = 2, 6, 5, 32, 64, 48
    o = operands(B, H, W, c1, N, ks=3, c2=c2)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, c2=c2, ld1=c1 + 32, ld2=c2, x1=True, x2=True, ksize=3, stride=2, n_out=N,
                  n_pad=N, bias=True, ldy=N)
    ref, bound = LR.launch_ref(f, o)["y"]
    x = torch.cat([nchw(o["x1"][..., :c1]), nchw(o["x2"])], 1)
    close(ref, rows(F.conv2d(x, w16(o["w"]), d64(o["bias"]), stride=2, padding=1)))
    assert bool((bound > 0).all())


def test_asymmetric_padding_and_nchw_f32_output_against_padded_conv2d():
    B, H, W, c1, N = 2, 8, 6, 32, 4
    o = operands(B, H, W, c1, N, ks=3)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=3, stride=2, n_out=N, n_pad=16, bias=True,
                  flags=L.F_PAD_ASYM | L.F_OUT_NCHW_F32, ldy=0)
    ref, bound = LR.launch_ref(f, o)["y"]
    want = F.conv2d(F.pad(nchw(o["x1"][..., :c1]), (0, 1, 0, 1)), w16(o["w"]), d64(o["bias"]), stride=2)
    close(ref, want)  # [B, n_out, Ho, Wo]: nothing of the 12 padding rows of n_pad
    assert bound.shape == want.shape and bool((bound >= R.E32 * want.abs()).all())


def test_nearest_2x_upsample_against_interpolate():
    B, H, W, c1, N = 2, 4, 3, 64, 32
    o = operands(B, H, W, c1, N, ks=3)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=3, stride=1, n_out=N, n_pad=N, bias=True,
                  flags=L.F_UPSAMPLE2X, ldy=N)
    ref, _ = LR.launch_ref(f, o)["y"]
    x = F.interpolate(nchw(o["x1"][..., :c1]), scale_factor=2, mode="nearest")
    close(ref, rows(F.conv2d(x, w16(o["w"]), d64(o["bias"]), padding=1)))


@pytest.mark.parametrize("ks,c4", [(3, 32), (1, 0)])
def test_appended_1x1_segment_against_two_conv2d(ks, c4):
    B, H, W, c1, c3, N = 2, 5, 4, 64, 96, 32
    o = operands(B, H, W, c1, N, ks=ks, seg=(c3, c4))
    o["residual"] = R.activations((B * H * W, N + 8), 9)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=ks, stride=1, n_out=N, n_pad=N, bias=True,
                  x3=True, c3=c3, ld3=c3, x4=bool(c4), c4=c4, ld4=c4, residual=True, ld_res=N + 8, ldy=N)
    ref, _ = LR.launch_ref(f, o)["y"]
    xs = nchw(o["x3"]) if not c4 else torch.cat([nchw(o["x3"]), nchw(o["x4"])], 1)
    want = F.conv2d(nchw(o["x1"][..., :c1]), w16(o["w"]), d64(o["bias"]), padding=ks // 2) + F.conv2d(xs, w16(o["w_app"]))
    close(ref, rows(want) + d64(o["residual"][:, :N]))


# ------------------------------------------------------------------------------------------------------ the epilogue
@pytest.mark.parametrize("act,f32", [(L.F_SILU, False), (L.F_QUICKGELU, False), (0, True)])
def test_bias_rowvec_activation_residual_in_the_kernels_order(act, f32):
    """v = acc + bias + rowvec[step][b]; v = act(v); v += residual (upgpt_amd/csrc/igemm_common.h Epi::store)."""
    B, H, W, c1, N = 3, 4, 2, 64, 32
    o = operands(B, H, W, c1, N)
    rv_ss, rv_bs, step = 200, 40, 2
    o["rowvec"], o["step"] = R.vector(3 * rv_ss, 11, 1.0), step
    o["residual"] = R.activations((B * H * W, N), 12)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=1, stride=1, n_out=N, n_pad=N, bias=True,
                  rowvec=True, rv_step_stride=rv_ss, rv_batch_stride=rv_bs, step=True, residual=True, ld_res=N,
                  flags=act | (L.F_OUT_F32 if f32 else 0), ldy=N)
    ref, bound = LR.launch_ref(f, o)["y"]
    v = F.linear(d64(o["x1"][..., :c1]), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))  # [B, H, W, N]
    rv = torch.stack([d64(o["rowvec"][step * rv_ss + b * rv_bs:][:N]) for b in range(B)])
    v = v + rv[:, None, None, :]
    v = F.silu(v) if act == L.F_SILU else v * torch.sigmoid(1.702 * v) if act == L.F_QUICKGELU else v
    close(ref, v.reshape(-1, N) + d64(o["residual"]))
    assert bool((bound >= (R.E32 * ref.abs() if f32 else R.u16(ref))).all())
    # without a step pointer row 0 of the table is read
    ref0, _ = LR.launch_ref(dict(f, step=False), o)["y"]
    assert float((ref0 - ref).abs().max()) > 0.1


def test_geglu_against_linear_and_gelu():
    M, c1, n_out = 24, 64, 64
    o = operands(1, M, 1, c1, 2 * n_out)
    f = LR.fields(batch=1, in_h=M, in_w=1, c1=c1, ld1=c1 + 32, x1=True, ksize=1, stride=1, n_out=n_out, n_pad=2 * n_out,
                  bias=True, flags=L.F_GEGLU, ldy=n_out)
    ref, _ = LR.launch_ref(f, o)["y"]
    h = F.linear(d64(o["x1"][0, :, 0, :c1]), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))
    close(ref, h[:, :n_out] * F.gelu(h[:, n_out:]))


def test_transposed_tail_against_a_permute():
    B, tok, c1, heads, dh = 2, 6, 32, 2, 8
    hd = heads * dh
    o = operands(1, B * tok, 1, c1, 3 * hd)
    f = LR.fields(batch=1, in_h=B * tok, in_w=1, c1=c1, ld1=c1 + 32, x1=True, ksize=1, stride=1, n_out=2 * hd, n_pad=3 * hd,
                  bias=True, ldy=2 * hd, vt=True, vt_from=2 * hd, vt_heads=heads, vt_dhead=dh, vt_ld=32, vt_tokens=tok)
    out = LR.launch_ref(f, o)
    full = F.linear(d64(o["x1"][0, :, 0, :c1]), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))
    close(out["y"][0], full[:, :2 * hd])
    close(out["vt"][0], full[:, 2 * hd:].reshape(B, tok, heads, dh).permute(0, 2, 3, 1))
    assert out["vt"][1].shape == (B, heads, dh, tok)


@pytest.mark.parametrize("rows_in", [False, True])
@pytest.mark.parametrize("geglu", [False, True])
def test_folded_layernorm_against_layer_norm_then_linear(rows_in, geglu):
    """W' = fp16(W gamma), b' = b + W beta, u = column sums of W': the launch equals LayerNorm (with the affine) followed
    by the Linear on W' / gamma — written here with the affine folded on the PyTorch side too, i.e. plain normalisation
    followed by F.linear(W', b')."""
    M, c1, N = 20, 64, 128
    n_out = N // 2 if geglu else N
    o = operands(1, M, 1, c1, N)
    o["x1"] = R.norm_input((1, M, 1, c1), 5, 1)
    o["ln_colsum"] = w16(o["w"])[:, :, 0, 0].sum(1).float()
    f = LR.fields(batch=1, in_h=M, in_w=1, c1=c1, ld1=c1, x1=True, ksize=1, stride=1, n_out=n_out, n_pad=N, bias=True,
                  ln_colsum=True, ln_eps=1e-5, ln_dim=c1, ln_rows_in=rows_in, ln_rows_slots=3 if rows_in else 0,
                  flags=L.F_GEGLU if geglu else 0, ldy=n_out)
    ref, bound = LR.launch_ref(f, o)["y"]
    x = d64(o["x1"][0, :, 0])
    h = F.linear(F.layer_norm(x, (c1,), None, None, 1e-5), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))
    want = h[:, :n_out] * F.gelu(h[:, n_out:]) if geglu else h
    # (u is an fp32 sum of fp16 values: the reference uses the fp32 u the kernel is given, PyTorch the exact one)
    assert float((ref - want).abs().max()) <= 1e-5 and float(((ref - want).abs() / bound).max()) < 0.05


def test_folded_layernorm_with_quickgelu_against_layer_norm_linear_and_the_sigmoid_form():
    """The fc1 launch of the CLIP towers: LayerNorm folded into the GEMM, UPK_F_QUICKGELU in its epilogue."""
    M, c1, N = 21, 96, 160
    o = operands(1, M, 1, c1, N, seed=40)
    o["x1"] = R.norm_input((1, M, 1, c1), 41, 1)
    o["ln_colsum"] = w16(o["w"])[:, :, 0, 0].sum(1).float()
    f = LR.fields(batch=1, in_h=M, in_w=1, c1=c1, ld1=c1, x1=True, ksize=1, stride=1, n_out=N, n_pad=N, bias=True,
                  ln_colsum=True, ln_eps=1e-5, ln_dim=c1, flags=L.F_QUICKGELU, ldy=N)
    assert LR.unhandled(f) == []
    ref, bound = LR.launch_ref(f, o)["y"]
    h = F.linear(F.layer_norm(d64(o["x1"][0, :, 0]), (c1,), None, None, 1e-5), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))
    want = h * torch.sigmoid(1.702 * h)
    # (u is the fp32 sum the kernel is given, PyTorch's the exact one: as in the test above)
    assert float((ref - want).abs().max()) <= 1e-5 and float(((ref - want).abs() / bound).max()) < 0.05
    plain, _ = LR.launch_ref(dict(f, flags=0), o)["y"]
    assert float((plain - ref).abs().max()) > 0.1  # (the activation is not a no-op on these operands)


@pytest.fixture(scope="module")
def odd_tokens_vt():
    """The towers' q | k | v launch in small: folded LayerNorm, V^T tail, 3 samples of 7 tokens (M = 21 rows: no power of
    two divides the sample boundaries, so an M tile of any height straddles them), 2 heads of 8, vt_ld = 32."""
    B, tok, c1, heads, dh = 3, 7, 64, 2, 8
    hd = heads * dh
    o = operands(B, tok, 1, c1, 3 * hd, seed=50)
    o["x1"] = R.norm_input((B, tok, 1, c1), 51, 1)
    o["ln_colsum"] = w16(o["w"])[:, :, 0, 0].sum(1).float()
    f = LR.fields(batch=B, in_h=tok, in_w=1, c1=c1, ld1=c1, x1=True, ksize=1, stride=1, n_out=2 * hd, n_pad=3 * hd, bias=True,
                  ldy=2 * hd, ln_colsum=True, ln_eps=1e-5, ln_dim=c1, vt=True, vt_from=2 * hd, vt_heads=heads, vt_dhead=dh,
                  vt_ld=32, vt_tokens=tok)
    assert LR.unhandled(f) == []
    return f, o, LR.launch_ref(f, o)


def test_folded_layernorm_with_a_transposed_tail_at_an_odd_token_count_against_a_permute(odd_tokens_vt):
    f, o, out = odd_tokens_vt
    B, tok, c1, heads, dh = f["batch"], f["vt_tokens"], f["c1"], f["vt_heads"], f["vt_dhead"]
    hd = heads * dh
    x = d64(o["x1"]).reshape(B * tok, c1)
    full = F.linear(F.layer_norm(x, (c1,), None, None, 1e-5), w16(o["w"])[:, :, 0, 0], d64(o["bias"]))
    assert out["y"][0].shape == (B * tok, 2 * hd) and out["vt"][0].shape == out["vt"][1].shape == (B, heads, dh, tok)
    assert float((out["y"][0] - full[:, :2 * hd]).abs().max()) <= 1e-5
    want = torch.empty(B, heads, dh, tok, dtype=F64)
    for b in range(B):  # (an independent permute: element by element from the row of (sample, token))
        for t in range(tok):
            want[b, :, :, t] = full[b * tok + t, 2 * hd:].reshape(heads, dh)
    assert float((out["vt"][0] - want).abs().max()) <= 1e-5
    assert float(((out["vt"][0] - want).abs() / out["vt"][1]).max()) < 0.05
    assert R.ratio(R.q16(out["vt"][0]), *out["vt"]) <= 1


def test_a_tile_that_ignores_the_sample_boundary_fails_at_an_odd_token_count(odd_tokens_vt):
    """Row 7 of the GEMM is (sample 1, token 0).  A tile that computes the V^T address as if the rows of its tile all
    belonged to the tile's first sample puts that row's values where sample 0's token 7 would be — for one element that
    is the slot of sample 0's LAST token, column 6 shifted by one: the value lands in [0, h, e, 6]."""
    f, _, out = odd_tokens_vt
    ref, bound = out["vt"]
    tok = f["vt_tokens"]
    for h, e in ((0, 0), (1, 5)):
        got = R.q16(ref)
        got[0, h, e, tok - 1] = got[1, h, e, 0]
        assert got[0, h, e, tok - 1] != R.q16(ref)[0, h, e, tok - 1]
        assert R.ratio(got, ref, bound) > 1
    for at in ((0, 0, 0, tok - 1), (1, 0, 0, 0), (2, 1, 7, 3)):
        for sign in (1, -1):
            got = R.q16(ref)
            got[at] += sign * 4 * R.u16(got[at])
            assert R.ratio(got, ref, bound) > 1


def test_plain_gemm_of_8_rows_with_fp32_output_against_linear():
    """The pooled projection of the text tower: M = batch rows, no bias, fp32 rows."""
    M, c1, N = 8, 96, 64
    o = operands(M, 1, 1, c1, N, seed=60)
    f = LR.fields(batch=M, in_h=1, in_w=1, c1=c1, ld1=c1 + 32, x1=True, ksize=1, stride=1, n_out=N, n_pad=N,
                  flags=L.F_OUT_F32, ldy=N)
    assert LR.unhandled(f) == []
    ref, bound = LR.launch_ref(f, o)["y"]
    want = F.linear(d64(o["x1"][:, 0, 0, :c1]), w16(o["w"])[:, :, 0, 0])
    close(ref, want)
    assert ref.shape == (M, N) and bool((bound >= R.E32 * want.abs()).all())
    # fp32 rows: the bound has no fp16 output rounding in it, so a correctly rounded fp32 output passes and one that
    # went through fp16 on the way does not
    assert R.ratio(d64(ref.float()), ref, bound) <= 1
    assert R.ratio(R.q16(ref), ref, bound) > 1
    got = ref.clone()
    got[M - 1] = want[M - 2]  # (the last row computed from its neighbour's input)
    assert R.ratio(got, ref, bound) > 1


def test_phase_form_equals_the_direct_3x3_on_weights_that_need_no_rounding():
    """Weights k / 64 with |k| <= 8: they and every sum of up to four taps are fp16 numbers, so neither form rounds
    anything and the four 2x2 convs on the low-resolution grid ARE the 3x3 conv on the upsampled one, exactly."""
    B, H, W, c1, N = 2, 5, 3, 32, 32
    o = operands(B, H, W, c1, N, ks=3)
    g = torch.Generator().manual_seed(3)
    o["w"] = torch.randint(-8, 9, (N, c1, 3, 3), generator=g).float() / 64
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=3, stride=1, n_out=N, n_pad=N, bias=True,
                  flags=L.F_UPSAMPLE2X, ldy=N)
    direct, _ = LR.launch_ref(f, o)["y"]
    phased, _ = LR.launch_ref(dict(f, w_phase=True), o)["y"]
    assert LR.phase_form(dict(f, w_phase=True)) and not LR.phase_form(f)
    close(phased, direct)
    # ... and with weights that do round, the phase form rounds the SUMMED taps (what the packing stores)
    o["w"] = R.weights((N, c1, 3, 3), 9 * c1, 4)
    rounded, _ = LR.launch_ref(dict(f, w_phase=True), o)["y"]
    x = nchw(o["x1"][..., :c1])
    want = torch.zeros(B, N, 2 * H, 2 * W, dtype=F64)
    for (py, px), wp in R.phase_weights(o["w"]).items():
        want[:, :, py::2, px::2] = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), w16(wp), d64(o["bias"]))
    close(rounded, rows(want))
    # a residual takes the launch out of the phase form (include/upk.h: plain epilogue only)
    assert not LR.phase_form(dict(f, w_phase=True, residual=True))


# ---------------------------------------------------------------------------------------------------- the by-products
def _stored(B, hw, N, ld, seed=21):
    return R.norm_input((B * hw, ld), seed, 1)


def test_layernorm_row_sums_and_groupnorm_partials_of_the_stored_output():
    B, H, W, N, ld = 2, 8, 4, 64, 72
    hw = H * W
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=32, ksize=1, stride=1, n_out=N, n_pad=N, ldy=ld, gn_groups=32, gn_stats_ws=True,
                  ln_rows_out=True)
    y = _stored(B, hw, N, ld)
    v = d64(y[:, :N])
    out = LR.byproduct_refs(f, {}, y, None, ln_slots=2)
    close(out["ln_rows"][0], torch.stack([v.sum(1), (v * v).sum(1)], 1))
    close(out["ln_rows"][1][:, 0], N * 2.0 ** -24 * v.abs().sum(1))
    out = LR.byproduct_refs(f, {}, y, None, gn_mode=2, gn_nblk=4, finalize=True)
    vb = v.reshape(B, 4, hw // 4, N)
    close(out["gn_part"][0], torch.stack([vb.sum(2), (vb * vb).sum(2)], 2))
    close(out["gn_part"][1][:, :, 0], (hw // 4) * 2.0 ** -24 * vb.abs().sum(2))
    vg = v.reshape(B, hw, 32, 2).permute(0, 2, 1, 3).reshape(B, 32, -1)
    close(out["gn_group"][0], torch.stack([vg.sum(2), (vg * vg).sum(2)], 2))
    assert torch.equal(out["gn_group"][0], LR.byproduct_refs(f, {}, y, None, gn_mode=1)["gn_group"][0])
    assert "gn_part" not in LR.byproduct_refs(f, {}, y, None, gn_mode=1)


@pytest.mark.parametrize("silu", [0, 1])
def test_normalising_reduce_against_group_norm(silu):
    B, H, W, N = 2, 4, 4, 128
    hw = H * W
    ops = {"gno_gamma": 1 + R.vector(N, 31), "gno_beta": R.vector(N, 32)}
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=32, ksize=1, stride=1, n_out=N, n_pad=N, ldy=N, gn_groups=32, gno_y=True,
                  gno_gamma=True, gno_beta=True, gno_eps=1e-5, gno_silu=silu, gno_ld=N)
    y = _stored(B, hw, N, N)
    want = F.group_norm(d64(y).reshape(B, hw, N).permute(0, 2, 1), 32, d64(ops["gno_gamma"]), d64(ops["gno_beta"]), 1e-5)
    want = (F.silu(want) if silu else want).permute(0, 2, 1).reshape(B * hw, N)
    ref, bound = LR.byproduct_refs(f, ops, y, None, gn_mode=3)["gno_y"]
    close(ref, want)
    # gno_skip_y: no y to read back, the GroupNorm of the reference output with the output's bound pushed through
    g = torch.Generator().manual_seed(1)
    dy = R.u16(d64(y))
    yr = d64(y) + dy * (torch.rand(y.shape, generator=g, dtype=F64) - 0.5)  # a reference the stored y is a rounding of
    ref2, bound2 = LR.byproduct_refs(dict(f, gno_skip_y=1), ops, None, (yr, dy), gn_mode=3)["gno_y"]
    assert float((ref2 - want).abs().max()) < 2e-2
    assert bool((bound2 > bound).all())
    # what the kernel normalises is its own fp16 y: its GroupNorm lies inside the bound around the reference's
    assert 0 < R.ratio(ref, ref2, bound2) <= 1


# ------------------------------------------------------------------------------------------------- what is not handled
def test_unhandled_fields_are_named():
    ok = LR.fields(batch=1, in_h=4, in_w=1, c1=32, ld1=32, x1=True, ksize=1, stride=1, n_out=16, n_pad=16, ldy=16)
    assert LR.unhandled(ok) == []
    assert any("flags" in s for s in LR.unhandled(dict(ok, flags=0x80)))
    assert any("ln_dim" in s for s in LR.unhandled(dict(ok, ln_colsum=True, ln_dim=28)))
    assert any("vt" in s for s in LR.unhandled(dict(ok, vt=True, residual=True, vt_from=16, vt_heads=1, vt_dhead=8)))
    assert "a_new_field" in LR.unhandled(dict(ok, a_new_field=0))
    assert set(LR.HANDLED) == {n for n, _ in L.ConvDesc._fields_}  # (a field added to the struct must be added to both)
    with pytest.raises(NotImplementedError, match="flags"):
        LR.launch_ref(dict(ok, flags=0x80), {})


# --------------------------------------------------------------------------------------------------------- sensitivity
@pytest.fixture(scope="module")
def bench_gemm():
    """A 1x1 launch of the headline's row count: B = 8, 32x32, M = 8192 (32 -> 32 channels keeps it cheap)."""
    B, H, W, c1, N = 8, 32, 32, 32, 32
    o = operands(B, H, W, c1, N)
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, ld1=c1 + 32, x1=True, ksize=1, stride=1, n_out=N, n_pad=N, bias=True, ldy=N)
    return f, o, LR.launch_ref(f, o)["y"]


def test_the_reference_passes_itself_and_a_correctly_rounded_output(bench_gemm):
    _, _, (ref, bound) = bench_gemm
    assert ref.shape == (8192, 32)
    assert R.ratio(ref, ref, bound) == 0
    assert R.ratio(R.q16(ref), ref, bound) <= 1


@pytest.mark.parametrize("m,n", [(0, 0), (8191, 31), (5000, 17), (1024, 16)])
def test_one_element_of_8192_rows_moved_by_4_ulp_fails(bench_gemm, m, n):
    _, _, (ref, bound) = bench_gemm
    for sign in (1, -1):
        got = R.q16(ref)
        got[m, n] += sign * 4 * R.u16(got[m, n])
        assert R.ratio(got, ref, bound) > 1


@pytest.fixture(scope="module")
def conv_case():
    """3x3, 64 | 32 -> 48 channels plus an appended 96-channel segment: K = 27 + 3 chunks of 32."""
    B, H, W, c1, c2, N = 2, 6, 5, 64, 32, 48
    o = operands(B, H, W, c1, N, ks=3, c2=c2, seg=(96, 0))
    f = LR.fields(batch=B, in_h=H, in_w=W, c1=c1, c2=c2, ld1=c1 + 32, ld2=c2, x1=True, x2=True, ksize=3, stride=1, n_out=N,
                  n_pad=N, bias=True, x3=True, c3=96, ld3=96, ldy=N)
    return f, o


def _a_matrix(f, o):
    x = torch.cat([nchw(o["x1"][..., :f["c1"]]), nchw(o["x2"])], 1)
    A = R.im2col(x, 3).reshape(-1, 9 * (f["c1"] + f["c2"]))
    A = torch.cat([A, d64(o["x3"]).reshape(A.shape[0], -1)], 1)
    W_ = torch.cat([R.wmat(w16(o["w"])), R.wmat(w16(o["w_app"]))], 1)
    return A, W_


@pytest.mark.parametrize("chunk", [0, 13, 26, 27, 29])
def test_one_k_chunk_missing_from_one_row_fails(conv_case, chunk):
    f, o = conv_case
    ref, bound = LR.launch_ref(f, o)["y"]
    A, W_ = _a_matrix(f, o)
    close(ref, A @ W_.t() + d64(o["bias"]))
    got, m = R.q16(ref), 37
    k = slice(32 * chunk, 32 * chunk + 32)
    got[m] = R.q16(ref[m] - A[m, k] @ W_[:, k].t())
    assert R.ratio(got, ref, bound) > 1


@pytest.mark.parametrize("splitk", [2, 5, LR.SPLITK_MAX])
def test_one_split_k_slice_missing_fails_under_the_split_k_bound(conv_case, splitk):
    f, o = conv_case
    ref, bound = LR.launch_ref(f, o, splitk=splitk)["y"]
    ref1, bound1 = LR.launch_ref(f, o)["y"]
    assert torch.equal(ref, ref1) and bool((bound >= bound1).all()) and bool((bound > bound1).any())
    assert R.ratio(R.q16(ref), ref, bound) <= 1
    A, W_ = _a_matrix(f, o)
    per = -(-30 // splitk)  # chunks per slice, as the library splits them
    for z in range(-(-30 // per)):
        k = slice(32 * per * z, min(32 * per * (z + 1), A.shape[1]))
        got = R.q16(ref - A[:, k] @ W_[:, k].t())
        assert R.ratio(got, ref, bound) > 1
        one_row = R.q16(ref)
        one_row[11] = got[11]
        assert R.ratio(one_row, ref, bound) > 1


def test_the_last_16_columns_missing_fails(conv_case, bench_gemm):
    for f, o, unwritten in ((*conv_case, 0.0), (*bench_gemm[:2], 7.0)):
        ref, bound = LR.launch_ref(f, o)["y"]
        got = R.q16(ref)
        got[:, -16:] = unwritten  # (what the buffer held before the launch)
        assert R.ratio(got, ref, bound) > 1
        got = R.q16(ref)
        got[-1, -16:] = unwritten  # ... in the last row alone
        assert R.ratio(got, ref, bound) > 1
