"""Lowers arch.* records + fp32 master weights to flat programs of libupk.so launches.

Design (MI355X-first, not a translation of the reference's nn.Module.forward chain):
  * activations live as token-major NHWC fp16 [B*H*W, C] for the whole network, so
    conv1x1 == Linear == GEMM and the reference's `b c h w <-> b (h w) c` rearranges
    (attention.py:256,259) and head split/merge copies (:178,192) do not exist;
  * channel concats (openaimodel.py:736) are never materialised — GroupNorm and the
    implicit-GEMM kernel read two sources; nearest-2x upsampling is folded into the
    following conv's addressing; bias / timestep-embedding add / residual / GEGLU / SiLU
    are GEMM epilogues;
  * shapes are static per (B, H, W, n_ctx): every buffer is allocated once, every launch
    descriptor is built once, and the per-step program is captured into ONE HIP graph that
    the sampler replays S times; the step index lives on the device (no per-step host
    work, no torch.full allocations as in ddim.py:189-192);
  * step-invariant work is hoisted out of the loop: the timestep-embedding MLP and all 22
    emb_layers projections for ALL S steps (one batched GEMM each) and the cross-attention
    K / V projections of the context.

PyTorch here = device allocator + stream handle only.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from . import knobs as K
from ._check import require
from .arch import UNetArch, VAEArch
from .emitter import Act, Emitter, Program  # noqa: F401  (re-exported: scripts and tests import them from here)
from .packing import (PW, PackedUNet, PackedVAEDecoder, PackedVAEEncoder, PackedVGG16, Packer, _rup,  # noqa: F401
                      geglu_rows_map, head_pad, pad_rows_map, qproj_pack, vgg16_convs)
from .tuning import TUNE_CACHE, TuneCache  # noqa: F401


class UNetPlan(Emitter):
    """Buffers + programs of one UNet for fixed (B, H, W, n_ctx, rows).

    rows = number of timestep-embedding rows: B in 'forward' mode (per-sample t, as
    UNetModel.forward takes them), S in 'sampler' mode (one row per DDIM step, shared by
    the batch: ddim.py:142 uses the same t for every sample)."""

    def __init__(self, ctx, packed: PackedUNet, B, H, W, n_ctx, rows, mode):
        super().__init__(ctx)
        require(mode in ("forward", "sampler"), "UNetPlan mode must be 'forward' or 'sampler'", ValueError)
        self.pk, self.arch = packed, packed.arch
        self.B, self.H, self.W, self.n_ctx, self.rows, self.mode = B, H, W, n_ctx, rows, mode
        a = self.arch
        mc, te = a.model_channels, a.time_embed_dim
        self.cin_pad = _rup(a.in_channels, 32)
        # inputs / outputs
        self.xin = Act(self.alloc(B * H * W, self.cin_pad, zero=True), B, H, W, a.in_channels)
        self.ctx32 = self.alloc(B * n_ctx, a.context_dim, dtype=torch.float32)
        self.ctx16 = Act(self.alloc(B * n_ctx, a.context_dim), 1, B * n_ctx, 1, a.context_dim)
        self.t_rows = self.alloc(rows, dtype=torch.float32)
        self.eps = self.alloc(B, a.out_channels, H, W, dtype=torch.float32)
        self.step = self.alloc(1, dtype=torch.int32, zero=True)
        self.gn_ws = self.alloc(max(64, ctx.groupnorm_ws_bytes(B, H * W) // 4), dtype=torch.float32)
        self.rowvecs = {}
        self.kv = {}
        self.sampler_states = {}  # (kind, guided) -> SamplerState (sampler_state())
        self._t_rows_key = None   # what t_rows holds (load_sampler_inputs); None: not a sampler's rows
        self.prep = Program(ctx)
        self.body = Program(ctx)
        self._emit_prep()
        self._emit_body()
        self.n_prefetch_links = self.link_weight_prefetch(self.body)

    # ---- step-invariant part
    def _emit_prep(self):
        P, a, w = self.prep, self.arch, self.pk.w
        mc, te, R = a.model_channels, a.time_embed_dim, self.rows
        lib, h, chk = self.lib, self.hctx, self._chk
        c32, c16 = self.ctx32, self.ctx16
        P.add(lambda s: chk(lib.upk_f32_to_f16(h, c32.data_ptr(), c32.shape[0], c32.shape[1], c16.t.data_ptr(),
                                               c16.ld, s)))
        temb = Act(self.alloc(R, mc), 1, R, 1, mc)
        tr = self.t_rows
        P.add(lambda s: chk(lib.upk_timestep_embed_f16(h, tr.data_ptr(), R, mc, 10000.0, temb.t.data_ptr(), mc, s)))
        # emb = Linear(SiLU(Linear(temb))) (openaimodel.py:506-511); every consumer applies SiLU
        # first (openaimodel.py:219), so SiLU(emb) is what is kept.
        h1 = self.conv(P, temb, w["time_embed.0"], flags=L.F_SILU)
        semb = self.conv(P, h1, w["time_embed.2"], flags=L.F_SILU)
        for Lr in a.all_layers():
            if Lr.kind == "res":
                rv = self.alloc(R, Lr.cout, dtype=torch.float32)
                self.conv(P, semb, w[Lr.name + ".emb_layers.1"], out_f32=rv)
                self.rowvecs[Lr.name] = rv
            elif Lr.kind == "st":
                heads, dp = Lr.heads, head_pad(Lr.dhead)
                hd = heads * dp
                vt_ld = _rup(self.n_ctx, 32)
                kc = Act(self.alloc(self.B * self.n_ctx, hd), 1, self.B * self.n_ctx, 1, hd)
                vtc = self.alloc(self.B, heads, dp, vt_ld, zero=True)
                self.conv(P, self.ctx16, w[Lr.name + ".transformer_blocks.0.attn2.kv"], out=kc,
                          vt=dict(t=vtc, heads=heads, dhead=dp, ld=vt_ld, tokens=self.n_ctx, **{"from": hd}))
                self.kv[Lr.name] = (kc, vtc, vt_ld)

    # ---- per-step part
    def _rv(self, name):
        rv = self.rowvecs[name]
        if self.mode == "sampler":
            return dict(rowvec=rv, rv_bs=0, rv_ss=rv.shape[1], step=self.step)
        return dict(rowvec=rv, rv_bs=rv.shape[1], rv_ss=0, step=None)

    def _res(self, P, Lr, x, skip):
        w, v = self.pk.w, self.pk.v
        n = Lr.name
        if skip is not None and (skip.H, skip.W, skip.B) != (x.H, x.W, x.B):
            # the reference fails in torch.cat here (openaimodel.py:736) when H or W is not a
            # multiple of 2^(levels-1); fail just as loudly instead of reading mismatched rows
            raise ValueError("UNet skip connection %dx%d does not match the decoder feature map %dx%d at %s: "
                             "latent height and width must be multiples of %d" % (
                                 skip.H, skip.W, x.H, x.W, n, 2 ** (len(self.arch.channel_mult) - 1)))
        g1, b1 = v[n + ".in_layers.0"]
        hh = self.conv(P, x, w[n + ".in_layers.2"], x2=skip, gn=(g1, b1, 1e-5, True, self.gn_ws), gn_stats=True,
                       **self._rv(n))
        gn2 = (*v[n + ".out_layers.0"], 1e-5, True, self.gn_ws, True)  # (hh has no reader but this GroupNorm)
        if Lr.cin != Lr.cout:
            if self.fold_skip(hh, w[n + ".out_layers.3"], w[n + ".skip_connection"], x, skip):
                # skip projection as an appended K segment of the second conv: one launch, no residual round trip
                return self.conv(P, hh, w[n + ".out_layers.3+skip"], append=(x, skip), gn=gn2, gn_stats=True)
            sk = self.conv(P, x, w[n + ".skip_connection"], x2=skip)
        else:
            require(skip is None, "decoder ResBlock without channel change got a skip tensor", RuntimeError)
            sk = x
        return self.conv(P, hh, w[n + ".out_layers.3"], residual=sk, gn=gn2, gn_stats=True)

    def _st(self, P, Lr, x):
        w, v = self.pk.w, self.pk.v
        n = Lr.name
        t = n + ".transformer_blocks.0"
        B, HW, M = x.B, x.H * x.W, x.M
        heads, dh = Lr.heads, Lr.dhead
        dp = head_pad(dh)
        hd = heads * dp
        scale = dh ** -0.5
        # self-attention
        qk = Act(self.alloc(M, 2 * hd), B, x.H, x.W, 2 * hd)
        vt_ld = _rup(HW, 32)
        vt = self.alloc(B, heads, dp, vt_ld, zero=True)
        t0 = None
        if self.head_block_ok(x, t, heads, dp, qk, vt_ld):
            t0 = self.head_block(P, x, n, t, heads, dp, qk, vt, vt_ld, (*v[n + ".norm"], 1e-6, self.gn_ws))
        if t0 is None:
            t0 = self.conv(P, x, w[n + ".proj_in"], gn=(*v[n + ".norm"], 1e-6, False, self.gn_ws))
            self.ln_linear(P, t0, t + ".attn1.qkv", t + ".norm1", out=qk,  # norm1 -> q|k|v (attention.py:203,212)
                           vt=dict(t=vt, heads=heads, dhead=dp, ld=vt_ld, tokens=HW, **{"from": 2 * hd}))
        a1 = Act(self.alloc(M, hd), B, x.H, x.W, hd)
        self.attention(P, qk.t, 2 * hd, HW * 2 * hd, qk.t[:, hd:], 2 * hd, HW * 2 * hd, vt, vt_ld, a1.t, hd, HW * hd,
                       B, heads, HW, HW, dp, scale)
        P.attn_flops += 4 * B * heads * HW * HW * dh
        # cross-attention over the (precomputed) context K / V
        kc, vtc, cld = self.kv[n]
        t2 = self.cross_block(P, a1, t0, t, kc, vtc, cld, heads, dp, scale)
        if t2 is not None:
            return self._st_ff(P, Lr, x, t2)
        t1 = self.conv(P, a1, w[t + ".attn1.to_out"], residual=t0)
        a2 = Act(self.alloc(M, hd), B, x.H, x.W, hd)
        # (pays while there are >= 2 waves per SIMD to hide a wave's serial projection -> scores chain: 32x32 level
        # 16 -> 12 us per block; at 16x16 (1 wave per SIMD, 4x the weight slice per wave) 16 -> 18 us)
        if (K.QPROJ_FUSE and (t + ".attn2.qproj") in w and t1.C == t1.ld and dp == 32
                and B * heads * ((HW + 31) // 32) >= 2048):
            # norm2 -> to_q inside the attention kernel (include/upk.h upk_attention_qproj_f16): no q GEMM, no q tensor
            wq, wu, wb = w[t + ".attn2.qproj"]
            fn, hh, chk = self.lib.upk_attention_qproj_f16, self.hctx, self._chk
            qa = (t1.t.data_ptr(), t1.ld, HW * t1.ld, t1.C, t1.C, 1e-5, wq.data_ptr(), wu.data_ptr(), wb.data_ptr(),
                  kc.t.data_ptr(), hd, self.n_ctx * hd, vtc.data_ptr(), cld, a2.t.data_ptr(), hd, HW * hd, B, heads, HW,
                  self.n_ctx, dp, float(scale))
            P.attn.append(dict(kind="qproj", ldx=t1.ld, xbs=HW * t1.ld, cq=t1.C, ln_dim=t1.C, eps=1e-5, ldk=hd,
                               kbs=self.n_ctx * hd, vt_ld=cld, ldo=hd, obs=HW * hd, B=B, heads=heads, nq=HW, nkv=self.n_ctx,
                               d=dp, scale=float(scale)))
            P.add(lambda s: chk(fn(hh, *qa, s)), t1, wq, wu, wb, kc, vtc, a2, cls="attention",
                  label="attn+q B%d h%d nq%d nkv%d d%d C%d" % (B, heads, HW, self.n_ctx, dp, t1.C))
            P.igemm_flops += 2 * M * heads * dh * t1.C
        else:
            q2 = self.ln_linear(P, t1, t + ".attn2.q", t + ".norm2")
            self.attention(P, q2.t, hd, HW * hd, kc.t, hd, self.n_ctx * hd, vtc, cld, a2.t, hd, HW * hd, B, heads, HW,
                           self.n_ctx, dp, scale)
        P.attn_flops += 4 * B * heads * HW * self.n_ctx * dh
        t2 = self.conv(P, a2, w[t + ".attn2.to_out"], residual=t1)
        return self._st_ff(P, Lr, x, t2)

    def _st_ff(self, P, Lr, x, t2):
        """GEGLU feed-forward of the block + the transformer's proj_out (attention.py:261, 330-336)."""
        w = self.pk.w
        n = Lr.name
        t = n + ".transformer_blocks.0"
        fused = self.geglu_mlp(P, t2, x, w[t + ".ff.geglu_ln"], w[n + ".ff.out+proj_out"])
        if fused is not None:
            return fused
        ff = self.ln_linear(P, t2, t + ".ff.geglu", t + ".norm3", flags=L.F_GEGLU)
        if self.fold_ff_out(ff, t2, w[t + ".ff.out"]):
            return self.conv(P, ff, w[n + ".ff.out+proj_out"], residual=x, append=(t2, None), gn_stats=True)
        t3 = self.conv(P, ff, w[t + ".ff.out"], residual=t2)
        return self.conv(P, t3, w[n + ".proj_out"], residual=x, gn_stats=True)

    def _layers(self, P, layers, x, skip=None):
        w = self.pk.w
        for Lr in layers:
            if Lr.kind == "conv":
                x = self.conv(P, x, w[Lr.name], gn_stats=True)
            elif Lr.kind == "res":
                x = self._res(P, Lr, x, skip)
                skip = None
            elif Lr.kind == "st":
                x = self._st(P, Lr, x)
            elif Lr.kind == "down":
                x = self.conv(P, x, w[Lr.name + ".op"], stride=2, gn_stats=True)
            elif Lr.kind == "up":
                x = self.conv(P, x, w[Lr.name + ".conv"], flags=L.F_UPSAMPLE2X, gn_stats=True)
        return x

    def _emit_body(self):
        P, a = self.body, self.arch
        hs = []
        x = self.xin
        self.taps = {}  # block name -> Act (debug / parity tests)
        for i, blk in enumerate(a.input_blocks):
            x = self._layers(P, blk, x)
            hs.append(x)
            self.taps["input_blocks.%d" % i] = x
        x = self._layers(P, a.middle_block, x)
        self.taps["middle_block"] = x
        for i, blk in enumerate(a.output_blocks):
            x = self._layers(P, blk, x, skip=hs.pop())
            self.taps["output_blocks.%d" % i] = x
        self.conv(P, x, self.pk.w["out.2"], nchw_out=self.eps, gn=(*self.pk.v["out.0"], 1e-5, True, self.gn_ws))

    # ---- host-facing helpers
    def sampler_state(self, kind, channels, cfg=False):
        """The plan's SamplerState of (kind, guided or not), made on first use: what a sampler's fast path runs its chain on."""
        st = self.sampler_states.get((kind, bool(cfg)))
        if st is None:
            st = self.sampler_states[(kind, bool(cfg))] = SamplerState(self, channels, kind, cfg)
        return st

    @property
    def _sampler_state(self):
        """The unguided DDIM state, under the name the benchmark reads after a run; no attribute before the first one."""
        try:
            return self.sampler_states[("ddim", False)]
        except KeyError:
            raise AttributeError("_sampler_state") from None

    def close(self):
        """Drops every sampler state of the plan (sampler_states) and releases what each holds outside the plan's buffer
        list: its captured graphs and the DDIM edit buffers."""
        while self.sampler_states:
            self.sampler_states.popitem()[1].close()

    def rows_fresh(self, rows_key):
        """Whether load_sampler_inputs would upload the timestep rows of `rows_key` (a sampler's lock rule asks first)."""
        return self._t_rows_key != rows_key

    def load_sampler_inputs(self, x, c_concat, c_cross, in_channels, rows_key, t_rows):
        """The per-call uploads of a sampler fast path: the latent (channels [0, C) of the stem input), the concat
        conditioning behind it, the context, and the timestep rows when `rows_key` differs from what the plan holds
        (one buffer shared by every sampler state of the plan)."""
        C = x.shape[1]
        self.load_x_nchw(x, 0, 0)
        ncat = 0
        if c_concat is not None:
            ncat = c_concat.shape[1]
            self.load_x_nchw(c_concat, C, self.cin_pad)
        require(C + ncat == in_channels, lambda: "latent %d + concat %d != UNet in_channels %d" % (C, ncat, in_channels),
                ValueError)
        self.load_context(c_cross)
        if self.rows_fresh(rows_key):
            self.t_rows.copy_(torch.as_tensor(t_rows))
            self._t_rows_key = rows_key

    def load_context(self, context):
        """context: [B, n_ctx, context_dim] tensor (any float dtype / device)."""
        require(tuple(context.shape) == (self.B, self.n_ctx, self.arch.context_dim), lambda: "context shape %s != plan %s" % (tuple(context.shape), (self.B, self.n_ctx, self.arch.context_dim)), ValueError)
        self.ctx32.copy_(context.reshape(self.B * self.n_ctx, -1).to(self.dev, torch.float32), non_blocking=True)

    def load_x_nchw(self, x, c_off=0, zero_pad_to=0):
        """fp32 NCHW [B, c, H, W] -> channels [c_off, c_off + c) of the stem input."""
        x = x.to(self.dev, torch.float32).contiguous()
        require(x.shape[0] == self.B and tuple(x.shape[2:]) == (self.H, self.W), lambda: "stem input %s does not match the plan (B=%d, %dx%d)" % (tuple(x.shape), self.B, self.H, self.W), ValueError)
        self.ctx.nchw_to_nhwc(x, self.B, x.shape[1], self.H * self.W, self.xin.t, self.xin.ld, c_off, zero_pad_to, 1.0)


class VAEDecodePlan(Emitter):
    """decode_first_stage (ddpm.py:771-829 plain branch): z / scale_factor ->
    post_quant_conv -> Decoder (model.py:535-568) -> fp32 NCHW image."""

    def __init__(self, ctx, packed: PackedVAEDecoder, B, h, w, scale_factor):
        super().__init__(ctx)
        self.pk, self.arch = packed, packed.arch
        a = self.arch
        self.B, self.h, self.w = B, h, w
        f = a.factor
        self.z = self.alloc(B, a.embed_dim, h, w, dtype=torch.float32)
        self.img = self.alloc(B, a.out_ch, h * f, w * f, dtype=torch.float32)
        self.gn_ws = self.alloc(max(64, ctx.groupnorm_ws_bytes(B, h * f * w * f) // 4), dtype=torch.float32)
        self.prog = Program(ctx)
        P, W_, V_ = self.prog, packed.w, packed.v
        zin = Act(self.alloc(B * h * w, _rup(a.embed_dim, 32), zero=True), B, h, w, a.embed_dim)
        lib, hh, chk, z = self.lib, self.hctx, self._chk, self.z
        inv = 1.0 / float(scale_factor)
        P.add(lambda s: chk(lib.upk_nchw_f32_to_nhwc_f16(hh, z.data_ptr(), B, a.embed_dim, h * w, zin.t.data_ptr(),
                                                         zin.ld, 0, 0, inv, s)))
        x = self.conv(P, zin, W_["post_quant_conv"],
                      out=Act(self.alloc(B * h * w, _rup(a.z_channels, 32), zero=True), B, h, w, a.z_channels))
        for Lr in a.decoder:
            n = Lr.name
            if Lr.kind == "conv":
                x = self.conv(P, x, W_[n], gn_stats=K.vae_gn_byproduct(x.M))
            elif Lr.kind == "resnet":
                h1 = self.conv(P, x, W_[n + ".conv1"], gn=(*V_[n + ".norm1"], 1e-6, True, self.gn_ws), gn_stats=K.vae_gn_byproduct(x.M))
                sk = self.conv(P, x, W_[n + ".nin_shortcut"]) if Lr.cin != Lr.cout else x
                x = self.conv(P, h1, W_[n + ".conv2"], residual=sk, gn=(*V_[n + ".norm2"], 1e-6, True, self.gn_ws),
                              gn_stats=K.vae_gn_byproduct(x.M))
            elif Lr.kind == "attn":
                c, HW = Lr.ch, x.H * x.W
                xn = self.groupnorm(P, x, *V_[n + ".norm"], 1e-6, False, self.gn_ws)
                qk = Act(self.alloc(x.M, 2 * c), x.B, x.H, x.W, 2 * c)
                vt_ld = _rup(HW, 32)
                vt = self.alloc(x.B, 1, c, vt_ld, zero=True)
                self.conv(P, xn, W_[n + ".qkv"], out=qk,
                          vt=dict(t=vt, heads=1, dhead=c, ld=vt_ld, tokens=HW, **{"from": 2 * c}))
                ao = Act(self.alloc(x.M, c), x.B, x.H, x.W, c)
                self.attention(P, qk.t, 2 * c, HW * 2 * c, qk.t[:, c:], 2 * c, HW * 2 * c, vt, vt_ld, ao.t, c, HW * c,
                               x.B, 1, HW, HW, c, int(c) ** -0.5)
                x = self.conv(P, ao, W_[n + ".proj_out"], residual=x, gn_stats=K.vae_gn_byproduct(x.M))
            elif Lr.kind == "upconv":
                x = self.conv(P, x, W_[n], flags=L.F_UPSAMPLE2X)
            elif Lr.kind == "norm_out":
                x = self.groupnorm(P, x, *V_[n], 1e-6, True, self.gn_ws)
            elif Lr.kind == "conv_out":
                self.conv(P, x, W_[n], nchw_out=self.img)
        self.graph = None

    def run(self, z):
        z = z.to(self.dev, torch.float32).contiguous()
        require(tuple(z.shape) == tuple(self.z.shape), lambda: repr((z.shape, self.z.shape)), ValueError)
        self.z.copy_(z)
        self.prog.run()
        return self.img


class VAEEncodePlan(Emitter):
    """AutoencoderKL.encode (autoencoder.py:324-328): Encoder (model.py:434-459) -> quant_conv ->
    posterior moments [B, 2*embed_dim, h, w] fp32 NCHW.  Same kernels as the decoder; the
    stride-2 Downsample uses the asymmetric (0,1,0,1) padding mode of the implicit GEMM."""

    def __init__(self, ctx, packed: PackedVAEEncoder, B, H, W):
        super().__init__(ctx)
        self.pk, self.arch = packed, packed.arch
        a = self.arch
        f = a.factor
        require(H % f == 0 and W % f == 0, lambda: "image size must be a multiple of %d" % f, ValueError)
        self.x = self.alloc(B, a.in_channels, H, W, dtype=torch.float32)
        self.moments = self.alloc(B, 2 * a.embed_dim, H // f, W // f, dtype=torch.float32)
        self.gn_ws = self.alloc(max(64, ctx.groupnorm_ws_bytes(B, H * W) // 4), dtype=torch.float32)
        self.prog = Program(ctx)
        P, W_, V_ = self.prog, packed.w, packed.v
        xin = Act(self.alloc(B * H * W, _rup(a.in_channels, 32), zero=True), B, H, W, a.in_channels)
        lib, hh, chk, xs = self.lib, self.hctx, self._chk, self.x
        P.add(lambda s: chk(lib.upk_nchw_f32_to_nhwc_f16(hh, xs.data_ptr(), B, a.in_channels, H * W,
                                                         xin.t.data_ptr(), xin.ld, 0, 0, 1.0, s)))
        x = xin
        for Lr in a.encoder:
            n = Lr.name
            if Lr.kind == "conv":
                x = self.conv(P, x, W_[n], gn_stats=K.vae_gn_byproduct(x.M))
            elif Lr.kind == "resnet":
                h1 = self.conv(P, x, W_[n + ".conv1"], gn=(*V_[n + ".norm1"], 1e-6, True, self.gn_ws), gn_stats=K.vae_gn_byproduct(x.M))
                sk = self.conv(P, x, W_[n + ".nin_shortcut"]) if Lr.cin != Lr.cout else x
                x = self.conv(P, h1, W_[n + ".conv2"], residual=sk, gn=(*V_[n + ".norm2"], 1e-6, True, self.gn_ws),
                              gn_stats=K.vae_gn_byproduct(x.M))
            elif Lr.kind == "attn":
                c, HW = Lr.ch, x.H * x.W
                xn = self.groupnorm(P, x, *V_[n + ".norm"], 1e-6, False, self.gn_ws)
                qk = Act(self.alloc(x.M, 2 * c), x.B, x.H, x.W, 2 * c)
                vt_ld = _rup(HW, 32)
                vt = self.alloc(x.B, 1, c, vt_ld, zero=True)
                self.conv(P, xn, W_[n + ".qkv"], out=qk,
                          vt=dict(t=vt, heads=1, dhead=c, ld=vt_ld, tokens=HW, **{"from": 2 * c}))
                ao = Act(self.alloc(x.M, c), x.B, x.H, x.W, c)
                self.attention(P, qk.t, 2 * c, HW * 2 * c, qk.t[:, c:], 2 * c, HW * 2 * c, vt, vt_ld, ao.t, c, HW * c,
                               x.B, 1, HW, HW, c, int(c) ** -0.5)
                x = self.conv(P, ao, W_[n + ".proj_out"], residual=x)
            elif Lr.kind == "downconv":
                x = self.conv(P, x, W_[n], stride=2, flags=L.F_PAD_ASYM)
            elif Lr.kind == "norm_out":
                x = self.groupnorm(P, x, *V_[n], 1e-6, True, self.gn_ws)
            elif Lr.kind == "conv_out":
                x = self.conv(P, x, W_[n], out=Act(self.alloc(x.M, _rup(Lr.cout, 32), zero=True), x.B, x.H, x.W,
                                                   Lr.cout))
        self.conv(P, x, W_["quant_conv"], nchw_out=self.moments)

    def run(self, img):
        img = img.to(self.dev, torch.float32).contiguous()
        require(tuple(img.shape) == tuple(self.x.shape), lambda: repr((img.shape, self.x.shape)), ValueError)
        self.x.copy_(img)
        self.prog.run()
        return self.moments


class LpipsPlan(Emitter):
    """lpips.LPIPS(net='vgg') (include/upk.h) for `pairs` picture pairs of H x W: scaling layer -> 13 x (conv
    3x3 + ReLU, a max-pool in front of slices 2..5) -> the five tap distances, out [pairs, 5] fp32.

    The 2 * pairs pictures live in ONE NHWC batch, the two pictures of a pair next to each other (2 i, 2 i + 1): the input
    pass, the 13 ReLU (+ pool) passes and the five tap kernels each cover the whole batch in one call.  The convolutions are
    upk_conv2d_nhwc_f16 as it stands with the cost model's tile / split-K choice, launched PER PAIR (batch 2): that choice
    depends on the launch's row count, and different tiles or split-K factors round differently, so a launch over the whole
    batch would make a pair's value depend on how many pairs share its pass.  Per pair the launch shape is a function of
    (H, W) alone, and so are the bits of the result."""

    def __init__(self, ctx, packed: PackedVGG16, pairs, H, W):
        super().__init__(ctx)
        require(pairs >= 1 and min(H, W) >= 16, "LPIPS needs min(H, W) >= 16 (the fifth tap must have a pixel), got %d x %d" % (H, W),
                ValueError)
        self.pk, self.pairs, self.H, self.W = packed, pairs, H, W
        B = 2 * pairs
        self.xin = Act(self.alloc(B * H * W, 32), B, H, W, 3)
        self.out = self.alloc(pairs, 5, dtype=torch.float32)
        self.ws = self.alloc(max(16, max(ctx.lpips_ws_bytes(pairs, (H >> l) * (W >> l), c)
                                         for l, c in enumerate((64, 128, 256, 512, 512)))), dtype=torch.uint8)
        self.prog = P = Program(ctx)
        self.n_relu = 0
        convs = vgg16_convs()
        x = self.xin
        for j, (s, i, cin, cout) in enumerate(convs):
            pw = packed.w["net.slice%d.%d" % (s, i)]
            y = Act(self.alloc(x.M, cout), x.B, x.H, x.W, cout)
            hw = x.H * x.W
            for k in range(pairs):  # (per pair: see the class docstring)
                rows = slice(2 * k * hw, 2 * (k + 1) * hw)
                self.conv(P, Act(x.t[rows], 2, x.H, x.W, x.C), pw, out=Act(y.t[rows], 2, x.H, x.W, cout))
            tap = j + 1 == len(convs) or convs[j + 1][0] != s
            pooled = None
            if tap and j + 1 < len(convs):
                pooled = Act(self.alloc(x.B * (x.H // 2) * (x.W // 2), cout), x.B, x.H // 2, x.W // 2, cout)
            self._relu(P, y, pooled)
            if tap:
                self._layer(P, y, s - 1)
            x = pooled if pooled is not None else y

    def _relu(self, P, y, pooled):
        fn, h, chk = self.lib.upk_relu_pool_nhwc_f16, self.hctx, self._chk
        a = (y.t.data_ptr(), y.ld, y.B, y.H, y.W, y.C, pooled.t.data_ptr() if pooled is not None else None,
             pooled.ld if pooled is not None else 0)
        P.add(lambda s: chk(fn(h, *a, s)), y, pooled, cls="other", label="relu%s M%d C%d" % ("+pool" if pooled is not None else "", y.M, y.C))
        self.n_relu += 1

    def _layer(self, P, y, l):
        fn, h, chk = self.lib.upk_lpips_layer_f16, self.hctx, self._chk
        hw, w = y.H * y.W, self.pk.lin[l]
        a = (y.t.data_ptr(), y.t[hw:].data_ptr(), y.ld, 2 * hw * y.ld, self.pairs, hw, y.C, w.data_ptr(), l,
             self.out.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        P.add(lambda s: chk(fn(h, *a, s)), y, w, cls="other", label="lpips tap %d hw%d C%d" % (l, hw, y.C))
        P.n_launch += 1  # partial sums + final pass

    def run(self, src0, src1, f32, normalize):
        """src0, src1: the two sides of the pairs, (tensor, row pitch, sample stride) as upk_lpips_input_f16 takes them.
        Returns the plan's own [pairs, 5] buffer (overwritten by the next run)."""
        hw32 = self.H * self.W * 32
        for side, (t, pitch, ss) in enumerate((src0, src1)):
            self.ctx.lpips_input(t, f32, pitch, ss, self.pairs, self.H, self.W, normalize, self.pk.shift_scale,
                                 self.xin.t[side * self.H * self.W:], 2 * hw32)
        self.prog.run()
        return self.out


class _Map:
    """A [B * H * W, C] window of an fp16 activation buffer: channels off .. off + C of rows `ld` apart."""
    __slots__ = ("t", "off", "B", "H", "W", "C")

    def __init__(self, t, off, B, H, W, C):
        self.t, self.off, self.B, self.H, self.W, self.C = t, off, B, H, W, C

    @property
    def ld(self):
        return self.t.shape[1]

    @property
    def ptr(self):
        return self.t.data_ptr() + 2 * self.off


class FidPlan(Emitter):
    """pytorch_fid's InceptionV3 (include/upk.h) for `pictures` pictures of H x W: upk_fid_input_f16 (bilinear
    resize to 299 x 299 when `resize`) -> 94 upk_conv2d_rect_f16 launches, 4 + 9 upk_pool3_nhwc_f16 launches (every branch
    writes its channel slice of the block's output: no concat pass) -> upk_avgpool_global_f32, out [pictures, 2048] fp32.

    All pictures share every launch: the convolution's tile and K walk do not depend on the batch (include/upk.h), so a
    picture's bits do not either.  Buffers of a finished block are handed to the next one (the launches are in stream order)."""

    def __init__(self, ctx, packed, pictures, H, W, resize):
        super().__init__(ctx)
        from .packing import FID_DIMS, INCEPTION_A, INCEPTION_C, INCEPTION_E, inception_units
        self.pk, self.B, self.H, self.W, self.resize = packed, pictures, H, W, bool(resize)
        self.units = inception_units()
        self.in_h, self.in_w = (299, 299) if resize else (H, W)
        require(pictures >= 1 and min(self.in_h, self.in_w) >= 75, "InceptionV3 without resizing needs min(H, W) >= 75 (Mixed_7a "
                "must leave a pixel), got %d x %d" % (H, W), ValueError)
        self._free, self._live = {}, []
        self.prog = P = Program(ctx)
        self.xin = self._new(self.in_h, self.in_w, 3)
        self.out = self.alloc(pictures, FID_DIMS, dtype=torch.float32)
        MAX, AVG = L.POOL_MAX, L.POOL_AVG
        conv, pool, new, sl, give = self._conv, self._pool, self._new, self._slice, self._give
        x = self.xin
        for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = conv(P, x, name)
        x = pool(P, x, MAX, 2)
        x = conv(P, conv(P, x, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
        x = pool(P, x, MAX, 2)
        for n, cin, pf in INCEPTION_A:
            y = new(x.H, x.W, 224 + pf)
            conv(P, x, n + ".branch1x1", sl(y, 0, 64))
            conv(P, conv(P, x, n + ".branch5x5_1"), n + ".branch5x5_2", sl(y, 64, 64))
            conv(P, conv(P, conv(P, x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2"), n + ".branch3x3dbl_3", sl(y, 128, 96))
            conv(P, pool(P, x, AVG, 1), n + ".branch_pool", sl(y, 224, pf))
            x = give(y)
        n = "Mixed_6a"
        y = new((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1, 768)
        conv(P, x, n + ".branch3x3", sl(y, 0, 384))
        conv(P, conv(P, conv(P, x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2"), n + ".branch3x3dbl_3", sl(y, 384, 96))
        pool(P, x, MAX, 2, sl(y, 480, 288))
        x = give(y)
        for n, c7 in INCEPTION_C:
            y = new(x.H, x.W, 768)
            conv(P, x, n + ".branch1x1", sl(y, 0, 192))
            t = conv(P, conv(P, x, n + ".branch7x7_1"), n + ".branch7x7_2")
            conv(P, t, n + ".branch7x7_3", sl(y, 192, 192))
            t = conv(P, x, n + ".branch7x7dbl_1")
            for k in (2, 3, 4):
                t = conv(P, t, n + ".branch7x7dbl_%d" % k)
            conv(P, t, n + ".branch7x7dbl_5", sl(y, 384, 192))
            conv(P, pool(P, x, AVG, 1), n + ".branch_pool", sl(y, 576, 192))
            x = give(y)
        n = "Mixed_7a"
        y = new((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1, 1280)
        conv(P, conv(P, x, n + ".branch3x3_1"), n + ".branch3x3_2", sl(y, 0, 320))
        t = conv(P, x, n + ".branch7x7x3_1")
        for k in (2, 3):
            t = conv(P, t, n + ".branch7x7x3_%d" % k)
        conv(P, t, n + ".branch7x7x3_4", sl(y, 320, 192))
        pool(P, x, MAX, 2, sl(y, 512, 768))
        x = give(y)
        for n, cin, kind in INCEPTION_E:
            y = new(x.H, x.W, 2048)
            conv(P, x, n + ".branch1x1", sl(y, 0, 320))
            t = conv(P, x, n + ".branch3x3_1")
            conv(P, t, n + ".branch3x3_2a", sl(y, 320, 384))
            conv(P, t, n + ".branch3x3_2b", sl(y, 704, 384))
            t = conv(P, conv(P, x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2")
            conv(P, t, n + ".branch3x3dbl_3a", sl(y, 1088, 384))
            conv(P, t, n + ".branch3x3dbl_3b", sl(y, 1472, 384))
            conv(P, pool(P, x, AVG if kind == "avg" else MAX, 1), n + ".branch_pool", sl(y, 1856, 192))
            x = give(y)
        fn, h, chk = self.lib.upk_avgpool_global_f32, self.hctx, self._chk
        a = (x.ptr, x.ld, x.B, x.H * x.W, x.C, self.out.data_ptr())
        P.add(lambda s: chk(fn(h, *a, s)), x.t, self.out, cls="other", label="global mean hw%d C%d" % (x.H * x.W, x.C))
        self.last = x

    # ---- buffers: a block's temporaries and its input go back to the pool when the block is emitted
    def _new(self, H, W, C):
        rows, ld = self.B * H * W, _rup(C, 32)
        require(rows * ld < 2 ** 31, "FidPlan: a %d x %d map of %d pictures and %d channels passes 2^31 elements; lower "
                "pictures_per_pass" % (H, W, self.B, C), ValueError)
        lst = self._free.get((rows, ld))
        t = lst.pop() if lst else self.alloc(rows, ld)
        self._live.append(t)
        return _Map(t, 0, self.B, H, W, C)

    def _give(self, keep):
        """End of a block: every buffer taken since the last call except `keep`'s is free again (the block's input and its
        temporaries are dead once its launches are in the stream; whoever takes them next writes behind those launches)."""
        for t in self._live:
            if t is not keep.t:
                self._free.setdefault(tuple(t.shape), []).append(t)
        self._live = [keep.t]
        return keep

    @staticmethod
    def _slice(y, off, c):
        return _Map(y.t, y.off + off, y.B, y.H, y.W, c)

    def _conv(self, P, x, name, dst=None):
        cin, cout, kh, kw, s, ph, pw_ = self.units[name]
        pw = self.pk.u[name]
        Ho, Wo = (x.H + 2 * ph - kh) // s + 1, (x.W + 2 * pw_ - kw) // s + 1
        require(x.off == 0 and x.C == cin and pw.k_packed <= x.ld, "%s reads %d channels, its source has %d" % (name, cin, x.C), ValueError)
        if dst is None:
            dst = self._new(Ho, Wo, cout)
        require((dst.H, dst.W) == (Ho, Wo) and dst.C == cout and dst.off + pw.n_out <= dst.ld, "%s: destination %dx%dx%d does not "
                "take its %dx%dx%d output" % (name, dst.H, dst.W, dst.C, Ho, Wo, cout), ValueError)
        fn, h, chk = self.lib.upk_conv2d_rect_f16, self.hctx, self._chk
        a = (x.ptr, x.ld, x.B, x.H, x.W, pw.k_packed, kh, kw, s, ph, pw_, pw.w.data_ptr(), pw.n_out, pw.n_pad, pw.bias.data_ptr(),
             1, dst.ptr, dst.ld)
        P.add(lambda st: chk(fn(h, *a, st)), x.t, dst.t, pw, cls="igemm_k%d" % max(kh, kw), label="%s M%d" % (name, x.B * Ho * Wo))
        fl = 2 * x.B * Ho * Wo * cout * cin * kh * kw
        P.igemm_flops += fl
        P.flops[-1] = fl
        return dst

    def _pool(self, P, x, mode, stride, dst=None):
        Ho, Wo = (x.H, x.W) if stride == 1 else ((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1)
        if dst is None:
            dst = self._new(Ho, Wo, x.C)
        fn, h, chk = self.lib.upk_pool3_nhwc_f16, self.hctx, self._chk
        a = (x.ptr, x.ld, x.B, x.H, x.W, x.C, mode, stride, dst.ptr, dst.ld)
        P.add(lambda st: chk(fn(h, *a, st)), x.t, dst.t, cls="other", label="pool3 %s s%d M%d C%d" % (
            "avg" if mode == L.POOL_AVG else "max", stride, x.B * Ho * Wo, x.C))
        return dst

    def run(self, src, f32, pitch, ss, normalize):
        """src: the pictures as upk_fid_input_f16 takes them.  Returns the plan's own [pictures, 2048] buffer (overwritten by
        the next run)."""
        self.ctx.fid_input(src, f32, pitch, ss, self.B, self.H, self.W, self.in_h, self.in_w, normalize, self.xin.t,
                           self.in_h * self.in_w * 32)
        self.prog.run()
        return self.out


# ====================================================================== sampler step graph
class SamplerState:
    """Device state of one sampler's chain on a sampler-mode UNetPlan: latent x (fp32 NCHW), pred_x0, the per-step
    coefficient / noise tables and the captured step graphs (UNet body -> the kind's step kernel, which also advances
    the device-side step counter).  A plan keeps its states in UNetPlan.sampler_states (UNetPlan.sampler_state()).

    kind: which step kernel a graph ends in, and `variant` (set_variant(), before graph() / launch()) which form of it the
    next launches run; each variant has graphs of its own.
      "ddim": plan rows = steps.  None = upk_ddim_step_f32 / _cfg_f32; "plain" = upk_ddim_step_edit_f32 without a mask
              (chains that start inside the schedule: decode, a shortened `timesteps`); "masked" = the same kernel with the
              keep table and the mask (inpainting).  A chain that starts at loop position k > 0 only presets plan.step to
              k: timestep rows and coefficients stay the S-row tables.
      "plms": one PLMS model evaluation, upk_plms_step_f32 (plan rows = evaluations = steps + 1; eps history `hist`).
      "ddpm": one DDPM ancestral step, upk_ddpm_step_f32 (plan rows = timesteps of the chain, coefficient rows of 8, no
              guidance); (flags, masked) = its DDPM_* flags and whether it blends q_sample(x0) under a mask.  The posterior
              noise table [rows, n] is always there, and a masked chain adds the q_sample noise table, x0 and the expanded
              mask: at B = 8, 32x24 and 1000 steps each table is 1000 * 24576 * 4 B = 98 MB.
      "dpm":  one DPM-Solver++(2M) step, upk_dpmpp_2m_step_f32 (coefficient rows of 8); x0_old [n] is the data prediction of
              the step before, which the kernel reads on second-order rows only, so nothing initialises it.
      "unipc": one UniPC model evaluation, upk_unipc_step_f32 (coefficient rows of 12): the corrector of the step that led to
              this point and the predictor of the next.  hist [3, n] is the ring of data predictions and x_corr [n] the last
              corrected latent; the rows say which of them exist, so nothing initialises them either.
      "dpm_sde": one SDE-DPM-Solver++(2M) step, upk_dpmpp_2m_sde_step_f32 (coefficient rows of 8, entry 5 the host's noise scale);
              m_old [n] is the data prediction of the step before, read only where a row's w is non-zero.  The noise table
              is allowed (eta > 0).  None = no mask; "masked" = the keep table, the expanded mask and x_plain of
              ensure_edit(), as DDIM's masked variant.  A chain that starts at loop position k > 0 presets plan.step to k and
              loads a table built for it (start = k) into rows k .. S - 1.
    cfg: classifier-free guidance — the plan runs 2*B rows ([unconditional ; conditional], ddim.py:173-178), the latent
    state has B = plan.B // 2 samples and the update combines the two halves of eps."""

    def __init__(self, plan: UNetPlan, channels, kind="ddim", cfg=False):
        require(plan.mode == "sampler", "SamplerState needs a sampler-mode plan", ValueError)
        require(kind in self._STEP, lambda: "SamplerState kind must be one of %s, got %r" % (tuple(self._STEP), kind), ValueError)
        require(not cfg or plan.B % 2 == 0, "guidance runs [uncond ; cond]: the plan's batch must be even", ValueError)
        require(not (cfg and kind == "ddpm"), "the DDPM step has no guidance", ValueError)
        self.plan = plan
        self.kind = kind
        self.cfg = bool(cfg)
        self.noise2 = self.x0 = self.mask = None
        self.keep = self.edit_mask = self.x_plain = None
        B, H, W, R = (plan.B // 2 if cfg else plan.B), plan.H, plan.W, plan.rows
        self.B = B
        self.C = channels
        self.x = plan.alloc(B, channels, H, W, dtype=torch.float32)
        self.pred_x0 = plan.alloc(B, channels, H, W, dtype=torch.float32)
        self.coefs = plan.alloc(R, {"ddpm": 8, "dpm": 8, "unipc": 12, "dpm_sde": 8}.get(kind, 4), dtype=torch.float32)
        self.noise = None
        self._coef_key = None  # what `coefs` holds (load_coefs)
        self._nscale_key = self._nscale = None  # keyed DDIM's per-row noise scale on the device (load_noise_scale)
        self.graphs = {}  # (with_noise, scale, nsteps, variant) -> instantiated graph, least recently used first
        self.step_done = plan.alloc(1, dtype=torch.int32, zero=True)  # arrival counter of the step kernels
        self.hist = plan.alloc(3, B * channels * H * W, dtype=torch.float32) if kind in ("plms", "unipc") else None
        self.x_corr = plan.alloc(B * channels * H * W, dtype=torch.float32) if kind == "unipc" else None
        self.x0_old = plan.alloc(B * channels * H * W, dtype=torch.float32) if kind == "dpm" else None
        self.m_old = plan.alloc(B * channels * H * W, dtype=torch.float32) if kind == "dpm_sde" else None
        self.set_variant((0, False) if kind == "ddpm" else None)

    def set_variant(self, variant):
        """The variant of the launches that follow (class docstring); the one place that checks it against the kind."""
        if self.kind == "ddpm":
            ok = isinstance(variant, tuple) and len(variant) == 2 and isinstance(variant[0], int) and isinstance(variant[1], bool)
        else:
            ok = variant is None or (self.kind == "ddim" and variant in ("plain", "masked")) or \
                (self.kind == "dpm_sde" and variant == "masked")
        require(ok, lambda: "a %r sampler state has no step variant %r" % (self.kind, variant), ValueError)
        self.variant = variant

    def close(self):
        """Destroys the instantiated HIP graphs (they hold device memory; called when the owning plan is dropped).
        sample() hands back a clone enqueued behind the last replay, so a replay may still be in flight when a new shape
        evicts this plan: the device is drained first (HIP does not promise deferred destruction of an executing graph)."""
        if self.graphs:
            torch.cuda.synchronize(self.plan.dev)
        for g in self.graphs.values():
            self.plan.ctx.graph_destroy(g)
        self.graphs = {}
        self.keep = self.edit_mask = self.x_plain = None  # (no graph is left that reads them)

    # ---- upload-once tables: a sampler asks "fresh?" in front of chain.upload_lock and loads under it only then, so the
    # key object of an unchanged table stays the one that was stored
    def coefs_fresh(self, key):
        return self._coef_key != key

    def load_coefs(self, key, table, row0=0):
        """The len(table) coefficient rows from row0 on (PLMS fills S of its S + 1; a "dpm_sde" chain from loop position k
        its rows k .. S - 1)."""
        self.coefs[row0:row0 + table.shape[0]].copy_(table)
        self._coef_key = key

    def scale_fresh(self, key):
        return self._nscale_key != key

    def load_noise_scale(self, key, scale):
        self._nscale = scale.to(self.plan.dev)
        self._nscale_key = key

    def ensure_noise(self):
        if self.noise is None:
            p = self.plan
            self.noise = p.alloc(p.rows, self.B * self.C * p.H * p.W, dtype=torch.float32)
        return self.noise

    def ensure_mask(self):
        """The masked-chain buffers (DDPM): q_sample noise table, x0 and the mask, both expanded to the latent."""
        if self.mask is None:
            p, n = self.plan, self.B * self.C * self.plan.H * self.plan.W
            self.noise2 = p.alloc(p.rows, n, dtype=torch.float32)
            self.x0 = p.alloc(n, dtype=torch.float32)
            self.mask = p.alloc(n, dtype=torch.float32)
        return self.noise2, self.x0, self.mask

    def ensure_edit(self):
        """The masked-chain buffers (DDIM): keep [rows, n] (row r = q_sample(x0, t) of loop position r), the mask expanded
        to the latent, and x_plain (the unblended x_prev the reference logs).  They belong to this state, not to the
        plan's buffer list: close() frees them.  At 200 steps, B = 8, 4x32x24 the table is 200 * 24576 * 4 B = 20 MB."""
        if self.keep is None:
            p, n = self.plan, self.B * self.C * self.plan.H * self.plan.W
            self.keep = torch.empty(p.rows, n, dtype=torch.float32, device=p.dev)
            self.edit_mask = torch.empty(n, dtype=torch.float32, device=p.dev)
            self.x_plain = torch.empty(self.B, self.C, p.H, p.W, dtype=torch.float32, device=p.dev)
        return self.keep, self.edit_mask, self.x_plain

    # ---- the step of (kind, variant): the buffers it needs besides the noise table, and (kernel, the arguments between the
    # context handle and the stream).  The arguments are read after the buffers exist.
    def _ddim_step(self, nz, scale):
        p, v = self.plan, self.variant
        head = (self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), nz)
        if v is not None:
            ptr = (lambda t: t.data_ptr()) if v == "masked" else (lambda t: None)
            return p.lib.upk_ddim_step_edit_f32, head + (
                ptr(self.keep), ptr(self.edit_mask), p.rows, p.step.data_ptr(), self.pred_x0.data_ptr(), ptr(self.x_plain),
                p.xin.t.data_ptr(), p.xin.ld, self.B, self.C, p.H * p.W, float(scale), int(self.cfg))
        tail = (p.step.data_ptr(), self.pred_x0.data_ptr(), p.xin.t.data_ptr(), p.xin.ld)
        if self.cfg:
            return p.lib.upk_ddim_step_cfg_f32, head + tail + (self.B, self.C, p.H * p.W, float(scale))
        return p.lib.upk_ddim_step_f32, head + tail + (p.B, self.C, p.H * p.W)

    def _plms_step(self, nz, scale):
        p = self.plan
        require(nz is None, "PLMS runs with eta = 0", ValueError)
        return p.lib.upk_plms_step_f32, (
            self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), p.step.data_ptr(), self.hist.data_ptr(),
            self.pred_x0.data_ptr(), p.xin.t.data_ptr(), p.xin.ld, self.B, self.C, p.H * p.W, float(scale), int(self.cfg))

    def _ddpm_step(self, nz, scale):
        p, (flags, masked) = self.plan, self.variant
        ptr = (lambda t: t.data_ptr()) if masked else (lambda t: None)
        return p.lib.upk_ddpm_step_f32, (
            self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), nz, ptr(self.noise2), ptr(self.x0), ptr(self.mask),
            p.step.data_ptr(), self.pred_x0.data_ptr(), p.xin.t.data_ptr(), p.xin.ld, self.B, self.C, p.H * p.W, int(flags))

    def _dpm_step(self, nz, scale):
        p = self.plan
        require(nz is None, "DPM-Solver++(2M) runs with eta = 0", ValueError)
        return p.lib.upk_dpmpp_2m_step_f32, (
            self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), p.step.data_ptr(), self.x0_old.data_ptr(),
            self.pred_x0.data_ptr(), p.xin.t.data_ptr(), p.xin.ld, self.B, self.C, p.H * p.W, 0, float(scale), int(self.cfg))

    def _unipc_step(self, nz, scale):
        p = self.plan
        require(nz is None, "UniPC runs with eta = 0", ValueError)
        return p.lib.upk_unipc_step_f32, (
            self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), p.step.data_ptr(), self.hist.data_ptr(),
            self.x_corr.data_ptr(), self.pred_x0.data_ptr(), p.xin.t.data_ptr(), p.xin.ld, self.B, self.C, p.H * p.W,
            float(scale), int(self.cfg))

    def _dpm_sde_step(self, nz, scale):
        p = self.plan
        ptr = (lambda t: t.data_ptr()) if self.variant == "masked" else (lambda t: None)
        return p.lib.upk_dpmpp_2m_sde_step_f32, (
            self.x.data_ptr(), p.eps.data_ptr(), self.coefs.data_ptr(), nz, ptr(self.keep), ptr(self.edit_mask), p.rows,
            p.step.data_ptr(), self.m_old.data_ptr(), self.pred_x0.data_ptr(), ptr(self.x_plain), p.xin.t.data_ptr(),
            p.xin.ld, self.B, self.C, p.H * p.W, float(scale), int(self.cfg))

    _STEP = {"ddim": _ddim_step, "plms": _plms_step, "ddpm": _ddpm_step, "dpm": _dpm_step, "unipc": _unipc_step,
             "dpm_sde": _dpm_sde_step}

    def _ensure(self, with_noise):
        """The buffers the step of (kind, variant) reads besides the state's own."""
        if with_noise:
            self.ensure_noise()
        if self.kind == "ddpm" and self.variant[1]:
            self.ensure_mask()
        if self.kind in ("ddim", "dpm_sde") and self.variant == "masked":
            self.ensure_edit()

    def _emit_tail(self, stream, with_noise, scale=1.0):
        p = self.plan
        fn, args = self._STEP[self.kind](self, self.noise.data_ptr() if with_noise else None, scale)
        # the step kernel also advances the device-side step counter (include/upk.h upk_step_autoadvance)
        p.ctx._chk(p.lib.upk_step_autoadvance(p.hctx, self.step_done.data_ptr()))
        try:
            p.ctx._chk(fn(p.hctx, *args, stream))
        finally:
            p.ctx._chk(p.lib.upk_step_autoadvance(p.hctx, None))

    def graph(self, with_noise, scale=1.0, nsteps=1):
        """`nsteps` consecutive steps of the current variant captured as ONE HIP graph (static shapes, device-side step
        index: the same graph serves every position of the loop; the guidance scale is a kernel argument, so each scale
        value gets its own graph).  nsteps > 1 saves the graph-to-graph launch gap of the steps inside."""
        key = (bool(with_noise), float(scale) if self.cfg else 1.0, int(nsteps), self.variant)
        g = self.graphs.pop(key, None)
        if g is not None:
            self.graphs[key] = g  # (most recently used last: eviction takes the least recently used graph)
        if g is None:
            p = self.plan
            self._ensure(with_noise)
            with L.host_io():  # (no other lane uploads from the host while this thread captures)
                side = torch.cuda.Stream(device=p.dev)
                side.wait_stream(torch.cuda.current_stream(p.dev))
                sp = side.cuda_stream
                p.ctx._chk(p.lib.upk_graph_begin(p.hctx, sp))
                try:
                    for _ in range(int(nsteps)):
                        p.body.run(sp)
                        self._emit_tail(sp, with_noise, scale)
                finally:
                    gh = C.c_void_p()
                    rc = p.lib.upk_graph_end(p.hctx, sp, C.byref(gh))
                p.ctx._chk(rc)
                torch.cuda.current_stream(p.dev).wait_stream(side)
            # one sample() makes up to three graphs per (noise, scale) (full groups of steps, the remainder, single steps
            # around a callback): 16 graphs = five guidance scales in rotation; least recently used first
            if len(self.graphs) >= 16:
                torch.cuda.synchronize(p.dev)  # (the evicted graph may still be executing)
                p.ctx.graph_destroy(self.graphs.pop(next(iter(self.graphs))))
            g = self.graphs[key] = gh
        return g

    def launch(self, with_noise, scale=1.0, nsteps=1):
        p = self.plan
        p.ctx._chk(p.lib.upk_graph_launch(p.hctx, self.graph(with_noise, scale, nsteps), p.ctx._s()))

