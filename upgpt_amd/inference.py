"""Caller glue of the demo / notebooks around the hot path: the reference's
`ldm/data/generate_utils.py` — `InferenceModel` (:137-189), the person-mask helpers `get_coord` / `get_mask` /
`interp_mask` (:110-134), `get_empty_style` (:103-104), `convert_fname` (:75-96), `load_model_from_config` (:34-49) —
so `app.py` and the inference notebooks drive THIS build through the calls they already make
(`from ldm.data.generate_utils import InferenceModel, convert_fname, interp_mask`).

What is different from the reference, by necessity of the environment rather than by design:

* no torchvision / omegaconf / skimage / pandas imports at module scope (none is needed for these functions; the CLIP
  normalisation constants are applied with torch);
* the CLIP weights: the reference's `clip.load("ViT-L/14")` downloads them; here `InferenceModel(..., clip_weights=path)`
  loads the `clip` package's state dict (one file, both towers) into the two HIP-kernel encoders, and `ckpt=None` /
  `clip_weights=None` leave the corresponding weights at their initial values (tests load recipe weights afterwards);
* the tokenizers (`clip.tokenize`, the hub tokenizer of FrozenCLIPEmbedder) need vocabulary files that are not on disk:
  pass `clip_tokenizer=` / `text_tokenizer=`; without them the string entry points raise RuntimeError.

All compute behind these calls runs through libupk.so (the two CLIP towers, the UNet x DDIM loop, the VAE).
"""
import copy
import re

import numpy as np
import torch

from .config import instantiate_from_config, to_plain

style_names = ['face', 'hair', 'headwear', 'background', 'top', 'outer', 'bottom', 'shoes', 'accesories']  # (sic)

# CLIP pre-processing constants (clip package `_transform`; generate_utils.py:98-101)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MASK_BG, MASK_FG = -1.0, -0.99215686  # person_mask values: 0/255 and 1/255 mapped to [-1, 1] (deepfashion_inshop.py:235-239)


def load_model_from_config(config, ckpt, verbose=False):
    """generate_utils.py:34-49.  `config` holds a `model` node; `ckpt` is a Lightning checkpoint ({'state_dict': ...}),
    or None for an un-initialised model."""
    cfg = to_plain(config)
    model = instantiate_from_config(cfg["model"] if "model" in cfg else cfg)
    if ckpt is not None:
        print(f"Loading model from {ckpt}")
        pl_sd = torch.load(ckpt, map_location="cpu", weights_only=False)
        if "global_step" in pl_sd:
            print(f"Global Step: {pl_sd['global_step']}")
        missing, unexpected = model.load_state_dict(pl_sd["state_dict"], strict=False)
        if verbose:
            for title, keys in (("missing keys:", missing), ("unexpected keys:", unexpected)):
                if len(keys) > 0:
                    print(title)
                    print(keys)
    model.eval()
    return model


def clip_normalize(img01):
    """[3, H, W] image in [0, 1] -> CLIP-normalised (the Normalize half of generate_utils.clip_transform)."""
    mean = torch.tensor(CLIP_MEAN, dtype=img01.dtype).view(3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=img01.dtype).view(3, 1, 1)
    return (img01 - mean) / std


def get_empty_style():
    """The 'no style' crop: a black 224x224 image through the CLIP transform (generate_utils.py:103-104; float64 like
    the reference's ToTensor of a float64 array)."""
    return clip_normalize(torch.zeros(3, 224, 224, dtype=torch.float64))


def denormalize_style(style):
    """Inverse of the CLIP normalisation for display ([3, H, W] -> [H, W, 3] in [0, 1]); generate_utils.py:52-56."""
    mean = torch.tensor(CLIP_MEAN, dtype=style.dtype).view(3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=style.dtype).view(3, 1, 1)
    return (style * std + mean).clamp(0, 1).permute(1, 2, 0)


def draw_styles(style_batch):
    """Grid of the first eight style crops (generate_utils.py:52-72); needs matplotlib."""
    import matplotlib.pyplot as plt
    fig, axs = plt.subplots(2, 4)
    fig.set_figheight(8)
    fig.set_figwidth(16)
    for i, (name, style) in enumerate(zip(style_names[:-1], style_batch[:-1])):
        ax = axs[i // 4, i % 4]
        ax.imshow(denormalize_style(style.detach().cpu().float()).numpy())
        ax.set_title(name)
        ax.axis('off')
    plt.show()


_FNAME = {"MEN": re.compile(r'MEN(\w+)id(\d+)_(\d)(\w+)'), "WOMEN": re.compile(r'WOMEN(\w+)id(\d+)_(\d)(\w+)')}


def convert_fname(long_name):
    """'fashionWOMENBlouses_Shirtsid0000311501_7additional___fashionWOMEN...01_2side' ->
    ['WOMEN/Blouses_Shirts/id_00003115/01_7_additional', 'WOMEN/Blouses_Shirts/id_00003115/01_2_side']
    (generate_utils.py:75-96: the gender is read from characters 7..9 of the first name and applied to all)."""
    gender = 'MEN' if long_name[7:10] == 'MEN' else 'WOMEN'
    joined = ' '.join(long_name.replace('fashion', '').split('___'))
    return ['%s/%s/id_%s/%s_%s_%s' % (gender, cat, num[:8], num[8:], view, desc)
            for cat, num, view, desc in _FNAME[gender].findall(joined)]


def get_coord(batch_mask):
    """Bounding box [xmin, xmax, ymin, ymax] (rows, then columns) of the non-background part of person_mask
    [1, h, w] (generate_utils.py:110-118).  Like the reference, background (-1) is zeroed IN PLACE when the mask lives
    on the CPU (`.cpu().numpy()` shares memory there)."""
    mask = batch_mask[0].cpu().numpy()
    mask[mask == MASK_BG] = 0
    rows = np.nonzero(np.mean(mask, 1))[0]
    cols = np.nonzero(np.mean(mask, 0))[0]
    return np.array([rows[0], rows[-1], cols[0], cols[-1]])


def get_mask(mask, coord):
    """person_mask of `mask`'s shape/device: background everywhere, foreground inside the inclusive box `coord`
    (generate_utils.py:120-126)."""
    xmin, xmax, ymin, ymax = coord
    new_mask = np.full(tuple(mask.shape), MASK_BG, dtype=mask.cpu().numpy().dtype)
    new_mask[0, xmin:xmax + 1, ymin:ymax + 1] = MASK_FG
    return torch.tensor(new_mask).to(mask.device)


def interp_mask(src_mask, dst_mask, alpha):
    """Box of src and dst blended alpha : (1 - alpha), truncated to int (generate_utils.py:128-134)."""
    coord = (alpha * get_coord(src_mask) + (1 - alpha) * get_coord(dst_mask)).astype(np.int32)
    return get_mask(src_mask, coord)


def load_clip_weights(path, text_encoder=None, image_encoder=None, cond_stage=None):
    """Loads a state dict of the `clip` package's CLIP model (as `clip.load(name, jit=False)[0].state_dict()` saves it:
    `visual.*`, `transformer.*`, `token_embedding.weight`, `positional_embedding`, `ln_final.*`, `text_projection`,
    `logit_scale`) into the text tower and/or the image tower.
    cond_stage: a CLIPTextImageCrossAtten; `path` then holds the state dict of transformers' `CLIPModel` (as
    `CLIPModel.from_pretrained(version).state_dict()` saves it), loaded into `cond_stage.model`; `position_ids`
    buffers of older transformers versions are ignored."""
    sd = torch.load(path, map_location="cpu", weights_only=False)
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
    if cond_stage is not None:
        want = cond_stage.model.state_dict()
        cond_stage.model.load_state_dict({k: sd[k].float().reshape(want[k].shape) for k in want})
        return
    if text_encoder is not None:
        want = text_encoder.model.state_dict()
        text_encoder.model.load_state_dict({k: sd[k].float() for k in want})
    if image_encoder is not None:
        want = image_encoder.model.visual.state_dict()
        image_encoder.model.visual.load_state_dict({k: sd["visual." + k].float() for k in want})


class InferenceModel:
    """generate_utils.py:137-189.  Holds the two CLIP encoders of the style mixer and the diffusion model whose style
    stage is a pass-through (`mix_style` hands over [9, 768] embeddings)."""

    def __init__(self, config, ckpt, device, clip_weights=None, clip_tokenizer=None, text_tokenizer=None):
        self.device = device
        config = copy.deepcopy(to_plain(config))
        params = config['model']['params']
        text_cfg = {'target': 'ldm.modules.encoders.modules.FrozenCLIPTextEmbedder',
                    'params': {'normalize': False, 'device': device}}
        self.clip_text_encoder = instantiate_from_config(text_cfg)
        self.clip_text_encoder.tokenizer = clip_tokenizer
        style_cfg = dict(params['extra_cond_stages']['style_cond'], params={'device': device})
        self.clip_image_encoder = instantiate_from_config(style_cfg)
        if clip_weights is not None:
            load_clip_weights(clip_weights, self.clip_text_encoder, self.clip_image_encoder)
        self.clip_text_encoder.to(device)
        self.clip_image_encoder.to(device)
        # the diffusion model receives style EMBEDDINGS; its first stage is filled from the checkpoint, not from a file
        params['extra_cond_stages']['style_cond']['target'] = 'ldm.modules.poses.poses.DummyModel'
        params['first_stage_config']['params']['ckpt_path'] = None
        params['cond_stage_config']['params'] = {'device': device}
        self.model = load_model_from_config(config, ckpt).to(device)
        if text_tokenizer is not None and hasattr(self.model.cond_stage_model, "tokenizer"):
            self.model.cond_stage_model.tokenizer = text_tokenizer

    def create_batch(self, batch, repeat=1):
        """One sample -> a batch of `repeat` copies on the device (tensors gain a leading axis, other entries become
        lists); modifies and returns `batch` like the reference (:150-158)."""
        for k, v in batch.items():
            if type(v) == torch.Tensor:
                batch[k] = v.unsqueeze(0).repeat([repeat] + [1] * v.dim()).to(self.device)
            else:
                batch[k] = [v] * repeat
        return batch

    def generate(self, batch, steps=200, repeat=1, use_ema=True, sampler="ddim", noise_keys=None):
        """log_images with the demo's settings -> {'reconstruction'?, 'samples'} as float numpy [b, h, w, 3] in [0, 1]
        (:160-170; `repeat` is unused there as well).  sampler: "ddim" (the reference's), "dpmpp_2m" for
        DPM-Solver++(2M), "unipc" for UniPC or "dpmpp_2m_sde" for SDE-DPM-Solver++(2M) (stochastic: log_images' eta of 1), each
        with `steps` steps (LatentDiffusion.sample_log).  noise_keys (upgpt_amd.rng.NoiseKeys, one key
        per sample): handed to log_images, which then draws keyed noise instead of the torch generator's."""
        extra = {} if sampler == "ddim" else {"sampler": sampler}
        if noise_keys is not None:
            extra["noise_keys"] = noise_keys
        with torch.no_grad():
            images = self.model.log_images(batch, ddim_steps=steps, use_ema=use_ema, unconditional_guidance_scale=3.,
                                           unconditional_guidance_label=[""], **extra)
        out = {}
        for k, v in images.items():
            v = torch.clamp(v.detach().cpu(), -1., 1.)
            out[k] = v.permute(0, 2, 3, 1).numpy() * 0.5 + 0.5
        return out

    FRAMES_PER_CALL = 8  # log_images' default N: the samples one generate() call returns at most

    def interpolate(self, batch, dst_pose, alphas, steps=200, use_ema=True, sampler="ddim", noise_seed=None, noise="shared"):
        """The demo's "Interpolate" button (app.py:280-308): n = len(alphas) frames between the pose of `batch` and
        `dst_pose`, frame i conditioned on alphas[i] of the source and 1 - alphas[i] of the destination -> generate's
        dict ('samples', 'reconstruction'?) with ALL n frames, float numpy [n, h, w, 3] in [0, 1].
        batch: the UN-batched sample the demo hands to create_batch (image, styles, txt, ...), with the source pose's
        `smpl` [1, d] and `person_mask` [1, h, w]; dst_pose: prepare.load_pose's dict, or any dict with `smpl` and
        `person_mask`.  alphas: floats in [0, 1] (ValueError otherwise, also for none at all).
        The conditioning of all frames is one launch on the device (prepare.interp_pose), bit for bit the reference's
        loop.  The frames are then produced in chunks of at most 8, log_images' cap N: the reference makes ONE generate
        call, so the demo's default of nine alphas silently yields eight pictures there, and nine here.
        noise_seed=None draws x_T and the step noise from the torch generator, independently per frame, as the reference
        does.  With a seed the frames are keyed (upgpt_amd.rng.NoiseKeys(noise_seed, ids)): noise="shared" gives every
        frame id 0, so x_T and every step's noise are the same for all frames and only the pose differs between them;
        noise="independent" gives frame i id i.
        Neither `batch` nor `dst_pose` is modified.  (The reference's get_coord zeroes the destination mask's background
        in place when that mask is a CPU tensor; this has no effect on any result and is not reproduced.)"""
        from . import prepare
        from ._check import require
        from .rng import NoiseKeys
        a = prepare.check_alphas(alphas)
        require(noise in ("shared", "independent"), lambda: "noise must be 'shared' or 'independent', got %r" % (noise,), ValueError)
        for name, d in (("batch", batch), ("dst_pose", dst_pose)):
            for k in ("smpl", "person_mask"):
                require(k in d, lambda: "interpolate: %s has no %r" % (name, k), ValueError)
        n = int(a.size)
        cond = prepare.interp_pose(batch["person_mask"], dst_pose["person_mask"], batch["smpl"], dst_pose["smpl"], a)
        keys = None
        if noise_seed is not None:
            keys = NoiseKeys(noise_seed, [0] * n if noise == "shared" else range(n), device=self.device)
        rest = {k: v for k, v in batch.items() if k not in ("smpl", "person_mask")}
        parts = []
        for lo in range(0, n, InferenceModel.FRAMES_PER_CALL):
            m = min(InferenceModel.FRAMES_PER_CALL, n - lo)
            chunk = InferenceModel.create_batch(self, dict(rest), repeat=m)  # (a copy of the dict: `batch` keeps its entries)
            chunk["smpl"], chunk["person_mask"] = cond["smpl"][lo:lo + m], cond["person_mask"][lo:lo + m]
            kw = {} if keys is None else {"noise_keys": keys[lo:lo + m]}
            parts.append(InferenceModel.generate(self, chunk, steps, use_ema=use_ema, sampler=sampler, **kw))
        return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}

    def upscale(self, pictures, styles, txt, steps=200, pad=(4, 0), use_ema=False, image=None, sampler="ddim"):
        """The demo's "Upscale" button (app.py:387-399), called on the InferenceModel that holds the upscale checkpoint:
        low-resolution pictures -> generate()'s dict, 'samples' float numpy [B, f H, f W, 3] in [0, 1] with [H, W] the
        model's image_size and f = 2 ** num_downs (512 x 384 for the reference's config).
        pictures: uint8 [B, h, w, 3], a device tensor (the bytes upk_image_finish_u8 wrote are taken in place), a host
        array / tensor, or a list of PIL images of one size; styles: [B, 9, 768] or [9, 768], mix_style's output; txt: a
        string or a list of B strings.  batch['lr'] is prepare.lr_transform(pictures, image_size, pad)[0], the
        reference's lr_transform (pad 4 columns by edge replication, bilinear resize as Pillow does it, ToTensor,
        x * 2 - 1) in one launch on the device; batch['image'] defaults to zeros [B, f H, f W, 3], standing in for the
        dummy picture the demo loads (only its shape matters outside the reconstruction).  As with generate, log_images'
        default N = 8 caps the samples of one call.  sampler: as in generate."""
        from . import prepare
        if isinstance(pictures, (list, tuple)):
            pictures = np.stack([np.asarray(p.convert("RGB") if hasattr(p, "convert") else p, dtype=np.uint8) for p in pictures])
        lr = prepare.lr_transform(pictures, self.model.image_size, pad)[0]
        n = int(lr.shape[0])
        styles = torch.as_tensor(styles)
        if styles.dim() == 2:
            styles = styles.unsqueeze(0).repeat(n, 1, 1)
        if isinstance(txt, str):
            txt = [txt] * n
        elif not torch.is_tensor(txt):  # (a tensor: embeddings for a model whose text stage is a pass-through)
            txt = list(txt)
        if styles.shape[0] != n or len(txt) != n:
            raise ValueError("upscale: %d pictures, %d styles, %d texts" % (n, styles.shape[0], len(txt)))
        if image is None:
            f = 2 ** self.model.num_downs
            image = torch.zeros(n, f * self.model.image_size[0], f * self.model.image_size[1], 3, device=lr.device)
        batch = {'image': image, 'lr': lr, 'styles': styles.to(lr.device), 'txt': txt}
        return self.generate(batch, steps, use_ema=use_ema, sampler=sampler)

    def extract_styles(self, picture, segm, segmenter='lip'):
        """The style crops of ONE source picture, ready for mix_style: fp32 [9, 3, 224, 224] on the device, one crop per
        entry of style_names, CLIP-normalised.  The reference's Segmenter.forward (segm_utils.py) and clip_transform,
        made by styles.style_crops in two launches on the device, without the reference's <style>.jpg files in between.
        picture: uint8 [H, W, 3] (a PIL image, a host array or a tensor; a device tensor is read in place); segm: the
        human-parsing label map uint8 [H, W] of the same size; segmenter: 'lip' (eight groups), 'mm' (face, background,
        skin) or a styles.Segmenter.  A style the segmenter does not produce, or whose cut is empty, is the empty
        style clip_norm(0)."""
        from . import styles

        def as_map(v, mode):
            if hasattr(v, "convert"):  # a PIL image
                v = np.asarray(v.convert(mode) if mode == "RGB" else v, dtype=np.uint8)
            return v[None] if isinstance(v, np.ndarray) or torch.is_tensor(v) else v
        return styles.style_crops(as_map(picture, "RGB"), as_map(segm, None), segmenter, style_names)[0][0]

    def edit_region(self, picture, segm, region, batch, steps=200, use_ema=True, sampler="ddim", segmenter='lip', dilate=8,
                    feather=4, noise_keys=None):
        """Region-locked editing: the photo with ONE region generated anew, e.g. a new top, and every
        pixel farther than dilate + feather from the old region byte-identical to the input.
        picture: uint8 [H, W, 3] or [B, H, W, 3] (a PIL image, a host array or a tensor; a device tensor is read in
        place), H x W the size the first stage decodes the model's latent to (ValueError otherwise); segm: the
        human-parsing label map(s) uint8 [H, W] / [B, H, W]; region / segmenter: edit.region_labels ('top', 'bottom',
        'hair', 'label:top', a list of names, ...).  batch: the conditioning as generate takes it after create_batch
        (txt, styles, smpl, person_mask, ...), with the NEW style already in its slot (a crop or a text through
        mix_style); it is not modified and an 'image' entry in it is ignored: the picture is the image.
        On the device: the picture as the model's input (prepare.lr_transform with both passes skipped, the reference's
        image_transform), edit.region_mask at the first stage's factor, LatentDiffusion.edit_images with generate's
        guidance arguments, upk_image_finish_u8 for the generated bytes, edit.composite against the original bytes; one
        copy and one synchronise at the end.  Returns host arrays {'edited' uint8 [B, H, W, 3], 'samples' uint8 [B, H,
        W, 3] (the whole generated pictures), 'mask' uint8 [B, H, W], 'alpha' uint8 [B, H, W], 'cells' int32 [B]}.
        A sample whose region is empty (cells 0) has alpha 0 everywhere and comes back as its input, with no special
        case.  At most 8 samples per call, like generate: more is a ValueError, not a silent cut."""
        from . import _lib, edit, prepare
        from ._check import require
        from .evaluate import finish_images

        def as_array(v, mode):
            if hasattr(v, "convert"):  # a PIL image
                v = np.asarray(v.convert(mode) if mode == "RGB" else v, dtype=np.uint8)
            return v
        edit.region_labels(region, segmenter)  # (everything refusable is refused before anything is uploaded)
        if sampler == "unipc":  # (a region edit is a masked chain)
            from .unipc import _MASKED
            raise NotImplementedError(_MASKED)
        require(0 <= int(dilate) <= edit.MAX_DILATE, lambda: "dilate must be 0 .. %d, got %r" % (edit.MAX_DILATE, dilate), ValueError)
        require(0 <= int(feather) <= edit.MAX_FEATHER, lambda: "feather must be 0 .. %d, got %r" % (edit.MAX_FEATHER, feather),
                ValueError)
        picture, segm = as_array(picture, "RGB"), as_array(segm, None)
        if (isinstance(picture, np.ndarray) or torch.is_tensor(picture)) and picture.ndim == 3:
            picture = picture[None]
        if (isinstance(segm, np.ndarray) or torch.is_tensor(segm)) and segm.ndim == 2:
            segm = segm[None]
        picture, segm = edit._u8("picture", picture, "[H, W, 3] or [B, H, W, 3]", 4), edit._u8("segm", segm, "[H, W] or [B, H, W]", 3)
        b, h, w = (int(v) for v in picture.shape[:3])
        require(picture.shape[3] == 3, lambda: "3-channel pictures only, got %s" % (tuple(picture.shape),), ValueError)
        require(tuple(segm.shape) == (b, h, w), lambda: "segm %s does not match picture %s" % (tuple(segm.shape), tuple(picture.shape)),
                ValueError)
        f = 2 ** int(self.model.num_downs)
        size = [f * int(v) for v in self.model.image_size]
        require([h, w] == size, lambda: "edit_region: a %d x %d picture, the model works on %d x %d" % (h, w, size[0], size[1]),
                ValueError)
        require(b <= InferenceModel.FRAMES_PER_CALL, lambda: "edit_region: %d samples, at most %d per call" % (
            b, InferenceModel.FRAMES_PER_CALL), ValueError)
        picture, segm = edit._on_device([picture, segm], "a region is edited on the MI355X (upk_region_mask_u8, upk_composite_u8)")
        cond = {k: v for k, v in batch.items() if k != "image"}
        cond["image"] = prepare.lr_transform(picture, size)[1]
        mask, keep, cells = edit.region_mask(segm, region, segmenter, dilate, f)
        extra = {} if sampler == "ddim" else {"sampler": sampler}
        with torch.no_grad():
            log = self.model.edit_images(cond, keep, N=b, ddim_steps=steps, noise_keys=noise_keys, use_ema=use_ema,
                                         unconditional_guidance_scale=3., unconditional_guidance_label=[""], **extra)
        samples = log["samples"].to(picture.device, torch.float32)
        gen = torch.empty((b, h, w, 3), dtype=torch.uint8, device=picture.device)
        finish_images(samples, gen, _lib.LAYOUT_NCHW, _lib.FINISH_SAMPLE)
        edited, alpha = edit.composite(picture, gen, mask, feather, return_alpha=True)
        parts = [("cells", cells, np.int32), ("edited", edited, np.uint8), ("samples", gen, np.uint8), ("mask", mask, np.uint8),
                 ("alpha", alpha, np.uint8)]
        buf = torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for _, t, _ in parts])
        host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        torch.cuda.current_stream(buf.device).synchronize()
        arr, out, off = host.numpy(), {}, 0
        for name, t, dtype in parts:
            nbytes = t.numel() * t.element_size()
            out[name] = arr[off:off + nbytes].view(dtype).reshape(tuple(t.shape)).copy()
            off += nbytes
        return out

    def mix_style(self, s, w, mask=[]):
        """Style embeddings [9, 768] of the crops `s` [9, 3, 224, 224]; slots named in `mask` are blanked (in `s`
        itself, as the reference does) and slots with a text in `w` take the CLIP TEXT embedding instead (:173-189)."""
        slot = {name: i for i, name in enumerate(style_names)}
        for m in mask:
            s[slot[m]] = get_empty_style()
        for k in w:
            if k not in slot:
                raise KeyError("unknown style slot %r (slots: %s)" % (k, ", ".join(style_names)))
        texts = [w.get(name, '') for name in style_names]
        with torch.no_grad():
            image_emb = self.clip_image_encoder(s.unsqueeze(0).to(self.device))
            if any(t != '' for t in texts):
                text_emb = self.clip_text_encoder([texts])
                for i, text in enumerate(texts):
                    if text != '':
                        image_emb[0, i] = text_emb[0, i]
        return image_emb.squeeze(0)
