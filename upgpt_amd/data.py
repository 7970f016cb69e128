"""The test split's loader: ldm.data.deepfashion_inshop.DeepFashionPair / DeepFashionSample (deepfashion_inshop.py:64-362),
the dataset every UPGPT model config names, with the batch assembled ON THE DEVICE.

The reference builds one sample at a time on CPU workers: the bounding box of a mask, Pillow's nearest-neighbour resize
to the latent size, ToTensor and x * 2 - 1, the CLIP normalisation of nine 224 x 224 crops, a label-to-weight map.  Here
PIL only decodes the files.  The bytes of a whole batch are packed into ONE pinned uint8 buffer (16-byte aligned
sections), uploaded in one copy, and every per-pixel operation is a HIP launch on the current stream (csrc/batch.hip,
csrc/resize.hip; include/upk.h), bit for bit the reference's fp32 arithmetic.  The result is the batch
dict LatentDiffusion.test_step takes as it is, with exactly the reference's keys (test_step passes N = len(batch)).

Two behaviours of the reference are deliberately NOT reproduced.  Its loader replaces a sample it cannot load by the
next one (skip_sample); here a missing or unreadable file, a picture of another size than its batch, a mask that is not
a 2-D uint8 array, an all-zero mask in 'bbox' mode or an empty `styles` cell raises ValueError naming the file or row (a
missing <style>.jpg is no error: the reference's clip_norm(zeros)).  And pictures are converted to RGB on decoding.
No CPU fallback: without a GPU the device functions raise."""
import csv
import json
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from . import _lib, prepare
from ._check import require
from .evaluate import _decode, center_crop_window
from .inference import CLIP_MEAN, CLIP_STD, style_names
from .styles import DeepfashionMMSegmenter, get_segmenter

STYLE_SIZE = 224           # the stored crops (Segmenter.forward: T.Resize(224), T.CenterCrop(224))
SMPL_CROP = (256, 192)     # smpl_image_transform: T.CenterCrop(size=(256, 192))
MASK_MODES = ('mask', 'smpl', 'bbox')
_tables = {}  # (device index, in, out) -> device int32 [out]


# ---- names (deepfashion_inshop.py:45-61)

def convert_fname(x):
    """'WOMEN/Blouses_Shirts/id_00003115/01_7_additional.jpg' -> 'fashionWOMENBlouses_Shirtsid0000311501_7additional'
    (deepfashion_inshop.py:45-49): the LAST '_' of the file name is dropped, 'id_' becomes 'id', the slashes go."""
    a, b = os.path.split(x)
    i = b.rfind('_')
    x = a + '/' + b[:i] + b[i + 1:]
    return 'fashion' + x.split('.jpg')[0].replace('id_', 'id').replace('/', '')


def get_name(src, dst):
    return convert_fname(src) + '___' + convert_fname(dst)


def list_subdirectories(path):
    """The leaf directories under `path` (deepfashion_inshop.py:56-61)."""
    return [dirpath for dirpath, dirnames, _ in os.walk(path) if not dirnames]


# ---- host tables

def nearest_table(in_size, out_size):
    """The source index Pillow's NEAREST resize reads per output index, int32 [out]: ImagingScaleAffine's own loop in
    double, a = in / out, xo = a * 0.5, per output idx = (int)xo, xo += a.  The closed form floor((i + 0.5) * in / out)
    is NOT the same function: the accumulated sum drifts, and at 256 -> 24 the two differ."""
    in_size, out_size = int(in_size), int(out_size)
    require(in_size >= 1 and out_size >= 1, "nearest_table: sizes must be positive, got %d -> %d" % (in_size, out_size),
            ValueError)
    a = in_size / out_size
    xo = a * 0.5
    tab = np.zeros(out_size, dtype=np.int32)
    for i in range(out_size):
        tab[i] = int(xo)
        xo += a
    return tab


def validate_table(tab, in_size):
    """What the kernels rely on: 0 <= idx < in (Pillow leaves a pixel whose index falls outside untouched; that never
    happens for a whole-picture resize, and a table for which it would is refused)."""
    require(tab.ndim == 1 and tab.size >= 1 and bool((tab >= 0).all() and (tab < in_size).all()),
            "nearest table leaves the %d-sample axis" % in_size, ValueError)


def device_table(device, in_size, out_size):
    """nearest_table on `device`, validated and uploaded once per (device, in, out); like prepare.device_coeffs, call it
    for the sizes in use before a graph capture begins."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(in_size), int(out_size))
    if key not in _tables:
        t = nearest_table(in_size, out_size)
        validate_table(t, int(in_size))
        with _lib.host_io():
            _tables[key] = torch.from_numpy(t).to(device)
    return _tables[key]


def mask_lut():
    """fp32 [256]: ToTensor and x * 2. - 1. of a byte, lut[u] = fl(fl(u / 255) * 2 - 1)."""
    return np.arange(256, dtype=np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)


def loss_lut(weights, segmenter='mm', default=1.0):
    """fp32 [256]: Segmenter.get_mask as a table, lut[label2id[name]] = weight, `default` elsewhere.  A mode-F PIL
    picture goes through NEAREST and ToTensor unscaled and unrounded, so the table's values are the map's."""
    seg = get_segmenter(segmenter)
    lut = np.full(256, default, dtype=np.float32)
    for label, value in (weights or {}).items():
        require(label in seg.label2id, "loss_weight names the label %r, which the segmenter does not have" % (label,), ValueError)
        lut[seg.label2id[label]] = value
    return lut


# ---- low-level device functions

def _size(size):
    size = [int(v) for v in size]
    require(len(size) == 2 and size[0] >= 1 and size[1] >= 1, "size must be [h, w] with positive entries, got %r" % (size,),
            ValueError)
    return size


def _device_u8(t, name, dims, what):
    """uint8 tensor of `dims` dimensions on the device, bytes dense inside a row (any row pitch and sample stride)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t) if t.flags.writeable else np.array(t))
    require(torch.is_tensor(t), "%s must be a uint8 tensor or array, got %s" % (name, type(t).__name__), TypeError)
    require(t.dtype == torch.uint8, "%s must be uint8, got %s" % (name, t.dtype), TypeError)
    require(t.dim() == dims and min(t.shape) >= 1, "%s must be a non-empty %s, got %s" % (name, what, tuple(t.shape)), ValueError)
    if not t.is_cuda:
        require(torch.cuda.is_available(), "the batch is assembled on the MI355X (csrc/batch.hip): no GPU is visible and there "
                "is no CPU fallback for the HIP path", RuntimeError)
        with _lib.host_io():
            t = t.contiguous().cuda()
    inner = 3 if dims == 4 else 1  # bytes per pixel
    ok = t.stride(-1) == 1 and t.stride(1) >= inner * t.shape[2] and t.stride(0) >= 0
    if dims == 4:
        ok = ok and t.shape[3] == 3 and t.stride(2) == 3
    else:
        ok = ok and t.stride(2) == 1
    return t if ok else t.contiguous()


def person_mask(maps, size, mode, return_boxes=False):
    """batch['person_mask'] fp32 [B, 1, h, w] on the device, size = [h, w] (the dataset's vae_z_size).
    mode 'mask': maps uint8 [B, H, W] -> Pillow's NEAREST resize, ToTensor, x * 2 - 1 (one upk_cond_gather_u8 launch).
    mode 'bbox': maps as above -> get_bbox, the box picture resized by NEAREST, and the reference's kept bug of 1 / 255:
        -0.99215686 inside, -1 outside (one upk_cond_bbox_u8 launch).  return_boxes=True also returns the boxes, int32
        [B, 4] = (r0, r1, c0, c1) on the device, -1 for a map without a non-zero byte (whose output is all background).
    mode 'smpl': maps uint8 [B, H, W, 3], the centre-cropped smpl pictures -> Pillow's BILINEAR resize
        (upk_resize_bilinear_u8), then torch.mean(x, 0) * 2 - 1 (upk_cond_smpl_u8): two launches.
    Device tensors are read in place whatever their row pitch and sample stride; host tensors / arrays are uploaded.
    Launches on the current stream, never synchronises."""
    require(mode in MASK_MODES, "mode must be one of %s, got %r" % (MASK_MODES, mode), ValueError)
    oh, ow = _size(size)
    if mode == 'smpl':
        src = _device_u8(maps, "maps", 4, "[B, H, W, 3]")
        b, dev = int(src.shape[0]), src.device
        u8 = prepare.resize_u8(src, [oh, ow])
        out = torch.empty((b, 1, oh, ow), dtype=torch.float32, device=dev)
        _lib.get_context(dev).cond_smpl(u8, u8.stride(1), u8.stride(0), b, oh, ow, out)
        return (out, None) if return_boxes else out
    src = _device_u8(maps, "maps", 3, "[B, H, W]")
    b, h, w = (int(v) for v in src.shape)
    dev = src.device
    ytab, xtab = device_table(dev, h, oh), device_table(dev, w, ow)
    out = torch.empty((b, 1, oh, ow), dtype=torch.float32, device=dev)
    ctx = _lib.get_context(dev)
    if mode == 'bbox':
        boxes = torch.empty((b, 4), dtype=torch.int32, device=dev)
        ctx.cond_bbox(src, src.stride(1), src.stride(0), b, h, w, ytab, xtab, oh, ow, out, boxes)
        return (out, boxes) if return_boxes else out
    ctx.cond_gather(src, src.stride(1), src.stride(0), b, h, w, ytab, xtab, oh, ow, mask_lut(), out)
    return (out, None) if return_boxes else out


def loss_weight(segm, size, weights, segmenter='mm'):
    """batch['loss_w'] fp32 [B, 1, h, w] on the device: Segmenter.get_mask(segm, weights) (1.0 where no listed label
    is), then loss_w_transform (NEAREST to size = [h, w], ToTensor of a float picture).  segm uint8 [B, H, W] label
    maps; weights {label name: weight}.  One upk_cond_gather_u8 launch."""
    lut = loss_lut(weights, segmenter)
    oh, ow = _size(size)
    src = _device_u8(segm, "segm", 3, "[B, H, W]")
    b, h, w = (int(v) for v in src.shape)
    dev = src.device
    out = torch.empty((b, 1, oh, ow), dtype=torch.float32, device=dev)
    _lib.get_context(dev).cond_gather(src, src.stride(1), src.stride(0), b, h, w, device_table(dev, h, oh),
                                      device_table(dev, w, ow), oh, ow, lut, out)
    return out


def clip_normalize(crops_u8, valid=None):
    """clip_transform of stored crops: uint8 [N, H, W, 3] -> fp32 [N, 3, H, W] on the device, fl(fl(fl(u / 255) - mean) /
    std) with the CLIP constants.  valid: int32 [N] or None; where it is 0 the result is clip_norm(0) and the crop's
    bytes are not read (a missing style file).  One upk_clip_normalize_u8 launch."""
    src = _device_u8(crops_u8, "crops_u8", 4, "[N, H, W, 3]")
    n, h, w = (int(v) for v in src.shape[:3])
    dev = src.device
    if valid is not None:
        if isinstance(valid, np.ndarray):
            valid = torch.from_numpy(np.ascontiguousarray(valid))
        require(torch.is_tensor(valid) and valid.dtype == torch.int32 and tuple(valid.shape) == (n,),
                "valid must be an int32 tensor [%d]" % n, TypeError)
        with _lib.host_io():
            valid = valid.to(dev).contiguous()
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    _lib.get_context(dev).clip_normalize_u8(src, src.stride(1), src.stride(0), valid, n, h, w, list(CLIP_MEAN) + list(CLIP_STD),
                                            out)
    return out


# ---- the tables of a split, with the standard library

def _read_csv(path):
    """(column names, rows as dicts of strings) of a csv file written by pandas; an empty cell reads ''."""
    with open(str(path), newline='') as f:
        rd = csv.DictReader(f)
        rows = [dict(r) for r in rd]
        return list(rd.fieldnames or []), rows


def _smpl_pose(path):
    """The `smpl` entry of one sample (deepfashion_inshop.py:245-251): pose, betas and camera of the first detection
    side by side, [1, n] in the pickle's own dtype (ToTensor does not convert a float array)."""
    with open(str(path), 'rb') as f:
        p = pickle.load(f)[0]
    pose = np.concatenate((p['pred_body_pose'], p['pred_betas'], np.expand_dims(p['pred_camera'], 0)), axis=1)
    return np.ascontiguousarray(pose).reshape(1, -1)


def _open_map(path, what):
    """A single-channel uint8 picture (PIL modes L / P) as a 2-D array."""
    from PIL import Image
    try:
        with Image.open(str(path)) as im:
            mode, arr = im.mode, np.array(im)
    except Exception:
        mode, arr = None, None
    require(arr is not None, "cannot read the %s %s" % (what, path), ValueError)
    require(mode in ('L', 'P') and arr.ndim == 2 and arr.dtype == np.uint8, "the %s %s is a mode-%s picture of shape %s: a "
            "2-D uint8 map (mode L or P) is needed" % (what, path, mode, arr.shape), ValueError)
    return arr


class _Pack:
    """The sections of one batch inside one pinned uint8 buffer, offsets multiples of 16 (like evaluate._sections)."""

    def __init__(self):
        self.items, self.total = {}, 0

    def add(self, name, arrays):
        arr = np.ascontiguousarray(np.stack(arrays))
        self.items[name] = (self.total, arr)
        self.total += (arr.nbytes + 15) // 16 * 16

    def upload(self, device):
        """name -> device tensor of the section's dtype and shape; one pinned buffer, one host -> device copy."""
        host = torch.empty(max(self.total, 16), dtype=torch.uint8, pin_memory=True)
        flat = host.numpy()
        for off, arr in self.items.values():
            flat[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        with _lib.host_io():
            dev = host.to(device, non_blocking=True)
        out = {}
        for name, (off, arr) in self.items.items():
            t = dev[off:off + arr.nbytes]
            out[name] = (t if arr.dtype == np.uint8 else t.view(getattr(torch, arr.dtype.name))).view(arr.shape)
        return out


class DeepFashionPair:
    """deepfashion_inshop.DeepFashionPair with the reference's constructor keywords.

    folder holds <image_dir>/, smpl_256/ (smpl/ for input_mask_type 'smpl'), styles/, segm_256/ and captions.json;
    data_file is the map csv (index column `image`, plus `text`, `styles`, `pose`), pair_file a list of pair csvs
    (`from`, `to`), concatenated in order.  df_filter keeps the pair rows whose cell of that column reads True;
    max_size != 0 takes sklearn's train_test_split(test_size=max_size, random_state=test_split_seed) subset;
    men_factor appends the MEN rows that many times.  image_size and f give the latent size of person_mask / loss_w.

    batches(batch_size) is the interface: dicts of device tensors ready for LatentDiffusion.test_step.  ds[i] returns
    one sample as unbatched tensors through the same device functions at B = 1; it is for inspection.

    Refused keywords (NotImplementedError): dropout, random_style and shuffle=True are training-time randomness, which
    a test split does not use; resize_size and pad are used by no UPGPT model config, only by an autoencoder training
    config.  See the module docstring for the errors raised instead of the reference's skip_sample."""

    def batch_keys(self):
        """The keys of a batch of this dataset, in the reference's order."""
        if self.image_only:
            return ("image", "txt")
        return ("image", "txt", "fname", "src_image", "styles", "smpl", "smpl_image", "person_mask") + (
            ("loss_w",) if self.loss_weight else ())

    def __init__(self, folder, image_dir, pair_file, data_file, df_filter=None, image_size=[256, 192], f=8, resize_size=None,
                 pad=None, max_size=0, test_split_seed=None, input_mask_type='mask', loss_weight=None, image_only=False,
                 dropout=None, random_style=False, men_factor=None, shuffle=False, **kwargs):
        for name, value in (("dropout", dropout), ("random_style", random_style), ("shuffle", shuffle),
                            ("resize_size", resize_size), ("pad", pad)):
            if value:
                raise NotImplementedError("DeepFashionPair(%s=%r) is not supported: %s" % (name, value, (
                    "training-time randomness has no place in the test split's loader" if name in ("dropout", "random_style", "shuffle")
                    else "no UPGPT model config uses it (only an autoencoder training config does)")))
        require(not kwargs, "unknown keywords %s" % sorted(kwargs), TypeError)
        require(input_mask_type in MASK_MODES, "input_mask_type must be one of %s, got %r" % (MASK_MODES, input_mask_type), ValueError)
        self.image_only = bool(image_only)
        self.input_mask_type = input_mask_type
        self.root = Path(folder)
        self.image_root = self.root / image_dir
        self.pose_root = self.root / ('smpl_256' if input_mask_type in ('mask', 'bbox') else 'smpl')
        self.style_root = self.root / 'styles'
        self.segm_root = self.root / 'segm_256'
        with open(str(self.root / 'captions.json')) as fh:
            self.texts = json.load(fh)
        cols, rows = _read_csv(data_file)
        require(all(c in cols for c in ('image', 'text', 'styles', 'pose')), "%s needs the columns image, text, styles, pose; it has "
                "%s" % (data_file, cols), ValueError)
        self.map = {r['image']: r for r in rows}
        self.vae_z_size = tuple(int(x) // int(f) for x in image_size)
        self.loss_weight = dict(loss_weight) if loss_weight else None
        self.segmenter = DeepfashionMMSegmenter()
        self.style_names = style_names
        if self.loss_weight:
            loss_lut(self.loss_weight, self.segmenter)  # (an unknown label is refused here, not at the first batch)
        pair_file = [pair_file] if isinstance(pair_file, (str, os.PathLike)) else list(pair_file)
        pairs = []
        for pf in pair_file:
            cols, rows = _read_csv(pf)
            require('from' in cols and 'to' in cols, "%s needs the columns from, to; it has %s" % (pf, cols), ValueError)
            require(not df_filter or df_filter in cols, "%s has no column %r to filter by" % (pf, df_filter), ValueError)
            pairs += rows
        if df_filter:
            pairs = [r for r in pairs if r[df_filter] == 'True']
        if max_size != 0:
            try:
                from sklearn.model_selection import train_test_split
            except ImportError as e:
                raise ImportError("DeepFashionPair(max_size=%r) takes the reference's subset with sklearn's train_test_split, and "
                                  "sklearn is not installed" % (max_size,)) from e
            _, keep = train_test_split(list(range(len(pairs))), test_size=max_size, random_state=test_split_seed)
            pairs = [pairs[i] for i in keep]
        if men_factor:
            men = [r for r in pairs if r['from'].split('/')[0] == 'MEN']
            pairs = pairs + men * int(men_factor)
        self.pairs = [(r['from'], r['to']) for r in pairs]

    def __len__(self):
        return len(self.pairs)

    # -- rows
    def _row(self, name, where):
        require(name in self.map, "%s: the image %r is not in the map file" % (where, name), ValueError)
        return self.map[name]

    def _samples(self, indices):
        """(source image name, target image name, fname or None) per index."""
        out = []
        for i in indices:
            src, dst = self.pairs[i]
            out.append((src, dst, get_name(src, dst)))
        return out

    def _picture(self, name, first):
        path = self.image_root / name
        arr = _decode(path) if path.is_file() else None
        require(arr is not None, "cannot read the picture %s" % path, ValueError)
        require(first is None or arr.shape == first.shape, "the picture %s is %s, the first picture of its batch %s" % (
            path, arr.shape, None if first is None else first.shape), ValueError)
        return arr

    # -- one batch
    @staticmethod
    def _device(device):
        require(torch.cuda.is_available(), "the batch is assembled on the MI355X (csrc/batch.hip): no GPU is visible and there is "
                "no CPU fallback for the HIP path", RuntimeError)
        return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def _assemble(self, samples, device=None):
        """Decodes and checks every file of the samples on the host (every ValueError is raised here, before a device is
        needed), then uploads and launches."""
        pack, n = _Pack(), len(samples)
        images, txt = [], []
        for _, dst, _ in samples:
            target = self._row(dst, "pair target")
            images.append(self._picture(dst, images[0] if images else None))
            txt.append(self.texts.get(target['text'], ''))
        pack.add("image", images)
        if self.image_only:
            up = pack.upload(self._device(device))
            return {"image": prepare.lr_transform(up["image"], images[0].shape[:2])[1], "txt": txt}
        sources, crops, valid, poses, smpl_pics, masks, segms, mask_files = [], [], [], [], [], [], [], []
        for src, dst, _ in samples:
            source, target = self._row(src, "pair source"), self._row(dst, "pair target")
            sources.append(self._picture(src, images[0]))
            require(source['styles'] != '', "the map row of %s has an empty `styles` cell" % src, ValueError)
            for name in self.style_names:
                f_path = self.style_root / source['styles'] / (name + ".jpg")
                if f_path.exists():
                    crop = _decode(f_path)
                    require(crop is not None and crop.shape == (STYLE_SIZE, STYLE_SIZE, 3), "the style crop %s is not a readable "
                            "%d x %d picture" % (f_path, STYLE_SIZE, STYLE_SIZE), ValueError)
                else:
                    crop = np.zeros((STYLE_SIZE, STYLE_SIZE, 3), dtype=np.uint8)
                crops.append(crop)
                valid.append(int(f_path.exists()))
            pose_path = str(self.pose_root / target['pose'])
            pic = _decode(pose_path + '.jpg') if os.path.isfile(pose_path + '.jpg') else None
            require(pic is not None, "cannot read the smpl picture %s.jpg" % pose_path, ValueError)
            require(not smpl_pics or pic.shape == smpl_pics[0].shape, "the smpl picture %s.jpg is %s, the first of its batch %s" % (
                pose_path, pic.shape, smpl_pics[0].shape if smpl_pics else None), ValueError)
            smpl_pics.append(pic)
            try:
                poses.append(_smpl_pose(pose_path + '.p'))
            except Exception as e:
                raise ValueError("cannot read the smpl parameters %s.p (%s)" % (pose_path, e)) from e
            require(poses[-1].shape == poses[0].shape and poses[-1].dtype == poses[0].dtype, "the smpl parameters %s.p are %s %s, "
                    "the first of their batch %s %s" % (pose_path, poses[-1].dtype, poses[-1].shape, poses[0].dtype, poses[0].shape),
                    ValueError)
            if self.input_mask_type in ('mask', 'bbox'):
                mask_files.append(pose_path + '_mask.png')
                masks.append(_open_map(mask_files[-1], "mask"))
                require(masks[-1].shape == masks[0].shape, "the mask %s is %s, the first of its batch %s" % (
                    mask_files[-1], masks[-1].shape, masks[0].shape), ValueError)
                require(self.input_mask_type != 'bbox' or masks[-1].any(), "the mask %s has no non-zero pixel: it has no bounding "
                        "box" % mask_files[-1], ValueError)
            if self.loss_weight:
                segm_path = str(self.segm_root / dst).replace('.jpg', '_segm.png')
                segms.append(_open_map(segm_path, "label map"))
                require(segms[-1].shape == segms[0].shape, "the label map %s is %s, the first of its batch %s" % (
                    segm_path, segms[-1].shape, segms[0].shape), ValueError)
        win = center_crop_window(smpl_pics[0].shape[0], smpl_pics[0].shape[1], SMPL_CROP)
        for name, arrs in (("src_image", sources), ("crops", crops), ("smpl_pic", smpl_pics), ("mask", masks), ("segm", segms),
                           ("smpl", poses)):
            if arrs:
                pack.add(name, arrs)
        pack.add("valid", [np.array(valid, dtype=np.int32)])
        up = pack.upload(self._device(device))
        size = images[0].shape[:2]
        top, left, ch, cw = win
        smpl_view = up["smpl_pic"][:, top:top + ch, left:left + cw]  # the centre crop: a window into the uploaded bytes
        batch = {"image": prepare.lr_transform(up["image"], size)[1], "txt": txt, "fname": [s[2] for s in samples],
                 "src_image": prepare.lr_transform(up["src_image"], size)[1],
                 "styles": clip_normalize(up["crops"], up["valid"][0]).view(n, len(self.style_names), 3, STYLE_SIZE, STYLE_SIZE),
                 "smpl": up["smpl"], "smpl_image": prepare.lr_transform(smpl_view, [ch, cw])[1]}
        boxes = None
        if self.input_mask_type == 'smpl':
            batch["person_mask"] = person_mask(smpl_view, self.vae_z_size, 'smpl')
        else:
            batch["person_mask"], boxes = person_mask(up["mask"], self.vae_z_size, self.input_mask_type, return_boxes=True)
        if self.loss_weight:
            batch["loss_w"] = loss_weight(up["segm"], self.vae_z_size, self.loss_weight, self.segmenter)
        # (an all-zero mask was refused above, before the upload; the boxes the device found are checked as well.)  The one
        # device -> host copy of a batch, after every launch is enqueued: 16 bytes per sample
        if boxes is not None:
            host = boxes.cpu().numpy()
            for row, path in zip(host, mask_files):
                require(row[0] >= 0, "the mask %s has no non-zero pixel: it has no bounding box" % path, ValueError)
        return batch

    def _finish(self, batch):
        return {k: batch[k] for k in self.batch_keys()}

    def batches(self, batch_size, start=0, stop=None, batch_start=0, batch_step=1):
        """Yields the batch dicts of samples [start, stop) in order, batch_size per dict (the last one may be smaller):
        tensors on the current device, `txt` and `fname` lists of strings.  Keys and key order are the reference's:
        image, txt, fname, src_image, styles, smpl, smpl_image, person_mask, and loss_w when loss_weight is set (image and
        txt only with image_only=True).  image / src_image / smpl_image fp32 [B, H, W, 3]; styles [B, 9, 3, 224, 224];
        smpl [B, 1, n] in the pickles' dtype; person_mask / loss_w [B, 1, h, w].  Per batch: one upload, the launches, and
        in 'bbox' mode one device -> host copy of the [B, 4] boxes (an all-zero mask is refused).
        batch_start, batch_step: only the batches batch_start, batch_start + batch_step, ... of that sequence are built
        (a shard of an evaluation, evaluate.run_validation(rank=, world=)); the others are never decoded."""
        batch_size, batch_start, batch_step = int(batch_size), int(batch_start), int(batch_step)
        require(batch_size >= 1, "batch_size must be positive", ValueError)
        require(batch_start >= 0 and batch_step >= 1, "batch_start must be >= 0 and batch_step >= 1", ValueError)
        idx = list(range(len(self)))[start:stop]
        for i in range(batch_start * batch_size, len(idx), batch_size * batch_step):
            yield self._finish(self._assemble(self._samples(idx[i:i + batch_size])))

    def __getitem__(self, index):
        """ONE sample as a dict of unbatched tensors (strings for txt / fname), built like a batch of one."""
        batch = self._finish(self._assemble(self._samples([index])))
        return {k: v[0] for k, v in batch.items()}


class DeepFashionSample(DeepFashionPair):
    """deepfashion_inshop.DeepFashionSample: source and target are the SAME picture, named by its `image` entry of the map
    file; ds[name] takes that name, not a number.  The keys, in the reference's order: src_image, styles, image, txt, smpl,
    smpl_image, person_mask (no fname, no loss_w).  batches(batch_size, names=...) takes the names to load; by default
    the map file's, in file order."""

    def batch_keys(self):
        return ("src_image", "styles", "image", "txt", "smpl", "smpl_image", "person_mask")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        require(not self.image_only and not self.loss_weight, "DeepFashionSample reads neither image_only nor loss_weight",
                ValueError)

    def _samples(self, names):
        return [(n, n, None) for n in names]

    def batches(self, batch_size, start=0, stop=None, names=None, batch_start=0, batch_step=1):
        batch_size, batch_start, batch_step = int(batch_size), int(batch_start), int(batch_step)
        require(batch_size >= 1, "batch_size must be positive", ValueError)
        require(batch_start >= 0 and batch_step >= 1, "batch_start must be >= 0 and batch_step >= 1", ValueError)
        names = list(self.map if names is None else names)[start:stop]
        for i in range(batch_start * batch_size, len(names), batch_size * batch_step):
            yield self._finish(self._assemble(self._samples(names[i:i + batch_size])))
