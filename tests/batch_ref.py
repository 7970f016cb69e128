"""numpy + Pillow + torch-CPU restatement of the reference's test-split loader, DeepFashionPair.__getitem__
(ldm/data/deepfashion_inshop.py:64-272) and Segmenter.get_mask (segm_utils.py:42-47).  torchvision is not a dependency of
the suite, so its transforms are restated operation for operation: T.Resize on a PIL picture is PIL.Image.resize (called
here, NEAREST and BILINEAR, so Pillow itself is the yardstick of every resize), T.ToTensor is HWC -> CHW with a division by
255 for bytes and nothing for floats, T.CenterCrop and T.Normalize as in tests/finish_ref.py and tests/styles_ref.py.
Everything else is the reference's own numpy / torch expression.  Nothing in this file calls the code under test.

make_tree writes a tiny dataset folder with PIL and pickle; nothing of it is committed."""
import csv
import json
import os
import pickle
from pathlib import Path

import numpy as np
import torch
from PIL import Image

import styles_ref as sr

STYLE_NAMES = sr.STYLE_NAMES
SMPL_CROP = (256, 192)
# the sizes at which the NEAREST table was compared with Pillow when the loader was written
NEAREST_PAIRS = [(256, 32), (256, 24), (192, 24), (512, 64), (384, 48), (13, 5), (7, 3), (100, 7), (750, 48), (1101, 64)]
# loss_weight of the test sets of the reference's models/upgpt/mm_512/config.yaml:159-163 and interp_256/config.yaml:160-164.
# 'left-arm' / 'right-arm' are LIP labels: the DeepFashion-MultiModal table has neither (the reference's label2id raises there)
LOSS_WEIGHTS = {"mm_512": {"background": 0.5, "left-arm": 2.0, "right-arm": 2.0, "face": 8.0},
                "interp_256": {"left-arm": 2.0, "right-arm": 2.0, "face": 8.0}}


def known_weights(weights, segmenter):
    """The entries of `weights` whose label the segmenter's table has."""
    ids = label2id(segmenter)
    return {k: v for k, v in weights.items() if k in ids}


def to_tensor(arr):
    """T.ToTensor of a PIL picture / array: [H, W(, C)] -> [C, H, W]; bytes become float32 and are divided by 255, a float
    picture (mode F) or array goes through as it is."""
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.array(arr.transpose(2, 0, 1), order='C'))  # (a writable copy: PIL's arrays are read-only)
    return t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t


def resize(arr, size, resample):
    """T.Resize(size=(h, w), interpolation) on the PIL picture of `arr`."""
    h, w = size
    return np.asarray(Image.fromarray(arr).resize((w, h), resample))


def nearest_index(in_size, out_size):
    """The source index PIL's NEAREST resize reads per output index, read off a resized index ramp (two rows of int32)."""
    ramp = np.arange(in_size, dtype=np.int32)[None].repeat(2, 0)
    return np.asarray(Image.fromarray(ramp, mode="I").resize((out_size, 2), Image.NEAREST))[0].astype(np.int64)


def image_transform(u8):
    """T.ToTensor, rearrange(x * 2. - 1., 'c h w -> h w c')."""
    return (to_tensor(u8) * 2. - 1.).permute(1, 2, 0).contiguous()


def center_crop(arr, size=SMPL_CROP):
    """T.CenterCrop(size) on an array [H, W, ...] at least that large."""
    ch, cw = size
    h, w = arr.shape[:2]
    assert h >= ch and w >= cw
    top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
    return np.ascontiguousarray(arr[top:top + ch, left:left + cw])


def get_bbox(mask):
    """deepfashion_inshop.py:164-171, verbatim."""
    x = np.nonzero(np.mean(mask, 1))[0]
    xmin, xmax = x[0], x[-1]
    y = np.nonzero(np.mean(mask, 0))[0]
    ymin, ymax = y[0], y[-1]
    bbox = np.zeros_like(mask, np.uint8)
    bbox[xmin:xmax + 1, ymin:ymax + 1] = 1
    return bbox


def box_of(mask):
    """(r0, r1, c0, c1) of get_bbox, or four times -1 for a map without a non-zero byte."""
    r, c = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    return [int(r[0]), int(r[-1]), int(c[0]), int(c[-1])] if r.size else [-1] * 4


def person_mask(arr, size, mode):
    """mask_transform (deepfashion_inshop.py:141-152, 228-241) -> fp32 [1, h, w].  'mask' / 'bbox': arr is the mask [H, W];
    'smpl': arr is the centre-cropped smpl picture [256, 192, 3]."""
    if mode == 'smpl':
        x = to_tensor(resize(arr, size, Image.BILINEAR))
        return torch.mean(x, 0, keepdim=True) * 2. - 1.
    if mode == 'bbox':
        arr = get_bbox(arr)  # (the kept bug: 1, not 255)
    return to_tensor(resize(arr, size, Image.NEAREST)) * 2. - 1.


def bbox_or_background(arr, size):
    """person_mask 'bbox' with the kernel's convention for a map the reference cannot take (x[0] raises): all background."""
    if not arr.any():
        return torch.full((1,) + tuple(size), -1.0)
    return person_mask(arr, size, 'bbox')


def label2id(segmenter):
    return {name: i for i, name in enumerate(sr.TABLES[segmenter][0])}


def get_mask(segm, mask_val, segmenter='mm', default_value=1.0):
    """Segmenter.get_mask, segm_utils.py:42-47."""
    ids = label2id(segmenter)
    mask = np.full(segm.shape, default_value, dtype=np.float32)
    if mask_val:
        for label, value in mask_val.items():
            mask[segm == ids[label]] = value
    return mask


def loss_w(segm, size, weights, segmenter='mm'):
    """loss_w_transform(Image.fromarray(get_mask(...))): a mode-F picture through NEAREST and ToTensor -> fp32 [1, h, w]."""
    return to_tensor(resize(get_mask(segm, weights, segmenter), size, Image.NEAREST))


def clip_transform(u8):
    """T.ToTensor + T.Normalize on bytes [..., 224, 224, 3] -> fp32 tensor [..., 3, 224, 224]."""
    return torch.from_numpy(sr.clip_norm(u8))


def smpl_pose(path):
    """deepfashion_inshop.py:245-251."""
    with open(str(path), 'rb') as f:
        smpl_params = pickle.load(f)
    pred_pose = smpl_params[0]['pred_body_pose']
    pred_betas = smpl_params[0]['pred_betas']
    pred_camera = np.expand_dims(smpl_params[0]['pred_camera'], 0)
    smpl_pose = np.concatenate((pred_pose, pred_betas, pred_camera), axis=1)
    return to_tensor(smpl_pose).view((1, -1))


def convert_fname(x):
    a, b = os.path.split(x)
    i = b.rfind('_')
    x = a + '/' + b[:i] + b[i + 1:]
    return 'fashion' + x.split('.jpg')[0].replace('id_', 'id').replace('/', '')


def get_name(src, dst):
    return convert_fname(src) + '___' + convert_fname(dst)


def read_csv(path):
    with open(str(path), newline='') as f:
        return list(csv.DictReader(f))


def rgb(path):
    return np.asarray(Image.open(str(path)).convert("RGB"))


class RefPair:
    """DeepFashionPair.__getitem__ for a test split, without its try / except."""

    def __init__(self, folder, image_dir, pair_file, data_file, image_size=(256, 192), f=8, input_mask_type='mask',
                 loss_weight=None):
        self.root = Path(folder)
        self.image_root = self.root / image_dir
        self.pose_root = self.root / ('smpl_256' if input_mask_type in ('mask', 'bbox') else 'smpl')
        self.style_root, self.segm_root = self.root / 'styles', self.root / 'segm_256'
        self.texts = json.load(open(str(self.root / 'captions.json')))
        self.map = {r['image']: r for r in read_csv(data_file)}
        self.df = [r for f_ in pair_file for r in read_csv(f_)]
        self.vae_z_size = tuple(x // f for x in image_size)
        self.mode, self.loss_weight = input_mask_type, loss_weight

    def __len__(self):
        return len(self.df)

    def styles(self, source):
        out = []
        for style_name in STYLE_NAMES:
            f_path = self.style_root / source['styles'] / f'{style_name}.jpg'
            if f_path.exists():
                out.append(clip_transform(rgb(f_path)))
            else:
                out.append(clip_transform(np.zeros((224, 224, 3), dtype=np.uint8)))  # clip_norm(torch.zeros(3, 224, 224))
        return torch.stack(out)

    def __getitem__(self, index):
        row = self.df[index]
        target, source = self.map[row['to']], self.map[row['from']]
        data = {"image": image_transform(rgb(self.image_root / target['image'])), "txt": self.texts.get(target['text'], '')}
        data.update({"fname": get_name(row['from'], row['to']),
                     "src_image": image_transform(rgb(self.image_root / source['image'])), "styles": self.styles(source)})
        pose_path = str(self.pose_root / target['pose'])
        smpl_image = center_crop(rgb(pose_path + '.jpg'))
        if self.mode == 'smpl':
            mask = person_mask(smpl_image, self.vae_z_size, 'smpl')
        else:
            mask = person_mask(np.array(Image.open(pose_path + '_mask.png')), self.vae_z_size, self.mode)
        data.update({'smpl': smpl_pose(pose_path + '.p'), 'smpl_image': image_transform(smpl_image), 'person_mask': mask})
        if self.loss_weight:
            segm = np.array(Image.open(str(self.segm_root / target['image']).replace('.jpg', '_segm.png')))
            data.update({'loss_w': loss_w(segm, self.vae_z_size, self.loss_weight)})
        return data


def collate(samples):
    """torch's default_collate for these dicts: tensors stacked, strings listed."""
    return {k: torch.stack([s[k] for s in samples]) if torch.is_tensor(samples[0][k]) else [s[k] for s in samples]
            for k in samples[0]}


# ---------------------------------------------------------------------------------------------------------------------
# a tiny dataset folder

def image_name(i):
    return "%s/Tees_Tanks/id_%08d/%02d_%d_front.jpg" % ("MEN" if i % 2 else "WOMEN", 100 + i, 1 + i % 3, 1 + i % 4)


def make_tree(root, n_images=6, pairs=((0, 1), (1, 2), (2, 3), (3, 4), (4, 5)), pic=(64, 48), mask=(64, 64), smpl_pic=(256, 256),
              pose_dtype=np.float32, missing_styles=((1, 'hair'),), seed=0):
    """Writes root/{img_256, smpl_256, smpl, styles, segm_256}/..., captions.json, map.csv and two pair files (the pairs split
    after the third); returns the keywords DeepFashionPair and RefPair share.  Every image has the styles of STYLE_NAMES but
    'accesories' (which no segmenter produces) and the (image, style) pairs of `missing_styles`.  Masks: rectangles of
    255 (even images) or 1 (odd images), image 2's stored as a mode-P picture."""
    root = Path(root)
    rng = np.random.default_rng(seed)
    captions, rows = {}, []
    for i in range(n_images):
        name = image_name(i)
        stem = name[:-len(".jpg")]
        for d in ("img_256", "smpl_256", "smpl", "segm_256"):
            os.makedirs(str((root / d / name).parent), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, pic + (3,), dtype=np.uint8)).save(str(root / "img_256" / name), quality=95)
        sdir = root / "styles" / stem
        os.makedirs(str(sdir), exist_ok=True)
        for s in STYLE_NAMES[:-1]:
            if (i, s) not in missing_styles:
                Image.fromarray(rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)).save(str(sdir / (s + ".jpg")), quality=90)
        m = np.zeros(mask, dtype=np.uint8)
        m[3 + 5 * i:mask[0] - 9 - 2 * i, 7 + 3 * i:mask[1] - 4 - 6 * i] = 1 if i % 2 else 255
        im = Image.fromarray(m)
        if i == 2:
            im = im.convert("P")
        for d in ("smpl_256", "smpl"):
            Image.fromarray(rng.integers(0, 256, smpl_pic + (3,), dtype=np.uint8)).save(str(root / d / name), quality=95)
            pose = [{'pred_body_pose': rng.standard_normal((1, 72)).astype(pose_dtype),
                     'pred_betas': rng.standard_normal((1, 10)).astype(pose_dtype),
                     'pred_camera': rng.standard_normal(3).astype(pose_dtype)}]
            with open(str(root / d / (stem + ".p")), 'wb') as f:
                pickle.dump(pose, f)
            im.save(str(root / d / (stem + "_mask.png")))
        Image.fromarray(rng.integers(0, 24, pic, dtype=np.uint8)).save(str(root / "segm_256" / (stem + "_segm.png")))
        captions["text_%d" % i] = "a person wearing garment number %d" % i
        rows.append({"image": name, "text": "text_%d" % i if i != 3 else "no_such_caption", "styles": stem, "pose": stem})
    json.dump(captions, open(str(root / "captions.json"), "w"))
    with open(str(root / "map.csv"), "w", newline='') as f:
        wr = csv.DictWriter(f, ["image", "text", "styles", "pose"])
        wr.writeheader()
        wr.writerows(rows)
    files = []
    for k, part in enumerate((pairs[:3], pairs[3:])):
        files.append(str(root / ("pairs_%d.csv" % k)))
        with open(files[-1], "w", newline='') as f:
            wr = csv.DictWriter(f, ["from", "to", "keep"])
            wr.writeheader()
            wr.writerows({"from": image_name(a), "to": image_name(b), "keep": str(a != 1)} for a, b in part)
    return dict(folder=str(root), image_dir="img_256", pair_file=files, data_file=str(root / "map.csv"))
