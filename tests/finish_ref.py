"""The yardstick of the image-finishing tests: what LatentDiffusion.test_step of the reference does to an image
(ddpm.py:1327-1377), restated with torch CPU ops.  torchvision is not a dependency of the suite, so its three
transforms are restated here operation for operation, each with the torchvision code it stands for; everything else is
the reference's own torch expression.  Nothing in this file calls the code under test."""
import numpy as np
import torch

# ddpm.py:1330-1331: the two T.Normalize of `denorm`, as written in the reference (Python floats)
DENORM_STD_1 = [1 / 0.226862954, 1 / 0.26130258, 1 / 0.27577711]
DENORM_MEAN_2 = [-0.48145466, -0.4578275, -0.40821073]
CONCAT_ORDER = ("src", "samples", "recon", "smpl")  # ddpm.py:1362: torch.cat([src_image, sample, recon_image, smpl_image], 2)


def center_crop_offsets(h, w, crop_size):
    """torchvision.transforms.functional.center_crop(img, output_size): an int becomes (size, size), a one-element
    sequence (size[0], size[0]);
        crop_top = int(round((image_height - crop_height) / 2.0)); crop_left = int(round((image_width - crop_width) / 2.0))
    (Python's round: half to even); an image smaller than the crop would be zero-padded first, which is outside what
    the suite covers."""
    if isinstance(crop_size, (int, np.integer)):
        ch, cw = int(crop_size), int(crop_size)
    elif len(crop_size) == 1:
        ch, cw = int(crop_size[0]), int(crop_size[0])
    else:
        ch, cw = int(crop_size[0]), int(crop_size[1])
    assert h >= ch and w >= cw
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0)), ch, cw


def center_crop(img, crop_size):
    """T.CenterCrop(crop_size)(img) on [..., H, W]: crop(img, crop_top, crop_left, crop_height, crop_width)."""
    top, left, ch, cw = center_crop_offsets(img.shape[-2], img.shape[-1], crop_size)
    return img[..., top:top + ch, left:left + cw]


def normalize(t, mean, std):
    """torchvision.transforms.functional.normalize(tensor, mean, std) on [..., C, H, W] (out of place):
        mean = torch.as_tensor(mean, dtype=tensor.dtype); std = torch.as_tensor(std, dtype=tensor.dtype)
        mean, std = mean.view(-1, 1, 1), std.view(-1, 1, 1); return tensor.clone().sub_(mean).div_(std)"""
    mean = torch.as_tensor(mean, dtype=t.dtype).view(-1, 1, 1)
    std = torch.as_tensor(std, dtype=t.dtype).view(-1, 1, 1)
    return t.clone().sub_(mean).div_(std)


def to_pil_array(pic, saturate=False):
    """T.ToPILImage()(pic) for a float CHW tensor, as the array PIL receives: pic.mul(255).byte(), then
    np.transpose(pic.numpy(), (1, 2, 0)).  `.byte()` of a float outside [0, 256) (or NaN) is undefined behaviour in C;
    saturate=True pins those cases the way include/upk.h documents (NaN -> 0, below 0 -> 0, above 255 -> 255) and is
    the same function everywhere `.byte()` is defined (tests/test_test_step_host.py checks that)."""
    p = pic.mul(255)
    if saturate:
        p = torch.nan_to_num(p, nan=0.0, posinf=255.0, neginf=0.0).clamp(0.0, 255.0)
    return np.ascontiguousarray(p.byte().numpy().transpose(1, 2, 0))


def sample_value(x, crop_size):
    """ddpm.py:1353-1354 on NCHW: crop, then (torch.clamp(x, -1., 1.) + 1.0) / 2.0."""
    return (torch.clamp(center_crop(x.detach(), crop_size), -1., 1.) + 1.0) / 2.0


def input_value(x, crop_size):
    """ddpm.py:1357 on 'b h w c': crop((rearrange(x, 'b h w c -> b c h w') + 1.0) / 2.0)."""
    return center_crop((x.permute(0, 3, 1, 2) + 1.0) / 2.0, crop_size)


def denorm_value(x):
    """ddpm.py:1330-1331, 1374 on [..., 3, H, W]: Normalize(mean 0, std 1 / s), then Normalize(mean -m, std 1)."""
    return normalize(normalize(x, [0., 0., 0.], DENORM_STD_1), DENORM_MEAN_2, [1., 1., 1.])


def finished(log, batch, crop_size, saturate=False):
    """The seven pictures per ddpm.py:1352-1377 as uint8 HWC arrays: {samples, recon, gt, src, smpl, concats: lists over
    the n = len(log['samples']) samples; styles: a list over the batch}.  Inputs are CPU tensors."""
    f32 = lambda t: t.detach().cpu().float()
    vals = {"samples": sample_value(f32(log["samples"]), crop_size), "recon": sample_value(f32(log["reconstruction"]), crop_size),
            "gt": input_value(f32(batch["image"]), crop_size), "src": input_value(f32(batch["src_image"]), crop_size),
            "smpl": input_value(f32(batch["smpl_image"]), crop_size)}
    n = vals["samples"].shape[0]
    out = {k: [to_pil_array(v[i], saturate) for i in range(n)] for k, v in vals.items()}
    out["concats"] = [to_pil_array(torch.cat([vals[k][i] for k in CONCAT_ORDER], 2), saturate) for i in range(n)]
    out["styles"] = [to_pil_array(torch.cat([denorm_value(s) for s in sb], 2), saturate) for sb in f32(batch["styles"])]
    return out
