"""LatentDiffusion.test_step (ddpm.py:1327-1377): a test batch -> results/{samples,concats,styles,gt,recon,src,smpl}.

The reference finishes every image on the host with a chain of torch / torchvision element-wise ops (centre crop,
clamp, rescale, CLIP de-normalisation, width concat, ToPILImage's mul(255).byte()).  Here all of it is
upk_image_finish_u8 (include/upk.h) on the current stream, writing uint8 HWC pictures into ONE device buffer per call;
that buffer crosses to pinned host memory in one copy behind one synchronise, and PIL encodes what arrives.  The
arithmetic contract (one correctly rounded fp32 operation at a time, in the reference's order; truncation; saturation
where the reference's .byte() is undefined) is stated in include/upk.h and DESIGN.md 16.

run_metrics is the step after it (scripts/eval_metrics.py): results/gt against results/samples -> metrics.csv and
metrics.txt with per-image SSIM and MS-SSIM from upk_ssim_u8 (upgpt_amd/metrics.py) and, given the two
public weight files, LPIPS (upgpt_amd/lpips.py) and, given pytorch_fid's Inception weights, the FID line of
metrics.txt (upgpt_amd/fid.py); `python -m upgpt_amd.evaluate --dir <save_dir>/results` runs it.

run_validation is the validation epoch (val/loss_simple_ema, the number a checkpoint is picked by); with noise_seed= every
sample meets the same keyed draws whatever its batch, lane or rank shard, and merge_validation forms the epoch means of
shards.

run_upscale is the second model's pass over a results tree: results/samples-sized pictures -> the `lr` conditioning on the
device (upgpt_amd/prepare.py, upk_resize_bilinear_u8) -> the upscale model -> results/upscaled.

run_interpolation is the demo's "Interpolate" flow: InferenceModel.interpolate -> interp/interp_{i}.jpg, interp_strip.jpg
and, with an upscale model, interp_upscaled/interp_{i}.png.
"""
import os
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._check import require

FOLDERS = ("samples", "concats", "styles", "gt", "recon", "src", "smpl")
CONCAT_ORDER = ("src", "samples", "recon", "smpl")  # ddpm.py:1362, left to right
# T.Normalize(mean=0, std=[1 / s]) then T.Normalize(mean=[-m], std=1) (ddpm.py:1330-1331): v / d - m with the quotient
# 1 / s formed in Python double and rounded to fp32, as T.Normalize does with its std list.  (0.226862954 is the
# reference's own first constant.)
DENORM_D = tuple(np.float32(1 / s) for s in (0.226862954, 0.26130258, 0.27577711))
DENORM_M = tuple(np.float32(-m) for m in (0.48145466, 0.4578275, 0.40821073))
# log_images arguments of the reference's test_step (ddpm.py:1348-1350); N is added per batch
LOG_DEFAULTS = dict(unconditional_guidance_scale=3.0, unconditional_guidance_label=["txt"])


class ResultDir:
    """The one attribute test_step reads of a Lightning logger, for callers without Lightning: model.logger =
    ResultDir(path)."""

    def __init__(self, save_dir):
        self.save_dir = str(save_dir)


def center_crop_window(h, w, crop_size):
    """(top, left, crop_h, crop_w) of torchvision's CenterCrop(crop_size) on an h x w image: top = int(round((h -
    crop_h) / 2.0)) with Python's round (x.5 goes to the even neighbour), likewise left.  crop_size: an int (square) or
    [crop_h, crop_w].  An image smaller than the crop is REFUSED (ValueError): torchvision would zero-pad it first, no
    UPGPT config asks for that."""
    if isinstance(crop_size, (int, np.integer)):
        ch = cw = int(crop_size)
    else:
        size = [int(v) for v in crop_size]
        require(len(size) in (1, 2), "crop_size must be an int or [h, w], got %r" % (crop_size,), ValueError)
        ch, cw = size[0], size[-1]
    require(ch > 0 and cw > 0, "crop_size must be positive, got %r" % (crop_size,), ValueError)
    require(h >= ch and w >= cw, "image %d x %d is smaller than crop_size %d x %d (the zero padding torchvision's "
            "CenterCrop would add is not supported)" % (h, w, ch, cw), ValueError)
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0)), ch, cw


def finish_images(src, dst, layout, mode, window=None, dst_x=0, denorm=None):
    """One upk_image_finish_u8 launch on the current stream.
    src: fp32 device tensor, [B, 3, H, W] (layout _lib.LAYOUT_NCHW) or [B, H, W, 3] (LAYOUT_NHWC); each sample dense,
    any batch stride.  window: (top, left, crop_h, crop_w) of the source, default the whole image.
    dst: uint8 device tensor [B, rows >= crop_h, width, 3], pixels dense inside a row (any row pitch / sample stride);
    columns [dst_x, dst_x + crop_w) of its first crop_h rows are written, nothing else.
    mode: _lib.FINISH_SAMPLE / FINISH_INPUT / FINISH_DENORM; denorm: (d, m) per-channel triples, default the CLIP
    constants of the reference.  No CPU fallback: host tensors raise."""
    require(torch.is_tensor(src) and torch.is_tensor(dst) and src.is_cuda and dst.is_cuda,
            "finish_images needs device tensors: there is no CPU fallback for the HIP path", RuntimeError)
    require(src.dtype == torch.float32 and src.dim() == 4, "finish_images: src must be a 4-d fp32 tensor", TypeError)
    require(dst.dtype == torch.uint8 and dst.dim() == 4 and dst.shape[3] == 3, "finish_images: dst must be uint8 [B, H, W, 3]",
            TypeError)
    nhwc = layout == _lib.LAYOUT_NHWC
    b, (h, w) = src.shape[0], (src.shape[1:3] if nhwc else src.shape[2:4])
    require(src.shape[3 if nhwc else 1] == 3, "finish_images: 3-channel images only, got %s" % (tuple(src.shape),), ValueError)
    require(src[0].is_contiguous() and src.stride(0) >= 0, "finish_images: every source sample must be dense", ValueError)
    require(dst.stride(3) == 1 and dst.stride(2) == 3, "finish_images: dst pixels must be dense inside a row", ValueError)
    top, left, ch, cw = (0, 0, h, w) if window is None else window
    require(dst.shape[0] == b and dst.shape[1] >= ch and dst_x >= 0 and dst_x + cw <= dst.shape[2],
            "finish_images: window %s at x = %d does not fit dst %s" % ((top, left, ch, cw), dst_x, tuple(dst.shape)), ValueError)
    dm = None
    if mode == _lib.FINISH_DENORM:
        d, m = (DENORM_D, DENORM_M) if denorm is None else denorm
        dm = list(d) + list(m)
    _lib.get_context(src.device).image_finish(src, layout, b, h, w, src.stride(0), top, left, ch, cw, dst, dst.stride(1),
                                              dst_x, dst.stride(0), mode, dm)


def _sections(n, ch, cw, styles_shape):
    """name -> (byte offset, shape) of the uint8 pictures inside the one buffer (offsets multiples of 16)."""
    bs, s, _, sh, sw = styles_shape
    shapes = [(k, (n, ch, cw, 3)) for k in ("samples", "recon", "gt", "src", "smpl")]
    shapes += [("concats", (n, ch, len(CONCAT_ORDER) * cw, 3)), ("styles", (bs, sh, s * sw, 3))]
    out, off = {}, 0
    for k, shp in shapes:
        out[k] = (off, shp)
        off += (int(np.prod(shp)) + 15) // 16 * 16
    return out, off


def finished_arrays(model, batch, log):
    """The device part of test_step: {samples, recon, gt, src, smpl, concats, styles} -> uint8 host arrays ([n, crop_h,
    crop_w, 3]; concats [n, crop_h, 4 crop_w, 3] = src | sample | recon | smpl; styles [B, 224, S 224, 3], the crops of
    a sample side by side, not centre-cropped).  n = the number of images log_images returned, B = the batch's.
    Every picture is written by upk_image_finish_u8 launches on the current stream into one uint8 device buffer, which
    is copied to pinned host memory once, behind one synchronise; no fp32 image goes to the host and no torch
    element-wise op touches a pixel."""
    dev = model.device
    samples, recon = log["samples"], log["reconstruction"]
    n = int(samples.shape[0])
    require(recon.shape == samples.shape, "reconstruction %s and samples %s differ in shape" % (
        tuple(recon.shape), tuple(samples.shape)), ValueError)
    win = center_crop_window(samples.shape[2], samples.shape[3], model.crop_size)
    ch, cw = win[2], win[3]
    nchw, nhwc = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC
    comps = {"samples": (samples.to(dev, torch.float32), nchw, _lib.FINISH_SAMPLE, win),
             "recon": (recon.to(dev, torch.float32), nchw, _lib.FINISH_SAMPLE, win)}
    for name, key in (("gt", "image"), ("src", "src_image"), ("smpl", "smpl_image")):
        x = batch[key]
        require(x.dim() == 4 and x.shape[0] >= n and x.shape[3] == 3, "batch[%r] must be [B >= %d, H, W, 3], got %s" % (
            key, n, tuple(x.shape)), ValueError)
        comps[name] = (x[:n].to(dev, torch.float32).contiguous(), nhwc, _lib.FINISH_INPUT,
                       center_crop_window(x.shape[1], x.shape[2], model.crop_size))
    styles = batch["styles"]
    require(styles.dim() == 5 and styles.shape[2] == 3, "batch['styles'] must be [B, S, 3, H, W] image crops, got %s" % (
        tuple(styles.shape),), ValueError)
    styles = styles.to(dev, torch.float32).contiguous()
    sect, total = _sections(n, ch, cw, tuple(styles.shape))
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    view = {k: buf[off:off + int(np.prod(shp))].view(shp) for k, (off, shp) in sect.items()}
    for name, (src, layout, mode, w) in comps.items():  # every component on its own ...
        finish_images(src, view[name], layout, mode, window=w)
    for slot, name in enumerate(CONCAT_ORDER):  # ... and into its slot of the strip: the width concat
        src, layout, mode, w = comps[name]
        finish_images(src, view["concats"], layout, mode, window=w, dst_x=slot * cw)
    for s in range(styles.shape[1]):
        finish_images(styles[:, s], view["styles"], nchw, _lib.FINISH_DENORM, dst_x=s * styles.shape[4])
    host = torch.empty(total, dtype=torch.uint8, pin_memory=buf.is_cuda)
    host.copy_(buf, non_blocking=True)
    if buf.is_cuda:
        torch.cuda.current_stream(dev).synchronize()
    arr = host.numpy()
    return {k: arr[off:off + int(np.prod(shp))].reshape(shp) for k, (off, shp) in sect.items()}


def test_step(model, batch, batch_idx, **log_kwargs):
    """LatentDiffusion.test_step (see its docstring)."""
    from PIL import Image
    save_dir = getattr(getattr(model, "logger", None), "save_dir", None)
    require(save_dir is not None, "test_step writes under model.logger.save_dir, and this model has no logger with a "
            "save_dir: set model.logger = upgpt_amd.evaluate.ResultDir(path) (or use evaluate.run_test)", ValueError)
    roots = {k: Path(save_dir) / "results" / k for k in FOLDERS}
    for r in roots.values():
        os.makedirs(str(r), exist_ok=True)
    kw = dict(LOG_DEFAULTS, N=len(batch), use_ema=model.use_ema)
    kw.update(log_kwargs)
    with torch.no_grad():
        log = model.log_images(batch, **kw)
        arrays = finished_arrays(model, batch, log)
    names = list(batch["fname"])
    per_sample = [k for k in FOLDERS if k != "styles"]
    for i, fname in zip(range(arrays["samples"].shape[0]), names):
        for k in per_sample:
            Image.fromarray(arrays[k][i]).save(roots[k] / f"{fname}.jpg")
    for fname, strip in zip(names, arrays["styles"]):  # (every fname: this loop is not capped by N)
        Image.fromarray(strip).save(roots["styles"] / f"{fname}.jpg")
    return None


test_step.__test__ = False  # (not a pytest test, whatever imports it)


def _keyed_batches(model, batches, noise_seed):
    """(index, batch, NoiseKeys or None) per batch; sample ids are the running sample indices over the batches."""
    from .rng import NoiseKeys
    seen = 0
    for j, batch in enumerate(batches):
        keys = None
        if noise_seed is not None:  # (without a seed the batch is not looked at: any batch object passes through)
            n = int(batch[model.first_stage_key].shape[0])
            keys = NoiseKeys(noise_seed, range(seen, seen + n), device=model.device)
            keys.keys  # (uploaded here, with the batch: under host_io() when lanes take their batches)
            seen += n
        yield j, batch, keys


def run_test(model, batches, save_dir, lanes=1, noise_seed=None, **log_kwargs):
    """What trainer.test(model, data) does with test_step (main.py:798), without Lightning: model.logger =
    ResultDir(save_dir) for the duration (set once, also with lanes), then test_step(batch, i, **log_kwargs) per batch.
    noise_seed (an int below 2^64): every batch samples with keyed noise, log_images(noise_keys=NoiseKeys(noise_seed,
    ids)) — `ids` are the RUNNING sample indices over `batches` (first sample of the first batch = 0), so a sample's
    noise, and with it its picture up to the GEMM tilings of its batch size, depends on neither batch_size nor the batch
    it falls into; for run_split they are the dataset's indices.  The torch generator is not used for sampling.
    lanes > 1: the batches are spread over that many execution lanes of a LanePool (upgpt_amd/lanes.py) and `noise_seed`
    is required — without it log_images draws from the process-wide device generator and the lanes would interleave
    those draws in an undefined order (ValueError).  Each lane thread takes the next batch from `batches` when it is free
    (the iterator is advanced under _lib.host_io(): the loader's uploads and launches run on the taking lane's stream and
    never overlap another lane's graph capture) and runs test_step in its lane — sampling, finishing, the one device ->
    host copy and PIL's JPEG encoding all happen in the lane thread, outside the lock.  Files and bytes equal the
    lanes=1 run with the same noise_seed (tests/test_lanes_eval_gpu.py).  An exception in a lane ends the run — the
    other lanes finish the batch they are on and take no further one — and is re-raised; nothing is retried."""
    lanes = int(lanes)
    require(lanes >= 1, "lanes must be >= 1", ValueError)
    require(lanes == 1 or noise_seed is not None, "lanes > 1 needs noise_seed: without keyed noise log_images draws from the "
            "process-wide device generator, and lane threads would interleave those draws in an undefined order", ValueError)
    had, prev = "logger" in vars(model), vars(model).get("logger")
    model.logger = ResultDir(save_dir)
    try:
        work = _keyed_batches(model, batches, noise_seed)
        kw = lambda keys: log_kwargs if keys is None else dict(log_kwargs, noise_keys=keys)
        if lanes == 1:
            for j, batch, keys in work:
                model.test_step(batch, j, **kw(keys))
        else:
            _run_lanes(model, work, lanes, lambda item: model.test_step(item[1], item[0], **kw(item[2])))
    finally:
        if had:
            model.logger = prev
        else:
            del model.logger
    return Path(save_dir) / "results"


def _run_lanes(model, work, lanes, step, ema=True):
    """The lane loop of run_test / run_validation / run_upscale: every lane thread takes the next item of the iterator
    `work` when it is free — under the take lock and _lib.host_io(), so whatever the iterator does to produce an item
    (decoding, uploads, loader launches) runs on the taking lane's stream, one taker at a time — and calls step(item) in
    its lane, outside the lock.  ema: one process-wide EMA scope around the run (the flows that only sample); a flow that
    alternates the weight sets per batch passes False and selects per thread (ema_scope(local=True))."""
    import contextlib
    import threading

    from .lanes import LanePool
    take, failed = threading.Lock(), threading.Event()

    def lane_loop(i):
        while not failed.is_set():
            try:
                with take, _lib.host_io():  # (batch assembly: uploads and loader launches, on this lane's stream)
                    item = next(work, None)
                if item is None:
                    return
                step(item)
            except BaseException:
                failed.set()
                raise

    # one EMA scope around the run: the weight override does not go out and in again between the lanes' batches
    with LanePool(lanes, device=model.device) as pool, (model.ema_scope() if ema else contextlib.nullcontext()):
        pool.run(lane_loop, lanes)  # "step" i = the whole loop of lane i, on lane i's thread and stream


def run_split(model, dataset, save_dir, batch_size=8, lanes=1, noise_seed=None, **log_kwargs):
    """run_test over a dataset of this package (upgpt_amd/data.py: DeepFashionPair, the `target` of the model configs'
    test set): dataset.batches(batch_size) assembles every batch on the device, test_step writes its seven folders.
    "dataset folder -> results/" with nothing supplied but paths and weights; run_metrics is the step after it.
    lanes / noise_seed: as run_test; dataset.batches yields the samples in index order from 0 and does not expose the
    indices, so the running sample index run_test keys the noise with IS the dataset index."""
    return run_test(model, dataset.batches(int(batch_size)), save_dir, lanes=lanes, noise_seed=noise_seed, **log_kwargs)


VAL_COLUMNS = ("id", "t", "simple", "plain", "t_ema", "simple_ema", "plain_ema")


def shard_batches(n_batches, rank, world):
    """The batch indices a call with (rank, world) processes: j in [0, n_batches) with j % world == rank."""
    rank, world = int(rank), int(world)
    require(world >= 1 and 0 <= rank < world, "rank must be in [0, world), got rank %d of %d" % (rank, world), ValueError)
    return list(range(rank, int(n_batches), world))


def _shard_work(dataset, batch_size, rank, world, max_batches):
    """(global batch index j, id of its first sample, batch) for the batches of this shard, in order.  A dataset whose
    batches() takes batch_start / batch_step (upgpt_amd/data.py) is asked for its own batches only — the others are never
    decoded — and the first id is j * batch_size (every batch but the last is full); any other source is walked through
    and counted."""
    import inspect
    fn = getattr(dataset, "batches", None) if batch_size is not None else None  # (None: `dataset` IS the batches)
    limit = None if max_batches is None else int(max_batches)
    if fn is not None and "batch_step" in inspect.signature(fn).parameters:
        for k, batch in enumerate(fn(batch_size, batch_start=rank, batch_step=world)):
            j = rank + k * world
            if limit is not None and j >= limit:
                return
            yield j, j * batch_size, batch
        return
    seen = 0
    for j, batch in enumerate(fn(batch_size) if fn is not None else dataset):
        if limit is not None and j >= limit:
            return
        first, seen = seen, seen + _batch_len(batch)
        if j % world == rank:
            yield j, first, batch


def _batch_len(batch):
    for v in batch.values():
        if torch.is_tensor(v) or isinstance(v, (list, tuple)):
            return len(v)
    raise ValueError("a batch without a tensor or a list: its size is unknown")


def _val_schedule(model, lvlb, logvar):
    """What the epoch means need besides the per-sample table (val_schedule.json): the loss weights and the two tables
    indexed by t (host sequences of the fp32 values widened to double)."""
    return {"prefix": "train" if model.training else "val", "l_simple_weight": float(model.l_simple_weight),
            "original_elbo_weight": float(model.original_elbo_weight), "learn_logvar": bool(model.learn_logvar),
            "lvlb_weights": [float(v) for v in lvlb], "logvar": [float(v) for v in logvar]}


def _ordered_sum(values):
    s = 0.0
    for v in values:  # (in sample-index order, one fp64 addition at a time: the order is part of the result)
        s += float(v)
    return s


def validation_means(table, sched):
    """The epoch means of a keyed validation run from its per-sample table: fp64 [N, 6] in sample-index order, columns
    t, simple, plain, t_ema, simple_ema, plain_ema (upk_p_losses_f32's per-sample values).  Formed as upk_p_losses_f32
    forms a batch's values, over the whole epoch and in fp64: loss_simple = mean simple, loss_gamma = mean(simple /
    exp(logvar[t]) + logvar[t]), loss_vlb = mean(lvlb_weights[t] * plain), loss = l_simple_weight * loss_gamma +
    original_elbo_weight * loss_vlb — Lightning's on_epoch mean of the batch means, weighted by the batch sizes, is the
    mean over the samples.  Keys and their order are validation_step's."""
    import math
    table = np.asarray(table, dtype=np.float64)
    require(table.ndim == 2 and table.shape[1] == 6 and table.shape[0] > 0, "validation_means: an [N, 6] table", ValueError)
    n, p = table.shape[0], sched["prefix"]
    lvlb, logvar = sched["lvlb_weights"], sched["logvar"]
    out = {}
    for suffix, off in (("", 0), ("_ema", 3)):
        t = [int(v) for v in table[:, off]]
        require(all(0 <= v < len(lvlb) for v in t), "validation_means: a timestep outside the schedule", ValueError)
        simple, plain = table[:, off + 1], table[:, off + 2]
        m_simple = _ordered_sum(simple) / n
        m_gamma = _ordered_sum(float(s) / math.exp(logvar[k]) + logvar[k] for s, k in zip(simple, t)) / n
        m_vlb = _ordered_sum(lvlb[k] * float(q) for q, k in zip(plain, t)) / n
        out[p + "/loss_simple" + suffix] = m_simple
        if sched["learn_logvar"]:
            out[p + "/loss_gamma" + suffix] = m_gamma
            out["logvar" + suffix] = _ordered_sum(logvar) / len(logvar)
        out[p + "/loss_vlb" + suffix] = m_vlb
        out[p + "/loss" + suffix] = sched["l_simple_weight"] * m_gamma + sched["original_elbo_weight"] * m_vlb
    return out


def _write_val_samples(path, ids, table):
    with open(path, "w") as f:
        f.write(",".join(VAL_COLUMNS) + "\n")
        for i, row in zip(ids, table):  # (repr of a double reads back as the same double)
            f.write("%d,%d,%r,%r,%d,%r,%r\n" % (i, int(row[0]), float(row[1]), float(row[2]), int(row[3]), float(row[4]),
                                                 float(row[5])))


def _read_val_samples(path):
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    require(lines and tuple(lines[0].split(",")) == VAL_COLUMNS, "%s: the header is not %s" % (path, ",".join(VAL_COLUMNS)),
            ValueError)
    ids, rows = [], []
    for ln in lines[1:]:
        cells = ln.split(",")
        require(len(cells) == len(VAL_COLUMNS), "%s: a row of %d cells" % (path, len(cells)), ValueError)
        ids.append(int(cells[0]))
        rows.append([float(c) for c in cells[1:]])
    return ids, rows


def merge_validation(save_dir):
    """The epoch means of a validation run that was evaluated in shards: reads every <save_dir>/val_samples.rank<r>of<w>.csv
    (run_validation(rank=r, world=w, save_dir=...)) and val_schedule.json, puts the rows into sample-index order and forms
    the means with validation_means — bit for bit the values of the world = 1 run with the same batch_size and noise_seed.
    Refused (ValueError): no shard, shards of different `world`, a rank missing or present twice, a sample id in two
    rows, and a gap in the ids 0 .. N - 1.  Writes val_metrics.json and the merged val_samples.csv; returns the means.
    No collective and no torch.distributed call: the shards meet in the directory."""
    import json
    import re
    save_dir = Path(save_dir)
    found = {}
    for name in sorted(os.listdir(str(save_dir))):
        m = re.fullmatch(r"val_samples\.rank(\d+)of(\d+)\.csv", name)
        if m:
            found[name] = (int(m.group(1)), int(m.group(2)))
    require(found, "merge_validation: no val_samples.rank<r>of<w>.csv in %s" % save_dir, ValueError)
    worlds = sorted({w for _, w in found.values()})
    require(len(worlds) == 1, "merge_validation: shards of different world sizes %s" % worlds, ValueError)
    ranks = sorted(r for r, _ in found.values())
    require(ranks == list(range(worlds[0])), "merge_validation: ranks %s of %d: every rank once" % (ranks, worlds[0]), ValueError)
    ids, rows = [], []
    for name in found:
        i, r = _read_val_samples(save_dir / name)
        ids += i
        rows += r
    require(len(set(ids)) == len(ids), lambda: "merge_validation: sample ids in more than one row: %s" % sorted(
        {i for i in ids if ids.count(i) > 1})[:8], ValueError)
    order = sorted(range(len(ids)), key=ids.__getitem__)
    ids = [ids[k] for k in order]
    require(ids == list(range(len(ids))), lambda: "merge_validation: the sample ids have gaps: %s missing" % sorted(
        set(range(max(ids) + 1)) - set(ids))[:8], ValueError)
    table = np.array([rows[k] for k in order], dtype=np.float64)
    with open(save_dir / "val_schedule.json") as f:
        sched = json.load(f)
    means = validation_means(table, sched)
    _write_val_samples(save_dir / "val_samples.csv", ids, table)
    with open(save_dir / "val_metrics.json", "w") as f:
        json.dump(means, f, indent=1)
    return means


def run_validation(model, dataset, batch_size=8, seed=0, max_batches=None, save_dir=None, lanes=1, noise_seed=None, rank=0,
                   world=1):
    """The validation epoch of trainer.validate without Lightning: dataset.batches(batch_size) (upgpt_amd/data.py; any
    object with that method, or a plain iterable of batch dicts) through model.validation_step, and the epoch means of
    its keys as Lightning's on_epoch reduction forms them — every batch's value weighted by the batch's size — as a plain
    {key: float} dict, e.g. 'val/loss_simple_ema', the number the UPGPT configs monitor.  With save_dir they are also
    written to <save_dir>/val_metrics.json.
    Without noise_seed the timesteps, the noise and the posterior samples come from the device generator, seeded with
    `seed` for the duration (the generators' states are put back afterwards), so a run is repeatable.  The values stay
    on the device: they are accumulated there in fp64 and cross to the host in one copy behind the run's only synchronise.
    noise_seed (an int below 2^64): validation_step(noise_keys=NoiseKeys(noise_seed, ids)) — `ids` are the RUNNING sample
    indices over the batches, as in run_test — so sample i meets the same (t, noise, posterior noise) whatever
    batch_size, max_batches or checkpoint, and two checkpoints differ by a paired difference; `seed` is not used.  The
    per-sample values {t, simple, plain} of both passes are gathered in a device fp64 table in batch-index order, cross
    to the host in one copy behind the run's one synchronise, and the epoch means are formed FROM that table in
    sample-index order (validation_means), so they do not depend on which lane finished first: lanes = 1, 2 and 4 give
    the same bits under the same tuning table (_lib.shared_chip).
    lanes > 1: the batches are spread over execution lanes as in run_test (noise_seed required: ValueError); the live and
    the EMA pass of a batch select their weight set for the lane's thread alone, so lanes sit on different sets.
    rank, world: this call evaluates the batches j with j % world == rank (noise_seed required); a dataset of
    upgpt_amd.data is asked for those batches only.  The ids stay the global running indices.  The returned means are
    the SHARD's; merge_validation(save_dir) forms the epoch's from the shards' files.
    save_dir with noise_seed: val_samples.csv (world > 1: val_samples.rank<r>of<w>.csv) with the columns id, t, simple,
    plain, t_ema, simple_ema, plain_ema; val_schedule.json (the loss weights and tables validation_means reads); and,
    with world = 1, val_metrics.json."""
    import json
    lanes, rank, world, batch_size = int(lanes), int(rank), int(world), int(batch_size)
    require(lanes >= 1, "lanes must be >= 1", ValueError)
    require(lanes == 1 or noise_seed is not None, "lanes > 1 needs noise_seed: without keyed noise validation_step draws from "
            "the process-wide device generator, and lane threads would interleave those draws in an undefined order", ValueError)
    require(world >= 1 and 0 <= rank < world, "rank must be in [0, world), got rank %d of %d" % (rank, world), ValueError)
    require(world == 1 or noise_seed is not None, "world > 1 needs noise_seed: without keyed noise a sample's draws depend on "
            "the batches evaluated before it", ValueError)
    dev = model.model.diffusion_model._device()
    if noise_seed is not None:
        return _run_validation_keyed(model, dataset, batch_size, max_batches, save_dir, lanes, int(noise_seed), rank, world, dev)
    batches = dataset.batches(batch_size) if hasattr(dataset, "batches") else dataset
    keys, acc, count = None, None, 0
    with torch.cuda.device(dev), torch.random.fork_rng(devices=[dev.index]):
        torch.manual_seed(int(seed))
        for i, batch in enumerate(batches):
            if max_batches is not None and i >= int(max_batches):
                break
            n = int(batch[model.first_stage_key].shape[0])
            d = model.validation_step(batch, i)
            if keys is None:
                keys = list(d)
                acc = torch.zeros(len(keys), dtype=torch.float64, device=dev)
            require(list(d) == keys, "validation_step returned other keys than for the first batch", RuntimeError)
            acc += torch.stack([d[k].reshape(()) for k in keys]).double() * n
            count += n
        require(count > 0, "run_validation: no batches", ValueError)
        host = torch.empty(len(keys), dtype=torch.float64, pin_memory=True)
        host.copy_(acc / count, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    means = {k: float(v) for k, v in zip(keys, host.tolist())}
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(str(save_dir), "val_metrics.json"), "w") as f:
            json.dump(means, f, indent=1)
    return means


def _run_validation_keyed(model, dataset, batch_size, max_batches, save_dir, lanes, noise_seed, rank, world, dev):
    import json

    from .rng import NoiseKeys
    per_sample = type(model).PER_SAMPLE
    done = {}  # global batch index -> (id of its first sample, device fp64 [n, 6])

    def work():
        for j, first, batch in _shard_work(dataset, batch_size, rank, world, max_batches):
            n = int(batch[model.first_stage_key].shape[0])
            keys = NoiseKeys(noise_seed, range(first, first + n), device=dev)
            keys.keys  # (uploaded here, with the batch: under host_io() when lanes take their batches)
            yield j, first, batch, keys

    def step(item):
        j, first, batch, keys = item
        done[j] = (first, model.validation_step(batch, j, noise_keys=keys)[per_sample])

    with torch.cuda.device(dev):
        model._logvar_table(dev)  # (a host logvar is uploaded here, once, not from a lane thread beside a capture)
        if lanes == 1:
            for item in work():
                step(item)
        else:
            _run_lanes(model, work(), lanes, step, ema=False)
        require(done, "run_validation: no batches", ValueError)
        order = sorted(done)
        # batch-index order, whichever lane made which batch; the two tables of the loss ride along in the one copy
        n_t = int(model.num_timesteps)
        blob = torch.cat([done[j][1].reshape(-1) for j in order] + [model.lvlb_weights.to(dev).double(),
                                                                    model._logvar_table(dev).double()])
        host = torch.empty(blob.numel(), dtype=torch.float64, pin_memory=True)
        host.copy_(blob, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    arr = host.numpy().copy()
    table, lvlb, logvar = arr[:-2 * n_t].reshape(-1, 6), arr[-2 * n_t:-n_t], arr[-n_t:]
    ids = [i for j in order for i in range(done[j][0], done[j][0] + int(done[j][1].shape[0]))]
    sched = _val_schedule(model, lvlb, logvar)
    means = validation_means(table, sched)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        name = "val_samples.csv" if world == 1 else "val_samples.rank%dof%d.csv" % (rank, world)
        _write_val_samples(os.path.join(str(save_dir), name), ids, table)
        with open(os.path.join(str(save_dir), "val_schedule.json"), "w") as f:
            json.dump(sched, f)
        if world == 1:
            with open(os.path.join(str(save_dir), "val_metrics.json"), "w") as f:
                json.dump(means, f, indent=1)
    return means


def run_upscale(model, batches, lr_dir, save_dir, pad=(8, 0), lanes=1, noise_seed=None, rank=0, world=1, **log_kwargs):
    """The second stage of an evaluation run, the flow of the reference's DeepFashionSuperResSampling dataset
    (deepfashion_inshop.py:419-479) through the upscale model: for every batch dict (`fname`, `styles`, `txt`, `image`)
    the low-resolution pictures lr_dir/<fname>.jpg are decoded by PIL, uploaded as bytes and turned into batch['lr']
    [B, 3, h, w] and batch['lr_image'] [B, h, w, 3] ON THE DEVICE by one upk_resize_bilinear_u8 launch
    (prepare.lr_transform with the dataset's pad of 8 columns, [h, w] = model.image_size); then
    model.log_images(batch, N=<batch size>, **LOG_DEFAULTS, use_ema=model.use_ema, **log_kwargs), and log['samples']
    finished by upk_image_finish_u8 (FINISH_SAMPLE, centre-cropped to model.crop_size).  The samples and the resized
    conditioning bytes share one device buffer that crosses to the host in one copy behind one synchronise, as in
    finished_arrays.  Written: save_dir/results/upscaled/<fname>.jpg and, the conditioning actually used,
    save_dir/results/lr/<fname>.jpg.  Returns the results directory.  The caller's batch dicts are left as they came.
    noise_seed / lanes / rank, world: as run_test and run_validation.  With noise_seed every batch samples with
    log_images(noise_keys=NoiseKeys(noise_seed, ids)), `ids` the running sample indices over `batches`; lanes > 1 (needs
    noise_seed: ValueError) spreads the batches over execution lanes — PIL's decoding of the lr pictures and their upload
    happen under the take lock (one taker at a time, on the taking lane's stream), the chain, the finishing, the one
    device -> host copy and the JPEG encoding in the lane thread — and writes the files of the lanes = 1 run with the same
    seed byte for byte under the same tuning table (_lib.shared_chip); rank, world (needs noise_seed) processes the
    batches j with j % world == rank, the ids staying the global ones.

    This is THIS PACKAGE'S extension: the reference's own test_step cannot run on that dataset's batches, because it
    reads `smpl_image` and `src_image`, which the dataset does not provide.  N is the batch size here, unlike
    test_step's len(batch).  A missing or unreadable (or differently sized) lr file raises ValueError naming the file;
    it is not silently replaced by the next sample, as the reference's loader would do."""
    from PIL import Image

    from . import prepare
    lanes, rank, world = int(lanes), int(rank), int(world)
    require(lanes >= 1, "lanes must be >= 1", ValueError)
    require(lanes == 1 or noise_seed is not None, "lanes > 1 needs noise_seed: without keyed noise log_images draws from the "
            "process-wide device generator, and lane threads would interleave those draws in an undefined order", ValueError)
    require(world >= 1 and 0 <= rank < world, "rank must be in [0, world), got rank %d of %d" % (rank, world), ValueError)
    require(world == 1 or noise_seed is not None, "world > 1 needs noise_seed: without keyed noise a sample's draws depend on "
            "the batches evaluated before it", ValueError)
    lr_dir = Path(lr_dir)
    roots = {k: Path(save_dir) / "results" / k for k in ("upscaled", "lr")}
    for r in roots.values():
        os.makedirs(str(r), exist_ok=True)
    dev = model.device
    oh, ow = (int(v) for v in model.image_size)
    f = 2 ** int(model.num_downs)
    win = center_crop_window(f * oh, f * ow, model.crop_size)
    ch, cw = win[2], win[3]

    def work():  # (what a lane does under the take lock: decoding, the upload, the keys)
        from .rng import NoiseKeys
        for j, first, batch in _shard_work(batches, None, rank, world, None):
            names = list(batch["fname"])
            pics = []
            for fname in names:
                path = lr_dir / f"{fname}.jpg"
                arr = _decode(path) if path.is_file() else None
                require(arr is not None, "run_upscale: cannot read the low-resolution picture %s" % path, ValueError)
                require(not pics or arr.shape == pics[0].shape, "run_upscale: %s is %s, the first picture of its batch %s" % (
                    path, arr.shape, pics[0].shape if pics else None), ValueError)
                pics.append(arr)
            src = torch.from_numpy(np.stack(pics)).to(dev, non_blocking=True)
            if lanes > 1:  # (the conditioning crosses here, under the lock, not from the lane thread beside a capture)
                batch = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in batch.items()}
            keys = None
            if noise_seed is not None:
                keys = NoiseKeys(noise_seed, range(first, first + len(names)), device=dev)
                keys.keys
            yield batch, names, src, keys

    def step(item):
        batch, names, src, keys = item
        n = len(names)
        off_lr = (n * ch * cw * 3 + 15) // 16 * 16
        total = off_lr + n * oh * ow * 3
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        up_view = buf[:n * ch * cw * 3].view(n, ch, cw, 3)
        lr_view = buf[off_lr:].view(n, oh, ow, 3)
        kw = dict(LOG_DEFAULTS, N=n, use_ema=model.use_ema)
        kw.update(log_kwargs)
        if keys is not None:
            kw["noise_keys"] = keys
        with torch.no_grad():
            lr, lr_image = prepare.lr_transform(src, [oh, ow], pad, out_u8=lr_view)
            log = model.log_images(dict(batch, lr=lr, lr_image=lr_image), **kw)
            samples = log["samples"]
            require(tuple(samples.shape[1:]) == (3, f * oh, f * ow), "run_upscale: samples %s, expected [n, 3, %d, %d]" % (
                tuple(samples.shape), f * oh, f * ow), ValueError)
            m = min(int(samples.shape[0]), n)
            finish_images(samples[:m].to(dev, torch.float32), up_view[:m], _lib.LAYOUT_NCHW, _lib.FINISH_SAMPLE, window=win)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=buf.is_cuda)
        host.copy_(buf, non_blocking=True)
        if buf.is_cuda:
            torch.cuda.current_stream(dev).synchronize()
        arr = host.numpy()
        up_arr = arr[:n * ch * cw * 3].reshape(n, ch, cw, 3)
        lr_arr = arr[off_lr:].reshape(n, oh, ow, 3)
        for i, fname in enumerate(names):
            if i < m:
                Image.fromarray(up_arr[i]).save(roots["upscaled"] / f"{fname}.jpg")
            Image.fromarray(lr_arr[i]).save(roots["lr"] / f"{fname}.jpg")

    if lanes == 1:
        for item in work():
            step(item)
    else:
        _run_lanes(model, work(), lanes, step)
    return Path(save_dir) / "results"


def run_interpolation(im, batch, dst_pose, alphas, save_dir, steps=200, sampler="ddim", noise_seed=0, upscale=None, txt=None):
    """The demo's "Interpolate" flow (app.py:280-308) as one call: im.interpolate(batch, dst_pose, alphas, steps=steps,
    sampler=sampler, noise_seed=noise_seed) — `im` an InferenceModel, `batch` its un-batched sample with the source pose,
    `dst_pose` prepare.load_pose's dict; with the default seed every frame meets the same keyed noise, noise_seed=None
    draws from the torch generator as the reference does — and then
      <save_dir>/interp/interp_{i}.jpg   every frame exactly as the app writes it: Image.fromarray(np.uint8(sample * 255))
      <save_dir>/interp_strip.jpg        the frames side by side, left to right in the order of `alphas`
    upscale (an InferenceModel holding the upscale checkpoint): the frames' bytes (those in memory, not the decoded JPEG
    files) go through upscale.upscale(frames, batch['styles'], txt, steps=steps, sampler=sampler) in chunks of 8, its cap
    per call, and are written as <save_dir>/interp_upscaled/interp_{i}.png; txt defaults to batch['txt'].
    Returns the list of the frames' paths (the .jpg files), in frame order."""
    from PIL import Image
    save_dir = Path(save_dir)
    out = im.interpolate(batch, dst_pose, alphas, steps=steps, sampler=sampler, noise_seed=noise_seed)
    frames = [np.uint8(sample * 255) for sample in out["samples"]]
    os.makedirs(str(save_dir / "interp"), exist_ok=True)
    paths = []
    for i, frame in enumerate(frames):
        paths.append(save_dir / "interp" / f"interp_{i}.jpg")
        Image.fromarray(frame).save(paths[-1])
    Image.fromarray(np.concatenate(frames, axis=1)).save(save_dir / "interp_strip.jpg")
    if upscale is not None:
        os.makedirs(str(save_dir / "interp_upscaled"), exist_ok=True)
        text = batch["txt"] if txt is None else txt
        cap = 8
        for lo in range(0, len(frames), cap):
            big = upscale.upscale(np.stack(frames[lo:lo + cap]), batch["styles"], text, steps=steps, sampler=sampler)["samples"]
            require(len(big) == len(frames[lo:lo + cap]), "run_interpolation: upscale returned %d pictures for %d frames" % (
                len(big), len(frames[lo:lo + cap])), ValueError)
            for j, sample in enumerate(big):
                Image.fromarray(np.uint8(sample * 255)).save(save_dir / "interp_upscaled" / f"interp_{lo + j}.png")
    return paths


def run_styles(image_root, segm_root, dst_root, segmenter='mm', batch_size=16):
    """The flow the reference's scripts/segment.py intends: for every label map segm_root/**/<id>_segm.png and its picture
    image_root/**/<id>.jpg the style crops are made ON THE DEVICE (styles.style_crops: two launches per batch, pictures
    of equal size batched up to `batch_size`) and every VALID group's crop is written from the device bytes to
    dst_root/**/<id with its first '_' turned into '/'>/<group>.jpg with Pillow's default save, the files the
    reference's datasets read back as batch['styles'].  An invalid crop (an empty cut, a face of more than 128 rows, a
    background without a pixel) writes no file, which the datasets read as the empty style.  Returns the number of
    label maps processed.  An unreadable picture or label map, or a pair of different sizes, raises ValueError naming
    the file."""
    from PIL import Image

    from . import styles
    seg = styles.get_segmenter(segmenter)
    segm_root, image_root, dst_root = Path(segm_root), Path(image_root), Path(dst_root)
    by_size = {}
    for segm_file in sorted(segm_root.rglob("*_segm.png")):
        rel = segm_file.relative_to(segm_root)
        stem = rel.name[:-len("_segm.png")]
        image_file = image_root / rel.parent / (stem + ".jpg")
        try:
            with Image.open(str(segm_file)) as im:
                segm = np.asarray(im, dtype=np.uint8)
        except Exception:
            segm = None
        require(segm is not None and segm.ndim == 2, "run_styles: cannot read the label map %s" % segm_file, ValueError)
        pic = _decode(image_file) if image_file.is_file() else None
        require(pic is not None, "run_styles: cannot read the picture %s" % image_file, ValueError)
        require(pic.shape[:2] == segm.shape, "run_styles: %s is %s, its label map %s" % (image_file, pic.shape[:2], segm.shape),
                ValueError)
        by_size.setdefault(segm.shape, []).append((dst_root / rel.parent / stem.replace('_', '/', 1), pic, segm))
    done = 0
    for items in by_size.values():
        for i in range(0, len(items), int(batch_size)):
            part = items[i:i + int(batch_size)]
            _, valid, u8 = styles.style_crops(np.stack([p for _, p, _ in part]), np.stack([s for _, _, s in part]), seg,
                                              seg.names, out_u8=True)
            valid, u8 = valid.cpu().numpy(), u8.cpu().numpy()
            for j, (dst_dir, _, _) in enumerate(part):
                os.makedirs(str(dst_dir), exist_ok=True)
                for g, name in enumerate(seg.names):
                    if valid[j, g]:
                        Image.fromarray(u8[j, g]).save(dst_dir / (name + ".jpg"))
            done += len(part)
    return done


def _decode(path):
    """uint8 [H, W, 3] of an image file, or None when it cannot be read."""
    from PIL import Image
    try:
        with Image.open(str(path)) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)
    except Exception:
        return None


def _lpips_net(lpips, device):
    """run_metrics' `lpips` argument -> an LPIPS on `device`, or None: an instance, a (vgg16_path, lin_path) pair, or the
    environment variables UPGPT_LPIPS_VGG / UPGPT_LPIPS_LIN (both, or neither)."""
    from .lpips import LPIPS
    if lpips is None:
        vgg, lin = os.environ.get("UPGPT_LPIPS_VGG"), os.environ.get("UPGPT_LPIPS_LIN")
        if not vgg and not lin:
            return None
        require(vgg and lin, "UPGPT_LPIPS_VGG and UPGPT_LPIPS_LIN must both be set (torchvision's vgg16 state dict and "
                "lpips' weights/v0.1/vgg.pth)", ValueError)
        lpips = (vgg, lin)
    if isinstance(lpips, LPIPS):
        return lpips
    require(isinstance(lpips, (tuple, list)) and len(lpips) == 2, "lpips must be an LPIPS instance or a (vgg16_path, "
            "lin_path) pair", TypeError)
    return LPIPS.from_files(lpips[0], lpips[1]).to(device)


FID_SUFFIXES = frozenset("." + e for e in ("bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"))  # pytorch_fid's


def _fid_net(fid, device):
    """run_metrics' `fid` argument -> a FIDInception on `device`, or None: an instance, a path to pytorch_fid's
    pt_inception-2015-12-05-6726825d.pth, or the environment variable UPGPT_FID_INCEPTION."""
    from .fid import FIDInception
    if fid is None:
        fid = os.environ.get("UPGPT_FID_INCEPTION") or None
        if fid is None:
            return None
    if isinstance(fid, FIDInception):
        return fid
    require(isinstance(fid, (str, os.PathLike)), "fid must be a FIDInception instance or the path of the weight file", TypeError)
    return FIDInception.from_file(fid).to(device)


def _fid_of_dirs(net, dirs, batch_size, device):
    """pytorch_fid's number for two folders: EVERY decodable picture of each (its suffix list, converted to RGB), one size at
    a time in (height, width, name) order, batches of batch_size through metrics.fid_features (one device -> host copy of
    2048 floats per picture each), statistics accumulated in fp64 (metrics.FidStats: the order of the pictures, which does
    not depend on batch_size, fixes every bit)."""
    from PIL import Image

    from . import metrics
    stats = []
    for d in dirs:
        by_size = {}
        for f in sorted(p for p in d.iterdir() if p.suffix.lower() in FID_SUFFIXES and p.is_file()):
            try:
                with Image.open(str(f)) as im:  # (the header: decoding happens batch by batch below)
                    by_size.setdefault((im.height, im.width), []).append(f)
            except Exception:
                continue
        acc = metrics.FidStats()
        for size in sorted(by_size):
            batch = []
            for i, f in enumerate(by_size[size]):
                im = _decode(f)
                if im is not None and im.shape[:2] == size:
                    batch.append(im)
                if batch and (len(batch) >= batch_size or i + 1 == len(by_size[size])):
                    x = torch.from_numpy(np.stack(batch)).to(device, non_blocking=True)
                    with torch.no_grad():
                        acc.add(metrics.fid_features(x, net).cpu())
                    batch = []
        stats.append(acc.stats())
    return metrics.fid_from_stats(*stats[0], *stats[1])


def run_metrics(results_dir=None, gt_dir=None, sample_dir=None, batch_size=100, device=None, lpips=None, fid=None):
    """scripts/eval_metrics.py's SSIM and MS-SSIM columns (its lines 110-111) for a results tree, its LPIPS column
    (line 112) and its FID line (line 102) when the weights are given: LPIPS needs the user's two weight files, FID
    pytorch_fid's Inception file.  Without that file FID is not computed.

    fid: an upgpt_amd.fid.FIDInception instance or the path of pt_inception-2015-12-05-6726825d.pth; None reads the path
    from UPGPT_FID_INCEPTION.  With weights metrics.txt gets, as its FIRST line (where the reference writes pytorch_fid's
    output), `FID:  <value>` with the two blanks of pytorch_fid's print, and the result the key "FID".  As for pytorch_fid
    the two sets are EVERY decodable picture of gt_dir and of sample_dir (suffixes bmp, jpg, jpeg, pgm, png, ppm, tif, tiff,
    webp; converted to RGB), independent of the pairing and of "skipped"; they are grouped by size, taken in (height,
    width, name) order and batched by batch_size, every batch one more device -> host copy (2048 floats per picture); a
    set of fewer than two pictures gives NaN.  metrics.csv is not touched by FID, and without weights every output is what it was before FID existed.

    lpips: an upgpt_amd.lpips.LPIPS instance or a (vgg16_path, lin_path) pair (torchvision's vgg16 state dict and lpips'
    weights/v0.1/vgg.pth); None reads the pair from UPGPT_LPIPS_VGG / UPGPT_LPIPS_LIN.  With weights metrics.csv has the
    columns name, SSIM, LPIPS, MSSIM (the reference's order), metrics.txt a third line LPIPS: <mean>, the result the key
    "LPIPS", and every batch one more device -> host copy (5 floats per picture); LPIPS is NaN for a picture with a side
    below 16 and its mean ignores those.  Without weights every output is what it was before LPIPS existed.

    gt_dir / sample_dir default to results_dir/gt and results_dir/samples.  Every *.jpg / *.png of sample_dir is paired
    with the file of the same name in gt_dir, decoded by PIL, grouped by picture size and sent to the device in batches of
    batch_size; each batch is one metrics.ssim_levels call and ONE device -> host copy (6 * levels floats per picture).
    Writes metrics.csv (columns name, SSIM, MSSIM; rows in name order) and metrics.txt (SSIM: <mean>, MSSIM: <mean>)
    into the parent of sample_dir, where the reference puts them, and returns {"SSIM": mean, "MSSIM": mean, "n": rows,
    "skipped": [names]}.

    MSSIM is NaN for a picture whose smaller side is <= 160 (ms_ssim is undefined there), and its mean ignores those.
    One behaviour of the reference is deliberately NOT reproduced: its loader substitutes the NEXT sample for a pair it
    cannot read, so that pair's neighbour is counted twice.  Here a sample without a readable ground truth of the same
    size (or smaller than the 11-tap window) goes into "skipped" and is left out of both files and both means."""
    import csv

    from . import metrics
    require(results_dir is not None or (gt_dir and sample_dir), "run_metrics needs results_dir, or gt_dir and sample_dir", ValueError)
    gt_dir = Path(gt_dir) if gt_dir else Path(results_dir) / "gt"
    sample_dir = Path(sample_dir) if sample_dir else Path(results_dir) / "samples"
    require(gt_dir.is_dir() and sample_dir.is_dir(), "run_metrics: %s and %s must be directories" % (gt_dir, sample_dir), ValueError)
    batch_size = int(batch_size)
    require(batch_size >= 1, "batch_size must be positive", ValueError)
    if device is None:  # (without a GPU metrics.ssim_levels refuses the host tensors: there is no CPU fallback)
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    nl = len(metrics.MS_WEIGHTS)
    net = _lpips_net(lpips, device)
    fid_net = _fid_net(fid, device)
    rows, skipped, pending = {}, [], {}

    def flush(size):
        names, gts, smps = pending.pop(size)
        deep = min(size) > metrics.MS_MIN_SIDE
        a = torch.from_numpy(np.stack(smps)).to(device, non_blocking=True)
        b = torch.from_numpy(np.stack(gts)).to(device, non_blocking=True)
        with torch.no_grad():
            lv = metrics.ssim_levels(a, b, nl if deep else 1).cpu()  # the one device -> host copy of the batch
        s = metrics.ssim_from_levels(lv).tolist()
        m = metrics.ms_ssim_from_levels(lv).tolist() if deep else [float("nan")] * len(names)
        lp = [float("nan")] * len(names)
        if net is not None and min(size) >= metrics.LPIPS_MIN_SIDE:
            with torch.no_grad():
                lp = metrics.lpips_from_layers(metrics.lpips_layers(a, b, net).cpu()).tolist()  # (the batch's second copy)
        rows.update({n: (si, mi, li) for n, si, mi, li in zip(names, s, m, lp)})

    for name in sorted(f.name for f in sample_dir.iterdir() if f.suffix in (".jpg", ".png") and f.is_file()):
        smp = _decode(sample_dir / name)
        gt = _decode(gt_dir / name) if (gt_dir / name).is_file() else None
        if smp is None or gt is None or smp.shape != gt.shape or min(smp.shape[:2]) < metrics.WINDOW:
            skipped.append(name)
            continue
        group = pending.setdefault(smp.shape[:2], ([], [], []))
        for lst, v in zip(group, (name, gt, smp)):
            lst.append(v)
        if len(group[0]) >= batch_size:
            flush(smp.shape[:2])
    for size in list(pending):
        flush(size)

    names = sorted(rows)
    ssim_vals = np.array([rows[n][0] for n in names], dtype=np.float64)
    ms_vals = np.array([rows[n][1] for n in names], dtype=np.float64)
    ms_ok = ms_vals[~np.isnan(ms_vals)]
    means = {"SSIM": float(ssim_vals.mean()) if len(names) else float("nan"),
             "MSSIM": float(ms_ok.mean()) if ms_ok.size else float("nan")}
    if net is not None:
        lp_vals = np.array([rows[n][2] for n in names], dtype=np.float64)
        lp_ok = lp_vals[~np.isnan(lp_vals)]
        means["LPIPS"] = float(lp_ok.mean()) if lp_ok.size else float("nan")
    if fid_net is not None:
        means["FID"] = _fid_of_dirs(fid_net, (gt_dir, sample_dir), batch_size, device)
    log_dir = sample_dir.resolve().parent
    with open(str(log_dir / "metrics.csv"), "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["name", "SSIM"] + (["LPIPS"] if net is not None else []) + ["MSSIM"])
        for n in names:
            wr.writerow([n, repr(rows[n][0])] + ([repr(rows[n][2])] if net is not None else []) + [repr(rows[n][1])])
    with open(str(log_dir / "metrics.txt"), "w") as f:
        if fid_net is not None:
            f.write("FID:  %r\n" % means["FID"])  # (pytorch_fid's print('FID: ', value))
        for k in ("SSIM", "MSSIM") + (("LPIPS",) if net is not None else ()):
            f.write("%s: %r\n" % (k, means[k]))
    return dict(means, n=len(names), skipped=skipped)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m upgpt_amd.evaluate", description="SSIM / MS-SSIM (with the two weight "
                                 "files LPIPS, with pytorch_fid's Inception weights FID) of a results tree (gt against samples) -> metrics.csv, metrics.txt next to "
                                 "the samples folder")
    ap.add_argument("--dir", default=None, help="results directory holding gt/ and samples/")
    ap.add_argument("--gt_dir", default=None, help="ground-truth pictures (default: DIR/gt)")
    ap.add_argument("--sample_dir", default=None, help="generated pictures (default: DIR/samples)")
    ap.add_argument("--gpu", type=int, default=0, help="device ordinal")
    ap.add_argument("--batch_size", type=int, default=100, help="pictures per kernel call")
    ap.add_argument("--lpips_vgg", default=None, help="torchvision's vgg16 state dict (default: $UPGPT_LPIPS_VGG); with "
                    "--lpips_lin it adds the LPIPS column")
    ap.add_argument("--lpips_lin", default=None, help="lpips' weights/v0.1/vgg.pth (default: $UPGPT_LPIPS_LIN)")
    ap.add_argument("--fid_inception", default=None, help="pytorch_fid's pt_inception-2015-12-05-6726825d.pth (default: "
                    "$UPGPT_FID_INCEPTION); adds the FID line of metrics.txt")
    a = ap.parse_args(argv)
    if a.dir is None and not (a.gt_dir and a.sample_dir):
        ap.error("give --dir, or both --gt_dir and --sample_dir")
    if bool(a.lpips_vgg) != bool(a.lpips_lin):
        ap.error("give both --lpips_vgg and --lpips_lin, or neither")
    res = run_metrics(a.dir, a.gt_dir, a.sample_dir, a.batch_size, a.gpu if torch.cuda.is_available() else None,
                      lpips=(a.lpips_vgg, a.lpips_lin) if a.lpips_vgg else None, fid=a.fid_inception)
    if "FID" in res:
        print("FID:  %r" % res["FID"])
    for k in ("SSIM", "MSSIM") + (("LPIPS",) if "LPIPS" in res else ()):
        print("%s: %r" % (k, res[k]))
    print("%d pictures, %d skipped" % (res["n"], len(res["skipped"])))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
