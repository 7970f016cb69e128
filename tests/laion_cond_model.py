"""The model block of the reference's configs/deepfashion/inshop_laion_clip.yaml restated as a plain dict (values only;
the first stage's ckpt_path is left out: the weights come from the recipe), and helpers shared by the host and GPU tests
of the CLIPTextImageCrossAtten conditioning stage."""
import copy
import os

import numpy as np
import torch

from upgpt_amd import synth

G = os.path.join(os.path.dirname(__file__), "golden")
STAGE = "ldm.modules.encoders.modules.CLIPTextImageCrossAtten"

MODEL = {
    "base_learning_rate": 2.5e-05,
    "target": "ldm.models.diffusion.ddpm.LatentDiffusion",
    "params": {
        "linear_start": 0.00085, "linear_end": 0.0120, "num_timesteps_cond": 1, "log_every_t": 200, "timesteps": 1000,
        "first_stage_key": "image", "cond_stage_key": "txt", "cond_stage_key_2": "styles", "concat_key": "person_mask",
        "image_size": [32, 24], "channels": 4, "cond_stage_trainable": True, "conditioning_key": "hybrid",
        "scale_factor": 0.18215,
        "scheduler_config": {"target": "ldm.lr_scheduler.LambdaLinearScheduler",
                             "params": {"warm_up_steps": [1], "cycle_lengths": [10000000000000], "f_start": [1.e-6],
                                        "f_max": [1.], "f_min": [1.]}},
        "unet_config": {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                        "params": {"image_size": 32, "in_channels": 5, "out_channels": 4, "model_channels": 224,
                                   "attention_resolutions": [4, 2, 1], "num_res_blocks": 2, "channel_mult": [1, 2, 4, 4],
                                   "num_heads": 8, "use_spatial_transformer": True, "transformer_depth": 1,
                                   "context_dim": 768, "use_checkpoint": True, "legacy": False}},
        "first_stage_config": {"target": "ldm.models.autoencoder.AutoencoderKL",
                               "params": {"embed_dim": 4, "monitor": "val/rec_loss",
                                          "ddconfig": {"double_z": True, "z_channels": 4, "resolution": 256, "in_channels": 3,
                                                       "out_ch": 3, "ch": 128, "ch_mult": [1, 2, 4, 4], "num_res_blocks": 2,
                                                       "attn_resolutions": [], "dropout": 0.0},
                                          "lossconfig": {"target": "torch.nn.Identity"}}},
        "cond_stage_config": {"target": STAGE},
        "extra_cond_stages": {"pose_cond": {"target": "ldm.modules.poses.poses.LinearProject", "cond_stage_key": "smpl",
                                            "params": {"input_dim": 85, "output_dim": 768}}},
    },
}


def build_model():
    from upgpt_amd.config import instantiate_from_config
    return instantiate_from_config(copy.deepcopy(MODEL)).eval()


def golden():
    return np.load(os.path.join(G, "laion_cond.npz"))


def golden_keys():
    with open(os.path.join(G, "laion_cond_keys.txt")) as f:
        return f.read().split()


def stage_state(stage):
    """Recipe weights under the checkpoint's names (cond_stage_model.*), as the golden's generator drew them."""
    return {k: synth.synth_tensor("cond_stage_model." + k, tuple(v.shape)) for k, v in stage.state_dict().items()}


def golden_inputs(g):
    """(ids int64 [2, 77], styles fp32 [2, 9, 3, 224, 224]) of the golden; the crops are redrawn from the seed."""
    import zlib
    gen = torch.Generator(device="cpu").manual_seed(2424)
    torch.randint(0, 49408, (2, 77), generator=gen)  # (the generator's first draw: the ids, stored in the file)
    styles = torch.randn(2, 9, 3, 224, 224, generator=gen)
    assert (zlib.crc32(styles.numpy().tobytes()) & 0xFFFFFFFF) == int(g["styles_crc"]), "torch.randn stream changed"
    return torch.as_tensor(g["ids"]).long(), styles


def rel_rms(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
