"""Host side of the CLIPTextImageCrossAtten conditioning stage: construction from the config node, the
reference's state-dict names, the no-fallback errors, and the fp64 restatement (tests/laion_cond_ref.py) against the golden
made by transformers' CLIPModel + the reference's CrossAttention (tests/golden/make_laion_cond_golden.py)."""
import pytest
import torch

import laion_cond_model as M
import laion_cond_ref as R
from upgpt_amd.config import instantiate_from_config


@pytest.fixture(scope="module")
def stage():
    return instantiate_from_config({"target": M.STAGE})


def test_stage_from_config_has_the_reference_keys(stage):
    from ldm.modules.encoders.modules import CLIPTextImageCrossAtten
    assert type(stage) is CLIPTextImageCrossAtten
    keys = M.golden_keys()
    assert set(stage.state_dict()) == set(keys) and len(keys) == int(M.golden()["n_keys"])
    for k in ("model.text_model.encoder.layers.11.mlp.fc2.weight", "model.vision_model.pre_layrnorm.weight",
              "model.vision_model.encoder.layers.23.self_attn.q_proj.bias", "model.visual_projection.weight",
              "model.text_projection.weight", "model.logit_scale", "cross_att.to_out.0.bias"):
        assert k in keys
    sd = stage.state_dict()
    assert tuple(sd["cross_att.to_k.weight"].shape) == (768, 768)
    assert tuple(sd["model.visual_projection.weight"].shape) == (768, 1024)
    # the CLIP model is frozen, the cross-attention is what the reference trains
    assert sorted(n for n, p in stage.named_parameters() if p.requires_grad) == sorted(
        "cross_att." + n for n in ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias"))
    assert stage.model.text_tower.config["hidden_act"] == stage.model.vision_tower.config["hidden_act"] == "gelu"


def test_stage_has_no_encode(stage):
    # (get_learned_conditioning must fall through to stage(**c), as with the reference's class)
    assert not hasattr(stage, "encode")
    for name in ("forward_image", "get_text_emb", "freeze"):
        assert callable(getattr(stage, name))


def test_checkpoint_entries_load_through_init_from_ckpt(tmp_path):
    from upgpt_amd.ddpm import _load_weights
    small = dict(text=dict(num_hidden_layers=1), vision=dict(layers=1, width=64, heads=2))
    a = instantiate_from_config({"target": M.STAGE, "params": small})
    sd = {"cond_stage_model." + k: v for k, v in M.stage_state(a).items()}
    # buffers of older transformers versions: not held, reported as unexpected, never an error
    sd["cond_stage_model.model.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    path = str(tmp_path / "ckpt.pt")
    torch.save({"state_dict": sd}, path)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cond_stage_model = instantiate_from_config({"target": M.STAGE, "params": small})

    h = Holder()
    res = _load_weights(h, path)
    assert not res.missing_keys and res.unexpected_keys == ["cond_stage_model.model.text_model.embeddings.position_ids"]
    for k, v in h.cond_stage_model.state_dict().items():
        assert torch.equal(v, sd["cond_stage_model." + k]), k


def test_load_clip_weights_into_the_stage(tmp_path):
    from upgpt_amd.inference import load_clip_weights
    small = dict(text=dict(num_hidden_layers=1), vision=dict(layers=1, width=64, heads=2))
    st = instantiate_from_config({"target": M.STAGE, "params": small})
    sd = {k[len("model."):]: v for k, v in M.stage_state(st).items() if k.startswith("model.")}
    sd["logit_scale"] = sd["logit_scale"].reshape(())
    torch.save(sd, str(tmp_path / "clip.pt"))
    load_clip_weights(str(tmp_path / "clip.pt"), cond_stage=st)
    assert all(torch.equal(v, sd[k]) for k, v in st.model.state_dict().items())
    assert float(st.cross_att.to_q.weight.detach().abs().max()) == 0.0


def test_latent_diffusion_from_the_laion_config():
    model = M.build_model()
    assert model.cond_stage_key == "txt" and model.cond_stage_key_2 == "styles"
    assert model.cond_stage_trainable and model.concat_key == "person_mask"
    assert type(model.cond_stage_model).__name__ == "CLIPTextImageCrossAtten"
    assert not model.cond_stage_model.training
    assert any(p.requires_grad for p in model.cond_stage_model.cross_att.parameters())
    assert len(model.extra_cond_models) == 1 and model.extra_cond_keys == ["smpl"]
    assert "cond_stage_model.cross_att.to_out.0.bias" in model.state_dict()


def test_no_cpu_fallback_and_no_text_styles(stage):
    ids, styles = torch.zeros(1, 77, dtype=torch.long), torch.zeros(1, 9, 3, 224, 224)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage(ids, styles)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage.forward_image(styles)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage.get_text_emb(ids)
    with pytest.raises(RuntimeError, match="tokenizer"):
        stage(["a woman in a red dress"], styles)  # the hub tokenizer's files are not on disk
    with pytest.raises(NotImplementedError, match="style_encode='text'"):
        instantiate_from_config({"target": M.STAGE, "params": {"style_encode": "text"}})
    from upgpt_amd.clip_text import hidden_act
    with pytest.raises(NotImplementedError, match="hidden_act"):
        hidden_act({"hidden_act": "relu"})  # (what a tower's plan asks when it is built)


def test_fp64_restatement_reproduces_the_golden(stage):
    """Pins the yardstick of the GPU tests: the plain-torch fp64 statement against the fp32 run of transformers' CLIPModel
    + the reference's CrossAttention.  Sample 1 only (the longer caption; its 9 crops are half of the tower work).
    Bound 2^-18 relative rms = 64 fp32 epsilons: the golden is an fp32 chain of 24 layers x ~5 rounded stages whose
    errors add like a random walk (~11 eps), times the dot products' own sqrt(K) eps / sqrt(K) ~ eps per stage; measured
    4.6e-7 .. 7.9e-7."""
    g = M.golden()
    ids, styles = M.golden_inputs(g)
    sd = M.stage_state(stage)
    with torch.no_grad():
        x, f, c = R.stage(sd, ids[1:], styles[1:])
    bound = 2.0 ** -18
    for name, got, ref in (("last_hidden_state", x[:, g["text_rows"].tolist()], g["last_hidden_state"][1:]),
                           ("image_features", f, g["image_features"][1:]), ("c", c[:, g["c_rows"].tolist()], g["c"][1:])):
        rel = M.rel_rms(got, torch.as_tensor(ref))
        print("fp64 restatement vs golden, %s: rel rms %.3e (bound %.3e)" % (name, rel, bound))
        assert rel <= bound, name
    # the text tower alone for the other sample too (cheap)
    with torch.no_grad():
        x0 = R.text_hidden_state(sd, ids[:1])
    assert M.rel_rms(x0[:, g["text_rows"].tolist()], torch.as_tensor(g["last_hidden_state"][:1])) <= bound
