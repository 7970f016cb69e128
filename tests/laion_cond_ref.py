"""fp64 restatement, in plain torch on the CPU, of the CLIPTextImageCrossAtten conditioning stage (the reference's
ldm/modules/encoders/modules.py:259-323): transformers' CLIP text tower (token + position embeddings, pre-LN layers with
causal self-attention and the exact erf GELU, final LayerNorm), the vision tower up to `visual_projection`
(`CLIPModel.get_image_features`), and `CrossAttention.forward` (ldm/modules/attention.py:170-193, no mask).

Every function takes the state dict under the stage's own key names (`model.text_model.*`, `model.vision_model.*`,
`model.visual_projection.weight`, `cross_att.*`); depth is read from the keys, widths from the shapes."""
import math

import torch
import torch.nn.functional as F

ACTS = {"gelu": lambda x: 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0))),
        "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x)}


def _layers(sd, prefix):
    n = 0
    while prefix + "%d.layer_norm1.weight" % n in sd:
        n += 1
    return n


def _encoder(sd, x, prefix, heads, eps, act, causal):
    get = lambda k: sd[k].to(x.dtype)
    B, S, D = x.shape
    dh = D // heads
    mask = torch.full((S, S), float("-inf"), dtype=x.dtype).triu(1) if causal else None
    for i in range(_layers(sd, prefix)):
        p = prefix + "%d." % i
        h = F.layer_norm(x, (D,), get(p + "layer_norm1.weight"), get(p + "layer_norm1.bias"), eps)
        q, k, v = (F.linear(h, get(p + "self_attn.%s_proj.weight" % n), get(p + "self_attn.%s_proj.bias" % n))
                   .view(B, S, heads, dh).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) * dh ** -0.5
        if mask is not None:
            s = s + mask
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, D)
        x = x + F.linear(a, get(p + "self_attn.out_proj.weight"), get(p + "self_attn.out_proj.bias"))
        h = F.layer_norm(x, (D,), get(p + "layer_norm2.weight"), get(p + "layer_norm2.bias"), eps)
        h = ACTS[act](F.linear(h, get(p + "mlp.fc1.weight"), get(p + "mlp.fc1.bias")))
        x = x + F.linear(h, get(p + "mlp.fc2.weight"), get(p + "mlp.fc2.bias"))
    return x


def text_hidden_state(sd, ids, heads=12, eps=1e-5, act="gelu", dtype=torch.float64, prefix="model.text_model."):
    """CLIPTextTransformer.forward(...).last_hidden_state: ids int [B, S] -> [B, S, D]."""
    get = lambda k: sd[prefix + k].to(dtype)
    x = get("embeddings.token_embedding.weight")[ids.long()] + get("embeddings.position_embedding.weight")[:ids.shape[1]]
    x = _encoder(sd, x, prefix + "encoder.layers.", heads, eps, act, causal=True)
    return F.layer_norm(x, (x.shape[-1],), get("final_layer_norm.weight"), get("final_layer_norm.bias"), eps)


def image_features(sd, images, heads=16, eps=1e-5, act="gelu", dtype=torch.float64, prefix="model."):
    """CLIPModel.get_image_features: [N, 3, H, W] -> [N, projection_dim]."""
    get = lambda k: sd[prefix + k].to(dtype)
    w = get("vision_model.embeddings.patch_embedding.weight")
    x = F.conv2d(images.to(dtype), w, stride=w.shape[-1]).flatten(2).transpose(1, 2)
    cls = get("vision_model.embeddings.class_embedding").expand(x.shape[0], 1, -1)
    x = torch.cat([cls, x], 1) + get("vision_model.embeddings.position_embedding.weight")
    D = x.shape[-1]
    x = F.layer_norm(x, (D,), get("vision_model.pre_layrnorm.weight"), get("vision_model.pre_layrnorm.bias"), eps)
    x = _encoder(sd, x, prefix + "vision_model.encoder.layers.", heads, eps, act, causal=False)
    pooled = F.layer_norm(x[:, 0], (D,), get("vision_model.post_layernorm.weight"), get("vision_model.post_layernorm.bias"), eps)
    return F.linear(pooled, get("visual_projection.weight"))


def cross_attention(sd, x, context, heads=8, prefix="cross_att."):
    """CrossAttention.forward(x, context) without a mask: [B, S, D], [B, n, Dc] -> [B, S, D]."""
    get = lambda k: sd[prefix + k].to(x.dtype)
    B, S, _ = x.shape
    q, k, v = F.linear(x, get("to_q.weight")), F.linear(context, get("to_k.weight")), F.linear(context, get("to_v.weight"))
    dh = q.shape[-1] // heads
    q, k, v = (t.view(B, t.shape[1], heads, dh).transpose(1, 2) for t in (q, k, v))
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v
    return F.linear(a.transpose(1, 2).reshape(B, S, heads * dh), get("to_out.0.weight"), get("to_out.0.bias"))


def stage(sd, ids, styles, text_heads=12, vision_heads=16, cross_heads=8, act="gelu", dtype=torch.float64):
    """CLIPTextImageCrossAtten.forward with style_encode='image' -> (last_hidden_state, image features [B, n, D], c)."""
    b, n = styles.shape[:2]
    x = text_hidden_state(sd, ids, text_heads, act=act, dtype=dtype)
    f = image_features(sd, styles.reshape(b * n, *styles.shape[2:]), vision_heads, act=act, dtype=dtype).view(b, n, -1)
    return x, f, cross_attention(sd, x, f, cross_heads)
