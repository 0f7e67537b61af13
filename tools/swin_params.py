"""Deterministic, name-keyed test weights of SwinUnet (shared by tools/gen_swin_golden.py and tests/test_*swin*.py).

The reference's init (trunc-normal 0.02 everywhere, a 0.02 bias table) makes every window's attention all but uniform: scores of order 1e-2, row maxima at
1/64, and a fixture on such weights would pin nothing of the softmax, the bias table or the shift mask.  Here the scales are chosen so that attention MOVES:
  * relative_position_bias_table ~ N(0, 1);
  * Linear / convolution weights ~ N(0, gain^2 / fan_in): the qkv rows then give q and k of unit variance on LayerNorm-ed input, i.e. scores
    (q 32^-0.5) k^T of order 1; gain 0.5 on the two products that write into the residual stream (attn.proj, mlp.fc2), 1 elsewhere;
  * LayerNorm weight 1 + 0.1 N(0, 1), every bias 0.1 N(0, 1).
tools/gen_swin_golden.py asserts per block that the median row maximum of the attention probabilities is at least 3/64.
One numpy default_rng(seed) stream, walked over the SORTED parameter names."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

EMBED, DEPTHS, HEADS, MLP_RATIO, PATCH, WINDOW = 96, (2, 2, 6, 2), (3, 6, 12, 24), 4, 4, 8


def _block_spec(spec, prefix, dim, heads):
    hid = dim * MLP_RATIO
    for n in ("norm1", "norm2"):
        spec[f"{prefix}.{n}.weight"] = (dim,)
        spec[f"{prefix}.{n}.bias"] = (dim,)
    spec[f"{prefix}.attn.relative_position_bias_table"] = ((2 * WINDOW - 1) ** 2, heads)
    spec[f"{prefix}.attn.qkv.weight"] = (3 * dim, dim)
    spec[f"{prefix}.attn.qkv.bias"] = (3 * dim,)
    spec[f"{prefix}.attn.proj.weight"] = (dim, dim)
    spec[f"{prefix}.attn.proj.bias"] = (dim,)
    spec[f"{prefix}.mlp.fc1.weight"] = (hid, dim)
    spec[f"{prefix}.mlp.fc1.bias"] = (hid,)
    spec[f"{prefix}.mlp.fc2.weight"] = (dim, hid)
    spec[f"{prefix}.mlp.fc2.bias"] = (dim,)


def _ln(spec, name, dim):
    spec[name + ".weight"] = (dim,)
    spec[name + ".bias"] = (dim,)


def swin_spec() -> "OrderedDict[str, tuple]":
    """name -> shape of every parameter of SwinUnet(img_size, window_size=8) (the shapes do not depend on img_size); SwinUnet.py:579-668"""
    spec = OrderedDict()
    P = "swin_unet."
    spec[P + "patch_embed.proj.weight"] = (EMBED, 3, PATCH, PATCH)
    spec[P + "patch_embed.proj.bias"] = (EMBED,)
    _ln(spec, P + "patch_embed.norm", EMBED)
    nl = len(DEPTHS)
    for i in range(nl):
        dim = EMBED * 2 ** i
        for j in range(DEPTHS[i]):
            _block_spec(spec, f"{P}layers.{i}.blocks.{j}", dim, HEADS[i])
        if i < nl - 1:
            spec[f"{P}layers.{i}.downsample.reduction.weight"] = (2 * dim, 4 * dim)
            _ln(spec, f"{P}layers.{i}.downsample.norm", 4 * dim)
    for i in range(nl):
        k = nl - 1 - i
        dim = EMBED * 2 ** k
        if i == 0:
            spec[f"{P}layers_up.0.expand.weight"] = (2 * dim, dim)
            _ln(spec, f"{P}layers_up.0.norm", dim // 2)
            continue
        spec[f"{P}concat_back_dim.{i}.weight"] = (dim, 2 * dim)
        spec[f"{P}concat_back_dim.{i}.bias"] = (dim,)
        for j in range(DEPTHS[k]):
            _block_spec(spec, f"{P}layers_up.{i}.blocks.{j}", dim, HEADS[k])
        if i < nl - 1:
            spec[f"{P}layers_up.{i}.upsample.expand.weight"] = (2 * dim, dim)
            _ln(spec, f"{P}layers_up.{i}.upsample.norm", dim // 2)
    _ln(spec, P + "norm", EMBED * 2 ** (nl - 1))
    _ln(spec, P + "norm_up", EMBED)
    spec[P + "up.expand.weight"] = (16 * EMBED, EMBED)
    _ln(spec, P + "up.norm", EMBED)
    spec[P + "output.weight"] = (1, EMBED, 1, 1)
    return spec


def _is_norm(name: str) -> bool:
    return name.split(".")[-2].startswith("norm")


def make_swin_params(seed: int) -> "OrderedDict[str, np.ndarray]":
    spec = swin_spec()
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name in sorted(spec):
        shape = spec[name]
        z = rng.standard_normal(shape)
        if name.endswith("relative_position_bias_table"):
            v = z
        elif _is_norm(name):
            v = 1.0 + 0.1 * z if name.endswith(".weight") else 0.1 * z
        elif len(shape) == 1:
            v = 0.1 * z
        else:
            gain = 0.5 if (".attn.proj." in name or ".mlp.fc2." in name) else 1.0
            v = z * gain / np.sqrt(float(np.prod(shape[1:])))
        out[name] = v.astype(np.float32)
    return out
