"""Deterministic, name-keyed test weights of BASE_DASE / BASE_USE (shared by tools/gen_adapter_golden.py and tests/test_*adapter*.py).

The trunk takes oracle.params.make_params(seed, model="BASE", adapt_method=False) as it is (the adapter models have BASE's trunk under BASE's names).
The adapters' Linear layers take the same splitmix64 counter generator keyed by the parameter's name, at a scale that makes the gates MOVE: with the
reference's init (trunc-normal 0.02, zero bias) every gate sits at sigmoid(0) = 0.5 whatever the input, and a fixture would pin nothing of the adapter.
tools/gen_adapter_golden.py asserts, per adapter site, that the gates span >= 0.2, that ReLU units are both on and off, and (DASE) that the branch
softmax is not uniform."""
from __future__ import annotations

import math
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (_stream_id is the name -> generator-stream hash make_params itself uses; oracle.params does not export it under a public name yet)
from oracle.params import EMBED_DIMS, _stream_id, make_params, uniform_pm1  # noqa: E402

MODELS = ("BASE_DASE", "BASE_USE")
GAIN_IN, GAIN_OUT, BIAS = 1.0, 1.0, 0.3          # fc.0 / fc_1 (C -> hidden / branches), fc.2 (hidden -> C), every bias


def adapter_sites(model: str):
    """[(module prefix, channels)] in forward order"""
    E = list(EMBED_DIMS)
    sites = [(f"encoder_adapters.{i}", E[i]) for i in range(4)]
    if model == "BASE_USE":
        sites.append(("bridge_adapter", 2 * E[3]))
    sites += [(f"decoder_adapters.{i}", E[-i - 1]) for i in range(4)]
    return sites


def adapter_spec(model: str) -> "OrderedDict[str, tuple]":
    """name -> shape of every adapter parameter (se_module_vector.py:8-25, domain_attention_module.py:45-46, base_sota_adapt.py:346-351,524-530)"""
    if model not in MODELS:
        raise KeyError(model)
    spec = OrderedDict()
    for prefix, C in adapter_sites(model):
        if model == "BASE_DASE":
            r = C // 16
            for k in range(4):
                spec[f"{prefix}.SE_Layers.{k}.fc.0.weight"] = (r, C)
                spec[f"{prefix}.SE_Layers.{k}.fc.0.bias"] = (r,)
                spec[f"{prefix}.SE_Layers.{k}.fc.2.weight"] = (C, r)
                spec[f"{prefix}.SE_Layers.{k}.fc.2.bias"] = (C,)
            spec[f"{prefix}.fc_1.weight"] = (4, C)
            spec[f"{prefix}.fc_1.bias"] = (4,)
        else:
            r = C // 8
            spec[f"{prefix}.se_layer.fc.0.weight"] = (r, C)
            spec[f"{prefix}.se_layer.fc.0.bias"] = (r,)
            spec[f"{prefix}.se_layer.fc.2.weight"] = (C, r)
            spec[f"{prefix}.se_layer.fc.2.bias"] = (C,)
    return spec


def make_adapter_params(seed: int, model: str) -> "OrderedDict[str, np.ndarray]":
    out = make_params(seed, model="BASE", adapt_method=False)
    for name, shape in adapter_spec(model).items():
        u = uniform_pm1(seed, _stream_id(name), int(np.prod(shape)))
        if len(shape) == 1:
            v = BIAS * u
        else:
            v = u * (GAIN_OUT if ".fc.2." in name else GAIN_IN) * math.sqrt(3.0 / shape[1])
        out[name] = v.astype(np.float32).reshape(shape)
    return out
