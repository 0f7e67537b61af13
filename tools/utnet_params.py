"""Deterministic, name-keyed test weights and buffers of UTNet (shared by tools/gen_utnet_golden.py and tests/test_*utnet*.py).

The reference's own initialisation (a 0.02 bias table, kaiming-uniform products on BatchNorm-ed input) leaves the attention close to uniform, and fresh BatchNorm
buffers (0 / 1) would pin nothing of the running statistics.  Here
  * every 4-d weight ~ N(0, 1.5 / fan_in); the pointwise products that make q, k and v (to_qkv / to_q / to_kv) times GAIN;
  * BatchNorm weight 1 + 0.2 N(0, 1), every bias 0.1 N(0, 1), bias tables ~ N(0, 1);
  * running_mean 0.1 N(0, 1), running_var U[0.5, 1.5], num_batches_tracked 0.
GAIN = 0.7 is a compromise the generator asserts from both sides: the median row maximum of every attention is at least 3/64 (the softmax, the bias and the
cell indexing all matter), while the model stays well-conditioned enough that the reference's own fp32 run reproduces its fp64 logits to 2.5e-4 (at twice the
fan-in scale the attention is peaked and fp32 and fp64 logits differ by 0.05 - 0.3: nothing could be pinned to 1e-3).
One numpy default_rng(seed) stream, walked over the SORTED names of parameters and buffers together."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

BASE, HEADS, GAIN = 32, 4, 0.7
CTOR = dict(in_chan=3, base_chan=BASE, num_classes=1, reduce_size=8, block_list='1234', num_blocks=[1, 1, 1, 1], num_heads=[4, 4, 4, 4], projection='interp',
            attn_drop=0.1, proj_drop=0.1, rel_pos=True, aux_loss=False, maxpool=True)
# parameters whose gradient is exactly zero in train mode: a per-channel constant in front of a batch-statistics BatchNorm cancels
ZERO_GRAD = ("up1.attn_decoder.conv_ch.bias", "up2.attn_decoder.conv_ch.bias", "up3.attn_decoder.conv_ch.bias", "up4.conv_ch.bias")


def _bn(spec, bufs, name, c):
    spec[name + ".weight"] = (c,)
    spec[name + ".bias"] = (c,)
    bufs[name + ".running_mean"] = (c,)
    bufs[name + ".running_var"] = (c,)
    bufs[name + ".num_batches_tracked"] = ()


def _basic(spec, bufs, p, inp, out):
    spec[p + ".conv1.weight"] = (out, inp, 3, 3)
    _bn(spec, bufs, p + ".bn1", inp)
    spec[p + ".conv2.weight"] = (out, out, 3, 3)
    _bn(spec, bufs, p + ".bn2", out)
    if inp != out:
        _bn(spec, bufs, p + ".shortcut.0", inp)
        spec[p + ".shortcut.2.weight"] = (out, inp, 1, 1)


def _dsc(spec, p, i, o):
    spec[p + ".depthwise.weight"] = (i, 1, 3, 3)
    spec[p + ".pointwise.weight"] = (o, i, 1, 1)


def _table(spec, bufs, p):
    spec[p + ".relative_position_encoding.relative_position_bias_table"] = (225, HEADS)
    bufs[p + ".relative_position_encoding.relative_position_index"] = (64, 64)


def _trans(spec, bufs, p, c):
    _bn(spec, bufs, p + ".bn1", c)
    _dsc(spec, p + ".attn.to_qkv", c, 3 * c)
    _dsc(spec, p + ".attn.to_out", c, c)
    _table(spec, bufs, p + ".attn")
    _bn(spec, bufs, p + ".bn2", c)
    spec[p + ".mlp.weight"] = (c, c, 1, 1)


def _decoder(spec, bufs, p, i, o):
    _bn(spec, bufs, p + ".bn_l", i)
    _bn(spec, bufs, p + ".bn_h", o)
    spec[p + ".conv_ch.weight"] = (o, i, 1, 1)
    spec[p + ".conv_ch.bias"] = (o,)
    _dsc(spec, p + ".attn.to_kv", i, 2 * o)
    _dsc(spec, p + ".attn.to_q", o, o)
    _dsc(spec, p + ".attn.to_out", o, o)
    _table(spec, bufs, p + ".attn")
    _bn(spec, bufs, p + ".bn2", o)
    spec[p + ".mlp.weight"] = (o, o, 1, 1)


def utnet_spec():
    """(parameters, buffers): name -> shape of UTNet(**CTOR) (UTNet.py:19-70)"""
    spec, bufs = OrderedDict(), OrderedDict()
    b = BASE
    _basic(spec, bufs, "inc.0", 3, b)
    _basic(spec, bufs, "inc.1", b, b)
    for k in range(1, 5):
        cin, cout = b * 2 ** (k - 1), b * 2 ** k
        _basic(spec, bufs, f"down{k}.blocks.1", cin, cout)
        _trans(spec, bufs, f"down{k}.blocks.2", cout)
    for name, k in (("up1", 3), ("up2", 2), ("up3", 1)):
        cin, cout = b * 2 ** (k + 1), b * 2 ** k
        _decoder(spec, bufs, name + ".attn_decoder", cin, cout)
        _basic(spec, bufs, name + ".blocks.0", 2 * cout, cout)
    spec["up4.conv_ch.weight"] = (b, 2 * b, 1, 1)
    spec["up4.conv_ch.bias"] = (b,)
    _basic(spec, bufs, "up4.conv.0", 2 * b, b)
    _basic(spec, bufs, "up4.conv.1", b, b)
    spec["outc.weight"] = (1, b, 1, 1)
    spec["outc.bias"] = (1,)
    return spec, bufs


def _value(rng, name, shape, gain):
    if name.endswith("num_batches_tracked"):
        return np.zeros((), np.int64)
    if name.endswith("running_var"):
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    z = rng.standard_normal(shape)
    if name.endswith("relative_position_bias_table"):
        v = z
    elif name.endswith("running_mean"):
        v = 0.1 * z
    elif len(shape) == 4:
        v = z * np.sqrt(1.5 / float(np.prod(shape[1:])))
        if any(name.endswith(s + ".pointwise.weight") for s in ("to_qkv", "to_q", "to_kv")):
            v = v * gain
    elif name.endswith(".weight"):          # one-dimensional: a BatchNorm weight
        v = 1.0 + 0.2 * z
    else:
        v = 0.1 * z
    return v.astype(np.float32)


def make_utnet_params(seed: int, gain: float = GAIN) -> "OrderedDict[str, np.ndarray]":
    """every state_dict entry but the relative_position_index buffers (which the constructor derives)"""
    spec, bufs = utnet_spec()
    shapes = dict(spec)
    shapes.update({k: s for k, s in bufs.items() if not k.endswith("relative_position_index")})
    rng = np.random.default_rng(seed)
    return OrderedDict((name, _value(rng, name, shapes[name], gain)) for name in sorted(shapes))


# ---- the two stand-alone attention modules of tests/golden/utnet_attention_small.npz -----------------------------------------------------------------
SMALL = {
    "enc": dict(kind="LinearAttention", args=(64,), kw=dict(heads=4, dim_head=16, reduce_size=8), x=(1, 64, 16, 24)),
    "dec": dict(kind="LinearAttentionDecoder", args=(128, 64), kw=dict(heads=4, dim_head=16, reduce_size=8), q=(1, 64, 16, 16), x=(1, 128, 8, 8)),
}


def small_attention_case(which: str, seed: int = 11):
    """-> (parameters {name: fp64 array}, inputs {name: fp64 NCHW array}, upstream gradient fp64 NCHW): weights at fan-in scale, the table at std 1"""
    c = SMALL[which]
    rng = np.random.default_rng(seed + (0 if which == "enc" else 1))
    if which == "enc":
        shapes = OrderedDict([("to_qkv.depthwise.weight", (64, 1, 3, 3)), ("to_qkv.pointwise.weight", (192, 64, 1, 1)), ("to_out.depthwise.weight", (64, 1, 3, 3)),
                              ("to_out.pointwise.weight", (64, 64, 1, 1)), ("relative_position_encoding.relative_position_bias_table", (225, 4))])
    else:
        shapes = OrderedDict([("to_kv.depthwise.weight", (128, 1, 3, 3)), ("to_kv.pointwise.weight", (128, 128, 1, 1)), ("to_q.depthwise.weight", (64, 1, 3, 3)),
                              ("to_q.pointwise.weight", (64, 64, 1, 1)), ("to_out.depthwise.weight", (64, 1, 3, 3)), ("to_out.pointwise.weight", (64, 64, 1, 1)),
                              ("relative_position_encoding.relative_position_bias_table", (225, 4))])
    params = OrderedDict()
    for name in sorted(shapes):
        z = rng.standard_normal(shapes[name])
        params[name] = z if name.endswith("table") else z / np.sqrt(float(np.prod(shapes[name][1:])))
    inputs = OrderedDict((k, rng.standard_normal(c[k])) for k in ("q", "x") if k in c)
    hw = c["x"][2:] if which == "enc" else c["q"][2:]
    return params, inputs, rng.standard_normal((1, 64) + tuple(hw))


def small_sample(t) -> np.ndarray:
    """the strided sample of a tensor that utnet_attention_small.npz holds: every 61st element of a large tensor, every 7th of one below 4096 elements"""
    a = t.detach().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = a.reshape(-1)
    return a[::61 if a.size > 4096 else 7].copy()
