"""Generate tests/golden/utnet_step_128.npz, utnet_step_256.npz and utnet_attention_small.npz by running the REAL reference classes
(Models/Hybrid_models/UTNetFolder: UTNet, LinearAttention, LinearAttentionDecoder -- imported read-only through oracle.ref_import) on the CPU, on the deterministic
weights of tools/utnet_params.py and the inputs of oracle.gen_golden.  Build container only:

    python tools/gen_utnet_golden.py

utnet_step_<S>: one train step as multi_train_BASE.py:168-200 (model(img), BCE + Dice, one backward) at S x S, batch 2, every nn.Dropout.p set to 0 on the
instance, and a digest of every buffer after it; then the eval-mode logits.  The weights carry random running statistics so that the step's momentum update is
pinned, but eval-mode on statistics that do not belong to the activations saturates every attention (logits of 1e4, fp32 and fp64 differing by a third): so
before the eval pass every BatchNorm's momentum is set to 1 and one more train-mode forward of the same batch makes the running statistics that batch's own
(mean and unbiased variance), and the eval logits are taken on those.  The values come from the reference run in FP64; the same
step in the reference's own fp32 gives e32_*, its deviation from them in the statistic the test uses.  Data only: a strided sample of the logits (train and
eval), the loss, a digest of every gradient and of every buffer after the step, the state_dict inventory, the constructor's defaults, the median row maximum of
every attention, and the names of the four biases whose gradient is exactly zero.

Asserted here, because the tests rest on it: every attention's median row maximum is at least 3/64; e32 of the logits is at most 2.5e-4; at most 10 % of the
gradient tensors have e32 > 1e-3; the fp64 gradients of the zero-gradient biases are below 1e-12 of the largest norm and every other norm is positive.

utnet_attention_small: one LinearAttention at 16 x 24 and one LinearAttentionDecoder at q 16 x 16 / x 8 x 8 (the no-resize branch) in fp64 with the table at
std 1, on the inputs and weights of utnet_params.small_attention_case: strided samples of the output, of the returned probabilities and of every input and
parameter gradient for that case's upstream gradient, and relative_position_index."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_adapter_golden import ctor_defaults  # noqa: E402
from oracle.gen_golden import GOLDEN_DIR, _sample, grad_digest, synth_image, synth_label  # noqa: E402
from oracle.ref_import import import_reference, load_params_into  # noqa: E402
from utnet_params import CTOR, SMALL, ZERO_GRAD, make_utnet_params, small_attention_case, small_sample, utnet_spec  # noqa: E402

SEED, B, STRIDE = 5, 2, 37


def _build(ref, dtype):
    m = ref.UTNet(**CTOR)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    load_params_into(m, make_utnet_params(SEED))
    return m.to(dtype)


def _step(ns, m, img, lab, dtype, pmax=None):
    attn = [(n, mod) for n, mod in m.named_modules() if type(mod).__name__ in ("LinearAttention", "LinearAttentionDecoder")]
    hooks = []
    if pmax is not None:
        for n, mod in attn:
            hooks.append(mod.register_forward_hook(lambda _m, _i, o, n=n: pmax.__setitem__(n, float(o[1].detach().max(-1).values.median()))))
    m.train()
    o = m(img.to(dtype))
    for h in hooks:
        h.remove()
    so = torch.sigmoid(o)
    loss = torch.nn.BCELoss()(so, lab.to(dtype)) + ns.dice_loss(so, lab.to(dtype))
    m.zero_grad()
    loss.backward()
    grads = grad_digest({n: p.grad for n, p in m.named_parameters()})
    bufs = grad_digest({n: b.detach().double() for n, b in m.named_buffers()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 1.0
    with torch.no_grad():
        m(img.to(dtype))          # momentum 1: the running statistics ARE this batch's
        m.eval()
        oe = m(img.to(dtype))
    return o.detach(), oe, float(loss.detach()), grads, bufs, [n for n, _ in attn]


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def gen_step(ns, ref, S):
    img, lab = synth_image(1500, B, S, S), synth_label(1600, B, S, S)
    pmax = {}
    m64 = _build(ref, torch.float64)
    spec, bufs_spec = utnet_spec()
    named = dict(m64.named_parameters())
    assert set(named) == set(spec) and all(tuple(named[k].shape) == tuple(s) for k, s in spec.items()), "parameter inventory differs from the reference"
    assert set(dict(m64.named_buffers())) == set(bufs_spec), "buffer inventory differs from the reference"
    o, oe, loss, (names, norms, heads), (bnames, bnorms, bheads), attn_names = _step(ns, m64, img, lab, torch.float64, pmax)
    o32, oe32, loss32, (_, norms32, heads32), _b, _a = _step(ns, _build(ref, torch.float32), img, lab, torch.float32)
    stat = np.array([pmax[n] for n in attn_names])
    for n, v in zip(attn_names, stat):
        print(f"  {S}: {n}: median row maximum {v:.4f}")
        assert v >= 3.0 / 64.0, (n, v)
    floor = np.maximum(norms, 1e-6 * norms.max())
    e32_norm = np.abs(norms32 - norms) / floor
    e32_head = np.abs(heads32.astype(np.float64) - heads.astype(np.float64)).max(axis=1) / floor
    e32_grad = np.maximum(e32_norm, e32_head)
    zero = np.array([n in ZERO_GRAD for n in names])
    e32_out = max(_relmax(_sample(o32, STRIDE), _sample(o, STRIDE)), _relmax(_sample(oe32, STRIDE), _sample(oe, STRIDE)))
    e32_loss = abs(loss32 - loss) / abs(loss)
    print(f"  {S}: loss {loss:.6f}; e32 logits {e32_out:.2e}, loss {e32_loss:.2e}, worst gradient {names[int(np.where(zero, 0, e32_grad).argmax())]} "
          f"{np.where(zero, 0, e32_grad).max():.2e}, {(e32_grad[~zero] > 1e-3).sum()} of {(~zero).sum()} above 1e-3")
    assert e32_out <= 2.5e-4, e32_out
    assert (e32_grad[~zero] > 1e-3).sum() <= 0.1 * (~zero).sum()
    assert zero.sum() == len(ZERO_GRAD) and norms[zero].max() < 1e-12 * norms.max(), norms[zero]
    assert norms[~zero].min() > 0.0
    sd = m64.state_dict()
    keys = sorted(sd)
    shapes = -np.ones((len(keys), 4), np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    return {"out": _sample(o, STRIDE), "out_eval": _sample(oe, STRIDE), "loss": np.array(loss), "grad_names": np.array(names), "grad_norms": norms,
            "grad_heads": heads, "buf_names": np.array(bnames), "buf_norms": bnorms, "buf_heads": bheads, "sd_keys": np.array(keys), "sd_shapes": shapes,
            "ctor": np.array(ctor_defaults(ref.UTNet)), "attn_names": np.array(attn_names), "pmax_median": stat, "zero_grad_names": np.array(sorted(ZERO_GRAD)),
            "e32_out": np.array(e32_out), "e32_loss": np.array(e32_loss), "e32_grad": e32_grad, "meta": np.array([S, B, SEED, STRIDE])}


def gen_small(cu):
    data = {}
    for which, c in SMALL.items():
        params, inputs, gy = small_attention_case(which)
        m = getattr(cu, c["kind"])(*c["args"], **c["kw"]).double()
        load_params_into(m, {k: v for k, v in params.items()})
        m.train()
        ins = {k: torch.from_numpy(v).requires_grad_(True) for k, v in inputs.items()}
        out, prob = m(ins["x"]) if which == "enc" else m(ins["q"], ins["x"])
        m.zero_grad()
        out.backward(torch.from_numpy(gy))
        data[which + "_out"] = small_sample(out)
        data[which + "_prob"] = small_sample(prob)
        for k, t in ins.items():
            data[f"{which}_grad_in_{k}"] = small_sample(t.grad)
        for k, p in m.named_parameters():
            data[f"{which}_grad_{k}"] = small_sample(p.grad)
        data["rel_index"] = m.relative_position_encoding.relative_position_index.numpy().astype(np.int16)
    return data


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ns = import_reference()
    from Models.Hybrid_models.UTNetFolder import UTNet as ref
    from Models.Hybrid_models.UTNetFolder import conv_trans_utils as cu
    out = {"utnet_attention_small": gen_small(cu)}
    for S in (128, 256):
        out[f"utnet_step_{S}"] = gen_step(ns, ref, S)
    for name, data in out.items():
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
