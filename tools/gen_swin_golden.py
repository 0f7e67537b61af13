"""Generate tests/golden/swinunet_step_256.npz by running the REAL reference class (Models/Transformer/SwinUnet.py: SwinUnet -- imported read-only through
oracle.ref_import) on the CPU, on the deterministic weights of tools/swin_params.py and the inputs of oracle.gen_golden.  Build container only:

    python tools/gen_swin_golden.py

One train step as multi_train_BASE.py:168-200 (model(img), BCE + Dice, one backward) at img_size 256, window_size 8, batch 2, every DropPath.drop_prob set
to 0 on the instance, then the eval-mode logits of the same weights.  The fixture holds data only: a strided sample of the logits (train and eval), the
loss, a digest of every gradient, the state_dict inventory, the constructor's defaults, per shifted block the per-window count of -100 entries of its
attn_mask, relative_position_index once, and per block the median over rows of the largest attention probability (a forward hook on the reference's own
softmax module).  Asserted here: that median is at least 3/64 in every block (attention is not uniform), and every shifted block has windows with and
without masked pairs."""
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
from swin_params import make_swin_params, swin_spec  # noqa: E402

SEED, S, B, STRIDE = 21, 256, 2, 37


def gen():
    ns = import_reference()
    from Models.Transformer import SwinUnet as ref
    m = ref.SwinUnet(img_size=S, window_size=8)
    spec = swin_spec()
    named = dict(m.named_parameters())
    assert set(named) == set(spec), "parameter inventory differs from the reference"
    assert all(tuple(named[k].shape) == tuple(s) for k, s in spec.items())
    load_params_into(m, make_swin_params(SEED))
    blocks = [(n, mod) for n, mod in m.named_modules() if type(mod).__name__ == "SwinTransformerBlock"]
    for _n, blk in blocks:
        if hasattr(blk.drop_path, "drop_prob"):
            blk.drop_path.drop_prob = 0.0
    pmax = {}
    for n, blk in blocks:
        blk.attn.softmax.register_forward_hook(lambda _m, _i, o, n=n: pmax.__setitem__(n, float(o.detach().max(-1).values.median())))
    m.train()
    img, lab = synth_image(1500 + SEED, B, S, S), synth_label(1600 + SEED, B, S, S)
    o = m(img)
    stat = np.array([pmax[n] for n, _ in blocks])
    for (n, _), v in zip(blocks, stat):
        print(f"  {n}: median row maximum {v:.4f}")
        assert v >= 3.0 / 64.0, (n, v)
    so = torch.sigmoid(o)
    loss = torch.nn.BCELoss()(so, lab) + ns.dice_loss(so, lab)
    m.zero_grad()
    loss.backward()
    names, norms, heads = grad_digest({n: p.grad for n, p in m.named_parameters()})
    sd = m.state_dict()
    keys = sorted(sd)
    shapes = -np.ones((len(keys), 4), np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    mask_blocks, mask_counts, mask_offsets = [], [], [0]
    for n, blk in blocks:
        if blk.attn_mask is None:
            continue
        c = (blk.attn_mask == -100.0).sum((1, 2)).numpy().astype(np.int64)
        assert (c > 0).any() and (c == 0).any(), n
        mask_blocks.append(n)
        mask_counts.append(c)
        mask_offsets.append(mask_offsets[-1] + c.size)
    m.eval()
    with torch.no_grad():
        oe = m(img)
    return {"out": _sample(o, STRIDE), "out_eval": _sample(oe, STRIDE), "loss": np.array(float(loss)), "grad_names": np.array(names), "grad_norms": norms,
            "grad_heads": heads, "sd_keys": np.array(keys), "sd_shapes": shapes, "ctor": np.array(ctor_defaults(ref.SwinUnet)),
            "mask_blocks": np.array(mask_blocks), "mask_counts": np.concatenate(mask_counts), "mask_offsets": np.array(mask_offsets, np.int64),
            "rel_index": blocks[0][1].attn.relative_position_index.numpy().astype(np.int64), "block_names": np.array([n for n, _ in blocks]), "pmax_median": stat,
            "meta": np.array([S, B, SEED, STRIDE])}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    data = gen()
    path = os.path.join(GOLDEN_DIR, "swinunet_step_256.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path)} bytes), loss {float(data['loss']):.6f}")


if __name__ == "__main__":
    main()
