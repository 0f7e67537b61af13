"""Generate tests/golden/base_dase_step_64.npz and base_use_step_64.npz by running the REAL reference classes
(Models/Sota_adapters/base_sota_adapt.py: BASE_DASE, BASE_USE -- imported read-only through oracle.ref_import) on the CPU, on the
deterministic weights of tools/adapter_params.py and the inputs of oracle.gen_golden.  Build container only:

    python tools/gen_adapter_golden.py

One train step as multi_train_BASE.py:168-200 (model(img), BCE + Dice, one backward) at img_size 64, batch 2, drop rates 0, then the eval-mode
logits of the same weights (the running statistics the train forward left).  Fixtures hold data only: logits, loss, a digest of every gradient,
the state_dict inventory, a strided sample of the BatchNorm running statistics, the constructor's defaults, the gate statistics per adapter site."""
from __future__ import annotations

import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from adapter_params import adapter_sites, adapter_spec, make_adapter_params  # noqa: E402
from oracle.gen_golden import GOLDEN_DIR, grad_digest, synth_image, synth_label  # noqa: E402
from oracle.ref_import import import_reference, load_params_into  # noqa: E402

SEEDS = {"BASE_DASE": 13, "BASE_USE": 14}
BN_STRIDE = 37


def ctor_defaults(cls) -> str:
    """the constructor's parameters as JSON [[name, default]]; a LayerNorm partial is written as {"LayerNorm": {keywords}}, a class by its name"""
    rows = []
    for name, p in inspect.signature(cls.__init__).parameters.items():
        if name == "self":
            continue
        if p.kind is inspect.Parameter.VAR_KEYWORD:
            rows.append(["**" + name, None])
            continue
        d = p.default
        if hasattr(d, "func") and hasattr(d, "keywords"):
            d = {d.func.__name__: dict(d.keywords)}
        elif inspect.isclass(d):
            d = d.__name__
        rows.append([name, d])
    return json.dumps(rows)


def bn_sample(sd) -> np.ndarray:
    names = sorted(k for k in sd if k.endswith("running_mean") or k.endswith("running_var"))
    return torch.cat([sd[k].reshape(-1).float() for k in names]).numpy()[::BN_STRIDE].copy()


def watch_gates(m, model):
    """forward hooks on the reference's own sub-modules: per adapter site the gate, the ReLU outputs and (DASE) the branch softmax"""
    seen = {}
    mods = dict(m.named_modules())
    for prefix, _C in adapter_sites(model):
        rec = seen.setdefault(prefix, {"relu": []})
        if model == "BASE_DASE":
            mods[prefix + ".sigmoid"].register_forward_hook(lambda _m, _i, o, rec=rec: rec.__setitem__("gate", o.detach().clone()))
            mods[prefix + ".softmax"].register_forward_hook(lambda _m, _i, o, rec=rec: rec.__setitem__("w", o.detach().clone()))
            relus = [mods[f"{prefix}.SE_Layers.{k}.fc.1"] for k in range(4)]
        else:
            mods[prefix + ".se_layer.fc.3"].register_forward_hook(lambda _m, _i, o, rec=rec: rec.__setitem__("gate", o.detach().clone()))
            relus = [mods[prefix + ".se_layer.fc.1"]]
        for r in relus:
            r.register_forward_hook(lambda _m, _i, o, rec=rec: rec["relu"].append(o.detach().clone()))
    return seen


def check_gates(seen, model):
    rows = []
    for prefix, rec in seen.items():
        g = rec["gate"]
        span = float(g.max() - g.min())
        act = torch.cat([r.reshape(-1) for r in rec["relu"]])
        on, off = int((act > 0).sum()), int((act <= 0).sum())
        wspan = float(rec["w"].max() - rec["w"].min()) if "w" in rec else float("nan")
        print(f"  {model} {prefix}: gate [{float(g.min()):.3f}, {float(g.max()):.3f}], ReLU on {on} / off {off}, softmax span {wspan:.3f}")
        assert span >= 0.2, (prefix, span)
        assert on >= 1 and off >= 1, (prefix, on, off)
        if model == "BASE_DASE":
            assert wspan >= 0.1, (prefix, wspan)
        rows.append([float(g.min()), float(g.max()), on, off, wspan])
        rec["relu"].clear()
    return np.array(rows)


def gen(model: str, S=64, B=2):
    ns = import_reference()
    from Models.Sota_adapters import base_sota_adapt as ref
    seed = SEEDS[model]
    cls = getattr(ref, model)
    m = cls(img_size=S, drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d)
    pn = make_adapter_params(seed, model)
    sd0 = m.state_dict()
    spec = adapter_spec(model)
    assert {k for k in sd0 if "adapter" in k} == set(spec), "adapter inventory differs from the reference"
    assert all(tuple(sd0[k].shape) == tuple(s) for k, s in spec.items())
    load_params_into(m, pn)
    m.train()
    seen = watch_gates(m, model)
    img, lab = synth_image(1500 + seed, B, S, S), synth_label(1600 + seed, B, S, S)
    o = m(img)
    gates = check_gates(seen, model)
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
    bn = bn_sample(sd)
    m.eval()
    with torch.no_grad():
        oe = m(img)
    return {"out": o.detach().numpy().copy(), "loss": np.array(float(loss)), "grad_names": np.array(names), "grad_norms": norms, "grad_heads": heads,
            "sd_keys": np.array(keys), "sd_shapes": shapes, "bn_sample": bn, "out_eval": oe.numpy().copy(), "gates": gates,
            "sites": np.array([p for p, _ in adapter_sites(model)]), "ctor": np.array(ctor_defaults(cls)), "meta": np.array([S, B, seed, BN_STRIDE])}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    for model in ("BASE_DASE", "BASE_USE"):
        data = gen(model)
        path = os.path.join(GOLDEN_DIR, model.lower() + "_step_64.npz")
        np.savez_compressed(path, **data)
        print(f"wrote {path} ({os.path.getsize(path)} bytes), loss {float(data['loss']):.6f}")


if __name__ == "__main__":
    main()
