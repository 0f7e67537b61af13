"""The squeeze-excite adapter operator (csrc/se_adapter.hip through ops.se_adapter) and the two models built on it, BASE_DASE / BASE_USE:
  (1) the operator against an fp64 restatement written here, forward and every gradient, bounded by the error of the SAME formula in fp32 on the CPU;
  (2) bit-identical repeats;  (3) an input that needs no gradient (dx == NULL), with a guard region behind the workspace;
  (4) one train step and the eval logits against the fixtures the real reference produced (tools/gen_adapter_golden.py);
  (5) train.base_train_step with fuse_domains == one forward per domain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_model import TOL, check, check_grad, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [("dase", 2, 4, 512), ("dase", 3, 256, 64), ("dase", 2, 100, 320), ("dase", 1, 1, 64), ("dase", 2, 4100, 128),
          ("use", 2, 4, 512), ("use", 3, 256, 64), ("use", 2, 100, 320), ("use", 1, 1, 64), ("use", 2, 4100, 128), ("use", 2, 4, 1024)]


def make_case(kind, B, N, Cn, seed=0):
    """fp64 CPU tensors: x, the upstream gradient, and the parameters in ops.se_adapter's order, at a scale where the gates vary"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * N + Cn + (0 if kind == "dase" else 1))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rn(B, N, Cn) + 0.5 * rn(B, 1, Cn)
    gy = rn(B, N, Cn)
    r = Cn // 16 if kind == "dase" else Cn // 8
    branch = lambda: [rn(r, Cn) * (2.0 / Cn ** 0.5), 0.3 * rn(r), rn(Cn, r) * (1.5 / r ** 0.5), 0.3 * rn(Cn)]
    if kind == "dase":
        P = [rn(4, Cn) * (2.0 / Cn ** 0.5), 0.3 * rn(4)]
        for _ in range(4):
            P += branch()
    else:
        P = branch()
    return x, gy, P


def se_restated(x, kind, P):
    """domain_attention_module.py:50-66 / base_sota_adapt.py:628-637 on tokens [B, N, C], in the dtype of its arguments"""
    p = x.mean(1)
    se = lambda W1, b1, W2, b2: torch.relu(p @ W1.t() + b1) @ W2.t() + b2
    if kind == "dase":
        w = torch.softmax(p @ P[0].t() + P[1], dim=1)                                   # [B, 4]
        z = torch.stack([se(*P[2 + 4 * k:6 + 4 * k]) for k in range(4)], dim=2)        # [B, C, 4]
        s = torch.sigmoid(torch.matmul(z, w.unsqueeze(2)).squeeze(2))
        return x * s.unsqueeze(1)
    s = torch.sigmoid(se(*P))
    return s.unsqueeze(1) * x + x


def run_restated(x, gy, P, kind, dtype):
    xs = x.to(dtype).clone().requires_grad_(True)
    Ps = [t.to(dtype).clone().requires_grad_(True) for t in P]
    y = se_restated(xs, kind, Ps)
    y.backward(gy.to(dtype))
    return [y.detach().double()] + [xs.grad.double()] + [t.grad.double() for t in Ps]


def run_op(x, gy, P, kind, x_grad=True):
    from mdvit_amd import ops
    xs = x.float().to(dev()).requires_grad_(x_grad)
    Ps = [t.float().to(dev()).requires_grad_(True) for t in P]
    y = ops.se_adapter(xs, kind, Ps)
    y.backward(gy.float().to(dev()))
    torch.cuda.synchronize()
    return [y.detach()] + [xs.grad] + [t.grad for t in Ps]


def rel_l2(a, b):
    return float((a.double().cpu() - b).norm() / max(float(b.norm()), 1e-300))


def tensor_names(kind):
    names = ["y", "dx"]
    if kind == "dase":
        names += ["dWg", "dbg"] + [f"d{n}_{k}" for k in range(4) for n in ("W1", "b1", "W2", "b2")]
    else:
        names += ["dW1", "db1", "dW2", "db2"]
    return names


@pytest.mark.parametrize("kind,B,N,Cn", SHAPES)
def test_operator_matches_fp64_restatement_within_10x_the_fp32_cpu_error(kind, B, N, Cn):
    """Bound per tensor (relative L2 against fp64): 10 x the error of the same formula evaluated by torch in fp32 on the CPU on the same inputs.
    The kernels differ from that baseline only in summation order and expf."""
    x, gy, P = make_case(kind, B, N, Cn)
    want = run_restated(x, gy, P, kind, torch.float64)
    base = run_restated(x, gy, P, kind, torch.float32)
    got = run_op(x, gy, P, kind)
    bad = []
    for name, w, b32, o in zip(tensor_names(kind), want, base, got):
        assert o is not None and tuple(o.shape) == tuple(w.shape), name
        e_base, e_op = rel_l2(b32, w), rel_l2(o, w)
        print(f"{kind} ({B},{N},{Cn}) {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  bound {10 * e_base:.3e}")
        if not (np.isfinite(e_op) and e_op <= 10.0 * e_base):
            bad.append((name, e_op, e_base))
    assert not bad, bad


@pytest.mark.parametrize("kind,B,N,Cn", [("dase", 2, 4100, 128), ("dase", 2, 100, 320), ("use", 2, 4, 1024), ("use", 3, 256, 64)])
def test_same_call_twice_is_bit_identical(kind, B, N, Cn):
    x, gy, P = make_case(kind, B, N, Cn, seed=1)
    a, b = run_op(x, gy, P, kind), run_op(x, gy, P, kind)
    for name, u, v in zip(tensor_names(kind), a, b):
        assert torch.equal(u, v), name


@pytest.mark.parametrize("kind,B,N,Cn", [("dase", 2, 100, 320), ("use", 3, 256, 64), ("use", 1, 1, 64)])
def test_input_without_gradient_and_workspace_guard(kind, B, N, Cn):
    """x.requires_grad == False: no dx, the parameter gradients still match; at the C ABI dx == NULL writes nothing outside the mdvit_se_adapter_ws_bytes
    bytes of workspace (a sentinel-filled guard region behind it stays intact) and yields the same parameter gradients, bit for bit, as a call with dx."""
    from mdvit_amd import _lib, ops
    x, gy, P = make_case(kind, B, N, Cn, seed=2)
    want = run_restated(x, gy, P, kind, torch.float64)
    base = run_restated(x, gy, P, kind, torch.float32)
    got = run_op(x, gy, P, kind, x_grad=False)
    assert got[1] is None
    for name, w, b32, o in list(zip(tensor_names(kind), want, base, got))[2:]:
        e_base, e_op = rel_l2(b32, w), rel_l2(o, w)
        print(f"{kind} ({B},{N},{Cn}) no-dx {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}")
        assert np.isfinite(e_op) and e_op <= 10.0 * e_base, (name, e_op, e_base)
    # the C ABI with caller-owned buffers
    lib = _lib.load()
    f = lambda t: t.float().to(dev()).contiguous()
    xs, gs = f(x), f(gy)
    if kind == "dase":
        Wg, bg = f(P[0]), f(P[1])
        W1, b1, W2, b2 = (torch.stack([f(P[2 + 4 * k + i]) for k in range(4)]) for i in range(4))
    else:
        (W1, b1, W2, b2), Wg, bg = [f(t) for t in P], None, None
    d = ops._se_desc(ops.SE_KINDS[kind], B, N, Cn, W1.shape[-2], W1, b1, W2, b2, Wg, bg)
    save_b, ws_b = lib.mdvit_se_adapter_save_bytes(C.byref(d)), lib.mdvit_se_adapter_ws_bytes(C.byref(d))
    assert save_b > 0 and ws_b > 0 and ws_b % 16 == 0
    GUARD, SENT = 4096, -12345.5
    st = ops._stream()
    y, save = torch.empty_like(xs), torch.empty(save_b // 4, device=dev())
    res = []
    for with_dx in (True, False):
        ws = torch.full((ws_b // 4 + GUARD,), SENT, device=dev())
        gpar = [torch.full_like(t, SENT) if t is not None else None for t in (W1, b1, W2, b2, Wg, bg)]
        dx = torch.full_like(xs, SENT)
        ops.call("mdvit_se_adapter_fwd", C.byref(d), ops._p(xs), ops._p(y), ops._p(save), ops._p(ws), ws_b, st)
        ops.call("mdvit_se_adapter_bwd", C.byref(d), ops._p(gs), ops._p(xs), ops._p(save), ops._p(dx) if with_dx else None, *[ops._p(t) for t in gpar],
                 ops._p(ws), ws_b, st)
        torch.cuda.synchronize()
        assert bool((ws[ws_b // 4:] == SENT).all()), "the guard region behind the workspace was written"
        assert bool((dx == SENT).all()) == (not with_dx)
        res.append(gpar)
    for u, v in zip(*res):
        if u is not None:
            assert not bool((u == SENT).any()) and torch.equal(u, v)
    check(y, want[0], tol=1e-5, name="C ABI y")


def _build(model, seed):
    import mdvit_amd
    from adapter_params import make_adapter_params
    from test_gpu_model import load_params
    m = getattr(mdvit_amd, model)(img_size=64, drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d)
    load_params(m, make_adapter_params(seed, model))
    return m.to(dev())


@pytest.mark.parametrize("model", ["BASE_DASE", "BASE_USE"])
def test_adapter_models_step_and_eval_vs_reference_fixture(golden, gemm_precision, model):
    """one step of multi_train_BASE.py:168-200 on the reference's fixture: logits, loss, gradient norms at the tolerances of test_base_step_vs_golden (the same
    trunk); the first four elements of every gradient within 5e-3 of that gradient's norm (an L2 error of 5e-3 of the norm, the bound the norms get, moves
    no element by more than that); then the BatchNorm running statistics and the eval-mode logits of the same weights."""
    from mdvit_amd.losses import seg_loss
    from oracle.gen_golden import grad_digest, synth_image, synth_label
    g = golden(model.lower() + "_step_64")
    S, B, seed, bn_stride = [int(v) for v in g["meta"]]
    m = _build(model, seed).train()
    img, lab = synth_image(1500 + seed, B, S, S).to(dev()), synth_label(1600 + seed, B, S, S).to(dev())
    out = m(img)
    check(out, g["out"], name=model + " out")
    loss = seg_loss(out, lab)
    check(loss, g["loss"], name=model + " loss")
    loss.backward()
    names, norms, heads = grad_digest({n: p.grad.detach().cpu() for n, p in m.named_parameters()})
    assert names == [str(n) for n in g["grad_names"]]
    ref = g["grad_norms"]
    rel = np.abs(norms - ref) / np.maximum(ref, 1e-6 * ref.max())
    print(f"{model} {gemm_precision}: worst gradient norm {names[int(rel.argmax())]} {rel.max():.2e}")
    assert rel.max() < 5e-3, f"{names[int(rel.argmax())]} {rel.max():.2e}"
    herr = np.abs(heads - g["grad_heads"]).max(axis=1) / np.maximum(ref, 1e-6 * ref.max())
    assert herr.max() < 5e-3, f"{names[int(herr.argmax())]} {herr.max():.2e}"
    assert min(norms[i] for i, n in enumerate(names) if "adapter" in n) > 0.0          # every adapter parameter is reached
    sd = m.state_dict()
    bn_names = sorted(k for k in sd if k.endswith("running_mean") or k.endswith("running_var"))
    bn = torch.cat([sd[k].reshape(-1).float() for k in bn_names]).cpu().numpy()[::bn_stride]
    check(bn, g["bn_sample"], name=model + " BN running statistics")
    m.eval()
    with torch.no_grad():
        check(m(img), g["out_eval"], name=model + " eval out")


@pytest.mark.parametrize("model", ["BASE_DASE", "BASE_USE"])
def test_base_train_step_fused_domains_equal_per_domain_forwards(model):
    """train.base_train_step(fuse_domains=2): ONE forward over two concatenated domain batches (BatchNorm statistics per batch; the adapters are per sample) ==
    one forward per domain -- loss, every gradient, every buffer; bounded as test_domain_batched_step_equals_per_domain_forwards bounds MDViT's"""
    from mdvit_amd.train import base_train_step
    from oracle.gen_golden import synth_image, synth_label
    batches = [(synth_image(1700 + d, 2, 64, 64).to(dev()), synth_label(1710 + d, 2, 64, 64).to(dev()), torch.full((2,), d, dtype=torch.long)) for d in range(2)]
    res = []
    for fuse in (1, 2):
        m = _build(model, 15).train()
        out = base_train_step(m, batches, optimizer=None, fuse_domains=fuse)
        res.append((out, {n: p.grad.clone() for n, p in m.named_parameters()}, {n: b.clone() for n, b in m.named_buffers()}))
    check(res[0][0]["loss"], res[1][0]["loss"], tol=1e-5, name="loss")
    for n in res[0][1]:
        check_grad(res[1][1][n], res[0][1][n], name=n, l2_tol=1e-3, max_tol=1e-2)
    for n in res[0][2]:
        check(res[1][2][n].double(), res[0][2][n].double(), tol=1e-5, name=n)


def test_adapter_train_step_with_fused_adamw_moves_every_adapter_parameter():
    """base_train_step + GradAccumulator + FusedAdamW (the bench's step harness) on BASE_USE: the adapters' gradients reach the buckets through autograd's
    .grad (they have no sink) and the fused optimizer updates them"""
    from mdvit_amd import ops
    from mdvit_amd.optim import FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    from mdvit_amd.train import base_train_step
    from oracle.gen_golden import synth_image, synth_label
    m = _build("BASE_USE", 16).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters() if "adapter" in n}
    acc = GradAccumulator(list(m.parameters()))
    acc.attach_sinks(True)
    try:
        opt = FusedAdamW(acc, lr=1e-3)
        batch = [(synth_image(1800, 2, 64, 64).to(dev()), synth_label(1810, 2, 64, 64).to(dev()), torch.zeros(2, dtype=torch.long))]
        out = base_train_step(m, batch, optimizer=opt, accumulator=acc)
        torch.cuda.synchronize()
    finally:
        acc.attach_sinks(False)
    assert np.isfinite(float(out["loss"]))
    for n, p in m.named_parameters():
        if "adapter" in n:
            assert not torch.equal(p.detach(), before[n]), n
