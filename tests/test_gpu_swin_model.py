"""GPU: SwinUnet end to end.
  (1) one train step of multi_train_BASE.py:168-200 and the eval logits against the fixture the real reference class produced (tools/gen_swin_golden.py),
      under both GEMM precisions, at the README's / test_gpu_adapter.py's bounds: logits sample and loss within 1e-3, gradient norms within 5e-3, eval
      logits within 1e-3;
  (2) DropPath on: the step runs, gradients are finite, two runs from one seed agree bit for bit, a sample whose scale was drawn as 0 contributes exactly
      its shortcut;
  (3) the loss graph holds no torch-native kernel; (4) train.base_train_step and evaluate() drive the model as they drive BASE."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_model import TOL, check, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

FIXTURE = "swinunet_step_256"


def _build(seed, drop_path=False):
    import mdvit_amd
    from swin_params import make_swin_params
    m = mdvit_amd.SwinUnet(img_size=256, window_size=8)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in make_swin_params(seed).items()}, strict=False)
    assert not unexpected and all(k.endswith(("relative_position_index", "attn_mask")) for k in missing), (missing[:5], unexpected[:5])
    if not drop_path:
        for mod in m.modules():
            if hasattr(mod, "drop_path_p"):
                mod.drop_path_p = 0.0
    return m.to(dev())


def _sample(t, stride):
    return t.detach().reshape(-1)[::stride].float().cpu().numpy()


def test_step_and_eval_vs_reference_fixture(golden, gemm_precision):
    from mdvit_amd.losses import seg_loss
    from oracle.gen_golden import grad_digest, synth_image, synth_label
    g = golden(FIXTURE)
    S, B, seed, stride = [int(v) for v in g["meta"]]
    m = _build(seed).train()
    img, lab = synth_image(1500 + seed, B, S, S).to(dev()), synth_label(1600 + seed, B, S, S).to(dev())
    out = m(img)
    assert tuple(out.shape) == (B, 1, S, S)
    check(_sample(out, stride), g["out"], name="out")
    loss = seg_loss(out, lab)
    check(loss, g["loss"], name="loss")
    loss.backward()
    torch.cuda.synchronize()
    names, norms, heads = grad_digest({n: p.grad.detach().cpu() for n, p in m.named_parameters()})
    assert names == [str(n) for n in g["grad_names"]]
    ref = g["grad_norms"]
    rel = np.abs(norms - ref) / np.maximum(ref, 1e-6 * ref.max())
    print(f"SwinUnet {gemm_precision}: worst gradient norm {names[int(rel.argmax())]} {rel.max():.2e}")
    assert rel.max() < 5e-3, f"{names[int(rel.argmax())]} {rel.max():.2e}"
    herr = np.abs(heads - g["grad_heads"]).max(axis=1) / np.maximum(ref, 1e-6 * ref.max())
    assert herr.max() < 5e-3, f"{names[int(herr.argmax())]} {herr.max():.2e}"
    assert norms.min() > 0.0          # every parameter is reached
    m.eval()
    with torch.no_grad():
        check(_sample(m(img), stride), g["out_eval"], name="eval out")
        one = m(img[:, :1].contiguous())          # a 1-channel input is repeated to 3 channels (SwinUnet.py:792-796)
        check(one, m(img[:, :1].repeat(1, 3, 1, 1)), tol=1e-6, name="1-channel input")


def test_loss_graph_holds_no_torch_native_kernel():
    from mdvit_amd import ops
    from mdvit_amd.losses import seg_loss
    from oracle.gen_golden import synth_image, synth_label
    m = _build(3, drop_path=True).train()
    loss = seg_loss(m(synth_image(1, 1, 256, 256).to(dev())), synth_label(2, 1, 256, 256).to(dev()))
    native, fanin = ops.audit_sweep_graph(loss)
    assert native == [] and fanin == [], (native, fanin)


def test_droppath_step_is_finite_and_repeatable():
    from mdvit_amd import ops
    from mdvit_amd.losses import seg_loss
    from oracle.gen_golden import synth_image, synth_label
    img, lab = synth_image(11, 2, 256, 256).to(dev()), synth_label(12, 2, 256, 256).to(dev())
    runs = []
    for _ in range(2):
        m = _build(4, drop_path=True).train()
        ops._key_counter = itertools.count(5)          # the same DropPath keys in every run
        torch.manual_seed(1234)
        out = m(img)
        seg_loss(out, lab).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
        drawn = [mod.last_scales.clone() for mod in m.modules() if getattr(mod, "last_scales", None) is not None]
        runs.append((out.detach().clone(), grads, drawn))
    assert len(runs[0][2]) == 20          # every block but the two with drop_path 0 drew its scales
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_a_dropped_sample_contributes_exactly_its_shortcut():
    """one shifted block at drop_path 0.5 through the module, the drawn scales read back: scales are 0 or 1 / keep; a sample with both branches dropped
    leaves the block as it entered, bit for bit; one with only the attention branch dropped is x + scale * Mlp(LN2(x))"""
    from mdvit_amd import ops
    from mdvit_amd.swin import SwinTransformerBlock
    torch.manual_seed(5)
    blk = SwinTransformerBlock(96, (16, 16), 3, 8, 4, 4.0, 0.5).to(dev()).train()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn_like(p) * (1.0 if p.dim() == 1 or p.shape[0] == 225 else p.shape[1] ** -0.5))
    Bn = 64
    x = torch.randn(Bn, 256, 96, device=dev())
    y = blk(x)
    s = blk.last_scales.cpu()
    assert tuple(s.shape) == (2, Bn) and set(s.unique().tolist()) <= {0.0, 2.0}
    both = (s[0] == 0) & (s[1] == 0)
    attn_only = (s[0] == 0) & (s[1] != 0)
    kept = (s[0] != 0) & (s[1] != 0)
    assert bool(both.any()) and bool(attn_only.any()) and bool(kept.any())
    assert torch.equal(y[both.to(dev())], x[both.to(dev())])
    assert not torch.equal(y[kept.to(dev())], x[kept.to(dev())])
    xs = x[attn_only.to(dev())].contiguous()
    m = blk.mlp
    want = xs + 2.0 * (ops.mlp_residual(blk.norm2(xs), torch.zeros_like(xs), m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, None, 0.0, 256))
    check(y[attn_only.to(dev())], want, tol=1e-5, name="attention branch dropped")


def test_base_train_step_updates_every_parameter():
    """base_train_step + GradAccumulator + FusedAdamW (the bench's step harness) over four synthetic domain batches"""
    from mdvit_amd.optim import FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    from mdvit_amd.train import base_train_step
    from oracle.gen_golden import synth_image, synth_label
    m = _build(6, drop_path=True).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    acc = GradAccumulator(list(m.parameters()))
    acc.attach_sinks(True)
    try:
        opt = FusedAdamW(acc, lr=1e-3)
        batches = [(synth_image(1800 + d, 1, 256, 256).to(dev()), synth_label(1810 + d, 1, 256, 256).to(dev()), torch.full((1,), d, dtype=torch.long)) for d in range(4)]
        out = base_train_step(m, batches, optimizer=opt, accumulator=acc)
        torch.cuda.synchronize()
    finally:
        acc.attach_sinks(False)
    assert np.isfinite(float(out["loss"]))
    same = [n for n, p in m.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not same, same[:5]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_table_gradient_through_a_sink_equals_the_autograd_gradient():
    """the gradient-sink route of ops.window_attention (table gradient accumulated by the kernel's second stage, on the side stream) == the plain route"""
    from mdvit_amd import ops
    torch.manual_seed(9)
    B, H, W, heads = 2, 16, 16, 3
    qkv = torch.randn(B, H * W, 3 * heads * 32, device=dev(), requires_grad=True)
    table = torch.randn(225, heads, device=dev(), requires_grad=True)
    gy = torch.randn(B, H * W, heads * 32, device=dev())
    ops.window_attention(qkv, table, H, W, heads, 4).backward(gy)
    want_t, want_x = table.grad.clone(), qkv.grad.clone()
    table.grad = qkv.grad = None
    sink = torch.ones_like(table)
    had_side = ops._side_stream is not None
    ops.enable_side_stream(True)
    ops.set_grad_sinks({table: sink})
    try:
        ops.window_attention(qkv, table, H, W, heads, 4).backward(gy)
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        ops.set_grad_sinks(None)
        ops.enable_side_stream(had_side)
    assert table.grad is None and torch.equal(qkv.grad, want_x)
    assert torch.equal(sink, 1.0 + want_t)


def test_evaluate_scores_the_model():
    from mdvit_amd import evaluate
    from oracle.gen_golden import synth_image, synth_label
    m = _build(7).train()
    loader = [(synth_image(1900 + i, 2, 256, 256), synth_label(1910 + i, 2, 256, 256), torch.zeros(2, dtype=torch.long)) for i in range(2)]
    res = evaluate(m, {0: loader}, num_domains=1, use_domain_label=False)
    assert m.training and res["total_images"] == 4
    for k in ("avg_dice", "avg_iou"):
        assert np.isfinite(res[k]) and 0.0 <= res[k] <= 1.0, (k, res[k])
    assert np.isfinite(res["dice"][0]) and np.isfinite(res["iou"][0])
    assert np.isfinite(res["sum_loss"])
