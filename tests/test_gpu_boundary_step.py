"""The train steps with `boundary_weight`: MDViT (MLPFM) and BASE at 64 x 64, drop rates 0, two images per domain.

weight 0 / omitted: the step of before, bit for bit, and the same result keys.  weight 0.05: every gradient tensor against the same step composed here from the
model's forward, domain_losses / seg_loss, `+ w * (torch.sigmoid(out) * phi)` reduced by torch ops from the same phi, and the reference's plain two sweeps; the
step's "boundary_loss" against the float64 restatement on its own `out`; the verdict of the aux sweep's graph audit with and without the weight."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import build_mdvit, check_grad, load_params
from test_signed_distance_host import loss_ref

pytestmark = pytest.mark.gpu

W_B = 0.05
FLOOR = 1e-5          # the run-to-run bound of test_gpu_model.py's determinism tests


def dev():
    return torch.device("cuda:0")


def batches_64():
    from mdvit_amd.synthetic import make_step_batches
    return make_step_batches(2, 64, rank=0, step=0, device=dev())


def grads_of(m):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def worst_rel_l2(g, g0):
    """the largest per-tensor relative L2 difference and its name; tensors that hold round-off only (a bias in front of a BatchNorm) are left out, as in
    test_gpu_model.py's determinism tests"""
    assert set(g) == set(g0)
    big = max(float(g0[n].double().norm()) for n in g0)
    return max((float((g[n].double() - g0[n].double()).norm()) / float(g0[n].double().norm()), n) for n in g0 if float(g0[n].double().norm()) > 1e-5 * big)


def group_reduce(sp, G, form):
    Bd = sp.shape[0] // G
    parts = [sp[g * Bd:(g + 1) * Bd] for g in range(G)]
    terms = [p.mean() if form == "mean" else p.sum() / p.numel() for p in parts]
    return sum(terms[1:], terms[0])


def composed_mdvit_step(m, batches, w, fuse, form, alpha=0.5):
    """the step by hand: per forward the fused losses, the boundary term by torch ops, the reference's two sweeps (adapters frozen in the first)"""
    from mdvit_amd import ops, train
    from mdvit_amd.losses import domain_losses
    ops.refresh_transposes()
    m.zero_grad(set_to_none=True)
    da = [p for n, p in m.named_parameters() if "domain_layer" in n]
    for b in (train._fuse_batches(batches, fuse, 4, True) if fuse > 1 else batches):
        img, lab, sid = b[0], b[1], b[2].cpu()
        G = b[4] if len(b) > 4 else 1
        Bd = img.shape[0] // G
        d = str(int(sid[0])) if G == 1 else [str(int(sid[g * Bd])) for g in range(G)]
        out, aux = m(img, F.one_hot(sid, 4).float().to(dev()), d)
        l, la, lk = domain_losses(out, aux, lab) if G == 1 else ops.seg_losses_groups(out, aux, lab, G)
        phi = ops.signed_distance(lab).reshape(out.shape)
        lb = group_reduce(torch.sigmoid(out) * phi, G, form)
        for p in da:
            p.requires_grad = False
        la.backward(retain_graph=True)
        for p in da:
            p.requires_grad = True
        (alpha * lk + (1 - alpha) * (l + w * lb)).backward()
    return grads_of(m)


def hook_outputs(m, store):
    return m.register_forward_hook(lambda mod, inp, o: store.append((o[0] if isinstance(o, (tuple, list)) else o).detach().clone()))


def check_boundary_value(res, outs, labels, groups):
    """res["boundary_loss"] by the rule of test_gpu_boundary_loss.py: error against float64 at most 10 x that of torch's fp32 evaluation on the CPU"""
    from mdvit_amd import ops
    want, base = 0.0, torch.zeros((), dtype=torch.float32)
    for out, lab, G in zip(outs, labels, groups):
        phi = ops.signed_distance(lab).reshape(out.shape).cpu()
        want += loss_ref(out.cpu().numpy(), phi.numpy(), G)
        base = base + group_reduce(torch.sigmoid(out.cpu()) * phi, G, "mean")
    got = float(res["boundary_loss"])
    e_op, e_base = abs(got - want) / abs(want), abs(float(base) - want) / abs(want)
    print(f"boundary_loss {got!r} (float64 {want!r}): op {e_op:.3e}  fp32-cpu {e_base:.3e}  ratio {e_op / max(e_base, 1e-300):.3f}")
    assert e_op <= 10.0 * e_base, (e_op, e_base)


@pytest.mark.parametrize("fuse", [1, 4], ids=["per_domain_forward", "fused_forward"])
def test_mdvit_step_weight_zero_is_the_step_of_before_and_weight_w_adds_the_torch_ops_term(fuse):
    """Bound: 10 x the largest per-tensor deviation between the two torch-ops forms of the term (.mean() / .sum() / N), floored at 1e-5.
    Measured on an MI355X (relative L2 per gradient tensor, worst tensor): the two forms differ by exactly 0 (their backward is the same expansion of g / N),
    so the bound is its floor, 1e-5.  The step against the torch-ops step: exactly 0 in all three configurations -- mdvit_boundary_loss_bwd takes its roundings
    in autograd's own order, (((g (1 / N)) phi) (1 - s)) s, and ops.fork's addition is the engine's.  (With the product associated as (g / N phi) ((1 - s) s)
    a third of the elements differed by an ulp, 4.7e-8 relative L2, and LayerNorm / adapter bias gradients -- sums with cancellation -- amplified that to
    1.5e-5 .. 2.1e-5: the comparison bites.)  The term itself moves the gradients by 0.38 (0.21 BASE)."""
    from mdvit_amd.train import mdvit_train_step
    batches = batches_64()
    m = build_mdvit(31, 64).train()
    # weight 0, and the argument omitted
    r_omit = mdvit_train_step(m, batches, optimizer=None, fuse_domains=fuse)
    g_omit = grads_of(m)
    r_zero = mdvit_train_step(m, batches, optimizer=None, fuse_domains=fuse, boundary_weight=0.0)
    g_zero = grads_of(m)
    assert set(r_zero) == set(r_omit) == {"loss", "aux_loss", "kt_loss"}
    assert set(g_zero) == set(g_omit) and all(torch.equal(g_zero[n], g_omit[n]) for n in g_omit), [n for n in g_omit if not torch.equal(g_zero[n], g_omit[n])][:5]
    assert all(torch.equal(r_zero[k], r_omit[k]) for k in r_omit)
    # weight w: the bound from the two forms of the torch-ops step, then the step against it
    g_mean = composed_mdvit_step(m, batches, W_B, fuse, "mean")
    g_sum = composed_mdvit_step(m, batches, W_B, fuse, "sum")
    dev_forms = worst_rel_l2(g_sum, g_mean)
    bound = max(FLOOR, 10.0 * dev_forms[0])
    outs = []
    h = hook_outputs(m, outs)
    res = mdvit_train_step(m, batches, optimizer=None, fuse_domains=fuse, boundary_weight=W_B)
    h.remove()
    g_step = grads_of(m)
    worst = worst_rel_l2(g_step, g_mean)
    moved = worst_rel_l2(g_step, g_zero)
    print(f"fuse={fuse}: torch-ops forms differ by {dev_forms[0]:.3e} ({dev_forms[1]}); bound {bound:.3e}; step vs torch-ops step {worst[0]:.3e} ({worst[1]}); "
          f"the term moves the gradients by {moved[0]:.3e} ({moved[1]})")
    assert moved[0] > 100 * bound          # the term is there: a step that ignored the weight would pass the comparison below only if the term were nothing
    assert set(res) == {"loss", "aux_loss", "kt_loss", "boundary_loss"} and res["boundary_loss"].dim() == 0 and not res["boundary_loss"].requires_grad
    for k in ("loss", "aux_loss", "kt_loss"):          # the region losses are those of weight 0
        assert torch.equal(res[k], r_zero[k]), k
    if fuse > 1:
        labels, groups = [torch.cat([b[1] for b in batches])], [4]
    else:
        labels, groups = [b[1] for b in batches], [1] * 4
    assert len(outs) == len(labels)
    check_boundary_value(res, outs, labels, groups)
    assert worst[0] <= bound, worst


def test_base_step_weight_zero_and_weight_w():
    import mdvit_amd
    from mdvit_amd import ops
    from mdvit_amd.losses import seg_loss
    from mdvit_amd.train import base_train_step
    from oracle.params import make_params
    batches = batches_64()
    m = mdvit_amd.BASE(drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d, adapt_method=False)
    load_params(m, make_params(33, model="BASE", adapt_method=False))
    m = m.to(dev()).train()
    r_omit = base_train_step(m, batches, optimizer=None)
    g_omit = grads_of(m)
    r_zero = base_train_step(m, batches, optimizer=None, boundary_weight=0.0)
    g_zero = grads_of(m)
    assert set(r_zero) == set(r_omit) == {"loss"} and torch.equal(r_zero["loss"], r_omit["loss"])
    assert set(g_zero) == set(g_omit) and all(torch.equal(g_zero[n], g_omit[n]) for n in g_omit), [n for n in g_omit if not torch.equal(g_zero[n], g_omit[n])][:5]

    def composed(form):
        ops.refresh_transposes()
        m.zero_grad(set_to_none=True)
        for img, lab, sid in batches:
            out = m(img)
            phi = ops.signed_distance(lab).reshape(out.shape)
            (seg_loss(out, lab) + W_B * group_reduce(torch.sigmoid(out) * phi, 1, form)).backward()
        return grads_of(m)

    g_mean, g_sum = composed("mean"), composed("sum")
    dev_forms = worst_rel_l2(g_sum, g_mean)
    bound = max(FLOOR, 10.0 * dev_forms[0])
    outs = []
    h = hook_outputs(m, outs)
    res = base_train_step(m, batches, optimizer=None, boundary_weight=W_B)
    h.remove()
    g_step = grads_of(m)
    worst, moved = worst_rel_l2(g_step, g_mean), worst_rel_l2(g_step, g_zero)
    print(f"BASE: torch-ops forms differ by {dev_forms[0]:.3e} ({dev_forms[1]}); bound {bound:.3e}; step vs torch-ops step {worst[0]:.3e} ({worst[1]}); "
          f"the term moves the gradients by {moved[0]:.3e} ({moved[1]})")
    assert moved[0] > 100 * bound
    assert set(res) == {"loss", "boundary_loss"} and torch.equal(res["loss"], r_zero["loss"])
    check_boundary_value(res, outs, [b[1] for b in batches], [1] * 4)
    assert worst[0] <= bound, worst


def test_aux_sweep_audit_verdict_is_the_same_with_the_weight():
    """the bench step's shape of the step (fused forward, merged sweeps, gradient sinks: the aux sweep on its own stream when its graph is ours): the audit
    finds nothing with weight 0 and nothing with weight w -- the boundary node hangs off a second alias of ops.fork(out, 2) and is not reachable from the aux
    loss -- and the merged step's gradients with the weight equal the plain two-sweep step's within test_merged_sweeps_equal_reference_two_sweeps' bounds"""
    from mdvit_amd import ops
    from mdvit_amd.parallel import GradAccumulator
    from mdvit_amd.train import mdvit_train_step
    batches = batches_64()
    m = build_mdvit(31, 64).train()
    mdvit_train_step(m, batches, optimizer=None, fuse_domains=4, boundary_weight=W_B)
    g_plain = grads_of(m)
    verdicts = []
    for w in (0.0, W_B):
        acc = GradAccumulator(m.parameters(), late=[p for n, p in m.named_parameters() if "domain_layer" in n])
        acc.attach_sinks()
        try:
            if hasattr(m, "_aux_sweep_graph_cache"):
                del m._aux_sweep_graph_cache          # audit again: the verdict is cached per model and graph signature
                del m._aux_sweep_graph_findings
            mdvit_train_step(m, batches, optimizer=None, accumulator=acc, merged_sweeps=True, fuse_domains=4, boundary_weight=w)
            ops.join_side_stream()
            verdicts.append((m._aux_sweep_graph_ok, m._aux_sweep_graph_findings))
            g_merged = grads_of(m)
        finally:
            ops.set_grad_sinks(None)
    assert verdicts[0] == verdicts[1] == (True, ([], [])), verdicts
    for n in g_plain:
        check_grad(g_merged[n], g_plain[n], name=n, l2_tol=2e-4, max_tol=2e-3)
