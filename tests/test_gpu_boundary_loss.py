"""ops.boundary_loss (mdvit_boundary_loss_fwd / _bwd, csrc/signed_distance.hip) against the float64 restatement of tests/test_signed_distance_host.py.

Bound (tests/test_gpu_adapter.py, docs/history.md): per tensor, the relative L2 error against float64 is at most 10 x the error of the same formula evaluated by
torch in fp32 on the CPU on the same inputs, the measured ratio printed.  The kernels differ from that baseline in expf and in the fp64 accumulators of the
sum; the backward takes its roundings in autograd's order, (((g * (1 / N)) * phi) * (1 - s)) * s.  Measured on an MI355X: loss 0.55 - 1.01 x, gradient
1.00 - 1.06 x the baseline's error."""
import numpy as np
import pytest
import torch

from test_signed_distance_host import grad_ref, loss_ref

pytestmark = pytest.mark.gpu

SHAPES = [((2, 1, 33, 45), 1), ((4, 1, 64, 65), 1), ((4, 1, 64, 65), 2), ((4, 1, 64, 65), 4), ((3, 40, 130), 1)]
IDS = [f"{'x'.join(map(str, s))}-G{g}" for s, g in SHAPES]


def dev():
    return torch.device("cuda:0")


def make_case(shape, seed=0, degenerate=False):
    """logits ~ N(0, 3^2) with some +-30 (saturated sigmoids), labels of a few random discs per image; phi from the device map"""
    from mdvit_amd import ops
    g = torch.Generator().manual_seed(1000 + seed)
    x = 3.0 * torch.randn(shape, generator=g)
    pick = torch.rand(shape, generator=g)
    x = torch.where(pick < 0.02, torch.full_like(x, 30.0), torch.where(pick > 0.98, torch.full_like(x, -30.0), x))
    B, H, W = shape[0], shape[-2], shape[-1]
    yy, xx = torch.arange(H).view(1, H, 1).float(), torch.arange(W).view(1, 1, W).float()
    lab = torch.zeros((B, H, W), dtype=torch.bool)
    for _ in range(3):
        c = torch.rand((B, 3), generator=g)
        lab |= ((yy - c[:, 0].view(B, 1, 1) * H) ** 2 + (xx - c[:, 1].view(B, 1, 1) * W) ** 2) <= ((0.08 + 0.2 * c[:, 2].view(B, 1, 1)) * min(H, W)) ** 2
    if degenerate:
        lab[0], lab[-1] = False, True          # one empty and one full label
    lab = lab.float().view(shape)
    phi = ops.signed_distance(lab.to(dev()))
    return x, lab, phi


def torch_formula(x, phi, groups, upstream, dtype):
    """(loss, dlogits) of sum_g mean_g(sigmoid(x) phi) by torch ops on the CPU in `dtype`"""
    xs = x.to(dtype).requires_grad_(True)
    p = phi.to(dtype)
    Bd = x.shape[0] // groups
    loss = sum((torch.sigmoid(xs[g * Bd:(g + 1) * Bd]) * p[g * Bd:(g + 1) * Bd]).mean() for g in range(groups))
    (gx,) = torch.autograd.grad(loss, xs, grad_outputs=torch.tensor(upstream, dtype=dtype))
    return loss.detach(), gx


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(float(np.linalg.norm(b.ravel())), 1e-300))


def run_op(x, phi, groups, upstream):
    from mdvit_amd import ops
    xs = x.to(dev()).requires_grad_(True)
    loss = ops.boundary_loss(xs, phi, groups)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (gx,) = torch.autograd.grad(loss, xs, grad_outputs=torch.tensor(upstream, device=dev()))
    torch.cuda.synchronize()
    return loss.detach().cpu(), gx.cpu()


@pytest.mark.parametrize("shape,groups", SHAPES, ids=IDS)
def test_loss_and_gradient_within_10x_the_fp32_cpu_error(shape, groups):
    upstream = -2.5          # a non-unit upstream gradient, read from device memory by the backward
    x, lab, phi = make_case(shape, seed=groups)
    phi_h = phi.cpu()
    assert float(phi_h.min()) < 0 < float(phi_h.max())
    want = (loss_ref(x.numpy(), phi_h.numpy(), groups), grad_ref(x.numpy(), phi_h.numpy(), upstream, groups))
    base = torch_formula(x, phi_h, groups, upstream, torch.float32)
    check = torch_formula(x, phi_h, groups, upstream, torch.float64)          # the restatement agrees with torch's own float64 evaluation
    assert abs(float(check[0]) - want[0]) <= 1e-12 * abs(want[0]) and rel_l2(check[1].numpy(), want[1]) <= 1e-9
    got = run_op(x, phi, groups, upstream)
    assert got[1].shape == x.shape
    bad = []
    for name, w, b32, o in zip(("loss", "dlogits"), want, base, got):
        e_base, e_op = rel_l2(b32.numpy(), w), rel_l2(o.numpy(), w)
        print(f"{tuple(shape)} G={groups} {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  ratio {e_op / max(e_base, 1e-300):.3f}  bound {10 * e_base:.3e}")
        if not (np.isfinite(e_op) and e_op <= 10.0 * e_base):
            bad.append((name, e_op, e_base))
    assert not bad, bad
    again = run_op(x, phi, groups, upstream)          # no atomics, fixed-order sums: bit-identical run to run
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_backward_through_a_weighted_sum_and_no_gradient_for_phi():
    from mdvit_amd import ops
    x, lab, phi = make_case((4, 1, 64, 65), seed=7)
    xs = x.to(dev()).requires_grad_(True)
    phi_g = phi.clone().requires_grad_(True)
    (0.3 * ops.boundary_loss(xs, phi_g, 2)).backward()
    torch.cuda.synchronize()
    assert phi_g.grad is None
    want = grad_ref(x.numpy(), phi.cpu().numpy(), 0.3, 2)
    assert rel_l2(xs.grad.cpu().numpy(), want) <= 1e-5          # element-wise fp32, a handful of roundings of 6e-8 each: two orders of margin
    with torch.no_grad():          # no graph, no saved tensors
        assert not ops.boundary_loss(xs, phi, 2).requires_grad


def test_empty_and_full_labels_contribute_nothing():
    """an image whose label is empty or full has phi = 0 everywhere: exactly zero rows of the gradient, and the loss is the other images' sum"""
    import mdvit_amd
    x, lab, phi = make_case((4, 1, 33, 45), seed=3, degenerate=True)
    assert not phi[0].any() and not phi[3].any() and phi[1].any() and phi[2].any()
    loss, gx = run_op(x, phi, 1, 1.0)
    assert not gx[0].any() and not gx[3].any() and gx[1].any() and gx[2].any()
    want = loss_ref(x.numpy()[1:3], phi.cpu().numpy()[1:3]) * 0.5          # two of the four images carry the whole sum
    assert abs(float(loss) - want) <= 1e-5 * float(phi.abs().mean())          # |s phi| <= |phi|: fp32 round-off of the terms, with two orders of margin
    via_losses = mdvit_amd.boundary_loss(x.to(dev()), lab.to(dev()))          # losses.boundary_loss computes the map itself
    assert torch.equal(via_losses.cpu(), loss)


def test_device_refusals():
    from mdvit_amd import ops
    x = torch.zeros((4, 1, 8, 9), device=dev())
    with pytest.raises(ValueError, match="disagree"):
        ops.boundary_loss(x, torch.zeros((4, 1, 9, 8), device=dev()))
    with pytest.raises(ValueError, match="equal domain batches"):
        ops.boundary_loss(x, torch.zeros_like(x), groups=3)
    with pytest.raises(ValueError, match="fp32"):
        ops.boundary_loss(x.double(), torch.zeros_like(x))
    nc = torch.zeros((4, 1, 9, 8), device=dev()).transpose(2, 3)          # non-contiguous inputs are made contiguous, as the neighbouring loss ops do
    assert float(ops.boundary_loss(nc, nc)) == 0.0
