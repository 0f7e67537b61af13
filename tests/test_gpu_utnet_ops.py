"""GPU: the two small operators UTNet adds to the set.
  mdvit_maxpool2x2_fwd / _bwd (ops.maxpool2x2, csrc/pool.hip) against torch's max_pool2d in fp64, with deliberate ties (the gradient goes to the first maximum in
  row-major order, as ATen) and channel counts that are no multiple of four;
  mdvit_resize_ac_fwd / _bwd where UTNet runs them and nothing did before -- DOWNsizing to 8 x 8 (64 -> 8, 16 -> 8, a non-square 16 x 24 -> 8 x 8) -- against
  F.interpolate(align_corners=True) in fp64, plus the adjoint identity <resize(x), g> = <x, resize_bwd(g)> to fp32 round-off."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import dev

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize("shape", [(2, 8, 12, 5), (1, 32, 32, 32), (3, 6, 4, 7), (1, 64, 48, 64)])
@pytest.mark.parametrize("ties", [False, True])
def test_maxpool2x2_matches_torch_including_ties(shape, ties):
    from mdvit_amd import ops
    B, H, W, Cn = shape
    g = torch.Generator().manual_seed(H * 31 + W * 7 + Cn)
    x = torch.randn(B, H, W, Cn, generator=g, dtype=torch.float64).float().double()          # fp32-exact values: the fp32 maximum is the fp64 one
    if ties:          # a handful of levels: most windows hold their maximum more than once; some windows constant
        x = torch.randint(0, 3, (B, H, W, Cn), generator=g).double()
        x[:, :2, :2] = 1.0
    gy = torch.randn(B, H // 2, W // 2, Cn, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.max_pool2d(xr, 2)
    want.backward(gy.permute(0, 3, 1, 2))
    xa = x.float().to(dev()).requires_grad_(True)
    y = ops.maxpool2x2(xa)
    y.backward(gy.float().to(dev()))
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu().double(), want.detach().permute(0, 2, 3, 1))          # a maximum of fp32-exact values is exact
    assert torch.equal(xa.grad.cpu(), xr.grad.permute(0, 2, 3, 1).float())                    # one gradient per window, at ATen's position


RESIZES = [(2, 64, 64, 32), (1, 16, 16, 64), (2, 16, 24, 20)]


@pytest.mark.parametrize("shape", RESIZES)
def test_resize_ac_down_to_8x8_matches_interpolate_and_its_backward_is_the_adjoint(shape):
    from mdvit_amd import ops
    B, H, W, Cn = shape
    g = torch.Generator().manual_seed(H + 3 * W + Cn)
    x = torch.randn(B, H, W, Cn, generator=g, dtype=torch.float64)
    gy = torch.randn(B, 8, 8, Cn, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.interpolate(xr, size=8, mode="bilinear", align_corners=True)
    want.backward(gy.permute(0, 3, 1, 2))
    xa = x.float().to(dev()).requires_grad_(True)
    y = ops.resize_ac_to(xa, 8, 8)
    y.backward(gy.float().to(dev()))
    torch.cuda.synchronize()
    e_y, e_dx = _rel(y.detach(), want.detach().permute(0, 2, 3, 1)), _rel(xa.grad, xr.grad.permute(0, 2, 3, 1))
    # two fp32 lerps of fp32 inputs with fp32 weights: a few ulp (6e-8 each) of the largest value
    print(f"{shape}: resize {e_y:.2e}, backward {e_dx:.2e}")
    assert e_y <= 2e-6 and e_dx <= 2e-6
    if H == 64:          # 63 / 7 = 9: every output pixel IS one input pixel; the other 63 of 64 feed nothing and their gradient is exactly zero, as the reference's
        zero = xr.grad.permute(0, 2, 3, 1) == 0
        assert float(zero.double().mean()) > 0.9 and bool((xa.grad.cpu()[zero] == 0).all())
    lhs = float((y.detach().double() * gy.to(dev())).sum())
    rhs = float((xa.detach().double() * xa.grad.double()).sum())
    scale = float((y.detach().double() * gy.to(dev())).abs().sum())
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)
