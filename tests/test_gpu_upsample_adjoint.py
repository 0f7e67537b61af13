"""The bilinear adjoints as ONE kernel (csrc/conv.hip: upsample_multi_bwd_fused_kernel for the peer heads' upsample_sum, upsample_bwd_fused_kernel for the C = 1
logit resizes) against the two passes they replace (mdvit_upsample_bwd_config(0): same taps, same order, same fmaf -- bit for bit) and against
F.interpolate(bilinear, align_corners=False) through autograd in fp64 on the CPU, at the tolerance of test_gpu_kernels.test_upsample."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import TOL, check, dev, rnd

pytestmark = pytest.mark.gpu

# (B, Ho, Wo, C, [(Hi, Wi), ...]).  The band is 16 dy rows, the channel slice 32:
CASES = {
    "two_bands_two_slices_two_images": (2, 32, 32, 64, [(16, 16), (8, 8), (4, 4)]),
    "middle_band_halos_both_sides": (2, 48, 32, 32, [(24, 16), (12, 8), (6, 4)]),
    "peer_head_row_one_band_both_borders": (1, 16, 128, 512, [(8, 64), (4, 32), (2, 16)]),          # Hi = 2 at x8: every input row is a clamped border row
    "two_sources_three_slices": (1, 32, 64, 96, [(16, 32), (8, 16)]),
    "x8_alone": (1, 16, 16, 32, [(2, 2)]),
    "x2_alone": (1, 16, 16, 32, [(8, 8)]),
    "h_and_w_factors_differ": (1, 32, 32, 32, [(8, 16), (16, 4)]),          # x4 down, x2 across / x2 down, x8 across: the one kernel takes these too
}
DECLINED = {
    "factor_3": (1, 12, 12, 32, [(4, 4)]),
    "c_8": (2, 16, 16, 8, [(8, 8), (4, 4)]),
    "odd_sizes": (1, 11, 13, 32, [(5, 7)]),
}


class _two_pass:
    """the two-pass kernels inside, the default (one kernel) back on the way out"""

    def __enter__(self):
        from mdvit_amd._lib import call
        call("mdvit_upsample_bwd_config", 0)

    def __exit__(self, *exc):
        from mdvit_amd._lib import call
        call("mdvit_upsample_bwd_config", 1)


def _inputs(case):
    B, Ho, Wo, Cn, dims = case
    xs = [rnd(B, h, w, Cn, seed=500 + i) for i, (h, w) in enumerate(dims)]
    return xs, rnd(B, Ho, Wo, Cn, seed=510)


def _sum_bwd(case):
    from mdvit_amd import ops
    B, Ho, Wo, Cn, dims = case
    xs, g = _inputs(case)
    ins = [x.to(dev()).requires_grad_(True) for x in xs]
    ops.upsample_sum(None, ins, Ho, Wo).backward(g.to(dev()))
    return [t.grad for t in ins]


@functools.lru_cache(maxsize=None)
def _results(name):
    """(dx_i of the one kernel, dx_i of the two passes, dx_i in fp64 on the CPU) of a case: computed once, shared, never written to"""
    case = {**CASES, **DECLINED}[name]
    B, Ho, Wo, Cn, dims = case
    one = _sum_bwd(case)
    with _two_pass():
        two = _sum_bwd(case)
    xs, g = _inputs(case)
    ins = [x.double().requires_grad_(True) for x in xs]
    y = sum(F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for x in ins)
    y.backward(g.double())
    return one, two, [t.grad for t in ins]


def _direct(case, fused):
    """mdvit_upsample_multi_bwd as ops._UpsampleSum.backward calls it, on a workspace full of NaN -> (dx_i, the workspace afterwards)"""
    from mdvit_amd import _lib, ops
    from mdvit_amd._lib import call
    B, Ho, Wo, Cn, dims = case
    g = _inputs(case)[1].to(dev())
    n = len(dims)
    dxs = [torch.empty(B, h, w, Cn, device=dev()) for h, w in dims]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in dxs])
    Hi = (C.c_int32 * n)(*[h for h, _ in dims])
    Wi = (C.c_int32 * n)(*[w for _, w in dims])
    wsb = _lib.load().mdvit_upsample_multi_bwd_ws_bytes(Wi, n, B, Ho, Cn)
    ws = torch.full((wsb // 4,), float("nan"), device=dev())
    call("mdvit_upsample_bwd_config", int(fused))
    try:
        call("mdvit_upsample_multi_bwd", ops._p(g), ptrs, Hi, Wi, n, ops._p(ws), wsb, B, Ho, Wo, Cn, ops._stream())
        torch.cuda.synchronize()
    finally:
        call("mdvit_upsample_bwd_config", 1)
    return dxs, ws


@pytest.mark.parametrize("name", list(CASES))
def test_one_kernel_equals_the_two_passes_bit_for_bit(name):
    one, two, _ = _results(name)
    for i, (a, b) in enumerate(zip(one, two)):
        assert a.shape == b.shape and torch.equal(a, b), f"dx{i}: {int((a != b).sum())} of {a.numel()} differ, max |diff| {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_one_kernel_against_fp64(name):
    one, two, ref = _results(name)
    for i, (a, b, r) in enumerate(zip(one, two, ref)):
        check(a, r, tol=TOL, name=f"dx{i} one kernel vs fp64")
        check(b, r, tol=TOL, name=f"dx{i} two passes vs fp64")


@pytest.mark.parametrize("name", list(CASES))
def test_one_kernel_leaves_the_workspace_unread_and_unwritten(name):
    dxs, ws = _direct(CASES[name], fused=1)
    assert bool(torch.isnan(ws).all()), "the one-kernel path wrote to the workspace"
    for i, (a, b) in enumerate(zip(dxs, _results(name)[0])):
        assert bool(torch.isfinite(a).all()), f"dx{i} is not finite: the workspace was read"
        assert torch.equal(a, b), f"dx{i} differs from the autograd call's"
    # ... and the same call with the switch off is the two passes: they fill the workspace (the width folds), all of it
    dxs0, ws0 = _direct(CASES[name], fused=0)
    assert bool(torch.isfinite(ws0).all())
    for a, b in zip(dxs0, dxs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(DECLINED))
def test_declined_shapes_keep_the_two_passes_and_are_right(name):
    dxs, ws = _direct(DECLINED[name], fused=1)
    assert bool(torch.isfinite(ws).all()), "a shape the one kernel declines must take the two passes (which fill the workspace)"
    one, two, ref = _results(name)
    for i, (d, a, b, r) in enumerate(zip(dxs, one, two, ref)):
        assert torch.equal(d, a) and torch.equal(a, b), f"dx{i}: the switch must not matter for a declined shape"
        check(a, r, tol=TOL, name=f"dx{i} vs fp64")


@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo", [(2, 8, 8, 32, 32), (1, 128, 128, 512, 512)])
def test_logit_resize_backward_in_one_launch(B, Hi, Wi, Ho, Wo):
    from mdvit_amd import ops
    x, g = rnd(B, Hi, Wi, 1, seed=520), rnd(B, Ho, Wo, 1, seed=521)

    def bwd():
        xi = x.to(dev()).requires_grad_(True)
        ops.upsample_bilinear(xi, Ho, Wo).backward(g.to(dev()))
        return xi.grad

    one = bwd()
    with _two_pass():
        two = bwd()
    assert torch.equal(one, two), f"{int((one != two).sum())} of {one.numel()} differ, max |diff| {float((one - two).abs().max()):.3e}"
    xr = x.double().requires_grad_(True)
    F.interpolate(xr.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).backward(g.double())
    check(one, xr.grad, tol=TOL, name="dx vs fp64")


def test_a_single_quad_takes_the_one_launch_too_and_wider_c_does_not_change():
    """C = 4 (one channel quad: the two passes run their float4 form) is inside the one-launch rule, C = 8 outside: both equal the two passes and fp64"""
    from mdvit_amd.ops import _Upsample
    for Cn in (4, 8):
        x, g = rnd(2, 4, 8, Cn, seed=530), rnd(2, 16, 16, Cn, seed=531)

        def bwd():
            xi = x.to(dev()).requires_grad_(True)
            _Upsample.apply(xi, 16, 16, None).backward(g.to(dev()))
            return xi.grad

        one = bwd()
        with _two_pass():
            two = bwd()
        assert torch.equal(one, two)
        xr = x.double().requires_grad_(True)
        F.interpolate(xr.permute(0, 3, 1, 2), size=(16, 16), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).backward(g.double())
        check(one, xr.grad, tol=TOL, name=f"C={Cn} dx vs fp64")
