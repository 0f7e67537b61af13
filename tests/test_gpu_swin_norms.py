"""GPU: LayerNorm with SwinUnet's patch rearrangements in its addressing (csrc/swin_norm.hip; ops.patch_merge_ln / ops.patch_expand_ln) against an fp64 torch
restatement (cat / rearrange + layer_norm: Models/Transformer/SwinUnet.py:311-320, :343-350, :366-373).

  merge  (B=2, 4x6, C=96)           H != W, two samples, 4C = 384
         (B=1, 4x4, C=384)          4C = 1536: beyond mdvit_layernorm_fwd's 1024
  expand (B=2, 2x3, p=2, c=48)      a row shorter than a wavefront, H != W
         (B=1, 2x2, p=2, c=384)     the widest slice
         (B=1, 2x3, p=4, c=96)      the head's 4 x 4 expansion

Bound (tests/test_gpu_adapter.py, docs/history.md): max|got - fp64| / max|fp64| per tensor at most 10 x the same statistic of torch's fp32 evaluation of the
restatement on the CPU, which itself must stay below 1e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_model import dev

pytestmark = pytest.mark.gpu

CASES = [("merge", 2, 4, 6, 2, 96), ("merge", 1, 4, 4, 2, 384), ("expand", 2, 2, 3, 2, 48), ("expand", 1, 2, 2, 2, 384), ("expand", 1, 2, 3, 4, 96)]
NAMES = ("y", "dx", "dgamma", "dbeta")
_cases = {}


def restated(x, gamma, beta, kind, p):
    if kind == "merge":
        z = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
    else:          # 'b h w (p1 p2 c) -> b (h p1) (w p2) c'
        B, H, W, Cx = x.shape
        c = Cx // (p * p)
        z = x.view(B, H, W, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H * p, W * p, c)
    return torch.nn.functional.layer_norm(z, (z.shape[-1],), gamma, beta, 1e-5)


def make_case(case):
    if case in _cases:
        return _cases[case]
    kind, B, H, W, p, c = case
    g = torch.Generator().manual_seed(11 * H + 3 * W + c + p + (0 if kind == "merge" else 1))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Cx, L = (c, 4 * c) if kind == "merge" else (p * p * c, c)
    x = rn(B, H, W, Cx) + 0.5 * rn(1, 1, 1, Cx)
    gamma, beta = 1.0 + 0.3 * rn(L), 0.3 * rn(L)
    gy = rn(*((B, H // 2, W // 2, L) if kind == "merge" else (B, H * p, W * p, L)))

    def run(dtype):
        ts = [t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta)]
        y = restated(*ts, kind, p)
        y.backward(gy.to(dtype))
        return [y.detach().double()] + [t.grad.double() for t in ts]

    _cases[case] = ((x, gamma, beta, gy), run(torch.float64), run(torch.float32))
    return _cases[case]


def run_op(inputs, case):
    from mdvit_amd import ops
    kind, B, H, W, p, c = case
    x, gamma, beta, gy = inputs
    ts = [t.float().to(dev()).requires_grad_(True) for t in (x, gamma, beta)]
    y = ops.patch_merge_ln(*ts) if kind == "merge" else ops.patch_expand_ln(*ts, p)
    y.backward(gy.float().to(dev()))
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in ts]


def stat(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize("case", CASES)
def test_patch_ln_matches_fp64_restatement_within_10x_the_fp32_cpu_error(case):
    inputs, want, base = make_case(case)
    got = run_op(inputs, case)
    bad = []
    for name, w, b32, o in zip(NAMES, want, base, got):
        assert o is not None and tuple(o.shape) == tuple(w.shape), name
        e_base, e_op = stat(b32, w), stat(o, w)
        print(f"{case} {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  bound {10 * e_base:.3e}")
        assert e_base < 1e-4, (name, e_base)
        if not (np.isfinite(e_op) and e_op <= 10.0 * e_base):
            bad.append((name, e_op, e_base))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_two_runs_are_bit_identical(case):
    inputs = make_case(case)[0]
    a, b = run_op(inputs, case), run_op(inputs, case)
    for name, u, v in zip(NAMES, a, b):
        assert torch.equal(u, v), name


@pytest.mark.parametrize("case", [CASES[0], CASES[4]])
def test_every_output_element_is_written_and_dgrad_only_matches(case):
    """NaN-filled caller-owned buffers at the C ABI come back finite everywhere; the data-gradient-only call (dgamma = dbeta = NULL) gives the same dx"""
    from mdvit_amd import _lib
    lib = _lib.load()
    kind, B, H, W, p, c = case
    x, gamma, beta, gy = (t.float().to(dev()).contiguous() for t in make_case(case)[0])
    L = gamma.numel()
    rows = gy.numel() // L
    nan = lambda *s: torch.full(s, float("nan"), device=dev(), dtype=torch.float32)
    y, mean, rstd, dx, dx2, dg, db = nan(*gy.shape), nan(rows), nan(rows), nan(*x.shape), nan(*x.shape), nan(L), nan(L)
    wsb = lib.mdvit_partials_ws_bytes(2 * L)
    ws = nan(wsb // 4)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geo = (B, H, W, c) if kind == "merge" else (B, H, W, p, c)
    fwd, bwd = getattr(lib, f"mdvit_patch_{kind}_ln_fwd"), getattr(lib, f"mdvit_patch_{kind}_ln_bwd")
    _lib.check(fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), *geo, 1e-5, st), "fwd")
    _lib.check(bwd(ptr(gy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), ptr(ws), wsb, 0, *geo, st), "bwd")
    _lib.check(bwd(ptr(gy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx2), None, None, None, 0, 0, *geo, st), "bwd dgrad")
    torch.cuda.synchronize()
    for name, t in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert bool(torch.isfinite(t).all()), name
    assert torch.equal(dx, dx2)
    # shapes the kernels are not built for are refused by name before any launch
    if kind == "merge":
        assert fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), B, H + 1, W, c, 1e-5, st) == 1
        assert fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), B, H, W, 388, 1e-5, st) == 1
    else:
        assert fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), B, H, W, 3, c, 1e-5, st) == 1
