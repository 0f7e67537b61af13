"""Per-kernel parity: each HIP entry point (through the C ABI, via mdvit_amd.ops) against a plain
torch CPU reference of the same op on the same seeded inputs.  fp32 tolerance: 1e-4 relative to the
tensor's max magnitude unless stated (north_star bar: 1e-3 rel)."""
import math
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def check(a, b, tol=TOL, name=""):
    assert a.shape == b.shape, f"{name}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = relerr(a, b)
    assert math.isfinite(e) and e <= tol, f"{name}: rel-to-max error {e:.3e} > {tol}"


def grads_of(fn, inputs, gout):
    ins = [t.clone().requires_grad_(True) for t in inputs]
    out = fn(*ins)
    out.backward(gout.to(out.device))
    return out, [t.grad for t in ins]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(70, 192, 64), (1000, 64, 512), (300, 320, 128), (257, 1024, 320), (8, 64, 64), (4096, 2048, 512), (33, 36, 28)])
def test_linear_fwd_bwd(M, N, K, gemm_precision):
    from mdvit_amd import ops
    x, W, b, g = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref, gr = grads_of(lambda x, W, b: F.linear(x.double(), W.double(), b.double()), [x, W, b], g.double())
    out, go = grads_of(lambda x, W, b: ops.linear(x, W, b), [x.to(dev()), W.to(dev()), b.to(dev())], g)
    check(out, ref, name="y")
    for n, a, r in zip(("dx", "dW", "db"), go, gr):
        check(a, r, name=n)


@pytest.mark.parametrize("M,N,K", [(1000, 192, 64), (333, 512, 320), (4096, 64, 512), (77, 1280, 320)])
def test_linear_and_mlp_bf16x3_vs_fp64(M, N, K):
    """bf16x3 GEMMs (hi/lo bf16 split, three bf16 MFMAs, fp32 accumulate): forward, dgrad through the transposed-weight
    cache, and the fused GELU / GELU' epilogues, against fp64 -- error class 1e-5, checked at 1e-4 of the tensor max"""
    from mdvit_amd import ops
    x, W, b, g = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref, gr = grads_of(lambda x, W, b: F.linear(x.double(), W.double(), b.double()), [x, W, b], g.double())
    W2, b2, res = rnd(K, N, seed=5, scale=N ** -0.5), rnd(K, seed=6), rnd(M, K, seed=7)
    g2 = rnd(M, K, seed=8)
    mref, mgr = grads_of(lambda x, W, b, W2, b2: res.double() + F.linear(F.gelu(F.linear(x.double(), W.double(), b.double())), W2.double(), b2.double()),
                         [x, W, b, W2, b2], g2.double())
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16x3")
    try:
        assert ops.gemm_precision() == "bf16x3"
        out, go = grads_of(lambda x, W, b: ops.linear(x, W, b), [x.to(dev()), W.to(dev()), b.to(dev())], g)
        mout, mgo = grads_of(lambda x, W, b, W2, b2: ops.mlp_residual(x, res.to(dev()), W, b, W2, b2),
                             [x.to(dev()), W.to(dev()), b.to(dev()), W2.to(dev()), b2.to(dev())], g2)
        ops.kernel_events_begin()
        ops.linear(x.to(dev()), W.to(dev()), b.to(dev()))
        names = list(ops.kernel_events_end())
    finally:
        ops.set_gemm_precision(prev)
    # the bf16x3 arithmetic really ran: the plane kernel with two planes, or the split-while-staging instantiation of gemm.hip
    assert names and all(n.startswith("gemm_bp_nt_kernel") and n.split(",")[2].strip() == "2" or n.split(">")[0].endswith("true") for n in names), names
    check(out, ref, name="y")
    for n, a, r in zip(("dx", "dW", "db"), go, gr):
        check(a, r, name=n)
    check(mout, mref, name="mlp y")
    for n, a, r in zip(("dx", "dW1", "db1", "dW2", "db2"), mgo, mgr):
        check(a, r, name="mlp " + n)


def test_weight_transpose_cache_follows_updates():
    from mdvit_amd import ops
    W = torch.nn.Parameter(rnd(96, 200, seed=9).to(dev()))
    t1 = ops.wt(W)
    assert torch.equal(t1, W.detach().t().contiguous())
    assert ops.wt(W) is t1                              # cached while the parameter is unchanged
    with torch.no_grad():
        W.add_(1.0)                                     # an optimizer step bumps the version counter
    t2 = ops.wt(W)                                      # refreshed into the same buffer
    assert t2 is t1 and torch.equal(t2, W.detach().t().contiguous())
    W2 = torch.nn.Parameter(rnd(40, 72, seed=11).to(dev()))
    u1 = ops.wt(W2)
    with torch.no_grad():
        W.mul_(0.5); W2.sub_(2.0)
    ops.refresh_transposes()                            # one launch for every cached weight
    assert torch.equal(t1, W.detach().t().contiguous()) and torch.equal(u1, W2.detach().t().contiguous())
    assert ops.wt(W) is t1 and ops.wt(W2) is u1
    Wv = torch.nn.Parameter(rnd(64, 320, seed=10).to(dev()))
    assert torch.equal(ops.wt(Wv[:, 128:192]), Wv.detach()[:, 128:192].t().contiguous())   # column-slice view


def test_linear_big_token_axis_split(gemm_precision):
    """wgrad reduces over 65536 tokens -> split-K + atomics path."""
    from mdvit_amd import ops
    M, N, K = 65536, 64, 64
    x, W, g = rnd(M, K, seed=5), rnd(N, K, seed=6, scale=0.125), rnd(M, N, seed=7)
    ref, gr = grads_of(lambda x, W: F.linear(x.double(), W.double()), [x, W], g.double())
    out, go = grads_of(lambda x, W: ops.linear(x, W, None), [x.to(dev()), W.to(dev())], g)
    check(out, ref, name="y")
    check(go[0], gr[0], name="dx")
    check(go[1], gr[1], tol=2e-4, name="dW")


def test_linear_weight_slice_and_residual(gemm_precision):
    from mdvit_amd import ops
    M, N, K = 200, 128, 64
    Wfull, x, res, g = rnd(N, 320, seed=8, scale=0.1), rnd(M, K, seed=9), rnd(M, N, seed=10), rnd(M, N, seed=11)

    def ref_fn(x, Wf, res):
        return res.double() + F.linear(x.double(), Wf.double()[:, 128:192])

    def hip_fn(x, Wf, res):
        return ops.linear(x, Wf[:, 128:192], None, residual=res)

    ref, gr = grads_of(ref_fn, [x, Wfull, res], g.double())
    out, go = grads_of(hip_fn, [x.to(dev()), Wfull.to(dev()), res.to(dev())], g)
    check(out, ref, name="y")
    for n, a, r in zip(("dx", "dWfull", "dres"), go, gr):
        check(a, r, name=n)


def test_matmul_composition():
    from mdvit_amd import ops
    A, B, g = rnd(512, 2112, seed=12, scale=0.05), rnd(512, 320, seed=13, scale=0.05), rnd(512, 320, seed=14)
    ref, gr = grads_of(lambda A, B: A.double()[:, 512:1024] @ B.double(), [A, B], g.double())
    out, go = grads_of(lambda A, B: ops.matmul(A[:, 512:1024], B), [A.to(dev()), B.to(dev())], g)
    check(out, ref, name="C")
    check(go[0], gr[0], name="dA")
    check(go[1], gr[1], name="dB")


def test_linear_dropout_droppath_statistics_and_backward_mask():
    from mdvit_amd import ops
    torch.manual_seed(0)
    B_, Ntok, K, N = 8, 128, 64, 256
    M = B_ * Ntok
    x, W, b = rnd(M, K, seed=15).to(dev()), rnd(N, K, seed=16, scale=0.2).to(dev()), rnd(N, seed=17).to(dev())
    res = torch.zeros(M, N, device=dev())
    rs = torch.tensor([0, 1 / 0.9, 1 / 0.9, 0, 1 / 0.9, 1 / 0.9, 1 / 0.9, 1 / 0.9], device=dev())
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y = ops.linear(xr, Wr, b, residual=res, rowscale=rs, drop_p=0.1, rows_per_scale=Ntok)
    plain = F.linear(x, W, b)
    ratio = (y / plain).detach()
    live = rs.repeat_interleave(Ntok) > 0
    kept = (ratio[live].abs() > 1e-6)
    frac = kept.float().mean().item()
    assert abs(frac - 0.9) < 0.01, f"keep rate {frac}"
    assert (y[~live] == 0).all(), "DropPath-ed samples must be exactly zero"
    exp_scale = (1 / 0.9) * (1 / 0.9)
    assert torch.allclose(y.detach()[live][kept], plain[live][kept] * exp_scale, rtol=1e-4, atol=5e-5)      # (bf16x3 GEMM against torch's fp32 matmul: ~1e-5 of the largest element)
    # backward must use the SAME mask
    g = rnd(M, N, seed=18).to(dev())
    y.backward(g)
    mask = torch.zeros_like(y)
    mask[live] = kept.float() * exp_scale
    gm = g * mask
    check(xr.grad, gm @ W, name="dx under dropout")
    check(Wr.grad, gm.t() @ x, tol=2e-4, name="dW under dropout")
    # a second call draws a different mask
    y2 = ops.linear(x, W, b, residual=res, rowscale=rs, drop_p=0.1, rows_per_scale=Ntok)
    assert (y2 != y.detach()).any()


def test_droppath_scales_from_the_counter_hash(monkeypatch):
    """ops.droppath_scales: per-sample Bernoulli(keep) / keep scales (timm drop_path in mdvit.py:353-360) drawn by the dropout kernel's
    counter hash -- values in {0, 1 / keep}, keep rate within 4 sigma, repeatable for equal keys, different for the next key"""
    from mdvit_amd import ops
    import itertools
    keep, n = 0.9, 40002
    monkeypatch.setattr(ops, "_key_counter", itertools.count(300))
    a = ops.droppath_scales((n // 2, 2), keep, dev())
    monkeypatch.setattr(ops, "_key_counter", itertools.count(300))
    b = ops.droppath_scales((n // 2, 2), keep, dev())
    c = ops.droppath_scales((n // 2, 2), keep, dev())
    assert a.shape == (n // 2, 2) and torch.equal(a, b) and not torch.equal(a, c)
    vals = torch.unique(a).cpu().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1 / keep) < 1e-6
    rate = float((a > 0).float().mean())
    assert abs(rate - keep) < 4 * (keep * (1 - keep) / n) ** 0.5, rate


@pytest.mark.parametrize("M,C,r", [(512, 64, 8), (130, 128, 8), (64, 320, 4), (16, 512, 4)])
def test_mlp_residual(M, C, r, gemm_precision):
    from mdvit_amd import ops
    Hd = C * r
    x, res = rnd(M, C, seed=20), rnd(M, C, seed=21)
    W1, b1, W2, b2 = rnd(Hd, C, seed=22, scale=C ** -0.5), rnd(Hd, seed=23, scale=0.1), rnd(C, Hd, seed=24, scale=Hd ** -0.5), rnd(C, seed=25, scale=0.1)
    g = rnd(M, C, seed=26)

    def ref_fn(x, res, W1, b1, W2, b2):
        return res.double() + F.linear(F.gelu(F.linear(x.double(), W1.double(), b1.double())), W2.double(), b2.double())

    ref, gr = grads_of(ref_fn, [x, res, W1, b1, W2, b2], g.double())
    out, go = grads_of(lambda *a: ops.mlp_residual(*a), [t.to(dev()) for t in (x, res, W1, b1, W2, b2)], g)
    # fp32 MFMA is an fmaf chain (1e-4 of the tensor max is generous); bf16x3 carries ~2^-17 per product through two chained GEMMs
    tol = 1e-4 if gemm_precision == "fp32" else 3e-4
    check(out, ref, tol=tol, name="y")
    for n, a, r_ in zip(("dx", "dres", "dW1", "db1", "dW2", "db2"), go, gr):
        check(a, r_, tol=tol, name=n)


@pytest.mark.parametrize("M,C,r,drop", [(512, 64, 8, 0.0), (1030, 64, 8, 0.25), (130, 128, 8, 0.1), (131, 128, 8, 0.1), (70, 32, 4, 0.0), (37, 64, 8, 0.1),
                                        (200, 64, 16, 0.0), (8192, 64, 8, 0.1)])
def test_mlp_recomputed_preactivation_is_bit_identical(M, C, r, drop, monkeypatch):
    """C <= 128 (bf16x3): the forward keeps gelu(u) only and the fc2 data-gradient GEMM recomputes u = x W1^T + b1 per output
    tile -- same slab / MFMA sequence as the forward, so every output and gradient equals the stored-u path bit for bit.
    C = 64 additionally runs the fused forward (mdvit_mlp_fwd_f32) and the fused backward data path (mdvit_mlp_bwd_dgrad_f32)
    against the separate GEMMs."""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("the recomputing epilogue is the bf16x3 path's")
    Hd = C * r
    if C == 128 and M == 131:
        monkeypatch.setattr(ops, "_mlp_rc16", False)      # the recomputing GEMM epilogue itself (MDVIT_MLP_RC16=0): bit for bit
    ins = [rnd(M, C, seed=120), rnd(M, C, seed=121), rnd(Hd, C, seed=122, scale=C ** -0.5), rnd(Hd, seed=123, scale=0.1),
           rnd(C, Hd, seed=124, scale=Hd ** -0.5), rnd(C, seed=125, scale=0.1)]
    g = rnd(M, C, seed=126)
    rowscale = (torch.rand(2, generator=torch.Generator().manual_seed(5)) < 0.7).float().div(0.7).to(dev()) if drop > 0 else None
    res = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "_mlp_recompute", flag)
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(77))       # the same dropout keys in both runs
        out, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 1) // 2),
                           [t.to(dev()) for t in ins], g)
        res.append([out.detach()] + go)
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], res[1]):
        if name == "db1":       # column sums riding on the wgrad: one float atomicAdd per tile and K-split, order not fixed
            check(a, b, tol=1e-5, name=name)
            continue
        if name == "dx" and C == 64:      # the fused backward sums the hidden axis in order; the GEMM form may split K at this small M
            check(a, b, tol=1e-5, name=name)
            continue
        if C == 64 or (C == 128 and ops._mlp_rc16):   # fused MLP kernels (mlp_rc.hip; C = 64 with hidden % 256 != 0: mlp.hip) against the GEMM path: the same
            check(a, b, tol=1e-5, name=name)      # products, but other compilations of the GELU epilogue (fma contraction), 16-token tiles at C = 128 and, for the
            continue                              # recomputing weight-gradient kernel, another summation order over the tokens: equal to a few ulp, not bit for bit
        assert torch.equal(a, b), f"{name}: recomputed-u path differs from the stored-u path (max {float((a - b).abs().max()):.3e})"


@pytest.mark.parametrize("M,r,drop", [(37, 8, 0.1), (4173, 8, 0.25), (1030, 4, 0.0), (20000, 8, 0.1), (300, 16, 0.1)])
def test_mlp_rc_kernels_vs_round2_kernels_and_fp64(M, r, drop, monkeypatch):
    """csrc/mlp_rc.hip (C = 64, bf16x3): forward, data-gradient and the RECOMPUTING weight-gradient kernel against (a) the fused kernels of
    mlp.hip + the two weight-gradient GEMMs on the same dropout keys -- same products in the same k order, the activation compiled twice:
    equal to a few ulp -- and (b) without dropout, an fp64 restatement of mpvit.py:71-78.  Also the data-gradient-only sweep and the
    accumulate-into-buckets form of the weight-gradient kernel."""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mlp_rc.hip is the bf16x3 path's")
    C, Hd = 64, 64 * r
    monkeypatch.setattr(ops, "_mlp_rc_bwd", "0")       # the two-kernel backward (data gradient + recomputing weight gradient); the one-kernel form: test_mlp_rc_backward_in_one_kernel...
    ins = [rnd(M, C, seed=220), rnd(M, C, seed=221), rnd(Hd, C, seed=222, scale=C ** -0.5), rnd(Hd, seed=223, scale=0.1),
           rnd(C, Hd, seed=224, scale=Hd ** -0.5), rnd(C, seed=225, scale=0.1)]
    g = rnd(M, C, seed=226)
    rowscale = (torch.rand(3, generator=torch.Generator().manual_seed(6)) < 0.7).float().div(0.7).to(dev()) if drop > 0 else None
    res = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "_mlp_rc", flag)
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(91))
        out, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3), [t.to(dev()) for t in ins], g)
        res.append([out.detach()] + go)
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], res[1]):
        check(a, b, tol=5e-6, name=name)
    monkeypatch.setattr(ops, "_mlp_rc", True)
    if drop == 0.0:
        def ref_fn(x, res_, W1, b1, W2, b2):
            return res_.double() + F.linear(F.gelu(F.linear(x.double(), W1.double(), b1.double())), W2.double(), b2.double())
        ref, gr = grads_of(ref_fn, ins, g.double())
        for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], [ref] + gr):
            check(a, b, tol=3e-4, name=name + " vs fp64")
    # data-gradient-only sweep: dx as before, no parameter gradients
    monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(91))
    ops.set_dgrad_only(True)
    try:
        _, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3), [t.to(dev()) for t in ins], g)
    finally:
        ops.set_dgrad_only(False)
    assert torch.equal(go[0], res[0][1]) and all(t is None for t in go[2:])
    # gradient sinks: the weight-gradient kernel ADDS into persistent buffers (bucket views), autograd receives None
    params = [t.to(dev()).requires_grad_(True) for t in ins[2:]]
    sinks = {p_: torch.full_like(p_, 0.5) for p_ in params}
    ops.set_grad_sinks(sinks)
    try:
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(91))
        x_ = ins[0].to(dev()).requires_grad_(True)
        y = ops.mlp_residual(x_, ins[1].to(dev()), *params, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3)
        y.backward(g.to(dev()))
        ops.join_side_stream()
    finally:
        ops.set_grad_sinks(None)
    for name, p_, want in zip(("dW1", "db1", "dW2", "db2"), params, res[0][3:]):
        assert p_.grad is None
        check(sinks[p_] - 0.5, want, tol=2e-6, name=name + " (sink)")


@pytest.mark.parametrize("M,r,drop", [(37, 8, 0.1), (4173, 8, 0.25), (1030, 4, 0.0), (20000, 8, 0.1)])
def test_mlp_rc_backward_in_one_kernel_equals_the_two_kernels(M, r, drop, monkeypatch):
    """mdvit_mlp_rc_bwd (round 5: the C = 64 MLP backward from ONE evaluation of u, d and the activation; dx as one partial per 256-wide hidden role) against
    mdvit_mlp_rc_dgrad + mdvit_mlp_rc_wgrad on the same dropout keys: the weight / bias gradients bit for bit (the same kernel body), dx to the summation order over
    the hidden axis (16x16x32 tiles over 256-wide roles instead of 32-wide steps in sequence)."""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mlp_rc.hip is the bf16x3 path's")
    C, Hd = 64, 64 * r
    ins = [rnd(M, C, seed=320), rnd(M, C, seed=321), rnd(Hd, C, seed=322, scale=C ** -0.5), rnd(Hd, seed=323, scale=0.1),
           rnd(C, Hd, seed=324, scale=Hd ** -0.5), rnd(C, seed=325, scale=0.1)]
    g = rnd(M, C, seed=326)
    rowscale = (torch.rand(3, generator=torch.Generator().manual_seed(6)) < 0.7).float().div(0.7).to(dev()) if drop > 0 else None
    res = []
    for mode in ("0", "1"):
        monkeypatch.setattr(ops, "_mlp_rc_bwd", mode)
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(91))
        out, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3), [t.to(dev()) for t in ins], g)
        res.append([out.detach()] + go)
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], res[1]):
        if name == "dx":
            check(b, a, tol=5e-6, name=name)
        else:
            assert torch.equal(a, b), f"{name}: fused backward differs from the two kernels (max {float((a - b).abs().max()):.3e})"


@pytest.mark.parametrize("M,N,K,full,drop", [(4173, 192, 64, False, 0.0), (70000, 64, 64, True, 0.1), (1030, 384, 128, False, 0.0), (2500, 128, 128, True, 0.25),
                                             (33, 512, 64, True, 0.0), (20000, 512, 128, False, 0.0), (1, 32, 64, True, 0.1)])
def test_linear_rc_streaming_kernel_is_the_tiled_gemm_bit_for_bit(M, N, K, full, drop):
    """mdvit_linear_rc (a wave owns 32 tokens, x in MFMA operand registers, weight planes streamed through LDS): the same bf16x3 products in the
    same order as mdvit_gemm_f32 -- bias, dropout mask, DropPath row scale and residual included -- so the outputs are EQUAL; and within the
    bf16x3 bound of an fp64 product"""
    from mdvit_amd import ops
    from mdvit_amd.ops import call, _p, _stream
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mdvit_linear_rc is the bf16x3 path's")
    d = dev()
    x, W, b = rnd(M, K, seed=260).to(d), rnd(N, K, seed=261, scale=K ** -0.5).to(d), rnd(N, seed=262, scale=0.1).to(d)
    res = rnd(M, N, seed=263).to(d) if full else None
    rps = max(1, (M + 2) // 3)
    rs = ((torch.rand(3, generator=torch.Generator().manual_seed(8)) < 0.7).float() / 0.7).to(d) if full else None
    y0, y1 = torch.empty(M, N, device=d), torch.empty(M, N, device=d)
    Wp = torch.empty(2, N, K, device=d, dtype=torch.bfloat16)
    call("mdvit_split_planes_t", _p(W), K, _p(Wp), K, N * K, N, K, 0, 2, _stream())
    ops.gemm(_p(x), _p(W), _p(y0), M, N, K, lda=K, ldb=K, ldc=N, bias=_p(b), e_drop=drop, e_key=(11, 22), e_rowscale=_p(rs), e_rows_per_scale=rps,
             residual=_p(res), ldr=N)
    call("mdvit_linear_rc", _p(x), K, _p(Wp), N * K, _p(b), _p(y1), N, M, N, K, drop, 11, 22, _p(rs), rps, _p(res), N, None, _stream())
    assert torch.equal(y0, y1)
    if drop == 0.0:
        ref = x.double() @ W.double().t() + b.double()
        if full:
            ref = ref * rs.double().repeat_interleave(rps)[:M, None] + res.double()
        check(y1, ref, tol=2e-5, name="y vs fp64")
    # the data-gradient form: planes of W^T, no bias
    if not full:
        g = rnd(M, N, seed=264).to(d)
        dx0, dx1 = torch.empty(M, K, device=d), torch.empty(M, K, device=d)
        if N in (64, 128) and K % 32 == 0:
            Wtp = torch.empty(2, K, N, device=d, dtype=torch.bfloat16)
            call("mdvit_split_planes_t", _p(W), K, _p(Wtp), N, K * N, N, K, 1, 2, _stream())
            Wt = W.t().contiguous()
            ops.gemm(_p(g), _p(Wt), _p(dx0), M, K, N, lda=N, ldb=N, ldc=K, trans_b=True)
            call("mdvit_linear_rc", _p(g), N, _p(Wtp), K * N, None, _p(dx1), K, M, K, N, 0.0, 0, 0, None, 1, None, 0, None, _stream())
            assert torch.equal(dx0, dx1)


@pytest.mark.parametrize("M,K,G,drop", [(1024, 64, 1, 0.1), (5000, 64, 1, 0.0), (4096, 128, 4, 0.1), (33, 128, 1, 0.0), (70000, 64, 2, 0.1)])
def test_layernorm_prologues_equal_the_separate_layernorm_bit_for_bit(M, K, G, drop):
    """mdvit_linear_rc_ln (LN1 -> qkv) and mdvit_mlp_rc_fwd_ln (LN2 -> Mlp): the LayerNorm in the consuming kernel's prologue reproduces
    mdvit_layernorm_fwd sum for sum -- statistics, normalised rows and the consumer's output are EQUAL to LayerNorm kernel + consumer kernel"""
    from mdvit_amd import ops
    from mdvit_amd.ops import call, _p, _stream
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("the register-chained kernels are the bf16x3 path's")
    d = dev()
    Mg = (M // G) * G
    x = (rnd(Mg, K, seed=280, scale=2.0) + 0.3).to(d)
    ga, be = (1 + 0.5 * rnd(G, K, seed=281)).to(d).contiguous(), rnd(G, K, seed=282, scale=0.1).to(d).contiguous()

    def planes(W, transposed=0):
        N, Kk = W.shape
        out = torch.empty((2, Kk, N) if transposed else (2, N, Kk), device=d, dtype=torch.bfloat16)
        call("mdvit_split_planes_t", _p(W), Kk, _p(out), N if transposed else Kk, N * Kk, N, Kk, transposed, 2, _stream())
        return out
    # LN1 -> qkv
    N = 3 * K
    W, b = rnd(N, K, seed=283, scale=K ** -0.5).to(d), rnd(N, seed=284, scale=0.1).to(d)
    Wp = planes(W)
    cur0, mean0, rstd0, y0 = torch.empty(Mg, K, device=d), torch.empty(Mg, device=d), torch.empty(Mg, device=d), torch.empty(Mg, N, device=d)
    cur1, mean1, rstd1, y1 = torch.empty(Mg, K, device=d), torch.empty(Mg, device=d), torch.empty(Mg, device=d), torch.empty(Mg, N, device=d)
    call("mdvit_layernorm_fwd", _p(x), _p(ga), _p(be), _p(cur0), _p(mean0), _p(rstd0), Mg, K, G, 1e-6, _stream())
    call("mdvit_linear_rc", _p(cur0), K, _p(Wp), N * K, _p(b), _p(y0), N, Mg, N, K, 0.0, 0, 0, None, 1, None, 0, None, _stream())
    call("mdvit_linear_rc_ln", _p(x), _p(ga), _p(be), G, 1e-6, _p(mean1), _p(rstd1), _p(cur1), _p(Wp), N * K, _p(b), _p(y1), N, Mg, N, K, _stream())
    for name, a0, a1 in (("mean", mean0, mean1), ("rstd", rstd0, rstd1), ("cur", cur0, cur1), ("qkv", y0, y1)):
        assert torch.equal(a0, a1), name
    check(cur1, F.layer_norm(x.double(), (K,), None, None, 1e-6) * ga.double().repeat_interleave(Mg // G, 0) + be.double().repeat_interleave(Mg // G, 0),
          tol=5e-6, name="normalised rows vs fp64")
    # LN2 -> Mlp
    Hd = 8 * K
    W1, b1 = rnd(Hd, K, seed=285, scale=K ** -0.5).to(d), rnd(Hd, seed=286, scale=0.1).to(d)
    W2, b2 = rnd(K, Hd, seed=287, scale=Hd ** -0.5).to(d), rnd(K, seed=288, scale=0.1).to(d)
    W1p, W2p = planes(W1), planes(W2)
    rps = max(1, Mg // 4)
    rs = ((torch.rand(4 + 1, generator=torch.Generator().manual_seed(9)) < 0.8).float() / 0.8).to(d)
    h0 = torch.empty(Mg, Hd, device=d) if K == 128 else None
    h1 = torch.empty(Mg, Hd, device=d) if K == 128 else None
    z0, z1 = torch.empty(Mg, K, device=d), torch.empty(Mg, K, device=d)
    if K == 64:
        call("mdvit_mlp_rc_fwd", _p(cur0), _p(W1p), _p(b1), _p(W2p), _p(b2), _p(x), _p(rs), rps, _p(z0), Mg, K, Hd, drop, 3, 4, 5, 6, None, _stream())
    else:
        call("mdvit_mlp_rc16_fwd", _p(cur0), _p(W1p), _p(b1), _p(W2p), _p(b2), _p(x), _p(rs), rps, _p(h0), _p(z0), Mg, K, Hd, drop, 3, 4, 5, 6, None, _stream())
    cur2, mean2, rstd2 = torch.empty(Mg, K, device=d), torch.empty(Mg, device=d), torch.empty(Mg, device=d)
    call("mdvit_mlp_rc_fwd_ln", _p(x), _p(ga), _p(be), G, 1e-6, _p(mean2), _p(rstd2), _p(cur2), _p(W1p), _p(b1), _p(W2p), _p(b2), _p(rs), rps, _p(h1), _p(z1),
         Mg, K, Hd, drop, 3, 4, 5, 6, None, _stream())
    for name, a0, a1 in (("mean", mean0, mean2), ("rstd", rstd0, rstd2), ("cur", cur0, cur2), ("y", z0, z1)) + ((("h", h0, h1),) if K == 128 else ()):
        assert torch.equal(a0, a1), name


def test_linear_layers_route_to_the_streaming_kernel_with_equal_results(monkeypatch):
    """ops.linear with MDVIT_LINEAR_RC on / off: forward, data gradient, weight and bias gradients equal (the weight gradient is the same TN GEMM)"""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mdvit_linear_rc is the bf16x3 path's")
    M, K, N = 5000, 64, 64
    ins = [rnd(M, K, seed=270), rnd(N, K, seed=271, scale=K ** -0.5), rnd(N, seed=272, scale=0.1), rnd(M, N, seed=273)]
    g = rnd(M, N, seed=274)
    res = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "_lin_rc", flag)
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(97))
        out, go = grads_of(lambda x, W, b, r: ops.linear(x, W, b, residual=r, drop_p=0.1), [t.to(dev()) for t in ins], g)
        res.append([out.detach()] + go)
    for name, a, b in zip(("y", "dx", "dW", "db", "dres"), res[0], res[1]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("M,r,drop", [(37, 8, 0.1), (4173, 8, 0.25), (1030, 4, 0.0), (9000, 8, 0.1)])
def test_mlp_rc16_kernels_vs_the_gemm_path_and_fp64(M, r, drop, monkeypatch):
    """mdvit_mlp_rc16_fwd / _dgrad (C = 128, bf16x3, 16-token waves: the MLP forward and the backward data path as ONE kernel each) against the
    GEMM path they replace (fc1 + GELU GEMM, fc2 GEMM; recomputing fc2 data-gradient GEMM, fc1 data-gradient GEMM) on the same dropout keys,
    and -- without dropout -- an fp64 restatement of mpvit.py:71-78; the data-gradient-only sweep writes no du and returns the same dx"""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mlp_rc.hip is the bf16x3 path's")
    C, Hd = 128, 128 * r
    ins = [rnd(M, C, seed=240), rnd(M, C, seed=241), rnd(Hd, C, seed=242, scale=C ** -0.5), rnd(Hd, seed=243, scale=0.1),
           rnd(C, Hd, seed=244, scale=Hd ** -0.5), rnd(C, seed=245, scale=0.1)]
    g = rnd(M, C, seed=246)
    rowscale = (torch.rand(3, generator=torch.Generator().manual_seed(7)) < 0.7).float().div(0.7).to(dev()) if drop > 0 else None
    res = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "_mlp_rc16", flag)
        monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(93))
        out, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3), [t.to(dev()) for t in ins], g)
        res.append([out.detach()] + go)
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], res[1]):
        check(a, b, tol=5e-6, name=name)
    monkeypatch.setattr(ops, "_mlp_rc16", True)
    if drop == 0.0:
        def ref_fn(x, res_, W1, b1, W2, b2):
            return res_.double() + F.linear(F.gelu(F.linear(x.double(), W1.double(), b1.double())), W2.double(), b2.double())
        ref, gr = grads_of(ref_fn, ins, g.double())
        for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res[0], [ref] + gr):
            check(a, b, tol=3e-4, name=name + " vs fp64")
    monkeypatch.setattr(ops, "_key_counter", __import__("itertools").count(93))
    ops.set_dgrad_only(True)
    try:
        _, go = grads_of(lambda *a: ops.mlp_residual(*a, rowscale=rowscale, drop_p=drop, rows_per_scale=(M + 2) // 3), [t.to(dev()) for t in ins], g)
    finally:
        ops.set_dgrad_only(False)
    check(go[0], res[0][1], tol=2e-6, name="dx of the data-gradient-only sweep")      # (another instantiation: no du store, the activation compiled again)
    assert all(t is None for t in go[2:])


def test_mlp_rc_keeps_no_hidden_sized_tensor(monkeypatch):
    """the point of mlp_rc.hip: neither pass allocates anything of size [tokens, hidden] -- round 2's kernels kept h for the backward and
    wrote du for the weight-gradient GEMMs: the peak allocation of one forward + backward drops by (at least 1.8 of) those two tensors"""
    from mdvit_amd import ops
    if ops.gemm_precision() != "bf16x3":
        pytest.skip("mlp_rc.hip is the bf16x3 path's")
    M, C, Hd = 65536, 64, 512
    x = rnd(M, C, seed=230).to(dev()).requires_grad_(True); res = rnd(M, C, seed=231).to(dev())
    W1, b1 = rnd(Hd, C, seed=232, scale=C ** -0.5).to(dev()).requires_grad_(True), rnd(Hd, seed=233, scale=0.1).to(dev()).requires_grad_(True)
    W2, b2 = rnd(C, Hd, seed=234, scale=Hd ** -0.5).to(dev()).requires_grad_(True), rnd(C, seed=235, scale=0.1).to(dev()).requires_grad_(True)
    g = rnd(M, C, seed=236).to(dev())
    peaks = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "_mlp_rc", flag)
        ops.mlp_residual(x, res, W1, b1, W2, b2, drop_p=0.1).backward(g)          # warm the weight caches of this path
        for t in (x, W1, b1, W2, b2):
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.mlp_residual(x, res, W1, b1, W2, b2, drop_p=0.1).backward(g)
        torch.cuda.synchronize()
        peaks[flag] = torch.cuda.max_memory_allocated() - base
        for t in (x, W1, b1, W2, b2):
            t.grad = None
    hidden = M * Hd * 4
    assert peaks[True] < hidden, f"rc path: peak extra allocation {peaks[True] / 2**20:.0f} MiB, one [tokens, hidden] tensor is {hidden / 2**20:.0f} MiB"
    # (round 5: the one-kernel backward hands dx over as one [tokens, C] partial per 256-wide hidden role -- two partials here, 1/8 of a hidden-sized tensor each)
    assert peaks[False] - peaks[True] > 1.5 * hidden, (peaks, hidden)


@pytest.mark.parametrize("M,C", [(1000, 64), (77, 128), (300, 320), (64, 512), (5, 1024), (33, 96), (4099, 64)])
def test_layernorm(M, C):
    from mdvit_amd import ops
    x, ga, be, g = rnd(M, C, seed=30, scale=2.0) + 0.5, 1 + 0.5 * rnd(C, seed=31), rnd(C, seed=32, scale=0.1), rnd(M, C, seed=33)
    ref, gr = grads_of(lambda x, ga, be: F.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-6), [x, ga, be], g.double())
    out, go = grads_of(lambda x, ga, be: ops.layer_norm(x, ga, be, 1e-6), [x.to(dev()), ga.to(dev()), be.to(dev())], g)
    check(out, ref, name="y")
    for n, a, r in zip(("dx", "dgamma", "dbeta"), go, gr):
        check(a, r, name=n)


@pytest.mark.parametrize("M,C,groups,p,scaled", [(4096, 64, 1, 0.1, True), (1536, 128, 4, 0.1, False), (640, 320, 1, 0.0, True), (512, 512, 2, 0.25, True)])
def test_layernorm_bwd_masked_second_output_is_the_two_pass_result_bit_for_bit(M, C, groups, p, scaled):
    """mdvit_layernorm_bwd_masked: dx, dgamma, dbeta == mdvit_layernorm_bwd, and its second output == mdvit_colsum_f32's masked copy of dx
    (dropout mask of the producing Linear x DropPath row scale) -- one pass over dx instead of two"""
    from mdvit_amd import ops
    from mdvit_amd.ops import call, _p, _stream, _partials_ws
    d = dev()
    x, g, add = (rnd(M, C, seed=50, scale=2.0) + 0.3).to(d), rnd(M, C, seed=51).to(d), rnd(M, C, seed=52).to(d)
    ga = (1 + 0.5 * rnd(groups, C, seed=53)).to(d).contiguous()
    be = rnd(groups, C, seed=54, scale=0.1).to(d).contiguous()
    y, mean, rstd = torch.empty_like(x), torch.empty(M, device=d), torch.empty(M, device=d)
    call("mdvit_layernorm_fwd", _p(x), _p(ga), _p(be), _p(y), _p(mean), _p(rstd), M, C, groups, 1e-6, _stream())
    rows_per_scale = 64
    rs = (torch.rand(M // rows_per_scale, device=d) > 0.3).float() / 0.7 if scaled else None
    k0, k1 = 0x1234abcd, 0x9e3779b9
    res = []
    for fused in (False, True):
        dx, dxm = torch.empty_like(x), torch.empty_like(x)
        dg, db = torch.empty(groups, C, device=d), torch.empty(groups, C, device=d)
        wsp, wsb, _keep = _partials_ws(2 * C, d)
        if fused:
            call("mdvit_layernorm_bwd_masked", _p(g), _p(x), _p(ga), _p(mean), _p(rstd), _p(add), _p(dx), _p(dxm), _p(dg), _p(db), wsp, wsb, M, C, groups,
                 p, k0, k1, _p(rs), rows_per_scale, None, _stream())
        else:
            call("mdvit_layernorm_bwd", _p(g), _p(x), _p(ga), _p(mean), _p(rstd), _p(add), _p(dx), _p(dg), _p(db), wsp, wsb, M, C, groups, _stream())
            call("mdvit_colsum_f32", _p(dx), C, None, _p(dxm), None, 0, M, C, p, k0, k1, _p(rs), rows_per_scale, 0, None, _stream())
        res.append((dx, dxm, dg, db))
    for name, a, b in zip(("dx", "dx_masked", "dgamma", "dbeta"), res[0], res[1]):
        assert torch.equal(a, b), name
    if p > 0:
        keep = float((res[1][1] != 0).float().mean())
        assert abs(keep - (1 - p) * (float((rs != 0).float().mean()) if scaled else 1.0)) < 0.02


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("B,H,W,C,stride,bias,add", [(2, 16, 16, 64, 1, True, True), (2, 17, 13, 128, 2, False, False), (1, 8, 8, 320, 2, False, False),
                                                     (3, 5, 7, 64, 1, False, False), (2, 4, 4, 512, 1, True, True)])
def test_dwconv3x3(B, H, W, C, stride, bias, add):
    from mdvit_amd import ops
    x, w, b = rnd(B, C, H, W, seed=40), rnd(C, 1, 3, 3, seed=41, scale=0.3), (rnd(C, seed=42, scale=0.1) if bias else None)

    def ref_fn(x, w, *bb):
        y = F.conv2d(x.double(), w.double(), bb[0].double() if bb else None, stride, 1, 1, C)
        return y + x.double() if add else y

    ins = [x, w] + ([b] if bias else [])
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = rnd(B, C, Ho, Wo, seed=43)
    ref, gr = grads_of(ref_fn, ins, g.double())

    def hip_fn(x, w, *bb):
        return ops.dwconv3x3(x, w, bb[0] if bb else None, stride, add)

    hin = [nhwc(x).to(dev()), w.to(dev())] + ([b.to(dev())] if bias else [])
    out, go = grads_of(hip_fn, hin, nhwc(g))
    check(nchw(out), ref, name="y")
    check(nchw(go[0]), gr[0], name="dx")
    check(go[1], gr[1], name="dw")
    if bias:
        check(go[2], gr[2], name="dbias")


@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 64), (1, 9, 7, 128), (2, 4, 4, 320), (1, 2, 2, 512)])
def test_gconv2(B, H, W, C):
    from mdvit_amd import ops
    skip, up, w, g = rnd(B, C, H, W, seed=50), rnd(B, C, H, W, seed=51), rnd(C, 2, 3, 3, seed=52, scale=0.3), rnd(B, C, H, W, seed=53)
    ref, gr = grads_of(lambda s, u, w: F.conv2d(torch.cat((s, u), 1).double(), w.double(), None, 1, 1, 1, C), [skip, up, w], g.double())
    out, go = grads_of(lambda s, u, w: ops.gconv2_3x3(s, u, w), [nhwc(skip).to(dev()), nhwc(up).to(dev()), w.to(dev())], nhwc(g))
    check(nchw(out), ref, name="y")
    check(nchw(go[0]), gr[0], name="dskip")
    check(nchw(go[1]), gr[1], name="dup")
    check(go[2], gr[2], name="dw")


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,bias", [(2, 16, 16, 32, 64, 2, False), (1, 8, 8, 512, 512, 1, True), (2, 5, 6, 64, 128, 1, True), (1, 9, 9, 32, 64, 2, False),
                                                        (2, 32, 32, 32, 64, 2, False), (1, 64, 32, 64, 32, 2, True),        # (these two: the parity-class order of the strided data gradient)
                                                        (16, 16, 16, 512, 1024, 1, True), (12, 16, 16, 512, 512, 1, True)])  # (the bridge at 16 / 12 images: 128 x 128 tiles over K ranges, gemm.hip's conv rule)
def test_conv3x3_dense(B, H, W, Cin, Cout, stride, bias):
    from mdvit_amd import ops
    x, w = rnd(B, Cin, H, W, seed=60), rnd(Cout, Cin, 3, 3, seed=61, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=62, scale=0.1) if bias else None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = rnd(B, Cout, Ho, Wo, seed=63)
    ins = [x, w] + ([b] if bias else [])
    ref, gr = grads_of(lambda x, w, *bb: F.conv2d(x.double(), w.double(), bb[0].double() if bb else None, stride, 1), ins, g.double())
    hin = [nhwc(x).to(dev()), w.to(dev())] + ([b.to(dev())] if bias else [])
    out, go = grads_of(lambda x, w, *bb: ops.conv3x3_dense(x, w, bb[0] if bb else None, stride), hin, nhwc(g))
    check(nchw(out), ref, name="y")
    check(nchw(go[0]), gr[0], name="dx")
    check(go[1], gr[1], name="dw")
    if bias:
        check(go[2], gr[2], name="db")


def test_strided_conv_data_gradient_in_parity_class_order_equals_the_zero_upsampled_walk(monkeypatch):
    """dx of a stride-2 3x3 convolution (the stem's second convolution, mpvit.py:172-187; torchvision's strided BasicBlocks): tiles ordered by the parity class of
    their input pixels skip the taps that fall between the gradient's samples -- the same sums without the zero terms: bit-for-bit the full nine-tap walk"""
    from mdvit_amd import ops
    for (B, H, W, Cin, Cout) in [(2, 32, 32, 32, 64), (1, 64, 64, 64, 32), (4, 32, 64, 128, 128)]:
        x, w = nhwc(rnd(B, Cin, H, W, seed=260)).to(dev()), rnd(Cout, Cin, 3, 3, seed=261, scale=(Cin * 9) ** -0.5).to(dev())
        g = nhwc(rnd(B, Cout, H // 2, W // 2, seed=263))
        res = []
        for mode in ("1", "0"):
            monkeypatch.setenv("MDVIT_CONV_PHASE", mode)
            _, go = grads_of(lambda x, w: ops.conv3x3_dense(x, w, None, 2), [x, w], g)
            res.append(go[0])
        assert torch.equal(res[0], res[1]), (B, H, W, Cin, Cout, float((res[0] - res[1]).abs().max()))


@pytest.mark.parametrize("B,H,W,Cin,Cout,dil", [(2, 16, 16, 32, 64, 6), (1, 8, 8, 64, 32, 12), (2, 5, 7, 32, 32, 18), (1, 20, 13, 32, 64, 2)])
def test_conv3x3_dense_dilated(B, H, W, Cin, Cout, dil):
    """the ASPP branches of the 'DeepLabV3' peer heads (Utils/_deeplab.py:115-122): 3x3, dilation = padding = 6 / 12 / 18, also
    where the dilation exceeds the feature map (only the centre tap stays inside)"""
    from mdvit_amd import ops
    x, w, g = rnd(B, Cin, H, W, seed=160), rnd(Cout, Cin, 3, 3, seed=161, scale=(Cin * 9) ** -0.5), rnd(B, Cout, H, W, seed=163)
    ref, gr = grads_of(lambda x, w: F.conv2d(x.double(), w.double(), None, 1, dil, dil), [x, w], g.double())
    out, go = grads_of(lambda x, w: ops.conv3x3_dense(x, w, None, 1, dilation=dil), [nhwc(x).to(dev()), w.to(dev())], nhwc(g))
    check(nchw(out), ref, name="y")
    check(nchw(go[0]), gr[0], name="dx")
    check(go[1], gr[1], name="dw")


@pytest.mark.parametrize("G", [1, 4])
def test_grouped_weight_composition_of_the_peer_heads(G):
    """Decoders.py:315-339 evaluated as resize((Wf_q W_q) x_q + Wf_q b_q) (decode.MLPDecoderFM): the G x 4 compositions Wf[:, q-block] @ W_q and Wf[:, q-block] . b_q as
    grouped launches (ops.compose_heads) against fp64, values and all three gradient families; a head composed alone equals the same head inside a group of four, bit for bit"""
    from mdvit_amd import ops
    hid, Cs = 128, (64, 128, 320, 512)
    Wf = [rnd(hid, 4 * hid + 64, seed=400 + g, scale=hid ** -0.5) for g in range(G)]          # (the fuse weight with its extra feature block: column-slice views below)
    W = [[rnd(hid, c, 1, 1, seed=410 + 7 * g + q, scale=c ** -0.5) for q, c in enumerate(Cs)] for g in range(G)]
    b = [[rnd(hid, seed=440 + 7 * g + q) for q in range(4)] for g in range(G)]
    gW = [[rnd(hid, c, seed=470 + 7 * g + q) for q, c in enumerate(Cs)] for g in range(G)]
    gb = [[rnd(hid, seed=500 + 7 * g + q) for q in range(4)] for g in range(G)]

    def run(Wf, W, b, f64):
        Wf = [t.clone().to(torch.float64 if f64 else torch.float32).to("cpu" if f64 else dev()).requires_grad_(True) for t in Wf]
        W = [[t.clone().to(Wf[0].dtype).to(Wf[0].device).requires_grad_(True) for t in ws] for ws in W]
        b = [[t.clone().to(Wf[0].dtype).to(Wf[0].device).requires_grad_(True) for t in bs] for bs in b]
        if f64:
            comp = [[(Wf[g][:, q * hid:(q + 1) * hid] @ W[g][q].view(hid, -1), Wf[g][:, q * hid:(q + 1) * hid] @ b[g][q]) for q in range(4)] for g in range(len(Wf))]
        else:
            comp = ops.compose_heads([w[:, :4 * hid] for w in Wf], W, b)
        loss = sum((comp[g][q][0] * gW[g][q].to(Wf[0])).sum() + (comp[g][q][1] * gb[g][q].to(Wf[0])).sum() for g in range(len(Wf)) for q in range(4))
        loss.backward()
        return comp, Wf, W, b

    ref, rWf, rW, rb = run(Wf, W, b, True)
    out, oWf, oW, ob = run(Wf, W, b, False)
    for g in range(G):
        check(oWf[g].grad, rWf[g].grad, name=f"dWf[{g}]")
        for q in range(4):
            check(out[g][q][0], ref[g][q][0], name=f"Wc[{g}][{q}]")
            check(out[g][q][1], ref[g][q][1], name=f"bc[{g}][{q}]")
            check(oW[g][q].grad, rW[g][q].grad, name=f"dW[{g}][{q}]")
            check(ob[g][q].grad, rb[g][q].grad, name=f"db[{g}][{q}]")
    if G > 1:        # head 2 alone
        one, aWf, aW, ab = run(Wf[2:3], W[2:3], b[2:3], False)
        gW[0], gb[0] = gW[2], gb[2]
        one, aWf, aW, ab = run(Wf[2:3], W[2:3], b[2:3], False)
        assert all(torch.equal(one[0][q][0], out[2][q][0]) and torch.equal(one[0][q][1], out[2][q][1]) for q in range(4))
        assert torch.equal(aWf[0].grad, oWf[2].grad) and all(torch.equal(aW[0][q].grad, oW[2][q].grad) and torch.equal(ab[0][q].grad, ob[2][q].grad) for q in range(4))


@pytest.mark.parametrize("n,G", [(2, 4), (1, 4), (2, 2)])
def test_fork_with_batch_group_views_sums_every_consumer_gradient_in_one_pass(n, G):
    """ops.fork_groups(x, n, G): n aliases + G batch-group views of x (the peer heads' inputs of the domain-batched forward); the backward is the sum of the n
    full gradients and the concatenation of the G part gradients (mdvit_add_parts) == autograd's own accumulation over aliases and torch.chunk, bit for bit
    ((a + b) + part in that order)."""
    from mdvit_amd import ops
    torch.manual_seed(n * 10 + G)
    x = torch.randn(8, 6, 6, 32, device=dev(), requires_grad=True)
    ws = [torch.randn_like(x) for _ in range(n)] + [torch.randn(8 // G, 6, 6, 32, device=dev()) for _ in range(G)]
    outs = ops.fork_groups(x, n, G)
    full, parts = outs[:n], outs[n]
    assert len(parts) == G and all(torch.equal(p, c) for p, c in zip(parts, x.detach().chunk(G, 0)))
    loss = sum((a * w).sum() for a, w in zip(full, ws[:n])) + sum((p * w).sum() for p, w in zip(parts, ws[n:]))
    (got,) = torch.autograd.grad(loss, x)
    want = ws[0] if n == 1 else ws[0] + ws[1]
    want = want + torch.cat(ws[n:], 0)
    assert torch.equal(got, want)
    # a part that no consumer used: the materialised path
    outs = ops.fork_groups(x, n, G)
    loss = sum((a * w).sum() for a, w in zip(outs[:n], ws[:n])) + (outs[n][0] * ws[n]).sum()
    (got,) = torch.autograd.grad(loss, x)
    want = (ws[0] if n == 1 else ws[0] + ws[1]) + torch.cat([ws[n]] + [torch.zeros_like(ws[n])] * (G - 1), 0)
    assert torch.allclose(got, want, rtol=0, atol=1e-6)


def test_grouped_linear_equals_one_linear_per_group():
    """ops.linear_grouped (the peer heads' low-resolution linear_c products of all heads in ONE launch, forward and data gradient) against one ops.linear per group:
    same values and gradients (fp64 bound), for two of the model's shapes"""
    from mdvit_amd import ops
    for (G, B, h, K, N) in [(4, 2, 8, 320, 128), (3, 1, 16, 512, 256)]:
        xs = [rnd(B, h, h, K, seed=600 + g) for g in range(G)]
        Ws = [rnd(N, K, seed=610 + g, scale=K ** -0.5) for g in range(G)]
        bs = [rnd(N, seed=620 + g) for g in range(G)]
        gs = [rnd(B, h, h, N, seed=630 + g) for g in range(G)]

        def run(grouped, f64=False):
            dt, dv = (torch.float64, "cpu") if f64 else (torch.float32, dev())
            x = [t.clone().to(dt).to(dv).requires_grad_(True) for t in xs]
            W = [t.clone().to(dt).to(dv).requires_grad_(True) for t in Ws]
            b = [t.clone().to(dt).to(dv).requires_grad_(True) for t in bs]
            if f64:
                ys = [F.linear(x[g], W[g], b[g]) for g in range(G)]
            elif grouped:
                ys = ops.linear_grouped(x, W, b)
            else:
                ys = [ops.linear(x[g], W[g], b[g]) for g in range(G)]
            sum((ys[g] * gs[g].to(dt).to(dv)).sum() for g in range(G)).backward()
            return ys, x, W, b

        ref, rx, rW, rb = run(False, True)
        out, ox, oW, ob = run(True)
        one, px, pW, pb = run(False)
        for g in range(G):
            check(out[g], ref[g], name=f"y[{g}]"); check(ox[g].grad, rx[g].grad, name=f"dx[{g}]")
            check(oW[g].grad, rW[g].grad, name=f"dW[{g}]"); check(ob[g].grad, rb[g].grad, name=f"db[{g}]")
            check(out[g], one[g], tol=2e-6, name=f"y[{g}] vs per-group launch"); check(ox[g].grad, px[g].grad, tol=2e-6, name=f"dx[{g}] vs per-group launch")


def test_elementwise_dropout_and_global_avg_pool(monkeypatch):
    from mdvit_amd import ops
    x = rnd(3, 11, 13, 64, seed=170).to(dev()).requires_grad_(True)
    # global average pool (nn.AdaptiveAvgPool2d(1)) and its broadcast backward
    g = rnd(3, 64, seed=171).to(dev())
    y = ops.global_avg_pool(x)
    y.backward(g)
    check(y, x.detach().double().mean(dim=(1, 2)), name="pooled")
    check(x.grad, (g.double() / (11 * 13)).view(3, 1, 1, 64).expand(3, 11, 13, 64), name="d pooled")
    # element-wise dropout: kept fraction, scaling, and the SAME mask on the gradient
    t = torch.ones(1 << 18, device=dev(), requires_grad=True)
    d = ops.dropout(t, 0.25, True)
    kept = d.detach() != 0
    assert abs(float(kept.float().mean()) - 0.75) < 5e-3
    assert torch.allclose(d.detach()[kept], torch.full_like(d.detach()[kept], 1.0 / 0.75))
    d.backward(torch.full_like(d, 3.0))
    assert torch.equal(t.grad != 0, kept) and torch.allclose(t.grad[kept], torch.full_like(t.grad[kept], 4.0))
    assert ops.dropout(t, 0.25, False) is t and ops.dropout(t, 0.0, True) is t
    d2 = ops.dropout(t, 0.25, True)
    assert not torch.equal(d2.detach() != 0, kept)                     # a new key per call


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (1, 17, 23), (3, 64, 48)])
def test_stem_conv(B, H, W):
    from mdvit_amd import ops
    img, w = rnd(B, 3, H, W, seed=70, scale=2.0), rnd(32, 3, 3, 3, seed=71, scale=0.2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = rnd(B, 32, Ho, Wo, seed=72)
    wr = w.clone().requires_grad_(True)
    ref = F.conv2d(img.double(), wr.double(), None, 2, 1)
    ref.backward(g.double())
    wh = w.to(dev()).requires_grad_(True)
    out = ops.stem_conv(img.to(dev()), wh)
    out.backward(nhwc(g).to(dev()))
    check(nchw(out), ref, name="y")
    check(wh.grad, wr.grad, name="dw")


def test_every_adapter_of_a_network_in_one_launch_equals_the_per_block_launches():
    """mdvit_da_fwd_many (ops.da_precomputed: the model computes every block's domain adapter at the top of its forward) against mdvit_da_fwd per adapter, bit for
    bit; and an attention node inside the context picks its adapter output up instead of launching (same result, gradients included)."""
    from mdvit_amd import ops
    B, D = 6, 4
    label = F.one_hot(torch.arange(B) % D, D).float().to(dev())
    ads = []
    for i, (Cn, heads) in enumerate(((64, 8), (128, 8), (320, 8), (512, 8), (64, 8))):
        hid = max(Cn // 2, 4)
        ads.append((rnd(hid, D, seed=500 + i).to(dev()), rnd(hid, seed=510 + i).to(dev()), rnd(Cn, hid, seed=520 + i, scale=hid ** -0.5).to(dev()), rnd(Cn, seed=530 + i).to(dev()), heads))
    ref = [ops.domain_adapter(label, W1, b1, W2, b2, h) for (W1, b1, W2, b2, h) in ads]
    with ops.da_precomputed(label, ads):
        for (W1, b1, W2, b2, h), r in zip(ads, ref):
            got = ops._da_lookup(W2, B)
            assert got is not None and torch.equal(got, r)
        assert ops._da_lookup(ads[0][2], B + 1) is None
    assert ops._da_pre is None
    # through the attention node: with and without the context
    Cn, heads, H, W_ = 64, 8, 8, 8
    W1, b1, W2, b2, _ = ads[0]
    qkv = rnd(B, H * W_, 3 * Cn, seed=540).to(dev())
    crpe = [rnd(*sh, seed=550 + i, scale=0.2).to(dev()) for i, sh in enumerate(((16, 1, 3, 3), (16,), (24, 1, 5, 5), (24,), (24, 1, 7, 7), (24,)))]
    g = rnd(B, H * W_, Cn, seed=560).to(dev())
    outs = []
    for pre in (False, True):
        ins = [t.clone().requires_grad_(True) for t in (qkv, W1, b1, W2, b2)]
        ctx = ops.da_precomputed(label, [(ins[1], ins[2], ins[3], ins[4], heads)]) if pre else contextlib.nullcontext()
        with ctx:
            y = ops.factor_att(ins[0], crpe, H, W_, heads, (2, 3, 3), label, (ins[1], ins[2], ins[3], ins[4]))
        y.backward(g)
        outs.append([y.detach()] + [t.grad for t in ins])
    assert torch.equal(outs[0][0], outs[1][0])                      # the forward: bit for bit
    for a_, b_ in zip(outs[0][1:], outs[1][1:]):                    # (the adapter's e sums float adds in LDS: run-to-run order, last-bit differences in either mode)
        assert float((a_ - b_).abs().max()) <= 1e-5 * float(b_.abs().max())


def test_every_adapter_backward_of_a_sweep_in_two_launches_equals_the_per_block_launches():
    """mdvit_da_bwd_many (ops._DaMany.backward: the blocks hand their e = a * dL/da out and the adapters' parameter gradients are formed once per sweep) against
    mdvit_da_bwd per adapter, bit for bit: both signs of the scale, an adapter without e skipped (its outputs untouched); and the same through autograd."""
    import ctypes as C
    from mdvit_amd import ops, _lib
    from mdvit_amd._lib import call
    B, D = 6, 4
    label = F.one_hot(torch.arange(B) % D, D).float().to(dev())
    ads = []
    for i, (Cn, heads) in enumerate(((64, 8), (128, 8), (320, 8), (512, 8), (64, 8), (216, 8))):
        hid = max(Cn // 2, 4)
        ads.append((rnd(hid, D, seed=600 + i).to(dev()), rnd(hid, seed=610 + i).to(dev()), rnd(Cn, hid, seed=620 + i, scale=hid ** -0.5).to(dev()), rnd(Cn, seed=630 + i).to(dev()), heads))
    params = [t for ad in ads for t in ad[:4]]
    heads = tuple(ad[4] for ad in ads)
    outs = ops._DaMany.apply(label, heads, *params)
    es = [rnd(B, ad[2].shape[0], seed=640 + i).to(dev()) for i, ad in enumerate(ads)]
    skip = 2
    for scale in (1.0, -1.0):
        m = ops._da_many_desc(label, params, heads, outs)
        g = _lib.DaManyGrads()
        got = []
        for i, ad in enumerate(ads):
            bufs = [torch.full_like(t, float("nan")) for t in ad[:4]]
            got.append(bufs)
            if i != skip:
                g.e[i] = ops._p(es[i])
                g.dW1[i], g.db1[i], g.dW2[i], g.db2[i] = (ops._p(t) for t in bufs)
        wsb = _lib.load().mdvit_da_many_ws_bytes(C.byref(m), B)
        ws = torch.empty(wsb // 4, device=dev())
        call("mdvit_da_bwd_many", C.byref(m), C.byref(g), ops._p(label), scale, ops._p(ws), wsb, B, D, ops._stream())
        for i, (W1, b1, W2, b2, h) in enumerate(ads):
            if i == skip:
                assert all(bool(torch.isnan(t).all()) for t in got[i])
                continue
            ref = [torch.full_like(t, float("nan")) for t in (W1, b1, W2, b2)]
            dab = _lib.load().mdvit_da_ws_bytes(B, W1.shape[0], W2.shape[0])
            daws = torch.empty(dab // 4, device=dev())
            call("mdvit_da_bwd", ops._p(label), ops._p(W1), ops._p(b1), ops._p(W2), ops._p(b2), ops._p(outs[i]), ops._p(es[i]), scale, *[ops._p(t) for t in ref],
                 ops._p(daws), dab, B, D, W1.shape[0], W2.shape[0], h, ops._stream())
            for a_, b_ in zip(got[i], ref):
                assert torch.equal(a_, b_), (i, scale)
    # through autograd: the node's backward with one e missing
    ps = [t.clone().requires_grad_(True) for t in params]
    outs2 = ops._DaMany.apply(label, heads, *ps)
    live = [i for i in range(len(ads)) if i != skip]
    torch.autograd.backward([outs2[i] for i in live], [es[i] for i in live])
    for i in range(len(ads)):
        for j in range(4):
            if i == skip:
                assert ps[4 * i + j].grad is None
            else:
                ref_ = got  # (scale -1 was the last direct run)
                assert torch.equal(ps[4 * i + j].grad, -ref_[i][j])


def test_conv_weight_layouts_of_many_weights_in_one_launch():
    """mdvit_conv_weight_relayout_many (the per-step refresh of every implicit-convolution weight layout, LDS-tiled since round 5) against the index definition
    (include/mdvit_hip.h: mode 0 out[co][tap][ci], mode 1 out[ci][8 - tap][co]) -- channel counts off the tile sizes included"""
    from mdvit_amd import ops
    from mdvit_amd._lib import call
    shapes = [(32, 3), (64, 64), (40, 20), (512, 320), (33, 257), (7, 5)]
    ws = [rnd(co, ci, 3, 3, seed=300 + i).to(dev()) for i, (co, ci) in enumerate(shapes)]
    rows, outs = [], []
    for w in ws:
        for mode in (0, 1):
            o = torch.full((w.numel(),), float("nan"), device=dev())
            outs.append((w, mode, o))
            rows.append([w.data_ptr(), o.data_ptr(), w.shape[0], w.shape[1], mode])
    table = torch.tensor(rows, dtype=torch.int64, device=dev())
    for blocks in (1, 7, 256):
        for _, _, o in outs:
            o.fill_(float("nan"))
        call("mdvit_conv_weight_relayout_many", ops._p(table), len(rows), blocks, ops._stream())
        torch.cuda.synchronize()
        for w, mode, o in outs:
            co, ci = w.shape[:2]
            ref = w.reshape(co, ci, 9).permute(0, 2, 1) if mode == 0 else w.reshape(co, ci, 9).flip(2).permute(1, 2, 0)
            assert torch.equal(o, ref.contiguous().reshape(-1)), (tuple(w.shape), mode, blocks)


@pytest.mark.parametrize("act", ["hswish", "relu"])
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 64), (4, 3, 5, 320), (1, 8, 8, 1024)])
def test_bn_act_train(act, B, H, W, C):
    from mdvit_amd import ops, _lib
    a = _lib.ACT_HSWISH if act == "hswish" else _lib.ACT_RELU
    fn = F.hardswish if act == "hswish" else F.relu
    y, ga, be, g = rnd(B, C, H, W, seed=80, scale=2.0) + 0.3, 1 + 0.5 * rnd(C, seed=81), rnd(C, seed=82, scale=0.2), rnd(B, C, H, W, seed=83)
    rm0, rv0 = rnd(C, seed=84, scale=0.1), 1 + 0.5 * rnd(C, seed=85)
    rm, rv = rm0.clone().double(), rv0.clone().double()
    ref, gr = grads_of(lambda y, ga, be: fn(F.batch_norm(y.double(), rm, rv, ga.double(), be.double(), True, 0.1, 1e-5)), [y, ga, be], g.double())
    rmh, rvh, nbt = rm0.to(dev()), rv0.to(dev()), torch.tensor(3, device=dev())
    out, go = grads_of(lambda y, ga, be: ops.bn_act(y, ga, be, rmh, rvh, nbt, True, a), [nhwc(y).to(dev()), ga.to(dev()), be.to(dev())], nhwc(g))
    check(nchw(out), ref, name="z")
    check(nchw(go[0]), gr[0], tol=3e-4, name="dy")
    check(go[1], gr[1], tol=3e-4, name="dgamma")
    check(go[2], gr[2], tol=3e-4, name="dbeta")
    check(rmh, rm, name="running_mean")
    check(rvh, rv, name="running_var")
    assert int(nbt) == 4


@pytest.mark.parametrize("G,Bg,H,W,C", [(4, 2, 8, 8, 64), (2, 3, 5, 3, 320), (4, 1, 16, 16, 32)])
def test_bn_act_grouped_equals_consecutive_forwards(G, Bg, H, W, C):
    """bn_groups(G): per-domain-batch statistics in ONE call == G consecutive BatchNorm forwards (outputs, all
    gradients, and the running statistics after G momentum updates in order)"""
    from mdvit_amd import ops, _lib
    y, ga, be, g = rnd(G * Bg, C, H, W, seed=86, scale=2.0) + 0.3, 1 + 0.5 * rnd(C, seed=87), rnd(C, seed=88, scale=0.2), rnd(G * Bg, C, H, W, seed=89)
    y = y + torch.arange(G).repeat_interleave(Bg).view(-1, 1, 1, 1).float()        # groups with different statistics
    rm0, rv0 = rnd(C, seed=84, scale=0.1), 1 + 0.5 * rnd(C, seed=85)
    rm, rv = rm0.clone().double(), rv0.clone().double()

    def ref_fn(y, ga, be):
        return torch.cat([F.hardswish(F.batch_norm(y[i * Bg:(i + 1) * Bg].double(), rm, rv, ga.double(), be.double(), True, 0.1, 1e-5))
                          for i in range(G)], 0)
    ref, gr = grads_of(ref_fn, [y, ga, be], g.double())
    rmh, rvh, nbt = rm0.to(dev()), rv0.to(dev()), torch.tensor(0, device=dev())

    def our_fn(y, ga, be):
        with ops.bn_groups(G):
            return ops.bn_act(y, ga, be, rmh, rvh, nbt, True, _lib.ACT_HSWISH)
    out, go = grads_of(our_fn, [nhwc(y).to(dev()), ga.to(dev()), be.to(dev())], nhwc(g))
    check(nchw(out), ref, name="z")
    check(nchw(go[0]), gr[0], tol=3e-4, name="dy")
    check(go[1], gr[1], tol=3e-4, name="dgamma")
    check(go[2], gr[2], tol=3e-4, name="dbeta")
    check(rmh, rm, name="running_mean")
    check(rvh, rv, name="running_var")
    assert int(nbt) == G
    # and it is bit-identical to calling the same kernels group by group
    rm2, rv2, nbt2 = rm0.to(dev()), rv0.to(dev()), torch.tensor(0, device=dev())
    yd = nhwc(y).to(dev())
    sep = torch.cat([ops.bn_act(yd[i * Bg:(i + 1) * Bg].contiguous(), ga.to(dev()), be.to(dev()), rm2, rv2, nbt2, True, _lib.ACT_HSWISH)
                     for i in range(G)], 0)
    assert torch.equal(sep, out.detach()) and torch.equal(rm2, rmh) and torch.equal(rv2, rvh)


@pytest.mark.parametrize("G,Bg,H,W,C,training", [(4, 2, 8, 8, 64, True), (2, 3, 5, 3, 320, True), (3, 1, 16, 16, 32, True), (4, 2, 4, 4, 128, False)])
def test_bn_act_per_group_parameters(G, Bg, H, W, C, training):
    """[G, C] parameter / running-statistic rows (the per-domain BatchNorm banks of MDViT_DSN on a domain-batched
    tensor): group g is normalised with row g and updates row g only == G independent BatchNorms"""
    from mdvit_amd import ops, _lib
    y, g = rnd(G * Bg, C, H, W, seed=186, scale=2.0) + 0.3, rnd(G * Bg, C, H, W, seed=189)
    y = y + torch.arange(G).repeat_interleave(Bg).view(-1, 1, 1, 1).float()
    ga, be = 1 + 0.5 * rnd(G, C, seed=187), rnd(G, C, seed=188, scale=0.2)
    rm0, rv0 = rnd(G, C, seed=184, scale=0.1), 1 + 0.5 * rnd(G, C, seed=185).abs()
    rm, rv = rm0.clone().double(), rv0.clone().double()

    def ref_fn(y, ga, be):
        return torch.cat([F.relu(F.batch_norm(y[i * Bg:(i + 1) * Bg].double(), rm[i], rv[i], ga[i].double(), be[i].double(), training, 0.1, 1e-5))
                          for i in range(G)], 0)
    ref, gr = grads_of(ref_fn, [y, ga, be], g.double())
    rmh, rvh, nbt = rm0.to(dev()), rv0.to(dev()), torch.zeros(G, dtype=torch.long, device=dev())

    def our_fn(y, ga, be):
        with ops.bn_groups(G):
            return ops.bn_act(y, ga, be, rmh, rvh, nbt, training, _lib.ACT_RELU)
    out, go = grads_of(our_fn, [nhwc(y).to(dev()), ga.to(dev()), be.to(dev())], nhwc(g))
    check(nchw(out), ref, name="z")
    check(nchw(go[0]), gr[0], tol=3e-4, name="dy")
    check(go[1], gr[1], tol=3e-4, name="dgamma rows")
    check(go[2], gr[2], tol=3e-4, name="dbeta rows")
    check(rmh, rm, name="running_mean rows")
    check(rvh, rv, name="running_var rows")
    assert nbt.tolist() == [1 if training else 0] * G
    with pytest.raises(ValueError):
        ops.bn_act(nhwc(y).to(dev()), ga.to(dev()), be.to(dev()), rmh, rvh, None, training, _lib.ACT_RELU)      # no bn_groups(G) active


@pytest.mark.parametrize("G,Mg,C", [(4, 128, 64), (2, 100, 128), (4, 37, 320), (3, 50, 512), (2, 33, 96), (1, 77, 64)])
def test_layer_norm_per_group_parameters(G, Mg, C):
    """gamma/beta [G, C]: row g normalises the g-th of G equal row groups (norm1s / norm2s of MDViT_DSN on a
    domain-batched token tensor) == G LayerNorms; the forked form adds the residual gradient"""
    from mdvit_amd import ops
    x, g, g2 = rnd(G * Mg, C, seed=190, scale=1.5) + 0.2, rnd(G * Mg, C, seed=191), rnd(G * Mg, C, seed=192)
    ga, be = 1 + 0.5 * rnd(G, C, seed=193), rnd(G, C, seed=194, scale=0.3)

    def ref_fn(x, ga, be):
        return torch.cat([F.layer_norm(x[i * Mg:(i + 1) * Mg].double(), (C,), ga[i].double(), be[i].double(), 1e-6) for i in range(G)], 0)
    ref, gr = grads_of(ref_fn, [x, ga, be], g.double())
    out, go = grads_of(lambda x, ga, be: ops.layer_norm(x, ga, be, 1e-6), [x.to(dev()), ga.to(dev()), be.to(dev())], g)
    check(out, ref, name="y")
    check(go[0], gr[0], tol=3e-4, name="dx")
    check(go[1], gr[1], tol=3e-4, name="dgamma rows")
    check(go[2], gr[2], tol=3e-4, name="dbeta rows")
    # forked: (LN(x), x) with the gradient of the second output added inside the backward kernel
    xs = [t.to(dev()).requires_grad_(True) for t in (x, ga, be)]
    yv, xr = ops.layer_norm_fork(xs[0], xs[1], xs[2], 1e-6)
    torch.autograd.backward([yv, xr], [g.to(dev()), g2.to(dev())])
    check(xs[0].grad, gr[0] + g2.double(), tol=3e-4, name="dx + residual gradient")
    check(xs[1].grad, gr[1], tol=3e-4, name="dgamma rows (fork)")


def test_split_groups_backward_handles_missing_gradients():
    from mdvit_amd import ops
    x = rnd(6, 5, 4, seed=120).to(dev()).requires_grad_(True)
    a, b, c = ops.split_groups(x, 3)
    (a.sum() * 2 + c.sum() * 3).backward()
    want = torch.cat([torch.full((2, 5, 4), 2.0), torch.zeros(2, 5, 4), torch.full((2, 5, 4), 3.0)]).to(dev())
    assert torch.equal(x.grad, want)


def test_bn_act_eval_and_dropout2d():
    from mdvit_amd import ops, _lib
    B, H, W, C = 4, 8, 8, 64
    y, ga, be = rnd(B, C, H, W, seed=90), 1 + 0.5 * rnd(C, seed=91), rnd(C, seed=92, scale=0.2)
    rm, rv = rnd(C, seed=93, scale=0.3), 1 + 0.5 * rnd(C, seed=94)
    ref = F.relu(F.batch_norm(y.double(), rm.double(), rv.double(), ga.double(), be.double(), False, 0.1, 1e-5))
    rmh, rvh = rm.to(dev()), rv.to(dev())
    out = ops.bn_act(nhwc(y).to(dev()), ga.to(dev()), be.to(dev()), rmh, rvh, None, False, _lib.ACT_RELU)
    check(nchw(out), ref, name="eval z")
    check(rmh, rm, tol=0, name="running_mean untouched")
    # Dropout2d: whole (sample, channel) planes are zeroed, survivors scaled by 1/keep
    B, H, W, C = 16, 4, 4, 512
    yy = (rnd(B, H, W, C, seed=95).abs() + 0.5).to(dev())
    one, zero = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    z_plain = ops.bn_act(yy, one, zero, zero.clone(), one.clone(), None, False, _lib.ACT_NONE)
    z = ops.bn_act(yy, one, zero, zero.clone(), one.clone(), None, True, _lib.ACT_NONE, drop2d_p=0.25)
    # training-mode BN normalises, so compare plane-wise zero pattern only
    planes = (z.abs().sum(dim=(1, 2)) == 0)
    frac = planes.float().mean().item()
    assert abs(frac - 0.25) < 0.03, f"dropped plane fraction {frac}"
    partial = ((z == 0).float().mean(dim=(1, 2)) > 0) & ~planes
    assert not partial.any(), "Dropout2d must drop whole planes"
    assert z_plain.abs().min() > 0


@pytest.mark.parametrize("B,H,W,C,act,drop,training", [(3, 16, 16, 512, "relu", 0.25, True), (2, 9, 7, 256, "hswish", 0.0, True), (2, 8, 8, 512, "relu", 0.0, False),
                                                        (1, 32, 32, 1024, "relu", 0.1, True)])
def test_bn_act_rowdot_fused_equals_bn_act_then_rowdot(B, H, W, C, act, drop, training, monkeypatch):
    """ops.bn_act_rowdot (BatchNorm -> activation -> Dropout2d -> 1-channel 1x1 conv in one op, the tail of the peer heads, Decoders.py:304-311)
    against the two operators it replaces on the same dropout key: output, data gradient, the four parameter gradients, running statistics;
    the data-gradient-only sweep; and without dropout against an fp64 restatement."""
    import itertools
    from mdvit_amd import ops
    from mdvit_amd._lib import ACT_HSWISH, ACT_RELU
    a = ACT_RELU if act == "relu" else ACT_HSWISH
    y0, gam, bet = rnd(B, H, W, C, seed=300, scale=2.0), rnd(C, seed=301) + 1.5, rnd(C, seed=302)
    w, b = rnd(1, C, 1, 1, seed=303, scale=0.2), rnd(1, seed=304)
    g = rnd(B, H, W, seed=305)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_key_counter", itertools.count(500))
        ins = [t.to(dev()).requires_grad_(True) for t in (y0, gam, bet, w, b)]
        rm, rv, nbt = torch.zeros(C, device=dev()), torch.ones(C, device=dev()), torch.zeros((), dtype=torch.long, device=dev())
        if not training:
            rm, rv = rnd(C, seed=306).to(dev()), (rnd(C, seed=307).abs() + 0.5).to(dev())
        if fused:
            low = ops.bn_act_rowdot(ins[0], ins[1], ins[2], rm, rv, nbt, training, a, ins[3], ins[4], drop2d_p=drop)
        else:
            low = ops.rowdot(ops.bn_act(ins[0], ins[1], ins[2], rm, rv, nbt, training, a, drop2d_p=drop), ins[3], ins[4])
        low.backward(g.to(dev()))
        res.append([low.detach()] + [t.grad for t in ins] + [rm.clone(), rv.clone()])
    for name, x_, r_ in zip(("low", "dy", "dgamma", "dbeta", "dw", "db", "running_mean", "running_var"), res[0], res[1]):
        check(x_, r_, tol=5e-6, name=name)
    # data-gradient-only sweep: dy alone
    monkeypatch.setattr(ops, "_key_counter", itertools.count(500))
    ins = [t.to(dev()).requires_grad_(True) for t in (y0, gam, bet, w, b)]
    rm, rv = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
    if not training:
        rm, rv = rnd(C, seed=306).to(dev()), (rnd(C, seed=307).abs() + 0.5).to(dev())
    low = ops.bn_act_rowdot(ins[0], ins[1], ins[2], rm, rv, None, training, a, ins[3], ins[4], drop2d_p=drop)
    ops.set_dgrad_only(True)
    try:
        low.backward(g.to(dev()))
    finally:
        ops.set_dgrad_only(False)
    check(ins[0].grad, res[0][1], tol=1e-6, name="dy (data-gradient-only sweep)")
    assert all(t.grad is None for t in ins[1:])
    if drop == 0.0:
        def ref_fn(y, gm_, bt_, w_, b_):
            y2 = y.double().reshape(-1, C)
            if training:
                mu, var = y2.mean(0), y2.var(0, unbiased=False)
            else:
                mu, var = rm.double().cpu(), rv.double().cpu()
            pre = (y2 - mu) / torch.sqrt(var + 1e-5) * gm_.double() + bt_.double()
            z = torch.relu(pre) if act == "relu" else F.hardswish(pre)
            return (z @ w_.double().reshape(-1) + b_.double()).reshape(B, H, W)
        ref, gr = grads_of(ref_fn, [y0, gam, bet, w, b], g.double())
        for name, x_, r_ in zip(("low", "dy", "dgamma", "dbeta", "dw", "db"), res[0], [ref] + gr):
            check(x_, r_, tol=2e-4, name=name + " vs fp64")


@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo,C", [(2, 8, 8, 16, 16, 64), (1, 4, 4, 32, 32, 128), (2, 16, 16, 64, 64, 1), (1, 3, 4, 24, 32, 512), (2, 5, 7, 11, 13, 8), (1, 6, 8, 6, 8, 64)])
def test_upsample(B, Hi, Wi, Ho, Wo, C):
    from mdvit_amd.ops import _Upsample
    x, g = rnd(B, C, Hi, Wi, seed=100), rnd(B, C, Ho, Wo, seed=101)
    ref, gr = grads_of(lambda x: F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=False), [x], g.double())
    out, go = grads_of(lambda x: _Upsample.apply(x, Ho, Wo, None), [nhwc(x).to(dev())], nhwc(g))
    check(nchw(out), ref, name="y")
    check(nchw(go[0]), gr[0], name="dx")
    base = rnd(B, Ho, Wo, C, seed=102).to(dev())
    out2 = _Upsample.apply(nhwc(x).to(dev()), Ho, Wo, base)          # base + resize(x) in one pass
    check(out2, out.detach() + base, name="accumulate")


@pytest.mark.parametrize("B,Ho,Wo,C", [(2, 24, 40, 64), (3, 8, 72, 72), (1, 16, 128, 512), (2, 24, 48, 128)], ids=["row_in_one_unit", "ragged_second_unit", "peer_head_row_lds_tiles", "lds_tiles_3x3_per_image"])
def test_upsample_sum_equals_chained_resizes(B, Ho, Wo, C):
    """ops.upsample_sum (base + three bilinear sources in one pass; the backward's width folds in one launch) == the chained single-source calls:
    forward and every gradient to fp32 round-off, and the forward against F.interpolate in fp64.  (The forward walks an output row in units of 1024 channel
    quads: one unit, a ragged second unit; shapes with Ho % 8 == Wo % 16 == C % 128 == 0 and upscale factors 2 / 4 / 8 take the LDS-tiled kernel
    -- the peer heads' 128 x 512 rows, and 3 x 3 tiles per image over two images.)"""
    from mdvit_amd import ops
    base = rnd(B, Ho, Wo, C, seed=400)
    xs = [rnd(B, Ho // 2, Wo // 2, C, seed=401), rnd(B, Ho // 4, Wo // 4, C, seed=402), rnd(B, Ho // 8, Wo // 8, C, seed=403)]
    g = rnd(B, Ho, Wo, C, seed=404).to(dev())
    res = []
    for fused in (True, False):
        ins = [t.to(dev()).requires_grad_(True) for t in [base] + xs]
        if fused:
            y = ops.upsample_sum(ins[0], ins[1:], Ho, Wo)
        else:
            y = ins[0]
            for x in ins[1:]:
                y = ops.upsample_bilinear(x, Ho, Wo, base=y)
        y.backward(g)
        res.append([y.detach()] + [t.grad for t in ins])
    check(res[0][0], res[1][0], tol=1e-6, name="y fused vs chained")       # the compiler contracts the tap sums differently: round-off, not bits
    for name, a, b in zip(("dbase", "dx1", "dx2", "dx3"), res[0][1:], res[1][1:]):
        check(a, b, tol=1e-6, name=name)
    ref = base.double() + sum(F.interpolate(x.double().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for x in xs)
    check(res[0][0], ref, tol=1e-5, name="y vs F.interpolate")
    # without a base
    y2 = ops.upsample_sum(None, [x.to(dev()) for x in xs[:2]], Ho, Wo)
    ref2 = sum(F.interpolate(x.double().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for x in xs[:2])
    check(y2, ref2, tol=1e-5, name="y without base")


def test_rowdot():
    from mdvit_amd import ops
    x, w, b, g = rnd(3000, 64, seed=110), rnd(1, 64, 1, 1, seed=111), rnd(1, seed=112), rnd(3000, seed=113)
    ref, gr = grads_of(lambda x, w, b: x.double() @ w.double().view(-1) + b.double(), [x, w, b], g.double())
    out, go = grads_of(lambda x, w, b: ops.rowdot(x, w, b), [x.to(dev()), w.to(dev()), b.to(dev())], g)
    check(out, ref, name="y")
    for n, a, r in zip(("dx", "dw", "db"), go, gr):
        check(a, r, name=n)
    # strided rows (a column slice of a wider matrix), K = 512
    Wf, v = rnd(512, 2112, seed=114), rnd(512, seed=115)
    ref2, gr2 = grads_of(lambda Wf, v: Wf.double()[:, 1024:1536] @ v.double(), [Wf, v], rnd(512, seed=116).double())
    out2, go2 = grads_of(lambda Wf, v: ops.rowdot(Wf[:, 1024:1536], v), [Wf.to(dev()), v.to(dev())], rnd(512, seed=116))
    check(out2, ref2, name="y slice")
    check(go2[0], gr2[0], name="dWf slice")
    check(go2[1], gr2[1], name="dv slice")


@pytest.mark.parametrize("C", [64, 128, 320, 512])
def test_domain_adapter_forward_and_exact_gather(C):
    from mdvit_amd import ops
    B, hid, heads = 5, max(C // 2, 4), 8
    lab = F.one_hot(torch.tensor([0, 3, 1, 2, 3]), 4).float()
    W1, b1, W2, b2 = rnd(hid, 4, seed=120, scale=1.5), rnd(hid, seed=121, scale=0.1), rnd(C, hid, seed=122, scale=3 / hid ** 0.5), rnd(C, seed=123, scale=0.1)
    z = F.linear(torch.relu(F.linear(lab.double(), W1.double(), b1.double())), W2.double(), b2.double())
    ref = torch.softmax(z.view(B, heads, C // heads), dim=1).reshape(B, C)
    P = [t.to(dev()) for t in (W1, b1, W2, b2)]
    check(ops.domain_adapter(lab.to(dev()), *P, heads), ref, name="a")
    # domain-id routing is exact: one_hot(d) @ W1^T == the gathered column W1[:, d] (bit-for-bit)
    for d in range(4):
        a_onehot = ops.domain_adapter(F.one_hot(torch.tensor([d]), 4).float().to(dev()), *P, heads)
        W1g = torch.zeros_like(W1); W1g[:, 0] = W1[:, d]
        a_gather = ops.domain_adapter(torch.tensor([[1.0, 0, 0, 0]], device=dev()), W1g.to(dev()), P[1], P[2], P[3], heads)
        assert torch.equal(a_onehot, a_gather), f"domain {d}: gather not bit-exact"


def _attn_ref(qkv, crpe, a, H, W, heads, splits=(2, 3, 3)):
    """restatement of the attention core on (B,N,3C) qkv (mdvit.py:293-304) in the dtype of its arguments (the tests pass doubles); splits = the head counts
    (s3, s5, s7) of the three window classes."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    Ch = C // heads
    q, k, v = [t.reshape(B, N, heads, Ch).permute(0, 2, 1, 3) for t in qkv.split(C, dim=2)]
    M = torch.softmax(k, dim=2).transpose(2, 3) @ v
    fa = q @ M
    vimg = v.permute(0, 1, 3, 2).reshape(B, C, H, W)
    w3, b3, w5, b5, w7, b7 = crpe
    c1, c2 = splits[0] * Ch, (splits[0] + splits[1]) * Ch
    conv = torch.cat([F.conv2d(vimg[:, :c1], w3, b3, 1, 1, 1, c1), F.conv2d(vimg[:, c1:c2], w5, b5, 1, 2, 1, c2 - c1),
                      F.conv2d(vimg[:, c2:], w7, b7, 1, 3, 1, C - c2)], 1)
    conv = conv.reshape(B, heads, Ch, N).permute(0, 1, 3, 2)
    y = Ch ** -0.5 * fa + q * conv
    if a is not None:
        y = a.view(B, heads, 1, Ch) * y
    return y.permute(0, 2, 1, 3).reshape(B, N, C)


@pytest.mark.parametrize("B,H,W,C,use_a", [(2, 16, 16, 64, True), (1, 9, 14, 128, True), (2, 8, 8, 320, True), (2, 4, 4, 512, True), (2, 12, 12, 64, False), (1, 40, 40, 64, True),
                                              (1, 64, 64, 64, True), (1, 70, 66, 128, False), (3, 33, 47, 64, True), (2, 50, 50, 128, True)])
def test_factor_att_core(B, H, W, C, use_a):
    """attention core + domain adapter node: forward, dqkv, crpe gradients and the adapter's parameter gradients
    (shapes 7 / 8 have >= 4096 tokens per image: the packed two-row stencil tiles of conv_tile.h, the second with ragged tile edges; the last two walk several
    64-token tiles per workgroup with a ragged last one on three / two images: round 6's streaming kernels fa_partial_s8 / fa_bwd_apply_s8 / _s16 at C = 64 / 128)"""
    from mdvit_amd import ops
    heads, Ch, N, hid = 8, C // 8, H * W, max(C // 2, 4)
    qkv = rnd(B, N, 3 * C, seed=130, scale=1.5)
    crpe = [rnd(2 * Ch, 1, 3, 3, seed=131, scale=0.3), rnd(2 * Ch, seed=132, scale=0.1), rnd(3 * Ch, 1, 5, 5, seed=133, scale=0.2), rnd(3 * Ch, seed=134, scale=0.1),
            rnd(3 * Ch, 1, 7, 7, seed=135, scale=0.15), rnd(3 * Ch, seed=136, scale=0.1)]
    da = [rnd(hid, 4, seed=137, scale=1.5), rnd(hid, seed=138, scale=0.1), rnd(C, hid, seed=139, scale=3 / hid ** 0.5), rnd(C, seed=140, scale=0.1)]
    lab = F.one_hot(torch.tensor([2, 0, 3][:B]), 4).float()
    g = rnd(B, N, C, seed=141)
    ins = [qkv] + crpe + (da if use_a else [])

    def ref_fn(qkv, *rest):
        cr = [t.double() for t in rest[:6]]
        a = None
        if use_a:
            W1, b1, W2, b2 = [t.double() for t in rest[6:]]
            z = F.linear(torch.relu(F.linear(lab.double(), W1, b1)), W2, b2)
            a = torch.softmax(z.view(B, heads, Ch), dim=1).reshape(B, C)
        return _attn_ref(qkv.double(), cr, a, H, W, heads)

    def hip_fn(qkv, *rest):
        if use_a:
            return ops.factor_att(qkv, tuple(rest[:6]), H, W, heads, (2, 3, 3), lab.to(dev()), tuple(rest[6:]))
        return ops.factor_att(qkv, tuple(rest[:6]), H, W, heads)

    ref, gr = grads_of(ref_fn, ins, g.double())
    out, go = grads_of(hip_fn, [t.to(dev()) for t in ins], g)
    check(out, ref, name="y")
    names = ["dqkv", "dw3", "db3", "dw5", "db5", "dw7", "db7"] + (["dW1", "db1", "dW2", "db2"] if use_a else [])
    for n, x, r in zip(names, go, gr):
        check(x, r, tol=3e-4, name=n)


def test_factor_att_softmax_is_shift_invariant_and_stable():
    """column softmax over tokens with a large offset on K must not overflow (online max handling)."""
    from mdvit_amd import ops
    B, H, W, C, heads = 1, 16, 16, 64, 8
    Ch = C // heads
    qkv = rnd(B, H * W, 3 * C, seed=140)
    crpe = [rnd(2 * Ch, 1, 3, 3, seed=141, scale=0.3), rnd(2 * Ch, seed=142), rnd(3 * Ch, 1, 5, 5, seed=143, scale=0.2), rnd(3 * Ch, seed=144),
            rnd(3 * Ch, 1, 7, 7, seed=145, scale=0.1), rnd(3 * Ch, seed=146)]
    crd = tuple(t.to(dev()) for t in crpe)
    y0 = ops.factor_att(qkv.to(dev()), crd, H, W, heads)
    q2 = qkv.clone(); q2[:, :, C:2 * C] += 300.0     # exp(300) overflows fp32 without max subtraction
    y1 = ops.factor_att(q2.to(dev()), crd, H, W, heads)
    assert torch.isfinite(y1).all()
    check(y1, y0, tol=2e-4, name="shift invariance")


def test_seg_losses(golden):
    from mdvit_amd import ops
    from oracle import mdvit_ref as R
    from oracle.gen_golden import synth_label, synth_tokens
    gd = golden("losses_small")
    o = synth_tokens(5, 1, (2, 1, 32, 32)) * 6.0
    a = synth_tokens(5, 2, (2, 1, 32, 32)) * 6.0
    o.view(-1)[:8] = torch.tensor([200.0, -200.0, 120.0, -120.0, 90.0, -90.0, 40.0, -40.0])
    lab = synth_label(5, 2, 32, 32)
    oh, ah = o.to(dev()).requires_grad_(True), a.to(dev()).requires_grad_(True)
    l = ops.seg_losses(oh, ah, lab.to(dev()))
    check(torch.stack(l).cpu(), torch.tensor(gd["losses"], dtype=torch.float32), tol=1e-5, name="losses vs golden")
    l[1].backward(retain_graph=True)
    assert oh.grad is None, "the aux sweep must not touch the main logits"
    check(ah.grad, torch.from_numpy(gd["d_aux_from_auxloss"]), tol=2e-4, name="d aux (aux sweep)")
    ah.grad = None; oh.grad = None
    (0.5 * l[2] + 0.5 * l[0]).backward()
    check(oh.grad, torch.from_numpy(gd["d_out_from_uni"]), tol=2e-4, name="d out (uni sweep)")
    check(ah.grad, torch.from_numpy(gd["d_aux_from_uni"]), tol=2e-4, name="d aux (uni sweep)")
    # BASE flavour (no aux)
    l0 = ops.seg_losses(o.to(dev()), None, lab.to(dev()))
    ref0 = R.bce_loss(torch.sigmoid(o.double()), lab.double()) + R.dice_loss(torch.sigmoid(o.double()), lab.double())
    assert abs(float(l0[0]) - float(ref0)) < 1e-5 * abs(float(ref0))


@pytest.mark.parametrize("G,partial", [(4, "full"), (4, "aux_only"), (2, "full")])
def test_seg_losses_of_the_domain_batches_in_one_launch_equal_one_op_per_domain(G, partial):
    """ops.seg_losses_groups(out, aux, label, G) (one sums / final / backward launch over the G domain batches of a domain-batched forward) == ops.seg_losses per domain
    batch, the losses added in batch order: the three losses bit for bit, the logit gradients bit for bit -- also when only loss_aux + kt are back-propagated (the
    aux sweep: the main logits then get their gradient through the KT term only)."""
    from mdvit_amd import ops
    torch.manual_seed(G)
    B, H = 3, 40
    out = (torch.randn(G * B, 1, H, H, device=dev()) * 2).requires_grad_(True)
    aux = (torch.randn(G * B, 1, H, H, device=dev()) * 2).requires_grad_(True)
    label = (torch.rand(G * B, 1, H, H, device=dev()) < 0.3).float()
    w = torch.tensor([0.7, 1.3, 0.5], device=dev())

    def total(ls):
        return w[1] * ls[1] + w[2] * ls[2] if partial == "aux_only" else w[0] * ls[0] + w[1] * ls[1] + w[2] * ls[2]

    lg = ops.seg_losses_groups(out, aux, label, G)
    go, ga = torch.autograd.grad(total(lg), (out, aux))
    per = [ops.seg_losses(out[g * B:(g + 1) * B], aux[g * B:(g + 1) * B], label[g * B:(g + 1) * B]) for g in range(G)]
    ref = []
    for j in range(3):
        t = per[0][j]
        for g in range(1, G):
            t = t + per[g][j]
        ref.append(t)
    ro, ra = torch.autograd.grad(total(ref), (out, aux))
    for a, b in zip(lg, ref):
        assert torch.equal(a, b), (float(a), float(b))
    assert torch.equal(go, ro) and torch.equal(ga, ra)
    assert torch.isfinite(go).all() and float(go.abs().max()) > 0


def test_seg_losses_global_batch_two_ranks_emulated():
    """Data-parallel loss semantics (nn.DataParallel: Dice / BCE over the gathered global batch): two 'ranks' on one GPU --
    each runs _sums on its half, the 16 doubles are added (the all-reduce), _final / _bwd use the global sums with
    n_total = 2n and dice_gain = 2.  Losses must equal the full-batch losses; the rank's logit gradients, divided by the
    world size (the gradient average), must equal the full-batch gradients of its half."""
    import ctypes as C
    from mdvit_amd import ops
    from mdvit_amd._lib import call
    from oracle.gen_golden import synth_label, synth_tokens
    o = (synth_tokens(7, 1, (4, 1, 32, 32)) * 4.0).to(dev())
    a = (synth_tokens(7, 2, (4, 1, 32, 32)) * 4.0).to(dev())
    lab = synth_label(7, 4, 32, 32).to(dev())
    of, af = o.clone().requires_grad_(True), a.clone().requires_grad_(True)
    lf = ops.seg_losses(of, af, lab)
    (lf[1] + 0.5 * lf[2] + 0.5 * lf[0]).backward()
    p, st = ops._p, ops._stream()
    halves = [(o[:2].contiguous(), a[:2].contiguous(), lab[:2].contiguous()), (o[2:].contiguous(), a[2:].contiguous(), lab[2:].contiguous())]
    n = halves[0][0].numel()
    sums = [torch.zeros(16, device=dev(), dtype=torch.float64) for _ in halves]
    for (oh, ah, lh), sm in zip(halves, sums):
        call("mdvit_seg_losses_sums", p(oh), p(ah), p(lh), p(sm), n, st)
    glob = sums[0] + sums[1]
    losses = torch.zeros(3, device=dev())
    call("mdvit_seg_losses_final", p(glob), p(losses), 2 * n, 1, st)
    check(losses, torch.stack(lf).detach(), tol=1e-6, name="global losses")
    g = torch.tensor([0.5, 1.0, 0.5], device=dev())
    for r, (oh, ah, lh) in enumerate(halves):
        do, da = torch.empty_like(oh), torch.empty_like(ah)
        call("mdvit_seg_losses_bwd", p(oh), p(ah), p(lh), p(glob), p(g), p(do), p(da), n, 2.0, st)
        check(do / 2, of.grad[2 * r:2 * r + 2], tol=1e-5, name=f"d out rank {r}")
        check(da / 2, af.grad[2 * r:2 * r + 2], tol=1e-5, name=f"d aux rank {r}")


def test_seg_metrics_counts_are_exact():
    """thresholded Dice / IoU on the device == medpy's dc / jc (restated in oracle/pipeline.py): integer counts bit-exact"""
    import numpy as np
    from mdvit_amd import ops
    from oracle import pipeline as P
    from oracle.gen_golden import synth_label, synth_tokens
    o = synth_tokens(11, 1, (3, 1, 40, 56)) * 3.0
    a = synth_tokens(11, 2, (3, 1, 40, 56)) * 3.0
    lab = synth_label(11, 3, 40, 56)
    m, c = ops.seg_metrics(o.to(dev()), a.to(dev()), lab.to(dev()))
    ob, ab, yb = torch.sigmoid(o).numpy() > 0.5, torch.sigmoid(a).numpy() > 0.5, lab.numpy().astype(bool)
    want = [np.count_nonzero(ob & yb), np.count_nonzero(ob), np.count_nonzero(yb), np.count_nonzero(ab & yb), np.count_nonzero(ab)]
    assert c[:5].tolist() == want
    ref = [P.dc(ob, yb), P.jc(ob, yb), P.dc(ab, yb), P.jc(ab, yb)]
    assert np.allclose(m.cpu().numpy(), np.array(ref, dtype=np.float32), rtol=1e-6, atol=0)
    d0, j0 = P.train_metrics(o, lab)
    assert abs(float(m[0]) - d0) < 1e-6 and abs(float(m[1]) - j0) < 1e-6
    m2, c2 = ops.seg_metrics(torch.full((1, 1, 8, 8), -5.0, device=dev()), None, torch.zeros(1, 1, 8, 8, device=dev()))
    assert m2.tolist() == [0.0, 0.0, 0.0, 0.0] and c2[:3].tolist() == [0, 0, 0]


def test_image_normalize_u8_bit_exact():
    """uint8 HWC -> normalised fp32 CHW on the device == the loader's norm01 + permute + Normalize sequence, bit for bit"""
    from mdvit_amd import ops
    from oracle import pipeline as P
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, 37, 53, 3), generator=g, dtype=torch.uint8)
    u8[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    got = ops.image_normalize_u8(u8.to(dev())).cpu()
    want = torch.stack([P.load_image(u8[b].numpy()) for b in range(2)])
    assert torch.equal(got, want)


def test_fused_adamw_matches_torch_adamw():
    """one-launch AdamW over the accumulator's buckets == torch.optim.AdamW (the reference's optimizer), 4 steps, odd sizes,
    a learning-rate change in between (StepLR), step counter and lr on the device"""
    from mdvit_amd.optim import FusedAdamW, StepLR
    from mdvit_amd.parallel import GradAccumulator
    shapes = [(64, 33), (7,), (320, 1, 3, 3), (1,), (513,), (128, 64)]
    ps = [torch.nn.Parameter(rnd(*sh, seed=200 + i).to(dev())) for i, sh in enumerate(shapes)]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    acc = GradAccumulator(ps, bucket_bytes=4096)
    opt = FusedAdamW(acc, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    ref = torch.optim.AdamW(qs, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    sch, rsch = StepLR(opt, step_size=2, gamma=0.5), torch.optim.lr_scheduler.StepLR(ref, step_size=2, gamma=0.5)
    for step in range(4):
        acc.zero()
        acc.begin_sweep(True)
        for i, (p, q) in enumerate(zip(ps, qs)):
            g = rnd(*p.shape, seed=300 + 10 * step + i).to(dev())
            p.grad = g.clone(); q.grad = g.clone()
        acc.end_sweep(True)                      # folds p.grad into the buckets, re-points p.grad at the bucket views
        opt.step(); ref.step()
        sch.step(); rsch.step()
        assert abs(sch.get_last_lr()[0] - rsch.get_last_lr()[0]) < 1e-12
    assert float(opt.step_dev[0]) == 4.0
    for i, (p, q) in enumerate(zip(ps, qs)):
        check(p.detach(), q.detach(), tol=2e-6, name=f"param {i} after 4 steps")


def test_abi_error_reporting():
    from mdvit_amd import ops, _lib
    x = torch.zeros(4, 6, device=dev())        # K = 6 is not a multiple of 4 -> MDVIT_E_ALIGN, not a crash
    W = torch.zeros(8, 6, device=dev())
    with pytest.raises(_lib.MdvitHipError, match="gemm"):
        ops.linear(x, W, None)
    with pytest.raises(_lib.MdvitHipError):
        ops.linear(torch.zeros(4, 8), torch.zeros(8, 8), None)      # CPU tensors: no CPU path


# ---- round 2: plane GEMMs (csrc/gemm_bp.hip) and the bf16 speed mode ------------------------------------------------------------
def test_plane_gemm_all_epilogues_vs_fp64():
    """mdvit_gemm_planes through the C ABI: every tile configuration x {plane A, fp32 A} x {fp32 / plane output, GELU (+u), DropPath +
    residual, gelu' with u read or recomputed, split-K + accumulate, one-plane bf16} against fp64 (tools/gemm_bp_check.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemm_bp_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_bp_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.correctness()


def test_phase_split_256_tile_is_the_128_tile_bit_for_bit_in_every_epilogue():
    """csrc/gemm_ph.hip (round 4: 256 x 256 tile, eight phase-split waves, global_load_lds ring with counted waits) through mdvit_gemm_planes with the plan
    forced: plane A and fp32 A (split while staged through hidden asm loads), one and two planes, ragged M / N, K from two tiles up, every epilogue
    (bias, GELU + u + dropout, DropPath + residual + dropout, gelu' x u, plane output, split-K + accumulate) -- against fp64 AND bit for bit against the
    128 x 128 plane tile; 20 repeats of every shape must agree bit for bit (a race in the hand-counted vmcnt / barrier protocol shows up as rare wrong tiles)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemm_ph_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_ph_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.correctness([3])


def test_phase_split_128_row_tile_is_the_128_tile_bit_for_bit_in_every_epilogue():
    """csrc/gemm_pm.hip (round 5: 128 x 160 / 128 x 128 tile, eight waves of unequal work on equal SIMDs, four-stage ring, the in-flight fp32 A rows in fixed registers)
    through mdvit_gemm_planes with the plan forced: fp32 A against two weight planes, ragged M / N, K from ONE tile up, every epilogue (bias, accumulate, GELU + u +
    dropout, DropPath + residual + dropout, gelu' x u) -- bit for bit against the 128 x 128 plane tile and against fp64; 20 repeats of every shape must agree bit for
    bit (the first build of this kernel read registers whose loads had not landed: results changed from run to run).  tools/gemm_pm_check.py"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemm_pm_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_pm_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.correctness()


def test_mid_size_products_take_the_128_row_tile_and_equal_the_split_while_staging_kernel_bit_for_bit():
    """mdvit_gemm_pm_prefers: the rule's two sides at the step's shapes; ops.linear on a shape it takes (16384 x 320 x 1280: fc2 of stage 2 at 16 images) runs
    gemm_pm_kernel and equals gemm.hip's forward, data gradient and weight gradient bit for bit (MDVIT_PM_GEMM / mdvit_gemm_pm_config(-1) switch it off)."""
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    assert lib.mdvit_gemm_pm_prefers(16384, 320, 1280, 2, 1) == 6 and lib.mdvit_gemm_pm_prefers(16384, 320, 320, 2, 1) == 6 and lib.mdvit_gemm_pm_prefers(8192, 512, 2048, 2, 1) == 7
    assert lib.mdvit_gemm_pm_prefers(16384, 1280, 320, 2, 1) == 0 and lib.mdvit_gemm_pm_prefers(4096, 512, 2048, 2, 1) == 0 and lib.mdvit_gemm_pm_prefers(16384, 320, 1280, 1, 1) == 0
    assert lib.mdvit_gemm_pm_prefers(16384, 320, 1280, 2, 0) == 0 and lib.mdvit_gemm_pm_prefers(16384, 324, 1280, 2, 1) == 0
    M, N, K = 16384, 320, 1280
    x, W, b, g = rnd(M, K, seed=1).to(dev()), rnd(N, K, seed=2, scale=K ** -0.5).to(dev()), rnd(N, seed=3).to(dev()), rnd(M, N, seed=4).to(dev())
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16x3")
    try:
        res = {}
        for mode in (0, -1):
            lib.mdvit_gemm_pm_config(mode); ops._ph_cache.clear()
            ops.kernel_events_begin()
            out, go = grads_of(lambda x, W, b: ops.linear(x, W, b), [x, W, b], g)
            names = list(ops.kernel_events_end())
            res[mode] = (out, go, names)
    finally:
        lib.mdvit_gemm_pm_config(0); ops._ph_cache.clear()
        ops.set_gemm_precision(prev)
    assert any(n.startswith("gemm_pm_kernel<3, 2") for n in res[0][2]), res[0][2]
    assert not any(n.startswith("gemm_pm_kernel") for n in res[-1][2]), res[-1][2]
    assert torch.equal(res[0][0], res[-1][0])
    for a, r in zip(res[0][1], res[-1][1]):
        assert torch.equal(a, r)


def test_few_tile_long_k_data_gradients_run_the_128_row_tile_over_k_ranges():
    """mdvit_gemm_pm_splits: a plain product whose 128-row tiles alone would leave most of the chip idle (the stage-3 data gradients at 16 images: 4096 x 512 x 1536 /
    2048) runs gemm_pm_kernel over 2 K ranges + the split-K reduction.  Per K range the kernel is the 128 x 128 plane tile bit for bit, the slabs are added in split
    order by the same reduction kernel: the result equals that tile forced to the same split bit for bit (and the unsplit product to round-off); the rule leaves
    short K, many-tile and epilogue-carrying products alone; ops._dgrad takes the route and MDVIT_PM_GEMM=0 / mdvit_gemm_pm_config(-1) switches it off."""
    from mdvit_amd import _lib, ops
    from mdvit_amd._lib import call
    lib = _lib.load()
    assert lib.mdvit_gemm_pm_splits(4096, 512, 2048, 2, 1) == 2 and lib.mdvit_gemm_pm_splits(4000, 512, 2048, 2, 1) == 2 and lib.mdvit_gemm_pm_splits(2048, 512, 4096, 2, 1) == 4
    assert lib.mdvit_gemm_pm_splits(4096, 512, 1536, 2, 1) == 1 and lib.mdvit_gemm_pm_splits(2048, 512, 2048, 2, 1) == 1         # ranges under 1024 lose to gemm.hip (measured)
    assert lib.mdvit_gemm_pm_splits(4096, 512, 512, 2, 1) == 1 and lib.mdvit_gemm_pm_splits(16384, 512, 2048, 2, 1) == 1 and lib.mdvit_gemm_pm_splits(4096, 512, 2048, 1, 1) == 1
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16x3")
    try:
        for (M, N, K) in ((4096, 512, 2048), (2048, 512, 4096), (4000, 512, 2048)):
            g, W = rnd(M, K, seed=11).to(dev()), rnd(K, N, seed=12, scale=K ** -0.5).to(dev())          # dx[M, N] = g[M, K] W[K, N]: the NT product against W^T's planes
            ref64 = (g.double() @ W.double())
            outs = {}
            sp_rule = lib.mdvit_gemm_pm_splits(M, N, K, 2, 1)
            for tag, cfg, sp in (("pm split", 7, sp_rule), ("128x128 split", 0, sp_rule), ("planner", -1, 0)):
                call("mdvit_gemm_planes_force_plan", cfg, sp)
                ops._plan_cache.clear()          # (the event names come from the cached plan of a shape)
                try:
                    dx = torch.full((M, N), float("nan"), device=dev())
                    ops.kernel_events_begin()
                    ops.gemm_nt(g, W, dx, M, N, K, w_transposed=True, allow_split=True)
                    names = list(ops.kernel_events_end())
                finally:
                    call("mdvit_gemm_planes_force_plan", -1, 0)
                outs[tag] = (dx, names)
            assert torch.equal(outs["pm split"][0], outs["128x128 split"][0]), (M, N, K)
            assert torch.equal(outs["planner"][0], outs["pm split"][0]), (M, N, K)              # the planner's own choice IS the two-range pm launch
            assert any(n.startswith("gemm_pm_kernel<2, 2, 0>+splitk_reduce") for n in outs["planner"][1]), outs["planner"][1]
            err = float((outs["planner"][0].double() - ref64).abs().max() / ref64.abs().max())
            assert err < 2e-5, err
            for _ in range(5):                                                                   # race screen
                dx2 = torch.full((M, N), float("nan"), device=dev())
                ops.gemm_nt(g, W, dx2, M, N, K, w_transposed=True, allow_split=True)
                assert torch.equal(dx2, outs["planner"][0])
        # the data-gradient route of ops (what the operator path and, through the same predicates, the C-level block take)
        M, N, K = 4096, 2048, 512          # Linear(512 -> 2048): dx = g[M, 2048] W[2048, 512]
        x, Wl, g = rnd(M, K, seed=21).to(dev()), rnd(N, K, seed=22, scale=K ** -0.5).to(dev()), rnd(M, N, seed=23).to(dev())
        res = {}
        for mode in (0, -1):
            lib.mdvit_gemm_pm_config(mode); ops._ph_cache.clear()
            ops.kernel_events_begin()
            out, go = grads_of(lambda x, W: ops.linear(x, W, None), [x, Wl], g)
            res[mode] = (out, go, list(ops.kernel_events_end()))
    finally:
        lib.mdvit_gemm_pm_config(0); ops._ph_cache.clear()
        ops.set_gemm_precision(prev)
    assert any(n.startswith("gemm_pm_kernel<2, 2, 0>+splitk_reduce") for n in res[0][2]), res[0][2]
    assert not any(n.startswith("gemm_pm_kernel") for n in res[-1][2]), res[-1][2]
    assert torch.equal(res[0][0], res[-1][0]) and torch.equal(res[0][1][1], res[-1][1][1])          # forward and weight gradient: untouched
    dxa, dxb = res[0][1][0], res[-1][1][0]
    assert float((dxa - dxb).abs().max()) <= 2e-6 * float(dxb.abs().max())                            # the data gradient: another summation order


def test_linear_on_the_256_tile_equals_the_split_while_staging_kernel_bit_for_bit():
    """ops.linear routes the products mdvit_gemm_ph_prefers accepts to the 256-wide plane kernel (MDVIT_PH_GEMM); forward, data gradient and the fused
    FULL epilogue equal gemm.hip's results bit for bit (same products, same order), so a block may mix the two freely."""
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    M, N, K = 8192, 1536, 512
    assert lib.mdvit_gemm_ph_prefers(M, N, K, 2) == 1 and lib.mdvit_gemm_ph_prefers(4096, 2048, 512, 2) == 0 and lib.mdvit_gemm_ph_prefers(M, N, 32, 2) == 0
    x, W, b, g = rnd(M, K, seed=1).to(dev()), rnd(N, K, seed=2, scale=K ** -0.5).to(dev()), rnd(N, seed=3).to(dev()), rnd(M, N, seed=4).to(dev())
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16x3")
    try:
        res = {}
        for mode in (0, -1):
            lib.mdvit_gemm_ph_config(mode); ops._ph_cache.clear()
            ops.kernel_events_begin()
            out, go = grads_of(lambda x, W, b: ops.linear(x, W, b), [x, W, b], g)
            names = list(ops.kernel_events_end())
            res[mode] = (out, go, names)
    finally:
        lib.mdvit_gemm_ph_config(0); ops._ph_cache.clear()
        ops.set_gemm_precision(prev)
    assert any(n.startswith("gemm_ph_kernel<2, true") for n in res[0][2]), res[0][2]
    assert not any(n.startswith("gemm_ph_kernel") or n.startswith("gemm_bp_nt_kernel") for n in res[-1][2]), res[-1][2]
    assert torch.equal(res[0][0], res[-1][0])
    for a, r in zip(res[0][1], res[-1][1]):
        assert torch.equal(a, r)
    ref, gr = grads_of(lambda x, W, b: F.linear(x.double(), W.double(), b.double()), [x.cpu(), W.cpu(), b.cpu()], g.cpu().double())
    check(res[0][0], ref, tol=1e-4, name="y")


def test_weight_plane_cache_follows_updates_and_the_optimizer_epoch():
    """the cached weight planes (W and W^T) are rebuilt when the parameter's version moves, and when an optimizer that writes
    through raw pointers says so (ops.mark_weights_updated: FusedAdamW.step does)"""
    from mdvit_amd import ops
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16x3")
    try:
        W = torch.nn.Parameter(rnd(96, 64, seed=9).to(dev()))

        def joined(t):
            return t.float().sum(0)
        p1, pt1 = ops._wplanes(W, False), ops._wplanes(W, True)
        assert p1.shape == (2, 96, 64) and pt1.shape == (2, 64, 96)
        assert float((joined(p1) - W.detach()).abs().max()) <= 2e-5 * float(W.abs().max())
        assert torch.equal(joined(pt1), joined(p1).t())
        assert ops._wplanes(W, False) is p1                     # cached while unchanged
        with torch.no_grad():
            W.add_(1.0)                                         # version bump (a torch optimizer)
        p2 = ops._wplanes(W, False); ops._wplanes(W, True)
        assert p2 is p1 and float((joined(p2) - W.detach()).abs().max()) <= 2e-5 * float(W.abs().max())
        W.data.mul_(0.5)                                        # a write the version counter does not see (as a kernel writing through data_ptr) ...
        ver = W._version
        assert W._version == ver and float((joined(ops._wplanes(W, True)).t() - W.detach()).abs().max()) > 0.1      # ... stale planes are still served
        ops.mark_weights_updated()                              # ... until the writer says so
        assert float((joined(ops._wplanes(W, True)).t() - W.detach()).abs().max()) <= 2e-5 * float(W.abs().max())
        ops.refresh_weight_planes()                             # the one-launch refresh of every cached orientation
        assert float((joined(ops._wplanes(W, False)) - W.detach()).abs().max()) <= 2e-5 * float(W.abs().max())
    finally:
        ops.set_gemm_precision(prev)


@pytest.mark.parametrize("M,N,K", [(1000, 192, 64), (4096, 64, 512), (300, 1280, 320)])
def test_linear_and_mlp_bf16_speed_mode(M, N, K):
    """--precision bf16: operands rounded to one bf16 plane, one MFMA per product, fp32 accumulate.  Error class 2^-9 per operand:
    checked at 2e-2 of the tensor max against fp64 (forward, dgrad, wgrad, MLP), and the one-plane kernel really ran."""
    from mdvit_amd import ops
    x, W, b, g = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref, gr = grads_of(lambda x, W, b: F.linear(x.double(), W.double(), b.double()), [x, W, b], g.double())
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16")
    try:
        out, go = grads_of(lambda x, W, b: ops.linear(x, W, b), [x.to(dev()), W.to(dev()), b.to(dev())], g)
        ops.kernel_events_begin()
        ops.linear(x.to(dev()), W.to(dev()), b.to(dev()))
        names = list(ops.kernel_events_end())
    finally:
        ops.set_gemm_precision(prev)
    assert names and all(n.startswith("gemm_bp_nt_kernel") and n.split(",")[2].strip() == "1" for n in names), names
    check(out, ref, tol=2e-2, name="y")
    for n, a, r in zip(("dx", "dW", "db"), go, gr):
        check(a, r, tol=2e-2, name=n)


# ---- round 2: the transposing-LDS-read weight-gradient kernel (csrc/gemm_tn.hip) ------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64, 1000), (320, 192, 4100), (128, 128, 777), (1280, 320, 2048), (192, 64, 33), (64, 512, 5000),
                                   (512, 64, 8192), (100, 36, 515), (512, 2048, 8), (4, 64, 300)])
def test_wgrad_tn_kernel_every_tile_and_split_vs_fp64_and_bitwise_repeatable(shape):
    """grad_out.t() @ input (TN layout, tokens on the long axis) on gemm_tn.hip: every tile config x forced K-split, ragged M / N / K,
    accumulate into a non-zero C, the bias gradient (column sums of A) riding on the same pass; results are bitwise repeatable
    (slab split-K and the column sums are reduced in a fixed order) and equal the general template's to rounding."""
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    M, N, K = shape
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M), generator=g).to(dev()); B = torch.randn((K, N), generator=g).to(dev())
    out0 = torch.randn((M, N), generator=g).to(dev()); cs0 = torch.randn((M,), generator=g).to(dev())
    ref = out0.double() + A.double().t() @ B.double()
    cref = cs0.double() + A.double().sum(0)

    def run():
        out, cs = out0.clone(), cs0.clone()
        ops.gemm(ops._p(A), ops._p(B), ops._p(out), M, N, K, lda=M, ldb=N, ldc=N, trans_a=True, trans_b=False, allow_split=True,
                 accumulate=True, precision=1, colsum_a=ops._p(cs))
        return out, cs
    try:
        for cfg in (-1, 0, 1, 2, 3):
            for sp in (0, 1, 3):
                lib.mdvit_gemm_tn_config(1, cfg, sp)
                out, cs = run()
                check(out, ref.float(), tol=2e-5, name=f"cfg {cfg} splits {sp}")
                check(cs, cref.float(), tol=1e-5, name=f"colsum cfg {cfg} splits {sp}")
                out2, cs2 = run()
                assert torch.equal(out, out2) and torch.equal(cs, cs2), f"cfg {cfg} splits {sp}: not bitwise repeatable"
        lib.mdvit_gemm_tn_config(0, -1, 0)                  # the general template
        old, cso = run()
        lib.mdvit_gemm_tn_config(1, -1, 0)
        new, csn = run()
        check(new, old, tol=2e-5, name="vs the general template"); check(csn, cso, tol=1e-5, name="colsum vs the general template")
    finally:
        lib.mdvit_gemm_tn_config(1, -1, 0)


@pytest.mark.parametrize("shape", [(192, 64, 8192), (1024, 128, 4096), (64, 512, 5000), (320, 320, 3000), (512, 512, 4096), (100, 36, 2050)])
def test_wgrad_tn_workgroup_order_over_the_xcds_does_not_change_a_bit(shape):
    """mdvit_gemm_tn_grid_order: the logical (K-split, tile) pair of a workgroup taken from the XCD-contiguous order of the whole grid (the tiles of a split
    share one L2) or from the order inside a split -- the same tiles, the same slab reduction order: C and the column sums are identical to the last bit,
    with the planner's splits and with forced ones (ragged last split included)."""
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    M, N, K = shape
    g = torch.Generator(device="cpu").manual_seed(M + 5 * N + K)
    A = torch.randn((K, M), generator=g).to(dev()); B = torch.randn((K, N), generator=g).to(dev())
    out0 = torch.randn((M, N), generator=g).to(dev()); cs0 = torch.randn((M,), generator=g).to(dev())

    def run():
        out, cs = out0.clone(), cs0.clone()
        ops.gemm(ops._p(A), ops._p(B), ops._p(out), M, N, K, lda=M, ldb=N, ldc=N, trans_a=True, trans_b=False, allow_split=True,
                 accumulate=True, precision=1, colsum_a=ops._p(cs))
        return out, cs
    try:
        for sp in (0, 5, 16):
            lib.mdvit_gemm_tn_config(1, -1, sp)
            res = []
            for mode in (0, 2, 1):
                lib.mdvit_gemm_tn_grid_order(mode)
                res.append(run())
            for (o, c), mode in zip(res[1:], (2, 1)):
                assert torch.equal(o, res[0][0]) and torch.equal(c, res[0][1]), f"splits {sp}: grid order {mode} differs from order 0"
        ref = out0.double() + A.double().t() @ B.double()
        check(res[0][0], ref.float(), tol=2e-5, name="vs fp64")
    finally:
        lib.mdvit_gemm_tn_config(1, -1, 0)
        lib.mdvit_gemm_tn_grid_order(-1)


@pytest.mark.parametrize("shape", [(1024, 128, 4096), (128, 1024, 3000), (64, 64, 777), (320, 192, 2050)])
@pytest.mark.parametrize("which", ["a", "b"])
def test_wgrad_tn_kernel_with_a_bf16_stored_operand(shape, which):
    """MdvitGemmDesc.a_bf16 / b_bf16: one operand of the weight-gradient product lives in HBM as bf16 (the mixed mode's saved hidden activations).  It is
    EXACTLY its single bf16 plane, so against fp64 on the same (rounded) values the product keeps the bf16x3 accuracy; the column sums of a bf16 A are the
    sums of the rounded values; every tile config and forced split, repeatable to the bit."""
    import ctypes as C
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    M, N, K = shape
    g = torch.Generator(device="cpu").manual_seed(M + 3 * N + K)
    A = torch.randn((K, M), generator=g).to(dev()); B = torch.randn((K, N), generator=g).to(dev())
    Ab, Bb = A.to(torch.bfloat16), B.to(torch.bfloat16)
    Aeff, Beff = (Ab.float(), B) if which == "a" else (A, Bb.float())
    out0 = torch.randn((M, N), generator=g).to(dev()); cs0 = torch.randn((M,), generator=g).to(dev())
    ref = out0.double() + Aeff.double().t() @ Beff.double()
    cref = cs0.double() + Aeff.double().sum(0)

    def run():
        out, cs = out0.clone(), cs0.clone()
        d = _lib.GemmDesc()
        d.A, d.B, d.C = ops._p(Ab if which == "a" else A), ops._p(Bb if which == "b" else B), ops._p(out)
        d.lda, d.ldb, d.ldc = M, N, N
        d.M, d.N, d.K = M, N, K
        d.trans_a, d.trans_b, d.allow_split, d.accumulate, d.precision = 1, 0, 1, 1, 1
        d.colsum_a = ops._p(cs)
        d.a_bf16, d.b_bf16 = int(which == "a"), int(which == "b")
        need = lib.mdvit_gemm_ws_bytes(C.byref(d))
        ws = torch.empty((max(need // 4, 1),), device=dev())
        d.ws, d.ws_bytes = ops._p(ws), need
        ops.call("mdvit_gemm_f32", C.byref(d), ops._stream())
        torch.cuda.synchronize()
        return out, cs
    try:
        for cfg in (-1, 0, 1, 2, 3):
            for sp in (0, 1, 5):
                lib.mdvit_gemm_tn_config(1, cfg, sp)
                out, cs = run()
                check(out, ref.float(), tol=2e-5, name=f"{which} bf16, cfg {cfg} splits {sp}")
                check(cs, cref.float(), tol=1e-5, name=f"colsum, {which} bf16, cfg {cfg} splits {sp}")
                out2, cs2 = run()
                assert torch.equal(out, out2) and torch.equal(cs, cs2)
    finally:
        lib.mdvit_gemm_tn_config(1, -1, 0)


def test_wgrad_tn_kernel_strided_operands_and_single_plane():
    """operands that are column blocks of wider tensors (lda > M, ldb > N), overwrite (no accumulate), and the one-bf16-plane mode"""
    from mdvit_amd import ops
    K, M, N = 3000, 128, 64
    Aw = torch.randn((K, 384), device=dev()); Bw = torch.randn((K, 256), device=dev())
    ref = Aw[:, 128:256].double().t() @ Bw[:, 64:128].double()
    for precision, tol in ((1, 2e-5), (2, 2e-2)):
        out = torch.full((M, N), float("nan"), device=dev())
        ops.gemm(ops._p(Aw[:, 128:256]), ops._p(Bw[:, 64:128]), ops._p(out), M, N, K, lda=384, ldb=256, ldc=N, trans_a=True, trans_b=False,
                 allow_split=True, precision=precision)
        check(out, ref.float(), tol=tol, name=f"precision {precision}")
    out = torch.full((M, N), float("nan"), device=dev())                # no workspace allowed: one slab, written directly
    ops.gemm(ops._p(Aw[:, 128:256]), ops._p(Bw[:, 64:128]), ops._p(out), M, N, K, lda=384, ldb=256, ldc=N, trans_a=True, trans_b=False, allow_split=False)
    check(out, ref.float(), tol=2e-5, name="allow_split=False")


def test_armed_gemm_launch_records_its_own_begin_and_end():
    """mdvit_timing_arm (bench.py's roofline timer): the NEXT GEMM launch -- and only that one -- writes its own begin / end timestamps
    into the two library events; the result of an armed launch is the result of a plain one; the event-sampled table of ops names the
    kernel and counts every launch."""
    import ctypes as C
    from mdvit_amd import _lib, ops
    M, N, K = 4096, 320, 512
    x, W = rnd(M, K, seed=5).to(dev()), rnd(N, K, seed=6).to(dev())
    y0, y1 = torch.empty((M, N), device=dev()), torch.empty((M, N), device=dev())
    ops.gemm(ops._p(x), ops._p(W), ops._p(y0), M, N, K, lda=K, ldb=K, ldc=N)
    h0, h1 = C.c_void_p(), C.c_void_p()
    _lib.call("mdvit_event_create", C.byref(h0)); _lib.call("mdvit_event_create", C.byref(h1))
    try:
        _lib.call("mdvit_timing_arm", h0.value, h1.value)
        ops.gemm(ops._p(x), ops._p(W), ops._p(y1), M, N, K, lda=K, ldb=K, ldc=N)
        ops.gemm(ops._p(x), ops._p(W), ops._p(y0), M, N, K, lda=K, ldb=K, ldc=N)       # not armed any more
        torch.cuda.synchronize()
        ms = C.c_float(-1.0)
        _lib.call("mdvit_event_elapsed_ms", h0.value, h1.value, C.byref(ms))
        assert 1e-3 < ms.value < 5.0, ms.value                   # one 1.3 GFLOP launch: microseconds, not the three of them, not zero
        assert torch.equal(y0, y1)
        with pytest.raises(_lib.MdvitHipError):
            _lib.call("mdvit_event_elapsed_ms", None, h1.value, C.byref(ms))
    finally:
        _lib.call("mdvit_timing_arm", None, None)
        _lib.call("mdvit_event_destroy", h0.value); _lib.call("mdvit_event_destroy", h1.value)
    ops.kernel_events_begin(stride=2)
    for _ in range(8):
        ops.gemm(ops._p(x), ops._p(W), ops._p(y1), M, N, K, lda=K, ldb=K, ldc=N)
    t = ops.kernel_events_end()
    assert len(t) == 1
    (name, rec), = t.items()
    assert name.startswith("gemm_f32_kernel<") and rec["launches"] == 8 and 1 <= rec["n"] <= 8 and rec["ms"] > 0
    assert rec["timer"].startswith("kernel begin/end") and rec["flop"] == rec["n"] * 2.0 * M * N * K


def test_upsample_multi_with_a_factor_of_three_takes_the_flat_kernel():
    """the LDS-tiled resize-and-sum sizes its source-patch pool with tile / factor + 2 rows per axis, which holds for power-of-two factors only -- three factor-3
    sources (Ho = 48 from 16) would stage 105 pixels into a 96-pixel pool.  Such shapes now go to the flat kernel; the result must equal torch's bilinear resize."""
    from mdvit_amd import ops
    B, Ho, C = 2, 48, 128
    xs = [rnd(B, 16, 16, C, seed=900 + i).to(dev()) for i in range(3)]
    base = rnd(B, Ho, Ho, C, seed=910).to(dev())
    got = ops.upsample_sum(base, xs, Ho, Ho)
    ref = base.double()
    for x in xs:
        ref = ref + F.interpolate(x.double().permute(0, 3, 1, 2), size=(Ho, Ho), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    check(got, ref, tol=2e-6, name="upsample_sum, factor 3")


@pytest.mark.parametrize("C,r,M", [(64, 8, 4173), (128, 8, 1031)])
def test_mlp_register_chained_kernels_on_one_plane_in_the_bf16_mode(C, r, M):
    """The bf16 speed mode runs the register-chained MLP kernels (mlp_rc.hip) on ONE bf16 plane per operand (mdvit_mlp_rc_planes(1), set by ops.set_gemm_precision("bf16")):
    forward and every gradient against an fp64 restatement of mpvit.py:71-78 within the bf16 class (2e-2 of the tensor's maximum; the parity mode holds 3e-4), nothing like
    the parity mode's bits (the switch really switches), and the parity arithmetic is back afterwards."""
    from mdvit_amd import ops
    Hd = C * r
    ins = [rnd(M, C, seed=420), rnd(M, C, seed=421), rnd(Hd, C, seed=422, scale=C ** -0.5), rnd(Hd, seed=423, scale=0.1), rnd(C, Hd, seed=424, scale=Hd ** -0.5), rnd(C, seed=425, scale=0.1)]
    g = rnd(M, C, seed=426)

    def ref_fn(x, res_, W1, b1, W2, b2):
        return res_.double() + F.linear(F.gelu(F.linear(x.double(), W1.double(), b1.double())), W2.double(), b2.double())
    ref, gr = grads_of(ref_fn, ins, g.double())
    prev = ops.gemm_precision()
    res = {}
    try:
        for mode in ("bf16x3", "bf16"):
            ops.set_gemm_precision(mode)
            out, go = grads_of(lambda *a: ops.mlp_residual(*a), [t.to(dev()) for t in ins], g)
            res[mode] = [out.detach()] + go
    finally:
        ops.set_gemm_precision(prev)
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res["bf16"], [ref] + gr):
        check(a, b, tol=2e-2, name=name + " (one plane) vs fp64")
    for name, a, b in zip(("y", "dx", "dres", "dW1", "db1", "dW2", "db2"), res["bf16x3"], [ref] + gr):
        check(a, b, tol=3e-4, name=name + " (bf16x3 afterwards / before) vs fp64")
    assert not torch.equal(res["bf16"][0], res["bf16x3"][0]) and float((res["bf16"][0] - res["bf16x3"][0]).abs().max()) > 1e-4


def test_launch_sampler_times_the_launches_of_one_symbol_from_every_site():
    """mdvit_gemm_sampler (round 6): every launch of a symbol is SEEN, a hashed 1-in-stride sample of them is TIMED with the kernel's own begin / end timestamps, other
    symbols are ignored; what bench.py's roofline line divides by"""
    import ctypes as C
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    M, N, K = 4096, 128, 256
    x, w = rnd(M, K, seed=901).to(dev()), rnd(N, K, seed=902).to(dev())
    g = rnd(M, N, seed=903).to(dev())
    out, dW = torch.empty(M, N, device=dev()), torch.empty(N, K, device=dev())

    def nt():
        ops.gemm(ops._p(x), ops._p(w), ops._p(out), M, N, K, lda=K, ldb=K, ldc=N, precision=1)

    def tn():
        ops.gemm(ops._p(g), ops._p(x), ops._p(dW), N, K, M, lda=N, ldb=K, ldc=K, trans_a=True, trans_b=False, allow_split=True, precision=1)

    def read():
        rows, i = {}, 0
        nm, seen, timed, ms = C.create_string_buffer(160), C.c_int64(), C.c_int64(), C.c_double()
        while lib.mdvit_gemm_sampler_read(i, nm, 160, C.byref(seen), C.byref(timed), C.byref(ms)) == 0:
            rows[nm.value.decode()] = (seen.value, timed.value, ms.value)
            i += 1
        return rows

    lib.mdvit_gemm_sampler(None, 1)
    for _ in range(6):
        nt(); tn()
    rows = read()
    assert len(rows) == 2 and all(v[0] == 6 and v[1] == 6 and 0.0 < v[2] < 50.0 for v in rows.values()), rows
    tn_name = next(k for k in rows if k.startswith("gemm_tn_kernel"))
    lib.mdvit_gemm_sampler(tn_name.encode(), 4)
    for _ in range(32):
        nt(); tn()
    rows = read()
    assert list(rows) == [tn_name] and rows[tn_name][0] == 32 and 2 <= rows[tn_name][1] <= 16 and rows[tn_name][2] > 0.0, rows
    nt(); tn()                      # reading ended the sampling: nothing is armed any more
    assert read() == rows
    torch.cuda.synchronize()


def test_the_chained_head_products_and_operator_level_deit_blocks_still_hold():
    """The forms round 6 replaced that are still reachable as A/B switches (read once per process): the peer heads' two chained products (MDVIT_HEAD_CAT=0) and the DeiT blocks
    through the operator-level entry points (MDVIT_DEIT_BLOCK_ENTRY=0) -- run the tests that pin them in a child process with the switches off, so that an A/B run compares
    two CORRECT paths.  (The attention core's superseded kernel forms and their switches are removed: nothing of them is left to keep alive.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MDVIT_HEAD_CAT="0", MDVIT_DEIT_BLOCK_ENTRY="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(root, "tests", "test_gpu_kernels.py"), "-k", "factor_att_core or factor_att_softmax",
                        os.path.join(root, "tests", "test_gpu_model.py") + "::test_mdvit_two_sweep_step_vs_golden"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
