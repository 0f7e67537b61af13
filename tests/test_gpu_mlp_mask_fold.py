"""The row-mask prologue of the fused MLP backward kernels (csrc/mlp_rc.hip, the mdvit_mlp_rc*_masked entries; switch mdvit_mlp_mask_config /
MDVIT_MLP_MASK_FOLD): a kernel that takes the UNMASKED upstream gradient g and forms gm = g * dropout mask * DropPath row scale where it loads the
rows, against the two-pass form of the same build -- mdvit_colsum_f32(g -> gm) followed by the plain entry on gm.  The operand is formed by the same
expression in the same order, so every comparison is BIT EQUALITY.

Shapes: 37 tokens (one wave's 32 + a ragged tail, and less than one 16-token workgroup of 128), 256, and 32 x 9 + 5 = 293 (several workgroups and a
tail); rows_per_scale = 48 puts a row-scale boundary inside a wave's 32 tokens."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOKENS = (37, 256, 32 * 9 + 5)
RPS = 48
SENTINEL = -7.25
# (mask drop_p, row scale?): both, dropout alone, row scale alone, neither (the descriptor is empty: the plain entry on g)
MASKS = ((0.1, True), (0.1, False), (0.0, True), (0.0, False))
KEY1, KEY2 = (3, 4), (5, 6)            # the hidden layer's dropout keys, the mask's keys
DROP1 = 0.1


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev())


def planes(W, transposed=0):
    from mdvit_amd.ops import call, _p, _stream
    N, K = W.shape
    out = torch.empty((2, K, N) if transposed else (2, N, K), device=dev(), dtype=torch.bfloat16)
    call("mdvit_split_planes_t", _p(W), K, _p(out), N if transposed else K, N * K, N, K, transposed, 2, _stream())
    return out


@functools.lru_cache(maxsize=None)
def operands(C, Hd):
    """weights (and their bf16 planes), the largest x / g, a row scale with a dropped sample, a device seed: made once, never written"""
    M = max(TOKENS)
    W1, b1, W2 = rnd(Hd, C, seed=1, scale=C ** -0.5), rnd(Hd, seed=2, scale=0.1), rnd(C, Hd, seed=3, scale=Hd ** -0.5)
    x, g = rnd(M, C, seed=4), rnd(M, C, seed=5)
    rs = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9, 1.0 / 0.9, 0.0, 1.0 / 0.9, 1.0 / 0.9][:(M + RPS - 1) // RPS], device=dev())
    seed = torch.tensor([0x1234567, 0x89abcd], dtype=torch.int32, device=dev())
    return dict(W1p=planes(W1), W2tp=planes(W2, 1), W1tp=planes(W1, 1), b1=b1, x=x, g=g, rs=rs, seed=seed)


def mask_pass(o, M, C, mp, rowscale, seed):
    """gm of the two-pass form: chan_reduce_kernel<2> through mdvit_colsum_f32 (no column sums wanted)"""
    from mdvit_amd.ops import call, _p, _stream
    g = o["g"][:M].contiguous()
    if not (mp > 0 or rowscale):
        return g, g
    gm = torch.empty_like(g)
    call("mdvit_colsum_f32", _p(g), C, None, _p(gm), None, 0, M, C, mp, KEY2[0], KEY2[1], _p(o["rs"]) if rowscale else None, RPS, 0,
         _p(seed) if mp > 0 else None, _stream())
    assert not torch.equal(g, gm), "the mask pass left g as it was: the comparison would say nothing"
    return g, gm


def cases():
    for M, (mp, rowscale), with_seed in itertools.product(TOKENS, MASKS, (False, True)):
        yield M, mp, rowscale, with_seed


@pytest.fixture(params=[2, 1], ids=["two_planes", "one_plane"])
def rc_planes(request):
    from mdvit_amd import ops
    assert ops.gemm_precision() == "bf16x3"
    ops.call("mdvit_mlp_rc_planes", request.param)
    yield request.param
    ops.set_gemm_precision(ops.gemm_precision())          # restores the plane count of the arithmetic mode


@pytest.mark.parametrize("Hd", [256, 512])
def test_c64_masked_kernels_equal_mask_pass_plus_kernel(Hd, rc_planes):
    """mdvit_mlp_rc_dgrad (dx), mdvit_mlp_rc_bwd (dx parts, dW1, db1, dW2) and mdvit_mlp_rc_wgrad (dW1, db1, dW2) at C = 64, one and two 256-wide hidden roles;
    and the masked fused backward twice: identical bits"""
    from mdvit_amd import _lib
    from mdvit_amd.ops import call, _p, _stream
    C = 64
    o = operands(C, Hd)
    d = dev()
    roles = Hd // 256
    for M, mp, rowscale, with_seed in cases():
        tag = f"M={M} mask_p={mp} rowscale={rowscale} seed={with_seed}"
        seed = o["seed"] if with_seed else None
        x = o["x"][:M].contiguous()
        g, gm = mask_pass(o, M, C, mp, rowscale, seed)
        mk = (mp, KEY2[0], KEY2[1], _p(seed), _p(o["rs"]) if rowscale else None, RPS)
        common = (_p(x), _p(o["W1p"]), _p(o["b1"]), _p(o["W2tp"]))
        # data gradient
        dx0, dx1 = torch.empty(M, C, device=d), torch.empty(M, C, device=d)
        call("mdvit_mlp_rc_dgrad", _p(gm), *common, _p(o["W1tp"]), _p(dx0), M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), _stream())
        call("mdvit_mlp_rc_dgrad_masked", _p(g), *common, _p(o["W1tp"]), _p(dx1), M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), *mk, _stream())
        assert torch.equal(dx0, dx1), f"dgrad dx: {tag}"
        wsb = _lib.load().mdvit_mlp_rc_wgrad_ws_bytes(M, C, Hd)
        ws = torch.empty(wsb // 4, device=d)

        def outs():
            return [torch.empty(roles, M, C, device=d), torch.empty(Hd, C, device=d), torch.empty(Hd, device=d), torch.empty(C, Hd, device=d)]
        # the whole backward in one kernel
        r0, r1, r2 = outs(), outs(), outs()
        call("mdvit_mlp_rc_bwd", _p(gm), *common, _p(o["W1tp"]), *[_p(t) for t in r0], _p(ws), wsb, M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), 0, _stream())
        for r in (r1, r2):
            call("mdvit_mlp_rc_bwd_masked", _p(g), *common, _p(o["W1tp"]), *[_p(t) for t in r], _p(ws), wsb, M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), *mk, 0,
                 _stream())
        for name, a, b, c in zip(("dx parts", "dW1", "db1", "dW2"), r0, r1, r2):
            assert torch.equal(a, b), f"bwd {name}: {tag}"
            assert torch.equal(b, c), f"bwd {name}, the same call again: {tag}"
        # the separate weight-gradient kernel
        w0, w1 = outs()[1:], outs()[1:]
        call("mdvit_mlp_rc_wgrad", _p(gm), *common, *[_p(t) for t in w0], _p(ws), wsb, M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), 0, _stream())
        call("mdvit_mlp_rc_wgrad_masked", _p(g), *common, *[_p(t) for t in w1], _p(ws), wsb, M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), *mk, 0, _stream())
        for name, a, b in zip(("dW1", "db1", "dW2"), w0, w1):
            assert torch.equal(a, b), f"wgrad {name}: {tag}"


@pytest.mark.parametrize("hbf", [False, True], ids=["du_fp32", "du_bf16"])
@pytest.mark.parametrize("Hd", [64, 1024])
def test_c128_masked_dgrad_equals_mask_pass_plus_kernel(Hd, hbf, rc_planes):
    """mdvit_mlp_rc16_dgrad[_hbf16] at C = 128: dx, du when requested, gm_out against the pass's gm, and the rows behind row M - 1 of gm_out untouched"""
    from mdvit_amd.ops import call, _p, _stream
    C = 128
    o = operands(C, Hd)
    d = dev()
    plain = "mdvit_mlp_rc16_dgrad_hbf16" if hbf else "mdvit_mlp_rc16_dgrad"
    masked = "mdvit_mlp_rc16_dgrad_masked_hbf16" if hbf else "mdvit_mlp_rc16_dgrad_masked"
    for (M, mp, rowscale, with_seed), want_du in itertools.product(cases(), (False, True)):
        tag = f"M={M} mask_p={mp} rowscale={rowscale} seed={with_seed} du={want_du}"
        seed = o["seed"] if with_seed else None
        x = o["x"][:M].contiguous()
        g, gm = mask_pass(o, M, C, mp, rowscale, seed)
        mk = (mp, KEY2[0], KEY2[1], _p(seed), _p(o["rs"]) if rowscale else None, RPS)
        w = (_p(x), _p(o["W1p"]), _p(o["b1"]), _p(o["W2tp"]), _p(o["W1tp"]))
        du0 = torch.zeros(M, Hd, device=d, dtype=torch.bfloat16 if hbf else torch.float32) if want_du else None
        du1 = torch.zeros_like(du0) if want_du else None
        dx0, dx1, dx2 = torch.empty(M, C, device=d), torch.empty(M, C, device=d), torch.empty(M, C, device=d)
        call(plain, _p(gm), *w, _p(du0), _p(dx0), M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), _stream())
        # without gm_out (the data-gradient-only sweep's form)
        call(masked, _p(g), *w, _p(du1), _p(dx1), None, M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), *mk, _stream())
        assert torch.equal(dx0, dx1), f"dx: {tag}"
        if want_du:
            assert torch.equal(du0, du1), f"du: {tag}"
        if mp > 0 or rowscale:
            # with gm_out: four guard rows behind row M - 1
            out = torch.full((M + 4, C), SENTINEL, device=d)
            call(masked, _p(g), *w, _p(du1), _p(dx2), _p(out), M, C, Hd, DROP1, KEY1[0], KEY1[1], _p(seed), *mk, _stream())
            assert torch.equal(dx0, dx2), f"dx with gm_out: {tag}"
            assert torch.equal(out[:M], gm), f"gm_out: {tag}"
            assert bool((out[M:] == SENTINEL).all()), f"gm_out written past row M - 1: {tag}"
            if want_du:
                assert torch.equal(du0, du1), f"du with gm_out: {tag}"


# ---- block level ---------------------------------------------------------------------------------------------------------------------------

def make_stage(C):
    from mdvit_amd.blocks import MHSA_stage_adapt, init_weights_
    torch.manual_seed(0)
    st = MHSA_stage_adapt(256, C, num_layers=2, num_heads=8, mlp_ratio=8, qkv_bias=True, drop_rate=0.1, drop_path_rate=0.1, adapt_method="Sup")
    init_weights_(st)
    with torch.no_grad():
        for p in st.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return st.to(dev()).train()


def run(st, x, label, H, W, g, entry, fold, monkeypatch, dgrad_only):
    from mdvit_amd import ops
    monkeypatch.setattr(ops, "_block_entry", entry)
    monkeypatch.setattr(ops, "_key_counter", itertools.count(41))
    torch.manual_seed(7)                               # the DropPath draws
    for p in st.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    ops.set_mlp_mask_fold(fold)
    try:
        y = st(xin, H, W, label)
        ops.set_dgrad_only(dgrad_only)
        try:
            y.backward(g)
        finally:
            ops.set_dgrad_only(False)
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        ops.set_mlp_mask_fold(1)
    return xin.grad, {n: (None if p.grad is None else p.grad.clone()) for n, p in st.named_parameters()}


def same(got, ref, what):
    """Bit equality -- except the gradients that the kernels of this project accumulate with float atomics (the window and depthwise-convolution weights,
    the adapters): those are not repeatable run to run in their last bits with or without this switch, so they are held to tests/test_gpu_block.py's
    2e-6 of the tensor's largest element.  None of them is computed by a kernel this switch touches."""
    assert torch.equal(got[0], ref[0]), f"{what}: dx differs by {float((got[0] - ref[0]).abs().max()):.3e}"
    for n in ref[1]:
        a, b = got[1][n], ref[1][n]
        assert (a is None) == (b is None), f"{what}: {n}"
        if a is None:
            continue
        if "crpe" in n or "cpe" in n or "domain_layer" in n:
            assert float((a - b).abs().max()) <= 2e-6 * max(float(b.abs().max()), 1e-12), f"{what}: {n}"
        else:
            assert torch.equal(a, b), f"{what}: {n} differs by {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("dgrad_only", [False, True], ids=["full_sweep", "dgrad_only_sweep"])
@pytest.mark.parametrize("C", [64, 128])
def test_block_backward_with_the_fold_equals_the_two_pass_form(C, dgrad_only, monkeypatch):
    """mdvit_block_bwd at B = 2, 8 x 8 tokens per image, dropout = DropPath = 0.1: switch on against switch off, and the operator path against the block entry"""
    from mdvit_amd import ops
    assert ops.gemm_precision() == "bf16x3"
    B, H, W = 2, 8, 8
    x = torch.randn(B, H * W, C, device=dev(), generator=torch.Generator(device=dev()).manual_seed(11))
    g = torch.randn(B, H * W, C, device=dev(), generator=torch.Generator(device=dev()).manual_seed(12))
    label = torch.nn.functional.one_hot(torch.tensor([1, 3]), 4).float().to(dev())
    st = make_stage(C)
    off = run(st, x, label, H, W, g, True, 0, monkeypatch, dgrad_only)
    on = run(st, x, label, H, W, g, True, 1, monkeypatch, dgrad_only)
    same(on, off, "block entry, fold on against off")
    op_on = run(st, x, label, H, W, g, False, 1, monkeypatch, dgrad_only)
    same(op_on, on, "operator path against block entry, fold on")
    op_off = run(st, x, label, H, W, g, False, 0, monkeypatch, dgrad_only)
    same(op_on, op_off, "operator path, fold on against off")
