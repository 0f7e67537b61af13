"""GPU: the shifted-window attention kernels (csrc/winattn.hip, ops.window_attention) against the fp64 restatement of tests/test_swin_host.py, which that
file pins to the reference's own mask construction and index rule on the CPU.

Shapes (B, H, W, heads, shift) -- the smallest at which the kernel can still go wrong:
  (2,16,16,3,4)   four windows per image, one of each mask class; the roll wraps on both axes; batch stride
  (1,16,24,6,4)   H != W: swapped axes in the shift / partition arithmetic
  (2,8,8,3,0)     one window, no mask, no shift (the last stage's case)
  (1,32,32,24,4)  interior windows without a masked pair beside edge windows; the widest channel stride (C = 768)
Two regimes each: scores at unit scale, and at gain 4 (q and k each doubled: peaked rows, median row maximum about 0.6 -- printed).

Bound (tests/test_gpu_adapter.py, docs/history.md): max|got - fp64| / max|fp64| per tensor (dtable also per head column) at most 10 x the same statistic of
torch's fp32 evaluation of the restatement on the CPU, which itself must stay below 1e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_model import dev
from test_swin_host import region_ids, window_attention_restated

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 16, 3, 4), (1, 16, 24, 6, 4), (2, 8, 8, 3, 0), (1, 32, 32, 24, 4)]
GAINS = [1.0, 4.0]
_cases = {}


def make_case(shape, gain):
    """fp64 CPU inputs (qkv with q, k scaled by sqrt(gain): the scores carry `gain`; a table of std 1; the upstream gradient) and, computed once per case, the
    fp64 and fp32 evaluations of the restatement: (inputs, want, base) with want / base = [out, dqkv, dtable]"""
    key = (shape, gain)
    if key in _cases:
        return _cases[key]
    B, H, W, heads, shift = shape
    Cn = heads * 32
    g = torch.Generator().manual_seed(17 * H + 5 * W + heads + shift + int(10 * gain))
    qkv = torch.randn(B, H * W, 3 * Cn, generator=g, dtype=torch.float64)
    qkv[..., :2 * Cn] *= gain ** 0.5
    table = torch.randn(225, heads, generator=g, dtype=torch.float64)
    gy = torch.randn(B, H * W, Cn, generator=g, dtype=torch.float64)

    def run(dtype):
        a, t = qkv.to(dtype).clone().requires_grad_(True), table.to(dtype).clone().requires_grad_(True)
        out, p = window_attention_restated(a, t, H, W, heads, shift)
        out.backward(gy.to(dtype))
        return [out.detach().double(), a.grad.double(), t.grad.double()], float(p.detach().max(-1).values.median())

    want, pmax = run(torch.float64)
    base, _ = run(torch.float32)
    _cases[key] = ((qkv, table, gy), want, base, pmax)
    return _cases[key]


def run_op(inputs, shape, qkv_grad=True):
    from mdvit_amd import ops
    B, H, W, heads, shift = shape
    qkv, table, gy = inputs
    a = qkv.float().to(dev()).requires_grad_(qkv_grad)
    t = table.float().to(dev()).requires_grad_(True)
    out = ops.window_attention(a, t, H, W, heads, shift)
    out.backward(gy.float().to(dev()))
    torch.cuda.synchronize()
    return [out.detach(), a.grad, t.grad]


def stat(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES)
def test_window_attention_matches_fp64_restatement_within_10x_the_fp32_cpu_error(shape, gain):
    inputs, want, base, pmax = make_case(shape, gain)
    got = run_op(inputs, shape)
    print(f"{shape} gain {gain}: median row maximum of the probabilities {pmax:.3f}")
    rows = [(n, w, b, o) for n, w, b, o in zip(("out", "dqkv", "dtable"), want, base, got)]
    rows += [(f"dtable[:, {h}]", want[2][:, h], base[2][:, h], got[2][:, h]) for h in range(shape[3])]
    bad = []
    for name, w, b32, o in rows:
        assert o is not None and tuple(o.shape) == tuple(w.shape), name
        e_base, e_op = stat(b32, w), stat(o, w)
        print(f"{shape} gain {gain} {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  bound {10 * e_base:.3e}")
        assert e_base < 1e-4, (name, e_base)
        if not (np.isfinite(e_op) and e_op <= 10.0 * e_base):
            bad.append((name, e_op, e_base))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_two_runs_are_bit_identical(shape):
    inputs = make_case(shape, 4.0)[0]
    a, b = run_op(inputs, shape), run_op(inputs, shape)
    for name, u, v in zip(("out", "dqkv", "dtable"), a, b):
        assert torch.equal(u, v), name


def test_table_gradient_alone_and_data_gradient_alone():
    """qkv without a gradient: the table's gradient is the same, bit for bit; the data-gradient-only sweep gives the same dqkv and no table gradient"""
    from mdvit_amd import ops
    shape = SHAPES[1]
    inputs = make_case(shape, 1.0)[0]
    full = run_op(inputs, shape)
    only_t = run_op(inputs, shape, qkv_grad=False)
    assert only_t[1] is None and torch.equal(only_t[2], full[2])
    ops.set_dgrad_only(True)
    try:
        only_x = run_op(inputs, shape)
    finally:
        ops.set_dgrad_only(False)
    assert only_x[2] is None and torch.equal(only_x[1], full[1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]])
def test_masked_pairs_contribute_nothing(shape):
    """v = the indicator of one region of the rolled image: a token of any OTHER region sees that region only through masked pairs (-100 on the score), or
    not at all -- its output is 0 to fp32 round-off (< 1e-30); a token of the region itself reads exactly its own kind: 1"""
    from mdvit_amd import ops
    B, H, W, heads, shift = shape
    Cn = heads * 32
    qkv, table, _ = make_case(shape, 1.0)[0]
    rid_rolled = region_ids(H, W, shift)                                            # indexed by shifted coordinates
    rid = torch.from_numpy(np.roll(rid_rolled, (shift, shift), axis=(0, 1)).reshape(-1))          # by natural token
    t = table.float().to(dev())
    for R in sorted(set(rid.tolist())):
        a = qkv.float().clone()
        a[..., 2 * Cn:] = (rid == R).float()[None, :, None]
        out = ops.window_attention(a.to(dev()), t, H, W, heads, shift).cpu()
        other = out[:, rid != R]
        assert float(other.abs().max()) < 1e-30, (R, float(other.abs().max()))
        assert torch.allclose(out[:, rid == R], torch.ones(()), rtol=0, atol=1e-5), R


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_every_output_element_is_written(shape):
    """NaN-filled caller-owned buffers at the C ABI: out, lse, dqkv and dtable come back finite everywhere; accumulate adds to what dtable held"""
    from mdvit_amd import _lib
    lib = _lib.load()
    B, H, W, heads, shift = shape
    Cn = heads * 32
    qkv, table, gy = (t.float().to(dev()).contiguous() for t in make_case(shape, 1.0)[0])
    nan = lambda *s: torch.full(s, float("nan"), device=dev(), dtype=torch.float32)
    out, lse, dqkv, dtable = nan(B, H * W, Cn), nan(B, heads, H * W), nan(B, H * W, 3 * Cn), nan(225, heads)
    wsb = lib.mdvit_winattn_bwd_ws_bytes(B, H, W, heads)
    ws = nan(wsb // 4)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.mdvit_winattn_fwd(p(qkv), p(table), p(out), p(lse), B, H, W, Cn, heads, shift, st), "winattn_fwd")
    _lib.check(lib.mdvit_winattn_bwd(p(gy), p(qkv), p(table), p(lse), p(dqkv), p(dtable), p(ws), wsb, 0, B, H, W, Cn, heads, shift, st), "winattn_bwd")
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv), ("dtable", dtable)):
        assert bool(torch.isfinite(t).all()), name
    acc = torch.ones(225, heads, device=dev())
    _lib.check(lib.mdvit_winattn_bwd(p(gy), p(qkv), p(table), p(lse), None, p(acc), p(ws), wsb, 1, B, H, W, Cn, heads, shift, st), "winattn_bwd")
    torch.cuda.synchronize()
    assert torch.equal(acc, 1.0 + dtable)
    # a short workspace is refused before any launch
    assert lib.mdvit_winattn_bwd(p(gy), p(qkv), p(table), p(lse), p(dqkv), p(dtable), p(ws), wsb - 4, 0, B, H, W, Cn, heads, shift, st) == 4
