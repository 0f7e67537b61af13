"""GPU: the low-rank attention kernels (csrc/lowrank_attn.hip, ops.lowrank_attention) against the fp64 restatement of tests/test_utnet_host.py, which that file
pins to the reference's own LinearAttention / LinearAttentionDecoder on the CPU.

Shapes (B, Hq, Wq, dim_head), heads = 4 -- the smallest at which the kernel can still go wrong:
  (2, 8, 8, 128)   one query per cell, the widest LDS footprint, batch stride
  (1, 16, 24, 16)  non-square grid with 2 x 3 queries per cell, 384 queries
  (2, 32, 32, 32)  several workgroups per (image, head): the second stage really sums
  (1, 64, 64, 64)  many partial rows
  (1, 24, 40, 16)  960 queries, 15 per cell: the last round of a workgroup is partly empty
Two regimes each: scores at unit scale, and at gain 4 (q and k each doubled: peaked rows -- the median row maximum is printed).

Bound (tests/test_gpu_adapter.py, docs/history.md): max|got - fp64| / max|fp64| per tensor (dtable also per head column) at most 10 x the same statistic of
torch's fp32 evaluation of the restatement on the CPU, which itself must stay below 1e-4.

At a step's launch counts, per row (NEW_SHAPES, `reached`, the second half of the file).  The shapes above run 64, 32, 16 and 4 cells per workgroup, one pass of
lrattn_kv_reduce_kernel and a batch fold over at most 2 images, and a whole-tensor statistic dilutes one wrong row of 16 numbers among a million.  NEW_SHAPES adds
  (1, 128, 128, 16)  a step's down1 / up3 image: ONE cell per workgroup, 64 partial dK / dV rows, a cell's bias sum carried over four rounds
  (1, 136, 128, 16)  272 queries per cell: five rounds, the last with 16 queries -- its second wavefront has no query at all, the first is half empty
  (1, 72, 64, 64)    two cells per workgroup, the cell boundary inside the last round
  (1, 40, 32, 32)    eight cells per workgroup of 20 queries: cells straddle rounds, the last round fills wavefront 0 only
  (17, 8, 8, 128)    1,114,112 dK / dV elements: the second pass of lrattn_kv_reduce_kernel's grid-stride loop; the bias gradient folded over 17 images
`reached` restates the host arithmetic (cells_per_wg, the round loop, the capped grid of the second stage); tests/test_attn_launch_arithmetic.py asserts without a GPU
that every shape reaches what it is listed for, and a test below holds the restatement against the library through mdvit_lrattn_bwd_ws_bytes.
Measure there: out, dq, dk, dv by the WORST ROW (one (image, token or key, head) vector over the head dimension) and the WORST COLUMN (one (image, channel) over all
tokens or keys) of max|got - fp64| / max|fp64| inside that row / column; dtable by the worst table row over the heads besides the per-head column.  Bound: FACTOR x
the same statistic of the fp32 CPU evaluation, which must stay below BASE_LIMIT (test_gpu_attention.py).  dq rows are measured at gain 1 only: with peaked
probabilities dS is nearly 0, a dq row is a difference of nearly equal numbers and the fp32 evaluation itself is off by 0.1 to 5 % there (dq is held by its columns
at gain 4, and a token left out is caught by the gain-1 rows).  Single table elements are not well conditioned either (up to 6e-3 in fp32): none is measured alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_attention import BASE_LIMIT, FACTOR
from test_gpu_model import dev
from test_utnet_host import lowrank_attention_restated

pytestmark = pytest.mark.gpu

HEADS = 4
SHAPES = [(2, 8, 8, 128), (1, 16, 24, 16), (2, 32, 32, 32), (1, 64, 64, 64), (1, 24, 40, 16)]
NEW_SHAPES = [(1, 128, 128, 16), (1, 136, 128, 16), (1, 72, 64, 64), (1, 40, 32, 32), (17, 8, 8, 128)]
GAINS = [1.0, 4.0]
NAMES = ("out", "dq", "dk", "dv", "dtable")
_cases = {}


def reached(B, Hq, Wq, D, heads=HEADS):
    """The host-side launch arithmetic of mdvit_lrattn_fwd / _bwd restated (cells_per_wg, the round loop of a workgroup, the grid of lrattn_kv_reduce_kernel capped at
    4096 workgroups of 256 threads, the batch loop of lrattn_table_reduce_kernel): which code a shape runs.
      qpc queries per cell; cpw cells per workgroup; nwg workgroups = partial dK / dV rows per (image, head); rounds of 64 queries a workgroup walks; last the queries of
      its last round; wave1_empty: the second wavefront of that round has no query; straddle: some cell's queries lie in two rounds (the running bias sum is carried);
      kv_passes of the second stage's grid-stride loop; fold the images the bias gradient is folded over."""
    qpc = (Hq // 8) * (Wq // 8)
    cpw = 64
    while cpw > 1 and cpw * qpc > 256:
        cpw //= 2
    n = cpw * qpc
    rounds = -(-n // 64)
    last = n - 64 * (rounds - 1)
    straddle = any(c * qpc // 64 != ((c + 1) * qpc - 1) // 64 for c in range(cpw))
    return dict(qpc=qpc, cpw=cpw, nwg=64 // cpw, rounds=rounds, last=last, wave1_empty=last <= 32, straddle=straddle,
                kv_passes=-(-(B * heads * 2 * 64 * D) // (4096 * 256)), fold=B)


# what `reached` must say of each shape (tests/test_attn_launch_arithmetic.py)
REACHES = {
    (2, 8, 8, 128): dict(qpc=1, cpw=64, nwg=1, rounds=1, last=64, straddle=False, kv_passes=1, fold=2),
    (1, 16, 24, 16): dict(qpc=6, cpw=32, nwg=2, rounds=3, last=64, straddle=True),
    (2, 32, 32, 32): dict(qpc=16, cpw=16, nwg=4, rounds=4, last=64, straddle=False, fold=2),
    (1, 64, 64, 64): dict(qpc=64, cpw=4, nwg=16, rounds=4, last=64, straddle=False),
    (1, 24, 40, 16): dict(qpc=15, cpw=16, nwg=4, rounds=4, last=48, wave1_empty=False, straddle=True),
    (1, 128, 128, 16): dict(qpc=256, cpw=1, nwg=64, rounds=4, last=64, wave1_empty=False, straddle=True, kv_passes=1),
    (1, 136, 128, 16): dict(qpc=272, cpw=1, nwg=64, rounds=5, last=16, wave1_empty=True, straddle=True),
    (1, 72, 64, 64): dict(qpc=72, cpw=2, nwg=32, rounds=3, last=16, straddle=True),
    (1, 40, 32, 32): dict(qpc=20, cpw=8, nwg=8, rounds=3, last=32, wave1_empty=True, straddle=True),
    (17, 8, 8, 128): dict(qpc=1, cpw=64, nwg=1, kv_passes=2, fold=17),
}


def restated(inputs, shape, dtype, keep=None):
    """[out, dq, dk, dv, dtable] of the restatement in `dtype`, as fp64, and the median row maximum of the probabilities"""
    B, Hq, Wq, D = shape
    q, k, v, table, gy = (t.to(dtype).clone() for t in inputs)
    leaves = [t.requires_grad_(True) for t in (q, k, v, table)]
    out, p = lowrank_attention_restated(*leaves, Hq, Wq, HEADS, keep=None if keep is None else keep.to(dtype))
    out.backward(gy)
    return [out.detach().double()] + [t.grad.double() for t in leaves], float(p.detach().max(-1).values.median())


def make_case(shape, gain):
    """fp64 CPU inputs (q, k scaled by sqrt(gain): the scores carry `gain`; a table of std 1; the upstream gradient) and, computed once per case, the fp64 and
    fp32 evaluations of the restatement"""
    key = (shape, gain)
    if key in _cases:
        return _cases[key]
    B, Hq, Wq, D = shape
    Cn, N = HEADS * D, Hq * Wq
    g = torch.Generator().manual_seed(17 * Hq + 5 * Wq + D + int(10 * gain))
    q = torch.randn(B, N, Cn, generator=g, dtype=torch.float64) * gain ** 0.5
    k = torch.randn(B, 64, Cn, generator=g, dtype=torch.float64) * gain ** 0.5
    v = torch.randn(B, 64, Cn, generator=g, dtype=torch.float64)
    table = torch.randn(225, HEADS, generator=g, dtype=torch.float64)
    gy = torch.randn(B, N, Cn, generator=g, dtype=torch.float64)
    inputs = (q, k, v, table, gy)
    want, pmax = restated(inputs, shape, torch.float64)
    base, _ = restated(inputs, shape, torch.float32)
    _cases[key] = (inputs, want, base, pmax)
    return _cases[key]


def run_op(inputs, shape, data_grad=True, drop_p=0.0, key=None):
    from mdvit_amd import ops
    B, Hq, Wq, D = shape
    q, k, v, table = (t.float().to(dev()).requires_grad_(data_grad or i == 3) for i, t in enumerate(inputs[:4]))
    out = ops.lowrank_attention(q, k, v, table, Hq, Wq, HEADS, drop_p, key)
    out.backward(inputs[4].float().to(dev()))
    torch.cuda.synchronize()
    return [out.detach(), q.grad, k.grad, v.grad, table.grad]


def stat(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def assert_within_bound(tag, want, base, got):
    rows = [(n, w, b, o) for n, w, b, o in zip(NAMES, want, base, got)]
    rows += [(f"dtable[:, {h}]", want[4][:, h], base[4][:, h], got[4][:, h]) for h in range(HEADS)]
    bad = []
    for name, w, b32, o in rows:
        assert o is not None and tuple(o.shape) == tuple(w.shape), name
        e_base, e_op = stat(b32, w), stat(o, w)
        print(f"{tag} {name}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  bound {10 * e_base:.3e}")
        assert e_base < 1e-4, (name, e_base)
        if not (np.isfinite(e_op) and e_op <= 10.0 * e_base):
            bad.append((name, e_op, e_base))
    assert not bad, bad


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES)
def test_lowrank_attention_matches_fp64_restatement_within_10x_the_fp32_cpu_error(shape, gain):
    inputs, want, base, pmax = make_case(shape, gain)
    print(f"{shape} gain {gain}: median row maximum of the probabilities {pmax:.3f}")
    assert_within_bound(f"{shape} gain {gain}", want, base, run_op(inputs, shape))


@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
def test_two_runs_are_bit_identical(shape):
    inputs = make_case(shape, 4.0)[0]
    a, b = run_op(inputs, shape), run_op(inputs, shape)
    for name, u, v in zip(NAMES, a, b):
        assert torch.equal(u, v), name


def test_q_as_a_column_slice_equals_q_contiguous():
    """q = the middle third of a [B, N, 3C] product, k and v the two halves of a [B, 64, 2C] one: the same bits as from contiguous copies"""
    from mdvit_amd import ops
    shape = SHAPES[2]
    B, Hq, Wq, D = shape
    Cn = HEADS * D
    q, k, v, table, gy = (t.float().to(dev()) for t in make_case(shape, 1.0)[0])
    full = run_op(make_case(shape, 1.0)[0], shape)
    wide = torch.randn(B, Hq * Wq, 3 * Cn, device=dev())
    wide[..., Cn:2 * Cn] = q
    wide.requires_grad_(True)
    kv = torch.cat([k, v], -1).requires_grad_(True)
    t = table.clone().requires_grad_(True)
    out = ops.lowrank_attention(wide[..., Cn:2 * Cn], kv[..., :Cn], kv[..., Cn:], t, Hq, Wq, HEADS)
    out.backward(gy)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), full[0])
    assert torch.equal(wide.grad[..., Cn:2 * Cn], full[1]) and float(wide.grad[..., :Cn].abs().max()) == 0.0 and float(wide.grad[..., 2 * Cn:].abs().max()) == 0.0
    assert torch.equal(kv.grad[..., :Cn], full[2]) and torch.equal(kv.grad[..., Cn:], full[3]) and torch.equal(t.grad, full[4])


def test_table_gradient_alone_and_data_gradient_alone():
    """q, k, v without a gradient: the table's gradient is the same, bit for bit; the data-gradient-only sweep gives the same dq, dk, dv and no table gradient"""
    from mdvit_amd import ops
    shape = SHAPES[4]
    inputs = make_case(shape, 1.0)[0]
    full = run_op(inputs, shape)
    only_t = run_op(inputs, shape, data_grad=False)
    assert only_t[1] is None and only_t[2] is None and only_t[3] is None and torch.equal(only_t[4], full[4])
    ops.set_dgrad_only(True)
    try:
        only_x = run_op(inputs, shape)
    finally:
        ops.set_dgrad_only(False)
    assert only_x[4] is None and all(torch.equal(only_x[i], full[i]) for i in (1, 2, 3))


def test_table_gradient_through_a_sink_equals_the_autograd_gradient():
    """the gradient-sink route (table gradient accumulated by the kernel's second stage, on the side stream) == the plain route"""
    from mdvit_amd import ops
    shape = SHAPES[2]
    B, Hq, Wq, D = shape
    inputs = make_case(shape, 1.0)[0]
    full = run_op(inputs, shape)
    q, k, v, table = (t.float().to(dev()).requires_grad_(True) for t in inputs[:4])
    sink = torch.ones_like(table)
    had_side = ops._side_stream is not None
    ops.enable_side_stream(True)
    ops.set_grad_sinks({table: sink})
    try:
        ops.lowrank_attention(q, k, v, table, Hq, Wq, HEADS).backward(inputs[4].float().to(dev()))
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        ops.set_grad_sinks(None)
        ops.enable_side_stream(had_side)
    assert table.grad is None and torch.equal(q.grad, full[1]) and torch.equal(k.grad, full[2]) and torch.equal(v.grad, full[3])
    assert torch.equal(sink, 1.0 + full[4])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], (1, 136, 128, 16)])
def test_every_output_element_is_written(shape):
    """NaN-filled caller-owned buffers at the C ABI: out, lse, dq, dk, dv and dtable come back finite everywhere; accumulate adds to what dtable held; a short
    workspace is refused before any launch"""
    from mdvit_amd import _lib
    lib = _lib.load()
    B, Hq, Wq, D = shape
    Cn, N = HEADS * D, Hq * Wq
    q, k, v, table, gy = (t.float().to(dev()).contiguous() for t in make_case(shape, 1.0)[0])
    nan = lambda *s: torch.full(s, float("nan"), device=dev(), dtype=torch.float32)
    out, lse, dq, dk, dv, dtable = nan(B, N, Cn), nan(B, HEADS, N), nan(B, N, Cn), nan(B, 64, Cn), nan(B, 64, Cn), nan(225, HEADS)
    wsb = lib.mdvit_lrattn_bwd_ws_bytes(B, Hq, Wq, D, HEADS)
    assert wsb > 0
    ws = nan(wsb // 4)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geo = (B, Hq, Wq, D, HEADS, 0.0, 0, 0, None, st)
    _lib.check(lib.mdvit_lrattn_fwd(p(q), Cn, p(k), p(v), Cn, p(table), p(out), p(lse), *geo), "lrattn_fwd")
    _lib.check(lib.mdvit_lrattn_bwd(p(gy), p(q), Cn, p(k), p(v), Cn, p(table), p(lse), p(dq), Cn, p(dk), p(dv), Cn, p(dtable), p(ws), wsb, 0, *geo), "lrattn_bwd")
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv), ("dtable", dtable)):
        assert bool(torch.isfinite(t).all()), name
    acc = torch.ones(225, HEADS, device=dev())
    _lib.check(lib.mdvit_lrattn_bwd(p(gy), p(q), Cn, p(k), p(v), Cn, p(table), p(lse), None, Cn, None, None, Cn, p(acc), p(ws), wsb, 1, *geo), "lrattn_bwd")
    torch.cuda.synchronize()
    assert torch.equal(acc, 1.0 + dtable)
    assert lib.mdvit_lrattn_bwd(p(gy), p(q), Cn, p(k), p(v), Cn, p(table), p(lse), p(dq), Cn, p(dk), p(dv), Cn, p(dtable), p(ws), wsb - 4, 0, *geo) == 4


def test_backward_workspace_is_smaller_than_one_score_tensor():
    from mdvit_amd import _lib
    B, Hq, Wq, D = 2, 64, 64, 16
    assert 0 < _lib.load().mdvit_lrattn_bwd_ws_bytes(B, Hq, Wq, D, HEADS) < B * HEADS * Hq * Wq * 64 * 4 == 8 << 20


# ---- dropout on the probabilities -------------------------------------------------------------------------------------------------------------------------
DROP_P, DROP_KEY = 0.1, (0x1234, 0x9ABC)


def read_mask(inputs, shape, key=DROP_KEY):
    """the dropped probability matrix [B, heads, N, 64], read out through v = 64-column blocks of the identity under ONE key"""
    from mdvit_amd import ops
    B, Hq, Wq, D = shape
    q, k, _v, table, _gy = inputs
    pd = torch.zeros(B, HEADS, Hq * Wq, 64)
    for j0 in range(0, 64, D):
        v = torch.zeros(B, 64, D, HEADS)
        for j in range(j0, min(j0 + D, 64)):
            v[:, j, j - j0, :] = 1.0
        out = ops.lowrank_attention(q.float().to(dev()), k.float().to(dev()), v.view(B, 64, D * HEADS).to(dev()), table.float().to(dev()), Hq, Wq, HEADS, DROP_P, key)
        o = out.cpu().view(B, Hq * Wq, D, HEADS).permute(0, 3, 1, 2)          # [B, heads, N, D]
        w = min(D, 64 - j0)
        pd[..., j0:j0 + w] = o[..., :w]
        if w < D:
            assert float(o[..., w:].abs().max()) == 0.0
    return pd


@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (1, 8, 8, 16), (1, 16, 8, 32), (1, 8, 8, 128)])
def test_dropout_mask_is_exact_repeatable_and_at_the_asked_rate(shape):
    inputs, want, _base, _ = make_case(shape, 1.0)
    p64 = lowrank_attention_restated(*inputs[:4], shape[1], shape[2], HEADS)[1]
    pd = read_mask(inputs, shape).double()
    kept = pd != 0
    assert float((pd - p64 / (1.0 - DROP_P))[kept].abs().max()) <= 1e-5          # every entry is 0 or P / 0.9
    n = kept.numel()
    share = float(kept.double().mean())
    sigma = (DROP_P * (1.0 - DROP_P) / n) ** 0.5
    print(f"{shape}: kept share {share:.5f} of {n} entries, {abs(share - (1 - DROP_P)) / sigma:.2f} standard deviations from {1 - DROP_P}")
    assert abs(share - (1.0 - DROP_P)) <= 5.0 * sigma
    per_bh = kept.double().mean((2, 3))          # no (image, head) shares its mask with another, none is off the rate
    assert float((per_bh - (1.0 - DROP_P)).abs().max()) <= 5.0 * (DROP_P * (1.0 - DROP_P) / (n / per_bh.numel())) ** 0.5
    flat = kept.view(-1, kept.shape[2] * 64)
    assert all(not torch.equal(flat[0], flat[i]) for i in range(1, flat.shape[0]))
    if shape[3] == 64:
        assert torch.equal(read_mask(inputs, shape) != 0, kept)                                    # the same key draws the same mask
        other = read_mask(inputs, shape, key=(DROP_KEY[0] + 1, DROP_KEY[1])) != 0
        assert 0.15 < float((other != kept).double().mean()) < 0.21                                # another key another one (independent: 2 * 0.9 * 0.1 = 0.18)


def test_dropout_backward_meets_the_bound_under_the_mask_read_from_the_forward():
    shape = (2, 16, 16, 64)
    inputs = make_case(shape, 1.0)[0]
    keep = (read_mask(inputs, shape) != 0).double() / (1.0 - DROP_P)
    want, _ = restated(inputs, shape, torch.float64, keep)
    base, _ = restated(inputs, shape, torch.float32, keep)
    got = run_op(inputs, shape, drop_p=DROP_P, key=DROP_KEY)
    assert_within_bound(f"{shape} dropout", want, base, got)
    again = run_op(inputs, shape, drop_p=DROP_P, key=DROP_KEY)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ---- at a step's launch counts, by the worst row and the worst column ---------------------------------------------------------------------------------------
def row_errors(got, ref):
    """[B, tokens, heads]: per (image, token or key, head) vector over the head dimension of a [B, tokens, d * heads + h] tensor, max_d |got - ref| / max_d |ref|"""
    got, ref = got.detach().double().cpu(), ref.double()
    B, T, Cn = ref.shape
    return (got - ref).abs().view(B, T, Cn // HEADS, HEADS).amax(dim=2) / ref.abs().view(B, T, Cn // HEADS, HEADS).amax(dim=2)


def column_errors(got, ref):
    """[B, C]: per (image, channel) column over all tokens or keys"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def table_row_errors(got, ref):
    """[225]: per table row over the heads"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def assert_rows_and_columns(tag, want, base, got, dq_rows):
    """every tensor's worst row and worst column within FACTOR x those of the fp32 CPU evaluation, which stay below BASE_LIMIT; all lines are printed first"""
    lines = []
    for i, name in enumerate(NAMES[:4]):
        assert got[i] is not None and tuple(got[i].shape) == tuple(want[i].shape), name
        if name != "dq" or dq_rows:
            lines.append((f"{name} rows", row_errors, i))
        lines.append((f"{name} columns", column_errors, i))
    lines.append(("dtable rows", table_row_errors, 4))
    loose, bad = [], []
    for label, fn, i in lines:
        e_op, e_base = float(fn(got[i], want[i]).max()), float(fn(base[i], want[i]).max())
        print(f"{tag} {label}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  ratio {e_op / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}")
        if not e_base < BASE_LIMIT:
            loose.append((label, e_base))
        if not (np.isfinite(e_op) and e_op <= FACTOR * e_base):
            bad.append((label, e_op, e_base))
    assert not loose, f"{tag}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (line, worst error) {loose}"
    assert not bad, f"{tag}: (line, worst error, fp32 CPU worst error) {bad}"


@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
def test_the_library_sizes_its_workspace_by_the_restated_workgroup_count(shape):
    """mdvit_lrattn_bwd_ws_bytes gives cells_per_wg back through the size: nwg partial [dK | dV] pairs and one [64, 64] bias gradient per (image, head)"""
    from mdvit_amd import _lib
    B, Hq, Wq, D = shape
    assert _lib.load().mdvit_lrattn_bwd_ws_bytes(B, Hq, Wq, D, HEADS) == 4 * B * HEADS * (reached(*shape)["nwg"] * 2 * 64 * D + 64 * 64)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
def test_lowrank_attention_by_the_worst_row_and_the_worst_column(shape, gain):
    """the old shapes and the new ones: the whole-tensor bound of the first test, then rows and columns (dq rows at gain 1 only: the top of the file)"""
    inputs, want, base, pmax = make_case(shape, gain)
    got = run_op(inputs, shape)
    tag = f"{shape} gain {gain}"
    print(f"{tag}: median row maximum of the probabilities {pmax:.3f}  {reached(*shape)}")
    assert_within_bound(tag, want, base, got)
    assert_rows_and_columns(tag, want, base, got, dq_rows=gain == 1.0)


def test_data_gradient_alone_in_two_passes_of_the_second_stage():
    """(17, 8, 8, 128) with dtable == NULL: the second pass of lrattn_kv_reduce_kernel without the table stage behind it -- dq, dk, dv as in the full run, bit for bit"""
    from mdvit_amd import ops
    shape = (17, 8, 8, 128)
    assert reached(*shape)["kv_passes"] == 2
    inputs = make_case(shape, 1.0)[0]
    full = run_op(inputs, shape)
    ops.set_dgrad_only(True)
    try:
        only_x = run_op(inputs, shape)
    finally:
        ops.set_dgrad_only(False)
    assert only_x[4] is None and all(torch.equal(only_x[i], full[i]) for i in (1, 2, 3))


@pytest.mark.parametrize("shape", [(1, 24, 40, 16), (1, 40, 32, 32), (1, 8, 8, 128)])
def test_dropout_backward_by_row_and_column_under_the_mask_read_from_the_forward(shape):
    """the procedure of the test above at 15 queries per cell with a ragged last round (the mask index is the natural token of the rows that exist, none is drawn for
    an empty row), with an empty second wavefront, and at the widest head: the mask read through identity v blocks, the restatement under it, the whole-tensor bound,
    rows and columns, two runs bit-identical"""
    inputs = make_case(shape, 1.0)[0]
    keep = (read_mask(inputs, shape) != 0).double() / (1.0 - DROP_P)
    want, _ = restated(inputs, shape, torch.float64, keep)
    base, _ = restated(inputs, shape, torch.float32, keep)
    got = run_op(inputs, shape, drop_p=DROP_P, key=DROP_KEY)
    assert_within_bound(f"{shape} dropout", want, base, got)
    assert_rows_and_columns(f"{shape} dropout", want, base, got, dq_rows=True)
    again = run_op(inputs, shape, drop_p=DROP_P, key=DROP_KEY)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
