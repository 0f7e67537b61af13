"""GPU: the shifted-window attention kernels (csrc/winattn.hip, ops.window_attention) against the fp64 restatement of tests/test_swin_host.py, which that
file pins to the reference's own mask construction and index rule on the CPU.

Shapes (B, H, W, heads, shift) -- the smallest at which the kernel can still go wrong:
  (2,16,16,3,4)   four windows per image, one of each mask class; the roll wraps on both axes; batch stride
  (1,16,24,6,4)   H != W: swapped axes in the shift / partition arithmetic
  (2,8,8,3,0)     one window, no mask, no shift (the last stage's case)
  (1,32,32,24,4)  interior windows without a masked pair beside edge windows; the widest channel stride (C = 768)
Two regimes each: scores at unit scale, and at gain 4 (q and k each doubled: peaked rows, median row maximum about 0.6 -- printed).

Bound (tests/test_gpu_adapter.py, docs/history.md): max|got - fp64| / max|fp64| per tensor (dtable also per head column) at most 10 x the same statistic of
torch's fp32 evaluation of the restatement on the CPU, which itself must stay below 1e-4.

At a step's launch counts, per row (NEW_SHAPES, `reached`, the end of the file).  Every Swin stage alternates shift 0 and shift 4, and the shapes above run shift 0
on ONE window; they hand winattn_table_reduce_kernel 8, 6, 2 and 16 partial rows (it adds the rows blk = j, j + 8, ...), where a step's first stage hands it 1024; and
the whole-tensor statistic lumps dq, dk and dv into one dqkv.  NEW_SHAPES adds
  (2, 16, 24, 3, 0)  shift 0 over six windows per image, H != W: the window addressing without the roll -- the first block of every stage
  (3, 16, 24, 3, 4)  18 partial rows: a second and a third, ragged, trip of the table reduce
  (4, 64, 64, 3, 4)  a step's stage-0 grid: 256 partial rows, interior windows outnumber edge windows
`reached` restates the host arithmetic; tests/test_attn_launch_arithmetic.py asserts without a GPU that every shape reaches what it is listed for.
Measure there: out and the three thirds of dqkv -- dq, dk, dv -- each by the WORST ROW (one (image, token, head) vector over the head dimension) and the WORST
COLUMN (one (image, channel) over all tokens) of max|got - fp64| / max|fp64| inside that row / column; dtable by the worst table row over the heads besides the
per-head column.  Bound: FACTOR x the same statistic of the fp32 CPU evaluation, which must stay below BASE_LIMIT (test_gpu_attention.py).  dq rows are measured at
gain 1 only: with peaked probabilities dS is nearly 0, a dq row is a difference of nearly equal numbers and the fp32 evaluation itself is off by 0.1 to 5 % there."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_attention import BASE_LIMIT, FACTOR
from test_gpu_model import dev
from test_swin_host import region_ids, window_attention_restated

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 16, 3, 4), (1, 16, 24, 6, 4), (2, 8, 8, 3, 0), (1, 32, 32, 24, 4)]
NEW_SHAPES = [(2, 16, 24, 3, 0), (3, 16, 24, 3, 4), (4, 64, 64, 3, 4)]
GAINS = [1.0, 4.0]
_cases = {}


def reached(B, H, W, heads, shift):
    """The host-side launch arithmetic of mdvit_winattn_bwd restated: nw windows per image, nblk = B nw workgroups per head = partial table rows, reduce_iters trips of
    winattn_table_reduce_kernel's loop over blk = j, j + 8, ... (the longest thread's), ragged: the last trip is not taken by all eight threads of an entry"""
    nw = (H // 8) * (W // 8)
    nblk = B * nw
    return dict(nw=nw, nblk=nblk, reduce_iters=-(-nblk // 8), ragged=nblk % 8 != 0, shift=shift)


# what `reached` must say of each shape (tests/test_attn_launch_arithmetic.py)
REACHES = {
    (2, 16, 16, 3, 4): dict(nw=4, nblk=8, reduce_iters=1, ragged=False),
    (1, 16, 24, 6, 4): dict(nw=6, nblk=6, reduce_iters=1, ragged=True),
    (2, 8, 8, 3, 0): dict(nw=1, nblk=2, reduce_iters=1, ragged=True, shift=0),
    (1, 32, 32, 24, 4): dict(nw=16, nblk=16, reduce_iters=2, ragged=False),
    (2, 16, 24, 3, 0): dict(nw=6, nblk=12, reduce_iters=2, ragged=True, shift=0),
    (3, 16, 24, 3, 4): dict(nw=6, nblk=18, reduce_iters=3, ragged=True, shift=4),
    (4, 64, 64, 3, 4): dict(nw=64, nblk=256, reduce_iters=32, ragged=False, shift=4),
}


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


@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
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


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], (2, 16, 24, 3, 0)])
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


# ---- at a step's launch counts, by the worst row and the worst column ---------------------------------------------------------------------------------------
def row_errors(got, ref):
    """[B, tokens, heads]: per (image, token, head) vector over the head dimension of a [B, tokens, h * 32 + d] tensor, max_d |got - ref| / max_d |ref|"""
    got, ref = got.detach().double().cpu(), ref.double()
    B, T, Cn = ref.shape
    return (got - ref).abs().view(B, T, Cn // 32, 32).amax(dim=3) / ref.abs().view(B, T, Cn // 32, 32).amax(dim=3)


def column_errors(got, ref):
    """[B, C]: per (image, channel) column over all tokens"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def table_row_errors(got, ref):
    """[225]: per table row over the heads"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def thirds(t):
    """[out, dqkv, dtable] -> out, dq, dk, dv, dtable"""
    return [t[0], *t[1].split(t[1].shape[2] // 3, dim=2), t[2]]


@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
def test_the_library_sizes_its_workspace_by_the_restated_partial_row_count(shape):
    from mdvit_amd import _lib
    B, H, W, heads, shift = shape
    assert _lib.load().mdvit_winattn_bwd_ws_bytes(B, H, W, heads) == 4 * reached(*shape)["nblk"] * heads * 225


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES + NEW_SHAPES)
def test_window_attention_by_the_worst_row_and_the_worst_column(shape, gain):
    """the old shapes and the new ones: the whole-tensor statistic of the first test on out, dqkv, dtable and its head columns, then out, dq, dk, dv by rows and columns
    and dtable by table rows (dq rows at gain 1 only: the top of the file)"""
    inputs, want, base, pmax = make_case(shape, gain)
    got = run_op(inputs, shape)
    tag = f"{shape} gain {gain}"
    print(f"{tag}: median row maximum of the probabilities {pmax:.3f}  {reached(*shape)}")
    for name, w, o in zip(("out", "dqkv", "dtable"), want, got):
        assert o is not None and tuple(o.shape) == tuple(w.shape), name
    lines = [(n, stat, w, b, o) for n, w, b, o in zip(("out", "dqkv", "dtable"), want, base, got)]
    lines += [(f"dtable[:, {h}]", stat, want[2][:, h], base[2][:, h], got[2][:, h]) for h in range(shape[3])]
    for name, w, b, o in zip(("out", "dq", "dk", "dv"), thirds(want), thirds(base), thirds(got)):
        if name != "dq" or gain == 1.0:
            lines.append((f"{name} rows", lambda x, y: float(row_errors(x, y).max()), w, b, o))
        lines.append((f"{name} columns", lambda x, y: float(column_errors(x, y).max()), w, b, o))
    lines.append(("dtable rows", lambda x, y: float(table_row_errors(x, y).max()), want[2], base[2], got[2]))
    loose, bad = [], []
    for label, fn, w, b32, o in lines:
        e_op, e_base = fn(o, w), fn(b32, w)
        print(f"{tag} {label}: op {e_op:.3e}  fp32-cpu {e_base:.3e}  ratio {e_op / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}")
        if not e_base < BASE_LIMIT:
            loose.append((label, e_base))
        if not (np.isfinite(e_op) and e_op <= FACTOR * e_base):
            bad.append((label, e_op, e_base))
    assert not loose, f"{tag}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (line, worst error) {loose}"
    assert not bad, f"{tag}: (line, worst error, fp32 CPU worst error) {bad}"
