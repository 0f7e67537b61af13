"""The TransFuse_S_adapt kernels (csrc/sdpa.hip, csrc/transfuse.hip) per row, under ties, and at the chunk counts a training step runs.

test_gpu_transfuse.py runs each of these kernels at one small shape, on continuous inputs uniform in [-1, 1], and divides the largest error by the largest magnitude
of the whole tensor; the model-level tests above it accept 2e-2 relative L2 per gradient tensor and compare the DeiT block with an operator path that runs the same
kernels.  This file is the kernel-level counterpart of test_gpu_attention.py for that leg.

A. Softmax attention with the domain adapter (T._SDPA and the C ABI): SDPA_SHAPES reach the three fp32-MFMA kernels (N = 256) and the LDS-tiled VALU kernels at
   N = 256, at ragged last tiles (N = 100: 4 rows, N = 37: 5 rows) and at one key per lane (N = 8); each case asserts the kernel family it took.  Five input regimes,
   all from qkv = rnd(B, N, 3C, seed=22): `flat` (as test_softmax_attention_with_domain_adapter: logits of standard deviation 0.3, every probability ~1/N), `sharp`
   (q, k x 3), `saturated` (q, k x 6: the median row maximum of P is 0.9 to 1.0, lse reaches 60), `offset` (k += 12 u, q += 3 u' with u, u' per image and channel,
   shared by all tokens: every query's logits move by a constant of its own, lse spans -23 to +34 -- max subtraction, m + log(sum) and exp(s - lse) at work) and
   `spike` (k of the last token x 8).  Against fp64 torch on the CPU: out, dq, dk, dv by TWO worst-unit statistics, no unit left out -- per (image, head, token) row
   max_d |got - ref| / max_d |ref| over the head's 64 channels, and per (image, channel) column the same quotient over the tokens; the row log-sum-exp (MFMA, through
   the C ABI) and the stored probabilities (VALU) as the worst absolute error.  Bound: FACTOR = 10 x the same statistic of the same formula evaluated by torch in fp32
   on the CPU (the rule and the factor of test_gpu_adapter.py and test_gpu_attention.py: the kernels differ from that baseline in summation order and __expf / __logf
   only).  The measure must be well conditioned, asserted on the two CPU evaluations alone: the fp32 evaluation's own worst unit stays below BASE_LIMIT = 1e-4.
   EXCEPTION, `saturated`: the rows of dq and dk are ill-conditioned there -- a query whose softmax is one-hot has dq = sum_n dS_n k_n ~ 0 as a difference of equal
   numbers (dS_n = P_n (dP_n - sum_m P_m dP_m) with P_n = 1 - 1e-7), and the fp32 CPU evaluation itself is off by up to 100 % in such rows (the test prints the
   figure).  So under `saturated` dq and dk are held by COLUMNS only; out, lse / P and dv keep both statistics.
   The adapter's four gradients keep test_gpu_transfuse.py's bar, 2e-4 of the tensor maximum.  Further: the no-adapter path (a = e = NULL) of both families through
   the C ABI; `a` without `e` is refused with MDVIT_E_SHAPE; the same call twice is bit-identical in every output; image 0 of a batch of three equals the image alone.
B. Pooling under ties.  In the model both pooling kernels read post-ReLU features, where exact zeros tie all the time; test_gpu_transfuse.py feeds continuous values.
   Inputs here are relu(round(2 randn) / 2): a quarter to a half of the 3x3 windows / of the pixels' channel vectors hold a tied maximum (asserted: >= 25 %), and the
   rule "first maximum in (kh, kw) order" / "first argmax over the channels" is restated explicitly and checked against torch's fp64 autograd before it is used.
C. Reductions past their split points: the channel gate at 65 pixel chunks and a half-full second channel block, the spatial gate at four trips per lane, the structure
   loss at 3 and 16 chunks per sample and with a 31-wide window larger than the image, BatchNorm1ch with four groups of 2220 values on 1024 threads, and the stem
   convolution's weight gradient at ppb = 80 on 1024 partial rows.  Each case restates the launch arithmetic it reaches and re-derives it in an assert.

Measured on an MI355X (docs/history.md has the table per tensor, shape and regime): the kernels' worst row / column error is 0.29 to 5.96 x the fp32 CPU evaluation's
(median 1.03; the MFMA kernels 0.44 to 3.72, the VALU kernels at N = 256 mostly 1.00), lse and P 0.78 to 3.30 x, the adapter's gradients at most 2.4e-6 of the tensor
maximum.  Before sdpa_mfma_bwd_rows_kernel took its delta from the recomputed P and dP (sdpa.hip) the rows of dq stood at 5.8 to 10.4 x in `spike` and `sharp`.
Every test prints got, baseline and ratio."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_transfuse import check, dev, grads_of, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu

FACTOR = 10.0          # x the fp32 CPU evaluation's error
BASE_LIMIT = 1e-4      # conditioning: the fp32 CPU evaluation's own worst row / column / element error
PARAM_TOL = 2e-4       # adapter gradients, relative to the tensor maximum (test_softmax_attention_with_domain_adapter's bar)
D = 64                 # head dimension
HID = 192              # the adapter's hidden width (as in test_gpu_transfuse.py)
LABELS = [1, 3, 0]
MDVIT_E_SHAPE = 1      # include/mdvit_hip.h


def _cdiv(a, b):
    return -(-a // b)


# ==== A. softmax attention with the domain adapter ===================================================================================================================
def sdpa_reached(N, mfma):
    """The launch arithmetic of mdvit_sdpa_mfma_* / mdvit_sdpa_* restated.  MFMA (N == 256 only): one workgroup per (head, image), 8 query / key tiles of 32 on 4 waves
    (2 trips each).  VALU: cdiv(N, 32) row tiles (forward, backward rows) and key tiles (backward keys) per (head, image); thread = (row tid / 8, slice tid % 8):
    `last` rows / keys in the last tile, `per_lane` keys per lane of a row's 8 (the last trip ragged unless N % 8 == 0)."""
    if mfma:
        assert N == 256
        return dict(family="mfma", tiles=8, trips=2)
    tiles = _cdiv(N, 32)
    return dict(family="valu", tiles=tiles, last=N - 32 * (tiles - 1), per_lane=_cdiv(N, 8))


# (B, N, heads, mfma, what `sdpa_reached` must say)
SDPA_SHAPES = [
    (2, 256, 6, True, dict(family="mfma", tiles=8, trips=2)),           # the DeiT trunk's shape
    (1, 256, 1, True, dict(family="mfma")),                             # one workgroup in all; one head: the adapter's head softmax is 1
    (3, 256, 3, True, dict(family="mfma")),                             # odd counts both ways
    (2, 256, 6, False, dict(family="valu", tiles=8, last=32, per_lane=32)),      # the VALU kernels at the trunk's shape (the A/B switch)
    (2, 100, 6, False, dict(family="valu", tiles=4, last=4, per_lane=13)),       # ragged: the last tile has 4 rows / keys, the last trip of a row 4 of 8 lanes
    (1, 37, 2, False, dict(family="valu", tiles=2, last=5, per_lane=5)),         # ragged: 5 rows / keys
    (2, 8, 1, False, dict(family="valu", tiles=1, last=8, per_lane=1)),          # one key per lane, 24 of the tile's 32 rows idle
]
REGIMES = ("flat", "sharp", "saturated", "offset", "spike")
ILL_ROWS = {"saturated": ("dq", "dk")}          # regime -> tensors whose ROW statistic is ill-conditioned (top of the file): held by columns only


def _shape_id(s):
    B, N, heads, mfma, _ = s
    return f"B{B}-N{N}-h{heads}-{'mfma' if mfma else 'valu'}"


@pytest.mark.parametrize("shape", SDPA_SHAPES, ids=_shape_id)
def test_the_shape_reaches_the_kernels_it_is_listed_for(shape):
    B, N, heads, mfma, want = shape
    got = sdpa_reached(N, mfma)
    assert {k: got.get(k) for k in want} == want
    assert (N == 256 and heads <= 6) or not mfma          # what _SDPA.forward sends to the MFMA kernels


def make_sdpa_inputs(B, N, heads, regime):
    """fp32 CPU tensors: qkv in the regime, the adapter's four parameters and labels (test_softmax_attention_with_domain_adapter's), the upstream gradient"""
    C = heads * D
    qkv = rnd(B, N, 3 * C, seed=22).clone()
    q, k = qkv[:, :, :C], qkv[:, :, C:2 * C]          # views
    if regime == "sharp":
        q *= 3.0; k *= 3.0
    elif regime == "saturated":
        q *= 6.0; k *= 6.0
    elif regime == "offset":
        k += 12.0 * rnd(B, 1, C, seed=41)
        q += 3.0 * rnd(B, 1, C, seed=42)
    elif regime == "spike":
        k[:, N - 1] *= 8.0
    else:
        assert regime == "flat"
    da = [rnd(HID, 4, seed=23), rnd(HID, seed=24, scale=0.1), rnd(C, HID, seed=25, scale=0.2), rnd(C, seed=26, scale=0.1)]
    lab = F.one_hot(torch.tensor(LABELS[:B]), 4).float()
    return dict(B=B, N=N, heads=heads, C=C, qkv=qkv, da=da, lab=lab, g=rnd(B, N, C, seed=27))


def first_image(inp):
    return dict(inp, B=1, qkv=inp["qkv"][:1].contiguous(), lab=inp["lab"][:1].contiguous(), g=inp["g"][:1].contiguous())


PARAM_NAMES = ("dW1", "db1", "dW2", "db2")


def restated(inp, dtype, adapter=True):
    """the operation in plain torch on the CPU in `dtype` (vision_transformer.py:148-169): y, dq, dk, dv, the adapter's gradients, the row log-sum-exp [B, heads, N]
    and the probabilities [B, heads, N, N] (results as doubles)"""
    B, N, heads, C = inp["B"], inp["N"], inp["heads"], inp["C"]
    qkv = inp["qkv"].detach().clone().to(dtype).requires_grad_(True)          # (clone: .to(float32) of an fp32 tensor IS that tensor)
    params = [t.detach().clone().to(dtype).requires_grad_(True) for t in inp["da"]]
    q, k, v = qkv.reshape(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * D ** -0.5
    P = s.softmax(-1)
    o = P @ v
    if adapter:
        W1, b1, W2, b2 = params
        z = F.linear(F.relu(F.linear(inp["lab"].to(dtype), W1, b1)), W2, b2)
        o = torch.softmax(z.view(B, heads, 1, D), dim=1) * o
    y = o.transpose(1, 2).reshape(B, N, C)
    y.backward(inp["g"].to(dtype))
    dq, dk, dv = [t.double() for t in qkv.grad.split(C, dim=2)]
    return dict(y=y.detach().double(), dq=dq, dk=dk, dv=dv, params=[t.grad.double() for t in params] if adapter else None,
                lse=torch.logsumexp(s.detach(), dim=-1).double(), P=P.detach().double())


def run_op(inp, mfma):
    """T._SDPA forward and backward as Attention_Sup calls it, on the kernel family asked for; `saved` is what the forward kept for the backward besides its inputs:
    the row log-sum-exp [B, heads, N] (MFMA) or the probabilities [B, heads, N, N] (VALU)"""
    from mdvit_amd import transfuse as T
    d = dev()
    qkv = inp["qkv"].detach().to(d).requires_grad_(True)
    params = [t.detach().to(d).requires_grad_(True) for t in inp["da"]]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_use_mfma_sdpa", bool(mfma))
        y = T._SDPA.apply(qkv, inp["lab"].to(d), *params, inp["heads"])
    saved = y.grad_fn.saved_tensors[-1]
    y.backward(inp["g"].to(d))
    torch.cuda.synchronize()
    dq, dk, dv = qkv.grad.split(inp["C"], dim=2)
    return dict(y=y.detach(), dqkv=qkv.grad, dq=dq, dk=dk, dv=dv, params=[t.grad for t in params], saved=saved.detach())


def run_abi(inp, mfma, adapter=True):
    """mdvit_sdpa_mfma_fwd / _bwd or mdvit_sdpa_fwd / _bwd through the C ABI (adapter=False: a = e = NULL).  Outputs are pre-filled with NaN: an element a ragged tile
    leaves unwritten cannot pass."""
    from mdvit_amd import ops
    from mdvit_amd._lib import call
    from mdvit_amd.ops import _p, _stream
    d = dev()
    B, N, heads, C = inp["B"], inp["N"], inp["heads"], inp["C"]
    nan = float("nan")
    qkv, g = inp["qkv"].to(d), inp["g"].to(d)
    a = ops.domain_adapter(inp["lab"].to(d), *[t.to(d) for t in inp["da"]], heads) if adapter else None
    out = torch.full((B, N, C), nan, device=d)
    saved = torch.full((B, heads, N) if mfma else (B, heads, N, N), nan, device=d)
    call("mdvit_sdpa_mfma_fwd" if mfma else "mdvit_sdpa_fwd", _p(qkv), _p(a), _p(out), _p(saved), B, N, C, heads, _stream())
    dqkv = torch.full((B, N, 3 * C), nan, device=d)
    e = torch.full((B, C), nan, device=d) if adapter else None
    scratch = torch.empty((2, B, heads, N) if mfma else (B, heads, N, N), device=d)
    call("mdvit_sdpa_mfma_bwd" if mfma else "mdvit_sdpa_bwd", _p(g), _p(qkv), _p(saved), _p(out), _p(a), _p(dqkv), _p(e), _p(scratch), B, N, C, heads, _stream())
    torch.cuda.synchronize()
    dq, dk, dv = dqkv.split(C, dim=2)
    return dict(y=out, dqkv=dqkv, dq=dq, dk=dk, dv=dv, e=e, saved=saved, lse=saved if mfma else None, P=None if mfma else saved)


# ---- measures -------------------------------------------------------------------------------------------------------------------------------------------------------
def row_errors(got, ref):
    """[B, N, heads]: per (image, head, token) row of a [B, N, heads * 64] tensor, max_d |got - ref| / max_d |ref| over the head's 64 channels"""
    got, ref = got.detach().double().cpu(), ref.double()
    B, N, C = ref.shape
    return (got - ref).abs().view(B, N, C // D, D).amax(dim=3) / ref.abs().view(B, N, C // D, D).amax(dim=3)


def column_errors(got, ref):
    """[B, C]: per (image, channel) column, max_n |got - ref| / max_n |ref| over the tokens"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def absolute_errors(got, ref):
    """|got - ref| per element (lse: per (image, head, query); P: its maximum over a row is the row's statistic, the maximum over all of it the worst row's)"""
    return (got.detach().double().cpu() - ref.double()).abs()


UNIT_MEASURES = (("row", row_errors), ("column", column_errors))


def assert_within(got, ref, base, names, where, ill_rows=()):
    """worst error of `got` against FACTOR x the worst error of the fp32 CPU evaluation `base`, both against the fp64 `ref`; every figure is printed.  The conditioning
    guard (the fp32 evaluation's own worst unit <= BASE_LIMIT) is asserted on the CPU evaluations alone.  ill_rows: tensors whose row statistic is printed, not held."""
    bad, loose = [], []
    for name in names:
        assert tuple(got[name].shape) == tuple(ref[name].shape), name
        measures = (("abs", absolute_errors),) if name in ("lse", "P") else UNIT_MEASURES
        for kind, fn in measures:
            e_got, e_base = float(fn(got[name], ref[name]).max()), float(fn(base[name], ref[name]).max())
            held = not (kind == "row" and name in ill_rows)
            print(f"{where} {name} worst {kind}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}"
                  + ("" if held else "  (ill-conditioned: not held)"))
            if not held:
                continue
            if not e_base <= BASE_LIMIT:
                loose.append((name, kind, e_base))
            if not (math.isfinite(e_got) and e_got <= FACTOR * e_base):
                bad.append((name, kind, e_got, e_base))
    assert not loose, f"{where}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (tensor, unit, worst error) {loose}"
    assert not bad, f"{where}: (tensor, unit, worst error, fp32 CPU worst error) {bad}"


# ---- one case = one shape in one regime: the references are computed once and shared by the tests below ---------------------------------------------------------------
SDPA_CASES = [(s, r) for s in SDPA_SHAPES for r in REGIMES]


@pytest.fixture(scope="module", params=SDPA_CASES, ids=lambda c: _shape_id(c[0]) + "-" + c[1])
def case(request):
    (B, N, heads, mfma, _), regime = request.param
    inp = make_sdpa_inputs(B, N, heads, regime)
    return dict(where=f"({B},{N},{heads}) {'mfma' if mfma else 'valu'} {regime}", regime=regime, mfma=mfma, inp=inp, ref=restated(inp, torch.float64),
                base=restated(inp, torch.float32), op=run_op(inp, mfma), abi=run_abi(inp, mfma))


def test_kernel_family_and_the_softmax_state(case):
    """the operator took the kernel family the case is listed for (what it saved is [B, heads, N] on the MFMA path, [B, heads, N, N] on the VALU path); the C ABI call's
    results are the operator's bit for bit; MFMA: lse against fp64 logsumexp, VALU: the stored probabilities against the fp64 softmax -- worst absolute error"""
    inp, op, abi = case["inp"], case["op"], case["abi"]
    B, N, heads = inp["B"], inp["N"], inp["heads"]
    assert tuple(op["saved"].shape) == ((B, heads, N) if case["mfma"] else (B, heads, N, N)), "the operator ran the other kernel family"
    for name in ("y", "dqkv", "saved"):
        assert torch.equal(abi[name], op[name]), name
    assert_within(abi, case["ref"], case["base"], ("lse",) if case["mfma"] else ("P",), case["where"])
    if not case["mfma"]:
        rows = abi["P"].double().sum(dim=-1)
        assert float((rows - 1).abs().max()) <= 1e-5, "a row of P does not sum to 1"


def test_output_and_data_gradients_by_the_worst_row_and_column(case):
    assert_within(case["op"], case["ref"], case["base"], ("y", "dq", "dk", "dv"), case["where"], ill_rows=ILL_ROWS.get(case["regime"], ()))


def test_adapter_gradients(case):
    """dW1, db1, dW2, db2 (the carrier e = sum_n g out reaches them): 2e-4 of the tensor maximum; the ratio to the fp32 CPU evaluation is printed for the record.  One
    head: the head softmax is constant 1 and all four gradients are exactly zero."""
    from test_gpu_transfuse import relerr
    bad = []
    for name, got, ref, base in zip(PARAM_NAMES, case["op"]["params"], case["ref"]["params"], case["base"]["params"]):
        assert got is not None and tuple(got.shape) == tuple(ref.shape), name
        if case["inp"]["heads"] == 1:          # nothing to divide by: |dW| <= |e| |h| with |e| <= N max|y| (|g| <= 1), held to fp32 round-off of a = 1 times that
            assert float(ref.abs().max()) == 0.0 and float(got.abs().max()) <= 1e-6 * case["inp"]["N"] * float(case["ref"]["y"].abs().max()), name
            continue
        e_got, e_base = relerr(got, ref), relerr(base, ref)
        print(f"{case['where']} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}")
        if not (math.isfinite(e_got) and e_got <= PARAM_TOL):
            bad.append((name, e_got))
    assert not bad, f"{case['where']}: rel-to-max error above {PARAM_TOL}: {bad}"


@pytest.mark.parametrize("shape", [SDPA_SHAPES[0], SDPA_SHAPES[5]], ids=_shape_id)
def test_no_adapter_path_through_the_c_abi(shape):
    """a = e = NULL (plain softmax attention), `sharp`: out, lse / P, dq, dk, dv as above; with `a` given and `e` NULL the backward is refused with MDVIT_E_SHAPE
    before anything is launched"""
    from mdvit_amd import ops
    from mdvit_amd._lib import MdvitHipError, call
    from mdvit_amd.ops import _p, _stream
    B, N, heads, mfma, _ = shape
    inp = make_sdpa_inputs(B, N, heads, "sharp")
    ref, base = restated(inp, torch.float64, adapter=False), restated(inp, torch.float32, adapter=False)
    got = run_abi(inp, mfma, adapter=False)
    assert_within(got, ref, base, ("lse" if mfma else "P", "y", "dq", "dk", "dv"), f"({B},{N},{heads}) {'mfma' if mfma else 'valu'} sharp, no adapter")
    d = dev()
    a = ops.domain_adapter(inp["lab"].to(d), *[t.to(d) for t in inp["da"]], heads)
    g, qkv = inp["g"].to(d), inp["qkv"].to(d)
    dqkv = torch.full_like(qkv, 7.0)
    scratch = torch.empty((2, B, heads, N) if mfma else (B, heads, N, N), device=d)
    with pytest.raises(MdvitHipError, match=rf"\(code {MDVIT_E_SHAPE}\)"):
        call("mdvit_sdpa_mfma_bwd" if mfma else "mdvit_sdpa_bwd", _p(g), _p(qkv), _p(got["saved"]), _p(got["y"]), _p(a), _p(dqkv), None, _p(scratch),
             B, N, inp["C"], heads, _stream())
    torch.cuda.synchronize()
    assert bool((dqkv == 7.0).all()), "the refused call wrote its output"


@pytest.mark.parametrize("shape", [SDPA_SHAPES[0], SDPA_SHAPES[4]], ids=_shape_id)
def test_same_sdpa_call_twice_is_bit_identical(shape):
    B, N, heads, mfma, _ = shape
    inp = make_sdpa_inputs(B, N, heads, "offset")
    a, b = run_op(inp, mfma), run_op(inp, mfma)
    for name in ("y", "dqkv", "saved"):
        assert torch.equal(a[name], b[name]), name
    for name, u, v in zip(PARAM_NAMES, a["params"], b["params"]):
        assert torch.equal(u, v), name
    fa, fb = run_abi(inp, mfma), run_abi(inp, mfma)
    for name in ("y", "dqkv", "saved", "e"):
        assert torch.equal(fa[name], fb[name]), name


def test_an_image_does_not_depend_on_the_batch_it_is_in():
    """(3, 256, 3), `sharp`: out, lse and dqkv of image 0 equal a B = 1 call on that image alone, bit for bit (one workgroup per (head, image) in all three kernels,
    four per image in the prep pass)"""
    B, N, heads, mfma, _ = SDPA_SHAPES[2]
    inp3 = make_sdpa_inputs(B, N, heads, "sharp")
    inp1 = first_image(inp3)
    o3, o1 = run_op(inp3, mfma), run_op(inp1, mfma)
    for name in ("y", "saved", "dqkv"):
        assert torch.equal(o3[name][:1], o1[name]), name
    f3, f1 = run_abi(inp3, mfma), run_abi(inp1, mfma)
    for name in ("y", "saved", "dqkv", "e"):
        assert torch.equal(f3[name][:1], f1[name]), name


# ==== B. pooling under ties ===========================================================================================================================================
def quantised(*shape, seed):
    """relu(round(2 randn) / 2): multiples of 0.5 with ~40 % exact zeros, as a post-ReLU feature map has them"""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.round(2.0 * torch.randn(shape, generator=g)) / 2.0)


def _windows3x3s2(x):
    """[B, C, 9, Ho * Wo]: the 3x3 / stride 2 / pad 1 windows of an NCHW tensor in (kh, kw) order, padding = -inf"""
    B, C, H, W = x.shape
    return F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)


def _first_max(v, dim):
    """one-hot mask of the FIRST maximum along dim"""
    hit = v == v.amax(dim=dim, keepdim=True)
    return hit & (hit.int().cumsum(dim=dim) == 1)


# (B, H, W, C): odd H (the last window row is clipped at the bottom), even W; and a tiny one with odd W (clipped at the right), one partial block
@pytest.mark.parametrize("B,H,W,C", [(2, 21, 30, 64), (1, 8, 9, 4)])
def test_maxpool_breaks_ties_by_the_first_maximum(B, H, W, C):
    """_MaxPool on quantised post-ReLU values: y equals fp64 torch exactly, dx (each value a sum of at most four gradient values: 1e-6 of the tensor maximum) shows the
    tap chosen.  One (image, channel) plane is entirely negative: a padding tap that took part in the maximum would win every border window there."""
    from mdvit_amd import transfuse as T
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    # launch arithmetic: thread = output element, 256 per workgroup, one trip (the grid covers the tensor); the last workgroup is partial
    total = B * Ho * Wo * C
    assert (total, _cdiv(total, 256), total % 256 != 0) == {(2, 21, 30, 64): (21120, 83, True), (1, 8, 9, 4): (80, 1, True)}[(B, H, W, C)]
    x = quantised(B, C, H, W, seed=50)
    x[0, C - 1] = -0.5 - quantised(H, W, seed=51)          # all negative, still tied
    g = rnd(B, Ho, Wo, C, seed=52)
    win = _windows3x3s2(x.double())
    tied = float(((win == win.amax(dim=2, keepdim=True)).sum(dim=2) > 1).double().mean())
    print(f"maxpool ({B},{H},{W},{C}): {100 * tied:.1f} % of the windows hold a tied maximum")
    assert tied >= 0.25
    ref, gr = grads_of(lambda x: nhwc(F.max_pool2d(x.double(), 3, 2, 1)), [x], g.double())
    # the rule, restated: the whole gradient goes to the first maximum in (kh, kw) order -- torch's fp64 autograd follows it (its gradient arrives rounded to the
    # fp32 leaf: 6e-8; a tie broken the other way moves a whole gradient value)
    onehot = _first_max(win, 2).double() * nchw(g.double()).reshape(B, C, 1, Ho * Wo)
    ruled = F.fold(onehot.view(B, C * 9, Ho * Wo), (H + 2, W + 2), 3, stride=2)[:, :, 1:-1, 1:-1]
    assert float((ruled - gr[0]).abs().max()) <= 1e-6 * float(gr[0].abs().max()), "torch's max_pool2d backward does not follow the first-maximum rule here"
    out, go = grads_of(lambda x: T._MaxPool.apply(x), [nhwc(x).to(dev())], g)
    assert torch.equal(out.detach().cpu().double(), ref.detach()), "maxpool y is not exact"
    assert bool((out.detach()[0, :, :, C - 1] < 0).all()), "a padding tap won in the all-negative plane"
    e = float((nchw(go[0]).cpu().double() - gr[0]).abs().max() / gr[0].abs().max())
    print(f"maxpool ({B},{H},{W},{C}) dx: rel-to-max error {e:.3e}  bound 1e-6")
    check(nchw(go[0]), gr[0], tol=1e-6, name="maxpool dx under ties")


# C: less than one trip of the wave (24 idle lanes), exactly one, four (a step runs 64, 128 and 256)
@pytest.mark.parametrize("C,trips,idle", [(40, 1, 24), (64, 1, 0), (256, 4, 0)])
def test_chanpool_breaks_ties_by_the_first_channel(C, trips, idle):
    """_ChanPool on quantised post-ReLU values, some pixels all zero (a C-way tie): both outputs against fp64 (the maximum exactly; the mean of exactly representable
    sums to 1e-6) and dx, which shows the index chosen"""
    from mdvit_amd import transfuse as T
    B, H, W = 2, 7, 9
    M = B * H * W
    # launch arithmetic: one wave per pixel, 4 per workgroup: 32 workgroups, the last holds 2 pixels; a lane walks channels lane, lane + 64, ...
    assert (M, _cdiv(M, 4), M % 4) == (126, 32, 2) and (_cdiv(C, 64), 64 * _cdiv(C, 64) - C) == (trips, idle)
    x = quantised(B, H, W, C, seed=60)
    x[0, 0, :3] = 0.0; x[1, H - 1, W - 1] = 0.0          # all-zero pixels, the last pixel among them
    g = rnd(B, H, W, 2, seed=61)
    xd = x.double()
    tied = float(((xd == xd.amax(dim=-1, keepdim=True)).sum(dim=-1) > 1).double().mean())
    print(f"chanpool C={C}: {100 * tied:.1f} % of the pixels hold a tied maximum")
    assert tied >= 0.25
    ref, gr = grads_of(lambda x: torch.stack((x.double().max(-1)[0], x.double().mean(-1)), -1), [x], g.double())
    ruled = _first_max(xd, -1).double() * g.double()[..., :1] + g.double()[..., 1:] / C
    assert float((ruled - gr[0]).abs().max()) <= 1e-6 * float(gr[0].abs().max()), "torch's max backward does not follow the first-argmax rule here"
    out, go = grads_of(lambda x: T._ChanPool.apply(x), [x.to(dev())], g)
    assert torch.equal(out.detach()[..., 0].cpu().double(), ref.detach()[..., 0]), "channel maximum is not exact"
    for name, a, r in (("mean", out[..., 1], ref[..., 1]), ("dx", go[0], gr[0])):
        e = float((a.detach().cpu().double() - r.detach()).abs().max() / r.detach().abs().max())
        print(f"chanpool C={C} {name}: rel-to-max error {e:.3e}  bound 1e-6")
        check(a, r, tol=1e-6, name=f"channel pool {name} under ties")


# ==== C. reductions past their split points ===========================================================================================================================
# (B, P, C, chunks, pixels in the last chunk, channel blocks, channels in the last block)
@pytest.mark.parametrize("B,P,C,want", [(2, 4100, 64, (65, 4, 1, 64)),          # 65 chunks (a step runs 64), the last holds 4 pixels: one per pixel slot
                                        (2, 1024, 96, (16, 64, 2, 32))])         # a second, half-full channel block
def test_channel_gate_past_one_chunk(B, P, C, want):
    """_Gate mode 1: gate_bwd_channel_kernel on (channel block, 64-pixel chunk, image) workgroups, one partial row per chunk, added in order by the final kernel"""
    from mdvit_amd import transfuse as T
    nchunk, nblock = _cdiv(P, 64), _cdiv(C, 64)
    assert (nchunk, P - 64 * (nchunk - 1), nblock, C - 64 * (nblock - 1)) == want
    x, s, g = rnd(B, P, C, seed=70), rnd(B, C, seed=71, scale=2.0), rnd(B, P, C, seed=72)
    ref, gr = grads_of(lambda x, s: torch.sigmoid(s.double()).view(B, 1, C) * x.double(), [x, s], g.double())
    out, go = grads_of(lambda x, s: T._Gate.apply(x, s, 1), [x.to(dev()), s.to(dev())], g)
    _report(f"channel gate ({B},{P},{C})", (("y", out, ref), ("dx", go[0], gr[0]), ("ds", go[1], gr[1])), 1e-4)


def _report(where, triples, tol):
    from test_gpu_transfuse import relerr
    for name, a, r in triples:
        print(f"{where} {name}: rel-to-max error {relerr(a, r):.3e}  bound {tol:.0e}")
    for name, a, r in triples:
        check(a, r, tol=tol, name=f"{where} {name}")


@pytest.mark.parametrize("C,trips,idle", [(256, 4, 0), (40, 1, 24)])
def test_spatial_gate_past_one_trip(C, trips, idle):
    """_Gate mode 0: gate_bwd_spatial_kernel, one wave per pixel; a lane walks channels lane, lane + 64, ... (a step runs C = 64 and 256)"""
    from mdvit_amd import transfuse as T
    B, P = 2, 51
    # 102 pixels, 4 per workgroup: 26 workgroups, the last holds 2
    assert (_cdiv(B * P, 4), (B * P) % 4) == (26, 2) and (_cdiv(C, 64), 64 * _cdiv(C, 64) - C) == (trips, idle)
    x, s, g = rnd(B, P, C, seed=73), rnd(B, P, seed=74, scale=2.0), rnd(B, P, C, seed=75)
    ref, gr = grads_of(lambda x, s: torch.sigmoid(s.double()).view(B, P, 1) * x.double(), [x, s], g.double())
    out, go = grads_of(lambda x, s: T._Gate.apply(x, s, 0), [x.to(dev()), s.to(dev())], g)
    _report(f"spatial gate C={C}", (("y", out, ref), ("dx", go[0], gr[0]), ("ds", go[1], gr[1])), 1e-4)


# (B, H, W, logit scale, chunks per sample)
@pytest.mark.parametrize("B,H,W,scale,chunks", [(2, 96, 96, 4.0, 3),            # 3 chunks of 3072
                                                (2, 256, 256, 4.0, 16),         # the step's count
                                                (1, 20, 45, 4.0, 1),            # the 31-wide window is taller than the image and wider than most of it: still / 961
                                                (2, 96, 96, 30.0, 3)])          # saturated sigmoid: everything finite
def test_structure_loss_past_one_chunk(B, H, W, scale, chunks):
    """sl_sums_kernel with several workgroups per sample (double atomics into the zeroed sums), box31_* at the image border.  Bars: loss 1e-5 relative and weit 1e-5 of
    the maximum (test_structure_loss_and_patch_embed_pieces'); dpred 2e-4 of EACH SAMPLE's own maximum (that test's 2e-4, per sample: samples differ in S1)."""
    from mdvit_amd import transfuse as T
    from oracle import transfuse_ref as R
    from oracle.gen_golden import synth_label
    HW = H * W
    assert min(_cdiv(HW, 4096), 64) == chunks          # mdvit_structure_loss_fwd's grid.y
    assert (H < 31 and W < 2 * 31) == ((H, W) == (20, 45))          # no pixel of (20, 45) has its whole window inside the image
    mask = synth_label(78, B, H, W)
    assert 0.02 < float(mask.mean()) < 0.98
    pred = rnd(B, 1, H, W, seed=28, scale=scale)
    weit_ref = 1 + 5 * torch.abs(F.avg_pool2d(mask.double(), 31, 1, 15) - mask.double())
    weit = T.structure_weight(mask.to(dev()))
    _report(f"structure ({B},{H},{W})", (("weit", weit, weit_ref),), 1e-5)
    pr = pred.clone().double().requires_grad_(True)
    lr = R.structure_loss(pr, mask.double())
    lr.backward()
    pg = pred.to(dev()).requires_grad_(True)
    lg = T.structure_loss(pg, mask.to(dev()))
    (2.5 * lg).backward()
    got_l, ref_l = float(lg.detach()), float(lr.detach())
    e = abs(got_l - ref_l) / abs(ref_l)
    print(f"structure ({B},{H},{W}) scale {scale}: loss {got_l:.7f}  fp64 {ref_l:.7f}  relative error {e:.3e}  bound 1e-5")
    assert math.isfinite(got_l) and e <= 1e-5
    got, ref = pg.grad.cpu().double().view(B, -1), 2.5 * pr.grad.view(B, -1)
    assert bool(torch.isfinite(got).all())
    per_sample = (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)
    print(f"structure ({B},{H},{W}) scale {scale}: dpred per sample, rel-to-max error {[f'{float(v):.3e}' for v in per_sample]}  bound 2e-4")
    assert float(per_sample.max()) <= 2e-4


@pytest.mark.parametrize("training", [True, False])
def test_single_channel_batchnorm_in_four_groups(training):
    """BatchNorm1ch under ops.bn_groups(4): 8 maps of 30 x 37 = four groups of 2220 values on 1024 threads (trips of 3, 3, 2 ... per thread), a mean far from zero
    (3.0 + 0.5 rnd) against fp64 BatchNorm2d(1) applied to the four groups in order; in eval mode the groups do not apply and the reference sees the whole batch"""
    from mdvit_amd import ops
    from mdvit_amd import transfuse as T
    G, B, H, W = 4, 8, 30, 37
    Mg = B // G * H * W
    assert Mg == 2220 and Mg % 1024 == 172 and _cdiv(Mg, 1024) == 3
    x = 3.0 + 0.5 * rnd(B, H, W, seed=80)
    gg = rnd(B, H, W, seed=81)
    ga, be, rm, rv = torch.tensor([1.3]), torch.tensor([-0.2]), torch.tensor([0.1]), torch.tensor([1.7])
    bn = torch.nn.BatchNorm2d(1).double()
    with torch.no_grad():
        bn.weight.copy_(ga); bn.bias.copy_(be); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(training)
    xr = x.clone().double().requires_grad_(True)
    if training:
        yr = torch.cat([bn(xr[i * (B // G):(i + 1) * (B // G)].view(B // G, 1, H, W)) for i in range(G)]).view(B, H, W)
    else:
        yr = bn(xr.view(B, 1, H, W)).view(B, H, W)
    yr.backward(gg.double())
    m = T.BatchNorm1ch().to(dev())
    with torch.no_grad():
        m.weight.copy_(ga); m.bias.copy_(be); m.running_mean.copy_(rm); m.running_var.copy_(rv)
    m.train(training)
    xg = x.to(dev()).requires_grad_(True)
    with ops.bn_groups(G):
        y = m(xg)
    y.backward(gg.to(dev()))
    _report(f"bn1 groups={G} train={training}", (("y", y, yr), ("dx", xg.grad, xr.grad), ("dgamma", m.weight.grad, bn.weight.grad), ("dbeta", m.bias.grad, bn.bias.grad),
                                                 ("running_mean", m.running_mean, bn.running_mean), ("running_var", m.running_var, bn.running_var)), 1e-4)
    assert int(m.num_batches_tracked) == int(bn.num_batches_tracked) == (G if training else 0)


def test_stem_conv_weight_gradient_past_the_ppb_floor():
    """_ImgConv's weight gradient at 5 x 3 x 256 x 256, Cout = 64: 81920 output pixels -> 80 per workgroup (the floor is 64) on 1024 partial rows; against fp64 and
    against the im2col + GEMM path (stem_conv7), each held to 1e-4 of the maximum, so the two to 2e-4 of each other"""
    from mdvit_amd import transfuse as T
    B, S, Cout = 5, 256, 64
    npix = B * (S // 2) * (S // 2)
    ppb = max(64, _cdiv(npix, 1024))          # mdvit_imgconv_wgrad
    assert (npix, ppb, _cdiv(npix, ppb)) == (81920, 80, 1024)
    img, w, g = rnd(B, 3, S, S, seed=1), rnd(Cout, 3, 7, 7, seed=2, scale=0.1), rnd(B, S // 2, S // 2, Cout, seed=3)
    ref, gr = grads_of(lambda w: nhwc(F.conv2d(img.double(), w.double(), None, 2, 3)), [w], g.double())
    out, go = grads_of(lambda w: T._ImgConv.apply(img.to(dev()), w), [w.to(dev())], g)
    out2, go2 = grads_of(lambda w: T.stem_conv7(img.to(dev()), w), [w.to(dev())], g)
    _report("conv1 5x3x256x256", (("y", out, ref), ("dw", go[0], gr[0]), ("y (im2col + GEMM)", out2, ref), ("dw (im2col + GEMM)", go2[0], gr[0])), 1e-4)
    _report("conv1 5x3x256x256", (("dw against the im2col + GEMM path", go[0], go2[0]),), 2e-4)
