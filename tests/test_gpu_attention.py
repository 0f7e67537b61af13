"""The attention core (csrc/attn.hip) at the tile counts a training step runs, on inputs that make the online softmax rescale, measured per column.

test_factor_att_core (test_gpu_kernels.py) runs head dim 40 / 64 on ONE 64-token tile, on K uniform in [-1.5, 1.5] (every exp(m_old - m_new) is ~1), and divides
the largest error by the largest magnitude of the whole tensor.  Here:
  * shapes (SHAPES below) that walk several tiles per workgroup, several partial rows per image, every combine kernel, every tiles-per-workgroup of the MFMA
    backward with ragged last workgroups, and the three-dimensional launch -- each case states the launch arithmetic it reaches, and a test re-derives it;
  * three input regimes: `flat` (as test_factor_att_core), `ramp` (K gets a per-image, per-channel linear ramp over the tokens, slopes in [-30, 30], minus 40: rising
    columns raise the running maximum in every tile by another amount per channel, falling ones leave it fixed while later tiles underflow, and the offset makes a
    padded zero row that is treated as a token dominate its column) and `spike` (+25 on K at the LAST token of an image, odd channels only: the rescale fires once, in
    the last -- ragged -- sub-tile of the last workgroup);
  * the forward state through the C ABI: kmax bit-equal to the column maximum, ksum per element, Mmat per (image, channel) row;
  * y, dq, dk, dv by the WORST (image, channel) column: max_n |got - fp64| / max_n |fp64| -- no column is left out;
  * bound: FACTOR x the same statistic of the same formula evaluated by torch in fp32 on the CPU (the rule of test_gpu_adapter.py: the kernels differ from that
    baseline in summation order and expf only).  Parameter gradients keep test_factor_att_core's 3e-4 of the tensor maximum.
  * the measure must be well conditioned, which is asserted on the two CPU evaluations alone: the fp32 evaluation's own worst column stays below BASE_LIMIT = 1e-4,
    so FACTOR x it holds every column to 1e-3 of ITS OWN maximum (test_gpu_kernels.py's north-star bar, per column instead of per tensor).  (A floor on the column
    maxima relative to the tensor maximum does not say that: with these inputs the adapter alone spreads the column maxima of y over 1 : 6e-4 at C = 512 -- harmless,
    a column's error scales with it -- while the one ill-conditioned family has no small neighbours to compare with.)  That family is dk in the spiked columns of
    `spike`: dk = P (x - sum_m P_m x_m) with P = 1 - 1e-8 at the spiked token is a difference of equal numbers, the fp32 evaluation itself is wrong by more than 100 %
    there, and the kernels by 10 to 1400 times that: torch forms the subtrahend as a sum over the TOKENS in which the spiked token's term is x_N bit for bit (the
    rounding of x_N cancels, what is lost is the 1e-8 x_N itself), while the kernels form it as a sum over the head's CHANNELS from the stored M = softmax(k)^T v (s_tc in fa_bwd_apply3_kernel): two Ch-term dot products rounded independently, an ordinary absolute
    error of a few ulp of the operands against a column maximum of 1e-8 of them.  So for dk in `spike` the baseline is the fp32 CPU evaluation of THAT algebraic form
    (dk_in_the_kernels_form, checked against autograd in fp64): all columns are held to FACTOR x it, without the conditioning guard; the columns without a spike are
    ADDITIONALLY held to the common baseline with the guard; and the spiked ones once more in absolute terms.
Measured on an MI355X: 0.07 to 1.3 x the fp32 CPU evaluation's error on every tensor and shape (docs/history.md has the table).  Every test prints got, baseline and
ratio."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import _attn_ref, dev, relerr, rnd

pytestmark = pytest.mark.gpu

FACTOR = 10.0          # x the fp32 CPU evaluation's error
PARAM_TOL = 3e-4       # parameter gradients, relative to the tensor maximum (test_factor_att_core's bar)
BASE_LIMIT = 1e-4      # conditioning: the fp32 CPU evaluation's own worst column / row / element error (FACTOR x it = 1e-3, the north-star bar, per column)
LABELS = [2, 0, 3, 1]


def _cdiv(a, b):
    return -(-a // b)


def reached(B, H, W, C, heads):
    """The host-side launch arithmetic of mdvit_factoratt_fwd / _bwd restated (FA_T = 64, fa_nsub, the combine choice, the tiles-per-workgroup loop of the MFMA
    backward): which code a shape runs.
      t64 64-token tiles per image; nsub tiles a workgroup of the partial kernels walks; rows partial rows per image (the backward's NTS); combine the LPO of
      fa_combine_softmax_kernel; and at head dim >= 32: t32 32-token tiles, tpb tiles per workgroup of fa_bwd_apply3_kernel, last the tiles of its last workgroup,
      xcd its one-dimensional (1) or three-dimensional (0) launch."""
    N, Ch = H * W, C // heads
    t64 = _cdiv(N, 64)
    nsub = 8 if t64 >= 128 else (4 if t64 >= 64 else (2 if t64 >= 16 else 1))
    rows = _cdiv(t64, nsub)
    r = dict(t64=t64, nsub=nsub, rows=rows, combine=32 if rows > 8 else (4 if rows > 2 else 1), tail=N - 64 * (t64 - 1))
    if Ch >= 32:
        t32, tpb = _cdiv(N, 32), 8
        while tpb > 2 and _cdiv(t32, tpb) * heads * B < 256:
            tpb //= 2
        gx = _cdiv(t32, tpb)
        r.update(t32=t32, tpb=tpb, last=t32 - (gx - 1) * tpb, xcd=int((gx * heads * B) % 8 == 0))
    return r


ALL = ("flat", "ramp", "spike")
# (B, H, W, C, heads, (s3, s5, s7), regimes, what `reached` must say)
SHAPES = [
    # a step's stage-2 image: two tiles per workgroup (ONE rescale of the MFMA accumulators, one prefetch), 8 partial rows, combine<4>
    (1, 32, 32, 320, 8, (2, 3, 3), ALL, dict(t64=16, nsub=2, rows=8, combine=4, tpb=2, xcd=1)),
    # odd tile count: the last workgroup of the partial kernels leaves at `tile >= NT`; its only tile has 3 tokens; 10 partial rows: combine<32> and the second group of
    # eight in the backward's dM sum; four tiles per workgroup in the MFMA backward, the last workgroup holds one ragged 32-token tile of 37
    (4, 35, 33, 320, 8, (2, 3, 3), ALL, dict(t64=19, tail=3, nsub=2, rows=10, combine=32, t32=37, tpb=4, last=1, xcd=1)),
    # eight tiles per workgroup in the MFMA backward, the last workgroup holds one of 65: its wave slot 1 has no tile
    (4, 46, 45, 320, 8, (2, 3, 3), ALL, dict(t64=33, nsub=2, rows=17, combine=32, t32=65, tpb=8, last=1, xcd=1)),
    # four tiles per workgroup: three rescales in a row
    (1, 64, 64, 320, 8, (2, 3, 3), ALL, dict(t64=64, nsub=4, rows=16, combine=32, tpb=4, xcd=1)),
    # a step's stage-3 image at head dim 64: one tile per workgroup, four partial rows, combine<4>
    (4, 16, 16, 512, 8, (2, 3, 3), ALL, dict(t64=4, nsub=1, rows=4, combine=4, tpb=2, xcd=1)),
    # head dim 64 with two tiles per workgroup, the odd tile count, combine<32>, four tiles per workgroup with a ragged last one
    (4, 35, 33, 512, 8, (2, 3, 3), ALL, dict(t64=19, tail=3, nsub=2, rows=10, combine=32, t32=37, tpb=4, last=1, xcd=1)),
    # head counts that are no multiple of 8 with an odd workgroup count (19 x 4 and 19 x 3): the three-dimensional launch of fa_bwd_apply3_kernel
    (1, 35, 33, 160, 4, (1, 1, 2), ALL, dict(t64=19, nsub=2, rows=10, combine=32, t32=37, tpb=2, last=1, xcd=0)),
    (1, 35, 33, 192, 3, (1, 1, 1), ALL, dict(t64=19, nsub=2, rows=10, combine=32, t32=37, tpb=2, last=1, xcd=0)),
    # the streaming kernels at head dim 8 / 16 (fa_partial_s8, fa_bwd_apply_tab; flat: test_factor_att_core)
    (3, 33, 47, 64, 8, (2, 3, 3), ("ramp", "spike"), dict(t64=25, tail=15, nsub=2, rows=13, combine=32)),
    (2, 50, 50, 128, 8, (2, 3, 3), ("ramp", "spike"), dict(t64=40, tail=4, nsub=2, rows=20, combine=32)),
]


def _shape_id(s):
    B, H, W, C, heads, splits, _, want = s
    return f"B{B}-{H}x{W}-C{C}-h{heads}[" + ",".join(f"{k}={v}" for k, v in want.items()) + "]"


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_the_shape_reaches_the_code_it_is_listed_for(shape):
    B, H, W, C, heads, splits, _, want = shape
    got = reached(B, H, W, C, heads)
    assert {k: got.get(k) for k in want} == want
    assert sum(splits) == heads and C % heads == 0


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, H, W, C, heads, splits, regime):
    """fp32 CPU tensors: qkv, the six window parameters, the adapter's four (test_factor_att_core's), the labels and the upstream gradient"""
    Ch, N, hid = C // heads, H * W, max(C // 2, 4)
    s3, s5, s7 = splits
    qkv = rnd(B, N, 3 * C, seed=130, scale=1.5)
    if regime == "ramp":
        slope = rnd(B, C, seed=142, scale=30.0)
        qkv[:, :, C:2 * C] += torch.linspace(0, 1, N)[None, :, None] * slope[:, None, :] - 40.0
    elif regime == "spike":
        qkv[:, N - 1, C + 1:2 * C:2] += 25.0
    else:
        assert regime == "flat"
    crpe = [rnd(s3 * Ch, 1, 3, 3, seed=131, scale=0.3), rnd(s3 * Ch, seed=132, scale=0.1), rnd(s5 * Ch, 1, 5, 5, seed=133, scale=0.2), rnd(s5 * Ch, seed=134, scale=0.1),
            rnd(s7 * Ch, 1, 7, 7, seed=135, scale=0.15), rnd(s7 * Ch, seed=136, scale=0.1)]
    da = [rnd(hid, 4, seed=137, scale=1.5), rnd(hid, seed=138, scale=0.1), rnd(C, hid, seed=139, scale=3 / hid ** 0.5), rnd(C, seed=140, scale=0.1)]
    lab = F.one_hot(torch.tensor(LABELS[:B]), 4).float()
    return dict(B=B, H=H, W=W, C=C, heads=heads, splits=splits, qkv=qkv, crpe=crpe, da=da, lab=lab, g=rnd(B, N, C, seed=141))


def first_image(inp):
    return dict(inp, B=1, qkv=inp["qkv"][:1].contiguous(), lab=inp["lab"][:1].contiguous(), g=inp["g"][:1].contiguous())


PARAM_NAMES = ("dw3", "db3", "dw5", "db5", "dw7", "db7", "dW1", "db1", "dW2", "db2")


def restated(inp, dtype):
    """the operation in plain torch on the CPU in `dtype`: y, dq, dk, dv, the parameter gradients and the forward state (results as doubles)"""
    B, C, heads, Ch = inp["B"], inp["C"], inp["heads"], inp["C"] // inp["heads"]
    qkv = inp["qkv"].detach().clone().to(dtype).requires_grad_(True)          # (clone: .to(float32) of an fp32 tensor IS that tensor -- the shared inputs stay plain data)
    params = [t.detach().clone().to(dtype).requires_grad_(True) for t in inp["crpe"] + inp["da"]]
    W1, b1, W2, b2 = params[6:]
    z = F.linear(torch.relu(F.linear(inp["lab"].to(dtype), W1, b1)), W2, b2)
    a = torch.softmax(z.view(B, heads, Ch), dim=1).reshape(B, C)
    y = _attn_ref(qkv, params[:6], a, inp["H"], inp["W"], heads, inp["splits"])
    y.backward(inp["g"].to(dtype))
    dq, dk, dv = [t.double() for t in qkv.grad.split(C, dim=2)]
    with torch.no_grad():
        k, v = qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
        kmax = k.amax(dim=1)
        ksum = torch.exp(k - kmax[:, None, :]).sum(dim=1)
        P = torch.softmax(k, dim=1).view(B, -1, heads, Ch)
        M = torch.einsum("bnhc,bnhe->bhce", P, v.reshape(B, -1, heads, Ch)).reshape(B, C, Ch)
    return dict(y=y.detach().double(), dq=dq, dk=dk, dv=dv, params=[t.grad.double() for t in params], kmax=kmax.double(), ksum=ksum.double(), M=M.double())


def run_op(inp):
    """ops.factor_att with the adapter, forward and backward, as the model calls it"""
    from mdvit_amd import ops
    d = dev()
    qkv = inp["qkv"].detach().to(d).requires_grad_(True)
    params = [t.detach().to(d).requires_grad_(True) for t in inp["crpe"] + inp["da"]]
    y = ops.factor_att(qkv, tuple(params[:6]), inp["H"], inp["W"], inp["heads"], inp["splits"], inp["lab"].to(d), tuple(params[6:]))
    y.backward(inp["g"].to(d))
    torch.cuda.synchronize()
    dq, dk, dv = qkv.grad.split(inp["C"], dim=2)
    return dict(y=y.detach(), dqkv=qkv.grad, dq=dq, dk=dk, dv=dv, params=[t.grad for t in params])


def run_forward_abi(inp):
    """mdvit_factoratt_fwd as _FactorAtt.forward calls it: the output and the state the backward is handed (kmax, ksum, Mmat)"""
    from mdvit_amd import _lib, ops
    from mdvit_amd.ops import _p, _stream, call
    d = dev()
    B, H, W, C, heads, splits = (inp[k] for k in ("B", "H", "W", "C", "heads", "splits"))
    N, Ch = H * W, C // heads
    qkv = inp["qkv"].to(d)
    crpe = [t.to(d) for t in inp["crpe"]]
    a = ops.domain_adapter(inp["lab"].to(d), *[t.to(d) for t in inp["da"]], heads)
    out, U = torch.empty(B, N, C, device=d), torch.empty(B, N, C, device=d)
    kmax, ksum, Mmat = torch.empty(B, C, device=d), torch.empty(B, C, device=d), torch.empty(B, C, Ch, device=d)
    wsb = _lib.load().mdvit_factoratt_ws_bytes(B, N, C, heads)
    ws = torch.empty(wsb // 4, device=d)
    call("mdvit_factoratt_fwd", _p(qkv), *[_p(t) for t in crpe], _p(a), _p(out), _p(U), _p(kmax), _p(ksum), _p(Mmat), _p(ws), wsb, B, H, W, C, heads, *splits, _stream())
    torch.cuda.synchronize()
    return dict(y=out, kmax=kmax, ksum=ksum, M=Mmat)


# ---- measures -----------------------------------------------------------------------------------------------------------------------------------------------
def column_errors(got, ref):
    """[B, C]: per (image, channel) column of a [B, N, C] tensor, max_n |got - ref| / max_n |ref|"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)


def row_errors(got, ref):
    """[B, C]: per (image, channel) row of Mmat [B, C, Ch]"""
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs().amax(dim=2) / ref.abs().amax(dim=2)


def element_errors(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return (got - ref).abs() / ref.abs()


def dk_in_the_kernels_form(inp, dtype):
    """dk [B, N, C] (as doubles) by the algebra the kernels use, in plain torch on the CPU in `dtype`: dk_n = P_n (x_n - t) with P = softmax over the tokens of k,
    dM[c][e] = Ch^-0.5 a[e] sum_n q[n][c] G[n][e], x_n[c] = sum_e dM[c][e] v_n[e] and t[c] = sum_e dM[c][e] M[c][e] over the head's CHANNELS from M = P^T v
    (autograd -- restated() -- forms t = sum_m P_m x_m over the TOKENS; the two agree exactly in exact arithmetic)."""
    B, C, heads = inp["B"], inp["C"], inp["heads"]
    Ch = C // heads
    with torch.no_grad():
        W1, b1, W2, b2 = [t.to(dtype) for t in inp["da"]]
        z = F.linear(torch.relu(F.linear(inp["lab"].to(dtype), W1, b1)), W2, b2)
        a = torch.softmax(z.view(B, heads, Ch), dim=1)
        q, k, v = [t.reshape(B, -1, heads, Ch) for t in inp["qkv"].to(dtype).split(C, dim=2)]
        G = inp["g"].to(dtype).reshape(B, -1, heads, Ch)
        P = torch.softmax(k, dim=1)
        M = torch.einsum("bnhc,bnhe->bhce", P, v)
        dM = Ch ** -0.5 * torch.einsum("bnhc,bnhe->bhce", q, G) * a[:, :, None, :]
        x = torch.einsum("bhce,bnhe->bnhc", dM, v)
        t = (dM * M).sum(dim=3)
        return (P * (x - t[:, None])).reshape(B, -1, C).double()


MEASURES = (("y", column_errors), ("dq", column_errors), ("dk", column_errors), ("dv", column_errors), ("ksum", element_errors), ("M", row_errors))


def assert_within(got, ref, base, names, where, limit=BASE_LIMIT, sel=None):
    """worst error of `got` against FACTOR x the worst error of the fp32 CPU evaluation `base`, both against the fp64 `ref`, per tensor; every figure is printed.
    limit: the conditioning guard on the CPU evaluations alone (None: not asserted).  sel: a channel slice -- the same statistic over those columns only."""
    bad, loose = [], []
    for name, fn in MEASURES:
        if name not in names:
            continue
        assert tuple(got[name].shape) == tuple(ref[name].shape), name
        g, r, b = (t[name] if sel is None else t[name][..., sel] for t in (got, ref, base))
        e_got, e_base = float(fn(g, r).max()), float(fn(b, r).max())
        print(f"{where} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}")
        if limit is not None and not e_base <= limit:
            loose.append((name, e_base))
        if not (math.isfinite(e_got) and e_got <= FACTOR * e_base):
            bad.append((name, e_got, e_base))
    assert not loose, f"{where}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (tensor, worst error) {loose}"
    assert not bad, f"{where}: (tensor, worst error, fp32 CPU worst error) {bad}"


# ---- one case = one shape in one regime: the references are computed once and shared by the three tests below ---------------------------------------------------
CASES = [(s, r) for s in SHAPES for r in s[6]]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: _shape_id(c[0]) + "-" + c[1])
def case(request):
    (B, H, W, C, heads, splits, _, _), regime = request.param
    inp = make_inputs(B, H, W, C, heads, splits, regime)
    return dict(where=f"({B},{H},{W},{C}) h{heads} {regime}", regime=regime, inp=inp, ref=restated(inp, torch.float64), base=restated(inp, torch.float32), op=run_op(inp),
                fwd=run_forward_abi(inp))


def test_forward_state(case):
    """kmax is the column maximum of K, bit for bit; ksum per element and Mmat per (image, channel) row against fp64; the ABI call's output is the operator's"""
    inp, ref, fwd = case["inp"], case["ref"], case["fwd"]
    C = inp["C"]
    assert torch.equal(fwd["kmax"].cpu(), inp["qkv"][:, :, C:2 * C].amax(dim=1)), "kmax is not the column maximum"
    assert torch.equal(fwd["y"], case["op"]["y"])
    assert_within(fwd, ref, case["base"], ("ksum", "M"), case["where"])


def test_output_and_data_gradients_by_the_worst_column(case):
    op, ref, base, where = case["op"], case["ref"], case["base"], case["where"]
    if case["regime"] != "spike":
        assert_within(op, ref, base, ("y", "dq", "dk", "dv"), where)
        return
    # spike: dk of the spiked (odd) columns is ill-conditioned (top of the file).  No column is left out: all columns against the fp32 evaluation of the kernels' form,
    # without the conditioning guard (it cannot hold there); the even columns against the common baseline with the guard; and the odd ones once more in absolute terms
    # (largest |error| over those columns: a column's own maximum is 1e-8 of its operands there).  The same FACTOR throughout.
    assert_within(op, ref, base, ("y", "dq", "dv"), where)
    form64, form32 = dk_in_the_kernels_form(case["inp"], torch.float64), dk_in_the_kernels_form(case["inp"], torch.float32)
    top = float(ref["dk"].abs().max())
    assert float((form64 - ref["dk"]).abs().max()) <= 1e-9 * top, "the restated form is not dk"
    assert_within(op, ref, dict(dk=form32), ("dk",), where + " all columns, baseline in the kernels' form", limit=None)
    assert_within(op, ref, base, ("dk",), where + " even columns", sel=slice(0, None, 2))
    odd = slice(1, None, 2)
    err, e_base = (float((t.detach().double().cpu() - ref["dk"]).abs()[:, :, odd].max()) for t in (op["dk"], form32))
    print(f"{where} odd columns dk, absolute: op {err:.3e} ({err / top:.2e} of the tensor maximum)  fp32-cpu in the kernels' form {e_base:.3e} ({e_base / top:.2e})  "
          f"ratio {err / e_base:.2f}  bound {FACTOR * e_base:.3e}")
    assert err <= FACTOR * e_base, f"{where}: dk in the spiked columns is off by {err:.3e}, {err / e_base:.1f} x the fp32 CPU evaluation in the kernels' form"


def test_parameter_gradients(case):
    """window weights / biases and the adapter's four (the carrier e = a dL/da reaches them): 3e-4 of the tensor maximum; the ratio to the fp32 CPU evaluation is
    printed for the record"""
    bad = []
    for name, got, ref, base in zip(PARAM_NAMES, case["op"]["params"], case["ref"]["params"], case["base"]["params"]):
        assert got is not None and tuple(got.shape) == tuple(ref.shape), name
        e_got, e_base = relerr(got, ref), relerr(base, ref)
        print(f"{case['where']} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}")
        if not (math.isfinite(e_got) and e_got <= PARAM_TOL):
            bad.append((name, e_got))
    assert not bad, f"{case['where']}: rel-to-max error above {PARAM_TOL}: {bad}"


# ---- repeatability, batch independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:2], ids=_shape_id)
def test_same_call_twice_is_bit_identical(shape):
    B, H, W, C, heads, splits, _, _ = shape
    inp = make_inputs(B, H, W, C, heads, splits, "ramp")
    a, b = run_op(inp), run_op(inp)
    for name in ("y", "dqkv"):
        assert torch.equal(a[name], b[name]), name
    for name, u, v in zip(PARAM_NAMES, a["params"], b["params"]):
        assert torch.equal(u, v), name
    fa, fb = run_forward_abi(inp), run_forward_abi(inp)
    for name in ("y", "kmax", "ksum", "M"):
        assert torch.equal(fa[name], fb[name]), name


def test_an_image_does_not_depend_on_the_batch_it_is_in():
    """(4, 35, 33, 320), ramp: the first image's y, kmax, ksum and Mmat equal a B = 1 call on that image alone, bit for bit (fa_nsub and the combine choice are
    functions of the image's token count).  dqkv: the B = 1 launch of fa_bwd_apply3_kernel takes 2 tiles per workgroup where B = 4 takes 4, so it is NOT compared bit
    for bit: the B = 1 result is held to the column bound against fp64 (the branch below compares bits should the two ever agree on the tiles per workgroup)."""
    B, H, W, C, heads, splits = 4, 35, 33, 320, 8, (2, 3, 3)
    inp4 = make_inputs(B, H, W, C, heads, splits, "ramp")
    inp1 = first_image(inp4)
    f4, f1 = run_forward_abi(inp4), run_forward_abi(inp1)
    for name in ("y", "kmax", "ksum", "M"):
        assert torch.equal(f4[name][:1], f1[name]), name
    o4, o1 = run_op(inp4), run_op(inp1)
    assert torch.equal(o4["y"][:1], o1["y"])
    if reached(1, H, W, C, heads)["tpb"] == reached(B, H, W, C, heads)["tpb"]:
        assert torch.equal(o4["dqkv"][:1], o1["dqkv"])
    else:
        ref, base = restated(inp1, torch.float64), restated(inp1, torch.float32)
        assert_within(o1, ref, base, ("dq", "dk", "dv"), "first image alone")
