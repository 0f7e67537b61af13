"""The window stencils (csrc/conv_tile.h, csrc/conv.hip) at the tile and partial-row counts a training step runs, counted exactly and measured per channel.

test_dwconv3x3 / test_gconv2 / test_factor_att_core / test_stem_conv (test_gpu_kernels.py) run shapes whose weight gradients walk ONE tile per workgroup and add at most 72
partial rows, two-row tiles with an even height only, gconv2 at C % 64 == 0 only, stride-2 / stem weight gradients at their smallest chunk size, and divide the largest
error by the largest magnitude of the whole tensor.  Here:
  * every case states the launch arithmetic it reaches (tiles per workgroup, the ragged last chunk, partial rows, which loop of the finish kernel runs, the two-row choice,
    gconv2's kernel choices, the stride-2 / stem chunk sizes) and a test re-derives it from a restatement of the host rules (`reached_*` below);
  * all-ones inputs make every weight-gradient entry an integer below 2^24 -- exact in fp32 in any summation order -- that counts the tokens each tap sees:
    dw[c][i][j] = B (H - |i - R|)(W - |j - R|), db[c] = B H W at stride 1 (checked against fp64 autograd for 3x3, 5x5, 7x7 by a test below), fp64 autograd itself at
    stride 2.  A dropped, doubled or misplaced tile, half tile or partial row changes an integer: torch.equal;
  * on seeded random inputs, against plain torch in fp64 on the CPU: y and the data gradients by the WORST (image, channel) plane, max |got - fp64| / max |fp64| over the
    plane, the weight gradients by the worst channel (over its taps): at most FACTOR x the same statistic of the same formula evaluated by torch in fp32 on the CPU, whose own
    error must stay below BASE_LIMIT (the rule and the constants of test_gpu_attention.py).  A bias gradient is a plain column sum: per element to TOL, on g + 0.5 (on a
    zero-mean g the fp32 CPU evaluation itself is off by 2.8e-3 at (64, 24, 40, 128)); one lost tile of 768 would cost 1.3e-3.  ConvRelPosEnc's db, y and dqkv keep
    test_factor_att_core's PARAM_TOL of the tensor maximum;
  * the accumulate path of mdvit_dwconv3x3_bwd at 512 partial rows: prefill + the plain result, bit for bit;
  * the two-row packed tiles (>= 4096 tokens) at an odd height on two images, and with a sentinel behind U: nothing is written past the last image.
Measured on an MI355X: 0.03 to 2.0 x the fp32 CPU evaluation's error on every tensor and shape (docs/history.md has the table, and what five injected mistakes do to
this file).  Every test prints got, baseline and ratio."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_attention import BASE_LIMIT, FACTOR, PARAM_TOL, assert_within, make_inputs, restated, run_op
from test_gpu_kernels import TOL, _attn_ref, dev, nchw, nhwc, relerr, rnd

pytestmark = pytest.mark.gpu


def _cdiv(a, b):
    return -(-a // b)


# ---- 1. the host-side launch arithmetic, restated ---------------------------------------------------------------------------------------------------------------
# conv_tile.h: CT_TH / CT_TW / CT_CL (line 16), conv_tile_wgrad_body's tile range and row index (311, 356), fa_conv_wgrad_finish_kernel's two loops (434-442),
# conv_wgrad_plan (459-464), conv3_wgrad_rows (483-490), the two-row choice of launch_conv3 (275) and launch_conv_tile (405: never for 3x3);
# conv.hip: mdvit_dwconv3x3_bwd's stride-2 chunk (1132-1134), mdvit_gconv2_3x3_fwd / _bwd's kernel choices (1148, 1163, 1172), mdvit_stemconv_wgrad (1236-1243) and the pass
# walk of stemconv_wgrad_mfma_kernel (503-515).  Change them together.
CT_TH, CT_TW, CT_CL, FIN_LANES, FIN_UNROLL = 8, 16, 32, 32, 8


def finish_loops(rows):
    """fa_conv_wgrad_finish_kernel on `rows` partial rows: row lane rl starts at b = rl, runs the unrolled loop while b + 7 * 32 < rows (b += 8 * 32) and then the tail loop
    (b += 32).  unrolled: lanes that run the unrolled loop at all; both: lanes that run it AND then a tail; tail_only: lanes that run the tail loop alone."""
    unrolled = both = tail_only = 0
    for rl in range(FIN_LANES):
        b, u = rl, 0
        while b + (FIN_UNROLL - 1) * FIN_LANES < rows:
            b, u = b + FIN_UNROLL * FIN_LANES, u + 1
        t = len(range(b, rows, FIN_LANES))
        unrolled += u > 0
        both += u > 0 and t > 0
        tail_only += u == 0 and t > 0
    return dict(unrolled=unrolled, both=both, tail_only=tail_only)


def wgrad_plan(B, H, W, cblocks):
    """conv_wgrad_plan / conv3_wgrad_rows: tiles per image, tiles per workgroup, chunks per image (gx), partial rows per 32-channel block, tiles of the last chunk"""
    tiles_w, tiles_h = _cdiv(W, CT_TW), _cdiv(H, CT_TH)
    tiles, tpb = tiles_w * tiles_h, 1
    while tpb < tiles and _cdiv(tiles, tpb * 2) * cblocks * B >= 512:
        tpb *= 2
    gx = _cdiv(tiles, tpb)
    return dict(tiles=tiles, tile_rows=tiles_h, tpb=tpb, gx=gx, rows=gx * B, last=tiles - (gx - 1) * tpb, ragged_w=int(W % CT_TW != 0), **finish_loops(gx * B))


def reached_dwconv(B, H, W, C, stride):
    if stride == 1:
        return wgrad_plan(B, H, W, _cdiv(C, CT_CL))
    ntok = B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    tpb = max(64, _cdiv(ntok, 1024))
    nblk = _cdiv(ntok, tpb)
    return dict(ntok=ntok, tokens_per_block=tpb, nblk=nblk, last=ntok - (nblk - 1) * tpb)


def reached_gconv2(B, H, W, C):
    """fwd / dgrad / wgrad: 'tile' (conv_tile.h) or 'elem' (the element-per-thread kernels); the tile weight gradient runs per concat half with GDIV = 2 into ONE workspace"""
    r = dict(fwd="tile" if C % 32 == 0 else "elem", dgrad="tile" if C % 64 == 0 else "elem", wgrad="tile" if C % 8 == 0 else "elem")
    if r["wgrad"] == "tile":
        r.update(wgrad_plan(B, H, W, _cdiv(C, CT_CL)), ncls=C)
    return r


def reached_crpe(B, H, W, C, heads, splits):
    """the three window classes inside ops.factor_att: two_row (launch_conv3's 16 x 16 packed tiles), the one-launch weight gradient's plan, its one-dimensional grid and
    what the XCD remap is left with (grid % 8), channels of each class's last 32-block (masks)"""
    Ch = C // heads
    ncls = [s * Ch for s in splits]
    cbs = [_cdiv(n, CT_CL) for n in ncls]
    r = wgrad_plan(B, H, W, sum(cbs))
    r.update(two_row=int(H * W >= 4096), cbs=tuple(cbs), masks=tuple(n - (cb - 1) * CT_CL for n, cb in zip(ncls, cbs)), grid=B * r["gx"] * sum(cbs))
    r.update(xcd_rem=r["grid"] % 8, odd_h=H % 2, ragged_w2=int(W % 16 != 0))
    return r


def reached_stem(B, H, W, Cout):
    """mdvit_stemconv_wgrad: kernel, pixels per workgroup, workgroups, pixels of the last one, trips of the cb loop; for the MFMA kernel the 16-pixel passes (wave w of a
    workgroup starts at p_beg + 16 w and advances by 64) that cross an image boundary (the ++b carry), that span more than two rows, and the index inside its workgroup of a
    pass with clamped lanes (px >= p_end)"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    per, npix = Ho * Wo, B * Ho * Wo
    if Cout % 32:
        ppb = max(64, _cdiv(npix, 2048))
        nblk = _cdiv(npix, ppb)
        return dict(kernel="scalar", ppb=ppb, nblk=nblk, last=npix - (nblk - 1) * ppb)
    ppb = max(128, _cdiv(npix, 1024))
    nblk = _cdiv(npix, ppb)
    crossing = rows3 = 0
    clamped = None
    for blk in range(nblk):
        p_beg, p_end = blk * ppb, min(npix, (blk + 1) * ppb)
        for i, p0 in enumerate(range(p_beg, p_end, 16)):
            p1 = min(p0 + 16, p_end) - 1
            crossing += p0 // per != p1 // per
            rows3 += p1 // Wo - p0 // Wo >= 2
            if p0 + 16 > p_end:
                clamped = i
    return dict(kernel="mfma", ppb=ppb, nblk=nblk, last=npix - (nblk - 1) * ppb, trips=Cout // 32, crossing=int(crossing > 0), rows3=int(rows3 > 0), clamped_pass=clamped)


# (B, H, W, C, bias, add_input, what reached_dwconv must say)
DW_S1 = [
    # ragged last chunk (1 tile of 3), ragged tile in W (40 = 2 x 16 + 8), 512 rows: every lane of the finish kernel runs the unrolled loop twice and no tail
    (256, 8, 40, 32, True, True, dict(tiles=3, tpb=2, gx=2, rows=512, last=1, ragged_w=1, unrolled=32, both=0, tail_only=0)),
    # four tiles per workgroup, last chunk of 1; 256 rows: the unrolled loop once
    (128, 8, 72, 64, False, False, dict(tiles=5, tpb=4, gx=2, rows=256, last=1, ragged_w=1, unrolled=32, both=0, tail_only=0)),
    # a step's eight tiles per workgroup, last chunk of 1, three tile rows; 128 rows: tail loop only
    (64, 24, 40, 128, True, False, dict(tiles=9, tile_rows=3, tpb=8, gx=2, rows=128, last=1, unrolled=0, tail_only=32)),
    # 240 rows: lanes 0-15 of the finish kernel unrolled, lanes 16-31 tail only
    (120, 8, 24, 64, False, False, dict(tiles=2, tpb=1, gx=2, rows=240, unrolled=16, both=0, tail_only=16)),
]
# (B, H, W, C, what reached_gconv2 must say)
GCONV2 = [
    # GDIV = 2, both halves through one workspace; 260 rows: the unrolled loop and then a tail of 4 rows (lanes 0-3)
    (130, 8, 40, 64, dict(fwd="tile", dgrad="tile", wgrad="tile", tiles=3, tpb=2, gx=2, rows=260, last=1, unrolled=32, both=4)),
    (64, 24, 40, 128, dict(fwd="tile", dgrad="tile", wgrad="tile", tiles=9, tpb=8, gx=2, rows=128, last=1)),
]
# the element-per-thread kernels: (2, 9, 7) and (1, 16, 16) x C in {8, 12, 32, 96}
_G2_PATHS = {8: dict(fwd="elem", dgrad="elem", wgrad="tile", ncls=8), 12: dict(fwd="elem", dgrad="elem", wgrad="elem"),
             32: dict(fwd="tile", dgrad="elem", wgrad="tile"), 96: dict(fwd="tile", dgrad="elem", wgrad="tile")}
GCONV2_SMALL = [(B, H, W, C, _G2_PATHS[C]) for (B, H, W) in ((2, 9, 7), (1, 16, 16)) for C in (8, 12, 32, 96)]
# ConvRelPosEnc through ops.factor_att without adapter: (B, H, W, C, heads, splits, what reached_crpe must say)
CRPE = [
    # three classes, one 32-block each with 16 / 24 / 24 live channels; 2 tiles per workgroup in 3 chunks; grid 720
    (80, 24, 32, 64, 8, (2, 3, 3), dict(two_row=0, tiles=6, tpb=2, gx=3, rows=240, last=2, cbs=(1, 1, 1), masks=(16, 24, 24), grid=720, xcd_rem=0, unrolled=16, tail_only=16)),
    # 8 tiles per workgroup, last chunk of 1; grid 540 = 4 mod 8: the XCD remap has a remainder
    (90, 24, 40, 64, 8, (2, 3, 3), dict(two_row=0, tiles=9, tpb=8, gx=2, rows=180, last=1, grid=540, xcd_rem=4, unrolled=0)),
]
# the two-row packed tiles with an odd height (the second: odd width too), a ragged last tile in W, two images
TWO_ROW = [
    (2, 65, 67, 64, 8, (2, 3, 3), dict(two_row=1, odd_h=1, ragged_w2=1)),
    (2, 67, 65, 128, 8, (2, 3, 3), dict(two_row=1, odd_h=1, ragged_w2=1)),
]
# stride 2: (B, H, W, C, what reached_dwconv must say)
DW_S2 = [(5, 230, 230, 8, dict(ntok=66125, tokens_per_block=65, nblk=1018, last=20))]
# the stem's weight gradient: (B, H, W, Cout, what reached_stem must say)
STEM = [
    # 99 pixels per image: a pass crosses an image boundary
    (3, 18, 22, 32, dict(kernel="mfma", ppb=128, crossing=1, trips=1)),
    # Ho = Wo = 3: a 16-pixel pass spans several rows and two (or three) images
    (40, 5, 5, 32, dict(kernel="mfma", ppb=128, crossing=1, rows3=1)),
    # 196605 pixels: 192 per workgroup, a last workgroup of 189 whose last pass (index 11) has clamped lanes, two trips of the cb loop
    (3, 510, 514, 64, dict(kernel="mfma", ppb=192, nblk=1024, last=189, trips=2, crossing=1, clamped_pass=11)),
    # Cout % 32 != 0: the scalar kernel
    (2, 17, 23, 48, dict(kernel="scalar", ppb=64, nblk=4, last=24)),
]

REACH = ([("dwconv", s[:4] + (1,), s[-1]) for s in DW_S1] + [("dwconv", s[:4] + (2,), s[-1]) for s in DW_S2] + [("gconv2", s[:4], s[-1]) for s in GCONV2 + GCONV2_SMALL]
         + [("crpe", s[:6], s[-1]) for s in CRPE + TWO_ROW] + [("stem", s[:4], s[-1]) for s in STEM])
_REACHED = dict(dwconv=reached_dwconv, gconv2=reached_gconv2, crpe=reached_crpe, stem=reached_stem)


def _sid(s):
    return "-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in s if not isinstance(v, dict))


@pytest.mark.parametrize("kind,shape,want", REACH, ids=[k + "-" + _sid(s) for k, s, _ in REACH])
def test_the_shape_reaches_the_code_it_is_listed_for(kind, shape, want):
    got = _REACHED[kind](*shape)
    assert {k: got.get(k) for k in want} == want, got
    if "rows" in got:
        assert got["rows"] <= 2048                     # MDVIT_MAX_PARTIAL_ROWS: the workspace ops._partials_ws hands over


def window_counts(B, H, W, win):
    """[win, win] doubles: the tokens tap (i, j) of a zero-padded stride-1 window sees on all-ones inputs, B (H - |i - R|)(W - |j - R|)"""
    d = (torch.arange(win) - win // 2).abs().double()
    return B * (H - d)[:, None] * (W - d)[None, :]


@pytest.mark.parametrize("win", [3, 5, 7])
def test_the_count_formula_is_fp64_autograd_on_ones(win):
    B, H, W, C = 2, 9, 11, 3
    w = torch.zeros(C, 1, win, win, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.ones(B, C, H, W, dtype=torch.float64), w, b, 1, win // 2, 1, C).sum().backward()
    assert torch.equal(w.grad, window_counts(B, H, W, win).expand(C, 1, win, win)) and torch.equal(b.grad, torch.full((C,), float(B * H * W), dtype=torch.float64))


# ---- measures ---------------------------------------------------------------------------------------------------------------------------------------------------
def plane_errors(got, ref, keep):
    """max |got - ref| / max |ref| over all but the first `keep` dimensions (keep = 2 on NCHW: per (image, channel) plane; keep = 1 on a weight gradient: per channel)"""
    got, ref = got.detach().double().cpu(), ref.double()
    dims = tuple(range(keep, ref.dim()))
    return (got - ref).abs().amax(dim=dims) / ref.abs().amax(dim=dims)


def held(where, got, ref, base, spec):
    """spec: (name, keep) -- the worst plane_errors of got[name] against FACTOR x that of the fp32 CPU evaluation base[name], which must itself stay below BASE_LIMIT;
    (name, None) -- per element to TOL (a bias gradient).  Every figure is printed; all tensors are measured before anything is asserted."""
    bad, loose = [], []
    for name, keep in spec:
        assert tuple(got[name].shape) == tuple(ref[name].shape), name
        if keep is None:
            e_got, e_base = (float(((t[name].detach().double().cpu() - ref[name]).abs() / ref[name].abs()).max()) for t in (got, base))
            print(f"{where} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {TOL:.1e} (per element)")
            if not (math.isfinite(e_got) and e_got <= TOL):
                bad.append((name, e_got, e_base))
            continue
        e_got, e_base = float(plane_errors(got[name], ref[name], keep).max()), float(plane_errors(base[name], ref[name], keep).max())
        print(f"{where} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}")
        if not e_base <= BASE_LIMIT:
            loose.append((name, e_base))
        if not (math.isfinite(e_got) and e_got <= FACTOR * e_base):
            bad.append((name, e_got, e_base))
    assert not loose, f"{where}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (tensor, worst error) {loose}"
    assert not bad, f"{where}: (tensor, worst error, fp32 CPU worst error) {bad}"


def _leaf(t, dtype):
    return None if t is None else t.detach().clone().to(dtype).requires_grad_(True)


def _on_gpu(t, grad=True):
    return None if t is None else t.detach().to(dev()).requires_grad_(grad)


# ---- depthwise 3x3 --------------------------------------------------------------------------------------------------------------------------------------------
def dwconv_inputs(B, H, W, C, stride, bias, ones=False):
    """NCHW fp32 CPU tensors, seeded as test_dwconv3x3's; with a bias g is shifted by 0.5 (a column sum of a zero-mean g is ill-conditioned per element)"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w, b = rnd(C, 1, 3, 3, seed=41, scale=0.3), (rnd(C, seed=42, scale=0.1) if bias else None)
    if ones:
        return dict(x=torch.ones(B, C, H, W), w=w, b=b, g=torch.ones(B, C, Ho, Wo))
    return dict(x=rnd(B, C, H, W, seed=40), w=w, b=b, g=rnd(B, C, Ho, Wo, seed=43) + (0.5 if bias else 0.0))


def dwconv_cpu(inp, stride, add, dtype):
    x, w, b = _leaf(inp["x"], dtype), _leaf(inp["w"], dtype), _leaf(inp["b"], dtype)
    y = F.conv2d(x, w, b, stride, 1, 1, x.shape[1])
    y = y + x if add else y
    y.backward(inp["g"].to(dtype))
    r = dict(y=y.detach().double(), dx=x.grad.double(), dw=w.grad.double())
    if b is not None:
        r["db"] = b.grad.double()
    return r


def dwconv_gpu(inp, stride, add, data_grad=True):
    from mdvit_amd import ops
    x, w, b = _on_gpu(nhwc(inp["x"]), data_grad), _on_gpu(inp["w"]), _on_gpu(inp["b"])
    y = ops.dwconv3x3(x, w, b, stride, add)
    y.backward(nhwc(inp["g"]).to(dev()))
    torch.cuda.synchronize()
    r = dict(y=nchw(y.detach()), dw=w.grad)
    if data_grad:
        r["dx"] = nchw(x.grad)
    if b is not None:
        r["db"] = b.grad
    return r


@pytest.mark.parametrize("B,H,W,C,bias,add,_", DW_S1, ids=[_sid(s) for s in DW_S1])
def test_dwconv_counts_every_tile_and_partial_row_once(B, H, W, C, bias, add, _):
    got = dwconv_gpu(dwconv_inputs(B, H, W, C, 1, bias, ones=True), 1, add, data_grad=False)
    assert torch.equal(got["dw"].double().cpu(), window_counts(B, H, W, 3).expand(C, 1, 3, 3))
    if bias:
        assert torch.equal(got["db"].double().cpu(), torch.full((C,), float(B * H * W), dtype=torch.float64))


@pytest.mark.parametrize("B,H,W,C,bias,add,_", DW_S1, ids=[_sid(s) for s in DW_S1])
def test_dwconv_values_by_the_worst_plane_and_channel(B, H, W, C, bias, add, _):
    inp = dwconv_inputs(B, H, W, C, 1, bias)
    ref, base, got = dwconv_cpu(inp, 1, add, torch.float64), dwconv_cpu(inp, 1, add, torch.float32), dwconv_gpu(inp, 1, add)
    held(f"dwconv3x3 ({B},{H},{W},{C})", got, ref, base, [("y", 2), ("dx", 2), ("dw", 1)] + ([("db", None)] if bias else []))


def test_dwconv_accumulate_is_the_prefill_plus_the_plain_result_bit_for_bit():
    """mdvit_dwconv3x3_bwd as _DwConv3x3.backward calls it on the side stream (dx = NULL, the workspace of ops._partials_ws, accumulate = 1) at 512 partial rows: the finish
    kernel's `*dst + t` is one fp32 add of the same t the plain call stores"""
    from mdvit_amd.ops import _p, _partials_ws, _stream, call
    B, H, W, C = DW_S1[0][:4]
    inp = dwconv_inputs(B, H, W, C, 1, True)
    x, g, w = nhwc(inp["x"]).to(dev()), nhwc(inp["g"]).to(dev()), inp["w"].to(dev())
    pre_w, pre_b = rnd(C, 1, 3, 3, seed=44, scale=50.0), rnd(C, seed=45, scale=500.0)
    out = []
    for accumulate in (0, 1):
        dw, db = (pre_w.to(dev()), pre_b.to(dev())) if accumulate else (torch.empty(C, 1, 3, 3, device=dev()), torch.empty(C, device=dev()))
        wsp, wsb, _keep = _partials_ws(10 * C, dev())
        call("mdvit_dwconv3x3_bwd", _p(g), _p(x), _p(w), None, _p(dw), _p(db), wsp, wsb, B, H, W, C, 1, 1, accumulate, _stream())
        torch.cuda.synchronize()
        out.append((dw.cpu(), db.cpu()))
    (dw0, db0), (dw1, db1) = out
    assert float(dw0.abs().max()) > 0 and float(db0.abs().max()) > 0
    assert torch.equal(dw1, pre_w + dw0) and torch.equal(db1, pre_b + db0)


@pytest.mark.parametrize("B,H,W,C,_", DW_S2, ids=[_sid(s) for s in DW_S2])
def test_dwconv_stride2_counts_every_token_chunk_once(B, H, W, C, _):
    """stride 2, pad 1: the counts are no longer the stride-1 formula -- fp64 autograd on the same ones, rounded to integers"""
    inp = dwconv_inputs(B, H, W, C, 2, True, ones=True)
    ref, got = dwconv_cpu(inp, 2, False, torch.float64), dwconv_gpu(inp, 2, False, data_grad=False)
    assert float(ref["dw"].max()) < 2 ** 24 and float(ref["dw"].min()) >= 1
    assert torch.equal(got["dw"].double().cpu(), ref["dw"].round()) and torch.equal(got["db"].double().cpu(), ref["db"].round())


@pytest.mark.parametrize("B,H,W,C,_", DW_S2, ids=[_sid(s) for s in DW_S2])
def test_dwconv_stride2_values_by_the_worst_plane_and_channel(B, H, W, C, _):
    inp = dwconv_inputs(B, H, W, C, 2, False)
    ref, base, got = dwconv_cpu(inp, 2, False, torch.float64), dwconv_cpu(inp, 2, False, torch.float32), dwconv_gpu(inp, 2, False)
    held(f"dwconv3x3 stride 2 ({B},{H},{W},{C})", got, ref, base, [("y", 2), ("dx", 2), ("dw", 1)])


# ---- the decoder's grouped convolution on (skip, up) --------------------------------------------------------------------------------------------------------------
def gconv2_inputs(B, H, W, C, ones=False):
    if ones:
        return dict(skip=torch.ones(B, C, H, W), up=torch.ones(B, C, H, W), w=rnd(C, 2, 3, 3, seed=52, scale=0.3), g=torch.ones(B, C, H, W))
    return dict(skip=rnd(B, C, H, W, seed=50), up=rnd(B, C, H, W, seed=51), w=rnd(C, 2, 3, 3, seed=52, scale=0.3), g=rnd(B, C, H, W, seed=53))


def gconv2_cpu(inp, dtype):
    s, u, w = _leaf(inp["skip"], dtype), _leaf(inp["up"], dtype), _leaf(inp["w"], dtype)
    y = F.conv2d(torch.cat((s, u), 1), w, None, 1, 1, 1, w.shape[0])
    y.backward(inp["g"].to(dtype))
    return dict(y=y.detach().double(), dskip=s.grad.double(), dup=u.grad.double(), dw=w.grad.double())


def gconv2_gpu(inp):
    from mdvit_amd import ops
    s, u, w = _on_gpu(nhwc(inp["skip"])), _on_gpu(nhwc(inp["up"])), _on_gpu(inp["w"])
    y = ops.gconv2_3x3(s, u, w)
    y.backward(nhwc(inp["g"]).to(dev()))
    torch.cuda.synchronize()
    return dict(y=nchw(y.detach()), dskip=nchw(s.grad), dup=nchw(u.grad), dw=w.grad)


@pytest.mark.parametrize("B,H,W,C,_", GCONV2, ids=[_sid(s) for s in GCONV2])
def test_gconv2_counts_every_tile_and_partial_row_once(B, H, W, C, _):
    got = gconv2_gpu(gconv2_inputs(B, H, W, C, ones=True))
    assert torch.equal(got["dw"].double().cpu(), window_counts(B, H, W, 3).expand(C, 2, 3, 3))


@pytest.mark.parametrize("B,H,W,C,_", GCONV2 + GCONV2_SMALL, ids=[_sid(s) for s in GCONV2 + GCONV2_SMALL])
def test_gconv2_values_by_the_worst_plane_and_channel(B, H, W, C, _):
    inp = gconv2_inputs(B, H, W, C)
    ref, base, got = gconv2_cpu(inp, torch.float64), gconv2_cpu(inp, torch.float32), gconv2_gpu(inp)
    held(f"gconv2 ({B},{H},{W},{C})", got, ref, base, [("y", 2), ("dskip", 2), ("dup", 2), ("dw", 1)])


# ---- ConvRelPosEnc inside the attention core ------------------------------------------------------------------------------------------------------------------------
CRPE_NAMES = ("dw3", "db3", "dw5", "db5", "dw7", "db7")


def crpe_inputs(B, H, W, C, heads, splits, ones=False):
    """make_inputs' qkv, window parameters and g (flat regime); ones: q = v = 1, k = 0, g = 1 -- without adapter dU = g q = 1 exactly, and the windows read v = 1"""
    inp = make_inputs(B, H, W, C, heads, splits, "flat")
    if ones:
        one = torch.ones(B, H * W, C)
        inp.update(qkv=torch.cat((one, torch.zeros_like(one), one), 2), g=one.clone())
    return inp


def crpe_cpu(inp, dtype):
    qkv, params = _leaf(inp["qkv"], dtype), [_leaf(t, dtype) for t in inp["crpe"]]
    y = _attn_ref(qkv, params, None, inp["H"], inp["W"], inp["heads"], inp["splits"])
    y.backward(inp["g"].to(dtype))
    return dict(y=y.detach().double(), dqkv=qkv.grad.double(), **{n: t.grad.double() for n, t in zip(CRPE_NAMES, params)})


def crpe_gpu(inp):
    from mdvit_amd import ops
    qkv, params = _on_gpu(inp["qkv"]), [_on_gpu(t) for t in inp["crpe"]]
    y = ops.factor_att(qkv, tuple(params), inp["H"], inp["W"], inp["heads"], inp["splits"])
    y.backward(inp["g"].to(dev()))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dqkv=qkv.grad, **{n: t.grad for n, t in zip(CRPE_NAMES, params)})


@pytest.mark.parametrize("B,H,W,C,heads,splits,_", CRPE, ids=[_sid(s) for s in CRPE])
def test_crpe_counts_every_tile_and_partial_row_once(B, H, W, C, heads, splits, _):
    got = crpe_gpu(crpe_inputs(B, H, W, C, heads, splits, ones=True))
    for win, s in zip((3, 5, 7), splits):
        n = s * (C // heads)
        assert torch.equal(got[f"dw{win}"].double().cpu(), window_counts(B, H, W, win).expand(n, 1, win, win)), f"dw{win}"
        assert torch.equal(got[f"db{win}"].double().cpu(), torch.full((n,), float(B * H * W), dtype=torch.float64)), f"db{win}"


@pytest.mark.parametrize("B,H,W,C,heads,splits,_", CRPE, ids=[_sid(s) for s in CRPE])
def test_crpe_values(B, H, W, C, heads, splits, _):
    """dw3 / dw5 / dw7 by the worst channel under the common rule; db, y and dqkv to PARAM_TOL of the tensor maximum, test_factor_att_core's bar (the counts above carry
    the bookkeeping of db)"""
    inp = crpe_inputs(B, H, W, C, heads, splits)
    ref, base, got = crpe_cpu(inp, torch.float64), crpe_cpu(inp, torch.float32), crpe_gpu(inp)
    where, bad = f"crpe ({B},{H},{W},{C})", []
    for name in ("y", "dqkv", "db3", "db5", "db7"):
        assert tuple(got[name].shape) == tuple(ref[name].shape), name
        e_got, e_base = relerr(got[name], ref[name]), relerr(base[name], ref[name])
        print(f"{where} {name}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {PARAM_TOL:.1e} (of the tensor maximum)")
        if not (math.isfinite(e_got) and e_got <= PARAM_TOL):
            bad.append((name, e_got))
    held(where, got, ref, base, [("dw3", 1), ("dw5", 1), ("dw7", 1)])
    assert not bad, f"{where}: rel-to-max error above {PARAM_TOL}: {bad}"


@pytest.mark.parametrize("B,H,W,C,heads,splits,_", TWO_ROW, ids=[_sid(s) for s in TWO_ROW])
def test_two_row_tiles_with_an_odd_height(B, H, W, C, heads, splits, _):
    """>= 4096 tokens, odd H: the last row pair of conv_tile2_body has h < H and h + 1 == H; a second row written anyway lands in row 0 of the next image (two images: it
    is seen) -- forward (U -> y) and the flipped-tap pass of the backward (dVc -> dv).  With the adapter, as the model calls it."""
    inp = make_inputs(B, H, W, C, heads, splits, "flat")
    ref, base, got = restated(inp, torch.float64), restated(inp, torch.float32), run_op(inp)
    where, bad = f"two-row ({B},{H},{W},{C})", []
    assert_within(got, ref, base, ("y", "dq", "dk", "dv"), where)
    for name, g_, r_ in zip(CRPE_NAMES + ("dW1", "db1", "dW2", "db2"), got["params"], ref["params"]):
        e_got = relerr(g_, r_)
        print(f"{where} {name}: op {e_got:.3e}  bound {PARAM_TOL:.1e} (of the tensor maximum)")
        if not (math.isfinite(e_got) and e_got <= PARAM_TOL):
            bad.append((name, e_got))
    assert not bad, f"{where}: rel-to-max error above {PARAM_TOL}: {bad}"


@pytest.mark.parametrize("B,H,W,C,heads,splits,_", TWO_ROW, ids=[_sid(s) for s in TWO_ROW])
def test_two_row_tiles_write_nothing_past_the_last_image(B, H, W, C, heads, splits, _):
    """In the test above a second row written at h + 1 == H races with the next image's own row 0 and may lose; on the LAST image it leaves the tensor.  So
    mdvit_factoratt_fwd is called through the C ABI with U (the windows' output, conv(v) + bias) as the head of a buffer that goes on for two more image rows holding a
    sentinel: they must come back untouched, U is the fp64 convolution, and `out` is the operator's bit for bit."""
    from mdvit_amd import _lib
    from mdvit_amd.ops import _p, _stream, call
    inp = crpe_inputs(B, H, W, C, heads, splits)
    N, Ch, d = H * W, C // heads, dev()
    qkv, crpe = inp["qkv"].to(d), [t.to(d) for t in inp["crpe"]]
    guard = 2 * W * C
    buf = torch.full((B * N * C + guard,), 12345.0, device=d)
    out = torch.empty(B, N, C, device=d)
    kmax, ksum, Mmat = torch.empty(B, C, device=d), torch.empty(B, C, device=d), torch.empty(B, C, Ch, device=d)
    wsb = _lib.load().mdvit_factoratt_ws_bytes(B, N, C, heads)
    ws = torch.empty(wsb // 4, device=d)
    call("mdvit_factoratt_fwd", _p(qkv), *[_p(t) for t in crpe], None, _p(out), _p(buf), _p(kmax), _p(ksum), _p(Mmat), _p(ws), wsb, B, H, W, C, heads, *splits, _stream())
    torch.cuda.synchronize()
    assert torch.equal(buf[B * N * C:].cpu(), torch.full((guard,), 12345.0)), "the windows wrote past the last image"
    v = inp["qkv"][:, :, 2 * C:].double().permute(0, 2, 1).reshape(B, C, H, W)
    w3, b3, w5, b5, w7, b7 = [t.double() for t in inp["crpe"]]
    c1, c2 = splits[0] * Ch, (splits[0] + splits[1]) * Ch
    conv = torch.cat([F.conv2d(v[:, :c1], w3, b3, 1, 1, 1, c1), F.conv2d(v[:, c1:c2], w5, b5, 1, 2, 1, c2 - c1), F.conv2d(v[:, c2:], w7, b7, 1, 3, 1, C - c2)], 1)
    e = float(plane_errors(buf[:B * N * C].view(B, N, C).permute(0, 2, 1), conv.reshape(B, C, N), 2).max())
    print(f"two-row ({B},{H},{W},{C}) U, worst (image, channel) plane: {e:.3e}  bound {TOL:.1e}")
    assert e <= TOL
    assert torch.equal(out, crpe_gpu(inp)["y"])


# ---- the stem's weight gradient -------------------------------------------------------------------------------------------------------------------------------
# Offsets of the random cases (settled on the CPU evaluations alone): dw[co][ci][tap] sums B Ho Wo products.  On test_stem_conv's zero-mean image and gradient the fp32 CPU
# evaluation's worst channel is off by 3e-7 to 5.0e-6 (196605 pixels) -- under BASE_LIMIT already, but a random walk's end point; image + 1 and g + 0.5 give every product
# the mean 0.5, the sum grows with the pixel count and the same statistic is 2e-7 to 2.8e-6.
STEM_IMG_OFFSET, STEM_G_OFFSET = 1.0, 0.5


def stem_inputs(B, H, W, Cout, ones=False):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = rnd(Cout, 3, 3, 3, seed=71, scale=0.2)
    if ones:
        return dict(img=torch.ones(B, 3, H, W), w=w, g=torch.ones(B, Cout, Ho, Wo))
    return dict(img=rnd(B, 3, H, W, seed=70, scale=2.0) + STEM_IMG_OFFSET, w=w, g=rnd(B, Cout, Ho, Wo, seed=72) + STEM_G_OFFSET)


def stem_cpu(inp, dtype):
    w = _leaf(inp["w"], dtype)
    y = F.conv2d(inp["img"].to(dtype), w, None, 2, 1)
    y.backward(inp["g"].to(dtype))
    return dict(y=y.detach().double(), dw=w.grad.double())


def stem_gpu(inp):
    from mdvit_amd import ops
    w = _on_gpu(inp["w"])
    y = ops.stem_conv(inp["img"].to(dev()), w)
    y.backward(nhwc(inp["g"]).to(dev()))
    torch.cuda.synchronize()
    return dict(y=nchw(y.detach()), dw=w.grad)


@pytest.mark.parametrize("B,H,W,Cout,_", STEM, ids=[_sid(s) for s in STEM])
def test_stem_counts_every_pixel_once(B, H, W, Cout, _):
    """all-ones image and gradient: dw[co][ci][tap] is the number of output pixels whose tap lies inside the image -- fp64 autograd on the same ones, rounded to integers"""
    inp = stem_inputs(B, H, W, Cout, ones=True)
    ref, got = stem_cpu(inp, torch.float64), stem_gpu(inp)
    assert float(ref["dw"].max()) < 2 ** 24 and float(ref["dw"].min()) >= 1
    assert torch.equal(got["dw"].double().cpu(), ref["dw"].round())


@pytest.mark.parametrize("B,H,W,Cout,_", STEM, ids=[_sid(s) for s in STEM])
def test_stem_values_by_the_worst_plane_and_channel(B, H, W, Cout, _):
    inp = stem_inputs(B, H, W, Cout)
    ref, base, got = stem_cpu(inp, torch.float64), stem_cpu(inp, torch.float32), stem_gpu(inp)
    held(f"stem ({B},{H},{W},{Cout})", got, ref, base, [("y", 2), ("dw", 1)])
