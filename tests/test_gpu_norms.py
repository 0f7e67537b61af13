"""LayerNorm, BatchNorm(+activation, +Dropout2d), rowdot and the column sums (csrc/norm.hip, the second stages of csrc/abi.hip) at the row and partial-row counts a training
step runs, counted exactly and measured per row and per channel.

test_layernorm / test_bn_act_train / test_rowdot (test_gpu_kernels.py) run at most 4099 rows, 8 BatchNorm partial rows and 65 LayerNorm partial rows, every C = 320 / 512
backward on the 16-rows-per-workgroup side, and divide the largest error by the largest magnitude of the whole tensor.  A step runs 4096 to 1 M rows.  Here:
  * every case states the launch arithmetic it reaches (passes of the grid-stride row loops and the rows of the last one, mdvit_ln_bwd's rows per workgroup, partial rows, the
    second-stage kernel and which of its lanes run the unrolled loop, chan_grid's round-up to a multiple of g, the trips of the four-rows-in-flight loops) and a test
    re-derives it from a restatement of the host rules (`reached_*` below), which is itself held against the library where the library gives the rule back (the workspace
    sizes of mdvit_bn_ws_bytes / mdvit_bn_rowdot_ws_bytes, and a workspace of exactly the restated size / 4 bytes short at every partial-row entry);
  * small-integer inputs make every column sum an integer below 2^24 -- exact in fp32 in any order: dbeta, dgamma (on +-1 rows, where x-hat is +-0.5), the column sums with
    an exact 0 / 2 row scale, the BatchNorm sums (mean bit for bit, rstd to 1 ulp, the running statistics to the rounding of their fp32 update, nbt), rowdot's db.  A dropped,
    doubled or misplaced row, partial row or group changes an integer: torch.equal;
  * on seeded continuous inputs, against plain torch in fp64 on the CPU: y, z, dx, dy by the WORST row and the WORST (group, channel) column, max |got - fp64| / max |fp64|
    inside the row or column; dgamma, dbeta, dw and the column sums per element (on g + 0.5, x with a per-column offset: a zero-mean column sum is ill-conditioned per
    element, docs/history.md); a 1-output product (rowdot's y, bn_rowdot's low) is one column.  Bound: FACTOR x the same statistic of the same formula evaluated by torch in
    fp32 on the CPU, which must itself stay below BASE_LIMIT (the rule and the constants of test_gpu_attention.py);
  * BatchNorm in two layers, since torch's CPU batch norm accumulates in double and says nothing about a fp32 E[x^2] - E[x]^2: (a) mdvit_bn_stats alone, rstd and the variance
    recovered from it to FACTOR 2^-24 (1 + mean^2 / var) per channel, mean to FACTOR 2^-24 max(|mean|, std), at the existing tests' inputs and at a per-channel mean of 4
    standard deviations (32: printed, not asserted); (b) the apply / backward kernels with the fp64 statistics rounded to fp32 given to kernel and reference alike, relu and
    hswish, training and eval, Dropout2d under the mask read back from the forward; and one end-to-end case per C through ops.bn_act.  Inputs are moved off the activations'
    kinks (a pre-activation within 1e-3 of one is pushed to 2e-3: there fp32 and fp64 may disagree on the branch, and the error is the whole gradient);
  * every case runs twice: bit-equal (no atomics in this family); NaN-filled outputs and workspaces come back finite, a sentinel row behind y / dx / z comes back untouched.
Measured on an MI355X: 0.02 to 2.0 x the fp32 CPU evaluation's error on every tensor, unit and shape, the statistics within 1.5 roundings x their conditioning; no defect
found (docs/history.md has the tables, the 32-sigma figures, the unreachable branch and what eleven injected mistakes do to this file).  Every test prints got, baseline and
ratio.  `python tests/test_gpu_norms.py` runs the launch arithmetic and the conditioning guards without a GPU."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_attention import BASE_LIMIT, FACTOR
from test_gpu_kernels import TOL, dev, relerr, rnd

pytestmark = pytest.mark.gpu

KEY = (0x1234abcd, 0x9e3779b9)
E_WORKSPACE = 4        # include/mdvit_hip.h
EPS_BN = 1e-5
SLACK_ROWS = 32        # NaN rows the tests own behind an exactly sized partial-row workspace: a second stage that reads a group of rows too many returns NaN, not stale memory
ULP = 2.0 ** -24       # half the spacing of fp32 numbers relative to their magnitude: one rounding


def _cdiv(a, b):
    return -(-a // b)


def _sid(s):
    return "-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in s if not isinstance(v, dict))


# ---- 1. the host-side launch arithmetic, restated ---------------------------------------------------------------------------------------------------------------
# norm.hip: chan_grid (752-766), CHAN_MAX_BLOCKS (876), the four-in-flight loops of chan_reduce_kernel (330-347) and bn_rowdot_reduce_kernel (685-693), chan_finalize_kernel's
# loops (395-401), bn_stats_finalize_kernel's (434-440), mdvit_layernorm_fwd's two grids (793, 801), mdvit_ln_bwd's rows_wg / nblk (855-856, 864), bn_ws_bytes (879-881),
# mdvit_bn_rowdot_ws_bytes (953), the grids of mdvit_bn_apply (923), mdvit_bn_bwd (943-946), mdvit_bn_rowdot_fwd (965), mdvit_bn_rowdot_bwd (989-993), colsum_impl (1021),
# mdvit_rowdot_fwd (1037), mdvit_rowdot_bwd (1046); common.h: mdvit_fast_ln (67); abi.hip: launch_reduce (191-202), the loops of reduce_partials_kernel<LPQ> (93-116) and of
# reduce_partials_wide_kernel (159-173).  Change them together.  (MDVIT_LN_BWD_ROWS and MDVIT_REDUCE_WIDE, the A/B switches of mdvit_ln_bwd and launch_reduce, must be unset.)
CHAN_MAX_BLOCKS, FAST_LN = 512, (64, 128, 320, 512)


def lane_loops(rows, lanes, unroll=4):
    """A second stage's row walk on `rows` partial rows: row lane rl starts at b = rl, runs the unrolled loop while b + (unroll - 1) * lanes < rows (b += unroll * lanes) and
    then the tail loop (b += lanes).  unrolled: lanes that run the unrolled loop at all; both: lanes that run it AND then a tail; tail_only: lanes that run the tail loop
    alone; trips: (unrolled trips, tail trips) of lane 0."""
    unrolled = both = tail_only = 0
    trips = None
    for rl in range(lanes):
        b, u = rl, 0
        while b + (unroll - 1) * lanes < rows:
            b, u = b + unroll * lanes, u + 1
        t = len(range(b, rows, lanes))
        trips = trips or (u, t)
        unrolled += u > 0
        both += u > 0 and t > 0
        tail_only += u == 0 and t > 0
    return dict(unrolled=unrolled, both=both, tail_only=tail_only, trips=trips)


def chan_grid(M, C, max_blocks):
    QC = C // 4
    g = QC // math.gcd(QC, 256)
    want = max(1, min(_cdiv(M * QC, 256 * 8), max_blocks))
    return _cdiv(want, g) * g


def reached_chan(M, C, max_blocks=CHAN_MAX_BLOCKS):
    """chan_reduce_kernel<0/1/2> / bn_rowdot_reduce_kernel on M rows (of one group): g, the grid asked for (want), the grid, rstep = grid * 256 / (C / 4), and the (four-in-
    flight trips, tail trips) of the threads that start at row 0 (first) and at row rstep - 1 (last); ragged: the two differ"""
    QC = C // 4
    grid = chan_grid(M, C, max_blocks)
    assert (grid * 256) % QC == 0
    rstep = grid * 256 // QC

    def trips(r):
        u = 0
        while r + 3 * rstep < M:
            r, u = r + 4 * rstep, u + 1
        return u, len(range(r, M, rstep))
    first, last = trips(0), trips(rstep - 1)
    return dict(g=QC // math.gcd(QC, 256), want=_cdiv(M * QC, 2048), grid=grid, rstep=rstep, first=first, last=last, ragged=int(first != last))


def reached_reduce(nblk, stride, n):
    """launch_reduce's four-way choice and the loops of the kernel it picks"""
    vec = stride % 4 == 0 and (nblk * stride) % 4 == 0          # (and a 16-byte aligned workspace, which every caller here has)
    if vec and nblk >= 64 and n % 4 == 0:
        return dict(reduce="wide", **lane_loops(nblk, 32))
    lpq = 256 if nblk >= 256 else (32 if nblk >= 16 else 4)
    if vec:                                                     # every quad is whole (n % 4 == 0 whenever vec: stride == n at every caller)
        return dict(reduce=str(lpq), vector=1, **lane_loops(nblk, lpq))
    return dict(reduce=str(lpq), vector=0, unrolled=0, both=0, tail_only=min(lpq, nblk), trips=(0, _cdiv(nblk, lpq)))


def _passes(rows, per_pass):
    p = _cdiv(rows, per_pass)
    return p, rows - (p - 1) * per_pass


def reached_ln(M, C, groups):
    """mdvit_layernorm_fwd and mdvit_ln_bwd on `groups` groups of M / groups rows: the forward's grid.x, passes of its row loop and rows of the last pass; the backward's rows
    per workgroup, partial rows per group (nblk), passes and rows of the last; the second stage (mdvit_reduce_partials_batched2: `groups` batches of nblk rows x 2 C)"""
    Mg = M // groups
    if C in FAST_LN:
        fgrid = min(_cdiv(Mg, 16), max(1, 4096 // groups))
        rows_wg = 16 if (C >= 320 and M * C <= 16384 * 512) else 64
        nblk = min(_cdiv(Mg, rows_wg), 1024 // groups)
        fper, bper = 16 * fgrid, 16 * nblk                      # 16 lanes per row: 16 rows per workgroup and pass
    else:
        fgrid = min(_cdiv(Mg, 4), max(1, 4096 // groups))
        rows_wg, nblk = 16, min(_cdiv(Mg, 16), 1024 // groups)
        fper, bper = 4 * fgrid, 4 * nblk                        # a wave per row: 4 rows per workgroup and pass
    (fp, fl), (bp, bl) = _passes(Mg, fper), _passes(Mg, bper)
    r = reached_reduce(nblk, 2 * C, 2 * C)
    return dict(kernel="16" if C in FAST_LN else "generic", fwd_grid=fgrid, fwd_passes=fp, fwd_last=fl, rows_wg=rows_wg, nblk=nblk, bwd_passes=bp, bwd_last=bl, batches=groups, **r)


def reached_bn(M, C, groups):
    """mdvit_bn_stats / mdvit_bn_bwd on `groups` groups of M / groups rows: chan_reduce_kernel<0/1> per group, the loops of bn_stats_finalize_kernel (fin_stats) and of
    chan_finalize_kernel (fin_chan) on its partial rows, the grid of the apply kernels"""
    Mg = M // groups
    r = reached_chan(Mg, C)
    return dict(r, fin_stats=lane_loops(r["grid"], 32), fin_chan=lane_loops(r["grid"], 8), apply_grid=chan_grid(Mg, C, max(1, 4096 // groups)))


def reached_bn_rowdot(M, C):
    """mdvit_bn_rowdot_fwd (a wave per row) and mdvit_bn_rowdot_bwd (bn_rowdot_reduce_kernel, chan_finalize_kernel on C2 = 3 C + 4 columns)"""
    grid = min(_cdiv(M, 4), 8192)
    p, last = _passes(M, 4 * grid)
    r = reached_chan(M, C)
    return dict(r, fwd_grid=grid, fwd_passes=p, fwd_last=last, C2=3 * C + 4, fin_chan=lane_loops(r["grid"], 8))


def reached_colsum(M, N, out=True):
    r = reached_chan(M, N, 1024 if out else 4096)
    return dict(r, **reached_reduce(r["grid"], N, N)) if out else r


def reached_rowdot(M, K):
    """mdvit_rowdot_fwd and mdvit_rowdot_bwd (partial rows [dw (K) | db]: stride K + 1)"""
    fgrid, nblk = min(_cdiv(M, 4), 8192), min(_cdiv(M, 4), 1024)
    (fp, fl), (bp, bl) = _passes(M, 4 * fgrid), _passes(M, 4 * nblk)
    return dict(fwd_grid=fgrid, fwd_passes=fp, fwd_last=fl, nblk=nblk, bwd_passes=bp, bwd_last=bl, **reached_reduce(nblk, K + 1, K + 1))


# (rows, C, groups, what reached_ln must say)
LN = [
    # forward: 4096 workgroups and a second pass of 21 rows; backward: 1024 workgroups x 64 rows in 5 passes, 1024 partial rows: every lane of the wide kernel unrolled 8 times
    (65557, 64, 1, dict(kernel="16", fwd_grid=4096, fwd_passes=2, fwd_last=21, rows_wg=64, nblk=1024, bwd_passes=5, bwd_last=21, reduce="wide", unrolled=32, both=0, tail_only=0,
                        trips=(8, 0))),
    # groups 4: grid.x 1024 / 256 per group, a second pass of 5 rows, the batched second stage at 256 rows x 4 batches
    (4 * 16389, 128, 4, dict(fwd_grid=1024, fwd_passes=2, fwd_last=5, rows_wg=64, nblk=256, bwd_passes=5, bwd_last=5, batches=4, reduce="wide", unrolled=32, both=0, trips=(2, 0))),
    # 240 partial rows: lanes 0-15 of the wide kernel unrolled twice, lanes 16-31 unrolled once and then the tail
    (15340, 64, 1, dict(rows_wg=64, nblk=240, bwd_passes=4, bwd_last=3820, reduce="wide", unrolled=32, both=16, tail_only=0)),
    # the two sides of the rows_wg switch at C = 320 ...
    (26214, 320, 1, dict(rows_wg=16, nblk=1024, bwd_passes=2, bwd_last=9830, reduce="wide")),
    (26215, 320, 1, dict(rows_wg=64, nblk=410, bwd_passes=4, bwd_last=6535, reduce="wide", unrolled=32, both=26, trips=(3, 1))),
    # ... and at C = 512 (the equality case is the 16-row side)
    (16384, 512, 1, dict(rows_wg=16, nblk=1024, bwd_passes=1, bwd_last=16384)),
    (16385, 512, 1, dict(rows_wg=64, nblk=257, bwd_passes=4, bwd_last=4049, reduce="wide")),
    # the generic kernels (SwinUnet's widths): VPT 2 with masked lanes and a second forward pass (4096 x 4 rows), VPT 16 at C = 768 (12 live), VPT 4 at C = 192 (3 live)
    (16403, 96, 1, dict(kernel="generic", fwd_grid=4096, fwd_passes=2, fwd_last=19, nblk=1024, bwd_passes=5, bwd_last=19, reduce="wide", trips=(8, 0))),
    (1029, 768, 1, dict(kernel="generic", fwd_passes=1, nblk=65, bwd_passes=4, bwd_last=249, reduce="wide", unrolled=0, tail_only=32)),
    (4100, 192, 1, dict(kernel="generic", fwd_passes=1, nblk=257, bwd_passes=4, bwd_last=1016, reduce="wide", unrolled=32, both=1)),
]
# (rows, C, groups, per-group parameters, what reached_bn must say)
BN = [
    # 98 partial rows: bn_stats_finalize lanes 0-1 unrolled, the rest tail only; chan_finalize unrolled 3 times, then a tail on lanes 0-1; rstep 1568 with a ragged eighth row
    (12500, 64, 1, 0, dict(g=1, grid=98, rstep=1568, first=(2, 0), last=(1, 3), ragged=1, fin_stats=dict(unrolled=2, both=0, tail_only=30, trips=(1, 0)),
                           fin_chan=dict(unrolled=8, both=2, tail_only=0, trips=(3, 1)))),
    # g = 5: 516 wanted -> the cap 512 -> 515; g = 3: 49 -> 51
    (13200, 320, 1, 0, dict(g=5, want=516, grid=515, rstep=1648, first=(2, 1), last=(2, 0), ragged=1)),
    (4099, 96, 1, 0, dict(g=3, want=49, grid=51, rstep=544, first=(2, 0), last=(1, 3), ragged=1)),
    # groups: per-group part / ws / mean at more than 24 rows per group; shared parameters: bn_bwd_apply's cross-group sum into one dgamma row
    (4 * 3125, 64, 4, 0, dict(g=1, grid=25, rstep=400, ragged=1, fin_chan=dict(unrolled=1, both=0, tail_only=7, trips=(1, 0)))),
    (4 * 3125, 64, 4, 1, dict(grid=25)),
    (2 * 6600, 320, 2, 0, dict(g=5, want=258, grid=260, rstep=832, ragged=1)),
    (2 * 6600, 320, 2, 1, dict(grid=260)),
]
# (rows, C, rows per sample, Dropout2d p, what reached_bn_rowdot must say)
BN_ROWDOT = [
    (32805, 256, 6561, 0.0, dict(fwd_grid=8192, fwd_passes=2, fwd_last=37, grid=512, C2=772)),
    # a sample boundary inside a pass of the forward, C2 = 1540 columns through chan_finalize at 257 rows
    (4100, 512, 1025, 0.25, dict(fwd_passes=1, grid=257, C2=1540, fin_chan=dict(unrolled=8, both=1, tail_only=0, trips=(8, 1)))),
    (2100, 1024, 525, 0.0, dict(grid=263, C2=3076)),
]
# (rows, N, what reached_colsum must say): reduce_partials_kernel<4>, <32>, the wide kernel tail only / mixed / at the cap; N = 960: g = 15
COLSUM = [
    (1000, 64, dict(grid=8, reduce="4", vector=1)),
    (5100, 64, dict(grid=40, reduce="32", vector=1, unrolled=0, tail_only=32)),
    (8200, 64, dict(grid=65, reduce="wide", unrolled=0, tail_only=32)),
    (30700, 64, dict(grid=240, reduce="wide", unrolled=32, both=16)),
    (131100, 64, dict(want=1025, grid=1024, reduce="wide", trips=(8, 0), ragged=1)),
    (300, 960, dict(g=15, want=36, grid=45, reduce="32", ragged=1)),
]
# (rows, K, what reached_rowdot must say): stride K + 1 -- the scalar loops of reduce_partials_kernel<4>, <32>, <256>; a second pass of the backward past 4096 rows
ROWDOT = [
    (40, 64, dict(nblk=10, reduce="4", vector=0)),
    (200, 64, dict(nblk=50, reduce="32", vector=0)),
    (1100, 64, dict(nblk=275, reduce="256", vector=0, trips=(0, 2))),
    (4133, 64, dict(nblk=1024, bwd_passes=2, bwd_last=37, reduce="256", vector=0, trips=(0, 4))),
    (4133, 512, dict(nblk=1024, bwd_passes=2, bwd_last=37, reduce="256", vector=0)),
    # the forward's second pass (8192 workgroups x 4 rows)
    (32805, 256, dict(fwd_grid=8192, fwd_passes=2, fwd_last=37, nblk=1024, bwd_passes=9, reduce="256", vector=0)),
]
# the masked-copy-only column pass behind the masked LayerNorm test: cap 4096
MASK_ONLY = [(4 * 16389, 128, dict(want=1025, grid=1025, ragged=1))]

REACH = ([("ln", s[:3], s[-1]) for s in LN] + [("bn", (s[0], s[1], s[2]), s[-1]) for s in BN] + [("bn_rowdot", s[:2], s[-1]) for s in BN_ROWDOT]
         + [("colsum", s[:2], s[-1]) for s in COLSUM] + [("rowdot", s[:2], s[-1]) for s in ROWDOT] + [("mask_only", s[:2], s[-1]) for s in MASK_ONLY])
_REACHED = dict(ln=reached_ln, bn=reached_bn, bn_rowdot=reached_bn_rowdot, colsum=reached_colsum, rowdot=reached_rowdot, mask_only=lambda M, N: reached_colsum(M, N, out=False))


@pytest.mark.parametrize("kind,shape,want", REACH, ids=[f"{k}-{_sid(s)}-{i}" for i, (k, s, _) in enumerate(REACH)])
def test_the_shape_reaches_the_code_it_is_listed_for(kind, shape, want):
    assert not os.environ.get("MDVIT_LN_BWD_ROWS") and os.environ.get("MDVIT_REDUCE_WIDE", "1") != "0"
    got = _REACHED[kind](*shape)
    assert {k: got.get(k) for k in want} == want, got


def test_the_restated_chan_grid_is_the_librarys():
    """mdvit_bn_ws_bytes = groups (2 C doubles + grid x 2 C floats), mdvit_bn_rowdot_ws_bytes = (3 C + 4) doubles + grid x (3 C + 4) floats: chan_grid through the size"""
    from mdvit_amd import _lib
    lib = _lib.load()
    cases = [(s[0], s[1], s[2]) for s in BN] + [(M, C, 1) for M in (1, 7, 129, 4099, 70000, 1 << 20) for C in (4, 36, 64, 96, 320, 960, 1024, 4096)]
    for M, C, G in cases:
        assert lib.mdvit_bn_ws_bytes(M, C, G) == G * (16 * C + 8 * C * chan_grid(M // G, C, CHAN_MAX_BLOCKS)), (M, C, G)
    for M, C in [s[:2] for s in BN_ROWDOT] + [(c[0], c[1]) for c in cases]:
        assert lib.mdvit_bn_rowdot_ws_bytes(M, C) == (8 + 4 * chan_grid(M, C, CHAN_MAX_BLOCKS)) * (3 * C + 4), (M, C)


def test_no_caller_reaches_the_vector_loop_of_the_256_lane_second_stage():
    """With the wide kernel on, reduce_partials_kernel<256> never runs its float4 loops: vec needs stride % 4 == 0, every caller passes n0 + n1 == stride, so n % 4 == 0 and
    64 or more rows go to the wide kernel.  (The same holds for its `vec && c + 3 >= n` element path at any LPQ.)  Unreachable code, listed in docs/history.md."""
    for nblk in (256, 257, 1024, 2048):
        for stride in range(1, 70):
            r = reached_reduce(nblk, stride, stride)
            assert r["reduce"] == "wide" or (r["reduce"] == "256" and r["vector"] == 0), (nblk, stride, r)


# ---- measures ---------------------------------------------------------------------------------------------------------------------------------------------------
def unit_errors(got, ref, unit, groups=1):
    """max |got - ref| / max |ref| inside a unit.  rows: each row of [M, C]; cols: each (group, channel) column; elem / scalar: each element; all: the tensor (a 1-output
    product).  A unit that is all zero in the reference (a channel whose every sample Dropout2d dropped) must be exactly zero: error 0, else infinite."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    if unit == "all":
        num, den = (got - ref).abs().max().reshape(1), ref.abs().max().reshape(1)
    elif unit in ("elem", "scalar"):
        num, den = (got - ref).abs(), ref.abs()
    else:
        C = ref.shape[-1]
        got, ref = (got.reshape(-1, C), ref.reshape(-1, C)) if unit == "rows" else (got.reshape(groups, -1, C), ref.reshape(groups, -1, C))
        num, den = (got - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
    zero = den == 0
    return torch.where(zero, torch.where(num == 0, 0.0, float("inf")).double(), num / torch.where(zero, torch.ones_like(den), den))


def measure(where, got, ref, base, spec, groups=1):
    """[(label, worst error of got, of the fp32 CPU evaluation)] for spec = [(name, unit), ...]; got = None: the CPU evaluations alone.  Every figure is printed."""
    out = []
    for name, unit in spec:
        e_base = float(unit_errors(base[name], ref[name], unit, groups).max())
        if got is None:
            print(f"{where} {name} by {unit}: fp32-cpu {e_base:.3e}")
            out.append((f"{name}/{unit}", None, e_base))
            continue
        assert tuple(got[name].shape) == tuple(ref[name].shape), (name, tuple(got[name].shape), tuple(ref[name].shape))
        e_got = float(unit_errors(got[name], ref[name], unit, groups).max())
        print(f"{where} {name} by {unit}: op {e_got:.3e}  fp32-cpu {e_base:.3e}  ratio {e_got / max(e_base, 1e-300):.2f}  bound {FACTOR * e_base:.3e}")
        out.append((f"{name}/{unit}", e_got, e_base))
    return out


def _bound(label, e_base):
    """FACTOR x the fp32 CPU evaluation's error; for a unit of ONE number (rowdot's db) not below FACTOR roundings: a single fp32 result is off by up to 2^-24 of itself
    however it is summed, and the CPU evaluation of one number can land on the correctly rounded one (error 0) by luck"""
    return FACTOR * (max(e_base, ULP) if label.endswith("/scalar") else e_base)


def held(where, got, ref, base, spec, groups=1):
    """the worst unit of got[name] is within FACTOR x that of the fp32 CPU evaluation base[name], which itself stays below BASE_LIMIT; all tensors are measured first"""
    figures = measure(where, got, ref, base, spec, groups)
    loose = [(n, b) for n, _, b in figures if not b <= BASE_LIMIT]
    bad = [(n, e, b) for n, e, b in figures if not (math.isfinite(e) and e <= _bound(n, b))]
    assert not loose, f"{where}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (tensor, worst error) {loose}"
    assert not bad, f"{where}: (tensor, worst error, fp32 CPU worst error) {bad}"


def well_conditioned(where, ref, base, spec, groups=1):
    """the guard alone, on the CPU: the inputs of a case were settled with this"""
    loose = [(n, b) for n, _, b in measure(where, None, ref, base, spec, groups) if not b <= BASE_LIMIT]
    assert not loose, f"{where}: ill-conditioned measure, the fp32 CPU evaluation itself is off by (tensor, worst error) {loose}"


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _leaf(t, dtype):
    return t.detach().clone().to(dtype).requires_grad_(True)


def _gpu(t, grad=False):
    return None if t is None else t.detach().to(dev()).requires_grad_(grad)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=dev())


def _abi():
    from mdvit_amd import _lib
    from mdvit_amd.ops import _p, _stream
    return _lib.load(), _p, _stream


def run(name, *args):
    """a C-ABI entry: the return code (0: done; E_WORKSPACE: refused before any launch)"""
    from mdvit_amd import _lib
    return getattr(_lib.load(), name)(*args)


def ok(name, *args):
    from mdvit_amd import _lib
    _lib.check(run(name, *args), name)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------------------
LN_SPEC = [("y", "rows"), ("y", "cols"), ("dx", "rows"), ("dx", "cols"), ("dgamma", "elem"), ("dbeta", "elem")]


def ln_inputs(M, C, G):
    """x: test_layernorm's with a per-column offset of +-1.5 (x-hat then has a column mean of about +-0.8 and dgamma = sum dy x-hat grows with the row count); dy + 0.5"""
    col = 1.5 * (1 - 2 * (torch.arange(C) % 2)).float()
    return dict(x=rnd(M, C, seed=30, scale=2.0) + 0.5 + col, ga=1 + 0.5 * rnd(G, C, seed=31), be=rnd(G, C, seed=32, scale=0.1), g=rnd(M, C, seed=33) + 0.5,
                add=rnd(M, C, seed=34))


def ln_cpu(inp, dtype, G):
    x, ga, be = _leaf(inp["x"], dtype), _leaf(inp["ga"], dtype), _leaf(inp["be"], dtype)
    M, C = x.shape
    y = torch.cat([F.layer_norm(x[i * (M // G):(i + 1) * (M // G)], (C,), ga[i], be[i], 1e-6) for i in range(G)], 0)
    y.backward(inp["g"].to(dtype))
    return dict(y=y.detach().double(), dx=x.grad.double(), dgamma=ga.grad.double(), dbeta=be.grad.double())


def ln_gpu(inp, G, eps=1e-6, fork=False):
    from mdvit_amd import ops
    x, ga, be = _gpu(inp["x"], True), _gpu(inp["ga"] if G > 1 else inp["ga"][0], True), _gpu(inp["be"] if G > 1 else inp["be"][0], True)
    if fork:
        y, xr = ops.layer_norm_fork(x, ga, be, eps)
        torch.autograd.backward([y, xr], [_gpu(inp["g"]), _gpu(inp["add"])])
    else:
        y = ops.layer_norm(x, ga, be, eps)
        y.backward(_gpu(inp["g"]))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=x.grad, dgamma=ga.grad.view(G, -1), dbeta=be.grad.view(G, -1))


@pytest.fixture(scope="module", params=LN, ids=[_sid(s) for s in LN])
def ln_case(request):
    M, C, G, _ = request.param
    inp = ln_inputs(M, C, G)
    return dict(where=f"layernorm ({M},{C}) groups {G}", G=G, inp=inp, ref=ln_cpu(inp, torch.float64, G), base=ln_cpu(inp, torch.float32, G), got=ln_gpu(inp, G), again=ln_gpu(inp, G))


def test_layernorm_values_by_the_worst_row_column_and_element(ln_case):
    held(ln_case["where"], ln_case["got"], ln_case["ref"], ln_case["base"], LN_SPEC, ln_case["G"])


def test_layernorm_twice_is_bit_equal(ln_case):
    assert same_bits(ln_case["got"], ln_case["again"])


def int_matrix(M, C):
    """(7 row + 3 c) % 5 - 2: small integers that weight every row differently"""
    return ((7 * torch.arange(M)[:, None] + 3 * torch.arange(C)[None, :]) % 5 - 2).float()


def random_int_matrix(M, C, seed=5):
    """seeded integers in [-2, 2]: no two rows weigh alike (the matrix above repeats every 5 rows, and a column of a multiple of 5 rows sums to 0)"""
    return torch.randint(-2, 3, (M, C), generator=torch.Generator().manual_seed(seed)).float()


def sign_matrix(M, C):
    """+-1, half of every row each (C even): the row mean is 0 and the row variance 1 exactly; the sign depends on the row"""
    return (1 - 2 * ((torch.arange(C)[None, :] + torch.arange(M)[:, None] // 3) % 2)).float()


@pytest.mark.parametrize("M,C,G,_", LN, ids=[_sid(s) for s in LN])
def test_layernorm_counts_every_row_and_partial_row_once(M, C, G, _):
    """dy = the integer matrix: dbeta[g][c] is an exact integer.  x = +-1 rows with gamma = 1 and eps = 3: mean 0, rstd = rsqrt(1 + 3) = 0.5, x-hat = +-0.5 on every element,
    so dgamma[g][c] = 0.5 x an integer, exact too (asserted through the forward's own rstd: dgamma / s is the integer sum, with s the one rstd value, a power of two).  The
    forked form adds `add` to dx, to one rounding, and leaves the sums alone."""
    from mdvit_amd.ops import _p, _stream
    Mg = M // G
    inp = dict(x=sign_matrix(M, C), ga=torch.ones(G, C), be=torch.zeros(G, C), add=rnd(M, C, seed=34))
    x, ga, be = _gpu(inp["x"]), _gpu(inp["ga"]), _gpu(inp["be"])
    y, mean, rstd = _nan(M, C), _nan(M), _nan(M)
    ok("mdvit_layernorm_fwd", _p(x), _p(ga), _p(be), _p(y), _p(mean), _p(rstd), M, C, G, 3.0, _stream())
    s = float(rstd[0])
    assert torch.equal(rstd.cpu(), torch.full((M,), s)) and torch.equal(mean.cpu(), torch.zeros(M)) and math.frexp(s)[0] == 0.5, s
    assert torch.equal(y.cpu(), inp["x"] * s)
    for which, g in (("the issue's matrix", int_matrix(M, C)), ("seeded integers", random_int_matrix(M, C))):
        inp["g"] = g
        want_b = g.long().view(G, Mg, C).sum(1)
        want_g = (g * inp["x"]).long().view(G, Mg, C).sum(1)
        assert int(want_b.abs().max()) < 2 ** 24 and int(want_g.abs().max()) < 2 ** 24 and int(want_g.abs().max()) > 0
        plain, fork = ln_gpu(inp, G, eps=3.0), ln_gpu(inp, G, eps=3.0, fork=True)
        for r in (plain, fork):
            assert torch.equal(r["dbeta"].cpu(), want_b.float()), f"dbeta, {which}"
            assert torch.equal(r["dgamma"].cpu() / s, want_g.float()), f"dgamma, {which}"
    add = _gpu(inp["add"])         # (one rounding: the compiler may contract the kernel's rs * (...) + add into one fused multiply-add)
    assert bool(((fork["dx"] - (plain["dx"] + add)).abs() <= 2 * ULP * (plain["dx"].abs() + add.abs())).all()), "the forked form is dx + add"


def test_layernorm_bwd_masked_with_groups_past_the_first_pass():
    """mdvit_layernorm_bwd_masked at groups 4 x 16389 rows, C = 128, drop_p 0.1 and a row scale: dx, dgamma, dbeta are mdvit_layernorm_bwd's, and dx_masked is dx x (the
    dropout mask x the row scale) bit for bit, the factor read from mdvit_colsum_f32's masked copy of a ones matrix under the same key -- at grow0 > 0 (the mask and scale
    indices of groups 1-3) and in passes 2 to 5 of the row loop.  NaN-filled outputs come back finite, a sentinel row behind dx and dx_masked untouched; the workspace is
    exactly the restated nblk x groups x 2 C floats, and 4 bytes less is refused before any launch."""
    from mdvit_amd.ops import _p, _stream
    M, C, G = LN[1][:3]
    r, d = reached_ln(M, C, G), dev()
    inp = ln_inputs(M, C, G)
    x, ga, be, g, add = (_gpu(inp[k]) for k in ("x", "ga", "be", "g", "add"))
    rps = 64
    gen = torch.Generator().manual_seed(7)
    rs = ((torch.rand(_cdiv(M, rps), generator=gen) > 0.3).float() / 0.7).to(d)
    y, mean, rstd = _nan(M, C), _nan(M), _nan(M)
    ok("mdvit_layernorm_fwd", _p(x), _p(ga), _p(be), _p(y), _p(mean), _p(rstd), M, C, G, 1e-6, _stream())
    ones, factor = torch.ones(M, C, device=d), _nan(M, C)
    ok("mdvit_colsum_f32", _p(ones), C, None, _p(factor), None, 0, M, C, 0.1, KEY[0], KEY[1], _p(rs), rps, 0, None, _stream())
    wsb = 4 * r["nblk"] * G * 2 * C
    res = []
    for masked in (False, True, True):
        dx, dxm, dg, db, ws = _nan(M + 1, C), _nan(M + 1, C), _nan(G, C), _nan(G, C), _nan(wsb // 4 + SLACK_ROWS * 2 * C)
        dx[M], dxm[M] = 12345.0, 12345.0
        if masked:
            args = (_p(g), _p(x), _p(ga), _p(mean), _p(rstd), _p(add), _p(dx), _p(dxm), _p(dg), _p(db), _p(ws))
            assert run("mdvit_layernorm_bwd_masked", *args, wsb - 4, M, C, G, 0.1, KEY[0], KEY[1], _p(rs), rps, None, _stream()) == E_WORKSPACE
            torch.cuda.synchronize()
            assert bool(torch.isnan(dx[:M]).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"
            ok("mdvit_layernorm_bwd_masked", *args, wsb, M, C, G, 0.1, KEY[0], KEY[1], _p(rs), rps, None, _stream())
        else:
            ok("mdvit_layernorm_bwd", _p(g), _p(x), _p(ga), _p(mean), _p(rstd), _p(add), _p(dx), _p(dg), _p(db), _p(ws), wsb, M, C, G, _stream())
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in (dx, dg, db, ws[:wsb // 4])) and (not masked or bool(torch.isfinite(dxm).all()))
        assert bool(torch.isnan(ws[wsb // 4:]).all()), "a partial row past the workspace was written"
        assert bool((dx[M] == 12345.0).all()) and (not masked or bool((dxm[M] == 12345.0).all())), "a row past the tensor was written"
        res.append(dict(dx=dx[:M], dxm=dxm[:M], dg=dg, db=db))
    plain, fused, again = res
    assert torch.equal(fused["dx"], plain["dx"]) and torch.equal(fused["dg"], plain["dg"]) and torch.equal(fused["db"], plain["db"])
    assert torch.equal(fused["dxm"], fused["dx"] * factor)
    assert same_bits(fused, again)
    keep = float((factor != 0).float().mean())
    assert abs(keep - 0.9 * float((rs != 0).float().mean())) < 0.01, keep
    ref = ln_cpu(inp, torch.float64, G)
    assert relerr(fused["dx"], ref["dx"] + inp["add"].double()) <= TOL


@pytest.mark.parametrize("M,C,G", [s[:3] for s in LN if s[2] == 1], ids=[_sid(s) for s in LN if s[2] == 1])
def test_layernorm_leaves_nothing_unwritten_and_writes_nothing_else(M, C, G):
    """NaN-filled y, mean, rstd, dx, dgamma, dbeta and workspace come back finite; the sentinel row behind y and dx comes back untouched; the workspace is exactly the
    restated partial rows (both sides of the rows_wg switch: the partial-row count is the one thing the switch changes), 4 bytes less is refused, and the SLACK_ROWS rows
    behind it that the test owns stay NaN"""
    from mdvit_amd.ops import _p, _stream
    r, inp = reached_ln(M, C, G), ln_inputs(M, C, G)
    x, ga, be, g = (_gpu(inp[k]) for k in ("x", "ga", "be", "g"))
    y, mean, rstd, dx, dg, db = _nan(M + 1, C), _nan(M), _nan(M), _nan(M + 1, C), _nan(G, C), _nan(G, C)
    y[M], dx[M] = 12345.0, 12345.0
    wsb = 4 * r["nblk"] * G * 2 * C
    ws = _nan(wsb // 4 + SLACK_ROWS * 2 * C)
    ok("mdvit_layernorm_fwd", _p(x), _p(ga), _p(be), _p(y), _p(mean), _p(rstd), M, C, G, 1e-6, _stream())
    args = (_p(g), _p(x), _p(ga), _p(mean), _p(rstd), None, _p(dx), _p(dg), _p(db), _p(ws))
    assert run("mdvit_layernorm_bwd", *args, wsb - 4, M, C, G, _stream()) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx[:M]).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"
    ok("mdvit_layernorm_bwd", *args, wsb, M, C, G, _stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (y, mean, rstd, dx, dg, db, ws[:wsb // 4]))
    assert bool(torch.isnan(ws[wsb // 4:]).all()), "a partial row past the workspace was written"
    assert bool((y[M] == 12345.0).all()) and bool((dx[M] == 12345.0).all()), "a row past the tensor was written"


# ---- BatchNorm: (a) the statistics ----------------------------------------------------------------------------------------------------------------------------------
SIGMA = 2.0 / 3.0 ** 0.5           # of rnd(...) * 2


def bn_y(M, C, G, sigmas=0.0):
    """test_bn_act_train's rnd * 2 + 0.3, groups apart by 0.5 (test_bn_act_grouped_equals_consecutive_forwards); sigmas: a per-channel mean of +-`sigmas` standard deviations"""
    y = rnd(M, C, seed=80, scale=2.0) + 0.3 + 0.5 * torch.arange(G).repeat_interleave(M // G)[:, None].float()
    return y + sigmas * SIGMA * (1 - 2 * (torch.arange(C) % 2)).float()


def bn_stats_gpu(y, G, pga, rm=None, rv=None, nbt=None, momentum=0.1, short=0):
    """mdvit_bn_stats on NaN-filled outputs and workspace -> (code, mean [G, C], rstd [G, C], the workspace's doubles, its partial rows)"""
    lib, _p, _stream = _abi()
    M, C = y.shape
    wsb = lib.mdvit_bn_ws_bytes(M, C, G)
    ws = _nan(wsb // 4)                     # (two fp32 NaNs read as one double: a NaN too)
    mean, rstd = _nan(G, C), _nan(G, C)
    code = run("mdvit_bn_stats", _p(y), _p(ws), wsb - short, _p(mean), _p(rstd), _p(rm), _p(rv), None if nbt is None else nbt.data_ptr(), M, C, G, pga, EPS_BN, momentum, _stream())
    torch.cuda.synchronize()
    return code, mean, rstd, ws[:G * 4 * C].view(torch.float64), ws[G * 4 * C:]


def stats_fp64(y, G):
    yd = y.double().view(G, -1, y.shape[1])
    return yd.mean(1), yd.var(1, unbiased=False)


BN_STATS = [(s[0], s[1], s[2]) for s in BN if not s[3]]


@pytest.mark.parametrize("M,C,G", BN_STATS, ids=[_sid(s) for s in BN_STATS])
@pytest.mark.parametrize("sigmas", [0.0, 4.0, 32.0], ids=["plain", "4-sigma", "32-sigma"])
def test_bn_stats_against_the_conditioning_of_its_formula(M, C, G, sigmas):
    """rstd, and the variance recovered from it, per channel against fp64: FACTOR 2^-24 (1 + mean^2 / var) -- the condition number of E[x^2] - E[x]^2 times one rounding times the
    project's factor; mean: FACTOR 2^-24 max(|mean|, std).  Asserted at the existing tests' inputs and at a mean of 4 standard deviations; 32: printed only.  Twice: bit-equal;
    the NaN-filled workspace comes back finite; 4 bytes less than mdvit_bn_ws_bytes is refused before any launch."""
    y = bn_y(M, C, G, sigmas)
    mu, var = stats_fp64(y, G)
    yd = _gpu(y)
    code, mean, rstd, ws, part = bn_stats_gpu(yd, G, 0, short=4)
    assert code == E_WORKSPACE and bool(torch.isnan(mean).all()) and bool(torch.isnan(part).all()), "a short workspace must be refused before any launch"
    code, mean, rstd, ws, part = bn_stats_gpu(yd, G, 0)
    assert code == 0 and all(bool(torch.isfinite(t).all()) for t in (mean, rstd, ws, part))
    again = bn_stats_gpu(yd, G, 0)
    assert torch.equal(mean, again[1]) and torch.equal(rstd, again[2]) and torch.equal(part, again[4])
    cond = 1 + mu * mu / var
    e_mean = (mean.double().cpu() - mu).abs() / torch.maximum(mu.abs(), var.sqrt())
    e_rstd = (rstd.double().cpu() * (var + EPS_BN).sqrt() - 1).abs()
    e_var = ((rstd.double().cpu() ** -2 - EPS_BN) / var - 1).abs()
    r_rstd, r_var = float((e_rstd / (ULP * cond)).max()), float((e_var / (ULP * cond)).max())
    print(f"bn_stats ({M},{C}) groups {G} at {sigmas:g} sigma: mean {float(e_mean.max()):.3e} ({float(e_mean.max()) / ULP:.2f} x 2^-24)  rstd {float(e_rstd.max()):.3e}  "
          f"variance {float(e_var.max()):.3e}  conditioning {float(cond.max()):.0f}  rstd / variance over 2^-24 x conditioning: {r_rstd:.2f} / {r_var:.2f} (bound {FACTOR:g})")
    if sigmas <= 4.0:
        assert float(e_mean.max()) <= FACTOR * ULP and r_rstd <= FACTOR and r_var <= FACTOR


@pytest.mark.parametrize("M,C,G,pga,_", BN, ids=[_sid(s) for s in BN])
def test_bn_stats_counts_every_row_and_partial_row_once(M, C, G, pga, _):
    """integer y in [-3, 3]: S1 and S2 are integers below 2^24, exact in the fp32 partial rows and the double second stage.  mean == float32(S1 / M) bit for bit; rstd within 1 ulp
    of float32(1 / sqrt(S2 / M - (S1 / M)^2 + eps)) in double; the running statistics within the rounding of bn_stats_finalize_kernel's fp32 update
    (1 - momentum) r + momentum v, 2^-23 (|(1 - momentum) r| + |momentum v|) per update; nbt advances by `groups`, or by one per row with per-group parameters."""
    Mg, mom = M // G, 0.1
    y = ((11 * torch.arange(M)[:, None] + 5 * torch.arange(C)[None, :] + torch.arange(M)[:, None] // 7) % 7 - 3).float()
    S1, S2 = y.long().view(G, Mg, C).sum(1), (y * y).long().view(G, Mg, C).sum(1)
    m = S1.double() / Mg
    var = (S2.double() / Mg - m * m).clamp_min(0)
    R = G if pga else 1
    rm0, rv0 = rnd(R, C, seed=84, scale=0.1), 1 + 0.5 * rnd(R, C, seed=85)
    rm, rv, nbt = _gpu(rm0), _gpu(rv0), torch.full((R,), 3, dtype=torch.long, device=dev())
    code, mean, rstd, ws, part = bn_stats_gpu(_gpu(y), G, pga, rm, rv, nbt, mom)
    assert code == 0
    assert torch.equal(ws.cpu().view(G, 2, C), torch.stack((S1, S2), 1).double()), "the sums"
    assert torch.equal(mean.cpu(), m.float()), "mean"
    want = (1 / (var + float(torch.tensor(EPS_BN, dtype=torch.float32))).sqrt()).float()
    assert int((rstd.cpu().view(torch.int32) - want.view(torch.int32)).abs().max()) <= 1, "rstd"
    unb = (var * (Mg / (Mg - 1))).float().double()
    c1, c2 = float(torch.tensor(1.0) - torch.tensor(mom)), float(torch.tensor(mom, dtype=torch.float32))
    for got, r0, v in ((rm, rm0.double(), m.float().double()), (rv, rv0.double(), unb)):
        if pga:
            want, slack = c1 * r0 + c2 * v, (c1 * r0).abs() + (c2 * v).abs()
        else:
            want, slack = r0[0], torch.zeros(C, dtype=torch.float64)
            for g in range(G):
                slack = slack + (c1 * want).abs() + (c2 * v[g]).abs()
                want = c1 * want + c2 * v[g]
        assert bool(((got.double().cpu().view(want.shape) - want).abs() <= 2 * ULP * slack).all()), "running statistics"
    assert nbt.tolist() == ([4] * G if pga else [3 + G])


# ---- BatchNorm: (b) the apply and backward kernels with the statistics given ------------------------------------------------------------------------------------------
KINKS = {"relu": (0.0,), "hswish": (-3.0, 3.0), "none": ()}


def act_fn(act, pre):
    return torch.relu(pre) if act == "relu" else (F.hardswish(pre) if act == "hswish" else pre)


def act_grad(act, pre):
    if act == "relu":
        return (pre > 0).to(pre.dtype)
    if act == "hswish":
        return torch.where(pre < -3, torch.zeros_like(pre), torch.where(pre > 3, torch.ones_like(pre), (2 * pre + 3) / 6))
    return torch.ones_like(pre)


def _act_code(act):
    from mdvit_amd import _lib
    return dict(relu=_lib.ACT_RELU, hswish=_lib.ACT_HSWISH, none=_lib.ACT_NONE)[act]


def off_the_kinks(y, mu, rs, ga, be, act, G):
    """y with every pre-activation that lies within 1e-3 of a kink of `act` moved to 2e-3 from it (mu, rs, ga, be: fp64 [G or 1, C])"""
    M, C = y.shape
    yd = y.double().view(G, -1, C)
    mu, rs, ga, be = (t.double().view(-1, 1, C) for t in (mu, rs, ga, be))
    pre = (yd - mu) * rs * ga + be
    for k in KINKS[act]:
        near = (pre - k).abs() < 1e-3
        side = torch.where(pre >= k, torch.ones_like(pre), -torch.ones_like(pre))
        yd = torch.where(near, (k + 2e-3 * side - be) / (ga * rs) + mu, yd)
    return yd.reshape(M, C).float()


def bn_formula(inp, dtype):
    """BatchNorm -> activation -> Dropout2d and its backward with GIVEN statistics, in plain torch on the CPU in `dtype` (test_the_bn_formula_is_fp64_autograd holds it against
    F.batch_norm): z, dy, dgamma, dbeta; with w (the fused 1-output conv of bn_rowdot: dz = g w^T): low, dw, db too"""
    G, C = inp["G"], inp["y"].shape[1]
    y, mu, rs = inp["y"].to(dtype).view(G, -1, C), inp["mean"].to(dtype).view(G, 1, C), inp["rstd"].to(dtype).view(G, 1, C)
    ga, be = inp["ga"].to(dtype).view(-1, 1, C), inp["be"].to(dtype).view(-1, 1, C)
    ds = torch.ones((), dtype=dtype) if inp.get("ds") is None else inp["ds"].to(dtype).view(G, -1, C)
    Mg = y.shape[1]
    xh = (y - mu) * rs
    pre = xh * ga + be
    z = act_fn(inp["act"], pre) * ds
    out = {}
    if "w" in inp:
        w, gv = inp["w"].to(dtype).view(1, 1, C), inp["g"].to(dtype).view(G, -1, 1)
        dz = gv * w
        out.update(low=((z * w).sum(2) + inp["b"].to(dtype)).reshape(-1).double(), dw=(gv * z).sum((0, 1)).double(), db=gv.sum().reshape(1).double())
    else:
        dz = inp["dz"].to(dtype).view(G, -1, C)
        out.update(z=z.reshape(-1, C).double())
    g = dz * act_grad(inp["act"], pre) * ds
    s1, s2 = g.sum(1, keepdim=True), (g * xh).sum(1, keepdim=True)
    dy = ga * rs * (g - s1 / Mg - xh * (s2 / Mg)) if inp["training"] else ga * rs * g
    pga = inp["ga"].shape[0] == G and G > 1
    out.update(dy=dy.reshape(-1, C).double(), dgamma=(s2[:, 0] if pga else s2.sum(0)).double(), dbeta=(s1[:, 0] if pga else s1.sum(0)).double())
    return out


@pytest.mark.parametrize("act", ["relu", "hswish"])
def test_the_bn_formula_is_fp64_autograd(act):
    """bn_formula with the batch's own statistics is autograd through F.batch_norm and the activation (fp64, no GPU)"""
    M, C = 300, 8
    y, ga, be, dz = rnd(M, C, seed=80, scale=2.0) + 0.3, 1 + 0.5 * rnd(1, C, seed=81), rnd(1, C, seed=82, scale=0.2), rnd(M, C, seed=83) + 0.5
    mu, var = stats_fp64(y, 1)
    f = bn_formula(dict(G=1, y=y, mean=mu, rstd=1 / (var + EPS_BN).sqrt(), ga=ga, be=be, dz=dz, act=act, training=True), torch.float64)
    yl, gl, bl = _leaf(y, torch.float64), _leaf(ga[0], torch.float64), _leaf(be[0], torch.float64)
    z = act_fn(act, F.batch_norm(yl, None, None, gl, bl, True, 0.1, EPS_BN))
    z.backward(dz.double())
    for a, b in ((f["z"], z.detach()), (f["dy"], yl.grad), (f["dgamma"][0], gl.grad), (f["dbeta"][0], bl.grad)):
        assert relerr(a, b) < 1e-12


# (index into BN, activation, training, Dropout2d p, rows per sample, sigmas)
BN_APPLY = [
    (0, "relu", True, 0.0, 625, 0.0), (0, "hswish", True, 0.25, 625, 4.0), (0, "relu", False, 0.25, 625, 0.0),
    (1, "hswish", True, 0.0, 330, 0.0), (1, "relu", True, 0.25, 330, 4.0), (1, "hswish", False, 0.0, 330, 4.0),
    (2, "relu", True, 0.25, 1025, 0.0), (2, "hswish", True, 0.0, 1025, 4.0),
    (3, "relu", True, 0.25, 625, 4.0), (4, "hswish", True, 0.0, 625, 0.0), (5, "hswish", True, 0.25, 330, 0.0), (6, "relu", True, 0.0, 330, 4.0),
]


def bn_inputs(M, C, G, pga, act, training, drop, rps, sigmas):
    """y off the kinks; the statistics: the fp64 batch statistics of that y (training) or running statistics (eval), rounded to fp32; dz + 0.5"""
    R = G if pga else 1
    y, ga, be = bn_y(M, C, G, sigmas), 1 + 0.5 * rnd(R, C, seed=81), rnd(R, C, seed=82, scale=0.2)
    mu, var = stats_fp64(y, G)
    if not training:
        mu, var = mu + rnd(G, C, seed=93, scale=0.3).double(), var * (1 + 0.5 * rnd(G, C, seed=94)).double()
    y = off_the_kinks(y, mu, 1 / (var + EPS_BN).sqrt(), ga, be, act, G)
    if training:
        mu, var = stats_fp64(y, G)
    return dict(G=G, pga=pga, y=y, ga=ga, be=be, act=act, training=training, drop=drop, rps=rps, mean=mu.float(), rstd=(1 / (var + EPS_BN).sqrt()).float(),
                dz=rnd(M, C, seed=83) + 0.5)


def bn_mask(M, C, G, drop, rps):
    """the Dropout2d factor (0 or 1 / keep) per element, read back from mdvit_bn_apply: z of an all-ones input under relu with mean 0, rstd 1, gamma 1, beta 0"""
    _, _p, _stream = _abi()
    one, zero, z = torch.ones(M, C, device=dev()), torch.zeros(G, C, device=dev()), _nan(M, C)
    ok("mdvit_bn_apply", _p(one), _p(zero), _p(one), _p(one), _p(zero), _p(z), M, C, G, 0, _act_code("relu"), drop, KEY[0], KEY[1], None, rps, _stream())
    torch.cuda.synchronize()
    return z.cpu()


def bn_gpu(inp):
    """mdvit_bn_apply and mdvit_bn_bwd on NaN-filled outputs and workspace, a sentinel row behind z and dy"""
    lib, _p, _stream = _abi()
    M, C = inp["y"].shape
    G, pga, R = inp["G"], inp["pga"], inp["ga"].shape[0]
    y, mean, rstd, ga, be, dz = (_gpu(inp[k]) for k in ("y", "mean", "rstd", "ga", "be", "dz"))
    z, dy, dg, db = _nan(M + 1, C), _nan(M + 1, C), _nan(R, C), _nan(R, C)
    z[M], dy[M] = 12345.0, 12345.0
    wsb = lib.mdvit_bn_ws_bytes(M, C, G)
    ws = torch.full((wsb // 8,), float("nan"), device=dev(), dtype=torch.float64)
    tail = (inp["drop"], KEY[0], KEY[1], None, inp["rps"], _stream())
    ok("mdvit_bn_apply", _p(y), _p(mean), _p(rstd), _p(ga), _p(be), _p(z), M, C, G, pga, _act_code(inp["act"]), *tail)
    args = (_p(dz), _p(y), _p(mean), _p(rstd), _p(ga), _p(be), _p(dy), _p(dg), _p(db), _p(ws))
    assert run("mdvit_bn_bwd", *args, wsb - 4, M, C, G, pga, _act_code(inp["act"]), int(inp["training"]), *tail) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(dy[:M]).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"
    ok("mdvit_bn_bwd", *args, wsb, M, C, G, pga, _act_code(inp["act"]), int(inp["training"]), *tail)
    torch.cuda.synchronize()
    assert bool((z[M] == 12345.0).all()) and bool((dy[M] == 12345.0).all()), "a row past the tensor was written"
    assert bool(torch.isfinite(ws[:G * 2 * C]).all()) and bool(torch.isfinite(ws[G * 2 * C:].view(torch.float32)).all()), "the workspace"
    return dict(z=z[:M], dy=dy[:M], dgamma=dg, dbeta=db)


BN_SPEC = [("z", "rows"), ("z", "cols"), ("dy", "rows"), ("dy", "cols"), ("dgamma", "elem"), ("dbeta", "elem")]


def _bn_id(c):
    i, act, training, drop, rps, sigmas = c
    return f"{_sid(BN[i])}-{act}-{'train' if training else 'eval'}-drop{drop:g}-{sigmas:g}sigma"


@pytest.fixture(scope="module", params=BN_APPLY, ids=_bn_id)
def bn_case(request):
    i, act, training, drop, rps, sigmas = request.param
    M, C, G, pga, _ = BN[i]
    if not training:
        G = 1                              # eval normalises every sample with the one set of running statistics (ops._BNAct.forward)
    inp = bn_inputs(M, C, G, pga and training, act, training, drop, rps, sigmas)
    if drop > 0:
        inp["ds"] = bn_mask(M, C, G, drop, rps)
    return dict(where=f"bn ({M},{C}) groups {G} {_bn_id(request.param)}", inp=inp, ref=bn_formula(inp, torch.float64), base=bn_formula(inp, torch.float32), got=bn_gpu(inp), again=bn_gpu(inp))


def test_bn_apply_and_bwd_values_by_the_worst_row_column_and_element(bn_case):
    inp = bn_case["inp"]
    if inp["drop"] > 0:
        planes = inp["ds"].view(-1, inp["rps"], inp["ds"].shape[1]) if inp["y"].shape[0] % inp["rps"] == 0 else inp["ds"][:inp["rps"]][None]
        assert bool((planes == planes[:, :1]).all()), "Dropout2d drops whole (sample, channel) planes"
        keep, scale, n = float((inp["ds"] != 0).float().mean()), float(inp["ds"].max()), _cdiv(inp["y"].shape[0], inp["rps"]) * inp["ds"].shape[1]
        assert scale == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(inp["drop"]))), scale
        assert abs(keep - (1 - inp["drop"])) < 4 * (inp["drop"] * (1 - inp["drop"]) / n) ** 0.5 + 0.01, (keep, n)       # four standard deviations of n planes (+ the ragged last sample)
    held(bn_case["where"], bn_case["got"], bn_case["ref"], bn_case["base"], BN_SPEC, inp["G"])


def test_bn_apply_and_bwd_twice_are_bit_equal(bn_case):
    assert same_bits(bn_case["got"], bn_case["again"])


E2E = [(4, 25, 125, 64, "relu"), (4, 50, 66, 320, "hswish"), (1, 4099, 1, 96, "relu")]


@pytest.mark.parametrize("B,H,W,C,act", E2E, ids=[_sid(s) for s in E2E])
def test_bn_act_end_to_end(B, H, W, C, act):
    """ops.bn_act (statistics + apply, backward) against fp64 autograd through F.batch_norm, the existing tests' inputs moved off the kinks; the running statistics to TOL"""
    from mdvit_amd import ops
    M = B * H * W
    inp = bn_inputs(M, C, 1, 0, act, True, 0.0, H * W, 0.0)
    rm0, rv0 = rnd(C, seed=84, scale=0.1), 1 + 0.5 * rnd(C, seed=85)

    def cpu(dtype):
        y, ga, be = _leaf(inp["y"], dtype), _leaf(inp["ga"][0], dtype), _leaf(inp["be"][0], dtype)
        rm, rv = rm0.clone().to(dtype), rv0.clone().to(dtype)
        z = act_fn(act, F.batch_norm(y, rm, rv, ga, be, True, 0.1, EPS_BN))
        z.backward(inp["dz"].to(dtype))
        return dict(z=z.detach().double(), dy=y.grad.double(), dgamma=ga.grad.double(), dbeta=be.grad.double(), rm=rm.double(), rv=rv.double())
    ref, base = cpu(torch.float64), cpu(torch.float32)
    y, ga, be = _gpu(inp["y"].view(B, H, W, C), True), _gpu(inp["ga"][0], True), _gpu(inp["be"][0], True)
    rm, rv, nbt = _gpu(rm0), _gpu(rv0), torch.tensor(3, device=dev())
    z = ops.bn_act(y, ga, be, rm, rv, nbt, True, _act_code(act))
    z.backward(_gpu(inp["dz"].view(B, H, W, C)))
    torch.cuda.synchronize()
    got = dict(z=z.detach().view(M, C), dy=y.grad.view(M, C), dgamma=ga.grad, dbeta=be.grad)
    assert relerr(rm, ref["rm"]) <= TOL and relerr(rv, ref["rv"]) <= TOL and int(nbt) == 4
    held(f"bn_act end to end ({M},{C}) {act}", got, ref, base, BN_SPEC)


# ---- BatchNorm -> activation -> Dropout2d -> 1-output conv ----------------------------------------------------------------------------------------------------------------
BNR_SPEC = [("low", "all"), ("dy", "rows"), ("dy", "cols"), ("dgamma", "elem"), ("dbeta", "elem"), ("dw", "elem"), ("db", "scalar")]
BN_ROWDOT_CASES = [(0, "hswish", True), (1, "relu", True), (1, "relu", False), (2, "relu", True)]


def bnr_gpu(inp):
    lib, _p, _stream = _abi()
    M, C = inp["y"].shape
    y, mean, rstd, ga, be, w, b, g = (_gpu(inp[k]) for k in ("y", "mean", "rstd", "ga", "be", "w", "b", "g"))
    low, dy, dg, db, dw, dbias = _nan(M + 1), _nan(M + 1, C), _nan(C), _nan(C), _nan(C), _nan(1)
    low[M], dy[M] = 12345.0, 12345.0
    wsb = lib.mdvit_bn_rowdot_ws_bytes(M, C)
    ws = torch.full((wsb // 8,), float("nan"), device=dev(), dtype=torch.float64)
    tail = (inp["drop"], KEY[0], KEY[1], None, inp["rps"], _stream())
    ok("mdvit_bn_rowdot_fwd", _p(y), _p(mean), _p(rstd), _p(ga), _p(be), _p(w), _p(b), _p(low), M, C, _act_code(inp["act"]), *tail)
    args = (_p(g), _p(y), _p(mean), _p(rstd), _p(ga), _p(be), _p(w), _p(dy), _p(dg), _p(db), _p(dw), _p(dbias), _p(ws))
    assert run("mdvit_bn_rowdot_bwd", *args, wsb - 4, M, C, _act_code(inp["act"]), int(inp["training"]), *tail) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(dy[:M]).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"
    ok("mdvit_bn_rowdot_bwd", *args, wsb, M, C, _act_code(inp["act"]), int(inp["training"]), *tail)
    torch.cuda.synchronize()
    assert float(low[M]) == 12345.0 and bool((dy[M] == 12345.0).all()), "a row past the tensor was written"
    assert bool(torch.isfinite(ws[:3 * C + 4]).all()) and bool(torch.isfinite(ws[3 * C + 4:].view(torch.float32)).all()), "the workspace"
    return dict(low=low[:M], dy=dy[:M], dgamma=dg.view(1, C), dbeta=db.view(1, C), dw=dw, db=dbias)


@pytest.fixture(scope="module", params=BN_ROWDOT_CASES, ids=lambda c: f"{_sid(BN_ROWDOT[c[0]])}-{c[1]}-{'train' if c[2] else 'eval'}")
def bnr_case(request):
    i, act, training = request.param
    M, C, rps, drop, _ = BN_ROWDOT[i]
    inp = bn_inputs(M, C, 1, 0, act, training, drop, rps, 0.0)
    inp.update(w=rnd(C, seed=303, scale=0.2) + 0.1, b=rnd(1, seed=304), g=rnd(M, seed=305) + 0.5)
    if drop > 0:
        inp["ds"] = bn_mask(M, C, 1, drop, rps)
    return dict(where=f"bn_rowdot ({M},{C}) {act} {'train' if training else 'eval'} drop {drop:g}", inp=inp, ref=bn_formula(inp, torch.float64), base=bn_formula(inp, torch.float32),
                got=bnr_gpu(inp), again=bnr_gpu(inp))


def test_bn_rowdot_values_by_the_worst_row_column_and_element(bnr_case):
    held(bnr_case["where"], bnr_case["got"], bnr_case["ref"], bnr_case["base"], BNR_SPEC)


def test_bn_rowdot_twice_is_bit_equal(bnr_case):
    assert same_bits(bnr_case["got"], bnr_case["again"])


# ---- column sums --------------------------------------------------------------------------------------------------------------------------------------------------
def colsum_gpu(A, N, drop=0.0, rs=None, rps=1, accumulate=0, pre=None, masked=False, short=0):
    """mdvit_colsum_f32 on the first N columns of A (lda = A's width) with a workspace of exactly the restated partial rows (and SLACK_ROWS NaN rows behind them that the
    library is not told of: they stay NaN) -> (code, out, masked copy, workspace)"""
    _, _p, _stream = _abi()
    M, nblk = A.shape[0], chan_grid(A.shape[0], N, 1024)
    out = _nan(N) if pre is None else pre.clone()
    mk, ws = (_nan(M + 1, N) if masked else None), _nan((nblk + SLACK_ROWS) * N)
    if masked:
        mk[M] = 12345.0
    code = run("mdvit_colsum_f32", _p(A), A.shape[1], _p(out), _p(mk), _p(ws), 4 * nblk * N - short, M, N, drop, KEY[0], KEY[1], _p(rs), rps, accumulate, None, _stream())
    torch.cuda.synchronize()
    assert not masked or bool((mk[M] == 12345.0).all()), "a row past the masked copy was written"
    assert bool(torch.isnan(ws[nblk * N:]).all()), "a partial row past the workspace was written"
    return code, out, (mk[:M] if masked else None), ws[:nblk * N]


@pytest.mark.parametrize("M,N,_", COLSUM, ids=[_sid(s) for s in COLSUM])
def test_colsum_counts_every_row_and_partial_row_once(M, N, _):
    """the integer matrix, and seeded integers: exact column sums; with an exact 0 / 2 row scale (64 rows each): the masked copy is the input times the scale bit for bit, the sums exact again"""
    gen = torch.Generator().manual_seed(11)
    rs = 2.0 * (torch.rand(_cdiv(M, 64), generator=gen) > 0.4).float()
    for A in (int_matrix(M, N), random_int_matrix(M, N)):
        Ad = _gpu(A)
        code, out, _, ws = colsum_gpu(Ad, N, short=4)
        assert code == E_WORKSPACE and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "a short workspace must be refused before any launch"
        code, out, _, ws = colsum_gpu(Ad, N)
        assert code == 0 and bool(torch.isfinite(ws).all())
        assert torch.equal(out.cpu(), A.long().sum(0).float())
        scaled = A * rs.repeat_interleave(64)[:M, None]
        code, out, mk, _ = colsum_gpu(Ad, N, rs=_gpu(rs), rps=64, masked=True)
        assert code == 0 and torch.equal(mk.cpu(), scaled) and torch.equal(out.cpu(), scaled.long().sum(0).float())


@pytest.mark.parametrize("M,N,_", COLSUM, ids=[_sid(s) for s in COLSUM])
def test_colsum_values_per_element(M, N, _):
    """A + 0.5 out of a wider matrix (lda = N + 8), plain and under dropout 0.1 x a row scale (the factor read back from the masked copy of a ones matrix); accumulate = 1 is
    the prefill plus the plain result, one fp32 add; twice: bit-equal"""
    A = rnd(M, N + 8, seed=60) + 0.5
    gen = torch.Generator().manual_seed(12)
    rs = ((torch.rand(_cdiv(M, 64), generator=gen) > 0.3).float() / 0.7)
    Ad, rsd = _gpu(A), _gpu(rs)
    _, _, factor, _ = colsum_gpu(torch.ones(M, N, device=dev()), N, drop=0.1, rs=rsd, rps=64, masked=True)
    factor = factor.cpu()
    _, plain, _, _ = colsum_gpu(Ad, N)
    _, dropped, mk, _ = colsum_gpu(Ad, N, drop=0.1, rs=rsd, rps=64, masked=True)
    assert torch.equal(mk.cpu(), A[:, :N] * factor)
    ref = dict(plain=A[:, :N].double().sum(0), dropped=(A[:, :N].double() * factor.double()).sum(0))
    base = dict(plain=A[:, :N].sum(0).double(), dropped=(A[:, :N] * factor).sum(0).double())
    held(f"colsum ({M},{N})", dict(plain=plain, dropped=dropped), ref, base, [("plain", "elem"), ("dropped", "elem")])
    pre = rnd(N, seed=61, scale=float(M)).to(dev())
    assert torch.equal(colsum_gpu(Ad, N, accumulate=1, pre=pre)[1], pre + plain), "accumulate"
    assert torch.equal(colsum_gpu(Ad, N)[1], plain) and torch.equal(colsum_gpu(Ad, N, drop=0.1, rs=rsd, rps=64, masked=True)[1], dropped)


# ---- rowdot -------------------------------------------------------------------------------------------------------------------------------------------------------
ROWDOT_SPEC = [("y", "all"), ("dx", "rows"), ("dx", "cols"), ("dw", "elem"), ("db", "scalar")]


def rowdot_inputs(M, K, wide):
    """x + 0.5 and g + 0.5 (dw = sum g x per element); wide: x is a column slice of a [M, K + 40] matrix (ldx = K + 40)"""
    X = rnd(M, K + (40 if wide else 0), seed=110) + 0.5
    return dict(X=X, lo=(24 if wide else 0), K=K, w=rnd(1, K, 1, 1, seed=111), b=rnd(1, seed=112), g=rnd(M, seed=113) + 0.5)


def rowdot_cpu(inp, dtype):
    X, w, b = _leaf(inp["X"], dtype), _leaf(inp["w"], dtype), _leaf(inp["b"], dtype)
    y = X[:, inp["lo"]:inp["lo"] + inp["K"]] @ w.view(-1) + b
    y.backward(inp["g"].to(dtype))
    return dict(y=y.detach().double(), dx=X.grad[:, inp["lo"]:inp["lo"] + inp["K"]].double(), dw=w.grad.reshape(-1).double(), db=b.grad.double())


def rowdot_gpu(inp):
    from mdvit_amd import ops
    X, w, b = _gpu(inp["X"], True), _gpu(inp["w"], True), _gpu(inp["b"], True)
    y = ops.rowdot(X[:, inp["lo"]:inp["lo"] + inp["K"]], w, b)
    y.backward(_gpu(inp["g"]))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=X.grad[:, inp["lo"]:inp["lo"] + inp["K"]], dw=w.grad.reshape(-1), db=b.grad)


ROWDOT_CASES = [(s[0], s[1], s[0] == 1100) for s in ROWDOT]


@pytest.fixture(scope="module", params=ROWDOT_CASES, ids=[_sid(s) for s in ROWDOT_CASES])
def rowdot_case(request):
    M, K, wide = request.param
    inp = rowdot_inputs(M, K, wide)
    return dict(where=f"rowdot ({M},{K}){' strided' if wide else ''}", inp=inp, ref=rowdot_cpu(inp, torch.float64), base=rowdot_cpu(inp, torch.float32), got=rowdot_gpu(inp), again=rowdot_gpu(inp))


def test_rowdot_values_by_the_worst_row_column_and_element(rowdot_case):
    held(rowdot_case["where"], rowdot_case["got"], rowdot_case["ref"], rowdot_case["base"], ROWDOT_SPEC)


def test_rowdot_twice_is_bit_equal(rowdot_case):
    assert same_bits(rowdot_case["got"], rowdot_case["again"])


@pytest.mark.parametrize("M,K,_", ROWDOT, ids=[_sid(s) for s in ROWDOT])
def test_rowdot_bwd_counts_every_row_and_partial_row_once(M, K, _):
    """integer dy: db = sum dy exactly; x = the integer matrix too: dw[k] = sum dy[m] x[m][k] exactly.  Through the C ABI with a workspace of exactly the restated nblk x (K + 1)
    floats (4 bytes less is refused), NaN-filled outputs, a sentinel row behind dx and y"""
    _, _p, _stream = _abi()
    x, g, w = int_matrix(M, K), ((3 * torch.arange(M)) % 7 - 3).float(), rnd(K, seed=111)
    xd, gd, wd = _gpu(x), _gpu(g), _gpu(w)
    nblk = reached_rowdot(M, K)["nblk"]
    dx, dw, db, ws, y = _nan(M + 1, K), _nan(K), _nan(1), _nan(nblk * (K + 1)), _nan(M + 1)
    dx[M], y[M] = 12345.0, 12345.0
    args = (_p(xd), K, _p(wd), _p(gd), _p(dx), K, _p(dw), _p(db), _p(ws))
    assert run("mdvit_rowdot_bwd", *args, 4 * nblk * (K + 1) - 4, M, K, _stream()) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx[:M]).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"
    ok("mdvit_rowdot_bwd", *args, 4 * nblk * (K + 1), M, K, _stream())
    ok("mdvit_rowdot_fwd", _p(xd), K, _p(wd), None, _p(y), M, K, 0, _stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (dx, dw, db, ws, y)) and bool((dx[M] == 12345.0).all()) and float(y[M]) == 12345.0
    assert torch.equal(db.cpu(), g.long().sum().float().reshape(1)) and torch.equal(dw.cpu(), (g[:, None] * x).long().sum(0).float())
    assert torch.equal(dx[:M].cpu(), g[:, None] * w[None, :])


# ---- the conditioning guards, on the CPU alone -----------------------------------------------------------------------------------------------------------------------
def conditioning_guards():
    """every value case's fp32 CPU evaluation against BASE_LIMIT, without a GPU (Dropout2d: no mask -- it only removes terms): the inputs above were settled with this"""
    for M, C, G, _ in LN:
        inp = ln_inputs(M, C, G)
        well_conditioned(f"layernorm ({M},{C}) groups {G}", ln_cpu(inp, torch.float64, G), ln_cpu(inp, torch.float32, G), LN_SPEC, G)
    for c in BN_APPLY:
        i, act, training, drop, rps, sigmas = c
        M, C, G, pga, _ = BN[i]
        G = G if training else 1
        inp = bn_inputs(M, C, G, pga and training, act, training, drop, rps, sigmas)
        well_conditioned(f"bn {_bn_id(c)}", bn_formula(inp, torch.float64), bn_formula(inp, torch.float32), BN_SPEC, G)
    for i, act, training in BN_ROWDOT_CASES:
        M, C, rps, drop, _ = BN_ROWDOT[i]
        inp = bn_inputs(M, C, 1, 0, act, training, drop, rps, 0.0)
        inp.update(w=rnd(C, seed=303, scale=0.2) + 0.1, b=rnd(1, seed=304), g=rnd(M, seed=305) + 0.5)
        well_conditioned(f"bn_rowdot ({M},{C}) {act} {training}", bn_formula(inp, torch.float64), bn_formula(inp, torch.float32), BNR_SPEC)
    for M, N, _ in COLSUM:
        A = rnd(M, N + 8, seed=60) + 0.5
        well_conditioned(f"colsum ({M},{N})", dict(plain=A[:, :N].double().sum(0)), dict(plain=A[:, :N].sum(0).double()), [("plain", "elem")])
    for M, K, wide in ROWDOT_CASES:
        inp = rowdot_inputs(M, K, wide)
        well_conditioned(f"rowdot ({M},{K})", rowdot_cpu(inp, torch.float64), rowdot_cpu(inp, torch.float32), ROWDOT_SPEC)


if __name__ == "__main__":          # the parts that need no GPU: the launch arithmetic against the library, and the conditioning guards
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for kind_, shape_, want_ in REACH:
        test_the_shape_reaches_the_code_it_is_listed_for(kind_, shape_, want_)
    test_the_restated_chan_grid_is_the_librarys()
    test_no_caller_reaches_the_vector_loop_of_the_256_lane_second_stage()
    for act_ in ("relu", "hswish"):
        test_the_bn_formula_is_fp64_autograd(act_)
    conditioning_guards()
    print("ok")
