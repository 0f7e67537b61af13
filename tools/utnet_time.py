"""Time the low-rank attention (mdvit_lrattn_fwd: one launch; mdvit_lrattn_bwd: one launch + the dK / dV and the table-gradient second stages; C ABI, caller-owned
buffers) alone at the seven attention shapes of a UTNet step -- 16 images at 256 x 256, heads 4: down1..4 at 128^2 / 64^2 / 32^2 / 16^2 queries with dim_head
16 / 32 / 64 / 128, up1 / up2 / up3 at 32^2 / 64^2 / 128^2 with 64 / 32 / 16 -- beside the kernel's byte floor at a given HBM rate (forward: q, out, lse, k and v
once; backward: those plus the upstream gradient and dq), and one full UTNet train step (forward, BCE + Dice, backward).  Report only.

    python tools/utnet_time.py [--json out.json] [--batch 16] [--size 256]

Each figure is the median over `--rounds` rounds of the mean of `--iters` back-to-back calls between two events, after a warm-up.  The MI355X has a 256 MiB
Infinity Cache: every call takes the NEXT of `copies` input sets whose total is at least `--rotate-mib` (default 512 MiB), so that an input has been evicted
before it is read again; the outputs (out, lse, dq, dk, dv, dtable, the workspace) are one set of buffers: the write side may still hit the cache."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_TBS = 8.0          # MI355X peak HBM rate the floor is quoted at
HEADS = 4


def timed(fn, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)          # us
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mib", type=float, default=512.0)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import mdvit_amd
    from mdvit_amd import _lib, ops
    from mdvit_amd.losses import seg_loss
    from utnet_params import CTOR, make_utnet_params
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    S = a.size
    sites = [("down1", S // 2, 16), ("down2", S // 4, 32), ("down3", S // 8, 64), ("down4", S // 16, 128), ("up1", S // 8, 64), ("up2", S // 4, 32), ("up3", S // 2, 16)]
    B = a.batch
    for name, H, D in sites:
        Cn, N = HEADS * D, H * H
        q_bytes = 4.0 * B * N * Cn
        small = 4.0 * B * (HEADS * N + 2 * 64 * Cn)          # lse, k, v
        copies = max(2, int(-(-a.rotate_mib * 2 ** 20 // (2 * q_bytes))))
        qs = [torch.randn(B, N, Cn, device=dev) for _ in range(copies)]
        gs = [torch.randn(B, N, Cn, device=dev) for _ in range(copies)]
        k, v, table = torch.randn(B, 64, Cn, device=dev), torch.randn(B, 64, Cn, device=dev), torch.randn(225, HEADS, device=dev)
        out, lse = torch.empty(B, N, Cn, device=dev), torch.empty(B, HEADS, N, device=dev)
        dq, dk, dv, dtable = torch.empty_like(out), torch.empty_like(k), torch.empty_like(v), torch.empty_like(table)
        wsb = lib.mdvit_lrattn_bwd_ws_bytes(B, H, H, D, HEADS)
        ws = torch.empty(wsb // 4, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        geo = (B, H, H, D, HEADS, a.drop, 11, 22, None, st)
        turn = [0]

        def fwd():
            turn[0] = (turn[0] + 1) % copies
            _lib.check(lib.mdvit_lrattn_fwd(qs[turn[0]].data_ptr(), Cn, k.data_ptr(), v.data_ptr(), Cn, table.data_ptr(), out.data_ptr(), lse.data_ptr(), *geo), "lrattn_fwd")

        t_fwd = timed(fwd, a.iters, a.rounds, a.warmup)
        lses = []
        for q in qs:          # the backward reads the row log-sum-exp of ITS input
            lses.append(torch.empty_like(lse))
            _lib.check(lib.mdvit_lrattn_fwd(q.data_ptr(), Cn, k.data_ptr(), v.data_ptr(), Cn, table.data_ptr(), out.data_ptr(), lses[-1].data_ptr(), *geo), "lrattn_fwd")

        def bwd():
            turn[0] = (turn[0] + 1) % copies
            j = turn[0]
            _lib.check(lib.mdvit_lrattn_bwd(gs[j].data_ptr(), qs[j].data_ptr(), Cn, k.data_ptr(), v.data_ptr(), Cn, table.data_ptr(), lses[j].data_ptr(), dq.data_ptr(), Cn,
                                            dk.data_ptr(), dv.data_ptr(), Cn, dtable.data_ptr(), ws.data_ptr(), wsb, 0, *geo), "lrattn_bwd")

        t_bwd = timed(bwd, a.iters, a.rounds, a.warmup)
        row = {"site": name, "shape": [B, H, H, D], "q_mb": q_bytes / 1e6, "ws_mb": wsb / 1e6, "input_copies": copies, "fwd_us": t_fwd, "bwd_us": t_bwd,
               "fwd_floor_us": (2 * q_bytes + small) / (HBM_TBS * 1e6), "bwd_floor_us": (3 * q_bytes + small) / (HBM_TBS * 1e6)}
        rows.append(row)
        print(f"{name}: [{B}, {H}x{H}, {Cn}] dim_head {D}:  fwd {t_fwd:7.1f} us (floor {row['fwd_floor_us']:6.1f})   bwd {t_bwd:7.1f} us (floor {row['bwd_floor_us']:6.1f})   "
              f"workspace {wsb / 2 ** 20:.1f} MiB", flush=True)
        del qs, gs, lses
    m = mdvit_amd.UTNet(**CTOR)
    m.load_state_dict({kk: torch.from_numpy(np.asarray(vv)) for kk, vv in make_utnet_params(1).items()}, strict=False)
    m = m.to(dev).train()
    img = torch.randn(B, 3, S, S, device=dev)
    lab = (torch.rand(B, 1, S, S, device=dev) > 0.5).float()

    def step():
        m.zero_grad(set_to_none=True)
        seg_loss(m(img), lab).backward()

    t_step = timed(step, max(2, a.iters // 10), a.rounds, 3)
    print(f"UTNet train step (forward, BCE + Dice, backward), batch {B} at {S} x {S}, dropout 0.1, {ops.gemm_precision()}: {t_step / 1e3:.2f} ms", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"hbm_tbs": HBM_TBS, "iters": a.iters, "rounds": a.rounds, "rows": rows, "step_ms": t_step / 1e3, "batch": B, "size": S}, f, indent=1)


if __name__ == "__main__":
    main()
