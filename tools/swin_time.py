"""Time the shifted-window attention (mdvit_winattn_fwd: one launch; mdvit_winattn_bwd: one launch + the table-gradient fold; C ABI,
caller-owned buffers) alone at the four stage shapes of a SwinUnet step -- 16 images at 256 x 256: [16, 64x64, 96] 3 heads, [16, 32x32, 192] 6 heads, [16, 16x16, 384] 12 heads, [16, 8x8, 768] 24 heads (shift 4,
0 in the last stage) -- beside the kernel's byte floor at a given HBM rate (forward: qkv read once, out written once; backward: qkv and the upstream gradient
read once, dqkv written once), and one full SwinUnet train step (forward, BCE + Dice, backward).  Report only.

    python tools/swin_time.py [--json out.json] [--batch 16] [--size 256]

Each figure is the median over `--rounds` rounds of the mean of `--iters` back-to-back calls between two events, after a warm-up.  The inputs of a stage are
2 - 75 MB and the MI355X has a 256 MiB Infinity Cache: every call takes the NEXT of `copies` input sets whose total is at least `--rotate-mib` (default 512
MiB), so that an input has been evicted before it is read again; the outputs (out, lse, dqkv, dtable, the workspace) are one set of buffers: the write side may still hit the cache."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_TBS = 8.0          # MI355X peak HBM rate the floor is quoted at


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate-mib", type=float, default=512.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import mdvit_amd
    from mdvit_amd import _lib, ops
    from mdvit_amd.losses import seg_loss
    from swin_params import make_swin_params
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for i, heads in enumerate((3, 6, 12, 24)):
        H = a.size // 4 // 2 ** i
        Cn, shift = heads * 32, (4 if H > 8 else 0)
        out_bytes = 4.0 * a.batch * H * H * Cn
        copies = max(2, int(-(-a.rotate_mib * 2 ** 20 // (4 * out_bytes))))
        qs = [torch.randn(a.batch, H * H, 3 * Cn, device=dev) for _ in range(copies)]
        gs = [torch.randn(a.batch, H * H, Cn, device=dev) for _ in range(copies)]
        table = torch.randn(225, heads, device=dev)
        # the C ABI on caller-owned buffers: through ops the two small stages would time the host (an autograd call and three allocations per launch pair)
        out, lse = torch.empty(a.batch, H * H, Cn, device=dev), torch.empty(a.batch, heads, H * H, device=dev)
        dqkv, dtable = torch.empty_like(qs[0]), torch.empty_like(table)
        wsb = lib.mdvit_winattn_bwd_ws_bytes(a.batch, H, H, heads)
        ws = torch.empty(wsb // 4, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        turn = [0]

        def fwd():
            turn[0] = (turn[0] + 1) % copies
            _lib.check(lib.mdvit_winattn_fwd(qs[turn[0]].data_ptr(), table.data_ptr(), out.data_ptr(), lse.data_ptr(), a.batch, H, H, Cn, heads, shift, st), "winattn_fwd")

        t_fwd = timed(fwd, a.iters, a.rounds, a.warmup)
        lses = []
        for q in qs:          # the backward reads the row log-sum-exp of ITS input
            lses.append(torch.empty_like(lse))
            _lib.check(lib.mdvit_winattn_fwd(q.data_ptr(), table.data_ptr(), out.data_ptr(), lses[-1].data_ptr(), a.batch, H, H, Cn, heads, shift, st), "winattn_fwd")

        def bwd():
            turn[0] = (turn[0] + 1) % copies
            j = turn[0]
            _lib.check(lib.mdvit_winattn_bwd(gs[j].data_ptr(), qs[j].data_ptr(), table.data_ptr(), lses[j].data_ptr(), dqkv.data_ptr(), dtable.data_ptr(), ws.data_ptr(), wsb, 0,
                                             a.batch, H, H, Cn, heads, shift, st), "winattn_bwd")

        t_bwd = timed(bwd, a.iters, a.rounds, a.warmup)
        row = {"shape": [a.batch, H, H, heads, shift], "qkv_mb": 3 * out_bytes / 1e6, "input_copies": copies, "fwd_us": t_fwd, "bwd_us": t_bwd,
               "fwd_floor_us": 4 * out_bytes / (HBM_TBS * 1e6), "bwd_floor_us": 7 * out_bytes / (HBM_TBS * 1e6)}
        rows.append(row)
        print(f"[{a.batch}, {H}x{H}, {Cn}] heads {heads} shift {shift}:  fwd {t_fwd:7.1f} us (floor {row['fwd_floor_us']:6.1f})   "
              f"bwd {t_bwd:7.1f} us (floor {row['bwd_floor_us']:6.1f})", flush=True)
    m = mdvit_amd.SwinUnet(img_size=a.size, window_size=8)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_swin_params(1).items()}, strict=False)
    m = m.to(dev).train()
    img = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    lab = (torch.rand(a.batch, 1, a.size, a.size, device=dev) > 0.5).float()

    def step():
        m.zero_grad(set_to_none=True)
        seg_loss(m(img), lab).backward()

    t_step = timed(step, max(2, a.iters // 10), a.rounds, 3)
    print(f"SwinUnet train step (forward, BCE + Dice, backward), batch {a.batch} at {a.size} x {a.size}, {ops.gemm_precision()}: {t_step / 1e3:.2f} ms", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"hbm_tbs": HBM_TBS, "iters": a.iters, "rounds": a.rounds, "rows": rows, "step_ms": t_step / 1e3, "batch": a.batch, "size": a.size}, f, indent=1)


if __name__ == "__main__":
    main()
