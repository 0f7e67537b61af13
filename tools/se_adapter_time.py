"""Time the squeeze-excite adapter (ops.se_adapter: forward launches, backward launches) at the stage shapes of the bench step -- 16 images at 512 x 512:
[16, 16384, 64], [16, 4096, 128], [16, 1024, 320], [16, 256, 512] -- against

  * its algorithmic byte floor at a given HBM rate: the forward reads x twice and writes y once (3 passes over [B, N, C] fp32), the backward reads g and x,
    then g again, and writes dx (4 passes); the O(B C r) gate traffic is left out of the floor;
  * the same math composed from torch ops on the same GPU (mean / matmul / relu / softmax / sigmoid / broadcast multiply and autograd's backward).

    python tools/se_adapter_time.py [--json out.json] [--batch 16] [--size 512]

Each figure is the median over `--rounds` rounds of the mean of `--iters` back-to-back calls between two events, after a warm-up.  One tensor is 8 - 67 MB and the
MI355X has a 256 MiB Infinity Cache, so calls on one set of buffers would be served from it: every call takes the NEXT of `copies` (x, g) input pairs whose total
is at least `--rotate-mib` (default 512 MiB, twice the cache), so that an input has been evicted before it is read again.  The outputs (y, dx) are fresh
allocations that the caching allocator hands back at the same addresses: the write side may still hit the cache."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS = 8.0          # MI355X peak HBM rate the floor is quoted at


def torch_adapter(x, kind, P):
    p = x.mean(1)
    se = lambda W1, b1, W2, b2: torch.relu(p @ W1.t() + b1) @ W2.t() + b2
    if kind == "dase":
        w = torch.softmax(p @ P[0].t() + P[1], dim=1)
        z = torch.stack([se(*P[2 + 4 * k:6 + 4 * k]) for k in range(4)], dim=2)
        return x * torch.sigmoid(torch.matmul(z, w.unsqueeze(2)).squeeze(2)).unsqueeze(1)
    return torch.sigmoid(se(*P)).unsqueeze(1) * x + x


def params(kind, Cn, dev):
    r = Cn // 16 if kind == "dase" else Cn // 8
    g = torch.Generator().manual_seed(Cn)
    rn = lambda *s: torch.randn(*s, generator=g)
    branch = lambda: [rn(r, Cn) / Cn ** 0.5, 0.1 * rn(r), rn(Cn, r) / r ** 0.5, 0.1 * rn(Cn)]
    P = ([rn(4, Cn) / Cn ** 0.5, 0.1 * rn(4)] + [t for _ in range(4) for t in branch()]) if kind == "dase" else branch()
    return [t.to(dev).requires_grad_(True) for t in P]


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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rotate-mib", type=float, default=512.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from mdvit_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for kind in ("dase", "use"):
        for i, Cn in enumerate((64, 128, 320, 512)):
            N = (a.size // 2 ** (i + 2)) ** 2
            nbytes = 4.0 * a.batch * N * Cn
            copies = max(2, int(-(-a.rotate_mib * 2 ** 20 // (2 * nbytes))))
            xs = [torch.randn(a.batch, N, Cn, device=dev).requires_grad_(True) for _ in range(copies)]
            gys = [torch.randn(a.batch, N, Cn, device=dev) for _ in range(copies)]
            P = params(kind, Cn, dev)
            res = {}
            for name, f in (("hip", lambda x: ops.se_adapter(x, kind, P)), ("torch", lambda x: torch_adapter(x, kind, P))):
                turn = [0]

                def fwd():
                    turn[0] = (turn[0] + 1) % copies
                    return f(xs[turn[0]])

                res[name + "_fwd_us"] = timed(fwd, a.iters, a.rounds, a.warmup)
                ys = [f(x) for x in xs]

                def bwd():
                    turn[0] = (turn[0] + 1) % copies
                    i = turn[0]
                    return torch.autograd.grad(ys[i], [xs[i]] + P, gys[i], retain_graph=True)

                res[name + "_bwd_us"] = timed(bwd, a.iters, a.rounds, a.warmup)
                del ys
            row = {"kind": kind, "shape": [a.batch, N, Cn], "tensor_mb": nbytes / 1e6, "input_copies": copies,
                   "fwd_floor_us": 3 * nbytes / (HBM_TBS * 1e6), "bwd_floor_us": 4 * nbytes / (HBM_TBS * 1e6), **res}
            rows.append(row)
            print(f"{kind:4s} [{a.batch},{N},{Cn}]  fwd {row['hip_fwd_us']:7.1f} us (floor {row['fwd_floor_us']:6.1f}, torch {row['torch_fwd_us']:7.1f})   "
                  f"bwd {row['hip_bwd_us']:7.1f} us (floor {row['bwd_floor_us']:6.1f}, torch {row['torch_bwd_us']:7.1f})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"hbm_tbs": HBM_TBS, "iters": a.iters, "rounds": a.rounds, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
