"""The bilinear adjoints ALONE (one stream, nothing else on the GPU), one kernel against the two passes it replaces, in one process and in alternating rounds
(mdvit_upsample_bwd_config flips the path between them):  python tools/upsample_adjoint_time.py [--iters 20] [--warmup 5] [--rounds 3]
  peer heads  mdvit_upsample_multi_bwd  dy [4,128,128,512] -> dx 64^2 / 32^2 / 16^2     (MLPDecoderFM.forward's upsample_sum, 8 calls per bs=4 step)
  logits      mdvit_upsample_bwd        dy [4,512,512,1]   -> dx 128^2                  (the C = 1 resizes of model.py / decode.py)
Prints the time per call (HIP events over `iters` calls) and the achieved GB/s against the bytes the result needs: dy in and dx out (178 MB for the peer heads).
The calls of one measurement go round four dy buffers (537 MB for the peer heads), so that no call finds its dy in the last-level cache from the call before."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdvit_amd import _lib, ops  # noqa: E402
from mdvit_amd._lib import call  # noqa: E402

_p = ops._p


def timed(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3          # us per call


def multi_call(B, Ho, Wo, Cn, dims, dev):
    g = torch.Generator().manual_seed(0)
    dys = [torch.randn(B, Ho, Wo, Cn, generator=g).to(dev) for _ in range(4)]
    n = len(dims)
    dxs = [torch.empty(B, h, w, Cn, device=dev) for h, w in dims]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in dxs])
    Hi = (C.c_int32 * n)(*[h for h, _ in dims])
    Wi = (C.c_int32 * n)(*[w for _, w in dims])
    wsb = _lib.load().mdvit_upsample_multi_bwd_ws_bytes(Wi, n, B, Ho, Cn)
    ws = torch.empty(wsb // 4, device=dev)
    st = ops._stream()
    nbytes = 4 * (dys[0].numel() + sum(t.numel() for t in dxs))
    return (lambda i: call("mdvit_upsample_multi_bwd", _p(dys[i % 4]), ptrs, Hi, Wi, n, _p(ws), wsb, B, Ho, Wo, Cn, st)), nbytes, (dys, dxs, ws)


def single_call(B, Hi, Wi, Ho, Wo, Cn, dev):
    g = torch.Generator().manual_seed(1)
    dys = [torch.randn(B, Ho, Wo, Cn, generator=g).to(dev) for _ in range(4)]
    dx = torch.empty(B, Hi, Wi, Cn, device=dev)
    wsb = _lib.load().mdvit_upsample_bwd_ws_bytes(B, Hi, Wi, Ho, Wo, Cn)
    ws = torch.empty(wsb // 4, device=dev)
    st = ops._stream()
    nbytes = 4 * (dys[0].numel() + dx.numel())
    return (lambda i: call("mdvit_upsample_bwd", _p(dys[i % 4]), _p(dx), _p(ws), wsb, B, Hi, Wi, Ho, Wo, Cn, st)), nbytes, (dys, dx, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert a.iters >= 20, "time at least 20 calls"
    dev = torch.device("cuda:0")
    print(f"library: {_lib.LIB_PATH}", flush=True)
    cases = (("peer heads [4,128,128,512] -> 64^2 32^2 16^2", multi_call(4, 128, 128, 512, [(64, 64), (32, 32), (16, 16)], dev)),
             ("logits     [4,512,512,1]   -> 128^2", single_call(4, 128, 128, 512, 512, 1, dev)))
    try:
        for name, (fn, nbytes, keep) in cases:
            print(f"{name}: {nbytes / 1e6:.1f} MB of dy and dx")
            us = {0: [], 1: []}
            for rnd in range(a.rounds):
                for fused in (0, 1):
                    call("mdvit_upsample_bwd_config", fused)
                    us[fused].append(timed(fn, a.iters, a.warmup))
                print(f"  round {rnd}:  two passes {us[0][-1]:8.1f} us {nbytes / us[0][-1] / 1e3:8.1f} GB/s    one kernel {us[1][-1]:8.1f} us {nbytes / us[1][-1] / 1e3:8.1f} GB/s"
                      f"    ratio {us[0][-1] / us[1][-1]:.2f}", flush=True)
            m0, m1 = sum(us[0]) / a.rounds, sum(us[1]) / a.rounds
            print(f"  mean:     two passes {m0:8.1f} us    one kernel {m1:8.1f} us    ratio {m0 / m1:.2f}")
    finally:
        call("mdvit_upsample_bwd_config", 1)


if __name__ == "__main__":
    main()
