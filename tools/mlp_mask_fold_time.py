"""The fused MLP backward kernels ALONE (one stream, nothing else on the GPU): the mask pass (mdvit_colsum_f32: gm = g * dropout mask * DropPath row scale) followed
by the kernel on gm, against the masked entry on g (csrc/mlp_rc.hip: mask on load):  python tools/mlp_mask_fold_time.py [--iters 20] [--warmup 5] [--rounds 3]
  C = 64   262144 tokens, hidden 512    mdvit_mlp_rc_dgrad (aux sweep), mdvit_mlp_rc_bwd (full sweep; its mask pass also takes db2, and stays as a read-only pass),
                                        mdvit_mlp_rc_wgrad
  C = 128   65536 tokens, hidden 1024   mdvit_mlp_rc16_dgrad without du (aux sweep: no gm_out) and with du (full sweep: with and without gm_out)
drop_p = 0.1 and a row scale per 4096 tokens, the headline step's shapes at 4 images per domain.  HIP events around `iters` launches after `warmup`; the calls go round four g
buffers so that no call finds its g in the last-level cache.  Every case runs in a process of its own under a time limit (--case runs one here); the first case
that fails or overruns ends the run."""
import argparse
import os
import subprocess
import sys

CASES = ("c64_dgrad", "c64_bwd", "c64_wgrad", "c128_dgrad", "c128_dgrad_du")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, iters, warmup):
    import torch
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


def run_case(name, iters, warmup, rounds):
    import torch
    sys.path.insert(0, ROOT)
    from mdvit_amd import _lib, ops
    from mdvit_amd._lib import call
    _p = ops._p
    dev = torch.device("cuda:0")
    C, M, Hd = (64, 262144, 512) if name.startswith("c64") else (128, 65536, 1024)
    gen = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev)

    def planes(W, transposed=0):
        N, K = W.shape
        out = torch.empty((2, K, N) if transposed else (2, N, K), device=dev, dtype=torch.bfloat16)
        call("mdvit_split_planes_t", _p(W), K, _p(out), N if transposed else K, N * K, N, K, transposed, 2, ops._stream())
        return out
    W1, b1, W2 = rnd(Hd, C, scale=C ** -0.5), rnd(Hd, scale=0.1), rnd(C, Hd, scale=Hd ** -0.5)
    W1p, W2tp, W1tp = planes(W1), planes(W2, 1), planes(W1, 1)
    x = rnd(M, C)
    gs = [rnd(M, C) for _ in range(4)]
    rps = 4096
    rs = ((torch.rand(M // rps, generator=gen) < 0.9).float() / 0.9).to(dev)
    gm, dx, db2 = torch.empty(M, C, device=dev), torch.empty(M, C, device=dev), torch.zeros(C, device=dev)
    st = ops._stream()
    p, k1, k2 = 0.1, (3, 4), (5, 6)
    mk = (p, k2[0], k2[1], None, _p(rs), rps)
    lib = _lib.load()

    def mask_pass(i, out=None, masked=True):
        wsb = lib.mdvit_partials_ws_bytes(C) if out is not None else 0
        call("mdvit_colsum_f32", _p(gs[i % 4]), C, _p(out), _p(gm) if masked else None, _p(pws) if out is not None else None, wsb, M, C, p, k2[0], k2[1], _p(rs), rps, 0,
             None, st)
    pws = torch.empty(lib.mdvit_partials_ws_bytes(C) // 4, device=dev)
    forms = {}
    if name == "c64_dgrad":
        def two(i):
            mask_pass(i)
            call("mdvit_mlp_rc_dgrad", _p(gm), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(W1tp), _p(dx), M, C, Hd, p, k1[0], k1[1], None, st)
        forms["mask pass + kernel"] = two
        forms["masked kernel"] = lambda i: call("mdvit_mlp_rc_dgrad_masked", _p(gs[i % 4]), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(W1tp), _p(dx), M, C, Hd, p, k1[0], k1[1], None,
                                                *mk, st)
    elif name in ("c64_bwd", "c64_wgrad"):
        wsb = lib.mdvit_mlp_rc_wgrad_ws_bytes(M, C, Hd)
        ws = torch.empty(wsb // 4, device=dev)
        parts = torch.empty(Hd // 256, M, C, device=dev)
        dW1, db1, dW2 = torch.empty(Hd, C, device=dev), torch.empty(Hd, device=dev), torch.empty(C, Hd, device=dev)
        if name == "c64_bwd":
            def kern(entry, g, *m):
                call(entry, _p(g), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(W1tp), _p(parts), _p(dW1), _p(db1), _p(dW2), _p(ws), wsb, M, C, Hd, p, k1[0], k1[1], None, *m, 0, st)
            e = "mdvit_mlp_rc_bwd"
        else:
            def kern(entry, g, *m):
                call(entry, _p(g), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(dW1), _p(db1), _p(dW2), _p(ws), wsb, M, C, Hd, p, k1[0], k1[1], None, *m, 0, st)
            e = "mdvit_mlp_rc_wgrad"

        def two(i):                     # the full sweep's pass: db2 and gm
            mask_pass(i, out=db2)
            kern(e, gm)

        def one(i):                     # the pass stays for db2, read-only
            mask_pass(i, out=db2, masked=False)
            kern(e + "_masked", gs[i % 4], *mk)
        forms["mask + db2 pass + kernel"] = two
        forms["db2 pass (read-only) + masked kernel"] = one
    else:
        du = torch.empty(M, Hd, device=dev) if name == "c128_dgrad_du" else None

        def two(i):
            mask_pass(i)
            call("mdvit_mlp_rc16_dgrad", _p(gm), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(W1tp), _p(du), _p(dx), M, C, Hd, p, k1[0], k1[1], None, st)

        def one(out):
            return lambda i: call("mdvit_mlp_rc16_dgrad_masked", _p(gs[i % 4]), _p(x), _p(W1p), _p(b1), _p(W2tp), _p(W1tp), _p(du), _p(dx), _p(out), M, C, Hd, p, k1[0],
                                  k1[1], None, *mk, st)
        forms["mask pass + kernel"] = two
        forms["masked kernel, no gm_out"] = one(None)
        if du is not None:
            forms["masked kernel, gm_out"] = one(gm)
    forms["mask pass alone"] = lambda i: mask_pass(i)
    print(f"{name}: {M} x {C}, hidden {Hd}, drop_p {p}, row scale per {rps} tokens  (library {_lib.LIB_PATH})", flush=True)
    us = {k: [] for k in forms}
    for r in range(rounds):
        for k, fn in forms.items():
            us[k].append(timed(fn, iters, warmup))
    for k, v in us.items():
        print(f"  {k:40s} " + " ".join(f"{t:8.1f}" for t in v) + f"   mean {sum(v) / len(v):8.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--case", choices=CASES, default=None)
    ap.add_argument("--limit", type=float, default=90.0, help="seconds per case")
    a = ap.parse_args()
    assert a.iters >= 20, "time at least 20 launches"
    if a.case:
        run_case(a.case, a.iters, a.warmup, a.rounds)
        return 0
    for c in CASES:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c, "--iters", str(a.iters), "--warmup", str(a.warmup), "--rounds", str(a.rounds)],
                                timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{c}: over its time limit of {a.limit:.0f} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{c}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
