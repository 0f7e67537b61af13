"""The signed distance map and the boundary loss alone at 16 x 256 x 256 and 16 x 512 x 512 on labels that are discs, the host way to the same map, and the
bench-shaped MDViT train step (4 domains x `--batch` x `--size`, fused forward, merged sweeps, fused AdamW) with `boundary_weight` 0 and 0.01:
python tools/boundary_loss_time.py [--iters 10] [--warmup 5] [--size 512] [--batch 4] [--kernel-iters 50]

  (a) ops.signed_distance (mdvit_signed_distance: two launches, workspace and output allocation included), ops.boundary_loss forward and forward + backward
  (b) the host way (Utils/losses.py:120-160's round trip): label.cpu().numpy(), per image two scipy.ndimage.distance_transform_edt calls, .cuda() again --
      where scipy.ndimage can be imported
  (c) mdvit_train_step with boundary_weight 0 and 0.01

The ops: HIP events over `kernel-iters` calls (host enqueue included); their kernels one by one from torch.profiler's device times where that is available.  The
steps: host clock around steps that end in a device synchronise.  Report only: one box's numbers, no threshold."""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdvit_amd  # noqa: E402
from mdvit_amd import ops  # noqa: E402
from mdvit_amd.synthetic import make_step_batches  # noqa: E402
from report_time import timed_epoch, timed_kernel  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def discs(n, S, gen):
    """labels [n,1,S,S] fp32: one disc per image, radius 0.1 .. 0.3 of the side"""
    r = torch.rand((n, 3), generator=gen)
    yy, xx = torch.arange(S).view(1, S, 1).float(), torch.arange(S).view(1, 1, S).float()
    cy, cx, rad = (0.3 + 0.4 * r[:, 0]).view(n, 1, 1) * S, (0.3 + 0.4 * r[:, 1]).view(n, 1, 1) * S, (0.1 + 0.2 * r[:, 2]).view(n, 1, 1) * S
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= rad ** 2).float().view(n, 1, S, S)


def host_map(label):
    """one_hot2dist per image on the host, and back to the device"""
    m = label.cpu().numpy().reshape(label.shape[0], label.shape[-2], label.shape[-1]) != 0
    out = np.zeros(m.shape, dtype=np.float32)
    for i in range(len(m)):
        if m[i].any() and not m[i].all():
            out[i] = ndimage.distance_transform_edt(~m[i]) * ~m[i] - (ndimage.distance_transform_edt(m[i]) - 1) * m[i]
    return torch.from_numpy(out).view(label.shape).to(label.device)


def kernel_times(fn, iters):
    """{kernel name: (us per launch, launches per call)} of the sd_* kernels from torch.profiler, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "sd_" in e.key:
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                out[re.search(r"sd_[a-z_]+", e.key).group(0)] = (total / max(e.count, 1), e.count / iters)
        return out or None
    except Exception as exc:          # report only: the figures are optional
        print(f"  (per-kernel times unavailable: {type(exc).__name__}: {exc})")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=50)
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(0)}; scipy.ndimage {'available' if ndimage is not None else 'NOT available: no host figures'}")
    g = torch.Generator().manual_seed(1)
    n = 16
    for S in (256, 512):
        label = discs(n, S, g).to(dev)
        logits = (3.0 * torch.randn((n, 1, S, S), generator=g)).to(dev).requires_grad_(True)
        px = n * S * S
        print(f"{n} x {S}^2 discs, {label.mean().item() * 100:.1f} % foreground, {ops.signed_distance_ws_bytes(n, S, S) / 1e6:.1f} MB of workspace")
        t = timed_kernel(lambda: ops.signed_distance(label), a.kernel_iters, 5)
        t2 = timed_kernel(lambda: ops.signed_distance(label, return_squared=True), a.kernel_iters, 5)
        print(f"  (a) signed_distance {t:9.1f} us ({t2:.1f} us with d2);  label read + packed distances written and read + phi written = {16 * px / 1e6:.1f} MB: "
              f"{16 * px / t / 1e6:.3f} TB/s")
        phi = ops.signed_distance(label)
        tf = timed_kernel(lambda: ops.boundary_loss(logits.detach(), phi), a.kernel_iters, 5)
        tb = timed_kernel(lambda: ops.boundary_loss(logits, phi).backward(), a.kernel_iters, 5)
        print(f"      boundary_loss forward {tf:9.1f} us ({8 * px / tf / 1e6:.3f} TB/s), forward + backward through autograd {tb:9.1f} us")
        per = kernel_times(lambda: ops.boundary_loss(logits, ops.signed_distance(label)).backward(), 20)
        if per:
            print("      per launch: " + ", ".join(f"{k} {v:.1f} us x{c:.0f}" for k, (v, c) in sorted(per.items())))
        if ndimage is not None:
            host_map(label)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                hm = host_map(label)
            torch.cuda.synchronize()
            print(f"  (b) host way (.cpu(), 2 x distance_transform_edt per image, .cuda()) {(time.perf_counter() - t0) / 3 * 1e3:9.2f} ms;  "
                  f"max |host - device| {float((hm - phi).abs().max()):.2e}")

    # the bench-shaped step
    from mdvit_amd.optim import FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    from mdvit_amd.train import mdvit_train_step
    torch.manual_seed(0)
    ops.reserve_streams(side=True, sweep=True)
    model = mdvit_amd.MDViT(img_size=a.size, drop_rate=0.1, drop_path_rate=0.1, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=4, decoder_name="MLPFM").to(dev).train()
    ops.enable_side_stream(True)
    accum = GradAccumulator(model.parameters(), late=[p for nm, p in model.named_parameters() if "domain_layer" in nm])
    accum.attach_sinks()
    opt = FusedAdamW(accum, lr=1e-4, weight_decay=0.05)
    pool = [make_step_batches(a.batch, a.size, rank=0, step=i, device=dev) for i in range(2)]
    print(f"(c) mdvit_train_step, 4 domains x {a.batch} x {a.size}^2, MDViT (MLPFM), fused forward, merged sweeps, fused AdamW; mean (min, max) of {a.iters} steps after {a.warmup}")
    for rnd in range(2):          # twice, interleaved: the second round shows what the order of the two did
        for w in (0.0, 0.01):
            k = [0]

            def step():
                k[0] += 1
                return mdvit_train_step(model, pool[k[0] % 2], optimizer=opt, accumulator=accum, merged_sweeps=True, fuse_domains=4, boundary_weight=w)
            mean, lo, hi = timed_epoch(step, a.iters, a.warmup)
            print(f"  round {rnd} boundary_weight {w:<5} {mean:8.2f} ms per step  (min {lo:.2f}, max {hi:.2f})")
    res = mdvit_train_step(model, pool[0], optimizer=opt, accumulator=accum, merged_sweeps=True, fuse_domains=4, boundary_weight=0.01)
    print("  last step: " + ", ".join(f"{k_} {float(v):.4f}" for k_, v in res.items()))


if __name__ == "__main__":
    main()
