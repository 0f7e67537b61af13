"""One snapshot of MDViT (MLPFM)'s state_dict timed two ways on the same tree, and the pack kernel alone:  python tools/snapshot_time.py [--iters 10] [--warmup 2]
[--size 512] [--kernel-iters 50]

  (a) what `torch.save(model.state_dict(), path)` does before it writes: one device-to-host copy and one synchronisation per tensor,
      {k: v.cpu() for k, v in model.state_dict().items()}
  (b) DeviceSnapshot.take() + wait(): one pack launch, one copy into pinned memory; take() alone is what the train loop waits for

Host clock around each, the device idle before (a synchronise) -- mean, min and max of `iters` after `warmup`.  The kernel: HIP events over `kernel-iters`
launches; bytes = 2 per byte packed (read once, written once) over the time.  Report only: one box's numbers, no threshold."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdvit_amd  # noqa: E402
from mdvit_amd import ops  # noqa: E402
from mdvit_amd._lib import call  # noqa: E402
from mdvit_amd.snapshot import DeviceSnapshot  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sum(ts) / len(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--kernel-iters", type=int, default=50)
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = mdvit_amd.MDViT(img_size=a.size, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=4, decoder_name="MLPFM").to(dev)
    sd = model.state_dict()
    snap = DeviceSnapshot(dict(sd))
    print(f"MDViT (MLPFM) state_dict: {len(sd)} tensors, {len(snap._tensors)} distinct, {snap.nbytes / 1e6:.1f} MB packed, {snap.n_rows} table rows, "
          f"{torch.cuda.get_device_name(0)}")

    def per_tensor():
        return {k: v.cpu() for k, v in model.state_dict().items()}

    def take_only():
        snap.take()

    def take_wait():
        snap.take()
        snap.wait()

    for name, fn in (("(a) {k: v.cpu()} per tensor", per_tensor), ("(b) take() alone (the copy still in flight)", take_only), ("(b) take() + wait()", take_wait)):
        mean, lo, hi = timed(fn, a.iters, a.warmup)
        print(f"  {name:48s} {mean:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {a.iters} runs)")
    snap.wait()
    got, want = snap.state_dict(), per_tensor()
    assert all(torch.equal(got[k], want[k]) for k in want), "the two snapshots differ"

    def pack():
        call("mdvit_table_pack", snap.table.data_ptr(), snap.n_rows, snap.staging.data_ptr(), snap.blocks, ops._stream())

    for _ in range(5):
        pack()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.kernel_iters):
        pack()
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / a.kernel_iters * 1e3
    print(f"  mdvit_table_pack alone: {snap.nbytes / 1e6:.1f} MB packed ({2 * snap.nbytes / 1e6:.1f} MB moved)  {us:9.1f} us   {2 * snap.nbytes / us / 1e6:6.3f} TB/s")


if __name__ == "__main__":
    main()
