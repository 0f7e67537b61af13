"""One synthetic validation epoch (4 domains, bs = 16, 512 x 512, `--batches` batches each) timed three ways on the same tree, and the fused evaluation kernel
alone next to the two kernels it fuses:  python tools/eval_time.py [--iters 3] [--warmup 1] [--batches 2] [--size 512] [--batch 16] [--kernel-iters 50]

  (a) the reference's loop shape (multi_train_MDViT.py:246-313): per batch a forward, torch's BCE + Dice, two full-resolution `.cpu().numpy()` copies and
      Dice / IoU in numpy on the host (medpy's dc / jc restated)
  (b) per batch ops.seg_losses + ops.seg_metrics, the figures kept on the device, one sync at the end of the epoch
  (c) mdvit_amd.evaluate(), per domain and with equal-sized batches of different domains fused into one forward

Epochs: host clock around work that ends in a device synchronise (the loops hold host work), mean of `iters` epochs after `warmup`.  Kernels: HIP events over
`kernel-iters` launches; bytes = 12 per element (out, aux, label read once) over the time.  Report only: one box's numbers, no threshold."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdvit_amd  # noqa: E402
from mdvit_amd import ops  # noqa: E402
from mdvit_amd.evaluate import EvalAccumulator, evaluate  # noqa: E402
from mdvit_amd.synthetic import make_domain_batch  # noqa: E402

D = 4


def epoch_reference_shape(model, loaders):
    """(a): everything the reference's validate loop does per batch, its host copies and syncs included"""
    rows = []
    with torch.no_grad():
        for d, batches in loaders.items():
            sums, num = np.zeros(5), 0
            for img, label, set_id in batches:
                dl = F.one_hot(set_id, D).float().cuda()
                out, aux = model(img, dl, str(int(set_id[0])))
                o, a = torch.sigmoid(out), torch.sigmoid(aux)
                loss = F.binary_cross_entropy(o, label) + 1 - (2 * (o * label).sum() + 1e-5) / ((o * o).sum() + (label * label).sum() + 1e-5)
                n = img.shape[0]
                ob, ab, yb = o.cpu().numpy() > 0.5, a.cpu().numpy() > 0.5, label.cpu().numpy().astype(bool)
                y = np.count_nonzero(yb)
                for k, p in ((1, ob), (3, ab)):
                    i, s = np.count_nonzero(p & yb), np.count_nonzero(p)
                    sums[k] += (2.0 * i / (s + y) if s + y else 0.0) * n
                    sums[k + 1] += (i / (s + y - i) if s + y - i else 0.0) * n
                sums[0] += float(loss) * n
                num += n
            rows.append(sums / num)
    return rows


def epoch_two_ops(model, loaders):
    """(b): the two per-batch ops the package offered before evaluate(); the `* batch_len` bookkeeping on the device, one sync at the end"""
    tot = torch.zeros((D, 5), device="cuda")
    with torch.no_grad():
        for d, batches in loaders.items():
            for img, label, set_id in batches:
                dl = F.one_hot(set_id, D).float().cuda()
                out, aux = model(img, dl, str(int(set_id[0])))
                loss = ops.seg_losses(out, None, label)[0]
                metrics, _ = ops.seg_metrics(out, aux, label)
                tot[d] += torch.cat([loss.reshape(1), metrics]) * img.shape[0]
    return tot.cpu()


def timed_epoch(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sum(ts) / len(ts), min(ts), max(ts)


def timed_kernel(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel-iters", type=int, default=50)
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = mdvit_amd.MDViT(img_size=a.size, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=D, decoder_name="MLPFM").to(dev).eval()
    loaders = {d: [make_domain_batch(a.batch, a.size, d, 100 + i, dev) for i in range(a.batches)] for d in range(D)}
    print(f"validation epoch: {D} domains x {a.batches} batches of {a.batch} x {a.size} x {a.size}, MDViT (MLPFM), {torch.cuda.get_device_name(0)}")
    rows = [("(a) reference loop shape: .cpu().numpy() metrics per batch", lambda: epoch_reference_shape(model, loaders)),
            ("(b) ops.seg_losses + ops.seg_metrics per batch, one sync", lambda: epoch_two_ops(model, loaders)),
            ("(c) evaluate(fuse_domains=False)", lambda: evaluate(model, loaders, num_domains=D, fuse_domains=False)),
            ("(c) evaluate(fuse_domains=True)", lambda: evaluate(model, loaders, num_domains=D, fuse_domains=True))]
    for name, fn in rows:
        mean, lo, hi = timed_epoch(fn, a.iters, a.warmup)
        print(f"  {name:62s} {mean:9.1f} ms per epoch  (min {lo:.1f}, max {hi:.1f}, {a.iters} epochs)")
    res = evaluate(model, loaders, num_domains=D)
    ref = epoch_reference_shape(model, loaders)
    print("  evaluate() vs (a), per domain |loss|, |dice|, |iou| differences: "
          + ", ".join(f"{abs(res['loss'][d] - ref[d][0]):.1e}/{abs(res['dice'][d] - ref[d][1]):.1e}/{abs(res['iou'][d] - ref[d][2]):.1e}" for d in range(D)))

    # the kernels alone
    g = torch.Generator().manual_seed(1)
    for G in (1, 4):
        shape = (G * a.batch, 1, a.size, a.size)
        out, aux = (torch.randn(shape, generator=g) * 3).to(dev), (torch.randn(shape, generator=g) * 3).to(dev)
        label = (torch.rand(shape, generator=g) < 0.3).float().to(dev)
        n = out.numel()
        acc = EvalAccumulator(D, dev)
        doms = list(range(G))
        with torch.no_grad():
            fused = timed_kernel(lambda: acc.update(out, aux, label, doms if G > 1 else 0), a.kernel_iters, 5)
            if G == 1:
                pair = timed_kernel(lambda: (ops.seg_losses(out, None, label), ops.seg_metrics(out, aux, label)), a.kernel_iters, 5)
            else:
                B = a.batch
                pair = timed_kernel(lambda: [(ops.seg_losses(out[i * B:(i + 1) * B], None, label[i * B:(i + 1) * B]),
                                              ops.seg_metrics(out[i * B:(i + 1) * B], aux[i * B:(i + 1) * B], label[i * B:(i + 1) * B])) for i in range(G)],
                                    a.kernel_iters, 5)
        print(f"kernels alone, {G} x {a.batch} x {a.size}^2 = {n} elements ({12 * n / 1e6:.1f} MB read once):")
        print(f"  eval_accumulate (sums + final)              {fused:9.1f} us   {12 * n / fused / 1e6:6.3f} TB/s")
        print(f"  seg_losses + seg_metrics ({G} x 2 ops)         {pair:9.1f} us   ({20 * n / 1e6:.1f} MB read: out, label twice, aux once; {20 * n / pair / 1e6:6.3f} TB/s)")


if __name__ == "__main__":
    main()
