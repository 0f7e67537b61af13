"""One synthetic validation epoch (4 domains, bs = 16, 256 x 256, `--batches` batches each) timed three ways on the same tree, and the two report kernels alone
beside the bytes they must move:  python tools/report_time.py [--iters 3] [--warmup 1] [--batches 2] [--size 256] [--batch 16] [--kernel-iters 50]

  (a) mdvit_amd.evaluate() alone
  (b) mdvit_amd.evaluate(report=ImageReport(masks, aux masks, structure)): per-image counts, packed masks and the structure term, one copy at the end
  (c) the host way to the same per-image figures: evaluate()'s loop with a `.cpu()` of every batch's logits, Dice per image in numpy (Utils/pieces.py:103-121)
      and structure_loss image by image in torch on the device (multi_train_TransFuse.py:29-38, restated below), its column copied per batch

Epochs: host clock around work that ends in a device synchronise, mean of `iters` epochs after `warmup`.  Kernels: HIP events over `kernel-iters` launches.
Report only: one box's numbers, no threshold."""
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
from mdvit_amd.evaluate import evaluate  # noqa: E402
from mdvit_amd.report import ImageReport, unpack_masks  # noqa: E402
from mdvit_amd.synthetic import make_domain_batch  # noqa: E402

D = 4


def structure_terms(pred, mask):
    """structure_loss before its mean over the batch: wbce + wiou per image, [B]"""
    weit = 1 + 5 * torch.abs(F.avg_pool2d(mask, kernel_size=31, stride=1, padding=15) - mask)
    wbce = F.binary_cross_entropy_with_logits(pred, mask, reduction="none")
    wbce = (weit * wbce).sum(dim=(2, 3)) / weit.sum(dim=(2, 3))
    p = torch.sigmoid(pred)
    inter, union = (p * mask * weit).sum(dim=(2, 3)), ((p + mask) * weit).sum(dim=(2, 3))
    return (wbce + 1 - (inter + 1) / (union - inter + 1)).reshape(-1)


def epoch_host_way(model, loaders):
    """(c): the per-image figures without the report -- every batch's logits cross to the host"""
    dice, structure, masks = [], [], []
    with torch.no_grad():
        for d, batches in loaders.items():
            for img, label, set_id in batches:
                dl = F.one_hot(set_id, D).float().cuda()
                out, aux = model(img, dl, str(int(set_id[0])))
                structure.append(structure_terms(out, label).cpu().numpy())
                for logits in (out, aux):
                    a = (torch.sigmoid(logits).cpu().numpy() > 0.5).reshape(img.shape[0], -1)
                    masks.append(a)
                y = label.cpu().numpy().reshape(img.shape[0], -1) != 0
                a = masks[-2]
                den = a.sum(1) + y.sum(1)
                dice.append(np.where(den > 0, 2.0 * (a & y).sum(1) / np.maximum(den, 1), 0.0))
    return np.concatenate(dice), np.concatenate(structure)


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
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel-iters", type=int, default=50)
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = mdvit_amd.MDViT(img_size=a.size, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=D, decoder_name="MLPFM").to(dev).eval()
    loaders = {d: [make_domain_batch(a.batch, a.size, d, 100 + i, dev) for i in range(a.batches)] for d in range(D)}
    N = D * a.batches * a.batch
    report = ImageReport(D, dev, masks=True, aux_masks=True, structure=True, capacity=N)
    print(f"validation epoch: {D} domains x {a.batches} batches of {a.batch} x {a.size} x {a.size} = {N} images, MDViT (MLPFM), {torch.cuda.get_device_name(0)}")
    rows = [("(a) evaluate()", lambda: evaluate(model, loaders, num_domains=D)),
            ("(b) evaluate(report: masks + aux masks + structure)", lambda: evaluate(model, loaders, num_domains=D, report=report)),
            ("(a) evaluate(fuse_domains=False)", lambda: evaluate(model, loaders, num_domains=D, fuse_domains=False)),
            ("(b) evaluate(fuse_domains=False, report: ...)", lambda: evaluate(model, loaders, num_domains=D, fuse_domains=False, report=report)),
            ("(c) host way: .cpu() logits per batch, numpy Dice, torch structure", lambda: epoch_host_way(model, loaders))]
    for name, fn in rows:
        mean, lo, hi = timed_epoch(fn, a.iters, a.warmup)
        print(f"  {name:70s} {mean:9.1f} ms per epoch  (min {lo:.1f}, max {hi:.1f}, {a.iters} epochs)")
    res = evaluate(model, loaders, num_domains=D, fuse_domains=False, report=report)["report"]
    dice, structure = epoch_host_way(model, loaders)
    m = unpack_masks(res["masks"], res["size"])
    print(f"  report vs (c): max |dice| difference {np.abs(res['dice'] - dice).max():.1e}, max relative structure difference "
          f"{(np.abs(res['structure'] - structure) / np.abs(structure)).max():.1e}; {m.shape[0]} masks of {m.shape[1]} x {m.shape[2]}, "
          f"{res['masks'].nbytes + res['aux_masks'].nbytes + res['counts'].nbytes + res['structure'].nbytes} bytes in the epoch's copy "
          f"({2 * 4 * N * a.size * a.size} bytes of logits cross in (c))")

    # the kernels alone
    g = torch.Generator().manual_seed(1)
    for n in (1, a.batch, 4 * a.batch):
        shape = (n, 1, a.size, a.size)
        out, aux = (torch.randn(shape, generator=g) * 3).to(dev), (torch.randn(shape, generator=g) * 3).to(dev)
        label = (torch.rand(shape, generator=g) < 0.3).float().to(dev)
        HW = a.size * a.size
        words = (HW + 63) // 64
        counts = torch.empty((n, 5), dtype=torch.int64, device=dev)
        bits, aux_bits = torch.empty((n, words), dtype=torch.int64, device=dev), torch.empty((n, words), dtype=torch.int64, device=dev)
        loss = torch.empty((n,), dtype=torch.float64, device=dev)
        ws_i = torch.empty((ops.eval_images_ws_bytes(n, HW) // 4,), dtype=torch.int32, device=dev)
        ws_s = torch.empty((ops.eval_structure_ws_bytes(n, a.size, a.size) // 8,), dtype=torch.float64, device=dev)
        t_i = timed_kernel(lambda: ops.eval_images(out, aux, label, counts, ws_i, bits, aux_bits), a.kernel_iters, 5)
        t_c = timed_kernel(lambda: ops.eval_images(out, aux, label, counts, ws_i), a.kernel_iters, 5)
        t_s = timed_kernel(lambda: ops.eval_structure(out, label, loss, ws_s), a.kernel_iters, 5)
        b_i, b_s = 12 * n * HW + 16 * n * words, 8 * n * HW
        print(f"kernels alone, {n} x {a.size}^2:")
        print(f"  eval_images (counts + masks + aux masks, words + fold)   {t_i:9.1f} us   {b_i / 1e6:8.2f} MB (out, aux, label read once; bits written)  {b_i / t_i / 1e6:6.3f} TB/s")
        print(f"  eval_images (counts only)                                {t_c:9.1f} us   {12 * n * HW / 1e6:8.2f} MB                                     {12 * n * HW / t_c / 1e6:6.3f} TB/s")
        print(f"  eval_structure (tiles + fold)                            {t_s:9.1f} us   {b_s / 1e6:8.2f} MB (pred, label read once, halo not counted) {b_s / t_s / 1e6:6.3f} TB/s")


if __name__ == "__main__":
    main()
