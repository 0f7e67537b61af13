"""One synthetic test epoch (4 domains, `--batches` batches of `--batch` x `--size` x `--size`) with and without the boundary columns of the per-image report,
the host way to the same figures, and mdvit_eval_boundary's kernels alone:  python tools/boundary_time.py [--iters 3] [--warmup 1] [--batches 2] [--size 256]
[--batch 16] [--kernel-iters 50] [--kernel-size 512]

  (a) mdvit_amd.evaluate(report=ImageReport(masks, aux masks))
  (b) the same with boundary=True: hd95 / hd / assd per image in the epoch's single copy
  (c) the host way from (a)'s result: unpack the masks, then per image and output two Euclidean distance transforms (scipy.ndimage where it can be
      imported, else the brute-force numpy restatement) and numpy.percentile

Epochs: host clock around work that ends in a device synchronise, mean of `iters` epochs after `warmup`.  The op: HIP events over `kernel-iters` calls (five
launches each, host enqueue included); its kernels one by one from torch.profiler's device times where that is available.  Report only: one box's numbers, no
threshold."""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdvit_amd  # noqa: E402
from mdvit_amd import ops  # noqa: E402
from mdvit_amd.evaluate import evaluate  # noqa: E402
from mdvit_amd.report import ImageReport, boundary_from_rows, unpack_masks  # noqa: E402
from mdvit_amd.synthetic import make_domain_batch  # noqa: E402
from report_time import timed_epoch, timed_kernel  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

D = 4


def border(m):
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def surface_distances(a, y):
    """medpy's __surface_distances (voxelspacing None, connectivity 1) for bool [H,W] masks"""
    if ndimage is not None:
        s = ndimage.generate_binary_structure(2, 1)
        ba, by = a ^ ndimage.binary_erosion(a, structure=s, iterations=1), y ^ ndimage.binary_erosion(y, structure=s, iterations=1)
        return ndimage.distance_transform_edt(~by)[ba]
    ba, by = border(a), border(y)
    sy, sx = np.nonzero(ba)
    ty, tx = np.nonzero(by)
    out = np.empty(len(sy))
    step = max(1, (1 << 22) // max(len(ty), 1))
    for i in range(0, len(sy), step):
        out[i:i + step] = np.sqrt(((sy[i:i + step, None] - ty[None]) ** 2 + (sx[i:i + step, None] - tx[None]) ** 2).min(1))
    return out


def host_way(res, labels):
    """(c): hd95 and assd per image and output from the report's packed masks; NaN where a mask is empty"""
    y = labels.reshape(labels.shape[0], *res["size"]) != 0
    cols = {}
    for pre, key in (("", "masks"), ("aux_", "aux_masks")):
        m = unpack_masks(res[key], res["size"]).astype(bool)
        hd95, assd = np.full(len(m), np.nan), np.full(len(m), np.nan)
        for i in range(len(m)):
            if m[i].any() and y[i].any():
                s1, s2 = surface_distances(m[i], y[i]), surface_distances(y[i], m[i])
                hd95[i], assd[i] = np.percentile(np.hstack((s1, s2)), 95), (s1.mean() + s2.mean()) / 2.0
        cols[pre + "hd95"], cols[pre + "assd"] = hd95, assd
    return cols


def blobs(n, size, gen, shift=0.0):
    """smooth random logits [n,1,size,size]: a few blobs per image, a border of a few thousand pixels at 512 x 512"""
    low = torch.randn((n, 1, max(size // 64, 2), max(size // 64, 2)), generator=gen)
    return F.interpolate(low, size=(size, size), mode="bicubic", align_corners=False) * 4 + shift


def kernel_times(fn, iters):
    """{kernel name: us per launch} of the eb_* kernels from torch.profiler, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "eb_" in e.key:
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                out[re.search(r"eb_[a-z_]+", e.key).group(0) + ("<aux>" if "<true>" in e.key else "")] = total / max(e.count, 1)
        return out or None
    except Exception as exc:          # report only: the figures are optional
        print(f"  (per-kernel times unavailable: {type(exc).__name__}: {exc})")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--kernel-size", type=int, default=512)
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = mdvit_amd.MDViT(img_size=a.size, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=D, decoder_name="MLPFM").to(dev).eval()
    loaders = {d: [make_domain_batch(a.batch, a.size, d, 100 + i, dev) for i in range(a.batches)] for d in range(D)}
    N = D * a.batches * a.batch
    plain = ImageReport(D, dev, masks=True, aux_masks=True, capacity=N)
    withb = ImageReport(D, dev, masks=True, aux_masks=True, boundary=True, capacity=N)
    print(f"test epoch: {D} domains x {a.batches} batches of {a.batch} x {a.size} x {a.size} = {N} images, MDViT (MLPFM), {torch.cuda.get_device_name(0)}")
    for name, fn in (("(a) evaluate(report: masks + aux masks)", lambda: evaluate(model, loaders, num_domains=D, report=plain)),
                     ("(b) evaluate(report: masks + aux masks + boundary)", lambda: evaluate(model, loaders, num_domains=D, report=withb))):
        mean, lo, hi = timed_epoch(fn, a.iters, a.warmup)
        print(f"  {name:70s} {mean:9.1f} ms per epoch  (min {lo:.1f}, max {hi:.1f}, {a.iters} epochs)")
    res = evaluate(model, loaders, num_domains=D, fuse_domains=False, report=withb)["report"]          # loader after loader: the order of `labels`
    labels = torch.cat([b[1] for d in loaders for b in loaders[d]]).cpu().numpy()
    assert np.array_equal((labels.reshape(N, -1) != 0).sum(1), res["counts"][:, 2])
    t0 = time.perf_counter()
    host = host_way(res, labels)
    t_host = (time.perf_counter() - t0) * 1e3
    how = "scipy.ndimage" if ndimage is not None else "numpy brute force"
    print(f"  {'(c) host way from the masks: unpack, ' + how + ', numpy.percentile':70s} {t_host:9.1f} ms on top of (a), {2 * N} (image, output) pairs")
    for k in ("hd95", "assd", "aux_hd95", "aux_assd"):
        ok = ~np.isnan(host[k])
        assert np.array_equal(ok, ~np.isnan(res[k]))
        err = (np.abs(res[k][ok] - host[k][ok]) / np.maximum(np.abs(host[k][ok]), 1e-300)).max() if ok.any() else 0.0
        print(f"  report vs (c) {k:9s}: {int(ok.sum())} valid images, max relative difference {err:.1e}, mean {np.nanmean(res[k]) if ok.any() else float('nan'):.3f} px")
    nb = res["boundary_rows"].nbytes + 8 * 4 * N
    print(f"  border pixels per image (prediction, label): mean {res['boundary_rows'][:, 0, 0].mean():.0f}, {res['boundary_rows'][:, 0, 1].mean():.0f}; "
          f"{nb} bytes of boundary tables in the epoch's copy")

    # the op and its kernels alone
    g = torch.Generator().manual_seed(1)
    S = a.kernel_size
    for n in (1, a.batch, 4 * a.batch):
        label_logits = blobs(n, S, g)
        out, aux = (label_logits + 0.5 * blobs(n, S, g)).to(dev), (label_logits + 1.0 * blobs(n, S, g)).to(dev)
        label = (label_logits > 0).float().to(dev)
        rows, sums = torch.empty((n, 2, 6), dtype=torch.int64, device=dev), torch.empty((n, 2, 2), dtype=torch.float64, device=dev)
        ws = torch.empty((ops.eval_boundary_ws_bytes(n, S, S) // 8,), dtype=torch.int64, device=dev)
        fn = lambda: ops.eval_boundary(out, aux, label, rows, sums, ws)
        t = timed_kernel(fn, a.kernel_iters, 5)
        t1 = timed_kernel(lambda: ops.eval_boundary(out, None, label, rows, sums, ws), a.kernel_iters, 5)
        fn()
        b = boundary_from_rows(rows.cpu().numpy(), sums.cpu().numpy(), [0] * n)
        r = rows.cpu().numpy()
        print(f"eval_boundary alone, {n} x {S}^2 (border pixels per image: prediction {r[:, 0, 0].mean():.0f}, label {r[:, 0, 1].mean():.0f}; "
              f"mean hd95 {np.nanmean(b['hd95']):.2f} px): {t:9.1f} us with aux, {t1:9.1f} us without; {12 * n * S * S / 1e6:.2f} MB of logits and labels read, "
              f"{ws.numel() * 8 / 1e6:.2f} MB of workspace")
        per = kernel_times(fn, 20)
        if per:
            print("  per launch: " + ", ".join(f"{k} {v:.1f} us" for k, v in sorted(per.items())))


if __name__ == "__main__":
    main()
