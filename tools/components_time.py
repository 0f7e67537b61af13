"""mdvit_eval_components and mdvit_label_components alone at 16 x 512 x 512 and 16 x 256 x 256 in the three modes, one synthetic validation epoch (4 domains,
`--batches` batches of `--batch` x `--size` x `--size`) with and without `postprocess`, and the host way to the same figures:
python tools/components_time.py [--iters 3] [--warmup 1] [--batches 2] [--size 256] [--batch 16] [--kernel-iters 50]

  (a) mdvit_amd.evaluate(report=ImageReport(masks, aux masks))
  (b) the same with postprocess="fill_largest": cleaned masks, their Dice / IoU and the component columns in the epoch's single copy
  (c) the host way from (a)'s result, where scipy.ndimage can be imported: unpack the masks, then per image and output binary_fill_holes, label, bincount,
      and Dice / IoU of the cleaned mask

Epochs: host clock around work that ends in a device synchronise, mean of `iters` epochs after `warmup`.  The ops: HIP events over `kernel-iters` calls (host
enqueue included); their kernels one by one from torch.profiler's device times where that is available.  Report only: one box's numbers, no threshold."""
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
from mdvit_amd.evaluate import evaluate  # noqa: E402
from mdvit_amd.report import ImageReport, postprocess_mode, unpack_masks  # noqa: E402
from mdvit_amd.synthetic import make_domain_batch  # noqa: E402
from boundary_time import blobs  # noqa: E402
from report_time import timed_epoch, timed_kernel  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

D = 4
MODES = ("fill", "largest", "fill_largest")


def host_clean(m, mode):
    if mode != "largest":
        m = ndimage.binary_fill_holes(m)
    if mode != "fill":
        lab, k = ndimage.label(m)
        if k:
            m = lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
    return m


def host_way(res, labels, mode):
    """(c): cleaned masks, their counts and the raw component counts per image and output from the report's packed masks"""
    y = labels.reshape(labels.shape[0], *res["size"]) != 0
    counts = np.zeros((len(y), 5), dtype=np.int64)
    comps = np.zeros((len(y), 2), dtype=np.int64)
    counts[:, 2] = y.reshape(len(y), -1).sum(1)
    for o, key in enumerate(("masks", "aux_masks")):
        m = unpack_masks(res[key], res["size"]).astype(bool)
        for i in range(len(m)):
            comps[i, o] = ndimage.label(m[i])[1]
            c = host_clean(m[i], mode)
            counts[i, 3 * o], counts[i, 3 * o + 1] = (c & y[i]).sum(), c.sum()
    return counts, comps


def kernel_times(fn, iters):
    """{kernel name: us per launch, launches per call} of the ec_* kernels from torch.profiler, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "ec_" in e.key:
                total = getattr(e, "device_time_total", None)
                total = e.cuda_time_total if total is None else total
                out[re.search(r"ec_[a-z_]+", e.key).group(0)] = (total / max(e.count, 1), e.count / iters)
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
    a = ap.parse_args()
    assert a.kernel_iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}; scipy.ndimage {'available' if ndimage is not None else 'NOT available: no host figures'}")

    # the two entries alone
    g = torch.Generator().manual_seed(1)
    n = a.batch
    for S in (512, 256):
        label_logits = blobs(n, S, g)
        noise = lambda: 3.0 * torch.randn((n, 1, S, S), generator=g) * (torch.rand((n, 1, S, S), generator=g) < 0.03)          # salt and pepper
        out, aux = (label_logits + 0.5 * blobs(n, S, g) + noise()).to(dev), (label_logits + 1.0 * blobs(n, S, g) + noise()).to(dev)
        label = (label_logits > 0).float().to(dev)
        words = (S * S + 63) // 64
        counts, rows = torch.empty((n, 5), dtype=torch.int64, device=dev), torch.empty((n, 3, 4), dtype=torch.int64, device=dev)
        bits, aux_bits = torch.empty((n, words), dtype=torch.int64, device=dev), torch.empty((n, words), dtype=torch.int64, device=dev)
        ws = torch.empty((ops.eval_components_ws_bytes(n, S, S) // 8,), dtype=torch.int64, device=dev)
        px = n * S * S
        print(f"eval_components alone, {n} x {S}^2, {12 * px / 1e6:.2f} MB of logits and labels read, {ws.numel() * 8 / 1e6:.1f} MB of workspace")
        for mode in MODES:
            fn = lambda: ops.eval_components(out, aux, label, postprocess_mode(mode), counts, rows, ws, bits, aux_bits)
            t = timed_kernel(fn, a.kernel_iters, 5)
            t1 = timed_kernel(lambda: ops.eval_components(out, None, label, postprocess_mode(mode), counts, rows, ws, bits), a.kernel_iters, 5)
            fn()
            r = rows.cpu().numpy()
            # bytes through the label arrays (4 B labels + 4 B area words per pixel and plane): runs write both, flatten reads and writes the labels, the
            # fill and compose read them once more; the word planes are 1/32 of that
            planes = {"fill": (5, 0), "largest": (3, 0), "fill_largest": (5, 2)}[mode]
            moved = 12 * px + (planes[0] + planes[1]) * px * (8 + 8) + 2 * px * 4
            print(f"  {mode:13s} {t:9.1f} us with aux, {t1:9.1f} us without;  components per image (prediction) {r[:, 0, 0].mean():.0f}, filled {r[:, 0, 2].mean():.0f}, "
                  f"removed {r[:, 0, 3].mean():.0f};  ~{moved / 1e6:.0f} MB moved: {moved / t / 1e6:.3f} TB/s")
            per = kernel_times(fn, 20)
            if per:
                print("    per launch: " + ", ".join(f"{k} {v:.1f} us x{c:.0f}" for k, (v, c) in sorted(per.items())))
        masks = (out[:, 0] > 0)
        ws1 = torch.empty((ops.label_components_ws_bytes(n, S, S) // 8,), dtype=torch.int64, device=dev)
        comps = torch.empty((n,), dtype=torch.int64, device=dev)
        t = timed_kernel(lambda: ops.label_components(masks, comps, ws1), a.kernel_iters, 5)
        print(f"  label_components alone (bool masks in, int32 labels out, allocation of the labels included) {t:9.1f} us; {comps.float().mean().item():.0f} components per image")
        if ndimage is not None:
            m = masks.cpu().numpy()
            t0 = time.perf_counter()
            for i in range(n):
                ndimage.label(m[i])
            print(f"  scipy.ndimage.label of the same {n} masks on the host: {(time.perf_counter() - t0) * 1e3:9.1f} ms")

    # the epoch
    model = mdvit_amd.MDViT(img_size=a.size, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=D, decoder_name="MLPFM").to(dev).eval()
    loaders = {d: [make_domain_batch(a.batch, a.size, d, 100 + i, dev) for i in range(a.batches)] for d in range(D)}
    N = D * a.batches * a.batch
    plain = ImageReport(D, dev, masks=True, aux_masks=True, capacity=N)
    withp = ImageReport(D, dev, masks=True, aux_masks=True, capacity=N, postprocess="fill_largest")
    print(f"validation epoch: {D} domains x {a.batches} batches of {a.batch} x {a.size} x {a.size} = {N} images, MDViT (MLPFM)")
    for name, fn in (("(a) evaluate(report: masks + aux masks)", lambda: evaluate(model, loaders, num_domains=D, report=plain)),
                     ("(b) evaluate(report: masks + aux masks + postprocess=fill_largest)", lambda: evaluate(model, loaders, num_domains=D, report=withp))):
        mean, lo, hi = timed_epoch(fn, a.iters, a.warmup)
        print(f"  {name:78s} {mean:9.1f} ms per epoch  (min {lo:.1f}, max {hi:.1f}, {a.iters} epochs)")
    if ndimage is not None:
        res = evaluate(model, loaders, num_domains=D, fuse_domains=False, report=withp)["report"]          # loader after loader: the order of `labels`
        labels = torch.cat([b[1] for d in loaders for b in loaders[d]]).cpu().numpy()
        t0 = time.perf_counter()
        counts, comps = host_way(res, labels, "fill_largest")
        t_host = (time.perf_counter() - t0) * 1e3
        print(f"  {'(c) host way from the masks: unpack, scipy.ndimage fill + label per image':78s} {t_host:9.1f} ms on top of (a), {2 * N} (image, output) pairs")
        print(f"  report vs (c): pp_counts equal {np.array_equal(counts, res['pp_counts'])}, components equal {np.array_equal(comps, res['components'][:, :2])}; "
              f"mean Dice raw {res['dice'].mean():.4f} -> cleaned {res['pp_dice'].mean():.4f}")

    # the same comparison at the size the feature is for: 16 x 512 x 512 masks from the op's own tables
    if ndimage is not None:
        S = 512
        label_logits = blobs(n, S, g)
        out = (label_logits + 0.5 * blobs(n, S, g) + 3.0 * torch.randn((n, 1, S, S), generator=g) * (torch.rand((n, 1, S, S), generator=g) < 0.03)).to(dev)
        label = (label_logits > 0).float().to(dev)
        rep = ImageReport(D, dev, masks=True, capacity=n)
        rep.update(out, None, label, 0)
        res = rep.result()
        t0 = time.perf_counter()
        m = unpack_masks(res["masks"], res["size"]).astype(bool)
        y = label.cpu().numpy().reshape(n, S, S) != 0
        inter = [int((host_clean(m[i], "fill_largest") & y[i]).sum()) for i in range(n)]
        t_host = (time.perf_counter() - t0) * 1e3
        rp = ImageReport(D, dev, masks=True, capacity=n, postprocess="fill_largest")
        t_dev = timed_epoch(lambda: (rp.reset(), rp.update(out, None, label, 0), rp.result()), 5, 1)[0]
        print(f"{n} x 512 x 512, one output: host way (unpack + scipy fill + label + largest) {t_host:.1f} ms; report update + result with postprocess {t_dev:.2f} ms "
              f"(intersections equal: {inter == rp.result()['pp_counts'][:, 0].tolist()})")


if __name__ == "__main__":
    main()
