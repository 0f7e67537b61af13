"""The device-resident loader next to the step it feeds (report only, nothing passes or fails):  python tools/dataset_time.py [--iters 50] [--warmup 10] [--steps 20]
  (1) DeviceDataset.batch() -- index upload + ops.gather_resize_u8 -- and batch() + TrainAug at B = 16, 512 x 512 -> 256 x 256, as GPU-event time per call over
      `iters` calls, beside the bytes moved: 16 x 4 source bytes read per output pixel at 2 : 1 (every source pixel is a tap once) and 4 written by the
      gather, then 4 read and 16 written by the augmentation;
  (2) one MDViT train step at 256 x 256, four domains of `--batch` images, fed from DomainBatches (pools of `--samples` 512 x 512 samples per domain):
      host clock around `steps` steps that end in a synchronise, with the batches drawn inside the window and with the same step on batches drawn before it,
      and the GPU-event time of drawing one step's four batches alone."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdvit_amd  # noqa: E402
from mdvit_amd.augment import TrainAug  # noqa: E402
from mdvit_amd.data import DeviceDataset, DomainBatches  # noqa: E402


def timed(fn, iters, warmup):
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


def pool(N, S, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randint(0, 256, (N, S, S, 3), generator=g, dtype=torch.uint8, device=dev),
            torch.randint(0, 2, (N, S, S), generator=g, dtype=torch.uint8, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T, B = 512, 256, 16

    img, mask = pool(256, S, 0, dev)
    ds = DeviceDataset(img, mask, size=T, set_id=0, device=dev)
    gen = torch.Generator().manual_seed(1)
    lists = [torch.randperm(len(ds), generator=gen)[:B] for _ in range(8)]
    aug, k = TrainAug(p=0.5, seed=2), [0]

    def nxt():
        k[0] += 1
        return lists[k[0] % len(lists)]

    gather_bytes, aug_bytes = B * (S * S * 4 + T * T * 4), B * T * T * 20
    print(f"B = {B}, {S} x {S} -> {T} x {T}; pool of {len(ds)} samples, {ds.nbytes / 2**20:.0f} MiB")
    us = timed(lambda: ds.batch(nxt()), a.iters, a.warmup)
    print(f"  batch()              {us:9.1f} us per call   {gather_bytes / 1e6:6.1f} MB moved   {gather_bytes / us / 1e6:6.3f} TB/s")
    us2 = timed(lambda: aug(*ds.batch(nxt())), a.iters, a.warmup)
    print(f"  batch() + TrainAug   {us2:9.1f} us per call   {(gather_bytes + aug_bytes) / 1e6:6.1f} MB moved   {(gather_bytes + aug_bytes) / us2 / 1e6:6.3f} TB/s")
    t0 = time.perf_counter()
    for _ in range(a.iters):
        aug(*ds.batch(nxt()))
    host_us = (time.perf_counter() - t0) / a.iters * 1e6
    torch.cuda.synchronize()
    print(f"  host enqueue of batch() + TrainAug (index checks, two table uploads, two launches): {host_us:.1f} us per call")
    del ds, img, mask

    from mdvit_amd.train import mdvit_train_step
    torch.manual_seed(0)
    model = mdvit_amd.MDViT(img_size=T, drop_rate=0.1, drop_path_rate=0.1, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=4,
                            decoder_name="MLPFM").to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05, fused=True)
    sets = {name: DeviceDataset(*pool(a.samples, S, 10 + d, dev), size=T, set_id=d, device=dev) for d, name in enumerate(("isic2018", "PH2", "DMF", "SKD"))}
    db = DomainBatches(sets, batch_size=a.batch, seed=3)
    epoch = [iter(db)]

    def draw():
        try:
            return next(epoch[0])
        except StopIteration:
            epoch[0] = iter(db)
            return next(epoch[0])

    fixed = draw()

    def steps(drawn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            mdvit_train_step(model, draw() if drawn else fixed, optimizer=opt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    steps(True)                                                 # warm-up of every shape
    rows = [(steps(False), steps(True)) for _ in range(3)]      # alternating, to see the spread
    print(f"MDViT step at {T} x {T}, 4 domains x {a.batch} images, AdamW (ms per step over {a.steps} steps; three alternating repeats)")
    for pre, drawn in rows:
        print(f"  one fixed step's batches, drawn before the window {pre:8.2f}    drawn from DomainBatches inside the window {drawn:8.2f}")
    us4 = timed(draw, a.iters, a.warmup)
    print(f"  drawing one step's four batches alone (4 x (batch() + TrainAug)): {us4:.1f} us of GPU-event time")


if __name__ == "__main__":
    main()
