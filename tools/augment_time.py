"""The train-augmentation kernel ALONE (ops.augment_normalize_u8, one stream, nothing else on the GPU) next to what it replaces when nothing is augmented
(ops.image_normalize_u8 plus the label cast) at 16 x 512 x 512 and 128 x 512 x 512:  python tools/augment_time.py [--iters 20] [--warmup 5] [--seed 0]
Tables: as drawn (draw_train_aug, p = 0.5), the same with the noise forced off, and the identity.  Prints the time per launch (HIP events over `iters`
launches) and the achieved bytes/s against the algorithmic bytes: 3 image + 1 mask bytes read and 16 bytes written per pixel."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdvit_amd import ops  # noqa: E402
from mdvit_amd.augment import IDENTITY, draw_train_aug  # noqa: E402


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
    return t0.elapsed_time(t1) / iters * 1e3          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    assert a.iters >= 20, "time at least 20 launches"
    dev = torch.device("cuda:0")
    for B, S in ((16, 512), (128, 512)):
        g = torch.Generator().manual_seed(a.seed)
        img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        mask = torch.randint(0, 2, (B, S, S), generator=g, dtype=torch.uint8).to(dev)
        params, keys, flags = draw_train_aug(B, S, S, g)
        quiet = params.clone()
        quiet[:, 8] = 0.0
        ident = torch.tensor(IDENTITY).expand(B, 9).contiguous()
        keys = keys.to(dev)
        nbytes = B * S * S * 20
        print(f"{B} x {S} x {S}: {nbytes / 1e6:.1f} MB algorithmic; drawn flags (noise hflip vflip ssr bc): {flags.sum(0).tolist()} of {B}")
        rows = [("image_normalize_u8 + label cast", lambda: (ops.image_normalize_u8(img), mask.unsqueeze(1).float()))]
        for name, t in (("augment, drawn tables", params), ("augment, drawn, noise off", quiet), ("augment, identity tables", ident)):
            td = t.to(dev)
            rows.append((name, lambda td=td: ops.augment_normalize_u8(img, mask, td, keys)))
        for name, fn in rows:
            us = timed(fn, a.iters, a.warmup)
            print(f"  {name:34s} {us:9.1f} us   {nbytes / us / 1e6:7.3f} TB/s")


if __name__ == "__main__":
    main()
