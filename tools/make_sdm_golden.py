"""Write tests/golden/signed_distance_cases.npz: the label masks of the signed-distance tests and what scipy makes of them (CPU only; needs scipy.ndimage;
never run by a test).

    python tools/make_sdm_golden.py

For every case, with pos the mask: Kervadec et al.'s one_hot2dist (MIDL 2019, "Boundary loss for highly unbalanced segmentation") on one 2-D image,
    phi = distance_transform_edt(~pos) * ~pos - (distance_transform_edt(pos) - 1) * pos        (float64)
    d2  = rint(distance_transform_edt(~pos) ** 2) on the background, rint(distance_transform_edt(pos) ** 2) on the foreground        (int32)
The two degenerate cases hold zeros: one_hot2dist returns zeros for an empty mask; for a full mask scipy measures to a zero that does not exist (1, 1.414,
2.236, ... on an all-ones image), which is no distance -- the project defines d2 = 0 and phi = 0 there too.

File layout: names [K] str, sizes [K,2] int32 (H, W), and per case k the arrays mask_k (numpy.packbits of the flattened mask, big-endian bit order),
d2_k int32 [H,W] and phi_k float64 [H,W]."""
import os
import sys

import numpy as np
from scipy.ndimage import distance_transform_edt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "signed_distance_cases.npz")


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[:H, :W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def random_mask(seed, H, W, density):
    """neither empty nor full"""
    m = np.random.default_rng(seed).random((H, W)) < density
    m.flat[0], m.flat[-1] = True, False
    return m


def cases():
    out = {}
    line = np.zeros(7, dtype=bool)
    line[[1, 5, 6]] = True
    out["row_1x7"], out["column_7x1"] = line.reshape(1, 7), line.reshape(7, 1)
    one = np.zeros((5, 5), dtype=bool)
    one[0, 4] = True
    out["corner_pixel_5x5"], out["single_background_5x5"] = one, ~np.roll(one, (2, -3), (0, 1))
    for dens in (0.02, 0.5, 0.98):
        out[f"random{dens}_33x45"] = random_mask(int(dens * 100), 33, 45, dens)          # rows of a partial 64-pixel word
    out["random0.3_64x65"] = random_mask(64, 64, 65, 0.3)                                # rows that cross a word
    out["random0.1_40x130"] = random_mask(40, 40, 130, 0.1)
    yy, xx = np.mgrid[:33, :45]
    out["checker_33x45"] = ((yy + xx) % 2) == 0                                           # every d2 = 1
    two = np.zeros((48, 64), dtype=bool)
    two[3:9, 4:11] = True
    two[36:45, 50:61] = True
    out["two_blobs_48x64"] = two                                                          # between them the nearest pixel of the other class is diagonal
    out["disc_48x64"] = disc(48, 64, 22, 30, 15)
    out["empty_33x45"], out["full_33x45"] = np.zeros((33, 45), dtype=bool), np.ones((33, 45), dtype=bool)
    lesion = disc(256, 256, 120, 140, 70) | disc(256, 256, 150, 90, 45) | disc(256, 256, 60, 200, 20)
    out["lesion_hole_256x256"] = lesion & ~disc(256, 256, 125, 130, 18)
    return out


def kervadec(pos):
    if not pos.any() or pos.all():
        return np.zeros(pos.shape, dtype=np.int32), np.zeros(pos.shape, dtype=np.float64)
    neg = ~pos
    out_d, in_d = distance_transform_edt(neg), distance_transform_edt(pos)
    phi = out_d * neg - (in_d - 1) * pos
    d2 = np.rint(np.where(pos, in_d, out_d) ** 2).astype(np.int32)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), np.where(pos, in_d, out_d))
    return d2, phi


def main():
    names, sizes, arrays = [], [], {}
    for k, (name, m) in enumerate(cases().items()):
        names.append(name)
        sizes.append(m.shape)
        arrays[f"mask_{k}"] = np.packbits(m.reshape(-1))
        arrays[f"d2_{k}"], arrays[f"phi_{k}"] = kervadec(m)
    np.savez_compressed(OUT, names=np.array(names), sizes=np.array(sizes, dtype=np.int32), **arrays)
    print(f"{OUT}: {len(names)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
