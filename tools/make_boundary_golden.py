"""Write tests/golden/boundary_cases.npz: the mask pairs of the boundary tests and what scipy + numpy make of them (CPU only; needs scipy.ndimage).

    python tools/make_boundary_golden.py

For every case: medpy 0.4.0 metric/binary.py __surface_distances restated with scipy (voxelspacing None, connectivity 1)
    border(M) = M ^ binary_erosion(M, generate_binary_structure(2, 1), iterations=1)
    sd(A->Y)  = distance_transform_edt(~border(Y))[border(A)]
hd95 = numpy.percentile(hstack(sd(A->Y), sd(Y->A)), 95), hd = max of both, asd = mean of one direction, assd = mean of the two asd, and the sorted integer
d^2 of each direction (from the transform's nearest-point indices, checked against the squared distances).  A case with an empty mask has NaN scores and
empty d^2 lists (medpy raises there).

File layout: names [K] str, sizes [K,2] int32 (H, W), scores [K,5] float64 (hd95, hd, assd, asd pred->label, asd label->pred), and per case k the arrays
pred_k / label_k (numpy.packbits of the flattened mask, big-endian bit order) and d2_p2l_k / d2_l2p_k (int32, ascending)."""
import os
import sys

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "boundary_cases.npz")

SIZES = [(1, 70), (70, 1), (33, 45), (64, 64), (37, 130), (128, 192)]


def box(H, W, y0, y1, x0, x1):
    """a filled rectangle given in fractions of the image, at least one pixel"""
    m = np.zeros((H, W), dtype=bool)
    r0, c0 = min(int(H * y0), H - 1), min(int(W * x0), W - 1)
    m[r0:max(r0 + 1, int(H * y1)), c0:max(c0 + 1, int(W * x1))] = True
    return m


def random_mask(rng, H, W, density):
    m = rng.random((H, W)) < density
    m[rng.integers(H), rng.integers(W)] = True          # never empty
    return m


def disk(H, W, cy, cx, r):
    yy, xx = np.mgrid[:H, :W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def cases():
    out = {}
    for H, W in SIZES:
        tag = f"{H}x{W}"
        rng = np.random.default_rng(1000 * H + W)
        for dens in (0.02, 0.3, 0.98):
            out[f"random{dens}_{tag}"] = (random_mask(rng, H, W, dens), random_mask(rng, H, W, dens))
        m = random_mask(rng, H, W, 0.4)
        out[f"identical_{tag}"] = (m, m.copy())
        px = np.zeros((H, W), dtype=bool)
        px[H // 3, W // 3] = True
        out[f"full_vs_pixel_{tag}"] = (np.ones((H, W), dtype=bool), px)
        a, b = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
        a[0, 0] = True
        b[H - 1, W - 1] = True
        out[f"corners_{tag}"] = (a, b)          # M = 2: hd95 interpolates between the two equal-rank values
        edges = box(H, W, 0.0, 1.0, 0.4, 0.6) | box(H, W, 0.4, 0.6, 0.0, 1.0)          # a cross that touches all four image edges
        out[f"edges_{tag}"] = (edges, box(H, W, 0.25, 0.75, 0.25, 0.75))
        yy, xx = np.mgrid[:H, :W]
        out[f"checker_{tag}"] = (((yy + xx) % 2) == 0, box(H, W, 0.3, 0.7, 0.2, 0.6))          # every set pixel is a border pixel
        out[f"blobs_{tag}"] = (box(H, W, 0.05, 0.4, 0.05, 0.4) | box(H, W, 0.6, 0.95, 0.55, 0.9), box(H, W, 0.3, 0.8, 0.3, 0.8))
        # border bits in a few columns (rows) only: whole columns without one, in both sets
        if W > 1:
            out[f"gaps_{tag}"] = (box(H, W, 0.1, 0.9, 0.0, 0.08), box(H, W, 0.5, 0.6, 0.9, 0.95))
        else:
            out[f"gaps_{tag}"] = (box(H, W, 0.0, 0.08, 0.0, 1.0), box(H, W, 0.9, 0.95, 0.0, 1.0))
    # made to one size's own condition
    H, W = 37, 130
    cols = np.zeros((H, W), dtype=bool)
    cols[5:30, 63:65] = True          # the columns x = 63 and x = 64: the horizontal neighbours sit in the next word
    out["carry_63_64_37x130"] = (cols, box(H, W, 0.2, 0.8, 0.3, 0.7))
    H, W = 33, 45
    rng = np.random.default_rng(7)
    out["tie_33x45"] = (random_mask(rng, H, W, 0.3), random_mask(rng, H, W, 0.3))          # the GPU test gives some background pixels a tiny positive logit
    some = random_mask(rng, H, W, 0.2)
    none = np.zeros((H, W), dtype=bool)
    out["empty_pred_33x45"] = (none, some)
    out["empty_label_33x45"] = (some, none)
    out["both_empty_33x45"] = (none, none.copy())
    # one 512 x 512 pair of images
    H = W = 512
    rng = np.random.default_rng(512)
    speck = rng.random((H, W)) < 0.0005
    out["disks_512x512"] = (disk(H, W, 250, 240, 120) | speck, disk(H, W, 262, 256, 110))
    out["ring_512x512"] = (disk(H, W, 256, 256, 200) & ~disk(H, W, 256, 256, 150), box(H, W, 0.1, 0.5, 0.1, 0.95) | disk(H, W, 400, 100, 40))
    return out


STRUCT = generate_binary_structure(2, 1)


def border(m):
    return m ^ binary_erosion(m, structure=STRUCT, iterations=1)


def surface_distances(a, y):
    """-> (sd float64, d2 int64) over the border pixels of a, against the border of y"""
    ba, by = border(a), border(y)
    dt, idx = distance_transform_edt(~by, return_indices=True)
    yy, xx = np.nonzero(ba)
    d2 = (idx[0][yy, xx] - yy).astype(np.int64) ** 2 + (idx[1][yy, xx] - xx).astype(np.int64) ** 2
    sd = dt[ba]
    assert np.array_equal(np.rint(sd * sd).astype(np.int64), d2) and np.array_equal(sd, np.sqrt(d2.astype(np.float64)))
    return sd, d2


def main():
    names, sizes, scores, arrays = [], [], [], {}
    for k, (name, (a, y)) in enumerate(cases().items()):
        names.append(name)
        sizes.append(a.shape)
        arrays[f"pred_{k}"], arrays[f"label_{k}"] = np.packbits(a.reshape(-1)), np.packbits(y.reshape(-1))
        if a.any() and y.any():
            (s1, d1), (s2, d2) = surface_distances(a, y), surface_distances(y, a)
            scores.append([np.percentile(np.hstack((s1, s2)), 95), max(s1.max(), s2.max()), (s1.mean() + s2.mean()) / 2.0, s1.mean(), s2.mean()])
        else:
            assert name.startswith(("empty_", "both_empty"))
            d1 = d2 = np.zeros((0,), dtype=np.int64)
            scores.append([np.nan] * 5)
        arrays[f"d2_p2l_{k}"], arrays[f"d2_l2p_{k}"] = np.sort(d1).astype(np.int32), np.sort(d2).astype(np.int32)
    np.savez_compressed(OUT, names=np.array(names), sizes=np.array(sizes, dtype=np.int32), scores=np.array(scores, dtype=np.float64), **arrays)
    print(f"{OUT}: {len(names)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
