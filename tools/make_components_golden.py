"""Write tests/golden/components_cases.npz: the masks of the connected-component tests and what scipy makes of them (CPU only; needs scipy.ndimage).

    python tools/make_components_golden.py

Connectivity 1 everywhere (generate_binary_structure(2, 1), the default of ndimage.label and ndimage.binary_fill_holes).  For a mask M:
    components(M) = ndimage.label(M);  areas = numpy.bincount(labels)[1:]  (scipy numbers components in the order of their first pixel)
    fill(M)       = ndimage.binary_fill_holes(M)
    largest(M)    = labels == 1 + argmax(areas)  (ties: the first, i.e. the smallest root label); an empty mask stays empty
    "fill" = fill(M), "largest" = largest(M), "fill_largest" = largest(fill(M))

File layout: names [K] str, sizes [K,2] int32 (H, W), and per case k, for every set s in pred / aux / label: s_k (numpy.packbits of the flattened mask,
big-endian bit order) and areas_s_k (int32, label order); for s in pred / aux and every mode: mode_s_k (the cleaned mask, packed the same way); for the
cases up to 64 x 64 and 37 x 130: labels_s_k, scipy's label image as uint16."""
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "components_cases.npz")
MODES = ("fill", "largest", "fill_largest")
SETS = ("pred", "aux", "label")
LABELS_UP_TO = ((1, 70), (70, 1), (33, 45), (64, 64), (37, 130))


# ---- patterns: (H, W, rng) -> bool [H,W] ------------------------------------------------------------------------------------------
def empty(H, W, rng):
    return np.zeros((H, W), dtype=bool)


def full(H, W, rng):
    return np.ones((H, W), dtype=bool)


def single(H, W, rng):
    m = empty(H, W, rng)
    m[H // 2, W // 2] = True
    return m


def checker(H, W, rng):
    yy, xx = np.mgrid[:H, :W]
    return (yy + xx) % 2 == 0


def spiral(H, W, rng):
    """a rectangular spiral one pixel wide with one-pixel gaps: one component with the longest label chain, and no hole"""
    m = empty(H, W, rng)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    inside = lambda a, b: 0 <= a < H and 0 <= b < W
    while True:
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and (not inside(ny2, nx2) or not m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def spiral_complement(H, W, rng):
    return ~spiral(H, W, rng)


def comb(H, W, rng):
    """a serpentine of vertical teeth joined alternately at the top and at the bottom: the teeth merge one U-turn at a time"""
    m = empty(H, W, rng)
    m[:, ::2] = True
    for k, x in enumerate(range(1, W - 1, 2)):
        m[0 if k % 2 == 0 else H - 1, x] = True
    return m


def frame(m, d, x_margin=None):
    """the one-pixel border of the rectangle at margin d (rows) / x_margin (columns)"""
    H, W = m.shape
    e = d if x_margin is None else x_margin
    m[d, e:W - e] = True
    m[H - 1 - d, e:W - e] = True
    m[d:H - d, e] = True
    m[d:H - d, W - 1 - e] = True


def rings(H, W, rng):
    """three nested rings with an island in the innermost hole; the outer ring runs along the image edge, so at 37 x 130 its hole ends at the last image
    column but one, next to the padding bits of a row-padded word"""
    m = empty(H, W, rng)
    for d in (0, 4, 8):
        frame(m, d)
    m[H // 2 - 1:H // 2 + 1, W // 2 - 2:W // 2 + 2] = True
    return m


def diag_ring(H, W, rng):
    """a ring whose top-left corner pixel is missing (closed there only diagonally: one component, the inside is still a hole under 4-connectivity of the
    background) around a second ring with two opposite corners missing (two components, and again a hole)"""
    m = empty(H, W, rng)
    frame(m, 2)
    m[2, 2] = False
    frame(m, 6)
    m[6, 6] = False
    m[H - 7, W - 7] = False
    return m


def gap_ring(H, W, rng):
    """a ring one pixel from the left edge with a one-pixel gap in the wall that faces it: the inside reaches the edge, so it is not a hole; a closed ring
    beside it"""
    m = empty(H, W, rng)
    h = min(H - 4, 20)
    m[2, 1:W // 2] = True
    m[2 + h - 1, 1:W // 2] = True
    m[2:2 + h, 1] = True
    m[2:2 + h, W // 2 - 1] = True
    m[2 + h // 2, 1] = False
    m[4:4 + 5, W // 2 + 2:W // 2 + 9] = True
    m[5:4 + 4, W // 2 + 3:W // 2 + 8] = False
    return m


def ties(H, W, rng):
    """two blobs of equal area (the later one in raster order is wider, the earlier one taller), a smaller third; the first wins"""
    m = empty(H, W, rng)
    m[H // 2:H // 2 + 6, 2:6] = True          # 24 pixels, later in raster order
    m[3:3 + 4, W - 9:W - 3] = True            # 24 pixels, first
    m[H - 4:H - 2, W // 2:W // 2 + 3] = True
    return m


def seam(H, W, rng):
    """a blob across x = 63 | 64 (one row or column images: a run across the seam) and a dot"""
    m = empty(H, W, rng)
    if W > 64:
        m[H // 4:H // 4 + max(1, H // 3), 57:70] = True
        m[H - 1, 3] = True
    else:          # 70 x 1: a vertical run across y = 63 | 64
        m[57:69, 0] = True
        m[3, 0] = True
    return m


def noise(H, W, rng):
    return rng.random((H, W)) < 0.55


def lesion(H, W, rng):
    """a few overlapping ellipses with salt-and-pepper noise: what a prediction looks like"""
    yy, xx = np.mgrid[:H, :W]
    m = empty(H, W, rng)
    for _ in range(3):
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        ry, rx = rng.uniform(0.12, 0.3) * H + 1, rng.uniform(0.12, 0.3) * W + 1
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m ^ (rng.random((H, W)) < 0.03)


PATTERNS = {f.__name__: f for f in (empty, full, single, checker, spiral, spiral_complement, comb, rings, diag_ring, gap_ring, ties, seam, noise, lesion)}

# (H, W): [(pred, aux, label)] -- empty inputs and ties appear for the auxiliary output too
CASES = {
    (1, 70): [("seam", "empty", "full"), ("noise", "seam", "noise"), ("full", "single", "seam"), ("empty", "noise", "single")],
    (70, 1): [("noise", "full", "single"), ("seam", "noise", "noise"), ("empty", "seam", "full")],
    (33, 45): [("rings", "ties", "lesion"), ("empty", "empty", "single"), ("diag_ring", "gap_ring", "rings"), ("ties", "rings", "ties"),
               ("checker", "spiral", "full"), ("noise", "diag_ring", "noise"), ("gap_ring", "lesion", "empty"), ("single", "full", "checker")],
    (64, 64): [("spiral", "spiral_complement", "comb"), ("comb", "checker", "spiral"), ("full", "ties", "empty"), ("rings", "noise", "lesion"),
               ("lesion", "rings", "lesion"), ("spiral_complement", "empty", "diag_ring")],
    (37, 130): [("rings", "seam", "lesion"), ("seam", "ties", "seam"), ("noise", "lesion", "noise"), ("gap_ring", "diag_ring", "rings"),
                ("spiral_complement", "comb", "spiral"), ("lesion", "rings", "ties")],
    (128, 192): [("noise", "lesion", "lesion"), ("checker", "rings", "comb"), ("rings", "seam", "lesion"), ("comb", "spiral", "checker")],
    (264, 300): [("lesion", "noise", "lesion"), ("spiral", "rings", "spiral_complement")],
}


def largest(m):
    lab, k = ndimage.label(m)
    if k == 0:
        return m.copy()
    return lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))


def clean(m, mode):
    if mode == "fill":
        return ndimage.binary_fill_holes(m)
    if mode == "largest":
        return largest(m)
    return largest(ndimage.binary_fill_holes(m))


def main():
    arrays, names, sizes = {}, [], []
    k = 0
    for (H, W), triples in CASES.items():
        for j, triple in enumerate(triples):
            rng = np.random.default_rng(1000 * H + 10 * W + j)
            masks = {s: PATTERNS[p](H, W, rng) for s, p in zip(SETS, triple)}
            names.append("{}+{}+{}_{}x{}".format(*triple, H, W))
            sizes.append((H, W))
            for s in SETS:
                m = masks[s]
                lab, cnt = ndimage.label(m)
                arrays[f"{s}_{k}"] = np.packbits(m.ravel())
                arrays[f"areas_{s}_{k}"] = np.bincount(lab.ravel(), minlength=1)[1:].astype(np.int32)
                assert len(arrays[f"areas_{s}_{k}"]) == cnt < 65536
                if (H, W) in LABELS_UP_TO:
                    arrays[f"labels_{s}_{k}"] = lab.astype(np.uint16)
                if s != "label":
                    for mode in MODES:
                        arrays[f"{mode}_{s}_{k}"] = np.packbits(clean(m, mode).ravel())
            k += 1
    # what the patterns promise
    for (H, W) in ((64, 64), (264, 300)):
        sp = spiral(H, W, None)
        assert ndimage.label(sp)[1] == 1 and ndimage.label(~sp)[1] == 1 and np.array_equal(ndimage.binary_fill_holes(sp), sp)
    assert ndimage.label(comb(64, 64, None))[1] == 1 and ndimage.label(checker(33, 45, None))[1] == (33 * 45 + 1) // 2
    r = rings(37, 130, None)
    assert ndimage.label(r)[1] == 4 and ndimage.binary_fill_holes(r).all() and not np.array_equal(largest(r), largest(ndimage.binary_fill_holes(r)))
    d = diag_ring(33, 45, None)
    assert ndimage.label(d)[1] == 3 and not d[2, 2] and not ndimage.binary_fill_holes(d)[2, 2]
    assert ndimage.binary_fill_holes(d)[3:-3, 3:-3].all()          # both insides are holes although the rings close only diagonally
    g = gap_ring(33, 45, None)
    assert not ndimage.binary_fill_holes(g)[4, 3] and ndimage.binary_fill_holes(g).sum() == g.sum() + 15
    t = ties(33, 45, None)
    a = np.bincount(ndimage.label(t)[0].ravel())[1:]
    assert a.tolist() == [24, 24, 6] and largest(t)[3, 45 - 9]
    np.savez_compressed(OUT, names=np.array(names), sizes=np.array(sizes, dtype=np.int32), **arrays)
    print(f"{OUT}: {k} cases, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
