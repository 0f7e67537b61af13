"""The device-resident dataset's host side (mdvit_amd/data.py) without a GPU: the resize rules restated here in numpy -- tables and pixel formula, written
independently of data.py's table builder -- checked for the properties A.Resize's cv2.resize has (INTER_LINEAR image, INTER_NEAREST mask), data.py's tables
against them, the DomainBatches sampler against the reference's train-loop sampling (multi_train_MDViT.py:38-43,129-139), and the C entry's argument
checks.  tests/test_gpu_dataset.py compares the kernel with restate_resize byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

# (N, Hs, Ws, H, W): the shapes the GPU test runs (tests/test_gpu_dataset.py) and the 2^31-byte pool's
SHAPES = [(5, 16, 16, 8, 8), (3, 12, 18, 8, 8), (2, 8, 8, 8, 8), (2, 6, 10, 16, 12), (4, 33, 47, 16, 16), (9, 512, 512, 256, 256),
          (3, 9, 7, 9, 7), (3, 9, 11, 10, 7)]
RATIOS = sorted({(s, d) for (_, Hs, Ws, H, W) in SHAPES for (s, d) in ((Hs, H), (Ws, W))} | {(512, 384), (512, 224), (7, 20), (1, 5), (5, 1), (640, 256)})


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
def restate_linear_axis(src, dst):
    """-> (s0, s1, a0, a1) int64 [dst]:  fx = float32((d + 0.5) * (src / dst) - 0.5), s = floor(fx), f = float32(fx - s); s < 0: s = 0, f = 0;
    s >= src - 1: s = src - 1, f = 0; second tap min(s + 1, src - 1); a0 = rint((1 - f) * 2048), a1 = rint(f * 2048), half to even"""
    s0, s1, a0, a1 = [], [], [], []
    scale = src / dst                                   # double
    for d in range(dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(fx))
        f = np.float32(fx - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0.0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0.0)
        s0.append(s)
        s1.append(min(s + 1, src - 1))
        a0.append(int(np.rint(np.float32(np.float32(1.0) - f) * np.float32(2048.0))))
        a1.append(int(np.rint(np.float32(f * np.float32(2048.0)))))
    return tuple(np.array(v, dtype=np.int64) for v in (s0, s1, a0, a1))


def restate_nearest_axis(src, dst):
    return np.array([min(int(np.floor(d * src / dst)), src - 1) for d in range(dst)], dtype=np.int64)


def restate_resize(img, mask, H, W):
    """img uint8 [..., Hs, Ws, 3], mask uint8 [..., Hs, Ws] or None -> (uint8 [..., H, W, 3], uint8 [..., H, W] or None)
    t(row) = S[row][sx] a0 + S[row][sx1] a1;  dst = (((b0 (t(sy) >> 4)) >> 16) + ((b1 (t(sy1) >> 4)) >> 16) + 2) >> 2;  the mask takes its nearest tap"""
    img = np.asarray(img)
    Hs, Ws = img.shape[-3], img.shape[-2]
    y0, y1, b0, b1 = restate_linear_axis(Hs, H)
    x0, x1, a0, a1 = restate_linear_axis(Ws, W)
    S = img.astype(np.int64)
    A0, A1 = a0[:, None], a1[:, None]                   # along x, broadcast over the channel
    t = S[..., :, x0, :] * A0 + S[..., :, x1, :] * A1   # [..., Hs, W, 3]
    B0, B1 = b0[:, None, None], b1[:, None, None]
    out = (((B0 * (t[..., y0, :, :] >> 4)) >> 16) + ((B1 * (t[..., y1, :, :] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    m = None
    if mask is not None:
        yn, xn = restate_nearest_axis(Hs, H), restate_nearest_axis(Ws, W)
        m = np.asarray(mask)[..., yn, :][..., :, xn]
    return out.astype(np.uint8), m


def rand_pool(seed, N, Hs, Ws):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8), (rng.random((N, Hs, Ws)) < 0.4).astype(np.uint8)


# ---- properties of the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", RATIOS)
def test_weights_sum_to_2048_and_taps_stay_inside(src, dst):
    s0, s1, a0, a1 = restate_linear_axis(src, dst)
    assert np.array_equal(a0 + a1, np.full(dst, 2048))
    assert a0.min() >= 0 and a1.min() >= 0
    for s in (s0, s1, restate_nearest_axis(src, dst)):
        assert s.min() >= 0 and s.max() <= src - 1
    assert np.all((s1 == s0 + 1) | (s1 == src - 1))


@pytest.mark.parametrize("shape", [(6, 10, 16, 12), (33, 47, 16, 16), (12, 18, 8, 8), (16, 16, 8, 8), (9, 11, 10, 7), (5, 7, 1, 1), (1, 1, 4, 3)])
def test_a_constant_image_stays_constant(shape):
    Hs, Ws, H, W = shape
    for level in (0, 1, 127, 128, 254, 255):
        out, m = restate_resize(np.full((Hs, Ws, 3), level, dtype=np.uint8), np.full((Hs, Ws), level & 1, dtype=np.uint8), H, W)
        assert np.all(out == level) and np.all(m == (level & 1)), (shape, level)


@pytest.mark.parametrize("Hs,Ws", [(8, 8), (9, 7), (1, 5), (64, 48)])
def test_equal_size_is_the_input(Hs, Ws):
    img, mask = rand_pool(1, 2, Hs, Ws)
    out, m = restate_resize(img, mask, Hs, Ws)
    assert np.array_equal(out, img) and np.array_equal(m, mask)


@pytest.mark.parametrize("Hs,Ws", [(16, 16), (12, 20), (512, 512)])
def test_two_to_one_is_the_box_mean(Hs, Ws):
    """exactly 2 : 1, the reference's 512 -> 256: (a + b + c + d + 2) >> 2 for every pixel, what OpenCV's fast path computes"""
    img, _ = rand_pool(2, 1, Hs, Ws)
    # the extremes too: all-255 quads and quads whose sum has every remainder mod 4
    img[0, :2, :4] = np.array([[[255] * 3, [255] * 3, [0] * 3, [1] * 3], [[255] * 3, [255] * 3, [0] * 3, [0] * 3]], dtype=np.uint8)
    out, _ = restate_resize(img, None, Hs // 2, Ws // 2)
    S = img.astype(np.int64)
    want = (S[:, 0::2, 0::2] + S[:, 0::2, 1::2] + S[:, 1::2, 0::2] + S[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(out, want.astype(np.uint8))


@pytest.mark.parametrize("src,dst", RATIOS)
def test_nearest_picks_the_floor(src, dst):
    sn = restate_nearest_axis(src, dst)
    for d in range(dst):
        assert sn[d] == min((d * src) // dst, src - 1)          # the same floor in exact integer arithmetic
    img = np.arange(src, dtype=np.uint8)[None, :].repeat(3, 0) if src <= 256 else None
    if img is not None:
        _, m = restate_resize(np.zeros((3, src, 3), dtype=np.uint8), img, 3, dst)
        assert np.array_equal(m[0], sn.astype(np.uint8))


def test_upscaling_clamps_both_borders():
    """6 -> 16: the first output positions have fx < 0 (tap 0, weight 2048), the last ones land on or past src - 1 (both taps src - 1, weight 2048 on the first)"""
    s0, s1, a0, a1 = restate_linear_axis(6, 16)
    assert s0[0] == 0 and a0[0] == 2048 and a1[0] == 0
    assert s0[-1] == 5 and s1[-1] == 5 and a0[-1] == 2048 and a1[-1] == 0
    assert 0 < a1[2] < 2048


# ---- data.py's tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", RATIOS)
def test_table_builder_agrees_with_the_restatement(src, dst):
    from mdvit_amd.data import resize_table
    tab = resize_table(src, dst)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (5, dst) and tab.is_contiguous()
    want = np.stack(list(restate_linear_axis(src, dst)) + [restate_nearest_axis(src, dst)])
    assert np.array_equal(tab.numpy().astype(np.int64), want)


def test_package_exports_the_classes():
    import mdvit_amd
    from mdvit_amd import data
    assert mdvit_amd.DeviceDataset is data.DeviceDataset and mdvit_amd.DomainBatches is data.DomainBatches
    assert "DeviceDataset" in mdvit_amd.__all__ and "DomainBatches" in mdvit_amd.__all__


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------------
class Sized:
    """stands in for a DeviceDataset where only the sampling is tested"""

    def __init__(self, n, set_id=0):
        self.n, self.set_id = n, set_id

    def __len__(self):
        return self.n


def make(seed=3, rank=0, world=1, sizes=(("a", 23), ("b", 9), ("c", 16)), bs=4):
    from mdvit_amd.data import DomainBatches
    return DomainBatches({name: Sized(n, k) for k, (name, n) in enumerate(sizes)}, batch_size=bs, seed=seed, rank=rank, world=world)


def test_sampler_epoch_is_a_permutation_without_the_short_batch():
    """drop_last=True as the reference's train DataLoader has it: 23 samples in batches of 4 are 5 batches of distinct indices; the epoch is as long as the longest domain"""
    db = make()
    assert len(db) == 5
    steps = list(db.indices())
    assert len(steps) == 5 and all(list(s) == ["a", "b", "c"] for s in steps)
    for s in steps:
        assert all(v.dtype == torch.int64 and v.numel() == 4 and not v.is_cuda for v in s.values())
    a = torch.cat([s["a"] for s in steps])
    assert a.numel() == 20 and len(set(a.tolist())) == 20 and 0 <= int(a.min()) and int(a.max()) < 23
    # 16 samples: the first four batches are one whole permutation
    c = torch.cat([s["c"] for s in steps[:4]])
    assert sorted(c.tolist()) == list(range(16))


def test_sampler_short_domain_restarts_and_carries_over():
    """9 samples are 2 batches per permutation: steps 0-1, 2-3 and 4-5 each come from one permutation (distinct indices), the restart happens while the
    longest domain finishes, and -- like the reference's train_iters -- the position carries into the next epoch"""
    db = make()
    b = [s["b"] for s in db.indices()] + [s["b"] for s in db.indices()]
    assert len(b) == 10
    for k in range(0, 10, 2):
        pair = torch.cat([b[k], b[k + 1]]).tolist()
        assert len(set(pair)) == 8 and max(pair) < 9, (k, pair)
    assert len({tuple(v.tolist()) for v in b}) > 2          # new permutations, not one repeated


def test_sampler_seeds():
    one, two, other = make(seed=3), make(seed=3), make(seed=4)
    s1, s2, s3 = list(one.indices()), list(two.indices()), list(other.indices())
    for x, y in zip(s1, s2):
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert any(not torch.equal(x[k], y[k]) for x, y in zip(s1, s3) for k in x)
    # every domain has its own generator: two domains of one size do not sample alike, and a domain's stream does not depend on its neighbours
    same = make(sizes=(("a", 16), ("b", 16)))
    st = list(same.indices())
    assert any(not torch.equal(s["a"], s["b"]) for s in st)
    alone = make(sizes=(("a", 16),))
    assert all(torch.equal(x["a"], y["a"]) for x, y in zip(st, alone.indices()))
    assert one.aug_seed == two.aug_seed != other.aug_seed


@pytest.mark.parametrize("world", [2, 3])
def test_sampler_ranks_partition_every_permutation(world):
    """batch j of a permutation goes to rank j % world: together the ranks hold exactly the single-process batches, none twice, and all take len() steps"""
    sizes = (("a", 45), ("b", 13))
    whole = make(sizes=sizes, bs=4)
    ranks = [make(sizes=sizes, bs=4, rank=r, world=world) for r in range(world)]
    assert len({len(r) for r in ranks}) == 1 and len(ranks[0]) == -(-11 // world)
    # the first permutation of "a": 11 batches
    ref = [whole.next_indices()["a"] for _ in range(11)]
    got = {}
    for r, db in enumerate(ranks):
        for k in range(len(range(r, 11, world))):
            got[r + k * world] = db.next_indices()["a"]
    assert sorted(got) == list(range(11))
    for j in range(11):
        assert torch.equal(got[j], ref[j]), j
    assert make(sizes=sizes, bs=4, rank=1, world=2).aug_seed != make(sizes=sizes, bs=4, rank=0, world=2).aug_seed


def test_sampler_refuses_what_cannot_be_dealt():
    from mdvit_amd.data import DomainBatches
    with pytest.raises(ValueError):
        DomainBatches({"a": Sized(3)}, batch_size=4, seed=0)                      # not one full batch
    with pytest.raises(ValueError):
        DomainBatches({"a": Sized(9)}, batch_size=4, seed=0, rank=0, world=3)     # two batches for three ranks
    with pytest.raises(ValueError):
        DomainBatches({"a": Sized(9)}, batch_size=4, seed=0, rank=2, world=2)
    with pytest.raises(ValueError):
        DomainBatches({}, batch_size=4, seed=0)


# ---- the C entry's argument checks --------------------------------------------------------------------------------------------------------------------
def test_gather_resize_abi_refuses_bad_arguments_without_gpu():
    """MDVIT_E_SHAPE (1) / MDVIT_E_ALIGN (3) before any launch: null operands, a mask pool without a mask output, non-positive sizes, B or N out of range,
    tables of the wrong length, misaligned index / tables"""
    from mdvit_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p = lambda off=0: C.c_void_p(base + off)

    def call(img_pool=p(), mask_pool=p(), index=p(), ytab=p(), ylen=40, xtab=p(), xlen=40, img_out=p(), mask_out=p(), N=2, B=2, Hs=16, Ws=16, H=8, W=8):
        return lib.mdvit_gather_resize_u8(img_pool, mask_pool, index, ytab, ylen, xtab, xlen, img_out, mask_out, N, B, Hs, Ws, H, W, None)

    for kw in (dict(img_pool=None), dict(index=None), dict(ytab=None), dict(xtab=None), dict(img_out=None)):
        assert call(**kw) == 1, kw
        assert b"gather_resize_u8" in lib.mdvit_last_error() and b"null" in lib.mdvit_last_error()
    for kw in (dict(mask_pool=None), dict(mask_out=None)):
        assert call(**kw) == 1, kw
        assert b"mask" in lib.mdvit_last_error()
    for kw in (dict(Hs=0), dict(Ws=0), dict(H=0, ylen=0), dict(W=0, xlen=0), dict(Hs=-16), dict(W=-8, xlen=-40),
               dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(N=-3), dict(N=1 << 41),
               dict(Hs=1 << 15, Ws=1 << 15), dict(H=1 << 15, W=1 << 15, ylen=5 << 15, xlen=5 << 15),
               dict(ylen=39), dict(ylen=8), dict(xlen=41), dict(xlen=0), dict(H=16), dict(W=12)):
        assert call(**kw) == 1, kw
        assert b"gather_resize_u8" in lib.mdvit_last_error(), kw
    for kw in (dict(index=p(4)), dict(ytab=p(2)), dict(xtab=p(1))):
        assert call(**kw) == 3, kw
        assert b"aligned" in lib.mdvit_last_error()
