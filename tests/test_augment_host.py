"""CPU-only checks of the device train augmentation (mdvit_amd/augment.py, csrc/augment_taps.h): the host-side draw of the per-sample tables, and the
tap arithmetic the kernel forms every address from, evaluated on the CPU through mdvit_augment_probe_taps."""
import ctypes as C
import math

import pytest
import torch

RANGES = {"noise_var": (10.0, 50.0), "dx": (-0.0625, 0.0625), "dy": (-0.0625, 0.0625), "scale": (0.9, 1.1), "angle": (-45.0, 45.0),
          "alpha": (0.8, 1.2), "beta": (-51.0, 51.0)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_draw_probabilities():
    """each transform applies independently with p = 0.5: over 20 000 samples every flag's frequency is within 4 sigma, sigma = sqrt(0.25 / 20000)"""
    from mdvit_amd.augment import draw_train_aug
    _, _, flags = draw_train_aug(20000, 512, 512, gen(11))
    assert flags.dtype == torch.bool and tuple(flags.shape) == (20000, 5)
    freq = flags.double().mean(0)
    assert bool(((freq - 0.5).abs() <= 0.015).all()), freq.tolist()
    # independent: no pair of flags moves together (|corr| of two fair coins over 20 000 draws: sigma = 0.007)
    c = torch.corrcoef(flags.double().T) - torch.eye(5, dtype=torch.float64)
    assert float(c.abs().max()) <= 0.03, c


def test_draw_ranges():
    from mdvit_amd.augment import draw_train_aug, draw_train_aug_scalars
    sc = draw_train_aug_scalars(20000, gen(12))
    for name, (lo, hi) in RANGES.items():
        v = sc[name]
        assert v.dtype == torch.float64 and float(v.min()) >= lo and float(v.max()) <= hi, name
        assert float(v.min()) < lo + 0.02 * (hi - lo) and float(v.max()) > hi - 0.02 * (hi - lo), f"{name} does not fill its range"
    params, keys, flags = draw_train_aug(20000, 96, 128, gen(12))
    assert params.dtype == torch.float32 and tuple(params.shape) == (20000, 9) and keys.dtype == torch.int32 and tuple(keys.shape) == (20000, 2)
    noise, bc = flags[:, 0], flags[:, 4]
    sig = params[:, 8]
    assert bool((sig[~noise] == 0).all()) and float(sig[noise].min()) >= math.sqrt(10.0) - 1e-6 and float(sig[noise].max()) <= math.sqrt(50.0) + 1e-6
    assert bool((params[~bc, 6] == 1).all()) and bool((params[~bc, 7] == 0).all())
    assert float(params[bc, 6].min()) >= 0.8 - 1e-6 and float(params[bc, 6].max()) <= 1.2 + 1e-6 and float(params[bc, 7].abs().max()) <= 51.0 + 1e-4
    # the linear part of the table is a rotation scaled by 1 / s, s in [0.9, 1.1], whatever the flips
    det = (params[:, 0] * params[:, 4] - params[:, 1] * params[:, 3]).abs().double()
    assert float(det.min()) >= 1 / 1.1 ** 2 - 1e-5 and float(det.max()) <= 1 / 0.9 ** 2 + 1e-5
    assert len(set(map(tuple, keys.tolist()))) == 20000          # the noise keys differ between samples


def test_draw_p0_is_identity():
    from mdvit_amd.augment import IDENTITY, draw_train_aug
    params, _, flags = draw_train_aug(257, 37, 53, gen(13), p=0.0)
    assert not bool(flags.any())
    assert torch.equal(params, torch.tensor(IDENTITY, dtype=torch.float32).expand(257, 9))
    assert not bool(torch.signbit(params).any())


def test_draw_is_deterministic():
    from mdvit_amd.augment import draw_train_aug
    a, b, c = draw_train_aug(64, 96, 128, gen(14)), draw_train_aug(64, 96, 128, gen(14)), draw_train_aug(64, 96, 128, gen(15))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # one generator, two batches: the second continues the stream
    g = gen(14)
    first, second = draw_train_aug(64, 96, 128, g), draw_train_aug(64, 96, 128, g)
    assert torch.equal(first[0], a[0]) and not torch.equal(second[0], a[0])


def test_draw_composition_matches_fp64_matrices():
    """the table is (M F)^-1 in fp64, cast: M = getRotationMatrix2D about ((W-1)/2, (H-1)/2) plus the shift, F the product of the drawn flips"""
    from mdvit_amd.augment import compose_train_aug, draw_train_aug, draw_train_aug_scalars
    H, W = 96, 128
    sc = draw_train_aug_scalars(64, gen(16))
    table = compose_train_aug(sc, H, W)
    assert torch.equal(table, draw_train_aug(64, H, W, gen(16))[0])
    fl = sc["flags"]
    assert all(bool(fl[:, i].any()) and not bool(fl[:, i].all()) for i in range(5))
    for i in range(64):
        noise, hflip, vflip, ssr, bc = (bool(f) for f in fl[i])
        M = torch.eye(3, dtype=torch.float64)
        if ssr:
            s, th = float(sc["scale"][i]), math.radians(float(sc["angle"][i]))
            a, b, cx, cy = s * math.cos(th), s * math.sin(th), (W - 1) / 2, (H - 1) / 2
            M = torch.tensor([[a, b, (1 - a) * cx - b * cy + float(sc["dx"][i]) * W], [-b, a, b * cx + (1 - a) * cy + float(sc["dy"][i]) * H], [0, 0, 1]],
                             dtype=torch.float64)
        F = torch.eye(3, dtype=torch.float64)
        if hflip:
            F = torch.tensor([[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]], dtype=torch.float64) @ F
        if vflip:
            F = torch.tensor([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]], dtype=torch.float64) @ F
        inv = torch.linalg.inv(M @ F)
        want = torch.cat([inv[0], inv[1], torch.tensor([float(sc["alpha"][i]) if bc else 1.0, float(sc["beta"][i]) if bc else 0.0,
                                                         math.sqrt(float(sc["noise_var"][i])) if noise else 0.0], dtype=torch.float64)])
        got = table[i].double()
        # relative to the row's scale: the translations are of the order of the image size, the linear entries of the order of 1
        scale = torch.tensor([1, 1, W, 1, 1, H, 1, 51, 1], dtype=torch.float64)
        assert float(((got - want).abs() / torch.maximum(want.abs(), scale)).max()) <= 1e-6, (i, got, want)


def probe(lib, xs, ys, H, W):
    idx, w = (C.c_int32 * 5)(), (C.c_float * 4)()
    assert lib.mdvit_augment_probe_taps(xs, ys, H, W, idx, w) == 0
    return list(idx), list(w)


def test_probe_taps_reflect_101():
    from mdvit_amd import _lib
    lib = _lib.load()
    for col, want in ((-1, 1), (-2, 2), (5, 3), (6, 2), (8, 0), (9, 1), (0, 0), (4, 4), (-8, 0), (-9, 1), (16, 0), (-4, 4)):
        idx, w = probe(lib, float(col), 0.0, 1, 5)
        assert idx[0] == want and idx[4] == want and w == [1.0, 0.0, 0.0, 0.0], (col, idx, w)
    # rows: the same reflection on the other axis
    for row, want in ((-1, 1), (-2, 2), (5, 3), (6, 2), (8, 0), (9, 1)):
        idx, _ = probe(lib, 2.0, float(row), 5, 7)
        assert idx[0] == want * 7 + 2 and idx[4] == want * 7 + 2, (row, idx)
    # the x + 1 / y + 1 taps reflect on their own: column 4.5 of 5 -> taps 4 and 3
    idx, w = probe(lib, 4.5, 0.0, 1, 5)
    assert idx[:2] == [4, 3] and w == [0.5, 0.5, 0.0, 0.0] and idx[4] == 3      # nearest: floor(5.0) = 5 -> 3
    # a single row / column: every tap is 0
    for xs, ys in ((3.7, -2.2), (-100.0, 55.5), (0.0, 0.0)):
        assert probe(lib, xs, ys, 1, 1)[0] == [0] * 5
        idx, _ = probe(lib, xs, ys, 5, 1)
        assert all(0 <= i < 5 for i in idx)
        idx, _ = probe(lib, xs, ys, 1, 5)
        assert all(0 <= i < 5 for i in idx)


def test_probe_taps_bilinear_weights():
    from mdvit_amd import _lib
    lib = _lib.load()
    for xs, ys in ((3.0, 4.0), (0.0, 0.0), (36.0, 52.0), (-3.0, 60.0)):      # integer coordinates: one tap
        idx, w = probe(lib, xs, ys, 53, 37)
        assert w == [1.0, 0.0, 0.0, 0.0], (xs, ys, w)
    idx, w = probe(lib, 3.25, 4.5, 53, 37)
    assert idx == [4 * 37 + 3, 4 * 37 + 4, 5 * 37 + 3, 5 * 37 + 4, 5 * 37 + 3] and w == [0.375, 0.125, 0.375, 0.125]
    idx, w = probe(lib, 3.75, 4.25, 53, 37)
    assert idx[4] == 4 * 37 + 4 and w == [0.1875, 0.5625, 0.0625, 0.1875]


def test_probe_taps_are_safe_for_every_float():
    """whatever the coordinate holds, every index lies inside the image and the weights are finite, in [0, 1] and sum to 1"""
    from mdvit_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    vals = [nan, inf, -inf, 1e30, -1e30, -0.0, -1e9, 1e9, 3.4e38, -3.4e38, 2147483648.0, -2147483648.0, 1073741824.0, -1e-30, 1e-45, 16777217.0, 0.49999997, -0.5]
    for H, W in ((37, 53), (1, 1), (1, 5), (512, 512), (2, 2)):
        for xs in vals:
            for ys in vals + [7.3]:
                idx, w = probe(lib, xs, ys, H, W)
                assert all(0 <= i <= H * W - 1 for i in idx), (xs, ys, H, W, idx)
                assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in w) and abs(sum(w) - 1.0) <= 1e-6, (xs, ys, w)
    # non-finite coordinates map to tap 0 with weight 1
    for bad in (nan, inf, -inf, -0.0):
        idx, w = probe(lib, bad, bad, 37, 53)
        assert idx[0] == 0 and idx[4] == 0 and w == [1.0, 0.0, 0.0, 0.0], (bad, idx, w)
    # -1e9 is still reflected exactly: |i| mod 2 (n - 1), mirrored
    i = 10 ** 9 % 104
    assert probe(lib, -1e9, 0.0, 1, 53)[0][0] == (i if i < 53 else 104 - i)


def test_augment_bad_arguments_return_error_codes_without_gpu():
    """argument validation happens before any HIP call, so it can be exercised on a CPU-only box"""
    from mdvit_amd import _lib
    lib = _lib.load()
    p = 64            # a non-NULL, aligned value: nothing is dereferenced before the checks pass
    assert lib.mdvit_augment_normalize_u8(None, None, p, p, p, None, 1, 8, 8, None) == 1          # MDVIT_E_SHAPE
    assert b"augment_normalize_u8" in lib.mdvit_last_error()
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, None, 0, 8, 8, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, None, 1, 0, 8, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, None, 1, 8, -1, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, None, p, p, None, 1, 8, 8, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, None, p, None, 1, 8, 8, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, None, None, 1, 8, 8, None) == 1
    # mask and label come together
    assert lib.mdvit_augment_normalize_u8(p, p, p, p, p, None, 1, 8, 8, None) == 1
    assert b"both" in lib.mdvit_last_error()
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, p, 1, 8, 8, None) == 1
    # the sample rides on a grid axis; the noise counter is 32 bits wide
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, None, 65536, 8, 8, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p, None, 1, 32768, 32768, None) == 1
    assert lib.mdvit_augment_normalize_u8(p, None, p, p, p + 2, None, 1, 8, 8, None) == 3         # MDVIT_E_ALIGN
    assert b"aligned" in lib.mdvit_last_error()
    idx, w = (C.c_int32 * 5)(), (C.c_float * 4)()
    assert lib.mdvit_augment_probe_taps(0.0, 0.0, 0, 5, idx, w) == 1
    assert lib.mdvit_augment_probe_taps(0.0, 0.0, 5, 5, None, w) == 1
    assert lib.mdvit_augment_probe_taps(0.0, 0.0, 5, 5, idx, None) == 1
    assert lib.mdvit_augment_probe_taps(0.0, 0.0, 65536, 65536, idx, w) == 1
    assert b"augment_probe_taps" in lib.mdvit_last_error()


def test_ops_and_trainaug_refuse_host_tensors():
    from mdvit_amd import _lib, ops
    from mdvit_amd.augment import TrainAug
    u8 = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(_lib.MdvitHipError):
        ops.augment_normalize_u8(u8, None, torch.zeros(1, 9), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        TrainAug()(u8)
