"""The train-augmentation kernel (csrc/augment.hip through ops.augment_normalize_u8 and mdvit_amd.augment.TrainAug) against restatements of its
specification written here: exact where the arithmetic is exact (identity, flips, integer maps, brightness / contrast, determinism), within one
level on a small share of the elements against an fp64 restatement where it is fp32 (general affine), statistically for the noise."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0]


def dev():
    return torch.device("cuda:0")


def rand_u8(shape, seed, hi=256):
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def normalize_cpu(levels):
    """levels [B,H,W,3] (integers 0..255) -> the loader's norm01 (float64 divide, cast) + permute + Normalize, fp32 [B,3,H,W]"""
    v = (levels.double() / 255.0).float()
    return ((v - MEAN) / STD).permute(0, 3, 1, 2).contiguous()


LUT = normalize_cpu(torch.arange(256).view(1, 1, 256, 1).expand(1, 1, 256, 3))[0, :, 0, :]       # [3, 256]


def to_levels(out):
    """normalised fp32 [B,3,H,W] -> the uint8 levels [B,H,W,3] it was made from; every value must BE one of the 256 normalised levels of its channel"""
    out = out.cpu()
    lv = torch.round((out * STD.view(1, 3, 1, 1) + MEAN.view(1, 3, 1, 1)) * 255.0).clamp(0, 255).long()
    back = torch.stack([LUT[c][lv[:, c]] for c in range(3)], dim=1)
    assert torch.equal(back, out), "an output value is not a normalised uint8 level"
    return lv.permute(0, 2, 3, 1).contiguous()


def run(img, mask, table, keys=None):
    from mdvit_amd import ops
    B = img.shape[0]
    params = torch.tensor(table, dtype=torch.float32).view(-1, 9) if not torch.is_tensor(table) else table.float().view(-1, 9)
    if params.shape[0] == 1 and B > 1:
        params = params.expand(B, 9).contiguous()
    keys = torch.zeros((B, 2), dtype=torch.int32) if keys is None else keys
    out, lab = ops.augment_normalize_u8(img.to(dev()), None if mask is None else mask.to(dev()), params.to(dev()), keys.to(dev()))
    torch.cuda.synchronize()
    return out.cpu(), None if lab is None else lab.cpu()


def reflect(i, n):
    """reflect-101 on an integer tensor"""
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    i = i.abs() % p
    return torch.where(i >= n, p - i, i)


# ---- the specification's noise and seven steps, restated (fp64, or fp32 to measure what rounding alone does) -----------------------------------
def hash32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def normals(k0, k1, e, dtype):
    """z(k0, k1; e): elements 2p and 2p + 1 are the cosine and sine branch of one Box-Muller draw from two hashes of p"""
    k0, k1, e = np.uint32(k0 & 0xffffffff), np.uint32(k1 & 0xffffffff), e.astype(np.uint32)
    p = e >> np.uint32(1)
    h1, h2 = hash32((p ^ k0) + k1), hash32((p ^ k1 ^ np.uint32(0x9e3779b9)) + k0)
    u1 = ((h1 >> np.uint32(8)).astype(np.int64) + 1).astype(dtype) * dtype(2.0 ** -24)
    u2 = (h2 >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
    r, ang = np.sqrt(dtype(-2.0) * np.log(u1)), dtype(2.0 * math.pi) * u2
    return np.where((e & np.uint32(1)) == 1, r * np.sin(ang), r * np.cos(ang)).astype(dtype)


def q(v):
    return torch.round(v).clamp(0, 255)          # torch.round: half to even


def restate(img, mask, params, keys, dtype):
    """the seven steps of the specification for a batch, in `dtype`: levels [B,H,W,3] (int64) and label [B,H,W] (bool)"""
    B, H, W, _ = img.shape
    npdt = np.float64 if dtype == torch.float64 else np.float32
    levels, labels = [], []
    ys_i, xs_i = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    x, y = xs_i.to(dtype), ys_i.to(dtype)
    for b in range(B):
        m00, m01, m02, m10, m11, m12, alpha, beta, sigma = (params[b, i].to(dtype) for i in range(9))
        xs, ys = m00 * x + m01 * y + m02, m10 * x + m11 * y + m12
        x0, y0 = torch.floor(xs), torch.floor(ys)
        fx, fy = (xs - x0).unsqueeze(-1), (ys - y0).unsqueeze(-1)
        src = img[b].to(dtype)
        if float(sigma) > 0:
            z = normals(int(keys[b, 0]), int(keys[b, 1]), np.arange(H * W * 3, dtype=np.int64), npdt)
            src = q(src + sigma * torch.from_numpy(z).view(H, W, 3))
        xa, xb, ya, yb = reflect(x0.long(), W), reflect(x0.long() + 1, W), reflect(y0.long(), H), reflect(y0.long() + 1, H)
        s00, s01, s10, s11 = src[ya, xa], src[ya, xb], src[yb, xa], src[yb, xb]
        v = (1 - fy) * ((1 - fx) * s00 + fx * s01) + fy * ((1 - fx) * s10 + fx * s11)
        t = q(alpha * q(v) + beta)
        levels.append(t.long())
        half = torch.tensor(0.5, dtype=dtype)
        labels.append(mask[b][reflect(torch.floor(ys + half).long(), H), reflect(torch.floor(xs + half).long(), W)] != 0)
    return torch.stack(levels), torch.stack(labels)


# ---- 1. identity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(3, 37, 53), (1, 1, 1), (1, 512, 512)])
def test_identity_is_image_normalize_u8(B, H, W):
    from mdvit_amd import ops
    img, mask = rand_u8((B, H, W, 3), 1), rand_u8((B, H, W), 2, hi=2)
    out, lab = run(img, mask, IDENT)
    want = ops.image_normalize_u8(img.to(dev())).cpu()
    assert out.shape == (B, 3, H, W) and lab.shape == (B, 1, H, W) and out.dtype == torch.float32 and lab.dtype == torch.float32
    assert torch.equal(out, want) and torch.equal(out, normalize_cpu(img))
    assert torch.equal(lab, mask.float().view(B, 1, H, W))
    out2, lab2 = run(img, None, IDENT)                       # without a mask: the same image, no label
    assert lab2 is None and torch.equal(out2, want)


# ---- 2. flips -----------------------------------------------------------------------------------------------------------------------------------
def flip_tables(H, W):
    return [IDENT, [-1.0, 0, W - 1.0, 0, 1, 0, 1, 0, 0], [1.0, 0, 0, 0, -1, H - 1.0, 1, 0, 0], [-1.0, 0, W - 1.0, 0, -1, H - 1.0, 1, 0, 0]]


def test_flips_are_exact():
    H, W = 37, 53
    img, mask = rand_u8((1, H, W, 3), 3).expand(4, H, W, 3).contiguous(), rand_u8((1, H, W), 4, hi=2).expand(4, H, W).contiguous()
    out, lab = run(img, mask, torch.tensor(flip_tables(H, W)))
    for b, dims in enumerate(([], [3], [2], [2, 3])):
        assert torch.equal(out[b], torch.flip(out[:1], dims)[0]) and torch.equal(lab[b], torch.flip(lab[:1], dims)[0]), dims
    assert torch.equal(out[0], normalize_cpu(img[:1])[0])


# ---- 3. exact integer maps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(32, 32), (37, 53)])
def test_integer_maps_are_exact_gathers(H, W):
    tables = [[0.0, 1, 0, -1, 0, H - 1.0, 1, 0, 0],          # a quarter turn
              [1.0, 0, 3, 0, 1, -2, 1, 0, 0], [1.0, 0, -40, 0, 1, 45, 1, 0, 0],      # shifts; the second crosses more than one reflection period
              [2.0, 0, 0, 0, 2, 0, 1, 0, 0]]                  # dst -> src scale of 2 about the origin
    B = len(tables)
    img, mask = rand_u8((B, H, W, 3), 5), rand_u8((B, H, W), 6, hi=2)
    out, lab = run(img, mask, torch.tensor(tables))
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for b, t in enumerate(tables):
        m = [int(v) for v in t[:6]]
        xs, ys = reflect(m[0] * x + m[1] * y + m[2], W), reflect(m[3] * x + m[4] * y + m[5], H)
        assert torch.equal(out[b], normalize_cpu(img[b][ys, xs].unsqueeze(0))[0]), t
        assert torch.equal(lab[b, 0], mask[b][ys, xs].float()), t


# ---- 4. general affine --------------------------------------------------------------------------------------------------------------------------
def test_general_affine_within_one_level_of_fp64():
    """Eight drawn tables (shift / scale / rotate forced on; flips, noise and brightness / contrast as drawn) at 96 x 128, a smooth and a random image,
    an ellipse mask, against the fp64 restatement: nothing off by more than one level, at most 2e-3 of the elements off by one, at most 1e-3 of the
    mask pixels different.  The same restatement in fp32 must itself stay below the caps (so the inputs cannot drift).
    Measured: fp32 restatement 1.7e-5 (smooth) / 2.2e-4 (random) of the elements off by one, none by more, 0 mask pixels; the kernel 1.4e-5 / 2.2e-4, none, 0."""
    from mdvit_amd.augment import compose_train_aug, draw_train_aug_scalars
    B, H, W = 8, 96, 128
    sc = draw_train_aug_scalars(B, torch.Generator().manual_seed(41))
    sc["flags"][:, 3] = True
    params, keys = compose_train_aug(sc, H, W), sc["keys"]
    assert bool(sc["flags"][:, 0].any()) and bool(sc["flags"][:, 4].any()) and bool(sc["flags"][:, 1].any())
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    smooth = torch.stack([127.5 + 127.5 * torch.sin(2 * math.pi * (x / W * (1 + 0.5 * c) + 0.1 * c)) * torch.cos(2 * math.pi * y / H * (1.5 - 0.25 * c)) for c in range(3)], -1)
    smooth = torch.round(smooth).clamp(0, 255).to(torch.uint8)
    mask = ((((y - 50) / 30) ** 2 + ((x - 60) / 45) ** 2) <= 1).to(torch.uint8).expand(B, H, W).contiguous()
    for name, img in (("smooth", smooth.expand(B, H, W, 3).contiguous()), ("random", rand_u8((1, H, W, 3), 7).expand(B, H, W, 3).contiguous())):
        want, want_lab = restate(img, mask, params, keys, torch.float64)
        r32, r32_lab = restate(img, mask, params, keys, torch.float32)
        d32 = (r32 - want).abs()
        print(f"{name}: fp32 restatement max {int(d32.max())} share {float((d32 == 1).double().mean()):.2e} mask {float((r32_lab != want_lab).double().mean()):.2e}")
        assert int(d32.max()) <= 1 and float((d32 == 1).double().mean()) <= 2e-3 and float((r32_lab != want_lab).double().mean()) <= 1e-3
        out, lab = run(img, mask, params, keys)
        d = (to_levels(out) - want).abs()
        miss = float(((lab[:, 0] != 0) != want_lab).double().mean())
        print(f"{name}: kernel max {int(d.max())} share {float((d == 1).double().mean()):.2e} mask {miss:.2e}")
        assert int(d.max()) <= 1, f"{name}: an element is off by {int(d.max())} levels"
        assert float((d == 1).double().mean()) <= 2e-3, f"{name}: {float((d == 1).double().mean()):.2e} of the elements are off by one level"
        assert miss <= 1e-3, f"{name}: {miss:.2e} of the mask pixels differ"
        assert bool(((lab == 0) | (lab == 1)).all())


# ---- 5. brightness / contrast -------------------------------------------------------------------------------------------------------------------
def test_brightness_contrast_is_exact_on_every_level():
    """alpha in {0.8125, 1, 1.1875} x beta in {-51, 0, 25.5}: every product and sum is exact in fp32, so the result is exactly q(alpha v + beta), with the
    clamps at both ends and the half-even ties (0.8125 * 8 = 6.5 -> 6, 0.8125 * 24 = 19.5 -> 20)"""
    ab = [(a, b) for a in (0.8125, 1.0, 1.1875) for b in (-51.0, 0.0, 25.5)]
    ramp = torch.arange(256).view(16, 16, 1)
    img = torch.cat([ramp, (ramp + 85) % 256, 255 - ramp], -1).to(torch.uint8).expand(len(ab), 16, 16, 3).contiguous()
    out, _ = run(img, None, torch.tensor([[1.0, 0, 0, 0, 1, 0, a, b, 0] for a, b in ab]))
    for i, (a, b) in enumerate(ab):
        want = q(a * img[i].float() + b)
        assert torch.equal(out[i], normalize_cpu(want.unsqueeze(0))[0]), (a, b)
    v = q(0.8125 * torch.tensor([8.0, 24.0]))
    assert v.tolist() == [6.0, 20.0]
    lv = to_levels(out)
    assert int(lv[0].min()) == 0 and int(lv[8].max()) == 255          # both clamps are reached


# ---- 6. noise -----------------------------------------------------------------------------------------------------------------------------------
def corr(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(torch.corrcoef(torch.stack([a, b]))[0, 1])


def test_noise_statistics_determinism_and_clamping():
    H = W = 128
    img = torch.full((3, H, W, 3), 128, dtype=torch.uint8)
    keys = torch.tensor([[0x1234567, -559038737], [77, 12345678], [0x1234567, -559038737]], dtype=torch.int32)
    noisy = [1.0, 0, 0, 0, 1, 0, 1, 0, 5.0]
    out, _ = run(img, None, noisy, keys)
    d = to_levels(out) - 128
    for b in range(3):
        db = d[b].double()
        mean, ratio, share = float(db.mean()), float(db.std() / math.sqrt(25 + 1 / 12)), float((db.abs() <= 5).double().mean())
        print(f"sample {b}: mean {mean:+.4f} std ratio {ratio:.4f} share(|d| <= 5) {share:.4f} (normal: {math.erf(5.5 / (5 * math.sqrt(2))):.4f})")
        assert abs(mean) <= 0.09 and abs(ratio - 1) <= 0.02 and abs(share - math.erf(5.5 / (5 * math.sqrt(2)))) <= 0.01
    cs = [corr(d[0, :, :, 0], d[0, :, :, 1]), corr(d[0, :, :, 1], d[0, :, :, 2]), corr(d[0, :, :, 0], d[0, :, :, 2]),
          corr(d[0, :, :-1], d[0, :, 1:]), corr(d[1, :, :-1], d[1, :, 1:]), corr(d[0], d[1])]
    print("correlations (channels 01 12 02, horizontal neighbours of samples 0 and 1, samples 0 / 1):", [f"{c:+.4f}" for c in cs])
    assert max(abs(c) for c in cs) <= 0.04, cs
    assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])          # the key alone decides the noise
    out_again, _ = run(img, None, noisy, keys)
    assert torch.equal(out_again, out)
    # noise lives on source pixels: the flipped launch is the flip of the unflipped one (on a varying image too)
    var = rand_u8((3, H, W, 3), 8)
    base, _ = run(var, None, noisy, keys)
    flipped, _ = run(var, None, [-1.0, 0, W - 1.0, 0, 1, 0, 1, 0, 5.0], keys)
    assert torch.equal(flipped, torch.flip(base, [3])) and not torch.equal(base, normalize_cpu(var))
    # clamping: on 0s and 255s every output is a level of [0, 255] (to_levels asserts that) and both ends stay reached
    ext = rand_u8((3, H, W, 3), 9, hi=2) * 255
    lv = to_levels(run(ext, None, noisy, keys)[0])
    assert int(lv.min()) == 0 and int(lv.max()) == 255
    assert bool((lv[ext == 0] <= 30).all()) and bool((lv[ext == 255] >= 225).all())          # |z| <= sqrt(2 * 24 ln 2) = 5.77


# ---- 7. TrainAug --------------------------------------------------------------------------------------------------------------------------------
def test_trainaug_batches_feed_the_model():
    import mdvit_amd
    from mdvit_amd.augment import TrainAug
    B, S = 4, 64
    img, mask = rand_u8((B, S, S, 3), 10).to(dev()), rand_u8((B, S, S), 11, hi=2).to(dev())
    a, b, c = TrainAug(seed=5), TrainAug(seed=5), TrainAug(seed=6)
    for _ in range(2):          # the second batch continues each generator
        ia, la = a(img, mask)
        ib, lb = b(img, mask)
        ic, _ = c(img, mask)
        assert torch.equal(ia, ib) and torch.equal(la, lb) and not torch.equal(ia, ic)
    assert ia.shape == (B, 3, S, S) and la.shape == (B, 1, S, S) and ia.dtype == la.dtype == torch.float32 and ia.is_contiguous() and la.is_contiguous()
    assert bool(((la == 0) | (la == 1)).all()) and tuple(a.flags.shape) == (B, 5)
    only, none = TrainAug(seed=5)(img)
    assert none is None and only.shape == (B, 3, S, S)
    ident, lab = TrainAug(p=0.0)(img, mask)
    assert torch.equal(ident.cpu(), normalize_cpu(img.cpu())) and torch.equal(lab[:, 0].cpu(), mask.cpu().float())
    # one forward and the step's losses take the pair as it is
    from mdvit_amd.losses import domain_losses
    m = mdvit_amd.MDViT(img_size=S, drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=4,
                        decoder_name="MLPFM").to(dev()).train()
    out, aux = m(ia, torch.nn.functional.one_hot(torch.full((B,), 1), 4).float().to(dev()), "1")
    assert out.shape == la.shape and bool(torch.isfinite(out).all())
    assert all(math.isfinite(float(v.detach())) for v in domain_losses(out, aux, la))
