"""The signed distance map and the boundary loss without a GPU: a numpy restatement of the map (d2 by brute force over the pairs of opposite-class pixels, then
the fp32 rule phi = pos ? 1 - sqrt(d2) : sqrt(d2), zeros for a one-class image) against the committed scipy results (tests/golden/signed_distance_cases.npz,
tools/make_sdm_golden.py), a float64 restatement of the loss and its gradient, the workspace queries, and the refusals that need no device.  The GPU tests import
the restatements and the fixture reader from here; nothing in this file imports scipy."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "signed_distance_cases.npz")


# ---- the restatement of the map -------------------------------------------------------------------------------------------------
def restate_d2(pos):
    """mask [H,W] -> int64 [H,W]: the squared distance of every pixel to the nearest pixel of the other class, brute force over the (foreground, background)
    pairs in chunks (one pair matrix serves both directions); zeros when the image holds one class only"""
    pos = np.asarray(pos, dtype=bool)
    out = np.zeros(pos.shape, dtype=np.int64)
    fy, fx = (v.astype(np.int32) for v in np.nonzero(pos))
    by, bx = (v.astype(np.int32) for v in np.nonzero(~pos))
    if len(fy) == 0 or len(by) == 0:
        return out
    f_best = np.empty(len(fy), dtype=np.int32)
    b_best = np.full(len(by), np.iinfo(np.int32).max, dtype=np.int32)
    step = max(1, (1 << 22) // len(by))
    for i in range(0, len(fy), step):
        dy, dx = fy[i:i + step, None] - by[None], fx[i:i + step, None] - bx[None]
        pair = dy * dy + dx * dx
        f_best[i:i + step] = pair.min(1)
        np.minimum(b_best, pair.min(0), out=b_best)
    out[fy, fx], out[by, bx] = f_best, b_best
    return out


def restate_phi(pos, d2):
    """the fp32 rule: r = sqrtf((float)d2), phi = pos ? 1 - r : r; zeros for a one-class image (there d2 = 0 everywhere)"""
    pos = np.asarray(pos, dtype=bool)
    if not pos.any() or pos.all():
        return np.zeros(pos.shape, dtype=np.float32)
    r = np.sqrt(d2.astype(np.float32))
    return np.where(pos, np.float32(1.0) - r, r).astype(np.float32)


# ---- the restatement of the loss, float64 ---------------------------------------------------------------------------------------
def loss_ref(x, phi, groups=1):
    """x, phi [B,...] -> the sum over the `groups` equal consecutive domain batches of mean(sigmoid(x) * phi), float64"""
    x, phi = np.asarray(x, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    Bd = x.shape[0] // groups
    return float(sum((s[g * Bd:(g + 1) * Bd] * phi[g * Bd:(g + 1) * Bd]).mean() for g in range(groups)))


def grad_ref(x, phi, g=1.0, groups=1):
    """dL/dx = g phi s (1 - s) / (Bd H W), float64; s (1 - s) = e / (1 + e)^2 with e = exp(-|x|), exact for saturated logits too"""
    x, phi = np.asarray(x, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return float(g) * phi * (e / (1.0 + e) ** 2) / (x.size // groups)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
_cache = {}


def load_cases():
    """{name: {"mask" bool [H,W], "d2" int64 [H,W], "phi" float64 [H,W]}} in the file's order, read once"""
    if "cases" not in _cache:
        z = np.load(GOLDEN, allow_pickle=False)
        cases = {}
        for k, name in enumerate(z["names"].tolist()):
            H, W = (int(v) for v in z["sizes"][k])
            cases[name] = {"mask": np.unpackbits(z[f"mask_{k}"])[:H * W].reshape(H, W).astype(bool), "d2": z[f"d2_{k}"].astype(np.int64), "phi": z[f"phi_{k}"]}
        _cache["cases"] = cases
    return _cache["cases"]


def restated(name):
    """(d2 int64, phi fp32) of a fixture case by the restatement, computed once per process"""
    if name not in _cache:
        m = load_cases()[name]["mask"]
        d2 = restate_d2(m)
        _cache[name] = (d2, restate_phi(m, d2))
    return _cache[name]


def case_names():
    return list(load_cases())


def ulps32(got, want):
    """the largest |got - want| in units of the fp32 spacing at `want`"""
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).max())


# ---- 1. the restatement against scipy's results ---------------------------------------------------------------------------------
def test_the_fixture_is_small_and_holds_the_listed_cases():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    sizes = [c["mask"].shape for c in load_cases().values()]
    assert set(sizes) == {(1, 7), (7, 1), (5, 5), (33, 45), (64, 65), (40, 130), (48, 64), (256, 256)}
    c = load_cases()
    assert c["corner_pixel_5x5"]["mask"].sum() == 1 and (~c["single_background_5x5"]["mask"]).sum() == 1
    assert not c["empty_33x45"]["mask"].any() and c["full_33x45"]["mask"].all()
    assert (c["checker_33x45"]["d2"] == 1).all()
    for name in ("empty_33x45", "full_33x45"):          # the two degenerate rules
        assert not c[name]["d2"].any() and not c[name]["phi"].any()
    # between the blobs (rows 3..8 x columns 4..10 and rows 36..44 x columns 50..60) the nearest pixel of the other class is diagonal: 14 rows and 20 columns away
    assert c["two_blobs_48x64"]["d2"][22, 30] == 14 ** 2 + 20 ** 2


@pytest.mark.parametrize("name", case_names())
def test_restatement_equals_scipy(name):
    c = load_cases()[name]
    d2, phi = restated(name)
    assert np.array_equal(d2, c["d2"])                    # integer for integer
    assert phi.dtype == np.float32
    u = ulps32(phi, c["phi"])
    print(f"{name}: max d2 {int(d2.max())}, phi against scipy's float64 map: {u:.3f} fp32 ulp")
    assert u <= 1.0
    m = c["mask"]
    if m.any() and not m.all():
        assert (phi[m] <= 0).all() and (phi[~m] >= 1).all() and (d2 >= 1).all()


def test_every_squared_distance_has_a_bit_exact_fp32_root():
    """d2 <= 2 * 1023^2 < 2^21: float32(sqrt_fp64(n)) == sqrt_fp32(float32(n)) for every such n, so a correctly rounded sqrtf pins phi bit for bit"""
    n = np.arange(2 * 1023 ** 2 + 1, dtype=np.int64)
    assert 2 * 1023 ** 2 < 1 << 21
    assert np.array_equal(np.sqrt(n.astype(np.float64)).astype(np.float32), np.sqrt(n.astype(np.float32)))


def test_loss_restatement_on_a_case_worked_by_hand():
    x = np.array([[[0.0, np.log(3.0)], [-np.log(3.0), 0.0]]])          # sigmoid: 1/2, 3/4, 1/4, 1/2
    phi = np.array([[[2.0, -1.0], [4.0, 0.0]]])
    assert np.isclose(loss_ref(x, phi), (1.0 - 0.75 + 1.0 + 0.0) / 4.0, rtol=1e-15)
    assert np.allclose(grad_ref(x, phi, 2.0), 2.0 * phi * np.array([[[0.25, 0.1875], [0.1875, 0.25]]]) / 4.0, rtol=1e-15)
    x2, phi2 = np.concatenate([x, -x]), np.concatenate([phi, 3.0 * phi])
    assert np.isclose(loss_ref(x2, phi2, groups=2), loss_ref(x, phi) + loss_ref(-x, 3.0 * phi), rtol=1e-15)          # the sum of the batches' means
    assert np.allclose(grad_ref(x2, phi2, 1.0, groups=2)[0], grad_ref(x, phi)[0], rtol=1e-15)
    assert grad_ref(np.array([[[40.0]]]), np.array([[[1.0]]]))[0, 0, 0] > 0          # a saturated logit keeps its (tiny) gradient


# ---- 2. the workspace queries and the refusals that need no device --------------------------------------------------------------
def test_workspace_queries():
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    prev = 0
    for n in (1, 2, 3, 16, 65535):
        got = lib.mdvit_signed_distance_ws_bytes(n, 33, 45)
        assert got >= n * 33 * 45 * 4 and got % 8 == 0 and got > prev, (n, got)          # two uint16 distances per pixel, monotone in n
        assert ops.signed_distance_ws_bytes(n, 33, 45) == got
        prev = got
    assert lib.mdvit_signed_distance_ws_bytes(65535, 1024, 1024) >= 65535 * 4 << 20          # no 32-bit overflow at the largest size
    for n, H, W in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 1025), (1, 1025, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.mdvit_signed_distance_ws_bytes(n, H, W) == 0, (n, H, W)
    prev = 0
    for n in (1, 2, 4, 64, 4096):
        got = lib.mdvit_boundary_loss_ws_bytes(n, 64 * 65, 1)
        assert got >= 8 and got % 8 == 0 and got >= prev, (n, got)
        prev = got
    assert lib.mdvit_boundary_loss_ws_bytes(4, 64 * 65, 4) == 4 * lib.mdvit_boundary_loss_ws_bytes(1, 64 * 65, 1)
    for n, hw, G in ((0, 8, 1), (4, 0, 1), (4, 8, 0), (4, 8, 3), (4, 8, 65), (4, 1024 * 1024 + 1, 1)):
        assert lib.mdvit_boundary_loss_ws_bytes(n, hw, G) == 0, (n, hw, G)


def test_entries_refuse_bad_arguments_before_any_launch():
    from mdvit_amd import _lib
    lib = _lib.load()
    assert lib.mdvit_signed_distance(None, 1, 1025, 8, None, None, None, 0, None) == 1          # MDVIT_E_SHAPE
    assert b"signed_distance" in lib.mdvit_last_error() and b"1024" in lib.mdvit_last_error()
    assert lib.mdvit_signed_distance(None, 1, 8, 8, None, None, None, 0, None) == 1
    assert b"NULL" in lib.mdvit_last_error()
    assert lib.mdvit_boundary_loss_fwd(None, None, 4, 64, 3, None, None, 0, None) == 1
    assert b"boundary_loss_fwd" in lib.mdvit_last_error() and b"groups" in lib.mdvit_last_error()
    assert lib.mdvit_boundary_loss_bwd(None, None, None, 4, 64, 2, None, None) == 1
    assert b"boundary_loss_bwd" in lib.mdvit_last_error() and b"NULL" in lib.mdvit_last_error()


def test_value_errors_that_need_no_device():
    import mdvit_amd
    from mdvit_amd import losses, ops
    assert mdvit_amd.signed_distance is ops.signed_distance and losses.signed_distance is ops.signed_distance and mdvit_amd.boundary_loss is losses.boundary_loss
    for shape in ((1, 1025, 8), (1, 1, 8, 1025)):          # a side > 1024
        with pytest.raises(ValueError, match="1024"):
            ops.signed_distance(torch.zeros(shape))
        with pytest.raises(ValueError, match="1024"):
            ops.boundary_loss(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="expects"):
        ops.signed_distance(torch.zeros((2, 3, 8, 8)))          # not 1-channel
    x = torch.zeros((4, 1, 8, 9))
    with pytest.raises(ValueError, match="disagree"):
        ops.boundary_loss(x, torch.zeros((4, 1, 9, 8)))
    with pytest.raises(ValueError, match="disagree"):
        ops.boundary_loss(x, torch.zeros((4, 8, 9)))
    for G in (3, 0, 8):
        with pytest.raises(ValueError, match="equal domain batches"):
            ops.boundary_loss(x, torch.zeros_like(x), groups=G)
    with pytest.raises(ValueError, match="fp32"):
        ops.boundary_loss(x.double(), torch.zeros_like(x))
    with pytest.raises(ValueError, match="fp32"):
        ops.boundary_loss(x, torch.zeros_like(x).half())


def test_the_train_steps_take_the_weight_and_default_to_zero():
    import inspect
    from mdvit_amd import train
    for fn in (train.mdvit_train_step, train.base_train_step):
        p = inspect.signature(fn).parameters["boundary_weight"]
        assert p.default == 0.0
