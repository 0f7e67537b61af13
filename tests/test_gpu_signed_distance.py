"""mdvit_signed_distance on the GPU against the numpy restatement of tests/test_signed_distance_host.py (itself pinned to scipy by the committed fixture): d2 integer
for integer, phi to 1 fp32 ulp (0 expected: sqrtf is correctly rounded and every d2 < 2^21 is an exact fp32 integer), every output element written, two runs
bit-identical, and the largest size by an analytic expectation."""
import numpy as np
import pytest
import torch

from test_signed_distance_host import case_names, load_cases, restated, ulps32

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def run(masks, squared=True, channel=True):
    """bool [n,H,W] -> (phi fp32, d2 int32) numpy [n,H,W] through the entry, outputs poisoned first: every element must be written"""
    from mdvit_amd import ops
    n, H, W = masks.shape
    label = torch.from_numpy(masks.astype(np.float32)).to(dev())
    phi = torch.full((n, H, W), float("nan"), device=dev())
    d2 = torch.full((n, H, W), -7, dtype=torch.int32, device=dev())
    nbytes = ops.signed_distance_ws_bytes(n, H, W)
    ws = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=dev())
    ops.call("mdvit_signed_distance", label.data_ptr(), n, H, W, phi.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    phi, d2 = phi.cpu().numpy(), d2.cpu().numpy()
    assert not np.isnan(phi).any() and (d2 >= 0).all(), "an output element was not written"
    # the public op: the same bits, the label's shape, d2 only on request
    lab4 = label.view(n, 1, H, W) if channel else label
    got = ops.signed_distance(lab4, return_squared=squared)
    p2, q2 = got if squared else (got, None)
    assert p2.shape == lab4.shape and p2.dtype == torch.float32 and np.array_equal(p2.cpu().numpy().reshape(n, H, W).view(np.int32), phi.view(np.int32))
    if squared:
        assert q2.shape == lab4.shape and q2.dtype == torch.int32 and np.array_equal(q2.cpu().numpy().reshape(n, H, W), d2)
    return phi, d2


def compare(name, phi, d2):
    want_d2, want_phi = restated(name)
    assert np.array_equal(d2.astype(np.int64), want_d2), f"{name}: d2 differs at {int((d2 != want_d2).sum())} pixels"
    u = ulps32(phi, want_phi)
    print(f"{name}: phi against the restatement: {u:.3f} fp32 ulp")
    assert u <= 1.0, name


@pytest.mark.parametrize("name", case_names())
def test_every_case_alone(name):
    m = load_cases()[name]["mask"]
    phi, d2 = run(m[None], squared=True, channel=(m.shape[0] % 2 == 1))
    compare(name, phi[0], d2[0])
    again = run(m[None])
    assert np.array_equal(again[0].view(np.int32), phi.view(np.int32)) and np.array_equal(again[1], d2)          # bit-identical run to run
    run(m[None], squared=False)


@pytest.mark.parametrize("size", [(5, 5), (33, 45), (48, 64)])
def test_equal_sized_cases_as_one_batch(size):
    names = [n for n in case_names() if load_cases()[n]["mask"].shape == size]
    assert len(names) >= 2
    masks = np.stack([load_cases()[n]["mask"] for n in names])
    assert len({m.tobytes() for m in masks}) == len(names)          # every image different
    phi, d2 = run(masks)
    for i, n in enumerate(names):
        compare(n, phi[i], d2[i])


@pytest.mark.parametrize("complement", [False, True])
def test_1024_square_with_a_single_pixel_of_one_class(complement):
    """one foreground pixel at (700, 300) of a 1024 x 1024 image, and the complement: (y - 700)^2 + (x - 300)^2 on the majority class, 1 on the single pixel --
    columns without any pixel of the other class (the sentinel) and the largest distances, without a brute-force restatement"""
    H = W = 1024
    m = np.zeros((1, H, W), dtype=bool)
    m[0, 700, 300] = True
    if complement:
        m = ~m
    phi, d2 = run(m)
    yy, xx = np.mgrid[:H, :W]
    want = ((yy - 700) ** 2 + (xx - 300) ** 2).astype(np.int64)
    want[700, 300] = 1
    assert np.array_equal(d2[0].astype(np.int64), want)
    r = np.sqrt(want.astype(np.float32))
    want_phi = np.where(m[0], np.float32(1.0) - r, r).astype(np.float32)
    u = ulps32(phi[0], want_phi)
    print(f"1024 x 1024, complement {complement}: max d2 {int(d2.max())}, phi {u:.3f} fp32 ulp")
    assert u <= 1.0
    assert phi[0, 700, 300] == (1.0 if complement else 0.0) and d2.max() == 700 ** 2 + 723 ** 2          # the single pixel: background at distance 1, or a foreground pixel that touches the background


def test_a_side_of_1025_is_refused():
    from mdvit_amd import ops
    for shape in ((1, 1, 1025, 8), (2, 8, 1025)):
        with pytest.raises(ValueError, match="1024"):
            ops.signed_distance(torch.zeros(shape, device=dev()))
