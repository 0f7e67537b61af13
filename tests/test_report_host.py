"""The host half of the per-image report (mdvit_amd/report.py): the packed-mask layout and the score arithmetic on hand-made counts.  No GPU."""
import numpy as np
import pytest
import torch

from mdvit_amd.report import pack_masks, scores_from_counts, unpack_masks


@pytest.mark.parametrize("size", [(5, 7), (8, 8), (5, 13), (20, 37)], ids=["HW35", "HW64", "HW65", "20x37"])
def test_pack_unpack_round_trip_and_zero_tail(size):
    H, W = size
    HW, words = H * W, (H * W + 63) // 64
    rng = np.random.default_rng(HW)
    masks = (rng.random((3, H, W)) < 0.5).astype(np.uint8)
    masks[1] = 1                                                     # every pixel set: the tail of the last word is all that stays 0
    packed = pack_masks(masks)
    assert packed.dtype == np.uint64 and packed.shape == (3, words)
    # bit l of word j is pixel 64 j + l, written out with Python integers
    for n in range(3):
        flat = masks[n].reshape(-1)
        for j in range(words):
            want = sum(int(flat[p]) << (p - 64 * j) for p in range(64 * j, min(64 * j + 64, HW)))
            assert int(packed[n, j]) == want, (n, j)
    if HW % 64:
        assert int(packed[1, -1]) == (1 << (HW % 64)) - 1              # tail bits are zero
    back = unpack_masks(packed, (H, W))
    assert back.dtype == np.uint8 and back.shape == (3, H, W) and np.array_equal(back, masks)
    # the device tables are int64 tensors of the same words; a {0, 255} mask packs like {0, 1}
    assert np.array_equal(unpack_masks(torch.from_numpy(packed.view(np.int64)), (H, W)), masks)
    assert np.array_equal(pack_masks(torch.from_numpy(masks * 255)), packed)
    with pytest.raises(ValueError):
        unpack_masks(packed, (H + 64, W))


def test_scores_from_hand_made_counts():
    #                 |A&Y| |A| |Y| |Aaux&Y| |Aaux|
    counts = np.array([[3, 4, 5, 2, 2],          # domain 0
                       [0, 0, 0, 0, 0],          # domain 2: empty label, empty prediction: 0/0 -> 0 everywhere
                       [0, 0, 7, 0, 0],          # domain 0: nothing predicted, aux 0/|Y| = 0
                       [6, 6, 6, 0, 3],          # domain 2: perfect main output
                       [0, 2, 0, 0, 0]],         # domain 3: empty label, two false positives
                      dtype=np.int64)
    domains = [0, 2, 0, 2, 3]
    structure = np.array([0.5, 1.25, 2.0, 0.25, 4.0])
    res = scores_from_counts(counts, domains, structure)
    assert res["domain"].dtype == np.int32 and res["domain"].tolist() == domains and np.array_equal(res["counts"], counts)
    for k in ("dice", "iou", "aux_dice", "aux_iou", "structure"):
        assert res[k].dtype == np.float64 and res[k].shape == (5,)
    assert res["dice"].tolist() == [2 * 3 / 9, 0.0, 0.0, 1.0, 0.0]
    assert res["iou"].tolist() == [3 / 6, 0.0, 0.0, 1.0, 0.0]
    assert res["aux_dice"].tolist() == [2 * 2 / 7, 0.0, 0.0, 0.0, 0.0]
    assert res["aux_iou"].tolist() == [2 / 5, 0.0, 0.0, 0.0, 0.0]
    assert not np.isnan(res["dice"]).any() and not np.isnan(res["aux_iou"]).any()
    assert res["empty"].dtype == np.bool_ and res["empty"].tolist() == [False, True, False, False, False]
    # per domain: against numpy on the images of that domain; domain 1 saw nothing and has no row
    assert sorted(res["per_domain"]) == [0, 2, 3]
    for d in (0, 2, 3):
        sel = np.array(domains) == d
        row = res["per_domain"][d]
        assert row["images"] == int(sel.sum())
        assert row["dice_mean"] == float(np.mean(res["dice"][sel])) and row["dice_std"] == float(np.std(res["dice"][sel]))
        assert row["iou_mean"] == float(np.mean(res["iou"][sel])) and row["iou_std"] == float(np.std(res["iou"][sel]))
        assert row["structure_loss"] == float(np.mean(structure[sel]))
    assert res["per_domain"][0]["dice_std"] == pytest.approx(1 / 3, abs=1e-15) and res["per_domain"][3]["dice_std"] == 0.0          # population std
    assert res["per_domain"][2]["structure_loss"] == 0.75
    assert res["sum_structure_loss"] == 1.25 + 0.75 + 4.0
    # without the structure column there is no structure key anywhere
    plain = scores_from_counts(counts, domains)
    assert "structure" not in plain and "sum_structure_loss" not in plain and "structure_loss" not in plain["per_domain"][0]
    none = scores_from_counts(np.zeros((0, 5), dtype=np.int64), [])
    assert none["dice"].shape == (0,) and none["per_domain"] == {}


def test_the_package_exports_the_report():
    import mdvit_amd
    assert mdvit_amd.ImageReport.__module__ == "mdvit_amd.report" and mdvit_amd.unpack_masks is unpack_masks
    with pytest.raises(ValueError):
        mdvit_amd.ImageReport(device="cpu")
