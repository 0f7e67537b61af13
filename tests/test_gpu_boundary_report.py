"""ImageReport(boundary=True) (mdvit_amd/report.py): the boundary columns ride with the other tables -- growth and offsets, the keys a report without them
returns stay identical, the packed masks and the metric agree by construction, update() does not synchronise, and evaluate(report=...) on the committed eval
fixture gives the columns of the restatement (tests/test_boundary_host.py) applied to the unpacked masks."""
import numpy as np
import pytest
import torch

from mdvit_amd.evaluate import evaluate
from mdvit_amd.report import ImageReport, unpack_masks
from test_boundary_host import SCORES, restate
from test_gpu_evaluate import D, dev, fixture_batches
from test_gpu_report import tie_case

pytestmark = pytest.mark.gpu

BOUNDARY_KEYS = [pre + s for pre in ("", "aux_") for s in SCORES + ("boundary_valid",)] + ["boundary_rows"]
DOMAIN_KEYS = ("hd95_mean", "hd95_std", "assd_mean", "assd_std", "boundary_images")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


def check_against_masks(res, label):
    """every boundary column of `res` from its own packed masks: restate(unpacked mask, label) per image, rows integer for integer, scores to 1e-10"""
    y = (label.reshape(label.shape[0], *res["size"]) != 0).cpu().numpy()
    for pre, key, o in (("", "masks", 0), ("aux_", "aux_masks", 1)):
        m = unpack_masks(res[key], res["size"]).astype(bool)
        for i in range(len(m)):
            want = restate(m[i], y[i])
            assert res["boundary_rows"][i, o].tolist() == want["row"], (pre, i)
            assert bool(res[pre + "boundary_valid"][i]) == want["valid"]
            for s in SCORES:
                got = float(res[pre + s][i])
                assert (np.isnan(got) and not want["valid"]) or abs(got - want[s]) <= 1e-10 * abs(want[s]), (pre, i, s, got, want[s])
    for d, row in res["per_domain"].items():
        sel = (res["domain"] == d) & res["boundary_valid"]
        assert row["boundary_images"] == int(sel.sum())
        if sel.any():
            assert row["hd95_mean"] == float(res["hd95"][sel].mean()) and row["hd95_std"] == float(res["hd95"][sel].std())
            assert row["assd_mean"] == float(res["assd"][sel].mean()) and row["assd_std"] == float(res["assd"][sel].std())
        else:
            assert all(np.isnan(row[k]) for k in DOMAIN_KEYS[:4])


def test_three_updates_from_capacity_two_equal_one_update_and_the_old_keys_stay():
    images, H, W = (3, 1, 5), 20, 37
    out, aux, label = (t.to(dev()) for t in tie_case(29, images, H, W))
    kw = dict(masks=True, aux_masks=True, structure=True)
    one = ImageReport(D, dev(), capacity=9, boundary=True, **kw)
    one.update(out, aux, label, [2, 0, 3], list(images))
    grown = ImageReport(D, dev(), capacity=2, boundary=True, **kw)
    grown.update(out[:3], aux[:3], label[:3], 2)
    grown.update(out[3:4], aux[3:4], label[3:4], [0], [1])
    grown.update(out[4:], aux[4:], label[4:], [3, 3], [2, 3])
    plain = ImageReport(D, dev(), capacity=9, **kw)
    plain.update(out, aux, label, [2, 0, 3], list(images))
    assert grown._cap >= 9 and grown.rows == one.rows == 9
    a, b, p = one.result(), grown.result(), plain.result()
    assert set(a) == set(b) == set(p) | set(BOUNDARY_KEYS)
    for k in a:
        if k != "per_domain":
            assert same(a[k], b[k]), k
    assert str(a["per_domain"]) == str(b["per_domain"])
    for k in p:          # the keys of a report without boundary columns: identical values
        if k == "per_domain":
            for d in p[k]:
                assert set(a[k][d]) == set(p[k][d]) | set(DOMAIN_KEYS)
                assert all(a[k][d][j] == p[k][d][j] for j in p[k][d])
        else:
            assert same(a[k], p[k]), k
    assert a["boundary_rows"].shape == (9, 2, 6) and a["boundary_rows"].dtype == np.int64
    assert a["boundary_valid"].all() and len({tuple(r) for r in a["boundary_rows"][:, 0].tolist()}) == 9          # a row at a wrong offset would show
    check_against_masks(a, label)          # the masks and the metric agree by construction, ties included


def test_refusals():
    out, aux, label = (t.to(dev()) for t in tie_case(31, (2,), 20, 37))
    with pytest.raises(ValueError, match="boundary=True needs"):
        ImageReport(D, dev(), boundary=True).update(out.view(1, 2, 20, 37), None, label.view(1, 2, 20, 37), 1)
    big = torch.zeros(1, 1, 1025, 8, device=dev())
    with pytest.raises(ValueError, match="1024 x 1024"):
        ImageReport(D, dev(), boundary=True).update(big, None, big, 1)
    rep = ImageReport(D, dev(), boundary=True)
    rep.update(out.view(2, 20, 37), None, label.view(2, 20, 37), 1)          # [B,H,W] is accepted; no auxiliary output: invalid aux columns
    res = rep.result()
    assert res["boundary_valid"].all() and not res["aux_boundary_valid"].any() and np.isnan(res["aux_hd95"]).all() and not res["boundary_rows"][:, 1].any()
    assert ImageReport(D, dev(), boundary=True).result()["boundary_rows"].shape == (0, 2, 6)


def test_update_does_not_synchronise():
    out, aux, label = (t.to(dev()) for t in tie_case(41, (3, 1, 5), 20, 37))
    rep = ImageReport(D, dev(), masks=True, aux_masks=True, structure=True, boundary=True, capacity=4)
    rep.update(out, aux, label, [0, 1, 2], [3, 1, 5])          # first use: code objects loaded outside the checked window
    rep.reset()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rep.update(out, aux, label, [0, 1, 2], [3, 1, 5])
        rep.update(out[:3], None, label[:3], 3)
        rep.update(out, aux, label, [0, 1, 2], [3, 1, 5])          # 21 rows: the tables grow inside the window too
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    res = rep.result()
    assert np.array_equal(res["boundary_rows"][:9], res["boundary_rows"][12:]) and same(res["hd95"][:9], res["hd95"][12:])
    assert not res["boundary_rows"][9:12, 1].any() and res["boundary_valid"].all()


@pytest.fixture(scope="module")
def fixture_model(golden):
    return fixture_batches(golden)


def test_evaluate_with_boundary_columns_on_the_eval_fixture(fixture_model):
    model, data = fixture_model
    model.eval()
    loaders = {f"set{d}": [data[d][:3]] for d in (0, 3)}
    got = {}
    for fuse in (False, True):
        rep = ImageReport(D, dev(), masks=True, aux_masks=True, boundary=True)
        got[fuse] = evaluate(model, loaders, num_domains=D, fuse_domains=fuse, report=rep)["report"]
    a, b = got[False], got[True]
    label = torch.cat([data[d][1] for d in (0, 3)])
    check_against_masks(a, label)
    check_against_masks(b, label)
    assert same(a["domain"], b["domain"])
    for key, keys in (("masks", BOUNDARY_KEYS[:6] + ["boundary_rows"]), ("aux_masks", BOUNDARY_KEYS[6:12])):
        if same(a[key], b[key]):          # the fused forward thresholds the same pixels: the same columns, bit for bit
            for k in keys:
                assert same(a[k] if k != "boundary_rows" else a[k][:, 0], b[k] if k != "boundary_rows" else b[k][:, 0]), k
    assert sorted(a["per_domain"]) == [0, 3] and all(k in a["per_domain"][0] for k in DOMAIN_KEYS)
