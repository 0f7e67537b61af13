"""ImageReport(postprocess=...) (mdvit_amd/report.py): the post-processing tables ride with the others -- evaluate() on canned logits of the committed
component cases gives scipy's columns, every key of a report without post-processing stays identical, a second epoch gives the same bytes, and a report that
grows past its capacity keeps its earlier rows."""
import numpy as np
import pytest
import torch

from mdvit_amd.evaluate import evaluate
from mdvit_amd.report import ImageReport, pack_masks, scores_from_counts
from test_components_host import expected, load_cases, names_of_size
from test_gpu_components import dev, logits_of

pytestmark = pytest.mark.gpu

D = 4
SIZE = (33, 45)
SPLIT = ((0, 3), (2, 3), (3, 2))          # (domain, images): the eight 33 x 45 cases in the fixture's order
PP_KEYS = {"pp_counts", "pp_dice", "pp_iou", "pp_aux_dice", "pp_aux_iou", "components", "largest_area", "filled", "removed", "pp_masks", "pp_aux_masks",
           "postprocess"}
PP_DOMAIN_KEYS = {"pp_dice_mean", "pp_dice_std", "pp_iou_mean", "pp_iou_std"}


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


@pytest.fixture(scope="module")
def canned():
    """the 33 x 45 cases as logits: image = [out, aux] stacked on the channel axis, so the `forward` given to evaluate() only splits it"""
    names = names_of_size(SIZE)
    assert len(names) == sum(k for _, k in SPLIT)
    cs = [load_cases()[n] for n in names]
    x = torch.stack([torch.stack([logits_of(c["pred"], 1 + i)[0], logits_of(c["aux"], 101 + i)[0]]) for i, c in enumerate(cs)])          # [8,2,H,W]
    y = torch.stack([torch.from_numpy(np.ascontiguousarray(c["label"])).float() for c in cs]).unsqueeze(1)
    loaders, r0 = {}, 0
    for d, k in SPLIT:
        loaders[f"set{d}"] = [(x[r0:r0 + k], y[r0:r0 + k], torch.full((k,), d, dtype=torch.long))]
        r0 += k
    model = torch.nn.Linear(1, 1).to(dev())          # evaluate() asks the model for its device and mode only
    forward = lambda img, dl, d: [img[:, :1].contiguous(), img[:, 1:2].contiguous()]
    return names, x.to(dev()), y.to(dev()), loaders, model, forward


def test_evaluate_with_postprocess_on_canned_logits(canned):
    names, _, _, loaders, model, forward = canned
    kw = dict(masks=True, aux_masks=True, boundary=True)
    rep = ImageReport(D, dev(), postprocess="fill_largest", **kw)
    a = evaluate(model, loaders, num_domains=D, forward=forward, report=rep)["report"]
    p = evaluate(model, loaders, num_domains=D, forward=forward, report=ImageReport(D, dev(), **kw))["report"]
    # every key of the same run without post-processing is present and equal
    assert set(a) == set(p) | PP_KEYS and not (set(p) & PP_KEYS)
    for k in p:
        if k == "per_domain":
            for d in p[k]:
                assert set(a[k][d]) == set(p[k][d]) | PP_DOMAIN_KEYS
                assert all(same(a[k][d][j], p[k][d][j]) for j in p[k][d])
        else:
            assert same(a[k], p[k]), k
    # the post-processing columns are scipy's
    exp = [expected(n, "fill_largest") for n in names]
    counts = np.array([e[0] for e in exp], dtype=np.int64)
    rows = np.array([e[1] for e in exp], dtype=np.int64)
    domains = [d for d, k in SPLIT for _ in range(k)]
    assert a["domain"].tolist() == domains and a["postprocess"] == "fill_largest" and a["size"] == SIZE
    assert a["pp_counts"].dtype == np.int64 and np.array_equal(a["pp_counts"], counts)
    for j, k in enumerate(("components", "largest_area", "filled", "removed")):
        assert a[k].dtype == np.int64 and np.array_equal(a[k], rows[:, :, j]), k
    assert np.array_equal(a["pp_masks"], pack_masks(np.stack([e[2] for e in exp]))) and a["pp_masks"].dtype == np.uint64
    assert np.array_equal(a["pp_aux_masks"], pack_masks(np.stack([e[3] for e in exp])))
    assert np.array_equal(a["masks"], pack_masks(np.stack([load_cases()[n]["pred"] for n in names])))          # the raw masks are still the raw masks
    ref = scores_from_counts(counts, domains)
    for k in ("dice", "iou", "aux_dice", "aux_iou"):
        assert np.array_equal(a["pp_" + k], ref[k]), k
    assert sorted(a["per_domain"]) == [0, 2, 3]
    for d, row in ref["per_domain"].items():
        for k in ("dice_mean", "dice_std", "iou_mean", "iou_std"):
            assert a["per_domain"][d]["pp_" + k] == row[k], (d, k)
    assert (a["filled"][:, :2].sum() > 0) and (a["removed"][:, :2].sum() > 0) and not a["filled"][:, 2].any() and not a["removed"][:, 2].any()
    # a second epoch with the same report (evaluate() resets it) gives the same bytes
    b = evaluate(model, loaders, num_domains=D, forward=forward, report=rep)["report"]
    assert set(a) == set(b)
    for k in a:
        assert str(a[k]) == str(b[k]) if k == "per_domain" else same(a[k], b[k]), k


@pytest.mark.parametrize("mode", ["fill", "largest"])
def test_a_report_that_grows_past_its_capacity_keeps_its_earlier_rows(canned, mode):
    names, x, y, _, _, _ = canned
    out, aux = x[:, :1].contiguous(), x[:, 1:2].contiguous()
    one = ImageReport(D, dev(), masks=True, aux_masks=True, capacity=8, postprocess=mode)
    one.update(out, aux, y, [1, 2], [3, 5])
    grown = ImageReport(D, dev(), masks=True, aux_masks=True, capacity=2, postprocess=mode)
    grown.update(out[:3], aux[:3], y[:3], 1)
    grown.update(out[3:4], aux[3:4], y[3:4], [2], [1])
    grown.update(out[4:], aux[4:], y[4:], [2, 2], [2, 2])
    assert grown._cap >= 8 and grown.rows == one.rows == 8
    a, b = one.result(), grown.result()
    assert set(a) == set(b)
    for k in a:
        assert str(a[k]) == str(b[k]) if k == "per_domain" else same(a[k], b[k]), k
    exp = [expected(n, mode) for n in names]
    assert np.array_equal(b["pp_counts"], np.array([e[0] for e in exp])) and np.array_equal(b["pp_masks"], pack_masks(np.stack([e[2] for e in exp])))
    assert np.array_equal(b["components"], np.array([e[1] for e in exp])[:, :, 0])
    # no auxiliary output in a forward: its cleaned masks are empty and set 1 is zeros
    grown.reset()
    grown.update(out[:2], None, y[:2], 0)
    c = grown.result()
    assert not c["pp_aux_masks"].any() and not c["components"][:, 1].any() and not c["pp_counts"][:, 3:].any()
    assert np.array_equal(c["pp_masks"], b["pp_masks"][:2])


def test_refusals_and_the_empty_report():
    with pytest.raises(ValueError, match="postprocess"):
        ImageReport(D, dev(), postprocess="connectivity=2")
    z = torch.zeros(1, 2, 8, 8, device=dev())
    with pytest.raises(ValueError, match="postprocess needs"):
        ImageReport(D, dev(), postprocess="fill").update(z, None, z, 1)
    big = torch.zeros(1, 1, 1025, 8, device=dev())
    with pytest.raises(ValueError, match="1024 x 1024"):
        ImageReport(D, dev(), postprocess="fill").update(big, None, big, 1)
    res = ImageReport(D, dev(), masks=True, postprocess="largest").result()
    assert res["pp_counts"].shape == (0, 5) and res["components"].shape == (0, 3) and res["postprocess"] == "largest" and res["pp_masks"].shape[0] == 0
    assert "pp_counts" not in ImageReport(D, dev(), masks=True).result()
