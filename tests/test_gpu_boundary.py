"""mdvit_eval_boundary (csrc/eval_boundary.hip) through ops.eval_boundary against the numpy restatement of tests/test_boundary_host.py (rows: integer for
integer; sums: 1e-10 relative -- at most 2^20 terms x 2^-53 of accumulation plus a correctly rounded fp64 sqrt) and against scipy's scores in the committed
fixture (1e-10 relative, through report.boundary_from_rows).  Logits are +-1 and +-30 with the sign from the mask.  No scipy here."""
import numpy as np
import pytest
import torch

from mdvit_amd import _lib, ops
from mdvit_amd.report import boundary_from_rows
from test_boundary_host import EMPTY, SCORES, case_names, load_cases, rel_close, restate, restated

pytestmark = pytest.mark.gpu

TIES = (1e-8, 6e-8)          # positive logits whose fp32 sigmoid rounds to 0.5: background (test_gpu_report.py's TIES)


def dev():
    return torch.device("cuda:0")


def logits_of(mask, seed=0, ties=False):
    """bool [H,W] -> fp32 logits [H,W]: +1 / +30 where set, -1 / -30 where not; with ties the first background pixels of every third row get a TIES value"""
    m = torch.from_numpy(np.ascontiguousarray(mask))
    big = torch.rand(m.shape, generator=torch.Generator().manual_seed(seed)) < 0.5
    x = torch.where(big, torch.tensor(30.0), torch.tensor(1.0)) * torch.where(m, torch.tensor(1.0), torch.tensor(-1.0))
    if ties:
        k = 0
        for y in range(0, m.shape[0], 3):
            for xx in torch.nonzero(~m[y])[:2, 0].tolist():
                x[y, xx] = TIES[k % 2]
                k += 1
        assert k > 4 and int((x > 0).sum()) == int(m.sum()) + k
    return x


def poison(*shape, dtype):
    t = torch.full(shape, float("nan"), dtype=torch.float64, device=dev())
    return t.view(torch.int64) if dtype == torch.int64 else t


POISON = int(torch.full((1,), float("nan"), dtype=torch.float64).view(torch.int64))


def run(preds, labels, auxs=None, ties=False):
    """lists of bool masks of one size -> (rows [n,2,6] int64, sums [n,2,2] float64) on the host; two runs on poisoned outputs, bit-identical"""
    n, (H, W) = len(preds), preds[0].shape
    out = torch.stack([logits_of(m, 1 + i, ties) for i, m in enumerate(preds)]).view(n, 1, H, W).to(dev())
    label = torch.stack([torch.from_numpy(np.ascontiguousarray(m)).float() for m in labels]).view(n, 1, H, W).to(dev())
    aux = None if auxs is None else torch.stack([logits_of(m, 101 + i) for i, m in enumerate(auxs)]).view(n, 1, H, W).to(dev())
    ws = torch.empty((ops.eval_boundary_ws_bytes(n, H, W) // 8,), dtype=torch.int64, device=dev())
    got = []
    for _ in range(2):
        rows, sums = poison(n, 2, 6, dtype=torch.int64), poison(n, 2, 2, dtype=torch.float64)
        ops.eval_boundary(out, aux, label, rows, sums, ws)
        got.append((rows.cpu(), sums.cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1].view(torch.int64), got[1][1].view(torch.int64))          # bit-reproducible
    rows, sums = got[0][0].numpy(), got[0][1].numpy()
    assert not (rows == POISON).any() and not np.isnan(sums).any()          # every element written
    return rows, sums


def check(name, row, sm, want):
    print(f"{name}: rows {row.tolist()} want {want['row']}; sums {sm.tolist()} want {want['sums']}")
    assert row.tolist() == want["row"], name
    for k in range(2):
        assert rel_close(float(sm[k]), want["sums"][k], 1e-10), (name, k, float(sm[k]), want["sums"][k])


def check_scores(name, res, i, pre, fixture_case):
    for s in SCORES:
        got, ref = float(res[pre + s][i]), fixture_case[s]
        if name in EMPTY:
            assert np.isnan(got) and np.isnan(ref) and not res[pre + "boundary_valid"][i]
        else:
            assert res[pre + "boundary_valid"][i] and rel_close(got, ref, 1e-10), (name, s, got, ref)


SINGLE = [n for n in case_names() if not n.endswith("512x512")]


@pytest.mark.parametrize("name", SINGLE)
def test_one_image_without_aux(name):
    """n = 1, aux None: rows and sums of output 0 against the restatement, the scores against scipy's; the rows of output 1 are zeros"""
    c = load_cases()[name]
    rows, sums = run([c["pred"]], [c["label"]], ties=name.startswith("tie"))
    check(name, rows[0, 0], sums[0, 0], restated(name))
    assert not rows[0, 1].any() and not sums[0, 1].any()
    res = boundary_from_rows(rows, sums, [0])
    check_scores(name, res, 0, "", c)
    assert not res["aux_boundary_valid"][0] and np.isnan(res["aux_hd95"][0])
    if name.startswith("identical"):
        assert rows[0, 0, 2:].tolist() == [0, 0, 0, 0] and sums[0, 0].tolist() == [0.0, 0.0] and rows[0, 0, 0] == rows[0, 0, 1] > 0


def batch_check(names):
    """one call over the cases `names` (one size) with aux given: image i's auxiliary output is the prediction of image i + 1.  Every image differs, so a row
    from another image's data would show."""
    cs = [load_cases()[n] for n in names]
    n = len(cs)
    auxs = [cs[(i + 1) % n]["pred"] for i in range(n)]
    rows, sums = run([c["pred"] for c in cs], [c["label"] for c in cs], auxs)
    res = boundary_from_rows(rows, sums, [0] * n)
    for i, name in enumerate(names):
        check(name, rows[i, 0], sums[i, 0], restated(name))
        check_scores(name, res, i, "", cs[i])
        want = restate(auxs[i], cs[i]["label"])
        check(name + " aux", rows[i, 1], sums[i, 1], want)
        for s in SCORES:
            got = float(res["aux_" + s][i])
            assert (np.isnan(got) and not want["valid"]) or rel_close(got, want[s], 1e-10), (name, s)
    return rows, res


def test_nine_different_images_with_aux():
    names = ["random0.02_33x45", "empty_pred_33x45", "random0.3_33x45", "checker_33x45", "empty_label_33x45", "blobs_33x45", "both_empty_33x45",
             "corners_33x45", "edges_33x45"]
    rows, res = batch_check(names)
    assert len({tuple(r) for r in rows[:, 0].tolist()}) == 9
    assert np.isnan(res["hd95"]).tolist() == [n in EMPTY for n in names]          # the only NaN rows are the three designated empty cases
    assert res["boundary_valid"].tolist() == [n not in EMPTY for n in names]


def test_two_512x512_images_with_aux():
    batch_check(["disks_512x512", "ring_512x512"])


def test_refusals_come_before_any_launch():
    H, W = 20, 37
    out, label = torch.randn(2, 1, H, W, device=dev()), torch.ones(2, 1, H, W, device=dev())
    ws = torch.empty((ops.eval_boundary_ws_bytes(2, H, W) // 8,), dtype=torch.int64, device=dev())
    rows, sums = poison(2, 2, 6, dtype=torch.int64), poison(2, 2, 2, dtype=torch.float64)
    E = _lib.MdvitHipError
    tall = torch.zeros(1, 1, 1025, 4, device=dev())
    with pytest.raises(E, match="1..1024"):
        ops.eval_boundary(tall, None, tall, rows[:1], sums[:1], ws)
    with pytest.raises(E, match="workspace"):
        ops.eval_boundary(out, None, label, rows, sums, ws[:-1])
    with pytest.raises(E, match="rows"):
        ops.eval_boundary(out, None, label, rows.view(torch.float64), sums, ws)
    with pytest.raises(E, match="rows"):
        ops.eval_boundary(out, None, label, rows.view(2, 12), sums, ws)
    with pytest.raises(E, match="sums"):
        ops.eval_boundary(out, None, label, rows, sums.float(), ws)
    with pytest.raises(E, match="sums"):
        ops.eval_boundary(out, None, label, rows, sums.view(2, 4), ws)
    with pytest.raises(E, match=r"\[n,1,H,W\]"):
        ops.eval_boundary(out.view(1, 2, H, W), None, label.view(1, 2, H, W), rows[:1], sums[:1], ws)          # multi-channel logits
    with pytest.raises(E, match=r"\[n,1,H,W\]"):
        ops.eval_boundary(torch.cat([out, out], 1), None, torch.cat([label, label], 1), rows, sums, ws)
    assert ops.eval_boundary_ws_bytes(1, 1025, 4) == 0
    torch.cuda.synchronize()
    assert bool((rows == POISON).all()) and bool(torch.isnan(sums).all())          # nothing was enqueued
    ops.eval_boundary(out.view(2, H, W), None, label.view(2, H, W), rows, sums, ws)          # [n,H,W] is accepted
    torch.cuda.synchronize()
    assert not bool((rows == POISON).any()) and not bool(torch.isnan(sums).any())
