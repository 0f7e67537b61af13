"""Connected-component post-processing without a GPU: a pure-numpy restatement (min-label propagation along runs; fill, largest, the three modes and the rows
table derived from it) against the committed scipy results (tests/golden/components_cases.npz, tools/make_components_golden.py), the host functions of
mdvit_amd/report.py, the workspace queries and every refusal of mdvit_eval_components / mdvit_label_components.  The GPU tests import the restatement and
the fixture reader from here; nothing in this file imports scipy.  Everything is an integer: every comparison is exact equality."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "components_cases.npz")
MODES = ("fill", "largest", "fill_largest")
SETS = ("pred", "aux", "label")
SIZES = [(1, 70), (70, 1), (33, 45), (64, 64), (37, 130), (128, 192), (264, 300)]
LABELLED = SIZES[:5]          # the sizes whose full label images are stored


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _run_min(lab, m):
    """every set pixel takes the minimum label of its horizontal run"""
    H, W = m.shape
    prev = np.zeros_like(m)
    prev[:, 1:] = m[:, :-1]
    ids = (np.cumsum((m & ~prev).ravel()) - 1).reshape(H, W)[m]
    if ids.size == 0:
        return lab
    buf = np.full(int(ids.max()) + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(buf, ids, lab[m])
    out = lab.copy()
    out[m] = buf[ids]
    return out


def root_labels(mask):
    """bool [H,W] -> int64 [H,W]: 1 + the flat row-major index of the first pixel of the pixel's 4-connected component, 0 for background.  Min-label
    propagation: every pixel starts with its own index + 1; minima over horizontal runs and over vertical runs alternate until nothing changes."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    lab = np.where(m, 1 + np.arange(H * W, dtype=np.int64).reshape(H, W), 0)
    while True:
        new = _run_min(lab, m)
        new = np.ascontiguousarray(_run_min(np.ascontiguousarray(new.T), np.ascontiguousarray(m.T)).T)
        if np.array_equal(new, lab):
            return lab
        lab = new


def renumber(roots):
    """root labels -> labels 1..K by rank (scipy.ndimage.label's numbers: components in the order of their first pixel) and the areas [K] in that order"""
    r = np.asarray(roots).astype(np.int64)
    u, inv, cnt = np.unique(r.ravel(), return_inverse=True, return_counts=True)
    if len(u) and u[0] == 0:
        return inv.reshape(r.shape), cnt[1:]
    return inv.reshape(r.shape) + 1, cnt


def fill(mask):
    """M | every 4-connected component of ~M that touches none of the four image edges"""
    m = np.asarray(mask, dtype=bool)
    r = root_labels(~m)
    edge = np.unique(np.concatenate([r[0], r[-1], r[:, 0], r[:, -1]]))
    return m | (~m & ~np.isin(r, edge))


def largest(mask):
    """the component with the most pixels, ties to the smallest root label; an empty mask stays empty"""
    m = np.asarray(mask, dtype=bool)
    r = root_labels(m)
    u, cnt = np.unique(r[m], return_counts=True)
    if len(u) == 0:
        return m.copy()
    return r == u[int(np.argmax(cnt))]          # argmax: the first maximum, and u ascends


def clean(mask, mode):
    if mode == "fill":
        return fill(mask)
    if mode == "largest":
        return largest(mask)
    if mode == "fill_largest":
        return largest(fill(mask))
    raise ValueError(mode)


def row_of(raw, mode, cleaned=None, filled=None):
    """mdvit_eval_components' row of one (image, set): components and largest area of the RAW mask, pixels the fill step set, pixels the largest step
    cleared.  cleaned None: the label's row (counted, never cleaned).  filled: fill(raw), needed for "fill_largest" only."""
    raw = np.asarray(raw, dtype=bool)
    _, areas = renumber(root_labels(raw))
    row = [len(areas), int(areas.max()) if len(areas) else 0, 0, 0]
    if cleaned is not None:
        n_raw, n_clean = int(raw.sum()), int(np.asarray(cleaned).sum())
        if mode == "fill":
            row[2] = n_clean - n_raw
        elif mode == "largest":
            row[3] = n_raw - n_clean
        else:
            n_fill = int(np.asarray(filled).sum())
            row[2], row[3] = n_fill - n_raw, n_fill - n_clean
    return row


def counts_of(pred_clean, aux_clean, label):
    """mdvit_eval_images' five columns on cleaned masks (aux_clean None: zeros)"""
    y = np.asarray(label, dtype=bool)
    a = np.asarray(pred_clean, dtype=bool)
    c = [int((a & y).sum()), int(a.sum()), int(y.sum()), 0, 0]
    if aux_clean is not None:
        b = np.asarray(aux_clean, dtype=bool)
        c[3], c[4] = int((b & y).sum()), int(b.sum())
    return c


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
_cache = {}


def load_cases():
    """{name: {"size", "pred" / "aux" / "label" bool [H,W], "areas_<set>" int64, "<mode>_pred" / "<mode>_aux" bool [H,W], "labels_<set>" int64 [H,W] where
    stored}} in the file's order, read once and never changed"""
    if "cases" not in _cache:
        z = np.load(GOLDEN, allow_pickle=False)
        cases = {}
        for k, name in enumerate(z["names"].tolist()):
            H, W = (int(v) for v in z["sizes"][k])
            un = lambda a: np.unpackbits(a)[:H * W].reshape(H, W).astype(bool)
            c = {"size": (H, W)}
            for s in SETS:
                c[s] = un(z[f"{s}_{k}"])
                c["areas_" + s] = z[f"areas_{s}_{k}"].astype(np.int64)
                if f"labels_{s}_{k}" in z.files:
                    c["labels_" + s] = z[f"labels_{s}_{k}"].astype(np.int64)
            for s in SETS[:2]:
                for mode in MODES:
                    c[f"{mode}_{s}"] = un(z[f"{mode}_{s}_{k}"])
            cases[name] = c
        _cache["cases"] = cases
    return _cache["cases"]


def case_names():
    return list(load_cases())


def names_of_size(size):
    return [n for n, c in load_cases().items() if c["size"] == tuple(size)]


def expected(name, mode, with_aux=True):
    """scipy's answer for one fixture case: (counts [5], rows [3][4], cleaned pred, cleaned aux or None)"""
    c = load_cases()[name]
    rows = []
    for s in SETS:
        areas = c["areas_" + s]
        row = [len(areas), int(areas.max()) if len(areas) else 0, 0, 0]
        if s != "label":
            n_raw, n_clean, n_fill = int(c[s].sum()), int(c[f"{mode}_{s}"].sum()), int(c[f"fill_{s}"].sum())
            if mode == "fill":
                row[2] = n_clean - n_raw
            elif mode == "largest":
                row[3] = n_raw - n_clean
            else:
                row[2], row[3] = n_fill - n_raw, n_fill - n_clean
        rows.append(row)
    if not with_aux:
        rows[1] = [0, 0, 0, 0]
    aux_clean = c[f"{mode}_aux"] if with_aux else None
    return counts_of(c[f"{mode}_pred"], aux_clean, c["label"]), rows, c[f"{mode}_pred"], aux_clean


SLOW = (264, 300)          # the restatement leaves this size out (a spiral of 150 turns); the fixture still pins it for the device


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_small_and_holds_the_listed_sizes_and_patterns():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    cases = load_cases()
    assert sorted({c["size"] for c in cases.values()}) == sorted(SIZES)
    for name, c in cases.items():
        assert ("labels_pred" in c) == (c["size"] in LABELLED), name
    pats = {p for n in cases for p in n.rsplit("_", 1)[0].split("+")}
    assert pats >= {"empty", "full", "single", "checker", "spiral", "spiral_complement", "comb", "rings", "diag_ring", "gap_ring", "ties", "seam", "noise", "lesion"}
    aux_pats = {n.split("+")[1] for n in cases}
    assert {"empty", "ties"} <= aux_pats          # empty inputs and ties for the auxiliary output too
    # what the patterns are there for
    chk = cases["checker+spiral+full_33x45"]
    assert len(chk["areas_pred"]) == (33 * 45 + 1) // 2 and len(chk["areas_aux"]) == 1 and np.array_equal(chk["fill_aux"], chk["aux"])
    rg = cases["rings+seam+lesion_37x130"]
    assert len(rg["areas_pred"]) == 4 and rg["fill_pred"].all() and not np.array_equal(rg["largest_pred"], rg["fill_largest_pred"])
    tie = cases["ties+rings+ties_33x45"]
    assert tie["areas_pred"].tolist() == [24, 24, 6] and tie["largest_pred"].sum() == 24 and tie["largest_pred"][3, 45 - 9]
    dg = cases["diag_ring+gap_ring+rings_33x45"]
    assert len(dg["areas_pred"]) == 3 and dg["fill_pred"][3:-3, 3:-3].all() and not dg["fill_aux"][4, 3]


# ---- 2. the restatement against scipy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in case_names() if load_cases()[n]["size"] != SLOW])
def test_restatement_equals_scipy(name):
    c = load_cases()[name]
    for s in SETS:
        roots = root_labels(c[s])
        lab, areas = renumber(roots)
        assert np.array_equal(areas, c["areas_" + s]), s
        if "labels_" + s in c:
            assert np.array_equal(lab, c["labels_" + s]), s
        assert np.array_equal(roots != 0, c[s])
        first = np.unique(roots[roots > 0]) - 1          # a root label points at a set pixel that carries it
        assert (roots.ravel()[first] == first + 1).all()
    for mode in MODES:
        want_counts, want_rows, want_pred, want_aux = expected(name, mode)
        got = {s: clean(c[s], mode) for s in SETS[:2]}
        assert np.array_equal(got["pred"], want_pred) and np.array_equal(got["aux"], want_aux), mode
        rows = [row_of(c[s], mode, got[s], fill(c[s])) for s in SETS[:2]] + [row_of(c["label"], mode)]
        assert rows == want_rows, mode
        assert counts_of(got["pred"], got["aux"], c["label"]) == want_counts


# ---- 3. report.py's host functions ----------------------------------------------------------------------------------------------
def test_postprocess_mode():
    from mdvit_amd.report import postprocess_mode
    assert [postprocess_mode(m) for m in MODES] == [1, 2, 3]
    for bad in ("", "Fill", "fill_largest ", "largest_fill", "connectivity=2", None, 2, b"fill"):
        with pytest.raises(ValueError, match="postprocess"):
            postprocess_mode(bad)


def test_pp_columns_are_scores_from_counts_on_the_cleaned_counts():
    from mdvit_amd.report import postprocess_from_rows, scores_from_counts
    names = names_of_size((33, 45))[:6]
    domains = [0, 0, 2, 1, 2, 0]
    exp = [expected(n, "fill_largest") for n in names]
    counts = np.array([e[0] for e in exp] + [[0, 0, 0, 0, 0]], dtype=np.int64)          # the last image: 0/0 -> 0
    rows = np.array([e[1] for e in exp] + [[[0] * 4] * 3], dtype=np.int64)
    domains.append(1)
    res = postprocess_from_rows(counts, rows, domains)
    ref = scores_from_counts(counts, domains)
    assert set(res) == {"pp_counts", "pp_dice", "pp_iou", "pp_aux_dice", "pp_aux_iou", "components", "largest_area", "filled", "removed", "per_domain"}
    assert np.array_equal(res["pp_counts"], counts) and res["pp_counts"].dtype == np.int64
    for k in ("dice", "iou", "aux_dice", "aux_iou"):
        assert np.array_equal(res["pp_" + k], ref[k]), k
    assert res["pp_dice"][-1] == 0.0 and res["pp_aux_iou"][-1] == 0.0
    for j, k in enumerate(("components", "largest_area", "filled", "removed")):
        assert res[k].shape == (7, 3) and res[k].dtype == np.int64 and np.array_equal(res[k], rows[:, :, j])
    assert sorted(res["per_domain"]) == [0, 1, 2]
    for d, row in res["per_domain"].items():
        assert set(row) == {"pp_dice_mean", "pp_dice_std", "pp_iou_mean", "pp_iou_std"}
        for k in row:
            assert row[k] == ref["per_domain"][d][k[3:]]
    assert res["per_domain"][0]["pp_dice_std"] > 0
    none = postprocess_from_rows(np.zeros((0, 5), dtype=np.int64), np.zeros((0, 3, 4), dtype=np.int64), [])
    assert none["components"].shape == (0, 3) and none["per_domain"] == {}


def test_scores_from_counts_is_unchanged_by_the_postprocess_columns():
    from mdvit_amd.report import scores_from_counts
    res = scores_from_counts(np.array([[3, 4, 5, 0, 0], [0, 0, 0, 0, 0]]), [1, 1])
    assert set(res) == {"domain", "counts", "dice", "iou", "aux_dice", "aux_iou", "empty", "per_domain"}
    assert set(res["per_domain"][1]) == {"images", "dice_mean", "dice_std", "iou_mean", "iou_std"}


# ---- 4. the workspace queries and the refusals ----------------------------------------------------------------------------------
def test_workspace_queries():
    from mdvit_amd import _lib, ops
    lib = _lib.load()
    for n, H, W in ((1, 1, 1), (9, 33, 45), (16, 512, 512), (65535, 1024, 1024)):
        words = H * ((W + 63) // 64)
        got = lib.mdvit_eval_components_ws_bytes(n, H, W)
        # at least the three raw, two complement and two filled planes and an int32 label per pixel of the five planes one pass labels
        assert got >= n * (7 * 8 * words + 5 * 4 * H * W) and got % 8 == 0, (n, H, W, got)
        assert ops.eval_components_ws_bytes(n, H, W) == got
        one = lib.mdvit_label_components_ws_bytes(n, H, W)
        assert n * (8 * words + 4 * H * W) <= one < got and one % 8 == 0, (n, H, W, one)
        assert ops.label_components_ws_bytes(n, H, W) == one
    assert lib.mdvit_eval_components_ws_bytes(65535, 1024, 1024) > 1 << 40          # no 32-bit overflow at the largest size
    for n, H, W in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 1025), (1, 1025, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.mdvit_eval_components_ws_bytes(n, H, W) == 0 and lib.mdvit_label_components_ws_bytes(n, H, W) == 0, (n, H, W)


def test_every_refusal_returns_its_code_without_a_gpu():
    """argument validation happens before any HIP call.  The pointers are made-up addresses: a refused call never touches them."""
    import ctypes as C
    from mdvit_amd import _lib
    lib = _lib.load()
    SHAPE, ALIGN, WORKSPACE = 1, 3, 4          # MDVIT_E_SHAPE, MDVIT_E_ALIGN, MDVIT_E_WORKSPACE
    p = lambda a: C.c_void_p(a)
    n, H, W = 2, 20, 37
    need = lib.mdvit_eval_components_ws_bytes(n, H, W)
    ok = dict(out=p(4096), aux=p(8192), label=p(12288), n=n, H=H, W=W, mode=3, counts=p(16384), rows=p(20480), bits=p(24576), aux_bits=p(28672), ws=p(1 << 20),
              ws_bytes=need)

    def ec(**kw):
        a = dict(ok, **kw)
        return lib.mdvit_eval_components(a["out"], a["aux"], a["label"], a["n"], a["H"], a["W"], a["mode"], a["counts"], a["rows"], a["bits"], a["aux_bits"],
                                         a["ws"], a["ws_bytes"], None)

    for kw in (dict(out=None), dict(label=None), dict(counts=None), dict(rows=None), dict(n=0), dict(n=65536), dict(H=0), dict(H=1025), dict(W=0), dict(W=1025),
               dict(mode=0), dict(mode=4), dict(mode=-1), dict(aux=None)):          # the last: aux_bits without aux
        assert ec(**kw) == SHAPE, kw
        assert b"eval_components" in lib.mdvit_last_error()
    assert ec(mode=4) == SHAPE and b"mode" in lib.mdvit_last_error()
    assert ec(aux=None) == SHAPE and b"aux_bits without aux" in lib.mdvit_last_error()
    for kw in (dict(counts=p(16388)), dict(rows=p(20484)), dict(bits=p(24580)), dict(aux_bits=p(28676)), dict(ws=p((1 << 20) + 4)), dict(out=p(4097))):
        assert ec(**kw) == ALIGN, kw
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None)):
        assert ec(**kw) == WORKSPACE, kw
        assert b"workspace" in lib.mdvit_last_error()

    need1 = lib.mdvit_label_components_ws_bytes(n, H, W)
    ok1 = dict(masks=p(4096), n=n, H=H, W=W, labels=p(8192), components=p(12288), ws=p(1 << 20), ws_bytes=need1)

    def lc(**kw):
        a = dict(ok1, **kw)
        return lib.mdvit_label_components(a["masks"], a["n"], a["H"], a["W"], a["labels"], a["components"], a["ws"], a["ws_bytes"], None)

    for kw in (dict(masks=None), dict(labels=None), dict(n=0), dict(n=65536), dict(H=0), dict(H=1025), dict(W=0), dict(W=1025)):
        assert lc(**kw) == SHAPE, kw
        assert b"label_components" in lib.mdvit_last_error()
    for kw in (dict(labels=p(8194)), dict(components=p(12292)), dict(ws=p((1 << 20) + 4))):
        assert lc(**kw) == ALIGN, kw
    for kw in (dict(ws_bytes=need1 - 1), dict(ws=None)):
        assert lc(**kw) == WORKSPACE, kw
