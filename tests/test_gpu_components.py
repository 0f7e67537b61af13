"""mdvit_label_components / mdvit_eval_components (csrc/eval_components.hip) through ops against scipy's results in the committed fixture
(tests/golden/components_cases.npz): labels, areas, counts, rows and the cleaned masks, integer for integer.  Logits are +-1 and +-30 with the sign from the
mask, and some background pixels carry a tiny positive logit whose sigmoid rounds to 0.5 (background).  No scipy here."""
import numpy as np
import pytest
import torch

from mdvit_amd import _lib, ops
from mdvit_amd.report import pack_masks, postprocess_mode
from test_components_host import MODES, SETS, SIZES, case_names, expected, load_cases, names_of_size, renumber

pytestmark = pytest.mark.gpu

TIES = (1e-8, 6e-8)          # positive logits whose fp32 sigmoid rounds to 0.5: background (test_gpu_boundary.py's TIES)
POISON = int(torch.full((1,), float("nan"), dtype=torch.float64).view(torch.int64))


def dev():
    return torch.device("cuda:0")


def logits_of(mask, seed=0, ties=True):
    """bool [H,W] -> fp32 logits [H,W] (test_gpu_boundary.py's logits_of): +1 / +30 where set, -1 / -30 where not; with ties the first two background pixels
    of every third row get a TIES value.  Returns the logits and the number of tie pixels."""
    m = torch.from_numpy(np.ascontiguousarray(mask))
    big = torch.rand(m.shape, generator=torch.Generator().manual_seed(seed)) < 0.5
    x = torch.where(big, torch.tensor(30.0), torch.tensor(1.0)) * torch.where(m, torch.tensor(1.0), torch.tensor(-1.0))
    k = 0
    if ties:
        for y in range(0, m.shape[0], 3):
            for xx in torch.nonzero(~m[y])[:2, 0].tolist():
                x[y, xx] = TIES[k % 2]
                k += 1
    assert int((x > 0).sum()) == int(m.sum()) + k
    return x, k


def poison(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=dev()).view(torch.int64)


def run(preds, labels, auxs, mode):
    """lists of bool masks of one size -> counts [n,5], rows [n,3,4], bits, aux_bits (None without aux) on the host; two calls on poisoned outputs, byte-identical"""
    n, (H, W) = len(preds), preds[0].shape
    words = (H * W + 63) // 64
    lg = [logits_of(m, 1 + i) for i, m in enumerate(preds)]
    out = torch.stack([x for x, _ in lg]).view(n, 1, H, W).to(dev())
    label = torch.stack([torch.from_numpy(np.ascontiguousarray(m)).float() for m in labels]).view(n, 1, H, W).to(dev())
    aux = None if auxs is None else torch.stack([logits_of(m, 101 + i)[0] for i, m in enumerate(auxs)]).view(n, 1, H, W).to(dev())
    ws = torch.empty((ops.eval_components_ws_bytes(n, H, W) // 8,), dtype=torch.int64, device=dev())
    got = []
    for _ in range(2):
        ws.fill_(POISON)          # the entry relies on nothing a previous call left behind
        counts, rows, bits = poison(n, 5), poison(n, 3, 4), poison(n, words)
        aux_bits = None if auxs is None else poison(n, words)
        ops.eval_components(out, aux, label, postprocess_mode(mode), counts, rows, ws, bits, aux_bits)
        got.append([None if t is None else t.cpu() for t in (counts, rows, bits, aux_bits)])
    for a, b in zip(*got):
        assert (a is None and b is None) or torch.equal(a, b)          # bit-reproducible
    counts, rows, bits, aux_bits = (None if t is None else t.numpy() for t in got[0])
    assert not (counts == POISON).any() and not (rows == POISON).any() and not (bits == POISON).any()          # every element written
    return counts, rows, bits, aux_bits, sum(k for _, k in lg)


def check(name, mode, counts, rows, bits, aux_bits, with_aux):
    want_counts, want_rows, want_pred, want_aux = expected(name, mode, with_aux)
    print(f"{name} {mode}: counts {counts.tolist()} want {want_counts}; rows {rows.tolist()} want {want_rows}")
    assert counts.tolist() == want_counts, (name, mode)
    assert rows.tolist() == want_rows, (name, mode)
    assert np.array_equal(bits.view(np.uint64), pack_masks(want_pred[None])[0]), (name, mode)
    if with_aux:
        assert np.array_equal(aux_bits.view(np.uint64), pack_masks(want_aux[None])[0]), (name, mode)


# ---- 1. the labelling alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_label_components_equals_scipy(name):
    """pred, aux and label of the case as three images of one call: root labels renumbered by rank are scipy's labels (where stored), their bincount is scipy's
    areas, the count is the areas' length; a root label is 1 + the flat index of a pixel that carries it"""
    c = load_cases()[name]
    masks = torch.from_numpy(np.stack([c[s] for s in SETS])).to(dev())
    comps = poison(3)
    roots = ops.label_components(masks, comps).cpu().numpy()
    again = ops.label_components(masks.to(torch.uint8) * 7).cpu().numpy()          # any nonzero byte is set; bit-reproducible
    assert roots.dtype == np.int32 and np.array_equal(roots, again)
    for i, s in enumerate(SETS):
        lab, areas = renumber(roots[i])
        assert np.array_equal(roots[i] != 0, c[s]), s
        assert np.array_equal(areas, c["areas_" + s]), s
        assert int(comps[i]) == len(c["areas_" + s]), s
        if "labels_" + s in c:
            assert np.array_equal(lab, c["labels_" + s]), s
        first = np.unique(roots[i][roots[i] > 0]).astype(np.int64) - 1
        assert (roots[i].ravel()[first] == first + 1).all() and (first[:1] == np.flatnonzero(c[s])[:1]).all()


# ---- 2. the report's entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_one_image_without_aux(name):
    """n = 1, aux None, the three modes: set 1 of rows and the aux columns of counts are zeros, and aux_bits is refused"""
    c = load_cases()[name]
    for mode in MODES:
        counts, rows, bits, aux_bits, _ = run([c["pred"]], [c["label"]], None, mode)
        assert aux_bits is None and not rows[0, 1].any() and not counts[0, 3:].any()
        check(name, mode, counts[0], rows[0], bits[0], None, False)
    H, W = c["size"]
    z = torch.zeros(1, 1, H, W, device=dev())
    ws = torch.empty((ops.eval_components_ws_bytes(1, H, W) // 8,), dtype=torch.int64, device=dev())
    with pytest.raises(_lib.MdvitHipError, match="aux_bits without aux"):
        ops.eval_components(z, None, z, 1, poison(1, 5), poison(1, 3, 4), ws, None, poison(1, (H * W + 63) // 64))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_all_cases_of_one_size_with_aux(size, mode):
    """one call over every case of the size, every image with its own prediction, auxiliary output and label: a row from another image's data would show"""
    names = names_of_size(size)
    cs = [load_cases()[n] for n in names]
    counts, rows, bits, aux_bits, ties = run([c["pred"] for c in cs], [c["label"] for c in cs], [c["aux"] for c in cs], mode)
    assert ties > 0          # tiny positive logits were there, and they are background
    for i, name in enumerate(names):
        check(name, mode, counts[i], rows[i], bits[i], aux_bits[i], True)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    H, W = 20, 37
    words = (H * W + 63) // 64
    out, label = torch.randn(2, 1, H, W, device=dev()), torch.ones(2, 1, H, W, device=dev())
    ws = torch.empty((ops.eval_components_ws_bytes(2, H, W) // 8,), dtype=torch.int64, device=dev())
    counts, rows, bits, aux_bits = poison(2, 5), poison(2, 3, 4), poison(2, words), poison(2, words)
    E = _lib.MdvitHipError
    tall = torch.zeros(1, 1, 1025, 4, device=dev())
    with pytest.raises(E, match="1..1024"):
        ops.eval_components(tall, None, tall, 1, counts[:1], rows[:1], ws)
    for bad in (0, 4):
        with pytest.raises(E, match="mode"):
            ops.eval_components(out, None, label, bad, counts, rows, ws, bits)
    with pytest.raises(E, match="workspace"):
        ops.eval_components(out, None, label, 3, counts, rows, ws[:-1], bits)
    with pytest.raises(E, match="counts"):
        ops.eval_components(out, None, label, 3, counts.view(torch.float64), rows, ws)
    with pytest.raises(E, match="rows"):
        ops.eval_components(out, None, label, 3, counts, rows.view(2, 12), ws)
    with pytest.raises(E, match="bits"):
        ops.eval_components(out, None, label, 3, counts, rows, ws, bits[:, :-1])
    with pytest.raises(E, match="aux_bits without aux"):
        ops.eval_components(out, None, label, 3, counts, rows, ws, bits, aux_bits)
    with pytest.raises(E, match=r"\[n,1,H,W\]"):
        ops.eval_components(out.view(1, 2, H, W), None, label.view(1, 2, H, W), 3, counts[:1], rows[:1], ws)          # multi-channel logits
    with pytest.raises(E, match="CUDA"):
        ops.label_components(torch.zeros(1, 4, 4, dtype=torch.bool))
    with pytest.raises(E, match="1024"):
        ops.label_components(torch.zeros(1, 1025, 4, dtype=torch.bool, device=dev()))
    comps = poison(2)
    with pytest.raises(E, match="workspace"):
        ops.label_components(label.view(2, H, W), comps, ws[:4])
    torch.cuda.synchronize()
    for t in (counts, rows, bits, aux_bits, comps):
        assert bool((t == POISON).all())          # nothing was enqueued
    ops.eval_components(out.view(2, H, W), out.view(2, H, W), label.view(2, H, W), 3, counts, rows, ws, bits, aux_bits)          # [n,H,W] is accepted
    torch.cuda.synchronize()
    for t in (counts, rows, bits, aux_bits):
        assert not bool((t == POISON).any())
    assert torch.equal(bits, aux_bits) and torch.equal(rows[:, 0], rows[:, 1]) and rows[:, 2].tolist() == [[1, H * W, 0, 0]] * 2
