"""The per-image report (mdvit_amd/report.py, csrc/eval_images.hip) against the validation pass it itemises (EvalAccumulator: same predicates, so the counts
agree integer for integer), against its own packed masks, against the fp64 restatement of structure_loss on each image alone and the train-side operator it
restates, and end to end through evaluate(report=...) on the committed eval fixture.

`reached` restates the host's launch rule (ei_plan / es_tiles and the two fold kernels' trips in csrc/eval_images.hip); REACHES says what each shape is listed
for.  tests/test_report_launch_arithmetic.py checks both without a GPU, the restatement against the library's own workspace sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdvit_amd import ops
from mdvit_amd.evaluate import EvalAccumulator, evaluate
from mdvit_amd.report import ImageReport, pack_masks, unpack_masks
from test_gpu_evaluate import D, dev, fixture_batches, make_case, restate_counts

pytestmark = pytest.mark.gpu

# (images per group, H, W)
CASES = {"sub_word_5x7": ((1,), 5, 7), "odd_20x37": ((3, 1, 5), 20, 37), "tile_edge_33x65": ((2,), 33, 65), "two_groups_64x64": ((2, 2), 64, 64),
         "multi_block_256x256": ((1,), 256, 256)}


def _cdiv(a, b):
    return (a + b - 1) // b


def reached(images, H, W):
    """the launch arithmetic of mdvit_eval_images and mdvit_eval_structure for n = sum(images) images of H x W"""
    HW = H * W
    words = _cdiv(HW, 64)
    b = min(_cdiv(words, 16), 1024)                         # EI_WORDS_PER_BLOCK, EI_MAX_BLOCKS
    wpb = _cdiv(words, b)
    nblk = _cdiv(words, wpb)
    tiles_y, tiles_x = _cdiv(H, 32), _cdiv(W, 64)           # ES_TH, ES_TW
    ntiles = tiles_y * tiles_x
    return {"n": sum(images), "words": words, "tail_bits": HW % 64, "nblk": nblk, "wave_trips": _cdiv(min(wpb, words), 4),
            "count_fold_trips": _cdiv(nblk, 48), "count_fold_ragged": nblk > 48 and nblk % 48 != 0,          # EI_FOLD_ROWS
            "tiles": (tiles_y, tiles_x), "ragged_tile": (H % 32 != 0, W % 64 != 0), "inside_window": (H < 31, W < 31),
            "sum_fold_trips": _cdiv(ntiles, 24), "sum_fold_ragged": ntiles > 24 and ntiles % 24 != 0,          # ES_FOLD_ROWS
            "ws_images": 4 * 5 * sum(images) * nblk, "ws_structure": 8 * 4 * sum(images) * ntiles}


REACHES = {
    "sub_word_5x7": {"words": 1, "tail_bits": 35, "nblk": 1, "tiles": (1, 1), "inside_window": (True, True)},                    # HW < 64: one partial word
    "odd_20x37": {"words": 12, "tail_bits": 36, "nblk": 1, "wave_trips": 3, "tiles": (1, 1), "inside_window": (True, False),      # a tail word, three words per wave,
                  "ragged_tile": (True, True)},                                                                                   # unequal groups
    "tile_edge_33x65": {"words": 34, "tail_bits": 33, "nblk": 3, "tiles": (2, 2), "ragged_tile": (True, True)},                   # a 1-row and a 1-column last tile
    "two_groups_64x64": {"words": 64, "tail_bits": 0, "nblk": 4, "tiles": (2, 1), "ragged_tile": (False, False)},                 # whole words, whole tiles
    "multi_block_256x256": {"n": 1, "nblk": 64, "count_fold_trips": 2, "count_fold_ragged": True, "tiles": (8, 4),                # 64 workgroups on one image:
                            "sum_fold_trips": 2, "sum_fold_ragged": True},                                                       # a full trip and a ragged one, twice
}

TIES = (0.0, -0.0, 1e-8, -1e-8, 6e-8, -6e-8, 1e-6, -1e-6)


def tie_case(seed, images, H, W):
    """make_case without its own specials (they index a third image), then the tie logits in EVERY image: at the head of out under label 1, 0, 1, ... and
    at the tail of aux"""
    out, aux, label = make_case(seed, images, H, W, specials=False)
    n, k = out.shape[0], len(TIES)
    t = torch.tensor(TIES)
    out.view(n, -1)[:, :k] = t
    aux.view(n, -1)[:, -k:] = t
    label.view(n, -1)[:, :k] = torch.tensor([1.0, 0.0] * (k // 2))
    return out, aux, label


def domains_of(images):
    return [2, 0, 3][:len(images)]


def run_report(out, aux, label, images, **kw):
    rep = ImageReport(D, dev(), **kw)
    doms = domains_of(images)
    rep.update(out.to(dev()), None if aux is None else aux.to(dev()), label.to(dev()), doms if len(images) > 1 else doms[0], list(images))
    return rep


# ---- 1. counts = the existing kernel's, exactly --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aux", [True, False], ids=["aux", "no_aux"])
@pytest.mark.parametrize("case", list(CASES))
def test_image_counts_sum_to_the_accumulators_exactly(case, with_aux):
    images, H, W = CASES[case]
    out, aux, label = tie_case(3, images, H, W)
    if not with_aux:
        aux = None
    doms = domains_of(images)
    acc = EvalAccumulator(D, dev())
    acc.update(out.to(dev()), None if aux is None else aux.to(dev()), label.to(dev()), doms if len(images) > 1 else doms[0], list(images))
    rep = run_report(out, aux, label, images, masks=True, aux_masks=with_aux)
    res = rep.result()
    assert res["counts"].shape == (sum(images), 5) and res["counts"].dtype == np.int64
    assert res["domain"].tolist() == [d for d, k in zip(doms, images) for _ in range(k)]
    want = acc.counts.cpu().numpy()
    r0 = 0
    for d, k in zip(doms, images):
        got = res["counts"][r0:r0 + k].sum(0)
        print(f"{case} domain {d}: image rows sum to {got.tolist()}, accumulator {want[d].tolist()}")
        assert np.array_equal(got, want[d])                    # integer for integer: the tie rule needs no tolerance
        r0 += k
    if not with_aux:
        assert not res["counts"][:, 3:].any() and rep.aux_bits is None          # aux columns 0, no aux buffer at all
    # the ties sit where the two rules part: sigmoid(1e-8) and sigmoid(6e-8) round to 0.5 (background) although the logit is positive
    assert int((out.view(out.shape[0], -1)[:, :len(TIES)] > 0).sum()) == 3 * out.shape[0]
    # 2. the bits agree with the counts
    y = (label.view(label.shape[0], H, W) != 0).numpy()
    for name, col_i, col_a in (("masks", 0, 1),) + ((("aux_masks", 3, 4),) if with_aux else ()):
        m = unpack_masks(res[name], res["size"])
        assert res["size"] == (H, W) and m.shape == (sum(images), H, W) and m.dtype == np.uint8 and m.max() <= 1
        assert np.array_equal(m.reshape(len(m), -1).sum(1), res["counts"][:, col_a])
        assert np.array_equal((m.astype(bool) & y).reshape(len(m), -1).sum(1), res["counts"][:, col_i])
    assert np.array_equal(y.reshape(len(y), -1).sum(1), res["counts"][:, 2])
    # on the host: scores from those counts, 0/0 -> 0
    c = res["counts"].astype(np.float64)
    assert np.allclose(res["dice"], np.where(c[:, 1] + c[:, 2] > 0, 2 * c[:, 0] / np.maximum(c[:, 1] + c[:, 2], 1), 0.0), rtol=0, atol=1e-15)


# ---- 2. bits = the sign where the sign decides; tail bits and untouched buffers --------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_bits_follow_the_sign_and_the_tail_is_zero_on_prefilled_buffers(case):
    images, H, W = CASES[case]
    n, HW = sum(images), H * W
    words = _cdiv(HW, 64)
    gen = torch.Generator().manual_seed(17)
    mk = lambda: (torch.randint(0, 2, (n, 1, H, W), generator=gen) * 2 - 1).float() * (1e-3 + torch.randn((n, 1, H, W), generator=gen).abs())
    out, aux = mk(), mk()
    label = (torch.rand((n, 1, H, W), generator=gen) < 0.4).float()
    nan_words = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev()).view(torch.int64)
    counts, bits, aux_bits = nan_words(n, 5), nan_words(n, words), nan_words(n, words)
    ws = torch.empty((ops.eval_images_ws_bytes(n, HW) // 4,), dtype=torch.int32, device=dev())
    ops.eval_images(out.to(dev()), aux.to(dev()), label.to(dev()), counts, ws, bits, aux_bits)
    for t, packed in ((out, bits), (aux, aux_bits)):
        p = packed.cpu().numpy().view(np.uint64)
        assert np.array_equal(unpack_masks(p, (H, W)), (t.view(n, H, W) > 0).numpy().astype(np.uint8))
        assert np.array_equal(p, pack_masks((t.view(n, H, W) > 0).numpy()))          # whole words: the bits past HW are zero
        if HW % 64:
            assert not (p[:, -1] >> np.uint64(HW % 64)).any()
    want = [restate_counts(out[i], aux[i], label[i]) for i in range(n)]          # |logit| >= 1e-3: fp64 sigmoid and the device agree on the side of 0.5
    assert counts.cpu().tolist() == want
    # aux=None: the aux columns are written as zeros over the NaN pattern, and there is no aux buffer to touch
    counts2, bits2 = nan_words(n, 5), nan_words(n, words)
    ops.eval_images(out.to(dev()), None, label.to(dev()), counts2, ws, bits2, None)
    assert torch.equal(counts2[:, :3], counts[:, :3]) and not bool(counts2[:, 3:].any()) and torch.equal(bits2, bits)
    with pytest.raises(Exception, match="aux_bits without aux"):
        ops.eval_images(out.to(dev()), None, label.to(dev()), counts2, ws, bits2, aux_bits)
    # a report that keeps aux masks and meets a forward without an auxiliary output: empty masks, not stale memory
    rep = ImageReport(D, dev(), masks=True, aux_masks=True, capacity=n)
    rep.update(out.to(dev()), None, label.to(dev()), 1)
    res = rep.result()
    assert not res["aux_masks"].any() and np.array_equal(res["masks"], bits.cpu().numpy().view(np.uint64))


# ---- 3. / 4. the structure term ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def structure_refs():
    """fp64 structure_loss of every image alone, computed once per (case, scale)"""
    from oracle import transfuse_ref as R
    cache = {}

    def get(case, scale):
        if (case, scale) not in cache:
            images, H, W = CASES[case]
            label = make_case(23, images, H, W, specials=False)[2]          # binary, 30 % set; with three groups an all-zero and an all-one group
            out = scale * torch.randn(label.shape, generator=torch.Generator().manual_seed(24))          # scale 30: a saturated sigmoid
            ref = [float(R.structure_loss(out[i:i + 1].double(), label[i:i + 1].double())) for i in range(out.shape[0])]
            cache[(case, scale)] = (out, label, ref)
        return cache[(case, scale)]
    return get


@pytest.mark.parametrize("scale", [1.0, 30.0], ids=["scale1", "scale30"])
@pytest.mark.parametrize("case", list(CASES))
def test_structure_term_per_image_against_fp64_and_the_operator(structure_refs, case, scale):
    """3. each image's term against oracle.transfuse_ref.structure_loss in fp64 on that image alone (B = 1: the mean is the term), bound 1e-5 relative
    (test_structure_loss_past_one_chunk's).  4. the mean over a group against transfuse.structure_loss of the group, bound 1e-6 relative: the same fp32 element
    expressions, an exact weit, double sums in another order, the operator's result rounded once to fp32.  Measured on an MI355X, worst over the five shapes:
    3. 1.4e-08 at scale 1 and 4.3e-09 at scale 30; 4. 3.7e-08 (half an fp32 ulp is 6e-08)."""
    from mdvit_amd import transfuse as T
    images, H, W = CASES[case]
    out, label, ref = structure_refs(case, scale)
    assert set(np.unique(label.numpy())) <= {0.0, 1.0}
    if len(images) == 3:          # make_case: group 1 has an all-zero label, group 2 an all-one label
        a, b = images[0], images[0] + images[1]
        assert not bool(label[a:b].any()) and bool((label[b:] == 1).all())
    rep = run_report(out, None, label, images, structure=True)
    sums = torch.empty((sum(images), 4), dtype=torch.float64, device=dev())
    loss = torch.empty((sum(images),), dtype=torch.float64, device=dev())
    ws = torch.empty((ops.eval_structure_ws_bytes(sum(images), H, W) // 8,), dtype=torch.float64, device=dev())
    ops.eval_structure(out.to(dev()), label.to(dev()), loss, ws, sums)
    res = rep.result()
    got = res["structure"]
    assert got.dtype == np.float64 and got.shape == (sum(images),) and torch.equal(loss.cpu(), torch.from_numpy(got))
    S = sums.cpu().numpy()
    assert np.allclose(S[:, 0] / S[:, 1] + 1.0 - (S[:, 2] + 1.0) / (S[:, 3] - S[:, 2] + 1.0), got, rtol=1e-14, atol=0)          # sl_final_kernel's expression of the sums
    err = np.abs(got - np.array(ref)) / np.abs(np.array(ref))
    print(f"structure {case} scale {scale}: per image relative error vs fp64 max {err.max():.3e} {[f'{e:.2e}' for e in err]}  bound 1e-5")
    assert np.isfinite(got).all() and err.max() <= 1e-5
    # 4. the operator it restates: mean over a group = structure_loss of the group
    r0, doms = 0, domains_of(images)
    for d, k in zip(doms, images):
        op = float(T.structure_loss(out[r0:r0 + k].to(dev()), label[r0:r0 + k].to(dev())))
        mean = float(got[r0:r0 + k].mean())
        rel = abs(mean - op) / abs(op)
        print(f"structure {case} scale {scale} group of {k}: report mean {mean!r} operator {op!r} relative difference {rel:.3e}  bound 1e-6")
        assert rel <= 1e-6
        assert res["per_domain"][d]["structure_loss"] == mean and res["per_domain"][d]["images"] == k
        r0 += k
    assert res["sum_structure_loss"] == sum(res["per_domain"][d]["structure_loss"] for d in doms)


# ---- 5. offsets, growth, refusals --------------------------------------------------------------------------------------------------
def test_three_updates_from_capacity_two_equal_one_update_of_the_concatenation():
    images, H, W = (3, 1, 5), 20, 37
    out, aux, label = (t.to(dev()) for t in tie_case(29, images, H, W))
    kw = dict(masks=True, aux_masks=True, structure=True)
    one = ImageReport(D, dev(), capacity=9, **kw)
    one.update(out, aux, label, [2, 0, 3], list(images))
    cap_before = one._cap
    grown = ImageReport(D, dev(), capacity=2, **kw)
    grown.update(out[:3], aux[:3], label[:3], 2)
    grown.update(out[3:4], aux[3:4], label[3:4], [0], [1])
    grown.update(out[4:], aux[4:], label[4:], [3, 3], [2, 3])
    assert cap_before == 9 and grown._cap >= 9 and grown.rows == one.rows == 9
    a, b = one.result(), grown.result()
    assert a["domain"].tolist() == b["domain"].tolist() == [2, 2, 2, 0, 3, 3, 3, 3, 3]
    for k in ("counts", "structure", "masks", "aux_masks", "dice", "iou", "aux_dice", "aux_iou", "empty"):
        assert np.array_equal(a[k], b[k]), k
    assert a["per_domain"] == b["per_domain"] and a["counts"][:, 1].all()
    # rows differ from image to image, so a row at a wrong offset would show
    assert len({tuple(r) for r in a["masks"].tolist()}) == 9
    # reset keeps the tables and starts again at row 0
    grown.reset()
    grown.update(out[3:4], aux[3:4], label[3:4], 0)
    c = grown.result()
    assert c["domain"].tolist() == [0] and np.array_equal(c["counts"][0], a["counts"][3]) and np.array_equal(c["masks"][0], a["masks"][3])


def test_refusals():
    out, aux, label = (t.to(dev()) for t in tie_case(31, (2,), 20, 37))
    rep = ImageReport(D, dev())
    rep.update(out, aux, label, 1)
    with pytest.raises(ValueError, match="20 x 37"):
        rep.update(out[:, :, :10], aux[:, :, :10], label[:, :, :10], 1)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        ImageReport(D, dev(), structure=True).update(out.view(2, 20, 37), None, label.view(2, 20, 37), 1)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        ImageReport(D, dev(), structure=True).update(out.view(1, 2, 20, 37), None, label.view(1, 2, 20, 37), 1)
    with pytest.raises(ValueError):
        rep.update(out, aux, label, [0, 1, 2])          # 2 images are not 3 equal domain batches
    with pytest.raises(ValueError):
        rep.update(out, aux, label, D)                  # a domain outside 0..D-1
    assert rep.rows == 2
    # C level: a short workspace is MDVIT_E_WORKSPACE (4), n = 0 is MDVIT_E_SHAPE (1), both before any launch
    from mdvit_amd import _lib
    lib = _lib.load()
    n, H, W = 2, 20, 37
    counts = torch.zeros((n, 5), dtype=torch.int64, device=dev())
    loss = torch.zeros((n,), dtype=torch.float64, device=dev())
    need_i, need_s = lib.mdvit_eval_images_ws_bytes(n, H * W), lib.mdvit_eval_structure_ws_bytes(n, H, W)
    assert need_i == reached((n,), H, W)["ws_images"] and need_s == reached((n,), H, W)["ws_structure"]
    ws = torch.zeros((max(need_i, need_s) // 8 + 1,), dtype=torch.float64, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.mdvit_eval_images(p(out), None, p(label), n, H * W, p(counts), None, None, p(ws), need_i - 1, None) == 4
    assert b"eval_images" in lib.mdvit_last_error() and b"workspace" in lib.mdvit_last_error()
    assert lib.mdvit_eval_images(p(out), None, p(label), 0, H * W, p(counts), None, None, p(ws), need_i, None) == 1
    assert lib.mdvit_eval_structure(p(out), p(label), n, H, W, p(loss), None, p(ws), need_s - 1, None) == 4
    assert b"eval_structure" in lib.mdvit_last_error()
    assert lib.mdvit_eval_structure(p(out), p(label), 0, H, W, p(loss), None, p(ws), need_s, None) == 1
    assert lib.mdvit_eval_images_ws_bytes(0, H * W) == 0 and lib.mdvit_eval_structure_ws_bytes(n, 0, W) == 0
    torch.cuda.synchronize()
    assert not bool(counts.any()) and not bool(loss.any())          # nothing was enqueued


# ---- 6. bit-reproducible ---------------------------------------------------------------------------------------------------------
def test_two_epochs_give_equal_tables():
    big = [t.to(dev()) for t in tie_case(37, (1,), 256, 256)]
    small = [t.to(dev()) for t in tie_case(38, (2,), 33, 65)]
    for tensors, plan in ((big, [(slice(0, 1), 1, None)]), (small, [(slice(0, 2), [0, 3], [1, 1]), (slice(1, 2), 2, None)])):
        runs = []
        for _ in range(2):
            rep = ImageReport(D, dev(), masks=True, aux_masks=True, structure=True)
            for sl, doms, images in plan:
                rep.update(tensors[0][sl], tensors[1][sl], tensors[2][sl], doms, images)
            runs.append([t[:rep.rows].clone() for t in (rep.counts, rep.structure_col, rep.bits, rep.aux_bits)])
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert bool(runs[0][0].any()) and bool(torch.isfinite(runs[0][1]).all())


# ---- 7. no synchronisation in update ---------------------------------------------------------------------------------------------
def test_update_does_not_synchronise():
    out, aux, label = (t.to(dev()) for t in tie_case(41, (3, 1, 5), 20, 37))
    rep = ImageReport(D, dev(), masks=True, aux_masks=True, structure=True, capacity=4)
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
    res = rep.result()          # the one copy to the host
    assert res["domain"].tolist() == [0] * 3 + [1] + [2] * 5 + [3] * 3 + [0] * 3 + [1] + [2] * 5
    assert np.array_equal(res["counts"][:9], res["counts"][12:]) and np.array_equal(res["masks"][:9], res["masks"][12:])


# ---- 8. evaluate(report=...) on the committed fixture -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_model(golden):
    return fixture_batches(golden)


@pytest.mark.parametrize("fuse", [False, True], ids=["per_domain", "fused"])
def test_evaluate_with_a_report_on_the_eval_fixture(fixture_model, fuse):
    model, data = fixture_model
    model.eval()
    loaders = {f"set{d}": [data[d][:3]] for d in (0, 3)}
    plain = evaluate(model, loaders, num_domains=D, fuse_domains=fuse)
    rep = ImageReport(D, dev(), masks=True, aux_masks=True)
    res = evaluate(model, loaders, num_domains=D, fuse_domains=fuse, report=rep)
    assert "report" not in plain and set(res) == set(plain) | {"report"}
    for k in plain:
        assert res[k] == plain[k], k                          # equal, not close
    r = res["report"]
    B, S = data[0][0].shape[0], data[0][0].shape[-1]
    assert r["domain"].tolist() == [0] * B + [3] * B         # evaluation order: loader after loader, and the fused forward keeps it
    for d in (0, 3):
        assert r["counts"][r["domain"] == d].sum(0).tolist() == res["counts"][d]
        assert r["per_domain"][d]["images"] == B
    assert sorted(r["per_domain"]) == [0, 3] and r["size"] == (S, S)
    m = unpack_masks(r["masks"], r["size"])
    assert m.shape == (2 * B, S, S) == unpack_masks(r["aux_masks"], r["size"]).shape
    assert np.array_equal(m.reshape(2 * B, -1).sum(1), r["counts"][:, 1])
    # a second epoch with the same report starts from row 0
    again = evaluate(model, loaders, num_domains=D, fuse_domains=fuse, report=rep)["report"]
    assert np.array_equal(again["counts"], r["counts"]) and np.array_equal(again["masks"], r["masks"])
