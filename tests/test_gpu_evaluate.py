"""The on-device validation pass (mdvit_amd/evaluate.py, csrc/evaluate.hip) against an fp64 restatement of the reference's loop written here
(multi_train_MDViT.py:253-313; medpy 0.4.0's dc = 2|A&B| / (|A|+|B|), jc = |A&B| / |A|B|, restated because medpy is not a dependency; 0/0 -> 0 as
seg_metric_final_kernel has it), against the kernels it fuses, and end to end on the committed eval fixture."""
import pytest
import torch
import torch.nn.functional as F

from mdvit_amd.evaluate import EvalAccumulator, evaluate

pytestmark = pytest.mark.gpu

D = 4


def dev():
    return torch.device("cuda:0")


# ---- the restatement (CPU, fp64) ------------------------------------------------------------------------------------
def restate_counts(out, aux, label):
    A, Y = torch.sigmoid(out.double()) > 0.5, label != 0
    c = [int((A & Y).sum()), int(A.sum()), int(Y.sum()), 0, 0]
    if aux is not None:
        B = torch.sigmoid(aux.double()) > 0.5
        c[3], c[4] = int((B & Y).sum()), int(B.sum())
    return c


def dc(i, a, y):
    return 2.0 * i / (a + y) if a + y > 0 else 0.0


def jc(i, a, y):
    return i / (a + y - i) if a + y - i > 0 else 0.0


def restate_batch(out, aux, label):
    """one batch as the reference scores it (:270-289): -> ([loss, dice, iou, aux dice, aux iou], counts)"""
    o, y = torch.sigmoid(out.double()).reshape(-1), label.double().reshape(-1)
    bce = -(y * torch.log(o).clamp(min=-100.0) + (1.0 - y) * torch.log(1.0 - o).clamp(min=-100.0)).mean()          # nn.BCELoss
    dice = 1.0 - (2.0 * (o * y).sum() + 1e-5) / ((o * o).sum() + (y * y).sum() + 1e-5)                             # Utils/losses.py:8-16
    c = restate_counts(out, aux, label)
    row = [float(bce + dice), dc(c[0], c[1], c[2]), jc(c[0], c[1], c[2])]
    row += [dc(c[3], c[4], c[2]), jc(c[3], c[4], c[2])] if aux is not None else [0.0, 0.0]
    return row, c


def restate_table(calls, num_domains=D):
    """calls: [(domain, images, row)] in any order -> table [D+1][6] (:278-313): sum(x * len) / num per domain; the sum of the losses, the means of the scores
    over the domains that saw images, the total images"""
    tab = torch.zeros(num_domains + 1, 6, dtype=torch.float64)
    for d in range(num_domains):
        mine = [(n, row) for dd, n, row in calls if dd == d]
        num = sum(n for n, _ in mine)
        if num:
            tab[d, :5] = torch.tensor([sum(row[k] * n for n, row in mine) / num for k in range(5)], dtype=torch.float64)
        tab[d, 5] = num
    seen = tab[:num_domains, 5] > 0
    tab[num_domains, 0] = tab[:num_domains, 0].sum()
    if bool(seen.any()):
        tab[num_domains, 1:5] = tab[:num_domains][seen][:, 1:5].mean(0)
    tab[num_domains, 5] = tab[:num_domains, 5].sum()
    return tab


def check_table(got, want, name):
    got = got.double().cpu()
    rel = (got[:, 0] - want[:, 0]).abs() / want[:, 0].abs().clamp(min=1e-30)
    print(f"{name}: max |dice/iou - restatement| {float((got[:, 1:5] - want[:, 1:5]).abs().max()):.3e}, max rel loss error {float(rel[want[:, 0] != 0].max()):.3e}")
    assert torch.equal(got[:, 5], want[:, 5]), (name, got[:, 5], want[:, 5])
    assert float((got[:, 1:5] - want[:, 1:5]).abs().max()) <= 1e-6, (name, got, want)           # fp32 cells of exact counts
    assert bool(((got[:, 0] - want[:, 0]).abs() <= 1e-4 * want[:, 0].abs()).all()), (name, got[:, 0], want[:, 0])      # kernel vs fp64


# ---- inputs -----------------------------------------------------------------------------------------------------------
def logits(gen, shape):
    """|logit| in [1e-3, 6]: the device's expf and torch's sigmoid agree on the side of 0.5, and 1 - sigmoid keeps its fp32 digits"""
    mag = 1e-3 + (6.0 - 1e-3) * torch.rand(shape, generator=gen)
    return mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


def make_case(seed, images, H, W, specials=True):
    """out / aux / label [sum(images),1,H,W] on the CPU.  With three groups: group 0 carries exact zeros and +-120 (the BCE clamp) under both label values,
    group 1 is empty in label and predictions, group 2 has an all-ones label."""
    gen = torch.Generator().manual_seed(seed)
    n = sum(images)
    out, aux = logits(gen, (n, 1, H, W)), logits(gen, (n, 1, H, W))
    label = (torch.rand((n, 1, H, W), generator=gen) < 0.3).float()
    if specials:
        npi = H * W
        for t in (out, aux):
            flat = t.view(-1)
            flat[0], flat[1], flat[2], flat[3], flat[4], flat[5] = 0.0, 0.0, 120.0, 120.0, -120.0, -120.0
            flat[npi - 1], flat[npi], flat[2 * npi + 3] = 120.0, -120.0, 0.0
        label.view(-1)[:6] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    if len(images) == 3:
        a, b = images[0], images[0] + images[1]
        label[a:b] = 0.0
        out[a:b], aux[a:b] = -out[a:b].abs(), -aux[a:b].abs()
        label[b:] = 1.0
    return out, aux, label


def groups_of(t, images):
    return list(torch.split(t, list(images))) if t is not None else [None] * len(images)


CASES = {"odd_37x29": ((3, 1, 2), 37, 29), "sub_wave_5x7": ((3, 1, 2), 5, 7), "multi_block_96x96": ((8,), 96, 96)}


@pytest.mark.parametrize("with_aux", [True, False], ids=["aux", "no_aux"])
@pytest.mark.parametrize("case", list(CASES))
def test_update_equals_the_fp64_restatement(case, with_aux):
    images, H, W = CASES[case]
    out, aux, label = make_case(7, images, H, W)
    if not with_aux:
        aux = None
    domains = [2, 0, 3][:len(images)]
    acc = EvalAccumulator(D, dev())
    rows = acc.update(out.to(dev()), None if aux is None else aux.to(dev()), label.to(dev()), domains if len(images) > 1 else domains[0], list(images)).cpu()
    calls, want_counts = [], torch.zeros(D, 5, dtype=torch.int64)
    for g, (o, a, y) in enumerate(zip(groups_of(out, images), groups_of(aux, images), groups_of(label, images))):
        row, c = restate_batch(o, a, y)
        calls.append((domains[g], images[g], row))
        want_counts[domains[g]] += torch.tensor(c)
        print(f"{case} group {g}: got {rows[g].tolist()} want {row}")
        assert float((rows[g, 1:].double() - torch.tensor(row[1:], dtype=torch.float64)).abs().max()) <= 1e-6
        assert abs(float(rows[g, 0]) - row[0]) <= 1e-4 * abs(row[0])
    assert torch.equal(acc.counts.cpu(), want_counts), (acc.counts.cpu(), want_counts)
    if len(images) == 3:          # the empty group scores 0 (0/0 -> 0), the all-ones label is counted whole
        assert rows[1, 1:].tolist() == [0.0, 0.0, 0.0, 0.0] and want_counts[0].tolist() == [0, 0, 0, 0, 0]
        assert int(want_counts[3, 2]) == images[2] * H * W
    check_table(acc.table(), restate_table(calls), case)
    res = acc.result()
    assert res["images"] == [int(v) for v in restate_table(calls)[:D, 5]] and res["counts"] == want_counts.tolist()


def test_update_equals_the_kernels_it_fuses_per_group():
    from mdvit_amd import ops
    images = (3, 1, 2)
    out, aux, label = (t.to(dev()) for t in make_case(11, images, 37, 29))
    acc = EvalAccumulator(D, dev())
    rows = acc.update(out, aux, label, [0, 1, 2], list(images)).clone()
    for g, (o, a, y) in enumerate(zip(groups_of(out, images), groups_of(aux, images), groups_of(label, images))):
        metrics, counts = ops.seg_metrics(o, a, y)
        assert torch.equal(acc.counts[g], counts[:5]), (g, acc.counts[g], counts)
        assert torch.equal(rows[g, 1:], metrics), (g, rows[g], metrics)                       # bit for bit
        l0 = float(ops.seg_losses(o, None, y)[0])
        print(f"group {g}: loss {float(rows[g, 0])!r} vs seg_losses {l0!r}")
        assert abs(float(rows[g, 0]) - l0) <= 1e-6 * abs(l0)


def test_accumulation_over_calls_and_shared_domains():
    """three calls: domain 0 appears in two of them, the third holds two groups of domain 1; domain 2 sees nothing"""
    acc = EvalAccumulator(D, dev())
    plan = [((2, 2), [0, 1], None), ((3,), 0, None), ((1, 2, 1), [1, 1, 3], [1, 2, 1])]
    calls = []
    for i, (images, domains, images_arg) in enumerate(plan):
        out, aux, label = make_case(20 + i, images, 37, 29, specials=(i == 0))
        acc.update(out.to(dev()), aux.to(dev()), label.to(dev()), domains, images_arg)
        ds = [domains] if isinstance(domains, int) else domains
        for g, (o, a, y) in enumerate(zip(groups_of(out, images), groups_of(aux, images), groups_of(label, images))):
            calls.append((ds[g], images[g], restate_batch(o, a, y)[0]))
    want = restate_table(calls)
    table = acc.table()
    check_table(table, want, "three calls")
    assert table[2].tolist() == [0.0] * 6 and want[:, 5].tolist() == [5.0, 5.0, 0.0, 1.0, 11.0]
    # the last row: the SUM of the three losses, the MEANS over the three domains that saw images
    t = table.double().cpu()
    assert abs(float(t[D, 0]) - float(t[[0, 1, 3], 0].sum())) <= 1e-6 * float(t[D, 0])
    assert float((t[D, 1:5] - t[[0, 1, 3], 1:5].mean(0)).abs().max()) <= 1e-6
    assert acc.acc.cpu()[:, 6].tolist() == [2.0, 3.0, 0.0, 1.0]          # batches per domain
    res = acc.result()
    assert res["images"] == [5, 5, 0, 1] and res["total_images"] == 11 and abs(res["sum_loss"] - float(want[D, 0])) <= 1e-4 * float(want[D, 0])
    assert abs(res["avg_iou"] - float(want[D, 2])) <= 1e-6 and abs(res["avg_aux_dice"] - float(want[D, 3])) <= 1e-6
    acc.reset()
    assert not bool(acc.table().any()) and not bool(acc.acc.any()) and not bool(acc.counts.any())


def test_epoch_state_is_bit_reproducible():
    out, aux, label = (t.to(dev()) for t in make_case(31, (8,), 96, 96))
    runs = []
    for _ in range(2):
        acc = EvalAccumulator(D, dev())
        acc.update(out, aux, label, 1)
        acc.update(out[:5], aux[:5], label[:5], [1, 2], [3, 2])
        runs.append((acc.acc.clone(), acc.counts.clone(), acc.table().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool(runs[0][1].any())


def test_update_and_table_do_not_synchronise():
    out, aux, label = (t.to(dev()) for t in make_case(41, (3, 1, 2), 37, 29))
    acc = EvalAccumulator(D, dev())
    acc.update(out, aux, label, [0, 1, 2], [3, 1, 2])          # first use: code objects loaded outside the checked window
    acc.table()
    acc.reset()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.update(out, aux, label, [0, 1, 2], [3, 1, 2])
        acc.update(out[:3], None, label[:3], 3)
        table = acc.table()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    res = acc.result()          # the one copy to the host
    assert res["images"] == [3, 1, 2, 3] and tuple(table.shape) == (D + 1, 6)


# ---- end to end on the committed fixture ------------------------------------------------------------------------------------
FLIP = 1e-3


def fixture_batches(golden):
    """-> (model, {domain: (image, label, set_id, fixture out, fixture aux)}), CPU tensors, as test_mdvit_eval_vs_golden builds them"""
    from oracle.gen_golden import synth_image, synth_label
    from test_gpu_model import build_mdvit
    g = golden("mdvit_eval_64")
    S, B, seed = [int(v) for v in g["meta"]]
    data = {}
    for d in (0, 3):
        data[d] = (synth_image(300 + d, B, S, S), synth_label(310 + d, B, S, S), torch.full((B,), d, dtype=torch.long),
                   torch.from_numpy(g[f"out_{d}"]), torch.from_numpy(g[f"aux_{d}"]))
    return build_mdvit(seed, S), data


def check_against_fixture(res, batches, name):
    """batches: [(domain, fixture out, fixture aux, label)], one per loader batch.  The device's logits and the fixture's agree to 1e-3, so a thresholded
    element may flip where the fixture's logit is within FLIP of zero: with k such elements in the tensor concerned every count may differ by k, Dice / IoU by
    2k / (|A|+|Y|-k); the loss is bound at 1e-3 relative (the project's logits / losses bound).  k <= 0.001 * elements, so the allowance hides no failure.
    (FLIP: 1e-3.  With 2e-3 the fixture's aux_0 holds 9 such elements of 8192, past the 0.001 guard whatever the code under test does; 1e-3 -- at most 3 per
    tensor -- satisfies the guard and allows fewer flips, so this asks more of the code, not less.)"""
    calls, want_counts, k_counts, slack = [], torch.zeros(D, 5, dtype=torch.int64), torch.zeros(D, 5, dtype=torch.int64), torch.zeros(D + 1, 6, dtype=torch.float64)
    for d, o, a, y in batches:
        row, c = restate_batch(o, a, y)
        calls.append((d, o.shape[0], row))
        want_counts[d] += torch.tensor(c)
        ko, ka = int((o.abs() <= FLIP).sum()), int((a.abs() <= FLIP).sum())
        assert ko <= 0.001 * o.numel() and ka <= 0.001 * a.numel(), (ko, ka, o.numel())
        k_counts[d] += torch.tensor([ko, ko, 0, ka, ka])
        so, sa = 2.0 * ko / (c[1] + c[2] - ko), 2.0 * ka / (c[4] + c[2] - ka)
        slack[d, 1:5] = torch.maximum(slack[d, 1:5], torch.tensor([so, so, sa, sa], dtype=torch.float64))
    slack[D, 1:5] = slack[:D, 1:5].max(0).values
    want = restate_table(calls)
    got_counts = torch.tensor(res["counts"])
    got = torch.tensor([[res[c][d] for c in ("loss", "dice", "iou", "aux_dice", "aux_iou", "images")] for d in range(D)]
                       + [[res["sum_loss"], res["avg_dice"], res["avg_iou"], res["avg_aux_dice"], res["avg_aux_iou"], res["total_images"]]], dtype=torch.float64)
    print(f"{name}: counts {got_counts.tolist()} fixture {want_counts.tolist()} allowance {k_counts.tolist()}")
    print(f"{name}: table {got.tolist()}\n{name}: fixture {want.tolist()}\n{name}: score allowance {slack[:, 1:5].tolist()}")
    assert torch.equal(got[:, 5], want[:, 5])
    assert bool(((got_counts - want_counts).abs() <= k_counts).all())
    assert bool(((got[:, 1:5] - want[:, 1:5]).abs() <= slack[:, 1:5] + 1e-6).all())
    assert bool(((got[:, 0] - want[:, 0]).abs() <= 1e-3 * want[:, 0].abs()).all())
    assert got[1].tolist() == [0.0] * 6 and got[2].tolist() == [0.0] * 6


@pytest.fixture(scope="module")
def fixture_model(golden):
    return fixture_batches(golden)


@pytest.mark.parametrize("fuse", [False, True], ids=["per_domain", "fused"])
def test_evaluate_on_the_eval_fixture(fixture_model, fuse):
    model, data = fixture_model
    model.train()
    loaders = {f"set{d}": [data[d][:3]] for d in (0, 3)}
    res = evaluate(model, loaders, num_domains=D, fuse_domains=fuse)
    assert model.training                                    # the mode it came in with
    model.eval()
    res2 = evaluate(model, loaders, num_domains=D, fuse_domains=fuse)
    assert not model.training and res2["images"] == res["images"] == [2, 0, 0, 2]
    check_against_fixture(res, [(d, data[d][3], data[d][4], data[d][1]) for d in (0, 3)], "fused" if fuse else "per domain")


def test_evaluate_with_a_short_last_batch(fixture_model):
    """domain 0: the fixture's batch of 2, then its first image alone (eval forwards score every image on its own); domain 3: one batch of 2.  Round 0 fuses the
    two batches of 2, round 1 runs the tail per domain."""
    model, data = fixture_model
    img, lab, sid, fo, fa = data[0]
    loaders = {0: [(img, lab, sid), (img[:1], lab[:1], sid[:1])], 3: [data[3][:3]]}
    res = evaluate(model.eval(), loaders, num_domains=D, fuse_domains=True)
    assert res["images"] == [3, 0, 0, 2]
    check_against_fixture(res, [(0, fo, fa, lab), (0, fo[:1], fa[:1], lab[:1]), (3, data[3][3], data[3][4], data[3][1])], "short last batch")
    # uint8 NHWC images go through ops.image_normalize_u8: the loader contract of synthetic.make_domain_batch with the image left as the camera gave it
    gen = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 64, 64, 3), generator=gen, dtype=torch.uint8)
    from mdvit_amd import ops
    res_u8 = evaluate(model, {3: [(u8, data[3][1], data[3][2])]}, num_domains=D)
    res_f = evaluate(model, {3: [(ops.image_normalize_u8(u8.to(dev())), data[3][1], data[3][2])]}, num_domains=D)
    print(f"uint8 loader: {res_u8}\nnormalised on the device first: {res_f}")
    assert res_u8["images"] == res_f["images"] == [0, 0, 0, 2]
    assert abs(res_u8["sum_loss"] - res_f["sum_loss"]) <= 1e-3 * res_f["sum_loss"] and abs(res_u8["avg_dice"] - res_f["avg_dice"]) <= 1e-3
