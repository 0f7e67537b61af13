"""CPU-only checks of the validation pass (mdvit_amd/evaluate.py, csrc/evaluate.hip): the C ABI's argument validation (before any HIP call), the planner that
decides which batches share a forward, the helper that finds the logits in a model's output, and the refusal of host tensors."""
import ctypes as C

import pytest
import torch

from mdvit_amd.evaluate import MAX_GROUPS, plan_epoch, plan_round, split_outputs

E_SHAPE = 1


def _ints(*v):
    return (C.c_int32 * len(v))(*v)


def _accumulate(lib, *, out=64, aux=None, label=64, images=(2,), domains=(0,), G=None, npi=16, nd=4, acc=64, counts=64, rows=None, ws=64, ws_bytes=None):
    """mdvit_eval_accumulate with stand-in addresses (64: non-NULL and aligned; nothing is dereferenced before the checks pass); -> (code, message)"""
    G = len(images) if G is None else G
    img = None if images is None else _ints(*images)
    dom = None if domains is None else _ints(*domains)
    ws_bytes = lib.mdvit_eval_ws_bytes(max(1, min(G, MAX_GROUPS))) if ws_bytes is None else ws_bytes
    rc = lib.mdvit_eval_accumulate(out, aux, label, img, dom, G, npi, nd, acc, counts, rows, ws, ws_bytes, None)
    return rc, lib.mdvit_last_error()


def test_eval_ws_bytes_is_positive_and_monotone_in_G():
    from mdvit_amd import _lib
    lib = _lib.load()
    sizes = [lib.mdvit_eval_ws_bytes(G) for G in range(1, MAX_GROUPS + 1)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert lib.mdvit_eval_ws_bytes(0) == 0 and lib.mdvit_eval_ws_bytes(MAX_GROUPS + 1) == 0 and lib.mdvit_eval_ws_bytes(-3) == 0


def test_eval_accumulate_bad_arguments_return_error_codes_without_gpu():
    """every rejected call: MDVIT_E_SHAPE, the entry's name in the message, and no HIP call (this box has no GPU to make one on)"""
    from mdvit_amd import _lib
    lib = _lib.load()
    bad = [dict(out=None), dict(label=None), dict(images=None, G=1), dict(domains=None, G=1), dict(acc=None), dict(counts=None), dict(ws=None),      # null pointers
           dict(images=(), domains=(), G=0), dict(images=(1,) * 17, domains=(0,) * 17, G=17), dict(G=-1),                                            # G = 0, 17
           dict(npi=0), dict(npi=-5),                                                                                                                 # n_per_image <= 0
           dict(images=(2, 0, 1), domains=(0, 1, 2)), dict(images=(-1,)),                                                                             # a group with 0 images
           dict(domains=(4,)), dict(domains=(-1,)), dict(images=(1, 1), domains=(0, 7)), dict(nd=0), dict(domains=(2,), nd=2),                        # a domain outside 0..num_domains-1
           dict(ws_bytes=0), dict(images=(1, 1), domains=(0, 1), ws_bytes=lib.mdvit_eval_ws_bytes(1)),                                                # a too-small workspace
           dict(images=(1,) * 16, domains=tuple(range(16)), nd=16, ws_bytes=lib.mdvit_eval_ws_bytes(16) - 1)]
    for kw in bad:
        rc, msg = _accumulate(lib, **kw)
        assert rc == E_SHAPE and b"eval_accumulate" in msg, (kw, rc, msg)
    rc, msg = _accumulate(lib, domains=(5,))
    assert b"domain 5" in msg, msg
    rc, msg = _accumulate(lib, ws_bytes=16)
    assert b"workspace too small" in msg and b"mdvit_eval_ws_bytes" in msg, msg


def test_eval_table_bad_arguments_return_error_codes_without_gpu():
    from mdvit_amd import _lib
    lib = _lib.load()
    for args in ((None, 4, 64), (64, 4, None), (64, 0, 64), (64, -1, 64)):
        assert lib.mdvit_eval_table(*args, None) == E_SHAPE, args
        assert b"eval_table" in lib.mdvit_last_error()


SIZES = {"isic": [4, 4, 4], "ph2": [4, 4, 4], "dmf": [4, 3], "skd": [1]}       # loaders of 3, 3, 2, 1 batches at bs = 4, last batches of 4, 4, 3, 1 images


def test_planner_covers_every_batch_once_and_fuses_equal_sizes_of_distinct_domains():
    steps = plan_epoch(SIZES)
    flat = [kb for step in steps for kb in step]
    want = [(k, i) for k, sizes in SIZES.items() for i in range(len(sizes))]
    assert sorted(flat) == sorted(want) and len(flat) == len(set(flat))
    for step in steps:
        assert len({SIZES[k][i] for k, i in step}) == 1, step             # equal sizes
        assert len({k for k, _ in step}) == len(step), step               # distinct domains
    fused = [s for s in steps if len(s) > 1]
    assert fused == [[("isic", 0), ("ph2", 0), ("dmf", 0)], [("isic", 1), ("ph2", 1)], [("isic", 2), ("ph2", 2)]]
    # the ragged tails run per domain, after their round's fused forward
    assert steps == [fused[0], [("skd", 0)], fused[1], [("dmf", 1)], fused[2]]
    # a loader's batches keep their order
    for k in SIZES:
        assert [i for step in steps for kk, i in step if kk == k] == list(range(len(SIZES[k])))


def test_planner_without_fusing_is_the_reference_order():
    steps = plan_epoch(SIZES, fuse_domains=False)
    assert steps == [[(k, i)] for k, sizes in SIZES.items() for i in range(len(sizes))]          # domain after domain (multi_train_MDViT.py:246-253)


def test_planner_never_puts_one_domain_twice_into_a_forward():
    # two loaders of the same domain: their batches may not share a forward, whatever their sizes
    assert plan_round([("a", 4, 1), ("b", 4, 1), ("c", 4, 2)]) == [["a", "c"], ["b"]]
    assert plan_epoch({"a": [4], "b": [4]}, domains={"a": 3, "b": 3}) == [[("a", 0)], [("b", 0)]]
    # different sizes never fuse; a full group opens the next one
    assert plan_round([("a", 4, 0), ("b", 3, 1), ("c", 3, 2), ("d", 4, 3)]) == [["a", "d"], ["b", "c"]]
    many = [(i, 2, i) for i in range(MAX_GROUPS + 3)]
    got = plan_round(many)
    assert [len(g) for g in got] == [MAX_GROUPS, 3] and [k for g in got for k in g] == list(range(MAX_GROUPS + 3))
    assert plan_round(many, fuse_domains=False) == [[i] for i in range(MAX_GROUPS + 3)]
    assert plan_round([]) == [] and plan_epoch({}) == []


def test_split_outputs_on_stand_in_tensors():
    out, aux, l0, l1 = (torch.full((2, 1, 4, 4), float(v)) for v in range(4))
    o, a = split_outputs([out, aux])                     # the MDViT family
    assert o is out and a is aux
    o, a = split_outputs(out)                            # the BASE family
    assert o is out and a is None
    o, a = split_outputs((l0, l1, out))                  # TransFuse's lateral maps: the last one is scored
    assert o is out and a is None
    o, a = split_outputs([out, None])                    # a domain without a peer head
    assert o is out and a is None
    o, a = split_outputs({"seg": [out, aux], "feat": l0})
    assert o is out and a is aux
    for bad in ([out], (out, aux, l0, l1), "logits", [out, 3]):
        with pytest.raises(TypeError):
            split_outputs(bad)


def test_ops_and_accumulator_refuse_host_tensors():
    import mdvit_amd
    from mdvit_amd import _lib, ops
    from mdvit_amd.evaluate import EvalAccumulator
    assert mdvit_amd.EvalAccumulator is EvalAccumulator and callable(mdvit_amd.evaluate)
    x = torch.zeros(2, 1, 4, 4)
    acc, counts, ws = torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 5, dtype=torch.int64), torch.zeros(1024, dtype=torch.int32)
    with pytest.raises(_lib.MdvitHipError):
        ops.eval_accumulate(x, x, x, [2], [0], acc, counts, ws)
    with pytest.raises(_lib.MdvitHipError):
        ops.eval_accumulate(x, None, x, [2], [0], acc, counts, ws)
    with pytest.raises(_lib.MdvitHipError):
        ops.eval_table(acc)
    with pytest.raises(ValueError):
        EvalAccumulator(4, device="cpu")
