"""CPU-only checks of the resume path: the C ABI of csrc/snapshot.hip and of mdvit_adam_step (declared, exported, arguments refused before any launch), the
snapshot's table builder, and the host-side state of StepLR, DomainBatches and TrainAug."""
import pytest
import torch

NEW_SYMBOLS = ("mdvit_adam_step", "mdvit_table_pack", "mdvit_table_unpack")
FAKE = 4096          # a non-null, 16-byte aligned "pointer": every call below is refused before anything dereferences it


def test_new_abi_symbols_are_in_the_header_and_the_built_library():
    from mdvit_amd import _lib
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name


@pytest.mark.parametrize("entry", ["mdvit_table_pack", "mdvit_table_unpack"])
def test_table_entries_refuse_bad_arguments_without_gpu(entry):
    from mdvit_amd import _lib
    lib = _lib.load()
    fn, tag = getattr(lib, entry), entry[len("mdvit_"):].encode()
    for args, code in (((None, 1, FAKE, 1, None), 1), ((FAKE, 1, None, 1, None), 1), ((FAKE, 0, FAKE, 1, None), 1), ((FAKE, -3, FAKE, 1, None), 1),
                       ((FAKE, 1, FAKE, 0, None), 1), ((FAKE, 1, FAKE, 65536, None), 1), ((FAKE, 1, FAKE + 4, 1, None), 3), ((FAKE, 1, FAKE + 8, 1, None), 3)):
        assert fn(*args) == code, (entry, args)
        assert tag in lib.mdvit_last_error(), (entry, args, lib.mdvit_last_error())


def test_adam_step_refuses_bad_arguments_without_gpu():
    from mdvit_amd import _lib
    lib = _lib.load()
    ok = dict(table=FAKE, n=1, blocks=1, lr=FAKE, step=FAKE, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, zero=0, mode=0)
    for change in ({"table": None}, {"lr": None}, {"step": None}, {"n": 0}, {"blocks": 0}, {"b1": 1.0}, {"b2": -0.1}, {"eps": 0.0}, {"mode": 2}, {"mode": -1}):
        a = {**ok, **change}
        assert lib.mdvit_adam_step(a["table"], a["n"], a["blocks"], a["lr"], a["step"], a["b1"], a["b2"], a["eps"], a["wd"], a["zero"], a["mode"], None) == 1, change
        assert b"adam_step" in lib.mdvit_last_error() and b"adamw_step" not in lib.mdvit_last_error(), change
    assert lib.mdvit_adamw_step(None, 1, 1, FAKE, FAKE, 0.9, 0.999, 1e-8, 0.0, 0, None) == 1 and b"adamw_step" in lib.mdvit_last_error()


def test_table_layout_slots_are_aligned_disjoint_and_chunked():
    from mdvit_amd.snapshot import CHUNK_BYTES, table_layout
    sizes = [4, 12, 28, 2052, 4 * (32768 + 5), 8, 5, 0, CHUNK_BYTES, 3 * CHUNK_BYTES + 1, 16]
    offsets, rows, total = table_layout(sizes)
    pad = [(n + 15) // 16 * 16 for n in sizes]
    assert total == sum(pad) and len(offsets) == len(sizes)
    for i, off in enumerate(offsets):
        assert off % 16 == 0
        assert off == sum(pad[:i])                                   # in order, back to back: no overlap, no hole beyond the padding
    assert all(0 < n <= CHUNK_BYTES for _, _, n in rows)
    for i, size in enumerate(sizes):                                 # the rows of a tensor tile it exactly, in order
        mine = [(c0, n) for t, c0, n in rows if t == i]
        assert sum(n for _, n in mine) == size
        assert [c0 for c0, _ in mine] == [k * CHUNK_BYTES for k in range(len(mine))]
    assert not [r for r in rows if r[0] == 7]                        # an empty tensor has a slot of zero bytes and no row
    assert table_layout([40], chunk=16) == ([0], [(0, 0, 16), (0, 16, 16), (0, 32, 8)], 48)
    for bad in (0, 24, -16):
        with pytest.raises(ValueError):
            table_layout([4], chunk=bad)
    with pytest.raises(ValueError):
        table_layout([4, -1])


class _Opt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def test_steplr_state_round_trip_reapplies_the_learning_rate():
    from mdvit_amd.optim import StepLR
    a = StepLR(_Opt(0.01), step_size=2, gamma=0.5)
    for _ in range(5):
        a.step()
    sd = a.state_dict()
    assert sd == {"last_epoch": 5, "base_lr": 0.01, "step_size": 2, "gamma": 0.5}
    opt = _Opt(123.0)
    b = StepLR(opt, step_size=7, gamma=0.9)
    b.load_state_dict(sd)
    assert b.state_dict() == sd and opt.param_groups[0]["lr"] == a.get_last_lr()[0] == 0.01 * 0.5 ** 2
    a.step(); b.step()
    assert b.get_last_lr() == a.get_last_lr() == [0.01 * 0.5 ** 3]


class _Len:
    """what DomainBatches.indices() needs of a dataset"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _batches(seed=5, batch_size=2, rank=0, world=1, lengths=(6, 7, 11, 4)):
    from mdvit_amd.data import DomainBatches
    return DomainBatches({f"d{k}": _Len(n) for k, n in enumerate(lengths)}, batch_size=batch_size, seed=seed, rank=rank, world=world)


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_index_stream_after_load_equals_the_uninterrupted_one_across_an_epoch_boundary(rank, world):
    """an epoch is 5 steps for one rank (the 11-sample domain): the save falls after step 3, where some domains have batches of a permutation queued, some
    have just used theirs up and the 4-sample domain is inside its second permutation; the comparison runs over the rest of the epoch and all of the next"""
    whole = _batches(rank=rank, world=world)
    steps = [whole.next_indices() for _ in range(2 * len(whole) + 3)]
    first = _batches(rank=rank, world=world)
    for k in range(3):
        assert _same(first.next_indices(), steps[k])
    sd = first.state_dict()
    assert any(len(q) for q in sd["queues"].values())
    sd = {k: v for k, v in sd.items()}
    later = _batches(seed=99, rank=rank, world=world)              # other generators, and advanced: all of it must be overwritten
    later.next_indices()
    later.load_state_dict(sd)
    first.next_indices()                                          # the state is a copy: the saving object going on does not change it
    for k in range(3, len(steps)):
        assert _same(later.next_indices(), steps[k]), k


def test_domain_batches_state_carries_the_augmentation_generator():
    from mdvit_amd.augment import draw_train_aug
    a, b = _batches(), _batches(seed=99)
    draw_train_aug(2, 16, 16, a.aug.generator, a.aug.p)
    b.load_state_dict(a.state_dict())
    for x, y in zip(draw_train_aug(2, 16, 16, a.aug.generator, a.aug.p), draw_train_aug(2, 16, 16, b.aug.generator, b.aug.p)):
        assert torch.equal(x, y)
    assert b.aug.p == a.aug.p


def test_domain_batches_refuses_a_state_saved_under_another_configuration():
    sd = _batches(world=2, rank=1).state_dict()
    for other in (dict(batch_size=1, world=2, rank=1), dict(world=1, rank=0), dict(world=2, rank=0), dict(world=2, rank=1, lengths=(6, 7, 11, 5)),
                  dict(world=2, rank=1, lengths=(6, 7, 11))):
        target = _batches(**other)
        before = target.state_dict()
        with pytest.raises(ValueError, match="DomainBatches.load_state_dict"):
            target.load_state_dict(sd)
        after = target.state_dict()                               # nothing was changed
        assert all(torch.equal(before["generators"][k], after["generators"][k]) for k in before["generators"])
    _batches(world=2, rank=1).load_state_dict(sd)
