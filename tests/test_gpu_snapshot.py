"""csrc/snapshot.hip through mdvit_amd.snapshot.DeviceSnapshot: pack / unpack byte for byte over odd sizes, dtypes and alignments, the table slicing past
65535 rows, take()'s ordering against later work on the stream without a synchronisation, and restore() under warm GEMM weight caches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev():
    return torch.device("cuda:0")


def rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def make_set(zero: bool):
    """-> ({name: device tensor}, {name: the larger buffer a view sits in}).  zero: the same set with every tensor zeroed (the buffers around the views keep the sentinel)"""
    bufs = {"view1": torch.full((1 + 513 + 6,), SENTINEL, device=dev()), "view3": torch.full((3 + 32768 + 5 + 9,), SENTINEL, device=dev())}
    t = {f"f{n}": rnd(n, n).to(dev()) for n in (1, 3, 7, 513, 32768 + 5)}                  # 16-byte aligned sources, every tail length
    t["view1"] = bufs["view1"][1:1 + 513]                                                  # element offset 1: only 4-byte aligned
    t["view3"] = bufs["view3"][3:3 + 32768 + 5]                                            # element offset 3, two table rows
    t["view1"].copy_(rnd(513, 21)); t["view3"].copy_(rnd(32768 + 5, 22))
    t["i64"] = torch.tensor(0x0123456789ABCDEF, dtype=torch.int64, device=dev())           # a 0-dim int64, as num_batches_tracked is
    t["u8"] = torch.tensor([1, 2, 3, 254, 255], dtype=torch.uint8, device=dev())
    t["empty"] = torch.empty((0, 4), device=dev())
    t["m2d"] = rnd(6 * 5, 23).view(6, 5).to(dev())
    if zero:
        for v in t.values():
            v.zero_()
    assert t["view1"].data_ptr() % 16 == 4 and t["view3"].data_ptr() % 16 == 12
    return t, bufs


def raw(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def test_pack_is_the_host_side_concatenation_and_unpack_restores_exactly():
    from mdvit_amd.snapshot import DeviceSnapshot, table_layout
    src, _ = make_set(False)
    snap = DeviceSnapshot(src)
    offsets, rows, total = table_layout([v.numel() * v.element_size() for v in src.values()])
    assert (snap.offsets, snap.total, snap.n_rows) == (offsets, total, len(rows)) and all(o % 16 == 0 for o in offsets)
    snap.staging.fill_(0xEE)
    snap.take()
    got = snap.state_dict()
    want = torch.full((total,), 0xEE, dtype=torch.uint8)          # the padding between slots is not written
    for off, v in zip(offsets, src.values()):
        want[off:off + v.numel() * v.element_size()] = raw(v)
    assert torch.equal(snap.pinned[:total], want)
    assert torch.equal(snap.staging.cpu()[:total], want)
    assert list(got) == list(src)
    for name, v in src.items():
        assert got[name].dtype == v.dtype and got[name].shape == v.shape and not got[name].is_cuda, name
        assert torch.equal(got[name], v.cpu()), name
    # unpack into a zeroed twin: every tensor exactly, and not a byte of the buffers around the 4-byte aligned views
    dst, bufs = make_set(True)
    twin = DeviceSnapshot(dst)
    twin.restore(got)
    torch.cuda.synchronize()
    for name, v in src.items():
        assert torch.equal(dst[name], v), name
    assert torch.equal(bufs["view1"][:1].cpu(), torch.full((1,), SENTINEL)) and torch.equal(bufs["view1"][1 + 513:].cpu(), torch.full((6,), SENTINEL))
    assert torch.equal(bufs["view3"][:3].cpu(), torch.full((3,), SENTINEL)) and torch.equal(bufs["view3"][3 + 32768 + 5:].cpu(), torch.full((9,), SENTINEL))
    with pytest.raises(ValueError, match="restore"):
        twin.restore({**got, "u8": torch.zeros(6, dtype=torch.uint8)})
    with pytest.raises(ValueError, match="restore"):
        twin.restore({**got, "i64": torch.tensor(1, dtype=torch.int32)})
    with pytest.raises(KeyError):
        twin.restore({k: v for k, v in got.items() if k != "f7"})


def test_aliased_names_share_a_slot():
    from mdvit_amd.snapshot import DeviceSnapshot
    w = rnd(40, 1).to(dev())
    snap = DeviceSnapshot({"a.weight": w, "b.weight": w, "other": rnd(3, 2).to(dev())})
    assert snap.total == 160 + 16
    snap.take()
    sd = snap.state_dict()
    assert torch.equal(sd["a.weight"], w.cpu()) and sd["a.weight"].data_ptr() == sd["b.weight"].data_ptr()


def test_a_table_of_70000_one_float_rows_is_sliced_past_65535():
    from mdvit_amd.snapshot import DeviceSnapshot
    n = 70000
    base = torch.arange(4 * n, dtype=torch.float32, device=dev())
    snap = DeviceSnapshot({str(i): base[4 * i + 1:4 * i + 2] for i in range(n)})
    assert snap.n_rows == n and snap.total == 16 * n
    snap.staging.zero_()
    snap.take()
    snap.wait()
    flat = snap.pinned[:16 * n].view(torch.float32).view(n, 4)
    assert torch.equal(flat[:, 0], base[1::4].cpu()) and not bool(flat[:, 1:].any())
    out = torch.zeros_like(base)
    twin = DeviceSnapshot({str(i): out[4 * i + 1:4 * i + 2] for i in range(n)})
    twin.restore(snap.state_dict())
    torch.cuda.synchronize()
    want = torch.zeros_like(base)
    want[1::4] = base[1::4]
    assert torch.equal(out, want)


def test_take_does_not_synchronise_and_holds_the_values_before_a_later_step():
    """take(), at once an optimizer step on the same stream that moves every parameter, then wait(): the snapshot holds the values from before the step.  take()
    and the step run under torch's sync debug mode 'error' (the technique of test_update_and_table_do_not_synchronise)."""
    from mdvit_amd.optim import FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    from mdvit_amd.snapshot import DeviceSnapshot
    ps = [torch.nn.Parameter(rnd(n, 30 + i).to(dev())) for i, n in enumerate((4 << 20, 513, 7, 1 << 20))]
    acc = GradAccumulator(ps)
    opt = FusedAdamW(acc, lr=1e-1, weight_decay=0.1)
    for v in acc.views:
        v.fill_(1.0)
    tensors = {f"p{i}": p for i, p in enumerate(ps)}
    tensors.update({f"m{i}": b for i, b in enumerate(opt.exp_avg)})          # the optimizer's flat moment buffers ride along
    snap = DeviceSnapshot(tensors)
    snap.take()          # first use: code objects loaded outside the checked window
    snap.wait()
    opt.step()
    torch.cuda.synchronize()
    before = {k: v.detach().clone() for k, v in tensors.items()}
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        snap.take()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    got = snap.state_dict()
    for k, v in tensors.items():
        assert torch.equal(got[k], before[k].cpu()), k
        assert not torch.equal(v.detach(), before[k]), k          # the step did move it
    # a second take() before the first was consumed waits for it: one staging pair, and the result is the newer state
    snap.take()
    snap.take()
    now = snap.state_dict()
    for k, v in tensors.items():
        assert torch.equal(now[k], v.detach().cpu()), k


def test_restore_under_warm_weight_caches_gives_the_saved_models_forward_bit_for_bit():
    """the GEMMs cache transposes and bf16 planes of the weights; restore() writes the weights through raw pointers and must invalidate them
    (ops.mark_weights_updated): a stale plane would make the next forward the OLD model's, or a mixture"""
    import mdvit_amd
    from mdvit_amd.snapshot import DeviceSnapshot

    def build(seed):
        torch.manual_seed(seed)
        return mdvit_amd.BASE(drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d, adapt_method=False).to(dev()).eval()

    x = rnd(2 * 3 * 64 * 64, 5).view(2, 3, 64, 64).to(dev())
    a, b = build(1), build(2)
    with torch.no_grad():
        for p in a.parameters():          # (the two seeds must not meet in the default-initialised norms either)
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
        ya = a(x).clone()
        yb = b(x).clone()          # b's caches are warm now, with b's weights
        assert torch.equal(a(x), ya) and not torch.equal(ya, yb)
        sa = DeviceSnapshot(dict(a.state_dict()))
        sa.take()
        sb = DeviceSnapshot(dict(b.state_dict()))
        sb.restore(sa.state_dict())
        assert torch.equal(b(x), ya)
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
