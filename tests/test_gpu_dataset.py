"""The device-resident dataset on the GPU (csrc/dataset.hip through ops.gather_resize_u8, mdvit_amd/data.py) against the numpy restatement of the resize
rules in tests/test_dataset_host.py: BYTE EQUALITY for image and mask, no tolerances -- the kernel is integer arithmetic on host-built tables.  Then end to
end: TrainAug over a DeviceDataset batch, one BASE train step fed from DomainBatches and evaluate() over eval_loaders(), each against the same batches
prepared on the host with the restatement, exactly."""
import numpy as np
import pytest
import torch

from test_dataset_host import SHAPES, rand_pool, restate_resize

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def dev():
    return torch.device("cuda:0")


def index_list(N, B=None):
    """repeats, descends, includes 0 and N - 1"""
    idx = [N - 1, 0, N // 2, N // 2, N - 1, 0] + list(range(N - 1, -1, -1))
    return idx[:B] if B else idx


_cases = {}


def case(shape):
    """pool, index list and the restated batch of one shape: computed once, shared, left unchanged"""
    if shape not in _cases:
        N, Hs, Ws, H, W = shape
        img, mask = rand_pool(100 + Hs * 7 + Ws, N, Hs, Ws)
        idx = index_list(N, 8 if Hs == 512 else None)
        want_img, want_mask = restate_resize(img[idx], mask[idx], H, W)
        for a in (img, mask, want_img, want_mask):
            a.setflags(write=False)
        _cases[shape] = (torch.from_numpy(img.copy()).to(dev()), torch.from_numpy(mask.copy()).to(dev()), idx, want_img, want_mask)
    return _cases[shape]


def tables(Hs, Ws, H, W):
    from mdvit_amd.data import resize_table
    return resize_table(Hs, H).to(dev()), resize_table(Ws, W).to(dev())


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no_mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}_to_{s[3]}x{s[4]}")
def test_gather_resize_equals_the_restatement(shape, with_mask):
    from mdvit_amd import ops
    N, Hs, Ws, H, W = shape
    pool, mpool, idx, want_img, want_mask = case(shape)
    ytab, xtab = tables(Hs, Ws, H, W)
    index = torch.tensor(idx, dtype=torch.int64, device=dev())
    B = len(idx)
    runs = []
    for _ in range(2):
        out = torch.full((B, H, W, 3), SENTINEL, dtype=torch.uint8, device=dev())
        mout = torch.full((B, H, W), SENTINEL, dtype=torch.uint8, device=dev()) if with_mask else None
        got, gmask = ops.gather_resize_u8(pool, mpool if with_mask else None, index, ytab, xtab, out_img=out, out_mask=mout)
        assert got is out and gmask is mout
        runs.append((got.cpu().numpy(), None if gmask is None else gmask.cpu().numpy()))
    diff = int((runs[0][0] != want_img).sum())
    print(f"{shape}: {diff} of {want_img.size} image bytes differ from the restatement")
    assert np.array_equal(runs[0][0], want_img)
    assert np.array_equal(runs[1][0], runs[0][0])
    if with_mask:
        assert np.array_equal(runs[0][1], want_mask) and np.array_equal(runs[1][1], runs[0][1])
    else:
        assert runs[0][1] is None
    # without buffers handed in, the same result in fresh ones
    got, gmask = ops.gather_resize_u8(pool, mpool if with_mask else None, index, ytab, xtab)
    assert np.array_equal(got.cpu().numpy(), want_img) and (gmask is None) == (not with_mask)


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no_mask"])
def test_pool_past_2_to_31_bytes(with_mask):
    """2731 samples of 512 x 512 x 3 are 2 147 745 792 bytes: the last sample starts past 2^31 - 1.  The pool is made on the device; only the two gathered
    samples come back for the restatement."""
    from mdvit_amd import ops
    N, S, T = 2731, 512, 256
    assert (N - 1) * S * S * 3 < 2 ** 31 < N * S * S * 3
    gen = torch.Generator(device=dev()).manual_seed(11)
    pool = torch.randint(0, 256, (N, S, S, 3), generator=gen, dtype=torch.uint8, device=dev())
    mpool = torch.randint(0, 2, (N, S, S), generator=gen, dtype=torch.uint8, device=dev()) if with_mask else None
    idx = [N - 1, N // 2]
    want_img, want_mask = restate_resize(pool[idx].cpu().numpy(), None if mpool is None else mpool[idx].cpu().numpy(), T, T)
    ytab, xtab = tables(S, S, T, T)
    index = torch.tensor(idx, dtype=torch.int64, device=dev())
    runs = []
    for _ in range(2):
        out = torch.full((2, T, T, 3), SENTINEL, dtype=torch.uint8, device=dev())
        mout = torch.full((2, T, T), SENTINEL, dtype=torch.uint8, device=dev()) if with_mask else None
        ops.gather_resize_u8(pool, mpool, index, ytab, xtab, out_img=out, out_mask=mout)
        runs.append((out.cpu().numpy(), None if mout is None else mout.cpu().numpy()))
    assert np.array_equal(runs[0][0], want_img) and np.array_equal(runs[1][0], runs[0][0])
    if with_mask:
        assert np.array_equal(runs[0][1], want_mask) and np.array_equal(runs[1][1], runs[0][1])
    # the plain gather takes the same 64-bit offsets
    yid, xid = tables(S, S, S, S)
    got, gmask = ops.gather_resize_u8(pool, mpool, index, yid, xid)
    assert torch.equal(got, pool[idx]) and (mpool is None or torch.equal(gmask, mpool[idx]))


def test_ops_wrapper_refuses_mismatched_operands():
    from mdvit_amd import _lib, ops
    pool, mpool, idx, _, _ = case(SHAPES[0])
    ytab, xtab = tables(16, 16, 8, 8)
    index = torch.tensor(idx, dtype=torch.int64, device=dev())
    for args in ((pool.cpu(), None, index, ytab, xtab), (pool, mpool[:2], index, ytab, xtab), (pool, mpool, index.int(), ytab, xtab),
                 (pool, mpool, index.cpu(), ytab, xtab), (pool, mpool, index, ytab.long(), xtab), (pool, mpool, index, ytab[:4], xtab),
                 (pool.permute(0, 2, 1, 3), None, index, ytab, xtab)):
        with pytest.raises(_lib.MdvitHipError):
            ops.gather_resize_u8(*args)
    with pytest.raises(_lib.MdvitHipError):
        ops.gather_resize_u8(pool, None, index, ytab, xtab, out_mask=torch.empty((len(idx), 8, 8), dtype=torch.uint8, device=dev()))


# ---- DeviceDataset ------------------------------------------------------------------------------------------------------------------------------------
def test_device_dataset_uploads_in_chunks_binarises_and_validates(monkeypatch):
    from mdvit_amd.data import DeviceDataset
    img, _ = rand_pool(7, 11, 12, 18)
    raw = np.random.default_rng(8).integers(0, 256, (11, 12, 18), dtype=np.uint8)          # masks as stored: 0 / 255 and everything between
    raw[0, 0, :4] = [0, 1, 255, 0]
    monkeypatch.setattr(DeviceDataset, "CHUNK_BYTES", 3 * 12 * 18 * 3)                     # three samples per staging buffer: four chunks, both buffers reused
    ds = DeviceDataset(img, raw, size=8, set_id=2, device=dev())
    assert len(ds) == 11 and ds.set_id == 2 and ds.nbytes == 11 * 12 * 18 * 4 and ds.size == (8, 8)
    assert np.array_equal(ds.images.cpu().numpy(), img)
    assert np.array_equal(ds.masks.cpu().numpy(), (raw > 0.5).astype(np.uint8))
    idx = [10, 0, 3, 3]
    want_img, want_mask = restate_resize(img[idx], (raw[idx] > 0.5).astype(np.uint8), 8, 8)
    for index in (idx, torch.tensor(idx), np.array(idx)):
        got, gmask = ds.batch(index)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want_img) and np.array_equal(gmask.cpu().numpy(), want_mask)
    for bad in ([0, 11], [-1, 2], torch.tensor([3, 1 << 40])):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(TypeError):
        ds.batch(torch.tensor(idx, device=dev()))
    # tensors are taken as they are; a rectangular size; a set without labels
    ds2 = DeviceDataset(torch.from_numpy(img.copy()), None, size=(16, 12), set_id=0, device=dev())
    got, gmask = ds2.batch([1])
    assert gmask is None and np.array_equal(got.cpu().numpy(), restate_resize(img[[1]], None, 16, 12)[0])
    with pytest.raises(TypeError):
        DeviceDataset(img.astype(np.float32), None, size=8, set_id=0, device=dev())


def test_device_dataset_from_files(tmp_path):
    """the .npy files the reference stores: uint8 images, labels of any dtype binarised with > 0.5 (create_dataset.py:156-162)"""
    from mdvit_amd.data import DeviceDataset
    img, mask = rand_pool(9, 5, 16, 16)
    ip, lp = [], []
    for k in range(5):
        ip.append(str(tmp_path / f"img{k}.npy"))
        lp.append(str(tmp_path / f"lab{k}.npy"))
        np.save(ip[-1], img[k])
        np.save(lp[-1], (mask[k] * (0.75 if k % 2 else 255.0)).astype(np.float32 if k % 2 else np.uint8) if k != 4 else mask[k].astype(bool))
    ds = DeviceDataset.from_files(ip, lp, size=8, set_id=1, device=dev())
    assert len(ds) == 5 and np.array_equal(ds.images.cpu().numpy(), img) and np.array_equal(ds.masks.cpu().numpy(), mask)
    want_img, want_mask = restate_resize(img[[4, 0]], mask[[4, 0]], 8, 8)
    got, gmask = ds.batch([4, 0])
    assert np.array_equal(got.cpu().numpy(), want_img) and np.array_equal(gmask.cpu().numpy(), want_mask)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def test_train_aug_over_a_device_batch_is_the_normalised_restatement():
    from mdvit_amd import ops
    from mdvit_amd.augment import TrainAug
    from mdvit_amd.data import DeviceDataset
    img, mask = rand_pool(21, 6, 33, 47)
    ds = DeviceDataset(img, mask, size=16, set_id=0, device=dev())
    idx = [5, 0, 2, 2]
    image, label = TrainAug(p=0.0, seed=1)(*ds.batch(idx))
    want_img, want_mask = restate_resize(img[idx], mask[idx], 16, 16)
    assert torch.equal(image, ops.image_normalize_u8(torch.from_numpy(want_img).to(dev())))
    assert label.dtype == torch.float32 and torch.equal(label.cpu(), torch.from_numpy(want_mask).float().unsqueeze(1))


@pytest.fixture(scope="module")
def two_domains():
    """two domains of 128 x 128 samples (9 and 5 of them) for a 64 x 64 model: (arrays, DeviceDatasets)"""
    from mdvit_amd.data import DeviceDataset
    arrays = {"isic": rand_pool(31, 9, 128, 128) + (0,), "ph2": rand_pool(32, 5, 128, 128) + (1,)}
    return arrays, {name: DeviceDataset(img, mask, size=64, set_id=sid, device=dev()) for name, (img, mask, sid) in arrays.items()}


def base_model():
    import mdvit_amd
    torch.manual_seed(5)
    m = mdvit_amd.BASE(drop_rate=0.0, drop_path_rate=0.0, conv_norm=torch.nn.BatchNorm2d, adapt_method=False)
    return m.to(dev())


@pytest.fixture(scope="module")
def two_steps(two_domains):
    """one base_train_step of BASE at 64 x 64 fed from 128 x 128 pools through DomainBatches (p = 0.5: every augmentation drawn), and the same step from the same
    weights fed batches resized on the host by the restatement, with the same indices and augmentation seed: (batches, loss, gradients) of each"""
    from mdvit_amd.augment import TrainAug
    from mdvit_amd.data import DomainBatches
    from mdvit_amd.train import base_train_step
    arrays, datasets = two_domains
    m = base_model().train()
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def step(batches):
        m.load_state_dict(state)
        out = base_train_step(m, batches, optimizer=None)
        torch.cuda.synchronize()
        return float(out["loss"]), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    db = DomainBatches(datasets, batch_size=2, seed=17, p=0.5)
    device_batches = next(iter(db))
    twin, aug = DomainBatches(datasets, batch_size=2, seed=17, p=0.5), TrainAug(p=0.5, seed=db.aug_seed)
    host_batches = []
    for name, idx in twin.next_indices().items():
        img, mask, sid = arrays[name]
        r_img, r_mask = restate_resize(img[idx.numpy()], mask[idx.numpy()], 64, 64)
        image, label = aug(torch.from_numpy(r_img).to(dev()), torch.from_numpy(r_mask).to(dev()))
        host_batches.append((image, label, torch.full((2,), sid, dtype=torch.int64)))
    return (device_batches,) + step(device_batches), (host_batches,) + step(host_batches)


def test_domain_batches_feed_the_step_the_host_resized_batches_and_loss(two_steps):
    """what DomainBatches hands base_train_step is, bit for bit, the batch resized on the host by the restatement and augmented from the same seed, in the
    form the step takes; the step's loss (a forward whose reductions run in a fixed order) is the same float"""
    (device_batches, loss_d, _), (host_batches, loss_h, _) = two_steps
    assert [tuple(b[0].shape) for b in device_batches] == [(2, 3, 64, 64)] * 2 and [tuple(b[1].shape) for b in device_batches] == [(2, 1, 64, 64)] * 2
    assert [b[2].tolist() for b in device_batches] == [[0, 0], [1, 1]] and not device_batches[0][2].is_cuda
    for a, b in zip(device_batches, host_batches):
        assert a[0].dtype == a[1].dtype == torch.float32
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    print(f"loss from DomainBatches {loss_d!r}, from host-resized batches {loss_h!r}")
    assert np.isfinite(loss_d) and loss_d == loss_h


def test_base_train_step_from_domain_batches_equals_host_resized_batches(two_steps):
    """the same loss and the same gradients BIT FOR BIT: the two steps get bit-identical batches (the test above), so this holds exactly as far as the step
    itself is reproducible.  It needs every weight gradient of BASE's step summed in a fixed order: the stride-2 depthwise one (dwconv3x3_wgrad_kernel,
    csrc/conv.hip) used LDS float atomics, and with them the three patch_embed_stages.{1,2,3}.patch_conv.dwconv.weight gradients differed by up to
    1.06e-7 relative L2 between ANY two runs on one list of batches, while the other 309 tensors were equal; it now sums its token lanes in lane order."""
    (_, loss_d, grads_d), (_, loss_h, grads_h) = two_steps
    assert np.isfinite(loss_d) and loss_d == loss_h
    assert len(grads_d) > 100 and sorted(grads_d) == sorted(grads_h)
    differ = [(float((grads_d[n].double() - grads_h[n].double()).norm() / max(float(grads_h[n].double().norm()), 1e-30)), n)
              for n in grads_d if not torch.equal(grads_d[n], grads_h[n])]
    print(f"{len(differ)} of {len(grads_d)} gradient tensors differ bit for bit (relative L2, name): {sorted(differ, reverse=True)[:6]}")
    assert not differ, differ


def test_evaluate_over_eval_loaders_equals_host_prepared_batches(two_domains):
    """evaluate() over eval_loaders() (sequential, the short last batch kept: 9 = 4 + 4 + 1, 5 = 4 + 1) returns exactly the dict it returns over the same
    batches resized on the host by the restatement"""
    from mdvit_amd.data import DomainBatches
    from mdvit_amd.evaluate import evaluate
    arrays, datasets = two_domains
    m = base_model().eval()
    loaders = DomainBatches(datasets, batch_size=4, seed=0).eval_loaders()
    assert [len(l) for l in loaders.values()] == [3, 2]
    sizes = [[int(b[0].shape[0]) for b in l] for l in loaders.values()]
    assert sizes == [[4, 4, 1], [4, 1]] and sizes == [[int(b[0].shape[0]) for b in l] for l in loaders.values()]          # re-iterable
    host = {}
    for name, (img, mask, sid) in arrays.items():
        host[name] = []
        for s in range(0, len(img), 4):
            r_img, r_mask = restate_resize(img[s:s + 4], mask[s:s + 4], 64, 64)
            host[name].append((torch.from_numpy(r_img), torch.from_numpy(r_mask).float().unsqueeze(1), torch.full((len(r_img),), sid, dtype=torch.int64)))
    got = evaluate(m, loaders, num_domains=4, use_domain_label=False)
    want = evaluate(m, host, num_domains=4, use_domain_label=False)
    print(f"evaluate over eval_loaders: {got}")
    assert got["images"] == [9, 5, 0, 0] and np.isfinite(got["sum_loss"])
    assert got == want
