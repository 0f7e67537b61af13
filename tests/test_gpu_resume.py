"""An interrupted run goes on as the uninterrupted one does (mdvit_amd.snapshot.TrainState): BASE through base_train_step and MDViT (MLPFM) through
mdvit_train_step, both with FusedAdamW, dropout and DropPath on, a StepLR change, DomainBatches with augmentation.

  run A    4 steps                                     run A'   the same again from the same seed (the control: run-to-run noise)
  run B    2 steps, the scheduler's step, TrainState.save;  FRESH objects from other seeds, one throwaway step on them (weights, caches, counters, generators and
           queues all in a wrong state);  TrainState.load;  2 steps

Bound, per tensor (parameters, BatchNorm buffers, both moments): relative L2 of B against A <= max(4 x that of A' against A, 1e-5).  1e-5 is the project's
run-to-run bound (test_bench_step_gradients_are_reproducible_run_to_run); the factor 4 covers one more process-local run as a source of atomic-order noise.
The sensitivity cases put ONE piece of the saved state back to the fresh objects' own (wrong) value before loading; each must break the bound on at least one
tensor (lr is 1e-2 for that), or the comparison above would not see that piece.

Measured (MI355X), largest per-tensor relative L2:   A' vs A: BASE 0.0, MDViT 0.0   B vs A: BASE 0.0, MDViT 0.0   (the runs agree bit for bit)"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

S, B, N_SAMPLES, LR = 64, 2, 6, 1e-2
FLOOR = 1e-5
PIECES = ("moments", "step", "rng", "sampler", "aug")


def dev():
    return torch.device("cuda:0")


_datasets = {}


def datasets():
    """four synthetic domains of 6 stored samples (80 x 72, resized to 64 x 64 by the dataset), uploaded once and only read"""
    from mdvit_amd.data import DeviceDataset
    if not _datasets:
        for d in range(4):
            g = torch.Generator().manual_seed(900 + d)
            img = torch.randint(0, 256, (N_SAMPLES, 80, 72, 3), generator=g, dtype=torch.uint8)
            yy, xx = torch.meshgrid(torch.arange(80), torch.arange(72), indexing="ij")
            cy, cx = torch.randint(20, 60, (N_SAMPLES, 1, 1), generator=g), torch.randint(20, 52, (N_SAMPLES, 1, 1), generator=g)
            mask = (((yy - cy) ** 2 + (xx - cx) ** 2) < (10 + 3 * d) ** 2).to(torch.uint8)
            _datasets[f"domain{d}"] = DeviceDataset(img, mask, S, set_id=d, device=dev())
    return _datasets


class Run:
    def __init__(self, kind, init_seed, sampler_seed, key_start):
        import mdvit_amd
        from mdvit_amd import ops
        from mdvit_amd.data import DomainBatches
        from mdvit_amd.optim import FusedAdamW, StepLR
        from mdvit_amd.parallel import GradAccumulator
        self.kind = kind
        torch.manual_seed(init_seed)                         # the initial weights AND torch.initial_seed(), which every dropout key mixes in
        ops._key_counter = itertools.count(key_start)
        if kind == "BASE":
            m = mdvit_amd.BASE(img_size=S, drop_rate=0.1, drop_path_rate=0.1, conv_norm=torch.nn.BatchNorm2d, adapt_method=False)
        else:
            m = mdvit_amd.MDViT(img_size=S, drop_rate=0.1, drop_path_rate=0.1, conv_norm=torch.nn.BatchNorm2d, adapt_method="Sup", num_domains=4, decoder_name="MLPFM")
        self.model = m.to(dev()).train()
        self.acc = GradAccumulator(self.model.parameters())
        self.opt = FusedAdamW(self.acc, lr=LR)
        self.sch = StepLR(self.opt, step_size=1)
        self.batches = DomainBatches(datasets(), batch_size=B, seed=sampler_seed, p=0.5)
        self.state = mdvit_amd.TrainState(self.model, self.opt, self.sch, self.batches)
        self._it = None

    def _draw(self):
        """the next step's batches through the public iterator, across epoch ends (an epoch is 3 steps: 6 samples, batches of 2)"""
        while True:
            if self._it is None:
                self._it = iter(self.batches)
            try:
                return next(self._it)
            except StopIteration:
                self._it = None

    def steps(self, n):
        from mdvit_amd.train import base_train_step, mdvit_train_step
        self.acc.attach_sinks(True)
        try:
            for _ in range(n):
                step = base_train_step if self.kind == "BASE" else mdvit_train_step
                step(self.model, self._draw(), optimizer=self.opt, accumulator=self.acc)
            torch.cuda.synchronize()
        finally:
            self.acc.attach_sinks(False)

    def tensors(self):
        out = {"param." + n: p for n, p in self.model.named_parameters()}
        out.update({"buffer." + n: b for n, b in self.model.named_buffers()})
        out.update({"exp_avg." + n: self.opt._moment(self.opt.exp_avg, p) for n, p in self.model.named_parameters()})
        out.update({"exp_avg_sq." + n: self.opt._moment(self.opt.exp_avg_sq, p) for n, p in self.model.named_parameters()})
        return {k: v.detach().double().cpu() for k, v in out.items()}


def uninterrupted(kind):
    r = Run(kind, init_seed=100, sampler_seed=7, key_start=5)
    r.steps(2)
    r.sch.step()
    r.steps(2)
    return r.tensors()


def rel_l2(got, want):
    return {k: float((got[k] - want[k]).norm() / max(float(want[k].norm()), 1e-300)) for k in want}


@pytest.fixture(scope="module", params=["BASE", "MDViT"])
def scenario(request, tmp_path_factory):
    """-> (kind, run A's tensors, the per-tensor bound from A' against A, the checkpoint after step 2 + the scheduler's step)"""
    from mdvit_amd import ops
    kind = request.param
    old_counter, old_seed = ops._key_counter, torch.initial_seed()
    a, a2 = uninterrupted(kind), uninterrupted(kind)
    noise = rel_l2(a2, a)
    first = Run(kind, init_seed=100, sampler_seed=7, key_start=5)
    first.steps(2)
    first.sch.step()
    assert any(len(q) for q in first.batches._queue.values())          # the save falls inside a permutation
    path = str(tmp_path_factory.mktemp("resume") / f"{kind}.pt")
    first.state.save(path, epoch=17, extra={"best_iou": 0.5})
    print(f"\n{kind}: A' vs A, largest per-tensor relative L2 = {max(noise.values()):.3e} ({max(noise, key=noise.get)})")
    yield kind, a, {k: max(4.0 * v, FLOOR) for k, v in noise.items()}, path
    ops._key_counter = old_counter
    torch.manual_seed(old_seed)


def resumed(kind, path, wrong_piece=None, tmp_path=None):
    """fresh objects from other seeds, one throwaway step, load (with one piece of the file put back to the fresh objects' own value if asked), 2 steps"""
    r = Run(kind, init_seed=321, sampler_seed=99, key_start=1000)
    r.steps(1)
    if wrong_piece is not None:
        mine = str(tmp_path / "fresh.pt")
        r.state.save(mine)
        ck, own = torch.load(path, weights_only=True), torch.load(mine, weights_only=True)
        if wrong_piece == "moments":
            for i, s in ck["optimizer"]["state"].items():
                s["exp_avg"], s["exp_avg_sq"] = own["optimizer"]["state"][i]["exp_avg"], own["optimizer"]["state"][i]["exp_avg_sq"]
        elif wrong_piece == "step":
            for i, s in ck["optimizer"]["state"].items():
                s["step"] = own["optimizer"]["state"][i]["step"]
        elif wrong_piece == "rng":
            ck["rng"] = own["rng"]
        elif wrong_piece == "sampler":
            ck["batches"]["generators"], ck["batches"]["queues"] = own["batches"]["generators"], own["batches"]["queues"]
        elif wrong_piece == "aug":
            ck["batches"]["aug"] = own["batches"]["aug"]
        else:
            raise KeyError(wrong_piece)
        path = str(tmp_path / "spliced.pt")
        torch.save(ck, path)
    back = r.state.load(path)
    assert back == {"epoch": 17, "extra": {"best_iou": 0.5}}
    assert r.sch.last_epoch == 1 and r.opt.param_groups[0]["lr"] == LR * 0.5
    r.steps(2)
    return r.tensors()


def test_resumed_run_matches_the_uninterrupted_one(scenario):
    kind, a, bound, path = scenario
    err = rel_l2(resumed(kind, path), a)
    worst = max(err, key=lambda k: err[k] / bound[k])
    print(f"\n{kind}: B vs A, largest per-tensor relative L2 = {max(err.values()):.3e}; worst against its bound: {worst} {err[worst]:.3e} (bound {bound[worst]:.3e})")
    bad = {k: (v, bound[k]) for k, v in err.items() if not v <= bound[k]}
    assert not bad, f"{len(bad)} of {len(err)} tensors differ after the resume: {dict(itertools.islice(bad.items(), 5))}"


@pytest.mark.parametrize("piece", PIECES)
def test_each_piece_of_the_state_is_needed(scenario, piece, tmp_path):
    kind, a, bound, path = scenario
    err = rel_l2(resumed(kind, path, wrong_piece=piece, tmp_path=tmp_path), a)
    over = [k for k, v in err.items() if not v <= bound[k]]
    print(f"\n{kind}: without the saved {piece}: {len(over)} of {len(err)} tensors over the bound, largest relative L2 {max(err.values()):.3e}")
    assert over, f"restoring everything but the {piece} still meets the bound: the comparison does not see this piece"


@pytest.mark.parametrize("kind", ["BASE", "MDViT"])
def test_save_model_writes_what_torch_save_of_the_state_dict_writes(kind, tmp_path):
    import mdvit_amd
    r = Run(kind, init_seed=11, sampler_seed=1, key_start=1)
    with torch.no_grad():
        for b in r.model.buffers():          # buffers away from their initial values, the int64 counters too
            b.add_(3) if not b.is_floating_point() else b.add_(torch.rand_like(b))
    path = str(tmp_path / "best.pth")
    mdvit_amd.TrainState(r.model).save_model(path)
    got, want = torch.load(path, weights_only=True), r.model.state_dict()
    assert list(got) == list(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and not got[k].is_cuda, k
        assert torch.equal(got[k], v.cpu()), k
    assert any(v.dtype == torch.int64 for v in got.values())
    other = Run(kind, init_seed=12, sampler_seed=1, key_start=1).model
    other.load_state_dict(torch.load(path), strict=True)
    for (k, v), w in zip(want.items(), other.state_dict().values()):
        assert torch.equal(v, w), k
