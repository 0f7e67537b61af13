"""FusedAdam against torch.optim.Adam, mdvit_adam_step(mode=0) against mdvit_adamw_step bit for bit, and the optimizer state in torch.optim's format
going both ways between FusedAdamW / FusedAdam and torch.optim.AdamW / Adam."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-6          # the bound of test_fused_adamw_matches_torch_adamw (tests/test_gpu_kernels.py): both optimizers share the update expression
SHAPES = [(64, 33), (7,), (320, 1, 3, 3), (1,), (513,), (128, 64)]          # those of that test
# The moments: the kernel forms 1 - beta in fp32 from the fp32 beta, torch in double.  1 - fl32(0.999) = 9.9998713e-04, 1.29e-5 (relative) below 0.001, so every
# exp_avg_sq is that much below torch's (1 - fl32(0.9) is 2.4e-7 off 0.1); the parameters see it through sqrt(v) in a term that is itself lr-sized.  2e-5 covers the
# 1.29e-5 plus fp32 rounding; it is the existing AdamW kernel's arithmetic, which must not move.
MOMENT_TOL = 2e-5
# the state exchange: two pairs of equal shapes, so that a permuted `params` still loads and only the values can tell
XSHAPES = [(64, 33), (7,), (7,), (320, 1, 3, 3), (1,), (513,), (128, 64), (64, 33)]


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def check(a, b, tol, name=""):
    assert a.shape == b.shape, f"{name}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = relerr(a, b)
    assert math.isfinite(e) and e <= tol, f"{name}: rel-to-max error {e:.3e} > {tol}"


def make_params(shapes, seed=200):
    ps = [torch.nn.Parameter(rnd(*sh, seed=seed + i).to(dev())) for i, sh in enumerate(shapes)]
    return ps, [torch.nn.Parameter(p.detach().clone()) for p in ps]


def grads(shapes, step):
    return [rnd(*sh, seed=300 + 10 * step + i).to(dev()) for i, sh in enumerate(shapes)]


def fused_step(acc, opt, ps, gs):
    acc.zero()
    acc.begin_sweep(True)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    acc.end_sweep(True)                      # folds p.grad into the buckets, re-points p.grad at the bucket views
    opt.step()


def torch_step(ref, qs, gs):
    for q, g in zip(qs, gs):
        q.grad = g.clone()
    ref.step()


@pytest.mark.parametrize("weight_decay", [0.0, 0.05])
def test_fused_adam_matches_torch_adam(weight_decay):
    """4 steps, a StepLR change in between, odd sizes and one tensor of 32768 + 5 elements (a chunk boundary of the table with a scalar tail)"""
    from mdvit_amd.optim import FusedAdam, StepLR
    from mdvit_amd.parallel import GradAccumulator
    shapes = SHAPES + [(32768 + 5,)]
    ps, qs = make_params(shapes)
    acc = GradAccumulator(ps, bucket_bytes=4096)
    opt = FusedAdam(acc, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    ref = torch.optim.Adam(qs, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    assert opt.n_rows == len(shapes) + 1
    sch, rsch = StepLR(opt, step_size=2, gamma=0.5), torch.optim.lr_scheduler.StepLR(ref, step_size=2, gamma=0.5)
    for step in range(4):
        gs = grads(shapes, step)
        fused_step(acc, opt, ps, gs)
        torch_step(ref, qs, gs)
        sch.step(); rsch.step()
        assert abs(sch.get_last_lr()[0] - rsch.get_last_lr()[0]) < 1e-12
    assert float(opt.step_dev[0]) == 4.0
    for i, (p, q) in enumerate(zip(ps, qs)):
        check(p.detach(), q.detach(), TOL, name=f"param {i} after 4 steps")
        check(opt._moment(opt.exp_avg, p), ref.state[q]["exp_avg"], MOMENT_TOL, name=f"exp_avg {i}")
        check(opt._moment(opt.exp_avg_sq, p), ref.state[q]["exp_avg_sq"], MOMENT_TOL, name=f"exp_avg_sq {i}")


def test_fused_adam_defaults_are_torch_adams():
    from mdvit_amd.optim import FusedAdam, FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    ps, _ = make_params([(5,)])
    opt = FusedAdam(GradAccumulator(ps))
    assert (opt.param_groups[0]["lr"], opt.betas, opt.eps, opt.weight_decay) == (1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert isinstance(opt, FusedAdamW) and "every step" in FusedAdam.__doc__


def test_adam_step_mode_0_is_adamw_step_bit_for_bit():
    """the two C entries on cloned state: parameters and both moments torch.equal after 3 steps (vector path, chunked rows and scalar tails)"""
    from mdvit_amd import ops
    from mdvit_amd._lib import call
    from mdvit_amd.optim import FusedAdamW
    from mdvit_amd.parallel import GradAccumulator
    shapes = SHAPES + [(32768 + 5,)]
    ps, qs = make_params(shapes)
    accs = [GradAccumulator(ps, bucket_bytes=4096), GradAccumulator(qs, bucket_bytes=4096)]
    opts = [FusedAdamW(a, lr=1e-2, weight_decay=0.05) for a in accs]
    for step in range(3):
        gs = grads(shapes, step)
        for k, (acc, opt, params) in enumerate(zip(accs, opts, (ps, qs))):
            acc.zero()
            for p, g in zip(params, gs):
                acc.view_of(p).copy_(g)
            head = (C.c_void_p(opt.table.data_ptr()), opt.n_rows, opt.blocks, C.c_void_p(opt.lr_dev.data_ptr()), C.c_void_p(opt.step_dev.data_ptr()), 0.9, 0.999, 1e-8, 0.05, 0)
            if k == 0:
                call("mdvit_adamw_step", *head, ops._stream())
            else:
                call("mdvit_adam_step", *head, 0, ops._stream())
    ops.mark_weights_updated()
    assert float(opts[0].step_dev[0]) == float(opts[1].step_dev[0]) == 3.0
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert torch.equal(p.detach(), q.detach()), i
        assert not torch.equal(p.detach(), rnd(*shapes[i], seed=200 + i).to(dev())), i
    for a, b in zip(opts[0].exp_avg + opts[0].exp_avg_sq, opts[1].exp_avg + opts[1].exp_avg_sq):
        assert torch.equal(a, b)


PAIRS = [("FusedAdamW", torch.optim.AdamW, 0.05), ("FusedAdam", torch.optim.Adam, 0.05)]


ACC_ORDER = [3, 0, 6, 1, 7, 5, 2, 4]          # the order the accumulator is handed the parameters in: not the order of `params`


def _fused(name, ps, **kw):
    from mdvit_amd import optim
    from mdvit_amd.parallel import GradAccumulator
    acc = GradAccumulator([ps[i] for i in ACC_ORDER], bucket_bytes=4096, late=[ps[5]])          # its own order, and a late class on top
    assert len(acc.reducer.buckets) > 2 and [id(p) for p in acc.params] != [id(p) for p in ps]          # several buckets, and an order that is not `params`'
    return acc, getattr(optim, name)(acc, **kw)


def _worst(ps, qs):
    return max(relerr(p, q) for p, q in zip(ps, qs))


@pytest.mark.parametrize("name,torch_cls,wd", PAIRS)
def test_fused_optimizer_loads_a_torch_state_dict(name, torch_cls, wd):
    """torch runs 2 steps, the fused optimizer loads its state_dict, both run 2 more; a permuted `params` loads too (equal shapes) and must NOT agree"""
    ps, qs = make_params(XSHAPES)
    ref = torch_cls(qs, lr=1e-2, weight_decay=wd)
    for step in range(2):
        torch_step(ref, qs, grads(XSHAPES, step))
    sd = copy.deepcopy(ref.state_dict())          # (torch hands out, and on load keeps, the live `step` tensors: every user below gets its own copy)
    swapped = [7, 2, 1, 3, 4, 5, 6, 0]
    results = {}
    for label, order in (("right", list(range(len(ps)))), ("permuted", swapped)):
        ps_ = [torch.nn.Parameter(q.detach().clone()) for q in qs]
        qs_ = [torch.nn.Parameter(q.detach().clone()) for q in qs]
        ref_ = torch_cls(qs_, lr=1e-2, weight_decay=wd)
        ref_.load_state_dict(copy.deepcopy(sd))
        acc, opt = _fused(name, ps_, lr=1e-3, weight_decay=0.5, betas=(0.5, 0.5), eps=1e-3)          # every hyper-parameter comes from the state
        ptrs = [t.data_ptr() for t in [opt.step_dev, opt.lr_dev] + opt.exp_avg + opt.exp_avg_sq]
        opt.load_state_dict(sd, [ps_[i] for i in order])
        assert ptrs == [t.data_ptr() for t in [opt.step_dev, opt.lr_dev] + opt.exp_avg + opt.exp_avg_sq]
        assert float(opt.step_dev[0]) == 2.0 and float(opt.lr_dev[0]) == np.float32(1e-2) and opt.param_groups[0]["lr"] == 1e-2
        assert (opt.betas, opt.eps, opt.weight_decay) == ((0.9, 0.999), 1e-8, wd)
        for step in range(2, 4):
            gs = grads(XSHAPES, step)
            fused_step(acc, opt, ps_, gs)
            torch_step(ref_, qs_, gs)
        results[label] = _worst(ps_, qs_)
    print(f"{name}: worst rel-to-max error after load + 2 steps: {results}")
    assert results["right"] <= TOL, results
    assert results["permuted"] > 100 * TOL, f"the comparison does not see the parameter order: {results}"


@pytest.mark.parametrize("name,torch_cls,wd", PAIRS)
def test_torch_optimizer_loads_a_fused_state_dict(name, torch_cls, wd):
    ps, _ = make_params(XSHAPES)
    acc, opt = _fused(name, ps, lr=1e-2, weight_decay=wd)
    for step in range(2):
        fused_step(acc, opt, ps, grads(XSHAPES, step))
    results = {}
    for label, order in (("right", list(range(len(ps)))), ("permuted", [7, 2, 1, 3, 4, 5, 6, 0])):
        sd = opt.state_dict([ps[i] for i in order])
        assert sorted(sd) == ["param_groups", "state"] and list(sd["state"]) == list(range(len(ps))) and sd["param_groups"][0]["params"] == list(range(len(ps)))
        g = sd["param_groups"][0]
        assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-2, (0.9, 0.999), 1e-8, wd, False)
        for i, j in enumerate(order):
            s = sd["state"][i]
            assert s["step"].dim() == 0 and s["step"].dtype == torch.float32 and float(s["step"]) == 2.0
            assert s["exp_avg"].shape == ps[j].shape == s["exp_avg_sq"].shape
            assert s["exp_avg"].data_ptr() != opt._moment(opt.exp_avg, ps[j]).data_ptr()          # a copy
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        ref = torch_cls(qs, lr=0.5, weight_decay=0.3)
        ref.load_state_dict(sd)
        # the fused optimizer goes on from a copy of itself, so that both orders start from the same point
        ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        acc2, opt2 = _fused(name, ps2, lr=1e-2, weight_decay=wd)
        opt2.load_state_dict(opt.state_dict(ps), ps2)
        for step in range(2, 4):
            gs = grads(XSHAPES, step)
            fused_step(acc2, opt2, ps2, gs)
            torch_step(ref, qs, gs)
        results[label] = _worst(ps2, qs)
    print(f"{name}: worst rel-to-max error after torch's load + 2 steps: {results}")
    assert results["right"] <= TOL, results
    assert results["permuted"] > 100 * TOL, f"the comparison does not see the parameter order: {results}"


def test_state_dict_round_trip_is_exact_and_a_fresh_state_is_step_zero():
    ps, _ = make_params(XSHAPES)
    acc, opt = _fused("FusedAdamW", ps, lr=1e-2)
    sd0 = opt.state_dict(ps)
    assert all(float(s["step"]) == 0.0 and not bool(s["exp_avg"].any()) for s in sd0["state"].values())
    for step in range(2):
        fused_step(acc, opt, ps, grads(XSHAPES, step))
    sd = opt.state_dict(ps)
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    acc2, opt2 = _fused("FusedAdamW", ps2, lr=1.0)
    opt2.load_state_dict(sd, ps2)
    for a, b in zip(opt.exp_avg + opt.exp_avg_sq + [opt.step_dev, opt.lr_dev], opt2.exp_avg + opt2.exp_avg_sq + [opt2.step_dev, opt2.lr_dev]):
        assert torch.equal(a, b)
    opt2.load_state_dict({"state": {}, "param_groups": sd["param_groups"]}, ps2)          # what torch writes before its first step
    assert float(opt2.step_dev[0]) == 0.0 and not any(bool(b.any()) for b in opt2.exp_avg + opt2.exp_avg_sq)


def test_load_state_dict_refusals_leave_the_state_alone():
    ps, _ = make_params(XSHAPES)
    acc, opt = _fused("FusedAdamW", ps, lr=1e-2)
    for step in range(2):
        fused_step(acc, opt, ps, grads(XSHAPES, step))
    good = opt.state_dict(ps)
    before = [t.clone() for t in opt.exp_avg + opt.exp_avg_sq + [opt.step_dev, opt.lr_dev]]

    def mutated(fn):
        sd = copy.deepcopy(good)
        fn(sd)
        return sd

    cases = {
        "step counts differ": mutated(lambda sd: sd["state"][3].__setitem__("step", torch.tensor(5.0))),
        "a parameter without state": mutated(lambda sd: sd["state"].pop(2)),
        "amsgrad": mutated(lambda sd: sd["param_groups"][0].__setitem__("amsgrad", True)),
        "maximize": mutated(lambda sd: sd["param_groups"][0].__setitem__("maximize", True)),
        "two groups": mutated(lambda sd: sd["param_groups"].append(copy.deepcopy(sd["param_groups"][0]))),
        "shape": mutated(lambda sd: sd["state"][1].__setitem__("exp_avg", torch.zeros(8))),
        "shape sq": mutated(lambda sd: sd["state"][0].__setitem__("exp_avg_sq", torch.zeros(33, 64))),
        "count": mutated(lambda sd: sd["param_groups"][0].__setitem__("params", list(range(7)))),
    }
    for what, sd in cases.items():
        with pytest.raises(ValueError, match="load_state_dict"):
            opt.load_state_dict(sd, ps)
        for a, b in zip(before, opt.exp_avg + opt.exp_avg_sq + [opt.step_dev, opt.lr_dev]):
            assert torch.equal(a, b), what
    for bad in (ps[:-1], ps + [ps[0]], ps[:-1] + [torch.nn.Parameter(torch.zeros(64, 33, device=dev()))], ps[:-1] + [ps[0]]):
        with pytest.raises(ValueError, match="params"):
            opt.state_dict(bad)
        with pytest.raises(ValueError, match="params"):
            opt.load_state_dict(good, bad)
    opt.load_state_dict(good, ps)
