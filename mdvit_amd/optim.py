"""AdamW / Adam + StepLR of the reference's train loop (multi_train_MDViT.py:88-95: optim.AdamW(lr, weight_decay) or, for `train.optimizer.mode: 'adam'`,
optim.Adam(model.parameters(), lr); lr_scheduler.StepLR(step_size=50, gamma=0.5)) as ONE HIP launch per step over every parameter.

FusedAdamW works on a parallel.GradAccumulator: the gradients are the accumulator's flat bucket views, the two moments
are flat buffers with the same layout, and a device table of pointers drives the kernel -- one table row per 32768-element CHUNK
of a parameter (the library slices tables of more than 65535 rows over several launches); the step counter and the
learning rate live in device memory (HIP-graph replay safe).  FusedAdam is the same object with the kernel's other decay rule.

Deviation from torch.optim.AdamW / Adam, by construction: the kernel updates EVERY parameter of the accumulator on every step (gradient =
the bucket view, zero if nothing was accumulated), so a parameter that received no gradient at all in a step is still weight-decayed
and its moments still decay -- torch skips parameters whose .grad is None.  In the train steps of this package every parameter is
reached by the summed loss on every step (checked by the golden gradient-norm tests: no zero-norm entries), so the two agree there.

State.  state_dict(params) / load_state_dict(sd, params) speak torch.optim's format, so a run can move between the two optimizers in either
direction.  `params` is the order the integer keys follow -- the list the reference hands torch.optim, `[p for p in model.parameters() if
p.requires_grad]` -- and has no default: the accumulator's own order is a bucketing order (reversed, late parameters last), and state keyed by it
would load into a torch optimizer without an error and permuted."""
from __future__ import annotations

import ctypes as C

import torch

from . import ops
from ._lib import call
from .parallel import GradAccumulator


class FusedAdamW:
    _CHUNK = 32768
    _MODE = 0                        # mdvit_adam_step's mode: 0 decoupled decay, 1 coupled L2
    _TORCH = torch.optim.AdamW       # the optimizer whose state_dict layout this one speaks

    def __init__(self, accumulator: GradAccumulator, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, zero_grad: bool = False):
        self.acc = accumulator
        self.params = accumulator.params
        if not self.params or not self.params[0].is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs CUDA parameters (there is no CPU fallback)")
        dev = self.params[0].device
        self.betas, self.eps, self.weight_decay, self.zero_grad_after = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay), bool(zero_grad)
        self.exp_avg = [torch.zeros_like(b) for b in accumulator.reducer.buckets]
        self.exp_avg_sq = [torch.zeros_like(b) for b in accumulator.reducer.buckets]
        # one table row per CHUNK of a parameter (<= _CHUNK elements, a multiple of 4 so that a 16-byte aligned tensor stays on the float4 path): the kernel gives every row
        # the same number of workgroups, and with one row per TENSOR the 64 workgroups of the largest weight (4.7 M elements of ~31 M) were still walking it when everything
        # else had long finished -- 236 us per step at 4.2 TB/s, alone on the GPU between the last gradient and the next forward
        rows = []
        self._slot = {}              # id(parameter) -> (bucket, first element, elements) of its moments in the flat buffers
        for p, g in zip(self.params, accumulator.views):
            bi = accumulator.reducer._bucket_of[p]
            off = g.data_ptr() - accumulator.reducer.buckets[bi].data_ptr()
            if not p.is_contiguous():
                raise RuntimeError(f"{type(self).__name__} needs contiguous parameters")
            m0, v0, n = self.exp_avg[bi].data_ptr() + off, self.exp_avg_sq[bi].data_ptr() + off, p.numel()
            self._slot[id(p)] = (bi, off // 4, n)
            for c0 in range(0, n, self._CHUNK):
                rows.append([p.data_ptr() + 4 * c0, g.data_ptr() + 4 * c0, m0 + 4 * c0, v0 + 4 * c0, min(self._CHUNK, n - c0)])
        self.n_rows = len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.lr_dev = torch.tensor([float(lr)], dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.param_groups = [{"lr": float(lr), "params": self.params}]      # what lr schedulers read and write
        self._lr_host = float(lr)
        biggest = min(self._CHUNK, max(p.numel() for p in self.params))
        self.blocks = int(min(8, max(1, (biggest // 4 + 255) // 256)))

    def set_lr(self, lr: float):
        """host-side schedule -> device scalar (one tiny H2D copy, outside any captured region)"""
        self._lr_host = float(lr)
        self.param_groups[0]["lr"] = float(lr)
        self.lr_dev.fill_(float(lr))

    def zero_grad(self, set_to_none: bool = True):
        self.acc.zero()

    def step(self):
        if self.param_groups[0]["lr"] != self._lr_host and not torch.cuda.is_current_stream_capturing():
            self.set_lr(self.param_groups[0]["lr"])          # a torch scheduler wrote the new rate into param_groups
        self._launch()
        # the kernel wrote the parameters through raw pointers: Tensor._version did not move, so the cached W^T copies and weight
        # planes of the GEMMs are invalidated HERE (they are rebuilt by ops.refresh_transposes() at the start of the next step,
        # or lazily by the first GEMM that touches a weight)
        ops.mark_weights_updated()

    def _launch(self):
        call("mdvit_adamw_step", C.c_void_p(self.table.data_ptr()), self.n_rows, self.blocks, C.c_void_p(self.lr_dev.data_ptr()),
             C.c_void_p(self.step_dev.data_ptr()), self.betas[0], self.betas[1], self.eps, self.weight_decay, int(self.zero_grad_after),
             ops._stream())

    # ---- state in torch.optim's format ---------------------------------------------------------------------------------------------
    def _ordered(self, params):
        """`params` as a list, after checking that it names exactly this optimizer's parameters"""
        params = list(params)
        if len(params) != len(self.params) or {id(p) for p in params} != set(self._slot) or len({id(p) for p in params}) != len(params):
            raise ValueError(f"{type(self).__name__}: `params` must list each of the accumulator's {len(self.params)} parameters once "
                             "([p for p in model.parameters() if p.requires_grad]); its order is the order of the state's integer keys")
        return params

    def _moment(self, flat, p):
        bi, off, n = self._slot[id(p)]
        return flat[bi][off:off + n].view(p.shape)

    def _torch_group(self):
        """the hyper-parameter keys of the installed torch's own param group (they differ between torch versions), filled with this optimizer's values"""
        ref = self._TORCH([torch.nn.Parameter(torch.zeros(1))], lr=self.param_groups[0]["lr"], betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        return ref.state_dict()["param_groups"][0]

    def state_dict(self, params, *, _flat=None, _step=None):
        """{'state': {i: {'step': 0-dim fp32, 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [{'lr', 'betas', 'eps', 'weight_decay', 'amsgrad': False, ...,
        'params': [0..n-1]}]}: what torch.optim.AdamW (FusedAdam: torch.optim.Adam) over `params` returns after the same steps, and what its load_state_dict
        takes.  The moments are copies, shaped like their parameter.  Reads the step counter from the device (one synchronising copy).
        (_flat / _step: host copies of the flat moment buffers and of the counter that a snapshot already holds -- snapshot.TrainState.)"""
        params = self._ordered(params)
        m_flat, v_flat = (self.exp_avg, self.exp_avg_sq) if _flat is None else _flat
        step = float(self.step_dev[0]) if _step is None else float(_step)
        state = {i: {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": self._moment(m_flat, p).clone(), "exp_avg_sq": self._moment(v_flat, p).clone()}
                 for i, p in enumerate(params)}
        group = self._torch_group()
        group["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict, params):
        """The inverse, also for a state_dict that torch.optim.AdamW (FusedAdam: torch.optim.Adam) over `params` wrote.  Moments, step counter and learning rate
        are written IN PLACE (a captured graph holds their addresses); betas, eps and weight_decay are taken over.  Everything is checked before anything is
        written.  Refused: more than one param group, amsgrad / maximize, per-parameter step counts that differ (one device counter serves all parameters
        here), a parameter without state next to others that have it, a moment whose shape is not its parameter's."""
        name = type(self).__name__
        params = self._ordered(params)
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"{name}.load_state_dict: {len(groups)} param groups; one group with one set of hyper-parameters is what the kernel applies")
        group = groups[0]
        for flag in ("amsgrad", "maximize"):
            if group.get(flag, False):
                raise ValueError(f"{name}.load_state_dict: {flag}=True is not built")
        index = list(group["params"])
        if len(index) != len(params):
            raise ValueError(f"{name}.load_state_dict: the state names {len(index)} parameters, `params` has {len(params)}")
        state = state_dict["state"]
        step, moments = 0.0, []
        if len(state):
            missing = [i for i in index if i not in state]
            if missing:
                raise ValueError(f"{name}.load_state_dict: parameters {missing[:8]} have no state while others do: their step counts differ (one counter serves all here)")
            steps = sorted({float(state[i]["step"]) for i in index})
            if len(steps) != 1:
                raise ValueError(f"{name}.load_state_dict: per-parameter step counts differ ({steps[:4]}): one device counter serves all parameters here")
            step = steps[0]
            for i, p in zip(index, params):
                m, v = state[i]["exp_avg"], state[i]["exp_avg_sq"]
                if tuple(m.shape) != tuple(p.shape) or tuple(v.shape) != tuple(p.shape):
                    raise ValueError(f"{name}.load_state_dict: state {i} has moments of shape {tuple(m.shape)} / {tuple(v.shape)}, its parameter is {tuple(p.shape)}")
                moments.append((p, m, v))
        betas = group.get("betas", self.betas)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps, self.weight_decay = float(group.get("eps", self.eps)), float(group.get("weight_decay", self.weight_decay))
        if moments:
            torch._foreach_copy_([self._moment(self.exp_avg, p) for p, _, _ in moments] + [self._moment(self.exp_avg_sq, p) for p, _, _ in moments],
                                 [m.to(p.device, torch.float32) for p, m, _ in moments] + [v.to(p.device, torch.float32) for p, _, v in moments])
        else:
            for b in self.exp_avg + self.exp_avg_sq:
                b.zero_()
        self.step_dev.fill_(step)
        self.set_lr(float(group["lr"]))


class FusedAdam(FusedAdamW):
    """torch.optim.Adam (the reference's `train.optimizer.mode: 'adam'`, multi_train_MDViT.py:88-90: optim.Adam(model.parameters(), lr)) on the same launch:
    weight_decay is the coupled L2 term, g <- g + weight_decay * p before the moments, and defaults to 0 as torch's does.  Everything else is FusedAdamW's: the
    table, the device-side lr / step (StepLR drives it unchanged), zero_grad, the state in torch's format.  The same deviation from torch holds: EVERY
    parameter of the accumulator is updated on every step, also one that received no gradient (torch skips those)."""
    _MODE = 1
    _TORCH = torch.optim.Adam

    def __init__(self, accumulator: GradAccumulator, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, zero_grad: bool = False):
        super().__init__(accumulator, lr, betas, eps, weight_decay, zero_grad)

    def _launch(self):
        call("mdvit_adam_step", C.c_void_p(self.table.data_ptr()), self.n_rows, self.blocks, C.c_void_p(self.lr_dev.data_ptr()),
             C.c_void_p(self.step_dev.data_ptr()), self.betas[0], self.betas[1], self.eps, self.weight_decay, int(self.zero_grad_after),
             self._MODE, ops._stream())


class StepLR:
    """lr = base_lr * gamma ** (epoch // step_size)   (optim.lr_scheduler.StepLR(optimizer, 50, 0.5), multi_train_MDViT.py:95)"""

    def __init__(self, optimizer, step_size: int = 50, gamma: float = 0.5):
        self.opt, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.base_lr = float(optimizer.param_groups[0]["lr"])
        self.last_epoch = 0

    def _apply(self):
        lr = self.base_lr * self.gamma ** (self.last_epoch // self.step_size)
        if hasattr(self.opt, "set_lr"):
            self.opt.set_lr(lr)
        else:
            for g in self.opt.param_groups:
                g["lr"] = lr

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lr": self.base_lr, "step_size": self.step_size, "gamma": self.gamma}

    def load_state_dict(self, state_dict):
        """takes the four values over and re-applies the learning rate they give to the optimizer"""
        self.last_epoch, self.base_lr = int(state_dict["last_epoch"]), float(state_dict["base_lr"])
        self.step_size, self.gamma = int(state_dict["step_size"]), float(state_dict["gamma"])
        self._apply()
