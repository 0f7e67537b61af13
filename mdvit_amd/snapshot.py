"""Snapshots and resumable training state (csrc/snapshot.hip).

The reference saves with `torch.save(model.state_dict(), best_model_dir)` at the start and on every IoU improvement (multi_train_MDViT.py): one
device-to-host copy and one synchronisation per tensor, 608 (MDViT, MLPFM) to 1460 of them, in the middle of the train loop.  DeviceSnapshot does what the
optimizer does for its update: a device table over the tensors, built once, and ONE launch that packs them into a flat staging buffer, followed by ONE copy
into pinned host memory on a side stream.  take() returns without synchronising; the step goes on while the copy drains.

TrainState is the whole resumable state of a run in one file: the model, the optimizer's state in torch.optim's format, the scheduler, the sampler and
augmentation generators, and the state of the dropout keys."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

CHUNK_BYTES = 131072          # one table row per 128 KiB of a tensor: the optimizer's 32768-element chunk (optim.FusedAdamW._CHUNK) in bytes
SLOT_ALIGN = 16               # every tensor's slot in the flat buffer starts on a 16-byte boundary


def table_layout(nbytes: Sequence[int], chunk: int = CHUNK_BYTES) -> Tuple[List[int], List[Tuple[int, int, int]], int]:
    """The flat buffer's layout for tensors of the given byte sizes, without touching a device: -> (offsets, rows, total).  offsets[i]: tensor i's slot, a
    multiple of 16, slots in order and back to back (each padded to 16 bytes);  rows: (tensor, byte offset inside the tensor, bytes <= chunk), none for an
    empty tensor;  total: the sum of the padded sizes."""
    if chunk <= 0 or chunk % SLOT_ALIGN:
        raise ValueError(f"table_layout: the chunk must be a positive multiple of {SLOT_ALIGN}, got {chunk}")
    offsets, rows, total = [], [], 0
    for i, n in enumerate(nbytes):
        n = int(n)
        if n < 0:
            raise ValueError(f"table_layout: tensor {i} has {n} bytes")
        offsets.append(total)
        rows.extend((i, c0, min(chunk, n - c0)) for c0 in range(0, n, chunk))
        total += (n + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
    return offsets, rows, total


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


class DeviceSnapshot:
    """A fixed set of named device tensors -- a model's state_dict() entries, parameters and buffers of any dtype, optionally an optimizer's flat moment
    buffers -- that can be copied to the host, or written back, as one piece.  Names that alias one tensor (a module registered under several names) share
    a slot.

    take(): one pack launch on the current stream into a device staging buffer, then one device-to-host copy into pinned memory on a side stream, ordered
    after the pack by an event.  No synchronisation: work enqueued after take() -- the optimizer step that overwrites the weights -- does not disturb it.
    wait() / state_dict(): CPU tensors under the original names, VIEWS of the pinned buffer: valid until the next take() or restore(); clone what must live longer.
    restore(state_dict): the inverse, one host-to-device copy and one unpack launch, then ops.mark_weights_updated() -- the tensors were written through raw
    pointers, which autograd's version counters do not see (what FusedAdamW.step does for the same reason).
    There is ONE staging pair: a take() or restore() while an earlier take() is still in flight waits for it first."""

    def __init__(self, tensors: Dict[str, torch.Tensor]):
        if not tensors:
            raise ValueError("DeviceSnapshot: no tensors")
        self.names = list(tensors)
        first = next(iter(tensors.values()))
        if not first.is_cuda:
            raise ValueError("DeviceSnapshot packs device tensors; there is no CPU path")
        self.device = first.device
        uniq, self._slot_of, seen = [], {}, {}
        for name, t in tensors.items():
            if not torch.is_tensor(t) or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"DeviceSnapshot: {name!r} must be a contiguous tensor on {self.device}")
            key = (t.data_ptr(), t.dtype, tuple(t.shape)) if t.numel() else ("empty", name)
            if key not in seen:
                seen[key] = len(uniq)
                uniq.append(t.detach())
            self._slot_of[name] = seen[key]
        self._tensors = uniq          # (kept alive: the table holds their addresses)
        self.offsets, rows, self.total = table_layout([_nbytes(t) for t in uniq])
        self.n_rows = len(rows)
        self.table = torch.tensor([[uniq[i].data_ptr() + c0, self.offsets[i] + c0, n] for i, c0, n in rows], dtype=torch.int64, device=self.device).reshape(-1, 3)
        size = max(self.total, SLOT_ALIGN)
        self.staging = torch.empty(size, dtype=torch.uint8, device=self.device)
        self.pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
        biggest = max((n for _, _, n in rows), default=0)
        self.blocks = int(min(8, max(1, (biggest // 16 + 255) // 256)))
        self.stream = torch.cuda.Stream(self.device)
        self._packed, self._copied = torch.cuda.Event(), torch.cuda.Event()
        self._in_flight = False

    @property
    def nbytes(self) -> int:
        """bytes one take() packs (and copies to the host)"""
        return self.total

    def _view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        i = self._slot_of[name]
        t = self._tensors[i]
        if t.numel() == 0:
            return torch.empty(t.shape, dtype=t.dtype, device=flat.device)
        return flat[self.offsets[i]:self.offsets[i] + _nbytes(t)].view(t.dtype).view(t.shape)

    def take(self):
        from . import ops
        from ._lib import call
        self.wait()
        if self.n_rows:
            call("mdvit_table_pack", self.table.data_ptr(), self.n_rows, self.staging.data_ptr(), self.blocks, ops._stream())
        self._packed.record()
        self.stream.wait_event(self._packed)
        with torch.cuda.stream(self.stream):
            self.pinned.copy_(self.staging, non_blocking=True)
            self._copied.record()
        self._in_flight = True

    def wait(self):
        """block the host until the last take()'s copy (or the last restore()'s upload) has left the pinned buffer"""
        if self._in_flight:
            self._copied.synchronize()
            self._in_flight = False

    def state_dict(self) -> Dict[str, torch.Tensor]:
        self.wait()
        return {name: self._view(self.pinned, name) for name in self.names}

    def restore(self, state_dict: Dict[str, torch.Tensor]):
        from . import ops
        from ._lib import call
        missing = [n for n in self.names if n not in state_dict]
        extra = [n for n in state_dict if n not in self._slot_of]
        if missing or extra:
            raise KeyError(f"DeviceSnapshot.restore: missing {missing[:5]}, unexpected {extra[:5]}")
        for name in self.names:
            t, src = self._tensors[self._slot_of[name]], state_dict[name]
            if tuple(src.shape) != tuple(t.shape) or src.dtype != t.dtype:
                raise ValueError(f"DeviceSnapshot.restore: {name!r} is {tuple(src.shape)} {src.dtype}, the snapshot holds {tuple(t.shape)} {t.dtype}")
        self.wait()
        done = set()
        for name in self.names:
            if self._slot_of[name] not in done and self._tensors[self._slot_of[name]].numel():
                done.add(self._slot_of[name])
                self._view(self.pinned, name).copy_(state_dict[name])
        self.staging.copy_(self.pinned, non_blocking=True)
        if self.n_rows:
            call("mdvit_table_unpack", self.table.data_ptr(), self.n_rows, self.staging.data_ptr(), self.blocks, ops._stream())
        self._copied.record()
        self._in_flight = True          # the upload reads the pinned buffer: the next host write into it waits
        ops.mark_weights_updated()


class TrainState:
    """Everything a run needs to go on where it stopped, in one torch.save file:
      model       the state_dict (DeviceSnapshot: one launch, one copy)
      optimizer   FusedAdamW / FusedAdam.state_dict in torch.optim's format, integer keys in `[p for p in model.parameters() if p.requires_grad]` order: a
                  torch.optim.AdamW / Adam over model.parameters() loads it as it is
      scheduler   StepLR.state_dict
      batches     DomainBatches.state_dict: sampler generators, queued batches, TrainAug's generator
      rng         ops.rng_state(): the dropout / DropPath key counter, torch's initial seed, the device seed words if enabled
      epoch, extra   the caller's: extra holds plain data (numbers, strings, lists, dicts, tensors)
    save_model(path) writes exactly what the reference's `torch.save(model.state_dict(), best_model_dir)` writes: the reference's test() or another framework
    loads it with load_state_dict(torch.load(path)).

    Several GPUs: every rank saves and loads its OWN file -- its sampler state (its share of each permutation) and its augmentation generator are its own.
    The weights and the optimizer state are replicated, so any rank's file holds them; nothing coordinates the ranks here."""

    def __init__(self, model: torch.nn.Module, optimizer=None, scheduler=None, batches=None):
        self.model, self.optimizer, self.scheduler, self.batches = model, optimizer, scheduler, batches
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.snapshot = DeviceSnapshot(dict(model.state_dict()))
        self._opt_snapshot = None
        if optimizer is not None:
            flats = {f"exp_avg.{i}": b for i, b in enumerate(optimizer.exp_avg)}
            flats.update({f"exp_avg_sq.{i}": b for i, b in enumerate(optimizer.exp_avg_sq)})
            flats["step"] = optimizer.step_dev
            self._opt_snapshot = DeviceSnapshot(flats)

    def _model_state(self) -> Dict[str, torch.Tensor]:
        """own CPU copies of the last take(); aliased names keep sharing one tensor, as in model.state_dict()"""
        views, out, own = self.snapshot.state_dict(), {}, {}
        for name, v in views.items():
            slot = self.snapshot._slot_of[name]
            if slot not in own:
                own[slot] = v.clone()
            out[name] = own[slot]
        return out

    def save_model(self, path):
        self.snapshot.take()
        torch.save(self._model_state(), path)

    def save(self, path, epoch: int = 0, extra=None):
        from . import ops
        self.snapshot.take()
        if self._opt_snapshot is not None:
            self._opt_snapshot.take()
        state = {"epoch": int(epoch), "extra": extra, "model": self._model_state(), "rng": ops.rng_state()}
        if self.optimizer is not None:
            flat, n = self._opt_snapshot.state_dict(), len(self.optimizer.exp_avg)
            state["optimizer"] = self.optimizer.state_dict(self.params, _flat=([flat[f"exp_avg.{i}"] for i in range(n)], [flat[f"exp_avg_sq.{i}"] for i in range(n)]),
                                                           _step=float(flat["step"][0]))
        if self.scheduler is not None:
            state["scheduler"] = self.scheduler.state_dict()
        if self.batches is not None:
            state["batches"] = self.batches.state_dict()
        torch.save(state, path)

    def load(self, path) -> dict:
        """restores every part this object was built with (a file without one of them is a KeyError) -> {'epoch', 'extra'}"""
        from . import ops
        state = torch.load(path, map_location="cpu", weights_only=True)
        self.snapshot.restore(state["model"])
        if self.optimizer is not None:
            self.optimizer.load_state_dict(state["optimizer"], self.params)
        if self.scheduler is not None:
            self.scheduler.load_state_dict(state["scheduler"])          # (after the optimizer: it re-applies the learning rate)
        if self.batches is not None:
            self.batches.load_state_dict(state["batches"])
        ops.set_rng_state(state["rng"])
        return {"epoch": state["epoch"], "extra": state["extra"]}
