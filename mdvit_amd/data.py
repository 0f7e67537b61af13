"""The loader in front of the train step, resident on the device (Datasets/create_dataset.py:119-185 SkinDataset_csv, multi_train_MDViT.py:38-49,106-139).

The reference keeps the stored images (Datasets/process_resize.py: 512 x 512 uint8 .npy files) on disk and, per sample and per step, loads one in a
DataLoader worker, runs A.Resize(img_size, img_size) on the host (img_size is 256 in Configs/multi_train_local.yml), augments, normalises and copies the
batch to the GPU.  A stored sample is 1 MiB and a training set a few thousand samples, so here the whole set is uploaded ONCE (DeviceDataset) and a batch
is an index list, one gather + resize launch (csrc/dataset.hip, ops.gather_resize_u8) and the augmentation kernel that was there already
(mdvit_amd.augment.TrainAug): no worker process, no host image arithmetic and no per-step image traffic over PCIe.  DomainBatches restates the
reference's train-loop sampling on top of it.

Parity status of the resize: the semantics are cv2.resize's INTER_LINEAR (image) and INTER_NEAREST (mask), A.Resize's defaults, restated from OpenCV's
published resize.cpp (the fixed-point path for 8-bit images: coefficients in 1/2048, two >> shifts and a rounding add).  Nothing is imported from OpenCV
and OpenCV is not on the build machine, so like the albumentations pipeline of mdvit_amd/augment.py the semantics are UNPINNED against the library: they
are tested against a second restatement (tests/test_dataset_host.py), byte for byte, not against cv2.  All floating-point work (source coordinates,
coefficients) happens here, once per size, in resize_table; the kernel is integer arithmetic only.
"""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .augment import TrainAug

COEF_BITS = 11          # OpenCV's INTER_RESIZE_COEF_BITS: weights are integers in 1/2048
_SEED_MIX = 1000003


def resize_table(src: int, dst: int) -> torch.Tensor:
    """One axis of the resize src -> dst as the kernel's int32 table [5, dst] (host): rows s0, s1 (source taps), a0, a1 (weights, a0 + a1 = 2048), sn (nearest tap).
    Linear, per output position d:  fx = float32((d + 0.5) src / dst - 0.5) with the product in double, s = floor(fx), f = float32(fx - s);  s < 0 -> s = 0, f = 0;
    s >= src - 1 -> s = src - 1, f = 0;  s1 = min(s + 1, src - 1);  a0 = rint((1 - f) 2048), a1 = rint(f 2048) in float32, half to even.
    Nearest:  sn = min(floor(d src / dst), src - 1)."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError(f"resize_table: sizes must be positive (src={src}, dst={dst})")
    d = np.arange(dst, dtype=np.int64)
    fx = ((d.astype(np.float64) + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    fl = np.floor(fx)
    f = (fx - fl).astype(np.float32)
    s = fl.astype(np.int64)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0.0), f).astype(np.float32)
    one, scale = np.float32(1.0), np.float32(1 << COEF_BITS)
    a0, a1 = np.rint((one - f) * scale), np.rint(f * scale)
    sn = np.minimum((d * src) // dst, src - 1)
    return torch.from_numpy(np.stack([s, np.minimum(s + 1, src - 1), a0.astype(np.int64), a1.astype(np.int64), sn]).astype(np.int32))


def _as_u8(a, what: str) -> torch.Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise TypeError(f"DeviceDataset: {what} must be uint8, got {t.dtype}")
    return t


def _binarise(m) -> torch.Tensor:
    """the reference's `np.load(label_path) > 0.5` (create_dataset.py:157), as uint8 {0, 1}"""
    t = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))
    return (t != 0 if not t.is_floating_point() else t > 0.5).to(torch.uint8)


class DeviceDataset:
    """One domain's images uint8 [N,Hs,Ws,3] and masks [N,Hs,Ws] (binarised as the reference does, > 0.5; None: a set without labels) held on the device.
    batch(index) -> (uint8 [B,size,size,3], uint8 [B,size,size] in {0, 1}) on the current stream: the named samples after A.Resize(size, size), in the
    layout TrainAug, ops.augment_normalize_u8 and ops.image_normalize_u8 take.  size: an int or (H, W)."""

    CHUNK_BYTES = 64 << 20          # one pinned staging buffer (two are in flight)

    def __init__(self, images, masks, size: Union[int, Tuple[int, int]], set_id: int, device=None):
        images = _as_u8(images, "images")
        if images.dim() != 4 or images.shape[-1] != 3 or images.shape[0] < 1:
            raise ValueError(f"DeviceDataset: images must be [N,Hs,Ws,3] with N >= 1, got {tuple(images.shape)}")
        if masks is not None and tuple(masks.shape) != tuple(images.shape[:3]):
            raise ValueError(f"DeviceDataset: masks must be {tuple(images.shape[:3])}, got {tuple(masks.shape)}")
        N = images.shape[0]
        per = max(1, self.CHUNK_BYTES // max(1, images[0].numel()))
        chunks = ((s, images[s:s + per], None if masks is None else _binarise(masks[s:s + per])) for s in range(0, N, per))
        self._build(N, tuple(images.shape[1:3]), masks is not None, chunks, size, set_id, device)

    @classmethod
    def from_files(cls, image_paths: Sequence[str], label_paths: Optional[Sequence[str]], size, set_id: int, device=None) -> "DeviceDataset":
        """over the .npy files the reference stores (Image/<ID>.npy [Hs,Ws,3], Label/<ID>.npy [Hs,Ws]; create_dataset.py:151-162: the image is cast to uint8,
        the label is `> 0.5`).  Files are read a chunk at a time: the set is never held whole on the host."""
        image_paths = list(image_paths)
        if not image_paths or (label_paths is not None and len(label_paths) != len(image_paths)):
            raise ValueError("DeviceDataset.from_files: one label path per image path, at least one image")
        first = np.load(image_paths[0])
        if first.ndim != 3 or first.shape[-1] != 3:
            raise ValueError(f"DeviceDataset.from_files: {image_paths[0]} holds {first.shape}, expected [Hs,Ws,3]")
        per = max(1, cls.CHUNK_BYTES // max(1, first.size))

        def chunks():
            for s in range(0, len(image_paths), per):
                img = np.stack([np.load(p).astype(np.uint8) for p in image_paths[s:s + per]])
                msk = None if label_paths is None else torch.from_numpy(np.stack([(np.load(p) > 0.5).astype(np.uint8) for p in label_paths[s:s + per]]))
                yield s, torch.from_numpy(img), msk

        self = cls.__new__(cls)
        self._build(len(image_paths), tuple(first.shape[:2]), label_paths is not None, chunks(), size, set_id, device)
        return self

    def _build(self, N, src_hw, has_mask, chunks, size, set_id, device):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("DeviceDataset lives on a CUDA(HIP) device; there is no CPU path")
        self.device, self.set_id = device, int(set_id)
        self.size = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
        Hs, Ws = src_hw
        self.images = torch.empty((N, Hs, Ws, 3), device=device, dtype=torch.uint8)
        self.masks = torch.empty((N, Hs, Ws), device=device, dtype=torch.uint8) if has_mask else None
        # the upload, once: through two pinned staging buffers, so the copy of one chunk overlaps the host's preparation of the next
        stage, events, k = [None, None], [None, None], 0
        for start, img, msk in chunks:
            c = img.shape[0]
            if tuple(img.shape[1:]) != (Hs, Ws, 3) or (msk is not None and tuple(msk.shape) != (c, Hs, Ws)):
                raise ValueError(f"DeviceDataset: samples {start}..{start + c - 1} are not {Hs} x {Ws}")
            if img.is_cuda:
                self.images[start:start + c].copy_(img)
                if has_mask:
                    self.masks[start:start + c].copy_(msk)
                continue
            if stage[k] is None or stage[k][0].shape[0] < c:
                stage[k] = (torch.empty((c, Hs, Ws, 3), dtype=torch.uint8).pin_memory(), torch.empty((c, Hs, Ws), dtype=torch.uint8).pin_memory() if has_mask else None)
            elif events[k] is not None:
                events[k].synchronize()          # the buffer's earlier copy has left it
            pi, pm = stage[k]
            pi[:c].copy_(img)
            self.images[start:start + c].copy_(pi[:c], non_blocking=True)
            if has_mask:
                pm[:c].copy_(msk)
                self.masks[start:start + c].copy_(pm[:c], non_blocking=True)
            events[k] = torch.cuda.Event()
            events[k].record()
            k ^= 1
        for ev in events:
            if ev is not None:
                ev.synchronize()
        self.ytab = resize_table(Hs, self.size[0]).to(device)
        self.xtab = resize_table(Ws, self.size[1]).to(device)

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def nbytes(self) -> int:
        """device bytes of the pools"""
        return self.images.numel() + (0 if self.masks is None else self.masks.numel())

    def batch(self, index) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """index: a host int64 tensor or a list.  Anything outside [0, N) raises IndexError before a launch (the kernel does not wrap negative indices)."""
        if torch.is_tensor(index) and index.is_cuda:
            raise TypeError("DeviceDataset.batch takes a HOST index list: it is validated before the launch")
        idx = torch.as_tensor(index, dtype=torch.int64).reshape(-1)
        if idx.numel() == 0:
            raise ValueError("DeviceDataset.batch: an empty index list")
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= len(self):
            raise IndexError(f"DeviceDataset.batch: index {lo if lo < 0 else hi} outside [0, {len(self)})")
        idx = idx.contiguous().pin_memory().to(self.device, non_blocking=True)
        return ops.gather_resize_u8(self.images, self.masks, idx, self.ytab, self.xtab)


class _SequentialLoader:
    """the reference's test loader (multi_train_MDViT.py:44-49: shuffle=False, drop_last=False) over a DeviceDataset, in the form evaluate() takes:
    (uint8 image [B,H,W,3], uint8 label [B,1,H,W], set_id int64 [B] on the host) per batch.  Re-iterable."""

    def __init__(self, dataset: DeviceDataset, batch_size: int):
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self) -> int:
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds, N = self.dataset, len(self.dataset)
        for s in range(0, N, self.batch_size):
            e = min(s + self.batch_size, N)
            img, mask = ds.batch(torch.arange(s, e, dtype=torch.int64))
            yield img, mask.unsqueeze(1), torch.full((e - s,), ds.set_id, dtype=torch.int64)


class DomainBatches:
    """The reference's train-loop sampling (multi_train_MDViT.py:38-43,106-112,129-139) over {name: DeviceDataset}: every domain has its own shuffled
    loader with drop_last=True (the short last batch of a permutation is DROPPED), a step takes the next batch of every domain in order, an exhausted domain
    draws a new permutation and goes on (its position carries over epoch boundaries, as the reference's `train_iters` do), and an epoch is as many steps
    as the longest domain has batches.  Each domain's permutations come from its own torch.Generator (torch.randperm, what the DataLoader's
    RandomSampler draws), seeded from `seed` and the domain's position: two objects with one seed sample alike.

    rank / world: the batches of one permutation are dealt round-robin, batch j to rank j % world; every rank draws the same permutations, so the ranks
    partition each of them without overlap or loss.  A rank that runs out first starts its share of the next permutation, so all ranks take
    len(self) = max over domains of ceil(batches / world) steps per epoch.

    Iterating yields one epoch: per step the list of (image fp32 [B,3,H,W], label fp32 [B,1,H,W], set_id int64 [B] on the host), one per domain, that
    mdvit_train_step / base_train_step / transfuse_train_step take.  The uint8 batch goes through a TrainAug this object owns (p: the probability of every
    transform, p=0: normalisation only; its seed is `aug_seed`).  indices() yields the same steps as {name: index tensor} without touching a device."""

    def __init__(self, datasets: Dict[str, DeviceDataset], batch_size: int, seed: int, rank: int = 0, world: int = 1, p: float = 0.5):
        if not datasets:
            raise ValueError("DomainBatches: no datasets")
        if not 0 <= int(rank) < int(world):
            raise ValueError(f"DomainBatches: rank {rank} outside [0, {world})")
        self.datasets, self.batch_size, self.seed, self.rank, self.world = dict(datasets), int(batch_size), int(seed), int(rank), int(world)
        for name, ds in self.datasets.items():
            if len(ds) // self.batch_size < self.world:
                raise ValueError(f"DomainBatches: domain {name!r} has {len(ds)} samples: fewer than one batch of {self.batch_size} per rank ({self.world})")
        self._gen = {name: torch.Generator().manual_seed((self.seed * _SEED_MIX + k) % (1 << 63)) for k, name in enumerate(self.datasets)}
        self._queue: Dict[str, List[torch.Tensor]] = {name: [] for name in self.datasets}
        self.aug_seed = (self.seed * _SEED_MIX + 1000 + self.rank) % (1 << 63)
        self.aug = TrainAug(p=p, seed=self.aug_seed)

    def __len__(self) -> int:
        return max(-(-(len(ds) // self.batch_size) // self.world) for ds in self.datasets.values())

    def _deal(self, name: str) -> List[torch.Tensor]:
        n, bs = len(self.datasets[name]), self.batch_size
        perm = torch.randperm(n, generator=self._gen[name])
        return [perm[j * bs:(j + 1) * bs] for j in range(self.rank, n // bs, self.world)]

    def next_indices(self) -> Dict[str, torch.Tensor]:
        step = {}
        for name, queue in self._queue.items():
            if not queue:
                queue.extend(self._deal(name))
            step[name] = queue.pop(0)
        return step

    def indices(self) -> Iterator[Dict[str, torch.Tensor]]:
        for _ in range(len(self)):
            yield self.next_indices()

    def __iter__(self):
        for step in self.indices():
            out = []
            for name, idx in step.items():
                ds = self.datasets[name]
                img, mask = ds.batch(idx)
                image, label = self.aug(img, mask)
                out.append((image, label, torch.full((idx.numel(),), ds.set_id, dtype=torch.int64)))
            yield out

    def state_dict(self) -> dict:
        """Where the sampling stands: every domain's generator state and the batches of its current permutation that are still queued (positions carry over
        epoch boundaries, so both are needed), TrainAug's state, and the configuration the index stream depends on -- batch size, rank, world, the domains'
        names and lengths -- which load_state_dict checks.  With several ranks every rank saves and loads its own: the queues are its share of the deal."""
        return {"batch_size": self.batch_size, "rank": self.rank, "world": self.world, "lengths": {name: len(ds) for name, ds in self.datasets.items()},
                "generators": {name: g.get_state() for name, g in self._gen.items()},
                "queues": {name: [t.clone() for t in q] for name, q in self._queue.items()},
                "aug": self.aug.state_dict()}

    def load_state_dict(self, state_dict: dict):
        """raises ValueError, before anything is changed, if the state was saved under another batch size, rank, world, or other domains or dataset lengths"""
        mine = {"batch_size": self.batch_size, "rank": self.rank, "world": self.world, "lengths": {name: len(ds) for name, ds in self.datasets.items()}}
        for key, have in mine.items():
            if state_dict[key] != have or (key == "lengths" and list(state_dict[key]) != list(have)):
                raise ValueError(f"DomainBatches.load_state_dict: the state was saved with {key} = {state_dict[key]}, this object has {have}")
        for name, g in self._gen.items():
            g.set_state(state_dict["generators"][name])
        self._queue = {name: [torch.as_tensor(t, dtype=torch.int64).clone() for t in state_dict["queues"][name]] for name in self.datasets}
        self.aug.load_state_dict(state_dict["aug"])

    def eval_loaders(self, batch_size: Optional[int] = None) -> Dict[str, Iterable]:
        """{name: sequential, unshuffled loader that keeps its short last batch} over the same datasets, for evaluate()"""
        bs = self.batch_size if batch_size is None else int(batch_size)
        return {name: _SequentialLoader(ds, bs) for name, ds in self.datasets.items()}
