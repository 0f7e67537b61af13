"""The validation / test half of an epoch on the device (multi_train_MDViT.py:236-322 validate, :351-408 test; the same loops in multi_train_BASE.py and
multi_train_TransFuse.py:236-260,325-345): per domain the mean over the images of the batch loss (BCE + Dice of the main output) and of the batch Dice /
IoU of the thresholded main and auxiliary outputs, then the reference's logged figures -- the sum of the per-domain losses and the means of the scores.

EvalAccumulator keeps the epoch's state on the device (ops.eval_accumulate: one streaming pass per forward, no device-to-host copy, no sync);
evaluate() drives a model over per-domain loaders and returns EvalAccumulator.result(), the epoch's single copy to the host.  The choice of `best.pth`
(`max_iou`, torch.save; multi_train_MDViT.py:329-335) stays with the caller: compare result()["avg_iou"] on the host.
"""
from __future__ import annotations

import inspect
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import ops

MAX_GROUPS = 16          # domain batches per eval_accumulate call (mdvit_eval_accumulate)
_COLUMNS = ("loss", "dice", "iou", "aux_dice", "aux_iou")


# ------------------------------------------------------------------------------------------------
# planning: which batches share a forward, in which order (pure Python: no tensor is touched)
# ------------------------------------------------------------------------------------------------
def plan_round(batches: Sequence[tuple], fuse_domains: bool = True, max_groups: int = MAX_GROUPS) -> List[list]:
    """One round = the next batch of every loader that still has one.  batches: [(key, size, domain)] in loader order -> the round's forwards, each a list of
    keys.  Batches of EQUAL size and DISTINCT domains share a forward (a domain-batched forward takes equal consecutive domain batches of distinct ids);
    the first key of a size opens its group, later keys join the first group of their size that lacks their domain.  A group of one is a per-domain
    forward: the ragged tails end up there.  Fused forwards come first, then the single ones, both in loader order."""
    if not fuse_domains:
        return [[key] for key, _, _ in batches]
    groups: List[dict] = []
    for key, size, domain in batches:
        for grp in groups:
            if grp["size"] == size and domain not in grp["domains"] and len(grp["keys"]) < max_groups:
                grp["keys"].append(key)
                grp["domains"].add(domain)
                break
        else:
            groups.append({"size": size, "domains": {domain}, "keys": [key]})
    return [g["keys"] for g in groups if len(g["keys"]) > 1] + [g["keys"] for g in groups if len(g["keys"]) == 1]


def _schedule(iterables: Dict, size_of: Callable, domain_of: Callable, fuse_domains: bool):
    """yields the epoch's forwards, each a list of (key, batch).  Without fusing: the reference's order, loader after loader.  With it: the loaders are
    zipped -- every round takes the next batch of each loader that has one left and plan_round groups them."""
    if not fuse_domains:
        for key, it in iterables.items():
            for batch in it:
                yield [(key, batch)]
        return
    iters = {key: iter(it) for key, it in iterables.items()}
    while iters:
        cur = {}
        for key in list(iters):
            try:
                cur[key] = next(iters[key])
            except StopIteration:
                del iters[key]
        for keys in plan_round([(key, size_of(b), domain_of(b)) for key, b in cur.items()], True):
            yield [(key, cur[key]) for key in keys]


def plan_epoch(batch_sizes: Dict, domains: Optional[Dict] = None, fuse_domains: bool = True) -> List[list]:
    """The forwards evaluate() runs for loaders whose batches have these sizes: batch_sizes {key: [size of batch 0, 1, ...]}, domains {key: domain id}
    (default: the key's position) -> [[(key, batch index), ...], ...], one entry per forward, in order."""
    dom = {key: (i if domains is None else domains[key]) for i, key in enumerate(batch_sizes)}
    stand_ins = {key: [(i, int(s), dom[key]) for i, s in enumerate(sizes)] for key, sizes in batch_sizes.items()}
    return [[(key, b[0]) for key, b in step] for step in _schedule(stand_ins, lambda b: b[1], lambda b: b[2], fuse_domains)]


# ------------------------------------------------------------------------------------------------
# model outputs
# ------------------------------------------------------------------------------------------------
def split_outputs(output):
    """what a model's forward returned -> (out, aux):  [out, aux] is the MDViT family (aux is None for a domain without a peer head, mdvit.py:723-724);
    a tensor is the BASE family; a 3-tuple is TransFuse's lateral maps, the last one scored (multi_train_TransFuse.py:240-243)."""
    if isinstance(output, dict) and "seg" in output:
        output = output["seg"]
    if torch.is_tensor(output):
        return output, None
    if isinstance(output, (list, tuple)):
        if len(output) == 2 and torch.is_tensor(output[0]) and (output[1] is None or torch.is_tensor(output[1])):
            return output[0], output[1]
        if len(output) == 3 and all(torch.is_tensor(t) for t in output):
            return output[2], None
    raise TypeError(f"evaluate: cannot tell the logits in a model output of type {type(output).__name__}"
                    + (f" of length {len(output)}" if isinstance(output, (list, tuple)) else ""))


# ------------------------------------------------------------------------------------------------
# the epoch's state
# ------------------------------------------------------------------------------------------------
class EvalAccumulator:
    """acc [D,8] float64 / counts [D,5] int64 (layout: mdvit_eval_accumulate in include/mdvit_hip.h) and the kernels' workspace, all on `device`.
    update() and table() enqueue kernels and return; result() is the one call that copies to the host."""

    def __init__(self, num_domains: int = 4, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("EvalAccumulator lives on a CUDA(HIP) device; there is no CPU path")
        self.num_domains = int(num_domains)
        self.device = device
        self.acc = torch.zeros((self.num_domains, 8), device=device, dtype=torch.float64)
        self.counts = torch.zeros((self.num_domains, 5), device=device, dtype=torch.int64)
        self.ws = torch.empty((ops.eval_ws_bytes(MAX_GROUPS) // 4,), device=device, dtype=torch.int32)
        self.batch_rows = torch.zeros((MAX_GROUPS, 5), device=device, dtype=torch.float32)
        self._table = torch.zeros((self.num_domains + 1, 6), device=device, dtype=torch.float32)

    def reset(self):
        self.acc.zero_()
        self.counts.zero_()
        return self

    def update(self, out, aux, label, domains, images=None):
        """logits of one forward -> the epoch state.  domains: an int (one domain batch) or a sequence of G ids, the forward's consecutive domain batches,
        images their sizes (default: G equal parts).  Returns this call's batch rows [G,5] (loss, dice, iou, aux dice, aux iou), a view of a buffer the
        next update() overwrites."""
        if isinstance(domains, (int, str)):
            domains, images = [int(domains)], [out.shape[0]]
        else:
            domains = [int(d) for d in domains]
            if images is None:
                if not domains or out.shape[0] % len(domains):
                    raise ValueError(f"batch {out.shape[0]} is not {len(domains)} equal domain batches")
                images = [out.shape[0] // len(domains)] * len(domains)
        if len(domains) > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} domain batches per update")
        rows = self.batch_rows[:len(domains)]
        ops.eval_accumulate(out, aux, label, images, domains, self.acc, self.counts, self.ws, rows)
        return rows

    def table(self):
        """[D+1,6] fp32 on the device (layout: mdvit_eval_table); no sync"""
        return ops.eval_table(self.acc, self._table)

    def result(self) -> dict:
        t = self.table()
        host = torch.cat([t.double().reshape(-1), self.counts.double().reshape(-1)]).cpu()          # the epoch's one copy (counts are exact in a double below 2^53)
        D = self.num_domains
        tab, cnt = host[:(D + 1) * 6].reshape(D + 1, 6), host[(D + 1) * 6:].reshape(D, 5)
        res = {name: [float(v) for v in tab[:D, k]] for k, name in enumerate(_COLUMNS)}
        res["images"] = [int(v) for v in tab[:D, 5]]
        res["sum_loss"] = float(tab[D, 0])
        for k, name in enumerate(_COLUMNS[1:], start=1):
            res["avg_" + name] = float(tab[D, k])
        res["total_images"] = int(tab[D, 5])
        res["counts"] = [[int(v) for v in row] for row in cnt]
        return res


# ------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------
def _set_id(batch):
    sid = batch[2]
    # set_id is a HOST tensor, as from the DataLoader: reading it must not wait for the GPU (train.py, multi_train_MDViT.py:256-257)
    return sid.cpu() if torch.is_tensor(sid) and sid.is_cuda else torch.as_tensor(sid)


def _prepare(batch, device):
    img, label = batch[0], batch[1]
    img = img.to(device, non_blocking=True)
    if img.dtype == torch.uint8:          # the loader's uint8 NHWC image: norm01 + permute + Normalize on the device
        img = ops.image_normalize_u8(img)
    else:
        img = img.float()
    label = label.to(device, non_blocking=True).float()
    return img, label


def evaluate(model, loaders: Dict, *, num_domains: int = 4, use_domain_label: bool = True, fuse_domains: bool = True, forward: Optional[Callable] = None,
             accumulator: Optional[EvalAccumulator] = None, report: Optional["ImageReport"] = None) -> dict:          # noqa: F821 (report.py imports this module)
    """One validation / test epoch.  loaders: {domain name or id: iterable of (image, label, set_id)} (the contract of synthetic.make_domain_batch; a uint8
    [B,H,W,3] image goes through ops.image_normalize_u8).  The model runs in eval() under no_grad and gets its mode back.  With fuse_domains, equal-sized
    batches of different domains run as ONE domain-batched forward, model(x, label, [d0, d1, ...]) -- no operator couples samples in eval; ragged tails,
    models whose forward takes no `d`, and a user-supplied forward(image, domain_label_or_None, d) run per domain.  Returns EvalAccumulator.result().
    report: a report.ImageReport -- it is reset, takes every forward's logits right after the accumulator, image by image in evaluation order, and its
    result() comes back as res["report"]; every other key is the same with and without it."""
    device = next(model.parameters()).device
    acc = (accumulator or EvalAccumulator(num_domains, device)).reset()
    if report is not None:
        report.reset()
    takes_d = forward is None and "d" in inspect.signature(model.forward).parameters
    fuse = bool(fuse_domains) and takes_d

    def run(x, set_id, d):
        dl = F.one_hot(set_id, num_domains).float().to(device, non_blocking=True) if use_domain_label else None
        if forward is not None:
            return forward(x, dl, d)
        if takes_d:
            return model(x, dl, d) if use_domain_label else model(x, d=d)
        return model(x, dl) if use_domain_label else model(x)

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for step in _schedule(loaders, lambda b: int(b[0].shape[0]), lambda b: int(_set_id(b)[0]), fuse):
                batches = [b for _, b in step]
                set_ids = [_set_id(b) for b in batches]
                ds = [int(s[0]) for s in set_ids]
                prepared = [_prepare(b, device) for b in batches]
                if len(step) == 1:
                    (x, label), d_arg = prepared[0], str(ds[0])
                else:
                    x, label = torch.cat([p[0] for p in prepared]), torch.cat([p[1] for p in prepared])
                    d_arg = [str(d) for d in ds]
                out, aux = split_outputs(run(x, torch.cat(set_ids) if len(step) > 1 else set_ids[0], d_arg))
                images = [int(p[0].shape[0]) for p in prepared]
                acc.update(out, aux, label, ds, images)
                if report is not None:
                    report.update(out, aux, label, ds, images)
    finally:
        model.train(was_training)
    res = acc.result()
    if report is not None:
        res["report"] = report.result()
    return res
