"""A per-image test report on the device (the reference's helper: Utils/pieces.py:103-121 dice_per_img; TransFuse's validation loss:
multi_train_TransFuse.py:29-38,245-268): for every image of an epoch the five thresholded counts of the validation pass, optionally the per-image term of
structure_loss and the thresholded masks packed one bit per pixel -- appended to device tables by ops.eval_images / ops.eval_structure, forward after forward,
without a copy or a sync; result() is the epoch's single copy to the host, where Dice / IoU, their mean and std per domain and the structure-loss column are
formed from the integer counts.  boundary=True adds the boundary distances medpy.metric.binary scores with (hd95, hd, assd, asd; ops.eval_boundary): two more
tables in the same copy, the scores formed on the host by boundary_from_rows.  postprocess="fill" | "largest" | "fill_largest" adds the connected-component
clean-up of the thresholded masks (scipy.ndimage's binary_fill_holes / label, connectivity 1; ops.eval_components) and the scores of the cleaned masks.

    report = ImageReport(num_domains=4, masks=True, structure=True)
    res = evaluate(model, loaders, report=report)["report"]
    res["dice"], res["per_domain"][d]["dice_std"], res["per_domain"][d]["structure_loss"], unpack_masks(res["masks"], res["size"])
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops
from .evaluate import MAX_GROUPS

_COUNT_COLUMNS = 5          # |A&Y| |A| |Y| |Aaux&Y| |Aaux| (mdvit_eval_images)
_BOUNDARY_COLUMNS = 6       # nA nY max d2(A->Y) max d2(Y->A) d2 at rank floor(h), ceil(h) (mdvit_eval_boundary), per output
_BOUNDARY_MAX_SIDE = 1024   # mdvit_eval_boundary's limit on H and W
_PP_MODES = {"fill": 1, "largest": 2, "fill_largest": 3}          # mdvit_eval_components' mode argument
_PP_ROW = (3, 4)            # per set (main, auxiliary, label): components, largest area, filled, removed (mdvit_eval_components)
_PP_MAX_SIDE = 1024         # mdvit_eval_components' limit on H and W


# ------------------------------------------------------------------------------------------------
# packed masks (host): word j of an image holds pixels 64 j .. 64 j + 63, pixel 64 j + l in bit l
# ------------------------------------------------------------------------------------------------
def _words(n_pixels: int) -> int:
    return (int(n_pixels) + 63) // 64


def pack_masks(masks) -> np.ndarray:
    """{0, nonzero} masks [N,H,W] (numpy or torch, host) -> uint64 [N, ceil(H W / 64)], the layout ImageReport returns; the bits past H W are 0.  For tests:
    the device packs its own."""
    m = masks.cpu().numpy() if torch.is_tensor(masks) else np.asarray(masks)
    n = m.shape[0]
    flat = (m.reshape(n, -1) != 0).astype(np.uint8)
    pad = _words(flat.shape[1]) * 64 - flat.shape[1]
    if pad:
        flat = np.concatenate([flat, np.zeros((n, pad), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(np.packbits(flat, axis=1, bitorder="little")).view("<u8").astype(np.uint64, copy=False).reshape(n, -1)


def unpack_masks(packed, size) -> np.ndarray:
    """packed uint64 (or int64) [N, words] -> uint8 [N,H,W] in {0, 1} on the host, size = (H, W); little-endian bit order within a word"""
    H, W = int(size[0]), int(size[1])
    p = packed.cpu().numpy() if torch.is_tensor(packed) else np.asarray(packed)
    if p.ndim != 2 or p.dtype.itemsize != 8 or p.shape[1] != _words(H * W):
        raise ValueError(f"unpack_masks: expected 64-bit words [N,{_words(H * W)}] for size {(H, W)}, got {p.dtype} {p.shape}")
    by = np.ascontiguousarray(p).view(np.uint64).astype("<u8", copy=False).view(np.uint8).reshape(p.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :H * W].reshape(p.shape[0], H, W)


# ------------------------------------------------------------------------------------------------
# scores from counts (host, float64)
# ------------------------------------------------------------------------------------------------
def _ratio(num, den):
    """num / den with 0/0 -> 0 (mdvit_seg_metrics' rule; dice_per_img's numpy division gives NaN there)"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den > 0)


def scores_from_counts(counts, domains, structure=None) -> dict:
    """counts int64 [N,5] and the images' domain ids [N] (+ the structure column [N]) -> the score columns of ImageReport.result(): per image
    dice = 2|A&Y| / (|A|+|Y|), iou = |A&Y| / (|A|+|Y|-|A&Y|) for the main and auxiliary output (mdvit_seg_metrics' expressions, 0/0 -> 0) and `empty`
    (|A|+|Y| == 0: the images where the two conventions differ); per domain that saw images the count, mean and population std of dice and iou over
    ITS images and the mean structure term (loss_val_epoch, multi_train_TransFuse.py:259); sum_structure_loss over the domains (:268)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, _COUNT_COLUMNS)
    dom = np.asarray(domains, dtype=np.int32).reshape(-1)
    i0, a0, y, i1, a1 = (c[:, k] for k in range(_COUNT_COLUMNS))
    res = {"domain": dom, "counts": c,
           "dice": _ratio(2 * i0, a0 + y), "iou": _ratio(i0, a0 + y - i0), "aux_dice": _ratio(2 * i1, a1 + y), "aux_iou": _ratio(i1, a1 + y - i1),
           "empty": (a0 + y) == 0}
    if structure is not None:
        res["structure"] = np.asarray(structure, dtype=np.float64).reshape(-1)
    per: Dict[int, dict] = {}
    for d in sorted(set(int(v) for v in dom)):
        sel = dom == d
        row = {"images": int(sel.sum()), "dice_mean": float(res["dice"][sel].mean()), "dice_std": float(res["dice"][sel].std()),
               "iou_mean": float(res["iou"][sel].mean()), "iou_std": float(res["iou"][sel].std())}
        if structure is not None:
            row["structure_loss"] = float(res["structure"][sel].mean())
        per[d] = row
    res["per_domain"] = per
    if structure is not None:
        res["sum_structure_loss"] = float(sum(row["structure_loss"] for row in per.values()))
    return res


# ------------------------------------------------------------------------------------------------
# boundary scores from rows (host, float64)
# ------------------------------------------------------------------------------------------------
def boundary_from_rows(rows, sums, domains) -> dict:
    """rows int64 [N,2,6], sums float64 [N,2,2] (mdvit_eval_boundary's tables) and the images' domain ids [N] -> the boundary columns of
    ImageReport.result(), medpy.metric.binary's hd95 / hd / assd / asd (voxelspacing None, connectivity 1) per image:
        hd95 = sqrt(lo) + (h - floor(h)) (sqrt(hi) - sqrt(lo)),  h = 0.95 (nA + nY - 1)      numpy.percentile(., 95) of the stacked distances
        hd = sqrt(max d2),  asd_pred_to_label = S(A->Y) / nA,  asd_label_to_pred = S(Y->A) / nY,  assd = their mean
    and boundary_valid = nA > 0 and nY > 0; the same six with the prefix aux_ for the auxiliary output.  medpy raises for an empty mask: here the image is
    invalid, its scores are NaN, and the statistics leave it out.  "per_domain" {domain: hd95_mean, hd95_std (population), assd_mean, assd_std,
    boundary_images} over the domain's valid images of the main output (NaN and 0 when it has none)."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 2, _BOUNDARY_COLUMNS)
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 2, 2)
    dom = np.asarray(domains, dtype=np.int32).reshape(-1)
    res = {}
    for o, pre in ((0, ""), (1, "aux_")):
        na, ny = r[:, o, 0], r[:, o, 1]
        valid = (na > 0) & (ny > 0)
        h = 0.95 * (na + ny - 1).astype(np.float64)
        lo, hi = np.sqrt(r[:, o, 4].astype(np.float64)), np.sqrt(r[:, o, 5].astype(np.float64))
        nan = np.full(len(r), np.nan)
        den_a, den_y = np.maximum(na, 1).astype(np.float64), np.maximum(ny, 1).astype(np.float64)
        a2y, y2a = s[:, o, 0] / den_a, s[:, o, 1] / den_y
        res[pre + "hd95"] = np.where(valid, lo + (h - np.floor(h)) * (hi - lo), nan)
        res[pre + "hd"] = np.where(valid, np.sqrt(np.maximum(r[:, o, 2], r[:, o, 3]).astype(np.float64)), nan)
        res[pre + "assd"] = np.where(valid, (a2y + y2a) / 2.0, nan)
        res[pre + "asd_pred_to_label"] = np.where(valid, a2y, nan)
        res[pre + "asd_label_to_pred"] = np.where(valid, y2a, nan)
        res[pre + "boundary_valid"] = valid
    per: Dict[int, dict] = {}
    for d in sorted(set(int(v) for v in dom)):
        sel = (dom == d) & res["boundary_valid"]
        k = int(sel.sum())
        stat = lambda col, fn: float(fn(res[col][sel])) if k else float("nan")
        per[d] = {"hd95_mean": stat("hd95", np.mean), "hd95_std": stat("hd95", np.std), "assd_mean": stat("assd", np.mean), "assd_std": stat("assd", np.std),
                  "boundary_images": k}
    res["per_domain"] = per
    return res


# ------------------------------------------------------------------------------------------------
# connected-component post-processing (host side)
# ------------------------------------------------------------------------------------------------
def postprocess_mode(name) -> int:
    """"fill" | "largest" | "fill_largest" -> mdvit_eval_components' mode (1, 2, 3); anything else is a ValueError (connectivity is always 1)"""
    if not isinstance(name, str) or name not in _PP_MODES:
        raise ValueError(f"postprocess must be None or one of {sorted(_PP_MODES)}, got {name!r}")
    return _PP_MODES[name]


def postprocess_from_rows(pp_counts, pp_rows, domains) -> dict:
    """pp_counts int64 [N,5] (eval_images' columns on the cleaned masks), pp_rows int64 [N,3,4] (mdvit_eval_components' rows) and the images' domain ids [N]
    -> the post-processing columns of ImageReport.result(): "pp_counts", "pp_dice" / "pp_iou" / "pp_aux_dice" / "pp_aux_iou" (scores_from_counts'
    expressions, 0/0 -> 0), "components" / "largest_area" (of the RAW masks) / "filled" / "removed" int64 [N,3] (main, auxiliary, label), and "per_domain"
    {domain: pp_dice_mean, pp_dice_std (population), pp_iou_mean, pp_iou_std}."""
    sc = scores_from_counts(pp_counts, domains)
    r = np.asarray(pp_rows, dtype=np.int64).reshape((-1,) + _PP_ROW)
    res = {"pp_counts": sc["counts"], "pp_dice": sc["dice"], "pp_iou": sc["iou"], "pp_aux_dice": sc["aux_dice"], "pp_aux_iou": sc["aux_iou"],
           "components": r[:, :, 0].copy(), "largest_area": r[:, :, 1].copy(), "filled": r[:, :, 2].copy(), "removed": r[:, :, 3].copy()}
    res["per_domain"] = {d: {"pp_" + k: row[k] for k in ("dice_mean", "dice_std", "iou_mean", "iou_std")} for d, row in sc["per_domain"].items()}
    return res


# ------------------------------------------------------------------------------------------------
# the epoch's tables
# ------------------------------------------------------------------------------------------------
class ImageReport:
    """counts [cap,5] int64, structure [cap] float64, bits / aux_bits [cap,words] int64 (uint64 words), boundary_rows [cap,2,6] int64 and boundary_sums
    [cap,2,2] float64, with postprocess also pp_counts [cap,5], pp_rows [cap,3,4] int64 and pp_bits / pp_aux_bits [cap,words] on `device`, one row per image
    in update() order.
    update() enqueues kernels and returns -- the row offset and the images' domains are host integers; result() is the one call that copies to the host.
    The tables double when they are full (a stream-ordered device copy); `capacity` = the epoch's image count avoids that."""

    def __init__(self, num_domains: int = 4, device=None, masks: bool = False, aux_masks: bool = False, structure: bool = False, capacity: int = 0,
                 boundary: bool = False, postprocess=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("ImageReport lives on a CUDA(HIP) device; there is no CPU path")
        self.num_domains = int(num_domains)
        self.device = device
        self.masks, self.aux_masks, self.structure = bool(masks), bool(aux_masks), bool(structure)
        self.boundary = bool(boundary)
        self.postprocess = postprocess
        self._pp_mode = None if postprocess is None else postprocess_mode(postprocess)
        self.capacity = max(int(capacity), 0)
        self.size = None          # (H, W), fixed by the first update
        self.rows = 0
        self.domains: list = []
        self.counts = self.structure_col = self.bits = self.aux_bits = self.boundary_rows = self.boundary_sums = None
        self.pp_counts = self.pp_rows = self.pp_bits = self.pp_aux_bits = None
        self._cap = 0
        self._ws = self._ws_s = self._ws_b = self._ws_c = None

    def reset(self):
        """forget the images (the tables, their capacity and the image size stay)"""
        self.rows = 0
        self.domains = []
        return self

    def _table(self, old, cap, cols, dtype):
        t = torch.empty((cap,) + cols, device=self.device, dtype=dtype)
        if old is not None and self.rows:
            t[:self.rows].copy_(old[:self.rows])
        return t

    def _reserve(self, need: int):
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, self.capacity, 1)
        words = _words(self.size[0] * self.size[1])
        self.counts = self._table(self.counts, cap, (_COUNT_COLUMNS,), torch.int64)
        if self.structure:
            self.structure_col = self._table(self.structure_col, cap, (), torch.float64)
        if self.masks:
            self.bits = self._table(self.bits, cap, (words,), torch.int64)
        if self.aux_masks:
            self.aux_bits = self._table(self.aux_bits, cap, (words,), torch.int64)
        if self.boundary:
            self.boundary_rows = self._table(self.boundary_rows, cap, (2, _BOUNDARY_COLUMNS), torch.int64)
            self.boundary_sums = self._table(self.boundary_sums, cap, (2, 2), torch.float64)
        if self._pp_mode is not None:
            self.pp_counts = self._table(self.pp_counts, cap, (_COUNT_COLUMNS,), torch.int64)
            self.pp_rows = self._table(self.pp_rows, cap, _PP_ROW, torch.int64)
            if self.masks:
                self.pp_bits = self._table(self.pp_bits, cap, (words,), torch.int64)
            if self.aux_masks:
                self.pp_aux_bits = self._table(self.pp_aux_bits, cap, (words,), torch.int64)
        self._cap = cap

    @staticmethod
    def _workspace(ws, nbytes):
        return ws if ws is not None and ws.numel() * 8 >= nbytes else None

    def update(self, out, aux, label, domains, images=None):
        """logits of one forward -> one row per image.  Arguments as EvalAccumulator.update: domains an int (one domain batch) or the ids of the forward's
        consecutive domain batches, images their sizes (default: equal parts).  Returns the number of rows the report holds."""
        if isinstance(domains, (int, str)):
            domains, images = [int(domains)], [out.shape[0]]
        else:
            domains = [int(d) for d in domains]
            if images is None:
                if not domains or out.shape[0] % len(domains):
                    raise ValueError(f"batch {out.shape[0]} is not {len(domains)} equal domain batches")
                images = [out.shape[0] // len(domains)] * len(domains)
        images = [int(v) for v in images]
        if len(domains) > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} domain batches per update")
        n = sum(images)
        if len(images) != len(domains) or min(images) <= 0 or n != out.shape[0] or out.dim() < 3:
            raise ValueError(f"logits {tuple(out.shape)} are not the domain batches {images} of images [..,H,W]")
        if min(domains) < 0 or max(domains) >= self.num_domains:
            raise ValueError(f"domains {domains}, expected 0..{self.num_domains - 1}")
        W = int(out.shape[-1])
        size = (out.numel() // n // W, W)          # [B,1,H,W] and [B,H,W]: (H, W); more channels stack as rows
        if self.structure and not (out.dim() == 4 and out.shape[1] == 1):
            raise ValueError(f"structure=True needs [B,1,H,W] logits, got {tuple(out.shape)}")
        if self.boundary:
            if not ((out.dim() == 4 and out.shape[1] == 1) or out.dim() == 3):
                raise ValueError(f"boundary=True needs [B,1,H,W] or [B,H,W] logits, got {tuple(out.shape)}")
            if max(size) > _BOUNDARY_MAX_SIDE:
                raise ValueError(f"boundary=True takes images up to {_BOUNDARY_MAX_SIDE} x {_BOUNDARY_MAX_SIDE}, got {size[0]} x {size[1]}")
        if self._pp_mode is not None:
            if not ((out.dim() == 4 and out.shape[1] == 1) or out.dim() == 3):
                raise ValueError(f"postprocess needs [B,1,H,W] or [B,H,W] logits, got {tuple(out.shape)}")
            if max(size) > _PP_MAX_SIDE:
                raise ValueError(f"postprocess takes images up to {_PP_MAX_SIDE} x {_PP_MAX_SIDE}, got {size[0]} x {size[1]}")
        if self.size is None:
            self.size = size
        elif size != self.size:
            raise ValueError(f"this report holds {self.size[0]} x {self.size[1]} images, got {size[0]} x {size[1]}")
        r0, r1 = self.rows, self.rows + n
        self._reserve(r1)
        nbytes = ops.eval_images_ws_bytes(n, size[0] * size[1])
        self._ws = self._workspace(self._ws, nbytes)
        if self._ws is None:
            self._ws = torch.empty(((nbytes + 7) // 8,), device=self.device, dtype=torch.int64)
        aux_bits = self.aux_bits[r0:r1] if self.aux_masks else None
        if aux is None and aux_bits is not None:
            aux_bits.zero_()          # no auxiliary output in this forward: its masks are empty
            aux_bits = None
        ops.eval_images(out, aux, label, self.counts[r0:r1], self._ws, self.bits[r0:r1] if self.masks else None, aux_bits)
        if self.structure:
            nbytes = ops.eval_structure_ws_bytes(n, size[0], size[1])
            self._ws_s = self._workspace(self._ws_s, nbytes)
            if self._ws_s is None:
                self._ws_s = torch.empty(((nbytes + 7) // 8,), device=self.device, dtype=torch.float64)
            ops.eval_structure(out, label, self.structure_col[r0:r1], self._ws_s)
        if self.boundary:
            nbytes = ops.eval_boundary_ws_bytes(n, size[0], size[1])
            self._ws_b = self._workspace(self._ws_b, nbytes)
            if self._ws_b is None:
                self._ws_b = torch.empty(((nbytes + 7) // 8,), device=self.device, dtype=torch.int64)
            ops.eval_boundary(out, aux, label, self.boundary_rows[r0:r1], self.boundary_sums[r0:r1], self._ws_b)
        if self._pp_mode is not None:
            nbytes = ops.eval_components_ws_bytes(n, size[0], size[1])
            self._ws_c = self._workspace(self._ws_c, nbytes)
            if self._ws_c is None:
                self._ws_c = torch.empty(((nbytes + 7) // 8,), device=self.device, dtype=torch.int64)
            pp_aux_bits = self.pp_aux_bits[r0:r1] if self.aux_masks else None
            if aux is None and pp_aux_bits is not None:
                pp_aux_bits.zero_()
                pp_aux_bits = None
            ops.eval_components(out, aux, label, self._pp_mode, self.pp_counts[r0:r1], self.pp_rows[r0:r1], self._ws_c,
                                self.pp_bits[r0:r1] if self.masks else None, pp_aux_bits)
        for d, k in zip(domains, images):
            self.domains.extend([d] * k)
        self.rows = r1
        return self.rows

    def result(self) -> dict:
        """the epoch's one copy: every table into ONE pinned buffer with one copy_, then the stream is synchronised.  Host numpy arrays, one row per image
        in update() order: "domain" int32 [N], "counts" int64 [N,5], "dice" / "iou" / "aux_dice" / "aux_iou" float64 [N] (0/0 -> 0) and "empty" bool [N]
        (scores_from_counts), "structure" float64 [N], "masks" / "aux_masks" uint64 [N,words] (unpack_masks) when asked for, "size" (H, W), "per_domain"
        {domain: images, dice_mean, dice_std, iou_mean, iou_std, structure_loss} and "sum_structure_loss".  With boundary=True also boundary_from_rows'
        columns ("hd95", "hd", "assd", "asd_pred_to_label", "asd_label_to_pred", "boundary_valid" and their aux_ twins; NaN where a mask is empty), its
        per-domain keys inside "per_domain" and "boundary_rows", the raw int64 table [N,2,6].  With postprocess also postprocess_from_rows' columns
    ("pp_counts", "pp_dice", "pp_iou", "pp_aux_dice", "pp_aux_iou", "components", "largest_area", "filled", "removed"), its per-domain keys
    (pp_dice_mean, pp_dice_std, pp_iou_mean, pp_iou_std), "pp_masks" / "pp_aux_masks" (the cleaned masks, when masks / aux_masks are on) and
    "postprocess", the mode."""
        N = self.rows
        parts = []          # (name, dtype, shape)
        if N:
            tabs = [("counts", self.counts, np.int64)]
            if self.structure:
                tabs.append(("structure", self.structure_col, np.float64))
            if self.masks:
                tabs.append(("masks", self.bits, np.uint64))
            if self.aux_masks:
                tabs.append(("aux_masks", self.aux_bits, np.uint64))
            if self.boundary:
                tabs.append(("boundary_rows", self.boundary_rows, np.int64))
                tabs.append(("boundary_sums", self.boundary_sums, np.float64))
            if self._pp_mode is not None:
                tabs.append(("pp_counts", self.pp_counts, np.int64))
                tabs.append(("pp_rows", self.pp_rows, np.int64))
                if self.masks:
                    tabs.append(("pp_masks", self.pp_bits, np.uint64))
                if self.aux_masks:
                    tabs.append(("pp_aux_masks", self.pp_aux_bits, np.uint64))
            dev = torch.cat([t[:N].reshape(-1).view(torch.uint8) for _, t, _ in tabs])          # every table is 8-byte elements: the offsets stay aligned
            host = torch.empty((dev.numel(),), dtype=torch.uint8, pin_memory=True)
            host.copy_(dev, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            buf, off = host.numpy(), 0
            for name, t, dt in tabs:
                nb = N * int(np.prod(t.shape[1:], dtype=np.int64)) * 8
                parts.append((name, buf[off:off + nb].view(dt).reshape((N,) + tuple(t.shape[1:])).copy()))
                off += nb
        got = dict(parts)
        res = scores_from_counts(got.get("counts", np.zeros((0, _COUNT_COLUMNS), dtype=np.int64)), np.asarray(self.domains, dtype=np.int32),
                                 got.get("structure", np.zeros((0,), dtype=np.float64)) if self.structure else None)
        words = _words(self.size[0] * self.size[1]) if self.size else 0
        for name, on in (("masks", self.masks), ("aux_masks", self.aux_masks)):
            if on:
                res[name] = got.get(name, np.zeros((0, words), dtype=np.uint64))
        res["size"] = self.size
        if self.boundary:
            rows = got.get("boundary_rows", np.zeros((0, 2, _BOUNDARY_COLUMNS), dtype=np.int64))
            b = boundary_from_rows(rows, got.get("boundary_sums", np.zeros((0, 2, 2), dtype=np.float64)), res["domain"])
            for d, row in b.pop("per_domain").items():
                res["per_domain"][d].update(row)
            res.update(b)
            res["boundary_rows"] = rows
        if self._pp_mode is not None:
            pp = postprocess_from_rows(got.get("pp_counts", np.zeros((0, _COUNT_COLUMNS), dtype=np.int64)),
                                       got.get("pp_rows", np.zeros((0,) + _PP_ROW, dtype=np.int64)), res["domain"])
            for d, row in pp.pop("per_domain").items():
                res["per_domain"][d].update(row)
            res.update(pp)
            for name, on in (("pp_masks", self.masks), ("pp_aux_masks", self.aux_masks)):
                if on:
                    res[name] = got.get(name, np.zeros((0, words), dtype=np.uint64))
            res["postprocess"] = self.postprocess
        return res
