"""The reference loader's train augmentations on the device (Datasets/create_dataset.py:131-139,159-172, `train_aug=True`).

The reference runs five albumentations transforms per image on the host -- GaussNoise, HorizontalFlip, VerticalFlip, ShiftScaleRotate,
RandomBrightnessContrast -- then norm01 and Normalize.  Here the random DRAW stays on the host (a few floats per sample, deterministic from a
torch.Generator) and the APPLICATION is one HIP gather kernel on the uint8 batch (csrc/augment.hip, ops.augment_normalize_u8), which also does the
normalisation and the label cast.  The A.Resize(img_size, img_size) in front of the pipeline is NOT done here (the kernel's input and output sizes are equal;
Datasets/process_resize.py stores 512 x 512 while Configs/multi_train_local.yml trains at 256): mdvit_amd.data.DeviceDataset.batch resizes on the device
(csrc/dataset.hip) and hands this module a batch at size; a host loader that feeds TrainAug directly keeps its own A.Resize.

The semantics are the published albumentations 1.x defaults, restated (nothing is imported from albumentations; the reference pins no version, so the
pipeline is parity-unpinned like oracle/pipeline.py):
  noise     sigma = sqrt(U(10, 50)) levels, per channel, added before the geometry
  shift     dx, dy ~ U(-0.0625, 0.0625) of W, H;  scale s ~ 1 + U(-0.1, 0.1);  rotation ~ U(-45, 45) degrees, about the centre ((W-1)/2, (H-1)/2),
            bilinear for the image and nearest for the mask, BORDER_REFLECT_101
  contrast  alpha ~ 1 + U(-0.2, 0.2);  brightness beta ~ 255 U(-0.2, 0.2) levels (brightness_by_max)
each applied independently with probability p.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

FLAG_NAMES = ("noise", "hflip", "vflip", "ssr", "bc")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)      # m00 m01 m02 m10 m11 m12 alpha beta sigma


def draw_train_aug_scalars(B: int, generator: torch.Generator, p: float = 0.5) -> Dict[str, torch.Tensor]:
    """The random part alone: which transforms apply (flags bool [B,5] in FLAG_NAMES order), every transform's value (fp64 [B], drawn whether
    the transform applies or not, so the stream of draws does not depend on the flags) and the noise keys (int32 [B,2])."""
    u = torch.rand((B, 12), generator=generator, dtype=torch.float64)
    k = torch.randint(0, 1 << 32, (B, 2), generator=generator, dtype=torch.int64)
    return {
        "flags": u[:, :5] < p,
        "noise_var": 10.0 + 40.0 * u[:, 5],
        "dx": -0.0625 + 0.125 * u[:, 6],
        "dy": -0.0625 + 0.125 * u[:, 7],
        "scale": 0.9 + 0.2 * u[:, 8],
        "angle": -45.0 + 90.0 * u[:, 9],                        # degrees
        "alpha": 0.8 + 0.4 * u[:, 10],
        "beta": 255.0 * (-0.2 + 0.4 * u[:, 11]),
        "keys": torch.where(k >= (1 << 31), k - (1 << 32), k).to(torch.int32),
    }


def compose_train_aug(sc: Dict[str, torch.Tensor], H: int, W: int) -> torch.Tensor:
    """scalars -> the kernel's table [B,9] f32 = (m00 m01 m02 m10 m11 m12 alpha beta sigma), composed in fp64.
    M = cv2.getRotationMatrix2D(centre, angle, scale) plus the shift maps source to destination after the flips F (x -> W-1-x, y -> H-1-y); the
    table holds (M F)^-1, the dst -> src map: reflect-101 commutes with a flip, so one matrix carries the whole geometry."""
    fl = sc["flags"]
    noise, hflip, vflip, ssr, bc = (fl[:, i] for i in range(5))
    one, zero = torch.ones_like(sc["scale"]), torch.zeros_like(sc["scale"])
    th = sc["angle"] * (math.pi / 180.0)
    a = torch.where(ssr, sc["scale"] * torch.cos(th), one)
    b = torch.where(ssr, sc["scale"] * torch.sin(th), zero)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    tx = torch.where(ssr, (1.0 - a) * cx - b * cy + sc["dx"] * W, zero)
    ty = torch.where(ssr, b * cx + (1.0 - a) * cy + sc["dy"] * H, zero)
    det = a * a + b * b
    # M^-1 = [A^-1 | -A^-1 t],  A = [[a, b], [-b, a]]
    r0 = [a / det, -b / det, -(a * tx - b * ty) / det]
    r1 = [b / det, a / det, -(b * tx + a * ty) / det]
    # F M^-1: a flip mirrors the SOURCE coordinate
    r0 = [torch.where(hflip, -r0[0], r0[0]), torch.where(hflip, -r0[1], r0[1]), torch.where(hflip, (W - 1.0) - r0[2], r0[2])]
    r1 = [torch.where(vflip, -r1[0], r1[0]), torch.where(vflip, -r1[1], r1[1]), torch.where(vflip, (H - 1.0) - r1[2], r1[2])]
    alpha = torch.where(bc, sc["alpha"], one)
    beta = torch.where(bc, sc["beta"], zero)
    sigma = torch.where(noise, torch.sqrt(sc["noise_var"]), zero)
    table = torch.stack(r0 + r1 + [alpha, beta, sigma], dim=1) + 0.0          # + 0.0: no negative zeros in the table
    return table.to(torch.float32)


def draw_train_aug(B: int, H: int, W: int, generator: torch.Generator, p: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Draw one batch's augmentation on the CPU: (params f32 [B,9], keys int32 [B,2], flags bool [B,5] = which of noise, hflip, vflip, ssr, bc apply)."""
    sc = draw_train_aug_scalars(B, generator, p)
    return compose_train_aug(sc, H, W), sc["keys"], sc["flags"]


class TrainAug:
    """aug(img_u8 [B,H,W,3] cuda, mask_u8 [B,H,W] cuda or None) -> (image fp32 [B,3,H,W], label fp32 [B,1,H,W] or None), what the reference's loader
    hands the model with train_aug=True.  Draws from its own generator, uploads the table without blocking, launches on the current stream."""

    def __init__(self, p: float = 0.5, seed: int = 0):
        self.p = float(p)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.flags: Optional[torch.Tensor] = None         # of the last batch

    def state_dict(self) -> dict:
        """the generator's state and p: the draws of the next batch are a function of these two alone"""
        return {"p": self.p, "generator": self.generator.get_state()}

    def load_state_dict(self, state_dict: dict):
        self.p = float(state_dict["p"])
        self.generator.set_state(state_dict["generator"])

    def __call__(self, img_u8: torch.Tensor, mask_u8: Optional[torch.Tensor] = None):
        from . import ops
        if img_u8.dim() != 4 or not img_u8.is_cuda:
            raise ValueError("TrainAug expects a CUDA uint8 batch [B,H,W,3]")
        B, H, W = img_u8.shape[:3]
        params, keys, self.flags = draw_train_aug(B, H, W, self.generator, self.p)
        params = params.pin_memory().to(img_u8.device, non_blocking=True)
        keys = keys.pin_memory().to(img_u8.device, non_blocking=True)
        return ops.augment_normalize_u8(img_u8, mask_u8, params, keys)
