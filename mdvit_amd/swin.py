"""SwinUnet (Models/Transformer/SwinUnet.py) behind the reference's constructor, module tree and state_dict, on HIP kernels throughout.

What `multi_train_BASE.py:82-88` builds is `SwinUnet(img_size=config.data.img_size, window_size=8)`: patch 4, embed 96, depths [2,2,6,2], heads [3,6,12,24],
mlp_ratio 4, qkv bias, drop_path_rate 0.1 (linspace over the 12 encoder blocks, mirrored in the decoder), LayerNorm eps 1e-5, no dropout, no BatchNorm.
The one operator without a counterpart elsewhere in this package is the shifted-window attention: ops.window_attention (csrc/winattn.hip) takes the qkv
product in natural token order and folds torch.roll / window_partition / window_reverse, the relative-position bias and the shift mask into its addressing.
PatchMerging's 2x2 gather and the PatchExpand rearrangements ride on their LayerNorm (ops.patch_merge_ln / ops.patch_expand_ln, csrc/swin_norm.hip).

Built: window_size = 8 with every stage's window equal to 8, i.e. img_size a multiple of 256, and num_classes = 1.  Anything else raises
NotImplementedError at construction (the attention kernel is built for 64-token windows at head dimension 32)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops
from ._lib import call
from .blocks import ConvParams, LayerNormParams, LinearParams
from .ops import _c, _p, _stream

WINDOW = 8
LN_EPS = 1e-5


def _relative_position_index(ws):
    """SwinUnet.py:88-97"""
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def _attn_mask(H, W, ws, shift):
    """SwinUnet.py:202-221: [nW, ws*ws, ws*ws] of 0 / -100.  Registered for the state_dict; the kernel derives the same mask from coordinates and never reads it."""
    img_mask = torch.zeros((1, H, W, 1))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mw = img_mask.view(1, H // ws, ws, W // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))


class WindowAttention(nn.Module):
    """parameters and buffer of SwinUnet.py:63-106; the compute is SwinTransformerBlock.forward's"""

    def __init__(self, dim, window_size, num_heads):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, (window_size, window_size), num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) * (2 * window_size - 1), num_heads))
        self.register_buffer("relative_position_index", _relative_position_index(window_size))
        self.qkv = LinearParams(dim, dim * 3)
        self.proj = LinearParams(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = LinearParams(dim, hidden)
        self.fc2 = LinearParams(hidden, dim)


class SwinTransformerBlock(nn.Module):
    """SwinUnet.py:227-264: x + DropPath(WMSA(LN1(x))), then x + DropPath(Mlp(LN2(x))) -- six launches-worth of operators: LayerNorm (fork), qkv product,
    window attention, proj product with the residual and the DropPath row scale in its epilogue, LayerNorm (fork), the MLP with its residual."""

    def __init__(self, dim, input_resolution, num_heads, window_size, shift_size, mlp_ratio, drop_path):
        super().__init__()
        self.dim, self.input_resolution, self.num_heads = dim, tuple(input_resolution), num_heads
        if min(self.input_resolution) <= window_size:          # :186-189
            shift_size, window_size = 0, min(self.input_resolution)
        if window_size != WINDOW or dim != num_heads * 32:
            raise NotImplementedError(f"window attention is built for 8 x 8 windows at head dimension 32 (window {window_size}, dim {dim}, heads {num_heads})")
        self.window_size, self.shift_size = window_size, shift_size
        self.norm1 = LayerNormParams(dim, LN_EPS)
        self.attn = WindowAttention(dim, window_size, num_heads)
        self.drop_path_p = float(drop_path)
        self.norm2 = LayerNormParams(dim, LN_EPS)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        H, W = self.input_resolution
        self.register_buffer("attn_mask", _attn_mask(H, W, window_size, shift_size) if shift_size > 0 else None)
        self.last_scales = None          # the DropPath scales of the last training forward ([2, B]: attention branch, MLP branch), for inspection

    def forward(self, x):
        H, W = self.input_resolution
        B, N, Cn = x.shape
        if N != H * W:
            raise ValueError(f"input feature has wrong size ({N} tokens for a {H} x {W} grid)")
        s1 = s2 = None
        if self.training and self.drop_path_p > 0.0:
            self.last_scales = ops.droppath_scales((2, B), 1.0 - self.drop_path_p, x.device)
            s1, s2 = self.last_scales[0], self.last_scales[1]
        a, m = self.attn, self.mlp
        cur, x = self.norm1.fork(x)
        qkv = ops.linear(cur, a.qkv.weight, a.qkv.bias)
        y = ops.window_attention(qkv, a.relative_position_bias_table, H, W, self.num_heads, self.shift_size)
        x = ops.linear(y, a.proj.weight, a.proj.bias, residual=x, rowscale=s1, rows_per_scale=N)
        cur, x = self.norm2.fork(x)
        return ops.mlp_residual(cur, x, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, s2, 0.0, N)


class PatchMerging(nn.Module):
    """SwinUnet.py:293-321"""

    def __init__(self, input_resolution, dim):
        super().__init__()
        self.input_resolution, self.dim = tuple(input_resolution), dim
        self.reduction = LinearParams(4 * dim, 2 * dim, bias=False)
        self.norm = LayerNormParams(4 * dim, LN_EPS)

    def forward(self, x):
        H, W = self.input_resolution
        B, N, Cn = x.shape
        y = ops.patch_merge_ln(_c(x).view(B, H, W, Cn), self.norm.weight, self.norm.bias, LN_EPS)
        return ops.linear(y.view(B, N // 4, 4 * Cn), self.reduction.weight)


class PatchExpand(nn.Module):
    """SwinUnet.py:332-354 (dim_scale 2) and FinalPatchExpand_X4 (:356-380, dim_scale 4)"""

    def __init__(self, input_resolution, dim, dim_scale=2):
        super().__init__()
        self.input_resolution, self.dim, self.dim_scale = tuple(input_resolution), dim, dim_scale
        self.expand = LinearParams(dim, (2 if dim_scale == 2 else 16) * dim, bias=False)
        self.norm = LayerNormParams(dim // 2 if dim_scale == 2 else dim, LN_EPS)

    def forward(self, x):
        H, W = self.input_resolution
        B, N, Cn = x.shape
        p = self.dim_scale
        u = ops.linear(x, self.expand.weight)
        y = ops.patch_expand_ln(u.view(B, H, W, u.shape[-1]), self.norm.weight, self.norm.bias, p, LN_EPS)
        return y.view(B, N * p * p, y.shape[-1])


class BasicLayer(nn.Module):
    """SwinUnet.py:401-440 (downsample) / BasicLayer_up :466-505 (upsample)"""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, drop_path, downsample=False, upsample=False):
        super().__init__()
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio,
                                                          drop_path[i]) for i in range(depth)])
        self.downsample = PatchMerging(input_resolution, dim) if downsample else None
        self.upsample = PatchExpand(input_resolution, dim, 2) if upsample else None

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        if self.downsample is not None:
            x = self.downsample(x)
        if self.upsample is not None:
            x = self.upsample(x)
        return x


class PatchEmbed(nn.Module):
    """SwinUnet.py:517-544: the 4 x 4 stride-4 convolution as a gather (mdvit_patchify) and one product, then LayerNorm"""

    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size, self.patch_size = (img_size, img_size), (patch_size, patch_size)
        self.patches_resolution = [img_size // patch_size, img_size // patch_size]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = ConvParams(embed_dim, in_chans, patch_size, patch_size)
        self.norm = LayerNormParams(embed_dim, LN_EPS)

    def forward(self, img):
        B, Cin, H, W = img.shape
        if (H, W) != self.img_size:
            raise ValueError(f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]}).")
        p = self.patch_size[0]
        ops._chk(img)
        patches = torch.empty((B * (H // p) * (W // p), Cin * p * p), device=img.device, dtype=torch.float32)
        call("mdvit_patchify", _p(_c(img)), _p(patches), B, Cin, H, W, p, _stream())
        w = self.proj
        x = ops.linear(patches, w.weight.view(w.weight.shape[0], -1), w.bias).view(B, -1, w.weight.shape[0])
        return self.norm(x)


class SwinTransformerSys(nn.Module):
    """SwinUnet.py:579-737 with final_upsample = "expand_first", ape off, patch_norm on"""

    def __init__(self, img_size, num_classes, window_size, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), mlp_ratio=4.,
                 drop_path_rate=0.1):
        super().__init__()
        self.num_classes, self.num_layers, self.embed_dim = num_classes, len(depths), embed_dim
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        res = self.patches_resolution = self.patch_embed.patches_resolution
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        nl = self.num_layers
        self.layers = nn.ModuleList()
        for i in range(nl):
            self.layers.append(BasicLayer(int(embed_dim * 2 ** i), (res[0] // 2 ** i, res[1] // 2 ** i), depths[i], num_heads[i], window_size, mlp_ratio,
                                             dpr[sum(depths[:i]):sum(depths[:i + 1])], downsample=i < nl - 1))
        self.layers_up = nn.ModuleList()
        self.concat_back_dim = nn.ModuleList()
        for i in range(nl):
            k = nl - 1 - i
            dim, r = int(embed_dim * 2 ** k), (res[0] // 2 ** k, res[1] // 2 ** k)
            self.concat_back_dim.append(LinearParams(2 * dim, dim) if i > 0 else nn.Identity())
            if i == 0:
                self.layers_up.append(PatchExpand(r, dim, 2))
            else:
                self.layers_up.append(BasicLayer(dim, r, depths[k], num_heads[k], window_size, mlp_ratio, dpr[sum(depths[:k]):sum(depths[:k + 1])],
                                                    upsample=i < nl - 1))
        self.norm = LayerNormParams(self.num_features, LN_EPS)
        self.norm_up = LayerNormParams(embed_dim, LN_EPS)
        self.up = PatchExpand((img_size // patch_size, img_size // patch_size), embed_dim, 4)
        self.output = ConvParams(num_classes, embed_dim, 1, 1, bias=False)
        self._init_weights()

    def _init_weights(self):
        """SwinUnet.py:672-679: Linear trunc_normal(.02) / 0, LayerNorm 1 / 0; the two convolutions keep nn.Conv2d's own initialisation"""
        for m in self.modules():
            if isinstance(m, LinearParams):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, LayerNormParams):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
            elif isinstance(m, ConvParams):
                nn.init.kaiming_uniform_(m.weight, a=math.sqrt(5))
                if m.bias is not None:
                    bound = 1.0 / math.sqrt(m.weight[0].numel())
                    nn.init.uniform_(m.bias, -bound, bound)

    def forward(self, img):
        x = self.patch_embed(img)
        skips = []
        for i, layer in enumerate(self.layers):
            if i < self.num_layers - 1:          # the layer's input also feeds the decoder's concatenation (x_downsample[3] is never read: :711)
                x, s = ops.fork(x, 2)
                skips.append(s)
            x = layer(x)
        x = self.norm(x)
        for i, layer_up in enumerate(self.layers_up):
            if i > 0:
                cb = self.concat_back_dim[i]
                x = ops.linear(ops.cat_channels(x, skips[self.num_layers - 1 - i]), cb.weight, cb.bias)
            x = layer_up(x)
        x = self.norm_up(x)
        H, W = self.patches_resolution
        B = x.shape[0]
        x = self.up(x)                                                          # [B, 16 H W, embed_dim]
        return ops.rowdot(x, self.output.weight).view(B, 1, 4 * H, 4 * W)        # the bias-free 1-channel 1x1 convolution


class SwinUnet(nn.Module):
    """SwinUnet.py:751-796.  model(img [B, 3 or 1, S, S]) -> logits [B, 1, S, S]"""

    def __init__(self, img_size=224, num_classes=1, window_size=7, zero_head=False, vis=False):
        super().__init__()
        if window_size != WINDOW or num_classes != 1 or img_size <= 0 or img_size % 256 != 0:
            raise NotImplementedError(
                f"SwinUnet(img_size={img_size}, num_classes={num_classes}, window_size={window_size}) is not built: the window-attention kernel covers "
                "window_size = 8 with 64-token windows in every stage (img_size a multiple of 256, as multi_train_BASE.py builds it) and num_classes = 1")
        self.num_classes, self.zero_head = num_classes, zero_head
        self.swin_unet = SwinTransformerSys(img_size, num_classes, window_size)

    def forward(self, x):
        if x.size()[1] == 1:
            x = x.repeat(1, 3, 1, 1)
        return self.swin_unet(x)
