"""UTNet (Models/Hybrid_models/UTNetFolder/UTNet.py, conv_trans_utils.py, unet_utils.py) behind the reference's constructor, module tree and state_dict, on HIP
kernels throughout.

What `multi_train_BASE.py:75-81` builds is `UTNet(in_chan=3, base_chan=32, num_classes=1, reduce_size=8, block_list='1234', num_blocks=[1,1,1,1],
num_heads=[4,4,4,4], projection='interp', attn_drop=0.1, proj_drop=0.1, rel_pos=True, aux_loss=False, maxpool=True)`: a U-Net of pre-activation residual blocks
whose four encoder stages and three of the four decoder stages carry one attention block each.  The one operator without a counterpart elsewhere in this package
is that attention: every query of an H x W map attends to the 64 keys of the map reduced to 8 x 8, with a relative-position bias indexed by the query's coarse
cell (ops.lowrank_attention, csrc/lowrank_attn.hip).  Everything else composes from the package's operators; activations are NHWC inside.

k / v reduction.  to_qkv / to_kv are a depthwise 3 x 3 and a bias-free pointwise product, and the align_corners=True resize to 8 x 8 is linear per channel, so the
pointwise product commutes with it: t = dwconv(x) once, q = t Wq^T over all tokens, kv = resize(t) Wkv^T over 64 tokens per image.  up_block's 1 x 1 convolution
(with bias; the bilinear weights sum to one) is commuted with its x2 resize the same way, so it runs at the low resolution.

Built: exactly that configuration, with attn_drop / proj_drop free in [0, 1) and base_chan such that every dim_head is one of 16 / 32 / 64 / 128.  Anything else raises
NotImplementedError at construction.  Input height and width are multiples of 128 (every query grid a multiple of 8, the deepest map at least 8 x 8)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops
from ._lib import ACT_NONE, ACT_RELU
from .blocks import BatchNormAct, ConvParams, _NoParams

REDUCE = 8
DIM_HEADS = (16, 32, 64, 128)


def _bn(bn: BatchNormAct, x):
    """bn on NHWC x; a map whose channels were zero-padded to a multiple of four (the image) is normalised with zero-padded parameters: the padding stays zero"""
    Cn, Cx = bn.weight.shape[0], x.shape[-1]
    if Cn == Cx:
        return bn(x)
    rm = torch.cat([bn.running_mean, bn.running_mean.new_zeros(Cx - Cn)])
    rv = torch.cat([bn.running_var, bn.running_var.new_ones(Cx - Cn)])
    z = ops.bn_act(x, ops.pad_zeros(bn.weight, 0, Cx), ops.pad_zeros(bn.bias, 0, Cx), rm, rv, bn.num_batches_tracked, bn.training, bn.act, bn.eps, bn.momentum)
    if bn.training:
        with torch.no_grad():
            bn.running_mean.copy_(rm[:Cn])
            bn.running_var.copy_(rv[:Cn])
    return z


class BasicBlock(nn.Module):
    """conv_trans_utils.py:46-78 (pre-activation): BN -> ReLU -> conv3x3, twice; the shortcut, where the widths differ, is a second BN of the same input -> ReLU -> 1x1,
    whose product takes the main path as its epilogue's residual"""

    def __init__(self, inplanes, planes, stride=1, exact=False):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("BasicBlock: stride 1 only (the built configuration pools with MaxPool2d)")
        self.conv1 = ConvParams(planes, inplanes, 3, 3, bias=False)
        self.bn1 = BatchNormAct(inplanes, ACT_RELU)
        self.relu = _NoParams()
        self.conv2 = ConvParams(planes, planes, 3, 3, bias=False)
        self.bn2 = BatchNormAct(planes, ACT_RELU)
        self.shortcut = nn.Sequential()
        if inplanes != planes:
            self.shortcut = nn.Sequential(BatchNormAct(inplanes, ACT_RELU), self.relu, ConvParams(planes, inplanes, 1, 1, bias=False))
        self.exact = bool(exact)

    def forward(self, x):
        a, s = ops.fork(x, 2)
        Cx = x.shape[-1]
        # exact: the products of the first stage (`inc`, at the image) with exact fp32 arithmetic in EVERY GEMM mode.  The BatchNorm affine gradients of the first
        # layers cancel to 1e-4 of their terms (the reference's own fp32 run is up to 1e-2 off its fp64 one there); the 1e-5 of the bf16x3 split in this
        # stage's forward alone moved them by 1.2 x the bound of tests/test_gpu_utnet_model.py, measured stage by stage.
        conv, lin = (ops.conv3x3_exact, ops.linear_exact) if self.exact else (ops.conv3x3_dense, ops.linear)
        out = conv(_bn(self.bn1, a), ops.pad_zeros(self.conv1.weight, 1, Cx))
        out = conv(self.bn2(out), self.conv2.weight)
        if len(self.shortcut) == 0:
            return ops.add(out, s)
        return lin(_bn(self.shortcut[0], s), ops.pad_zeros(self.shortcut[2].weight, 1, Cx), residual=out)


class depthwise_separable_conv(nn.Module):
    """conv_trans_utils.py:14-24; parameters only, the attention modules run the two halves where they need them"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.depthwise = ConvParams(in_ch, 1, 3, 3, bias=False, groups=in_ch)
        self.pointwise = ConvParams(out_ch, in_ch, 1, 1, bias=False)


def _relative_position_index(h, w):
    """conv_trans_utils.py:357-367"""
    coords = torch.stack(torch.meshgrid([torch.arange(h), torch.arange(w)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += h - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * h - 1
    return rel.sum(-1)


class RelativePositionBias(nn.Module):
    """conv_trans_utils.py:344-379: the table and the index buffer; the kernel derives the index from the coordinates and indexes the table by the query's cell"""

    def __init__(self, num_heads, h, w):
        super().__init__()
        self.num_heads, self.h, self.w = num_heads, h, w
        self.relative_position_bias_table = nn.Parameter(torch.randn((2 * h - 1) * (2 * w - 1), num_heads) * 0.02)
        self.register_buffer("relative_position_index", _relative_position_index(h, w))


class _AttentionBase(nn.Module):
    def _setup(self, heads, dim_head, attn_drop, proj_drop, reduce_size, projection, rel_pos):
        if dim_head not in DIM_HEADS or reduce_size != REDUCE or projection != "interp" or not rel_pos:
            raise NotImplementedError(f"low-rank attention is built for dim_head 16 / 32 / 64 / 128, reduce_size 8, projection 'interp' and rel_pos=True "
                                      f"(dim_head {dim_head}, reduce_size {reduce_size}, projection {projection!r}, rel_pos {rel_pos})")
        self.inner_dim, self.heads, self.dim_head, self.scale = dim_head * heads, heads, dim_head, dim_head ** (-0.5)
        self.reduce_size, self.projection, self.rel_pos = reduce_size, projection, rel_pos
        self.attn_drop_p, self.proj_drop_p = float(attn_drop), float(proj_drop)

    def _reduce(self, t):
        """[B, H, W, C] -> [B, 64, C]: the align_corners=True resize to 8 x 8, skipped where the map is 8 high already (as the reference tests H alone)"""
        B, H, W, Cn = t.shape
        if H != REDUCE:
            t = ops.resize_ac_to(t, REDUCE, REDUCE)
        elif W != REDUCE:
            raise ValueError(f"a map {H} x {W} is 8 high but not 8 wide: the reference skips the resize and then fails to rearrange it")
        return t.view(B, REDUCE * REDUCE, Cn)

    def _attend(self, q, kv, Hq, Wq, residual):
        """q [B, Hq*Wq, C], kv [B, 64, 2C] -> proj_drop(to_out(attention)) + residual, [B, Hq, Wq, dim]"""
        B, N, Cn = q.shape
        k, v = ops.split_cols(kv.view(B * REDUCE * REDUCE, 2 * Cn), (Cn, Cn))
        o = ops.lowrank_attention(q, k.view(B, REDUCE * REDUCE, Cn), v.view(B, REDUCE * REDUCE, Cn), self.relative_position_encoding.relative_position_bias_table,
                                  Hq, Wq, self.heads, self.attn_drop_p, training=self.training)
        o = ops.dwconv3x3(o.view(B, Hq, Wq, Cn), self.to_out.depthwise.weight)
        return ops.linear(o, self.to_out.pointwise.weight, residual=residual, drop_p=self.proj_drop_p if self.training else 0.0)


class LinearAttention(_AttentionBase):
    """conv_trans_utils.py:150-215"""

    def __init__(self, dim, heads=4, dim_head=64, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp', rel_pos=True):
        super().__init__()
        self._setup(heads, dim_head, attn_drop, proj_drop, reduce_size, projection, rel_pos)
        self.to_qkv = depthwise_separable_conv(dim, self.inner_dim * 3)
        self.to_out = depthwise_separable_conv(self.inner_dim, dim)
        self.relative_position_encoding = RelativePositionBias(heads, reduce_size, reduce_size)

    def forward(self, x, residual):
        B, H, W, _ = x.shape
        t = ops.dwconv3x3(x, self.to_qkv.depthwise.weight)
        tq, tr = ops.fork(t, 2)
        Wq, Wkv = ops.split_rows(self.to_qkv.pointwise.weight, (self.inner_dim, 2 * self.inner_dim))
        q = ops.linear(tq.view(B, H * W, -1), Wq)
        kv = ops.linear(self._reduce(tr), Wkv)
        return self._attend(q, kv, H, W, residual)


class LinearAttentionDecoder(_AttentionBase):
    """conv_trans_utils.py:217-282"""

    def __init__(self, in_dim, out_dim, heads=4, dim_head=64, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp', rel_pos=True):
        super().__init__()
        self._setup(heads, dim_head, attn_drop, proj_drop, reduce_size, projection, rel_pos)
        self.to_kv = depthwise_separable_conv(in_dim, self.inner_dim * 2)
        self.to_q = depthwise_separable_conv(out_dim, self.inner_dim)
        self.to_out = depthwise_separable_conv(self.inner_dim, out_dim)
        self.relative_position_encoding = RelativePositionBias(heads, reduce_size, reduce_size)

    def forward(self, q, x, residual):
        B, HH, WH, _ = q.shape
        kv = ops.linear(self._reduce(ops.dwconv3x3(x, self.to_kv.depthwise.weight)), self.to_kv.pointwise.weight)
        qq = ops.linear(ops.dwconv3x3(q, self.to_q.depthwise.weight).view(B, HH * WH, -1), self.to_q.pointwise.weight)
        return self._attend(qq, kv, HH, WH, residual)


class BasicTransBlock(nn.Module):
    """conv_trans_utils.py:80-107"""

    def __init__(self, in_ch, heads, dim_head, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp', rel_pos=True):
        super().__init__()
        self.bn1 = BatchNormAct(in_ch, ACT_NONE)
        self.attn = LinearAttention(in_ch, heads=heads, dim_head=in_ch // heads, attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size, projection=projection,
                                    rel_pos=rel_pos)
        self.bn2 = BatchNormAct(in_ch, ACT_RELU)
        self.relu = _NoParams()
        self.mlp = ConvParams(in_ch, in_ch, 1, 1, bias=False)

    def forward(self, x):
        a, r = ops.fork(x, 2)
        out = self.attn(self.bn1(a), r)
        o, r2 = ops.fork(out, 2)
        return ops.linear(self.bn2(o), self.mlp.weight, residual=r2)


class BasicTransDecoderBlock(nn.Module):
    """conv_trans_utils.py:109-142"""

    def __init__(self, in_ch, out_ch, heads, dim_head, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp', rel_pos=True):
        super().__init__()
        self.bn_l = BatchNormAct(in_ch, ACT_NONE)
        self.bn_h = BatchNormAct(out_ch, ACT_NONE)
        self.conv_ch = ConvParams(out_ch, in_ch, 1, 1)
        self.attn = LinearAttentionDecoder(in_ch, out_ch, heads=heads, dim_head=out_ch // heads, attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size,
                                           projection=projection, rel_pos=rel_pos)
        self.bn2 = BatchNormAct(out_ch, ACT_RELU)
        self.relu = _NoParams()
        self.mlp = ConvParams(out_ch, out_ch, 1, 1, bias=False)

    def forward(self, x1, x2):
        """x1: low-resolution, x2: high-resolution"""
        xa, xb = ops.fork(x1, 2)
        residue = ops.resize_ac_to(ops.linear(xa, self.conv_ch.weight, self.conv_ch.bias), x2.shape[1], x2.shape[2])
        out = self.attn(self.bn_h(x2), self.bn_l(xb), residue)
        o, r2 = ops.fork(out, 2)
        return ops.linear(self.bn2(o), self.mlp.weight, residual=r2)


class _MaxPool2d(nn.Module):
    """the nn.MaxPool2d(2) slot of a down block (no parameters)"""

    def forward(self, x):
        return ops.maxpool2x2(x)


class down_block_trans(nn.Module):
    """conv_trans_utils.py:385-416"""

    def __init__(self, in_ch, out_ch, num_block, bottleneck=False, maxpool=True, heads=4, dim_head=64, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp',
                 rel_pos=True):
        super().__init__()
        if bottleneck or not maxpool:
            raise NotImplementedError("down_block_trans: bottleneck=False and maxpool=True only")
        assert num_block > 0
        blocks = [_MaxPool2d(), BasicBlock(in_ch, out_ch, stride=1)]
        for _ in range(num_block):
            blocks.append(BasicTransBlock(out_ch, heads, dim_head, attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size, projection=projection, rel_pos=rel_pos))
        self.blocks = nn.Sequential(*blocks)

    def forward(self, x):
        return self.blocks(x)


class up_block_trans(nn.Module):
    """conv_trans_utils.py:418-445"""

    def __init__(self, in_ch, out_ch, num_block, bottleneck=False, heads=4, dim_head=64, attn_drop=0., proj_drop=0., reduce_size=16, projection='interp', rel_pos=True):
        super().__init__()
        if bottleneck:
            raise NotImplementedError("up_block_trans: bottleneck=False only")
        self.attn_decoder = BasicTransDecoderBlock(in_ch, out_ch, heads=heads, dim_head=dim_head, attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size,
                                                   projection=projection, rel_pos=rel_pos)
        blocks = [BasicTransBlock(out_ch, heads, dim_head, attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size, projection=projection, rel_pos=rel_pos)
                  for _ in range(num_block)]
        blocks.append(BasicBlock(2 * out_ch, out_ch, stride=1))
        self.blocks = nn.Sequential(*blocks)

    def forward(self, x1, x2):
        xa, xb = ops.fork(x2, 2)
        return self.blocks(ops.cat_channels(self.attn_decoder(x1, xa), xb))


class up_block(nn.Module):
    """unet_utils.py:280-308: resize x2 and the 1 x 1 convolution with bias (commuted: the product runs at the low resolution), cat([x2, x1]), BasicBlocks"""

    def __init__(self, in_ch, out_ch, num_block, scale=(2, 2), bottleneck=False):
        super().__init__()
        if bottleneck or tuple(scale) != (2, 2):
            raise NotImplementedError("up_block: scale (2, 2) and bottleneck=False only")
        self.scale = scale
        self.conv_ch = ConvParams(out_ch, in_ch, 1, 1)
        blocks = [BasicBlock(2 * out_ch, out_ch)] + [BasicBlock(out_ch, out_ch) for _ in range(num_block - 1)]
        self.conv = nn.Sequential(*blocks)

    def forward(self, x1, x2):
        x1 = ops.resize_ac_to(ops.linear(x1, self.conv_ch.weight, self.conv_ch.bias), 2 * x1.shape[1], 2 * x1.shape[2])
        return self.conv(ops.cat_channels(x2, x1))


class UTNet(nn.Module):
    """UTNet.py:19-105.  model(img [B, in_chan, H, W]) -> logits [B, 1, H, W]; H and W multiples of 128"""

    def __init__(self, in_chan, base_chan, num_classes=1, reduce_size=8, block_list='234', num_blocks=[1, 2, 4], projection='interp', num_heads=[2, 4, 8], attn_drop=0.,
                 proj_drop=0., bottleneck=False, maxpool=True, rel_pos=True, aux_loss=False):
        super().__init__()
        built = (block_list == '1234' and list(num_blocks) == [1, 1, 1, 1] and list(num_heads) == [4, 4, 4, 4] and projection == 'interp' and reduce_size == REDUCE
                 and rel_pos and not aux_loss and not bottleneck and maxpool and num_classes == 1)
        dim_heads = [base_chan * m // 4 for m in (2, 4, 8, 16)]
        if not built or base_chan % 16 != 0 or any(d not in DIM_HEADS for d in dim_heads) or in_chan <= 0 or not (0.0 <= attn_drop < 1.0 and 0.0 <= proj_drop < 1.0):
            raise NotImplementedError(
                f"UTNet(in_chan={in_chan}, base_chan={base_chan}, num_classes={num_classes}, reduce_size={reduce_size}, block_list={block_list!r}, num_blocks={num_blocks}, "
                f"projection={projection!r}, num_heads={num_heads}, attn_drop={attn_drop}, proj_drop={proj_drop}, bottleneck={bottleneck}, maxpool={maxpool}, "
                f"rel_pos={rel_pos}, aux_loss={aux_loss}) is not built: the kernels cover block_list='1234', num_blocks=[1,1,1,1], num_heads=[4,4,4,4], "
                "projection='interp', reduce_size=8, rel_pos=True, aux_loss=False, bottleneck=False, maxpool=True, num_classes=1 (as multi_train_BASE.py builds it), "
                "every dim_head in 16 / 32 / 64 / 128 and dropout rates in [0, 1)")
        self.aux_loss = aux_loss
        self.in_chan = in_chan
        b = base_chan
        kw = dict(attn_drop=attn_drop, proj_drop=proj_drop, reduce_size=reduce_size, projection=projection, rel_pos=rel_pos)
        self.inc = nn.Sequential(BasicBlock(in_chan, b, exact=True), BasicBlock(b, b, exact=True))
        self.up4 = up_block(2 * b, b, scale=(2, 2), num_block=2)
        self.down1 = down_block_trans(b, 2 * b, num_block=num_blocks[-4], bottleneck=bottleneck, maxpool=maxpool, heads=num_heads[-4], dim_head=2 * b // num_heads[-4], **kw)
        self.up3 = up_block_trans(4 * b, 2 * b, num_block=0, bottleneck=bottleneck, heads=num_heads[-3], dim_head=2 * b // num_heads[-3], **kw)
        self.down2 = down_block_trans(2 * b, 4 * b, num_block=num_blocks[-3], bottleneck=bottleneck, maxpool=maxpool, heads=num_heads[-3], dim_head=4 * b // num_heads[-3], **kw)
        self.up2 = up_block_trans(8 * b, 4 * b, num_block=0, bottleneck=bottleneck, heads=num_heads[-2], dim_head=4 * b // num_heads[-2], **kw)
        self.down3 = down_block_trans(4 * b, 8 * b, num_block=num_blocks[-2], bottleneck=bottleneck, maxpool=maxpool, heads=num_heads[-2], dim_head=8 * b // num_heads[-2], **kw)
        self.up1 = up_block_trans(16 * b, 8 * b, num_block=0, bottleneck=bottleneck, heads=num_heads[-1], dim_head=8 * b // num_heads[-1], **kw)
        self.down4 = down_block_trans(8 * b, 16 * b, num_block=num_blocks[-1], bottleneck=bottleneck, maxpool=maxpool, heads=num_heads[-1], dim_head=16 * b // num_heads[-1], **kw)
        self.outc = ConvParams(num_classes, b, 1, 1)
        self._init_weights()

    def _init_weights(self):
        """nn.Conv2d's own initialisation everywhere (the reference sets nothing else); BatchNorm 1 / 0; the bias tables are drawn in their constructor"""
        for m in self.modules():
            if isinstance(m, ConvParams):
                nn.init.kaiming_uniform_(m.weight, a=math.sqrt(5))
                if m.bias is not None:
                    bound = 1.0 / math.sqrt(m.weight[0].numel())
                    nn.init.uniform_(m.bias, -bound, bound)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_chan:
            raise ValueError(f"UTNet: input [B, {self.in_chan}, H, W] expected, got {tuple(x.shape)}")
        B, Cin, H, W = x.shape
        if H <= 0 or W <= 0 or H % 128 or W % 128 or (H // 16 == REDUCE) != (W // 16 == REDUCE):
            raise ValueError(f"UTNet: input height and width must be multiples of 128 (every query grid a multiple of 8, the deepest map at least 8 x 8), and a map "
                             f"that is 8 high must be 8 wide; got {H} x {W}")
        x = x.permute(0, 2, 3, 1)
        if Cin % 4:          # the NHWC kernels take channel counts that are multiples of four: zero channels, which the first block's padded parameters keep at zero
            x = torch.cat([x, x.new_zeros(B, H, W, 4 - Cin % 4)], dim=-1)
        x = x.contiguous()
        x1, s1 = ops.fork(self.inc(x), 2)
        x2, s2 = ops.fork(self.down1(x1), 2)
        x3, s3 = ops.fork(self.down2(x2), 2)
        x4, s4 = ops.fork(self.down3(x3), 2)
        x5 = self.down4(x4)
        out = self.up1(x5, s4)
        out = self.up2(out, s3)
        out = self.up3(out, s2)
        out = self.up4(out, s1)
        return ops.rowdot(out, self.outc.weight, self.outc.bias).view(B, 1, H, W)
