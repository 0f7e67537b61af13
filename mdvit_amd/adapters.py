"""The squeeze-excite adapters of the reference's "SOTA adapter" baselines, under the reference's attribute names (so that a
reference state_dict loads key for key), computing through ops.se_adapter (csrc/se_adapter.hip):

  SELayer          <- Models/Sota_adapters/se_module_vector.py:8-31          fc.0 / fc.2 Linear (ReLU between, Sigmoid behind when with_sigmoid)
  DomainAttention  <- Models/Sota_adapters/domain_attention_module.py:19-66  SE_Layers.{0..3} (no sigmoid) mixed by softmax(fc_1(pool)), one sigmoid, x * gate
  SEBlock          <- Models/Sota_adapters/base_sota_adapt.py:628-637        se_layer (with sigmoid), se * x + x

Activations are NHWC tokens [B, H, W, C] or [B, N, C]; the gate is per (sample, channel)."""
from __future__ import annotations

from torch import nn

from . import ops
from .blocks import LinearParams, _NoParams


class SELayer(nn.Module):
    """parameters only: the owner (DomainAttention / SEBlock) runs the whole adapter in one operator"""

    def __init__(self, channel, reduction=16, with_sigmoid=True):
        super().__init__()
        self.with_sigmoid = with_sigmoid
        slots = [LinearParams(channel, channel // reduction), _NoParams(), LinearParams(channel // reduction, channel)]
        self.fc = nn.Sequential(*(slots + ([_NoParams()] if with_sigmoid else [])))

    def params(self):
        return [self.fc[0].weight, self.fc[0].bias, self.fc[2].weight, self.fc[2].bias]

    def forward(self, *a, **k):
        raise RuntimeError("SELayer only holds parameters; DomainAttention / SEBlock compute through mdvit_amd.ops.se_adapter (HIP)")


class DomainAttention(nn.Module):
    def __init__(self, planes, reduction=16, nclass_list=None, fixed_block=False):
        super().__init__()
        if fixed_block:
            raise NotImplementedError("fixed_block=True is not built (the reference's models never set it)")
        self.planes = planes
        self.n_datasets = 4                    # num_adapters, domain_attention_module.py:24
        self.fixed_block = fixed_block
        self.SE_Layers = nn.ModuleList([SELayer(planes, reduction, with_sigmoid=False) for _ in range(self.n_datasets)])
        self.fc_1 = LinearParams(planes, self.n_datasets)

    def forward(self, x):
        params = [self.fc_1.weight, self.fc_1.bias]
        for se in self.SE_Layers:
            params += se.params()
        return ops.se_adapter(x, "dase", params)


class SEBlock(nn.Module):
    def __init__(self, channel, reduction):
        super().__init__()
        self.se_layer = SELayer(channel, reduction, with_sigmoid=True)

    def forward(self, x):
        return ops.se_adapter(x, "use", self.se_layer.params())
