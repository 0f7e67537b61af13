"""CPU-only checks of UTNet's surface (state_dict inventory, constructor, buffers: recorded from the real reference class by tools/gen_utnet_golden.py) and of the
low-rank attention: the pure-torch restatement the GPU tests compare against, in THIS package's layout (NHWC tokens, interleaved heads, the bias indexed by the
query's coarse cell and added before the scale, k / v reduced to 8 x 8 BEFORE their pointwise product), pinned to 1e-10 to the fp64 outputs, probabilities and
gradients of the reference's own LinearAttention / LinearAttentionDecoder (Models/Hybrid_models/UTNetFolder/conv_trans_utils.py:150-282); and the C ABI's
argument validation (error codes before any launch)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

R = 8
FIXTURES = ("utnet_step_128", "utnet_step_256")


# ---- the restatement (the dtype of its arguments; fp64 is the GPU tests' yardstick) -----------------------------------------------------------------
def relative_position_index(r=R):
    """conv_trans_utils.py:357-367"""
    coords = torch.stack(torch.meshgrid([torch.arange(r), torch.arange(r)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += r - 1
    rel[:, :, 1] += r - 1
    rel[:, :, 0] *= 2 * r - 1
    return rel.sum(-1)


def query_cells(Hq, Wq, r=R):
    """cell(i) = (y // (Hq/8)) * 8 + x // (Wq/8) for the Hq * Wq queries in row-major order: what repeat_interleave of the [8, 8, 64, heads] bias amounts to"""
    y, x = torch.meshgrid(torch.arange(Hq), torch.arange(Wq), indexing="ij")
    return ((y // (Hq // r)) * r + x // (Wq // r)).reshape(-1)


def lowrank_attention_restated(q, k, v, table, Hq, Wq, heads, keep=None):
    """q [B, Hq*Wq, C], k and v [B, 64, C], channel = d * heads + h; table [225, heads]; keep: optional [B, heads, N, 64] dropout scales (0 or 1 / (1 - p)).
    -> (out [B, N, C], P [B, heads, N, 64])"""
    B, N, Cn = q.shape
    D = Cn // heads
    qh, kh, vh = (t.view(B, -1, D, heads).permute(0, 3, 1, 2) for t in (q, k, v))          # [B, heads, tokens, D]
    bias = table[relative_position_index().view(-1)].view(R * R, R * R, heads)[query_cells(Hq, Wq)]          # [N, 64, heads]
    s = (qh @ kh.transpose(-1, -2) + bias.permute(2, 0, 1).unsqueeze(0)) * D ** -0.5
    p = s.softmax(-1)
    pd = p if keep is None else p * keep
    out = (pd @ vh).permute(0, 2, 3, 1).reshape(B, N, Cn)
    return out, p


def _pw(w):
    return w.view(w.shape[0], -1)


def _dw(x_nhwc, w):
    """depthwise 3 x 3 on NHWC"""
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2), w, padding=1, groups=w.shape[0]).permute(0, 2, 3, 1)


def _reduce(t_nhwc):
    """align_corners=True resize to 8 x 8, skipped where the map is 8 high (conv_trans_utils.py:188, :255)"""
    if t_nhwc.shape[1] == R:
        return t_nhwc
    return F.interpolate(t_nhwc.permute(0, 3, 1, 2), size=R, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


def linear_attention_restated(x, P, heads=4):
    """LinearAttention.forward in this package's order of operations: x NHWC [B, H, W, C] -> (out NHWC, probabilities)"""
    B, H, W, Cn = x.shape
    t = _dw(x, P["to_qkv.depthwise.weight"])
    Wqkv = _pw(P["to_qkv.pointwise.weight"])
    inner = Wqkv.shape[0] // 3
    q = t.reshape(B, H * W, Cn) @ Wqkv[:inner].T
    kv = _reduce(t).reshape(B, R * R, Cn) @ Wqkv[inner:].T          # reduce, then project: the product commutes with the per-channel resize
    o, p = lowrank_attention_restated(q, kv[..., :inner], kv[..., inner:], P["relative_position_encoding.relative_position_bias_table"], H, W, heads)
    return _dw(o.view(B, H, W, inner), P["to_out.depthwise.weight"]) @ _pw(P["to_out.pointwise.weight"]).T, p


def linear_attention_decoder_restated(q_in, x, P, heads=4):
    """LinearAttentionDecoder.forward: q_in NHWC [B, HH, WH, out_dim] (high resolution), x NHWC [B, H, W, in_dim] (low resolution)"""
    B, HH, WH, _ = q_in.shape
    Wkv = _pw(P["to_kv.pointwise.weight"])
    inner = Wkv.shape[0] // 2
    kv = _reduce(_dw(x, P["to_kv.depthwise.weight"])).reshape(B, R * R, -1) @ Wkv.T
    q = _dw(q_in, P["to_q.depthwise.weight"]).reshape(B, HH * WH, -1) @ _pw(P["to_q.pointwise.weight"]).T
    o, p = lowrank_attention_restated(q, kv[..., :inner], kv[..., inner:], P["relative_position_encoding.relative_position_bias_table"], HH, WH, heads)
    return _dw(o.view(B, HH, WH, inner), P["to_out.depthwise.weight"]) @ _pw(P["to_out.pointwise.weight"]).T, p


def _close(got, want, name, tol=1e-10):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert e <= tol, f"{name}: {e:.2e}"


@pytest.mark.parametrize("which", ["enc", "dec"])
def test_restatement_reproduces_the_reference_modules_in_fp64(golden, which):
    """output, probabilities, input gradients and parameter gradients of the reference's own modules, to 1e-10"""
    from utnet_params import small_attention_case, small_sample
    g = golden("utnet_attention_small")
    assert np.array_equal(g["rel_index"].astype(np.int64), relative_position_index().numpy())
    params, inputs, gy = small_attention_case(which)
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in params.items()}
    ins = {k: torch.from_numpy(v).requires_grad_(True) for k, v in inputs.items()}
    nhwc = {k: t.permute(0, 2, 3, 1) for k, t in ins.items()}
    out, prob = linear_attention_restated(nhwc["x"], P) if which == "enc" else linear_attention_decoder_restated(nhwc["q"], nhwc["x"], P)
    out_nchw = out.permute(0, 3, 1, 2)
    _close(small_sample(out_nchw.contiguous()), g[which + "_out"], "out")
    _close(small_sample(prob.contiguous()), g[which + "_prob"], "probabilities")
    out_nchw.backward(torch.from_numpy(gy))
    for k, t in ins.items():
        _close(small_sample(t.grad), g[f"{which}_grad_in_{k}"], "grad " + k)
    for k, t in P.items():
        _close(small_sample(t.grad), g[f"{which}_grad_{k}"], "grad " + k)


def test_cells_are_what_repeat_interleave_of_the_bias_gives():
    """conv_trans_utils.py:371-379 on a [8, 8] grid of cell ids"""
    for Hq, Wq in ((8, 8), (16, 24), (24, 40), (64, 64)):
        ids = torch.arange(R * R).view(R, R)
        want = torch.repeat_interleave(torch.repeat_interleave(ids, Hq // R, dim=0), Wq // R, dim=1).reshape(-1)
        assert torch.equal(query_cells(Hq, Wq), want)


# ---- the model's surface against the fixtures of the real class --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import mdvit_amd
    from utnet_params import CTOR
    return mdvit_amd.UTNet(**CTOR)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_state_dict_inventory_and_parameter_names_are_the_reference_fixture(golden, model, fixture):
    from utnet_params import ZERO_GRAD, utnet_spec
    g = golden(fixture)
    sd = model.state_dict()
    keys = [str(k) for k in g["sd_keys"]]
    assert len(keys) == 336 and sorted(sd) == keys
    for k, shp in zip(keys, g["sd_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v >= 0), k
    names = sorted(n for n, _ in model.named_parameters())
    assert len(names) == 185 and names == [str(n) for n in g["grad_names"]]
    spec, bufs = utnet_spec()
    assert sorted(spec) == names and all(tuple(sd[k].shape) == tuple(s) for k, s in spec.items())
    assert sorted(bufs) == sorted(n for n, _ in model.named_buffers()) == [str(n) for n in g["buf_names"]]
    assert [str(n) for n in g["zero_grad_names"]] == sorted(ZERO_GRAD) and set(ZERO_GRAD) <= set(names)
    attn = [n for n, m in model.named_modules() if type(m).__name__ in ("LinearAttention", "LinearAttentionDecoder")]
    assert attn == [str(n) for n in g["attn_names"]] and len(attn) == 7
    assert float(g["pmax_median"].min()) >= 3.0 / 64.0


def test_buffers_and_dim_heads_are_the_reference_ones(golden, model):
    g = golden("utnet_attention_small")
    mods = dict(model.named_modules())
    want = {"down1.blocks.2.attn": 16, "down2.blocks.2.attn": 32, "down3.blocks.2.attn": 64, "down4.blocks.2.attn": 128, "up3.attn_decoder.attn": 16,
            "up2.attn_decoder.attn": 32, "up1.attn_decoder.attn": 64}
    for n, d in want.items():
        a = mods[n]
        assert (a.dim_head, a.heads, a.reduce_size) == (d, 4, 8), n
        idx = a.relative_position_encoding.relative_position_index
        assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), g["rel_index"].astype(np.int64)), n
    assert type(model.up4).__name__ == "up_block" and not hasattr(model.up4, "attn_decoder")


def test_constructor_defaults_are_the_reference_ones(golden):
    import mdvit_amd
    want = json.loads(str(golden(FIXTURES[0])["ctor"]))
    # (a parameter without a default is recorded under the name of inspect's marker class)
    got = [[n, ("_empty" if p.default is inspect.Parameter.empty else p.default)] for n, p in inspect.signature(mdvit_amd.UTNet.__init__).parameters.items() if n != "self"]
    assert got == want and want[0] == ["in_chan", "_empty"]
    assert list(inspect.signature(mdvit_amd.UTNet.forward).parameters) == ["self", "x"]


def test_unbuilt_configurations_raise_at_construction():
    import mdvit_amd
    from utnet_params import CTOR
    with pytest.raises(NotImplementedError, match="block_list='1234'"):
        mdvit_amd.UTNet(3, 32)          # the constructor's own defaults: block_list '234', num_blocks [1, 2, 4], num_heads [2, 4, 8]
    for kw in ({"block_list": "234"}, {"block_list": "01234"}, {"num_blocks": [1, 2, 1, 1]}, {"num_heads": [2, 4, 4, 4]}, {"projection": "maxpool"}, {"reduce_size": 16},
               {"rel_pos": False}, {"aux_loss": True}, {"bottleneck": True}, {"maxpool": False}, {"num_classes": 2}, {"base_chan": 64}, {"base_chan": 16}, {"base_chan": 40},
               {"attn_drop": 1.0}, {"proj_drop": -0.1}):
        with pytest.raises(NotImplementedError, match="is not built"):
            mdvit_amd.UTNet(**{**CTOR, **kw})
    for kw in ({"attn_drop": 0.0, "proj_drop": 0.0}, {"attn_drop": 0.5, "proj_drop": 0.3}):
        mdvit_amd.UTNet(**{**CTOR, **kw})


def test_input_sizes_that_are_no_multiple_of_128_raise_value_error(model):
    for shape in ((1, 3, 192, 192), (1, 3, 128, 200), (1, 3, 64, 64), (1, 1, 128, 128), (1, 3, 128, 256)):
        with pytest.raises(ValueError):
            model(torch.zeros(shape))


def test_reference_shaped_checkpoints_load_strictly(golden, model):
    """a single-GPU checkpoint (the state_dict as it is, buffers included) with strict=True; a DataParallel one ('module.' prefix) through load_reference_state_dict"""
    import mdvit_amd
    from utnet_params import CTOR, make_utnet_params
    g = golden(FIXTURES[0])
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_utnet_params(5).items()}
    for k in g["sd_keys"]:
        if str(k) not in sd:
            assert str(k).endswith("relative_position_index")
            sd[str(k)] = relative_position_index()
    assert len(sd) == 336
    m = mdvit_amd.UTNet(**CTOR)
    m.load_state_dict(sd, strict=True)
    mdvit_amd.load_reference_state_dict(m, {"module." + k: v for k, v in sd.items()})
    assert torch.equal(m.down3.blocks[2].attn.to_qkv.pointwise.weight.detach(), sd["down3.blocks.2.attn.to_qkv.pointwise.weight"])
    assert torch.equal(m.up2.attn_decoder.bn_l.running_var, sd["up2.attn_decoder.bn_l.running_var"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.endswith("outc.bias")}, strict=True)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("mdvit_lrattn_fwd", "mdvit_lrattn_bwd", "mdvit_lrattn_bwd_ws_bytes", "mdvit_maxpool2x2_fwd", "mdvit_maxpool2x2_bwd")


def test_new_abi_symbols_are_in_the_header_and_the_built_library():
    from mdvit_amd import _lib
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_lrattn_abi_refuses_unbuilt_shapes_without_gpu():
    from mdvit_amd import _lib
    lib = _lib.load()
    none18 = lambda B, Hq, Wq, D, heads: lib.mdvit_lrattn_fwd(None, 0, None, None, 0, None, None, None, B, Hq, Wq, D, heads, 0.0, 0, 0, None, None)
    for B, Hq, Wq, D, heads in ((2, 12, 16, 16, 4), (2, 16, 20, 32, 4), (2, 16, 16, 48, 4), (2, 16, 16, 8, 4), (0, 16, 16, 16, 4), (2, 4, 8, 16, 4), (2, 16, 16, 16, 0)):
        assert none18(B, Hq, Wq, D, heads) == 1, (B, Hq, Wq, D, heads)
        assert b"lrattn_fwd" in lib.mdvit_last_error()
        assert lib.mdvit_lrattn_bwd(None, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, 0, B, Hq, Wq, D, heads, 0.0, 0, 0, None, None) == 1
        assert b"lrattn_bwd" in lib.mdvit_last_error()
        assert lib.mdvit_lrattn_bwd_ws_bytes(B, Hq, Wq, D, heads) == 0
    assert none18(2, 16, 16, 16, 4) == 1 and b"null operand" in lib.mdvit_last_error()          # a built shape: the operands are checked next
    # the workspace: one [dK | dV] partial pair per workgroup plus the [64 cells, 64 keys] bias gradient, per image and head
    assert lib.mdvit_lrattn_bwd_ws_bytes(2, 64, 64, 16, 4) == 4 * 2 * 4 * (16 * 2 * 64 * 16 + 64 * 64)
    assert lib.mdvit_lrattn_bwd_ws_bytes(2, 64, 64, 16, 4) < 2 * 4 * 64 * 64 * 64 * 4          # smaller than ONE [B, heads, N, 64] fp32 tensor (8 MiB)
    assert lib.mdvit_lrattn_bwd_ws_bytes(1, 8, 8, 128, 4) == 4 * 4 * (2 * 64 * 128 + 64 * 64)
    assert lib.mdvit_maxpool2x2_fwd(None, None, None, 1, 8, 8, 4, None) == 1 and b"maxpool2x2_fwd" in lib.mdvit_last_error()
    assert lib.mdvit_maxpool2x2_bwd(None, None, None, 1, 8, 8, 4, None) == 1 and b"maxpool2x2_bwd" in lib.mdvit_last_error()
