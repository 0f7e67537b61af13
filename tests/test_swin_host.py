"""CPU-only checks of SwinUnet's surface (state_dict inventory, constructor, buffers: recorded from the real reference class by tools/gen_swin_golden.py)
and of the shifted-window attention: the pure-torch restatement the GPU tests compare against (roll / partition / bias / mask / softmax,
Models/Transformer/SwinUnet.py:108-139 and :186-258), the region-id rule the kernel derives its shift mask from against the reference's construction of the
attn_mask buffer, the relative-position index, and the C ABI's argument validation (error codes before any launch)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

WS = 8
FIXTURE = "swinunet_step_256"


# ---- the restatement (the dtype of its arguments; fp64 is the GPU tests' yardstick) -----------------------------------------------------------------
def window_partition(x, ws=WS):
    """SwinUnet.py:38-50: [B, H, W, C] -> [B * nW, ws, ws, C]"""
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def window_reverse(windows, H, W, ws=WS):
    """SwinUnet.py:53-67"""
    B = int(windows.shape[0] / (H * W / ws / ws))
    x = windows.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def relative_position_index(ws=WS):
    """SwinUnet.py:88-97"""
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def reference_attn_mask(H, W, shift, ws=WS):
    """SwinUnet.py:202-221: [nW, ws*ws, ws*ws] of 0 / -100, None without a shift"""
    if shift == 0:
        return None
    img_mask = torch.zeros((1, H, W, 1))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img_mask, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))


def region_ids(H, W, shift, ws=WS):
    """the kernel's rule, in numpy: region id 3 r(y') + r(x') of the SHIFTED coordinates, r(t) = (t >= n - ws) + (t >= n - shift) -> [H, W] ints"""
    r = lambda t, n: (t >= n - ws).astype(np.int64) + (t >= n - shift).astype(np.int64)
    return 3 * r(np.arange(H), H)[:, None] + r(np.arange(W), W)[None, :]


def kernel_rule_mask(H, W, shift, ws=WS):
    """[nW, 64, 64] of 0 / -100 from region_ids, windows in window_partition's order"""
    rid = region_ids(H, W, shift, ws).reshape(H // ws, ws, W // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)
    return np.where(rid[:, :, None] != rid[:, None, :], -100.0, 0.0)


def window_attention_restated(qkv, table, H, W, heads, shift, ws=WS):
    """SwinTransformerBlock.forward's attention path (:234-258) around WindowAttention.forward (:114-136) without its two Linear layers, which act per token and
    commute with the rearrangements: qkv [B, H*W, 3C] natural order -> (out [B, H*W, C] natural order, probabilities [B*nW, heads, 64, 64])"""
    B, N, C3 = qkv.shape
    Cn = C3 // 3
    x = qkv.view(B, H, W, C3)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = window_partition(x, ws).view(-1, ws * ws, C3)
    B_, n = xw.shape[0], ws * ws
    t = xw.reshape(B_, n, 3, heads, Cn // heads).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    q = q * (Cn // heads) ** -0.5
    attn = q @ k.transpose(-2, -1)
    bias = table[relative_position_index(ws).view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    mask = reference_attn_mask(H, W, shift, ws)
    if mask is not None:
        nW = mask.shape[0]
        attn = attn.view(B_ // nW, nW, heads, n, n) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, n, n)
    p = torch.softmax(attn, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B_, n, Cn)
    o = window_reverse(o.view(-1, ws, ws, Cn), H, W, ws)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B, N, Cn), p


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (16, 24), (32, 32), (64, 64), (24, 16)])
def test_region_id_rule_reproduces_the_reference_mask_construction(H, W):
    """the mask the kernel derives from shifted coordinates == the attn_mask buffer SwinTransformerBlock.__init__ builds, window by window"""
    want = reference_attn_mask(H, W, 4).numpy()
    got = kernel_rule_mask(H, W, 4)
    assert want.shape == got.shape == ((H // 8) * (W // 8), 64, 64)
    assert np.array_equal(want, got)
    # four classes: a window's mask depends only on being in the last window row and / or column
    nwy, nwx = H // 8, W // 8
    cls = {}
    for w in range(nwy * nwx):
        key = (w // nwx == nwy - 1, w % nwx == nwx - 1)
        cls.setdefault(key, got[w])
        assert np.array_equal(cls[key], got[w])
    assert not cls[(False, False)].any() and all(cls[k].any() for k in cls if k != (False, False))


def test_relative_position_index_is_the_closed_form_the_kernel_uses():
    idx = relative_position_index().numpy()
    i, j = np.arange(64)[:, None], np.arange(64)[None, :]
    assert np.array_equal(idx, ((i >> 3) - (j >> 3) + 7) * 15 + ((i & 7) - (j & 7) + 7))
    assert idx.min() == 0 and idx.max() == 224


def test_restatement_is_a_per_window_softmax_with_wrapped_neighbours():
    """independent of the rearrangement helpers: one output row recomputed token by token from the definition (shifted window membership by coordinates,
    region mask, bias by coordinate difference)"""
    g = torch.Generator().manual_seed(3)
    B, H, W, heads, shift = 1, 16, 24, 2, 4
    Cn = heads * 32
    qkv = torch.randn(B, H * W, 3 * Cn, generator=g, dtype=torch.float64)
    table = torch.randn(225, heads, generator=g, dtype=torch.float64)
    out, _ = window_attention_restated(qkv, table, H, W, heads, shift)
    rid = region_ids(H, W, shift)
    for (y, x, h) in ((0, 0, 0), (3, 5, 1), (15, 23, 0), (4, 4, 1), (11, 20, 1), (12, 3, 0)):
        ys, xs = (y - shift) % H, (x - shift) % W          # where the token sits in the rolled image
        wy, wx = ys // 8, xs // 8
        q = qkv[0, y * W + x, h * 32:(h + 1) * 32] * 32 ** -0.5
        s, vs = [], []
        for jy in range(8):
            for jx in range(8):
                kys, kxs = wy * 8 + jy, wx * 8 + jx
                tok = ((kys + shift) % H) * W + (kxs + shift) % W
                k = qkv[0, tok, Cn + h * 32:Cn + (h + 1) * 32]
                bias = table[(ys % 8 - jy + 7) * 15 + (xs % 8 - jx + 7), h]
                s.append(q @ k + bias + (-100.0 if rid[kys, kxs] != rid[ys, xs] else 0.0))
                vs.append(qkv[0, tok, 2 * Cn + h * 32:2 * Cn + (h + 1) * 32])
        p = torch.softmax(torch.stack(s), 0)
        want = (p[:, None] * torch.stack(vs)).sum(0)
        assert torch.allclose(out[0, y * W + x, h * 32:(h + 1) * 32], want, rtol=1e-12, atol=1e-12), (y, x, h)


def test_winattn_abi_refuses_unbuilt_shapes_without_gpu():
    """MDVIT_E_SHAPE (1) before any launch: H or W no multiple of 8, C != heads * 32, a shift outside {0, 4}, a shift with a one-window-high / -wide grid"""
    from mdvit_amd import _lib
    lib = _lib.load()
    bad = [(1, 12, 16, 96, 3, 0), (1, 16, 20, 96, 3, 0), (1, 16, 16, 96, 4, 0), (1, 16, 16, 100, 3, 0), (1, 16, 16, 96, 3, 2), (1, 16, 16, 96, 3, 8),
           (1, 16, 16, 96, 3, -4), (1, 8, 16, 96, 3, 4), (1, 16, 8, 96, 3, 4), (1, 8, 8, 96, 3, 4), (0, 16, 16, 96, 3, 0), (1, 0, 16, 96, 3, 0)]
    for (B, H, W, Cn, heads, shift) in bad:
        assert lib.mdvit_winattn_fwd(None, None, None, None, B, H, W, Cn, heads, shift, None) == 1, (B, H, W, Cn, heads, shift)
        assert b"winattn_fwd" in lib.mdvit_last_error()
        assert lib.mdvit_winattn_bwd(None, None, None, None, None, None, None, 0, 0, B, H, W, Cn, heads, shift, None) == 1, (B, H, W, Cn, heads, shift)
        assert b"winattn_bwd" in lib.mdvit_last_error()
    # a built shape with null operands is refused too, still without a launch
    assert lib.mdvit_winattn_fwd(None, None, None, None, 1, 16, 16, 96, 3, 4, None) == 1
    assert b"null" in lib.mdvit_last_error()
    assert lib.mdvit_winattn_bwd(None, None, None, None, None, None, None, 0, 0, 2, 8, 8, 96, 3, 0, None) == 1
    # the partial rows of the table gradient: one row of 225 per (sample, window, head)
    assert lib.mdvit_winattn_bwd_ws_bytes(2, 16, 24, 6) == 4 * 2 * 6 * 6 * 225
    assert lib.mdvit_winattn_bwd_ws_bytes(2, 12, 24, 6) == 0


# ---- the model's surface against the fixture of the real class --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import mdvit_amd
    return mdvit_amd.SwinUnet(img_size=256, window_size=8)


def test_state_dict_inventory_and_parameter_names_are_the_reference_fixture(golden, model):
    from swin_params import swin_spec
    g = golden(FIXTURE)
    sd = model.state_dict()
    keys = [str(k) for k in g["sd_keys"]]
    assert len(keys) == 354 and sorted(sd) == keys
    for k, shp in zip(keys, g["sd_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v >= 0), k
    names = sorted(n for n, _ in model.named_parameters())
    assert len(names) == 322 and names == [str(n) for n in g["grad_names"]]
    spec = swin_spec()
    assert sorted(spec) == names and all(tuple(sd[k].shape) == tuple(s) for k, s in spec.items())


def test_constructor_defaults_are_the_reference_ones(golden):
    import mdvit_amd
    want = json.loads(str(golden(FIXTURE)["ctor"]))
    got = [[n, p.default] for n, p in inspect.signature(mdvit_amd.SwinUnet.__init__).parameters.items() if n != "self"]
    assert got == want
    assert list(inspect.signature(mdvit_amd.SwinUnet.forward).parameters) == ["self", "x"]


def test_unbuilt_configurations_raise_at_construction():
    import mdvit_amd
    for kw in ({}, {"img_size": 256, "window_size": 7}, {"img_size": 320, "window_size": 8}, {"img_size": 256, "window_size": 8, "num_classes": 2}):
        with pytest.raises(NotImplementedError, match="window_size = 8"):
            mdvit_amd.SwinUnet(**kw)


def test_reference_shaped_checkpoints_load_strictly(golden, model):
    """a single-GPU checkpoint (the state_dict as it is, buffers included) with strict=True; a DataParallel one ('module.' prefix) through load_reference_state_dict"""
    import mdvit_amd
    from swin_params import make_swin_params
    g = golden(FIXTURE)
    sd = {k: torch.from_numpy(v) for k, v in make_swin_params(5).items()}
    for k, shp in zip(g["sd_keys"], g["sd_shapes"]):
        k = str(k)
        if k not in sd:          # the buffers a reference checkpoint carries: relative_position_index (int64) and attn_mask
            shape = tuple(int(v) for v in shp if v >= 0)
            sd[k] = torch.zeros(shape, dtype=torch.int64 if k.endswith("relative_position_index") else torch.float32)
    assert len(sd) == 354
    m = mdvit_amd.SwinUnet(img_size=256, window_size=8)
    m.load_state_dict(sd, strict=True)
    mdvit_amd.load_reference_state_dict(m, {"module." + k: v for k, v in sd.items()})
    w = m.swin_unet.layers[2].blocks[3].attn.qkv.weight
    assert torch.equal(w.detach(), sd["swin_unet.layers.2.blocks.3.attn.qkv.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.endswith("norm_up.weight")}, strict=True)


def test_init_weights_follow_the_reference(model):
    """SwinUnet.py:672-679 and :105: Linear trunc-normal 0.02 with zero bias, LayerNorm 1 / 0, the bias table trunc-normal 0.02"""
    s = model.swin_unet
    for w in (s.layers[1].blocks[0].attn.qkv.weight, s.layers_up[1].blocks[2].mlp.fc2.weight, s.up.expand.weight, s.concat_back_dim[2].weight,
              s.layers[3].blocks[1].attn.relative_position_bias_table):
        assert abs(float(w.detach().std()) - 0.02) < 0.004 and float(w.detach().abs().max()) <= 2.0
    assert float(s.layers[0].blocks[1].attn.proj.bias.detach().abs().max()) == 0.0 and float(s.concat_back_dim[1].bias.detach().abs().max()) == 0.0
    n = s.layers[0].downsample.norm
    assert bool((n.weight == 1).all()) and bool((n.bias == 0).all()) and n.eps == 1e-5
    # DropPath: the linspace rule over the 12 encoder blocks, mirrored in the decoder
    enc = [b.drop_path_p for l in s.layers for b in l.blocks]
    assert np.allclose(enc, np.linspace(0, 0.1, 12)) and enc[0] == 0.0
    assert [b.drop_path_p for b in s.layers_up[1].blocks] == enc[4:10] and [b.drop_path_p for b in s.layers_up[3].blocks] == enc[0:2]


def test_buffers_are_the_reference_ones_and_the_kernel_rule_matches_them(golden, model):
    g = golden(FIXTURE)
    mods = dict(model.named_modules())
    names = [str(n) for n in g["block_names"]]
    assert names == [n for n, m in model.named_modules() if type(m).__name__ == "SwinTransformerBlock"] and len(names) == 22
    for n in names:
        assert np.array_equal(mods[n].attn.relative_position_index.numpy(), g["rel_index"]), n
        assert mods[n].attn.relative_position_index.dtype == torch.int64
    shifted = [str(n) for n in g["mask_blocks"]]
    assert shifted == [n for n in names if mods[n].attn_mask is not None] == [n for n in names if mods[n].shift_size > 0] and len(shifted) == 10
    off = g["mask_offsets"]
    for i, n in enumerate(shifted):
        blk = mods[n]
        H, W = blk.input_resolution
        mask = blk.attn_mask.numpy()
        assert mask.dtype == np.float32 and blk.shift_size == 4
        assert np.array_equal((mask == -100.0).sum((1, 2)), g["mask_counts"][off[i]:off[i + 1]]), n
        assert np.array_equal(mask, kernel_rule_mask(H, W, 4)), n          # what the kernel derives from coordinates == the buffer it never reads
    # the last stage: the grid is one window, the shift is dropped (:186-189)
    assert all(b.shift_size == 0 and b.window_size == 8 for b in model.swin_unet.layers[3].blocks)


def test_restatement_reproduces_the_reference_attention_statistic_of_a_shifted_block(golden):
    """layers.0.blocks.1 (shift 4, 64 windows with all four mask classes) rebuilt in fp64 from the fixture's weights and input: patch embedding, block 0, then
    LN1, the qkv product and the restatement -- the median over rows of the largest probability equals what a forward hook on the reference's own softmax
    module recorded.  This pins the comparator the GPU tests use to the reference's WindowAttention plus shift logic."""
    import torch.nn.functional as F
    from oracle.gen_golden import synth_image
    from swin_params import make_swin_params
    g = golden(FIXTURE)
    S, B, seed, _ = (int(v) for v in g["meta"])
    P = {k: torch.from_numpy(v).double() for k, v in make_swin_params(seed).items()}
    pre = "swin_unet."
    ln = lambda x, n: F.layer_norm(x, (x.shape[-1],), P[pre + n + ".weight"], P[pre + n + ".bias"], 1e-5)
    lin = lambda x, n: F.linear(x, P[pre + n + ".weight"], P.get(pre + n + ".bias"))
    x = F.conv2d(synth_image(1500 + seed, B, S, S).double(), P[pre + "patch_embed.proj.weight"], P[pre + "patch_embed.proj.bias"], stride=4).flatten(2).transpose(1, 2)
    x = ln(x, "patch_embed.norm")
    H = W = S // 4
    stats = []
    for j, shift in ((0, 0), (1, 4)):
        b = f"layers.0.blocks.{j}"
        o, p = window_attention_restated(lin(ln(x, b + ".norm1"), b + ".attn.qkv"), P[pre + b + ".attn.relative_position_bias_table"], H, W, 3, shift)
        stats.append(float(p.max(-1).values.median()))
        x = x + lin(o, b + ".attn.proj")
        x = x + lin(F.gelu(lin(ln(x, b + ".norm2"), b + ".mlp.fc1")), b + ".mlp.fc2")
    names = [str(n) for n in g["block_names"]]
    for j in (0, 1):
        want = float(g["pmax_median"][names.index(f"swin_unet.layers.0.blocks.{j}")])
        assert abs(stats[j] - want) <= 1e-4 * want, (j, stats[j], want)
