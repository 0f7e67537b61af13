"""CPU-only checks of the BASE_DASE / BASE_USE surface: the state_dict inventory and the constructor the real reference has (recorded in the fixtures by
tools/gen_adapter_golden.py), the C ABI's argument validation and struct layout, and the import path without the library."""
import ctypes as C
import inspect
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

MODELS = ("BASE_DASE", "BASE_USE")


@pytest.mark.parametrize("model", MODELS)
def test_state_dict_inventory_is_the_reference_fixture(golden, model):
    import mdvit_amd
    from adapter_params import adapter_spec, make_adapter_params
    g = golden(model.lower() + "_step_64")
    m = getattr(mdvit_amd, model)(img_size=64)
    sd = m.state_dict()
    keys = [str(k) for k in g["sd_keys"]]
    assert len(keys) == {"BASE_DASE": 620, "BASE_USE": 512}[model]
    assert sorted(sd) == keys
    for k, shp in zip(keys, g["sd_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v >= 0), k
    assert sorted(n for n, _ in m.named_parameters()) == [str(n) for n in g["grad_names"]]
    # the shared weight rule names exactly the adapters' parameters, and a strict load of it (plus the shared-module aliases) leaves nothing open
    spec = adapter_spec(model)
    assert set(spec) == {k for k in sd if "adapter" in k} and all(tuple(sd[k].shape) == tuple(s) for k, s in spec.items())
    from oracle.params import alias_map
    full = {k: torch.from_numpy(v) for k, v in make_adapter_params(3, model).items()}
    full.update({a: full[s] for a, s in alias_map("BASE").items()})
    m.load_state_dict(full, strict=True)


@pytest.mark.parametrize("model", MODELS)
def test_constructor_defaults_are_the_reference_ones(golden, model):
    import mdvit_amd
    want = json.loads(str(golden(model.lower() + "_step_64")["ctor"]))
    got = []
    for name, p in inspect.signature(getattr(mdvit_amd, model).__init__).parameters.items():
        if name == "self":
            continue
        if p.kind is inspect.Parameter.VAR_KEYWORD:
            got.append(["**" + name, None])
            continue
        d = p.default
        if hasattr(d, "func") and hasattr(d, "keywords"):
            d = {d.func.__name__: dict(d.keywords)}
        elif inspect.isclass(d):
            d = d.__name__
        got.append([name, d])
    assert got == want
    fwd = inspect.signature(getattr(mdvit_amd, model).forward).parameters
    assert list(fwd)[:4] == ["self", "x", "out_feat", "out_seg"] and fwd["out_feat"].default is False and fwd["out_seg"].default is True
    m = getattr(mdvit_amd, model)(img_size=64)
    w = m.decoder_adapters[0].SE_Layers[1].fc[2].weight if model == "BASE_DASE" else m.bridge_adapter.se_layer.fc[0].weight
    assert abs(float(w.detach().std()) - 0.02) < 0.004 and float(w.detach().abs().max()) <= 2.0          # _init_weights: Linear trunc-normal 0.02 ...
    assert all(float(p.detach().abs().max()) == 0.0 for n, p in m.named_parameters() if "adapter" in n and n.endswith(".bias"))      # ... bias 0


def test_existing_models_have_no_adapter_hooks():
    import mdvit_amd
    for cls in (mdvit_amd.BASE, mdvit_amd.MDViT, mdvit_amd.BASE_DSN, mdvit_amd.MDViT_DSN):
        assert cls._encoder_adapter is None and cls._decoder_adapter is None and cls._bridge_adapter_fn is None


def test_package_with_the_adapter_models_imports_without_the_library(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import torch, mdvit_amd\n"
        "from mdvit_amd import _lib, ops, adapters\n"
        "m = mdvit_amd.BASE_USE(img_size=64)\n"
        "assert _lib._lib is None\n"
        "d = ops._se_desc(ops.SE_KINDS['use'], 1, 4, 64, 8, None, None, None, None, None, None)\n"
        "try:\n"
        "    ops._se_sizes(d)\n"
        "except _lib.MdvitHipError as e:\n"
        "    assert 'is missing' in str(e), str(e)\n"
        "else:\n"
        "    raise SystemExit('the adapter sized its buffers without the library')\n"
        "print('ok')\n") % (ROOT,)
    env = dict(os.environ, MDVIT_HIP_LIB=str(tmp_path / "not_built" / "libmdvit_hip.so"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])


def test_se_adapter_refuses_cpu_tensors():
    from mdvit_amd import _lib, ops
    r = 8
    P = [torch.zeros(r, 64), torch.zeros(r), torch.zeros(64, r), torch.zeros(64)]
    with pytest.raises(_lib.MdvitHipError):
        ops.se_adapter(torch.zeros(2, 4, 64), "use", P)


def _desc(kind=0, B=2, N=100, Cn=320, r=20, ptr=None):
    from mdvit_amd import _lib
    d = _lib.SeAdapterDesc()
    d.kind, d.B, d.N, d.C, d.r = kind, B, N, Cn, r
    d.W1 = d.b1 = d.W2 = d.b2 = ptr
    if kind == 0:
        d.Wg = d.bg = ptr
    return d


def test_se_adapter_abi_validates_before_any_launch():
    """descriptor and buffer checks run before any HIP call (no GPU needed); the workspace size is a function of the descriptor alone"""
    from mdvit_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    d = _desc(ptr=p)
    ws_b, save_b = lib.mdvit_se_adapter_ws_bytes(C.byref(d)), lib.mdvit_se_adapter_save_bytes(C.byref(d))
    # [partials B x slabs x C | dz B x 4 x C | dh B x 80 | dlogit B x 4 | dp B x C];  save row: p C | h 80 | w 4 | z 4 C | s C
    assert ws_b == 4 * (2 * 1 * 320 + 2 * 4 * 320 + 2 * 80 + 2 * 4 + 2 * 320) and save_b == 4 * 2 * (320 + 80 + 4 + 4 * 320 + 320)
    u = _desc(kind=1, B=2, N=4100, Cn=128, r=16, ptr=p)
    assert lib.mdvit_se_adapter_ws_bytes(C.byref(u)) == 4 * (2 * 33 * 128 + 2 * 128 + 2 * 16 + 2 * 4 + 2 * 128)
    for bad, word in ((_desc(kind=2, ptr=p), b"kind"), (_desc(Cn=322, ptr=p), b"multiple of 4"), (_desc(Cn=2048, r=128, ptr=p), b"at most"),
                      (_desc(B=0, ptr=p), b"bad shape"), (_desc(kind=0, Cn=1024, r=256, ptr=p), b"hidden units")):
        assert lib.mdvit_se_adapter_ws_bytes(C.byref(bad)) == 0 and lib.mdvit_se_adapter_save_bytes(C.byref(bad)) == 0
        assert lib.mdvit_se_adapter_fwd(C.byref(bad), p, p, p, p, 1 << 30, None) == 1 and word in lib.mdvit_last_error(), lib.mdvit_last_error()
        assert lib.mdvit_se_adapter_bwd(C.byref(bad), p, p, p, None, *[None] * 6, p, 1 << 30, None) == 1 and word in lib.mdvit_last_error()
    assert lib.mdvit_se_adapter_fwd(C.byref(_desc(ptr=None)), p, p, p, p, 1 << 30, None) == 1 and b"NULL weight" in lib.mdvit_last_error()
    assert lib.mdvit_se_adapter_fwd(C.byref(d), p, p, p, p, ws_b - 4, None) == 4 and b"workspace too small" in lib.mdvit_last_error()      # MDVIT_E_WORKSPACE
    assert lib.mdvit_se_adapter_bwd(C.byref(d), p, p, p, None, *[None] * 6, p, ws_b - 4, None) == 4      # ... whether or not dx is asked for
    assert lib.mdvit_se_adapter_bwd(C.byref(d), p, p, p, p, *[None] * 6, p, ws_b - 4, None) == 4
    assert lib.mdvit_se_adapter_bwd(C.byref(u), p, p, p, None, None, None, None, None, p, None, p, 1 << 30, None) == 1 and b"USE has no" in lib.mdvit_last_error()
    off = C.c_void_p(p.value + 4)
    assert lib.mdvit_se_adapter_fwd(C.byref(d), off, p, p, p, 1 << 30, None) == 3                          # MDVIT_E_ALIGN


def test_se_adapter_desc_mirror_has_the_layout_of_the_header(tmp_path):
    from mdvit_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include "mdvit_hip.h"', 'int main(void) {', '    printf("size %zu\\n", sizeof(MdvitSeAdapterDesc));']
    for fname, _t in _lib.SeAdapterDesc._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(MdvitSeAdapterDesc, {fname}));')
    lines += ['    printf("kinds %d %d\\n", MDVIT_SE_DASE, MDVIT_SE_USE);', '    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=30).stdout.strip().splitlines()]
    vals = {l[0]: l[1:] for l in out}
    assert int(vals["size"][0]) == C.sizeof(_lib.SeAdapterDesc)
    for fname, _t in _lib.SeAdapterDesc._fields_:
        assert int(vals[fname][0]) == getattr(_lib.SeAdapterDesc, fname).offset, fname
    assert [int(v) for v in vals["kinds"]] == [_lib.SE_DASE, _lib.SE_USE]
