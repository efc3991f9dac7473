"""CPU: the 2-byte value entry points of include/dfx_msda.h (csrc/msda_forward.hip, csrc/msda_backward.hip) are
declared with fp32 locations and weights, bound in dfx/_lib.py, exported by the library, and the CPU-tensor rule of the
operator covers them."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dfx_msda_forward_bf16", "dfx_msda_forward_f16", "dfx_msda_backward_bf16", "dfx_msda_backward_f16")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_msda.h")).read(), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} not declared"
    return " ".join(m.group(1).split())


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_half_entry_points(name):
    decl = _declaration(name)
    assert decl.startswith("const uint16_t *value,")
    assert "const float *loc, const float *aw" in decl
    if "backward" in name:
        assert "const uint16_t *grad_out" in decl and "float *grad_value_f32, float *grad_loc, float *grad_aw" in decl
    else:
        assert "uint16_t *out, void *stream" in decl


def test_binding_and_library():
    from dfx import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("bf16", "f32").replace("f16", "f32")]
    lib = ctypes.CDLL(_lib.library_path())
    for name in NAMES:
        assert hasattr(lib, name)
    assert _lib.abi_version() == 5


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_cpu_tensors_are_rejected(dt):
    import MultiScaleDeformableAttention as MSDA
    v = torch.zeros(1, 4, 8, 32, dtype=dt)
    s = torch.tensor([[2, 2]])
    l = torch.tensor([0])
    loc = torch.zeros(1, 3, 8, 1, 4, 2)
    aw = torch.zeros(1, 3, 8, 1, 4)
    with pytest.raises(RuntimeError, match="CPU"):
        MSDA.ms_deform_attn_forward(v, s, l, loc, aw, 64)
    with pytest.raises(RuntimeError, match="CPU"):
        MSDA.ms_deform_attn_backward(v, s, l, loc, aw, torch.zeros(1, 3, 256, dtype=dt), 64)
