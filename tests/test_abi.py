"""CPU: the C-ABI library loads and exports every symbol include/*.h declares."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names += re.findall(r"\b(dfx_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def test_header_declares_the_operator_entry_points():
    names = declared_symbols()
    for must in ("dfx_msda_forward_f32", "dfx_msda_forward_f64", "dfx_msda_backward_f32",
                 "dfx_msda_backward_f64", "dfx_msda_fused_forward_f32", "dfx_abi_version", "dfx_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from dfx import _lib
    assert os.path.exists(_lib.library_path()), "libdfx.so not built (python __graft_entry__.py build)"
    lib = ctypes.CDLL(_lib.library_path())
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
    lib.dfx_abi_version.restype = ctypes.c_int
    assert lib.dfx_abi_version() >= 1


def test_python_binding_covers_the_header():
    from dfx import _lib
    bound = set(_lib.SIGNATURES) | {"dfx_abi_version", "dfx_last_error"}
    assert set(declared_symbols()) <= bound


def test_cpu_tensors_are_rejected_like_the_reference():
    """ms_deform_attn.h:38 - AT_ERROR("Not implemented on the CPU")."""
    import torch
    import MultiScaleDeformableAttention as MSDA
    v = torch.zeros(1, 4, 8, 32)
    s = torch.tensor([[2, 2]])
    l = torch.tensor([0])
    loc = torch.zeros(1, 3, 8, 1, 4, 2)
    aw = torch.zeros(1, 3, 8, 1, 4)
    with pytest.raises(RuntimeError, match="CPU"):
        MSDA.ms_deform_attn_forward(v, s, l, loc, aw, 64)
    with pytest.raises(RuntimeError, match="CPU"):
        MSDA.ms_deform_attn_backward(v, s, l, loc, aw, torch.zeros(1, 3, 256), 64)


def test_module_has_reference_surface():
    from models.ops.modules import MSDeformAttn
    m = MSDeformAttn(256, 1, 8, 4)
    keys = set(m.state_dict())
    assert keys == {f"{n}.{p}" for n in ("sampling_offsets", "attention_weights", "value_proj", "output_proj")
                    for p in ("weight", "bias")}
    assert m.im2col_step == 64
    assert m.sampling_offsets.weight.shape == (64, 256) and m.attention_weights.weight.shape == (32, 256)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """Argument validation returns an error code without touching the GPU (no compute call is made here):
    activation codes outside 0..2, kernel sides beyond the 32-bit tap masks of the implicit GEMM."""
    from dfx import _lib
    lib = _lib.load()
    one = 16       # any non-null, 16-byte aligned address: the checks below fail before it would be used
    rc = lib.dfx_gemm_f32(one, 0, 4, 0, one, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, one, 4, 0, 4, 4, 4, 1, 3, 0, 0, 0, None)
    assert rc != 0 and b"activation" in lib.dfx_last_error()
    rc = lib.dfx_gemm_splitk_f32(one, 4, one, 4, 0, 0, 0, 0, 0, one, 4, 4, 4, 4, 7, 2, one, None)
    assert rc != 0 and b"activation" in lib.dfx_last_error()
    rc = lib.dfx_conv2d_igemm_f32(one, one, one, 0, one, 1, 4, 8, 40, 4, 8, 8, 144, 1, 33, 1, 0, 1, 0, 0, None)
    assert rc != 0 and b"kernel sides" in lib.dfx_last_error()


ONE, ODD = 16, 20      # non-null addresses, 16-byte aligned and not: every call below fails (or is empty) before they would be used


def _refused(lib, name, args, cause):
    rc = getattr(lib, name)(*args, None)
    assert rc != 0 and cause in lib.dfx_last_error(), (name, args, rc, lib.dfx_last_error())


def _swap(args, i, value):
    return args[:i] + (value,) + args[i + 1:]


def test_bias_act_entry_rejects_bad_arguments_before_any_launch():
    """x, bias, residual | NULL, out, N, C, HW, relu."""
    lib = _lib_loaded()
    ok = (ONE, ONE, 0, ONE, 2, 3, 8, 1)
    for i, bad in ((4, -1), (5, 0), (5, -3), (6, -1)):
        _refused(lib, "dfx_bias_act_nchw_f32", _swap(ok, i, bad), b"bad dimension")
    for i in (0, 1, 3):
        _refused(lib, "dfx_bias_act_nchw_f32", _swap(ok, i, 0), b"null pointer")
    _refused(lib, "dfx_bias_act_nchw_f32", (ONE, ONE, 0, ONE, 65536, 32768, 1, 1), b"too many planes")
    assert lib.dfx_bias_act_nchw_f32(0, 0, 0, 0, 0, 3, 8, 1, None) == 0          # empty: asked before the pointers
    assert lib.dfx_bias_act_nchw_f32(0, 0, 0, 0, 2, 3, 0, 1, None) == 0


def test_bias_relu_maxpool_entry_rejects_bad_arguments_before_any_launch():
    """x, bias, out, N, C, H, W."""
    lib = _lib_loaded()
    ok = (ONE, ONE, ONE, 2, 3, 5, 7)
    for i, bad in ((3, -1), (4, 0), (5, 0), (6, 0), (6, -2)):
        _refused(lib, "dfx_bias_relu_maxpool_f32", _swap(ok, i, bad), b"bad dimension")
    for i in (0, 1, 2):
        _refused(lib, "dfx_bias_relu_maxpool_f32", _swap(ok, i, 0), b"null pointer")
    assert lib.dfx_bias_relu_maxpool_f32(0, 0, 0, 0, 3, 5, 7, None) == 0


def test_add_layernorm_entry_rejects_bad_arguments_before_any_launch():
    """x, res | NULL, gamma, beta, out, rows, C, eps."""
    lib = _lib_loaded()
    ok = (ONE, ONE, ONE, ONE, ONE, 5, 256, 1e-5)
    for i, bad in ((5, -1), (6, 0), (6, -4)):
        _refused(lib, "dfx_add_layernorm_f32", _swap(ok, i, bad), b"bad dimension")
    for i in (0, 2, 3, 4):
        _refused(lib, "dfx_add_layernorm_f32", _swap(ok, i, 0), b"null pointer")
    for C in (6, 255, 1028, 2048):
        _refused(lib, "dfx_add_layernorm_f32", _swap(ok, 6, C), b"multiple of 4 and <= 1024")
    for i in (0, 1, 2, 3, 4):
        _refused(lib, "dfx_add_layernorm_f32", _swap(ok, i, ODD), b"16-byte aligned")
    _refused(lib, "dfx_add_layernorm_f32", _swap(ok, 5, 1 << 33), b"too many rows")
    assert lib.dfx_add_layernorm_f32(0, 0, 0, 0, 0, 0, 256, 1e-5, None) == 0


def test_box_refine_entry_rejects_bad_arguments_before_any_launch():
    """delta, ref, ref_dim, out, rows, eps."""
    lib = _lib_loaded()
    ok = (ONE, ONE, 4, ONE, 300, 1e-5)
    for i, bad in ((4, -1), (2, 3), (2, 0), (2, 5)):
        _refused(lib, "dfx_box_refine_f32", _swap(ok, i, bad), b"bad dimension")
    for i in (0, 1, 3):
        _refused(lib, "dfx_box_refine_f32", _swap(ok, i, 0), b"null pointer")
    for i in (0, 3):
        _refused(lib, "dfx_box_refine_f32", _swap(ok, i, ODD), b"16-byte aligned")
    _refused(lib, "dfx_box_refine_f32", _swap(ok, 4, 1 << 39), b"too many rows")
    assert lib.dfx_box_refine_f32(0, 0, 2, 0, 0, 1e-5, None) == 0


def test_group_norm_entry_rejects_bad_arguments_before_any_launch():
    """x, gamma, beta, stats, y, N, C, HW, groups, eps, tokens_out."""
    lib = _lib_loaded()
    ok = (ONE, ONE, ONE, ONE, ONE, 2, 64, 49, 32, 1e-5, 0)
    for i, bad in ((5, -1), (6, 0), (7, -1), (8, 0), (8, -2), (8, 24), (6, 65)):          # the last two: C % groups
        _refused(lib, "dfx_group_norm_f32", _swap(ok, i, bad), b"bad dimension")
    for i in (0, 1, 2, 3, 4):
        _refused(lib, "dfx_group_norm_f32", _swap(ok, i, 0), b"null pointer")
    _refused(lib, "dfx_group_norm_f32", _swap(ok, 5, 65536), b"too large")
    _refused(lib, "dfx_group_norm_f32", _swap(ok, 7, 1 << 31), b"too large")
    _refused(lib, "dfx_group_norm_f32", _swap(_swap(_swap(ok, 5, 60000), 6, 40000), 8, 40000), b"too large")   # N * groups
    assert lib.dfx_group_norm_f32(0, 0, 0, 0, 0, 0, 64, 49, 32, 1e-5, 0, None) == 0
    assert lib.dfx_group_norm_f32(0, 0, 0, 0, 0, 2, 64, 0, 32, 1e-5, 1, None) == 0


def test_dynamic_conv_entry_rejects_bad_arguments_before_any_launch():
    """feats, params, p_stride, g1, b1, g2, b2, out, K, R, C, dd, eps."""
    lib = _lib_loaded()
    row = 2 * 256 * 64
    ok = (ONE, ONE, row, ONE, ONE, ONE, ONE, ONE, 5, 49, 256, 64, 1e-5)
    for i, bad in ((8, -1), (9, 0), (9, -7)):
        _refused(lib, "dfx_dynamic_conv_f32", _swap(ok, i, bad), b"bad dimension")
    for i, bad in ((10, 128), (11, 32), (9, 65)):
        _refused(lib, "dfx_dynamic_conv_f32", _swap(ok, i, bad), b"built for C = 256, dim_dynamic = 64, at most 64 rows")
    for i in (0, 1, 3, 4, 5, 6, 7):
        _refused(lib, "dfx_dynamic_conv_f32", _swap(ok, i, 0), b"null pointer")
    for stride in (row - 4, row + 2, 0):
        _refused(lib, "dfx_dynamic_conv_f32", _swap(ok, 2, stride), b"params rows must hold 2*C*dd floats")
    for i in (0, 1, 3, 4, 5, 6, 7):
        _refused(lib, "dfx_dynamic_conv_f32", _swap(ok, i, ODD), b"16-byte aligned")
    assert lib.dfx_dynamic_conv_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 49, 256, 64, 1e-5, None) == 0


def _lib_loaded():
    from dfx import _lib
    return _lib.load()
