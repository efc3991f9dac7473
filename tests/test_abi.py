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


_I, _L, _F, _D, _P = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
# one entry point of every shape the header parser has to read, its types stated by hand from the header
HAND_STATED = {
    # A, A2, lda, strideA, B, ldb, strideB, b_is_kn, bias, bias_per_row, R, ldr, strideR, row_mask, strideMask, C, ldc, strideC,
    # M, N, K, batch, relu, c_block, c_block_stride, a_block_stride, stream
    "dfx_gemm_f32": (_I, [_P, _P, _L, _L, _P, _L, _L, _I, _P, _I, _P, _L, _L, _P, _L, _P, _L, _L,
                          _I, _I, _I, _I, _I, _I, _L, _L, _P]),
    "dfx_tuning_reload": (_I, []),                                                                    # (void)
    # x, gamma, beta, running_mean, running_var, y, stats, workspace, N, C, HW, eps, momentum, act, stream: doubles
    "dfx_batch_norm_train_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _D, _D, _I, _P]),
    # input, rois, N, C, H, W, K, ph, pw, spatial_scale, sampling_ratio, aligned, out, stream: a float in the middle
    "dfx_roi_align_nhwc_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P]),
    # value, ref, ref_dim, off, logits, layout (a struct pointer), N, H, W, Lq, out, stream
    "dfx_msda_fused_level_forward_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "dfx_last_error": (ctypes.c_char_p, []),                                                          # const char *(void)
}


@pytest.mark.parametrize("name", sorted(HAND_STATED))
def test_binding_reads_the_hand_stated_types_from_the_header(name):
    from dfx import _lib
    restype, argtypes = HAND_STATED[name]
    assert _lib.SIGNATURES[name] == argtypes
    assert getattr(_lib.load(), name).restype is restype


def test_loaded_library_carries_every_parsed_signature():
    from dfx import _lib
    lib = _lib.load()
    assert set(_lib.SIGNATURES) == set(declared_symbols())
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes, name
        assert fn.restype is (ctypes.c_char_p if name == "dfx_last_error" else ctypes.c_int), name


def test_parser_refuses_what_it_does_not_know_by_name():
    """A scalar type outside int / long / float / double, or a macro value that is no integer or product of integers, raises and
    names the function and parameter, or the macro: nothing is guessed, nothing is silently left out."""
    from dfx import _lib
    for text, names in (("int dfx_x(short a, void *stream);", ("dfx_x", "short a")),
                        ("int dfx_y(int n, unsigned int flags);", ("dfx_y", "unsigned int flags")),
                        ("int dfx_z(int);", ("dfx_z", "int")),
                        ("#define DFX_BAD (1 << 4)\n", ("DFX_BAD",)),
                        ("#define DFX_SUM (2 + 3)\n", ("DFX_SUM",)),
                        ("#define DFX_ALIAS DFX_OTHER\n", ("DFX_ALIAS",))):
        with pytest.raises(RuntimeError) as err:
            _lib.parse_header(text)
        for name in names:
            assert name in str(err.value), (text, str(err.value))
    prototypes, constants = _lib.parse_header(
        "/* int dfx_commented(short a); */\n#define DFX_GUARD_H\n#define DFX_FN(x) ((x) + 1)\n#define DFX_NEG (-7) /* why */\n"
        "#define DFX_PROD (3 * 5)\n#define DFX_PLAIN 9\nconst char *dfx_s(void);\nint dfx_f(const long *p, double d,\n  long n);\n")
    assert constants == {"DFX_NEG": -7, "DFX_PROD": 15, "DFX_PLAIN": 9}
    assert prototypes == {"dfx_s": (ctypes.c_char_p, []), "dfx_f": (ctypes.c_int, [_P, _D, _L])}


def test_constants_hold_every_integer_define_of_the_headers():
    from dfx import _lib
    assert _lib.CONSTANTS["DFX_DYNCONV_BWD_WS_FLOATS"] == 163840
    assert _lib.CONSTANTS["DFX_ENONFINITE"] == -4 == _lib.ENONFINITE
    hand_stated = {
        "DFX_OK": 0, "DFX_EINVAL": -1, "DFX_ELAUNCH": -2, "DFX_ERANGE": -3, "DFX_ENONFINITE": -4,
        "DFX_ACT_NONE": 0, "DFX_ACT_RELU": 1, "DFX_ACT_GELU": 2, "DFX_DT_F32": 0, "DFX_DT_BF16": 1,
        "DFX_ADDLN_BWD_ROWS_PER_BLOCK": 16, "DFX_ADDLN_BWD_MAX_GRID": 1024, "DFX_GN_BWD_CHUNKS": 16,
        "DFX_BN_CHUNK_PIXELS": 8192, "DFX_BN_BWD_MAX_GROUPS": 128, "DFX_OPTIM_CHUNK": 8192,
        "DFX_DYNCONV_BWD_WS_FLOATS": 163840}
    assert {k: _lib.CONSTANTS.get(k) for k in hand_stated} == hand_stated
    # no value-carrying object-like macro of the headers is missing: names found here without the binding's parser
    valued = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        valued += re.findall(r"^\s*#\s*define\s+(DFX_\w+)[ \t]+[-(\d]", open(h).read(), flags=re.M)
    assert len(valued) >= len(hand_stated) and sorted(valued) == sorted(_lib.CONSTANTS)


def test_ops_constants_are_the_headers():
    from dfx import _lib, ops
    c = _lib.CONSTANTS
    assert ops.DYNCONV_BWD_WS_FLOATS == c["DFX_DYNCONV_BWD_WS_FLOATS"] and ops.GN_BWD_CHUNKS == c["DFX_GN_BWD_CHUNKS"]
    assert (ops.ADDLN_BWD_ROWS_PER_BLOCK, ops.ADDLN_BWD_MAX_GRID) == (c["DFX_ADDLN_BWD_ROWS_PER_BLOCK"], c["DFX_ADDLN_BWD_MAX_GRID"])
    assert ops.BN_CHUNK_PIXELS == c["DFX_BN_CHUNK_PIXELS"]
    assert ops.ACT == {None: 0, "none": 0, "relu": 1, "gelu": 2}


def test_gemm_helper_puts_every_argument_where_the_header_names_it(monkeypatch):
    """ops._gemm_f32 takes the header's parameter names; each value must reach the position the prototype gives that name
    (no launch: ops._call is replaced by a recorder)."""
    import inspect
    from dfx import ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_gemm.h")).read(), flags=re.S)
    params = re.search(r"int dfx_gemm_f32\(([^)]*)\)", text).group(1).split(",")
    names = [p.split()[-1].lstrip("*") for p in params][:-1]          # the stream is _call's to add
    assert len(names) == 26 and names[0] == "A" and names[-1] == "a_block_stride"
    helper = list(inspect.signature(ops._gemm_f32).parameters)
    assert helper[:2] == ["what", "dev"] and sorted(helper[2:]) == sorted(names)
    calls = []
    monkeypatch.setattr(ops, "_call", lambda what, name, dev, *args: calls.append((what, name, dev, args)))
    ops._gemm_f32("w", "d", **{n: 100 + i for i, n in enumerate(names)})
    assert calls == [("w", "dfx_gemm_f32", "d", tuple(range(100, 126)))]
    ops._gemm_f32("w", "d", 1, 2, 3, 4, 5, 6, 7, 8, 9)                # A, B, C, M, N, K, lda, ldb, ldc; the rest absent
    given = dict(A=1, B=2, C=3, M=4, N=5, K=6, lda=7, ldb=8, ldc=9, batch=1)
    assert calls[1][3] == tuple(given.get(n, 0) for n in names)


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
