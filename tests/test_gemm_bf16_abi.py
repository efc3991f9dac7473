"""CPU, no launch: dfx_gemm_bf16 (include/dfx_gemm_bf16.h) is exported and bound, refuses what its header says it refuses
before any launch, and dfx.ops.linear_bf16 refuses CPU tensors, non-bf16 weights and K % 8 != 0."""
import pytest
import torch

ONE, ODD, EVEN2, ODD1 = 64, 20, 18, 17     # non-null addresses: 16-byte aligned, 4-byte only, 2-byte only, odd
GIB2 = 1 << 31


def _lib_loaded():
    from dfx import _lib
    return _lib.load()


def _refused(lib, args, cause, code=None):
    rc = lib.dfx_gemm_bf16(*args, None)
    assert rc != 0 and cause in lib.dfx_last_error(), (args, rc, lib.dfx_last_error())
    if code is not None:
        assert rc == code, (args, rc)


def _swap(args, *pairs):
    args = list(args)
    for i, v in pairs:
        args[i] = v
    return tuple(args)


# A, a_dtype, lda, W, ldw, bias, R, ldr, C, c_dtype, ldc, M, N, K, act
OK = (ONE, 0, 16, ONE, 16, ONE, ONE, 8, ONE, 0, 8, 5, 8, 16, 1)
A, ADT, LDA, W, LDW, BIAS, R, LDR, C, CDT, LDC, M, N, K, ACT = range(15)
EINVAL, ERANGE = -1, -3


def test_symbol_is_exported_and_bound():
    from dfx import _lib
    lib = _lib_loaded()
    assert hasattr(lib, "dfx_gemm_bf16") and len(_lib.SIGNATURES["dfx_gemm_bf16"]) == 16
    assert lib.dfx_gemm_bf16.argtypes == _lib.SIGNATURES["dfx_gemm_bf16"]
    assert lib.dfx_abi_version() == 5          # an addition: the version stays


def test_bad_dimensions_pointers_and_codes_are_refused():
    lib = _lib_loaded()
    for i, bad in ((M, -1), (N, -2), (K, 0), (K, -8)):
        _refused(lib, _swap(OK, (i, bad)), b"bad dimension", EINVAL)
    for i in (A, W, C):
        _refused(lib, _swap(OK, (i, 0)), b"null pointer", EINVAL)
    for k in (4, 12, 17, 260):
        _refused(lib, _swap(OK, (K, k), (LDA, 512), (LDW, 512)), b"K must be a multiple of 8", EINVAL)
    for act in (-1, 3, 7):
        _refused(lib, _swap(OK, (ACT, act)), b"activation", EINVAL)
    for i in (ADT, CDT):
        for code in (-1, 2, 5):
            _refused(lib, _swap(OK, (i, code)), b"unknown dtype code", EINVAL)


def test_short_pitches_are_refused():
    lib = _lib_loaded()
    _refused(lib, _swap(OK, (LDA, 8)), b"row pitch", EINVAL)
    _refused(lib, _swap(OK, (LDW, 8)), b"row pitch", EINVAL)
    _refused(lib, _swap(OK, (LDR, 4)), b"row pitch", EINVAL)
    _refused(lib, _swap(OK, (LDC, 7)), b"row pitch", EINVAL)


def test_misalignment_is_refused():
    lib = _lib_loaded()
    for i in (A, W):
        _refused(lib, _swap(OK, (i, ODD)), b"16-byte aligned", EINVAL)
    _refused(lib, _swap(OK, (LDA, 18)), b"16-byte aligned", EINVAL)                  # fp32 rows of 72 bytes
    _refused(lib, _swap(OK, (ADT, 1), (LDA, 20)), b"16-byte aligned", EINVAL)        # bf16 rows of 40 bytes
    _refused(lib, _swap(OK, (LDW, 20)), b"16-byte aligned", EINVAL)
    _refused(lib, _swap(OK, (C, EVEN2)), b"element size", EINVAL)                    # fp32 C on a 2-byte boundary
    _refused(lib, _swap(OK, (C, ODD1), (CDT, 1)), b"element size", EINVAL)           # bf16 C on an odd address
    _refused(lib, _swap(OK, (BIAS, EVEN2)), b"element size", EINVAL)
    _refused(lib, _swap(OK, (R, EVEN2)), b"element size", EINVAL)


def test_operands_of_2_gib_are_refused():
    lib = _lib_loaded()
    rows = GIB2 // (16 * 4)                                                          # fp32 A rows of 16: exactly 2 GiB
    _refused(lib, _swap(OK, (M, rows), (LDC, 8)), b"2 GiB", ERANGE)
    _refused(lib, _swap(OK, (ADT, 1), (M, 2 * rows)), b"2 GiB", ERANGE)              # bf16 A
    _refused(lib, _swap(OK, (N, GIB2 // (16 * 2)), (LDC, GIB2), (LDR, GIB2)), b"2 GiB", ERANGE)      # W
    _refused(lib, _swap(OK, (LDC, GIB2 // 4 // 5 + 1)), b"2 GiB", ERANGE)            # C, 5 rows
    _refused(lib, _swap(OK, (LDR, GIB2 // 4 // 5 + 1)), b"2 GiB", ERANGE)            # R
    _refused(lib, _swap(OK, (CDT, 1), (LDC, GIB2 // 2 // 5 + 1)), b"2 GiB", ERANGE)  # bf16 C


def test_empty_products_return_ok_without_a_launch():
    lib = _lib_loaded()
    assert lib.dfx_gemm_bf16(*_swap(OK, (M, 0)), None) == 0
    assert lib.dfx_gemm_bf16(*_swap(OK, (N, 0)), None) == 0
    assert lib.dfx_gemm_bf16(0, 0, 16, 0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, None) == 0       # asked before the pointers


def test_linear_bf16_refuses_cpu_tensors_other_weights_and_k_not_a_multiple_of_8():
    from dfx import ops
    x, w = torch.zeros(3, 16), torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.linear_bf16(x, w)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.linear_bf16(x.to(torch.bfloat16), w, out_dtype=torch.bfloat16)
    for other in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(RuntimeError, match="weight must be bfloat16"):
            ops.linear_bf16(x, w.to(other))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.linear_bf16(torch.zeros(3, 12), torch.zeros(4, 12, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.linear_bf16(x, torch.zeros(4, 24, dtype=torch.bfloat16))                # weight [N, K'] with K' != K
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.linear_bf16(x.double(), w)
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.linear_bf16(x, w, out_dtype=torch.float16)


def test_the_switch_is_off_by_default_and_the_weight_copy_follows_its_key():
    import os
    from torch import nn
    from models import fused
    assert fused.LINEAR_BF16 == (os.environ.get("DFX_LINEAR_BF16", "0") == "1")
    lin = nn.Linear(16, 4)
    w = fused.bf16_weight(lin)
    assert w.dtype == torch.bfloat16 and torch.equal(w, lin.weight.detach().to(torch.bfloat16)) and fused.bf16_weight(lin) is w
    with torch.no_grad():
        lin.weight.add_(1.0)
    w2 = fused.bf16_weight(lin)
    assert w2 is not w and torch.equal(w2, lin.weight.detach().to(torch.bfloat16))
    lin.weight.data = torch.ones(4, 16)
    assert torch.equal(fused.bf16_weight(lin), torch.ones(4, 16, dtype=torch.bfloat16))
    from util import memo
    memo.clear()                                      # (the memo is the process's: earlier tests may have left entries)
    assert fused.drop_derived(nn.Sequential(lin)) == 1 and "_weight_bf16" not in lin.__dict__
    assert not fused.linear_bf16_usable(torch.zeros(3, 16), lin)                     # CPU tensors never take the route
