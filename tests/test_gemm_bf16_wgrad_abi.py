"""CPU, no launch: the two weight-gradient entries on the one frame (csrc/wgrad_frame.h) - dfx_gemm_bf16_wgrad
(include/dfx_gemm_bf16.h) and dfx_gemm_wgrad_f32 (include/dfx_gemm.h) - are exported and bound and refuse what their headers say
they refuse before any launch, each with its own granule (8 or 4 columns) and its own bound on a range of rows;
dfx.ops.linear_bf16_backward refuses CPU tensors, non-bf16 weight copies and N or K not multiples of 8; the LINEAR_BF16_TRAIN
switch is off by default and the pair of bf16 weight copies follows its key."""
import collections
import os

import pytest
import torch
from torch import nn

ONE, TWO, ODD = 64, 128, 20     # non-null addresses: 16-byte aligned (two of them), 4-byte only
GIB2 = 1 << 31
EINVAL, ERANGE = -1, -3

# dY, ldy, X, ldx, dW, ldw, db, M, N, K, splits, workspace
OK = (ONE, 16, ONE, 24, ONE, 24, ONE, 40, 16, 24, 1, TWO)
DY, LDY, X, LDX, DW, LDW, DB, M, N, K, SPLITS, WS = range(12)

# granule: columns N and K must be multiples of; step: rows of a K-step; reach: rows beyond a range that its 2 GiB bound allows for
Entry = collections.namedtuple("Entry", "name granule step reach")
BF16 = Entry("dfx_gemm_bf16_wgrad", 8, 32, 32)
F32 = Entry("dfx_gemm_wgrad_f32", 4, 16, 0)


def _lib_loaded():
    from dfx import _lib
    return _lib.load()


def _refused(lib, e, args, cause, code):
    rc = getattr(lib, e.name)(*args, None)
    assert rc == code and cause in lib.dfx_last_error(), (e.name, args, rc, lib.dfx_last_error())


def _swap(args, *pairs):
    args = list(args)
    for i, v in pairs:
        args[i] = v
    return tuple(args)


# ---- the checks of the frame, for either entry ---------------------------------------------------------------------------
def symbol_is_exported_and_bound(e):
    from dfx import _lib
    lib = _lib_loaded()
    assert hasattr(lib, e.name) and len(_lib.SIGNATURES[e.name]) == 13
    assert getattr(lib, e.name).argtypes == _lib.SIGNATURES[e.name]
    assert lib.dfx_abi_version() == 5          # an addition: the version stays


def bad_dimensions_and_pointers_are_refused(e):
    lib = _lib_loaded()
    for i, bad in ((M, -1), (N, -8), (K, -8), (SPLITS, 0), (SPLITS, -3)):
        _refused(lib, e, _swap(OK, (i, bad)), b"bad dimension", EINVAL)
    for i in (DY, X, DW):
        _refused(lib, e, _swap(OK, (i, 0)), b"null pointer", EINVAL)
    _refused(lib, e, _swap(OK, (SPLITS, 2), (M, 100), (WS, 0)), b"needs a workspace", EINVAL)


def n_and_k_must_be_multiples_of_the_granule(e):
    lib, g = _lib_loaded(), e.granule
    cause = b"N and K must be multiples of %d" % g
    for n in (g // 2, g + g // 2, 17, 256 + g // 2):          # (bf16: 4, 12, 17, 260)
        _refused(lib, e, _swap(OK, (N, n), (LDY, 512)), cause, EINVAL)
    for k in (g // 2, g + g // 2, 17, 256 + g // 2):
        _refused(lib, e, _swap(OK, (K, k), (LDX, 512), (LDW, 512)), cause, EINVAL)


def pitches_short_or_not_multiples_of_4_are_refused(e):
    lib = _lib_loaded()
    for i, short in ((LDY, 8), (LDX, 16), (LDW, 16)):
        _refused(lib, e, _swap(OK, (i, short)), b"multiples of 4 that cover a row", EINVAL)
    for i in (LDY, LDX, LDW):
        for odd in (25, 26, 27):
            _refused(lib, e, _swap(OK, (i, odd)), b"multiples of 4 that cover a row", EINVAL)


def misalignment_is_refused(e):
    lib = _lib_loaded()
    for i in (DY, X, DW, WS):
        _refused(lib, e, _swap(OK, (i, ODD)), b"16-byte aligned", EINVAL)


def ranges_and_outputs_of_2_gib_are_refused(e):
    lib = _lib_loaded()
    rows = GIB2 // (24 * 4)                                                     # one range of X rows of 24 floats: 2 GiB
    _refused(lib, e, _swap(OK, (M, rows + 32)), b"2 GiB", ERANGE)
    _refused(lib, e, _swap(OK, (M, 4 * rows), (SPLITS, 2)), b"2 GiB", ERANGE)      # two ranges of 2 GiB each
    _refused(lib, e, _swap(OK, (M, 64), (LDY, GIB2 // 4 // 64)), b"2 GiB", ERANGE)  # the pitch of dY alone
    _refused(lib, e, _swap(OK, (LDW, GIB2 // 4 // 16)), b"2 GiB", ERANGE)          # dW
    _refused(lib, e, _swap(OK, (M, e.step * 70000), (SPLITS, 70000)), b"too many splits", ERANGE)


def the_range_bound_is_the_entrys_own(e):
    """X rows of 32 floats: 2^24 rows are exactly 2 GiB.  Two ranges of `edge` = 2^24 - reach rows each are refused, two of one
    step less pass the bound - shown without a launch by the next refusal in the entry's order, the missing workspace."""
    lib = _lib_loaded()
    rows = GIB2 // (32 * 4)
    assert rows * 32 * 4 == GIB2 and rows % e.step == 0
    edge = rows - e.reach
    _refused(lib, e, _swap(OK, (LDX, 32), (M, 2 * edge), (SPLITS, 2), (WS, 0)), b"2 GiB", ERANGE)
    _refused(lib, e, _swap(OK, (LDX, 32), (M, 2 * (edge - e.step)), (SPLITS, 2), (WS, 0)), b"needs a workspace", EINVAL)
    _refused(lib, e, _swap(OK, (LDY, 32), (M, 2 * edge), (SPLITS, 2), (WS, 0)), b"2 GiB", ERANGE)     # the wider pitch counts, dY's too
    _refused(lib, e, _swap(OK, (LDY, 32), (M, 2 * (edge - e.step)), (SPLITS, 2), (WS, 0)), b"needs a workspace", EINVAL)


def empty_products_return_ok_without_a_launch(e):
    fn = getattr(_lib_loaded(), e.name)
    assert fn(*_swap(OK, (N, 0)), None) == 0
    assert fn(*_swap(OK, (K, 0)), None) == 0
    assert fn(0, 0, 0, 0, 0, 0, 0, 5, 0, 8, 1, 0, None) == 0       # asked before the pointers and pitches


FRAME_CHECKS = [symbol_is_exported_and_bound, bad_dimensions_and_pointers_are_refused, n_and_k_must_be_multiples_of_the_granule,
                pitches_short_or_not_multiples_of_4_are_refused, misalignment_is_refused, ranges_and_outputs_of_2_gib_are_refused,
                the_range_bound_is_the_entrys_own, empty_products_return_ok_without_a_launch]


# ---- dfx_gemm_wgrad_f32: every check of the frame ------------------------------------------------------------------------
@pytest.mark.parametrize("check", FRAME_CHECKS, ids=lambda f: f.__name__)
def test_fp32_entry(check):
    check(F32)


# ---- dfx_gemm_bf16_wgrad: the same checks under the names they have had --------------------------------------------------
def test_symbol_is_exported_and_bound():
    symbol_is_exported_and_bound(BF16)


def test_bad_dimensions_and_pointers_are_refused():
    bad_dimensions_and_pointers_are_refused(BF16)


def test_n_and_k_must_be_multiples_of_8():
    n_and_k_must_be_multiples_of_the_granule(BF16)


def test_pitches_short_or_not_multiples_of_4_are_refused():
    pitches_short_or_not_multiples_of_4_are_refused(BF16)


def test_misalignment_is_refused():
    misalignment_is_refused(BF16)


def test_ranges_and_outputs_of_2_gib_are_refused():
    ranges_and_outputs_of_2_gib_are_refused(BF16)


def test_the_range_bound_reaches_one_step_further():
    the_range_bound_is_the_entrys_own(BF16)


def test_empty_products_return_ok_without_a_launch():
    empty_products_return_ok_without_a_launch(BF16)


def test_linear_bf16_backward_refuses_cpu_tensors_other_copies_and_sizes_not_multiples_of_8():
    from dfx import ops
    go, x, wt = torch.zeros(3, 8), torch.zeros(3, 16), torch.zeros(16, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.linear_bf16_backward(go, x, wt)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.linear_bf16_backward(go, x, wt, need_x=False)
    for other in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(RuntimeError, match="must be bfloat16"):
            ops.linear_bf16_backward(go, x, wt.to(other))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.linear_bf16_backward(torch.zeros(3, 12), x, torch.zeros(16, 12, dtype=torch.bfloat16))        # N = 12
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.linear_bf16_backward(go, torch.zeros(3, 20), torch.zeros(20, 8, dtype=torch.bfloat16))        # K = 20
    with pytest.raises(RuntimeError, match="must be float32"):
        ops.linear_bf16_backward(go.double(), x, wt)
    with pytest.raises(RuntimeError, match=r"grad_out \[M,N\]"):
        ops.linear_bf16_backward(go, torch.zeros(3, 24), wt)
    with pytest.raises(RuntimeError, match="same rows"):
        ops.linear_bf16_backward(go, torch.zeros(4, 16), wt)


def test_split_rule_counts_whole_32_row_steps_and_leaves_no_range_empty():
    from dfx import ops
    assert ops._wgrad_bf16_ranges(1000, 7) == (160, 7) and ops._wgrad_bf16_ranges(100, 7) == (32, 4)
    assert ops._wgrad_bf16_splits(0, 256, 256) == 1 and ops._wgrad_bf16_splits(300, 256, 1024) == 1
    for rows in (9600, 4 * 4200, 32 * 4200):
        for n, k in ((1024, 256), (256, 1024), (256, 256), (64, 256)):
            s = ops._wgrad_bf16_splits(rows, n, k)
            kper, ranges = ops._wgrad_bf16_ranges(rows, s)
            assert ranges == s and (s - 1) * kper < rows and (s == 1 or kper >= 32 * ops._WGRAD_MIN_STEPS)
            assert s * ops._wgrad_tiles(n, k)[0] <= ops._WGRAD_BF16_SLOTS and s <= ops._WGRAD_BF16_MAX_RANGES
    assert ops._wgrad_bf16_splits(32 * 4200, 1024, 256) == 32 and ops._wgrad_bf16_splits(32 * 4200, 256, 256) == 64
    assert ops._wgrad_bf16_splits(9600, 256, 1024) == 18 and ops._wgrad_bf16_splits(4 * 4200, 64, 256) == 31


def test_the_switch_is_off_by_default_and_the_weight_copies_follow_their_key():
    from models import fused
    assert fused.LINEAR_BF16_TRAIN == (os.environ.get("DFX_LINEAR_BF16_TRAIN", "0") == "1")
    if "DFX_LINEAR_BF16_TRAIN" not in os.environ:
        assert fused.LINEAR_BF16_TRAIN is False
    lin = nn.Linear(16, 8)
    w, wt = fused.bf16_weight_pair(lin)
    want = lin.weight.detach().to(torch.bfloat16)
    assert w.dtype == wt.dtype == torch.bfloat16 and w.shape == (8, 16) and wt.shape == (16, 8)
    assert w.is_contiguous() and wt.is_contiguous() and torch.equal(w, want) and torch.equal(wt, want.t())
    again = fused.bf16_weight_pair(lin)
    assert again[0] is w and again[1] is wt
    with torch.no_grad():
        lin.weight.add_(1.0)
    w2, wt2 = fused.bf16_weight_pair(lin)
    want = lin.weight.detach().to(torch.bfloat16)
    assert w2 is not w and torch.equal(w2, want) and torch.equal(wt2, want.t())
    lin.weight.data = torch.ones(8, 16)
    w3, wt3 = fused.bf16_weight_pair(lin)
    assert torch.equal(w3, torch.ones(8, 16, dtype=torch.bfloat16)) and torch.equal(wt3, torch.ones(16, 8, dtype=torch.bfloat16))
    assert "_weight_bf16" not in lin.__dict__                   # the no_grad route's name stays its own
    assert "_weight_bf16_pair" in fused.DERIVED_ATTRIBUTES_BF16 and "_weight_bf16_pair" not in fused.DERIVED_ATTRIBUTES
    from util import memo
    memo.clear()                                      # (the memo is the process's: earlier tests may have left entries)
    assert fused.drop_derived(nn.Sequential(lin)) == 1 and "_weight_bf16_pair" not in lin.__dict__


def test_the_switch_off_leaves_a_cpu_linear_as_it_was(monkeypatch):
    from models import fused
    lin = fused.Linear(16, 8)
    x = torch.randn(3, 16, generator=torch.Generator().manual_seed(0), requires_grad=True)
    want = nn.functional.linear(x, lin.weight, lin.bias)
    for on in (False, True):                                    # CPU tensors keep nn.Linear whatever the switch says
        monkeypatch.setattr(fused, "LINEAR_BF16_TRAIN", on)
        assert torch.equal(lin(x), want) and "_weight_bf16_pair" not in lin.__dict__
