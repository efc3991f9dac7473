"""GPU: the bf16 weight-gradient kernel (csrc/gemm_bf16_wgrad.hip on csrc/wgrad_frame.h, dfx_gemm_bf16_wgrad) and
dfx.ops.linear_bf16_backward - exact cases bit for bit at every element, the rounding of both operands, random operands against
fp64 with a worked-out bound on every element, padding, run-to-run bits, the need_* flags and row pitches.  What tests the
frame and not the operand path - exact integers, row pitches, tails - runs on the fp32 entry too (csrc/gemm_wgrad.hip,
dfx_gemm_wgrad_f32, dfx.ops.linear_backward).

Bounds (u = 2^-8, the unit roundoff of bf16; products of bf16 operands are exact in fp32):
  dW vs fp64 of the ROUNDED operands:   |dW - ref| <= M 2^-23 S + 2^-23 |ref|,  S = |bf16(dY)|^T |bf16(X)|
      (the fp32 summation bound for any order over at most 2M additions: the steps of a range, then the ranges)
  dW vs fp64 of the UNROUNDED operands: the above + (2u + u^2) |dY|^T |X|
  db (from the unrounded dY):           |db - ref| <= M 2^-23 sum_m |dY|
  grad_x = bf16(dY) @ W:                |gx - ref| <= N 2^-23 S' + 2^-23 |ref|,  S' = |bf16(dY)| |W|   (tests/test_gemm_bf16_gpu.py's
      bound with K -> N)
  fp32 entry, dW vs fp64 of the operands: |dW - ref| <= M 2^-23 S + 2^-23 |ref|,  S = |dY|^T |X|   (no rounding of the operands)
Every case prints its worst ratio to the bound (pytest -s shows them)."""
import collections
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N, K, splits): a ragged last step and a ragged last range, one octet, partial and crossing tiles, both FFN orientations,
# the 64-row tile (N <= 64)
SHAPES = [(1, 8, 8, 1), (15, 24, 40, 1), (17, 8, 264, 1), (33, 136, 264, 1), (100, 256, 256, 2), (1000, 1024, 256, 7),
          (1000, 256, 1024, 7), (1000, 64, 72, 3)]
# the fp32 entry takes every multiple of 4: one quad, a quad past a column tile, one quad past a 128 tile in both directions, the
# 64-row tile with a ragged last range
SHAPES_F32 = SHAPES + [(1, 4, 4, 1), (17, 12, 260, 1), (33, 132, 260, 1), (1000, 60, 68, 3)]
U = 2.0 ** -8
EPS = 2.0 ** -23
ids = lambda s: "x".join(map(str, s))      # noqa: E731


def _gen(shape, salt):
    M, N, K, _ = shape
    return torch.Generator(device="cuda").manual_seed(1000003 * M + 1009 * N + K + salt)


# an entry of the frame: its symbol, and the (dW, db) half of its backward function on contiguous operands
Entry = collections.namedtuple("Entry", "name wgrad")


def _wgrad(go, x, splits, need_b=True):
    from dfx import ops
    N = go.shape[1]
    wt = torch.zeros(x.shape[1], N, dtype=torch.bfloat16, device="cuda")
    _, gw, gb = ops.linear_bf16_backward(go, x, wt, need_x=False, need_w=True, need_b=need_b, splits=splits)
    return gw, gb


def _wgrad_f32(go, x, splits, need_b=True):
    from dfx import ops
    w = torch.zeros(go.shape[1], x.shape[1], device="cuda")
    _, gw, gb = ops.linear_backward(go, x, w, need_x=False, need_w=True, need_b=need_b, splits=splits)
    return gw, gb


BF16 = Entry("dfx_gemm_bf16_wgrad", _wgrad)
F32 = Entry("dfx_gemm_wgrad_f32", _wgrad_f32)


def _raw(buf_y, ldy, buf_x, ldx, M, N, K, splits, ldw=None, with_db=True, entry=BF16):
    """the entry point itself, on operands with row pitches of their own"""
    from dfx import ops
    ldw = K if ldw is None else ldw
    dW = torch.full((N, ldw), float("nan"), device="cuda")
    db = torch.full((N,), float("nan"), device="cuda") if with_db else None
    ws = torch.full((splits * (N * K + N),), float("nan"), device="cuda") if splits > 1 else None
    ops._call("test", entry.name, buf_y.device, buf_y.data_ptr(), ldy, buf_x.data_ptr(), ldx, dW.data_ptr(), ldw,
              ops._ptr(db), M, N, K, splits, ops._ptr(ws))
    return dW, db


def _worst(err, bound, what):
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"  {what}: worst |got - ref| / bound = {ratio:.4f}")
    return ratio


# ---- 1. exact ----------------------------------------------------------------------------------------------------------
def _integer_operands_are_bit_equal(entry, shape):
    M, N, K, splits = shape
    g = _gen(shape, 1)
    go = torch.randint(-8, 9, (M, N), generator=g, device="cuda").float()
    x = torch.randint(-8, 9, (M, K), generator=g, device="cuda").float()
    gw, gb = entry.wgrad(go, x, splits)
    ref_w, ref_b = go.double().t() @ x.double(), go.double().sum(0)
    assert gw.shape == (N, K) and gb.shape == (N,) and gw.dtype == gb.dtype == torch.float32
    bad = (gw.double() != ref_w).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), len(bad))
    assert torch.equal(gb.double(), ref_b)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_integer_operands_are_bit_equal_at_every_element(shape):
    """integers in [-8, 8] are bf16 numbers and every partial sum stays below 2^24: fp32 is exact in any order"""
    _integer_operands_are_bit_equal(BF16, shape)


@pytest.mark.parametrize("shape", SHAPES_F32, ids=ids)
def test_fp32_integer_operands_are_bit_equal_at_every_element(shape):
    """products of at most 64 over at most 1000 rows: every partial sum stays below 64 000 < 2^24, fp32 is exact in any order"""
    _integer_operands_are_bit_equal(F32, shape)


def test_no_rows_write_zeros():
    gw, gb = _wgrad(torch.zeros(0, 24, device="cuda"), torch.zeros(0, 40, device="cuda"), 1)
    assert gw.shape == (24, 40) and not gw.any() and gb.shape == (24,) and not gb.any()


# ---- 2. rounding -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ties(rows, cols):
    """ties and near-ties of bf16 (1 + 2^-8 lies half way between 1 and 1 + 2^-7, 1 + 3 2^-8 between 1 + 2^-7 and 1 + 2^-6), both
    signs, scaled by powers of two over 12 decades (2^-20 .. 2^20)"""
    base = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,
                         1 + 3 * 2.0 ** -8 + 2.0 ** -22, 1 + 3 * 2.0 ** -8 - 2.0 ** -22, 1 + 5 * 2.0 ** -8, 1 + 7 * 2.0 ** -8,
                         1.0, 1 + 2.0 ** -7, 2 - 2.0 ** -8, 2 - 2.0 ** -9], dtype=torch.float64)
    i = torch.arange(rows * cols)
    v = base[i % len(base)] * torch.pow(2.0, ((i * 7) % 41 - 20).double()) * (1 - 2 * ((i // 3) % 2)).double()
    return v.float().reshape(rows, cols).cuda()


@pytest.mark.parametrize("M,N,K,splits", [(50, 24, 64, 1), (64, 136, 64, 2), (200, 72, 264, 3)])
def test_dY_is_rounded_to_nearest_even(M, N, K, splits):
    """X is one-hot 1.0 per row (k = m; M <= K), so dW[n][k] is bf16(dY[k][n]) alone - no sum, no second rounding"""
    go = _ties(M, N)
    x = torch.zeros(M, K, device="cuda")
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    gw, gb = _wgrad(go, x, splits)
    want = torch.zeros(N, K, device="cuda")
    want[:, :M] = go.to(torch.bfloat16).float().t()
    assert (want[:, :M] != go.t()).any()                       # (the case does round)
    assert torch.equal(gw, want)
    ref_b = go.double().sum(0)
    assert _worst((gb.double() - ref_b).abs(), M * EPS * go.double().abs().sum(0), "db of the unrounded dY") <= 1


@pytest.mark.parametrize("M,N,K,splits", [(24, 24, 64, 1), (64, 64, 136, 2), (200, 264, 72, 3)])
def test_X_is_rounded_to_nearest_even(M, N, K, splits):
    """the roles swapped: dY is one-hot (n = m; M <= N), dW[n][k] is bf16(X[n][k])"""
    x = _ties(M, K)
    go = torch.zeros(M, N, device="cuda")
    go[torch.arange(M), torch.arange(M) % N] = 1.0
    gw, gb = _wgrad(go, x, splits)
    want = torch.zeros(N, K, device="cuda")
    want[:M] = x.to(torch.bfloat16).float()
    assert torch.equal(gw, want)
    assert torch.equal(gb, go.sum(0))


# ---- 3. random operands ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _randoms(shape):
    """(dY, X, W bf16 [N,K]) and the fp64 references, computed once per shape and left unchanged"""
    M, N, K, _ = shape
    g = _gen(shape, 2)
    go, x = torch.randn(M, N, generator=g, device="cuda"), torch.randn(M, K, generator=g, device="cuda")
    w = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(torch.bfloat16)
    gr, xr = go.to(torch.bfloat16).double(), x.to(torch.bfloat16).double()
    ref = dict(w_rounded=gr.t() @ xr, S=gr.abs().t() @ xr.abs(), w_exact=go.double().t() @ x.double(),
               S_exact=go.double().abs().t() @ x.double().abs(), b=go.double().sum(0), b_abs=go.double().abs().sum(0),
               x=gr @ w.double(), Sx=gr.abs() @ w.double().abs())
    return go, x, w, ref


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_random_operands_meet_the_bounds_at_every_element(shape):
    from dfx import ops
    M, N, K, splits = shape
    go, x, w, ref = _randoms(shape)
    gx, gw, gb = ops.linear_bf16_backward(go, x, w.t().contiguous(), splits=splits)
    assert gx.shape == x.shape and gx.dtype == torch.float32
    bound = M * EPS * ref["S"] + EPS * ref["w_rounded"].abs()
    r1 = _worst((gw.double() - ref["w_rounded"]).abs(), bound, f"{ids(shape)} dW vs fp64 of the rounded operands")
    r2 = _worst((gw.double() - ref["w_exact"]).abs(), bound + (2 * U + U * U) * ref["S_exact"], f"{ids(shape)} dW vs fp64 of the unrounded operands")
    r3 = _worst((gb.double() - ref["b"]).abs(), M * EPS * ref["b_abs"], f"{ids(shape)} db")
    r4 = _worst((gx.double() - ref["x"]).abs(), N * EPS * ref["Sx"] + EPS * ref["x"].abs(), f"{ids(shape)} grad_x")
    assert max(r1, r2, r3, r4) <= 1, (r1, r2, r3, r4)


# ---- 4. padding --------------------------------------------------------------------------------------------------------
def _tail_rows_and_columns_read_as_zeros(entry, rounded):
    """``rounded``: what the entry makes of an operand before the products (bf16: the rounding; fp32: nothing)"""
    M, N, K, ldy, ldx = 33, 64, 40, 72, 52
    g = torch.Generator(device="cuda").manual_seed(33)
    by = (torch.rand(M + 40, ldy, generator=g, device="cuda") + 0.5) * 1024
    bx = (torch.rand(M + 40, ldx, generator=g, device="cuda") + 0.5) * 1024
    go, x = by[:M, :N], bx[:M, :K]
    gw, gb = _raw(by, ldy, bx, ldx, M, N, K, 1, entry=entry)
    gr, xr = rounded(go).double(), rounded(x).double()
    ref = gr.t() @ xr
    assert _worst((gw.double() - ref).abs(), M * EPS * (gr.abs().t() @ xr.abs()) + EPS * ref.abs(), f"{entry.name} padding dW") <= 1
    assert _worst((gb.double() - go.double().sum(0)).abs(), M * EPS * go.double().abs().sum(0), f"{entry.name} padding db") <= 1


def test_tail_rows_and_columns_are_exactly_zero():
    """M = 33, N = 64, K = 40, operands of order 1024 inside larger buffers of the same order: rows beyond M, the columns between
    N / K and the pitch, and the padded part of the tile may only ever be read as zeros - one stray product is ~10^6 against a
    bound of ~10^2"""
    _tail_rows_and_columns_read_as_zeros(BF16, lambda t: t.to(torch.bfloat16))


def test_fp32_tail_rows_and_columns_are_exactly_zero():
    """the same buffers through the fp32 entry, against fp64 of the unrounded operands"""
    _tail_rows_and_columns_read_as_zeros(F32, lambda t: t)


# ---- 5. the same bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 7])
def test_two_calls_give_the_same_bits(splits):
    """No atomics, the ranges are added in ascending order; the outputs and the workspace are allocated with ``empty``."""
    go, x, _, _ = _randoms((1000, 256, 256, splits))
    a = _wgrad(go, x, splits)
    junk = torch.full((splits * (256 * 256 + 256) + 1000 * 256,), float("nan"), device="cuda")     # what the next ``empty`` may hand out
    del junk
    b = _wgrad(go, x, splits)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and torch.isfinite(v).all()


def test_unrequested_gradients_are_none_and_the_others_keep_their_bits():
    from dfx import ops
    shape = (100, 256, 256, 2)
    go, x, w, _ = _randoms(shape)
    wt = w.t().contiguous()
    gx, gw, gb = ops.linear_bf16_backward(go, x, wt, splits=2)
    for need in [(True, False, False), (False, True, False), (False, True, True), (False, False, True), (True, True, False),
                 (False, False, False)]:
        got = ops.linear_bf16_backward(go, x, wt, need_x=need[0], need_w=need[1], need_b=need[2], splits=2)
        assert [t is not None for t in got] == list(need)
        if need[0]:
            assert torch.equal(got[0], gx)
        if need[1]:
            assert torch.equal(got[1], gw)
        if need[2] and need[1]:
            assert torch.equal(got[2], gb)
        if need[2] and not need[1]:
            assert torch.equal(got[2], go.sum(0))


PITCHED = [(33, 136, 264, 1), (100, 256, 256, 2), (1000, 64, 72, 3)]


def _row_pitches_give_the_bits_of_the_packed_call(entry, shape):
    M, N, K, splits = shape
    go, x, _, _ = _randoms(shape)
    gw, gb = entry.wgrad(go, x, splits)
    ldy, ldx, ldw = N + 12, K + 4, K + 8
    by = torch.full((M, ldy), 1e6, device="cuda")
    bx = torch.full((M, ldx), -1e6, device="cuda")
    by[:, :N], bx[:, :K] = go, x
    pw, pb = _raw(by, ldy, bx, ldx, M, N, K, splits, ldw=ldw, entry=entry)
    assert torch.equal(pw[:, :K], gw) and torch.equal(pb, gb)
    assert torch.isnan(pw[:, K:]).all()                        # nothing outside [N, K] of dW is written
    nw, nb = _raw(by, ldy, bx, ldx, M, N, K, splits, with_db=False, entry=entry)
    assert nb is None and torch.equal(nw, gw)


@pytest.mark.parametrize("shape", PITCHED, ids=ids)
def test_row_pitches_give_the_bits_of_the_packed_call(shape):
    _row_pitches_give_the_bits_of_the_packed_call(BF16, shape)


@pytest.mark.parametrize("shape", PITCHED + [(33, 132, 260, 1)], ids=ids)
def test_fp32_row_pitches_give_the_bits_of_the_packed_call(shape):
    _row_pitches_give_the_bits_of_the_packed_call(F32, shape)
