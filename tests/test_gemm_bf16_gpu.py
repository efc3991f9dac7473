"""GPU: the bf16 MFMA GEMM (csrc/gemm_bf16.hip, dfx.ops.linear_bf16) - exact cases bit for bit, the rounding of an fp32 A,
random operands against fp64 of the rounded operands with a worked-out bound on every element, what the input rounding
costs, run-to-run bits, row pitches, canaries and row ranges.

Bounds (u = 2^-8, the unit roundoff of bf16; products of bf16 operands are exact in fp32):
  fp32 C:  |got - ref| <= E,  E = K 2^-23 S + 2^-23 |ref|,  S = |bf16(x)| @ |W|^T  (each of the K additions errs by at most 2^-23
           relative, even if the matrix pipe truncates; the last term is the epilogue's rounding)
  bf16 C:  |got - ref| <= E + 2^-8 (|ref| + E)
  GELU:    1.13 E + 4e-6 max(1, |pre|) on the pre-activation bound (1.13 bounds |gelu'|; 4e-6 is the allowance
           tests/test_gemm_gpu.py gives the same activate())
Every case prints its worst ratio to the bound (pytest -s shows them; profiles/r21_ffn_bf16.txt keeps a copy)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the issue's shapes, and three at which the launcher takes the 128 x 128 tile (>= 512 such tiles): tails in M, N and K, odd N
SHAPES = [(1, 1, 8), (5, 4, 8), (33, 3, 16), (129, 300, 264), (64, 128, 2048), (257, 1024, 256), (300, 256, 1024),
          (4200, 256, 256), (8200, 1024, 64), (5509, 1576, 40), (5509, 1573, 40)]
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -8


def _id(v):
    return {torch.float32: "f32", torch.bfloat16: "bf16"}.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


shapes_and_dtypes = lambda f: pytest.mark.parametrize("shape", SHAPES, ids=_id)(                      # noqa: E731
    pytest.mark.parametrize("a_dtype", DTYPES, ids=lambda d: "A" + _id(d))(
        pytest.mark.parametrize("c_dtype", DTYPES, ids=lambda d: "C" + _id(d))(f)))


def _gen(shape, salt):
    M, N, K = shape
    return torch.Generator(device="cuda").manual_seed(1000003 * M + 1009 * N + K + salt)


@functools.lru_cache(maxsize=None)
def _integers(shape):
    """integer-valued operands in [-8, 8]: every partial sum stays below 2^24, so fp32 is exact in any order"""
    M, N, K = shape
    g = _gen(shape, 1)
    r = lambda *s: torch.randint(-8, 9, s, generator=g, device="cuda").float()      # noqa: E731
    return r(M, K), r(N, K), r(N), r(M, N)


@functools.lru_cache(maxsize=None)
def _randoms(shape):
    M, N, K = shape
    g = _gen(shape, 2)
    r = lambda *s: torch.randn(s, generator=g, device="cuda")      # noqa: E731
    return r(M, K), r(N, K) / K ** 0.5, r(N), r(M, N)


@functools.lru_cache(maxsize=None)
def _products(shape, a_dtype):
    """(x as the kernel gets it, W, fp64 product of the rounded operands, S) - computed once per shape and A dtype"""
    x, w, _, _ = _randoms(shape)
    xa, W = x.to(a_dtype), w.to(torch.bfloat16)
    xb = xa.to(torch.bfloat16).double()
    return xa, W, xb @ W.double().t(), xb.abs() @ W.double().abs().t()


def _worst(err, bound, what):
    ratio = (err / bound).max().item()
    print(f"  {what}: worst |got - ref| / bound = {ratio:.4f}")
    return ratio


@shapes_and_dtypes
@pytest.mark.parametrize("variant", ["plain", "bias_relu", "bias_res"])
def test_exact_cases_are_bit_equal(shape, a_dtype, c_dtype, variant):
    from dfx import ops
    x, w, b, res = _integers(shape)
    b, res = (None if variant == "plain" else b), (res if variant == "bias_res" else None)
    got = ops.linear_bf16(x.to(a_dtype), w.to(torch.bfloat16), b, act="relu" if variant == "bias_relu" else None, residual=res,
                          out_dtype=c_dtype)
    ref = x.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    if res is not None:
        ref = ref + res.double()
    if variant == "bias_relu":
        ref = ref.relu()
    assert got.dtype == c_dtype and got.shape == ref.shape
    if c_dtype == torch.float32:
        assert torch.equal(got.double(), ref)
    else:
        assert torch.equal(got, ref.to(torch.bfloat16)), "one rounding of the exact result"


@pytest.mark.parametrize("rows", [1, 70, 333])
def test_fp32_a_is_rounded_to_nearest_even(rows):
    from dfx import ops
    K = 64
    g = torch.Generator(device="cuda").manual_seed(rows)
    a = torch.randn(rows, K, generator=g, device="cuda") * torch.logspace(-6, 6, K, device="cuda")
    ties = {1 + 2.0 ** -8: 1.0, 1 + 3 * 2.0 ** -8: 1.015625, 1 + 2.0 ** -8 + 2.0 ** -20: 1.0078125}
    crafted = [s * v for v in ties for s in (1.0, -1.0)]
    a[0, :len(crafted)] = torch.tensor(crafted, device="cuda")
    for i, (v, want) in enumerate(ties.items()):                   # the test's own arithmetic: torch rounds them as stated
        assert a[0, 2 * i].to(torch.bfloat16).item() == want and a[0, 2 * i + 1].to(torch.bfloat16).item() == -want
    assert torch.isfinite(a).all()
    eye = torch.eye(K, device="cuda", dtype=torch.bfloat16)
    got = ops.linear_bf16(a, eye)
    assert torch.equal(got, a.to(torch.bfloat16).float())


@shapes_and_dtypes
@pytest.mark.parametrize("variant", ["plain", "bias_relu", "bias_res", "bias_res_gelu"])
def test_random_operands_within_the_bound_on_every_element(shape, a_dtype, c_dtype, variant):
    from dfx import ops
    K = shape[2]
    _, _, b, res = _randoms(shape)
    xa, W, prod, S = _products(shape, a_dtype)
    b, res = (None if variant == "plain" else b), (res if "res" in variant else None)
    act = {"bias_relu": "relu", "bias_res_gelu": "gelu"}.get(variant)
    got = ops.linear_bf16(xa, W, b, act=act, residual=res, out_dtype=c_dtype)
    pre = prod
    if b is not None:
        pre = pre + b.double()
    if res is not None:
        pre = pre + res.double()
    E = K * 2.0 ** -23 * S + 2.0 ** -23 * pre.abs()
    ref = pre.relu() if act == "relu" else F.gelu(pre) if act == "gelu" else pre
    bound = 1.13 * E + 4e-6 * pre.abs().clamp(min=1.0) if act == "gelu" else E
    if c_dtype == torch.bfloat16:
        bound = bound + U * (ref.abs() + bound)
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    ratio = _worst(err, bound, f"{_id(shape)} A {_id(a_dtype)} C {_id(c_dtype)} {variant}")
    assert (err <= bound).all(), f"worst ratio {ratio}"


@shapes_and_dtypes
def test_input_rounding_costs_at_most_2u_of_the_absolute_product(shape, a_dtype, c_dtype):
    """What the mode costs: fp64 of the rounded operands (and the kernel's result with it) against the unrounded product."""
    from dfx import ops
    K = shape[2]
    x, w, _, _ = _randoms(shape)
    xa, W, prod, S = _products(shape, a_dtype)
    x0 = xa.double() if a_dtype == torch.bfloat16 else x.double()          # a bf16 A is the caller's input: only W is rounded then
    exact = x0 @ w.double().t()
    cost = (2 * U + U * U) * (x0.abs() @ w.double().abs().t())
    ratio = _worst((prod - exact).abs(), cost, f"{_id(shape)} A {_id(a_dtype)} input rounding")
    assert ((prod - exact).abs() <= cost).all(), f"worst ratio {ratio}"
    got = ops.linear_bf16(xa, W, out_dtype=c_dtype)
    E = K * 2.0 ** -23 * S + 2.0 ** -23 * prod.abs()
    bound = cost + (E if c_dtype == torch.float32 else E + U * (prod.abs() + E))
    assert ((got.double() - exact).abs() <= bound).all()


@shapes_and_dtypes
def test_five_calls_give_the_same_bits(shape, a_dtype, c_dtype):
    from dfx import ops
    _, _, b, res = _randoms(shape)
    xa, W, _, _ = _products(shape, a_dtype)
    first = ops.linear_bf16(xa, W, b, act="gelu", residual=res, out_dtype=c_dtype)
    for _ in range(4):
        assert torch.equal(ops.linear_bf16(xa, W, b, act="gelu", residual=res, out_dtype=c_dtype), first)


@shapes_and_dtypes
@pytest.mark.parametrize("pitch", ["aligned", "odd"])
def test_pitches_are_honoured_and_nothing_outside_c_is_written(shape, a_dtype, c_dtype, pitch):
    """A, R and C are slices of wider tensors; canaries in the padding columns and in rows beyond M stay."""
    from dfx import ops
    M, N, K = shape
    _, _, b, res = _randoms(shape)
    xa, W, _, _ = _products(shape, a_dtype)
    want = ops.linear_bf16(xa, W, b, act="relu", residual=res, out_dtype=c_dtype)
    lda, ldw = K + 8, K + 16                                       # rows of A and W stay 16-byte aligned
    ldr, ldc = (N + 4, N + 8) if pitch == "aligned" else (N + 1, N + 3)
    canary = 77.0                                                  # exact in bf16
    wide = lambda t, ld, rows: torch.full((rows, ld), canary, dtype=t.dtype, device="cuda")      # noqa: E731
    A, Wp, R, C = wide(xa, lda, M), wide(W, ldw, N), wide(res, ldr, M), torch.full((M + 3, ldc), canary, dtype=c_dtype, device="cuda")
    A[:, :K], Wp[:, :K], R[:, :N] = xa, W, res
    codes = {torch.float32: 0, torch.bfloat16: 1}
    ops._call("dfx_gemm_bf16", "dfx_gemm_bf16", A.device, A.data_ptr(), codes[a_dtype], lda, Wp.data_ptr(), ldw, b.data_ptr(),
              R.data_ptr(), ldr, C.data_ptr(), codes[c_dtype], ldc, M, N, K, 1)
    assert torch.equal(C[:M, :N], want), "the pitched call gives the contiguous call's bits"
    assert (C[:M, N:] == canary).all(), "padding columns of C were written"
    assert (C[M:] == canary).all(), "rows beyond M were written"
    assert (A[:, K:] == canary).all() and (R[:, N:] == canary).all() and (Wp[:, K:] == canary).all()


@shapes_and_dtypes
def test_row_ranges_give_the_single_call_bits(shape, a_dtype, c_dtype, monkeypatch):
    from dfx import ops
    _, _, b, res = _randoms(shape)
    xa, W, _, _ = _products(shape, a_dtype)
    want = ops.linear_bf16(xa, W, b, residual=res, out_dtype=c_dtype)
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda *a: (calls.append(a[-4]), real(*a))[1])      # a[-4]: the rows of the call
    monkeypatch.setattr(ops, "_GEMM_MAX_BYTES", 1)                                        # -> ranges of 128 rows
    got = ops.linear_bf16(xa, W, b, residual=res, out_dtype=c_dtype)
    assert calls == [min(128, shape[0] - r) for r in range(0, shape[0], 128)]
    assert torch.equal(got, want)


def test_leading_dimensions_are_kept_and_empty_inputs_return_empty():
    from dfx import ops
    x = torch.randn(2, 3, 5, 16, device="cuda")
    w = torch.randn(24, 16, device="cuda").to(torch.bfloat16)
    y = ops.linear_bf16(x, w, out_dtype=torch.bfloat16)
    assert y.shape == (2, 3, 5, 24) and torch.equal(y.reshape(30, 24), ops.linear_bf16(x.reshape(30, 16), w, out_dtype=torch.bfloat16))
    assert ops.linear_bf16(x[:0], w).shape == (0, 3, 5, 24)
