"""CPU: the RoIAlign backward reference of tests/_roi_cases.py is pinned to the committed oracle, and the two backward
entry points of include/dfx_roi.h are declared, exported, bound and reject bad arguments before any launch."""
import ctypes
import os
import re

import pytest
import torch

from tests import _roi_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dfx_roi_align_backward_nhwc_f32", "dfx_roi_align_backward_nchw_f32")


@pytest.mark.parametrize("H,W", [(13, 21), (50, 84)])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("sr", [1, 2, 3])
def test_restatement_equals_the_oracle(oracle, H, W, aligned, sr):
    """Both are fp32 evaluations of the same <= 36 products per element and differ in the order of the sum and of the
    1/sr^2 scaling only: measured bit-equal at sr = 1 and 4.8e-7 at worst over the twelve combinations on unit-normal
    data; the tolerance is 4x that.  A wrong corner, weight or skip decision shows at 1e-2 and above."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, H, W, generator=g)
    rois = rc.random_family(H, W, aligned, sr, seed=100 + sr)
    want = oracle.roi_align(x, rois, 7, 1 / 32, sr, aligned)
    got = rc.roi_align_torch(x, rois, 7, 1 / 32, sr, aligned)
    err = (got - want).abs().max().item()
    print(f"map {H}x{W} aligned={aligned} sr={sr}: {rois.shape[0]} RoIs, max |restatement - oracle| = {err:.3e}")
    assert err <= 2e-6


def test_restatement_is_its_own_adjoint_in_fp64():
    """<roi(x), g> = <x, roi^T(g)>: the chunked backward helper is the transpose of the forward."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 13, 21, generator=g, dtype=torch.float64)
    rois = rc.random_family(13, 21, True, 2, seed=7, per_image=100)
    go = torch.randn(rois.shape[0], 8, 7, 7, generator=g, dtype=torch.float64)
    lhs = (rc.roi_align_torch(x, rois, 7, 1 / 32, 2, True) * go).sum().item()
    rhs = (x * rc.reference_backward(x.shape, rois, go, 7, 1 / 32, 2, True, chunk=37)).sum().item()
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_exact_family_is_exact_on_the_cpu(oracle):
    """The builder's claim, without a GPU: fp32 autograd equals fp64 autograd and the oracle equals the fp64 forward,
    bit for bit."""
    x, rois, go = rc.exact_family()
    want = rc.roi_align_torch(x.double(), rois, rc.EXACT_SIZE, rc.EXACT_SCALE, rc.EXACT_SR, True)
    live = (rois[:, 0] >= 0) & (rois[:, 0] < x.shape[0])      # the oracle refuses a batch index outside [0, N)
    assert torch.equal(oracle.roi_align(x, rois[live], rc.EXACT_SIZE, rc.EXACT_SCALE, rc.EXACT_SR, True).double(), want[live])
    assert (~live).sum() == 2 and want[~live].abs().max() == 0
    xf = x.clone().requires_grad_(True)
    rc.roi_align_torch(xf, rois, rc.EXACT_SIZE, rc.EXACT_SCALE, rc.EXACT_SR, True).backward(go)
    ref = rc.reference_backward(x.shape, rois, go, rc.EXACT_SIZE, rc.EXACT_SCALE, rc.EXACT_SR, True)
    assert torch.equal(xf.grad.double(), ref) and ref.abs().max() > 0


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_roi.h")).read(), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} not declared"
    return " ".join(m.group(1).split())


@pytest.mark.parametrize("name", NAMES)
def test_header_library_and_binding_carry_the_backward(name):
    assert _declaration(name) == ("const float *grad_out, const float *rois, int N, int C, int H, int W, int K, "
                                  "int ph, int pw, float spatial_scale, int sampling_ratio, int aligned, "
                                  "float *grad_input, void *stream")
    from dfx import _lib
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_backward", "")]
    assert hasattr(ctypes.CDLL(_lib.library_path()), name)


@pytest.mark.parametrize("name", NAMES)
def test_backward_entry_points_reject_bad_arguments_before_any_launch(name):
    """Argument validation returns an error code without touching the GPU (no zero fill, no kernel)."""
    from dfx import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    one = 16       # any non-null, 16-byte aligned address: the checks below fail before it would be used
    assert fn(one, one, 1, 8, 4, 4, 1, 7, 7, 1.0, 2, 1, None, None) != 0 and b"null pointer" in lib.dfx_last_error()
    assert fn(None, one, 1, 8, 4, 4, 1, 7, 7, 1.0, 2, 1, one, None) != 0 and b"null pointer" in lib.dfx_last_error()
    assert fn(one, None, 1, 8, 4, 4, 1, 7, 7, 1.0, 2, 1, one, None) != 0 and b"null pointer" in lib.dfx_last_error()
    assert fn(one, one, 1, 8, 4, 4, 1, 7, 7, 1.0, 0, 1, one, None) != 0 and b"sampling_ratio" in lib.dfx_last_error()
    assert fn(one, one, 0, 8, 4, 4, 1, 7, 7, 1.0, 2, 1, one, None) != 0 and b"bad dimension" in lib.dfx_last_error()
    assert fn(one, one, 1, 8, 4, 4, -1, 7, 7, 1.0, 2, 1, one, None) != 0 and b"bad dimension" in lib.dfx_last_error()
    if "nhwc" in name:
        assert fn(one, one, 1, 6, 4, 4, 1, 7, 7, 1.0, 2, 1, one, None) != 0 and b"C % 4" in lib.dfx_last_error()
        assert fn(one, one, 1, 8, 4, 4, 1, 7, 7, 1.0, 2, 1, 20, None) != 0 and b"16-byte" in lib.dfx_last_error()


@pytest.mark.parametrize("channels_last", [False, True])
def test_cpu_tensors_are_rejected(channels_last):
    from dfx import ops
    go = torch.zeros(1, 49, 8) if channels_last else torch.zeros(1, 8, 7, 7)
    shape = (1, 4, 4, 8) if channels_last else (1, 8, 4, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.roi_align_backward(go, torch.tensor([[0, 0., 0., 8., 8.]]), shape, 7, 1.0, 2, True, channels_last)
