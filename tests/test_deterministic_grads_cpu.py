"""CPU: the host half of the deterministic training mode (dfx/ops.py, csrc/fixed_sum.h) - the mode decision, the fraction
bits of the host bound, the alert of the routes without a fixed-point twin, the new symbols of the library."""
import importlib
import math
import warnings

import pytest
import torch


@pytest.fixture()
def flag():
    """``flag(on, warn_only)`` sets torch's deterministic flag; restored at teardown."""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield lambda on=True, warn_only=False: torch.use_deterministic_algorithms(on, warn_only=warn_only)
    torch.use_deterministic_algorithms(was[0], warn_only=was[1])


@pytest.fixture()
def reloaded_ops(monkeypatch):
    """``reloaded_ops(value)``: dfx.ops imported afresh with DFX_DETERMINISTIC = value (None: unset); the module the rest of
    the process uses is put back at teardown by one more reload under the restored environment."""
    from dfx import ops

    def load(value):
        if value is None:
            monkeypatch.delenv("DFX_DETERMINISTIC", raising=False)
        else:
            monkeypatch.setenv("DFX_DETERMINISTIC", value)
        return importlib.reload(ops)

    yield load
    monkeypatch.undo()
    importlib.reload(ops)


def test_the_mode_follows_torch_unless_the_environment_says_otherwise(flag, reloaded_ops):
    ops = reloaded_ops(None)
    flag(False)
    assert not ops.deterministic_mode()
    flag(True)
    assert ops.deterministic_mode()
    flag(True, warn_only=True)
    assert ops.deterministic_mode()
    ops = reloaded_ops("0")                 # opted out: whatever torch says
    assert not ops.deterministic_mode()
    flag(False)
    assert not ops.deterministic_mode()
    ops = reloaded_ops("1")                 # on without the torch flag
    assert ops.deterministic_mode()
    flag(True)
    assert ops.deterministic_mode()


def test_the_environment_is_read_once_at_import(flag, reloaded_ops, monkeypatch):
    ops = reloaded_ops("1")
    flag(False)
    monkeypatch.setenv("DFX_DETERMINISTIC", "0")
    assert ops.deterministic_mode(), "a change after the import must not be seen"
    monkeypatch.delenv("DFX_DETERMINISTIC")
    assert ops.deterministic_mode()
    assert not importlib.reload(ops).deterministic_mode()


def _checked(F, n):
    assert 0 < F <= 50
    assert n * 2 ** F <= 2 ** 61
    assert F == min(50, 61 - math.ceil(math.log2(n)))


def test_fraction_bits_of_the_host_bounds():
    """F = min(50, 61 - ceil(log2 n)): n * 2^F <= 2^61, for the shapes of the GPU tests and the largest shipped ones."""
    from dfx import _lib
    lib = _lib.load()
    msda = [lib.dfx_msda_fixed_fraction_bits(lq) for lq in (1, 5, 37, 128, 129, 1100, 4200, 22223, 1 << 20)]
    for lq, F in zip((1, 5, 37, 128, 129, 1100, 4200, 22223, 1 << 20), msda):
        _checked(F, 16 * lq)                # (query, point, corner) triples of one head and level
    assert msda == sorted(msda, reverse=True), "more terms must never get more fraction bits"
    assert msda[0] == 50 and msda[3] == 50 and msda[4] == 49 and lib.dfx_msda_fixed_fraction_bits(22223) == 42
    assert lib.dfx_msda_fixed_fraction_bits(0) == 50
    roi = []
    for K, sr in ((1, 1), (64, 2), (127, 2), (607, 3), (9600, 2), (9600, 4), (100000, 4)):
        F = lib.dfx_roi_align_fixed_fraction_bits(K, 7, 7, sr)
        _checked(F, 4 * sr * sr * 49 * K)   # (RoI, bin, sample, corner) hits of one pixel
        roi.append(F)
    assert roi == sorted(roi, reverse=True)
    assert lib.dfx_roi_align_fixed_fraction_bits(9600, 7, 7, 2) == 38
    assert lib.dfx_roi_align_fixed_fraction_bits(0, 7, 7, 2) == lib.dfx_roi_align_fixed_fraction_bits(1, 7, 7, 2)


def test_alert_under_the_three_torch_settings(flag, monkeypatch):
    from dfx import ops
    monkeypatch.setattr(ops, "_DETERMINISTIC_ENV", None)
    monkeypatch.setattr(ops, "_ALERTED", set())
    flag(False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops._alert_not_deterministic("some_op")             # outside the mode: nothing
    flag(True)
    with pytest.raises(RuntimeError, match="some_op does not have a deterministic implementation"):
        ops._alert_not_deterministic("some_op")
    flag(True, warn_only=True)
    with pytest.warns(UserWarning, match="some_op does not have a deterministic implementation"):
        ops._alert_not_deterministic("some_op")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops._alert_not_deterministic("some_op")             # once per operation
    with pytest.warns(UserWarning, match="other_op"):
        ops._alert_not_deterministic("other_op")
    flag(False)
    with pytest.raises(RuntimeError, match="third_op"):     # a caller that has decided the mode itself
        ops._alert_not_deterministic("third_op", True)


def test_routes_without_a_twin_alert_before_they_look_at_their_operands(flag, monkeypatch):
    """The plain operator and the NCHW RoIAlign backward name themselves under the flag (on CPU tensors the refusal
    comes first; outside the mode the usual 'not implemented on the CPU' answer is unchanged)."""
    from dfx import ops
    monkeypatch.setattr(ops, "_DETERMINISTIC_ENV", None)
    v, s, l = torch.zeros(1, 4, 8, 32), torch.tensor([[2, 2]]), torch.tensor([0])
    loc, aw, go = torch.zeros(1, 3, 8, 1, 4, 2), torch.zeros(1, 3, 8, 1, 4), torch.zeros(1, 3, 256)
    roi = (torch.zeros(1, 4, 7, 7), torch.tensor([[0, 0., 0., 8., 8.]]), (1, 4, 8, 8), 7, 1.0)
    flag(False)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.msda_backward(v, s, l, loc, aw, go)
    flag(True)
    with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
        ops.msda_backward(v, s, l, loc, aw, go)
    with pytest.raises(RuntimeError, match=r"roi_align_backward \(NCHW\)"):
        ops.roi_align_backward(*roi, 2, True)
    with pytest.raises(RuntimeError, match="adaptive sampling_ratio"):
        ops.roi_align_backward(torch.zeros(1, 49, 4), roi[1], (1, 8, 8, 4), 7, 1.0, 0, True, channels_last=True)
    monkeypatch.setattr(ops, "_DETERMINISTIC_ENV", "0")     # opted out: the usual answer
    with pytest.raises(RuntimeError, match="CPU"):
        ops.msda_backward(v, s, l, loc, aw, go)


def test_the_library_exports_the_fixed_entries_and_keeps_its_abi_version():
    from dfx import _lib
    lib = _lib.load()
    for name in ("dfx_msda_level_grad_value_fixed_f32", "dfx_msda_fused_backward_fixed_f32",
                 "dfx_roi_align_backward_nhwc_fixed_f32", "dfx_msda_fixed_fraction_bits",
                 "dfx_roi_align_fixed_fraction_bits"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.abi_version() == 5
    # a null workspace or scratch word is refused before anything is enqueued (no GPU is touched here)
    one = 16
    assert lib.dfx_roi_align_backward_nhwc_fixed_f32(one, one, 1, 4, 8, 8, 1, 7, 7, 1.0, 2, 1, one, None, one, None) != 0
    assert b"workspace" in lib.dfx_last_error()
    assert lib.dfx_msda_level_grad_value_fixed_f32(one, 2, one, 64, one, 32, one, 1, 5, 7, 3, one, None, None) != 0
    assert b"scratch" in lib.dfx_last_error()
