"""torch-tensor front ends of the C ABI (device pointers + torch's current stream).

Mirrors the host half of the reference's CUDA op
(/root/reference/models/ops/src/cuda/ms_deform_attn_cuda.cu:20-153): the same
argument checks, the same dimension derivation (L from spatial_shapes.size(0), Lq from
sampling_loc.size(1), P from sampling_loc.size(4)), fresh output tensors.
"""
import ctypes
import os
import warnings

import torch

from . import _lib

_SUFFIX = {torch.float32: "f32", torch.float64: "f64"}
# 2-byte value maps (mixed precision, csrc/msda_forward.hip / msda_backward.hip): sampling_loc and attn_weight stay fp32
_HALF_SUFFIX = {torch.bfloat16: "bf16", torch.float16: "f16"}
_C = _lib.CONSTANTS      # the headers' #defines: workspace sizes and codes are the library's, never restated here
ACT = {None: _C["DFX_ACT_NONE"], "none": _C["DFX_ACT_NONE"], "relu": _C["DFX_ACT_RELU"], "gelu": _C["DFX_ACT_GELU"]}

# Single-level attention with many queries (encoder, depth fusion) runs on the level-in-LDS kernel
# (csrc/msda_level.hip) when the level fits the CU's LDS; DFX_MSDA_LEVEL=0 keeps the wave-per-query
# kernel (A/B measurements).  LEVEL_MIN_QUERIES: below it staging the level costs more than it saves.
USE_LEVEL_KERNEL = os.environ.get("DFX_MSDA_LEVEL", "1") == "1"
LEVEL_MIN_QUERIES = 1024
# In grad mode a single-level layer's grad_value is summed in LDS (csrc/msda_level_backward.hip) instead of by global
# atomics when the level fits and the launch has enough queries; DFX_MSDA_LEVEL_BWD=0 keeps the atomics everywhere (A/B
# measurements).  LEVEL_BWD_MIN_QUERIES (N * Lq) is the smallest launch MEASURED faster than the atomics beyond the
# repetition spread (profiles/r12_msda_level_backward.txt, 50 x 84 level): 1.18x at 32 frames x 300 queries, 1.09x / 1.57x
# at 4 / 32 frames x 4200; at 4 x 300 = 1200 the two routes tie inside a 20-35 % spread, and nothing between was measured.
USE_LEVEL_BWD = os.environ.get("DFX_MSDA_LEVEL_BWD", "1") != "0"
LEVEL_BWD_MIN_QUERIES = 9600
# Deterministic mode: the gradients many queries / RoIs add into - grad_value of the fused MSDA backward,
# grad_input of the channels-last RoIAlign - are summed in 64-bit fixed point (csrc/fixed_sum.h), bit-identical from call
# to call and under any order of the queries / RoIs.  On with torch.use_deterministic_algorithms(True); DFX_DETERMINISTIC=0
# opts this library out (A/B runs), DFX_DETERMINISTIC=1 turns the mode on without the torch flag.  Read once, at import.
_DETERMINISTIC_ENV = os.environ.get("DFX_DETERMINISTIC")
# convolutions of <= 4 input channels from an LDS-resident input tile (csrc/conv_tile.hip); 0: on the implicit GEMM (A/B runs)
USE_TILE_CONV = os.environ.get("DFX_TILE_CONV", "1") == "1"

# Measurement hook (bench.py): profile_start() makes every fused MSDA kernel stamp its own begin / end
# timestamps (include/dfx_msda.h, dfx_profile_*); profile_stop() returns [(seconds, algorithmic_bytes,
# Lq, S), ...] for the launches in between.
def profile_start():
    _lib.load().dfx_profile_enable(1)


def reload_tuning():
    """The library reads its DFX_* environment switches once per process (csrc/dfx_common.h:Tuning); call this after
    changing one of them in a running process (tests, A/B tools)."""
    _lib.load().dfx_tuning_reload()


def profile_stop(cap=65536):
    lib = _lib.load()
    lib.dfx_profile_enable(0)
    ms = (ctypes.c_float * cap)()
    nb = (ctypes.c_long * cap)()
    lq = (ctypes.c_int * cap)()
    s = (ctypes.c_int * cap)()
    n = lib.dfx_profile_drain(ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(nb, ctypes.c_void_p),
                              ctypes.cast(lq, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), cap)
    return [(ms[i] * 1e-3, nb[i], lq[i], s[i]) for i in range(n)]


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def deterministic_mode():
    """True when the backward routes must give the same bits on every call: torch's flag, unless DFX_DETERMINISTIC says
    otherwise.  The autograd nodes ask at backward time, as torch's own operators do."""
    if _DETERMINISTIC_ENV == "0":
        return False
    return _DETERMINISTIC_ENV == "1" or torch.are_deterministic_algorithms_enabled()


_ALERTED = set()       # operations that have warned under warn_only (once each)


def _alert_not_deterministic(op, deterministic=None):
    """What a torch operator without a deterministic implementation does, for the routes without a fixed-point twin:
    under the mode (`deterministic` None: ask it) raise RuntimeError naming `op`, or - when torch is set to warn only -
    warn once per operation and let the caller run as it does today.  Outside the mode nothing happens."""
    if not (deterministic_mode() if deterministic is None else deterministic):
        return
    msg = (f"{op} does not have a deterministic implementation, but the deterministic mode is on "
           "(torch.use_deterministic_algorithms(True) or DFX_DETERMINISTIC=1).  Turn the mode off for this operation "
           "(DFX_DETERMINISTIC=0 for this library alone) or pass warn_only=True to torch.use_deterministic_algorithms.")
    if not torch.is_deterministic_algorithms_warn_only_enabled():
        raise RuntimeError(msg)
    if op not in _ALERTED:
        _ALERTED.add(op)
        warnings.warn(msg, UserWarning, stacklevel=3)


def _check_inputs(named):
    # (messages are only formatted on failure: this runs for every launch of the path)
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError(f"{name} tensor has to be contiguous")
    for name, t in named:
        # the reference raises "Not implemented on the CPU" (ms_deform_attn.h:38,60)
        if not t.is_cuda:
            raise RuntimeError(f"Not implemented on the CPU ({name} must be a CUDA tensor)")
    dev = named[0][1].device
    for name, t in named:
        if t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, expected {dev}")


def _dims(value, spatial_shapes, sampling_loc, im2col_step):
    N, S, M, D = value.shape
    L = spatial_shapes.shape[0]
    Lq = sampling_loc.shape[1]
    P = sampling_loc.shape[4]
    step = min(N, im2col_step)
    _require(step > 0 and N % step == 0, f"batch({N}) must divide im2col_step({step})")
    return N, S, M, D, L, Lq, P


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev):
    """Raw handle of the current stream of `dev` (host time matters here: ~450 launches per 13 ms step of a 4-frame block)."""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(dev):
    """Context that makes `dev` the current device - a no-op object when it already is (one process per GPU: always)."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(dev)


_ENTRIES = {}      # name -> bound ctypes function of the loaded library


def _call(what, name, dev, *args):
    """One launch: the library's `name`(*args, current stream of `dev`) with `dev` current; a failure raises as `what`."""
    fn = _ENTRIES.get(name)
    if fn is None:
        fn = _ENTRIES[name] = getattr(_lib.load(), name)
    current = torch.cuda.current_device()
    if _raw_stream is not None and dev.index in (None, current):     # one process per GPU: always (host time, see _stream)
        rc = fn(*args, _raw_stream(current))
    else:
        with _on(dev):
            rc = fn(*args, _stream(dev))
    if rc != 0:
        _lib.check(rc, what)


def _operand_dtypes(what, value, sampling_loc, attn_weight):
    """The operator's dtype contract -> library suffix: fp32 / fp64 with locations and weights of the same dtype, or a
    bf16 / fp16 value with fp32 locations and weights (what MSDeformAttn produces under torch.autocast)."""
    if value.dtype in _HALF_SUFFIX:
        if sampling_loc.dtype != torch.float32 or attn_weight.dtype != torch.float32:
            raise RuntimeError(f"{what}: a {value.dtype} value needs fp32 (torch.float32) sampling_loc and attn_weight, "
                               f"got {sampling_loc.dtype} and {attn_weight.dtype}")
        return _HALF_SUFFIX[value.dtype]
    _require(value.dtype in _SUFFIX, f"{what} not implemented for {value.dtype}")
    _require(sampling_loc.dtype == value.dtype and attn_weight.dtype == value.dtype,
             "value, sampling_loc and attn_weight must share one dtype")
    return _SUFFIX[value.dtype]


def msda_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=64):
    _check_inputs([("value", value), ("spatial_shapes", spatial_shapes),
                   ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
                   ("attn_weight", attn_weight)])
    suffix = _operand_dtypes("ms_deform_attn_forward", value, sampling_loc, attn_weight)
    _require(spatial_shapes.dtype == torch.int64 and level_start_index.dtype == torch.int64,
             "spatial_shapes and level_start_index must be int64")
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, sampling_loc, im2col_step)
    _require(sampling_loc.numel() >= N * Lq * M * L * P * 2 and attn_weight.numel() >= N * Lq * M * L * P,
             "sampling_loc / attn_weight smaller than N*Lq*M*L*P")
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    _call("ms_deform_attn_forward", "dfx_msda_forward_" + suffix, value.device,
          value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
          attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr())
    return out


def msda_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                  im2col_step=64):
    # float atomics for every dtype; the reference's C signature has no room for a workspace
    _alert_not_deterministic("ms_deform_attn_backward")
    _check_inputs([("value", value), ("spatial_shapes", spatial_shapes),
                   ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
                   ("attn_weight", attn_weight), ("grad_output", grad_output)])
    suffix = _operand_dtypes("ms_deform_attn_backward", value, sampling_loc, attn_weight)
    _require(grad_output.dtype == value.dtype, f"grad_output must have value's dtype {value.dtype}, got {grad_output.dtype}")
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, sampling_loc, im2col_step)
    _require(grad_output.numel() == N * Lq * M * D, "grad_output has the wrong size")
    half = value.dtype in _HALF_SUFFIX
    # a 2-byte value's gradient is accumulated in fp32 (atomics) and rounded once below
    grad_value = torch.zeros(value.shape, dtype=torch.float32, device=value.device) if half else torch.zeros_like(value)
    grad_loc = torch.zeros_like(sampling_loc)
    grad_aw = torch.zeros_like(attn_weight)
    _call("ms_deform_attn_backward", "dfx_msda_backward_" + suffix, value.device,
          value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
          attn_weight.data_ptr(), grad_output.data_ptr(), N, S, M, D, L, Lq, P, grad_value.data_ptr(), grad_loc.data_ptr(),
          grad_aw.data_ptr())
    if half:
        grad_value = grad_value.to(value.dtype)
    return [grad_value, grad_loc, grad_aw]


def fused_supported(value, M, D, L, P, Lr):
    """Geometry the fused front-end kernel covers (else callers take the unfused op)."""
    return (value.is_cuda and value.dtype == torch.float32 and M == 8 and D == 32 and P == 4
            and 1 <= L <= 4 and (Lr == L or L == 1))


def _pitched_rows(t, N, Lq, width):
    """(tensor, row pitch in floats) of a [N,Lq,width] operand of the fused entry points: kept as it is when its rows
    are contiguous, 16-byte aligned and one constant pitch apart (a column slice of a wider buffer), else copied."""
    pitch = t.stride(1) if Lq > 1 else (t.stride(0) if N > 1 else width)
    if (t.stride(2) == 1 and pitch >= width and pitch % 4 == 0 and t.data_ptr() % 16 == 0
            and (N <= 1 or Lq <= 1 or t.stride(0) == Lq * pitch)):
        return t, pitch
    return t.contiguous(), width


def _msda_fused_operands(what, value, spatial_shapes, level_start_index, reference_points, rows, flat_read=False):
    """The operand contract of the fused taps kernel (include/dfx_msda.h), stated once for the forward, the trainable form
    and the backward: shapes and dtypes first, then placement (contiguous, on one GPU).
    rows: ((name, tensor, k), ...), the per-query operands, each [N,Lq,k*M*L*P] fp32 on value's device (rows may be
    strided).  flat_read admits Lr != L reference levels over a single value level (the temporal decoder's flat read,
    csrc/msda_fused.hip); without it there is one reference level per value level.
    -> N, S, M, D, L, Lq, P, Lr, ref_dim"""
    # (messages are only formatted on failure: this runs for every launch of the path)
    if value.dim() != 4 or spatial_shapes.dim() != 2:
        raise RuntimeError(f"{what}: value must be [N,S,M,D], spatial_shapes [L,2]")
    N, S, M, D = value.shape
    L = spatial_shapes.shape[0]
    Lr = reference_points.shape[2] if reference_points.dim() == 4 else -1
    if Lr < 0 or reference_points.shape[0] != N or not (Lr == L or (flat_read and L == 1)):
        raise RuntimeError(f"{what}: reference_points must be [N,Lq,{L},2|4] (one reference level per value level)")
    Lq, ref_dim = reference_points.shape[1], reference_points.shape[3]
    name, first, k = rows[0]
    if level_start_index.shape[0] != L or L <= 0 or M <= 0 or first.dim() != 3 or first.shape[2] % (k * M * L) != 0:
        raise RuntimeError(f"{what}: level_start_index must be [L] and {name} [N,Lq,{k}*M*L*P]")
    P = first.shape[2] // (k * M * L)
    if value.dtype != torch.float32 or reference_points.dtype != torch.float32:
        raise RuntimeError(f"{what} is implemented for float32")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("spatial_shapes and level_start_index must be int64")
    for name, t, k in rows:
        if t.shape != (N, Lq, k * M * L * P):
            raise RuntimeError(f"{what}: {name} must be [N,Lq,{k}*M*L*P]")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what} is implemented for float32")
    _check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                   ("reference_points", reference_points)])
    for name, t, _ in rows:
        if not t.is_cuda or t.device != value.device:
            raise RuntimeError(f"Not implemented on the CPU ({name} must be a CUDA tensor on {value.device})")
    return N, S, M, D, L, Lq, P, Lr, ref_dim


def _msda_fused_launch(what, value, spatial_shapes, level_start_index, reference_points, ref_dim, Lr,
                       offsets_ptr, off_pitch, logits_ptr, logit_pitch, N, S, M, D, L, Lq, P):
    """dfx_msda_fused_forward_f32 on validated operands: offsets and logits as two pointers with their row pitches in
    floats (two tensors, or two columns of one joint row).  -> [N,Lq,M*D]"""
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    _call(what, "dfx_msda_fused_forward_f32", value.device,
          value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), reference_points.data_ptr(), ref_dim, Lr,
          offsets_ptr, off_pitch, logits_ptr, logit_pitch, N, S, M, D, L, Lq, P, out.data_ptr())
    return out


def msda_fused_forward(value, spatial_shapes, level_start_index, reference_points, qproj, n_levels, n_points):
    """softmax + location arithmetic + sampling in one launch (include/dfx_msda.h,
    dfx_msda_fused_forward_f32).

    value            [N,S,M,D] fp32, contiguous
    reference_points [N,Lq,Lr,2|4]  (Lr = n_levels, or any Lr over a single value level: the flat read)
    qproj            [N,Lq,3*M*L*P] = one row per query holding the raw sampling_offsets
                     Linear output (M*L*P*2 floats) followed by the raw attention_weights
                     Linear output (M*L*P floats)
    -> [N,Lq,M*D]
    """
    reference_points = reference_points.contiguous()
    _require(spatial_shapes.shape[0] == n_levels, "spatial_shapes rows must equal n_levels")
    N, S, M, D, L, Lq, P, Lr, ref_dim = _msda_fused_operands(
        "msda_fused_forward", value, spatial_shapes, level_start_index, reference_points, (("qproj", qproj, 3),), flat_read=True)
    _require(P == n_points, "qproj has the wrong shape/dtype")
    _require(qproj.is_contiguous(), "qproj tensor has to be contiguous")
    mlp = M * L * P
    base = qproj.data_ptr()      # both columns of the joint row by address: no tensor views on this path
    return _msda_fused_launch("msda_fused_forward", value, spatial_shapes, level_start_index, reference_points, ref_dim, Lr,
                              base, 3 * mlp, base + 2 * mlp * 4, 3 * mlp, N, S, M, D, L, Lq, P)


def _msda_fused_forward_split(value, spatial_shapes, level_start_index, reference_points, offsets, logits):
    """The same launch on offsets and logits as two tensors; no autograd node."""
    N, S, M, D, L, Lq, P, Lr, ref_dim = _msda_fused_operands(
        "msda_fused", value, spatial_shapes, level_start_index, reference_points, (("offsets", offsets, 2), ("logits", logits, 1)))
    offsets, off_pitch = _pitched_rows(offsets, N, Lq, M * L * P * 2)
    logits, logit_pitch = _pitched_rows(logits, N, Lq, M * L * P)
    return _msda_fused_launch("msda_fused", value, spatial_shapes, level_start_index, reference_points, ref_dim, Lr,
                              offsets.data_ptr(), off_pitch, logits.data_ptr(), logit_pitch, N, S, M, D, L, Lq, P)


def msda_fused_backward(grad_out, value, spatial_shapes, level_start_index, reference_points, offsets, logits,
                        need_value=True, need_ref=False, deterministic=None):
    """Gradients of msda_fused from its inputs alone (include/dfx_msda.h, dfx_msda_fused_backward_f32: the kernel
    recomputes the softmax weights and the locations).  grad_out [N,Lq,M*D]; reference_points contiguous; offsets /
    logits as for msda_fused (rows may be column slices of a wider buffer).
    -> (grad_value [N,S,M,D] | None, grad_offsets like offsets, grad_logits like logits, grad_ref like reference_points | None)
    grad_value is summed with float atomics - global ones into a zero-filled buffer, or, for a single level that
    level_backward_supported admits, LDS ones in a second launch (dfx_msda_level_grad_value_f32) - and is only computed
    (and its buffer only allocated) with need_value; the other three are plain stores: two calls on the same inputs give
    the same bits.  deterministic (None: deterministic_mode()): the same routing rule with each side's fixed-point twin
    (dfx_msda_fused_backward_fixed_f32 / dfx_msda_level_grad_value_fixed_f32, csrc/fixed_sum.h) - grad_value too is then
    bit-identical from call to call and under any order of the queries; the other three keep their bits."""
    # (an empty value map has no workspace to hand over and nothing to sum: the float entry answers it)
    fixed = need_value and value.numel() > 0 and (deterministic_mode() if deterministic is None else bool(deterministic))
    N, S, M, D, L, Lq, P, _, ref_dim = _msda_fused_operands(
        "msda_fused_backward", value, spatial_shapes, level_start_index, reference_points,
        (("offsets", offsets, 2), ("logits", logits, 1)))
    grad_out = grad_out.contiguous()
    _require(grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.numel() == N * Lq * M * D,
             "msda_fused_backward: grad_out must be [N,Lq,M*D] fp32 on the GPU")
    offsets, off_pitch = _pitched_rows(offsets, N, Lq, M * L * P * 2)
    logits, logit_pitch = _pitched_rows(logits, N, Lq, M * L * P)
    dev = value.device
    # a single level that fits a CU's LDS under enough queries: the atomic-free instantiation for the small gradients, then
    # grad_value summed in LDS by msda_level_grad_value (two launches, no global atomic, no zero fill)
    hw = _level_backward_size(spatial_shapes, M, D, L, P, N, Lq) if need_value else None
    if hw is not None:
        # the kernel writes N * H * W rows and nothing else: a host copy of the sizes that disagrees with the value map
        # (a shapes tensor changed in place) must not reach it
        _require(hw[0] * hw[1] == S, "msda_fused_backward: the level's H * W differs from the value map's token count")
        grad_value = torch.empty_like(value)
    else:
        # the one buffer the float kernel accumulates into (the fixed-point form allocates its own below)
        grad_value = torch.zeros_like(value) if need_value and not fixed else None
    grad_off = torch.empty((N, Lq, M * L * P * 2), dtype=torch.float32, device=dev)
    grad_logits = torch.empty((N, Lq, M * L * P), dtype=torch.float32, device=dev)
    grad_ref = torch.empty((N, Lq, L, ref_dim), dtype=torch.float32, device=dev) if need_ref else None
    front = (value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), reference_points.data_ptr(), ref_dim,
             offsets.data_ptr(), off_pitch, logits.data_ptr(), logit_pitch, grad_out.data_ptr(), N, S, M, D, L, Lq, P)
    small = (grad_off.data_ptr(), M * L * P * 2, grad_logits.data_ptr(), M * L * P, _ptr(grad_ref))
    if fixed and hw is None:
        # the global form: int64 sums in a zero-filled workspace, which the entry converts into grad_value (written in full)
        grad_value = torch.empty_like(value)
        workspace = torch.zeros(value.shape, dtype=torch.int64, device=dev)
        _call("msda_fused_backward", "dfx_msda_fused_backward_fixed_f32", dev, *front, grad_value.data_ptr(),
              workspace.data_ptr(), _fixed_scratch(dev).data_ptr(), *small)
        return grad_value, grad_off, grad_logits, grad_ref
    _call("msda_fused_backward", "dfx_msda_fused_backward_f32", dev, *front, None if hw is not None else _ptr(grad_value), *small)
    if hw is not None:
        level = (reference_points.data_ptr(), ref_dim, offsets.data_ptr(), off_pitch, logits.data_ptr(), logit_pitch,
                 grad_out.data_ptr(), N, hw[0], hw[1], Lq, grad_value.data_ptr())
        if fixed:
            _call("msda_fused_backward", "dfx_msda_level_grad_value_fixed_f32", dev, *level, _fixed_scratch(dev).data_ptr())
        else:
            _call("msda_fused_backward", "dfx_msda_level_grad_value_f32", dev, *level)
    return grad_value, grad_off, grad_logits, grad_ref


def _fixed_scratch(dev):
    """The 16-byte scale word of a fixed-point launch (csrc/fixed_sum.h): fresh per call, cleared and filled on the device."""
    return torch.empty(4, dtype=torch.int32, device=dev)


def level_backward_supported(L, H, W, N, Lq, M=8, D=32, P=4):
    """Host decision: grad_value of this launch is summed in LDS by msda_level_grad_value (csrc/msda_level_backward.hip) -
    one level, the fused geometry, a level that fits the CU's LDS, the switch on and enough queries in the launch."""
    return (USE_LEVEL_BWD and L == 1 and M == 8 and D == 32 and P == 4 and N * Lq >= LEVEL_BWD_MIN_QUERIES
            and H > 0 and W > 0 and bool(_lib.load().dfx_msda_fused_level_fits(int(H), int(W))))


def _level_backward_size(spatial_shapes, M, D, L, P, N, Lq):
    """(H, W) of the single level when level_backward_supported, else None.  The host sizes ride on the shapes tensor
    (models.transformer_layers.make_level_tensors); a shapes tensor without them is read back once and keeps them."""
    if L != 1 or N * Lq == 0 or not level_backward_supported(L, 1, 1, N, Lq, M, D, P):     # all but the level's size
        return None
    host = getattr(spatial_shapes, "_dfx_host", None)
    if host is None:
        host = [(int(h), int(w)) for h, w in spatial_shapes.tolist()]
        spatial_shapes._dfx_host = host
    H, W = host[0]
    return (H, W) if level_backward_supported(L, H, W, N, Lq, M, D, P) else None


def msda_level_grad_value(grad_out, reference_points, offsets, logits, N, H, W, deterministic=None):
    """grad_value of single-level fused MSDA summed in LDS (include/dfx_msda.h, dfx_msda_level_grad_value_f32), on the
    operands of msda_fused_backward with one level.  A level that does not fit the CU's LDS raises; no other kernel steps in.

    grad_out [N,Lq,256], reference_points [N,Lq,1,2|4], offsets [N,Lq,64], logits [N,Lq,32] (rows may be column slices of
    a wider buffer), all fp32 on one GPU  -> [N,H*W,8,32], every element written; last bits may differ between calls,
    unless deterministic (None: deterministic_mode()) selects dfx_msda_level_grad_value_fixed_f32 (csrc/fixed_sum.h)."""
    what = "msda_level_grad_value"
    reference_points = _level_reference_points(reference_points, N)
    Lq, ref_dim = reference_points.shape[1], reference_points.shape[3]
    _require(ref_dim in (2, 4), f"{what}: reference_points must be [N, Lq, 1, 2|4]")
    rows = (("grad_out", grad_out, 256), ("offsets", offsets, 64), ("logits", logits, 32))
    # shapes and dtypes first, then placement (as _msda_fused_operands)
    for name, t, width in rows:
        if t.dim() != 3 or t.shape != (N, Lq, width):
            raise RuntimeError(f"{what}: {name} must be [N,Lq,{width}]")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what} is implemented for float32")
    _check_inputs([("reference_points", reference_points)])
    for name, t, _ in rows:
        if not t.is_cuda or t.device != reference_points.device:
            raise RuntimeError(f"Not implemented on the CPU ({name} must be a CUDA tensor on {reference_points.device})")
    _require(H > 0 and W > 0 and bool(_lib.load().dfx_msda_fused_level_fits(int(H), int(W))),
             f"{what}: a {H} x {W} level does not fit the level-in-LDS kernel")
    grad_out = grad_out.contiguous()
    offsets, off_pitch = _pitched_rows(offsets, N, Lq, 64)
    logits, logit_pitch = _pitched_rows(logits, N, Lq, 32)
    grad_value = torch.empty((N, H * W, 8, 32), dtype=torch.float32, device=grad_out.device)
    fixed = deterministic_mode() if deterministic is None else bool(deterministic)
    _call(what, "dfx_msda_level_grad_value_fixed_f32" if fixed else "dfx_msda_level_grad_value_f32", grad_out.device,
          reference_points.data_ptr(), ref_dim, offsets.data_ptr(), off_pitch, logits.data_ptr(), logit_pitch,
          grad_out.data_ptr(), N, int(H), int(W), Lq, grad_value.data_ptr(),
          *((_fixed_scratch(grad_out.device).data_ptr(),) if fixed else ()))
    return grad_value


class _MSDAFusedFunction(torch.autograd.Function):
    """apply(value, spatial_shapes, level_start_index, reference_points, offsets, logits): saves its inputs only; the
    backward kernel recomputes the rest."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, reference_points, offsets, logits):
        ctx.save_for_backward(value, spatial_shapes, level_start_index, reference_points, offsets, logits)
        return _msda_fused_forward_split(value, spatial_shapes, level_start_index, reference_points, offsets, logits)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        need = ctx.needs_input_grad
        # (deterministic=None: msda_fused_backward asks deterministic_mode() now, at backward time, as torch's operators do)
        gv, go, gl, gr = msda_fused_backward(grad_output, *ctx.saved_tensors, need_value=need[0], need_ref=need[3])
        return gv, None, None, gr, go if need[4] else None, gl if need[5] else None


def msda_fused(value, spatial_shapes, level_start_index, reference_points, offsets, logits, n_levels, n_points):
    """softmax + location arithmetic + sampling in one launch, trainable (include/dfx_msda.h,
    dfx_msda_fused_forward_f32 / dfx_msda_fused_backward_f32).

    value            [N,S,M,D] fp32, contiguous (M = 8, D = 32)
    reference_points [N,Lq,n_levels,2|4]
    offsets          [N,Lq,M*L*P*2]  raw sampling_offsets Linear output   \\ last dimension contiguous; rows may be
    logits           [N,Lq,M*L*P]    raw attention_weights Linear output  / column slices of one wider buffer
    -> [N,Lq,M*D], the bits of msda_fused_forward on the concatenated rows.
    With grad mode on and value, reference_points, offsets or logits requiring a gradient the result carries it back
    through msda_fused_backward (gradients for exactly the inputs that ask for one); otherwise no autograd node is made."""
    _require(spatial_shapes.shape[0] == n_levels and logits.shape[-1] == value.shape[2] * n_levels * n_points,
             "msda_fused: spatial_shapes rows must equal n_levels and logits be [N,Lq,M*n_levels*n_points]")
    reference_points = reference_points.contiguous()
    # (the operands are validated once, by the forward helper both branches end in)
    if torch.is_grad_enabled() and (value.requires_grad or reference_points.requires_grad or offsets.requires_grad
                                    or logits.requires_grad):
        return _MSDAFusedFunction.apply(value, spatial_shapes, level_start_index, reference_points, offsets, logits)
    return _msda_fused_forward_split(value, spatial_shapes, level_start_index, reference_points, offsets, logits)


def level_supported(value_like, H, W, Lq, n_heads, head_dim, n_levels, n_points, n_ref_levels):
    """Single-level attention the level-in-LDS kernel (csrc/msda_level.hip) should run: its
    geometry, a level that fits the CU's LDS, and enough queries to pay for staging the level."""
    return (USE_LEVEL_KERNEL and value_like.is_cuda and value_like.dtype == torch.float32 and n_heads == 8
            and head_dim == 32 and n_points == 4 and n_levels == 1 and n_ref_levels == 1
            and Lq >= LEVEL_MIN_QUERIES and bool(_lib.load().dfx_msda_fused_level_fits(int(H), int(W))))


def _msda_level_launch(what, value, reference_points, qproj, logits_at, layout, N, H, W, out_shape):
    """dfx_msda_fused_level_forward_f32 (include/dfx_msda.h) on operands whose shapes the caller has checked: `layout` holds
    their strides, the logits of a query's first head start `logits_at` floats behind its offsets."""
    Lq, ref_dim = reference_points.shape[1], reference_points.shape[3]
    out = torch.empty(out_shape, dtype=torch.float32, device=value.device)
    base = qproj.data_ptr()
    _call(what, "dfx_msda_fused_level_forward_f32", value.device, value.data_ptr(), reference_points.data_ptr(), ref_dim,
          base, base + 4 * logits_at, ctypes.byref(layout), N, H, W, Lq, out.data_ptr())
    return out


def _level_reference_points(reference_points, N):
    reference_points = reference_points.contiguous()
    _require(reference_points.dim() == 4 and reference_points.shape[0] == N and reference_points.shape[2] == 1
             and reference_points.dtype == torch.float32, "reference_points must be [N, Lq, 1, 2|4] fp32")
    return reference_points


def msda_level_forward(value_blk, reference_points, qproj_blk, N, H, W):
    """Fused single-level MSDA on operands in the block-major layouts linear(col_block=...) writes and
    linear(x_blocked=True) reads (include/dfx_msda.h, dfx_msda_fused_level_forward_f32):

    value_blk        [64, N*H*W, 4]  4-channel chunk k of every token (value_proj, col_block=4)
    reference_points [N, Lq, 1, 2|4]
    qproj_blk        [8, N*Lq, 12]   per head: 4 points x (x, y) offsets, then the 4 logits (col_block=12 of the
                                     head-interleaved sampling_offsets / attention_weights Linear)
    -> [64, N*Lq, 4]  the sampled values, 4-channel chunk k of every query (output_proj's x_blocked operand)
    """
    reference_points = _level_reference_points(reference_points, N)
    _check_inputs([("value_blk", value_blk), ("reference_points", reference_points), ("qproj_blk", qproj_blk)])
    Lq = reference_points.shape[1]
    ns, nq = N * H * W, N * Lq
    _require(value_blk.shape == (64, ns, 4) and value_blk.dtype == torch.float32, "value_blk must be [64, N*H*W, 4] fp32")
    _require(qproj_blk.shape == (8, nq, 12) and qproj_blk.dtype == torch.float32, "qproj_blk must be [8, N*Lq, 12] fp32")
    ly = _lib.LevelLayout(H * W * 4, 4, 32 * ns, 8 * ns, 4 * ns, 12, 12 * nq, 12, 12 * nq, 4, 32 * nq, 8 * nq, 4 * nq)
    return _msda_level_launch("msda_level_forward", value_blk, reference_points, qproj_blk, 8, ly, N, H, W, (64, nq, 4))


def msda_level_forward_reference(value, reference_points, qproj, H, W):
    """The level-in-LDS kernel on operands in the reference layouts, those of msda_fused_forward with one level.  There it
    is slower than the wave-per-query kernel (33 vs 26 us at the encoder geometry), so no product path calls it: parity
    tests and probes do, by this name.  A level that does not fit the CU's LDS raises; no other kernel steps in.

    value [N,H*W,8,32] fp32, reference_points [N,Lq,1,2|4], qproj [N,Lq,96] (64 offsets | 32 logits)  -> [N,Lq,256]
    """
    _require(value.dim() == 4 and qproj.dim() == 3, "value must be [N,H*W,8,32], qproj [N,Lq,96]")
    N = value.shape[0]
    reference_points = _level_reference_points(reference_points, N)
    _check_inputs([("value", value), ("reference_points", reference_points), ("qproj", qproj)])
    Lq, S = reference_points.shape[1], H * W
    _require(value.shape == (N, S, 8, 32) and value.dtype == torch.float32, "value must be [N, H*W, 8, 32] fp32")
    _require(qproj.shape == (N, Lq, 96) and qproj.dtype == torch.float32, "qproj must be [N, Lq, 96] fp32")
    _require(bool(_lib.load().dfx_msda_fused_level_fits(int(H), int(W))),
             f"msda_level_forward_reference: a {H} x {W} level does not fit the level-in-LDS kernel")
    ly = _lib.LevelLayout(S * 256, 256, 32, 8, 4, 96, 8, 96, 4, 256, 32, 8, 4)
    return _msda_level_launch("msda_level_forward_reference", value, reference_points, qproj, 64, ly, N, H, W, (N, Lq, 256))


def _roi_align_forward(inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last):
    """The forward entry of include/dfx_roi.h on a float [K,5] contiguous `rois`; no autograd node."""
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    _check_inputs([("input", inp), ("rois", rois)])
    _require(inp.dtype == torch.float32, "roi_align is implemented for float32")
    _require(rois.dim() == 2 and rois.shape[1] == 5, "rois must be [K,5]")
    K = rois.shape[0]
    if channels_last:
        N, H, W, C = inp.shape
        out = torch.empty((K, ph * pw, C), dtype=inp.dtype, device=inp.device)
        fn = "dfx_roi_align_nhwc_f32"
    else:
        N, C, H, W = inp.shape
        out = torch.empty((K, C, ph, pw), dtype=inp.dtype, device=inp.device)
        fn = "dfx_roi_align_nchw_f32"
    _call("roi_align", fn, inp.device, inp.data_ptr(), rois.data_ptr(), N, C, H, W, K, ph, pw, float(spatial_scale),
          int(sampling_ratio), int(bool(aligned)), out.data_ptr())
    return out


def roi_align_backward(grad_out, rois, input_shape, output_size, spatial_scale, sampling_ratio, aligned=True,
                       channels_last=False, deterministic=None):
    """Gradient of roi_align with respect to its input (the RoIs get none) through include/dfx_roi.h.

    channels_last=False: grad_out [K,C,ph,pw] contiguous -> [N,C,H,W] = input_shape
    channels_last=True : grad_out [K,ph*pw,C] contiguous -> [N,H,W,C] = input_shape
    The library zero-fills the fresh result and accumulates into it with fp32 atomics.
    deterministic (None: deterministic_mode()): the channels-last form sums in 64-bit fixed point instead
    (dfx_roi_align_backward_nhwc_fixed_f32, csrc/fixed_sum.h) - the same bits on every call and for any order of the RoIs.
    The NCHW form and the adaptive grid (sampling_ratio <= 0) have no such twin: under the mode they raise, or warn once
    and run as above when torch is set to warn only.
    """
    fixed = deterministic_mode() if deterministic is None else bool(deterministic)
    if fixed and not channels_last:
        _alert_not_deterministic("roi_align_backward (NCHW)", True)
        fixed = False
    elif fixed and int(sampling_ratio) <= 0:
        _alert_not_deterministic("roi_align_backward (adaptive sampling_ratio)", True)
        fixed = False
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    rois = rois.contiguous().float()
    _check_inputs([("grad_output", grad_out), ("rois", rois)])
    _require(grad_out.dtype == torch.float32, "roi_align_backward is implemented for float32")
    _require(rois.dim() == 2 and rois.shape[1] == 5, "rois must be [K,5]")
    _require(len(input_shape) == 4, "input_shape must be the forward input's 4-d shape")
    K = rois.shape[0]
    if channels_last:
        N, H, W, C = input_shape
        want, fn = (K, ph * pw, C), "dfx_roi_align_backward_nhwc_f32"
    else:
        N, C, H, W = input_shape
        want, fn = (K, C, ph, pw), "dfx_roi_align_backward_nchw_f32"
    _require(tuple(grad_out.shape) == want, f"grad_output must be {want}, got {tuple(grad_out.shape)}")
    grad_input = torch.empty(tuple(input_shape), dtype=grad_out.dtype, device=grad_out.device)
    extra = ()
    if fixed:
        fn = "dfx_roi_align_backward_nhwc_fixed_f32"
        workspace = torch.zeros(tuple(input_shape), dtype=torch.int64, device=grad_out.device)
        extra = (workspace.data_ptr(), _fixed_scratch(grad_out.device).data_ptr())
    _call("roi_align_backward", fn, grad_out.device, grad_out.data_ptr(), rois.data_ptr(), N, C, H, W, K, ph, pw,
          float(spatial_scale), int(sampling_ratio), int(bool(aligned)), grad_input.data_ptr(), *extra)
    return grad_input


class _RoIAlignFunction(torch.autograd.Function):
    """apply(inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last); gradient for `inp` only."""

    @staticmethod
    def forward(ctx, inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last):
        ctx.args = (tuple(inp.shape), output_size, spatial_scale, sampling_ratio, aligned, channels_last)
        ctx.save_for_backward(rois)
        return _roi_align_forward(inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        rois, = ctx.saved_tensors
        shape, output_size, spatial_scale, sampling_ratio, aligned, channels_last = ctx.args
        # (the mode is asked inside, at backward time)
        grad_input = roi_align_backward(grad_output.contiguous(), rois, shape, output_size, spatial_scale, sampling_ratio,
                                        aligned, channels_last)
        return grad_input, None, None, None, None, None, None


def roi_align(inp, rois, output_size, spatial_scale, sampling_ratio, aligned=True, channels_last=False):
    """RoIAlign (avg, fixed sampling grid) through include/dfx_roi.h.

    channels_last=False: inp [N,C,H,W] contiguous -> [K,C,ph,pw]
    channels_last=True : inp [N,H,W,C] contiguous -> [K,ph*pw,C]   (token-major memory, no transpose)
    rois [K,5] = (batch index, x1, y1, x2, y2)
    With grad mode on and an input that requires a gradient the result carries it back into `inp`
    (roi_align_backward); the RoIs get no gradient.  Otherwise no autograd node is made.
    """
    rois = rois.contiguous().float()
    if inp.requires_grad and torch.is_grad_enabled():
        return _RoIAlignFunction.apply(inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last)
    return _roi_align_forward(inp, rois, output_size, spatial_scale, sampling_ratio, aligned, channels_last)


def bias_act_(x, bias, residual=None, relu=True):
    """In place on ``x`` [N,C,*spatial] (contiguous NCHW): x = relu?(x + bias[c] (+ residual)).
    One HBM pass for what the reference runs as FrozenBatchNorm2d (after folding its scale into
    the convolution weights) + residual add + ReLU (include/dfx_fused.h).
    The arithmetic is (x + b) + r in fp32, then fmaxf(., 0): finite and infinite values come out bit-equal to that
    expression in torch.  A NaN does not: fmaxf returns its other operand, so with ``relu`` a NaN element becomes 0
    where torch.relu would keep it; without ``relu`` it stays NaN."""
    named = [("x", x), ("bias", bias)] + ([("residual", residual)] if residual is not None else [])
    _check_inputs(named)
    _require(x.dtype == torch.float32 and bias.dtype == torch.float32, "bias_act_ is implemented for float32")
    N, C = x.shape[0], x.shape[1]
    _require(bias.numel() == C, "bias must have one entry per channel")
    if residual is not None:
        _require(residual.shape == x.shape and residual.dtype == x.dtype, "residual must match x")
    hw = x.numel() // max(N * C, 1)
    _call("bias_act_", "dfx_bias_act_nchw_f32", x.device, x.data_ptr(), bias.data_ptr(), _ptr(residual), x.data_ptr(),
          N, C, hw, int(bool(relu)))
    return x


def _ptr(t):
    return 0 if t is None else t.data_ptr()


_GEMM_MAX_BYTES = 1 << 31          # tests lower it to exercise the row-range path on small tensors
# (linear(norm=...) is the GEMM followed by add_layernorm: LayerNorm in the GEMM epilogue was measured slower, DESIGN.md "Residual + LayerNorm in the epilogue")
_SPLITK_MIN_K = int(os.environ.get("DFX_SPLITK_MIN_K", "2048"))      # (A/B aids)
_SPLITK_RANGE = int(os.environ.get("DFX_SPLITK_RANGE", "512"))


def _split_k(M, N, K):
    """Number of K ranges for a GEMM with few output tiles and a long K (0 = no split): as many as keep the
    128 x 128 (or 64 x 128 for small M) tiles x ranges within one resident round of workgroups (3 per CU for the
    large tile, 4 for the small one), at least 32 K-steps per range."""
    if K < _SPLITK_MIN_K:
        return 0
    if M >= 128 and N >= 128:
        tiles, slots = -(-M // 128) * -(-N // 128), 768
    else:
        tiles, slots = -(-M // 64) * -(-N // 128), 1024
    if tiles * 2 > slots:
        return 0
    return max(1, min(K // _SPLITK_RANGE, slots // tiles))


def _gemm_f32(what, dev, A, B, C, M, N, K, lda, ldb, ldc, A2=0, strideA=0, strideB=0, b_is_kn=0, bias=0, bias_per_row=0,
              R=0, ldr=0, strideR=0, row_mask=0, strideMask=0, strideC=0, batch=1, relu=0, c_block=0, c_block_stride=0,
              a_block_stride=0):
    """One ``dfx_gemm_f32`` launch under the parameter names of include/dfx_gemm.h, which documents them.  A, B, C and the
    optional operands are device addresses; what a caller leaves out is absent (NULL, stride 0, a single batch)."""
    _call(what, "dfx_gemm_f32", dev, A, A2, lda, strideA, B, ldb, strideB, b_is_kn, bias, bias_per_row, R, ldr, strideR,
          row_mask, strideMask, C, ldc, strideC, M, N, K, batch, relu, c_block, c_block_stride, a_block_stride)


def _row_ranges(M, row_bytes, rows_max=None):
    """(r0, r1) row ranges that cover M rows.  The GEMM kernels address an operand with 32-bit byte offsets (buffer loads), so
    one call's operands stay below ``_GEMM_MAX_BYTES`` (read here, at call time): at most that many rows of ``row_bytes``,
    the widest operand's row - or ``rows_max`` where the caller has another cap - in whole multiples of 128, at least 128.
    Every layout of these front ends is row-separable (strides are explicit arguments): a range is the same call on offset
    pointers."""
    if rows_max is None:
        rows_max = (_GEMM_MAX_BYTES - 1) // row_bytes
    rows_max = max(128, rows_max // 128 * 128)
    for r0 in range(0, M, rows_max):
        yield r0, min(M, r0 + rows_max)


def linear(x, weight, bias=None, relu=False, residual=None, add=None, row_mask=None, col_block=0, x_blocked=False,
           act=None, norm=None, act_first=False):
    """y = act((x (+ add)) @ weight.T + bias (+ residual)), rows where row_mask is True set to 0.
    act: None / "relu" / "gelu" (``relu=True`` is the older spelling of act="relu").
    The hand-written fp32 MFMA GEMM (include/dfx_gemm.h) standing in for nn.Linear with its
    neighbours fused: the ``src + pos`` query add, the bias, ReLU, the residual add and
    value_proj's masked_fill.  x [..., K] contiguous, weight [N, K] -> [..., N].

    norm: an nn.LayerNorm(256) applied to the result rows by an add_layernorm launch after the GEMM:
    y = norm(residual + act(...)) with ``act_first`` (the activation before the residual add), else norm(act(... + residual));
    needs N == 256, no row_mask, no col_block.

    col_block = w > 0 stores the result column-block-major instead: [N / w, rows, w] (the layout
    msda_level_forward reads), N a multiple of w.  x_blocked: x is K-block-major [K/4, rows, 4] (the
    layout msda_level_forward writes); the result is then [rows, N]."""
    N = weight.shape[0]
    if x_blocked:
        _require(x.dim() == 3 and x.shape[2] == 4 and add is None, "x_blocked: x must be [K/4, rows, 4], no add")
        K, M, x2 = x.shape[0] * 4, x.shape[1], x
    else:
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
    named = [("x", x2), ("weight", weight)]
    for nm, t in (("bias", bias), ("residual", residual), ("add", add), ("row_mask", row_mask)):
        if t is not None:
            named.append((nm, t))
    _check_inputs(named)
    _require(x2.dtype == torch.float32 and weight.dtype == torch.float32, "linear is implemented for float32")
    _require(weight.shape[1] == K and K % 4 == 0, "weight must be [N, K] with K a multiple of 4")
    if add is not None:
        _require(add.shape == x.shape, "add must match x")
    if col_block:
        _require(N % col_block == 0 and residual is None, "col_block must divide N; no residual in this layout")
        out = torch.empty((N // col_block, M, col_block), dtype=x.dtype, device=x.device)
    elif x_blocked:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    else:
        out = torch.empty(x.shape[:-1] + (N,), dtype=x.dtype, device=x.device)
    if residual is not None:
        _require(residual.shape == out.shape or (x_blocked and residual.numel() == out.numel()),
                 "residual must match the output")
    if row_mask is not None:
        _require(row_mask.numel() == M, "row_mask must have one entry per row")
        row_mask = row_mask.reshape(-1).to(torch.uint8) if row_mask.dtype != torch.uint8 else row_mask.reshape(-1)
    code = ACT[act] if act is not None else int(bool(relu))
    if norm is not None:
        _require(N == 256 and row_mask is None and not col_block and norm.weight.numel() == 256 and norm.weight.is_cuda,
                 "linear(norm=...): a LayerNorm over exactly 256 output columns, no row_mask / col_block")
        if code and not act_first:
            # the residual rides in the GEMM's epilogue (prefetched while the tile crosses LDS): the LayerNorm pass then reads one
            # tensor instead of two.  Same sum, same order: (x W^T + b) + residual
            y = linear(x, weight, bias, residual=residual, add=add, x_blocked=x_blocked, act=act, relu=relu)
            return add_layernorm(y, None, norm)
        y = linear(x, weight, bias, add=add, x_blocked=x_blocked, act=act, relu=relu)
        return add_layernorm(y, None if residual is None else residual.reshape(y.shape), norm)
    splits = _split_k(M, N, K) if (add is None and row_mask is None and not col_block and not x_blocked and N % 4 == 0) else 0
    if splits > 1:
        ws = torch.empty((splits, M, N), dtype=torch.float32, device=x.device)
        _call("linear (split-K)", "dfx_gemm_splitk_f32", x.device, x2.data_ptr(), K, weight.data_ptr(), K, 0, _ptr(bias), 0,
              _ptr(residual), N, out.data_ptr(), N, M, N, K, code, splits, ws.data_ptr())
        return out
    # A, and the residual, must stay below 2 GiB per call: more rows than that (long clips of multi-scale token maps) go
    # through in row ranges
    if x_blocked:
        _require(M * K * 4 < _GEMM_MAX_BYTES, "linear: a K-block-major x of 2 GiB or more is not supported")
    out_row = int(col_block) if col_block else N            # elements a row advances the output pointer by
    with _on(x.device):
        for r0, r1 in _row_ranges(M, 4 * max(K, N if residual is not None else 1), rows_max=M if x_blocked else None):
            off = lambda t, per_row: 0 if t is None else t.data_ptr() + r0 * per_row * t.element_size()  # noqa: E731
            _gemm_f32("linear", x.device, off(x2, 4 if x_blocked else K), weight.data_ptr(), off(out, out_row), r1 - r0, N, K,
                      K, K, N, A2=off(add, K), bias=_ptr(bias), R=off(residual, N), ldr=N, row_mask=off(row_mask, 1), relu=code,
                      c_block=int(col_block), c_block_stride=M * int(col_block), a_block_stride=M * 4 if x_blocked else 0)
    return out


_BF16_DTYPE_CODE = {torch.float32: _C["DFX_DT_F32"], torch.bfloat16: _C["DFX_DT_BF16"]}


def linear_bf16(x, weight_bf16, bias=None, act=None, residual=None, out_dtype=torch.float32):
    """y = act(x @ weight_bf16.T + bias (+ residual)) on the bf16 MFMA GEMM (include/dfx_gemm_bf16.h, csrc/gemm_bf16.hip):
    bf16 products, fp32 accumulation, bias / residual / activation in fp32.
    x [..., K] contiguous, fp32 (rounded to bf16 as ``x.to(torch.bfloat16)`` does, inside the kernel) or bf16; weight_bf16 [N, K]
    bf16; bias [N] and residual [..., N] fp32.  act: None / "relu" / "gelu".  -> [..., N] in ``out_dtype`` (fp32, or bf16 rounded
    once from the fp32 result).  K must be a multiple of 8."""
    K = x.shape[-1]
    N = weight_bf16.shape[0]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    named = [("x", x2), ("weight", weight_bf16)]
    for nm, t in (("bias", bias), ("residual", residual)):
        if t is not None:
            named.append((nm, t))
    # (dtypes and shapes first: they are refused the same way wherever the tensors live)
    _require(x2.dtype in _BF16_DTYPE_CODE and out_dtype in _BF16_DTYPE_CODE, "linear_bf16: x and out_dtype must be float32 or bfloat16")
    _require(weight_bf16.dtype == torch.bfloat16, "linear_bf16: the weight must be bfloat16")
    _require(weight_bf16.dim() == 2 and weight_bf16.shape[1] == K and K % 8 == 0 and K > 0,
             "linear_bf16: weight must be [N, K] with K a multiple of 8")
    _check_inputs(named)
    _require(bias is None or (bias.dtype == torch.float32 and bias.numel() == N), "linear_bf16: bias must be float32 [N]")
    out = torch.empty(x.shape[:-1] + (N,), dtype=out_dtype, device=x.device)
    if residual is not None:
        _require(residual.dtype == torch.float32 and residual.shape == out.shape, "linear_bf16: residual must be float32 and match the output")
    ea, ec = x2.element_size(), out.element_size()
    a_code, c_code, code = _BF16_DTYPE_CODE[x2.dtype], _BF16_DTYPE_CODE[out_dtype], ACT[act]
    for r0, r1 in _row_ranges(M, max(K * ea, N * ec, N * 4 if residual is not None else 1)):
        _call("linear_bf16", "dfx_gemm_bf16", x.device, x2.data_ptr() + r0 * K * ea, a_code, K, weight_bf16.data_ptr(), K, _ptr(bias),
              0 if residual is None else residual.data_ptr() + r0 * N * 4, N, out.data_ptr() + r0 * N * ec, c_code, N,
              r1 - r0, N, K, code)
    return out


# ---- Linear in grad mode (include/dfx_gemm.h dfx_gemm_wgrad_f32, include/dfx_gemm_bf16.h dfx_gemm_bf16_wgrad; csrc/wgrad_frame.h) ----
# The fp32 split rule's two constants, both measured (tools/bench_linear_train.py, profiles/r14_linear_train.txt): ranges of at
# least 16 row steps are 5-9 % ahead of 32-step ranges at 9600 rows (36 ranges against 18) and tie elsewhere; beyond ~256
# ranges the reduction's traffic costs more than the shorter ranges save (32 x 4200 rows, N <= 128: 382-495 ranges 7-29 %
# behind 255).  DFX_WGRAD_MIN_STEPS / DFX_WGRAD_MAX_RANGES are A/B aids.
_WGRAD_MIN_STEPS = int(os.environ.get("DFX_WGRAD_MIN_STEPS", "16"))
_WGRAD_MAX_RANGES = int(os.environ.get("DFX_WGRAD_MAX_RANGES", "256"))

# The split rule's constants for the bf16 kernel, measured (tools/bench_linear_bf16_train.py --ranges, profiles/r22_linear_bf16_train.txt).
# The kernel moves a range two to three times faster than the fp32 one, so the reduction's traffic weighs more and fewer, longer
# ranges win: tiles x ranges within 512 workgroups (two per CU) and at most 64 ranges are within 5 % of the best count at every
# shape tried (32 x 4200 rows: 256 -> 1024 177 us at 32 ranges against 193 at 48 and 213 at 64; 256 -> 256 90 us at 64, 87 at 96,
# 111 at 191; 256 -> 64 64 us at 64, 61 at 96, 101 at 248).  The shortest range stays ``_WGRAD_MIN_STEPS`` = 16 steps, here of 32
# rows: at 9600 and 4 x 4200 rows 16-step ranges are the best or within 2 % of it, 32-step ranges are 8-19 % behind.
_WGRAD_BF16_SLOTS = 512
_WGRAD_BF16_MAX_RANGES = 64


def _wgrad_ranges(M, splits, step=16):
    """(rows per range, ranges) the library makes of a request for ``splits`` ranges over M rows: whole steps of ``step`` rows
    (16: the fp32 kernels, 32: ``dfx_gemm_bf16_wgrad``), none empty."""
    kper = ((M + splits - 1) // splits + step - 1) // step * step
    return kper, (M + kper - 1) // kper


def _wgrad_tiles(N, K):
    """(output tiles, workgroups of one resident round) of a weight gradient dW[N,K]: ceil(N / 128) * ceil(K / 128) tiles of
    128 x 128 at 3 workgroups per CU, or, for N <= 64, one row of 64 x 128 tiles at 4 per CU."""
    if N <= 64:
        return -(-K // 128), 1024
    return -(-N // 128) * -(-K // 128), 768


def _wgrad_split_rule(M, N, K, step, slots, max_ranges):
    """Number of row ranges of the weight gradient dW[N,K] = dY[M,N]^T x[M,K] (pure host rule, ``_split_k``'s): the output has
    only ``_wgrad_tiles`` tiles, so the M rows are cut into as many ranges as keep tiles x ranges within ``slots`` workgroups,
    each at least ``_WGRAD_MIN_STEPS`` steps of ``step`` rows long, at most ``max_ranges`` of them.  The result is what the
    library will run: no range is empty."""
    if M <= 0:
        return 1
    want = max(1, min(-(-M // step) // _WGRAD_MIN_STEPS, slots // _wgrad_tiles(N, K)[0], max_ranges, 65535))
    return _wgrad_ranges(M, want, step)[1]


def _wgrad_splits(M, N, K):
    """The rule for ``dfx_gemm_wgrad_f32``: 16-row steps, one resident round of workgroups, ``_WGRAD_MAX_RANGES``."""
    return _wgrad_split_rule(M, N, K, 16, _wgrad_tiles(N, K)[1], _WGRAD_MAX_RANGES)


def _wgrad_bf16_ranges(M, splits):
    return _wgrad_ranges(M, splits, 32)


def _wgrad_bf16_splits(M, N, K):
    """The rule for ``dfx_gemm_bf16_wgrad``: 32-row steps and the constants measured for it."""
    return _wgrad_split_rule(M, N, K, 32, _WGRAD_BF16_SLOTS, _WGRAD_BF16_MAX_RANGES)


def _linear_wgrad(what, entry, rule, go, x2, need_w, need_b, splits):
    """-> (grad_w | None, grad_b | None) of go [M,N] and x2 [M,K] from one call of ``entry`` (``rule(M, N, K)`` row ranges, or
    ``splits``); without a weight gradient no launch of it: a bias gradient on its own is ``go.sum(0)`` of the library."""
    (M, N), K, dev = go.shape, x2.shape[1], x2.device
    grad_w = grad_b = None
    if need_w:
        grad_w = torch.empty((N, K), dtype=torch.float32, device=dev)
        grad_b = torch.empty((N,), dtype=torch.float32, device=dev) if need_b else None
        n = rule(M, N, K) if splits is None else int(splits)
        ws = torch.empty((n * (N * K + N),), dtype=torch.float32, device=dev) if n > 1 else None
        _call(what + " (grad_w)", entry, dev, go.data_ptr(), N, x2.data_ptr(), K, grad_w.data_ptr(), K, _ptr(grad_b), M, N, K, n, _ptr(ws))
    elif need_b:
        grad_b = go.sum(0)
    return grad_w, grad_b


def linear_backward(grad_out, x, weight, need_x=True, need_w=True, need_b=True, splits=None):
    """Gradients of ``y = linear(x, weight, bias)``: -> (grad_x | None, grad_w | None, grad_b | None), fp32, fresh tensors.
    grad_out [..., N], x [..., K] contiguous, weight [N, K]; N and K multiples of 4.
    grad_x = grad_out @ weight is ``dfx_gemm_f32`` with the weight as its [K,N] operand, in the row ranges ``linear`` uses for
    operands of 2 GiB and more.  grad_w = grad_out^T @ x and grad_b = grad_out.sum(0) come from one ``dfx_gemm_wgrad_f32``
    call (split over the rows by ``_wgrad_splits``, or ``splits``; partial sums are added in a fixed order: two calls give
    the same bits).  ``need_w=False`` makes no weight-gradient launch; a bias gradient on its own (rare: a frozen weight
    with a trained bias) is ``grad_out.sum(0)`` of the library."""
    N, K = weight.shape
    go, x2 = grad_out.reshape(-1, N), x.reshape(-1, K)
    M = go.shape[0]
    _check_inputs([("grad_out", go), ("x", x2), ("weight", weight)])
    _require(go.dtype == torch.float32 and x2.dtype == torch.float32 and weight.dtype == torch.float32,
             "linear_backward is implemented for float32")
    _require(x2.shape[0] == M and N % 4 == 0 and K % 4 == 0, "linear_backward: grad_out [M,N], x [M,K] with N and K multiples of 4")
    dev = x.device
    grad_x = None
    if need_x:
        grad_x = torch.empty(x.shape, dtype=torch.float32, device=dev)
        for r0, r1 in _row_ranges(M, 4 * max(N, K)):
            _gemm_f32("linear_backward (grad_x)", dev, go.data_ptr() + r0 * N * 4, weight.data_ptr(), grad_x.data_ptr() + r0 * K * 4,
                      r1 - r0, K, N, N, K, K, b_is_kn=1)
    return (grad_x,) + _linear_wgrad("linear_backward", "dfx_gemm_wgrad_f32", _wgrad_splits, go, x2, need_w, need_b, splits)


# The node's forward is the function above, bound here: what a module calls by name (``ops.linear``, ``ops.linear_train``) is
# its route and can be wrapped or recorded as such; the product inside the autograd node is not a route of its own.
_linear_forward = linear


def _node_backward(backward, ctx, grad_output):
    """the backward of both Linear nodes: (x, the weight operand) were saved; gradients for exactly the inputs that ask"""
    x, weight = ctx.saved_tensors
    need = ctx.needs_input_grad
    return backward(grad_output.contiguous(), x, weight, need_x=need[0], need_w=need[1], need_b=need[2])


class _LinearFunction(torch.autograd.Function):
    """apply(x, weight, bias | None): saves the contiguous x and the weight, as nn.Linear does."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return _linear_forward(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return _node_backward(linear_backward, ctx, grad_output)      # (looked up at call time: tests wrap it)


def linear_train(x, weight, bias=None):
    """``linear(x, weight, bias)`` that trains: with grad mode on and x, weight or bias requiring a gradient the result carries
    it back through ``linear_backward`` - computed for exactly the inputs that ask for one; otherwise no autograd node is
    made.  Either way the forward is ``linear`` itself (the same bits).  N and K multiples of 4."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        _require(weight.shape[0] % 4 == 0 and weight.shape[1] % 4 == 0, "linear_train: N and K must be multiples of 4")
        return _LinearFunction.apply(x.contiguous(), weight, bias)
    return linear(x, weight, bias)


# ---- Linear in grad mode on bf16 products (include/dfx_gemm_bf16.h, dfx_gemm_bf16_wgrad; csrc/gemm_bf16_wgrad.hip) ----------------
def linear_bf16_backward(grad_out, x, weight_t_bf16, need_x=True, need_w=True, need_b=True, splits=None):
    """Gradients of ``y = linear_bf16(x, weight_bf16, bias)`` on bf16 products with fp32 accumulation:
    -> (grad_x | None, grad_w | None, grad_b | None), fp32, fresh tensors.
    grad_out [..., N] and x [..., K] fp32 contiguous; weight_t_bf16 [K, N] bf16 contiguous, the transpose of the layer's bf16
    weight; N and K multiples of 8.
    grad_x = grad_out @ W is ``linear_bf16(grad_out, weight_t_bf16)``: the forward kernel with the transposed copy as its
    [N', K'] operand, grad_out rounded to bf16 while it is staged, in ``linear_bf16``'s row ranges.  grad_w = grad_out^T @ x
    (both rounded to bf16 while they are staged) and grad_b = grad_out.sum(0) (of the unrounded values) come from one
    ``dfx_gemm_bf16_wgrad`` call, split over the rows by ``_wgrad_bf16_splits`` or ``splits``; partial sums are added in a fixed
    order: two calls give the same bits.  ``need_w=False`` makes no weight-gradient launch; a bias gradient on its own is
    ``grad_out.sum(0)`` of the library."""
    _require(weight_t_bf16.dim() == 2, "linear_bf16_backward: weight_t_bf16 must be [K, N]")
    K, N = weight_t_bf16.shape
    _require(weight_t_bf16.dtype == torch.bfloat16, "linear_bf16_backward: the transposed weight copy must be bfloat16")
    _require(grad_out.dtype == torch.float32 and x.dtype == torch.float32, "linear_bf16_backward: grad_out and x must be float32")
    _require(N % 8 == 0 and K % 8 == 0 and N > 0 and K > 0, "linear_bf16_backward: N and K must be multiples of 8")
    _require(grad_out.shape[-1] == N and x.shape[-1] == K, "linear_bf16_backward: grad_out [M,N], x [M,K], weight_t_bf16 [K,N]")
    go, x2 = grad_out.reshape(-1, N), x.reshape(-1, K)
    _require(x2.shape[0] == go.shape[0], "linear_bf16_backward: grad_out and x must have the same rows")
    _check_inputs([("grad_out", go), ("x", x2), ("weight_t_bf16", weight_t_bf16)])
    grad_x = linear_bf16(go, weight_t_bf16).reshape(x.shape) if need_x else None
    return (grad_x,) + _linear_wgrad("linear_bf16_backward", "dfx_gemm_bf16_wgrad", _wgrad_bf16_splits, go, x2, need_w, need_b, splits)


_linear_bf16_forward = linear_bf16      # (bound for the node, as ``_linear_forward`` is)


class _LinearBf16Function(torch.autograd.Function):
    """apply(x, weight, bias | None, weight_bf16, weight_t_bf16): saves the contiguous fp32 x and the transposed bf16 copy.
    ``weight`` is an input only to receive its gradient; the products read the two bf16 copies."""

    @staticmethod
    def forward(ctx, x, weight, bias, weight_bf16, weight_t_bf16):
        ctx.save_for_backward(x, weight_t_bf16)
        return _linear_bf16_forward(x, weight_bf16, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return _node_backward(linear_bf16_backward, ctx, grad_output) + (None, None)      # (looked up at call time: tests wrap it)


def linear_bf16_train(x, weight, bias, weight_bf16, weight_t_bf16):
    """``linear_bf16(x, weight_bf16, bias)`` (fp32 in, fp32 out) that trains ``weight`` [N, K] fp32, of which ``weight_bf16``
    [N, K] and ``weight_t_bf16`` [K, N] are the caller's bf16 copies (models.fused.bf16_weight_pair): with grad mode on and x,
    weight or bias requiring a gradient the result carries it back through ``linear_bf16_backward`` - computed for exactly the
    inputs that ask for one, the weight's as fp32 in ``weight``'s shape; otherwise no autograd node is made.  Either way the
    forward is ``linear_bf16`` itself (the same bits).  N and K multiples of 8."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        N, K = weight.shape
        _require(N % 8 == 0 and K % 8 == 0, "linear_bf16_train: N and K must be multiples of 8")
        _require(weight_bf16.shape == (N, K) and weight_t_bf16.shape == (K, N) and weight_t_bf16.dtype == torch.bfloat16
                 and weight_t_bf16.is_contiguous(), "linear_bf16_train: weight_bf16 [N,K] and a contiguous bf16 weight_t_bf16 [K,N]")
        _require(x.dtype == torch.float32, "linear_bf16_train: x must be float32")
        return _LinearBf16Function.apply(x.contiguous(), weight, bias, weight_bf16, weight_t_bf16)
    return linear_bf16(x, weight_bf16, bias)


def conv1x1(x, weight, bias=None, residual=None, relu=False, stride=1):
    """1x1 convolution on NCHW as a batched GEMM W[Co,Ci] x X_n[Ci,HW] with the folded-BN bias,
    the residual add and ReLU fused into the epilogue.  x [N,Ci,H,W], weight [Co,Ci(,1,1)]."""
    if stride != 1:
        x = x[:, :, ::stride, ::stride].contiguous()
    Nb, Ci, H, W = x.shape
    Co = weight.shape[0]
    w2 = weight.reshape(Co, -1)
    named = [("x", x), ("weight", w2)] + [(n, t) for n, t in (("bias", bias), ("residual", residual)) if t is not None]
    _check_inputs(named)
    _require(x.dtype == torch.float32 and w2.shape[1] == Ci, "conv1x1: fp32, weight [Co,Ci]")
    HW = H * W
    _require(Ci % 4 == 0 and HW % 4 == 0, "conv1x1 needs Ci and H*W to be multiples of 4")
    out = torch.empty((Nb, Co, H, W), dtype=x.dtype, device=x.device)
    if residual is not None:
        _require(residual.shape == out.shape, "residual must match the output")
    _gemm_f32("conv1x1", x.device, w2.data_ptr(), x.data_ptr(), out.data_ptr(), Co, HW, Ci, Ci, HW, HW, strideB=Ci * HW, b_is_kn=1,
              bias=_ptr(bias), bias_per_row=1, R=_ptr(residual), ldr=HW, strideR=Co * HW, strideC=Co * HW, batch=Nb,
              relu=int(bool(relu)))
    return out


# ---- 1x1 convolution in grad mode (include/dfx_gemm.h, dfx_conv1x1_wgrad_f32) -------------------------------------------------
# (bound here for the autograd node and its backward, as ``_linear_forward`` is: ``ops.conv1x1`` by name is a module's route)
_conv1x1_forward = conv1x1


def _conv1x1_wgrad_splits(Co, Ci, HW, batch):
    """Pixel ranges per image of the weight gradient dW[Co,Ci] = sum_n dZ[n] X[n]^T (pure host rule, ``_wgrad_splits``' with the
    images as a second source of workgroups): ``_wgrad_tiles`` x images x ranges stay within one resident round of workgroups,
    a range is at least ``_WGRAD_MIN_STEPS`` 16-deep steps long and images x ranges stay within ``_WGRAD_MAX_RANGES`` slabs.
    Both constants are taken over from ``_wgrad_splits`` as they are; they were measured for Linear layers and not re-tuned
    for this product.  The result is what the library will run: no range is empty."""
    if HW <= 0 or batch <= 0:
        return 1
    tiles, slots = _wgrad_tiles(Co, Ci)
    want = max(1, min(-(-HW // 16) // _WGRAD_MIN_STEPS, slots // (tiles * batch), _WGRAD_MAX_RANGES // batch))
    return _wgrad_ranges(HW, want)[1]


def conv1x1_backward(grad_out, x, weight, need_x=True, need_w=True, need_b=True, splits=None):
    """Gradients of ``y = conv1x1(x, weight, bias)``: -> (grad_x | None, grad_w | None, grad_b | None), fp32, fresh tensors.
    grad_out [N,Co,H,W] and x [N,Ci,H,W] contiguous, weight [Co,Ci(,1,1)]; Co, Ci and H*W multiples of 4.
    grad_x[n] = weight^T x grad_out[n] is ``dfx_gemm_f32`` with ``weight.t().contiguous()`` as A and grad_out as the [K,N]
    operand of every image.  grad_w comes from ``dfx_conv1x1_wgrad_f32`` (``_conv1x1_wgrad_splits`` pixel ranges per image, or
    ``splits``; the slabs are added in ascending (image, range) order: two calls give the same bits) and has weight's shape.
    grad_b = grad_out.sum((0, 2, 3)) is the library's reduction: the product kernel stages grad_out in its A operand's
    K-contiguous layout, where a column sum would cost the flagship GEMM registers it has none to spare."""
    Nb, Ci, H, W = x.shape
    Co, HW = weight.shape[0], H * W
    w2 = weight.reshape(Co, -1)
    _check_inputs([("grad_out", grad_out), ("x", x), ("weight", w2)])
    _require(grad_out.dtype == torch.float32 and x.dtype == torch.float32 and w2.dtype == torch.float32,
             "conv1x1_backward is implemented for float32")
    _require(grad_out.shape == (Nb, Co, H, W) and w2.shape[1] == Ci and Co % 4 == 0 and Ci % 4 == 0 and HW % 4 == 0,
             "conv1x1_backward: grad_out [N,Co,H,W], x [N,Ci,H,W] with Co, Ci and H*W multiples of 4")
    dev = x.device
    grad_x = grad_w = grad_b = None
    if need_x:
        grad_x = _conv1x1_forward(grad_out, w2.t().contiguous())
    if need_w:
        grad_w = torch.empty(weight.shape, dtype=torch.float32, device=dev)
        if Nb * HW == 0:
            grad_w.zero_()
        else:
            n = _conv1x1_wgrad_splits(Co, Ci, HW, Nb) if splits is None else _wgrad_ranges(HW, max(1, int(splits)))[1]
            ws = torch.empty((Nb * n * Co * Ci,), dtype=torch.float32, device=dev) if Nb * n > 1 else None
            _call("conv1x1_backward (grad_w)", "dfx_conv1x1_wgrad_f32", dev, grad_out.data_ptr(), Co * HW, x.data_ptr(), Ci * HW,
                  grad_w.data_ptr(), Co, Ci, HW, Nb, n, _ptr(ws))
    if need_b:
        grad_b = grad_out.sum((0, 2, 3))
    return grad_x, grad_w, grad_b


class _Conv1x1Function(torch.autograd.Function):
    """apply(x, weight, bias | None): saves the contiguous x and the weight, as nn.Conv2d does."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return _conv1x1_forward(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        # (looked up at call time: tests wrap it)
        return conv1x1_backward(grad_output.contiguous(), x, weight, need_x=need[0], need_w=need[1], need_b=need[2])


def conv1x1_train(x, weight, bias=None):
    """``conv1x1(x, weight, bias)`` that trains: with grad mode on and x, weight or bias requiring a gradient the result
    carries it back through ``conv1x1_backward`` - computed for exactly the inputs that ask for one; otherwise no autograd
    node is made.  Either way the forward is ``conv1x1`` itself (the same bits).  Co, Ci and H*W multiples of 4."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        _require(weight.shape[0] % 4 == 0, "conv1x1_train: Co must be a multiple of 4")
        return _Conv1x1Function.apply(x.contiguous(), weight, bias)
    return conv1x1(x, weight, bias)


def conv1x1_pair(x1, x2, weight, bias=None, relu=False):
    """relu?(weight x [x1 ; x2] + bias): two NCHW inputs of one map size concatenated along the channels inside the
    product (include/dfx_gemm.h, dfx_conv1x1_pair_f32) - a bottleneck's last 1x1 convolution and its stride-1
    projection shortcut in one GEMM.  x1 [N,K1,H,W], x2 [N,K2,H,W], weight [Co,K1+K2] -> [N,Co,H,W]."""
    _check_inputs([("x1", x1), ("x2", x2), ("weight", weight)] + ([("bias", bias)] if bias is not None else []))
    Nb, K1, H, W = x1.shape
    K2 = x2.shape[1]
    Co = weight.shape[0]
    _require(x1.dtype == torch.float32 and x2.shape == (Nb, K2, H, W) and weight.shape == (Co, K1 + K2),
             "conv1x1_pair: x1 [N,K1,H,W], x2 [N,K2,H,W], weight [Co,K1+K2], fp32")
    out = torch.empty((Nb, Co, H, W), dtype=x1.dtype, device=x1.device)
    _call("conv1x1_pair", "dfx_conv1x1_pair_f32", x1.device, weight.data_ptr(), x1.data_ptr(), K1 * H * W, K1, x2.data_ptr(),
          K2 * H * W, K2, _ptr(bias), out.data_ptr(), Co * H * W, Co, H * W, Nb, int(bool(relu)))
    return out


def conv1x1_chain_supported(Co, K1, K2, C1, HW):
    """Shapes dfx_conv1x1_chain_f32 covers (include/dfx_gemm.h): a wave keeps its [K, 32] activation panel and its
    [C1, 32] accumulators in registers."""
    K = K1 + K2
    return (Co > 0 and Co % 32 == 0 and C1 > 0 and C1 % 32 == 0 and K % 32 == 0 and K1 % 16 == 0 and K2 % 16 == 0 and
            K <= 128 and C1 <= 256 and HW % 4 == 0 and max(Co, 256) * HW * 4 < (1 << 31))


def conv1x1_chain(x, w3, b3, w1, b1, residual=None, x2=None, relu_z=True):
    """A bottleneck's last 1x1 convolution and the next block's first one as one launch (include/dfx_gemm.h,
    dfx_conv1x1_chain_f32):  y = relu(w3 x [x ; x2] + b3 + residual),  z = relu_z?(w1 x y + b1)  ->  (y, z).
    x [N,K1,H,W], x2 [N,K2,H,W] or None, w3 [Co,K1+K2], w1 [C1,Co], residual [N,Co,H,W] or None.
    A shape the fused kernel does not cover runs as the two separate launches (conv1x1 / conv1x1_pair, then conv1x1):
    the results are the same bit for bit."""
    Nb, K1, H, W = x.shape
    K2 = 0 if x2 is None else x2.shape[1]
    Co, C1, HW = w3.shape[0], w1.shape[0], H * W
    w3, w1 = w3.reshape(Co, -1), w1.reshape(C1, -1)
    named = [("x", x), ("w3", w3), ("w1", w1)] + [(n, t) for n, t in (("x2", x2), ("b3", b3), ("b1", b1), ("residual", residual))
                                                  if t is not None]
    _check_inputs(named)
    _require(x.dtype == torch.float32 and w3.shape[1] == K1 + K2 and w1.shape[1] == Co and
             (x2 is None or x2.shape == (Nb, K2, H, W)), "conv1x1_chain: fp32, w3 [Co,K1+K2], w1 [C1,Co], x2 [N,K2,H,W]")
    _require(x2 is None or residual is None, "conv1x1_chain: the two-segment form takes no residual")
    if residual is not None:
        _require(residual.shape == (Nb, Co, H, W), "residual must match the output")
    if not conv1x1_chain_supported(Co, K1, K2, C1, HW) or Nb == 0:
        y = (conv1x1(x, w3, b3, residual=residual, relu=True) if x2 is None else conv1x1_pair(x, x2, w3, b3, relu=True))
        return y, conv1x1(y, w1, b1, relu=relu_z)
    y = torch.empty((Nb, Co, H, W), dtype=x.dtype, device=x.device)
    z = torch.empty((Nb, C1, H, W), dtype=x.dtype, device=x.device)
    _call("conv1x1_chain", "dfx_conv1x1_chain_f32", x.device, w3.data_ptr(), x.data_ptr(), K1 * HW, K1, _ptr(x2), K2 * HW, K2,
          _ptr(b3), _ptr(residual), Co * HW, y.data_ptr(), Co * HW, w1.data_ptr(), _ptr(b1), z.data_ptr(), C1 * HW, Co, C1, HW,
          Nb, int(bool(relu_z)))
    return y, z


def _dynamic_conv_checks(feats, params, norm1, norm2):
    _check_inputs([("feats", feats), ("norm1.weight", norm1.weight), ("norm2.weight", norm2.weight)])
    K, R, C = feats.shape
    dd = norm1.normalized_shape[0]
    _require(params.is_cuda and params.dim() == 2 and params.shape[0] == K and params.stride(1) == 1
             and params.shape[1] >= 2 * C * dd and params.dtype == torch.float32 and feats.dtype == torch.float32,
             "dynamic_conv: params must be [K, 2*C*dd] fp32 with contiguous rows")
    _require(norm2.normalized_shape[0] == C and norm1.eps == norm2.eps, "dynamic_conv: norm shapes / eps")
    return K, R, C, dd


def _dynamic_conv_forward(feats, params, norm1, norm2):
    """The forward entry of include/dfx_roi.h (dfx_dynamic_conv_f32); no autograd node."""
    K, R, C, dd = _dynamic_conv_checks(feats, params, norm1, norm2)
    out = torch.empty_like(feats)
    _call("dynamic_conv", "dfx_dynamic_conv_f32", feats.device, feats.data_ptr(), params.data_ptr(), params.stride(0),
          norm1.weight.data_ptr(), norm1.bias.data_ptr(), norm2.weight.data_ptr(), norm2.bias.data_ptr(), out.data_ptr(),
          K, R, C, dd, float(norm1.eps))
    return out


DYNCONV_BWD_WS_FLOATS = _C["DFX_DYNCONV_BWD_WS_FLOATS"]


def dynamic_conv_backward(grad_out, feats, params, norm1, norm2, need_feats=True, need_params=True):
    """Gradients of dynamic_conv from its inputs alone (include/dfx_roi.h, dfx_dynamic_conv_backward_f32: the kernel
    recomputes the intermediates).  grad_out [K,R,256] contiguous.
    -> (grad_feats [K,R,256] | None, grad_params like params (zeros beyond column 2*C*dd) | None,
        grad_norm1_weight, grad_norm1_bias, grad_norm2_weight, grad_norm2_bias)
    No atomics: two calls on the same inputs give the same bits."""
    K, R, C, dd = _dynamic_conv_checks(feats, params, norm1, norm2)
    _check_inputs([("grad_out", grad_out)])
    _require(grad_out.shape == feats.shape and grad_out.dtype == torch.float32 and grad_out.device == feats.device,
             "dynamic_conv_backward: grad_out must match feats")
    width = params.shape[1]
    grad_feats = torch.empty_like(feats) if need_feats else None
    grad_params = None
    pitch = (width + 3) // 4 * 4          # the kernel wants rows that start 16-byte aligned; the result is a column slice
    if need_params:       # the kernel writes columns 0 .. 2*C*dd of every row
        grad_params = (torch.empty if width == 2 * C * dd else torch.zeros)((K, pitch), dtype=torch.float32, device=feats.device)
    grad_ln = torch.empty(2 * dd + 2 * C, dtype=torch.float32, device=feats.device)
    ws = torch.empty(DYNCONV_BWD_WS_FLOATS, dtype=torch.float32, device=feats.device)
    _call("dynamic_conv_backward", "dfx_dynamic_conv_backward_f32", feats.device,
          grad_out.data_ptr(), feats.data_ptr(), params.data_ptr(), params.stride(0), norm1.weight.data_ptr(),
          norm1.bias.data_ptr(), norm2.weight.data_ptr(), norm2.bias.data_ptr(), _ptr(grad_feats), _ptr(grad_params), pitch,
          grad_ln.data_ptr(), ws.data_ptr(), K, R, C, dd, float(norm1.eps))
    dg1, db1, dg2, db2 = grad_ln.split([dd, dd, C, C])
    if grad_params is not None and pitch != width:
        grad_params = grad_params[:, :width]
    return grad_feats, grad_params, dg1, db1, dg2, db2


class _NormView:
    """What the entry points read of an nn.LayerNorm, over saved tensors."""

    def __init__(self, weight, bias, eps):
        self.weight, self.bias, self.eps, self.normalized_shape = weight, bias, eps, tuple(weight.shape)


class _DynamicConvFunction(torch.autograd.Function):
    """apply(feats, params, g1, b1, g2, b2, eps): saves its inputs only; the backward kernel recomputes the rest."""

    @staticmethod
    def forward(ctx, feats, params, g1, b1, g2, b2, eps):
        ctx.eps = eps
        ctx.save_for_backward(feats, params, g1, b1, g2, b2)
        return _dynamic_conv_forward(feats, params, _NormView(g1, b1, eps), _NormView(g2, b2, eps))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        feats, params, g1, b1, g2, b2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        gf, gp, dg1, db1, dg2, db2 = dynamic_conv_backward(grad_output.contiguous(), feats, params, _NormView(g1, b1, ctx.eps),
                                                           _NormView(g2, b2, ctx.eps), need_feats=need[0], need_params=need[1])
        return (gf, gp, dg1 if need[2] else None, db1 if need[3] else None, dg2 if need[4] else None,
                db2 if need[5] else None, None)


def dynamic_conv(feats, params, norm1, norm2):
    """relu(norm2(relu(norm1(feats @ k1)) @ k2)) per RoI with k1, k2 cut from ``params`` (include/dfx_roi.h,
    dfx_dynamic_conv_f32): feats [K,R,256] contiguous, params [K, 2*256*64] (rows may be strided), norm1 / norm2
    nn.LayerNorm(64) / nn.LayerNorm(256).  -> [K,R,256]
    With grad mode on and feats, params or a LayerNorm parameter requiring a gradient the result carries it back
    through dynamic_conv_backward; otherwise no autograd node is made."""
    if torch.is_grad_enabled() and (feats.requires_grad or params.requires_grad or norm1.weight.requires_grad
                                    or norm1.bias.requires_grad or norm2.weight.requires_grad or norm2.bias.requires_grad):
        _dynamic_conv_checks(feats, params, norm1, norm2)
        return _DynamicConvFunction.apply(feats, params, norm1.weight, norm1.bias, norm2.weight, norm2.bias, float(norm1.eps))
    return _dynamic_conv_forward(feats, params, norm1, norm2)


def _mha_checks(q, k, v, heads):
    for nm, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda:
            raise RuntimeError(f"{nm} must be a CUDA tensor (the fused attention has no CPU path)")
        _require(t.dim() == 3 and t.dtype == torch.float32 and t.stride(2) == 1 and t.shape[2] == 32 * heads,
                 f"mha: {nm} must be [B,L,32*heads] fp32 with a contiguous last dimension")
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _require(k.shape == (B, Lk, E) and v.shape == (B, Lk, E), "mha: k and v must be [B,Lk,E]")
    return B, Lq, Lk, E


def _mha_drop(drop, q, B, heads, Lq, Lk):
    """data pointer of the dropout mask ([B,heads,Lq,Lk] or [B*heads,Lq,Lk], contiguous fp32), None without one"""
    if drop is None:
        return None
    _require(drop.is_cuda and drop.device == q.device and drop.dtype == torch.float32 and drop.is_contiguous()
             and tuple(drop.shape) in ((B, heads, Lq, Lk), (B * heads, Lq, Lk)),
             "mha: drop must be a contiguous fp32 [B,heads,Lq,Lk] (or [B*heads,Lq,Lk]) tensor on q's device")
    return drop.data_ptr()


def _strided(t):
    return (t.data_ptr(), t.stride(0), t.stride(1))


def mha_train_forward(q, k, v, heads, scale, drop=None):
    """The attention with what its backward needs (include/dfx_mha.h, dfx_mha_train_forward_f32): -> (out [B,Lq,E],
    lse [B,heads,Lq] = ln sum_j exp(scale <q_i,k_j>)).  drop (0 or 1/(1-p)) multiplies the normalised probabilities.
    No autograd node; without ``drop`` the output has the bits of the inference entry."""
    B, Lq, Lk, E = _mha_checks(q, k, v, heads)
    out = torch.empty((B, Lq, E), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, heads, Lq), dtype=torch.float32, device=q.device)
    _call("mha", "dfx_mha_train_forward_f32", q.device, *_strided(q), *_strided(k), *_strided(v), out.data_ptr(), Lq * E, E,
          lse.data_ptr(), _mha_drop(drop, q, B, heads, Lq, Lk), B, heads, Lq, Lk, float(scale))
    return out, lse


def mha_backward(grad_out, q, k, v, out, lse, heads, scale, drop=None, need_q=True, need_kv=True):
    """Gradients of ``mha`` (include/dfx_mha.h, dfx_mha_backward_f32) from its inputs, its output and ``lse`` of
    ``mha_train_forward``; the probabilities are recomputed.  -> (grad_q | None, grad_k | None, grad_v | None), each
    contiguous; grad_k and grad_v come together.  One launch without atomics: two calls give the same bits."""
    B, Lq, Lk, E = _mha_checks(q, k, v, heads)
    for nm, t in (("grad_out", grad_out), ("out", out)):
        _require(t.is_cuda and t.device == q.device and t.dtype == torch.float32 and tuple(t.shape) == (B, Lq, E)
                 and t.stride(2) == 1, f"mha_backward: {nm} must be [B,Lq,E] fp32 with a contiguous last dimension")
    _require(lse.is_cuda and lse.device == q.device and lse.dtype == torch.float32 and tuple(lse.shape) == (B, heads, Lq)
             and lse.is_contiguous(), "mha_backward: lse must be a contiguous fp32 [B,heads,Lq] tensor")
    grad_q = torch.empty((B, Lq, E), dtype=torch.float32, device=q.device) if need_q else None
    grad_k = torch.empty((B, Lk, E), dtype=torch.float32, device=q.device) if need_kv else None
    grad_v = torch.empty((B, Lk, E), dtype=torch.float32, device=q.device) if need_kv else None
    if need_q or need_kv:
        _call("mha_backward", "dfx_mha_backward_f32", q.device, *_strided(grad_out), *_strided(q), *_strided(k), *_strided(v),
              *_strided(out), lse.data_ptr(), _mha_drop(drop, q, B, heads, Lq, Lk), _ptr(grad_q), Lq * E, E, _ptr(grad_k),
              Lk * E, E, _ptr(grad_v), Lk * E, E, B, heads, Lq, Lk, float(scale))
    return grad_q, grad_k, grad_v


class _MhaFunction(torch.autograd.Function):
    """apply(q, k, v, drop, heads, scale): saves q, k, v, out, lse and the mask; nothing of size Lq x Lk but the mask."""

    @staticmethod
    def forward(ctx, q, k, v, drop, heads, scale):
        out, lse = mha_train_forward(q, k, v, heads, scale, drop)
        ctx.heads, ctx.scale = heads, scale
        ctx.save_for_backward(q, k, v, out, lse, drop)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        q, k, v, out, lse, drop = ctx.saved_tensors
        need = ctx.needs_input_grad
        gq, gk, gv = mha_backward(grad_output.contiguous(), q, k, v, out, lse, ctx.heads, ctx.scale, drop, need_q=need[0],
                                  need_kv=need[1] or need[2])
        return gq, gk if need[1] else None, gv if need[2] else None, None, None, None


def mha(q, k, v, heads, scale, drop=None):
    """softmax(scale * q k^T) v per head (include/dfx_mha.h): q [B,Lq,E], k / v [B,Lk,E], E = 32*heads, fp32.
    The tensors may be column slices of a joint projection (last dimension contiguous).  -> [B,Lq,E]
    drop [B,heads,Lq,Lk] (0 or 1/(1-p)): attention dropout, multiplies the normalised probabilities.
    With grad mode on and q, k or v requiring a gradient the result carries it back through ``mha_backward``; otherwise
    no autograd node is made and, without a mask, the call is the inference entry dfx_mha_f32."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        _mha_checks(q, k, v, heads)
        return _MhaFunction.apply(q, k, v, drop, heads, float(scale))
    if drop is not None:
        return mha_train_forward(q, k, v, heads, scale, drop)[0]
    B, Lq, Lk, E = _mha_checks(q, k, v, heads)
    out = torch.empty((B, Lq, E), dtype=torch.float32, device=q.device)
    _call("mha", "dfx_mha_f32", q.device, q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
          v.data_ptr(), v.stride(0), v.stride(1), out.data_ptr(), Lq * E, E, B, heads, Lq, Lk, float(scale))
    return out


def box_refine(delta, reference, eps=1e-5):
    """sigmoid(delta + inverse_sigmoid(reference)) on the first reference.shape[-1] (2 or 4) of the 4 box
    columns, sigmoid(delta) on the others, in one launch (include/dfx_fused.h).  delta [...,4]."""
    delta, reference = delta.contiguous(), reference.contiguous()
    _check_inputs([("delta", delta), ("reference", reference)])
    rd = reference.shape[-1]
    _require(delta.shape[-1] == 4 and rd in (2, 4) and delta.shape[:-1] == reference.shape[:-1]
             and delta.dtype == torch.float32 and reference.dtype == torch.float32,
             "box_refine: delta [...,4], reference [...,2|4], fp32")
    out = torch.empty_like(delta)
    _call("box_refine", "dfx_box_refine_f32", delta.device, delta.data_ptr(), reference.data_ptr(), rd, out.data_ptr(),
          delta.numel() // 4, float(eps))
    return out


def add_layernorm(x, residual, norm):
    """``norm(x + residual)`` for an nn.LayerNorm over the last dimension, in one pass
    (include/dfx_fused.h); residual may be None."""
    C = x.shape[-1]
    x2 = x.contiguous()
    named = [("x", x2), ("weight", norm.weight), ("bias", norm.bias)]
    if residual is not None:
        residual = residual.contiguous()
        named.append(("residual", residual))
        _require(residual.shape == x2.shape, "residual must match x")
    _check_inputs(named)
    _require(x2.dtype == torch.float32 and norm.weight.numel() == C, "add_layernorm: fp32, LayerNorm over the last dim")
    out = torch.empty_like(x2)
    _call("add_layernorm", "dfx_add_layernorm_f32", x2.device, x2.data_ptr(), _ptr(residual), norm.weight.data_ptr(),
          norm.bias.data_ptr(), out.data_ptr(), x2.numel() // C, C, float(norm.eps))
    return out


ADDLN_BWD_ROWS_PER_BLOCK, ADDLN_BWD_MAX_GRID = _C["DFX_ADDLN_BWD_ROWS_PER_BLOCK"], _C["DFX_ADDLN_BWD_MAX_GRID"]


def add_layernorm_backward_grid(rows):
    """Workgroups of the backward launch = rows of its workspace (DFX_ADDLN_BWD_GRID): a function of ``rows`` alone."""
    return min((rows + ADDLN_BWD_ROWS_PER_BLOCK - 1) // ADDLN_BWD_ROWS_PER_BLOCK, ADDLN_BWD_MAX_GRID)


def _addln_rows(what, x, C):
    _require(x.dim() >= 1 and x.dtype == torch.float32 and x.shape[-1] == C and C % 4 == 0 and 0 < C <= 1024,
             f"{what}: fp32 rows of C columns, C a multiple of 4 and <= 1024")
    return x.numel() // C


def add_layernorm_train_forward(x, residual, weight, bias, eps, mask=None):
    """``LayerNorm(residual + x * mask)`` with what its backward reads (include/dfx_fused.h, dfx_add_layernorm_train_f32):
    -> (out, s, mean, rstd, keep).  s = residual + x * mask, fp32 like x; mean, rstd [rows]; keep uint8 like x, 1 where
    mask != 0, None without a mask.  residual and mask (fp32, x's shape, 0 or 1/(1-p)) may be None.  No autograd node.
    Without a mask ``out`` has the bits of ``add_layernorm``, with one those of ``add_layernorm(x * mask, residual)``."""
    C = weight.numel()
    x2 = x.contiguous()
    named = [("x", x2), ("weight", weight), ("bias", bias)]
    for nm, t in (("residual", residual), ("mask", mask)):
        if t is not None:
            _require(t.shape == x.shape and t.dtype == torch.float32, f"add_layernorm_train: {nm} must match x")
            named.append((nm, t.contiguous()))
    _check_inputs(named)
    rows = _addln_rows("add_layernorm_train", x2, C)
    _require(weight.dtype == torch.float32 and bias.dtype == torch.float32 and bias.numel() == C,
             "add_layernorm_train: fp32 weight and bias of C elements")
    residual, mask = (dict(named).get(nm) for nm in ("residual", "mask"))
    out, s = torch.empty_like(x2), torch.empty_like(x2)
    mean = torch.empty((rows,), dtype=torch.float32, device=x2.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x2.device)
    keep = None if mask is None else torch.empty(x2.shape, dtype=torch.uint8, device=x2.device)
    _call("add_layernorm_train", "dfx_add_layernorm_train_f32", x2.device, x2.data_ptr(), _ptr(residual), _ptr(mask),
          weight.data_ptr(), bias.data_ptr(), out.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(keep),
          rows, C, float(eps))
    return out, s, mean, rstd, keep


def add_layernorm_backward(grad_out, s, mean, rstd, weight, keep=None, scale=1.0, need_x=True, need_residual=True,
                           need_gamma=True, need_beta=True):
    """Gradients of ``add_layernorm_train_forward`` (include/dfx_fused.h, dfx_add_layernorm_backward_f32) ->
    (grad_x | None, grad_residual | None, grad_gamma | None, grad_beta | None), fresh fp32 tensors; only what is asked
    for is computed.  Without ``keep`` grad_x and grad_residual are the same values and come back as ONE tensor.
    Two launches without atomics, sums in a fixed order: two calls give the same bits."""
    C = weight.numel()
    grad_out = grad_out.contiguous()
    named = [("grad_out", grad_out), ("s", s), ("mean", mean), ("rstd", rstd), ("weight", weight)]
    if keep is not None:
        named.append(("keep", keep))
        _require(keep.dtype == torch.uint8 and keep.shape == s.shape, "add_layernorm_backward: keep must be uint8 of s's shape")
    _check_inputs(named)
    rows = _addln_rows("add_layernorm_backward", s, C)
    _require(grad_out.dtype == torch.float32 and grad_out.shape == s.shape and weight.dtype == torch.float32
             and mean.dtype == torch.float32 and rstd.dtype == torch.float32 and mean.numel() == rows and rstd.numel() == rows,
             "add_layernorm_backward: fp32 grad_out of s's shape, mean and rstd of one element per row")
    dev = s.device
    shared = keep is None and need_x and need_residual
    grad_x = torch.empty_like(s) if need_x else None
    grad_res = grad_x if shared else torch.empty_like(s) if need_residual else None
    new = torch.zeros if rows == 0 else torch.empty
    grad_gamma = new((C,), dtype=torch.float32, device=dev) if need_gamma else None
    grad_beta = new((C,), dtype=torch.float32, device=dev) if need_beta else None
    if rows > 0 and (need_x or need_residual or need_gamma or need_beta):
        ws = (torch.empty((add_layernorm_backward_grid(rows), 2 * C), dtype=torch.float32, device=dev)
              if need_gamma or need_beta else None)
        _call("add_layernorm_backward", "dfx_add_layernorm_backward_f32", dev, grad_out.data_ptr(), s.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), weight.data_ptr(), _ptr(keep), float(scale), _ptr(grad_x), None if shared else _ptr(grad_res),
              _ptr(grad_gamma), _ptr(grad_beta), _ptr(ws), rows, C)
    return grad_x, grad_res, grad_gamma, grad_beta


class _AddLayerNormFunction(torch.autograd.Function):
    """apply(x, residual | None, weight, bias, mask | None, eps, scale): saves s, mean, rstd, the 1-byte keep mask and the
    weight - what the library's add + LayerNorm + dropout nodes save, and not the float mask."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, mask, eps, scale):
        out, s, mean, rstd, keep = add_layernorm_train_forward(x, residual, weight, bias, eps, mask)
        ctx.save_for_backward(s, mean, rstd, keep, weight)
        ctx.scale = scale
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        s, mean, rstd, keep, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        # (looked up at call time: tests wrap it)
        gx, gr, gg, gb = add_layernorm_backward(grad_output, s, mean, rstd, weight, keep, ctx.scale, need_x=need[0],
                                                need_residual=need[1], need_gamma=need[2], need_beta=need[3])
        return gx, gr, gg, gb, None, None, None


def add_layernorm_train(x, residual, norm, dropout=None):
    """``norm(residual + dropout(x))`` for an nn.LayerNorm over the last dimension - the tail of a transformer sub-layer -
    in one launch, with an autograd node whose backward is two (``add_layernorm_backward``); residual may be None.
    dropout: the sub-layer's nn.Dropout.  When it is live (training, p > 0) the mask is drawn as
    ``F.dropout(ones_like(x), p, True)`` right here, where the module would call ``F.dropout(x, p, True)``: the same shape
    from the same generator gives the same numbers (the rule of models.fused_mha.attention_dropout_mask), so under a fixed
    seed both routes drop the same elements and x * mask has the bits of the module's output.
    Without grad mode, or when neither x, residual nor the norm's parameters require a gradient, no node is made."""
    import torch.nn.functional as F
    _require(isinstance(norm, torch.nn.LayerNorm) and len(norm.normalized_shape) == 1 and norm.weight is not None
             and norm.bias is not None, "add_layernorm_train: an affine nn.LayerNorm over the last dimension")
    _require(residual is None or residual.shape == x.shape, "add_layernorm_train: residual must match x")
    _addln_rows("add_layernorm_train", x, norm.weight.numel())
    mask, scale = None, 1.0
    if dropout is not None and dropout.training and dropout.p > 0:
        mask = F.dropout(torch.ones_like(x), dropout.p, True)
        scale = 1.0 / (1.0 - dropout.p) if dropout.p < 1 else 0.0
    if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)
                                    or norm.weight.requires_grad or norm.bias.requires_grad):
        return _AddLayerNormFunction.apply(x, residual, norm.weight, norm.bias, mask, float(norm.eps), scale)
    return add_layernorm_train_forward(x, residual, norm.weight, norm.bias, norm.eps, mask)[0]


def bias_relu_maxpool(x, bias):
    """maxpool3x3/s2/p1(relu(x + bias[c])) on NCHW in one pass: the ResNet stem's epilogue
    (include/dfx_fused.h)."""
    _check_inputs([("x", x), ("bias", bias)])
    _require(x.dtype == torch.float32 and x.dim() == 4 and bias.numel() == x.shape[1], "bias_relu_maxpool: fp32 NCHW")
    N, C, H, W = x.shape
    out = torch.empty((N, C, (H + 1) // 2, (W + 1) // 2), dtype=x.dtype, device=x.device)
    _call("bias_relu_maxpool", "dfx_bias_relu_maxpool_f32", x.device, x.data_ptr(), bias.data_ptr(), out.data_ptr(), N, C, H, W)
    return out


def _conv_batch_ranges(algo, N, per_image, image_stride, limit):
    """The image ranges [(n0, n1), ...] of ConvPlan's launches for a batch of N images of ``per_image`` elements each
    (``image_stride`` apart when the input is a channel slice read in place, else 0).  Winograd: one launch while the batch
    stays below ``limit`` elements, else as many whole images as fit below it; the tile kernel: as many images as span at most
    ``limit`` elements; the implicit GEMM: one launch.  Always at least one image per launch; an empty batch launches nothing."""
    step = N
    if algo == "wino" and N * per_image >= limit:
        step = (limit - 1) // per_image
    if algo == "tile":
        step = min(N, limit // max(image_stride, per_image))
    step = max(1, step)
    return [(n0, min(N, n0 + step)) for n0 in range(0, N, step)]


class ConvPlan:
    """One convolution prepared for the hand-written kernels (include/dfx_conv.h): 3x3 / stride 1 / "same"
    convolutions with Ci % 8 == 0 and Co % 64 == 0 run as fused Winograd F(2x2, 3x3) (weights pre-transformed
    on the GPU by dfx_wino_weights_f32), convolutions of at most 4 input channels (the 7x7/2 ResNet stem, the first
    DFormer convolution) as a direct convolution from an LDS-resident input tile (algo "tile", csrc/conv_tile.hip),
    everything else as an implicit GEMM over a tap table (weights re-ordered [Co, (ky, kx, ci)], K padded to a
    multiple of 16; the tile kernel takes the same weights).  ``scale`` (per output channel, e.g. the
    folded FrozenBatchNorm2d factor) is multiplied into the weights; ``bias`` and ``act`` run in the epilogue.
    ``weight`` is [Co, Ci, kh, kw] of an ungrouped convolution with zero padding: callers hand over ``conv.groups`` /
    ``conv.padding_mode`` (or check them) - anything else raises."""
    WINO_MAX_ELEMENTS = 1 << 30      # input elements per Winograd launch (32-bit offsets in the kernel); more go in image ranges
    TILE_MAX_ELEMENTS = (1 << 30) - 4  # ... per tile-kernel launch, image strides included (32-bit byte offsets: below 4 GiB)

    def __init__(self, weight, bias=None, stride=1, padding=0, dilation=1, act=None, scale=None, algo=None, groups=1,
                 padding_mode="zeros"):
        _require(weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4, "ConvPlan: fp32 CUDA weight [Co,Ci,kh,kw]")
        for nm, v in (("stride", stride), ("padding", padding), ("dilation", dilation)):
            _require(not isinstance(v, (tuple, list)) or len(set(int(e) for e in v)) == 1,
                     f"ConvPlan: {nm} must be the same along both axes (got {tuple(v) if isinstance(v, (tuple, list)) else v})")
        stride, padding, dilation = (v[0] if isinstance(v, (tuple, list)) else v for v in (stride, padding, dilation))
        Co, Ci, kh, kw = weight.shape
        _require(groups == 1 and padding_mode == "zeros", "ConvPlan: grouped convolutions / non-zero padding modes are not covered")
        _require(kh <= 32 and kw <= 32, "ConvPlan: kernel sides up to 32")
        self.Co, self.Ci, self.kh, self.kw = Co, Ci, kh, kw
        self.stride, self.padding, self.dilation, self.act = int(stride), int(padding), int(dilation), ACT[act]
        self.bias = None if bias is None else bias.detach().float().contiguous()
        wino_ok = kh == 3 and kw == 3 and stride == 1 and padding == dilation and Ci % 8 == 0 and Co % 64 == 0
        tile_ok = bool(_lib.load().dfx_conv2d_tile_fits(Ci, Co, kh, kw, int(stride), int(dilation)))
        self.algo = algo or ("wino" if wino_ok else "tile" if (tile_ok and Ci <= 4 and USE_TILE_CONV) else "igemm")
        _require(self.algo != "wino" or wino_ok, "ConvPlan: geometry not covered by the Winograd kernel")
        _require(self.algo != "tile" or tile_ok, "ConvPlan: geometry not covered by the tile kernel")
        w = weight.detach().contiguous()
        if self.algo == "wino":
            self.u = torch.empty(16 * Co * Ci, dtype=torch.float32, device=w.device)
            sc = None if scale is None else scale.detach().float().contiguous()
            _call("wino_weights", "dfx_wino_weights_f32", w.device, w.data_ptr(), _ptr(sc), self.u.data_ptr(), Co, Ci)
        else:
            if scale is not None:
                w = w * scale.detach().reshape(-1, 1, 1, 1)
            K = kh * kw * Ci
            Kpad = (K + 15) // 16 * 16
            _require(kh * kw <= 64, "ConvPlan: at most 64 taps")
            wp = torch.zeros(Co, Kpad, dtype=torch.float32, device=w.device)
            wp[:, :K] = w.permute(0, 2, 3, 1).reshape(Co, K)
            self.wp, self.Kpad, self.K, self._tabs = wp, Kpad, K, {}

    def _ktab(self, H, W, device):
        """Tap table of the implicit GEMM for an H x W input (include/dfx_conv.h): per k {tap index, byte offset}."""
        key = (H, W, str(device))
        if key not in self._tabs:
            ky, kx, ci = torch.meshgrid(torch.arange(self.kh), torch.arange(self.kw), torch.arange(self.Ci), indexing="ij")
            tab = torch.zeros((self.Kpad, 2), dtype=torch.int32)
            tab[:, 0] = -1
            tab[:self.K, 0] = (ky * self.kw + kx).reshape(-1).to(torch.int32)
            tab[:self.K, 1] = ((ci * (H * W) + ky * self.dilation * W + kx * self.dilation) * 4).reshape(-1).to(torch.int32)
            self._tabs[key] = tab.to(device)
        return self._tabs[key]

    def out_size(self, H, W):
        eff_h, eff_w = (self.kh - 1) * self.dilation + 1, (self.kw - 1) * self.dilation + 1
        return (H + 2 * self.padding - eff_h) // self.stride + 1, (W + 2 * self.padding - eff_w) // self.stride + 1

    def __call__(self, x):
        _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.Ci,
                 "conv: x must be a CUDA fp32 tensor [N,Ci,H,W] (no CPU path)")
        N, _, H, W = x.shape
        # a channel slice of a wider NCHW tensor (x[:, :3] of an RGB-D clip) is read in place by the implicit GEMM
        sliced = (self.algo in ("igemm", "tile") and not x.is_contiguous() and x.stride(3) == 1 and x.stride(2) == W
                  and x.stride(1) == H * W and x.stride(0) >= self.Ci * H * W)
        image_stride = x.stride(0) if sliced else 0
        if not sliced:
            x = x.contiguous()
        Ho, Wo = self.out_size(H, W)
        y = torch.empty((N, self.Co, Ho, Wo), dtype=torch.float32, device=x.device)
        limit = {"wino": self.WINO_MAX_ELEMENTS, "tile": self.TILE_MAX_ELEMENTS}.get(self.algo)
        with _on(x.device):
            for n0, n1 in _conv_batch_ranges(self.algo, N, self.Ci * H * W, image_stride, limit):
                xs, ys = x[n0:n1], y[n0:n1]
                if self.algo == "wino":
                    _call("conv wino", "dfx_conv3x3_wino_f32", x.device, xs.data_ptr(), self.u.data_ptr(), _ptr(self.bias),
                          ys.data_ptr(), n1 - n0, self.Ci, H, W, self.Co, self.dilation, self.act)
                elif self.algo == "tile":
                    _call("conv tile", "dfx_conv2d_tile_f32", x.device, xs.data_ptr(), self.wp.data_ptr(), _ptr(self.bias),
                          ys.data_ptr(), n1 - n0, self.Ci, H, W, self.Co, Ho, Wo, self.Kpad, self.kh, self.kw, self.stride,
                          self.padding, self.act, image_stride)
                else:
                    _call("conv igemm", "dfx_conv2d_igemm_f32", x.device, xs.data_ptr(), self.wp.data_ptr(),
                          self._ktab(H, W, x.device).data_ptr(), _ptr(self.bias), ys.data_ptr(), n1 - n0, self.Ci, H, W, self.Co,
                          Ho, Wo, self.Kpad, self.kh, self.kw, self.stride, self.padding, self.dilation, self.act, image_stride)
        return y


def _group_norm_forward(x, weight, bias, groups, eps, tokens_out):
    """-> (y, stats): y [N,H*W,C] with tokens_out, else [N,C,H,W]; stats [N*groups*2] (mean, rstd) as the backward reads them"""
    _check_inputs([("x", x), ("weight", weight), ("bias", bias)])
    _require(x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == weight.numel(), "group_norm: fp32 NCHW")
    N, C, H, W = x.shape
    stats = torch.empty(N * groups * 2, dtype=torch.float32, device=x.device)
    y = torch.empty((N, H * W, C) if tokens_out else (N, C, H, W), dtype=torch.float32, device=x.device)
    _call("group_norm", "dfx_group_norm_f32", x.device, x.data_ptr(), weight.data_ptr(), bias.data_ptr(),
          stats.data_ptr(), y.data_ptr(), N, C, H * W, groups, float(eps), int(bool(tokens_out)))
    return y, stats


GN_BWD_CHUNKS = _C["DFX_GN_BWD_CHUNKS"]


def group_norm_backward(grad_out, x, stats, gamma, groups, tokens=False, need_x=True, need_gamma=True, need_beta=True):
    """Gradients of ``group_norm``: -> (grad_x | None, grad_gamma | None, grad_beta | None), fp32, fresh tensors
    (include/dfx_fused.h, dfx_group_norm_backward_f32: two streaming launches, no atomics, the same bits every call).
    x [N,C,H,W] contiguous, stats as the forward wrote them, gamma [C]; grad_out contiguous, [N,C,H,W] or - ``tokens`` -
    [N,H*W,C], the memory layout of the forward's tokens_out result: it is read as it lies, through an LDS transpose."""
    N, C, H, W = x.shape
    _check_inputs([("grad_out", grad_out), ("x", x), ("stats", stats), ("gamma", gamma)])
    _require(grad_out.dtype == torch.float32 and x.dtype == torch.float32 and gamma.numel() == C and C % groups == 0
             and stats.numel() == N * groups * 2, "group_norm_backward: fp32, gamma [C], stats [N*groups*2]")
    _require(tuple(grad_out.shape) == ((N, H * W, C) if tokens else (N, C, H, W)), "group_norm_backward: grad_out [N,H*W,C] (tokens) or [N,C,H,W]")
    dev = x.device
    new = torch.zeros if N * H * W == 0 else torch.empty
    grad_x = torch.empty_like(x) if need_x else None
    grad_gamma = new((C,), dtype=torch.float32, device=dev) if need_gamma else None
    grad_beta = new((C,), dtype=torch.float32, device=dev) if need_beta else None
    if N * H * W > 0 and (need_x or need_gamma or need_beta):
        ws = torch.empty((N * C * 2 * GN_BWD_CHUNKS,), dtype=torch.float32, device=dev)
        _call("group_norm_backward", "dfx_group_norm_backward_f32", dev, grad_out.data_ptr(), x.data_ptr(), stats.data_ptr(),
              gamma.data_ptr(), _ptr(grad_x), _ptr(grad_gamma), _ptr(grad_beta), ws.data_ptr(), N, C, H * W, groups, int(bool(tokens)))
    return grad_x, grad_gamma, grad_beta


class _GroupNormFunction(torch.autograd.Function):
    """apply(x, weight, bias, groups, eps, tokens_out) -> y as ``_group_norm_forward`` lays it out; saves x, stats and the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, tokens_out):
        y, stats = _group_norm_forward(x, weight, bias, groups, eps, tokens_out)
        ctx.save_for_backward(x, stats, weight)
        ctx.groups, ctx.tokens_out = groups, tokens_out
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, stats, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        # the kernel reads either layout as it lies: a gradient that is contiguous in the other one (token-major flowing back
        # into an NCHW result or the reverse) is handed over under that layout's flag, not copied
        N, C, H, W = x.shape
        g, tokens = grad_output, ctx.tokens_out
        if not g.is_contiguous():
            other = g.transpose(1, 2) if tokens else g.permute(0, 2, 3, 1)          # [N,C,H*W] / [N,H,W,C]
            if other.is_contiguous():
                g, tokens = other.reshape((N, C, H, W) if tokens else (N, H * W, C)), not tokens
            else:
                g = g.contiguous()
        # (looked up at call time: tests wrap it)
        gx, gg, gb = group_norm_backward(g, x, stats, weight, ctx.groups, tokens=tokens, need_x=need[0], need_gamma=need[1],
                                         need_beta=need[2])
        return gx, gg, gb, None, None, None


def group_norm(x, norm, tokens_out=False):
    """nn.GroupNorm ``norm`` applied to x [N,C,H,W] (contiguous NCHW) in two streaming launches
    (include/dfx_fused.h, dfx_group_norm_f32).  tokens_out: the result is written token-major [N,H*W,C] and
    returned as an NCHW-shaped VIEW of that memory, so ``y.flatten(2).transpose(1, 2)`` - what the transformer
    does next - is already contiguous and costs nothing.
    With grad mode on and x or a parameter of ``norm`` requiring a gradient the same forward runs under an autograd node
    whose backward is ``group_norm_backward`` (computed for exactly the inputs that ask); otherwise no node is made."""
    if torch.is_grad_enabled() and (x.requires_grad or norm.weight.requires_grad or norm.bias.requires_grad):
        y = _GroupNormFunction.apply(x, norm.weight, norm.bias, norm.num_groups, float(norm.eps), bool(tokens_out))
    else:
        y = _group_norm_forward(x, norm.weight, norm.bias, norm.num_groups, norm.eps, tokens_out)[0]
    return y.transpose(1, 2).unflatten(2, (x.shape[2], x.shape[3])) if tokens_out else y


# ---- BatchNorm2d with batch statistics (+ GELU) in grad mode (include/dfx_fused.h, csrc/batchnorm_train.hip) --------------------
BN_CHUNK_PIXELS = _C["DFX_BN_CHUNK_PIXELS"]


def _bn_partials(N, HW):
    """chunks of all images of one channel: the workspace holds 6 (forward) / 8 (backward) floats per channel and chunk"""
    return N * (-(-HW // BN_CHUNK_PIXELS))


def batch_norm_train_forward(x, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=None):
    """-> (y, stats): y = act(batch_norm(x)) with the statistics of this batch, act None or "gelu"; stats [2C] fp32, the
    batch mean [C] followed by 1 / sqrt(biased var + eps) [C], as ``batch_norm_backward`` reads them.  x [N,C,H,W] contiguous
    fp32 with more than one value per channel.  running_mean / running_var (each may be None) are updated IN PLACE by the
    kernel as nn.BatchNorm2d updates them (the unbiased variance, ``momentum`` a float) and their version counters moved, so
    that ``models.fused.derived_key`` sees it; ``num_batches_tracked`` is the caller's."""
    named = [("x", x), ("weight", weight), ("bias", bias)]
    named += [(n, t) for n, t in (("running_mean", running_mean), ("running_var", running_var)) if t is not None]
    _check_inputs(named)
    _require(act in (None, "none", "gelu"), "batch_norm_train: act is None or 'gelu'")
    _require(x.dim() == 4 and all(t.dtype == torch.float32 for _, t in named) and all(t.numel() == x.shape[1] for _, t in named[1:]),
             "batch_norm_train: fp32, x [N,C,H,W], parameters and running statistics [C]")
    N, C, H, W = x.shape
    dev = x.device
    y = torch.empty_like(x)
    stats = torch.empty((2 * C,), dtype=torch.float32, device=dev)
    ws = torch.empty((6 * C * _bn_partials(N, H * W),), dtype=torch.float32, device=dev)
    _call("batch_norm_train", "dfx_batch_norm_train_f32", dev, x.data_ptr(), weight.data_ptr(), bias.data_ptr(), _ptr(running_mean),
          _ptr(running_var), y.data_ptr(), stats.data_ptr(), ws.data_ptr(), N, C, H * W, float(eps), float(momentum), ACT[act])
    for t in (running_mean, running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return y, stats


def batch_norm_backward(grad_out, x, stats, weight, bias, eps=1e-5, act=None, need_x=True, need_gamma=True, need_beta=True):
    """Gradients of ``batch_norm_train_forward``: -> (grad_x | None, grad_gamma | None, grad_beta | None), fp32, fresh tensors
    (include/dfx_fused.h, dfx_batch_norm_backward_f32: two streaming launches, no atomics, the same bits every call).
    grad_out and x [N,C,H,W] contiguous, stats [2C] as the forward wrote them, weight and bias [C], the forward's eps; with
    act "gelu" the GELU's argument is recomputed from x: nothing else of the forward is needed."""
    _check_inputs([("grad_out", grad_out), ("x", x), ("stats", stats), ("weight", weight), ("bias", bias)])
    _require(act in (None, "none", "gelu"), "batch_norm_backward: act is None or 'gelu'")
    _require(x.dim() == 4 and grad_out.shape == x.shape and grad_out.dtype == torch.float32 and x.dtype == torch.float32
             and stats.dtype == torch.float32 and weight.dtype == torch.float32 and bias.dtype == torch.float32
             and weight.numel() == x.shape[1] and bias.numel() == x.shape[1] and stats.numel() == 2 * x.shape[1],
             "batch_norm_backward: fp32, grad_out and x [N,C,H,W], weight and bias [C], stats [2C]")
    N, C, H, W = x.shape
    dev = x.device
    grad_x = torch.empty_like(x) if need_x else None
    grad_gamma = torch.empty((C,), dtype=torch.float32, device=dev) if need_gamma else None
    grad_beta = torch.empty((C,), dtype=torch.float32, device=dev) if need_beta else None
    if need_x or need_gamma or need_beta:
        ws = torch.empty((8 * C * _bn_partials(N, H * W),), dtype=torch.float32, device=dev)
        _call("batch_norm_backward", "dfx_batch_norm_backward_f32", dev, grad_out.data_ptr(), x.data_ptr(), stats.data_ptr(),
              weight.data_ptr(), bias.data_ptr(), _ptr(grad_x), _ptr(grad_gamma), _ptr(grad_beta), ws.data_ptr(), N, C, H * W, float(eps), ACT[act])
    return grad_x, grad_gamma, grad_beta


class _BatchNormFunction(torch.autograd.Function):
    """apply(x, weight, bias, running_mean | None, running_var | None, momentum, eps, act) -> (y, the running buffers that were
    given); keeps x and stats (and the two parameters, which are inputs) for the backward - neither the BatchNorm output nor
    the GELU output."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, act):
        y, stats = batch_norm_train_forward(x, weight, bias, running_mean, running_var, momentum, eps, act)
        ctx.save_for_backward(x, stats, weight, bias)
        ctx.eps, ctx.act = eps, act
        # the running buffers are inputs written in place: declared dirty (and so returned), never differentiated
        buffers = tuple(t for t in (running_mean, running_var) if t is not None)
        if buffers:
            ctx.mark_dirty(*buffers)
            ctx.mark_non_differentiable(*buffers)
        return (y,) + buffers

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output, *_buffers):
        x, stats, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        # (looked up at call time: tests wrap it)
        gx, gg, gb = batch_norm_backward(grad_output.contiguous(), x, stats, weight, bias, ctx.eps, ctx.act, need_x=need[0], need_gamma=need[1],
                                         need_beta=need[2])
        return gx, gg, gb, None, None, None, None, None


def batch_norm_train_supported(bn):
    """Is ``bn`` a BatchNorm the kernels cover: nn.BatchNorm2d in training mode (batch statistics), affine, a float momentum"""
    return (type(bn) is torch.nn.BatchNorm2d and bn.training and bn.affine and isinstance(bn.momentum, float)
            and 0.0 <= bn.momentum <= 1.0 and bn.weight.dtype == torch.float32)


def batch_norm_train(x, bn, act=None):
    """``bn(x)`` of an nn.BatchNorm2d in training mode (``batch_norm_train_supported``), followed by nn.GELU() when act is
    "gelu", in three streaming launches; running statistics and ``num_batches_tracked`` move as the module moves them.  With
    grad mode on and x or a parameter requiring a gradient the result carries an autograd node whose backward is
    ``batch_norm_backward`` (computed for exactly the inputs that ask); otherwise no node is made."""
    _require(batch_norm_train_supported(bn), "batch_norm_train: an affine nn.BatchNorm2d in training mode with a float momentum")
    track = bn.track_running_stats and bn.running_mean is not None
    rm, rv = (bn.running_mean, bn.running_var) if track else (None, None)
    x = x.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad):
        y = _BatchNormFunction.apply(x, bn.weight, bn.bias, rm, rv, float(bn.momentum), float(bn.eps), act)[0]
    else:
        y = batch_norm_train_forward(x, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, act)[0]
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return y


# ---- training criterion (include/dfx_criterion.h, csrc/criterion.hip) ------------------------------------------------
def criterion_layout(queries, zero_labels, counts):
    """The ragged layout of one criterion call -> (descriptor as a list of ints, (S, B, rows, Ttot)).  ``queries``: Q_s per
    prediction set, ``zero_labels``: per set, "its labels are all 0" (enc_outputs), ``counts``: targets per image."""
    S, B = len(queries), len(counts)
    desc, row = [], 0
    for Q, zero in zip(queries, zero_labels):
        desc += [int(Q), row, int(bool(zero))]
        row += B * int(Q)
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    _require(row * 4 < 2 ** 31 and sum(queries) * off[-1] < 2 ** 31, "criterion_layout: too many rows or pairs")
    return desc + off, (S, B, row, off[-1])


def _criterion_operands(what, logits, boxes, tgt_labels, tgt_boxes, desc, dims):
    S, B, rows, Ttot = dims
    _check_inputs([("logits", logits), ("boxes", boxes), ("tgt_labels", tgt_labels), ("tgt_boxes", tgt_boxes), ("desc", desc)])
    _require(logits.dtype == torch.float32 and boxes.dtype == torch.float32 and tgt_boxes.dtype == torch.float32
             and tgt_labels.dtype == torch.int32 and desc.dtype == torch.int32, f"{what}: fp32 operands, int32 labels and descriptor")
    _require(tuple(logits.shape) == (rows, 3) and tuple(boxes.shape) == (rows, 4) and tgt_labels.numel() == Ttot
             and tgt_boxes.numel() == 4 * Ttot and desc.numel() == 3 * S + B + 1,
             f"{what}: logits [rows,3] (the reference's three-column loss), boxes [rows,4], labels [Ttot], target boxes [Ttot,4], "
             "descriptor 3*S + B + 1 ints")


def match_cost(logits, boxes, tgt_labels, tgt_boxes, desc, dims, cost_class, cost_bbox, cost_giou):
    """Matching costs of every (set, image, query, target of that image) pair in one launch -> flat fp32 [sum(Q) * Ttot]:
    block (s, b) is a row-major [Q_s, T_b] matrix at Ttot * sum(Q_s' < s) + Q_s * tgt_off[b] (dfx_match_cost_f32)."""
    _criterion_operands("match_cost", logits, boxes, tgt_labels, tgt_boxes, desc, dims)
    S, B, rows, Ttot = dims
    cost = torch.empty(((rows // B if B else 0) * Ttot,), dtype=torch.float32, device=logits.device)
    _call("match_cost", "dfx_match_cost_f32", logits.device, logits.data_ptr(), boxes.data_ptr(), tgt_labels.data_ptr(),
          tgt_boxes.data_ptr(), desc.data_ptr(), S, B, rows, Ttot, float(cost_class), float(cost_bbox), float(cost_giou), cost.data_ptr())
    return cost


def _lsap_check(rc, what):
    if rc == _lib.ENONFINITE:
        raise ValueError("matrix contains invalid numeric entries")          # scipy's wording for the same input
    if rc != 0:
        _lib.check(rc, what)


def lsap(cost):
    """Rectangular linear sum assignment of a [Q, T] matrix in host memory (dfx_lsap_f32: host code, shortest augmenting
    paths, double accumulation over the fp32 entries) -> (rows, cols): min(Q, T) int64 indices each, sorted by row.  A NaN
    or infinite entry raises ValueError, as scipy.optimize.linear_sum_assignment does."""
    cost = torch.as_tensor(cost)
    _require(cost.dim() == 2 and not cost.is_cuda, "lsap: a 2-d matrix in host memory")
    cost = cost.to(torch.float32).contiguous()
    Q, T = cost.shape
    n = min(Q, T)
    rows, cols = torch.empty(n, dtype=torch.int32), torch.empty(n, dtype=torch.int32)
    _lsap_check(_lib.load().dfx_lsap_f32(cost.data_ptr(), Q, T, rows.data_ptr(), cols.data_ptr()), "lsap")
    return rows.long(), cols.long()


def lsap_ragged(cost, desc, dims, row_target=None):
    """dfx_lsap_f32 on every block of a ``match_cost`` result held in HOST memory (fp32, flat), ``desc`` the descriptor in host
    memory (int32) -> row_target [rows] int32 in host memory (``row_target`` when given): global target index or -1."""
    S, B, rows, Ttot = dims
    _require(not cost.is_cuda and not desc.is_cuda and cost.dtype == torch.float32 and desc.dtype == torch.int32
             and cost.is_contiguous() and desc.is_contiguous() and cost.numel() >= (rows // B if B else 0) * Ttot
             and desc.numel() >= 3 * S + B + 1, "lsap_ragged: contiguous fp32 costs and int32 descriptor in host memory")
    if row_target is None:
        row_target = torch.empty(rows, dtype=torch.int32)
    _require(not row_target.is_cuda and row_target.dtype == torch.int32 and row_target.is_contiguous()
             and row_target.numel() >= rows, "lsap_ragged: row_target is int32 [rows] in host memory")
    _lsap_check(_lib.load().dfx_lsap_ragged_f32(cost.data_ptr(), desc.data_ptr(), S, B, rows, Ttot, row_target.data_ptr()), "lsap_ragged")
    return row_target


def set_loss_forward(logits, boxes, tgt_labels, tgt_boxes, row_target, desc, dims, inv_num_boxes):
    """-> out [S, 5] fp32 = loss_ce, class_error, loss_bbox, loss_giou, cardinality_error of every set, one launch
    (dfx_set_loss_forward_f32); ``row_target`` [rows] int32 on the device."""
    _criterion_operands("set_loss_forward", logits, boxes, tgt_labels, tgt_boxes, desc, dims)
    S, B, rows, Ttot = dims
    _check_inputs([("logits", logits), ("row_target", row_target)])
    _require(row_target.dtype == torch.int32 and row_target.numel() == rows, "set_loss_forward: row_target is int32 [rows]")
    out = torch.empty((S, 5), dtype=torch.float32, device=logits.device)
    _call("set_loss_forward", "dfx_set_loss_forward_f32", logits.device, logits.data_ptr(), boxes.data_ptr(), tgt_labels.data_ptr(),
          tgt_boxes.data_ptr(), row_target.data_ptr(), desc.data_ptr(), S, B, rows, Ttot, float(inv_num_boxes), out.data_ptr())
    return out


def set_loss_backward(grad_out, logits, boxes, tgt_labels, tgt_boxes, row_target, desc, dims, inv_num_boxes,
                      need_logits=True, need_boxes=True):
    """Gradients of sum(grad_out * out) of ``set_loss_forward`` in closed form, one launch -> (grad_logits | None,
    grad_boxes | None), fresh tensors written in full (dfx_set_loss_backward_f32).  Column 0 of grad_logits and the box
    gradient of unmatched rows are exact zeros."""
    _criterion_operands("set_loss_backward", logits, boxes, tgt_labels, tgt_boxes, desc, dims)
    S, B, rows, Ttot = dims
    _check_inputs([("logits", logits), ("row_target", row_target), ("grad_out", grad_out)])
    _require(row_target.dtype == torch.int32 and row_target.numel() == rows and grad_out.dtype == torch.float32
             and tuple(grad_out.shape) == (S, 5), "set_loss_backward: row_target is int32 [rows], grad_out fp32 [S,5]")
    grad_logits = torch.empty_like(logits) if need_logits else None
    grad_boxes = torch.empty_like(boxes) if need_boxes else None
    if need_logits or need_boxes:
        _call("set_loss_backward", "dfx_set_loss_backward_f32", logits.device, grad_out.data_ptr(), logits.data_ptr(), boxes.data_ptr(),
              tgt_labels.data_ptr(), tgt_boxes.data_ptr(), row_target.data_ptr(), desc.data_ptr(), S, B, rows, Ttot,
              float(inv_num_boxes), _ptr(grad_logits), _ptr(grad_boxes))
    return grad_logits, grad_boxes


class SetLossFunction(torch.autograd.Function):
    """apply(logits [rows,3], boxes [rows,4], tgt_labels, tgt_boxes, row_target, desc, dims, inv_num_boxes) -> out [S,5].
    Keeps its inputs, row_target and the descriptor - nothing of the forward's arithmetic; columns 1 and 4 of the result
    (class_error, cardinality_error) have no gradient."""

    @staticmethod
    def forward(ctx, logits, boxes, tgt_labels, tgt_boxes, row_target, desc, dims, inv_num_boxes):
        out = set_loss_forward(logits, boxes, tgt_labels, tgt_boxes, row_target, desc, dims, inv_num_boxes)
        ctx.save_for_backward(logits, boxes, tgt_labels, tgt_boxes, row_target, desc)
        ctx.dims, ctx.inv_num_boxes = dims, inv_num_boxes
        return out

    @staticmethod
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad
        gl, gb = set_loss_backward(grad_out.contiguous(), *ctx.saved_tensors, ctx.dims, ctx.inv_num_boxes,
                                   need_logits=need[0], need_boxes=need[1])
        return gl, gb, None, None, None, None, None, None
