"""ctypes loader of libdfx.so (the C ABI declared in include/dfx_msda.h)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFX_LIBRARY selects another build of the library (diagnostic / ablation builds of tools/ab.sh); it must exist - there is no
# fall back to the shipped one
_SO = os.environ.get("DFX_LIBRARY") or os.path.join(_HERE, "libdfx.so")
_lib = None

_i, _l, _p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
_DIMS = [_i] * 7  # N, S, M, D, L, Lq, P

# name -> argtypes; every function returns int (0 = ok, <0 = DFX_E*)
SIGNATURES = {
    "dfx_msda_forward_f32": [_p] * 5 + _DIMS + [_p, _p],
    "dfx_msda_forward_f64": [_p] * 5 + _DIMS + [_p, _p],
    "dfx_msda_backward_f32": [_p] * 6 + _DIMS + [_p, _p, _p, _p],
    "dfx_msda_backward_f64": [_p] * 6 + _DIMS + [_p, _p, _p, _p],
    # 2-byte value / grad_out / out, fp32 loc / aw / gradients (csrc/msda_forward.hip, csrc/msda_backward.hip)
    "dfx_msda_forward_bf16": [_p] * 5 + _DIMS + [_p, _p],
    "dfx_msda_forward_f16": [_p] * 5 + _DIMS + [_p, _p],
    "dfx_msda_backward_bf16": [_p] * 6 + _DIMS + [_p, _p, _p, _p],
    "dfx_msda_backward_f16": [_p] * 6 + _DIMS + [_p, _p, _p, _p],
    "dfx_msda_fused_forward_f32": [_p, _p, _p, _p, _i, _i, _p, _l, _p, _l] + _DIMS + [_p, _p],
    # value, shapes, lsi, ref, ref_dim, off, off_stride, logits, logit_stride, grad_out, dims, grad_value | NULL,
    # grad_off, stride, grad_logits, stride, grad_ref | NULL, stream (csrc/msda_fused_backward.hip)
    "dfx_msda_fused_backward_f32": [_p, _p, _p, _p, _i, _p, _l, _p, _l, _p] + _DIMS + [_p, _p, _l, _p, _l, _p, _p],
    # ref, ref_dim, off, off_pitch, logits, logit_pitch, grad_out, N, H, W, Lq, grad_value, stream (csrc/msda_level_backward.hip)
    "dfx_msda_level_grad_value_f32": [_p, _i, _p, _l, _p, _l, _p, _i, _i, _i, _i, _p, _p],
    # the deterministic twins (csrc/fixed_sum.h): ... grad_value, [int64 workspace,] 16-byte scratch word, ...
    "dfx_msda_fixed_fraction_bits": [_i],
    "dfx_msda_level_grad_value_fixed_f32": [_p, _i, _p, _l, _p, _l, _p, _i, _i, _i, _i, _p, _p, _p],
    "dfx_msda_fused_backward_fixed_f32": [_p, _p, _p, _p, _i, _p, _l, _p, _l, _p] + _DIMS + [_p, _p, _p, _p, _l, _p, _l, _p, _p],
    # K, ph, pw, sampling_ratio;  the float entry's arguments + int64 workspace, scratch word, stream
    "dfx_roi_align_fixed_fraction_bits": [_i, _i, _i, _i],
    "dfx_roi_align_backward_nhwc_fixed_f32": [_p, _p] + [_i] * 7 + [ctypes.c_float, _i, _i, _p, _p, _p, _p],
    "dfx_profile_enable": [_i],
    "dfx_tuning_reload": [],
    "dfx_profile_drain": [_p, _p, _p, _p, _i],
    "dfx_msda_fused_level_fits": [_i, _i],
    "dfx_msda_fused_level_forward_f32": [_p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    # include/dfx_mha.h: (ptr, batch stride, row stride) x (q, k, v, out), B, heads, Lq, Lk, scale, stream
    "dfx_mha_f32": [_p, _l, _l, _p, _l, _l, _p, _l, _l, _p, _l, _l, _i, _i, _i, _i, ctypes.c_float, _p],
    # ... + lse, drop | NULL in front of B
    "dfx_mha_train_forward_f32": [_p, _l, _l] * 4 + [_p, _p, _i, _i, _i, _i, ctypes.c_float, _p],
    # (grad_out, q, k, v, out) x (ptr, batch, row), lse, drop | NULL, (grad_q | NULL, grad_k | NULL, grad_v | NULL) x (ptr, batch, row)
    "dfx_mha_backward_f32": [_p, _l, _l] * 5 + [_p, _p] + [_p, _l, _l] * 3 + [_i, _i, _i, _i, ctypes.c_float, _p],
    # include/dfx_roi.h: input, rois, N, C, H, W, K, ph, pw, scale, sampling_ratio, aligned, out, stream
    "dfx_roi_align_nchw_f32": [_p, _p] + [_i] * 7 + [ctypes.c_float, _i, _i, _p, _p],
    "dfx_roi_align_nhwc_f32": [_p, _p] + [_i] * 7 + [ctypes.c_float, _i, _i, _p, _p],
    # grad_out, rois, N, C, H, W, K, ph, pw, scale, sampling_ratio, aligned, grad_input (zero-filled by the call), stream
    "dfx_roi_align_backward_nchw_f32": [_p, _p] + [_i] * 7 + [ctypes.c_float, _i, _i, _p, _p],
    "dfx_roi_align_backward_nhwc_f32": [_p, _p] + [_i] * 7 + [ctypes.c_float, _i, _i, _p, _p],
    "dfx_dynamic_conv_f32": [_p, _p, _l, _p, _p, _p, _p, _p, _i, _i, _i, _i, ctypes.c_float, _p],
    # grad_out, feats, params, p_stride, g1, b1, g2, b2, grad_feats, grad_params, gp_stride, grad_ln, workspace, K, R, C, dd, eps
    "dfx_dynamic_conv_backward_f32": [_p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _l, _p, _p, _i, _i, _i, _i, ctypes.c_float, _p],
    # include/dfx_preprocess.h
    "dfx_preprocess_u8_f32": [_p, _i, _i, _i, _p, _p, _i, _p, _p, _i, _i, _i, _p, _p, _p, _l, _i, _i, _p, _p],
    # include/dfx_gemm.h
    "dfx_gemm_f32": [_p, _p, _l, _l, _p, _l, _l, _i, _p, _i, _p, _l, _l, _p, _l, _p, _l, _l, _i, _i, _i, _i, _i, _i, _l, _l, _p],
    "dfx_gemm_splitk_f32": [_p, _l, _p, _l, _i, _p, _i, _p, _l, _p, _l, _i, _i, _i, _i, _i, _p, _p],
    "dfx_conv1x1_pair_f32": [_p, _p, _l, _i, _p, _l, _i, _p, _p, _l, _i, _i, _i, _i, _p],
    # W3, X1, stride, K1, X2, stride, K2, b3, R, stride, Y, stride, W1, b1, Z, stride, Co, C1, HW, batch, act_z, stream
    "dfx_conv1x1_chain_f32": [_p, _p, _l, _i, _p, _l, _i, _p, _p, _l, _p, _l, _p, _p, _p, _l, _i, _i, _i, _i, _i, _p],
    # dY, ldy, X, ldx, dW, ldw, db | NULL, M, N, K, splits, workspace | NULL, stream (csrc/gemm_wgrad.hip)
    "dfx_gemm_wgrad_f32": [_p, _l, _p, _l, _p, _l, _p, _i, _i, _i, _i, _p, _p],
    # dZ, image stride, X, image stride, dW, Co, Ci, HW, batch, splits, workspace | NULL, stream (csrc/gemm_f32.hip)
    "dfx_conv1x1_wgrad_f32": [_p, _l, _p, _l, _p, _i, _i, _i, _i, _i, _p, _p],
    # include/dfx_gemm_bf16.h: A, a_dtype, lda, W (bf16), ldw, bias | NULL, R | NULL, ldr, C, c_dtype, ldc, M, N, K, act, stream
    "dfx_gemm_bf16": [_p, _i, _l, _p, _l, _p, _p, _l, _p, _i, _l, _i, _i, _i, _i, _p],
    # include/dfx_fused.h: x, bias, residual, out, N, C, HW, relu, stream
    "dfx_bias_act_nchw_f32": [_p, _p, _p, _p, _i, _i, _l, _i, _p],
    "dfx_bias_relu_maxpool_f32": [_p, _p, _p, _i, _i, _i, _i, _p],
    "dfx_add_layernorm_f32": [_p, _p, _p, _p, _p, _l, _i, ctypes.c_float, _p],
    # x, res | NULL, mask | NULL, gamma, beta, out, s, mean, rstd, keep | NULL, rows, C, eps, stream (csrc/layernorm_train.hip)
    "dfx_add_layernorm_train_f32": [_p] * 10 + [_l, _i, ctypes.c_float, _p],
    # dy, s, mean, rstd, gamma, keep | NULL, scale, grad_x | NULL, grad_res | NULL, grad_gamma | NULL, grad_beta | NULL,
    # workspace | NULL, rows, C, stream
    "dfx_add_layernorm_backward_f32": [_p] * 6 + [ctypes.c_float] + [_p] * 5 + [_l, _i, _p],
    "dfx_box_refine_f32": [_p, _p, _i, _p, _l, ctypes.c_float, _p],
    "dfx_group_norm_f32": [_p, _p, _p, _p, _p, _i, _i, _l, _i, ctypes.c_float, _i, _p],
    # dy, x, stats, gamma, dx | NULL, dgamma | NULL, dbeta | NULL, workspace, N, C, HW, groups, dy_tokens, stream
    # (csrc/groupnorm_backward.hip)
    "dfx_group_norm_backward_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _l, _i, _i, _p],
    # x, gamma, beta, running_mean | NULL, running_var | NULL, y | NULL, stats, workspace, N, C, HW, eps, momentum, act, stream
    # (csrc/batchnorm_train.hip)
    "dfx_batch_norm_train_f32": [_p] * 8 + [_i, _i, _l, ctypes.c_double, ctypes.c_double, _i, _p],
    # dy, x, stats, gamma, beta, dx | NULL, dgamma | NULL, dbeta | NULL, workspace, N, C, HW, eps, act, stream
    "dfx_batch_norm_backward_f32": [_p] * 9 + [_i, _i, _l, ctypes.c_double, _i, _p],
    # include/dfx_conv.h
    "dfx_conv2d_igemm_f32": [_p, _p, _p, _p, _p] + [_i] * 14 + [_l, _p],
    "dfx_conv2d_tile_fits": [_i] * 6,
    "dfx_conv2d_tile_f32": [_p, _p, _p, _p] + [_i] * 13 + [_l, _p],
    "dfx_conv3x3_wino_f32": [_p, _p, _p, _p] + [_i] * 7 + [_p],
    "dfx_wino_weights_f32": [_p, _p, _p, _i, _i, _p],
    # include/dfx_criterion.h: logits, boxes, tgt_labels, tgt_boxes, desc, S, B, rows, Ttot, cost weights x 3, cost, stream
    "dfx_match_cost_f32": [_p] * 5 + [_i] * 4 + [ctypes.c_float] * 3 + [_p, _p],
    # logits, boxes, tgt_labels, tgt_boxes, row_target, desc, S, B, rows, Ttot, 1/num_boxes, out, stream
    "dfx_set_loss_forward_f32": [_p] * 6 + [_i] * 4 + [ctypes.c_double, _p, _p],
    # grad_out, the forward's six pointers, S, B, rows, Ttot, 1/num_boxes, grad_logits | NULL, grad_boxes | NULL, stream
    "dfx_set_loss_backward_f32": [_p] * 7 + [_i] * 4 + [ctypes.c_double, _p, _p, _p],
    # host code, host pointers: cost [Q,T], Q, T, rows, cols;  cost, desc, S, B, rows, Ttot, row_target
    "dfx_lsap_f32": [_p, _i, _i, _p, _p],
    "dfx_lsap_ragged_f32": [_p, _p, _i, _i, _i, _i, _p],
    # include/dfx_optim.h: tensors, chunks, n_chunks, partials, stream
    "dfx_optim_chunk_elements": [],
    "dfx_grad_sqnorm_f32": [_p, _p, _i, _p, _p],
    # tensors, chunks, n_chunks, partials | NULL, max_norm, norm_out | NULL, stream
    "dfx_adamw_step_f32": [_p, _p, _i, _p, ctypes.c_float, _p, _p],
}
ENONFINITE = -4       # DFX_ENONFINITE of include/dfx_criterion.h


class LevelLayout(ctypes.Structure):
    """dfx_msda_level_layout (include/dfx_msda.h): operand strides of the level-in-LDS kernel, in floats."""
    _fields_ = [(n, ctypes.c_long) for n in (
        "value_frame", "value_token", "value_head", "value_oct", "value_chunk",
        "off_row", "off_head", "logit_row", "logit_head",
        "out_row", "out_head", "out_oct", "out_chunk")]


def library_path():
    return _SO


def load():
    """Return the loaded library; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                f"{_SO} is missing: the HIP extension has not been built "
                "(run `python __graft_entry__.py build` or `make -C <pkg>/csrc`). "
                "There is no CPU or PyTorch fallback for this operator.")
        lib = ctypes.CDLL(_SO)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        lib.dfx_abi_version.restype = ctypes.c_int
        lib.dfx_last_error.restype = ctypes.c_char_p
        _lib = lib
    return _lib


def abi_version():
    return load().dfx_abi_version()


def check(rc, what):
    if rc != 0:
        msg = load().dfx_last_error().decode() or f"error code {rc}"
        raise RuntimeError(f"{what}: {msg}")
