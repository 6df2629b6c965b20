"""ctypes binding of libtpspp_hip.so.  The C ABI is the headers under include/; `_SIGNATURES` maps each header's file name
to the `{name: (argtypes, restype)}` of the functions it declares, `headers()` lists them and `symbols(header)` gives one
header's names (tests/test_capi_symbols.py holds every header, this table and the shared object to each other).  A new
entry point goes under the header that declares it; a new header is a new key.  There is no fallback: if the library is
missing or fails to load, `lib()` raises.  Tensors cross this boundary as raw pointers."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtpspp_hip.so")
ABI_VERSION = 12

_f = ctypes.c_void_p       # device pointers travel as integers
_i = ctypes.c_int
_l = ctypes.c_longlong
_u64 = ctypes.c_ulonglong

# header file name -> {function: (argtypes, restype)}; the entries keep a flat indent so that a signature is one short line
_SIGNATURES = {"tpspp.h": {
    "tpspp_abi_version": ([], _i),
    "tpspp_last_error": ([], ctypes.c_char_p),
    "tpspp_solve_T": ([_f, _f, _i, _i, _f, _f], _i),
    "tpspp_build_grid": ([_f, _i, _f, _f, _f, _i, _i, _i, _f, _f], _i),
    "tpspp_grid_sample": ([_f, _f, _i, _i, _i, _i, _i, _i, _f, _f, _f], _i),
    "tpspp_transpose_p_hat": ([_f, _i, _i, _i, _f, _f], _i),
    "tpspp_table_mirror_symmetry": ([_f, _i, _i, _i, _i], _i),
    "tpspp_prepared_table_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_prepare_mirror_table": ([_f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_warp_fwd": ([_f, _i, _i, _i, _f, _i, _i, _i, _f, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i,
                        _f, _f, _f, _f, _f], _i),
    "tpspp_warp_plan_create": ([_f, _i, _i, _i, _f, _i, _i, _i, _f, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i,
                                _f, _f, _f, _f, _f, _f], _i),
    "tpspp_warp_plan_run": ([_f], _i),
    "tpspp_warp_plan_run_on": ([_f, _f], _i),
    "tpspp_warp_plan_destroy": ([_f], None),
    "tpspp_conv2d_fwd": ([_f, _f, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _f], _i),
    "tpspp_conv2d_route": ([_f] + [_i] * 11, _i),
    "tpspp_conv2d_bf16_fwd": ([_f, _f, _i, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _f], _i),
    "tpspp_conv2d_bf16_route": ([_f, _f, _i, _f, _f, _f, _i, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i], _i),
    "tpspp_conv2d_bwd_data": ([_f, _f, _i, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f], _i),
    "tpspp_conv2d_bwd_weight_workspace_floats": ([_f, _i, _i, _i, _i, _i, _i, _i], ctypes.c_size_t),
    "tpspp_conv2d_bwd_weight": ([_f, _f, _i, _f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, ctypes.c_size_t,
                                 _f], _i),
    "tpspp_conv2d_prep_weight": ([_f, _i, _i, _i, _i, _f, _f, _f], _i),
    "tpspp_mm_f32": ([_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _i, ctypes.c_float, _i, _f], _i),
    "tpspp_linear_bwd_weight_workspace_floats": ([_l, _i, _i], ctypes.c_size_t),
    "tpspp_linear_bwd_weight": ([_f, _f, _f, _i, _l, _i, _i, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_act_bwd": ([_i, _l, _f, _f, ctypes.c_float, _f, _f], _i),
    "tpspp_plane_ln_fwd": ([_f, _f, _f, _l, _i, ctypes.c_float, _f, _f, _f, _f], _i),
    "tpspp_plane_ln_bwd_workspace_floats": ([_l, _i], ctypes.c_size_t),
    "tpspp_plane_ln_bwd": ([_f, _f, _f, _f, _f, _l, _i, _f, _i, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_dgab_pool_fwd": ([_f, _f, _i, _i, _i, _i, _i, _f, _f, _f], _i),
    "tpspp_dgab_pool_bwd": ([_f, _f, _i, _i, _i, _i, _i, _f, _f, _f], _i),
    "tpspp_dgab_gate_fwd": ([_f, _f, _f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_dgab_gate_bwd": ([_f, _f, _f, _f, _i, _i, _i, _i, _f, _f, _f, _f], _i),
    "tpspp_cbam_train_fwd": ([_f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f, _f, _f], _i),
    "tpspp_cbam_bwd_workspace_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_cbam_bwd": ([_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_bn_stats_workspace_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_bn_train_stats": ([_f, _i, _i, _i, ctypes.c_float, ctypes.c_float, _f, _f, _f, _f, _f, _f, ctypes.c_size_t, _f],
                             _i),
    "tpspp_bn_eval_stats": ([_f, _f, _i, ctypes.c_float, _f, _f, _f], _i),
    "tpspp_bn_apply_fwd": ([_f, _f, _f, _f, _f, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_bn_bwd_reduce_workspace_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_bn_bwd_reduce": ([_f, _f, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _f, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_bn_bwd_data": ([_f, _f, _i, _f, _f, _f, _f, _f, _i, _f, _f, _f, _f, _f, _f, _i, _f, _f, _f, _i, _i, _i, _i, _f],
                          _i),
    "tpspp_bn_pool2x2_fwd": ([_f, _f, _f, _f, _f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_bn_pool2x2_bwd_reduce_workspace_floats": ([_i, _i, _i, _i], ctypes.c_size_t),
    "tpspp_bn_pool2x2_bwd_reduce": ([_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_bn_pool2x2_bwd_data": ([_f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_global_avgpool_bwd": ([_f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_crnn_maxpool_bwd": ([_f, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _f], _i),
    "tpspp_conv_bf16_chunk_channels": ([_i], _i),
    "tpspp_dgab_fwd": ([_f] * 16 + [_i, _i, _f], _i),
    "tpspp_dgab_bf16_fwd": ([_f] * 16 + [_i, _i, _i, _f], _i),
    "tpspp_score_fwd": ([_f, _f, _f, _f, _f, _f, ctypes.c_float, _f, _i, _i, _f], _i),
    "tpspp_score_x3_fwd": ([_f, _f, _f, _f, _f, _f, ctypes.c_float, _f, _i, _i, _f], _i),
    "tpspp_front_fwd": ([_f] * 15 + [_i, _i, _i, _f], _i),
    "tpspp_front_bf16_fwd": ([_f] * 15 + [_i, _i, _i, _i, _i, _f], _i),
    "tpspp_down_fused_bf16_fwd": ([_f] * 6 + [_i, _i, _i, _i, _f], _i),
    "tpspp_down_fused_x3_fwd": ([_f] * 6 + [_i, _i, _i, _i, _f], _i),
    "tpspp_down_fused_f32_fwd": ([_f] * 6 + [_i, _i, _i, _i, _f], _i),
    "tpspp_token_gemm_bf16_fwd": ([_f] * 5 + [_i, _i, _i, _i, _i, _i, _f], _i),
    "tpspp_mm_bf16": ([_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _f], _i),
    "tpspp_crnn_lstm_bf16_fwd": ([_f, _f, _f, _i, _i, _i, _i, _i, _f], _i),
    "tpspp_crnn_lstm_bf16_train_fwd": ([_f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f], _i),
    "tpspp_crnn_lstm_bf16_bwd": ([_f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f], _i),
    "tpspp_linear_bwd_weight_bf16_workspace_floats": ([_i, _i, _i, _i], ctypes.c_size_t),
    "tpspp_linear_bwd_weight_bf16": ([_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, ctypes.c_size_t, _i, _f], _i),
    "tpspp_cbam_fwd": ([_f, _f, _f, _f, _f, _f, _i, _f], _i),
    "tpspp_tpe_points_fwd": ([_f] * 13 + [_i, _f], _i),
    "tpspp_maxpool2x2_fwd": ([_f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_global_avgpool_fwd": ([_f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_conv_chunk_channels": ([_i], _i),
    "tpspp_conv_set_tuning": ([_i], _i),
    "tpspp_warp_set_tuning": ([_i, _i, _i, _i], _i),
    "tpspp_warp_set_trace": ([_f], _i),
    "tpspp_head_set_trace": ([_f], _i),
    "tpspp_lab_occupy": ([_i, _i, _i, _f], _i),
    "tpspp_warp_bwd_workspace_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_warp_bwd_set_accumulator": ([_i], _i),
    "tpspp_warp_bwd": ([_f, _f, _i, _i, _i, _f, _f, _i, _i, _i, _f, _f, _f, _f, _i, _f, _f, _f, _i, _i, _i, _i, _i,
                        _f, _f, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_warp_bwd_route": ([_f, _f, _i, _i, _i, _f, _f, _i, _i, _i, _f, _f, _f, _f, _i, _f, _f, _f, _i, _i, _i, _i, _i,
                              _f, _f, _f, _f, _f, ctypes.c_size_t, _f, _i], _i),
    "tpspp_transpose2d": ([_f, _i, _i, _f, _f], _i),
    "tpspp_layernorm_cm_fwd": ([_f, _f, _f, _i, _i, ctypes.c_float, _f, _f], _i),
    "tpspp_attn_enc_fwd": ([_f, _i, _i, _i, _f, _f, _f], _i),
    "tpspp_linear_ln_fwd": ([_f, _i, _i, ctypes.c_float, _f, _f, _i, _f, _i, _f, _i, _f, _f], _i),
    "tpspp_resize_normalize_fwd": ([_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _i, _f], _i),
    "tpspp_nrtr_encoder_workspace": ([_i, _i, _i, _i], ctypes.c_size_t),
    "tpspp_nrtr_decoder_workspace": ([_i] * 7, ctypes.c_size_t),
    "tpspp_nrtr_encoder_fwd": ([_f, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, ctypes.c_size_t, _f, _f, _i, _f], _i),
    "tpspp_nrtr_decoder_fwd": ([_f, _i, _i, _i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _f, _i, _i, _i, _i, _f, _f,
                                _f, ctypes.c_size_t, _f, _f, _f, _i, _f], _i),
    "tpspp_nrtr_decoder_route": ([_i, _i, _i, _i, _f, _i, _i, _i], _i),
    "tpspp_blocked_to_nchw_bf16": ([_f, _i, _i, _i, _f, _f], _i),
    "tpspp_attn_tensor2idx_fwd": ([_f, _i, _i, _i, _i, _i, _f, _f, _f], _i),
}, "tpspp_train_attn.h": {      # the encoder's attention training kernels
    "tpspp_attn_train_fwd": ([_f, _f, _f, _l, _i, _i, _i, _i, _i, _f, ctypes.c_float, _u64, _u64, _f, _f, _f], _i),
    "tpspp_attn_train_bwd": ([_f, _f, _f, _f, _l, _f, _f, _i, _i, _i, _i, _i, _f, ctypes.c_float, _u64, _u64, _f, _f, _f, _l,
                              _f], _i),
    "tpspp_attn_dropout_mask": ([_i, _i, _i, _i, ctypes.c_float, _u64, _u64, _f, _f], _i),
}, "tpspp_train_dec.h": {       # the decoder's attention, its embedding and the sequence cross-entropy
    "tpspp_attn_train_fwd_ex": ([_f, _l, _f, _f, _l, _i, _i, _i, _i, _i, _f, _f, _i, ctypes.c_float, _u64, _u64, _f, _f, _f], _i),
    "tpspp_attn_train_bwd_ex": ([_f, _f, _l, _f, _f, _l, _f, _f, _i, _i, _i, _i, _i, _f, _f, _i, ctypes.c_float, _u64, _u64,
                                 _f, _l, _f, _f, _l, _f], _i),
    "tpspp_embed_pos_fwd": ([_f, _f, _f, _i, _i, _i, _i, _f, _f], _i),
    "tpspp_embed_bwd_workspace_floats": ([_l, _i, _i], ctypes.c_size_t),
    "tpspp_embed_bwd": ([_f, _f, _l, _i, _i, _i, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_seq_ce_fwd": ([_f, _l, _l, _l, _f, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f], _i),
    "tpspp_seq_ce_bwd": ([_f, _f, _l, _l, _l, _f, _f, _f, _i, _i, _i, _i, _i, _i, _f, _f], _i),
}, "tpspp_train_opt.h": {       # multi-tensor Adam / AdamW, the gradient norm and its clipping coefficient, zeroing
    "tpspp_mt_adam": ([_f, _f, _i, _f, _i, _i, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double, _i, _f, _f], _i),
    "tpspp_mt_sumsq": ([_f, _i, _f, _i, _i, _i, _f, ctypes.c_size_t, _f], _i),
    "tpspp_mt_norm_finish": ([_f, _i, ctypes.c_float, _f, _f], _i),
    "tpspp_mt_zero": ([_f, _i, _f, _i, _i, _i, _f], _i),
}, "tpspp_augment.h": {         # the train pipeline's resize + augmentation + normalisation kernel
    "tpspp_augment_normalize_fwd": ([_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _i, _f, _f, _i, _i, _f], _i),
}, "tpspp_crnn.h": {            # the CRNN recogniser: rectangular max-pool, LSTM recurrence, CTC greedy decode
    "tpspp_crnn_maxpool_fwd": ([_f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _f], _i),
    "tpspp_crnn_lstm_fwd": ([_f, _f, _f, _i, _i, _i, _i, _f], _i),
    "tpspp_crnn_lstm_plan": ([_i, _i, _i], _i),
    "tpspp_crnn_ctc_decode": ([_f, _f, _i, _i, _i, _i, _f, _f, _f], _i),
}, "tpspp_crnn_train.h": {      # the CRNN decoder's and the CTC loss's training kernels
    "tpspp_crnn_lstm_train_fwd": ([_f, _f, _f, _f, _f, _i, _i, _i, _i, _f], _i),
    "tpspp_crnn_lstm_bwd": ([_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _f], _i),
    "tpspp_crnn_ctc_loss_workspace_floats": ([_i, _i, _i], ctypes.c_size_t),
    "tpspp_crnn_ctc_loss_fwd": ([_f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, ctypes.c_size_t, _f], _i),
    "tpspp_crnn_ctc_loss_bwd": ([_f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f], _i),
}, "tpspp_crnn_bf16.h": {       # VeryDeepVgg's reduced modes: the max-pools on blocked bf16 / fp32 maps
    "tpspp_crnn_maxpool_blk_fwd": ([_f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _f], _i),
}}

_lib = None


class TpsppError(RuntimeError):
    pass


def headers():
    """File names of the headers under include/ that declare the C ABI."""
    return list(_SIGNATURES)


def symbols(header):
    """Names the header declares (kept in sync by tests/test_capi_symbols.py)."""
    return sorted(_SIGNATURES[header])


def lib():
    """The loaded library; raises if it is absent (build it: `python -m tps_pp_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TpsppError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -m tps_pp_amd.build`). There is no CPU or PyTorch fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for table in _SIGNATURES.values():
            for name, (argtypes, restype) in table.items():
                fn = getattr(L, name)      # AttributeError if the ABI lost a symbol
                fn.argtypes = argtypes
                fn.restype = restype
        got = L.tpspp_abi_version()
        if got != ABI_VERSION:
            raise TpsppError(f"libtpspp_hip.so ABI {got} != binding ABI {ABI_VERSION}: rebuild")
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().tpspp_last_error().decode("utf-8", "replace")
        raise TpsppError(f"{what} failed ({rc}): {msg}")
