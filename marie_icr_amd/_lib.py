"""ctypes binding of libmarie_hip.so (the C ABI declared in include/marie_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call
fails, the product path raises.  Build it with ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C marie_icr_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MARIE_HIP_LIB selects another build of the same library (kernel A/B experiments); never a fallback
LIB_PATH = os.environ.get("MARIE_HIP_LIB") or os.path.join(_HERE, "libmarie_hip.so")

PREC_F16 = 0
PREC_F32 = 1
STAGE_GUARD = 4096   # MHIP_STAGE_GUARD: elements behind every output of a stage entry

# every symbol include/marie_hip.h declares: (name, restype, argtypes)
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_SIGNATURES = (
    ("mhip_init", _i, [_i, C.POINTER(_vp)]),
    ("mhip_destroy", _i, [_vp]),
    ("mhip_last_error", C.c_char_p, [_vp]),
    ("mhip_set_stream", _i, [_vp, _vp]),
    ("mhip_synchronize", _i, [_vp]),
    ("mhip_device_info", _i, [_vp, C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    ("mhip_memcpy_dev", _i, [_vp, _vp, _vp, _sz]),
    ("mhip_gate_create", _i, [_vp, C.POINTER(_vp)]),
    ("mhip_gate_destroy", _i, [_vp]),
    ("mhip_gate_signal", _i, [_vp, _vp]),
    ("mhip_gate_count", C.c_longlong, [_vp]),
    ("mhip_gate_open", _i, [_vp, _i]),
    ("mhip_gate_wait", _i, [_vp, _vp, C.c_longlong, _i]),
    ("mhip_profile_enable", _i, [_vp, _i]),
    ("mhip_profile_reset", _i, [_vp]),
    ("mhip_profile_read", _i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ("mhip_profile_flops", _i, [_vp, _i, C.POINTER(C.c_double)]),
    ("mhip_kernel_count", _i, []),
    ("mhip_kernel_name", C.c_char_p, [_i]),
    ("mhip_conv2d_nhwc", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_conv2d_nhwc_ex", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_icr_create", _i, [_vp, _i, _i, C.POINTER(_vp)]),
    ("mhip_icr_destroy", _i, [_vp]),
    ("mhip_icr_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_icr_finalize", _i, [_vp]),
    ("mhip_icr_alloc_arena", _i, [_vp]),
    ("mhip_icr_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_icr_steps", _i, []),
    ("mhip_icr_forward", _i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("mhip_icr_forward_host", _i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("mhip_craft_create", _i, [_vp, _i, C.POINTER(_vp)]),
    ("mhip_craft_destroy", _i, [_vp]),
    ("mhip_craft_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_craft_finalize", _i, [_vp]),
    ("mhip_craft_alloc_arena", _i, [_vp]),
    ("mhip_craft_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_craft_geometry", _i, [_i, _i, _i, C.c_double, C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(_i),
                                 C.POINTER(_i), C.POINTER(_i)]),
    ("mhip_craft_workspace_bytes", _sz, [_vp, _i, _i, _i, C.c_double]),
    ("mhip_craft_kernel_flops", C.c_double, [_vp, _i, _i, _i, _i, C.c_double]),
    ("mhip_craft_forward", _i, [_vp, _vp, _i, _i, _i, C.c_double, _vp]),
    ("mhip_craft_detect", _i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_float, C.c_float, C.c_float, _vp, _i,
                               C.POINTER(_i), _vp, C.POINTER(C.c_double)]),
    ("mhip_craft_detect_host", _i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_float, C.c_float, C.c_float, _vp, _i,
                                    C.POINTER(_i), _vp, C.POINTER(C.c_double)]),
    ("mhip_craft_boxes_host", _i, [_vp, _vp, _i, _i, C.c_float, C.c_float, C.c_float, _vp, _i, C.POINTER(_i), _vp, _vp,
                                   _vp, _i, C.POINTER(_i)]),
    ("mhip_crop_batch", _i, [_vp, _vp, _vp, _i, _i, _vp]),
    ("mhip_pil_resize_rgb_host", _i, [_vp, _vp, _i, _i, _vp, _i, _i, _i]),
    ("mhip_pil_resize_fragments_host", _i, [_vp, _vp, _sz, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_vit_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_vit_destroy", _i, [_vp]),
    ("mhip_vit_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_vit_finalize", _i, [_vp]),
    ("mhip_vit_alloc_arena", _i, [_vp]),
    ("mhip_vit_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_vit_forward_host", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_dit_default_config", _i, [_i, _vp]),
    ("mhip_dit_resized_shape", _i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    ("mhip_dit_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_dit_destroy", _i, [_vp]),
    ("mhip_dit_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_dit_finalize", _i, [_vp]),
    ("mhip_dit_alloc_arena", _i, [_vp]),
    ("mhip_dit_arena", _i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_dit_workspace_bytes", _sz, [_vp, _i, _i, _i]),
    ("mhip_dit_detect", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("mhip_dit_detect_host", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("mhip_dit_detect_ex", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("mhip_dit_detect_ex_host", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("mhip_dit_debug_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_dit_debug_taps_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_rpn_proposals_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_float, _vp, _vp, _vp]),
    ("mhip_roi_align_host", _i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    ("mhip_det_final_host", _i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_float, C.c_float, _i, _vp, _vp, _vp]),
    ("mhip_det_final_multi_host", _i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, C.c_float, C.c_float, _i, _vp, _vp,
                                       _vp, _vp]),
    ("mhip_register_warp", _i, [_vp, _vp, _i, _i, C.c_size_t, _vp, _vp, _vp]),
    ("mhip_register_warp_host", _i, [_vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_blackout_bboxes", _i, [_vp, _vp, _i, _i, _vp, _i, C.POINTER(_i)]),
    ("mhip_content_extents", _i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    ("mhip_overlay_create", _i, [_vp, _i, _i, C.POINTER(_vp)]),
    ("mhip_overlay_destroy", _i, [_vp]),
    ("mhip_overlay_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_overlay_finalize", _i, [_vp]),
    ("mhip_overlay_padded_shape", _i, [_i, _i, C.POINTER(_i), C.POINTER(_i)]),
    ("mhip_overlay_forward", _i, [_vp, _vp, _i, _i, _vp]),
    ("mhip_overlay_forward_host", _i, [_vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_overlay_blend", _i, [_vp, _vp, _vp, _vp, _sz]),
    ("mhip_trocr_default_config", _i, [_i, _vp]),
    ("mhip_trocr_max_len", _i, [_vp]),
    ("mhip_trocr_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_trocr_destroy", _i, [_vp]),
    ("mhip_trocr_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_trocr_finalize", _i, [_vp]),
    ("mhip_trocr_alloc_arena", _i, [_vp]),
    ("mhip_trocr_arena", _i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_trocr_workspace_bytes", _sz, [_vp, _i]),
    ("mhip_trocr_set_decode_gate", _i, [_vp, _vp]),
    ("mhip_trocr_generate", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    ("mhip_trocr_generate_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_trocr_generate_fragments", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    ("mhip_trocr_encode_begin", _i, [_vp, _i]),
    ("mhip_trocr_encode_fragments", _i, [_vp, _vp, _vp, _i, _i]),
    ("mhip_trocr_encoded", _i, [_vp]),
    ("mhip_trocr_decode", _i, [_vp, _vp, _vp, _vp]),
    ("mhip_trocr_generate_trace_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    ("mhip_cross_attention_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_cross_attention_stages_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    ("mhip_decode_attention_host", _i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    ("mhip_beam_candidates_host", _i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    ("mhip_beam_search_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    ("mhip_gemm_ln_fold", _i, [_vp, _i, _vp]),
    ("mhip_ln_finalize", _i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, C.c_float]),
    ("mhip_token_init_split", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    ("mhip_layoutlmv3_default_config", _i, [_vp]),
    ("mhip_layoutlmv3_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_layoutlmv3_destroy", _i, [_vp]),
    ("mhip_layoutlmv3_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_layoutlmv3_finalize", _i, [_vp]),
    ("mhip_layoutlmv3_alloc_arena", _i, [_vp]),
    ("mhip_layoutlmv3_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_layoutlmv3_set_resample", _i, [_vp, _i]),
    ("mhip_layoutlmv3_seq_len", _i, [_vp]),
    ("mhip_layoutlmv3_bucket", _i, [_i, _i, _i]),
    ("mhip_layoutlmv3_max_token_labels", _i, [_i]),
    ("mhip_layoutlmv3_classify", _i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("mhip_layoutlmv3_hidden_host", _i, [_vp, _vp, _sz, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_layoutlmv3_tag", _i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_layoutlmv3_tag_host", _i, [_vp, _vp, _sz, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_token_head_host", _i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_attention_bias_host", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_attention_host", _i, [_vp, _vp]),
    ("mhip_vq_template_create", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, C.POINTER(_vp)]),
    ("mhip_vq_template_destroy", _i, [_vp]),
    ("mhip_vq_template_state", _i, [_vp, C.POINTER(_i), C.POINTER(_i), _vp, _vp]),
    ("mhip_vq_template_set_filters", _i, [_vp, _vp, _vp]),
    ("mhip_vq_match", _i, [_vp, _vp, _i, _i, _sz, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    ("mhip_vq_assign_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    ("mhip_vq_kmeans_step_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    ("mhip_vq_heatmap_host", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("mhip_vq_peaks_host", _i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    ("mhip_clip_cosine_host", _i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    ("mhip_lev_ngrams_host", _i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_clipvis_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_clipvis_destroy", _i, [_vp]),
    ("mhip_clipvis_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_clipvis_finalize", _i, [_vp]),
    ("mhip_clipvis_alloc_arena", _i, [_vp]),
    ("mhip_clipvis_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_clipvis_workspace_bytes", _sz, [_vp, _i]),
    ("mhip_clipvis_embed_host", _i, [_vp, _vp, _i, _i, _vp]),
    ("mhip_clipvis_embed_pairs_host", _i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    ("mhip_clipvis_debug_taps_host", _i, [_vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_clipvis_quick_gelu_host", _i, [_vp, _i, _vp, _i, _vp]),
    ("mhip_clipvis_embed_rows_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, _vp]),
    ("mhip_clipvis_head_host", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, C.c_float, _vp, _i, _vp]),
    ("mhip_clipvis_pair_cosine_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    ("mhip_cliprn_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_cliprn_destroy", _i, [_vp]),
    ("mhip_cliprn_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_cliprn_finalize", _i, [_vp]),
    ("mhip_cliprn_alloc_arena", _i, [_vp]),
    ("mhip_cliprn_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_cliprn_workspace_bytes", _sz, [_vp, _i]),
    ("mhip_cliprn_embed_host", _i, [_vp, _vp, _i, _i, _vp]),
    ("mhip_cliprn_embed_pairs_host", _i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    ("mhip_cliprn_tap_shape", _i, [_vp, _i, _vp]),
    ("mhip_cliprn_debug_taps_host", _i, [_vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_cliprn_stem_host", _i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    ("mhip_avgpool_nhwc_host", _i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_cliprn_attnpool_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_cliptext_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_cliptext_destroy", _i, [_vp]),
    ("mhip_cliptext_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_cliptext_finalize", _i, [_vp]),
    ("mhip_cliptext_alloc_arena", _i, [_vp]),
    ("mhip_cliptext_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_cliptext_workspace_bytes", _sz, [_vp, _i, _i]),
    ("mhip_cliptext_embed_host", _i, [_vp, _vp, _vp, _i, _i, _vp]),
    ("mhip_cliptext_embed_pairs_host", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    ("mhip_cliptext_debug_taps_host", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_cliptext_embed_rows_host", _i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_cliptext_attention_host", _i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    ("mhip_cliptext_head_host", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, C.c_float, _vp, _i, _vp, _vp]),
    ("mhip_berttext_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_berttext_create_ex", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_berttext_destroy", _i, [_vp]),
    ("mhip_berttext_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_berttext_finalize", _i, [_vp]),
    ("mhip_berttext_alloc_arena", _i, [_vp]),
    ("mhip_berttext_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_berttext_workspace_bytes", _sz, [_vp, _i, _i]),
    ("mhip_berttext_alibi_slopes", _i, [_i, _vp]),
    ("mhip_berttext_embed_host", _i, [_vp, _vp, _vp, _i, _i, _vp]),
    ("mhip_berttext_embed_pairs_host", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    ("mhip_berttext_debug_taps_host", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_berttext_embed_rows_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_attention_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_attention_long_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_rel_table", _i, [_i, _i, _vp, _i, _vp]),
    ("mhip_berttext_embed_rows_ex_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_attention_rel_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_attention_rel_long_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_geglu_host", _i, [_vp, _i, _vp, _i, _i, _vp]),
    ("mhip_berttext_pool_host", _i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_create_cls", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_berttext_classify_host", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_berttext_attention_window_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_berttext_attention_global_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    ("mhip_berttext_cls_head_host", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    ("mhip_layoutreader_create", _i, [_vp, _i, _vp, C.POINTER(_vp)]),
    ("mhip_layoutreader_destroy", _i, [_vp]),
    ("mhip_layoutreader_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_layoutreader_finalize", _i, [_vp]),
    ("mhip_layoutreader_alloc_arena", _i, [_vp]),
    ("mhip_layoutreader_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_layoutreader_workspace_bytes", _sz, [_vp, _i]),
    ("mhip_layoutreader_order_host", _i, [_vp, _vp, _vp, _i, _vp]),
    ("mhip_layoutreader_debug_host", _i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_layoutreader_attention_host", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("mhip_max_page_size", _i, [_i, _i, _i, _i, C.c_double, C.POINTER(_i), C.POINTER(_i)]),
    ("mhip_resize_area_u8", _i, [_vp, _vp, _i, _i, _i, C.c_size_t, _vp, _i, _i]),
    ("mhip_resize_area_u8_host", _i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    ("mhip_resize_cubic_u8", _i, [_vp, _vp, _i, _i, _i, C.c_size_t, _vp, _i, _i]),
    ("mhip_resize_cubic_u8_host", _i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    ("mhip_merge_boxes", _i, [_vp, _i, _vp, C.POINTER(_i)]),
    ("mhip_line_merge", _i, [_vp, _i, _vp, C.POINTER(_i)]),
    ("mhip_find_line_numbers", _i, [_vp, _i, _vp, _i, _vp]),
    ("mhip_lines_from_bboxes", _i, [_vp, _i, _i, _i, _vp, _i, C.POINTER(_i)]),
    ("mhip_crnn_forward_crops", _i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_crnn_forward_fragments_host", _i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_crnn_create", _i, [_vp, _i, _i, C.POINTER(_vp)]),
    ("mhip_crnn_destroy", _i, [_vp]),
    ("mhip_crnn_set_tensor", _i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    ("mhip_crnn_finalize", _i, [_vp]),
    ("mhip_crnn_alloc_arena", _i, [_vp]),
    ("mhip_crnn_arena", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("mhip_crnn_seq_len", _i, [_i]),
    ("mhip_crnn_forward", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_crnn_forward_host", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("mhip_crnn_workspace_bytes", _sz, [_vp, _i, _i]),
    ("mhip_crnn_kernel_flops", C.c_double, [_vp, _i, _i, _i]),
    ("mhip_lstm_rec_host", _i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    ("mhip_conv_gray_first_host", _i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("mhip_maxpool_s21_p01_host", _i, [_vp, _i, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_avgpool_hw_host", _i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    ("mhip_tps_sample_host", _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_attn_context_host", _i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    ("mhip_attn_cell_host", _i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    ("mhip_argmax_rows_host", _i, [_vp, _vp, _i, _i, _i, _vp]),
    ("mhip_rowmax_softmax_host", _i, [_vp, _vp, _i, _i, _vp, _vp]),
    ("mhip_row_layernorm_host", _i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, C.c_float, _i, _vp, _vp]),
    ("mhip_resize_linear_u8_host", _i, [_vp, _vp, _i, _i, _vp, _i, _i]),
    ("mhip_conv_rgb_first_host", _i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("mhip_maxpool_host", _i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    ("mhip_upsample_bilinear_host", _i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    ("mhip_score_head_host", _i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, C.c_longlong, _vp]),
)
EXPORTED_SYMBOLS = tuple(s[0] for s in _SIGNATURES)



class ConvDesc(C.Structure):
    """mirror of ``mhip_conv_desc`` (include/marie_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "Cin", "KH", "KW", "pad", "N", "pool", "relu", "out_f32",
                                         "dil", "Cin1", "ldc", "pad_cols_writable")]


class ConvExDesc(C.Structure):
    """mirror of ``mhip_conv_ex_desc`` (include/marie_hip.h); res_dev is an HBM address"""
    _fields_ = (ConvDesc._fields_ + [(n, C.c_int32) for n in ("sy", "pad_x", "row_period", "row_stride", "row_offset")] +
                [("res_dev", C.c_void_p)])


EPI_LN_ROWS, EPI_LN_COLS, EPI_SPLIT = 1, 2, 3


class GemmFoldDesc(C.Structure):
    """mirror of ``mhip_gemm_fold_desc`` (include/marie_hip.h); the pointers are HBM addresses"""
    _fields_ = ([(n, C.c_void_p) for n in ("in_dev", "w_dev", "scale_dev", "bias_dev", "out_dev", "ln_a_dev", "ln_b_dev",
                                           "ln_cs_dev", "row_bias_dev", "out2_dev", "res_dev", "res2_dev", "stats_dev")] +
                [(n, C.c_int32) for n in ("epi", "M", "N", "K", "act", "stats_ld", "row_period", "row_stride", "row_offset")])


class VitConfig(C.Structure):
    """mirror of mhip_vit_config (include/marie_hip.h)"""
    _fields_ = [("dim", C.c_int), ("depth", C.c_int), ("heads", C.c_int), ("patch", C.c_int), ("pos_h", C.c_int),
                ("pos_w", C.c_int), ("layer_scale", C.c_int), ("qkv_bias", C.c_int), ("final_norm", C.c_int),
                ("fpn", C.c_int), ("taps", C.c_int * 4), ("ln_eps", C.c_float)]


class DitConfig(C.Structure):
    """mirror of mhip_dit_config (include/marie_hip.h)"""
    _fields_ = [("model", C.c_int), ("min_size_test", C.c_int), ("max_size_test", C.c_int),
                ("detections_per_image", C.c_int), ("anchor_sizes", C.c_float * 5), ("aspect_ratios", C.c_float * 3),
                ("rpn_nms_thresh", C.c_float), ("score_thresh", C.c_float), ("nms_thresh", C.c_float),
                ("num_classes", C.c_int)]


class RegisterDesc(C.Structure):
    """mirror of mhip_register_desc (include/marie_hip.h)"""
    _fields_ = [("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_w", C.c_int), ("crop_h", C.c_int), ("out_w", C.c_int),
                ("out_h", C.c_int), ("left", C.c_int), ("top", C.c_int), ("canvas_w", C.c_int), ("canvas_h", C.c_int),
                ("n_markers", C.c_int), ("marker_x", C.c_int * 4), ("marker_y", C.c_int * 4), ("marker_radius", C.c_int),
                ("marker_color", C.c_int * 3), ("final_w", C.c_int), ("final_h", C.c_int)]


class TrocrConfig(C.Structure):
    """mirror of mhip_trocr_config (include/marie_hip.h)"""
    _fields_ = [("enc_dim", C.c_int), ("enc_depth", C.c_int), ("enc_heads", C.c_int), ("dec_dim", C.c_int),
                ("dec_layers", C.c_int), ("dec_heads", C.c_int), ("dec_ffn", C.c_int), ("vocab", C.c_int),
                ("max_positions", C.c_int), ("beam", C.c_int), ("max_len_b", C.c_int), ("min_len", C.c_int),
                ("pad", C.c_int), ("eos", C.c_int), ("embed_scale", C.c_float), ("img_size", C.c_int)]


class BeamTrace(C.Structure):
    """mirror of mhip_beam_trace (include/marie_hip.h); the pointers are host arrays"""
    _fields_ = ([(n, C.c_void_p) for n in ("cand_scores", "cand_tokens", "cand_beams", "parent", "last_tok", "cum", "ignore",
                                           "finished", "fin_count", "tokens", "anc", "remaining", "fin_tokens", "fin_len",
                                           "fin_score", "out_tokens", "out_len", "out_score")] + [("steps", C.c_int32)])


class LayoutLMv3Config(C.Structure):
    """mirror of mhip_layoutlmv3_config (include/marie_hip.h)"""
    _fields_ = [("hidden", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("ffn", C.c_int), ("vocab", C.c_int),
                ("type_vocab", C.c_int), ("max_position_embeddings", C.c_int), ("max_2d_position_embeddings", C.c_int),
                ("coordinate_size", C.c_int), ("shape_size", C.c_int), ("input_size", C.c_int), ("patch", C.c_int),
                ("rel_pos_bins", C.c_int), ("max_rel_pos", C.c_int), ("rel_2d_pos_bins", C.c_int),
                ("max_rel_2d_pos", C.c_int), ("layer_norm_eps", C.c_float), ("pad_id", C.c_int), ("num_labels", C.c_int),
                ("max_text", C.c_int)]


class ClipVisConfig(C.Structure):
    """mirror of mhip_clipvis_config (include/marie_hip.h)"""
    _fields_ = [("dim", C.c_int), ("depth", C.c_int), ("heads", C.c_int), ("patch", C.c_int), ("image_size", C.c_int),
                ("ffn", C.c_int), ("proj_dim", C.c_int), ("ln_eps", C.c_float)]


class ClipResNetConfig(C.Structure):
    """mirror of mhip_cliprn_config (include/marie_hip.h); ``embed_dim``, ``heads`` and ``grid`` are derived as
    ``clip.build_model`` derives them"""
    _fields_ = [("width", C.c_int), ("layers", C.c_int * 4), ("image_size", C.c_int), ("proj_dim", C.c_int),
                ("bn_eps", C.c_float)]

    @property
    def embed_dim(self) -> int:
        return 32 * self.width

    @property
    def heads(self) -> int:
        return self.width * 32 // 64

    @property
    def grid(self) -> int:
        return self.image_size // 32


class ClipTextConfig(C.Structure):
    """mirror of mhip_cliptext_config (include/marie_hip.h)"""
    _fields_ = [("vocab", C.c_int), ("context", C.c_int), ("dim", C.c_int), ("heads", C.c_int), ("depth", C.c_int),
                ("ffn", C.c_int), ("proj_dim", C.c_int), ("ln_eps", C.c_float)]


class BertTextConfig(C.Structure):
    """mirror of mhip_berttext_config (include/marie_hip.h)"""
    _fields_ = [("vocab", C.c_int), ("max_position", C.c_int), ("type_vocab", C.c_int), ("dim", C.c_int), ("heads", C.c_int),
                ("depth", C.c_int), ("ffn", C.c_int), ("ln_eps", C.c_float), ("position", C.c_int), ("mlp", C.c_int),
                ("pool", C.c_int), ("normalize", C.c_int)]


class SentenceEncoderConfig(BertTextConfig):
    """mirror of mhip_berttext_config_ex (include/marie_hip.h): the fields above, then those of the other families"""
    _fields_ = [("pos_offset", C.c_int), ("rel_buckets", C.c_int), ("rel_max_distance", C.c_int)]


class TextClassifierConfig(C.Structure):
    """mirror of mhip_berttext_config_cls (include/marie_hip.h).  ``attention_window`` points at an int array the owner keeps
    alive for the duration of the create call"""
    _fields_ = [("ex", SentenceEncoderConfig), ("attention_window", C.POINTER(C.c_int)), ("num_labels", C.c_int),
                ("head_function", C.c_int)]


class LayoutReaderConfig(C.Structure):
    """mirror of mhip_layoutreader_config (include/marie_hip.h)"""
    _fields_ = [("dim", C.c_int), ("heads", C.c_int), ("depth", C.c_int), ("ffn", C.c_int), ("max_position", C.c_int),
                ("max_2d", C.c_int), ("max_source", C.c_int), ("type_vocab", C.c_int), ("source_type", C.c_int),
                ("target_type", C.c_int), ("ln_eps", C.c_float)]


class AttentionHostDesc(C.Structure):
    """mirror of ``mhip_attention_host_desc`` (include/marie_hip.h); the pointers are host arrays"""
    _fields_ = ([(n, C.c_int32) for n in ("precision", "layout", "images", "heads", "n_queries", "n_keys", "npad_q", "npad_k")] +
                [(n, C.c_void_p) for n in ("q", "k", "vt", "qcode", "kcode", "w1", "wx", "wy")] +
                [(n, C.c_int32) for n in ("bins_1d", "max_1d", "bins_2d", "max_2d", "dp", "dx")] + [("out", C.c_void_p)])


class VqFilters(C.Structure):
    """mirror of ``mhip_vq_filters`` (include/marie_hip.h)"""
    _fields_ = [("n", C.c_int32), ("taps", (C.c_float * 16) * 6), ("dil", (C.c_int32 * 2) * 6), ("weight", C.c_double * 6)]


class CropDesc(C.Structure):
    """mirror of ``mhip_crop_desc`` (include/marie_hip.h)"""
    _fields_ = [("src_offset", C.c_uint64), ("h", C.c_int32), ("w", C.c_int32), ("row_stride", C.c_int32),
                ("channels", C.c_int32)]


POOL_NONE, POOL_2x2, POOL_2x1 = 0, 1, 2

_lib = None


class MarieHipError(RuntimeError):
    pass


def load():
    """dlopen libmarie_hip.so and type every entry point.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.  If libmarie_hip.so were loaded first it would bring in
    # the system copy and a later `import torch` a second one: two HIP runtimes in one process, which intermittently
    # leaves torch with "No HIP GPUs are available".  Loading torch first makes both share torch's runtime (same
    # SONAME).  Without torch installed the system runtime is used alone.
    import importlib.util
    import sys

    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise MarieHipError(
            f"{LIB_PATH} is missing — the HIP extension is not built; there is no CPU fallback "
            "(run __graft_entry__.build() or `make -C marie_icr_amd/csrc`)")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx_handle, rc: int, what: str):
    if rc != 0:
        msg = load().mhip_last_error(ctx_handle)
        raise MarieHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


class Context:
    """One per (process, GPU).  reference counterpart: the `.to(device)` plumbing of
    marie/document/craft_ocr_processor.py:142-146."""

    def __init__(self, device_id: int = 0):
        lib = load()
        h = C.c_void_p()
        rc = lib.mhip_init(int(device_id), C.byref(h))
        if rc != 0 or not h.value:
            raise MarieHipError(f"mhip_init(device={device_id}) failed ({rc}): no usable HIP device")
        self.h = h
        self.lib = lib
        self.device_id = int(device_id)
        self._children = weakref.WeakSet()   # models created on this context; closed before the context is

    def adopt(self, child):
        self._children.add(child)

    def set_stream(self, stream_handle: int | None):
        check(self.h, self.lib.mhip_set_stream(self.h, C.c_void_p(stream_handle or 0)), "mhip_set_stream")

    def synchronize(self):
        check(self.h, self.lib.mhip_synchronize(self.h), "mhip_synchronize")

    def device_info(self):
        arch = C.create_string_buffer(64)
        cu = C.c_int()
        hbm = C.c_size_t()
        check(self.h, self.lib.mhip_device_info(self.h, arch, 64, C.byref(cu), C.byref(hbm)), "mhip_device_info")
        return {"arch": arch.value.decode(), "cu_count": cu.value, "hbm_bytes": hbm.value}

    def memcpy_dev(self, dst_ptr: int, src_ptr: int, nbytes: int):
        check(self.h, self.lib.mhip_memcpy_dev(self.h, C.c_void_p(dst_ptr), C.c_void_p(src_ptr), int(nbytes)),
              "mhip_memcpy_dev")

    def conv2d_nhwc(self, precision: int, desc: "ConvDesc", in_ptr: int, w_ptr: int, scale_ptr: int, bias_ptr: int,
                    out_ptr: int, in2_ptr: int = 0):
        """Enqueue one NHWC conv/GEMM on the ctx stream; pointers are HBM addresses."""
        check(self.h, self.lib.mhip_conv2d_nhwc(self.h, int(precision), C.byref(desc), C.c_void_p(in_ptr),
                                                C.c_void_p(in2_ptr or 0), C.c_void_p(w_ptr), C.c_void_p(scale_ptr or 0),
                                                C.c_void_p(bias_ptr or 0), C.c_void_p(out_ptr)),
              "mhip_conv2d_nhwc")

    def conv2d_nhwc_ex(self, precision: int, desc: "ConvExDesc", in_ptr: int, w_ptr: int, scale_ptr: int, bias_ptr: int,
                       out_ptr: int, in2_ptr: int = 0):
        """conv2d_nhwc with vertical stride, pad_x, residual (desc.res_dev) and the periodic output-row mapping."""
        check(self.h, self.lib.mhip_conv2d_nhwc_ex(self.h, int(precision), C.byref(desc), C.c_void_p(in_ptr),
                                                   C.c_void_p(in2_ptr or 0), C.c_void_p(w_ptr), C.c_void_p(scale_ptr or 0),
                                                   C.c_void_p(bias_ptr or 0), C.c_void_p(out_ptr)),
              "mhip_conv2d_nhwc_ex")

    def gemm_ln_fold(self, precision: int, desc: "GemmFoldDesc"):
        """Enqueue one LayerNorm-folded GEMM of a ViT block (EPI_SPLIT / EPI_LN_ROWS / EPI_LN_COLS) on the ctx stream."""
        check(self.h, self.lib.mhip_gemm_ln_fold(self.h, int(precision), C.byref(desc)), "mhip_gemm_ln_fold")

    def ln_finalize(self, stats_ptr: int, chunks: int, ld: int, rstd_ptr: int, mur_ptr: int, rows: int, D: int, eps: float):
        """Enqueue the merge of EPI_SPLIT's row statistics into rstd and mean * rstd."""
        check(self.h, self.lib.mhip_ln_finalize(self.h, C.c_void_p(stats_ptr), int(chunks), int(ld), C.c_void_p(rstd_ptr),
                                                C.c_void_p(mur_ptr), int(rows), int(D), float(eps)), "mhip_ln_finalize")

    def token_init_split(self, hi_ptr: int, lo_ptr: int, cls_row_ptr: int, cls_stats_ptr: int, stats_ptr: int, stats_ld: int,
                         B: int, npad: int, n_tok: int, D: int):
        """Enqueue the cls / pad rows of the split stream and their row statistics."""
        check(self.h, self.lib.mhip_token_init_split(self.h, C.c_void_p(hi_ptr), C.c_void_p(lo_ptr), C.c_void_p(cls_row_ptr),
                                                     C.c_void_p(cls_stats_ptr), C.c_void_p(stats_ptr), int(stats_ld), int(B),
                                                     int(npad), int(n_tok), int(D)), "mhip_token_init_split")

    def profile_enable(self, on: bool):
        check(self.h, self.lib.mhip_profile_enable(self.h, 1 if on else 0), "mhip_profile_enable")

    def profile_reset(self):
        check(self.h, self.lib.mhip_profile_reset(self.h), "mhip_profile_reset")

    def profile_read(self):
        out = {}
        for k in range(self.lib.mhip_kernel_count()):
            ms = C.c_double()
            n = C.c_int64()
            check(self.h, self.lib.mhip_profile_read(self.h, k, C.byref(ms), C.byref(n)), "mhip_profile_read")
            fl = C.c_double()
            check(self.h, self.lib.mhip_profile_flops(self.h, k, C.byref(fl)), "mhip_profile_flops")
            out[self.lib.mhip_kernel_name(k).decode()] = {"id": k, "total_ms": ms.value, "launches": n.value,
                                                          "flops": fl.value}
        return out

    def make_gate(self) -> "PhaseGate":
        return PhaseGate(self)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            for child in list(getattr(self, "_children", ())):
                child.close()
            self.lib.mhip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelHandle:
    """Base of the model handles: one ``mhip_<stem>_*`` object of the library on a :class:`Context`.  It owns create +
    ``ctx.adopt``, the state_dict upload (``set_tensor`` per tensor, then ``finalize``, which packs the device weight
    arena), the arena entries of the RCCL start-up broadcast (marie_icr_amd/dist.py) and destroy."""

    def __init__(self, ctx: Context, stem: str, *create_args):
        self.ctx, self.lib, self._stem = ctx, ctx.lib, stem
        h = C.c_void_p()
        check(ctx.h, self._fn("create")(ctx.h, *create_args, C.byref(h)), f"mhip_{stem}_create")
        self.h = h
        ctx.adopt(self)

    def _fn(self, what: str):
        return getattr(self.lib, f"mhip_{self._stem}_{what}")

    def _call(self, what: str, *args):
        check(self.ctx.h, self._fn(what)(self.h, *args), f"mhip_{self._stem}_{what}")

    def load_state(self, state):
        """Every tensor of ``state`` (name -> array) to the library, then pack the arena (reference:
        ``model.load_state_dict``).  The library strips a DataParallel ``module.`` prefix where the checkpoints carry one."""
        set_tensor = self._fn("set_tensor")
        for key, val in state.items():
            arr = np.ascontiguousarray(np.asarray(val), dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            check(self.ctx.h, set_tensor(self.h, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim),
                  f"mhip_{self._stem}_set_tensor({key})")
        self._call("finalize")

    def alloc_arena(self):
        """Allocate the arena(s) unfilled: the receiving ranks of the broadcast."""
        self._call("alloc_arena")

    def arena(self):
        """(device pointer, bytes) of the packed weight arena of the single-arena models (CRAFT, CRNN, ICR, ViT): the
        RCCL broadcast unit.  The overlay generator exposes no arena."""
        p, n = C.c_void_p(), C.c_size_t()
        self._call("arena", C.byref(p), C.byref(n))
        return p.value, n.value

    def arenas(self):
        """[(device pointer, bytes), ...] of the models that keep two arenas (DiT, TrOCR: the ViT encoder, then the
        heads / decoder)."""
        out = []
        for which in (0, 1):
            p, n = C.c_void_p(), C.c_size_t()
            self._call("arena", which, C.byref(p), C.byref(n))
            out.append((p.value, n.value))
        return out

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PhaseGate:
    """``mhip_gate`` (include/marie_hip.h): one thread says where a phase starts in its stream (``signal``), another makes its
    own stream wait for that point (``wait``).  ``open()`` lets every waiter through — the error path."""

    def __init__(self, ctx: Context):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        check(ctx.h, self.lib.mhip_gate_create(ctx.h, C.byref(h)), "mhip_gate_create")
        self.h = h
        ctx.adopt(self)

    def signal(self, ctx: Context):
        check(ctx.h, self.lib.mhip_gate_signal(self.h, ctx.h), "mhip_gate_signal")

    def count(self) -> int:
        return int(self.lib.mhip_gate_count(self.h))

    def open(self, opened: bool = True):
        self.lib.mhip_gate_open(self.h, 1 if opened else 0)

    def wait(self, ctx: Context, seq: int, timeout_ms: int = 60000) -> bool:
        rc = self.lib.mhip_gate_wait(self.h, ctx.h, int(seq), int(timeout_ms))
        if rc < 0:
            check(ctx.h, rc, "mhip_gate_wait")
        return rc == 1

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mhip_gate_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
