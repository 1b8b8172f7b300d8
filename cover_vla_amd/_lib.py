"""ctypes binding of libcover_hip.so (C ABI declared in include/cover_hip.h).

The product path fails loudly when the shared library is missing: there is no CPU fallback anywhere in this
package. Structures mirror the header one-to-one; `check_abi()` compares every mirrored sizeof with the
library's own (cover_sizeof) so a drifted layout is an import-time error, not silent corruption.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch-ROCm bundles its own libamdhip64; it MUST be the HIP runtime this process uses (device pointers and streams
# are shared with torch), so torch is imported before libcover_hip.so is dlopen'ed: the loader then resolves the
# library's libamdhip64.so.7 dependency to the copy torch already mapped instead of loading a second runtime.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COVER_LIB_PATH") or os.path.join(_HERE, "libcover_hip.so")   # override: A/B runs of two builds

c_p = C.c_void_p
c_ll = C.c_longlong
c_i = C.c_int
c_f = C.c_float


class CoverError(RuntimeError):
    pass


class GemmEpi(C.Structure):
    _fields_ = [("bias", c_p), ("residual", c_p), ("layer_scale", c_p), ("ld_residual", c_i), ("residual_f32", c_i),
                ("act", c_i), ("glu", c_i), ("out_f32", c_i), ("out_scale", c_f),
                ("norm_w", c_p), ("norm_out", c_p), ("ld_norm_out", c_i), ("norm_style", c_i), ("norm_w_offset", c_f),
                ("norm_eps", c_f), ("norm_b", c_p), ("w8", c_p), ("w8_scale", c_p), ("a8", c_p), ("a8_scale", c_p), ("ld_a8", c_i), ("ld_norm_out8", c_i),
                ("norm_out8", c_p), ("norm_out8_scale", c_p),
                ("a8_mx", c_p), ("out8", c_p), ("out8_mx", c_p), ("ld_out8", c_i), ("w8_klinear", c_i)]


class KvSegment(C.Structure):
    _fields_ = [("k", c_p), ("vt", c_p),
                ("k_slot_stride", c_ll), ("k_t_stride", c_ll), ("k_h_stride", c_ll),
                ("vt_slot_stride", c_ll), ("vt_h_stride", c_ll), ("vt_d_stride", c_ll),
                ("slot_of_batch", c_p), ("len_of_batch", c_p), ("vis_len", c_p),
                ("len", c_i), ("mask_mode", c_i), ("causal_offset", c_i), ("_pad", c_i)]


class AttnArgs(C.Structure):
    _fields_ = [("q", c_p), ("out", c_p),
                ("q_b_stride", c_ll), ("q_t_stride", c_ll), ("q_h_stride", c_ll),
                ("o_b_stride", c_ll), ("o_t_stride", c_ll), ("o_h_stride", c_ll),
                ("B", c_i), ("Tq", c_i), ("Hq", c_i), ("Hkv", c_i), ("D", c_i), ("scale", c_f),
                ("n_seg", c_i), ("_pad", c_i), ("seg", KvSegment * 3),
                ("state_in_o", c_p), ("state_in_ml", c_p), ("state_out_o", c_p), ("state_out_ml", c_p),
                ("out8", c_p), ("out8_mx", c_p), ("out8_rows", c_i), ("_pad2", c_i)]


class DecodeAttnArgs(C.Structure):
    _fields_ = [("qkv", c_p), ("ld_qkv", c_i), ("n_splits", c_i), ("partial", c_p), ("bias", c_p),
                ("N", c_i), ("H", c_i), ("D", c_i), ("scale", c_f),
                ("positions", c_p), ("cos_table", c_p), ("sin_table", c_p), ("n_pos", c_i), ("rope_mode", c_i),
                ("seg", KvSegment * 3), ("write_t", c_i), ("_pad", c_i), ("out", c_p), ("out_row_stride", c_ll)]


class OwnAttnArgs(C.Structure):
    _fields_ = [("qkv", c_p), ("ld_qkv", c_i), ("N", c_i), ("H", c_i), ("D", c_i), ("scale", c_f),
                ("positions", c_p), ("cos_table", c_p), ("sin_table", c_p), ("n_pos", c_i), ("rope_mode", c_i),
                ("k", c_p), ("v", c_p), ("k_scale", c_p), ("v_scale", c_p), ("fp8", c_i), ("t_cap", c_i),
                ("slot_stride", c_ll), ("slot_of_batch", c_p), ("write_t", c_i), ("_pad", c_i),
                ("state_o", c_p), ("state_ml", c_p)]


class RopeArgs(C.Structure):
    _fields_ = [("qkv", c_p), ("ld_qkv", c_i),
                ("B", c_i), ("T", c_i), ("Hq", c_i), ("Hkv", c_i), ("D", c_i),
                ("positions", c_p), ("cos_table", c_p), ("sin_table", c_p), ("n_pos", c_i),
                ("rope_mode", c_i),
                ("k_cache", c_p), ("k_slot_stride", c_ll), ("k_t_stride", c_ll), ("k_h_stride", c_ll),
                ("vt_cache", c_p), ("vt_slot_stride", c_ll), ("vt_h_stride", c_ll), ("vt_d_stride", c_ll),
                ("slot_of_batch", c_p), ("t_offset_of_batch", c_p), ("t_offset", c_i), ("n_splits", c_i),
                ("partial", c_p), ("bias", c_p)]


class PatchifyArgs(C.Structure):
    _fields_ = [("img", c_p), ("in_u8_hwc", c_i), ("H", c_i), ("W", c_i), ("patch", c_i), ("n_img", c_i),
                ("img_stride", c_ll), ("mul", c_f * 3), ("add", c_f * 3), ("out", c_p), ("ld_out", c_i)]


class GemmF32Args(C.Structure):
    _fields_ = [("A", c_p), ("a_row_stride", c_ll), ("a_k_stride", c_ll),
                ("B", c_p), ("b_row_stride", c_ll), ("b_k_stride", c_ll),
                ("C", c_p), ("c_row_stride", c_ll),
                ("bias", c_p), ("residual", c_p), ("ld_residual", c_ll),
                ("M", c_i), ("N", c_i), ("K", c_i), ("act", c_i), ("alpha", c_f),
                ("batch", c_i), ("a_batch_stride", c_ll), ("b_batch_stride", c_ll), ("c_batch_stride", c_ll),
                ("bias_batch_stride", c_ll)]


class MhaF32Args(C.Structure):
    _fields_ = [("q", c_p), ("q_b_stride", c_ll), ("q_t_stride", c_ll),
                ("k", c_p), ("k_b_stride", c_ll), ("k_t_stride", c_ll),
                ("v", c_p), ("v_b_stride", c_ll), ("v_t_stride", c_ll),
                ("out", c_p), ("o_b_stride", c_ll), ("o_t_stride", c_ll),
                ("key_pad", c_p), ("B", c_i), ("Tq", c_i), ("Tk", c_i), ("H", c_i), ("Dh", c_i), ("scale", c_f)]


class TokenSelectArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("uniform", c_p), ("temperature", c_f), ("token_out", c_p), ("logit_out", c_p)]


class TokenSampleArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("uniform", c_p), ("temperature", c_f), ("top_k", c_i), ("top_p", c_f),
                ("token_out", c_p), ("logit_out", c_p), ("kept_out", c_p)]


class TokenSampleScoredArgs(C.Structure):
    _fields_ = TokenSampleArgs._fields_ + [("logprob_out", c_p)]


class TokenLogprobArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("temperature", c_f), ("top_k", c_i), ("top_p", c_f),
                ("token", c_p), ("logprob_out", c_p), ("kept_out", c_p)]


class TokenTopnArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("temperature", c_f), ("top_k", c_i), ("top_p", c_f), ("n", c_i),
                ("token_out", c_p), ("ld_tok", c_ll), ("logprob_out", c_p), ("ld_lp", c_ll),
                ("entropy_out", c_p), ("kept_out", c_p)]


class TokenSampleRowsArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("uniform", c_p), ("temperature", c_p), ("top_k", c_p), ("top_p", c_p),
                ("token_out", c_p), ("logit_out", c_p), ("kept_out", c_p), ("logprob_out", c_p)]


class TokenLogprobRowsArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("temperature", c_p), ("top_k", c_p), ("top_p", c_p),
                ("token", c_p), ("logprob_out", c_p), ("kept_out", c_p)]


class TokenTopnRowsArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i),
                ("temperature", c_p), ("top_k", c_p), ("top_p", c_p), ("n", c_i),
                ("token_out", c_p), ("ld_tok", c_ll), ("logprob_out", c_p), ("ld_lp", c_ll),
                ("entropy_out", c_p), ("kept_out", c_p)]


class TokenAllow(C.Structure):
    _fields_ = [("bits", c_p), ("ld_words", c_ll), ("n_sets", c_i), ("_pad", c_i), ("set_of_row", c_p)]


class TokenRef(C.Structure):
    _fields_ = [("temperature", c_f), ("_pad", c_i), ("logprob_out", c_p)]


class DecodeFeedbackArgs(C.Structure):
    _fields_ = [("pick", c_p), ("force", c_p), ("force_stride", c_ll), ("lp", c_p), ("lp_out", c_p), ("ld_lp", c_ll),
                ("done", c_p), ("tok_out", c_p), ("ld_tok", c_ll), ("eos", c_ll), ("pad", c_ll),
                ("table", c_p), ("vocab", c_i), ("dim", c_i), ("scale", c_f), ("x_out", c_p), ("ldo", c_i),
                ("live", c_p), ("rows", c_i)]


class TokenFsm(C.Structure):
    _fields_ = [("class_of_token", c_p), ("trans", c_p), ("set_of_state", c_p), ("n_states", c_i), ("n_classes", c_i),
                ("state", c_p), ("set_of_row", c_p)]


class ScoreSelectArgs(C.Structure):
    _fields_ = [("it", c_p), ("act", c_p), ("n_members", c_i), ("N", c_i), ("dim", c_i), ("group_size", c_i),
                ("scores_out", c_p), ("result_out", c_p), ("best_out", c_p), ("fused_it_out", c_p),
                ("fused_act_out", c_p)]


class PriorSelectArgs(C.Structure):
    _fields_ = [("scores", c_p), ("logprobs", c_p), ("lp_n_stride", c_ll), ("lp_t_stride", c_ll),
                ("tokens", c_p), ("tok_n_stride", c_ll), ("tok_t_stride", c_ll), ("pad_token_id", c_ll),
                ("N", c_i), ("steps", c_i), ("group_size", c_i), ("top_m", c_i), ("beta", c_f), ("length_normalize", c_i),
                ("prior_out", c_p), ("combined_out", c_p), ("group_mean_out", c_p), ("result_out", c_p), ("best_out", c_p),
                ("ranked_out", c_p)]


class MemberScoresArgs(C.Structure):
    _fields_ = [("it", c_p), ("act", c_p), ("scores", c_p), ("n_members", c_i), ("N", c_i), ("dim", c_i), ("group_size", c_i),
                ("kappa", c_f), ("mode", c_i), ("member_scores_out", c_p), ("mean_out", c_p), ("spread_out", c_p), ("min_out", c_p),
                ("min_member_out", c_p), ("robust_out", c_p), ("result_out", c_p), ("best_out", c_p), ("member_result_out", c_p),
                ("member_best_out", c_p)]


class AugmentArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("normals", c_p), ("centers", c_p),
                ("n_centers", c_i), ("tok_vocab", c_i), ("G", c_i), ("n", c_i), ("K", c_i), ("h", c_i),
                ("sigma", c_f), ("sd_floor", c_f), ("clip_lo", c_f), ("clip_hi", c_f),
                ("out", c_p), ("mean_out", c_p), ("sd_out", c_p), ("votes_out", c_p)]


class ProposalPriorArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("centers", c_p), ("log_share", c_p),
                ("n_centers", c_i), ("tok_vocab", c_i), ("G", c_i), ("group_rows", c_i), ("n_fit", c_i), ("h", c_i),
                ("sigma", c_f), ("sd_floor", c_f), ("prior_out", c_p), ("mean_out", c_p), ("sd_out", c_p), ("votes_out", c_p)]


class RefineArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("scores", c_p), ("normals", c_p), ("centers", c_p),
                ("n_centers", c_i), ("tok_vocab", c_i), ("G", c_i), ("group_rows", c_i), ("n_elite", c_i), ("K", c_i), ("h", c_i), ("_pad", c_i),
                ("sigma", c_f), ("sd_floor", c_f), ("clip_lo", c_f), ("clip_hi", c_f),
                ("out", c_p), ("elite_rows_out", c_p), ("elite_scores_out", c_p), ("mean_out", c_p), ("sd_out", c_p), ("votes_out", c_p)]


class SmoothArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("scores", c_p), ("dim_scale", c_p), ("centers", c_p),
                ("n_centers", c_i), ("tok_vocab", c_i), ("G", c_i), ("group_rows", c_i), ("h", c_i), ("split_gripper", c_i),
                ("radius2", c_f), ("shrink", c_f),
                ("smoothed_out", c_p), ("density_out", c_p), ("neighbours_out", c_p), ("group_mean_out", c_p)]


class CoherenceArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("centers", c_p), ("n_centers", c_i), ("tok_vocab", c_i),
                ("ref", c_p), ("ref_g_stride", c_ll), ("ref_r_stride", c_ll), ("ref_weight", c_p), ("w_g_stride", c_ll),
                ("step_weight", c_p), ("dim_scale", c_p),
                ("G", c_i), ("group_rows", c_i), ("h", c_i), ("R", c_i), ("hr", c_i), ("shift", c_i), ("gripper_penalty", c_f),
                ("prior_out", c_p), ("min_dist_out", c_p), ("nearest_out", c_p)]


class DiverseArgs(C.Structure):
    _fields_ = [("src", c_p), ("n_stride", c_ll), ("t_stride", c_ll), ("centers", c_p), ("n_centers", c_i), ("tok_vocab", c_i),
                ("quality", c_p), ("step_weight", c_p), ("dim_scale", c_p),
                ("G", c_i), ("group_rows", c_i), ("m", c_i), ("h", c_i),
                ("weight", c_f), ("cover_dist", c_f), ("gripper_penalty", c_f), ("_pad", c_f),
                ("picked_rows_out", c_p), ("count_out", c_p), ("pick_value_out", c_p), ("pick_dist_out", c_p), ("assign_out", c_p),
                ("row_dist_out", c_p), ("out", c_p)]


class FastDecodeArgs(C.Structure):
    _fields_ = [("tokens", c_p), ("tok_row_stride", c_ll), ("tok_step_stride", c_ll), ("band_lo", c_ll), ("band_hi", c_ll),
                ("stop_ids", c_ll * 4), ("skip_ids", c_ll * 8), ("n_stop", c_i), ("n_skip", c_i),
                ("piece_off", c_p), ("piece_sym", c_p), ("basis", c_p),
                ("B", c_i), ("L", c_i), ("n_pieces", c_i), ("min_token", c_i), ("H", c_i), ("D", c_i), ("relaxed", c_i), ("scale", c_f),
                ("out", c_p), ("out_n_stride", c_ll), ("out_t_stride", c_ll), ("coeff_out", c_p), ("n_symbols", c_p), ("status", c_p)]


class BeamMergeArgs(C.Structure):
    _fields_ = [("cum", c_p), ("cand_tok", c_p), ("ld_tok", c_ll), ("cand_lp", c_p), ("ld_lp", c_ll), ("feed_pad", c_ll),
                ("groups", c_i), ("B", c_i), ("parent_out", c_p), ("token_out", c_p), ("feed_out", c_p), ("cum_out", c_p),
                ("step_lp_out", c_p)]


class KvGatherSlotsArgs(C.Structure):
    _fields_ = [("k_base", c_p), ("vt_base", c_p), ("k_offset", c_ll), ("vt_offset", c_ll), ("k_slot_stride", c_ll),
                ("vt_slot_stride", c_ll), ("src_slot", c_p), ("dst_slot", c_p),
                ("n_layers", c_i), ("rows", c_i), ("n_slots", c_i), ("cap", c_i), ("Hkv", c_i), ("D", c_i), ("n_t", c_i), ("_pad", c_i)]


class BeamBacktrackArgs(C.Structure):
    _fields_ = [("parent", c_p), ("token", c_p), ("step_lp", c_p), ("steps", c_i), ("rows", c_i), ("B", c_i), ("_pad", c_i),
                ("tokens_out", c_p), ("logprobs_out", c_p)]


class GumbelTopnArgs(C.Structure):
    _fields_ = [("logits", c_p), ("ld", c_ll), ("rows", c_i), ("lo", c_i), ("hi", c_i), ("temperature", c_f),
                ("phi", c_p), ("g_parent", c_p), ("uniform", c_p), ("ld_u", c_ll), ("n", c_i), ("_pad", c_i),
                ("token_out", c_p), ("ld_tok", c_ll), ("logprob_out", c_p), ("ld_lp", c_ll), ("perturbed_out", c_p), ("ld_g", c_ll)]


class BeamMergeGumbelArgs(C.Structure):
    _fields_ = [("cum", c_p), ("cand_tok", c_p), ("ld_tok", c_ll), ("cand_lp", c_p), ("ld_lp", c_ll), ("cand_g", c_p), ("ld_g", c_ll),
                ("feed_pad", c_ll), ("groups", c_i), ("B", c_i), ("parent_out", c_p), ("token_out", c_p), ("feed_out", c_p),
                ("cum_out", c_p), ("step_lp_out", c_p), ("g_out", c_p), ("kappa_out", c_p)]


class Workspace(C.Structure):
    _fields_ = [("ptr", c_p), ("bytes", C.c_size_t)]


class VitLayer(C.Structure):
    _fields_ = [("ln1_w", c_p), ("ln1_b", c_p), ("ln2_w", c_p), ("ln2_b", c_p),
                ("qkv_w", c_p), ("qkv_b", c_p), ("proj_w", c_p), ("proj_b", c_p),
                ("fc1_w", c_p), ("fc1_b", c_p), ("fc2_w", c_p), ("fc2_b", c_p), ("ls1", c_p), ("ls2", c_p)]


class VitDesc(C.Structure):
    _fields_ = [("dim", c_i), ("heads", c_i), ("head_dim_p", c_i), ("mlp_p", c_i), ("n_layers", c_i), ("act", c_i),
                ("ln_eps", c_f), ("attn_scale", c_f), ("layers_host", C.POINTER(VitLayer)),
                ("last_attn_only", c_i), ("_pad", c_i)]


class DecLayer(C.Structure):
    _fields_ = [("in_norm_w", c_p), ("post_norm_w", c_p), ("qkv_w", c_p), ("qkv_b", c_p), ("o_w", c_p),
                ("gate_up_w", c_p), ("down_w", c_p), ("k_cache", c_p), ("vt_cache", c_p),
                ("qkv_w8", c_p), ("qkv_s", c_p), ("o_w8", c_p), ("o_s", c_p), ("gate_up_w8", c_p), ("gate_up_s", c_p),
                ("down_w8", c_p), ("down_s", c_p), ("down_klinear", c_i), ("o_klinear", c_i)]


class DecDesc(C.Structure):
    _fields_ = [("dim", c_i), ("Hq", c_i), ("Hkv", c_i), ("D", c_i), ("mlp", c_i), ("n_layers", c_i), ("act", c_i),
                ("norm_style", c_i), ("norm_eps", c_f), ("norm_w_offset", c_f), ("attn_scale", c_f),
                ("rope_mode", c_i), ("n_pos", c_i), ("_pad", c_i),
                ("cos_table", c_p), ("sin_table", c_p), ("final_norm_w", c_p),
                ("layers_host", C.POINTER(DecLayer))]


class DecGroup(C.Structure):
    _fields_ = [("B", c_i), ("T", c_i), ("positions", c_p), ("n_seg", c_i), ("write_seg", c_i),
                ("segs", KvSegment * 3), ("seg_k_offset", c_ll * 3), ("seg_vt_offset", c_ll * 3),
                ("write_slot_of_batch", c_p), ("write_t_offset_of_batch", c_p),
                ("write_t_offset", c_i), ("seg0_shared", c_i),
                ("own_kv_mode", c_i), ("seg1_group", c_i), ("seg1_slot_of_group", c_p), ("seg1_len_of_group", c_p),
                ("own_region_elems", c_ll)]


class DecPass(C.Structure):
    _fields_ = [("n_groups", c_i), ("final_norm", c_i), ("x_f32", c_p), ("groups", DecGroup * 2)]


_STRUCTS = {
    "cover_gemm_epi": GemmEpi, "cover_kv_segment": KvSegment, "cover_attn_args": AttnArgs,
    "cover_rope_args": RopeArgs, "cover_patchify_args": PatchifyArgs, "cover_gemm_f32_args": GemmF32Args,
    "cover_mha_f32_args": MhaF32Args, "cover_token_select_args": TokenSelectArgs,
    "cover_token_sample_args": TokenSampleArgs, "cover_token_sample_scored_args": TokenSampleScoredArgs,
    "cover_token_logprob_args": TokenLogprobArgs, "cover_token_topn_args": TokenTopnArgs,
    "cover_token_sample_rows_args": TokenSampleRowsArgs, "cover_token_logprob_rows_args": TokenLogprobRowsArgs,
    "cover_token_topn_rows_args": TokenTopnRowsArgs, "cover_token_allow": TokenAllow, "cover_token_ref": TokenRef, "cover_decode_feedback_args": DecodeFeedbackArgs,
    "cover_token_fsm": TokenFsm,
    "cover_score_select_args": ScoreSelectArgs, "cover_prior_select_args": PriorSelectArgs, "cover_augment_args": AugmentArgs,
    "cover_proposal_prior_args": ProposalPriorArgs, "cover_member_scores_args": MemberScoresArgs,
    "cover_refine_args": RefineArgs, "cover_smooth_args": SmoothArgs, "cover_coherence_args": CoherenceArgs,
    "cover_diverse_args": DiverseArgs, "cover_fast_decode_args": FastDecodeArgs,
    "cover_beam_merge_args": BeamMergeArgs,
    "cover_kv_gather_slots_args": KvGatherSlotsArgs, "cover_beam_backtrack_args": BeamBacktrackArgs,
    "cover_gumbel_topn_args": GumbelTopnArgs, "cover_beam_merge_gumbel_args": BeamMergeGumbelArgs, "cover_workspace": Workspace, "cover_vit_layer": VitLayer,
    "cover_vit_desc": VitDesc, "cover_dec_layer": DecLayer, "cover_dec_desc": DecDesc, "cover_dec_group": DecGroup,
    "cover_dec_pass": DecPass, "cover_decode_attn_args": DecodeAttnArgs, "cover_own_attn_args": OwnAttnArgs,
}

# every symbol include/cover_hip.h declares: (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "cover_abi_version": (c_i, []),
    "cover_last_error": (C.c_char_p, []),
    "cover_device_info": (c_i, [c_i, _P(c_i), _P(C.c_size_t), C.c_char_p, c_i]),
    "cover_packed_weight_bytes": (C.c_size_t, [c_i, c_i]),
    "cover_packed_k": (c_i, [c_i]),
    "cover_pack_weight_bf16": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p]),
    "cover_packed_weight_fp8_bytes": (C.c_size_t, [c_i, c_i]),
    "cover_quantize_rows_fp8": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "cover_pack_weight_fp8": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_p]),
    "cover_quantize_act_fp8": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "cover_quantize_act_fp8_mx": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "cover_pack_weight_fp8_klinear": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p]),
    "cover_gemm_workspace_bytes": (C.c_size_t, [c_i, c_i, c_i]),
    "cover_gemm_bf16": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_i, _P(GemmEpi), c_p, C.c_size_t, c_i, c_p]),
    "cover_gemm_plan_counts": (c_i, [C.POINTER(C.c_longlong), c_i, c_i]),
    "cover_gemm_plan": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_i, _P(GemmEpi), c_p, C.c_size_t, c_i, C.POINTER(c_i)]),
    "cover_gemm_probe": (c_i, [C.POINTER(C.c_ulonglong)]),
    "cover_attention_bf16": (c_i, [_P(AttnArgs), c_p]),
    "cover_attention_plan": (c_i, [_P(AttnArgs), _P(c_i)]),
    "cover_attention_bf16_pair": (c_i, [_P(AttnArgs), _P(AttnArgs), c_p]),
    "cover_attention_pair_plan": (c_i, [_P(AttnArgs), _P(AttnArgs), _P(c_i)]),
    "cover_decode_attention_fused": (c_i, [_P(DecodeAttnArgs), c_p]),
    "cover_decode_own_attention": (c_i, [_P(OwnAttnArgs), c_p]),
    "cover_layernorm_bf16": (c_i, [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p]),
    "cover_rmsnorm_bf16": (c_i, [c_p, c_i, c_i, c_p, c_f, c_i, c_p, c_i, c_i, c_i, c_f, c_p]),
    "cover_rmsnorm_bf16_q8": (c_i, [c_p, c_i, c_i, c_p, c_f, c_i, c_p, c_i, c_i, c_i, c_f, c_p, c_i, c_p, c_p]),
    "cover_rope_kv_write": (c_i, [_P(RopeArgs), c_p]),
    "cover_rope_kv_write_pair": (c_i, [_P(RopeArgs), _P(RopeArgs), c_p]),
    "cover_embed_gather": (c_i, [c_p, c_i, c_p, c_i, c_f, c_p, c_i, c_p]),
    "cover_patchify": (c_i, [_P(PatchifyArgs), c_p]),
    "cover_copy_rows_bf16": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "cover_add_rows_bf16": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p]),
    "cover_scale_bf16": (c_i, [c_p, c_i, c_i, c_i, c_f, c_f, c_p]),
    "cover_cast_f32_to_bf16": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "cover_cast_bf16_to_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "cover_gemm_f32": (c_i, [_P(GemmF32Args), c_p]),
    "cover_gemm_f32_plan": (c_i, [_P(GemmF32Args), _P(c_i)]),
    "cover_layernorm_f32": (c_i, [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p]),
    "cover_layernorm_f32_grouped": (c_i, [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_i, c_ll, c_p]),
    "cover_softmax_rows_f32": (c_i, [c_p, c_i, c_i, c_i, c_f, c_p]),
    "cover_l2norm_rows_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "cover_add_f32": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p]),
    "cover_xent_diag_f32": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "cover_act_f32": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p]),
    "cover_mha_f32": (c_i, [_P(MhaF32Args), c_p]),
    "cover_masked_mean_f32": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "cover_sincos_time_embed": (c_i, [c_p, c_i, c_i, C.c_double, C.c_double, c_p, c_i, c_p]),
    "cover_token_select": (c_i, [_P(TokenSelectArgs), c_p]),
    "cover_token_sample": (c_i, [_P(TokenSampleArgs), c_p]),
    "cover_token_sample_scored": (c_i, [_P(TokenSampleScoredArgs), c_p]),
    "cover_token_logprob": (c_i, [_P(TokenLogprobArgs), c_p]),
    "cover_token_topn": (c_i, [_P(TokenTopnArgs), c_p]),
    "cover_token_sample_rows": (c_i, [_P(TokenSampleRowsArgs), c_p]),
    "cover_token_logprob_rows": (c_i, [_P(TokenLogprobRowsArgs), c_p]),
    "cover_token_topn_rows": (c_i, [_P(TokenTopnRowsArgs), c_p]),
    "cover_token_sample_rows_allowed": (c_i, [_P(TokenSampleRowsArgs), _P(TokenAllow), c_p]),
    "cover_token_logprob_rows_allowed": (c_i, [_P(TokenLogprobRowsArgs), _P(TokenAllow), c_p]),
    "cover_token_topn_rows_allowed": (c_i, [_P(TokenTopnRowsArgs), _P(TokenAllow), c_p]),
    "cover_token_sample_rows_ref": (c_i, [_P(TokenSampleRowsArgs), _P(TokenAllow), _P(TokenRef), c_p]),
    "cover_decode_feedback": (c_i, [_P(DecodeFeedbackArgs), c_p]),
    "cover_decode_feedback_lp2": (c_i, [_P(DecodeFeedbackArgs), c_p, c_p, c_ll, c_p]),
    "cover_decode_feedback_fsm": (c_i, [_P(DecodeFeedbackArgs), _P(TokenFsm), c_p, c_p, c_ll, c_p]),
    "cover_score_select": (c_i, [_P(ScoreSelectArgs), c_p]),
    "cover_group_argmax": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p]),
    "cover_prior_select": (c_i, [_P(PriorSelectArgs), c_p]),
    "cover_member_scores": (c_i, [_P(MemberScoresArgs), c_p]),
    "cover_augment_tokens": (c_i, [_P(AugmentArgs), c_p]),
    "cover_augment_actions": (c_i, [_P(AugmentArgs), c_p]),
    "cover_proposal_prior_tokens": (c_i, [_P(ProposalPriorArgs), c_p]),
    "cover_proposal_prior_actions": (c_i, [_P(ProposalPriorArgs), c_p]),
    "cover_refine_tokens": (c_i, [_P(RefineArgs), c_p]),
    "cover_refine_actions": (c_i, [_P(RefineArgs), c_p]),
    "cover_smooth_scores_tokens": (c_i, [_P(SmoothArgs), c_p]),
    "cover_smooth_scores_actions": (c_i, [_P(SmoothArgs), c_p]),
    "cover_coherence_prior_tokens": (c_i, [_P(CoherenceArgs), c_p]),
    "cover_coherence_prior_actions": (c_i, [_P(CoherenceArgs), c_p]),
    "cover_diverse_subset_tokens": (c_i, [_P(DiverseArgs), c_p]),
    "cover_diverse_subset_actions": (c_i, [_P(DiverseArgs), c_p]),
    "cover_fast_decode": (c_i, [_P(FastDecodeArgs), c_p]),
    "cover_beam_merge": (c_i, [_P(BeamMergeArgs), c_p]),
    "cover_kv_gather_slots": (c_i, [_P(KvGatherSlotsArgs), c_p]),
    "cover_beam_backtrack": (c_i, [_P(BeamBacktrackArgs), c_p]),
    "cover_gumbel_topn": (c_i, [_P(GumbelTopnArgs), c_p]),
    "cover_beam_merge_gumbel": (c_i, [_P(BeamMergeGumbelArgs), c_p]),
    "cover_tokens_to_histories": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_f, c_p, c_p, c_p]),
    "cover_tokens_to_histories_steps": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_i, c_f, c_p, c_p, c_p]),
    "cover_actions_to_histories": (c_i, [c_p, c_ll, c_ll, c_i, c_i, c_p, c_p, c_i, c_f, c_p, c_p, c_p]),
    "cover_resample_axis": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p]),
    "cover_u8_hwc_to_f32_chw_norm": (c_i, [c_p, c_p, c_i, c_i, _P(c_f), _P(c_f), c_p]),
    "cover_u8_hwc_to_f32_chw_scale_norm": (c_i, [c_p, c_p, c_i, c_i, c_f, _P(c_f), _P(c_f), c_p]),
    "cover_resize_bilinear_pad_f32": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "cover_vit_workspace_bytes": (C.c_size_t, [_P(VitDesc), c_i, c_i]),
    "cover_vit_forward": (c_i, [_P(VitDesc), c_p, c_i, c_i, c_p, Workspace, c_i, c_p]),
    "cover_decoder_workspace_bytes": (C.c_size_t, [_P(DecDesc), c_i]),
    "cover_decoder_forward": (c_i, [_P(DecDesc), _P(DecPass), c_p, Workspace, c_i, c_p]),
    "cover_graph_begin": (c_i, [c_p]),
    "cover_graph_end": (c_i, [c_p, _P(c_p)]),
    "cover_graph_launch": (c_i, [c_p, c_p]),
    "cover_graph_destroy": (c_i, [c_p]),
    "cover_timer_create": (c_i, [_P(c_p)]),
    "cover_timer_start": (c_i, [c_p, c_p]),
    "cover_timer_stop": (c_i, [c_p, c_p, _P(c_f)]),
    "cover_timer_destroy": (c_i, [c_p]),
    "cover_stream_sync": (c_i, [c_p]),
    "cover_profile_begin": (c_i, [c_i]),
    "cover_profile_end": (c_i, [_P(C.c_double), _P(C.c_longlong), _P(C.c_double)]),
    "cover_profile_end_n": (c_i, [_P(C.c_double), _P(C.c_longlong), _P(C.c_double), c_i]),
    "cover_sizeof": (C.c_size_t, [C.c_char_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libcover_hip.so (once). Raises CoverError if it has not been built: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CoverError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). cover_vla_amd has no CPU fallback.")
    h = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(h, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = h
    check_abi()
    return _lib


def check_abi() -> None:
    h = _lib
    v = h.cover_abi_version()
    if v != 1:
        raise CoverError(f"libcover_hip ABI version {v}, binding expects 1")
    for cname, st in _STRUCTS.items():
        n = h.cover_sizeof(cname.encode())
        if n != C.sizeof(st):
            raise CoverError(f"struct {cname}: library sizeof {n} != binding sizeof {C.sizeof(st)}")


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = _lib.cover_last_error().decode(errors="replace") if _lib is not None else ""
        raise CoverError(f"{what or 'libcover_hip call'} failed ({rc}): {msg}")
