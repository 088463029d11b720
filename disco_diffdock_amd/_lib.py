"""ctypes binding of libddk.so (include/ddk.h).  There is NO fallback: if the HIP library is missing
or fails to load, importing the operators raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DDK_LIB') or os.path.join(_HERE, 'libddk.so')   # DDK_LIB: an alternative build of the library (kernel experiments)


class ddk_config(C.Structure):
    _fields_ = [('ns', C.c_int32), ('nv', C.c_int32), ('num_conv_layers', C.c_int32),
                ('sigma_embed_dim', C.c_int32), ('distance_embed_dim', C.c_int32), ('cross_distance_embed_dim', C.c_int32),
                ('lig_max_radius', C.c_float), ('rec_max_radius', C.c_float), ('cross_max_distance', C.c_float),
                ('center_max_distance', C.c_float), ('dynamic_max_cross', C.c_int32), ('embedding_scale', C.c_float),
                ('scale_by_sigma', C.c_int32), ('no_torsion', C.c_int32), ('batch_norm', C.c_int32),
                ('latent_dim', C.c_int32), ('latent_vocab', C.c_int32), ('latent_droprate', C.c_float),
                ('lm_embedding_dim', C.c_int32),
                ('tr_sigma_min', C.c_float), ('tr_sigma_max', C.c_float), ('rot_sigma_min', C.c_float),
                ('rot_sigma_max', C.c_float), ('tor_sigma_min', C.c_float), ('tor_sigma_max', C.c_float),
                ('device', C.c_int32), ('all_atoms', C.c_int32), ('num_confidence_outputs', C.c_int32),
                ('confidence_no_batchnorm', C.c_int32), ('conv_kernel', C.c_int32), ('deterministic', C.c_int32), ('confidence_mode', C.c_int32)]


class ddk_complex_desc(C.Structure):
    _fields_ = [('n_lig', C.c_int32), ('n_rec', C.c_int32), ('n_bond_edges', C.c_int32), ('n_rot', C.c_int32),
                ('n_rec_edges', C.c_int32), ('rec_feat_dim', C.c_int32),
                ('lig_x', C.c_void_p), ('bond_index', C.c_void_p), ('bond_attr', C.c_void_p), ('edge_mask', C.c_void_p),
                ('mask_rotate', C.c_void_p), ('rec_x', C.c_void_p), ('rec_pos', C.c_void_p), ('rec_edge_index', C.c_void_p)]


class ddk_atoms_desc(C.Structure):
    _fields_ = [('n_atom', C.c_int32), ('n_atom_edges', C.c_int32), ('atom_x', C.c_void_p), ('atom_pos', C.c_void_p),
                ('atom_edge_index', C.c_void_p), ('atom_rec_index', C.c_void_p)]


class ddk_trajectory(C.Structure):
    # device arrays of ddk_sample_trajectory's record, member order of include/ddk.h (tests/test_trajectory_host.py compares the two)
    _fields_ = [('pos', C.c_void_p), ('scores', C.c_void_p), ('perturb', C.c_void_p), ('edge_counts', C.c_void_p)]


class ddk_perturbation(C.Structure):
    # device arrays of ddk_rng_perturbation's result, member order of include/ddk.h
    _fields_ = [('tr_update', C.c_void_p), ('rot_update', C.c_void_p), ('tor_update', C.c_void_p),
                ('tr_score', C.c_void_p), ('rot_score', C.c_void_p), ('tor_score', C.c_void_p)]


class ddk_match_options(C.Structure):
    # the HOST options of ddk_conformer_match, member order of include/ddk.h
    _fields_ = [('popsize', C.c_int32), ('maxiter', C.c_int32), ('tol', C.c_float), ('polish_iters', C.c_int32), ('n_islands', C.c_int32),
                ('seed', C.c_uint64), ('stream_id', C.c_uint64)]


_lib = None

# every symbol include/ddk.h declares (tests check that the library exports all of them)
SYMBOLS = ['ddk_create', 'ddk_destroy', 'ddk_last_error', 'ddk_version', 'ddk_load_weights', 'ddk_finalize_weights',
           'ddk_set_score_norm_tables', 'ddk_tp_forward', 'ddk_tp_backward', 'ddk_rtp_forward', 'ddk_rtp_backward', 'ddk_rtp_backward_workspace', 'ddk_rconv_forward', 'ddk_rconv_backward', 'ddk_rconv_workspace', 'ddk_rhid_forward', 'ddk_rhid_backward', 'ddk_rhid_workspace', 'ddk_hconv_forward', 'ddk_hconv_backward', 'ddk_hconv_workspace', 'ddk_eemb_forward', 'ddk_eemb_backward', 'ddk_eemb_workspace', 'ddk_eemb_latent_forward', 'ddk_eemb_latent_backward', 'ddk_eemb_latent_workspace', 'ddk_gumbel_softmax_batch', 'ddk_gumbel_softmax_batch_backward', 'ddk_gumbel_pick_samples', 'ddk_rng_latent_keep', 'ddk_node_cross_entropy_batch', 'ddk_node_cross_entropy_batch_backward', 'ddk_rng_decoding_index', 'ddk_seg_sum', 'ddk_conv_forward', 'ddk_complex_create', 'ddk_complex_destroy',
           'ddk_score_forward', 'ddk_se3_update', 'ddk_sample', 'ddk_last_graph_stats', 'ddk_last_node_features',
           'ddk_profile_enable', 'ddk_profile_read', 'ddk_profile_read_forwards', 'ddk_set_latents', 'ddk_set_guidance',
           'ddk_set_keep_receptor_features', 'ddk_randomize_position', 'ddk_complex_set_atoms',
           'ddk_confidence_forward', 'ddk_score_confidence', 'ddk_pose_metrics', 'ddk_build_graph', 'ddk_set_receptive_field_pruning', 'ddk_ar_logits', 'ddk_ar_decode', 'ddk_confidence_status',
           'ddk_sample_trajectory', 'ddk_pose_pairwise_rmsd', 'ddk_pose_cluster',
           'ddk_ligand_automorphisms_workspace', 'ddk_ligand_automorphisms',
           'ddk_receptor_knn_graph_workspace', 'ddk_receptor_knn_graph', 'ddk_radius_graph_workspace', 'ddk_radius_graph',
           'ddk_ligand_transformation_mask_workspace', 'ddk_ligand_transformation_mask',
           'ddk_rng_noise', 'ddk_rng_initial', 'ddk_rng_uniform',
           'ddk_so3_rows', 'ddk_torus_score', 'ddk_rng_perturbation', 'ddk_score_matching_loss',
           'ddk_conformer_match_workspace', 'ddk_conformer_rmsd', 'ddk_conformer_match',
           'ddk_rng_perturbation_batch', 'ddk_rng_forward_times', 'ddk_modify_conformer_batch', 'ddk_randomize_position_batch', 'ddk_score_matching_loss_batch',
           'ddk_score_matching_loss_batch_backward']

# test hooks (include/ddk_debug.h): not part of the drop-in boundary
DEBUG_SYMBOLS = ['ddk_debug_export', 'ddk_debug_read_edges', 'ddk_debug_conf_counts', 'ddk_debug_conf_table', 'ddk_debug_conf_nodes', 'ddk_debug_conf_edges', 'ddk_debug_kabsch', 'ddk_debug_axis_angle', 'ddk_debug_set_layer0_dedup', 'ddk_debug_read_patch', 'ddk_debug_split3', 'ddk_debug_conv_trace', 'ddk_debug_pool_stats', 'ddk_debug_set_conv_workgroups', 'ddk_debug_set_alloc_limit', 'ddk_debug_cross_mirror']


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} not found: build the HIP extension first (python -m disco_diffdock_amd.build). '
                           'disco_diffdock_amd has no CPU fallback.')
    import torch  # noqa: F401  (first: libddk.so must bind to the HIP runtime PyTorch-ROCm ships; loaded before torch it binds to /opt/rocm's copy,
    #                and two HIP runtimes in one process leave the second without a device: "no ROCm-capable device is detected")
    L = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS + DEBUG_SYMBOLS if not hasattr(L, s)]
    if missing:      # a library built from older sources: fail here, not with an AttributeError at the first call of the new entry
        raise RuntimeError(f'{LIB_PATH} does not export {", ".join(missing)}: it is stale, build the HIP extension again '
                           '(python -m disco_diffdock_amd.build). disco_diffdock_amd has no CPU fallback.')
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.ddk_create.argtypes = [C.POINTER(ddk_config), C.POINTER(vp)]
    L.ddk_destroy.argtypes = [vp]
    L.ddk_destroy.restype = None
    L.ddk_last_error.argtypes = [vp]
    L.ddk_last_error.restype = C.c_char_p
    L.ddk_version.restype = C.c_char_p
    L.ddk_load_weights.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
    L.ddk_finalize_weights.argtypes = [vp]
    L.ddk_set_score_norm_tables.argtypes = [vp, vp, i32, vp, i32]
    L.ddk_tp_forward.argtypes = [vp, i32, vp, vp, vp, i64, vp, vp]
    L.ddk_tp_backward.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.ddk_rtp_forward.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i64), i32, vp, vp, i64, vp, vp]
    L.ddk_rtp_backward.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i64), i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_rtp_backward_workspace.argtypes = [i32, i64, i32]
    L.ddk_rtp_backward_workspace.restype = i64
    # ctx, layer, x_nodes, n_in, n_out, edge_src, edge_dst, src_order, src_ptr, [dst_order, dst_ptr,] sh, h, group_offsets, n_groups, w2, b2, ...
    L.ddk_rconv_forward.argtypes = [vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64), i32, vp, vp, i64, vp, vp, vp]
    L.ddk_rconv_backward.argtypes = [vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_rconv_workspace.argtypes = [i32, i64, i32, i64, i64, i32]
    L.ddk_rconv_workspace.restype = i64
    # ctx, xs, n_nodes, edge_src, edge_dst, [src_order, src_ptr, dst_order, dst_ptr,] emb, [h,] group_offsets, n_groups, w1, ...
    L.ddk_rhid_forward.argtypes = [vp, vp, i64, vp, vp, vp, C.POINTER(i64), i32, vp, vp, f32, C.c_uint64, i64, vp, vp]
    L.ddk_rhid_backward.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), i32, vp, vp, f32, i64, vp, vp, vp, vp, vp, vp]
    L.ddk_rhid_workspace.argtypes = [i64, i32, i64]
    L.ddk_rhid_workspace.restype = i64
    # ctx, head, x_nodes, n_in, n_out, edge_src, edge_dst, src_order, src_ptr, [dst_order, dst_ptr,] sh, h, w2, b2, ...
    L.ddk_hconv_forward.argtypes = [vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.ddk_hconv_backward.argtypes = [vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.ddk_hconv_workspace.argtypes = [i32, i64, i64, i64, i32]
    L.ddk_hconv_workspace.restype = i64
    eemb = [vp, vp, i64, vp, i64, vp, vp, vp, i32, vp, i64, vp, f32, f32, i32, vp, vp, vp, vp, f32, C.c_uint64]      # ctx and the operands both directions read
    L.ddk_eemb_forward.argtypes = eemb + [i64, vp, vp, vp]
    L.ddk_eemb_backward.argtypes = eemb + [vp, i64, vp, vp, vp, vp, vp, vp]
    L.ddk_eemb_workspace.argtypes = [i64, i32]
    L.ddk_eemb_workspace.restype = i64
    latent = [vp, vp, i32, i32, vp, vp]      # lat_a, lat_b, L, zero_latent, unc_a, uemb
    L.ddk_eemb_latent_forward.argtypes = eemb + latent + [i64, vp, vp, vp]
    L.ddk_eemb_latent_backward.argtypes = eemb + latent + [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_eemb_latent_workspace.argtypes = [i64, i32, i32]
    L.ddk_eemb_latent_workspace.restype = i64
    gumbel = [vp, i32, i32, vp, i64, vp, i64, vp, vp, f32]      # ctx, G, D, a table pair with its node counts, lig_ptr, rec_ptr, T
    L.ddk_gumbel_softmax_batch.argtypes = gumbel + [C.c_uint64, vp, i32, i32, vp, vp, vp, vp, vp]
    L.ddk_gumbel_softmax_batch_backward.argtypes = gumbel + [vp, vp, vp, vp, vp]
    # ctx, B, D, logit_l, n_lig, logit_r, n_rec, T, seed, stream_id, sample0, draw, lig_latent, rec_latent, choices, stream
    L.ddk_gumbel_pick_samples.argtypes = [vp, i32, i32, vp, i64, vp, i64, f32, C.c_uint64, C.c_uint64, i32, i32, vp, vp, vp, vp]
    L.ddk_rng_latent_keep.argtypes = [vp, C.c_uint64, i32, vp, i32, i32, f32, vp]
    node_ce = [vp, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32]      # ctx, G, D, the logit pair with its node counts, lig_ptr, rec_ptr, the teacher pair, column, soft
    L.ddk_node_cross_entropy_batch.argtypes = node_ce + [vp, vp, vp, vp, vp]
    L.ddk_node_cross_entropy_batch_backward.argtypes = node_ce + [vp, vp, vp, vp, vp, vp]
    L.ddk_rng_decoding_index.argtypes = [vp, C.c_uint64, i32, vp, i32, i32, i32, vp]
    L.ddk_seg_sum.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp]
    L.ddk_conv_forward.argtypes = [vp, i32, vp, i64, vp, vp, C.POINTER(i64), vp, vp, vp, vp]
    L.ddk_complex_create.argtypes = [vp, C.POINTER(ddk_complex_desc), i32, C.POINTER(vp)]
    L.ddk_complex_destroy.argtypes = [vp, vp]
    L.ddk_complex_destroy.restype = None
    L.ddk_score_forward.argtypes = [vp, vp, i32, vp, f32, f32, f32, vp, vp, vp, vp]
    L.ddk_se3_update.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ddk_randomize_position.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ddk_complex_set_atoms.argtypes = [vp, vp, vp, vp, vp, i32]
    L.ddk_confidence_forward.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ddk_score_confidence.argtypes = [vp, vp, i32, vp, C.c_float, C.c_float, C.c_float, vp, vp]
    L.ddk_pose_metrics.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp]
    L.ddk_pose_pairwise_rmsd.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp]
    L.ddk_pose_cluster.argtypes = [vp, i32, vp, vp, f32, vp, vp, vp, vp]
    L.ddk_ligand_automorphisms_workspace.argtypes = [i32, i32]
    L.ddk_ligand_automorphisms_workspace.restype = i64
    L.ddk_ligand_automorphisms.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    for name in ('ddk_receptor_knn_graph_workspace', 'ddk_radius_graph_workspace', 'ddk_ligand_transformation_mask_workspace'):
        getattr(L, name).argtypes = [i32, i32]
        getattr(L, name).restype = i64
    L.ddk_receptor_knn_graph.argtypes = [vp, i32, vp, f32, i32, vp, i32, vp, vp, vp]
    L.ddk_radius_graph.argtypes = [vp, i32, vp, f32, i32, vp, i32, vp, vp, vp]
    L.ddk_ligand_transformation_mask.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, vp, vp]
    u64 = C.c_uint64      # (seed, stream_id) of the ddk_rng_* calls: DDK_RNG_LAYOUT of include/ddk.h
    L.ddk_rng_noise.argtypes = [vp, u64, u64, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.ddk_rng_initial.argtypes = [vp, u64, u64, i32, i32, i32, f32, i32, vp, vp, vp, vp]
    L.ddk_rng_uniform.argtypes = [vp, u64, u64, i32, i32, i32, vp, vp]
    L.ddk_so3_rows.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.ddk_torus_score.argtypes = [vp, i64, vp, i32, vp, vp]
    L.ddk_rng_perturbation.argtypes = [vp, u64, u64, i32, i32, i32, i32, f32, f32, i32, vp, vp, C.POINTER(ddk_perturbation), vp]
    L.ddk_score_matching_loss.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, f32, vp, vp]
    # the ragged batch forms: ctx, [seed,] G, per-graph device tables ...
    L.ddk_rng_perturbation_batch.argtypes = [vp, u64, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, C.POINTER(ddk_perturbation), vp]
    L.ddk_rng_forward_times.argtypes = [vp, u64, i32, vp, i32, i32, vp]
    L.ddk_modify_conformer_batch.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_randomize_position_batch.argtypes = [vp, u64, i32, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, f32, vp, vp, vp]
    L.ddk_score_matching_loss_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_score_matching_loss_batch_backward.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ddk_conformer_match_workspace.argtypes = [i32, i32, i32, i32]
    L.ddk_conformer_match_workspace.restype = i64
    L.ddk_conformer_rmsd.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.ddk_conformer_match.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(ddk_match_options), vp, vp, vp, vp, vp, vp]
    L.ddk_sample.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.ddk_sample_trajectory.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, C.POINTER(ddk_trajectory), vp]
    L.ddk_last_graph_stats.argtypes = [vp, vp, vp, vp]
    L.ddk_build_graph.argtypes = [vp, vp, C.c_int32, vp, C.c_float, vp, vp, C.c_int64, vp, vp]
    L.ddk_last_node_features.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ddk_set_latents.argtypes = [vp, vp, vp, vp, f32]
    L.ddk_set_guidance.argtypes = [vp, vp, f32, f32, f32]
    L.ddk_set_keep_receptor_features.argtypes = [vp, vp, i32]
    L.ddk_profile_enable.argtypes = [vp, i32]
    L.ddk_set_receptive_field_pruning.argtypes = [vp, i32]
    L.ddk_ar_logits.argtypes = [vp, vp, i32, vp, vp]
    L.ddk_confidence_status.argtypes = [vp, vp, vp, vp]
    L.ddk_ar_decode.argtypes = [vp, vp, i32, vp, f32, vp, i32, i32, vp, vp, vp, vp]
    L.ddk_profile_read.argtypes = [vp, vp, i32]
    L.ddk_profile_read_forwards.argtypes = [vp, vp, i32]
    L.ddk_debug_export.argtypes = [vp, C.c_char_p, vp, i64]
    L.ddk_debug_export.restype = i64
    _declare_debug(L)
    _lib = L
    return L


def _declare_debug(L):
    import ctypes as C
    L.ddk_debug_read_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64]
    L.ddk_debug_cross_mirror.argtypes = [C.c_void_p, C.c_void_p]
    L.ddk_debug_kabsch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ddk_debug_axis_angle.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ddk_debug_set_layer0_dedup.argtypes = [C.c_void_p, C.c_int32]
    L.ddk_debug_read_patch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.ddk_debug_split3.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ddk_debug_conv_trace.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.ddk_debug_pool_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.ddk_debug_set_conv_workgroups.argtypes = [C.c_void_p, C.c_int32]
    L.ddk_debug_set_alloc_limit.argtypes = [C.c_void_p, C.c_int64]
    L.ddk_debug_conf_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ddk_debug_conf_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.ddk_debug_conf_nodes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.ddk_debug_conf_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
