"""ctypes binding of liblgu_corr.so (C ABI declared in include/lgu_corr.h).

There is NO fallback: if the shared library is missing or fails to load, every
operator raises.  Build it with `python __graft_entry__.py build` (or
`lgu_slam_amd._build.build()`), which needs only hipcc.
"""
import ctypes
import os

from . import _build

_c_float_p = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_int = ctypes.c_int


class FlowConv7Args(ctypes.Structure):
    """lgu_flow_conv7_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("H", _int), ("W", _int)]


class Conv3Args(ctypes.Structure):
    """lgu_conv3_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("H", _int), ("W", _int),
                ("Cout", _int), ("flags", _int)]


class HeadArgs(ctypes.Structure):
    """lgu_head_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("H", _int), ("W", _int),
                ("Cout", _int), ("flags", _int)]


class Conv3FanoutArgs(ctypes.Structure):
    """lgu_conv3_fanout_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp * 3), ("bias", _vp * 3), ("out", _vp * 3), ("N", _int), ("H", _int), ("W", _int),
                ("G", _int), ("flags", _int)]


class HeadPairArgs(ctypes.Structure):
    """lgu_head_pair_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp * 2), ("wpack", _vp * 2), ("bias", _vp * 2), ("out", _vp * 2), ("coords", _vp), ("N", _int), ("H", _int),
                ("W", _int), ("flags", _int)]


class UpmaskArgs(ctypes.Structure):
    """lgu_upmask_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("H", _int), ("W", _int), ("flags", _int)]


class UpmaskUpsArgs(ctypes.Structure):
    """lgu_upmask_ups_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("disps", _vp), ("ix", _vp), ("disps_up", _vp), ("U", _int),
                ("N", _int), ("ht", _int), ("wd", _int), ("flags", _int)]


class Conv1Args(ctypes.Structure):
    """lgu_conv1_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("Cin", _int), ("H", _int), ("W", _int),
                ("flags", _int)]


class GruConvArgs(ctypes.Structure):
    """lgu_gruconv_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("seg", _vp * 4), ("wpack", _vp), ("bias", _vp), ("k0", _vp), ("k1", _vp), ("net", _vp), ("z", _vp),
                ("out0", _vp), ("out1", _vp), ("seg_ch", _int * 4), ("nseg", _int), ("N", _int), ("H", _int), ("W", _int),
                ("Cout", _int), ("mode", _int), ("flags", _int)]


class EncConvArgs(ctypes.Structure):
    """lgu_encconv_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("res", _vp), ("out", _vp), ("dpack", _vp), ("dbias", _vp), ("r", _vp),
                ("N", _int), ("H", _int), ("W", _int), ("Cin", _int), ("Cout", _int), ("stride", _int), ("flags", _int)]


class EncConvNormArgs(ctypes.Structure):
    """lgu_encconv_norm_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("dpack", _vp), ("dbias", _vp), ("r", _vp), ("y", _vp),
                ("stats_x", _vp), ("stats_y", _vp), ("keep", _vp), ("stats_out", _vp), ("stats_r", _vp), ("eps", ctypes.c_float),
                ("N", _int), ("H", _int), ("W", _int), ("Cin", _int), ("Cout", _int), ("stride", _int), ("mode", _int), ("flags", _int)]


class EncStatsArgs(ctypes.Structure):
    """lgu_encstats_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("acc", _vp), ("mean_rstd", _vp), ("planes", ctypes.c_long), ("cnt", ctypes.c_long), ("eps", ctypes.c_float)]


class EncStemArgs(ctypes.Structure):
    """lgu_encstem_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("N", _int), ("H", _int), ("W", _int), ("Cin", _int),
                ("Cout", _int), ("flags", _int)]


class EncOutArgs(ctypes.Structure):
    """lgu_encout_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("out", _vp), ("inp", _vp), ("N", _int), ("H", _int), ("W", _int),
                ("Cin", _int), ("Cout", _int), ("flags", _int)]


class GaussHeadArgs(ctypes.Structure):
    """lgu_gausshead_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("x", _vp), ("wpack", _vp), ("bias", _vp), ("mean_ofs", _vp), ("cov_raw", _vp), ("hidden", _vp), ("E", _int),
                ("H", _int), ("W", _int), ("flags", _int)]


class CloudArgs(ctypes.Structure):
    """lgu_cloud_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("thresh", _vp), ("floor", _vp), ("images", _vp),
                ("scratch", _vp), ("offsets", _vp), ("points", _vp), ("colors", _vp), ("cap", ctypes.c_longlong), ("np", _int),
                ("nd", _int), ("ht", _int), ("wd", _int), ("num", _int), ("min_count", _int), ("ni", _int), ("H", _int), ("W", _int),
                ("stride", _int), ("phase", _int), ("color_u8", _int)]


class RenderArgs(ctypes.Structure):
    """lgu_render_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("points", _vp), ("colors", _vp), ("view", _vp), ("intrinsics", _vp), ("cameras", _vp), ("scratch", _vp),
                ("image", _vp), ("depth", _vp), ("npoints", ctypes.c_longlong), ("near", ctypes.c_float),
                ("camera_scale", ctypes.c_float), ("ncam", _int), ("H", _int), ("W", _int), ("point_size", _int), ("color_u8", _int),
                ("background", ctypes.c_ubyte * 3), ("camera_color", ctypes.c_ubyte * 3)]


class IntakeCamera(ctypes.Structure):
    """lgu_intake_camera of include/lgu_corr.h: 22 doubles."""
    _fields_ = [("k", ctypes.c_double * 4), ("kn", ctypes.c_double * 4), ("ir", ctypes.c_double * 9), ("d", ctypes.c_double * 5)]


class IntakeArgs(ctypes.Structure):
    """lgu_intake_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("raw", _vp), ("image", _vp), ("inputs", _vp), ("cam_table", _vp), ("cam", IntakeCamera * 2),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3), ("N", _int), ("h0", _int), ("w0", _int), ("C", _int),
                ("h1", _int), ("w1", _int), ("top", _int), ("left", _int), ("H", _int), ("W", _int), ("ncam", _int), ("path", _int)]


class IntakeDepthArgs(ctypes.Structure):
    """lgu_intake_depth_args of include/lgu_corr.h, passed by value."""
    _fields_ = [("raw", _vp), ("out", _vp), ("scale", ctypes.c_double), ("N", _int), ("h0", _int), ("w0", _int), ("h1", _int),
                ("w1", _int), ("top", _int), ("left", _int), ("H", _int), ("W", _int), ("src_u16", _int)]


# name -> argument types; the return type is int unless RESTYPES names another
SIGNATURES = {
    "lgu_defcorr_fwd_f32": [_vp, _vp, _vp, _vp] + [_int] * 6 + [_vp],
    "lgu_defcorr_bwd_f32": [_vp] * 6 + [_int] * 6 + [_vp],
    "lgu_corridx_fwd_f32": [_vp, _vp, _vp] + [_int] * 6 + [_vp],
    "lgu_corridx_bwd_f32": [_vp] * 4 + [_int] * 6 + [_vp],
    "lgu_gaussmask_fwd_f32": [_vp] * 4 + [_int] * 6 + [_vp],
    "lgu_gaussmask_bwd_f32": [_vp] * 6 + [_int] * 6 + [_vp],
    "lgu_defcorr_pyramid_fwd_f32": [ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int,
                                    ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _vp],
    "lgu_defcorr_pyramid_slots_fwd_f32": [ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int,
                                          ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _vp],
    "lgu_volume_pyramid_f32": [_vp, _vp, _vp, ctypes.POINTER(_vp), _int, _int, _int, _int, _int, _int, _int, _vp],
    "lgu_volume_pyramid_tiled_f32": [_vp, _vp, _vp, ctypes.POINTER(_vp), _int, _int, _int, _int, _int, _int, _int, _vp],
    "lgu_volume_pyramid_h16": [_vp, _vp, _vp, ctypes.POINTER(_vp), _int, _int, _int, _int, _int, _int, _int, _int, _vp],
    "lgu_volume_pyramid_det": [_vp, _vp, _vp, _int, _vp, _int, ctypes.POINTER(_vp)] + [_int] * 8 + [_vp],
    "lgu_volume_build_pyramid_f32": [_vp] * 5 + [_int, ctypes.POINTER(_vp)] + [_int] * 6 + [_vp],
    "lgu_volume_build_pyramid_h16": [_vp] * 5 + [_int, ctypes.POINTER(_vp)] + [_int] * 6 + [_vp],
    "lgu_gaussian_params": [_vp] * 5 + [_int] * 4 + [ctypes.c_float, _vp],
    "lgu_probe_mask_scale_f32": [_vp, _vp, _int, _int, _int, _int, _vp],
    "lgu_offset_conv_frames_h16": [_vp] * 7 + [_int] * 5 + [_vp],
    "lgu_offset_heads_mark": [_vp, _vp, _int, _vp, _int, _vp, _vp, _vp],
    "lgu_offset_conv_worklist_h16": [_vp] * 4 + [_int] + [_vp] * 5 + [_int] * 4 + [_vp],
    "lgu_offset_heads_combine_f32": [_vp] * 5 + [_int] * 2 + [_vp, _vp],
    "lgu_offsets_finalize": [_vp] * 5 + [_int] * 7 + [ctypes.c_float, _vp],
    "lgu_offsets_finalize_masked": [_vp] * 3 + [_int] + [_vp] * 3 + [_int] * 7 + [ctypes.c_float, _vp],
    "lgu_volume_retile_f32": [_vp, _vp, ctypes.c_longlong, _int, _int, _int, _vp],
    "lgu_lowmem_defsample_fwd_f32": [_vp] * 5 + [_int] * 9 + [_vp],
    "lgu_altcorr_fwd_f32": [_vp] * 4 + [_int] * 8 + [_vp],
    "lgu_lowmem_defsample_fwd_h16": [_vp] * 5 + [_int] * 9 + [_vp],
    "lgu_altcorr_fwd_h16": [_vp] * 4 + [_int] * 8 + [_vp],
    "lgu_lowmem_pyramid_fwd_h16": [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int, _int, _int,
                                   ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _int, _vp, _vp, _vp],
    "lgu_lowmem_pyramid_chunked_fwd_h16": [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int, _int, _int,
                                   ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _int, _vp, _vp, _vp],
    "lgu_lowmem_pyramid_chunked_fwd_f32": [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int, _int, _int,
                                   ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _int, _vp, _vp, _vp],
    # fmap1, fmap2[], coords, offsets[], out, L, lbase, B, H1, W1, H2[], W2[], C, NO, off_row, radius, ii, jj, chunked, stream
    "lgu_lowmem_pyramid_calls_fwd_h16": [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int, _int,
                                         ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _vp, _int, _vp, _vp, _int, _vp],
    "lgu_lowmem_pyramid_fwd_f32": [_vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp, _int, _int, _int, _int, _int, _int,
                                   ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _int, _vp, _vp, _vp],
    "lgu_ba_build_f32": [_vp] * 14 + [_int] * 3 + [_vp],
    "lgu_ba_build_slices": [_int],
    "lgu_ba_accum_f32": [_vp] * 4 + [_int] * 2 + [_vp],
    "lgu_ba_depth_system_f32": [_vp] * 8 + [_int] + [_vp] * 2 + [_int] * 2 + [_vp],
    "lgu_ba_depth_update_f32": [_vp] * 8 + [_int] * 2 + [_vp],
    "lgu_ba_scatter_sum_f64": [_vp] * 5 + [_int] * 2 + [ctypes.c_double, _vp],
    "lgu_ba_eet_f32": [_vp] * 4 + [_int] * 2 + [_vp],
    "lgu_ba_ev_f32": [_vp] * 5 + [_int] * 2 + [_vp],
    "lgu_ba_evt_f32": [_vp] * 4 + [_int] * 3 + [_vp],
    "lgu_ba_solve_f64": [_vp, _vp, _vp, _int, ctypes.c_double, ctypes.c_double, _vp],
    "lgu_ba_solve_blocked_f64": [_vp, _vp, _vp, _vp, _int, ctypes.c_double, ctypes.c_double, _vp],
    "lgu_ba_pose_retr_f32": [_vp] * 2 + [_int] * 2 + [_vp],
    "lgu_ba_assemble_f64": [_vp] * 14 + [_int, _vp],
    "lgu_ba_disp_retr_f32": [_vp] * 3 + [_int] * 2 + [_vp],
    "lgu_altcorr_bwd_f32": [_vp] * 6 + [_int] * 8 + [_vp],
    "lgu_defcorr_pyramid_enc_fwd_f32": [ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp), _vp, _vp, _vp, _int, _int, _int,
                                        _int, ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int, _int, _vp],
    # poses, np, disps, nd, ht, wd, intrinsics, ...
    "lgu_frame_distance_f32": [_vp, _int, _vp, _int, _int, _int, _vp, _vp, _vp, _int, ctypes.c_float, _vp, _vp],
    "lgu_projmap_f32": [_vp, _int, _vp, _int, _int, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp],
    "lgu_depth_filter_f32": [_vp, _int, _vp, _int, _int, _int, _vp, _vp, _vp, _int, _vp, _vp],
    "lgu_iproj_f32": [_vp, _int, _vp, _int, _int, _int, _vp, _vp, _vp],
    # poses, disps, intrinsics, ii, jj, B, np, nd, ni, ht, wd, num, ...
    "lgu_projective_transform_f32": [_vp] * 5 + [_int] * 8 + [_vp] * 6,
    "lgu_motion_features_f32": [_vp] * 6 + [_int] * 7 + [ctypes.c_float] + [_vp] * 4,
    # src, index, outer, n, inner, M, out, stream
    "lgu_scatter_mean_f32": [_vp, _vp, _int, _int, ctypes.c_longlong, _int, _vp, _vp],
    "lgu_scatter_mean_h16": [_vp, _vp, _int, _int, ctypes.c_longlong, _int, _vp, _vp],
    # data, mask, B, ht, wd, flags, out, stream
    "lgu_cvx_upsample_f32": [_vp, _vp] + [_int] * 4 + [_vp, _vp],
    # disps, N, ht, wd, ix, U, mask, flags, disps_up, stream
    "lgu_upsample_disps_f32": [_vp, _int, _int, _int, _vp, _int, _vp, _int, _vp, _vp],
    # KAN-bias GRU: net, weight, bias, E, HW, partial, glo, stream
    "lgu_kangru_context_f32": [_vp] * 3 + [_int] * 2 + [_vp] * 3,
    "lgu_kangru_context_h16": [_vp] * 3 + [_int] * 2 + [_vp] * 3,
    # glo, grid, wpack, E, out, stream
    "lgu_kan_heads_f32": [_vp] * 3 + [_int] + [_vp] * 2,
    "lgu_kan_heads_h16": [_vp] * 3 + [_int] + [_vp] * 2,
    # cz, cr, kz, kr, net, E, HW, z, net_inp, stream
    "lgu_kangru_gates_f32": [_vp] * 5 + [_int] * 2 + [_vp] * 3,
    "lgu_kangru_gates_h16": [_vp] * 5 + [_int] * 2 + [_vp] * 3,
    # cq, kq, z, net, E, HW, out, stream
    "lgu_kangru_blend_f32": [_vp] * 4 + [_int] * 2 + [_vp] * 2,
    "lgu_kangru_blend_h16": [_vp] * 4 + [_int] * 2 + [_vp] * 2,
    # proximity edges: dist, known_ii, known_jj, num_known, t, t0, t1, rad, nms, thresh, max_factors, stereo, e_ii, e_jj,
    # capacity, count, stream
    "lgu_proximity_select_small": [_vp] * 3 + [_int] * 6 + [ctypes.c_double, ctypes.c_longlong, _int, _vp, _vp,
                                                            ctypes.c_longlong, _vp, _vp],
    # dist, known_ii, known_jj, num_known, t, t0, t1, rad, nms, thresh, stereo, keys, work, stream
    "lgu_proximity_keys": [_vp] * 3 + [_int] * 6 + [ctypes.c_double, _int, _vp, _vp, _vp],
    # sorted_keys, work, t, t0, t1, rad, nms, max_factors, stereo, e_ii, e_jj, capacity, count, stream
    "lgu_proximity_select_sorted": [_vp] * 2 + [_int] * 5 + [ctypes.c_longlong, _int, _vp, _vp, ctypes.c_longlong, _vp, _vp],
    # Lie groups (group = LGU_LIE_SO3 / LGU_LIE_SE3).  Per element: group, inputs, n, out, stream
    "lgu_lie_inv_f32": [_int, _vp, _int, _vp, _vp],
    "lgu_lie_mul_f32": [_int, _vp, _vp, _int, _vp, _vp],
    "lgu_lie_retr_f32": [_int, _vp, _vp, _int, _vp, _vp],
    "lgu_lie_exp_f32": [_int, _vp, _int, _vp, _vp],
    "lgu_lie_log_f32": [_int, _vp, _int, _vp, _vp],
    "lgu_lie_matrix_f32": [_int, _vp, _int, _vp, _vp],
    # broadcast: group, G, ng, operand, width | transpose, rows, g_div, out, stream
    "lgu_lie_act_f32": [_int, _vp, ctypes.c_longlong, _vp, _int, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp],
    "lgu_lie_adj_f32": [_int, _vp, ctypes.c_longlong, _vp, _int, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp],
    # feature encoder: a, b, out, planes, hw, eps, mode, stream
    "lgu_instnorm_relu_f32": [_vp] * 3 + [ctypes.c_long] * 2 + [ctypes.c_float, _int, _vp],
    "lgu_instnorm_relu_h16": [_vp] * 3 + [ctypes.c_long] * 2 + [ctypes.c_float, _int, _vp],
    "lgu_instnorm_resident_limit": [_int],   # elem_bytes
    # img, out, n, hw, mean[3], std[3], stream
    "lgu_image_normalize_u8": [_vp, _vp, ctypes.c_long, ctypes.c_long, _c_float_p, _c_float_p, _vp],
    # motion encoder: {x, wpack, bias, out, N, H, W} by value, stream
    "lgu_flow_conv7_relu_h16": [FlowConv7Args, _vp],
    # 3x3 convolution, 128 in: {x, wpack, bias, out, N, H, W, Cout, flags} by value, stream
    "lgu_conv3x3_c128_h16": [Conv3Args, _vp],
    # the narrow 3x3 heads, 128 in, Cout 1 | 2: {x, wpack, bias, out, N, H, W, Cout, flags} by value, stream
    "lgu_head3x3_c128_h16": [HeadArgs, _vp],
    # 2 or 3 convolutions 128 -> 128 of one input: {x, wpack[3], bias[3], out[3], N, H, W, G, flags} by value, stream
    "lgu_conv3x3_fanout_c128_h16": [Conv3FanoutArgs, _vp],
    # delta[2] and weight[2] in one launch, edge-major: {x[2], wpack[2], bias[2], out[2], coords, N, H, W, flags} by value, stream
    "lgu_head3x3_pair_c128_h16": [HeadPairArgs, _vp],
    # the GRU's 3x3 convolutions, 448 in, with gates / blend: {seg[4], wpack, bias, k0, k1, net, z, out0, out1, seg_ch[4],
    # nseg, N, H, W, Cout, mode, flags} by value, stream
    "lgu_gruconv3x3_c448_h16": [GruConvArgs, _vp],
    # GraphAgg's upmask 1x1, 128 -> 576: {x, wpack, bias, out, N, H, W, flags} by value, stream
    "lgu_upmask1x1_c128_h16": [UpmaskArgs, _vp],
    # upmask + softmax + convex upsample: {x, wpack, bias, disps, ix, disps_up, U, N, ht, wd, flags} by value, stream
    "lgu_upmask_upsample_f32": [UpmaskUpsArgs, _vp],
    # 1x1 convolution, Cin <= 224 -> 128 (corr_encoder[0]): {x, wpack, bias, out, N, Cin, H, W, flags} by value, stream
    "lgu_conv1x1_o128_h16": [Conv1Args, _vp],
    # the encoders' residual-stage 3x3 convolutions with their tail and the 1x1 stride-2 branch: {x, wpack, bias, res, out,
    # dpack, dbias, r, N, H, W, Cin, Cout, stride, flags} by value, stream
    "lgu_encconv3x3_h16": [EncConvArgs, _vp],
    # the same convolutions with the feature encoder's instance norms folded in: {x, wpack, bias, out, dpack, dbias, r, y,
    # stats_x, stats_y, keep, stats_out, stats_r, eps, N, H, W, Cin, Cout, stride, mode, flags} by value, stream
    "lgu_encconv3x3_norm_h16": [EncConvNormArgs, _vp],
    # {acc, mean_rstd, planes, cnt, eps} by value, stream
    "lgu_encstats_finalize": [EncStatsArgs, _vp],
    "lgu_encstats_replicas": [],
    # the encoders' stem, 7x7 stride 2, 3 -> 32: {x, wpack, bias, out, N, H, W, Cin, Cout, flags} by value, stream
    "lgu_encstem7x7_h16": [EncStemArgs, _vp],
    # the encoders' output 1x1, 128 -> 128 | 256, with the tanh / relu split: {x, wpack, bias, out, inp, N, H, W, Cin, Cout,
    # flags} by value, stream
    "lgu_encout1x1_c128_h16": [EncOutArgs, _vp],
    # the Gaussian mask's parameter head, Linear(256,16) + tanh + 2 x Linear(16,2): {x, wpack, bias, mean_ofs, cov_raw, hidden,
    # E, H, W, flags} by value, stream
    "lgu_gaussian_head": [GaussHeadArgs, _vp],
    # the map export: {poses, disps, intrinsics, ix, thresh, floor, images, scratch, offsets, points, colors, cap, np, nd, ht,
    # wd, num, min_count, ni, H, W, stride, phase, color_u8} by value, stream
    "lgu_cloud_decide_f32": [CloudArgs, _vp],
    "lgu_cloud_write_f32": [CloudArgs, _vp],
    # the frame intake: {raw, image, inputs, cam_table, cam[2], mean[3], std[3], N, h0, w0, C, h1, w1, top, left, H, W, ncam,
    # path} by value, stream; {raw, out, scale, N, h0, w0, h1, w1, top, left, H, W, src_u16} by value, stream
    "lgu_intake_frame_u8": [IntakeArgs, _vp],
    "lgu_intake_depth_f32": [IntakeDepthArgs, _vp],
    # the offscreen view: {points, colors, view, intrinsics, cameras, scratch, image, depth, npoints, near, camera_scale, ncam,
    # H, W, point_size, color_u8, background[3], camera_color[3]} by value, stream
    "lgu_render_view": [RenderArgs, _vp],
    # size queries (host only) and the library's own description
    "lgu_ba_solve_blocked_work_doubles": [_int],
    "lgu_offsets_finalize_scratch_bytes": [_int],
    "lgu_cloud_scratch_bytes": [_int] * 3,
    "lgu_render_scratch_bytes": [_int] * 2,
    "lgu_proximity_prefix_len": [_int] * 4,
    "lgu_proximity_capacity": [_int] * 5 + [ctypes.c_longlong],
    "lgu_proximity_work_bytes": [_int] * 3,
    "lgu_version": [],
    "lgu_error_string": [_int],
    "lgu_debug_knobs_enabled": [],
}
RESTYPES = {name: ctypes.c_longlong for name in (
    "lgu_ba_solve_blocked_work_doubles", "lgu_offsets_finalize_scratch_bytes", "lgu_proximity_prefix_len", "lgu_proximity_capacity",
    "lgu_proximity_work_bytes", "lgu_cloud_scratch_bytes", "lgu_render_scratch_bytes")}
RESTYPES.update(lgu_instnorm_resident_limit=ctypes.c_long, lgu_version=ctypes.c_char_p, lgu_error_string=ctypes.c_char_p)

_lib = None


class LguLibraryError(RuntimeError):
    pass


class UnsupportedShape(RuntimeError):
    """The kernels do not serve this shape / argument pattern (LGU_E_UNSUPPORTED)."""


LGU_E_BADARG, LGU_E_UNSUPPORTED = 100001, 100002


def so_path():
    """The library this process loads.  LGU_LIB_PATH (experiments only: tools/ab_lib_*.sh) points at another build —
    variants are loaded from where they were built, the in-tree default library is never overwritten."""
    return os.environ.get("LGU_LIB_PATH") or _build.SO_PATH


def load():
    """Load the HIP library once; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    path = so_path()
    if not os.path.exists(path):
        raise LguLibraryError(
            "lgu_slam_amd: %s is missing — the gfx950 HIP kernels are not built and there is no CPU "
            "fallback. Run `python __graft_entry__.py build`." % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:  # pragma: no cover - depends on the ROCm install
        raise LguLibraryError("lgu_slam_amd: cannot load %s: %s" % (path, exc)) from exc
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch, let it surface
        fn.argtypes = argtypes
        fn.restype = RESTYPES.get(name, _int)
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().lgu_error_string(code).decode()
        raise (UnsupportedShape if code == LGU_E_UNSUPPORTED else RuntimeError)("%s failed: %s (code %d)" % (what, msg, code))


def version():
    return load().lgu_version().decode()


def debug_knobs_enabled():
    """True if the LGU_* debug variables are live in this process (LGU_DEBUG_KNOBS=1 when the library was loaded)."""
    return bool(load().lgu_debug_knobs_enabled())
