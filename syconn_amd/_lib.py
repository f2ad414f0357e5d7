"""ctypes binding of ``libsyconn_dense_hip.so`` (C ABI: ``include/syconn_dense.h``).

There is deliberately no fallback: if the shared library is missing (not built) loading raises, and if no MI355X is visible ``sd_init``
returns ``SD_ERR_NODEVICE`` which is raised as ``RuntimeError``.  Device entries outside the prediction path are called through ``_dev.call``.
"""
import ctypes as C
import os

SD_OK, SD_ERR_INVALID, SD_ERR_NOMEM, SD_ERR_HIP, SD_ERR_NODEVICE = 0, -1, -2, -3, -4
SD_U8, SD_F32, SD_BF16, SD_F16, SD_U64, SD_U32, SD_F16X2 = 0, 1, 2, 3, 4, 5, 6
SD_OUT_LOGITS_F32, SD_OUT_PROBS_F32, SD_OUT_PROBS_U8 = 0, 1, 2
SD_OP_CONV, SD_OP_POOL, SD_OP_UPCONV, SD_OP_GROUPNORM, SD_OP_FINAL = 1, 2, 3, 4, 5
SD_MOP_OPENING, SD_MOP_CLOSING, SD_MOP_DILATION, SD_MOP_EROSION = 1, 2, 3, 4
SD_CS_FIRST, SD_CS_LAST = 1, 2
SD_CST_COLS = 24
SD_SYNSSV_MAP_ITEM = 1024
SD_SPINEHEAD_VOX_GRID, SD_SPINEHEAD_VERT_GRID, SD_SPINEHEAD_ID_GRID = 8192, 1024, 1024
SD_SYN_PROPS_MAX_K, SD_SYN_PROPS_CELL_GRID, SD_SYN_PROPS_POINT_GRID, SD_SYN_PROPS_QUERY_GRID, SD_SYN_PROPS_FOREST_GRID = 64, 4096, 1024, 8192, 1024
SD_SKEL_MAX_CLASSES, SD_SKEL_LDS_NODES, SD_SKEL_VOTE_GRID, SD_SKEL_NODE_GRID, SD_SKEL_EDGE_GRID, SD_SKEL_REDO_GRID, SD_SKEL_REDO_BYTES = 64, 512, 2048, 1024, 1024, 1024, 1 << 28
SD_CELLASM_GRID = 1024
SD_MESH_GRID = 256
SD_GLIA_GRID = 1024
SD_VIEWS_GRID, SD_VIEWS_RASTER_GRID, SD_VIEWS_MAX_VIEWS, SD_VIEWS_TILE_PX = 1024, 4096, 16, 32768
SD_LOCATIONS_GRID, SD_LOCATIONS_WAVE_GRID, SD_LOCATIONS_MAX_CELLS = 1024, 4096, 1 << 21
SD_VIEWNET_GRID, SD_VIEWNET_HEAD_GRID, SD_VIEWNET_HEAD_TILE_GRID = 2048, 32, 1024
SD_GLIA_VIEWS_GRID, SD_GLIA_VIEWS_LDS_BYTES = 1024, 163840
SD_SKELETONIZE_TILE, SD_SKELETONIZE_MAX_EXTENT, SD_SKELETONIZE_MAX_ANISOTROPY, SD_SKELETONIZE_MAX_EXPONENT, SD_SKELETONIZE_MAX_SWEEPS = 16, 2048, 32768, 64, 1536
SD_SKELETONIZE_VOX_GRID, SD_SKELETONIZE_TILE_GRID, SD_SKELETONIZE_COMP_GRID, SD_SKELETONIZE_NODE_GRID = 8192, 2048, 1024, 2048

LIB_NAME = 'libsyconn_dense_hip.so'
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.environ.get('SD_LIB_NAME', LIB_NAME))

# every symbol include/syconn_dense.h declares (checked by tests/test_abi.py)
EXPORTS = ['sd_init', 'sd_device_count', 'sd_model_create', 'sd_model_destroy', 'sd_workspace_bytes', 'sd_model_overflow', 'sd_forward', 'sd_forward_batch', 'sd_forward_labels_batch',
           'sd_tile_gather', 'sd_tile_scatter', 'sd_postproc_labels', 'sd_profile_enable', 'sd_profile_read',
           'sd_debug_read_buffer', 'sd_model_num_ops', 'sd_debug_last_launch_count', 'sd_debug_op_kernel', 'sd_last_error', 'sd_version', 'sd_snappy_max_compressed_length',
           'sd_snappy_compress', 'sd_snappy_uncompressed_length', 'sd_snappy_uncompress', 'sd_downsample2', 'sd_box_majority',
           'sd_objtable_bytes', 'sd_pairtable_bytes', 'sd_segstats_scan', 'sd_segstats_compact_objects',
           'sd_segstats_compact_pairs', 'sd_objseg_workspace_bytes', 'sd_object_segmentation', 'sd_objseg_watershed_workspace_bytes',
           'sd_object_segmentation_watershed', 'sd_marker_flood', 'sd_host_box_copy', 'sd_host_zero', 'sd_plan_clip_window',
           'sd_gauss_workspace_bytes', 'sd_gaussian_threshold', 'sd_model_set_roi', 'sd_labels_make_unique', 'sd_labels_box_lut',
           'sd_chunkprops_append', 'sd_chunkpairs_append', 'sd_propmerge_temp_bytes', 'sd_propmerge_objects', 'sd_propmerge_pairs', 'sd_profile_read_clocks', 'sd_probe_mfma_rate', 'sd_memcpy2d_async',
           'sd_seg_boundaries', 'sd_contact_partners_workspace_bytes', 'sd_contact_partners', 'sd_cs_close_dilate',
           'sd_binary_morphology', 'sd_cs_syntype_table_bytes', 'sd_cs_syntype_scan', 'sd_cs_syntype_compact', 'sd_cs_syntype_records',
           'sd_cs_syntype_voxels', 'sd_syntype_masks', 'sd_cs_merge_append', 'sd_cs_merge_temp_bytes', 'sd_cs_merge_objects',
           'sd_cs_merge_synapses', 'sd_syn_ssv_temp_bytes', 'sd_syn_ssv_components', 'sd_syn_ssv_stats',
           'sd_synssv_map_pairs_temp_bytes', 'sd_synssv_map_pairs', 'sd_synssv_map_query_temp_bytes', 'sd_synssv_map_query',
           'sd_syn_props_knn_temp_bytes', 'sd_syn_props_knn', 'sd_syn_props_forest', 'sd_spinehead_workspace_bytes', 'sd_edt_squared',
           'sd_spinehead_window_mask', 'sd_spinehead_fill_holes', 'sd_spinehead_peaks', 'sd_spinehead_box_vertices_temp_bytes',
           'sd_spinehead_box_vertices', 'sd_spinehead_queries', 'sd_spinehead_markers', 'sd_spinehead_select', 'sd_skel_csr_temp_bytes', 'sd_skel_csr',
           'sd_skel_vote_temp_bytes', 'sd_skel_vote', 'sd_skel_components_temp_bytes', 'sd_skel_components',
           'sd_svgraph_components_temp_bytes', 'sd_svgraph_components', 'sd_cell_props', 'sd_cell_mapping_temp_bytes', 'sd_cell_mapping',
           'sd_cell_synapses_temp_bytes', 'sd_cell_synapses', 'sd_mesh_count', 'sd_mesh_build_temp_bytes', 'sd_mesh_build',
           'sd_mesh_merge_temp_bytes', 'sd_mesh_merge', 'sd_glia_split_temp_bytes', 'sd_glia_split', 'sd_glia_pred',
           'sd_views_rotations_temp_bytes', 'sd_views_rotations', 'sd_views_flag_empty', 'sd_views_index_bytes', 'sd_views_index_temp_bytes', 'sd_views_index',
           'sd_views_candidates_temp_bytes', 'sd_views_candidates', 'sd_views_render_temp_bytes', 'sd_views_render', 'sd_views_render_index',
           'sd_views_vote_temp_bytes', 'sd_views_vote', 'sd_locations_voxel_temp_bytes', 'sd_locations_voxel', 'sd_locations_surface_temp_bytes',
           'sd_locations_surface', 'sd_viewnet_create', 'sd_viewnet_destroy', 'sd_viewnet_workspace_bytes', 'sd_viewnet_forward', 'sd_viewnet_forward_timed',
           'sd_viewnet_overflow', 'sd_viewnet_read_buffer', 'sd_viewnet_num_ops', 'sd_viewnet_embed', 'sd_viewnet_embed_timed',
           'sd_viewnet_embed_tile_samples', 'sd_fcn_create', 'sd_fcn_destroy', 'sd_fcn_workspace_bytes',
           'sd_fcn_forward', 'sd_fcn_forward_timed', 'sd_fcn_overflow', 'sd_fcn_read_buffer', 'sd_fcn_num_ops',
           'sd_glia_view_probas', 'sd_views_center_component', 'sd_skeletonize_temp_bytes', 'sd_skeletonize_components', 'sd_skeletonize_d2',
           'sd_skeletonize_field_start', 'sd_skeletonize_relax', 'sd_skeletonize_argmax', 'sd_skeletonize_penalty', 'sd_skeletonize_round',
           'sd_skeletonize_emit_temp_bytes', 'sd_skeletonize_emit']


class OpDesc(C.Structure):
    """Mirror of ``sd_op_desc``."""
    _fields_ = [('kind', C.c_int32), ('src0', C.c_int32), ('src1', C.c_int32), ('dst', C.c_int32),
                ('cin0', C.c_int32), ('cin1', C.c_int32), ('cout', C.c_int32),
                ('kz', C.c_int32), ('ky', C.c_int32), ('kx', C.c_int32),
                ('relu', C.c_int32), ('norm', C.c_int32), ('groups', C.c_int32), ('eps', C.c_float),
                ('w_off', C.c_int64), ('b_off', C.c_int64), ('gamma_off', C.c_int64), ('beta_off', C.c_int64),
                ('mean_off', C.c_int64), ('var_off', C.c_int64)]


class ViewNetLayerDesc(C.Structure):
    """Mirror of ``sd_viewnet_layer_desc``."""
    _fields_ = [('cout', C.c_int32), ('k', C.c_int32), ('pool', C.c_int32)]


_lib = None


def load():
    """Load the library once; raise if it has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not found: build it with `make -C syconn_amd/csrc` '
                          f'(or __graft_entry__.build()); syconn_amd has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.sd_init.argtypes = [i32]; lib.sd_init.restype = i32
    lib.sd_device_count.argtypes = []; lib.sd_device_count.restype = i32
    lib.sd_model_create.argtypes = [C.POINTER(OpDesc), i32, C.POINTER(C.c_float), sz, i32, C.POINTER(vp)]
    lib.sd_model_create.restype = i32
    lib.sd_model_destroy.argtypes = [vp]; lib.sd_model_destroy.restype = None
    lib.sd_workspace_bytes.argtypes = [vp, i32, i32, i32]; lib.sd_workspace_bytes.restype = sz
    lib.sd_model_overflow.argtypes = [vp, vp, C.POINTER(C.c_int)]; lib.sd_model_overflow.restype = i32
    lib.sd_forward.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, sz, vp]; lib.sd_forward.restype = i32
    lib.sd_forward_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, sz, vp]
    lib.sd_forward_batch.restype = i32
    lib.sd_forward_labels_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_double), i32,
                                            vp, vp, sz, vp]
    lib.sd_forward_labels_batch.restype = i32
    lib.sd_tile_gather.argtypes = [vp, i32] + [i32] * 6 + [vp] + [i32] * 3 + [vp]; lib.sd_tile_gather.restype = i32
    lib.sd_tile_scatter.argtypes = [vp, i32] + [i32] * 10 + [vp] + [i32] * 6 + [vp]; lib.sd_tile_scatter.restype = i32
    lib.sd_postproc_labels.argtypes = [vp, i32, sz, C.POINTER(C.c_int32), C.POINTER(C.c_double), i32, vp, i32, vp]
    lib.sd_postproc_labels.restype = i32
    lib.sd_profile_enable.argtypes = [vp, i32]; lib.sd_profile_enable.restype = i32
    lib.sd_profile_read.argtypes = [vp, i32, C.POINTER(C.c_float), i32]; lib.sd_profile_read.restype = i32
    lib.sd_profile_read_clocks.argtypes = [vp, i32, C.POINTER(C.c_uint64), i32]; lib.sd_profile_read_clocks.restype = i32
    lib.sd_probe_mfma_rate.argtypes = [i32, i32, i32, C.c_double, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.sd_probe_mfma_rate.restype = i32
    lib.sd_memcpy2d_async.argtypes = [vp, sz, vp, sz, sz, sz, i32, vp]; lib.sd_memcpy2d_async.restype = i32
    lib.sd_debug_read_buffer.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_int32), vp]
    lib.sd_debug_read_buffer.restype = i32
    lib.sd_model_num_ops.argtypes = [vp]; lib.sd_model_num_ops.restype = i32
    lib.sd_debug_last_launch_count.argtypes = [vp]; lib.sd_debug_last_launch_count.restype = i32
    lib.sd_debug_op_kernel.argtypes = [vp, i32, C.c_char_p, i32]; lib.sd_debug_op_kernel.restype = i32
    lib.sd_last_error.argtypes = []; lib.sd_last_error.restype = C.c_char_p
    lib.sd_version.argtypes = []; lib.sd_version.restype = C.c_char_p
    lib.sd_snappy_max_compressed_length.argtypes = [sz]; lib.sd_snappy_max_compressed_length.restype = sz
    lib.sd_snappy_compress.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]; lib.sd_snappy_compress.restype = i32
    lib.sd_snappy_uncompressed_length.argtypes = [vp, sz, C.POINTER(sz)]; lib.sd_snappy_uncompressed_length.restype = i32
    lib.sd_snappy_uncompress.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]; lib.sd_snappy_uncompress.restype = i32
    lib.sd_downsample2.argtypes = [vp, i32, i32, i32, i32, vp, vp]; lib.sd_downsample2.restype = i32
    lib.sd_box_majority.argtypes = [vp, i32, i32, i32, vp, sz, i32, i32, i32, C.c_double, C.c_double, vp, vp]
    lib.sd_box_majority.restype = i32
    lib.sd_objtable_bytes.argtypes = [sz]; lib.sd_objtable_bytes.restype = sz
    lib.sd_pairtable_bytes.argtypes = [sz]; lib.sd_pairtable_bytes.restype = sz
    lib.sd_segstats_scan.argtypes = [vp, C.POINTER(vp), i32, i32, i32, i32, i32, vp, C.POINTER(vp), sz, C.POINTER(vp), sz,
                                     i32, vp, vp]
    lib.sd_segstats_scan.restype = i32
    lib.sd_segstats_compact_objects.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp]
    lib.sd_segstats_compact_objects.restype = i32
    lib.sd_segstats_compact_pairs.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp]
    lib.sd_segstats_compact_pairs.restype = i32
    lib.sd_objseg_workspace_bytes.argtypes = [i32, i32, i32, i32]; lib.sd_objseg_workspace_bytes.restype = sz
    lib.sd_object_segmentation.argtypes = [vp, i32, i32, i32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32,
                                           vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.sd_object_segmentation.restype = i32
    lib.sd_objseg_watershed_workspace_bytes.argtypes = [i32, i32, i32, i32]; lib.sd_objseg_watershed_workspace_bytes.restype = sz
    lib.sd_object_segmentation_watershed.argtypes = [vp, i32, i32, i32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32,
                                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32, vp, i32, i32, i32, i32,
                                                     C.POINTER(C.c_int32), vp, vp, vp, vp, vp, vp, sz, vp]
    lib.sd_object_segmentation_watershed.restype = i32
    lib.sd_marker_flood.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]; lib.sd_marker_flood.restype = i32
    lib.sd_model_set_roi.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]; lib.sd_model_set_roi.restype = i32
    lib.sd_gauss_workspace_bytes.argtypes = [i32, i32, i32]; lib.sd_gauss_workspace_bytes.restype = sz
    lib.sd_gaussian_threshold.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), C.c_double, vp, vp, vp, sz, vp]
    lib.sd_gaussian_threshold.restype = i32
    lib.sd_labels_make_unique.argtypes = [vp, sz, C.c_uint64, vp, vp]; lib.sd_labels_make_unique.restype = i32
    lib.sd_labels_box_lut.argtypes = [vp] + [i32] * 9 + [vp, sz, vp, vp, vp]; lib.sd_labels_box_lut.restype = i32
    lib.sd_chunkprops_append.argtypes = [vp, sz] + [i32] * 6 + [C.c_uint64, vp, vp, vp, vp, sz, vp, vp]
    lib.sd_chunkprops_append.restype = i32
    lib.sd_chunkpairs_append.argtypes = [vp, sz, vp, vp, sz] + [i32] * 3 + [C.c_uint64, vp, vp, vp, sz, vp, vp]
    lib.sd_chunkpairs_append.restype = i32
    lib.sd_propmerge_temp_bytes.argtypes = [sz]; lib.sd_propmerge_temp_bytes.restype = sz
    lib.sd_propmerge_objects.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, vp]; lib.sd_propmerge_objects.restype = i32
    lib.sd_propmerge_pairs.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]; lib.sd_propmerge_pairs.restype = i32
    i64 = C.c_int64
    lib.sd_host_box_copy.argtypes = [vp, i64, i64, vp, i64, i64, i64, i64, i64, i32]; lib.sd_host_box_copy.restype = i32
    lib.sd_host_zero.argtypes = [vp, i64, i32]; lib.sd_host_zero.restype = i32
    lib.sd_plan_clip_window.argtypes = [C.POINTER(OpDesc), i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.sd_plan_clip_window.restype = i32
    lib.sd_seg_boundaries.argtypes = [vp, i32, i32, i32, vp, vp]; lib.sd_seg_boundaries.restype = i32
    lib.sd_contact_partners_workspace_bytes.argtypes = []; lib.sd_contact_partners_workspace_bytes.restype = sz
    lib.sd_contact_partners.argtypes = [vp, vp] + [i32] * 6 + [vp, vp, sz, vp]; lib.sd_contact_partners.restype = i32
    lib.sd_cs_close_dilate.argtypes = [vp, i32, i32, i32, vp, i64, i64, i32, i32, i32, vp, vp, sz, vp]
    lib.sd_cs_close_dilate.restype = i32
    # block_processing_C.pyx:78-158 (extract_cs_syntype) and cs_extraction_steps.py:402-433 (sj morphology, syn-type masks)
    lib.sd_binary_morphology.argtypes = [vp, i32, i32, i32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i32, vp, i32, i32,
                                         i32, vp, vp, sz, vp]
    lib.sd_binary_morphology.restype = i32
    lib.sd_cs_syntype_table_bytes.argtypes = [sz]; lib.sd_cs_syntype_table_bytes.restype = sz
    lib.sd_cs_syntype_scan.argtypes = [vp, i32, vp, vp, vp] + [i32] * 9 + [vp, sz, vp, vp, vp, vp]
    lib.sd_cs_syntype_scan.restype = i32
    lib.sd_cs_syntype_compact.argtypes = [vp, sz, vp, vp, sz, vp, vp]; lib.sd_cs_syntype_compact.restype = i32
    lib.sd_cs_syntype_records.argtypes = [vp, sz, vp, i64, i32, i32, i32, vp, vp, vp]; lib.sd_cs_syntype_records.restype = i32
    lib.sd_cs_syntype_voxels.argtypes = [vp, i32, vp] + [i32] * 6 + [vp, i64, i64, C.POINTER(i64), vp, vp, vp]
    lib.sd_cs_syntype_voxels.restype = i32
    lib.sd_syntype_masks.argtypes = [vp, i32, sz, C.c_uint64, C.c_uint64, vp, vp, vp]; lib.sd_syntype_masks.restype = i32
    # cs_extraction_steps.py:484-492, :544-623, :631-673 (the dataset merge of contact sites and synapses)
    lib.sd_cs_merge_append.argtypes = [vp, sz, vp, sz, i32, i32, i32, vp, vp, vp, vp, sz] + [vp] * 7 + [sz, vp, sz, vp, vp]
    lib.sd_cs_merge_append.restype = i32
    lib.sd_cs_merge_temp_bytes.argtypes = [sz]; lib.sd_cs_merge_temp_bytes.restype = sz
    lib.sd_cs_merge_objects.argtypes = [vp, vp, vp, vp, sz, C.c_uint64] + [vp] * 8 + [sz, vp]; lib.sd_cs_merge_objects.restype = i32
    lib.sd_cs_merge_synapses.argtypes = [vp] * 7 + [sz, vp, sz, vp, vp, sz, C.c_uint64] + [vp] * 13 + [sz, vp]
    lib.sd_cs_merge_synapses.restype = i32
    # cs_processing_steps.py:552-602 (connected_cluster_kdtree) and :453-474 (per-component attributes of syn_ssv)
    lib.sd_syn_ssv_temp_bytes.argtypes = [sz]; lib.sd_syn_ssv_temp_bytes.restype = sz
    lib.sd_syn_ssv_components.argtypes = [vp, vp, vp, vp, sz, sz, sz, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), i32, vp, vp, vp, sz, vp]
    lib.sd_syn_ssv_components.restype = i32
    lib.sd_syn_ssv_stats.argtypes = [vp, vp, vp, sz, sz, C.POINTER(C.c_double), C.c_uint64] + [vp] * 8 + [vp, sz, vp]
    lib.sd_syn_ssv_stats.restype = i32
    # cs_processing_steps.py:888-1009 (candidate organelles of every synapse side) and :1012-1052 (vertices against synapse voxels)
    lib.sd_synssv_map_pairs_temp_bytes.argtypes = [sz]; lib.sd_synssv_map_pairs_temp_bytes.restype = sz
    lib.sd_synssv_map_pairs.argtypes = [vp, vp, sz, vp, vp, vp, sz, C.POINTER(C.c_double), C.c_double, vp, vp, sz, vp, vp, sz, vp]
    lib.sd_synssv_map_pairs.restype = i32
    lib.sd_synssv_map_query_temp_bytes.argtypes = [sz, sz, sz]; lib.sd_synssv_map_query_temp_bytes.restype = sz
    lib.sd_synssv_map_query.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, sz, sz, vp, vp, sz, sz, i32, C.POINTER(C.c_double), C.c_double, i32,
                                        sz, vp, vp, vp, vp, vp, sz, vp]
    lib.sd_synssv_map_query.restype = i32
    # cs_processing_steps.py:161-164 (the two cKDTrees per cell behind the partner properties) and :1155-1156 (predict_proba per synapse)
    lib.sd_syn_props_knn_temp_bytes.argtypes = [sz, sz]; lib.sd_syn_props_knn_temp_bytes.restype = sz
    lib.sd_syn_props_knn.argtypes = [vp, i32, vp, sz, sz, vp, vp, vp, sz, i32, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.sd_syn_props_knn.restype = i32
    lib.sd_syn_props_forest.argtypes = [vp, sz, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.sd_syn_props_forest.restype = i32
    # reps/super_segmentation_helper.py:2068-2198 (extract_spinehead_volume_mesh, the per-window steps)
    i64p, i32p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.sd_spinehead_workspace_bytes.argtypes = [i32, i32, i32]; lib.sd_spinehead_workspace_bytes.restype = sz
    lib.sd_edt_squared.argtypes = [vp, i32, i32, i32, vp, vp, sz, vp]; lib.sd_edt_squared.restype = i32
    lib.sd_spinehead_window_mask.argtypes = [vp, i32, i32, i32, i64p, i64p, vp, vp, vp, i32, i32, i32, vp, sz, vp, vp]
    lib.sd_spinehead_window_mask.restype = i32
    lib.sd_spinehead_fill_holes.argtypes = [vp, i32, i32, i32, vp, vp, vp, sz, vp]; lib.sd_spinehead_fill_holes.restype = i32
    lib.sd_spinehead_peaks.argtypes = [vp, vp, i32, i32, i32, vp, sz, vp, vp, sz, vp]; lib.sd_spinehead_peaks.restype = i32
    lib.sd_spinehead_box_vertices_temp_bytes.argtypes = [sz, sz]; lib.sd_spinehead_box_vertices_temp_bytes.restype = sz
    lib.sd_spinehead_box_vertices.argtypes = [vp, i32, vp, sz, vp, sz, i32p, i32, vp, vp, vp, sz, vp, sz, vp]
    lib.sd_spinehead_box_vertices.restype = i32
    lib.sd_spinehead_queries.argtypes = [vp, vp, sz, sz, sz, f64p, vp, vp, vp]; lib.sd_spinehead_queries.restype = i32
    lib.sd_spinehead_markers.argtypes = [vp, vp, vp, sz, i32, i32, i32, vp, vp]; lib.sd_spinehead_markers.restype = i32
    lib.sd_spinehead_select.argtypes = [vp, i32, i32, i32, i64p, i64p, f64p, vp, vp, vp, sz, vp]; lib.sd_spinehead_select.restype = i32
    # reps/super_segmentation_helper.py:1270-1302 (majorityvote_skeleton_property) and :1233-1266 (majority_vote_compartments)
    lib.sd_skel_csr_temp_bytes.argtypes = [sz]; lib.sd_skel_csr_temp_bytes.restype = sz
    lib.sd_skel_csr.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, sz, vp]; lib.sd_skel_csr.restype = i32
    lib.sd_skel_vote_temp_bytes.argtypes = [sz, sz]; lib.sd_skel_vote_temp_bytes.restype = sz
    lib.sd_skel_vote.argtypes = [vp, vp, vp, sz, vp, sz, sz, sz, vp, i32, C.c_double, vp, vp, vp, vp, sz, vp]; lib.sd_skel_vote.restype = i32
    lib.sd_skel_components_temp_bytes.argtypes = [sz]; lib.sd_skel_components_temp_bytes.restype = sz
    lib.sd_skel_components.argtypes = [vp, vp, vp, sz, sz, sz, vp, i32, i32, i32, vp, vp, vp, sz, vp]; lib.sd_skel_components.restype = i32
    # exec/exec_init.py:299-367, :61-80 with proc/graphs.py:220-249 (cells from the supervoxel graph), reps/super_segmentation_object.py:713-727,
    # :1148-1168 (cell properties), proc/sd_proc.py:1063-1084 with proc/ssd_proc.py:55-91, :126-238 (organelles to cells), :315-342 (synapses)
    f64 = C.c_double
    lib.sd_svgraph_components_temp_bytes.argtypes = [sz, sz]; lib.sd_svgraph_components_temp_bytes.restype = sz
    lib.sd_svgraph_components.argtypes = [vp, sz, vp, vp, vp, vp, sz, sz, f64p, f64, i32] + [vp] * 8 + [vp, sz, vp]; lib.sd_svgraph_components.restype = i32
    lib.sd_cell_props.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]; lib.sd_cell_props.restype = i32
    lib.sd_cell_mapping_temp_bytes.argtypes = [sz, sz]; lib.sd_cell_mapping_temp_bytes.restype = sz
    lib.sd_cell_mapping.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, sz, f64, f64, f64] + [vp] * 9 + [vp, sz, vp]; lib.sd_cell_mapping.restype = i32
    lib.sd_cell_synapses_temp_bytes.argtypes = [sz]; lib.sd_cell_synapses_temp_bytes.restype = sz
    lib.sd_cell_synapses.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp]; lib.sd_cell_synapses.restype = i32
    # proc/meshes.py:937-994 (find_meshes, all labels of a chunk in one pass) and proc/sd_proc.py:951-975 (merge, mesh_bb, mesh_area)
    lib.sd_mesh_count.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, sz, vp, vp]; lib.sd_mesh_count.restype = i32
    lib.sd_mesh_build_temp_bytes.argtypes = [i32, i32, i32, sz, sz]; lib.sd_mesh_build_temp_bytes.restype = sz
    lib.sd_mesh_build.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, sz, f64p, f64p, sz, sz] + [vp] * 7 + [vp, sz, vp]
    lib.sd_mesh_build.restype = i32
    lib.sd_mesh_merge_temp_bytes.argtypes = [sz]; lib.sd_mesh_merge_temp_bytes.restype = sz
    lib.sd_mesh_merge.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz] + [vp] * 8 + [vp, sz, vp]; lib.sd_mesh_merge.restype = i32
    # proc/graphs.py:173-360 (remove_glia_nodes for all cells), proc/glia_splitting.py:37-161, reps/segmentation_helper.py:32-78 (glia_pred_so)
    lib.sd_glia_split_temp_bytes.argtypes = [sz, sz, sz]; lib.sd_glia_split_temp_bytes.restype = sz
    lib.sd_glia_split.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, f64, vp, f64, vp, sz, sz] + [vp] * 18 + [vp, vp, sz, vp]; lib.sd_glia_split.restype = i32
    lib.sd_glia_pred.argtypes = [vp, i32, vp, sz, sz, f64, i32, vp, vp, vp, vp]; lib.sd_glia_pred.restype = i32
    # proc/rendering_egl.py:130-174, :460-681 (the views), proc/meshes.py:69-175, :236-360 (normalisation, rotations),
    # reps/super_segmentation_helper.py:1527-1551, :1603-1615 (the pixel -> vertex vote)
    f32, f32p = C.c_float, C.POINTER(C.c_float)
    lib.sd_views_rotations_temp_bytes.argtypes = [sz, sz]; lib.sd_views_rotations_temp_bytes.restype = sz
    lib.sd_views_rotations.argtypes = [vp, sz, sz, vp, sz, f32p, f32, f32, vp, vp, vp, vp, sz, vp]; lib.sd_views_rotations.restype = i32
    lib.sd_views_flag_empty.argtypes = [vp, sz, sz, vp, sz, f32p, f32, f32, vp, vp, vp, sz, vp]; lib.sd_views_flag_empty.restype = i32
    lib.sd_views_index_bytes.argtypes = [sz]; lib.sd_views_index_bytes.restype = sz
    lib.sd_views_index_temp_bytes.argtypes = [sz]; lib.sd_views_index_temp_bytes.restype = sz
    lib.sd_views_index.argtypes = [vp, sz, vp, sz, f32p, f32, vp, sz, vp, vp, sz, vp]; lib.sd_views_index.restype = i32
    lib.sd_views_candidates_temp_bytes.argtypes = [sz]; lib.sd_views_candidates_temp_bytes.restype = sz
    lib.sd_views_candidates.argtypes = [vp, sz, vp, sz, f32p, f32, f64p, vp, vp, sz, vp, vp, sz, vp]; lib.sd_views_candidates.restype = i32
    lib.sd_views_render_temp_bytes.argtypes = [sz, i32]; lib.sd_views_render_temp_bytes.restype = sz
    lib.sd_views_render.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, f32p, f32, f64p, f64p, f64p, i32, i32, i32, f64p, vp, vp, sz, vp, sz, vp, vp, sz, vp]
    lib.sd_views_render.restype = i32
    lib.sd_views_render_index.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, f32p, f32, f64p, f64p, f64p, i32, i32, i32, vp, vp, sz, vp, sz, vp, vp, sz, vp]
    lib.sd_views_render_index.restype = i32
    lib.sd_views_vote_temp_bytes.argtypes = [sz, i32]; lib.sd_views_vote_temp_bytes.restype = sz
    lib.sd_views_vote.argtypes = [vp, vp, sz, C.c_uint32, sz, i32, i32, vp, vp, vp, vp, sz, vp]; lib.sd_views_vote.restype = i32
    # reps/segmentation.py:700-732 (sample_locations), handler/multiviews.py:339-355 (generate_rendering_locs), reps/rep_helper.py:376-417
    # (surface_samples): the rendering locations of all objects of a table in one call
    lib.sd_locations_voxel_temp_bytes.argtypes = [sz, sz]; lib.sd_locations_voxel_temp_bytes.restype = sz
    lib.sd_locations_voxel.argtypes = [vp, i32, vp, sz, sz, f64, vp, vp, sz, vp, vp, sz, vp]; lib.sd_locations_voxel.restype = i32
    lib.sd_locations_surface_temp_bytes.argtypes = [sz, sz]; lib.sd_locations_surface_temp_bytes.restype = sz
    lib.sd_locations_surface.argtypes = [vp, vp, sz, sz, f32p, f64, vp, vp, sz, vp, vp, sz, vp]; lib.sd_locations_surface.restype = i32
    # handler/prediction.py:985-1000 (get_celltype_model_e3 -> InferenceModel.predict_proba) for cnn/cnn_celltype_cmn_j0251.py:22-60
    lib.sd_viewnet_create.argtypes = [C.POINTER(ViewNetLayerDesc), i32, i32p, i32, i32, i32, i32, f32p, sz, i32, C.POINTER(vp)]
    lib.sd_viewnet_create.restype = i32
    lib.sd_viewnet_destroy.argtypes = [vp]; lib.sd_viewnet_destroy.restype = None
    lib.sd_viewnet_workspace_bytes.argtypes = [vp, sz, i32, i32, i32]; lib.sd_viewnet_workspace_bytes.restype = sz
    lib.sd_viewnet_forward.argtypes = [vp, vp, sz, i32, i32, i32, vp, sz, i32, vp, vp, vp, sz, vp, vp]; lib.sd_viewnet_forward.restype = i32
    lib.sd_viewnet_forward_timed.argtypes = lib.sd_viewnet_forward.argtypes + [f32p]; lib.sd_viewnet_forward_timed.restype = i32
    # reps/super_segmentation_helper.py:1758-1817 (view_embedding_of_sso_nocache) for cnn/cnn_atn.py:21-55 (RepresentationNetwork)
    lib.sd_viewnet_embed.argtypes = lib.sd_viewnet_forward.argtypes; lib.sd_viewnet_embed.restype = i32
    lib.sd_viewnet_embed_timed.argtypes = lib.sd_viewnet_forward_timed.argtypes; lib.sd_viewnet_embed_timed.restype = i32
    lib.sd_viewnet_embed_tile_samples.argtypes = [vp]; lib.sd_viewnet_embed_tile_samples.restype = i32
    lib.sd_viewnet_overflow.argtypes = [vp, vp, vp, i32p]; lib.sd_viewnet_overflow.restype = i32
    lib.sd_viewnet_read_buffer.argtypes = [vp, i32, vp, vp, sz, i32, i32, i32, f32p, i32p, vp]; lib.sd_viewnet_read_buffer.restype = i32
    lib.sd_viewnet_num_ops.argtypes = [vp]; lib.sd_viewnet_num_ops.restype = i32
    # handler/prediction.py:1003-1030 (get_semseg_spiness_model, get_semseg_axon_model) as reps/super_segmentation_helper.py:1353-1392
    # (predict_views_semseg) calls them
    lib.sd_fcn_create.argtypes = [i32, i32p, i32p, i32, i32, f32p, sz, i32, C.POINTER(vp)]; lib.sd_fcn_create.restype = i32
    lib.sd_fcn_destroy.argtypes = [vp]; lib.sd_fcn_destroy.restype = None
    lib.sd_fcn_workspace_bytes.argtypes = [vp, sz, i32, i32]; lib.sd_fcn_workspace_bytes.restype = sz
    lib.sd_fcn_forward.argtypes = [vp, vp, sz, i32, i32, i32, sz, sz, vp, vp, vp, sz, vp, vp]; lib.sd_fcn_forward.restype = i32
    lib.sd_fcn_forward_timed.argtypes = lib.sd_fcn_forward.argtypes + [f32p]; lib.sd_fcn_forward_timed.restype = i32
    lib.sd_fcn_overflow.argtypes = [vp, vp, vp, i32p]; lib.sd_fcn_overflow.restype = i32
    lib.sd_fcn_read_buffer.argtypes = [vp, i32, vp, vp, sz, i32, i32, f32p, i32p, vp]; lib.sd_fcn_read_buffer.restype = i32
    lib.sd_fcn_num_ops.argtypes = [vp]; lib.sd_fcn_num_ops.restype = i32
    # handler/prediction.py:978-982 (get_glia_model_e3: the probabilities), proc/image.py:125-144 (single_conn_comp_img)
    lib.sd_glia_view_probas.argtypes = [vp, sz, vp, vp, vp]; lib.sd_glia_view_probas.restype = i32
    lib.sd_views_center_component.argtypes = [vp, sz, i32, i32, i32, vp, vp]; lib.sd_views_center_component.restype = i32
    # proc/skeleton.py:21-86 (kimimaro_skelgen: the TEASAR tracing of a labelled chunk, stage by stage)
    lib.sd_skeletonize_temp_bytes.argtypes = [i32, i32, i32]; lib.sd_skeletonize_temp_bytes.restype = sz
    lib.sd_skeletonize_components.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, sz, vp, vp, sz, vp]; lib.sd_skeletonize_components.restype = i32
    lib.sd_skeletonize_d2.argtypes = [vp, i32, i32, i32, i32p, sz, vp, vp, vp, vp, vp, sz, vp]; lib.sd_skeletonize_d2.restype = i32
    lib.sd_skeletonize_field_start.argtypes = [vp, i32, i32, i32, vp, sz, vp, i32, vp, sz, vp]; lib.sd_skeletonize_field_start.restype = i32
    lib.sd_skeletonize_relax.argtypes = [vp, i32, i32, i32, i32p, vp, vp, i32, vp, vp, sz, vp]; lib.sd_skeletonize_relax.restype = i32
    lib.sd_skeletonize_argmax.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]; lib.sd_skeletonize_argmax.restype = i32
    lib.sd_skeletonize_penalty.argtypes = [vp, vp, vp, sz, sz, vp, vp, f64, i32, vp, vp]; lib.sd_skeletonize_penalty.restype = i32
    lib.sd_skeletonize_round.argtypes = [vp, i32, i32, i32, i32p, vp, vp, vp, vp, vp, vp, vp, sz, f32, f32, vp, vp, vp, sz, vp]; lib.sd_skeletonize_round.restype = i32
    lib.sd_skeletonize_emit_temp_bytes.argtypes = [sz]; lib.sd_skeletonize_emit_temp_bytes.restype = sz
    lib.sd_skeletonize_emit.argtypes = [vp, i32, i32, i32, i32p, vp, vp, vp, vp, sz, sz] + [vp] * 7 + [vp, sz, vp, sz, vp]; lib.sd_skeletonize_emit.restype = i32
    _lib = lib
    return lib


class ActivationOverflowError(RuntimeError, FloatingPointError):
    """fp16 activation storage ('f16', 'f16x2') overflowed (> 65504) during a forward pass: its results are invalid.  Use
    act_dtype='bf16' / 'f32' (fp32's exponent range)."""


def check(rc: int, what: str = ''):
    """Map library error codes to the exceptions the reference's callers expect
    (RuntimeError == 'out of device memory' for the tile-halving loop)."""
    if rc == SD_OK:
        return
    msg = load().sd_last_error().decode(errors='replace')
    text = f'{what}: {msg}' if what else msg
    if rc == SD_ERR_INVALID:
        raise ValueError(text)
    raise RuntimeError(text)


def host_box_copy(dst, src, n_threads: int = 16):
    """dst[...] = src for two 3D uint8 CPU tensors / arrays of equal shape whose last axis is contiguous (views into larger
    volumes are the point), copied row by row on `n_threads` host threads by the C helper."""
    import torch
    d = dst if isinstance(dst, torch.Tensor) else torch.from_numpy(dst)
    s = src if isinstance(src, torch.Tensor) else torch.from_numpy(src)
    assert d.dtype == torch.uint8 and s.dtype == torch.uint8 and d.dim() == 3 and tuple(d.shape) == tuple(s.shape)
    assert (d.stride(2) == 1 or d.shape[2] <= 1) and (s.stride(2) == 1 or s.shape[2] <= 1)
    rc = load().sd_host_box_copy(s.data_ptr(), s.stride(0), s.stride(1), d.data_ptr(), d.stride(0), d.stride(1),
                                 d.shape[0], d.shape[1], d.shape[2], int(n_threads))
    if rc != SD_OK:
        raise ValueError('sd_host_box_copy: bad argument')


def host_zero(t, n_threads: int = 16):
    assert t.is_contiguous() and t.dtype.itemsize == 1
    load().sd_host_zero(t.data_ptr(), t.numel(), int(n_threads))


# -- snappy raw format (host side; the codec of the KNOSSOS ``*.seg.sz.zip`` overlay cubes) ---------------------------
def snappy_compress(data) -> bytes:
    """``snappy.compress(data)`` of python-snappy (raw format), computed by the C codec of the library."""
    lib = load()
    buf = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    n = len(buf)
    cap = lib.sd_snappy_max_compressed_length(n)
    out = C.create_string_buffer(cap)
    out_len = C.c_size_t(0)
    src = (C.c_char * n).from_buffer_copy(buf) if n else None
    rc = lib.sd_snappy_compress(src, n, out, cap, C.byref(out_len))
    if rc != SD_OK:
        raise ValueError('snappy_compress: invalid argument')
    return out.raw[:out_len.value]


def snappy_decompress(data) -> bytes:
    """``snappy.decompress(data)``; raises ValueError on a corrupt or truncated stream."""
    lib = load()
    buf = bytes(data)
    n = len(buf)
    src = (C.c_char * n).from_buffer_copy(buf) if n else None
    ulen = C.c_size_t(0)
    if lib.sd_snappy_uncompressed_length(src, n, C.byref(ulen)) != SD_OK:
        raise ValueError('snappy_decompress: corrupt input (length preamble)')
    out = C.create_string_buffer(max(ulen.value, 1))
    out_len = C.c_size_t(0)
    if lib.sd_snappy_uncompress(src, n, out, ulen.value, C.byref(out_len)) != SD_OK:
        raise ValueError('snappy_decompress: corrupt input')
    return out.raw[:out_len.value]
