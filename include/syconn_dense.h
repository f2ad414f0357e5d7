/*
 * syconn_dense.h -- C ABI of libsyconn_dense_hip.so: the MI355X (gfx950) compute layer under SyConn's chunked
 * dense 3D-CNN prediction path.
 *
 * The reference has NO FFI on this path: its boundary is the Python API of
 *   syconn/handler/prediction.py:594-868  (predict_dense_to_kd / dense_predictor / dense_predicton_helper)
 * which calls the third-party elektronn3.inference.Predictor (prediction.py:770-781, 863) which in turn runs a
 * TorchScript elektronn3 U-Net through torch/cuDNN.  This header is the C ABI the build adds UNDER that Python
 * API; every entry point cites the reference step it replaces.  INTEGRATION.md shows the
 * ctypes binding a SyConn maintainer would add.
 *
 * Conventions
 *   - return 0 (SD_OK) on success, negative on error; sd_last_error() gives the message (thread-local).
 *     SD_ERR_NOMEM is mapped by the Python layer to RuntimeError so that the reference's tile-halving retry
 *     loop (prediction.py:783-794) keeps working.
 *   - all device buffers are CALLER-OWNED (the host framework's allocator); the library owns only the packed
 *     weights inside an sd_model.  Pointers are plain device addresses, sizes are bytes / elements as stated.
 *   - outputs, tables, `temp_dev` and workspaces need not be initialised by the caller: whatever an entry reads of
 *     them it has written in the same call (counts_dev / status / flag words included), so their previous bytes never
 *     reach a result.  The exceptions are stated at their entries: the per-dataset cursors and record arrays that
 *     the caller zeroes once before the first chunk (sd_chunkprops_append / sd_chunkpairs_append, sd_cs_syntype_records).
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream); the caller
 *     synchronises.  A handle is bound to one device and is not thread-safe.
 *   - volumes are z,y,x (x fastest).  Network input is one channel, planar.  Network output is planar
 *     (C, D, H, W).  Activations inside the workspace are channel-blocked ([C/16][z][y][x][16]) in the model's
 *     activation dtype; that layout is private to the library.
 */
#ifndef SYCONN_DENSE_H
#define SYCONN_DENSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID (-1) /* bad argument / unsupported layer combination */
#define SD_ERR_NOMEM (-2)   /* workspace too small or device allocation failed */
#define SD_ERR_HIP (-3)     /* HIP runtime error */
#define SD_ERR_NODEVICE (-4)

/* element types of caller-visible buffers */
enum sd_dtype { SD_U8 = 0, SD_F32 = 1, SD_BF16 = 2, SD_F16 = 3, SD_U64 = 4, SD_U32 = 5,
                SD_F16X2 = 6 /* only as act_dtype of sd_model_create: split-fp16 storage, see there */ };

/* what sd_forward writes: raw logits (model(inp)), softmax(1) (Predictor(apply_softmax=True), prediction.py:779),
 * or floor(255*softmax) as uint8 (dense_predicton_helper, prediction.py:864-865) */
enum sd_out_kind { SD_OUT_LOGITS_F32 = 0, SD_OUT_PROBS_F32 = 1, SD_OUT_PROBS_U8 = 2,
                   SD_OUT_LABELS_U8 = 3 /* only through sd_forward_labels_batch */ };

/* layer kinds of the network plan (the elektronn3 U-Net block structure) */
enum sd_op_kind {
    SD_OP_CONV = 1,      /* Conv3d k=(3,3,3)|(1,3,3), 'same' zero padding, +bias, +folded eval-BatchNorm, +ReLU;
                            src1 >= 0: input is cat((crop(src0), src1), channel) (UpConv merge, autocrop) */
    SD_OP_POOL = 2,      /* MaxPool3d k=(2,2,2)|(1,2,2), ceil_mode=True */
    SD_OP_UPCONV = 3,    /* ConvTranspose3d k=s=(2,2,2)|(1,2,2), +bias, +folded eval-BatchNorm, +ReLU */
    SD_OP_GROUPNORM = 4, /* in-place GroupNorm(groups) + ReLU on buffer src0, statistics over the region cropped to
                            the shape of buffer src1 (if >= 0) */
    SD_OP_FINAL = 5      /* Conv3d k=1 to `cout` classes (+ softmax / uint8 epilogue chosen at sd_forward) */
};

/* One layer.  Buffer id 0 is the network input (1 channel); every other id names an activation buffer inside the
 * workspace.  All *_off fields are FLOAT offsets into the weight blob given to sd_model_create, -1 if absent.
 * Weights are in PyTorch layout: Conv3d [cout][cin][kz][ky][kx], ConvTranspose3d [cin][cout][kz][ky][kx]. */
typedef struct sd_op_desc {
    int32_t kind;
    int32_t src0, src1, dst;
    int32_t cin0, cin1, cout;
    int32_t kz, ky, kx;
    int32_t relu;
    int32_t norm;   /* 0: none, 1: eval-mode BatchNorm folded into the layer (gamma/beta/mean/var offsets) */
    int32_t groups; /* SD_OP_GROUPNORM */
    float eps;
    int64_t w_off, b_off, gamma_off, beta_off, mean_off, var_off;
} sd_op_desc;

typedef struct sd_model sd_model;

/* Bind the calling thread to a device (replaces Predictor's device pick, row P1).  Returns SD_ERR_NODEVICE when no
 * gfx950 device is visible -- there is no CPU fallback in this library. */
int sd_init(int device_ordinal);

/* Number of visible HIP devices (0 if none). */
int sd_device_count(void);

/* Build a model: validate the plan, fold BatchNorm, convert + pack weights into MFMA fragment order and upload
 * them.  Replaces torch.jit.load(model.pts).to(device) (prediction.py:777, 1061-1062).
 * act_dtype: SD_BF16 or SD_F16 (storage type of activations / MFMA operands; accumulation is fp32); SD_F16X2 = the
 * REFERENCE-PRECISION plan ON THE MATRIX CORES: every activation and weight is kept as two fp16 numbers hi + lo (22 mantissa
 * bits; weights times a power of two per layer so that their lo parts stay normal) and every product is three fp16 MFMAs
 * Wlo.Xhi + Whi.Xhi + Whi.Xlo accumulated in fp32 -- fp32-level logits (what the reference computes, prediction.py:777-779)
 * at ~3x the cost of the SD_F16 plan; range-guarded like SD_F16 (sd_model_overflow); or SD_F32 = the
 * REFERENCE-PRECISION mode: fp32 storage and fp32 FMA arithmetic like the reference's own torch path (Predictor is built
 * without float16, prediction.py:777-779); planar activations, one plain launch per layer, ~25x slower than the bf16
 * plan -- for label-exactness checks against an fp32 implementation, not for throughput. */
int sd_model_create(const sd_op_desc* ops, int n_ops, const float* weights, size_t n_floats, int act_dtype,
                    sd_model** out);
void sd_model_destroy(sd_model* m);

/* Output box of interest for the following forward passes of this model (lo inclusive, hi exclusive, z,y,x in tile coordinates;
 * two NULLs: the whole tile again).  tiled_apply (elektronn3, row P3) keeps only the core of every tile and throws the overlap
 * rim away (prediction.py:777-779 overlap_shape; dense_predictor also crops the chunk's halo, :812): with a box set, the decoder
 * layers (up-convolutions, the convolutions behind them, the fused final layer) compute only the sub-boxes that box depends on
 * -- every value INSIDE the box is the one a whole-tile pass computes, bit for bit; what the output holds outside it is
 * unspecified.  The fused level-0 decoder kernel is replaced by its layers, so call this BEFORE sd_workspace_bytes.  Networks
 * with GroupNorm (statistics over whole tensors) and SD_F32 ignore the box. */
int sd_model_set_roi(sd_model* m, const int32_t* lo_zyx, const int32_t* hi_zyx);

/* Workspace bytes sd_forward needs for a (D,H,W) input tile (a multiple of 256); 0 on error.  sd_forward_batch needs
 * N times this value. */
size_t sd_workspace_bytes(const sd_model* m, int D, int H, int W);

/* One forward pass of the network on one tile = Predictor._predict (row P4: model(inp) [+ softmax(1)]).
 * in_dev: (D,H,W) planar, in_dtype SD_U8 (normalised as float32(v)/255, prediction.py:808) or SD_F32.
 * out_dev: (cout_final, D, H, W) planar, float32 or uint8 according to out_kind.
 * Size limits (SD_ERR_INVALID beyond them): a tile has fewer than 2^31 voxels and every activation tensor fewer than 2^32
 * 8-channel groups (the streaming passes decode element indices with 32-bit arithmetic); the reference's tiles are
 * 178 x 243 x 331 = 1.4e7 voxels. */
int sd_forward(sd_model* m, const void* in_dev, int in_dtype, int D, int H, int W, void* out_dev, int out_kind,
               void* workspace_dev, size_t ws_bytes, void* stream);

/* The same for N independent tiles of one shape in ONE set of launches = Predictor.predict's batch split
 * (`batch_size`, row P2): in_dev (N,D,H,W), out_dev (N,cout_final,D,H,W), both dense; workspace N *
 * sd_workspace_bytes(D,H,W).  Every kernel simply sees N times as many blocks, which fills the 256 CUs in the deep,
 * small layers of the network and amortises launch gaps; results are identical to N sd_forward calls. */
int sd_forward_batch(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W, void* out_dev,
                     int out_kind, void* workspace_dev, size_t ws_bytes, void* stream);

/* fp16 range guard.  With act_dtype SD_F16 an activation above 65504 is stored as inf and reaches the final layer as inf / NaN
 * logits; the final-layer kernels raise a device flag when that happens (the reference computes in fp32 and cannot overflow
 * there, prediction.py:777-779).  Copies the flag to *flag_out (1 = some forward pass since the last call overflowed: its
 * results are invalid; rerun with SD_BF16 or SD_F32) and clears it.  SYNCHRONISES `stream` (the stream the forwards were
 * enqueued on).  Always 0 for SD_BF16 / SD_F32 models, whose storage types share fp32's exponent range. */
int sd_model_overflow(sd_model* m, void* stream, int* flag_out);

/* Forward pass with the label rule of dense_predictor (prediction.py:813-833, row A7) applied in the final layer's
 * epilogue: out_dev (N, D, H, W) uint8 = what sd_postproc_labels computes from the SD_OUT_PROBS_U8 result of
 * sd_forward_batch -- label = 0; for i in order: if floor(255*p[ids[i]]) > thresholds[i] then label = ids[i] -- without
 * writing and re-reading the probability maps.  ids in [0, cout_final), n_ids <= 16, thresholds in uint8 units. */
int sd_forward_labels_batch(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W,
                            const int32_t* ids, const double* thresholds, int n_ids, uint8_t* out_dev,
                            void* workspace_dev, size_t ws_bytes, void* stream);

/* tiled_apply helpers (row P3).  Gather: copy the (TD,TH,TW) box starting at (oz,oy,ox) -- which may lie partly
 * outside the (VD,VH,VW) volume -- into a dense tile, zeros outside (zero-padded tile extraction).
 * dtype: SD_U8 or SD_F32 (copied verbatim). */
int sd_tile_gather(const void* vol_dev, int dtype, int VD, int VH, int VW, int oz, int oy, int ox, void* tile_dev,
                   int TD, int TH, int TW, void* stream);
/* Scatter: for each of C channels copy tile[c, cz:cz+KD, cy:cy+KH, cx:cx+KW] (tile is (C,TD,TH,TW)) into
 * vol[c, oz:oz+KD, oy:oy+KH, ox:ox+KW] (vol is (C,VD,VH,VW)); the crop-only stitching of tiled_apply and the
 * halo crop of prediction.py:812.  dtype: SD_U8 or SD_F32. */
int sd_tile_scatter(const void* tile_dev, int dtype, int C, int TD, int TH, int TW, int cz, int cy, int cx, int KD,
                    int KH, int KW, void* vol_dev, int VD, int VH, int VW, int oz, int oy, int ox, void* stream);

/* The label rule of prediction.py:813-833 for ONE multi-id target: out[v] = 0; for i in order:
 * if (probs[ids[i]][v] > thresholds[i]) out[v] = ids[i].  probs: (C, nvox) uint8; `ids` / `thresholds` are HOST
 * arrays (n_ids <= 16), thresholds already resolved by the caller (None -> 127.5, t<1 -> 255*t) and compared
 * exactly as numpy compares uint8 with a float64; out_dtype SD_U8 or SD_U64 (save_seg takes uint64). */
int sd_postproc_labels(const uint8_t* probs_dev, int C, size_t nvox, const int32_t* ids, const double* thresholds,
                       int n_ids, void* out_dev, int out_dtype, void* stream);

/* `height` pieces of `width_bytes` contiguous bytes each, `*_pitch` bytes apart (hipMemcpy2DAsync on `stream`): how a (z-range,
 * y-range, all x) strip of a (z,y,x) volume travels between a page-locked host volume and its device copy without touching the
 * rows around it (syconn_amd.parallel: per-strip result downloads).  kind: 0 host -> device, 1 device -> host, 2 device -> device. */
int sd_memcpy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t height, int kind,
                      void* stream);

/* Measurement / test support.  With n_slots > 0 every layer launch of an sd_forward is bracketed by HIP events
 * recorded on the launch stream; forward number k uses event set k % n_slots (counted from this call), so a timed
 * region of many forwards can be read back afterwards without synchronising inside it.  n_slots = 0 switches off.
 * sd_profile_read returns the per-layer milliseconds of one slot (the caller synchronised the stream before). */
int sd_profile_enable(sd_model* m, int n_slots);
int sd_profile_read(sd_model* m, int slot, float* ms_per_op, int n_ops);
/* With profiling enabled every convolution launch also stamps, from its first workgroup, the shader cycle counter and the constant
 * 100 MHz counter on entry and on exit: stamps[4 * op + {0,1,2,3}] = {cycles at entry, ticks at entry, cycles at exit, ticks at exit}
 * (zeros for ops without a convolution launch of their own) -- shader clock of the launch = (c1 - c0) / ((t1 - t0) * 10 ns).
 * The caller synchronised the stream before. */
int sd_profile_read_clocks(sd_model* m, int slot, uint64_t* stamps, int n_ops);
/* Box calibration: a chip-wide dense bf16 MFMA loop (n_workgroups x waves_per_workgroup waves, `iters` x 4 v_mfma_f32_32x32x16_bf16
 * each, no memory traffic) launched back to back for at least min_seconds; reports the LAST launch: sustained TFLOP/s and the median
 * shader clock of its waves.  random_operands != 0: four pseudo-random A / B fragment pairs take turns (operand buses toggle as in
 * a convolution; the part draws more power and holds a lower clock than on the constant operands of random_operands = 0).
 * Synchronises `stream`. */
int sd_probe_mfma_rate(int n_workgroups, int waves_per_workgroup, int iters, double min_seconds, int random_operands,
                       double* tflops_out, double* shader_ghz_out, void* stream);
/* Copy activation buffer `buf` of the last sd_forward out of the workspace as float32 planar (C, d, h, w);
 * dims are returned in dims4 = {C, d, h, w}.  out_dev may be NULL to query dims only. */
int sd_debug_read_buffer(sd_model* m, int buf, const void* workspace_dev, float* out_dev, int32_t* dims4,
                         void* stream);
int sd_model_num_ops(const sd_model* m);
/* Number of plan ops the last sd_forward* call executed as launches of their own (the others ran inside a fused launch:
 * pooling / final layer in a convolution's epilogue, first convolution inside the second, the level-0 decoder inside its
 * up-convolution's launch).  For tests that must know which plan a shape was served by. */
int sd_debug_last_launch_count(const sd_model* m);
/* Which kernel computed plan op `op` in the last sd_forward* call: returns the index of the op whose LAUNCH did it (`op` itself, or the
 * op it is fused into: a pooling / final layer in a convolution's epilogue, a first convolution inside the second, the members of the
 * level-0 decoder), -1 when it did not run; the kernel symbol of that launch ("k_conv_mfma<bf16,3x3x3,NT=2,WAVES=8,NSLOT=0,MT=4,MODE=0>")
 * is copied into buf (n bytes, NUL-terminated).  What bench.py names its roofline kernel by -- the launchers note what they picked. */
int sd_debug_op_kernel(const sd_model* m, int op, char* buf, int n);

const char* sd_last_error(void);
const char* sd_version(void);

/* ---- KNOSSOS overlay cubes (host side, no GPU needed) -------------------------------
 * Snappy raw-format codec for "*.seg.sz.zip": knossos_utils (third-party, called at
 * /root/reference/syconn/handler/prediction.py:700-702, 835-843) stores each 128^3 uint64 cube as
 * python-snappy compress(cube.tobytes()) inside a zip member.  Restates google/snappy format_description.txt (pinned
 * upstream: snappy 1.1.8 / python-snappy 0.6.0); any conforming stream decodes, the encoder's output is decodable by
 * any conforming decoder.  All return SD_OK or SD_ERR_INVALID (corrupt / truncated stream, capacity too small). */
size_t sd_snappy_max_compressed_length(size_t n);
int sd_snappy_compress(const void* src, size_t n, void* dst, size_t dst_capacity, size_t* dst_len);
int sd_snappy_uncompressed_length(const void* src, size_t n, size_t* result);
int sd_snappy_uncompress(const void* src, size_t n, void* dst, size_t dst_capacity, size_t* dst_len);

/* Order-0 down-sampling by 2 per axis on the device = one level of the mag pyramid KnossosDataset.save_raw /
 * save_seg(..., mags=[m, 2m, 4m], fast_resampling=True) writes (prediction.py:834-843): dst[z,y,x] = src[2z,2y,2x],
 * dst dims = ceil(src dims / 2).  dtype: SD_U8 or SD_U64. */
int sd_downsample2(const void* src_dev, int dtype, int D, int H, int W, void* dst_dev, void* stream);

/* ---- first consumer of the myelin probability map -----------------------------------
 * map_myelin2coords (/root/reference/syconn/reps/super_segmentation_helper.py:550-615): for each of n boxes with
 * origin origins_zyx[3i..3i+2] (voxels of `vol`, may lie partly outside = zeros, like kd.load_raw) and extent
 * (ez,ey,ex): out[i] = (count(vol > thresh_proba) / (ez*ey*ex) > thresh_majority), the division in float64 as in
 * the reference (:611-612).  vol: (D,H,W) uint8 on the device; origins int32 and out uint8 on the device. */
int sd_box_majority(const uint8_t* vol_dev, int D, int H, int W, const int32_t* origins_zyx_dev, size_t n, int ez, int ey,
                    int ex, double thresh_proba, double thresh_majority, uint8_t* out_dev, void* stream);

/* ---- label-volume statistics ------------------------------------------------------------
 * Device counterpart of the reference's Cython natives /root/reference/syconn/extraction/find_object_properties_C.pyx:
 * find_object_properties (:24-49), map_subcell_C (:72-109), map_subcell_extract_props (:112-192).  Volumes are
 * (X,Y,Z) with z fastest (the reference indexes chunk[x, y, z]), dtype SD_U32 or SD_U64, id 0 = background.
 * One streaming pass fills open-addressing hash tables in CALLER-OWNED device memory:
 *   object table  (sd_objtable_bytes(cap) bytes, cap a power of two <= 2^31): per non-zero id the smallest raster index
 *                 (= the reference's representative coordinate, the first voxel its scan meets), the voxel count and the
 *                 bounding box [min, max + 1);
 *   pair table    (sd_pairtable_bytes(cap) bytes): per (subcell id, cell id) the number of voxels where both are set.
 * sd_segstats_scan initialises the tables itself.  cell_dev may be NULL (properties of the `sub` volumes only); n_sub may
 * be 0 (= find_object_properties(cell)); want_props = 0 computes the overlap counts only (= map_subcell_C).
 * status_dev: int32[2], set to 1 when the object tables ([0]) / pair tables ([1]) were too small -- the caller retries
 * with a larger capacity (results of an overflowed pass are incomplete and must be discarded). */
size_t sd_objtable_bytes(size_t capacity);
size_t sd_pairtable_bytes(size_t capacity);
int sd_segstats_scan(const void* cell_dev, const void* const* sub_devs /* host array of device pointers */, int n_sub,
                     int dtype, int X, int Y, int Z, void* cell_table, void* const* sub_tables, size_t cap_obj,
                     void* const* pair_tables, size_t cap_pair, int want_props, int32_t* status_dev, void* stream);
/* Turn a filled object table into dense arrays (any order): ids / first raster index / voxel count (uint64 each) and
 * bbox int32[n][6] = (min x,y,z, max+1 x,y,z).  *count_dev = number of objects (may exceed max_out: then only max_out
 * records were written). */
int sd_segstats_compact_objects(const void* table, size_t cap_obj, uint64_t* ids_dev, uint64_t* first_dev,
                                uint64_t* size_dev, int32_t* bbox_dev, size_t max_out, uint64_t* count_dev, void* stream);
/* Dense (subcell id, cell id, overlap count) triples of one pair table; the ids are looked up in the two object tables
 * the same sd_segstats_scan call filled. */
int sd_segstats_compact_pairs(const void* pair_table, size_t cap_pair, const void* sub_table, const void* cell_table,
                              size_t cap_obj, uint64_t* sub_ids_dev, uint64_t* cell_ids_dev, uint64_t* counts_dev,
                              size_t max_out, uint64_t* count_dev, void* stream);

/* ---- dataset-wide merge of per-chunk statistics (the chunk driver around the natives) ----------------
 * Replaces, on record arrays in HBM, what /root/reference/syconn/proc/sd_proc.py does with Python dictionaries per chunk:
 * the filter of _map_subcell_extract_props_thread (:640-650, :657-670: an object that lies purely inside its chunk -- on none of the
 * six faces -- and has fewer than min_obj_vx voxels is dropped, for organelles from the overlap counts too), merge_prop_dicts
 * (:1248-1273) and merge_map_dicts (:1300-1322).
 * sd_chunkprops_append: reads an object table sd_segstats_scan filled for a chunk of extent (X,Y,Z) at origin (ox,oy,oz) and appends
 *   one record per surviving object at *cursor_dev (a device counter the caller zeroes once per dataset; NOT reset here): id, global
 *   representative coordinate int32[3], global box int32[6] = (min, max + 1), voxel count.  min_obj_vx <= 1: no filter.  Records
 *   beyond max_records are not written but still counted: the caller compares the final cursor with max_records.
 * sd_chunkpairs_append: the same for a pair table: (subcell id, cell id, overlap voxels), filter by the SUBCELL table's entry. */
int sd_chunkprops_append(const void* table, size_t cap_obj, int X, int Y, int Z, int ox, int oy, int oz, uint64_t min_obj_vx,
                         uint64_t* ids_dev, int32_t* rc_dev, int32_t* bbox_dev, uint64_t* sizes_dev, size_t max_records,
                         uint64_t* cursor_dev, void* stream);
int sd_chunkpairs_append(const void* pair_table, size_t cap_pair, const void* sub_table, const void* cell_table, size_t cap_obj,
                         int X, int Y, int Z, uint64_t min_obj_vx, uint64_t* sub_ids_dev, uint64_t* cell_ids_dev, uint64_t* counts_dev,
                         size_t max_records, uint64_t* cursor_dev, void* stream);
/* Merge n appended records (chunks appended in processing order): stable sort by id + one segment per id.
 *   uniq_ids / tot_sizes / last_rc[.][3]: per id (ascending) the summed voxel count and the representative coordinate of the LAST
 *   chunk holding it (dict.update order of merge_prop_dicts); seg_begin[u]: first position of id u in bbox_sorted int32[n][6], the
 *   per-chunk boxes in chunk order (the reference keeps a list of boxes per id); *n_unique_dev: number of ids.  Output arrays hold n
 *   entries each; temp_dev: sd_propmerge_temp_bytes(n) bytes.
 * sd_propmerge_pairs: unique (subcell id, cell id) ascending lexicographically with summed counts. */
size_t sd_propmerge_temp_bytes(size_t n_records);
int sd_propmerge_objects(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev, size_t n,
                         uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev, uint32_t* seg_begin_dev,
                         int32_t* bbox_sorted_dev, uint64_t* n_unique_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_propmerge_pairs(const uint64_t* sub_ids_dev, const uint64_t* cell_ids_dev, const uint64_t* counts_dev, size_t n,
                       uint64_t* out_sub_dev, uint64_t* out_cell_dev, uint64_t* out_counts_dev, uint64_t* n_unique_dev, void* temp_dev,
                       size_t temp_bytes, void* stream);

/* ---- globally unique objects across chunks (the steps behind the per-chunk first stage) ----------------
 * make_unique_labels (/root/reference/syconn/extraction/object_extraction_steps.py:369-443: `matrix[matrix > 0] += offset` on the
 * chunk's component labels widened to uint64, offset = number of components in all earlier chunks,
 * object_extraction_wrapper.py:300-312): labels_dev int32[n] -> out_dev uint64[n]. */
int sd_labels_make_unique(const int32_t* labels_dev, size_t n, uint64_t offset, uint64_t* out_dev, void* stream);
/* Cut the box [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz) out of an (X,Y,Z) uint64 label volume (z fastest) into a contiguous
 * (nx,ny,nz) array, optionally through a look-up table: dst = lut[src] (lut_dev NULL: dst = src).  Serves
 *   * apply_merge_list (object_extraction_steps.py:717-731): crop the chunk's overlap margin and map every id through the
 *     merge list (`id_changer[this_cc]`), lut_len = max_label + 1;
 *   * the face slabs make_stitch_list compares (:560-575, cut_array_in_one_dim), whose co-occurring id pairs sd_segstats_scan counts.
 * status_dev (optional int32): set to 1 when an id >= lut_len was met (it passes through unmapped). */
int sd_labels_box_lut(const uint64_t* src_dev, int X, int Y, int Z, int x0, int y0, int z0, int nx, int ny, int nz,
                      const uint64_t* lut_dev, size_t lut_len, uint64_t* dst_dev, int32_t* status_dev, void* stream);

/* ---- probability map -> object segmentation, first stage ---------------------------------
 * Non-watershed branches of _object_segmentation_thread (/root/reference/syconn/extraction/object_extraction_steps.py:
 * 316-317 threshold, 354-358 morphology + scipy.ndimage.label) with the morphology semantics of
 * /root/reference/syconn/proc/image.py:357-438, 485-507 (_multi_mop_findobjects / apply_morphological_operations) on a
 * binary volume.  prob_dev: (X,Y,Z) uint8, z fastest (the reference's arrays are x,y,z here).
 *   threshold   uint8 scale, mask = prob > threshold (0: prob already is a 0/1 mask, object_extraction_steps.py:316);
 *   ops/iterations (HOST arrays, n_ops entries): the reference's operation list with runs of equal operations merged
 *               into `iterations` (image.py:510-519).  SD_MOP_EROSION selects the reference's watershed branch
 *               (:319-352) and is rejected here with SD_ERR_INVALID: use sd_object_segmentation_watershed below.
 *   struct_host (sx,sy,sz) uint8 HOST array, odd extents: the structuring element (get_aniso_struct, image.py:522-539);
 *   labels_dev  (X,Y,Z) int32: 6-connected components numbered 1..N in raster order of their first voxel, 0 = background
 *               -- identical to scipy.ndimage.label; *max_label_dev = N;
 *   mask_out_dev optional (X,Y,Z) uint8: the binary volume after the morphology.
 * Workspace: sd_objseg_workspace_bytes(X, Y, Z, largest `iterations` of any closing / dilation). */
enum sd_morph_op { SD_MOP_OPENING = 1, SD_MOP_CLOSING = 2, SD_MOP_DILATION = 3, SD_MOP_EROSION = 4 };
size_t sd_objseg_workspace_bytes(int X, int Y, int Z, int max_iterations);
int sd_object_segmentation(const uint8_t* prob_dev, int X, int Y, int Z, double threshold, const int32_t* ops,
                           const int32_t* iterations, int n_ops, const uint8_t* struct_host, int sx, int sy, int sz,
                           int32_t* labels_dev, int32_t* max_label_dev, uint8_t* mask_out_dev, void* workspace_dev,
                           size_t ws_bytes, void* stream);

/* Mask-only form of the same morphology (cs_extraction_steps.py:405-408: apply_morphological_operations on the sj mask): mask =
 * in > threshold (0: any value != 0), then the operation list (erosion allowed here; runs merged by the caller), mask_out_dev
 * (X,Y,Z) uint8 = the 0/1 result.  An empty mask stays empty.  Workspace: sd_objseg_workspace_bytes as above. */
int sd_binary_morphology(const uint8_t* in_dev, int X, int Y, int Z, double threshold, const int32_t* ops, const int32_t* iterations,
                         int n_ops, const uint8_t* struct_host, int sx, int sy, int sz, uint8_t* mask_out_dev, void* workspace_dev,
                         size_t ws_bytes, void* stream);

/* The WATERSHED branch of the same function (object_extraction_steps.py:319-352) -- what SyConn's default config selects for
 * mi / sj / vc (config.yml:130-136: opening, closing, erosion(s)); taken when the operation list contains 'binary_erosion':
 *   ops / iterations          the operations BEFORE the first erosion -> tmp_data (:320-322);
 *   seed_ops / ...            the operations from the first erosion on (runs merged separately, image.py:510-519), applied to a
 *                             copy of tmp_data -> scipy.ndimage.label -> markers (:323-327);
 *   min_seed_vx               > 1: markers with fewer voxels are deleted and the freed ids handed to the largest surviving ids
 *                             (the reference's hole filling + relabel_vol, :330-347; block_processing_C.pyx:161-169);
 *   pixel_pitch_xyz           HOST int32[3] voxel size (scaling.astype(uint32)): the distance transform of tmp_data to its
 *                             background is exact Euclidean with that pitch (vigra distanceTransform(background=False), :349);
 *   labels_dev                skimage.segmentation.watershed(-distance, markers, mask=tmp_data) (:351): priority flood, 6-connected;
 *   markers_out_dev           optional (X,Y,Z) int32: the relabelled marker volume -- everything up to here is scipy / numpy in the
 *                             reference and reproduced bit for bit (pinned by tests/golden/g10_objseg_ws.npz);
 *   distance_out_dev          optional (X,Y,Z) float32: the distance transform.
 * vigra and skimage are absent from the reference tree and this image: distance transform and flood restate their published
 * algorithms (flood order: value, then age, marker voxels of equal value by raster index) and are parity-UNPINNED. */
size_t sd_objseg_watershed_workspace_bytes(int X, int Y, int Z, int max_iterations);
int sd_object_segmentation_watershed(const uint8_t* prob_dev, int X, int Y, int Z, double threshold, const int32_t* ops,
                                     const int32_t* iterations, int n_ops, const int32_t* seed_ops,
                                     const int32_t* seed_iterations, int n_seed_ops, const uint8_t* struct_host, int sx, int sy,
                                     int sz, int min_seed_vx, const int32_t* pixel_pitch_xyz, int32_t* labels_dev,
                                     int32_t* max_label_dev, int32_t* markers_out_dev, float* distance_out_dev,
                                     uint8_t* mask_out_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* The flood of that branch on its own: skimage.segmentation.watershed(-distance, markers, mask) (:351; watershed_raveled with
 * connectivity 1, no compactness, no watershed line) for distance^2 = d2_dev (int32 >= 0), an int32 marker volume (0 = none;
 * markers outside the mask are ignored) and a uint8 mask, all (X,Y,Z) with z fastest.  Pop order: higher d2 first, then
 * first-in first-out, marker voxels (all queued before anything else) among themselves by raster index; a voxel takes the label
 * of the popped neighbour that reaches it first.  Runs level-synchronously, one workgroup per mask component that holds several
 * markers (csrc/sd_objseg.hip::k_ws_flood); SD_WS_SEQUENTIAL=1 in the environment selects a sequential restatement (one lane per
 * component) that the tests cross-check it with.  Workspace: sd_objseg_watershed_workspace_bytes(X, Y, Z, 0). */
int sd_marker_flood(const int32_t* d2_dev, const int32_t* markers_dev, const uint8_t* mask_dev, int X, int Y, int Z,
                    int32_t* labels_dev, int32_t* max_label_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* Gaussian pre-smoothing of a probability map followed by the threshold (object_extraction_steps.py:296-297
 * `gaussianSmoothing(tmp_data, sigmas[...])`, vigra; :316-317 `tmp_data > thresholds[...]`) -- the optional first step of
 * _object_segmentation_thread (SyConn's own pipeline passes no sigmas).  prob_dev (X,Y,Z) uint8, z fastest; sigma_xyz HOST
 * double[3] per axis in voxels (0: axis not smoothed).  vigra's published algorithm restated (parity UNPINNED, vigra is absent
 * here): separable, axis order x, y, z, window radius int(3 sigma + 0.5) (>= 1, <= 64) of exp(-t^2 / 2 sigma^2) normalised to
 * sum 1, reflective border without repeating the edge, sums in double, every pass stored as float32.
 *   mask_dev     (X,Y,Z) uint8: 1 where smoothed > threshold (uint8 scale like the input), else 0 -- pass it to
 *                sd_object_segmentation* with threshold 0;
 *   smoothed_dev optional (X,Y,Z) float32: the smoothed map. */
size_t sd_gauss_workspace_bytes(int X, int Y, int Z);
int sd_gaussian_threshold(const uint8_t* prob_dev, int X, int Y, int Z, const double* sigma_xyz, double threshold,
                          uint8_t* mask_dev, float* smoothed_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* ---- contact sites (/root/reference/syconn/extraction/cs_extraction_steps.py:317-495) ----------
 * detect_seg_boundaries (/root/reference/syconn/extraction/find_object_properties.py:424-455): mask_dev (X,Y,Z) uint8 = 1 where a
 * non-zero voxel of seg_dev (uint32, z fastest) has an in-array 6-neighbour of another value (0 included), else 0. */
int sd_seg_boundaries(const uint32_t* seg_dev, int X, int Y, int Z, uint8_t* mask_dev, void* stream);
/* process_block_nonzero + kernel (/root/reference/syconn/extraction/block_processing_C.pyx:21-75): valid convolution of the
 * (sx,sy,sz) stencil (odd extents) over seg_dev; out_dev uint64 (X-sx+1, Y-sy+1, Z-sz+1).  For a centre with edges_dev != 0 the
 * most frequent id of its window other than 0 and the centre id c wins (ties: the smallest id), out = (min(c,k) << 32) | max(c,k);
 * 0 when the window holds no other id or the centre is not flagged.  Exact for any number of distinct ids per window (windows
 * with more than 8 go through an exact second kernel).  Stencils up to (sx+7)(sy+7)(sz+15) <= 16384 and sx*sy*sz <= 4096.
 * Workspace: sd_contact_partners_workspace_bytes(). */
size_t sd_contact_partners_workspace_bytes(void);
int sd_contact_partners(const uint8_t* edges_dev, const uint32_t* seg_dev, int X, int Y, int Z, int sx, int sy, int sz,
                        uint64_t* out_dev, void* workspace_dev, size_t ws_bytes, void* stream);
/* The closing loop of _contact_site_extraction_thread (cs_extraction_steps.py:437-461) on a contact volume c0_dev (uint64, X,Y,Z):
 * per site id, res = binary_dilation^n_dilate(binary_closing^n_close(c0 == id)) (6-connected cross, border_value 0) computed inside
 * the site's box only, and background voxels of c0 inside res take the id.  Where several sites claim a voxel the SMALLEST id wins
 * (the reference's order is that of an unordered_map: DESIGN.md section 7).  One call handles a batch of sites:
 *   table_dev  int64[n_obj][8]: id, box origin x, y, z, box extent x, y, z (the reference's [max(lo - n_close, 0), hi + n_close)
 *              clipped at the array end), offset of the box in the workspace planes (ascending; boxes packed without gaps);
 *   tot_vox    summed box volume of the batch; workspace >= 2 * tot_vox bytes;
 *   flags      SD_CS_FIRST: out = c0 before the batch (first batch); SD_CS_LAST: unclaimed voxels become 0 (last batch).
 * Voxels that are non-zero in c0 keep their value.  The id 2^64 - 1 is reserved (it marks unclaimed voxels): no site may carry
 * it (packed cell pairs never do). */
enum sd_cs_flags { SD_CS_FIRST = 1, SD_CS_LAST = 2 };
int sd_cs_close_dilate(const uint64_t* c0_dev, int X, int Y, int Z, const int64_t* table_dev, int64_t n_obj, int64_t tot_vox,
                       int n_close, int n_dilate, int flags, uint64_t* out_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* Synapse statistics of the contact sites of a chunk (/root/reference/syconn/extraction/block_processing_C.pyx:78-158
 * extract_cs_syntype, called by _contact_site_extraction_thread, cs_extraction_steps.py:464-470).  All volumes are (X,Y,Z) with z
 * fastest; the calls read the window [ox, ox+nx) x [oy, oy+ny) x [oz, oz+nz) of them (the worker's core inside its halo volume).
 *   sd_cs_syntype_scan     one pass over cs_dev (uint32 / uint64 site ids, 0 = background) and the uint8 masks syn_dev (any value
 *                          != 0 is syn), asym_dev, sym_dev (== 1 counts) into the hash table of `cap` slots (power of two,
 *                          sd_cs_syntype_table_bytes(cap) bytes; the call initialises it).  Per site: the cs record (first voxel in
 *                          the x, y, z scan, box, size), the syn record (the same over its syn voxels) and the voxel counts of
 *                          syn && asym == 1 and syn && sym == 1.  cs_out_dev / syn_out_dev (optional, (nx,ny,nz) of the id type): the
 *                          window's ids, and its ids where syn != 0 else 0 (the worker's syn segmentation, :476-480).
 *                          *status_dev = 1 when the table overflowed: repeat with a larger capacity.
 *   sd_cs_syntype_compact  the occupied slots: ids_dev / slots_dev (unordered), *count_dev = their number.
 *   sd_cs_syntype_records  rec_dev int64[n][SD_CST_COLS] for the slots in the order given (the caller sorts them by id):
 *                          0 id | 1-3 first voxel (window coordinates) | 4 size | 5-7 box min | 8-10 box max + 1 |
 *                          11-20 the same for the syn voxels (zeros when the site has none) | 21 asym count | 22 sym count |
 *                          23 offset of the site's syn voxels (exclusive sum of column 14); *n_syn_dev = the total.
 *   sd_cs_syntype_voxels   vox_dev int64[n_syn][3]: every site's syn voxels in scan order from row column 23 on, as window
 *                          coordinates + offset_host[3] (HOST array; voxels_syn of the reference).  *status_dev = 1 if a count
 *                          disagreed with the records (not expected).
 * sd_syntype_masks: the syn-type masks of the worker (cs_extraction_steps.py:411-433) on n voxels: dtype SD_U8 (raw data):
 * out_a = vol >= 123; SD_U64 (labels): out_a = vol == label_a and, when out_b_dev is given, out_b = vol == label_b. */
enum { SD_CST_COLS = 24 };
size_t sd_cs_syntype_table_bytes(size_t capacity);
int sd_cs_syntype_scan(const void* cs_dev, int dtype, const uint8_t* syn_dev, const uint8_t* asym_dev, const uint8_t* sym_dev, int X,
                       int Y, int Z, int ox, int oy, int oz, int nx, int ny, int nz, void* table_dev, size_t cap, void* cs_out_dev,
                       void* syn_out_dev, int32_t* status_dev, void* stream);
int sd_cs_syntype_compact(const void* table_dev, size_t cap, uint64_t* ids_dev, int32_t* slots_dev, size_t max_out,
                          uint64_t* count_dev, void* stream);
int sd_cs_syntype_records(const void* table_dev, size_t cap, const int32_t* slots_dev, int64_t n, int nx, int ny, int nz,
                          int64_t* rec_dev, int64_t* n_syn_dev, void* stream);
int sd_cs_syntype_voxels(const void* cs_dev, int dtype, const uint8_t* syn_dev, int X, int Y, int Z, int ox, int oy, int oz,
                         const int64_t* rec_dev, int64_t n, int64_t n_syn, const int64_t* offset_host, int64_t* vox_dev,
                         int32_t* status_dev, void* stream);
int sd_syntype_masks(const void* vol_dev, int dtype, size_t n, uint64_t label_a, uint64_t label_b, uint8_t* out_a_dev,
                     uint8_t* out_b_dev, void* stream);

/* Dataset-wide merge of contact sites and synapses (/root/reference/syconn/extraction/cs_extraction_steps.py: the running merges
 * of _contact_site_extraction_thread :484-492, _write_props_collect_helper :631-673 and the merge / join / filter of
 * _write_props_to_syn_thread :544-623), on record arrays that stay on the device; the counterpart of sd_chunkprops_append /
 * sd_propmerge_objects for the records of sd_cs_syntype_records.  Coordinates are int32, ids uint64, counts uint64.
 *   sd_cs_merge_append    one chunk core: rec_dev int64[n][SD_CST_COLS] and vox_dev int64[n_vox][3] (n_vox = the sum of column 14,
 *                         rows as sd_cs_syntype_voxels lays them out, origin already added there).  Appends at cursors_dev (uint64[3]:
 *                         cs records, syn records, voxel rows; zeroed by the caller before the first chunk) one cs record per site
 *                         (id, first voxel + (ox,oy,oz), box + (ox,oy,oz), size), one syn record per site with column 14 > 0 (the
 *                         same from columns 11-20, the asym and sym counts, and the row at which its voxel run starts in vox_all_dev;
 *                         the run's length is its size) and the voxel rows as uint32[.][3].  Cursors count past max_cs / max_syn /
 *                         max_vox (the caller detects the overrun); nothing is written beyond them.  Asynchronous, no host sync.
 *   sd_cs_merge_objects   n records -> one row per id with merged size >= min_obj_vx, ids ascending: uniq_ids, tot_sizes, last_rc
 *                         [.][3] (the record appended last), union_bbox [.][6] (min of mins | max of maxes), seg_begin = first slot of
 *                         the id in bbox_sorted [.][6] (the kept records' boxes, id-major, append order inside an id).
 *                         counts_dev uint64[4] = kept ids, kept boxes, 0, ids before the filter.  Outputs hold n rows; temp: sd_cs_merge_temp_bytes(n).
 *   sd_cs_merge_synapses  the same for the syn records, and: an id is kept only if it is among cs_ids_dev[n_cs] (ascending: the
 *                         uniq_ids sd_cs_merge_objects kept) -- cs_size = cs_sizes_dev there; asym_tot / sym_tot = summed counts;
 *                         vox_out_dev uint32[.][3] = the voxel runs of every kept id gathered into one run (append order inside an id,
 *                         row order inside a run), starting at row vox_begin; counts_dev[2] = kept rows, [3] = ids before the filter.
 *                         vox_out holds n_vox rows.
 * Limits: n < 2^32 records and n_vox < 2^32 voxel rows per merge call (SD_ERR_INVALID otherwise). */
int sd_cs_merge_append(const int64_t* rec_dev, size_t n, const int64_t* vox_dev, size_t n_vox, int ox, int oy, int oz,
                       uint64_t* cs_ids_dev, int32_t* cs_rc_dev, int32_t* cs_bbox_dev, uint64_t* cs_sizes_dev, size_t max_cs,
                       uint64_t* syn_ids_dev, int32_t* syn_rc_dev, int32_t* syn_bbox_dev, uint64_t* syn_sizes_dev, uint64_t* syn_asym_dev,
                       uint64_t* syn_sym_dev, uint64_t* syn_vpos_dev, size_t max_syn, uint32_t* vox_all_dev, size_t max_vox,
                       uint64_t* cursors_dev, void* stream);
size_t sd_cs_merge_temp_bytes(size_t n_records);
int sd_cs_merge_objects(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev, size_t n,
                        uint64_t min_obj_vx, uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev,
                        int32_t* union_bbox_dev, uint32_t* seg_begin_dev, int32_t* bbox_sorted_dev, uint64_t* counts_dev, void* temp_dev,
                        size_t temp_bytes, void* stream);
int sd_cs_merge_synapses(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev,
                         const uint64_t* asym_dev, const uint64_t* sym_dev, const uint64_t* vpos_dev, size_t n,
                         const uint32_t* vox_all_dev, size_t n_vox, const uint64_t* cs_ids_dev, const uint64_t* cs_sizes_dev, size_t n_cs,
                         uint64_t min_obj_vx, uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev,
                         int32_t* union_bbox_dev, uint32_t* seg_begin_dev, int32_t* bbox_sorted_dev, uint64_t* asym_tot_dev,
                         uint64_t* sym_tot_dev, uint64_t* cs_size_dev, uint32_t* vox_begin_dev, uint32_t* vox_out_dev,
                         uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);

/* Synapse agglomeration: supervoxel-level syn fragments -> cell-level synapses (/root/reference/syconn/extraction/
 * cs_processing_steps.py: connected_cluster_kdtree :552-602 and the per-component half of _combine_and_split_syn_thread :453-474),
 * for all cell pairs ("groups") of a dataset in one set of launches.  vox_dev int32[n_vox][3] holds the voxels in the reference's flat
 * order (group-major, the fragments of a group in list order, stored order inside a fragment), vox_frag_dev[n_vox] the fragment
 * number of every voxel (ascending), frag_group_dev[n_frag] the group of every fragment, group_origin_dev int32[n_group][3] the
 * smallest coordinate of every group.
 *   sd_syn_ssv_components  replaces :552-602: labels_dev[n_vox] = the component of every voxel, numbered over the whole input in
 *                          ascending order of the component's smallest flat index (the reference's order inside a group; groups in
 *                          input order).  Two voxels of a group are joined when their scaled distance (float64 of voxel * scale) is
 *                          strictly below gap_nm.  cell_host[3] = the binning cell in voxels (its scaled diagonal must be below the
 *                          gap), bits_host[3] = key bits per axis for the cell coordinates relative to the group origin.  stages: bit 0
 *                          cells, bit 1 link, bit 2 number (7 = all; a probe times them apart on one scratch).  counts_dev uint64[8] =
 *                          components, cells, neighbour cells found, of those: too far by their boxes, joined by their boxes alone,
 *                          in one set already, voxel-tested; [7] != 0: an input row was out of range (results invalid).
 *   sd_syn_ssv_stats       replaces :456-474: comp_begin_dev[n_comp + 1] = offsets of the components in the (component, flat index)
 *                          order (sizes are the differences), bbox_dev int32[n_comp][6] (min | max, inclusive), rep_flat_dev[n_comp] =
 *                          flat index of the voxel nearest the scaled mean of all voxels (ties: the smallest flat index), the voxel
 *                          count of every (component, fragment) that occurs: pair_comp / pair_frag / pair_begin (n_vox + 1 rows
 *                          reserved, counts_dev[0] used, pair_begin has one more), and vox_out_dev uint32[.][3] = the voxels of the
 *                          components with >= min_obj_vx voxels, component-major, ascending flat index inside (counts_dev[1] rows).
 *                          counts_dev uint64[4]; [3] != 0: a label was >= n_comp.
 * Scratch for either: sd_syn_ssv_temp_bytes(n_vox).  Limits: n_vox < 2^31, group bits + cell bits <= 63 (SD_ERR_INVALID otherwise). */
size_t sd_syn_ssv_temp_bytes(size_t n_vox);
int sd_syn_ssv_components(const int32_t* vox_dev, const uint32_t* vox_frag_dev, const uint32_t* frag_group_dev, const int32_t* group_origin_dev,
                          size_t n_vox, size_t n_frag, size_t n_group, const double* scale_host, double gap_nm, const int32_t* cell_host,
                          const int32_t* bits_host, int stages, int32_t* labels_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                          void* stream);
int sd_syn_ssv_stats(const int32_t* vox_dev, const uint32_t* vox_frag_dev, const int32_t* labels_dev, size_t n_vox, size_t n_comp,
                     const double* scale_host, uint64_t min_obj_vx, uint32_t* comp_begin_dev, int32_t* bbox_dev, uint32_t* rep_flat_dev,
                     uint32_t* pair_comp_dev, uint32_t* pair_frag_dev, uint32_t* pair_begin_dev, uint32_t* vox_out_dev, uint64_t* counts_dev,
                     void* temp_dev, size_t temp_bytes, void* stream);

/* Organelles of the partner cells mapped to the cell-level synapses: cps.map_objects_from_synssv_partners of the reference
 * (extraction/cs_processing_steps.py:811-1093), one organelle type per call.  A side is (synapse row i, partner slot p) = 2 i + p.
 *   sd_synssv_map_pairs  replaces :955-965 (three cKDTrees per cell, query_ball_tree): side_cell_dev[n_sides] = the cell of every side
 *                        (neuron_partners row-major; 0 = none), syn_rep_dev int32[n_sides / 2][3]; the organelles that have a cell,
 *                        sorted by cell: org_cell_dev[n_org] ascending, org_row_dev[n_org] = the row that is reported for each,
 *                        org_rep_dev int32[n_org][3].  An organelle is a candidate of a side of its cell when the float64 distance
 *                        of rep * scale is <= max_rep_dist_nm (compared as d^2 <= D^2).  Without pair_obj_dev: side_begin_dev
 *                        [n_sides + 1] = offsets of the sides in the pair list, counts_dev uint64[8], [0] = pairs.  With pair_obj_dev
 *                        [pair_cap] (and the side_begin_dev of the first call): the reported rows, side-major, in the order of the
 *                        cell's run.  Scratch: sd_synssv_map_pairs_temp_bytes(n_sides).
 *   sd_synssv_map_query  replaces :1032-1045 (one cKDTree per synapse, queried per organelle).  vox_dev uint32[n_vox][3] /
 *                        vox_begin_dev uint64[n_syn + 1] = the voxel runs, sampled_begin_dev uint64[n_syn + 1] = offsets of the
 *                        sampled voxels (rows 0, f, 2 f, ... of every run: ceil(len / f) each, n_sampled_vox in all); vert_dev
 *                        float[n_vert][3] in nm / vert_begin_dev uint64[n_org + 1] over the rows pair_obj_dev names.  stages bit 0:
 *                        the sampled voxels as float64(voxel) * scale, sorted inside a synapse and cut into tiles of 64 with boxes
 *                        (kept in the scratch: a later call with bit 1 alone over the same scratch, n_syn, n_sampled_vox and
 *                        scratch_pairs reuses it); bit 1: per pair pair_len_dev = ceil(vertices / f), pair_close_dev = sampled
 *                        vertices whose nearest sampled voxel is at d^2 < R^2 (d^2 = ((dx dx) + dy dy) + dz dz in float64, nothing
 *                        fused), pair_min_d2_dev = bits of the smallest such d^2 (+inf if none).  Pairs are split into work items of
 *                        SD_SYNSSV_MAP_ITEM sampled vertices; n_items_hint sizes the grid (0: the largest).  counts_dev uint64[8] =
 *                        pairs, work items, vertices dropped by the synapse's box, tiles skipped, tiles staged, point tests, 0;
 *                        [7] != 0: an offset or row was out of range (results invalid).
 *                        Scratch: sd_synssv_map_query_temp_bytes(n_syn, n_sampled_vox, scratch_pairs), scratch_pairs >= n_pairs.
 * Asynchronous on the stream.  Limits (SD_ERR_INVALID beyond): n_sides, n_org, pairs, n_sampled_vox < 2^31, n_syn < 2^30,
 * sample_fact >= 1; on the device: < 2^32 sampled vertices per organelle and < 2^32 work items per call (counts_dev[7]). */
#define SD_SYNSSV_MAP_ITEM 1024
size_t sd_synssv_map_pairs_temp_bytes(size_t n_sides);
int sd_synssv_map_pairs(const uint64_t* side_cell_dev, const int32_t* syn_rep_dev, size_t n_sides, const uint64_t* org_cell_dev,
                        const uint32_t* org_row_dev, const int32_t* org_rep_dev, size_t n_org, const double* scale_host,
                        double max_rep_dist_nm, uint32_t* side_begin_dev, uint32_t* pair_obj_dev, size_t pair_cap, uint64_t* counts_dev,
                        void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_synssv_map_query_temp_bytes(size_t n_syn, size_t n_sampled_vox, size_t n_pairs);
int sd_synssv_map_query(const uint32_t* vox_dev, const uint64_t* vox_begin_dev, const uint64_t* sampled_begin_dev, size_t n_syn, size_t n_vox,
                        size_t n_sampled_vox, const float* vert_dev, const uint64_t* vert_begin_dev, size_t n_org, size_t n_vert,
                        const uint32_t* side_begin_dev, const uint32_t* pair_obj_dev, size_t n_pairs, size_t scratch_pairs, int sample_fact,
                        const double* scale_host, double max_vert_dist_nm, int stages, size_t n_items_hint, uint32_t* pair_close_dev,
                        uint32_t* pair_len_dev, uint64_t* pair_min_d2_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                        void* stream);

/* Properties of the partner cells at every cell-level synapse and the synapse classifier (csrc/sd_syn_props.hip).
 *   sd_syn_props_knn     replaces the two cKDTrees per cell of cps._collect_properties_from_ssv_partners_thread (/root/reference/syconn/
 *                        extraction/cs_processing_steps.py:161-164): colorcode_vertices (reps/rep_helper.py:320-330, k nearest mesh
 *                        vertices and a Counter vote) and attr_for_coords (reps/super_segmentation_object.py:2961-2963, the nearest
 *                        skeleton node), for all cells in one call.  points_dev [n_points][3], float64 or (points_f32 != 0) float32
 *                        widened exactly; cell c owns rows begin_dev[c] .. begin_dev[c + 1] (uint64[n_cells + 1], ascending from 0 to
 *                        n_points); labels_dev int32[n_points], or NULL: the label of a point is its row.  Query q = (q_cell_dev[q],
 *                        q_xyz_dev[q][3]).  Its neighbours are the k_eff = min(k, points of the cell) points of its cell with the
 *                        smallest (d^2, row), d^2 = ((dx dx) + dy dy) + dz dz in float64, nothing fused.  vote_dev[q] = the label with
 *                        the highest count among them, on equal counts the one that occurs first in that order (-1 for a cell without
 *                        points); optional nn_idx_dev int32[n_q][k] / nn_d2_dev double[n_q][k] = the neighbours in that order, padded
 *                        with -1 / +inf.  stages bit 0: sort the points inside every cell and cut them into tiles of 64 with boxes
 *                        (kept in the scratch: a later call with bit 1 alone over the same scratch, points and cells reuses it); bit 1:
 *                        the queries.  counts_dev uint64[8] = tiles visited, tiles skipped by their box, ...; [7] != 0: an offset, a
 *                        cell row or a point row was out of range (results invalid).
 *                        Scratch: sd_syn_props_knn_temp_bytes(n_points, n_cells).  Limits (SD_ERR_INVALID beyond): 1 <= k <=
 *                        SD_SYN_PROPS_MAX_K, n_points, n_q, n_cells < 2^31.
 *   sd_syn_props_forest  replaces rfc.predict_proba([feats]) per synapse (cs_processing_steps.py:1155-1156).  The packed forest: per
 *                        node feature_dev, threshold_dev, left_dev / right_dev (rows of the node arrays, -1 at a leaf; a child's row is
 *                        above its parent's), proba_dev double[n_nodes][n_classes] (the class fractions of the node), tree_begin_dev
 *                        [n_trees + 1] = the root of every tree.  out_dev double[n_rows][n_classes]: rows_dev double[n_rows]
 *                        [n_features] cast to float32, in every tree left iff x[feature] <= threshold (float32 widened), the leaves'
 *                        fractions added in tree order, divided by n_trees.  counts_dev uint64[8]; [7] != 0: a node or feature was out
 *                        of range.
 * Asynchronous on the stream.  One grid stride of the kernels is SD_SYN_PROPS_CELL_GRID blocks of four cells, SD_SYN_PROPS_POINT_GRID
 * blocks of 256 points, SD_SYN_PROPS_QUERY_GRID blocks of four queries, SD_SYN_PROPS_FOREST_GRID blocks of 256 rows. */
#define SD_SYN_PROPS_MAX_K 64
#define SD_SYN_PROPS_CELL_GRID 4096
#define SD_SYN_PROPS_POINT_GRID 1024
#define SD_SYN_PROPS_QUERY_GRID 8192
#define SD_SYN_PROPS_FOREST_GRID 1024
size_t sd_syn_props_knn_temp_bytes(size_t n_points, size_t n_cells);
int sd_syn_props_knn(const void* points_dev, int points_f32, const uint64_t* begin_dev, size_t n_cells, size_t n_points,
                     const int32_t* labels_dev, const uint32_t* q_cell_dev, const double* q_xyz_dev, size_t n_q, int k, int stages,
                     int32_t* vote_dev, int32_t* nn_idx_dev, double* nn_d2_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                     void* stream);
int sd_syn_props_forest(const double* rows_dev, size_t n_rows, int n_features, const int32_t* feature_dev, const double* threshold_dev,
                        const int32_t* left_dev, const int32_t* right_dev, const double* proba_dev, const int32_t* tree_begin_dev, int n_trees,
                        int n_nodes, int n_classes, double* out_dev, uint64_t* counts_dev, void* stream);

/* ---- spine head volumes (csrc/sd_spinehead.hip) ------------------------------------------------------------------------
 * The per-window steps of extract_spinehead_volume_mesh (/root/reference/syconn/reps/super_segmentation_helper.py:2068-2198) that the
 * entries above do not cover.  All volumes (X,Y,Z) with z fastest, < 2^31 voxels; everything is asynchronous on the stream.  One grid
 * stride of the kernels is SD_SPINEHEAD_VOX_GRID blocks of 256 voxels (or peaks, or queries), SD_SPINEHEAD_VERT_GRID blocks of 256
 * (window, vertex) pairs, SD_SPINEHEAD_ID_GRID blocks of 256 table rows.  Scratch of every entry that takes `workspace_dev`:
 * sd_spinehead_workspace_bytes(X, Y, Z), which also covers sd_edt_squared and sd_marker_flood on the same extents.
 *   sd_edt_squared (csrc/sd_objseg.hip)  ndimage.distance_transform_edt(seg) (:2161) as exact SQUARED distances: d2_dev int32 = squared
 *                        Euclidean distance (pitch 1, 1, 1) of every mask voxel to the nearest voxel that is 0 INSIDE the array, 0 in the
 *                        background; the kernels of sd_object_segmentation_watershed on the whole volume.  A mask without any background
 *                        voxel gives 0x3f000000 everywhere (scipy's result is undefined there).  Extents <= 18000.  Scratch:
 *                        sd_objseg_workspace_bytes(X, Y, Z, 0).
 *   sd_spinehead_window_mask  kd.load_seg(offset, size) + ndimage.zoom(seg, 1 / ds, order=0) + relabel_vol_nonexist2zero / (seg ==
 *                        sv_ids[0]) (:2135-2141; both branches give the same 0/1 mask).  seg_dev: a resident (VX,VY,VZ) uint64 volume
 *                        whose voxel 0 is vol_origin_xyz (HOST int64[3]); voxels outside it read 0.  win_offset_xyz HOST int64[3].
 *                        tab_*_dev int32[X] / [Y] / [Z]: the source index of every output sample along the axis, -1 = scipy's constant
 *                        0 (the order-0 zoom is separable; the host builds the tables by scipy's rule: n_out = round(n_in / ds),
 *                        coordinate c = i (n_in - 1) / (n_out - 1) in double, c > n_in - 1 -> -1, else floor(c + 0.5)).
 *                        cell_sv_dev: the cell's supervoxel ids, sorted ascending, n_sv >= 1 (binary search per voxel).
 *   sd_spinehead_fill_holes  ndimage.binary_fill_holes (:2143): a background voxel becomes foreground unless its 6-connected background
 *                        component owns a voxel of the window border (the inverted mask labelled by sd_object_segmentation's
 *                        components).  *n_filled_dev = foreground voxels of filled_dev (0: the reference raises ValueError, :2144).
 *   sd_spinehead_peaks   peak_local_max(distance, footprint=np.ones((3, 3, 3)), labels=seg) (:2162) restated from skimage 0.18 / 0.19;
 *                        skimage is absent from the reference tree and this image: parity-UNPINNED.  roi = bounding box of the mask
 *                        voxels that are not on the outermost voxel layer of the window (exclude_border with min_distance 1; none: no
 *                        peaks).  A mask voxel inside roi is a peak iff its d2 equals the largest d2 over the mask voxels of its 3x3x3
 *                        neighbourhood clipped to roi and d2 > 0; mask voxels outside roi are neither peaks nor seen.  If EVERY mask voxel
 *                        in roi equals its neighbourhood maximum (skimage's "trivial image", e.g. a sheet one voxel thick) there are no
 *                        peaks.  ensure_spacing with spacing 1 culls nothing: every voxel of a plateau is a peak.  peaks_dev int32
 *                        [max_peaks][3] in raster order (flag + scan); *n_peaks_dev = their number, which may exceed max_peaks (the
 *                        list is cut: the caller must treat that as an error).
 *   sd_spinehead_box_vertices  in_bounding_box(verts, [offset + size / 2, size]) (:2150-2153, extraction/in_bounding_boxC.pyx) for n_win
 *                        windows at once: vertex v (verts_dev [n_verts][3] in voxels, float64 or float32 widened exactly, labels_dev int32)
 *                        is in window w iff -e < v - (win_offset_dev[w] + size / 2) < e on every axis in float64, e = the half edge
 *                        rounded to C float.  stages bit 0: flags, scan, begin_dev uint64[n_win + 2] (begin[w] = vertices in windows < w;
 *                        entries n_win and n_win + 1 = the total: segment n_win is empty); bit 1: points_dev double[total][3] = v -
 *                        window offset (:2165) and point_labels_dev with label 0 rewritten to 9 (:2160), window by window in vertex
 *                        order -- the segmented point set sd_syn_props_knn takes.  Scratch sd_spinehead_box_vertices_temp_bytes (kept
 *                        between the two stages); n_verts, n_win >= 1, n_verts * n_win < 2^31.
 *   sd_spinehead_queries the queries of colorcode_vertices (:2165): q_slots <= max_peaks slots per window (the caller sizes them by the
 *                        largest peak count of its batch); for window w and slot p < min(n_peaks_dev[w], q_slots): q_cell = w, q_xyz =
 *                        peak * ds_xyz (HOST double[3]); other slots: q_cell = n_win (the empty segment: vote -1).  peaks_dev
 *                        [n_win][max_peaks][3], q_*_dev [n_win * q_slots].
 *   sd_spinehead_markers local_maxi (:2167-2168): markers_dev int32 = 0, then votes_dev[p] at peak p of one window (negative votes: 0).
 *   sd_spinehead_select  :2171-2196.  head = (flood_dev == 1); its 6-connected components numbered like ndimage.label (objects_dev,
 *                        optional int32 output); nb_obj <= 1: id 1; else the id with the most voxels in labels[c - 10 : c + 11] per axis
 *                        with numpy's slice rules (a negative start wraps, so c < 10 on an axis empties the slice; the stop clips),
 *                        the smallest id on equal counts; if the slice holds no labelled voxel the object owning the voxel nearest to c
 *                        in the reference's own float64 arithmetic (:2189-2191, cKDTree): per axis d = (v + offset) * scaling -
 *                        (c + offset) * scaling, both points scaled and then subtracted, d2 = ((dx dx) + dy dy) + dz dz with every
 *                        product and sum rounded, never fused; ties in d2: lowest id, then raster index (the project's rule: cKDTree's
 *                        pick among equal distances follows its tree order).  c_xyz HOST int64[3] = rep_coord - offset (mag-1 voxels
 *                        indexing the zoomed volume, as the reference does), win_offset_xyz HOST int64[3] = the window offset (it moves
 *                        the rounding of the scaled points, so it decides near-ties for non-integral voxel sizes; |v + offset| < 2^53),
 *                        scaling_xyz HOST double[3].  result_dev int32[3] = voxels of the chosen object (0 if nb_obj == 0), the chosen
 *                        id, nb_obj. */
#define SD_SPINEHEAD_VOX_GRID 8192
#define SD_SPINEHEAD_VERT_GRID 1024
#define SD_SPINEHEAD_ID_GRID 1024
size_t sd_spinehead_workspace_bytes(int X, int Y, int Z);
int sd_edt_squared(const uint8_t* mask_dev, int X, int Y, int Z, int32_t* d2_dev, void* workspace_dev, size_t ws_bytes, void* stream);
int sd_spinehead_window_mask(const uint64_t* seg_dev, int VX, int VY, int VZ, const int64_t* vol_origin_xyz, const int64_t* win_offset_xyz,
                             const int32_t* tab_x_dev, const int32_t* tab_y_dev, const int32_t* tab_z_dev, int X, int Y, int Z,
                             const uint64_t* cell_sv_dev, size_t n_sv, uint8_t* mask_dev, void* stream);
int sd_spinehead_fill_holes(const uint8_t* mask_dev, int X, int Y, int Z, uint8_t* filled_dev, int32_t* n_filled_dev, void* workspace_dev,
                            size_t ws_bytes, void* stream);
int sd_spinehead_peaks(const uint8_t* mask_dev, const int32_t* d2_dev, int X, int Y, int Z, int32_t* peaks_dev, size_t max_peaks,
                       int32_t* n_peaks_dev, void* workspace_dev, size_t ws_bytes, void* stream);
size_t sd_spinehead_box_vertices_temp_bytes(size_t n_verts, size_t n_win);
int sd_spinehead_box_vertices(const void* verts_dev, int verts_f32, const int32_t* labels_dev, size_t n_verts, const int64_t* win_offset_dev,
                              size_t n_win, const int32_t* win_size_xyz, int stages, uint64_t* begin_dev, double* points_dev,
                              int32_t* point_labels_dev, size_t max_points, void* temp_dev, size_t temp_bytes, void* stream);
int sd_spinehead_queries(const int32_t* peaks_dev, const int32_t* n_peaks_dev, size_t n_win, size_t max_peaks, size_t q_slots,
                         const double* ds_xyz, uint32_t* q_cell_dev, double* q_xyz_dev, void* stream);
int sd_spinehead_markers(const int32_t* peaks_dev, const int32_t* n_peaks_dev, const int32_t* votes_dev, size_t max_peaks, int X, int Y, int Z,
                         int32_t* markers_dev, void* stream);
int sd_spinehead_select(const int32_t* flood_dev, int X, int Y, int Z, const int64_t* c_xyz, const int64_t* win_offset_xyz, const double* scaling_xyz,
                        int32_t* objects_dev, int32_t* result_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* ---- majority votes along skeletons (csrc/sd_skeleton.hip) -------------------------------------------------------------
 * The array form of majorityvote_skeleton_property (/root/reference/syconn/reps/super_segmentation_helper.py:1270-1302, one
 * nx.single_source_dijkstra_path and one np.unique per skeleton node, over SuperSegmentationObject.weighted_graph, reps/
 * super_segmentation_object.py:1440-1451) and of majority_vote_compartments (:1233-1266), for all cells in one call.  Cell c owns the
 * table rows node_begin_dev[c] .. node_begin_dev[c + 1] and the edges edge_begin_dev[c] .. edge_begin_dev[c + 1] (uint64[n_cells + 1],
 * ascending from 0 to the total); edges_dev int64[n_edges][2] names nodes by their index INSIDE the cell.  classes_dev uint8[n_nodes]:
 * dense classes below n_classes <= SD_SKEL_MAX_CLASSES (the caller maps its labels with np.unique, so the smaller class is the smaller
 * label).  Limits (SD_ERR_INVALID beyond): n_cells < 2^31, n_nodes < 2^31 - 1, n_edges < 2^30.  Asynchronous on the stream.
 *   sd_skel_csr          the adjacency: adj_begin_dev uint64[n_nodes + 1], adj_nbr_dev uint32[2 n_edges] (the neighbour's index inside the
 *                        cell), adj_w_dev double[2 n_edges]; weight_dev double[n_edges] is computed by the caller (np.linalg.norm of
 *                        the scaled end points: the reference's own expression, its dtype promotion included).  Parallel edges and self
 *                        loops stay in the rows.  counts_dev uint64[8]; [7] != 0: an offset table is not ascending from 0 to the total,
 *                        an edge names a node outside its cell (it is left out of every row, nothing is read through it) or a weight
 *                        is negative or NaN (stored as +inf).  Scratch: sd_skel_csr_temp_bytes(n_edges).
 *   sd_skel_vote         vote_dev[g] uint8 = the most frequent class, on equal counts the smallest, among the nodes v of g's cell with
 *                        dist(g, v) <= max_dist, dist = the minimum over all paths of the left-to-right float64 sum of the weights (what
 *                        Dijkstra yields; g itself is always in).  Optional n_reached_dev uint32[n_nodes] = the size of that window.
 *                        One wave per source; a window of up to SD_SKEL_LDS_NODES nodes is held in LDS, a larger one is redone over
 *                        arrays in the scratch that are sized by max_cell_nodes (>= the nodes of every cell; [7] otherwise).
 *                        counts_dev uint64[8] = sources redone that way, relaxation steps of the first pass, of the second, ...; [7] !=
 *                        0: an offset or a cell size was out of range.  Scratch: sd_skel_vote_temp_bytes(n_nodes, max_cell_nodes): one
 *                        byte per node and 20 bytes per node of the largest cell for each wave of the second pass, which runs
 *                        SD_SKEL_REDO_GRID blocks, fewer where those arrays would pass SD_SKEL_REDO_BYTES.
 *   sd_skel_components   out_dev[g] uint8: nodes of class soma_class keep it; the others form connected components over the edges whose
 *                        two nodes are not soma (a node without such an edge is a component), and every node gets its component's
 *                        most frequent class, the smallest on equal counts; where that is one_class with a count c1 and 50 c1 < 33
 *                        total (the reference's float32 test `c1 / total < 0.66`, equal to it for total < 2^24) it gets zero_class.
 *                        soma_class / one_class may be -1 (no such class).  counts_dev uint64[8]; [6] != 0: such a component had 2^24
 *                        nodes or more; [7] != 0: an offset or an edge was out of range (the edge is ignored).
 *                        Scratch: sd_skel_components_temp_bytes(n_nodes).
 * One grid stride of the kernels is SD_SKEL_VOTE_GRID blocks of four sources, SD_SKEL_NODE_GRID blocks of 256 nodes (or cells),
 * SD_SKEL_EDGE_GRID blocks of 256 half edges (or edges). */
#define SD_SKEL_MAX_CLASSES 64
#define SD_SKEL_LDS_NODES 512
#define SD_SKEL_VOTE_GRID 2048
#define SD_SKEL_NODE_GRID 1024
#define SD_SKEL_EDGE_GRID 1024
#define SD_SKEL_REDO_GRID 1024
#define SD_SKEL_REDO_BYTES 268435456
size_t sd_skel_csr_temp_bytes(size_t n_edges);
int sd_skel_csr(const int64_t* edges_dev, const uint64_t* edge_begin_dev, const uint64_t* node_begin_dev, size_t n_cells, size_t n_nodes,
                size_t n_edges, const double* weight_dev, uint64_t* adj_begin_dev, uint32_t* adj_nbr_dev, double* adj_w_dev, uint64_t* counts_dev,
                void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_skel_vote_temp_bytes(size_t n_nodes, size_t max_cell_nodes);
int sd_skel_vote(const uint64_t* adj_begin_dev, const uint32_t* adj_nbr_dev, const double* adj_w_dev, size_t n_adj, const uint64_t* node_begin_dev,
                 size_t n_cells, size_t n_nodes, size_t max_cell_nodes, const uint8_t* classes_dev, int n_classes, double max_dist,
                 uint8_t* vote_dev, uint32_t* n_reached_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_skel_components_temp_bytes(size_t n_nodes);
int sd_skel_components(const int64_t* edges_dev, const uint64_t* edge_begin_dev, const uint64_t* node_begin_dev, size_t n_cells, size_t n_nodes,
                       size_t n_edges, const uint8_t* classes_dev, int soma_class, int one_class, int zero_class, uint8_t* out_dev,
                       uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);

/* ---- cells from the supervoxel graph, organelles to cells (csrc/sd_cell_assembly.hip) -----------------------------------
 * The array form of /root/reference/syconn/exec/exec_init.py run_create_rag (:299-367) and the apply_ssv_size_threshold branch of
 * run_create_neuron_ssd (:61-80) with proc/graphs.py create_ccsize_dict (:220-249); of the cell properties of reps/
 * super_segmentation_object.py (:713-727, :1148-1168); of proc/sd_proc.py:1063-1084 with proc/ssd_proc.py
 * _aggregate_segmentation_object_mappings_thread (:55-91) and _apply_mapping_decisions_thread (:126-238); and of
 * map_synssv_objects_thread (:315-342).  Ids use all 64 bits, 0 is "no object".  A supervoxel table is ids_dev uint64[n_ids] strictly
 * ascending, sizes_dev int64[n_ids] (voxels), rep_coords_dev int32[n_ids][3], box_begin_dev uint64[n_ids + 1] (ascending from 0 to
 * n_boxes) into boxes_dev int32[n_boxes][6] (min | max, one box per chunk that holds the id).  Cells are a CSR table: sv_begin_dev
 * uint64[n_cells + 1] into sv_ids_dev uint64[n_sv].  counts_dev uint64[8] is zeroed by every call; counts[7] != 0: an offset table does
 * not ascend from 0 to its total or an id table does not ascend strictly (nothing is read out of range through either).  Every count
 * per call stays below 2^31 (SD_ERR_INVALID beyond).  Asynchronous on the stream; no float atomics anywhere.
 *   sd_svgraph_components  edges_dev uint64[n_edges][2] (self loops, duplicates and endpoints 0 are legal).  Nodes = the table ids and
 *                        every endpoint, without 0 (:319-320, with its edges); a table id without an edge is a component of its own
 *                        (:327-330).  node_ids_dev uint64[n_ids + 2 n_edges] = the nodes ascending, counts[0] of them; node_comp_dev =
 *                        per node the smallest id of its component (the reference's cc_dict key, :80), or 0 where the component is
 *                        dropped; node_size_dev double = per node the size of its component, create_ccsize_dict's value:
 *                        sqrt(((dx dx) + dy dy) + dz dz) over d = max * scaling - min * scaling of ALL corners of all boxes of the
 *                        component's table supervoxels (an endpoint outside the table joins the component and has no box), every
 *                        product and sum rounded on its own, the root correctly rounded.  A component without any box: counts[6] = 1,
 *                        counts[5] = one of its ids (the reference raises ValueError, graphs.py:241-242).  Dropped: size <=
 *                        min_cc_size (strict != 0, :349) or size < min_cc_size (strict == 0, :75).  The kept cells as CSR:
 *                        ssv_ids_dev ascending (counts[1] cells), sv_begin_dev, sv_ids_dev ascending inside a cell (counts[2]); arrays
 *                        of n_ids + 2 n_edges (+ 1) entries.  edges_out_dev uint64[n_edges][2] = the edges whose component is kept, in
 *                        input order (counts[3]; the pruned graph, :359).  counts[4] = the voxels of the kept table supervoxels
 *                        (total_size, :352-354).  scaling_xyz HOST double[3] > 0.  Scratch: sd_svgraph_components_temp_bytes.
 *   sd_cell_props        per cell of a CSR table (any order inside a cell): cell_size_dev int64 = the sum of its supervoxels' sizes
 *                        (:1152), cell_box_dev int32[6] = min of the lower, max of the upper corners (:1166-1167), cell_rep_dev
 *                        int32[3] = the representative coordinate of its FIRST supervoxel (:725).  counts[0] = supervoxels that are not
 *                        in the table (counts[5] = one of them): they contribute nothing; a cell without a known supervoxel has size
 *                        0 and the zero box (:1158-1161).
 *   sd_cell_mapping      records (rec_sub_dev organelle id, rec_sv_dev supervoxel id, rec_count_dev int64 voxels) of ONE organelle
 *                        kind, in any order; org_ids_dev / org_sizes_dev its table.  A record is dropped when its organelle is not in
 *                        the table (sd_proc.py:1075-1077), its supervoxel is 0 or in no cell, or its count is <= 0 (a Counter keeps no
 *                        such entry).  ratio = count / size in float64 (:1081); per (cell, organelle) the ratios are added ONE AFTER
 *                        ANOTHER in the order of the cell's supervoxel list, starting from 0.0 (Counter.__iadd__, ssd_proc.py:83).
 *                        Pairs ascend by (cell row, organelle id): cell_begin_dev uint64[n_cells + 1] into pair_org_dev /
 *                        pair_ratio_dev / pair_accepted_dev (n_records entries each, counts[1] used).  Accepted (:222-231): ratio >
 *                        lower_ratio, and ratio <= upper_ratio unless upper_ratio >= 1, and (double) size > size_threshold.
 *                        acc_begin_dev uint64[n_cells + 1] into acc_org_dev (counts[2]): the accepted organelles per cell.
 *                        org_n_cells_dev uint32[n_org] = accepting cells, org_first_cell_dev uint32[n_org] = the smallest row among
 *                        them (0xffffffff: none).  counts[0] = records kept.  counts[6] != 0: a supervoxel appears twice in the cell
 *                        lists, or 0 does.  Scratch: sd_cell_mapping_temp_bytes(n_records, n_sv).
 *   sd_cell_synapses     partners_dev uint64[n_syn][2], keep_dev uint8[n_syn] (the caller's `syn_prob > thresh`, :329-330),
 *                        ssv_ids_dev uint64[n_cells] strictly ascending.  syn_begin_dev uint64[n_cells + 1] into out_ids_dev
 *                        uint64[2 n_syn] (counts[0] used): per cell the kept syn_ids_dev with the cell in slot 0, in row order, then
 *                        those with it in slot 1 (:338-340).  Scratch: sd_cell_synapses_temp_bytes(n_syn).
 * One grid stride of every kernel is SD_CELLASM_GRID blocks of 256 items. */
#define SD_CELLASM_GRID 1024
size_t sd_svgraph_components_temp_bytes(size_t n_ids, size_t n_edges);
int sd_svgraph_components(const uint64_t* edges_dev, size_t n_edges, const uint64_t* ids_dev, const int64_t* sizes_dev, const uint64_t* box_begin_dev,
                          const int32_t* boxes_dev, size_t n_ids, size_t n_boxes, const double* scaling_xyz, double min_cc_size, int strict,
                          uint64_t* node_ids_dev, uint64_t* node_comp_dev, double* node_size_dev, uint64_t* ssv_ids_dev, uint64_t* sv_begin_dev,
                          uint64_t* sv_ids_dev, uint64_t* edges_out_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_cell_props(const uint64_t* sv_begin_dev, const uint64_t* sv_ids_dev, size_t n_cells, size_t n_sv, const uint64_t* ids_dev, const int64_t* sizes_dev,
                  const int32_t* rep_coords_dev, const uint64_t* box_begin_dev, const int32_t* boxes_dev, size_t n_ids, size_t n_boxes,
                  int64_t* cell_size_dev, int32_t* cell_box_dev, int32_t* cell_rep_dev, uint64_t* counts_dev, void* stream);
size_t sd_cell_mapping_temp_bytes(size_t n_records, size_t n_sv);
int sd_cell_mapping(const uint64_t* rec_sub_dev, const uint64_t* rec_sv_dev, const int64_t* rec_count_dev, size_t n_records, const uint64_t* org_ids_dev,
                    const int64_t* org_sizes_dev, size_t n_org, const uint64_t* sv_begin_dev, const uint64_t* sv_ids_dev, size_t n_cells, size_t n_sv,
                    double lower_ratio, double upper_ratio, double size_threshold, uint64_t* cell_begin_dev, uint64_t* pair_org_dev,
                    double* pair_ratio_dev, uint8_t* pair_accepted_dev, uint64_t* acc_begin_dev, uint64_t* acc_org_dev, uint32_t* org_n_cells_dev,
                    uint32_t* org_first_cell_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_cell_synapses_temp_bytes(size_t n_syn);
int sd_cell_synapses(const uint64_t* partners_dev, const uint8_t* keep_dev, const uint64_t* syn_ids_dev, size_t n_syn, const uint64_t* ssv_ids_dev,
                     size_t n_cells, uint64_t* syn_begin_dev, uint64_t* out_ids_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);

/* ---- astrocyte splitting of the supervoxel graph (csrc/sd_glia.hip) --------------------------------------------------------
 * The array form, for all cells of a dataset at once, of /root/reference/syconn/proc/graphs.py remove_glia_nodes (:278-360) with
 * create_ccsize_dict (:220-249), of proc/glia_splitting.py collect_glia_sv (:37-63) and write_astrocyte_svgraph (:77-161), and of
 * reps/segmentation_helper.py glia_pred_so / glia_proba_so (:32-78) with reps/segmentation.py glia_pred (:799-814).  Ids use all 64 bits
 * and none is special.  Asynchronous on the stream; no float atomics; every count per call stays below 2^31 (SD_ERR_INVALID beyond).
 *   sd_glia_split  edges_dev uint64[n_edges][2] (self loops and duplicates are legal: a single-supervoxel cell is a self loop),
 *                  nodes_dev uint64[n_nodes] (optional: nodes without an edge; repeats of endpoints are legal).  The supervoxel table:
 *                  ids_dev uint64[n_ids] strictly ascending, boxes_dev double[n_ids][2][3] in nm (finite; the supervoxel's mesh_bb),
 *                  glia_dev uint8[n_ids] (0 neuron, else glia).  Nodes = the distinct endpoints and extra nodes, ascending; a cell = a
 *                  component of the graph.  size(component) = sqrt(((dx dx) + dy dy) + dz dz) of d = max - min over BOTH corners of
 *                  the boxes of its nodes, every product and sum rounded on its own, the root correctly rounded.  Per cell, with T =
 *                  min_size: (1) no component of its neuron nodes has size > T: all of it is glia; (2) else no component of its glia
 *                  nodes has size > T: all of it is neuron; (3) else glia nodes whose glia component has size < T are tiny fragments,
 *                  nodes whose component among neuron nodes and tiny fragments has size < T leave, what stays is neuron and the rest
 *                  glia.  Per node (node_cap entries each; counts[0] nodes): node_ids_dev, node_cell_dev (the smallest id of its
 *                  cell), node_class_dev uint8 (final: 0 neuron, 1 glia), node_comp_dev (the smallest id of its component among the
 *                  nodes of its final class), node_size1_dev (the size of its same-class component of steps 1 / 2), node_size2_dev
 *                  (its size in step 3's neuron-or-tiny components, NaN where it took no part).  Per cell, ascending (node_cap
 *                  entries; counts[1] cells): cell_ids_dev, cell_outcome_dev uint8 = 1, 2 or 3, the step that decided.  Two component
 *                  tables in CSR form, neuron (ncc_, counts[2] components, counts[3] supervoxels) and glia (gcc_, counts[4],
 *                  counts[5]): *_ids_dev ascending (node_cap entries), *_cell_dev, *_begin_dev uint64[node_cap + 1], *_sv_dev
 *                  ascending inside a component (node_cap entries); for outcomes 1 and 2 the one component is the whole cell.
 *                  neuron_edges_dev / astrocyte_edges_dev uint64[edge_cap][2] (counts[6] / counts[8]): the input edges with both
 *                  endpoints neuron / glia, in input order, self loops included; a neuron node all of whose neighbours became glia
 *                  is in the component table and, without a self loop, in no edge (the reference's lists and edge-list file differ
 *                  in the same way).  cell_size_dev double[n_ids] (optional): a node with cell_size < min_cell_size (the size of its
 *                  ORIGINAL cell, the caller's) is left out of both edge arrays, both component tables and counts[9] (:125-127,
 *                  :147-149); its per-node outputs stay.  sv_sizes_dev int64[n_ids] (optional): counts[9] = the voxels of the glia
 *                  nodes (total_size, :152-154).  counts_dev uint64[16], zeroed by every call: [7] != 0 ids_dev does not ascend
 *                  strictly; [10] != 0 a node is not in the table (the reference raises KeyError) and [11] = the smallest such id
 *                  (the outputs are then unusable); [12] != 0 node_cap or edge_cap was smaller than needed and records were lost
 *                  (nothing is written past a capacity); [13], [14], [15] = cells of outcome 1, 2, 3.  node_cap = the distinct
 *                  nodes (2 n_edges + n_nodes always suffices), edge_cap = n_edges always suffices.
 *                  Scratch: sd_glia_split_temp_bytes(n_ids, n_edges, n_nodes).
 *   sd_glia_pred   probas_dev float32 (is_f64 == 0) or float64 [n_views]: column 1 of every supervoxel's glia_probas, one after
 *                  another; view_begin_dev uint64[n_sv + 1] ascending from 0 to n_views.  mean_dev double[n_sv] = the float64 sum in
 *                  view order divided once by the number of views (NaN without views; numpy sums pairwise in the input dtype: equal
 *                  whenever the sum is exact).  class_dev uint8[n_sv]: point_model == 0: mean > thresh and votes > (long long)
 *                  ((double) views * 0.7) with votes = #(p > thresh); point_model != 0: mean >= thresh; no views: 0.
 *                  counts_dev uint64[8]: [7] != 0 the offsets do not ascend from 0 to n_views.
 * One grid stride of every kernel is SD_GLIA_GRID blocks of 256 items. */
#define SD_GLIA_GRID 1024
size_t sd_glia_split_temp_bytes(size_t n_ids, size_t n_edges, size_t n_nodes);
int sd_glia_split(const uint64_t* edges_dev, size_t n_edges, const uint64_t* nodes_dev, size_t n_nodes, const uint64_t* ids_dev, const double* boxes_dev,
                  const uint8_t* glia_dev, size_t n_ids, double min_size, const double* cell_size_dev, double min_cell_size, const int64_t* sv_sizes_dev,
                  size_t node_cap, size_t edge_cap, uint64_t* node_ids_dev, uint64_t* node_cell_dev, uint8_t* node_class_dev, uint64_t* node_comp_dev,
                  double* node_size1_dev, double* node_size2_dev, uint64_t* cell_ids_dev, uint8_t* cell_outcome_dev, uint64_t* ncc_ids_dev,
                  uint64_t* ncc_cell_dev, uint64_t* ncc_begin_dev, uint64_t* ncc_sv_dev, uint64_t* gcc_ids_dev, uint64_t* gcc_cell_dev,
                  uint64_t* gcc_begin_dev, uint64_t* gcc_sv_dev, uint64_t* neuron_edges_dev, uint64_t* astrocyte_edges_dev, uint64_t* counts_dev,
                  void* temp_dev, size_t temp_bytes, void* stream);
int sd_glia_pred(const void* probas_dev, int is_f64, const uint64_t* view_begin_dev, size_t n_sv, size_t n_views, double thresh, int point_model,
                 uint8_t* class_dev, double* mean_dev, uint64_t* counts_dev, void* stream);

/* ---- multi-view depth and index images of a mesh, view rotations, pixel -> vertex vote (csrc/sd_views.hip) ----------------------
 * The compute form of what the reference renders with OpenGL: proc/rendering_egl.py _render_mesh_coords (:611-681),
 * multi_view_mesh_coords (:460-590), screen_shot (:130-174); proc/meshes.py MeshObject (:69-175), calc_rot_matrices (:236-329),
 * flag_empty_spaces (:332-360) with extraction/in_bounding_boxC.pyx; proc/rendering.py render_sso_coords_index_views (:300-396);
 * reps/super_segmentation_helper.py semseg2mesh_counter (:1527-1551) and the decision of semseg2mesh (:1603-1615).  The raster rule is
 * this build's own and is stated in DESIGN.md section 7 (tests/_views_ref.py says the same in numpy).  Asynchronous on the stream; no
 * float atomics; every count per call stays below 2^31 (SD_ERR_INVALID beyond).  counts_dev uint64[8], zeroed by every call.
 * Common arguments: verts_dev float32[n_verts][3] and coords_dev float32[n_loc][3] are RAW; center3 (host, 3 floats) and max_dist > 0
 * normalise both wherever they are read: vn = fl32(fl32(v - center) / max_dist) (center 0 and max_dist 1 leave them as they are).
 * tris_dev uint32[n_tris][3].  edge3 (host, 3 doubles) = [cw, cw / 2, cw] / max_dist.
 *   sd_views_rotations    rot_dev double[n_loc][16]: per location the PCA of the normalised vertices 0, stride, 2 stride, ... that lie
 *                         inside the box of edge_length (normalised units) around it by in_bounding_box's float32 test (strict on both
 *                         sides, half edge = fl32(edge_length / 2)): mean and covariance (divisor n - 1) in float64, rows = eigenvectors
 *                         by descending eigenvalue, rot[i + 4 j] = row i, component j; rot[15] = 1; <= 2 inliers: 16 zeros.  The
 *                         component of largest magnitude of every row is positive (lowest index on a tie).  empty_dev uint8[n_loc]
 *                         (optional): 1 where no vertex is inside.  sd_views_flag_empty: only that.  Scratch:
 *                         sd_views_rotations_temp_bytes(n_verts, stride).
 *   sd_views_index        index_dev (sd_views_index_bytes(n_tris) bytes, opaque): a uniform grid over the normalised triangles keyed by
 *                         centroid cell, the largest distance of a vertex to its triangle's centroid, and whether any normalised vertex
 *                         is not 0.  counts[3] != 0: a triangle names a vertex >= n_verts (it is in no cell).  Scratch:
 *                         sd_views_index_temp_bytes(n_tris).
 *   sd_views_candidates   cand_begin_dev uint64[n_loc + 1], cand_dev uint32[cand_cap]: per location the triangles of the grid cells that
 *                         meet the sphere of radius 0.5 |edge3| + that distance around it, a superset of what any view of the location
 *                         shows.  counts[0] = their number; with cand_cap == 0 nothing is emitted (the sizing call); counts[1] != 0:
 *                         cand_cap was too small, nothing is written past it; counts[6] != 0: 2^31 candidates or more (split the
 *                         locations).  Scratch: sd_views_candidates_temp_bytes(n_loc).
 *   sd_views_render       views_dev uint8[n_loc][n_views][H][W] (views_cap elements): view m of a location is its matrix rot_dev[loc]
 *                         followed by the rotation about x with cos_v[m], sin_v[m] (host, n_views <= SD_VIEWS_MAX_VIEWS doubles each);
 *                         weights7 (host) the 7 filter weights.  255 where nothing is drawn, for a location whose matrix is all zero
 *                         and for a mesh whose normalised vertices are all zero.  counts[2] = triangles dropped because a snapped
 *                         coordinate reached 2^22 (per location and view), counts[3] != 0: a bad triangle or vertex number.  A window
 *                         of at most SD_VIEWS_TILE_PX pixels is one LDS tile; larger ones are cut into tiles of 250 x 122 (+ 3 halo).
 *   sd_views_render_index views_dev uint32[n_loc][n_views][H][W]: the last vertex of the nearest triangle (lowest triangle number at equal
 *                         depth), 2^32 - 2 where nothing is drawn.  One tile holds SD_VIEWS_TILE_PX / 2 pixels, larger windows are cut
 *                         into tiles of 128 x 128.  Scratch of both: sd_views_render_temp_bytes(n_loc, n_views).
 *   sd_views_vote         index_dev uint32[n_px], labels_dev uint8[n_px]: vertex_labels_dev uint8[n_verts] = the first label of the
 *                         largest count among the pixels of the vertex, counts taken modulo 256; `unpredicted` where they sum to 0.
 *                         Pixels equal to background_id are skipped.  table_dev uint8[n_verts][n_labels] (optional): the wrapped counts.
 *                         counts[0] = predicted vertices, counts[3] != 0: a pixel names a vertex >= n_verts, counts[4] != 0: a label
 *                         >= n_labels (both are skipped).  Scratch: sd_views_vote_temp_bytes(n_verts, n_labels).
 * One grid stride of the 1D kernels is SD_VIEWS_GRID blocks of 256 threads, of the raster SD_VIEWS_RASTER_GRID workgroups. */
#define SD_VIEWS_GRID 1024
#define SD_VIEWS_RASTER_GRID 4096
#define SD_VIEWS_MAX_VIEWS 16
#define SD_VIEWS_TILE_PX 32768
size_t sd_views_rotations_temp_bytes(size_t n_verts, size_t stride);
int sd_views_rotations(const float* verts_dev, size_t n_verts, size_t stride, const float* coords_dev, size_t n_loc, const float* center3, float max_dist,
                       float edge_length, double* rot_dev, uint8_t* empty_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_views_flag_empty(const float* verts_dev, size_t n_verts, size_t stride, const float* coords_dev, size_t n_loc, const float* center3, float max_dist,
                        float edge_length, uint8_t* empty_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_views_index_bytes(size_t n_tris);
size_t sd_views_index_temp_bytes(size_t n_tris);
int sd_views_index(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const float* center3, float max_dist, void* index_dev,
                   size_t index_bytes, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_views_candidates_temp_bytes(size_t n_loc);
int sd_views_candidates(const void* index_dev, size_t n_tris, const float* coords_dev, size_t n_loc, const float* center3, float max_dist, const double* edge3,
                        uint64_t* cand_begin_dev, uint32_t* cand_dev, size_t cand_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_views_render_temp_bytes(size_t n_loc, int n_views);
int sd_views_render(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const void* index_dev, const float* coords_dev,
                    size_t n_loc, const double* rot_dev, const float* center3, float max_dist, const double* edge3, const double* cos_v, const double* sin_v,
                    int n_views, int W, int H, const double* weights7, const uint64_t* cand_begin_dev, const uint32_t* cand_dev, size_t cand_n,
                    uint8_t* views_dev, size_t views_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_views_render_index(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const void* index_dev, const float* coords_dev,
                          size_t n_loc, const double* rot_dev, const float* center3, float max_dist, const double* edge3, const double* cos_v,
                          const double* sin_v, int n_views, int W, int H, const uint64_t* cand_begin_dev, const uint32_t* cand_dev, size_t cand_n,
                          uint32_t* views_dev, size_t views_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_views_vote_temp_bytes(size_t n_verts, int n_labels);
int sd_views_vote(const uint32_t* index_dev, const uint8_t* labels_dev, size_t n_px, uint32_t background_id, size_t n_verts, int n_labels, int unpredicted,
                  uint8_t* vertex_labels_dev, uint8_t* table_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);

/* ---- surface meshes of labelled objects (csrc/sd_mesh.hip) -----------------------------------------------------------------
 * The meshing of the reference's find_meshes (proc/meshes.py:937-994) for ALL non-zero labels of a chunk in one pass, and the merge of
 * per-chunk meshes with the mesh_bb / mesh_area of proc/sd_proc.py:951-975 (merge_meshes_incl_norm, proc/meshes.py:483-519).  The
 * surface is the UNSIMPLIFIED marching-cubes surface of every "label == id" volume over the triangle table of csrc/sd_mc_table.h
 * (tools/gen_mc_table.py states the rule it is derived from); no normals.
 * Input: labels_dev uint64 [X][Y][Z] and three int32 source-index tables tx_dev[NX], ty_dev[NY], tz_dev[NZ] that combine the
 * reference's zoom (order 0) and edge pad: padded[i, j, k] = labels[tx[i], ty[j], tz[k]], an entry -1 reads as label 0 (scipy's
 * constant).  No zoomed or padded copy is made.  ids_dev uint64[n_ids] strictly ascending, without 0: the objects, in output order (the
 * caller has them from the label statistics; a label of the volume that is not listed has no mesh and raises counts[6]).
 * Output, a CSR by object: vert_begin_dev / tri_begin_dev uint64[n_ids + 1]; verts_dev float32[vert_cap][3] in nm; tris_dev
 * uint32[tri_cap][3], indices local to the object; mesh_bb_dev float32[n_ids][2][3] (min | max of the vertices, zeros without any);
 * area_dev double[n_ids] in um^2 = (sum over triangles of |cross(v0 - v1, v0 - v2)|) / 2 / 1e6 in float64 over the float32 vertices.
 * Order (part of the contract): one vertex per grid edge of the padded array whose two voxels differ in membership, ascending by the
 * key ((x NY + y) NZ + z) * 3 + axis of the edge's lower voxel; triangles ascending by cube (x, y, z) in C order, then in table order,
 * their three indices in the table's order.  Coordinates: v = float32(max(0, g * scale + offset)) per axis in float64, every product and
 * sum rounded on its own, g the half-integer grid position in the padded array (voxel i at coordinate i); scale_xyz / offset_xyz
 * HOST double[3] = scaling * ds and offset_vox * scaling - pad * scaling * ds.
 * counts_dev uint64[8], zeroed by every call: [0] vertices, [1] triangles of the volume (sd_mesh_count: what sd_mesh_build needs as
 * capacities), [2] != 0: a capacity was smaller and records were lost (nothing is written past a capacity; the outputs are then
 * unusable), [5] != 0: a triangle without its vertex (only after [2]), [6] != 0: a label outside ids_dev, [7] != 0: a table entry
 * outside [-1, extent) or ids not strictly ascending.  The padded volume holds at most 2^31 voxels and every count per call stays
 * below 2^31 (SD_ERR_INVALID beyond).  Asynchronous on the stream; no float atomics; integer atomics only count.
 *   sd_mesh_merge   pieces = the objects of several such tables, concatenated in the order of the tables: piece_ids_dev uint64[n_pieces]
 *                   (any order, repeats = one object in several chunks), piece_vert_begin_dev / piece_tri_begin_dev uint64[n_pieces + 1]
 *                   into verts_dev / tris_dev.  One stable sort by id, one scan, one gather: obj_ids_dev uint64[n_pieces] ascending
 *                   (counts[0] objects), vert_begin_dev / tri_begin_dev [n_pieces + 1], the pieces of an object one after another in
 *                   input order with their indices shifted (seam vertices stay twice, as in the reference), mesh_bb_dev / area_dev
 *                   [n_pieces] recomputed.  counts[7] != 0: an offset table does not ascend from 0 to its total.
 * One grid stride of every kernel is SD_MESH_GRID blocks of 256 threads (voxel kernels: 256 voxels per block and step; per-object
 * kernel: 4 objects per block and step). */
#define SD_MESH_GRID 256
int sd_mesh_count(const uint64_t* labels_dev, int X, int Y, int Z, const int32_t* tx_dev, const int32_t* ty_dev, const int32_t* tz_dev, int NX, int NY,
                  int NZ, const uint64_t* ids_dev, size_t n_ids, uint64_t* counts_dev, void* stream);
size_t sd_mesh_build_temp_bytes(int NX, int NY, int NZ, size_t vert_cap, size_t tri_cap);
int sd_mesh_build(const uint64_t* labels_dev, int X, int Y, int Z, const int32_t* tx_dev, const int32_t* ty_dev, const int32_t* tz_dev, int NX, int NY,
                  int NZ, const uint64_t* ids_dev, size_t n_ids, const double* scale_xyz, const double* offset_xyz, size_t vert_cap, size_t tri_cap,
                  uint64_t* vert_begin_dev, uint64_t* tri_begin_dev, float* verts_dev, uint32_t* tris_dev, float* mesh_bb_dev, double* area_dev,
                  uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_mesh_merge_temp_bytes(size_t n_pieces);
int sd_mesh_merge(const uint64_t* piece_ids_dev, const uint64_t* piece_vert_begin_dev, const uint64_t* piece_tri_begin_dev, size_t n_pieces,
                  const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, uint64_t* obj_ids_dev, uint64_t* vert_begin_dev,
                  uint64_t* tri_begin_dev, float* verts_out_dev, uint32_t* tris_out_dev, float* mesh_bb_dev, double* area_dev, uint64_t* counts_dev,
                  void* temp_dev, size_t temp_bytes, void* stream);

/* ---- rendering locations of all objects of a vertex table (csrc/sd_locations.hip) ------------------------------------------------
 * What the reference computes per supervoxel in SegmentationObject.sample_locations (reps/segmentation.py:700-732; the batch job
 * batchjob_sample_location_caching.py, SuperSegmentationObject.sample_locations on top of it), for ALL objects of a table in one call.
 * Object s owns verts_dev[vert_begin_dev[s] : vert_begin_dev[s + 1]] (uint64[n_obj + 1] ascending from 0 to n_verts, the layout of
 * sd_mesh_build's vert_begin_dev).  Output, a CSR by object: loc_begin_dev uint64[n_obj + 1], loc_dev [loc_cap][3].  An object without
 * vertices has no location.  With loc_cap == 0 nothing is emitted (the sizing call: counts[0] is the capacity the emitting call needs).
 *   sd_locations_voxel    generate_rendering_locs (handler/multiviews.py:339-355), open3d's voxel_down_sample as open3d publishes it:
 *                         verts_dev float32 (verts_f32 != 0) or float64 [n_verts][3]; per object in float64 vmin = min - 0.5 ds, voxel
 *                         floor((p - vmin) / ds) per axis, a location = the sum of the voxel's vertices in ascending vertex order
 *                         divided by their number; loc_dev double, ascending by voxel (ix, iy, iz), x most significant (open3d: the
 *                         order of a hash map).
 *   sd_locations_surface  surface_samples (reps/rep_helper.py:376-417): verts_dev float32; bin_sizes3 (host, 3 floats), r the ball's
 *                         radius; max_nb_samples has no effect in the reference and is no argument.  histogramdd's float32 edges,
 *                         the centre (b + 0.5) bin_size of every occupied bin in C order, the nearest vertex in float64 (lowest index on
 *                         a tie), the ball ((dx dx) + dy dy) + dz dz <= r r around it, the float32 sum of its members in ascending
 *                         vertex order, one float32 division, + the object's minimum; loc_dev float.  csrc/sd_locations.hip states the
 *                         rule in full, tests/_locations_ref.py in numpy.
 * An object may span at most SD_LOCATIONS_MAX_CELLS voxels / bins per axis (3 x 21 key bits).  counts_dev uint64[8], zeroed by every
 * call: [0] locations, [1] != 0: loc_cap was smaller, nothing is written past it, [2] / [3] tiles visited / skipped by the surface
 * rule, [4] != 0: an object beyond SD_LOCATIONS_MAX_CELLS, [5] != 0: a vertex is NaN or infinite, [7] != 0: the offsets do not ascend
 * from 0 to n_verts (after [4], [5] or [7] the outputs are unusable; nothing is written outside them).  Every count per call stays
 * below 2^31 (SD_ERR_INVALID beyond).  Asynchronous on the stream; no float atomics.  One grid stride of the 1D kernels is
 * SD_LOCATIONS_GRID blocks of 256 threads, of the kernels with one wave per object or location SD_LOCATIONS_WAVE_GRID blocks of 4
 * waves; neither constant rests on a measurement. */
#define SD_LOCATIONS_GRID 1024
#define SD_LOCATIONS_WAVE_GRID 4096
#define SD_LOCATIONS_MAX_CELLS 2097152
size_t sd_locations_voxel_temp_bytes(size_t n_verts, size_t n_obj);
int sd_locations_voxel(const void* verts_dev, int verts_f32, const uint64_t* vert_begin_dev, size_t n_obj, size_t n_verts, double ds,
                       uint64_t* loc_begin_dev, double* loc_dev, size_t loc_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
size_t sd_locations_surface_temp_bytes(size_t n_verts, size_t n_obj);
int sd_locations_surface(const float* verts_dev, const uint64_t* vert_begin_dev, size_t n_obj, size_t n_verts, const float* bin_sizes3, double r,
                         uint64_t* loc_begin_dev, float* loc_dev, size_t loc_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);

/* ---- host-side helpers of the chunk pipeline (no GPU) -----------------------------------------------------------------
 * Multi-threaded strided copy of an (nz, ny, nx)-byte box between two uint8 host arrays whose x-rows are contiguous
 * (strides in bytes), and a multi-threaded memset: what numpy slicing does on one core when the reference cuts a chunk
 * (+ halo) out of a volume and crops the result (/root/reference/syconn/handler/prediction.py:806-812). */
int sd_host_box_copy(const uint8_t* src, int64_t src_stride_z, int64_t src_stride_y, uint8_t* dst, int64_t dst_stride_z,
                     int64_t dst_stride_y, int64_t nz, int64_t ny, int64_t nx, int n_threads);
int sd_host_zero(uint8_t* dst, int64_t nbytes, int n_threads);

/* Window clipping for model tiles of which only a part is wanted (host arithmetic on the plan, no GPU).  The reference's
 * chunk grid overhangs the dataset (fit_box_size=True, /root/reference/syconn/handler/prediction.py:679-683), every chunk is
 * predicted with a halo ring that is cropped afterwards (:812), and tiled_apply (elektronn3, row P3) runs every tile on its
 * full window.  Along `axis` (0 = z, 1 = y, 2 = x) the outputs lo <= index < hi of a window of `full` voxels depend on a cone of
 * the input only; this returns the sub-window [*start, *start + *extent) on which those outputs have the SAME values as on the
 * whole window: the far border of every layer ('same' padding, partial ceil-mode pooling windows, the up-convolution crop)
 * stays outside every cone (backward pass: conv k reads k/2 further, pooling f reads f times as far, a transposed conv f
 * ceil(/ f)), and the near border moves only by multiples of the network's total pooling stride along the axis, never past
 * the lowest index a wanted output reads in any buffer.  *extent is a multiple of `multiple` (or what is left of `full`), *start a
 * multiple of lcm(stride, multiple).  Plans with SD_OP_GROUPNORM (statistics over the whole window) return (0, full). */
int sd_plan_clip_window(const sd_op_desc* ops, int n_ops, int axis, int lo, int hi, int full, int multiple, int* start,
                        int* extent);

/* ---- the multi-view network of the cell type step (csrc/sd_viewnet.hip; host-only plan: csrc/sd_viewnet.h) -----------------
 * Replaces the network behind /root/reference/syconn/handler/prediction.py:985-1000 (get_celltype_model_e3 -> InferenceModel
 * .predict_proba) for the architecture of /root/reference/syconn/cnn/cnn_celltype_cmn_j0251.py:22-60
 * (StackedConv2ScalarWithLatentAdd): planar layers "valid k x k convolution, (1, p, p) floor max-pool, activation" and a chain
 * of Linear layers over [flattened features, scalars].  elektronn3's Conv3DLayer is not part of the reference tree; DESIGN.md says
 * what of it is pinned by the tree's text and what is a stated assumption.
 *   sd_viewnet_create     layers[n_layers] = (cout, k, pool) with k in {1, 2, 4, 5}, pool in {1, 2}, cout <= 80; in_channels 1..4;
 *                         fc[n_fc + 1] = (inputs of the first Linear = flattened features + n_scalar, outputs of every Linear),
 *                         1 <= n_fc <= 4; act 0 = ReLU, 1 = LeakyReLU(0.01); weights = float32 in registration order: per layer
 *                         w[cout][cin][k][k] then b[cout], per Linear w[out][in] then b[out]; act_dtype SD_F16 or SD_BF16 (storage of
 *                         activations and convolution weights; accumulation, bias and the whole head are fp32).
 *   sd_viewnet_forward    views_dev uint8[n_loc][in_channels][nb_views][H][W] as sd_views_render leaves them, n_planes_total =
 *                         n_loc * nb_views; sample_table_dev int32[n_samples][D]: plane loc * nb_views + view of every slot of every
 *                         sample (the input is never copied into sample order; the first layer computes conv(u / 255 - 0.5) from the
 *                         integers u with the normalisation in its fp32 epilogue); scalars_dev float[n_samples][n_scalar] (may be
 *                         null when n_scalar = 0); logits_dev float[n_samples][n_classes]; workspace of sd_viewnet_workspace_bytes;
 *                         flags_dev int32[2], zeroed by the call: [0] != 0 an fp16 activation overflowed (results invalid),
 *                         [1] != 0 a table entry outside [0, n_planes_total): that plane is not read and the results are invalid; its
 *                         layer-1 output keeps what the workspace held, the later layers run over it, and flag 0 may then be set by
 *                         those values too.  Both flags are plain stores of 1 by every thread that sees the condition.
 *   sd_viewnet_forward_timed  sd_viewnet_forward with a HIP event behind every launch; waits for the stream; ms_out[n_layers + 1] =
 *                         the time of every layer kernel and of the head kernel (tools/celltype_probe.py).
 *   sd_viewnet_overflow   flags_out[2] = the two flags (waits for the stream).
 *   sd_viewnet_read_buffer  after a forward, index i < n_layers: the stored output of layer i as float32
 *                         [n_samples * D][Ho][Wo][cout]; n_layers <= i < sd_viewnet_num_ops: the output of Linear i - n_layers (behind
 *                         its activation; the last one is the logits) as float32 [n_samples][out].  dims_out[4] = those extents
 *                         (the head's as [n_samples][1][1][out]).  out_host may be null to query dims_out only.
 *   sd_viewnet_num_ops    n_layers + n_fc.
 *   sd_viewnet_embed      sd_viewnet_forward -- the same arguments, layer launches, flags, workspace layout and checks -- with the
 *                         sample-tiled head: the form for calls of many samples with little convolution work each, as the
 *                         morphology embedding of /root/reference/syconn/reps/super_segmentation_helper.py:1758-1817 and
 *                         super_segmentation_object.py:3032-3079 through the RepresentationNetwork of
 *                         /root/reference/syconn/cnn/cnn_atn.py:21-55 (one sample = view 0 of one rendering location: D = 1,
 *                         table entry loc * nb_views).  A workgroup takes TS consecutive samples and reads every head weight once
 *                         per tile; per sample the arithmetic is that of sd_viewnet_forward's head, operation for operation, so the
 *                         logits and every hidden vector have the same bits.  TS = the largest of 8, 4, 2, 1 for which
 *                         4 TS (inputs of the first Linear + 2 x the widest Linear output) bytes fit 160 KiB.
 *   sd_viewnet_embed_timed  the same with the events of sd_viewnet_forward_timed (tools/embedding_probe.py).
 *   sd_viewnet_embed_tile_samples  TS of the model (0 for null).
 *   sd_viewnet_read_buffer works after either entry.
 * One grid stride of the layer kernel is SD_VIEWNET_GRID blocks (one block = 8 x 32 convolution outputs of one plane), of the head
 * kernel SD_VIEWNET_HEAD_GRID blocks (one block = one sample), of the tiled head kernel SD_VIEWNET_HEAD_TILE_GRID blocks (one block =
 * one tile of TS samples); none of the three constants rests on a measurement. */
#define SD_VIEWNET_GRID 2048
#define SD_VIEWNET_HEAD_GRID 32
#define SD_VIEWNET_HEAD_TILE_GRID 1024
typedef struct sd_viewnet_layer_desc { int32_t cout, k, pool; } sd_viewnet_layer_desc;
typedef struct sd_viewnet sd_viewnet;
int sd_viewnet_create(const sd_viewnet_layer_desc* layers, int n_layers, const int32_t* fc, int n_fc, int in_channels, int n_scalar, int act,
                      const float* weights, size_t n_floats, int act_dtype, sd_viewnet** out);
void sd_viewnet_destroy(sd_viewnet* m);
size_t sd_viewnet_workspace_bytes(sd_viewnet* m, size_t n_samples, int D, int H, int W);
int sd_viewnet_forward(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, const int32_t* sample_table_dev,
                       size_t n_samples, int D, const float* scalars_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes,
                       int32_t* flags_dev, void* stream);
int sd_viewnet_forward_timed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W,
                             const int32_t* sample_table_dev, size_t n_samples, int D, const float* scalars_dev, float* logits_dev,
                             void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out);
int sd_viewnet_embed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, const int32_t* sample_table_dev,
                     size_t n_samples, int D, const float* scalars_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes,
                     int32_t* flags_dev, void* stream);
int sd_viewnet_embed_timed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W,
                           const int32_t* sample_table_dev, size_t n_samples, int D, const float* scalars_dev, float* logits_dev,
                           void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out);
int sd_viewnet_embed_tile_samples(sd_viewnet* m);
int sd_viewnet_overflow(sd_viewnet* m, const int32_t* flags_dev, void* stream, int32_t* flags_out);
int sd_viewnet_read_buffer(sd_viewnet* m, int index, const void* workspace_dev, const float* logits_dev, size_t n_samples, int D, int H, int W,
                           float* out_host, int32_t* dims_out, void* stream);
int sd_viewnet_num_ops(sd_viewnet* m);

/* ---- the FCN semantic-segmentation network of the compartment step (csrc/sd_fcn.hip; host-only plan: csrc/sd_fcn.h) ---------------
 * Replaces the networks behind /root/reference/syconn/handler/prediction.py:1003-1030 (get_semseg_spiness_model,
 * get_semseg_axon_model -> InferenceModel) as /root/reference/syconn/reps/super_segmentation_helper.py:1353-1392
 * (predict_views_semseg) calls them: views / 255 -> FCNs(VGGNet) -> argmax over the classes.  elektronn3's fcn_2d is not part of the
 * reference tree; the architecture is stated, not pinned (syconn_amd/cnn/fcn_spec.py): five encoder blocks of 1 to 3
 * "3 x 3 convolution (padding 1) + ReLU" and a 2 x 2 max-pool each, five decoder steps "ConvTranspose2d(3, stride 2, padding 1,
 * output_padding 1) -> ReLU -> eval BatchNorm (eps 1e-5) -> + skip" (no skip behind the fifth), a 1 x 1 classifier.
 *   sd_fcn_create         blocks = output channels (1..512) of all encoder convolutions, block after block, block_len[5] = convolutions
 *                         per block (1..3); dec_last 1..512; n_class 1..16; in_channels 1..4; weights = float32 in registration order:
 *                         encoder w[cout][cin][3][3], b[cout]; per decoder step w[cin][cout][3][3], b, gamma, beta, running_mean,
 *                         running_var [cout]; classifier w[n_class][dec_last], b; act_dtype SD_F16 or SD_BF16 (storage of activations
 *                         and of the 3 x 3 weights; accumulation, bias, BatchNorm constants and the classifier are fp32).  A weight
 *                         that rounds to infinity in the storage type is refused.
 *   sd_fcn_forward        views_dev uint8[n_loc][in_channels][nb_views][H][W] as sd_views_render leaves them, n_planes_total =
 *                         n_loc * nb_views, H and W multiples of 32; the planes [plane0, plane0 + n_planes) are computed (plane =
 *                         loc * nb_views + view; the input is never copied into plane order; the first layer multiplies the integers u
 *                         and applies 1 / 255 in its fp32 epilogue).  labels_dev uint8[n_planes][H][W]: the argmax, the lowest index
 *                         wins exact ties -- for plane0 = 0 and all planes this is [n_loc][1][nb_views][H][W]; logits_dev
 *                         float[n_planes][n_class][H][W] or null; workspace of sd_fcn_workspace_bytes(m, n_planes, H, W), 16-byte
 *                         aligned; flags_dev int32[1], zeroed by the call: != 0 an fp16 activation reached 65520 before rounding
 *                         (results invalid; a plain store of 1 by every thread that sees it).
 *   sd_fcn_forward_timed  sd_fcn_forward with a HIP event behind the launches of every op; waits for the stream; ms_out[n_ops]
 *                         (tools/semseg_probe.py).
 *   sd_fcn_overflow       flags_out[1] = the flag (waits for the stream).
 *   sd_fcn_read_buffer    after a forward, index i < n_ops - 1: the stored output of op i as float32 [n_planes][h][w][c]; i = n_ops - 1:
 *                         the logits [n_planes][n_class][H][W] (needs logits_dev).  dims_out[4] = those extents; out_host may be null.
 *   sd_fcn_num_ops        encoder convolutions (the pool is part of a block's last one) + 5 decoder steps + the classifier.
 * A workgroup of the MFMA kernels computes 8 x 32 positions for at most 64 output channels; no grid is capped, a call whose launches
 * would pass 2^31 - 1 blocks is refused. */
typedef struct sd_fcn sd_fcn;
int sd_fcn_create(int in_channels, const int32_t* blocks, const int32_t* block_len, int dec_last, int n_class, const float* weights, size_t n_floats,
                  int act_dtype, sd_fcn** out);
void sd_fcn_destroy(sd_fcn* m);
size_t sd_fcn_workspace_bytes(sd_fcn* m, size_t n_planes, int H, int W);
int sd_fcn_forward(sd_fcn* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, size_t plane0, size_t n_planes,
                   uint8_t* labels_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream);
int sd_fcn_forward_timed(sd_fcn* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, size_t plane0, size_t n_planes,
                         uint8_t* labels_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream,
                         float* ms_out);
int sd_fcn_overflow(sd_fcn* m, const int32_t* flags_dev, void* stream, int32_t* flags_out);
int sd_fcn_read_buffer(sd_fcn* m, int index, const void* workspace_dev, const float* logits_dev, size_t n_planes, int H, int W, float* out_host,
                       int32_t* dims_out, void* stream);
int sd_fcn_num_ops(sd_fcn* m);

/* ---- glia probabilities from supervoxel views: the steps around the view network (csrc/sd_glia_views.hip) -------------------------
 *   sd_glia_view_probas        the probabilities behind /root/reference/syconn/handler/prediction.py:978-982 (get_glia_model_e3 ->
 *                              InferenceModel.predict_proba over cnn/cnn_gliaviews_e3.py:27 get_model), which reps/segmentation.py:799-814
 *                              thresholds: logits_dev float32[n][2] -> probas_dev float32[n][2] = softmax of every row, taken in float64
 *                              from the float32 logits with the row maximum subtracted and rounded once to float32.  Both 8-byte aligned;
 *                              n = 0 is legal.  flag_dev int32[1], zeroed by the call: != 0 a logit was NaN or infinite (that row's
 *                              result is meaningless).
 *   sd_views_center_component  /root/reference/syconn/proc/image.py:125-144 single_conn_comp_img, as proc/sd_proc.py:1404-1411
 *                              (predict_views, single_cc_only) applies it plane by plane, for a batch: in_dev / out_dev
 *                              uint8[n_planes][H][W], equal or disjoint.  Per plane: foreground = pixel != background; the pixels of the
 *                              4-connected foreground component (scipy.ndimage.label's default structure) that holds the centre pixel
 *                              (H / 2, W / 2) keep their value, every other pixel becomes background; a background centre empties the
 *                              plane (the reference's labeled == 0 branch).  One workgroup per plane holds two bit masks of the plane in
 *                              LDS: 8 H ceil(W / 32) + 16 bytes, which is what the launch requests; a plane for which that exceeds
 *                              SD_GLIA_VIEWS_LDS_BYTES (the LDS of a compute unit; 512 x 1024 fits) is SD_ERR_INVALID before anything
 *                              is launched.  n_planes = 0 is legal.
 * Asynchronous on the stream.  One grid stride of either kernel is SD_GLIA_VIEWS_GRID blocks (256 samples, or one plane, per block);
 * the constant rests on no measurement. */
#define SD_GLIA_VIEWS_GRID 1024
#define SD_GLIA_VIEWS_LDS_BYTES 163840
int sd_glia_view_probas(const float* logits_dev, size_t n, float* probas_dev, int32_t* flag_dev, void* stream);
int sd_views_center_component(const uint8_t* in_dev, size_t n_planes, int H, int W, int background, uint8_t* out_dev, void* stream);

/* ---- cell skeletons from a labelled chunk: TEASAR tracing (csrc/sd_skeletonize.hip) -----------------------------------------------
 * What proc/skeleton.py:21-86 (kimimaro_skelgen) gets from kimimaro.skeletonize, per chunk and for all cells at once.  kimimaro is not in
 * the reference tree: the rules are this build's, and the device equals their CPU restatement bit for bit.  Volumes
 * are (X, Y, Z) with z fastest, extents 1 .. SD_SKELETONIZE_MAX_EXTENT, fewer than 2^31 voxels; the raster index of a voxel is
 * (x Y + y) Z + z.  anisotropy_xyz: three integers 1 .. SD_SKELETONIZE_MAX_ANISOTROPY (nm per voxel; proc/skeleton.py:21-86 passes
 * kd.scales[0] * ds).  Tables per component are indexed by the component number c = 1 .. n_comp (entry 0 unused), so they hold n_comp + 1
 * entries.  Everything is asynchronous on the stream; argument errors are SD_ERR_INVALID with sd_last_error.  All entries with a
 * temp_dev take the scratch of sd_skeletonize_temp_bytes(X, Y, Z); it carries the dirty-tile state from sd_skeletonize_field_start /
 * sd_skeletonize_round to sd_skeletonize_relax, so the chain of one chunk uses one scratch.  counts_dev uint64[8].
 *   sd_skeletonize_components  (proc/skeleton.py:21-86, the cc3d step inside kimimaro) comp_dev int32: the 26-connected components of equal
 *                        non-zero label of seg_dev uint64, numbered 1 .. N in raster order of their first voxel; components with fewer
 *                        than dust_threshold voxels are 0 and take no number.  sizes_dev / labels_dev uint64[max_comps + 1], first_dev
 *                        int32[max_comps + 1] (first voxel).  counts[0] = N; [7] != 0: N > max_comps (the rest is numbered 0).
 *   sd_skeletonize_d2    (proc/skeleton.py:21-86, the edt step) d2_dev uint64 = min over voxels q of the array whose component number
 *                        differs (0 included) of sum_a (w_a (v_a - q_a))^2, 0 outside the components; the array border is no boundary.
 *                        dbf_dev float32 = float32(sqrt(double(d2))), dbf_max_dev float32[n_comp + 1] its maximum per component.
 *                        counts[1] != 0: a component has no differing voxel in the array (its d2 is 2^64 - 1, its dbf +inf).
 *   sd_skeletonize_field_start  (proc/skeleton.py:21-86, the dijkstra3d fields) field_dev (float32, or float64 with field_f64 = 1) = +inf,
 *                        0 at source_dev[c] (int32[n_comp + 1], < 0: none) of every component; marks the tiles around the sources.
 *   sd_skeletonize_relax (proc/skeleton.py:21-86) up to max_sweeps (rounded up to a multiple of 6, at most SD_SKELETONIZE_MAX_SWEEPS)
 *                        sweeps towards the fixed point of field(v) = min over the 26 same-component neighbours u of
 *                        fl(field(u) + cost): penalty_dev == NULL: float32 field, cost = float32(sqrt(double(sum (w_a o_a)^2))) of the
 *                        offset; else float64 field, cost = penalty_dev[v].  A sweep is one launch over the dirty tiles of edge
 *                        SD_SKELETONIZE_TILE, each relaxed to local convergence in LDS; a launch without dirty tiles returns at once.
 *                        counts[3] = dirty tiles left (0: converged; otherwise call again, the field continues from its values),
 *                        [4] += sweeps that had work, [5] += tiles relaxed, [6] != 0: a tile passed its local bound of
 *                        SD_SKELETONIZE_TILE^3 + 1 steps.  The caller bounds the sweeps by the foreground voxels + 1.
 *   sd_skeletonize_argmax  (proc/skeleton.py:21-86, root and target selection) index_dev int32[n_comp + 1] = the voxel with the largest
 *                        field_dev value (float32, >= 0) per component among those with valid_dev != 0 (NULL: all), the smallest raster
 *                        index on ties, -1 without one; value_dev float32[n_comp + 1] (may be NULL); keys_dev uint64[n_comp + 1] scratch.
 *   sd_skeletonize_penalty  (proc/skeleton.py:21-86, the PDRF) penalty_dev float64 = pdrf_scale (1 - double(dbf) / m_dev[c])^e +
 *                        double(daf) / double(daf_max_dev[c]) (the second term 0 where daf_max is 0), e = 1 .. SD_SKELETONIZE_MAX_EXPONENT
 *                        by e - 1 multiplications, every operation rounded once.  m_dev float64[n_comp + 1] is the caller's dbf_max ** 1.01.
 *   sd_skeletonize_round (proc/skeleton.py:21-86, one path with fix_branching) per component that is not void: walk from target_dev[c]
 *                        (< 0: none) by parent steps -- the same-component neighbour with the smallest dist_dev, the smallest raster
 *                        index on ties -- to the first voxel with dist == 0; the walked voxels get parent_dev (int32, -1 before), dist 0,
 *                        and clear valid_dev (uint8) for the voxels u of their component with |u_a - v_a| <= floor(double(r) / w_a),
 *                        r = fl32(fl32(inv_scale dbf(v)) + inv_const).  root_dev (int32[n_comp + 1]; NULL after the first round) joins
 *                        the new nodes with parent = itself.  The new sources' tiles are marked: sd_skeletonize_relax on dist follows.
 *                        counts[1] != 0: a walk passed sizes_dev[c] steps, [2] += walks whose step did not lower dist (float64
 *                        absorption); both set void_dev[c] (int32[n_comp + 1], zeroed by the caller), which empties c's result.
 *   sd_skeletonize_emit  (proc/skeleton.py:21-86, the skeleton of every component) nodes = voxels with parent >= 0 of components that
 *                        are not void, by component and ascending raster index: node_begin_dev / edge_begin_dev uint64[n_comp + 2]
 *                        (entry c .. c + 1 bounds component c), node_voxel_dev int32[max_nodes], vertices_dev float32[max_nodes][3] =
 *                        float32(voxel w), radii_dev float32 = dbf, edges_dev int32[max_nodes][2] = (node, parent) as indices inside the
 *                        component, one per node that is not the root, in node order.  counts[0] = nodes needed; above max_nodes
 *                        only the two offset tables are written (and mean nothing).  Further scratch: sd_skeletonize_emit_temp_bytes.
 * One grid stride: SD_SKELETONIZE_VOX_GRID blocks of 256 voxels, SD_SKELETONIZE_TILE_GRID tiles, SD_SKELETONIZE_COMP_GRID blocks of 256
 * components, SD_SKELETONIZE_NODE_GRID blocks (one new node each, or 256 table rows).  None of the constants rests on a measurement. */
#define SD_SKELETONIZE_TILE 16
#define SD_SKELETONIZE_MAX_EXTENT 2048
#define SD_SKELETONIZE_MAX_ANISOTROPY 32768
#define SD_SKELETONIZE_MAX_EXPONENT 64
#define SD_SKELETONIZE_MAX_SWEEPS 1536
#define SD_SKELETONIZE_VOX_GRID 8192
#define SD_SKELETONIZE_TILE_GRID 2048
#define SD_SKELETONIZE_COMP_GRID 1024
#define SD_SKELETONIZE_NODE_GRID 2048
size_t sd_skeletonize_temp_bytes(int X, int Y, int Z);
int sd_skeletonize_components(const uint64_t* seg_dev, int X, int Y, int Z, uint64_t dust_threshold, int32_t* comp_dev, uint64_t* sizes_dev,
                              uint64_t* labels_dev, int32_t* first_dev, size_t max_comps, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                              void* stream);
int sd_skeletonize_d2(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, size_t n_comp, uint64_t* d2_dev, float* dbf_dev,
                      float* dbf_max_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_skeletonize_field_start(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* source_dev, size_t n_comp, void* field_dev, int field_f64,
                               void* temp_dev, size_t temp_bytes, void* stream);
int sd_skeletonize_relax(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, void* field_dev, const double* penalty_dev,
                         int max_sweeps, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream);
int sd_skeletonize_argmax(const int32_t* comp_dev, const float* field_dev, const uint8_t* valid_dev, size_t n_vox, size_t n_comp, int32_t* index_dev,
                          float* value_dev, uint64_t* keys_dev, void* stream);
int sd_skeletonize_penalty(const int32_t* comp_dev, const float* dbf_dev, const float* daf_dev, size_t n_vox, size_t n_comp, const double* m_dev,
                           const float* daf_max_dev, double pdrf_scale, int pdrf_exponent, double* penalty_dev, void* stream);
int sd_skeletonize_round(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, const float* dbf_dev, double* dist_dev,
                         uint8_t* valid_dev, int32_t* parent_dev, const int32_t* target_dev, const int32_t* root_dev, const uint64_t* sizes_dev,
                         size_t n_comp, float inv_scale, float inv_const, int32_t* void_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                         void* stream);
size_t sd_skeletonize_emit_temp_bytes(size_t max_nodes);
int sd_skeletonize_emit(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, const int32_t* parent_dev, const float* dbf_dev,
                        const int32_t* root_dev, const int32_t* void_dev, size_t n_comp, size_t max_nodes, uint64_t* node_begin_dev,
                        uint64_t* edge_begin_dev, int32_t* node_voxel_dev, float* vertices_dev, float* radii_dev, int32_t* edges_dev,
                        uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* emit_temp_dev, size_t emit_temp_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYCONN_DENSE_H */
