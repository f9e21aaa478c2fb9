/* emap_hip.h -- C ABI of the MI355X (gfx950) elevation-map fusion core.
 *
 * The reference (leggedrobotics/elevation_mapping_cupy) has no C FFI: its numeric core is a set of CuPy
 * ElementwiseKernels JIT-compiled from strings and driven by the Python class ElevationMap.  This header is
 * the drop-in boundary a maintainer binds instead (ctypes stub in INTEGRATION.md); every entry point cites
 * the reference interface it replaces.  `EM/` = elevation_mapping_cupy/script/elevation_mapping_cupy/.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * emap_status; nothing throws; no global state; one HIP stream per context; a context is
 * thread-compatible (callers serialise per context, as the reference does with map_lock).
 * Host pointers are borrowed for the duration of the call; the context owns all device memory.
 */
#ifndef EMAP_HIP_H_
#define EMAP_HIP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4/5): emap_halo_pack / emap_halo_unpack / emap_halo_bytes move 16-byte COLD half cells (halo * cell_n * 4 floats) instead of
 * 32-byte cells; emap_upload_points de-interleaves the extra channels; emap_comm_init makes the ranks agree on this number. */
#define EMAP_ABI_VERSION 3

typedef enum {
  EMAP_OK = 0,
  EMAP_ERR_INVALID = -1,   /* bad argument */
  EMAP_ERR_HIP = -2,       /* HIP runtime error, see emap_last_error */
  EMAP_ERR_NO_POINTS = -3, /* stage needs a point cloud but none is bound */
  EMAP_ERR_UNSUPPORTED = -4,
  EMAP_ERR_COMM = -5       /* RCCL could not be loaded or a collective failed, see emap_last_error */
} emap_status;

/* index/rounding mode: 0 reproduces the reference's CuPy float16 helper-parameter rounding
 * bit for bit (valid for cell_n <= 2049); 1 = the same source with float16 := float (any cell_n), the cell index evaluated
 * in float: trunc(x * float(1/resolution) + cell_n/2), two roundings, clamped to [0, cell_n-1]. */
enum { EMAP_MODE_REFERENCE_FP16 = 0, EMAP_MODE_FP32 = 1 };

/* Mirrors the scalar fields of the reference's Parameter dataclass (EM/parameter.py:137-216) that the hot
 * path bakes into its kernels (EM/elevation_mapping.py:228-282).  Doubles hold the Python floats exactly. */
typedef struct emap_params {
  int32_t cell_n;                    /* map side incl. the 1-cell border (parameter.py:287) */
  int32_t mode;                      /* EMAP_MODE_* */
  int32_t enable_edge_sharpen, enable_visibility_cleanup, enable_drift_compensation, enable_overlap_clearance;
  int32_t dilation_size, pad_;
  double resolution, sensor_noise_factor, mahalanobis_thresh, outlier_variance;
  double drift_compensation_variance_inlier, traversability_inlier, wall_num_thresh, max_ray_length;
  double cleanup_step, cleanup_cos_thresh, min_valid_distance, max_height_range;
  double ramped_height_range_a, ramped_height_range_b, ramped_height_range_c, max_variance;
  double initial_variance, time_variance, time_interval, min_height_drift_cnt;
  double max_drift, drift_compensation_alpha, position_noise_thresh, orientation_noise_thresh;
  double overlap_clear_range_xy, overlap_clear_range_z, ray_step, reserved_;
  float w1[36], w2[36], w3[36], w_out[12]; /* traversability filter weights (EM/traversability_filter.py:15-24) */
} emap_params;

/* Row-strip placement of this context inside the global map (single GPU: row_begin 0, row_count cell_n,
 * halo_rows 0).  Cell index = cell_n * ix + iy (custom_kernels.py:45-49), so a strip is a range of ix. */
typedef struct emap_strip {
  int32_t row_begin, row_count, halo_rows, pad_;
} emap_strip;

typedef struct emap_stats {
  double err_sum;          /* sum of z - map_h over drift inliers (custom_kernels.py:331-334), local strip */
  uint32_t err_cnt;        /* number of drift inliers, local strip */
  int32_t gate_fired;      /* drift gate of elevation_mapping.py:346-354 fired this frame */
  float mean_error;        /* elevation_mapping.py:355 */
  float additive_mean_error; /* elevation_mapping.py:356 / get_additive_mean_error :412 */
  float shift;             /* amount added to the elevation plane (:357), 0 if none */
  uint32_t n_points;       /* points bound for the frame */
  uint64_t ray_visits;     /* inside-map cells visited by the visibility pass (0 unless stats requested).  Row strips marching BY ROW: the
                              visits inside this strip's rows; marching BY RAY (emap_set_ray_mode): the visits of THIS rank's rays over the
                              whole ray window -- either way the sum over the ranks is the single context's count */
} emap_stats;

typedef struct emap_ctx emap_ctx;

/* plane ids for emap_get_layer / emap_set_layer: 0..6 = the reference's elevation_map planes in its order
 * (elevation, variance, is_valid, traversability, time, upper_bound, is_upper_bound; elevation_mapping.py:68-77),
 * 7..9 = normal_map x,y,z (:81), 10 = traversability_input (dilated upper bound, :377-383). */
enum { EMAP_PLANE_ELEVATION = 0, EMAP_PLANE_VARIANCE, EMAP_PLANE_IS_VALID, EMAP_PLANE_TRAVERSABILITY, EMAP_PLANE_TIME,
       EMAP_PLANE_UPPER_BOUND, EMAP_PLANE_IS_UPPER_BOUND, EMAP_PLANE_NORMAL_X, EMAP_PLANE_NORMAL_Y,
       EMAP_PLANE_NORMAL_Z, EMAP_PLANE_TRAV_INPUT, EMAP_PLANE_COUNT };

/* ---- lifetime ------------------------------------------------------------------------------------- */
int emap_abi_version(void);
/* Replaces ElevationMap.__init__ allocation + compile_kernels (EM/elevation_mapping.py:52-117, 228-282).
 * `stream` = an existing hipStream_t to enqueue on (e.g. torch's current stream) or NULL for a private one. */
int emap_create(const emap_params* params, const emap_strip* strip_or_null, int device, void* stream, emap_ctx** out);
int emap_destroy(emap_ctx* ctx);
int emap_set_params(emap_ctx* ctx, const emap_params* params); /* same cell_n; parameters are kernargs, no JIT */
const char* emap_last_error(const emap_ctx* ctx);
int emap_sync(emap_ctx* ctx);
/* ElevationMap.clear (EM/elevation_mapping.py:119-128) */
int emap_clear(emap_ctx* ctx);

/* ---- point cloud ------------------------------------------------------------------------------------ */
/* ElevationMap.input_pointcloud's H2D + cast (EM/elevation_mapping.py:456): rows of `stride` elements,
 * xyz first; dtype 0 = float32, 1 = float64.  Rows with NaN in xyz are skipped inside the kernels (:458).
 * A cloud with extra channels (stride > 3) is de-interleaved while it is converted: on the device it is an (n, 3) xyz matrix
 * and an (n, stride - 3) channel matrix (the reference keeps the interleaved rows and strides over them in every kernel). */
int emap_upload_points(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype);
/* Row strips (multi-GPU): every rank is handed the SAME sensor cloud, but only the points of its rows reach its tile kernels.  Converts,
 * uploads and binds only the points that can land in this strip's rows under the pose (R, t map-centre relative, as emap_update takes
 * them) -- a conservative superset decided on the host, order preserved, so the strip's maps stay bit-identical -- i.e. 1 / G of the
 * cloud crosses PCIe and is streamed per rank (reference side: input_pointcloud uploads the whole cloud, EM/elevation_mapping.py:434-466;
 * SURVEY 8(e) "host bucket by strip").  The frame that follows must use the same pose and must not march its rays BY ROW
 * (emap_update_sharded checks both); class_bayesian / bayesian_inference fusions need the whole cloud (global point index).  On a
 * whole-map context it is emap_upload_points.  n_kept (may be NULL): points bound. */
int emap_upload_points_strip(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype, const float R[9], const float t[3], int64_t* n_kept);
/* the same predicate as data: keep[i] = 1 iff emap_upload_points_strip would upload point i (for callers that keep their clouds on
 * the device and bucket them themselves; they then declare the bound cloud with emap_declare_points_bucketed) */
int emap_strip_point_mask(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype, const float R[9], const float t[3], uint8_t* keep);
int emap_declare_points_bucketed(emap_ctx* ctx, const float R[9], const float t[3], int64_t n_all);   /* n_all: size of the whole cloud */
/* bind a device-resident float32 cloud without copying (update_map_with_kernel takes device arrays, :316) */
int emap_set_points_device(emap_ctx* ctx, const float* dev, int64_t n, int64_t stride);
/* the same for a cloud that is already de-interleaved on the device (what emap_upload_points produces): xyz (n, 3) and the
 * extra channels (n, n_chan), both row-major float32; channel column c of the caller's (n, 3 + n_chan) numbering is column
 * c - 3 of chan_dev */
int emap_set_points_device_split(emap_ctx* ctx, const float* xyz_dev, const float* chan_dev, int64_t n, int64_t n_chan);
/* Depth-image input.  The reference back-projects a depth camera's frame on the HOST and hands the float cloud to input_pointcloud
 * (sensor_processing/semantic_sensor/.../pointcloud_node.py:205-250 create_pcl_from_image, :261-269 process_image); here the images
 * are uploaded (2-4 bytes a pixel instead of 12-24 a point) and the cloud is produced on the device, into a buffer the context owns,
 * and bound like a caller's de-interleaved device cloud.  depth: height x width row-major, float32 metres (depth_dtype 0) or uint16
 * units of depth_scale metres (depth_dtype 1).  Every step-th row and column is sampled: Hs = ceil(height / step), Ws = ceil(width /
 * step), n = Hs Ws rows in the reference's nonzero order (row i = (v / step) Ws + u / step), NOT compacted: a pixel that is not
 * valid -- valid = isfinite(z) && z > min_depth && z < max_depth && (no confidence image || confidence >= confidence_threshold), the
 * reference's rule with min 0, max 8 -- becomes a row of NaNs (bits 0x7FC00000), which every kernel skips.  A valid pixel:
 * x = (((float)u - cx) * z) / fx, y = (((float)v - cy) * z) / fy, z, in float32, round to nearest, never contracted.  Channels (written
 * for every row): the colour first if has_rgb (rgb: height x width x 3 uint8; a float with the BITS r << 16 | g << 8 | b, the wire
 * format of process_image), then features[k][v][u], k < n_features (planar float32); at most 16 in all.  confidence: height x width
 * float32 or NULL.  Refused with EMAP_ERR_INVALID before anything is copied or launched, the previous binding untouched: a NULL
 * required pointer, sides outside 1 .. 8192, step outside 1 .. 64, fx or fy zero or not finite, cx / cy / min_depth / max_depth not
 * finite, min_depth < 0, max_depth <= min_depth, uint16 depth with a depth_scale that is not finite and > 0, more than 16 channels, an
 * unknown depth_dtype.  The caller's images are only borrowed (copied before the call returns); nothing waits for the device.
 * n_points_out (may be NULL): n.  Row-strip contexts: the cloud is bound whole and unbucketed. */
typedef struct emap_depth_desc {
  int32_t height, width, depth_dtype, step, has_rgb, n_features;
  float fx, fy, cx, cy, depth_scale, min_depth, max_depth, confidence_threshold;
} emap_depth_desc;
int emap_bind_depth_image(emap_ctx* ctx, const emap_depth_desc* desc, const void* depth, const uint8_t* rgb_or_null, const float* features_or_null,
                          const float* confidence_or_null, int64_t* n_points_out);
/* PointCloud2 input.  The reference's node walks a sensor_msgs/PointCloud2 message on the HOST, one point and one field at a time
 * (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:319-338: memcpy(&temp, &data[i * point_step + fields[j].offset], 4), widened
 * into an (n, fields) float64 matrix), and input_pointcloud casts the matrix back to float32 and uploads it; here the message's BYTES
 * are uploaded (point_step a point) and unpacked on the device, into the buffer the depth-image input owns, and bound exactly as that
 * input binds its cloud.  data: height * row_step bytes.
 * Rows: n = height * width; output row i = r * width + c reads its point at byte r * row_step + c * point_step.  The reference
 * ignores row_step (:335, i * point_step); with row_step == width * point_step the two agree.  Nothing is compacted: a row whose x, y
 * or z is NaN is skipped by every kernel, as for any bound cloud; no range filter is applied.
 * Columns: n_cols = 3 + channels; column c is read at offset[c] inside the point; columns 0, 1, 2 are x, y, z.
 *   conv[c] == 0 (pure move, the node's memcpy): the output float has the four message bytes at the offset as its bits (little
 *   endian), moved with integer operations only -- NaN payloads and subnormal patterns such as the packed rgb colour arrive untouched.
 *   conv[c] == 1 .. 8 (typed; the sensor_msgs/PointField datatype: 1 INT8 2 UINT8 3 INT16 4 UINT16 5 INT32 6 UINT32 7 FLOAT32 8 FLOAT64):
 *   the value is loaded little-endian at the field's width and converted to float32 with ONE C conversion, round to nearest even,
 *   subnormals kept; a float64 too large for float32 becomes +-inf; a float64 NaN stays a NaN (its payload bits are not part of the
 *   contract); conv 7 produces the bits of conv 0.
 * Output: the layout emap_set_points_device_split takes -- xyz (n, 3), the channels (n, n_cols - 3) at a 256-byte boundary behind it
 * -- read back by emap_get_bound_points.  Row-strip contexts: the cloud is bound whole and unbucketed.
 * Refused with EMAP_ERR_INVALID before anything is copied or launched, the previous binding untouched and *n_points_out not written:
 * a NULL ctx, desc or data; is_bigendian != 0; height or width < 1; n > 2^26; point_step outside 1 .. 256; row_step < width *
 * point_step; height * row_step >= 2^31; n_cols outside 3 .. 19; an unknown conv; an offset < 0; a column whose bytes (4 for conv 0,
 * the datatype's size otherwise) do not lie inside the point -- a departure: the reference would read into the next point there.
 * The caller's bytes are only borrowed (copied into a pinned slot before the call returns; a message of more than 2 MB by the
 * upload's worker threads, chunk by chunk, each chunk's DMA behind it); nothing waits for the device on the success path.
 * n_points_out (may be NULL): n. */
typedef struct emap_cloud_msg_desc {
  int32_t height, width, point_step, row_step, is_bigendian, n_cols;   /* n_cols = 3 + channels, 3 .. 19 */
  int32_t offset[19];    /* byte offset of column c inside a point; columns 0, 1, 2 are x, y, z */
  int32_t conv[19];      /* 0: the 4 bytes at the offset ARE the float32 (pure move, the node's memcpy);
                            1..8: convert from that sensor_msgs/PointField datatype
                            (1 INT8 2 UINT8 3 INT16 4 UINT16 5 INT32 6 UINT32 7 FLOAT32 8 FLOAT64) to float32 */
} emap_cloud_msg_desc;
int emap_bind_cloud_message(emap_ctx* ctx, const emap_cloud_msg_desc* desc, const uint8_t* data, int64_t* n_points_out);
/* the cloud bound now, whoever bound it (uploaded, a caller's device cloud interleaved or split, a back-projected depth image -- what
 * pointcloud_node.py:205-250, 261-269 would have published): xyz_host (n, 3), chan_host_or_null (n, n_cols - 3), float32.  Waits for
 * the stream.  EMAP_ERR_NO_POINTS when nothing is bound. */
int emap_get_bound_points(emap_ctx* ctx, float* xyz_host, float* chan_host_or_null);
/* tail of add_points_kernel (custom_kernels.py:260-262): per point cell idx, is_valid, is_inside */
int emap_point_index(emap_ctx* ctx, const float R[9], const float t[3], int32_t* idx, uint8_t* valid, uint8_t* inside);

/* ---- one frame = update_map_with_kernel (EM/elevation_mapping.py:316-391); t already centre-relative --
 * After the call returns, the stream holds the frame up to its stencil pass (dilation, traversability filter, normals).  The pass is
 * queued by the next call that needs it, or with the next frame.  Any library call that reads, changes or waits for the map sees the
 * complete frame.
 * (A whole-map frame on the tile-binned path leaves the pass pending; the next such frame runs it in one launch with its own
 * histogram, k_post_hist.  The calls that do not queue it are the ones a frame is made of or that touch neither the map nor the stream:
 * emap_set_points_device, emap_set_points_device_split, emap_frame_semantics, emap_update, emap_last_error, emap_last_update_path,
 * emap_get_stage_times, emap_enable_stage_timing, emap_timer_begin.  A caller that enqueues work of its own on a stream it handed to
 * emap_create orders it behind the frame with emap_sync or any other call.  EMAP_POST_DEFER=0 in the environment: every frame queues
 * its own pass, as before.) */
int emap_update(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise,
                emap_stats* stats_or_null);
/* individually callable stages (same order inside emap_update) */
int emap_count(emap_ctx* ctx, const float R[9], const float t[3]);          /* error_counting_kernel :334-345 */
int emap_set_drift_inputs(emap_ctx* ctx, double position_noise, double orientation_noise, const double* err_sum_override,
                          const uint32_t* err_cnt_override); /* gate inputs (:346-354); overrides = all-reduced totals */
/* row strips: publish the strip-local (err_sum, err_cnt) as 2 doubles in DEVICE memory (async, no host sync) so
 * the caller can all-reduce them (RCCL), then gate on the reduced totals read from device memory. The _local_ form
 * is the blocking host variant. */
int emap_drift_sums_to_device(emap_ctx* ctx, double* dev_out2);
int emap_set_drift_inputs_device(emap_ctx* ctx, double position_noise, double orientation_noise, const double* dev_totals2);
int emap_local_drift_sums(emap_ctx* ctx, double* err_sum, uint32_t* err_cnt);
/* how the count/fuse passes scatter into the map: 0 = auto (tile-binned LDS reduction for clouds >= 131072 points, else global
 * atomics), 1 = global atomics, 2 = tile-binned. Results are bit-identical. Bins are 16x64-cell tiles; maps with more than
 * 16384 tiles stack 2, 4, ... tiles per bin. Test hook: bits 8..15 of `mode` force a minimum stacking factor (power of two). */
int emap_set_scatter_mode(emap_ctx* ctx, int32_t mode);
int emap_fuse(emap_ctx* ctx, const float R[9], const float t[3]);           /* add_points_kernel fusion part */
int emap_fuse_average(emap_ctx* ctx, const float R[9], const float t[3]);   /* fuse+commit+average when no ray pass follows */
int emap_commit(emap_ctx* ctx);                                             /* side effects of :174,:189-192 -> S1 */
int emap_rays(emap_ctx* ctx, const float R[9], const float t[3]);           /* add_points_kernel visibility part */
int emap_average(emap_ctx* ctx);                                            /* average_map_kernel :369 */
int emap_overlap_clear(emap_ctx* ctx, float t_z);                           /* clear_overlap_map :393-410 */
int emap_dilate(emap_ctx* ctx);                                             /* dilation_filter_kernel :376-383 */
int emap_traversability_normals(emap_ctx* ctx);                             /* :385-391 (filter + update_normal) */
int emap_post(emap_ctx* ctx);                                               /* the two stages above fused (used by emap_update) */
/* row strips: part 1 = tile rows independent of the halo (overlaps the halo exchange), part 2 = boundary tile rows */
int emap_post_part(emap_ctx* ctx, int32_t part);
int emap_update_variance(emap_ctx* ctx);                                    /* :420-422 */
int emap_update_time(emap_ctx* ctx);                                        /* :424-426 */
int emap_get_stats(emap_ctx* ctx, emap_stats* out);                         /* blocking D2H of the frame scalars */

/* ---- state access (elevation_map attribute / get_map_with_name_ref's raw planes; test state injection) */
int emap_get_layer(emap_ctx* ctx, int plane, float* host_out /* (row_count, cell_n) */);
int emap_set_layer(emap_ctx* ctx, int plane, const float* host_in);
/* ElevationMap.get_map_with_name_ref for the built-in layers (EM/elevation_mapping.py:579-775): fills a C-order
 * (cell_n-2, cell_n-2) buffer: border stripped, both axes flipped, NaN for unknown cells, +center_z for heights.
 * kind: 0 elevation, 1 variance, 2 traversability, 3 time, 4 upper_bound, 5 is_upper_bound, 6..8 normal_x/y/z */
int emap_publish_layer(emap_ctx* ctx, int32_t kind, float center_z, int32_t use_only_above_for_upper_bound, float* host_out);
/* GridMap message output: every device-resident layer a grid_map_msgs/GridMap publisher asks for, from ONE launch, one device-to-host
 * copy per run of adjacent slots and one wait (the reference's node: one get_map_with_name_ref per layer, a transposing copy in
 * gridMap.add, a host loop for the normal colour, one more copy in toMessage -- elevation_mapping_wrapper.cpp:213-252, :296-314;
 * elevation_mapping_ros.cpp:269-301).  host_out holds host_slots planes of M * M floats, M = cell_n - 2; layer k of the table lands in
 * plane layers[k].slot; planes the table does not name are not written (the caller fills them, e.g. with plugin layers).  Element
 * (i, j) of a plane -- border stripped, both axes flipped: logical source cell (M - i, M - j) -- lies at
 *   order EMAP_GRID_ROWS     i * M + j   what emap_publish_layer / get_map_with_name_ref leave in a C-order buffer
 *   order EMAP_GRID_MESSAGE  j * M + i   the column-major Float32MultiArray of grid_map_msgs/GridMap: dim[0] = {"column_index", M, M * M},
 *                                        dim[1] = {"row_index", M, M}, data_offset 0, start indices 0
 * kind EMAP_GRID_BUILTIN: index = emap_publish_layer's kind 0 .. 8, the same values bit for bit (center_z and
 * use_only_above_for_upper_bound as there).  kind EMAP_GRID_SEMANTIC: index = the semantic layer; its 32-bit words are moved as they
 * are (colour and class layers hold bit patterns): no NaN fill, no center_z, as SemanticMap.get_map_with_name.  kind
 * EMAP_GRID_NORMAL_COLOR (index ignored): the wrapper's addNormalColorLayer on the normal planes -- cx = (float)((nx + 1.0) / 2.0), cy
 * likewise, cz = nz; r, g, b = (int)(c * 255.0f), truncated; the value is the float whose bits are (r << 16) | (g << 8) | b.  A
 * component that is not finite or beyond int is undefined in the reference; here the conversion saturates and NaN gives 0.
 * A half of a cell and a normal plane are read at most once per launch however many layers need them, and not at all if none does.
 * Refused with EMAP_ERR_INVALID before anything is launched or copied, host_out untouched: a NULL pointer; n_layers outside 1 .. 32;
 * an unknown kind or order; a built-in index outside 0 .. 8; a semantic index that is not configured; a slot outside [0, host_slots);
 * a slot named twice; a row-strip context.  Returns when host_out is filled. */
enum { EMAP_GRID_ROWS = 0, EMAP_GRID_MESSAGE = 1 };
enum { EMAP_GRID_BUILTIN = 0, EMAP_GRID_SEMANTIC = 1, EMAP_GRID_NORMAL_COLOR = 2 };
#define EMAP_GRID_MAX_LAYERS 32
typedef struct emap_grid_layer { int32_t kind, index, slot; } emap_grid_layer;
int emap_publish_grid_map(emap_ctx* ctx, const emap_grid_layer* layers, int32_t n_layers, int32_t order,
                          float center_z, int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots);
/* The same launch with plugin layers read from the context's resident planes (emap_plugin_planes / emap_plugin_chain below) next to the
 * cells: kind EMAP_GRID_PLUGIN, index = the resident plane, which holds the plugin's RAW output (cell_n x cell_n, logical order, border
 * included: PluginManager.layers[index], EM/plugins/plugin_manager.py:130).  The plane is read at the logical source cell
 * (M - i, M - j) and published as ElevationMap.process_map_for_publish does (EM/elevation_mapping.py:579-596), in its order: flags
 * EMAP_GRID_FILL_NAN -- NaN where is_valid is not above 0.5 (the plugin's fill_nan) -- then EMAP_GRID_ADD_Z -- + center_z in float32
 * (its is_height_layer).  flags must be 0 on every other kind.  Everything else, every refusal included, as emap_publish_grid_map;
 * refused as well: a plugin plane outside the reservation, an unknown flag.  emap_publish_grid_map is this call without flags and
 * without kind EMAP_GRID_PLUGIN, which it refuses. */
enum { EMAP_GRID_PLUGIN = 3 };
enum { EMAP_GRID_FILL_NAN = 1, EMAP_GRID_ADD_Z = 2 };
typedef struct emap_grid_layer_ex { int32_t kind, index, slot, flags; } emap_grid_layer_ex;
int emap_publish_grid_map_ex(emap_ctx* ctx, const emap_grid_layer_ex* layers, int32_t n_layers, int32_t order,
                             float center_z, int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots);
/* Submap service: a batch of WINDOWS of the published map from one launch -- what the node's get_submap service
 * (elevation_mapping_ros.cpp:507-553, grid_map_msgs/GetGridMap: GridMap::getSubmap, then toMessage) cuts out of the whole grid map on
 * the host, here without reading, writing or copying anything of the size of the map.  Window w covers the published elements
 * (i0 + i, j0 + j), 0 <= i < ni, 0 <= j < nj, of the index space emap_publish_grid_map_ex writes (M = cell_n - 2 a side).  Layers,
 * kinds, flags, values, center_z, use_only_above_for_upper_bound and order are exactly those of emap_publish_grid_map_ex, bit for bit;
 * the slot of an entry is NOT read.  host_out is packed: window w starts at float n_layers * (the sum of ni * nj over the windows
 * before it); inside a window layer k of the table is plane k (ni * nj floats), and element (i, j) of the window lies at
 *   order EMAP_GRID_ROWS     i * nj + j
 *   order EMAP_GRID_MESSAGE  j * ni + i   dim[0] = {"column_index", nj, ni * nj}, dim[1] = {"row_index", ni, ni}
 * Overlapping and repeated windows are legal.  One upload of the window table, one launch, ONE device-to-host copy, one wait; the
 * buffers belong to the context and grow on demand.  Refused with EMAP_ERR_INVALID before anything is uploaded, launched or copied,
 * host_out and the map untouched: everything emap_publish_grid_map_ex refuses of a layer table; a NULL windows; n_windows outside
 * 1 .. EMAP_GRID_MAX_WINDOWS (a cap, not a measurement); a window with ni < 1, nj < 1, i0 < 0, j0 < 0, i0 + ni > M or j0 + nj > M;
 * host_floats different from the packed total; a row-strip context. */
#define EMAP_GRID_MAX_WINDOWS 64
typedef struct emap_grid_window { int32_t i0, j0, ni, nj; } emap_grid_window;
int emap_publish_grid_windows(emap_ctx* ctx, const emap_grid_layer_ex* layers, int32_t n_layers, int32_t order,
                              float center_z, int32_t use_only_above_for_upper_bound, const emap_grid_window* windows, int32_t n_windows,
                              float* host_out, int64_t host_floats);
/* Point-cloud output: the VALID cells of the published map as the records of a sensor_msgs/PointCloud2, packed on the device in
 * grid_map's iterator order -- what the node's elevation_map_points publisher (elevation_mapping_ros.cpp:501-505,
 * GridMapRosConverter::toPointCloud) and its normal arrows (:751-809) walk the whole grid map for on the host.  The index space is
 * that of emap_publish_grid_map_ex (M = cell_n - 2 a side, element (i, j) = logical source cell (M - i, M - j)); GridMapIterator runs
 * lin = j * M + i, j outer: the flat order of an EMAP_GRID_MESSAGE plane.  Record k is the k-th cell of that order that passes; the bytes
 * are unique for a map state (no atomic decides a position).  grid_map is restated here, not pinned by a compiled reference.
 * fields: kind / index / flags of an entry are those of emap_grid_layer_ex, the values bit for bit.  cloud_flags: EMAP_CLOUD_POINT --
 * exactly one entry: it emits x, y, z (x = x_of_i[i], y = y_of_j[j], z = its value) and a cell passes only if its value is finite;
 * EMAP_CLOUD_TEST -- a cell passes only if the entry's value is finite (a basic layer); EMAP_CLOUD_HIDDEN (with TEST) -- tested, not
 * emitted.  Every entry that is not HIDDEN emits one float32 (POINT: three), in table order, 4 bytes apart.  call_flags:
 * EMAP_CLOUD_NORMAL_MIN -- a cell passes only if !(sqrt((nx nx + ny ny) + nz nz) < normal_min) in double on its normal (a NaN normal
 * passes); EMAP_CLOUD_INDEX -- lin is appended to every record as a 4-byte integer.  x_of_i, y_of_j: M floats each, computed by the
 * caller (in double, then rounded).  *point_step = 4 * the dwords of a record; *n_points = the cells that pass.
 * One upload of the position tables, three launches (count, scan, write), a 4-byte copy of the count and a wait; then ONE copy of
 * exactly *n_points * *point_step bytes to host_out and a second wait (none when no cell passes).  If more than capacity_points
 * cells pass, *n_points and *point_step are set, host_out is NOT written and EMAP_ERR_INVALID is returned (a caller tells it from a
 * refusal by *n_points > capacity_points).  The buffers belong to the context and grow on demand.
 * Refused with EMAP_ERR_INVALID before anything is uploaded, launched or copied, host_out, *n_points, *point_step and the map
 * untouched: a NULL pointer; n_fields outside 1 .. EMAP_GRID_MAX_LAYERS; everything emap_publish_grid_map_ex refuses of an entry; an
 * unknown cloud or call flag; no or more than one POINT entry; HIDDEN without TEST or with POINT; a negative capacity_points; a
 * normal_min that is not finite with NORMAL_MIN; a row-strip context. */
enum { EMAP_CLOUD_POINT = 1, EMAP_CLOUD_TEST = 2, EMAP_CLOUD_HIDDEN = 4, EMAP_CLOUD_NORMAL_MIN = 8, EMAP_CLOUD_INDEX = 16 };
typedef struct emap_cloud_field { int32_t kind, index, flags, cloud_flags; } emap_cloud_field;
int emap_publish_point_cloud(emap_ctx* ctx, const emap_cloud_field* fields, int32_t n_fields, float center_z,
                             int32_t use_only_above_for_upper_bound, const float* x_of_i, const float* y_of_j, double normal_min,
                             int32_t call_flags, uint8_t* host_out, int64_t capacity_points, int64_t* n_points, int32_t* point_step);
/* Plane segmentation: the front of convex_plane_decomposition on ONE layer of the published map, on the device -- what
 * SlidingWindowPlaneExtractor::runExtraction (SlidingWindowPlaneExtractor.cpp:49-77) does with a downloaded GridMap:
 * runSlidingWindowDetector (:115-144: a plane fitted to the kernel_size^2 window of every cell with a finite height, :79-105, :19-41;
 * planar when the error and the inclination pass, :107-113; optionally an opening with a cross, :137-143), runSegmentation (:147-150:
 * connected components, connectivity 4 or 8), computePlaneParametersForLabel without RANSAC (:165-199 and the else branch :213-219: a
 * label with fewer than max(min_number_points_per_label, 3) finite cells gets no plane and keeps its cells; a label whose plane is
 * steeper than the inclination limit becomes background) and the verdict of isGloballyPlanar (:277-300) as needs_refinement.  RANSAC
 * itself, contours and the preprocessing are not part of it.  The contract -- a FIXED number of Jacobi sweeps, the order of the window
 * sums, the edge rule, the numbering, the fixed-point label moments -- is DESIGN.md section 21; grid_map's SlidingWindowIterator and
 * OpenCV's connectedComponents are restated there, not pinned by a compiled reference.
 * source: kind / index / flags as in emap_publish_grid_map_ex (slot is not read).  The index space is that door's: M = cell_n - 2 a
 * side, cell (i, j) at i * M + j.  params: angles arrive as COSINES and the caller computes them in double; origin_x / origin_y: the
 * position of cell (0, 0); a cell's point is (origin_x - i * resolution, origin_y - j * resolution, height).
 * host_labels: M * M int32, 0 = background, label = 1 + the rank of the component's first cell in row-major order (a rejected label
 * leaves a gap).  host_normals: NULL or 3 * M * M floats, the window normals (zero where the height is not finite).  host_planes:
 * one record per label that has a plane, in ascending label order; n_left_out: cells farther than 32 m from the label's first cell,
 * which the fixed-point moments leave out.  *n_labels: the components; *n_planes: the records.
 * Two waits: the chain up to the numbering, an 8-byte copy of the label and slot counts, a wait; the context sizes its slot buffer by
 * that count; moments, planes and final labels, the copies, a second wait.  If more than capacity_planes labels have a plane,
 * *n_labels, *n_planes, host_labels and host_normals are set, NO record is written and EMAP_ERR_INVALID is returned (a caller tells
 * it from a refusal by *n_planes > capacity_planes).  The buffers belong to the context and grow on demand.
 * Refused with EMAP_ERR_INVALID before anything is launched or copied, every output and the map untouched: a NULL pointer (host_normals
 * may be NULL); everything emap_publish_grid_map_ex refuses of an entry; kernel_size other than 3, 5, 7; connectivity other than 4, 8;
 * planarity_opening_filter outside 0 .. EMAP_PLANE_OPEN_MAX; min_number_points_per_label < 0; a resolution or threshold that is not
 * positive and finite; a cosine outside [-1, 1]; an origin or center_z that is not finite; a negative capacity_planes; a row-strip
 * context. */
enum { EMAP_PLANE_OPEN_MAX = 8 };
typedef struct emap_plane_params {
  int32_t kernel_size, planarity_opening_filter, min_number_points_per_label, connectivity, use_only_above_for_upper_bound, reserved;
  float center_z, reserved_f;
  double resolution, origin_x, origin_y, plane_patch_error_threshold, cos_local_plane_inclination, cos_plane_inclination,
         global_plane_fit_distance_error_threshold, cos_global_plane_fit_angle;
} emap_plane_params;
typedef struct emap_plane_record { int32_t label, n_points, needs_refinement, n_left_out; double support[3], normal[3]; } emap_plane_record;
int emap_plane_segmentation(emap_ctx* ctx, const emap_grid_layer_ex* source, const emap_plane_params* params, int32_t* host_labels,
                            float* host_normals, emap_plane_record* host_planes, int64_t capacity_planes, int32_t* n_labels,
                            int64_t* n_planes);
/* Planar terrain: what convex_plane_decomposition publishes around that segmentation, on the device, as one chain of launches --
 * GridMapPreprocessing::preprocess (GridMapPreprocessing.cpp:14-39) in front of it with terrain->preprocess = 1: minValues inpainting
 * (grid_map_filters_rsl inpainting.cpp:25-94: every NaN cell gets the smallest value that is not NaN around its 4-connected NaN
 * component) and a median (smoothing.cpp:23-42, cv::medianBlur: median_kernel_size is clamped to 1 .. 5 as :21 does, 1 is a no-op,
 * median_repeats passes, BORDER_REPLICATE); and Postprocessing::postprocess (Postprocessing.cpp:14-31) behind it: smooth_planar
 * (:73-144: the planar heights inpainted, closed with an ellipse, dilated with a slope of one cell height per cell, box mean,
 * Gaussian; the three smoothing sizes are HALF widths in metres, a kernel is 2 * int(round(size / resolution)) + 1 cells), the
 * elevation dilated in non-planar cells (:33-53, an ellipse of 2 * nonplanar_horizontal_offset + 1 cells, skipped at 0) and lifted
 * (:55-65), and support[2] of every record raised by extracted_planes_height_offset (:65-71).  The resampling step, RANSAC, contours
 * and convex regions are not part of it.  The contract -- minima, maxima and medians on the bits, the elliptic element, the SHIFTED
 * window of the sloped dilation, the summation order of the two means, one quiet NaN -- is DESIGN.md section 22; OpenCV and grid_map
 * are restated there, not pinned by a compiled reference.
 * source, params, host_labels .. n_planes: as emap_plane_segmentation; with preprocess = 0 they receive exactly what that call gives
 * (support[2] aside).  out->plane[k] receives plane k (M * M floats, cell (i, j) at i * M + j) if bit k of terrain->want is set and
 * is not touched otherwise: EMAP_TERRAIN_ELEVATION (the post-processed elevation), _SMOOTH_PLANAR, _CLASSIFICATION (1.0 where the
 * final label is not 0, else 0.0), _BEFORE (the elevation the segmentation read: preprocessed, or the source), and the reference's
 * helper layers elevationWithNaN, elevationWithNaN_i, elevationWithNaNClosed, elevationWithNaNClosedDilated.
 * Waits: the segmentation's two, and one behind the copies of the planes.  The buffers belong to the context and grow on demand.
 * Refused with EMAP_ERR_INVALID before anything is launched or copied, every output and the map untouched: everything
 * emap_plane_segmentation refuses; a NULL terrain or out; preprocess other than 0, 1; with preprocess an even median size after the
 * clamp or median_repeats outside 0 .. EMAP_TERRAIN_REPEATS_MAX; nonplanar_horizontal_offset outside 0 .. EMAP_TERRAIN_OFFSET_MAX; a
 * smoothing size that is negative or not finite; any kernel of more than EMAP_TERRAIN_KERNEL_MAX cells or more than M cells; a height
 * offset that is not finite; an unknown bit in want, or a set bit whose pointer is NULL. */
enum { EMAP_TERRAIN_KERNEL_MAX = 31, EMAP_TERRAIN_OFFSET_MAX = 15, EMAP_TERRAIN_REPEATS_MAX = 8, EMAP_TERRAIN_PLANES = 8 };
enum { EMAP_TERRAIN_ELEVATION = 1, EMAP_TERRAIN_SMOOTH_PLANAR = 2, EMAP_TERRAIN_CLASSIFICATION = 4, EMAP_TERRAIN_BEFORE = 8,
       EMAP_TERRAIN_WITH_NAN = 16, EMAP_TERRAIN_WITH_NAN_I = 32, EMAP_TERRAIN_CLOSED = 64, EMAP_TERRAIN_CLOSED_DILATED = 128,
       EMAP_TERRAIN_ALL = 255 };
typedef struct emap_terrain_params {
  int32_t preprocess, median_kernel_size, median_repeats, nonplanar_horizontal_offset, want, reserved;
  double smoothing_dilation_size, smoothing_box_kernel_size, smoothing_gauss_kernel_size, extracted_planes_height_offset,
         nonplanar_height_offset;
} emap_terrain_params;
typedef struct emap_terrain_planes { float* plane[8]; } emap_terrain_planes;
int emap_planar_terrain(emap_ctx* ctx, const emap_grid_layer_ex* source, const emap_plane_params* params,
                        const emap_terrain_params* terrain, int32_t* host_labels, float* host_normals, emap_plane_record* host_planes,
                        int64_t capacity_planes, int32_t* n_labels, int64_t* n_planes, const emap_terrain_planes* out);
/* Planar regions: the middle stage of the same pipeline, ContourExtraction::extractPlanarRegions (ContourExtraction.cpp:28-128), on
 * the device -- per connected piece of a label a boundary polygon with holes and its inset polygons, traced on the x 3 upsampled label
 * image (Upsampling.cpp:12-68; U = 3 * side - 2 pixels a side, never materialised on the host).  The answer is integer exact and a
 * function of the label plane alone.  The contract -- the upsampling rule, the all-label erosions with the margin ellipse of
 * 2 * (1 + margin_size) + 1 pixels and the 3 x 3 cross, the per-label fallback to the cross, 8-connected components, borders as cycles
 * of CRACKS, the vertex rule of CHAIN_APPROX_SIMPLE, the order of the answer -- is DESIGN.md section 23; OpenCV's erode / findContours
 * and CGAL's isInside are restated there, not pinned by a compiled reference.  RANSAC and convex region growing are not part of it.
 * host_labels: side * side int32 in 0 .. n_labels (0: background), uploaded and used; or NULL: the labels the last
 * emap_plane_segmentation / emap_planar_terrain left on this context (side must be 0 or cell_n - 2; n_labels is not read).
 * params->mode 0: regions.  mode 1: host_labels is a mask of 0 and 1 traced as it is (U = side; A is the mask, B its cross erosion with
 * the frame zeroed; margin_size is not read).
 * A crack is (pixel p, side s) with the index 4 * (row * U + column) + s: side 0 the top edge travelled west, 1 the left edge travelled
 * south, 2 the bottom edge travelled east, 3 the right edge travelled north.  host_rings: one record per border (ring), image 0 (the
 * boundaries, A) before image 1 (the insets, B), in ascending smallest crack within an image: first_vertex / n_vertices: its run of
 * host_vertices; is_hole: 0 for the outer ring of its component; label; root: the smallest pixel index of its 8-connected component;
 * crack: its smallest crack; boundary: the root of the image-0 component that holds the pixel `root`.  host_vertices: (x = column,
 * y = row) int32 pairs, in ring order, then in the order of travel from the ring's smallest crack on.
 * Three waits: the crack count; the ring and vertex counts; exactly the rings and vertices.  If a capacity is too small, *n_rings and
 * *n_vertices are set, nothing else is written and EMAP_ERR_INVALID is returned (a caller tells it from a refusal by the counts).  The
 * buffers belong to the context and grow on demand.
 * Refused with EMAP_ERR_INVALID before anything is uploaded, launched or copied, every output untouched: a NULL params, n_rings or
 * n_vertices, a NULL host_rings / host_vertices with a positive capacity, a negative capacity; an unknown mode; margin_size outside
 * 0 .. EMAP_REGION_MARGIN_MAX (mode 0); side < 2 or beyond EMAP_REGION_SIDE_MAX (mode 1: EMAP_REGION_RAW_SIDE_MAX): crack indices are
 * 32-bit; a label outside 0 .. n_labels, a negative n_labels, a mask value other than 0 and 1; NULL host_labels in mode 1, without
 * valid resident labels (none yet, or emap_clear / emap_shift since) or with a side that is not the map's; a row-strip context. */
enum { EMAP_REGION_MARGIN_MAX = 14, EMAP_REGION_SIDE_MAX = 7724, EMAP_REGION_RAW_SIDE_MAX = 23170 };
typedef struct emap_region_params { int32_t mode, margin_size, reserved[2]; } emap_region_params;
typedef struct emap_region_ring { int32_t first_vertex, n_vertices, image, is_hole, label, root, crack, boundary; } emap_region_ring;
int emap_planar_regions(emap_ctx* ctx, const int32_t* host_labels, int32_t side, int32_t n_labels, const emap_region_params* params,
                        emap_region_ring* host_rings, int64_t capacity_rings, int32_t* host_vertices, int64_t capacity_vertices,
                        int64_t* n_rings, int64_t* n_vertices);
/* ElevationMap.shift_map_xy / shift_map_z (EM/elevation_mapping.py:200-226): roll by (dx rows, dy cols) with
 * padding (0; variance plane initial_variance), planes 0 and 5 += dz -- as a rotation of the map's circular origin plus a pending
 * entry that later kernels replay: no cell is moved, only the entering band of the semantic layers is cleared.  Works on strips
 * (every rank calls it with the same arguments; a strip keeps its PHYSICAL rows, the logical rows it holds change). */
int emap_shift(emap_ctx* ctx, int32_t shift_rows, int32_t shift_cols, float dz);
/* first LOGICAL map row of the (row_count, cell_n) views emap_get_layer / emap_set_layer exchange (0 for a full map; a strip holds
 * the logical rows begin, begin + 1, ... modulo cell_n, which change with every row shift) */
int emap_strip_logical_begin(emap_ctx* ctx, int32_t* logical_row);

/* ---- RGB / semantic point-cloud fusion (EM/semantic_map.py:223-259; kernels EM/kernels/custom_semantic_kernels.py:
 * sum :9-51 + average :167-194 (kind 0) or class_average :233-267 (kind 1); add_color :270-317 + color_average :320-375;
 * kind 2 = class_bayesian (EM/fusion/pointcloud_class_bayesian.py:12-75: alpha kernel + renormalisation over the kind-2 layers
 * of the call, pseudo-counts persist in the "alpha" planes = the reference's new_map layers, semantic_map.py:54-56);
 * kind 3 = bayesian_inference (EM/fusion/pointcloud_bayesian_inference.py:12-122, restated literally).
 * Channel indices are column indices of the bound cloud (>= 3), layer indices address the semantic layer store. */
typedef struct emap_sem_spec {
  int32_t n_sum, sum_chan[16], sum_layer[16], sum_kind[16];
  int32_t n_col, col_chan[4], col_layer[4];
  double alpha; /* Parameter.average_weight */
} emap_sem_spec;
int emap_semantic_configure(emap_ctx* ctx, int32_t n_layers);                 /* SemanticMap.add_layer */
int emap_semantic_update(emap_ctx* ctx, const float R[9], const float t[3], const emap_sem_spec* spec); /* after emap_update */
/* semantic_map.update_layers_pointcloud as the reference runs it -- INSIDE update_map_with_kernel, between average_map_kernel and
 * clear_overlap_map (EM/elevation_mapping.py:366-368; EM/semantic_map.py:223-259): declares the fusion of the extra channels of
 * the bound cloud for the NEXT emap_update / emap_update_sharded call, which then fuses them before it returns (the declaration is
 * consumed by that one frame, also when the frame fails; spec_or_null == NULL or an empty spec withdraws it).  The layers hold what
 * an emap_semantic_update call after the frame would have left.  What the frame gains: a tile-binned frame without a visibility pass
 * whose fusions are average / class_average / at most one colour channel over at most four consecutive channel columns sorts 32-byte
 * records that carry those columns and fuses them in the tile pass that fuses the heights (no second pass over the records, no gather
 * of channel rows by point index, no count plane).  keep_counts != 0: the frame also leaves the per-cell accepted counts (new_map[2])
 * for a later emap_semantic_update / emap_semantic_class_max call on the same frame.  The spec is checked against the cloud that is
 * bound when the frame starts (EMAP_ERR_INVALID from that emap_update). */
int emap_frame_semantics(emap_ctx* ctx, const emap_sem_spec* spec_or_null, int32_t keep_counts);
int emap_semantic_get_layer(emap_ctx* ctx, int32_t layer, float* host_out);
int emap_semantic_set_layer(emap_ctx* ctx, int32_t layer, const float* host_in);
int emap_semantic_clear(emap_ctx* ctx);                                        /* SemanticMap.clear (layers only, :47-49) */

/* pointcloud_class_max (EM/fusion/pointcloud_class_max.py:80-126) on the bound cloud: channels chan[k] carry (half probability |
 * class id << 16) packed in a float, layer[k] the k-th of the fusion's layers (n_ch <= 8).  Per frame: sorted union of the ids in the
 * cloud and in the map's id planes; per (class, cell) the EXACT sum of the probabilities of the valid, inside points (64-bit integers
 * in units of 2^-24); per layer in turn the per-cell maximum over the classes and its id, the planes of all winning classes set to
 * zero before the next layer; the layers of a cell normalised by their sum.  The id planes are the layers' persistent planes
 * (emap_semantic_get_alpha returns them as uint32 bit patterns; they move with the map).  prev_unique / unique_out: the fusion's
 * unique_id array of the previous / this frame (n_prev = 0 before the first frame). */
int emap_semantic_class_max(emap_ctx* ctx, const float R[9], const float t[3], int32_t n_ch, const int32_t* chan, const int32_t* layer,
                            const uint32_t* prev_unique, int32_t n_prev, uint32_t* unique_out, int32_t unique_cap, int32_t* n_unique_out);
/* ---- the reference's semantic KERNEL FACTORIES on caller arrays (EM/kernels/custom_semantic_kernels.py) -------------------
 * Raw-array elementwise kernels over `size` elements; the points carry (cell index, valid, inside) in their first three columns
 * (what add_points_kernel leaves there, custom_kernels.py:260-262).  Host arrays in and out, for the staged / test surface
 * (compat/elevation_mapping_cupy/kernels); the per-frame path is emap_semantic_update.
 *   accumulate op: 0 sum_kernel (:9-51), 1 sum_compact_kernel (:54-86), 2 sum_max_kernel (:89-123), 3 alpha_kernel (:126-164),
 *                  4 add_color_kernel (:270-318; newmap_inout is the uint32 colour map of 3 n_ch + 1 planes)
 *   finalize op:   0 average_kernel (:167-194), 1 class_average_kernel (:233-267), 2 bayesian_inference_kernel (:197-230; newmap
 *                  = the variance planes, updated in place), 3 color_average_kernel (:320-375; newmap = the uint32 colour map)
 * new_elmap3: the (3, cells) planes the reference hands over, of which plane 2 (accepted points per cell) is read. */
int emap_semantic_accumulate(emap_ctx* ctx, int32_t op, const float* points, int64_t n_rows, int32_t stride, const int32_t* pcl_chan,
                             const int32_t* map_lay, int32_t n_ch, int64_t size, int64_t cells, void* newmap_inout, int32_t newmap_layers,
                             const float* max_pt, const int32_t* max_id, int32_t n_max);
int emap_semantic_finalize(emap_ctx* ctx, int32_t op, void* newmap_inout, int32_t newmap_layers, const int32_t* map_lay, int32_t n_ch, int64_t size,
                           int64_t cells, const float* new_elmap3, const float* sum_mean, int32_t sum_layers, float* map_inout, int32_t map_layers,
                           double alpha);
int emap_semantic_get_alpha(emap_ctx* ctx, int32_t layer, float* host_out);    /* SemanticMap.new_map[layer] of a class_bayesian layer */
int emap_semantic_set_alpha(emap_ctx* ctx, int32_t layer, const float* host_in);

/* MinFilter plugin (EM/plugins/min_filter.py:84-118): fills cells with valid < 0.5 by the window minimum of already
 * filled values, up to iteration_n sweeps, stops after the sweep that filled everything; NaN where still unfilled.
 * Planes are (cell_n, cell_n) host buffers handed to the plugin (PluginBase.__call__ convention); with both inputs NULL the
 * map's own elevation / is_valid planes are taken on the device (the built-in plugin: only the result crosses PCIe). */
int emap_min_filter(emap_ctx* ctx, const float* host_elevation, const float* host_valid, int32_t dilation_size,
                    int32_t iteration_n, float* host_out, int32_t* sweeps_run_or_null);

/* MaxFilter plugin (EM/plugins/max_filter.py:36-112): same sweep structure with the window maximum; a cell is filled while its
 * running mask is < 0.5 and the reference itself runs this one out of place. */
int emap_max_filter(emap_ctx* ctx, const float* host_elevation, const float* host_valid, int32_t dilation_size,
                    int32_t iteration_n, float* host_out, int32_t* sweeps_run_or_null);
/* SmoothFilter plugin (EM/plugins/smooth_filter.py:56-58): `passes` applications of a 3x3 uniform filter with the semantics of
 * scipy.ndimage.uniform_filter(size=3) ('reflect' borders, separable, float32 intermediate); the plugin uses passes = 2. */
int emap_smooth_filter(emap_ctx* ctx, const float* host_in, int32_t passes, float* host_out);

/* Erosion plugin (EM/plugins/erosion.py:96-104): what its cv2.erode(img, ones((k, k)), iterations=n) call computes -- the k x k
 * window minimum (anchor k/2, pixels outside the image ignored), n times.  OpenCV is third-party and absent: parity unpinned. */
int emap_erode(emap_ctx* ctx, const float* host_in, int32_t kernel_size, int32_t iterations, float* host_out);

/* ---- publish-time plugins on device-resident planes --------------------------------------------------------------------------------
 * The reference keeps every plugin's output in PluginManager.layers, a (n_plugins, cell_n, cell_n) array on ITS device
 * (EM/plugins/plugin_manager.py:130, :181-236), and a plugin reads the others' outputs there.  The context owns the same: up to
 * EMAP_PLUGIN_MAX_PLANES planes of cell_n x cell_n floats, each the RAW output of a plugin (logical row-major order, border included,
 * unflipped).  Single-strip contexts only.
 * emap_plugin_planes: reserve n planes, 0 .. 32.  New planes are zero (as PluginManager.layers starts); growing keeps the existing ones.
 * emap_plugin_plane_write: host array -> plane, enqueued behind what the stream holds, no wait for the device.  host_in is ordinary
 *   (pageable) memory: the runtime stages such a copy before hipMemcpyAsync returns, and on that the rule rests that the host array
 *   may be reused when the call returns -- a caller who hands in pinned memory must keep it unchanged until the next call that waits.
 * emap_plugin_plane_read: plane -> host array, returns when host_out is filled (and with it everything enqueued before). */
#define EMAP_PLUGIN_MAX_PLANES 32
int emap_plugin_planes(emap_ctx* ctx, int32_t n_planes);
int emap_plugin_plane_write(emap_ctx* ctx, int32_t plane, const float* host_in);
int emap_plugin_plane_read(emap_ctx* ctx, int32_t plane, float* host_out);
/* emap_plugin_chain: n_ops (1 .. EMAP_PLUGIN_MAX_OPS) plugins, run in order on the context's stream into their dst_plane.  ENQUEUES
 * and does NOT wait: emap_publish_grid_map_ex (kind EMAP_GRID_PLUGIN) or emap_plugin_plane_read behind it see the results.  A pending
 * map shift is written out first.  Each op restates the plugin's own arithmetic bit for bit:
 *   EMAP_PLUGIN_MIN_FILTER / _MAX_FILTER (EM/plugins/min_filter.py:84-118, max_filter.py:36-112): i0 = dilation_size 0 .. 32, i1 =
 *     iteration_n 0 .. 4096, on the map's own elevation / is_valid as emap_min_filter with NULL inputs (device-side early exit); the
 *     plane gets mask > 0.5 ? value : NaN.  The sweeps a chain ran are not reported (nothing waits).  src_* ignored.
 *   EMAP_PLUGIN_SMOOTH (EM/plugins/smooth_filter.py:56-58): uniform_filter(size=3) twice, as emap_smooth_filter with passes = 2.
 *   EMAP_PLUGIN_EROSION (EM/plugins/erosion.py:60-113): i0 = kernel_size 1 .. 63, i1 = iterations 0 .. 256, flag EMAP_PLUGIN_REVERSE
 *     (1 - layer before and after): lo / hi of the layer on the device, ((layer - lo) * 255 / (hi - lo)) truncated to 8 bits, emap_erode's
 *     window minimum, q * (hi - lo) / 255 + lo.  A layer with hi <= lo or with a NaN is returned as it came (under REVERSE as 1 - (1 - x), the
 *     plugin's own double reversal).
 *   EMAP_PLUGIN_ROBOT_CENTRIC (EM/plugins/robot_centric_elevation.py:54-57, :96-118): (R6 rx + R7 ry) + R8 h on valid cells, rx =
 *     (float)row * (float)resolution, rotation9 row-major; flag EMAP_PLUGIN_THRESHOLD: 1 / 0 for z >= f0 instead.  src_* ignored.
 *   EMAP_PLUGIN_INPAINT_FRONTS (plugins/inpainting.py, method "telea_fronts"; EM/plugins/inpainting.py:53-61 around the fill): on the map's
 *     own RAW elevation / is_valid, src_* ignored.  known = is_valid >= 0.5 (>=: this plugin's own comparison).  With no known cell, or
 *     with every cell known, the plane is the elevation as it is.  Otherwise h_min / h_max over the known cells (on the device), span =
 *     (float)((double)h_max - (double)h_min) if h_max > h_min else 1, the image clip((h - h_min) * 255 / span, 0, 255) truncated to 8
 *     bits (every operation rounded to float32), the fill of emap_inpaint_telea_fronts_u8 with radius 1 on (image, !known) without its
 *     copies and without its read-back -- ceil((2 cell_n - 2) / S) launches of S fronts, the geometric bound of the L1 distance, instead
 *     of ceil(max d / S); the launches behind the last front do nothing -- and (float)out * span / 255 + h_min in three roundings.  i0 =
 *     fronts per launch S, 1 .. 16, or 0 for the default (16); the plane does not depend on it.  i1 must be 0, f0 is ignored, no flag.
 *     The fronts run is not reported (nothing waits).  The elevation is assumed finite in every cell: the cast of a NaN to 8 bits is
 *     undefined on the plugin's host route as well, and no rule is made up for it here.
 * src_kind EMAP_PLUGIN_SRC_LAYER: src_index = RAW map layer 0 .. 6 (elevation, variance, is_valid, traversability, time, upper_bound,
 * is_upper_bound: emap_get_layer's planes); EMAP_PLUGIN_SRC_PLANE: a resident plane -- as it is when the op runs, i.e. what an earlier
 * op of the chain or an earlier call left.  Refused with EMAP_ERR_INVALID before anything is enqueued, planes and map untouched: a NULL
 * pointer (rotation9 may be NULL without a ROBOT_CENTRIC op), n_ops outside 1 .. 32, an unknown type / src_kind / flag, a plane outside
 * the reservation, a SMOOTH whose source is its own dst_plane, sizes outside the bounds above, a row-strip context.  Every op of a chain
 * has scratch of its own in the context (two inpaint ops share no image, distance plane or range record). */
#define EMAP_PLUGIN_MAX_OPS 32
enum { EMAP_PLUGIN_MIN_FILTER = 0, EMAP_PLUGIN_MAX_FILTER = 1, EMAP_PLUGIN_SMOOTH = 2, EMAP_PLUGIN_EROSION = 3, EMAP_PLUGIN_ROBOT_CENTRIC = 4,
       EMAP_PLUGIN_INPAINT_FRONTS = 6 };      /* (5 is unassigned and refused) */
enum { EMAP_PLUGIN_SRC_LAYER = 0, EMAP_PLUGIN_SRC_PLANE = 1 };
enum { EMAP_PLUGIN_REVERSE = 1, EMAP_PLUGIN_THRESHOLD = 2 };
typedef struct emap_plugin_op { int32_t type, dst_plane, src_kind, src_index, i0, i1, flags; float f0; } emap_plugin_op;
int emap_plugin_chain(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9);
/* emap_plugin_chain_ex: emap_plugin_chain with a side table of sources, for the ops that read SEVERAL layers -- the reference's four
 * semantic plugins.  For such an op src_kind is ignored, src_index is the first entry of the op's run in srcs[0 .. n_srcs) and i0 the
 * number of entries; i1 must be 0 and f0 is ignored.  An entry names its layer by kind / index -- EMAP_PLUGIN_SRC_LAYER (RAW map layer
 * 0 .. 6), EMAP_PLUGIN_SRC_PLANE (resident plane, as it is when the op runs) or EMAP_PLUGIN_SRC_SEMANTIC (semantic layer `index`, read at
 * the logical cell: the plane emap_semantic_get_layer returns) -- and carries the op's per-source flags and constants.  The table is read
 * during the call (it travels in the kernels' arguments): the caller's array need not outlive it.  emap_plugin_chain is this call with
 * an empty table; it refuses the four types below and names emap_plugin_chain_ex.  For the ops of emap_plugin_chain src_kind stays 0 or 1.
 * Every op leaves, bit for bit, what the plugin's __call__ leaves in the float32 host array under NumPy 2 (NEP 50: a Python float beside a
 * float32 array stays float32, a NumPy float64 scalar widens the operation to double):
 *   EMAP_PLUGIN_SEMANTIC_FILTER (EM/plugins/semantic_filter.py:112-133): 0 .. 64 sources, in the order map layers, plugin layers, semantic
 *     layers.  id = argmax over the sources (:128) as np.argmax takes it: the first NaN wins, otherwise the first maximum, -0 == +0.  The
 *     plane is the colour of id (:132; table entry id + 1, :42-62): the bits of id + 1 dealt round-robin to r, g, b from the top bit down
 *     (bit 3 j + ch of the index -> bit 7 - j of channel ch), entries 1 and 2 = (81, 113, 162), entry 3 = (188, 63, 59), packed 0x00RRGGBB
 *     as the float's bits.  Computed in the kernel: no table is uploaded.  0 sources: the colour of id 0 everywhere.  No source flag.
 *   EMAP_PLUGIN_SEMANTIC_TRAV (EM/plugins/semantic_traversability.py:70-82): 1 .. 16 sources, map layers or planes, d0 = the threshold.  A
 *     source votes where layer >= d0, with flag EMAP_PLUGIN_SRC_AT_MOST (type "traversability") where layer <= d0 (:76, :79).  The plugin
 *     keeps its thresholds as NumPy float64 scalars, so the comparison is (double)layer vs d0: 0.3f <= 0.3 is false.  A NaN never votes.
 *     The plane is 1.0f where at least one source voted and 0.1f elsewhere (:81: the vote sum is a small integer, <= 0.9 means 0; the
 *     double 0.1 is cast to float32 when the plane is stored).
 *   EMAP_PLUGIN_MAX_LAYER (EM/plugins/max_layer_filter.py:66-108): 1 .. 16 sources of any kind.  Per source, in the plugin's order: flag
 *     EMAP_PLUGIN_SRC_ZERO_DEFAULT: x == 0 ? f0 : x (:75; float32: f0 is float(default_value) rounded to float32; -0 counts as 0);
 *     EMAP_PLUGIN_SRC_REVERSE: 1.0f - x (:88); EMAP_PLUGIN_SRC_SCALE: x * f1 (:90, float32); EMAP_PLUGIN_SRC_THRESHOLD: x > (float)d0 ? 1 : 0
 *     (:92, float32 comparison; a NaN gives 0).  Then the maximum, with op flag EMAP_PLUGIN_MIN the minimum, over the sources in table
 *     order as np.max / np.min reduce a stack along its first axis: any NaN gives NaN; among equal values the LATER source is kept (acc > x ?
 *     acc : x), which decides the sign of a zero.  np.stack widens a mix of thresholded (int64) and other (float32) layers to float64
 *     and the plane is cast back to float32 when stored: float32 -> float64 -> float32 changes no value, so the op stays in float32.
 *   EMAP_PLUGIN_FEATURES_PCA (EM/plugins/features_pca.py:66-96): 3 .. 16 sources of any kind, no source flag.  In double on x clipped to
 *     [-1, 1] (:74): per-feature means; the F x F matrix of centred second moments in a second pass; its eigenvectors by cyclic Jacobi in
 *     one workgroup; eigenvalues sorted descending, the three leading eigenvectors kept, each signed so that its entry of largest
 *     magnitude is positive (the first among equals: sklearn's v-based svd_flip, :80); scores (x - mean) . v; lo / hi per component
 *     over the map (:84-85), span = hi > lo ? hi - lo : 1; level = (uint8)((score - lo) / span * 255) by truncation (:88), packed
 *     0x00RRGGBB.  Every reduction is order-fixed (per-workgroup partials, then a fold): two runs give the same bits.  The definition is
 *     pinned, the last ulp of an eigenvector is not: against the host's SVD a level may differ by 1 in a few cells.
 * Refused before anything is enqueued, beyond emap_plugin_chain's cases: srcs NULL with n_srcs != 0, n_srcs outside 0 .. 2048, a run
 * outside the table, a count outside the op's limits, a kind outside 0 .. 2 (SEMANTIC_TRAV: outside 0 .. 1), a map layer outside 0 .. 6, a
 * semantic index >= the configured semantic layers, a plane outside the reservation, a source that is the op's own dst_plane, a source
 * flag the op does not know, reserved != 0, i1 != 0. */
enum { EMAP_PLUGIN_SEMANTIC_FILTER = 7, EMAP_PLUGIN_SEMANTIC_TRAV = 8, EMAP_PLUGIN_MAX_LAYER = 9, EMAP_PLUGIN_FEATURES_PCA = 10 };
enum { EMAP_PLUGIN_SRC_SEMANTIC = 2 };
enum { EMAP_PLUGIN_MIN = 4 };                    /* op flag of MAX_LAYER (beside EMAP_PLUGIN_REVERSE / _THRESHOLD of the other ops) */
enum { EMAP_PLUGIN_SRC_AT_MOST = 1, EMAP_PLUGIN_SRC_ZERO_DEFAULT = 2, EMAP_PLUGIN_SRC_REVERSE = 4, EMAP_PLUGIN_SRC_SCALE = 8, EMAP_PLUGIN_SRC_THRESHOLD = 16 };
#define EMAP_PLUGIN_MAX_SRCS 2048                /* entries of one side table: 32 ops x 64 */
typedef struct emap_plugin_src { int32_t kind, index, flags, reserved; float f0, f1; double d0; } emap_plugin_src;
int emap_plugin_chain_ex(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, int32_t n_srcs);

/* Inpainting plugin (EM/plugins/inpainting.py:53-61) -- DOCUMENTED SUBSTITUTE for the OpenCV Telea call it makes: fills
 * the pixels with known == 0 of a (cell_n, cell_n) image holding 8-bit values, front by front, with the distance-weighted
 * mean of the known 8-neighbours. Values stay in [0, 255], integers. */
int emap_inpaint_u8(emap_ctx* ctx, const float* host_image, const float* host_known, int32_t max_sweeps, float* host_out,
                    int32_t* sweeps_run_or_null);
/* Inpainting plugin, method "telea" (EM/plugins/inpainting.py:59: cv2.inpaint(h, mask, 1, cv2.INPAINT_TELEA) on the host): Telea's
 * fast-marching fill of the pixels with mask != 0 in an 8-bit image, HOST arrays in and out, no context needed -- a serial
 * priority-queue algorithm that the reference also runs on the CPU.  A restatement of the published algorithm (OpenCV is absent
 * offline: parity with its values is not pinned).  Images of fewer than 2 x 2 pixels are rejected (EMAP_ERR_INVALID), as by
 * emap_inpaint_ns_u8: the clamped neighbour rows / columns of the image-gradient term need two of each. */
int emap_inpaint_telea_u8(const uint8_t* image, const uint8_t* mask, int32_t rows, int32_t cols, int32_t radius, uint8_t* out);
/* Inpainting plugin, method "ns" (EM/plugins/inpainting.py:33-38,59: cv2.inpaint(h, mask, 1, cv2.INPAINT_NS) on the host): the
   Navier-Stokes based fill in its fast-marching form -- same march as above, a pixel = mean of the known pixels within `radius`
   weighted along the isophote direction (csrc/emap_inpaint_ns.cpp).  HOST code, no context, same arguments and errors as
   emap_inpaint_telea_u8; images of fewer than 2 x 2 pixels are rejected (EMAP_ERR_INVALID).  Parity with OpenCV's values is NOT pinned
   (OpenCV absent offline); pinned against oracle/ns_inpaint.py. */
int emap_inpaint_ns_u8(const uint8_t* image, const uint8_t* mask, int32_t rows, int32_t cols, int32_t radius, uint8_t* out);
/* Inpainting plugin, method "telea_fronts": Telea's estimator ON THE GPU, scheduled by fronts (csrc/emap_inpaint_fronts.hip, DESIGN.md
 * §8).  d(p) = L1 distance from p to the nearest pixel with mask == 0; fronts k = 1 .. max d are filled in order, every pixel of front k
 * at once, with the float32 arithmetic of emap_inpaint_telea_u8 (radius 1) in which "known" means d(q) < k (the 1-pixel frame around
 * the image counts as known), pixels with d >= k read as T = 1e6 with their input value, and a known pixel 4-adjacent to the hole starts
 * at T = -0.0f.  Deterministic and exactly specified (tests/_telea_fronts.py restates it); NOT equal to the serial host march, whose
 * order is that of a priority queue (agreement measured in tests/test_inpaint_fronts.py).  HOST arrays in and out, like
 * emap_inpaint_telea_u8; known pixels are returned unchanged; no known pixel or nothing to fill: out = image, *fronts_run = 0.
 * Otherwise *fronts_run (may be NULL) = max d.  radius != 1, images of fewer than 2 x 2 pixels, NULL pointers: EMAP_ERR_INVALID.
 * An inpainter is created on `device` (-1: the calling thread's current device) and enqueues on `stream` (a hipStream_t, NULL = the null stream); it keeps its device scratch,
 * grown to the largest image seen, until destroyed.  Calls on one inpainter are serialised by the caller; each call returns after
 * the stream has delivered `out`.  The stream is the caller's: it is used only inside emap_inpaint_telea_fronts_u8 and must be valid
 * during each such call; emap_inpainter_destroy does not touch it.  emap_inpainter_set_steps: fronts advanced per launch (1 .. 16,
 * default 16; results do not depend on it). */
typedef struct emap_inpainter emap_inpainter;
int emap_inpainter_create(int32_t device, void* stream, emap_inpainter** out);
int emap_inpainter_destroy(emap_inpainter* ip);
int emap_inpainter_set_steps(emap_inpainter* ip, int32_t steps);
int emap_inpaint_telea_fronts_u8(emap_inpainter* ip, const uint8_t* image, const uint8_t* mask, int32_t rows, int32_t cols,
                                 int32_t radius, uint8_t* out, int32_t* fronts_run);

/* ---- camera path: ElevationMap.input_image (EM/elevation_mapping.py:468-562).
 * emap_image_correspondence = image_to_map_correspondence_kernel (EM/kernels/custom_image_kernels.py:9-157): x1, y1 = camera
 * cell (integer valued, see GUARD), z1 = camera height above the map centre, P = K [R|t] row major, D = 5 radtan coefficients (all 0 =
 * none).  emap_image_fuse = exponential_ (kind 0, alpha 0.7 in the reference) / color_ (kind 1, planes 0..2 = r,g,b) / average_
 * (kind 2: the sample replaces the value, :160-192) correspondences_to_map_kernel applied to semantic layer `layer` with a host image
 * (n_planes, H, W) float32.  emap_image_set_tolerance = the factory parameter tolerance_z_collision of the occlusion walk (:9; the
 * reference's only call passes 0.10, the default).  emap_image_fuse_arrays = the same three kernels on caller arrays (one
 * (cell_n, cell_n) semantic plane in, one out, uv (2, cell_n, cell_n), valid (cell_n, cell_n) bytes): what the kernel factories bind.
 * GUARD (a departure from the reference, whose kernel does not terminate there): the occlusion walk ends only by REACHING the camera
 * cell, so emap_image_correspondence returns EMAP_ERR_INVALID, before anything is launched and with the previous correspondence
 * untouched, when x1 or y1 is not finite, not integer valued, or beyond 65536 cells in magnitude (a cap, not a measurement: 2.6 km at
 * 4 cm cells).  A NEGATIVE integer cell is valid: a camera on the low side of the map, walked like one beyond the high side.  The
 * reference casts the cell through uint32, which wraps such a pose to about 2^32; ElevationMap.input_image computes a signed index
 * instead (camera_cell) and raises ValueError beyond the same cap. */
int emap_image_correspondence(emap_ctx* ctx, float x1, float y1, float z1, const float P[12], const float K[9], const float D[5],
                              float image_height, float image_width, const float center[3]);
int emap_image_get_correspondence(emap_ctx* ctx, float* uv_host /* (2, cell_n, cell_n) */, uint8_t* valid_host);
int emap_image_fuse(emap_ctx* ctx, int32_t kind, int32_t layer, const float* host_image, int32_t n_planes, int32_t height,
                    int32_t width, double alpha);
int emap_image_set_tolerance(emap_ctx* ctx, double tolerance_z_collision);
int emap_image_fuse_arrays(emap_ctx* ctx, int32_t kind, const float* sem_plane, const float* host_image, int32_t n_planes, int32_t height,
                           int32_t width, const float* uv, const uint8_t* valid, double alpha, float* out_plane);
/* Image message input: one camera frame from the BYTES of a sensor_msgs/Image, in one launch.  The reference's node converts the
 * message on the host (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:375-446: cvtColor for bgr8 / bgra8, cv::split, cv2eigen
 * into one float matrix per channel), input_image uploads the float stack and launches the correspondence kernel and one sampling
 * kernel per channel; here the message's bytes are uploaded as they are and ONE kernel computes the correspondence (written where
 * emap_image_get_correspondence reads it) and, per visible cell, walks the entry table in order, sampling the bytes on the device.
 * The result is bit for bit what emap_image_correspondence + one emap_image_fuse per entry leave for the planes defined below.
 * Message: height * step bytes; pixel (v, u) starts at byte v * step + u * n_chan * size(elem); padding bytes are never read.
 * elem: the OpenCV depth code, 0 8U 1 8S 2 16U 3 16S 4 32S 5 32F 6 64F.  Plane p of pixel (v, u) is message channel c of that pixel,
 * c = 2 - p if swap_rb and p is 0 or 2 (the node's BGR -> RGB for bgr8 / bgra8), else c = p; loaded at the element's width in the
 * message's byte order (is_bigendian), alignment safe (step may be odd), and converted to float32 with ONE C conversion, round to
 * nearest even, subnormals kept; a float64 beyond float32 becomes +-inf; a NaN stays a NaN (its payload is not part of the contract);
 * a 32F element is moved.
 * specs: 1 .. 4 entries, applied in order inside each visible cell: kind 0 exponential (alpha), 1 colour (planes 0, 1, 2 = r, g, b; plane
 * is ignored), 2 average (the sample replaces the value); layer: the semantic layer; plane: the plane sampled (kinds 0, 2).
 * Refused with EMAP_ERR_INVALID before anything is copied or launched, correspondence and layers untouched: a NULL pointer; a camera
 * cell emap_image_correspondence refuses; a row-strip context; height or width outside 1 .. 8192; step < width * n_chan * size(elem);
 * height * step >= 2^31; an unknown elem; n_chan outside 1 .. 4; n_specs outside 1 .. 4; a kind outside 0 .. 2; a layer that is not
 * configured; plane < 0 or >= n_chan; a colour entry or swap_rb with n_chan < 3; height * width * (3 with a colour entry, else 1) > 2^24 (beyond
 * it the reference's float index arithmetic is no longer exact: emap_image_fuse remains for such images).
 * The caller's bytes are only borrowed (copied into a pinned slot of the camera path's own before the call returns; a message of more
 * than 2 MB by the upload's worker threads, chunk by chunk); the bound cloud stays bound; nothing waits for the device. */
typedef struct emap_image_msg_desc { int32_t height, width, step, elem, n_chan, is_bigendian, swap_rb; } emap_image_msg_desc;
typedef struct emap_image_spec { int32_t kind, layer, plane, pad; double alpha; } emap_image_spec;
int emap_input_image_message(emap_ctx* ctx, const emap_image_msg_desc* desc, const uint8_t* data, float x1, float y1, float z1,
                             const float P[12], const float K[9], const float D[5], const float center[3],
                             const emap_image_spec* specs, int32_t n_specs);

/* ---- safety-polygon service: polygon_mask_kernel (EM/kernels/custom_kernels.py:509-651) as launched by
 * ElevationMap.get_polygon_traversability (EM/elevation_mapping.py:837-889).  `polygon_xy` = (n, 2) float32 world
 * coordinates already clipped to the map (:851-855); writes the (cell_n, cell_n) 0/1 mask to host memory. */
int emap_polygon_mask(emap_ctx* ctx, const float* polygon_xy, int32_t n_vertices, float center_x, float center_y, float* host_mask);

/* ---- safety-polygon service on the device: what ElevationMap.get_polygon_traversability (EM/elevation_mapping.py:837-889)
 * reduces from the mask of polygon_mask_kernel (EM/kernels/custom_kernels.py:509-651), the checker layer and is_valid, for a
 * BATCH of footprints in one call: one upload, two launches, one copy back of a few hundred bytes per polygon, one wait.
 * No mask is written and no plane is downloaded.
 *
 * `polygons_xy`: the vertices of all polygons one behind the other, (x, y) float32 world coordinates already clipped to the
 * map (:851-855) as for emap_polygon_mask; polygon p holds the vertices vertex_begin[p] .. vertex_begin[p + 1] - 1
 * (vertex_begin[0] = 0, increasing).  The checker value of a cell is read where it lies: layer_kind EMAP_POLY_MAP_LAYER = raw
 * map layer `layer_index` 0 .. 6 (emap_get_layer), EMAP_POLY_SEMANTIC = semantic layer `layer_index`, EMAP_POLY_PLUGIN =
 * resident plugin plane `layer_index` (emap_plugin_chain).  A cell inside a polygon has risk = is_valid > 0.5 ? 1 - value : 0
 * in float32; it is risky when risk > risky_above (the float32 of 1 - safe_thresh).  Only the interior rows and columns
 * 1 .. cell_n - 2 count.
 *
 * verdicts[p]: n_inside cells inside, sum_valid = the sum of is_valid over them and sum_risk = the sum of risk, both in
 * double and in a fixed order (the same bytes wherever the polygon stands in a batch); n_risky; max_risk over the interior
 * (a cell outside a polygon counts 0).  flags bit 0: a NaN risk inside; bit 1: a known cell ANYWHERE in the interior whose
 * risk is not finite -- the reference multiplies the risk plane by the mask, so such a cell outside the polygon is
 * inf * 0 = NaN in its sum and maximum; either bit makes sum_risk and max_risk NaN.  row_begin, n_rows, col_begin, n_cols:
 * the polygon's bounding box in cells, clipped to the interior.
 *
 * row_extremes: for row q of polygon p's box (logical row row_begin + q) the smallest and the largest column of a risky cell
 * at row_extremes[2 * (row_extremes_begin[p] + q)] and the word behind it, both -1 when the row has none -- the convex hull
 * of the risky cells is the hull of these at most 2 n_rows cells.  row_extremes_begin[p + 1] - row_extremes_begin[p] rows
 * are the caller's room for polygon p (cell_n - 2 always suffice); rows beyond n_rows are not written.
 *
 * Refused before any device is touched: null pointers, n_polygons outside 1 .. EMAP_POLY_MAX_BATCH, a polygon with fewer than
 * 1 or more than EMAP_POLY_MAX_VERTS vertices, vertex_begin not increasing from 0, an unknown layer kind or an index outside
 * its kind, a plugin plane that is not reserved, a strip context, too little room for a polygon's rows, and a batch of more
 * than EMAP_POLY_MAX_TILES tiles of 32 x 32 cells.  The three limits are caps, not measurements: they bound the context's
 * scratch (a part record of 288 bytes per tile), nothing in the kernels depends on them but the vertex stage in LDS. */
#define EMAP_POLY_MAX_BATCH 4096
#define EMAP_POLY_MAX_VERTS 256
#define EMAP_POLY_MAX_TILES 262144
#define EMAP_POLY_MAP_LAYER 0
#define EMAP_POLY_SEMANTIC 1
#define EMAP_POLY_PLUGIN 3
#define EMAP_POLY_HAS_NAN 1
#define EMAP_POLY_POISON 2
typedef struct emap_polygon_verdict { double sum_valid, sum_risk; float max_risk; int32_t n_inside, n_risky, flags, row_begin, n_rows, col_begin, n_cols; } emap_polygon_verdict;
int emap_polygon_safety(emap_ctx* ctx, const float* polygons_xy, const int32_t* vertex_begin /* n_polygons + 1 */, int32_t n_polygons,
                        float center_x, float center_y, int32_t layer_kind, int32_t layer_index, float risky_above,
                        emap_polygon_verdict* verdicts, int32_t* row_extremes, const int64_t* row_extremes_begin /* n_polygons + 1 */);

/* dilation_filter_kernel (EM/kernels/custom_kernels.py:392-449) on host planes (cell_n x cell_n), `iterations` out-of-place
 * passes -- the two passes of ElevationMap.initialize_map (EM/elevation_mapping.py:914-921; in place, i.e. racy, there). */
int emap_dilate_planes(emap_ctx* ctx, const float* host_plane, const float* host_mask, int32_t dilation_size, int32_t iterations,
                       float* host_out, float* host_out_mask);

/* ---- row-strip halos (multi-GPU; exchange itself is done by the caller, e.g. torch.distributed/RCCL) ---- */
/* pack `halo_rows` owned boundary rows next to the lower (side 0) / upper (side 1) neighbour into a device buffer; unpack a
 * neighbour's rows into the halo.  Only what the stencils read of a halo row travels: the 16-byte cold half cells (time,
 * upper_bound, is_upper_bound, is_valid).  Buffers: halo_rows*cell_n*4 floats (emap_halo_bytes). */
int emap_halo_bytes(emap_ctx* ctx, int64_t* bytes_per_side);
int emap_halo_pack(emap_ctx* ctx, int side, float* dev_buf);
int emap_halo_unpack(emap_ctx* ctx, int side, const float* dev_buf);
/* The strips are physical row ranges of a circular map: neighbours form a RING (rank 0's lower neighbour is the last rank).
 * After a row shift the normal planes (not shifted in the reference) lag the cells by emap_normal_row_lag rows; when that is not
 * 0 and the visibility pass is on, the callers exchange the planes' boundary rows too (3 x halo_rows x cell_n floats per side)
 * before emap_rays.  emap_update_sharded does both by itself. */
int emap_normal_row_lag(emap_ctx* ctx, int32_t* lag);
int emap_normal_halo_pack(emap_ctx* ctx, int side, float* dev_buf);
int emap_normal_halo_unpack(emap_ctx* ctx, int side, const float* dev_buf);
/* Row strips after a ROW shift of more than halo_rows: which rank's normal rows each rank's cells belong to (emap_update_sharded
 * fetches them itself, emap_api_comm.hip: normal_exchange; EM/elevation_mapping.py:200-214 -- normal_map is not shifted with the map).  Pure
 * host arithmetic, exposed for tests and for callers that drive the exchange themselves: rank q needs physical rows [src, src + rows),
 * owned by rank r, as rows [dst, dst + rows) of its row-aligned copy; pieces5 = {q, r, src, dst, rows} per piece, in posting order. */
int emap_normal_lag_plan(int32_t cell_n, int32_t world, const int32_t* cut_begin, const int32_t* cut_count, int32_t lag,
                         int32_t* pieces5, int32_t max_pieces, int32_t* n_pieces);

/* ---- row-strip communicator: one process per GPU, RCCL over xGMI issued from the library itself -------------
 * Nothing like it exists in the reference (single GPU).  `rccl_path` names the RCCL shared object to dlopen (NULL =
 * "librccl.so.1" from the loader path); rank 0 creates the 128-byte ncclUniqueId, the caller distributes it (any
 * bootstrap channel) and every rank calls emap_comm_init -- a collective call.  emap_update_sharded is emap_update for a
 * strip: count -> all-reduce(2 x f64 drift sums) -> gate -> fuse [-> commit -> rays] -> average -> overlap clearance ->
 * halo exchange of the boundary rows (in place, on a second stream) overlapped with the interior stencil tiles ->
 * boundary stencil tiles.  emap_comm_selftest checks an all-reduce and a send/recv round trip on the hardware.
 * emap_comm_init (world <= 16) also gathers every rank's rows (who holds which normal rows after a map shift), allocates the ray window
 * of a frame that marches its rays by ray -- so that no rank can fail alone in the middle of a frame's collectives -- and makes the
 * ranks agree on EMAP_ABI_VERSION. */
int emap_comm_unique_id(const char* rccl_path, uint8_t id_out[128]);
int emap_comm_init(emap_ctx* ctx, const char* rccl_path, const uint8_t id[128], int32_t rank, int32_t world);
int emap_comm_destroy(emap_ctx* ctx);
int emap_comm_selftest(emap_ctx* ctx);
/* number of ranks RCCL itself reports for the communicator (ncclCommCount): what a launcher prints as evidence that the
 * strips really talk through one RCCL communicator of that size */
int emap_comm_count(emap_ctx* ctx, int32_t* ranks);
/* bytes THIS rank sent + received in the exchange steps of the last frame's visibility pass when it marched BY RAY; 0 for a frame that
 * marched by row.  Round 6: the window records (32 B per window cell) are broadcast by the owners of its rows and the effects (20 B
 * per cell) are reduced to them -- grouped ncclSend / ncclRecv, an owner then folds the parts it received (k_win_reduce); an owner of
 * a share f of the window moves (W - 1) f (32 + 20) + (1 - f) (32 + 20) bytes per cell, a rank that owns none of it 52.  With
 * EMAP_BYRAY_ALLREDUCE=1, or strips that do not tile the map: the three all-reduces of rounds 4 / 5 (52 B per cell of payload on
 * every rank, moved 2 (W - 1) / W times by a ring). */
int emap_comm_wire_bytes(emap_ctx* ctx, uint64_t* bytes);
/* out-of-band reductions over the ranks through the communicator itself (barriers and timing reductions of a launcher:
 * no second bootstrap channel needed once RCCL is up): all-reduce of n <= 16 host doubles, op 0 = sum, 1 = max, in place;
 * blocks until the result is back on the host, i.e. it is also a barrier behind all work enqueued on the strip's stream. */
int emap_comm_allreduce_host(emap_ctx* ctx, double* inout, int32_t n, int32_t op);
/* one plane (EMAP_PLANE_*) of the FULL map on every rank: the strips' rows placed at their logical rows in a zeroed cell_n x cell_n
 * plane, all-reduced (exact: x + 0; -0.0 returns as +0.0).  Collective; for read-back / publishing, not on the per-frame path.
 * The reference has one map object and reads it directly (get_map_with_name_ref, elevation_mapping.py:720-775). */
int emap_comm_gather_layer(emap_ctx* ctx, int32_t plane, float* host_full_out);
int emap_update_sharded(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise,
                        emap_stats* stats /* may be NULL: no host synchronisation */);
/* How a sharded frame runs the visibility pass (the ray part of add_points_kernel, EM/kernels/custom_kernels.py:198-259; the
 * reference is single GPU).  Every ray starts at the sensor, so with rays marched BY ROW (each rank marches every ray through its
 * own rows) the strips around the sensor do what the whole map does.  BY RAY: every rank marches the rays of the points of its rows
 * over a replicated copy of the cells a ray can reach (one exact integer all-reduce of the window around the sensor), the effects
 * are all-reduced (sum of the validity decrements and hit counts, max of the upper-bound keys) and the owners apply their rows:
 * the same visits, bit-identical maps.  mode 0 = automatic (by ray from 2048 x 2048 cells on, frames on the tile-binned path),
 * 1 = always by row, 2 = by ray whenever the frame is on the tile-binned path.  Every rank must use the same mode. */
int emap_set_ray_mode(emap_ctx* ctx, int32_t mode);

/* ---- timing on the context's stream (hipEvents; bench.py's roofline leg) -------------------------- */
int emap_timer_begin(emap_ctx* ctx);
int emap_timer_end(emap_ctx* ctx, float* elapsed_ms); /* records, synchronises, returns elapsed */
/* per-stage device times of the last emap_update when profiling is enabled (order: hist, scan, scatter, gate, fuse,
 * commit, rays, average, overlap, post; hist/scan are 0 and "scatter" is the count kernel on the global-atomic path);
 * enabling inserts hipEvents between the stages (each costs a few microseconds of its own) */
int emap_enable_stage_timing(emap_ctx* ctx, int enable);
int emap_get_stage_times(emap_ctx* ctx, float ms_out[10]);
/* which kernels the last emap_update ran for phases count .. commit / average (results are bit-identical on all three):
 * 0 = chain of launches with global atomics (k_count, k_fuse, k_commit / k_average), 1 = tile-binned (sort front-end + tile kernels),
 * 2 = ONE launch, k_small_frame: small clouds on maps of up to 512^2 cells -- the robot-scale configuration the reference ships
 * (EM/parameter.py:137,165 -> 202^2 cells; EM/elevation_mapping.py:316-391 is a chain of ~12 dependent launches there).
 * EMAP_SMALL_FRAME=0 in the environment keeps such frames on path 0.
 * Bits 2-3 (the value & 3 is the path above): how the frame fused the channels declared by emap_frame_semantics -- 4 = inside the tile
 * kernel that fused the heights (32-byte sorted records), 8 = 32-byte records, stand-alone semantic kernel (a launch with heavy-tile
 * parts), neither = stand-alone kernels on 16-byte records / the atomic path.  EMAP_SEM_CARRY=0 keeps every frame on the last form.
 * Bits 4-5: what the frame did with the pending stencil pass of the frame before it (emap_update) -- 16 = ran it in its histogram launch
 * with only the outputs the frame reads itself (traversability; the normals too in front of a visibility pass), 32 = read none of them
 * (drift gate ruled out, no visibility pass) and launched no stencil workgroup; either way the pass stays pending and the next full pass
 * writes every output.  EMAP_POST_LEAN=0 in the environment: a pass taken along writes everything, as before. */
int emap_last_update_path(emap_ctx* ctx, int32_t* path);
/* k_small_frame synchronises its own grid (two barriers inside ONE launch).  If foreign work on the device keeps part of that grid from
 * starting for ~0.1 s, the launch aborts -- one compare-and-swap decides for the whole grid -- and leaves the map, the frame
 * accumulators and the drift record bit for bit as it found them; small frames already queued behind it do nothing.  The library re-runs
 * those frames, in order, on the chain of launches (path 0) before the next call on the context reads or changes anything: a frame
 * always completes, as the reference's does (EM/elevation_mapping.py:316-391), only later.  Precondition inherited from
 * emap_set_points_device: a device cloud stays valid until the frame that reads it has completed (emap_sync).  *frames = how many
 * frames have been re-run this way since emap_create (normally 0).  Test hooks: EMAP_SF_TEST_ABORT=1|2 (workgroup 0 gives up at once
 * at that barrier), EMAP_SF_SPIN_LIMIT=<polls> (a waiter's patience). */
int emap_small_frame_aborts(emap_ctx* ctx, uint32_t* frames);
/* *launches = how many frames since emap_create ran the stencil pass of the frame before them in one launch with their own histogram
 * (k_post_hist; see emap_update).  The call itself queues a pending pass, like every call that is not listed at emap_update. */
int emap_post_fused_launches(emap_ctx* ctx, uint32_t* launches);

#ifdef __cplusplus
}
#endif
#endif
