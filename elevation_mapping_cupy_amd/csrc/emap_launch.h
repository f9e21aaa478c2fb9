// The launchers of the kernel files, the kernel argument structs that travel by value between a host file and a kernel file, and
// the limits both sides size their buffers by -- declared ONCE.  Every file that defines a launcher includes this header, so a
// prototype that drifts from its definition fails to compile or link instead of failing at the first call.
#pragma once
#include "emap_device.h"
#include <cstddef>

// ---- kernel arguments built on the host (host files) and read by value in kernels (emap_semantic.hip) ----------------------------
struct SemRaw { int op, stride, K, n_max; long size, cells; double alpha; };      // the semantic kernel factories on caller arrays (k_semraw_acc / k_semraw_fin)
struct CamArgs { float P[12], K[9], D[5], center[3]; float x1, y1, z1, ih, iw; double tol; };      // tol = tolerance_z_collision (custom_image_kernels.py:9; 0.10 in the reference's call)
// The occlusion walk of k_image_corr ends only when it REACHES the camera cell (x1, y1): the cell must be integer valued, and its
// magnitude bounds the walk's length.  65536 cells is a cap, not a measurement: 2.6 km at 4 cm cells, far beyond any map, and it keeps
// every walk short.  emap_image_correspondence refuses anything else before it launches (ElevationMap.camera_cell raises the same way).
#define EM_CAM_CELL_MAX 65536
struct CmaxSpec { int n; int chan[8]; int layer[8]; };      // pointcloud_class_max: the fusion's channels and layers
// k_depth_cloud (emap_depth.hip): the images on the device, the sampled grid (Hs x Ws = n rows) and the cloud it writes; plane = H W
struct DepthArgs { int H, W, step, Hs, Ws, has_rgb, n_feat; long n, plane; float fx, fy, cx, cy, depth_scale, min_depth, max_depth, conf_thr;
                   const void* depth; const float* conf; const unsigned char* rgb; const float* feat; float* xyz; float* chan; };
#define EM_DEPTH_MAX_SIDE 8192      /* emap_bind_depth_image: image sides, step and channel count it accepts */
#define EM_DEPTH_MAX_STEP 64
#define EM_DEPTH_MAX_CHAN 16
// k_cloud_unpack (emap_cloudmsg.hip): the message on the device (`rows` rows of `width` points, row r at byte r * row_step; a message
// with tight rows travels as ONE row of n points), the column table (byte offset inside the point | conv << 16) and the cloud it writes
#define EM_CLOUDMSG_MAX_COLS 19
#define EM_CLOUDMSG_MAX_STEP 256
#define EM_CLOUDMSG_MAX_POINTS (1L << 26)
#define EM_CLOUDMSG_STAGE_BYTES 16384      /* message bytes a workgroup stages in LDS (+ 32 of alignment head and look-ahead) */
struct CloudMsgArgs { const unsigned char* msg; float* xyz; float* chan; long row_step; int rows, width, point_step, n_cols, tile, tiles_per_row;
                      unsigned int col[EM_CLOUDMSG_MAX_COLS]; };
// points per workgroup: the largest power of two in 64 .. 1024 whose bytes fit the stage (point_step 1 .. 256: 64 * 256 = the stage)
static inline int cloud_unpack_tile(int point_step) {
  int t = 1024;
  while (t > 64 && (long)t * point_step > EM_CLOUDMSG_STAGE_BYTES) t >>= 1;
  return t;
}
// k_image_frame (emap_image_msg.hip): a sensor_msgs/Image message on the device (pixel (v, u) at byte v * step + u * n_chan * esize,
// esize = the element's bytes) and the table of fusion entries a visible cell walks in order (emap_hip.h: emap_image_spec).  elem: the
// OpenCV depth code 0 .. 6 (8U 8S 16U 16S 32S 32F 64F).  The device copy of the message carries EM_IMGMSG_SLACK bytes behind its end:
// an element of 2 .. 8 bytes is read as the two or three aligned dwords around it.
#define EM_IMGMSG_MAX_SIDE 8192
#define EM_IMGMSG_MAX_SPECS 4
#define EM_IMGMSG_MAX_INDEX (1L << 24)      /* H W (x 3 with a colour entry): beyond it the reference's float index arithmetic is not exact */
#define EM_IMGMSG_SLACK 16
struct ImgMsgEntry { int kind, layer, plane, pad; double alpha; };
struct ImgMsgArgs { const unsigned char* msg; int H, W, step, elem, esize, n_chan, big, swap, n_specs, pad; ImgMsgEntry e[EM_IMGMSG_MAX_SPECS]; };
// The layer table of the output doors on the published map (LayerTab, grid_need), the device code that walks it and GridArgs, the
// arguments of k_grid_map / k_grid_windows: emap_publish_tile.h.
#include "emap_publish_tile.h"

// ---- limits shared by the host layer and emap_binned.hip -----------------------------------------------------------------------------
#define BIN_MAX_T 16384   /* LDS histogram / cursor arrays are dynamic: 4 B per tile */
#define BIN_MAX_B 2048
#define SEM_SPLIT_SLOTS 128      /* heavy tiles whose semantic sums several workgroups may share (19 MB of scratch) */
#ifndef EMAP_SPLIT_POOL_DEFAULT
#define EMAP_SPLIT_POOL_DEFAULT 0       /* standing pool of extra tile workgroups (emap_count): off -- measured, see there */
#endif

// launchers (emap_kernels.hip)
bool launch_count(hipStream_t, const KP&, const Pose&, const float*, long, int, Cells, AccF*, ErrSlot*, const GateArgs*, FrameDev*, unsigned int*);
void launch_gate(hipStream_t, const GateArgs&, ErrSlot*, FrameDev*, int, double*, const double*);
int small_frame_grid(const KP&, long);
void launch_small_frame(hipStream_t, int, const KP&, const Pose&, const float*, long, int, Cells, AccF*, unsigned int*, const OverlapArgs&,
                        const GateArgs&, FrameDev*, FrameDev*, ErrSlot*, unsigned int*, unsigned int*, unsigned int*, unsigned int*, unsigned int, unsigned int, int);
void launch_fuse(hipStream_t, const KP&, const Pose&, const float*, long, int, Cells, AccF*, const FrameDev*);
void launch_commit(hipStream_t, const KP&, Cells, const AccF*, const FrameDev*, unsigned long long*);
void launch_rays(hipStream_t, const KP&, const Pose&, const RayTab&, const float*, long, int, Cells, const AccRView&, const float*, long, FrameDev*, bool, const unsigned long long*, const unsigned int*, int, const float*, const unsigned int*, const unsigned int*);
void launch_win_pack(hipStream_t, const KP&, const Win&, Cells, const float*, long, const unsigned int*, const unsigned long long*, float);
void launch_win_prepare(hipStream_t, const Win&, int);
void launch_win_unpack(hipStream_t, const KP&, const Win&, AccR*);
void launch_win_reduce(hipStream_t, long long*, unsigned int*, const long long*, const unsigned int*, int, long, long, long);
void launch_ray_apply(hipStream_t, const KP&, Cells, AccR*, unsigned long long*, const OverlapArgs&, FrameDev*, unsigned int*, int);
void launch_average(hipStream_t, const KP&, Cells, AccF*, AccR*, const FrameDev*, bool, bool, unsigned int*, const OverlapArgs&);
void launch_overlap(hipStream_t, const KP&, Cells, int, int, float, float);
void launch_var_time(hipStream_t, const KP&, Cells, int, int);
int post_tile_rows(const KP&);
void launch_post(hipStream_t, const KP&, const float*, const float*, const float*, const float*, Cells, float*, float*, long, int, int, const int*, const int*, int, int);
int post_hist_tile_rows(const KP&, int);
// output set of the stencil pass a frame takes along (POST_CELL, emap_kernels.hip): everything | no traversability_input | traversability
// only, as the drift gate's predicate in the flag plane (TRAV_FLAG_*, one byte per cell; the last pointer) | traversability only, as the
// word in the hot half (EMAP_POST_FLAGS=0)
enum { POST_OUT_FULL = 0, POST_OUT_TRAV_NORMALS = 1, POST_OUT_TRAV = 2, POST_OUT_TRAV_WORD = 3 };
// A byte of the flag plane: the cell's traversability is not / is above traversability_inlier, or the stencil pass does not decide the
// cell (the 3-cell border) and the word in the hot half holds.
enum { TRAV_FLAG_BELOW = 0, TRAV_FLAG_ABOVE = 1, TRAV_FLAG_WORD = 2 };
bool launch_post_hist(hipStream_t, int, const KP&, const float*, const float*, const float*, const float*, Cells, float*, float*, long, int,
                      const Pose&, const BinGeo&, const float*, long, int, unsigned int*, long, int, unsigned char*);
void launch_get_plane(hipStream_t, const KP&, Cells, int, float*);
void launch_publish(hipStream_t, const KP&, Cells, const float*, long, int, float, int, float*);
void launch_set_plane(hipStream_t, const KP&, Cells, int, const float*);
void launch_fill_cells(hipStream_t, Cells, long, const Cell&);
void launch_point_index(hipStream_t, const KP&, const Pose&, const float*, long, int, int*, unsigned char*);
void launch_plane_view(hipStream_t, const KP&, int, int, float*, float*, int);
void launch_materialize(hipStream_t, const KP&, Cells);
void launch_band_clear(hipStream_t, const KP&, float*, int, long, int, int);

// semantic layers, camera path and publish-time plugins (emap_semantic.hip)
void launch_sem_points(hipStream_t, const KP&, const Pose&, const SemSpec&, const float*, long, int, const ChanView&, double*, unsigned int*, long);
void launch_sem_finalize(hipStream_t, const KP&, const SemSpec&, const unsigned int*, double*, unsigned int*, float*, float*, long);
void launch_semraw_acc(hipStream_t, const SemRaw&, const float*, const int*, const int*, const float*, const int*, float*, unsigned int*);
void launch_semraw_fin(hipStream_t, const SemRaw&, float*, const unsigned int*, const int*, const float*, const float*, float*);
void launch_polygon_mask(hipStream_t, int, const int*, const int*, int, const int*, float*);
void launch_dilate_planes(hipStream_t, int, int, const float*, const float*, float*, float*);
void launch_cmax_ids(hipStream_t, const KP&, const CmaxSpec&, const ChanView&, long, const float*, long, unsigned char*, unsigned char*);
void launch_cmax_sum(hipStream_t, const KP&, const Pose&, const CmaxSpec&, const float*, long, int, const ChanView&, const int*, long long*, long);
void launch_cmax_select(hipStream_t, const KP&, const CmaxSpec&, int, const long long*, long, unsigned char*, unsigned char*, const unsigned int*, float*, float*, float*);
void launch_image_corr(hipStream_t, const KP&, const CamArgs&, Cells, float*, unsigned char*);
void launch_image_fuse(hipStream_t, const KP&, int, float*, const float*, const float*, const unsigned char*, float, float, double);
void launch_inpaint_sweep(hipStream_t, int, const float*, const float*, float*, float*, const unsigned int*, unsigned int*);
void launch_min_sweep(hipStream_t, int, int, const float*, const float*, const float*, float*, float*, const unsigned int*, unsigned int*, bool);
void launch_box3(hipStream_t, int, const float*, float*);
void launch_erode(hipStream_t, int, int, const float*, float*);

// tile-binned scatter (emap_binned.hip)
void launch_bin_hist(hipStream_t, const KP&, const Pose&, const BinGeo&, const float*, long, int, unsigned int*, BinStg*, unsigned int*);
void launch_bin_scan(hipStream_t, const BinGeo&, unsigned int*, unsigned int*, unsigned int*, unsigned int*, const SplitView&);
void launch_bin_scatter(hipStream_t, const KP&, const Pose&, const BinGeo&, const float*, long, int, const unsigned int*, const unsigned int*, BinRec*, const BinStg*, const unsigned int*, const ChanView&, const SemCarry&);
void launch_tile_count(hipStream_t, const KP&, const BinGeo&, const BinRec*, int, const unsigned int*, Cells, ErrSlot*, const SplitView&, long,
                       const unsigned char* trav_flag);      // trav_flag: the flag plane this frame's k_post_hist wrote (POST_OUT_TRAV), or nullptr: traversability is the word in the hot half
void launch_tile_semantic(hipStream_t, const KP&, const BinGeo&, const SemSpec&, const BinRec*, int, int, const unsigned int*, const ChanView&, long,
                          const unsigned int*, float*, float*, long, const SplitView&, void*, int);
size_t sem_split_bytes(int);
bool sem_split_possible(const SemSpec&);
void launch_bin_fuse(hipStream_t, const KP&, const BinGeo&, const BinRec*, int, const unsigned int*, Cells, AccF*, FrameDev*, bool, bool, unsigned int*, unsigned long long*, unsigned int*, float*, const OverlapArgs&, const GateFold&, const SplitView&, long, const SemMini*);
bool bin_fuse_takes_semantics(const SplitView&, bool, bool, int);

// depth-image input (emap_depth.hip)
void launch_depth_cloud(hipStream_t, const DepthArgs&, int);

// PointCloud2 input (emap_cloudmsg.hip); aligned4: every field read is one aligned dword of the message
void launch_cloud_unpack(hipStream_t, const CloudMsgArgs&, bool aligned4);

// Image message input (emap_image_msg.hip): correspondence + sampling of the message bytes + fusion, one launch; the instantiation is
// chosen by the element's size (image_frame_variant: 0 .. 3 for 1, 2, 4, 8 bytes)
static inline int image_frame_variant(int esize) { return esize == 1 ? 0 : esize == 2 ? 1 : esize == 4 ? 2 : 3; }
void launch_image_frame(hipStream_t, const KP&, const CamArgs&, Cells, float*, unsigned char*, const ImgMsgArgs&, float*, long);

// GridMap message output (emap_gridmsg.hip): whole-map contexts only (the caller checks)
void launch_grid_map(hipStream_t, const KP&, Cells, const GridArgs&);

// publish-time plugins on resident planes (emap_plugchain.hip); EM_RANGE_FLOATS: scratch of launch_range (256 partial triples + the result)
#define EM_RANGE_FLOATS (3 * 256 + 4)
void launch_mask_nan(hipStream_t, long, const float*, const float*, float*);
void launch_smooth2(hipStream_t, int, const float*, float*);
void launch_range(hipStream_t, long, const float*, int, float*, float*);
void launch_quantise(hipStream_t, long, const float*, int, const float*, float*);
void launch_dequantise(hipStream_t, long, const float*, const float*, int, const float*, float*);
void launch_robot_centric(hipStream_t, int, float, const float*, int, float, const float*, const float*, float*);
// The ops that read several layers (EMAP_PLUGIN_SEMANTIC_FILTER .. _FEATURES_PCA).  PlugSrcs: the op's run of the side table, by value --
// code[k] = kind << 8 | index (kind 0: RAW map layer read in the cells, 1: resident plane `index` of `planes`, 2: semantic layer `index` of
// `sem`, planes of sem_plane floats at the map's circular origin); PlugPars: the flags and constants of the ops with at most 16 sources.
#define EM_PLUG_SRC_MAX 64
#define EM_PLUG_PAR_MAX 16
struct PlugSrcs { int n, pad_; long sem_plane; const float* sem; const float* planes; unsigned short code[EM_PLUG_SRC_MAX]; };
struct PlugPars { int flags[EM_PLUG_PAR_MAX]; float f0[EM_PLUG_PAR_MAX], f1[EM_PLUG_PAR_MAX]; double d0[EM_PLUG_PAR_MAX]; };
void launch_semantic_filter(hipStream_t, const KP&, Cells, const PlugSrcs&, float* dst);
void launch_semantic_trav(hipStream_t, const KP&, Cells, const PlugSrcs&, const PlugPars&, float* dst);
void launch_max_layer(hipStream_t, const KP&, Cells, const PlugSrcs&, const PlugPars&, int take_min, float* dst);
// FEATURES_PCA (emap_pca.hip).  Scratch of one op, in doubles: per-workgroup partials of the means (16 each), of the moments (256 each)
// and of the score ranges (6 each), behind them the folded means (16), moments (256), the three signed eigenvectors (48) and lo / hi (6)
#define EM_PCA_PARTS 256
#define EM_PCA_F 16
#define EM_PCA_DOUBLES ((size_t)EM_PCA_PARTS * (EM_PCA_F + EM_PCA_F * EM_PCA_F + 6) + EM_PCA_F + EM_PCA_F * EM_PCA_F + 3 * EM_PCA_F + 6)
void launch_features_pca(hipStream_t, const KP&, Cells, const PlugSrcs&, double* scratch, float* dst);
// the value of source k of S at the logical cell li = r * C + c of a full map, ci = owned_cell(P, r, c)
__device__ __forceinline__ float plug_src_read(const PlugSrcs& S, int k, const Cells& cells, long L, long li, long ci) {
  const int code = S.code[k], kind = code >> 8, idx = code & 255;      // (uniform: the table travels in the kernel's arguments)
  if (kind == 0) return idx < 4 ? reinterpret_cast<const float*>(cells.hot + ci)[idx] : reinterpret_cast<const float*>(cells.cold + ci)[idx - 4];
  if (kind == 1) return S.planes[(long)idx * L + li];
  return S.sem[(long)idx * S.sem_plane + ci];
}

// Inpainting on resident planes (EMAP_PLUGIN_INPAINT_FRONTS).  FrontsDev: the device images and planes of one run of the fronts pipeline
// (emap_inpaint_fronts.hip) -- the handle of emap_inpaint_telea_fronts_u8 owns one, every inpaint op of a chain carves its own out of the
// context's scratch (fronts_carve; fronts_bytes: what it takes).  launch_fronts enqueues the distance transform, k_fr_init and `n_advance`
// launches of k_fr_advance (fronts 1 .. n_advance * S) on images that are on the device, and waits for nothing; a launch beyond the last
// front finds no tile that holds one of its fronts and returns at its first test.
struct FrontsDev { unsigned char *in, *mask, *out; int *g, *d; float* T; int2* tile_mm; int* dmax; int* blk; };
#define EM_FRONTS_S_MAX 16
int fronts_default_steps();
size_t fronts_bytes(int rows, int cols, int S);
FrontsDev fronts_carve(unsigned char* base, int rows, int cols, int S);
void launch_fronts(hipStream_t, const FrontsDev&, int rows, int cols, int S, int n_advance);
// the op's arithmetic around the fill (emap_inpaint_chain.hip); InpRange: lo / hi of elevation over the cells with is_valid >= 0.5 and
// how many cells are known / unknown -- EM_INP_PARTS partial records and the folded one behind them
struct InpRange { float lo, hi; unsigned int known, unknown; };
#define EM_INP_PARTS 256
void launch_inpaint_range(hipStream_t, const KP&, Cells, InpRange* parts, InpRange* rec);
void launch_inpaint_quantise(hipStream_t, const KP&, Cells, const InpRange* rec, unsigned char* q8, unsigned char* mask);
void launch_inpaint_dequantise(hipStream_t, const KP&, Cells, const InpRange* rec, const unsigned char* out8, float* dst);

// Safety-polygon service on the device (emap_polysafe.hip).  PolyDesc: one polygon of the batch -- its run of the vertex table (the nv
// row indices at verts[2 vbeg], the nv column indices behind them), the bounding box in cells as the reference's kernel culls by it,
// the box clipped to the interior (row0 / col0, nrows x ncols cells; ntr x ntc tiles of EM_POLY_TILE, enumerated row-major from
// work item item0) and the first row of its per-row extremes (ext0, in rows).  PolyItem: one tile.  PolyPart: what one tile's workgroup
// found inside the polygon -- rmin / rmax: per row of the tile the smallest and largest column of a risky cell (EM_POLY_EMPTY_MIN / -1:
// none).  PolySrc: where the checker value lies -- kind 0: raw map layer `index` (0 .. 6), 1: semantic plane `index` of `base` (planes
// of `plane` floats at the map's circular origin), 3: resident plugin plane `index` of `base` (logical order); thr: a cell is risky
// above it.  PolyOut: struct emap_polygon_verdict (emap_hip.h; emap_api_polysafe.hip asserts the layout).
#define EM_POLY_TILE 32
#define EM_POLY_SWEEP_WG 256      /* workgroups of the poison sweep: a fixed number, one per CU */
#define EM_POLY_MAX_VERTS 256
#define EM_POLY_EMPTY_MIN 0x7fffffff
struct PolyDesc { int vbeg, nv, bminx, bminy, bmaxx, bmaxy, item0, ntr, ntc, row0, nrows, col0, ncols, pad_; long ext0; };
struct PolyItem { int poly, tr, tc, pad_; };
struct PolyPart { double sum_valid, sum_risk; float max_risk; int n_inside, n_risky, has_nan; int rmin[EM_POLY_TILE], rmax[EM_POLY_TILE]; };
struct PolySrc { int kind, index; long plane; const float* base; float thr; int pad_; };
struct PolyOut { double sum_valid, sum_risk; float max_risk; int n_inside, n_risky, flags, row_begin, n_rows, col_begin, n_cols; };
void launch_polysafe_tiles(hipStream_t, const KP&, Cells, const PolySrc&, const PolyDesc*, const int*, const PolyItem*, int, PolyPart*, unsigned int*);
void launch_polysafe_fold(hipStream_t, int, const PolyDesc*, int, const PolyPart*, const unsigned int*, PolyOut*, int*);

// Submap service on the device (emap_submap.hip): a batch of windows of the published index space from ONE launch.  GridWin: one window
// -- element (i, j) of it is published element (i0 + i, j0 + j), i.e. logical source cell (M - (i0 + i), M - (j0 + j)) -- and the float
// at which its planes begin in the packed output (base = n_layers * the cells of the windows before it; plane l of the layer table
// follows at pos[l] * ni * nj with pos[l] = l: no slot indirection).  GridItem: one 32 x 32 tile of one window, a workgroup each.
#define EM_GRID_MAX_WINDOWS 64
struct GridWin { int i0, j0, ni, nj; long base; long pad_; };
struct GridItem { int win, tr, tc, pad_; };
void launch_grid_windows(hipStream_t, const KP&, Cells, const GridArgs&, const GridWin*, const GridItem*, int);

// Point-cloud output on the device (emap_cloudout.hip): the valid cells of the published map packed in grid_map's iterator order
// (lin = j * M + i).  CloudArgs: a layer table (LayerTab, emap_publish_tile.h) -- the TESTED entries for k_cloud_count, the EMITTED
// ones for k_cloud_write, where field[l] is the first dword of entry l in a
// record of n_fields dwords and cflags[l] & EM_CLOUD_POINT marks the entry that emits x, y, z.  call: EM_CLOUD_NORMAL_MIN -- a cell
// passes only if !((nx nx + ny ny) + nz nz < sum_min) in double (sum_min: the smallest double whose square root is not below the
// caller's bound, so the test IS the one on the norm) --, EM_CLOUD_INDEX -- the last dword of a record is lin.  nt = ceil(M / 32);
// cap: the records the output buffer holds.  The scan takes EM_CLOUD_SCAN_TRIP mask words per trip of its one workgroup: the mask and
// offset buffers are sized to a multiple of it.
#define EM_CLOUD_POINT 1
#define EM_CLOUD_NORMAL_MIN 8
#define EM_CLOUD_INDEX 16
#define EM_CLOUD_SCAN_BLOCK 1024
#define EM_CLOUD_SCAN_TRIP (4 * EM_CLOUD_SCAN_BLOCK)
struct CloudArgs { LayerTab tab; int call, nt, n_fields, pad_; long cap; double sum_min; unsigned char cflags[EM_GRID_MAX_LAYERS], field[EM_GRID_MAX_LAYERS]; };
void launch_cloud_count(hipStream_t, const KP&, Cells, const CloudArgs&, unsigned int* masks);
void launch_cloud_scan(hipStream_t, const unsigned int* masks, unsigned int* offs, long W, unsigned int* total);
void launch_cloud_write(hipStream_t, const KP&, Cells, const CloudArgs&, const float* xs, const float* ys, const unsigned int* masks, const unsigned int* offs, float* out);

// Plane segmentation on the device (emap_planeseg.hip): the front of convex_plane_decomposition's SlidingWindowPlaneExtractor on ONE
// source layer of the published map -- planar cells, connected labels, one plane per label.  Every plane below is
// dense M x M in published index space, cell (i, j) at idx = i * M + j.  PlaneArgs: the call's constants (angles arrive as cosines, the
// patch threshold squared, all in double).  PlaneBufs: the planes and words the chain works on, carved by the host file out of buffers
// the context owns -- src: the source heights; nrm: 3 planes of window normals (float); bit / bit2: the planar bytes and the opening's
// second image; parent: the union-find links (a link only ever points to a SMALLER idx; -1: not planar), later the numbered labels;
// root: every cell's root, a plane of its own; cnt / amin: per ROOT cell the finite members and the smallest finite member; mask1 /
// offs1: a bit per cell "is a root" and the exclusive scan of its popcounts (k_cloud_scan's layout: EM_CLOUD_SCAN_TRIP words a trip);
// mask2 / offs2: the same for "is a root with at least min_points members", i.e. owns a slot; head: [0] labels, [1] slots.
// PlaneSlot: one label that gets a plane.  s[]: the exact integer moments n, S di, S dj, S q, S di di, S dj dj, S di dj, S di q,
// S dj q, S q q about the anchor (root cell, height of cell amin); kdist / kdot: monotone keys of the largest plane distance and of
// the largest NEGATED normal dot product (atomicMax, identity 0); the rest is written by k_ps_finalise.
#define EM_PLANE_SWEEPS 4        /* Jacobi sweeps of the 3 x 3 eigenproblem: FIXED (tests/test_plane_seg_cases.py measures the count) */
#define EM_PLANE_OPEN_MAX 8      /* opening radius the door accepts (a cap, not a measurement) */
#define EM_PLANE_Q_BITS 13       /* heights enter the label moments as multiples of 2^-13 m about the anchor */
#define EM_PLANE_Q_RANGE 32.0    /* ... and a cell farther than this from its anchor is left out and counted */
struct PlaneArgs { int M, K, conn, open_r, min_points, pad_; double res, thr2, cos_local, cos_plane, ox, oy; };
struct PlaneBufs { float* src; float* nrm; unsigned char* bit; unsigned char* bit2; int* parent; int* root; int* cnt; int* amin;
                   unsigned int* mask1; unsigned int* offs1; unsigned int* mask2; unsigned int* offs2; unsigned int* head; };
struct PlaneSlot { long long s[10]; unsigned long long kdist, kdot; double support[3], normal[3]; int label, root, accept, left_out; };
void launch_ps_source(hipStream_t, const KP&, Cells, const LayerTab&, float* src);
void launch_ps_window(hipStream_t, const PlaneArgs&, const PlaneBufs&);
void launch_ps_morph(hipStream_t, int M, int radius, int dilate, const unsigned char* in, unsigned char* out);
void launch_ps_labels(hipStream_t, const PlaneArgs&, const PlaneBufs&, const unsigned char* bit);
void launch_ps_moments(hipStream_t, const PlaneArgs&, const PlaneBufs&, PlaneSlot* slots);
void launch_ps_planes(hipStream_t, const PlaneArgs&, const PlaneBufs&, PlaneSlot* slots, int n_slots, int* labels);
// k_ps_local / k_ps_merge / k_ps_flatten alone: the root of every set cell of a byte plane (root[]: -1 where the byte is 0), cnt[] zeroed and
// amin[] at 0x7fffffff for every cell, mask1 the "is a root" bits.  launch_ps_labels starts with it; the planar terrain (below) labels its
// NaN cells with it.
void launch_ps_components(hipStream_t, int M, int conn, const unsigned char* bit, int* parent, int* root, int* cnt, int* amin, unsigned int* mask1);

// Planar terrain on the device (emap_terrain.hip): what convex_plane_decomposition publishes around the segmentation -- the preprocessing
// of GridMapPreprocessing::preprocess (minValues inpainting, median) in front of it, Postprocessing::postprocess (smooth_planar, the
// dilated and lifted elevation) behind it.  Every plane is dense M x M in published index space, as above.
// TerrainTab: the call's small tables, built on the host and uploaded -- close / lift: the row spans of OpenCV's elliptic structuring
// element of the closing (size kd) and of the dilation in non-planar regions (row a covers the columns [lo[a], hi[a])); off: the sloped
// dilation's kd x kd height offsets; gauss: the Gaussian's taps.  A float's monotone KEY (tr_key) is an int whose signed order is the
// numeric order, -0 below +0: every minimum, maximum and order statistic of the chain is taken on keys, so it is a function of the bits.
#define EM_TERRAIN_KERNEL_MAX 31      /* every kernel size of the chain, in cells (a cap: the LDS tile holds a halo of 15) */
#define EM_TERRAIN_OFFSET_MAX 15      /* nonplanar_horizontal_offset: a dilation of 2 * 15 + 1 cells */
#define EM_TERRAIN_REPEATS_MAX 8      /* median passes (a cap, not a measurement) */
struct TerrainSpans { signed char lo[EM_TERRAIN_KERNEL_MAX + 1], hi[EM_TERRAIN_KERNEL_MAX + 1]; };
struct TerrainTab { TerrainSpans close, lift; float gauss[EM_TERRAIN_KERNEL_MAX + 1]; float off[EM_TERRAIN_KERNEL_MAX * EM_TERRAIN_KERNEL_MAX + 3]; };
void launch_tr_nanbit(hipStream_t, long N, const float* in, unsigned char* bit);
void launch_tr_rim(hipStream_t, int M, const float* in, const unsigned char* bit, const int* root, int* amin);
void launch_tr_fill(hipStream_t, long N, const float* in, const unsigned char* bit, const int* root, const int* amin, float* out);
void launch_tr_median(hipStream_t, int M, int k, const float* in, float* out);
void launch_tr_mask(hipStream_t, long N, const float* e, const int* labels, float* w, float* m, unsigned char* bit);
void launch_tr_morph(hipStream_t, int M, int kd, int dilate, const TerrainSpans* spans, const float* in, float* out);
void launch_tr_sloped(hipStream_t, int M, int kd, const float* off, const float* in, float* out);
void launch_tr_blur(hipStream_t, int M, int k, const float* taps, double scale, const float* in, float* out);
void launch_tr_lift(hipStream_t, long N, const float* e, const float* d, const float* m, int add_on, float add, int sub_on, float sub, float* out);
// k_ps_link (emap_planeseg.hip): element k of 0 .. n - 1 united with other[k] by the segmentation's union-find on global memory (the
// invariant in that file's head: parent[k] == k before the launch, every access to parent[] an agent-scope atomic -- the workgroups of a
// launch run on several XCDs whose L2s are not coherent for plain accesses --, the root of a set its smallest index whatever the order of
// the atomics).  With a permutation in other[], the sets are its cycles: the planar regions (below) find their rings with it.
void launch_ps_link(hipStream_t, int n, const int* other, int* parent);

// Planar regions on the device (emap_regions.hip): the contour stage of convex_plane_decomposition on a label plane -- per connected piece
// of a label a boundary polygon with holes and its insets.  RegionArgs: M the side of the label plane, U the side
// of the traced images (3 M - 2, raw mode: M), k the margin ellipse's size in pixels, Wc the crack-mask words of ONE image
// (ceil(U U / 8)).  RegionBufs: what is sized by the pixels -- labels: the label plane (raw mode: the U x U mask); em: per pixel bit 0
// "survives the margin ellipse", bit 1 "survives the cross"; bm: the byte "in B_m"; flag: n_labels + 1 words "the label keeps its
// margin", zeroed by the caller; A / B: the boundary and the inset image; bitA / bitB: their != 0 bytes; rootA / rootB: every pixel's
// component root; cmask / coffs: 4 crack bits per pixel, A's words in front of B's, and their scan (k_cloud_scan's layout); head: [0]
// cracks, [1] rings, [2] vertices.  RegionCracks: what is sized by the cracks, in COMPACT indices (the rank of the crack's bit) -- raw:
// image << 31 | 4 idx + s; succ / pred: the permutation and its inverse; parent / cyc: the union-find links and every crack's ring (its
// smallest crack); vbit: the crack emits a vertex; nv: the doubling's two buffers (next, vertices from here to the ring's end); hmask /
// hoffs: the bit "is a ring's smallest crack" and its scan; rcnt / rfirst: per ring its vertices and their exclusive prefix; rings /
// verts: the answer.  RegionRing: struct emap_region_ring (emap_hip.h; emap_api_regions.hip asserts the layout).
#define EM_REGION_MARGIN_MAX 14      /* 2 (1 + 14) + 1 = EM_TERRAIN_KERNEL_MAX pixels */
struct RegionArgs { int M, U, mode, k; long Wc; };
struct RegionBufs { const int* labels; unsigned char* em; unsigned char* bm; unsigned int* flag; int* A; int* B; unsigned char* bitA; unsigned char* bitB;
                    int* rootA; int* rootB; unsigned int* cmask; unsigned int* coffs; unsigned int* head; };
struct RegionRing { int first_vertex, n_vertices, image, is_hole, label, root, crack, boundary; };
struct RegionCracks { unsigned int* raw; int* succ; int* pred; int* parent; int* cyc; unsigned char* vbit; int2* nv[2]; unsigned int* hmask; unsigned int* hoffs;
                      int* rcnt; int* rfirst; RegionRing* rings; int2* verts; };
// ceil(log2 n) doubling rounds (at least 1): 2^rounds steps reach every crack of the longest possible ring
static inline int region_rounds(int n) { int r = 1; while ((1L << r) < (long)n) ++r; return r; }
void launch_rg_images(hipStream_t, const RegionArgs&, const TerrainSpans&, const RegionBufs&);
void launch_rg_cracks(hipStream_t, const RegionArgs&, const RegionBufs&);
void launch_rg_trace(hipStream_t, const RegionArgs&, const RegionBufs&, const RegionCracks&, int n_cracks);
