// What the host files of the C ABI share (emap_api.hip: the core; emap_api_semantic.hip: semantic layers and the camera path;
// emap_api_plugins.hip: the publish-time plugins on caller planes; emap_api_comm.hip: halos, the RCCL communicator, rays by ray; the
// doors emap_api_{depth,cloudmsg,image_msg,gridmsg,plugchain}.hip): the context, the frame record, the error macros and the three
// mechanisms every door is built from -- a buffer grown on demand (grow), caller bytes staged through pinned slots (Stage) and the
// bound cloud (BoundCloud) -- each described where it is defined below, plus the few helpers that cross a file boundary.
// Whatever has a symbol here lives in namespace emap_host, so that nothing can collide with a symbol of the program that loads the
// library.  RCCL stays inside emap_api_comm.hip: the context holds the communicator and the bound entry points as opaque pointers.
#pragma once
#include "emap_launch.h"
#include "../../include/emap_hip.h"
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// timed stages of emap_update (emap_get_stage_times): hist+scan are 0 on the atomic path, where "scatter" is k_count
enum { ST_HIST = 0, ST_SCAN, ST_SCATTER, ST_GATE, ST_FUSE, ST_COMMIT, ST_RAYS, ST_AVERAGE, ST_OVERLAP, ST_POST, ST_N };

struct RcclApi;      // the RCCL entry points of the path, bound with dlsym (emap_api_comm.hip)
struct ncclComm;     // (rccl.h: ncclComm_t is a pointer to it)

namespace emap_host {
// ---- asynchronous cloud upload (a1: ElevationMap.input_pointcloud, EM/elevation_mapping.py:456-458) ------------------------------
// The ROS wrapper hands over a pageable float64 matrix.  It is converted to float32 on the HOST by a few worker threads straight
// into a pinned slot (so only 12 of the 24 bytes per point cross PCIe and no device-side cast pass is needed), chunk by chunk, each
// chunk's DMA on a copy stream overlapping the next chunk's conversion; the device buffer is double buffered so the upload of frame
// k+1 overlaps the kernels of frame k.  The call returns when the caller's buffer has been consumed (it is only borrowed).
struct Workers {
  std::vector<std::thread> th; std::mutex m; std::condition_variable cv, done_cv;
  std::function<void(int, int)> job; int gen = 0, pending = 0; bool stop = false;
  explicit Workers(int n) {
    for (int i = 0; i < n; ++i) th.emplace_back([this, i, n] {
      int seen = 0;
      for (;;) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen; auto f = job; l.unlock();
        f(i, n);
        l.lock(); if (--pending == 0) done_cv.notify_all();
      }
    });
  }
  void run(const std::function<void(int, int)>& f) {       // f(worker, n_workers) on every worker; returns when all are done
    std::unique_lock<std::mutex> l(m);
    job = f; pending = (int)th.size(); ++gen; cv.notify_all();
    done_cv.wait(l, [&] { return pending == 0; });
  }
  ~Workers() { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_all(); for (auto& t : th) t.join(); }
};

// A device buffer for the duration of a call, freed when it goes out of scope on every way out: plain scratch (alloc), or the device
// copy of a host array (put) that get() copies back.
struct DevBuf {
  void* d = nullptr; size_t bytes = 0; void* back = nullptr;
  hipError_t alloc(size_t n) { bytes = n; return hipMalloc(&d, n); }
  hipError_t put(const void* host, size_t n, hipStream_t s, void* write_back) {
    bytes = n; back = write_back;
    if (!n) return hipSuccess;
    hipError_t e = hipMalloc(&d, n);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(d, host, n, hipMemcpyHostToDevice, s);
  }
  hipError_t get(hipStream_t s) { return (back && bytes) ? hipMemcpyAsync(back, d, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (d) hipFree(d); }
};

// The cloud the frame kernels read: bound by an upload, a caller's device pointers or a door that produces its cloud on the device.
// One record, so that whoever has to remember a binding (the small-frame ring, sf_recover) copies it whole.
struct BoundCloud {
  const float* pts; long n; int stride;      // xyz: rows of `stride` floats (3 for a de-interleaved cloud)
  long n_all;                                // size of the cloud the caller handed over (> n for a bucketed one): what every rank of a sharded map shares
  ChanView chan; int n_cols;                 // its extra channels (emap_device.h: ChanView); n_cols = columns of the caller's matrix (3 + K)
};
// A de-interleaved cloud in ONE buffer: xyz as an (n, 3) matrix, the K channels as an (n, K) matrix behind it at a 256-byte boundary.
struct CloudLayout { long chan_off, tot; };      // floats
inline CloudLayout cloud_layout(long n, long K) {
  const long off = K ? ((3 * n + 63) & ~63L) : 0;
  return {off, K ? off + K * n : 3 * n};
}

// Caller bytes on their way to the device: two pinned slots, used in turn, and ONE device buffer.  A slot is written by the host while
// the other's DMA may still run; its event says that its own DMA of two calls ago is done (long done in a running stream).  The device
// buffer is overwritten in stream order, behind the kernel that read what the call before put there.  (stage_next, stage_send,
// stage_free: emap_api.hip.)
struct Stage {
  unsigned char* pin[2]; size_t pin_cap[2]; hipEvent_t ev[2]; bool ev_on[2]; int slot;
  unsigned char* dev; size_t dev_cap;        // bytes
};
}  // namespace emap_host

struct emap_ctx {
  emap_params prm;
  emap_strip strip;
  KP kp;
  int device;
  hipStream_t stream;
  bool own_stream;
  long ncells_alloc;        // (rows + 2*halo) * C
  Cells cells;                     // two planes of 16-byte half cells (emap_device.h)
  int torg_r, torg_c;              // origin traversability_input was written with (kp.norg_*: the normal planes)
  AccF* acc; AccR* accr;
  float* trav_in; float* normal;   // normal: 3 planes of ncells_alloc
  float* scratch;                  // one plane (get/set staging)
  float* plug_buf; size_t plug_cap; unsigned int* plug_cnt; size_t plug_cnt_cap;   // plane scratch of the publish-time plugins (kept between calls)
  ErrSlot* slots; FrameDev* frame;
  RayTab rt; float* ray_S; unsigned short* ray_lut;
  unsigned long long* inert;       // 1 bit per owned cell (rows of ceil(C/64) words), written by k_commit / k_tile_fuse<true, true>
  unsigned int* inl_plane;         // newmap[3] of frames whose tile kernel commits itself (binned path + visibility pass), on demand
  float* ray_thr;                  // same frames: per 8 x 8 block height at or above which a ray sample cannot affect any cell of the block
  bool inert_zero;                 // the bitmap is all zero (k_ray_apply leaves it so; k_commit overwrites it)
  // tile-binned scatter buffers (allocated on demand)
  int scatter_mode;                // 0 auto, 1 atomic, 2 binned
  int force_sub;                   // test hook: minimum bin height factor (emap_set_scatter_mode bits 8..15)
  bool frame_binned;               // the count stage of the current frame used the binned path
  unsigned int* bin_sync;          // ticket counters of k_bin_scan (last_block_ticket), zero between launches
  SplitView split;                 // heavy tiles reduced by several workgroups (emap_device.h); split.on: this frame's scan listed them
  void* split_mem;                 // one allocation behind split's arrays
  void* sem_split_mem;             // scratch of the split semantic tile kernel (SemSplit), zero between launches
  volatile unsigned int* split_need;   // host-mapped word: the parts the last scan the device has finished would have listed
  bool split_dirty;                // k_tile_count has filled slots that no k_tile_fuse has cleared yet
  unsigned int* cnt_sync;          // ticket words of k_count's folded gate (Frame::fold_gate)
  // robot scale: count -> gate -> fuse -> commit + average in one launch (k_small_frame): its barriers' release words live behind the
  // ticket words of cnt_sync.  A launch whose grid barrier is ABORTED leaves map, accumulators and drift record exactly as it found
  // them, and the launches queued behind it do nothing (device-side poison word).  sf_host = two host-mapped words: [0] epoch of the
  // last launch that will be applied, [1] epoch of the first aborted launch.  The frames issued and not yet known to be applied wait
  // in sf_ring with everything needed to run them again; sf_settle (every entry point but the ones that only bind a cloud) learns
  // their fate and, after an abort, re-runs them in order on the chain of launches.
  unsigned int sf_epoch; volatile unsigned int* sf_host; unsigned int* sf_host_dev; unsigned int* sf_poison;
  FrameDev* frame_save;            // the frame record as the gate of the last k_small_frame found it
  struct SfFrame { unsigned int epoch; float R[9], t[3]; double pn, on; Moves mv; emap_host::BoundCloud cloud; };
  enum { SF_RING = 8 };
  SfFrame sf_ring[SF_RING]; int sf_head, sf_count;
  bool sf_redo;                    // inside sf_recover: frames take the chain of launches
  unsigned int sf_aborts;          // frames re-run so far (emap_small_frame_aborts)
  int update_path;                 // emap_last_update_path
  // The stencil pass of the last frame, not launched yet (frame_impl): the next binned whole-map frame runs it in one grid with its own
  // histogram (k_post_hist); every other way into the library launches it first (post_settle, part of SF_CHECK).  Nothing that changes
  // the map, its origin or the parameters gets past it, so what is launched then is what post_part_impl(ctx, 0) would have launched when
  // the frame ended.  A frame may take the pass along LEAN -- only the outputs it reads itself (count_impl) -- or, reading none, not
  // launch it at all: the pass then stays pending, and the first FULL pass clears the flag (post_settle has the invariant).
  bool post_pending;
  int post_took;                   // this frame and the pending pass, as bits of update_path: 16 taken along lean, 32 left owed without a launch
  unsigned int post_fused;         // fused launches since creation (emap_post_fused_launches)
  // The flag plane: one byte per cell in the storage order of cells.hot (ncells_alloc bytes, TRAV_FLAG_*), made the first time a pass goes
  // along with POST_OUT_TRAV.  It lives from that k_post_hist launch to the k_tile_count of the same frame (count_impl) and means nothing
  // outside it: every other reader of traversability takes the word in the hot half, behind a full pass.
  unsigned char* trav_flag;
  BinGeo bg; BinRec* bin_recs; size_t bin_recs_cap; bool bin_strip;
  float4* bin_own; size_t bin_own_cap; unsigned int* bin_own_cnt;   // staged 16-byte records (BinStg: emap_binned.hip) of the owned points per block (strip contexts without a visibility pass); bin_own_cnt: BIN_MAX_B words, sized once
  unsigned int* bin_hist; size_t bin_hist_cap; unsigned int* bin_tile_total; unsigned int* bin_tile_start;
  // The semantic fusion declared for the NEXT whole frame (emap_frame_semantics): run inside the frame.  A frame that can CARRIES the
  // channels in 32-byte sorted records (bin_rs = 2, carry: which columns) and fuses them in the tile kernel itself;
  // every other frame runs the stand-alone semantic kernels before it returns -- the result is the same either way.
  bool fsem_set; int fsem_keep_counts; SemSpec fsem;
  int bin_rs; SemCarry carry;      // stride of the current frame's sorted records in 16-byte units; the carried columns (on = 0: none)
  // semantic layers (planar float planes + double / uint32 accumulators), allocated on demand
  float* img_uv; unsigned char* img_valid; float* img_buf; size_t img_cap;   // camera path
  double img_tol; bool img_tol_set;   // tolerance_z_collision of the occlusion walk (0.10 unless emap_image_set_tolerance was called)
  float* sem_alpha;   // class_bayesian pseudo-counts (the reference's persistent new_map layers), sem_layers planes, on demand
  int sem_layers; float* sem; double* sem_sums; unsigned int* sem_col; unsigned int* cnt_plane;
  // point cloud
  float* pts_dev[2]; size_t pts_cap[2];    // owned device buffers (floats), ping-pong between consecutive uploads
  float* pts_pin[2]; size_t pin_cap[2];    // pinned host slots the clouds are converted / copied into
  hipEvent_t ev_copied[2], ev_used[2];     // DMA of slot done (copy stream) / the frame that read the slot's device buffer done (main stream)
  int up_slot; bool up_used[2]; hipStream_t copy_stream; emap_host::Workers* workers;
  emap_host::BoundCloud cloud;
  bool pts_bucketed; float bucket_R[9], bucket_t[3]; int bucket_org_r;   // the bound cloud only holds the points that can land in this strip's rows under this pose (emap_upload_points_strip)
  int* tail_idx; size_t tail_idx_cap; unsigned char* tail_flags; size_t tail_flags_cap;
  // the doors that produce their cloud on the device (depth image, PointCloud2 message): the caller's bytes pass through cloud_stage,
  // the cloud the kernel writes lives in ONE owned buffer (stream order: the kernels of the frame before precede the overwrite).  Only one
  // cloud is bound at a time, so both doors share them.
  emap_host::Stage cloud_stage; float* own_cloud; size_t own_cloud_cap;      // floats
  // image message input: a Stage of the camera path's OWN -- never cloud_stage or own_cloud, whose cloud stays bound while a camera
  // frame runs and which the small frames in flight keep raw pointers into
  emap_host::Stage image_stage;
  // GridMap message output (emap_api_gridmsg.hip): the planes k_grid_map writes, grown on demand (`scratch` stays the single plane it is)
  float* grid_buf; size_t grid_cap;                           // floats
  // publish-time plugins on resident planes (emap_api_plugchain.hip): plane_n planes of cell_n x cell_n floats, each the RAW output of a
  // plugin (logical order, border included) -- what PluginManager.layers[k] holds; the scratch planes, counters and reduction words of a
  // chain, one set per op, grown on demand
  float* plane_buf; int plane_n, plane_cap;
  float* chain_buf; size_t chain_cap; unsigned int* chain_cnt; size_t chain_cnt_cap; float* chain_red; size_t chain_red_cap;   // floats / words
  unsigned char* chain_inp; size_t chain_inp_cap;      // bytes: the byte images, fronts state and range records of the chain's inpaint ops, one set per op
  double* chain_pca; size_t chain_pca_cap;            // doubles: partial sums, means, moments, eigenvectors and score ranges of the chain's FEATURES_PCA ops, one set per op
  // safety-polygon service on the device (emap_api_polysafe.hip): ONE device buffer -- the uploaded tables (flag word, polygons, vertex cells,
  // work items), the part records, and the verdicts and row extremes that travel back -- and one pinned host buffer the tables are built in
  // and the results land in; both grown on demand, no allocation per call
  unsigned char* poly_buf; size_t poly_cap; unsigned char* poly_pin; size_t poly_pin_cap;      // bytes
  // submap service on the device (emap_api_submap.hip): the uploaded tables (windows, work items) on the device and in the pinned buffer
  // they are built in, and the packed planes k_grid_windows writes; all grown on demand, no allocation per call
  unsigned char* sub_tab; size_t sub_tab_cap; unsigned char* sub_pin; size_t sub_pin_cap;      // bytes
  float* sub_out; size_t sub_out_cap;                         // floats
  // point-cloud output on the device (emap_api_cloudout.hip): ONE device buffer -- the count word, the position tables, the mask words and
  // their offsets --, the pinned buffer the tables are built in and the count lands in, and the records k_cloud_write packs; all grown
  // on demand, no allocation per call
  unsigned char* cloud_tab; size_t cloud_tab_cap; unsigned char* cloud_pin; size_t cloud_pin_cap;      // bytes
  float* cloud_out; size_t cloud_out_cap;                     // floats
  // plane segmentation on the device (emap_api_planeseg.hip): ONE device buffer for the per-cell planes, the mask and offset words and
  // the head words (PlaneBufs, emap_launch.h), the slots of the labels that get a plane -- sized by how many there ARE, known after the
  // first wait -- and the pinned buffer the head words and the slots land in; all grown on demand, no allocation per call
  unsigned char* pseg_buf; size_t pseg_cap; unsigned char* pseg_pin; size_t pseg_pin_cap;      // bytes
  PlaneSlot* pseg_slots; size_t pseg_slots_cap;               // slots
  // planar terrain on the device (emap_api_terrain.hip): ONE device buffer -- the uploaded tables (TerrainTab, emap_launch.h), the float
  // planes of the pre- and postprocessing and the links, roots and keys of the NaN components -- and the pinned buffer the tables are
  // built in; both grown on demand, no allocation per call
  unsigned char* terr_buf; size_t terr_cap; unsigned char* terr_pin; size_t terr_pin_cap;      // bytes
  // planar regions on the device (emap_api_regions.hip): the buffer sized by the pixels of the traced images (RegionBufs, emap_launch.h),
  // the buffer sized by the cracks -- known after the first wait -- (RegionCracks) and the pinned buffer the counts land in; all grown on
  // demand, no allocation per call.  The call reads the labels of the last segmentation where they lie: pseg_labels points into
  // pseg_buf (PlaneBufs::parent, M x M, pseg_n_labels components) and is valid from the moment planeseg_segment has the final labels in
  // place until the buffer is carved again (planeseg_source), the map is cleared or it is shifted; nullptr: no valid labels
  unsigned char* reg_buf; size_t reg_cap; unsigned char* reg_cracks; size_t reg_cracks_cap; unsigned char* reg_pin; size_t reg_pin_cap;      // bytes
  const int* pseg_labels; int pseg_n_labels;
  // frame state
  bool use_override; double sum_override; unsigned int cnt_override;
  bool committed;
  bool stage_timing; hipEvent_t ev[ST_N + 1]; float stage_ms[ST_N];
  hipEvent_t t0, t1;
  bool want_ray_stats;
  // row-strip communicator (emap_comm_init): RCCL resolved at run time, exchange on its own stream so that it overlaps the interior stencils
  struct RcclApi* rccl; struct ncclComm* comm; int comm_rank, comm_world;      // (both opaque here: emap_api_comm.hip)
  float* gather_buf;            // cell_n x cell_n plane of emap_comm_gather_layer (on demand)
  // rays by ray (multi-GPU frames with a visibility pass): the replicated ray window around the sensor (emap_device.h: Win)
  int ray_mode;                 // 0 auto (by ray from 2048^2 cells on), 1 always by row, 2 by ray whenever the frame allows it
  bool byray_allreduce;         // the communicator's by-ray exchange: three all-reduces instead of the owners' sends / receives (emap_comm_init)
  size_t wire_bytes;            // payload of the last by-ray frame's three all-reduces (bytes per rank)
  int ray_par;                  // parity of the k_ray_apply launches (FrameDev::quiet_sum)
  unsigned int* win_state; unsigned int* win_rec; unsigned long long* win_bits; float* win_thr; long long* win_dh; unsigned int* win_key; long win_cap;
  long long* win_red_dh; unsigned int* win_red_key;      // by-ray effects reduced to the owners: (world - 1) parts of win_cap cells each
  hipStream_t comm_stream; hipEvent_t ev_ready, ev_done; double* comm_sums;   // [0..1] local err_sum / err_cnt, [2..3] totals, [4..36) emap_comm_allreduce_host
  // the un-shifted normal planes after a row shift (normal_exchange): a row-aligned copy of the rows this strip's cells belong to
  std::vector<int> cut_begin, cut_count;   // every rank's owned PHYSICAL rows (gathered by emap_comm_init)
  float* nlag_buf; size_t nlag_cap;        // 3 planes of row_count x cell_n
  bool cuts_ok;                            // the gathered strips tile the map
  std::string err;
};

#define CK(call)                                                                                         \
  do { hipError_t e_ = (call);                                                                           \
       if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return EMAP_ERR_HIP; } } while (0)
#define CKARG(cond, msg) do { if (!(cond)) { if (ctx) ctx->err = msg; return EMAP_ERR_INVALID; } } while (0)

// What one frame (frame_impl: emap_update, emap_update_sharded) decided, handed to the stage helpers it calls.  It lives on the
// frame's stack: an error on the way leaves nothing behind for the next call.  The staged entry points pass nullptr: the per-tile
// error statistics are gathered, plain 16-byte records sorted, the gate runs on its own, the rays march by row over the committed
// snapshot, nothing is folded.
struct Frame {
  bool gate_possible;      // the drift gate can fire (elevation_mapping.py:346-349); if not, the per-tile error statistics are skipped
                           // (they could not have any effect; err_sum / err_cnt report 0)
  bool fold_gate;          // whole map on the atomic path: the gate rides in k_count's last workgroup (cnt_sync: its ticket words)
  bool carry;              // the sort may carry the declared semantic channels in 32-byte records (frame_sem_begin)
  bool by_ray;             // sharded frame whose visibility pass marches by ray (rays_by_ray_pass)
  bool rays_fused;         // the tile kernel committed + averaged, k_ray_apply follows the rays
  bool nlag;               // normal_exchange filled the row-aligned copy of the normal planes for the visibility pass
  GateArgs gate;           // the drift gate's inputs (k_count's fold, k_small_frame, gate_fold)
  GateFold gate_fold;      // sharded frame on the binned path: the decision on the all-reduced totals in the tile kernel's head (mode 0: k_gate ran)
  OverlapArgs ov;          // clear_overlap_map, folded into the kernel that rewrites the cells last (tile kernel, k_average or k_ray_apply)
};

// ---- the helpers that cross a file boundary ------------------------------------------------------------------------------------------
namespace emap_host {
// emap_api.hip
float q16(float x);
int sf_settle(emap_ctx* ctx);
int upload_setup(emap_ctx* ctx);
Pose make_pose(const emap_ctx* ctx, const float R[9], const float t[3]);
int flush_moves(emap_ctx* ctx);
int post_settle(emap_ctx* ctx);
int normal_row_lag(const emap_ctx* ctx);
int plugin_scratch(emap_ctx* ctx, size_t planes, int counters);
bool takes_bins(const emap_ctx* ctx, long n);
// emap_api_plugins.hip: get_idx of the reference's polygon kernel -- cell (*ix, *iy) of a world point, float16 quirk included
int polygon_cell(const emap_params& p, float x, float y, float cx, float cy, int* ix, int* iy);
// emap_api_semantic.hip: the frame's semantic fusion
int frame_sem_begin(emap_ctx* ctx, bool rays_on, Frame* fr);
int frame_sem_finish(emap_ctx* ctx, const float R[9], const float t[3], bool merged);
// emap_api_comm.hip: the exchange steps of a sharded frame
int drift_allreduce(emap_ctx* ctx);
int halo_exchange_start(emap_ctx* ctx);
int normal_exchange(emap_ctx* ctx);
bool rays_by_ray(const emap_ctx* ctx);
int rays_by_ray_pass(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f);
// emap_api_planeseg.hip: the two halves of emap_plane_segmentation -- the source layer as a dense plane in the context's buffers (grown
// and carved: *B, the call's constants: *A), and the segmentation of the M x M floats B.src points to (two waits; `who` ends in ": ")
int planeseg_source(emap_ctx* ctx, const emap_grid_layer_ex& source, const emap_plane_params& p, PlaneArgs* A, PlaneBufs* B);
int planeseg_segment(emap_ctx* ctx, const std::string& who, const emap_plane_params& p, const PlaneArgs& A, const PlaneBufs& B, int32_t* host_labels, float* host_normals,
                     emap_plane_record* host_planes, int64_t capacity_planes, int32_t* n_labels, int64_t* n_planes);
// getStructuringElement(MORPH_ELLIPSE, (k, k)), k odd and at most EM_TERRAIN_KERNEL_MAX: row a covers the columns [lo[a], hi[a]) -- the
// element of the planar terrain's closing and dilation and of the planar regions' margin erosion
inline void ellipse_spans(int k, TerrainSpans* sp) {
  memset(sp, 0, sizeof *sp);
  const int r = k / 2, c = k / 2;
  for (int a = 0; a < k; ++a) {
    const int dy = a - r;
    const int dx = r ? (int)std::rint((double)c * std::sqrt((double)(r * r - dy * dy) / (double)(r * r))) : 0;
    sp->lo[a] = (signed char)(c - dx > 0 ? c - dx : 0);
    sp->hi[a] = (signed char)(c + dx + 1 < k ? c + dx + 1 : k);
  }
}
// emap_api_depth.hip: the next slot of cloud_stage and the owned cloud (tot floats) of the doors that produce their cloud
int owned_cloud_prepare(emap_ctx* ctx, size_t pin_bytes, size_t dev_bytes, long tot);

// Stage (above).  stage_next: the other slot becomes the current one, its DMA of two calls ago is waited for, and it holds pin_bytes,
// the device buffer dev_bytes.  stage_send: `bytes` from src into the current slot (one memcpy up to 2 MB, beyond that the worker threads
// chunk by chunk) and on to the device buffer, a DMA behind each chunk, in order on ctx->stream; src == nullptr sends what the caller
// placed in the slot itself, in one DMA.
int stage_next(emap_ctx* ctx, Stage* s, size_t pin_bytes, size_t dev_bytes);
int stage_send(emap_ctx* ctx, Stage* s, const void* src, size_t bytes);
void stage_free(Stage* s);

// A context buffer of `need` elements, grown on demand; the old contents are NOT kept.  Kernels enqueued earlier may still read the old
// buffer, so the stream is drained before it is freed -- unless the caller's own events cover every reader (Grow::covered: the
// ping-pong buffers of upload_impl) or the buffer is a pinned host slot whose DMA the caller has waited for (Grow::pinned).  An
// allocation that fails leaves *buf == nullptr, *cap == 0.
enum class Grow { drain, covered, pinned };
template <class T> int grow(emap_ctx* ctx, T** buf, size_t* cap, size_t need, Grow how = Grow::drain) {
  if (need <= *cap) return EMAP_OK;
  if (how == Grow::drain) CK(hipStreamSynchronize(ctx->stream));
  if (*buf) CK(how == Grow::pinned ? hipHostFree(*buf) : hipFree(*buf));
  *buf = nullptr; *cap = 0;
  void* m = nullptr;
  CK(how == Grow::pinned ? hipHostMalloc(&m, sizeof(T) * need, hipHostMallocDefault) : hipMalloc(&m, sizeof(T) * need));
  *buf = static_cast<T*>(m); *cap = need;
  return EMAP_OK;
}

// Binds a de-interleaved cloud: xyz (n, 3) at `xyz`, K channels (n, K) at `chan` (CloudLayout: xyz + chan_off; or a buffer of the
// caller's), whole and unbucketed unless the caller says otherwise afterwards.  (Interleaved rows: emap_set_points_device.)
inline void bind_split_cloud(emap_ctx* ctx, const float* xyz, const float* chan, long n, long n_all, int K) {
  ctx->cloud = BoundCloud{xyz, n, 3, n_all, ChanView{K ? chan : xyz, K ? K : 3, K ? 3 : 0}, 3 + K};
  ctx->pts_bucketed = false;
}

// The layer table of the output doors on the published map (LayerTab, emap_publish_tile.h).  check_layer_entry: one entry of a caller's
// table, refused with the caller's name (`who` ends in ": ") in front; plugin_ok admits EMAP_GRID_PLUGIN.
inline int check_layer_entry(emap_ctx* ctx, const std::string& who, int kind, int index, int flags, bool plugin_ok) {
  if (plugin_ok) CKARG(kind >= EMAP_GRID_BUILTIN && kind <= EMAP_GRID_PLUGIN, who + "kind must be 0 (built-in), 1 (semantic), 2 (normal colour) or 3 (plugin plane)");
  else CKARG(kind >= EMAP_GRID_BUILTIN && kind <= EMAP_GRID_NORMAL_COLOR, who + "kind must be 0 (built-in), 1 (semantic) or 2 (normal colour)");
  CKARG(kind != EMAP_GRID_BUILTIN || (index >= 0 && index <= 8), who + "a built-in index must lie in 0 .. 8");
  CKARG(kind != EMAP_GRID_SEMANTIC || (index >= 0 && index < ctx->sem_layers), who + "semantic layer is not configured");
  CKARG(kind != EMAP_GRID_PLUGIN || (index >= 0 && index < ctx->plane_n), who + "plugin plane is not reserved (emap_plugin_planes)");
  CKARG(kind == EMAP_GRID_PLUGIN ? (flags & ~(EMAP_GRID_FILL_NAN | EMAP_GRID_ADD_Z)) == 0 : flags == 0, who + "flags: FILL_NAN / ADD_Z, on a plugin plane only");
  return EMAP_OK;
}
// tab_init: an empty table on the context's planes; tab_put: appends a checked entry and returns its place; tab_finish: once all are in.
inline LayerTab tab_init(const emap_ctx* ctx, float center_z, int only_above) {
  LayerTab t; memset(&t, 0, sizeof t);
  t.only_above = only_above ? 1 : 0; t.center_z = center_z;
  t.plane = ctx->ncells_alloc; t.sem_plane = ctx->ncells_alloc; t.normal = ctx->normal; t.sem = ctx->sem; t.plug = ctx->plane_buf;
  return t;
}
inline int tab_put(LayerTab& t, int kind, int index, int flags) {
  const int l = t.n++;
  t.kind[l] = (unsigned char)kind; t.index[l] = kind == EMAP_GRID_NORMAL_COLOR ? 0 : index; t.flags[l] = (unsigned char)flags;
  t.need |= grid_need(kind, index);
  return l;
}
inline void tab_finish(LayerTab& t) {
  bool fill_nan = false;
  for (int l = 0; l < t.n; ++l) fill_nan = fill_nan || (t.flags[l] & EMAP_GRID_FILL_NAN);
  if (fill_nan && !(t.need & 3)) t.need |= 1;      // FILL_NAN reads is_valid: the hot half, unless the cold half (w mirrors it) is loaded anyway
}
}  // namespace emap_host

// Every entry point that reads or changes the map, the drift record or a cloud buffer settles the small frames in flight first
// (emap_api.hip: sf_settle); map shifts are lazy (emap_shift) and written out before anything but a frame kernel looks at the cells.
// The same door settles the last frame's pending stencil pass (post_settle): every entry point passes through SF_CHECK but the ones that
// make up the next frame or touch neither the map nor the stream (DESIGN.md section 5 lists them; tests/test_post_settle_surface.py
// holds the list).  SF_SETTLE_FRAMES: the small frames alone -- frame_impl, which decides about the pending pass itself.
#define SF_SETTLE_FRAMES() do { if (ctx->sf_count > 0) { int rc_sf_ = emap_host::sf_settle(ctx); if (rc_sf_) return rc_sf_; } } while (0)
#define SF_CHECK() do { SF_SETTLE_FRAMES(); if (ctx->post_pending) { int rc_ps_ = emap_host::post_settle(ctx); if (rc_ps_) return rc_ps_; } } while (0)
#define FLUSH() do { int rc_ = emap_host::flush_moves(ctx); if (rc_) return rc_; } while (0)
#define NEED_POINTS() do { if (!ctx->cloud.pts && ctx->cloud.n) { ctx->err = "no point cloud bound"; return EMAP_ERR_NO_POINTS; } } while (0)
