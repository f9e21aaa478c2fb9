// C ABI of the MI355X elevation-map fusion core, host side of the RGB / semantic layers (kernels: emap_semantic.hip, k_tile_semantic in
// emap_binned.hip): the layers' planes, the fusion a frame declares and runs, the reference's kernel factories on caller arrays,
// pointcloud_class_max and the camera path.
#include "emap_host.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace emap_host;

static_assert(offsetof(SemSpec, sum_K) == sizeof(emap_sem_spec), "emap_sem_spec is the leading part of SemSpec");

extern "C" {

// ---- RGB / semantic layers (EM/semantic_map.py, EM/fusion/pointcloud_{average,class_average,color}.py) -------------
int emap_semantic_configure(emap_ctx* ctx, int32_t n_layers) {
  CKARG(ctx && n_layers >= 0 && n_layers <= 64, "bad layer count"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long n = ctx->ncells_alloc;
  if (!ctx->cnt_plane) {
    CK(hipMalloc((void**)&ctx->cnt_plane, sizeof(unsigned int) * n));
    CK(hipMemsetAsync(ctx->cnt_plane, 0, sizeof(unsigned int) * n, ctx->stream));
    CK(hipMalloc((void**)&ctx->sem_col, sizeof(unsigned int) * n * 13));
    CK(hipMemsetAsync(ctx->sem_col, 0, sizeof(unsigned int) * n * 13, ctx->stream));
  }
  if (n_layers > ctx->sem_layers) {      // grow, KEEPING the existing layers (SemanticMap.add_layer, semantic_map.py:80-97): not emap_host::grow, which drops the old contents
    float* ns = nullptr; double* nq = nullptr;
    CK(hipMalloc((void**)&ns, sizeof(float) * n * n_layers));
    CK(hipMalloc((void**)&nq, sizeof(double) * n * n_layers));
    CK(hipMemsetAsync(ns, 0, sizeof(float) * n * n_layers, ctx->stream));
    CK(hipMemsetAsync(nq, 0, sizeof(double) * n * n_layers, ctx->stream));
    if (ctx->sem_layers > 0) CK(hipMemcpyAsync(ns, ctx->sem, sizeof(float) * n * ctx->sem_layers, hipMemcpyDeviceToDevice, ctx->stream));
    if (ctx->sem_alpha) {
      float* na = nullptr;
      CK(hipMalloc((void**)&na, sizeof(float) * n * n_layers));
      CK(hipMemsetAsync(na, 0, sizeof(float) * n * n_layers, ctx->stream));
      CK(hipMemcpyAsync(na, ctx->sem_alpha, sizeof(float) * n * ctx->sem_layers, hipMemcpyDeviceToDevice, ctx->stream));
      CK(hipStreamSynchronize(ctx->stream));
      CK(hipFree(ctx->sem_alpha)); ctx->sem_alpha = na;
    }
    CK(hipStreamSynchronize(ctx->stream));
    if (ctx->sem) CK(hipFree(ctx->sem));
    if (ctx->sem_sums) CK(hipFree(ctx->sem_sums));
    ctx->sem = ns; ctx->sem_sums = nq; ctx->sem_layers = n_layers;
  }
  return EMAP_OK;
}

static int ensure_alpha(emap_ctx* ctx) {
  if (ctx->sem_alpha || ctx->sem_layers == 0) return EMAP_OK;
  CK(hipMalloc((void**)&ctx->sem_alpha, sizeof(float) * ctx->ncells_alloc * ctx->sem_layers));
  CK(hipMemsetAsync(ctx->sem_alpha, 0, sizeof(float) * ctx->ncells_alloc * ctx->sem_layers, ctx->stream));
  return EMAP_OK;
}

// emap_sem_spec -> SemSpec, checked against the bound cloud and the configured layers
static int sem_spec_checked(emap_ctx* ctx, const emap_sem_spec* spec, SemSpec* out) {
  CKARG(spec->n_sum >= 0 && spec->n_sum <= SEM_MAX_CH && spec->n_col >= 0 && spec->n_col <= 4, "too many channels");
  CKARG(ctx->cnt_plane, "emap_semantic_configure must be called before the frame (the average pass records the counts)");
  for (int k = 0; k < spec->n_sum; ++k)
    CKARG(spec->sum_layer[k] >= 0 && spec->sum_layer[k] < ctx->sem_layers && spec->sum_chan[k] >= 3 && spec->sum_chan[k] < ctx->cloud.n_cols, "bad channel/layer index");
  for (int k = 0; k < spec->n_col; ++k)
    CKARG(spec->col_layer[k] >= 0 && spec->col_layer[k] < ctx->sem_layers && spec->col_chan[k] >= 3 && spec->col_chan[k] < ctx->cloud.n_cols, "bad colour channel/layer index");
  SemSpec& S = *out; memset(&S, 0, sizeof S); memcpy(&S, spec, sizeof *spec);
  int nk[4] = {0, 0, 0, 0};
  for (int k = 0; k < S.n_sum; ++k) { CKARG(S.sum_kind[k] >= 0 && S.sum_kind[k] <= 3, "bad fusion kind"); nk[S.sum_kind[k]]++; }
  int seen[4] = {0, 0, 0, 0};
  for (int k = 0; k < S.n_sum; ++k) {
    const int kind = S.sum_kind[k];
    S.sum_K[k] = kind >= 2 ? nk[kind] : 1;
    S.sum_q[k] = kind >= 2 ? seen[kind]++ : 0;
  }
  S.any_bayes = nk[2] > 0;
  // class_bayesian / bayesian_inference reproduce the reference's launch decode (element exists while id * K + q < N): the GLOBAL point
  // index and cloud size -- a cloud bucketed for a strip renumbers its points
  CKARG(!(ctx->pts_bucketed && (nk[2] + nk[3]) > 0), "a bucketed cloud (emap_upload_points_strip) cannot feed class_bayesian / bayesian_inference fusions: they decode the global point index");
  return EMAP_OK;
}
static int semantic_update_impl(emap_ctx* ctx, const float R[9], const float t[3], const SemSpec& S);

int emap_frame_semantics(emap_ctx* ctx, const emap_sem_spec* spec_or_null, int32_t keep_counts) {
  CKARG(ctx, "null ctx");
  ctx->fsem_set = false; ctx->fsem_keep_counts = keep_counts != 0;
  if (!spec_or_null || spec_or_null->n_sum + spec_or_null->n_col == 0) return EMAP_OK;
  CKARG(spec_or_null->n_sum >= 0 && spec_or_null->n_sum <= SEM_MAX_CH && spec_or_null->n_col >= 0 && spec_or_null->n_col <= 4, "too many channels");
  memset(&ctx->fsem, 0, sizeof ctx->fsem); memcpy(&ctx->fsem, spec_or_null, sizeof *spec_or_null);      // (checked against the cloud bound when the frame starts)
  ctx->fsem_set = true;
  return EMAP_OK;
}
// Start of a whole frame: check the declared fusion against the bound cloud and decide whether the frame's sort may CARRY the channels
// (32-byte records): kinds average / class_average and at most one colour channel, at most four channel columns, all within four
// consecutive columns of the cloud; no visibility pass (k_rays walks 16-byte records).  emap_count then settles it (tile-binned
// path, plain point passes: ensure_bins).  EMAP_SEM_CARRY=0: never (A/B and test hook).
extern "C++" int emap_host::frame_sem_begin(emap_ctx* ctx, bool rays_on, Frame* fr) {
  memset(&ctx->carry, 0, sizeof ctx->carry);
  if (!ctx->fsem_set) return EMAP_OK;
  emap_sem_spec raw; memcpy(&raw, &ctx->fsem, sizeof raw);
  SemSpec S;
  int rc = sem_spec_checked(ctx, &raw, &S);
  if (rc) { ctx->fsem_set = false; return rc; }
  ctx->fsem = S;
  if (S.any_bayes && (rc = ensure_alpha(ctx))) { ctx->fsem_set = false; return rc; }
  static const bool off = getenv("EMAP_SEM_CARRY") && atoi(getenv("EMAP_SEM_CARRY")) == 0;
  if (off || rays_on || S.n_sum > 4 || S.n_col > 1 || S.n_sum + S.n_col == 0) return EMAP_OK;
  int cmin = 1 << 30, cmax = -1;
  for (int k = 0; k < S.n_sum; ++k) { if (S.sum_kind[k] > 1) return EMAP_OK; cmin = std::min(cmin, S.sum_chan[k]); cmax = std::max(cmax, S.sum_chan[k]); }
  for (int k = 0; k < S.n_col; ++k) { cmin = std::min(cmin, S.col_chan[k]); cmax = std::max(cmax, S.col_chan[k]); }
  if (cmax - cmin >= 4) return EMAP_OK;
  fr->carry = true;
  ctx->carry.c0 = cmin; ctx->carry.ncols = ctx->cloud.n_cols;
  // the de-interleaved (N, 4) channel matrix of an uploaded cloud: one aligned 16-byte load per point
  ctx->carry.on = (ctx->cloud.chan.stride == 4 && ctx->cloud.chan.col0 == cmin && ((uintptr_t)ctx->cloud.chan.p & 15) == 0) ? 2 : 1;
  return EMAP_OK;
}
// End of the frame's fusion stages: whatever the tile kernel did not fuse itself (merged) runs now (the frame's counts are in cnt_plane)
extern "C++" int emap_host::frame_sem_finish(emap_ctx* ctx, const float R[9], const float t[3], bool merged) {
  if (!ctx->fsem_set) return EMAP_OK;
  ctx->fsem_set = false;
  if (merged) return EMAP_OK;
  return semantic_update_impl(ctx, R, t, ctx->fsem);
}

int emap_semantic_update(emap_ctx* ctx, const float R[9], const float t[3], const emap_sem_spec* spec) {
  CKARG(ctx && R && t && spec, "null argument"); SF_CHECK(); NEED_POINTS();
  SemSpec S;
  int rc = sem_spec_checked(ctx, spec, &S);
  if (rc) return rc;
  return semantic_update_impl(ctx, R, t, S);
}
static int semantic_update_impl(emap_ctx* ctx, const float R[9], const float t[3], const SemSpec& S) {
  CK(hipSetDevice(ctx->device));
  if (S.any_bayes) { int rc = ensure_alpha(ctx); if (rc) return rc; }
  if (ctx->frame_binned) {   // the frame's tile-sorted records are still valid: reduce in LDS, no global atomics
    if (ctx->split.on && ctx->split.cap > 0 && !ctx->sem_split_mem && sem_split_possible(S)) {      // the frame listed heavy tiles: their semantic sums are shared too
      void* m = nullptr;
      CK(hipMalloc(&m, sem_split_bytes(SEM_SPLIT_SLOTS)));
      if (hipMemsetAsync(m, 0, sem_split_bytes(SEM_SPLIT_SLOTS), ctx->stream) != hipSuccess) { hipFree(m); ctx->err = "hipMemsetAsync(semantic split scratch)"; return EMAP_ERR_HIP; }
      ctx->sem_split_mem = m;
    }
    launch_tile_semantic(ctx->stream, ctx->kp, ctx->bg, S, ctx->bin_recs, ctx->bin_rs, ctx->carry.on ? ctx->carry.c0 : -1, ctx->bin_tile_start, ctx->cloud.chan, ctx->cloud.n,
                         ctx->cnt_plane, ctx->sem, ctx->sem_alpha, ctx->ncells_alloc, ctx->split, ctx->sem_split_mem, SEM_SPLIT_SLOTS);
    CK(hipGetLastError());
    return EMAP_OK;
  }
  launch_sem_points(ctx->stream, ctx->kp, make_pose(ctx, R, t), S, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cloud.chan, ctx->sem_sums, ctx->sem_col, ctx->ncells_alloc);
  launch_sem_finalize(ctx->stream, ctx->kp, S, ctx->cnt_plane, ctx->sem_sums, ctx->sem_col, ctx->sem, ctx->sem_alpha, ctx->ncells_alloc);
  CK(hipGetLastError());
  return EMAP_OK;
}

// ---- the reference's semantic kernel factories on caller arrays (EM/kernels/custom_semantic_kernels.py) ------------------------
// Host arrays in, host arrays out (the factories of the compat package hand NumPy arrays over); device buffers live for the call.
int emap_semantic_accumulate(emap_ctx* ctx, int32_t op, const float* points, int64_t n_rows, int32_t stride, const int32_t* pcl_chan,
                             const int32_t* map_lay, int32_t n_ch, int64_t size, int64_t cells, void* newmap_inout, int32_t newmap_layers,
                             const float* max_pt, const int32_t* max_id, int32_t n_max) {
  CKARG(ctx && points && newmap_inout && op >= 0 && op <= 4, "bad argument");
  CKARG(n_rows >= 0 && stride >= 3 && n_ch >= 1 && n_ch <= 64 && size >= 0 && cells > 0 && newmap_layers >= 1, "bad shape");
  CKARG(op == 2 ? (max_pt && max_id && n_max >= 1 && size <= n_rows) : (pcl_chan && map_lay && size <= n_rows * (int64_t)n_ch), "bad channel description / size"); SF_CHECK();
  // The index CONTENTS decide which plane / column a thread touches: check them on the host before anything is
  // launched -- a bad index from a caller of the kernel factories must not write into other device memory of the shared context.
  if (op == 2) {
    for (int64_t k = 0; k < size * (int64_t)n_max; ++k) CKARG(max_id[k] >= 0 && max_id[k] < newmap_layers, "sum_max: class id outside the planes of newmap");
  } else {
    for (int k = 0; k < n_ch; ++k) {
      CKARG(pcl_chan[k] >= 0 && pcl_chan[k] < stride, "pcl channel index outside the point rows");
      CKARG(op == 1 || op == 4 || (map_lay[k] >= 0 && map_lay[k] < newmap_layers), "map layer index outside the planes of newmap");
    }
    CKARG(op != 1 || n_ch <= newmap_layers, "sum_compact: newmap needs one plane per channel");
    CKARG(op != 4 || 3 * n_ch + 1 <= newmap_layers, "add_color: the colour map needs 3 n_ch + 1 planes");
  }
  CK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf P, PC, ML, MP, MI, NM;
  CK(P.put(points, sizeof(float) * (size_t)n_rows * stride, st, nullptr));
  if (pcl_chan) { CK(PC.put(pcl_chan, sizeof(int) * n_ch, st, nullptr)); CK(ML.put(map_lay, sizeof(int) * n_ch, st, nullptr)); }
  if (op == 2) { CK(MP.put(max_pt, sizeof(float) * (size_t)n_rows * n_max, st, nullptr)); CK(MI.put(max_id, sizeof(int) * (size_t)n_rows * n_max, st, nullptr)); }
  CK(NM.put(newmap_inout, 4 * (size_t)newmap_layers * cells, st, newmap_inout));
  SemRaw A; memset(&A, 0, sizeof A);
  A.op = op; A.stride = stride; A.K = n_ch; A.n_max = n_max; A.size = size; A.cells = cells;
  launch_semraw_acc(st, A, (const float*)P.d, (const int*)PC.d, (const int*)ML.d, (const float*)MP.d, (const int*)MI.d, (float*)NM.d, (unsigned int*)NM.d);
  CK(hipGetLastError());
  CK(NM.get(st));
  CK(hipStreamSynchronize(st));
  return EMAP_OK;
}

int emap_semantic_finalize(emap_ctx* ctx, int32_t op, void* newmap_inout, int32_t newmap_layers, const int32_t* map_lay, int32_t n_ch, int64_t size,
                           int64_t cells, const float* new_elmap3, const float* sum_mean, int32_t sum_layers, float* map_inout, int32_t map_layers, double alpha) {
  CKARG(ctx && newmap_inout && map_lay && map_inout && op >= 0 && op <= 3, "bad argument");
  CKARG(n_ch >= 1 && n_ch <= 64 && size >= 0 && size <= cells * (int64_t)n_ch && cells > 0 && newmap_layers >= 1 && map_layers >= 1, "bad shape");
  CKARG(op == 3 || new_elmap3, "the accepted-point counts (new_elmap plane 2) are needed");
  CKARG(op != 2 || (sum_mean && sum_layers >= n_ch), "bayesian_inference needs sum_mean"); SF_CHECK();
  for (int k = 0; k < n_ch; ++k)      // (colour: newmap is the colour map, indexed by channel; every other op indexes newmap AND map with map_lay)
    CKARG(map_lay[k] >= 0 && map_lay[k] < map_layers && (op == 3 || map_lay[k] < newmap_layers), "map layer index outside the planes of map / newmap");
  CKARG(op != 3 || 3 * n_ch + 1 <= newmap_layers, "color_average: the colour map needs 3 n_ch + 1 planes");
  CK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf NM, ML, EL, SM, MP;
  CK(NM.put(newmap_inout, 4 * (size_t)newmap_layers * cells, st, op == 2 ? newmap_inout : nullptr));
  CK(ML.put(map_lay, sizeof(int) * n_ch, st, nullptr));
  if (new_elmap3) CK(EL.put(new_elmap3, sizeof(float) * 3 * (size_t)cells, st, nullptr));
  if (sum_mean) CK(SM.put(sum_mean, sizeof(float) * (size_t)sum_layers * cells, st, nullptr));
  CK(MP.put(map_inout, sizeof(float) * (size_t)map_layers * cells, st, map_inout));
  SemRaw A; memset(&A, 0, sizeof A);
  A.op = op; A.K = n_ch; A.size = size; A.cells = cells; A.alpha = alpha;
  launch_semraw_fin(st, A, (float*)NM.d, (const unsigned int*)NM.d, (const int*)ML.d, (const float*)EL.d, (const float*)SM.d, (float*)MP.d);
  CK(hipGetLastError());
  CK(NM.get(st)); CK(MP.get(st));
  CK(hipStreamSynchronize(st));
  return EMAP_OK;
}

// ---- pointcloud_class_max (EM/fusion/pointcloud_class_max.py:80-126; kernels: emap_semantic.hip) ------------------------------
// The class-id planes (the reference's elements_to_shift["id_max"]) live in the layers' persistent planes (sem_alpha): they move
// with the map and read back through emap_semantic_get_alpha as uint32 bit patterns.  `prev_unique` is the fusion's unique_id array
// of the previous frame ([0] before the first: :59).  The reference gathers unique_id[id_max] (:85) -- the planes hold class VALUES
// and the table is indexed with them; positions beyond the table wrap around (CuPy's integer-array indexing), reproduced here and
// pinned by the reference's own statements executed from its file (tests/golden/class_max_ref66.npz).
int emap_semantic_class_max(emap_ctx* ctx, const float R[9], const float t[3], int32_t n_ch, const int32_t* chan, const int32_t* layer,
                            const uint32_t* prev_unique, int32_t n_prev, uint32_t* unique_out, int32_t unique_cap, int32_t* n_unique_out) {
  CKARG(ctx && R && t && chan && layer && unique_out && n_unique_out && n_ch >= 1 && n_ch <= 8 && n_prev >= 0 && (n_prev == 0 || prev_unique), "bad argument"); SF_CHECK();
  // the id set and the planes zeroed between two layers are properties of the WHOLE map: a row strip would take them from its own rows
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "class_max: single-strip contexts only");
  NEED_POINTS();
  for (int k = 0; k < n_ch; ++k)
    CKARG(layer[k] >= 0 && layer[k] < ctx->sem_layers && chan[k] >= 3 && chan[k] < ctx->cloud.n_cols, "bad channel/layer index");
  CK(hipSetDevice(ctx->device));
  { int rc = ensure_alpha(ctx); if (rc) return rc; }
  hipStream_t st = ctx->stream;
  CmaxSpec S; memset(&S, 0, sizeof S);
  S.n = n_ch; for (int k = 0; k < n_ch; ++k) { S.chan[k] = chan[k]; S.layer[k] = layer[k]; }
  const long plane = ctx->ncells_alloc;
  // (1) the ids of this frame and of the map
  DevBuf b_seen;
  CK(b_seen.alloc(2 * 65536));
  unsigned char* const d_seen = (unsigned char*)b_seen.d;
  CK(hipMemsetAsync(d_seen, 0, 2 * 65536, st));
  launch_cmax_ids(st, ctx->kp, S, ctx->cloud.chan, ctx->cloud.n, ctx->sem_alpha, plane, d_seen, d_seen + 65536);
  CK(hipGetLastError());
  std::vector<unsigned char> seen(2 * 65536);
  CK(hipMemcpyAsync(seen.data(), d_seen, 2 * 65536, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  const uint32_t zero_id = 0;
  if (n_prev == 0) { prev_unique = &zero_id; n_prev = 1; }
  std::vector<unsigned char> in_set(65536, 0);
  for (int v = 0; v < 65536; ++v) {
    if (seen[v]) in_set[v] = 1;                                                            // unique(pt_id) (:84)
    if (seen[65536 + v] && prev_unique[v % n_prev] < 65536u) in_set[prev_unique[v % n_prev]] = 1;      // unique(unique_id[id_max]) (:85): positions beyond the table wrap around, like CuPy's integer-array gather
  }
  std::vector<uint32_t> uniq; std::vector<int> pos(65536, 0);
  for (int v = 0; v < 65536; ++v) if (in_set[v]) { pos[v] = (int)uniq.size(); uniq.push_back((uint32_t)v); }
  const int U = (int)uniq.size();
  CKARG(U <= unique_cap, "unique_out too small for the class ids of this frame");
  const size_t sum_bytes = sizeof(long long) * (size_t)U * plane;
  CKARG(sum_bytes <= ((size_t)16 << 30), "class_max: (classes x cells) probability sums beyond 16 GB");
  // (2) probability sums per (class, cell)
  DevBuf b_sum, b_pos, b_uniq, b_flags, b_new;
  CK(b_sum.alloc(sum_bytes));
  CK(b_pos.alloc(sizeof(int) * 65536));
  CK(b_uniq.alloc(sizeof(unsigned int) * U));
  CK(b_flags.alloc(2 * (size_t)U));
  CK(b_new.alloc(sizeof(float) * (size_t)n_ch * plane));
  long long* const d_sum = (long long*)b_sum.d; int* const d_pos = (int*)b_pos.d; unsigned int* const d_uniq = (unsigned int*)b_uniq.d;
  unsigned char* const d_flags = (unsigned char*)b_flags.d; float* const d_new = (float*)b_new.d;
  CK(hipMemsetAsync(d_sum, 0, sum_bytes, st));
  CK(hipMemsetAsync(d_flags, 0, 2 * (size_t)U, st));
  CK(hipMemsetAsync(d_new, 0, sizeof(float) * (size_t)n_ch * plane, st));
  CK(hipMemcpyAsync(d_pos, pos.data(), sizeof(int) * 65536, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(d_uniq, uniq.data(), sizeof(unsigned int) * U, hipMemcpyHostToDevice, st));
  launch_cmax_sum(st, ctx->kp, make_pose(ctx, R, t), S, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cloud.chan, d_pos, d_sum, plane);
  // (3) + (4): per layer the maximum and its class, the winners' planes zeroed in between; then the normalisation
  launch_cmax_select(st, ctx->kp, S, U, d_sum, plane, d_flags, d_flags + U, d_uniq, d_new, ctx->sem_alpha, ctx->sem);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(st));              // the host vectors and the temporaries end with the call
  memcpy(unique_out, uniq.data(), sizeof(uint32_t) * U);
  *n_unique_out = U;
  return EMAP_OK;
}

static int sem_view(emap_ctx* ctx, float* planes, int32_t layer, float* host, bool to_device) { SF_CHECK();   // semantic layers share the map's origin
  const size_t bytes = sizeof(float) * (size_t)ctx->strip.row_count * ctx->prm.cell_n;
  if (to_device) CK(hipMemcpyAsync(ctx->scratch, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  launch_plane_view(ctx->stream, ctx->kp, ctx->kp.org_r, ctx->kp.org_c, planes + (long)layer * ctx->ncells_alloc, ctx->scratch, to_device);
  CK(hipGetLastError());
  if (!to_device) CK(hipMemcpyAsync(host, ctx->scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}
int emap_semantic_get_alpha(emap_ctx* ctx, int32_t layer, float* host_out) {
  CKARG(ctx && host_out && layer >= 0 && layer < ctx->sem_layers, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  int rc = ensure_alpha(ctx); if (rc) return rc;
  return sem_view(ctx, ctx->sem_alpha, layer, host_out, false);
}
int emap_semantic_set_alpha(emap_ctx* ctx, int32_t layer, const float* host_in) {
  CKARG(ctx && host_in && layer >= 0 && layer < ctx->sem_layers, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  int rc = ensure_alpha(ctx); if (rc) return rc;
  return sem_view(ctx, ctx->sem_alpha, layer, const_cast<float*>(host_in), true);
}

int emap_semantic_get_layer(emap_ctx* ctx, int32_t layer, float* host_out) {
  CKARG(ctx && host_out && layer >= 0 && layer < ctx->sem_layers, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  return sem_view(ctx, ctx->sem, layer, host_out, false);
}
int emap_semantic_set_layer(emap_ctx* ctx, int32_t layer, const float* host_in) {
  CKARG(ctx && host_in && layer >= 0 && layer < ctx->sem_layers, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  return sem_view(ctx, ctx->sem, layer, const_cast<float*>(host_in), true);
}
int emap_semantic_clear(emap_ctx* ctx) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  if (ctx->sem_layers > 0) CK(hipMemsetAsync(ctx->sem, 0, sizeof(float) * ctx->ncells_alloc * ctx->sem_layers, ctx->stream));
  return EMAP_OK;
}

// ---- camera path (EM/elevation_mapping.py:468-562, EM/kernels/custom_image_kernels.py) -------------------------------
static bool cam_cell_ok(float v) { return std::isfinite(v) && v == truncf(v) && fabsf(v) <= (float)EM_CAM_CELL_MAX; }
int emap_image_correspondence(emap_ctx* ctx, float x1, float y1, float z1, const float P[12], const float K[9], const float D[5],
                              float image_height, float image_width, const float center[3]) {
  CKARG(ctx && P && K && D && center, "null argument");
  // the walk of k_image_corr terminates by reaching (x1, y1) exactly: refuse, before anything is launched, a camera cell it cannot reach
  // (not finite, not integer valued) or would take too long to reach (EM_CAM_CELL_MAX).  The reference does not terminate there.
  CKARG(cam_cell_ok(x1) && cam_cell_ok(y1), "camera cell (x1, y1) must be integer valued and within +-65536 cells");
  SF_CHECK();
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "camera path: single-strip contexts only");
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t L = (size_t)ctx->prm.cell_n * ctx->prm.cell_n;
  if (!ctx->img_uv) { CK(hipMalloc((void**)&ctx->img_uv, sizeof(float) * 2 * L)); CK(hipMalloc((void**)&ctx->img_valid, L)); }
  CamArgs A;
  memcpy(A.P, P, sizeof A.P); memcpy(A.K, K, sizeof A.K); memcpy(A.D, D, sizeof A.D); memcpy(A.center, center, sizeof A.center);
  A.x1 = x1; A.y1 = y1; A.z1 = z1; A.ih = image_height; A.iw = image_width; A.tol = ctx->img_tol_set ? ctx->img_tol : 0.10;
  launch_image_corr(ctx->stream, ctx->kp, A, ctx->cells, ctx->img_uv, ctx->img_valid);
  CK(hipGetLastError());
  return EMAP_OK;
}
int emap_image_get_correspondence(emap_ctx* ctx, float* uv_host, uint8_t* valid_host) {
  CKARG(ctx && uv_host && valid_host && ctx->img_uv, "no correspondence computed yet"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const size_t L = (size_t)ctx->prm.cell_n * ctx->prm.cell_n;
  CK(hipMemcpyAsync(uv_host, ctx->img_uv, sizeof(float) * 2 * L, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(valid_host, ctx->img_valid, L, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}
int emap_image_fuse(emap_ctx* ctx, int32_t kind, int32_t layer, const float* host_image, int32_t n_planes, int32_t height, int32_t width,
                    double alpha) {
  CKARG(ctx && host_image && kind >= 0 && kind <= 2 && layer >= 0 && layer < ctx->sem_layers, "bad argument"); SF_CHECK();
  CKARG(ctx->img_uv, "emap_image_correspondence must run first");
  CKARG(n_planes >= (kind == 1 ? 3 : 1) && height > 0 && width > 0, "bad image shape");
  CK(hipSetDevice(ctx->device));
  const size_t need = (size_t)n_planes * height * width;
  { const int rc = grow(ctx, &ctx->img_buf, &ctx->img_cap, need); if (rc) return rc; }
  CK(hipMemcpyAsync(ctx->img_buf, host_image, sizeof(float) * need, hipMemcpyHostToDevice, ctx->stream));
  launch_image_fuse(ctx->stream, ctx->kp, kind, ctx->sem + (size_t)layer * ctx->ncells_alloc, ctx->img_buf, ctx->img_uv, ctx->img_valid,
                    (float)height, (float)width, alpha);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));   // host image is only borrowed for the call
  return EMAP_OK;
}

int emap_image_set_tolerance(emap_ctx* ctx, double tolerance_z_collision) {
  CKARG(ctx && tolerance_z_collision == tolerance_z_collision, "bad argument"); SF_CHECK();
  ctx->img_tol = tolerance_z_collision; ctx->img_tol_set = true;
  return EMAP_OK;
}
// the three *_correspondences_to_map kernels on caller arrays (the factories of the compat package): one (cell_n, cell_n) plane in,
// one out; cells without a valid correspondence keep their value (the reference's else branch copies sem_map to new_sem_map)
int emap_image_fuse_arrays(emap_ctx* ctx, int32_t kind, const float* sem_plane, const float* host_image, int32_t n_planes, int32_t height,
                           int32_t width, const float* uv, const uint8_t* valid, double alpha, float* out_plane) {
  CKARG(ctx && sem_plane && host_image && uv && valid && out_plane && kind >= 0 && kind <= 2, "bad argument"); SF_CHECK();
  CKARG(n_planes >= (kind == 1 ? 3 : 1) && height > 0 && width > 0, "bad image shape");
  CK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t L = (size_t)ctx->prm.cell_n * ctx->prm.cell_n;
  DevBuf S, I, U, V;
  CK(S.put(sem_plane, sizeof(float) * L, st, out_plane));
  CK(I.put(host_image, sizeof(float) * (size_t)n_planes * height * width, st, nullptr));
  CK(U.put(uv, sizeof(float) * 2 * L, st, nullptr));
  CK(V.put(valid, L, st, nullptr));
  KP kp = ctx->kp; kp.org_r = kp.org_c = 0;               // caller arrays are logical: no circular origin
  launch_image_fuse(st, kp, kind, (float*)S.d, (const float*)I.d, (const float*)U.d, (const unsigned char*)V.d, (float)height, (float)width, alpha);
  CK(hipGetLastError());
  CK(S.get(st));
  CK(hipStreamSynchronize(st));
  return EMAP_OK;
}

}  // extern "C"
