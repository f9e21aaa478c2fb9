// C ABI of the MI355X elevation-map fusion core, host side of the plane segmentation on the device (kernels: emap_planeseg.hip): the
// front of convex_plane_decomposition's SlidingWindowPlaneExtractor::runExtraction (SlidingWindowPlaneExtractor.cpp:49-77) -- window
// planes (:115-144), connected labels (:147-150), one plane per label (:165-220) and the verdict of isGloballyPlanar (:277-300) -- on
// one layer of the published map, which the reference's node downloads as a GridMap for it.  One chain of launches up to the numbering,
// an 8-byte copy of the label and slot counts and a wait; the slot buffer is sized by that count (a checkerboard has M * M / 2 labels
// and no slot); moments, planes and final labels, the copies and a second wait.  Every buffer belongs to the context.  The chain has two
// halves, planeseg_source and planeseg_segment (behind the entry point): emap_planar_terrain segments a preprocessed plane with the second.
#include "emap_host.h"
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(EMAP_PLANE_OPEN_MAX == EM_PLANE_OPEN_MAX, "opening cap");
static_assert(sizeof(emap_plane_params) == 96 && sizeof(emap_plane_record) == 64 && sizeof(PlaneSlot) % 8 == 0, "layout");

namespace {
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }
bool is_cos(double v) { return v >= -1.0 && v <= 1.0; }
// the double behind a monotone key (ps_key, emap_planeseg.hip)
double unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v; memcpy(&v, &b, 8);
  return v;
}
}  // namespace

extern "C" {

int emap_plane_segmentation(emap_ctx* ctx, const emap_grid_layer_ex* source, const emap_plane_params* params, int32_t* host_labels,
                            float* host_normals, emap_plane_record* host_planes, int64_t capacity_planes, int32_t* n_labels,
                            int64_t* n_planes) {
  // everything is refused BEFORE anything is launched or copied: the outputs and the map stay as they are
  const std::string w = "emap_plane_segmentation: ";
  CKARG(ctx, "null ctx");
  CKARG(source && params && host_labels && host_planes && n_labels && n_planes, w + "null argument");
  const emap_plane_params& p = *params;
  CKARG(p.kernel_size == 3 || p.kernel_size == 5 || p.kernel_size == 7, w + "kernel_size must be 3, 5 or 7");
  CKARG(p.connectivity == 4 || p.connectivity == 8, w + "connectivity must be 4 or 8");
  CKARG(p.planarity_opening_filter >= 0 && p.planarity_opening_filter <= EMAP_PLANE_OPEN_MAX, w + "planarity_opening_filter must lie in 0 .. 8");
  CKARG(p.min_number_points_per_label >= 0, w + "min_number_points_per_label is negative");
  CKARG(pos_finite(p.resolution) && pos_finite(p.plane_patch_error_threshold) && pos_finite(p.global_plane_fit_distance_error_threshold),
        w + "resolution and thresholds must be positive and finite");
  CKARG(is_cos(p.cos_local_plane_inclination) && is_cos(p.cos_plane_inclination) && is_cos(p.cos_global_plane_fit_angle), w + "a cosine must lie in [-1, 1]");
  CKARG(std::isfinite(p.origin_x) && std::isfinite(p.origin_y) && std::isfinite(p.center_z), w + "origin and center_z must be finite");
  CKARG(capacity_planes >= 0, w + "capacity_planes is negative");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, w + "single-strip contexts only");
  { const int rc = check_layer_entry(ctx, w, source->kind, source->index, source->flags, true); if (rc) return rc; }

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  PlaneArgs A; PlaneBufs B;
  { const int rc = planeseg_source(ctx, *source, p, &A, &B); if (rc) return rc; }
  return planeseg_segment(ctx, w, p, A, B, host_labels, host_normals, host_planes, capacity_planes, n_labels, n_planes);
}

}  // extern "C"

// ---- the two halves of the chain (also behind emap_planar_terrain, emap_api_terrain.hip, which segments a preprocessed plane) ----------------
namespace emap_host {
// the context's buffers, grown and carved (*B), the call's constants (*A) and the source layer as a dense M x M plane in B->src
int planeseg_source(emap_ctx* ctx, const emap_grid_layer_ex& source, const emap_plane_params& p, PlaneArgs* Aout, PlaneBufs* Bout) {
  const int M = ctx->prm.cell_n - 2;
  const size_t N = (size_t)M * M, W = (N + 31) / 32, Wp = (W + EM_CLOUD_SCAN_TRIP - 1) / EM_CLOUD_SCAN_TRIP * EM_CLOUD_SCAN_TRIP;
  // the device buffer: [head words] [src] [nrm x 3] [parent] [root] [cnt] [amin] [mask1] [offs1] [mask2] [offs2] [bit] [bit2]
  const size_t o_src = 16, o_nrm = o_src + up16(4 * N), o_par = o_nrm + up16(12 * N), o_root = o_par + up16(4 * N), o_cnt = o_root + up16(4 * N),
               o_amin = o_cnt + up16(4 * N), o_m1 = o_amin + up16(4 * N), o_o1 = o_m1 + 4 * Wp, o_m2 = o_o1 + 4 * Wp, o_o2 = o_m2 + 4 * Wp,
               o_bit = o_o2 + 4 * Wp, o_bit2 = o_bit + up16(N), dev_bytes = o_bit2 + up16(N);
  PlaneArgs& A = *Aout; memset(&A, 0, sizeof A);
  A.M = M; A.K = p.kernel_size; A.conn = p.connectivity; A.open_r = p.planarity_opening_filter;
  A.min_points = p.min_number_points_per_label > 3 ? p.min_number_points_per_label : 3;      // (:193)
  A.res = p.resolution; A.thr2 = p.plane_patch_error_threshold * p.plane_patch_error_threshold;      // (:108)
  A.cos_local = p.cos_local_plane_inclination; A.cos_plane = p.cos_plane_inclination; A.ox = p.origin_x; A.oy = p.origin_y;

  ctx->pseg_labels = nullptr;                                  // the buffer is carved again: the labels of the call before are gone (emap_planar_regions)
  { const int rc = grow(ctx, &ctx->pseg_buf, &ctx->pseg_cap, dev_bytes); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->pseg_pin, &ctx->pseg_pin_cap, (size_t)16, Grow::pinned); if (rc) return rc; }      // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  unsigned char* d = ctx->pseg_buf;
  PlaneBufs& B = *Bout;
  B.head = reinterpret_cast<unsigned int*>(d); B.src = reinterpret_cast<float*>(d + o_src); B.nrm = reinterpret_cast<float*>(d + o_nrm);
  B.parent = reinterpret_cast<int*>(d + o_par); B.root = reinterpret_cast<int*>(d + o_root); B.cnt = reinterpret_cast<int*>(d + o_cnt);
  B.amin = reinterpret_cast<int*>(d + o_amin); B.mask1 = reinterpret_cast<unsigned int*>(d + o_m1); B.offs1 = reinterpret_cast<unsigned int*>(d + o_o1);
  B.mask2 = reinterpret_cast<unsigned int*>(d + o_m2); B.offs2 = reinterpret_cast<unsigned int*>(d + o_o2); B.bit = d + o_bit; B.bit2 = d + o_bit2;
  LayerTab tab = tab_init(ctx, p.center_z, p.use_only_above_for_upper_bound);
  tab_put(tab, source.kind, source.index, source.flags);
  tab_finish(tab);
  launch_ps_source(ctx->stream, ctx->kp, ctx->cells, tab, B.src);
  return EMAP_OK;
}

// the planes of B.src (M x M floats on the device, wherever they lie) segmented: window planes, labels, one plane per label; the labels
// stay in B.parent, the normals in B.nrm
int planeseg_segment(emap_ctx* ctx, const std::string& w, const emap_plane_params& p, const PlaneArgs& A, const PlaneBufs& B, int32_t* host_labels, float* host_normals,
                     emap_plane_record* host_planes, int64_t capacity_planes, int32_t* n_labels, int64_t* n_planes) {
  const int M = A.M;
  const size_t N = (size_t)M * M, W = (N + 31) / 32;
  launch_ps_window(ctx->stream, A, B);
  if (A.open_r > 0) {                                           // MORPH_OPEN: erode, then dilate (:137-143)
    launch_ps_morph(ctx->stream, M, A.open_r, 0, B.bit, B.bit2);
    launch_ps_morph(ctx->stream, M, A.open_r, 1, B.bit2, B.bit);
  }
  launch_ps_labels(ctx->stream, A, B, B.bit);
  launch_cloud_scan(ctx->stream, B.mask1, B.offs1, (long)W, B.head);
  launch_cloud_scan(ctx->stream, B.mask2, B.offs2, (long)W, B.head + 1);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->pseg_pin, B.head, 8, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  unsigned int head[2]; memcpy(head, ctx->pseg_pin, 8);
  const size_t n_slots = head[1], slot_bytes = n_slots * sizeof(PlaneSlot);

  { const int rc = grow(ctx, &ctx->pseg_slots, &ctx->pseg_slots_cap, n_slots ? n_slots : 1); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->pseg_pin, &ctx->pseg_pin_cap, 16 + slot_bytes, Grow::pinned); if (rc) return rc; }
  if (n_slots) {
    CK(hipMemsetAsync(ctx->pseg_slots, 0, slot_bytes, ctx->stream));
    launch_ps_moments(ctx->stream, A, B, ctx->pseg_slots);
  }
  launch_ps_planes(ctx->stream, A, B, ctx->pseg_slots, (int)n_slots, B.parent);      // the final labels take the place of the links
  CK(hipGetLastError());
  if (n_slots) CK(hipMemcpyAsync(ctx->pseg_pin + 16, ctx->pseg_slots, slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(host_labels, B.parent, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  if (host_normals) CK(hipMemcpyAsync(host_normals, B.nrm, 12 * N, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  ctx->pseg_labels = B.parent; ctx->pseg_n_labels = (int)head[0];      // the final labels are in place (emap_planar_regions reads them there)

  int64_t accepted = 0;
  for (size_t k = 0; k < n_slots; ++k) { PlaneSlot s; memcpy(&s, ctx->pseg_pin + 16 + k * sizeof(PlaneSlot), sizeof s); accepted += s.accept ? 1 : 0; }
  *n_labels = (int32_t)head[0]; *n_planes = accepted;
  if (accepted > capacity_planes) { ctx->err = w + "more labels have a plane than capacity_planes (*n_planes tells how many)"; return EMAP_ERR_INVALID; }
  int64_t o = 0;
  for (size_t k = 0; k < n_slots; ++k) {                        // slots are in ascending root order: ascending labels
    PlaneSlot s; memcpy(&s, ctx->pseg_pin + 16 + k * sizeof(PlaneSlot), sizeof s);
    if (!s.accept) continue;
    emap_plane_record& r = host_planes[o++];
    r.label = s.label; r.n_points = (int32_t)s.s[0]; r.n_left_out = s.left_out;
    r.needs_refinement = (s.kdist && (unkey(s.kdist) > p.global_plane_fit_distance_error_threshold || -unkey(s.kdot) < p.cos_global_plane_fit_angle)) ? 1 : 0;      // (:294)
    for (int a = 0; a < 3; ++a) { r.support[a] = s.support[a]; r.normal[a] = s.normal[a]; }
  }
  return EMAP_OK;
}
}  // namespace emap_host
