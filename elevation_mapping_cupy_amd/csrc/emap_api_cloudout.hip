// C ABI of the MI355X elevation-map fusion core, host side of the point-cloud output on the device (kernels: emap_cloudout.hip): the
// valid cells of the published map as the records of a sensor_msgs/PointCloud2 in grid_map's iterator order -- what the node's
// elevation_map_points publisher (elevation_mapping_ros.cpp:501-505) and its normal arrows (:751-809) walk the whole grid map for on
// the host.  One upload of the position tables, three launches (count, scan, write), a 4-byte copy of the count and one wait; then one
// copy of exactly n * point_step bytes and a second wait.  Nothing of the size of the map leaves the device when the map is mostly
// empty.  The tables, the mask and offset words and the records live in buffers the context owns.
#include "emap_host.h"
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(EMAP_CLOUD_POINT == EM_CLOUD_POINT && EMAP_CLOUD_NORMAL_MIN == EM_CLOUD_NORMAL_MIN && EMAP_CLOUD_INDEX == EM_CLOUD_INDEX, "cloud flags");
static_assert(EM_CLOUD_SCAN_TRIP % 4 == 0 && sizeof(emap_cloud_field) == 16, "carving");

namespace {
// the smallest double s with sqrt(s) >= t (sqrt: IEEE, correctly rounded, monotonic), so that for every sum s of squares
// (sqrt(s) < t) == (s < sum_min(t)): the kernel tests the norm without taking a root.  t <= 0: no norm is below it.
double sum_min(double t) {
  if (!(t > 0.0)) return 0.0;
  double s = t * t;
  for (int k = 0; k < 8 && std::sqrt(s) < t; ++k) s = std::nextafter(s, INFINITY);
  for (int k = 0; k < 8 && s > 0.0 && std::sqrt(std::nextafter(s, 0.0)) >= t; ++k) s = std::nextafter(s, 0.0);
  return s;
}
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
}  // namespace

extern "C" {

int emap_publish_point_cloud(emap_ctx* ctx, const emap_cloud_field* fields, int32_t n_fields, float center_z,
                             int32_t use_only_above_for_upper_bound, const float* x_of_i, const float* y_of_j, double normal_min,
                             int32_t call_flags, uint8_t* host_out, int64_t capacity_points, int64_t* n_points, int32_t* point_step) {
  // everything is refused BEFORE anything is uploaded, launched or copied: host_out, *n_points, *point_step and the map stay as they are
  const char* w = "emap_publish_point_cloud: ";
  CKARG(ctx, "null ctx");
  CKARG(fields && x_of_i && y_of_j && host_out && n_points && point_step, std::string(w) + "null argument");
  CKARG(n_fields >= 1 && n_fields <= EMAP_GRID_MAX_LAYERS, std::string(w) + "n_fields must lie in 1 .. 32");
  CKARG(capacity_points >= 0, std::string(w) + "capacity_points is negative");
  CKARG((call_flags & ~(EMAP_CLOUD_NORMAL_MIN | EMAP_CLOUD_INDEX)) == 0, std::string(w) + "call_flags: NORMAL_MIN / INDEX");
  CKARG(!(call_flags & EMAP_CLOUD_NORMAL_MIN) || std::isfinite(normal_min), std::string(w) + "normal_min is not finite");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, std::string(w) + "single-strip contexts only");
  int n_point = 0;
  for (int k = 0; k < n_fields; ++k) {
    const emap_cloud_field& g = fields[k];
    { const int rc = check_layer_entry(ctx, w, g.kind, g.index, g.flags, true); if (rc) return rc; }
    CKARG((g.cloud_flags & ~(EMAP_CLOUD_POINT | EMAP_CLOUD_TEST | EMAP_CLOUD_HIDDEN)) == 0, std::string(w) + "cloud_flags: POINT / TEST / HIDDEN");
    CKARG(!(g.cloud_flags & EMAP_CLOUD_HIDDEN) || (g.cloud_flags & EMAP_CLOUD_TEST), std::string(w) + "a HIDDEN entry must be a TEST entry");
    CKARG(!(g.cloud_flags & EMAP_CLOUD_HIDDEN) || !(g.cloud_flags & EMAP_CLOUD_POINT), std::string(w) + "the POINT entry cannot be HIDDEN");
    n_point += (g.cloud_flags & EMAP_CLOUD_POINT) ? 1 : 0;
  }
  CKARG(n_point == 1, std::string(w) + "exactly one entry carries POINT");

  // the two tables: what the count kernel tests, what the write kernel emits
  const int M = ctx->prm.cell_n - 2, NT = (M + EM_GRID_TILE - 1) / EM_GRID_TILE;
  CloudArgs Tst, Emt; memset(&Tst, 0, sizeof Tst);
  Tst.tab = tab_init(ctx, center_z, use_only_above_for_upper_bound); Tst.call = call_flags; Tst.nt = NT;
  Tst.sum_min = (call_flags & EMAP_CLOUD_NORMAL_MIN) ? sum_min(normal_min) : 0.0;
  Emt = Tst;
  int n_dwords = 0;
  for (int k = 0; k < n_fields; ++k) {
    const emap_cloud_field& g = fields[k];
    auto put = [&](CloudArgs& A) {
      const int l = tab_put(A.tab, g.kind, g.index, g.flags);
      A.cflags[l] = (unsigned char)g.cloud_flags; A.field[l] = (unsigned char)n_dwords;
    };
    if (g.cloud_flags & (EMAP_CLOUD_POINT | EMAP_CLOUD_TEST)) put(Tst);
    if (!(g.cloud_flags & EMAP_CLOUD_HIDDEN)) { put(Emt); n_dwords += (g.cloud_flags & EMAP_CLOUD_POINT) ? 3 : 1; }
  }
  if (call_flags & EMAP_CLOUD_INDEX) n_dwords += 1;
  if (call_flags & EMAP_CLOUD_NORMAL_MIN) Tst.tab.need |= 4 | 8 | 16;
  tab_finish(Tst.tab); tab_finish(Emt.tab);
  const long cells = (long)M * M;
  const long cap = capacity_points < cells ? (long)capacity_points : cells;      // records the device buffer holds: never more than cells pass
  Tst.n_fields = Emt.n_fields = n_dwords; Tst.cap = Emt.cap = cap;

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const long W = (long)M * NT;
  const size_t Wp = (size_t)((W + EM_CLOUD_SCAN_TRIP - 1) / EM_CLOUD_SCAN_TRIP) * EM_CLOUD_SCAN_TRIP;
  const size_t o_xs = 16, o_ys = o_xs + sizeof(float) * (size_t)M, up_bytes = up16(o_ys + sizeof(float) * (size_t)M);      // [count word] [x_of_i] [y_of_j]
  const size_t o_mask = up_bytes, o_offs = o_mask + 4 * Wp, tab_bytes = o_offs + 4 * Wp;
  { const int rc = grow(ctx, &ctx->cloud_tab, &ctx->cloud_tab_cap, tab_bytes); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->cloud_pin, &ctx->cloud_pin_cap, up_bytes, Grow::pinned); if (rc) return rc; }      // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  { const int rc = grow(ctx, &ctx->cloud_out, &ctx->cloud_out_cap, (size_t)(cap > 0 ? cap : 1) * (size_t)n_dwords); if (rc) return rc; }
  memset(ctx->cloud_pin, 0, o_xs);
  memcpy(ctx->cloud_pin + o_xs, x_of_i, sizeof(float) * (size_t)M);
  memcpy(ctx->cloud_pin + o_ys, y_of_j, sizeof(float) * (size_t)M);
  CK(hipMemcpyAsync(ctx->cloud_tab, ctx->cloud_pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  unsigned int* total = reinterpret_cast<unsigned int*>(ctx->cloud_tab);
  unsigned int* masks = reinterpret_cast<unsigned int*>(ctx->cloud_tab + o_mask);
  unsigned int* offs = reinterpret_cast<unsigned int*>(ctx->cloud_tab + o_offs);
  launch_cloud_count(ctx->stream, ctx->kp, ctx->cells, Tst, masks);
  launch_cloud_scan(ctx->stream, masks, offs, W, total);
  launch_cloud_write(ctx->stream, ctx->kp, ctx->cells, Emt, reinterpret_cast<const float*>(ctx->cloud_tab + o_xs), reinterpret_cast<const float*>(ctx->cloud_tab + o_ys),
                     masks, offs, ctx->cloud_out);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->cloud_pin, ctx->cloud_tab, 4, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  unsigned int n = 0; memcpy(&n, ctx->cloud_pin, 4);
  *n_points = (int64_t)n; *point_step = 4 * n_dwords;
  if ((int64_t)n > capacity_points) { ctx->err = std::string(w) + "the cloud holds more points than capacity_points (*n_points tells how many)"; return EMAP_ERR_INVALID; }
  if (n) {
    CK(hipMemcpyAsync(host_out, ctx->cloud_out, (size_t)n * 4 * (size_t)n_dwords, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
  }
  return EMAP_OK;
}

}  // extern "C"
