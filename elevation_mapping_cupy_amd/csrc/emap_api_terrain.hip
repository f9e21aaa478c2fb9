// C ABI of the MI355X elevation-map fusion core, host side of the planar terrain on the device (kernels: emap_terrain.hip, and the
// segmentation's, emap_planeseg.hip): what convex_plane_decomposition publishes around its segmentation -- GridMapPreprocessing::preprocess
// (GridMapPreprocessing.cpp:14-39) in front of it, Postprocessing::postprocess (Postprocessing.cpp:14-31) behind it -- as ONE chain of
// launches on the context's stream: [inpaint, median] -> the segmentation's two halves (emap_api_planeseg.hip: its two waits) -> mask,
// inpaint, closing, sloped dilation, box, Gaussian, dilation, lift -> the copies of the planes asked for and a wait.  The small tables
// (element row spans, height offsets, Gaussian taps) are built here and uploaded; every buffer belongs to the context.
#include "emap_host.h"
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(EMAP_TERRAIN_KERNEL_MAX == EM_TERRAIN_KERNEL_MAX && EMAP_TERRAIN_OFFSET_MAX == EM_TERRAIN_OFFSET_MAX && EMAP_TERRAIN_REPEATS_MAX == EM_TERRAIN_REPEATS_MAX, "caps");
static_assert(sizeof(emap_terrain_params) == 64 && sizeof(emap_terrain_planes) == EMAP_TERRAIN_PLANES * sizeof(float*), "layout");
static_assert(2 * EM_TERRAIN_OFFSET_MAX + 1 <= EM_TERRAIN_KERNEL_MAX && sizeof(TerrainTab) % 16 == 0, "tables");

namespace {
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }
bool is_cos(double v) { return v >= -1.0 && v <= 1.0; }

// kernelSizeInPixels (Postprocessing.cpp:75-77): 2 * int(round(size / res)) + 1, round half away from zero; 0 if it cannot be a kernel
int kernel_cells(double size, double res) {
  if (!std::isfinite(size) || size < 0.0) return 0;
  const double r = std::round(size / res);
  return r > (double)EM_TERRAIN_KERNEL_MAX ? 0 : 2 * (int)r + 1;
}
// (ellipse_spans, getStructuringElement(MORPH_ELLIPSE, (k, k)): emap_host.h -- the planar regions erode with the same element)
// getGaussianKernel(k, 0) rounded to float: the fixed tables up to 7, else sigma = 0.3 ((k - 1) / 2 - 1) + 0.8, normalised in double
void gauss_taps(int k, float* t) {
  static const float small[4][7] = {{1.f}, {0.25f, 0.5f, 0.25f}, {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}, {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
  if (k <= 7) { for (int a = 0; a < k; ++a) t[a] = small[k / 2][a]; return; }
  const double sigma = 0.3 * ((double)(k - 1) * 0.5 - 1.0) + 0.8;
  double e[EM_TERRAIN_KERNEL_MAX], sum = 0.0;
  for (int a = 0; a < k; ++a) { const double x = (double)a - (double)(k - 1) * 0.5; e[a] = std::exp(-(x * x) / (2.0 * sigma * sigma)); sum += e[a]; }
  for (int a = 0; a < k; ++a) t[a] = (float)(e[a] / sum);
}

struct TerrainBufs { TerrainTab* tab; float* tmp; float* w; float* wi; float* t1; float* closed; float* dil; float* box; float* smooth; float* lifted; float* elev; float* mask;
                     unsigned char* bit; int* parent; int* root; int* cnt; int* amin; unsigned int* mask1; };

// minValues (inpainting.cpp:25-94) on `in` -> `out` (in == out is allowed); bit_ready: T.bit already holds isnan(in)
void inpaint(hipStream_t s, int M, const TerrainBufs& T, const float* in, float* out, bool bit_ready) {
  const long N = (long)M * M;
  if (!bit_ready) launch_tr_nanbit(s, N, in, T.bit);
  launch_ps_components(s, M, 4, T.bit, T.parent, T.root, T.cnt, T.amin, T.mask1);
  launch_tr_rim(s, M, in, T.bit, T.root, T.amin);
  launch_tr_fill(s, N, in, T.bit, T.root, T.amin, out);
}
}  // namespace

extern "C" {

int emap_planar_terrain(emap_ctx* ctx, const emap_grid_layer_ex* source, const emap_plane_params* params, const emap_terrain_params* terrain,
                        int32_t* host_labels, float* host_normals, emap_plane_record* host_planes, int64_t capacity_planes, int32_t* n_labels,
                        int64_t* n_planes, const emap_terrain_planes* out) {
  // everything is refused BEFORE anything is launched or copied: the outputs and the map stay as they are
  const std::string w = "emap_planar_terrain: ";
  CKARG(ctx, "null ctx");
  CKARG(source && params && terrain && host_labels && host_planes && n_labels && n_planes && out, w + "null argument");
  const emap_plane_params& p = *params;
  const emap_terrain_params& t = *terrain;
  // (the segmentation's own refusals, as emap_plane_segmentation states them)
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
  // the terrain's own
  const int M = ctx->prm.cell_n - 2;
  const int cap = M < EM_TERRAIN_KERNEL_MAX ? M : EM_TERRAIN_KERNEL_MAX;      // every kernel fits the map and the LDS tile
  const int km = t.median_kernel_size < 1 ? 1 : (t.median_kernel_size > 5 ? 5 : t.median_kernel_size);      // (GridMapPreprocessing.cpp:21)
  CKARG(t.preprocess == 0 || t.preprocess == 1, w + "preprocess must be 0 or 1");
  CKARG(!t.preprocess || (km % 2 == 1 && km <= cap), w + "the median's kernelSize must be odd after its clamp to 1 .. 5, and at most the map's side");
  CKARG(!t.preprocess || (t.median_repeats >= 0 && t.median_repeats <= EM_TERRAIN_REPEATS_MAX), w + "numberOfRepeats must lie in 0 .. 8");
  CKARG(t.nonplanar_horizontal_offset >= 0 && t.nonplanar_horizontal_offset <= EM_TERRAIN_OFFSET_MAX && 2 * t.nonplanar_horizontal_offset + 1 <= cap,
        w + "nonplanar_horizontal_offset must lie in 0 .. 15, its kernel within the map's side");
  const int kd = kernel_cells(t.smoothing_dilation_size, p.resolution), kb = kernel_cells(t.smoothing_box_kernel_size, p.resolution),
            kg = kernel_cells(t.smoothing_gauss_kernel_size, p.resolution), kl = 2 * t.nonplanar_horizontal_offset + 1;
  CKARG(kd >= 1 && kd <= cap && kb >= 1 && kb <= cap && kg >= 1 && kg <= cap, w + "a smoothing kernel must be 1 .. 31 cells and at most the map's side");
  CKARG(std::isfinite(t.extracted_planes_height_offset) && std::isfinite(t.nonplanar_height_offset), w + "height offsets must be finite");
  CKARG((t.want & ~EMAP_TERRAIN_ALL) == 0, w + "want: unknown plane");
  for (int k = 0; k < EMAP_TERRAIN_PLANES; ++k) CKARG(!((t.want >> k) & 1) || out->plane[k], w + "a plane of want has no buffer");

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  PlaneArgs A; PlaneBufs B;
  { const int rc = planeseg_source(ctx, *source, p, &A, &B); if (rc) return rc; }
  const size_t N = (size_t)M * M, W = (N + 31) / 32, Wp = (W + EM_CLOUD_SCAN_TRIP - 1) / EM_CLOUD_SCAN_TRIP * EM_CLOUD_SCAN_TRIP, F = up16(4 * N);
  // the device buffer: [tables] [11 float planes] [parent] [root] [cnt] [amin] [mask1] [bit]
  const size_t o_f = up16(sizeof(TerrainTab)), o_par = o_f + 11 * F, o_m1 = o_par + 4 * F, o_bit = o_m1 + 4 * Wp, dev_bytes = o_bit + up16(N);
  { const int rc = grow(ctx, &ctx->terr_buf, &ctx->terr_cap, dev_bytes); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->terr_pin, &ctx->terr_pin_cap, sizeof(TerrainTab), Grow::pinned); if (rc) return rc; }      // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  unsigned char* d = ctx->terr_buf;
  auto fp = [&](int k) { return reinterpret_cast<float*>(d + o_f + (size_t)k * F); };
  auto ip = [&](int k) { return reinterpret_cast<int*>(d + o_par + (size_t)k * F); };
  TerrainBufs T = {reinterpret_cast<TerrainTab*>(d), fp(0), fp(1), fp(2), fp(3), fp(4), fp(5), fp(6), fp(7), fp(8), fp(9), fp(10),
                   d + o_bit, ip(0), ip(1), ip(2), ip(3), reinterpret_cast<unsigned int*>(d + o_m1)};
  TerrainTab* tab = reinterpret_cast<TerrainTab*>(ctx->terr_pin);
  memset(tab, 0, sizeof *tab);
  ellipse_spans(kd, &tab->close); ellipse_spans(kl, &tab->lift); gauss_taps(kg, tab->gauss);
  for (int a = 0; a < kd; ++a)                                   // (Postprocessing.cpp:116-125) slope = float(resolution), the product in double, stored as float
    for (int b = 0; b < kd; ++b) { const int da = a - kd / 2, db = b - kd / 2; tab->off[a * kd + b] = (float)((double)(float)p.resolution * std::sqrt((double)(da * da + db * db))); }
  CK(hipMemcpyAsync(T.tab, tab, sizeof *tab, hipMemcpyHostToDevice, ctx->stream));

  hipStream_t s = ctx->stream;
  if (t.preprocess) {                                           // P1, P2: the segmentation reads what they leave
    float* const first = B.src;
    inpaint(s, M, T, first, first, false);
    if (km > 1)
      for (int r = 0; r < t.median_repeats; ++r) { float* to = B.src == first ? T.tmp : first; launch_tr_median(s, M, km, B.src, to); B.src = to; }      // ping-pong
  }
  const float* e = B.src;
  { const int rc = planeseg_segment(ctx, w, p, A, B, host_labels, host_normals, host_planes, capacity_planes, n_labels, n_planes); if (rc) return rc; }
  if (t.extracted_planes_height_offset != 0.0) for (int64_t k = 0; k < *n_planes; ++k) host_planes[k].support[2] += t.extracted_planes_height_offset;      // (:65-71)

  launch_tr_mask(s, (long)N, e, B.parent, T.w, T.mask, T.bit);                                   // Q1
  inpaint(s, M, T, T.w, T.wi, true);
  launch_tr_morph(s, M, kd, 1, &T.tab->close, T.wi, T.t1);                                       // Q2: dilate, erode
  launch_tr_morph(s, M, kd, 0, &T.tab->close, T.t1, T.closed);
  launch_tr_sloped(s, M, kd, T.tab->off, T.closed, T.dil);                                       // Q3
  launch_tr_blur(s, M, kb, nullptr, 1.0 / (double)(kb * kb), T.dil, T.box);                      // Q4
  launch_tr_blur(s, M, kg, T.tab->gauss, 1.0, T.box, T.smooth);
  const bool lift_on = t.nonplanar_horizontal_offset > 0;
  const double a = t.extracted_planes_height_offset, b = t.nonplanar_height_offset;
  if (lift_on) launch_tr_morph(s, M, kl, 1, &T.tab->lift, e, T.lifted);                          // Q5
  launch_tr_lift(s, (long)N, e, lift_on ? T.lifted : nullptr, T.mask, (a != 0.0 || b != 0.0) ? 1 : 0, (float)(a + b), b != 0.0 ? 1 : 0, (float)b, T.elev);      // Q6
  CK(hipGetLastError());
  const float* planes[EMAP_TERRAIN_PLANES] = {T.elev, T.smooth, T.mask, e, T.w, T.wi, T.closed, T.dil};
  for (int k = 0; k < EMAP_TERRAIN_PLANES; ++k)
    if ((t.want >> k) & 1) CK(hipMemcpyAsync(out->plane[k], planes[k], 4 * N, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return EMAP_OK;
}

}  // extern "C"
