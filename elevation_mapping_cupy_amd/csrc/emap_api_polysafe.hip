// C ABI of the MI355X elevation-map fusion core, host side of the safety-polygon service on the device (kernels: emap_polysafe.hip): a
// batch of footprints is answered by one upload of the tables, two launches, one copy back of the verdicts and the rows' extremes and
// one wait -- where get_polygon_traversability (reference EM/elevation_mapping.py:837-889) writes a cell_n x cell_n mask per polygon and
// reduces it with two more whole planes.  The vertex and bounding-box cells are computed here with the reference's own get_idx
// (polygon_cell, emap_api_plugins.hip: float16 quirk included), exactly as emap_polygon_mask computes them.
//
// One device buffer the context owns (poly_buf), carved per call:
//   [ flag word | PolyDesc x n | vertex cells | PolyItem x tiles ]  uploaded from the pinned buffer in ONE copy
//   [ PolyPart x tiles ]                                            written by pass 1, read by pass 2
//   [ PolyOut x n | row extremes ]                                  copied back into the pinned buffer in ONE copy
#include "emap_host.h"
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(sizeof(PolyOut) == sizeof(emap_polygon_verdict) && offsetof(PolyOut, max_risk) == offsetof(emap_polygon_verdict, max_risk) &&
              offsetof(PolyOut, flags) == offsetof(emap_polygon_verdict, flags) && offsetof(PolyOut, n_cols) == offsetof(emap_polygon_verdict, n_cols), "verdict record");
static_assert(EMAP_POLY_MAX_VERTS == EM_POLY_MAX_VERTS, "vertex stage");
static_assert(sizeof(PolyDesc) % 16 == 0 && sizeof(PolyItem) == 16 && sizeof(PolyPart) % 16 == 0 && sizeof(PolyOut) % 16 == 0, "carving");

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" {

int emap_polygon_safety(emap_ctx* ctx, const float* polygons_xy, const int32_t* vertex_begin, int32_t n_polygons, float center_x, float center_y,
                        int32_t layer_kind, int32_t layer_index, float risky_above, emap_polygon_verdict* verdicts, int32_t* row_extremes,
                        const int64_t* row_extremes_begin) {
  // everything is refused BEFORE a device is touched; what needs no context first
  CKARG(ctx && polygons_xy && vertex_begin && verdicts && row_extremes && row_extremes_begin, "emap_polygon_safety: null argument");
  CKARG(n_polygons >= 1 && n_polygons <= EMAP_POLY_MAX_BATCH, "emap_polygon_safety: n_polygons must lie in 1 .. 4096");
  CKARG(vertex_begin[0] == 0, "emap_polygon_safety: vertex_begin[0] must be 0");
  for (int p = 0; p < n_polygons; ++p) {
    const int64_t nv = (int64_t)vertex_begin[p + 1] - vertex_begin[p];
    CKARG(nv >= 1, "emap_polygon_safety: vertex_begin must increase (a polygon has at least 1 vertex)");
    CKARG(nv <= EMAP_POLY_MAX_VERTS, "emap_polygon_safety: a polygon has at most 256 vertices");
    CKARG(row_extremes_begin[p + 1] >= row_extremes_begin[p] && row_extremes_begin[p] >= 0, "emap_polygon_safety: row_extremes_begin must not decrease");
  }
  CKARG(layer_kind == EMAP_POLY_MAP_LAYER || layer_kind == EMAP_POLY_SEMANTIC || layer_kind == EMAP_POLY_PLUGIN,
        "emap_polygon_safety: layer_kind must be 0 (map layer), 1 (semantic) or 3 (plugin plane)");
  CKARG(layer_kind != EMAP_POLY_MAP_LAYER || (layer_index >= 0 && layer_index <= 6), "emap_polygon_safety: a map layer index must lie in 0 .. 6");
  CKARG(layer_kind != EMAP_POLY_SEMANTIC || (layer_index >= 0 && layer_index < ctx->sem_layers), "emap_polygon_safety: semantic layer is not configured");
  CKARG(layer_kind != EMAP_POLY_PLUGIN || (layer_index >= 0 && layer_index < ctx->plane_n), "emap_polygon_safety: plugin plane is not reserved (emap_plugin_planes)");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_polygon_safety: single-strip contexts only");

  // the tables, on the host: vertex cells, bounding boxes and the tiling of each box -- a function of the polygon and the map alone
  const int C = ctx->prm.cell_n, T = EM_POLY_TILE, n = n_polygons;
  const int n_verts = vertex_begin[n];
  std::vector<PolyDesc> desc((size_t)n);
  long n_items = 0, n_rows = 0;
  for (int p = 0; p < n; ++p) {
    PolyDesc& D = desc[p];
    const float* xy = polygons_xy + 2 * (size_t)vertex_begin[p];
    D.vbeg = vertex_begin[p]; D.nv = vertex_begin[p + 1] - vertex_begin[p]; D.pad_ = 0;
    float mn[2] = {xy[0], xy[1]}, mx[2] = {xy[0], xy[1]};
    for (int j = 0; j < D.nv; ++j)
      for (int a = 0; a < 2; ++a) { mn[a] = fminf(mn[a], xy[2 * j + a]); mx[a] = fmaxf(mx[a], xy[2 * j + a]); }
    polygon_cell(ctx->prm, mn[0], mn[1], center_x, center_y, &D.bminx, &D.bminy);
    polygon_cell(ctx->prm, mx[0], mx[1], center_x, center_y, &D.bmaxx, &D.bmaxy);
    const int r0 = D.bminx > 1 ? D.bminx : 1, r1 = D.bmaxx < C - 2 ? D.bmaxx : C - 2;
    const int c0 = D.bminy > 1 ? D.bminy : 1, c1 = D.bmaxy < C - 2 ? D.bmaxy : C - 2;
    D.row0 = r0; D.col0 = c0;
    D.nrows = r1 >= r0 && c1 >= c0 ? r1 - r0 + 1 : 0;
    D.ncols = D.nrows ? c1 - c0 + 1 : 0;
    D.ntr = (D.nrows + T - 1) / T; D.ntc = (D.ncols + T - 1) / T;
    D.item0 = (int)n_items; D.ext0 = n_rows;
    n_items += (long)D.ntr * D.ntc; n_rows += D.nrows;
    CKARG(n_items <= EMAP_POLY_MAX_TILES, "emap_polygon_safety: the batch covers more than 262144 tiles of 32 x 32 cells");
    CKARG(row_extremes_begin[p + 1] - row_extremes_begin[p] >= D.nrows, "emap_polygon_safety: too little room for a polygon's rows (cell_n - 2 always suffice)");
  }

  SF_CHECK();                                  // (traversability may be owed by a pending stencil pass)
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t o_desc = 16, o_vert = o_desc + sizeof(PolyDesc) * n, o_item = up16(o_vert + sizeof(int) * 2 * (size_t)n_verts);
  const size_t up_bytes = o_item + sizeof(PolyItem) * (size_t)n_items;
  const size_t o_part = up_bytes, o_out = o_part + sizeof(PolyPart) * (size_t)n_items, o_ext = o_out + sizeof(PolyOut) * n;
  const size_t down_bytes = sizeof(PolyOut) * n + sizeof(int) * 2 * (size_t)n_rows, total = o_out + down_bytes;
  { int rc = grow(ctx, &ctx->poly_buf, &ctx->poly_cap, total); if (rc) return rc; }
  { int rc = grow(ctx, &ctx->poly_pin, &ctx->poly_pin_cap, up_bytes > down_bytes ? up_bytes : down_bytes, Grow::pinned); if (rc) return rc; }   // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  unsigned char* pin = ctx->poly_pin;
  memset(pin, 0, o_desc);                      // the flag word
  memcpy(pin + o_desc, desc.data(), sizeof(PolyDesc) * n);
  int* verts = reinterpret_cast<int*>(pin + o_vert);
  PolyItem* items = reinterpret_cast<PolyItem*>(pin + o_item);
  for (int p = 0; p < n; ++p) {
    const PolyDesc& D = desc[p];
    const float* xy = polygons_xy + 2 * (size_t)D.vbeg;
    int* vx = verts + 2 * (size_t)D.vbeg; int* vy = vx + D.nv;
    for (int j = 0; j < D.nv; ++j) polygon_cell(ctx->prm, xy[2 * j], xy[2 * j + 1], center_x, center_y, &vx[j], &vy[j]);
    PolyItem* it = items + D.item0;
    for (int tr = 0; tr < D.ntr; ++tr)
      for (int tc = 0; tc < D.ntc; ++tc) *it++ = PolyItem{p, tr, tc, 0};
  }
  unsigned char* dev = ctx->poly_buf;
  CK(hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  PolySrc S; memset(&S, 0, sizeof S);
  S.kind = layer_kind; S.index = layer_index; S.thr = risky_above;
  S.plane = ctx->ncells_alloc; S.base = layer_kind == EMAP_POLY_SEMANTIC ? ctx->sem : (layer_kind == EMAP_POLY_PLUGIN ? ctx->plane_buf : nullptr);
  const PolyDesc* d_desc = reinterpret_cast<const PolyDesc*>(dev + o_desc);
  PolyPart* d_part = reinterpret_cast<PolyPart*>(dev + o_part);
  unsigned int* d_flag = reinterpret_cast<unsigned int*>(dev);
  launch_polysafe_tiles(ctx->stream, ctx->kp, ctx->cells, S, d_desc, reinterpret_cast<const int*>(dev + o_vert), reinterpret_cast<const PolyItem*>(dev + o_item),
                        (int)n_items, d_part, d_flag);
  CK(hipGetLastError());
  launch_polysafe_fold(ctx->stream, C, d_desc, n, d_part, d_flag, reinterpret_cast<PolyOut*>(dev + o_out), reinterpret_cast<int*>(dev + o_ext));
  CK(hipGetLastError());
  CK(hipMemcpyAsync(pin, dev + o_out, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  memcpy(verdicts, pin, sizeof(PolyOut) * n);
  const int* ext = reinterpret_cast<const int*>(pin + sizeof(PolyOut) * n);
  for (int p = 0; p < n; ++p)
    if (desc[p].nrows) memcpy(row_extremes + 2 * row_extremes_begin[p], ext + 2 * desc[p].ext0, sizeof(int) * 2 * (size_t)desc[p].nrows);
  return EMAP_OK;
}

}  // extern "C"
