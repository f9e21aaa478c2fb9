// C ABI of the MI355X elevation-map fusion core, host side of the submap service on the device (kernel: emap_submap.hip): a batch of
// windows of the published map -- what the node's get_submap service cuts out of its grid map for a planner
// (elevation_mapping_ros.cpp:507-553) -- is answered by one upload of the window and work-item tables, ONE launch over the tiles of all
// windows, ONE device-to-host copy of the packed result and one wait.  The cells outside the windows are not read and nothing of the
// size of the map is written or copied.  The tables and the packed planes live in buffers the context owns.
#include "emap_host.h"
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(sizeof(GridWin) == 32 && sizeof(GridItem) == 16, "carving");
static_assert(EMAP_GRID_MAX_WINDOWS == EM_GRID_MAX_WINDOWS, "window table");

extern "C" {

int emap_publish_grid_windows(emap_ctx* ctx, const emap_grid_layer_ex* layers, int32_t n_layers, int32_t order, float center_z,
                              int32_t use_only_above_for_upper_bound, const emap_grid_window* windows, int32_t n_windows, float* host_out,
                              int64_t host_floats) {
  // everything is refused BEFORE anything is uploaded, launched or copied: host_out and the map stay as they are
  const char* w = "emap_publish_grid_windows: ";
  CKARG(ctx, "null ctx");
  CKARG(layers && windows && host_out, std::string(w) + "null argument");
  CKARG(n_layers >= 1 && n_layers <= EMAP_GRID_MAX_LAYERS, std::string(w) + "n_layers must lie in 1 .. 32");
  CKARG(n_windows >= 1 && n_windows <= EMAP_GRID_MAX_WINDOWS, std::string(w) + "n_windows must lie in 1 .. 64");
  CKARG(order == EMAP_GRID_ROWS || order == EMAP_GRID_MESSAGE, std::string(w) + "order must be 0 (rows) or 1 (message)");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, std::string(w) + "single-strip contexts only");
  for (int k = 0; k < n_layers; ++k) {      // (the slot of an entry is not read: layer k is plane k of every window)
    const emap_grid_layer_ex& g = layers[k];
    CKARG(g.kind >= EMAP_GRID_BUILTIN && g.kind <= EMAP_GRID_PLUGIN, std::string(w) + "kind must be 0 (built-in), 1 (semantic), 2 (normal colour) or 3 (plugin plane)");
    CKARG(g.kind != EMAP_GRID_BUILTIN || (g.index >= 0 && g.index <= 8), std::string(w) + "a built-in index must lie in 0 .. 8");
    CKARG(g.kind != EMAP_GRID_SEMANTIC || (g.index >= 0 && g.index < ctx->sem_layers), std::string(w) + "semantic layer is not configured");
    CKARG(g.kind != EMAP_GRID_PLUGIN || (g.index >= 0 && g.index < ctx->plane_n), std::string(w) + "plugin plane is not reserved (emap_plugin_planes)");
    CKARG(g.kind == EMAP_GRID_PLUGIN ? (g.flags & ~(EMAP_GRID_FILL_NAN | EMAP_GRID_ADD_Z)) == 0 : g.flags == 0, std::string(w) + "flags: FILL_NAN / ADD_Z, on a plugin plane only");
  }
  const int M = ctx->prm.cell_n - 2, T = EM_GRID_TILE;
  int64_t cells_total = 0, n_items = 0;
  for (int v = 0; v < n_windows; ++v) {
    const emap_grid_window& g = windows[v];
    CKARG(g.ni >= 1 && g.nj >= 1, std::string(w) + "a window has at least 1 x 1 cells");
    CKARG(g.i0 >= 0 && g.j0 >= 0 && (int64_t)g.i0 + g.ni <= M && (int64_t)g.j0 + g.nj <= M, std::string(w) + "a window reaches outside the published map (cell_n - 2 cells a side)");
    cells_total += (int64_t)g.ni * g.nj;
    n_items += (int64_t)((g.ni + T - 1) / T) * ((g.nj + T - 1) / T);
  }
  CKARG(host_floats == (int64_t)n_layers * cells_total, std::string(w) + "host_floats must be n_layers times the cells of all windows");
  CKARG(n_items <= 0x7fffffff, std::string(w) + "the batch covers more than 2^31 - 1 tiles of 32 x 32 cells");

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t o_item = sizeof(GridWin) * (size_t)n_windows, up_bytes = o_item + sizeof(GridItem) * (size_t)n_items;
  { const int rc = grow(ctx, &ctx->sub_tab, &ctx->sub_tab_cap, up_bytes); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->sub_pin, &ctx->sub_pin_cap, up_bytes, Grow::pinned); if (rc) return rc; }      // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  { const int rc = grow(ctx, &ctx->sub_out, &ctx->sub_out_cap, (size_t)host_floats); if (rc) return rc; }
  GridWin* wins = reinterpret_cast<GridWin*>(ctx->sub_pin);
  GridItem* items = reinterpret_cast<GridItem*>(ctx->sub_pin + o_item);
  long base = 0;
  for (int v = 0; v < n_windows; ++v) {
    const emap_grid_window& g = windows[v];
    wins[v] = GridWin{g.i0, g.j0, g.ni, g.nj, base, 0};
    base += (long)n_layers * g.ni * g.nj;
    const int ntr = (g.ni + T - 1) / T, ntc = (g.nj + T - 1) / T;
    for (int tr = 0; tr < ntr; ++tr)
      for (int tc = 0; tc < ntc; ++tc) *items++ = GridItem{v, tr, tc, 0};
  }
  CK(hipMemcpyAsync(ctx->sub_tab, ctx->sub_pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  GridArgs A; memset(&A, 0, sizeof A);
  A.n = n_layers; A.order = order; A.only_above = use_only_above_for_upper_bound ? 1 : 0; A.center_z = center_z;
  A.plane = ctx->ncells_alloc; A.sem_plane = ctx->ncells_alloc; A.normal = ctx->normal; A.sem = ctx->sem; A.out = ctx->sub_out; A.plug = ctx->plane_buf;
  bool fill_nan = false;
  for (int k = 0; k < n_layers; ++k) {
    A.kind[k] = (unsigned char)layers[k].kind; A.index[k] = layers[k].kind == EMAP_GRID_NORMAL_COLOR ? 0 : layers[k].index; A.pos[k] = (unsigned char)k;
    A.flags[k] = (unsigned char)layers[k].flags;
    A.need |= grid_need(layers[k].kind, layers[k].index);
    fill_nan = fill_nan || (layers[k].flags & EMAP_GRID_FILL_NAN);
  }
  if (fill_nan && !(A.need & 3)) A.need |= 1;      // FILL_NAN reads is_valid: the hot half, unless the cold half (w mirrors it) is loaded anyway
  launch_grid_windows(ctx->stream, ctx->kp, ctx->cells, A, reinterpret_cast<const GridWin*>(ctx->sub_tab), reinterpret_cast<const GridItem*>(ctx->sub_tab + o_item), (int)n_items);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(host_out, ctx->sub_out, sizeof(float) * (size_t)host_floats, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

}  // extern "C"
