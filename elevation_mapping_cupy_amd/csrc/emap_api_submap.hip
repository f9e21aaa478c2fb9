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
    { const int rc = check_layer_entry(ctx, w, g.kind, g.index, g.flags, true); if (rc) return rc; }
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
  A.tab = tab_init(ctx, center_z, use_only_above_for_upper_bound); A.order = order; A.out = ctx->sub_out;
  for (int k = 0; k < n_layers; ++k) A.pos[k] = (unsigned char)tab_put(A.tab, layers[k].kind, layers[k].index, layers[k].flags);      // layer k is plane k of every window
  tab_finish(A.tab);
  launch_grid_windows(ctx->stream, ctx->kp, ctx->cells, A, reinterpret_cast<const GridWin*>(ctx->sub_tab), reinterpret_cast<const GridItem*>(ctx->sub_tab + o_item), (int)n_items);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(host_out, ctx->sub_out, sizeof(float) * (size_t)host_floats, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

}  // extern "C"
