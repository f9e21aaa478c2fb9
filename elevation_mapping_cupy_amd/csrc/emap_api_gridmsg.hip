// C ABI of the MI355X elevation-map fusion core, host side of the GridMap message output (kernel: emap_gridmsg.hip): the layer list of
// a grid_map_msgs/GridMap publisher is answered by ONE launch that reads each cell once and writes every device-resident layer in the
// layout asked for, one device-to-host copy per run of adjacent slots and one wait -- where the reference's node makes one
// get_map_with_name_ref call per layer and copies each layer twice more on the host (elevation_mapping_wrapper.cpp:213-252;
// elevation_mapping_ros.cpp:269-301).  The planes the kernel writes are packed in ascending slot order in a buffer the context owns
// (grid_buf), so that slots adjacent in the caller's buffer are adjacent there too.
#include "emap_host.h"
#include <algorithm>
#include <cstring>
#include <string>

using namespace emap_host;

extern "C" {

// Both entry points: `who` names the caller in every refusal, plugin_ok admits EMAP_GRID_PLUGIN (emap_publish_grid_map_ex).
static int grid_publish(emap_ctx* ctx, const emap_grid_layer_ex* layers, int32_t n_layers, int32_t order, float center_z,
                        int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots, const char* who, bool plugin_ok) {
  CKARG(ctx, "null ctx");
  const std::string w = std::string(who) + ": ";
  // everything is refused BEFORE anything is launched or copied: host_out and the map stay as they are
  CKARG(layers && host_out, w + "null argument");
  CKARG(n_layers >= 1 && n_layers <= EMAP_GRID_MAX_LAYERS, w + "n_layers must lie in 1 .. 32");
  CKARG(order == EMAP_GRID_ROWS || order == EMAP_GRID_MESSAGE, w + "order must be 0 (rows) or 1 (message)");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, w + "single-strip contexts only");
  int by_slot[EMAP_GRID_MAX_LAYERS];
  for (int k = 0; k < n_layers; ++k) {
    const emap_grid_layer_ex& g = layers[k];
    { const int rc = check_layer_entry(ctx, w, g.kind, g.index, g.flags, plugin_ok); if (rc) return rc; }
    CKARG(g.slot >= 0 && (int64_t)g.slot < host_slots, w + "slot outside [0, host_slots)");
    by_slot[k] = k;
  }
  std::sort(by_slot, by_slot + n_layers, [&](int a, int b) { return layers[a].slot < layers[b].slot; });
  for (int p = 1; p < n_layers; ++p) CKARG(layers[by_slot[p]].slot != layers[by_slot[p - 1]].slot, w + "a slot is named twice");
  static_assert(EMAP_GRID_MAX_LAYERS == EM_GRID_MAX_LAYERS, "layer table");
  static_assert(EMAP_GRID_FILL_NAN == EM_GRID_FILL_NAN && EMAP_GRID_ADD_Z == EM_GRID_ADD_Z, "layer flags");

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t MM = (size_t)(ctx->prm.cell_n - 2) * (ctx->prm.cell_n - 2);
  { const int rc = grow(ctx, &ctx->grid_buf, &ctx->grid_cap, (size_t)n_layers * MM); if (rc) return rc; }
  GridArgs A; memset(&A, 0, sizeof A);
  A.tab = tab_init(ctx, center_z, use_only_above_for_upper_bound); A.order = order; A.out = ctx->grid_buf;
  for (int k = 0; k < n_layers; ++k) tab_put(A.tab, layers[k].kind, layers[k].index, layers[k].flags);
  tab_finish(A.tab);
  for (int p = 0; p < n_layers; ++p) A.pos[by_slot[p]] = (unsigned char)p;      // the planes packed in ascending slot order
  launch_grid_map(ctx->stream, ctx->kp, ctx->cells, A);
  CK(hipGetLastError());
  for (int p = 0; p < n_layers;) {             // one copy per maximal run of adjacent slots
    int q = p + 1;
    while (q < n_layers && layers[by_slot[q]].slot == layers[by_slot[q - 1]].slot + 1) ++q;
    CK(hipMemcpyAsync(host_out + (size_t)layers[by_slot[p]].slot * MM, ctx->grid_buf + (size_t)p * MM, sizeof(float) * (size_t)(q - p) * MM,
                      hipMemcpyDeviceToHost, ctx->stream));
    p = q;
  }
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

int emap_publish_grid_map_ex(emap_ctx* ctx, const emap_grid_layer_ex* layers, int32_t n_layers, int32_t order,
                             float center_z, int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  return grid_publish(ctx, layers, n_layers, order, center_z, use_only_above_for_upper_bound, host_out, host_slots, "emap_publish_grid_map_ex", true);
}

// the table without flags: built-in, semantic and normal-colour layers only (a plugin plane is refused here as it always was)
int emap_publish_grid_map(emap_ctx* ctx, const emap_grid_layer* layers, int32_t n_layers, int32_t order,
                          float center_z, int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  emap_grid_layer_ex ex[EMAP_GRID_MAX_LAYERS];
  if (layers && n_layers >= 1 && n_layers <= EMAP_GRID_MAX_LAYERS)
    for (int k = 0; k < n_layers; ++k) { ex[k].kind = layers[k].kind; ex[k].index = layers[k].index; ex[k].slot = layers[k].slot; ex[k].flags = 0; }
  return grid_publish(ctx, layers ? ex : nullptr, n_layers, order, center_z, use_only_above_for_upper_bound, host_out, host_slots, "emap_publish_grid_map", false);
}

}  // extern "C"
