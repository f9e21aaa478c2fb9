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
    if (plugin_ok) CKARG(g.kind >= EMAP_GRID_BUILTIN && g.kind <= EMAP_GRID_PLUGIN, w + "kind must be 0 (built-in), 1 (semantic), 2 (normal colour) or 3 (plugin plane)");
    else CKARG(g.kind >= EMAP_GRID_BUILTIN && g.kind <= EMAP_GRID_NORMAL_COLOR, w + "kind must be 0 (built-in), 1 (semantic) or 2 (normal colour)");
    CKARG(g.kind != EMAP_GRID_BUILTIN || (g.index >= 0 && g.index <= 8), w + "a built-in index must lie in 0 .. 8");
    CKARG(g.kind != EMAP_GRID_SEMANTIC || (g.index >= 0 && g.index < ctx->sem_layers), w + "semantic layer is not configured");
    CKARG(g.kind != EMAP_GRID_PLUGIN || (g.index >= 0 && g.index < ctx->plane_n), w + "plugin plane is not reserved (emap_plugin_planes)");
    CKARG(g.kind == EMAP_GRID_PLUGIN ? (g.flags & ~(EMAP_GRID_FILL_NAN | EMAP_GRID_ADD_Z)) == 0 : g.flags == 0, w + "flags: FILL_NAN / ADD_Z, on a plugin plane only");
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
  A.n = n_layers; A.order = order; A.only_above = use_only_above_for_upper_bound ? 1 : 0; A.center_z = center_z;
  A.plane = ctx->ncells_alloc; A.sem_plane = ctx->ncells_alloc; A.normal = ctx->normal; A.sem = ctx->sem; A.out = ctx->grid_buf; A.plug = ctx->plane_buf;
  bool fill_nan = false;
  for (int p = 0; p < n_layers; ++p) {
    const int k = by_slot[p];
    A.kind[k] = (unsigned char)layers[k].kind; A.index[k] = layers[k].kind == EMAP_GRID_NORMAL_COLOR ? 0 : layers[k].index; A.pos[k] = (unsigned char)p;
    A.flags[k] = (unsigned char)layers[k].flags;
    A.need |= grid_need(layers[k].kind, layers[k].index);
    fill_nan = fill_nan || (layers[k].flags & EMAP_GRID_FILL_NAN);
  }
  if (fill_nan && !(A.need & 3)) A.need |= 1;      // FILL_NAN reads is_valid: the hot half, unless the cold half (w mirrors it) is loaded anyway
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
