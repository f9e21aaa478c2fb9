// C ABI of the MI355X elevation-map fusion core, host side of the GridMap message output (kernel: emap_gridmsg.hip): the layer list of
// a grid_map_msgs/GridMap publisher is answered by ONE launch that reads each cell once and writes every device-resident layer in the
// layout asked for, one device-to-host copy per run of adjacent slots and one wait -- where the reference's node makes one
// get_map_with_name_ref call per layer and copies each layer twice more on the host (elevation_mapping_wrapper.cpp:213-252;
// elevation_mapping_ros.cpp:269-301).  The planes the kernel writes are packed in ascending slot order in a buffer the context owns
// (grid_buf), so that slots adjacent in the caller's buffer are adjacent there too.
#include "emap_host.h"
#include <algorithm>
#include <cstring>

using namespace emap_host;

extern "C" {

int emap_publish_grid_map(emap_ctx* ctx, const emap_grid_layer* layers, int32_t n_layers, int32_t order,
                          float center_z, int32_t use_only_above_for_upper_bound, float* host_out, int64_t host_slots) {
  CKARG(ctx, "null ctx");
  // everything is refused BEFORE anything is launched or copied: host_out and the map stay as they are
  CKARG(layers && host_out, "emap_publish_grid_map: null argument");
  CKARG(n_layers >= 1 && n_layers <= EMAP_GRID_MAX_LAYERS, "emap_publish_grid_map: n_layers must lie in 1 .. 32");
  CKARG(order == EMAP_GRID_ROWS || order == EMAP_GRID_MESSAGE, "emap_publish_grid_map: order must be 0 (rows) or 1 (message)");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_publish_grid_map: single-strip contexts only");
  int by_slot[EMAP_GRID_MAX_LAYERS];
  for (int k = 0; k < n_layers; ++k) {
    const emap_grid_layer& g = layers[k];
    CKARG(g.kind >= EMAP_GRID_BUILTIN && g.kind <= EMAP_GRID_NORMAL_COLOR, "emap_publish_grid_map: kind must be 0 (built-in), 1 (semantic) or 2 (normal colour)");
    CKARG(g.kind != EMAP_GRID_BUILTIN || (g.index >= 0 && g.index <= 8), "emap_publish_grid_map: a built-in index must lie in 0 .. 8");
    CKARG(g.kind != EMAP_GRID_SEMANTIC || (g.index >= 0 && g.index < ctx->sem_layers), "emap_publish_grid_map: semantic layer is not configured");
    CKARG(g.slot >= 0 && (int64_t)g.slot < host_slots, "emap_publish_grid_map: slot outside [0, host_slots)");
    by_slot[k] = k;
  }
  std::sort(by_slot, by_slot + n_layers, [&](int a, int b) { return layers[a].slot < layers[b].slot; });
  for (int p = 1; p < n_layers; ++p) CKARG(layers[by_slot[p]].slot != layers[by_slot[p - 1]].slot, "emap_publish_grid_map: a slot is named twice");
  static_assert(EMAP_GRID_MAX_LAYERS == EM_GRID_MAX_LAYERS, "layer table");

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t MM = (size_t)(ctx->prm.cell_n - 2) * (ctx->prm.cell_n - 2);
  if ((size_t)n_layers * MM > ctx->grid_cap) {
    CK(hipStreamSynchronize(ctx->stream));      // (nothing reads the old buffer any more: every call ends with a wait; kept for safety on a caller's stream)
    if (ctx->grid_buf) CK(hipFree(ctx->grid_buf));
    ctx->grid_buf = nullptr; ctx->grid_cap = 0;
    CK(hipMalloc((void**)&ctx->grid_buf, sizeof(float) * (size_t)n_layers * MM));
    ctx->grid_cap = (size_t)n_layers * MM;
  }
  GridArgs A; memset(&A, 0, sizeof A);
  A.n = n_layers; A.order = order; A.only_above = use_only_above_for_upper_bound ? 1 : 0; A.center_z = center_z;
  A.plane = ctx->ncells_alloc; A.sem_plane = ctx->ncells_alloc; A.normal = ctx->normal; A.sem = ctx->sem; A.out = ctx->grid_buf;
  for (int p = 0; p < n_layers; ++p) {
    const int k = by_slot[p];
    A.kind[k] = (unsigned char)layers[k].kind; A.index[k] = layers[k].kind == EMAP_GRID_NORMAL_COLOR ? 0 : layers[k].index; A.pos[k] = (unsigned char)p;
    A.need |= grid_need(layers[k].kind, layers[k].index);
  }
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

}  // extern "C"
