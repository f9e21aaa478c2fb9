// Submap service on the device (gfx950): a batch of windows of the published map -- the patches a foothold planner asks the node's
// get_submap service for (elevation_mapping_ros.cpp:507-553, grid_map_msgs/GetGridMap) -- from ONE launch that reads only the cells of
// the windows and writes every layer of the table packed, window after window.  Element (i, j) of a window is element (i0 + i, j0 + j)
// of what get_map_with_name_ref leaves: logical source cell (M - (i0 + i), M - (j0 + j)), M = C - 2.  It lands at i * nj + j (order 0)
// or at j * ni + i (order 1: the column-major Float32MultiArray of the message) of plane l of its window.
//
// A workgroup owns one work item = a 32 x 32 tile of one window (the host enumerates the tiles of all windows in one table: GridItem).
// The loads, the layer walk and the transpose are grid_tile (emap_publish_tile.h), which k_grid_map runs over the whole map; here the
// window and the float at which its planes begin come from the window table.
#include "emap_launch.h"

template <int ORDER>
__global__ __launch_bounds__(EM_BLOCK) void k_grid_windows(KP P, Cells cells, GridArgs A, const GridWin* __restrict__ wins, const GridItem* __restrict__ items) {
  const GridItem it = items[blockIdx.x];                       // uniform
  const GridWin W = wins[it.win];                              // (the host checked i0 + ni <= M, j0 + nj <= M)
  publish_tile::grid_tile<ORDER>(P, cells, A, W.i0, W.j0, W.ni, W.nj, it.tr, it.tc, W.base);
}

void launch_grid_windows(hipStream_t s, const KP& P, Cells cells, const GridArgs& A, const GridWin* wins, const GridItem* items, int n_items) {
  if (A.order) hipLaunchKernelGGL(k_grid_windows<1>, dim3(n_items), dim3(EM_BLOCK), 0, s, P, cells, A, wins, items);
  else hipLaunchKernelGGL(k_grid_windows<0>, dim3(n_items), dim3(EM_BLOCK), 0, s, P, cells, A, wins, items);
}
