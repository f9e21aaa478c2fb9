// GridMap message output (gfx950): every device-resident layer a grid_map_msgs/GridMap publisher asks for, from ONE launch that reads
// each cell once and writes the layers in the message's own layout.  The reference's node makes one get_map_with_name_ref call per
// layer into a row-major matrix, gridMap.add transposes it on the host into grid_map's column-major MatrixXf, addNormalColorLayer loops
// over the cells on the host, and GridMapRosConverter::toMessage copies every layer once more (elevation_mapping_wrapper.cpp:213-252,
// :296-314; elevation_mapping_ros.cpp:269-301).  Here element (i, j) of a layer -- logical source cell (M - i, M - j), M = C - 2 -- lands
// at i * M + j (order 0: what get_map_with_name_ref leaves) or at j * M + i (order 1: the column-major Float32MultiArray of the message).
//
// A workgroup owns one 32 x 32 tile of the whole map, the window (0, 0, M, M) of emap_publish_tile.h: the loads, the layer walk and the
// transpose are grid_tile there.  No window table is read: the tile is the block index and the planes begin at A.out.
#include "emap_launch.h"

template <int ORDER>
__global__ __launch_bounds__(EM_BLOCK) void k_grid_map(KP P, Cells cells, GridArgs A) {
  const int M = P.C - 2;
  publish_tile::grid_tile<ORDER>(P, cells, A, 0, 0, M, M, blockIdx.y, blockIdx.x, 0);
}

void launch_grid_map(hipStream_t s, const KP& P, Cells cells, const GridArgs& A) {
  const int M = P.C - 2, nt = (M + EM_GRID_TILE - 1) / EM_GRID_TILE;
  if (A.order) hipLaunchKernelGGL(k_grid_map<1>, dim3(nt, nt), dim3(EM_BLOCK), 0, s, P, cells, A);
  else hipLaunchKernelGGL(k_grid_map<0>, dim3(nt, nt), dim3(EM_BLOCK), 0, s, P, cells, A);
}
