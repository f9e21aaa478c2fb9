// Submap service on the device (gfx950): a batch of windows of the published map -- the patches a foothold planner asks the node's
// get_submap service for (elevation_mapping_ros.cpp:507-553, grid_map_msgs/GetGridMap) -- from ONE launch that reads only the cells of
// the windows and writes every layer of the table packed, window after window.  Element (i, j) of a window is element (i0 + i, j0 + j)
// of what get_map_with_name_ref leaves: logical source cell (M - (i0 + i), M - (j0 + j)), M = C - 2.  It lands at i * nj + j (order 0)
// or at j * ni + i (order 1: the column-major Float32MultiArray of the message) of plane l of its window.
//
// A workgroup of 256 threads owns one work item = a 32 x 32 tile of one window (the host enumerates the tiles of all windows in one
// table: GridItem); thread (x, y) = (tid % 32, tid / 32) holds the four cells (ti + y + 8 k, tj + x) of the window.  Everything else is
// k_grid_map (emap_gridmsg.hip): lanes run along j; every half cell and normal plane the table's need mask names is loaded ONCE into
// registers and the table is walked over them; the values are publish_value / normal_color (emap_device.h), the same definition.
// Every lane wraps its own row and column through phys_row / phys_col (normals: their own origin), so a window may straddle the circular
// seam anywhere.  Order 1 goes through the padded 32 x 33 LDS tile, written [x][i] and read [j][x] (x * 33 + i and j * 33 + x are
// conflict free over 32 banks), double buffered with one barrier per layer; the stores then run along i at stride 1 with a row pitch of
// ni, which differs from nj.  A lane outside the window loads nothing and stores nothing, and reaches every barrier: the layer loop is
// uniform.
#include "emap_launch.h"

template <int ORDER>
__global__ __launch_bounds__(EM_BLOCK) void k_grid_windows(KP P, Cells cells, GridArgs A, const GridWin* __restrict__ wins, const GridItem* __restrict__ items) {
  constexpr int T = EM_GRID_TILE, NK = T * T / EM_BLOCK;      // 4 cells per thread
  __shared__ float tile[ORDER ? 2 : 1][ORDER ? T : 1][T + 1];
  const GridItem it = items[blockIdx.x];                       // uniform
  const GridWin W = wins[it.win];
  const int C = P.C, M = C - 2;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  const int ti = it.tr * T, tj = it.tc * T;                    // the tile's first element inside the window
  const int j = tj + x;
  const bool jin = j < W.nj;
  const int c = jin ? M - (W.j0 + j) : 1;                      // logical source column in [1, M] (the host checked j0 + nj <= M)
  const int pcol = phys_col(P, c), ncol = wrap_up(c + P.norg_c, C);

  long ci[NK]; long ni[NK]; bool in[NK]; int rr[NK];
  float4 hot[NK], cold[NK]; float nrm[3][NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = ti + y + (T / NK) * k;
    in[k] = jin && i < W.ni;
    const int r = in[k] ? M - (W.i0 + i) : 1;                  // logical source row in [1, M]
    rr[k] = r;
    ci[k] = (long)(phys_row(P, r) + P.halo) * C + pcol;       // cells and semantic planes: the map's origin
    ni[k] = (long)wrap_up(r + P.norg_r, C) * C + ncol;        // normal planes: the origin they were written with
    hot[k] = make_float4(0.f, 0.f, 0.f, 0.f); cold[k] = hot[k];
    nrm[0][k] = nrm[1][k] = nrm[2][k] = 0.f;
  }
  if (A.need & 1) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) hot[k] = cells.hot[ci[k]];
  }
  if (A.need & 2) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) cold[k] = cells.cold[ci[k]];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (A.need & (4 << a)) {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (in[k]) nrm[a][k] = A.normal[(long)a * A.plane + ni[k]];
    }
  }
  const bool have_hot = A.need & 1;
  const long cells_w = (long)W.ni * W.nj;

  for (int l = 0; l < A.n; ++l) {
    const int kind = A.kind[l], index = A.index[l];            // uniform
    float* __restrict__ out = A.out + W.base + (long)l * cells_w;
    float v[NK];
    if (kind == 1) {
      const float* __restrict__ sp = A.sem + (long)index * A.sem_plane;
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = in[k] ? sp[ci[k]] : 0.f;
    } else if (kind == 2) {
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = normal_color(nrm[0][k], nrm[1][k], nrm[2][k]);
    } else if (kind == 3) {                                    // resident plugin plane, then _publish's order: FILL_NAN, ADD_Z
      const float* __restrict__ pp = A.plug + (long)index * C * C;
      const int fl = A.flags[l];
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = in[k] ? pp[(long)rr[k] * C + c] : 0.f;      // the LOGICAL cell (no circular origin)
      if (fl & EM_GRID_FILL_NAN) {
#pragma unroll
        for (int k = 0; k < NK; ++k) if (!((have_hot ? hot[k].z : cold[k].w) > 0.5f)) v[k] = __uint_as_float(0x7fc00000u);
      }
      if (fl & EM_GRID_ADD_Z) {
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = v[k] + A.center_z;
      }
    } else if (index >= 6) {
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = index == 6 ? nrm[0][k] : (index == 7 ? nrm[1][k] : nrm[2][k]);
    } else {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        Cell m;
        m.h = hot[k].x; m.v = hot[k].y; m.valid = have_hot ? hot[k].z : cold[k].w; m.trav = hot[k].w;      // cold.w mirrors valid
        m.time = cold[k].x; m.upper = cold[k].y; m.is_upper = cold[k].z; m.pad = 0.f;
        v[k] = publish_value(index, m, rr[k], c, C, A.center_z, A.only_above);
      }
    }
    if constexpr (ORDER == 0) {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (in[k]) out[(long)(ti + y + (T / NK) * k) * W.nj + j] = v[k];
    } else {
      float (*tb)[T + 1] = tile[l & 1];
#pragma unroll
      for (int k = 0; k < NK; ++k) tb[x][y + (T / NK) * k] = v[k];
      __syncthreads();       // (two buffers: whoever writes this one again, for layer l + 2, has passed the barrier of layer l + 1, which every reader of layer l reaches after its reads)
      const int ii = ti + x;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int jl = y + (T / NK) * k, jj = tj + jl;
        if (ii < W.ni && jj < W.nj) out[(long)jj * W.ni + ii] = tb[jl][x];
      }
    }
  }
}

void launch_grid_windows(hipStream_t s, const KP& P, Cells cells, const GridArgs& A, const GridWin* wins, const GridItem* items, int n_items) {
  if (A.order) hipLaunchKernelGGL(k_grid_windows<1>, dim3(n_items), dim3(EM_BLOCK), 0, s, P, cells, A, wins, items);
  else hipLaunchKernelGGL(k_grid_windows<0>, dim3(n_items), dim3(EM_BLOCK), 0, s, P, cells, A, wins, items);
}
