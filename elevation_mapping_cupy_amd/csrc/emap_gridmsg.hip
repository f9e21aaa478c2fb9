// GridMap message output (gfx950): every device-resident layer a grid_map_msgs/GridMap publisher asks for, from ONE launch that reads
// each cell once and writes the layers in the message's own layout.  The reference's node makes one get_map_with_name_ref call per
// layer into a row-major matrix, gridMap.add transposes it on the host into grid_map's column-major MatrixXf, addNormalColorLayer loops
// over the cells on the host, and GridMapRosConverter::toMessage copies every layer once more (elevation_mapping_wrapper.cpp:213-252,
// :296-314; elevation_mapping_ros.cpp:269-301).  Here element (i, j) of a layer -- logical source cell (M - i, M - j), M = C - 2: border
// stripped, both axes flipped, as k_publish -- lands at i * M + j (order 0: what get_map_with_name_ref leaves) or at j * M + i (order 1:
// the column-major Float32MultiArray of the message).
//
// A workgroup of 256 threads owns a 32 x 32 tile of (i, j); thread (x, y) = (tid % 32, tid / 32) holds the four cells (i0 + y + 8 k,
// j0 + x).  Lanes run along j, i.e. along the source's columns (descending; the circular origin may cut a row of the tile into two
// runs): every half cell and every normal plane the table needs is loaded ONCE into registers -- a half nobody asked for is not
// loaded -- and the table is then walked over the registers; semantic planes are moved as 32-bit words (colours and class ids are
// bit patterns).  Order 0 stores straight from the registers (lanes along the output's unit stride).  Order 1 goes through a padded
// 32 x 33 LDS tile, written [x][i] and read [j][x], so that the stores run along i in full 128-byte lines; ds_read_b32 / ds_write_b32
// are serviced in groups of 32 lanes over 32 banks: x * 33 + i and j * 33 + x are both conflict free.  The tile is double buffered:
// one barrier per layer.
#include "emap_launch.h"

// (the values: publish_value and normal_color, emap_device.h -- one definition with k_grid_windows, emap_submap.hip)

template <int ORDER>
__global__ __launch_bounds__(EM_BLOCK) void k_grid_map(KP P, Cells cells, GridArgs A) {
  constexpr int T = EM_GRID_TILE, NK = T * T / EM_BLOCK;      // 4 cells per thread
  __shared__ float tile[ORDER ? 2 : 1][ORDER ? T : 1][T + 1];
  const int C = P.C, M = C - 2;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
  const int j = j0 + x;
  const bool jin = j < M;
  const int c = jin ? M - j : 1;                               // logical source column in [1, M] (a lane outside the map reads nothing)
  const int pcol = phys_col(P, c), ncol = wrap_up(c + P.norg_c, C);

  long ci[NK]; long ni[NK]; bool in[NK]; int rr[NK];
  float4 hot[NK], cold[NK]; float nrm[3][NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = i0 + y + (T / NK) * k;
    in[k] = jin && i < M;
    const int r = in[k] ? M - i : 1;
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

  for (int l = 0; l < A.n; ++l) {
    const int kind = A.kind[l], index = A.index[l];            // uniform
    float* __restrict__ out = A.out + (long)A.pos[l] * M * M;
    float v[NK];
    if (kind == 1) {
      const float* __restrict__ sp = A.sem + (long)index * A.sem_plane;
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = in[k] ? sp[ci[k]] : 0.f;
    } else if (kind == 2) {
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = normal_color(nrm[0][k], nrm[1][k], nrm[2][k]);
    } else if (kind == 3) {                                    // resident plugin plane: LOGICAL cell (no circular origin), then _publish's order
      const float* __restrict__ pp = A.plug + (long)index * C * C + (long)rr[0] * C + c;      // (rr[0] = 1 for a thread below the map: the pointer stays inside the plane)
      const int fl = A.flags[l];
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = in[k] ? pp[-(T / NK) * k * C] : 0.f;      // row M - i: (T / NK) k rows above the thread's first (cell_n <= 46340: an int)
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
      for (int k = 0; k < NK; ++k) if (in[k]) out[(long)(i0 + y + (T / NK) * k) * M + j] = v[k];
    } else {
      float (*tb)[T + 1] = tile[l & 1];
#pragma unroll
      for (int k = 0; k < NK; ++k) tb[x][y + (T / NK) * k] = v[k];
      __syncthreads();       // (two buffers: whoever writes this one again, for layer l + 2, has passed the barrier of layer l + 1, which every reader of layer l reaches after its reads)
      const int ii = i0 + x;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int jl = y + (T / NK) * k, jj = j0 + jl;
        if (ii < M && jj < M) out[(long)jj * M + ii] = tb[jl][x];
      }
    }
  }
}

void launch_grid_map(hipStream_t s, const KP& P, Cells cells, const GridArgs& A) {
  const int M = P.C - 2, nt = (M + EM_GRID_TILE - 1) / EM_GRID_TILE;
  if (A.order) hipLaunchKernelGGL(k_grid_map<1>, dim3(nt, nt), dim3(EM_BLOCK), 0, s, P, cells, A);
  else hipLaunchKernelGGL(k_grid_map<0>, dim3(nt, nt), dim3(EM_BLOCK), 0, s, P, cells, A);
}
