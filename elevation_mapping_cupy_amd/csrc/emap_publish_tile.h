// The walk over the published map that the GridMap message (emap_gridmsg.hip), the submap service (emap_submap.hip) and the point-cloud
// output (emap_cloudout.hip) share -- written ONCE.  The index space is what get_map_with_name_ref leaves: element (i, j) is logical
// source cell (M - i, M - j), M = C - 2 (border stripped, both axes flipped, as k_publish).  A workgroup of 256 threads owns a 32 x 32
// tile (tr, tc) of a window (i0, j0, ni, nj) of that space -- the whole map is the window (0, 0, M, M) --; thread (x, y) = (tid % 32,
// tid / 32) holds the four elements (32 tr + y + 8 k, 32 tc + x) of the window.  Lanes run along j, i.e. along the source's columns
// (descending); every lane wraps its own row and column through phys_row / phys_col (normals: their own origin), so a window may
// straddle the circular seam anywhere.  Every half cell and every normal plane the table's need mask names is loaded ONCE into registers
// (tile_load) -- a half nobody asked for is not loaded -- and the table is then walked over the registers (tile_value); semantic planes
// are moved as 32-bit words (colours and class ids are bit patterns).  A lane outside the window loads nothing and reaches every barrier.
#pragma once
#include "emap_device.h"

// LayerTab: the layer table every door carries.  kind / index: emap_hip.h (EMAP_GRID_*).  need: what the table reads of a cell -- bit 0
// the hot half, 1 the cold half, 2 .. 4 the normal planes x, y, z (grid_need; a FILL_NAN entry adds a half that carries valid, see
// tab_finish in emap_host.h).  kind 3: resident plugin plane `index` of `plug` (planes of C * C floats in LOGICAL order: no circular
// origin), read at the logical source cell; flags[l] bit 0: NaN where the cell is not valid, bit 1: + center_z (the plugin's fill_nan /
// is_height_layer).  plane / sem_plane: the floats of a normal / semantic plane.
#define EM_GRID_MAX_LAYERS 32
#define EM_GRID_TILE 32
#define EM_GRID_FILL_NAN 1
#define EM_GRID_ADD_Z 2
struct LayerTab { int n, need, only_above; float center_z; long plane, sem_plane; const float* normal; const float* sem; const float* plug;
                  int index[EM_GRID_MAX_LAYERS]; unsigned char kind[EM_GRID_MAX_LAYERS], flags[EM_GRID_MAX_LAYERS]; };
static inline int grid_need(int kind, int index) {
  if (kind == 3) return 0;                                              // plugin plane: its own plane
  if (kind == 1) return 0;                                              // semantic: its own plane
  if (kind == 2) return 4 | 8 | 16;                                     // normal colour
  if (index >= 6) return 4 << (index - 6);                              // normal_x / y / z
  return index == 2 ? 3 : (index <= 1 ? 1 : 2);                         // traversability: both halves; elevation, variance: hot; time, upper_bound, is_upper_bound: cold (w = valid)
}

namespace publish_tile {
constexpr int T = EM_GRID_TILE, NK = T * T / EM_BLOCK;      // 4 cells per thread

// the four cells of a thread: addresses, logical row / column, and every half and plane `need` names
struct TileCells { long ci[NK], ni[NK]; bool in[NK]; int rr[NK], c; float4 hot[NK], cold[NK]; float nrm[3][NK]; };

__device__ __forceinline__ void tile_load(const KP& P, const Cells& cells, const LayerTab& A, int i0, int j0, int ni, int nj, int tr, int tc, TileCells& q) {
  const int C = P.C, M = C - 2;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  const int j = tc * T + x;
  const bool jin = j < nj;
  q.c = jin ? M - (j0 + j) : 1;                               // logical source column in [1, M] (the window lies inside the map; a lane outside it reads nothing)
  const int pcol = phys_col(P, q.c), ncol = wrap_up(q.c + P.norg_c, C);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = tr * T + y + (T / NK) * k;
    q.in[k] = jin && i < ni;
    const int r = q.in[k] ? M - (i0 + i) : 1;                 // logical source row in [1, M]
    q.rr[k] = r;
    q.ci[k] = (long)(phys_row(P, r) + P.halo) * C + pcol;    // cells and semantic planes: the map's origin
    q.ni[k] = (long)wrap_up(r + P.norg_r, C) * C + ncol;     // normal planes: the origin they were written with
    q.hot[k] = make_float4(0.f, 0.f, 0.f, 0.f); q.cold[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    q.nrm[0][k] = q.nrm[1][k] = q.nrm[2][k] = 0.f;
  }
  if (A.need & 1) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (q.in[k]) q.hot[k] = cells.hot[q.ci[k]];
  }
  if (A.need & 2) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (q.in[k]) q.cold[k] = cells.cold[q.ci[k]];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (A.need & (4 << a)) {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (q.in[k]) q.nrm[a][k] = A.normal[(long)a * A.plane + q.ni[k]];
    }
  }
}

// is_valid of cell k from the half that is loaded: cold.w mirrors hot.z (two values, not a choice of address inside q: q stays in registers)
__device__ __forceinline__ float tile_valid(const TileCells& q, int k, bool have_hot) {
  const float hz = q.hot[k].z, cw = q.cold[k].w;
  return have_hot ? hz : cw;
}

// entry l of the table at the thread's four cells (the values themselves: publish_value / normal_color, emap_device.h)
__device__ __forceinline__ void tile_value(const LayerTab& A, int l, const TileCells& q, int C, float (&v)[NK]) {
  const int kind = A.kind[l], index = A.index[l];              // uniform
  const bool have_hot = A.need & 1;
  if (kind == 1) {
    const float* __restrict__ sp = A.sem + (long)index * A.sem_plane;
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = q.in[k] ? sp[q.ci[k]] : 0.f;
  } else if (kind == 2) {
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = normal_color(q.nrm[0][k], q.nrm[1][k], q.nrm[2][k]);
  } else if (kind == 3) {                                      // resident plugin plane, then _publish's order: FILL_NAN, ADD_Z
    const float* __restrict__ pp = A.plug + (long)index * C * C + (long)q.rr[0] * C + q.c;      // the LOGICAL cell (no circular origin); rr[0] = 1 for a thread outside the window: the pointer stays inside the plane
    const int fl = A.flags[l];
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = q.in[k] ? pp[-(T / NK) * k * C] : 0.f;      // in[k] implies in[0]: row rr[k] lies (T / NK) k rows above rr[0] (cell_n <= 46340: an int)
    if (fl & EM_GRID_FILL_NAN) {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (!(tile_valid(q, k, have_hot) > 0.5f)) v[k] = __uint_as_float(0x7fc00000u);
    }
    if (fl & EM_GRID_ADD_Z) {
#pragma unroll
      for (int k = 0; k < NK; ++k) v[k] = v[k] + A.center_z;
    }
  } else if (index >= 6) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const float nx = q.nrm[0][k], ny = q.nrm[1][k], nz = q.nrm[2][k];      // (values, not a choice of address inside q: q stays in registers)
      v[k] = index == 6 ? nx : (index == 7 ? ny : nz);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      Cell m;
      m.h = q.hot[k].x; m.v = q.hot[k].y; m.valid = tile_valid(q, k, have_hot); m.trav = q.hot[k].w;
      m.time = q.cold[k].x; m.upper = q.cold[k].y; m.is_upper = q.cold[k].z; m.pad = 0.f;
      v[k] = publish_value(index, m, q.rr[k], q.c, C, A.center_z, A.only_above);
    }
  }
}

// One step of the transpose through a padded 32 x 33 LDS tile, written [x][i] and read [j][x]: thread (x, y) puts its values of the
// elements (y + 8 k, x) and, behind the barrier, gets those of (x, y + 8 k), so that lanes run along i.  ds_read_b32 / ds_write_b32 are
// serviced in groups of 32 lanes over 32 banks: x * 33 + i and j * 33 + x are both conflict free.  The caller alternates two buffers
// (tile[l & 1]) and that is why ONE barrier per layer suffices: whoever writes this buffer again, for layer l + 2, has passed the barrier
// of layer l + 1, which every reader of layer l reaches after its reads.  A value the caller does not store is not read back.
__device__ __forceinline__ void transpose_put(float (*tb)[T + 1], const float (&v)[NK]) {
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
#pragma unroll
  for (int k = 0; k < NK; ++k) tb[x][y + (T / NK) * k] = v[k];
  __syncthreads();
}
__device__ __forceinline__ float transpose_get(const float (*tb)[T + 1], int k) { return tb[threadIdx.x / T + (T / NK) * k][threadIdx.x & (T - 1)]; }
}  // namespace publish_tile

// GridArgs: the table of k_grid_map / k_grid_windows.  Layer l is written to plane pos[l] of the window's planes in `out` (planes of
// ni * nj floats; the whole-map host code packs the caller's slots in ascending order, the submap host code sets pos[l] = l), element
// (i, j) at i * nj + j (order 0) or j * ni + i (order 1: the message's column-major Float32MultiArray).
struct GridArgs { LayerTab tab; int order, pad_; float* out; unsigned char pos[EM_GRID_MAX_LAYERS]; };

namespace publish_tile {
// Tile (tr, tc) of the window (i0, j0, ni, nj), whose planes begin at float `base` of A.out.  Order 0 stores straight from the registers
// (lanes along the output's unit stride).  Order 1 goes through transpose_put / transpose_get, so that the stores run along i in full 128-byte lines
// with a row pitch of ni.
template <int ORDER>
__device__ __forceinline__ void grid_tile(const KP& P, const Cells& cells, const GridArgs& A, int i0, int j0, int ni, int nj, int tr, int tc, long base) {
  __shared__ float tile[ORDER ? 2 : 1][ORDER ? T : 1][T + 1];
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  const int ti = tr * T, tj = tc * T;                          // the tile's first element inside the window
  TileCells q;
  tile_load(P, cells, A.tab, i0, j0, ni, nj, tr, tc, q);
  for (int l = 0; l < A.tab.n; ++l) {                          // uniform
    float* __restrict__ out = A.out + base + (long)A.pos[l] * ni * nj;
    float v[NK];
    tile_value(A.tab, l, q, P.C, v);
    if constexpr (ORDER == 0) {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (q.in[k]) out[(long)(ti + y + (T / NK) * k) * nj + tj + x] = v[k];
    } else {
      transpose_put(tile[l & 1], v);
      const int ii = ti + x;                                   // now thread (x, y) holds the elements (ti + x, tj + y + 8 k)
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int jj = tj + y + (T / NK) * k;
        if (ii < ni && jj < nj) out[(long)jj * ni + ii] = transpose_get(tile[l & 1], k);
      }
    }
  }
}
}  // namespace publish_tile
