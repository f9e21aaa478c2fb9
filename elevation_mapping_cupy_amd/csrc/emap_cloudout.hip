// Point-cloud output on the device (gfx950): the valid cells of the published map packed in grid_map's iterator order -- what the node's
// elevation_map_points publisher (elevation_mapping_ros.cpp:501-505, GridMapRosConverter::toPointCloud) and its normal arrows (:751-809)
// walk the whole grid map for on the host.  The index space is that of k_grid_map / k_grid_windows: element (i, j) of what
// get_map_with_name_ref leaves, logical source cell (M - i, M - j), M = C - 2.  GridMapIterator runs lin = j * M + i (j outer, i inner):
// the flat order of the message's column-major planes.  Point k of the output is the k-th cell of that order that passes the predicate;
// no atomic decides a position, so the bytes are unique for a map state.  Three launches:
//
//   k_cloud_count  one workgroup of 256 threads per 32 x 32 tile (tr: 32 rows i, tc: 32 columns j); thread (x, y) = (tid % 32, tid / 32)
//                  holds the cells (32 tr + y + 8 k, 32 tc + x), k = 0 .. 3: lanes run along j, as the loads of k_grid_windows.  Only the
//                  halves and planes the TESTED entries need are loaded.  A wave's ballot holds two rows of 32 column bits; the 32 row
//                  words go through LDS and 32 threads regroup them into one word per column: bit b of masks[j * NT + tr] = cell
//                  (32 tr + b, j) passes.  In memory order (j major, tr minor) the words ARE the iteration order.
//   k_cloud_scan   ONE workgroup of 1024 threads: the exclusive prefix of the popcounts of the W = M * NT words, EM_CLOUD_SCAN_TRIP = 4096
//                  words per trip (a uint4 per thread, wave shuffles, 16 wave totals through LDS), the carry in a register; the total
//                  goes to a device word.  Integer sums: the order of summation is free, the result is not.
//   k_cloud_write  one workgroup per tile.  It reads its 32 mask and offset words first and leaves if no cell of the tile passes.  Then
//                  every half and plane the EMITTED entries need is loaded once, the table is walked as k_grid_windows walks it, each
//                  layer goes through the padded 32 x 33 LDS tile so that lanes run along i, and the lane of bit b stores its value at
//                  record rank = offs[j * NT + tr] + popcount(mask & ((1 << b) - 1)), field `field[l]`: the valid cells of a column
//                  segment are consecutive records.  A rank at or beyond `cap` (the records the output buffer holds) is not stored.
//
// A lane outside the map loads nothing, stores nothing and reaches every barrier.  The values are publish_value / normal_color
// (emap_device.h): the same definitions as k_grid_map, and ONE walk of the table (cloud_value) for the count and the write kernel.
#include "emap_launch.h"

namespace {
constexpr int T = EM_GRID_TILE, NK = T * T / EM_BLOCK;      // 4 cells per thread

// the four cells of a thread, lanes along j: addresses, and every half and plane `need` names (grid_need's bits)
// (separate arrays, not one struct: each stays in registers)
#define CLOUD_CELLS long ci[NK], ni[NK]; bool in[NK]; int rr[NK]; int c; float4 hot[NK], cold[NK]; float nx[NK], ny[NK], nz[NK]
#define CLOUD_CELLS_PARAMS long (&ci)[NK], long (&ni)[NK], bool (&in)[NK], int (&rr)[NK], int& c, float4 (&hot)[NK], float4 (&cold)[NK], float (&nx)[NK], float (&ny)[NK], float (&nz)[NK]
#define CLOUD_CELLS_CONST const long (&ci)[NK], const long (&ni)[NK], const bool (&in)[NK], const int (&rr)[NK], const int& c, const float4 (&hot)[NK], const float4 (&cold)[NK], const float (&nx)[NK], const float (&ny)[NK], const float (&nz)[NK]
#define CLOUD_CELLS_ARGS ci, ni, in, rr, c, hot, cold, nx, ny, nz

__device__ __forceinline__ void cloud_load(const KP& P, const Cells& cells, const CloudArgs& A, int tr, int tc, CLOUD_CELLS_PARAMS) {
  const int C = P.C, M = C - 2;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  const int j = tc * T + x;
  const bool jin = j < M;
  c = jin ? M - j : 1;                                       // logical source column in [1, M]
  const int pcol = phys_col(P, c), ncol = wrap_up(c + P.norg_c, C);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = tr * T + y + (T / NK) * k;
    in[k] = jin && i < M;
    const int r = in[k] ? M - i : 1;                         // logical source row in [1, M]
    rr[k] = r;
    ci[k] = (long)(phys_row(P, r) + P.halo) * C + pcol;     // cells and semantic planes: the map's origin
    ni[k] = (long)wrap_up(r + P.norg_r, C) * C + ncol;      // normal planes: the origin they were written with
    hot[k] = make_float4(0.f, 0.f, 0.f, 0.f); cold[k] = hot[k];
    nx[k] = ny[k] = nz[k] = 0.f;
  }
  if (A.need & 1) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) hot[k] = cells.hot[ci[k]];
  }
  if (A.need & 2) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) cold[k] = cells.cold[ci[k]];
  }
  if (A.need & 4) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) nx[k] = A.normal[ni[k]];
  }
  if (A.need & 8) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) ny[k] = A.normal[A.plane + ni[k]];
  }
  if (A.need & 16) {
#pragma unroll
    for (int k = 0; k < NK; ++k) if (in[k]) nz[k] = A.normal[2 * A.plane + ni[k]];
  }
}

// entry l of the table at the thread's four cells: the layer walk of k_grid_windows
__device__ __forceinline__ void cloud_value(const CloudArgs& A, int l, CLOUD_CELLS_CONST, int C, float (&v)[NK]) {
  const int kind = A.kind[l], index = A.index[l];              // uniform
  const bool have_hot = A.need & 1;
  if (kind == 1) {
    const float* __restrict__ sp = A.sem + (long)index * A.sem_plane;
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = in[k] ? sp[ci[k]] : 0.f;
  } else if (kind == 2) {
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = normal_color(nx[k], ny[k], nz[k]);
  } else if (kind == 3) {                                      // resident plugin plane, then _publish's order: FILL_NAN, ADD_Z
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
    for (int k = 0; k < NK; ++k) v[k] = index == 6 ? nx[k] : (index == 7 ? ny[k] : nz[k]);
  } else {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      Cell m;
      m.h = hot[k].x; m.v = hot[k].y; m.valid = have_hot ? hot[k].z : cold[k].w; m.trav = hot[k].w;      // cold.w mirrors valid
      m.time = cold[k].x; m.upper = cold[k].y; m.is_upper = cold[k].z; m.pad = 0.f;
      v[k] = publish_value(index, m, rr[k], c, C, A.center_z, A.only_above);
    }
  }
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
}  // namespace

// A: the TESTED entries.  masks: M * NT words (NT = the row tiles of a column).
__global__ __launch_bounds__(EM_BLOCK) void k_cloud_count(KP P, Cells cells, CloudArgs A, unsigned int* __restrict__ masks) {
  __shared__ unsigned int rowbits[T];
  const int C = P.C, M = C - 2, NT = A.nt;
  const int tc = blockIdx.x / NT, tr = blockIdx.x - tc * NT;   // tiles in mask order: column tile major
  CLOUD_CELLS;
  cloud_load(P, cells, A, tr, tc, CLOUD_CELLS_ARGS);
  bool ok[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) ok[k] = in[k];
  for (int l = 0; l < A.n; ++l) {
    float v[NK];
    cloud_value(A, l, CLOUD_CELLS_ARGS, C, v);
#pragma unroll
    for (int k = 0; k < NK; ++k) ok[k] = ok[k] && finite_bits(v[k]);
  }
  if (A.call & EM_CLOUD_NORMAL_MIN) {                          // !(sqrt((x x + y y) + z z) < normal_min) in double; the host turned the bound into one on the sum (sum_min)
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const double dx = nx[k], dy = ny[k], dz = nz[k];
      const double s = (dx * dx + dy * dy) + dz * dz;          // squares of floats are exact in double; -ffp-contract=off: no fused step
      ok[k] = ok[k] && !(s < A.sum_min);                       // a NaN normal is not skipped
    }
  }
  const int lane = threadIdx.x & 63, y0 = 2 * (threadIdx.x >> 6);      // a wave holds the rows y0 (lanes 0 .. 31) and y0 + 1 (lanes 32 .. 63)
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const unsigned long long b = __ballot(ok[k]);
    if (lane == 0) { rowbits[y0 + (T / NK) * k] = (unsigned int)b; rowbits[y0 + 1 + (T / NK) * k] = (unsigned int)(b >> 32); }
  }
  __syncthreads();
  if (threadIdx.x < T) {
    const int x = threadIdx.x, j = tc * T + x;
    unsigned int word = 0;
#pragma unroll
    for (int b = 0; b < T; ++b) word |= ((rowbits[b] >> x) & 1u) << b;
    if (j < M) masks[(long)j * NT + tr] = word;
  }
}

// masks / offs: buffers of a multiple of EM_CLOUD_SCAN_TRIP words (the words from W on are not read as counts and their offsets mean nothing)
__global__ __launch_bounds__(EM_CLOUD_SCAN_BLOCK) void k_cloud_scan(const unsigned int* __restrict__ masks, unsigned int* __restrict__ offs, long W, unsigned int* __restrict__ total) {
  constexpr int NW = EM_CLOUD_SCAN_BLOCK / 64;
  __shared__ unsigned int wsum[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned int carry = 0;
  for (long base = 0; base < W; base += EM_CLOUD_SCAN_TRIP) {      // uniform
    const long idx = base + 4L * tid;
    const uint4 m = *reinterpret_cast<const uint4*>(masks + idx);
    const unsigned int c0 = idx < W ? __popc(m.x) : 0u, c1 = idx + 1 < W ? __popc(m.y) : 0u, c2 = idx + 2 < W ? __popc(m.z) : 0u, c3 = idx + 3 < W ? __popc(m.w) : 0u;
    const unsigned int s = (c0 + c1) + (c2 + c3);
    unsigned int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const unsigned int t = wsum[w]; all += t; if (w < wave) before += t; }
    const unsigned int e = carry + before + (incl - s);
    *reinterpret_cast<uint4*>(offs + idx) = make_uint4(e, e + c0, e + c0 + c1, e + c0 + c1 + c2);
    carry += all;
    __syncthreads();                                           // wsum is written again in the next trip
  }
  if (tid == 0) *total = carry;
}

// A: the EMITTED entries.  xs / ys: the positions of row i / column j.  out: records of A.n_fields dwords, `cap` of them.
__global__ __launch_bounds__(EM_BLOCK) void k_cloud_write(KP P, Cells cells, CloudArgs A, const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const unsigned int* __restrict__ masks, const unsigned int* __restrict__ offs, float* __restrict__ out) {
  __shared__ float tile[2][T][T + 1];
  const int C = P.C, M = C - 2, NT = A.nt;
  const int tc = blockIdx.x / NT, tr = blockIdx.x - tc * NT;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
  // after the transpose: thread (x, y) holds the cells (32 tr + x, 32 tc + y + 8 k) -- lanes run along i, bit x of the column's word
  const int ii = tr * T + x;
  bool live[NK]; long rec[NK]; int any = 0;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int jj = tc * T + y + (T / NK) * k;
    unsigned int word = 0, off = 0;
    if (jj < M) { word = masks[(long)jj * NT + tr]; off = offs[(long)jj * NT + tr]; }      // (32 lanes read one word)
    const unsigned int rank = off + __popc(word & ((1u << x) - 1u));
    live[k] = ((word >> x) & 1u) && (long)rank < A.cap;
    rec[k] = (long)rank * A.n_fields;
    any |= live[k];
  }
  if (!__syncthreads_or(any)) return;                           // uniform: no record of this tile is stored, nothing of it is loaded

  CLOUD_CELLS;
  cloud_load(P, cells, A, tr, tc, CLOUD_CELLS_ARGS);
  for (int l = 0; l < A.n; ++l) {
    float v[NK];
    cloud_value(A, l, CLOUD_CELLS_ARGS, C, v);
    float (*tb)[T + 1] = tile[l & 1];
#pragma unroll
    for (int k = 0; k < NK; ++k) tb[x][y + (T / NK) * k] = v[k];
    __syncthreads();       // (two buffers: whoever writes this one again, for entry l + 2, has passed the barrier of entry l + 1, which every reader of entry l reaches after its reads)
    const int f = A.field[l];
    if (A.cflags[l] & EM_CLOUD_POINT) {                        // x, y, z
      const float px = ii < M ? xs[ii] : 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int jl = y + (T / NK) * k;
        if (live[k]) { float* o = out + rec[k] + f; o[0] = px; o[1] = ys[tc * T + jl]; o[2] = tb[jl][x]; }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int jl = y + (T / NK) * k;
        if (live[k]) out[rec[k] + f] = tb[jl][x];
      }
    }
  }
  if (A.call & EM_CLOUD_INDEX) {                               // lin = j * M + i, the iterator's linear index, as a 4-byte integer
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int jj = tc * T + y + (T / NK) * k;
      if (live[k]) out[rec[k] + A.n_fields - 1] = __int_as_float(jj * M + ii);
    }
  }
}

void launch_cloud_count(hipStream_t s, const KP& P, Cells cells, const CloudArgs& A, unsigned int* masks) {
  hipLaunchKernelGGL(k_cloud_count, dim3(A.nt * A.nt), dim3(EM_BLOCK), 0, s, P, cells, A, masks);
}
void launch_cloud_scan(hipStream_t s, const unsigned int* masks, unsigned int* offs, long W, unsigned int* total) {
  hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(EM_CLOUD_SCAN_BLOCK), 0, s, masks, offs, W, total);
}
void launch_cloud_write(hipStream_t s, const KP& P, Cells cells, const CloudArgs& A, const float* xs, const float* ys, const unsigned int* masks,
                        const unsigned int* offs, float* out) {
  hipLaunchKernelGGL(k_cloud_write, dim3(A.nt * A.nt), dim3(EM_BLOCK), 0, s, P, cells, A, xs, ys, masks, offs, out);
}
