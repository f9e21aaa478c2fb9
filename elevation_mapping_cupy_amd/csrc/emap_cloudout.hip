// Point-cloud output on the device (gfx950): the valid cells of the published map packed in grid_map's iterator order -- what the node's
// elevation_map_points publisher (elevation_mapping_ros.cpp:501-505, GridMapRosConverter::toPointCloud) and its normal arrows (:751-809)
// walk the whole grid map for on the host.  The index space is that of k_grid_map / k_grid_windows: element (i, j) of what
// get_map_with_name_ref leaves, logical source cell (M - i, M - j), M = C - 2.  GridMapIterator runs lin = j * M + i (j outer, i inner):
// the flat order of the message's column-major planes.  Point k of the output is the k-th cell of that order that passes the predicate;
// no atomic decides a position, so the bytes are unique for a map state.  Three launches:
//
//   k_cloud_count  one workgroup of 256 threads per 32 x 32 tile (tr: 32 rows i, tc: 32 columns j); thread (x, y) = (tid % 32, tid / 32)
//                  holds the cells (32 tr + y + 8 k, 32 tc + x), k = 0 .. 3: lanes run along j (tile_load, emap_publish_tile.h).  Only the
//                  halves and planes the TESTED entries need are loaded.  A wave's ballot holds two rows of 32 column bits; the 32 row
//                  words go through LDS and 32 threads regroup them into one word per column: bit b of masks[j * NT + tr] = cell
//                  (32 tr + b, j) passes.  In memory order (j major, tr minor) the words ARE the iteration order.
//   k_cloud_scan   ONE workgroup of 1024 threads: the exclusive prefix of the popcounts of the W = M * NT words, EM_CLOUD_SCAN_TRIP = 4096
//                  words per trip (a uint4 per thread, wave shuffles, 16 wave totals through LDS), the carry in a register; the total
//                  goes to a device word.  Integer sums: the order of summation is free, the result is not.
//   k_cloud_write  one workgroup per tile.  It reads its 32 mask and offset words first and leaves if no cell of the tile passes.  Then
//                  every half and plane the EMITTED entries need is loaded once, the table is walked (tile_value), each layer goes
//                  through the padded 32 x 33 LDS tile (tile_transpose) so that lanes run along i, and the lane of bit b stores its value at
//                  record rank = offs[j * NT + tr] + popcount(mask & ((1 << b) - 1)), field `field[l]`: the valid cells of a column
//                  segment are consecutive records.  A rank at or beyond `cap` (the records the output buffer holds) is not stored.
//
// A lane outside the map loads nothing, stores nothing and reaches every barrier.  The loads and the walk of the table are those of
// k_grid_map / k_grid_windows over the window (0, 0, M, M): one definition (emap_publish_tile.h) for every door and for both kernels here.
#include "emap_launch.h"

using namespace publish_tile;

namespace {
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
}  // namespace

// A: the TESTED entries.  masks: M * NT words (NT = the row tiles of a column).
__global__ __launch_bounds__(EM_BLOCK) void k_cloud_count(KP P, Cells cells, CloudArgs A, unsigned int* __restrict__ masks) {
  __shared__ unsigned int rowbits[T];
  const int C = P.C, M = C - 2, NT = A.nt;
  const int tc = blockIdx.x / NT, tr = blockIdx.x - tc * NT;   // tiles in mask order: column tile major
  TileCells q;
  tile_load(P, cells, A.tab, 0, 0, M, M, tr, tc, q);
  bool ok[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) ok[k] = q.in[k];
  for (int l = 0; l < A.tab.n; ++l) {
    float v[NK];
    tile_value(A.tab, l, q, C, v);
#pragma unroll
    for (int k = 0; k < NK; ++k) ok[k] = ok[k] && finite_bits(v[k]);
  }
  if (A.call & EM_CLOUD_NORMAL_MIN) {                          // !(sqrt((x x + y y) + z z) < normal_min) in double; the host turned the bound into one on the sum (sum_min)
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const double dx = q.nrm[0][k], dy = q.nrm[1][k], dz = q.nrm[2][k];
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

  TileCells q;
  tile_load(P, cells, A.tab, 0, 0, M, M, tr, tc, q);
  for (int l = 0; l < A.tab.n; ++l) {
    float v[NK];
    tile_value(A.tab, l, q, C, v);
    transpose_put(tile[l & 1], v);
    const int f = A.field[l];
    if (A.cflags[l] & EM_CLOUD_POINT) {                        // x, y, z
      const float px = ii < M ? xs[ii] : 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (live[k]) { float* o = out + rec[k] + f; o[0] = px; o[1] = ys[tc * T + y + (T / NK) * k]; o[2] = transpose_get(tile[l & 1], k); }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NK; ++k) if (live[k]) out[rec[k] + f] = transpose_get(tile[l & 1], k);
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
