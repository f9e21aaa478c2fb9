// What the histogram pass of the tile-binned scatter (emap_binned.hip) shares with the stencil kernel file (emap_kernels.hip), whose
// k_post_hist runs the histogram of the NEXT frame's cloud beside the stencil tiles of the frame before: the tile geometry, the sort bin
// of a point, the chunk a workgroup takes and the histogram of one chunk.
#pragma once
#include "emap_device.h"

#define BIN_TR 16
#define BIN_TC 64

// (BinGeo, BinRec: emap_device.h; BIN_MAX_T: emap_launch.h)

// sort bin of a point (-1: none) and its cell inside the bin.  Tiles are PHYSICAL: 16 owned rows x 64 columns of memory.
__device__ __forceinline__ int bin_of(const KP& P, const BinGeo& G, const Geo& g, unsigned int& lc) {
  const int lrow = phys_row(P, g.ix) - P.row0, pcol = phys_col(P, g.iy);
  lc = 0u;
  if (!(g.finite && g.valid)) return -1;
  if (g.inside && lrow >= 0 && lrow < P.nrows) {
    const int BR = BIN_TR * G.sub;
    lc = (unsigned int)((lrow % BR) * BIN_TC + (pcol % BIN_TC));
    return (lrow / BR) * G.tiles_x + (pcol / BIN_TC);
  }
  return G.raybin ? G.T : -1;             // ray only (custom_kernels.py:199-258 marches every valid point)
}

// Which chunk of the cloud (= row of the (block, tile) matrix, region of the staging array) workgroup b of the two point passes takes.
// A tile's records are the runs of chunks 0, 1, 2, ... one behind the other, about four records (64 bytes) each at 1 M points; workgroup b
// runs on XCD b % 8 (observed dispatch rule, as in bin_of_block: for speed only), so with chunk = b every 128-byte line of the record
// buffer is put together from pieces that lie dirty in two or three different L2s and each piece goes to memory on its own.  rho sends
// the workgroups of one residue class mod 8 to CONSECUTIVE chunks: neighbouring runs of a tile then meet in one L2.  A bijection on
// [0, B) for every B (B = 8 q + r: class x holds q + (x < r) workgroups and starts at chunk x q + min(x, r); B < 8 is the identity);
// rows stay indexed by chunk, so the scan, the record order and every byte of the sorted records are what they were -- only who
// writes them changes, and nothing depends on the placement for correctness.  The identity order (chunk = b) was the other side of the
// measurement and lost: k_bin_scatter 12.2 -> 11.0 us, 30.0 -> 27.2 MB written at 1 M points.
__device__ __forceinline__ unsigned int bin_chunk_of_block(unsigned int b, unsigned int B) {
  const unsigned int q = B >> 3, r = B & 7u, x = b & 7u, j = b >> 3;
  return x * q + min(x, r) + j;
}
__device__ __forceinline__ unsigned int bin_chunk_of_block() { return bin_chunk_of_block(blockIdx.x, gridDim.x); }

// The histogram of one chunk (k_bin_hist without a strip; the histogram workgroups of k_post_hist): BLK threads zero the LDS row h,
// take the chunk's points U at a time with their loads in flight together, count every point's bin with an LDS atomic and store the
// row as row rho(b, B) of the (block, tile) matrix: workgroup b of the B that share the cloud.
#ifndef HIST_U
#define HIST_U 4
#endif
template <int MODE, int BLK, int U>
__device__ __forceinline__ void bin_hist_chunk(const KP P, const Pose T, const BinGeo G, const float* __restrict__ pts, long n, int stride,
                                               unsigned int* __restrict__ hist, unsigned int* h, unsigned int b, unsigned int B) {
  for (int t = threadIdx.x; t < G.TB; t += BLK) h[t] = 0u;
  const unsigned int blk = bin_chunk_of_block(b, B);         // the chunk this workgroup takes
  const long base = (long)blk * G.chunk;
  __syncthreads();
  for (long k0 = threadIdx.x; k0 < G.chunk; k0 += (long)U * BLK) {      // U loads in flight per thread (as in k_bin_scatter)
    float rx[U], ry[U], rz[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long k = k0 + (long)u * BLK, i = base + k;
      rx[u] = ry[u] = rz[u] = NAN;                           // (a NaN row: no bin)
      if (k < G.chunk && i < n) load_point(pts, i, stride, rx[u], ry[u], rz[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unsigned int lc;
      const int bin = bin_of(P, G, geometry<MODE>(P, T, rx[u], ry[u], rz[u]), lc);
      if (bin >= 0) atomicAdd(&h[bin], 1u);
    }
  }
  __syncthreads();
  unsigned int* row = hist + (long)blk * G.pitch;
  for (int t = threadIdx.x; t < G.pitch; t += BLK) row[t] = t < G.TB ? h[t] : 0u;
}
