// Safety-polygon service on the device (gfx950): the statistics get_polygon_traversability reduces on the host (reference
// EM/elevation_mapping.py:837-889) computed next to the cells, for a BATCH of polygons in two launches.  The host route writes a
// cell_n x cell_n mask, downloads it with the checker layer and is_valid, and reduces the three planes with NumPy; here nothing but
// the verdicts and the per-row extremes of the risky cells -- a few hundred bytes per polygon -- leaves the device.
//
// Pass 1 (k_polysafe_tiles): one workgroup of 256 threads per work item = a 32 x 32 tile of LOGICAL cells of one polygon's bounding
// box, clipped to the interior rows and columns 1 .. C-2 the host slices.  Thread (x, y) = (tid % 32, tid / 32) holds the four cells
// (row0 + y + 8 k, col0 + x): lanes run along the columns, as in k_grid_map, so a row of the tile is one or two runs of adjacent cells
// (the circular origin may cut it).  The polygon's vertex cells are staged once in LDS (every lane reads the same word: a broadcast);
// the inside test is the reference's integer ray-crossing test (emap_polygon.h, shared with k_polygon_mask).  Only a cell inside the
// polygon is read.  Every reduction has a fixed order -- the thread's cells in k order, an xor butterfly over the wave (a + b and
// b + a are the same bits, so every lane ends with the same value), the four waves in index order -- and the workgroup writes ONE part
// record at its work-item index with plain stores: no atomics, no ticket, the same bytes wherever the polygon stands in the batch.
// A row of the tile is held by the 32 lanes of one half wave, which fold its extremes among themselves.
//
// The same launch carries EM_POLY_SWEEP_WG extra workgroups that stride over the whole interior and set ONE flag word (atomic OR of a
// constant: order free) when a KNOWN cell has a risk that is not finite: the host multiplies the risk plane by the mask, so an infinity
// or NaN on a known cell OUTSIDE the polygon becomes inf * 0 = NaN and turns the sum and the maximum into NaN.
//
// Pass 2 (k_polysafe_fold), behind the kernel boundary: one wave per polygon folds the polygon's part records in work-item order into
// the verdict and merges the rows' extremes across the tiles of a tile row.
#include "emap_launch.h"
#include "emap_polygon.h"

// valid and the checker value of the LOGICAL cell (r, c) of a full map
__device__ __forceinline__ void polysafe_read(const KP& P, const Cells& cells, const PolySrc& S, int r, int c, float* valid, float* value) {
  const long ci = (long)(phys_row(P, r) + P.halo) * P.C + phys_col(P, c);
  const float4 h = cells.hot[ci];                     // (h, v, valid, trav): the default checker and is_valid in one 16-byte load
  *valid = h.z;
  if (S.kind == 0) {                                  // uniform
    if (S.index < 4) *value = S.index == 0 ? h.x : (S.index == 1 ? h.y : (S.index == 2 ? h.z : h.w));
    else { const float4 q = cells.cold[ci]; *value = S.index == 4 ? q.x : (S.index == 5 ? q.y : q.z); }
  } else if (S.kind == 1) *value = S.base[(long)S.index * S.plane + ci];        // semantic plane: the map's circular origin
  else *value = S.base[(long)S.index * P.C * P.C + (long)r * P.C + c];          // resident plugin plane: logical order
}

__global__ __launch_bounds__(EM_BLOCK) void k_polysafe_tiles(KP P, Cells cells, PolySrc S, const PolyDesc* __restrict__ polys, const int* __restrict__ verts,
                                                              const PolyItem* __restrict__ items, int n_items, PolyPart* __restrict__ parts,
                                                              unsigned int* __restrict__ flag) {
  constexpr int T = EM_POLY_TILE, NK = T * T / EM_BLOCK;      // 4 cells per thread
  const int C = P.C, M = C - 2, tid = threadIdx.x;
  if ((int)blockIdx.x >= n_items) {                            // poison sweep: a known cell anywhere in the interior whose risk is not finite
    bool bad = false;
    const long MM = (long)M * M;
    for (long i = (long)((int)blockIdx.x - n_items) * EM_BLOCK + tid; i < MM; i += (long)EM_BLOCK * EM_POLY_SWEEP_WG) {
      float valid, value;
      polysafe_read(P, cells, S, 1 + (int)(i / M), 1 + (int)(i % M), &valid, &value);
      if (valid > 0.5f) { const float risk = 1.0f - value; bad = bad || !(fabsf(risk) <= 3.402823466e+38f); }
    }
    if (__syncthreads_or(bad) && tid == 0) atomicOr(flag, 1u);
    return;
  }
  __shared__ int svx[EM_POLY_MAX_VERTS], svy[EM_POLY_MAX_VERTS];
  __shared__ double w_sv[EM_BLOCK / 64], w_sr[EM_BLOCK / 64];
  __shared__ float w_mx[EM_BLOCK / 64];
  __shared__ int w_ni[EM_BLOCK / 64], w_nr[EM_BLOCK / 64], w_nan[EM_BLOCK / 64];
  const PolyItem it = items[blockIdx.x];                       // uniform
  const PolyDesc D = polys[it.poly];
  for (int j = tid; j < D.nv; j += EM_BLOCK) { svx[j] = verts[2 * D.vbeg + j]; svy[j] = verts[2 * D.vbeg + D.nv + j]; }
  __syncthreads();
  const int x = tid & (T - 1), y = tid / T;
  const int c = D.col0 + it.tc * T + x;
  const bool cin = c < D.col0 + D.ncols;
  PolyPart* __restrict__ part = parts + blockIdx.x;

  double sv = 0.0, sr = 0.0; float mx = -INFINITY; int ni = 0, nr = 0, hn = 0;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int w = y + (T / NK) * k, r = D.row0 + it.tr * T + w;
    const PtI p = {r, c};
    const bool inside = cin && r < D.row0 + D.nrows && pm_inside(p, svx, svy, D.nv, D.bminx, D.bminy, D.bmaxx, D.bmaxy);
    bool risky = false;
    if (inside) {
      float valid, value;
      polysafe_read(P, cells, S, r, c, &valid, &value);
      const float risk = valid > 0.5f ? 1.0f - value : 0.0f;      // np.where(known > 0.5, 1.0 - layer, 0.0), float32
      ni += 1; sv += (double)valid; sr += (double)risk;
      risky = risk > S.thr; nr += risky ? 1 : 0;
      mx = fmaxf(mx, risk); hn |= (risk != risk) ? 1 : 0;         // (fmaxf drops a NaN, NumPy's max does not: the flag carries it)
    }
    int lo = risky ? c : EM_POLY_EMPTY_MIN, hi = risky ? c : -1;   // the row's extremes: its 32 lanes are one half of the wave
#pragma unroll
    for (int o = T / 2; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if (x == 0) { part->rmin[w] = lo; part->rmax[w] = hi; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sv += __shfl_xor(sv, o, 64); sr += __shfl_xor(sr, o, 64); mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    ni += __shfl_xor(ni, o, 64); nr += __shfl_xor(nr, o, 64); hn |= __shfl_xor(hn, o, 64);
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { w_sv[wave] = sv; w_sr[wave] = sr; w_mx[wave] = mx; w_ni[wave] = ni; w_nr[wave] = nr; w_nan[wave] = hn; }
  __syncthreads();
  if (tid == 0) {
    sv = w_sv[0]; sr = w_sr[0]; mx = w_mx[0]; ni = w_ni[0]; nr = w_nr[0]; hn = w_nan[0];
    for (int q = 1; q < EM_BLOCK / 64; ++q) { sv += w_sv[q]; sr += w_sr[q]; mx = fmaxf(mx, w_mx[q]); ni += w_ni[q]; nr += w_nr[q]; hn |= w_nan[q]; }
    part->sum_valid = sv; part->sum_risk = sr; part->max_risk = mx; part->n_inside = ni; part->n_risky = nr; part->has_nan = hn;
  }
}

__global__ __launch_bounds__(EM_BLOCK) void k_polysafe_fold(int C, const PolyDesc* __restrict__ polys, int n_polys, const PolyPart* __restrict__ parts,
                                                             const unsigned int* __restrict__ flag, PolyOut* __restrict__ out, int* __restrict__ ext) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * (EM_BLOCK / 64) + (threadIdx.x >> 6);
  if (p >= n_polys) return;                                    // (a whole wave)
  const PolyDesc D = polys[p];
  const int nt = D.ntr * D.ntc;
  const PolyPart* __restrict__ pp = parts + D.item0;
  double sv = 0.0, sr = 0.0; float mx = -INFINITY; int ni = 0, nr = 0, hn = 0;
  for (int base = 0; base < nt; base += 64) {                 // 64 records at a time into the lanes, folded in work-item order
    const int i = base + lane; const bool have = i < nt;
    const double lsv = have ? pp[i].sum_valid : 0.0, lsr = have ? pp[i].sum_risk : 0.0;
    const float lmx = have ? pp[i].max_risk : -INFINITY;
    const int lni = have ? pp[i].n_inside : 0, lnr = have ? pp[i].n_risky : 0, lnan = have ? pp[i].has_nan : 0;
    const int cnt = nt - base < 64 ? nt - base : 64;
    for (int j = 0; j < cnt; ++j) {
      sv += __shfl(lsv, j, 64); sr += __shfl(lsr, j, 64); mx = fmaxf(mx, __shfl(lmx, j, 64));
      ni += __shfl(lni, j, 64); nr += __shfl(lnr, j, 64); hn |= __shfl(lnan, j, 64);
    }
  }
  // the host's maximum runs over the whole interior, where a cell outside the polygon holds risk * 0 = 0; -0.0 never leaves
  const long MM = (long)(C - 2) * (C - 2);
  if ((long)ni < MM) mx = fmaxf(mx, 0.0f);
  mx = mx + 0.0f;
  const int poison = (int)(*flag & 1u);
  if (hn || poison) { sr = __longlong_as_double(0x7ff8000000000000LL); mx = __uint_as_float(0x7fc00000u); }
  if (lane == 0) {
    PolyOut o;
    o.sum_valid = sv; o.sum_risk = sr; o.max_risk = mx; o.n_inside = ni; o.n_risky = nr; o.flags = hn | (poison << 1);
    o.row_begin = D.row0; o.n_rows = D.nrows; o.col_begin = D.col0; o.n_cols = D.ncols;
    out[p] = o;
  }
  for (int q = lane; q < D.nrows; q += 64) {                  // row q of the bbox: tile row q / 32, merged across that row's tiles
    const PolyPart* __restrict__ row = pp + (q / EM_POLY_TILE) * D.ntc;
    const int w = q % EM_POLY_TILE;
    int lo = EM_POLY_EMPTY_MIN, hi = -1;
    for (int tc = 0; tc < D.ntc; ++tc) { lo = min(lo, row[tc].rmin[w]); hi = max(hi, row[tc].rmax[w]); }
    ext[2 * (D.ext0 + q)] = hi < 0 ? -1 : lo;
    ext[2 * (D.ext0 + q) + 1] = hi;
  }
}

void launch_polysafe_tiles(hipStream_t s, const KP& P, Cells cells, const PolySrc& S, const PolyDesc* polys, const int* verts, const PolyItem* items,
                           int n_items, PolyPart* parts, unsigned int* flag) {
  hipLaunchKernelGGL(k_polysafe_tiles, dim3(n_items + EM_POLY_SWEEP_WG), dim3(EM_BLOCK), 0, s, P, cells, S, polys, verts, items, n_items, parts, flag);
}
void launch_polysafe_fold(hipStream_t s, int C, const PolyDesc* polys, int n_polys, const PolyPart* parts, const unsigned int* flag, PolyOut* out, int* ext) {
  hipLaunchKernelGGL(k_polysafe_fold, dim3((n_polys + EM_BLOCK / 64 - 1) / (EM_BLOCK / 64)), dim3(EM_BLOCK), 0, s, C, polys, n_polys, parts, flag, out, ext);
}
