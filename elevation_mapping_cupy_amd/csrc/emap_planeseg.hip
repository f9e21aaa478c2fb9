// Plane segmentation on the device (gfx950): the front of convex_plane_decomposition's SlidingWindowPlaneExtractor::runExtraction
// (SlidingWindowPlaneExtractor.cpp:49-77) on ONE source layer of the published map -- runSlidingWindowDetector (:115-144),
// runSegmentation (:147-150), computePlaneParametersForLabel without RANSAC (:165-220) and the verdict of isGloballyPlanar (:277-300).
// The contract (eigen routine, window points, edge rule, numbering, fixed-point moments) is DESIGN.md section 21; grid_map's
// SlidingWindowIterator and OpenCV's connectedComponents are RESTATED there, neither is pinned by a compiled reference.  Every plane
// is dense M x M in published index space, cell (i, j) at idx = i * M + j.  A chain of launches, nothing waited for in between:
//
//   k_ps_source    the source layer through the shared walk (tile_load / tile_value, emap_publish_tile.h): the values are k_grid_map's;
//                  the circular origin, a pending shift and the plugin flags are handled there and nowhere else.
//   k_ps_window<K> one thread per cell, an 8 x 32 tile plus a halo of K / 2 in LDS (cells outside the map: NaN, i.e. no point).  The
//                  K x K points, their moments, the covariance and its eigenproblem in double registers (ps_plane_normal): the planar
//                  byte and the float normal.
//   k_ps_morph     the opening's erosion / dilation with a cross of radius r, indices clamped at the border (BORDER_REPLICATE).
//   k_ps_local     union-find of a 32 x 32 tile in LDS; parent[] gets GLOBAL indices.
//   k_ps_merge     the links across tile borders: EVERY access to parent[] is an agent-scope atomic.
//   k_ps_flatten   root[] = the root of every cell, a plane of its own, and the bit "is a root" per cell (mask1).
//   k_ps_count     per root the finite members (cnt) and the smallest finite member (amin): integer atomicAdd / atomicMin.
//   k_ps_bits2     the bit "is a root with at least min_points members" (mask2).
//   k_cloud_scan   (emap_cloudout.hip) twice: the order-fixed prefix of both masks.  Label = 1 + rank of the root among the roots in
//                  ascending idx; slot = rank among the roots of mask2.  No atomic decides a number.
//   k_ps_moments   the exact integer moments of every slot's members about its anchor: 64-bit atomicAdd, order-free because exact.
//   k_ps_finalise  one lane per slot: covariance in metres, the same eigen routine, support vector, inclination test.
//   k_ps_fold      per cell the final label (a rejected label: 0; the numbers of the others do not move) and per slot the largest
//                  plane distance and the smallest normal dot product as atomicMax on monotone keys.
//
// Union-find invariant: a link only ever points to a SMALLER idx (parent[x] <= x, and parent[x] only decreases).  So a find walks a
// strictly decreasing chain, and every trip of a union lowers the larger of its two indices: both loops end after at most M * M
// trips whatever the other threads do -- no spin, no grid barrier.  The root of a component is its smallest idx whatever the order
// of the atomics: the result is a function of the map alone.
#include "emap_launch.h"

using namespace publish_tile;

namespace {
constexpr int PS_WT_R = 8, PS_WT_C = 32;                       // k_ps_window's tile: rows x columns, one cell a thread
__device__ __forceinline__ bool ps_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double ps_sel(int i, double a0, double a1, double a2) { return i == 0 ? a0 : (i == 1 ? a1 : a2); }

// One Jacobi rotation of the pair (p, q) of a symmetric 3 x 3 matrix (r: the third index) and of the vectors' columns p, q.
// theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) as emap_pca.hip; a pair with apq == 0 is skipped.
__device__ __forceinline__ void ps_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                          double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq; arp = rp; arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q; v0p = a0; v0q = b0;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q; v1p = a1; v1q = b1;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q; v2p = a2; v2q = b2;
}

// normalAndErrorFromCovariance (:19-41) on cov = sumSquared / n - mean mean^T, the eigenproblem by EM_PLANE_SWEEPS cyclic Jacobi
// sweeps over (0,1), (0,2), (1,2); eigenvalues ascending, ties to the lower index.  q: the upper triangle xx xy xz yy yz zz of the
// sum of squares, s: the sums.  Only + - * / sqrt (-ffp-contract=off: nothing is fused).
__device__ __forceinline__ void ps_plane_normal(double n, const double (&s)[3], const double (&q)[6], double (&nrm)[3], double& err) {
  const double m0 = s[0] / n, m1 = s[1] / n, m2 = s[2] / n;
  double a00 = q[0] / n - m0 * m0, a01 = q[1] / n - m0 * m1, a02 = q[2] / n - m0 * m2;
  double a11 = q[3] / n - m1 * m1, a12 = q[4] / n - m1 * m2, a22 = q[5] / n - m2 * m2;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;      // v[row][column]
#pragma unroll 1
  for (int sweep = 0; sweep < EM_PLANE_SWEEPS; ++sweep) {
    ps_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
    ps_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
    ps_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
  }
  int i0 = 0, i1 = 1, i2 = 2;                                  // a stable sort of three: strict comparisons keep the lower index first
  if (ps_sel(i1, a00, a11, a22) < ps_sel(i0, a00, a11, a22)) { const int t = i0; i0 = i1; i1 = t; }
  if (ps_sel(i2, a00, a11, a22) < ps_sel(i1, a00, a11, a22)) { const int t = i1; i1 = i2; i2 = t; }
  if (ps_sel(i1, a00, a11, a22) < ps_sel(i0, a00, a11, a22)) { const int t = i0; i0 = i1; i1 = t; }
  const double w0 = ps_sel(i0, a00, a11, a22), w1 = ps_sel(i1, a00, a11, a22);
  if (w1 > 1e-8) {
    double x = ps_sel(i0, v00, v01, v02), y = ps_sel(i0, v10, v11, v12), z = ps_sel(i0, v20, v21, v22);
    if (z < 0.0) { x = -x; y = -y; z = -z; }
    nrm[0] = x; nrm[1] = y; nrm[2] = z;
    err = w0 > 0.0 ? w0 : 0.0;
  } else {                                                     // the second eigenvalue is zero: the normal is not defined (:38-40)
    nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; err = 1e30;
  }
}

// ---- union-find: see the invariant in the head of this file --------------------------------------------------------------------------
__device__ __forceinline__ int ps_find_lds(int* lp, int x) {
  for (;;) {                                                   // p < x on every trip but the last: x strictly decreases
    const int p = __hip_atomic_load(&lp[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void ps_union_lds(int* lp, int a, int b) {
  for (;;) {                                                   // max(a, b) strictly decreases from trip to trip
    a = ps_find_lds(lp, a); b = ps_find_lds(lp, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }              // a > b
    const int old = atomicMin(&lp[a], b);
    if (old == a) return;                                      // a was a root: it now hangs below b
    a = old;                                                   // old < a: a had been linked meanwhile; what it pointed to still has to meet b
  }
}
__device__ __forceinline__ int ps_find_agent(int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void ps_union_agent(int* parent, int a, int b) {
  for (;;) {
    a = ps_find_agent(parent, a); b = ps_find_agent(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);                 // (device scope)
    if (old == a) return;
    a = old;
  }
}

// rank of the set bit `x` of a mask / offset pair in k_cloud_scan's layout
__device__ __forceinline__ unsigned int ps_rank(const unsigned int* __restrict__ mask, const unsigned int* __restrict__ offs, int x) {
  return offs[x >> 5] + __popc(mask[x >> 5] & ((1u << (x & 31)) - 1u));
}
__device__ __forceinline__ bool ps_bit(const unsigned int* __restrict__ mask, int x) { return (mask[x >> 5] >> (x & 31)) & 1u; }

// The lanes of a wave that hold a contribution, one label at a time: `todo` starts as the ballot of those lanes; each call picks the
// label of the first lane left (`lead`), marks the lanes that hold the same label (`mine`) and takes them off.  Every lane of the wave
// must call this; the result is uniform.  PS_GROUPS labels of a wave go out as one set of atomics each, lanes left after that on their own.
constexpr int PS_GROUPS = 4;
__device__ __forceinline__ bool ps_next_group(unsigned long long& todo, bool valid, int key, int& lead, bool& mine) {
  if (!todo) return false;
  lead = __ffsll((long long)todo) - 1;
  const int k0 = __shfl(key, lead, 64);
  mine = valid && key == k0;
  todo &= ~__ballot(mine);
  return true;
}
// monotone key of a double: unsigned order = numeric order
__device__ __forceinline__ unsigned long long ps_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ long long ps_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long ps_wave_max_ll(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long ps_wave_max(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64); v = o > v ? o : v; }
  return v;
}
}  // namespace

// ---- a. the source plane -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_ps_source(KP P, Cells cells, LayerTab tab, int nt, float* __restrict__ src) {
  const int C = P.C, M = C - 2;
  const int tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt;
  TileCells q;
  tile_load(P, cells, tab, 0, 0, M, M, tr, tc, q);
  float v[NK];
  tile_value(tab, 0, q, C, v);
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T;
#pragma unroll
  for (int k = 0; k < NK; ++k) if (q.in[k]) src[(long)(tr * T + y + (T / NK) * k) * M + tc * T + x] = v[k];
}

// ---- b. the window pass ------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(PS_WT_R* PS_WT_C) void k_ps_window(PlaneArgs A, const float* __restrict__ src, float* __restrict__ nrm, unsigned char* __restrict__ bit) {
  constexpr int H = K / 2, LR = PS_WT_R + 2 * H, LC = PS_WT_C + 2 * H;
  __shared__ float tile[LR][LC + 1];
  const int M = A.M;
  const int i0 = blockIdx.y * PS_WT_R, j0 = blockIdx.x * PS_WT_C;
  for (int e = threadIdx.x; e < LR * LC; e += PS_WT_R * PS_WT_C) {
    const int lr = e / LC, lc = e - lr * LC, i = i0 + lr - H, j = j0 + lc - H;
    tile[lr][lc] = (i >= 0 && i < M && j >= 0 && j < M) ? src[(long)i * M + j] : __uint_as_float(0x7fc00000u);      // outside the map: no point
  }
  __syncthreads();
  const int lx = threadIdx.x & (PS_WT_C - 1), ly = threadIdx.x / PS_WT_C, i = i0 + ly, j = j0 + lx;
  if (i >= M || j >= M) return;                                // (behind the only barrier)
  const long idx = (long)i * M + j, N = (long)M * M;
  float nx = 0.f, ny = 0.f, nz = 0.f; unsigned char planar = 0;
  if (ps_finite(tile[ly + H][lx + H])) {
    double n = 0.0, s[3] = {0.0, 0.0, 0.0}, q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kc = 0; kc < K; ++kc) {                           // column outer, row inner (:84-85); kr, kc count from the UNCLIPPED window's corner
      const double py = (double)(-kc) * A.res;
#pragma unroll
      for (int kr = 0; kr < K; ++kr) {
        const float h = tile[ly + kr][lx + kc];
        if (ps_finite(h)) {
          const double px = (double)(-kr) * A.res, pz = (double)h;
          n += 1.0; s[0] += px; s[1] += py; s[2] += pz;
          q[0] += px * px; q[1] += px * py; q[2] += px * pz; q[3] += py * py; q[4] += py * pz; q[5] += pz * pz;
        }
      }
    }
    double nv[3] = {0.0, 0.0, 1.0}, err = 1e30;               // fewer than 3 points: no normal direction (:98-100)
    if (n >= 3.0) ps_plane_normal(n, s, q, nv, err);
    nx = (float)nv[0]; ny = (float)nv[1]; nz = (float)nv[2];
    planar = (err < A.thr2 && nv[2] > A.cos_local) ? 1 : 0;    // isLocallyPlanar (:107-113)
  }
  nrm[idx] = nx; nrm[N + idx] = ny; nrm[2 * N + idx] = nz;
  bit[idx] = planar;
}

// ---- c. the opening's two halves ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_ps_morph(int M, int radius, int dilate, const unsigned char* __restrict__ in, unsigned char* __restrict__ out) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= (long)M * M) return;
  const int i = (int)(idx / M), j = (int)(idx - (long)i * M);
  int v = in[idx];
  for (int d = 1; d <= radius; ++d) {                          // a cross: the centre row and the centre column; indices clamped
    const int iu = i - d < 0 ? 0 : i - d, id = i + d > M - 1 ? M - 1 : i + d, jl = j - d < 0 ? 0 : j - d, jr = j + d > M - 1 ? M - 1 : j + d;
    const int a = in[(long)iu * M + j], b = in[(long)id * M + j], c = in[(long)i * M + jl], e = in[(long)i * M + jr];
    v = dilate ? (v | a | b | c | e) : (v & a & b & c & e);
  }
  out[idx] = (unsigned char)v;
}

// ---- d. labels ---------------------------------------------------------------------------------------------------------------------------
// one workgroup per 32 x 32 tile, thread (x, y) holds the cells (32 tr + y + 8 k, 32 tc + x); lp: links inside the tile, local index
// l = 32 * row + column -- monotone in idx among the cells of a tile, so the local root is the tile's smallest idx of the component
__global__ __launch_bounds__(EM_BLOCK) void k_ps_local(int M, int conn, const unsigned char* __restrict__ bit, int* __restrict__ parent, int* __restrict__ cnt, int* __restrict__ amin) {
  __shared__ int lp[T * T];
  const int nt = (M + T - 1) / T, tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt;
  const int x = threadIdx.x & (T - 1), y = threadIdx.x / T, j = tc * T + x;
  bool on[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int ly = y + (T / NK) * k, i = tr * T + ly;
    const bool in = i < M && j < M;
    on[k] = in && bit[(long)i * M + j];
    lp[ly * T + x] = on[k] ? ly * T + x : -1;
    if (in) { cnt[(long)i * M + j] = 0; amin[(long)i * M + j] = 0x7fffffff; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int ly = y + (T / NK) * k, l = ly * T + x;
    if (!on[k]) continue;
    if (x > 0 && lp[l - 1] >= 0) ps_union_lds(lp, l, l - 1);
    if (ly > 0 && lp[l - T] >= 0) ps_union_lds(lp, l, l - T);
    if (conn == 8 && ly > 0) {
      if (x > 0 && lp[l - T - 1] >= 0) ps_union_lds(lp, l, l - T - 1);
      if (x < T - 1 && lp[l - T + 1] >= 0) ps_union_lds(lp, l, l - T + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int ly = y + (T / NK) * k, i = tr * T + ly;
    if (i < M && j < M) {
      int g = -1;
      if (on[k]) { const int r = ps_find_lds(lp, ly * T + x); g = (tr * T + (r >> 5)) * M + tc * T + (r & (T - 1)); }
      parent[(long)i * M + j] = g;
    }
  }
}

// the neighbours of a cell that lie in ANOTHER tile (left, up, and with connectivity 8 the two upper diagonals)
__global__ __launch_bounds__(EM_BLOCK) void k_ps_merge(int M, int conn, const unsigned char* __restrict__ bit, int* parent) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= (long)M * M) return;
  const int i = (int)(idx / M), j = (int)(idx - (long)i * M), lx = j & (T - 1), ly = i & (T - 1);
  if ((lx != 0 && ly != 0 && lx != T - 1) || !bit[idx]) return;
  const int g = (int)idx;
  if (lx == 0 && j > 0 && bit[idx - 1]) ps_union_agent(parent, g, g - 1);
  if (ly == 0 && i > 0 && bit[idx - M]) ps_union_agent(parent, g, g - M);
  if (conn == 8 && i > 0) {
    if ((lx == 0 || ly == 0) && j > 0 && bit[idx - M - 1]) ps_union_agent(parent, g, g - M - 1);
    if ((lx == T - 1 || ly == 0) && j < M - 1 && bit[idx - M + 1]) ps_union_agent(parent, g, g - M + 1);
  }
}

// a launch of its own: parent[] is final and read plainly; the roots go to a SEPARATE plane.  mask1: words of 32 consecutive idx.
__global__ __launch_bounds__(EM_BLOCK) void k_ps_flatten(long N, const int* __restrict__ parent, int* __restrict__ root, unsigned int* __restrict__ mask1) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  int r = -1;
  if (idx < N) {
    int x = parent[idx];
    if (x >= 0) { for (;;) { const int p = parent[x]; if (p == x) break; x = p; } r = x; }      // strictly decreasing
    root[idx] = r;
  }
  const unsigned long long b = __ballot(idx < N && r == (int)idx);
  if ((threadIdx.x & 63) == 0) { const long w = (idx >> 5); mask1[w] = (unsigned int)b; mask1[w + 1] = (unsigned int)(b >> 32); }
}

// ---- f. per root: finite members, the first of them --------------------------------------------------------------------------------------
// The three per-cell kernels that fold into per-label words (k_ps_count, k_ps_moments, k_ps_fold) give a thread PS_CPT CONSECUTIVE cells
// (a wave: 1024 consecutive cells, about a row of a 1024^2 map) and keep the contributions of its current label in registers: they go
// out when the label changes inside the thread's run and at the end, there as ONE set of atomics per wave and label (ps_next_group).  Atomic instructions on one cache line are served one after the other (measured: about 37 ns each from 256 CUs), and a
// large label would otherwise send one set per cell or per wave of 64 cells to the same line.  Integer sums, minima and maxima: any
// grouping gives the same words.
constexpr int PS_CPT = 16;

__global__ __launch_bounds__(EM_BLOCK) void k_ps_count(long N, const float* __restrict__ src, const int* __restrict__ root, int* cnt, int* amin) {
  const long base = ((long)blockIdx.x * EM_BLOCK + threadIdx.x) * PS_CPT;
  int cur = -1, n = 0, first = 0x7fffffff;
  for (int k = 0; k < PS_CPT; ++k) {
    const long idx = base + k;
    const int r = idx < N ? root[idx] : -1;
    if (r < 0 || !ps_finite(src[idx])) continue;
    if (r != cur) {
      if (cur >= 0) { atomicAdd(&cnt[cur], n); atomicMin(&amin[cur], first); }
      cur = r; n = 0; first = (int)idx;                        // idx ascends with k: the first cell seen is the run's smallest
    }
    ++n;
  }
  const bool valid = cur >= 0;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  int lead; bool mine;
  for (int g = 0; g < PS_GROUPS && ps_next_group(todo, valid, cur, lead, mine); ++g) {
    const int tot = (int)ps_wave_sum(mine ? n : 0), mn = -(int)ps_wave_max_ll(mine ? -(long long)first : -(long long)0x7fffffff);
    if (lane == lead) { atomicAdd(&cnt[cur], tot); atomicMin(&amin[cur], mn); }
  }
  if (valid && ((todo >> lane) & 1)) { atomicAdd(&cnt[cur], n); atomicMin(&amin[cur], first); }
}

__global__ __launch_bounds__(EM_BLOCK) void k_ps_bits2(long N, int min_points, const int* __restrict__ root, const int* __restrict__ cnt, unsigned int* __restrict__ mask2) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const bool own = idx < N && root[idx] == (int)idx && cnt[idx] >= min_points;
  const unsigned long long b = __ballot(own);
  if ((threadIdx.x & 63) == 0) { const long w = (idx >> 5); mask2[w] = (unsigned int)b; mask2[w + 1] = (unsigned int)(b >> 32); }
}

// ---- f. the moments of every slot --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ps_flush_moments(PlaneSlot* slots, int slot, const long long (&c)[10]) {
#pragma unroll
  for (int k = 0; k < 10; ++k) if (c[k] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&slots[slot].s[k]), (unsigned long long)c[k]);
}

__global__ __launch_bounds__(EM_BLOCK) void k_ps_moments(PlaneArgs A, PlaneBufs B, PlaneSlot* slots) {
  const int M = A.M;
  const long N = (long)M * M, base = ((long)blockIdx.x * EM_BLOCK + threadIdx.x) * PS_CPT;
  int cur = -1; long long c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < PS_CPT; ++k) {
    const long idx = base + k;
    const int r = idx < N ? B.root[idx] : -1;
    if (r < 0 || !ps_bit(B.mask2, r)) continue;
    const int slot = (int)ps_rank(B.mask2, B.offs2, r);
    if (idx == r) { slots[slot].root = r; slots[slot].label = 1 + (int)ps_rank(B.mask1, B.offs1, r); }
    const float h = B.src[idx];
    if (!ps_finite(h)) continue;
    const double d = (double)h - (double)B.src[B.amin[r]];     // the anchor's height: the first finite member (the root itself whenever its height is finite)
    if (fabs(d) > EM_PLANE_Q_RANGE) { atomicAdd(&slots[slot].left_out, 1); continue; }
    if (slot != cur) {
      if (cur >= 0) ps_flush_moments(slots, cur, c);
      cur = slot;
#pragma unroll
      for (int e = 0; e < 10; ++e) c[e] = 0;
    }
    const int i = (int)(idx / M), j = (int)(idx - (long)i * M), ia = r / M, ja = r - ia * M;
    const long long di = i - ia, dj = j - ja, q = __double2ll_rn(d * (double)(1 << EM_PLANE_Q_BITS));
    c[0] += 1; c[1] += di; c[2] += dj; c[3] += q; c[4] += di * di; c[5] += dj * dj; c[6] += di * dj; c[7] += di * q; c[8] += dj * q; c[9] += q * q;
  }
  const bool valid = cur >= 0;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  int lead; bool mine;
  for (int g = 0; g < PS_GROUPS && ps_next_group(todo, valid, cur, lead, mine); ++g) {      // exact integer sums: the grouping does not change them
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const long long t = ps_wave_sum(mine ? c[k] : 0);
      if (lane == lead && t != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&slots[cur].s[k]), (unsigned long long)t);
    }
  }
  if (valid && ((todo >> lane) & 1)) ps_flush_moments(slots, cur, c);
}

// ---- g. one lane per slot ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ps_finalise(PlaneArgs A, PlaneBufs B, PlaneSlot* slots, int n_slots) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_slots) return;
  PlaneSlot& S = slots[k];
  const double n = (double)S.s[0], res = A.res, rr = res * res, u = 1.0 / (double)(1 << EM_PLANE_Q_BITS), uu = u * u;
  const double s[3] = {-((double)S.s[1] * res), -((double)S.s[2] * res), (double)S.s[3] * u};
  const double q[6] = {(double)S.s[4] * rr, (double)S.s[6] * rr, -((double)S.s[7] * res) * u, (double)S.s[5] * rr, -((double)S.s[8] * res) * u, (double)S.s[9] * uu};
  double nv[3] = {0.0, 0.0, 1.0}, err = 1e30;
  if (n >= 1.0) ps_plane_normal(n, s, q, nv, err);
  const int r = S.root, ia = r / A.M, ja = r - ia * A.M;
  const double ha = n >= 1.0 ? (double)B.src[B.amin[r]] : 0.0, nn = n >= 1.0 ? n : 1.0;
  S.support[0] = (A.ox - (double)ia * res) + s[0] / nn;
  S.support[1] = (A.oy - (double)ja * res) + s[1] / nn;
  S.support[2] = ha + s[2] / nn;
  S.normal[0] = nv[0]; S.normal[1] = nv[1]; S.normal[2] = nv[2];
  S.accept = nv[2] > A.cos_plane ? 1 : 0;                     // isWithinInclinationLimit (:302-304)
}

__global__ __launch_bounds__(EM_BLOCK) void k_ps_fold(PlaneArgs A, PlaneBufs B, PlaneSlot* slots, int* __restrict__ labels) {
  const int M = A.M;
  const long N = (long)M * M, base = ((long)blockIdx.x * EM_BLOCK + threadIdx.x) * PS_CPT;
  int cur = -1; unsigned long long kd = 0, kn = 0;
  for (int k = 0; k < PS_CPT; ++k) {
    const long idx = base + k;
    if (idx >= N) break;
    const int r = B.root[idx];
    int label = 0;
    if (r >= 0) {
      label = 1 + (int)ps_rank(B.mask1, B.offs1, r);
      if (ps_bit(B.mask2, r)) {
        const int slot = (int)ps_rank(B.mask2, B.offs2, r);
        const PlaneSlot& S = slots[slot];
        if (!S.accept) label = 0;                              // setToBackground (:306-308); the numbers of the other labels do not move
        const float h = B.src[idx];
        if (S.accept && ps_finite(h)) {                        // isGloballyPlanar (:277-300), folded per label
          const int i = (int)(idx / M), j = (int)(idx - (long)i * M);
          const double px = A.ox - (double)i * A.res, py = A.oy - (double)j * A.res, pz = (double)h;
          const double nx = S.normal[0], ny = S.normal[1], nz = S.normal[2];
          const double dist = fabs(((nx * px + ny * py) + nz * pz) - ((nx * S.support[0] + ny * S.support[1]) + nz * S.support[2]));
          const double dot = (nx * (double)B.nrm[idx] + ny * (double)B.nrm[N + idx]) + nz * (double)B.nrm[2 * N + idx];
          if (slot != cur) {
            if (cur >= 0) { atomicMax(&slots[cur].kdist, kd); atomicMax(&slots[cur].kdot, kn); }
            cur = slot; kd = 0; kn = 0;
          }
          const unsigned long long a = ps_key(dist), b = ps_key(-dot);
          kd = a > kd ? a : kd; kn = b > kn ? b : kn;
        }
      }
    }
    labels[idx] = label;
  }
  const bool valid = cur >= 0;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  int lead; bool mine;
  for (int g = 0; g < PS_GROUPS && ps_next_group(todo, valid, cur, lead, mine); ++g) {      // maxima: any grouping gives the same words
    const unsigned long long a = ps_wave_max(mine ? kd : 0), b = ps_wave_max(mine ? kn : 0);
    if (lane == lead) { atomicMax(&slots[cur].kdist, a); atomicMax(&slots[cur].kdot, b); }
  }
  if (valid && ((todo >> lane) & 1)) { atomicMax(&slots[cur].kdist, kd); atomicMax(&slots[cur].kdot, kn); }
}

// ---- h. the same union-find on a list of pairs (k, other[k]): the cycles of a permutation (the planar regions' cracks, emap_regions.hip) ------
__global__ __launch_bounds__(EM_BLOCK) void k_ps_link(int n, const int* __restrict__ other, int* parent) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k < n) ps_union_agent(parent, k, other[k]);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned int ps_blocks(long N) { return (unsigned int)((N + EM_BLOCK - 1) / EM_BLOCK); }
static inline unsigned int ps_fold_blocks(long N) { return (unsigned int)((N + EM_BLOCK * PS_CPT - 1) / (EM_BLOCK * PS_CPT)); }

void launch_ps_source(hipStream_t s, const KP& P, Cells cells, const LayerTab& tab, float* src) {
  const int nt = (P.C - 2 + T - 1) / T;
  hipLaunchKernelGGL(k_ps_source, dim3(nt * nt), dim3(EM_BLOCK), 0, s, P, cells, tab, nt, src);
}
void launch_ps_window(hipStream_t s, const PlaneArgs& A, const PlaneBufs& B) {
  const dim3 grid((A.M + PS_WT_C - 1) / PS_WT_C, (A.M + PS_WT_R - 1) / PS_WT_R), block(PS_WT_R * PS_WT_C);
  if (A.K == 3) hipLaunchKernelGGL(k_ps_window<3>, grid, block, 0, s, A, B.src, B.nrm, B.bit);
  else if (A.K == 5) hipLaunchKernelGGL(k_ps_window<5>, grid, block, 0, s, A, B.src, B.nrm, B.bit);
  else hipLaunchKernelGGL(k_ps_window<7>, grid, block, 0, s, A, B.src, B.nrm, B.bit);
}
void launch_ps_morph(hipStream_t s, int M, int radius, int dilate, const unsigned char* in, unsigned char* out) {
  hipLaunchKernelGGL(k_ps_morph, dim3(ps_blocks((long)M * M)), dim3(EM_BLOCK), 0, s, M, radius, dilate, in, out);
}
// local pass, border merge, flatten + root bits (launch_ps_components: also the planar terrain's NaN components, emap_terrain.hip), then
// member counts, slot bits: parent, root, cnt, amin, mask1, mask2 are written
void launch_ps_components(hipStream_t s, int M, int conn, const unsigned char* bit, int* parent, int* root, int* cnt, int* amin, unsigned int* mask1) {
  const int nt = (M + T - 1) / T;
  const long N = (long)M * M;
  hipLaunchKernelGGL(k_ps_local, dim3(nt * nt), dim3(EM_BLOCK), 0, s, M, conn, bit, parent, cnt, amin);
  if (nt > 1) hipLaunchKernelGGL(k_ps_merge, dim3(ps_blocks(N)), dim3(EM_BLOCK), 0, s, M, conn, bit, parent);
  hipLaunchKernelGGL(k_ps_flatten, dim3(ps_blocks(N)), dim3(EM_BLOCK), 0, s, N, parent, root, mask1);
}
void launch_ps_link(hipStream_t s, int n, const int* other, int* parent) {
  if (n > 0) hipLaunchKernelGGL(k_ps_link, dim3(ps_blocks(n)), dim3(EM_BLOCK), 0, s, n, other, parent);
}
void launch_ps_labels(hipStream_t s, const PlaneArgs& A, const PlaneBufs& B, const unsigned char* bit) {
  const long N = (long)A.M * A.M;
  launch_ps_components(s, A.M, A.conn, bit, B.parent, B.root, B.cnt, B.amin, B.mask1);
  hipLaunchKernelGGL(k_ps_count, dim3(ps_fold_blocks(N)), dim3(EM_BLOCK), 0, s, N, B.src, B.root, B.cnt, B.amin);
  hipLaunchKernelGGL(k_ps_bits2, dim3(ps_blocks(N)), dim3(EM_BLOCK), 0, s, N, A.min_points, B.root, B.cnt, B.mask2);
}
void launch_ps_moments(hipStream_t s, const PlaneArgs& A, const PlaneBufs& B, PlaneSlot* slots) {
  hipLaunchKernelGGL(k_ps_moments, dim3(ps_fold_blocks((long)A.M * A.M)), dim3(EM_BLOCK), 0, s, A, B, slots);
}
void launch_ps_planes(hipStream_t s, const PlaneArgs& A, const PlaneBufs& B, PlaneSlot* slots, int n_slots, int* labels) {
  if (n_slots > 0) hipLaunchKernelGGL(k_ps_finalise, dim3((n_slots + 63) / 64), dim3(64), 0, s, A, B, slots, n_slots);
  hipLaunchKernelGGL(k_ps_fold, dim3(ps_fold_blocks((long)A.M * A.M)), dim3(EM_BLOCK), 0, s, A, B, slots, labels);
}
