// Planar regions on the device (gfx950): the middle stage of convex_plane_decomposition's PlaneDecompositionPipeline::update --
// ContourExtraction::extractPlanarRegions (ContourExtraction.cpp:28-128) on the x 3 upsampled label image (Upsampling.cpp:12-68): per
// connected piece of a label a boundary polygon with holes and its inset polygons.  The contract (upsampling rule, all-label erosions,
// the local fallback, crack cycles, vertex rule, order of the answer) is DESIGN.md section 23; OpenCV's erode / findContours and CGAL's
// isInside are RESTATED there, neither is pinned by a compiled reference.  Every image is dense U x U, pixel (r, c) at idx = r * U + c
// (U = 3 M - 2; raw mode: U = M, the plane traced as it is).  Crack (p, s) has the index 4 idx(p) + s: side 0 the top edge travelled
// west, 1 the left edge travelled south, 2 the bottom edge travelled east, 3 the right edge travelled north -- the foreground on the
// left hand.  A chain of launches, nothing waited for in between but the crack count:
//
//   k_rg_erode     per pixel two bits: the pixel survives the margin ellipse (A_m) / the 3 x 3 cross (A_c), all labels in one pass,
//                  indices clamped at the edge.  The upsampled image is never written: a pixel reads its cell.
//   k_rg_bm        the byte "in B_m": the cross erosion of A_m with the frame zeroed.
//   k_rg_flag      flag[L] |= 1 where a pixel of B_m with label L has an 8-neighbour of B_m with label L (an idempotent atomic OR, one per
//                  wave and label): the label keeps its margin, otherwise it falls back to A_c.
//   k_rg_images    A (the per-label choice) and B (its cross erosion, frame zeroed) as int planes, and their "!= 0" bytes.
//   k_ps_local / _merge / _flatten (emap_planeseg.hip, launch_ps_components, conn = 8) on both: every pixel's component root.
//   k_rg_cracks    4 bits per pixel "crack (p, s) exists", a word per 8 pixels, A's words in front of B's.
//   k_cloud_scan   (emap_cloudout.hip) the order-fixed prefix: a crack's COMPACT index is its rank, so A's cracks precede B's and the
//                  smallest compact index of a cycle is its smallest crack.  -- the crack count travels to the host, a wait --
//   k_rg_succ      per crack its raw index, its successor (compact) and, scattered through the permutation, its predecessor.
//   k_ps_link      (emap_planeseg.hip) every crack united with its successor by the segmentation's union-find: the root of a cycle is its
//                  smallest crack whatever the order of the atomics.  k_rg_vertex: the vertex bit of every crack.
//   k_rg_flatten   cyc[] = every crack's root, a plane of its own; the bit "is a root"; the doubling's first buffer.
//   k_rg_double    ceil(log2 n_cracks) times, double buffered: (next, vertices from here to the ring's end), the root as terminal.
//   k_cloud_scan   the rank of every ring among the rings; k_rg_ring_count, k_rg_scan (the exclusive prefix of the ring's vertex counts,
//                  one workgroup) and k_rg_write: ring records and vertices.  No atomic decides a position.
//
// No lane walks a border: a crack looks at most 3 cracks back (its owner's run) and once ahead.
#include "emap_launch.h"

namespace {
__device__ __forceinline__ int rg_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// the cell pixel u reads (Upsampling.cpp:12-58): the first and the last cell give 2 pixels, the others 3
__device__ __forceinline__ int rg_cell(int u, int U, int M) { return u < 2 ? 0 : (u >= U - 2 ? M - 1 : 1 + (u - 2) / 3); }
__device__ __forceinline__ int rg_label(const RegionArgs& G, const int* __restrict__ labels, int r, int c) {
  return labels[(long)rg_cell(r, G.U, G.M) * G.M + rg_cell(c, G.U, G.M)];
}
__device__ __forceinline__ unsigned int rg_rank(const unsigned int* __restrict__ mask, const unsigned int* __restrict__ offs, long bit) {
  return offs[bit >> 5] + __popc(mask[bit >> 5] & ((1u << (bit & 31)) - 1u));
}
// side s: the direction of travel and the pixel across the edge, as (row, column) steps
__device__ __forceinline__ void rg_dirs(int s, int& dr, int& dc, int& br, int& bc) {
  dr = s == 1 ? 1 : (s == 3 ? -1 : 0); dc = s == 0 ? -1 : (s == 2 ? 1 : 0);
  br = s == 0 ? -1 : (s == 2 ? 1 : 0); bc = s == 1 ? -1 : (s == 3 ? 1 : 0);
}
__device__ __forceinline__ int rg_at(const int* __restrict__ X, int U, int r, int c) { return (r >= 0 && r < U && c >= 0 && c < U) ? X[(long)r * U + c] : 0; }
}  // namespace

// ---- a. erosions, fallback, images -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_rg_erode(RegionArgs G, TerrainSpans sp, const int* __restrict__ labels, unsigned char* __restrict__ em) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const int U = G.U;
  if (idx >= (long)U * U) return;
  const int r = (int)(idx / U), c = (int)(idx - (long)r * U), L = rg_label(G, labels, r, c);
  int bits = 0;
  if (L != 0) {
    const bool cross = rg_label(G, labels, rg_clamp(r - 1, U - 1), c) == L && rg_label(G, labels, rg_clamp(r + 1, U - 1), c) == L &&
                       rg_label(G, labels, r, rg_clamp(c - 1, U - 1)) == L && rg_label(G, labels, r, rg_clamp(c + 1, U - 1)) == L;
    bool ell = cross;                                          // every such ellipse contains the cross
    const int h = G.k / 2;
    for (int a = 0; a < G.k && ell; ++a) {
      const int rr = rg_clamp(r + a - h, U - 1);
      for (int b = sp.lo[a]; b < sp.hi[a]; ++b)
        if (rg_label(G, labels, rr, rg_clamp(c + b - h, U - 1)) != L) { ell = false; break; }
    }
    bits = (ell ? 1 : 0) | (cross ? 2 : 0);
  }
  em[idx] = (unsigned char)bits;
}

__global__ __launch_bounds__(EM_BLOCK) void k_rg_bm(RegionArgs G, const int* __restrict__ labels, const unsigned char* __restrict__ em, unsigned char* __restrict__ bm) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const int U = G.U;
  if (idx >= (long)U * U) return;
  const int r = (int)(idx / U), c = (int)(idx - (long)r * U);
  bool in = false;
  if (r > 0 && r < U - 1 && c > 0 && c < U - 1 && (em[idx] & 1)) {      // the frame is zeroed: every neighbour is inside
    const int L = rg_label(G, labels, r, c);
    in = (em[idx - U] & 1) && (em[idx + U] & 1) && (em[idx - 1] & 1) && (em[idx + 1] & 1) && rg_label(G, labels, r - 1, c) == L &&
         rg_label(G, labels, r + 1, c) == L && rg_label(G, labels, r, c - 1) == L && rg_label(G, labels, r, c + 1) == L;
  }
  bm[idx] = in ? 1 : 0;
}

__global__ __launch_bounds__(EM_BLOCK) void k_rg_flag(RegionArgs G, const int* __restrict__ labels, const unsigned char* __restrict__ bm, unsigned int* flag) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const int U = G.U;
  bool found = false; int L = 0;
  if (idx < (long)U * U && bm[idx]) {                          // (a pixel of B_m is not on the frame)
    const int r = (int)(idx / U), c = (int)(idx - (long)r * U);
    L = rg_label(G, labels, r, c);
    for (int a = -1; a <= 1 && !found; ++a)
      for (int b = -1; b <= 1; ++b)
        if ((a || b) && bm[idx + (long)a * U + b] && rg_label(G, labels, r + a, c + b) == L) { found = true; break; }
  }
  unsigned long long todo = __ballot(found);                   // one OR per wave and label; the OR is idempotent, so who sends it does not matter
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1, L0 = __shfl(L, lead, 64);
    const bool mine = found && L == L0;
    todo &= ~__ballot(mine);
    if (lane == lead && __hip_atomic_load(&flag[L], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(&flag[L], 1u);
  }
}

namespace {
// A at a pixel INSIDE the image
__device__ __forceinline__ int rg_a(const RegionArgs& G, const int* __restrict__ labels, const unsigned char* __restrict__ em, const unsigned int* __restrict__ flag, int r, int c) {
  if (G.mode == 1) return labels[(long)r * G.U + c];
  const int L = rg_label(G, labels, r, c);
  if (L == 0) return 0;
  const int e = em[(long)r * G.U + c];
  return (flag[L] ? (e & 1) : (e & 2)) ? L : 0;
}
}  // namespace

__global__ __launch_bounds__(EM_BLOCK) void k_rg_images(RegionArgs G, const int* __restrict__ labels, const unsigned char* __restrict__ em, const unsigned int* __restrict__ flag,
                                                        int* __restrict__ A, int* __restrict__ B, unsigned char* __restrict__ bitA, unsigned char* __restrict__ bitB) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const int U = G.U;
  if (idx >= (long)U * U) return;
  const int r = (int)(idx / U), c = (int)(idx - (long)r * U);
  const int a = rg_a(G, labels, em, flag, r, c);
  int b = 0;
  if (a != 0 && r > 0 && r < U - 1 && c > 0 && c < U - 1 && rg_a(G, labels, em, flag, r - 1, c) == a && rg_a(G, labels, em, flag, r + 1, c) == a &&
      rg_a(G, labels, em, flag, r, c - 1) == a && rg_a(G, labels, em, flag, r, c + 1) == a) b = a;
  A[idx] = a; B[idx] = b; bitA[idx] = a != 0; bitB[idx] = b != 0;
}

// ---- b. cracks ---------------------------------------------------------------------------------------------------------------------------
// word w of image `img` (at cmask[img * Wc + w]) holds the cracks of the pixels 8 w .. 8 w + 7: bit 4 (idx & 7) + s
__global__ __launch_bounds__(EM_BLOCK) void k_rg_cracks(int U, long Wc, const int* __restrict__ A, const int* __restrict__ B, unsigned int* __restrict__ cmask) {
  const long t = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (t >= 2 * Wc) return;
  const int img = t >= Wc ? 1 : 0;
  const long w = t - (long)img * Wc, N = (long)U * U;
  const int* __restrict__ X = img ? B : A;
  unsigned int word = 0;
  for (int e = 0; e < 8; ++e) {
    const long idx = 8 * w + e;
    if (idx >= N) break;
    const int v = X[idx];
    if (v == 0) continue;
    const int r = (int)(idx / U), c = (int)(idx - (long)r * U);
    const unsigned int b = (rg_at(X, U, r - 1, c) != v ? 1u : 0u) | (rg_at(X, U, r, c - 1) != v ? 2u : 0u) | (rg_at(X, U, r + 1, c) != v ? 4u : 0u) |
                           (rg_at(X, U, r, c + 1) != v ? 8u : 0u);
    word |= b << (4 * e);
  }
  cmask[t] = word;
}

// one thread per pixel and image: raw[k] = image << 31 | crack, succ[k], pred[succ[k]] = k (a permutation: every word is written once),
// parent[k] = k
__global__ __launch_bounds__(EM_BLOCK) void k_rg_succ(int U, long Wc, const int* __restrict__ A, const int* __restrict__ B, const unsigned int* __restrict__ cmask,
                                                      const unsigned int* __restrict__ coffs, unsigned int* __restrict__ raw, int* __restrict__ succ, int* __restrict__ pred, int* __restrict__ parent) {
  const long t = (long)blockIdx.x * EM_BLOCK + threadIdx.x, N = (long)U * U;
  if (t >= 2 * N) return;
  const int img = t >= N ? 1 : 0;
  const long idx = t - (long)img * N, base = (long)img * Wc * 32;
  const unsigned int four = (cmask[img * Wc + (idx >> 3)] >> (4 * (idx & 7))) & 15u;
  if (!four) return;
  const int* __restrict__ X = img ? B : A;
  const int r = (int)(idx / U), c = (int)(idx - (long)r * U), v = X[idx];
  for (int s = 0; s < 4; ++s) {
    if (!((four >> s) & 1u)) continue;
    int dr, dc, br, bc; rg_dirs(s, dr, dc, br, bc);
    long o; int so;
    if (rg_at(X, U, r + br + dr, c + bc + dc) == v) { o = idx + (long)(br + dr) * U + (bc + dc); so = (s + 3) & 3; }      // turn right
    else if (rg_at(X, U, r + dr, c + dc) == v) { o = idx + (long)dr * U + dc; so = s; }                                      // straight
    else { o = idx; so = (s + 1) & 3; }                                                                                      // turn left
    const int k = (int)rg_rank(cmask, coffs, base + 4 * idx + s), ks = (int)rg_rank(cmask, coffs, base + 4 * o + so);
    raw[k] = ((unsigned int)img << 31) | (unsigned int)(4 * idx + s);
    succ[k] = ks; pred[ks] = k; parent[k] = k;
  }
}

// the vertex bit: crack k is the LAST crack of its owner's run (at most 4 cracks) and the chain pixel's incoming step differs from its
// outgoing step (CHAIN_APPROX_SIMPLE); the crack (p, 0) of an isolated pixel, whose ring has one owner
__global__ __launch_bounds__(EM_BLOCK) void k_rg_vertex(int U, int n, const unsigned int* __restrict__ raw, const int* __restrict__ succ, const int* __restrict__ pred,
                                                        unsigned char* __restrict__ vbit) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int nx = succ[k];
  const unsigned int own = raw[k] >> 2, onx = raw[nx] >> 2;      // (the image bit travels along: cracks of two images never share a ring)
  bool v = false;
  if (onx != own) {
    int f = k;
    for (int e = 0; e < 3; ++e) { const int b = pred[f]; if ((raw[b] >> 2) != own) break; f = b; }
    const unsigned int oin = raw[pred[f]] >> 2, m = 0x1fffffffu;
    const int p = (int)(own & m), q = (int)(oin & m), z = (int)(onx & m);
    v = (p / U - q / U != z / U - p / U) || (p % U - q % U != z % U - p % U);
  } else if ((raw[k] & 3u) == 0u) {
    v = succ[succ[succ[nx]]] == k;                             // the ring IS the pixel's four sides (a pixel that hangs on a diagonal has the same run inside a longer ring)
  }
  vbit[k] = v ? 1 : 0;
}

// a launch of its own: parent[] is final and read plainly
__global__ __launch_bounds__(EM_BLOCK) void k_rg_flatten(int n, const int* __restrict__ parent, const int* __restrict__ succ, const unsigned char* __restrict__ vbit,
                                                         int* __restrict__ cyc, unsigned int* __restrict__ hmask, int2* __restrict__ nv) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  int x = -1;
  if (k < n) {
    x = parent[k];
    for (;;) { const int p = parent[x]; if (p == x) break; x = p; }      // strictly decreasing
    cyc[k] = x;
    nv[k] = x == k ? make_int2(k, 0) : make_int2(succ[k], (int)vbit[k]);
  }
  const unsigned long long b = __ballot(k < n && x == k);
  if ((threadIdx.x & 63) == 0) { const int w = k >> 5; hmask[w] = (unsigned int)b; hmask[w + 1] = (unsigned int)(b >> 32); }
}

__global__ __launch_bounds__(EM_BLOCK) void k_rg_double(int n, const int2* __restrict__ in, int2* __restrict__ out) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int2 a = in[k], b = in[a.x];
  out[k] = make_int2(b.x, a.y + b.y);
}

__global__ __launch_bounds__(EM_BLOCK) void k_rg_ring_count(int n, const int* __restrict__ cyc, const int* __restrict__ succ, const unsigned char* __restrict__ vbit, const int2* __restrict__ nv,
                                                            const unsigned int* __restrict__ hmask, const unsigned int* __restrict__ hoffs, int* __restrict__ rcnt) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= n || cyc[k] != k) return;
  rcnt[rg_rank(hmask, hoffs, k)] = (int)vbit[k] + nv[succ[k]].y;
}

// ONE workgroup: first[] = the exclusive prefix of cnt[0 .. *n_rings), the total to *total.  Integer sums: the order is free
__global__ __launch_bounds__(EM_CLOUD_SCAN_BLOCK) void k_rg_scan(const unsigned int* __restrict__ n_rings, const int* __restrict__ cnt, int* __restrict__ first, unsigned int* __restrict__ total) {
  constexpr int NW = EM_CLOUD_SCAN_BLOCK / 64;
  __shared__ int wsum[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = (int)*n_rings;
  int carry = 0;
  for (int base = 0; base < n; base += EM_CLOUD_SCAN_BLOCK) {  // uniform
    const int i = base + tid, s = i < n ? cnt[i] : 0;
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const int t = wsum[w]; all += t; if (w < wave) before += t; }
    if (i < n) first[i] = carry + before + (incl - s);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = (unsigned int)carry;
}

// the head of a ring writes its record; a crack with the vertex bit writes its owner at the ring's first vertex + the vertices met from
// the smallest crack on before it
__global__ __launch_bounds__(EM_BLOCK) void k_rg_write(int U, int n, const unsigned int* __restrict__ raw, const int* __restrict__ succ, const int* __restrict__ cyc, const unsigned char* __restrict__ vbit,
                                                       const int2* __restrict__ nv, const unsigned int* __restrict__ hmask, const unsigned int* __restrict__ hoffs, const int* __restrict__ rcnt,
                                                       const int* __restrict__ rfirst, const int* __restrict__ A, const int* __restrict__ B, const int* __restrict__ rootA,
                                                       const int* __restrict__ rootB, RegionRing* __restrict__ rings, int2* __restrict__ verts) {
  const int k = blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int head = cyc[k], ring = (int)rg_rank(hmask, hoffs, head);
  const unsigned int w = raw[k];
  const int img = (int)(w >> 31), crack = (int)(w & 0x7fffffffu), pix = crack >> 2;
  if (head == k) {
    const int root = (img ? rootB : rootA)[pix];
    RegionRing R;
    R.first_vertex = rfirst[ring]; R.n_vertices = rcnt[ring]; R.image = img; R.is_hole = (pix == root && (crack & 3) == 0) ? 0 : 1;
    R.label = (img ? B : A)[pix]; R.root = root; R.crack = crack; R.boundary = rootA[root];      // B is a subset of A pixelwise: rootA[root] is a root
    rings[ring] = R;
  }
  if (vbit[k]) {
    const int at = head == k ? 0 : (int)vbit[head] + nv[succ[head]].y - nv[k].y;
    if (at >= 0 && at < rcnt[ring]) verts[rfirst[ring] + at] = make_int2(pix % U, pix / U);      // (always so: the positions of a ring's vertices are 0 .. n - 1, each once)
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned int rg_blocks(long n) { return (unsigned int)((n + EM_BLOCK - 1) / EM_BLOCK); }

void launch_rg_images(hipStream_t s, const RegionArgs& G, const TerrainSpans& sp, const RegionBufs& R) {
  const long N = (long)G.U * G.U;
  if (G.mode == 0) {
    hipLaunchKernelGGL(k_rg_erode, dim3(rg_blocks(N)), dim3(EM_BLOCK), 0, s, G, sp, R.labels, R.em);
    hipLaunchKernelGGL(k_rg_bm, dim3(rg_blocks(N)), dim3(EM_BLOCK), 0, s, G, R.labels, R.em, R.bm);
    hipLaunchKernelGGL(k_rg_flag, dim3(rg_blocks(N)), dim3(EM_BLOCK), 0, s, G, R.labels, R.bm, R.flag);
  }
  hipLaunchKernelGGL(k_rg_images, dim3(rg_blocks(N)), dim3(EM_BLOCK), 0, s, G, R.labels, R.em, R.flag, R.A, R.B, R.bitA, R.bitB);
}
void launch_rg_cracks(hipStream_t s, const RegionArgs& G, const RegionBufs& R) {
  hipLaunchKernelGGL(k_rg_cracks, dim3(rg_blocks(2 * G.Wc)), dim3(EM_BLOCK), 0, s, G.U, G.Wc, R.A, R.B, R.cmask);
}
// everything behind the crack count n (> 0): successors, cycles, vertex ranks, ring records, vertices; head[1] / head[2] get the ring and
// vertex counts
void launch_rg_trace(hipStream_t s, const RegionArgs& G, const RegionBufs& R, const RegionCracks& K, int n) {
  const long N = (long)G.U * G.U;
  hipLaunchKernelGGL(k_rg_succ, dim3(rg_blocks(2 * N)), dim3(EM_BLOCK), 0, s, G.U, G.Wc, R.A, R.B, R.cmask, R.coffs, K.raw, K.succ, K.pred, K.parent);
  launch_ps_link(s, n, K.succ, K.parent);
  hipLaunchKernelGGL(k_rg_vertex, dim3(rg_blocks(n)), dim3(EM_BLOCK), 0, s, G.U, n, K.raw, K.succ, K.pred, K.vbit);
  hipLaunchKernelGGL(k_rg_flatten, dim3(rg_blocks(n)), dim3(EM_BLOCK), 0, s, n, K.parent, K.succ, K.vbit, K.cyc, K.hmask, K.nv[0]);
  int cur = 0;
  for (int r = 0; r < region_rounds(n); ++r, cur ^= 1) hipLaunchKernelGGL(k_rg_double, dim3(rg_blocks(n)), dim3(EM_BLOCK), 0, s, n, K.nv[cur], K.nv[cur ^ 1]);
  launch_cloud_scan(s, K.hmask, K.hoffs, ((long)n + 31) / 32, R.head + 1);
  hipLaunchKernelGGL(k_rg_ring_count, dim3(rg_blocks(n)), dim3(EM_BLOCK), 0, s, n, K.cyc, K.succ, K.vbit, K.nv[cur], K.hmask, K.hoffs, K.rcnt);
  hipLaunchKernelGGL(k_rg_scan, dim3(1), dim3(EM_CLOUD_SCAN_BLOCK), 0, s, R.head + 1, K.rcnt, K.rfirst, R.head + 2);
  hipLaunchKernelGGL(k_rg_write, dim3(rg_blocks(n)), dim3(EM_BLOCK), 0, s, G.U, n, K.raw, K.succ, K.cyc, K.vbit, K.nv[cur], K.hmask, K.hoffs, K.rcnt, K.rfirst, R.A, R.B, R.rootA,
                     R.rootB, K.rings, K.verts);
}
