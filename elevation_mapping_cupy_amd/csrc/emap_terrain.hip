// Planar terrain on the device (gfx950): what convex_plane_decomposition publishes around its segmentation, on planes that already lie on
// the device -- GridMapPreprocessing::preprocess (GridMapPreprocessing.cpp:14-39: minValues inpainting, inpainting.cpp:25-94, and
// cv::medianBlur, smoothing.cpp:23-42) in front of it and Postprocessing::postprocess (Postprocessing.cpp:14-31: smooth_planar, :73-144;
// the dilation in non-planar regions, :33-53; the height offsets, :55-65) behind it.  The contract is DESIGN.md section 22; OpenCV and
// grid_map are RESTATED there, neither is pinned by a compiled reference.  Every plane is dense M x M in published index space, cell
// (i, j) at idx = i * M + j.  The stencils give a workgroup a 32 x 32 tile, a thread four of its cells, and stage the tile with the
// rows and columns its windows reach into LDS once -- at most 62 x 62 floats, indices clamped at the map's border (BORDER_REPLICATE).
//
//   k_tr_nanbit    the byte plane isnan(src); k_ps_local / k_ps_merge / k_ps_flatten (emap_planeseg.hip, connectivity 4) find the root
//                  of every NaN cell.
//   k_tr_rim       every cell that is not NaN and has a NaN 4-neighbour: atomicMin of its key on amin[root of that neighbour].  A
//                  minimum of integers: the order of the atomics does not matter.  No spin, no barrier across workgroups.
//   k_tr_fill      a NaN cell takes the value behind its root's key; a component without a rim (the all-NaN map) stays as it is.
//   k_tr_median<K> the (K^2 - 1) / 2-th order statistic of the clamp-indexed K x K window, by rank counting on keys held in registers;
//                  a window with a NaN gives NaN.
//   k_tr_mask      w = label > 0 ? e : NaN, the 0 / 1 float mask, and isnan(w) for the second inpainting.
//   k_tr_morph     maximum or minimum over OpenCV's elliptic element (row spans from the table), NaN skipped.
//   k_tr_sloped    max over the finite x - off of the SHIFTED (not clipped) window of grid_map's applyKernelFunction.
//   k_tr_blur      s = sum_a t[a] * (sum_b t[b] * double(x)), rows outer, columns inner, both ascending, in double: the inner sums of a
//                  tile's rows once in LDS, then the outer sum.  Box (t = 1, scaled by 1 / k^2) and Gaussian (taps from the table).
//   k_tr_lift      m e + (1 - m) d, + float(a + b), - float(b) m: Postprocessing.cpp:50, :57, :60 in float, literally.
// Every NaN a kernel of this file computes or makes up is written as the quiet NaN 0x7fc00000; a NaN that is only passed on (k_tr_fill)
// keeps its bits.
#include "emap_launch.h"

namespace {
constexpr int TT = 32, TR_NK = TT * TT / EM_BLOCK, TR_LW = TT + EM_TERRAIN_KERNEL_MAX - 1, TR_LS = TR_LW + 1;      // tile side, cells a thread, staged side, its stride
constexpr int TR_NO_KEY = 0x7fffffff;                          // amin[] as k_ps_local leaves it: above the key of every value that is not NaN
static_assert(TT * TT % EM_BLOCK == 0 && EM_TERRAIN_KERNEL_MAX % 2 == 1, "tile");

__device__ __forceinline__ bool tr_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool tr_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float tr_quiet_nan() { return __uint_as_float(0x7fc00000u); }
// monotone key of a float that is not NaN: signed order = numeric order, -0 below +0; its own inverse
__device__ __forceinline__ int tr_key(float v) { const int b = __float_as_int(v); return b >= 0 ? b : b ^ 0x7fffffff; }
__device__ __forceinline__ float tr_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
__device__ __forceinline__ int tr_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// rows r0 .. r0 + nr - 1, columns c0 .. c0 + nc - 1 of `in` into LDS, indices clamped to the map; every thread of the workgroup calls it
__device__ __forceinline__ void tr_stage(const float* __restrict__ in, int M, int r0, int c0, int nr, int nc, float* tile) {
  for (int e = threadIdx.x; e < nr * nc; e += EM_BLOCK) {
    const int lr = e / nc, lc = e - lr * nc;
    tile[lr * TR_LS + lc] = in[(long)tr_clamp(r0 + lr, M - 1) * M + tr_clamp(c0 + lc, M - 1)];
  }
  __syncthreads();
}
// corner of grid_map's kernel window (processing.cpp:160-171): moved inwards at an edge, not clipped
__device__ __forceinline__ int tr_corner(int i, int h, int k, int M) {
  const int c = i - h < 0 ? 0 : i - h;
  return c + k > M ? M - k : c;
}
}  // namespace

// ---- P1: minValues inpainting ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_tr_nanbit(long N, const float* __restrict__ in, unsigned char* __restrict__ bit) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx < N) bit[idx] = tr_nan(in[idx]) ? 1 : 0;
}

__global__ __launch_bounds__(EM_BLOCK) void k_tr_rim(int M, const float* __restrict__ in, const unsigned char* __restrict__ bit, const int* __restrict__ root, int* amin) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= (long)M * M || bit[idx]) return;
  const int i = (int)(idx / M), j = (int)(idx - (long)i * M), key = tr_key(in[idx]);
  int done = -1;                                               // two neighbours mostly share a root: one atomic
  const long nb[4] = {j > 0 ? idx - 1 : -1, j < M - 1 ? idx + 1 : -1, i > 0 ? idx - M : -1, i < M - 1 ? idx + M : -1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (nb[k] < 0 || !bit[nb[k]]) continue;
    const int r = root[nb[k]];
    if (r == done) continue;
    done = r;
    // amin[r] only ever decreases: a value read earlier that is not above the key already settles it
    if (__hip_atomic_load(&amin[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(&amin[r], key);      // (device scope)
  }
}

// (in == out is allowed: a cell reads and writes only itself)
__global__ __launch_bounds__(EM_BLOCK) void k_tr_fill(long N, const float* in, const unsigned char* __restrict__ bit, const int* __restrict__ root, const int* __restrict__ amin, float* out) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= N) return;
  float v = in[idx];
  if (bit[idx]) { const int k = amin[root[idx]]; if (k != TR_NO_KEY) v = tr_unkey(k); }
  out[idx] = v;
}

// ---- P2: median --------------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(EM_BLOCK) void k_tr_median(int M, const float* __restrict__ in, float* __restrict__ out) {
  constexpr int H = K / 2, MID = (K * K - 1) / 2;
  __shared__ float tile[(TT + 2 * H) * TR_LS];
  const int nt = (M + TT - 1) / TT, tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt, i0 = tr * TT, j0 = tc * TT;
  tr_stage(in, M, i0 - H, j0 - H, TT + 2 * H, TT + 2 * H, tile);
  const int x = threadIdx.x & (TT - 1), y = threadIdx.x / TT;
#pragma unroll 1
  for (int k = 0; k < TR_NK; ++k) {
    const int ly = y + (TT / TR_NK) * k, i = i0 + ly, j = j0 + x;
    if (i >= M || j >= M) continue;                            // (behind the only barrier)
    int key[K * K]; bool nan = false;
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int b = 0; b < K; ++b) { const float v = tile[(ly + a) * TR_LS + x + b]; nan = nan || tr_nan(v); key[a * K + b] = tr_key(v); }
    int med = 0;
#pragma unroll
    for (int c = 0; c < K * K; ++c) {                          // the value with at most MID keys below it and more than MID not above it
      int less = 0, leq = 0;
#pragma unroll
      for (int e = 0; e < K * K; ++e) { less += key[e] < key[c] ? 1 : 0; leq += key[e] <= key[c] ? 1 : 0; }
      if (less <= MID && MID < leq) med = key[c];
    }
    out[(long)i * M + j] = nan ? tr_quiet_nan() : tr_unkey(med);
  }
}

// ---- Q1: the planar heights, the mask -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_tr_mask(long N, const float* __restrict__ e, const int* __restrict__ labels, float* __restrict__ w, float* __restrict__ m,
                                                      unsigned char* __restrict__ bit) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= N) return;
  const bool planar = labels[idx] > 0;
  const float v = planar ? e[idx] : tr_quiet_nan();
  w[idx] = v; m[idx] = planar ? 1.0f : 0.0f; bit[idx] = tr_nan(v) ? 1 : 0;
}

// ---- Q2 / Q5: maximum or minimum over the elliptic element --------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_tr_morph(int M, int kd, int dilate, const TerrainSpans* __restrict__ spans, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float tile[TR_LW * TR_LS];
  const int h = kd / 2, nt = (M + TT - 1) / TT, tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt, i0 = tr * TT, j0 = tc * TT;
  tr_stage(in, M, i0 - h, j0 - h, TT + 2 * h, TT + 2 * h, tile);
  const int x = threadIdx.x & (TT - 1), y = threadIdx.x / TT;
#pragma unroll 1
  for (int k = 0; k < TR_NK; ++k) {
    const int ly = y + (TT / TR_NK) * k, i = i0 + ly, j = j0 + x;
    if (i >= M || j >= M) continue;
    int best = 0; bool any = false;
    for (int a = 0; a < kd; ++a) {
      const int lo = spans->lo[a], hi = spans->hi[a];
      for (int b = lo; b < hi; ++b) {
        const float v = tile[(ly + a) * TR_LS + x + b];
        if (tr_nan(v)) continue;
        const int q = tr_key(v);
        best = !any ? q : (dilate ? (q > best ? q : best) : (q < best ? q : best));
        any = true;
      }
    }
    out[(long)i * M + j] = any ? tr_unkey(best) : tr_quiet_nan();
  }
}

// ---- Q3: the sloped dilation ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_tr_sloped(int M, int kd, const float* __restrict__ off, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float tile[TR_LW * TR_LS];
  const int h = kd / 2, nt = (M + TT - 1) / TT, tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt, i0 = tr * TT, j0 = tc * TT;
  // the corner moves by at most one cell from a cell to the next: the windows of 32 consecutive cells span at most 31 + kd rows
  const int r0 = tr_corner(i0, h, kd, M), c0 = tr_corner(j0, h, kd, M);
  tr_stage(in, M, r0, c0, TT + kd - 1, TT + kd - 1, tile);
  const int x = threadIdx.x & (TT - 1), y = threadIdx.x / TT;
#pragma unroll 1
  for (int k = 0; k < TR_NK; ++k) {
    const int ly = y + (TT / TR_NK) * k, i = i0 + ly, j = j0 + x;
    if (i >= M || j >= M) continue;
    const int lr = tr_corner(i, h, kd, M) - r0, lc = tr_corner(j, h, kd, M) - c0;
    int best = 0; bool any = false;
    for (int a = 0; a < kd; ++a)
      for (int b = 0; b < kd; ++b) {
        const float v = tile[(lr + a) * TR_LS + lc + b] - off[a * kd + b];
        if (!tr_finite(v)) continue;
        const int q = tr_key(v);
        best = (!any || q > best) ? q : best;
        any = true;
      }
    out[(long)i * M + j] = any ? tr_unkey(best) : tr_quiet_nan();
  }
}

// ---- Q4: box mean and Gaussian -------------------------------------------------------------------------------------------------------------
// taps == nullptr: the box (every tap 1.0, the sum scaled by `scale` = 1 / k^2); else the sum itself
__global__ __launch_bounds__(EM_BLOCK) void k_tr_blur(int M, int kk, const float* __restrict__ taps, double scale, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float tile[TR_LW * TR_LS];
  __shared__ double inner[TR_LW * TT];                         // per staged row and tile column: the sum over the window's columns
  const int h = kk / 2, nt = (M + TT - 1) / TT, tr = blockIdx.x / nt, tc = blockIdx.x - tr * nt, i0 = tr * TT, j0 = tc * TT;
  tr_stage(in, M, i0 - h, j0 - h, TT + 2 * h, TT + 2 * h, tile);
  for (int e = threadIdx.x; e < (TT + 2 * h) * TT; e += EM_BLOCK) {
    const int lr = e / TT, x = e - lr * TT;
    double s = 0.0;
    for (int b = 0; b < kk; ++b) s += (taps ? (double)taps[b] : 1.0) * (double)tile[lr * TR_LS + x + b];
    inner[lr * TT + x] = s;
  }
  __syncthreads();
  const int x = threadIdx.x & (TT - 1), y = threadIdx.x / TT;
#pragma unroll 1
  for (int k = 0; k < TR_NK; ++k) {
    const int ly = y + (TT / TR_NK) * k, i = i0 + ly, j = j0 + x;
    if (i >= M || j >= M) continue;                            // (behind the last barrier)
    double s = 0.0;
    for (int a = 0; a < kk; ++a) s += (taps ? (double)taps[a] : 1.0) * inner[(ly + a) * TT + x];
    const float v = taps ? (float)s : (float)(s * scale);
    out[(long)i * M + j] = tr_nan(v) ? tr_quiet_nan() : v;    // one NaN: the sign of an invalid operation's NaN differs between machines
  }
}

// ---- Q5 / Q6: the merge and the height offsets ---------------------------------------------------------------------------------------------
// d == nullptr: no dilation in non-planar regions (nonplanar_horizontal_offset == 0)
__global__ __launch_bounds__(EM_BLOCK) void k_tr_lift(long N, const float* __restrict__ e, const float* __restrict__ d, const float* __restrict__ m, int add_on, float add, int sub_on,
                                                      float sub, float* __restrict__ out) {
  const long idx = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (idx >= N) return;
  const float mk = m[idx];
  float v = e[idx];
  if (d) v = mk * v + (1.0f - mk) * d[idx];                    // (:50) a NaN e stays NaN where mk == 0, as 0 * NaN does there
  if (add_on) v = v + add;                                     // (:57)
  if (sub_on) v = v - sub * mk;                                // (:60)
  out[idx] = tr_nan(v) ? tr_quiet_nan() : v;                  // (one NaN, as k_tr_blur)
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned int tr_blocks(long N) { return (unsigned int)((N + EM_BLOCK - 1) / EM_BLOCK); }
static inline unsigned int tr_tiles(int M) { const int nt = (M + TT - 1) / TT; return (unsigned int)(nt * nt); }

void launch_tr_nanbit(hipStream_t s, long N, const float* in, unsigned char* bit) {
  hipLaunchKernelGGL(k_tr_nanbit, dim3(tr_blocks(N)), dim3(EM_BLOCK), 0, s, N, in, bit);
}
void launch_tr_rim(hipStream_t s, int M, const float* in, const unsigned char* bit, const int* root, int* amin) {
  hipLaunchKernelGGL(k_tr_rim, dim3(tr_blocks((long)M * M)), dim3(EM_BLOCK), 0, s, M, in, bit, root, amin);
}
void launch_tr_fill(hipStream_t s, long N, const float* in, const unsigned char* bit, const int* root, const int* amin, float* out) {
  hipLaunchKernelGGL(k_tr_fill, dim3(tr_blocks(N)), dim3(EM_BLOCK), 0, s, N, in, bit, root, amin, out);
}
void launch_tr_median(hipStream_t s, int M, int k, const float* in, float* out) {
  if (k == 3) hipLaunchKernelGGL(k_tr_median<3>, dim3(tr_tiles(M)), dim3(EM_BLOCK), 0, s, M, in, out);
  else hipLaunchKernelGGL(k_tr_median<5>, dim3(tr_tiles(M)), dim3(EM_BLOCK), 0, s, M, in, out);
}
void launch_tr_mask(hipStream_t s, long N, const float* e, const int* labels, float* w, float* m, unsigned char* bit) {
  hipLaunchKernelGGL(k_tr_mask, dim3(tr_blocks(N)), dim3(EM_BLOCK), 0, s, N, e, labels, w, m, bit);
}
void launch_tr_morph(hipStream_t s, int M, int kd, int dilate, const TerrainSpans* spans, const float* in, float* out) {
  hipLaunchKernelGGL(k_tr_morph, dim3(tr_tiles(M)), dim3(EM_BLOCK), 0, s, M, kd, dilate, spans, in, out);
}
void launch_tr_sloped(hipStream_t s, int M, int kd, const float* off, const float* in, float* out) {
  hipLaunchKernelGGL(k_tr_sloped, dim3(tr_tiles(M)), dim3(EM_BLOCK), 0, s, M, kd, off, in, out);
}
void launch_tr_blur(hipStream_t s, int M, int k, const float* taps, double scale, const float* in, float* out) {
  hipLaunchKernelGGL(k_tr_blur, dim3(tr_tiles(M)), dim3(EM_BLOCK), 0, s, M, k, taps, scale, in, out);
}
void launch_tr_lift(hipStream_t s, long N, const float* e, const float* d, const float* m, int add_on, float add, int sub_on, float sub, float* out) {
  hipLaunchKernelGGL(k_tr_lift, dim3(tr_blocks(N)), dim3(EM_BLOCK), 0, s, N, e, d, m, add_on, add, sub_on, sub, out);
}
