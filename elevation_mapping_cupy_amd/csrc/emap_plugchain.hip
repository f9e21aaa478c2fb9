// Publish-time plugins on device-resident planes (gfx950): the kernels a plugin chain (emap_api_plugchain.hip: emap_plugin_chain) adds to
// the sweeps, the erosion and the plane reads that emap_semantic.hip / emap_kernels.hip already hold.  Every kernel restates, bit for
// bit, a step the host route of the plugin takes on host arrays (plugins/*.py, emap_api_plugins.hip); the planes are (C, C) floats in
// logical row-major order.  The build compiles with -ffp-contract=off; the expressions whose rounding NumPy fixes are written with the
// round-to-nearest intrinsics all the same, so that no flag can fuse them.
#include "emap_launch.h"

// ---- MinFilter / MaxFilter, last step (EM/plugins/min_filter.py:116): cp.where(mask > 0.5, filtered, nan) -----------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_mask_nan(long n, const float* __restrict__ val, const float* __restrict__ msk, float* __restrict__ out) {
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = msk[i] > 0.5f ? val[i] : __uint_as_float(0x7fc00000u);
}
void launch_mask_nan(hipStream_t s, long n, const float* val, const float* msk, float* out) {
  hipLaunchKernelGGL(k_mask_nan, dim3((unsigned int)((n + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, n, val, msk, out);
}

// ---- SmoothFilter (EM/plugins/smooth_filter.py:56-58): both uniform_filter(size=3) passes from one launch ------------------------------
// One pass is k_box3 (emap_semantic.hip): per output the three column sums of the 3 x 3 window in double, each divided by 3.0 and rounded
// to float32 (the axis-0 pass of scipy), their sum in double divided by 3.0 and rounded; 'reflect' borders = indices clamped to the map.
// A workgroup owns SM_R x SM_C outputs.  The input lands in LDS with a halo of 2, pass 1 is evaluated on the tile with a halo of 1 into
// a second LDS tile as float32, pass 2 reads it there.  A clamped index of a cell of the map is a cell of the map inside the same halo,
// so LDS positions outside the map are never read; lanes run along a row, so every LDS access of a wave is 64 consecutive words (no
// bank conflict at any pitch) and every store a run of 256 bytes.
#define SM_R 16
#define SM_C 64
__device__ __forceinline__ int sm_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// k_box3 of the cell (r, c) of the map on an LDS tile whose element (0, 0) is the map's cell (r_org, c_org)
__device__ __forceinline__ float sm_box3(const float* t, int pitch, int r_org, int c_org, int r, int c, int C) {
  const int rows[3] = {sm_clamp(r - 1, C) - r_org, r - r_org, sm_clamp(r + 1, C) - r_org};
  const int cols[3] = {sm_clamp(c - 1, C) - c_org, c - c_org, sm_clamp(c + 1, C) - c_org};
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    double col = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) col += (double)t[rows[a] * pitch + cols[b]];
    acc += (double)(float)(col / 3.0);
  }
  return (float)(acc / 3.0);
}
__global__ __launch_bounds__(EM_BLOCK) void k_smooth2(int C, const float* __restrict__ in, float* __restrict__ out) {
  constexpr int H0 = SM_R + 4, W0 = SM_C + 4, P0 = W0 + 1, H1 = SM_R + 2, W1 = SM_C + 2, P1 = W1 + 1;
  __shared__ float s_in[H0 * P0];
  __shared__ float s_p1[H1 * P1];
  const int tr = blockIdx.y * SM_R, tc = blockIdx.x * SM_C;
  for (int e = threadIdx.x; e < H0 * W0; e += EM_BLOCK) {
    const int lr = e / W0, lc = e % W0, r = tr - 2 + lr, c = tc - 2 + lc;
    s_in[lr * P0 + lc] = (r >= 0 && r < C && c >= 0 && c < C) ? in[(long)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < H1 * W1; e += EM_BLOCK) {
    const int lr = e / W1, lc = e % W1, r = tr - 1 + lr, c = tc - 1 + lc;
    s_p1[lr * P1 + lc] = (r >= 0 && r < C && c >= 0 && c < C) ? sm_box3(s_in, P0, tr - 2, tc - 2, r, c, C) : 0.f;
  }
  __syncthreads();
  const int lc = threadIdx.x & (SM_C - 1), c = tc + lc;
  if (c >= C) return;
  for (int lr = threadIdx.x / SM_C; lr < SM_R; lr += EM_BLOCK / SM_C) {
    const int r = tr + lr;
    if (r >= C) break;
    out[(long)r * C + c] = sm_box3(s_p1, P1, tr - 1, tc - 1, r, c, C);
  }
}
void launch_smooth2(hipStream_t s, int C, const float* in, float* out) {
  hipLaunchKernelGGL(k_smooth2, dim3((C + SM_C - 1) / SM_C, (C + SM_R - 1) / SM_R), dim3(EM_BLOCK), 0, s, C, in, out);
}

// ---- Erosion (EM/plugins/erosion.py:96-104) around k_erode ---------------------------------------------------------------------------------
// The plugin takes lo = layer.min(), hi = layer.max() of the (reversed) layer on the host.  Here: two stages, no float atomics.  Stage 1
// leaves one (lo, hi, has-NaN) triple per workgroup, stage 2 (one workgroup) folds them into red[0 .. 2].  The minimum and maximum are
// taken with comparisons on the values (right for negative values; -0 and +0 compare equal, and which of them is kept changes no bit of
// what follows: x - lo, hi - lo, q * span / 255 + lo give the same floats for either zero); a NaN is recorded in the flag, as np.min
// would return it.
#define ER_PARTS 256
__device__ __forceinline__ float er_value(float x, int reverse) { return reverse ? __fsub_rn(1.0f, x) : x; }
__device__ __forceinline__ void er_fold(float& lo, float& hi, unsigned int& nan, float olo, float ohi, unsigned int onan) {
  lo = olo < lo ? olo : lo; hi = ohi > hi ? ohi : hi; nan |= onan;
}
__device__ __forceinline__ void er_block_reduce(float lo, float hi, unsigned int nan, float* red) {
  __shared__ float s_lo[EM_BLOCK / 64], s_hi[EM_BLOCK / 64];
  __shared__ unsigned int s_nan[EM_BLOCK / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) er_fold(lo, hi, nan, __shfl_xor(lo, o, 64), __shfl_xor(hi, o, 64), (unsigned int)__shfl_xor((int)nan, o, 64));
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; s_nan[threadIdx.x >> 6] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EM_BLOCK / 64; ++w) er_fold(lo, hi, nan, s_lo[w], s_hi[w], s_nan[w]);
    red[0] = lo; red[1] = hi; red[2] = __uint_as_float(nan);
  }
}
__global__ __launch_bounds__(EM_BLOCK) void k_range_parts(long n, const float* __restrict__ in, int reverse, float* __restrict__ parts) {
  float lo = INFINITY, hi = -INFINITY; unsigned int nan = 0u;
  for (long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * EM_BLOCK) {
    const float x = er_value(in[i], reverse);
    if (x != x) nan = 1u; else er_fold(lo, hi, nan, x, x, 0u);
  }
  er_block_reduce(lo, hi, nan, parts + 3 * blockIdx.x);
}
__global__ __launch_bounds__(EM_BLOCK) void k_range_final(int n_parts, const float* __restrict__ parts, float* __restrict__ red) {
  float lo = INFINITY, hi = -INFINITY; unsigned int nan = 0u;
  for (int p = threadIdx.x; p < n_parts; p += EM_BLOCK) er_fold(lo, hi, nan, parts[3 * p], parts[3 * p + 1], __float_as_uint(parts[3 * p + 2]));
  er_block_reduce(lo, hi, nan, red);
}
void launch_range(hipStream_t s, long n, const float* in, int reverse, float* parts, float* red) {
  long nb = (n + EM_BLOCK - 1) / EM_BLOCK;
  const int n_parts = (int)(nb < ER_PARTS ? nb : ER_PARTS);
  hipLaunchKernelGGL(k_range_parts, dim3(n_parts), dim3(EM_BLOCK), 0, s, n, in, reverse, parts);
  hipLaunchKernelGGL(k_range_final, dim3(1), dim3(EM_BLOCK), 0, s, n_parts, parts, red);
}
__device__ __forceinline__ bool er_flat(const float* red) { return __float_as_uint(red[2]) != 0u || !(red[1] > red[0]); }
// ((layer - lo) * 255 / (hi - lo)).astype("uint8") in float32: the divisor is the float of the double difference, the cast truncates
__global__ __launch_bounds__(EM_BLOCK) void k_quantise(long n, const float* __restrict__ in, int reverse, const float* __restrict__ red, float* __restrict__ q) {
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (er_flat(red)) { q[i] = 0.f; return; }              // (the flat rule: nothing downstream reads q)
  const float lo = red[0], span = (float)((double)red[1] - (double)lo);
  const float v = __fdiv_rn(__fmul_rn(__fsub_rn(er_value(in[i], reverse), lo), 255.0f), span);
  q[i] = (float)(unsigned char)__float2int_rz(v);
}
// q * (hi - lo) / 255 + lo, three roundings, then 1 - x under reverse; a flat layer (or one that holds a NaN) is returned as it came
// (under reverse as 1 - (1 - x): erosion.py reverses first and un-reverses what it returns)
__global__ __launch_bounds__(EM_BLOCK) void k_dequantise(long n, const float* __restrict__ q, const float* in, int reverse,
                                                          const float* __restrict__ red, float* out) {      // (in may be out)
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (er_flat(red)) { out[i] = reverse ? __fsub_rn(1.0f, __fsub_rn(1.0f, in[i])) : in[i]; return; }      // the plugin un-reverses what it reversed: two roundings
  const float lo = red[0], span = (float)((double)red[1] - (double)lo);
  const float v = __fadd_rn(__fdiv_rn(__fmul_rn(q[i], span), 255.0f), lo);
  out[i] = reverse ? __fsub_rn(1.0f, v) : v;
}
void launch_quantise(hipStream_t s, long n, const float* in, int reverse, const float* red, float* q) {
  hipLaunchKernelGGL(k_quantise, dim3((unsigned int)((n + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, n, in, reverse, red, q);
}
void launch_dequantise(hipStream_t s, long n, const float* q, const float* in, int reverse, const float* red, float* out) {
  hipLaunchKernelGGL(k_dequantise, dim3((unsigned int)((n + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, n, q, in, reverse, red, out);
}

// ---- RobotCentricElevation (EM/plugins/robot_centric_elevation.py:54-57, :96-118) ---------------------------------------------------------
// z_b = (R6 rx + R7 ry) + R8 h with rx = (float)row * (float)resolution, every product and sum rounded on its own; valid cells take z_b
// (or z_b >= threshold as 1 / 0), the others keep h.
__global__ __launch_bounds__(EM_BLOCK) void k_robot_centric(int C, float res, float r6, float r7, float r8, int use_threshold, float threshold,
                                                             const float* __restrict__ h, const float* __restrict__ valid, float* __restrict__ out) {
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= (long)C * C) return;
  const int r = (int)(i / C), c = (int)(i % C);
  const float hv = h[i];
  const float rx = __fmul_rn((float)r, res), ry = __fmul_rn((float)c, res);
  const float zb = __fadd_rn(__fadd_rn(__fmul_rn(r6, rx), __fmul_rn(r7, ry)), __fmul_rn(r8, hv));
  float o = hv;
  if (valid[i] > 0.5f) o = use_threshold ? (zb >= threshold ? 1.0f : 0.0f) : zb;
  out[i] = o;
}
void launch_robot_centric(hipStream_t s, int C, float res, const float* R9, int use_threshold, float threshold, const float* h, const float* valid, float* out) {
  hipLaunchKernelGGL(k_robot_centric, dim3((unsigned int)(((long)C * C + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, C, res, R9[6], R9[7], R9[8],
                     use_threshold, threshold, h, valid, out);
}

// ---- the plugins that read several layers: one thread per logical cell, every source read once, one store ---------------------------------
// The table of sources travels in the kernel's arguments, so the walk over it is uniform and nothing is staged in scratch planes.  The
// plugins run under NumPy 2 (NEP 50): a Python float beside a float32 array keeps the operation in float32, a NumPy float64 scalar
// widens it to double -- which of the two each step is, is written at the step.
__device__ __forceinline__ bool plug_cell(const KP& P, long& li, long& ci) {
  li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.C * P.C) return false;
  const int r = (int)(li / P.C), c = (int)(li - (long)r * P.C);
  ci = owned_cell(P, r, c);      // (a full map owns every row)
  return ci >= 0;
}
static unsigned int plug_grid(const KP& P) { return (unsigned int)(((long)P.C * P.C + EM_BLOCK - 1) / EM_BLOCK); }

// SemanticFilter (EM/plugins/semantic_filter.py:128, :132): np.argmax over the sources -- the first NaN wins, otherwise the first maximum
// (a later value replaces the best only when it is GREATER, so -0 and +0 tie) -- then entry id + 1 of the colour table (:42-62), dealt
// from the bits of the index here: bit 3 j + ch -> bit 7 - j of channel ch; entries 1, 2 and 3 are the reference's overrides.
__device__ __forceinline__ unsigned int sem_filter_colour(unsigned int i) {
  unsigned int r = 0u, g = 0u, b = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    r |= ((i >> (3 * j)) & 1u) << (7 - j); g |= ((i >> (3 * j + 1)) & 1u) << (7 - j); b |= ((i >> (3 * j + 2)) & 1u) << (7 - j);
  }
  if (i == 1u || i == 2u) { r = 81u; g = 113u; b = 162u; }
  if (i == 3u) { r = 188u; g = 63u; b = 59u; }
  return (r << 16) | (g << 8) | b;
}
__global__ __launch_bounds__(EM_BLOCK) void k_semantic_filter(KP P, Cells cells, PlugSrcs S, float* __restrict__ dst) {
  long li, ci;
  if (!plug_cell(P, li, ci)) return;
  const long L = (long)P.C * P.C;
  int best = 0; float bv = 0.f; bool nan = false;
  for (int k = 0; k < S.n; ++k) {
    const float v = plug_src_read(S, k, cells, L, li, ci);
    if (k == 0) { bv = v; nan = v != v; }
    else if (!nan) {
      if (v != v) { best = k; nan = true; } else if (v > bv) { best = k; bv = v; }
    }
  }
  dst[li] = __uint_as_float(sem_filter_colour((unsigned int)best + 1u));
}
void launch_semantic_filter(hipStream_t s, const KP& P, Cells cells, const PlugSrcs& S, float* dst) {
  hipLaunchKernelGGL(k_semantic_filter, dim3(plug_grid(P)), dim3(EM_BLOCK), 0, s, P, cells, S, dst);
}

// SemanticTraversability (EM/plugins/semantic_traversability.py:70-82): the plugin keeps its thresholds as np.float64 scalars, so
// layer <= thresholds[it] compares in DOUBLE (0.3f <= 0.3 is false: the float is the larger); a NaN compares false both ways.  The
// vote sum is a small integer, so `votes <= 0.9` is "nobody voted"; np.where(..., 0.1, 1.0) is float64 and the manager's cast to
// float32 makes it 0.1f.
__global__ __launch_bounds__(EM_BLOCK) void k_semantic_trav(KP P, Cells cells, PlugSrcs S, PlugPars R, float* __restrict__ dst) {
  long li, ci;
  if (!plug_cell(P, li, ci)) return;
  const long L = (long)P.C * P.C;
  bool any = false;
  for (int k = 0; k < S.n; ++k) {
    const double x = (double)plug_src_read(S, k, cells, L, li, ci);
    any |= (R.flags[k] & 1) ? x <= R.d0[k] : x >= R.d0[k];      // (1: EMAP_PLUGIN_SRC_AT_MOST)
  }
  dst[li] = any ? 1.0f : 0.1f;
}
void launch_semantic_trav(hipStream_t s, const KP& P, Cells cells, const PlugSrcs& S, const PlugPars& R, float* dst) {
  hipLaunchKernelGGL(k_semantic_trav, dim3(plug_grid(P)), dim3(EM_BLOCK), 0, s, P, cells, S, R, dst);
}

// MaxLayerFilter (EM/plugins/max_layer_filter.py:66-108).  Every step of a layer stays float32: np.where(layer == 0.0, float(d), layer),
// 1.0 - layer, layer * float(s) and layer > float(t) all meet a Python float.  The thresholded layers are int64 and np.stack widens a
// mixed stack to float64, but 0 / 1 and a float32 are exact there and the manager casts the result back, so the reduction runs in float32
// on the same values.  np.max / np.min along the first axis of the stack: acc = acc > x ? acc : x (acc < x for the minimum) in stack
// order -- of two equal values the LATER one is kept, which is what the sign of a zero shows -- and any NaN makes the result NaN.
__global__ __launch_bounds__(EM_BLOCK) void k_max_layer(KP P, Cells cells, PlugSrcs S, PlugPars R, int take_min, float* __restrict__ dst) {
  long li, ci;
  if (!plug_cell(P, li, ci)) return;
  const long L = (long)P.C * P.C;
  float acc = 0.f; bool nan = false;
  for (int k = 0; k < S.n; ++k) {
    float x = plug_src_read(S, k, cells, L, li, ci);
    const int fl = R.flags[k];
    if ((fl & 2) && x == 0.0f) x = R.f0[k];                       // EMAP_PLUGIN_SRC_ZERO_DEFAULT (:75)
    if (fl & 4) x = __fsub_rn(1.0f, x);                           // EMAP_PLUGIN_SRC_REVERSE (:88)
    if (fl & 8) x = __fmul_rn(x, R.f1[k]);                        // EMAP_PLUGIN_SRC_SCALE (:90)
    if (fl & 16) x = x > (float)R.d0[k] ? 1.0f : 0.0f;            // EMAP_PLUGIN_SRC_THRESHOLD (:92)
    nan |= x != x;
    if (k == 0) acc = x; else acc = take_min ? (acc < x ? acc : x) : (acc > x ? acc : x);
  }
  dst[li] = nan ? __uint_as_float(0x7fc00000u) : acc;
}
void launch_max_layer(hipStream_t s, const KP& P, Cells cells, const PlugSrcs& S, const PlugPars& R, int take_min, float* dst) {
  hipLaunchKernelGGL(k_max_layer, dim3(plug_grid(P)), dim3(EM_BLOCK), 0, s, P, cells, S, R, take_min, dst);
}
