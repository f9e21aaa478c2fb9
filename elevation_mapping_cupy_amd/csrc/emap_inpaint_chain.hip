// Inpainting plugin, method "telea_fronts", as an op of a plugin chain (EMAP_PLUGIN_INPAINT_FRONTS, emap_api_plugchain.hip): what
// plugins/inpainting.py does around the fill on host arrays -- the range of the known heights, the 8-bit image and the mask, the
// de-quantisation -- restated bit for bit on the map's cells, so that the fronts pipeline (emap_inpaint_fronts.hip: launch_fronts) runs
// on images that never leave the device.  known = is_valid >= 0.5 (the plugin's own comparison; the other plugins test > 0.5).
// The kernels read the hot half of the cells themselves (h and is_valid come with ONE 16-byte load) instead of two k_get_plane passes
// into scratch planes: the range needs no order at all and walks the cells as they lie, the other two address the cell of a logical
// position like k_get_plane does for a full map -- lanes run along a row, a thread keeps ONE 32-bit cell offset (physical column + row
// base; a wave's cells are one or two runs of consecutive 16-byte halves) and steps it from row to row.
// The build compiles with -ffp-contract=off; the expressions whose rounding NumPy fixes are written with the round-to-nearest intrinsics
// all the same.  Heights are assumed finite in every cell (NumPy's cast of a NaN to uint8 is undefined on the host route as well).
#include "emap_launch.h"

namespace {
constexpr int IC_ROWS = 4;      // rows a workgroup of k_inp_quantise / k_inp_dequantise walks

__device__ __forceinline__ void ic_fold(InpRange& a, float lo, float hi, unsigned int known, unsigned int unknown) {
  a.lo = lo < a.lo ? lo : a.lo; a.hi = hi > a.hi ? hi : a.hi; a.known += known; a.unknown += unknown;
}
__device__ __forceinline__ void ic_block_reduce(InpRange a, InpRange* out) {
  __shared__ InpRange s[EM_BLOCK / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    ic_fold(a, __shfl_xor(a.lo, o, 64), __shfl_xor(a.hi, o, 64), (unsigned int)__shfl_xor((int)a.known, o, 64), (unsigned int)__shfl_xor((int)a.unknown, o, 64));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EM_BLOCK / 64; ++w) ic_fold(a, s[w].lo, s[w].hi, s[w].known, s[w].unknown);
    *out = a;
  }
}
// the plugin returns the elevation as it is when no cell or every cell is known
__device__ __forceinline__ bool ic_flat(const InpRange& r) { return r.known == 0u || r.unknown == 0u; }
// h_max - h_min in double, rounded to float32 where it meets the float32 image; 1 for a constant layer
__device__ __forceinline__ float ic_span(const InpRange& r) { return r.hi > r.lo ? (float)((double)r.hi - (double)r.lo) : 1.0f; }
}  // namespace

// ---- masked range: two stages, no float atomics (the pattern of k_range_parts / k_range_final, emap_plugchain.hip) -----------------------
// Comparisons on the values: right for negative heights; -0 and +0 compare equal, and which of them is kept changes no bit of what
// follows (x - lo clipped at 0, hi - lo, q * span / 255 + lo give the same floats for either zero).
__global__ __launch_bounds__(EM_BLOCK) void k_inp_range_parts(unsigned int n, const float4* __restrict__ hot, InpRange* __restrict__ parts) {
  InpRange a{INFINITY, -INFINITY, 0u, 0u};
  for (unsigned int i = blockIdx.x * EM_BLOCK + threadIdx.x; i < n; i += gridDim.x * EM_BLOCK) {
    const float4 m = hot[i];
    if (m.z >= 0.5f) ic_fold(a, m.x, m.x, 1u, 0u); else a.unknown += 1u;
  }
  ic_block_reduce(a, parts + blockIdx.x);
}
__global__ __launch_bounds__(EM_BLOCK) void k_inp_range_final(int n_parts, const InpRange* __restrict__ parts, InpRange* __restrict__ rec) {
  InpRange a{INFINITY, -INFINITY, 0u, 0u};
  for (int p = threadIdx.x; p < n_parts; p += EM_BLOCK) ic_fold(a, parts[p].lo, parts[p].hi, parts[p].known, parts[p].unknown);
  ic_block_reduce(a, rec);
}
void launch_inpaint_range(hipStream_t s, const KP& P, Cells cells, InpRange* parts, InpRange* rec) {
  const unsigned int n = (unsigned int)P.C * P.C, nb = (n + EM_BLOCK - 1) / EM_BLOCK;
  const int n_parts = (int)(nb < EM_INP_PARTS ? nb : EM_INP_PARTS);
  hipLaunchKernelGGL(k_inp_range_parts, dim3(n_parts), dim3(EM_BLOCK), 0, s, n, cells.hot, parts);
  hipLaunchKernelGGL(k_inp_range_final, dim3(1), dim3(EM_BLOCK), 0, s, n_parts, parts, rec);
}

// ---- quantise + mask: np.clip((h - h_min) * 255 / span, 0, 255).astype(uint8) and ~known, one pass over the cells ---------------------------
// A flat map (ic_flat) gets an all-known mask: the fronts pipeline then finds nothing to fill and k_inp_dequantise copies the elevation.
__global__ __launch_bounds__(EM_BLOCK) void k_inp_quantise(int C, int org_r, int org_c, const float4* __restrict__ hot, const InpRange* __restrict__ rec,
                                                           unsigned char* __restrict__ q8, unsigned char* __restrict__ mask) {
  const int c = blockIdx.x * EM_BLOCK + threadIdx.x, r0 = blockIdx.y * IC_ROWS;
  if (c >= C) return;
  const InpRange R = *rec;
  const bool flat = ic_flat(R);
  const float span = ic_span(R);
  int pr = r0 + org_r; pr = pr >= C ? pr - C : pr;
  const int pc = c + org_c;
  unsigned int ci = (unsigned int)pr * C + (pc >= C ? pc - C : pc), li = (unsigned int)r0 * C + c;
#pragma unroll
  for (int u = 0; u < IC_ROWS; ++u) {
    if (r0 + u >= C) break;
    const float4 m = hot[ci];
    float v = __fdiv_rn(__fmul_rn(__fsub_rn(m.x, R.lo), 255.0f), span);
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    q8[li] = flat ? (unsigned char)0 : (unsigned char)__float2int_rz(v);
    mask[li] = (flat || m.z >= 0.5f) ? (unsigned char)0 : (unsigned char)1;
    li += C; ci += C; ++pr;
    if (pr == C) { pr = 0; ci -= (unsigned int)C * C; }
  }
}
// row of the cell array that holds logical row 0 of a full map (view_cell: local_row of phys_row, no halo)
static int ic_row_origin(const KP& P) { return ((P.org_r - P.row0) % P.C + P.C) % P.C; }
void launch_inpaint_quantise(hipStream_t s, const KP& P, Cells cells, const InpRange* rec, unsigned char* q8, unsigned char* mask) {
  hipLaunchKernelGGL(k_inp_quantise, dim3((P.C + EM_BLOCK - 1) / EM_BLOCK, (P.C + IC_ROWS - 1) / IC_ROWS), dim3(EM_BLOCK), 0, s, P.C, ic_row_origin(P), P.org_c,
                     cells.hot, rec, q8, mask);
}

// ---- de-quantise: (float)out8 * span / 255 + h_min, three roundings; the elevation itself for a flat map ------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_inp_dequantise(int C, int org_r, int org_c, const float4* __restrict__ hot, const InpRange* __restrict__ rec,
                                                             const unsigned char* __restrict__ out8, float* __restrict__ dst) {
  const int c = blockIdx.x * EM_BLOCK + threadIdx.x, r0 = blockIdx.y * IC_ROWS;
  if (c >= C) return;
  const InpRange R = *rec;
  const float span = ic_span(R);
  unsigned int li = (unsigned int)r0 * C + c;
  if (!ic_flat(R)) {
#pragma unroll
    for (int u = 0; u < IC_ROWS; ++u) {
      if (r0 + u >= C) break;
      dst[li] = __fadd_rn(__fdiv_rn(__fmul_rn((float)out8[li], span), 255.0f), R.lo);
      li += C;
    }
    return;
  }
  int pr = r0 + org_r; pr = pr >= C ? pr - C : pr;
  const int pc = c + org_c;
  unsigned int ci = (unsigned int)pr * C + (pc >= C ? pc - C : pc);
#pragma unroll
  for (int u = 0; u < IC_ROWS; ++u) {
    if (r0 + u >= C) break;
    dst[li] = hot[ci].x;
    li += C; ci += C; ++pr;
    if (pr == C) { pr = 0; ci -= (unsigned int)C * C; }
  }
}
void launch_inpaint_dequantise(hipStream_t s, const KP& P, Cells cells, const InpRange* rec, const unsigned char* out8, float* dst) {
  hipLaunchKernelGGL(k_inp_dequantise, dim3((P.C + EM_BLOCK - 1) / EM_BLOCK, (P.C + IC_ROWS - 1) / IC_ROWS), dim3(EM_BLOCK), 0, s, P.C, ic_row_origin(P), P.org_c,
                     cells.hot, rec, out8, dst);
}
