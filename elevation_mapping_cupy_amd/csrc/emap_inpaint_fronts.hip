// Inpainting plugin, method "telea_fronts": Telea's estimator (the arithmetic of telea() in emap_inpaint_host.hip, radius 1) on the
// MI355X, scheduled by fronts instead of by a serial priority queue.  Contract (include/emap_hip.h):
//   d(p) = L1 distance from p to the nearest pixel with mask == 0 (0 for known pixels, k for front k);
//   fronts k = 1 .. max d run in order, every pixel of front k at once; "not INSIDE" in the host arithmetic means d(q) < k (the
//   1-pixel frame outside the image counts as known); pixels with d >= k read as T = 1e6 and hold their input value; a known pixel
//   4-adjacent to the hole starts at T = -0.0f (the host's empty outside march with radius 1), every other known pixel at 1e6.
// The pipeline runs on images that are on the device (launch_fronts, emap_launch.h: the core an op of a plugin chain enqueues with the
// geometric bound of max d as its launch count); emap_inpaint_telea_fronts_u8 is the host door around it: uploads, the
// 4-byte read-back of max d, ceil(max d / S) launches, the download.
// Pipeline per call, one stream, no grid-wide barrier:
//   k_fr_dt_cols_local, k_fr_dt_cols_carry   exact separable L1 distance transform, column pass: two sweeps per (column, block of 32
//                  rows), then the carries of the blocks above and below
//   k_fr_dt_rows   row pass (one wave per row: min-plus over |dj| as a prefix / suffix minimum of g -+ j)
//   k_fr_init      per tile: initial T, output = input, min / max d of the tile, max d of the image (one 4-byte read-back)
//   k_fr_advance   ceil(max d / S) launches; a workgroup loads its tile plus a halo of 2 S pixels into LDS (T f32, value u8,
//                  input value u8, d - k0 clamped to u8), advances S fronts with a barrier between them, writes back the interior.
//                  A pixel of front k reads pixels of earlier fronts within Chebyshev distance 2 (its 4-neighbours, and their
//                  neighbours through the image-gradient term), so the valid region shrinks by 2 per front: 2 S of halo suffice.
//                  Halo pixels another workgroup writes in the same launch have d > k0 and are read as (1e6, input value), which is
//                  what they held before the launch: no race decides a result.
#include "../../include/emap_hip.h"
#include "emap_launch.h"
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include <cstring>

namespace {
constexpr int FW = 94;                 // LDS tile side: interior FW - 4 S plus a halo of 2 S on each side; 7 bytes a pixel -> 61.9 KB,
                                       // the largest side under 64 KB of LDS per workgroup
constexpr int FN = FW * FW;
constexpr int FB = 256;                // threads per workgroup of every kernel here
constexpr int FINF = 1 << 29;          // "no known pixel" distance
constexpr int S_MAX = EM_FRONTS_S_MAX;  // fronts per launch: interior FW - 4 S >= 30
constexpr int S_DEFAULT = 16;          // measured (tools/exp_inpaint_fronts.py): the fastest S at 202^2, within 4 % at 1024^2

// Lanes of one wave hand cell indices to each other through LDS: a wave-scope release / acquire pair around the wave barrier orders the
// LDS writes before the reads of the other lanes (and the reads before the overwrite that follows them).
__device__ __forceinline__ void fr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline float fr_min4(float a, float b, float c, float d) { a = a < b ? a : b; c = c < d ? c : d; return a < c ? a : c; }

// ---- distance transform ---------------------------------------------------------------------------------------------------------
// Column pass in row blocks of DTB rows, one thread per (column, block): g(i, j) = distance along column j to the nearest known pixel, FINF
// without one.  k_fr_dt_cols_local runs the two sweeps inside its block (the recurrence in registers, all loads issued together) and leaves
// the block's summary: top = distance from the block's first row DOWN to its first known pixel, bot = from its last row UP to its last
// known pixel (FINF: none).  k_fr_dt_cols_carry walks the summaries of the blocks above and below to the nearest one that holds a known
// pixel -- every block but the last is full, so that pixel lies (blocks between) * DTB + 1 + bot (or top) rows beyond the block's edge --
// and lowers its block's values by the two carries.  The result is the integer the one-thread-per-column sweeps gave.
constexpr int DTB = 32;
__global__ __launch_bounds__(FB) void k_fr_dt_cols_local(const uint8_t* __restrict__ mask, int32_t* __restrict__ g, int32_t* __restrict__ top,
                                                         int32_t* __restrict__ bot, int rows, int cols) {
  const int j = blockIdx.x * FB + threadIdx.x, i0 = blockIdx.y * DTB;
  if (j >= cols) return;
  const int n = rows - i0 < DTB ? rows - i0 : DTB;
  const size_t p0 = (size_t)i0 * cols + j;
  uint8_t m[DTB]; int32_t f[DTB];
#pragma unroll
  for (int u = 0; u < DTB; ++u) m[u] = u < n ? mask[p0 + (size_t)u * cols] : 1;      // rows beyond the image: never known
  int h = FINF, first = FINF, last = FINF;
#pragma unroll
  for (int u = 0; u < DTB; ++u) {
    h = m[u] ? (h >= FINF ? FINF : h + 1) : 0;
    f[u] = h;
    if (!m[u]) { first = first < FINF ? first : u; last = n - 1 - u; }
  }
  h = FINF;
#pragma unroll
  for (int u = DTB - 1; u >= 0; --u) {
    h = m[u] ? (h >= FINF ? FINF : h + 1) : 0;
    if (u < n) g[p0 + (size_t)u * cols] = f[u] < h ? f[u] : h;
  }
  top[(size_t)blockIdx.y * cols + j] = first;
  bot[(size_t)blockIdx.y * cols + j] = last;
}
__global__ __launch_bounds__(FB) void k_fr_dt_cols_carry(int32_t* __restrict__ g, const int32_t* __restrict__ top, const int32_t* __restrict__ bot,
                                                         int rows, int cols, int nb) {
  const int j = blockIdx.x * FB + threadIdx.x, b = blockIdx.y, i0 = b * DTB;
  if (j >= cols) return;
  const int n = rows - i0 < DTB ? rows - i0 : DTB;
  int cu = FINF, cd = FINF;      // from the block's first row up / from its last row down to the nearest known pixel outside the block
  for (int q = b - 1; q >= 0; --q) { const int t = bot[(size_t)q * cols + j]; if (t < FINF) { cu = (b - q - 1) * DTB + 1 + t; break; } }
  for (int q = b + 1; q < nb; ++q) { const int t = top[(size_t)q * cols + j]; if (t < FINF) { cd = (q - b - 1) * DTB + 1 + t; break; } }
  if (cu >= FINF && cd >= FINF) return;
  const size_t p0 = (size_t)i0 * cols + j;
  int32_t v[DTB];
#pragma unroll
  for (int u = 0; u < DTB; ++u) v[u] = u < n ? g[p0 + (size_t)u * cols] : 0;
#pragma unroll
  for (int u = 0; u < DTB; ++u) {
    if (u >= n) break;
    int x = v[u];
    if (cu < FINF) x = cu + u < x ? cu + u : x;
    if (cd < FINF) x = cd + (n - 1 - u) < x ? cd + (n - 1 - u) : x;
    g[p0 + (size_t)u * cols] = x;
  }
}

// d(i, j) = min_j' g(i, j') + |j - j'| = min(j + min_{j' <= j}(g - j'), min_{j' >= j}(g + j') - j)
__global__ __launch_bounds__(FB) void k_fr_dt_rows(const int32_t* __restrict__ g, int32_t* __restrict__ d, int rows, int cols) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * (FB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                                   // (whole waves: the shuffles below see full waves)
  const int32_t* gr = g + (size_t)row * cols;
  int32_t* dr = d + (size_t)row * cols;
  int carry = INT_MAX;
  for (int b = 0; b < cols; b += 64) {
    const int j = b + lane;
    int x = j < cols ? gr[j] - j : INT_MAX;
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x = x < y ? x : y; }
    x = x < carry ? x : carry;
    carry = __shfl(x, 63, 64);
    if (j < cols) dr[j] = x + j;
  }
  carry = INT_MAX;
  for (int b = (cols - 1) & ~63; b >= 0; b -= 64) {
    const int j = b + lane;
    int x = j < cols ? gr[j] + j : INT_MAX;
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_down(x, o, 64); if (lane + o < 64) x = x < y ? x : y; }
    x = x < carry ? x : carry;
    carry = __shfl(x, 0, 64);
    if (j < cols) { const int f = dr[j], v = x - j, m = f < v ? f : v; dr[j] = m < FINF ? m : FINF; }
  }
}

// ---- per tile: initial state, tile min / max of d, image max of d ------------------------------------------------------------------
__global__ __launch_bounds__(FB) void k_fr_init(const uint8_t* __restrict__ in, const uint8_t* __restrict__ mask, const int32_t* __restrict__ d,
                                                float* __restrict__ T, uint8_t* __restrict__ out, int2* __restrict__ tile_mm,
                                                int* __restrict__ dmax, int rows, int cols, int tw, int ntx) {
  const int ti = blockIdx.x / ntx, tj = blockIdx.x % ntx;
  int lo = INT_MAX, hi = 0;
  for (int q = threadIdx.x; q < tw * tw; q += FB) {
    const int i = ti * tw + q / tw, j = tj * tw + q % tw;
    if (i >= rows || j >= cols) continue;
    const size_t p = (size_t)i * cols + j;
    const int dd = d[p];
    lo = dd < lo ? dd : lo; hi = dd > hi ? dd : hi;
    const bool band = !mask[p] && ((i > 0 && mask[p - cols]) || (j > 0 && mask[p - 1]) || (j + 1 < cols && mask[p + 1]) || (i + 1 < rows && mask[p + cols]));
    T[p] = band ? -0.0f : 1.0e6f;
    out[p] = in[p];
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo; hi = b > hi ? b : hi;
  }
  __shared__ int slo[FB / 64], shi[FB / 64];
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FB / 64; ++w) { lo = slo[w] < lo ? slo[w] : lo; hi = shi[w] > hi ? shi[w] : hi; }
    tile_mm[blockIdx.x] = make_int2(lo, hi);
    atomicMax(dmax, hi);
  }
}

// ---- S fronts per launch in LDS ---------------------------------------------------------------------------------------------------
struct FrontTile {
  float t[FN];                         // T; pixels of later fronts and outside the image hold 1e6
  uint8_t cur[FN];                     // value: computed for d <= k0 + s - 1, the input value otherwise
  uint8_t org[FN];                     // input value (what a pixel of the current or a later front reads as)
  uint8_t dl[FN];                      // min(max(d - k0, 0), S + 1); 0 outside the image (the frame counts as known)
};

// One pixel of front k0 + s at local (r, c), image (i, j): telea() of emap_inpaint_host.hip with radius 1, same float32 operations.
// Every LDS read is issued before the branches that select among them (they are independent: the reads overlap instead of forming a
// chain).  Cells outside the image hold dl = 0 and t = 1e6 in LDS, i.e. they read as the host's frame: known, T = 1e6.
__device__ __forceinline__ void fr_pixel(const FrontTile& L, int r, int c, int i, int j, int rows, int cols, int oi, int oj, int s,
                                         float& Tout, uint8_t& Vout) {
  const int x0 = r * FW + c;
  const int U = x0 - FW, D = x0 + FW, Lf = x0 - 1, Rt = x0 + 1;
  const bool kU = L.dl[U] < s, kD = L.dl[D] < s, kL = L.dl[Lf] < s, kR = L.dl[Rt] < s;
  const float tU = kU ? L.t[U] : 1.0e6f, tD = kD ? L.t[D] : 1.0e6f, tL = kL ? L.t[Lf] : 1.0e6f, tR = kR ? L.t[Rt] : 1.0e6f;
  auto solve = [](float a11, bool k1, float a22, bool k2) -> float {
    const float m12 = a11 < a22 ? a11 : a22;
    if (k1) {
      if (k2) return fabsf(a11 - a22) >= 1.0f ? 1.0f + m12 : (a11 + a22 + __fsqrt_rn(2.0f - (a11 - a22) * (a11 - a22))) * 0.5f;
      return 1.0f + a11;
    }
    if (k2) return 1.0f + a22;
    return 1.0f + m12;
  };
  const float dist = fr_min4(solve(tU, kU, tL, kL), solve(tD, kD, tL, kL), solve(tU, kU, tR, kR), solve(tD, kD, tR, kR));
  float gx, gy;
  if (kR) gx = kL ? (tR - tL) * 0.5f : tR - dist;
  else gx = kL ? dist - tL : 0.0f;
  if (kD) gy = kU ? (tD - tU) * 0.5f : tD - dist;
  else gy = kU ? dist - tU : 0.0f;
  auto ov = [&](int x, int y) -> float {         // value at IMAGE position (x, y) (always inside the image)
    const int q = (x - oi) * FW + (y - oj);
    return (float)(L.dl[q] < s ? L.cur[q] : L.org[q]);
  };
  float Ia = 0.f, Jx = 0.f, Jy = 0.f, sw = 1.0e-20f;
  const int na[4] = {-1, 0, 0, 1}, nb[4] = {0, -1, 1, 0};       // the radius-1 window in the host's row-major order
  const bool kn4[4] = {kU, kL, kR, kD};
  const float tn4[4] = {tU, tL, tR, tD};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int a = na[n], b = nb[n], k = i + a, l = j + b;
    if (k < 0 || l < 0 || k >= rows || l >= cols || !kn4[n]) continue;
    const int km = k + (k == 0), kp = k - (k == rows - 1), lm = l + (l == 0), lp = l - (l == cols - 1);
    const int xn = x0 + a * FW + b;
    const bool kxp = L.dl[xn + 1] < s, kxm = L.dl[xn - 1] < s, kyp = L.dl[xn + FW] < s, kym = L.dl[xn - FW] < s;
    const float o_c = ov(km, lm), o_xp1 = ov(km, lp + 1), o_xm1 = ov(km, lm - 1), o_xp = ov(km, lp);
    const float o_yp1 = ov(kp + 1, lm), o_ym1 = ov(km - 1, lm), o_yp = ov(kp, lm);
    const float ry = (float)(-a), rx = (float)(-b), len2 = rx * rx + ry * ry;
    const float dst = __fdiv_rn(1.0f, len2 * __fsqrt_rn(len2));
    const float lev = __fdiv_rn(1.0f, 1.0f + fabsf(tn4[n] - dist));
    float dir = rx * gx + ry * gy;
    if (fabsf(dir) <= 0.01f) dir = 0.000001f;
    const float w = fabsf(dst * lev * dir);
    float gIx, gIy;
    if (kxp) gIx = kxm ? (o_xp1 - o_xm1) * 2.0f : o_xp1 - o_c;
    else gIx = kxm ? o_xp - o_xm1 : 0.0f;
    if (kyp) gIy = kym ? (o_yp1 - o_ym1) * 2.0f : o_yp1 - o_c;
    else gIy = kym ? o_yp - o_ym1 : 0.0f;
    Ia += w * o_c;
    Jx -= w * gIx * rx;
    Jy -= w * gIy * ry;
    sw += w;
  }
  const float sat = __fdiv_rn(Ia, sw) + __fdiv_rn(Jx + Jy, __fsqrt_rn(Jx * Jx + Jy * Jy) + 1.0e-20f);
  const float rr = __builtin_rintf(sat);                           // lrintf: nearest, ties to even
  Tout = dist;
  Vout = (uint8_t)(rr < 0.0f ? 0 : (rr > 255.0f ? 255 : (int)rr));
}

__global__ __launch_bounds__(FB) void k_fr_advance(const uint8_t* __restrict__ in, const int32_t* __restrict__ d, float* __restrict__ T,
                                                   uint8_t* __restrict__ out, const int2* __restrict__ tile_mm, int rows, int cols,
                                                   int ntx, int S, int k0) {
  const int2 mm = tile_mm[blockIdx.x];
  if (mm.y <= k0 || mm.x > k0 + S) return;                     // no pixel of fronts k0 + 1 .. k0 + S in this tile
  __shared__ FrontTile L;
  __shared__ uint16_t work[FB / 64][64];                         // per wave: cells of the current front waiting for a lane
  const int tw = FW - 4 * S, h = 2 * S;
  const int oi = (int)(blockIdx.x / ntx) * tw - h, oj = (int)(blockIdx.x % ntx) * tw - h;
  for (int q = threadIdx.x; q < FN; q += FB) {
    const int i = oi + q / FW, j = oj + q % FW;
    if (i < 0 || j < 0 || i >= rows || j >= cols) { L.t[q] = 1.0e6f; L.cur[q] = L.org[q] = 0; L.dl[q] = 0; continue; }
    const size_t p = (size_t)i * cols + j;
    const int dd = d[p];
    const bool done = dd <= k0;
    const uint8_t v = in[p];
    L.org[q] = v;
    L.cur[q] = done ? out[p] : v;
    L.t[q] = done ? T[p] : 1.0e6f;
    L.dl[q] = (uint8_t)(done ? 0 : (dd - k0 > S ? S + 1 : dd - k0));
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint16_t* wq = work[wv];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int s = 1; s <= S; ++s) {
    // fronts earlier than s are complete in the local region at distance >= 2 (s - 1) from the edge; front s is computed where all its
    // reads (distance <= 2) stay inside that region.  A pixel of front s reads no other pixel of front s through t / cur.  The cells of
    // front s are packed 64 to a wave (ballot) so that a wave runs the estimator once per 64 cells, not once per 64 cells scanned.
    const int lo = 2 * s, n = FW - 4 * s, nn = n * n;
    auto run = [&](int x) {
      const int r = x / FW, c = x % FW;
      float tv; uint8_t vv;
      fr_pixel(L, r, c, oi + r, oj + c, rows, cols, oi, oj, s, tv, vv);
      L.t[x] = tv; L.cur[x] = vv;
    };
    int cnt = 0;
    for (int q0 = wv * 64; q0 < nn; q0 += FB) {
      const int q = q0 + lane;
      int x = 0;
      bool act = false;
      if (q < nn) { x = (lo + q / n) * FW + lo + q % n; act = L.dl[x] == s; }
      const unsigned long long m = __ballot(act);
      const int nact = __popcll(m), rank = __popcll(m & below);
      if (act && cnt + rank < 64) wq[cnt + rank] = (uint16_t)x;
      if (cnt + nact >= 64) {
        fr_wave_sync();
        const int y = wq[lane];
        fr_wave_sync();
        if (act && cnt + rank >= 64) wq[cnt + rank - 64] = (uint16_t)x;
        cnt = cnt + nact - 64;
        run(y);
      } else {
        cnt += nact;
      }
    }
    fr_wave_sync();
    if (lane < cnt) run(wq[lane]);
    __syncthreads();
  }
  for (int q = threadIdx.x; q < tw * tw; q += FB) {
    const int r = h + q / tw, c = h + q % tw, i = oi + r, j = oj + c, x = r * FW + c;
    if (i >= rows || j >= cols) continue;
    const int dl = L.dl[x];
    if (dl >= 1 && dl <= S) { const size_t p = (size_t)i * cols + j; T[p] = L.t[x]; out[p] = L.cur[x]; }
  }
}
}  // namespace

// ---- the pipeline on device images (emap_launch.h: FrontsDev) ------------------------------------------------------------------------
namespace {
size_t fr_tiles(int rows, int cols, int S) { const int tw = FW - 4 * S; return (size_t)((cols + tw - 1) / tw) * ((rows + tw - 1) / tw); }
size_t fr_up(size_t b) { return (b + 255) & ~(size_t)255; }
size_t fr_blk(int rows, int cols) { return 2 * (size_t)((rows + DTB - 1) / DTB) * cols; }      // ints: top and bot of every (block, column)
// distance transform and the tiles' initial state (k_fr_init leaves max d in *f.dmax, which the caller has zeroed if it reads it)
void fr_begin(hipStream_t st, const FrontsDev& f, int rows, int cols, int S) {
  const int tw = FW - 4 * S, ntx = (cols + tw - 1) / tw;
  const int nb = (rows + DTB - 1) / DTB;
  hipLaunchKernelGGL(k_fr_dt_cols_local, dim3((cols + FB - 1) / FB, nb), dim3(FB), 0, st, f.mask, f.g, f.blk, f.blk + (size_t)nb * cols, rows, cols);
  if (nb > 1)      // (one block: its own sweeps are the whole column)
    hipLaunchKernelGGL(k_fr_dt_cols_carry, dim3((cols + FB - 1) / FB, nb), dim3(FB), 0, st, f.g, f.blk, f.blk + (size_t)nb * cols, rows, cols, nb);
  hipLaunchKernelGGL(k_fr_dt_rows, dim3((rows + FB / 64 - 1) / (FB / 64)), dim3(FB), 0, st, f.g, f.d, rows, cols);
  hipLaunchKernelGGL(k_fr_init, dim3((unsigned)fr_tiles(rows, cols, S)), dim3(FB), 0, st, f.in, f.mask, f.d, f.T, f.out, f.tile_mm, f.dmax,
                     rows, cols, tw, ntx);
}
// fronts 1 .. n_advance * S, S per launch
void fr_advance(hipStream_t st, const FrontsDev& f, int rows, int cols, int S, int n_advance) {
  const int tw = FW - 4 * S, ntx = (cols + tw - 1) / tw;
  const unsigned ntiles = (unsigned)fr_tiles(rows, cols, S);
  for (int k = 0; k < n_advance; ++k)
    hipLaunchKernelGGL(k_fr_advance, dim3(ntiles), dim3(FB), 0, st, f.in, f.d, f.T, f.out, f.tile_mm, rows, cols, ntx, S, k * S);
}
}  // namespace

int fronts_default_steps() { return S_DEFAULT; }
size_t fronts_bytes(int rows, int cols, int S) {
  const size_t n = (size_t)rows * cols;
  return 3 * fr_up(n) + 3 * fr_up(4 * n) + fr_up(fr_tiles(rows, cols, S) * sizeof(int2)) + fr_up(sizeof(int)) + fr_up(fr_blk(rows, cols) * sizeof(int));
}
FrontsDev fronts_carve(unsigned char* b, int rows, int cols, int S) {
  const size_t n = (size_t)rows * cols, n1 = fr_up(n), n4 = fr_up(4 * n);
  FrontsDev f;
  f.in = b; f.mask = b + n1; f.out = b + 2 * n1; b += 3 * n1;
  f.g = (int*)b; f.d = (int*)(b + n4); f.T = (float*)(b + 2 * n4); b += 3 * n4;
  f.tile_mm = (int2*)b; b += fr_up(fr_tiles(rows, cols, S) * sizeof(int2));
  f.dmax = (int*)b; b += fr_up(sizeof(int));
  f.blk = (int*)b;
  return f;
}
void launch_fronts(hipStream_t st, const FrontsDev& f, int rows, int cols, int S, int n_advance) {
  fr_begin(st, f, rows, cols, S);
  fr_advance(st, f, rows, cols, S, n_advance);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
struct emap_inpainter {
  int device = 0;
  hipStream_t stream = nullptr;
  int steps = S_DEFAULT;
  size_t cap = 0, tcap = 0, bcap = 0;  // pixels / tiles / block summaries the scratch holds (grown to the largest image seen, never shrunk)
  uint8_t *in = nullptr, *mask = nullptr, *out = nullptr;
  int32_t *g = nullptr, *d = nullptr;
  float* T = nullptr;
  int2* tile_mm = nullptr;
  int* blk = nullptr;                  // top / bot of the column pass's row blocks
  int* dmax = nullptr;
  int* dmax_host = nullptr;            // pinned 4-byte landing slot
};

namespace {
void fr_free(emap_inpainter* ip) {
  hipFree(ip->in); hipFree(ip->mask); hipFree(ip->out); hipFree(ip->g); hipFree(ip->d); hipFree(ip->T);
  ip->in = ip->mask = ip->out = nullptr; ip->g = ip->d = nullptr; ip->T = nullptr; ip->cap = 0;
}
#define FR_CK(x) do { if ((x) != hipSuccess) return EMAP_ERR_HIP; } while (0)
}  // namespace

extern "C" int emap_inpainter_create(int32_t device, void* stream, emap_inpainter** out) {
  if (!out) return EMAP_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return EMAP_ERR_INVALID;
  if (device < 0) FR_CK(hipGetDevice(&device));               // -1: the calling thread's current device
  if (device >= n) return EMAP_ERR_INVALID;
  FR_CK(hipSetDevice(device));
  emap_inpainter* ip = new emap_inpainter();
  ip->device = device; ip->stream = (hipStream_t)stream;
  if (hipMalloc((void**)&ip->dmax, sizeof(int)) != hipSuccess || hipHostMalloc((void**)&ip->dmax_host, sizeof(int)) != hipSuccess) {
    hipFree(ip->dmax); delete ip; return EMAP_ERR_HIP;
  }
  *out = ip;
  return EMAP_OK;
}

extern "C" int emap_inpainter_destroy(emap_inpainter* ip) {
  if (!ip) return EMAP_OK;
  hipSetDevice(ip->device);            // (every call has synchronised its stream before returning: the caller's stream is not touched here)
  fr_free(ip);
  hipFree(ip->tile_mm); hipFree(ip->blk); hipFree(ip->dmax); hipHostFree(ip->dmax_host);
  delete ip;
  return EMAP_OK;
}

extern "C" int emap_inpainter_set_steps(emap_inpainter* ip, int32_t steps) {
  if (!ip || steps < 1 || steps > S_MAX) return EMAP_ERR_INVALID;
  ip->steps = steps;
  return EMAP_OK;
}

extern "C" int emap_inpaint_telea_fronts_u8(emap_inpainter* ip, const uint8_t* image, const uint8_t* mask, int32_t rows, int32_t cols,
                                            int32_t radius, uint8_t* out, int32_t* fronts_run) {
  if (!ip || !image || !mask || !out || radius != 1 || rows < 2 || cols < 2 || (int64_t)rows * cols > (int64_t)1 << 30) return EMAP_ERR_INVALID;
  if (fronts_run) *fronts_run = 0;
  FR_CK(hipSetDevice(ip->device));
  const size_t n = (size_t)rows * cols;
  const int S = ip->steps;
  const size_t ntiles = fr_tiles(rows, cols, S);
  if (n > ip->cap) {
    FR_CK(hipStreamSynchronize(ip->stream));
    fr_free(ip);
    FR_CK(hipMalloc((void**)&ip->in, n)); FR_CK(hipMalloc((void**)&ip->mask, n)); FR_CK(hipMalloc((void**)&ip->out, n));
    FR_CK(hipMalloc((void**)&ip->g, n * sizeof(int32_t))); FR_CK(hipMalloc((void**)&ip->d, n * sizeof(int32_t)));
    FR_CK(hipMalloc((void**)&ip->T, n * sizeof(float)));
    ip->cap = n;
  }
  if (ntiles > ip->tcap) {
    FR_CK(hipStreamSynchronize(ip->stream));
    hipFree(ip->tile_mm); ip->tile_mm = nullptr; ip->tcap = 0;
    FR_CK(hipMalloc((void**)&ip->tile_mm, ntiles * sizeof(int2)));
    ip->tcap = ntiles;
  }
  if (fr_blk(rows, cols) > ip->bcap) {
    FR_CK(hipStreamSynchronize(ip->stream));
    hipFree(ip->blk); ip->blk = nullptr; ip->bcap = 0;
    FR_CK(hipMalloc((void**)&ip->blk, fr_blk(rows, cols) * sizeof(int)));
    ip->bcap = fr_blk(rows, cols);
  }
  hipStream_t st = ip->stream;
  const FrontsDev f{ip->in, ip->mask, ip->out, ip->g, ip->d, ip->T, ip->tile_mm, ip->dmax, ip->blk};
  FR_CK(hipMemcpyAsync(ip->in, image, n, hipMemcpyHostToDevice, st));
  FR_CK(hipMemcpyAsync(ip->mask, mask, n, hipMemcpyHostToDevice, st));
  FR_CK(hipMemsetAsync(ip->dmax, 0, sizeof(int), st));
  fr_begin(st, f, rows, cols, S);
  FR_CK(hipGetLastError());
  FR_CK(hipMemcpyAsync(ip->dmax_host, ip->dmax, sizeof(int), hipMemcpyDeviceToHost, st));
  FR_CK(hipStreamSynchronize(st));
  const int dmax = *ip->dmax_host;
  if (dmax == 0 || dmax >= FINF) {                             // nothing to fill, or no known pixel: the output is the input
    memcpy(out, image, n);
    return EMAP_OK;
  }
  fr_advance(st, f, rows, cols, S, (dmax + S - 1) / S);
  FR_CK(hipGetLastError());
  FR_CK(hipMemcpyAsync(out, ip->out, n, hipMemcpyDeviceToHost, st));
  FR_CK(hipStreamSynchronize(st));
  if (fronts_run) *fronts_run = dmax;
  return EMAP_OK;
}
