// Hand-written CDNA4 (gfx950) kernels of the elevation-map fusion hot path.
// Reference semantics: leggedrobotics/elevation_mapping_cupy, EM/kernels/custom_kernels.py (cited per kernel);
// execution model: the deterministic two-phase contract of DESIGN.md (fuse and ray passes only READ the map and
// write integer/fixed-point accumulators, per-cell passes commit) -- not a translation of the CuPy kernels.
// Compiled with -ffp-contract=off: decisions (indices, gates) must be bit-identical to the oracle.
#include "emap_launch.h"
#include "emap_bin_hist.h"
#include <cstdlib>
#include <cstring>

// ---------------------------------------------------------------------------------------------------------
// Phase A: drift statistics + points-per-cell (error_counting_kernel, custom_kernels.py:280-345)
// One point per lane, coalesced 12-B xyz loads; one 16-B gather of (h, v, valid, trav); ONE 64-bit atomic per
// point (points and inliers packed); the two global sums are wave-reduced and spread over 256 slots.
// ---------------------------------------------------------------------------------------------------------
// GATE (round 5): whole frames on this path (small clouds: the robot-scale configuration the reference ships is a chain of six
// launches of ~4.5 us each) evaluate the drift gate in the LAST workgroup to finish -- the two-level ticket k_bin_scan uses: a
// workgroup's slot atomics are performed at the memory side, s_waitcnt waits for their acknowledgements, then the ticket -- instead of
// in a launch of their own (k_gate); the staged API and the multi-GPU frame keep k_gate.
struct CountGate { int on, pad_; GateArgs A; FrameDev* F; unsigned int* sync; };
template <int MODE>
__global__ __launch_bounds__(EM_BLOCK) void k_count(KP P, Pose T, const float* __restrict__ pts, long n, int stride,
                                                     Cells cells, AccF* __restrict__ acc,
                                                     ErrSlot* __restrict__ slots, CountGate CG) {
  long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  long long e_fix = 0;
  unsigned int inl = 0;
  if (i < n) {
    float rx, ry, rz;
    load_point(pts, i, stride, rx, ry, rz);
    Geo g = geometry<MODE>(P, T, rx, ry, rz);
    Owned oc = owned(P, g.ix, g.iy);
    long c = (g.finite && g.valid && g.inside) ? oc.c : -1;
    if (c >= 0) {
      float4 m = cells.hot[c];   // h, v, valid, trav
      cell_now(P, m, oc.prow, oc.pcol);
      bool inlier = m.z > 0.5f && (double)fabsf(m.x - g.z) < (double)m.y * P.mt && (double)m.y < P.dcvi_half &&
                    (double)m.w > P.trav_inlier;
      if (inlier) { inl = 1; e_fix = __double2ll_rn((double)(g.z - m.x) * EM_SCALE_E); }
      atomicAdd(&acc[c].pts_inl, 1ull | ((unsigned long long)inl << 32));
    }
  }
  if (__any(inl)) {
    long long s = wave_sum_ll(e_fix);
    unsigned long long k = __popcll(__ballot(inl));
    if ((threadIdx.x & 63) == 0) {
      unsigned int slot = (blockIdx.x * (EM_BLOCK / 64) + (threadIdx.x >> 6)) & (EM_ERR_SLOTS - 1);
      atomicAdd(reinterpret_cast<unsigned long long*>(&slots[slot].sum), (unsigned long long)s);
      atomicAdd(&slots[slot].cnt, k);
    }
  }
  if (CG.on) {                                                 // (uniform)
    __shared__ bool s_last;
    __builtin_amdgcn_s_waitcnt(0);                             // this wave's slot atomics are acknowledged
    __syncthreads();
    if (threadIdx.x == 0) s_last = last_block_ticket(CG.sync, blockIdx.x, gridDim.x);
    __syncthreads();
    if (s_last && threadIdx.x < 64) gate_eval(CG.A, slots, CG.F, (int)threadIdx.x, 0, nullptr, nullptr);
  }
}

// Phase A': drift gate (elevation_mapping.py:346-357) evaluated on the device by one wave: reduces the slots
// (integer => order independent), decides the shift, keeps additive_mean_error, re-arms the slots.
// Row-strip contexts: `reduce_only` publishes the local sums (2 doubles, device memory) for the all-reduce and stops;
// `dev_totals` (2 doubles, device memory, e.g. the all-reduced tensor) replaces the local sums in the gate.
__global__ __launch_bounds__(64) void k_gate(GateArgs A, ErrSlot* __restrict__ slots, FrameDev* __restrict__ F, int reduce_only,
                                             double* __restrict__ dev_out, const double* __restrict__ dev_totals) {
  gate_eval(A, slots, F, threadIdx.x, reduce_only, dev_out, dev_totals);
}

// ---------------------------------------------------------------------------------------------------------
// Phase B: Kalman fusion (add_points_kernel fusion part, custom_kernels.py:160-197) against snapshot S0.
// Reads (h, v) + points-per-cell, writes ONLY accumulators: <= 4 64-bit integer atomics into one 40-B record.
// ---------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(EM_BLOCK) void k_fuse(KP P, Pose T, const float* __restrict__ pts, long n, int stride,
                                                    Cells cells, AccF* __restrict__ acc,
                                                    const FrameDev* __restrict__ F) {
  long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  float rx, ry, rz;
  load_point(pts, i, stride, rx, ry, rz);
  Geo g = geometry<MODE>(P, T, rx, ry, rz);
  const Owned oc = owned(P, g.ix, g.iy);
  long c = (g.finite && g.valid && g.inside) ? oc.c : -1;
  if (c < 0) return;
  const float shift = F->shift;
  float4 hv = cells.hot[c];
  cell_now(P, hv, oc.prow, oc.pcol);
  float map_h = hv.x + shift, map_v = hv.y;
  const unsigned int n_pts = (unsigned int)(acc[c].pts_inl & 0xffffffffull);
  float num_points = (float)n_pts;
  // a cell that received exactly one point this frame has a single writer: plain stores, no atomics (an atomic costs
  // ~44 ns/Mop on MI355X regardless of width or locality -- tools/microbench.hip -- a plain 8-B store a third of that)
  const bool single = n_pts == 1u;
  if ((double)fabsf(map_h - g.z) > (double)map_v * P.mt) {          // outlier :173-175
    if (single) acc[c].cnt_out = 1ull << 32; else atomicAdd(&acc[c].cnt_out, 1ull << 32);
    return;
  }
  if (P.edge && (double)num_points > P.wall &&
      (double)g.z < (double)map_h - (double)map_v * P.mt / (double)num_points) return;   // edge sharpening :177-179
  float new_h = (map_h * g.v + g.z * map_v) / (map_v + g.v);          // :181-182
  float new_v = (map_v * g.v) / (map_v + g.v);
  const long long fh = __double2ll_rn((double)new_h * EM_SCALE_H), fv = __double2ll_rn((double)new_v * EM_SCALE_V);
  const unsigned long long lt = ((unsigned long long)(i + 1) << 32) | (unsigned long long)__float_as_uint(new_h);
  if (single) {
    acc[c].cnt_out = 1ull; acc[c].sum_h = fh; acc[c].sum_v = fv; acc[c].latest = lt;
    return;
  }
  atomicAdd(reinterpret_cast<unsigned long long*>(&acc[c].sum_h), (unsigned long long)fh);
  atomicAdd(reinterpret_cast<unsigned long long*>(&acc[c].sum_v), (unsigned long long)fv);
  atomicAdd(&acc[c].cnt_out, 1ull);
  atomicMax(&acc[c].latest, lt);
}

// Phase B': materialise S1 (only launched on the staged / global-atomic path; the tile kernel k_tile_fuse<true, true> commits itself)
// Also emits the "inert" bitmap (1 bit per owned cell: known AND updated recently).  A ray step on such a cell cannot
// have any effect (custom_kernels.py:228-237), so k_rays tests the bit (128 KB for a 1024^2 map, cache resident)
// instead of gathering the 32-byte cell.  Border cells (is_inside false, :34-44 -- rays never act there) are marked inert too, which
// is how k_rays implements `if (!is_inside(nidx)) continue` (:211) without a test of its own.  The bitmap is indexed by LOGICAL
// column and, on single-strip contexts, logical row (strips: local physical row) -- what the march has at hand (bitmap_row).  Layout: one row of ceil(C / 64) 64-bit words per map row (a 64-column tile segment of a
// row is exactly one word, so the tile kernel can store a wave ballot); grid: x = 64-column groups, y = rows, one wave per word.
__global__ __launch_bounds__(64) void k_commit(KP P, Cells cells, const AccF* __restrict__ acc,
                                               const FrameDev* __restrict__ F, unsigned long long* __restrict__ inert) {
  // one wave = 64 LOGICAL columns of one owned physical row (so that its ballot is one aligned word of the logical bitmap)
  const int lrow = blockIdx.y, lcol = blockIdx.x * 64 + threadIdx.x, prow = P.row0 + lrow;
  bool quiet = false;
  if (lcol < P.C) {
    const int pcol = phys_col(P, lcol);
    const long c = (long)(lrow + P.halo) * P.C + pcol;
    Cell m = cells[c];
    cell_now(P, m, prow, pcol);                   // pending map shifts are written out here
    AccF a = acc[c];
    m.h += F->shift;
    commit_cell(P, m, a);
    cells[c] = m;
    quiet = (!(m.valid < 0.5f) && m.time < 0.5f) || border_cell(P, logi_row(P, prow), lcol);
  }
  const unsigned long long bits = __ballot(quiet);
  if (threadIdx.x == 0) inert[(long)bitmap_row(P, prow) * gridDim.x + blockIdx.x] = bits;
}

// ---------------------------------------------------------------------------------------------------------
// Phase C: visibility clean-up (add_points_kernel ray part, custom_kernels.py:198-259) against snapshot S1.
// One ray per lane; each step gathers ONE 32-byte cell; all effects go to the 16-byte AccR record
// (fixed-point add / integer add / ordered-uint max) so the result is independent of scheduling.
// ---------------------------------------------------------------------------------------------------------
// ALU diet (the first version of this kernel was VALU-bound on two fp64 divisions per step, profiles/r01_a_*):
//   * the step sequence s_k = half(s_{k-1} + step) does not depend on the ray: host-built table, scalar loads;
//   * reference_fp16 mode: a coordinate is rounded to half before the index computation, so the cell index is a
//     function of 16 bits: host-built lookup table (exact double arithmetic of the reference), compacted to the
//     exponent range where it varies and staged in LDS (~37 KB for a 1024^2 map) -> no fp64 in the loop;
//   * float-vs-double-constant comparisons use host-rounded float thresholds (exactly equivalent).
// min-reduce of nz into the ordered-uint key.  Thousands of rays cross the same unknown cell and an atomic costs
// ~44 ns/Mop whatever the address pattern, so test first with a plain (possibly stale => conservative) load: the key
// only grows, a stale smaller value can only cause a redundant atomic, never a missed one.
__device__ __forceinline__ unsigned int ray_key_load(const unsigned int* key_ptr) {
  // a DEVICE-COHERENT load (sc1): the atomics execute at the memory side, so a plain / nt load keeps seeing the value its own XCD's L2
  // cached before the other seven XCDs raised the key -- and every visit below that stale value issues another atomic (the first
  // frame after clear(), where every visit of the 39 % unknown cells comes here: measured in round 4).  The non-temporal load
  // (__builtin_nontemporal_load) was the other side of that measurement and lost -- first frame after clear() 1.52-1.63 ms against
  // 1.02 ms at 1024^2, 6.46 against 4.17 ms at 4096^2, steady state equal -- and is no longer kept as a build.
  return __hip_atomic_load(key_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ray_upper_min(unsigned int* key_ptr, float nz) {
  const unsigned int key = ~float_ord(nz);
  if (ray_key_load(key_ptr) < key) atomicMax(key_ptr, key);
}

// Cell index of a sample coordinate along one axis.  IDX selects how:
//   0  the defining arithmetic (axis_idx: the reference's fp64 expression in reference_fp16 mode)
//   1  reference_fp16 only: host-built table over the half bit pattern, staged in LDS (exact by construction)
//   2  reference_fp16 only: one float fma + floor + add + clamp + truncation on the half-rounded coordinate -- the host proves it equal to the
//      defining arithmetic for EVERY half bit pattern before selecting it (emap_api.hip: build_ray_tables), 5 VALU, no LDS
template <int MODE, int IDX> struct AxisIdx {
  const unsigned short* t; unsigned int lo_m1, hi, span;   // IDX 1: per sign [small, idx(lo..hi-1), big]
  float frac_v;                                            // IDX 2: hw_frac_f in a VECTOR register (the fma already has a scalar operand)
  __device__ __forceinline__ int operator()(const KP& P, float x) const {
    if constexpr (IDX == 1) {   // branch-free: clamp the magnitude into the tabulated range (sentinels hold the constant tails)
      const unsigned int b = (unsigned int)__builtin_bit_cast(unsigned short, (_Float16)x);
      const unsigned int mag = b & 0x7fffu, sg = b > 0x8000u;          // -0.0 indexes like +0.0 (get_idx(-0.0) == get_idx(0.0))
      const unsigned int m = min(max(mag, lo_m1), hi) - lo_m1;
      return (int)t[(sg ? span : 0u) + m];
    } else if constexpr (IDX == 2) {
      // floor BEFORE the half width is added: a tiny negative coordinate would otherwise round up to exactly C/2 in fp32 where the
      // reference's double stays just below it and truncates to C/2 - 1 (the integer add afterwards is exact)
      const float q = (float)(_Float16)x;
      const float f = __builtin_floorf(__builtin_fmaf(q, P.inv_res_f, frac_v)) + P.hw_int_f;
      return (int)__builtin_amdgcn_fmed3f(f, 0.0f, P.cm1_f);
    } else return axis_idx<MODE>(P, Qf<MODE>(x));
  }
};

// a * b + c on the low 24 bits of a and b (v_mad_u32_u24; the compiler's own pattern masks the operands first)
__device__ __forceinline__ unsigned int mad24(unsigned int a, unsigned int b, unsigned int c) {
  unsigned int r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// The march.  All lanes of a wave walk the SAME step index k (the step sequence s_k does not depend on the ray), so s_k is a
// scalar load and the loop counter lives in SGPRs; a lane takes part while k is inside its own range [kb, ke): ke = number of
// samples with s_k < ray_length (binary search once per ray instead of a compare + break per step), kb > 0 only on row strips.
// Per step and lane: 4 VALU for the sample position, the two axis indices, one mad for the flat index, the same-cell / inside /
// range predicate, one bitmap bit; everything else happens only for the few cells that are neither known-and-fresh nor out.
// (launch bounds: 8 waves per SIMD, i.e. two 1024-thread workgroups per CU -- measured: with 82 instead of 70 SGPRs the kernel
// silently dropped to one workgroup per CU and ran 13 % slower)
// Which part of the bitmap the LMAP variants of whole-map contexts keep in LDS (round 6): no ray reaches beyond max_ray_length from the
// sensor, so only the rows [r0, r0 + nr) x 32-bit word columns [w0, w0 + wpr) around it are staged -- 520 x 576 cells = 37 KB at
// 10 m / 0.04 m whatever the size of the map (before: the whole map's bitmap, 128 KB at 1024^2, and no LDS variant at all beyond
// ~1100^2 cells: the 4096^2 frame marched at 661 G visits / s against 914 at 1024^2).  Computed by the host (ray_lds_window) with a
// margin that bounds every rounding between the sensor position and a sample's cell; the whole map when it is no larger.
struct LWin { int r0, nr, w0, wpr; };
template <int MODE, bool STATS, int IDX, bool STRIP, int BLOCK, bool LMAP, int LPR>
#ifndef RAY_OCC
#define RAY_OCC 8
#endif
__global__ __launch_bounds__(BLOCK, LMAP ? 4 : RAY_OCC) void k_rays(KP P, Pose T, RayTab Rt, const float* __restrict__ pts, long n, int stride,
                                                 Cells cells,
                                                 AccRView AR, const float* __restrict__ normal,
                                                 long plane_stride, FrameDev* __restrict__ F,
                                                 const unsigned long long* __restrict__ inert64,
                                                 const unsigned int* __restrict__ inl, int inl_stride, const float* __restrict__ thr,
                                                 const unsigned int* __restrict__ order, const unsigned int* __restrict__ n_sorted, LWin LW) {
  // walking sorted records: workgroups behind the last record leave before the prologue (a frame that marches its rays by ray sorts
  // only the points of the strip's rows: most of a grid sized for the whole cloud is empty then)
  // The workgroups take the chunks of the sorted records OUTSIDE IN (first, last, second, second to last, ...).  The records are sorted
  // by end-point tile, row-major over the map, and the map rides with the robot: the first and the last chunks are the far field --
  // rays at the clip length, 350 steps, ~40 us per 1024-ray workgroup -- and the middle ones end next to the sensor (20-60 steps).
  // Dispatched in tile order, a scan-ordered cloud finished with a round of far-field workgroups on a fifth of the CUs (terrain scene:
  // 4.3x fewer wave cycles than the uniform cloud, 1.28x less time); now the long ones start first and the short ones fill the gaps:
  // 221 -> 217 us there, 310 -> 301 us on four alternating uniform clouds (same box).  What remains of that gap is latency: a far-field
  // wave works off a batch of queued visits (unknown cells between the scan rings) every other step, each a dependent trip to the
  // threshold table; with the bitmap in global memory and two workgroups per CU the terrain pass takes 187 us, the uniform one more.  (The valid points outside the owned cells sit in the last bin: long rays, first.)
  unsigned int chunk = blockIdx.x;
  if (order) {
    const unsigned int nbs = (unsigned int)(((long)*n_sorted * LPR + BLOCK - 1) / BLOCK);
    if (blockIdx.x >= nbs) return;
    chunk = (blockIdx.x & 1u) ? nbs - 1u - (blockIdx.x >> 1) : (blockIdx.x >> 1);      // (plain tile order, chunk = blockIdx.x, is the side that lost those measurements: 221 and 310 us)
  }
  const unsigned int* __restrict__ inert = reinterpret_cast<const unsigned int*>(inert64);   // 32-bit words: cheaper shifts
  const unsigned int wpr32 = (unsigned int)((P.pitch + 63) / 64) * 2u;                       // 32-bit words per bitmap row (pitch = C; a ray window: its width)
  // LDS words: [table (span)] [s_k (nS)] [queues (BLOCK/64 * 384)]
  extern __shared__ unsigned int slut32[];
  const unsigned int span = IDX == 1 ? (unsigned int)(Rt.hi - Rt.lo) + 2u : 0u;
  float* sS = reinterpret_cast<float*>(slut32 + ((span + 3u) & ~3u));      // step table s_k in LDS (16-byte aligned, padded by 8 x +inf: the march reads float4)
  const int nS = Rt.nS, nSp = ((nS + 3) & ~3) + 8 * LPR;
  if (IDX == 1) {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(Rt.lut);   // 2 signs * span u16 = span u32
    for (unsigned int k = threadIdx.x; k < span; k += BLOCK) slut32[k] = src[k];
  }
  for (int k = threadIdx.x; k < nSp; k += BLOCK) sS[k] = k < nS ? Rt.S[k] : INFINITY;
  unsigned int* qbase = reinterpret_cast<unsigned int*>(sS + nSp);                 // per-wave visit queues: 3 x 128 words each
  // LMAP: the whole bitmap (+ the all-ones word behind it) is staged in LDS when it fits next to the queues (128 KB for a 1024^2
  // map: one workgroup per CU, which costs nothing -- 4 and 8 waves per SIMD run this kernel equally fast).  A scattered 64-lane
  // dword load keeps the CU's single texture addresser busy for ~45 clocks; the LDS serves it in a handful (measured: frame 0.495
  // -> 0.449 ms at 1024^2 / 1 M rays).
  // (the copy starts at an LDS offset aligned to the row pitch: the word address is then (row * pitch) + ((column part) | base), one
  // v_and_or instead of an and + an add per step)
  typedef __attribute__((address_space(3))) unsigned int lds_u32;
  constexpr bool WIN = LMAP && !STRIP;                          // whole-map contexts stage the sensor's reach window only (LWin)
  const unsigned int lwpr32 = WIN ? (unsigned int)LW.wpr : wpr32, lrows = WIN ? (unsigned int)LW.nr : (unsigned int)P.nrows;      // the LDS copy: 32-bit words per row, rows
  unsigned int map_align = 16u; if (!WIN) { map_align = 4u; while (map_align < wpr32 * 4u) map_align <<= 1; }      // (!WIN: aligned to the row pitch, see above; WIN adds its base)
  // (A per-wave KEY CACHE for the first frame after clear() -- {cell, key} pairs the wave has already pushed, 256 direct-mapped 64-bit
  // entries per wave, a visit whose key is not above the cached one skips the device-coherent key load and the atomic -- was built and
  // measured in round 6: bit-identical, and SLOWER, same box: steady uniform pass 218.6 -> 228 us, first frame after clear() 0.90 -> 1.0 ms.
  // The cold frame is not bound by its key traffic: with an all-zero bitmap EVERY step of every ray goes through the visit queue.)
  const unsigned int q_end = (unsigned int)(size_t)(lds_u32*)(qbase + (BLOCK / 64) * 384);       // byte offset in LDS
  const unsigned int smap_base = LMAP ? (q_end + map_align - 1u) & ~(map_align - 1u) : 0u;
  if (LMAP) {     // a pure copy: LDS-DMA, one kilobyte per wave instruction; the two trailing all-ones words by hand
    lds_u32* smap = (lds_u32*)(size_t)smap_base;
    const unsigned int nb = lrows * lwpr32 * 4u;                                // bytes of the staged bitmap
    const char* src = reinterpret_cast<const char*>(inert);
    const unsigned int wave0 = (unsigned int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 1024u, lane16 = (threadIdx.x & 63u) * 16u;
    if (WIN && (lwpr32 != wpr32 || LW.r0 != 0)) {
      // a window: 16-byte pieces enumerated row-major over the window land contiguously in LDS (lane i of a wave at base + 16 i)
      // whatever their global addresses (host: w0 and wpr are multiples of 4 words, the map's row pitch of 16 bytes)
      const unsigned int ppr = lwpr32 / 4u;
      for (unsigned int off = wave0; off < nb; off += (BLOCK / 64) * 1024u) {
        const unsigned int pce = (off + lane16) / 16u, row = pce / ppr, j = pce - row * ppr;
        if (off + lane16 < nb) lds_dma16_at(src + ((size_t)((unsigned int)LW.r0 + row) * wpr32 + (unsigned int)LW.w0) * 4u + j * 16u, smap_base + off);
      }
      if (threadIdx.x < 2) smap[nb / 4u + threadIdx.x] = 0xffffffffu;
    } else {
      for (unsigned int off = wave0; off < nb; off += (BLOCK / 64) * 1024u)
        if (off + lane16 < nb) lds_dma16_at(src + off + lane16, smap_base + off);
      if (threadIdx.x < 2) smap[nb / 4u + threadIdx.x] = inert[nb / 4u + threadIdx.x];
    }
  }
  __syncthreads();
  float frac_v = P.hw_frac_f;
  asm volatile("" : "+v"(frac_v));
  AxisIdx<MODE, IDX> aidx{reinterpret_cast<const unsigned short*>(slut32), (unsigned int)Rt.lo - 1u, (unsigned int)Rt.hi, span, frac_v};
  // Ray order.  All 64 lanes of a wave march until the LONGEST of their rays ends; with the cloud in sensor order a wave holds
  // unrelated rays (mean length / longest ~ 0.55 for a uniform cloud).  On binned frames the counting sort by end-point tile is
  // already there: `order` = the sorted 16-byte records (word 3: point index; valid points outside the owned cells sit in a last
  // bin), *n_sorted their number -- a wave then marches 64 rays into the same 16 x 64 cell tile: equal lengths, neighbouring
  // bitmap words.  The effects are order-independent accumulator updates: results are unchanged.
  // LPR lanes per ray (small clouds): lane `sub` of a ray marches the samples K = LPR * k + sub -- the march is a chain of ~350
  // dependent steps per wave, which is pure latency when the cloud cannot fill the chip; four lanes per ray cut the chain to a quarter
  // (each lane computes the cell of sample K - 1 itself for the new-cell test).
  const long gi = (long)chunk * BLOCK + threadIdx.x;
  const int sub = LPR > 1 ? (int)(gi % LPR) : 0;
  long i = gi / LPR;
  bool have = i < n;
  if (order) { have = have && i < (long)*n_sorted; if (have) i = (long)order[i * 4 + 3]; }
  const int C = P.C;
  float gx = 0.f, gy = 0.f, gz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f, dec = 0.f;
  int kb = 0x7fffffff, ke = 0;                       // empty range: lanes without a (valid) ray never take part
  if (have) {
    float rx_, ry_, rz_;
    load_point(pts, i, stride, rx_, ry_, rz_);
    Geo g = geometry<MODE>(P, T, rx_, ry_, rz_);
    // invalid points march but never act (:226); non-finite geometry is undefined in the reference and skipped here
    if (g.finite && g.valid && fabsf(g.x) < INFINITY && fabsf(g.y) < INFINITY && fabsf(g.z) < INFINITY) {
      gx = g.x; gy = g.y; gz = g.z;
      // ray_vector (:83-101): every intermediate is a float16 variable in the reference
      float px = Qf<MODE>(g.x), py = Qf<MODE>(g.y), pz = Qf<MODE>(g.z);
      float vx = Qf<MODE>(px - T.tq[0]), vy = Qf<MODE>(py - T.tq[1]), vz = Qf<MODE>(pz - T.tq[2]);
      float norm = Qf<MODE>(sqrtf(vx * vx + vy * vy + vz * vz));
      if (norm > 0.f) { rx = Qf<MODE>(vx / norm); ry = Qf<MODE>(vy / norm); rz = Qf<MODE>(vz / norm); }
      const float ray_length = fminf(norm, P.q_mrl);
      dec = (float)(-P.cs / ((double)ray_length / P.mrl));
      int lo = 0, hi = nS;                                      // ke = first k with !(s_k < ray_length); s_k is strictly increasing
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (sS[mid] < ray_length) lo = mid + 1; else hi = mid; }
      kb = 0; ke = lo;
      // Row strips: the rows of a strip are a band in x, and x(s) is monotone along a ray, so the samples that can land in owned
      // rows form one contiguous range of the step table.  March only that range (band widened by 2 cells: more than the
      // float16 rounding of the sample position can move a cell, and it lets the same-cell test warm up before the first
      // owned row exactly as in the full march); the per-sample ownership test stays.
      if (STRIP) {
        // the owned PHYSICAL rows are the logical rows [ls, ls + nrows) mod C; when that interval wraps the whole ray is marched
        const int ls = logi_row(P, P.row0);
        if (ls + P.nrows <= C) {
          const float xlo = (float)(((double)(ls - 2) - P.half_w) * P.res), xhi = (float)(((double)(ls + P.nrows + 2) - P.half_w) * P.res);
          float s_lo = -INFINITY, s_hi = INFINITY;
          if (fabsf(rx) > 1e-6f) {
            const float a = (xlo - T.t[0]) / rx, b = (xhi - T.t[0]) / rx;
            s_lo = fminf(a, b); s_hi = fmaxf(a, b);
          } else if (T.t[0] < xlo || T.t[0] > xhi) s_hi = -INFINITY;
          s_lo -= 2.0f * P.q_step; s_hi += 2.0f * P.q_step;
          lo = 0; hi = nS;                                        // first k with S[k] >= s_lo
          while (lo < hi) { const int mid = (lo + hi) >> 1; if (sS[mid] < s_lo) lo = mid + 1; else hi = mid; }
          kb = lo;
          hi = nS;                                                // first k with S[k] > s_hi
          while (lo < hi) { const int mid = (lo + hi) >> 1; if (sS[mid] <= s_hi) lo = mid + 1; else hi = mid; }
          ke = min(ke, lo);
          if (ke <= kb) { kb = 0x7fffffff; ke = 0; }
        }
      }
    }
  }
  const int wb = __builtin_amdgcn_readfirstlane(wave_min_i(kb)), we = __builtin_amdgcn_readfirstlane(wave_max_i(ke));   // SGPRs
  unsigned long long visits = 0;
  // Deferred cell work.  Only a few percent of the visits need the cell at all (it is neither known-and-fresh nor next to the
  // ray's end point), but with 64 unrelated rays per wave almost every step has ONE such lane, and its dependent loads (cell ->
  // normals -> inlier count) then stall the whole wave for a memory round trip per step.  The march therefore only QUEUES those
  // visits (cell, step s, lane of the ray) in a per-wave LDS stack; whenever 64 are waiting, the wave works them off with all lanes
  // busy -- lane j takes visit j and fetches the ray's direction and decrement from the owning lane's registers (ds_bpermute).
  // Results are unchanged: every effect is an order-independent accumulator update.
  constexpr int QCAP = 128;
  unsigned int* qc = qbase + (threadIdx.x >> 6) * (3 * QCAP);
  float* qz = reinterpret_cast<float*>(qc + QCAP);
  unsigned int* ql = qc + 2 * QCAP;
  const int lane = threadIdx.x & 63;
  int qn = 0;                                   // wave-uniform number of queued visits
  auto work = [&](int first, int count) {       // visits [first, first + count), count <= 64; executed by the whole wave
    const bool has = lane < count;
    const unsigned int xy = has ? qc[first + lane] : 0u;
    const int lix = (int)(xy >> 16), liy = (int)(xy & 0xffffu);                                   // logical cell of the visit
    const unsigned int lrow = (unsigned int)(phys_row(P, lix) - P.row0), col = (unsigned int)(phys_col(P, liy) - P.col0);   // owned (physical) row, column [of the ray window]
    const unsigned int c = (lrow + (unsigned int)P.halo) * (unsigned int)P.pitch + col;
    const float s = has ? qz[first + lane] : 0.f;
    const int src = has ? (int)ql[first + lane] : lane;
    // Block threshold first (written by k_tile_fuse<true, true>): no cell of this 8 x 8 block can be affected by a sample at or above it
    // (unknown cells: their upper bound; known stale cells: height + 0.05 > every nz that passes the penetration test).  A random
    // 32-byte cell costs a 128-byte line across the fabric -- 1.4 GB per frame before this filter; the table is 64 KB and L2 resident.
    // It needs only the sample height (one lane exchange) and rejects ~99 % of the queued visits; the rest of the ray (six more
    // exchanges, the distance test) is fetched only when some visit of the batch survives.
    const float erz = __shfl(rz, src, 64);
    const float nz = T.t[2] + erz * s;                                                   // the sample height, recomputed bit for bit
    const float bthr = (has && thr) ? thr[(lrow >> 3) * (unsigned int)((P.pitch + 7) >> 3) + (col >> 3)] : 3.4028234664e38f;
    const bool live = has && !(nz >= bthr);
    if (!__builtin_amdgcn_ballot_w64(live)) return;                                      // wave-uniform
    const float erx = __shfl(rx, src, 64), ery = __shfl(ry, src, 64), edec = __shfl(dec, src, 64);
    const float egx = __shfl(gx, src, 64), egy = __shfl(gy, src, 64), egz = __shfl(gz, src, 64);
    // What the visit contributes: a decrement + a hit (the penetration branch) and / or a lower upper bound.  Rays that end in one
    // tile travel together, so many of the 64 visits of a batch meet in the SAME cell at the same step -- after a long occlusion
    // (every cell stale) or a clear() (every cell unknown) each of them used to cost two or three device atomics at ~45 ns/Mop, the
    // whole frame 35x the steady one.  The contributions are integers under add / max, so the wave first combines the visits of a
    // cell in LDS (32 slots hashed by cell, carved out of the 64 queue entries this batch has just vacated) and one lane per slot
    // goes out to memory; a visit whose slot went to another cell goes out by itself.  Any grouping gives the same bits.
    long long c_dec = 0; unsigned int c_key = 0u, c_hit = 0u; bool contrib = false;
    if (live) {
      const float nx = T.t[0] + erx * s, ny = T.t[1] + ery * s;
      const float ddx = egx - nx, ddy = egy - ny, ddz = egz - nz;
      const float d = Qf<MODE>(ddx * ddx + ddy * ddy + ddz * ddz);
      if (!(d < Rt.f_d_thresh)) {                // (double)d < 0.1: too close to the point (:225-226)
        // a VIRGIN block (+INF: every cell quiet or unknown without a bound -- a cleared map, the band a map shift brings in): the
        // visit can only lower the cell's upper bound (:228-234 with is_upper_bound < 0.5), no cell load needed
        if (bthr == INFINITY) { contrib = true; c_key = ~float_ord(nz); }
        else {
          const float4 m0 = cells.hot[c], m1 = cells.cold[c];       // h v valid trav | time upper is_upper valid'
          if (m0.z < 0.5f) {                       // unknown cell: upper bound (:228-234)
            if (nz < m1.y || m1.z < 0.5f) { contrib = true; c_key = ~float_ord(nz); }
          } else if (!(m1.x < 0.5f) &&             // not updated recently (:236)
                     (double)m0.x > (double)nz + 0.01 - fmin((double)m0.y, 1.0) * 0.05) {
            // the normal planes keep the origin they were written with (the reference does not shift normal_map): logical -> their rows
            float n0 = 0.f, n1 = 0.f, n2 = 0.f;
            if (P.wmode) { n0 = normal[c]; n1 = normal[plane_stride + c]; n2 = normal[2 * plane_stride + c]; }      // (uniform) ray window: the planes were gathered cell by cell
            else {
              const long cn = normal_index(P, (int)lrow, lix, liy);
              if (cn >= 0) { n0 = normal[cn]; n1 = normal[plane_stride + cn]; n2 = normal[2 * plane_stride + cn]; }
            }
            const float ip = erx * Qf<MODE>(n0) + ery * Qf<MODE>(n1) + erz * Qf<MODE>(n2);
            if (!(fabsf(ip) < Rt.f_cos_thresh)) {
              // newmap[3]: drift inliers of this frame in the cell; a ray window carries the comparison's result, evaluated by the cell's owner (k_win_pack)
              const bool wall = P.wmode ? inl[(long)c * inl_stride] != 0u : (float)inl[(long)c * inl_stride] > Rt.f_wall;
              if (!(wall && m1.x < 1.0f)) {
                contrib = true; c_hit = 1u;
                c_dec = __double2ll_rn((double)edec * EM_SCALE_V);
                if (nz < m1.y || m1.z < 0.5f) c_key = ~float_ord(nz);
              }
            }
          }
        }
      }
    }
    const unsigned long long cm = __builtin_amdgcn_ballot_w64(contrib);
    if (!cm) return;                                                   // wave-uniform
    auto flush = [&](unsigned int cc, long long d_sum, unsigned int hits, unsigned int key) {
      if (hits) {
        atomicAdd(reinterpret_cast<unsigned long long*>(accr_dec(AR, cc)), (unsigned long long)d_sum);
        atomicAdd(accr_hits(AR, cc), hits);
      }
      if (key) { unsigned int* kp = accr_key(AR, cc); if (ray_key_load(kp) < key) atomicMax(kp, key); }     // (loading the key WITH the cell, ahead of the tests, measured no gain: 219 vs 221 us on the terrain)
    };
    // How the contributions of a batch go out.  With penetrations in it (or at least a handful of contributions) the wave combines
    // the visits of a cell in LDS first (below).  Upper bounds only -- the frames after clear(), a band a shift brought in: the visits
    // of one step sit in the queue in lane order, so the rays that share a cell are mostly NEIGHBOURS: a visit is dropped when the next
    // lane's lowers the same cell at least as far (the lowest of a run always goes out), the rest goes out directly.  Round 6: when
    // MANY neighbours share cells (a scan-ordered cloud: the rays of a wave travel together) the batch takes the LDS combination too --
    // the first frame of the terrain scene after clear() 0.89 -> 0.33 ms (5.4x -> 2.0x its steady pass); a uniform-random cloud, whose
    // rays share next to nothing, keeps the direct path (combining every batch cost it 5 % there).
#ifndef RAY_COMBINE_DUPS
#define RAY_COMBINE_DUPS 24   /* same box, 4 .. 32: first frame after clear() uniform 1.01 / 0.96 / 0.94 / 0.91 / 0.855 / 0.85 ms (never combining: 0.92), terrain 0.33-0.35 for all (never: 0.78-0.89); steady passes within 1-3 % */
#endif
    const unsigned int cn = (unsigned int)__shfl_down((int)c, 1, 64), kn = (unsigned int)__shfl_down((int)c_key, 1, 64);
    const bool same_next = contrib && lane < 63 && cn == c;
    const bool hits_in_batch = __builtin_amdgcn_ballot_w64(c_hit != 0u) != 0ull;
    const bool combine = __popcll(cm) >= 4 && (hits_in_batch || __popcll(__builtin_amdgcn_ballot_w64(same_next)) >= RAY_COMBINE_DUPS);      // (wave-uniform)
    if (!combine) {
      const bool covered = !c_hit && same_next && c_key <= kn;
      if (contrib && !covered) flush(c, c_dec, c_hit, c_key);
      return;
    }
    // slots: tag | key in the batch's qc entries, hits in its ql entries, the 64-bit sums in its qz entries (8-byte aligned: one word of slack)
    unsigned int* a_tag = qc + first;  unsigned int* a_key = a_tag + 32;  unsigned int* a_hit = ql + first;
    unsigned long long* a_dec = reinterpret_cast<unsigned long long*>(qz + ((first + 1) & ~1));
    __builtin_amdgcn_wave_barrier();                                   // (the batch was read into registers above)
    if (lane < 32) { a_tag[lane] = 0xffffffffu; a_key[lane] = 0u; a_hit[lane] = 0u; a_dec[lane] = 0ull; }
    __builtin_amdgcn_wave_barrier();
    const unsigned int slot = (c * 0x9E3779B1u) >> 27;
    if (contrib) a_tag[slot] = c;                                      // one of the cells that hash here wins the slot
    __builtin_amdgcn_wave_barrier();
    const bool member = contrib && a_tag[slot] == c;
    if (member) {
      if (c_hit) { atomicAdd(&a_dec[slot], (unsigned long long)c_dec); atomicAdd(&a_hit[slot], 1u); }
      if (c_key) atomicMax(&a_key[slot], c_key);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 32) { const unsigned int cc = a_tag[lane]; if (cc != 0xffffffffu) flush(cc, (long long)a_dec[lane], a_hit[lane], a_key[lane]); }
    if (contrib && !member) flush(c, c_dec, c_hit, c_key);
  };
  // ---- the march ----------------------------------------------------------------------------------------------------------
  // Measured on MI355X (tools/clockbench.hip, 8 waves per SIMD): a SIMD issues about ONE instruction per nanosecond whatever its
  // kind -- a scalar instruction costs as much as a vector one, a branch (taken or not) about four.  The loop is therefore built
  // to need almost no scalar instructions and one branch per FOUR steps:
  //  * a lane stops at its own last sample by clamping the step, s = min(s_k, s_end): beyond its range the sample stays in the cell
  //    it visited last, and the new-cell test (:209-210) then keeps the lane passive -- no step counter, no range compare (a lane
  //    without a ray sits in the sensor's cell from the start); row strips keep the explicit range test (kb > 0);
  //  * the bitmap word of a visit is requested for every lane (a passive lane reads the all-ones word behind the last row) and
  //    looked at one group of four steps LATER: four loads in flight per wave, no branch around them, one ballot + branch per group
  //    decides whether anything has to be queued at all;
  //  * the groups alternate between two register sets (no copy has to wait for a load in flight).
  auto push = [&](unsigned int w, unsigned int xy, float s) {      // bit iy & 31 clear: not (known + fresh), something may happen -> queue the visit
    const bool need = __builtin_amdgcn_ubfe(w, xy, 1u) == 0u;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(need);
    if (mask) {                                                 // wave-uniform
      if (need) {
        const int pos = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
        qc[pos] = xy; qz[pos] = s; ql[pos] = (unsigned int)lane;
      }
      qn += __popcll(mask);
      __builtin_amdgcn_wave_barrier();
      if (qn >= 64) { qn -= 64; work(qn, 64); __builtin_amdgcn_wave_barrier(); }
    }
  };
  constexpr int GU = 4;                                         // steps per group
  struct Group { unsigned int w[GU], xy[GU]; float s[GU]; };
  auto consume = [&](const Group& g) {
    unsigned int inert_all = 1u;                                // every visit of the group hit a (known + fresh) cell
#pragma unroll
    for (int u = 0; u < GU; ++u) inert_all &= __builtin_amdgcn_ubfe(g.w[u], g.xy[u], 1u);      // bit iy & 31 of the word
    if (__builtin_amdgcn_ballot_w64(inert_all == 0u) == 0ull) return;         // the common case: one branch per four steps
#pragma unroll
    for (int u = 0; u < GU; ++u) push(g.w[u], g.xy[u], g.s[u]);
  };
  typedef float v2f __attribute__((ext_vector_type(2)));
  typedef _Float16 v2h __attribute__((ext_vector_type(2)));
  const v2f txy = {T.t[0], T.t[1]};
  // loop constants that feed a second scalar operand slot live in vector registers (one scalar source per VALU instruction on
  // gfx9: the compiler would otherwise re-materialise them with a v_mov in every step)
  // (WIN: the word of cell (ix, iy) lies at ix * row bytes + (iy >> 5) * 4 + base_v with the window's origin folded into base_v -- an
  // ADD, v_lshl_add_u32, where the whole-map copy ORs its pitch-aligned base in: the same instruction count per step)
  unsigned int ones_off = lrows * lwpr32 * 4u + smap_base, base_v = WIN ? smap_base - ((unsigned int)LW.r0 * lwpr32 + (unsigned int)LW.w0) * 4u : smap_base,
               mask_v = (IDX == 2 && !STRIP) ? 0x1ffcu : 0x1ffffffcu;      // (PK: the shifted key still carries the row above bit 12)
  asm volatile("" : "+v"(ones_off), "+v"(base_v), "+v"(mask_v));
  auto cell_xy = [&](v2f n, int& ix, int& iy) -> unsigned int {                   // sample position -> cell, key (ix << 16) | iy   (cell_n <= 46340: 16 bits each)
    if constexpr (IDX == 2) {
      // both axes together: one packed conversion to half (v_cvt_pk_f16_f32), the two mixed-precision FMAs read its halves, one
      // packed add of the half width -- AxisIdx<0, 2>'s arithmetic, operation for operation
      const v2h h = __builtin_convertvector(n, v2h);
      const unsigned int hb = __builtin_bit_cast(unsigned int, h);
      float fx, fy;
      asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(fx) : "v"(hb), "s"(P.inv_res_f), "v"(frac_v));
      asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(fy) : "v"(hb), "s"(P.inv_res_f), "v"(frac_v));
      const v2f f = (v2f){__builtin_floorf(fx), __builtin_floorf(fy)} + (v2f){P.hw_int_f, P.hw_int_f};
      ix = (int)__builtin_amdgcn_fmed3f(f.x, 0.0f, P.cm1_f); iy = (int)__builtin_amdgcn_fmed3f(f.y, 0.0f, P.cm1_f);
    } else { ix = aidx(P, n.x); iy = aidx(P, n.y); }
    return ((unsigned int)ix << 16) | (unsigned int)iy;
  };
  // PK (round 5): the float formula on whole-map contexts finishes BOTH axes in packed 16-bit integer arithmetic -- floor + conversion in one
  // instruction per axis (v_cvt_flr_i32_f32), one saturating pack (v_cvt_pk_i16_i32), then + half width / max 0 / min C - 1 on the pair
  // (v_pk_add_i16 clamp, v_pk_max_i16, v_pk_min_i16): six instructions where floor x 2, packed add, v_med3_f32 x 2, conversion x 2 and
  // the shift-or that builds the key were eight, and the bitmap row is taken from the key's high half by v_mad_u32_u16 (op_sel).  Same
  // index for every finite coordinate: clamp(floor(v) + hw, 0, C - 1) with hw <= 16383 is unchanged by saturating floor(v) to int16 first
  // (a saturated value stays on its side of the clamp).  NaN samples do not occur (the rays of NaN points are never marched).
  constexpr bool PK = IDX == 2 && !STRIP;
  unsigned int hwhw_v = 0u, zero_v = 0u, cm1cm1_v = 0u;
  if constexpr (PK) {
    const unsigned int hw = (unsigned int)(int)P.hw_int_f, cm1 = (unsigned int)(C - 1);
    hwhw_v = (hw << 16) | hw; cm1cm1_v = (cm1 << 16) | cm1;
    asm volatile("" : "+v"(hwhw_v), "+v"(zero_v), "+v"(cm1cm1_v));
  }
  auto cell_key = [&](v2f n) -> unsigned int {                                    // PK only: sample position -> key (ix << 16) | iy
    const v2h h = __builtin_convertvector(n, v2h);
    const unsigned int hb = __builtin_bit_cast(unsigned int, h);
    float fx, fy;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(fx) : "v"(hb), "s"(P.inv_res_f), "v"(frac_v));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(fy) : "v"(hb), "s"(P.inv_res_f), "v"(frac_v));
    int fxi, fyi;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(fxi) : "v"(fx));
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(fyi) : "v"(fy));
    unsigned int k;
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(k) : "v"(fyi), "v"(fxi));            // low half: y, high half: x (signed saturation)
    asm("v_pk_add_i16 %0, %1, %2 clamp" : "=v"(k) : "v"(k), "v"(hwhw_v));
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(k) : "v"(k), "v"(zero_v));
    asm("v_pk_min_i16 %0, %1, %2" : "=v"(k) : "v"(k), "v"(cm1cm1_v));
    return k;
  };
  unsigned int last_xy = 0xffffffffu;                           // the cell of the lane's previous sample (no cell: the first sample always acts)
  float s_end = 0.f;                                            // the lane's last sample (0: none -- the lane then never leaves the sensor's cell)
  if (!STRIP) {
    if (ke > 0) s_end = sS[ke - 1];
    if (ke <= 0) { int ix0, iy0; rx = 0.f; ry = 0.f; if constexpr (PK) last_xy = cell_key(txy); else last_xy = cell_xy(txy, ix0, iy0); }
  }
  const v2f rxy_m = {rx, ry};
  int kg = STRIP ? ((wb / LPR) & ~(2 * GU - 1)) : 0;            // first (lane) step of the current group (multiple of 8: the step table is read as float4)
  const int we_l = (we + LPR - 1) / LPR;                         // lane steps: lane `sub` of a ray marches the samples LPR * k + sub
  auto step = [&](int k, float sk, unsigned int& w, unsigned int& xy_out, float& s_out) {
    float s = sk;
    unsigned int prev_xy = last_xy;                             // the cell of the previous sample
    int K = k;                                                  // the sample index
    if constexpr (LPR > 1) {                                    // several lanes per ray: own sample and its predecessor from the table, per lane
      K = LPR * k + sub;
      const int Kc = min(K, nSp - 1);
      s = sS[Kc];
      float sp = sS[max(Kc - 1, 0)];
      if (!STRIP) { asm("v_min_f32 %0, %1, %2" : "=v"(s) : "v"(s), "v"(s_end)); asm("v_min_f32 %0, %1, %2" : "=v"(sp) : "v"(sp), "v"(s_end)); }
      int ixp = 0, iyp = 0;
      unsigned int xyp;
      if constexpr (PK) xyp = cell_key(txy + rxy_m * sp); else xyp = cell_xy(txy + rxy_m * sp, ixp, iyp);
      if (!STRIP) prev_xy = K == 0 ? last_xy : xyp;             // (last_xy keeps its initial value here: none, or the sensor's cell for a lane without a ray)
      else prev_xy = ((unsigned int)(K - 1 - kb) < (unsigned int)(ke - kb)) ? xyp : 0xffffffffu;
    } else if (!STRIP) asm("v_min_f32 %0, %1, %2" : "=v"(s) : "v"(sk), "v"(s_end));
    int ixs = 0, iys = 0;
    unsigned int xy;                                                      // x, y of the sample (its height is only needed for queued visits)
    if constexpr (PK) { xy = cell_key(txy + rxy_m * s); if (STATS) { ixs = (int)(xy >> 16); iys = (int)(xy & 0xffffu); } }
    else xy = cell_xy(txy + rxy_m * s, ixs, iys);
    const unsigned int ix = (unsigned int)ixs, iy = (unsigned int)iys;
    // own sample & new cell (:209-210) [& owned by this strip]; border cells (:211) read as inert in the bitmap
    bool act;
    unsigned int brow = ix, bcol = iy;                          // bitmap row / column: the logical row ...
    if (STRIP) {
      const bool mine = (unsigned int)(K - kb) < (unsigned int)(ke - kb);
      brow = (unsigned int)(phys_row(P, (int)ix) - P.row0);     // ... or, on strips, the local physical row (also the ownership test)
      bcol = iy - (unsigned int)P.col0;                         // (0 on strips; a ray window starts at column col0, a multiple of 64: the bit inside the word stays iy & 31)
      act = mine & (xy != prev_xy) & (brow < (unsigned int)P.nrows) & (bcol < (unsigned int)P.ncols);
      if (LPR == 1) last_xy = mine ? xy : last_xy;
    } else {
      act = xy != prev_xy;
      if (LPR == 1) last_xy = xy;
    }
    if (STATS) visits += (act && max(ix - 1u, iy - 1u) < (unsigned int)(C - 2)) ? 1u : 0u;
    unsigned int colpart, off_a;                                // ((iy >> 3) & ~3) | LDS base: byte offset of the word within its row
    if constexpr (PK) {                                         // the key's low half is iy (the mask drops the ix bits), its high half the bitmap row
      if constexpr (WIN) {
        unsigned int wi;
        asm("v_bfe_u32 %0, %1, 5, 11" : "=v"(wi) : "v"(xy));                                     // iy >> 5: the word column
        asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(colpart) : "v"(wi), "v"(base_v));
      } else asm("v_and_or_b32 %0, %1, %3, %2" : "=v"(colpart) : "v"(xy >> 3), "v"(base_v), "v"(mask_v));
      asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(off_a) : "v"(xy), "s"(lwpr32 * 4u), "v"(colpart));
    } else {
      if constexpr (WIN) asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(colpart) : "v"(bcol >> 5), "v"(base_v));
      else asm("v_and_or_b32 %0, %1, %3, %2" : "=v"(colpart) : "v"(bcol >> 3), "v"(base_v), "v"(mask_v));      // (no VOP3 literals on gfx9: the mask is a register)
      off_a = mad24(brow, lwpr32 * 4u, colpart);
    }
    const unsigned int off = act ? off_a : ones_off;
    if (LMAP) w = *(const lds_u32*)(size_t)off;
    else w = *reinterpret_cast<const unsigned int*>(reinterpret_cast<const char*>(inert) + off);
    xy_out = xy; s_out = s;
  };
  Group gA, gB;
#pragma unroll
  for (int u = 0; u < GU; ++u) { gA.w[u] = ~0u; gA.xy[u] = 0u; gA.s[u] = 0.f; gB.w[u] = ~0u; gB.xy[u] = 0u; gB.s[u] = 0.f; }
  for (; kg < we_l; kg += 2 * GU) {                             // (steps past a lane's range request nothing; the table is padded by 8 entries)
    const float4 s0 = *reinterpret_cast<const float4*>(sS + kg), s1 = *reinterpret_cast<const float4*>(sS + kg + GU);   // wave-uniform reads
    step(kg + 0, s0.x, gA.w[0], gA.xy[0], gA.s[0]); step(kg + 1, s0.y, gA.w[1], gA.xy[1], gA.s[1]);
    step(kg + 2, s0.z, gA.w[2], gA.xy[2], gA.s[2]); step(kg + 3, s0.w, gA.w[3], gA.xy[3], gA.s[3]);
    consume(gB);
    step(kg + 4, s1.x, gB.w[0], gB.xy[0], gB.s[0]); step(kg + 5, s1.y, gB.w[1], gB.xy[1], gB.s[1]);
    step(kg + 6, s1.z, gB.w[2], gB.xy[2], gB.s[2]); step(kg + 7, s1.w, gB.w[3], gB.xy[3], gB.s[3]);
    consume(gA);
  }
  consume(gB);
  __builtin_amdgcn_wave_barrier();
  if (qn > 0) work(0, qn);
  if (STATS) {
    visits = (unsigned long long)wave_sum_ll((long long)visits);
    if ((threadIdx.x & 63) == 0 && visits) atomicAdd(&F->ray_visits, visits);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Phase D: per-cell commit of ray effects + average_map_kernel (custom_kernels.py:348-389) + drift shift
// materialisation (elevation_mapping.py:357) + accumulator re-arm (replaces `new_map *= 0`, :327).
// Streaming: reads 32+40(+16) B, writes 32 B (+zeroes) per cell.
// ---------------------------------------------------------------------------------------------------------
template <bool COMMITTED, bool RAYS>
__global__ __launch_bounds__(EM_BLOCK) void k_average(KP P, Cells cells, AccF* __restrict__ acc,
                                                       AccR* __restrict__ accr, const FrameDev* __restrict__ F,
                                                       unsigned int* __restrict__ cnt_out, OverlapArgs O) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  long c = li + (long)P.halo * P.C;
  Cell m = cells[c];
  AccF a = acc[c];
  if (!COMMITTED) {
    if (P.mv.n) { const int lrow = (int)(li / P.C); cell_now(P, m, P.row0 + lrow, (int)(li - (long)lrow * P.C)); }     // pending map shifts
    m.h += F->shift; commit_cell(P, m, a);
  }
  if (RAYS) {
    AccR r = accr[c];
    if (r.hits) { m.valid = m.valid + (float)((double)r.dec / EM_SCALE_V); m.v = m.v + P.ov_f * (float)r.hits; }
    if (r.upper_key) { m.upper = ord_float(~r.upper_key); m.is_upper = 1.0f; }
    if (r.hits | r.upper_key) { AccR z = {0, 0u, 0u}; accr[c] = z; }
  }
  if (cnt_out) cnt_out[c] = (unsigned int)(a.cnt_out & 0xffffffffull);   // survives for the semantic fusion (new_elmap plane 2)
  average_cell(P, m, a);
  if (O.on) {                                       // clear_overlap_map (:372-375) rides on this rewrite (whole frames; staged API: k_overlap)
    const int lrow = (int)(li / P.C);
    if (overlap_window(O, logi_row(P, P.row0 + lrow), logi_col(P, (int)(li - (long)lrow * P.C)))) overlap_cell(P, O, m);
  }
  cells[c] = m;
  if (a.pts_inl | a.cnt_out) { AccF z = {0ull, 0ull, 0ll, 0ll, 0ull}; acc[c] = z; }
}

// ---------------------------------------------------------------------------------------------------------
// Robot scale (round 5): phases A, A', B and B' + D of a small frame in ONE launch.
// The configuration the reference ships (202^2 cells, ~50 k points per cloud: parameter.py:137,165) is neither bandwidth nor
// issue bound here: its frame is a chain of dependent launches of 2-4 us of work each, and every launch costs ~4.5 us of dispatch +
// drain on this stack.  k_small_frame runs count -> gate -> fuse -> commit + average as ONE grid with two grid-wide barriers in
// between (emap_device.h: sf_arrive / sf_decide_last / sf_wait_decision):
//   * a thread keeps ITS point (geometry, cell, the cell's hot half) in registers from the count to the fuse phase: the cloud is read
//     and transformed once per frame instead of twice;
//   * what one phase writes and the next reads on ANOTHER XCD (per-cell counts, the accumulators, the shift) only ever moves through
//     device-scope atomics and device-coherent (sc1) loads / stores -- the XCDs' L2s are not coherent with each other inside a launch.
//     Same hand-off as last_block_ticket: stores acknowledged (s_waitcnt), workgroup barrier, ticket; see the note there;
//   * the arithmetic is k_count's, k_fuse's and k_average's, statement for statement: the accumulators are integers, so the frame is
//     bit-identical to the chain of launches (tests/test_hip_small_frame.py), which stays as the staged API, as the path of larger
//     maps / clouds, of frames with a visibility pass or a declared semantic fusion, and as the way a frame is RE-RUN after an abort.
// Round 6 -- a barrier can no longer leave the map undefined.  The grid fits the device four times over, but it is not a cooperative
// launch: while another process' kernels hold the CUs, part of this grid may wait at a barrier for workgroups that have not started.
// A waiter that runs out of patience ABORTS the barrier for the whole grid, consistently (one compare-and-swap decides between
// "released" and "aborted"): every workgroup -- those that only start afterwards included -- then leaves at that barrier, and the LAST
// one to arrive there (every other workgroup's atomics are acknowledged by then, nobody writes any more) puts things back: the frame
// accumulators and the error slots to zero (what every launch finds), the frame record to what the gate found.  No cell is written
// before the second barrier has passed: after an abort the map, the accumulators and the drift record are bit for bit what the
// launch found.  The aborting launch also raises a device-side POISON word: the k_small_frame launches already queued behind it
// (frames may be pipelined) find it and leave at once, so no later frame is fused onto a map that lacks an earlier one.  Two
// host-mapped words keep the host informed -- [0] the epoch of the last launch whose second barrier passed, [1] the epoch of the first
// aborted launch -- and the host re-runs the aborted frame and every small frame issued after it, in order, on the chain of
// launches, before anything else looks at the map (emap_api.hip: sf_settle / sf_recover).
// ---------------------------------------------------------------------------------------------------------
struct SmallFrame {
  GateArgs A; FrameDev* F; FrameDev* F_save; ErrSlot* slots;
  unsigned int* sync;        // two sets of ticket words (1024 apart), zero between launches
  unsigned int* flag;        // 64-bit release words: [0..1] barrier 1 {epoch [| SF_ABORT], that frame's shift}; [32..33] barrier 2
  unsigned int* host;        // host-mapped: [0] epoch of the last launch whose second barrier passed, [1] epoch of the first aborted launch (0: none)
  unsigned int* poison;      // device word, non-zero: an earlier launch was aborted and the host has not re-run it yet -- do nothing
  unsigned int epoch;        // distinct per launch, 1 .. 2^31 - 1
  unsigned int spin_limit;   // polls before a waiter gives up
  int test_abort;            // test hook: workgroup 0 gives up at once at barrier 1 / 2 (0: never)
};
__device__ __forceinline__ unsigned long long ld_dev(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_dev(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ AccF acc_load_dev(const AccF* a) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(a);
  AccF r; r.pts_inl = ld_dev(q); r.cnt_out = ld_dev(q + 1); r.sum_h = (long long)ld_dev(q + 2); r.sum_v = (long long)ld_dev(q + 3); r.latest = ld_dev(q + 4);
  return r;
}
template <int MODE>
__global__ __launch_bounds__(EM_BLOCK) void k_small_frame(KP P, Pose T, const float* __restrict__ pts, long n, int stride, Cells cells,
                                                           AccF* __restrict__ acc, unsigned int* __restrict__ cnt_out,
                                                           OverlapArgs O, SmallFrame S) {
  __shared__ bool s_last;
  __shared__ unsigned long long s_word;
  const unsigned int poisoned = __hip_atomic_load(S.poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (written by an EARLIER launch: the same for every workgroup; needed in front of the first atomic)
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;          // one point per thread (the host launches at least n threads)
  // ---- phase A: k_count ------------------------------------------------------------------------------------------------------
  long c = -1;
  float gz = 0.f, gv = 0.f;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  long long e_fix = 0;
  unsigned int inl = 0;
  if (i < n) {
    float rx, ry, rz;
    load_point(pts, i, stride, rx, ry, rz);
    const Geo g = geometry<MODE>(P, T, rx, ry, rz);
    const Owned oc = owned(P, g.ix, g.iy);
    c = (g.finite && g.valid && g.inside) ? oc.c : -1;
    gz = g.z; gv = g.v;
    if (c >= 0) {
      m = cells.hot[c];   // h, v, valid, trav
      cell_now(P, m, oc.prow, oc.pcol);
      const bool inlier = m.z > 0.5f && (double)fabsf(m.x - gz) < (double)m.y * P.mt && (double)m.y < P.dcvi_half &&
                          (double)m.w > P.trav_inlier;
      if (inlier) { inl = 1; e_fix = __double2ll_rn((double)(gz - m.x) * EM_SCALE_E); }
      if (poisoned) return;                                           // (uniform over the grid)
      atomicAdd(&acc[c].pts_inl, 1ull | ((unsigned long long)inl << 32));
    }
  }
  if (poisoned) return;
  if (__any(inl)) {
    const long long s = wave_sum_ll(e_fix);
    const unsigned long long k = __popcll(__ballot(inl));
    if ((threadIdx.x & 63) == 0) {
      const unsigned int slot = (blockIdx.x * (EM_BLOCK / 64) + (threadIdx.x >> 6)) & (EM_ERR_SLOTS - 1);
      atomicAdd(reinterpret_cast<unsigned long long*>(&S.slots[slot].sum), (unsigned long long)s);
      atomicAdd(&S.slots[slot].cnt, k);
    }
  }
  // an aborted barrier, in the LAST workgroup to arrive at it: every accumulator word and every error slot back to zero, and the poison
  // word raised for the launches queued behind this one
  auto wipe = [&]() {
    if (threadIdx.x == 0) __hip_atomic_store(S.poison, S.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long nall = (long)(P.nrows + 2 * P.halo) * P.C;
    for (long k = threadIdx.x; k < nall * 5; k += EM_BLOCK) st_dev(reinterpret_cast<unsigned long long*>(acc) + k, 0ull);
    for (int k = threadIdx.x; k < EM_ERR_SLOTS; k += EM_BLOCK) { st_dev(reinterpret_cast<unsigned long long*>(&S.slots[k].sum), 0ull); st_dev(&S.slots[k].cnt, 0ull); }
  };
  // ---- barrier 1; the last workgroup to arrive is the drift gate (k_gate) ------------------------------------------------------------
  // It releases the others WITH the shift -- one 8-byte word {epoch, shift} -- as soon as it has the slot sums, and does the gate's
  // bookkeeping (frame record, additive_mean_error, slots re-armed: nothing anybody reads in this launch) afterwards: a separate shift
  // word cost two more dependent trips to the memory side per frame (its acknowledgement before the release, its load after the wait).
  unsigned long long* const rel1 = reinterpret_cast<unsigned long long*>(S.flag);
  unsigned long long* const rel2 = reinterpret_cast<unsigned long long*>(S.flag + 32);
  const bool last1 = sf_arrive(S.sync, &s_last);                     // (this workgroup's own phase-A results were acknowledged before it took its ticket)
  if (last1) {
    if (threadIdx.x < 64) {
      const float sh = gate_shift_only(S.A, S.slots, (int)threadIdx.x);
      unsigned long long w = 0ull;
      if (threadIdx.x == 0) { w = sf_decide_last(rel1, S.epoch, __float_as_uint(sh)); s_word = w; }
      w = __shfl(w, 0, 64);
      if (!((unsigned int)w & SF_ABORT)) {
        // the frame record as the gate finds it: what an abort of the SECOND barrier puts back (device-coherent: read by another workgroup)
        if (threadIdx.x < (int)(sizeof(FrameDev) / 8)) st_dev(reinterpret_cast<unsigned long long*>(S.F_save) + threadIdx.x, reinterpret_cast<const unsigned long long*>(S.F)[threadIdx.x]);
        gate_eval(S.A, S.slots, S.F, (int)threadIdx.x, 0, nullptr, nullptr);
      }
    }
  } else if (threadIdx.x == 0) s_word = sf_wait_decision(rel1, S.epoch, S.spin_limit, S.test_abort == 1 && blockIdx.x == 0, S.host + 1, S.epoch);
  __syncthreads();
  const unsigned long long w1 = s_word;
  if ((unsigned int)w1 & SF_ABORT) { if (last1) wipe(); return; }    // (uniform over the GRID: one compare-and-swap decided)
  const float shift = __uint_as_float((unsigned int)(w1 >> 32));
  // ---- phase B: k_fuse against snapshot S0 ---------------------------------------------------------------------------------------
  if (c >= 0) {
    unsigned long long* const a = reinterpret_cast<unsigned long long*>(acc + c);      // pts_inl, cnt_out, sum_h, sum_v, latest
    const float map_h = m.x + shift, map_v = m.y;
    const unsigned int n_pts = (unsigned int)(ld_dev(a) & 0xffffffffull);
    const float num_points = (float)n_pts;
    const bool single = n_pts == 1u;                                 // a single writer: stores instead of atomics
    if ((double)fabsf(map_h - gz) > (double)map_v * P.mt) {          // outlier :173-175
      if (single) st_dev(a + 1, 1ull << 32); else atomicAdd(a + 1, 1ull << 32);
    } else if (!(P.edge && (double)num_points > P.wall &&
                 (double)gz < (double)map_h - (double)map_v * P.mt / (double)num_points)) {   // edge sharpening :177-179
      const float new_h = (map_h * gv + gz * map_v) / (map_v + gv);          // :181-182
      const float new_v = (map_v * gv) / (map_v + gv);
      const long long fh = __double2ll_rn((double)new_h * EM_SCALE_H), fv = __double2ll_rn((double)new_v * EM_SCALE_V);
      const unsigned long long lt = ((unsigned long long)(i + 1) << 32) | (unsigned long long)__float_as_uint(new_h);
      if (single) { st_dev(a + 1, 1ull); st_dev(a + 2, (unsigned long long)fh); st_dev(a + 3, (unsigned long long)fv); st_dev(a + 4, lt); }
      else {
        atomicAdd(a + 2, (unsigned long long)fh);
        atomicAdd(a + 3, (unsigned long long)fv);
        atomicAdd(a + 1, 1ull);
        atomicMax(a + 4, lt);
      }
    }
  }
  // ---- barrier 2 -------------------------------------------------------------------------------------------------------------------
  const bool last2 = sf_arrive(S.sync + 1024, &s_last);
  if (threadIdx.x == 0)
    s_word = last2 ? sf_decide_last(rel2, S.epoch, 0u) : sf_wait_decision(rel2, S.epoch, S.spin_limit, S.test_abort == 2 && blockIdx.x == 0, S.host + 1, S.epoch);
  __syncthreads();
  if ((unsigned int)s_word & SF_ABORT) {                             // (uniform over the grid)
    if (last2) {                                                      // every other workgroup is through its phase B -- and through the gate's bookkeeping
      wipe();
      if (threadIdx.x < (int)(sizeof(FrameDev) / 8))
        reinterpret_cast<unsigned long long*>(S.F)[threadIdx.x] = ld_dev(reinterpret_cast<const unsigned long long*>(S.F_save) + threadIdx.x);
    }
    return;
  }
  if (last2 && threadIdx.x == 0) __hip_atomic_store(S.host, S.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // the frame WILL be applied: the host may forget it
  // ---- per cell: k_average<false, false> -- commit + average + overlap clearing + re-arm ---------------------------------------------
  const long ncell = (long)P.nrows * P.C, gstride = (long)gridDim.x * EM_BLOCK;
  for (long li = i; li < ncell; li += gstride) {
    const long cc = li + (long)P.halo * P.C;
    Cell q = cells[cc];
    const AccF a = acc_load_dev(acc + cc);
    const int lrow = (int)(li / P.C), pcol = (int)(li - (long)lrow * P.C);
    if (P.mv.n) cell_now(P, q, P.row0 + lrow, pcol);               // pending map shifts
    q.h += shift; commit_cell(P, q, a);
    if (cnt_out) cnt_out[cc] = (unsigned int)(a.cnt_out & 0xffffffffull);
    average_cell(P, q, a);
    if (O.on && overlap_window(O, logi_row(P, P.row0 + lrow), logi_col(P, pcol))) overlap_cell(P, O, q);
    cells[cc] = q;
    if (a.pts_inl | a.cnt_out) { AccF z = {0ull, 0ull, 0ll, 0ll, 0ull}; acc[cc] = z; }
  }
}

// Applies the effects of the visibility pass when the tile kernel has already committed AND averaged the frame (binned path):
// only cells that are not fused this frame can carry ray effects (a fused cell is known and fresh: every ray skips it), so this is
// a 16-byte stream over the ray accumulators with a read-modify-write of the few touched cells: validity decrement + variance
// inflation (custom_kernels.py:251-252), upper bound (:230-233, :254-255), then average_map_kernel's reset of cells whose
// validity fell below 0.5 (:380-384); re-arms the accumulators.
__global__ __launch_bounds__(EM_BLOCK) void k_ray_apply(KP P, Cells cells, AccR* __restrict__ accr,
                                                        unsigned long long* __restrict__ inert, OverlapArgs O, FrameDev* __restrict__ F,
                                                        unsigned int* __restrict__ ray_pref_host, int par) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  const long words = (long)P.nrows * ((P.C + 63) / 64);
  if ((long)blockIdx.x * EM_BLOCK < words) {                         // (uniform per workgroup) the rays are done with the bitmap: count its bits, leave it zeroed for the tile kernel's ORs
    __shared__ unsigned int s_q;
    if (threadIdx.x == 0) s_q = 0u;
    __syncthreads();
    unsigned int q = 0u;
    if (li < words) { q = (unsigned int)__popcll(inert[li]); inert[li] = 0ull; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += (unsigned int)__shfl_xor((int)q, o, 64);
    if ((threadIdx.x & 63) == 0 && q) atomicAdd(&s_q, q);
    __syncthreads();
    if (threadIdx.x == 0 && s_q) atomicAdd(&F->quiet_sum[par & 1], s_q);
  }
  if (li == 0) {                                                     // the PREVIOUS launch's finished count -> which ray kernel the next frames use (FrameDev)
    const unsigned int q = F->quiet_sum[(par & 1) ^ 1];
    F->quiet_sum[(par & 1) ^ 1] = 0u;
    const unsigned int cls = (unsigned long long)q * 10ull < (unsigned long long)P.nrows * (unsigned long long)P.C * 3ull ? 1u : 0u;      // fewer than 30 % quiet
    // (q = 0: no finished count yet -- a real one holds at least the border cells)
    if (q && ray_pref_host && cls != F->ray_class) { F->ray_class = cls; __hip_atomic_store(ray_pref_host, cls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
  }
  if (li >= (long)P.nrows * P.C) return;
  long c = li + (long)P.halo * P.C;
  const AccR r = accr[c];
  bool win = false;                                                  // clear_overlap_map follows the averaging (:372-375): centred window
  if (O.on) { const int lrow = (int)(li / P.C); win = overlap_window(O, logi_row(P, P.row0 + lrow), logi_col(P, (int)(li - (long)lrow * P.C))); }
  if (!(r.hits | r.upper_key) && !win) return;
  Cell m = cells[c];
  bool ch = false;
  if (r.hits | r.upper_key) {
    if (r.hits) { m.valid = m.valid + (float)((double)r.dec / EM_SCALE_V); m.v = m.v + P.ov_f * (float)r.hits; }
    if (r.upper_key) { m.upper = ord_float(~r.upper_key); m.is_upper = 1.0f; }
    if (m.valid < 0.5f) { m.h = 0.f; m.v = P.init_var; m.valid = 0.f; }
    AccR z = {0, 0u, 0u}; accr[c] = z;
    ch = true;
  }
  if (win) ch = overlap_cell(P, O, m) || ch;
  if (ch) cells[c] = m;
}

// ---------------------------------------------------------------------------------------------------------
// Rays by ray on row strips (multi-GPU frames, emap_api_comm.hip: rays_by_ray).  Every ray starts at the sensor, so the strips around it
// march what the whole map marches -- row strips do not scale the visibility pass (measured: 1.02x at 1024^2, 1.34x at 4096^2 on 8
// ranks).  Instead every rank marches the rays of ITS points (those whose end cell lies in its rows: 1 / G of a uniform cloud, already
// tile sorted) over a replicated copy of the RAY WINDOW -- the (2 max_ray_length / resolution)^2 cells around the sensor that any ray
// can reach -- and the effects are reduced back to the owners of the rows.  Exactly the same visits as the row march, every effect an
// order-independent integer accumulation: bit-identical results.
//   k_win_pack     the owner of a window row copies its cells (hot, cold with w := quiet bit of S1 from its inert bitmap), normals
//                  and inlier counts into the window buffer (logical coordinates: independent of the circular origin); all other
//                  rows stay zero, an integer all-reduce (x + 0 + ... + 0: exact) then replicates the window
//   k_win_prepare  every rank: inert bitmap (one wave ballot per 64 columns) + 8 x 8 block thresholds of the window, with the
//                  definitions of k_tile_fuse<true, true> evaluated on the gathered cells (below: why the post-average cell suffices)
//   k_win_unpack   after the all-reduce of the effects: the owners move their rows into their AccR records (k_ray_apply follows)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_win_pack(KP P, Win W, Cells cells, const float* __restrict__ normal, long plane_stride,
                                                       const unsigned int* __restrict__ inl_plane, const unsigned long long* __restrict__ inert, float f_wall) {
  const long k = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= (long)W.nr * W.nc) return;
  const int wr = (int)(k / W.nc), wc = (int)(k - (long)wr * W.nc), lr = W.r0 + wr, lc = W.c0 + wc;
  if (lr >= P.C || lc >= P.C) return;
  const int prow = phys_row(P, lr), rel = prow - P.row0;
  if (rel < 0 || rel >= P.nrows) return;                                    // another rank's row
  const int pcol = phys_col(P, lc);
  const long c = (long)(rel + P.halo) * P.C + pcol;
  const float4 h = cells.hot[c], cd = cells.cold[c];
  const unsigned long long word = inert[(long)bitmap_row(P, prow) * ((P.C + 63) / 64) + (lc >> 6)];   // bitmap: LOGICAL column, local row
  const bool quiet = (word >> (lc & 63)) & 1ull;
  float n0 = 0.f, n1 = 0.f, n2 = 0.f;                                       // the normal planes keep the origin they were written with (k_rays)
  const long cn = normal_index(P, rel, lr, lc);
  if (cn >= 0) { n0 = normal[cn]; n1 = normal[plane_stride + cn]; n2 = normal[2 * plane_stride + cn]; }
  // the tests the march makes on (valid, is_upper, inlier count) travel as bits: !(x < 0.5) keeps what `x < 0.5f` decides (NaN included),
  // and the wall test n_inl > wall_num_thresh (custom_kernels.py:248) is evaluated here, by the owner
  const unsigned int flags = (!(h.z < 0.5f) ? 1u : 0u) | (!(cd.z < 0.5f) ? 2u : 0u) | (quiet ? 4u : 0u) | ((float)inl_plane[c] > f_wall ? 8u : 0u);
  uint4* rec = reinterpret_cast<uint4*>(W.rec) + 2 * k;
  rec[0] = make_uint4(__float_as_uint(h.x), __float_as_uint(h.y), __float_as_uint(cd.x), __float_as_uint(cd.y));
  rec[1] = make_uint4(__float_as_uint(n0), __float_as_uint(n1), __float_as_uint(n2), flags);
}
// One workgroup = 8 window rows x 64 columns.  quiet = the bit the owner's tile kernel derived from snapshot S1.  The visit threshold
// of a cell that is NOT quiet is a function of (valid, h, upper, is_upper), and for such a cell the averaged state the window holds
// equals S1 in those fields: it was not fused this frame (a fused cell is known and fresh, i.e. quiet), so commit only touched its
// variance and the averaging pass left it alone or reset an already unknown cell's (h, v) -- neither enters the threshold of an
// unknown cell.  Cells beyond the map are inert.
__global__ __launch_bounds__(512) void k_win_prepare(Win W, int C) {
  __shared__ unsigned int s_thr[8], s_other[8];
  const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6, wr = blockIdx.y * 8 + tr, wc = blockIdx.x * 64 + tc;
  if (threadIdx.x < 8) { s_thr[threadIdx.x] = 0u; s_other[threadIdx.x] = 0u; }
  __syncthreads();
  const long k = (long)wr * W.nc + wc;
  bool quiet = true, other = false;
  float visit_thr = -INFINITY;
  {   // expand the travelled record into the arrays k_rays addresses (hot / cold half cells, normal planes, the wall flag)
    const uint4 a = reinterpret_cast<const uint4*>(W.rec)[2 * k], b = reinterpret_cast<const uint4*>(W.rec)[2 * k + 1];
    const long wn = (long)W.nr * W.nc;
    W.hot[k] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), (b.w & 1u) ? 1.0f : 0.0f, 0.0f);
    W.cold[k] = make_float4(__uint_as_float(a.z), __uint_as_float(a.w), (b.w & 2u) ? 1.0f : 0.0f, (b.w & 4u) ? 1.0f : 0.0f);
    W.normal[k] = __uint_as_float(b.x); W.normal[wn + k] = __uint_as_float(b.y); W.normal[2 * wn + k] = __uint_as_float(b.z);
    W.inl[k] = (b.w >> 3) & 1u;
  }
  if (W.r0 + wr < C && W.c0 + wc < C) {
    const float4 h = W.hot[k], cd = W.cold[k];
    quiet = cd.w != 0.0f;
    if (!quiet) {
      visit_thr = h.z < 0.5f ? ((cd.z < 0.5f || !(cd.y <= 3.0e38f)) ? INFINITY : cd.y) : h.x + 0.05f;
      if (!(visit_thr >= -INFINITY)) visit_thr = INFINITY;
      other = !(h.z < 0.5f && cd.z < 0.5f);
    }
  }
  const unsigned long long bits = __ballot(quiet);
  if (tc == 0) W.bits[(long)wr * (W.nc >> 6) + blockIdx.x] = bits;
  unsigned int o = float_ord(visit_thr);
  o = max(o, (unsigned int)__shfl_xor((int)o, 1, 64)); o = max(o, (unsigned int)__shfl_xor((int)o, 2, 64)); o = max(o, (unsigned int)__shfl_xor((int)o, 4, 64));
  const unsigned long long ob = __ballot(other);
  if ((tc & 7) == 0) { atomicMax(&s_thr[tc >> 3], o); if ((ob >> tc) & 0xffull) s_other[tc >> 3] = 1u; }
  __syncthreads();
  if (threadIdx.x < 8) {
    float bt = ord_float(s_thr[threadIdx.x]);
    if (bt == INFINITY && s_other[threadIdx.x]) bt = 3.4028234664e38f;       // +INF only for virgin blocks (k_tile_fuse)
    W.thr[(long)blockIdx.y * (W.nc >> 3) + blockIdx.x * 8 + threadIdx.x] = bt;
  }
}
__global__ __launch_bounds__(EM_BLOCK) void k_win_unpack(KP P, Win W, AccR* __restrict__ accr) {
  const long k = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= (long)W.nr * W.nc) return;
  const long long dec = W.dh[2 * k], hits = W.dh[2 * k + 1];
  const unsigned int key = W.key[k];
  if (!(dec | hits | (long long)key)) return;
  const int wr = (int)(k / W.nc), wc = (int)(k - (long)wr * W.nc), lr = W.r0 + wr, lc = W.c0 + wc;
  if (lr >= P.C || lc >= P.C) return;
  const int rel = phys_row(P, lr) - P.row0;
  if (rel < 0 || rel >= P.nrows) return;
  AccR r; r.dec = dec; r.hits = (unsigned int)hits; r.upper_key = key;
  accr[(long)(rel + P.halo) * P.C + phys_col(P, lc)] = r;
}

// Effects of a by-ray frame reduced TO THE OWNERS (round 6): `parts` slabs of {dec, hits} pairs and keys, received from the other
// ranks for `cells` consecutive window cells this rank owns, are folded into the rank's own slab -- integer sums and a maximum, the
// order of the parts does not matter.  Part j's pairs start at dh_parts + j * part_stride pairs, its keys at key_parts + j * part_stride.
__global__ __launch_bounds__(EM_BLOCK) void k_win_reduce(long long* __restrict__ dh, unsigned int* __restrict__ key, const long long* __restrict__ dh_parts,
                                                         const unsigned int* __restrict__ key_parts, int parts, long part_stride, long off, long cells) {
  const long k = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= cells) return;
  long long d = dh[2 * k], h = dh[2 * k + 1];
  unsigned int ky = key[k];
  for (int j = 0; j < parts; ++j) {
    const long q = (long)j * part_stride + off + k;
    d += dh_parts[2 * q]; h += dh_parts[2 * q + 1];
    ky = max(ky, key_parts[q]);
  }
  dh[2 * k] = d; dh[2 * k + 1] = h; key[k] = ky;
}

// clear_overlap_map (elevation_mapping.py:393-410): centred window, one launch instead of ~12
__global__ __launch_bounds__(EM_BLOCK) void k_overlap(KP P, Cells cells, int cmin, int cmax, float hmin, float hmax) {
  int w = cmax - cmin;
  long k = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= (long)w * w) return;
  int ix = cmin + (int)(k / w), iy = cmin + (int)(k % w);
  long c = owned_cell(P, ix, iy);
  if (c < 0) return;
  Cell m = cells[c];
  const OverlapArgs O = {1, cmin, cmax, 0, hmin, hmax};
  if (overlap_cell(P, O, m)) cells[c] = m;
}

// (The 12 x 9 taps are explicit fma chains in a fixed order; the reference's cuDNN summation order is unspecified, tolerance 1e-5.)
struct TravW { float w[3][9][4]; float wo[3][4]; };   // weights of the traversability filter (traversability_filter.py:8-47) as kernargs (SGPRs): [filter][tap][channel]

// ---------------------------------------------------------------------------------------------------------
// k_post = dilation -> traversability filter + normals in ONE launch (elevation_mapping.py:376-391).  The dilated
// plane only ever feeds these two stencils, so the tile (+3 halo) of dilated values is produced in LDS from a raw
// (value, mask) tile (+3+d halo) and consumed in place; `traversability_input` is still written (interior only)
// because it is a readable attribute of the reference class.
// ---------------------------------------------------------------------------------------------------------
#define PT_C 64
#define POST_KW 2               /* (row, column) pairs of the walk per thread whose loads are in flight together, next to the rows' */
#ifndef POST_T32
#define POST_T32 512   /* threads of a 32-row stencil tile: 8 waves, four output rows per thread, two workgroups per CU */
#endif
// PT_R = tile height: 16 for large maps (less halo amplification), 4 for small maps (4x more workgroups: a robot-scale
// 200^2 map has only 52 tiles of 16 rows and the kernel time is then one workgroup's latency chain).
// Rows are LOGICAL map rows here (the stencils are defined on the logical map; a tile never straddles the circular seam because
// the launcher hands over logical row intervals [seg_b, seg_e)): local_row(phys_row(.)) / phys_col(.) place a cell in memory.
// STAGE 0: everything; 1: dilation only (traversability_input), the separately callable stage of the parity tests.
// Up to four logical row intervals per launch (a strip's rows around the circular seam, the boundary rows of a strip): a launch of a
// few tiles alone costs a whole workgroup latency chain (~18 us measured), so the pieces go into ONE grid.
struct PostSegs { int n, b[4], e[4], t0[4]; unsigned int emagic; };     // interval [b, e) starts at tile row t0 of the grid; emagic = ceil(2^32 / (6 + 2d))
// Epilogue arithmetic of the stencil kernel.  The NORMALS feed a decision of the next frame's visibility pass (half rounding, then
// |r . n| < cleanup_cos_thresh, custom_kernels.py:243-246), so their epilogue uses IEEE division and square root exactly like
// normal_filter_kernel (custom_kernels.py:493-500) and the oracle: bit-identical planes, tests/test_hip_normals_exact.py.  (Round 2
// used 1-ulp sequences there.  An exhaustive search over all 2^32 numerators showed the 3-instruction constant division
// a * (1/res) + residual correct only for 1e-32 < |a| < 1e37, and guarding that range costs what the sequence saves.)
// correctly rounded sqrt for x >= 1 (or +inf / NaN): v_sqrt_f32 is within 1 ulp, the two residuals pick the neighbour when it is the
// nearer one -- the compiler's own IEEE sequence (sqrtf) without its input scaling for x < 2^-96 and its zero / infinity class test,
// neither of which can apply here (x = nx^2 + ny^2 + 1; for x = inf every comparison below is false and inf stays).
// NB __fsqrt_rn is NOT this: it lowers to the bare 1-ulp instruction.
__device__ __forceinline__ float sqrt_rn_ge1(float x) {
  float s = __builtin_amdgcn_sqrtf(x);
  const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
  const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
  s = rd <= 0.0f ? sd : s;
  s = ru > 0.0f ? su : s;
  return s;
}
// exp(-a) of the traversability epilogue (traversability_filter.py:44, torch.exp in the reference), a >= 0.  Built from operations
// that exist bit for bit on the host as well -- round-to-nearest-even, fused multiply-adds, ldexp -- so that the oracle evaluates the
// SAME function (the CPU checker restates this sequence literally) and the traversability plane, which feeds the drift-inlier decision of the next
// frame (custom_kernels.py:329: traversability > traversability_inlier), compares bit for bit: n = rint(x log2 e), r = x - n ln 2
// (two-constant reduction), e^r by the degree-6 Taylor polynomial (|r| <= 0.347: truncation 1.2e-7 relative), 2^n by ldexp.  Within
// 3 ulp of expf; the hardware exponential (v_exp_f32) is faster by 8 instructions per cell but not reproducible off the GPU.
__device__ __forceinline__ float exp_neg(float a) {
  const float x = -(!(a > 200.0f) ? a : 200.0f);                         // exp(-200) = 0 in fp32; NaN stays NaN
  const float n = __builtin_rintf(x * 0x1.715476p+0f);
  float r = __builtin_fmaf(n, -0x1.62e400p-1f, x);
  r = __builtin_fmaf(n, -0x1.7f7d1cp-20f, r);
  float p = 0x1.6c16c2p-10f;
  p = __builtin_fmaf(p, r, 0x1.111112p-7f);
  p = __builtin_fmaf(p, r, 0x1.555556p-5f);
  p = __builtin_fmaf(p, r, 0x1.555556p-3f);
  p = __builtin_fmaf(p, r, 0.5f);
  p = __builtin_fmaf(p, r, 1.0f);
  p = __builtin_fmaf(p, r, 1.0f);
  return __builtin_amdgcn_ldexpf(p, (int)n);
}

// One output cell of the fused stencils: traversability_input (the dilated value), the traversability filter and the normal.
// t0 = the cell's dilated value inside an LDS plane with element stride ES (floats) and row pitch dp (elements).  The four channels
// of a dilated 3x3 filter go through packed fp32 FMAs in PAIRS (v_pk_fma_f32: the two channels' weights are one aligned scalar
// register pair, the tap is broadcast): each channel keeps the reference's tap order, and the 1x1 output convolution is the same
// scalar chain over (filter, channel) as the unfused stage -- half the vector instructions of the 12 x 9-tap filter bank.
// A MACRO, not a function: as an inlined function the compiler keeps all 120 weights live across the unrolled rows and spills them
// through v_readlane / v_writelane (+370 instructions per wave, +2 us: measured in round 3); expanded in the row loop it reloads
// them per row with scalar loads.
// OUT (a constant of the kernel the macro expands in) is the pass's OUTPUT SET.  The full pass writes everything.  The pass a frame takes
// along in its histogram launch (k_post_hist) writes what THAT frame reads -- traversability (its drift statistics), the normals too
// when it runs a visibility pass -- and stays owed: a full pass rewrites every output before anything else can look (post_settle,
// emap_api.hip).  POST_OUT_TRAV drops the store of traversability_input, the normal epilogue (five IEEE divisions, the square root)
// and its three stores -- and the traversability WORD: in that frame the value has one reader, the drift gate's predicate
// (double)trav > traversability_inlier (drift_inlier, emap_binned.hip), and a 4-byte store at stride 16 dirties every line of the hot
// array (17.6 MB written back for 4 MB of payload at 1024^2) to carry one bit per cell.  The predicate goes as ONE BYTE into the flag
// plane `tflag` (a constant of the expanding kernel as OUT is: null where OUT never selects it), indexed as cells.hot is; a cell the
// stencils do not decide (do_trav false: the 3-cell border) gets TRAV_FLAG_WORD, "the word you hold".  hot.w is not written and stays
// stale until the next full pass (post_settle has the invariant).  POST_OUT_TRAV_WORD: the same set with the word store
// (EMAP_POST_FLAGS=0).  (The values: emap_launch.h.)
#define POST_CELL(WT, ES, t0, dp, own_valid, do_trav, do_normal, c)                                                         \
  do {                                                                                                                    \
    typedef float v2f __attribute__((ext_vector_type(2)));                                                               \
    const float h = (t0)[0];                                                                                              \
    if (OUT == POST_OUT_FULL) trav_in[c] = h;                                                                             \
    if (STAGE == 1) break;                                                                                                \
    if (do_trav) {                                                                                                        \
      float acc = 0.f;                                                                                                    \
      _Pragma("unroll") for (int q = 0; q < 3; ++q) {                                                                     \
        const int dl = q + 1;                                                                                             \
        v2f s01 = {0.f, 0.f}, s23 = {0.f, 0.f};                                                                           \
        _Pragma("unroll") for (int a2 = 0; a2 < 3; ++a2)                                                                  \
          _Pragma("unroll") for (int b2 = 0; b2 < 3; ++b2) {                                                              \
            const float t = (t0)[((a2 - 1) * dl * (dp) + (b2 - 1) * dl) * (ES)];                                          \
            const v2f tt = {t, t};                                                                                        \
            const auto* w = (WT).w[q][a2 * 3 + b2];                                                                       \
            s01 = __builtin_elementwise_fma((v2f){w[0], w[1]}, tt, s01);                                                  \
            s23 = __builtin_elementwise_fma((v2f){w[2], w[3]}, tt, s23);                                                  \
          }                                                                                                               \
        acc = fmaf((WT).wo[q][0], fabsf(s01.x), acc);                                                                       \
        acc = fmaf((WT).wo[q][1], fabsf(s01.y), acc);                                                                       \
        acc = fmaf((WT).wo[q][2], fabsf(s23.x), acc);                                                                       \
        acc = fmaf((WT).wo[q][3], fabsf(s23.y), acc);                                                                       \
      }                                                                                                                   \
      const float tv = exp_neg(acc);                                                                                      \
      if (OUT == POST_OUT_TRAV) tflag[c] = (double)tv > P.trav_inlier ? TRAV_FLAG_ABOVE : TRAV_FLAG_BELOW;   /* the one reader's predicate (drift_inlier), one byte */ \
      else cells.hot[c].w = tv;                       /* trav: a 4-byte store into the 16-byte hot half */                \
    } else if (OUT == POST_OUT_TRAV) tflag[c] = TRAV_FLAG_WORD;           /* border: the word the hot half holds */      \
    if (OUT == POST_OUT_TRAV || OUT == POST_OUT_TRAV_WORD) break;                                                         \
    float nx = 0.f, ny = 0.f, nz = 0.f;                                                                                   \
    if ((do_normal) && (own_valid) > 0.5f) {                              /* (is_valid of the cell itself) */             \
      const float dzdx = (t0)[ES] - h, dzdy = (t0)[(ES) * (dp)] - h;                                                      \
      const float ax = -dzdy / P.res_f, ay = -dzdx / P.res_f;           /* IEEE: v_div_scale / v_div_fmas / v_div_fixup */ \
      const float nrm = sqrt_rn_ge1((ax * ax) + (ay * ay) + 1.0f);                                                        \
      nx = ax / nrm; ny = ay / nrm; nz = 1.0f / nrm;                                                                      \
    }                                                                                                                     \
    normal[c] = nx; normal[plane_stride + c] = ny; normal[2 * plane_stride + c] = nz;                                     \
  } while (0)

// ---------------------------------------------------------------------------------------------------------
// SPARSE tiles of the fused stencils.  A hole (mask < 0.5) searches its (2d + 1)^2 neighbourhood for the first source in the
// reference's scan order (ascending anti-diagonals dx + dy, :429-436) and gives up after all 49 reads when there is none -- on a
// white-noise map a source is two or three reads away, but a real map is mostly UNKNOWN beyond the sensor's dense zone (scan rings
// further apart than the dilation reach, the shadow of a wall): 86 % holes at 1024^2 on the ray-cast terrain of tests/_fixtures.py, a
// hole between two scan rings probed 10-40 cells in LDS before it found one, and the stencil launch took 69 us instead of 19.5.
// Round 4 put a reach mask in front of the search (source ballots smeared by d, OR-ed over 2d + 1 rows: 69 -> 56 us).  Round 5 runs
// the search itself on bits, in tiles where three cells of four are holes (dense tiles keep the probing loop: one or two probes beat
// seven window reads): the raw SOURCE bits of every region row go to LDS (one ballot per row, no smearing); a hole takes the
// (2d + 1)-bit window of each of its 2d + 1 rows and shifts row dy's window left by dy + d -- after that every anti-diagonal
// dx + dy = const is ONE bit position in all rows -- and ORs them: the first set bit is the first anti-diagonal with a source, the
// first row that has that bit the first dy of the reference's order; nothing set = no source in reach, the raw value stays.  ~60
// instructions per hole whatever the distance, the same cell as the probing loop picks: terrain 56 -> 40 us, 8192^2 / 16 M points
// (79 % holes) 0.947 -> 0.910 ms.
template <int PT_THREADS, class SrcFn>
__device__ __forceinline__ void post_source_masks(unsigned int* __restrict__ sm, int RH, int RW, SrcFn src) {      // 5 words per region row: columns 0 .. 127 + a zero word
  constexpr int PT_WAVES = PT_THREADS / 64;
  const int tc = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int r = wv; r < RH; r += PT_WAVES) {
    const unsigned long long lo = __builtin_amdgcn_ballot_w64(src(r, tc));
    const unsigned long long hi = __builtin_amdgcn_ballot_w64(64 + tc < RW && src(r, 64 + tc));
    if (tc == 0) { sm[5 * r] = (unsigned int)lo; sm[5 * r + 1] = (unsigned int)(lo >> 32); sm[5 * r + 2] = (unsigned int)hi; sm[5 * r + 3] = (unsigned int)(hi >> 32); sm[5 * r + 4] = 0u; }
  }
  __syncthreads();
}
// k_post's staging loop, once for interior and edge tiles.  The first 64 columns of the RH x (64 + EC) region go row-wise (one wave per
// region row, lane = column), the remaining EC = 6 + 2d columns as a linear walk over (row, column) pairs, full lanes.  A turn requests
// the wave's next U rows AND the thread's next POST_KW pairs, then consumes them -- the 44 x 76 region of a 32-row tile at d = 3 is ONE
// trip to memory (its walk is 528 pairs for 512 threads: the rows, the pair and sixteen lanes' second pair used to be three trips behind
// each other); large radii take max(row turns, walk turns) trips instead of their sum.  Uniform trip count.
// No branch stands around a load: a slot past the last row / pair reads the last one again and is dropped.  Behind a skipped load the
// compiler cannot count what is outstanding, and it re-uses the destination of a load that MAY be pending for the next address:
// either way it waits for everything (vmcnt(0)) between the loads -- the six rows of a wave were three to five trips, not one.  (The
// loops that did that -- rows with `if (r < RH)` around each load, then the walk -- were kept for one comparison and lost it:
// k_post<32, 0> 18.6-18.7 -> 17.7-17.8 us, frame 68.6 -> 67.6 us)
// load_row(r) / load_pair(r, cc): the lane's cell of region row r / the cell (r, cc), with a tag that travels into put(r, cc, cell)
// (edge tiles: the flag word; interior tiles pass a constant, which costs nothing).  wv, tc: the caller's wave (scalar) and lane;
// emagic = ceil(2^32 / EC).
struct PostLd { float4 q; int tag; };
template <int U, int PT_THREADS, class RowFn, class PairFn, class PutFn>
__device__ __forceinline__ void post_stage_trips(int wv, int tc, int RH, int EC, unsigned int emagic, RowFn load_row, PairFn load_pair, PutFn put) {
  constexpr int PT_WAVES = PT_THREADS / 64;
  const int etotal = RH * EC;
  const int wturns = (etotal + PT_THREADS * POST_KW - 1) / (PT_THREADS * POST_KW);
  int rb = wv, eb0 = threadIdx.x;
  for (int turn = 0; rb < RH || turn < wturns; ++turn, rb += PT_WAVES * U, eb0 += PT_THREADS * POST_KW) {
    PostLd q[U], qe[POST_KW];
    int er[POST_KW], ec[POST_KW];
#pragma unroll
    for (int u = 0; u < U; ++u) q[u] = load_row(min(rb + u * PT_WAVES, RH - 1));      // (scalar row)
#pragma unroll
    for (int j = 0; j < POST_KW; ++j) {
      const int eb = min(eb0 + j * PT_THREADS, etotal - 1);
      er[j] = (int)__umulhi((unsigned int)eb, emagic); ec[j] = 64 + eb - er[j] * EC;
      qe[j] = load_pair(er[j], ec[j]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rb + u * PT_WAVES;
      if (r < RH) put(r, tc, q[u]);
    }
#pragma unroll
    for (int j = 0; j < POST_KW; ++j) if (eb0 + j * PT_THREADS < etotal) put(er[j], ec[j], qe[j]);
  }
}
// first source of the hole at region (R0, C0) in the reference's scan order: true + its offsets, false: none within reach
__device__ __forceinline__ bool post_first_source(const unsigned int* __restrict__ sm, int R0, int C0, int d, int& dy_out, int& dx_out) {
  const int cs = C0 - d, k = cs >> 5, sh = cs & 31;
  const unsigned int wmask = (2u << (2 * d)) - 1u;                  // 2d + 1 bits
  unsigned long long any = 0ull;
  for (int dy = -d; dy <= d; ++dy) {
    const unsigned int* m = sm + 5 * (R0 + dy) + k;
    any |= (unsigned long long)(__builtin_amdgcn_alignbit(m[1], m[0], sh) & wmask) << (dy + d);
  }
  if (!any) return false;
  const int s2 = (int)__builtin_ctzll(any) - 2 * d;                 // the first anti-diagonal dx + dy with a source
  for (int dy = max(-d, s2 - d); dy <= min(d, s2 + d); ++dy) {
    const unsigned int* m = sm + 5 * (R0 + dy) + k;
    if ((__builtin_amdgcn_alignbit(m[1], m[0], sh) >> (s2 - dy + d)) & 1u) { dy_out = dy; dx_out = s2 - dy; return true; }
  }
  return false;                                                     // (not reached: the bit came from one of these rows)
}

// k_post_dma: the same fused stencils with the region staged by gfx950's LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes
// straight from HBM into LDS, no VGPR round trip, no ds_write).  The region is a pure copy of 16-byte cold halves (time, upper,
// is_upper, valid'), so a wave moves one region row per instruction: lane = column, the LDS destination is wave-uniform base +
// 16 x lane (what the instruction offers), the SOURCE address is per lane -- which is where the circular origin, the strip's local
// rows and the reference's flat-index row wrap (:403-407) go.  Every wave computes the row terms it needs in registers (one
// region row per lane, fetched with a lane permute): no table and no barrier in front of the loads.  Cells that do not exist
// (beyond the map or the strip's rows) are read from a constant cell with mask 1 (never a hole) whose position excludes it as a
// source in the (rare) hole search.  A second, LDS-only pass extracts the value plane the stencils read (unit stride: free of bank
// conflicts -- tap reads on the 16-byte records would be 4-way conflicts) and lists the holes.
// Measured (round 3, MI355X, event spacing, three sessions): with 16-row tiles (46 KB of LDS: three workgroups per CU) 244-252 us
// at 4096^2 against 256-275 us for round 2's register-staged k_post, 22.1-22.9 vs 22.9 us at 1024^2 -- a gain of 2-10 %, not the
// third the instruction count suggested: the kernel is not purely issue bound; with 32-row tiles (72 KB: two per CU) 265 / 24.1 us;
// with the 4-row tiles of robot-scale maps 12.0 vs 9.7 us (those keep k_post).
// Two dead ends on the way: the 12-byte DMA form (upper, is_upper, valid' only) still writes its lanes at a 16-byte LDS stride
// (tools/dbg/dma12.hip), so it cannot produce conflict-free three-dword records; and a "lean" register-staged rewrite of the
// staging loops (same structure as here, loads through VGPRs) compiled to 106 VGPRs and ran 30 % slower than round 2's kernel.
// Large dilation radii (more than 62 region rows) keep k_post.
// ---------------------------------------------------------------------------------------------------------
struct NullCold { float time, upper, is_upper, valid; };
__device__ const NullCold k_null_cold = {0.f, 0.f, 0.f, 1.f};

template <int PT_R, int STAGE>
__global__ __launch_bounds__(512) void k_post_dma(KP P, TravW Wt, Cells cells, float* __restrict__ trav_in,
                                                  float* __restrict__ normal, long plane_stride, int d, PostSegs S) {
  constexpr int OUT = POST_OUT_FULL;
  constexpr unsigned char* tflag = nullptr;      // (POST_CELL: the full pass writes no flag plane)
  int seg_b = S.b[0], seg_e = S.e[0], ty = blockIdx.y;
#pragma unroll
  for (int k = 1; k < 4; ++k) if (k < S.n && (int)blockIdx.y >= S.t0[k]) { seg_b = S.b[k]; seg_e = S.e[k]; ty = blockIdx.y - S.t0[k]; }
  constexpr int PT_THREADS = 512, PT_WAVES = PT_THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int RW = PT_C + 6 + 2 * d, RH = PT_R + 6 + 2 * d, vp = RW + 1;     // staged region: tile + halo 3 + d (RH + 2 <= 64); vp: pitch of the value plane
  const int DW = PT_C + 6, DH = PT_R + 6;                                   // region whose DILATED value is needed (halo 3)
  float4* raw = reinterpret_cast<float4*>(lds);                             // [RH][RW] cold halves as they lie in HBM
  float* val = lds + 4 * RH * RW;                                           // [RH][vp] upper_bound, holes of the DW x DH region overwritten by their dilated value
  int* rtab = reinterpret_cast<int*>(val + RH * vp);                        // RH + 2 row terms (hole search, epilogue)
  unsigned int* hs = reinterpret_cast<unsigned int*>(rtab + ((RH + 3) & ~1));      // sparse tiles: source bits of the region rows, 5 words each (post_source_masks); 8 words per row reserved
  unsigned short* holes = reinterpret_cast<unsigned short*>(hs + 8 * RH);
  __shared__ unsigned int n_holes;
  if (threadIdx.x == 0) n_holes = 0u;
  const int C = P.C;
  const int tile_r = seg_b + ty * PT_R, tile_c = blockIdx.x * PT_C;        // logical row / column of the tile origin
  const int tc = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = tile_r - 3 - d, c0 = tile_c - 3 - d;
  // row term of region row lane - 1 (one extra row on both sides for the flat-index carry): local row of the arrays (bits 0..23;
  // bit 31 set: not in the map / strip), bit 30: a border row (never a dilation source)
  int rowT;
  {
    const int g = r0 - 1 + tc;
    const bool in_map = g >= 0 && g <= C - 1 && tc < RH + 2;
    const int lr = in_map ? local_row(P, phys_row(P, g)) : -1;
    rowT = lr < 0 ? (int)0x80000000 : lr | ((g >= 1 && g <= C - 2) ? 0 : 0x40000000);
    if (wv == 0 && tc < RH + 2) rtab[tc] = rowT;                   // visible after the barrier below
  }
  auto col_terms = [&](int cc, int& dr, int& pc, int& flags) {     // region column -> row carry, physical column, flag bits
    int cl = c0 + cc; dr = 0;
    if (cl < 0) { cl += C; dr = -1; } else if (cl >= C) { cl -= C; dr = 1; }
    flags = ((cl >= 1 && cl <= C - 2) ? 0 : 0x40000000) | ((cl >= 0 && cl < C) ? 0 : (int)0x80000000);      // (a region wider than the map: columns past the wrap are unused)
    pc = (cl >= 0 && cl < C) ? phys_col(P, cl) : 0;
  };
  const int nchunk = (RW + 63) >> 6;
  for (int k = 0; k < nchunk; ++k) {                               // phase 1: one DMA instruction per (region row, 64 columns)
    const int cc = k * 64 + tc;
    int dr, pc, fl;
    col_terms(cc, dr, pc, fl);
    for (int r = wv; r < RH; r += PT_WAVES) {
      const int T = __shfl(rowT, r + 1 + dr, 64) | fl;             // (every lane takes part in the permute: a disabled source lane would read as 0)
      const float4* src = T >= 0 ? cells.cold + (long)(__umul24((unsigned int)T & 0xffffffu, (unsigned int)C) + (unsigned int)pc)
                                 : reinterpret_cast<const float4*>(&k_null_cold);
      if (cc < RW) lds_dma16(src, raw + r * RW + k * 64);
    }
  }
  __syncthreads();                                                 // (drains the DMA queue: the compiler places vmcnt(0) in front of the barrier)
  for (int k = 0; k < nchunk; ++k) {                               // phase 2: value plane + hole list, LDS only
    const int cc = k * 64 + tc;
    const bool cwin = (unsigned int)(cc - d) < (unsigned int)DW;
    if (cc < RW)
      for (int r = wv; r < RH; r += PT_WAVES) {
        const float4 q = raw[r * RW + cc];
        val[r * vp + cc] = q.y;
        // a hole of the region whose dilated value is needed (the constant cell of non-existent positions has mask 1: never listed)
        if (q.z + q.w < 0.5f && cwin && (unsigned int)(r - d) < (unsigned int)DH) holes[atomicAdd(&n_holes, 1u)] = (unsigned short)((r - d) * DW + (cc - d));
      }
  }
  __syncthreads();
  // Hole search, one hole per lane: first hit on ascending anti-diagonals == the reference's scan order with its signed dx+dy
  // criterion (:429-436).  Sources are cells with mask > 0.5 that exist and are is_inside (custom_kernels.py:34-44); a source is
  // never a hole, so the in-place writes cannot feed another search (Jacobi semantics of the reference kernel).
  const unsigned int nh = n_holes;
  const bool sparse = 4 * (int)nh > 3 * DW * DH && RW <= 128 && d <= 15;       // (uniform) three cells of four are holes
  if (sparse) {                                                     // mostly unknown tile: the search on bit masks (post_first_source)
    post_source_masks<PT_THREADS>(hs, RH, RW, [&](int r, int cc) {
      const int c1 = min(cc, RW - 1);
      const float4 q = raw[r * RW + c1];
      int dr, pc, fl;
      col_terms(c1, dr, pc, fl);
      return q.z + q.w > 0.5f && ((rtab[r + 1 + dr] | fl) & (int)0xC0000000) == 0;      // a source: mask > 0.5, exists, is_inside
    });
    for (unsigned int hi = threadIdx.x; hi < nh; hi += PT_THREADS) {
      const int pos = holes[hi], r = pos / DW + d, cc = pos - (pos / DW) * DW + d;
      int dy, dx;
      if (post_first_source(hs, r, cc, d, dy, dx)) val[r * vp + cc] = raw[(r + dy) * RW + cc + dx].y;
    }
  } else
  for (unsigned int hi = threadIdx.x; hi < nh; hi += PT_THREADS) {
    const int pos = holes[hi], r = pos / DW + d, cc = pos - (pos / DW) * DW + d;
    bool found = false;
    for (int s2 = -2 * d; s2 <= 2 * d && !found; ++s2) {
      const int dy0 = max(-d, s2 - d), dy1 = min(d, s2 + d);
      for (int dy = dy0; dy <= dy1; ++dy) {
        const int rs = r + dy, cs = cc + (s2 - dy);
        const float4 q = raw[rs * RW + cs];
        if (q.z + q.w > 0.5f) {
          int dr, pc, fl;
          col_terms(cs, dr, pc, fl);
          if (((rtab[rs + 1 + dr] | fl) & (int)0xC0000000) == 0) { val[r * vp + cc] = q.y; found = true; break; }
        }
      }
    }
  }
  if (nh) __syncthreads();                       // (uniform: every thread read the same count)
  const int col = tile_c + tc;                   // logical column
  if (col >= C) return;
  const int pcol = phys_col(P, col);
  constexpr int RPW = PT_R >= PT_WAVES ? PT_R / PT_WAVES : 1;
  const bool col_in = STAGE == 0 && col >= 3 && col <= C - 4;
  const bool col_n = col >= 1 && col <= C - 3;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int tr = wv * RPW + k, gr = tile_r + tr;                 // scalar
    if (tr >= PT_R || gr >= seg_e) break;
    const int rr = tr + 3 + d, rc = tc + 3 + d;
    const long c = (long)(rtab[rr + 1] & 0xffffff) * C + pcol;
    const float* t0 = &val[rr * vp + rc];
    const float own_valid = raw[rr * RW + rc].w;
    POST_CELL(Wt, 1, t0, vp, own_valid, col_in && gr >= 3 && gr <= C - 4, col_n && gr >= 1 && gr <= C - 3, c);
  }
}

template <int PT_R, int STAGE>
__global__ __launch_bounds__(PT_R >= 32 ? POST_T32 : 512) void k_post(KP P, TravW Wt, Cells cells, float* __restrict__ trav_in,
                                                    float* __restrict__ normal, long plane_stride, int d, PostSegs S) {
  constexpr int OUT = POST_OUT_FULL;
  constexpr unsigned char* tflag = nullptr;      // (POST_CELL: the full pass writes no flag plane)
#define POST_BX blockIdx.x
#define POST_BY blockIdx.y
#include "emap_post_tile.h"
#undef POST_BX
#undef POST_BY
}

// k_post_hist: the stencil pass of frame N and the histogram of frame N + 1's cloud in ONE grid.  The two ends of the frame are where the
// chip is least busy -- k_bin_hist is one short latency chain per CU, k_post<32, 0> two issue-bound workgroups per CU with room for a
// third -- and they do not depend on each other: the histogram reads the cloud, the pose and the map's geometry, the stencils read and
// write map planes.  Workgroups [tile0, tile0 + n_tiles) take the stencil tile ((b - tile0) % tiles_x, (b - tile0) / tiles_x), workgroups
// [hist0, hist0 + G.B) the chunk rho(b - hist0, G.B) of the cloud (emap_bin_hist.h), 8 points per thread in two batches; the rest of the grid is idle
// padding.  No workgroup waits for another.  The host launches it only when all of them are resident at once (launch_post_hist) and keeps
// hist0 a multiple of 8: workgroup b runs on XCD b % 8, so the histogram workgroup of a chunk then sits on the XCD of its twin in
// k_bin_scatter (bin_chunk_of_block), as it does in k_bin_hist.  That placement is for speed only; nothing depends on it for the result.
// The tiles stand in front of the histogram workgroups (hist0 = n_tiles rounded up to 8); the other order was measured
// (EMAP_POST_HIST_FRONT).  Stage 0, one row interval, 512 threads.  OUT: the output set of the stencil tiles (POST_CELL);
// tflag: the flag plane POST_OUT_TRAV writes (one byte per cell of cells.hot; not looked at by the other sets).
#ifndef POST_HIST_U
#define POST_HIST_U 4      /* loads in flight per thread of a histogram workgroup: two batches of 4; one batch of 8 was measured slower */
#endif
template <int MODE, int PT_R, int OUT>
__global__ __launch_bounds__(512) void k_post_hist(KP P, TravW Wt, Cells cells, float* __restrict__ trav_in, float* __restrict__ normal,
                                                   long plane_stride, int d, PostSegs S, int tiles_x, int n_tiles, int tile0, int hist0,
                                                   Pose T, BinGeo G, const float* __restrict__ pts, long n, int stride,
                                                   unsigned int* __restrict__ hist, unsigned char* __restrict__ tflag) {
  static_assert(PT_R < 32 || POST_T32 == 512, "k_post_hist runs both bodies with 512 threads");
  const int b = (int)blockIdx.x;                               // (uniform)
  if ((unsigned int)(b - tile0) < (unsigned int)n_tiles) {
    constexpr int STAGE = 0;
    const unsigned int bx = (unsigned int)((b - tile0) % tiles_x), by = (unsigned int)((b - tile0) / tiles_x);
#define POST_BX bx
#define POST_BY by
#include "emap_post_tile.h"
#undef POST_BX
#undef POST_BY
  } else if ((unsigned int)(b - hist0) < (unsigned int)G.B) {
    extern __shared__ float lds[];
    bin_hist_chunk<MODE, 512, POST_HIST_U>(P, T, G, pts, n, stride, hist, reinterpret_cast<unsigned int*>(lds),
                                           (unsigned int)(b - hist0), (unsigned int)G.B);
  }
}

// update_variance + update_time (elevation_mapping.py:420-426)
__global__ __launch_bounds__(EM_BLOCK) void k_var_time(KP P, Cells cells, int do_var, int do_time) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const long ci = li + (long)P.halo * P.C;
  if (P.mv.n) {                                   // pending map shifts: the whole cell is written out first (uniform branch)
    const int lrow = (int)(li / P.C);
    Cell c = cells[ci];
    cell_now(P, c, P.row0 + lrow, (int)(li - (long)lrow * P.C));
    if (do_var) c.v = c.v + P.time_var * c.valid;
    if (do_time) c.time = c.time + P.time_int;
    cells[ci] = c;
    return;
  }
  if (do_var) { float4 a = cells.hot[ci]; a.y = a.y + P.time_var * a.z; cells.hot[ci] = a; }     // variance lives in the hot half,
  if (do_time) cells.cold[ci].x = cells.cold[ci].x + P.time_int;                                 // time in the cold one
}

// ---- layer read-back for publishing (get_map_with_name_ref, elevation_mapping.py:579-775): border stripped, both axes
// flipped, NaN for unknown cells, +center_z for height layers -- one kernel + one D2H instead of several host passes.
// kind: 0 elevation, 1 variance, 2 traversability, 3 time, 4 upper_bound, 5 is_upper_bound, 6..8 normal x/y/z
__global__ __launch_bounds__(EM_BLOCK) void k_publish(KP P, Cells cells, const float* __restrict__ normal,
                                                       long plane_stride, int kind, float center_z, int only_above,
                                                       float* __restrict__ out) {
  const int C = P.C, M = C - 2;
  long k = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (k >= (long)M * M) return;
  const int orow = (int)(k / M), ocol = (int)(k % M);
  const int r = M - orow, c = M - ocol;                 // flip of the [1:-1, 1:-1] view: source cell (r, c) in [1, C-2], logical
  float v;
  if (kind >= 6) v = normal[(long)(kind - 6) * plane_stride + (long)wrap_up(r + P.norg_r, C) * C + wrap_up(c + P.norg_c, C)];
  else {
    const Cell m = cells[(long)(phys_row(P, r) + P.halo) * C + phys_col(P, c)];
    v = publish_value(kind, m, r, c, C, center_z, only_above);      // (emap_device.h: shared with k_grid_map)
  }
  out[k] = v;
}

// ---- state access helpers --------------------------------------------------------------------------------
// External views are in the order of the strip's LOGICAL rows (row j of the view = logical row logi_row(row0) + j, wrapping) and
// logical columns; (org_r, org_c) = origin of the array being viewed (cells and semantic layers: the map origin; normal planes and
// traversability_input: the origin they were written with).
__device__ __forceinline__ long view_cell(const KP& P, long li, int org_r, int org_c) {
  const int j = (int)(li / P.C), c = (int)(li - (long)j * P.C);
  const int r = P.nrows == P.C ? j : wrap_up(logi_row(P, P.row0) + j, P.C);   // logical row (a full map is viewed from logical row 0)
  const int lr = local_row(P, wrap_up(r + org_r, P.C));
  return lr < 0 ? -1 : (long)lr * P.C + wrap_up(c + org_c, P.C);
}
__global__ __launch_bounds__(EM_BLOCK) void k_get_plane(KP P, Cells cells, int word, float* __restrict__ out) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const long ci = view_cell(P, li, P.org_r, P.org_c);
  out[li] = word < 4 ? reinterpret_cast<const float*>(cells.hot + ci)[word] : reinterpret_cast<const float*>(cells.cold + ci)[word - 4];
}
__global__ __launch_bounds__(EM_BLOCK) void k_set_plane(KP P, Cells cells, int word, const float* __restrict__ in) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const long ci = view_cell(P, li, P.org_r, P.org_c);
  if (word < 4) reinterpret_cast<float*>(cells.hot + ci)[word] = in[li]; else reinterpret_cast<float*>(cells.cold + ci)[word - 4] = in[li];
  if (word == 2) cells.cold[ci].w = in[li];                 // is_valid is mirrored in the cold half
}
// planar float arrays (semantic layers, normal planes, traversability_input): gather / scatter between the view and the array
__global__ __launch_bounds__(EM_BLOCK) void k_plane_view(KP P, int org_r, int org_c, float* __restrict__ plane, float* __restrict__ view, int to_plane) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const long c = view_cell(P, li, org_r, org_c);
  if (to_plane) { if (c >= 0) plane[c] = view[li]; }
  else view[li] = c >= 0 ? plane[c] : 0.0f;        // rows this strip does not hold (normals written before a row shift): 0
}
// writes the pending map shifts into every owned cell (one full pass; needed only when something reads the map between a
// move and the next frame)
__global__ __launch_bounds__(EM_BLOCK) void k_materialize(KP P, Cells cells) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const int lrow = (int)(li / P.C);
  const long ci = li + (long)P.halo * P.C;
  Cell m = cells[ci];
  cell_now(P, m, P.row0 + lrow, (int)(li - (long)lrow * P.C));
  cells[ci] = m;
}
// zero-fills the band that a roll by (sr, sc) brought in (SemanticMap.shift_map_xy, semantic_map.py:127-136) in `nl` planes
__global__ __launch_bounds__(EM_BLOCK) void k_band_clear(KP P, float* __restrict__ planes, int nl, long plane_stride, int sr, int sc) {
  long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= (long)P.nrows * P.C) return;
  const int lrow = (int)(li / P.C), pcol = (int)(li - (long)lrow * P.C);
  const int r = logi_row(P, P.row0 + lrow), c = logi_col(P, pcol);
  if (!((sr > 0 && r < sr) || (sr < 0 && r >= P.C + sr) || (sc > 0 && c < sc) || (sc < 0 && c >= P.C + sc))) return;
  for (int l = 0; l < nl; ++l) planes[(long)l * plane_stride + li + (long)P.halo * P.C] = 0.0f;
}
__global__ __launch_bounds__(EM_BLOCK) void k_fill_cells(Cells cells, long n, Cell v) {
  long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i < n) cells[i] = v;
}
template <int MODE>
__global__ __launch_bounds__(EM_BLOCK) void k_point_index(KP P, Pose T, const float* __restrict__ pts, long n, int stride,
                                                           int* __restrict__ idx, unsigned char* __restrict__ flags) {
  long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  float rx, ry, rz;
  load_point(pts, i, stride, rx, ry, rz);
  Geo g = geometry<MODE>(P, T, rx, ry, rz);
  idx[i] = g.finite ? P.C * g.ix + g.iy : -1;
  flags[i] = g.finite ? (unsigned char)((g.valid ? 1 : 0) | (g.inside ? 2 : 0)) : 0;
}

// halo rows: contiguous 32-B cells, so pack/unpack are plain device copies done by the host API.

// ---- launch wrappers (emap_launch.h) -------------------------------------------------------------------
static inline unsigned int nblk(long n) { return (unsigned int)((n + EM_BLOCK - 1) / EM_BLOCK); }

// gate != nullptr: the drift gate rides in the last workgroup (whole frames: emap_update); false is returned when nothing was launched
bool launch_count(hipStream_t s, const KP& P, const Pose& T, const float* pts, long n, int stride, Cells cells,
                  AccF* acc, ErrSlot* slots, const GateArgs* gate, FrameDev* F, unsigned int* sync) {
  if (n <= 0) return false;
  CountGate CG; memset(&CG, 0, sizeof CG);
  if (gate && F && sync) { CG.on = 1; CG.A = *gate; CG.F = F; CG.sync = sync; }
  if (P.mode == 0) hipLaunchKernelGGL(k_count<0>, dim3(nblk(n)), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, cells, acc, slots, CG);
  else hipLaunchKernelGGL(k_count<1>, dim3(nblk(n)), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, cells, acc, slots, CG);
  return CG.on != 0;
}
// Workgroups k_small_frame may use on the current device: a QUARTER of what the device holds at once (all of them must be resident;
// the margin leaves room for the grids of other contexts / streams on the same device).  0: do not use it.
static int small_frame_limit() {
  static int limit[EM_MAX_DEV]; static bool known[EM_MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EM_MAX_DEV) return 0;
  if (!known[dev]) {
    int cus = 0, nb0 = 0, nb1 = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb0, reinterpret_cast<const void*>(k_small_frame<0>), EM_BLOCK, 0) != hipSuccess) nb0 = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb1, reinterpret_cast<const void*>(k_small_frame<1>), EM_BLOCK, 0) != hipSuccess) nb1 = 0;
    (void)hipGetLastError();
    const long all = (long)cus * (nb0 < nb1 ? nb0 : nb1);
    limit[dev] = (int)(all / 4 > 512 ? 512 : all / 4);             // (512 x 256 threads = the largest cloud of the atomic path)
    known[dev] = true;
  }
  return limit[dev];
}
// the grid of k_small_frame for n points on P's map, 0: the frame keeps the chain of launches
int small_frame_grid(const KP& P, long n) {
  if (n <= 0 || P.nrows != P.C || P.halo != 0 || P.C > 512) return 0;
  const long cells = (long)P.nrows * P.C;
  long g = nblk(n);
  const long gc = nblk(cells) < 256 ? nblk(cells) : 256;           // small clouds: enough workgroups for the per-cell phase
  if (g < gc) g = gc;
  const int limit = small_frame_limit();
  return g <= limit ? (int)g : 0;
}
void launch_small_frame(hipStream_t s, int grid, const KP& P, const Pose& T, const float* pts, long n, int stride, Cells cells, AccF* acc,
                        unsigned int* cnt_out, const OverlapArgs& O, const GateArgs& gate, FrameDev* F, FrameDev* F_save,
                        ErrSlot* slots, unsigned int* sync, unsigned int* flag, unsigned int* host2, unsigned int* poison, unsigned int epoch,
                        unsigned int spin_limit, int test_abort) {
  SmallFrame S; memset(&S, 0, sizeof S);
  S.A = gate; S.F = F; S.F_save = F_save; S.slots = slots; S.sync = sync; S.flag = flag; S.host = host2; S.poison = poison; S.epoch = epoch;
  S.spin_limit = spin_limit; S.test_abort = test_abort;
  if (P.mode == 0) hipLaunchKernelGGL(k_small_frame<0>, dim3(grid), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, cells, acc, cnt_out, O, S);
  else hipLaunchKernelGGL(k_small_frame<1>, dim3(grid), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, cells, acc, cnt_out, O, S);
}
void launch_gate(hipStream_t s, const GateArgs& A, ErrSlot* slots, FrameDev* F, int reduce_only, double* dev_out, const double* dev_totals) {
  hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, s, A, slots, F, reduce_only, dev_out, dev_totals);
}
void launch_fuse(hipStream_t s, const KP& P, const Pose& T, const float* pts, long n, int stride, Cells cells, AccF* acc,
                 const FrameDev* F) {
  if (n <= 0) return;
  dim3 g(nblk(n)), b(EM_BLOCK);
  if (P.mode == 0) hipLaunchKernelGGL(k_fuse<0>, g, b, 0, s, P, T, pts, n, stride, cells, acc, F);
  else hipLaunchKernelGGL(k_fuse<1>, g, b, 0, s, P, T, pts, n, stride, cells, acc, F);
}
void launch_commit(hipStream_t s, const KP& P, Cells cells, const AccF* acc, const FrameDev* F, unsigned long long* inert) {
  hipLaunchKernelGGL(k_commit, dim3((P.C + 63) / 64, P.nrows), dim3(64), 0, s, P, cells, acc, F, inert);
}
void launch_ray_apply(hipStream_t s, const KP& P, Cells cells, AccR* accr, unsigned long long* inert, const OverlapArgs& O, FrameDev* F, unsigned int* ray_pref_host, int par) {
  hipLaunchKernelGGL(k_ray_apply, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, cells, accr, inert, O, F, ray_pref_host, par);
}
// 512 threads per workgroup (round 6; 1024 until round 5): with the reach window an LDS-bitmap workgroup needs ~60 KB, two fit a CU,
// and one's prologue (table, window copy, barrier) overlaps the other's march -- same box, 1024 / 512 / 256: uniform 1024^2 pass 224 /
// 217 / 224 us, terrain scene 184 / 164 / 153 us, 4096^2 / 4 M rays 1.65 / 1.48 / 1.67 ms.
#ifndef RAY_BLOCK
#define RAY_BLOCK 512
#endif
// The reach window of the rays of one frame on a whole-map context, in bitmap coordinates (logical rows, 32-bit word columns): a sample
// lies at t + r * s with s <= Q(max_ray_length) and |r_x|, |r_y| <= 1 + 2^-10 (unit vector, components rounded to half in
// reference_fp16 mode); its coordinate is then rounded to half (2^-11 relative; fp32 mode: 2^-24) and indexed by floor(x / res + C / 2),
// clamped to the map.  D bounds all of that with room to spare, + 2 cells.  false: no window (non-finite pose, a row pitch the 2-D copy
// cannot take, or nothing to gain: the window is the map).
static bool ray_lds_window(const KP& P, const Pose& T, LWin* w) {
  const int C = P.C, wpr32 = ((P.pitch + 63) / 64) * 2;
  if ((wpr32 * 4) % 16 != 0 || P.pitch != P.C || P.nrows != P.C) return false;
  int lo[2], hi[2];
  for (int a = 0; a < 2; ++a) {
    const double t = (double)T.t[a];
    if (!(fabs(t) < 1.0e6)) return false;
    const double D = (double)P.q_mrl * 1.004 + (fabs(t) + (double)P.q_mrl) * (P.mode == 0 ? 1.0 / 512.0 : 1.0e-5) + 2.0 * P.res;
    const double l = floor((t - D) / P.res + P.half_w) - 2.0, h = floor((t + D) / P.res + P.half_w) + 2.0;
    lo[a] = (int)fmin(fmax(l, 0.0), (double)(C - 1)); hi[a] = (int)fmin(fmax(h, 0.0), (double)(C - 1));
  }
  LWin v;
  v.r0 = lo[0]; v.nr = hi[0] - lo[0] + 1;
  v.w0 = (lo[1] / 128) * 4;                                    // 128 columns = four 32-bit words = one 16-byte piece
  int w1 = (hi[1] / 128 + 1) * 4; if (w1 > wpr32) w1 = wpr32;
  v.wpr = w1 - v.w0;
  if (v.wpr % 4 != 0) return false;                            // (a pitch that is not a multiple of 128 columns cuts the last piece)
  if ((long)v.nr * v.wpr >= (long)P.nrows * wpr32) return false;
  *w = v;
  return true;
}
template <int MODE, bool STATS, int IDX, bool STRIP> static void launch_rays_i(hipStream_t s, const KP& P, const Pose& T, const RayTab& Rt, const float* pts,
                                                                              long n, int stride, Cells cells, const AccRView& accr,
                                                                              const float* normal, long plane_stride, FrameDev* F, const unsigned long long* inert,
                                                                              const unsigned int* inl, int inl_stride, const float* thr, const unsigned int* order, const unsigned int* n_sorted) {
  constexpr int SMALL_BLOCK = 256, SMALL_LPR = 4;
  // Small clouds (robot scale: 50 k rays = 49 workgroups of 1024) leave most of the 256 CUs idle while every wave walks its ~350
  // dependent steps: 256-thread workgroups spread the same waves over four times as many CUs, one wave per SIMD.
  const bool small = n < 131072;
  const int block = small ? SMALL_BLOCK : RAY_BLOCK;
  const int lpr = small ? SMALL_LPR : 1;
  const size_t lds = (IDX == 1 ? (((size_t)(Rt.hi - Rt.lo) + 2 + 3) & ~(size_t)3) * 4 : 0) + (size_t)(((Rt.nS + 3) & ~3) + 8 * lpr) * 4 + (size_t)(block / 64) * 3 * 128 * 4;      // [index table] + step table + the waves' visit queues
  size_t map_bytes = ((size_t)P.nrows * ((P.pitch + 63) / 64) * 2 + 2) * 4;       // bitmap + the all-ones word ...
  { size_t al = 4; while (al < (size_t)((P.pitch + 63) / 64) * 8) al <<= 1; map_bytes += al; }      // ... + alignment to the row pitch
  LWin lw = {0, P.nrows, 0, ((P.pitch + 63) / 64) * 2};
  if (!STRIP) {                                    // whole-map contexts: only the sensor's reach window (EMAP_RAY_WINDOW=0: the whole bitmap, A/B and test hook)
    static const bool win_off = getenv("EMAP_RAY_WINDOW") && atoi(getenv("EMAP_RAY_WINDOW")) == 0;
    if (!win_off && ray_lds_window(P, T, &lw)) map_bytes = ((size_t)lw.nr * lw.wpr + 2) * 4 + 16;
  }
  // EMAP_RAY_LMAP = 0 / 1: never / whenever it fits (tuning and test hook); unset: whenever it fits unless the map is mostly unknown or
  // stale (KP::ray_pref, from the previous frames' share of quiet cells): there the march queues cell work at almost every step and
  // is latency bound -- the global-bitmap variant runs two workgroups per CU (terrain scene: 187 vs 217 us; uniform benchmark: LDS 10 % ahead)
  static const int lmap_env = getenv("EMAP_RAY_LMAP") ? atoi(getenv("EMAP_RAY_LMAP")) : -1;
  const bool lmap = !small && lds + map_bytes <= 158 * 1024 && (lmap_env == 1 || (lmap_env != 0 && !P.ray_pref));      // (small clouds: staging the bitmap per workgroup would dominate)
  dim3 g((unsigned int)((n * lpr + block - 1) / block)), b(block);
  auto go = [&](auto kern, LdsRaised& raised, size_t bytes) {    // per instantiation and device: the half -> index table + queues [+ bitmap] can exceed the default 64 KB window
    if (!raise_lds(kern, raised, 158 * 1024) && bytes > 64 * 1024) return;      // (the launch below would fail: hipGetLastError reports it to the caller)
    hipLaunchKernelGGL(kern, g, b, bytes, s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted, lw);
  };
  static LdsRaised raised0, raised1, raised2;
  if (small) go(k_rays<MODE, STATS, IDX, STRIP, SMALL_BLOCK, false, SMALL_LPR>, raised2, lds);
  else if (lmap) go(k_rays<MODE, STATS, IDX, STRIP, RAY_BLOCK, true, 1>, raised1, lds + map_bytes);
  else go(k_rays<MODE, STATS, IDX, STRIP, RAY_BLOCK, false, 1>, raised0, lds);
}
template <int MODE, bool STATS> static void launch_rays_t(hipStream_t s, const KP& P, const Pose& T, const RayTab& Rt, const float* pts,
                                                          long n, int stride, Cells cells, const AccRView& accr,
                                                          const float* normal, long plane_stride, FrameDev* F, const unsigned long long* inert,
                                                          const unsigned int* inl, int inl_stride, const float* thr, const unsigned int* order, const unsigned int* n_sorted) {
  const bool strip = P.nrows < P.C || P.wmode;          // (a ray window is addressed like a strip: offset rows and columns, own pitch)
  // index method (AxisIdx): the float formula when the host proved it exact (reference_fp16) or when it IS the definition (fp32);
  // else the half -> index table if it fits the default LDS window next to the step table; else the defining arithmetic
  int idx = 0;
  if (MODE == 0 && Rt.formula_ok) idx = 2;
  else if (MODE == 0 && Rt.lut != nullptr && ((size_t)(Rt.hi - Rt.lo) + 2) * 4 + (size_t)Rt.nS * 4 <= 100 * 1024) idx = 1;
#define RAYS_GO(I, S) launch_rays_i<MODE, STATS, I, S>(s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted)
  if (MODE == 0) {
    if (idx == 2) { if (strip) RAYS_GO(2, true); else RAYS_GO(2, false); }
    else if (idx == 1) { if (strip) RAYS_GO(1, true); else RAYS_GO(1, false); }
    else { if (strip) RAYS_GO(0, true); else RAYS_GO(0, false); }
  } else { if (strip) RAYS_GO(0, true); else RAYS_GO(0, false); }
#undef RAYS_GO
}
// `thr`: per 8 x 8 block visit threshold of k_tile_fuse<true, true> (nullptr: no filter).  `inl` / `inl_stride`: per-cell drift-inlier counts of the frame (newmap[3]) as 32-bit words with an element stride -- the dense
// plane of the tile kernel (stride 1) or the high halves of AccF::pts_inl (stride 10, offset 1) on the staged / atomic path
void launch_rays(hipStream_t s, const KP& P, const Pose& T, const RayTab& Rt, const float* pts, long n, int stride, Cells cells,
                 const AccRView& accr, const float* normal, long plane_stride, FrameDev* F, bool stats,
                 const unsigned long long* inert, const unsigned int* inl, int inl_stride, const float* thr,
                 const unsigned int* order, const unsigned int* n_sorted) {
  if (n <= 0) return;
  if (P.mode == 0) {
    if (stats) launch_rays_t<0, true>(s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted);
    else launch_rays_t<0, false>(s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted);
  } else {
    if (stats) launch_rays_t<1, true>(s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted);
    else launch_rays_t<1, false>(s, P, T, Rt, pts, n, stride, cells, accr, normal, plane_stride, F, inert, inl, inl_stride, thr, order, n_sorted);
  }
}
void launch_win_pack(hipStream_t s, const KP& P, const Win& W, Cells cells, const float* normal, long plane_stride, const unsigned int* inl_plane, const unsigned long long* inert, float f_wall) {
  hipLaunchKernelGGL(k_win_pack, dim3(nblk((long)W.nr * W.nc)), dim3(EM_BLOCK), 0, s, P, W, cells, normal, plane_stride, inl_plane, inert, f_wall);
}
void launch_win_prepare(hipStream_t s, const Win& W, int C) {
  hipLaunchKernelGGL(k_win_prepare, dim3(W.nc / 64, W.nr / 8), dim3(512), 0, s, W, C);
}
void launch_win_reduce(hipStream_t s, long long* dh, unsigned int* key, const long long* dh_parts, const unsigned int* key_parts, int parts, long part_stride, long off, long cells) {
  if (cells > 0 && parts > 0) hipLaunchKernelGGL(k_win_reduce, dim3(nblk(cells)), dim3(EM_BLOCK), 0, s, dh, key, dh_parts, key_parts, parts, part_stride, off, cells);
}
void launch_win_unpack(hipStream_t s, const KP& P, const Win& W, AccR* accr) {
  hipLaunchKernelGGL(k_win_unpack, dim3(nblk((long)W.nr * W.nc)), dim3(EM_BLOCK), 0, s, P, W, accr);
}
void launch_average(hipStream_t s, const KP& P, Cells cells, AccF* acc, AccR* accr, const FrameDev* F, bool committed, bool rays,
                    unsigned int* cnt_out, const OverlapArgs& O) {
  dim3 g(nblk((long)P.nrows * P.C)), b(EM_BLOCK);
  if (committed) {
    if (rays) hipLaunchKernelGGL((k_average<true, true>), g, b, 0, s, P, cells, acc, accr, F, cnt_out, O);
    else hipLaunchKernelGGL((k_average<true, false>), g, b, 0, s, P, cells, acc, accr, F, cnt_out, O);
  } else {
    if (rays) hipLaunchKernelGGL((k_average<false, true>), g, b, 0, s, P, cells, acc, accr, F, cnt_out, O);
    else hipLaunchKernelGGL((k_average<false, false>), g, b, 0, s, P, cells, acc, accr, F, cnt_out, O);
  }
}
void launch_overlap(hipStream_t s, const KP& P, Cells cells, int cmin, int cmax, float hmin, float hmax) {
  long w = cmax - cmin;
  if (w <= 0) return;
  hipLaunchKernelGGL(k_overlap, dim3(nblk(w * w)), dim3(EM_BLOCK), 0, s, P, cells, cmin, cmax, hmin, hmax);
}
static size_t post_lds_bytes(int R, int d) {      // k_post: (value, mask, valid) region, row table, hole list
  return sizeof(float) * ((size_t)3 * (R + 6 + 2 * d) * (PT_C + 6 + 2 * d + 1) + (size_t)(R + 6 + 2 * d + 4)) + sizeof(unsigned short) * (size_t)(R + 6) * (PT_C + 6) + 32 * (size_t)(R + 6 + 2 * d) + 16;
}
static size_t post_dma_lds_bytes(int R, int d) {  // k_post_dma: 16-byte region cells + value plane, row table, hole list
  const size_t RH = R + 6 + 2 * d, RW = PT_C + 6 + 2 * d;
  return 16 * RH * RW + 4 * RH * (RW + 1) + 4 * (RH + 4) + 32 * RH + sizeof(unsigned short) * (size_t)(R + 6) * (PT_C + 6) + 16;
}
// true: the LDS-DMA kernel handles this (tile height, radius) -- one lane per region row for the row terms, three workgroups per CU
static bool post_use_dma(int R, int d) {
  static const bool dma_off = getenv("EMAP_POST_DMA") && atoi(getenv("EMAP_POST_DMA")) == 0;     // A/B and test hook: round 2's kernel
  static const long lds_kb = []() { const char* e = getenv("EMAP_POST_DMA_LDS_KB"); long v = e ? atol(e) : 0; return v >= 16 && v <= 150 ? v : 52; }();   // tuning knob
  return !dma_off && R >= 16 && R + 8 + 2 * d <= 64 && (long)post_dma_lds_bytes(R, d) <= lds_kb * 1024;     // (4-row tiles of robot-scale maps: 12.0 vs 9.7 us, measured)
}
int post_tile_rows(const KP& P) {
  static const int force_r = []() { const char* e = getenv("EMAP_POST_R"); int v = e ? atoi(e) : 0; return (v == 4 || v == 8 || v == 16 || v == 32) ? v : 0; }();
  int R;
  if (force_r) R = force_r;
  else if ((long)P.nrows * P.C <= 512L * 512L) R = 4;
  else if (post_lds_bytes(32, P.dil) > 60 * 1024) R = 16;             // large dilation radii: keep two workgroups per CU
  else R = (long)((P.C + PT_C - 1) / PT_C) * ((P.nrows + 31) / 32) >= 512 ? 32 : 16;
  // the DMA kernel wants three workgroups per CU, i.e. 16-row tiles -- and only where it was MEASURED ahead of the register-staged
  // kernel (event spacing, MI355X, round 3): 2048^2 57.7 vs 57.2 us (equal), 4096^2 231 vs 264 us (-12 %), 6144^2 737 vs 610 us
  // (+21 %), 8192^2 1894 vs 1186 us (+60 %, sparse map) / 1414 vs 982 us (cfg5); at 1024^2 (one round of 512 workgroups) rocprofv3
  // puts it behind as well (20.8 vs 18.4 us).  The degradation with the map's ROW PITCH (96 / 128 KB between consecutive rows of a
  // region) is not understood -- the sources and the 12 ... 44 rows a workgroup touches are the same in both kernels -- so the window
  // is set from the measurements: 3072^2 <= cells < 5120^2 (BASELINE configs[3]).  EMAP_POST_DMA_WINDOW="lo hi" (side lengths) overrides.
  static long win_lo = 3072, win_hi = 5120;
  static const bool win_env = []() { const char* e = getenv("EMAP_POST_DMA_WINDOW"); long a = 0, b = 0; if (e && sscanf(e, "%ld %ld", &a, &b) == 2 && a >= 1 && b > a) { win_lo = a; win_hi = b; } return true; }();
  (void)win_env;
  const long cells = (long)P.nrows * P.C;
  if (!force_r && R == 32 && !post_use_dma(32, P.dil) && post_use_dma(16, P.dil) && cells >= win_lo * win_lo && cells < win_hi * win_hi && P.C < win_hi) R = 16;      // (the row pitch counts: strips of wider maps keep k_post)
  while (R > 4 && !post_use_dma(R, P.dil) && post_lds_bytes(R, P.dil) > 150 * 1024) R /= 2;      // dilation radii up to 32: the staged region must fit the 160 KB LDS
  return R;
}
// outputs for up to four LOGICAL row intervals [seg_b[k], seg_e[k]) (owned by this strip, no circular seam inside); stage 1 = dilation only
// tile_rows: 0 = the size post_tile_rows picks for the whole strip; else the tile height for THIS launch (the boundary bands of a strip
// are dilation_size + 4 rows high: 32-row tiles would stage 44 region rows for 7 output rows)
static TravW post_weights(const float* w1, const float* w2, const float* w3, const float* wo) {
  TravW W;
  const float* wq[3] = {w1, w2, w3};                       // conv weights [channel][tap] -> [tap][channel]
  for (int q = 0; q < 3; ++q)
    for (int ch = 0; ch < 4; ++ch) {
      for (int tap = 0; tap < 9; ++tap) W.w[q][tap][ch] = wq[q][ch * 9 + tap];
      W.wo[q][ch] = wo[q * 4 + ch];
    }
  return W;
}
static unsigned int post_emagic(int d) { return (unsigned int)((0x100000000ull + (unsigned long long)(6 + 2 * d) - 1ull) / (unsigned long long)(6 + 2 * d)); }
// the kernel launch_post picks for tile height R: the LDS-DMA one?
static bool post_launch_dma(const KP& P, int R, int d) {
  const long cells_ = (long)P.nrows * P.C;
  static const bool win_forced = getenv("EMAP_POST_DMA_WINDOW") != nullptr || getenv("EMAP_POST_R") != nullptr;
  return post_use_dma(R, d) && (win_forced || (R == 16 && cells_ >= 3072L * 3072L && cells_ < 5120L * 5120L && P.C < 5120));
}
void launch_post(hipStream_t s, const KP& P, const float* w1, const float* w2, const float* w3, const float* wo, Cells cells,
                 float* trav_in, float* normal, long plane_stride, int d, int nseg, const int* seg_b, const int* seg_e, int stage, int tile_rows) {
  const TravW W = post_weights(w1, w2, w3, wo);
  int R = post_tile_rows(P);
  if (tile_rows == 4 || tile_rows == 8 || tile_rows == 16 || tile_rows == 32) { if (tile_rows < R && post_lds_bytes(tile_rows, d) <= 150 * 1024) R = tile_rows; }
  PostSegs S; memset(&S, 0, sizeof S);
  S.emagic = post_emagic(d);
  int tiles = 0;
  for (int k = 0; k < nseg && S.n < 4; ++k) {
    if (seg_e[k] <= seg_b[k]) continue;
    S.b[S.n] = seg_b[k]; S.e[S.n] = seg_e[k]; S.t0[S.n] = tiles; tiles += (seg_e[k] - seg_b[k] + R - 1) / R; S.n++;
  }
  if (!tiles) return;
  const bool dma = post_launch_dma(P, R, d);
  dim3 g((P.C + PT_C - 1) / PT_C, tiles), b(dma ? 512 : (R >= 32 ? POST_T32 : 512));
  const size_t lds = dma ? post_dma_lds_bytes(R, d) : post_lds_bytes(R, d);
#define POST_GO(KERN, RR, ST) do { auto kern = KERN<RR, ST>; static LdsRaised raised; \
    raise_lds(kern, raised, 158 * 1024); \
    hipLaunchKernelGGL(kern, g, b, lds, s, P, W, cells, trav_in, normal, plane_stride, d, S); } while (0)
#define POST_ALL(KERN) do { \
    if (stage == 1) { if (R == 4) POST_GO(KERN, 4, 1); else if (R == 8) POST_GO(KERN, 8, 1); else if (R == 32) POST_GO(KERN, 32, 1); else POST_GO(KERN, 16, 1); } \
    else { if (R == 4) POST_GO(KERN, 4, 0); else if (R == 8) POST_GO(KERN, 8, 0); else if (R == 32) POST_GO(KERN, 32, 0); else POST_GO(KERN, 16, 0); } } while (0)
  if (dma) POST_ALL(k_post_dma); else POST_ALL(k_post);
#undef POST_ALL
#undef POST_GO
}
// The whole map's stencil pass (launch_post: stage 0, the one interval [0, C), the tile height of post_tile_rows) as k_post_hist can run
// it: the tile height when that launch is the plain k_post<16, 0> or k_post<32, 0>, else 0.
int post_hist_tile_rows(const KP& P, int d) {
  if (P.nrows != P.C) return 0;
  const int R = post_tile_rows(P);
  return (R == 16 || R == 32) && !post_launch_dma(P, R, d) && post_lds_bytes(R, d) <= 150 * 1024 ? R : 0;
}
// workgroups of k_post_hist that are resident at once: what the occupancy calculator gives per CU x the CUs (per instantiation, LDS size and device;
// the kernel is a template VALUE: the instantiations share one pointer type, and a function per type would share one memo among them)
template <auto KERN> static long post_hist_resident(size_t lds, int dev) {
  struct Memo { bool on; size_t lds; long wg; };
  static Memo memo[EM_MAX_DEV];
  Memo& m = memo[dev >= 0 && dev < EM_MAX_DEV ? dev : 0];
  if (m.on && m.lds == lds) return m.wg;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(KERN), 512, lds) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  m.on = true; m.lds = lds; m.wg = (long)per_cu * cus;
  return m.wg;
}
// The stencil pass launch_post(.., whole map, stage 0) would run + launch_bin_hist of the next frame's cloud in one grid.  false: nothing
// was launched -- the stencil tiles and the histogram chunks are not resident together (or more than max_wg workgroups: test hook), and
// the caller runs the two launches.  out: the output set of the stencil tiles (POST_OUT_*); anything but POST_OUT_FULL leaves the pass owed.
bool launch_post_hist(hipStream_t s, int dev, const KP& P, const float* w1, const float* w2, const float* w3, const float* wo, Cells cells,
                      float* trav_in, float* normal, long plane_stride, int d, const Pose& T, const BinGeo& G, const float* pts, long n, int stride,
                      unsigned int* hist, long max_wg, int out, unsigned char* tflag) {
  const int R = post_hist_tile_rows(P, d);
  if (!R || (out == POST_OUT_TRAV && !tflag)) return false;
  const TravW W = post_weights(w1, w2, w3, wo);
  PostSegs S; memset(&S, 0, sizeof S);
  S.emagic = post_emagic(d);
  S.n = 1; S.b[0] = 0; S.e[0] = P.C; S.t0[0] = 0;
  // tiles in front, the histogram workgroups from the next multiple of 8 on (see k_post_hist); EMAP_POST_HIST_FRONT=1 (A/B knob): the
  // histogram workgroups in front, the tiles from the next multiple of 8 on
  static const bool hist_front = getenv("EMAP_POST_HIST_FRONT") && atoi(getenv("EMAP_POST_HIST_FRONT")) != 0;
  const int tiles_x = (P.C + PT_C - 1) / PT_C, n_tiles = tiles_x * ((P.C + R - 1) / R);
  const int tile0 = hist_front ? (G.B + 7) & ~7 : 0, hist0 = hist_front ? 0 : (n_tiles + 7) & ~7;
  const long grid = hist_front ? (long)tile0 + n_tiles : (long)hist0 + G.B;
  const size_t hist_lds = sizeof(unsigned int) * (size_t)G.pitch, lds = post_lds_bytes(R, d) > hist_lds ? post_lds_bytes(R, d) : hist_lds;
  if (lds > 158 * 1024) return false;
  bool ok = false;
#define POST_HIST_GO(MODE, RR, OO) do { auto kern = k_post_hist<MODE, RR, OO>; static LdsRaised raised; \
    if (!raise_lds(kern, raised, 158 * 1024) && lds > 64 * 1024) break; \
    const long room = post_hist_resident<k_post_hist<MODE, RR, OO>>(lds, dev); \
    if (grid > (max_wg > 0 && max_wg < room ? max_wg : room)) break; \
    hipLaunchKernelGGL(kern, dim3((unsigned int)grid), dim3(512), lds, s, P, W, cells, trav_in, normal, plane_stride, d, S, tiles_x, n_tiles, tile0, hist0, \
                       T, G, pts, n, stride, hist, tflag); ok = true; } while (0)
#define POST_HIST_OUT(MODE, RR) do { if (out == POST_OUT_TRAV) POST_HIST_GO(MODE, RR, POST_OUT_TRAV); \
    else if (out == POST_OUT_TRAV_WORD) POST_HIST_GO(MODE, RR, POST_OUT_TRAV_WORD); \
    else if (out == POST_OUT_TRAV_NORMALS) POST_HIST_GO(MODE, RR, POST_OUT_TRAV_NORMALS); else POST_HIST_GO(MODE, RR, POST_OUT_FULL); } while (0)
  if (P.mode == 0) { if (R == 32) POST_HIST_OUT(0, 32); else POST_HIST_OUT(0, 16); }
  else { if (R == 32) POST_HIST_OUT(1, 32); else POST_HIST_OUT(1, 16); }
#undef POST_HIST_OUT
#undef POST_HIST_GO
  return ok;
}
void launch_var_time(hipStream_t s, const KP& P, Cells cells, int do_var, int do_time) {
  hipLaunchKernelGGL(k_var_time, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, cells, do_var, do_time);
}
void launch_publish(hipStream_t s, const KP& P, Cells cells, const float* normal, long plane_stride, int kind, float center_z,
                    int only_above, float* out) {
  const long M = P.C - 2;
  hipLaunchKernelGGL(k_publish, dim3(nblk(M * M)), dim3(EM_BLOCK), 0, s, P, cells, normal, plane_stride, kind, center_z, only_above, out);
}
void launch_get_plane(hipStream_t s, const KP& P, Cells cells, int word, float* out) {
  hipLaunchKernelGGL(k_get_plane, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, cells, word, out);
}
void launch_set_plane(hipStream_t s, const KP& P, Cells cells, int word, const float* in) {
  hipLaunchKernelGGL(k_set_plane, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, cells, word, in);
}
void launch_fill_cells(hipStream_t s, Cells cells, long n, const Cell& v) {
  hipLaunchKernelGGL(k_fill_cells, dim3(nblk(n)), dim3(EM_BLOCK), 0, s, cells, n, v);
}
void launch_point_index(hipStream_t s, const KP& P, const Pose& T, const float* pts, long n, int stride, int* idx, unsigned char* flags) {
  if (n <= 0) return;
  if (P.mode == 0) hipLaunchKernelGGL(k_point_index<0>, dim3(nblk(n)), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, idx, flags);
  else hipLaunchKernelGGL(k_point_index<1>, dim3(nblk(n)), dim3(EM_BLOCK), 0, s, P, T, pts, n, stride, idx, flags);
}
void launch_plane_view(hipStream_t s, const KP& P, int org_r, int org_c, float* plane, float* view, int to_plane) {
  hipLaunchKernelGGL(k_plane_view, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, org_r, org_c, plane, view, to_plane);
}
void launch_materialize(hipStream_t s, const KP& P, Cells cells) {
  hipLaunchKernelGGL(k_materialize, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, cells);
}
void launch_band_clear(hipStream_t s, const KP& P, float* planes, int nl, long plane_stride, int sr, int sc) {
  if (nl > 0) hipLaunchKernelGGL(k_band_clear, dim3(nblk((long)P.nrows * P.C)), dim3(EM_BLOCK), 0, s, P, planes, nl, plane_stride, sr, sc);
}
