/* TEST INFRASTRUCTURE ONLY -- CPU oracle; never linked into or called from the product path.
 *
 * Plain-C restatement of the per-frame hot path of leggedrobotics/elevation_mapping_cupy
 * (ElevationMap.update_map_with_kernel, reference elevation_mapping.py:316-391) with the DETERMINISTIC
 * TWO-PHASE CONTRACT documented in DESIGN.md ("Determinism contract"): the reference kernels race with
 * themselves (custom_kernels.py:170-192, 213-256); this file defines the one outcome the HIP kernels
 * must reproduce:
 *   A  count    (error_counting_kernel, custom_kernels.py:280-345)  reads the map of the previous frame
 *   A' gate     (elevation_mapping.py:346-357)                       host scalar logic
 *   B  fuse     (add_points_kernel fusion part, :160-197)            reads snapshot S0, writes accumulators only
 *   B' commit   (effects of :174, :189-192)                          per cell -> snapshot S1
 *   C  rays     (add_points_kernel visibility part, :198-259)        reads S1, writes accumulators only
 *   D  average  (average_map_kernel :348-389 + ray commit)           per cell
 *   then overlap clearance (elevation_mapping.py:393-410), dilation (:392-449), traversability
 *   (traversability_filter.py:8-47), normals (:452-506), update_variance / update_time (:420-426).
 * Arithmetic follows the reference expression by expression, including the CuPy `float16` helper-parameter
 * rounding (mode 0 = reference_fp16); mode 1 = fp32 is the same source with float16 := float.
 * Pinned by: oracle/ref_kernels (the reference source compiled for the host) on race-free fixtures and
 * order-independent outputs, see tests/test_oracle_vs_reference_source.py, and tests/golden/.
 *
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC  (see oracle/emap_oracle.py).
 * Map layout here is the reference's planar (7, C, C) float32; plane order
 * elevation, variance, is_valid, traversability, time, upper_bound, is_upper_bound (elevation_mapping.py:68-77).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  int32_t cell_n, mode;
  int32_t enable_edge_sharpen, enable_visibility_cleanup, enable_drift_compensation, enable_overlap_clearance;
  int32_t dilation_size, pad_;
  double resolution, sensor_noise_factor, mahalanobis_thresh, outlier_variance;
  double drift_compensation_variance_inlier, traversability_inlier, wall_num_thresh, max_ray_length;
  double cleanup_step, cleanup_cos_thresh, min_valid_distance, max_height_range;
  double ramped_height_range_a, ramped_height_range_b, ramped_height_range_c, max_variance;
  double initial_variance, time_variance, time_interval, min_height_drift_cnt;
  double max_drift, drift_compensation_alpha, position_noise_thresh, orientation_noise_thresh;
  double overlap_clear_range_xy, overlap_clear_range_z, ray_step, reserved_;
  float w1[36], w2[36], w3[36], w_out[12];
} eo_params;

/* ---- IEEE binary16 <-> binary32, round-to-nearest-even (what CuPy's float16(float) ctor does) ---- */
static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

uint16_t eo_f32_to_f16(float f) {
  uint32_t x = f2u(f), sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
  if (ax >= 0x7f800000u) return (uint16_t)(sign | (ax > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            /* >= 65520 rounds to inf */
  if (ax < 0x33000001u) return (uint16_t)sign;                           /* <= 2^-25 rounds to 0 */
  int e = (int)(ax >> 23) - 127;
  uint32_t m = (ax & 0x7fffffu) | 0x800000u;
  int shift = (e < -14) ? (13 + (-14 - e)) : 13;                         /* subnormal: extra shift */
  uint32_t r = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (r & 1))) r++;
  uint32_t h = (e < -14) ? r : ((uint32_t)(e + 15) << 10) + (r - 0x400u); /* carry propagates into exponent */
  return (uint16_t)(sign | h);
}
float eo_f16_to_f32(uint16_t h) {
  uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ffu;
  if (e == 0) { if (!m) return u2f(sign); float v = (float)m * 5.9604644775390625e-08f; return sign ? -v : v; }
  if (e == 31) return u2f(sign | 0x7f800000u | (m << 13));
  return u2f(sign | ((e + 112) << 23) | (m << 13));
}
#define Q(x) (P->mode == 0 ? eo_f16_to_f32(eo_f32_to_f16(x)) : (x))

static inline int sat_int(double v) {           /* CUDA float->int conversion saturates, NaN -> 0 */
  if (!(v == v)) return 0;
  if (v >= 2147483647.0) return 2147483647;
  if (v <= -2147483648.0) return (int)0x80000000;
  return (int)v;
}
/* map_utils.transform_p (custom_kernels.py:54-57): all seven arguments are float16 parameters */
static inline float transform_p(const eo_params* P, float x, float y, float z, float r0, float r1, float r2, float t) {
  return Q(r0) * Q(x) + Q(r1) * Q(y) + Q(r2) * Q(z) + Q(t);
}
/* get_x_idx / get_y_idx + clamp (custom_kernels.py:22-33, 45-49) */
static inline int axis_idx(const eo_params* P, float x, float c) {
  const int W = P->cell_n;
  float d = Q(x) - Q(c);
  if (P->mode != 0) {   /* fp32 mode, defined by this project for maps beyond the float16 range: float multiply, float add
                           (two roundings), truncation, integer clamp */
    volatile float m = d * (float)(1.0 / P->resolution);
    volatile float v = m + 0.5f * (float)W;
    int i = sat_int((double)v);
    return i < 0 ? 0 : (i > W - 1 ? W - 1 : i);
  }
  int i = sat_int((double)d / P->resolution + 0.5 * W);
  float fi = Q((float)i), lo = Q(0.0f), hi = Q((float)(W - 1));
  float r = fmaxf(fminf(fi, hi), lo);
  return (int)r;
}
static inline int get_idx(const eo_params* P, float x, float y, float cx, float cy) {
  return P->cell_n * axis_idx(P, x, cx) + axis_idx(P, y, cy);
}
static inline int is_inside(const eo_params* P, int idx) { /* custom_kernels.py:34-44 */
  const int W = P->cell_n;
  int ix = idx / W, iy = idx % W;
  return !(ix == 0 || ix == W - 1 || iy == 0 || iy == W - 1);
}
static inline float z_noise(const eo_params* P, float z) { /* :58-60 */
  double zz = (double)Q(z);
  return (float)(P->sensor_noise_factor * zz * zz);
}
static inline int is_valid(const eo_params* P, float x_, float y_, float z_, float sx_, float sy_, float sz_) { /* :62-81 */
  float x = Q(x_), y = Q(y_), z = Q(z_), sx = Q(sx_), sy = Q(sy_), sz = Q(sz_);
  float d = (x - sx) * (x - sx) + (y - sy) * (y - sy) + (z - sz) * (z - sz);
  float dxy = (float)fmax((double)sqrtf(x * x + y * y) - P->ramped_height_range_b, 0.0);
  if ((double)d < P->min_valid_distance * P->min_valid_distance) return 0;
  if ((double)(z - sz) > (double)dxy * P->ramped_height_range_a + P->ramped_height_range_c ||
      (double)(z - sz) > P->max_height_range) return 0;
  return 1;
}

typedef struct { float x, y, z, v; int idx, valid, inside, finite; } pt_t;

/* Optional OpenMP parallelism over points / cells for bench.py's cpu_baseline leg ("all cores"): eo_set_threads(n).
 * Every accumulator of the contract is an INTEGER -- counts, and the three sums in fixed point (drift error Q27.36, new heights
 * Q31.32, new variances and validity decrements Q23.40: each addend rounded to nearest once, llrint) -- so a result does not
 * depend on the order of the points or on the thread count, and the HIP kernels (which accumulate the same integers in LDS / HBM)
 * reproduce every plane BIT FOR BIT.  The reference itself accumulates with racing float32 atomics; any fixed summation order is
 * one outcome it can produce within a few ulp, and the restatement stays pinned to its compiled kernels within 1e-5. */
#define EO_SCALE_H 4294967296.0          /* 2^32 */
#define EO_SCALE_V 1099511627776.0       /* 2^40 */
#define EO_SCALE_E 68719476736.0         /* 2^36 */
static int g_threads = 1;
void eo_set_threads(int n) { g_threads = n < 1 ? 1 : n; }
static inline long long fix_of(double x, double scale) { return llrint(x * scale); }   /* round to nearest even, like __double2ll_rn */
static inline void atomic_max_u64(uint64_t* p, uint64_t v) {
  uint64_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
static inline void atomic_min_f32(float* p, float v) {   /* plain float min via CAS on the bit pattern */
  uint32_t* u = (uint32_t*)p; uint32_t old = __atomic_load_n(u, __ATOMIC_RELAXED);
  for (;;) { float f; memcpy(&f, &old, 4); if (!(v < f)) return; uint32_t nv; memcpy(&nv, &v, 4);
             if (__atomic_compare_exchange_n(u, &old, nv, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return; }
}

/* Row-strip view used by the multi-process (gloo) sharding tests: point / ray stages only touch cells whose row
 * (ix = idx / C) lies in [g_row0, g_row1).  Default = whole map. */
static int g_row0 = 0, g_row1 = 0x7fffffff;
void eo_set_strip(int row0, int row1) { g_row0 = row0; g_row1 = row1; }
static inline int owned(const eo_params* P, int idx) { int ix = idx / P->cell_n; return ix >= g_row0 && ix < g_row1; }

static inline pt_t point_geometry(const eo_params* P, const float* p, const float* R, const float* t) {
  pt_t o; memset(&o, 0, sizeof o);
  float rx = p[0], ry = p[1], rz = p[2];
  o.finite = !(isnan(rx) || isnan(ry) || isnan(rz)); /* rows with NaN are dropped: elevation_mapping.py:458 */
  if (!o.finite) { o.idx = -1; return o; }
  o.x = transform_p(P, rx, ry, rz, R[0], R[1], R[2], t[0]);
  o.y = transform_p(P, rx, ry, rz, R[3], R[4], R[5], t[1]);
  o.z = transform_p(P, rx, ry, rz, R[6], R[7], R[8], t[2]);
  o.v = z_noise(P, rz);
  o.idx = get_idx(P, o.x, o.y, 0.0f, 0.0f);  /* kernels always receive center 0 (elevation_mapping.py:337-338) */
  o.valid = is_valid(P, o.x, o.y, o.z, t[0], t[1], t[2]);
  o.inside = is_inside(P, o.idx);
  return o;
}

/* tail of add_points_kernel (custom_kernels.py:260-262), exported for the bit-exact index tests */
void eo_point_index(const eo_params* P, const float* pts, long n, long stride, const float* R, const float* t,
                    int32_t* idx, uint8_t* valid, uint8_t* inside) {
  for (long i = 0; i < n; ++i) {
    pt_t g = point_geometry(P, pts + i * stride, R, t);
    idx[i] = g.idx; valid[i] = (uint8_t)g.valid; inside[i] = (uint8_t)g.inside;
  }
}

/* Phase A: error_counting_kernel (custom_kernels.py:280-345). err_sum is accumulated in Q27.36 and returned as a double. */
void eo_count(const eo_params* P, const float* map, const float* pts, long n, long stride, const float* R,
              const float* t, uint32_t* n_pts, uint32_t* n_inl, double* err_sum, uint32_t* err_cnt) {
  const long L = (long)P->cell_n * P->cell_n;
  long long es = 0; unsigned long ec = 0;
#pragma omp parallel for num_threads(g_threads) reduction(+ : es, ec) schedule(static) if (g_threads > 1)
  for (long i = 0; i < n; ++i) {
    pt_t g = point_geometry(P, pts + i * stride, R, t);
    if (!g.finite || !g.valid || !g.inside || !owned(P, g.idx)) continue;
    float h = map[g.idx], v = map[L + g.idx], valid = map[2 * L + g.idx], trav = map[3 * L + g.idx];
    if (valid > 0.5f && (double)fabsf(h - g.z) < (double)v * P->mahalanobis_thresh &&
        (double)v < P->drift_compensation_variance_inlier / 2.0 && (double)trav > P->traversability_inlier) {
      es += fix_of((double)(g.z - h), EO_SCALE_E);
      ec += 1;
      __atomic_fetch_add(&n_inl[g.idx], 1u, __ATOMIC_RELAXED);
    }
    __atomic_fetch_add(&n_pts[g.idx], 1u, __ATOMIC_RELAXED);
  }
  *err_sum += (double)es / EO_SCALE_E; *err_cnt += (uint32_t)ec;
}

/* Phase A': drift gate (elevation_mapping.py:346-357). Returns the shift to add to plane 0 (0 if none);
 * *mean_out receives mean_error when the gate fired (else unchanged), *fired says whether it did. */
float eo_gate(const eo_params* P, double err_sum, uint32_t err_cnt, double position_noise, double orientation_noise,
              float* mean_out, int* fired) {
  *fired = 0;
  float cnt = (float)err_cnt;
  if (P->enable_drift_compensation && (double)cnt > P->min_height_drift_cnt &&
      (position_noise > P->position_noise_thresh || orientation_noise > P->orientation_noise_thresh)) {
    float mean = (float)err_sum / cnt;
    *mean_out = mean; *fired = 1;
    if ((double)fabsf(mean) < P->max_drift) return mean * (float)P->drift_compensation_alpha;
  }
  return 0.0f;
}

/* Phase B: fusion part of add_points_kernel (custom_kernels.py:160-197) against snapshot S0 = `map`
 * (drift shift already applied). Accumulators only; `latest_h` = new_h of the accepted point with the
 * largest input index (sequential last-writer of :191). */
void eo_fuse(const eo_params* P, const float* map, const float* pts, long n, long stride, const float* R,
             const float* t, const uint32_t* n_pts, long long* sum_h /* Q31.32 */, long long* sum_v /* Q23.40 */, uint32_t* cnt,
             uint32_t* n_out, float* latest_h) {
  const long L = (long)P->cell_n * P->cell_n;
  if (g_threads <= 1) {
    for (long i = 0; i < n; ++i) {
      pt_t g = point_geometry(P, pts + i * stride, R, t);
      if (!g.finite || !g.valid || !g.inside || !owned(P, g.idx)) continue;
      float map_h = map[g.idx], map_v = map[L + g.idx], num_points = (float)n_pts[g.idx];
      if ((double)fabsf(map_h - g.z) > (double)map_v * P->mahalanobis_thresh) { n_out[g.idx] += 1; continue; }
      if (P->enable_edge_sharpen && (double)num_points > P->wall_num_thresh &&
          (double)g.z < (double)map_h - (double)map_v * P->mahalanobis_thresh / (double)num_points) continue;
      float new_h = (map_h * g.v + g.z * map_v) / (map_v + g.v);
      float new_v = (map_v * g.v) / (map_v + g.v);
      sum_h[g.idx] += fix_of((double)new_h, EO_SCALE_H); sum_v[g.idx] += fix_of((double)new_v, EO_SCALE_V); cnt[g.idx] += 1;
      latest_h[g.idx] = new_h;
    }
    return;
  }
  uint64_t* key = calloc(L, 8);     /* ((i + 1) << 32) | bits(new_h): largest point index wins, as in the sequential loop */
#pragma omp parallel for num_threads(g_threads) schedule(static)
  for (long i = 0; i < n; ++i) {
    pt_t g = point_geometry(P, pts + i * stride, R, t);
    if (!g.finite || !g.valid || !g.inside || !owned(P, g.idx)) continue;
    float map_h = map[g.idx], map_v = map[L + g.idx], num_points = (float)n_pts[g.idx];
    if ((double)fabsf(map_h - g.z) > (double)map_v * P->mahalanobis_thresh) { __atomic_fetch_add(&n_out[g.idx], 1u, __ATOMIC_RELAXED); continue; }
    if (P->enable_edge_sharpen && (double)num_points > P->wall_num_thresh &&
        (double)g.z < (double)map_h - (double)map_v * P->mahalanobis_thresh / (double)num_points) continue;
    float new_h = (map_h * g.v + g.z * map_v) / (map_v + g.v);
    float new_v = (map_v * g.v) / (map_v + g.v);
    __atomic_fetch_add(&sum_h[g.idx], fix_of((double)new_h, EO_SCALE_H), __ATOMIC_RELAXED);
    __atomic_fetch_add(&sum_v[g.idx], fix_of((double)new_v, EO_SCALE_V), __ATOMIC_RELAXED);
    __atomic_fetch_add(&cnt[g.idx], 1u, __ATOMIC_RELAXED);
    atomic_max_u64(&key[g.idx], ((uint64_t)(i + 1) << 32) | f2u(new_h));
  }
#pragma omp parallel for num_threads(g_threads) schedule(static)
  for (long c = 0; c < L; ++c) if (key[c]) latest_h[c] = u2f((uint32_t)key[c]);
  free(key);
}

/* Phase B': per-cell commit of the fuse side effects -> snapshot S1 */
void eo_commit(const eo_params* P, float* map, const uint32_t* cnt, const uint32_t* n_out, const float* latest_h) {
  const long L = (long)P->cell_n * P->cell_n;
  const float ov = (float)P->outlier_variance;
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (long c = 0; c < L; ++c) {
    if (n_out[c]) map[L + c] = map[L + c] + ov * (float)n_out[c];
    if (cnt[c]) { map[2 * L + c] = 1.0f; map[4 * L + c] = 0.0f; map[5 * L + c] = latest_h[c]; map[6 * L + c] = 0.0f; }
  }
}

/* Phase C: visibility-cleanup part of add_points_kernel (custom_kernels.py:198-259) against snapshot S1.
 * Outputs (accumulators, applied by eo_average): ray_dec = sum of validity decrements (Q23.40),
 * ray_hits = number of penetrations, ray_upper = min qualifying nz (init +INF). */
void eo_rays(const eo_params* P, const float* map, const float* normal, const uint32_t* n_inl, const float* pts,
             long n, long stride, const float* R, const float* t, long long* ray_dec, uint32_t* ray_hits,
             float* ray_upper, uint64_t* visits_out) {
  const long L = (long)P->cell_n * P->cell_n;
  uint64_t visits = 0;
  const int mt = g_threads > 1;
#pragma omp parallel for num_threads(g_threads) reduction(+ : visits) schedule(dynamic, 256) if (g_threads > 1)
  for (long i = 0; i < n; ++i) {
    pt_t g = point_geometry(P, pts + i * stride, R, t);
    if (!g.finite || !g.valid) continue; /* invalid points march but never act (:226) */
    /* ray_vector(t, p) :83-101 -- every quantity below is a float16 variable in the reference */
    float tx = Q(t[0]), ty = Q(t[1]), tz = Q(t[2]), px = Q(g.x), py = Q(g.y), pz = Q(g.z);
    float vx = Q(px - tx), vy = Q(py - ty), vz = Q(pz - tz);
    float norm = Q(sqrtf(vx * vx + vy * vy + vz * vz));
    float rx = 0, ry = 0, rz = 0;
    if (norm > 0) { rx = Q(vx / norm); ry = Q(vy / norm); rz = Q(vz / norm); }
    float ray_length = Q(fminf(norm, Q((float)P->max_ray_length)));
    int last = -1;
    for (float s = Q((float)P->ray_step); s < ray_length; s = Q((float)((double)s + P->ray_step))) {
      float nx = t[0] + rx * s, ny = t[1] + ry * s, nz = t[2] + rz * s;
      int nidx = get_idx(P, nx, ny, 0.0f, 0.0f);
      if (nidx == last) continue;
      last = nidx;
      if (!is_inside(P, nidx) || !owned(P, nidx)) continue;
      visits++;
      float h = map[nidx], v = map[L + nidx], valid = map[2 * L + nidx], time = map[4 * L + nidx];
      float upper = map[5 * L + nidx], is_upper = map[6 * L + nidx];
      float d = Q((g.x - nx) * (g.x - nx) + (g.y - ny) * (g.y - ny) + (g.z - nz) * (g.z - nz));
      if ((double)d < 0.1) continue;
      if (valid < 0.5f) {
        if (nz < upper || is_upper < 0.5f) { if (mt) atomic_min_f32(&ray_upper[nidx], nz); else if (nz < ray_upper[nidx]) ray_upper[nidx] = nz; }
        continue;
      }
      if (time < 0.5f) continue;
      if ((double)h > (double)nz + 0.01 - fmin((double)v, 1.0) * 0.05) {
        float ip = Q(rx) * Q(normal[nidx]) + Q(ry) * Q(normal[L + nidx]) + Q(rz) * Q(normal[2 * L + nidx]);
        if ((double)fabsf(ip) < P->cleanup_cos_thresh) continue;
        if ((double)(float)n_inl[nidx] > P->wall_num_thresh && (double)time < 1.0) continue;
        const long long dec = fix_of((double)(float)(-P->cleanup_step / ((double)ray_length / P->max_ray_length)), EO_SCALE_V);
        if (mt) { __atomic_fetch_add(&ray_dec[nidx], dec, __ATOMIC_RELAXED); __atomic_fetch_add(&ray_hits[nidx], 1u, __ATOMIC_RELAXED); }
        else { ray_dec[nidx] += dec; ray_hits[nidx] += 1; }
        if (nz < upper || is_upper < 0.5f) { if (mt) atomic_min_f32(&ray_upper[nidx], nz); else if (nz < ray_upper[nidx]) ray_upper[nidx] = nz; }
      }
    }
  }
  if (visits_out) *visits_out = visits;
}

/* Phase D: ray commit + average_map_kernel (custom_kernels.py:348-389) */
void eo_average(const eo_params* P, float* map, const long long* sum_h, const long long* sum_v, const uint32_t* cnt,
                const long long* ray_dec, const uint32_t* ray_hits, const float* ray_upper) {
  const long L = (long)P->cell_n * P->cell_n;
  const float ov = (float)P->outlier_variance;
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (long c = 0; c < L; ++c) {
    if (ray_hits && ray_hits[c]) {
      map[2 * L + c] = map[2 * L + c] + (float)((double)ray_dec[c] / EO_SCALE_V);
      map[L + c] = map[L + c] + ov * (float)ray_hits[c];
    }
    if (ray_upper && ray_upper[c] < INFINITY) { map[5 * L + c] = ray_upper[c]; map[6 * L + c] = 1.0f; }
    float valid0 = map[2 * L + c];
    if (cnt[c] > 0) {
      float fc = (float)cnt[c];
      float nh = (float)(((double)sum_h[c] / EO_SCALE_H) / (double)cnt[c]), nv = (float)(((double)sum_v[c] / EO_SCALE_V) / (double)cnt[c]);
      (void)fc;
      if ((double)nv > P->max_variance) { map[c] = 0; map[L + c] = (float)P->initial_variance; map[2 * L + c] = 0; }
      else { map[c] = nh; map[L + c] = nv; map[2 * L + c] = 1; }
    }
    if (valid0 < 0.5f) { map[c] = 0; map[L + c] = (float)P->initial_variance; map[2 * L + c] = 0; }
  }
}

/* clear_overlap_map (elevation_mapping.py:393-410; window from :88-91) */
void eo_overlap_clear(const eo_params* P, float* map, float tz) {
  const int C = P->cell_n; const long L = (long)C * C;
  int cell_range = (int)(P->overlap_clear_range_xy / P->resolution);
  if (cell_range < 0) cell_range = 0; if (cell_range > C) cell_range = C;
  int cmin = C / 2 - cell_range / 2, cmax = C / 2 + cell_range / 2;
  /* t is a float32 array, range_z a python float: numpy/cupy keep float32 for array-scalar arithmetic */
  float hmin = tz - (float)P->overlap_clear_range_z, hmax = tz + (float)P->overlap_clear_range_z;
  for (int r = cmin; r < cmax; ++r) for (int c = cmin; c < cmax; ++c) {
    long i = (long)r * C + c;
    if (map[i] < hmin || map[i] > hmax) { map[i] = 0; map[L + i] = (float)P->initial_variance; map[2 * L + i] = 0; }
    if (map[5 * L + i] < hmin || map[5 * L + i] > hmax) { map[5 * L + i] = 0; map[6 * L + i] = 0; }
  }
}

/* dilation_filter_kernel (custom_kernels.py:392-449) incl. flat-index row wrap and signed dx+dy */
void eo_dilate(int C, int d, const float* plane, const float* mask, float* out, float* outmask) {
  const long L = (long)C * C;
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (long i = 0; i < L; ++i) {
    out[i] = plane[i];
    if (mask[i] < 0.5f) {
      float distance = 100, near_value = 0;
      for (int dy = -d; dy <= d; ++dy) for (int dx = -d; dx <= d; ++dx) {
        long j = i + (long)C * dy + dx;
        if (j < 0 || j >= L) continue;
        long jx = j / C, jy = j % C;
        if (jx <= 0 || jx >= C - 1 || jy <= 0 || jy >= C - 1) continue;
        if (mask[j] > 0.5f && (float)(dx + dy) < distance) { distance = (float)(dx + dy); near_value = plane[j]; }
      }
      if (distance < 100) { out[i] = near_value; if (outmask) outmask[i] = 1.0f; }
    }
  }
}

/* traversability filter (traversability_filter.py:8-47): three dilated 3x3 correlations (4 ch each, no bias,
 * no padding) -> abs -> 1x1 conv -> exp(-x); written to plane 3 interior [3:-3,3:-3] (elevation_mapping.py:385-388).
 * The reference runs this through torch.nn.Conv2d (cuDNN / MIOpen): neither the summation order nor the use of fused
 * multiply-adds is specified there, so the restatement fixes ONE order -- filter, channel, taps row-major, every step a fused
 * multiply-add (what GPU convolution kernels issue) -- and is pinned against torch's CPU fp32 convolution within 1e-5
 * (tests/test_oracle_golden.py).  On heights of magnitude H the orders differ by O(108 * ulp(H)), i.e. beyond 1e-5 for |H| > ~10 m. */
/* exp(-a), a >= 0: the reference calls torch.exp (traversability_filter.py:44), whose last bits differ between back ends.  The
 * restatement uses one fixed sequence of correctly rounded operations (rint, fmaf, ldexpf) that the HIP kernel repeats literally
 * (emap_kernels.hip: exp_neg), so the plane -- an input of the next frame's drift-inlier decision, custom_kernels.py:329 -- compares
 * bit for bit; within 3 ulp of expf (tests/test_oracle_golden.py pins it against expf / torch within 1e-5). */
static inline float exp_neg_det(float a) {
  const float x = -(!(a > 200.0f) ? a : 200.0f);
  const float n = rintf(x * 0x1.715476p+0f);
  float r = fmaf(n, -0x1.62e400p-1f, x);
  r = fmaf(n, -0x1.7f7d1cp-20f, r);
  float p = 0x1.6c16c2p-10f;
  p = fmaf(p, r, 0x1.111112p-7f);
  p = fmaf(p, r, 0x1.555556p-5f);
  p = fmaf(p, r, 0x1.555556p-3f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  return ldexpf(p, n == n ? (int)n : 0);
}
float eo_exp_neg(float a) { return exp_neg_det(a); }
void eo_traversability(const eo_params* P, const float* in, float* trav_plane) {
  const int C = P->cell_n;
  const float* w[3] = {P->w1, P->w2, P->w3};
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (int r = 3; r < C - 3; ++r) for (int c = 3; c < C - 3; ++c) {
    float acc = 0.0f;
    for (int k = 0; k < 3; ++k) { const int dl = k + 1;
      for (int ch = 0; ch < 4; ++ch) {
        float s = 0.0f;      /* fused multiply-adds, taps in row-major order: see the note above */
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b)
          s = fmaf(w[k][ch * 9 + a * 3 + b], in[(long)(r + (a - 1) * dl) * C + (c + (b - 1) * dl)], s);
        acc = fmaf(P->w_out[k * 4 + ch], fabsf(s), acc);
      } }
    trav_plane[(long)r * C + c] = exp_neg_det(acc);
  }
}

/* normal_filter_kernel (custom_kernels.py:452-506); `out` (3,C,C) is zeroed first (elevation_mapping.py:571) */
void eo_normals(const eo_params* P, const float* plane, const float* valid, float* out) {
  const int C = P->cell_n; const long L = (long)C * C;
  memset(out, 0, sizeof(float) * 3 * L);
  const float res = (float)P->resolution;
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (long i = 0; i < L; ++i) {
    if (!(valid[i] > 0.5f)) continue;
    long a = i + 1, b = i + C;
    if (b >= L) continue;
    long ax = a / C, ay = a % C, bx = b / C, by = b % C;
    if (ax <= 0 || ax >= C - 1 || ay <= 0 || ay >= C - 1) continue;
    if (bx <= 0 || bx >= C - 1 || by <= 0 || by >= C - 1) continue;
    float h = plane[i], dzdx = plane[a] - h, dzdy = plane[b] - h;
    float nx = -dzdy / res, ny = -dzdx / res;
    float nrm = sqrtf((nx * nx) + (ny * ny) + 1);
    out[i] = nx / nrm; out[L + i] = ny / nrm; out[2 * L + i] = 1.0f / nrm;
  }
}

void eo_update_variance(const eo_params* P, float* map) { /* elevation_mapping.py:420-422 */
  const long L = (long)P->cell_n * P->cell_n; const float tv = (float)P->time_variance;
  for (long c = 0; c < L; ++c) map[L + c] += tv * map[2 * L + c];
}
void eo_update_time(const eo_params* P, float* map) { /* :424-426 */
  const long L = (long)P->cell_n * P->cell_n; const float ti = (float)P->time_interval;
  for (long c = 0; c < L; ++c) map[4 * L + c] += ti;
}

/* ---- semantic point-cloud fusion (reference fusion/pointcloud_average.py, _class_average.py, _color.py and
 * custom_semantic_kernels.py:9-51,167-194,233-267,270-375). Points flagged valid&inside contribute. ---- */
void eo_sem_sum(const eo_params* P, const float* pts, long n, long stride, const float* R, const float* t,
                int n_ch, const int32_t* pcl_chan, const int32_t* layer, double* sums /* (n_layers_total, C, C) */) {
  const long L = (long)P->cell_n * P->cell_n;
  for (long i = 0; i < n; ++i) {
    pt_t g = point_geometry(P, pts + i * stride, R, t);
    if (!g.finite || !g.valid || !g.inside) continue;
    for (int k = 0; k < n_ch; ++k) sums[(long)layer[k] * L + g.idx] += (double)pts[i * stride + pcl_chan[k]];
  }
}
void eo_sem_average(const eo_params* P, const double* sums, const uint32_t* cnt, int n_ch, const int32_t* layer,
                    float* smap) {
  const long L = (long)P->cell_n * P->cell_n;
  for (long c = 0; c < L; ++c) if (cnt[c] > 0)
    for (int k = 0; k < n_ch; ++k) smap[(long)layer[k] * L + c] = (float)(sums[(long)layer[k] * L + c] / (double)cnt[c]);
}
void eo_sem_class_average(const eo_params* P, const double* sums, const uint32_t* cnt, int n_ch, const int32_t* layer,
                          double alpha, float* smap) {
  const long L = (long)P->cell_n * P->cell_n;
  for (long c = 0; c < L; ++c) if (cnt[c] > 0)
    for (int k = 0; k < n_ch; ++k) {
      long j = (long)layer[k] * L + c;
      float prev = smap[j];
      smap[j] = (prev == 0.0f) ? (float)(sums[j] / (double)cnt[c])
                               : (float)(alpha * (double)prev + (1.0 - alpha) * sums[j] / (double)cnt[c]);
    }
}
/* class_bayesian (reference fusion/pointcloud_class_bayesian.py:12-75): Dirichlet pseudo-counts.  The alpha kernel is launched
 * with size = N while decoding id = i / K, layer = i % K, so element (id, layer) exists only while id*K + layer < N; theta
 * below zero (or NaN) adds nothing.  `alpha` (the reference's persistent new_map layers) accumulates over frames; afterwards
 * every cell of the K layers is renormalised: semantic = alpha / (sum over the K layers, 1 where that sum is 0). */
void eo_sem_class_bayesian(const eo_params* P, const float* pts, long n, long stride, const float* R, const float* t,
                           int n_ch, const int32_t* pcl_chan, const int32_t* layer, float* alpha, float* smap) {
  const long L = (long)P->cell_n * P->cell_n;
  double* sums = (double*)calloc((size_t)n_ch * L, 8);
  for (long id = 0; id < n; ++id) {
    pt_t g = point_geometry(P, pts + id * stride, R, t);
    if (!g.finite || !g.valid || !g.inside) continue;
    for (int k = 0; k < n_ch; ++k) {
      if (id * n_ch + k >= n) continue;
      float theta = pts[id * stride + pcl_chan[k]];
      if (theta >= 0.0f) sums[(long)k * L + g.idx] += (double)theta;
    }
  }
  for (long c = 0; c < L; ++c) {
    float tot = 0.0f;
    for (int k = 0; k < n_ch; ++k) {
      long j = (long)layer[k] * L + c;
      alpha[j] = (float)((double)alpha[j] + sums[(long)k * L + c]);
      tot += alpha[j];
    }
    if (tot == 0.0f) tot = 1.0f;
    for (int k = 0; k < n_ch; ++k) { long j = (long)layer[k] * L + c; smap[j] = alpha[j] / tot; }
  }
  free(sums);
}
/* bayesian_inference (reference fusion/pointcloud_bayesian_inference.py:12-122), restated literally: the prior variance
 * lives in new_map layers that semantic_map.py:243 zeroes before every fusion, so sigma_old == 0 and the posterior mean
 * equals the old value (+ 0 * measurement mean, NaN if that mean is not finite); both kernels decode id = i / K. */
void eo_sem_bayesian_inference(const eo_params* P, const float* pts, long n, long stride, const float* R, const float* t,
                               const uint32_t* cnt, int n_ch, const int32_t* pcl_chan, const int32_t* layer, float* smap) {
  const long L = (long)P->cell_n * P->cell_n;
  double* sums = (double*)calloc((size_t)n_ch * L, 8);
  for (long id = 0; id < n; ++id) {
    pt_t g = point_geometry(P, pts + id * stride, R, t);
    if (!g.finite || !g.valid || !g.inside) continue;
    for (int k = 0; k < n_ch; ++k) if (id * n_ch + k < n) sums[(long)k * L + g.idx] += (double)pts[id * stride + pcl_chan[k]];
  }
  for (long c = 0; c < L; ++c) for (int k = 0; k < n_ch; ++k) {
    if (c * n_ch + k >= L || cnt[c] == 0) continue;
    const float cn = (float)cnt[c], feat_ml = (float)(sums[(long)k * L + c]) / cn, sigma_old = 0.0f, sigma = 1.0f;
    long j = (long)layer[k] * L + c;
    smap[j] = sigma * smap[j] / (cn * sigma_old + sigma) + cn * sigma_old * feat_ml / (cn * sigma_old + sigma);
  }
  free(sums);
}
/* colour (reference fusion/pointcloud_color.py:131-152; add_color_kernel + color_average_kernel, custom_semantic_kernels.py:270-375),
 * K packed 0x00RRGGBB channels as the reference LAUNCHES them: both kernels decode id = i / K, layer = i % K, but add_color runs over
 * size = N elements (not N * K) and color_average over size = C * C (not C * C * K).  So point id feeds layer l only while
 * id * K + l < N, cell id gets layer l only while id * K + l < C * C (the flat cell index: with K = 2 the upper half of the rows),
 * and ONE counter plane is incremented once per (point, layer) element -- the component sums of every layer are divided by the
 * elements of ALL layers in the cell (truncating integer division).  K = 1: the plain per-cell integer mean. */
void eo_sem_colors(const eo_params* P, const float* pts, long n, long stride, const float* R, const float* t,
                   int K, const int32_t* pcl_chan, const int32_t* layer, float* smap) {
  const long L = (long)P->cell_n * P->cell_n;
  uint32_t* acc = (uint32_t*)calloc((size_t)(3 * K + 1) * L, 4);
  for (long i = 0; i < n; ++i) {
    const long id = i / K; const int l = (int)(i % K);
    pt_t g = point_geometry(P, pts + id * stride, R, t);
    if (!g.finite || !g.valid || !g.inside) continue;
    uint32_t col = f2u(pts[id * stride + pcl_chan[l]]);
    acc[(long)(3 * l) * L + g.idx] += (col >> 16) & 0xff; acc[(long)(3 * l + 1) * L + g.idx] += (col >> 8) & 0xff;
    acc[(long)(3 * l + 2) * L + g.idx] += col & 0xff;
    acc[(long)(3 * K) * L + g.idx] += 1;
  }
  for (long i = 0; i < L; ++i) {
    const long id = i / K; const int l = (int)(i % K);
    const uint32_t k = acc[(long)(3 * K) * L + id];
    if (!k) continue;
    uint32_t r = acc[(long)(3 * l) * L + id] / k, g = acc[(long)(3 * l + 1) * L + id] / k, b = acc[(long)(3 * l + 2) * L + id] / k;
    smap[(long)layer[l] * L + id] = u2f((r << 16) + (g << 8) + b);
  }
  free(acc);
}
/* ---- safety polygon: polygon_mask_kernel (reference kernels/custom_kernels.py:509-651).  get_idx of THIS kernel divides in
 * fp32 (`const float resolution`), rounds coordinates / centre / index through float16 like the other helpers. ---- */
typedef struct { int x, y; } pt_i;
static int pm_axis(const eo_params* P, float v, float c) {
  float a = Q(v), b = Q(c);
  float q = (a - b) / (float)P->resolution;
  double val = (double)q + 0.5 * (double)(float)P->cell_n;
  int i = (int)val;
  float fi = Q((float)i), hi = Q((float)(P->cell_n - 1));
  fi = fmaxf(fminf(fi, hi), 0.0f);
  return (int)fi;
}
static int pm_on_segment(pt_i p, pt_i q, pt_i r) {
  return q.x <= (p.x > r.x ? p.x : r.x) && q.x >= (p.x < r.x ? p.x : r.x) && q.y <= (p.y > r.y ? p.y : r.y) && q.y >= (p.y < r.y ? p.y : r.y);
}
static int pm_orientation(pt_i p, pt_i q, pt_i r) {
  int val = (q.y - p.y) * (r.x - q.x) - (q.x - p.x) * (r.y - q.y);
  return val == 0 ? 0 : (val > 0 ? 1 : 2);
}
static int pm_intersect(pt_i p1, pt_i q1, pt_i p2, pt_i q2) {
  int o1 = pm_orientation(p1, q1, p2), o2 = pm_orientation(p1, q1, q2), o3 = pm_orientation(p2, q2, p1), o4 = pm_orientation(p2, q2, q1);
  if (o1 != o2 && o3 != o4) return 1;
  if (o1 == 0 && pm_on_segment(p1, p2, q1)) return 1;
  if (o2 == 0 && pm_on_segment(p1, q2, q1)) return 1;
  if (o3 == 0 && pm_on_segment(p2, p1, q2)) return 1;
  if (o4 == 0 && pm_on_segment(p2, q1, q2)) return 1;
  return 0;
}
void eo_polygon_mask(const eo_params* P, const float* polygon, int n, float cx, float cy, const float* bbox, float* mask) {
  const int C = P->cell_n;
  pt_i* v = (pt_i*)malloc(sizeof(pt_i) * (size_t)n);
  for (int j = 0; j < n; ++j) { v[j].x = pm_axis(P, polygon[2 * j], cx); v[j].y = pm_axis(P, polygon[2 * j + 1], cy); }
  pt_i bmin = {pm_axis(P, bbox[0], cx), pm_axis(P, bbox[1], cy)}, bmax = {pm_axis(P, bbox[2], cx), pm_axis(P, bbox[3], cy)};
  for (long i = 0; i < (long)C * C; ++i) {
    pt_i p = {(int)(i / C), (int)(i % C)}, extreme = {100000, p.y};
    if (p.x < bmin.x || p.x > bmax.x || p.y < bmin.y || p.y > bmax.y) { mask[i] = 0; continue; }
    int cnt = 0, on_edge = 0;
    for (int j = 0; j < n && !on_edge; ++j) {
      pt_i p1 = v[j], p2 = v[(j + 1) % n];
      if (pm_intersect(p1, p2, p, extreme)) {
        if (pm_orientation(p1, p, p2) == 0) { if (pm_on_segment(p1, p, p2)) on_edge = 1; }
        else if (((p1.y <= p.y) && (p2.y > p.y)) || ((p1.y > p.y) && (p2.y <= p.y))) cnt++;
      }
    }
    mask[i] = on_edge ? 1.0f : (cnt % 2 == 0 ? 0.0f : 1.0f);
  }
  free(v);
}

/* ---- camera path: image_to_map_correspondence_kernel (reference kernels/custom_image_kernels.py:9-157) and the
 * per-cell samplers exponential_/color_correspondences_to_map_kernel (:195-271).  Per-cell, race free.  The scalars
 * x1, y1 (camera cell, uint32 valued), z1, image_height, image_width arrive as float32 like in the reference call
 * (elevation_mapping.py:531-554). ---- */
static inline float l2_distance(int x0, int y0, int x1, int y1) { float dx = x0 - x1, dy = y0 - y1; return sqrtf(dx * dx + dy * dy); }
/* tol = tolerance_z_collision, the factory parameter of the kernel (:9); the reference's only call passes 0.10.  The walk ends only by
 * reaching (x1, y1): the Python wrapper refuses a camera cell that is not an integer within the library's cap, as the C ABI does. */
void eo_image_correspondence_tol(const eo_params* P, const float* map, float x1, float y1, float z1, const float* Pm, const float* K,
                                 const float* D, float image_height, float image_width, const float* center, double tol, float* uv,
                                 uint8_t* valid) {
  const int W = P->cell_n; const long L = (long)W * W;
  const double res = P->resolution;
  for (long i = 0; i < L; ++i) {
    if (map[2 * L + i] != 1) continue;
    int y0 = (int)(i % W), x0 = (int)(i / W);
    float p1 = (float)((x0 - (W / 2)) * res + center[0]);
    float p2 = (float)((y0 - (W / 2)) * res + center[1]);
    float p3 = map[i] + center[2];
    float u = p1 * Pm[0] + p2 * Pm[1] + p3 * Pm[2] + Pm[3];
    float v = p1 * Pm[4] + p2 * Pm[5] + p3 * Pm[6] + Pm[7];
    float d = p1 * Pm[8] + p2 * Pm[9] + p3 * Pm[10] + Pm[11];
    if (d <= 0) continue;
    u = u / d; v = v / d;
    int d_zero = (D[0] == 0 && D[1] == 0 && D[2] == 0 && D[3] == 0 && D[4] == 0);
    if (!d_zero) {
      float k1 = D[0], k2 = D[1], q1 = D[2], q2 = D[3], k3 = D[4], fx = K[0], fy = K[4], cx = K[2], cy = K[5];
      float x = (u - cx) / fx, y = (v - cy) / fy;
      float r2 = x * x + y * y;
      float radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
      float uc = x * radial + 2 * q1 * x * y + q2 * (r2 + 2 * x * x);
      float vc = y * radial + 2 * q2 * x * y + q1 * (r2 + 2 * y * y);
      u = fx * uc + cx; v = fy * vc + cy;
    }
    if ((u < 0) || (v < 0) || (u >= image_width) || (v >= image_height)) continue;
    const int y0c = y0, x0c = x0;
    float total_dis = l2_distance(x0c, y0c, (int)x1, (int)y1);
    float z0 = map[i], delta_z = z1 - z0;
    int dx = (int)fabsf(x1 - x0), sx = x0 < x1 ? 1 : -1, dy = -(int)fabsf(y1 - y0), sy = y0 < y1 ? 1 : -1, error = dx + dy;
    int ok = 1;
    for (;;) {
      if (x0 == x1 && y0 == y1) break;
      if (x0 >= 0 && y0 >= 0 && x0 < W && y0 < W) {
        long idx = y0 + (long)x0 * W;
        if (map[2 * L + idx]) {
          float dis = l2_distance(x0c, y0c, x0, y0);
          float rayheight = z0 + (dis / total_dis * delta_z);
          if ((double)map[idx] - tol > (double)rayheight) { ok = 0; break; }
        }
      }
      int e2 = 2 * error;
      if (e2 >= dy) { if (x0 == x1) break; error += dy; x0 += sx; }
      if (e2 <= dx) { if (y0 == y1) break; error += dx; y0 += sy; }
    }
    uv[i] = u; uv[L + i] = v; valid[i] = (uint8_t)ok;
  }
}
void eo_image_correspondence(const eo_params* P, const float* map, float x1, float y1, float z1, const float* Pm, const float* K,
                             const float* D, float image_height, float image_width, const float* center, float* uv, uint8_t* valid) {
  eo_image_correspondence_tol(P, map, x1, y1, z1, Pm, K, D, image_height, image_width, center, 0.10, uv, valid);
}
/* kind 0: exponential (alpha), image = (H, W) plane; kind 1: colour, image = (3, H, W) planes; updates `sem` in place */
void eo_image_fuse(const eo_params* P, int kind, float* sem, const float* image, const float* uv, const uint8_t* valid,
                   float image_height, float image_width, double alpha) {
  const long L = (long)P->cell_n * P->cell_n;
  for (long i = 0; i < L; ++i) {
    if (!valid[i]) continue;
    int idx = (int)((float)(int)uv[i] + (float)(int)uv[L + i] * image_width);
    if (kind == 0) sem[i] = (float)((double)sem[i] * (1 - alpha) + alpha * (double)image[idx]);
    else if (kind == 2) sem[i] = image[idx];      /* average_correspondences_to_map_kernel (custom_image_kernels.py:160-192): despite its name, a plain replace */
    else {
      int ig = (int)(image_width * image_height + (float)idx), ib = (int)(image_width * image_height * 2 + (float)idx);
      unsigned int r = (unsigned int)image[idx], g = (unsigned int)image[ig], b = (unsigned int)image[ib];
      sem[i] = u2f((r << 16) + (g << 8) + b);
    }
  }
}

/* MinFilter plugin (reference plugins/min_filter.py:29-118), Jacobi sweeps (every cell reads the previous sweep). */
static int eo_minmax_filter(int C, int d, int iteration_n, const float* elevation, const float* valid, float* out, int is_max);
int eo_min_filter(int C, int d, int iteration_n, const float* elevation, const float* valid, float* out) {
  return eo_minmax_filter(C, d, iteration_n, elevation, valid, out, 0);
}
/* MaxFilter plugin (reference plugins/max_filter.py:36-112): maximum, the RUNNING mask decides which cells are filled, inputs are
 * copies (out of place) in the reference too. */
int eo_max_filter(int C, int d, int iteration_n, const float* elevation, const float* valid, float* out) {
  return eo_minmax_filter(C, d, iteration_n, elevation, valid, out, 1);
}
static int eo_minmax_filter(int C, int d, int iteration_n, const float* elevation, const float* valid, float* out, int is_max) {
  const long L = (long)C * C;
  float* v0 = malloc(L * 4); float* m0 = malloc(L * 4); float* v1 = malloc(L * 4); float* m1 = malloc(L * 4);
  memcpy(v0, elevation, L * 4); memcpy(m0, valid, L * 4);
  int sweeps = 0;
  for (int k = 0; k < iteration_n; ++k) {
    long open_cells = 0;
    for (long i = 0; i < L; ++i) {
      float v = v0[i], m = m0[i];
      if ((is_max ? m : valid[i]) < 0.5f) {
        float mn = is_max ? -1000000.0f : 1000000.0f;
        for (int dy = -d; dy <= d; ++dy) for (int dx = -d; dx <= d; ++dx) {
          long j = i + (long)C * dy + dx;
          if (j < 0 || j >= L) continue;
          long jx = j / C, jy = j % C;
          if (jx <= 0 || jx >= C - 1 || jy <= 0 || jy >= C - 1) continue;
          if (m0[j] > 0.5f && (is_max ? v0[j] > mn : v0[j] < mn)) mn = v0[j];
        }
        if (is_max ? (mn > -1000000.0f + 1.0f) : (mn < 1000000.0f - 1.0f)) { v = mn; m = 0.6f; }
      }
      v1[i] = v; m1[i] = m; open_cells += !(m > 0.5f);
    }
    float* t; t = v0; v0 = v1; v1 = t; t = m0; m0 = m1; m1 = t;
    ++sweeps;
    if (open_cells == 0) break;
  }
  for (long i = 0; i < L; ++i) out[i] = (m0[i] > 0.5f) ? v0[i] : NAN;
  free(v0); free(m0); free(v1); free(m1);
  return sweeps;
}

/* ---- one whole frame (what bench.py's cpu_baseline leg times) ---------------------------------------- */
typedef struct { double err_sum; uint32_t err_cnt; int32_t gate_fired; float mean_error; float shift; uint64_t ray_visits; } eo_stats;

void eo_frame(const eo_params* P, float* map, float* normal, float* trav_input, const float* pts, long n, long stride,
              const float* R, const float* t, double position_noise, double orientation_noise, eo_stats* st) {
  const int C = P->cell_n; const long L = (long)C * C;
  uint32_t* n_pts = calloc(L, 4); uint32_t* n_inl = calloc(L, 4); uint32_t* cnt = calloc(L, 4); uint32_t* n_out = calloc(L, 4);
  long long* sum_h = calloc(L, 8); long long* sum_v = calloc(L, 8); float* latest = calloc(L, 4);
  memset(st, 0, sizeof *st);
  eo_count(P, map, pts, n, stride, R, t, n_pts, n_inl, &st->err_sum, &st->err_cnt);
  st->shift = eo_gate(P, st->err_sum, st->err_cnt, position_noise, orientation_noise, &st->mean_error, &st->gate_fired);
  if (st->shift != 0.0f) {
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
    for (long c = 0; c < L; ++c) map[c] += st->shift;
  }
  eo_fuse(P, map, pts, n, stride, R, t, n_pts, sum_h, sum_v, cnt, n_out, latest);
  eo_commit(P, map, cnt, n_out, latest);
  long long* ray_dec = NULL; uint32_t* ray_hits = NULL; float* ray_upper = NULL;
  if (P->enable_visibility_cleanup) {
    ray_dec = calloc(L, 8); ray_hits = calloc(L, 4); ray_upper = malloc(L * 4);
    for (long c = 0; c < L; ++c) ray_upper[c] = INFINITY;
    eo_rays(P, map, normal, n_inl, pts, n, stride, R, t, ray_dec, ray_hits, ray_upper, &st->ray_visits);
  }
  eo_average(P, map, sum_h, sum_v, cnt, ray_dec, ray_hits, ray_upper);
  if (P->enable_overlap_clearance) eo_overlap_clear(P, map, t[2]);
  float* mask = malloc(L * 4);
#pragma omp parallel for num_threads(g_threads) schedule(static) if (g_threads > 1)
  for (long c = 0; c < L; ++c) mask[c] = map[2 * L + c] + map[6 * L + c];
  memset(trav_input, 0, L * 4);
  eo_dilate(C, P->dilation_size, map + 5 * L, mask, trav_input, NULL);
  eo_traversability(P, trav_input, map + 3 * L);
  eo_normals(P, trav_input, map + 2 * L, normal);
  free(n_pts); free(n_inl); free(cnt); free(n_out); free(sum_h); free(sum_v); free(latest); free(mask);
  free(ray_dec); free(ray_hits); free(ray_upper);
}
