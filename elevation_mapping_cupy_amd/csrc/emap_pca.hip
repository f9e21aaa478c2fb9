// FeaturesPca on device-resident planes (gfx950): op EMAP_PLUGIN_FEATURES_PCA of a plugin chain (emap_api_plugchain.hip).  The plugin
// (EM/plugins/features_pca.py:66-96) downloads every matching layer, clips it to [-1, 1], fits scikit-learn's PCA(3) on the cell_n^2 x F
// matrix and scales each component to 0 .. 255 over the map.  The principal axes are the eigenvectors of the F x F matrix of centred
// second moments, so the map is read in passes and the eigenproblem is tiny:
//   1. k_pca_mean_parts / k_pca_mean_final    per-feature means
//   2. k_pca_mom_parts / k_pca_mom_final      sum (x_a - m_a)(x_b - m_b), b >= a, in a second pass over the planes (not E[x x^T] - m m^T)
//   3. k_pca_eig                              cyclic Jacobi in one wave, eigenvalues descending, three eigenvectors, the sign rule
//   4. k_pca_range_parts / k_pca_range_final  lo / hi of the three scores (x - m) . v over the map
//   5. k_pca_pack                             (uint8)((score - lo) / span * 255), packed 0x00RRGGBB
// All arithmetic is double on float32 inputs.  Every reduction is order-fixed -- a grid-stride sum per thread, a butterfly per wave, the
// waves of a workgroup and then the workgroups folded in index order; no float atomics -- so two runs on the same planes give the same
// bits.  The build compiles with -ffp-contract=off: the scores of pass 4 and pass 5 are the same doubles.
//
// Registers: 16 features have 136 moments, far beyond a lane's budget.  The moment pass splits the matrix over blockIdx.y: a workgroup
// owns ONE row a and keeps the sums against b = a .. F - 1, at most 16 doubles (32 VGPRs) per lane.  Per-lane arrays are indexed by
// unrolled constants only (the guards `b < F` are uniform), so nothing lives in scratch memory.
#include "emap_launch.h"

#define PCA_WAVES (EM_BLOCK / 64)
static_assert(EM_BLOCK == EM_PCA_F * EM_PCA_F && EM_BLOCK >= 3 * EM_PCA_F, "k_pca_mom_final: one thread per moment; pca_load_model: one per word");

__device__ __forceinline__ double pca_clip(float x) { return (double)(x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x)); }      // np.clip(layer, -1, 1) (:74), then float64
__device__ __forceinline__ long pca_cell(const KP& P, long li) {
  const int r = (int)(li / P.C), c = (int)(li - (long)r * P.C);
  return owned_cell(P, r, c);
}
__device__ __forceinline__ double pca_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// acc[0 .. 16) of every thread -> out[0 .. 16): butterfly per wave, then the waves in index order
__device__ __forceinline__ void pca_block_sums(double (&acc)[EM_PCA_F], double* __restrict__ out) {
  __shared__ double s_w[EM_PCA_F][PCA_WAVES];
#pragma unroll
  for (int b = 0; b < EM_PCA_F; ++b) {
    const double v = pca_wave_sum(acc[b]);
    if ((threadIdx.x & 63) == 0) s_w[b][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < EM_PCA_F) {
    double v = s_w[threadIdx.x][0];
    for (int w = 1; w < PCA_WAVES; ++w) v += s_w[threadIdx.x][w];
    out[threadIdx.x] = v;
  }
}

// ---- 1. means ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_pca_mean_parts(KP P, Cells cells, PlugSrcs S, double* __restrict__ parts) {
  const long L = (long)P.C * P.C;
  double acc[EM_PCA_F];
#pragma unroll
  for (int b = 0; b < EM_PCA_F; ++b) acc[b] = 0.0;
  for (long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x; li < L; li += (long)gridDim.x * EM_BLOCK) {
    const long ci = pca_cell(P, li);
#pragma unroll
    for (int b = 0; b < EM_PCA_F; ++b)
      if (b < S.n) acc[b] += pca_clip(plug_src_read(S, b, cells, L, li, ci));
  }
  pca_block_sums(acc, parts + (long)blockIdx.x * EM_PCA_F);
}
__global__ __launch_bounds__(64) void k_pca_mean_final(int n_parts, int F, long L, const double* __restrict__ parts, double* __restrict__ mean) {
  if (threadIdx.x >= EM_PCA_F) return;
  double v = 0.0;
  if (threadIdx.x < F) {
    for (int p = 0; p < n_parts; ++p) v += parts[(long)p * EM_PCA_F + threadIdx.x];
    v /= (double)L;
  }
  mean[threadIdx.x] = v;
}

// ---- 2. centred second moments: workgroup (x, a) sums (x_a - m_a)(x_b - m_b) for b >= a over its cells ---------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void k_pca_mom_parts(KP P, Cells cells, PlugSrcs S, const double* __restrict__ mean, double* __restrict__ parts) {
  __shared__ double s_m[EM_PCA_F];
  const long L = (long)P.C * P.C;
  const int a = blockIdx.y;
  if (threadIdx.x < EM_PCA_F) s_m[threadIdx.x] = mean[threadIdx.x];
  __syncthreads();
  double acc[EM_PCA_F];
#pragma unroll
  for (int b = 0; b < EM_PCA_F; ++b) acc[b] = 0.0;
  for (long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x; li < L; li += (long)gridDim.x * EM_BLOCK) {
    const long ci = pca_cell(P, li);
    const double da = pca_clip(plug_src_read(S, a, cells, L, li, ci)) - s_m[a];
#pragma unroll
    for (int b = 0; b < EM_PCA_F; ++b)
      if (b >= a && b < S.n) acc[b] += da * (pca_clip(plug_src_read(S, b, cells, L, li, ci)) - s_m[b]);
  }
  __syncthreads();
  pca_block_sums(acc, parts + ((long)blockIdx.x * EM_PCA_F + a) * EM_PCA_F);
}
__global__ __launch_bounds__(EM_BLOCK) void k_pca_mom_final(int n_parts, int F, const double* __restrict__ parts, double* __restrict__ cov) {
  const int a = threadIdx.x / EM_PCA_F, b = threadIdx.x % EM_PCA_F;
  if (a >= EM_PCA_F || b < a) return;
  double v = 0.0;
  if (b < F) for (int p = 0; p < n_parts; ++p) v += parts[((long)p * EM_PCA_F + a) * EM_PCA_F + b];
  cov[a * EM_PCA_F + b] = v; cov[b * EM_PCA_F + a] = v;
}

// ---- 3. the symmetric eigenproblem: cyclic Jacobi in one wave ------------------------------------------------------------------------------
// Every lane computes the rotation of the pair (p, q) from the same three LDS words; lane k < F then rotates columns p, q of row k of A
// and of V, and after a barrier rows p, q of column k of A (A' = J^T A J, V' = V J).  A sweep is the F (F - 1) / 2 pairs in row order; the
// sweeps end when the off-diagonal mass is below 1e-30 of the diagonal's (double: eps^2 = 5e-32) or after PCA_SWEEPS.  Lane 0 then
// takes the three largest eigenvalues (the lower index first among equals) and signs each eigenvector so that its entry of largest
// magnitude is positive, the first index among equals (sklearn.utils.extmath.svd_flip, v-based; plugins/features_pca.py: _pca3).
#define PCA_SWEEPS 30
__global__ __launch_bounds__(64) void k_pca_eig(int F, const double* __restrict__ cov, double* __restrict__ vec) {
  __shared__ double A[EM_PCA_F][EM_PCA_F + 1], V[EM_PCA_F][EM_PCA_F + 1];
  const int k = threadIdx.x;
  for (int e = k; e < EM_PCA_F * EM_PCA_F; e += 64) {
    const int i = e / EM_PCA_F, j = e % EM_PCA_F;
    A[i][j] = (i < F && j < F) ? cov[e] : 0.0; V[i][j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sweep = 0; sweep < PCA_SWEEPS; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < F; ++i)
      for (int j = 0; j < F; ++j) { const double v = A[i][j] * A[i][j]; if (i == j) dia += v; else off += v; }
    if (!(off > 1e-30 * dia)) break;                       // (uniform: every lane read the same words)
    for (int p = 0; p < F - 1; ++p)
      for (int q = p + 1; q < F; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        __syncthreads();
        if (apq == 0.0) continue;                          // (uniform)
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        if (k < F) {
          const double akp = A[k][p], akq = A[k][q], vkp = V[k][p], vkq = V[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
        __syncthreads();
        if (k < F) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = k == q ? 0.0 : c * apk - s * aqk; A[q][k] = k == p ? 0.0 : s * apk + c * aqk;      // (the pair's own element: zero by construction)
        }
        __syncthreads();
      }
  }
  __syncthreads();
  if (k == 0) {
    int used[3] = {-1, -1, -1};
    for (int comp = 0; comp < 3; ++comp) {
      int best = -1;
      for (int i = 0; i < F; ++i) {
        if (i == used[0] || i == used[1]) continue;
        if (best < 0 || A[i][i] > A[best][best]) best = i;
      }
      used[comp] = best;
      int big = 0;
      for (int f = 1; f < F; ++f) if (fabs(V[f][best]) > fabs(V[big][best])) big = f;
      const double sign = V[big][best] < 0.0 ? -1.0 : 1.0;
      for (int f = 0; f < EM_PCA_F; ++f) vec[comp * EM_PCA_F + f] = f < F ? sign * V[f][best] : 0.0;
    }
  }
}

// ---- 4. / 5. scores, their range, the packed levels ----------------------------------------------------------------------------------------
struct PcaModel { double m[EM_PCA_F]; double v[3][EM_PCA_F]; };
__device__ __forceinline__ void pca_load_model(PcaModel* M, const double* __restrict__ mean, const double* __restrict__ vec) {
  if (threadIdx.x < EM_PCA_F) M->m[threadIdx.x] = mean[threadIdx.x];
  if (threadIdx.x < 3 * EM_PCA_F) M->v[threadIdx.x / EM_PCA_F][threadIdx.x % EM_PCA_F] = vec[threadIdx.x];
  __syncthreads();
}
__device__ __forceinline__ void pca_scores(const PcaModel* M, const KP& P, const Cells& cells, const PlugSrcs& S, long L, long li, double (&sc)[3]) {
  const long ci = pca_cell(P, li);
  sc[0] = sc[1] = sc[2] = 0.0;
#pragma unroll
  for (int b = 0; b < EM_PCA_F; ++b)
    if (b < S.n) {
      const double d = pca_clip(plug_src_read(S, b, cells, L, li, ci)) - M->m[b];
      sc[0] += d * M->v[0][b]; sc[1] += d * M->v[1][b]; sc[2] += d * M->v[2][b];
    }
}
__device__ __forceinline__ void pca_range_fold(double (&lo)[3], double (&hi)[3], double* __restrict__ out) {
  __shared__ double s_r[6][PCA_WAVES];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double a = lo[j], b = hi[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64); a = oa < a ? oa : a; b = ob > b ? ob : b; }
    if ((threadIdx.x & 63) == 0) { s_r[j][threadIdx.x >> 6] = a; s_r[3 + j][threadIdx.x >> 6] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double v = s_r[threadIdx.x][0];
    for (int w = 1; w < PCA_WAVES; ++w) { const double o = s_r[threadIdx.x][w]; v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v); }
    out[threadIdx.x] = v;
  }
}
__global__ __launch_bounds__(EM_BLOCK) void k_pca_range_parts(KP P, Cells cells, PlugSrcs S, const double* __restrict__ mean, const double* __restrict__ vec,
                                                               double* __restrict__ parts) {
  __shared__ PcaModel M;
  pca_load_model(&M, mean, vec);
  const long L = (long)P.C * P.C;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x; li < L; li += (long)gridDim.x * EM_BLOCK) {
    double sc[3];
    pca_scores(&M, P, cells, S, L, li, sc);
#pragma unroll
    for (int j = 0; j < 3; ++j) { lo[j] = sc[j] < lo[j] ? sc[j] : lo[j]; hi[j] = sc[j] > hi[j] ? sc[j] : hi[j]; }
  }
  pca_range_fold(lo, hi, parts + (long)blockIdx.x * 6);
}
__global__ __launch_bounds__(EM_BLOCK) void k_pca_range_final(int n_parts, const double* __restrict__ parts, double* __restrict__ range) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int p = threadIdx.x; p < n_parts; p += EM_BLOCK) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double a = parts[(long)p * 6 + j], b = parts[(long)p * 6 + 3 + j];
      lo[j] = a < lo[j] ? a : lo[j]; hi[j] = b > hi[j] ? b : hi[j];
    }
  }
  pca_range_fold(lo, hi, range);
}
// ((comp - lo) / span * 255).astype(uint8) (:84-88): span = hi - lo where hi > lo, else 1; the cast truncates
__global__ __launch_bounds__(EM_BLOCK) void k_pca_pack(KP P, Cells cells, PlugSrcs S, const double* __restrict__ mean, const double* __restrict__ vec,
                                                        const double* __restrict__ range, float* __restrict__ dst) {
  __shared__ PcaModel M;
  pca_load_model(&M, mean, vec);
  const long L = (long)P.C * P.C;
  const long li = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (li >= L) return;
  double sc[3];
  pca_scores(&M, P, cells, S, L, li, sc);
  unsigned int rgb = 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double lo = range[j], hi = range[3 + j], span = hi > lo ? hi - lo : 1.0;
    rgb = (rgb << 8) | ((unsigned int)__double2int_rz((sc[j] - lo) / span * 255.0) & 255u);
  }
  dst[li] = __uint_as_float(rgb);
}

void launch_features_pca(hipStream_t s, const KP& P, Cells cells, const PlugSrcs& S, double* scratch, float* dst) {
  const long L = (long)P.C * P.C, nb = (L + EM_BLOCK - 1) / EM_BLOCK;
  const int n_parts = (int)(nb < EM_PCA_PARTS ? nb : EM_PCA_PARTS), F = S.n;
  double* mean_parts = scratch;
  double* mom_parts = mean_parts + (size_t)EM_PCA_PARTS * EM_PCA_F;
  double* range_parts = mom_parts + (size_t)EM_PCA_PARTS * EM_PCA_F * EM_PCA_F;
  double* mean = range_parts + (size_t)EM_PCA_PARTS * 6;
  double* cov = mean + EM_PCA_F;
  double* vec = cov + EM_PCA_F * EM_PCA_F;
  double* range = vec + 3 * EM_PCA_F;
  hipLaunchKernelGGL(k_pca_mean_parts, dim3(n_parts), dim3(EM_BLOCK), 0, s, P, cells, S, mean_parts);
  hipLaunchKernelGGL(k_pca_mean_final, dim3(1), dim3(64), 0, s, n_parts, F, L, mean_parts, mean);
  hipLaunchKernelGGL(k_pca_mom_parts, dim3(n_parts, F), dim3(EM_BLOCK), 0, s, P, cells, S, mean, mom_parts);
  hipLaunchKernelGGL(k_pca_mom_final, dim3(1), dim3(EM_BLOCK), 0, s, n_parts, F, mom_parts, cov);
  hipLaunchKernelGGL(k_pca_eig, dim3(1), dim3(64), 0, s, F, cov, vec);
  hipLaunchKernelGGL(k_pca_range_parts, dim3(n_parts), dim3(EM_BLOCK), 0, s, P, cells, S, mean, vec, range_parts);
  hipLaunchKernelGGL(k_pca_range_final, dim3(1), dim3(EM_BLOCK), 0, s, n_parts, range_parts, range);
  hipLaunchKernelGGL(k_pca_pack, dim3((unsigned int)nb), dim3(EM_BLOCK), 0, s, P, cells, S, mean, vec, range, dst);
}
