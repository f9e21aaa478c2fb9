// The inside test of the safety-polygon service: polygon_mask_kernel (reference EM/kernels/custom_kernels.py:509-651), shared by
// k_polygon_mask (emap_semantic.hip: the whole mask) and k_polysafe_tiles (emap_polysafe.hip: the statistics next to the cells).  The
// vertex and bounding-box cell indices depend only on the polygon, so the host computes them once with the reference's arithmetic
// (float16 helper parameters, fp32 division; emap_api_plugins.hip: polygon_cell); the per-cell test below is the reference's integer
// ray-crossing test, literally.
#pragma once
#include "emap_device.h"

struct PtI { int x, y; };
__device__ __forceinline__ bool pm_on_segment(PtI p, PtI q, PtI r) {
  return q.x <= max(p.x, r.x) && q.x >= min(p.x, r.x) && q.y <= max(p.y, r.y) && q.y >= min(p.y, r.y);
}
__device__ __forceinline__ int pm_orientation(PtI p, PtI q, PtI r) {
  int val = (q.y - p.y) * (r.x - q.x) - (q.x - p.x) * (r.y - q.y);
  if (val == 0) return 0;
  return (val > 0) ? 1 : 2;
}
__device__ __forceinline__ bool pm_intersect(PtI p1, PtI q1, PtI p2, PtI q2) {
  int o1 = pm_orientation(p1, q1, p2), o2 = pm_orientation(p1, q1, q2), o3 = pm_orientation(p2, q2, p1), o4 = pm_orientation(p2, q2, q1);
  if (o1 != o2 && o3 != o4) return true;
  if (o1 == 0 && pm_on_segment(p1, p2, q1)) return true;
  if (o2 == 0 && pm_on_segment(p1, q2, q1)) return true;
  if (o3 == 0 && pm_on_segment(p2, p1, q2)) return true;
  if (o4 == 0 && pm_on_segment(p2, q1, q2)) return true;
  return false;
}
// Is cell p = (row, column) inside the polygon of n vertex cells (vx[j], vy[j]) with the bounding box bmin .. bmax: the bbox cull and
// the loop of the reference's kernel.  vx / vy: global memory or LDS.
__device__ __forceinline__ bool pm_inside(PtI p, const int* vx, const int* vy, int n, int bminx, int bminy, int bmaxx, int bmaxy) {
  if (p.x < bminx || p.x > bmaxx || p.y < bminy || p.y > bmaxy) return false;
  const PtI extreme = {100000, p.y};
  int cnt = 0;
  for (int j = 0; j < n; ++j) {
    const int j2 = (j + 1) % n;
    PtI p1 = {vx[j], vy[j]}, p2 = {vx[j2], vy[j2]};
    if (pm_intersect(p1, p2, p, extreme)) {
      if (pm_orientation(p1, p, p2) == 0) {
        if (pm_on_segment(p1, p, p2)) return true;
      } else if (((p1.y <= p.y) && (p2.y > p.y)) || ((p1.y > p.y) && (p2.y <= p.y))) cnt++;
    }
  }
  return (cnt % 2) != 0;
}
