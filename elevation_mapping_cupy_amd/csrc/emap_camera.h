// The per-cell correspondence of the camera path, shared by the two kernels that compute it: k_image_corr (emap_semantic.hip, the
// stand-alone launch of emap_image_correspondence) and k_image_frame (emap_image_msg.hip, the one-launch camera frame of
// emap_input_image_message).  image_to_map_correspondence_kernel (reference EM/kernels/custom_image_kernels.py:9-157): every known cell
// is projected into the image (P = K [R|t], optional radtan distortion) and a Bresenham walk towards the camera cell rejects it when
// terrain in between rises above the line of sight.  One body, so that both kernels produce the same uv / valid bit for bit.
#pragma once
#include "emap_launch.h"

__device__ __forceinline__ float l2_dist(int x0, int y0, int x1, int y1) { float dx = (float)(x0 - x1), dy = (float)(y0 - y1); return sqrtf(dx * dx + dy * dy); }

// logical cell i = x0 * C + y0 of a single-strip context: (u, v) and whether the cell sees the camera; (0, 0, false) for a cell that is
// not projected at all
__device__ __forceinline__ bool image_corr_cell(const KP& P, const CamArgs& A, const Cells& cells, long i, float& out_u, float& out_v) {
  const int W = P.C;
  out_u = 0.f; out_v = 0.f;
  int y0 = (int)(i % W), x0 = (int)(i / W);                              // logical cell; single-strip contexts: physical row = local row
  const Cell me = cells[(long)phys_row(P, x0) * W + phys_col(P, y0)];
  if (me.valid != 1.0f) return false;                                    // only cells with is_valid == 1 (:40-42)
  float p1 = (float)((double)(x0 - (W / 2)) * P.res + (double)A.center[0]);
  float p2 = (float)((double)(y0 - (W / 2)) * P.res + (double)A.center[1]);
  const float z0 = me.h;
  float p3 = z0 + A.center[2];
  float u = p1 * A.P[0] + p2 * A.P[1] + p3 * A.P[2] + A.P[3];
  float v = p1 * A.P[4] + p2 * A.P[5] + p3 * A.P[6] + A.P[7];
  float d = p1 * A.P[8] + p2 * A.P[9] + p3 * A.P[10] + A.P[11];
  if (d <= 0.f) return false;
  u = u / d; v = v / d;
  if (!(A.D[0] == 0.f && A.D[1] == 0.f && A.D[2] == 0.f && A.D[3] == 0.f && A.D[4] == 0.f)) {     // radtan (:66-86)
    const float k1 = A.D[0], k2 = A.D[1], q1 = A.D[2], q2 = A.D[3], k3 = A.D[4], fx = A.K[0], fy = A.K[4], cx = A.K[2], cy = A.K[5];
    float x = (u - cx) / fx, y = (v - cy) / fy;
    float r2 = x * x + y * y;
    float radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
    float uc = x * radial + 2 * q1 * x * y + q2 * (r2 + 2 * x * x);
    float vc = y * radial + 2 * q2 * x * y + q1 * (r2 + 2 * y * y);
    u = fx * uc + cx; v = fy * vc + cy;
  }
  if ((u < 0.f) || (v < 0.f) || (u >= A.iw) || (v >= A.ih)) return false;
  const int x0c = x0, y0c = y0;
  const float x1 = A.x1, y1 = A.y1;
  const float total_dis = l2_dist(x0c, y0c, (int)x1, (int)y1);
  const float delta_z = A.z1 - z0;
  const int dx = (int)fabsf(x1 - (float)x0), sx = (float)x0 < x1 ? 1 : -1, dy = -(int)fabsf(y1 - (float)y0), sy = (float)y0 < y1 ? 1 : -1;
  int error = dx + dy;
  bool ok = true;
  for (;;) {                                                               // Bresenham towards the camera cell (:103-147)
    if ((float)x0 == x1 && (float)y0 == y1) break;
    if (x0 >= 0 && y0 >= 0 && x0 < W && y0 < W) {
      const long idx = phys_col(P, y0) + (long)phys_row(P, x0) * W;
      const float4 hv = cells.hot[idx];     // h, (v), valid
      if (hv.z != 0.f) {
        float dis = l2_dist(x0c, y0c, x0, y0);
        float rayheight = z0 + (dis / total_dis * delta_z);
        if ((double)hv.x - A.tol > (double)rayheight) { ok = false; break; }
      }
    }
    const int e2 = 2 * error;
    if (e2 >= dy) { if ((float)x0 == x1) break; error += dy; x0 += sx; }
    if (e2 <= dx) { if ((float)y0 == y1) break; error += dx; y0 += sy; }
  }
  out_u = u; out_v = v;
  return ok;
}
