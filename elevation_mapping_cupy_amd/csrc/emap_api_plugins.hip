// C ABI of the MI355X elevation-map fusion core, host side of the publish-time plugins on caller planes (kernels: emap_semantic.hip):
// MinFilter / MaxFilter, SmoothFilter, Erosion, the Inpainting substitute, the safety polygon and the dilation of initialize_map.
#include "emap_host.h"
#include <cmath>
#include <vector>

using namespace emap_host;

// ---- safety polygon (reference elevation_mapping.py:837-889, polygon_mask_kernel custom_kernels.py:509-651) -------------
// get_idx of the polygon kernel (:587-603): float16 helper parameters, FLOAT resolution / width constants (unlike the map
// kernels), index clamped through float16.
int emap_host::polygon_cell(const emap_params& p, float x, float y, float cx, float cy, int* ix, int* iy) {
  const bool h = p.mode == EMAP_MODE_REFERENCE_FP16;
  auto Q = [&](float v) { return h ? q16(v) : v; };
  auto axis = [&](float v, float c) {
    const float q = (Q(v) - Q(c)) / (float)p.resolution;
    const double val = (double)q + 0.5 * (double)(float)p.cell_n;
    int i = (val != val) ? 0 : (int)fmin(fmax(val, -2147483648.0), 2147483647.0);
    float fi = Q((float)i);
    fi = fmaxf(fminf(fi, Q((float)(p.cell_n - 1))), Q(0.0f));
    return (int)fi;
  };
  const int idx = p.cell_n * axis(x, cx) + axis(y, cy);
  *ix = idx / p.cell_n; *iy = idx % p.cell_n;
  return idx;
}

extern "C" {

// ---- MinFilter plugin (EM/plugins/min_filter.py:84-118) on caller-provided planes ------------------------------------
static int minmax_filter(emap_ctx* ctx, const float* host_elevation, const float* host_valid, int32_t dilation_size, int32_t iteration_n,
                         float* host_out, int32_t* sweeps_run, bool is_max) {
  CKARG(ctx && host_out && ((host_elevation && host_valid) || (!host_elevation && !host_valid)), "null argument");
  CKARG(dilation_size >= 0 && dilation_size <= 32 && iteration_n >= 0 && iteration_n <= 4096, "bad filter size / iteration count");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_min_filter: single-strip contexts only");
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n; const size_t L = (size_t)C * C, bytes = L * sizeof(float);
  int rc = plugin_scratch(ctx, 5, iteration_n + 1); if (rc) return rc;
  float* buf = ctx->plug_buf; unsigned int* cnt = ctx->plug_cnt;
  float *orig = buf, *v0 = buf + L, *m0 = buf + 2 * L, *v1 = buf + 3 * L, *m1 = buf + 4 * L;
  if (host_elevation) {
    CK(hipMemcpyAsync(orig, host_valid, bytes, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(v0, host_elevation, bytes, hipMemcpyHostToDevice, ctx->stream));
  } else {                         // the map's own planes, de-interleaved on the device (no PCIe round trip of the inputs)
    FLUSH();
    launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 2, orig);
    launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 0, v0);
  }
  CK(hipMemcpyAsync(m0, orig, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  CK(hipMemsetAsync(cnt, 0, sizeof(unsigned int) * (iteration_n + 1), ctx->stream));
  for (int k = 0; k < iteration_n; ++k) {
    launch_min_sweep(ctx->stream, C, dilation_size, orig, (k & 1) ? v1 : v0, (k & 1) ? m1 : m0, (k & 1) ? v0 : v1, (k & 1) ? m0 : m1,
                     k > 0 ? cnt + (k - 1) : nullptr, cnt + k, is_max);
    CK(hipGetLastError());
  }
  const float* fv = (iteration_n & 1) ? v1 : v0; const float* fm = (iteration_n & 1) ? m1 : m0;
  std::vector<float> mask(L);
  std::vector<unsigned int> hc(iteration_n + 1);
  CK(hipMemcpyAsync(host_out, fv, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(mask.data(), fm, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(hc.data(), cnt, sizeof(unsigned int) * (iteration_n + 1), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < L; ++i) if (!(mask[i] > 0.5f)) host_out[i] = NAN;     // cp.where(mask > 0.5, filtered, nan), :116
  if (sweeps_run) { int n = 0; for (int k = 0; k < iteration_n; ++k) { ++n; if (hc[k] == 0) break; } *sweeps_run = n; }
  return EMAP_OK;
}

int emap_min_filter(emap_ctx* ctx, const float* host_elevation, const float* host_valid, int32_t dilation_size, int32_t iteration_n,
                    float* host_out, int32_t* sweeps_run) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  return minmax_filter(ctx, host_elevation, host_valid, dilation_size, iteration_n, host_out, sweeps_run, false);
}
int emap_max_filter(emap_ctx* ctx, const float* host_elevation, const float* host_valid, int32_t dilation_size, int32_t iteration_n,
                    float* host_out, int32_t* sweeps_run) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  return minmax_filter(ctx, host_elevation, host_valid, dilation_size, iteration_n, host_out, sweeps_run, true);
}

// ---- SmoothFilter plugin (EM/plugins/smooth_filter.py:56-58): `passes` x uniform_filter(size=3) on a host plane ---------------
int emap_smooth_filter(emap_ctx* ctx, const float* host_in, int32_t passes, float* host_out) {
  CKARG(ctx && host_in && host_out && passes >= 1 && passes <= 64, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n; const size_t L = (size_t)C * C, bytes = L * sizeof(float);
  DevBuf buf;
  CK(buf.alloc(bytes * 2));
  float *a = (float*)buf.d, *b = a + L;
  CK(hipMemcpyAsync(a, host_in, bytes, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < passes; ++k) { launch_box3(ctx->stream, C, a, b); CK(hipGetLastError()); float* t = a; a = b; b = t; }
  CK(hipMemcpyAsync(host_out, a, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

// ---- Erosion plugin (EM/plugins/erosion.py:96-104): cv2.erode with a k x k rectangle, `iterations` times, on a host plane ------
int emap_erode(emap_ctx* ctx, const float* host_in, int32_t kernel_size, int32_t iterations, float* host_out) {
  CKARG(ctx && host_in && host_out && kernel_size >= 1 && kernel_size <= 63 && iterations >= 0 && iterations <= 256, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n; const size_t L = (size_t)C * C, bytes = L * sizeof(float);
  DevBuf buf;
  CK(buf.alloc(bytes * 2));
  float *a = (float*)buf.d, *b = a + L;
  CK(hipMemcpyAsync(a, host_in, bytes, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < iterations; ++k) { launch_erode(ctx->stream, C, kernel_size, a, b); CK(hipGetLastError()); float* t = a; a = b; b = t; }
  CK(hipMemcpyAsync(host_out, a, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

// ---- Inpainting plugin substitute (see emap_semantic.hip): fill the pixels with known == 0 of an 8-bit image ---------
int emap_inpaint_u8(emap_ctx* ctx, const float* host_image, const float* host_known, int32_t max_sweeps, float* host_out,
                    int32_t* sweeps_run) {
  CKARG(ctx && host_image && host_known && host_out && max_sweeps >= 0 && max_sweeps <= 65536, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n; const size_t L = (size_t)C * C, bytes = L * sizeof(float);
  const int BATCH = 16;                      // sweeps between two looks at the unfilled counter
  int rc = plugin_scratch(ctx, 4, BATCH + 1); if (rc) return rc;
  float* buf = ctx->plug_buf; unsigned int* cnt = ctx->plug_cnt;
  float *v0 = buf, *m0 = buf + L, *v1 = buf + 2 * L, *m1 = buf + 3 * L;
  CK(hipMemcpyAsync(v0, host_image, bytes, hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(m0, host_known, bytes, hipMemcpyHostToDevice, ctx->stream));
  int done = 0; bool filled = false;
  std::vector<unsigned int> hc(BATCH + 1);
  while (done < max_sweeps && !filled) {      // the front usually closes after a few sweeps: stop launching once nothing is left
    const int nb = max_sweeps - done < BATCH ? max_sweeps - done : BATCH;
    CK(hipMemsetAsync(cnt, 0, sizeof(unsigned int) * (BATCH + 1), ctx->stream));
    for (int k = 0; k < nb; ++k) {
      const int g = done + k;
      launch_inpaint_sweep(ctx->stream, C, (g & 1) ? v1 : v0, (g & 1) ? m1 : m0, (g & 1) ? v0 : v1, (g & 1) ? m0 : m1,
                           k > 0 ? cnt + (k - 1) : nullptr, cnt + k);
      CK(hipGetLastError());
    }
    CK(hipMemcpyAsync(hc.data(), cnt, sizeof(unsigned int) * (BATCH + 1), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    int used = nb;
    for (int k = 0; k < nb; ++k) if (hc[k] == 0) { used = k + 1; filled = true; break; }
    done += nb;                               // sweeps after the closing one are copies: the result is the latest buffer either way
    if (sweeps_run) *sweeps_run = done - nb + used;
  }
  if (sweeps_run && max_sweeps == 0) *sweeps_run = 0;
  CK(hipMemcpyAsync(host_out, (done & 1) ? v1 : v0, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

// ---- safety polygon: the mask alone (the statistics on the device: emap_api_polysafe.hip) ------------------------------
int emap_polygon_mask(emap_ctx* ctx, const float* polygon_xy, int32_t n_vertices, float center_x, float center_y, float* host_mask) {
  CKARG(ctx && polygon_xy && host_mask && n_vertices >= 1 && n_vertices <= 4096, "bad polygon");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_polygon_mask: single-strip contexts only"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n;
  std::vector<int> v(2 * (size_t)n_vertices);
  float mn[2] = {polygon_xy[0], polygon_xy[1]}, mx[2] = {polygon_xy[0], polygon_xy[1]};
  for (int j = 0; j < n_vertices; ++j) {
    polygon_cell(ctx->prm, polygon_xy[2 * j], polygon_xy[2 * j + 1], center_x, center_y, &v[j], &v[n_vertices + j]);
    for (int a = 0; a < 2; ++a) { mn[a] = fminf(mn[a], polygon_xy[2 * j + a]); mx[a] = fmaxf(mx[a], polygon_xy[2 * j + a]); }
  }
  int bbox[4];
  polygon_cell(ctx->prm, mn[0], mn[1], center_x, center_y, &bbox[0], &bbox[1]);
  polygon_cell(ctx->prm, mx[0], mx[1], center_x, center_y, &bbox[2], &bbox[3]);
  DevBuf dvb;
  CK(dvb.alloc(sizeof(int) * v.size()));
  int* const dv = (int*)dvb.d;
  CK(hipMemcpyAsync(dv, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, ctx->stream));
  launch_polygon_mask(ctx->stream, C, dv, dv + n_vertices, n_vertices, bbox, ctx->scratch);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(host_mask, ctx->scratch, sizeof(float) * (size_t)C * C, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

// ---- dilation of caller planes: ElevationMap.initialize_map (reference elevation_mapping.py:899-923) ---------------------
int emap_dilate_planes(emap_ctx* ctx, const float* host_plane, const float* host_mask, int32_t dilation_size, int32_t iterations,
                       float* host_out, float* host_out_mask) {
  CKARG(ctx && host_plane && host_mask && host_out && host_out_mask, "null argument");
  CKARG(dilation_size >= 0 && dilation_size <= 64 && iterations >= 1 && iterations <= 64, "bad dilation size / iteration count"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n; const size_t L = (size_t)C * C, bytes = L * sizeof(float);
  DevBuf buf;
  CK(buf.alloc(bytes * 4));
  float *p0 = (float*)buf.d, *m0 = p0 + L, *p1 = p0 + 2 * L, *m1 = p0 + 3 * L;
  CK(hipMemcpyAsync(p0, host_plane, bytes, hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(m0, host_mask, bytes, hipMemcpyHostToDevice, ctx->stream));
  for (int it = 0; it < iterations; ++it) {
    launch_dilate_planes(ctx->stream, C, dilation_size, p0, m0, p1, m1);
    CK(hipGetLastError());
    float* t = p0; p0 = p1; p1 = t; t = m0; m0 = m1; m1 = t;
  }
  CK(hipMemcpyAsync(host_out, p0, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(host_out_mask, m0, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

}  // extern "C"
