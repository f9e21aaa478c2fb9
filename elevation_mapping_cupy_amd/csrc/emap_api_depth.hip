// C ABI of the MI355X elevation-map fusion core, host side of the depth-image input (kernel: emap_depth.hip): a depth camera's frame
// is uploaded as IMAGES and back-projected on the device into a cloud the context owns and binds -- the reference back-projects on
// the host (sensor_processing/semantic_sensor/.../pointcloud_node.py:205-250, 261-269) and hands the float cloud to
// input_pointcloud.  Also the owned cloud of the doors that produce theirs (owned_cloud_prepare) and the read-back of whatever cloud
// is bound (emap_get_bound_points).
#include "emap_host.h"
#include <cmath>
#include <cstring>

using namespace emap_host;

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// The next slot of cloud_stage and the owned cloud of `tot` floats.  The small frames in flight keep raw pointers to the cloud they
// read and may be re-run after an abort: the caller has settled them (SF_CHECK) before the owned buffer is overwritten.
int emap_host::owned_cloud_prepare(emap_ctx* ctx, size_t pin_bytes, size_t dev_bytes, long tot) {
  const int rc = stage_next(ctx, &ctx->cloud_stage, pin_bytes, dev_bytes); if (rc) return rc;
  // a cloud about to be replaced must not stay bound
  if ((size_t)tot > ctx->own_cloud_cap && ctx->own_cloud && ctx->cloud.pts == ctx->own_cloud) { ctx->cloud.pts = nullptr; ctx->cloud.n = 0; ctx->cloud.n_all = 0; ctx->pts_bucketed = false; }
  return grow(ctx, &ctx->own_cloud, &ctx->own_cloud_cap, (size_t)tot);
}

extern "C" {

int emap_bind_depth_image(emap_ctx* ctx, const emap_depth_desc* d, const void* depth, const uint8_t* rgb_or_null, const float* features_or_null,
                          const float* confidence_or_null, int64_t* n_points_out) {
  CKARG(ctx, "null ctx");
  // everything is refused BEFORE any launch or copy: the previous binding stays as it is
  CKARG(d && depth, "emap_bind_depth_image: null argument");
  CKARG(d->height >= 1 && d->height <= EM_DEPTH_MAX_SIDE && d->width >= 1 && d->width <= EM_DEPTH_MAX_SIDE, "emap_bind_depth_image: image sides must lie in 1 .. 8192");
  CKARG(d->step >= 1 && d->step <= EM_DEPTH_MAX_STEP, "emap_bind_depth_image: step must lie in 1 .. 64");
  CKARG(d->depth_dtype == 0 || d->depth_dtype == 1, "emap_bind_depth_image: depth_dtype must be 0 (float32 metres) or 1 (uint16 units)");
  CKARG(std::isfinite(d->fx) && std::isfinite(d->fy) && d->fx != 0.f && d->fy != 0.f, "emap_bind_depth_image: fx, fy must be finite and non-zero");
  CKARG(std::isfinite(d->cx) && std::isfinite(d->cy) && std::isfinite(d->min_depth) && std::isfinite(d->max_depth), "emap_bind_depth_image: cx, cy, min_depth, max_depth must be finite");
  CKARG(d->min_depth >= 0.f && d->max_depth > d->min_depth, "emap_bind_depth_image: 0 <= min_depth < max_depth required");
  CKARG(d->depth_dtype == 0 || (std::isfinite(d->depth_scale) && d->depth_scale > 0.f), "emap_bind_depth_image: uint16 depth needs a finite depth_scale > 0");
  CKARG(d->n_features >= 0 && d->n_features <= EM_DEPTH_MAX_CHAN && (d->has_rgb ? 1 : 0) + d->n_features <= EM_DEPTH_MAX_CHAN,
        "emap_bind_depth_image: at most 16 channels (colour + features)");
  CKARG((!d->has_rgb || rgb_or_null) && (d->n_features == 0 || features_or_null), "emap_bind_depth_image: null channel image");
  SF_CHECK();
  CK(hipSetDevice(ctx->device));

  DepthArgs A; memset(&A, 0, sizeof A);
  A.H = d->height; A.W = d->width; A.step = d->step; A.Hs = (A.H + A.step - 1) / A.step; A.Ws = (A.W + A.step - 1) / A.step;
  A.n = (long)A.Hs * A.Ws; A.plane = (long)A.H * A.W; A.has_rgb = d->has_rgb ? 1 : 0; A.n_feat = d->n_features;
  A.fx = d->fx; A.fy = d->fy; A.cx = d->cx; A.cy = d->cy; A.depth_scale = d->depth_scale; A.min_depth = d->min_depth; A.max_depth = d->max_depth; A.conf_thr = d->confidence_threshold;
  const int Kc = A.has_rgb + A.n_feat;
  const size_t px = (size_t)A.plane;
  // the images in one block, every one at a 256-byte boundary: depth | confidence | features | rgb
  const size_t b_depth = px * (d->depth_dtype == 0 ? 4 : 2), b_conf = confidence_or_null ? px * 4 : 0, b_feat = px * 4 * (size_t)A.n_feat, b_rgb = A.has_rgb ? px * 3 : 0;
  const size_t o_conf = up256(b_depth), o_feat = o_conf + up256(b_conf), o_rgb = o_feat + up256(b_feat), img_bytes = o_rgb + up256(b_rgb);
  const CloudLayout lay = cloud_layout(A.n, Kc);

  { const int rc = owned_cloud_prepare(ctx, img_bytes, img_bytes, lay.tot); if (rc) return rc; }
  Stage& st = ctx->cloud_stage;
  unsigned char* pin = st.pin[st.slot];
  memcpy(pin, depth, b_depth);
  if (b_conf) memcpy(pin + o_conf, confidence_or_null, b_conf);
  if (b_feat) memcpy(pin + o_feat, features_or_null, b_feat);
  if (b_rgb) memcpy(pin + o_rgb, rgb_or_null, b_rgb);
  // one block when the images fill it (the gaps are < 256 bytes each): one DMA
  { const int rc = stage_send(ctx, &st, nullptr, img_bytes); if (rc) return rc; }
  A.depth = st.dev; A.conf = b_conf ? reinterpret_cast<const float*>(st.dev + o_conf) : nullptr;
  A.feat = b_feat ? reinterpret_cast<const float*>(st.dev + o_feat) : nullptr; A.rgb = b_rgb ? st.dev + o_rgb : nullptr;
  A.xyz = ctx->own_cloud; A.chan = Kc ? ctx->own_cloud + lay.chan_off : nullptr;
  launch_depth_cloud(ctx->stream, A, d->depth_dtype);
  CK(hipGetLastError());
  bind_split_cloud(ctx, ctx->own_cloud, ctx->own_cloud + lay.chan_off, A.n, A.n, Kc);
  if (n_points_out) *n_points_out = A.n;
  return EMAP_OK;
}

int emap_get_bound_points(emap_ctx* ctx, float* xyz_host, float* chan_host_or_null) {
  CKARG(ctx && xyz_host, "null argument"); SF_CHECK();
  if (!ctx->cloud.pts) { ctx->err = "no point cloud bound"; return EMAP_ERR_NO_POINTS; }
  CK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->cloud.n, K = (size_t)(ctx->cloud.n_cols - 3);
  if (n) {
    // rows of `stride` floats (xyz) / of chan.stride floats with the caller's column 3 at chan.p + 3 - col0 (emap_device.h: ChanView)
    if (ctx->cloud.stride == 3) CK(hipMemcpyAsync(xyz_host, ctx->cloud.pts, 12 * n, hipMemcpyDeviceToHost, ctx->stream));
    else CK(hipMemcpy2DAsync(xyz_host, 12, ctx->cloud.pts, sizeof(float) * (size_t)ctx->cloud.stride, 12, n, hipMemcpyDeviceToHost, ctx->stream));
    if (chan_host_or_null && K) {
      const float* src = ctx->cloud.chan.p + (3 - ctx->cloud.chan.col0);
      if ((size_t)ctx->cloud.chan.stride == K) CK(hipMemcpyAsync(chan_host_or_null, src, sizeof(float) * K * n, hipMemcpyDeviceToHost, ctx->stream));
      else CK(hipMemcpy2DAsync(chan_host_or_null, sizeof(float) * K, src, sizeof(float) * (size_t)ctx->cloud.chan.stride, sizeof(float) * K, n, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

}  // extern "C"
