// C ABI of the MI355X elevation-map fusion core, host side of the image message input (kernel: emap_image_msg.hip): the raw bytes of a
// sensor_msgs/Image are uploaded as they are and ONE launch computes the correspondence and fuses every channel -- the reference's node
// converts the message to one float matrix per channel on the host (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:375-446) and
// input_image (EM/elevation_mapping.py:468-562) uploads the stack, then launches the correspondence kernel and one sampling kernel per
// channel.  The bytes pass through the context's image_stage (emap_host.h), the camera path's own.
#include "emap_host.h"
#include <cmath>
#include <cstring>

using namespace emap_host;

static bool cam_cell_ok(float v) { return std::isfinite(v) && v == truncf(v) && fabsf(v) <= (float)EM_CAM_CELL_MAX; }

extern "C" {

int emap_input_image_message(emap_ctx* ctx, const emap_image_msg_desc* d, const uint8_t* data, float x1, float y1, float z1,
                             const float P[12], const float K[9], const float D[5], const float center[3],
                             const emap_image_spec* specs, int32_t n_specs) {
  CKARG(ctx, "null ctx");
  // everything is refused BEFORE any copy or launch: correspondence and layers stay as they are
  CKARG(d && data && P && K && D && center && specs, "emap_input_image_message: null argument");
  CKARG(cam_cell_ok(x1) && cam_cell_ok(y1), "emap_input_image_message: camera cell (x1, y1) must be integer valued and within +-65536 cells");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_input_image_message: single-strip contexts only");
  CKARG(d->height >= 1 && d->height <= EM_IMGMSG_MAX_SIDE && d->width >= 1 && d->width <= EM_IMGMSG_MAX_SIDE, "emap_input_image_message: image sides must lie in 1 .. 8192");
  CKARG(d->elem >= 0 && d->elem <= 6, "emap_input_image_message: unknown element type (0 8U 1 8S 2 16U 3 16S 4 32S 5 32F 6 64F)");
  CKARG(d->n_chan >= 1 && d->n_chan <= 4, "emap_input_image_message: n_chan must lie in 1 .. 4");
  CKARG(!d->swap_rb || d->n_chan >= 3, "emap_input_image_message: swap_rb needs at least 3 channels");
  static const int size_of[7] = {1, 1, 2, 2, 4, 4, 8};
  const int esize = size_of[d->elem];
  CKARG((int64_t)d->step >= (int64_t)d->width * d->n_chan * esize, "emap_input_image_message: step is smaller than width * n_chan * element size");
  const int64_t bytes = (int64_t)d->height * d->step;
  CKARG(bytes < ((int64_t)1 << 31), "emap_input_image_message: height * step must stay below 2^31 bytes");
  CKARG(n_specs >= 1 && n_specs <= EM_IMGMSG_MAX_SPECS, "emap_input_image_message: n_specs must lie in 1 .. 4");
  bool colour = false;
  for (int k = 0; k < n_specs; ++k) {
    CKARG(specs[k].kind >= 0 && specs[k].kind <= 2, "emap_input_image_message: kind must be 0 (exponential), 1 (colour) or 2 (average)");
    CKARG(specs[k].layer >= 0 && specs[k].layer < ctx->sem_layers, "emap_input_image_message: layer is not configured");
    CKARG(specs[k].plane >= 0 && specs[k].plane < d->n_chan, "emap_input_image_message: plane must lie in 0 .. n_chan - 1");
    CKARG(specs[k].kind != 1 || d->n_chan >= 3, "emap_input_image_message: a colour entry needs at least 3 channels");
    colour = colour || specs[k].kind == 1;
  }
  CKARG((int64_t)d->height * d->width * (colour ? 3 : 1) <= EM_IMGMSG_MAX_INDEX,
        "emap_input_image_message: height * width (x 3 with a colour entry) beyond 2^24: the reference's float index arithmetic is not exact there");
  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const size_t L = (size_t)ctx->prm.cell_n * ctx->prm.cell_n;
  if (!ctx->img_uv) { CK(hipMalloc((void**)&ctx->img_uv, sizeof(float) * 2 * L)); CK(hipMalloc((void**)&ctx->img_valid, L)); }

  // EM_IMGMSG_SLACK behind the device copy: the kernel's aligned loads run up to the message's end rounded up
  Stage& st = ctx->image_stage;
  { const int rc = stage_next(ctx, &st, (size_t)bytes, (size_t)bytes + EM_IMGMSG_SLACK); if (rc) return rc; }
  { const int rc = stage_send(ctx, &st, data, (size_t)bytes); if (rc) return rc; }

  CamArgs A;
  memcpy(A.P, P, sizeof A.P); memcpy(A.K, K, sizeof A.K); memcpy(A.D, D, sizeof A.D); memcpy(A.center, center, sizeof A.center);
  A.x1 = x1; A.y1 = y1; A.z1 = z1; A.ih = (float)d->height; A.iw = (float)d->width; A.tol = ctx->img_tol_set ? ctx->img_tol : 0.10;
  ImgMsgArgs M; memset(&M, 0, sizeof M);
  M.msg = st.dev; M.H = d->height; M.W = d->width; M.step = d->step; M.elem = d->elem; M.esize = esize; M.n_chan = d->n_chan;
  M.big = d->is_bigendian ? 1 : 0; M.swap = d->swap_rb ? 1 : 0; M.n_specs = n_specs;
  for (int k = 0; k < n_specs; ++k) { M.e[k].kind = specs[k].kind; M.e[k].layer = specs[k].layer; M.e[k].plane = specs[k].plane; M.e[k].alpha = specs[k].alpha; }
  launch_image_frame(ctx->stream, ctx->kp, A, ctx->cells, ctx->img_uv, ctx->img_valid, M, ctx->sem, ctx->ncells_alloc);
  CK(hipGetLastError());
  return EMAP_OK;
}

}  // extern "C"
