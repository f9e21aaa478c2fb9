// C ABI of the MI355X elevation-map fusion core, host side of the PointCloud2 input (kernel: emap_cloudmsg.hip): the raw bytes of a
// sensor_msgs/PointCloud2 message are uploaded as they are and unpacked on the device into a cloud the context owns and binds -- the
// reference's node gathers them on the host, one point and one field at a time, into a float64 matrix
// (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:319-338) that input_pointcloud casts back to float32 and uploads.
// Only one cloud is bound at a time: the message bytes and the produced cloud live in the buffers of the depth-image input
// (emap_api_depth.hip: owned_cloud_prepare), under the same stream order.
#include "emap_host.h"
#include <cstring>
#include <functional>

using namespace emap_host;

extern "C" {

int emap_bind_cloud_message(emap_ctx* ctx, const emap_cloud_msg_desc* d, const uint8_t* data, int64_t* n_points_out) {
  CKARG(ctx, "null ctx");
  // everything is refused BEFORE any launch or copy: the previous binding stays as it is
  CKARG(d && data, "emap_bind_cloud_message: null argument");
  CKARG(d->is_bigendian == 0, "emap_bind_cloud_message: big-endian messages are not supported");
  CKARG(d->height >= 1 && d->width >= 1, "emap_bind_cloud_message: height and width must be at least 1");
  const int64_t n = (int64_t)d->height * d->width;
  CKARG(n <= EM_CLOUDMSG_MAX_POINTS, "emap_bind_cloud_message: at most 2^26 points");
  CKARG(d->point_step >= 1 && d->point_step <= EM_CLOUDMSG_MAX_STEP, "emap_bind_cloud_message: point_step must lie in 1 .. 256");
  const int64_t tight = (int64_t)d->width * d->point_step;
  CKARG(d->row_step >= tight, "emap_bind_cloud_message: row_step is smaller than width * point_step");
  const int64_t bytes = (int64_t)d->height * d->row_step;
  CKARG(bytes < ((int64_t)1 << 31), "emap_bind_cloud_message: height * row_step must stay below 2^31 bytes");
  CKARG(d->n_cols >= 3 && d->n_cols <= EM_CLOUDMSG_MAX_COLS, "emap_bind_cloud_message: n_cols must lie in 3 .. 19");
  static const int size_of[9] = {4, 1, 1, 2, 2, 4, 4, 4, 8};      // conv 0: the node's 4-byte memcpy; 1 .. 8: sensor_msgs/PointField datatypes
  bool aligned4 = d->point_step % 4 == 0 && (d->row_step == tight || d->row_step % 4 == 0);
  for (int c = 0; c < d->n_cols; ++c) {
    CKARG(d->conv[c] >= 0 && d->conv[c] <= 8, "emap_bind_cloud_message: unknown conv code");
    CKARG(d->offset[c] >= 0, "emap_bind_cloud_message: negative field offset");
    CKARG(d->offset[c] + size_of[d->conv[c]] <= d->point_step, "emap_bind_cloud_message: a column's bytes do not lie inside the point");
    aligned4 = aligned4 && d->offset[c] % 4 == 0 && size_of[d->conv[c]] == 4;
  }
  // the small frames in flight keep raw pointers to the cloud they read and may be re-run after an abort: settled before the owned
  // buffer is overwritten (as upload_impl does)
  SF_CHECK();
  CK(hipSetDevice(ctx->device));

  CloudMsgArgs A; memset(&A, 0, sizeof A);
  // tight rows: the whole message is one row of n points
  if (d->row_step == tight) { A.rows = 1; A.width = (int)n; A.row_step = (long)bytes; }
  else { A.rows = d->height; A.width = d->width; A.row_step = d->row_step; }
  A.point_step = d->point_step; A.n_cols = d->n_cols; A.tile = cloud_unpack_tile(d->point_step); A.tiles_per_row = (A.width + A.tile - 1) / A.tile;
  for (int c = 0; c < d->n_cols; ++c) A.col[c] = (unsigned)d->offset[c] | ((unsigned)d->conv[c] << 16);
  const int Kc = d->n_cols - 3;
  // the cloud as upload_impl lays it out: xyz (n, 3), the channel matrix behind it at a 256-byte boundary
  const long chan_off = Kc ? ((3 * (long)n + 63) & ~63L) : 0, tot = Kc ? chan_off + (long)Kc * n : 3 * (long)n;
  // 16 bytes of slack behind the device copy: the kernel's aligned 16-byte loads run up to the message's end rounded up
  int sl;
  { const int rc = owned_cloud_prepare(ctx, (size_t)bytes, (size_t)bytes + 16, tot, &sl); if (rc) return rc; }
  // A message of a million points is 16-32 MB: one host thread copying it into the pinned slot would take longer than its DMA.  So,
  // like the host cloud's upload (emap_api.hip: upload_impl), the worker threads copy it chunk by chunk, and each chunk's DMA -- on
  // the context's stream, in order -- overlaps the copy of the next; a message of one chunk is one memcpy and one DMA.
  unsigned char* pin = ctx->depth_pin[sl];
  const size_t total = (size_t)bytes, chunk = (size_t)2 << 20;
  if (total > chunk) { const int rc = upload_setup(ctx); if (rc) return rc; }
  for (size_t o = 0; o < total; o += chunk) {
    const size_t len = total - o < chunk ? total - o : chunk;
    if (total <= chunk) memcpy(pin, data, len);
    else ctx->workers->run([&](int w, int nw) {
      const size_t per = ((len + nw - 1) / nw + 63) & ~(size_t)63, a = (size_t)w * per;
      if (a < len) memcpy(pin + o + a, data + o + a, len - a < per ? len - a : per);
    });
    CK(hipMemcpyAsync(ctx->depth_img + o, pin + o, len, hipMemcpyHostToDevice, ctx->stream));
  }
  CK(hipEventRecord(ctx->depth_ev[sl], ctx->stream));
  ctx->depth_ev_on[sl] = true;
  A.msg = ctx->depth_img; A.xyz = ctx->depth_cloud; A.chan = Kc ? ctx->depth_cloud + chan_off : nullptr;
  launch_cloud_unpack(ctx->stream, A, aligned4);
  CK(hipGetLastError());
  // bound exactly as emap_bind_depth_image binds its cloud (a row-strip context: whole and unbucketed)
  ctx->pts = ctx->depth_cloud; ctx->n_pts = (long)n; ctx->stride = 3; ctx->n_cols = 3 + Kc; ctx->pts_bucketed = false; ctx->n_pts_all = (long)n;
  ctx->chan.p = Kc ? ctx->depth_cloud + chan_off : ctx->depth_cloud; ctx->chan.stride = Kc ? Kc : 3; ctx->chan.col0 = Kc ? 3 : 0;
  if (n_points_out) *n_points_out = n;
  return EMAP_OK;
}

}  // extern "C"
