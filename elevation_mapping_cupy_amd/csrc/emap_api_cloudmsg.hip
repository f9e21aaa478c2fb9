// C ABI of the MI355X elevation-map fusion core, host side of the PointCloud2 input (kernel: emap_cloudmsg.hip): the raw bytes of a
// sensor_msgs/PointCloud2 message are uploaded as they are and unpacked on the device into a cloud the context owns and binds -- the
// reference's node gathers them on the host, one point and one field at a time, into a float64 matrix
// (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:319-338) that input_pointcloud casts back to float32 and uploads.
// The message bytes pass through the context's cloud_stage, the produced cloud is its owned cloud (emap_host.h).
#include "emap_host.h"
#include <cstring>

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
  SF_CHECK();
  CK(hipSetDevice(ctx->device));

  CloudMsgArgs A; memset(&A, 0, sizeof A);
  // tight rows: the whole message is one row of n points
  if (d->row_step == tight) { A.rows = 1; A.width = (int)n; A.row_step = (long)bytes; }
  else { A.rows = d->height; A.width = d->width; A.row_step = d->row_step; }
  A.point_step = d->point_step; A.n_cols = d->n_cols; A.tile = cloud_unpack_tile(d->point_step); A.tiles_per_row = (A.width + A.tile - 1) / A.tile;
  for (int c = 0; c < d->n_cols; ++c) A.col[c] = (unsigned)d->offset[c] | ((unsigned)d->conv[c] << 16);
  const int Kc = d->n_cols - 3;
  const CloudLayout lay = cloud_layout((long)n, Kc);
  // 16 bytes of slack behind the device copy: the kernel's aligned 16-byte loads run up to the message's end rounded up
  { const int rc = owned_cloud_prepare(ctx, (size_t)bytes, (size_t)bytes + 16, lay.tot); if (rc) return rc; }
  { const int rc = stage_send(ctx, &ctx->cloud_stage, data, (size_t)bytes); if (rc) return rc; }
  A.msg = ctx->cloud_stage.dev; A.xyz = ctx->own_cloud; A.chan = Kc ? ctx->own_cloud + lay.chan_off : nullptr;
  launch_cloud_unpack(ctx->stream, A, aligned4);
  CK(hipGetLastError());
  bind_split_cloud(ctx, ctx->own_cloud, ctx->own_cloud + lay.chan_off, (long)n, (long)n, Kc);
  if (n_points_out) *n_points_out = n;
  return EMAP_OK;
}

}  // extern "C"
