// Depth-image input: the back-projection of a depth camera's frame on the device (emap_bind_depth_image, emap_api_depth.hip).
// Reference: sensor_processing/semantic_sensor/.../pointcloud_node.py:205-250 (create_pcl_from_image: validity rule, the pinhole
// expression, the nonzero order) and :261-269 (process_image: the colour's wire format).  The image is uploaded (2-4 bytes a pixel)
// instead of the cloud (12 + 4 Kc bytes a point), and the cloud is produced in the layout the frame kernels read: an (n, 3) xyz matrix
// and an (n, Kc) channel matrix (emap_device.h: ChanView).  Nothing is compacted: an invalid pixel becomes a row of quiet NaNs (bits
// 0x7FC00000), which every kernel of the frame skips like any NaN row of an uploaded cloud.
//
// Per sampled pixel (v, u) = (step r, step c), output row i = r Ws + c:
//   z = depth[v, u]                      (float32 metres)      or      z = (float)raw * depth_scale      (uint16: ONE float32 multiply)
//   valid = isfinite(z) && z > min_depth && z < max_depth && (no confidence || confidence[v, u] >= threshold)      (a NaN confidence: invalid)
//   x = (((float)u - cx) * z) / fx,  y = (((float)v - cy) * z) / fy,  z as is:  three float32 operations each, left to right, round to
//   nearest, never contracted (csrc/build.py: -ffp-contract=off; the division is hipcc's correctly rounded one, the default).
// Channels: [colour,] features[0 .. K): the colour's float has the BITS (r << 16) | (g << 8) | b; written for every row, valid or not.
//
// Float mode (read from the compiled code object, .amdhsa_float_denorm_mode_32 = 3 in every instantiation's kernel descriptor, the
// default of hipcc without -fgpu-flush-denormals-to-zero): float32 subnormals are KEPT, as inputs and as results, so the three
// operations round exactly like IEEE-754 binary32 on a host (NumPy) everywhere, gradual underflow included; the correctly rounded
// division's expansion scales its operands (v_div_scale / v_div_fixup) and is exact there as well.  The colour's float is a subnormal
// bit pattern by construction (< 2^24): it is only MOVED (integer ops and a store), never computed with, so no mode could flush it.
//
// k_depth_cloud<DT, CONF, QUAD> is INSTANTIATED on the depth type (0 float32, 1 uint16), on whether a confidence image is given, and
// on the lane shape, eight kernels, instead of branching uniformly: the type decides the WIDTH of the lane's depth load (16 or 8
// bytes), a template parameter keeps the confidence load out of the code of frames without one, and the two lane shapes share nothing
// but the per-pixel function.  The channel record (Kc, colour or not, 16-byte or dword stores) IS a uniform branch: its cost is a few
// scalar compares per lane against 4 Kc bytes of traffic, and instantiating it would multiply the eight by five.
//   QUAD (step == 1): rows are linear over the image (u = i % W, v = i / W), a lane takes the four consecutive rows 4j .. 4j + 3 (a
//   group may span a row end): one 16-byte (float32) / 8-byte (uint16) depth load, one 16-byte confidence load, and its 48 bytes of xyz
//   leave as three 16-byte stores -- the xyz matrix is 16-byte aligned, a wave writes 3 KB contiguous.  The last n % 4 rows are taken
//   one by one by the lane behind the last group (the scalar tail).
//   !QUAD (step > 1): one row per lane, dword loads and stores.
// Streaming and HBM-bound: 2-4 (+4) bytes read per pixel plus 3 + 4 K bytes of images, 12 + 4 Kc bytes written.  Plain C++ loads and
// stores only.
#include "emap_launch.h"

namespace {

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// one pixel: the contract's validity rule and pinhole expression, statement for statement
template <bool CONF>
__device__ __forceinline__ void back_project(const DepthArgs& A, int u, int v, float z, float conf, float& x, float& y, float& zo) {
  bool valid = isfinite(z) && z > A.min_depth && z < A.max_depth;
  if (CONF) valid = valid && conf >= A.conf_thr;
  const float px = (((float)u - A.cx) * z) / A.fx;
  const float py = (((float)v - A.cy) * z) / A.fy;
  x = valid ? px : quiet_nan(); y = valid ? py : quiet_nan(); zo = valid ? z : quiet_nan();
}

template <int DT>
__device__ __forceinline__ float depth_at(const DepthArgs& A, long pix) {
  if (DT == 0) return static_cast<const float*>(A.depth)[pix];
  return (float)static_cast<const unsigned short*>(A.depth)[pix] * A.depth_scale;
}

__device__ __forceinline__ float chan_value(const DepthArgs& A, long pix, int c) {
  if (A.has_rgb) {
    if (c == 0) { const unsigned char* q = A.rgb + 3 * pix; return __uint_as_float(((unsigned)q[0] << 16) | ((unsigned)q[1] << 8) | (unsigned)q[2]); }
    --c;
  }
  return A.feat[(long)c * A.plane + pix];
}

// the Kc-float record of output row i (image pixel pix): 16-byte stores where the records are 16-byte aligned (Kc % 4 == 0)
__device__ __forceinline__ void write_channels(const DepthArgs& A, long i, long pix) {
  const int Kc = A.has_rgb + A.n_feat;
  if (Kc == 0) return;
  float* o = A.chan + i * Kc;
  if ((Kc & 3) == 0) {
    for (int c = 0; c < Kc; c += 4)
      *reinterpret_cast<float4*>(o + c) = make_float4(chan_value(A, pix, c), chan_value(A, pix, c + 1), chan_value(A, pix, c + 2), chan_value(A, pix, c + 3));
  } else {
    for (int c = 0; c < Kc; ++c) o[c] = chan_value(A, pix, c);
  }
}

template <int DT, bool CONF>
__device__ __forceinline__ void one_row(const DepthArgs& A, long i, int u, int v) {
  const long pix = (long)v * A.W + u;
  float x, y, z;
  back_project<CONF>(A, u, v, depth_at<DT>(A, pix), CONF ? A.conf[pix] : 0.f, x, y, z);
  float* o = A.xyz + 3 * i;
  o[0] = x; o[1] = y; o[2] = z;
  write_channels(A, i, pix);
}

}  // namespace

template <int DT, bool CONF, bool QUAD>
__global__ __launch_bounds__(EM_BLOCK) void k_depth_cloud(DepthArgs A) {
  const long j = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (!QUAD) {
    if (j >= A.n) return;
    const int r = (int)(j / A.Ws), c = (int)(j - (long)r * A.Ws);
    one_row<DT, CONF>(A, j, c * A.step, r * A.step);
    return;
  }
  const long nq = A.n >> 2;      // (step == 1: n = H W, row i is pixel i)
  if (j > nq) return;
  const long i0 = 4 * j;
  int v = (int)(i0 / A.W), u = (int)(i0 - (long)v * A.W);
  if (j == nq) {                 // the scalar tail: rows 4 nq .. n - 1
    for (long i = i0; i < A.n; ++i) {
      one_row<DT, CONF>(A, i, u, v);
      if (++u == A.W) { u = 0; ++v; }
    }
    return;
  }
  float z[4], cf[4] = {0.f, 0.f, 0.f, 0.f};
  if (DT == 0) {
    const float4 d = static_cast<const float4*>(A.depth)[j];
    z[0] = d.x; z[1] = d.y; z[2] = d.z; z[3] = d.w;
  } else {
    const ushort4 d = static_cast<const ushort4*>(A.depth)[j];
    z[0] = (float)d.x * A.depth_scale; z[1] = (float)d.y * A.depth_scale; z[2] = (float)d.z * A.depth_scale; z[3] = (float)d.w * A.depth_scale;
  }
  if (CONF) {
    const float4 q = reinterpret_cast<const float4*>(A.conf)[j];
    cf[0] = q.x; cf[1] = q.y; cf[2] = q.z; cf[3] = q.w;
  }
  float o[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    back_project<CONF>(A, u, v, z[k], cf[k], o[3 * k], o[3 * k + 1], o[3 * k + 2]);
    write_channels(A, i0 + k, i0 + k);
    if (++u == A.W) { u = 0; ++v; }
  }
  float4* out = reinterpret_cast<float4*>(A.xyz + 3 * i0);
  out[0] = make_float4(o[0], o[1], o[2], o[3]);
  out[1] = make_float4(o[4], o[5], o[6], o[7]);
  out[2] = make_float4(o[8], o[9], o[10], o[11]);
}

template <int DT, bool CONF>
static void launch_dc(hipStream_t s, const DepthArgs& A) {
  if (A.step == 1) {
    const long lanes = (A.n >> 2) + ((A.n & 3) ? 1 : 0);
    hipLaunchKernelGGL((k_depth_cloud<DT, CONF, true>), dim3((unsigned)((lanes + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, A);
  } else {
    hipLaunchKernelGGL((k_depth_cloud<DT, CONF, false>), dim3((unsigned)((A.n + EM_BLOCK - 1) / EM_BLOCK)), dim3(EM_BLOCK), 0, s, A);
  }
}

void launch_depth_cloud(hipStream_t s, const DepthArgs& A, int depth_dtype) {
  if (A.n <= 0) return;
  const bool conf = A.conf != nullptr;
  if (depth_dtype == 0) { if (conf) launch_dc<0, true>(s, A); else launch_dc<0, false>(s, A); }
  else { if (conf) launch_dc<1, true>(s, A); else launch_dc<1, false>(s, A); }
}
