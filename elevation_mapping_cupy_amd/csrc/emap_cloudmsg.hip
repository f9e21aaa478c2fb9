// PointCloud2 input: the raw bytes of a sensor_msgs/PointCloud2 message unpacked on the device (emap_bind_cloud_message,
// emap_api_cloudmsg.hip).  Reference: the node's host loop, elevation_mapping_cupy/src/elevation_mapping_ros.cpp:319-338 -- per point
// and field memcpy(&temp, &data[i * point_step + fields[j].offset], 4) into an (n, fields) float64 matrix, cast back to float32 in
// input_pointcloud.  Here the message is uploaded as it is (point_step bytes a point) and turned into the layout the frame kernels
// read: an (n, 3) xyz matrix and an (n, Kc) channel matrix (emap_device.h: ChanView).  Nothing is compacted.
//
// The work is a transpose of an array of point_step-byte structs, whose fields need not be aligned (Velodyne: 22-byte points, a float
// at offset 18), into two dense float32 matrices.  k_cloud_unpack streams it through LDS:
//   1. A workgroup takes T = cloud_unpack_tile(point_step) consecutive points of one message row (emap_launch.h: a power of two in
//      64 .. 1024 with T * point_step <= 16 KB, so nine workgroups fit a CU's LDS).  Their bytes [b0, b1) are contiguous; they are
//      loaded with 16-byte loads from b0 aligned DOWN to 16 up to b1 aligned UP (the device copy of the message carries 16 bytes of
//      slack behind its end), four loads in flight per lane, fully coalesced whatever point_step is, and stored to LDS as they are.
//   2. After the barrier both output matrices of the tile are walked as FLAT float arrays: the tile's rows [R0, R0 + cnt) of an
//      (n, W) matrix are the floats [R0 W, (R0 + cnt) W), a lane takes one 16-byte aligned group of four of them (element e: row
//      e / W, column e % W -- a group spans records when W % 4 != 0), fetches each from LDS and stores the group with ONE 16-byte
//      store; only the groups cut by the tile's first or last float (at most two per matrix) store dwords.  So xyz (W = 3) and every
//      channel count leave in 16-byte stores, a wave writes 1 KB contiguous.
// An element's fetch: the 4 bytes at head + row * point_step + offset[col] of the staged range.
//   ALIGNED4 (point_step, every offset and the row stride multiples of 4, every conv 0 or a 4-byte type): one dword LDS read.
//   general: the two (FLOAT64: three) aligned dwords around the field, joined by a funnel shift (v_alignbit_b32), then narrowed.
// conv 0 moves the 32 bits with integer operations only (the outputs are stored as integers): NaN payloads and subnormal patterns such
// as the packed rgb colour arrive untouched.  conv 1 .. 8: ONE conversion to float32, round to nearest even (the mode hipcc leaves),
// subnormals kept (.amdhsa_float_denorm_mode_32 = 3, _16_64 = 3); a float64 beyond float32 becomes +-inf, a NaN stays a NaN.
// LDS banks: a wave's k-th element reads are 16 output bytes apart per lane, i.e. 16 point_step / (4 W) input bytes on average: for
// the tight 12-byte point that is stride 4 dwords (4-way on ds_read_b32), for 16 / 22 / 32-byte points with one to four channels
// the strides are odd multiples or fractions and spread; at 4-way the LDS still delivers 32 B/clk/CU, several times the CU's share of
// HBM.  The column table (offset | conv << 16) is uniform kernel arguments, copied to LDS once because a lane's column is not uniform.
// Plain C++ loads and stores and builtins only.
#include "emap_launch.h"

namespace {

constexpr int CM_BLOCK = 256;
constexpr int CM_CHUNKS = EM_CLOUDMSG_STAGE_BYTES / 16 + 2;      // 15 bytes of head + the tile + the funnel's look-ahead (<= 8 bytes)

template <bool A4>
__device__ __forceinline__ unsigned fetch(const unsigned* lds, const unsigned* tab, unsigned head, unsigned ps, unsigned row, unsigned col) {
  const unsigned e = tab[col], conv = e >> 16;
  const unsigned addr = head + row * ps + (e & 0xFFFFu);
  if (A4) {
    const unsigned v = lds[addr >> 2];
    if (conv == 5) return __float_as_uint((float)(int)v);
    if (conv == 6) return __float_as_uint((float)v);
    return v;                                                      // 0, 7: moved
  }
  const unsigned w = addr >> 2, sh = (addr & 3u) * 8u;
  const unsigned d0 = lds[w], d1 = lds[w + 1];
  const unsigned lo = __builtin_amdgcn_alignbit(d1, d0, sh);       // the 4 bytes at addr, little-endian
  switch (conv) {
    case 1: return __float_as_uint((float)(int)(signed char)(lo & 0xFFu));
    case 2: return __float_as_uint((float)(lo & 0xFFu));
    case 3: return __float_as_uint((float)(int)(short)(lo & 0xFFFFu));
    case 4: return __float_as_uint((float)(lo & 0xFFFFu));
    case 5: return __float_as_uint((float)(int)lo);
    case 6: return __float_as_uint((float)lo);
    case 8: {
      const unsigned hi = __builtin_amdgcn_alignbit(lds[w + 2], d1, sh);
      return __float_as_uint((float)__hiloint2double((int)hi, (int)lo));
    }
    default: return lo;                                            // 0, 7: moved
  }
}

// the tile's rows [R0, R0 + cnt) of the (n, W) matrix `out` (16-byte aligned), message columns col0 .. col0 + W
template <bool A4>
__device__ __forceinline__ void write_matrix(const unsigned* lds, const unsigned* tab, unsigned head, unsigned ps, unsigned* out, unsigned W, unsigned col0,
                                             long R0, unsigned cnt) {
  const long F0 = R0 * W, F1 = F0 + (long)cnt * W;
  const long q0 = F0 >> 2;
  const unsigned nq = (unsigned)(((F1 + 3) >> 2) - q0);
  for (unsigned q = threadIdx.x; q < nq; q += CM_BLOCK) {
    const long f = (q0 + q) << 2;                                  // floats f .. f + 3 of the matrix
    const int e0 = (int)(f - F0);                                  // < 0 only in the tile's first group
    const unsigned ec = e0 < 0 ? 0u : (unsigned)e0;
    unsigned row = ec / W, col = ec - row * W;
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = e0 + k >= 0 && f + k < F1;
      v[k] = in ? fetch<A4>(lds, tab, head, ps, row, col0 + col) : 0u;
      if (e0 + k >= 0 && ++col == W) { col = 0; ++row; }
    }
    if (e0 >= 0 && f + 4 <= F1) {
      *reinterpret_cast<uint4*>(out + f) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k >= 0 && f + k < F1) out[f + k] = v[k];
    }
  }
}

}  // namespace

template <bool A4>
__global__ __launch_bounds__(CM_BLOCK) void k_cloud_unpack(CloudMsgArgs A) {
  __shared__ uint4 stage[CM_CHUNKS];
  __shared__ unsigned tab[EM_CLOUDMSG_MAX_COLS + 1];
  const unsigned tid = threadIdx.x;
  const unsigned r = blockIdx.x / (unsigned)A.tiles_per_row, t = blockIdx.x - r * (unsigned)A.tiles_per_row;
  const unsigned p0 = t * (unsigned)A.tile;
  const unsigned cnt = min((unsigned)A.tile, (unsigned)A.width - p0);
  const long b0 = (long)r * A.row_step + (long)p0 * A.point_step;
  const long a0 = b0 & ~15L;
  const unsigned head = (unsigned)(b0 - a0);
  const unsigned nch = (head + cnt * (unsigned)A.point_step + 15u) >> 4;      // <= CM_CHUNKS - 1
  const uint4* src = reinterpret_cast<const uint4*>(A.msg + a0);
  for (unsigned c = tid; c < nch; c += 4 * CM_BLOCK) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = src[min(c + k * CM_BLOCK, nch - 1)];
    // clamped, not skipped, on both sides: four loads in flight per lane, no branch between them and their LDS stores (a lane past the
    // end rewrites the last chunk with the bytes it already holds)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      stage[min(c + k * CM_BLOCK, nch - 1)] = v[k];
  }
  for (int c = 0; c < A.n_cols; ++c)                               // (a uniform index: scalar loads of the kernel arguments, no private copy)
    if (tid == (unsigned)c) tab[c] = A.col[c];
  __syncthreads();
  const unsigned* lds = reinterpret_cast<const unsigned*>(stage);
  const long R0 = (long)r * A.width + p0;
  write_matrix<A4>(lds, tab, head, (unsigned)A.point_step, reinterpret_cast<unsigned*>(A.xyz), 3u, 0u, R0, cnt);
  if (A.n_cols > 3) write_matrix<A4>(lds, tab, head, (unsigned)A.point_step, reinterpret_cast<unsigned*>(A.chan), (unsigned)(A.n_cols - 3), 3u, R0, cnt);
}

void launch_cloud_unpack(hipStream_t s, const CloudMsgArgs& A, bool aligned4) {
  if (A.rows <= 0 || A.width <= 0) return;
  const dim3 grid((unsigned)((long)A.rows * A.tiles_per_row)), block(CM_BLOCK);
  if (aligned4) hipLaunchKernelGGL((k_cloud_unpack<true>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_cloud_unpack<false>), grid, block, 0, s, A);
}
