// Image message input: one camera frame in ONE launch (emap_input_image_message, emap_api_image_msg.hip).  Reference: the node turns a
// sensor_msgs/Image into one float matrix per channel on the host (elevation_mapping_cupy/src/elevation_mapping_ros.cpp:375-446:
// cvtColor for bgr8 / bgra8, cv::split, cv2eigen), input_image (EM/elevation_mapping.py:468-562) uploads the stack, launches the
// correspondence kernel and then one sampling kernel per channel (EM/kernels/custom_image_kernels.py:160-271).  Here the message's BYTES
// are on the device and k_image_frame, one thread per cell,
//   1. computes the cell's correspondence with the body k_image_corr runs (emap_camera.h) and writes uv / valid where
//      emap_image_get_correspondence reads them;
//   2. if the cell sees the camera, walks the table of fusion entries IN ORDER inside the thread (a later entry on the same layer reads
//      what the earlier one stored, as the reference's sequential launches do) and applies k_image_fuse's arithmetic to each:
//      idx = (int)((float)(int)u + (float)(int)v * iw), the colour kind's planes at iw * ih + idx and iw * ih * 2 + idx in float, the
//      exponential blend in double.  The host admits only images with H W (x 3 for colour) <= 2^24, where that float arithmetic is exact.
// A sample = plane p of pixel idx: message channel c (c = 2 - p for p in {0, 2} of bgr8 / bgra8, else p) at byte
// (idx / W) * step + ((idx % W) * n_chan + c) * esize, loaded at the element's width, byte-swapped for a big-endian message and converted
// to float32 by ONE conversion (round to nearest even, subnormals kept, a float64 beyond float32 -> +-inf); a 32F element is moved.
// This is a gather from an image that fits in L2: no LDS, no staging.  step may be odd, so an element may sit at any address: a 1-byte
// element is one byte load; a 2 / 4-byte element is read as the TWO aligned dwords around it and an 8-byte element as the three, joined
// by a funnel shift (v_alignbit_b32) -- always aligned loads, the device copy carries EM_IMGMSG_SLACK bytes behind the message's end.
// Variants: one instantiation per element SIZE (1, 2, 4, 8 bytes: the loads differ); the element CODE, the byte order and the entry
// table are kernel arguments -- the same in every lane, so the switches below are scalar branches.  Plain C++ and builtins only.
#include "emap_launch.h"
#include "emap_camera.h"

namespace {

// the 4 (ESIZE 8: 8) bytes at byte address a of the message as little-endian integers, from aligned dword loads
template <int ESIZE>
__device__ __forceinline__ unsigned long long load_elem(const unsigned char* __restrict__ msg, long a) {
  if (ESIZE == 1) return msg[a];
  const unsigned* w = reinterpret_cast<const unsigned*>(msg + (a & ~3L));
  const unsigned sh = ((unsigned)a & 3u) * 8u;
  const unsigned d0 = w[0], d1 = w[1];
  const unsigned lo = __builtin_amdgcn_alignbit(d1, d0, sh);
  if (ESIZE != 8) return lo;
  const unsigned hi = __builtin_amdgcn_alignbit(w[2], d1, sh);
  return ((unsigned long long)hi << 32) | lo;
}

// plane p of pixel pix (both clamped into the message: the host's checks make the clamps idle) as a float32's bits
template <int ESIZE>
__device__ __forceinline__ float sample(const ImgMsgArgs& M, int p, int pix) {
  p = min(max(p, 0), M.n_chan - 1);
  pix = min(max(pix, 0), M.H * M.W - 1);
  const int c = (M.swap && (p == 0 || p == 2)) ? 2 - p : p;
  const int v = pix / M.W, u = pix - v * M.W;
  const long a = (long)v * M.step + ((long)u * M.n_chan + c) * ESIZE;
  const unsigned long long raw = load_elem<ESIZE>(M.msg, a);
  if (ESIZE == 1) return M.elem == 0 ? (float)(unsigned)(raw & 0xFFu) : (float)(int)(signed char)(raw & 0xFFu);
  if (ESIZE == 2) {
    unsigned h = (unsigned)raw & 0xFFFFu;
    if (M.big) h = ((h & 0xFFu) << 8) | (h >> 8);
    return M.elem == 2 ? (float)h : (float)(int)(short)h;
  }
  if (ESIZE == 4) {
    unsigned d = (unsigned)raw;
    if (M.big) d = __builtin_bswap32(d);
    return M.elem == 4 ? (float)(int)d : __uint_as_float(d);               // 32F: moved
  }
  unsigned long long q = raw;
  if (M.big) q = __builtin_bswap64(q);
  return (float)__longlong_as_double((long long)q);
}

}  // namespace

template <int ESIZE>
__global__ __launch_bounds__(EM_BLOCK) void k_image_frame(KP P, CamArgs A, Cells cells, float* __restrict__ uv, unsigned char* __restrict__ valid,
                                                           ImgMsgArgs M, float* __restrict__ sem, long plane) {
  const long L = (long)P.C * P.C;
  const long i = (long)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= L) return;
  float cu, cv;
  const bool ok = image_corr_cell(P, A, cells, i, cu, cv);
  uv[i] = cu; uv[L + i] = cv; valid[i] = ok ? 1 : 0;
  if (!ok) return;
  const float ih = A.ih, iw = A.iw;
  const int idx = (int)((float)(int)cu + (float)(int)cv * iw);              // k_image_fuse, literally
  const int x0 = (int)(i / P.C), y0 = (int)(i - (long)x0 * P.C);
  const long pc = (long)phys_row(P, x0) * P.C + phys_col(P, y0);            // the layers are stored with the map's circular origin
  const int HW = M.H * M.W;
  for (int k = 0; k < M.n_specs; ++k) {                                      // (uniform: scalar loads of the kernel arguments)
    const ImgMsgEntry e = M.e[k];
    float* const cell = sem + (long)e.layer * plane + pc;
    if (e.kind == 0) *cell = (float)((double)*cell * (1 - e.alpha) + e.alpha * (double)sample<ESIZE>(M, e.plane, idx));
    else if (e.kind == 2) *cell = sample<ESIZE>(M, e.plane, idx);           // average_correspondences_to_map_kernel: the sample replaces the value
    else {
      // the reference indexes the float stack: its planes 0, 1, 2 at idx, iw * ih + idx, iw * ih * 2 + idx
      const int ig = (int)(iw * ih + (float)idx), ib = (int)(iw * ih * 2 + (float)idx);
      const int pg = ig / HW, pb = ib / HW;
      const unsigned int r = (unsigned int)sample<ESIZE>(M, 0, idx), g = (unsigned int)sample<ESIZE>(M, pg, ig - pg * HW),
                         b = (unsigned int)sample<ESIZE>(M, pb, ib - pb * HW);
      *cell = __uint_as_float((r << 16) + (g << 8) + b);
    }
  }
}

void launch_image_frame(hipStream_t s, const KP& P, const CamArgs& A, Cells cells, float* uv, unsigned char* valid, const ImgMsgArgs& M, float* sem,
                        long plane) {
  const dim3 grid((unsigned)(((long)P.C * P.C + EM_BLOCK - 1) / EM_BLOCK)), block(EM_BLOCK);
  switch (image_frame_variant(M.esize)) {
    case 0: hipLaunchKernelGGL((k_image_frame<1>), grid, block, 0, s, P, A, cells, uv, valid, M, sem, plane); break;
    case 1: hipLaunchKernelGGL((k_image_frame<2>), grid, block, 0, s, P, A, cells, uv, valid, M, sem, plane); break;
    case 2: hipLaunchKernelGGL((k_image_frame<4>), grid, block, 0, s, P, A, cells, uv, valid, M, sem, plane); break;
    default: hipLaunchKernelGGL((k_image_frame<8>), grid, block, 0, s, P, A, cells, uv, valid, M, sem, plane); break;
  }
}
