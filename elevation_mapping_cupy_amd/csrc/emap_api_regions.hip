// C ABI of the MI355X elevation-map fusion core, host side of the planar regions on the device (kernels: emap_regions.hip, the
// segmentation's union-find, emap_planeseg.hip, and the scan of emap_cloudout.hip): the middle stage of convex_plane_decomposition's
// PlaneDecompositionPipeline::update, ContourExtraction::extractPlanarRegions (ContourExtraction.cpp:28-128), on a label plane -- the one
// the last segmentation left on the context, or one of the caller's.  ONE chain of launches on the context's stream with three waits:
// images, components and crack bits -> the crack count; the buffers sized by it; successors, cycles, vertex ranks, records -> the ring
// and vertex counts; exactly the rings and vertices.  Every buffer belongs to the context.
#include "emap_host.h"
#include <cstddef>
#include <cstring>

using namespace emap_host;

static_assert(EMAP_REGION_MARGIN_MAX == EM_REGION_MARGIN_MAX && 2 * (1 + EM_REGION_MARGIN_MAX) + 1 <= EM_TERRAIN_KERNEL_MAX, "margin cap");
static_assert(sizeof(emap_region_params) == 16 && sizeof(emap_region_ring) == 32 && sizeof(RegionRing) == sizeof(emap_region_ring) &&
              offsetof(emap_region_ring, boundary) == offsetof(RegionRing, boundary), "layout");
static_assert(4LL * (3LL * EMAP_REGION_SIDE_MAX - 2) * (3LL * EMAP_REGION_SIDE_MAX - 2) < (1LL << 31) && 4LL * (3LL * (EMAP_REGION_SIDE_MAX + 1) - 2) * (3LL * (EMAP_REGION_SIDE_MAX + 1) - 2) >= (1LL << 31) &&
              4LL * EMAP_REGION_RAW_SIDE_MAX * EMAP_REGION_RAW_SIDE_MAX < (1LL << 31), "crack indices are int");

namespace {
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
size_t trip(size_t words) { return (words + EM_CLOUD_SCAN_TRIP - 1) / EM_CLOUD_SCAN_TRIP * EM_CLOUD_SCAN_TRIP; }
}  // namespace

extern "C" {

int emap_planar_regions(emap_ctx* ctx, const int32_t* host_labels, int32_t side, int32_t n_labels, const emap_region_params* params,
                        emap_region_ring* host_rings, int64_t capacity_rings, int32_t* host_vertices, int64_t capacity_vertices,
                        int64_t* n_rings, int64_t* n_vertices) {
  // everything is refused BEFORE anything is uploaded, launched or copied: the outputs stay as they are
  const std::string w = "emap_planar_regions: ";
  CKARG(ctx, "null ctx");
  CKARG(params && n_rings && n_vertices, w + "null argument");
  CKARG(capacity_rings >= 0 && capacity_vertices >= 0, w + "a capacity is negative");
  CKARG((host_rings || capacity_rings == 0) && (host_vertices || capacity_vertices == 0), w + "a buffer with a capacity is NULL");
  const int mode = params->mode;
  CKARG(mode == 0 || mode == 1, w + "mode must be 0 (regions) or 1 (raw mask)");
  CKARG(mode == 1 || (params->margin_size >= 0 && params->margin_size <= EMAP_REGION_MARGIN_MAX), w + "margin_size must lie in 0 .. 14");
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, w + "single-strip contexts only");
  int M = side;
  if (!host_labels) {
    CKARG(mode == 0, w + "a raw mask is the caller's: host_labels is NULL");
    CKARG(ctx->pseg_labels, w + "no valid resident labels (no segmentation on this context yet, or the map was cleared or shifted since)");
    CKARG(side == 0 || side == ctx->prm.cell_n - 2, w + "side is not the map's");
    M = ctx->prm.cell_n - 2; n_labels = ctx->pseg_n_labels;
  }
  CKARG(M >= 2, w + "the plane must have at least 2 x 2 cells");
  CKARG(M <= (mode == 0 ? EMAP_REGION_SIDE_MAX : EMAP_REGION_RAW_SIDE_MAX), w + "the plane is too large: crack indices are 32-bit");
  CKARG(n_labels >= 0, w + "n_labels is negative");
  const size_t NL = (size_t)M * M;
  if (host_labels) {                                           // the kernels index a table of n_labels + 1 words with these
    const int hi = mode == 1 ? 1 : n_labels;
    bool ok = true;
    for (size_t k = 0; k < NL && ok; ++k) ok = host_labels[k] >= 0 && host_labels[k] <= hi;
    CKARG(ok, w + (mode == 1 ? "a raw mask holds only 0 and 1" : "a label lies outside 0 .. n_labels"));
  }

  SF_CHECK();
  CK(hipSetDevice(ctx->device));
  RegionArgs G;
  G.M = M; G.U = mode == 0 ? 3 * M - 2 : M; G.mode = mode; G.k = mode == 0 ? 2 * (1 + params->margin_size) + 1 : 1;
  const size_t N = (size_t)G.U * G.U, W = (N + 31) / 32, Wc = (N + 7) / 8;
  G.Wc = (long)Wc;
  // the buffer sized by the pixels: [head words] [labels] [flag] [A] [B] [rootA] [rootB] [parent] [cnt] [amin] [mask1] [cmask] [coffs] [em] [bm] [bitA] [bitB]
  const size_t P = up16(4 * N), o_lab = 16, o_flag = o_lab + up16(4 * NL), o_int = o_flag + up16(4 * ((size_t)n_labels + 1)), o_m1 = o_int + 7 * P,
               o_cm = o_m1 + 4 * trip(W), o_co = o_cm + 4 * trip(2 * Wc), o_byte = o_co + 4 * trip(2 * Wc), dev_bytes = o_byte + 4 * up16(N);
  { const int rc = grow(ctx, &ctx->reg_buf, &ctx->reg_cap, dev_bytes); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->reg_pin, &ctx->reg_pin_cap, (size_t)16, Grow::pinned); if (rc) return rc; }      // (every call ends with a wait: no DMA of the pinned buffer is in flight here)
  unsigned char* d = ctx->reg_buf;
  auto ip = [&](int k) { return reinterpret_cast<int*>(d + o_int + (size_t)k * P); };
  auto bp = [&](int k) { return d + o_byte + (size_t)k * up16(N); };
  int* dev_labels = reinterpret_cast<int*>(d + o_lab);
  RegionBufs R = {host_labels ? dev_labels : ctx->pseg_labels, bp(0), bp(1), reinterpret_cast<unsigned int*>(d + o_flag), ip(0), ip(1), bp(2), bp(3), ip(2), ip(3),
                  reinterpret_cast<unsigned int*>(d + o_cm), reinterpret_cast<unsigned int*>(d + o_co), reinterpret_cast<unsigned int*>(d)};
  int* const parent = ip(4); int* const cnt = ip(5); int* const amin = ip(6);
  unsigned int* const mask1 = reinterpret_cast<unsigned int*>(d + o_m1);
  hipStream_t s = ctx->stream;
  if (host_labels) CK(hipMemcpyAsync(dev_labels, host_labels, 4 * NL, hipMemcpyHostToDevice, s));
  CK(hipMemsetAsync(d, 0, 16, s));
  CK(hipMemsetAsync(R.flag, 0, 4 * ((size_t)n_labels + 1), s));
  TerrainSpans sp; ellipse_spans(G.k, &sp);
  launch_rg_images(s, G, sp, R);
  launch_ps_components(s, G.U, 8, R.bitA, parent, R.rootA, cnt, amin, mask1);
  launch_ps_components(s, G.U, 8, R.bitB, parent, R.rootB, cnt, amin, mask1);
  launch_rg_cracks(s, G, R);
  launch_cloud_scan(s, R.cmask, R.coffs, (long)(2 * Wc), R.head);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->reg_pin, R.head, 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));                                 // wait 1: the cracks
  unsigned int head[3] = {0, 0, 0};
  memcpy(head, ctx->reg_pin, 4);
  const size_t n = head[0];
  if (n >= ((size_t)1 << 30)) { ctx->err = w + "more than 2^30 cracks"; return EMAP_ERR_INVALID; }

  RegionCracks K; memset(&K, 0, sizeof K);
  if (n) {
    // the buffer sized by the cracks: [raw] [succ] [pred] [parent] [cyc] [nv 0] [nv 1] [hmask] [hoffs] [rcnt] [rfirst] [rings] [verts] [vbit]
    const size_t I = up16(4 * n), Wh = trip((n + 31) / 32), Q = up16(4 * (n / 4 + 1));
    const size_t o_nv = 5 * I, o_hm = o_nv + 2 * up16(8 * n), o_rc = o_hm + 8 * Wh, o_rg = o_rc + 2 * Q, o_vt = o_rg + up16(sizeof(RegionRing) * (n / 4 + 1)),
                 o_vb = o_vt + up16(8 * n), crack_bytes = o_vb + up16(n);
    { const int rc = grow(ctx, &ctx->reg_cracks, &ctx->reg_cracks_cap, crack_bytes); if (rc) return rc; }
    unsigned char* c = ctx->reg_cracks;
    auto ci = [&](int k) { return reinterpret_cast<int*>(c + (size_t)k * I); };
    K.raw = reinterpret_cast<unsigned int*>(c); K.succ = ci(1); K.pred = ci(2); K.parent = ci(3); K.cyc = ci(4);
    K.nv[0] = reinterpret_cast<int2*>(c + o_nv); K.nv[1] = reinterpret_cast<int2*>(c + o_nv + up16(8 * n));
    K.hmask = reinterpret_cast<unsigned int*>(c + o_hm); K.hoffs = reinterpret_cast<unsigned int*>(c + o_hm + 4 * Wh);
    K.rcnt = reinterpret_cast<int*>(c + o_rc); K.rfirst = reinterpret_cast<int*>(c + o_rc + Q);
    K.rings = reinterpret_cast<RegionRing*>(c + o_rg); K.verts = reinterpret_cast<int2*>(c + o_vt); K.vbit = c + o_vb;
    launch_rg_trace(s, G, R, K, (int)n);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->reg_pin, R.head, 12, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));                               // wait 2: the rings and the vertices
    memcpy(head, ctx->reg_pin, 12);
  }
  *n_rings = (int64_t)head[1]; *n_vertices = (int64_t)head[2];
  if ((int64_t)head[1] > capacity_rings || (int64_t)head[2] > capacity_vertices) {
    ctx->err = w + "more rings or vertices than the capacities (*n_rings and *n_vertices tell how many)"; return EMAP_ERR_INVALID;
  }
  if (head[1]) {
    CK(hipMemcpyAsync(host_rings, K.rings, sizeof(RegionRing) * (size_t)head[1], hipMemcpyDeviceToHost, s));
    if (head[2]) CK(hipMemcpyAsync(host_vertices, K.verts, 8 * (size_t)head[2], hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));                               // wait 3
  }
  return EMAP_OK;
}

}  // extern "C"
