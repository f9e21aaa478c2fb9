// C ABI of the MI355X elevation-map fusion core, host side of the publish-time plugins on device-resident planes (kernels:
// emap_plugchain.hip, emap_semantic.hip, emap_inpaint_chain.hip, emap_inpaint_fronts.hip).  The reference keeps the plugins' outputs in PluginManager.layers on its device
// (EM/plugins/plugin_manager.py:130, :181-236); the host route here (emap_api_plugins.hip) moves every plane over PCIe twice per plugin.
// A chain enqueues the plugins of a publisher on the context's stream into planes the context owns and does not wait: k_grid_map
// (emap_api_gridmsg.hip, kind EMAP_GRID_PLUGIN) reads them next to the cells, so a publisher's tick has one wait.
#include "emap_host.h"
#include <cstring>

using namespace emap_host;

namespace {
bool full_map(const emap_ctx* ctx) { return ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n; }
size_t plane_len(const emap_ctx* ctx) { return (size_t)ctx->prm.cell_n * ctx->prm.cell_n; }

// scratch planes / counters of one op (each op of a chain has its own: two filters in one chain must not share counters)
size_t op_planes(const emap_plugin_op& o) {
  switch (o.type) {
    case EMAP_PLUGIN_MIN_FILTER: case EMAP_PLUGIN_MAX_FILTER: return 5;       // orig mask, two (value, mask) pairs
    case EMAP_PLUGIN_SMOOTH: return o.src_kind == EMAP_PLUGIN_SRC_LAYER ? 1 : 0;
    case EMAP_PLUGIN_EROSION: return 2 + (o.src_kind == EMAP_PLUGIN_SRC_LAYER ? 1 : 0);
    case EMAP_PLUGIN_INPAINT_FRONTS: return 0;                                  // byte images and fronts state: op_inpaint_bytes
    case EMAP_PLUGIN_SEMANTIC_FILTER: case EMAP_PLUGIN_SEMANTIC_TRAV: case EMAP_PLUGIN_MAX_LAYER: case EMAP_PLUGIN_FEATURES_PCA: return 0;      // every source is read where it lies
    default: return 2;                                                          // ROBOT_CENTRIC: elevation, is_valid
  }
}
size_t op_counters(const emap_plugin_op& o) { return o.type <= EMAP_PLUGIN_MAX_FILTER ? (size_t)o.i1 + 1 : 0; }
// INPAINT_FRONTS: fronts per launch, and the bytes of its own scratch -- the fronts pipeline's images and planes (emap_launch.h:
// FrontsDev), behind them the partial range records and the folded one
int inpaint_steps(const emap_plugin_op& o) { return o.i0 ? o.i0 : fronts_default_steps(); }
size_t inpaint_range_bytes() { return ((EM_INP_PARTS + 1) * sizeof(InpRange) + 255) & ~(size_t)255; }
size_t op_inpaint_bytes(const emap_ctx* ctx, const emap_plugin_op& o) {
  return o.type == EMAP_PLUGIN_INPAINT_FRONTS ? fronts_bytes(ctx->prm.cell_n, ctx->prm.cell_n, inpaint_steps(o)) + inpaint_range_bytes() : 0;
}

// the ops that read a run of the side table (emap_plugin_chain_ex): the limits of the run's length, the kinds and the source flags they know
bool multi_src(int type) { return type >= EMAP_PLUGIN_SEMANTIC_FILTER && type <= EMAP_PLUGIN_FEATURES_PCA; }
int src_min(int type) { return type == EMAP_PLUGIN_SEMANTIC_FILTER ? 0 : (type == EMAP_PLUGIN_FEATURES_PCA ? 3 : 1); }
int src_max(int type) { return type == EMAP_PLUGIN_SEMANTIC_FILTER ? EM_PLUG_SRC_MAX : EM_PLUG_PAR_MAX; }
int src_flags(int type) {
  return type == EMAP_PLUGIN_SEMANTIC_TRAV ? EMAP_PLUGIN_SRC_AT_MOST
       : type == EMAP_PLUGIN_MAX_LAYER ? (EMAP_PLUGIN_SRC_ZERO_DEFAULT | EMAP_PLUGIN_SRC_REVERSE | EMAP_PLUGIN_SRC_SCALE | EMAP_PLUGIN_SRC_THRESHOLD) : 0;
}
static_assert(sizeof(emap_plugin_op) == 32 && sizeof(emap_plugin_src) == 32, "the records of the plugin chain are 32 bytes");
static_assert(EM_PCA_F == EM_PLUG_PAR_MAX && EMAP_PLUGIN_MAX_SRCS == EMAP_PLUGIN_MAX_OPS * EM_PLUG_SRC_MAX, "limits");

// what a chain needs of the context's scratch: planes, counters, bytes of the inpaint ops, doubles of the PCA ops
struct ChainNeed { size_t planes, counters, inpaint, pca; };
int chain_check(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, int32_t n_srcs, bool ex, ChainNeed* need);
int chain_enqueue(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, const ChainNeed& need);

}  // namespace

extern "C" {

int emap_plugin_planes(emap_ctx* ctx, int32_t n_planes) {
  CKARG(ctx, "null ctx");
  CKARG(n_planes >= 0 && n_planes <= EMAP_PLUGIN_MAX_PLANES, "emap_plugin_planes: n_planes must lie in 0 .. 32");
  CKARG(full_map(ctx), "emap_plugin_planes: single-strip contexts only"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const size_t L = plane_len(ctx);
  if (n_planes > ctx->plane_cap) {      // (not emap_host::grow: the planes already written are kept)
    float* nb = nullptr;
    CK(hipMalloc((void**)&nb, sizeof(float) * L * n_planes));
    hipError_t e = hipSuccess;
    if (ctx->plane_n) e = hipMemcpyAsync(nb, ctx->plane_buf, sizeof(float) * L * ctx->plane_n, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nb + L * ctx->plane_n, 0, sizeof(float) * L * (n_planes - ctx->plane_n), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // (whatever read or wrote the old planes is done before they are freed)
    if (e != hipSuccess) { hipFree(nb); CK(e); }
    if (ctx->plane_buf) CK(hipFree(ctx->plane_buf));
    ctx->plane_buf = nb; ctx->plane_cap = n_planes;
  } else if (n_planes > ctx->plane_n) {
    CK(hipMemsetAsync(ctx->plane_buf + L * ctx->plane_n, 0, sizeof(float) * L * (n_planes - ctx->plane_n), ctx->stream));
  }
  ctx->plane_n = n_planes;
  return EMAP_OK;
}

int emap_plugin_plane_write(emap_ctx* ctx, int32_t plane, const float* host_in) {
  CKARG(ctx, "null ctx");
  CKARG(host_in, "emap_plugin_plane_write: null argument");
  CKARG(plane >= 0 && plane < ctx->plane_n, "emap_plugin_plane_write: plane outside the reservation (emap_plugin_planes)"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const size_t L = plane_len(ctx);
  CK(hipMemcpyAsync(ctx->plane_buf + L * plane, host_in, sizeof(float) * L, hipMemcpyHostToDevice, ctx->stream));
  return EMAP_OK;
}

int emap_plugin_plane_read(emap_ctx* ctx, int32_t plane, float* host_out) {
  CKARG(ctx, "null ctx");
  CKARG(host_out, "emap_plugin_plane_read: null argument");
  CKARG(plane >= 0 && plane < ctx->plane_n, "emap_plugin_plane_read: plane outside the reservation (emap_plugin_planes)"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const size_t L = plane_len(ctx);
  CK(hipMemcpyAsync(host_out, ctx->plane_buf + L * plane, sizeof(float) * L, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

int emap_plugin_chain(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9) {
  ChainNeed need;
  int rc = chain_check(ctx, ops, n_ops, rotation9, nullptr, 0, false, &need); if (rc) return rc;
  SF_CHECK();
  return chain_enqueue(ctx, ops, n_ops, rotation9, nullptr, need);
}
int emap_plugin_chain_ex(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, int32_t n_srcs) {
  ChainNeed need;
  int rc = chain_check(ctx, ops, n_ops, rotation9, srcs, n_srcs, true, &need); if (rc) return rc;
  SF_CHECK();
  return chain_enqueue(ctx, ops, n_ops, rotation9, srcs, need);
}

}  // extern "C"

namespace {
int chain_check(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, int32_t n_srcs, bool ex, ChainNeed* need) {
  CKARG(ctx, "null ctx");
  // everything is refused BEFORE anything is enqueued: the planes and the map stay as they are
  CKARG(ops, "emap_plugin_chain: null argument");
  CKARG(n_ops >= 1 && n_ops <= EMAP_PLUGIN_MAX_OPS, "emap_plugin_chain: n_ops must lie in 1 .. 32");
  CKARG(full_map(ctx), "emap_plugin_chain: single-strip contexts only");
  CKARG(n_srcs >= 0 && n_srcs <= EMAP_PLUGIN_MAX_SRCS && (srcs || n_srcs == 0), "emap_plugin_chain_ex: n_srcs must lie in 0 .. 2048, with a table behind it");
  size_t planes = 0, counters = 0, inpaint = 0, pca = 0;
  for (int k = 0; k < n_ops; ++k) {
    const emap_plugin_op& o = ops[k];
    CKARG(ex || !multi_src(o.type), "emap_plugin_chain: the semantic ops (types 7 .. 10) read a table of sources: call emap_plugin_chain_ex");
    CKARG((o.type >= EMAP_PLUGIN_MIN_FILTER && o.type <= EMAP_PLUGIN_ROBOT_CENTRIC) || o.type == EMAP_PLUGIN_INPAINT_FRONTS || multi_src(o.type), "emap_plugin_chain: unknown op type");
    CKARG(o.dst_plane >= 0 && o.dst_plane < ctx->plane_n, "emap_plugin_chain: dst_plane outside the reservation (emap_plugin_planes)");
    const bool reads_src = o.type == EMAP_PLUGIN_SMOOTH || o.type == EMAP_PLUGIN_EROSION;
    if (reads_src) {
      CKARG(o.src_kind == EMAP_PLUGIN_SRC_LAYER || o.src_kind == EMAP_PLUGIN_SRC_PLANE, "emap_plugin_chain: src_kind must be 0 (map layer) or 1 (resident plane)");
      CKARG(o.src_kind != EMAP_PLUGIN_SRC_LAYER || (o.src_index >= 0 && o.src_index <= 6), "emap_plugin_chain: a map layer index must lie in 0 .. 6");
      CKARG(o.src_kind != EMAP_PLUGIN_SRC_PLANE || (o.src_index >= 0 && o.src_index < ctx->plane_n), "emap_plugin_chain: source plane outside the reservation (emap_plugin_planes)");
    }
    if (o.type == EMAP_PLUGIN_SMOOTH)
      CKARG(!(o.src_kind == EMAP_PLUGIN_SRC_PLANE && o.src_index == o.dst_plane), "emap_plugin_chain: a smooth filter cannot run in place (source plane = dst_plane)");
    if (o.type <= EMAP_PLUGIN_MAX_FILTER)
      CKARG(o.i0 >= 0 && o.i0 <= 32 && o.i1 >= 0 && o.i1 <= 4096, "emap_plugin_chain: bad filter size / iteration count");
    if (o.type == EMAP_PLUGIN_EROSION)
      CKARG(o.i0 >= 1 && o.i0 <= 63 && o.i1 >= 0 && o.i1 <= 256, "emap_plugin_chain: bad erosion kernel size / iteration count");
    if (o.type == EMAP_PLUGIN_INPAINT_FRONTS)
      CKARG(o.i0 >= 0 && o.i0 <= EM_FRONTS_S_MAX && o.i1 == 0, "emap_plugin_chain: bad fronts per launch (i0 must lie in 0 .. 16, i1 must be 0)");
    if (multi_src(o.type)) {
      CKARG(o.i0 >= src_min(o.type) && o.i0 <= src_max(o.type) && o.i1 == 0,
            "emap_plugin_chain_ex: source count outside the op's limits (filter 0 .. 64, votes and layer max 1 .. 16, PCA 3 .. 16; i1 must be 0)");
      CKARG(o.src_index >= 0 && o.src_index <= n_srcs && o.i0 <= n_srcs - o.src_index, "emap_plugin_chain_ex: the op's run of sources lies outside the table");
      for (int j = 0; j < o.i0; ++j) {
        const emap_plugin_src& q = srcs[o.src_index + j];
        CKARG(q.kind >= EMAP_PLUGIN_SRC_LAYER && q.kind <= (o.type == EMAP_PLUGIN_SEMANTIC_TRAV ? EMAP_PLUGIN_SRC_PLANE : EMAP_PLUGIN_SRC_SEMANTIC),
              "emap_plugin_chain_ex: source kind must be 0 (map layer), 1 (resident plane) or 2 (semantic layer; not for the votes)");
        CKARG(q.kind != EMAP_PLUGIN_SRC_LAYER || (q.index >= 0 && q.index <= 6), "emap_plugin_chain_ex: a map layer index must lie in 0 .. 6");
        CKARG(q.kind != EMAP_PLUGIN_SRC_PLANE || (q.index >= 0 && q.index < ctx->plane_n), "emap_plugin_chain_ex: source plane outside the reservation (emap_plugin_planes)");
        CKARG(q.kind != EMAP_PLUGIN_SRC_PLANE || q.index != o.dst_plane, "emap_plugin_chain_ex: a source is the op's own dst_plane");
        CKARG(q.kind != EMAP_PLUGIN_SRC_SEMANTIC || (q.index >= 0 && q.index < ctx->sem_layers), "emap_plugin_chain_ex: semantic layer outside the configured ones");
        CKARG((q.flags & ~src_flags(o.type)) == 0, "emap_plugin_chain_ex: a source flag the op does not know");
        CKARG(q.reserved == 0, "emap_plugin_chain_ex: reserved must be 0");
      }
      if (o.type == EMAP_PLUGIN_FEATURES_PCA) pca += EM_PCA_DOUBLES;
    }
    const int allowed = o.type == EMAP_PLUGIN_EROSION ? EMAP_PLUGIN_REVERSE : (o.type == EMAP_PLUGIN_ROBOT_CENTRIC ? EMAP_PLUGIN_THRESHOLD : (o.type == EMAP_PLUGIN_MAX_LAYER ? EMAP_PLUGIN_MIN : 0));
    CKARG((o.flags & ~allowed) == 0, "emap_plugin_chain: a flag the op does not know");
    CKARG(o.type != EMAP_PLUGIN_ROBOT_CENTRIC || rotation9, "emap_plugin_chain: null argument (rotation9)");
    planes += op_planes(o); counters += op_counters(o); inpaint += op_inpaint_bytes(ctx, o);
  }
  *need = ChainNeed{planes, counters, inpaint, pca};
  return EMAP_OK;
}

int chain_enqueue(emap_ctx* ctx, const emap_plugin_op* ops, int32_t n_ops, const float* rotation9, const emap_plugin_src* srcs, const ChainNeed& need) {
  const size_t planes = need.planes, counters = need.counters, inpaint = need.inpaint, pca = need.pca;
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const int C = ctx->prm.cell_n; const size_t L = plane_len(ctx), bytes = L * sizeof(float);
  int rc = grow(ctx, &ctx->chain_buf, &ctx->chain_cap, planes * L); if (rc) return rc;
  rc = grow(ctx, &ctx->chain_cnt, &ctx->chain_cnt_cap, counters); if (rc) return rc;
  rc = grow(ctx, &ctx->chain_red, &ctx->chain_red_cap, (size_t)n_ops * EM_RANGE_FLOATS); if (rc) return rc;
  rc = grow(ctx, &ctx->chain_inp, &ctx->chain_inp_cap, inpaint); if (rc) return rc;
  rc = grow(ctx, &ctx->chain_pca, &ctx->chain_pca_cap, pca); if (rc) return rc;
  if (counters) CK(hipMemsetAsync(ctx->chain_cnt, 0, sizeof(unsigned int) * counters, ctx->stream));

  float* buf = ctx->chain_buf; unsigned int* cnt = ctx->chain_cnt; unsigned char* inp = ctx->chain_inp; double* pcs = ctx->chain_pca;
  for (int k = 0; k < n_ops; ++k) {
    const emap_plugin_op& o = ops[k];
    float* dst = ctx->plane_buf + L * o.dst_plane;
    float* scr = buf; buf += op_planes(o) * L;
    const float* src = nullptr;      // SMOOTH / EROSION: the layer de-interleaved into the op's last scratch plane, or the resident plane
    if (o.type == EMAP_PLUGIN_SMOOTH || o.type == EMAP_PLUGIN_EROSION) {
      if (o.src_kind == EMAP_PLUGIN_SRC_LAYER) {
        float* own = scr + (op_planes(o) - 1) * L;
        launch_get_plane(ctx->stream, ctx->kp, ctx->cells, o.src_index, own);
        src = own;
      } else src = ctx->plane_buf + L * o.src_index;
    }
    switch (o.type) {
      case EMAP_PLUGIN_MIN_FILTER: case EMAP_PLUGIN_MAX_FILTER: {
        float *orig = scr, *v0 = scr + L, *m0 = scr + 2 * L, *v1 = scr + 3 * L, *m1 = scr + 4 * L;
        launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 2, orig);
        launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 0, v0);
        CK(hipMemcpyAsync(m0, orig, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        for (int it = 0; it < o.i1; ++it)
          launch_min_sweep(ctx->stream, C, o.i0, orig, (it & 1) ? v1 : v0, (it & 1) ? m1 : m0, (it & 1) ? v0 : v1, (it & 1) ? m0 : m1,
                           it > 0 ? cnt + (it - 1) : nullptr, cnt + it, o.type == EMAP_PLUGIN_MAX_FILTER);
        launch_mask_nan(ctx->stream, (long)L, (o.i1 & 1) ? v1 : v0, (o.i1 & 1) ? m1 : m0, dst);
        cnt += op_counters(o);
      } break;
      case EMAP_PLUGIN_SMOOTH:
        launch_smooth2(ctx->stream, C, src, dst);
        break;
      case EMAP_PLUGIN_EROSION: {
        float* red = ctx->chain_red + (size_t)k * EM_RANGE_FLOATS;      // [0 .. 3): lo, hi, has-NaN; behind them the partial triples
        const int rev = (o.flags & EMAP_PLUGIN_REVERSE) ? 1 : 0;
        float *a = scr, *b = scr + L;
        launch_range(ctx->stream, (long)L, src, rev, red + 4, red);
        launch_quantise(ctx->stream, (long)L, src, rev, red, a);
        for (int it = 0; it < o.i1; ++it) { launch_erode(ctx->stream, C, o.i0, a, b); float* t = a; a = b; b = t; }
        launch_dequantise(ctx->stream, (long)L, a, src, rev, red, dst);      // (src may be dst: element i is read before it is written, by one thread)
      } break;
      case EMAP_PLUGIN_INPAINT_FRONTS: {
        // max d is not read back: d is the L1 distance to a known cell INSIDE the map, so max d <= 2 C - 2, and the launches behind the last
        // front return at their first test (emap_inpaint_fronts.hip: k_fr_advance)
        const int S = inpaint_steps(o);
        const FrontsDev f = fronts_carve(inp, C, C, S);
        InpRange* parts = reinterpret_cast<InpRange*>(inp + fronts_bytes(C, C, S));
        InpRange* rec = parts + EM_INP_PARTS;
        inp += op_inpaint_bytes(ctx, o);
        launch_inpaint_range(ctx->stream, ctx->kp, ctx->cells, parts, rec);
        launch_inpaint_quantise(ctx->stream, ctx->kp, ctx->cells, rec, f.in, f.mask);
        launch_fronts(ctx->stream, f, C, C, S, (2 * C - 2 + S - 1) / S);
        launch_inpaint_dequantise(ctx->stream, ctx->kp, ctx->cells, rec, f.out, dst);
      } break;
      case EMAP_PLUGIN_SEMANTIC_FILTER: case EMAP_PLUGIN_SEMANTIC_TRAV: case EMAP_PLUGIN_MAX_LAYER: case EMAP_PLUGIN_FEATURES_PCA: {
        PlugSrcs S; PlugPars R;
        memset(&S, 0, sizeof(S)); memset(&R, 0, sizeof(R));
        S.n = o.i0; S.sem_plane = (long)ctx->ncells_alloc; S.sem = ctx->sem; S.planes = ctx->plane_buf;
        for (int j = 0; j < o.i0; ++j) {
          const emap_plugin_src& q = srcs[o.src_index + j];
          S.code[j] = (unsigned short)((q.kind << 8) | q.index);
          if (j < EM_PLUG_PAR_MAX) { R.flags[j] = q.flags; R.f0[j] = q.f0; R.f1[j] = q.f1; R.d0[j] = q.d0; }
        }
        if (o.type == EMAP_PLUGIN_SEMANTIC_FILTER) launch_semantic_filter(ctx->stream, ctx->kp, ctx->cells, S, dst);
        else if (o.type == EMAP_PLUGIN_SEMANTIC_TRAV) launch_semantic_trav(ctx->stream, ctx->kp, ctx->cells, S, R, dst);
        else if (o.type == EMAP_PLUGIN_MAX_LAYER) launch_max_layer(ctx->stream, ctx->kp, ctx->cells, S, R, (o.flags & EMAP_PLUGIN_MIN) ? 1 : 0, dst);
        else { launch_features_pca(ctx->stream, ctx->kp, ctx->cells, S, pcs, dst); pcs += EM_PCA_DOUBLES; }
      } break;
      default:
        launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 0, scr);
        launch_get_plane(ctx->stream, ctx->kp, ctx->cells, 2, scr + L);
        launch_robot_centric(ctx->stream, C, (float)ctx->prm.resolution, rotation9, (o.flags & EMAP_PLUGIN_THRESHOLD) ? 1 : 0, o.f0, scr, scr + L, dst);
        break;
    }
    CK(hipGetLastError());
  }
  return EMAP_OK;
}

}  // namespace
