// C ABI of the MI355X elevation-map fusion core (declared in include/emap_hip.h), the core of its host side: context lifecycle, the
// small-frame ring, the cloud upload, the staged entry points, state access and the frame pipeline.  (Semantic layers and the camera
// path: emap_api_semantic.hip; publish-time plugins: emap_api_plugins.hip; halos, communicator, rays by ray: emap_api_comm.hip.)
// Host-side orchestration only: owns device memory, turns emap_params into kernargs, enqueues the kernels of
// emap_kernels.hip on ONE stream in the order of the reference's update_map_with_kernel
// (EM/elevation_mapping.py:316-391).  No per-frame allocation, no D2H sync inside a frame unless stats are asked for.
#include "emap_host.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace emap_host;

float emap_host::q16(float x) { return (float)(_Float16)x; }
// The k_small_frame launches that are issued and not yet known to be applied (emap_ctx::sf_ring).  sf_settle waits until the device
// has decided the fate of the last of them (a poll of a host-mapped word: the decision falls at the launch's second barrier, long
// before the stream is idle), forgets those that will be applied, and after an ABORT (the launch left everything as it found it, the
// launches behind it did nothing: emap_kernels.hip) drains the stream and re-runs the aborted frame and every one after it, in order,
// on the chain of launches, each on the cloud that was bound when it was issued.  Every entry point that reads or changes the map, the
// drift record or a cloud buffer passes through SF_CHECK first; binding another device cloud and emap_update's own small-frame path do
// not (frames pipeline), they only make room in the ring.
static int frame_impl(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats, bool sharded);
static void sf_forget_applied(emap_ctx* ctx) {
  const unsigned int passed = ctx->sf_host[0];
  while (ctx->sf_count > 0 && ctx->sf_ring[ctx->sf_head].epoch <= passed) { ctx->sf_head = (ctx->sf_head + 1) % emap_ctx::SF_RING; --ctx->sf_count; }
}
static int sf_recover(emap_ctx* ctx) {
  CK(hipSetDevice(ctx->device));
  CK(hipStreamSynchronize(ctx->stream));      // the aborted launch, the idle ones behind it and their stencil launches have drained
  const unsigned int first = ctx->sf_host[1];
  ctx->sf_host[1] = 0u;
  CK(hipMemset(ctx->sf_poison, 0, 4));
  // the binding of the moment (maybe a cloud for a frame that has not been issued yet) comes back afterwards
  const BoundCloud bound = ctx->cloud;
  const bool fsem_set = ctx->fsem_set; ctx->fsem_set = false;      // (a fusion declared for the frame to come is not the re-run frames')
  int rc = EMAP_OK;
  ctx->sf_redo = true;
  bool first_done = false;
  while (ctx->sf_count > 0) {
    const emap_ctx::SfFrame f = ctx->sf_ring[ctx->sf_head];
    ctx->sf_head = (ctx->sf_head + 1) % emap_ctx::SF_RING; --ctx->sf_count;
    if (f.epoch < first) continue;            // applied before the abort
    if (!first_done) { ctx->kp.mv = f.mv; first_done = true; }      // the pending map shifts the aborted launch was to write out (later frames: none, no shift can lie between unsettled frames)
    ctx->cloud = f.cloud;
    ++ctx->sf_aborts;
    if (rc == EMAP_OK) rc = frame_impl(ctx, f.R, f.t, f.pn, f.on, nullptr, false);
  }
  ctx->sf_redo = false; ctx->fsem_set = fsem_set;
  ctx->cloud = bound;
  return rc;
}
int emap_host::sf_settle(emap_ctx* ctx) {
  if (ctx->sf_redo || ctx->sf_count == 0) return EMAP_OK;
  const unsigned int last = ctx->sf_ring[(ctx->sf_head + ctx->sf_count - 1) % emap_ctx::SF_RING].epoch;
  for (long spins = 0; ctx->sf_host[1] == 0u && ctx->sf_host[0] < last; ++spins) {
    if (spins > (1L << 22)) {                 // (something else is very slow on this stream: wait for it the ordinary way)
      CK(hipSetDevice(ctx->device)); CK(hipStreamSynchronize(ctx->stream));
      if (ctx->sf_host[1] == 0u && ctx->sf_host[0] < last) { ctx->err = "k_small_frame finished without reporting its outcome"; return EMAP_ERR_HIP; }
      break;
    }
  }
  if (ctx->sf_host[1] != 0u) return sf_recover(ctx);
  sf_forget_applied(ctx);
  return EMAP_OK;
}

static void build_kp(emap_ctx* ctx) {
  const emap_params& p = ctx->prm;
  KP& k = ctx->kp;
  const KP old = k;
  memset(&k, 0, sizeof k);
  k.org_r = old.org_r; k.org_c = old.org_c; k.norg_r = old.norg_r; k.norg_c = old.norg_c; k.mv = old.mv;   // map-shift state survives a parameter update
  k.C = p.cell_n; k.mode = p.mode; k.row0 = ctx->strip.row_begin; k.nrows = ctx->strip.row_count; k.halo = ctx->strip.halo_rows;
  k.edge = p.enable_edge_sharpen; k.dil = p.dilation_size;
  k.res = p.resolution; k.half_w = 0.5 * p.cell_n; k.snf = p.sensor_noise_factor; k.mt = p.mahalanobis_thresh;
  k.ov = p.outlier_variance; k.dcvi_half = p.drift_compensation_variance_inlier / 2.0; k.trav_inlier = p.traversability_inlier;
  k.wall = p.wall_num_thresh; k.mrl = p.max_ray_length; k.cs = p.cleanup_step; k.cos_thresh = p.cleanup_cos_thresh;
  k.mvd2 = p.min_valid_distance * p.min_valid_distance; k.mhr = p.max_height_range;
  k.ra = p.ramped_height_range_a; k.rb = p.ramped_height_range_b; k.rc = p.ramped_height_range_c;
  k.max_var = p.max_variance; k.ray_step = p.ray_step;
  k.init_var = (float)p.initial_variance; k.ov_f = (float)p.outlier_variance;
  const bool h = p.mode == EMAP_MODE_REFERENCE_FP16;
  k.q_wm1 = h ? q16((float)(p.cell_n - 1)) : (float)(p.cell_n - 1);
  k.q_mrl = h ? q16((float)p.max_ray_length) : (float)p.max_ray_length;
  k.q_step = h ? q16((float)p.ray_step) : (float)p.ray_step;
  k.time_var = (float)p.time_variance; k.time_int = (float)p.time_interval; k.res_f = (float)p.resolution;
  k.inv_res_f = (float)(1.0 / p.resolution); k.half_w_f = 0.5f * (float)p.cell_n; k.cm1_f = (float)(p.cell_n - 1);
  k.hw_int_f = (float)(p.cell_n / 2); k.hw_frac_f = (p.cell_n & 1) ? 0.5f : 0.0f; k.pad1 = 0.f;
  k.col0 = 0; k.ncols = p.cell_n; k.pitch = p.cell_n; k.wmode = 0;
}

// smallest float >= c (a < c  <=>  a < up(c) for float a) / largest float <= c (a > c <=> a > dn(c))
static float f_up(double c) { float f = (float)c; if ((double)f < c) f = nextafterf(f, INFINITY); return f; }
static float f_dn(double c) { float f = (float)c; if ((double)f > c) f = nextafterf(f, -INFINITY); return f; }

static int host_axis_idx(const emap_params& p, float xq, float q_wm1, bool half_mode) {
  if (!half_mode) {   // fp32 mode: float multiply + float add, truncation, integer clamp (emap_device.h: axis_idx<1>)
    volatile float m = xq * (float)(1.0 / p.resolution);
    volatile float vf = m + 0.5f * (float)p.cell_n;
    const float f = vf;
    int i = !(f == f) ? 0 : (f >= 2147483648.0f ? 2147483647 : (f <= -2147483648.0f ? (int)0x80000000 : (int)f));
    return i < 0 ? 0 : (i > p.cell_n - 1 ? p.cell_n - 1 : i);
  }
  double v = (double)xq / p.resolution + 0.5 * p.cell_n;
  int i = !(v == v) ? 0 : (v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (int)0x80000000 : (int)v));
  float fi = half_mode ? q16((float)i) : (float)i;
  float r = fmaxf(fminf(fi, q_wm1), 0.0f);
  return (int)r;
}

// Tables of the visibility pass: step sequence (custom_kernels.py:203) and, for reference_fp16, the
// half-bits -> cell-index table (custom_kernels.py:22-33,45-49 evaluated exactly on the host).
static int build_ray_tables(emap_ctx* ctx) {
  const emap_params& p = ctx->prm;
  const bool h = p.mode == EMAP_MODE_REFERENCE_FP16;
  RayTab& rt = ctx->rt;
  if (ctx->ray_S) { CK(hipStreamSynchronize(ctx->stream)); CK(hipFree(ctx->ray_S)); ctx->ray_S = nullptr; }
  if (ctx->ray_lut) { CK(hipStreamSynchronize(ctx->stream)); CK(hipFree(ctx->ray_lut)); ctx->ray_lut = nullptr; }
  memset(&rt, 0, sizeof rt);
  std::vector<float> S;
  const float q_mrl = ctx->kp.q_mrl;
  float s = ctx->kp.q_step;
  while (s < q_mrl) {
    if (S.size() >= 8192u) {                  // the table is staged in LDS (<= 32 KB): refuse instead of silently shortening the rays
      ctx->err = "max_ray_length / ray_step needs more than 8192 ray samples"; return EMAP_ERR_INVALID; }
    S.push_back(s);
    float nx = (float)((double)s + p.ray_step);
    if (h) nx = q16(nx);
    if (!(nx > s)) break;   // half saturated: the reference's loop would never terminate here
    s = nx;
  }
  rt.nS = (int)S.size();
  if (rt.nS) {
    CK(hipMalloc((void**)&ctx->ray_S, sizeof(float) * S.size()));
    CK(hipMemcpyAsync(ctx->ray_S, S.data(), sizeof(float) * S.size(), hipMemcpyHostToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
  }
  rt.S = ctx->ray_S;
  rt.f_d_thresh = f_up(0.1); rt.f_cos_thresh = f_up(p.cleanup_cos_thresh); rt.f_wall = f_dn(p.wall_num_thresh);
  if (h) {
    std::vector<int> full(65536);
    for (int b = 0; b < 65536; ++b) {
      unsigned short us = (unsigned short)b; _Float16 hf; memcpy(&hf, &us, 2);
      full[b] = host_axis_idx(p, (float)hf, ctx->kp.q_wm1, true);
    }
    auto at = [&](int sg, int mag) { return full[(sg << 15) | mag]; };
    {   // AxisIdx<0, 2>: is the float formula exact for every half pattern (NaNs excluded: non-finite samples never march)?
      bool same = true;
      // index = floor(q / res [+ 0.5 for odd cell_n]) + cell_n / 2, clamped: the floor is taken BEFORE the half width is added (a tiny
      // negative coordinate would otherwise round up to exactly cell_n / 2 in fp32, where the reference's double truncates below it)
      const float inv = ctx->kp.inv_res_f, hwi = ctx->kp.hw_int_f, hwf = ctx->kp.hw_frac_f, cm1 = ctx->kp.cm1_f;
      for (int b = 0; b < 65536 && same; ++b) {
        if ((b & 0x7fff) > 0x7c00) continue;
        unsigned short us = (unsigned short)b; _Float16 hf; memcpy(&hf, &us, 2);
        const float q = (float)hf, f = floorf(fmaf(q, inv, hwf)) + hwi;
        const int got = (int)fminf(fmaxf(f, 0.0f), cm1);
        if (got != full[b]) same = false;
      }
      rt.formula_ok = same ? 1 : 0;
      ctx->kp.idx_formula = rt.formula_ok;       // the point passes index with the same formula (geometry())
      if (const char* e = getenv("EMAP_RAY_IDX")) { if (atoi(e) != 2) rt.formula_ok = 0; }     // test / tuning hook: force the table path
    }
    int lo = 0x7c00, hi = 1;
    for (int sg = 0; sg < 2; ++sg) {
      for (int m = 1; m < 0x7c00; ++m) if (at(sg, m) != at(sg, 1)) { if (m < lo) lo = m; break; }
      for (int m = 0x7bff; m >= 1; --m) if (at(sg, m) != at(sg, 0x7c00)) { if (m + 1 > hi) hi = m + 1; break; }
    }
    if (hi < lo) { hi = lo; }
    // verify the compact form against the full table (every pattern), else fall back to in-kernel arithmetic
    bool ok = at(0, 0) == at(0, 1) && at(1, 0) == at(0, 1);
    rt.small_pos = at(0, 1); rt.small_neg = at(1, 1); rt.big_pos = at(0, 0x7c00); rt.big_neg = at(1, 0x7c00); rt.nan_val = at(0, 0x7e00);
    for (int sg = 0; sg < 2 && ok; ++sg)
      for (int m = 1; m < 0x8000; ++m) {
        int want = at(sg, m), got;
        if (m >= lo && m < hi) continue;
        if (m < lo) got = sg ? rt.small_neg : rt.small_pos; else if (m > 0x7c00) got = rt.nan_val; else got = sg ? rt.big_neg : rt.big_pos;
        if (got != want) { ok = false; break; }
      }
    const size_t entries = (size_t)2 * (hi - lo);
    if (ok && entries > 0 && lo >= 1 && (entries + 4) * 2 <= 60 * 1024 && p.cell_n <= 65535) {
      const size_t span = (size_t)(hi - lo) + 2;   // per sign: [small, idx(lo..hi-1), big]
      std::vector<unsigned short> lut(2 * span + 2);
      for (int sg = 0; sg < 2; ++sg) {
        lut[sg * span] = (unsigned short)(sg ? rt.small_neg : rt.small_pos);
        for (int m = lo; m < hi; ++m) lut[sg * span + 1 + (m - lo)] = (unsigned short)at(sg, m);
        lut[sg * span + span - 1] = (unsigned short)(sg ? rt.big_neg : rt.big_pos);
      }
      CK(hipMalloc((void**)&ctx->ray_lut, sizeof(unsigned short) * lut.size()));
      CK(hipMemcpyAsync(ctx->ray_lut, lut.data(), sizeof(unsigned short) * lut.size(), hipMemcpyHostToDevice, ctx->stream));
      CK(hipStreamSynchronize(ctx->stream));
      rt.lut = ctx->ray_lut; rt.lo = lo; rt.hi = hi;
    }
  }
  return EMAP_OK;
}

Pose emap_host::make_pose(const emap_ctx* ctx, const float R[9], const float t[3]) {
  Pose T;
  const bool h = ctx->prm.mode == EMAP_MODE_REFERENCE_FP16;
  for (int i = 0; i < 9; ++i) T.Rq[i] = h ? q16(R[i]) : R[i];
  for (int i = 0; i < 3; ++i) { T.tq[i] = h ? q16(t[i]) : t[i]; T.t[i] = t[i] + 0.0f; }   // -0.0 -> +0.0 (same arithmetic, see IdxLut)
  return T;
}

// Map shifts are lazy (emap_shift): kernels of the frame replay them, everything else sees them written out first.
int emap_host::flush_moves(emap_ctx* ctx) {
  if (ctx->kp.mv.n == 0) return EMAP_OK;
  launch_materialize(ctx->stream, ctx->kp, ctx->cells);
  ctx->kp.mv.n = 0;
  CK(hipGetLastError());
  return EMAP_OK;
}

// The last frame's stencil pass, left pending by frame_impl for the next frame's fused launch: launched now, exactly as the frame would
// have launched it.  On an error the pass stays pending.
// A pass that a frame took along LEAN (count_impl: only the outputs that frame reads, or no launch at all) is still pending, and what is
// launched here is always the FULL k_post on the map as it is.  The invariant that makes the lean launch safe: between it and the next
// full pass no entry point reads or changes the map, its planes, its origin or its parameters without passing through this function
// (SF_CHECK; tests/test_post_settle_surface.py holds the list of the calls that pass by, none of which looks at a plane), the frame
// that made the lean launch ends with a pass of its own -- pending again, or launched in full -- and a frame that fails in between
// returns with the flag still set.  Every output is a pure function of the map, so the late full pass writes what an early one would have.
static int post_part_impl(emap_ctx* ctx, int32_t part);
int emap_host::post_settle(emap_ctx* ctx) {
  if (!ctx->post_pending) return EMAP_OK;
  const int rc = post_part_impl(ctx, 0);
  if (rc == EMAP_OK) ctx->post_pending = false;
  return rc;
}

// rows between the origin the normal planes were written with and the map's origin (signed, shortest way round)
int emap_host::normal_row_lag(const emap_ctx* ctx) {
  const int C = ctx->prm.cell_n;
  int d = ((ctx->kp.norg_r - ctx->kp.org_r) % C + C) % C;
  return d > C / 2 ? d - C : d;
}

int emap_host::plugin_scratch(emap_ctx* ctx, size_t planes, int counters) {
  int rc = grow(ctx, &ctx->plug_buf, &ctx->plug_cap, planes * (size_t)ctx->prm.cell_n * ctx->prm.cell_n); if (rc) return rc;
  return grow(ctx, &ctx->plug_cnt, &ctx->plug_cnt_cap, (size_t)counters);
}

static int validate(const emap_params* p, const emap_strip* s, std::string* why) {
  if (!p) { *why = "params null"; return 0; }
  if (p->cell_n < 8 || p->cell_n > 46340) { *why = "cell_n out of range"; return 0; }
  if (p->mode != EMAP_MODE_REFERENCE_FP16 && p->mode != EMAP_MODE_FP32) { *why = "bad mode"; return 0; }
  if (p->mode == EMAP_MODE_REFERENCE_FP16 && p->cell_n > 2049) {
    *why = "reference_fp16 index mode is only defined for cell_n <= 2049 (half cannot hold larger indices)"; return 0; }
  if (!(p->resolution > 0)) { *why = "resolution must be > 0"; return 0; }
  if (p->dilation_size < 0 || p->dilation_size > 32) { *why = "dilation_size out of range"; return 0; }
  if (s) {
    if (s->row_begin < 0 || s->row_count <= 0 || s->row_begin + s->row_count > p->cell_n || s->halo_rows < 0) {
      *why = "bad strip"; return 0; }
  }
  return 1;
}

// the copy stream, its events and the host worker threads of the upload paths, made at the first upload (stage_send: the workers)
int emap_host::upload_setup(emap_ctx* ctx) {
  if (ctx->copy_stream) return EMAP_OK;
  CK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) { CK(hipEventCreateWithFlags(&ctx->ev_copied[k], hipEventDisableTiming)); CK(hipEventCreateWithFlags(&ctx->ev_used[k], hipEventDisableTiming)); }
  int nt = (int)std::thread::hardware_concurrency() / 2; if (nt > 8) nt = 8; if (nt < 1) nt = 1;
  if (const char* e = getenv("EMAP_UPLOAD_THREADS")) { int v = atoi(e); if (v >= 1 && v <= 64) nt = v; }
  ctx->workers = new Workers(nt);
  return EMAP_OK;
}

// ---- Stage (emap_host.h) ----------------------------------------------------------------------------------------------------------
int emap_host::stage_next(emap_ctx* ctx, Stage* s, size_t pin_bytes, size_t dev_bytes) {
  const int sl = s->slot ^= 1;
  if (!s->ev[sl]) CK(hipEventCreateWithFlags(&s->ev[sl], hipEventDisableTiming));
  if (s->ev_on[sl]) { CK(hipEventSynchronize(s->ev[sl])); s->ev_on[sl] = false; }
  int rc = grow(ctx, &s->pin[sl], &s->pin_cap[sl], pin_bytes, Grow::pinned); if (rc) return rc;
  return grow(ctx, &s->dev, &s->dev_cap, dev_bytes);
}
// A message of a million points is 16-32 MB: one host thread copying it into the pinned slot would take longer than its DMA, so the
// workers share every chunk, and each chunk's DMA overlaps the copy of the next; a message of one chunk is one memcpy and one DMA.
int emap_host::stage_send(emap_ctx* ctx, Stage* s, const void* src, size_t bytes) {
  const int sl = s->slot;
  unsigned char* pin = s->pin[sl];
  const unsigned char* data = static_cast<const unsigned char*>(src);
  const size_t chunk = src ? (size_t)2 << 20 : bytes;
  if (bytes > chunk) { const int rc = upload_setup(ctx); if (rc) return rc; }
  for (size_t o = 0; o < bytes; o += chunk) {
    const size_t len = bytes - o < chunk ? bytes - o : chunk;
    if (bytes <= chunk) { if (src) memcpy(pin, data, len); }
    else ctx->workers->run([&](int w, int nw) {
      const size_t per = ((len + nw - 1) / nw + 63) & ~(size_t)63, a = (size_t)w * per;
      if (a < len) memcpy(pin + o + a, data + o + a, len - a < per ? len - a : per);
    });
    CK(hipMemcpyAsync(s->dev + o, pin + o, len, hipMemcpyHostToDevice, ctx->stream));
  }
  CK(hipEventRecord(s->ev[sl], ctx->stream));
  s->ev_on[sl] = true;
  return EMAP_OK;
}
void emap_host::stage_free(Stage* s) {
  for (int k = 0; k < 2; ++k) { if (s->pin[k]) hipHostFree(s->pin[k]); if (s->ev[k]) hipEventDestroy(s->ev[k]); }
  hipFree(s->dev);
  *s = Stage{};
}

extern "C" {

int emap_abi_version(void) { return EMAP_ABI_VERSION; }

const char* emap_last_error(const emap_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int emap_destroy(emap_ctx* ctx) {
  if (!ctx) return EMAP_OK;
  hipSetDevice(ctx->device);
  if (ctx->post_pending) post_settle(ctx);      // (the stream ends with the complete frame, whoever looks at it next)
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  hipFree(ctx->cells.hot); hipFree(ctx->cells.cold); hipFree(ctx->acc); hipFree(ctx->accr); hipFree(ctx->trav_in); hipFree(ctx->trav_flag);
  hipFree(ctx->normal); hipFree(ctx->scratch); hipFree(ctx->plug_buf); hipFree(ctx->plug_cnt); hipFree(ctx->slots); hipFree(ctx->frame); hipFree(ctx->cnt_sync);
  for (int k = 0; k < 2; ++k) { hipFree(ctx->pts_dev[k]); if (ctx->pts_pin[k]) hipHostFree(ctx->pts_pin[k]); if (ctx->ev_copied[k]) hipEventDestroy(ctx->ev_copied[k]); if (ctx->ev_used[k]) hipEventDestroy(ctx->ev_used[k]); }
  hipFree(ctx->own_cloud); stage_free(&ctx->cloud_stage); stage_free(&ctx->image_stage);
  if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
  delete ctx->workers;
  hipFree(ctx->tail_idx); hipFree(ctx->tail_flags); hipFree(ctx->ray_S); hipFree(ctx->ray_lut); hipFree(ctx->inert); hipFree(ctx->inl_plane); hipFree(ctx->ray_thr);
  hipFree(ctx->bin_recs); hipFree(ctx->bin_own); hipFree(ctx->bin_own_cnt); hipFree(ctx->bin_hist); hipFree(ctx->bin_tile_total); hipFree(ctx->bin_tile_start); hipFree(ctx->bin_sync); hipFree(ctx->split_mem); hipFree(ctx->sem_split_mem); if (ctx->split_need) hipHostFree((void*)ctx->split_need); if (ctx->sf_host) hipHostFree((void*)ctx->sf_host); hipFree(ctx->frame_save); hipFree(ctx->sf_poison);
  hipFree(ctx->img_uv); hipFree(ctx->img_valid); hipFree(ctx->img_buf);
  hipFree(ctx->grid_buf);
  hipFree(ctx->poly_buf); if (ctx->poly_pin) hipHostFree(ctx->poly_pin);
  hipFree(ctx->sub_tab); hipFree(ctx->sub_out); if (ctx->sub_pin) hipHostFree(ctx->sub_pin);
  hipFree(ctx->cloud_tab); hipFree(ctx->cloud_out); if (ctx->cloud_pin) hipHostFree(ctx->cloud_pin);
  hipFree(ctx->pseg_buf); hipFree(ctx->pseg_slots); if (ctx->pseg_pin) hipHostFree(ctx->pseg_pin);
  hipFree(ctx->terr_buf); if (ctx->terr_pin) hipHostFree(ctx->terr_pin);
  hipFree(ctx->reg_buf); hipFree(ctx->reg_cracks); if (ctx->reg_pin) hipHostFree(ctx->reg_pin);
  hipFree(ctx->plane_buf); hipFree(ctx->chain_buf); hipFree(ctx->chain_cnt); hipFree(ctx->chain_red); hipFree(ctx->chain_inp); hipFree(ctx->chain_pca);
  hipFree(ctx->sem_alpha); hipFree(ctx->sem); hipFree(ctx->sem_sums); hipFree(ctx->sem_col); hipFree(ctx->cnt_plane);
  emap_comm_destroy(ctx);
  hipFree(ctx->win_state); hipFree(ctx->win_rec); hipFree(ctx->win_bits); hipFree(ctx->win_thr); hipFree(ctx->win_dh); hipFree(ctx->win_key); hipFree(ctx->win_red_dh); hipFree(ctx->win_red_key);
  for (int i = 0; i <= ST_N; ++i) if (ctx->ev[i]) hipEventDestroy(ctx->ev[i]);
  if (ctx->t0) hipEventDestroy(ctx->t0);
  if (ctx->t1) hipEventDestroy(ctx->t1);
  if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return EMAP_OK;
}

int emap_clear(emap_ctx* ctx) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  ctx->pseg_labels = nullptr;                                  // the labels of the last segmentation are not this map's any more
  // ElevationMap.clear (elevation_mapping.py:119-128): all planes 0, variance = initial_variance
  Cell z = {0.f, (float)ctx->prm.initial_variance, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  launch_fill_cells(ctx->stream, ctx->cells, ctx->ncells_alloc, z);
  ctx->kp.mv.n = 0;                   // every cell has just been written
  CK(hipMemsetAsync(ctx->acc, 0, sizeof(AccF) * ctx->ncells_alloc, ctx->stream));
  CK(hipMemsetAsync(ctx->accr, 0, sizeof(AccR) * ctx->ncells_alloc, ctx->stream));
  CK(hipMemsetAsync(ctx->slots, 0, sizeof(ErrSlot) * EM_ERR_SLOTS, ctx->stream));
  CK(hipMemsetAsync(ctx->frame, 0, sizeof(FrameDev), ctx->stream));
  if (ctx->split_need) {              // FrameDev::ray_class and its host-mapped mirror restart together (no frame is in flight after the wait)
    CK(hipStreamSynchronize(ctx->stream));
    ctx->split_need[1] = 0u;
  }
  ctx->committed = false;
  CK(hipGetLastError());
  return EMAP_OK;
}

int emap_create(const emap_params* params, const emap_strip* strip, int device, void* stream, emap_ctx** out) {
  if (!out) return EMAP_ERR_INVALID;
  *out = nullptr;
  std::string why;
  if (!validate(params, strip, &why)) { fprintf(stderr, "emap_create: %s\n", why.c_str()); return EMAP_ERR_INVALID; }
  emap_ctx* ctx = new (std::nothrow) emap_ctx();
  if (!ctx) return EMAP_ERR_INVALID;
  ctx->prm = *params;
  if (strip) ctx->strip = *strip; else { ctx->strip.row_begin = 0; ctx->strip.row_count = params->cell_n; ctx->strip.halo_rows = 0; ctx->strip.pad_ = 0; }
  ctx->device = device;
  ctx->bin_rs = 1;
  build_kp(ctx);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) { fprintf(stderr, "emap_create: hipSetDevice(%d): %s\n", device, hipGetErrorString(e)); delete ctx; return EMAP_ERR_HIP; }
  if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
  else { e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking); ctx->own_stream = true;
         if (e != hipSuccess) { fprintf(stderr, "emap_create: stream: %s\n", hipGetErrorString(e)); delete ctx; return EMAP_ERR_HIP; } }
  const long C = params->cell_n;
  ctx->ncells_alloc = (long)(ctx->strip.row_count + 2 * ctx->strip.halo_rows) * C;
  const long n = ctx->ncells_alloc;
  int rc = EMAP_OK;
  auto alloc = [&](void** p, size_t bytes) { if (rc == EMAP_OK && hipMalloc(p, bytes) != hipSuccess) { rc = EMAP_ERR_HIP; fprintf(stderr, "emap_create: hipMalloc(%zu) failed\n", bytes); } };
  alloc((void**)&ctx->cells.hot, sizeof(float4) * n); alloc((void**)&ctx->cells.cold, sizeof(float4) * n); alloc((void**)&ctx->acc, sizeof(AccF) * n); alloc((void**)&ctx->accr, sizeof(AccR) * n);
  alloc((void**)&ctx->trav_in, sizeof(float) * n); alloc((void**)&ctx->normal, sizeof(float) * 3 * n);
  alloc((void**)&ctx->scratch, sizeof(float) * n); alloc((void**)&ctx->slots, sizeof(ErrSlot) * EM_ERR_SLOTS);
  alloc((void**)&ctx->frame, sizeof(FrameDev));
  alloc((void**)&ctx->cnt_sync, sizeof(unsigned int) * EM_TICKET_WORDS);      // tickets of k_count's folded gate (zero between launches)
  alloc((void**)&ctx->inert, sizeof(unsigned long long) * ((size_t)ctx->strip.row_count * ((C + 63) / 64) + 2));      // + an all-ones word behind the last row (k_rays)
  if (rc == EMAP_OK) {
    hipEventCreate(&ctx->t0); hipEventCreate(&ctx->t1);
    for (int i = 0; i <= ST_N; ++i) hipEventCreate(&ctx->ev[i]);
    hipMemsetAsync(ctx->trav_in, 0, sizeof(float) * n, ctx->stream);
    hipMemsetAsync(ctx->cnt_sync, 0, sizeof(unsigned int) * EM_TICKET_WORDS, ctx->stream);
    hipMemsetAsync(ctx->inert + (size_t)ctx->strip.row_count * ((C + 63) / 64), 0xff, 2 * sizeof(unsigned long long), ctx->stream);
    hipMemsetAsync(ctx->normal, 0, sizeof(float) * 3 * n, ctx->stream);
    rc = emap_clear(ctx);
    if (rc == EMAP_OK) rc = build_ray_tables(ctx);
    if (rc == EMAP_OK) {
      // ElevationMap.__init__: traversability plane starts at 1 (elevation_mapping.py:84)
      Cell z = {0.f, (float)params->initial_variance, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
      launch_fill_cells(ctx->stream, ctx->cells, n, z);
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = EMAP_ERR_HIP;
    }
  }
  if (rc != EMAP_OK) { emap_destroy(ctx); return rc; }
  *out = ctx;
  return EMAP_OK;
}

int emap_set_params(emap_ctx* ctx, const emap_params* params) {
  CKARG(ctx && params, "null argument"); SF_CHECK();
  CKARG(params->cell_n == ctx->prm.cell_n, "cell_n cannot change");
  std::string why;
  if (!validate(params, &ctx->strip, &why)) { ctx->err = why; return EMAP_ERR_INVALID; }
  ctx->prm = *params;
  build_kp(ctx);
  CK(hipSetDevice(ctx->device));
  return build_ray_tables(ctx);
}

int emap_sync(emap_ctx* ctx) {
  CKARG(ctx, "null ctx"); CK(hipSetDevice(ctx->device));
  if (ctx->post_pending) SF_CHECK();            // the last frame's stencil pass is queued before the wait
  CK(hipStreamSynchronize(ctx->stream));
  if (ctx->sf_count > 0) { SF_CHECK(); CK(hipStreamSynchronize(ctx->stream)); }      // (an aborted small frame is re-run before the caller is told the stream is idle)
  return EMAP_OK;
}

// ---- point cloud --------------------------------------------------------------------------------------
// Which points of a cloud can land in THIS strip's rows under the pose (R, t map-centre relative)?  A conservative host-side test in
// double arithmetic: the kernels decide the row with the index mode's own rounding (emap_device.h: geometry / axis_idx -- in
// reference_fp16 mode coordinates, R and t pass through binary16), so the row estimate gets a margin that bounds every rounding on
// that path (2^-10 relative on every term in reference_fp16 mode, 2^-20 in fp32 mode) plus two cells; points outside the map clamp to
// its first / last row like the kernels' index does.  A point with a NaN coordinate is skipped by every kernel: never kept; one the
// test cannot place (non-finite row estimate, magnitudes beyond binary16) is kept everywhere.  The kept set is a SUPERSET of the
// points the strip's kernels act on, in the cloud's order -- so the strip's maps stay bit-identical (the kernels repeat the exact test).
struct StripKeep {
  double R0, R1, R2, t0, res, eps, half_c; int C, ls, nrows; bool half_mode;
  StripKeep(const emap_ctx* ctx, const float R[9], const float t[3]) {
    const emap_params& p = ctx->prm;
    R0 = R[0]; R1 = R[1]; R2 = R[2]; t0 = t[0]; res = p.resolution; C = p.cell_n; half_c = 0.5 * C;
    half_mode = p.mode == EMAP_MODE_REFERENCE_FP16;
    eps = half_mode ? 1.0 / 1024.0 : 1.0 / 1048576.0;
    ls = ((ctx->strip.row_begin - ctx->kp.org_r) % C + C) % C;      // logical row of the strip's first physical row
    nrows = ctx->strip.row_count;
  }
  bool operator()(double x, double y, double z) const {
    if (x != x || y != y || z != z) return false;
    const double a = R0 * x, b = R1 * y, c = R2 * z, xf = a + b + c + t0;
    if (!(std::fabs(xf) <= 1.0e30) || (half_mode && (std::fabs(x) > 60000.0 || std::fabs(y) > 60000.0 || std::fabs(z) > 60000.0 || std::fabs(xf) > 60000.0))) return true;
    const double m = eps * (2.0 * (std::fabs(a) + std::fabs(b) + std::fabs(c)) + std::fabs(t0) + std::fabs(xf)) + 2.0 * res;
    auto row = [&](double v) { const double r = std::floor(v / res + half_c); return r < 0.0 ? 0 : (r > C - 1 ? C - 1 : (int)r); };
    const int lo = row(xf - m), hi = row(xf + m);
    const int d = ((lo - ls) % C + C) % C;
    return d < nrows || d + (hi - lo) >= C;
  }
};

// conversion + (optional) order-preserving compaction of a host cloud into the pinned slot and out to the device, chunk by chunk
static int upload_impl(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype, const StripKeep* keep, int64_t* n_kept) { SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long tot = (long)n * stride + (stride > 3 ? 64 : 0);      // (+ the padding in front of the channel matrix)
  { const int rc = upload_setup(ctx); if (rc) return rc; }
  // everything enqueued so far may read the buffer of the previous upload: mark the point after which that buffer is free again
  if (ctx->up_used[ctx->up_slot]) CK(hipEventRecord(ctx->ev_used[ctx->up_slot], ctx->stream));
  const int sl = ctx->up_slot ^= 1;
  // this slot's device buffer was read by the kernels before the previous upload, its pinned memory by the DMA two uploads ago
  if (ctx->up_used[sl]) { CK(hipEventSynchronize(ctx->ev_used[sl])); CK(hipEventSynchronize(ctx->ev_copied[sl])); }
  // (no stream drain: the two waits above cover every reader, and a drain would serialise the upload against the frame in front)
  { const int rc = grow(ctx, &ctx->pts_dev[sl], &ctx->pts_cap[sl], (size_t)tot, Grow::covered); if (rc) return rc; }
  { const int rc = grow(ctx, &ctx->pts_pin[sl], &ctx->pin_cap[sl], (size_t)tot, Grow::pinned); if (rc) return rc; }
  // A cloud with extra channels is DE-INTERLEAVED on the way (CloudLayout) -- the conversion touches every element anyway -- so that the frame's point
  // passes stream 12 bytes per point instead of 12 + 4 K and the semantic fusion reads one K-float record per point.
  // With `keep` (row strips, emap_upload_points_strip) only the points that pass it are written, in order: every worker counts the
  // survivors of its share of the chunk, the shares' offsets follow, a second pass over the (cache-resident) share writes them.
  const long K = stride - 3, chan_off = cloud_layout((long)n, K).chan_off;
  long kept = 0;
  if (tot > 0) {
    float* pin = ctx->pts_pin[sl];
    const long cp = (1L << 19) / stride > 0 ? (1L << 19) / stride : 1;      // points per chunk: about 2 MB of float32 per DMA
    std::vector<long> cnt, off;
    for (long p0 = 0; p0 < (long)n; p0 += cp) {
      const long p1 = p0 + cp < (long)n ? p0 + cp : (long)n;
      long out0 = p0, out1 = p1;                                    // rows [out0, out1) of the device matrices this chunk fills
      auto coord = [&](long i, int k) -> double { return dtype == 0 ? (double)static_cast<const float*>(host)[i * stride + k] : static_cast<const double*>(host)[i * stride + k]; };
      if (keep) {
        cnt.assign(ctx->workers->th.size(), 0); off.assign(ctx->workers->th.size(), 0);
        ctx->workers->run([&](int w, int nw) {
          const long per = (p1 - p0 + nw - 1) / nw, a = p0 + (long)w * per, b = a + per < p1 ? a + per : p1;
          long c = 0;
          for (long i = a; i < b; ++i) c += (*keep)(coord(i, 0), coord(i, 1), coord(i, 2)) ? 1 : 0;
          cnt[w] = c;
        });
        long run = kept;
        for (size_t w = 0; w < cnt.size(); ++w) { off[w] = run; run += cnt[w]; }
        out0 = kept; out1 = run;
      }
      ctx->workers->run([&](int w, int nw) {
        const long per = (p1 - p0 + nw - 1) / nw, a = p0 + (long)w * per, b = a + per < p1 ? a + per : p1;
        if (b <= a) return;
        if (keep) {
          long o = off[w];
          for (long i = a; i < b; ++i) {
            const double x = coord(i, 0), y = coord(i, 1), z = coord(i, 2);
            if (!(*keep)(x, y, z)) continue;
            pin[3 * o] = (float)x; pin[3 * o + 1] = (float)y; pin[3 * o + 2] = (float)z;      // fp32 cast (:456)
            for (long k = 0; k < K; ++k) pin[chan_off + K * o + k] = (float)coord(i, 3 + (int)k);
            ++o;
          }
        } else if (K == 0) {
          if (dtype == 0) memcpy(pin + 3 * a, static_cast<const float*>(host) + 3 * a, sizeof(float) * 3 * (size_t)(b - a));
          else { const double* src = static_cast<const double*>(host); for (long i = 3 * a; i < 3 * b; ++i) pin[i] = (float)src[i]; }   // fp32 cast (:456)
        } else if (dtype == 0) {
          const float* src = static_cast<const float*>(host);
          for (long i = a; i < b; ++i) {
            const float* r = src + i * stride;
            pin[3 * i] = r[0]; pin[3 * i + 1] = r[1]; pin[3 * i + 2] = r[2];
            for (long k = 0; k < K; ++k) pin[chan_off + K * i + k] = r[3 + k];
          }
        } else {
          const double* src = static_cast<const double*>(host);
          for (long i = a; i < b; ++i) {
            const double* r = src + i * stride;
            pin[3 * i] = (float)r[0]; pin[3 * i + 1] = (float)r[1]; pin[3 * i + 2] = (float)r[2];
            for (long k = 0; k < K; ++k) pin[chan_off + K * i + k] = (float)r[3 + k];
          }
        }
      });
      kept = keep ? out1 : p1;
      if (out1 > out0) {
        CK(hipMemcpyAsync(ctx->pts_dev[sl] + 3 * out0, pin + 3 * out0, sizeof(float) * 3 * (size_t)(out1 - out0), hipMemcpyHostToDevice, ctx->copy_stream));
        if (K) CK(hipMemcpyAsync(ctx->pts_dev[sl] + chan_off + K * out0, pin + chan_off + K * out0, sizeof(float) * (size_t)K * (size_t)(out1 - out0), hipMemcpyHostToDevice, ctx->copy_stream));
      }
    }
    if (keep && kept == 0 && n > 0) {
      // none of the cloud's points can land in this strip's rows: bind ONE row of NaNs (skipped by every kernel, like any NaN row of a
      // cloud) so that the frame takes the same path -- launches, collectives -- as on the ranks that did get points
      pin[0] = pin[1] = pin[2] = NAN;
      for (long k = 0; k < K; ++k) pin[chan_off + k] = 0.f;
      CK(hipMemcpyAsync(ctx->pts_dev[sl], pin, sizeof(float) * 3, hipMemcpyHostToDevice, ctx->copy_stream));
      if (K) CK(hipMemcpyAsync(ctx->pts_dev[sl] + chan_off, pin + chan_off, sizeof(float) * (size_t)K, hipMemcpyHostToDevice, ctx->copy_stream));
      kept = 1;
    }
    CK(hipEventRecord(ctx->ev_copied[sl], ctx->copy_stream));
    CK(hipStreamWaitEvent(ctx->stream, ctx->ev_copied[sl], 0));     // kernels enqueued from now on see the cloud; nothing waits on the host
    ctx->up_used[sl] = true;
  }
  bind_split_cloud(ctx, ctx->pts_dev[sl], ctx->pts_dev[sl] + chan_off, keep ? kept : (long)n, (long)n, (int)K);
  if (n_kept) *n_kept = ctx->cloud.n;
  return EMAP_OK;
}

int emap_upload_points(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype) {
  CKARG(ctx, "null ctx");
  CKARG(n >= 0 && stride >= 3 && stride < 4096 && (dtype == 0 || dtype == 1), "bad point buffer description");
  CKARG(n == 0 || host, "null host buffer"); SF_CHECK();
  return upload_impl(ctx, host, n, stride, dtype, nullptr, nullptr);
}

// Row strips: every rank of a multi-GPU map is handed the SAME cloud (one sensor message), but only the points of its rows ever reach
// its tile kernels.  This entry point converts, uploads and binds only those (StripKeep: a conservative superset, order preserved), so a
// rank moves and streams 1 / G of the cloud: 8 x 192 MB over PCIe per 16 M-point frame on 8 GPUs become 192 MB.  The frame that follows
// must use the SAME pose (checked) and must not march its rays by row (every valid point marches a ray through every strip then:
// emap_update_sharded refuses); a cloud of a whole-map context is uploaded as by emap_upload_points.
int emap_upload_points_strip(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype, const float R[9], const float t[3], int64_t* n_kept) {
  CKARG(ctx && R && t, "null argument");
  CKARG(n >= 0 && stride >= 3 && stride < 4096 && (dtype == 0 || dtype == 1), "bad point buffer description");
  CKARG(n == 0 || host, "null host buffer"); SF_CHECK();
  if (ctx->strip.row_count >= ctx->prm.cell_n) return upload_impl(ctx, host, n, stride, dtype, nullptr, n_kept);
  const StripKeep keep(ctx, R, t);
  int rc = upload_impl(ctx, host, n, stride, dtype, &keep, n_kept);
  if (rc) return rc;
  ctx->pts_bucketed = true; ctx->bucket_org_r = ctx->kp.org_r;
  memcpy(ctx->bucket_R, R, sizeof ctx->bucket_R); memcpy(ctx->bucket_t, t, sizeof ctx->bucket_t);
  return EMAP_OK;
}

// the same predicate as data: keep[i] = 1 iff point i would be uploaded by emap_upload_points_strip (callers that keep their clouds
// on the device -- bench.py -- bucket them once with it; tests check the superset property against the exact cell indices)
int emap_strip_point_mask(emap_ctx* ctx, const void* host, int64_t n, int64_t stride, int dtype, const float R[9], const float t[3], uint8_t* keep_out) {
  CKARG(ctx && R && t && keep_out, "null argument");
  CKARG(n >= 0 && stride >= 3 && stride < 4096 && (dtype == 0 || dtype == 1), "bad point buffer description");
  CKARG(n == 0 || host, "null host buffer"); SF_CHECK();
  const bool whole = ctx->strip.row_count >= ctx->prm.cell_n;
  const StripKeep keep(ctx, R, t);
  for (int64_t i = 0; i < n; ++i) {
    const double x = dtype == 0 ? (double)static_cast<const float*>(host)[i * stride] : static_cast<const double*>(host)[i * stride];
    const double y = dtype == 0 ? (double)static_cast<const float*>(host)[i * stride + 1] : static_cast<const double*>(host)[i * stride + 1];
    const double z = dtype == 0 ? (double)static_cast<const float*>(host)[i * stride + 2] : static_cast<const double*>(host)[i * stride + 2];
    keep_out[i] = (whole || keep(x, y, z)) ? 1 : 0;
  }
  return EMAP_OK;
}

// A device-resident cloud the caller bucketed itself (with emap_strip_point_mask's predicate, for THIS pose): declares it, so that the
// frame checks pose and ray mode as for an uploaded one.
int emap_declare_points_bucketed(emap_ctx* ctx, const float R[9], const float t[3], int64_t n_all) {
  CKARG(ctx && R && t && n_all >= ctx->cloud.n, "bad argument"); SF_CHECK();
  if (ctx->strip.row_count >= ctx->prm.cell_n) return EMAP_OK;
  ctx->pts_bucketed = true; ctx->cloud.n_all = (long)n_all; ctx->bucket_org_r = ctx->kp.org_r;
  memcpy(ctx->bucket_R, R, sizeof ctx->bucket_R); memcpy(ctx->bucket_t, t, sizeof ctx->bucket_t);
  return EMAP_OK;
}

int emap_set_points_device_split(emap_ctx* ctx, const float* xyz_dev, const float* chan_dev, int64_t n, int64_t n_chan) {
  CKARG(ctx, "null ctx");
  CKARG(n >= 0 && n_chan >= 0 && n_chan < 4093 && (n == 0 || (xyz_dev && (n_chan == 0 || chan_dev))), "bad device point buffers");
  bind_split_cloud(ctx, xyz_dev, chan_dev, (long)n, (long)n, (int)n_chan);
  return EMAP_OK;
}

int emap_set_points_device(emap_ctx* ctx, const float* dev, int64_t n, int64_t stride) {
  CKARG(ctx, "null ctx");
  CKARG(n >= 0 && stride >= 3 && stride < 4096 && (n == 0 || dev), "bad device point buffer");
  ctx->cloud = BoundCloud{dev, (long)n, (int)stride, (long)n, ChanView{dev, (int)stride, 0}, (int)stride};      // interleaved rows: the channels sit behind xyz
  ctx->pts_bucketed = false;
  return EMAP_OK;
}

static int ensure_tail(emap_ctx* ctx) {
  int rc = grow(ctx, &ctx->tail_idx, &ctx->tail_idx_cap, (size_t)ctx->cloud.n); if (rc) return rc;
  return grow(ctx, &ctx->tail_flags, &ctx->tail_flags_cap, (size_t)ctx->cloud.n);
}

int emap_point_index(emap_ctx* ctx, const float R[9], const float t[3], int32_t* idx, uint8_t* valid, uint8_t* inside) {
  CKARG(ctx && R && t && idx && valid && inside, "null argument"); SF_CHECK();
  NEED_POINTS();
  CK(hipSetDevice(ctx->device));
  if (ctx->cloud.n == 0) return EMAP_OK;
  int rc = ensure_tail(ctx); if (rc) return rc;
  launch_point_index(ctx->stream, ctx->kp, make_pose(ctx, R, t), ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->tail_idx, ctx->tail_flags);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(idx, ctx->tail_idx, sizeof(int) * ctx->cloud.n, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(valid, ctx->tail_flags, ctx->cloud.n, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (long i = 0; i < ctx->cloud.n; ++i) { uint8_t f = valid[i]; valid[i] = f & 1; inside[i] = (f >> 1) & 1; }
  return EMAP_OK;
}

// ---- stages -----------------------------------------------------------------------------------------------

// bins of `sub` stacked 16 x 64 tiles: the smallest power of two that keeps the bin count within the LDS histogram
static int bin_sub(const emap_ctx* ctx) {
  const long tx = (ctx->prm.cell_n + 63) / 64;
  for (int sub = ctx->force_sub > 0 ? ctx->force_sub : 1; sub <= 64; sub *= 2) {
    const long ty = (ctx->strip.row_count + 16 * sub - 1) / (16 * sub);
    if (tx * ty <= BIN_MAX_T) return sub;
  }
  return 0;
}
static bool bins_possible(const emap_ctx* ctx) { return bin_sub(ctx) > 0; }
// Small clouds: two launches with global atomics win; large clouds: counting sort by tile + LDS reduction.  The crossover measured on
// MI355X lies at 60-135 k points for 202^2 .. 1024^2 maps.  n: the size of the WHOLE cloud -- a cloud bucketed for a
// strip decides by it, so every rank of a sharded frame takes the same path.
#define BIN_MIN_POINTS 131072
extern "C++" bool emap_host::takes_bins(const emap_ctx* ctx, long n) {
  return ctx->scatter_mode == 2 || (ctx->scatter_mode == 0 && bins_possible(ctx) && n >= BIN_MIN_POINTS);
}
static int ensure_bins(emap_ctx* ctx, bool raybin, const Frame* f) {
  const long n = ctx->cloud.n;
  BinGeo& g = ctx->bg;
  g.sub = bin_sub(ctx);
  g.tiles_x = (ctx->prm.cell_n + 63) / 64; g.tiles_y = (ctx->strip.row_count + 16 * g.sub - 1) / (16 * g.sub); g.T = g.tiles_x * g.tiles_y; g.TB = g.T + 1;
  g.pitch = (g.TB + 3) & ~3; g.raybin = raybin ? 1 : 0;
  // strip contexts without a visibility pass: cheap ownership test + lane compaction in the point passes (emap_binned.hip)
  // ... and strips whose frame marches its rays BY RAY: a rank then needs exactly the points of its rows (the valid ones that are not
  // is_inside ride in the ray-only bin) -- the other ranks march the rest
  // ... but not for a cloud that was BUCKETED for this strip on the host (emap_upload_points_strip): nearly every point is an owned one
  // then, the ownership pre-test and the staging record (16 B written + read per point) buy nothing -- the plain kernels sort 2 M
  // points in 42 us where the strip variants take 52
  // (a by-ray frame keeps the strip variants: there the EXACT ownership test decides which rank marches a point's ray -- a point the
  // host-side superset kept for two neighbouring strips must not ride in both ranks' ray-only bins)
  ctx->bin_strip = ctx->strip.row_count < ctx->prm.cell_n && (!raybin || (f && f->by_ray)) && !(ctx->pts_bucketed && !raybin);
  if (const char* e = getenv("EMAP_BIN_STRIP")) { if (atoi(e) == 0) ctx->bin_strip = false; }      // test / tuning hook
  // 32-byte records that carry the frame's semantic channels (frame_sem_begin): plain point passes only (a strip's staging records
  // hold no channels), never in front of a visibility pass (k_rays walks 16-byte records)
  ctx->bin_rs = (f && f->carry && !ctx->bin_strip && !raybin) ? 2 : 1;
  if (ctx->bin_rs == 1) ctx->carry.on = 0;
  // Blocks: ~4096 points each, but every block carries a row of the (block, tile) matrix through three passes (written, scanned,
  // read): keep the matrix (4 B x TB x B, x4) below the cloud's own traffic (12 B x n, x2) -- B <= n / (3 TB) -- without dropping
  // under one block per CU.  (8192^2 / 16 M points: 2048 blocks of 16385 bins were 537 MB of matrix traffic per frame.)
  long target = n >= 1000000 ? 4096 : 2048;
  if (const char* e = getenv("EMAP_BIN_CHUNK")) { long v = atol(e); if (v >= 256 && v <= 65536) target = v; }   // tuning knob
  long B = (n + target - 1) / target;
  long bmax = n / (3L * g.TB); if (bmax < 256) bmax = 256; if (bmax > BIN_MAX_B) bmax = BIN_MAX_B;
  if (B > bmax) B = bmax;
  if (B > 256) B -= B % 256;       // whole rounds of workgroups on the 256 CUs (325 blocks = one and a quarter rounds ran as long as 512)
  if (B < 1) B = 1;
  const long unit = ctx->bin_strip ? 4096 : 1024;   /* a multiple of every hist / scatter block size [x 4 loads in flight on strips] */
  long chunk = (n + B - 1) / B; chunk = ((chunk + unit - 1) / unit) * unit;
  g.B = (int)((n + chunk - 1) / chunk); if (g.B < 1) g.B = 1;
  g.chunk = chunk;
  int rc = grow(ctx, &ctx->bin_hist, &ctx->bin_hist_cap, (size_t)g.pitch * (size_t)g.B); if (rc) return rc;
  if (!ctx->bin_tile_total) {
    CK(hipMalloc((void**)&ctx->bin_tile_total, sizeof(unsigned int) * (BIN_MAX_T + 2)));
    CK(hipMalloc((void**)&ctx->bin_tile_start, sizeof(unsigned int) * (BIN_MAX_T + 2)));
    CK(hipMalloc((void**)&ctx->bin_sync, sizeof(unsigned int) * EM_TICKET_WORDS));
    CK(hipMemsetAsync(ctx->bin_sync, 0, sizeof(unsigned int) * EM_TICKET_WORDS, ctx->stream));
  }
  if (!ctx->split_mem) {           // scratch of the heavy tiles (SplitView): 40 bytes per cell of SPLIT_MAX_SLOTS tiles + the lists, zero between frames
    const size_t cells = (size_t)SPLIT_MAX_SLOTS * SPLIT_CELLS;
    const size_t words = (size_t)(BIN_MAX_T + 2) + SPLIT_MAX_EXTRA + 8 + SPLIT_MAX_SLOTS + 4 * cells, bytes = 4 * words + 8 * 3 * cells + 64;
    void* m = nullptr;
    CK(hipMalloc(&m, bytes));
    if (hipMemsetAsync(m, 0, bytes, ctx->stream) != hipSuccess) { hipFree(m); ctx->err = "hipMemsetAsync(split scratch)"; return EMAP_ERR_HIP; }
    ctx->split_mem = m;
    unsigned long long* q = reinterpret_cast<unsigned long long*>(m);          // the 64-bit planes first (alignment)
    ctx->split.h = q; ctx->split.v = q + cells; ctx->split.latest = q + 2 * cells;
    unsigned int* u = reinterpret_cast<unsigned int*>(q + 3 * cells);
    ctx->split.pts = u; ctx->split.inl = u + cells; ctx->split.cnt = u + 2 * cells; ctx->split.out = u + 3 * cells; u += 4 * cells;
    ctx->split.tick = u; u += SPLIT_MAX_SLOTS;
    ctx->split.tile_slot = u; u += BIN_MAX_T + 2;
    ctx->split.extra = u; u += SPLIT_MAX_EXTRA;
    ctx->split.n_extra = u;
    CK(hipHostMalloc((void**)&ctx->split_need, 64, hipHostMallocMapped));
    ctx->split_need[0] = 0u; ctx->split_need[1] = 0u;      // [0]: heavy-tile parts (k_bin_scan), [1]: the ray kernel the map's state asks for (k_ray_apply)
    CK(hipHostGetDevicePointer((void**)&ctx->split.need_host, const_cast<unsigned int*>(ctx->split_need), 0));
    ctx->split.on = 0;
  }
  if ((rc = grow(ctx, &ctx->bin_recs, &ctx->bin_recs_cap, (size_t)n * ctx->bin_rs))) return rc;
  if (ctx->bin_strip) {
    if ((rc = grow(ctx, &ctx->bin_own, &ctx->bin_own_cap, (size_t)g.B * chunk))) return rc;      // only the owned share is ever touched
    if (!ctx->bin_own_cnt) CK(hipMalloc((void**)&ctx->bin_own_cnt, sizeof(unsigned int) * (size_t)BIN_MAX_B));
  }
  return EMAP_OK;
}

int emap_set_scatter_mode(emap_ctx* ctx, int32_t mode) {
  const int m = mode & 0xff, sub = (mode >> 8) & 0xff;
  CKARG(ctx && m >= 0 && m <= 2 && (mode >> 16) == 0, "scatter mode: 0 auto, 1 atomic, 2 binned"); SF_CHECK();
  CKARG(sub == 0 || (sub <= 64 && (sub & (sub - 1)) == 0), "bin height factor must be a power of two <= 64");
  ctx->force_sub = sub;
  CKARG(m != 2 || bins_possible(ctx), "binned scatter: too many bins for the LDS histogram");
  ctx->scatter_mode = m;
  return EMAP_OK;
}

int emap_set_ray_mode(emap_ctx* ctx, int32_t mode) {
  CKARG(ctx && mode >= 0 && mode <= 2, "ray mode: 0 auto, 1 by row, 2 by ray"); SF_CHECK();
  ctx->ray_mode = mode;
  return EMAP_OK;
}

// the host-mapped word a grid barrier that gave up sets (k_small_frame: emap_device.h)
static int ensure_barrier_word(emap_ctx* ctx) {
  if (ctx->sf_host) return EMAP_OK;
  if (!ctx->frame_save) CK(hipMalloc((void**)&ctx->frame_save, sizeof(FrameDev)));
  if (!ctx->sf_poison) { CK(hipMalloc((void**)&ctx->sf_poison, 64)); CK(hipMemsetAsync(ctx->sf_poison, 0, 64, ctx->stream)); }
  volatile unsigned int* h = nullptr;
  CK(hipHostMalloc((void**)&h, 64, hipHostMallocMapped));
  h[0] = 0u; h[1] = 0u;
  if (hipHostGetDevicePointer((void**)&ctx->sf_host_dev, const_cast<unsigned int*>(h), 0) != hipSuccess) { hipHostFree((void*)h); ctx->err = "hipHostGetDevicePointer"; return EMAP_ERR_HIP; }
  ctx->sf_host = h;
  return EMAP_OK;
}

static GateArgs gate_args(emap_ctx* ctx, double position_noise, double orientation_noise) {
  const emap_params& p = ctx->prm;
  GateArgs g; memset(&g, 0, sizeof g);
  g.enable = p.enable_drift_compensation; g.min_cnt = p.min_height_drift_cnt; g.max_drift = p.max_drift; g.alpha = (float)p.drift_compensation_alpha;
  g.noise_ok = (position_noise > p.position_noise_thresh) || (orientation_noise > p.orientation_noise_thresh);
  g.use_override = ctx->use_override ? 1 : 0; g.sum_override = ctx->sum_override; g.cnt_override = ctx->cnt_override;
  g.n_points = (unsigned int)ctx->cloud.n;
  return g;
}

// The count stage.  gate_folded (frames only): k_count's last workgroup was the drift gate.
static int count_impl(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f, bool* gate_folded);
int emap_count(emap_ctx* ctx, const float R[9], const float t[3]) {
  CKARG(ctx && R && t, "null argument"); SF_CHECK(); NEED_POINTS();
  return count_impl(ctx, R, t, nullptr, nullptr);
}
static int count_impl(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f, bool* gate_folded) {
  // a cloud bucketed for this strip holds the points of its rows under ONE pose and ONE row origin: the common entry point of every
  // frame (whole, sharded or staged) checks both -- a row shift in between moves the strip's logical rows under the kept points
  if (ctx->pts_bucketed) {
    CKARG(memcmp(ctx->bucket_R, R, sizeof ctx->bucket_R) == 0 && memcmp(ctx->bucket_t, t, sizeof ctx->bucket_t) == 0, "the bound cloud was bucketed for another pose (emap_upload_points_strip)");
    CKARG(ctx->bucket_org_r == ctx->kp.org_r, "the map's rows shifted since the bound cloud was bucketed for this strip (emap_upload_points_strip): upload it again");
  }
  const bool gate_possible = !f || f->gate_possible;
  ctx->bin_rs = 1;
  CK(hipSetDevice(ctx->device));
  const bool binned = ctx->cloud.n > 0 && takes_bins(ctx, ctx->cloud.n_all);
  ctx->frame_binned = binned;
  const bool tm = ctx->stage_timing && f;
  if (binned) {
    // the ray-only sort bin exists when the parameters enable the visibility pass (a staged emap_rays call on a context without it
    // marches the cloud in its own order instead of the sorted records)
    int rc = ensure_bins(ctx, ctx->prm.enable_visibility_cleanup != 0, f); if (rc) return rc;
    const Pose pose = make_pose(ctx, R, t);
    BinStg* own = ctx->bin_strip ? reinterpret_cast<BinStg*>(ctx->bin_own) : nullptr;
    if (tm) CK(hipEventRecord(ctx->ev[ST_HIST], ctx->stream));
    // The stencil pass the frame before left pending runs in ONE grid with this frame's histogram (k_post_hist) when the workgroups of
    // both are resident together -- the launcher asks the occupancy calculator; EMAP_POST_FUSE_MAX_WG (test hook, read per frame) lowers
    // the bound.  Otherwise the pass is launched first and the frame runs the launches it always ran.
    // What the pass taken along WRITES is what this frame reads of it: traversability in the drift statistics (drift_inlier: k_tile_count,
    // which runs when gate_possible, and the inlier plane of a frame with a visibility pass), the normals in the visibility pass,
    // traversability_input nowhere; k_tile_fuse without a visibility pass copies the traversability word through untested, and the
    // semantic kernels read counts and their own planes.  The frame ends with a pass of its own, pending or launched, that rewrites every
    // output from the map as it is then, so a launch that wrote less than everything leaves the pass OWED (post_pending stays set), and a
    // frame that reads nothing launches the plain histogram and leaves it owed as well.  EMAP_POST_LEAN=0 (read per frame: A/B knob and
    // test hook): the full pass, as before.
    // Without a visibility pass the ONE reader of the pass taken along is drift_inlier in this frame's k_tile_count, and all it asks is
    // whether traversability is above traversability_inlier: POST_OUT_TRAV writes that predicate as a byte per cell into the flag plane
    // (ctx->trav_flag) and no word into the hot half, and k_tile_count is launched in the form that reads the plane -- exactly then;
    // every other launch of it (a FULL or TRAV_NORMALS pass, a settled or staged frame, emap_count) reads the word, which a full pass
    // has written by then.  The word stays stale from the lean launch to the next full pass, as traversability_input and the normals
    // already did: the invariant at post_settle covers it.  EMAP_POST_FLAGS=0 (read per frame: A/B knob and test hook): the word store.
    bool hist_done = false, flags_written = false;
    if (ctx->post_pending) {
      const bool along = f && !tm && !own && ctx->kp.mv.n == 0;
      const bool rays_on = ctx->prm.enable_visibility_cleanup != 0;
      int out = POST_OUT_FULL;
      if (along) {
        out = rays_on ? POST_OUT_TRAV_NORMALS : POST_OUT_TRAV;
        if (const char* e = getenv("EMAP_POST_LEAN")) { if (atoi(e) == 0) out = POST_OUT_FULL; }
      }
      const bool trav_only = out == POST_OUT_TRAV;
      if (along && trav_only && !gate_possible) ctx->post_took = 32;      // nothing of the pass is read: no stencil workgroup is launched
      else {
        if (trav_only) {
          if (const char* e = getenv("EMAP_POST_FLAGS")) { if (atoi(e) == 0) out = POST_OUT_TRAV_WORD; }
          if (out == POST_OUT_TRAV && !ctx->trav_flag) {      // the first lean launch of this context: every byte "the word you hold"
            unsigned char* pl = nullptr;
            CK(hipMalloc((void**)&pl, (size_t)ctx->ncells_alloc));
            if (hipMemsetAsync(pl, TRAV_FLAG_WORD, (size_t)ctx->ncells_alloc, ctx->stream) != hipSuccess) { hipFree(pl); ctx->err = "hipMemsetAsync(trav_flag)"; return EMAP_ERR_HIP; }
            ctx->trav_flag = pl;
          }
        }
        if (along) {
          long max_wg = 0;
          if (const char* e = getenv("EMAP_POST_FUSE_MAX_WG")) max_wg = atol(e);
          hist_done = launch_post_hist(ctx->stream, ctx->device, ctx->kp, ctx->prm.w1, ctx->prm.w2, ctx->prm.w3, ctx->prm.w_out, ctx->cells, ctx->trav_in, ctx->normal,
                                       ctx->ncells_alloc, ctx->prm.dilation_size, pose, ctx->bg, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->bin_hist, max_wg, out, ctx->trav_flag);
        }
        if (hist_done) {
          ++ctx->post_fused;
          flags_written = out == POST_OUT_TRAV;
          if (out == POST_OUT_FULL) ctx->post_pending = false; else ctx->post_took = 16;
          // outputs carry the current origin (post_part_impl) -- the planes that were written
          if (!trav_only) { ctx->kp.norg_r = ctx->kp.org_r; ctx->kp.norg_c = ctx->kp.org_c; }
          if (out == POST_OUT_FULL) { ctx->torg_r = ctx->kp.org_r; ctx->torg_c = ctx->kp.org_c; }
        } else if ((rc = post_settle(ctx))) return rc;
      }
    }
    if (!hist_done) launch_bin_hist(ctx->stream, ctx->kp, pose, ctx->bg, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->bin_hist, own, ctx->bin_own_cnt);
    if (tm) CK(hipEventRecord(ctx->ev[ST_SCAN], ctx->stream));
    // heavy tiles are split only when k_tile_count runs in this frame (it leaves the per-cell counts k_tile_fuse's parts need)
    static const bool split_off = getenv("EMAP_SPLIT") && atoi(getenv("EMAP_SPLIT")) == 0;      // A/B and test hook
    ctx->split.on = gate_possible && !split_off ? 1 : 0;
    {   // extra workgroups of this frame's tile kernels: what the most recent finished scan asked for, + 25 %, and never fewer than a
        // STANDING POOL (EMAP_SPLIT_POOL, default 0 = none).  A heavy tile takes as many parts as it finds room for (k_bin_scan's
        // tail), so a pool would split the heavy tiles of a scene the host has not heard of yet.  Measured with a pool of 16 (round 5,
        // same box A/B): launches with extras are the SPLIT instantiations of the tile kernels, and those cost the uniform benchmarks
        // more than the pool saves -- cfg2 70.7 -> 73.9 us per frame (k_tile_count + 1.8, k_tile_fuse + 1.4 us), cfg5 3.39 -> 4.06 ms
        // (k_tile_semantic<true> alone + 0.55 ms) -- while the first terrain frame after uniform frames only went from 0.484 to 0.468
        // ms (steady 0.309: the pool's 16 parts go to whichever heavy tiles reserve first, not to the one that holds a third of the
        // cloud).  A sensor's near field is heavy in every frame, so the lag is one frame per scene change: the pool stays off.
      static const int cap_forced = getenv("EMAP_SPLIT_CAP") ? atoi(getenv("EMAP_SPLIT_CAP")) : -1;      // test hook
      static const int pool = getenv("EMAP_SPLIT_POOL") ? atoi(getenv("EMAP_SPLIT_POOL")) : EMAP_SPLIT_POOL_DEFAULT;      // A/B knob
      const unsigned int need = *ctx->split_need;
      long cap = need ? (long)need + need / 4 + 8 : 0;
      if (ctx->split.on && cap < pool) cap = pool;
      if (cap_forced >= 0) cap = cap_forced;
      if (cap > (long)SPLIT_MAX_EXTRA) cap = SPLIT_MAX_EXTRA;
      ctx->split.cap = (int)((cap + 7) & ~7L);
    }
    // a count stage whose fuse stage never came (staged API, an error in between): its slots are still filled.  The flag is only
    // cleared by what really empties them -- this memset or a fuse stage (fuse_impl) -- never by a frame that splits nothing: such a
    // frame in between must not make the NEXT split frame add its counts on top of stale ones.
    if (ctx->split.on && ctx->split_dirty) {
      CK(hipMemsetAsync(ctx->split_mem, 0, (size_t)SPLIT_MAX_SLOTS * SPLIT_CELLS * 40 + 4 * SPLIT_MAX_SLOTS, ctx->stream));
      ctx->split_dirty = false;
    }
    ctx->split_dirty = ctx->split_dirty || (ctx->split.on != 0 && ctx->split.cap > 0);      // (slots are only used by the SPLIT instantiations: extra workgroups in the launch)
    launch_bin_scan(ctx->stream, ctx->bg, ctx->bin_hist, ctx->bin_tile_total, ctx->bin_tile_start, ctx->bin_sync, ctx->split);
    if (tm) CK(hipEventRecord(ctx->ev[ST_SCATTER], ctx->stream));
    launch_bin_scatter(ctx->stream, ctx->kp, pose, ctx->bg, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->bin_hist, ctx->bin_tile_start, ctx->bin_recs, own, ctx->bin_own_cnt,
                       ctx->cloud.chan, ctx->carry);
    if (tm) CK(hipEventRecord(ctx->ev[ST_GATE], ctx->stream));        // the "gate" stage = per-tile error sums + k_gate
    if (gate_possible) launch_tile_count(ctx->stream, ctx->kp, ctx->bg, ctx->bin_recs, ctx->bin_rs, ctx->bin_tile_start, ctx->cells, ctx->slots, ctx->split, ctx->cloud.n,
                                         flags_written ? ctx->trav_flag : nullptr);
  } else {
    { const int rc = post_settle(ctx); if (rc) return rc; }
    ctx->carry.on = 0;
    if (tm) for (int e = ST_HIST; e <= ST_SCATTER; ++e) CK(hipEventRecord(ctx->ev[e], ctx->stream));
    // whole frames (emap_update) on this path: the drift gate rides in k_count's last workgroup, one launch less in a chain of six
    static const bool fold_off = getenv("EMAP_GATE_FOLD") && atoi(getenv("EMAP_GATE_FOLD")) == 0;      // A/B and test hook
    const bool fold = f && f->fold_gate && !fold_off && ctx->cnt_sync;
    const bool folded = launch_count(ctx->stream, ctx->kp, make_pose(ctx, R, t), ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cells, ctx->acc, ctx->slots,
                                     fold ? &f->gate : nullptr, ctx->frame, ctx->cnt_sync);
    if (gate_folded) *gate_folded = folded;
    if (tm) CK(hipEventRecord(ctx->ev[ST_GATE], ctx->stream));
  }
  CK(hipGetLastError());
  return EMAP_OK;
}

static int gate_impl(emap_ctx* ctx, double position_noise, double orientation_noise, int reduce_only, double* dev_out,
                     const double* dev_totals) {
  CK(hipSetDevice(ctx->device));
  launch_gate(ctx->stream, gate_args(ctx, position_noise, orientation_noise), ctx->slots, ctx->frame, reduce_only, dev_out, dev_totals);
  CK(hipGetLastError());
  ctx->committed = false;
  return EMAP_OK;
}

int emap_set_drift_inputs(emap_ctx* ctx, double position_noise, double orientation_noise, const double* err_sum_override,
                          const uint32_t* err_cnt_override) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  ctx->use_override = err_sum_override && err_cnt_override;
  if (ctx->use_override) { ctx->sum_override = *err_sum_override; ctx->cnt_override = *err_cnt_override; }
  return gate_impl(ctx, position_noise, orientation_noise, 0, nullptr, nullptr);
}

int emap_drift_sums_to_device(emap_ctx* ctx, double* dev_out2) {
  CKARG(ctx && dev_out2, "null argument"); SF_CHECK();
  ctx->use_override = false;
  return gate_impl(ctx, 0.0, 0.0, 1, dev_out2, nullptr);
}

int emap_set_drift_inputs_device(emap_ctx* ctx, double position_noise, double orientation_noise, const double* dev_totals2) {
  CKARG(ctx && dev_totals2, "null argument"); SF_CHECK();
  ctx->use_override = false;
  return gate_impl(ctx, position_noise, orientation_noise, 0, nullptr, dev_totals2);
}

int emap_local_drift_sums(emap_ctx* ctx, double* err_sum, uint32_t* err_cnt) {
  CKARG(ctx && err_sum && err_cnt, "null argument"); SF_CHECK();
  ctx->use_override = false;
  int rc = gate_impl(ctx, 0.0, 0.0, 1, nullptr, nullptr);
  if (rc) return rc;
  emap_stats st;
  rc = emap_get_stats(ctx, &st);
  if (rc) return rc;
  *err_sum = st.err_sum; *err_cnt = st.err_cnt;
  return EMAP_OK;
}

// sem_merged (frames only): the tile kernel fused the declared semantic channels itself
static int fuse_impl(emap_ctx* ctx, const float R[9], const float t[3], bool fuse_average = false, bool rays = false, const Frame* f = nullptr,
                     bool* sem_merged = nullptr) {
  NEED_POINTS();
  CK(hipSetDevice(ctx->device));
  if (ctx->frame_binned) {
    if (fuse_average && rays && !ctx->inl_plane) {        // each buffer on its own: a failed second allocation must not leave the first one "done"
      unsigned int* pl = nullptr;
      CK(hipMalloc((void**)&pl, sizeof(unsigned int) * ctx->ncells_alloc));
      if (hipMemsetAsync(pl, 0, sizeof(unsigned int) * ctx->ncells_alloc, ctx->stream) != hipSuccess) { hipFree(pl); ctx->err = "hipMemsetAsync(inl_plane)"; return EMAP_ERR_HIP; }
      ctx->inl_plane = pl;
    }
    if (fuse_average && rays && !ctx->ray_thr)
      CK(hipMalloc((void**)&ctx->ray_thr, sizeof(float) * (size_t)((ctx->strip.row_count + 7) / 8 + 2) * ((ctx->prm.cell_n + 7) / 8)));
    if (fuse_average && rays && ((ctx->kp.org_c | ctx->prm.cell_n) & 63) != 0 && !ctx->inert_zero)     // unaligned columns: the tile kernel ORs its ballots into the logical bitmap
      CK(hipMemsetAsync(ctx->inert, 0, sizeof(unsigned long long) * ((size_t)ctx->strip.row_count * ((ctx->prm.cell_n + 63) / 64)), ctx->stream));
    if (fuse_average && rays) ctx->inert_zero = false;
    // a carrying frame fuses its semantic channels inside the tile kernel (emap_binned.hip: k_tile_fuse<.., SEM>) unless the launch
    // holds heavy-tile parts: then the stand-alone kernel follows (frame_sem_finish), reading the channels from the records all the same
    SemMini sm; memset(&sm, 0, sizeof sm);
    const bool merged = ctx->fsem_set && ctx->carry.on && bin_fuse_takes_semantics(ctx->split, fuse_average, rays, ctx->bin_rs);
    if (merged) {
      const SemSpec& S = ctx->fsem;
      sm.n_sum = S.n_sum; sm.n_col = S.n_col; sm.alpha = S.alpha; sm.sem = ctx->sem; sm.plane = ctx->ncells_alloc;
      for (int q = 0; q < S.n_sum; ++q) { sm.slot[q] = S.sum_chan[q] - ctx->carry.c0; sm.layer[q] = S.sum_layer[q]; sm.kind[q] = S.sum_kind[q]; }
      if (S.n_col) { sm.col_slot = S.col_chan[0] - ctx->carry.c0; sm.col_layer = S.col_layer[0]; }
    }
    if (sem_merged) *sem_merged = merged;
    if (ctx->fsem_set) ctx->update_path |= merged ? 4 : (ctx->carry.on ? 8 : 0);      // (emap_last_update_path)
    launch_bin_fuse(ctx->stream, ctx->kp, ctx->bg, ctx->bin_recs, ctx->bin_rs, ctx->bin_tile_start, ctx->cells, ctx->acc, ctx->frame, fuse_average, rays,
                    (merged && !ctx->fsem_keep_counts) ? nullptr : ctx->cnt_plane, ctx->inert, ctx->inl_plane, ctx->ray_thr, f ? f->ov : OverlapArgs{},
                    f ? f->gate_fold : GateFold{}, ctx->split, ctx->cloud.n, merged ? &sm : nullptr);
    if (ctx->split.on) ctx->split_dirty = false;        // k_tile_fuse's parts cleared their slots (a frame that splits nothing leaves an older count stage's slots as they are)
    if (fuse_average) ctx->kp.mv.n = 0;   // every owned cell rewritten: pending map shifts are in memory now
    CK(hipGetLastError());
    return EMAP_OK;
  }
  launch_fuse(ctx->stream, ctx->kp, make_pose(ctx, R, t), ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cells, ctx->acc, ctx->frame);
  CK(hipGetLastError());
  return EMAP_OK;
}
int emap_fuse(emap_ctx* ctx, const float R[9], const float t[3]) { CKARG(ctx && R && t, "null argument"); SF_CHECK(); return fuse_impl(ctx, R, t); }

// fuse + commit + average_map in one call for frames without a visibility pass (one tile kernel on the binned path)
int emap_fuse_average(emap_ctx* ctx, const float R[9], const float t[3]) {
  CKARG(ctx && R && t, "null argument"); SF_CHECK();
  const bool fused = ctx->frame_binned;
  int rc = fuse_impl(ctx, R, t, fused);
  if (rc) return rc;
  if (!fused) { launch_average(ctx->stream, ctx->kp, ctx->cells, ctx->acc, ctx->accr, ctx->frame, ctx->committed, false, ctx->cnt_plane, OverlapArgs{}); ctx->kp.mv.n = 0; }
  ctx->committed = false;
  CK(hipGetLastError());
  return EMAP_OK;
}

int emap_commit(emap_ctx* ctx) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  if (!ctx->committed) {
    launch_commit(ctx->stream, ctx->kp, ctx->cells, ctx->acc, ctx->frame, ctx->inert);
    ctx->committed = true; ctx->inert_zero = false;
    ctx->kp.mv.n = 0;                 // k_commit rewrote every owned cell: pending map shifts are in memory now
  }
  CK(hipGetLastError());
  return EMAP_OK;
}

static int rays_impl(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f);
int emap_rays(emap_ctx* ctx, const float R[9], const float t[3]) {
  CKARG(ctx && R && t, "null argument"); SF_CHECK(); NEED_POINTS();
  return rays_impl(ctx, R, t, nullptr);
}
static int rays_impl(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f) {
  CK(hipSetDevice(ctx->device));
  const bool fused = f && f->rays_fused, nlag = f && f->nlag;
  CKARG(ctx->committed || fused, "emap_rays needs emap_commit first (rays read snapshot S1)");
  CKARG(!ctx->pts_bucketed, "a bucketed cloud (emap_upload_points_strip) cannot march its rays by row: every valid point marches a ray through every strip");
  // newmap[3]: the tile kernel's dense plane, or the high halves of AccF::pts_inl (5 x u64 records) on the staged / atomic path
  const unsigned int* inl = fused ? ctx->inl_plane : reinterpret_cast<const unsigned int*>(ctx->acc) + 1;
  const bool sorted = ctx->frame_binned && ctx->bg.raybin;      // the sorted records hold EVERY valid point only with the ray-only bin
  char* const ab = reinterpret_cast<char*>(ctx->accr);
  const AccRView av = {ab + offsetof(AccR, dec), ab + offsetof(AccR, hits), ab + offsetof(AccR, upper_key), (int)sizeof(AccR), (int)sizeof(AccR), (int)sizeof(AccR), 0};
  KP kr = ctx->kp;
  kr.nlag = nlag ? 1 : 0;                                // sharded frame after a row shift: the row-aligned copy of the normal planes (normal_exchange)
  kr.ray_pref = ctx->split_need ? (int)ctx->split_need[1] : 0;      // (host-mapped word written by k_ray_apply: FrameDev::ray_class)
  launch_rays(ctx->stream, kr, make_pose(ctx, R, t), ctx->rt, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cells, av,
              nlag ? ctx->nlag_buf : ctx->normal, nlag ? (long)ctx->strip.row_count * ctx->prm.cell_n : ctx->ncells_alloc,
              ctx->frame, ctx->want_ray_stats, ctx->inert, inl, fused ? 1 : (int)(sizeof(AccF) / 4),
              fused ? ctx->ray_thr : nullptr,
              sorted ? reinterpret_cast<const unsigned int*>(ctx->bin_recs) : nullptr,        // march in tile-sorted order
              sorted ? ctx->bin_tile_start + ctx->bg.TB : nullptr);
  CK(hipGetLastError());
  return EMAP_OK;
}

int emap_average(emap_ctx* ctx) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  launch_average(ctx->stream, ctx->kp, ctx->cells, ctx->acc, ctx->accr, ctx->frame, ctx->committed, true, ctx->cnt_plane, OverlapArgs{});
  ctx->committed = false; ctx->kp.mv.n = 0;       // (uncommitted: k_average wrote the pending map shifts out itself)
  CK(hipGetLastError());
  return EMAP_OK;
}

static OverlapArgs overlap_args(const emap_ctx* ctx, float t_z, bool on) {
  const emap_params& p = ctx->prm;
  int cell_range = (int)(p.overlap_clear_range_xy / p.resolution);     // elevation_mapping.py:88-91
  if (cell_range < 0) cell_range = 0; if (cell_range > p.cell_n) cell_range = p.cell_n;
  OverlapArgs o; memset(&o, 0, sizeof o);
  o.on = on ? 1 : 0;
  o.cmin = p.cell_n / 2 - cell_range / 2; o.cmax = p.cell_n / 2 + cell_range / 2;
  o.hmin = t_z - (float)p.overlap_clear_range_z; o.hmax = t_z + (float)p.overlap_clear_range_z;
  return o;
}

int emap_overlap_clear(emap_ctx* ctx, float t_z) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const OverlapArgs o = overlap_args(ctx, t_z, true);
  launch_overlap(ctx->stream, ctx->kp, ctx->cells, o.cmin, o.cmax, o.hmin, o.hmax);
  CK(hipGetLastError());
  return EMAP_OK;
}

// Stencil stages.  The kernels work on LOGICAL rows; a strip owns the physical rows [row_begin, row_begin + row_count), i.e. the
// logical rows ls + j (mod cell_n), j = 0 .. row_count-1, with ls = (row_begin - org_r) mod cell_n: one or two logical intervals.
static void post_rows(emap_ctx* ctx, int nj, const int* j0, const int* j1, int stage, int tile_rows = 0) {      // outputs for the strip's rows j0[k] <= j < j1[k]
  const int C = ctx->prm.cell_n;
  const int ls = ((ctx->strip.row_begin - ctx->kp.org_r) % C + C) % C;
  int sb[4], se[4], n = 0;
  if (ctx->strip.row_count == C && nj == 1 && j0[0] == 0 && j1[0] == C) {      // the whole map: one interval, tiles aligned to logical row 0
    sb[0] = 0; se[0] = C; n = 1; nj = 0;
  }
  for (int k = 0; k < nj; ++k) {
    if (j1[k] <= j0[k]) continue;
    const int b = ls + j0[k], e = ls + j1[k];                             // unwrapped logical rows
    if (e <= C) { sb[n] = b; se[n] = e; n++; }
    else if (b >= C) { sb[n] = b - C; se[n] = e - C; n++; }
    else { sb[n] = b; se[n] = C; n++; sb[n] = 0; se[n] = e - C; n++; }    // the circular seam lies inside: never inside one tile
  }
  launch_post(ctx->stream, ctx->kp, ctx->prm.w1, ctx->prm.w2, ctx->prm.w3, ctx->prm.w_out, ctx->cells, ctx->trav_in, ctx->normal,
              ctx->ncells_alloc, ctx->prm.dilation_size, n, sb, se, stage, tile_rows);
}

int emap_dilate(emap_ctx* ctx) {          // dilation_filter_kernel alone: traversability_input (k_post, stage 1)
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FLUSH();
  { const int j0 = 0, j1 = ctx->strip.row_count; post_rows(ctx, 1, &j0, &j1, 1); }
  ctx->torg_r = ctx->kp.org_r; ctx->torg_c = ctx->kp.org_c;
  CK(hipGetLastError());
  return EMAP_OK;
}

int emap_traversability_normals(emap_ctx* ctx) { CKARG(ctx, "null ctx"); SF_CHECK(); return emap_post_part(ctx, 0); }     // (recomputes the dilation it consumes: same values)

// dilation + traversability + normals in one launch.  part: 0 = whole strip,
// 1 = only the rows that do not depend on halo rows (can run while the halo exchange is in flight),
// 2 = the remaining (boundary) rows.
static int post_part_impl(emap_ctx* ctx, int32_t part);
int emap_post_part(emap_ctx* ctx, int32_t part) { CKARG(ctx && part >= 0 && part <= 2, "bad argument"); SF_CHECK(); return post_part_impl(ctx, part); }
static int post_part_impl(emap_ctx* ctx, int32_t part) {      // (inside a frame: no SF_CHECK -- a small frame just issued must not be waited for)
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const int n = ctx->strip.row_count;
  const int reach = ctx->prm.dilation_size + 4;                  // rows a stencil looks beyond its own (dilation + filter + row wrap)
  const int lo = reach < n ? reach : n, hi = n - reach > lo ? n - reach : lo;      // interior rows [lo, hi)
  const int jb0[2] = {0, hi}, je0[2] = {lo, n}, z = 0;
  if (part == 0) post_rows(ctx, 1, &z, &n, 0);
  else if (part == 1) post_rows(ctx, 1, &lo, &hi, 0);
  else { int tr = 4; while (tr < reach && tr < 32) tr *= 2;      // the boundary bands are `reach` rows high: tiles of that height, not the strip's 32-row tiles
         post_rows(ctx, 2, jb0, je0, 0, tr); }          // at most 3 logical intervals: the seam lies in one of the two boundary bands
  if (part != 1) { ctx->kp.norg_r = ctx->torg_r = ctx->kp.org_r; ctx->kp.norg_c = ctx->torg_c = ctx->kp.org_c; }   // outputs carry the current origin
  CK(hipGetLastError());
  return EMAP_OK;
}
int emap_post(emap_ctx* ctx) { CKARG(ctx, "null ctx"); SF_CHECK(); return emap_post_part(ctx, 0); }

int emap_update_variance(emap_ctx* ctx) { CKARG(ctx, "null ctx"); SF_CHECK(); CK(hipSetDevice(ctx->device)); launch_var_time(ctx->stream, ctx->kp, ctx->cells, 1, 0); ctx->kp.mv.n = 0; CK(hipGetLastError()); return EMAP_OK; }
int emap_update_time(emap_ctx* ctx) { CKARG(ctx, "null ctx"); SF_CHECK(); CK(hipSetDevice(ctx->device)); launch_var_time(ctx->stream, ctx->kp, ctx->cells, 0, 1); ctx->kp.mv.n = 0; CK(hipGetLastError()); return EMAP_OK; }

int emap_get_stats(emap_ctx* ctx, emap_stats* out) {
  CKARG(ctx && out, "null argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  FrameDev f;
  CK(hipMemcpyAsync(&f, ctx->frame, sizeof f, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  out->err_sum = (double)f.err_sum_fix / EM_SCALE_E; out->err_cnt = (uint32_t)f.err_cnt; out->gate_fired = f.gate_fired;
  out->mean_error = f.mean_error; out->additive_mean_error = f.additive_mean_error; out->shift = f.shift;
  out->n_points = f.n_points; out->ray_visits = f.ray_visits;
  return EMAP_OK;
}

// ---- state access -------------------------------------------------------------------------------------------
// Views are (row_count, cell_n) host arrays in LOGICAL order (k_plane_view / k_get_plane): row j = logical row j of a full map,
// or the j-th logical row of a strip (emap_strip_logical_begin), columns logical.
static int plane_view(emap_ctx* ctx, int plane, float* host, bool to_device) { SF_CHECK();
  const size_t bytes = sizeof(float) * (size_t)ctx->strip.row_count * ctx->prm.cell_n;
  FLUSH();
  if (to_device) CK(hipMemcpyAsync(ctx->scratch, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (plane < 7) {
    if (to_device) launch_set_plane(ctx->stream, ctx->kp, ctx->cells, plane, ctx->scratch);
    else launch_get_plane(ctx->stream, ctx->kp, ctx->cells, plane, ctx->scratch);
  } else if (plane == EMAP_PLANE_TRAV_INPUT) launch_plane_view(ctx->stream, ctx->kp, ctx->torg_r, ctx->torg_c, ctx->trav_in, ctx->scratch, to_device);
  else launch_plane_view(ctx->stream, ctx->kp, ctx->kp.norg_r, ctx->kp.norg_c, ctx->normal + (long)(plane - EMAP_PLANE_NORMAL_X) * ctx->ncells_alloc,
                         ctx->scratch, to_device);
  CK(hipGetLastError());
  if (!to_device) CK(hipMemcpyAsync(host, ctx->scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

int emap_get_layer(emap_ctx* ctx, int plane, float* host_out) {
  CKARG(ctx && host_out && plane >= 0 && plane < EMAP_PLANE_COUNT, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  return plane_view(ctx, plane, host_out, false);
}

int emap_publish_layer(emap_ctx* ctx, int32_t kind, float center_z, int32_t use_only_above_for_upper_bound, float* host_out) {
  CKARG(ctx && host_out && kind >= 0 && kind <= 8, "bad argument"); SF_CHECK();
  CKARG(ctx->strip.halo_rows == 0 && ctx->strip.row_count == ctx->prm.cell_n, "emap_publish_layer: single-strip contexts only");
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const long M = ctx->prm.cell_n - 2;
  launch_publish(ctx->stream, ctx->kp, ctx->cells, ctx->normal, ctx->ncells_alloc, kind, center_z, use_only_above_for_upper_bound, ctx->scratch);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(host_out, ctx->scratch, sizeof(float) * (size_t)(M * M), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

int emap_set_layer(emap_ctx* ctx, int plane, const float* host_in) {
  CKARG(ctx && host_in && plane >= 0 && plane < EMAP_PLANE_COUNT, "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  return plane_view(ctx, plane, const_cast<float*>(host_in), true);
}

int emap_strip_logical_begin(emap_ctx* ctx, int32_t* logical_row) {
  CKARG(ctx && logical_row, "null argument"); SF_CHECK();
  const int C = ctx->prm.cell_n;
  *logical_row = ctx->strip.row_count == C ? 0 : ((ctx->strip.row_begin - ctx->kp.org_r) % C + C) % C;
  return EMAP_OK;
}

// ElevationMap.shift_map_xy / shift_map_z (EM/elevation_mapping.py:200-226) WITHOUT moving data: the roll becomes a rotation of the
// circular origin, the reset of the entering band and the z offset become a pending entry that the frame kernels replay (cell_now)
// and the next full rewrite of the cells writes out; only the semantic layers clear their entering band here (O(border) bytes).
// The normal planes and traversability_input keep their own origin: the reference does not shift them.
int emap_shift(emap_ctx* ctx, int32_t shift_rows, int32_t shift_cols, float dz) {
  CKARG(ctx, "null ctx"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const int C = ctx->prm.cell_n;
  CKARG(shift_rows > -(1 << 20) && shift_rows < (1 << 20) && shift_cols > -(1 << 20) && shift_cols < (1 << 20), "absurd shift");   // (a shift of cell_n or more resets every cell: the replay predicate covers it)
  if (shift_rows == 0 && shift_cols == 0 && dz == 0.f) return EMAP_OK;
  ctx->pseg_labels = nullptr;                                  // (as emap_clear)
  if (ctx->kp.mv.n == EM_MAX_MOVES) FLUSH();       // more moves than the replay list holds before the next frame: one full pass
  KP& k = ctx->kp;
  k.org_r = ((k.org_r - shift_rows) % C + C) % C;   // roll: new logical r holds old logical r - shift  =>  physical = r - shift + org
  k.org_c = ((k.org_c - shift_cols) % C + C) % C;
  Moves& mv = k.mv;
  mv.org_r[mv.n] = k.org_r; mv.org_c[mv.n] = k.org_c; mv.sr[mv.n] = shift_rows; mv.sc[mv.n] = shift_cols; mv.dz[mv.n] = dz;
  mv.n++;
  if (ctx->sem_layers > 0 && (shift_rows != 0 || shift_cols != 0)) {   // SemanticMap.shift_map_xy (semantic_map.py:127-136): roll + zero pad
    launch_band_clear(ctx->stream, k, ctx->sem, ctx->sem_layers, ctx->ncells_alloc, shift_rows, shift_cols);
    if (ctx->sem_alpha) launch_band_clear(ctx->stream, k, ctx->sem_alpha, ctx->sem_layers, ctx->ncells_alloc, shift_rows, shift_cols);   // new_map too (:135-136)
    CK(hipGetLastError());
  }
  return EMAP_OK;
}

// ---- one frame -----------------------------------------------------------------------------------------------------------
// emap_update runs a whole map (or a strip on its own), emap_update_sharded a row strip of a map shared through the communicator: the
// stage order of ShardedElevationMap.update (sharded.py) with both exchange steps issued from here -- no Python, no host
// synchronisation between the stages.  The two differ only in whether the frame may take the small-frame path, how the drift gate
// gets its totals, how the rays march and how the stencils run.  sf_recover re-runs aborted small frames through frame_impl too.
static int run_frame(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats, bool sharded) {
  const int rc = frame_impl(ctx, R, t, position_noise, orientation_noise, stats, sharded);
  if (ctx) ctx->fsem_set = false;      // the declared semantic fusion belongs to ONE frame, whatever became of it
  return rc;
}
int emap_update(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats) {
  return run_frame(ctx, R, t, position_noise, orientation_noise, stats, false);
}
int emap_update_sharded(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats) {
  if (ctx && ctx->post_pending) { const int rc = post_settle(ctx); if (rc) return rc; }      // (a sharded frame never takes a pending pass along)
  return run_frame(ctx, R, t, position_noise, orientation_noise, stats, true);
}
static int frame_impl(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats, bool sharded) {
  CKARG(ctx && R && t, "null argument"); NEED_POINTS();
  CKARG(!sharded || (ctx->rccl && ctx->comm), "emap_comm_init has not been called");
  CK(hipSetDevice(ctx->device));
  const emap_params& p = ctx->prm;
  const bool tm = ctx->stage_timing, rays_on = p.enable_visibility_cleanup != 0;
  int rc;
#define STAGE(i) do { if (tm) CK(hipEventRecord(ctx->ev[i], ctx->stream)); } while (0)
  // robot scale (small clouds on small maps: the atomic path): count, gate, fuse and commit / average in ONE launch
  // (not with a visibility pass or a declared semantic fusion behind it: an ABORTED launch must leave nothing for the rest of the frame to
  // act on -- the stencil launch that follows is a pure function of the map -- until sf_recover has re-run the frame)
  static const bool sf_env_off = getenv("EMAP_SMALL_FRAME") && atoi(getenv("EMAP_SMALL_FRAME")) == 0;      // A/B and test hook
  const int sf_grid = (!sharded && !sf_env_off && !ctx->sf_redo && !takes_bins(ctx, ctx->cloud.n_all) && ctx->cnt_sync && !ctx->pts_bucketed && !rays_on && !ctx->fsem_set)
                      ? small_frame_grid(ctx->kp, ctx->cloud.n) : 0;
  if (sf_grid == 0) SF_SETTLE_FRAMES();         // (a frame on any other path: the small frames in flight are settled first)
  // The stencil pass of the frame before may be pending (below).  A binned whole-map frame takes it into its histogram launch
  // (count_impl); every other frame -- a small-frame launch, the atomic path, a sharded or timed frame -- launches it first.
  if (ctx->post_pending && !(!sharded && sf_grid == 0 && !tm && ctx->cloud.n > 0 && takes_bins(ctx, ctx->cloud.n_all)) && (rc = post_settle(ctx))) return rc;
  ctx->post_took = 0;
  Frame fr; memset(&fr, 0, sizeof fr);
  if ((rc = frame_sem_begin(ctx, rays_on, &fr))) return rc;
  fr.gate_possible = p.enable_drift_compensation && (position_noise > p.position_noise_thresh || orientation_noise > p.orientation_noise_thresh);
  fr.fold_gate = !sharded;
  ctx->use_override = false;
  fr.gate = gate_args(ctx, position_noise, orientation_noise);
  // clear_overlap_map rides on the kernel that rewrites the cells last (tile kernel / k_average, or k_ray_apply after a visibility pass)
  fr.ov = overlap_args(ctx, t[2], p.enable_overlap_clearance != 0);
  if (sharded) {
    fr.by_ray = rays_by_ray(ctx);             // (before the sort: a by-ray frame sorts only the points of the strip's rows)
    ctx->wire_bytes = 0;
    if (ctx->pts_bucketed) {                  // emap_upload_points_strip: the cloud only holds the points of this strip's rows, for ONE pose
      CKARG(memcmp(ctx->bucket_R, R, sizeof ctx->bucket_R) == 0 && memcmp(ctx->bucket_t, t, sizeof ctx->bucket_t) == 0, "the bound cloud was bucketed for another pose (emap_upload_points_strip)");
      CKARG(!rays_on || fr.by_ray, "a bucketed cloud cannot feed a visibility pass that marches BY ROW (every valid point marches a ray through every strip): upload the whole cloud, or march by ray (emap_set_ray_mode)");
    }
  }
  bool fused_small = false;
  if (sf_grid > 0) {
    if ((rc = ensure_barrier_word(ctx))) return rc;
    sf_forget_applied(ctx);
    if (ctx->sf_count == emap_ctx::SF_RING || ctx->sf_epoch >= 0x7ffffff0u) {      // no room to remember another frame (or the epochs wrap): settle the ones in flight
      if ((rc = sf_settle(ctx))) return rc;
      if (ctx->sf_epoch >= 0x7ffffff0u) { CK(hipStreamSynchronize(ctx->stream)); ctx->sf_epoch = 0u; ctx->sf_host[0] = 0u; }
    }
    for (int e = ST_HIST; e <= ST_SCATTER; ++e) STAGE(e);
    ctx->frame_binned = false;
    ++ctx->sf_epoch;
    {   // what the launch stands for, should a barrier be aborted (sf_recover)
      emap_ctx::SfFrame& f = ctx->sf_ring[(ctx->sf_head + ctx->sf_count) % emap_ctx::SF_RING];
      f.epoch = ctx->sf_epoch; memcpy(f.R, R, sizeof f.R); memcpy(f.t, t, sizeof f.t); f.pn = position_noise; f.on = orientation_noise; f.mv = ctx->kp.mv;
      f.cloud = ctx->cloud;
      ++ctx->sf_count;
    }
    unsigned int spin = SF_SPIN_DEFAULT; int test_abort = 0;      // test hooks (read per frame: a test toggles them)
    if (const char* e = getenv("EMAP_SF_SPIN_LIMIT")) { const long v = atol(e); if (v >= 1 && v <= (1L << 24)) spin = (unsigned int)v; }
    if (const char* e = getenv("EMAP_SF_TEST_ABORT")) test_abort = atoi(e);
    launch_small_frame(ctx->stream, sf_grid, ctx->kp, make_pose(ctx, R, t), ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, ctx->cells, ctx->acc,
                       ctx->cnt_plane, fr.ov, fr.gate, ctx->frame, ctx->frame_save, ctx->slots,
                       ctx->cnt_sync, ctx->cnt_sync + 2048, ctx->sf_host_dev, ctx->sf_poison, ctx->sf_epoch, spin, test_abort);
    CK(hipGetLastError());
    fused_small = true;
    STAGE(ST_GATE);
  } else {
    bool gate_folded = false;
    if ((rc = count_impl(ctx, R, t, &fr, &gate_folded))) return rc;     // records ST_HIST .. ST_GATE itself: "gate" starts with the per-tile error sums
    CKARG(!fr.by_ray || ctx->frame_binned, "rays by ray: this rank could not take the tile-binned path the other ranks take");
    if (gate_folded) ctx->committed = false;                              // (small clouds: k_count's last workgroup was the gate)
    else if (!sharded) { if ((rc = gate_impl(ctx, position_noise, orientation_noise, 0, nullptr, nullptr))) return rc; }
    else {                                    // local sums + all-reduce + gate
      if ((rc = gate_impl(ctx, 0.0, 0.0, 1, ctx->comm_sums, nullptr))) return rc;                                     // local sums -> device
      if ((rc = drift_allreduce(ctx))) return rc;                                                                       // exchange step 1
      if (ctx->frame_binned) {                // the decision on the all-reduced totals rides in the head of the tile kernel
        fr.gate_fold.mode = 1; fr.gate_fold.dev_totals = ctx->comm_sums + 2; fr.gate_fold.A = fr.gate;
        ctx->committed = false;
      } else if ((rc = gate_impl(ctx, position_noise, orientation_noise, 0, nullptr, ctx->comm_sums + 2))) return rc;
    }
  }
  ctx->update_path = fused_small ? 2 : (ctx->frame_binned ? 1 : 0);
  ctx->update_path |= ctx->post_took;      // 16: the pending pass was taken along lean, 32: left owed without a launch (count_impl)
  STAGE(ST_FUSE);
  // binned scatter: fusion, commit and averaging happen in ONE tile kernel; with the visibility pass it also writes the inert
  // bitmap and the inlier plane, and the ray effects are applied by k_ray_apply ("average" stage) afterwards
  const bool fused_avg = ctx->frame_binned;
  bool sem_merged = false;
  if (!fused_small && (rc = fuse_impl(ctx, R, t, fused_avg, rays_on, &fr, &sem_merged))) return rc;
  STAGE(ST_COMMIT);
  fr.rays_fused = fused_avg && rays_on;
  if (rays_on) {
    if (!fused_avg && (rc = emap_commit(ctx))) return rc;
    STAGE(ST_RAYS);
    if (sharded && ctx->comm_world > 1 && normal_row_lag(ctx) != 0) {
      if ((rc = normal_exchange(ctx))) return rc;
      fr.nlag = true;
    }
    if ((rc = fr.by_ray ? rays_by_ray_pass(ctx, R, t, &fr) : rays_impl(ctx, R, t, &fr))) return rc;
  } else STAGE(ST_RAYS);
  STAGE(ST_AVERAGE);
  if (fused_small) ctx->kp.mv.n = 0;                        // (k_small_frame committed and averaged: every cell rewritten)
  else if (!fused_avg) { launch_average(ctx->stream, ctx->kp, ctx->cells, ctx->acc, ctx->accr, ctx->frame, ctx->committed, rays_on, ctx->cnt_plane, fr.ov); ctx->kp.mv.n = 0; }
  else if (rays_on) { launch_ray_apply(ctx->stream, ctx->kp, ctx->cells, ctx->accr, ctx->inert, fr.ov, ctx->frame, ctx->split.need_host ? ctx->split.need_host + 1 : nullptr, ctx->ray_par ^= 1); ctx->inert_zero = true; }
  ctx->committed = false;
  CK(hipGetLastError());
  if ((rc = frame_sem_finish(ctx, R, t, sem_merged))) return rc;      // semantic_map.update_layers_pointcloud (elevation_mapping.py:368) -- unless the tile kernel fused the channels itself
  STAGE(ST_OVERLAP);                          // (empty: clear_overlap_map rode on the kernel that rewrote the cells last, fr.ov)
  STAGE(ST_POST);                             // "post" = halo exchange + stencils
  if (sharded && ctx->comm_world > 1) {
    if ((rc = halo_exchange_start(ctx))) return rc;                                                 // exchange step 2 ...
    if ((rc = post_part_impl(ctx, 1))) return rc;                                                   // ... overlapped with the interior tiles
    CK(hipStreamWaitEvent(ctx->stream, ctx->ev_done, 0));
    if ((rc = post_part_impl(ctx, 2))) return rc;
  } else {
    // A whole-map frame on the binned path whose stencil launch is the plain k_post with 16- or 32-row tiles leaves the pass PENDING: the
    // next such frame runs it beside its own histogram (count_impl, k_post_hist), anything else that enters the library launches it
    // first (SF_CHECK).  EMAP_POST_DEFER=0 (read per frame: a test toggles it) launches it here, as every other frame does.
    bool defer = !sharded && ctx->frame_binned && !tm && ctx->kp.mv.n == 0 && ctx->strip.row_count == p.cell_n && ctx->strip.halo_rows == 0 &&
                 post_hist_tile_rows(ctx->kp, p.dilation_size) != 0;
    if (defer) { if (const char* e = getenv("EMAP_POST_DEFER")) defer = atoi(e) != 0; }
    if (defer) ctx->post_pending = true;
    else { if ((rc = post_part_impl(ctx, 0))) return rc; ctx->post_pending = false; }      // (a full pass: whatever a lean launch left owed is paid)
  }
  STAGE(ST_N);
#undef STAGE
  if (tm) {
    CK(hipEventSynchronize(ctx->ev[ST_N]));
    for (int i = 0; i < ST_N; ++i) CK(hipEventElapsedTime(&ctx->stage_ms[i], ctx->ev[i], ctx->ev[i + 1]));
  }
  if (stats) return emap_get_stats(ctx, stats);
  return EMAP_OK;
}

// ---- timing -----------------------------------------------------------------------------------------------------
int emap_timer_begin(emap_ctx* ctx) { CKARG(ctx, "null ctx"); CK(hipSetDevice(ctx->device)); CK(hipEventRecord(ctx->t0, ctx->stream)); return EMAP_OK; }
int emap_timer_end(emap_ctx* ctx, float* ms) {
  CKARG(ctx && ms, "null argument"); SF_CHECK();      // (the interval ends behind the complete last frame)
  CK(hipSetDevice(ctx->device));
  CK(hipEventRecord(ctx->t1, ctx->stream)); CK(hipEventSynchronize(ctx->t1)); CK(hipEventElapsedTime(ms, ctx->t0, ctx->t1));
  return EMAP_OK;
}
int emap_enable_stage_timing(emap_ctx* ctx, int enable) { CKARG(ctx, "null ctx"); ctx->stage_timing = enable != 0; ctx->want_ray_stats = enable > 1; return EMAP_OK; }
int emap_small_frame_aborts(emap_ctx* ctx, uint32_t* frames) { CKARG(ctx && frames, "null argument"); SF_CHECK(); *frames = ctx->sf_aborts; return EMAP_OK; }
int emap_post_fused_launches(emap_ctx* ctx, uint32_t* launches) { CKARG(ctx && launches, "null argument"); SF_CHECK(); *launches = ctx->post_fused; return EMAP_OK; }
int emap_last_update_path(emap_ctx* ctx, int32_t* path) { CKARG(ctx && path, "null argument"); *path = ctx->update_path; return EMAP_OK; }
int emap_get_stage_times(emap_ctx* ctx, float ms_out[10]) { CKARG(ctx && ms_out, "null argument"); for (int i = 0; i < ST_N; ++i) ms_out[i] = ctx->stage_ms[i]; return EMAP_OK; }

}  // extern "C"
