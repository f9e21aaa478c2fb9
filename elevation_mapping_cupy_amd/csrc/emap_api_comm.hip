// C ABI of the MI355X elevation-map fusion core, host side of the row-strip multi-GPU path: the halo pack / unpack entry points, the
// RCCL communicator (resolved at run time), the exchange of the un-shifted normal planes and the visibility pass by ray.  The only
// file that sees rccl.h: the others reach the collectives of a frame through the helpers of emap_host.h.
#include "emap_host.h"
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library itself is dlopen()ed by emap_comm_init
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace emap_host;

// the ten RCCL entry points of the path, bound with dlsym (no link-time dependency: the .so loads on machines without RCCL)
struct RcclApi {
  void* handle;
  decltype(&ncclGetUniqueId) GetUniqueId; decltype(&ncclCommInitRank) CommInitRank; decltype(&ncclCommDestroy) CommDestroy;
  decltype(&ncclAllReduce) AllReduce; decltype(&ncclSend) Send; decltype(&ncclRecv) Recv;
  decltype(&ncclGroupStart) GroupStart; decltype(&ncclGroupEnd) GroupEnd; decltype(&ncclGetErrorString) GetErrorString;
  decltype(&ncclCommCount) CommCount;
};

extern "C" {

// ---- halos ----------------------------------------------------------------------------------------------------
int emap_halo_bytes(emap_ctx* ctx, int64_t* bytes_per_side) {
  CKARG(ctx && bytes_per_side, "null argument"); SF_CHECK();
  *bytes_per_side = (int64_t)ctx->strip.halo_rows * ctx->prm.cell_n * (int64_t)sizeof(float4);      // the cold half-cell plane only (see halo_exchange_start)
  return EMAP_OK;
}
int emap_halo_pack(emap_ctx* ctx, int side, float* dev_buf) {
  CKARG(ctx && dev_buf && (side == 0 || side == 1), "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long H = ctx->strip.halo_rows, C = ctx->prm.cell_n, n = ctx->strip.row_count;
  if (H == 0) return EMAP_OK;
  CKARG(n >= H, "strip thinner than its halo");
  const long off = side == 0 ? H * C : (H + n - H) * C;                   // first / last H owned rows of the COLD half-cell plane
  CK(hipMemcpyAsync(dev_buf, ctx->cells.cold + off, sizeof(float4) * H * C, hipMemcpyDeviceToDevice, ctx->stream));
  return EMAP_OK;
}
int emap_halo_unpack(emap_ctx* ctx, int side, const float* dev_buf) {
  CKARG(ctx && dev_buf && (side == 0 || side == 1), "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long H = ctx->strip.halo_rows, C = ctx->prm.cell_n, n = ctx->strip.row_count;
  if (H == 0) return EMAP_OK;
  const long off = side == 0 ? 0 : (H + n) * C;
  CK(hipMemcpyAsync(ctx->cells.cold + off, dev_buf, sizeof(float4) * H * C, hipMemcpyDeviceToDevice, ctx->stream));
  return EMAP_OK;
}

// boundary rows of the three normal planes (3 x halo_rows x cell_n floats per side) for the exchange after a row shift
// (see normal_exchange); emap_normal_row_lag tells the caller whether it is due
int emap_normal_row_lag(emap_ctx* ctx, int32_t* lag) { CKARG(ctx && lag, "null argument"); SF_CHECK(); *lag = normal_row_lag(ctx); return EMAP_OK; }
int emap_normal_halo_pack(emap_ctx* ctx, int side, float* dev_buf) {
  CKARG(ctx && dev_buf && (side == 0 || side == 1), "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long H = ctx->strip.halo_rows, C = ctx->prm.cell_n, n = ctx->strip.row_count;
  if (H == 0) return EMAP_OK;
  for (int k = 0; k < 3; ++k)
    CK(hipMemcpyAsync(dev_buf + (size_t)k * H * C, ctx->normal + (size_t)k * ctx->ncells_alloc + (side == 0 ? H * C : n * C), sizeof(float) * H * C,
                      hipMemcpyDeviceToDevice, ctx->stream));
  return EMAP_OK;
}
int emap_normal_halo_unpack(emap_ctx* ctx, int side, const float* dev_buf) {
  CKARG(ctx && dev_buf && (side == 0 || side == 1), "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const long H = ctx->strip.halo_rows, C = ctx->prm.cell_n, n = ctx->strip.row_count;
  if (H == 0) return EMAP_OK;
  for (int k = 0; k < 3; ++k)
    CK(hipMemcpyAsync(ctx->normal + (size_t)k * ctx->ncells_alloc + (side == 0 ? 0 : (H + n) * C), dev_buf + (size_t)k * H * C, sizeof(float) * H * C,
                      hipMemcpyDeviceToDevice, ctx->stream));
  return EMAP_OK;
}

// ---- multi-GPU: row strips, one process per GPU, RCCL over xGMI ---------------------------------------------------
// The two exchange steps of the path: an all-reduce of the drift sums (2 x f64) between the count and fuse
// stages, and the neighbour exchange of halo rows before the stencils.  Halo rows are contiguous in the cold half-cell plane (the
// only one the stencils read), so RCCL sends the first / last owned rows and receives into the halo rows IN PLACE (no pack / unpack copies); the
// exchange runs on its own stream while the stencil tiles that do not depend on halo rows run on the main stream.
static RcclApi* rccl_open(const char* path, std::string* why) {
  void* h = dlopen(path && *path ? path : "librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) { *why = std::string("dlopen: ") + dlerror(); return nullptr; }
  RcclApi* a = new RcclApi(); a->handle = h;
  bool ok = true;
#define SYM(field, name) do { a->field = (decltype(a->field))dlsym(h, name); if (!a->field) { ok = false; *why = std::string("missing symbol ") + name; } } while (0)
  SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
  SYM(AllReduce, "ncclAllReduce"); SYM(Send, "ncclSend"); SYM(Recv, "ncclRecv"); SYM(GroupStart, "ncclGroupStart");
  SYM(GroupEnd, "ncclGroupEnd"); SYM(GetErrorString, "ncclGetErrorString"); SYM(CommCount, "ncclCommCount");
#undef SYM
  if (!ok) { delete a; return nullptr; }   // the handle stays open: unloading a GPU runtime library is not safe
  return a;
}
#define CKN(call)                                                                                                       \
  do { ncclResult_t r_ = (call);                                                                                        \
       if (r_ != ncclSuccess) { ctx->err = std::string(#call) + ": " + ctx->rccl->GetErrorString(r_); return EMAP_ERR_COMM; } } while (0)
// the same between ncclGroupStart and ncclGroupEnd: a failure closes the group before it returns (the next call must not land in it)
#define CKG(call)                                                                                                       \
  do { ncclResult_t r_ = (call);                                                                                        \
       if (r_ != ncclSuccess) { ctx->err = std::string(#call) + ": " + ctx->rccl->GetErrorString(r_); ctx->rccl->GroupEnd(); return EMAP_ERR_COMM; } } while (0)

int emap_comm_unique_id(const char* rccl_path, uint8_t id_out[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  if (!id_out) return EMAP_ERR_INVALID;
  std::string why;
  RcclApi* a = rccl_open(rccl_path, &why);
  if (!a) { fprintf(stderr, "emap_comm_unique_id: %s\n", why.c_str()); return EMAP_ERR_COMM; }
  ncclUniqueId id;
  ncclResult_t r = a->GetUniqueId(&id);
  if (r != ncclSuccess) { fprintf(stderr, "emap_comm_unique_id: %s\n", a->GetErrorString(r)); delete a; return EMAP_ERR_COMM; }
  memcpy(id_out, &id, 128);
  delete a;
  return EMAP_OK;
}

static long window_cap(const emap_ctx* ctx);
static int alloc_window(emap_ctx* ctx, long cap);
int emap_comm_init(emap_ctx* ctx, const char* rccl_path, const uint8_t id[128], int32_t rank, int32_t world) {
  CKARG(ctx && id && world >= 1 && rank >= 0 && rank < world, "bad rank / world");
  CKARG(world <= 16, "at most 16 ranks");                    // (before anything collective: every rank sees the same `world`)
  CKARG(!ctx->rccl, "communicator already initialised");
  CKARG(world == 1 || ctx->strip.halo_rows > 0, "a strip of a multi-rank map needs halo rows"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  std::string why;
  RcclApi* a = rccl_open(rccl_path, &why);
  if (!a) { ctx->err = why; return EMAP_ERR_COMM; }
  ctx->rccl = a;
  ncclUniqueId uid; memcpy(&uid, id, 128);
  ncclResult_t r = a->CommInitRank(&ctx->comm, world, uid, rank);
  if (r != ncclSuccess) { ctx->err = std::string("ncclCommInitRank: ") + a->GetErrorString(r); delete a; ctx->rccl = nullptr; ctx->comm = nullptr; return EMAP_ERR_COMM; }
  ctx->comm_rank = rank; ctx->comm_world = world;
  // From here on the call is COLLECTIVE: a rank that fails locally must not leave the others waiting in an all-reduce.  The local set-up
  // therefore only collects a status; the first all-reduce carries it (max over the ranks) together with the ABI check, every rank
  // returns the same verdict, and a failed init leaves no half-built communicator behind.
  int local_rc = EMAP_OK;
  auto step = [&](hipError_t e, const char* what) { if (local_rc == EMAP_OK && e != hipSuccess) { local_rc = EMAP_ERR_HIP; ctx->err = std::string(what) + ": " + hipGetErrorString(e); } };
  step(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking), "hipStreamCreate(comm)");
  step(hipEventCreateWithFlags(&ctx->ev_ready, hipEventDisableTiming), "hipEventCreate");
  step(hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming), "hipEventCreate");
  step(hipMalloc((void**)&ctx->comm_sums, sizeof(double) * 36), "hipMalloc(comm_sums)");
  if (local_rc == EMAP_OK) step(hipMemsetAsync(ctx->comm_sums, 0, sizeof(double) * 36, ctx->stream), "hipMemsetAsync(comm_sums)");
  if (local_rc == EMAP_OK && world > 1 && ctx->prm.enable_visibility_cleanup && ctx->win_cap < window_cap(ctx))      // rays by ray: see ensure_window
    local_rc = alloc_window(ctx, window_cap(ctx));
  // EMAP_BYRAY_ALLREDUCE=1: the by-ray frames exchange their window by the three all-reduces of round 4 / 5 (rays_by_ray_pass); the
  // ranks agree on it below -- one rank alone on the other protocol would wait forever
  ctx->byray_allreduce = getenv("EMAP_BYRAY_ALLREDUCE") && atoi(getenv("EMAP_BYRAY_ALLREDUCE")) != 0;
  auto fail = [&](int rc) { const std::string keep = ctx->err; emap_comm_destroy(ctx); ctx->err = keep; return rc; };
  if (world > 1 && !ctx->comm_sums) return fail(local_rc ? local_rc : EMAP_ERR_HIP);      // (nothing to reduce through: the peers time out in RCCL -- an out-of-memory device at start-up)
  // every rank's owned physical rows (the strips need not be equally high): who holds which normal rows after a row shift
  ctx->cut_begin.assign(world, 0); ctx->cut_count.assign(world, 0);
  ctx->cut_begin[rank] = ctx->strip.row_begin; ctx->cut_count[rank] = ctx->strip.row_count;
  if (world > 1) {
    // Every rank must speak the same ABI: the halo rows are raw 16-byte cold half cells and the ray window raw 32-byte records, so a
    // peer built against another layout would exchange misaligned bytes silently.  max(v) and max(-v) over the ranks: equal and
    // opposite iff all ranks agree; the third word is the worst local status, the fourth the by-ray exchange (all-reduces if any rank asks).
    const double mine[4] = {(double)EMAP_ABI_VERSION, -(double)EMAP_ABI_VERSION, (double)(local_rc != EMAP_OK), (double)ctx->byray_allreduce};
    double got[4] = {0.0, 0.0, 0.0, 0.0};
    CK(hipMemcpyAsync(ctx->comm_sums + 16, mine, sizeof mine, hipMemcpyHostToDevice, ctx->stream));
    CKN(a->AllReduce(ctx->comm_sums + 16, ctx->comm_sums + 20, 4, ncclFloat64, ncclMax, ctx->comm, ctx->stream));
    CK(hipMemcpyAsync(got, ctx->comm_sums + 20, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (got[2] != 0.0) {
      if (local_rc == EMAP_OK) ctx->err = "emap_comm_init: another rank could not set up its communicator state";
      return fail(local_rc ? local_rc : EMAP_ERR_COMM);
    }
    if (got[0] != mine[0] || got[1] != mine[1]) {
      ctx->err = "emap_comm_init: the ranks were built against different EMAP_ABI_VERSIONs (" + std::to_string((int)-got[1]) + " .. " + std::to_string((int)got[0]) + ", this rank: " + std::to_string(EMAP_ABI_VERSION) + ")";
      return fail(EMAP_ERR_COMM);
    }
    ctx->byray_allreduce = got[3] != 0.0;
    double cuts[32], all[32];
    for (int k = 0; k < 32; ++k) cuts[k] = 0.0;
    cuts[2 * rank] = ctx->strip.row_begin; cuts[2 * rank + 1] = ctx->strip.row_count;
    CK(hipMemcpyAsync(ctx->comm_sums + 4, cuts, sizeof(double) * 2 * 16, hipMemcpyHostToDevice, ctx->stream));      // ([4..36): the host all-reduce's slots)
    CKN(a->AllReduce(ctx->comm_sums + 4, ctx->comm_sums + 4, 2 * (size_t)world, ncclFloat64, ncclSum, ctx->comm, ctx->stream));
    CK(hipMemcpyAsync(all, ctx->comm_sums + 4, sizeof(double) * 2 * world, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    long total = 0;
    for (int q = 0; q < world; ++q) { ctx->cut_begin[q] = (int)all[2 * q]; ctx->cut_count[q] = (int)all[2 * q + 1]; total += ctx->cut_count[q]; }
    ctx->cuts_ok = total == ctx->prm.cell_n;               // (checked where the boundaries are needed: normal_exchange)
  } else if (local_rc != EMAP_OK) return fail(local_rc);
  return EMAP_OK;
}

int emap_comm_destroy(emap_ctx* ctx) {
  if (!ctx || !ctx->rccl) return EMAP_OK;
  hipSetDevice(ctx->device);
  if (ctx->post_pending) post_settle(ctx);
  if (ctx->comm_stream) hipStreamSynchronize(ctx->comm_stream);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->comm) ctx->rccl->CommDestroy(ctx->comm);
  if (ctx->comm_stream) hipStreamDestroy(ctx->comm_stream);
  if (ctx->ev_ready) hipEventDestroy(ctx->ev_ready);
  if (ctx->ev_done) hipEventDestroy(ctx->ev_done);
  hipFree(ctx->comm_sums); hipFree(ctx->gather_buf); ctx->gather_buf = nullptr;
  hipFree(ctx->nlag_buf); ctx->nlag_buf = nullptr; ctx->nlag_cap = 0;
  delete ctx->rccl;
  ctx->rccl = nullptr; ctx->comm = nullptr; ctx->comm_stream = nullptr; ctx->ev_ready = ctx->ev_done = nullptr; ctx->comm_sums = nullptr;
  return EMAP_OK;
}

// halo exchange with the strip neighbours, in place, on the communication stream; main-stream work issued after this call and
// before the wait on ev_done overlaps it.  The strips are PHYSICAL row ranges of a circular map, so the neighbours form a ring:
// rank r sends its first H owned rows to r-1 and its last H owned rows to r+1 (mod world).  The logical seam of the map lies
// wherever the circular origin put it; rows across it are received like any others and masked by the stencils (is_inside).
// Posting order (sends: low, high; receives: upper halo, lower halo) keeps the pairs apart when both neighbours are the same rank.
static int ring_exchange(emap_ctx* ctx, char* base, size_t row_bytes, hipStream_t st) {
  const long H = ctx->strip.halo_rows, n = ctx->strip.row_count;
  const size_t bytes = row_bytes * (size_t)H;
  const RcclApi* a = ctx->rccl;
  const int W = ctx->comm_world, prev = (ctx->comm_rank + W - 1) % W, next = (ctx->comm_rank + 1) % W;
  CKN(a->GroupStart());
  CKG(a->Send(base + row_bytes * H, bytes, ncclChar, prev, ctx->comm, st));                  // first H owned rows
  CKG(a->Send(base + row_bytes * n, bytes, ncclChar, next, ctx->comm, st));                  // rows [n-H, n) of the strip
  CKG(a->Recv(base + row_bytes * (H + n), bytes, ncclChar, next, ctx->comm, st));            // upper halo
  CKG(a->Recv(base, bytes, ncclChar, prev, ctx->comm, st));                                  // lower halo
  CKN(a->GroupEnd());
  return EMAP_OK;
}
extern "C++" int emap_host::halo_exchange_start(emap_ctx* ctx) {
  CK(hipEventRecord(ctx->ev_ready, ctx->stream));
  CK(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_ready, 0));
  // Only the COLD half-cell plane travels: the halo rows have exactly one reader, the stencil kernel's staging loop, and it reads
  // (upper_bound, is_upper_bound, valid') from cells.cold alone (emap_kernels.hip: k_post / k_post_dma) -- the point passes, the ray
  // pass and every per-cell pass address owned rows only.  (Until round 3 both planes were sent: twice the xGMI bytes for nothing.)
  int rc = ring_exchange(ctx, reinterpret_cast<char*>(ctx->cells.cold), sizeof(float4) * (size_t)ctx->prm.cell_n, ctx->comm_stream);
  if (rc) return rc;
  CK(hipEventRecord(ctx->ev_done, ctx->comm_stream));
  return EMAP_OK;
}
// After a row shift the un-shifted normal planes (the reference does not roll normal_map, elevation_mapping.py:200-214) sit `lag`
// rows away from the cells they belong to: the normal of the cell in PHYSICAL row p lives in physical row (p + lag) mod C of the
// planes -- in this strip, with a neighbour, or (a robot that moved further than a strip is high) with a rank further away.  Before
// the visibility pass every rank therefore fetches the rows [(row_begin + lag) mod C, + row_count) into a ROW-ALIGNED copy (row j =
// the normals of owned row j; columns stay at the planes' own origin: normal_index in emap_device.h) from whoever owns them: local
// pieces by device copies, the others by ONE grouped send / receive.  Every rank derives the same list of pieces from the strips'
// boundaries (gathered by emap_comm_init) and the lag (a property of the shared origin), walks it in the same order, and so posts its
// sends and receives in matching order.  Any lag, any strip heights: a strip never reads zeros where the single context reads stale
// normals (until round 4 only lags up to halo_rows were served, from the planes' halo rows).
struct LagPiece { int q, r, src, dst, rows; };      // rank q needs physical rows [src, src + rows), owned by rank r, as rows [dst, dst + rows) of its copy
static void lag_pieces(int C, int W, const int* cut_begin, const int* cut_count, int lag, std::vector<LagPiece>& out) {
  lag = ((lag % C) + C) % C;
  for (int q = 0; q < W; ++q) {                               // rank q needs the physical rows [(b_q + lag) mod C, + n_q): <= 2 linear pieces
    const int b = (cut_begin[q] + lag) % C, nq = cut_count[q];
    for (int piece = 0; piece < 2; ++piece) {
      const int p0 = piece == 0 ? b : 0, p1 = piece == 0 ? std::min(C, b + nq) : b + nq - C;      // physical rows [p0, p1)
      const int d0 = piece == 0 ? 0 : C - b;                                                       // row of q's copy where the piece starts
      if (p1 <= p0) continue;
      for (int r = 0; r < W; ++r) {                           // ... cut by the owners of those rows
        const int o0 = std::max(p0, cut_begin[r]), o1 = std::min(p1, cut_begin[r] + cut_count[r]);
        if (o1 > o0) out.push_back(LagPiece{q, r, o0, d0 + o0 - p0, o1 - o0});
      }
    }
  }
}
// the plan as data (CPU property tests: every row of every rank's copy is written exactly once, from the row it belongs to)
int emap_normal_lag_plan(int32_t cell_n, int32_t world, const int32_t* cut_begin, const int32_t* cut_count, int32_t lag, int32_t* pieces5, int32_t max_pieces, int32_t* n_pieces) {
  if (!cut_begin || !cut_count || !pieces5 || !n_pieces || cell_n < 1 || world < 1 || max_pieces < 0) return EMAP_ERR_INVALID;
  std::vector<LagPiece> v;
  lag_pieces(cell_n, world, cut_begin, cut_count, lag, v);
  *n_pieces = (int32_t)v.size();
  if ((long)v.size() > max_pieces) return EMAP_ERR_INVALID;
  for (size_t k = 0; k < v.size(); ++k) { pieces5[5 * k] = v[k].q; pieces5[5 * k + 1] = v[k].r; pieces5[5 * k + 2] = v[k].src; pieces5[5 * k + 3] = v[k].dst; pieces5[5 * k + 4] = v[k].rows; }
  return EMAP_OK;
}
extern "C++" int emap_host::normal_exchange(emap_ctx* ctx) {
  const int C = ctx->prm.cell_n, W = ctx->comm_world, me = ctx->comm_rank;
  const long n = ctx->strip.row_count, H = ctx->strip.halo_rows;
  if (!ctx->cuts_ok) { ctx->err = "normal_exchange: the strips the ranks reported to emap_comm_init do not tile the map"; return EMAP_ERR_COMM; }
  { const int rc = grow(ctx, &ctx->nlag_buf, &ctx->nlag_cap, 3 * (size_t)n * C); if (rc) return rc; }
  std::vector<LagPiece> plan;
  lag_pieces(C, W, ctx->cut_begin.data(), ctx->cut_count.data(), normal_row_lag(ctx), plan);
  const RcclApi* a = ctx->rccl;
  const size_t rowb = sizeof(float) * (size_t)C;
  bool grouped = false;
  for (const LagPiece& pc : plan) {
    if (pc.q != me && pc.r != me) continue;
    const size_t bytes = rowb * (size_t)pc.rows;
    for (int k = 0; k < 3; ++k) {
      float* dst = ctx->nlag_buf + (size_t)k * n * C + (size_t)pc.dst * C;                                                  // (q == me)
      const float* src = ctx->normal + (size_t)k * ctx->ncells_alloc + (size_t)(H + pc.src - ctx->strip.row_begin) * C;     // (r == me)
      if (pc.q == me && pc.r == me) {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) { if (grouped) a->GroupEnd(); ctx->err = std::string("hipMemcpyAsync(normal rows): ") + hipGetErrorString(e); return EMAP_ERR_HIP; }
      } else {
        if (!grouped) { CKN(a->GroupStart()); grouped = true; }
        if (pc.q == me) CKG(a->Recv(dst, bytes, ncclChar, pc.r, ctx->comm, ctx->stream));
        else CKG(a->Send(src, bytes, ncclChar, pc.q, ctx->comm, ctx->stream));
      }
    }
  }
  if (grouped) CKN(a->GroupEnd());
  return EMAP_OK;
}

// ---- rays by ray (emap_kernels.hip: k_win_pack / k_win_prepare / k_win_unpack) ---------------------------------------------------
// Decided from values every rank shares (parameters, world size, cloud size): all ranks take the same branch of the collective code.
extern "C++" bool emap_host::rays_by_ray(const emap_ctx* ctx) {
  if (!ctx->rccl || ctx->comm_world <= 1 || !ctx->prm.enable_visibility_cleanup || ctx->ray_mode == 1) return false;
  if (!(ctx->cloud.n_all > 0 && takes_bins(ctx, ctx->cloud.n_all))) return false;      // the window march walks the frame's tile-sorted records
  // by row below 2048^2 cells: the window exchange (three all-reduces) costs about what the whole pass costs there
  return ctx->ray_mode == 2 || ctx->prm.cell_n >= 2048;
}
// the window of this frame: everything within reach of a ray of at most max_ray_length that starts at the sensor (t is map-centre
// relative); false: no cell of the map is within reach
static bool ray_window(const emap_ctx* ctx, const float t[3], Win* w) {
  const emap_params& p = ctx->prm;
  const int C = p.cell_n;
  const double reach = p.max_ray_length * 1.01 + 4.0 * p.resolution;     // (the float16 ray direction is a unit vector to 2^-10; the sample positions are rounded to half)
  auto lo = [&](double x) { double v = std::floor((x - reach) / p.resolution + 0.5 * C) - 2.0; return v < 0 ? 0 : (v > C ? C : (int)v); };
  auto hi = [&](double x) { double v = std::ceil((x + reach) / p.resolution + 0.5 * C) + 3.0; return v < 0 ? 0 : (v > C ? C : (int)v); };
  const int r_lo = lo(t[0]), r_hi = hi(t[0]), c_lo = lo(t[1]), c_hi = hi(t[1]);
  if (r_hi <= r_lo || c_hi <= c_lo) return false;
  w->r0 = r_lo & ~7; w->nr = ((r_hi - w->r0) + 7) & ~7;
  w->c0 = c_lo & ~63; w->nc = ((c_hi - w->c0) + 63) & ~63;
  return true;
}
// The largest window ray_window can return for the context's parameters (reach on both sides + its alignment slack, clipped to the map).
static long window_cap(const emap_ctx* ctx) {
  const emap_params& p = ctx->prm;
  const long C = p.cell_n;
  const double reach = p.max_ray_length * 1.01 + 4.0 * p.resolution;
  const long W = 2 * (long)std::ceil(reach / p.resolution) + 8;
  const long nr = std::min<long>(((W + 7) & ~7L) + 8, (C + 7) & ~7L), nc = std::min<long>(((W + 63) & ~63L) + 64, (C + 63) & ~63L);
  return nr * nc;
}
// (not emap_host::grow: eight buffers share one capacity, and the allocation is collective -- see ensure_window)
static int alloc_window(emap_ctx* ctx, long cap) {
  CK(hipStreamSynchronize(ctx->stream));
  hipFree(ctx->win_state); hipFree(ctx->win_rec); hipFree(ctx->win_bits); hipFree(ctx->win_thr); hipFree(ctx->win_dh); hipFree(ctx->win_key); hipFree(ctx->win_red_dh); hipFree(ctx->win_red_key);
  ctx->win_state = nullptr; ctx->win_rec = nullptr; ctx->win_bits = nullptr; ctx->win_thr = nullptr; ctx->win_dh = nullptr; ctx->win_key = nullptr; ctx->win_red_dh = nullptr; ctx->win_red_key = nullptr; ctx->win_cap = 0;
  CK(hipMalloc((void**)&ctx->win_state, sizeof(unsigned int) * 12 * (size_t)cap));      // hot 4 + cold 4 + normals 3 + wall flag 1 words per cell (local expansion)
  CK(hipMalloc((void**)&ctx->win_rec, sizeof(unsigned int) * 8 * (size_t)cap));         // the 32-byte records that travel
  CK(hipMalloc((void**)&ctx->win_bits, sizeof(unsigned long long) * ((size_t)cap / 64 + 2)));
  CK(hipMalloc((void**)&ctx->win_thr, sizeof(float) * ((size_t)cap / 64 + 1)));
  CK(hipMalloc((void**)&ctx->win_dh, sizeof(long long) * 2 * (size_t)cap));
  CK(hipMalloc((void**)&ctx->win_key, sizeof(unsigned int) * (size_t)cap));
  if (ctx->comm_world > 1) {       // what the other ranks send an owner: their {dec, hits} pairs and keys for its rows (at most the whole window, from every other rank)
    CK(hipMalloc((void**)&ctx->win_red_dh, sizeof(long long) * 2 * (size_t)cap * (size_t)(ctx->comm_world - 1)));
    CK(hipMalloc((void**)&ctx->win_red_key, sizeof(unsigned int) * (size_t)cap * (size_t)(ctx->comm_world - 1)));
  }
  ctx->win_cap = cap;
  return EMAP_OK;
}
// The window buffers are allocated COLLECTIVELY, in emap_comm_init (every rank, for the largest window its parameters allow; the
// caller's agreement step follows): an allocation that fails on one rank in the middle of a frame would leave the other ranks alone
// in the three all-reduces below.  The growth path here only runs when the parameters changed after emap_comm_init.
static int ensure_window(emap_ctx* ctx, Win* w) {
  const long n = (long)w->nr * w->nc;
  if (n > ctx->win_cap) { int rc = alloc_window(ctx, std::max(n + n / 8, window_cap(ctx))); if (rc) return rc; }
  w->hot = reinterpret_cast<float4*>(ctx->win_state); w->cold = w->hot + n;
  w->normal = reinterpret_cast<float*>(w->cold + n); w->inl = ctx->win_state + 11 * n;
  w->bits = ctx->win_bits; w->thr = ctx->win_thr; w->dh = ctx->win_dh; w->key = ctx->win_key; w->rec = ctx->win_rec;
  return EMAP_OK;
}
// The visibility pass of a sharded frame, by ray: called where emap_rays would be, between the tile kernel and k_ray_apply.
extern "C++" int emap_host::rays_by_ray_pass(emap_ctx* ctx, const float R[9], const float t[3], const Frame* f) {
  Win w; memset(&w, 0, sizeof w);
  if (!ray_window(ctx, t, &w)) return EMAP_OK;                    // the same decision on every rank: no collective is skipped one-sidedly
  int rc = ensure_window(ctx, &w); if (rc) return rc;
  const RcclApi* a = ctx->rccl;
  const long n = (long)w.nr * w.nc;
  hipStream_t st = ctx->stream;
  // (1) the window's cells, normals and wall flags as 32-byte records: owners fill their rows, an exact integer all-reduce replicates them
  CK(hipMemsetAsync(ctx->win_rec, 0, sizeof(unsigned int) * 8 * (size_t)n, st));
  KP kpk = ctx->kp;
  kpk.nlag = f->nlag ? 1 : 0;
  launch_win_pack(st, kpk, w, ctx->cells, f->nlag ? ctx->nlag_buf : ctx->normal, f->nlag ? (long)ctx->strip.row_count * ctx->prm.cell_n : ctx->ncells_alloc,
                  ctx->inl_plane, ctx->inert, ctx->rt.f_wall);
  CK(hipGetLastError());
  // Who owns which rows of the window: runs of consecutive window rows per owner, from the strips' physical rows (gathered by
  // emap_comm_init) and the map's row origin -- the same list on every rank.  With it the window is replicated by BROADCASTS from its
  // two or three owners and the effects return by REDUCTIONS to them (round 6): grouped sends / receives, every rank receives each window
  // byte once and only the owners receive effects -- a ring all-reduce moves 2 (W - 1) / W of the whole window through every rank, twice.
  // EMAP_BYRAY_ALLREDUCE=1 on any rank (emap_comm_init), or strips that do not tile the map: the three all-reduces of round 4 / 5.
  struct Run { int q, a, rows; };
  std::vector<Run> runs;
  bool owners = ctx->comm_world > 1 && ctx->cuts_ok && !ctx->byray_allreduce;
  if (owners) {
    const int C = ctx->prm.cell_n;
    for (int wr = 0; wr < w.nr && w.r0 + wr < C && owners; ++wr) {
      const int prow = (w.r0 + wr + ctx->kp.org_r) % C;
      int q = -1;
      for (int r = 0; r < ctx->comm_world; ++r) if (prow >= ctx->cut_begin[r] && prow < ctx->cut_begin[r] + ctx->cut_count[r]) { q = r; break; }
      if (q < 0) { owners = false; break; }
      if (!runs.empty() && runs.back().q == q && runs.back().a + runs.back().rows == wr) runs.back().rows++;
      else runs.push_back(Run{q, wr, 1});
    }
  }
  const int me = ctx->comm_rank, W = ctx->comm_world;
  size_t moved = 0;                                          // bytes this rank sends + receives in the frame's three exchange steps
  if (owners) {
    CKN(a->GroupStart());
    for (const Run& r : runs) {
      char* slab = reinterpret_cast<char*>(ctx->win_rec) + (size_t)r.a * w.nc * 32;
      const size_t bytes = (size_t)r.rows * w.nc * 32;
      if (r.q == me) { for (int p = 0; p < W; ++p) if (p != me) { CKG(a->Send(slab, bytes, ncclChar, p, ctx->comm, st)); moved += bytes; } }
      else { CKG(a->Recv(slab, bytes, ncclChar, r.q, ctx->comm, st)); moved += bytes; }
    }
    CKN(a->GroupEnd());
  } else {
    CKN(a->AllReduce(ctx->win_rec, ctx->win_rec, 8 * (size_t)n, ncclUint32, ncclSum, ctx->comm, st));
    moved = 32 * (size_t)n + 16 * (size_t)n + 4 * (size_t)n;      // per rank and frame: the window records + the effects ({dec, hits} sums, key maxima) that come back
  }
  // (2) bitmap + block thresholds of the window, accumulators re-armed
  launch_win_prepare(st, w, ctx->prm.cell_n);
  CK(hipMemsetAsync(w.bits + n / 64, 0xff, sizeof(unsigned long long), st));          // the all-ones word behind the last row (k_rays' passive lanes)
  CK(hipMemsetAsync(w.dh, 0, sizeof(long long) * 2 * (size_t)n, st));
  CK(hipMemsetAsync(w.key, 0, sizeof(unsigned int) * (size_t)n, st));
  // (3) the march: this rank's sorted records = the valid points of its rows, over the window
  KP kw = ctx->kp;
  kw.ray_pref = ctx->split_need ? (int)ctx->split_need[1] : 0;
  kw.org_r = kw.org_c = kw.norg_r = kw.norg_c = 0; kw.mv.n = 0;
  kw.row0 = w.r0; kw.nrows = w.nr; kw.halo = 0; kw.col0 = w.c0; kw.ncols = w.nc; kw.pitch = w.nc; kw.wmode = 1;
  Cells wc; wc.hot = w.hot; wc.cold = w.cold;
  char* const db = reinterpret_cast<char*>(w.dh);
  const AccRView av = {db, db + 8, reinterpret_cast<char*>(w.key), 16, 16, 4, 0};
  launch_rays(st, kw, make_pose(ctx, R, t), ctx->rt, ctx->cloud.pts, ctx->cloud.n, ctx->cloud.stride, wc, av, w.normal, n, ctx->frame, ctx->want_ray_stats,
              w.bits, w.inl, 1, w.thr, reinterpret_cast<const unsigned int*>(ctx->bin_recs), ctx->bin_tile_start + ctx->bg.TB);
  CK(hipGetLastError());
  // (4) effects back to the owners: sums of {dec, hits}, maxima of the upper-bound keys
  if (owners) {
    // every rank sends its pairs and keys for a run to the run's owner; an owner receives W - 1 parts per run, packed run after run
    // (part j = the j-th other rank), and folds them into its own slab
    CKN(a->GroupStart());
    long off = 0;
    for (const Run& r : runs) {
      const size_t cells = (size_t)r.rows * w.nc;
      if (r.q == me) {
        for (int p = 0, j = 0; p < W; ++p) if (p != me) {
          CKG(a->Recv(reinterpret_cast<char*>(ctx->win_red_dh + 2 * ((size_t)j * ctx->win_cap + off)), cells * 16, ncclChar, p, ctx->comm, st));
          CKG(a->Recv(reinterpret_cast<char*>(ctx->win_red_key + ((size_t)j * ctx->win_cap + off)), cells * 4, ncclChar, p, ctx->comm, st));
          moved += cells * 20; ++j;
        }
        off += (long)cells;
      } else {
        CKG(a->Send(reinterpret_cast<char*>(w.dh + 2 * (size_t)r.a * w.nc), cells * 16, ncclChar, r.q, ctx->comm, st));
        CKG(a->Send(reinterpret_cast<char*>(w.key + (size_t)r.a * w.nc), cells * 4, ncclChar, r.q, ctx->comm, st));
        moved += cells * 20;
      }
    }
    CKN(a->GroupEnd());
    off = 0;
    for (const Run& r : runs) if (r.q == me) {
      const long cells = (long)r.rows * w.nc;
      launch_win_reduce(st, w.dh + 2 * (size_t)r.a * w.nc, w.key + (size_t)r.a * w.nc, ctx->win_red_dh, ctx->win_red_key, W - 1, ctx->win_cap, off, cells);
      off += cells;
    }
  } else {
    CKN(a->AllReduce(w.dh, w.dh, 2 * (size_t)n, ncclInt64, ncclSum, ctx->comm, st));
    CKN(a->AllReduce(w.key, w.key, (size_t)n, ncclUint32, ncclMax, ctx->comm, st));
  }
  ctx->wire_bytes = moved;
  launch_win_unpack(st, ctx->kp, w, ctx->accr);
  CK(hipGetLastError());
  return EMAP_OK;
}

// exchange step 1 of a sharded frame: the ranks' drift sums (comm_sums[0..1], left there by k_gate's reduce-only launch) -> totals in [2..3]
extern "C++" int emap_host::drift_allreduce(emap_ctx* ctx) {
  CKN(ctx->rccl->AllReduce(ctx->comm_sums, ctx->comm_sums + 2, 2, ncclFloat64, ncclSum, ctx->comm, ctx->stream));
  return EMAP_OK;
}

int emap_comm_wire_bytes(emap_ctx* ctx, uint64_t* bytes) {
  CKARG(ctx && bytes, "null argument"); SF_CHECK();
  *bytes = (uint64_t)ctx->wire_bytes;
  return EMAP_OK;
}

int emap_comm_count(emap_ctx* ctx, int32_t* ranks) {
  CKARG(ctx && ranks && ctx->rccl && ctx->comm, "emap_comm_init has not been called"); SF_CHECK();
  int n = 0;
  CKN(ctx->rccl->CommCount(ctx->comm, &n));
  *ranks = n;
  return EMAP_OK;
}

// One plane of the FULL map on every rank, assembled from the strips: every rank writes its rows (logical order) into a zeroed
// cell_n x cell_n device plane and the planes are all-reduced (x + 0 + ... + 0 is exact for every x; only -0.0 comes back as +0.0).
// Read-back for publishing on a sharded map; not on the per-frame path.
int emap_comm_gather_layer(emap_ctx* ctx, int32_t plane, float* host_full_out) {
  CKARG(ctx && ctx->rccl && ctx->comm, "emap_comm_init has not been called"); SF_CHECK();
  CKARG(host_full_out && plane >= 0 && plane < EMAP_PLANE_COUNT, "bad argument");
  CK(hipSetDevice(ctx->device));
  FLUSH();
  const long C = ctx->prm.cell_n, rows = ctx->strip.row_count;
  if (!ctx->gather_buf) CK(hipMalloc((void**)&ctx->gather_buf, sizeof(float) * (size_t)C * C));
  if (plane < 7) launch_get_plane(ctx->stream, ctx->kp, ctx->cells, plane, ctx->scratch);
  else if (plane == EMAP_PLANE_TRAV_INPUT) launch_plane_view(ctx->stream, ctx->kp, ctx->torg_r, ctx->torg_c, ctx->trav_in, ctx->scratch, 0);
  else launch_plane_view(ctx->stream, ctx->kp, ctx->kp.norg_r, ctx->kp.norg_c, ctx->normal + (long)(plane - EMAP_PLANE_NORMAL_X) * ctx->ncells_alloc, ctx->scratch, 0);
  CK(hipGetLastError());
  CK(hipMemsetAsync(ctx->gather_buf, 0, sizeof(float) * (size_t)C * C, ctx->stream));
  int32_t b = 0; emap_strip_logical_begin(ctx, &b);                       // view row j = logical row (b + j) mod cell_n
  const long first = rows < C - b ? rows : C - b;
  CK(hipMemcpyAsync(ctx->gather_buf + (size_t)b * C, ctx->scratch, sizeof(float) * (size_t)first * C, hipMemcpyDeviceToDevice, ctx->stream));
  if (first < rows) CK(hipMemcpyAsync(ctx->gather_buf, ctx->scratch + (size_t)first * C, sizeof(float) * (size_t)(rows - first) * C, hipMemcpyDeviceToDevice, ctx->stream));
  CKN(ctx->rccl->AllReduce(ctx->gather_buf, ctx->gather_buf, (size_t)C * C, ncclFloat32, ncclSum, ctx->comm, ctx->stream));
  CK(hipMemcpyAsync(host_full_out, ctx->gather_buf, sizeof(float) * (size_t)C * C, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

int emap_comm_allreduce_host(emap_ctx* ctx, double* inout, int32_t n, int32_t op) {
  CKARG(ctx && ctx->rccl && ctx->comm, "emap_comm_init has not been called");
  CKARG(inout && n >= 1 && n <= 16 && (op == 0 || op == 1), "bad argument"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  double* buf = ctx->comm_sums + 4;     // [4..20) send, [20..36) receive
  CK(hipMemcpyAsync(buf, inout, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  CKN(ctx->rccl->AllReduce(buf, buf + 16, (size_t)n, ncclFloat64, op == 0 ? ncclSum : ncclMax, ctx->comm, ctx->stream));
  CK(hipMemcpyAsync(inout, buf + 16, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return EMAP_OK;
}

// Hardware self-test of the communicator (any world size): all-reduce of known values and one halo round trip.  With a single
// rank the halo rows are exchanged with the rank itself (send to / receive from rank 0 inside one group).
int emap_comm_selftest(emap_ctx* ctx) {
  CKARG(ctx && ctx->rccl && ctx->comm, "emap_comm_init has not been called"); SF_CHECK();
  CK(hipSetDevice(ctx->device));
  const RcclApi* a = ctx->rccl;
  const double mine[2] = {1.0 + ctx->comm_rank, 0.5};
  CK(hipMemcpyAsync(ctx->comm_sums, mine, sizeof mine, hipMemcpyHostToDevice, ctx->stream));
  CKN(a->AllReduce(ctx->comm_sums, ctx->comm_sums + 2, 2, ncclFloat64, ncclSum, ctx->comm, ctx->stream));
  double got[2];
  CK(hipMemcpyAsync(got, ctx->comm_sums + 2, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  const int W = ctx->comm_world;
  if (got[0] != W * (W + 1) / 2.0 || got[1] != 0.5 * W) { ctx->err = "all-reduce self-test: wrong sum"; return EMAP_ERR_COMM; }
  if (W == 1) {   // self send / recv of one row of cells through the scratch plane
    const size_t bytes = sizeof(float) * (size_t)ctx->prm.cell_n;
    float* src = ctx->scratch; float* dst = ctx->scratch + ctx->prm.cell_n;
    if ((size_t)ctx->ncells_alloc < 2 * (size_t)ctx->prm.cell_n) return EMAP_OK;
    std::string pat(bytes, 0); for (size_t i = 0; i < bytes; ++i) pat[i] = (char)(i * 7 + 3);
    CK(hipMemcpyAsync(src, pat.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(dst, 0, bytes, ctx->stream));
    CK(hipEventRecord(ctx->ev_ready, ctx->stream));
    CK(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_ready, 0));
    CKN(a->GroupStart());
    CKN(a->Send(src, bytes, ncclChar, 0, ctx->comm, ctx->comm_stream));
    CKN(a->Recv(dst, bytes, ncclChar, 0, ctx->comm, ctx->comm_stream));
    CKN(a->GroupEnd());
    CK(hipEventRecord(ctx->ev_done, ctx->comm_stream));
    CK(hipStreamWaitEvent(ctx->stream, ctx->ev_done, 0));
    std::string back(bytes, 0);
    CK(hipMemcpyAsync(&back[0], dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (back != pat) { ctx->err = "send/recv self-test: payload mismatch"; return EMAP_ERR_COMM; }
  } else if (ctx->strip.halo_rows > 0) {
    int rc = halo_exchange_start(ctx); if (rc) return rc;
    CK(hipStreamWaitEvent(ctx->stream, ctx->ev_done, 0));
    CK(hipStreamSynchronize(ctx->stream));
  }
  return EMAP_OK;
}

}  // extern "C"
