// Internal declarations shared by the gpx HIP translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/gpx.h"
#include "gpx_sweep_layout.h"  // NB, TILE, TT, WG, the PRUNE_* sizes and the sweep's workspace layout
#include "gpx_svgp_layout.h"   // the SVGP calls' workspace layout and its carve

namespace gpx {

static_assert(TILE == GPX_TILE, "the padding granule of the C ABI");

typedef double d4 __attribute__((ext_vector_type(4)));

// p.d and p.kind as template arguments: f gets DMAX (4, 8, 16 or 32) resp. the kernel kind as a std::integral_constant.
// A combination without a kernel (the MFMA build and the fused sweep at DMAX = 32, ...) is left out by the callers with
// `if constexpr`, so only the kernels they name are built.
template <int V>
using Const = std::integral_constant<int, V>;
template <class F>
inline void with_dmax(int d, F&& f) {
  d <= 4 ? f(Const<4>{}) : d <= 8 ? f(Const<8>{}) : d <= 16 ? f(Const<16>{}) : f(Const<32>{});
}
template <class F>
inline void with_kind(int kind, F&& f) {
  kind == GPX_KERNEL_RBF        ? f(Const<GPX_KERNEL_RBF>{})
  : kind == GPX_KERNEL_MATERN52 ? f(Const<GPX_KERNEL_MATERN52>{})
                                : f(Const<GPX_KERNEL_SCALE_LINEAR_MATERN52>{});
}

// ---- context -----------------------------------------------------------------------------------
struct PendingTimer {
  int timer;
  hipEvent_t start, stop;
};

struct Context {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  int32_t timing_mask = 0;
  double timer_ms[GPX_TIMER_COUNT] = {0};
  int64_t timer_launches[GPX_TIMER_COUNT] = {0};
  std::vector<PendingTimer> pending;
  std::vector<hipEvent_t> free_events;
  int cu_count = 0;  // CUs of the device (queried once: persistent solve grid, Cholesky slot budget)
  // bounded spins of the in-launch hand-offs (potrs): passes before a waiter gives up and reports a timeout
  unsigned spin_limit = 1u << 22;
  // options (include/gpx.h GPX_OPT_*; set by gpx_set_option or GPX_OPTIONS at gpx_create)
  int sweep_fused = 1;     // fused small-n sweep where it applies
  int gram_split = 0;      // 0 by size, else workgroups per Gram tile
  int potrf_lazy = 0;      // multi-launch flush interval, 0 by size
  int potrf_mode = -1;     // multi-launch panel mode, -1 by size
  int potrf_switch = -1;   // launch at which a single fit switches schedule (gpx_potrf.hip potrf_switch), -1 by size
  int potrf_split = -1;    // panel split policy (gpx_potrf.hip step_plan): -1 fits the slots, 1 never, 3 one per CU
  int sweep_prune = 1;     // pruned acquisition sweep: 1 where it pays, 0 never, 2 at every padded n >= 384, -2 as 2
                           // with the lazy head's exact means instead of their bound
  int sweep_head = 1;      // (gpx_debug_set_sweep_head, no option slot) lazy pruned sweep's head: 1 K* rows 0 .. 127 and row tile 0 of the product in one kernel,
                           // 0 the K* launch and the first stage apart
  int sweep_order = 1;     // (gpx_debug_set_sweep_order, no option slot) seeded lazy pruned sweep: 1 mean-first (prune on the mean's bound with
                           // the prior variance, the head over what is left), 0 the head over every column first
  int sweep_tail_sync = 1;  // (gpx_debug_set_sweep_tail_sync, no option slot) lazy pruned sweep's tail: 1 the host reads a span's
                           // survivor count back and enqueues only the rounds it needs, 0 the worst case, never waiting
  // the read-back's pinned host word and the event behind its copy (gpx_create .. gpx_destroy)
  int32_t* tail_count = nullptr;
  hipEvent_t tail_event = nullptr;
  // gpx_debug_get_tail_rounds of the last acquire or top-k call, summed over its spans: tail rounds enqueued, their
  // worst case, the survivor counts read back (-1: none was)
  int64_t tail_rounds[3] = {0, 0, -1};
  // gpx_sweep_stats of the last acquire call: the host-known parts, plus the device counters of the pruned path
  // ({candidates computed to the last row tile, product tiles executed}; they live in that call's workspace)
  int64_t sweep_stats[4] = {0, 0, 0, 0};
  const int64_t* sweep_stats_dev = nullptr;
};

// Scoped device switch of one C ABI call: makes the handle's device current and restores the caller's current device
// on exit, so a call on an engine of device k never moves the caller's (e.g. torch's) current device.
struct DeviceScope {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) {
      err = hipSetDevice(device);
      if (err != hipSuccess) prev = -1;
    } else {
      prev = -1;  // nothing to restore
    }
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// Scoped timer: records a start event on construction and a stop event on destruction when the
// timer's bit is set in the context's mask.
struct LaunchTimer {
  Context* c;
  int timer;
  hipEvent_t s = nullptr, e = nullptr;
  LaunchTimer(Context* ctx, int t);
  ~LaunchTimer();
};

// ---- batched fits -------------------------------------------------------------------------------
// `count` independent problems of the same n / d / kernel parameters (restarts or seeds, BASELINE configs[3]) run in
// the same launches: the problem index is one more grid dimension and every array of problem b starts at
// base + b * stride (element strides; a workspace slice of `ws` doubles per problem).  count = 1: a single fit.
// Read-only inputs (x, y) may use any stride >= 0 (0: every problem reads the same X, e.g. the T outputs of one
// multi-output model; y = 1 with ldy = T: output column b of one n x T target matrix).  means (device, optional): per-problem
// constant means written by the fit's Gram launches when the problems carry their own kernel parameters
// (gpx_fit_*_batched_params_f64); the triangular solves then read means[b] instead of their scalar const_mean.
struct Batch {
  int count = 1;
  int64_t x = 0, y = 0, k = 0, dinv = 0, w = 0, alpha = 0, ws = 0;
  const double* means = nullptr;
};

// ---- launch wrappers (defined in the .hip files) -------------------------------------------------
// zero / zero_bytes (optional, a multiple of 8): a buffer the Gram launch clears besides (the next launches' flags)
// mean_out (optional): mean_out[b] = p.const_mean for each problem b of the launch (Batch::means of the solves)
hipError_t launch_gram(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                       double* K, int64_t ldk, const Batch& bt = Batch(), int rb0 = 0, int32_t* info = nullptr,
                       void* zero = nullptr, size_t zero_bytes = 0, double* mean_out = nullptr);
// The forward half of alpha's triangular solve folded into the dataflow Cholesky: z = L^{-1} (Y - mean), with the
// padded rows and right-hand sides >= nrhs at 0.  buf (per problem, stride 2 npad nr doubles): the running right-hand
// sides (npad x nr), then z (npad x nr); nr = 1 for one right-hand side, else GPX_MAX_RHS (potrs' layout).
struct ForwardRhs {
  const double* Y = nullptr;
  int64_t ldy = 0, sy = 0;  // sy: Y stride per problem
  int nrhs = 1, n = 0;
  double mean = 0.0;
  const double* means = nullptr;  // per-problem means (device), overriding `mean` (Batch::means)
  double* buf = nullptr;
};
inline int rhs_row(int nrhs) { return nrhs == 1 ? 1 : GPX_MAX_RHS; }
// W (optional): the Dinv pass also writes W's diagonal blocks D_k^T (what trtri_diag would), so a fit that follows
// with launch_trtri(..., diag_done = true) saves one dispatch.  fr (optional): fold the forward substitution into the
// factorisation where the dataflow schedule runs; *z_done tells whether it did (z = buf + npad nr per problem).
hipError_t launch_potrf(Context* c, int npad, double* A, int64_t lda, double* Dinv, int32_t* info,
                        const Batch& bt = Batch(), double* W = nullptr, int64_t ldw = 0,
                        const ForwardRhs* fr = nullptr, bool* z_done = nullptr);
hipError_t launch_trtri(Context* c, int npad, const double* L, int64_t ldl, const double* Dinv, double* W,
                        int64_t ldw, double* T, const Batch& bt = Batch(), bool diag_done = false);
hipError_t launch_alpha(Context* c, int n, int npad, const double* W, int64_t ldw, const double* Y, int64_t ldy,
                        int nrhs, double const_mean, double* alpha, double* zpart, double* z,
                        const Batch& bt = Batch());
// alpha from L + Dinv by forward/backward triangular solves (gpx_potrs.hip); ws: potrs_workspace_bytes, zeroed by
// the launch itself (its hand-off granules)
size_t potrs_workspace_bytes(int64_t npad, int64_t nrhs, int64_t batch);
// ws_cleared: the granule block (potrs_clear_bytes) was already zeroed on the stream (by launch_gram in a fit)
size_t potrs_clear_bytes(int64_t npad, int64_t nrhs, int64_t batch);
// byte offset in the potrs workspace of the ForwardRhs buffer (2 npad nr doubles per problem)
size_t potrs_forward_offset(int64_t npad, int64_t nrhs, int64_t batch);
// z (optional): z = L^{-1} (Y - mean) from the factorisation (ForwardRhs; per problem at z + b * sz): the backward half
// only
hipError_t launch_potrs(Context* c, int n, int npad, const double* L, int64_t ldl, const double* Dinv,
                        const double* Y, int64_t ldy, int nrhs, double const_mean, double* alpha,
                        int32_t* info, void* ws, const Batch& bt = Batch(), bool ws_cleared = false,
                        const double* z = nullptr, int64_t sz = 0);

struct SweepBuffers {
  double* kstar;     // npad x C
  double* mu_part;   // (npad/64) x nrhs x C
  double* ss_part;   // (npad/128) x C
  double* rec_val;   // records (one per 256-candidate block over the whole sweep)
  int64_t* rec_idx;
  int64_t chunk;     // C
};
// One output t of a linear objective sum_t w_t f_t over independent GPs (gpx_acquire_argmax_multi_f64): the chunk's
// posterior of output t, untransformed by (y_mean, y_scale), weighted into chunk-sized accumulators.
struct MultiOutput {
  double weight = 1.0, y_mean = 0.0, y_scale = 1.0;
  int first = 1;
  double* acc_mu = nullptr;
  double* acc_var = nullptr;
};
// What every launch of the sweep reads: the fitted model, and the candidates of one chunk, super-chunk or round.
struct SweepModel {
  Context* c;
  const gpx_kernel_params& p;
  int n, npad;
  const double* X; int64_t ldx;
  const double* W; int64_t ldw;
  const double* alpha; int nrhs;
};
struct SweepCands {
  const double* Xs;
  int64_t ldxs, m, index_offset;  // (the global index of candidate 0)
  SweepCands first(int64_t count) const { return {Xs, ldxs, count, index_offset}; }  // the leading `count` of them
};
// Per-candidate outputs of launch_sweep_chunk: the posterior's (y_mean / y_scale per output, nullptr = identity) or the
// acquisition's optional scores.
struct SweepOut {
  double* scores = nullptr;
  const double* y_mean = nullptr;
  const double* y_scale = nullptr;
  double* mean = nullptr;
  int64_t ldmean = 0;
  double* var = nullptr;
};
// a = nullptr: posterior (write mean/var); else acquisition (records + optional scores); mo != nullptr: accumulate one
// output of a multi-output objective instead, scored afterwards by launch_multi_score
hipError_t launch_sweep_chunk(const SweepModel& M, const SweepCands& q, const SweepBuffers& b, const gpx_acq_params* a,
                              const SweepOut& out = SweepOut(), int64_t rec_offset = 0,
                              const MultiOutput* mo = nullptr);

// ---- pruned acquisition sweep (gpx_sweep.hip) ----------------------------------------------
// The product's row tiles run in stages [R_s, R_{s+1}); after each stage but the last, candidates whose score upper
// bound (variance bound from the row tiles done so far) lies below the incumbent are dropped, and the surviving K*
// columns are gathered into a compact buffer once they are at most half of the active ones.  All state is on the device.
constexpr int PRUNE_DEFAULT_NPAD = 384; // sweep_prune = 1 prunes from this padded n on (>= PRUNE_MIN_NPAD)
struct PruneDesc {  // the active column set of one stage (written by the launch before it, read by its launches)
  int buf;     // 0: the chunk's K*, 1 / 2: the compact buffers
  int col0;    // first column in the buffer (buf 0 only: the columns after the seed block)
  int ncols;   // active candidates (slots 0 .. ncols-1)
  int ntiles;  // 128-column tiles covering them
  int list;    // -1: slot s is chunk column col0 + s; 0 / 1: the index list mapping slots to chunk columns; 2: the
               // round's part of the head phase's survivor list (lazy form)
  int pad[3];
};
static_assert(sizeof(PruneDesc) == PRUNE_DESC_BYTES, "the layout's descriptor slots");
struct PruneState {  // device pointers into the sweep workspace
  double* cbuf[2];   // compact K* buffers (npad rows)
  int64_t ldc[2];    // C/2 and C/4 columns (rounded up to the tile)
  int2* list[2];     // {chunk column (-1: padding), slot in the buffer the list was built from}; C entries each
  PruneDesc* desc;   // one per stage
  int* count;        // survivors after each stage
  unsigned long long* tau;  // the incumbent, as an order-preserving key (atomic max)
  int64_t* stats;    // {candidates computed to the last row tile, 128 x 128 product tiles executed}
};
// The top-k form of the pruned sweep (gpx_acquire_topk_f64): device pointers into the call's top-k workspace.
// Every launch that scores candidates in full appends their (score, global index) to the scored list, and
// topk_pool_kernel, enqueued behind it, merges the list into the pool of the k best pairs so far and sets the incumbent
// to the pool's k-th score (-inf while the pool holds fewer than k).  nullptr in the launch functions: the argmax form.
static_assert(GPX_TOPK_SWEEP_MAX == PRUNE_SEED, "the seed block fills the pool for every legal k");
struct TopkSweep {
  int k;
  int* head;          // [0] entries in the scored list, [1] entries in the pool
  double* pool_val;   // k pairs in the result's order (score descending, index ascending)
  int64_t* pool_idx;
  double* list_val;   // the scored list: one entry per candidate a launch can score in full (sweep_chunk_size)
  int64_t* list_idx;
  double* scores;     // the composed path's score array (m) and its top-k workspace
  void* sort_ws;
  size_t sort_bytes;
};
// the pool's pairs to the caller's arrays (pruned path) / the composed path's local indices to global ones
hipError_t launch_topk_result(Context* c, const TopkSweep& tk, double* val_out, int64_t* idx_out);
hipError_t launch_index_shift(Context* c, int64_t* idx, int64_t k, int64_t offset);
bool sweep_fused_ok(const Context* c, const gpx_kernel_params& p, int npad, int nrhs);
// the pruned path applies: unfused sweep, padded n >= the option's threshold (the caller excludes scores_out != NULL)
bool sweep_prune_ok(const Context* c, const gpx_kernel_params& p, int npad);
// One chunk of gpx_acquire_argmax_f64 through the staged product; first: the call's first chunk (resets the incumbent
// and the counters, scores the seed block in full).  host_stats[1], [2] gain the seed block's share.  tk: the top-k form
// (gpx_acquire_topk_f64): same launches, the incumbent is the k-th best exact score instead of the best.
hipError_t launch_sweep_chunk_pruned(const SweepModel& M, const SweepCands& q, const SweepBuffers& b,
                                     const PruneState& ps, const gpx_acq_params* a, int64_t rec_offset, bool first,
                                     int64_t* host_stats, const TopkSweep* tk = nullptr);
// The lazy form (launch_sweep_super_pruned): K* in full height only for the survivors of the first row tile.
struct PruneHead {    // device pointers into the sweep workspace, after the compact buffers
  int64_t super;      // candidates per super-chunk (sweep_super_size); the pitch of the three arrays below
  int2* survivors;    // the head phase's survivor list: {super-chunk column, slot}; super + 128 entries
  double* head;       // PRUNE_HEAD_ROWS x super
  double* mu_part;    // (npad/64) x super
  double* ss_part;    // (npad/128) x super
  double* rec_val;    // records of the call
  int64_t* rec_idx;
  double* prep;       // the mean bound's scratch: SweepLayout::mu_prep, a view of the chunk's K*
};
// Every pointer a sweep call has into its workspace, from the one layout (gpx_sweep_layout.h).  The parts the layout
// leaves out (bytes = 0) are null.
struct SweepWorkspace {
  SweepBuffers b;
  PruneState ps;
  PruneHead ph;
  TopkSweep tk;
  double *acc_mu, *acc_var;  // the multi-output accumulators (MultiOutput)
  double* after_main;  // SweepLayout::after_main (the SVGP predictive keeps its second partials there)
};
inline SweepWorkspace sweep_carve(void* ws, const SweepLayout& L, int64_t k = 0) {
  char* base = reinterpret_cast<char*>(up256(reinterpret_cast<uintptr_t>(ws)));
  auto at = [&](SweepRegion id) { return L.r[id].bytes ? base + L.r[id].at : nullptr; };
  auto dbl = [&](SweepRegion id) { return reinterpret_cast<double*>(at(id)); };
  auto i64 = [&](SweepRegion id) { return reinterpret_cast<int64_t*>(at(id)); };
  auto i2 = [&](SweepRegion id) { return reinterpret_cast<int2*>(at(id)); };
  SweepWorkspace w;
  w.b = {dbl(SR_KSTAR), dbl(SR_MU_PART), dbl(SR_SS_PART), dbl(SR_REC_VAL), i64(SR_REC_IDX), L.C};
  w.ps = {{dbl(SR_CBUF0), dbl(SR_CBUF1)}, {prune_ld(L.C, 0), prune_ld(L.C, 1)}, {i2(SR_LIST0), i2(SR_LIST1)},
          reinterpret_cast<PruneDesc*>(at(SR_DESC)), reinterpret_cast<int*>(at(SR_COUNT)),
          reinterpret_cast<unsigned long long*>(at(SR_TAU)), i64(SR_STATS)};
  w.ph = {L.MA, i2(SR_SURVIVORS), dbl(SR_HEAD), dbl(SR_HEAD_MU_PART), dbl(SR_HEAD_SS_PART), dbl(SR_LAZY_REC_VAL),
          i64(SR_LAZY_REC_IDX), L.mu_prep.bytes ? reinterpret_cast<double*>(base + L.mu_prep.at) : nullptr};
  w.tk = {(int)k, reinterpret_cast<int*>(at(SR_TOPK_HEAD)), dbl(SR_POOL_VAL), i64(SR_POOL_IDX), dbl(SR_LIST_VAL),
          i64(SR_LIST_IDX), dbl(SR_SCORES), at(SR_SORT_WS), L.r[SR_SORT_WS].bytes};
  w.acc_mu = dbl(SR_ACC_MU);
  w.acc_var = dbl(SR_ACC_VAR);
  w.after_main = reinterpret_cast<double*>(base + L.after_main);
  return w;
}
// gpx_acquire_topk_multi_f64: the multi-output sweep's pointers, and the top-k part from the regions behind its total
inline SweepWorkspace topk_multi_carve(void* ws, const TopkMultiLayout& T, int64_t k) {
  SweepWorkspace w = sweep_carve(ws, T.sweep);
  char* base = reinterpret_cast<char*>(up256(reinterpret_cast<uintptr_t>(ws)));
  auto at = [&](TopkMultiRegion id) { return T.r[id].bytes ? base + T.r[id].at : nullptr; };
  auto dbl = [&](TopkMultiRegion id) { return reinterpret_cast<double*>(at(id)); };
  auto i64 = [&](TopkMultiRegion id) { return reinterpret_cast<int64_t*>(at(id)); };
  w.tk = {(int)k, reinterpret_cast<int*>(at(TM_TOPK_HEAD)), dbl(TM_POOL_VAL), i64(TM_POOL_IDX), dbl(TM_LIST_VAL),
          i64(TM_LIST_IDX), dbl(TM_SCORES), at(TM_SORT_WS), T.r[TM_SORT_WS].bytes};
  return w;
}
// the configurations of the MFMA K* build (fp64 covariance, d <= 16); the others keep launch_sweep_chunk_pruned
bool sweep_lazy_ok(const gpx_kernel_params& p);
// One chunk of gpx_acquire_topk_multi_f64's pruned form: the seed block of the call's first chunk through
// the full multi-output path, then per output the first row tile of the staged columns (exact objective mean, upper
// bound of its variance), one bound-and-select launch against the pool's k-th score, and per output the survivors'
// full product; their exact scores are merged into the pool.  host_stats[1], [2] gain the seed block's share.
struct MultiModel {  // one output of the objective
  const gpx_kernel_params* p;
  const double* W; int64_t ldw;
  const double* alpha;
  double weight, y_mean, y_scale;
};
hipError_t launch_topk_multi_chunk(Context* c, int T, const MultiModel* outs, int n, int npad, const double* X,
                                   int64_t ldx, const SweepCands& q, const SweepWorkspace& w, const gpx_acq_params& a,
                                   bool first, int64_t* host_stats);
// One super-chunk of gpx_acquire_argmax_f64; first: the call's first (resets the incumbent and the counters and makes the
// first incumbent: the leading block in full, or in a call longer than one chunk the head bound's best of every slice).  *recs: the records written so far, advanced.  host_stats as above.
hipError_t launch_sweep_super_pruned(const SweepModel& M, const SweepCands& q, const SweepBuffers& b,
                                     const PruneState& ps, const PruneHead& ph, const gpx_acq_params* a, int64_t* recs,
                                     bool first, int64_t* host_stats, const TopkSweep* tk = nullptr);
// K(X, Xs) through the sweep's K* build (gpx_debug_kstar_f64): list = nullptr the full-store build of columns 0 .. m-1,
// else the gather build of columns list[0 .. *count - 1] (m: the most the list can hold).  out: npad rows of pitch ldout.
hipError_t launch_debug_kstar(const SweepModel& M, const SweepCands& q, const int* list, const int* count, double* out,
                              int64_t ldout, double* mu_scratch, double* mu_part = nullptr, int64_t ldmu = 0);
// (M.alpha != nullptr, gpx_debug_kstar_mu_f64: the build's mean partials too.  Full build: mu_part[jb * ldout + c], no
// scratch; gather build: mu_part[jb * ldmu + list[s]], the partials KSTAR_FULL gives that candidate, other entries kept.)
// One stage of the staged product in a named tile shape (gpx_debug_stage_product_f64): row tiles I0 .. I0 + nrows - 1
// over slots 0 .. ncols - 1 of kstar (pitch ldk), shape 0 wide / 1 narrow, list (device, ncols entries, optional) the
// slots' output columns; ss[I * ldss + c].  ws: debug_stage_product_bytes(ncols), 256-byte aligned.
size_t debug_stage_product_bytes(int64_t ncols);
hipError_t launch_debug_stage_product(Context* c, int npad, const double* W, int64_t ldw, const double* kstar,
                                      int64_t ldk, int ncols, const int* list, int I0, int nrows, int shape, double* ss,
                                      int64_t ldss, void* ws);
// The lazy pruned sweep's fused head through the production kernel (gpx_debug_head_product_f64): ss[c] = row tile 0's
// variance partial and mu_part[jb * ld + c], jb = 0, 1, for every column up to q.m rounded up to 256 (ld at least that).
// list != nullptr (gpx_debug_head_product_list_f64): the list-driven instance over the columns list[2 s], s < *count.
hipError_t launch_debug_head_product(const SweepModel& M, const SweepCands& q, double* ss, double* mu_part, int64_t ld,
                                     const int32_t* list = nullptr, const int32_t* count = nullptr);
// The lazy pruned sweep's bound of the posterior mean (gpx_mubound.hip; RBF, fp64 covariance, d <= 16):
// mu_approx[c] +- mu_slack[c] holds the exact path's mean of candidate c.  prep: mu_prep_doubles(npad, d) doubles,
// 256-byte aligned; its first int64 ends up as the count of 256-candidate workgroups on the unfactorised path.
bool sweep_mu_bound_ok(const gpx_kernel_params& p);
hipError_t launch_mu_bound(const SweepModel& M, const SweepCands& q, double* prep, double* mu_approx, double* mu_slack);
hipError_t launch_multi_score(Context* c, const SweepCands& q, const MultiOutput& mo, const gpx_acq_params& a,
                              double* scores_out, double* rec_val, int64_t* rec_idx);
hipError_t launch_argmax_final(Context* c, const double* vals, const int64_t* idx, int64_t count, double* best_val,
                               int64_t* best_idx);
// the cross-GPU exchange (gpx_comm.cpp): pack the device record into {double value; int64 index}, and reduce
// `count` such packed records
hipError_t launch_record_pack(Context* c, const double* best_val, const int64_t* best_idx, int64_t* rec);
hipError_t launch_argmax_records(Context* c, const int64_t* rec, int64_t count, double* best_val, int64_t* best_idx);

// SVGP predictive of one task over a chunk (gpx_sweep.hip); ss2: (Mpad/128) x C partials of the full W2 product.
// mo != nullptr (gpx_svgp_acquire_f64): the same K* build and products, then the task's latent moments weighted into
// mo's accumulators (scored afterwards by launch_multi_score) instead of the predictive's outputs.
hipError_t launch_svgp_chunk(Context* c, const gpx_kernel_params& p, double min_var, int task, int M, int Mpad,
                             const double* Z, int64_t ldz, const double* W, const double* W2, int64_t ldw,
                             const double* alpha, const double* Xs, int64_t ldxs, int64_t m_chunk,
                             const SweepBuffers& b, double* ss2, double* mean_out, int64_t ldmean, double* var_out,
                             int64_t ldvar, double* score, const MultiOutput* mo = nullptr);
// The collapsed SVGP fit (gpx_svgpfit.hip; launch_svgp_kchunk: its covariance chunk through the sweep's K* build).
hipError_t launch_svgp_kchunk(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                              const double* zero_alpha, const double* Xs, int64_t ldxs, int64_t m_chunk, int64_t ldk,
                              double* kstar, double* mu_scratch);
// one chunk of one task: projection (rows reversed), residual and b_acc update; scal: {sum k(x,x), r^T r, tr}
hipError_t launch_svgp_fit_project(Context* c, const gpx_kernel_params& p, int Mpad, const double* W, const double* kc,
                                   double* phi, int64_t ldk, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                                   int mc, double* r, double* bacc, double* scal);
// the chunk's B_acc update of all tasks in one launch (task strides sp of phi, sb of B_acc)
hipError_t launch_svgp_fit_syrk(Context* c, int ntask, int Mpad, const double* phi, int64_t sp, int64_t ldk, int mc,
                                double* Bacc, int64_t sb);
// B' = I + B_acc / s2 and b' = b_acc / s2 in place (identity / 0 for a task whose *info != 0), scal[2] = tr B_acc
hipError_t launch_svgp_fit_system(Context* c, int Mpad, double s2, const int32_t* info, double* B, double* bvec,
                                  double* scal);
// u = W'^T b' per task (task strides sw / sv)
hipError_t launch_svgp_fit_utvec(Context* c, int ntask, int Mpad, const double* Wp, int64_t sw, const double* bvec,
                                 double* u, int64_t sv);
// vmean / vchol (back in the caller's index order) and the bound's GPX_SVGP_BOUND_NOUT values of one task
hipError_t launch_svgp_fit_finish(Context* c, int M, int Mpad, int64_t n, double s2, const double* Lp, const double* Wp,
                                  const double* u, const double* mrev, const double* scal, double* vmean, double* vchol,
                                  int64_t ldc, double* bound);
hipError_t launch_svgp_fit_bound(Context* c, int Mpad, int64_t n, double s2, const double* Lp, const double* u,
                                 const double* scal, double* bound);
// Conditioning on new data (gpx_svgpcond.hip).  Per chunk and task behind launch_svgp_kchunk(alpha = the
// task's alpha'): the residual e from the build's nJB rows of mean partials, then (gpx_svgpfit.hip) the projection
// U' = the row-reversed W2^T K chunk over the full k range and b_acc += U' e.
hipError_t launch_svgp_cond_resid(Context* c, double const_mean, const double* Y, int64_t ldy, int mc, const double* mu,
                                  int64_t ldk, int nJB, double* e);
hipError_t launch_svgp_cond_project(Context* c, int Mpad, const double* W2, const double* kc, double* phi, int64_t ldk,
                                    int mc, const double* e, double* bacc);
// spad = tril(vchol) zero-padded (task stride sdst doubles)
hipError_t launch_svgp_cond_pad(Context* c, int ntask, int M, int Mpad, const double* vchol, int64_t ldc,
                                int64_t stride_c, double* spad, int64_t sdst);
// out = A D per task (strides sa / sw / so), D[k][j] = Wp[Mpad-1-k][Mpad-1-j] read in place.  A full: out is Mpad x Mpad
// with exact zeros in rows / columns >= M; tri (A lower triangular): out is M x M, rows ldo apart, zeros above the
// diagonal.
hipError_t launch_svgp_compose(Context* c, int ntask, int M, int Mpad, const double* A, int64_t sa, const double* Wp,
                               int64_t sw, double* out, int64_t ldo, int64_t so, bool tri);
// alpha_out = alpha + W2 g and (vchol non-null) vmean_out = vmean + tril(vchol) g with g = the un-reversed m' (task
// stride smrev); then info[t] = 1 + the first non-finite entry of g where info[t] was 0 and there is one
hipError_t launch_svgp_cond_finish(Context* c, int ntask, int M, int Mpad, const double* W2, const double* alpha,
                                   const double* mrev, int64_t smrev, double* alpha_out, const double* vmean,
                                   int64_t stride_m, const double* vchol, int64_t ldc, int64_t stride_c,
                                   double* vmean_out, int32_t* info);
// The bound's hyperparameter gradient (gpx_svgpgrad.hip).  Between the passes, all tasks per launch (task stride ts
// doubles for every array): T1 = I - S and Q = 2I - S - B - m m^T in natural order from W', B', m' (reversed order);
// out = scale W T W^T for a symmetric T (tmp: the intermediate W T); m in natural order and sc2[2] = tr T1.
hipError_t launch_svgp_grad_sq(Context* c, int ntask, int Mpad, int64_t ts, const double* Wp, const double* Bp,
                               const double* mrev, double* T1, double* Q);
hipError_t launch_svgp_grad_conj(Context* c, int ntask, int Mpad, int64_t ts, const double* W, const double* T,
                                 double scale, double* tmp, double* out);
hipError_t launch_svgp_grad_unreverse(Context* c, int ntask, int Mpad, int64_t ts, const double* mrev, const double* T1,
                                      double* mnat, double* sc2);
// gacc (GPX_MLL_NOUT doubles, GPX_MLL_D_* slots) += sum G_A dK_ZZ/dtheta; part: (Mpad / 128)^2 rows of scratch.
// zacc (the inducing-location gradient's accumulator, Mpad rows of dmax(d) doubles; null: not wanted) = its K_ZZ part
hipError_t launch_svgp_grad_kzz(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                                const double* GA, double* part, double* gacc, double* zacc);
// one chunk of one task behind launch_svgp_kchunk(alpha = c_v): e, sc2 += {sum e, e^T e, .., sum x_k^2 at 8 + k},
// gacc += sum G_u dK_u/dtheta; part: (Mpad / 128) ceil(mc / 128) rows of scratch.  With zacc: zacc += the chunk's part of
// dF/dZ through K_u, the tiles' row partials passing through zpart ((Mpad / 128) ceil(mc / 128) blocks of 128 x dmax(d))
hipError_t launch_svgp_grad_chunk(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                                  const double* H, const double* kc, const double* mu, int64_t ldk, const double* X,
                                  int64_t ldx, const double* Y, int64_t ldy, int mc, const double* cv, double* ev,
                                  double* sc2, double* part, double* gacc, double* zpart, double* zacc);
// (with zacc: dZ[a][k] = -zacc[a][k] for a < M, k < d, rows lddz apart)
hipError_t launch_svgp_grad_finish(Context* c, const gpx_kernel_params& p, int M, int64_t n, const double* bound,
                                   const double* scal, const double* sc2, const double* gacc, double* out,
                                   const double* zacc, double* dZ, int64_t lddz);
// SVGP preparation helpers (gpx_svgp.hip)
hipError_t launch_svgp_pad(Context* c, int ntask, int M, int Mpad, const double* vmean, int64_t stride_m,
                           const double* vchol, int64_t ldc, int64_t stride_c, double* mpad, double* spad,
                           int64_t sdst);
hipError_t launch_trmv_upper(Context* c, int npad, const double* W, int64_t ldw, const double* z, double* out,
                             const Batch& bt);
hipError_t launch_svgp_w2(Context* c, int ntask, int Mpad, const double* W, const double* S, int64_t s_stride,
                          double* W2);
size_t topk_workspace_bytes(int64_t m);
hipError_t launch_topk(Context* c, const double* scores, int64_t m, int64_t k, int64_t* idx_out, double* val_out,
                       void* ws, size_t ws_bytes);
hipError_t launch_fps(Context* c, const double* X, int64_t m, int d, int64_t ldx, int64_t k, int64_t start,
                      int64_t* idx_out);

hipError_t launch_append(Context* c, const gpx_kernel_params& p, int n_old, int n_new, const double* X, int64_t ldx,
                         double* L, int64_t ldl, double* Dinv, double* W, int64_t ldw, int32_t* info, double* ws);
size_t append_workspace_bytes(int64_t n_old, int64_t n_new);

size_t moments_grad_ws_doubles(int npad, int m);
hipError_t launch_moments_grad(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                               const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t ldxs,
                               int m, int q, double* mean, double* dmean, double* cov, double* dcov, double* ws);

// K*[i][c] = k(X_i, Xs_c) for i < n, c < m; 0 elsewhere (npad x mpad, row length mpad).  Defined in gpx_grad.hip; also
// launched by gpx_svgpmom.hip.
__global__ void __launch_bounds__(WG) kstar_plain_kernel(gpx_kernel_params p, int n, int npad, int m, int mpad,
                                                         const double* __restrict__ X, int64_t ldx,
                                                         const double* __restrict__ Xs, int64_t ldxs,
                                                         double* __restrict__ Ks);

// The same for one task of an SVGP (gpx_svgpmom.hip): W, W2 (Mpad x Mpad) and alpha (Mpad) are the task's blocks of
// gpx_svgp_prepare_f64.  dmean / dcov both null: values only (the same bits of mean and cov).
size_t svgp_moments_ws_doubles(int Mpad, int m);
hipError_t launch_svgp_moments(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                               const double* W, const double* W2, const double* alpha, const double* Xs, int64_t ldxs,
                               int m, int q, double* mean, double* dmean, double* cov, double* dcov, double* ws);

// MC q-batch acquisition from the moments (gpx_mcacq.hip); gmean / gcov both null: value only
size_t mc_acq_ws_doubles(int64_t B, int64_t q, int64_t S);
hipError_t launch_mc_acq(Context* c, const gpx_mcacq_params& a, int B, int q, int S, const double* mean,
                         const double* cov, const double* z, double* value, double* gmean, double* gcov, int32_t* info,
                         double* ws);

// MC noisy expected improvement from the moments and the cross-covariance to the baseline (gpx_mcacq.hip); gmean /
// gcov / gcross all null: value only
size_t mc_nei_ws_doubles(int64_t B, int64_t q, int64_t nb, int64_t S);
hipError_t launch_mc_nei(Context* c, const gpx_mcnei_params& a, int B, int q, int nb, int S, const double* mean,
                         const double* cov, const double* cross, const double* Linv, const double* zb,
                         const double* best, const double* zq, double* value, double* gmean, double* gcov,
                         double* gcross, int32_t* info, double* ws);

// joint posterior at the baseline points and the cross-covariance of candidates to them (gpx_grad.hip)
size_t joint_moments_ws_doubles(int npad, int mb);
hipError_t launch_joint_moments(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xb, int mb,
                                int64_t ldxb, double* mean_b, double* cov_bb, double* Sb, int64_t ldsb, double* ws);
hipError_t launch_cross_cov_grad(Context* c, const gpx_kernel_params& p, int n, const double* X, int64_t ldx,
                                 const double* Sb, int64_t ldsb, const double* Xb, int nb, int64_t ldxb,
                                 const double* Xs, int m, int64_t ldxs, double* cross, double* dcross);

size_t mll_workspace_bytes(int64_t npad);
hipError_t launch_mll(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                      const double* Y, int64_t ldy, int nrhs, const double* L, int64_t ldl, const double* W,
                      int64_t ldw, const double* alpha, double* out, double* part);

}  // namespace gpx
