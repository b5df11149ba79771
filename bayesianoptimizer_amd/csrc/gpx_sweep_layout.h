// The one description of the acquisition sweep's workspace: the chunk and super-chunk sizes, the spans a
// call is cut into, and sweep_layout, which walks every region once with a bump cursor.  The reported sizes
// (gpx_sweep_workspace_size, gpx_acquire_topk_workspace_size, gpx_sweep_multi_workspace_size) and the pointers the
// launches get (sweep_carve, gpx_internal.h) both come from it.  No HIP in here: tests/host/sweep_layout_check.cpp
// compiles this file alone with the host compiler and checks it against a second statement of the layout.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gpx {

constexpr int NB = 64;     // Cholesky / TRTRI block (64x64 diagonal blocks); rows per mean partial
constexpr int TILE = 128;  // padding granule and sweep tile (GPX_TILE)
constexpr int TT = 128;    // trmm tile (rows of V x candidates); rows per variance partial
constexpr int WG = 256;    // threads per workgroup (4 waves of 64); candidates per record
constexpr int PRUNE_MIN_NPAD = 384;   // below: the fused sweep, or one or two row tiles (nothing to stage)
constexpr int PRUNE_SEED = 1024;      // leading candidates of a call scored in full: the first incumbent
constexpr int PRUNE_MAX_STAGES = 8;
constexpr int PRUNE_HEAD_ROWS = 128;  // K* rows the head phase stores: the product's first row tile
constexpr int PRUNE_DESC_BYTES = 32;  // sizeof(PruneDesc)
static_assert(PRUNE_DESC_BYTES * PRUNE_MAX_STAGES <= 256 && 4 * PRUNE_MAX_STAGES <= 256, "header slots");

// The mean bound's scratch (gpx_mubound.hip): MUF_HEAD doubles of call-wide values, then per 64-row block the records
// MuPrep, MuFact, MuStat and, where the fp32 form is built, MuFact32 (gpx_mubound.hip checks the sum against the structs).
constexpr int MUF_HEAD = 32;
constexpr bool mu_fp32_form(int DMAX) { return DMAX == 8; }
constexpr int mu_prep_block_doubles(int D) {
  return (NB * D + 2 * NB + D + 2) + (NB * D + NB / 2) + (D + 4) + (mu_fp32_form(D) ? (NB * D + NB) / 2 : 0);
}
inline size_t mu_prep_doubles(int64_t npad, int d) {
  return MUF_HEAD + (size_t)(npad / NB) * mu_prep_block_doubles(d <= 4 ? 4 : d <= 8 ? 8 : 16);
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t sweep_blocks_of(int64_t m) { return m < 1 ? 256 : ((m + 255) / 256) * 256; }  // m in whole 256-blocks

inline int64_t sweep_chunk_size(int64_t npad, int64_t m) {
  // K* chunk of at most ~1 GiB, multiple of 256 candidates (tools/chunk_sweep.sh at n = 4096: 256 MiB / 8192
  // candidates -> 3.74e6, 512 MiB -> 3.78e6, 1 GiB / 32768 -> 3.81e6, 2 GiB / 65536 -> 3.73e6 candidates/s: fewer
  // launch tails and K* / finalize launches until K* outgrows what the Infinity Cache keeps warm for the trmm
  // re-reads).  The byte budget alone sets small-n chunks (tools/small_n_rates.py, 2^22 candidates: a 32768 cap
  // left n = 64 / 256 launch-bound at 3.4e8 / 2.5e8 candidates/s, 1.15e9 / 4.4e8 without it).
  int64_t cap = ((int64_t)1 << 30) / 8 / npad;
  cap = (cap / 256) * 256;
  if (cap < 256) cap = 256;
  if (cap > ((int64_t)1 << 20)) cap = (int64_t)1 << 20;
  return sweep_blocks_of(m) < cap ? sweep_blocks_of(m) : cap;
}
// The head phase's super-chunk: as many candidates as a byte budget over its per-candidate arrays holds (PRUNE_HEAD_ROWS
// rows of K*, the mean partials of every 64-row block, the variance partials of every row tile), at most 2^20 and the
// call, a multiple of 256.  1.75 GiB is 2^20 candidates at padded n = 4096; the budget bounds the arrays at any n.
inline int64_t sweep_super_size(int64_t npad, int64_t m) {
  const int64_t per = 8 * (PRUNE_HEAD_ROWS + npad / NB + npad / TT);
  int64_t cap = ((((int64_t)7 << 28) / per) / 256) * 256;
  if (cap > ((int64_t)1 << 20)) cap = (int64_t)1 << 20;
  const int64_t C = sweep_chunk_size(npad, m);
  if (cap < C) cap = C;  // (never at the sizes the library accepts: a column of K* outweighs the per-candidate arrays)
  return sweep_blocks_of(m) < cap ? sweep_blocks_of(m) : cap;
}
// The candidates of the span a call's chunk loop starts at s: a chunk, or on the lazy pruned path a super-chunk, the
// call's first one included.  Where that one is longer than a chunk its incumbent comes from the head bound's best
// column in each of PRUNE_SEED slices of the span (launch_sweep_super_pruned), not from the leading block, so a short
// first span has nothing to add.  (With the leading block as the seed a first span of 2^20 cost 23537 product tiles on
// the bench problem and a first span of one chunk 9121, profiles/r08_variants_probe.jsonl.)
inline int64_t sweep_span_size(bool lazy, int64_t s, int64_t m, int64_t C, int64_t MA) {
  const int64_t lim = lazy ? MA : C;
  return (m - s) < lim ? (m - s) : lim;
}
// Records of the lazy pruned sweep: per super-chunk the seed block's and one 256-candidate block per 256 columns of every
// tail round it can need.
inline int64_t sweep_lazy_records(int64_t npad, int64_t m) {
  const int64_t C = sweep_chunk_size(npad, m), MA = sweep_super_size(npad, m);
  const int64_t supers = (m + MA - 1) / MA + 1, rounds = (MA + C - 1) / C;  // (+ 1: room the spans no longer need since the first became a whole one; the reported sizes are pinned)
  return PRUNE_SEED / WG + supers * rounds * (C / WG);
}
// Tail rounds of a lazy span with `count` survivors among its ncols staged columns, C at most per round: one at least
// (round 0 is enqueued before the count is known), and never more than the span's worst case.  A count outside
// [0, ncols] cannot come from the passes that write it; it gets the worst case.
inline int64_t sweep_tail_rounds(int64_t count, int64_t ncols, int64_t C) {
  const int64_t worst = (ncols + C - 1) / C;
  if (count < 0 || count > ncols) return worst;
  const int64_t need = count < 1 ? 1 : (count + C - 1) / C;
  return need < worst ? need : worst;
}
// The compact K* buffers hold C/2 and C/4 columns, rounded up to the tile (a compaction at least halves the active
// columns, so they alternate: DESIGN §3).
inline int64_t prune_ld(int64_t C, int which) {
  const int64_t cols = which == 0 ? C / 2 : C / 4;
  return ((cols + TT - 1) / TT) * TT;
}

// The regions, in the order they lie in the workspace.
enum SweepRegion {
  // main part: every sweep
  SR_KSTAR,    // npad x C doubles
  SR_MU_PART,  // (npad/64) x nrhs x C doubles
  SR_SS_PART,  // (npad/128) x C doubles
  SR_REC_VAL,  // nrec doubles: a record per 256-candidate block of the call, and one more
  SR_REC_IDX,  // nrec int64
  // pruned part (one right-hand side, npad >= PRUNE_MIN_NPAD), 256-aligned
  SR_DESC,   // 256 bytes: a PruneDesc per stage
  SR_COUNT,  // 256 bytes: survivors after each stage (int)
  SR_TAU,    // 64 bytes: the incumbent
  SR_STATS,  // 192 bytes: the device counters
  SR_LIST0,  // C int2 each
  SR_LIST1,
  SR_CBUF0,  // npad x prune_ld(C, 0) doubles
  SR_CBUF1,  // npad x prune_ld(C, 1) doubles
  SR_SURVIVORS,     // the head phase: MA + 128 int2 (one tile of padding slots)
  SR_HEAD,          // PRUNE_HEAD_ROWS x MA doubles
  SR_HEAD_MU_PART,  // (npad/64) x MA doubles
  SR_HEAD_SS_PART,  // (npad/128) x MA doubles
  SR_LAZY_REC_VAL,  // sweep_lazy_records doubles
  SR_LAZY_REC_IDX,  // sweep_lazy_records int64
  // top-k part (k >= 1), behind the sweep's total; every region 256-aligned
  SR_TOPK_HEAD,  // 256 bytes: entries in the scored list and in the pool
  SR_POOL_VAL,   // k doubles
  SR_POOL_IDX,   // k int64
  SR_LIST_VAL,   // the scored list: C pairs (no launch scores more candidates in full)
  SR_LIST_IDX,
  SR_SCORES,   // the composed path's m scores
  SR_SORT_WS,  // and its sort workspace (topk_workspace_bytes)
  // multi-output part, at the sweep's total rounded up to 256
  SR_ACC_MU,  // C doubles each
  SR_ACC_VAR,
  SR_REGIONS
};
struct SweepLayout {
  struct Region { size_t at = 0, bytes = 0; };  // offset from the 256-aligned base; bytes = 0: not in this workspace
  Region r[SR_REGIONS];
  // a view, not a region of its own: the mean bound's scratch (mu_prep_doubles(npad, 16)) lies over the chunk's K*, idle
  // between the seed block's scoring and the first gather.  It must fit: the host check verifies it wherever it can run.
  Region mu_prep;
  int64_t C = 0, MA = 0;           // candidates per chunk and per super-chunk
  int64_t nrec = 0, lazy_nrec = 0; // records of the full / chunked sweep and of the lazy one
  bool pruned = false;             // the pruned part is there
  size_t after_main = 0;           // the main part's end rounded up to 256 (where the pruned part starts)
  size_t sweep_total = 0;          // gpx_sweep_workspace_size
  size_t total = 0;                // the call's reported size: sweep_total, or with the top-k or multi part
};

// npad: padded n.  k >= 1: with the top-k part (sort_bytes: topk_workspace_bytes(m), which only the HIP side knows);
// multi: with the multi-output part.  skew: the bytes from the caller's pointer up to the 256-aligned base (0 .. 255;
// only the top-k part, which starts at the first aligned address behind pointer + sweep_total, depends on it).
// `total` keeps a full 256 bytes of slack for every alignment step, whatever the step consumes.
inline SweepLayout sweep_layout(int64_t npad, int64_t nrhs, int64_t m, int64_t k = 0, bool multi = false,
                                size_t sort_bytes = 0, size_t skew = 0) {
  SweepLayout L;
  const int64_t C = L.C = sweep_chunk_size(npad, m), MA = L.MA = sweep_super_size(npad, m);
  L.nrec = (m + 255) / 256 + 1;
  size_t at = 0, reported = 256;  // (the base's own alignment)
  auto take = [&](SweepRegion id, size_t bytes) {
    L.r[id].at = at;
    L.r[id].bytes = bytes;
    at += bytes;
    reported += bytes;
  };
  take(SR_KSTAR, (size_t)npad * C * 8);
  take(SR_MU_PART, (size_t)(npad / NB) * nrhs * C * 8);
  take(SR_SS_PART, (size_t)(npad / TT) * C * 8);
  take(SR_REC_VAL, (size_t)L.nrec * 8);
  take(SR_REC_IDX, (size_t)L.nrec * 8);
  L.after_main = up256(at);
  L.pruned = nrhs == 1 && npad >= PRUNE_MIN_NPAD;
  if (L.pruned) {
    L.lazy_nrec = sweep_lazy_records(npad, m);
    at = L.after_main;
    reported += 256;
    take(SR_DESC, 256);
    take(SR_COUNT, 256);
    take(SR_TAU, 64);
    take(SR_STATS, 192);
    take(SR_LIST0, (size_t)C * 8);
    take(SR_LIST1, (size_t)C * 8);
    take(SR_CBUF0, (size_t)npad * prune_ld(C, 0) * 8);
    take(SR_CBUF1, (size_t)npad * prune_ld(C, 1) * 8);
    take(SR_SURVIVORS, (size_t)(MA + TT) * 8);
    take(SR_HEAD, (size_t)PRUNE_HEAD_ROWS * MA * 8);
    take(SR_HEAD_MU_PART, (size_t)(npad / NB) * MA * 8);
    take(SR_HEAD_SS_PART, (size_t)(npad / TT) * MA * 8);
    take(SR_LAZY_REC_VAL, (size_t)L.lazy_nrec * 8);
    take(SR_LAZY_REC_IDX, (size_t)L.lazy_nrec * 8);
    L.mu_prep.at = L.r[SR_KSTAR].at;
    L.mu_prep.bytes = mu_prep_doubles(npad, 16) * 8;
  }
  L.sweep_total = reported;
  if (k > 0) {
    at = up256(L.sweep_total - skew);
    reported += 256;
    take(SR_TOPK_HEAD, 256);
    take(SR_POOL_VAL, up256((size_t)k * 8));
    take(SR_POOL_IDX, up256((size_t)k * 8));
    take(SR_LIST_VAL, up256((size_t)C * 8));
    take(SR_LIST_IDX, up256((size_t)C * 8));
    take(SR_SCORES, up256((size_t)m * 8));
    take(SR_SORT_WS, sort_bytes);
  } else if (multi) {
    at = reported = up256(L.sweep_total);
    reported += 256;
    take(SR_ACC_MU, (size_t)C * 8);
    take(SR_ACC_VAR, (size_t)C * 8);
  }
  L.total = reported;
  return L;
}

// gpx_acquire_topk_multi_f64's workspace: the multi-output sweep's (sweep_layout with multi: the chunk's K*, partials
// and records, the pruned part's descriptors, counts, incumbent, counters and survivor list, the two accumulators), and
// behind its total the top-k regions, each 256-aligned.  The offsets count from the same 256-aligned base as the
// sweep's; the extra part starts at the first aligned offset behind the accumulators, so it does not depend on the
// caller's pointer.  tests/host/topk_multi_layout_check.cpp checks it against a second statement.
enum TopkMultiRegion {
  TM_TOPK_HEAD,  // 256 bytes: entries in the scored list and in the pool
  TM_POOL_VAL,   // k doubles
  TM_POOL_IDX,   // k int64
  TM_LIST_VAL,   // the scored list: C pairs
  TM_LIST_IDX,
  TM_SCORES,     // the composed path's m scores
  TM_SORT_WS,    // and its sort workspace (topk_workspace_bytes)
  TM_REGIONS
};
struct TopkMultiLayout {
  SweepLayout sweep;  // the multi-output sweep's regions (sweep.total: gpx_sweep_multi_workspace_size)
  SweepLayout::Region r[TM_REGIONS];
  size_t total = 0;   // gpx_acquire_topk_multi_workspace_size
};
inline TopkMultiLayout topk_multi_layout(int64_t npad, int64_t m, int64_t k, size_t sort_bytes) {
  TopkMultiLayout T;
  T.sweep = sweep_layout(npad, 1, m, 0, true);
  const SweepLayout::Region& last = T.sweep.r[SR_ACC_VAR];
  size_t at = up256(last.at + last.bytes), reported = T.sweep.total + 256;  // (one more alignment step)
  auto take = [&](TopkMultiRegion id, size_t bytes) {
    T.r[id].at = at;
    T.r[id].bytes = bytes;
    at += bytes;
    reported += bytes;
  };
  take(TM_TOPK_HEAD, 256);
  take(TM_POOL_VAL, up256((size_t)k * 8));
  take(TM_POOL_IDX, up256((size_t)k * 8));
  take(TM_LIST_VAL, up256((size_t)T.sweep.C * 8));
  take(TM_LIST_IDX, up256((size_t)T.sweep.C * 8));
  take(TM_SCORES, up256((size_t)m * 8));
  take(TM_SORT_WS, up256(sort_bytes));
  T.total = reported;
  return T;
}

}  // namespace gpx
