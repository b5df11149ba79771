// Stand-alone check of the acquisition sweep's workspace layout (bayesianoptimizer_amd/csrc/gpx_sweep_layout.h, the
// only project header included).  Built and run by tests/test_sweep_workspace_sizes.py with the host compiler's address
// and undefined-behaviour sanitizers.  Over the grid of tests/golden/sweep_workspace_sizes.json, with the caller's
// pointer 256-aligned and 8 bytes past an aligned address, it checks that
//  - the regions are pairwise disjoint (the mean bound's scratch is the one declared view, over K*) and each lies within
//    [pointer, pointer + total), by arithmetic and, for workspaces up to 8 MiB, by filling every region of a real
//    allocation of exactly `total` bytes and reading the fills back;
//  - each region has its alignment;
//  - the mean bound's scratch fits the K* region wherever the pruned part exists;
//  - the lazy records cover what the span iteration of the C ABI (sweep_span_size) and the rounds of
//    launch_sweep_super_pruned write;
//  - every offset and total equals a second, closed-form statement of the layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../bayesianoptimizer_amd/csrc/gpx_sweep_layout.h"

using namespace gpx;

static long failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++failures <= 20) {                     \
        std::printf("FAIL %s: ", #cond);          \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

static size_t up(size_t b) { return (b + 255) / 256 * 256; }

// alignment each region must have (bytes)
static size_t alignment(int id) {
  switch (id) {
    case SR_KSTAR: case SR_DESC: case SR_COUNT: case SR_TAU: case SR_LIST0:
    case SR_TOPK_HEAD: case SR_POOL_VAL: case SR_POOL_IDX: case SR_LIST_VAL: case SR_LIST_IDX: case SR_SCORES:
    case SR_SORT_WS: case SR_ACC_MU:
      return 256;
    case SR_STATS:
      return 64;
    default:
      return 8;
  }
}

// the second statement of the layout: offsets from the aligned base, region by region (skew: pointer to base)
static void closed_form(int64_t npad, int64_t nrhs, int64_t m, int64_t k, bool multi, size_t sort, size_t skew,
                        const SweepLayout& L, const char* tag) {
  const size_t C = (size_t)L.C, MA = (size_t)L.MA, n8 = (size_t)npad * 8;
  const size_t nrec = (size_t)((m + 255) / 256 + 1);
  CHECK((size_t)L.nrec == nrec, "%s nrec", tag);
  const size_t mu = n8 * C, ss = mu + n8 / 64 * nrhs * C, rv = ss + n8 / 128 * C, ri = rv + 8 * nrec, end = ri + 8 * nrec;
  CHECK(L.r[SR_KSTAR].at == 0 && L.r[SR_MU_PART].at == mu && L.r[SR_SS_PART].at == ss && L.r[SR_REC_VAL].at == rv &&
            L.r[SR_REC_IDX].at == ri && L.after_main == up(end), "%s main part", tag);
  size_t total = end + 256;
  const bool pruned = nrhs == 1 && npad >= 384;
  CHECK(L.pruned == pruned, "%s pruned", tag);
  if (pruned) {
    const size_t q = up(end), ld0 = (C / 2 + 127) / 128 * 128, ld1 = (C / 4 + 127) / 128 * 128;
    const size_t lazy = (size_t)sweep_lazy_records(npad, m);
    const size_t list1 = q + 768 + 8 * C, c0 = list1 + 8 * C, c1 = c0 + n8 * ld0, sv = c1 + n8 * ld1;
    const size_t hd = sv + 8 * (MA + 128), hmu = hd + 8 * 128 * MA, hss = hmu + n8 / 64 * MA, lv = hss + n8 / 128 * MA;
    CHECK(L.r[SR_DESC].at == q && L.r[SR_COUNT].at == q + 256 && L.r[SR_TAU].at == q + 512 &&
              L.r[SR_STATS].at == q + 576 && L.r[SR_LIST0].at == q + 768 && L.r[SR_LIST1].at == list1, "%s header", tag);
    CHECK(L.r[SR_CBUF0].at == c0 && L.r[SR_CBUF1].at == c1 && L.r[SR_SURVIVORS].at == sv, "%s compact buffers", tag);
    CHECK(L.r[SR_HEAD].at == hd && L.r[SR_HEAD_MU_PART].at == hmu && L.r[SR_HEAD_SS_PART].at == hss &&
              L.r[SR_LAZY_REC_VAL].at == lv && L.r[SR_LAZY_REC_IDX].at == lv + 8 * lazy, "%s head", tag);
    CHECK((size_t)prune_ld(L.C, 0) == ld0 && (size_t)prune_ld(L.C, 1) == ld1 && (size_t)L.lazy_nrec == lazy, "%s ld", tag);
    CHECK(L.mu_prep.at == 0 && L.mu_prep.bytes > 0, "%s prep view", tag);
    total += 256 + (lv + 16 * lazy - q);
  } else {
    for (int id = SR_DESC; id <= SR_LAZY_REC_IDX; ++id) CHECK(L.r[id].bytes == 0, "%s region %d absent", tag, id);
    CHECK(L.mu_prep.bytes == 0, "%s no prep view", tag);
  }
  CHECK(L.sweep_total == total, "%s sweep total %zu, closed form %zu", tag, L.sweep_total, total);
  if (k > 0) {
    const size_t t0 = up(total - skew), pk = up(8 * (size_t)k), pc = up(8 * C);  // first aligned address behind the sweep
    CHECK(L.r[SR_TOPK_HEAD].at == t0 && L.r[SR_POOL_VAL].at == t0 + 256 && L.r[SR_POOL_IDX].at == t0 + 256 + pk &&
              L.r[SR_LIST_VAL].at == t0 + 256 + 2 * pk && L.r[SR_LIST_IDX].at == t0 + 256 + 2 * pk + pc &&
              L.r[SR_SCORES].at == t0 + 256 + 2 * pk + 2 * pc &&
              L.r[SR_SORT_WS].at == t0 + 256 + 2 * pk + 2 * pc + up(8 * (size_t)m), "%s top-k part", tag);
    CHECK(L.r[SR_SORT_WS].bytes == sort, "%s sort workspace", tag);
    total += 512 + 2 * pk + 2 * pc + up(8 * (size_t)m) + sort;
  } else if (multi) {
    CHECK(L.r[SR_ACC_MU].at == up(total) && L.r[SR_ACC_VAR].at == up(total) + 8 * C, "%s multi part", tag);
    total = up(total) + 16 * C + 256;
  }
  CHECK(L.total == total, "%s total %zu, closed form %zu", tag, L.total, total);
}

// the records the lazy path writes: the spans of the C ABI's loop, per span the seed block's (first span only) and one
// block per 256 columns of each tail round (launch_sweep_super_pruned)
static int64_t lazy_records_written(const SweepLayout& L, int64_t m, int64_t* supers_out, int64_t* rounds_out) {
  int64_t recs = 0, supers = 0, rounds_max = 0;
  for (int64_t s = 0, ms = 0; s < m; s += ms, ++supers) {
    ms = sweep_span_size(true, s, m, L.C, L.MA);
    int64_t seed = s == 0 ? (ms < PRUNE_SEED ? ms : PRUNE_SEED) : 0;
    if (seed > L.C) seed = L.C;
    recs += (seed + WG - 1) / WG;
    const int64_t col0 = (seed + TT - 1) / TT * TT, ncols = ms > col0 ? ms - col0 : 0;
    int64_t rounds = 0;
    for (int64_t r0 = 0; r0 < ncols; r0 += L.C, ++rounds) {
      const int64_t cap = ncols - r0 < L.C ? ncols - r0 : L.C;
      recs += (cap + WG - 1) / WG;
    }
    if (rounds > rounds_max) rounds_max = rounds;
  }
  *supers_out = supers;
  *rounds_out = rounds_max;
  return recs;
}

static void check(int64_t n, int64_t nrhs, int64_t m, int64_t k, bool multi, size_t skew, long* count) {
  const int64_t npad = (n + TILE - 1) / TILE * TILE;
  const size_t sort = k > 0 ? 4 * up(8 * (size_t)m) + up((size_t)m) + 256 : 0;  // (a stand-in of topk_workspace_bytes)
  const SweepLayout L = sweep_layout(npad, nrhs, m, k, multi, sort, skew);
  char tag[128];
  std::snprintf(tag, sizeof tag, "n=%lld nrhs=%lld m=%lld k=%lld multi=%d skew=%zu:", (long long)n, (long long)nrhs,
                (long long)m, (long long)k, (int)multi, skew);
  ++*count;
  CHECK(L.C % 256 == 0 && L.MA % 256 == 0 && L.C >= 256 && L.C <= L.MA, "%s C = %lld, MA = %lld", tag, (long long)L.C,
        (long long)L.MA);
  CHECK(sweep_layout(npad, nrhs, m, k, multi, sort, 0).total == L.total, "%s total depends on the pointer", tag);
  closed_form(npad, nrhs, m, k, multi, sort, skew, L, tag);
  // disjoint (the regions are in the order of their ids), aligned, inside the reported bytes
  size_t prev_end = 0;
  for (int id = 0; id < SR_REGIONS; ++id) {
    const SweepLayout::Region& r = L.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % alignment(id) == 0, "%s region %d at %zu not %zu-aligned", tag, id, r.at, alignment(id));
    CHECK(skew + r.at + r.bytes <= L.total, "%s region %d ends at %zu of %zu", tag, id, skew + r.at + r.bytes, L.total);
    prev_end = r.at + r.bytes;
  }
  if (L.pruned) {
    CHECK(L.mu_prep.at == L.r[SR_KSTAR].at && L.mu_prep.bytes <= L.r[SR_KSTAR].bytes,
          "%s the mean bound's scratch (%zu bytes) outgrows K* (%zu)", tag, L.mu_prep.bytes, L.r[SR_KSTAR].bytes);
    CHECK(L.mu_prep.bytes == 8 * mu_prep_doubles(npad, 16) && mu_prep_doubles(npad, 16) >= mu_prep_doubles(npad, 8) &&
              mu_prep_doubles(npad, 16) >= mu_prep_doubles(npad, 4), "%s the scratch is sized for the widest d", tag);
    int64_t supers = 0, rounds = 0;
    const int64_t written = lazy_records_written(L, m, &supers, &rounds);
    CHECK(L.lazy_nrec >= PRUNE_SEED / 256 + supers * rounds * (L.C / 256), "%s %lld lazy records, %lld supers x %lld rounds",
          tag, (long long)L.lazy_nrec, (long long)supers, (long long)rounds);
    CHECK(L.lazy_nrec >= written, "%s %lld lazy records, %lld written", tag, (long long)L.lazy_nrec, (long long)written);
    CHECK(L.r[SR_LAZY_REC_VAL].bytes == 8 * (size_t)L.lazy_nrec && L.r[SR_LAZY_REC_IDX].bytes == 8 * (size_t)L.lazy_nrec,
          "%s lazy record regions", tag);
  }
  CHECK(L.nrec >= (m + 255) / 256, "%s records of the chunked sweep", tag);
  // a real workspace of exactly the reported size: fill every region with its id, read the fills back
  if (L.total <= ((size_t)8 << 20)) {
    // (the allocation stands for [pointer, pointer + total): the sanitizer guards both ends to the byte; the base is
    // `skew` bytes in, whatever the allocation's own address)
    char* ws = static_cast<char*>(std::malloc(L.total));
    CHECK(ws != nullptr, "%s malloc(%zu)", tag, L.total);
    if (!ws) return;
    for (int id = 0; id < SR_REGIONS; ++id)
      if (L.r[id].bytes) std::memset(ws + skew + L.r[id].at, id + 1, L.r[id].bytes);
    for (int id = 0; id < SR_REGIONS; ++id)
      if (L.r[id].bytes) {
        const char* p = ws + skew + L.r[id].at;
        CHECK(p[0] == id + 1 && p[L.r[id].bytes - 1] == id + 1 && p[L.r[id].bytes / 2] == id + 1,
              "%s region %d overwritten", tag, id);
      }
    std::free(ws);
  }
}

int main() {
  const int64_t N[] = {1, 128, 200, 256, 257, 300, 384, 640, 1000, 4096, 16384, 100096};
  const int64_t NRHS[] = {1, 3, 8};
  const int64_t M[] = {1, 255, 256, 257, 5000, 349440, 349441, 1 << 20, (1 << 20) + 1, 1 << 22};
  const int64_t K[] = {1, 16, 1024};
  long count = 0;
  for (size_t skew : {(size_t)0, (size_t)248})  // the pointer aligned, and 8 bytes past an aligned address
    for (int64_t n : N)
      for (int64_t m : M) {
        for (int64_t nrhs : NRHS) check(n, nrhs, m, 0, false, skew, &count);
        for (int64_t k : K)
          if (k <= m) check(n, 1, m, k, false, skew, &count);
        check(n, 1, m, 0, true, skew, &count);
      }
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  return failures ? 1 : 0;
}
