// Stand-alone check of gpx_acquire_topk_multi_f64's workspace layout (topk_multi_layout in
// bayesianoptimizer_amd/csrc/gpx_sweep_layout.h, the only project header included).  Built and run by
// tests/test_topk_multi_host.py with the host compiler's address and undefined-behaviour sanitizers.  Over a grid of
// (n, m, k), with the caller's pointer 256-aligned and 8 bytes past an aligned address, it checks that
//  - the multi-output sweep's regions and the top-k regions behind them are pairwise disjoint, each inside
//    [pointer, pointer + total), by arithmetic and, for workspaces up to 8 MiB, by filling every region of a real
//    allocation of exactly `total` bytes and reading the fills back;
//  - every top-k region is 256-aligned;
//  - the parts the pruned form needs are there (descriptors, counts, incumbent, counters, survivor list, accumulators)
//    wherever the multi-output sweep's layout has a pruned part, and are large enough for a chunk;
//  - the sweep's own part is the one gpx_sweep_multi_workspace_size reports, untouched;
//  - every offset and the total equal a second, closed-form statement.
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

static void check(int64_t n, int64_t m, int64_t k, size_t skew, long* count) {
  const int64_t npad = (n + TILE - 1) / TILE * TILE;
  const size_t sort = 4 * up(8 * (size_t)m) + up((size_t)m) + 256 + 8;  // (a stand-in of topk_workspace_bytes, unaligned)
  const TopkMultiLayout T = topk_multi_layout(npad, m, k, sort);
  const SweepLayout S = sweep_layout(npad, 1, m, 0, true);
  char tag[128];
  std::snprintf(tag, sizeof tag, "n=%lld m=%lld k=%lld skew=%zu:", (long long)n, (long long)m, (long long)k, skew);
  ++*count;
  // the sweep's part is the multi-output sweep's, region by region
  CHECK(T.sweep.total == S.total && T.sweep.C == S.C && T.sweep.MA == S.MA && T.sweep.pruned == S.pruned, "%s sweep part",
        tag);
  for (int id = 0; id < SR_REGIONS; ++id)
    CHECK(T.sweep.r[id].at == S.r[id].at && T.sweep.r[id].bytes == S.r[id].bytes, "%s sweep region %d", tag, id);
  for (int id = SR_TOPK_HEAD; id <= SR_SORT_WS; ++id) CHECK(S.r[id].bytes == 0, "%s sweep region %d absent", tag, id);
  const size_t C = (size_t)S.C;
  CHECK(S.r[SR_ACC_MU].bytes == 8 * C && S.r[SR_ACC_VAR].bytes == 8 * C, "%s accumulators", tag);
  if (S.pruned) {
    CHECK(S.r[SR_DESC].bytes >= 2 * PRUNE_DESC_BYTES && S.r[SR_COUNT].bytes >= 4 * PRUNE_MAX_STAGES &&
              S.r[SR_TAU].bytes >= 8 && S.r[SR_STATS].bytes >= 16, "%s header", tag);
    CHECK(S.r[SR_SURVIVORS].bytes >= 8 * (C + TT), "%s survivor list holds a chunk and a tile of padding", tag);
  }
  CHECK((size_t)S.nrec >= (C + 255) / 256, "%s records of one scoring launch", tag);
  // closed form: the top-k part starts at the accumulators' end (S.total - 256 from the base), rounded up
  const size_t t0 = up(S.total - 256), pk = up(8 * (size_t)k), pc = up(8 * C), pm = up(8 * (size_t)m);
  CHECK(S.r[SR_ACC_VAR].at + S.r[SR_ACC_VAR].bytes == S.total - 256, "%s accumulators end the sweep part", tag);
  CHECK(T.r[TM_TOPK_HEAD].at == t0 && T.r[TM_POOL_VAL].at == t0 + 256 && T.r[TM_POOL_IDX].at == t0 + 256 + pk &&
            T.r[TM_LIST_VAL].at == t0 + 256 + 2 * pk && T.r[TM_LIST_IDX].at == t0 + 256 + 2 * pk + pc &&
            T.r[TM_SCORES].at == t0 + 256 + 2 * pk + 2 * pc && T.r[TM_SORT_WS].at == t0 + 256 + 2 * pk + 2 * pc + pm,
        "%s top-k offsets", tag);
  CHECK(T.r[TM_TOPK_HEAD].bytes == 256 && T.r[TM_POOL_VAL].bytes == pk && T.r[TM_POOL_IDX].bytes == pk &&
            T.r[TM_LIST_VAL].bytes == pc && T.r[TM_LIST_IDX].bytes == pc && T.r[TM_SCORES].bytes == pm &&
            T.r[TM_SORT_WS].bytes == up(sort), "%s top-k sizes", tag);
  CHECK(T.total == S.total + 512 + 2 * pk + 2 * pc + pm + up(sort), "%s total %zu", tag, T.total);
  CHECK(T.total >= S.total, "%s at least the multi-output sweep's", tag);
  // disjoint, aligned, inside: the sweep's regions in the order of their ids, then the top-k regions
  size_t prev_end = 0;
  for (int id = 0; id < SR_REGIONS; ++id) {
    const SweepLayout::Region& r = T.sweep.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s sweep region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(skew + r.at + r.bytes <= T.total, "%s sweep region %d ends at %zu of %zu", tag, id, skew + r.at + r.bytes, T.total);
    prev_end = r.at + r.bytes;
  }
  for (int id = 0; id < TM_REGIONS; ++id) {
    const SweepLayout::Region& r = T.r[id];
    CHECK(r.bytes > 0, "%s top-k region %d present", tag, id);
    CHECK(r.at >= prev_end, "%s top-k region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 256 == 0, "%s top-k region %d at %zu not 256-aligned", tag, id, r.at);
    CHECK(skew + r.at + r.bytes <= T.total, "%s top-k region %d ends at %zu of %zu", tag, id, skew + r.at + r.bytes, T.total);
    prev_end = r.at + r.bytes;
  }
  if (T.total <= ((size_t)8 << 20)) {
    // (the allocation stands for [pointer, pointer + total): the sanitizer guards both ends to the byte)
    char* ws = static_cast<char*>(std::malloc(T.total));
    CHECK(ws != nullptr, "%s malloc(%zu)", tag, T.total);
    if (!ws) return;
    auto fill = [&](const SweepLayout::Region& r, int v) {
      if (r.bytes) std::memset(ws + skew + r.at, v, r.bytes);
    };
    auto kept = [&](const SweepLayout::Region& r, int v) {
      if (!r.bytes) return true;
      const char* p = ws + skew + r.at;
      return p[0] == v && p[r.bytes - 1] == v && p[r.bytes / 2] == v;
    };
    for (int id = 0; id < SR_REGIONS; ++id) fill(T.sweep.r[id], id + 1);
    for (int id = 0; id < TM_REGIONS; ++id) fill(T.r[id], 100 + id);
    for (int id = 0; id < SR_REGIONS; ++id) CHECK(kept(T.sweep.r[id], id + 1), "%s sweep region %d overwritten", tag, id);
    for (int id = 0; id < TM_REGIONS; ++id) CHECK(kept(T.r[id], 100 + id), "%s top-k region %d overwritten", tag, id);
    std::free(ws);
  }
}

int main() {
  const int64_t N[] = {1, 128, 200, 256, 257, 300, 384, 640, 1000, 4096, 16384};
  const int64_t M[] = {1, 255, 256, 257, 700, 5000, 349440, 349441, 400000, 1 << 20, (1 << 20) + 1};
  const int64_t K[] = {1, 16, 33, 300, 1024};
  long count = 0;
  for (size_t skew : {(size_t)0, (size_t)248, (size_t)255})
    for (int64_t n : N)
      for (int64_t m : M)
        for (int64_t k : K)
          if (k <= m) check(n, m, k, skew, &count);
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  return failures ? 1 : 0;
}
