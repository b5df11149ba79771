// Stand-alone check of gpx_svgp_acquire_f64's workspace layout (svgp_acquire_layout in
// bayesianoptimizer_amd/csrc/gpx_svgp_layout.h, which includes gpx_sweep_layout.h; no other project header).  Built
// and run by tests/test_svgp_acquire_host.py with the host compiler's address and undefined-behaviour sanitizers.  Over
// a grid of (M, m), with the caller's pointer 256-aligned and 8, 248 and 255 bytes before an aligned address, it
// checks that
//  - the sweep's regions and the call's own regions behind them are pairwise disjoint, each inside
//    [pointer, pointer + total), by arithmetic and, for workspaces up to 8 MiB, by filling every region of a real
//    allocation of exactly `total` bytes and reading the fills back;
//  - every region of the call's own is present and 256-aligned, and holds what the launches put there (the second
//    product's partials of a chunk, a chunk of each accumulator, m scores, the sort's scratch);
//  - the sweep's part is gpx_sweep_workspace_size(M, 1, m)'s, untouched, and its records hold one scoring launch per
//    chunk of the call;
//  - the total is no smaller than gpx_svgp_predict_workspace_size(M, m)'s;
//  - every offset and the total equal a second, closed-form statement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../bayesianoptimizer_amd/csrc/gpx_svgp_layout.h"

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

static void check(int64_t M, int64_t m, size_t skew, long* count) {
  const int64_t Mpad = (M + TILE - 1) / TILE * TILE;
  const size_t sort = 4 * up(8 * (size_t)m) + up((size_t)m) + 256 + 8;  // (a stand-in of topk_workspace_bytes, unaligned)
  const SvgpAcquireLayout A = svgp_acquire_layout(Mpad, m, sort);
  const SweepLayout S = sweep_layout(Mpad, 1, m);
  char tag[128];
  std::snprintf(tag, sizeof tag, "M=%lld m=%lld skew=%zu:", (long long)M, (long long)m, skew);
  ++*count;
  // the sweep's part is the single sweep's, region by region, without a top-k or multi-output part
  CHECK(A.sweep.total == S.total && A.sweep.C == S.C && A.sweep.nrec == S.nrec, "%s sweep part", tag);
  for (int id = 0; id < SR_REGIONS; ++id)
    CHECK(A.sweep.r[id].at == S.r[id].at && A.sweep.r[id].bytes == S.r[id].bytes, "%s sweep region %d", tag, id);
  for (int id = SR_TOPK_HEAD; id < SR_REGIONS; ++id) CHECK(S.r[id].bytes == 0, "%s sweep region %d absent", tag, id);
  const size_t C = (size_t)S.C, nI = (size_t)(Mpad / 128);
  CHECK(S.r[SR_KSTAR].bytes == 8 * (size_t)Mpad * C && S.r[SR_MU_PART].bytes == 8 * (size_t)(Mpad / 64) * C &&
            S.r[SR_SS_PART].bytes == 8 * nI * C, "%s the chunk's K* and partials", tag);
  // one record per 256 candidates of every chunk's scoring launch, the chunks' blocks laid end to end
  const size_t chunks = ((size_t)m + C - 1) / C, last = (size_t)m - (chunks - 1) * C;
  CHECK((size_t)S.nrec >= (chunks - 1) * (C / 256) + (last + 255) / 256, "%s records of the scoring launches", tag);
  CHECK(S.r[SR_REC_VAL].bytes == 8 * (size_t)S.nrec && S.r[SR_REC_IDX].bytes == 8 * (size_t)S.nrec, "%s records", tag);
  // closed form
  const size_t t0 = up(S.total), p2 = 8 * nI * C, pc = 8 * C, pm = up(8 * (size_t)m);
  CHECK(p2 % 256 == 0 && pc % 256 == 0, "%s a chunk is whole 256-blocks", tag);
  CHECK(A.r[SQ_SS2_PART].at == t0 && A.r[SQ_ACC_MU].at == t0 + p2 && A.r[SQ_ACC_VAR].at == t0 + p2 + pc &&
            A.r[SQ_SCORES].at == t0 + p2 + 2 * pc && A.r[SQ_SORT_WS].at == t0 + p2 + 2 * pc + pm, "%s offsets", tag);
  CHECK(A.r[SQ_SS2_PART].bytes == p2 && A.r[SQ_ACC_MU].bytes == pc && A.r[SQ_ACC_VAR].bytes == pc &&
            A.r[SQ_SCORES].bytes == pm && A.r[SQ_SORT_WS].bytes == up(sort), "%s sizes", tag);
  CHECK(A.total == t0 + 256 + p2 + 2 * pc + pm + up(sort), "%s total %zu", tag, A.total);
  // no smaller than the predictive's (gpx_svgp_predict_workspace_size): a buffer of this call's size serves it too
  CHECK(A.total >= S.total + nI * C * 8 + 512, "%s smaller than the predictive's", tag);
  // disjoint, aligned, inside: the sweep's regions in the order of their ids, then the call's own
  size_t prev_end = 0;
  for (int id = 0; id < SR_REGIONS; ++id) {
    const SweepLayout::Region& r = A.sweep.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s sweep region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 8 == 0, "%s sweep region %d at %zu not 8-aligned", tag, id, r.at);
    CHECK(skew + r.at + r.bytes <= A.total, "%s sweep region %d ends at %zu of %zu", tag, id, skew + r.at + r.bytes, A.total);
    prev_end = r.at + r.bytes;
  }
  for (int id = 0; id < SQ_REGIONS; ++id) {
    const SweepLayout::Region& r = A.r[id];
    CHECK(r.bytes > 0, "%s region %d present", tag, id);
    CHECK(r.at >= prev_end, "%s region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 256 == 0, "%s region %d at %zu not 256-aligned", tag, id, r.at);
    CHECK(skew + r.at + r.bytes <= A.total, "%s region %d ends at %zu of %zu", tag, id, skew + r.at + r.bytes, A.total);
    prev_end = r.at + r.bytes;
  }
  if (A.total <= ((size_t)8 << 20)) {
    // (the allocation stands for [pointer, pointer + total): the sanitizer guards both ends to the byte)
    char* ws = static_cast<char*>(std::malloc(A.total));
    CHECK(ws != nullptr, "%s malloc(%zu)", tag, A.total);
    if (!ws) return;
    auto fill = [&](const SweepLayout::Region& r, int v) {
      if (r.bytes) std::memset(ws + skew + r.at, v, r.bytes);
    };
    auto kept = [&](const SweepLayout::Region& r, int v) {
      if (!r.bytes) return true;
      const char* p = ws + skew + r.at;
      return p[0] == v && p[r.bytes - 1] == v && p[r.bytes / 2] == v;
    };
    for (int id = 0; id < SR_REGIONS; ++id) fill(A.sweep.r[id], id + 1);
    for (int id = 0; id < SQ_REGIONS; ++id) fill(A.r[id], 100 + id);
    for (int id = 0; id < SR_REGIONS; ++id) CHECK(kept(A.sweep.r[id], id + 1), "%s sweep region %d overwritten", tag, id);
    for (int id = 0; id < SQ_REGIONS; ++id) CHECK(kept(A.r[id], 100 + id), "%s region %d overwritten", tag, id);
    std::free(ws);
  }
}

int main() {
  const int64_t MS[] = {1, 64, 128, 130, 200, 256, 257, 384, 640, 2048, 4096, 65536};
  const int64_t CANDS[] = {1, 255, 256, 257, 700, 1000, 5000, 131072, 1 << 20, (1 << 20) + 300, (3 << 20) + 1};
  long count = 0;
  for (size_t skew : {(size_t)0, (size_t)8, (size_t)248, (size_t)255})
    for (int64_t M : MS)
      for (int64_t m : CANDS) check(M, m, skew, &count);
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  return failures ? 1 : 0;
}
