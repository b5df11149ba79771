// Stand-alone check of the records the lazy pruned sweep writes since its first span became a whole super-chunk
// (bayesianoptimizer_amd/csrc/gpx_sweep_layout.h, the only project header included).  Built and run by
// tests/test_sweep_seed_records.py with the host compiler's address and undefined-behaviour sanitizers.  Over the sizes
// tests/host/sweep_layout_check.cpp walks it states a second time, in closed form, what launch_sweep_super_pruned writes
// per span and checks it against sweep_lazy_records:
//  - the spans are [k MA, min(m, (k + 1) MA)), and sweep_span_size agrees;
//  - a first span longer than one chunk (the seeded order): PRUNE_SEED / 256 records of the seed round, then one record
//    per 256 columns of every round over ALL the span's columns (the seed's columns are not staged separately);
//  - a first span of one chunk or less (the leading block as the seed): its blocks, then the rounds over the columns
//    from the tile behind it on;
//  - a later span: the rounds over its columns;
//  - every record index a span writes lies below sweep_lazy_records.
#include <cstdio>

#include "../../bayesianoptimizer_amd/csrc/gpx_sweep_layout.h"

using namespace gpx;

static long failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++failures <= 20) {            \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// records of rounds of at most C columns over `cols` columns: whole rounds of C / 256 and the last one's blocks
static int64_t round_records(int64_t cols, int64_t C) { return cols / C * (C / 256) + ceil_div(cols % C, 256); }

static void check(int64_t n, int64_t m, long* count) {
  const int64_t npad = (n + TILE - 1) / TILE * TILE;
  if (npad < PRUNE_MIN_NPAD) return;
  const int64_t C = sweep_chunk_size(npad, m), MA = sweep_super_size(npad, m), room = sweep_lazy_records(npad, m);
  ++*count;
  int64_t recs = 0, walked = 0;
  for (int64_t k = 0; k * MA < m; ++k) {
    const int64_t s = k * MA, span = (m - s < MA) ? m - s : MA;
    CHECK(sweep_span_size(true, walked, m, C, MA) == span && walked == s, "n=%lld m=%lld span %lld", (long long)n,
          (long long)m, (long long)k);
    walked += span;
    if (k == 0 && span > C && C >= PRUNE_SEED) {
      recs += PRUNE_SEED / 256 + round_records(span, C);
    } else if (k == 0) {
      int64_t seed = span < PRUNE_SEED ? span : PRUNE_SEED;
      if (seed > C) seed = C;
      const int64_t col0 = ceil_div(seed, 128) * 128;
      recs += ceil_div(seed, 256) + (span > col0 ? round_records(span - col0, C) : 0);
    } else {
      recs += round_records(span, C);
    }
    CHECK(recs <= room, "n=%lld m=%lld: %lld records after span %lld, room for %lld", (long long)n, (long long)m,
          (long long)recs, (long long)k, (long long)room);
  }
  CHECK(walked == m, "n=%lld m=%lld: spans cover %lld", (long long)n, (long long)m, (long long)walked);
  // the seeded order needs a list of PRUNE_SEED columns in a chunk-sized index list and a count behind the stages'
  CHECK(!(m > C) || C >= PRUNE_SEED, "n=%lld m=%lld: chunk of %lld below the seed", (long long)n, (long long)m,
        (long long)C);
  CHECK(4 * (PRUNE_MAX_STAGES + 1) <= 256, "count slot");
}

int main() {
  const int64_t N[] = {1, 128, 200, 256, 257, 300, 384, 640, 1000, 4096, 16384, 100096};
  const int64_t M[] = {1, 255, 256, 257, 5000, 349440, 349441, 1 << 20, (1 << 20) + 1, 1 << 22};
  long count = 0;
  for (int64_t n : N)
    for (int64_t m : M) check(n, m, &count);
  std::printf("%ld record plans checked, %ld failures\n", count, failures);
  return failures ? 1 : 0;
}
