// Stand-alone check of sweep_tail_rounds (bayesianoptimizer_amd/csrc/gpx_sweep_layout.h, the only project header
// included): the tail rounds launch_sweep_super_pruned enqueues once the host has read a span's survivor count back.
// Built and run by tests/test_sweep_tail_rounds.py with the host compiler's address and undefined-behaviour sanitizers.
//  - the rounds are ceil(count / C), at least 1 (round 0 is enqueued before the count is known) and at most the span's
//    worst case ceil(ncols / C): count 0, 1, C - 1, C, C + 1, ncols, and a count beyond ncols, which is clamped;
//  - ncols that is no multiple of C; ncols <= C (one round whatever the count); ncols 0 (no round);
//  - over the chunk and super-chunk sizes of the layout: the rounds' records stay inside sweep_lazy_records, and rounds
//    r .. worst - 1 that are left out hold no survivor (r C >= count).
#include <cstdio>

#include "../../bayesianoptimizer_amd/csrc/gpx_sweep_layout.h"

using namespace gpx;

static long failures = 0, checks = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    ++checks;                            \
    if (!(cond)) {                       \
      if (++failures <= 20) {            \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static void expect(int64_t count, int64_t ncols, int64_t C, int64_t want) {
  const int64_t got = sweep_tail_rounds(count, ncols, C);
  CHECK(got == want, "count=%lld ncols=%lld C=%lld: %lld rounds, want %lld", (long long)count, (long long)ncols,
        (long long)C, (long long)got, (long long)want);
}

// one span of ncols staged columns and chunk C: the named counts, then the properties over a grid of counts
static void span(int64_t ncols, int64_t C) {
  const int64_t worst = ceil_div(ncols, C);
  if (ncols == 0) {
    expect(0, 0, C, 0);
    return;
  }
  expect(0, ncols, C, 1);
  expect(1, ncols, C, 1);
  if (C - 1 <= ncols) expect(C - 1, ncols, C, 1);
  if (C <= ncols) expect(C, ncols, C, 1);
  if (C + 1 <= ncols) expect(C + 1, ncols, C, 2);
  expect(ncols, ncols, C, worst);
  expect(ncols + 1, ncols, C, worst);                // clamped
  expect(ncols + 5 * C, ncols, C, worst);            // clamped
  expect((int64_t)0x7fffffff, ncols, C, worst);      // the largest value the device word can hold
  expect(-1, ncols, C, worst);                       // (never written by a pass: the worst case, not fewer)
  const int64_t step = ncols / 97 + 1;
  for (int64_t count = 0; count <= ncols; count += step) {
    const int64_t r = sweep_tail_rounds(count, ncols, C);
    CHECK(r >= 1 && r <= worst, "count=%lld ncols=%lld C=%lld: %lld rounds outside [1, %lld]", (long long)count,
          (long long)ncols, (long long)C, (long long)r, (long long)worst);
    CHECK(r * C >= count, "count=%lld ncols=%lld C=%lld: %lld rounds leave survivors out", (long long)count,
          (long long)ncols, (long long)C, (long long)r);
    CHECK(r == 1 || (r - 1) * C < count, "count=%lld ncols=%lld C=%lld: round %lld is empty", (long long)count,
          (long long)ncols, (long long)C, (long long)(r - 1));
  }
}

int main() {
  // the issue's shapes by hand: padded n = 384, C = 349440
  const int64_t C0 = 349440;
  expect(3, 400000, C0, 1);
  expect(C0, 400000, C0, 1);
  expect(C0 + 1, 400000, C0, 2);
  expect(400000, 400000, C0, 2);
  expect(30, (int64_t)1 << 20, C0, 1);
  expect((int64_t)1 << 20, (int64_t)1 << 20, C0, 4);
  expect(3 * C0, (int64_t)1 << 20, C0, 3);
  expect(3 * C0 + 1, (int64_t)1 << 20, C0, 4);
  expect(77, 100000, C0, 1);  // one round: no read-back is issued, and the function agrees
  // the bench shape: 32 rounds of 32768
  expect(3, (int64_t)1 << 20, 32768, 1);
  expect((int64_t)1 << 20, (int64_t)1 << 20, 32768, 32);
  // small chunks, ncols a multiple of C and not
  const int64_t Cs[] = {256, 1024, 32768, C0};
  for (int64_t C : Cs) {
    const int64_t NC[] = {0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C - 1, 5 * C + 128, 7 * C};
    for (int64_t ncols : NC) span(ncols, C);
  }
  // the layout's own chunk and super-chunk sizes: every span of a call, staged from column 0
  const int64_t N[] = {300, 384, 640, 1000, 2048, 4096, 16384};
  const int64_t M[] = {5000, 349440, 349441, 400000, 1 << 20, (1 << 20) + 1, 1100000, 1 << 22};
  for (int64_t n : N)
    for (int64_t m : M) {
      const int64_t npad = (n + TILE - 1) / TILE * TILE;
      const int64_t C = sweep_chunk_size(npad, m), MA = sweep_super_size(npad, m), room = sweep_lazy_records(npad, m);
      int64_t recs = PRUNE_SEED / WG;
      for (int64_t s = 0; s < m; s += MA) {
        const int64_t ncols = sweep_span_size(true, s, m, C, MA);
        span(ncols, C);
        recs += ceil_div(ncols, C) * (C / WG);  // at most: the worst case, whole rounds
      }
      CHECK(recs <= room, "n=%lld m=%lld: %lld records, room for %lld", (long long)n, (long long)m, (long long)recs,
            (long long)room);
    }
  std::printf("%ld tail round checks, %ld failures\n", checks, failures);
  return failures ? 1 : 0;
}
