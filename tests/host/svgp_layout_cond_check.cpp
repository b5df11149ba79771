// Stand-alone check of the workspace layout of gpx_svgp_condition_f64 (the kind SVGP_CONDITION of
// bayesianoptimizer_amd/csrc/gpx_svgp_layout.h, the only project header included).  Built and run by
// tests/test_svgp_condition_layout.py, with the host compiler's address and undefined-behaviour sanitizers where they
// are installed.  Over a grid of (M, ntask, chunk width), with the caller's pointer 256-aligned and 8 bytes past an
// aligned address, it checks that
//  - the new kind's regions are pairwise disjoint, 256-aligned and inside [pointer, pointer + reported size), by
//    arithmetic and, for workspaces up to 8 MiB, by filling every region of a real allocation of exactly the reported
//    size through SvgpWorkspace's pointers and reading the fills back;
//  - every offset, the task pitch, the chunk pitch, the clear span and the total equal a closed form restated here: the
//    fit's regions without the zero vector and the second info words, plus the padded S;
//  - the four older kinds equal their closed forms and are not changed by the new kind's existence;
//  - svgp_chunk_width of the new kind equals a downward loop over the reported sizes, refuses a workspace one byte
//    below the chunk = 128 size and allows that size.
// Its last lines print the reported bytes of the cases pinned by tests/golden/svgp_condition_workspace_sizes.json.
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

static const int64_t NOUT = 72;         // GPX_MLL_NOUT (include/gpx.h)
static const int64_t ZDIM = 32;         // GPX_MAX_DIM
static const int64_t CHUNK_CAP = 4096;  // GPX_SVGP_FIT_CHUNK

static size_t up(size_t b) { return (b + 255) / 256 * 256; }
static size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// The older kinds' task pitch and total in closed form (the sums of the regions DESIGN §7 lists)
static void closed_form(SvgpKind kind, size_t Mpad, size_t T, size_t C, size_t* task, size_t* total) {
  const size_t mat = up(8 * Mpad * Mpad), vec = up(8 * Mpad), D = up(1024 * Mpad), tr = 2 * Mpad * Mpad + 256;
  if (kind == SVGP_PREPARE) {
    *task = mat + D + up(max2(tr, (Mpad / 128 + 1) * Mpad * 8 + 512)) + mat + vec;
    *total = *task * T;
    return;
  }
  const bool grad = kind == SVGP_GRAD || kind == SVGP_GRAD_Z;
  *task = 2 * mat + D + up(tr) + 3 * vec + 256;
  if (grad) *task += 3 * mat + 2 * vec + 512 + up(8 * NOUT) + 256;
  if (kind == SVGP_GRAD_Z) *task += up(8 * Mpad * ZDIM);
  const size_t ldk = (C + 255) / 256 * 256, pt = up(8 * Mpad * ldk);
  *total = *task * T + vec + up(4 * T) + (1 + T) * pt + up(8 * (Mpad / 64) * ldk) + up(8 * ldk);
  if (grad) {
    const size_t nI = Mpad / 128, ncb = C / 128;
    *total += up(8 * ldk) + up(8 * nI * max2(nI, ncb) * NOUT);
    if (kind == SVGP_GRAD_Z) *total += up(8 * nI * max2(nI, ncb) * 128 * ZDIM);
  }
}

static void check_old(SvgpKind kind, int64_t M, int64_t ntask, int64_t C, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128;
  const SvgpLayout L = svgp_layout(kind, Mpad, ntask, C, NOUT, ZDIM);
  size_t task, total;
  closed_form(kind, (size_t)Mpad, (size_t)ntask, (size_t)C, &task, &total);
  ++*count;
  CHECK(L.task == task && L.total == total, "kind=%d M=%lld ntask=%lld C=%lld: pitch %zu total %zu, closed form %zu %zu",
        (int)kind, (long long)M, (long long)ntask, (long long)C, L.task, L.total, task, total);
  if (kind != SVGP_PREPARE)
    CHECK(L.r[SV_SPAD].bytes == 0 && L.r[SV_ZERO].bytes != 0 && L.r[SV_INFO2].bytes != 0,
          "kind=%d: the padded S / the zero vector / the second info words", (int)kind);
}

static void check_cond(int64_t M, int64_t ntask, int64_t C, size_t skew, long* count) {
  const size_t Mpad = (size_t)((M + 127) / 128 * 128), T = (size_t)ntask;
  const SvgpLayout L = svgp_layout(SVGP_CONDITION, (int64_t)Mpad, ntask, C);
  const size_t reported = L.total + 256;
  char tag[128];
  std::snprintf(tag, sizeof tag, "M=%lld ntask=%lld C=%lld skew=%zu:", (long long)M, (long long)ntask, (long long)C,
                skew);
  ++*count;
  CHECK(L.task % 256 == 0 && L.task > 0, "%s task pitch %zu", tag, L.task);
  // disjoint (the regions lie in the order of their ids), aligned, inside the block resp. the reported bytes
  size_t prev_end = 0;
  for (int id = 0; id < SV_REGIONS; ++id) {
    if (id == SV_SHARED) {
      CHECK(prev_end <= L.task, "%s the task's regions end at %zu of %zu", tag, prev_end, L.task);
      prev_end = L.task * T;
    }
    const SvgpLayout::Region& r = L.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 256 == 0, "%s region %d at %zu not 256-aligned", tag, id, r.at);
    prev_end = r.at + r.bytes;
  }
  CHECK(prev_end <= L.total && skew + L.total <= reported, "%s regions end at %zu of %zu", tag, prev_end, L.total);
  // the closed form: which regions, where, how large
  const size_t mat = up(8 * Mpad * Mpad), vec = up(8 * Mpad), D = up(1024 * Mpad), tr = up(2 * Mpad * Mpad + 256);
  const size_t ldk = ((size_t)C + 255) / 256 * 256, pt = up(8 * Mpad * ldk), mu = up(8 * (Mpad / 64) * ldk);
  const size_t task = 3 * mat + D + tr + 3 * vec + 256;
  struct Want { SvgpRegion id; size_t at, bytes; };
  const Want want[] = {
      {SV_A, 0, mat},
      {SV_WB, mat, mat},
      {SV_DINV, 2 * mat, D},
      {SV_SLICE, 2 * mat + D, tr},
      {SV_SPAD, 2 * mat + D + tr, mat},
      {SV_BVEC, 3 * mat + D + tr, vec},
      {SV_U, 3 * mat + D + tr + vec, vec},
      {SV_MREV, 3 * mat + D + tr + 2 * vec, vec},
      {SV_SCAL, 3 * mat + D + tr + 3 * vec, 256},
      {SV_KC, task * T, pt},
      {SV_PHI, task * T + pt, pt * T},
      {SV_MU, task * T + (1 + T) * pt, mu},
      {SV_R, task * T + (1 + T) * pt + mu, up(8 * ldk)},
  };
  bool listed[SV_REGIONS] = {};
  for (const Want& q : want) {
    listed[q.id] = true;
    CHECK(L.r[q.id].at == q.at && L.r[q.id].bytes == q.bytes, "%s region %d: at %zu, %zu bytes; closed form %zu, %zu", tag,
          (int)q.id, L.r[q.id].at, L.r[q.id].bytes, q.at, q.bytes);
  }
  for (int id = 0; id < SV_REGIONS; ++id)
    if (!listed[id]) CHECK(L.r[id].bytes == 0, "%s region %d is not the conditioning call's", tag, id);
  CHECK(L.task == task && L.phi_task == pt && (size_t)L.ldk == ldk &&
            L.total == task * T + (1 + T) * pt + mu + up(8 * ldk),
        "%s pitch %zu, chunk pitch %zu, ldk %lld, total %zu", tag, L.task, L.phi_task, (long long)L.ldk, L.total);
  CHECK(L.acc.at == L.r[SV_BVEC].at && L.acc.bytes == 3 * vec + 256 && L.acc2.bytes == 0, "%s clear spans", tag);
  // what the launches write fits: the chunk and its projections (Mpad x ldk), the mean partials, the residual
  CHECK(pt >= 8 * Mpad * (size_t)C && mu >= 8 * (Mpad / 64) * (size_t)C && L.r[SV_R].bytes >= 8 * (size_t)C, "%s chunk regions",
        tag);
  // a real workspace of exactly the reported size, the base `skew` bytes behind the caller's pointer
  if (reported <= ((size_t)8 << 20)) {
    const size_t lead = (256 - skew) % 256;
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, lead + reported) != 0) raw = nullptr;
    CHECK(raw != nullptr, "%s posix_memalign(%zu)", tag, lead + reported);
    if (!raw) return;
    char* ptr = static_cast<char*>(raw) + lead;
    const SvgpWorkspace w(ptr, L);
    CHECK(w.base == ptr + skew, "%s base %p for pointer %p", tag, (void*)w.base, (void*)ptr);
    auto fill = [&](int64_t t, int id) { return (int)(1 + (id + SV_REGIONS * t) % 250); };
    auto region = [&](int64_t t, int id) {
      return id < SV_SHARED ? w.task<unsigned char>(t, (SvgpRegion)id) : w.shared<unsigned char>((SvgpRegion)id);
    };
    for (int id = 0; id < SV_REGIONS; ++id)
      for (int64_t t = 0; t < (id < SV_SHARED ? ntask : 1); ++t) {
        CHECK((region(t, id) != nullptr) == (L.r[id].bytes != 0), "%s region %d: pointer and size disagree", tag, id);
        if (L.r[id].bytes) {
          CHECK(region(t, id) >= (unsigned char*)ptr && region(t, id) + L.r[id].bytes <= (unsigned char*)ptr + reported,
                "%s region %d outside the workspace", tag, id);
          std::memset(region(t, id), fill(t, id), L.r[id].bytes);
        }
      }
    for (int id = 0; id < SV_REGIONS; ++id)
      for (int64_t t = 0; t < (id < SV_SHARED ? ntask : 1); ++t)
        if (L.r[id].bytes) {
          const unsigned char* p = region(t, id);
          const size_t b = L.r[id].bytes;
          CHECK(p[0] == fill(t, id) && p[b - 1] == fill(t, id) && p[b / 2] == fill(t, id),
                "%s region %d of task %lld overwritten", tag, id, (long long)t);
        }
    std::free(raw);
  }
}

static void check_chunk_width(int64_t M, int64_t ntask, int64_t n, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128, n128 = (n + 127) / 128 * 128;
  const int64_t top = CHUNK_CAP < n128 ? CHUNK_CAP : n128;
  ++*count;
  auto size_of = [&](int64_t C) { return svgp_layout(SVGP_CONDITION, Mpad, ntask, C).total + 256; };
  // the downward loop, restated: the largest multiple of 128 up to `top` whose reported size fits
  auto loop = [&](size_t bytes) {
    for (int64_t C = top; C >= 128; C -= 128)
      if (size_of(C) <= bytes) return C;
    return (int64_t)0;
  };
  for (int64_t C = 128; C <= top; C += 128) {
    const size_t size = size_of(C);
    const int64_t below = svgp_chunk_width(SVGP_CONDITION, Mpad, ntask, n, CHUNK_CAP, size - 1);
    const int64_t at = svgp_chunk_width(SVGP_CONDITION, Mpad, ntask, n, CHUNK_CAP, size);
    CHECK(at == loop(size) && below == loop(size - 1) && at >= C && below < C,
          "M=%lld ntask=%lld n=%lld C=%lld: widths %lld / %lld around its size, the loop's %lld / %lld", (long long)M,
          (long long)ntask, (long long)n, (long long)C, (long long)below, (long long)at, (long long)loop(size - 1),
          (long long)loop(size));
  }
  CHECK(svgp_chunk_width(SVGP_CONDITION, Mpad, ntask, n, CHUNK_CAP, size_of(128) - 1) == 0, "below the chunk = 128 size");
  CHECK(svgp_chunk_width(SVGP_CONDITION, Mpad, ntask, n, CHUNK_CAP, ~(size_t)0) == top, "the cap");
}

int main() {
  const int64_t Ms[] = {1, 128, 129, 130, 200, 2048, 65536};
  const int64_t NTASK[] = {1, 3, 8, 64};
  const int64_t Cs[] = {128, 256, 384, 640, 4096, 16384, 1 << 20};
  const int64_t Ns[] = {1, 128, 129, 700, 100000};
  long count = 0;
  for (int64_t M : Ms)
    for (int64_t ntask : NTASK) {
      check_old(SVGP_PREPARE, M, ntask, 0, &count);
      for (int64_t C : Cs) {
        check_old(SVGP_FIT, M, ntask, C, &count);
        check_old(SVGP_GRAD, M, ntask, C, &count);
        check_old(SVGP_GRAD_Z, M, ntask, C, &count);
        for (size_t skew : {(size_t)0, (size_t)248}) check_cond(M, ntask, C, skew, &count);
      }
      for (int64_t n : Ns) check_chunk_width(M, ntask, n, &count);
    }
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  for (auto c : {std::initializer_list<int64_t>{130, 1, 128}, {200, 3, 256}, {2048, 8, 4096}}) {
    const int64_t* v = c.begin();
    std::printf("size %lld %lld %lld %zu\n", (long long)v[0], (long long)v[1], (long long)v[2],
                svgp_layout(SVGP_CONDITION, (v[0] + 127) / 128 * 128, v[1], v[2]).total + 256);
  }
  return failures ? 1 : 0;
}
