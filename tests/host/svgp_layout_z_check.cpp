// Stand-alone check of the workspace layout of gpx_svgp_bound_grad_z_f64 (the kind SVGP_GRAD_Z of
// bayesianoptimizer_amd/csrc/gpx_svgp_layout.h, the only project header included).  Built and run by
// tests/test_svgp_zgrad_layout.py, with the host compiler's address and undefined-behaviour sanitizers where they are
// installed.  Over a grid of (M, ntask, chunk width), with the caller's pointer 256-aligned and 8 bytes past an aligned
// address, it checks that
//  - the new kind's regions are pairwise disjoint, 256-aligned and inside [pointer, pointer + reported size), by
//    arithmetic and, for workspaces up to 8 MiB, by filling every region of a real allocation of exactly the reported
//    size through SvgpWorkspace's pointers and reading the fills back;
//  - on every region the gradient's layout has, the new kind equals it (same bytes, same offset in the task's block
//    resp. from the start of the shared part), and its two own regions hold what the launches write;
//  - the three older kinds equal a closed form recomputed here, and leave the two new regions out;
//  - a workspace of the size either gradient kind reports for a chunk width gives both kinds the same chunk width;
//  - svgp_chunk_width of the new kind refuses a workspace one byte below the chunk = 128 size and allows that size.
// Its last lines print the reported bytes of the cases pinned by tests/golden/svgp_z_workspace_sizes.json.
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
  *task = 2 * mat + D + up(tr) + 3 * vec + 256;
  if (kind == SVGP_GRAD) *task += 3 * mat + 2 * vec + 512 + up(8 * NOUT) + 256;
  const size_t ldk = (C + 255) / 256 * 256, pt = up(8 * Mpad * ldk);
  *total = *task * T + vec + up(4 * T) + (1 + T) * pt + up(8 * (Mpad / 64) * ldk) + up(8 * ldk);
  if (kind == SVGP_GRAD) {
    const size_t nI = Mpad / 128, ncb = C / 128;
    *total += up(8 * ldk) + up(8 * nI * max2(nI, ncb) * NOUT);
  }
}

static void check_old(SvgpKind kind, int64_t M, int64_t ntask, int64_t C, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128;
  const SvgpLayout L = svgp_layout(kind, Mpad, ntask, C, NOUT);
  size_t task, total;
  closed_form(kind, (size_t)Mpad, (size_t)ntask, (size_t)C, &task, &total);
  ++*count;
  CHECK(L.task == task && L.total == total, "kind=%d M=%lld ntask=%lld C=%lld: pitch %zu total %zu, closed form %zu %zu",
        (int)kind, (long long)M, (long long)ntask, (long long)C, L.task, L.total, task, total);
  CHECK(L.r[SV_ZACC].bytes == 0 && L.r[SV_ZPART].bytes == 0, "kind=%d has the inducing-location gradient's regions",
        (int)kind);
  // a zdim given to an older kind changes nothing
  const SvgpLayout Lz = svgp_layout(kind, Mpad, ntask, C, NOUT, ZDIM);
  CHECK(Lz.task == L.task && Lz.total == L.total, "kind=%d: zdim changes the layout", (int)kind);
}

static void check_z(int64_t M, int64_t ntask, int64_t C, size_t skew, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128;
  const SvgpLayout L = svgp_layout(SVGP_GRAD_Z, Mpad, ntask, C, NOUT, ZDIM);
  const SvgpLayout Gr = svgp_layout(SVGP_GRAD, Mpad, ntask, C, NOUT);
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
      prev_end = L.task * (size_t)ntask;
    }
    const SvgpLayout::Region& r = L.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 256 == 0, "%s region %d at %zu not 256-aligned", tag, id, r.at);
    prev_end = r.at + r.bytes;
  }
  CHECK(prev_end <= L.total && skew + L.total <= reported, "%s regions end at %zu of %zu", tag, prev_end, L.total);
  // the gradient inside: every region it has, at the same place
  for (int id = 0; id < SV_REGIONS; ++id) {
    if (!Gr.r[id].bytes) continue;
    const size_t g0 = id < SV_SHARED ? 0 : Gr.task * (size_t)ntask, z0 = id < SV_SHARED ? 0 : L.task * (size_t)ntask;
    CHECK(L.r[id].bytes == Gr.r[id].bytes && L.r[id].at - z0 == Gr.r[id].at - g0, "%s gradient region %d moved", tag, id);
  }
  CHECK(L.acc.at == Gr.acc.at && L.acc.bytes == Gr.acc.bytes && L.acc2.at == Gr.acc2.at &&
            L.acc2.bytes == Gr.acc2.bytes && L.ldk == Gr.ldk && L.phi_task == Gr.phi_task,
        "%s clear spans / pitches differ from the gradient's", tag);
  // the two new regions: the accumulator of dF/dZ behind the gradient's block, the row partials behind its shared part
  const size_t nI = (size_t)Mpad / 128, ncb = (size_t)C / 128;
  CHECK(L.r[SV_ZACC].at == Gr.task && L.r[SV_ZACC].bytes == up((size_t)Mpad * ZDIM * 8) &&
            L.task == Gr.task + L.r[SV_ZACC].bytes, "%s accumulator: at %zu, %zu bytes, pitch %zu", tag, L.r[SV_ZACC].at,
        L.r[SV_ZACC].bytes, L.task);
  CHECK(L.r[SV_ZPART].bytes == up(nI * max2(nI, ncb) * 128 * ZDIM * 8) &&
            L.r[SV_ZPART].bytes >= nI * ncb * 128 * ZDIM * 8 &&
            L.r[SV_ZPART].at - L.task * (size_t)ntask == Gr.total - Gr.task * (size_t)ntask &&
            L.total == L.r[SV_ZPART].at + L.r[SV_ZPART].bytes, "%s row partials: at %zu, %zu bytes", tag,
        L.r[SV_ZPART].at, L.r[SV_ZPART].bytes);
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
        if (L.r[id].bytes) std::memset(region(t, id), fill(t, id), L.r[id].bytes);
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
  for (int64_t C = 128; C <= top; C += 128) {
    const size_t size = svgp_layout(SVGP_GRAD_Z, Mpad, ntask, C, NOUT, ZDIM).total + 256;
    const int64_t below = svgp_chunk_width(SVGP_GRAD_Z, Mpad, ntask, n, CHUNK_CAP, size - 1, NOUT, ZDIM);
    const int64_t at = svgp_chunk_width(SVGP_GRAD_Z, Mpad, ntask, n, CHUNK_CAP, size, NOUT, ZDIM);
    const size_t gsize = svgp_layout(SVGP_GRAD, Mpad, ntask, C, NOUT).total + 256;
    const int64_t gat = svgp_chunk_width(SVGP_GRAD, Mpad, ntask, n, CHUNK_CAP, gsize, NOUT);
    // (sizes can tie between neighbouring widths: the call runs the largest that fits, the same one for both kinds)
    CHECK(at >= C && at == gat && below < C,
          "M=%lld ntask=%lld n=%lld C=%lld: widths %lld / %lld around its size, %lld in the gradient's", (long long)M,
          (long long)ntask, (long long)n, (long long)C, (long long)below, (long long)at, (long long)gat);
  }
  CHECK(svgp_chunk_width(SVGP_GRAD_Z, Mpad, ntask, n, CHUNK_CAP, ~(size_t)0, NOUT, ZDIM) == top, "the cap");
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
        for (size_t skew : {(size_t)0, (size_t)248}) check_z(M, ntask, C, skew, &count);
      }
      for (int64_t n : Ns) check_chunk_width(M, ntask, n, &count);
    }
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  for (auto c : {std::initializer_list<int64_t>{130, 1, 128}, {200, 3, 256}, {2048, 8, 4096}}) {
    const int64_t* v = c.begin();
    std::printf("size %lld %lld %lld %zu\n", (long long)v[0], (long long)v[1], (long long)v[2],
                svgp_layout(SVGP_GRAD_Z, (v[0] + 127) / 128 * 128, v[1], v[2], NOUT, ZDIM).total + 256);
  }
  return failures ? 1 : 0;
}
