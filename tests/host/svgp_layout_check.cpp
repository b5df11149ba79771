// Stand-alone check of the SVGP calls' workspace layout (bayesianoptimizer_amd/csrc/gpx_svgp_layout.h, the only project
// header included).  Built and run by tests/test_svgp_workspace_sizes.py with the host compiler's address and
// undefined-behaviour sanitizers.  Over a grid of (M, ntask, chunk width, call), with the caller's pointer 256-aligned
// and 8 bytes past an aligned address, it checks that
//  - the regions of every task's block and the shared ones are pairwise disjoint and lie within
//    [pointer, pointer + reported size), by arithmetic and, for workspaces up to 8 MiB, by filling every region of a
//    real allocation of exactly the reported size through SvgpWorkspace's pointers and reading the fills back;
//  - every region is 256-aligned, and the task pitch a multiple of 256 (the batched launches take it in doubles);
//  - every offset, the task pitch and the total equal a second, closed-form statement of the layout: the formulas the
//    three calls had each for itself before this header;
//  - the two clear spans are exactly their members, contiguous and in order;
//  - the fit's regions lie at the same offsets in the gradient's layout (only the task pitch and what follows differ);
//  - the tasks' projected chunks stay inside their region, and the partial rows hold what one launch writes;
//  - svgp_chunk_width, for workspace sizes around every size boundary, equals a downward loop over the closed form.
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

static const int64_t NOUT = 72;        // GPX_MLL_NOUT (include/gpx.h)
static const int64_t CHUNK_CAP = 4096; // GPX_SVGP_FIT_CHUNK

static size_t up(size_t b) { return (b + 255) / 256 * 256; }
static size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// the second statement of the layout: offsets (per task: inside the task's block; shared: from the aligned base)
struct Closed {
  size_t at[SV_REGIONS], bytes[SV_REGIONS], task, total;
};
static Closed closed_form(SvgpKind kind, int64_t Mpad_, int64_t ntask, int64_t C_) {
  Closed c;
  std::memset(&c, 0, sizeof c);
  const size_t Mpad = (size_t)Mpad_, T = (size_t)ntask, C = (size_t)C_;
  const size_t mat = up(8 * Mpad * Mpad), vec = up(8 * Mpad), D = up(1024 * Mpad), tr = 2 * Mpad * Mpad + 256;
  if (kind == SVGP_PREPARE) {
    const size_t fs = up(max2(tr, (Mpad / 128 + 1) * Mpad * 8 + 512));
    c.at[SV_A] = 0, c.bytes[SV_A] = mat;
    c.at[SV_DINV] = mat, c.bytes[SV_DINV] = D;
    c.at[SV_SLICE] = mat + D, c.bytes[SV_SLICE] = fs;
    c.at[SV_SPAD] = mat + D + fs, c.bytes[SV_SPAD] = mat;
    c.at[SV_MPAD] = c.at[SV_SPAD] + mat, c.bytes[SV_MPAD] = vec;
    c.task = c.at[SV_MPAD] + vec;
    c.total = c.task * T;
    return c;
  }
  const bool grad = kind == SVGP_GRAD;
  // per task: the fit's block, and behind its scalars the gradient's tail
  c.at[SV_A] = 0, c.bytes[SV_A] = mat;
  c.at[SV_WB] = mat, c.bytes[SV_WB] = mat;
  c.at[SV_DINV] = 2 * mat, c.bytes[SV_DINV] = D;
  c.at[SV_SLICE] = 2 * mat + D, c.bytes[SV_SLICE] = up(tr);
  c.at[SV_BVEC] = c.at[SV_SLICE] + up(tr), c.bytes[SV_BVEC] = vec;
  c.at[SV_U] = c.at[SV_BVEC] + vec, c.bytes[SV_U] = vec;
  c.at[SV_MREV] = c.at[SV_BVEC] + 2 * vec, c.bytes[SV_MREV] = vec;
  c.at[SV_SCAL] = c.at[SV_BVEC] + 3 * vec, c.bytes[SV_SCAL] = 256;
  const size_t tail = c.at[SV_SCAL] + 256;
  c.task = tail;
  if (grad) {
    c.task += 3 * mat + 2 * vec + 512 + up(8 * NOUT) + 256;
    c.at[SV_WK] = tail, c.bytes[SV_WK] = mat;
    c.at[SV_BC] = tail + mat, c.bytes[SV_BC] = mat;
    c.at[SV_X1] = tail + 2 * mat, c.bytes[SV_X1] = mat;
    c.at[SV_CV] = tail + 3 * mat, c.bytes[SV_CV] = vec;
    c.at[SV_MNAT] = tail + 3 * mat + vec, c.bytes[SV_MNAT] = vec;
    c.at[SV_SC2] = tail + 3 * mat + 2 * vec, c.bytes[SV_SC2] = 512;
    c.at[SV_GACC] = c.at[SV_SC2] + 512, c.bytes[SV_GACC] = up(8 * NOUT);
    c.at[SV_BND] = c.at[SV_GACC] + up(8 * NOUT), c.bytes[SV_BND] = 256;
  }
  // shared: the fixed part, then the part that scales with the chunk width
  const size_t ldk = (C + 255) / 256 * 256, pt = up(8 * Mpad * ldk);
  c.at[SV_ZERO] = c.task * T, c.bytes[SV_ZERO] = vec;
  c.at[SV_INFO2] = c.at[SV_ZERO] + vec, c.bytes[SV_INFO2] = up(4 * T);
  c.at[SV_KC] = c.at[SV_INFO2] + up(4 * T), c.bytes[SV_KC] = pt;
  c.at[SV_PHI] = c.at[SV_KC] + pt, c.bytes[SV_PHI] = T * pt;
  c.at[SV_MU] = c.at[SV_PHI] + T * pt, c.bytes[SV_MU] = up(8 * (Mpad / 64) * ldk);
  c.at[SV_R] = c.at[SV_MU] + c.bytes[SV_MU], c.bytes[SV_R] = up(8 * ldk);
  c.total = c.task * T + vec + up(4 * T) + (1 + T) * pt + up(8 * (Mpad / 64) * ldk) + up(8 * ldk);
  if (grad) {
    const size_t nI = Mpad / 128, ncb = C / 128;
    c.at[SV_EV] = c.total, c.bytes[SV_EV] = up(8 * ldk);
    c.at[SV_PART] = c.total + up(8 * ldk), c.bytes[SV_PART] = up(8 * nI * max2(nI, ncb) * NOUT);
    c.total += up(8 * ldk) + up(8 * nI * max2(nI, ncb) * NOUT);
  }
  return c;
}

static void members(const SvgpLayout& L, const SvgpLayout::Region& span, std::initializer_list<SvgpRegion> ids,
                    const char* tag, const char* name) {
  size_t at = span.at;
  for (SvgpRegion id : ids) {
    CHECK(L.r[id].bytes > 0 && L.r[id].at == at, "%s span %s: member %d at %zu, expected %zu", tag, name, (int)id,
          L.r[id].at, at);
    at += L.r[id].bytes;
  }
  CHECK(at == span.at + span.bytes, "%s span %s ends at %zu, its members at %zu", tag, name, span.at + span.bytes, at);
}

static void check(SvgpKind kind, int64_t M, int64_t ntask, int64_t C, size_t skew, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128;
  const SvgpLayout L = svgp_layout(kind, Mpad, ntask, C, NOUT);
  const size_t reported = L.total + 256;
  char tag[128];
  std::snprintf(tag, sizeof tag, "kind=%d M=%lld ntask=%lld C=%lld skew=%zu:", (int)kind, (long long)M,
                (long long)ntask, (long long)C, skew);
  ++*count;
  // the second statement
  const Closed c = closed_form(kind, Mpad, ntask, C);
  for (int id = 0; id < SV_REGIONS; ++id) {
    CHECK(L.r[id].bytes == c.bytes[id], "%s region %d: %zu bytes, closed form %zu", tag, id, L.r[id].bytes, c.bytes[id]);
    if (c.bytes[id]) CHECK(L.r[id].at == c.at[id], "%s region %d at %zu, closed form %zu", tag, id, L.r[id].at, c.at[id]);
  }
  CHECK(L.task == c.task, "%s task pitch %zu, closed form %zu", tag, L.task, c.task);
  CHECK(L.total == c.total, "%s total %zu, closed form %zu", tag, L.total, c.total);
  CHECK(L.task % 256 == 0 && L.task > 0, "%s task pitch %zu", tag, L.task);
  // disjoint (the regions are in the order of their ids), aligned, inside the block resp. the reported bytes
  size_t prev_end = 0;
  for (int id = 0; id < SV_REGIONS; ++id) {
    if (id == SV_SHARED) {
      CHECK(prev_end <= L.task, "%s the task's regions end at %zu of %zu", tag, prev_end, L.task);
      prev_end = L.task * (size_t)ntask;  // the last task's block ends here
    }
    const SvgpLayout::Region& r = L.r[id];
    if (!r.bytes) continue;
    CHECK(r.at >= prev_end, "%s region %d at %zu overlaps the one before it (ends %zu)", tag, id, r.at, prev_end);
    CHECK(r.at % 256 == 0, "%s region %d at %zu not 256-aligned", tag, id, r.at);
    prev_end = r.at + r.bytes;
  }
  CHECK(prev_end <= L.total && skew + L.total <= reported, "%s regions end at %zu of %zu", tag, prev_end, L.total);
  // the clear spans
  if (kind == SVGP_PREPARE) {
    CHECK(L.acc.bytes == 0 && L.acc2.bytes == 0, "%s prepare has no clear spans", tag);
  } else {
    members(L, L.acc, {SV_BVEC, SV_U, SV_MREV, SV_SCAL}, tag, "acc");
    if (kind == SVGP_GRAD) {
      members(L, L.acc2, {SV_SC2, SV_GACC}, tag, "acc2");
      CHECK(L.r[SV_BND].at == L.acc2.at + L.acc2.bytes, "%s the bound's values follow acc2", tag);
    } else {
      CHECK(L.acc2.bytes == 0, "%s the fit has no second span", tag);
    }
    // chunk-width regions
    CHECK(L.ldk >= C && L.ldk % 256 == 0 && L.ldk < C + 256, "%s ldk %lld", tag, (long long)L.ldk);
    CHECK(L.phi_task % 8 == 0 && L.phi_task >= (size_t)Mpad * L.ldk * 8 &&
              L.phi_task * (size_t)ntask <= L.r[SV_PHI].bytes && L.r[SV_KC].bytes >= (size_t)Mpad * L.ldk * 8,
          "%s projected chunks: pitch %zu x %lld tasks in %zu bytes", tag, L.phi_task, (long long)ntask,
          L.r[SV_PHI].bytes);
    CHECK(L.r[SV_ZERO].bytes >= (size_t)Mpad * 8 && L.r[SV_INFO2].bytes >= (size_t)ntask * 4, "%s zero / info2", tag);
  }
  if (kind == SVGP_GRAD) {
    const size_t nI = (size_t)Mpad / 128, ncb = (size_t)C / 128;
    CHECK(L.r[SV_PART].bytes == up(nI * max2(nI, ncb) * NOUT * 8), "%s partial rows: %zu bytes", tag, L.r[SV_PART].bytes);
    CHECK(L.r[SV_EV].bytes >= (size_t)L.ldk * 8, "%s residual e", tag);
    // the fit inside the gradient: same offsets in the task's block, same offsets from the start of the shared part
    const SvgpLayout F = svgp_layout(SVGP_FIT, Mpad, ntask, C, NOUT);
    for (int id = 0; id < SV_REGIONS; ++id) {
      if (!F.r[id].bytes) continue;
      const size_t f0 = id < SV_SHARED ? 0 : F.task * (size_t)ntask, g0 = id < SV_SHARED ? 0 : L.task * (size_t)ntask;
      CHECK(L.r[id].bytes == F.r[id].bytes && L.r[id].at - g0 == F.r[id].at - f0, "%s fit region %d moved", tag, id);
    }
    CHECK(F.acc.at == L.acc.at && F.acc.bytes == L.acc.bytes && F.ldk == L.ldk && F.phi_task == L.phi_task &&
              F.task < L.task, "%s fit spans / pitches", tag);
    for (int id = SV_WK; id <= SV_BND; ++id) CHECK(F.r[id].bytes == 0, "%s the fit has region %d", tag, id);
    CHECK(F.r[SV_EV].bytes == 0 && F.r[SV_PART].bytes == 0, "%s the fit has gradient regions", tag);
  }
  // a real workspace of exactly the reported size, the base `skew` bytes behind the caller's pointer: fill every region
  // of every task through the carve, read the fills back (the sanitizer guards the allocation's end to the byte)
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
    if (L.acc.bytes) CHECK(w.task<char>(1 % ntask, L.acc) == w.task<char>(1 % ntask, SV_BVEC), "%s acc pointer", tag);
    if (L.acc2.bytes) CHECK(w.task<char>(0, L.acc2) == w.task<char>(0, SV_SC2), "%s acc2 pointer", tag);
    CHECK(w.pitch() * 8 == (int64_t)L.task && w.phi_pitch() * 8 == (int64_t)L.phi_task, "%s pitches", tag);
    std::free(raw);
  }
}

// svgp_chunk_width against a downward loop over the closed form, for workspace sizes around every size boundary
static void check_chunk_width(SvgpKind kind, int64_t M, int64_t ntask, int64_t n, long* count) {
  const int64_t Mpad = (M + 127) / 128 * 128, n128 = (n + 127) / 128 * 128;
  const int64_t top = CHUNK_CAP < n128 ? CHUNK_CAP : n128;
  auto brute = [&](size_t ws_bytes) {
    for (int64_t C = top; C >= 128; C -= 128)
      if (closed_form(kind, Mpad, ntask, C).total + 256 <= ws_bytes) return C;
    return (int64_t)0;
  };
  auto same = [&](size_t ws_bytes) {
    const int64_t got = svgp_chunk_width(kind, Mpad, ntask, n, CHUNK_CAP, ws_bytes, NOUT), want = brute(ws_bytes);
    CHECK(got == want, "kind=%d M=%lld ntask=%lld n=%lld ws_bytes=%zu: chunk width %lld, downward loop %lld", (int)kind,
          (long long)M, (long long)ntask, (long long)n, ws_bytes, (long long)got, (long long)want);
    return got;
  };
  ++*count;
  for (int64_t C = 128; C <= top; C += 128) {
    const size_t size = closed_form(kind, Mpad, ntask, C).total + 256;
    same(size - 1);
    CHECK(same(size) >= C, "kind=%d M=%lld ntask=%lld n=%lld: the size of C=%lld does not allow it", (int)kind,
          (long long)M, (long long)ntask, (long long)n, (long long)C);
    same(size + 1);
  }
  CHECK(same(closed_form(kind, Mpad, ntask, 128).total + 255) == 0 && same(0) == 0 && same(256) == 0,
        "kind=%d M=%lld ntask=%lld n=%lld: a chunk width below the size of 128", (int)kind, (long long)M,
        (long long)ntask, (long long)n);
  CHECK(same(~(size_t)0) == top, "kind=%d M=%lld ntask=%lld n=%lld: the cap", (int)kind, (long long)M, (long long)ntask,
        (long long)n);
}

int main() {
  const int64_t Ms[] = {1, 64, 128, 129, 130, 200, 2048, 65536};
  const int64_t NTASK[] = {1, 3, 8, 64};
  const int64_t Cs[] = {128, 256, 384, 640, 4096, 16384, 1 << 20};
  const int64_t Ns[] = {1, 127, 128, 129, 700, 100000};
  long count = 0;
  for (size_t skew : {(size_t)0, (size_t)248})  // the pointer aligned, and 8 bytes past an aligned address
    for (int64_t M : Ms)
      for (int64_t ntask : NTASK) {
        check(SVGP_PREPARE, M, ntask, 0, skew, &count);
        for (int64_t C : Cs) {
          check(SVGP_FIT, M, ntask, C, skew, &count);
          check(SVGP_GRAD, M, ntask, C, skew, &count);
        }
      }
  for (int64_t M : Ms)
    for (int64_t ntask : NTASK)
      for (int64_t n : Ns) {
        check_chunk_width(SVGP_FIT, M, ntask, n, &count);
        check_chunk_width(SVGP_GRAD, M, ntask, n, &count);
      }
  std::printf("%ld layouts checked, %ld failures\n", count, failures);
  return failures ? 1 : 0;
}
