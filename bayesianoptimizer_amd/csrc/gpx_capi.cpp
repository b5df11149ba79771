// The C ABI of libgpx.so (include/gpx.h): argument validation, workspace carving, chunk loop and timers.
// Every exported symbol is extern "C" with plain pointers; no torch types cross this boundary.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <utility>
#include "gpx_internal.h"

using gpx::Context;

namespace {

// GPX_SOURCE_SHA256: sha256 over csrc/* and include/gpx.h (the Makefile stamps it; tests/test_capi.py recomputes it from
// the working tree, so a stale or foreign libgpx.so is caught)
#ifndef GPX_SOURCE_SHA256
#define GPX_SOURCE_SHA256 "unstamped"
#endif
constexpr const char* kVersion = "gpx 0.5.0 (gfx950, fp64 MFMA) src " GPX_SOURCE_SHA256;

gpx_status fail(Context* c, gpx_status st, const std::string& msg) {
  if (c) c->last_error = msg;
  return st;
}

gpx_status hip_check(Context* c, hipError_t e, const char* where) {
  if (e == hipSuccess) return GPX_OK;
  return fail(c, GPX_HIP_ERROR, std::string(where) + ": " + hipGetErrorString(e));
}


int64_t padded(int64_t n) { return ((n + GPX_TILE - 1) / GPX_TILE) * GPX_TILE; }

gpx_status check_params(Context* c, const gpx_kernel_params* p) {
  if (!p) return fail(c, GPX_INVALID_ARG, "kernel params pointer is NULL");
  if (p->kind < GPX_KERNEL_RBF || p->kind > GPX_KERNEL_SCALE_LINEAR_MATERN52)
    return fail(c, GPX_INVALID_ARG, "unknown kernel kind " + std::to_string(p->kind));
  if (p->d < 1 || p->d > GPX_MAX_DIM)
    return fail(c, GPX_INVALID_ARG, "input dimension d=" + std::to_string(p->d) + " outside [1, 32]");
  for (int k = 0; k < p->d; ++k)
    if (!(p->lengthscale[k] > 0.0) || !std::isfinite(p->lengthscale[k]))
      return fail(c, GPX_INVALID_ARG, "lengthscale[" + std::to_string(k) + "] must be positive and finite");
  if (!(p->outputscale >= 0.0) || !(p->noise >= 0.0) || !(p->jitter >= 0.0))
    return fail(c, GPX_INVALID_ARG, "outputscale/noise/jitter must be non-negative");
  // The trailing int32 pair is part of the contract: a caller whose struct definition stops before it (552 instead of
  // gpx_kernel_params_size() bytes) would hand over whatever follows its struct in memory, and a stray non-zero
  // cov_fp32 would silently switch the covariance build to fp32.  Anything but {0, 1} / 0 is rejected.
  if (p->cov_fp32 != 0 && p->cov_fp32 != 1)
    return fail(c, GPX_INVALID_ARG, "cov_fp32 must be 0 or 1 (got " + std::to_string(p->cov_fp32) +
                                        "; is the caller's gpx_kernel_params " + std::to_string(sizeof(gpx_kernel_params)) +
                                        " bytes?)");
  if (p->reserved != 0) return fail(c, GPX_INVALID_ARG, "gpx_kernel_params.reserved must be 0");
  return GPX_OK;
}

gpx_status check_n(Context* c, int64_t n) {
  if (n < 1 || n > (int64_t)1 << 20) return fail(c, GPX_INVALID_ARG, "n must be in [1, 2^20]");
  return GPX_OK;
}

gpx_status check_ld(Context* c, int64_t ld, int64_t minimum, const char* name, bool even) {
  if (ld < minimum) return fail(c, GPX_INVALID_ARG, std::string(name) + " leading dimension too small");
  if (even && (ld & 1)) return fail(c, GPX_INVALID_ARG, std::string(name) + " leading dimension must be even");
  // the matrix kernels address 128-row tiles through buffer descriptors with 32-bit byte offsets
  if (even && ld > GPX_MAX_LD)
    return fail(c, GPX_INVALID_ARG, std::string(name) + " leading dimension above GPX_MAX_LD (2^20)");
  return GPX_OK;
}

#define GPX_TRY(expr)               \
  do {                              \
    gpx_status _st = (expr);        \
    if (_st != GPX_OK) return _st;  \
  } while (0)

// Makes the handle's device current for the rest of the calling entry point and restores the caller's device on return.
#define GPX_USE_DEVICE(c)                                  \
  gpx::DeviceScope _gpx_dev((c)->device);                  \
  if (_gpx_dev.err != hipSuccess) return hip_check((c), _gpx_dev.err, "hipSetDevice")

#define GPX_NONNULL(c, ptr) \
  do { if (!(ptr)) return fail((c), GPX_INVALID_ARG, #ptr " is NULL"); } while (0)

using gpx::alpha_ws;  // (gpx_svgp_layout.h)
using gpx::trtri_ws;

double* align256(void* p) {
  uintptr_t u = reinterpret_cast<uintptr_t>(p);
  u = (u + 255) & ~(uintptr_t)255;
  return reinterpret_cast<double*>(u);
}

}  // namespace

namespace gpx {

LaunchTimer::LaunchTimer(Context* ctx, int t) : c(ctx), timer(t) {
  if (!(c->timing_mask & (1 << t))) return;
  auto take = [&]() {
    hipEvent_t ev;
    if (!c->free_events.empty()) {
      ev = c->free_events.back();
      c->free_events.pop_back();
    } else if (hipEventCreate(&ev) != hipSuccess) {
      return (hipEvent_t) nullptr;
    }
    return ev;
  };
  s = take();
  e = take();
  if (s) (void)hipEventRecord(s, c->stream);
}

LaunchTimer::~LaunchTimer() {
  if (!s || !e) return;
  (void)hipEventRecord(e, c->stream);
  c->pending.push_back({timer, s, e});
}

}  // namespace gpx

extern "C" {

const char* gpx_version(void) { return kVersion; }

int64_t gpx_padded_n(int64_t n) { return padded(n); }

size_t gpx_kernel_params_size(void) { return sizeof(gpx_kernel_params); }

size_t gpx_acq_params_size(void) { return sizeof(gpx_acq_params); }

static void apply_env_options(Context* c);

gpx_status gpx_create(int32_t device, gpx_handle* out) {
  if (!out) return GPX_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return GPX_HIP_ERROR;
  if (device < 0 || device >= count) return GPX_INVALID_ARG;
  Context* c = new (std::nothrow) Context();
  if (!c) return GPX_HIP_ERROR;
  c->device = device;
  apply_env_options(c);
  {
    gpx::DeviceScope dev(device);  // the device must be selectable; the caller's current device is left as it was
    if (dev.err != hipSuccess) {
      delete c;
      return GPX_HIP_ERROR;
    }
    // the pruned sweep's read-back of a span's survivor count (launch_sweep_super_pruned): a pinned word and an event
    void* word = nullptr;
    if (hipHostMalloc(&word, 64, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&c->tail_event, hipEventDisableTiming) != hipSuccess) {
      if (word) (void)hipHostFree(word);
      delete c;
      return GPX_HIP_ERROR;
    }
    c->tail_count = static_cast<int32_t*>(word);
    *c->tail_count = 0;
  }
  *out = reinterpret_cast<gpx_handle>(c);
  return GPX_OK;
}

gpx_status gpx_destroy(gpx_handle h) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  (void)hipStreamSynchronize(c->stream);
  for (auto& pt : c->pending) {
    (void)hipEventDestroy(pt.start);
    (void)hipEventDestroy(pt.stop);
  }
  for (auto ev : c->free_events) (void)hipEventDestroy(ev);
  if (c->tail_event) (void)hipEventDestroy(c->tail_event);
  if (c->tail_count) (void)hipHostFree(c->tail_count);
  delete c;
  return GPX_OK;
}

gpx_status gpx_set_stream(gpx_handle h, void* stream) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  c->stream = reinterpret_cast<hipStream_t>(stream);
  return GPX_OK;
}

static gpx_status set_option(Context* c, int32_t option, int64_t v) {
  switch (option) {
    case GPX_OPT_SPIN_LIMIT:
      if (v < 0 || v > 0x7fffffff) return fail(c, GPX_INVALID_ARG, "spin_limit must be in [0, 2^31)");
      c->spin_limit = (unsigned)v;
      return GPX_OK;
    case GPX_OPT_SWEEP_FUSED:
      if (v != 0 && v != 1) return fail(c, GPX_INVALID_ARG, "sweep_fused must be 0 or 1");
      c->sweep_fused = (int)v;
      return GPX_OK;
    case GPX_OPT_GRAM_SPLIT:
      if (v != 0 && v != 1 && v != 2 && v != 4) return fail(c, GPX_INVALID_ARG, "gram_split must be 0, 1, 2 or 4");
      c->gram_split = (int)v;
      return GPX_OK;
    case GPX_OPT_POTRF_LAZY:
      if (v < 0 || v > 16) return fail(c, GPX_INVALID_ARG, "potrf_lazy must be in [0, 16]");
      c->potrf_lazy = (int)v;
      return GPX_OK;
    case GPX_OPT_POTRF_MODE:
      if (v < -1 || v > 1) return fail(c, GPX_INVALID_ARG, "potrf_mode must be -1, 0 or 1");
      c->potrf_mode = (int)v;
      return GPX_OK;
    case GPX_OPT_POTRF_SWITCH:
      if (v < -1 || v > 16384) return fail(c, GPX_INVALID_ARG, "potrf_switch must be in [-1, 16384]");
      c->potrf_switch = (int)v;
      return GPX_OK;
    case GPX_OPT_POTRF_SPLIT:
      if (v != -1 && v != 1 && v != 3) return fail(c, GPX_INVALID_ARG, "potrf_split must be -1, 1 or 3");
      c->potrf_split = (int)v;
      return GPX_OK;
    case GPX_OPT_SWEEP_PRUNE:
      if (v != -2 && (v < 0 || v > 2)) return fail(c, GPX_INVALID_ARG, "sweep_prune must be 0, 1, 2 or -2");
      c->sweep_prune = (int)v;
      return GPX_OK;
    default:
      return fail(c, GPX_INVALID_ARG, "unknown option " + std::to_string(option));
  }
}

static int option_by_name(const std::string& name) {
  // index = GPX_OPT_* number; slot 0 is reserved (the removed potrf_schedule) and has no name
  static const char* names[GPX_OPT_COUNT] = {"", "spin_limit", "sweep_fused", "gram_split", "potrf_lazy", "potrf_mode",
                                               "potrf_switch", "potrf_split", "sweep_prune"};
  for (int i = 1; i < GPX_OPT_COUNT; ++i)
    if (name == names[i]) return i;
  return -1;
}

// GPX_OPTIONS="name=value,...": the library's only read of the environment (tuning / A-B tools)
static void apply_env_options(Context* c) {
  const char* e = std::getenv("GPX_OPTIONS");
  if (!e) return;
  std::string all(e);
  size_t pos = 0;
  while (pos < all.size()) {
    size_t end = all.find(',', pos);
    if (end == std::string::npos) end = all.size();
    const std::string item = all.substr(pos, end - pos);
    const size_t eq = item.find('=');
    if (eq != std::string::npos) {
      const int opt = option_by_name(item.substr(0, eq));
      if (opt >= 0) {
        if (set_option(c, opt, std::atoll(item.c_str() + eq + 1)) != GPX_OK)
          std::fprintf(stderr, "gpx: GPX_OPTIONS: %s (ignored)\n", c->last_error.c_str());
      } else {
        std::fprintf(stderr, "gpx: GPX_OPTIONS: unknown option '%s' (ignored)\n", item.substr(0, eq).c_str());
      }
    } else if (!item.empty()) {
      std::fprintf(stderr, "gpx: GPX_OPTIONS: '%s' is not name=value (ignored)\n", item.c_str());
    }
    pos = end + 1;
  }
  c->last_error.clear();
}

gpx_status gpx_set_option(gpx_handle h, int32_t option, int64_t value) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  return set_option(c, option, value);
}

gpx_status gpx_get_option(gpx_handle h, int32_t option, int64_t* value_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, value_host);
  switch (option) {
    case GPX_OPT_SPIN_LIMIT: *value_host = c->spin_limit; return GPX_OK;
    case GPX_OPT_SWEEP_FUSED: *value_host = c->sweep_fused; return GPX_OK;
    case GPX_OPT_GRAM_SPLIT: *value_host = c->gram_split; return GPX_OK;
    case GPX_OPT_POTRF_LAZY: *value_host = c->potrf_lazy; return GPX_OK;
    case GPX_OPT_POTRF_MODE: *value_host = c->potrf_mode; return GPX_OK;
    case GPX_OPT_POTRF_SWITCH: *value_host = c->potrf_switch; return GPX_OK;
    case GPX_OPT_POTRF_SPLIT: *value_host = c->potrf_split; return GPX_OK;
    case GPX_OPT_SWEEP_PRUNE: *value_host = c->sweep_prune; return GPX_OK;
    default: return fail(c, GPX_INVALID_ARG, "unknown option " + std::to_string(option));
  }
}

const char* gpx_last_error(gpx_handle h) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return "invalid handle";
  return c->last_error.c_str();
}

// gram_impl clears *info (when given) inside the gram kernel: the fit needs no separate memset dispatch
static gpx_status gram_impl(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                            double* K, int64_t ldk, int32_t* info, void* zero = nullptr, size_t zero_bytes = 0) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, K);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldk, npad, "K", true));
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_gram(c, *p, (int)n, (int)npad, X, ldx, K, ldk, gpx::Batch(), 0, info, zero, zero_bytes),
                   "gram");
}

gpx_status gpx_gram_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                        double* K, int64_t ldk) {
  return gram_impl(h, p, n, X, ldx, K, ldk, nullptr);
}

static gpx_status potrf_impl(gpx_handle h, int64_t n, double* A, int64_t lda, double* Dinv, int32_t* info,
                             bool clear_info, double* W = nullptr, int64_t ldw = 0,
                             const gpx::ForwardRhs* fr = nullptr, bool* z_done = nullptr) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, A);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, info);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, lda, npad, "A", true));
  GPX_USE_DEVICE(c);
  if (clear_info) GPX_TRY(hip_check(c, hipMemsetAsync(info, 0, sizeof(int32_t), c->stream), "memset info"));
  return hip_check(c, gpx::launch_potrf(c, (int)npad, A, lda, Dinv, info, gpx::Batch(), W, ldw, fr, z_done), "potrf");
}

gpx_status gpx_potrf_f64(gpx_handle h, int64_t n, double* A, int64_t lda, double* Dinv, int32_t* info) {
  return potrf_impl(h, n, A, lda, Dinv, info, true);
}

gpx_status gpx_trtri_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 1) return GPX_INVALID_ARG;
  *bytes = trtri_ws(padded(n));
  return GPX_OK;
}

static gpx_status trtri_impl(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv, double* W,
                             int64_t ldw, void* ws, size_t ws_bytes, bool diag_done) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldl, npad, "L", true));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  if (ws_bytes < trtri_ws(npad)) return fail(c, GPX_INVALID_ARG, "trtri workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_trtri(c, (int)npad, L, ldl, Dinv, W, ldw, align256(ws), gpx::Batch(), diag_done),
                   "trtri");
}

gpx_status gpx_trtri_f64(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv, double* W,
                         int64_t ldw, void* ws, size_t ws_bytes) {
  return trtri_impl(h, n, L, ldl, Dinv, W, ldw, ws, ws_bytes, false);
}

gpx_status gpx_trtri_batched_workspace_size(int64_t n, int64_t batch, size_t* bytes) {
  if (!bytes || n < 1 || batch < 1 || batch > 65535) return GPX_INVALID_ARG;
  *bytes = ((trtri_ws(padded(n)) + 255) & ~(size_t)255) * (size_t)batch + 256;
  return GPX_OK;
}

gpx_status gpx_trtri_batched_f64(gpx_handle h, int64_t batch, int64_t n, const double* L, int64_t ldl, int64_t stride_l,
                                 const double* Dinv, int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w,
                                 void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  if (batch < 1 || batch > 65535) return fail(c, GPX_INVALID_ARG, "batch must be in [1, 65535]");
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldl, npad, "L", true));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  if (batch > 1) {
    if (stride_l < npad * ldl || stride_w < npad * ldw || stride_dinv < 2 * (npad / gpx::NB) * gpx::NB * gpx::NB)
      return fail(c, GPX_INVALID_ARG, "batch strides smaller than one problem");
    if ((stride_l | stride_w | stride_dinv) & 1) return fail(c, GPX_INVALID_ARG, "L/W/Dinv strides must be even");
  }
  size_t need = 0;
  GPX_TRY(gpx_trtri_batched_workspace_size(n, batch, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "batched trtri workspace too small");
  GPX_USE_DEVICE(c);
  gpx::Batch bt;
  bt.count = (int)batch;
  bt.k = stride_l;
  bt.dinv = stride_dinv;
  bt.w = stride_w;
  bt.ws = (int64_t)(((trtri_ws(npad) + 255) & ~(size_t)255) / sizeof(double));
  return hip_check(c, gpx::launch_trtri(c, (int)npad, L, ldl, Dinv, W, ldw, align256(ws), bt, false), "trtri");
}

gpx_status gpx_alpha_workspace_size(int64_t n, int64_t nrhs, size_t* bytes) {
  if (!bytes || n < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS) return GPX_INVALID_ARG;
  *bytes = alpha_ws(padded(n), nrhs);
  return GPX_OK;
}

gpx_status gpx_alpha_f64(gpx_handle h, int64_t n, const double* W, int64_t ldw, const double* Y, int64_t ldy,
                         int64_t nrhs, double const_mean, double* alpha, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  if (ws_bytes < alpha_ws(npad, nrhs)) return fail(c, GPX_INVALID_ARG, "alpha workspace too small");
  GPX_USE_DEVICE(c);
  double* zpart = align256(ws);
  double* z = zpart + (size_t)(npad / 128) * npad * nrhs;
  return hip_check(c, gpx::launch_alpha(c, (int)n, (int)npad, W, ldw, Y, ldy, (int)nrhs, const_mean, alpha, zpart, z),
                   "alpha");
}

gpx_status gpx_fit_workspace_size(int64_t n, int64_t nrhs, size_t* bytes) {
  if (!bytes || n < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS) return GPX_INVALID_ARG;
  const int64_t npad = padded(n);
  size_t a = trtri_ws(npad), b = alpha_ws(npad, nrhs);
  *bytes = a > b ? a : b;
  return GPX_OK;
}

gpx_status gpx_fit_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                       const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv, double* W,
                       int64_t ldw, double* alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  size_t need = 0;
  if (gpx_fit_workspace_size(n, nrhs, &need) != GPX_OK)
    return fail(c, GPX_INVALID_ARG, "invalid n / nrhs for fit");
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "fit workspace too small");
  if (!info) return fail(c, GPX_INVALID_ARG, "info is NULL");
  GPX_TRY(gram_impl(h, p, n, X, ldx, K, ldk, info));
  if (!W) return fail(c, GPX_INVALID_ARG, "W is NULL");
  // W's leading dimension is validated before the Dinv pass writes W's diagonal blocks
  GPX_TRY(check_ld(c, ldw, padded(n), "W", true));
  GPX_TRY(potrf_impl(h, n, K, ldk, Dinv, info, false, W, ldw));
  GPX_TRY(trtri_impl(h, n, K, ldk, Dinv, W, ldw, ws, ws_bytes, true));
  return gpx_alpha_f64(h, n, W, ldw, Y, ldy, nrhs, p->const_mean, alpha, ws, ws_bytes);
}

gpx_status gpx_fit_f64_sync(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                            const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv,
                            double* W, int64_t ldw, double* alpha, int32_t* info, void* ws, size_t ws_bytes,
                            int32_t* info_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(gpx_fit_f64(h, p, n, X, ldx, Y, ldy, nrhs, K, ldk, Dinv, W, ldw, alpha, info, ws, ws_bytes));
  int32_t hinfo = 0;
  GPX_TRY(hip_check(c, hipMemcpyAsync(&hinfo, info, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream), "info D2H"));
  GPX_TRY(hip_check(c, hipStreamSynchronize(c->stream), "sync"));
  if (info_host) *info_host = hinfo;
  if (hinfo == GPX_INFO_TIMEOUT)
    return fail(c, GPX_TIMEOUT, "an in-launch hand-off of the factorisation timed out (spin limit)");
  if (hinfo != 0)
    return fail(c, GPX_NOT_PD, "Gram matrix not positive definite at pivot " + std::to_string(hinfo - 1));
  return GPX_OK;
}

gpx_status gpx_potrs_workspace_size(int64_t n, int64_t nrhs, size_t* bytes) {
  if (!bytes || n < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS) return GPX_INVALID_ARG;
  *bytes = gpx::potrs_workspace_bytes(padded(n), nrhs, 1) + 256;
  return GPX_OK;
}

static gpx_status potrs_impl(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv,
                             const double* Y, int64_t ldy, int64_t nrhs, double const_mean, double* alpha,
                             int32_t* info, void* ws, size_t ws_bytes, bool ws_cleared, const double* z = nullptr);

gpx_status gpx_potrs_f64(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv, const double* Y,
                         int64_t ldy, int64_t nrhs, double const_mean, double* alpha, int32_t* info, void* ws,
                         size_t ws_bytes) {
  return potrs_impl(h, n, L, ldl, Dinv, Y, ldy, nrhs, const_mean, alpha, info, ws, ws_bytes, false);
}

static gpx_status potrs_impl(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv,
                             const double* Y, int64_t ldy, int64_t nrhs, double const_mean, double* alpha,
                             int32_t* info, void* ws, size_t ws_bytes, bool ws_cleared, const double* z) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldl, npad, "L", true));
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  size_t need = 0;
  GPX_TRY(gpx_potrs_workspace_size(n, nrhs, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "potrs workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_potrs(c, (int)n, (int)npad, L, ldl, Dinv, Y, ldy, (int)nrhs, const_mean, alpha, info,
                                        align256(ws), gpx::Batch(), ws_cleared, z),
                   "potrs");
}

gpx_status gpx_fit_factor_workspace_size(int64_t n, int64_t nrhs, size_t* bytes) {
  return gpx_potrs_workspace_size(n, nrhs, bytes);
}

gpx_status gpx_fit_factor_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                              const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv,
                              double* alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  size_t need = 0;
  if (gpx_fit_factor_workspace_size(n, nrhs, &need) != GPX_OK)
    return fail(c, GPX_INVALID_ARG, "invalid n / nrhs for fit");
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "fit workspace too small");
  if (!info) return fail(c, GPX_INVALID_ARG, "info is NULL");
  if (!ws) return fail(c, GPX_INVALID_ARG, "ws is NULL");
  GPX_NONNULL(c, Y);
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  // the Gram launch also clears the triangular solve's hand-off granules (no memset dispatch)
  const int64_t npad = padded(n);
  GPX_TRY(gram_impl(h, p, n, X, ldx, K, ldk, info, align256(ws), gpx::potrs_clear_bytes(npad, nrhs, 1)));
  // the dataflow Cholesky also runs the forward substitution; the solve is then its backward half
  gpx::ForwardRhs fr;
  fr.Y = Y;
  fr.ldy = ldy;
  fr.nrhs = (int)nrhs;
  fr.n = (int)n;
  fr.mean = p->const_mean;
  fr.buf = reinterpret_cast<double*>(reinterpret_cast<char*>(align256(ws)) + gpx::potrs_forward_offset(npad, nrhs, 1));
  bool z_done = false;
  GPX_TRY(potrf_impl(h, n, K, ldk, Dinv, info, false, nullptr, 0, &fr, &z_done));
  return potrs_impl(h, n, K, ldk, Dinv, Y, ldy, nrhs, p->const_mean, alpha, info, ws, ws_bytes, true,
                    z_done ? fr.buf + npad * gpx::rhs_row((int)nrhs) : nullptr);
}

gpx_status gpx_append_workspace_size(int64_t n_old, int64_t n_new, int64_t nrhs, size_t* bytes) {
  if (!bytes || n_old < 1 || n_new <= n_old || nrhs < 1 || nrhs > GPX_MAX_RHS) return GPX_INVALID_ARG;
  size_t a = gpx::append_workspace_bytes(n_old, n_new), b = alpha_ws(padded(n_new), nrhs);
  *bytes = (a > b ? a : b) + 256;
  return GPX_OK;
}

gpx_status gpx_append_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n_old, int64_t n_new, const double* X,
                          int64_t ldx, const double* Y, int64_t ldy, int64_t nrhs, double* L, int64_t ldl,
                          double* Dinv, double* W, int64_t ldw, double* alpha, int32_t* info, void* ws,
                          size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n_new));
  if (n_old < 1 || n_new <= n_old) return fail(c, GPX_INVALID_ARG, "append needs 1 <= n_old < n_new");
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n_new);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  GPX_TRY(check_ld(c, ldl, npad, "L", true));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  size_t need = 0;
  GPX_TRY(gpx_append_workspace_size(n_old, n_new, nrhs, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "append workspace too small");
  GPX_USE_DEVICE(c);
  double* base = align256(ws);
  GPX_TRY(hip_check(c, hipMemsetAsync(info, 0, sizeof(int32_t), c->stream), "memset info"));
  GPX_TRY(hip_check(c, gpx::launch_append(c, *p, (int)n_old, (int)n_new, X, ldx, L, ldl, Dinv, W, ldw, info, base),
                    "append"));
  double* zpart = base;
  double* z = zpart + (size_t)(npad / 128) * npad * nrhs;
  return hip_check(c, gpx::launch_alpha(c, (int)n_new, (int)npad, W, ldw, Y, ldy, (int)nrhs, p->const_mean, alpha,
                                        zpart, z),
                   "alpha");
}

static size_t fit_slice_bytes(int64_t npad, int64_t nrhs) {
  size_t a = trtri_ws(npad), b = alpha_ws(npad, nrhs);
  return ((a > b ? a : b) + 255) & ~(size_t)255;
}

// Bytes at the end of a batched fit's workspace for the per-problem constant means (Batch::means) of a fit whose
// problems carry their own kernel parameters.
static size_t means_bytes(int64_t batch) { return ((size_t)batch * 8 + 255) & ~(size_t)255; }

gpx_status gpx_fit_batched_workspace_size(int64_t n, int64_t nrhs, int64_t batch, size_t* bytes) {
  if (!bytes || n < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS || batch < 1 || batch > 65535) return GPX_INVALID_ARG;
  *bytes = fit_slice_bytes(padded(n), nrhs) * (size_t)batch + means_bytes(batch) + 256;
  return GPX_OK;
}

gpx_status gpx_fit_factor_batched_workspace_size(int64_t n, int64_t nrhs, int64_t batch, size_t* bytes) {
  if (!bytes || n < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS || batch < 1 || batch > 65535) return GPX_INVALID_ARG;
  *bytes = ((gpx::potrs_workspace_bytes(padded(n), nrhs, batch) + 255) & ~(size_t)255) + means_bytes(batch) + 256;
  return GPX_OK;
}

// Batched posterior updates; W == nullptr: factor + triangular solves only (gpx_fit_factor_batched_f64).  p points to
// one gpx_kernel_params (pstep = 0: shared by every problem) or to `batch` of them (pstep = 1, the
// gpx_fit_*_batched_params_f64 entry points).  Per-problem parameters that differ are served by one Gram launch per
// problem (its covariance parameters as kernel arguments; each launch fills the GPU from n ~ 1000 on) which also writes
// the problem's constant mean into the workspace for the solves; the Cholesky, the forward / backward solves and the
// inverse stay ONE set of launches over all problems (the latency-bound chain is what batching amortises).
static gpx_status fit_batched_impl(gpx_handle h, const gpx_kernel_params* p, int64_t pstep, int64_t batch, int64_t n,
                                   const double* X, int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy,
                                   int64_t stride_y, int64_t nrhs, double* K, int64_t ldk, int64_t stride_k,
                                   double* Dinv, int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w,
                                   double* alpha, int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  const bool inverse = W != nullptr;
  if (batch < 1 || batch > 65535) return fail(c, GPX_INVALID_ARG, "batch must be in [1, 65535]");
  GPX_NONNULL(c, p);
  bool shared = true;
  for (int64_t b = 0; b < (pstep ? batch : 1); ++b) {
    const gpx_status st = check_params(c, p + b);
    if (st != GPX_OK) return fail(c, st, "problem " + std::to_string(b) + ": " + c->last_error);
    if (p[b].d != p[0].d)
      return fail(c, GPX_INVALID_ARG, "every problem of a batched fit needs the same input dimension d");
    if (b > 0 && std::memcmp(p + b, p, sizeof(gpx_kernel_params)) != 0) shared = false;
  }
  GPX_TRY(check_n(c, n));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, K);
  GPX_NONNULL(c, Dinv);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  GPX_TRY(check_ld(c, ldk, npad, "K", true));
  if (inverse) GPX_TRY(check_ld(c, ldw, npad, "W", true));
  const int64_t nblk = npad / gpx::NB;
  if (batch > 1) {
    // outputs must not overlap (a stride of 0 would make the problems race on the same output); the read-only inputs
    // may be shared (stride 0: one X for the T outputs of a multi-output model) or interleaved (Y stride 1, ldy = T:
    // output column b of an n x T target matrix)
    if (stride_x < 0 || stride_y < 0) return fail(c, GPX_INVALID_ARG, "X / Y strides must be >= 0");
    if (stride_k < npad * ldk || (inverse && stride_w < npad * ldw) || stride_dinv < 2 * nblk * gpx::NB * gpx::NB ||
        stride_alpha < npad * nrhs)
      return fail(c, GPX_INVALID_ARG, "batch strides smaller than one problem");
    if ((stride_k | (inverse ? stride_w : 0) | stride_dinv) & 1)
      return fail(c, GPX_INVALID_ARG, "K/W/Dinv strides must be even");
  }
  size_t need = 0;
  if (inverse)
    GPX_TRY(gpx_fit_batched_workspace_size(n, nrhs, batch, &need));
  else
    GPX_TRY(gpx_fit_factor_batched_workspace_size(n, nrhs, batch, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "batched fit workspace too small");
  GPX_USE_DEVICE(c);
  gpx::Batch bt;
  bt.count = (int)batch;
  bt.x = stride_x;
  bt.y = stride_y;
  bt.k = stride_k;
  bt.dinv = stride_dinv;
  bt.w = stride_w;
  bt.alpha = stride_alpha;
  bt.ws = (int64_t)(fit_slice_bytes(npad, nrhs) / sizeof(double));
  double* slice = align256(ws);
  // per-problem constant means after the solves' part of the workspace
  const size_t solve_bytes = inverse ? fit_slice_bytes(npad, nrhs) * (size_t)batch
                                     : ((gpx::potrs_workspace_bytes(npad, nrhs, batch) + 255) & ~(size_t)255);
  double* means = shared ? nullptr : reinterpret_cast<double*>(reinterpret_cast<char*>(slice) + solve_bytes);
  bt.means = means;
  // the gram kernel clears info[0 .. batch) before the Cholesky (no separate memset dispatch), and in a factor-only fit
  // the triangular solve's hand-off granules of every problem
  void* zero = inverse ? nullptr : slice;
  const size_t zero_bytes = inverse ? 0 : gpx::potrs_clear_bytes(npad, nrhs, batch);
  if (shared) {
    GPX_TRY(hip_check(c, gpx::launch_gram(c, *p, (int)n, (int)npad, X, ldx, K, ldk, bt, 0, info, zero, zero_bytes),
                      "gram"));
  } else {
    for (int64_t b = 0; b < batch; ++b)
      GPX_TRY(hip_check(c, gpx::launch_gram(c, p[b], (int)n, (int)npad, X + b * stride_x, ldx, K + b * stride_k, ldk,
                                            gpx::Batch(), 0, info + b, b == 0 ? zero : nullptr, b == 0 ? zero_bytes : 0,
                                            means + b),
                        "gram"));
  }
  if (!inverse) {
    // factor + forward substitution (dataflow schedule), then the backward half of the solve
    gpx::ForwardRhs fr;
    fr.Y = Y;
    fr.ldy = ldy;
    fr.sy = stride_y;
    fr.nrhs = (int)nrhs;
    fr.n = (int)n;
    fr.mean = p->const_mean;
    fr.means = means;
    fr.buf = reinterpret_cast<double*>(reinterpret_cast<char*>(slice) + gpx::potrs_forward_offset(npad, nrhs, batch));
    bool z_done = false;
    GPX_TRY(hip_check(c, gpx::launch_potrf(c, (int)npad, K, ldk, Dinv, info, bt, nullptr, 0, &fr, &z_done), "potrf"));
    const int64_t nr = gpx::rhs_row((int)nrhs);
    return hip_check(c, gpx::launch_potrs(c, (int)n, (int)npad, K, ldk, Dinv, Y, ldy, (int)nrhs, p->const_mean, alpha,
                                          info, slice, bt, true, z_done ? fr.buf + npad * nr : nullptr, 2 * npad * nr),
                     "potrs");
  }
  GPX_TRY(hip_check(c, gpx::launch_potrf(c, (int)npad, K, ldk, Dinv, info, bt, W, ldw), "potrf"));
  GPX_TRY(hip_check(c, gpx::launch_trtri(c, (int)npad, K, ldk, Dinv, W, ldw, slice, bt, true), "trtri"));
  double* zpart = slice;
  double* z = zpart + (size_t)(npad / 128) * npad * nrhs;
  return hip_check(c, gpx::launch_alpha(c, (int)n, (int)npad, W, ldw, Y, ldy, (int)nrhs, p->const_mean, alpha, zpart, z,
                                        bt),
                   "alpha");
}

gpx_status gpx_fit_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n, const double* X,
                               int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy, int64_t stride_y,
                               int64_t nrhs, double* K, int64_t ldk, int64_t stride_k, double* Dinv,
                               int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w, double* alpha,
                               int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, W);
  return fit_batched_impl(h, p, 0, batch, n, X, ldx, stride_x, Y, ldy, stride_y, nrhs, K, ldk, stride_k, Dinv,
                          stride_dinv, W, ldw, stride_w, alpha, stride_alpha, info, ws, ws_bytes);
}

gpx_status gpx_fit_factor_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                      const double* X, int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy,
                                      int64_t stride_y, int64_t nrhs, double* K, int64_t ldk, int64_t stride_k,
                                      double* Dinv, int64_t stride_dinv, double* alpha, int64_t stride_alpha,
                                      int32_t* info, void* ws, size_t ws_bytes) {
  return fit_batched_impl(h, p, 0, batch, n, X, ldx, stride_x, Y, ldy, stride_y, nrhs, K, ldk, stride_k, Dinv,
                          stride_dinv, nullptr, 0, 0, alpha, stride_alpha, info, ws, ws_bytes);
}

gpx_status gpx_fit_batched_params_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                      const double* X, int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy,
                                      int64_t stride_y, int64_t nrhs, double* K, int64_t ldk, int64_t stride_k,
                                      double* Dinv, int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w,
                                      double* alpha, int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, W);
  return fit_batched_impl(h, p, 1, batch, n, X, ldx, stride_x, Y, ldy, stride_y, nrhs, K, ldk, stride_k, Dinv,
                          stride_dinv, W, ldw, stride_w, alpha, stride_alpha, info, ws, ws_bytes);
}

gpx_status gpx_fit_factor_batched_params_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                             const double* X, int64_t ldx, int64_t stride_x, const double* Y,
                                             int64_t ldy, int64_t stride_y, int64_t nrhs, double* K, int64_t ldk,
                                             int64_t stride_k, double* Dinv, int64_t stride_dinv, double* alpha,
                                             int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes) {
  return fit_batched_impl(h, p, 1, batch, n, X, ldx, stride_x, Y, ldy, stride_y, nrhs, K, ldk, stride_k, Dinv,
                          stride_dinv, nullptr, 0, 0, alpha, stride_alpha, info, ws, ws_bytes);
}

gpx_status gpx_mll_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 1 || n > ((int64_t)1 << 20)) return GPX_INVALID_ARG;
  *bytes = gpx::mll_workspace_bytes(padded(n)) + 256;
  return GPX_OK;
}

gpx_status gpx_mll_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                            const double* Y, int64_t ldy, int64_t nrhs, const double* L, int64_t ldl,
                            const double* W, int64_t ldw, const double* alpha, double* out, void* ws,
                            size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, out);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldl, npad, "L", false));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  if (ws_bytes < gpx::mll_workspace_bytes(npad) + 256) return fail(c, GPX_INVALID_ARG, "mll workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_mll(c, *p, (int)n, (int)npad, X, ldx, Y, ldy, (int)nrhs, L, ldl, W, ldw, alpha, out,
                                      align256(ws)), "mll");
}

// T independent problems (one gpx_kernel_params each): the fitted state of problem b at base + b * stride_*, out at
// out + b * GPX_MLL_NOUT.  One gradient pass per problem on the stream, the workspace of gpx_mll_workspace_size reused by
// each (the pass fills the GPU from n ~ 1000 on; the per-problem parameters enter the contraction's dK/dtheta epilogue).
gpx_status gpx_mll_grad_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n, const double* X,
                                    int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy, int64_t stride_y,
                                    int64_t nrhs, const double* L, int64_t ldl, int64_t stride_l, const double* W,
                                    int64_t ldw, int64_t stride_w, const double* alpha, int64_t stride_alpha,
                                    double* out, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (batch < 1 || batch > 65535) return fail(c, GPX_INVALID_ARG, "batch must be in [1, 65535]");
  GPX_NONNULL(c, p);
  for (int64_t b = 0; b < batch; ++b) {
    const gpx_status st = check_params(c, p + b);
    if (st != GPX_OK) return fail(c, st, "problem " + std::to_string(b) + ": " + c->last_error);
  }
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Y);
  GPX_NONNULL(c, L);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, out);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  for (int64_t b = 0; b < batch; ++b) GPX_TRY(check_ld(c, ldx, p[b].d, "X", false));
  GPX_TRY(check_ld(c, ldl, npad, "L", false));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  GPX_TRY(check_ld(c, ldy, nrhs, "Y", false));
  if (batch > 1 && (stride_x < 0 || stride_y < 0 || stride_l < npad * ldl || stride_w < npad * ldw ||
                    stride_alpha < npad * nrhs))
    return fail(c, GPX_INVALID_ARG, "batch strides smaller than one problem (X / Y: >= 0)");
  if (ws_bytes < gpx::mll_workspace_bytes(npad) + 256) return fail(c, GPX_INVALID_ARG, "mll workspace too small");
  GPX_USE_DEVICE(c);
  for (int64_t b = 0; b < batch; ++b)
    GPX_TRY(hip_check(c, gpx::launch_mll(c, p[b], (int)n, (int)npad, X + b * stride_x, ldx, Y + b * stride_y, ldy,
                                         (int)nrhs, L + b * stride_l, ldl, W + b * stride_w, ldw, alpha + b * stride_alpha,
                                         out + b * GPX_MLL_NOUT, align256(ws)),
                      "mll"));
  return GPX_OK;
}

gpx_status gpx_moments_grad_workspace_size(int64_t n, int64_t m, size_t* bytes) {
  if (!bytes || n < 1 || m < 1 || m > GPX_MAX_GRAD_CANDIDATES) return GPX_INVALID_ARG;
  *bytes = gpx::moments_grad_ws_doubles((int)padded(n), (int)m) * sizeof(double) + 256;
  return GPX_OK;
}

gpx_status gpx_moments_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                                int64_t q, int64_t ldxs, double* mean, double* dmean, double* cov, double* dcov,
                                void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  if (m < 1 || m > GPX_MAX_GRAD_CANDIDATES) return fail(c, GPX_INVALID_ARG, "m must be in [1, GPX_MAX_GRAD_CANDIDATES]");
  if (q < 1 || q > GPX_MAX_Q || m % q != 0) return fail(c, GPX_INVALID_ARG, "q must be in [1, GPX_MAX_Q] and divide m");
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, Xs);
  GPX_NONNULL(c, mean);
  GPX_NONNULL(c, dmean);
  GPX_NONNULL(c, cov);
  GPX_NONNULL(c, dcov);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  GPX_TRY(check_ld(c, ldxs, p->d, "Xs", false));
  size_t need = 0;
  GPX_TRY(gpx_moments_grad_workspace_size(n, m, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "moments_grad workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_moments_grad(c, *p, (int)n, (int)npad, X, ldx, W, ldw, alpha, Xs, ldxs, (int)m,
                                               (int)q, mean, dmean, cov, dcov, align256(ws)),
                   "moments_grad");
}

size_t gpx_mcacq_params_size(void) { return sizeof(gpx_mcacq_params); }

gpx_status gpx_mc_acq_workspace_size(int64_t B, int64_t q, int64_t S, size_t* bytes) {
  if (!bytes || q < 1 || q > GPX_MAX_Q || B < 1 || B * q > GPX_MAX_GRAD_CANDIDATES || S < 1 || S > (int64_t)1 << 20)
    return GPX_INVALID_ARG;
  *bytes = gpx::mc_acq_ws_doubles(B, q, S) * sizeof(double) + 256;
  return GPX_OK;
}

gpx_status gpx_mc_acq_f64(gpx_handle h, const gpx_mcacq_params* a, int64_t B, int64_t q, int64_t S, const double* mean,
                          const double* cov, const double* z, double* value, double* gmean, double* gcov,
                          int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, a);
  if (a->kind != GPX_MCACQ_QLOGEI && a->kind != GPX_MCACQ_QPSD)
    return fail(c, GPX_INVALID_ARG, "unknown MC acquisition kind " + std::to_string(a->kind));
  if ((a->fat_relu != 0 && a->fat_relu != 1) || (a->fat_max != 0 && a->fat_max != 1))
    return fail(c, GPX_INVALID_ARG, "gpx_mcacq_params.fat_relu / fat_max must be 0 or 1");
  if (a->reserved != 0) return fail(c, GPX_INVALID_ARG, "gpx_mcacq_params.reserved must be 0");
  if (!(a->tau_relu > 0.0) || !(a->tau_max > 0.0) || !std::isfinite(a->tau_relu) || !std::isfinite(a->tau_max))
    return fail(c, GPX_INVALID_ARG, "tau_relu and tau_max must be positive and finite");
  if (q < 1 || q > GPX_MAX_Q) return fail(c, GPX_INVALID_ARG, "q must be in [1, GPX_MAX_Q]");
  if (B < 1 || B * q > GPX_MAX_GRAD_CANDIDATES)
    return fail(c, GPX_INVALID_ARG, "B must be at least 1 and B * q at most GPX_MAX_GRAD_CANDIDATES");
  if (S < (a->kind == GPX_MCACQ_QPSD ? 2 : 1) || S > (int64_t)1 << 20)
    return fail(c, GPX_INVALID_ARG, "S must be in [1, 2^20], and at least 2 for GPX_MCACQ_QPSD");
  if ((gmean == nullptr) != (gcov == nullptr))
    return fail(c, GPX_INVALID_ARG, "gmean and gcov must be both NULL or both set");
  GPX_NONNULL(c, mean);
  GPX_NONNULL(c, cov);
  GPX_NONNULL(c, z);
  GPX_NONNULL(c, value);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  size_t need = 0;
  GPX_TRY(gpx_mc_acq_workspace_size(B, q, S, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "mc_acq workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_mc_acq(c, *a, (int)B, (int)q, (int)S, mean, cov, z, value, gmean, gcov, info,
                                         align256(ws)),
                   "mc_acq");
}

gpx_status gpx_joint_moments_workspace_size(int64_t n, int64_t mb, size_t* bytes) {
  if (!bytes || n < 1 || mb < 1 || mb > GPX_MAX_JOINT) return GPX_INVALID_ARG;
  *bytes = gpx::joint_moments_ws_doubles((int)padded(n), (int)mb) * sizeof(double) + 256;
  return GPX_OK;
}

gpx_status gpx_joint_moments_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                 const double* W, int64_t ldw, const double* alpha, const double* Xb, int64_t mb,
                                 int64_t ldxb, double* mean_b, double* cov_bb, double* Sb, int64_t ldsb, void* ws,
                                 size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  if (mb < 1 || mb > GPX_MAX_JOINT) return fail(c, GPX_INVALID_ARG, "mb must be in [1, GPX_MAX_JOINT]");
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, Xb);
  GPX_NONNULL(c, mean_b);
  GPX_NONNULL(c, cov_bb);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldw, npad, "W", true));
  GPX_TRY(check_ld(c, ldxb, p->d, "Xb", false));
  if (Sb) GPX_TRY(check_ld(c, ldsb, (mb + 63) / 64 * 64, "Sb", true));
  size_t need = 0;
  GPX_TRY(gpx_joint_moments_workspace_size(n, mb, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "joint_moments workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_joint_moments(c, *p, (int)n, (int)npad, X, ldx, W, ldw, alpha, Xb, (int)mb, ldxb,
                                                mean_b, cov_bb, Sb, ldsb, align256(ws)),
                   "joint_moments");
}

gpx_status gpx_cross_cov_grad_workspace_size(int64_t n, int64_t nb, int64_t m, size_t* bytes) {
  if (!bytes || n < 1 || nb < 1 || nb > GPX_MAX_BASELINE || m < 1 || m > GPX_MAX_GRAD_CANDIDATES)
    return GPX_INVALID_ARG;
  *bytes = 0;
  return GPX_OK;
}

gpx_status gpx_cross_cov_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* Sb, int64_t ldsb, const double* Xb, int64_t nb, int64_t ldxb,
                                  const double* Xs, int64_t m, int64_t ldxs, double* cross, double* dcross, void* ws,
                                  size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  (void)ws;
  (void)ws_bytes;
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  if (nb < 1 || nb > GPX_MAX_BASELINE) return fail(c, GPX_INVALID_ARG, "nb must be in [1, GPX_MAX_BASELINE]");
  if (m < 1 || m > GPX_MAX_GRAD_CANDIDATES) return fail(c, GPX_INVALID_ARG, "m must be in [1, GPX_MAX_GRAD_CANDIDATES]");
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Sb);
  GPX_NONNULL(c, Xb);
  GPX_NONNULL(c, Xs);
  GPX_NONNULL(c, cross);
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  GPX_TRY(check_ld(c, ldsb, nb, "Sb", false));
  GPX_TRY(check_ld(c, ldxb, p->d, "Xb", false));
  GPX_TRY(check_ld(c, ldxs, p->d, "Xs", false));
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_cross_cov_grad(c, *p, (int)n, X, ldx, Sb, ldsb, Xb, (int)nb, ldxb, Xs, (int)m, ldxs,
                                                 cross, dcross),
                   "cross_cov_grad");
}

size_t gpx_mcnei_params_size(void) { return sizeof(gpx_mcnei_params); }

gpx_status gpx_mc_nei_workspace_size(int64_t B, int64_t q, int64_t nb, int64_t S, size_t* bytes) {
  if (!bytes || q < 1 || q > GPX_MAX_Q || B < 1 || B * q > GPX_MAX_GRAD_CANDIDATES || nb < 1 ||
      nb > GPX_MAX_BASELINE || S < 1 || S > (int64_t)1 << 20)
    return GPX_INVALID_ARG;
  *bytes = gpx::mc_nei_ws_doubles(B, q, nb, S) * sizeof(double) + 256;
  return GPX_OK;
}

gpx_status gpx_mc_nei_f64(gpx_handle h, const gpx_mcnei_params* a, int64_t B, int64_t q, int64_t nb, int64_t S,
                          const double* mean, const double* cov, const double* cross, const double* Linv,
                          const double* zb, const double* best, const double* zq, double* value, double* gmean,
                          double* gcov, double* gcross, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, a);
  if ((a->log != 0 && a->log != 1) || (a->fat_relu != 0 && a->fat_relu != 1) || (a->fat_max != 0 && a->fat_max != 1))
    return fail(c, GPX_INVALID_ARG, "gpx_mcnei_params.log / fat_relu / fat_max must be 0 or 1");
  if (a->reserved != 0) return fail(c, GPX_INVALID_ARG, "gpx_mcnei_params.reserved must be 0");
  if (!(a->tau_relu > 0.0) || !(a->tau_max > 0.0) || !std::isfinite(a->tau_relu) || !std::isfinite(a->tau_max))
    return fail(c, GPX_INVALID_ARG, "tau_relu and tau_max must be positive and finite");
  if (q < 1 || q > GPX_MAX_Q) return fail(c, GPX_INVALID_ARG, "q must be in [1, GPX_MAX_Q]");
  if (B < 1 || B * q > GPX_MAX_GRAD_CANDIDATES)
    return fail(c, GPX_INVALID_ARG, "B must be at least 1 and B * q at most GPX_MAX_GRAD_CANDIDATES");
  if (nb < 1 || nb > GPX_MAX_BASELINE) return fail(c, GPX_INVALID_ARG, "nb must be in [1, GPX_MAX_BASELINE]");
  if (S < 1 || S > (int64_t)1 << 20) return fail(c, GPX_INVALID_ARG, "S must be in [1, 2^20]");
  const int ngrad = (gmean != nullptr) + (gcov != nullptr) + (gcross != nullptr);
  if (ngrad != 0 && ngrad != 3)
    return fail(c, GPX_INVALID_ARG, "gmean, gcov and gcross must be all NULL or all set");
  GPX_NONNULL(c, mean);
  GPX_NONNULL(c, cov);
  GPX_NONNULL(c, cross);
  GPX_NONNULL(c, Linv);
  GPX_NONNULL(c, zb);
  GPX_NONNULL(c, best);
  GPX_NONNULL(c, zq);
  GPX_NONNULL(c, value);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  size_t need = 0;
  GPX_TRY(gpx_mc_nei_workspace_size(B, q, nb, S, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "mc_nei workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_mc_nei(c, *a, (int)B, (int)q, (int)nb, (int)S, mean, cov, cross, Linv, zb, best, zq,
                                         value, gmean, gcov, gcross, info, align256(ws)),
                   "mc_nei");
}

// ---- the sweep entry points' shared checks (the first failing one wins, in the order of the calls below) ----
// the model and the candidate count; m_max = 0: any m >= 1 (the sweeps chunk it), else the debug calls' cap
static gpx_status check_sweep_sizes(Context* c, const gpx_kernel_params* p, int64_t n, int64_t m, int64_t m_max = 0) {
  GPX_TRY(check_params(c, p));
  GPX_TRY(check_n(c, n));
  if (m < 1 || (m_max && m > m_max))
    return fail(c, GPX_INVALID_ARG, m_max ? "m must be in [1, 2^30]" : "m must be >= 1");
  return GPX_OK;
}
constexpr int64_t kDebugMaxM = (int64_t)1 << 30;
// the arrays (every pointer, then the pitches of X, W where the call has one, and Xs)
using NamedPtr = std::pair<const void*, const char*>;
static gpx_status check_sweep_arrays(Context* c, std::initializer_list<NamedPtr> ptrs, const gpx_kernel_params* p,
                                     int64_t ldx, int64_t ldxs, const int64_t* ldw = nullptr, int64_t npad = 0) {
  for (const NamedPtr& q : ptrs)
    if (!q.first) return fail(c, GPX_INVALID_ARG, std::string(q.second) + " is NULL");
  GPX_TRY(check_ld(c, ldx, p->d, "X", false));
  if (ldw) GPX_TRY(check_ld(c, *ldw, npad, "W", true));
  return check_ld(c, ldxs, p->d, "Xs", false);
}
// the acquisition and the index offset (y_scale: the single-output calls, which untransform by a's own pair)
static gpx_status check_acq(Context* c, const gpx_acq_params* a, int64_t index_offset, bool y_scale) {
  if (!a) return fail(c, GPX_INVALID_ARG, "acquisition params pointer is NULL");
  if (a->kind < GPX_ACQ_EI || a->kind > GPX_ACQ_VARIANCE) return fail(c, GPX_INVALID_ARG, "unknown acquisition kind");
  if (a->reserved != 0) return fail(c, GPX_INVALID_ARG, "gpx_acq_params.reserved must be 0");
  if (y_scale && !(a->y_scale > 0.0)) return fail(c, GPX_INVALID_ARG, "y_scale must be positive");
  if (a->kind == GPX_ACQ_UCB && !(a->beta >= 0.0)) return fail(c, GPX_INVALID_ARG, "UCB beta must be >= 0");
  if (index_offset < 0) return fail(c, GPX_INVALID_ARG, "index_offset must be >= 0");
  return GPX_OK;
}
// the workspace against the layout's total, then every pointer into it
static gpx_status carve_sweep(Context* c, const gpx::SweepLayout& L, void* ws, size_t ws_bytes, const char* too_small,
                              gpx::SweepWorkspace* w, int64_t k = 0) {
  if (ws && ws_bytes < L.total) return fail(c, GPX_INVALID_ARG, too_small);
  if (!ws) return fail(c, GPX_INVALID_ARG, "sweep workspace is NULL");
  *w = gpx::sweep_carve(ws, L, k);
  return GPX_OK;
}
static size_t ws_skew(const void* ws) { return (size_t)(-reinterpret_cast<uintptr_t>(ws) & 255); }

gpx_status gpx_sweep_workspace_size(int64_t n, int64_t nrhs, int64_t m, size_t* bytes) {
  if (!bytes || n < 1 || m < 1 || nrhs < 1 || nrhs > GPX_MAX_RHS) return GPX_INVALID_ARG;
  *bytes = gpx::sweep_layout(padded(n), nrhs, m).total;
  return GPX_OK;
}

gpx_status gpx_posterior_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                             const double* W, int64_t ldw, const double* alpha, int64_t nrhs, const double* Xs,
                             int64_t m, int64_t ldxs, const double* y_mean_host, const double* y_scale_host,
                             double* mean_out, int64_t ldmean, double* var_out, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_sweep_sizes(c, p, n, m));
  if (nrhs < 1 || nrhs > GPX_MAX_RHS) return fail(c, GPX_INVALID_ARG, "nrhs must be in [1, 8]");
  const int64_t npad = padded(n);
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {W, "W"}, {alpha, "alpha"}, {Xs, "Xs"}, {mean_out, "mean_out"},
                                 {var_out, "var_out"}}, p, ldx, ldxs, &ldw, npad));
  GPX_TRY(check_ld(c, ldmean, nrhs, "mean", false));
  gpx::SweepWorkspace w;
  GPX_TRY(carve_sweep(c, gpx::sweep_layout(npad, nrhs, m), ws, ws_bytes, "sweep workspace too small", &w));
  GPX_USE_DEVICE(c);
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, W, ldw, alpha, (int)nrhs};
  for (int64_t s = 0; s < m; s += w.b.chunk) {
    const gpx::SweepCands q{Xs + s * ldxs, ldxs, gpx::sweep_span_size(false, s, m, w.b.chunk, 0), 0};
    const gpx::SweepOut out{nullptr, y_mean_host, y_scale_host, mean_out + s * ldmean, ldmean, var_out + s};
    GPX_TRY(hip_check(c, gpx::launch_sweep_chunk(M, q, w.b, nullptr, out), "posterior"));
  }
  return GPX_OK;
}

// gpx_acquire_argmax_f64 (k = 0: best_val / best_idx, optional scores_out) and gpx_acquire_topk_f64 (k >= 1: val_out /
// idx_out, the top-k part of the workspace behind the sweep's) share validation, chunking and counters.
static gpx_status acquire_impl(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                               const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                               int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, double* best_val,
                               int64_t* best_idx, double* scores_out, void* ws, size_t ws_bytes, int64_t k,
                               double* val_out, int64_t* idx_out) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  const bool topk = val_out || idx_out || k != 0;
  GPX_TRY(check_sweep_sizes(c, p, n, m));
  GPX_TRY(check_acq(c, a, index_offset, true));
  if (topk && (k < 1 || k > m || k > GPX_TOPK_SWEEP_MAX))
    return fail(c, GPX_INVALID_ARG, "k must be in [1, min(m, GPX_TOPK_SWEEP_MAX)]");
  const int64_t npad = padded(n);
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {W, "W"}, {alpha, "alpha"}, {Xs, "Xs"},
                                 {topk ? val_out : best_val, topk ? "val_out" : "best_val"},
                                 {topk ? idx_out : best_idx, topk ? "idx_out" : "best_idx"}}, p, ldx, ldxs, &ldw, npad));
  gpx::SweepWorkspace w;
  GPX_TRY(carve_sweep(c, gpx::sweep_layout(npad, 1, m, k, false, topk ? gpx::topk_workspace_bytes(m) : 0, ws_skew(ws)),
                      ws, ws_bytes, topk ? "acquire_topk workspace too small" : "sweep workspace too small", &w, k));
  const gpx::SweepBuffers& b = w.b;
  // scores_out wants every score: the full sweep
  const bool prune = !scores_out && gpx::sweep_prune_ok(c, *p, (int)npad);
  const gpx::TopkSweep* tk = topk && prune ? &w.tk : nullptr;
  // the top-k call where the pruned sweep does not apply: the full sweep into its own score array, then the sort
  if (topk && !prune) scores_out = w.tk.scores;
  // the MFMA K* build's configurations take the lazy form (K* in full height for the first tile's survivors only)
  const bool lazy = prune && gpx::sweep_lazy_ok(*p);
  GPX_USE_DEVICE(c);
  const bool fused = gpx::sweep_fused_ok(c, *p, (int)npad, 1);
  const auto tiles = [&](int64_t mc) { return (mc + 127) / 128 * (npad / 128); };
  c->sweep_stats[0] = m;
  c->sweep_stats[1] = prune ? 0 : m;
  c->sweep_stats[2] = 0;
  // [3]: the tiles of the full sweep, with the full path's chunking
  c->sweep_stats[3] = fused ? 0 : m / b.chunk * tiles(b.chunk) + tiles(m % b.chunk);
  c->sweep_stats_dev = prune ? w.ps.stats : nullptr;
  c->tail_rounds[0] = c->tail_rounds[1] = 0;
  c->tail_rounds[2] = -1;
  // spans of a chunk, or on the lazy path of a super-chunk (sweep_span_size)
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, W, ldw, alpha, 1};
  int64_t rec = 0;
  for (int64_t s = 0, ms = 0; s < m; s += ms) {
    ms = gpx::sweep_span_size(lazy, s, m, b.chunk, w.ph.super);
    const gpx::SweepCands q{Xs + s * ldxs, ldxs, ms, index_offset + s};
    const gpx::SweepOut out{scores_out ? scores_out + s : nullptr};
    const hipError_t e =
        lazy    ? gpx::launch_sweep_super_pruned(M, q, b, w.ps, w.ph, a, &rec, s == 0, c->sweep_stats, tk)
        : prune ? gpx::launch_sweep_chunk_pruned(M, q, b, w.ps, a, rec, s == 0, c->sweep_stats, tk)
                : gpx::launch_sweep_chunk(M, q, b, a, out, rec);
    GPX_TRY(hip_check(c, e, "acquire"));
    if (!lazy) rec += (ms + 255) / 256;  // (the lazy path counts its own: the rounds' blocks)
  }
  if (!prune) c->sweep_stats[2] = c->sweep_stats[3];
  if (tk) return hip_check(c, gpx::launch_topk_result(c, *tk, val_out, idx_out), "topk result");
  if (topk) {
    GPX_TRY(hip_check(c, gpx::launch_topk(c, w.tk.scores, m, k, idx_out, val_out, w.tk.sort_ws, w.tk.sort_bytes), "topk"));
    return hip_check(c, gpx::launch_index_shift(c, idx_out, k, index_offset), "topk indices");
  }
  return hip_check(c, gpx::launch_argmax_final(c, lazy ? w.ph.rec_val : b.rec_val, lazy ? w.ph.rec_idx : b.rec_idx, rec,
                                               best_val, best_idx),
                   "argmax");
}

gpx_status gpx_acquire_argmax_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                                  int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, double* best_val,
                                  int64_t* best_idx, double* scores_out, void* ws, size_t ws_bytes) {
  return acquire_impl(h, p, n, X, ldx, W, ldw, alpha, Xs, m, ldxs, a, index_offset, best_val, best_idx, scores_out, ws,
                      ws_bytes, 0, nullptr, nullptr);
}

gpx_status gpx_acquire_topk_workspace_size(int64_t n, int64_t m, int64_t k, size_t* bytes) {
  if (!bytes || n < 1 || m < 1 || k < 1 || k > m || k > GPX_TOPK_SWEEP_MAX) return GPX_INVALID_ARG;
  *bytes = gpx::sweep_layout(padded(n), 1, m, k, false, gpx::topk_workspace_bytes(m)).total;
  return GPX_OK;
}

gpx_status gpx_acquire_topk_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                                int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, int64_t k, double* val_out,
                                int64_t* idx_out, void* ws, size_t ws_bytes) {
  if (h && k == 0) return fail(reinterpret_cast<Context*>(h), GPX_INVALID_ARG, "k must be >= 1");
  return acquire_impl(h, p, n, X, ldx, W, ldw, alpha, Xs, m, ldxs, a, index_offset, nullptr, nullptr, nullptr, ws,
                      ws_bytes, k, val_out, idx_out);
}

gpx_status gpx_sweep_stats(gpx_handle h, int64_t* out) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, out);
  for (int i = 0; i < 4; ++i) out[i] = c->sweep_stats[i];
  if (c->sweep_stats_dev) {
    GPX_USE_DEVICE(c);
    int64_t dev[2];
    GPX_TRY(hip_check(c, hipMemcpyAsync(dev, c->sweep_stats_dev, sizeof(dev), hipMemcpyDeviceToHost, c->stream),
                      "sweep_stats"));
    GPX_TRY(hip_check(c, hipStreamSynchronize(c->stream), "sweep_stats"));
    out[1] += dev[0];
    out[2] += dev[1];
  }
  return GPX_OK;
}

gpx_status gpx_debug_kstar_workspace_size(int64_t n, int64_t ldout, size_t* bytes) {
  if (!bytes || n < 1 || ldout < 256) return GPX_INVALID_ARG;
  const int64_t npad = padded(n);
  *bytes = ((size_t)(npad / gpx::NB) * ldout + npad) * 8 + 256;
  return GPX_OK;
}

gpx_status gpx_debug_kstar_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                               const double* Xs, int64_t m, int64_t ldxs, const int32_t* list, const int32_t* count,
                               double* out, int64_t ldout, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_sweep_sizes(c, p, n, m, kDebugMaxM));
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {Xs, "Xs"}, {out, "out"}}, p, ldx, ldxs));
  const int64_t npad = padded(n);
  if (ldout < (m + 255) / 256 * 256) return fail(c, GPX_INVALID_ARG, "ldout must be >= m rounded up to 256");
  if (list && !count) return fail(c, GPX_INVALID_ARG, "count is NULL");
  if (list && !gpx::sweep_lazy_ok(*p))
    return fail(c, GPX_INVALID_ARG, "the gather build covers the fp64 covariance with d <= 16");
  double* scratch = nullptr;
  if (!list) {  // the full build writes its mean partials: scratch for them and a zero alpha
    size_t need = 0;
    GPX_TRY(gpx_debug_kstar_workspace_size(n, ldout, &need));
    if (!ws || ws_bytes < need) return fail(c, GPX_INVALID_ARG, "debug_kstar workspace too small");
    scratch = align256(ws);
  }
  GPX_USE_DEVICE(c);
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, nullptr, 0, nullptr, 1};
  return hip_check(c, gpx::launch_debug_kstar(M, {Xs, ldxs, m, 0}, list, count, out, ldout, scratch), "debug_kstar");
}

gpx_status gpx_debug_kstar_mu_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* alpha, const double* Xs, int64_t m, int64_t ldxs, const int32_t* list,
                                  const int32_t* count, double* out, int64_t ldout, double* mu_part, int64_t ldmu) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_sweep_sizes(c, p, n, m, kDebugMaxM));
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {alpha, "alpha"}, {Xs, "Xs"}, {out, "out"}, {mu_part, "mu_part"}}, p, ldx,
                             ldxs));
  const int64_t npad = padded(n);
  if (ldout < (m + 255) / 256 * 256) return fail(c, GPX_INVALID_ARG, "ldout must be >= m rounded up to 256");
  if (list && !count) return fail(c, GPX_INVALID_ARG, "count is NULL");
  if (list && ldmu < 1) return fail(c, GPX_INVALID_ARG, "ldmu must be >= 1");
  if (!gpx::sweep_lazy_ok(*p)) return fail(c, GPX_INVALID_ARG, "the MFMA K* build covers the fp64 covariance with d <= 16");
  GPX_USE_DEVICE(c);
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, nullptr, 0, alpha, 1};
  return hip_check(c, gpx::launch_debug_kstar(M, {Xs, ldxs, m, 0}, list, count, out, ldout, nullptr, mu_part, ldmu),
                   "debug_kstar_mu");
}

gpx_status gpx_debug_set_sweep_head(gpx_handle h, int32_t value) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (value != 0 && value != 1) return fail(c, GPX_INVALID_ARG, "sweep_head must be 0 or 1");
  c->sweep_head = value;
  return GPX_OK;
}

gpx_status gpx_debug_get_sweep_head(gpx_handle h, int32_t* value_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, value_host);
  *value_host = c->sweep_head;
  return GPX_OK;
}

gpx_status gpx_debug_set_sweep_order(gpx_handle h, int32_t value) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (value != 0 && value != 1) return fail(c, GPX_INVALID_ARG, "sweep_order must be 0 or 1");
  c->sweep_order = value;
  return GPX_OK;
}

gpx_status gpx_debug_get_sweep_order(gpx_handle h, int32_t* value_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, value_host);
  *value_host = c->sweep_order;
  return GPX_OK;
}

gpx_status gpx_debug_set_sweep_tail_sync(gpx_handle h, int32_t value) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (value != 0 && value != 1) return fail(c, GPX_INVALID_ARG, "sweep_tail_sync must be 0 or 1");
  c->sweep_tail_sync = value;
  return GPX_OK;
}

gpx_status gpx_debug_get_sweep_tail_sync(gpx_handle h, int32_t* value_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, value_host);
  *value_host = c->sweep_tail_sync;
  return GPX_OK;
}

gpx_status gpx_debug_get_tail_rounds(gpx_handle h, int64_t* out) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, out);
  for (int i = 0; i < 3; ++i) out[i] = c->tail_rounds[i];
  return GPX_OK;
}

static gpx_status debug_head_product(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                     const double* alpha, const double* Xs, int64_t m, int64_t ldxs, const double* W,
                                     int64_t ldw, double* ss, double* mu_part, int64_t ldmu, const int32_t* list,
                                     const int32_t* count) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_sweep_sizes(c, p, n, m, kDebugMaxM));
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {alpha, "alpha"}, {Xs, "Xs"}, {W, "W"}, {ss, "ss"}, {mu_part, "mu_part"}}, p,
                             ldx, ldxs));
  const int64_t npad = padded(n);
  if (ldw < npad) return fail(c, GPX_INVALID_ARG, "ldw must be >= padded n");
  if (ldmu < (m + 255) / 256 * 256) return fail(c, GPX_INVALID_ARG, "ldmu must be >= m rounded up to 256");
  if (!gpx::sweep_lazy_ok(*p)) return fail(c, GPX_INVALID_ARG, "the fused head covers the fp64 covariance with d <= 16");
  GPX_USE_DEVICE(c);
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, W, ldw, alpha, 1};
  return hip_check(c, gpx::launch_debug_head_product(M, {Xs, ldxs, m, 0}, ss, mu_part, ldmu, list, count),
                   "debug_head_product");
}

gpx_status gpx_debug_head_product_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                      const double* alpha, const double* Xs, int64_t m, int64_t ldxs, const double* W,
                                      int64_t ldw, double* ss, double* mu_part, int64_t ldmu) {
  return debug_head_product(h, p, n, X, ldx, alpha, Xs, m, ldxs, W, ldw, ss, mu_part, ldmu, nullptr, nullptr);
}

gpx_status gpx_debug_head_product_list_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X,
                                           int64_t ldx, const double* alpha, const double* Xs, int64_t m, int64_t ldxs,
                                           const double* W, int64_t ldw, double* ss, double* mu_part, int64_t ldmu,
                                           const int32_t* list, const int32_t* count) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, list);
  GPX_NONNULL(c, count);
  if (reinterpret_cast<uintptr_t>(list) % 8) return fail(c, GPX_INVALID_ARG, "list must be 8-byte aligned");
  return debug_head_product(h, p, n, X, ldx, alpha, Xs, m, ldxs, W, ldw, ss, mu_part, ldmu, list, count);
}

gpx_status gpx_debug_stage_product_workspace_size(int64_t ncols, size_t* bytes) {
  if (!bytes || ncols < 1 || ncols > ((int64_t)1 << 20)) return GPX_INVALID_ARG;
  *bytes = gpx::debug_stage_product_bytes(ncols) + 256;
  return GPX_OK;
}

gpx_status gpx_debug_stage_product_f64(gpx_handle h, int64_t n, const double* W, int64_t ldw, const double* kstar,
                                       int64_t ldk, int64_t ncols, const int32_t* list, int32_t I0, int32_t nrows,
                                       int32_t shape, double* ss, int64_t ldss, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_n(c, n));
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, kstar);
  GPX_NONNULL(c, ss);
  GPX_NONNULL(c, ws);
  const int64_t npad = padded(n), nI = npad / gpx::TILE;
  if (ncols < 1 || ncols > ((int64_t)1 << 20)) return fail(c, GPX_INVALID_ARG, "ncols must be in [1, 2^20]");
  if (I0 < 0 || nrows < 1 || (int64_t)I0 + nrows > nI)
    return fail(c, GPX_INVALID_ARG, "the stage's row tiles must be I0 >= 0, nrows >= 1, I0 + nrows <= padded n / 128");
  if (shape != 0 && shape != 1) return fail(c, GPX_INVALID_ARG, "shape must be 0 (wide) or 1 (narrow)");
  const int64_t cpad = (ncols + gpx::TILE - 1) / gpx::TILE * gpx::TILE;
  if (ldw < npad || (ldw & 1) || (reinterpret_cast<uintptr_t>(W) & 15))
    return fail(c, GPX_INVALID_ARG, "W must be 16-byte aligned with an even pitch >= padded n");
  if (ldk < cpad || (ldk & 1) || (reinterpret_cast<uintptr_t>(kstar) & 15))
    return fail(c, GPX_INVALID_ARG, "kstar must be 16-byte aligned with an even pitch >= ncols rounded up to 128");
  if (ldss < cpad) return fail(c, GPX_INVALID_ARG, "ldss must be >= ncols rounded up to 128");
  size_t need = 0;
  GPX_TRY(gpx_debug_stage_product_workspace_size(ncols, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "debug_stage_product workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c,
                   gpx::launch_debug_stage_product(c, (int)npad, W, ldw, kstar, ldk, (int)ncols, list, I0, nrows, shape,
                                                   ss, ldss, align256(ws)),
                   "debug_stage_product");
}

gpx_status gpx_debug_mu_bound_workspace_size(int64_t n, size_t* bytes) {
  if (!bytes || n < 1) return GPX_INVALID_ARG;
  *bytes = gpx::mu_prep_doubles(padded(n), 16) * 8 + 256;
  return GPX_OK;
}

gpx_status gpx_debug_mu_bound_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* alpha, const double* Xs, int64_t m, int64_t ldxs, double* mu_approx,
                                  double* mu_slack, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_sweep_sizes(c, p, n, m, kDebugMaxM));
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {alpha, "alpha"}, {Xs, "Xs"}, {mu_approx, "mu_approx"},
                                 {mu_slack, "mu_slack"}}, p, ldx, ldxs));
  const int64_t npad = padded(n);
  if (!gpx::sweep_mu_bound_ok(*p))
    return fail(c, GPX_INVALID_ARG, "the mean bound covers the RBF kernel, the fp64 covariance and d <= 16");
  size_t need = 0;
  GPX_TRY(gpx_debug_mu_bound_workspace_size(n, &need));
  if (!ws || ws_bytes < need) return fail(c, GPX_INVALID_ARG, "debug_mu_bound workspace too small");
  GPX_USE_DEVICE(c);
  const gpx::SweepModel M{c, *p, (int)n, (int)npad, X, ldx, nullptr, 0, alpha, 1};
  return hip_check(c, gpx::launch_mu_bound(M, {Xs, ldxs, m, 0}, align256(ws), mu_approx, mu_slack), "debug_mu_bound");
}

gpx_status gpx_sweep_multi_workspace_size(int64_t n, int64_t m, size_t* bytes) {
  if (!bytes || n < 1 || m < 1) return GPX_INVALID_ARG;
  *bytes = gpx::sweep_layout(padded(n), 1, m, 0, true).total;
  return GPX_OK;
}

// gpx_acquire_argmax_multi_f64 (k = 0: best_val / best_idx, optional scores_out) and gpx_acquire_topk_multi_f64 (k >= 1:
// val_out / idx_out, the top-k regions behind the multi-output sweep's workspace) share validation and the full sweep.
static gpx_status acquire_multi_impl(gpx_handle h, const gpx_kernel_params* p, int64_t T, int64_t n, const double* X,
                                     int64_t ldx, const double* const* W_host, const int64_t* ldw_host,
                                     const double* const* alpha_host, const double* weights_host,
                                     const double* y_mean_host, const double* y_scale_host, const double* Xs,
                                     int64_t m, int64_t ldxs, const gpx_acq_params* a, int64_t index_offset,
                                     double* best_val, int64_t* best_idx, double* scores_out, void* ws,
                                     size_t ws_bytes, int64_t k, double* val_out, int64_t* idx_out) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  const bool topk = val_out || idx_out || k != 0;
  if (T < 1 || T > 64) return fail(c, GPX_INVALID_ARG, "T (outputs) must be in [1, 64]");
  GPX_NONNULL(c, p);
  GPX_NONNULL(c, weights_host);
  for (int64_t t = 0; t < T; ++t) {
    const gpx_status st = check_params(c, p + t);
    if (st != GPX_OK) return fail(c, st, "output " + std::to_string(t) + ": " + c->last_error);
    if (p[t].d != p[0].d) return fail(c, GPX_INVALID_ARG, "every output needs the same input dimension d");
    if (!std::isfinite(weights_host[t])) return fail(c, GPX_INVALID_ARG, "objective weights must be finite");
    if (y_scale_host && !(y_scale_host[t] > 0.0)) return fail(c, GPX_INVALID_ARG, "y_scale must be positive");
  }
  GPX_TRY(check_sweep_sizes(c, p, n, m));
  GPX_TRY(check_acq(c, a, index_offset, false));
  if (topk && (k < 1 || k > m || k > GPX_TOPK_SWEEP_MAX))
    return fail(c, GPX_INVALID_ARG, "k must be in [1, min(m, GPX_TOPK_SWEEP_MAX)]");
  GPX_TRY(check_sweep_arrays(c, {{X, "X"}, {W_host, "W_host"}, {ldw_host, "ldw_host"}, {alpha_host, "alpha_host"},
                                 {Xs, "Xs"}, {topk ? val_out : best_val, topk ? "val_out" : "best_val"},
                                 {topk ? (void*)idx_out : (void*)best_idx, topk ? "idx_out" : "best_idx"}, {ws, "ws"}},
                             p, ldx, ldxs));
  const int64_t npad = padded(n);
  for (int64_t t = 0; t < T; ++t) {
    if (!W_host[t] || !alpha_host[t]) return fail(c, GPX_INVALID_ARG, "W / alpha of output " + std::to_string(t) + " is NULL");
    GPX_TRY(check_ld(c, ldw_host[t], npad, "W", true));
  }
  gpx::SweepWorkspace w;
  if (topk) {
    const gpx::TopkMultiLayout TL = gpx::topk_multi_layout(npad, m, k, gpx::topk_workspace_bytes(m));
    if (ws_bytes < TL.total) return fail(c, GPX_INVALID_ARG, "acquire_topk_multi workspace too small");
    w = gpx::topk_multi_carve(ws, TL, k);
  } else {
    GPX_TRY(carve_sweep(c, gpx::sweep_layout(npad, 1, m, 0, true), ws, ws_bytes,
                        "multi-output sweep workspace too small", &w));
  }
  const gpx::SweepBuffers& b = w.b;
  GPX_USE_DEVICE(c);
  if (topk) {
    // the pruned form where gpx_acquire_topk_f64 would take its lazy one for every output; else the full sweep into the
    // call's own score array, then the sort
    bool prune = true;
    for (int64_t t = 0; t < T; ++t) prune = prune && gpx::sweep_prune_ok(c, p[t], (int)npad) && gpx::sweep_lazy_ok(p[t]);
    const auto tiles = [&](int64_t mc) { return (mc + 127) / 128 * (npad / 128); };
    c->sweep_stats[0] = m;
    c->sweep_stats[1] = prune ? 0 : m;
    c->sweep_stats[2] = c->sweep_stats[3] = 0;
    // [3]: the tiles of the full multi-output sweep, every unfused output's share
    for (int64_t t = 0; t < T; ++t)
      if (!gpx::sweep_fused_ok(c, p[t], (int)npad, 1)) c->sweep_stats[3] += m / b.chunk * tiles(b.chunk) + tiles(m % b.chunk);
    c->sweep_stats_dev = prune ? w.ps.stats : nullptr;
    if (prune) {
      gpx::MultiModel outs[64];  // (T <= 64)
      for (int64_t t = 0; t < T; ++t)
        outs[t] = {p + t, W_host[t], ldw_host[t], alpha_host[t], weights_host[t],
                   y_mean_host ? y_mean_host[t] : 0.0, y_scale_host ? y_scale_host[t] : 1.0};
      for (int64_t s = 0; s < m; s += b.chunk) {
        const int64_t mc = gpx::sweep_span_size(false, s, m, b.chunk, 0);
        GPX_TRY(hip_check(c, gpx::launch_topk_multi_chunk(c, (int)T, outs, (int)n, (int)npad, X, ldx,
                                                          {Xs + s * ldxs, ldxs, mc, index_offset + s}, w, *a, s == 0,
                                                          c->sweep_stats),
                          "acquire_topk (multi-output)"));
      }
      return hip_check(c, gpx::launch_topk_result(c, w.tk, val_out, idx_out), "topk result");
    }
    c->sweep_stats[2] = c->sweep_stats[3];
    scores_out = w.tk.scores;
  }
  gpx::MultiOutput mo;
  mo.acc_mu = w.acc_mu;
  mo.acc_var = w.acc_var;
  int64_t rec = 0;
  for (int64_t s = 0; s < m; s += b.chunk) {
    const int64_t mc = gpx::sweep_span_size(false, s, m, b.chunk, 0);
    for (int64_t t = 0; t < T; ++t) {
      mo.weight = weights_host[t];
      mo.y_mean = y_mean_host ? y_mean_host[t] : 0.0;
      mo.y_scale = y_scale_host ? y_scale_host[t] : 1.0;
      mo.first = t == 0;
      const gpx::SweepModel M{c, p[t], (int)n, (int)npad, X, ldx, W_host[t], ldw_host[t], alpha_host[t], 1};
      GPX_TRY(hip_check(c, gpx::launch_sweep_chunk(M, {Xs + s * ldxs, ldxs, mc, 0}, b, a, gpx::SweepOut(), 0, &mo),
                        "acquire (multi-output)"));
    }
    GPX_TRY(hip_check(c, gpx::launch_multi_score(c, {nullptr, 0, mc, index_offset + s}, mo, *a,
                                                 scores_out ? scores_out + s : nullptr, b.rec_val + rec, b.rec_idx + rec),
                      "acquire (multi-output score)"));
    rec += (mc + 255) / 256;
  }
  if (topk) {
    GPX_TRY(hip_check(c, gpx::launch_topk(c, w.tk.scores, m, k, idx_out, val_out, w.tk.sort_ws, w.tk.sort_bytes), "topk"));
    return hip_check(c, gpx::launch_index_shift(c, idx_out, k, index_offset), "topk indices");
  }
  return hip_check(c, gpx::launch_argmax_final(c, b.rec_val, b.rec_idx, rec, best_val, best_idx), "argmax");
}

gpx_status gpx_acquire_argmax_multi_f64(gpx_handle h, const gpx_kernel_params* p, int64_t T, int64_t n, const double* X,
                                        int64_t ldx, const double* const* W_host, const int64_t* ldw_host,
                                        const double* const* alpha_host, const double* weights_host,
                                        const double* y_mean_host, const double* y_scale_host, const double* Xs,
                                        int64_t m, int64_t ldxs, const gpx_acq_params* a, int64_t index_offset,
                                        double* best_val, int64_t* best_idx, double* scores_out, void* ws,
                                        size_t ws_bytes) {
  return acquire_multi_impl(h, p, T, n, X, ldx, W_host, ldw_host, alpha_host, weights_host, y_mean_host, y_scale_host,
                            Xs, m, ldxs, a, index_offset, best_val, best_idx, scores_out, ws, ws_bytes, 0, nullptr,
                            nullptr);
}

gpx_status gpx_acquire_topk_multi_workspace_size(int64_t n, int64_t m, int64_t k, size_t* bytes) {
  if (!bytes || n < 1 || m < 1 || k < 1 || k > m || k > GPX_TOPK_SWEEP_MAX) return GPX_INVALID_ARG;
  *bytes = gpx::topk_multi_layout(padded(n), m, k, gpx::topk_workspace_bytes(m)).total;
  return GPX_OK;
}

gpx_status gpx_acquire_topk_multi_f64(gpx_handle h, const gpx_kernel_params* p, int64_t T, int64_t n, const double* X,
                                      int64_t ldx, const double* const* W_host, const int64_t* ldw_host,
                                      const double* const* alpha_host, const double* weights_host,
                                      const double* y_mean_host, const double* y_scale_host, const double* Xs,
                                      int64_t m, int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, int64_t k,
                                      double* val_out, int64_t* idx_out, void* ws, size_t ws_bytes) {
  if (h && k == 0) return fail(reinterpret_cast<Context*>(h), GPX_INVALID_ARG, "k must be >= 1");
  return acquire_multi_impl(h, p, T, n, X, ldx, W_host, ldw_host, alpha_host, weights_host, y_mean_host, y_scale_host,
                            Xs, m, ldxs, a, index_offset, nullptr, nullptr, nullptr, ws, ws_bytes, k, val_out, idx_out);
}

gpx_status gpx_argmax_combine_f64(gpx_handle h, const double* vals, const int64_t* idx, int64_t count,
                                  double* best_val, int64_t* best_idx) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (count < 1) return fail(c, GPX_INVALID_ARG, "count must be >= 1");
  GPX_NONNULL(c, vals);
  GPX_NONNULL(c, idx);
  GPX_NONNULL(c, best_val);
  GPX_NONNULL(c, best_idx);
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_argmax_final(c, vals, idx, count, best_val, best_idx), "argmax_combine");
}

// ---- SVGP predictive + pool-scan selection --------------------------------------
// The workspaces of the prepare, fit and gradient calls: gpx_svgp_layout.h.
namespace {
using gpx::SvgpWorkspace;
using gpx::up128;
gpx_status check_svgp(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t M) {
  if (ntask < 1 || ntask > 64) return fail(c, GPX_INVALID_ARG, "ntask must be in [1, 64]");
  if (M < 1 || M > 65536) return fail(c, GPX_INVALID_ARG, "number of inducing points must be in [1, 65536]");
  if (!p) return fail(c, GPX_INVALID_ARG, "kernel params pointer is NULL");
  for (int64_t t = 0; t < ntask; ++t) {
    GPX_TRY(check_params(c, p + t));
    if (p[t].d != p[0].d) return fail(c, GPX_INVALID_ARG, "all tasks must share the input dimension");
  }
  return GPX_OK;
}
// W = (chol(K_ZZ + jitter I))^{-T} per task, batched over the tasks: K_ZZ into the tasks' A (the hyperparameters differ
// per task; the likelihood noise is not part of K_ZZ), its factor in place, the inverse's transpose into W (wpitch
// doubles between tasks).  *bt: the batch strides of the two launches.
gpx_status svgp_inducing_factor(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t M, int64_t Mpad,
                                double jitter, const double* Z, int64_t ldz, int64_t stride_z, const SvgpWorkspace& w,
                                double* W, int64_t wpitch, int32_t* info, gpx::Batch* bt) {
  for (int64_t t = 0; t < ntask; ++t) {
    gpx_kernel_params q = p[t];
    q.noise = 0.0;
    q.jitter = jitter;
    GPX_TRY(hip_check(c, gpx::launch_gram(c, q, (int)M, (int)Mpad, Z + t * stride_z, ldz, w.task(t, gpx::SV_A), Mpad),
                      "gram"));
  }
  bt->count = (int)ntask;
  bt->k = bt->dinv = bt->ws = w.pitch();
  bt->w = wpitch;
  GPX_TRY(hip_check(c, gpx::launch_potrf(c, (int)Mpad, w.task(0, gpx::SV_A), Mpad, w.task(0, gpx::SV_DINV), info, *bt),
                    "potrf"));
  return hip_check(c, gpx::launch_trtri(c, (int)Mpad, w.task(0, gpx::SV_A), Mpad, w.task(0, gpx::SV_DINV), W, Mpad,
                                        w.task(0, gpx::SV_SLICE), *bt),
                   "trtri");
}
}  // namespace

gpx_status gpx_svgp_prepare_workspace_size(int64_t M, int64_t ntask, size_t* bytes) {
  if (!bytes || M < 1 || ntask < 1) return GPX_INVALID_ARG;
  *bytes = gpx::svgp_layout(gpx::SVGP_PREPARE, padded(M), ntask).total + 256;
  return GPX_OK;
}

gpx_status gpx_svgp_prepare_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                const double* Z, int64_t ldz, int64_t stride_z, const double* vmean,
                                int64_t stride_m, const double* vchol, int64_t ldc, int64_t stride_c, double* W,
                                double* W2, double* alpha, int32_t* info, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_svgp(c, p, ntask, M));
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, vmean);
  GPX_NONNULL(c, vchol);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, W2);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  if (!(jitter >= 0.0)) return fail(c, GPX_INVALID_ARG, "jitter must be non-negative");
  GPX_TRY(check_ld(c, ldz, p[0].d, "Z", false));
  GPX_TRY(check_ld(c, ldc, M, "chol_variational_covar", false));
  if (ntask > 1 && (stride_z < M * ldz || stride_m < M || stride_c < M * ldc))
    return fail(c, GPX_INVALID_ARG, "task strides smaller than one task");
  const int64_t Mpad = padded(M);
  size_t need = 0;
  GPX_TRY(gpx_svgp_prepare_workspace_size(M, ntask, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "svgp prepare workspace too small");
  GPX_USE_DEVICE(c);
  const SvgpWorkspace w(ws, gpx::svgp_layout(gpx::SVGP_PREPARE, Mpad, ntask));
  GPX_TRY(hip_check(c, hipMemsetAsync(info, 0, sizeof(int32_t) * ntask, c->stream), "memset info"));
  gpx::Batch bt;
  GPX_TRY(svgp_inducing_factor(c, p, ntask, M, Mpad, jitter, Z, ldz, stride_z, w, W, Mpad * Mpad, info, &bt));
  // zero-padded m and S = tril(chol) in the workspace, then alpha' = W m and W2 = W S
  GPX_TRY(hip_check(c, gpx::launch_svgp_pad(c, (int)ntask, (int)M, (int)Mpad, vmean, stride_m, vchol, ldc, stride_c,
                                            w.task(0, gpx::SV_MPAD), w.task(0, gpx::SV_SPAD), w.pitch()),
                    "svgp pad"));
  gpx::Batch tv;
  tv.count = (int)ntask;
  tv.w = Mpad * Mpad;
  tv.y = w.pitch();
  tv.alpha = Mpad;
  GPX_TRY(hip_check(c, gpx::launch_trmv_upper(c, (int)Mpad, W, Mpad, w.task(0, gpx::SV_MPAD), alpha, tv), "alpha'"));
  return hip_check(c, gpx::launch_svgp_w2(c, (int)ntask, (int)Mpad, W, w.task(0, gpx::SV_SPAD), w.pitch(), W2),
                   "svgp W2");
}

gpx_status gpx_svgp_predict_workspace_size(int64_t M, int64_t m, size_t* bytes) {
  if (!bytes || M < 1 || m < 1) return GPX_INVALID_ARG;
  const int64_t Mpad = padded(M);
  const gpx::SweepLayout L = gpx::sweep_layout(Mpad, 1, m);
  *bytes = L.total + (size_t)(Mpad / 128) * L.C * 8 + 512;
  return GPX_OK;
}

gpx_status gpx_svgp_predict_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                const double* Xs, int64_t m, int64_t ldxs, double min_var, double* mean_out,
                                int64_t ldmean, double* var_out, int64_t ldvar, double* score_out, void* ws,
                                size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_svgp(c, p, ntask, M));
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, W2);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, Xs);
  GPX_NONNULL(c, ws);
  if (m < 1) return fail(c, GPX_INVALID_ARG, "m must be >= 1");
  if (!mean_out && !var_out && !score_out) return fail(c, GPX_INVALID_ARG, "no output requested");
  if (!(min_var >= 0.0)) return fail(c, GPX_INVALID_ARG, "min_var must be non-negative");
  GPX_TRY(check_ld(c, ldz, p[0].d, "Z", false));
  GPX_TRY(check_ld(c, ldxs, p[0].d, "Xs", false));
  if (mean_out) GPX_TRY(check_ld(c, ldmean, ntask, "mean", false));
  if (var_out) GPX_TRY(check_ld(c, ldvar, ntask, "var", false));
  if (ntask > 1 && stride_z < M * ldz) return fail(c, GPX_INVALID_ARG, "task stride of Z smaller than one task");
  const int64_t Mpad = padded(M);
  size_t need = 0;
  GPX_TRY(gpx_svgp_predict_workspace_size(M, m, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "svgp predict workspace too small");
  const gpx::SweepWorkspace w = gpx::sweep_carve(ws, gpx::sweep_layout(Mpad, 1, m));
  const gpx::SweepBuffers& b = w.b;
  double* ss2 = w.after_main;  // (over the pruned part of the sweep's layout, which this call does not use)
  GPX_USE_DEVICE(c);
  for (int64_t s = 0; s < m; s += b.chunk) {
    const int64_t mc = (m - s) < b.chunk ? (m - s) : b.chunk;
    for (int64_t t = 0; t < ntask; ++t) {
      GPX_TRY(hip_check(c,
                        gpx::launch_svgp_chunk(c, p[t], min_var, (int)t, (int)M, (int)Mpad, Z + t * stride_z, ldz,
                                               W + t * Mpad * Mpad, W2 + t * Mpad * Mpad, Mpad, alpha + t * Mpad,
                                               Xs + s * ldxs, ldxs, mc, b, ss2, mean_out ? mean_out + s * ldmean : nullptr,
                                               ldmean, var_out ? var_out + s * ldvar : nullptr, ldvar,
                                               score_out ? score_out + s : nullptr),
                        "svgp predict"));
    }
  }
  return GPX_OK;
}

gpx_status gpx_svgp_acquire_workspace_size(int64_t M, int64_t m, int64_t k, size_t* bytes) {
  if (!bytes || M < 1 || M > 65536 || m < 1 || m > ((int64_t)1 << 30) || k < 1 || k > m) return GPX_INVALID_ARG;
  *bytes = gpx::svgp_acquire_layout(padded(M), m, gpx::topk_workspace_bytes(m)).total;
  return GPX_OK;
}

gpx_status gpx_svgp_acquire_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                const double* weights_host, const double* y_mean_host, const double* y_scale_host,
                                const double* Xs, int64_t m, int64_t ldxs, const gpx_acq_params* a,
                                int64_t index_offset, int64_t k, double* val_out, int64_t* idx_out, double* scores_out,
                                void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_svgp(c, p, ntask, M));
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, W2);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, weights_host);
  GPX_NONNULL(c, Xs);
  GPX_NONNULL(c, val_out);
  GPX_NONNULL(c, idx_out);
  GPX_NONNULL(c, ws);
  for (int64_t t = 0; t < ntask; ++t) {
    if (!std::isfinite(weights_host[t])) return fail(c, GPX_INVALID_ARG, "objective weights must be finite");
    if (y_scale_host && !(y_scale_host[t] > 0.0)) return fail(c, GPX_INVALID_ARG, "y_scale must be positive");
  }
  if (m < 1 || m > ((int64_t)1 << 30)) return fail(c, GPX_INVALID_ARG, "m must be in [1, 2^30]");
  GPX_TRY(check_acq(c, a, index_offset, false));
  if (k < 1 || k > m) return fail(c, GPX_INVALID_ARG, "k must be in [1, m]");
  GPX_TRY(check_ld(c, ldz, p[0].d, "Z", false));
  GPX_TRY(check_ld(c, ldxs, p[0].d, "Xs", false));
  if (ntask > 1 && stride_z < M * ldz) return fail(c, GPX_INVALID_ARG, "task stride of Z smaller than one task");
  const int64_t Mpad = padded(M);
  const gpx::SvgpAcquireLayout A = gpx::svgp_acquire_layout(Mpad, m, gpx::topk_workspace_bytes(m));
  if (ws_bytes < A.total) return fail(c, GPX_INVALID_ARG, "svgp acquire workspace too small");
  const gpx::SweepBuffers b = gpx::sweep_carve(ws, A.sweep).b;
  char* base = reinterpret_cast<char*>(gpx::up256(reinterpret_cast<uintptr_t>(ws)));
  auto dbl = [&](gpx::SvgpAcquireRegion id) { return reinterpret_cast<double*>(base + A.r[id].at); };
  double* ss2 = dbl(gpx::SQ_SS2_PART);
  double* scores = scores_out ? scores_out : dbl(gpx::SQ_SCORES);
  gpx::MultiOutput mo;
  mo.acc_mu = dbl(gpx::SQ_ACC_MU);
  mo.acc_var = dbl(gpx::SQ_ACC_VAR);
  GPX_USE_DEVICE(c);
  int64_t rec = 0;
  for (int64_t s = 0; s < m; s += b.chunk) {
    const int64_t mc = (m - s) < b.chunk ? (m - s) : b.chunk;
    for (int64_t t = 0; t < ntask; ++t) {
      mo.weight = weights_host[t];
      mo.y_mean = y_mean_host ? y_mean_host[t] : 0.0;
      mo.y_scale = y_scale_host ? y_scale_host[t] : 1.0;
      mo.first = t == 0;
      GPX_TRY(hip_check(c,
                        gpx::launch_svgp_chunk(c, p[t], 0.0, (int)t, (int)M, (int)Mpad, Z + t * stride_z, ldz,
                                               W + t * Mpad * Mpad, W2 + t * Mpad * Mpad, Mpad, alpha + t * Mpad,
                                               Xs + s * ldxs, ldxs, mc, b, ss2, nullptr, 0, nullptr, 0, nullptr, &mo),
                        "svgp acquire"));
    }
    // the accumulators' score pass: the chunk's scores; its block records are not read (the selection below sorts the scores)
    GPX_TRY(hip_check(c, gpx::launch_multi_score(c, {nullptr, 0, mc, index_offset + s}, mo, *a, scores + s,
                                                 b.rec_val + rec, b.rec_idx + rec),
                      "svgp acquire (score)"));
    rec += (mc + 255) / 256;
  }
  GPX_TRY(hip_check(c, gpx::launch_topk(c, scores, m, k, idx_out, val_out, base + A.r[gpx::SQ_SORT_WS].at,
                                        A.r[gpx::SQ_SORT_WS].bytes),
                    "svgp acquire (topk)"));
  return hip_check(c, gpx::launch_index_shift(c, idx_out, k, index_offset), "svgp acquire (indices)");
}

gpx_status gpx_svgp_moments_grad_workspace_size(int64_t M, int64_t m, size_t* bytes) {
  if (!bytes || M < 1 || M > 65536 || m < 1 || m > GPX_MAX_GRAD_CANDIDATES) return GPX_INVALID_ARG;
  *bytes = gpx::svgp_moments_ws_doubles((int)padded(M), (int)m) * sizeof(double) + 256;
  return GPX_OK;
}

gpx_status gpx_svgp_moments_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t M, const double* Z, int64_t ldz,
                                     const double* W, const double* W2, const double* alpha, const double* Xs,
                                     int64_t m, int64_t q, int64_t ldxs, double* mean, double* dmean, double* cov,
                                     double* dcov, void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_svgp(c, p, 1, M));
  if (m < 1 || m > GPX_MAX_GRAD_CANDIDATES) return fail(c, GPX_INVALID_ARG, "m must be in [1, GPX_MAX_GRAD_CANDIDATES]");
  if (q < 1 || q > GPX_MAX_Q || m % q != 0) return fail(c, GPX_INVALID_ARG, "q must be in [1, GPX_MAX_Q] and divide m");
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, W2);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, Xs);
  GPX_NONNULL(c, mean);
  GPX_NONNULL(c, cov);
  GPX_NONNULL(c, ws);
  if ((dmean == nullptr) != (dcov == nullptr))
    return fail(c, GPX_INVALID_ARG, "dmean and dcov must both be set or both be NULL");
  GPX_TRY(check_ld(c, ldz, p->d, "Z", false));
  GPX_TRY(check_ld(c, ldxs, p->d, "Xs", false));
  size_t need = 0;
  GPX_TRY(gpx_svgp_moments_grad_workspace_size(M, m, &need));
  if (ws_bytes < need) return fail(c, GPX_INVALID_ARG, "svgp moments_grad workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_svgp_moments(c, *p, (int)M, (int)padded(M), Z, ldz, W, W2, alpha, Xs, ldxs, (int)m,
                                               (int)q, mean, dmean, cov, dcov, align256(ws)),
                   "svgp moments_grad");
}

// ---- SVGP variational posterior in closed form (gpx_svgpfit.hip) and the hyperparameter gradient of its
// ---- bound (gpx_svgpgrad.hip): the gradient call is the fit's launches up to m', then a second pass over X ----------
namespace {
// The chunk width a size function reports for: the default, or `chunk` rounded up to 128.  0: invalid arguments.
int64_t svgp_size_chunk(int64_t M, int64_t n, int64_t ntask, int64_t chunk, const size_t* bytes) {
  if (!bytes || M < 1 || M > 65536 || n < 1 || ntask < 1 || ntask > 64 || chunk < 0 || chunk > ((int64_t)1 << 20))
    return 0;
  return chunk == 0 ? GPX_SVGP_FIT_CHUNK : up128(chunk);
}
// The argument checks of the fit and of the gradient.  outs: the call's own outputs, under the names the messages give
// them.  q: the fit's {stride_m, ldc, stride_c} of the variational outputs; null in the gradient, which has none.
gpx_status check_svgp_data(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                           const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n, int64_t ldx,
                           const double* Y, int64_t ldy,
                           std::initializer_list<std::pair<const void*, const char*>> outs, const int32_t* info,
                           const void* ws, const int64_t* q) {
  GPX_TRY(check_svgp(c, p, ntask, M));
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, Y);
  for (const auto& o : outs)
    if (!o.first) return fail(c, GPX_INVALID_ARG, std::string(o.second) + " is NULL");
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  if (!(jitter >= 0.0)) return fail(c, GPX_INVALID_ARG, "jitter must be non-negative");
  if (n < 1 || n > ((int64_t)1 << 40)) return fail(c, GPX_INVALID_ARG, "n must be in [1, 2^40]");
  GPX_TRY(check_ld(c, ldz, p[0].d, "Z", false));
  GPX_TRY(check_ld(c, ldx, p[0].d, "X", false));
  GPX_TRY(check_ld(c, ldy, ntask, "Y", false));
  if (q) {
    GPX_TRY(check_ld(c, q[1], M, "chol_variational_covar", false));
    if (ntask > 1 && (stride_z < M * ldz || q[0] < M || q[2] < M * q[1]))
      return fail(c, GPX_INVALID_ARG, "task strides smaller than one task");
  } else if (ntask > 1 && stride_z < M * ldz) {
    return fail(c, GPX_INVALID_ARG, "task stride of Z smaller than one task");
  }
  for (int64_t t = 0; t < ntask; ++t)
    if (!(p[t].noise > 0.0)) return fail(c, GPX_INVALID_ARG, "the likelihood noise must be positive");
  return GPX_OK;
}
gpx_status svgp_system_tail(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t Mpad, const int32_t* info,
                            int32_t* info2, const SvgpWorkspace& w, const gpx::Batch& bt);
// The fit's launches up to m' (arguments checked by the entry points; the device is current): on return, per task, A
// holds L' (B' = L' L'^T), Wb holds W' = L'^{-T}, and bvec / u / mrev / scal are final.  Where the layout has Wk and Bc
// (the gradient's), they get copies of W = L_ZZ^{-T} and of B' before those are overwritten.
gpx_status svgp_fit_core(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t M, int64_t Mpad, double jitter,
                         const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n, int64_t ldx,
                         const double* Y, int64_t ldy, int32_t* info, const SvgpWorkspace& w, int64_t C) {
  using namespace gpx;  // (the region names)
  const int64_t ldk = w.L.ldk, tstride = w.pitch(), pstride = w.phi_pitch();
  int32_t* info2 = w.shared<int32_t>(SV_INFO2);
  GPX_TRY(hip_check(c, hipMemsetAsync(info, 0, sizeof(int32_t) * ntask, c->stream), "memset info"));
  GPX_TRY(hip_check(c, hipMemsetAsync(info2, 0, sizeof(int32_t) * ntask, c->stream), "memset info"));
  GPX_TRY(hip_check(c, hipMemsetAsync(w.shared(SV_ZERO), 0, (size_t)Mpad * 8, c->stream), "memset"));
  Batch bt;
  GPX_TRY(svgp_inducing_factor(c, p, ntask, M, Mpad, jitter, Z, ldz, stride_z, w, w.task(0, SV_WB), tstride, info,
                               &bt));
  if (w.task(0, SV_WK))  // (W' will overwrite W below)
    for (int64_t t = 0; t < ntask; ++t)
      GPX_TRY(hip_check(c, hipMemcpyAsync(w.task(t, SV_WK), w.task(t, SV_WB), (size_t)Mpad * Mpad * 8,
                                          hipMemcpyDeviceToDevice, c->stream), "keep W"));
  // the accumulators: B_acc over the factor (no longer needed), b_acc and the scalar sums
  for (int64_t t = 0; t < ntask; ++t) {
    GPX_TRY(hip_check(c, hipMemsetAsync(w.task(t, SV_A), 0, (size_t)Mpad * Mpad * 8, c->stream), "memset"));
    GPX_TRY(hip_check(c, hipMemsetAsync(w.task(t, w.L.acc), 0, w.L.acc.bytes, c->stream), "memset"));
  }
  // chunks outside, tasks inside: one fixed order of accumulation per task
  for (int64_t s = 0; s < n; s += C) {
    const int64_t mc = (n - s) < C ? (n - s) : C;
    for (int64_t t = 0; t < ntask; ++t) {
      GPX_TRY(hip_check(c,
                        launch_svgp_kchunk(c, p[t], (int)M, (int)Mpad, Z + t * stride_z, ldz, w.shared(SV_ZERO),
                                           X + s * ldx, ldx, mc, ldk, w.shared(SV_KC), w.shared(SV_MU)),
                        "svgp fit covariance"));
      GPX_TRY(hip_check(c,
                        launch_svgp_fit_project(c, p[t], (int)Mpad, w.task(t, SV_WB), w.shared(SV_KC),
                                                w.shared(SV_PHI) + t * pstride, ldk, X + s * ldx, ldx, Y + s * ldy + t,
                                                ldy, (int)mc, w.shared(SV_R), w.task(t, SV_BVEC), w.task(t, SV_SCAL)),
                        "svgp fit projection"));
    }
    GPX_TRY(hip_check(c,
                      launch_svgp_fit_syrk(c, (int)ntask, (int)Mpad, w.shared(SV_PHI), pstride, ldk, (int)mc,
                                           w.task(0, SV_A), tstride),
                      "svgp fit rank update"));
  }
  return svgp_system_tail(c, p, ntask, Mpad, info, info2, w, bt);
}
// The tail of the fit and of the conditioning call behind their chunk loops: from the tasks' accumulators B_acc (in A)
// and b_acc (in bvec), B' = I + B_acc / s2 = L' L'^T and W' = L'^{-T} (in reversed index order), batched over the tasks,
// then u and m'.  info: the words svgp_bfinal_kernel reads (a task with info != 0 gets B' = I, b' = 0); info2: the
// factorisation's (they may be the same words: the launches run in stream order).
gpx_status svgp_system_tail(Context* c, const gpx_kernel_params* p, int64_t ntask, int64_t Mpad, const int32_t* info,
                            int32_t* info2, const SvgpWorkspace& w, const gpx::Batch& bt) {
  using namespace gpx;  // (the region names)
  const int64_t tstride = w.pitch();
  for (int64_t t = 0; t < ntask; ++t)
    GPX_TRY(hip_check(c,
                      launch_svgp_fit_system(c, (int)Mpad, p[t].noise, info + t, w.task(t, SV_A), w.task(t, SV_BVEC),
                                             w.task(t, SV_SCAL)),
                      "svgp fit system"));
  if (w.task(0, SV_BC))  // (B' on its lower 128-tiles, the others 0, before its factor overwrites it)
    for (int64_t t = 0; t < ntask; ++t)
      GPX_TRY(hip_check(c, hipMemcpyAsync(w.task(t, SV_BC), w.task(t, SV_A), (size_t)Mpad * Mpad * 8,
                                          hipMemcpyDeviceToDevice, c->stream), "keep B"));
  GPX_TRY(hip_check(c, launch_potrf(c, (int)Mpad, w.task(0, SV_A), Mpad, w.task(0, SV_DINV), info2, bt), "potrf B"));
  GPX_TRY(hip_check(c, launch_trtri(c, (int)Mpad, w.task(0, SV_A), Mpad, w.task(0, SV_DINV), w.task(0, SV_WB), Mpad,
                                    w.task(0, SV_SLICE), bt),
                    "trtri B"));
  // u = W'^T b', m' = W' u
  GPX_TRY(hip_check(c,
                    launch_svgp_fit_utvec(c, (int)ntask, (int)Mpad, w.task(0, SV_WB), tstride, w.task(0, SV_BVEC),
                                          w.task(0, SV_U), tstride),
                    "svgp fit u"));
  Batch tv;
  tv.count = (int)ntask;
  tv.w = tv.y = tv.alpha = tstride;
  return hip_check(c, launch_trmv_upper(c, (int)Mpad, w.task(0, SV_WB), Mpad, w.task(0, SV_U), w.task(0, SV_MREV), tv),
                   "svgp fit mean");
}
}  // namespace

gpx_status gpx_svgp_fit_collapsed_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes) {
  int64_t C = svgp_size_chunk(M, n, ntask, chunk, bytes);
  if (!C) return GPX_INVALID_ARG;
  if (C > up128(n)) C = up128(n);
  *bytes = gpx::svgp_layout(gpx::SVGP_FIT, padded(M), ntask, C).total + 256;
  return GPX_OK;
}

gpx_status gpx_svgp_fit_collapsed_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                      const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                      int64_t ldx, const double* Y, int64_t ldy, double* vmean, int64_t stride_m,
                                      double* vchol, int64_t ldc, int64_t stride_c, double* bound, int32_t* info,
                                      void* ws, size_t ws_bytes) {
  using namespace gpx;  // (the region names)
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  const int64_t q[3] = {stride_m, ldc, stride_c};
  GPX_TRY(check_svgp_data(c, p, ntask, M, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy,
                          {{vmean, "vmean"}, {vchol, "vchol"}, {bound, "bound"}}, info, ws, q));
  const int64_t Mpad = padded(M);
  const int64_t C = svgp_chunk_width(SVGP_FIT, Mpad, ntask, n, GPX_SVGP_FIT_CHUNK, ws_bytes);
  if (!C) return fail(c, GPX_INVALID_ARG, "svgp fit workspace too small");
  const SvgpWorkspace w(ws, svgp_layout(SVGP_FIT, Mpad, ntask, C));
  GPX_USE_DEVICE(c);
  GPX_TRY(svgp_fit_core(c, p, ntask, M, Mpad, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, info, w, C));
  for (int64_t t = 0; t < ntask; ++t)
    GPX_TRY(hip_check(c,
                      launch_svgp_fit_finish(c, (int)M, (int)Mpad, n, p[t].noise, w.task(t, SV_A), w.task(t, SV_WB),
                                             w.task(t, SV_U), w.task(t, SV_MREV), w.task(t, SV_SCAL),
                                             vmean + t * stride_m, vchol + t * stride_c, ldc,
                                             bound + t * GPX_SVGP_BOUND_NOUT),
                      "svgp fit finish"));
  return GPX_OK;
}

// ---- Conditioning the sparse model on new data (gpx_svgpcond.hip): the fit's chunk loop with W2^T K in
// ---- Phi's place and the residual against the current mean, the shared tail, then the compose products ------------
gpx_status gpx_svgp_condition_workspace_size(int64_t M, int64_t n_new, int64_t ntask, int64_t chunk, size_t* bytes) {
  int64_t C = svgp_size_chunk(M, n_new, ntask, chunk, bytes);
  if (!C || n_new > ((int64_t)1 << 30)) return GPX_INVALID_ARG;
  if (C > up128(n_new)) C = up128(n_new);
  *bytes = gpx::svgp_layout(gpx::SVGP_CONDITION, padded(M), ntask, C).total + 256;
  return GPX_OK;
}

gpx_status gpx_svgp_condition_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                  int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                  const double* Xn, int64_t n_new, int64_t ldx, const double* Yn, int64_t ldy,
                                  double* W2_out, double* alpha_out, const double* vmean, int64_t stride_m,
                                  const double* vchol, int64_t ldc, int64_t stride_c, double* vmean_out,
                                  double* vchol_out, int32_t* info, void* ws, size_t ws_bytes) {
  using namespace gpx;  // (the region names)
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_TRY(check_svgp(c, p, ntask, M));
  GPX_NONNULL(c, Z);
  GPX_NONNULL(c, W);
  GPX_NONNULL(c, W2);
  GPX_NONNULL(c, alpha);
  GPX_NONNULL(c, Xn);
  GPX_NONNULL(c, Yn);
  GPX_NONNULL(c, W2_out);
  GPX_NONNULL(c, alpha_out);
  GPX_NONNULL(c, info);
  GPX_NONNULL(c, ws);
  const int nvar = (vmean != nullptr) + (vchol != nullptr) + (vmean_out != nullptr) + (vchol_out != nullptr);
  if (nvar != 0 && nvar != 4)
    return fail(c, GPX_INVALID_ARG, "vmean, vchol, vmean_out and vchol_out must all be set or all be NULL");
  const bool var = nvar == 4;
  if (n_new < 1 || n_new > ((int64_t)1 << 30)) return fail(c, GPX_INVALID_ARG, "n_new must be in [1, 2^30]");
  GPX_TRY(check_ld(c, ldz, p[0].d, "Z", false));
  GPX_TRY(check_ld(c, ldx, p[0].d, "Xn", false));
  GPX_TRY(check_ld(c, ldy, ntask, "Yn", false));
  if (ntask > 1 && stride_z < M * ldz) return fail(c, GPX_INVALID_ARG, "task stride of Z smaller than one task");
  if (var) {
    GPX_TRY(check_ld(c, ldc, M, "chol_variational_covar", false));
    if (ntask > 1 && (stride_m < M || stride_c < M * ldc))
      return fail(c, GPX_INVALID_ARG, "task strides smaller than one task");
  }
  for (int64_t t = 0; t < ntask; ++t)
    if (!(p[t].noise > 0.0)) return fail(c, GPX_INVALID_ARG, "the likelihood noise must be positive");
  if (W2_out == W2 || alpha_out == alpha || (var && (vmean_out == vmean || vchol_out == vchol)))
    return fail(c, GPX_INVALID_ARG, "the outputs must not alias the state they are computed from");
  const int64_t Mpad = padded(M);
  const int64_t C = svgp_chunk_width(SVGP_CONDITION, Mpad, ntask, n_new, GPX_SVGP_FIT_CHUNK, ws_bytes);
  if (!C) return fail(c, GPX_INVALID_ARG, "svgp condition workspace too small");
  const SvgpWorkspace w(ws, svgp_layout(SVGP_CONDITION, Mpad, ntask, C));
  const int64_t ldk = w.L.ldk, tstride = w.pitch(), pstride = w.phi_pitch(), mat = Mpad * Mpad;
  GPX_USE_DEVICE(c);
  GPX_TRY(hip_check(c, hipMemsetAsync(info, 0, sizeof(int32_t) * ntask, c->stream), "memset info"));
  // the accumulators: P_acc, b_acc and the scalar sums
  for (int64_t t = 0; t < ntask; ++t) {
    GPX_TRY(hip_check(c, hipMemsetAsync(w.task(t, SV_A), 0, (size_t)mat * 8, c->stream), "memset"));
    GPX_TRY(hip_check(c, hipMemsetAsync(w.task(t, w.L.acc), 0, w.L.acc.bytes, c->stream), "memset"));
  }
  // chunks outside, tasks inside, as in the fit: one fixed order of accumulation per task
  for (int64_t s = 0; s < n_new; s += C) {
    const int64_t mc = (n_new - s) < C ? (n_new - s) : C;
    for (int64_t t = 0; t < ntask; ++t) {
      GPX_TRY(hip_check(c,
                        launch_svgp_kchunk(c, p[t], (int)M, (int)Mpad, Z + t * stride_z, ldz, alpha + t * Mpad,
                                           Xn + s * ldx, ldx, mc, ldk, w.shared(SV_KC), w.shared(SV_MU)),
                        "svgp condition covariance"));
      GPX_TRY(hip_check(c,
                        launch_svgp_cond_resid(c, p[t].const_mean, Yn + s * ldy + t, ldy, (int)mc, w.shared(SV_MU), ldk,
                                               (int)(Mpad / gpx::NB), w.shared(SV_R)),
                        "svgp condition residual"));
      GPX_TRY(hip_check(c,
                        launch_svgp_cond_project(c, (int)Mpad, W2 + t * mat, w.shared(SV_KC),
                                                 w.shared(SV_PHI) + t * pstride, ldk, (int)mc, w.shared(SV_R),
                                                 w.task(t, SV_BVEC)),
                        "svgp condition projection"));
    }
    GPX_TRY(hip_check(c,
                      launch_svgp_fit_syrk(c, (int)ntask, (int)Mpad, w.shared(SV_PHI), pstride, ldk, (int)mc,
                                           w.task(0, SV_A), tstride),
                      "svgp condition rank update"));
  }
  Batch bt;
  bt.count = (int)ntask;
  bt.k = bt.dinv = bt.ws = bt.w = tstride;
  GPX_TRY(svgp_system_tail(c, p, ntask, Mpad, info, info, w, bt));
  // W2_new = W2 D and C_new = C D with D = J W' J read in place; alpha'_new = alpha' + W2 g, m_new = m + C g
  GPX_TRY(hip_check(c,
                    launch_svgp_compose(c, (int)ntask, (int)M, (int)Mpad, W2, mat, w.task(0, SV_WB), tstride, W2_out,
                                        Mpad, mat, false),
                    "svgp condition W2"));
  if (var) {
    GPX_TRY(hip_check(c,
                      launch_svgp_cond_pad(c, (int)ntask, (int)M, (int)Mpad, vchol, ldc, stride_c, w.task(0, SV_SPAD),
                                           tstride),
                      "svgp condition pad"));
    GPX_TRY(hip_check(c,
                      launch_svgp_compose(c, (int)ntask, (int)M, (int)Mpad, w.task(0, SV_SPAD), tstride,
                                          w.task(0, SV_WB), tstride, vchol_out, ldc, stride_c, true),
                      "svgp condition chol"));
  }
  return hip_check(c,
                   launch_svgp_cond_finish(c, (int)ntask, (int)M, (int)Mpad, W2, alpha, w.task(0, SV_MREV), tstride,
                                           alpha_out, vmean, stride_m, vchol, ldc, stride_c, vmean_out, info),
                   "svgp condition finish");
}

gpx_status gpx_svgp_bound_grad_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes) {
  // (the size does not depend on n: a chunk wider than n only leaves columns unused)
  const int64_t C = svgp_size_chunk(M, n, ntask, chunk, bytes);
  if (!C) return GPX_INVALID_ARG;
  *bytes = gpx::svgp_layout(gpx::SVGP_GRAD, padded(M), ntask, C, GPX_MLL_NOUT).total + 256;
  return GPX_OK;
}

gpx_status gpx_svgp_bound_grad_z_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes) {
  const int64_t C = svgp_size_chunk(M, n, ntask, chunk, bytes);
  if (!C) return GPX_INVALID_ARG;
  *bytes = gpx::svgp_layout(gpx::SVGP_GRAD_Z, padded(M), ntask, C, GPX_MLL_NOUT, GPX_MAX_DIM).total + 256;
  return GPX_OK;
}

namespace {
// The driver of both gradient calls.  zg: gpx_svgp_bound_grad_z_f64, whose layout has the two regions of dF/dZ; the
// K_ZZ contraction and the chunks' tile contractions then also fill them (null pointers otherwise: not wanted).
// The fit's matrices are reused between the passes: A holds L', then T1 = I - S, then G_A; Wb holds W', then the
// products' intermediate U.
gpx_status svgp_bound_grad_driver(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                  const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                  int64_t ldx, const double* Y, int64_t ldy, double* out, bool zg, double* dZ,
                                  int64_t lddz, int64_t stride_dz, int32_t* info, void* ws, size_t ws_bytes) {
  using namespace gpx;  // (the region names)
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (zg)
    GPX_TRY(check_svgp_data(c, p, ntask, M, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, {{out, "out"}, {dZ, "dZ"}},
                            info, ws, nullptr));
  else
    GPX_TRY(check_svgp_data(c, p, ntask, M, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, {{out, "out"}}, info, ws,
                            nullptr));
  if (zg) {
    GPX_TRY(check_ld(c, lddz, p[0].d, "dZ", false));
    if (ntask > 1 && stride_dz < M * lddz) return fail(c, GPX_INVALID_ARG, "task stride of dZ smaller than one task");
  }
  const int64_t Mpad = padded(M);
  const SvgpKind kind = zg ? SVGP_GRAD_Z : SVGP_GRAD;
  const int64_t zdim = zg ? GPX_MAX_DIM : 0;
  const int64_t C = svgp_chunk_width(kind, Mpad, ntask, n, GPX_SVGP_FIT_CHUNK, ws_bytes, GPX_MLL_NOUT, zdim);
  if (!C) return fail(c, GPX_INVALID_ARG, "svgp bound gradient workspace too small");
  const SvgpWorkspace w(ws, svgp_layout(kind, Mpad, ntask, C, GPX_MLL_NOUT, zdim));
  const int64_t ldk = w.L.ldk, ts = w.pitch();
  GPX_USE_DEVICE(c);
  // pass 1: the fit, keeping W and B'; then the bound while L' and u are in place
  GPX_TRY(svgp_fit_core(c, p, ntask, M, Mpad, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, info, w, C));
  for (int64_t t = 0; t < ntask; ++t) {
    GPX_TRY(hip_check(c,
                      launch_svgp_fit_bound(c, (int)Mpad, n, p[t].noise, w.task(t, SV_A), w.task(t, SV_U),
                                            w.task(t, SV_SCAL), w.task(t, SV_BND)),
                      "svgp bound"));
    GPX_TRY(hip_check(c, hipMemsetAsync(w.task(t, w.L.acc2), 0, w.L.acc2.bytes, c->stream), "memset"));
  }
  // between the passes: T1 = I - S -> A, Q -> X1; H = W T1 W^T -> Bc; G_A = W Q W^T / 2 -> A; c_v = W m
  GPX_TRY(hip_check(c,
                    launch_svgp_grad_sq(c, (int)ntask, (int)Mpad, ts, w.task(0, SV_WB), w.task(0, SV_BC),
                                        w.task(0, SV_MREV), w.task(0, SV_A), w.task(0, SV_X1)),
                    "svgp grad S"));
  GPX_TRY(hip_check(c,
                    launch_svgp_grad_unreverse(c, (int)ntask, (int)Mpad, ts, w.task(0, SV_MREV), w.task(0, SV_A),
                                               w.task(0, SV_MNAT), w.task(0, SV_SC2)),
                    "svgp grad m"));
  Batch tv;
  tv.count = (int)ntask;
  tv.w = tv.y = tv.alpha = ts;
  GPX_TRY(hip_check(c,
                    launch_trmv_upper(c, (int)Mpad, w.task(0, SV_WK), Mpad, w.task(0, SV_MNAT), w.task(0, SV_CV), tv),
                    "svgp grad c_v"));
  GPX_TRY(hip_check(c,
                    launch_svgp_grad_conj(c, (int)ntask, (int)Mpad, ts, w.task(0, SV_WK), w.task(0, SV_A), 1.0,
                                          w.task(0, SV_WB), w.task(0, SV_BC)),
                    "svgp grad H"));
  GPX_TRY(hip_check(c,
                    launch_svgp_grad_conj(c, (int)ntask, (int)Mpad, ts, w.task(0, SV_WK), w.task(0, SV_X1), 0.5,
                                          w.task(0, SV_WB), w.task(0, SV_A)),
                    "svgp grad G_A"));
  for (int64_t t = 0; t < ntask; ++t)
    GPX_TRY(hip_check(c,
                      launch_svgp_grad_kzz(c, p[t], (int)M, (int)Mpad, Z + t * stride_z, ldz, w.task(t, SV_A),
                                           w.shared(SV_PART), w.task(t, SV_GACC), w.task(t, SV_ZACC)),
                      "svgp grad K_ZZ"));
  // pass 2: chunks outside, tasks inside, as in pass 1
  for (int64_t s = 0; s < n; s += C) {
    const int64_t mc = (n - s) < C ? (n - s) : C;
    for (int64_t t = 0; t < ntask; ++t) {
      GPX_TRY(hip_check(c,
                        launch_svgp_kchunk(c, p[t], (int)M, (int)Mpad, Z + t * stride_z, ldz, w.task(t, SV_CV),
                                           X + s * ldx, ldx, mc, ldk, w.shared(SV_KC), w.shared(SV_MU)),
                        "svgp grad covariance"));
      GPX_TRY(hip_check(c,
                        launch_svgp_grad_chunk(c, p[t], (int)M, (int)Mpad, Z + t * stride_z, ldz, w.task(t, SV_BC),
                                               w.shared(SV_KC), w.shared(SV_MU), ldk, X + s * ldx, ldx, Y + s * ldy + t,
                                               ldy, (int)mc, w.task(t, SV_CV), w.shared(SV_EV), w.task(t, SV_SC2),
                                               w.shared(SV_PART), w.task(t, SV_GACC), w.shared(SV_ZPART),
                                               w.task(t, SV_ZACC)),
                        "svgp grad chunk"));
    }
  }
  for (int64_t t = 0; t < ntask; ++t)
    GPX_TRY(hip_check(c,
                      launch_svgp_grad_finish(c, p[t], (int)M, n, w.task(t, SV_BND), w.task(t, SV_SCAL),
                                              w.task(t, SV_SC2), w.task(t, SV_GACC), out + t * GPX_SVGP_GRAD_NOUT,
                                              w.task(t, SV_ZACC), zg ? dZ + t * stride_dz : nullptr, lddz),
                      "svgp grad finish"));
  return GPX_OK;
}
}  // namespace

gpx_status gpx_svgp_bound_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                   const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                   int64_t ldx, const double* Y, int64_t ldy, double* out, int32_t* info, void* ws,
                                   size_t ws_bytes) {
  return svgp_bound_grad_driver(h, p, ntask, M, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, out, false, nullptr, 0, 0,
                                info, ws, ws_bytes);
}

gpx_status gpx_svgp_bound_grad_z_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                     const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                     int64_t ldx, const double* Y, int64_t ldy, double* out, double* dZ, int64_t lddz,
                                     int64_t stride_dz, int32_t* info, void* ws, size_t ws_bytes) {
  return svgp_bound_grad_driver(h, p, ntask, M, jitter, Z, ldz, stride_z, X, n, ldx, Y, ldy, out, true, dZ, lddz,
                                stride_dz, info, ws, ws_bytes);
}

gpx_status gpx_topk_workspace_size(int64_t m, size_t* bytes) {
  if (!bytes || m < 1 || m > ((int64_t)1 << 30)) return GPX_INVALID_ARG;
  *bytes = gpx::topk_workspace_bytes(m);
  return GPX_OK;
}

gpx_status gpx_topk_f64(gpx_handle h, const double* scores, int64_t m, int64_t k, int64_t* idx_out, double* val_out,
                        void* ws, size_t ws_bytes) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, scores);
  GPX_NONNULL(c, idx_out);
  GPX_NONNULL(c, ws);
  if (m < 1 || m > ((int64_t)1 << 30)) return fail(c, GPX_INVALID_ARG, "m must be in [1, 2^30]");
  if (k < 1 || k > m) return fail(c, GPX_INVALID_ARG, "k must be in [1, m]");
  if (ws_bytes < gpx::topk_workspace_bytes(m)) return fail(c, GPX_INVALID_ARG, "topk workspace too small");
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_topk(c, scores, m, k, idx_out, val_out, ws, ws_bytes), "topk");
}

gpx_status gpx_fps_f64(gpx_handle h, const double* X, int64_t m, int64_t d, int64_t ldx, int64_t k, int64_t start,
                       int64_t* idx_out) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  GPX_NONNULL(c, X);
  GPX_NONNULL(c, idx_out);
  if (m < 1 || m > 32 * 1024) return fail(c, GPX_INVALID_ARG, "fps supports 1 <= m <= 32768 points");
  if (d < 1 || d > GPX_MAX_DIM) return fail(c, GPX_INVALID_ARG, "d must be in [1, 32]");
  if (k < 1 || k > m) return fail(c, GPX_INVALID_ARG, "k must be in [1, m]");
  if (start < 0 || start >= m) return fail(c, GPX_INVALID_ARG, "start index outside [0, m)");
  GPX_TRY(check_ld(c, ldx, d, "X", false));
  GPX_USE_DEVICE(c);
  return hip_check(c, gpx::launch_fps(c, X, m, (int)d, ldx, k, start, idx_out), "fps");
}

gpx_status gpx_timing_enable(gpx_handle h, int32_t mask) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  c->timing_mask = mask;
  return GPX_OK;
}

gpx_status gpx_timing_reset(gpx_handle h) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (!c->pending.empty()) (void)hipStreamSynchronize(c->stream);
  for (auto& pt : c->pending) {
    c->free_events.push_back(pt.start);
    c->free_events.push_back(pt.stop);
  }
  c->pending.clear();
  for (int t = 0; t < GPX_TIMER_COUNT; ++t) {
    c->timer_ms[t] = 0.0;
    c->timer_launches[t] = 0;
  }
  return GPX_OK;
}

gpx_status gpx_timing_query(gpx_handle h, int32_t timer, double* total_ms_host, int64_t* launches_host) {
  Context* c = reinterpret_cast<Context*>(h);
  if (!c) return GPX_INVALID_ARG;
  if (timer < 0 || timer >= GPX_TIMER_COUNT) return fail(c, GPX_INVALID_ARG, "unknown timer");
  if (!c->pending.empty()) {
    GPX_TRY(hip_check(c, hipStreamSynchronize(c->stream), "timing sync"));
    for (auto& pt : c->pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pt.start, pt.stop) == hipSuccess) {
        c->timer_ms[pt.timer] += ms;
        c->timer_launches[pt.timer] += 1;
      }
      c->free_events.push_back(pt.start);
      c->free_events.push_back(pt.stop);
    }
    c->pending.clear();
  }
  if (total_ms_host) *total_ms_host = c->timer_ms[timer];
  if (launches_host) *launches_host = c->timer_launches[timer];
  return GPX_OK;
}

}  // extern "C"
