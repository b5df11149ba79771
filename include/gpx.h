/*
 * gpx.h — C ABI of the MI355X-native exact-GP posterior engine (libgpx.so).
 *
 * This is the drop-in boundary for the hot path of billbearhunter/BayesianOptimizer.  In the reference
 * the path runs inside BoTorch/GPyTorch (not vendored); each entry point below names the reference call
 * site whose arithmetic it replaces.  Python binds it with ctypes (bayesianoptimizer_amd/_capi.py); see
 * INTEGRATION.md for the binding stub a maintainer adds to the reference.
 *
 * Conventions
 *  - Every array pointer is a DEVICE pointer owned by the caller (PyTorch tensors serve as containers).
 *    Host pointers are only the parameter structs and the out-scalars named *_host.
 *  - All matrices are row-major fp64 with an explicit leading dimension (in elements).  The leading dimensions of the
 *    matrix arguments (K, L, W, Sb) must be even and at most GPX_MAX_LD.  Bytes of an output outside its defined
 *    region (pitch gaps, rows past the padded size, gaps between the problems of a batch) are never written.
 *  - Training size n is padded internally to gpx_padded_n(n) (a multiple of GPX_TILE); padded rows of K are
 *    the identity, so L, L^{-1} and alpha are exact block extensions of the unpadded ones.  Buffers named
 *    "padded" must have gpx_padded_n(n) rows/cols.
 *  - Calls are asynchronous on the handle's stream (gpx_set_stream) and never allocate device memory;
 *    scratch comes from the caller's workspace (size from the *_workspace_size queries).  The calls that say so
 *    synchronise; gpx_acquire_argmax_f64 and gpx_acquire_topk_f64 wait once for a 4-byte read-back in the calls
 *    described at gpx_debug_set_sweep_tail_sync.  A workspace's contents on
 *    entry are arbitrary, and its address needs only 8-byte alignment.
 *  - Errors: return a gpx_status; gpx_last_error(h) gives a message.  NOT_PD is reported through a device
 *    int32 `info` (0 = OK, > 0 failing pivot + 1, LAPACK potrf convention) so the fit stays asynchronous;
 *    gpx_fit_f64_sync reads it back and returns GPX_NOT_PD, like the reference's jitter-retry path
 *    (optimization/Bayesian6.py:481-488) expects an exception.  info = GPX_INFO_TIMEOUT (negative) means an
 *    in-launch hand-off of the factorisation or of the triangular solve gave up after its bounded spin
 *    (gpx_fit_f64_sync: GPX_TIMEOUT); the factor / alpha are then invalid.
 */
#ifndef GPX_H
#define GPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_MAX_DIM 32
#define GPX_MAX_RHS 8
#define GPX_TILE 128
#define GPX_MAX_LD (1 << 20)            /* leading dimension limit of the matrix arguments (K, L, W) */
#define GPX_MAX_Q 32                    /* q-batch size of gpx_moments_grad_f64 */
#define GPX_MAX_GRAD_CANDIDATES 16384  /* candidates per gpx_moments_grad_f64 call */
#define GPX_MAX_JOINT 8192             /* points per gpx_joint_moments_f64 call */
#define GPX_MAX_BASELINE 64            /* baseline points of gpx_cross_cov_grad_f64 / gpx_mc_nei_f64 */

typedef struct gpx_context* gpx_handle;
typedef struct gpx_comm_s* gpx_comm;   /* RCCL communicator of the cross-GPU record exchange */
#define GPX_COMM_ID_BYTES 128          /* ncclUniqueId */
typedef int32_t gpx_status;

enum {
  GPX_OK = 0,
  GPX_NOT_PD = 1,
  GPX_INVALID_ARG = 2,
  GPX_HIP_ERROR = 3,
  GPX_RCCL_ERROR = 4,
  GPX_TIMEOUT = 5 /* a persistent launch's hand-off timed out (device info = GPX_INFO_TIMEOUT) */
};
#define GPX_INFO_TIMEOUT ((int32_t)0x80000000)

/* Covariance modules used by the reference.
 * RBF: BoTorch SingleTaskGP default (optimization/Bayesian.py:91, Bayesian1.py:109) [upstream]
 * MATERN52: MaternKernel(nu=2.5) (config 3 of BASELINE.json)
 * SCALE_LINEAR_MATERN52: ScaleKernel(LinearKernel + MaternKernel(2.5)) (optimization/Bayesian6.py:471-473,
 *                        optimization/Bayesian7.py:162-166) */
enum { GPX_KERNEL_RBF = 0, GPX_KERNEL_MATERN52 = 1, GPX_KERNEL_SCALE_LINEAR_MATERN52 = 2 };

/* Acquisition scores (maximised). EI/LOGEI/UCB: BoTorch analytic forms [upstream] of the qLogEI call
 * (optimization/Bayesian.py:100-101); VARIANCE: the pool-scan score of optimization/Bayesian7.py:671.
 * With sigma = sqrt(var), u = (mu - best_f) / sigma:
 *   EI    = sigma (phi(u) + u Phi(u)), the plain sum as BoTorch's.  For u <= 0 its error is a few tens of eps of
 *           sigma phi(u) (1 + |u|), the size of the two terms that cancel, not of the result (~ sigma phi(u) / u^2).
 *           Below u ~ -37.5 Phi(u), then phi(u), are denormal: the result is then only bounded, 0 <= EI <= sigma phi(u)
 *           (never negative), and it is 0 from u ~ -38.6 down.  Use LOGEI where improvements that small matter.
 *   LOGEI = log EI in a stable form (the log of the sum down to u = -1, an erfcx form down to -1024, the asymptotic
 *           series below): within a few tens of eps of 1 + |LOGEI| for every finite u; -inf where u^2 overflows
 *           (|u| > 1.3e154). */
enum { GPX_ACQ_EI = 0, GPX_ACQ_LOGEI = 1, GPX_ACQ_UCB = 2, GPX_ACQ_VARIANCE = 3 };

/* Timers kept by gpx_timing_* (one per kernel family; gpx_timing_enable takes a bitmask of 1<<timer). */
enum {
  GPX_TIMER_GRAM = 0,
  GPX_TIMER_POTRF = 1,
  GPX_TIMER_TRTRI = 2,
  GPX_TIMER_ALPHA = 3,
  GPX_TIMER_KSTAR = 4,
  GPX_TIMER_TRMM = 5,
  GPX_TIMER_ACQ = 6,
  GPX_TIMER_MLL = 7,
  GPX_TIMER_COUNT = 8
};

/* Layout of the gpx_mll_grad_f64 output vector (GPX_MLL_NOUT doubles).  Gradients are of the negative log
 * marginal likelihood w.r.t. the natural (constrained) hyperparameters of gpx_kernel_params. */
enum {
  GPX_MLL_NLL = 0,            /* -log p(y) = QUAD + LOGDET/2 + n/2 log(2 pi) */
  GPX_MLL_QUAD = 1,           /* (y - m)^T K^{-1} (y - m) / 2 */
  GPX_MLL_LOGDET = 2,         /* log |K| = 2 sum log L_ii */
  GPX_MLL_D_NOISE = 3,
  GPX_MLL_D_OUTPUTSCALE = 4,
  GPX_MLL_D_MEAN = 5,
  GPX_MLL_D_LENGTHSCALE = 8,  /* GPX_MAX_DIM entries */
  GPX_MLL_D_LINVAR = 40,      /* GPX_MAX_DIM entries (SCALE_LINEAR_MATERN52 only) */
  GPX_MLL_NOUT = 72
};

typedef struct {
  int32_t kind;                          /* GPX_KERNEL_* */
  int32_t d;                             /* input dimension, 1..GPX_MAX_DIM */
  double lengthscale[GPX_MAX_DIM];       /* ARD lengthscales (Matérn / RBF part) */
  double linear_variance[GPX_MAX_DIM];   /* ARD LinearKernel variances (SCALE_LINEAR_MATERN52 only) */
  double outputscale;                    /* ScaleKernel s^2 (1.0 for BoTorch>=0.12 RBF default) */
  double noise;                          /* GaussianLikelihood noise sigma^2 */
  double jitter;                         /* extra diagonal (gpytorch.settings.cholesky_jitter) */
  double const_mean;                     /* ConstantMean */
  int32_t cov_fp32;                      /* 1: evaluate distances / exp / Matérn polynomial in fp32 (BASELINE
                                            configs[4] mixed-precision build), widen to fp64 before the fp64
                                            factorisation and sweep; 0: fp64 throughout */
  int32_t reserved;                      /* must be 0 */
} gpx_kernel_params;

typedef struct {
  int32_t kind;     /* GPX_ACQ_* */
  int32_t reserved; /* must be 0 */
  double best_f;    /* incumbent, in untransformed units (optimization/Bayesian.py:98) */
  double beta;      /* UCB beta */
  double y_mean;    /* Standardize untransform: mu_out = y_mean + y_scale * mu */
  double y_scale;   /*                          var_out = y_scale^2 * var       */
} gpx_acq_params;

/* ---- library / handle ---------------------------------------------------------------------------- */
const char* gpx_version(void);
gpx_status gpx_create(int32_t device, gpx_handle* out);
gpx_status gpx_destroy(gpx_handle h);
/* stream: a hipStream_t passed as void* (NULL = default stream). */
gpx_status gpx_set_stream(gpx_handle h, void* stream);
const char* gpx_last_error(gpx_handle h);
int64_t gpx_padded_n(int64_t n);
/* sizeof(gpx_kernel_params) (560) and sizeof(gpx_acq_params) (40) as compiled into the library: a binding checks its
 * own struct definitions against these once at load time.  Every entry point taking a
 * gpx_kernel_params also rejects cov_fp32 outside {0, 1} and reserved != 0 with GPX_INVALID_ARG. */
size_t gpx_kernel_params_size(void);
size_t gpx_acq_params_size(void);

/* Per-handle options (tuning and diagnostics; every default is the measured best).  gpx_create reads the environment
 * variable GPX_OPTIONS once ("name=value,name=value", names as below in lower case without the prefix, e.g.
 * "sweep_fused=0,potrf_mode=1"; an unknown name is reported on stderr and ignored); nothing else in the library reads
 * the environment.  The numbers are stable ABI: a removed option keeps its slot as GPX_OPT_RESERVED_n, which
 * gpx_set_option / gpx_get_option reject with GPX_INVALID_ARG.  The Cholesky schedule options (potrf_*) and gram_split
 * change no result bit: the schedules are arithmetic-invariant (any schedule that folds the forward substitution - every
 * default, and every potrf_mode 1 or potrf_lazy 1 setting - gives the same L, z and alpha; potrf_mode 0 with
 * potrf_lazy > 1 runs the forward substitution as a separate solve, so only alpha's rounding differs there).
 * sweep_fused = 0 takes the K* + trmm path at padded n <= 256, which sums in a different order: its results agree with
 * the fused path to the parity tolerance, not bit for bit.
 *  GPX_OPT_RESERVED_0      (was GPX_OPT_POTRF_SCHEDULE, removed in 0.4)
 *  GPX_OPT_SPIN_LIMIT      polls before an in-launch hand-off (the triangular solve's) gives up and
 *                          reports GPX_INFO_TIMEOUT (default 4194304; 0 = give up at the first unmet poll: tests)
 *  GPX_OPT_SWEEP_FUSED     1 (default) the fused small-n sweep where it applies (padded n <= 256), 0 the K* + trmm path
 *  GPX_OPT_GRAM_SPLIT      0 by size (default), else 1, 2 or 4 workgroups per 64x64 Gram tile
 *  GPX_OPT_POTRF_LAZY      multi-launch schedule: 0 by size and batch (default), else flush the trailing update every g columns
 *  GPX_OPT_POTRF_MODE      multi-launch schedule: -1 by size and batch (default), 0 eager panels, 1 lookahead panels
 *  GPX_OPT_POTRF_SWITCH    multi-launch schedule: -1 by size and batch (default), 0 no switch, k > 0: launches < k on
 *                          the lookahead schedule (flush every potrf_lazy, default 3 / by size), the rest eager (rounded
 *                          down to the launch after a flush)
 *  GPX_OPT_POTRF_SPLIT     panel row blocks per workgroup: -1 (default) split in 2 where the launch still fits the
 *                          co-resident slots, 1 never split, 3 split only where the split launch fits one workgroup per CU
 *  GPX_OPT_SWEEP_PRUNE     gpx_acquire_argmax_f64 without scores_out, and gpx_acquire_topk_f64, on the K* + trmm path: 1 (default) the pruned sweep
 *                          from padded n 384 on, 0 the full sweep, 2 the pruned sweep at every padded n >= 384 (tests),
 *                          -2 as 2 but the lazy form's head phase computes every candidate's exact mean instead of the
 *                          bound of it that 1 and 2 take for the RBF kernel (A/B measurements, tests; 3 is not a value).
 *                          The returned (value, index) pair has the same bits either way. */
enum {
  GPX_OPT_RESERVED_0 = 0,
  GPX_OPT_SPIN_LIMIT = 1,
  GPX_OPT_SWEEP_FUSED = 2,
  GPX_OPT_GRAM_SPLIT = 3,
  GPX_OPT_POTRF_LAZY = 4,
  GPX_OPT_POTRF_MODE = 5,
  GPX_OPT_POTRF_SWITCH = 6,
  GPX_OPT_POTRF_SPLIT = 7,
  GPX_OPT_SWEEP_PRUNE = 8,
  GPX_OPT_COUNT = 9
};
gpx_status gpx_set_option(gpx_handle h, int32_t option, int64_t value);
gpx_status gpx_get_option(gpx_handle h, int32_t option, int64_t* value_host);

/* ---- fit = posterior update ----------------------------------------------- */
/* Gram K(X,X)+(noise+jitter)I into the lower triangle of the padded K (replaces the covar_module(X) +
 * likelihood evaluation inside ExactMarginalLogLikelihood / ExactGP prediction strategy [upstream],
 * reached from optimization/Bayesian.py:91-93 and optimization/Bayesian6.py:476-484). */
gpx_status gpx_gram_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                        double* K, int64_t ldk);

/* In-place blocked lower Cholesky of the padded matrix (replaces psd_safe_cholesky [upstream];
 * jitter policy optimization/Bayesian6.py:483,487).  Dinv (2 * padded_n/64 * 64*64 doubles) receives the
 * inverses of the 64x64 diagonal blocks in its first half; the second half is scratch.  Only the lower
 * triangle of A is defined afterwards.  info: device int32, 0 or pivot+1. */
gpx_status gpx_potrf_f64(gpx_handle h, int64_t n, double* A, int64_t lda, double* Dinv, int32_t* info);

/* W = L^{-T} (upper triangular, row-major, i.e. W[k][i] = (L^{-1})[i][k]; strict lower part zeroed).
 * Needs the Dinv of gpx_potrf_f64.  Used by alpha and the candidate sweep. */
gpx_status gpx_trtri_workspace_size(int64_t n, size_t* bytes);
gpx_status gpx_trtri_f64(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv, double* W,
                         int64_t ldw, void* ws, size_t ws_bytes);

/* The same for `batch` factors at fixed element strides (the W of gpx_fit_factor_batched_f64's problems before their
 * sweeps), in the same launches. */
gpx_status gpx_trtri_batched_workspace_size(int64_t n, int64_t batch, size_t* bytes);
gpx_status gpx_trtri_batched_f64(gpx_handle h, int64_t batch, int64_t n, const double* L, int64_t ldl, int64_t stride_l,
                                 const double* Dinv, int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w,
                                 void* ws, size_t ws_bytes);

/* alpha = K^{-1} (Y - const_mean) = W W^T (Y - m) for nrhs <= GPX_MAX_RHS right-hand sides.  Y: n x nrhs
 * row-major with leading dim ldy; alpha: contiguous padded_n x nrhs (rows >= n are set to 0).
 * Replaces the ExactGP mean_cache [upstream]. */
gpx_status gpx_alpha_workspace_size(int64_t n, int64_t nrhs, size_t* bytes);
gpx_status gpx_alpha_f64(gpx_handle h, int64_t n, const double* W, int64_t ldw, const double* Y, int64_t ldy,
                         int64_t nrhs, double const_mean, double* alpha, void* ws, size_t ws_bytes);

/* One full posterior update: Gram + Cholesky + L^{-T} + alpha.  K (padded, in/out: holds L afterwards),
 * W, Dinv, alpha as above.  Asynchronous; *info (device) reports NOT_PD. */
gpx_status gpx_fit_workspace_size(int64_t n, int64_t nrhs, size_t* bytes);
gpx_status gpx_fit_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                       const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv,
                       double* W, int64_t ldw, double* alpha, int32_t* info, void* ws, size_t ws_bytes);
/* Same, then synchronises the stream and returns GPX_NOT_PD with *info_host = pivot+1 on failure. */
gpx_status gpx_fit_f64_sync(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                            const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv,
                            double* W, int64_t ldw, double* alpha, int32_t* info, void* ws, size_t ws_bytes,
                            int32_t* info_host);

/* alpha = K^{-1} (Y - const_mean) from the factor alone (LAPACK potrs): forward L z = Y - m, backward L^T alpha = z,
 * with L and Dinv as gpx_potrf_f64 left them (no W needed).  Y: n x nrhs (leading dim ldy), alpha: contiguous
 * padded_n x nrhs (rows >= n are 0).  info (device, nullable): the factor's pivot word — a failed factor (non-zero)
 * leaves alpha untouched; a solve whose in-launch hand-off times out writes GPX_INFO_TIMEOUT into it (and NaN into
 * alpha).  One launch; its workgroups hand 128-row blocks of z / alpha to each other inside it (deterministic: fixed
 * accumulation order).  Replaces the ExactGP mean_cache [upstream]. */
gpx_status gpx_potrs_workspace_size(int64_t n, int64_t nrhs, size_t* bytes);
gpx_status gpx_potrs_f64(gpx_handle h, int64_t n, const double* L, int64_t ldl, const double* Dinv, const double* Y,
                         int64_t ldy, int64_t nrhs, double const_mean, double* alpha, int32_t* info, void* ws,
                         size_t ws_bytes);

/* The posterior update as SURVEY §8d defines it — Gram + Cholesky + alpha — WITHOUT the explicit inverse: alpha by
 * gpx_potrs_f64.  K (padded, in/out: holds L afterwards), Dinv, alpha, info as in gpx_fit_f64.  Everything the fit
 * caches for prediction is then ready except W = L^{-T}, which gpx_trtri_f64(L, Dinv) builds when a sweep, a posterior,
 * an MLL gradient or an append needs it (the inverse costs as much as the factorisation; an update that is followed
 * by more updates before the next sweep never pays it). */
gpx_status gpx_fit_factor_workspace_size(int64_t n, int64_t nrhs, size_t* bytes);
gpx_status gpx_fit_factor_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                              const double* Y, int64_t ldy, int64_t nrhs, double* K, int64_t ldk, double* Dinv,
                              double* alpha, int32_t* info, void* ws, size_t ws_bytes);

/* Batched posterior updates: `batch` independent problems of the same n, d and kernel parameters (restarts /
 * seeds: BASELINE configs[3], the per-batch `info` of the SURVEY §8b proposal) in the SAME launches, the problem
 * index being one more grid dimension.  Every array of problem b starts at base + b * stride_* (element strides;
 * outputs K / Dinv / W / alpha >= one problem; the read-only X and Y any stride >= 0: X stride 0 = one X shared by
 * every problem, Y stride 1 with ldy = batch = column b of an n x batch target matrix); info: device int32[batch],
 * each 0 or that problem's failing pivot + 1.  Results are identical bit for
 * bit to `batch` calls of gpx_fit_f64 with the default options, although the batch may take a different Cholesky
 * schedule (every schedule computes each factor entry by the same MFMA chain, gpx_potrf.hip trailing_tile_at), so a
 * problem's result does not depend on how many problems share its GPU.  The Cholesky is a latency-bound chain of nblk dependent launches, so a batch of B
 * costs far less than B fits (replaces the per-restart fits of optimize_acqf / fit_gpytorch_mll restarts [upstream]). */
gpx_status gpx_fit_batched_workspace_size(int64_t n, int64_t nrhs, int64_t batch, size_t* bytes);
gpx_status gpx_fit_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n, const double* X,
                               int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy, int64_t stride_y,
                               int64_t nrhs, double* K, int64_t ldk, int64_t stride_k, double* Dinv,
                               int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w, double* alpha,
                               int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes);
/* The same without W (gpx_fit_factor_f64 per problem, bit-identical to it). */
gpx_status gpx_fit_factor_batched_workspace_size(int64_t n, int64_t nrhs, int64_t batch, size_t* bytes);
gpx_status gpx_fit_factor_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                      const double* X, int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy,
                                      int64_t stride_y, int64_t nrhs, double* K, int64_t ldk, int64_t stride_k,
                                      double* Dinv, int64_t stride_dinv, double* alpha, int64_t stride_alpha,
                                      int32_t* info, void* ws, size_t ws_bytes);

/* The same with ONE PARAMETER SET PER PROBLEM: p points to `batch` parameter structs of the same d (any kind, lengthscales,
 * outputscale, linear variances, noise, jitter and constant mean).  This is the reference's multi-output SingleTaskGP
 * (optimization/Bayesian1.py:108-116: SingleTaskGP(X, Y[n, 8], Standardize(m=8)), a batch of 8 independent GPs on one X,
 * each with its own lengthscales, outputscale, noise and ConstantMean [upstream]; optimization/Bayesian6.py:474-478
 * shares the covariance module, but its likelihood noise and mean are still per output): X stride 0, Y stride 1 with
 * ldy = batch and nrhs = 1.  The covariance of each problem is built with its own parameters (one Gram launch per
 * problem when they differ), the Cholesky and the solves run once over all problems; a problem's result is bit for bit
 * the single fit with its parameters.  Workspace sizes as for the shared-parameter entry points. */
gpx_status gpx_fit_batched_params_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                      const double* X, int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy,
                                      int64_t stride_y, int64_t nrhs, double* K, int64_t ldk, int64_t stride_k,
                                      double* Dinv, int64_t stride_dinv, double* W, int64_t ldw, int64_t stride_w,
                                      double* alpha, int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes);
gpx_status gpx_fit_factor_batched_params_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n,
                                             const double* X, int64_t ldx, int64_t stride_x, const double* Y,
                                             int64_t ldy, int64_t stride_y, int64_t nrhs, double* K, int64_t ldk,
                                             int64_t stride_k, double* Dinv, int64_t stride_dinv, double* alpha,
                                             int64_t stride_alpha, int32_t* info, void* ws, size_t ws_bytes);

/* Incremental posterior update: rows n_old .. n_new-1 of X / Y appended to a GP whose L, Dinv and W
 * hold a successful fit (gpx_fit_f64 or an earlier append) of the first n_old rows with the SAME kernel parameters.
 * The reference appends the new observations and refits from scratch every round (optimization/Bayesian7.py:628-631,
 * 692-700 then :639; optimization/Bayesian.py:163-174); with the hyperparameters unchanged the leading block of the
 * factor is unchanged, so this bordered update costs O(n^2 q) (q = n_new - n_old) instead of O(n^3) and produces the
 * factor, W and alpha a fresh gpx_fit_f64 of all n_new rows would (rows past the last full 128-tile of the old fit
 * are refactored).  L / W must have leading dims >= gpx_padded_n(n_new) (allocate with spare capacity), Dinv room
 * for 2 * gpx_padded_n(n_new)/64 blocks, alpha gpx_padded_n(n_new) x nrhs.  Y holds all n_new targets (alpha is
 * recomputed, so a re-standardised Y is fine).  info: device int32, 0 or global failing pivot + 1. */
gpx_status gpx_append_workspace_size(int64_t n_old, int64_t n_new, int64_t nrhs, size_t* bytes);
gpx_status gpx_append_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n_old, int64_t n_new, const double* X,
                          int64_t ldx, const double* Y, int64_t ldy, int64_t nrhs, double* L, int64_t ldl,
                          double* Dinv, double* W, int64_t ldw, double* alpha, int32_t* info, void* ws,
                          size_t ws_bytes);

/* ---- posterior / acquisition ---------------------------------------------- */
/* Posterior at m points Xs (m x d, ld ldxs): mean (m x nrhs, ld ldmean) and variance (m), untransformed
 * by (y_mean[r], y_scale[r]) per output r (host arrays of nrhs; NULL = identity).  Replaces
 * model.posterior(X).mean/.variance (optimization/Bayesian2.py:169-171, optimization/Bayesian6.py:615-617).
 * var_out is the variance of output 0's untransform (all outputs share the factor). */
gpx_status gpx_sweep_workspace_size(int64_t n, int64_t nrhs, int64_t m, size_t* bytes);
gpx_status gpx_posterior_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                             const double* W, int64_t ldw, const double* alpha, int64_t nrhs, const double* Xs,
                             int64_t m, int64_t ldxs, const double* y_mean_host, const double* y_scale_host,
                             double* mean_out, int64_t ldmean, double* var_out, void* ws, size_t ws_bytes);

/* Candidate sweep: score m candidates with an analytic acquisition on the posterior whose mean uses the
 * padded_n vector `alpha` (one output column of gpx_alpha_f64, or a weighted combination of columns for a
 * linear objective) and reduce to (best value, lowest index among ties); reported indices are
 * index_offset + local index (candidate shards on several GPUs).  best_val/best_idx are device scalars; scores_out
 * (device, m) is optional (NULL = not written).  Replaces the raw-sample sweep + argmax of optimize_acqf
 * (optimization/Bayesian.py:105-113) and the pool scan + topk of optimization/Bayesian7.py:646-681.
 * The returned pair is exact: without scores_out the sweep may stop a candidate's variance product early once an upper
 * bound of its score (every acquisition here grows with the variance, and the variance only shrinks as the product
 * proceeds) lies below a score already computed in full; such a candidate cannot be the argmax, and the pair has the
 * bits of the full sweep (GPX_OPT_SWEEP_PRUNE = 0).  scores_out != NULL forces the full sweep: every score is wanted.
 * Asynchronous, except that a call of the lazy pruned sweep with more candidates than one of its chunks holds waits
 * once per such span for the survivor count (gpx_debug_set_sweep_tail_sync; never on a stream in capture). */
gpx_status gpx_acquire_argmax_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X,
                                  int64_t ldx, const double* W, int64_t ldw, const double* alpha,
                                  const double* Xs, int64_t m, int64_t ldxs, const gpx_acq_params* a,
                                  int64_t index_offset, double* best_val, int64_t* best_idx,
                                  double* scores_out, void* ws, size_t ws_bytes);
/* Work counters of the handle's last sweep, a gpx_acquire_argmax_f64, gpx_acquire_topk_f64 or
 * gpx_acquire_topk_multi_f64 call (the last one's meanings: at its declaration below) (synchronises the
 * handle's stream; the workspace of that call must still be allocated): out_host[0] candidates seen, [1] candidates
 * whose last 128-row tile of the variance product was computed, [2] 128 x 128 product tiles executed, [3] the tiles the
 * full sweep executes (0 / 0 on the fused small-n path, which has no tiles). */
gpx_status gpx_sweep_stats(gpx_handle h, int64_t* out_host);

/* The k best candidates of the sweep above without the full sweep: val_out / idx_out (device, k each) hold exactly what
 * gpx_acquire_argmax_f64 with scores_out = S followed by gpx_topk_f64(S, m, k) gives: the k largest scores in
 * descending order, equal scores with the lower index first, a NaN score ranked (and returned) as -inf, -0 as +0;
 * the values have the bits of the full sweep's scores and the indices are index_offset + local index.
 * Where the pruned sweep applies (GPX_OPT_SWEEP_PRUNE, the K* + trmm path) the incumbent of its bound test is the k-th
 * best score computed in full so far: a dropped candidate lies strictly below k exactly scored ones, so it can neither
 * be among the k best nor tie with the k-th.  Elsewhere (GPX_OPT_SWEEP_PRUNE = 0, the fused small-n sweep, padded
 * n < 384) the call runs the full sweep into a score array of its own workspace and gpx_topk_f64's sort.
 * Arguments and validation as gpx_acquire_argmax_f64, plus 1 <= k <= min(m, GPX_TOPK_SWEEP_MAX): the pruned sweep
 * scores its leading GPX_TOPK_SWEEP_MAX candidates in full before its first bound pass, which fills the pool of the k
 * best for every legal k.  Asynchronous on the handle's stream but for the wait gpx_acquire_argmax_f64 names, no
 * allocation, the same bits on every call.  gpx_acquire_topk_workspace_size: gpx_sweep_workspace_size(n, 1, m) plus
 * the top-k part (a 256-byte header, the pool of k 16-byte pairs, one 16-byte scored-list entry per candidate of a sweep chunk, the composed
 * path's m scores and gpx_topk_workspace_size(m), each rounded up to 256 bytes). */
enum { GPX_TOPK_SWEEP_MAX = 1024 };
gpx_status gpx_acquire_topk_workspace_size(int64_t n, int64_t m, int64_t k, size_t* bytes);
gpx_status gpx_acquire_topk_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                                int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, int64_t k,
                                double* val_out /* k, device */, int64_t* idx_out /* k, device */,
                                void* ws, size_t ws_bytes);

/* Candidate sweep of a LINEAR OBJECTIVE over T independent GPs on the same training inputs X (the outputs of the batched
 * fits above, or of separate fits / appends of the same n): f = sum_t w_t (y_mean[t] + y_scale[t] g_t) with g_t the
 * posterior of output t: its own p[t], W_host[t] (device pointer to its W = L^{-T}, leading dim ldw_host[t]) and
 * alpha_host[t] (device pointer to its padded_n alpha column); W_host / ldw_host / alpha_host are host arrays of T.  So mean = sum_t w_t (y_mean[t] +
 * y_scale[t] mu_t) and, the outputs being independent, variance = sum_t w_t^2 y_scale[t]^2 var_t (each var_t floored at
 * 1e-10 in its standardised space, the sum at 1e-12: GPyTorch's / BoTorch's floors [upstream]).  Scored with a's kind /
 * best_f / beta (a->y_mean, a->y_scale are not used: the per-output y_mean_host / y_scale_host are, NULL = 0 / 1) and
 * reduced like gpx_acquire_argmax_f64.  VARIANCE with w_t = 1 is the variance-sum pool-scan score of
 * optimization/Bayesian7.py:671 over independent outputs; EI / LogEI / UCB with weights the scalarised objective of a
 * multi-output model (optimization/Bayesian1.py:119-140's mean-of-8 objective, analytic form).  T = 1, w = 1 gives
 * gpx_acquire_argmax_f64's scores bit for bit. */
gpx_status gpx_sweep_multi_workspace_size(int64_t n, int64_t m, size_t* bytes);
gpx_status gpx_acquire_argmax_multi_f64(gpx_handle h, const gpx_kernel_params* p, int64_t T, int64_t n, const double* X,
                                        int64_t ldx, const double* const* W_host, const int64_t* ldw_host,
                                        const double* const* alpha_host, const double* weights_host,
                                        const double* y_mean_host, const double* y_scale_host, const double* Xs,
                                        int64_t m, int64_t ldxs, const gpx_acq_params* a, int64_t index_offset,
                                        double* best_val, int64_t* best_idx, double* scores_out, void* ws,
                                        size_t ws_bytes);

/* The k best candidates of the multi-output sweep above without the full sweep: val_out / idx_out (device, k each) hold
 * exactly what gpx_acquire_argmax_multi_f64 with scores_out = S followed by gpx_topk_f64(S, m, k) and the index shift
 * gives (descending, equal scores with the lower index first, NaN as -inf, -0 as +0, the bits of the full sweep's
 * scores); k = 1 is gpx_acquire_argmax_multi_f64's pair after that keying, and T = 1 with w = 1 gives
 * gpx_acquire_topk_f64's bits.  Arguments and validation as gpx_acquire_argmax_multi_f64, plus
 * 1 <= k <= min(m, GPX_TOPK_SWEEP_MAX).
 * The pruned form runs where GPX_OPT_SWEEP_PRUNE admits it (unfused path, padded n at or above its threshold) and every
 * output has the fp64 covariance build and d <= 16.  The objective's variance sum_t w_t^2 y_scale[t]^2 var_t has
 * non-negative terms and each var_t can only shrink as row tiles of its product are added, so the variance summed from
 * the first 128-row tile of every output is an upper bound of the exact one (in floating point too: rounded sums, fmax
 * and products with a non-negative constant are monotone); the mean is computed exactly, and every acquisition is
 * non-decreasing in the variance.  A candidate whose bound lies below the k-th best score computed in full so far is
 * dropped; the others get the full product of every output.  Elsewhere (GPX_OPT_SWEEP_PRUNE = 0, padded n < 384, the
 * fused small-n sweep, cov_fp32, d > 16) the call runs the full multi-output sweep into a score array of its own
 * workspace and gpx_topk_f64's sort.  Asynchronous on the handle's stream, no allocation, no host synchronisation, the
 * same bits on every call.
 * gpx_sweep_stats after this call: [0] candidates seen, [1] candidates whose product was computed to the last row tile
 * for every output, [2] 128 x 128 product tiles executed, summed over the outputs, [3] the tiles of the full
 * multi-output sweep (T times the single sweep's; the fused path has none).
 * gpx_acquire_topk_multi_workspace_size: gpx_sweep_multi_workspace_size(n, m) plus the top-k part of
 * gpx_acquire_topk_workspace_size. */
gpx_status gpx_acquire_topk_multi_workspace_size(int64_t n, int64_t m, int64_t k, size_t* bytes);
gpx_status gpx_acquire_topk_multi_f64(gpx_handle h, const gpx_kernel_params* p, int64_t T, int64_t n, const double* X,
                                      int64_t ldx, const double* const* W_host, const int64_t* ldw_host,
                                      const double* const* alpha_host, const double* weights_host,
                                      const double* y_mean_host, const double* y_scale_host, const double* Xs,
                                      int64_t m, int64_t ldxs, const gpx_acq_params* a, int64_t index_offset, int64_t k,
                                      double* val_out /* k, device */, int64_t* idx_out /* k, device */, void* ws,
                                      size_t ws_bytes);

/* Deterministic (value, index) reduction of `count` device records: max value, then lowest index; NaN
 * never wins.  Used after the cross-GPU all-gather of per-rank records. */
gpx_status gpx_argmax_combine_f64(gpx_handle h, const double* vals, const int64_t* idx, int64_t count,
                                  double* best_val, int64_t* best_idx);

/* ---- gradients for acquisition optimisation ---------------------------------------------- */
/* Posterior moments of m candidates Xs (m x d) grouped in consecutive q-batches (m/q batches of q points: restarts of
 * optimize_acqf x its q, optimization/Bayesian.py:105-112, optimization/Bayesian2.py:240-245) and their derivatives
 * w.r.t. the candidates, for the L-BFGS-B refinement that BoTorch drives with torch autograd [upstream].  In the
 * engine's (standardised) units, with alpha one padded_n column and c ranging over a's batch:
 *   mean[a]   = const_mean + k_a^T alpha                 dmean[a*d + j]       = d mean[a] / d x_aj
 *   cov[a*q + c'] = k(x_a, x_c) - k_a^T K^{-1} k_c     dcov[(a*d + j)*q + c'] = d1 k(x_a, x_c)/dx_aj - d k_a/dx_aj^T K^{-1} k_c
 * (c = batch start + c'; d1 = derivative in the first argument only, so that the gradient of a function L of the batch
 * covariance is dL/dx_aj = sum_c' (G[a][c] + G[c][a]) dcov[(a*d+j)*q + c'] with G = dL/dcov).  K^{-1} k_c = W (W^T k_c)
 * on fp64 MFMA; the q-batch posterior covariance is noise-free (add noise for observation noise).  All outputs are
 * device arrays; deterministic. */
gpx_status gpx_moments_grad_workspace_size(int64_t n, int64_t m, size_t* bytes);
gpx_status gpx_moments_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t m,
                                int64_t q, int64_t ldxs, double* mean, double* dmean, double* cov, double* dcov,
                                void* ws, size_t ws_bytes);

/* Monte-Carlo acquisition value of B q-batches from their joint moments (mean B x q, cov B x q x q, as
 * gpx_moments_grad_f64 gives them after the caller's scaling) and S x q base samples z, with the gradients w.r.t. the
 * moments: the q x q part of optimize_acqf that follows the moments call.  QLOGEI is qLogExpectedImprovement with
 * q = batch_size (optimization/Bayesian.py:100-112, optimization/Bayesian2.py:226-245); QPSD is
 * qPosteriorStandardDeviation of one output (optimization/Bayesian6.py:113-130, 896-919).  Per q-batch b:
 *   A = (cov + cov^T) / 2 = L L^T; a pivot <= 0 or NaN retries that batch with A + j I, j = 1e-8, 1e-7, 1e-6
 *   (GPyTorch psd_safe_cholesky for fp64 [upstream, unverified]); info[b] = 0 clean, k = 1..3 factored at retry k,
 *   -1 not factored: value[b] and the gradients of b are NaN then, the other batches are unaffected.
 *   f_s = mean + L z_s, y = (f - best_f) / tau_relu
 *   QLOGEI  li = log tau_relu + log(softplus(y) + 0.1 / (1 + y^2))   (fat_relu = 1; 0: log tau_relu + log softplus(y),
 *           = y below y <= -37)
 *           r_s = tau_max logsumexp_i(li / tau_max)                  (fat_max = 0), or with M = max_i li, alpha = 2,
 *           t_i = 1 + (M - li_i) / (alpha tau_max): r_s = M + tau_max log sum_i t_i^-alpha  (fat_max = 1: BoTorch
 *           safe_math.fatmax [upstream, unverified])
 *           value = logsumexp_s r_s - log S
 *   QPSD    value = sum_i std_s(f_si), the unbiased standard deviation over the samples (S >= 2), in the closed form
 *           sqrt(l_i C l_i^T) with l_i row i of L and C the unbiased sample covariance of the rows of z; gmean = 0.
 * gmean = d value / d mean and gcov = d value / d cov, the latter through the symmetrised factorisation (symmetric:
 * what torch gives for cholesky((cov + cov^T) / 2)).  gmean and gcov are both NULL (value only: raw-sample scoring) or
 * both set; the value has the same bits either way.  Limits: 1 <= q <= GPX_MAX_Q, B q <= GPX_MAX_GRAD_CANDIDATES,
 * 1 <= S <= 2^20 (QPSD: S >= 2).  reserved != 0, a flag outside {0, 1}, a tau that is not positive or an unknown kind
 * is GPX_INVALID_ARG, and nothing is launched.  Device pointers, contiguous fp64; asynchronous on the handle's stream,
 * no allocation; every sum runs in a fixed order, so two calls give the same bits. */
enum { GPX_MCACQ_QLOGEI = 0, GPX_MCACQ_QPSD = 1 };
typedef struct {
  int32_t kind;     /* GPX_MCACQ_* */
  int32_t fat_relu; /* QLOGEI: 1 log_fatplus, 0 log_softplus */
  int32_t fat_max;  /* QLOGEI: 1 fatmax (alpha = 2), 0 tau_max * logsumexp */
  int32_t reserved; /* must be 0 */
  double best_f, tau_relu, tau_max;
} gpx_mcacq_params;
/* sizeof(gpx_mcacq_params) (40) as compiled into the library, for a binding's load-time check */
size_t gpx_mcacq_params_size(void);
gpx_status gpx_mc_acq_workspace_size(int64_t B, int64_t q, int64_t S, size_t* bytes);
gpx_status gpx_mc_acq_f64(gpx_handle h, const gpx_mcacq_params* a, int64_t B, int64_t q, int64_t S,
                          const double* mean /* B x q */, const double* cov /* B x q x q */,
                          const double* z /* S x q base samples */, double* value /* B */,
                          double* gmean /* B x q or NULL */, double* gcov /* B x q x q or NULL */,
                          int32_t* info /* B */, void* ws, size_t ws_bytes);

/* ---- noisy expected improvement (qNoisyExpectedImprovement, optimization/Bayesian1.py:118-140) -------------------- */
/* Joint noise-free posterior at mb points Xb (mb x d): mean_b[c] = const_mean + k_c^T alpha and the full covariance
 * cov_bb[c * mb + e] = k(xb_c, xb_e) - k_c^T K^{-1} k_e (K* on the device, V = W^T K*, K_bb - V^T V on fp64 MFMA).  Sb,
 * when not NULL, receives K^{-1} K(X, Xb) = W V as padded_n rows of length ldsb >= mb rounded up to 64: the operand of
 * gpx_cross_cov_grad_f64.  The set-up call of qNEI (once per baseline) and of the pruning of the baseline.
 * Limits: 1 <= mb <= GPX_MAX_JOINT.  Device arrays; deterministic. */
gpx_status gpx_joint_moments_workspace_size(int64_t n, int64_t mb, size_t* bytes);
gpx_status gpx_joint_moments_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                 const double* W, int64_t ldw, const double* alpha, const double* Xb, int64_t mb,
                                 int64_t ldxb, double* mean_b /* mb */, double* cov_bb /* mb x mb */,
                                 double* Sb /* padded_n x ldsb or NULL */, int64_t ldsb, void* ws, size_t ws_bytes);

/* Posterior cross-covariance of m candidates Xs to nb fixed baseline points Xb and its derivative w.r.t. the candidates
 * (the baseline does not move, so the derivative is complete), with Sb from gpx_joint_moments_f64 on the same Xb:
 *   cross[a * nb + b]            = k(x_a, xb_b) - sum_i k(x_a, X_i) Sb[i][b]
 *   dcross[(a * d + j) * nb + b] = d1 k(x_a, xb_b)/dx_aj - sum_i d1 k(x_a, X_i)/dx_aj Sb[i][b]
 * dcross may be NULL (value-only scoring: another kernel, four candidates per workgroup, so cross then agrees with
 * the gradient call's to rounding, not to the bit).  Both run on the vector units.
 * Limits: 1 <= nb <= GPX_MAX_BASELINE, 1 <= m <= GPX_MAX_GRAD_CANDIDATES.  The workspace is unused (0 bytes asked). */
gpx_status gpx_cross_cov_grad_workspace_size(int64_t n, int64_t nb, int64_t m, size_t* bytes);
gpx_status gpx_cross_cov_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* Sb, int64_t ldsb, const double* Xb, int64_t nb, int64_t ldxb,
                                  const double* Xs, int64_t m, int64_t ldxs, double* cross /* m x nb */,
                                  double* dcross /* m x d x nb or NULL */, void* ws, size_t ws_bytes);

/* Monte-Carlo noisy expected improvement of B q-batches, baseline first, then the q-batch (BoTorch's cached-root form
 * [upstream, unverified]).  The caller forms once per baseline: L_b = chol of the baseline's joint covariance,
 * Linv = L_b^{-1} (nb x nb, row-major), base samples zb (S x nb) and zq (S x q), and the per-sample incumbent
 * best[s] = max_j (mu_b + L_b zb_s)_j.  Per q-batch, with mean (q), cov (q x q) and cross (q x nb) of the objective:
 *   A = cross Linv^T, D = (cov + cov^T) / 2 - A A^T = L L^T with the jitter ladder and info[] of gpx_mc_acq_f64
 *   f_si = mean_i + sum_j A_ij zb_sj + sum_{j <= i} L_ij zq_sj
 *   log = 0 (qNEI)     value = (1/S) sum_s max(0, max_i f_si - best_s); the gradient of the max goes to the lowest
 *                      maximal index; a batch in which no sample improves has value 0 and gradients exactly 0
 *   log = 1 (qLogNEI)  li_si = log tau_relu + log_improvement((f_si - best_s) / tau_relu), r_s and value as QLOGEI of
 *                      gpx_mc_acq_f64 (fat_relu, fat_max, tau_relu, tau_max with the same meaning)
 * gmean = d value / d mean, gcov = d value / d cov (symmetric), gcross = d value / d cross = (Abar - 2 gcov A) Linv with
 * Abar_ij = sum_s fbar_si zb_sj.  gmean, gcov and gcross are all NULL (value only) or all set; the value has the same
 * bits either way.  Limits: those of gpx_mc_acq_f64 and 1 <= nb <= GPX_MAX_BASELINE.  Bad arguments are
 * GPX_INVALID_ARG, and nothing is launched.  Every sum runs in a fixed order: two calls give the same bits. */
typedef struct {
  int32_t log;      /* 0 qNEI, 1 qLogNEI */
  int32_t fat_relu; /* log = 1: 1 log_fatplus, 0 log_softplus */
  int32_t fat_max;  /* log = 1: 1 fatmax (alpha = 2), 0 tau_max * logsumexp */
  int32_t reserved; /* must be 0 */
  double tau_relu, tau_max;
} gpx_mcnei_params;
/* sizeof(gpx_mcnei_params) (32) as compiled into the library, for a binding's load-time check */
size_t gpx_mcnei_params_size(void);
gpx_status gpx_mc_nei_workspace_size(int64_t B, int64_t q, int64_t nb, int64_t S, size_t* bytes);
gpx_status gpx_mc_nei_f64(gpx_handle h, const gpx_mcnei_params* a, int64_t B, int64_t q, int64_t nb, int64_t S,
                          const double* mean /* B x q */, const double* cov /* B x q x q */,
                          const double* cross /* B x q x nb */, const double* Linv /* nb x nb */,
                          const double* zb /* S x nb */, const double* best /* S */, const double* zq /* S x q */,
                          double* value /* B */, double* gmean /* B x q or NULL */,
                          double* gcov /* B x q x q or NULL */, double* gcross /* B x q x nb or NULL */,
                          int32_t* info /* B */, void* ws, size_t ws_bytes);

/* ---- cross-GPU selection exchange (SURVEY §8b gpx_allreduce_argmax, §8e) ------------------------------------------ */
/* One process per GPU.  Rank 0 creates the communicator id (gpx_comm_unique_id), the host side broadcasts its
 * GPX_COMM_ID_BYTES bytes (e.g. over torch.distributed), every rank calls gpx_comm_init (collective).
 * gpx_allreduce_argmax replaces every rank's device (best_val, best_idx) record by the global best: the record is
 * packed into one 16-byte {fp64 value, int64 index} on the device, ONE RCCL all-gather of those 16 bytes per rank runs
 * over xGMI, then the argmax_combine kernel (max value, lowest global index, NaN never wins) on the handle's stream —
 * RCCL has no MAXLOC.  Three stream operations per exchange; no host synchronisation.  Replaces the final best-candidate selection across the
 * independent restarts/shards (BASELINE configs[3]). */
gpx_status gpx_comm_unique_id(uint8_t* id_out);
gpx_status gpx_comm_init(gpx_handle h, const uint8_t* id, int32_t nranks, int32_t rank, gpx_comm* out);
gpx_status gpx_comm_destroy(gpx_comm c);
gpx_status gpx_allreduce_argmax_workspace_size(gpx_comm c, size_t* bytes);
gpx_status gpx_allreduce_argmax(gpx_handle h, gpx_comm c, double* best_val, int64_t* best_idx, void* ws,
                                size_t ws_bytes);

/* ---- marginal likelihood -------------------------------------------------------- */
/* Negative log marginal likelihood of a fitted exact GP with T = nrhs outputs sharing the covariance (T = 1:
 * the SingleTaskGP objective) and its gradient w.r.t. the shared hyperparameters:
 *   -log p(Y) = sum_t [ (y_t - m)^T alpha_t / 2 ] + T (sum log L_ii + n/2 log 2 pi)
 *   d/d theta = 1/2 sum_ij (T K^{-1} - sum_t alpha_t alpha_t^T)_ij dK_ij/d theta,   d/dm = -sum_t sum_i alpha_ti,
 * with K^{-1} = W W^T formed tile by tile on the MFMA units and contracted against dK/d theta recomputed
 * from X inside the same kernel (K^{-1} is never stored).  Inputs are the outputs of gpx_fit_f64: L (the
 * factored K), W, alpha (contiguous padded_n x nrhs), and the targets Y (n x nrhs, leading dim ldy) the fit
 * used.  out: device array of GPX_MLL_NOUT doubles (layout above; QUAD and LOGDET are the totals over the
 * outputs and one log|K|; the covariance is differentiated in fp64 regardless of cov_fp32).  Deterministic
 * (fixed reduction order).  Replaces ExactMarginalLogLikelihood(...).backward() inside fit_gpytorch_mll
 * [upstream] (optimization/Bayesian.py:92-93, optimization/Bayesian1.py:114-115, optimization/Bayesian6.py:480-488). */
gpx_status gpx_mll_workspace_size(int64_t n, size_t* bytes);
/* (the batched form is below) */
gpx_status gpx_mll_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                            const double* Y, int64_t ldy, int64_t nrhs, const double* L, int64_t ldl,
                            const double* W, int64_t ldw, const double* alpha, double* out, void* ws,
                            size_t ws_bytes);

/* The same for `batch` independent problems with one parameter set each (the fits of gpx_fit_batched_params_f64):
 * problem b's X, Y, L, W, alpha at base + b * stride_* (X / Y strides >= 0, as in the batched fit), its output vector at
 * out + b * GPX_MLL_NOUT.  The reference's multi-output fit_gpytorch_mll minimises the SUM of the per-output losses
 * (optimization/Bayesian1.py:114-115 [upstream]); the host side (mll.py) sums them.  Workspace: gpx_mll_workspace_size. */
gpx_status gpx_mll_grad_batched_f64(gpx_handle h, const gpx_kernel_params* p, int64_t batch, int64_t n, const double* X,
                                    int64_t ldx, int64_t stride_x, const double* Y, int64_t ldy, int64_t stride_y,
                                    int64_t nrhs, const double* L, int64_t ldl, int64_t stride_l, const double* W,
                                    int64_t ldw, int64_t stride_w, const double* alpha, int64_t stride_alpha,
                                    double* out, void* ws, size_t ws_bytes);

/* ---- SVGP predictive + pool-scan selection: the driven variant ---------------- */
/* optimization/Bayesian7.py's BatchSVGP (ntask outputs, each with its own ScaleKernel(Linear + Matérn-5/2)
 * hyperparameters p[t], ConstantMean p[t].const_mean and GaussianLikelihood noise p[t].noise) served from its trained
 * variational state: inducing points Z (ntask x M x d), variational mean m (ntask x M) and chol_variational_covar
 * (ntask x M x M, only its lower triangle is used, like CholeskyVariationalDistribution [upstream]).
 *
 * gpx_svgp_prepare_f64 (once per trained model) factors K_ZZ + jitter I per task (gpytorch's VariationalStrategy
 * jitter: 1e-4 for the reference's float32 model [upstream]) and stores per task, in padded Mpad x Mpad blocks
 * (Mpad = gpx_padded_n(M)): W = L_ZZ^{-T}, W2 = W S, and alpha' = W m (Mpad entries).  info: int32[ntask].
 * gpx_svgp_predict_f64 evaluates the whitened predictive of every task at m points Xs (already input-transformed,
 * Bayesian7.py:181-190): mean = const + k*^T alpha', var = max(k** - |W^T k*|^2 + |W2^T k*|^2 + noise, min_var)
 * (= likelihood(model(x)).variance, Bayesian7.py:558,668) into mean_out / var_out (m x ntask, NULL = skip) and
 * score_out[m] = sum over tasks of var (the pool-scan uncertainty score, Bayesian7.py:671; NULL = skip). */
gpx_status gpx_svgp_prepare_workspace_size(int64_t M, int64_t ntask, size_t* bytes);
gpx_status gpx_svgp_prepare_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                const double* Z, int64_t ldz, int64_t stride_z, const double* vmean,
                                int64_t stride_m, const double* vchol, int64_t ldc, int64_t stride_c, double* W,
                                double* W2, double* alpha, int32_t* info, void* ws, size_t ws_bytes);
gpx_status gpx_svgp_predict_workspace_size(int64_t M, int64_t m, size_t* bytes);
gpx_status gpx_svgp_predict_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                const double* Xs, int64_t m, int64_t ldxs, double min_var, double* mean_out,
                                int64_t ldmean, double* var_out, int64_t ldvar, double* score_out, void* ws,
                                size_t ws_bytes);

/* Analytic acquisition sweep on a prepared SVGP: gpx_acquire_argmax_multi_f64 / gpx_acquire_topk_multi_f64 for the
 * sparse model, a LINEAR OBJECTIVE f = sum_t w_t (y_mean[t] + y_scale[t] g_t) over its ntask independent tasks.  Z,
 * ldz, stride_z, W, W2, alpha: as gpx_svgp_predict_f64 (the blocks of gpx_svgp_prepare_f64).  Per task t and candidate
 * x, with k* = K(Z_t, x):
 *   mu_t = const_mean_t + k*^T alpha'_t,   var_t = max((k_t(x, x) - |W_t^T k*|^2) + |W2_t^T k*|^2, 1e-10)
 * var_t is the LATENT variance (no likelihood noise: an analytic acquisition is about f, as gpx_svgp_moments_grad_f64
 * has it; p[t].noise is not read), in gpx_svgp_predict_f64's operation order; S S^T <= I is not assumed.  Then
 *   mean = sum_t w_t (y_mean[t] + y_scale[t] mu_t),   variance = max(sum_t w_t^2 y_scale[t]^2 var_t, 1e-12)
 * (tasks summed in ascending order, the first one starting the sum: gpx_acquire_argmax_multi_f64's arithmetic and
 * floors) and score = a's kind / best_f / beta of (mean, variance); a->y_mean and a->y_scale are not used.
 * weights_host: ntask finite host doubles; y_mean_host / y_scale_host: ntask host doubles or NULL = 0 / 1.
 * scores_out (device, m; NULL = skip) gets the raw scores, a NaN staying a NaN.  val_out / idx_out (device, k each) are
 * what gpx_topk_f64 of those scores gives: descending, equal scores with the lower index first, NaN keyed as -inf and
 * -0 as +0, the indices shifted by index_offset; k = 1 is the argmax pair.  A candidate's score does not depend on m,
 * on its row, on index_offset or on k.  Two bit identities follow from sharing the predictive's launches: VARIANCE with
 * w_t = 1 and no untransform equals gpx_svgp_predict_f64's score_out of the same model with every noise = 0 and
 * min_var = 1e-10; ntask = 1, w = 1, UCB with beta = 0 equals its mean_out.
 * Validation as gpx_svgp_predict_f64 (the model, ldz, stride_z, ldxs) and gpx_acquire_argmax_multi_f64 (a, beta >= 0,
 * index_offset >= 0, finite weights, y_scale > 0), plus 1 <= k <= m <= 2^30; a workspace smaller than
 * gpx_svgp_acquire_workspace_size(M, m, k) is GPX_INVALID_ARG.  Every candidate gets both products in full: the sweep
 * is not pruned (the second product raises the variance, so the exact sweep's bound does not hold), and
 * gpx_sweep_stats is NOT defined after this call.  Asynchronous on the handle's stream, deterministic, no allocation,
 * no host synchronisation.
 * Workspace: gpx_sweep_workspace_size(M, 1, m) (the K* chunk, the mean partials, the first product's variance
 * partials, block records), then, each rounded up to 256 bytes: the second product's partials, the chunk's two
 * objective accumulators, m scores (used when scores_out is NULL) and gpx_topk_workspace_size(m).  It is never smaller
 * than gpx_svgp_predict_workspace_size(M, m). */
gpx_status gpx_svgp_acquire_workspace_size(int64_t M, int64_t m, int64_t k, size_t* bytes);
gpx_status gpx_svgp_acquire_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                const double* weights_host, const double* y_mean_host, const double* y_scale_host,
                                const double* Xs, int64_t m, int64_t ldxs, const gpx_acq_params* a,
                                int64_t index_offset, int64_t k, double* val_out /* k, device */,
                                int64_t* idx_out /* k, device */, double* scores_out /* m, device, or NULL */,
                                void* ws, size_t ws_bytes);

/* Posterior moments of m candidates Xs (m x d, consecutive q-batches) under ONE task of a prepared SVGP, and their
 * derivatives w.r.t. the candidates: gpx_moments_grad_f64 for the sparse model (optimize_acqf on the per-output SVGPs of
 * optimization/Bayesian6.py:492-577, 896-919).  p: the task's parameters; Z (M x d): its inducing points; W, W2
 * (Mpad x Mpad each) and alpha (Mpad): the task's blocks of gpx_svgp_prepare_f64.  With k_a = K(Z, x_a) and c ranging over
 * a's batch:
 *   v_c = W^T k_c,  u_c = W2^T k_c,  h_c = W v_c - W2 u_c          (= L^{-T} (I - S S^T) L^{-1} k_c)
 *   mean[a]       = const_mean + k_a^T alpha                  dmean[a*d + j]         = sum_i d1 k(x_a, z_i)/dx_aj alpha_i
 *   cov[a*q + c'] = k(x_a, x_c) - k_a^T h_c                   dcov[(a*d + j)*q + c'] = d1 k(x_a, x_c)/dx_aj - sum_i d1 k(x_a, z_i)/dx_aj h_c[i]
 * Shapes, the first-argument derivative d1 and the chain rule are gpx_moments_grad_f64's (W (I - S S^T) W^T is
 * symmetric).  K* is projected first and contracted afterwards; S S^T <= I is not assumed.  The covariance is the latent
 * one: no likelihood noise and no variance floor (gpx_svgp_predict_f64 adds the noise and clamps).  dmean and dcov may
 * both be NULL: values only, with the same bits of mean and cov.  Limits: 1 <= q <= GPX_MAX_Q, m % q == 0,
 * m <= GPX_MAX_GRAD_CANDIDATES.  Asynchronous on the handle's stream, deterministic, no allocation.
 * Workspace (doubles from the 256-byte aligned start; mpad = m rounded up to 64, blk = Mpad * mpad):
 *   [0, blk) K(Z, Xs), then H (K* is dead once V and U exist);  [blk, 2 blk) V = W^T K*;  [2 blk, 3 blk) U = W2^T K*;
 *   from 3 blk on the fp64-MFMA products' split-K partials. */
gpx_status gpx_svgp_moments_grad_workspace_size(int64_t M, int64_t m, size_t* bytes);
gpx_status gpx_svgp_moments_grad_f64(gpx_handle h, const gpx_kernel_params* p /* one task */, int64_t M,
                                     const double* Z, int64_t ldz, const double* W, const double* W2,
                                     const double* alpha, const double* Xs, int64_t m, int64_t q, int64_t ldxs,
                                     double* mean, double* dmean /* or NULL */, double* cov,
                                     double* dcov /* or NULL, with dmean */, void* ws, size_t ws_bytes);

/* ---- SVGP variational posterior in closed form (the collapsed bound of Titsias 2009) ------------------------------ */
/* For given hyperparameters p[t] and inducing points Z, the optimum of the whitened variational distribution
 * q(u) = N(m, S) of Bayesian7.py's model (Gaussian likelihood) under the full-batch ELBO, per task t, all fp64:
 *   K_ZZ + jitter I = L L^T, W = L^{-T};  Phi = W^T K(Z, X) (M x n);  r = y_t - const_mean;  s2 = noise
 *   B = I + Phi Phi^T / s2,  b = Phi r / s2;  S = B^{-1},  m = S b
 * vmean = m (ntask x M), vchol = the lower-triangular C with positive diagonal and C C^T = S (ntask x M x M, strict
 * upper triangle written as 0): the layout gpx_svgp_prepare_f64 reads.  X (n x d, already input-transformed) is streamed
 * in chunks of columns: Phi's chunk is formed first (projected), then Phi Phi^T and Phi r are accumulated from it, chunk
 * after chunk in a fixed order, so equal inputs and an equal chunk width give equal bits.
 * bound (ntask x GPX_SVGP_BOUND_NOUT): the collapsed bound F and its five terms (indices below).
 * info: int32[ntask], K_ZZ's failing pivot + 1 (as gpx_svgp_prepare_f64); a failed task's outputs are unspecified, the
 * other tasks are computed.
 * Workspace: gpx_svgp_fit_collapsed_workspace_size(M, n, ntask, chunk) for a chunk width `chunk` (rounded up to a
 * multiple of 128; 0 = the default, GPX_SVGP_FIT_CHUNK); it does not grow with n.  The call derives its chunk width from
 * ws_bytes: the largest multiple of 128, at most the default, that fits; below the chunk = 128 size: GPX_INVALID_ARG. */
enum {
  GPX_SVGP_BOUND_F = 0,       /* the sum of the five terms */
  GPX_SVGP_BOUND_CONST = 1,   /* -(n/2) log(2 pi s2) */
  GPX_SVGP_BOUND_LOGDET = 2,  /* -(1/2) log |B| */
  GPX_SVGP_BOUND_QUAD = 3,    /* -(1/2) r^T r / s2 */
  GPX_SVGP_BOUND_FIT = 4,     /* +(1/2) b^T B^{-1} b */
  GPX_SVGP_BOUND_TRACE = 5,   /* -(1/2) (sum_i k(x_i, x_i) - tr Phi Phi^T) / s2 */
  GPX_SVGP_BOUND_NOUT = 6
};
#define GPX_SVGP_FIT_CHUNK 4096
gpx_status gpx_svgp_fit_collapsed_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes);
gpx_status gpx_svgp_fit_collapsed_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                      const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                      int64_t ldx, const double* Y, int64_t ldy, double* vmean, int64_t stride_m,
                                      double* vchol, int64_t ldc, int64_t stride_c, double* bound, int32_t* info,
                                      void* ws, size_t ws_bytes);

/* ---- Hyperparameter gradient of the collapsed bound ------------------------------------------------------------- */
/* F(theta) of gpx_svgp_fit_collapsed_f64 (q(u) already at its optimum) and the gradient of -F with respect to the
 * natural hyperparameters of every task: likelihood noise, outputscale, constant mean, lengthscales and linear variances
 * (the jitter is a constant; Z is not differentiated).  One evaluation is the fit's pass over X and a second one: with
 * c_v = W m, e = r - K(Z, X)^T c_v, H = W (I - S) W^T,
 *   dF/dK(Z, X) = (H K(Z, X) + c_v e^T) / s2  is formed tile by tile and contracted with dK/dtheta on the spot,
 *   dF/dK_ZZ    = W (2I - S - B - m m^T) W^T / 2,   dF/dk(x_i, x_i) = -1 / (2 s2).
 * out (ntask x GPX_SVGP_GRAD_NOUT): F and its five terms in the GPX_SVGP_BOUND_* order (the bits
 * gpx_svgp_fit_collapsed_f64 writes for equal inputs and an equal chunk width), then from GPX_SVGP_GRAD_MLL on a block
 * in the layout of gpx_mll_grad_f64's output with -F in the place of -log p(y): out[GPX_SVGP_GRAD_MLL + GPX_MLL_NLL] =
 * -F, [.. + GPX_MLL_D_NOISE], [.. + GPX_MLL_D_OUTPUTSCALE], [.. + GPX_MLL_D_MEAN], [.. + GPX_MLL_D_LENGTHSCALE + k],
 * [.. + GPX_MLL_D_LINVAR + k] the derivatives of -F (QUAD, LOGDET and unused slots 0).
 * Arguments, info and the chunk rule as gpx_svgp_fit_collapsed_f64: chunks and tasks run in stream order without
 * floating-point atomics, so equal inputs and an equal chunk width give equal bits.
 * Workspace: gpx_svgp_bound_grad_workspace_size(M, n, ntask, chunk); with Mpad = gpx_padded_n(M), C the chunk width and
 * ldk = C rounded up to 256 it is about ntask 5 Mpad^2 8 + (1 + ntask) Mpad ldk 8 bytes (the fit's two matrices per
 * task and three more: W kept, H, and dF/dK_ZZ's inner matrix), and does not depend on n. */
enum {
  GPX_SVGP_GRAD_BOUND = 0,  /* GPX_SVGP_BOUND_NOUT values: F and its five terms */
  GPX_SVGP_GRAD_MLL = 8,    /* GPX_MLL_NOUT values in the GPX_MLL_* layout, of -F */
  GPX_SVGP_GRAD_NOUT = 80
};
gpx_status gpx_svgp_bound_grad_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes);
gpx_status gpx_svgp_bound_grad_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                   const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                   int64_t ldx, const double* Y, int64_t ldy, double* out, int32_t* info, void* ws,
                                   size_t ws_bytes);

/* The same evaluation together with the gradient with respect to the inducing locations.  Per task, with G_u =
 * dF/dK(Z, X) and G_A = dF/dK_ZZ as above and d1 the derivative in the first argument,
 *   dF/dz_ak = sum_i G_u[a][i] d1 k(z_a, x_i)_k + 2 sum_b G_A[a][b] d1 k(z_a, z_b)_k :
 * every tile of G_u, formed once, is contracted against dK/dtheta and against d1 k before it is dropped.
 * dZ (ntask x M x d; rows lddz >= d apart, tasks stride_dz >= M lddz apart when ntask > 1): dZ[t][a][k] =
 * d(-F_t)/dz_ak, the sign of the GPX_MLL block; columns k >= d of a wider row are not written.  out and info as
 * gpx_svgp_bound_grad_f64: for equal inputs and an equal chunk width out holds the bits that call writes.  A task whose
 * info is not 0 has unspecified dZ; the other tasks are computed.  The chunk rule and the determinism are those of
 * gpx_svgp_bound_grad_f64.  Workspace: gpx_svgp_bound_grad_z_workspace_size(M, n, ntask, chunk): the gradient's and
 * ntask Mpad GPX_MAX_DIM 8 + (Mpad / 128) max(Mpad / 128, C / 128) 128 GPX_MAX_DIM 8 bytes (the accumulators of dF/dZ
 * and the row partials of one launch).  A workspace of the size either call's size function reports for `chunk` gives
 * both calls the same chunk width. */
gpx_status gpx_svgp_bound_grad_z_workspace_size(int64_t M, int64_t n, int64_t ntask, int64_t chunk, size_t* bytes);
gpx_status gpx_svgp_bound_grad_z_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, double jitter,
                                     const double* Z, int64_t ldz, int64_t stride_z, const double* X, int64_t n,
                                     int64_t ldx, const double* Y, int64_t ldy, double* out, double* dZ, int64_t lddz,
                                     int64_t stride_dz, int32_t* info, void* ws, size_t ws_bytes);

/* ---- Conditioning the sparse model on new data -------------------------------------------------------------------- */
/* The exact Bayesian update of every task's whitened q(u) = N(m, C C^T) by new Gaussian observations (Xn, Yn):
 *   q'(u) proportional to q(u) prod_i N(y_i | const_mean + phi_i^T u, s2),  phi_i = L_ZZ^{-1} k(Z, x_i),  s2 = noise.
 * In the basis of the current posterior, u = m + C u~, with U = C^T Phi_n = W2^T K(Z, Xn) and the residual against the
 * current predictive mean e = y_n - (const_mean + K(Z, Xn)^T alpha'):
 *   P = I + U U^T / s2,  D lower triangular with positive diagonal and D D^T = P^{-1},  g = D D^T U e / s2,
 *   m_new = m + C g,  C_new = C D,  W2_new = W2 D,  alpha'_new = alpha' + W2 g.
 * For a state from gpx_svgp_fit_collapsed_f64 with the same p, Z and jitter, (m_new, C_new) is the collapsed fit of the
 * old and the new points together (Cholesky factors are unique).  For any other state it is the same update of that q:
 * S S^T <= I is not assumed, so a loaded checkpoint can be conditioned.  The bound of the enlarged data set is not
 * returned: it cannot be updated from (m, C) alone.  K_ZZ is not factorised again and the old points are not visited.
 * Z, W, W2, alpha: the prepared state, as gpx_svgp_predict_f64 takes it.  Xn: n_new x d, already input-transformed; Yn:
 * n_new x ntask, read by column; 1 <= n_new <= 2^30.
 * W2_out (ntask x Mpad x Mpad), alpha_out (ntask x Mpad): in the layout of the prepared blocks, rows / columns / entries
 * >= M exactly 0: with the unchanged Z and W they are a prepared state for gpx_svgp_predict_f64, gpx_svgp_acquire_f64,
 * gpx_svgp_moments_grad_f64 and this call again.
 * vmean, vchol (optional): the variational pair in the layout gpx_svgp_prepare_f64 reads (the lower triangle of vchol
 * only); vmean_out, vchol_out: the updated pair with the inputs' strides, vchol_out's strict upper triangle written as
 * exactly 0, its diagonal positive.  The four are given together or all NULL (any other mix: GPX_INVALID_ARG).
 * No output may be the input it is computed from (W2_out == W2, alpha_out == alpha, vmean_out == vmean, vchol_out ==
 * vchol: GPX_INVALID_ARG), and outputs must not overlap inputs: the old state stays valid.
 * info: int32[ntask], 0, or the failing pivot + 1 of P's factorisation, or, where that went through (P does not depend
 * on Yn) but the update g is not finite, 1 + the index of its first non-finite entry; either needs non-finite input,
 * since P >= I.  A failed task's outputs are unspecified; the other tasks are computed.
 * Asynchronous on the handle's stream, no allocation, no host synchronisation; fixed-order reductions and no
 * floating-point atomics: equal inputs and an equal chunk width give equal bits.
 * Workspace: gpx_svgp_condition_workspace_size(M, n_new, ntask, chunk); the chunk rule is gpx_svgp_fit_collapsed_f64's
 * (Xn is streamed in chunks of columns; `chunk` rounded up to a multiple of 128, 0 = GPX_SVGP_FIT_CHUNK; the call derives
 * its width from ws_bytes; below the chunk = 128 size: GPX_INVALID_ARG), and the size does not grow with n_new beyond
 * one chunk: about ntask 3 Mpad^2 8 + (1 + ntask) Mpad ldk 8 bytes. */
gpx_status gpx_svgp_condition_workspace_size(int64_t M, int64_t n_new, int64_t ntask, int64_t chunk, size_t* bytes);
gpx_status gpx_svgp_condition_f64(gpx_handle h, const gpx_kernel_params* p, int64_t ntask, int64_t M, const double* Z,
                                  int64_t ldz, int64_t stride_z, const double* W, const double* W2, const double* alpha,
                                  const double* Xn, int64_t n_new, int64_t ldx, const double* Yn, int64_t ldy,
                                  double* W2_out, double* alpha_out, const double* vmean /* or NULL */,
                                  int64_t stride_m, const double* vchol /* or NULL */, int64_t ldc, int64_t stride_c,
                                  double* vmean_out /* or NULL */, double* vchol_out /* or NULL */, int32_t* info,
                                  void* ws, size_t ws_bytes);

/* The k largest scores in descending order (replaces torch.topk, Bayesian7.py:681): stable, so equal scores keep
 * the lower index first; NaN ranks last.  idx_out: int64[k], val_out: double[k] (NULL = skip). */
gpx_status gpx_topk_workspace_size(int64_t m, size_t* bytes);
gpx_status gpx_topk_f64(gpx_handle h, const double* scores, int64_t m, int64_t k, int64_t* idx_out, double* val_out,
                        void* ws, size_t ws_bytes);

/* Greedy farthest point sampling of k of the m points X (m <= 32768), starting at index `start` (the reference
 * draws it with torch.randint): farthest_point_sampling of Bayesian7.py:82-106.  Squared Euclidean distances in
 * fp64, argmax with the lowest index among ties (torch.argmax).  idx_out: int64[k], the selection order. */
gpx_status gpx_fps_f64(gpx_handle h, const double* X, int64_t m, int64_t d, int64_t ldx, int64_t k, int64_t start,
                       int64_t* idx_out);

/* ---- instrumentation ------------------------------------------------------------------------------ */
/* For every timer whose bit is set in `mask`, each launch of that kernel family is bracketed by hipEvents
 * on the handle's stream; totals are read with gpx_timing_query (synchronises the stream). mask 0 = off. */
gpx_status gpx_timing_enable(gpx_handle h, int32_t mask);
gpx_status gpx_timing_reset(gpx_handle h);
gpx_status gpx_timing_query(gpx_handle h, int32_t timer, double* total_ms_host, int64_t* launches_host);

/* K(X, X*) through the candidate sweep's own K* build, for bit checks (no production path uses it): out (device,
 * padded_n rows of pitch ldout >= m rounded up to 256) gets column c = K(X, Xs[c]) for c < m, rows >= n zero.  With
 * list = NULL the full-store build (the full sweep's launch; ws of gpx_debug_kstar_workspace_size bytes for its mean
 * partials).  With a device index list and a device count (at most m) the gather build of the pruned sweep's tail:
 * column s = K(X, Xs[list[s]]) for s < *count, zero for a negative entry and up to the end of the last written
 * 256-column group; columns beyond are not written; ws is not used.  The gather build covers the fp64 covariance with
 * d <= 16.  A column has the same bits from either build.  Asynchronous on the handle's stream, no allocation. */
gpx_status gpx_debug_kstar_workspace_size(int64_t n, int64_t ldout, size_t* bytes);
gpx_status gpx_debug_kstar_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                               const double* Xs, int64_t m, int64_t ldxs, const int32_t* list, const int32_t* count,
                               double* out, int64_t ldout, void* ws, size_t ws_bytes);
/* The same builds with a device alpha (n values), returning their mean partials too (fp64 covariance, d <= 16).  Full
 * build (list = NULL): mu_part[jb * ldout + c] = sum over the 64 rows of block jb of alpha_j K(x_j, Xs[c]); the sweep's
 * mean is their sum over jb in ascending order.  Gather build: the partials of the listed candidates go to
 * mu_part[jb * ldmu + list[s]] (ldmu > every list entry) with the bits of the full build's; no other entry is written. */
gpx_status gpx_debug_kstar_mu_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* alpha, const double* Xs, int64_t m, int64_t ldxs, const int32_t* list,
                                  const int32_t* count, double* out, int64_t ldout, double* mu_part, int64_t ldmu);
/* The pruned sweep's bound of the posterior mean, through the production kernel (RBF, fp64 covariance, d <= 16; DESIGN
 * §3): mu_approx[c] - mu_slack[c] <= mu_c <= mu_approx[c] + mu_slack[c] for c < m, mu_c being the mean the full build's
 * partials sum to (without the constant mean).  ws: gpx_debug_mu_bound_workspace_size bytes; on return the int64 at its
 * start (rounded up to 256 bytes) counts the workgroups of 256 candidates that took the unfactorised form of the bound,
 * and the int64 at byte 160 from there those that took the fp64 factorised form (eligible for a factorised form, but d <=
 * 4, d > 8 or over the fp32 form's error limit); every other workgroup ran the fp32 factorised form. */
gpx_status gpx_debug_mu_bound_workspace_size(int64_t n, size_t* bytes);
gpx_status gpx_debug_mu_bound_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                  const double* alpha, const double* Xs, int64_t m, int64_t ldxs, double* mu_approx,
                                  double* mu_slack, void* ws, size_t ws_bytes);
/* Which head the lazy pruned sweep of this handle runs (fp64 covariance, d <= 16; A/B measurements and tests, not a
 * tuning option: it has no slot among GPX_OPT_* and no GPX_OPTIONS name).  1 (default): K* rows 0 .. 127 are built in
 * registers and multiplied into row tile 0 of the product by one kernel.  0: a K* launch that stores them and the
 * product's first stage that reads them back.  The same bits and the same gpx_sweep_stats either way.  Any other value
 * is GPX_INVALID_ARG. */
gpx_status gpx_debug_set_sweep_head(gpx_handle h, int32_t value);
gpx_status gpx_debug_get_sweep_head(gpx_handle h, int32_t* value_host);
/* The lazy pruned sweep's fused head through the production kernel, for bit checks (fp64 covariance, d <= 16; DESIGN
 * §3): of every candidate c < m rounded up to 256 (candidates >= m are the origin), from training rows 0 .. 127 alone,
 * ss[c] = the sum over rows 0 .. 127 of V[.][c]^2, V = W^T K*, and mu_part[jb * ldmu + c], jb = 0, 1, the mean partials
 * of row blocks 0 and 1.  W: device, upper triangular, at least 128 x 128 of pitch ldw >= padded_n (its leading 128 x
 * 128 block is read); ss: ldmu values; mu_part: 2 rows of pitch ldmu >= m rounded up to 256.  The bits are those of
 * gpx_debug_kstar_mu_f64's full build followed by gpx_debug_stage_product_f64 of row tile 0.  Any n >= 1.
 * Asynchronous on the handle's stream, no allocation, no workspace. */
gpx_status gpx_debug_head_product_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X, int64_t ldx,
                                      const double* alpha, const double* Xs, int64_t m, int64_t ldxs, const double* W,
                                      int64_t ldw, double* ss, double* mu_part, int64_t ldmu);
/* The same kernel's list-driven instance (the mean-first order's head): of the candidates list[2 s], s = 0 ..
 * *count - 1 (list: device, 8-byte aligned, pairs of int32 {candidate in [0, m), ignored}, at most m rounded up to 256
 * pairs; count: device), ss[c] and mu_part[jb * ldmu + c] at the candidate's own place c with the bits gpx_debug_head_product_f64
 * gives that candidate; no other entry is written, and a count of 0 writes nothing. */
gpx_status gpx_debug_head_product_list_f64(gpx_handle h, const gpx_kernel_params* p, int64_t n, const double* X,
                                           int64_t ldx, const double* alpha, const double* Xs, int64_t m, int64_t ldxs,
                                           const double* W, int64_t ldw, double* ss, double* mu_part, int64_t ldmu,
                                           const int32_t* list, const int32_t* count);
/* The order of the lazy pruned sweep's seeded spans and of the spans behind them (calls longer than one chunk, RBF with
 * the mean's bound, the fused head, EI or logEI, the top-k form up to k = 64; A/B measurements and tests, no slot among
 * GPX_OPT_*).  1 (default): mean-first: the
 * columns are ranked and pruned on the mean's bound with the prior variance, and K* rows 0 .. 127 and row tile 0 of the
 * product are built only for the columns that pass.  0: the head over every column first.  The same results either
 * way; gpx_sweep_stats [1] and [2] count what ran.  Any other value is GPX_INVALID_ARG. */
gpx_status gpx_debug_set_sweep_order(gpx_handle h, int32_t value);
gpx_status gpx_debug_get_sweep_order(gpx_handle h, int32_t* value_host);
/* The tail of the lazy pruned sweep (gpx_acquire_argmax_f64 and gpx_acquire_topk_f64 at padded n >= 384; no
 * slot among GPX_OPT_*).  1 (default): in every span whose survivors could need more than one round (more staged columns
 * than a chunk holds) the call copies the span's survivor count to the host, enqueues the first round, waits for the
 * copy (hipEventSynchronize: the call blocks the calling thread once per such span) and enqueues only the rounds the
 * count needs.  0: the worst-case number of rounds is enqueued and the call never waits.  A call on a stream that is
 * being captured behaves as 0, so a captured graph replays for any count.  The same results and gpx_sweep_stats either
 * way.  Any other value is GPX_INVALID_ARG. */
gpx_status gpx_debug_set_sweep_tail_sync(gpx_handle h, int32_t value);
gpx_status gpx_debug_get_sweep_tail_sync(gpx_handle h, int32_t* value_host);
/* Of the handle's last gpx_acquire_argmax_f64 or gpx_acquire_topk_f64 call, summed over its spans: out[0] tail rounds
 * enqueued, out[1] their worst case, out[2] the survivor counts read back (-1: no span read one back).  All 0, 0, -1
 * where the lazy pruned sweep did not run.  Host-side values: no synchronisation, no device access. */
gpx_status gpx_debug_get_tail_rounds(gpx_handle h, int64_t* out);
/* One stage of the pruned sweep's product in a named tile shape, for bit checks (no production path uses it; DESIGN
 * §3): row tiles I0 .. I0 + nrows - 1 of V = W^T K* over slots 0 .. ncols - 1 of a caller's K* buffer.  W: device,
 * padded_n x padded_n upper triangular (pitch ldw), kstar: device, padded_n rows of pitch ldk >= ncols rounded up to
 * 128 (the tiles read whole 128-column groups), both 16-byte aligned with even pitches.  shape 0: the wide 128 x 128
 * tile, 1: the narrow 128 x 32 one.  ss[I * ldss + c] gets the sum over the 128 rows of row tile I of V[.][slot]^2,
 * c = slot without a list (every slot up to ncols rounded up to 128 is written), else c = list[slot] (device, ncols
 * entries in [-1, ldss); -1 marks a padding slot, which is not written).  A column has the same bits in either shape.
 * ws: device, gpx_debug_stage_product_workspace_size bytes.  Asynchronous on the handle's stream, no allocation. */
gpx_status gpx_debug_stage_product_workspace_size(int64_t ncols, size_t* bytes);
gpx_status gpx_debug_stage_product_f64(gpx_handle h, int64_t n, const double* W, int64_t ldw, const double* kstar,
                                       int64_t ldk, int64_t ncols, const int32_t* list, int32_t I0, int32_t nrows,
                                       int32_t shape, double* ss, int64_t ldss, void* ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H */
