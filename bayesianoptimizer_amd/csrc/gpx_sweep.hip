// Posterior / acquisition sweep over a chunk of C candidates.
// Replaces model.posterior(X) (optimization/Bayesian2.py:169-171, optimization/Bayesian6.py:615-617,688-690),
// the raw-sample sweep + argmax inside optimize_acqf (optimization/Bayesian.py:105-113) and the pool scan +
// top-k of optimization/Bayesian7.py:646-681.
//
// Per chunk, three launches:
//  1. kstar_kernel   K*[j][c] = k(x_j, xs_c) for all padded rows j (row-major npad x C, zero for j >= n),
//                    and the partial means mu_part[jb][r][c] = sum_{j in block jb} alpha[j][r] K*[j][c].
//  2. trmm_sumsq     V = L^{-1} K* = W^T K* as a triangular fp64-MFMA product (128x128 tiles, k < (I+1)*128
//                    for row tile I), never stored: each workgroup writes the column sums of V^2 over its 128
//                    rows into ss_part[I][c].  This is the n^2-flops-per-candidate term and the dominant
//                    kernel of the whole hot path.
//  3. finalize       mu = m + sum mu_part, var = k** - sum ss_part (fixed summation order: deterministic),
//                    GPyTorch/BoTorch variance floors, Standardize untransform, analytic acquisition, and a
//                    256-candidate block argmax record (max value, then lowest index; NaN never wins).  One body,
//                    finalize_kernel<PASS>, compiled per pass (FinalizePass): the posterior, one output into a
//                    multi-output objective's accumulators, and score or bound from the partials or the accumulators.
// launch_argmax_final reduces the records of the whole sweep in one workgroup.
// gpx_acquire_argmax_f64 without scores_out takes the PRUNED form of launch 2 (launch_sweep_chunk_pruned):
// the row tiles run in stages (trmm_stage_kernel; after the first trmm_stage_dual_kernel, whose workgroups take a
// 128 x 32 tile when the stage has fewer 128 x 128 tiles than the device has CUs); after each stage finalize_kernel's
// bound pass drops the candidates whose score bound cannot reach the best score computed in full so far, and
// prune_compact_kernel gathers the surviving K* columns; the (value, index) pair has the bits of the full sweep.  Where
// the MFMA K* build applies the pruned form is lazy (launch_sweep_super_pruned): K* rows 0 .. 127 for every candidate,
// built in registers and multiplied into row tile 0 by one kernel (head_product_kernel; gpx_debug_set_sweep_head 0:
// stored by a K* launch and read back by the first stage), full-height columns rebuilt from the survivor list; a call
// longer than one chunk takes its first incumbent from the head's bound (seed_select_kernel, seed_prune_kernel).  Both share launch_seed_block and launch_stages;
// gpx_acquire_topk_f64 is the same sweep with the k-th best exact score as its incumbent (topk_pool_kernel), and
// gpx_acquire_topk_multi_f64 (launch_topk_multi_chunk) its form for a linear objective over independent outputs: one
// head tile per output, the variance bounds summed in the accumulators before one bound pass.
// Workspace: gpx_sweep_layout.h (sweep_carve, gpx_internal.h, turns it into pointers); head mean bound: gpx_mubound.hip.
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_trmm_asm.h"
#include <cstdlib>
#include <type_traits>

namespace gpx {

// ---- acquisition math (BoTorch analytic forms [upstream], restated; oracle/gp_oracle.py mirrors them) ----
__device__ __forceinline__ double ndtr_d(double a) {  // standard normal cdf, cephes-style branches
  const double x = a * 0.70710678118654752440084436210485;
  const double z = fabs(x);
  if (z < 0.70710678118654752440084436210485) return 0.5 + 0.5 * erf(x);
  const double y = 0.5 * erfc(z);
  return (x > 0.0) ? 1.0 - y : y;
}
__device__ __forceinline__ double phi_d(double u) { return exp(-0.5 * u * u) * 0.39894228040143267793994605993438; }
__device__ __forceinline__ double ei_helper_d(double u) { return phi_d(u) + u * ndtr_d(u); }
__device__ __forceinline__ double log1mexp_d(double x) {
  return (x > -0.69314718055994530941723212145818) ? log(-expm1(x)) : log1p(-exp(x));
}
// log(phi(u) + u Phi(u)): the log of the sum down to u = -1, the erfcx form down to -1024, the asymptotic series below.
// The erfcx form takes log(1 - e^w) of w ~ -1/u^2, which it knows to ~1e-16 only: it loses u^2 eps of the sum, and at
// BoTorch's hand-over -1/sqrt(eps) [upstream] the rounded w reaches 0 and beyond (log of zero or of a negative number).
// The series u^-2 (1 - 3 u^-2 + 15 u^-4) loses 105 u^-6, below eps from 1024 on.
__device__ __forceinline__ double log_ei_helper_d(double u) {
  const double asymptotic_bound = -1024.0;
  if (u > -1.0) return log(ei_helper_d(u));
  const double log_phi = -0.5 * u * u - 0.91893853320467274178032973640562;  // log(sqrt(2 pi))
  if (u > asymptotic_bound) {
    const double w = log(erfcx(-u * 0.70710678118654752440084436210485) * fabs(u)) +
                     0.22579135264472743236309761494744;  // log(sqrt(pi/2))
    return log_phi + log1mexp_d(w);
  }
  const double r = 1.0 / (u * u);
  return log_phi - 2.0 * log(fabs(u)) + log1p(r * (15.0 * r - 3.0));
}
// EI: phi(u) and Phi(u) are denormal below u ~ -37.5 and their difference may round below zero; EI is not negative.
__device__ __forceinline__ double acq_score(int kind, double mu, double var, double best_f, double beta) {
  const double sigma = sqrt(var);
  if (kind == GPX_ACQ_EI) {
    const double h = ei_helper_d((mu - best_f) / sigma);
    return sigma * (h < 0.0 ? 0.0 : h);  // NaN stays NaN
  }
  if (kind == GPX_ACQ_LOGEI) return log_ei_helper_d((mu - best_f) / sigma) + log(sigma);
  if (kind == GPX_ACQ_UCB) return mu + sqrt(beta) * sigma;
  return var;
}

// Sum of `cnt` partials spaced `stride` apart, in a fixed order: 8 independent loads in flight per group
// (a plain loop over a runtime count waited for every load before the next: 32 serial round trips).
__device__ __forceinline__ double sum_partials(const double* __restrict__ p, int cnt, int64_t stride) {
  double s = 0.0;
  int i = 0;
  for (; i + 8 <= cnt; i += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = p[(int64_t)(i + q) * stride];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  for (; i < cnt; ++i) s += p[(int64_t)i * stride];
  return s;
}

// (value, index) order: larger value wins, equal values -> lower index; NaN already mapped to -inf.
__device__ __forceinline__ void argmax_merge(double& v, int64_t& i, double v2, int64_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// The pruned sweep's incumbent as an unsigned key with the order of the doubles (NaN never stored), so that the best
// exact score so far is one atomicMax whatever the order of the workgroups.
__device__ __forceinline__ unsigned long long tau_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double tau_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <int DMAX>
__device__ __forceinline__ void load_point(const gpx_kernel_params& p, const double* __restrict__ x, bool valid,
                                           double (&xs)[DMAX], double (&xr)[DMAX]) {
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    const double v = (valid && k < p.d) ? x[k] : 0.0;
    xs[k] = (k < p.d) ? v / p.lengthscale[k] : 0.0;
    xr[k] = v;
  }
}

// ---- 1. K* and partial means ---------------------------------------------------------------------------
// KIND and ONE_RHS are compile-time so the per-element loop carries no uniform branches (kind dispatch, nrhs
// predicates); dimensions k >= d are zero in both sx/sr and xs/xr, so the distance and linear sums run over all DMAX
// without a k < d test (adding +0 leaves r2 and lv bitwise unchanged).  Rows j >= n of the last block are zero.
template <int DMAX, bool F32, int KIND, bool ONE_RHS>
__global__ void __launch_bounds__(WG) kstar_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                   int64_t ldx, const double* __restrict__ alpha, int nrhs,
                                                   const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                   int64_t C, double* __restrict__ kstar,
                                                   double* __restrict__ mu_part) {
  __shared__ double sx[NB][DMAX + 1], sr[NB][DMAX + 1], sa[NB][GPX_MAX_RHS];
  const int jb = blockIdx.y;
  const int j0 = jb * NB;
  const int d = p.d;
  for (int e = threadIdx.x; e < NB * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    double v = 0.0;
    if (k < d && j0 + r < n) v = X[(int64_t)(j0 + r) * ldx + k];
    sx[r][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
    sr[r][k] = (k < d) ? v * p.linear_variance[k] : 0.0;
  }
  for (int e = threadIdx.x; e < NB * nrhs; e += WG) {
    const int r = e / nrhs, q = e % nrhs;
    sa[r][q] = alpha[(int64_t)(j0 + r) * nrhs + q];
  }
  __syncthreads();
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  const bool valid = c < m_chunk;
  double xs[DMAX], xr[DMAX];
  load_point<DMAX>(p, Xs + (valid ? c * ldxs : 0), valid, xs, xr);
  double mu[GPX_MAX_RHS];
#pragma unroll
  for (int q = 0; q < GPX_MAX_RHS; ++q) mu[q] = 0.0;
  const int jn = n - j0 < NB ? n - j0 : NB;  // real rows of this block (<= 0 for an all-padding block)
  int j = 0;
  // four rows in flight (independent distance / exp chains; the mean accumulates in row order)
#pragma unroll 4
  for (; j < jn; ++j) {
    double lv = 0.0;
    if (KIND == GPX_KERNEL_SCALE_LINEAR_MATERN52) {
#pragma unroll
      for (int k = 0; k < DMAX; ++k) lv += sr[j][k] * xr[k];
    }
    double kv;
    if (F32) {
      float r2 = 0.0f;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        const float df = (float)sx[j][k] - (float)xs[k];
        r2 += df * df;
      }
      kv = cov_from_r2_f32(KIND, p.outputscale, r2, lv);
    } else {
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        const double df = sx[j][k] - xs[k];
        r2 += df * df;
      }
      kv = cov_from_r2(KIND, p.outputscale, r2, lv);
    }
    kstar[(int64_t)(j0 + j) * C + c] = kv;
    if (ONE_RHS) {
      mu[0] += sa[j][0] * kv;
    } else {
#pragma unroll
      for (int q = 0; q < GPX_MAX_RHS; ++q)
        if (q < nrhs) mu[q] += sa[j][q] * kv;
    }
  }
  for (; j < NB; ++j) kstar[(int64_t)(j0 + j) * C + c] = 0.0;
  for (int q = 0; q < nrhs; ++q) mu_part[((int64_t)jb * nrhs + q) * C + c] = mu[q];
}

// fp64 K* with the distance's cross term on the matrix cores (GPyTorch's ||a||^2 + ||b||^2 - 2 a.b clamped at 0
// [upstream]; gram_mfma_kernel's arithmetic, centred by the mean of the workgroup's valid training rows).  A workgroup
// owns the 64 training rows of block jb x 256 candidates, wave w the candidates 64 w .. 64 w + 63 (four 16-column MFMA
// blocks) over the four 16-row strips.  The MFMA accumulator gives a lane rows kq + 4 r of column m of a block; before the
// stores, each group of four registers (the four column blocks of one r) is transposed across the wave's four 16-lane
// rows by two v_permlane32_swap + two v_permlane16_swap, so every store instruction writes one K* row of 64 consecutive
// candidates (512 bytes) like the difference-form kernel (an untransposed first version, four 128-byte row segments per
// instruction, ran at 3.5 vs 4.7 TB/s).  Per element: one fma, a compare and the covariance, no per-dimension VALU work.
//
// MODE (one element arithmetic for all three: a column's K* entries have the same bits whichever mode built them, whatever
// slot it sits in):
//  KSTAR_FULL    every row block stores its rows and its mean partials (the full sweep, the seed block).
//  KSTAR_MU      the pruned sweep's head phase beyond the head rows: row blocks aux.jb0 + blockIdx.y add their mean
//                partials and store no K* (the head rows themselves, PRUNE_HEAD_ROWS of them, are a KSTAR_FULL launch
//                over the first row blocks: the rows the first stage of the product reads).
//  KSTAR_GATHER  the pruned sweep's tail: column s of the output is candidate list[first + s] for s below the round's
//                column count min(*count - first, cap) (clamped at 0), zero up to the end of the workgroup's 256 columns;
//                mean partials only on request (aux.mu_out: KSTAR_FULL's bits, stored at the listed candidate's own
//                place).  The grid is one-dimensional and bounded (tail_grid): its workgroups stride over the live
//                (column block, row block) units, column block fastest, so an empty round costs that bounded grid
//                of workgroups that read the count and return.  Workgroup 0 also writes the round's first descriptor
//                and resets its survivor counts (read by later launches only), once, before its first unit.
constexpr int KSTAR_FULL = 0, KSTAR_MU = 1, KSTAR_GATHER = 2;
struct KstarAux {
  int jb0;           // MU: first row block of the launch
  const int* list;   // GATHER: entry s at list[s * lstride] (the survivor list's int2 .x, or a plain index array)
  int lstride;
  const int* count;  // GATHER: entries in the list (device)
  int first, cap;    // GATHER: this round's entries first .. first + cap - 1
  int nrb;           // GATHER: row blocks of the launch (set by launch_kstar)
  int* pad;          // GATHER, optional: the list again, to mark the last tile's padding slots with -1
  PruneDesc* desc;   // GATHER, optional: the round's first descriptor
  int* rcount;       // its stages' survivor counts (PRUNE_MAX_STAGES - 1 of them)
  int64_t* stats;    // the pruned sweep's counters
  int rows0, last;   // row tiles of the round's first stage; it is also the last
  double* mu_out;    // GATHER, optional: the listed candidates' mean partials (KSTAR_FULL's bits) go to
  int64_t ldmu;      //   mu_out[jb * ldmu + candidate]; alpha is read only then
};

// One workgroup's unit of kstar_mfma_kernel: row block jb x the 256 columns from c0 on.  GATHER: nr columns in the
// round, ntl tiles.
template <int DMAX, int KIND, bool ONE_RHS, int MODE>
__device__ __forceinline__ void kstar_mfma_unit(const gpx_kernel_params& p, int n, const double* __restrict__ X,
                                                int64_t ldx, const double* __restrict__ alpha, int nrhs,
                                                const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                int64_t C, double* __restrict__ kstar, double* __restrict__ mu_part,
                                                const KstarAux& aux, int jb, int64_t c0, int nr, int ntl) {
  constexpr bool lin = (KIND == GPX_KERNEL_SCALE_LINEAR_MATERN52);
  constexpr bool gather = MODE == KSTAR_GATHER;
  constexpr int KS = DMAX / 4;
  constexpr int NRQ = ONE_RHS ? 1 : GPX_MAX_RHS;
  __shared__ double sa[NB][DMAX + 1], sb[WG][DMAX + 1], ra[lin ? NB : 1][DMAX + 1], rb[lin ? WG : 1][DMAX + 1];
  __shared__ double na[NB], nb[WG], cen[DMAX], sal[NB][NRQ];
  __shared__ int sidx[gather ? WG : 1];
  const int j0 = jb * NB, d = p.d;
  int t = threadIdx.x;
  // (GATHER runs this body in a loop: an opaque thread index keeps the compiler from hoisting every address that
  // depends on it out of the loop, which cost the d = 8 instance its fourth wave per SIMD)
  if constexpr (gather) asm volatile("" : "+v"(t));
  const int nv = n - j0 < NB ? n - j0 : NB;  // valid training rows of the block (<= 0: all padding)
  if constexpr (gather) {
    const int slot = (int)c0 + t;
    sidx[t] = slot < nr ? aux.list[(int64_t)(aux.first + slot) * aux.lstride] : -1;
    if (aux.pad && jb == 0 && slot >= nr && slot < ntl * 128)
      aux.pad[(int64_t)(aux.first + slot) * aux.lstride] = -1;
    __syncthreads();
  }
  for (int e = t; e < NB * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    const double v = (k < d && j0 + r < n) ? X[(int64_t)(j0 + r) * ldx + k] : 0.0;
    sa[r][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
    if constexpr (lin) ra[r][k] = (k < d) ? v * p.linear_variance[k] : 0.0;
  }
  for (int e = t; e < WG * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    double v;
    if constexpr (gather)
      v = (k < d && sidx[r] >= 0) ? Xs[(int64_t)sidx[r] * ldxs + k] : 0.0;
    else
      v = (k < d && c0 + r < m_chunk) ? Xs[(c0 + r) * ldxs + k] : 0.0;
    sb[r][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
    if constexpr (lin) rb[r][k] = v;
  }
  if constexpr (!gather) {
    for (int e = t; e < NB * NRQ; e += WG) {
      const int r = e / NRQ, q = e % NRQ;
      sal[r][q] = (q < nrhs && j0 + r < n) ? alpha[(int64_t)(j0 + r) * nrhs + q] : 0.0;
    }
  } else {
    if (t < NB) sal[t][0] = (aux.mu_out && j0 + t < n) ? alpha[j0 + t] : 0.0;
  }
  __syncthreads();
  if (t < DMAX) {
    double s = 0.0;
    for (int r = 0; r < nv; ++r) s += sa[r][t];
    cen[t] = nv > 0 ? s / nv : 0.0;
  }
  __syncthreads();
  for (int e = t; e < NB * DMAX; e += WG) sa[e / DMAX][e % DMAX] -= cen[e % DMAX];
  for (int e = t; e < WG * DMAX; e += WG) sb[e / DMAX][e % DMAX] -= cen[e % DMAX];
  __syncthreads();
  {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) v = fma(sb[t][k], sb[t][k], v);
    nb[t] = v;
    if (t < NB) {
      double u = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) u = fma(sa[t][k], sa[t][k], u);
      na[t] = u;
    }
  }
  __syncthreads();
  const int lane = t & 63, w = t >> 6, m = lane & 15, kq = lane >> 4;
  double mu[4][NRQ];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < NRQ; ++q) mu[cb][q] = 0.0;
  double nbc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) nbc[cb] = nb[64 * w + 16 * cb + m];
  bool cok[4] = {true, true, true, true};  // GATHER: the column is a listed candidate (else a zero column)
  if constexpr (gather) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) cok[cb] = sidx[64 * w + 16 * cb + m] >= 0;
  }
#pragma unroll 1
  for (int rs = 0; rs < NB; rs += 16) {
    double kv[4][4];  // [r][cb]: row rs + kq + 4 r, candidate 64 w + 16 cb + m
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      d4 acc = {0.0, 0.0, 0.0, 0.0}, lac = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        acc = mfma16x16x4(sa[rs + m][4 * k + kq], sb[64 * w + 16 * cb + m][4 * k + kq], acc);
        if constexpr (lin) lac = mfma16x16x4(ra[rs + m][4 * k + kq], rb[64 * w + 16 * cb + m][4 * k + kq], lac);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = rs + kq + 4 * r;
        double v = cov_from_r2(KIND, p.outputscale, sqdist_expanded(na[j], nbc[cb], acc[r]), lin ? lac[r] : 0.0);
        if constexpr (gather)
          v = (j < nv && cok[cb]) ? v : 0.0;
        else
          v = j < nv ? v : 0.0;
        kv[r][cb] = v;
#pragma unroll
        for (int q = 0; q < NRQ; ++q) mu[cb][q] = fma(sal[j][q], v, mu[cb][q]);
      }
    }
    // after the transpose, register q of 16-lane row g holds row rs + q + 4 r, candidate 64 w + 16 g + m
    if constexpr (MODE != KSTAR_MU) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        transpose_rows4(kv[r]);
#pragma unroll
        for (int q = 0; q < 4; ++q) kstar[(int64_t)(j0 + rs + q + 4 * r) * C + c0 + 64 * w + lane] = kv[r][q];
      }
    }
  }
  if constexpr (gather) {
    // the survivors' exact mean partials, at the candidates' own places (the head bounded their means only)
    if (!aux.mu_out) return;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      double v = mu[cb][0];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      const int sc = sidx[64 * w + 16 * cb + m];
      if (kq == 0 && sc >= 0) aux.mu_out[(int64_t)jb * aux.ldmu + sc] = v;
    }
    return;
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < NRQ; ++q) {
      double v = mu[cb][q];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (kq == 0 && q < nrhs) mu_part[((int64_t)jb * nrhs + q) * C + c0 + 64 * w + 16 * cb + m] = v;
    }
}

template <int DMAX, int KIND, bool ONE_RHS, int MODE>
__global__ void __launch_bounds__(WG) kstar_mfma_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                        int64_t ldx, const double* __restrict__ alpha, int nrhs,
                                                        const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                        int64_t C, double* __restrict__ kstar,
                                                        double* __restrict__ mu_part, KstarAux aux) {
  if constexpr (MODE != KSTAR_GATHER) {
    const int jb = MODE == KSTAR_MU ? (int)blockIdx.y + aux.jb0 : (int)blockIdx.y;
    kstar_mfma_unit<DMAX, KIND, ONE_RHS, MODE>(p, n, X, ldx, alpha, nrhs, Xs, ldxs, m_chunk, C, kstar, mu_part, aux, jb,
                                               (int64_t)blockIdx.x * WG, 0, 0);
  } else {
    const int left = *aux.count - aux.first;
    const int nr = left < 0 ? 0 : left < aux.cap ? left : aux.cap;
    const int ntl = (nr + 127) / 128;
    if (blockIdx.x == 0 && threadIdx.x == 0 && aux.desc) {
      PruneDesc o;
      o.buf = 0;
      o.col0 = 0;
      o.ncols = nr;
      o.ntiles = ntl;
      o.list = 2;
      o.pad[0] = o.pad[1] = o.pad[2] = 0;
      *aux.desc = o;
      for (int s = 0; s < PRUNE_MAX_STAGES - 1; ++s) aux.rcount[s] = 0;
      aux.stats[1] += (int64_t)ntl * aux.rows0;
      if (aux.last) aux.stats[0] += nr;
    }
    const int ncb = (nr + WG - 1) / WG, units = ncb * aux.nrb;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
      if (u != (int)blockIdx.x) __syncthreads();  // the unit before this one has read its LDS image to the end
      kstar_mfma_unit<DMAX, KIND, ONE_RHS, MODE>(p, n, X, ldx, alpha, nrhs, Xs, ldxs, m_chunk, C, kstar, mu_part, aux,
                                                 u / ncb, (int64_t)(u % ncb) * WG, nr, ntl);
    }
  }
}

// ---- 2. triangular product + column sums of squares ------------------------------------------------------
// (TT = 128, gpx_sweep_layout.h: the trmm tile, rows of V x candidates)
using TrmmTile = MfmaTile<TT, TT, 16, true, true>;  // its accumulator layout (row_of / col_of) and LDS size
static_assert(TrmmTile::LDS_DOUBLES * 8 == trmm_asm::LDS_BYTES, "hand-placed tile uses MfmaTile's LDS image");

// Workgroup b of a launch over `nrows` row tiles x `ncb` candidate tiles -> (l, cb), l = 0 the heaviest row tile.
// Candidate tiles in groups of G = 64 (every row tile of a group, heaviest first, before the next group), and inside a
// group XCD-aware: workgroups b, b+8, ... share an XCD (dispatch is round-robin; speed only, never correctness), so
// XCD x gets the group's candidate tiles cb = x (mod 8) and walks them row tile by row tile.  Groups keep the K*
// panels the resident workgroups read to a quarter of the chunk at n = 4096: 7.65 vs 8.03 ms per launch (tools/
// trmm_asm_bench.hip A4 vs A2, profiles/r05_trmm_asm_groups.log; groups of 16 / 32 / 128: 8.17 / 7.91 / 7.82 ms).
__device__ __forceinline__ void trmm_tile_order(int b, int nrows, int ncb, int& l, int& cb) {
  constexpr int G = 64;
  if ((ncb % G) == 0) {
    const int g = b / (nrows * G), bb = b % (nrows * G);
    const int x = bb & 7, q = bb >> 3;
    l = q / (G / 8);
    cb = g * G + 8 * (q % (G / 8)) + x;
  } else if ((ncb & 7) == 0) {
    const int x = b & 7, q = b >> 3, per = ncb >> 3;
    l = q / per;
    cb = 8 * (q % per) + x;
  } else {
    l = b / ncb;
    cb = b % ncb;
  }
}

// The buffers a stage of the pruned sweep can read its K* columns from, and the two index lists (PruneDesc).
struct PruneBufs {
  const double* kstar;
  double* c1;
  double* c2;
  int64_t ld0, ld1, ld2;
  int2* list0;
  int2* list1;
  const int2* list2;  // the round's part of the head phase's survivor list (PruneDesc::list = 2)
};
// One stage of the pruned sweep (trmm_stage_kernel / trmm_stage_dual_kernel).
struct PruneStage {
  PruneBufs pb;
  const PruneDesc* desc;  // the active columns, written by an earlier launch
  int I0, nrows;          // the stage's row tiles I0 .. I0 + nrows - 1
  int narrow_below;       // dual kernel: the narrow shape runs when desc->ntiles * nrows is below this (0: never)
};

// The NARROW shape of the product's tile: 128 rows x 32 columns, a quarter of the wide tile's columns with the same four
// waves in 2 x 2 (MfmaTile<128, 32, ..>: WM = 4 row blocks, WN = 1, the wide tile's row_of).  A stage that has fewer
// wide tiles than the device has CUs lasts as long as its deepest tile, one workgroup walking (I + 1) k-ranges of 64
// MFMAs per wave and k-tile while the other CUs idle; four narrow workgroups compute the same 128 columns with 16 MFMAs
// per wave and k-tile each.  Bits: a 16 x 16 accumulator block's MFMA chain (k ascending in steps of 4 from 0, lane
// (kr, m) supplying W[k0 + kr][I*128 + m] and K*[k0 + kr][c]) does not depend on the blocks that share its workgroup,
// the diagonal 128-block skips the zero row blocks by run_tri's rule, and the column sums are trmm_colsum_store's for
// both shapes, so a column's partial is the wide tile's.
// No LDS staging: with 16 MFMAs (~1000 cycles) per k-tile a workgroup cannot cover a load round trip behind one staged
// tile, and a combined kernel must keep the wide shape's 73,728 B of LDS (two workgroups per CU).  Every wave
// loads its own fragments straight into registers (each 16-lane row a contiguous 128 bytes of one k-row; the A
// fragments are read by the two waves of a row half, the B fragment by the two of a column half: L1 / L2 hits) in
// blocks of one k-tile (16 fragment loads A + 4 B), four blocks in registers: three k-tiles (~3000 cycles of MFMAs)
// between a block's loads and its use, against ~550 / ~900 cycles of Infinity Cache / HBM latency.  The kernels of this
// shape are held to 256 registers (__launch_bounds__(WG, 2)): two waves per SIMD, as the wide shape has.  Measured
// (DESIGN §5): 5.4 us per k-range of 128 against the wide tile's 13.6; the 80 fragment loads per CU and k-tile, not the
// MFMAs (3.4 us), set the pace.
constexpr int TNW = 32;
using NarrowTile = MfmaTile<TT, TNW, 16, true, true>;  // (layout only: row_of / col_of)
static_assert(NarrowTile::WM == TrmmTile::WM && NarrowTile::WN == 1, "the wide tile's row blocks, one column block");
struct TrmmNarrow {
  struct Blk {  // the fragments of one k-tile of 16: substep s, row block i
    double a[4][4], b[4];
  };
  d4 acc[4][1];
  const double* pa;  // W[kr][I*128 + wm0 + cl], advanced by k-tile
  const double* pb;  // K*[kr][column wn0 + cl]
  int64_t lda, ldb;

  // (sched_barrier: hipcc's scheduler otherwise gathers the four blocks' loads at the top of a loop trip and waits for
  // them there, which exposes a load round trip per trip)
  __device__ __forceinline__ void load(Blk& f, int kt) const {
    __builtin_amdgcn_sched_barrier(0);
    const double* a = pa + (int64_t)kt * 16 * lda;
    const double* b = pb + (int64_t)kt * 16 * ldb;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < 4; ++i) f.a[s][i] = a[(int64_t)(4 * s) * lda + 16 * i];
      f.b[s] = b[(int64_t)(4 * s) * ldb];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // SKIP (0 .. 4): the wave's first SKIP row blocks are zero in this k-tile of W (TileT::ktile's rule)
  template <int SKIP>
  __device__ __forceinline__ void mm(const Blk& f) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = SKIP; i < 4; ++i) acc[i][0] = mfma16x16x4(f.a[s][i], f.b[s], acc[i][0]);
  }
  // local k-tile J of the diagonal 128-block: the waves of rows 0-63 (lo = 0) skip their row blocks i < J, the waves of
  // rows 64-127 (lo = 4) their row blocks i < J - 4 (run_tri's rule)
  template <int J>
  __device__ __forceinline__ void mm_diag(const Blk& f, int lo) {
    if (lo == 0)
      mm<(J < 4 ? J : 4)>(f);
    else
      mm<(J > 4 ? J - 4 : 0)>(f);
  }
  // acc = A B over nk k-tiles of 16 (nk a multiple of 8) for an upper-triangular block row A whose last 8 k-tiles are
  // the diagonal 128-block
  __device__ __forceinline__ void run(const double* __restrict__ Ag, int64_t lda_, const double* __restrict__ Bg,
                                      int64_t ldb_, int nk) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, kr = lane >> 4, cl = lane & 15;
    lda = lda_;
    ldb = ldb_;
    pa = Ag + (int64_t)kr * lda + (w >> 1) * (TT / 2) + cl;
    pb = Bg + (int64_t)kr * ldb + (w & 1) * (TNW / 2) + cl;
    const int lo = __builtin_amdgcn_readfirstlane(w >> 1) == 0 ? 0 : 4;
    const int kd = nk - 8;  // first k-tile of the diagonal block
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = (d4){0.0, 0.0, 0.0, 0.0};
    Blk f0, f1, f2, f3;
    load(f0, 0);
    load(f1, 1);
    load(f2, 2);
    load(f3, 3);
    for (int kt = 0; kt < kd; kt += 4) {
      mm<0>(f0);
      load(f0, kt + 4);
      mm<0>(f1);
      load(f1, kt + 5);
      mm<0>(f2);
      load(f2, kt + 6);
      mm<0>(f3);
      load(f3, kt + 7);
    }
    mm_diag<0>(f0, lo);
    load(f0, kd + 4);
    mm_diag<1>(f1, lo);
    load(f1, kd + 5);
    mm_diag<2>(f2, lo);
    load(f2, kd + 6);
    mm_diag<3>(f3, lo);
    load(f3, kd + 7);
    mm_diag<4>(f0, lo);
    mm_diag<5>(f1, lo);
    mm_diag<6>(f2, lo);
    mm_diag<7>(f3, lo);
  }
};

// Column sums of squares of a 128 x TN tile's accumulators (MfmaTile<128, TN> layout, WN = TN / 32 column blocks per
// wave) and their store: over the wave's rows (lane-sequential over i, r), then over the lanes holding the same column,
// then the two waves of each column half through LDS.  One code for both shapes: a column's partial does not depend on
// the tile's width.  slot0: the tile's first slot; STAGED: slot -> chunk column through list / col0, padding skipped.
template <int TN, bool STAGED>
__device__ __forceinline__ void trmm_colsum_store(const d4 (&acc)[4][TN / 32], int I, int64_t C, int64_t slot0,
                                                  const int2* list, int col0, double* __restrict__ ss_part,
                                                  double* red) {
  using L = MfmaTile<TT, TN, 16, true, true>;
  static_assert(L::WM == 4, "128 rows");
  double s[L::WN];
#pragma unroll
  for (int j = 0; j < L::WN; ++j) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < L::WM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v += acc[i][j][r] * acc[i][j][r];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    s[j] = v;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if ((w >> 1) == 1 && lane < 16) {
#pragma unroll
    for (int j = 0; j < L::WN; ++j) red[L::col_of(j)] = s[j];
  }
  __syncthreads();
  if ((w >> 1) == 0 && lane < 16) {
#pragma unroll
    for (int j = 0; j < L::WN; ++j) {
      const int col = L::col_of(j);
      if constexpr (STAGED) {
        const int slot = (int)slot0 + col;
        const int c = list ? list[slot].x : col0 + slot;  // -1: a padding column of the last compact tile
        if (c >= 0) ss_part[(int64_t)I * C + c] = s[j] + red[col];
      } else {
        ss_part[(int64_t)I * C + slot0 + col] = s[j] + red[col];
      }
    }
  }
}

// kfull = 0: W upper triangular (k < (I+1)*128); kfull = 1: W is a full npad x npad matrix (the SVGP's
// W2 = L^{-T} S term, gpx_svgp.hip), k over all nI row tiles.
// With W2 (the SVGP's second product, grid.y = 2): blockIdx.y = 0 runs W2 with kfull = 1 into ss2 (the heavier,
// full-k tiles dispatched first), blockIdx.y = 1 the product given by (W, ss_part, kfull): both products of a chunk in
// one launch share its K* and one launch tail (two launches before).
// STAGED (a stage of the pruned sweep): row tiles st.I0 .. st.I0 + st.nrows - 1 of the columns active in
// *st.desc.  The grid covers every candidate tile the chunk could still have; workgroups beyond the active tiles
// return at once.  Same tile, same order (heaviest row tile first, XCD-aware) and, for a column, the same MFMA chain
// whatever slot of whatever buffer it sits in; its sums go to ss_part at the column's place in the chunk, so the
// partials of a candidate are the ones the plain product writes.
// SHAPE: TRMM_WIDE the hand-placed 128 x 128 tile; TRMM_NARROW the narrow one over 4 ncb column tiles (ncb counts wide
// tiles in every shape); TRMM_DUAL (staged) the workgroups read the stage's tile count and take the narrow shape when
// the wide one would leave CUs without a tile (ncb * nrows < st.narrow_below), each tile as four workgroups.
enum { TRMM_WIDE = 0, TRMM_NARROW = 1, TRMM_DUAL = 2 };
template <bool STAGED, int SHAPE>
__device__ __forceinline__ void trmm_sumsq_body(const double* __restrict__ W, int64_t ldw,
                                                const double* __restrict__ kstar, int64_t C, int nI, int ncb,
                                                double* __restrict__ ss_part, int kfull,
                                                const double* __restrict__ W2, double* __restrict__ ss2,
                                                PruneStage st, double* smem) {
  if (W2 && blockIdx.y == 0) {
    W = W2;
    ss_part = ss2;
    kfull = 1;
  }
  int I0 = 0, nrows = nI, col0 = 0;
  int64_t ldb = C;
  const int2* list = nullptr;
  bool narrow = SHAPE == TRMM_NARROW;
  if constexpr (STAGED) {
    // (the tile's buffer descriptors want base and pitch in scalar registers: make the uniformity explicit)
    const int buf = __builtin_amdgcn_readfirstlane(st.desc->buf);
    const int li = __builtin_amdgcn_readfirstlane(st.desc->list);
    col0 = __builtin_amdgcn_readfirstlane(st.desc->col0);
    ncb = __builtin_amdgcn_readfirstlane(st.desc->ntiles);
    I0 = st.I0;
    nrows = st.nrows;
    if constexpr (SHAPE == TRMM_DUAL) narrow = ncb * nrows < st.narrow_below;
    if ((int)blockIdx.x >= (narrow ? 4 : 1) * ncb * nrows) return;
    kstar = buf == 0 ? st.pb.kstar : buf == 1 ? st.pb.c1 : st.pb.c2;
    ldb = buf == 0 ? st.pb.ld0 : buf == 1 ? st.pb.ld1 : st.pb.ld2;
    list = li < 0 ? nullptr : li == 2 ? st.pb.list2 : li ? st.pb.list1 : st.pb.list0;
  }
  int l, cb;
  if (SHAPE != TRMM_WIDE && narrow) {
    trmm_tile_order(blockIdx.x, nrows, 4 * ncb, l, cb);
    const int I = I0 + nrows - 1 - l;
    TrmmNarrow tile;
    tile.run(W + (int64_t)I * TT, ldw, kstar + col0 + (int64_t)cb * TNW, ldb, (I + 1) * (TT / 16));  // (kfull = 0 only)
    trmm_colsum_store<TNW, STAGED>(tile.acc, I, C, (int64_t)cb * TNW, list, col0, ss_part, smem);
    return;
  }
  if constexpr (SHAPE != TRMM_NARROW) {
    trmm_tile_order(blockIdx.x, nrows, ncb, l, cb);
    const int I = I0 + nrows - 1 - l;
    const double* Ab = W + (int64_t)I * TT;               // A(m=i,k) = W[k][I*128 + i]
    const double* Bb = kstar + col0 + (int64_t)cb * TT;   // B(k,n=c) = K*[k][col0 + cb*128 + c]
    // the k loop with a hand-placed instruction stream (gpx_trmm_asm.h; same MFMA sequence per accumulator as
    // MfmaTile::run, so the same bits); for the triangular W every wave skips the zero 16 x 16 blocks of the diagonal
    // 128-tile (trmm_asm::TileT::run_tri)
    trmm_asm::TileTag<SHAPE == TRMM_DUAL ? 2 : STAGED ? 1 : 0> tile;  // (a tag per kernel: gpx_trmm_asm.h TileT)
    tile.run(Ab, ldw, Bb, ldb, (kfull ? nI : I + 1) * (TT / 16), smem, !kfull);
    // (smem is free after run())
    trmm_colsum_store<TT, STAGED>(tile.acc, I, C, (int64_t)cb * TT, list, col0, ss_part, smem);
  }
}

__global__ void __launch_bounds__(WG)
trmm_sumsq_kernel(const double* __restrict__ W, int64_t ldw, const double* __restrict__ kstar, int64_t C, int nI,
                  int ncb, double* __restrict__ ss_part, int kfull, const double* __restrict__ W2 = nullptr,
                  double* __restrict__ ss2 = nullptr) {
  __shared__ __attribute__((aligned(16))) double smem[TrmmTile::LDS_DOUBLES];
  trmm_sumsq_body<false, TRMM_WIDE>(W, ldw, kstar, C, nI, ncb, ss_part, kfull, W2, ss2, PruneStage{}, smem);
}
// the plain product on narrow tiles (4 ncb * nI workgroups): the seed block, whose 8 wide column tiles leave the launch
// as long as its deepest row tile
__global__ void __launch_bounds__(WG, 2)
trmm_sumsq_narrow_kernel(const double* __restrict__ W, int64_t ldw, const double* __restrict__ kstar, int64_t C, int nI,
                         int ncb, double* __restrict__ ss_part) {
  __shared__ double red[TNW];
  trmm_sumsq_body<false, TRMM_NARROW>(W, ldw, kstar, C, nI, ncb, ss_part, 0, nullptr, nullptr, PruneStage{}, red);
}
// a stage on wide tiles: the first stage of a chunk or super-chunk, never sparse
__global__ void __launch_bounds__(WG)
trmm_stage_kernel(const double* __restrict__ W, int64_t ldw, int64_t C, int nI, double* __restrict__ ss_part,
                  PruneStage st) {
  __shared__ __attribute__((aligned(16))) double smem[TrmmTile::LDS_DOUBLES];
  trmm_sumsq_body<true, TRMM_WIDE>(W, ldw, nullptr, C, nI, 0, ss_part, 0, nullptr, nullptr, st, smem);
}
// a later stage: either shape, chosen by its workgroups from the stage's tile count (launch_tail_stage)
__global__ void __launch_bounds__(WG, 2)
trmm_stage_dual_kernel(const double* __restrict__ W, int64_t ldw, int64_t C, int nI, double* __restrict__ ss_part,
                       PruneStage st) {
  __shared__ __attribute__((aligned(16))) double smem[TrmmTile::LDS_DOUBLES];
  trmm_sumsq_body<true, TRMM_DUAL>(W, ldw, nullptr, C, nI, 0, ss_part, 0, nullptr, nullptr, st, smem);
}
// one shape by name, for gpx_debug_stage_product_f64
__global__ void __launch_bounds__(WG, 2)
trmm_stage_narrow_kernel(const double* __restrict__ W, int64_t ldw, int64_t C, int nI, double* __restrict__ ss_part,
                         PruneStage st) {
  __shared__ double red[TNW];
  trmm_sumsq_body<true, TRMM_NARROW>(W, ldw, nullptr, C, nI, 0, ss_part, 0, nullptr, nullptr, st, red);
}

// ---- the head of the lazy pruned sweep: K* rows 0 .. 127 and row tile 0 of the product in one kernel -----------------
// The head needs, of every candidate, the mean partials of row blocks 0 and 1 and |W11^T k*[0..127]|^2; K* itself is
// read by nothing else (the gathers rebuild their columns at full height).  So the K* entries never leave the registers:
// a wave owns 32 candidates (two 16-column blocks) and all eight 16-row blocks of the tile, walks the two row blocks
// jb = 0, 1 of K* with kstar_mfma_unit's arithmetic (the block's own centre, the cross term on the MFMA,
// sqdist_expanded, cov_from_r2, zero for rows >= n, the mean partials' fma order and lane reduction), and after
// cov_from_r2 its kv[r][cb] of lane (kq, m) = K*[k0 + kq][16 cb + m], k0 = 64 jb + rs + 4 r, is the B fragment of
// v_mfma_f64_16x16x4 for that k-step as it stands: acc[ib][cb] += W[k0 + kq][16 ib + m] * kv[r][cb] for the row blocks
// ib >= k0 / 16 and only those (run_tri's rule: row block ib is skipped for every k-tile J > ib, the diagonal 16 x 16
// block runs in full).  Every accumulator block's chain is k ascending in steps of 4 from zero, the chain of the wide
// and the narrow tile, so the bits are theirs, NaN and infinite candidates included.  The column sums of squares
// reproduce trmm_colsum_store<128>: rows 0-63 and 64-127 apart (the tile's two wave rows), each i outer, r inner over
// the lane's rows, + xor-16, + xor-32, then low + high.
// The A fragments come from L2 (W11's 36 nonzero blocks are 72 KB, read alike by every workgroup), one k-tile's at a
// time and before the tile's covariance arithmetic, which covers their latency.  The workgroups are persistent: they
// stride over the groups of 128 candidates, and the training rows' part of the setup (scaled rows, centres, norms,
// alpha, for both row blocks) is done once per workgroup.  One instruction stream: the k-tile loop is not unrolled, the
// row-block skip is a uniform branch on its counter.
// ss goes to ss_part[c] (row tile 0) for the staged columns c0s <= c < c1s only, mu_part blocks 0 and 1 for every
// column of the grid's groups, as the two launches this replaces wrote them.
// The list-driven instance (list != nullptr; the mean-first order's head over the columns its first prune pass kept,
// DESIGN §3): group g takes the columns list[128 g .. 128 g + 127].x, slots at or past *count are padding (zeros loaded,
// nothing stored), the workgroups stride over the ceil(*count / 128) live groups, and both outputs go to the column's
// own place.  Only the candidate loads' and the stores' addresses differ from the contiguous instance, so a column has
// the same bits in either.  Workgroup 0 then writes the list's descriptor for the bound pass behind it (desc_out: list
// 2, *count slots) and adds the groups to the product tiles run (stats[1]).
constexpr int HP_COLS = 128;  // candidates per workgroup trip
template <int DMAX, int KIND>
__global__ void __launch_bounds__(WG, 2)
head_product_kernel(gpx_kernel_params p, int n, const double* __restrict__ X, int64_t ldx,
                    const double* __restrict__ alpha, const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                    int64_t C, const double* __restrict__ W, int64_t ldw, int ngroups, int64_t c0s, int64_t c1s,
                    double* __restrict__ mu_part, double* __restrict__ ss_part, const int2* __restrict__ list,
                    const int* __restrict__ count, PruneDesc* __restrict__ desc_out, int64_t* __restrict__ stats) {
  int cnt = 0;
  if (list) {
    cnt = *count;
    ngroups = (cnt + HP_COLS - 1) / HP_COLS;
    if (desc_out && blockIdx.x == 0 && threadIdx.x == 0) {
      PruneDesc o;
      o.buf = 0;
      o.col0 = 0;
      o.ncols = cnt;
      o.ntiles = ngroups;
      o.list = 2;
      o.pad[0] = o.pad[1] = o.pad[2] = 0;
      *desc_out = o;
    }
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[1] += ngroups;
  }
  if ((int)blockIdx.x >= ngroups) return;  // (a short list: the launch costs its grid)
  constexpr bool lin = (KIND == GPX_KERNEL_SCALE_LINEAR_MATERN52);
  constexpr int KS = DMAX / 4;
  constexpr int NJB = PRUNE_HEAD_ROWS / NB;
  static_assert(NJB == 2 && PRUNE_HEAD_ROWS == TT, "two row blocks, one row tile");
  __shared__ double sa[NJB][NB][DMAX + 1], ra[lin ? NJB : 1][lin ? NB : 1][DMAX + 1];
  __shared__ double sb[HP_COLS][DMAX + 1], rb[lin ? HP_COLS : 1][DMAX + 1];
  __shared__ double na[NJB][NB], sal[NJB][NB], nb[HP_COLS], cen[NJB][DMAX];
  const int t = threadIdx.x, d = p.d;
  // the training rows' side, once per workgroup
  for (int e = t; e < NJB * NB * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;  // r: row 0 .. 127
    const double v = (k < d && r < n) ? X[(int64_t)r * ldx + k] : 0.0;
    sa[r / NB][r % NB][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
    if constexpr (lin) ra[r / NB][r % NB][k] = (k < d) ? v * p.linear_variance[k] : 0.0;
  }
  if (t < NJB * NB) sal[t / NB][t % NB] = t < n ? alpha[t] : 0.0;
  __syncthreads();
  if (t < NJB * DMAX) {
    const int jb = t / DMAX, k = t % DMAX;
    const int nv = n - jb * NB < NB ? n - jb * NB : NB;
    double s = 0.0;
    for (int r = 0; r < nv; ++r) s += sa[jb][r][k];
    cen[jb][k] = nv > 0 ? s / nv : 0.0;
  }
  __syncthreads();
  for (int e = t; e < NJB * NB * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    sa[r / NB][r % NB][k] -= cen[r / NB][k];
  }
  __syncthreads();
  if (t < NJB * NB) {
    double u = 0.0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) u = fma(sa[t / NB][t % NB][k], sa[t / NB][t % NB][k], u);
    na[t / NB][t % NB] = u;
  }
#pragma unroll 1
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t c0 = (int64_t)g * HP_COLS;
    d4 acc[8][2];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) acc[ib][cb] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int jb = 0; jb < NJB; ++jb) {
      const int nv = n - jb * NB < NB ? n - jb * NB : NB;  // valid training rows of the block (<= 0: all padding)
      // (an opaque thread index per trip keeps the compiler from hoisting every address that depends on it out of the
      // loops, which spilled them: the accumulators leave no room for loop invariants)
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      int lane = t & 63;
      const int w = t >> 6;
      __syncthreads();  // the row block before this one has read sb / nb to the end (and na is written)
      for (int e = t; e < HP_COLS * DMAX; e += WG) {
        const int r = e / DMAX, k = e % DMAX;
        int64_t col = c0 + r < m_chunk ? c0 + r : -1;
        if (list) col = c0 + r < cnt ? list[c0 + r].x : -1;
        const double v = (k < d && col >= 0) ? Xs[col * ldxs + k] : 0.0;
        const double s = (k < d) ? v / p.lengthscale[k] : 0.0;
        sb[r][k] = s - cen[jb][k];
        if constexpr (lin) rb[r][k] = v;
      }
      __syncthreads();
      if (t < HP_COLS) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) v = fma(sb[t][k], sb[t][k], v);
        nb[t] = v;
      }
      __syncthreads();
      double mu[2] = {0.0, 0.0}, nbc[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) nbc[cb] = nb[32 * w + 16 * cb + (lane & 15)];
#pragma unroll 1
      for (int rs = 0; rs < NB; rs += 16) {
        const int J = (jb * NB + rs) / 16;  // the k-tile: row blocks ib < J of W are zero in it
        asm volatile("" : "+v"(lane));       // (per k-tile too: the scaled-linear kind's four LDS images)
        const int m = lane & 15, kq = lane >> 4;
        // the tile's A fragments W[16 J + 4 r + kq][16 ib + m], one k-step's at a time and one k-step ahead: the first
        // before the covariance arithmetic, which covers its latency, the others behind the MFMAs of the step before
        double a[2][8];
        const double* Wj = W + (int64_t)(16 * J + kq) * ldw + m;  // W[16 J + kq][m]
        auto load_a = [&](double(&f)[8], int r) {
#pragma unroll
          for (int ib = 0; ib < 8; ++ib) f[ib] = ib >= J ? Wj[(int64_t)(4 * r) * ldw + 16 * ib] : 0.0;
        };
        load_a(a[0], 0);
        double kv[4][2];  // [r][cb]: row rs + kq + 4 r of the block, candidate 32 w + 16 cb + m
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          d4 dot = {0.0, 0.0, 0.0, 0.0}, lac = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < KS; ++k) {
            dot = mfma16x16x4(sa[jb][rs + m][4 * k + kq], sb[32 * w + 16 * cb + m][4 * k + kq], dot);
            if constexpr (lin)
              lac = mfma16x16x4(ra[jb][rs + m][4 * k + kq], rb[32 * w + 16 * cb + m][4 * k + kq], lac);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = rs + kq + 4 * r;
            double v =
                cov_from_r2(KIND, p.outputscale, sqdist_expanded(na[jb][j], nbc[cb], dot[r]), lin ? lac[r] : 0.0);
            v = j < nv ? v : 0.0;
            kv[r][cb] = v;
            mu[cb] = fma(sal[jb][j], v, mu[cb]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r < 3) load_a(a[(r + 1) & 1], r + 1);
#pragma unroll
          for (int ib = 0; ib < 8; ++ib)
            if (ib >= J) {
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) acc[ib][cb] = mfma16x16x4(a[r & 1][ib], kv[r][cb], acc[ib][cb]);
            }
        }
      }
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        double v = mu[cb];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        int64_t col = c0 + 32 * w + 16 * cb + lane;
        bool live = lane < 16;
        if (list) {
          live = live && col < cnt;
          col = live ? list[col].x : 0;
        }
        if (live) mu_part[(int64_t)jb * C + col] = v;
      }
    }
    // trmm_colsum_store<128>'s sums: the tile's two wave rows apart, then low + high
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      double s[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) v += acc[4 * h + i][cb][r] * acc[4 * h + i][cb][r];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        s[h] = v;
      }
      int64_t c = c0 + 32 * w + 16 * cb + m;
      bool live = kq == 0 && c >= c0s && c < c1s;
      if (list) {
        live = kq == 0 && c < cnt;
        c = live ? list[c].x : 0;
      }
      if (live) ss_part[c] = s[0] + s[1];
    }
  }
}

// ---- 1+2 fused, small n (npad <= 256) ----------------------------------------------------------
// At small n the K* round trip through HBM and the 128-row trmm tiles (whose triangle is at most two tiles deep)
// cost more than the product (profiles/r01_small_n_rates.log, n = 256: kstar 2.2 + trmm 6.4 ms per 2^22 candidates
// at 43 TF/s).  Here one wave owns 16 candidates and walks k in steps of 4: each lane evaluates K*[k][c]
// (k = k0 + lane/16, c = lane%16) straight into the B operand of v_mfma_f64_16x16x4 (no K* buffer), and the A
// operands W[k][16 ib + lane%16] of the row blocks ib >= k/16 come from L2 (W is npad^2 fp64 <= 512 KiB, shared by
// every workgroup).  The triangle is walked in 16-row blocks, so the diagonal waste is 1/16 instead of 1/2 of a
// 128-row tile.  Outputs per candidate: mu (alpha^T K* per output, no constant mean) and ss = |W^T K*|^2, in the
// layout of one mu_part / ss_part block so finalize_kernel runs unchanged with nJB = nI = 1.  The summation order differs from the
// unfused path (both are checked against the oracle at the same tolerance).
// NR = 1 (acquisition, single-output posterior) or GPX_MAX_RHS (multi-output posterior, alpha zero-padded to 8 columns
// so the mean loop has no nrhs test; mu_out[q][c] for q < nrhs).
template <int NPAD, int DMAX, int KIND, int NR>
__global__ void __launch_bounds__(WG) sweep_small_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                         int64_t ldx, const double* __restrict__ alpha, int nrhs,
                                                         const double* __restrict__ W, int64_t ldw,
                                                         const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                         int64_t C, double* __restrict__ mu_out,
                                                         double* __restrict__ ss_out) {
  constexpr int NRB = NPAD / 16;
  constexpr int KS = DMAX / 4;
  constexpr bool LIN = KIND == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  // XT: the distance's cross term on MFMA (gram_mfma_kernel's arithmetic, centred by the mean of the training inputs):
  // 1.745e9 / 1.784e9 vs 1.651e9 / 1.698e9 candidates/s at n = 64 / 128, but 4.60e8 vs 5.81e8 at n = 256, where the
  // dot operands beside 16 accumulator blocks cost occupancy (tools/small_n_rates.py, profiles/r04_small_n_xterm_ab.log);
  // npad = 256 keeps the difference form.
  constexpr bool XT = NPAD <= 128;
  __shared__ double sx[NPAD][DMAX + 1], sr[LIN ? NPAD : 1][DMAX + 1], sa[NPAD][NR], sn[XT ? NPAD : 1], cen[DMAX];
  const int d = p.d, t = threadIdx.x;
  for (int e = t; e < NPAD * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    const double v = (k < d && r < n) ? X[(int64_t)r * ldx + k] : 0.0;
    sx[r][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
    if constexpr (LIN) sr[r][k] = (k < d) ? v * p.linear_variance[k] : 0.0;
  }
  for (int e = t; e < NPAD * NR; e += WG) {
    const int r = e / NR, q = e % NR;
    sa[r][q] = (r < n && q < nrhs) ? alpha[(int64_t)r * nrhs + q] : 0.0;
  }
  __syncthreads();
  if constexpr (XT) {
    if (t < DMAX) {
      double s = 0.0;
      for (int r = 0; r < n; ++r) s += sx[r][t];
      cen[t] = n > 0 ? s / n : 0.0;
    }
    __syncthreads();
    for (int e = t; e < NPAD * DMAX; e += WG) sx[e / DMAX][e % DMAX] -= cen[e % DMAX];
    __syncthreads();
    for (int r = t; r < NPAD; r += WG) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) v = fma(sx[r][k], sx[r][k], v);
      sn[r] = v;
    }
    __syncthreads();
  }
  const int lane = t & 63, w = t >> 6;
  const int kr = lane >> 4, m = lane & 15;
  const int64_t c = ((int64_t)blockIdx.x * (WG / 64) + w) * 16 + m;
  const bool valid = c < m_chunk;
  // XT: this lane's B operands of the dot (candidate m, dimensions 4 s + kr) and the candidate's squared norm; else the
  // candidate's whole point (difference form, one K* element per lane and k-step)
  double bo[XT ? KS : 1], br[XT ? KS : 1], nb = 0.0;
  double xs[XT ? 1 : DMAX], xr[XT ? 1 : DMAX];
  if constexpr (XT) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + kr;
      const double v = (valid && k < d) ? Xs[c * ldxs + k] : 0.0;
      bo[s] = (k < d) ? v / p.lengthscale[k] - cen[k] : 0.0;
      br[s] = v;
      nb = fma(bo[s], bo[s], nb);
    }
    nb += __shfl_xor(nb, 16);
    nb += __shfl_xor(nb, 32);
  } else {
    load_point<DMAX>(p, Xs + (valid ? c * ldxs : 0), valid, xs, xr);
  }
  d4 acc[NRB];
#pragma unroll
  for (int ib = 0; ib < NRB; ++ib) acc[ib] = (d4){0.0, 0.0, 0.0, 0.0};
  double mu[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) mu[q] = 0.0;
  const double* __restrict__ Wl = W + (int64_t)kr * ldw + (lane & 15);
#pragma unroll
  for (int kb = 0; kb < NRB; ++kb) {
    // XT: a.b for the 16 rows of block kb x the wave's 16 candidates; register r of the accumulator holds row
    // 16 kb + kr + 4 r of candidate m, i.e. exactly the B operand of k-step r below
    d4 dot = {0.0, 0.0, 0.0, 0.0}, lac = {0.0, 0.0, 0.0, 0.0};
    if constexpr (XT) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        dot = mfma16x16x4(sx[16 * kb + m][4 * s + kr], bo[s], dot);
        if constexpr (LIN) lac = mfma16x16x4(sr[16 * kb + m][4 * s + kr], br[s], lac);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k0 = 16 * kb + 4 * ks;
      const int j = k0 + kr;
      double kv;
      if constexpr (XT) {
        kv = cov_from_r2(KIND, p.outputscale, sqdist_expanded(sn[j], nb, dot[ks]), LIN ? lac[ks] : 0.0);
      } else {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          const double df = sx[j][k] - xs[k];
          r2 += df * df;
        }
        double lv = 0.0;
        if constexpr (LIN) {
#pragma unroll
          for (int k = 0; k < DMAX; ++k) lv += sr[j][k] * xr[k];
        }
        kv = cov_from_r2(KIND, p.outputscale, r2, lv);
      }
      kv = j < n ? kv : 0.0;
#pragma unroll
      for (int q = 0; q < NR; ++q) mu[q] += sa[j][q] * kv;
#pragma unroll
      for (int ib = kb; ib < NRB; ++ib) acc[ib] = mfma16x16x4(Wl[(int64_t)k0 * ldw + 16 * ib], kv, acc[ib]);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int ib = 0; ib < NRB; ++ib)
#pragma unroll
    for (int r = 0; r < 4; ++r) s += acc[ib][r] * acc[ib][r];
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    mu[q] += __shfl_xor(mu[q], 16);
    mu[q] += __shfl_xor(mu[q], 32);
  }
  if (lane < 16 && valid) {
#pragma unroll
    for (int q = 0; q < NR; ++q)
      if (q < nrhs) mu_out[(int64_t)q * C + c] = mu[q];
    ss_out[c] = s;
  }
}

// ---- 3. finalize: the passes over a chunk's columns and the pieces they share --------------------------------------
// The model and the objective of a finalize pass.
struct FinalizeArgs {
  gpx_kernel_params p;
  double y_mean[GPX_MAX_RHS];
  double y_scale[GPX_MAX_RHS];
  int acq_kind;
  double best_f, beta;
  // a linear objective sum_t w_t f_t over T independent GPs (gpx_acquire_argmax_multi_f64)
  double weight;     // FIN_ACCUMULATE: w_t of this output
  int first;         // FIN_ACCUMULATE: the first output of the chunk (overwrites the accumulators)
  double* acc_mu;    // sum_t w_t (y_mean_t + y_scale_t mu_t)                 (chunk-sized)
  double* acc_var;   // sum_t w_t^2 y_scale_t^2 max(k** - |v_t|^2, 1e-10)      (chunk-sized)
};

// What a pass reads and writes, one group per concern; a launch site sets the groups its pass has (launch_finalize).
struct Partials {  // the chunk's partial sums: mu_part[(jb * nrhs + q) * C + c], ss_part[I * C + c]
  const double* mu_part;
  const double* ss_part;
  int64_t C;
  int nJB, nI, nrhs;  // (a bound pass: nI row tiles done so far)
};
// The pruned sweep's active column set (desc = nullptr: thread t is chunk column t < q.m): thread t is slot t of *desc.
// A bound pass appends its survivors to the list that *desc does not use.
struct ColumnSet {
  const PruneDesc* desc;
  int2* list0;
  int2* list1;
  const int2* list2;  // read only (PruneDesc::list = 2); its survivors go to list0
};
struct PosteriorOut {  // FIN_POSTERIOR
  double* mean;
  int64_t ldmean;
  double* var;
};
struct ScoreOut {  // the score passes: one (value, index) record per workgroup
  double* rec_val;
  int64_t* rec_idx;
  double* scores;           // optional: every column's score
  unsigned long long* tau;  // optional: the incumbent, raised to the workgroup's best score (the argmax form)
  // the top-k form (gpx_acquire_topk_f64; null everywhere else): every valid candidate's (score, global index) is
  // appended to the scored list and the incumbent left alone (tau = nullptr): topk_pool_kernel sets it
  double* sc_val;
  int64_t* sc_idx;
  int* sc_count;
};
struct BoundSel {  // the bound passes
  int* count;                     // survivors appended so far
  const unsigned long long* tau;  // the incumbent's key
  const double* mu_bound;  // the lazy head's pass: mu_approx at [c], mu_slack at [C + c] (mu_bound_kernel) stand in for
                           // the mean partials
  double* u_out;  // no incumbent yet (the seeded order's bound pass): the bound of column c goes to u_out[c], nothing
                  // is selected; seed_select_kernel and seed_prune_kernel read it
};
struct FinalizeIo {
  SweepCands q;  // the candidates: index_offset + c is column c's global index
  Partials part;
  ColumnSet cols;
  PosteriorOut post;
  ScoreOut score;
  BoundSel bound;
};

// Prior variance k(x, x) of column c.
__device__ __forceinline__ double prior_variance(const gpx_kernel_params& p, const double* __restrict__ Xs,
                                                 int64_t ldxs, int64_t c) {
  if (p.kind != GPX_KERNEL_SCALE_LINEAR_MATERN52) return p.outputscale;
  double lv = 0.0;
  for (int k = 0; k < p.d; ++k) {
    const double v = Xs[c * ldxs + k];
    lv += v * v * p.linear_variance[k];
  }
  return p.outputscale * (lv + 1.0);
}

// The bound test of the pruned sweep: a candidate whose score bound is `score` survives unless the bound lies below the
// incumbent by more than the margin of acq_score's rounding.  A NaN bound survives.
constexpr double PRUNE_EPS = 1e-9;
__device__ __forceinline__ bool bound_keeps(double score, double tau) {
  return !(score + PRUNE_EPS * (fabs(score) + fabs(tau) + 1.0) < tau);
}

// A compact list fed by whole waves: the slot of a lane with `pred` (other lanes: no meaning).  One ballot and one
// atomic add per wave, none for a wave without such a lane; the slot order may vary from run to run, no result depends
// on it.
__device__ __forceinline__ int wave_append(bool pred, int* __restrict__ count) {
  const unsigned long long mask = __ballot(pred);
  if (mask == 0) return 0;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(mask));
  base = __shfl(base, 0);
  return base + __popcll(mask & ((1ull << lane) - 1));
}

// The argmax of a 256-thread workgroup's (bv, bi) pairs, on thread 0 (argmax_merge: max value, then lowest index).  One
// __syncthreads, which every thread of the workgroup must reach.
__device__ __forceinline__ void block_argmax(double& bv, int64_t& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(bv, o);
    const int64_t i2 = __shfl_xor(bi, o);
    argmax_merge(bv, bi, v2, i2);
  }
  __shared__ double wv[4];
  __shared__ int64_t wi[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    wv[w] = bv;
    wi[w] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < 4; ++q) argmax_merge(bv, bi, wv[q], wi[q]);
}

// One output's standardised moments at column c into the objective's accumulators: untransform, weight, overwrite (the
// chunk's first output) or add.
__device__ __forceinline__ void accumulate_output(double* acc_mu, double* acc_var, int64_t c, int first, double weight,
                                                  double y_mean, double y_scale, double mu, double var) {
  mu = y_mean + y_scale * mu;
  var = var * (y_scale * y_scale);
  const double wm = weight * mu, wv = (weight * weight) * var;
  acc_mu[c] = first ? wm : acc_mu[c] + wm;
  acc_var[c] = first ? wv : acc_var[c] + wv;
}

// The accumulated objective's moments at column c (what FIN_ACCUMULATE summed over the outputs), BoTorch's floor on the
// scored variance.
__device__ __forceinline__ void objective_moments(const FinalizeArgs& fa, int64_t c, double& mu, double& var) {
  mu = fa.acc_mu[c];
  var = fmax(fa.acc_var[c], 1e-12);
}

// The passes.  Two end early: the posterior (mean / variance out) and one output of a multi-output objective into the
// accumulators.  The others are a source of moments, the chunk's partials or the accumulators, crossed with a sink:
//  score  acquisition, optional scores_out and scored list, 256-candidate block argmax record, incumbent raised.  A NaN
//         score counts as -inf for the record and the list and stays NaN in scores_out.
//  bound  of the pruned sweep: the score from the first nI row tiles' partials only (the accumulators: from every
//         output's first tile) is an upper bound of the candidate's score (the variance can only shrink with further
//         tiles, and every acquisition grows with it); the candidate survives if bound_keeps, or without an incumbent
//         the bound itself is kept (u_out).
// Variance floors: GPyTorch's 1e-10 per output in the standardised space, BoTorch's 1e-12 on the scored variance
// [upstream] (T = 1, w = 1: FIN_ACCUMULATE + FIN_SCORE_ACC give FIN_SCORE's value bit for bit).
enum FinalizePass { FIN_POSTERIOR, FIN_ACCUMULATE, FIN_SCORE, FIN_SCORE_ACC, FIN_BOUND, FIN_BOUND_ACC };

template <FinalizePass PASS>
__global__ void __launch_bounds__(WG) finalize_kernel(FinalizeArgs fa, FinalizeIo io) {
  constexpr bool BOUND = PASS == FIN_BOUND || PASS == FIN_BOUND_ACC;
  constexpr bool FROM_ACC = PASS == FIN_SCORE_ACC || PASS == FIN_BOUND_ACC;
  const gpx_kernel_params& p = fa.p;
  const Partials& pt = io.part;
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  int64_t c = t;
  bool valid = t < io.q.m;
  int2* survivors = nullptr;
  if (io.cols.desc) {
    const PruneDesc d = *io.cols.desc;
    if (BOUND && (int64_t)blockIdx.x * WG >= d.ncols) return;
    valid = t < d.ncols;
    c = !valid       ? 0
        : d.list < 0 ? d.col0 + t
                     : (d.list == 2 ? io.cols.list2 : d.list ? io.cols.list1 : io.cols.list0)[t].x;
    survivors = d.list == 0 ? io.cols.list1 : io.cols.list0;
  }
  double score = -INFINITY;
  if (valid) {
    double mu, var;
    if constexpr (FROM_ACC) {
      objective_moments(fa, c, mu, var);
    } else {
      const double ss = sum_partials(pt.ss_part + c, pt.nI, pt.C);
      var = fmax(prior_variance(p, io.q.Xs, io.q.ldxs, c) - ss, 1e-10);  // gpytorch min_variance (float64) [upstream]
      if constexpr (PASS == FIN_POSTERIOR) {
        for (int q = 0; q < pt.nrhs; ++q) {
          double mq = sum_partials(pt.mu_part + (int64_t)q * pt.C + c, pt.nJB, (int64_t)pt.nrhs * pt.C);
          mq += p.const_mean;
          io.post.mean[c * io.post.ldmean + q] = fa.y_mean[q] + fa.y_scale[q] * mq;
        }
        io.post.var[c] = fmax(var * (fa.y_scale[0] * fa.y_scale[0]), 1e-12);  // BoTorch min_var [upstream]
        return;
      }
      // (a bound pass with a mean bound: the score is non-decreasing in the mean too, so its upper end bounds it)
      mu = (BOUND && io.bound.mu_bound) ? io.bound.mu_bound[c] + io.bound.mu_bound[pt.C + c]
                                        : sum_partials(pt.mu_part + c, pt.nJB, pt.C);
      mu += p.const_mean;
      if constexpr (PASS == FIN_ACCUMULATE) {
        accumulate_output(fa.acc_mu, fa.acc_var, c, fa.first, fa.weight, fa.y_mean[0], fa.y_scale[0], mu, var);
        return;
      }
      mu = fa.y_mean[0] + fa.y_scale[0] * mu;
      var = fmax(var * (fa.y_scale[0] * fa.y_scale[0]), 1e-12);
    }
    score = acq_score(fa.acq_kind, mu, var, fa.best_f, fa.beta);
  }
  if constexpr (PASS == FIN_POSTERIOR || PASS == FIN_ACCUMULATE) {
    return;
  } else if constexpr (BOUND) {
    if (io.bound.u_out) {
      if (valid) io.bound.u_out[c] = score;
      return;
    }
    const bool keep = valid && bound_keeps(score, tau_value(*io.bound.tau));
    const int slot = wave_append(keep, io.bound.count);
    if (keep) survivors[slot] = make_int2((int)c, (int)t);
  } else {
    const ScoreOut& so = io.score;
    if (valid && so.scores) so.scores[c] = score;
    if (score != score) score = -INFINITY;
    if (so.sc_count) {
      // the top-k form's scored list; the value is gpx_topk_f64's key of the score (NaN is -inf already, -0 becomes +0)
      const int slot = wave_append(valid, so.sc_count);
      if (valid) {
        so.sc_val[slot] = score + 0.0;
        so.sc_idx[slot] = io.q.index_offset + c;
      }
    }
    double bv = score;
    int64_t bi = valid ? io.q.index_offset + c : INT64_MAX;
    block_argmax(bv, bi);
    if (threadIdx.x == 0) {
      so.rec_val[blockIdx.x] = bv;
      so.rec_idx[blockIdx.x] = bi;
      if (so.tau) atomicMax(so.tau, tau_key(bv));
    }
  }
}

// ---- the seeded order of the lazy form (launch_sweep_super_pruned) ---------------------------------------
// The span's m >= PRUNE_SEED columns in PRUNE_SEED contiguous slices: slice s is [s m / PRUNE_SEED, (s + 1) m /
// PRUNE_SEED), rounded down.  None is empty and none longer than ceil(m / PRUNE_SEED), so one column per slice is
// exactly PRUNE_SEED distinct columns in ascending order, whatever m.
__device__ __forceinline__ int64_t seed_slice_begin(int64_t s, int64_t m) { return s * m / PRUNE_SEED; }
__device__ __forceinline__ int seed_slice_of(int64_t c, int64_t m) { return (int)(((c + 1) * PRUNE_SEED - 1) / m); }

// The seed of a span: per slice (one workgroup each) the column with the largest score bound U, the lowest such column
// on ties; a NaN bound counts as -inf, so it wins only a slice without a larger one.  seed[s] = {column, s}; workgroup 0
// also writes the list's length where the gather build reads it.  Plain reductions in a fixed order: deterministic.
__global__ void __launch_bounds__(WG) seed_select_kernel(const double* __restrict__ U, int64_t m,
                                                         int2* __restrict__ seed, int* __restrict__ count) {
  const int s = blockIdx.x;
  const int64_t c1 = seed_slice_begin(s + 1, m);
  double bv = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int64_t c = seed_slice_begin(s, m) + threadIdx.x; c < c1; c += WG) {
    const double u = U[c];
    argmax_merge(bv, bi, u != u ? -INFINITY : u, c);
  }
  block_argmax(bv, bi);
  if (threadIdx.x == 0) {
    seed[s] = make_int2((int)bi, s);
    if (s == 0) *count = PRUNE_SEED;
  }
}

// The seeded order's prune pass: the bound test of the stored bounds U against the incumbent the seed left, the seed's
// own columns left out (they are scored already); survivors {column, column} to the list.
__global__ void __launch_bounds__(WG) seed_prune_kernel(const double* __restrict__ U, int64_t m,
                                                        const int2* __restrict__ seed,
                                                        const unsigned long long* __restrict__ tau_key_in,
                                                        int2* __restrict__ survivors, int* __restrict__ count) {
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  const bool valid = c < m && seed[seed_slice_of(c, m)].x != (int)c;
  const double score = valid ? U[c] : -INFINITY;
  const bool keep = valid && bound_keeps(score, tau_value(*tau_key_in));
  const int slot = wave_append(keep, count);
  if (keep) survivors[slot] = make_int2((int)c, (int)c);
}

// The pruned sweep's per-chunk reset (one thread): the first stage's column set (the chunk's columns from col0 on, in
// place), zero survivor counts, and on the call's first chunk the incumbent (-inf), the counters and, in the top-k form
// (tk_head), the scored list's and the pool's counts.  count2 (the mean-first order): one more count to zero.
__global__ void prune_init_kernel(PruneDesc* __restrict__ desc, int* __restrict__ count,
                                  unsigned long long* __restrict__ tau, int64_t* __restrict__ stats, int col0,
                                  int ncols, int rows0, int last, int first, int* __restrict__ tk_head,
                                  int* __restrict__ count2 = nullptr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (first && tk_head) tk_head[0] = tk_head[1] = 0;  // the top-k form: empty scored list, empty pool
  PruneDesc d;
  d.buf = 0;
  d.col0 = col0;
  d.ncols = ncols;
  d.ntiles = (ncols + TT - 1) / TT;
  d.list = -1;
  d.pad[0] = d.pad[1] = d.pad[2] = 0;
  desc[0] = d;
  for (int s = 0; s < PRUNE_MAX_STAGES; ++s) count[s] = 0;
  if (count2) *count2 = 0;
  if (first) {
    *tau = tau_key(-INFINITY);
    stats[0] = stats[1] = 0;
  }
  stats[1] += (int64_t)d.ntiles * rows0;
  if (last) stats[0] += ncols;
}

// After a stage's bound and select: the next stage's column set.  If the survivors are at most half of the active
// columns, their K* columns are gathered into the other compact buffer (dense 128-column tiles, the last one padded
// with zero columns whose list entry is -1), else the next stage keeps the buffer and the columns it has: the copy
// traffic stays below the K* it replaces, and an unprunable chunk pays only the bound passes.  Every workgroup takes
// the same decision from what earlier launches wrote; thread 0 of workgroup (0, 0) writes the next descriptor (read by
// later launches only) and the counters.  The grid is one-dimensional and bounded (tail_grid; at least a workgroup per
// 256 slots of the set's capacity), and the workgroups divide the live work among themselves: with nx blocks of 256
// slots to move, each block's npad rows are split evenly over gridDim.x / nx workgroups (down to min_rows rows each),
// so a small set is copied by as many workgroups as a large one and an empty launch costs its bounded grid.
__global__ void __launch_bounds__(WG) prune_compact_kernel(PruneBufs pb, const PruneDesc* __restrict__ din,
                                                           PruneDesc* __restrict__ dout,
                                                           const int* __restrict__ count, int npad, int min_rows,
                                                           int next_rows, int last, int64_t* __restrict__ stats) {
  const PruneDesc d = *din;
  const int surv = *count;
  const bool compact = 2 * (int64_t)surv <= d.ncols;
  const int ntl = (surv + TT - 1) / TT;
  const int out_list = d.list == 0 ? 1 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    PruneDesc o = d;
    if (compact) {
      o.buf = d.buf == 1 ? 2 : 1;
      o.col0 = 0;
      o.ncols = surv;
      o.ntiles = ntl;
      o.list = out_list;
    }
    *dout = o;
    stats[1] += (int64_t)o.ntiles * next_rows;
    if (last) stats[0] += o.ncols;
  }
  if (!compact || ntl == 0) return;
  int2* list = out_list ? pb.list1 : pb.list0;
  const double* src = d.buf == 0 ? pb.kstar : d.buf == 1 ? pb.c1 : pb.c2;
  const int64_t lds = d.buf == 0 ? pb.ld0 : d.buf == 1 ? pb.ld1 : pb.ld2;
  double* dst = d.buf == 1 ? pb.c2 : pb.c1;
  const int64_t ldd = d.buf == 1 ? pb.ld2 : pb.ld1;
  const int nx = (ntl * TT + WG - 1) / WG;
  int per = (int)gridDim.x / nx;  // workgroups per block of slots (the grid has one per block at least)
  per = per > npad / min_rows ? npad / min_rows : per;
  const int slot = ((int)blockIdx.x / per) * WG + threadIdx.x, y = (int)blockIdx.x % per;
  if (slot >= ntl * TT) return;
  const bool real = slot < surv;
  if (!real && y == 0) list[slot] = make_int2(-1, 0);
  const int64_t sc = real ? d.col0 + list[slot].y : 0;
  const int r1 = (int)((int64_t)(y + 1) * npad / per);
#pragma unroll 8
  for (int r = (int)((int64_t)y * npad / per); r < r1; ++r)
    dst[(int64_t)r * ldd + slot] = real ? src[(int64_t)r * lds + sc] : 0.0;
}

// records e = 0 .. count-1 at vals[e * stride] / idx[e * stride] (stride 1: separate arrays; 2: packed 16-byte
// (value, index) records of the cross-GPU exchange)
__global__ void __launch_bounds__(WG) argmax_final_kernel(const double* __restrict__ vals,
                                                          const int64_t* __restrict__ idx, int64_t count,
                                                          int stride, double* __restrict__ best_val,
                                                          int64_t* __restrict__ best_idx) {
  double bv = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int64_t e = threadIdx.x; e < count; e += WG) {
    double v = vals[e * stride];
    if (v != v) v = -INFINITY;
    argmax_merge(bv, bi, v, idx[e * stride]);
  }
  block_argmax(bv, bi);
  if (threadIdx.x == 0) {
    *best_val = bv;
    *best_idx = bi;
  }
}

// ---- the top-k form of the pruned sweep (gpx_acquire_topk_f64) ---------------------------------------
// The result's order: larger score first, equal scores -> lower index (gpx_topk_f64's stable descending sort of its
// keys; the list's values are those keys, so no NaN and no -0 gets here).  Indices are distinct, so the order is total
// and the k best of a set do not depend on the order its members arrive in.
__device__ __forceinline__ bool topk_before(double va, int64_t ia, double vb, int64_t ib) {
  return va > vb || (va == vb && ia < ib);
}
constexpr int TOPK_LDS = 2 * GPX_TOPK_SWEEP_MAX;  // entries of the merge buffer: the pool and as many new ones

// One workgroup, enqueued behind every launch that scores candidates in full (a score pass of finalize_kernel with a
// scored list): merges the list's n entries into the pool of the k best (score, index) pairs scored so far, empties the
// list and sets the incumbent of the bound passes that follow:
//     tau = the pool's k-th score once the pool holds k pairs, else -inf.
// Soundness.  tau is the k-th best of a subset of the call's exact scores, hence <= the k-th best of all of them.  The
// bound pass drops a candidate only if its bound ub >= its exact score lies below tau by more than bound_keeps' margin:
// a dropped candidate scores strictly below k candidates scored in full, so it is not among the call's k best and does
// not tie with the k-th; a candidate that ties the k-th place is always scored, and the lowest index wins it in the
// merge.  Every member of the final k best is therefore scored in full and passes through a merge: the pool at the end
// of the call is the answer.  With k = 1 tau takes the values the argmax form's atomicMax gives it.
// Entries that cannot enter a full pool (not before its k-th pair) are filtered by a ballot pass before anything is
// sorted: after the seed block that is almost all of them, so an unprunable round costs a read of its list.  What is
// left is appended behind the pool in LDS and merged by a bitonic sort over the next power of two (at most TOPK_LDS
// pairs, 32 KB), in batches when a launch produced more than the buffer takes.  No hand-off between workgroups: the
// launch boundaries of the stream order list, pool and incumbent.  An empty list returns at once.
__global__ void __launch_bounds__(WG) topk_pool_kernel(int k, int cap, int* __restrict__ head,
                                                       double* __restrict__ pool_val, int64_t* __restrict__ pool_idx,
                                                       const double* __restrict__ list_val,
                                                       const int64_t* __restrict__ list_idx,
                                                       unsigned long long* __restrict__ tau) {
  __shared__ double sv[TOPK_LDS];
  __shared__ int64_t si[TOPK_LDS];
  __shared__ int wcnt[WG / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int n = head[0];
  if (n <= 0) return;
  n = n < cap ? n : cap;
  int pn = head[1];
  pn = pn < 0 ? 0 : pn < k ? pn : k;
  for (int e = t; e < pn; e += WG) {
    sv[e] = pool_val[e];
    si[e] = pool_idx[e];
  }
  __syncthreads();
  int fill = 0;  // new entries behind the pool (uniform)
  bool merged = false;
  // pool + new entries -> sorted, the best min(k, all) of them the new pool
  auto merge = [&]() {
    const int total = pn + fill;
    int P = 2;
    while (P < total) P <<= 1;
    for (int e = total + t; e < P; e += WG) {
      sv[e] = -INFINITY;
      si[e] = INT64_MAX;  // behind every real pair
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int e = t; e < P / 2; e += WG) {
          const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
          const double vl = sv[lo], vh = sv[hi];
          const int64_t il = si[lo], ih = si[hi];
          const bool up = (lo & size) == 0;
          if (up ? topk_before(vh, ih, vl, il) : topk_before(vl, il, vh, ih)) {
            sv[lo] = vh, si[lo] = ih;
            sv[hi] = vl, si[hi] = il;
          }
        }
        __syncthreads();
      }
    pn = total < k ? total : k;
    fill = 0;
    merged = true;
  };
  for (int base = 0; base < n; base += WG) {
    const int e = base + t;
    bool take = e < n;
    double v = 0.0;
    int64_t i = 0;
    if (take) {
      v = list_val[e];
      i = list_idx[e];
      if (pn == k) take = topk_before(v, i, sv[k - 1], si[k - 1]);
    }
    const unsigned long long mask = __ballot(take);
    if (lane == 0) wcnt[w] = __popcll(mask);
    __syncthreads();
    int off = pn + fill, tot = 0;
    for (int q = 0; q < WG / 64; ++q) {
      if (q < w) off += wcnt[q];
      tot += wcnt[q];
    }
    if (take) {
      const int slot = off + __popcll(mask & ((1ull << lane) - 1));
      sv[slot] = v;
      si[slot] = i;
    }
    fill += tot;
    __syncthreads();
    if (pn + fill > TOPK_LDS - WG) merge();  // (the next pass could overflow the buffer)
  }
  if (fill) merge();
  if (merged) {
    for (int e = t; e < pn; e += WG) {
      pool_val[e] = sv[e];
      pool_idx[e] = si[e];
    }
  }
  if (t == 0) {
    head[0] = 0;
    if (merged) {
      head[1] = pn;
      *tau = tau_key(pn == k ? sv[k - 1] : -INFINITY);
    }
  }
}

__global__ void __launch_bounds__(WG) topk_result_kernel(int k, const int* __restrict__ head,
                                                         const double* __restrict__ pool_val,
                                                         const int64_t* __restrict__ pool_idx,
                                                         double* __restrict__ val_out, int64_t* __restrict__ idx_out) {
  const int e = blockIdx.x * WG + threadIdx.x;
  if (e >= k) return;
  // (the pool is full at the end of a call: k <= the seed block <= the candidates scored in full)
  const bool have = e < head[1];
  val_out[e] = have ? pool_val[e] : -INFINITY;
  idx_out[e] = have ? pool_idx[e] : INT64_MAX;
}

__global__ void __launch_bounds__(WG) index_shift_kernel(int64_t* __restrict__ idx, int64_t k, int64_t offset) {
  const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (e < k) idx[e] += offset;
}

// ---- host side -------------------------------------------------------------------------------------------
// The grid of a finalize pass: a workgroup per 256 of the io.q.m columns the launch can have.
template <FinalizePass PASS>
static void launch_finalize(Context* c, const FinalizeArgs& fa, const FinalizeIo& io) {
  finalize_kernel<PASS><<<(unsigned)((io.q.m + WG - 1) / WG), WG, 0, c->stream>>>(fa, io);
}
// The sink of a pruned sweep's score pass: the argmax form raises the incumbent itself, the top-k form feeds the scored
// list and leaves the incumbent to topk_pool_kernel
static ScoreOut pruned_score_out(double* rec_val, int64_t* rec_idx, const PruneState& ps, const TopkSweep* tk) {
  ScoreOut so{rec_val, rec_idx};
  so.tau = tk ? nullptr : ps.tau;
  if (tk) {
    so.sc_val = tk->list_val;
    so.sc_idx = tk->list_idx;
    so.sc_count = tk->head;
  }
  return so;
}
static void launch_topk_pool(Context* c, const PruneState& ps, const TopkSweep* tk, int64_t C) {
  if (!tk) return;
  topk_pool_kernel<<<1, WG, 0, c->stream>>>(tk->k, (int)C, tk->head, tk->pool_val, tk->pool_idx, tk->list_val,
                                            tk->list_idx, ps.tau);
}
hipError_t launch_topk_result(Context* c, const TopkSweep& tk, double* val_out, int64_t* idx_out) {
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  topk_result_kernel<<<(tk.k + WG - 1) / WG, WG, 0, c->stream>>>(tk.k, tk.head, tk.pool_val, tk.pool_idx, val_out,
                                                                 idx_out);
  return hipGetLastError();
}
hipError_t launch_index_shift(Context* c, int64_t* idx, int64_t k, int64_t offset) {
  index_shift_kernel<<<(unsigned)((k + WG - 1) / WG), WG, 0, c->stream>>>(idx, k, offset);
  return hipGetLastError();
}


// The fused small-n sweep covers npad <= 256, d <= 16 (1..8 outputs) and the fp64 covariance build; the rest takes
// the K* + trmm path.  An npad = 384 instance (d <= 8, 226 VGPRs, 2 waves/SIMD) measured slower than the K* + trmm path
// (2.20e8 vs 2.66e8 candidates/s at n = 384, profiles/r01_small_n_rates.log): 24 row blocks of A operands per k-step
// from L2 and half the occupancy of the npad = 256 instance.  The handle option GPX_OPT_SWEEP_FUSED = 0 forces the
// unfused path (A/B measurements, parity tests of both paths).
bool sweep_fused_ok(const Context* c, const gpx_kernel_params& p, int npad, int nrhs) {
  return c->sweep_fused && (npad == 128 || npad == 256) && p.d <= 16 && !p.cov_fp32;
}

bool sweep_prune_ok(const Context* c, const gpx_kernel_params& p, int npad) {
  if (c->sweep_prune == 0 || sweep_fused_ok(c, p, npad, 1)) return false;
  return npad >= (c->sweep_prune != 1 ? PRUNE_MIN_NPAD : PRUNE_DEFAULT_NPAD);  // (-2: forced, exact head means)
}

static int sweep_cu_count(Context* c) {
  if (c->cu_count <= 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      c->cu_count = cus;
  }
  return c->cu_count > 0 ? c->cu_count : 0;  // (unknown: the wide shape throughout)
}

// The grid of a tail launch whose work only the device knows (the gather, the compaction): `units` workgroups would
// cover the round's capacity, but a round is mostly far below it and often empty, and an empty launch costs its grid
// (DESIGN §5).  So at most per_cu workgroups per CU are launched, a small multiple of what the device holds at once,
// and divide the live work among themselves.  Unknown residency or CU count: `units`.
static unsigned tail_grid(Context* c, int per_cu, int64_t units) {
  const int64_t bound = (int64_t)per_cu * sweep_cu_count(c);
  return (unsigned)(bound > 0 && bound < units ? bound : units);
}

// A KSTAR_GATHER round over entries first .. first + cap - 1 of a survivor list of *count {column, slot} pairs: the
// gather writes the round's first descriptor (rows0 row tiles in its first stage; last: that stage is also the last)
// and zeroes its stages' counts, with pad marks the last tile's padding slots in the list, and with mu_out scatters
// the listed candidates' mean partials to mu_out[jb * ldmu + column].
static KstarAux gather_aux(int2* list, const int* count, int first, int cap, const PruneState& ps, int rows0, bool last,
                           double* mu_out, int64_t ldmu, bool pad = true) {
  KstarAux aux{};
  aux.list = reinterpret_cast<int*>(list);
  if (pad) aux.pad = reinterpret_cast<int*>(list);
  aux.lstride = 2;
  aux.count = count;
  aux.first = first;
  aux.cap = cap;
  aux.desc = ps.desc + 1;
  aux.rcount = ps.count + 1;
  aux.stats = ps.stats;
  aux.rows0 = rows0;
  aux.last = last;
  aux.mu_out = mu_out;
  aux.ldmu = ldmu;
  return aux;
}

// K* and the partial means of one chunk (launch 1 of the file comment)
static void launch_kstar(const SweepModel& M, const SweepCands& q, const SweepBuffers& b, int mode = KSTAR_FULL,
                         const KstarAux& aux_in = KstarAux{}, int rows = 0) {
  if (rows == 0) rows = M.npad;  // (KSTAR_FULL over the leading `rows` rows only: the head phase)
  LaunchTimer tm(M.c, GPX_TIMER_KSTAR);
  const gpx_kernel_params& p = M.p;
  const int64_t C = b.chunk;
  hipStream_t stream = M.c->stream;
  // (KSTAR_GATHER: q.m is the most columns the round can have; the kernel reads the count itself and its workgroups
  // stride over the live (column block, row block) units)
  const dim3 g((unsigned)((q.m + WG - 1) / WG), (mode == KSTAR_MU ? M.npad - PRUNE_HEAD_ROWS : rows) / NB);
  KstarAux aux = aux_in;
  aux.nrb = (int)g.y;
  with_dmax(p.d, [&](auto D) {
    constexpr int DM = decltype(D)::value;
    auto diff = [&](auto F32) {  // the difference form
      with_kind(p.kind, [&](auto K) {
        auto rhs = [&](auto ONE) {
          kstar_kernel<DM, decltype(F32)::value, decltype(K)::value, decltype(ONE)::value><<<g, WG, 0, stream>>>(
              p, M.n, M.X, M.ldx, M.alpha, M.nrhs, q.Xs, q.ldxs, q.m, C, b.kstar, b.mu_part);
        };
        M.nrhs == 1 ? rhs(std::true_type{}) : rhs(std::false_type{});
      });
    };
    if (p.cov_fp32) {
      diff(std::true_type{});
    } else if constexpr (DM == 32) {  // d > 16: the MFMA kernel's candidate tile would not fit 64 KB of LDS
      diff(std::false_type{});
    } else {
      with_kind(p.kind, [&](auto K) {
        auto mfma = [&](auto ONE, auto MODE) {
          auto kernel = kstar_mfma_kernel<DM, decltype(K)::value, decltype(ONE)::value, decltype(MODE)::value>;
          dim3 grid = g;
          if constexpr (decltype(MODE)::value == KSTAR_GATHER) {
            static const int resident = [&] {  // workgroups of this instance a CU holds (registers, LDS); 0: unknown
              int r = 0;
              return hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, kernel, WG, 0) == hipSuccess ? r : 0;
            }();
            // twice the resident workgroups: with exactly one wave of them every workgroup of a full round runs its
            // trips in step with the others, and the unprunable case measured 0.4 % slower than with this
            grid = dim3(tail_grid(M.c, 2 * resident, (int64_t)g.x * g.y));
          }
          kernel<<<grid, WG, 0, stream>>>(p, M.n, M.X, M.ldx, M.alpha, M.nrhs, q.Xs, q.ldxs, q.m, C, b.kstar, b.mu_part,
                                          aux);
        };
        M.nrhs != 1          ? mfma(std::false_type{}, Const<KSTAR_FULL>{})
        : mode == KSTAR_FULL ? mfma(std::true_type{}, Const<KSTAR_FULL>{})
        : mode == KSTAR_MU   ? mfma(std::true_type{}, Const<KSTAR_MU>{})
                             : mfma(std::true_type{}, Const<KSTAR_GATHER>{});
      });
    }
  });
}

// The fused head of the lazy form (head_product_kernel): mean partials of row blocks 0 and 1 for the columns the head's
// K* launch covers (whole 256-column blocks of q.m), row tile 0's variance partial for the staged columns' tiles (from
// col0 on, ncols of them), both at pitch C.  The grid is what the device holds at once; the workgroups stride.
// list != nullptr: the list-driven instance over list[0 .. *count - 1] (q.m: the most the list can hold; the same
// bounded grid, so a full list runs as the contiguous launch and a short one costs the grid); desc_out / stats optional.
static void launch_head_product(const SweepModel& M, const SweepCands& q, int64_t C, double* mu_part, double* ss_part,
                                int col0, int64_t ncols, const int2* list = nullptr, const int* count = nullptr,
                                PruneDesc* desc_out = nullptr, int64_t* stats = nullptr) {
  const gpx_kernel_params& p = M.p;
  const int ngroups = (int)((q.m + WG - 1) / WG) * (WG / HP_COLS);
  const int64_t c1s = col0 + (ncols + TT - 1) / TT * TT;
  with_dmax(p.d, [&](auto D) {
    constexpr int DM = decltype(D)::value;
    if constexpr (DM <= 16) {  // (sweep_lazy_ok: d <= 16)
      with_kind(p.kind, [&](auto K) {
        auto kernel = head_product_kernel<DM, decltype(K)::value>;
        static const int resident = [&] {  // workgroups of this instance a CU holds; 0: unknown
          int r = 0;
          return hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, kernel, WG, 0) == hipSuccess ? r : 0;
        }();
        kernel<<<tail_grid(M.c, resident, ngroups), WG, 0, M.c->stream>>>(p, M.n, M.X, M.ldx, M.alpha, q.Xs, q.ldxs, q.m,
                                                                         C, M.W, M.ldw, ngroups, col0, c1s, mu_part,
                                                                         ss_part, list, count, desc_out, stats);
      });
    }
  });
}

// finalize_kernel's arguments of a posterior (a = nullptr: per-output y_mean / y_scale, nullptr = identity) or of an
// acquisition (a's y_mean / y_scale for the one output)
static FinalizeArgs finalize_args(const gpx_kernel_params& p, const gpx_acq_params* a, int nrhs, const double* y_mean,
                                  const double* y_scale) {
  FinalizeArgs fa;
  fa.p = p;
  for (int q = 0; q < GPX_MAX_RHS; ++q) {
    fa.y_mean[q] = (y_mean && q < nrhs) ? y_mean[q] : 0.0;
    fa.y_scale[q] = (y_scale && q < nrhs) ? y_scale[q] : 1.0;
  }
  fa.acq_kind = a ? a->kind : 0;
  fa.best_f = a ? a->best_f : 0.0;
  fa.beta = a ? a->beta : 0.0;
  if (a) {
    fa.y_mean[0] = a->y_mean;
    fa.y_scale[0] = a->y_scale;
  }
  fa.weight = 1.0;
  fa.first = 0;
  fa.acc_mu = fa.acc_var = nullptr;
  return fa;
}
// One output of a multi-output objective in fa's place: its untransform and weight, and the accumulators it goes to
static void set_output(FinalizeArgs& fa, double y_mean, double y_scale, double weight, bool first, double* acc_mu,
                       double* acc_var) {
  fa.y_mean[0] = y_mean;
  fa.y_scale[0] = y_scale;
  fa.weight = weight;
  fa.first = first;
  fa.acc_mu = acc_mu;
  fa.acc_var = acc_var;
}
// The arguments of the passes that read the accumulators alone: no model, no untransform
static FinalizeArgs objective_args(const gpx_acq_params& a, double* acc_mu, double* acc_var) {
  FinalizeArgs fa{};
  fa.acq_kind = a.kind;
  fa.best_f = a.best_f;
  fa.beta = a.beta;
  fa.acc_mu = acc_mu;
  fa.acc_var = acc_var;
  return fa;
}

// K*, the product (launches 1 and 2 of the file comment, or the fused small-n kernel) and one finalize pass over the
// chunk's columns; io: the pass's outputs
template <FinalizePass PASS>
static void sweep_chunk_pass(const SweepModel& M, const SweepCands& q, const SweepBuffers& b, const FinalizeArgs& fa,
                             FinalizeIo io) {
  Context* c = M.c;
  const gpx_kernel_params& p = M.p;
  const int64_t C = b.chunk;
  int nJB = M.npad / NB, nI = M.npad / TT;
  if (sweep_fused_ok(c, p, M.npad, M.nrhs)) {
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    const int nwg = (int)((q.m + 63) / 64);
    auto small = [&](auto NP, auto D, auto K, auto NR) {
      sweep_small_kernel<decltype(NP)::value, decltype(D)::value, decltype(K)::value, decltype(NR)::value>
          <<<nwg, WG, 0, c->stream>>>(p, M.n, M.X, M.ldx, M.alpha, M.nrhs, M.W, M.ldw, q.Xs, q.ldxs, q.m, C, b.mu_part,
                                      b.ss_part);
    };
    auto rows = [&](auto NP) {
      with_dmax(p.d, [&](auto D) {
        if constexpr (decltype(D)::value <= 16)  // (sweep_fused_ok)
          with_kind(p.kind, [&](auto K) {
            M.nrhs == 1 ? small(NP, D, K, Const<1>{}) : small(NP, D, K, Const<GPX_MAX_RHS>{});
          });
      });
    };
    M.npad == 128 ? rows(Const<128>{}) : rows(Const<256>{});
    nJB = nI = 1;
  } else {
    launch_kstar(M, q, b);
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    const int ncbt = (int)((q.m + TT - 1) / TT);
    trmm_sumsq_kernel<<<ncbt * nI, WG, 0, c->stream>>>(M.W, M.ldw, b.kstar, C, nI, ncbt, b.ss_part, 0);
  }
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  io.q = q;
  io.part = {b.mu_part, b.ss_part, C, nJB, nI, M.nrhs};
  launch_finalize<PASS>(c, fa, io);
}

hipError_t launch_sweep_chunk(const SweepModel& M, const SweepCands& q, const SweepBuffers& b, const gpx_acq_params* a,
                              const SweepOut& out, int64_t rec_offset, const MultiOutput* mo) {
  FinalizeArgs fa = finalize_args(M.p, a, M.nrhs, out.y_mean, out.y_scale);
  FinalizeIo io{};
  if (mo) {  // one output of a multi-output objective: accumulate, score later (launch_multi_score)
    set_output(fa, mo->y_mean, mo->y_scale, mo->weight, mo->first, mo->acc_mu, mo->acc_var);
    sweep_chunk_pass<FIN_ACCUMULATE>(M, q, b, fa, io);
  } else if (!a) {
    io.post = {out.mean, out.ldmean, out.var};
    sweep_chunk_pass<FIN_POSTERIOR>(M, q, b, fa, io);
  } else {
    io.score = {b.rec_val + rec_offset, b.rec_idx + rec_offset, out.scores};
    sweep_chunk_pass<FIN_SCORE>(M, q, b, fa, io);
  }
  return hipGetLastError();
}

hipError_t launch_multi_score(Context* c, const SweepCands& q, const MultiOutput& mo, const gpx_acq_params& a,
                              double* scores_out, double* rec_val, int64_t* rec_idx) {
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  FinalizeIo io{};
  io.q = q;
  io.score = {rec_val, rec_idx, scores_out};
  launch_finalize<FIN_SCORE_ACC>(c, objective_args(a, mo.acc_mu, mo.acc_var), io);
  return hipGetLastError();
}

// Stage boundaries of the pruned product: R[0] = 0 < 1 < 2 < 4 < 8 < 16 < nI (those below nI), doubling so that a
// stage costs about three times everything before it: a candidate dropped after stage s has paid R(R+1) / (nI(nI+1)) of
// its product, R = R[s+1].  Returns the number of stages.
static int prune_stage_bounds(int nI, int* R) {
  int S = 0;
  R[0] = 0;
  for (int r = 1; r < nI && r <= 16; r *= 2) R[++S] = r;
  R[++S] = nI;
  return S;
}

// A stage after the first of a chunk, super-chunk or round: `tiles` wide tiles at most, how many are active only the
// device knows.  One launch of the dual kernel; its workgroups take the narrow shape when the stage's wide tiles would
// not give every CU one (trmm_sumsq_body).  The grid is the larger of the two shapes' needs: the narrow shape runs
// below cus wide tiles only, so it needs fewer than 4 cus workgroups.  narrow_below: another bound than cus (0: cus).
static void launch_tail_stage(Context* c, const double* W, int64_t ldw, int64_t C, int nI, double* ss_part,
                              PruneStage st, int tiles, int narrow_below = 0) {
  const int cus = narrow_below ? narrow_below : sweep_cu_count(c);
  st.narrow_below = cus;
  const int64_t wide = (int64_t)tiles * st.nrows;
  const int64_t narrow = 4 * (wide < cus ? wide : (int64_t)cus);
  trmm_stage_dual_kernel<<<(unsigned)(wide > narrow ? wide : narrow), WG, 0, c->stream>>>(W, ldw, C, nI, ss_part, st);
}

// ---- the staged driver: what the chunked and the lazy form of the pruned sweep share --------------------------------
// The columns of a chunk or super-chunk of m candidates: the seed block (the call's first incumbent: its leading
// PRUNE_SEED candidates through the full product and finalize; later candidates start from the best score of
// everything scored before them), and the staged columns behind it.
struct SeedPlan {
  int seed, seed_blocks;  // candidates of the seed block (0: not the call's first), their 256-candidate blocks
  int col0, ncols;        // the staged columns: from the tile behind the seed block on (a short chunk: none)
};
static SeedPlan seed_plan(bool first, int64_t m, int64_t C) {
  SeedPlan sp;
  sp.seed = first ? (int)(m < PRUNE_SEED ? m : PRUNE_SEED) : 0;
  if (sp.seed > C) sp.seed = (int)C;
  sp.seed_blocks = (sp.seed + WG - 1) / WG;
  sp.col0 = ((sp.seed + TT - 1) / TT) * TT;
  sp.ncols = m > sp.col0 ? (int)(m - sp.col0) : 0;
  return sp;
}

static PruneBufs prune_bufs(const double* kstar, int64_t ld0, const PruneState& ps, const int2* list2 = nullptr) {
  return PruneBufs{kstar, ps.cbuf[0], ps.cbuf[1], ld0, ps.ldc[0], ps.ldc[1], ps.list[0], ps.list[1], list2};
}

// prune_init_kernel, then the seed block where the plan has one: K* of its columns (build_kstar: the lazy form; the
// chunked form built the whole chunk's before), the full product in narrow tiles, the score pass, pool.
static void launch_seed_block(const SweepModel& M, const SweepCands& q, const SweepBuffers& b, const PruneState& ps,
                              const FinalizeArgs& fa, const SeedPlan& sp, int R1, bool one_stage, bool first,
                              bool build_kstar, double* rec_val, int64_t* rec_idx, int64_t* host_stats,
                              const TopkSweep* tk, int* count2 = nullptr) {
  Context* c = M.c;
  const int64_t C = b.chunk;
  const int nJB = M.npad / NB, nI = M.npad / TT;
  auto product = [&] {
    const int ncbt = (sp.seed + TT - 1) / TT;
    trmm_sumsq_narrow_kernel<<<4 * ncbt * nI, WG, 0, c->stream>>>(M.W, M.ldw, b.kstar, C, nI, ncbt, b.ss_part);
    host_stats[1] += sp.seed;
    host_stats[2] += (int64_t)ncbt * nI;
  };
  {
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    prune_init_kernel<<<1, 64, 0, c->stream>>>(ps.desc, ps.count, ps.tau, ps.stats, sp.col0, sp.ncols, R1, one_stage,
                                               first, tk ? tk->head : nullptr, count2);
    if (sp.seed && !build_kstar) product();
  }
  if (!sp.seed) return;
  if (build_kstar) {
    launch_kstar(M, q.first(sp.seed), b);
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    product();
  }
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  FinalizeIo io{};
  io.q = q.first(sp.seed);
  io.part = {b.mu_part, b.ss_part, C, nJB, nI, 1};
  io.score = pruned_score_out(rec_val, rec_idx, ps, tk);
  launch_finalize<FIN_SCORE>(c, fa, io);
  launch_topk_pool(c, ps, tk, C);
}

// The staged product of one column set: per stage s the row tiles R[s] .. R[s+1] - 1 of the active columns, after every
// stage but the last the bound pass (FIN_BOUND) and the compaction; then the score pass (FIN_SCORE) over what is left,
// pool.
struct StagePlan {
  PruneBufs pb;          // the K* source and its pitch, the compact buffers, the index lists
  double* mu_part;       // the partial arrays of the columns' own places, and their pitch
  double* ss_part;
  int64_t pitch;
  const int* R;          // stage bounds R[0] < .. < R[ns] = nI
  int ns;
  int desc0;             // descriptor and count of stage 0 (ps.desc + desc0, ps.count + desc0)
  bool wide_first;       // stage 0 is one launch of the wide trmm_stage_kernel; else it goes through launch_tail_stage
  int cap;               // the most columns the set can have
  double* rec_val;       // the record cursor
  int64_t* rec_idx;
  int narrow_below = 0;  // launch_tail_stage's bound for the narrow shape (0: the CU count)
};
static void launch_stages(const SweepModel& M, const SweepCands& q, const PruneState& ps, const FinalizeArgs& fa,
                          const StagePlan& sg, int64_t C, const TopkSweep* tk) {
  Context* c = M.c;
  const int nJB = M.npad / NB, nI = M.npad / TT;
  const int tiles = (sg.cap + TT - 1) / TT;
  PruneDesc* desc = ps.desc + sg.desc0;
  int* count = ps.count + sg.desc0;
  FinalizeIo io{};
  io.q = q.first(sg.cap);
  io.part = {sg.mu_part, sg.ss_part, sg.pitch, nJB, nI, 1};
  io.cols = {nullptr, ps.list[0], ps.list[1], sg.pb.list2};
  {
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    // compaction: a workgroup per 256 slots x 32 rows of the set's capacity at most and per 256 slots at least (no
    // more than the 8 per CU the device holds otherwise); a workgroup copies ROWS rows at least
    const unsigned nsb = (unsigned)((sg.cap / 2 + TT + WG - 1) / WG);
    const unsigned gc = std::max(tail_grid(c, 8, (int64_t)nsb * (M.npad / 32)), nsb);
    constexpr int ROWS = 8;
    for (int s = 0; s < sg.ns; ++s) {
      const PruneStage st{sg.pb, desc + s, sg.R[s], sg.R[s + 1] - sg.R[s], 0};
      if (s == 0 && sg.wide_first)
        trmm_stage_kernel<<<tiles * st.nrows, WG, 0, c->stream>>>(M.W, M.ldw, sg.pitch, nI, sg.ss_part, st);
      else
        launch_tail_stage(c, M.W, M.ldw, sg.pitch, nI, sg.ss_part, st, tiles, sg.narrow_below);
      if (s == sg.ns - 1) break;
      io.cols.desc = desc + s;
      io.part.nI = sg.R[s + 1];
      io.bound = {count + s, ps.tau};
      launch_finalize<FIN_BOUND>(c, fa, io);
      prune_compact_kernel<<<gc, WG, 0, c->stream>>>(sg.pb, desc + s, desc + s + 1, count + s, M.npad, ROWS,
                                                     sg.R[s + 2] - sg.R[s + 1], s + 2 == sg.ns, ps.stats);
    }
  }
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  io.cols.desc = desc + sg.ns - 1;
  io.part.nI = nI;
  io.score = pruned_score_out(sg.rec_val, sg.rec_idx, ps, tk);
  launch_finalize<FIN_SCORE>(c, fa, io);
  launch_topk_pool(c, ps, tk, C);
}

hipError_t launch_sweep_chunk_pruned(const SweepModel& M, const SweepCands& q, const SweepBuffers& b,
                                     const PruneState& ps, const gpx_acq_params* a, int64_t rec_offset, bool first,
                                     int64_t* host_stats, const TopkSweep* tk) {
  const int64_t C = b.chunk;
  int R[PRUNE_MAX_STAGES];
  const int S = prune_stage_bounds(M.npad / TT, R);
  launch_kstar(M, q, b);
  const FinalizeArgs fa = finalize_args(M.p, a, 1, nullptr, nullptr);
  const SeedPlan sp = seed_plan(first, q.m, C);  // (a seed block short of PRUNE_SEED: the whole chunk, no staged columns)
  double* rec_val = b.rec_val + rec_offset;
  int64_t* rec_idx = b.rec_idx + rec_offset;
  launch_seed_block(M, q, b, ps, fa, sp, R[1], S == 1, first, false, rec_val, rec_idx, host_stats, tk);
  if (sp.ncols == 0) return hipGetLastError();
  launch_stages(M, q, ps, fa,
                StagePlan{prune_bufs(b.kstar, C, ps), b.mu_part, b.ss_part, C, R, S, 0, true, sp.ncols,
                          rec_val + sp.seed_blocks, rec_idx + sp.seed_blocks},
                C, tk);
  return hipGetLastError();
}

// The lazy form of the pruned sweep, for the configurations of kstar_mfma_kernel: K* is built in full only
// for the candidates that survive the first row tile.  Per super-chunk of ph.super candidates:
//  head   KSTAR_FULL over the head rows (K* rows 0 .. 127), then the mean of every candidate: for the RBF kernel its bound
//         (gpx_mubound.hip; the bound pass scores its upper end), else or with sweep_prune = -2 KSTAR_MU over the other
//         row blocks (every mean partial); the first stage of the product and its bound pass as one launch each; the
//         survivors land in ph.survivors.  With sweep_head (the default) the KSTAR_FULL launch and the first stage are
//         one launch of head_product_kernel in the first stage's place: the same mean partials of row blocks 0 and 1
//         and the same partial of row tile 0, K* rows 0 .. 127 never stored (ph.head stays unused).
//  seed   the call's first incumbent, in one of two orders.
//         A call of one chunk or less: BEFORE the head, its leading PRUNE_SEED candidates through the full path
//         (launch_seed_block); the head's bound pass selects against their best.
//         A longer call (its first super-chunk): the leading block is a weak seed (on the bench problem its best logEI
//         is -38.7, the optimum -0.66), and the head's bound ranks the candidates without any incumbent.  So the bound
//         pass runs first and keeps every column's bound U (FIN_BOUND with u_out); seed_select_kernel takes the
//         column of the largest U in each of PRUNE_SEED contiguous slices of the span (seed_slice_begin); those columns
//         go through a round like the tail's (gather build, row tiles 1 .. nI - 1 in one stage, the score pass:
//         records, incumbent, for top-k the scored list and the pool); seed_prune_kernel then tests every other
//         column's U against that incumbent.  No column is scored twice.  Later super-chunks have no seed.
//         That is the parent order of a seeded span (sweep_order 0, and always for UCB, the variance acquisition, the
//         top-k form above k = 64, the exact head means and sweep_head 0).  The default, mean-first (sweep_order 1),
//         runs no head before the bound pass: U0 = score_ub(mean bound, prior variance), which bounds U from above
//         because the prior variance bounds the posterior's; the seed is the slice maxima of U0 through EVERY row tile
//         of the product; seed_prune_kernel keeps S1 = {U0 >= incumbent}; the list-driven head_product_kernel builds K*
//         rows 0 .. 127 and row tile 0 for S1 alone; and a second bound pass (FIN_BOUND over S1's list) keeps columns
//         with U >= incumbent: the parent order's survivors whenever the seed's incumbent is the same.  Later
//         super-chunks take the same two passes against the running incumbent, without a seed.
//  tail   rounds of at most C survivors: KSTAR_GATHER rebuilds their full-height columns into the chunk buffer (the bits
//         of the full build) and, after a mean bound, their exact mean partials into ph.mu_part, then the staged pipeline
//         of launch_sweep_chunk_pruned (launch_stages) from row tile 1 on, the partials
//         going to the columns' own places in ph.ss_part.  A span of at most C staged columns has one round and the call
//         stays asynchronous.  A longer one can need up to ceil(ncols / C); the host learns how many (sweep_tail_sync 1,
//         the default): behind the last pass that writes the survivor count ps.count[0] a 4-byte copy takes it to the
//         handle's pinned word with an event behind it, round 0 is enqueued as ever, so the device has work while the
//         host waits for the event, and rounds 1 .. sweep_tail_rounds(count) - 1 follow, mostly none.  With
//         sweep_tail_sync 0, or on a stream that is being captured, the worst case is enqueued and the workgroups of an
//         empty round return at once.  Either way the rounds after the first take fewer, coarser stages (the stage
//         grouping does not change a column's partials), and a round that is enqueued is the same launches in both.
// *recs: records used so far (in ph.rec_val / ph.rec_idx); it advances for the rounds enqueued only.
bool sweep_lazy_ok(const gpx_kernel_params& p) { return !p.cov_fp32 && p.d <= 16; }

hipError_t launch_sweep_super_pruned(const SweepModel& M, const SweepCands& q, const SweepBuffers& b,
                                     const PruneState& ps, const PruneHead& ph, const gpx_acq_params* a, int64_t* recs,
                                     bool first, int64_t* host_stats, const TopkSweep* tk) {
  Context* c = M.c;
  const bool mu_bound = c->sweep_prune != -2 && sweep_mu_bound_ok(M.p);
  const int64_t C = b.chunk, MA = ph.super;
  const int nJB = M.npad / NB, nI = M.npad / TT;
  int R[PRUNE_MAX_STAGES];
  const int S = prune_stage_bounds(nI, R);  // (nI >= 3: S >= 3, R[1] = 1 = the head's row tile)
  static_assert(PRUNE_HEAD_ROWS == TT, "the head phase is the product's first row tile");
  const FinalizeArgs fa = finalize_args(M.p, a, 1, nullptr, nullptr);
  // the seeded order: the call's first span when the call is longer than one chunk (a list of PRUNE_SEED fits a chunk's)
  const bool seeded = first && q.m > C && C >= PRUNE_SEED;
  // the mean-first order (sweep_order 1): a seeded span and the spans behind the first, with the mean's bound and the
  // fused head.  S1, the columns its first prune pass keeps, goes to the head rows' region (idle under sweep_head), its
  // count to the slot behind the seed list's.  EI and logEI only: the RBF prior variance is the same for every column,
  // so U0 ranks by the mean alone, and UCB and the variance acquisition, whose order the variance decides, got a weaker
  // seed and more survivors from it than from the head's bound.  The top-k form up to k = 64 only: its incumbent is the
  // k-th best of the seed's 1024 exact scores, so near k = 1024 every slice's seed counts, and U0 picks them worse than
  // the head's bound does.  Both limits are measured in DESIGN §5 (tools/order_limits_probe.py on a build with
  // GPX_MEAN_FIRST_UNLIMITED, which drops them: a measurement build, never the shipped one).
#ifdef GPX_MEAN_FIRST_UNLIMITED
  const bool mean_ranked = true;
#else
  const bool mean_ranked = (a->kind == GPX_ACQ_EI || a->kind == GPX_ACQ_LOGEI) && (!tk || tk->k <= 64);
#endif
  const bool mean_first = c->sweep_order == 1 && c->sweep_head && mu_bound && mean_ranked && (seeded || !first);
  static_assert(4 * (PRUNE_MAX_STAGES + 2) <= 256, "two slots behind the stages' counts");
  int2* s1 = reinterpret_cast<int2*>(ph.head);
  int* n1 = ps.count + PRUNE_MAX_STAGES + 1;
  const SeedPlan sp = seed_plan(first && !seeded, q.m, C);  // (seeded: no leading block, every column is staged)
  // (mean-first: the head's tiles are counted by its own launch, from S1)
  launch_seed_block(M, q, b, ps, fa, sp, mean_first ? 0 : R[1], false, first, true, ph.rec_val + *recs,
                    ph.rec_idx + *recs, host_stats, tk, mean_first ? n1 : nullptr);
  *recs += sp.seed_blocks;
  if (sp.ncols == 0) return hipGetLastError();
  // head: the columns of the whole super-chunk (a leading seed block's again: the head kernel has no column offset)
  {
    SweepBuffers hb = b;
    hb.kstar = ph.head;
    hb.mu_part = ph.mu_part;
    hb.chunk = MA;
    // (sweep_head: head_product_kernel below builds these rows in registers, in the first stage's place)
    if (!c->sweep_head) launch_kstar(M, q, hb, KSTAR_FULL, KstarAux{}, PRUNE_HEAD_ROWS);
    if (mu_bound) {
      // the mean's bound instead of the mean.  Its two values per candidate go to the mean partials' rows of blocks 2
      // and 3 (the head rows' launch wrote blocks 0 and 1; nothing writes the others before the gather), the row
      // blocks' records to ph.prep (the layout's view of the chunk's K* buffer, idle between the seed block's scoring
      // and the first gather).
      static_assert(PRUNE_MIN_NPAD / NB >= 4, "mean partial rows 2 and 3 exist");
      (void)launch_mu_bound(M, q, ph.prep, ph.mu_part + 2 * MA, ph.mu_part + 3 * MA);  // (the error is read at the end)
    } else {
      KstarAux aux{};
      aux.jb0 = PRUNE_HEAD_ROWS / NB;
      launch_kstar(M, q, hb, KSTAR_MU, aux);
    }
  }
  // The seeded order keeps every column's score bound U in the variance partials' row of tile 1: no stage writes it before
  // the seed's and the survivors' own, each at its columns only and before any pass reads them there.  The seed list is
  // the second index list: a round of one stage has no bound pass, so neither list is written before the prune pass.
  static_assert(PRUNE_MIN_NPAD / TT >= 2 && 4 * (PRUNE_MAX_STAGES + 1) <= 256, "partial row 1; a slot behind the counts");
  double* U = ph.ss_part + MA;
  int2* seed = ps.list[1];
  int* nseed = ps.count + PRUNE_MAX_STAGES;
  {
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    if (mean_first) {
      // no product before the bound pass: it takes the prior variance in the variance bound's place and reads no
      // partial.  A seeded span keeps these bounds U0 in U; a later span selects S1 against the running incumbent.
    } else if (c->sweep_head) {
      launch_head_product(M, q, MA, ph.mu_part, ph.ss_part, sp.col0, sp.ncols);
    } else {
      const PruneStage st{prune_bufs(ph.head, MA, ps), ps.desc, 0, R[1], 0};
      trmm_stage_kernel<<<(sp.ncols + TT - 1) / TT * st.nrows, WG, 0, c->stream>>>(M.W, M.ldw, MA, nI, ph.ss_part, st);
    }
    FinalizeIo io{};
    io.q = q.first(sp.ncols);
    io.part = {ph.mu_part, ph.ss_part, MA, nJB, mean_first ? 0 : R[1], 1};
    io.cols.desc = ps.desc;
    io.cols.list0 = mean_first ? s1 : ph.survivors;  // (the descriptor's list is -1: the survivors go to list0)
    io.bound.count = mean_first ? n1 : ps.count;
    io.bound.tau = ps.tau;
    io.bound.mu_bound = mu_bound ? ph.mu_part + 2 * MA : nullptr;
    io.bound.u_out = seeded ? U : nullptr;  // (seeded: no incumbent yet, the bounds are kept)
    launch_finalize<FIN_BOUND>(c, fa, io);
    if (seeded) seed_select_kernel<<<PRUNE_SEED, WG, 0, c->stream>>>(U, q.m, seed, nseed);
  }
  if (seeded) {
    // seed: the best bound of each slice through the gather build and the rest of the product (tile 0's partial is the
    // head's; mean-first: every row tile, the stage kernels' tile 0 has the head's bits) as one round of one stage:
    // exact scores, records, the incumbent (top-k: the scored list and the pool)
    const int Rs[2] = {mean_first ? 0 : 1, nI};
    // (mean-first at padded n = 4096: the seed's 8 x 32 wide tiles are exactly the 256 CUs, one tile each, and the stage
    // lasts as long as its deepest tile: 0.46 ms in the wide shape against 0.37 ms for the parent's 8 x 31 narrow ones,
    // DESIGN §5.  So the seed's stage keeps the narrow shape at equality too.)
    const int seed_narrow = mean_first && sweep_cu_count(c) > 0 ? sweep_cu_count(c) + 1 : 0;
    // (pad = false: the seed list is whole tiles and lives in an index list, nothing to mark in it)
    launch_kstar(M, q.first(PRUNE_SEED), b, KSTAR_GATHER,
                 gather_aux(seed, nseed, 0, PRUNE_SEED, ps, nI - Rs[0], true, mu_bound ? ph.mu_part : nullptr, MA,
                            false));
    launch_stages(M, q, ps, fa,
                  StagePlan{prune_bufs(b.kstar, C, ps, seed), ph.mu_part, ph.ss_part, MA, Rs, 1, 1, false, PRUNE_SEED,
                            ph.rec_val + *recs, ph.rec_idx + *recs, seed_narrow},
                  C, tk);
    *recs += PRUNE_SEED / WG;
    // prune: every other column's bound against the seed's incumbent (mean-first: pass 1, into S1)
    LaunchTimer tm(c, GPX_TIMER_ACQ);
    seed_prune_kernel<<<(sp.ncols + WG - 1) / WG, WG, 0, c->stream>>>(U, q.m, seed, ps.tau, mean_first ? s1 : ph.survivors,
                                                                      mean_first ? n1 : ps.count);
  }
  if (mean_first) {
    // the head over S1 alone (it also writes S1's descriptor to ps.desc[0], read by nothing else from here on), then
    // prune pass 2: the bound pass of the parent's order over S1, with the head's variance partial.  U1 <= U0, so the
    // survivors are the parent's whenever the incumbent is.
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    launch_head_product(M, q.first(sp.ncols), MA, ph.mu_part, ph.ss_part, 0, 0, s1, n1, ps.desc, ps.stats);
    FinalizeIo io{};
    io.q = q.first(sp.ncols);
    io.part = {ph.mu_part, ph.ss_part, MA, nJB, R[1], 1};
    io.cols.desc = ps.desc;
    io.cols.list0 = ph.survivors;  // (the descriptor's list is 2: the survivors go to list0)
    io.cols.list2 = s1;
    io.bound = {ps.count, ps.tau, ph.mu_part + 2 * MA};
    launch_finalize<FIN_BOUND>(c, fa, io);
  }
  // tail (its passes read the survivors' exact partials, written by their gather).  Nothing from here on writes
  // ps.count[0] (the rounds' counts start at ps.count + 1), so a span that can need more than one round sends the count
  // to the host now, behind the last pass that wrote it; round 0 is enqueued before the host waits for it.
  const int64_t worst = (sp.ncols + C - 1) / C;
  int64_t rounds = worst;
  bool readback = worst > 1 && c->sweep_tail_sync && c->tail_count && c->tail_event;
  if (readback) {
    // (a wait on an event recorded during capture is an error, and a captured call must replay for any count)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) {
      (void)hipGetLastError();
      readback = false;
    } else if (cap != hipStreamCaptureStatusNone) {
      readback = false;
    }
  }
  if (readback) {
    hipError_t e = hipMemcpyAsync(c->tail_count, ps.count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->tail_event, c->stream);
    if (e != hipSuccess) return e;
  }
  c->tail_rounds[1] += worst;
  for (int64_t r0 = 0; r0 < sp.ncols; r0 += C) {
    if (r0 == C && readback) {
      const hipError_t e = hipEventSynchronize(c->tail_event);
      if (e != hipSuccess) return e;
      const int64_t count = *static_cast<volatile int32_t*>(c->tail_count);
      c->tail_rounds[2] = (c->tail_rounds[2] < 0 ? 0 : c->tail_rounds[2]) + count;
      rounds = sweep_tail_rounds(count, sp.ncols, C);
    }
    if (r0 / C >= rounds) break;
    ++c->tail_rounds[0];
    const int cap = (int)(sp.ncols - r0 < C ? sp.ncols - r0 : C);  // the most columns this round can have
    // stage boundaries Rr[0] = 1 < .. < Rr[ns] = nI: round 0 the doubling ones, later rounds 1 < 4 < nI
    int Rr[PRUNE_MAX_STAGES], ns = 0;
    if (r0 == 0) {
      for (int s = 1; s <= S; ++s) Rr[s - 1] = R[s];
      ns = S - 1;
    } else {
      Rr[0] = 1;
      if (nI > 4) Rr[++ns] = 4;
      Rr[++ns] = nI;
    }
    launch_kstar(M, q.first(cap), b, KSTAR_GATHER,
                 gather_aux(ph.survivors, ps.count, (int)r0, cap, ps, Rr[1] - Rr[0], ns == 1,
                            mu_bound ? ph.mu_part : nullptr, MA));
    launch_stages(M, q, ps, fa,
                  StagePlan{prune_bufs(b.kstar, C, ps, ph.survivors + r0), ph.mu_part, ph.ss_part, MA, Rr, ns, 1, false,
                            cap, ph.rec_val + *recs, ph.rec_idx + *recs},
                  C, tk);
    *recs += (cap + WG - 1) / WG;
  }
  return hipGetLastError();
}

// The pruned top-k sweep of a linear objective over T independent outputs (gpx_acquire_topk_multi_f64), one
// chunk.  One K*, mu_part and ss_part buffer serves the outputs in turn, always in ascending t, so the accumulators of a
// candidate scored in full form in the full multi-output sweep's order.
//  seed   (the call's first chunk) the leading PRUNE_SEED candidates through launch_sweep_chunk with the accumulators,
//         FIN_SCORE_ACC into the scored list, pool: the pool's k-th score is the incumbent.
//  head   per output: K* rows 0 .. 127 (KSTAR_FULL) and the other row blocks' mean partials (KSTAR_MU), row tile 0 of
//         the product, FIN_ACCUMULATE over that tile's partial alone: exact mean, upper bound of the variance.  Then
//         FIN_BOUND_ACC: the survivors go to ph.survivors, their count to ps.count[0].
//  tail   per output: KSTAR_GATHER rebuilds the survivors' columns (mean partials scattered to the columns' own places),
//         every row tile through launch_tail_stage, FIN_ACCUMULATE through the round's descriptor with all nI partials.
//         Then FIN_SCORE_ACC through the descriptor into the scored list, pool.  The grids are sized for every staged
//         column; workgroups beyond the survivors return at once.
hipError_t launch_topk_multi_chunk(Context* c, int T, const MultiModel* outs, int n, int npad, const double* X,
                                   int64_t ldx, const SweepCands& q, const SweepWorkspace& w, const gpx_acq_params& a,
                                   bool first, int64_t* host_stats) {
  const SweepBuffers& b = w.b;
  const PruneState& ps = w.ps;
  const TopkSweep* tk = &w.tk;
  const int64_t C = b.chunk;
  const int nJB = npad / NB, nI = npad / TT;
  const SeedPlan sp = seed_plan(first, q.m, C);
  auto model = [&](int t) {
    return SweepModel{c, *outs[t].p, n, npad, X, ldx, outs[t].W, outs[t].ldw, outs[t].alpha, 1};
  };
  auto accumulate = [&](int t) {  // FIN_ACCUMULATE's arguments of output t
    FinalizeArgs fa = finalize_args(*outs[t].p, &a, 1, nullptr, nullptr);
    set_output(fa, outs[t].y_mean, outs[t].y_scale, outs[t].weight, t == 0, w.acc_mu, w.acc_var);
    return fa;
  };
  const FinalizeArgs fs = objective_args(a, w.acc_mu, w.acc_var);  // the accumulators' score and bound passes
  auto score = [&](int64_t cols, const ColumnSet& set) {  // the accumulators' score into the scored list, then the pool
    LaunchTimer tm(c, GPX_TIMER_ACQ);
    FinalizeIo io{};
    io.q = q.first(cols);
    io.cols = set;
    io.score = pruned_score_out(b.rec_val, b.rec_idx, ps, tk);
    launch_finalize<FIN_SCORE_ACC>(c, fs, io);
    launch_topk_pool(c, ps, tk, C);
  };
  // (rows0 = T: the head runs one row tile per output over the staged columns' tiles)
  prune_init_kernel<<<1, 64, 0, c->stream>>>(ps.desc, ps.count, ps.tau, ps.stats, sp.col0, sp.ncols, T, 0, first,
                                             tk->head);
  if (sp.seed) {
    for (int t = 0; t < T; ++t)
      sweep_chunk_pass<FIN_ACCUMULATE>(model(t), q.first(sp.seed), b, accumulate(t), FinalizeIo{});
    host_stats[1] += sp.seed;
    host_stats[2] += (int64_t)T * ((sp.seed + TT - 1) / TT) * nI;
    score(sp.seed, ColumnSet{});
  }
  if (sp.ncols == 0) return hipGetLastError();
  const int tiles = (sp.ncols + TT - 1) / TT;
  FinalizeIo io{};  // the staged columns' passes: the head's through the chunk's descriptor, the tail's the round's
  io.q = q.first(sp.ncols);
  io.part = {b.mu_part, b.ss_part, C, nJB, 1, 1};
  io.cols.desc = ps.desc;
  for (int t = 0; t < T; ++t) {
    const SweepModel M = model(t);
    launch_kstar(M, q, b, KSTAR_FULL, KstarAux{}, PRUNE_HEAD_ROWS);
    KstarAux aux{};
    aux.jb0 = PRUNE_HEAD_ROWS / NB;
    launch_kstar(M, q, b, KSTAR_MU, aux);
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    const PruneStage st{prune_bufs(b.kstar, C, ps), ps.desc, 0, 1, 0};
    trmm_stage_kernel<<<tiles, WG, 0, c->stream>>>(M.W, M.ldw, C, nI, b.ss_part, st);
    launch_finalize<FIN_ACCUMULATE>(c, accumulate(t), io);
  }
  {
    LaunchTimer tm(c, GPX_TIMER_ACQ);
    FinalizeIo sel = io;
    sel.cols.list0 = w.ph.survivors;  // (the descriptor's list is -1: the survivors go to list0)
    sel.bound = {ps.count, ps.tau};
    launch_finalize<FIN_BOUND_ACC>(c, fs, sel);
  }
  io.part.nI = nI;
  io.cols.desc = ps.desc + 1;
  io.cols.list2 = w.ph.survivors;
  for (int t = 0; t < T; ++t) {
    const SweepModel M = model(t);
    // (last: the survivors count as computed to the end once, with the last output)
    launch_kstar(M, q.first(sp.ncols), b, KSTAR_GATHER,
                 gather_aux(w.ph.survivors, ps.count, 0, sp.ncols, ps, nI, t == T - 1, b.mu_part, C));
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    const PruneStage st{prune_bufs(b.kstar, C, ps, w.ph.survivors), ps.desc + 1, 0, nI, 0};
    launch_tail_stage(c, M.W, M.ldw, C, nI, b.ss_part, st, tiles);
    launch_finalize<FIN_ACCUMULATE>(c, accumulate(t), io);
  }
  score(sp.ncols, io.cols);
  return hipGetLastError();
}

// gpx_debug_stage_product_f64's column set: the descriptor of slots 0 .. ncols - 1 in place and, with a list, its
// {output column, slot} form padded with -1 to the last wide tile's end.
__global__ void __launch_bounds__(WG) debug_stage_setup_kernel(PruneDesc* __restrict__ desc, int2* __restrict__ out,
                                                               const int* __restrict__ list, int ncols, int ntiles) {
  const int s = blockIdx.x * WG + threadIdx.x;
  if (s == 0) {
    PruneDesc d;
    d.buf = 0;
    d.col0 = 0;
    d.ncols = ncols;
    d.ntiles = ntiles;
    d.list = list ? 0 : -1;
    d.pad[0] = d.pad[1] = d.pad[2] = 0;
    *desc = d;
  }
  if (list && s < ntiles * TT) out[s] = make_int2(s < ncols ? list[s] : -1, s);
}

size_t debug_stage_product_bytes(int64_t ncols) { return 256 + (size_t)((ncols + TT - 1) / TT) * TT * sizeof(int2); }

hipError_t launch_debug_stage_product(Context* c, int npad, const double* W, int64_t ldw, const double* kstar,
                                      int64_t ldk, int ncols, const int* list, int I0, int nrows, int shape, double* ss,
                                      int64_t ldss, void* ws) {
  const int nI = npad / TT, ntiles = (ncols + TT - 1) / TT;
  PruneDesc* desc = reinterpret_cast<PruneDesc*>(ws);
  int2* list2 = reinterpret_cast<int2*>(reinterpret_cast<char*>(ws) + 256);
  debug_stage_setup_kernel<<<(ntiles * TT + WG - 1) / WG, WG, 0, c->stream>>>(desc, list2, list, ncols, ntiles);
  PruneBufs pb{};
  pb.kstar = kstar;
  pb.ld0 = ldk;
  pb.list0 = list2;
  const PruneStage st{pb, desc, I0, nrows, 0};
  if (shape == 0)
    trmm_stage_kernel<<<ntiles * nrows, WG, 0, c->stream>>>(W, ldw, ldss, nI, ss, st);
  else
    trmm_stage_narrow_kernel<<<4 * ntiles * nrows, WG, 0, c->stream>>>(W, ldw, ldss, nI, ss, st);
  return hipGetLastError();
}

hipError_t launch_debug_head_product(const SweepModel& M, const SweepCands& q, double* ss, double* mu_part, int64_t ld,
                                     const int32_t* list, const int32_t* count) {
  launch_head_product(M, q, ld, mu_part, ss, 0, (q.m + WG - 1) / WG * WG, reinterpret_cast<const int2*>(list), count);
  return hipGetLastError();
}

hipError_t launch_debug_kstar(const SweepModel& M, const SweepCands& q, const int* list, const int* count, double* out,
                              int64_t ldout, double* mu_scratch, double* mu_part, int64_t ldmu) {
  SweepBuffers b{};
  b.kstar = out;
  b.chunk = ldout;
  b.mu_part = mu_scratch;  // (npad/64) x ldout mean partials of a zero alpha, then the zero alpha
  if (!list && M.alpha) {  // the full build's own mean partials (pitch ldout)
    b.mu_part = mu_part;
    launch_kstar(M, q, b);
  } else if (!list) {
    double* alpha = mu_scratch + (size_t)(M.npad / NB) * ldout;
    hipError_t e = hipMemsetAsync(alpha, 0, (size_t)M.npad * 8, M.c->stream);
    if (e != hipSuccess) return e;
    launch_kstar(SweepModel{M.c, M.p, M.n, M.npad, M.X, M.ldx, nullptr, 0, alpha, 1}, q, b);
  } else {  // the gather build (no mean: alpha unread; else it scatters the listed candidates' partials to
            // mu_part[jb * ldmu + list[s]])
    KstarAux aux{};
    aux.list = list;
    aux.lstride = 1;
    aux.count = count;
    aux.first = 0;
    aux.cap = (int)q.m;
    if (M.alpha) {
      aux.mu_out = mu_part;
      aux.ldmu = ldmu;
    }
    launch_kstar(M, q, b, KSTAR_GATHER, aux);
  }
  return hipGetLastError();
}

// ---- SVGP predictive: one task of Bayesian7's batched SVGP over a chunk --------------------
// mean = const + K_*Z alpha' (alpha' = L^{-T} m), var = k** - |L^{-1} k*|^2 + |S^T L^{-1} k*|^2 + noise, i.e. the
// whitened VariationalStrategy predictive k** + k*^T L^{-T} (S S^T - I) L^{-1} k* plus the GaussianLikelihood noise
// [upstream]; score (optional) accumulates sum_t var_t over the tasks (the pool-scan score, Bayesian7.py:671).
__global__ void __launch_bounds__(WG) svgp_finalize_kernel(gpx_kernel_params p, double min_var, int task,
                                                           const double* __restrict__ Xs, int64_t ldxs,
                                                           int64_t m_chunk, int64_t C, int nJB, int nI,
                                                           const double* __restrict__ mu_part,
                                                           const double* __restrict__ ss1,
                                                           const double* __restrict__ ss2,
                                                           double* __restrict__ mean_out, int64_t ldmean,
                                                           double* __restrict__ var_out, int64_t ldvar,
                                                           double* __restrict__ score) {
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (c >= m_chunk) return;
  const double kd = prior_variance(p, Xs, ldxs, c);
  const double s1 = sum_partials(ss1 + c, nI, C);
  const double s2 = sum_partials(ss2 + c, nI, C);
  const double var = fmax(kd - s1 + s2 + p.noise, min_var);
  const double mu = sum_partials(mu_part + c, nJB, C) + p.const_mean;
  if (mean_out) mean_out[c * ldmean + task] = mu;
  if (var_out) var_out[c * ldvar + task] = var;
  if (score) score[c] = (task == 0 ? 0.0 : score[c]) + var;
}

// One task of gpx_svgp_acquire_f64's objective in svgp_finalize_kernel's place: the task's LATENT moments from the same
// partials in the same operation order (no likelihood noise: an analytic acquisition is about f; GPyTorch's 1e-10
// floor), into the chunk's accumulators by FIN_ACCUMULATE's own step (accumulate_output).  FIN_SCORE_ACC scores them
// (launch_multi_score): objective_moments and acq_score stay the only statements of the floors and formulas.
__global__ void __launch_bounds__(WG) svgp_objective_kernel(gpx_kernel_params p, MultiOutput mo,
                                                            const double* __restrict__ Xs, int64_t ldxs,
                                                            int64_t m_chunk, int64_t C, int nJB, int nI,
                                                            const double* __restrict__ mu_part,
                                                            const double* __restrict__ ss1,
                                                            const double* __restrict__ ss2) {
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (c >= m_chunk) return;
  const double kd = prior_variance(p, Xs, ldxs, c);
  const double s1 = sum_partials(ss1 + c, nI, C);
  const double s2 = sum_partials(ss2 + c, nI, C);
  const double var = fmax(kd - s1 + s2, 1e-10);  // gpytorch min_variance (float64) [upstream]
  const double mu = sum_partials(mu_part + c, nJB, C) + p.const_mean;
  accumulate_output(mo.acc_mu, mo.acc_var, c, mo.first, mo.weight, mo.y_mean, mo.y_scale, mu, var);
}

// (mo: gpx_svgp_acquire_f64's form; min_var, task and the output pointers are then not used)
hipError_t launch_svgp_chunk(Context* c, const gpx_kernel_params& p, double min_var, int task, int M, int Mpad,
                             const double* Z, int64_t ldz, const double* W, const double* W2, int64_t ldw,
                             const double* alpha, const double* Xs, int64_t ldxs, int64_t m_chunk,
                             const SweepBuffers& b, double* ss2, double* mean_out, int64_t ldmean, double* var_out,
                             int64_t ldvar, double* score, const MultiOutput* mo) {
  const int64_t C = b.chunk;
  const int nJB = Mpad / NB, nI = Mpad / TT;
  const int ncb = (int)((m_chunk + WG - 1) / WG);
  {
    LaunchTimer tm(c, GPX_TIMER_KSTAR);
    dim3 g(ncb, nJB);
    with_dmax(p.d, [&](auto D) {
      with_kind(p.kind, [&](auto K) {
        kstar_kernel<decltype(D)::value, false, decltype(K)::value, true><<<g, WG, 0, c->stream>>>(
            p, M, Z, ldz, alpha, 1, Xs, ldxs, m_chunk, C, b.kstar, b.mu_part);
      });
    });
  }
  {
    LaunchTimer tm(c, GPX_TIMER_TRMM);
    const int ncbt = (int)((m_chunk + TT - 1) / TT);
    trmm_sumsq_kernel<<<dim3(ncbt * nI, 2), WG, 0, c->stream>>>(W, ldw, b.kstar, C, nI, ncbt, b.ss_part, 0, W2, ss2);
  }
  {
    LaunchTimer tm(c, GPX_TIMER_ACQ);
    if (mo)
      svgp_objective_kernel<<<ncb, WG, 0, c->stream>>>(p, *mo, Xs, ldxs, m_chunk, C, nJB, nI, b.mu_part, b.ss_part,
                                                       ss2);
    else
      svgp_finalize_kernel<<<ncb, WG, 0, c->stream>>>(p, min_var, task, Xs, ldxs, m_chunk, C, nJB, nI, b.mu_part,
                                                      b.ss_part, ss2, mean_out, ldmean, var_out, ldvar, score);
  }
  return hipGetLastError();
}

// K(Z, X_chunk) alone through the same build (the collapsed SVGP fit, gpx_svgpfit.hip): kstar is Mpad x ldk (ldk a
// multiple of 256, the build's column granule), rows >= M zero; zero_alpha: Mpad zeros, mu_scratch: (Mpad / 64) x ldk.
hipError_t launch_svgp_kchunk(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                              const double* zero_alpha, const double* Xs, int64_t ldxs, int64_t m_chunk, int64_t ldk,
                              double* kstar, double* mu_scratch) {
  LaunchTimer tm(c, GPX_TIMER_KSTAR);
  dim3 g((int)((m_chunk + WG - 1) / WG), Mpad / NB);
  with_dmax(p.d, [&](auto D) {
    with_kind(p.kind, [&](auto K) {
      kstar_kernel<decltype(D)::value, false, decltype(K)::value, true><<<g, WG, 0, c->stream>>>(
          p, M, Z, ldz, zero_alpha, 1, Xs, ldxs, m_chunk, ldk, kstar, mu_scratch);
    });
  });
  return hipGetLastError();
}

hipError_t launch_argmax_final(Context* c, const double* vals, const int64_t* idx, int64_t count, double* best_val,
                               int64_t* best_idx) {
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  argmax_final_kernel<<<1, WG, 0, c->stream>>>(vals, idx, count, 1, best_val, best_idx);
  return hipGetLastError();
}

// (best_val, best_idx) -> one 16-byte record {double value; int64 index} (the send buffer of the exchange)
__global__ void record_pack_kernel(const double* __restrict__ best_val, const int64_t* __restrict__ best_idx,
                                   int64_t* __restrict__ rec) {
  if (threadIdx.x == 0) {
    rec[0] = __double_as_longlong(*best_val);
    rec[1] = *best_idx;
  }
}

hipError_t launch_record_pack(Context* c, const double* best_val, const int64_t* best_idx, int64_t* rec) {
  record_pack_kernel<<<1, 64, 0, c->stream>>>(best_val, best_idx, rec);
  return hipGetLastError();
}

hipError_t launch_argmax_records(Context* c, const int64_t* rec, int64_t count, double* best_val, int64_t* best_idx) {
  LaunchTimer tm(c, GPX_TIMER_ACQ);
  argmax_final_kernel<<<1, WG, 0, c->stream>>>(reinterpret_cast<const double*>(rec), rec + 1, count, 2, best_val,
                                               best_idx);
  return hipGetLastError();
}

}  // namespace gpx
