// Monte-Carlo q-batch acquisition values and their gradients w.r.t. the q-batch moments (gpx_mc_acq_f64): the small
// q x q part of optimize_acqf that follows gpx_moments_grad_f64 (optimization/Bayesian.py:100-112 and
// Bayesian2.py:240-245: qLogEI with q = batch_size; Bayesian6.py:113-130, 896-919: qPosteriorStandardDeviation).
// One workgroup per q-batch b:
//   A = (cov + cov^T) / 2, L = chol(A) with a per-batch jitter retry (A + j I, j = 1e-8, 1e-7, 1e-6), f_s = mean + L z_s
//   QLOGEI  li = log tau_relu + log(softplus(y) + 0.1 / (1 + y^2)), y = (f - best_f) / tau_relu   (fat_relu; else the
//           log-softplus form with its branch at y <= -37); r_s = fatmax_i or tau_max logsumexp_i of li;
//           value = logsumexp_s r_s - log S
//   QPSD    value = sum_i sqrt(l_i C l_i^T), C the unbiased sample covariance of the rows of z (formed once per call)
// and backward: Lbar = d value / d L (lower triangle), P = Phi(L^T Lbar) (lower triangle, diagonal halved),
// G = L^{-T} P L^{-1}, gcov = (G + G^T) / 2, which is what differentiating the symmetrised Cholesky gives.
// mcnei_kernel (gpx_mc_nei_f64) is the same chain for qNoisyExpectedImprovement (optimization/Bayesian1.py:118-140): the
// q-batch conditioned on the baseline points' samples, improvement against a per-sample incumbent.
// Every sum runs in a fixed order (strided partials, then fixed trees): two calls give the same bits.  No inline asm.
#include "gpx_internal.h"

namespace gpx {

namespace {

constexpr int MQ = GPX_MAX_Q;
constexpr int LDQ = MQ + 1;  // LDS row pitch of the q x q matrices (odd: a column walk touches distinct banks)
constexpr int LDB = GPX_MAX_BASELINE + 1;  // LDS row pitch of the q x nb matrix A of mcnei_kernel
constexpr double FAT_ALPHA = 2.0;

__device__ inline double softplus64(double y) { return fmax(y, 0.0) + log1p(exp(-fabs(y))); }

__device__ inline double sigmoid64(double y) {
  if (y >= 0.0) return 1.0 / (1.0 + exp(-y));
  const double e = exp(y);
  return e / (1.0 + e);
}

// log-improvement of one sample entry, in units of y = (f - best_f) / tau_relu (log tau_relu is added by the caller)
__device__ inline double log_improvement(double y, int fat_relu) {
  if (fat_relu) return log(softplus64(y) + 0.1 / (1.0 + y * y));
  return y > -37.0 ? log(softplus64(y)) : y;
}

// d li / d y
__device__ inline double log_improvement_dy(double y, int fat_relu) {
  if (fat_relu) {
    const double c = 1.0 + y * y;
    return (sigmoid64(y) - 0.2 * y / (c * c)) / (softplus64(y) + 0.1 / c);
  }
  return y > -37.0 ? sigmoid64(y) / softplus64(y) : 1.0;
}

// Sum of term(s) over s = 0 .. S-1 by the P consecutive lanes of one group (P a power of two <= 64, groups aligned
// to P, every lane of a group calls together): lane p adds s = p, p + P, ... in order, then an xor butterfly.  Every
// lane of the group returns the same bits.
template <class F>
__device__ inline double group_sum(int p, int P, int S, F term) {
  double acc = 0.0;
  for (int s = p; s < S; s += P) acc += term(s);
  for (int o = P >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// lanes per group for E independent sums over the workgroup's WG threads
__device__ inline int group_lanes(int E) {
  int P = 64;
  while (P > 1 && P * E > WG) P >>= 1;
  return P;
}

// (i, j), j <= i, of the t-th entry of a row-major lower triangle
__device__ inline void tri_index(int t, int* i, int* j) {
  int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  *i = r;
  *j = t - r * (r + 1) / 2;
}

// fixed-order tree over the workgroup; red: WG doubles of LDS.  Every thread returns the result.
template <bool MAX>
__device__ inline double block_reduce(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = WG / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = MAX ? fmax(red[tid], red[tid + o]) : red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// L = chol(A + jitter I) of the q x q matrix As into Ls (lower triangle), column by column: thread i owns row i; a
// failed pivot retries with the next jitter.  Returns the attempt that factored (0 .. 3) or -1, uniform over the
// workgroup.  col: MQ doubles, bad: one int of LDS.
__device__ __forceinline__ int jittered_factor(int q, const double* As, double* Ls, double* col, int* bad) {
  const int tid = threadIdx.x;
  int status = -1;
  for (int attempt = 0; attempt < 4; ++attempt) {
    const double jitter = attempt == 0 ? 0.0 : attempt == 1 ? 1e-8 : attempt == 2 ? 1e-7 : 1e-6;
    if (tid == 0) *bad = 0;
    __syncthreads();
    for (int j = 0; j < q; ++j) {
      if (tid >= j && tid < q) {
        double s = As[tid * LDQ + j];
        if (tid == j) s += jitter;
        for (int k = 0; k < j; ++k) s -= Ls[tid * LDQ + k] * Ls[j * LDQ + k];
        col[tid] = s;
      }
      __syncthreads();
      const double piv = col[j];
      if (!(piv > 0.0)) {  // <= 0 or NaN; uniform over the workgroup
        if (tid == 0) *bad = 1;
        break;
      }
      if (tid >= j && tid < q) Ls[tid * LDQ + j] = tid == j ? sqrt(piv) : col[tid] / sqrt(piv);
      __syncthreads();
    }
    __syncthreads();
    if (!*bad) {
      status = attempt;
      break;
    }
    __syncthreads();
  }
  return status;
}

// Through the factor: from Lbar = d value / d L (Lb, lower triangle) to G = d value / d A of A = L L^T symmetrised:
// P = Phi(L^T Lbar), X = P L^{-1} (row r by thread r), G = L^{-T} X (column c by thread c), gcov = (G + G^T) / 2
// (q x q, row pitch q).  Ws keeps G unsymmetrised.
__device__ __forceinline__ void factor_backward(int q, const double* Ls, const double* Lb, double* Ws,
                                                double* __restrict__ gcov) {
  const int tid = threadIdx.x;
  for (int e = tid; e < q * q; e += WG) {
    const int i = e / q, j = e % q;
    double v = 0.0;
    if (j <= i) {
      for (int k = i; k < q; ++k) v += Ls[k * LDQ + i] * Lb[k * LDQ + j];
      if (i == j) v *= 0.5;
    }
    Ws[i * LDQ + j] = v;
  }
  __syncthreads();
  if (tid < q) {
    double* x = Ws + tid * LDQ;
    for (int j = q - 1; j >= 0; --j) {
      double v = x[j];
      for (int k = j + 1; k < q; ++k) v -= x[k] * Ls[k * LDQ + j];
      x[j] = v / Ls[j * LDQ + j];
    }
  }
  __syncthreads();
  if (tid < q) {
    for (int i = q - 1; i >= 0; --i) {
      double v = Ws[i * LDQ + tid];
      for (int k = i + 1; k < q; ++k) v -= Ls[k * LDQ + i] * Ws[k * LDQ + tid];
      Ws[i * LDQ + tid] = v / Ls[i * LDQ + i];
    }
  }
  __syncthreads();
  for (int e = tid; e < q * q; e += WG) {
    const int i = e / q, j = e % q;
    gcov[e] = 0.5 * (Ws[i * LDQ + j] + Ws[j * LDQ + i]);
  }
}

// q-reduction r_s of sample s from its log-improvements Li[i * S + s] and their maximum M
__device__ __forceinline__ double q_reduce(const double* Li, int S, int s, int q, double M, int fat_max, double tau_max,
                                           double inv_max, double inv_fat) {
  double sum = 0.0;
  for (int i = 0; i < q; ++i) {
    const double li = Li[(int64_t)i * S + s];
    if (fat_max) {
      const double t = 1.0 + (M - li) * inv_fat;
      sum += 1.0 / (t * t);
    } else {
      sum += exp((li - M) * inv_max);
    }
  }
  return M + tau_max * log(sum);
}

// backward of sample s with weight w = d value / d r_s: fbar_si = w dr/dli_i dli_i/df_i, written over f in F[i * S + s]
__device__ __forceinline__ void q_reduce_backward(const double* Li, double* F, int S, int s, int q, double w,
                                                  double best_f, int fat_relu, int fat_max, double inv_relu,
                                                  double inv_max, double inv_fat) {
  double M = -INFINITY;
  int am = 0;
  for (int i = 0; i < q; ++i) {
    const double li = Li[(int64_t)i * S + s];
    if (li > M) {
      M = li;
      am = i;
    }
  }
  double den = 0.0, num3 = 0.0;  // sum_i t^-2 (or exp), and sum_{i != am} t^-3
  for (int i = 0; i < q; ++i) {
    const double li = Li[(int64_t)i * S + s];
    if (fat_max) {
      const double t = 1.0 + (M - li) * inv_fat;
      den += 1.0 / (t * t);
      if (i != am) num3 += 1.0 / (t * t * t);
    } else {
      den += exp((li - M) * inv_max);
    }
  }
  for (int i = 0; i < q; ++i) {
    const double li = Li[(int64_t)i * S + s];
    double dr;
    if (fat_max) {
      // the maximum enters r directly and through every t: its share is what keeps the weights summing to one
      const double t = 1.0 + (M - li) * inv_fat;
      dr = i == am ? 1.0 - num3 / den : 1.0 / (t * t * t) / den;
    } else {
      dr = exp((li - M) * inv_max) / den;
    }
    const double y = (F[(int64_t)i * S + s] - best_f) * inv_relu;
    F[(int64_t)i * S + s] = w * dr * log_improvement_dy(y, fat_relu) * inv_relu;
  }
}

// C (q x q, row pitch q) = unbiased sample covariance of the rows of z (S x q); one workgroup
__global__ void __launch_bounds__(WG) mcacq_zcov_kernel(int q, int S, const double* __restrict__ z,
                                                        double* __restrict__ C) {
  __shared__ double zbar[MQ];
  const int tid = threadIdx.x;
  {
    const int P = group_lanes(q), p = tid % P;
    for (int e = tid / P; e < q; e += WG / P) {
      const double v = group_sum(p, P, S, [&](int s) { return z[(int64_t)s * q + e]; });
      if (p == 0) zbar[e] = v / (double)S;
    }
  }
  __syncthreads();
  const int E = q * (q + 1) / 2;
  const int P = group_lanes(E), p = tid % P;
  for (int e = tid / P; e < E; e += WG / P) {
    int i, j;
    tri_index(e, &i, &j);
    const double zi = zbar[i], zj = zbar[j];
    const double v = group_sum(p, P, S, [&](int s) {
      return (z[(int64_t)s * q + i] - zi) * (z[(int64_t)s * q + j] - zj);
    });
    if (p == 0) {
      C[i * q + j] = v / (double)(S - 1);
      C[j * q + i] = v / (double)(S - 1);
    }
  }
}

// r: S doubles per batch; Li, F: q x S per batch (entry i of sample s at [i * S + s])
__global__ void __launch_bounds__(WG) mcacq_kernel(gpx_mcacq_params a, int q, int S, const double* __restrict__ mean,
                                                   const double* __restrict__ cov, const double* __restrict__ z,
                                                   const double* __restrict__ C, double* __restrict__ value,
                                                   double* __restrict__ gmean, double* __restrict__ gcov,
                                                   int32_t* __restrict__ info, double* __restrict__ Rws,
                                                   double* __restrict__ Liws, double* __restrict__ Fws) {
  __shared__ double As[MQ * LDQ], Ls[MQ * LDQ], Lb[MQ * LDQ], Ws[MQ * LDQ];
  __shared__ double mu[MQ], col[MQ], red[WG];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const bool grad = gmean != nullptr;
  const double nan = __builtin_nan("");
  cov += b * q * q;
  mean += b * q;

  for (int e = tid; e < q * q; e += WG) {
    const int i = e / q, j = e % q;
    As[i * LDQ + j] = 0.5 * (cov[i * q + j] + cov[j * q + i]);
  }
  if (tid < q) mu[tid] = mean[tid];

  const int status = jittered_factor(q, As, Ls, col, &bad);
  if (tid == 0) info[b] = status;
  if (status < 0) {
    if (tid == 0) value[b] = nan;
    if (grad) {
      if (tid < q) gmean[b * q + tid] = nan;
      for (int e = tid; e < q * q; e += WG) gcov[b * q * q + e] = nan;
    }
    return;
  }
  for (int e = tid; e < q * q; e += WG) {  // clear what the factor did not write
    const int i = e / q, j = e % q;
    if (j > i) Ls[i * LDQ + j] = 0.0;
    Lb[i * LDQ + j] = 0.0;
  }
  __syncthreads();

  if (a.kind == GPX_MCACQ_QPSD) {
    // U = L C; var_i = sum_{j <= i} U_ij L_ij; value = sum_i sqrt(var_i); Lbar_ij = U_ij / std_i
    for (int e = tid; e < q * q; e += WG) {
      const int i = e / q, j = e % q;
      double u = 0.0;
      for (int k = 0; k <= i; ++k) u += Ls[i * LDQ + k] * C[k * q + j];
      Ws[i * LDQ + j] = u;
    }
    __syncthreads();
    if (tid < q) {
      double v = 0.0;
      for (int j = 0; j <= tid; ++j) v += Ws[tid * LDQ + j] * Ls[tid * LDQ + j];
      col[tid] = sqrt(v);
    }
    __syncthreads();
    if (tid == 0) {
      double v = 0.0;
      for (int i = 0; i < q; ++i) v += col[i];
      value[b] = v;
    }
    if (!grad) return;
    if (tid < q) gmean[b * q + tid] = 0.0;
    for (int e = tid; e < q * q; e += WG) {
      const int i = e / q, j = e % q;
      if (j <= i) Lb[i * LDQ + j] = Ws[i * LDQ + j] / col[i];
    }
    __syncthreads();
  } else {
    double* R = Rws + b * S;
    double* Li = Liws + b * q * S;
    double* F = Fws + b * q * S;
    const double inv_relu = 1.0 / a.tau_relu, log_relu = log(a.tau_relu);
    const double inv_max = 1.0 / a.tau_max, inv_fat = 1.0 / (FAT_ALPHA * a.tau_max);
    // ---- forward: f, li and the q-reduction r_s of the thread's samples
    double rmax = -INFINITY;
    for (int s = tid; s < S; s += WG) {
      const double* zs = z + (int64_t)s * q;
      double M = -INFINITY;
      for (int i = 0; i < q; ++i) {
        double f = mu[i];
        for (int j = 0; j <= i; ++j) f += Ls[i * LDQ + j] * zs[j];
        const double li = log_relu + log_improvement((f - a.best_f) * inv_relu, a.fat_relu);
        if (grad) F[(int64_t)i * S + s] = f;
        Li[(int64_t)i * S + s] = li;
        M = fmax(M, li);
      }
      const double r = q_reduce(Li, S, s, q, M, a.fat_max, a.tau_max, inv_max, inv_fat);
      R[s] = r;
      rmax = fmax(rmax, r);
    }
    rmax = block_reduce<true>(rmax, red);
    double part = 0.0;
    for (int s = tid; s < S; s += WG) part += exp(R[s] - rmax);
    const double lse = rmax + log(block_reduce<false>(part, red));
    if (tid == 0) value[b] = lse - log((double)S);
    if (!grad) return;
    // ---- backward per sample: fbar_si = w_s dr/dli_i dli_i/df_i, written over f
    for (int s = tid; s < S; s += WG) {
      const double w = exp(R[s] - lse);
      q_reduce_backward(Li, F, S, s, q, w, a.best_f, a.fat_relu, a.fat_max, inv_relu, inv_max, inv_fat);
    }
    __syncthreads();  // fbar of every sample is visible to the workgroup
    // ---- gmean_i = sum_s fbar_si; Lbar_ij = sum_s fbar_si z_sj (j <= i)
    const int E = q + q * (q + 1) / 2;
    const int P = group_lanes(E), p = tid % P;
    for (int e = tid / P; e < E; e += WG / P) {
      if (e < q) {
        const double* Fi = F + (int64_t)e * S;
        const double v = group_sum(p, P, S, [&](int s) { return Fi[s]; });
        if (p == 0) gmean[b * q + e] = v;
      } else {
        int i, j;
        tri_index(e - q, &i, &j);
        const double* Fi = F + (int64_t)i * S;
        const double v = group_sum(p, P, S, [&](int s) { return Fi[s] * z[(int64_t)s * q + j]; });
        if (p == 0) Lb[i * LDQ + j] = v;
      }
    }
    __syncthreads();
  }

  factor_backward(q, Ls, Lb, Ws, gcov + b * q * q);
}

// Noisy expected improvement (gpx_mc_nei_f64): the q-batch conditioned on the nb baseline points.  Per q-batch b, with
// Linv the inverse of the baseline's factor (nb x nb, shared by every batch, read from global memory):
//   A = cross Linv^T (q x nb), D = (cov + cov^T) / 2 - A A^T = L L^T (the jitter ladder of mcacq_kernel),
//   f_si = mean_i + sum_j A_ij zb_sj + sum_{j <= i} L_ij zq_sj, improvement against the sample's incumbent best_s
//   log = 0: value = (1/S) sum_s max(0, max_i f_si - best_s), the gradient of the max at the lowest maximal index
//   log = 1: mcacq_kernel's QLOGEI chain with best_s in the place of best_f
// and backward: gcov = d value / d D through the factor, Abar_ij = sum_s fbar_si zb_sj, gcross = (Abar - 2 gcov A) Linv.
// r: S doubles per batch; Li, F: q x S per batch; T: q x nb per batch.
__global__ void __launch_bounds__(WG) mcnei_kernel(gpx_mcnei_params a, int q, int nb, int S,
                                                   const double* __restrict__ mean, const double* __restrict__ cov,
                                                   const double* __restrict__ cross, const double* __restrict__ Linv,
                                                   const double* __restrict__ zb, const double* __restrict__ best,
                                                   const double* __restrict__ zq, double* __restrict__ value,
                                                   double* __restrict__ gmean, double* __restrict__ gcov,
                                                   double* __restrict__ gcross, int32_t* __restrict__ info,
                                                   double* __restrict__ Rws, double* __restrict__ Liws,
                                                   double* __restrict__ Fws, double* __restrict__ Tws) {
  __shared__ double As[MQ * LDQ], Ls[MQ * LDQ], Lb[MQ * LDQ], Ws[MQ * LDQ];
  __shared__ double Am[MQ * LDB];
  __shared__ double mu[MQ], col[MQ], red[WG];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const bool grad = gmean != nullptr;
  const double nan = __builtin_nan("");
  cov += b * q * q;
  mean += b * q;
  cross += b * q * nb;

  if (tid < q) mu[tid] = mean[tid];
  for (int e = tid; e < q * nb; e += WG) {
    const int i = e / nb, j = e % nb;
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += cross[i * nb + k] * Linv[j * nb + k];
    Am[i * LDB + j] = v;
  }
  __syncthreads();
  for (int e = tid; e < q * q; e += WG) {
    const int i = e / q, j = e % q;
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += Am[i * LDB + k] * Am[j * LDB + k];
    As[i * LDQ + j] = 0.5 * (cov[i * q + j] + cov[j * q + i]) - v;
  }

  const int status = jittered_factor(q, As, Ls, col, &bad);
  if (tid == 0) info[b] = status;
  if (status < 0) {
    if (tid == 0) value[b] = nan;
    if (grad) {
      if (tid < q) gmean[b * q + tid] = nan;
      for (int e = tid; e < q * q; e += WG) gcov[b * q * q + e] = nan;
      for (int e = tid; e < q * nb; e += WG) gcross[b * q * nb + e] = nan;
    }
    return;
  }
  for (int e = tid; e < q * q; e += WG) {  // clear what the factor did not write
    const int i = e / q, j = e % q;
    if (j > i) Ls[i * LDQ + j] = 0.0;
    Lb[i * LDQ + j] = 0.0;
  }
  __syncthreads();

  double* R = Rws + b * S;
  double* Li = Liws + b * q * S;
  double* F = Fws + b * q * S;
  double* T = Tws + b * q * nb;
  const double inv_relu = 1.0 / a.tau_relu, log_relu = log(a.tau_relu);
  const double inv_max = 1.0 / a.tau_max, inv_fat = 1.0 / (FAT_ALPHA * a.tau_max);
  // ---- forward: f, then the improvement (log = 0) or li and the q-reduction r_s (log = 1) of the thread's samples
  double rmax = -INFINITY, part = 0.0;
  for (int s = tid; s < S; s += WG) {
    const double* zbs = zb + (int64_t)s * nb;
    const double* zqs = zq + (int64_t)s * q;
    const double bs = best[s];
    double M = -INFINITY;
    for (int i = 0; i < q; ++i) {
      double f = mu[i];
      for (int j = 0; j < nb; ++j) f += Am[i * LDB + j] * zbs[j];
      for (int j = 0; j <= i; ++j) f += Ls[i * LDQ + j] * zqs[j];
      if (grad) F[(int64_t)i * S + s] = f;
      if (a.log) {
        const double li = log_relu + log_improvement((f - bs) * inv_relu, a.fat_relu);
        Li[(int64_t)i * S + s] = li;
        M = fmax(M, li);
      } else {
        M = fmax(M, f);
      }
    }
    if (a.log) {
      const double r = q_reduce(Li, S, s, q, M, a.fat_max, a.tau_max, inv_max, inv_fat);
      R[s] = r;
      rmax = fmax(rmax, r);
    } else {
      part += fmax(M - bs, 0.0);
    }
  }
  double lse = 0.0;
  if (a.log) {
    rmax = block_reduce<true>(rmax, red);
    for (int s = tid; s < S; s += WG) part += exp(R[s] - rmax);
    lse = rmax + log(block_reduce<false>(part, red));
    if (tid == 0) value[b] = lse - log((double)S);
  } else {
    const double total = block_reduce<false>(part, red);
    if (tid == 0) value[b] = total / (double)S;
  }
  if (!grad) return;
  // ---- backward per sample: fbar_si written over f
  for (int s = tid; s < S; s += WG) {
    if (a.log) {
      const double w = exp(R[s] - lse);
      q_reduce_backward(Li, F, S, s, q, w, best[s], a.fat_relu, a.fat_max, inv_relu, inv_max, inv_fat);
    } else {
      double M = -INFINITY;
      int am = 0;
      for (int i = 0; i < q; ++i) {
        const double f = F[(int64_t)i * S + s];
        if (f > M) {  // strict: the lowest maximal index
          M = f;
          am = i;
        }
      }
      const double w = M > best[s] ? 1.0 / (double)S : 0.0;
      for (int i = 0; i < q; ++i) F[(int64_t)i * S + s] = i == am ? w : 0.0;
    }
  }
  __syncthreads();  // fbar of every sample is visible to the workgroup
  // ---- gmean_i = sum_s fbar_si; Lbar_ij = sum_s fbar_si zq_sj (j <= i); Abar_ij = sum_s fbar_si zb_sj
  const int E1 = q + q * (q + 1) / 2, E = E1 + q * nb;
  const int P = group_lanes(E), p = tid % P;
  for (int e = tid / P; e < E; e += WG / P) {
    if (e < q) {
      const double* Fi = F + (int64_t)e * S;
      const double v = group_sum(p, P, S, [&](int s) { return Fi[s]; });
      if (p == 0) gmean[b * q + e] = v;
    } else if (e < E1) {
      int i, j;
      tri_index(e - q, &i, &j);
      const double* Fi = F + (int64_t)i * S;
      const double v = group_sum(p, P, S, [&](int s) { return Fi[s] * zq[(int64_t)s * q + j]; });
      if (p == 0) Lb[i * LDQ + j] = v;
    } else {
      const int i = (e - E1) / nb, j = (e - E1) % nb;
      const double* Fi = F + (int64_t)i * S;
      const double v = group_sum(p, P, S, [&](int s) { return Fi[s] * zb[(int64_t)s * nb + j]; });
      if (p == 0) T[i * nb + j] = v;
    }
  }
  __syncthreads();

  factor_backward(q, Ls, Lb, Ws, gcov + b * q * q);
  // ---- T = Abar - 2 gcov A (each thread its own entries), then gcross = T Linv
  for (int e = tid; e < q * nb; e += WG) {
    const int i = e / nb, j = e % nb;
    double v = 0.0;
    for (int k = 0; k < q; ++k) v += (Ws[i * LDQ + k] + Ws[k * LDQ + i]) * Am[k * LDB + j];
    T[e] -= v;
  }
  __syncthreads();
  for (int e = tid; e < q * nb; e += WG) {
    const int i = e / nb, j = e % nb;
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += T[i * nb + k] * Linv[k * nb + j];
    gcross[b * q * nb + e] = v;
  }
}

}  // namespace

size_t mc_acq_ws_doubles(int64_t B, int64_t q, int64_t S) { return (size_t)(MQ * MQ) + (size_t)B * S * (2 * q + 1); }

hipError_t launch_mc_acq(Context* c, const gpx_mcacq_params& a, int B, int q, int S, const double* mean,
                         const double* cov, const double* z, double* value, double* gmean, double* gcov, int32_t* info,
                         double* ws) {
  double* C = ws;
  double* R = C + MQ * MQ;
  double* Li = R + (size_t)B * S;
  double* F = Li + (size_t)B * q * S;
  if (a.kind == GPX_MCACQ_QPSD) mcacq_zcov_kernel<<<1, WG, 0, c->stream>>>(q, S, z, C);
  mcacq_kernel<<<(unsigned)B, WG, 0, c->stream>>>(a, q, S, mean, cov, z, C, value, gmean, gcov, info, R, Li, F);
  return hipGetLastError();
}

size_t mc_nei_ws_doubles(int64_t B, int64_t q, int64_t nb, int64_t S) {
  return (size_t)B * S * (2 * q + 1) + (size_t)B * q * nb;
}

hipError_t launch_mc_nei(Context* c, const gpx_mcnei_params& a, int B, int q, int nb, int S, const double* mean,
                         const double* cov, const double* cross, const double* Linv, const double* zb,
                         const double* best, const double* zq, double* value, double* gmean, double* gcov,
                         double* gcross, int32_t* info, double* ws) {
  double* R = ws;
  double* Li = R + (size_t)B * S;
  double* F = Li + (size_t)B * q * S;
  double* T = F + (size_t)B * q * S;
  mcnei_kernel<<<(unsigned)B, WG, 0, c->stream>>>(a, q, nb, S, mean, cov, cross, Linv, zb, best, zq, value, gmean, gcov,
                                                  gcross, info, R, Li, F, T);
  return hipGetLastError();
}

}  // namespace gpx
