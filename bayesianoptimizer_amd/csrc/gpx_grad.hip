// Posterior moments of q-batches of candidates and their derivatives w.r.t. the candidate inputs: the GPU side of
// gradient-based acquisition optimisation (SURVEY §8f row 4 — optimize_acqf's L-BFGS-B restarts on qLogEI,
// optimization/Bayesian.py:100-112, optimization/Bayesian2.py:218-245; BoTorch differentiates the exact GP posterior
// with torch autograd [upstream]).  For candidates x_a (rows of Xs, consecutive q-batches) and c in a's batch:
//   mean[a]        = m + k_a^T alpha                    dmean[a][j]   = sum_i d1k(x_a, X_i)/dx_aj alpha_i
//   cov[a][c]      = k(x_a, x_c) - k_a^T K^{-1} k_c     dcov[a][j][c] = d1k(x_a, x_c)/dx_aj - sum_i d1k(x_a, X_i)/dx_aj s_ic
// with s_c = K^{-1} k_c = W (W^T k_c) (two triangular fp64-MFMA products over npad x mpad, gpx_gemm.h) and d1k the
// partial derivative in the kernel's FIRST argument.  The chain rule through the symmetric q x q covariance is then
//   dL/dx_aj = gmean[a] dmean[a][j] + sum_c (gcov[a][c] + gcov[c][a]) dcov[a][j][c]
// (bayesianoptimizer_amd/acqf.py), the diagonal included (d k(x,x) = 2 d1k(x,x) by symmetry).
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_gemm.h"

namespace gpx {

// K*[i][c] = k(X_i, Xs_c) for i < n, c < m; 0 elsewhere (npad x mpad, row length mpad).
__global__ void __launch_bounds__(WG) kstar_plain_kernel(gpx_kernel_params p, int n, int npad, int m, int mpad,
                                                         const double* __restrict__ X, int64_t ldx,
                                                         const double* __restrict__ Xs, int64_t ldxs,
                                                         double* __restrict__ Ks) {
  const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (e >= (int64_t)npad * mpad) return;
  const int i = (int)(e / mpad), c = (int)(e % mpad);
  double v = 0.0;
  if (i < n && c < m) {
    const bool lin = p.kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
    double r2 = 0.0, lv = 0.0;
    for (int k = 0; k < p.d; ++k) {
      const double a = X[(int64_t)i * ldx + k], b = Xs[(int64_t)c * ldxs + k];
      const double df = a / p.lengthscale[k] - b / p.lengthscale[k];
      r2 += df * df;
      if (lin) lv += a * p.linear_variance[k] * b;
    }
    v = cov_from_r2(p.kind, p.outputscale, r2, lv);
  }
  Ks[e] = v;
}

// Deterministic 256-thread sum of `cnt` per-thread values (wave shuffles, then the 4 wave partials in order).
template <int CNT>
__device__ __forceinline__ void block_sum(double (&v)[CNT], double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < CNT; ++q) {
    double s = v[q];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[w * CNT + q] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < CNT; ++q) v[q] = ((red[q] + red[CNT + q]) + red[2 * CNT + q]) + red[3 * CNT + q];
  __syncthreads();
}

// One workgroup per (candidate a = blockIdx.y, batch member cc = blockIdx.x).
template <int DMAX>
__global__ void __launch_bounds__(WG) moments_grad_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                          int64_t ldx, const double* __restrict__ alpha,
                                                          const double* __restrict__ Xs, int64_t ldxs, int q,
                                                          const double* __restrict__ S, int mpad,
                                                          double* __restrict__ mean, double* __restrict__ dmean,
                                                          double* __restrict__ cov, double* __restrict__ dcov) {
  __shared__ double red[4 * (2 * DMAX + 2)];
  const int a = blockIdx.y, cc = blockIdx.x;
  const int c = (a / q) * q + cc;  // batch member
  const int d = p.d;
  double xa[DMAX], xc[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    xa[k] = (k < d) ? Xs[(int64_t)a * ldxs + k] : 0.0;
    xc[k] = (k < d) ? Xs[(int64_t)c * ldxs + k] : 0.0;
  }
  const bool first = (cc == 0);
  // acc[0] = sum k s_ic, acc[1..d] = sum dk s_ic, acc[DMAX+1] = sum k alpha_i, acc[DMAX+2..] = sum dk alpha_i
  double acc[2 * DMAX + 2];
#pragma unroll
  for (int q2 = 0; q2 < 2 * DMAX + 2; ++q2) acc[q2] = 0.0;
  for (int i = threadIdx.x; i < n; i += WG) {
    double xi[DMAX], g[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) xi[k] = (k < d) ? X[(int64_t)i * ldx + k] : 0.0;
    const double kv = cov_and_grad<DMAX>(p, xa, xi, g);
    const double s = S[(int64_t)i * mpad + c];
    acc[0] += kv * s;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) acc[1 + k] += g[k] * s;
    if (first) {
      const double al = alpha[i];
      acc[DMAX + 1] += kv * al;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) acc[DMAX + 2 + k] += g[k] * al;
    }
  }
  block_sum<2 * DMAX + 2>(acc, red);
  if (threadIdx.x != 0) return;
  double gp[DMAX];
  const double kac = cov_and_grad<DMAX>(p, xa, xc, gp);
  cov[(int64_t)a * q + cc] = kac - acc[0];
  for (int k = 0; k < d; ++k) dcov[((int64_t)a * d + k) * q + cc] = gp[k] - acc[1 + k];
  if (first) {
    mean[a] = p.const_mean + acc[DMAX + 1];
    for (int k = 0; k < d; ++k) dmean[(int64_t)a * d + k] = acc[DMAX + 2 + k];
  }
}

size_t moments_grad_ws_doubles(int npad, int m) {
  const int mpad = ((m + NB - 1) / NB) * NB;
  const size_t blk = (size_t)npad * mpad;
  size_t p1 = gemm_split_doubles(npad, mpad, npad);
  return 3 * blk + p1 + 64;
}

hipError_t launch_moments_grad(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                               const double* W, int64_t ldw, const double* alpha, const double* Xs, int64_t ldxs,
                               int m, int q, double* mean, double* dmean, double* cov, double* dcov, double* ws) {
  const int mpad = ((m + NB - 1) / NB) * NB;
  const size_t blk = (size_t)npad * mpad;
  double* Ks = ws;
  double* V = Ks + blk;
  double* S = V + blk;
  double* P = S + blk;
  const int64_t tot = (int64_t)npad * mpad;
  kstar_plain_kernel<<<(unsigned)((tot + WG - 1) / WG), WG, 0, c->stream>>>(p, n, npad, m, mpad, X, ldx, Xs, ldxs, Ks);
  // V = W^T K*  (A(r, k) = W[k][r], nonzero for k <= r)
  hipError_t e = launch_gemm64<true, true, KR_A_LOWER>(c, npad, mpad, npad, W, ldw, Ks, mpad, nullptr, 0, V, mpad, 1.0,
                                                       0, P);
  if (e != hipSuccess) return e;
  // S = W V = K^{-1} K*  (A(r, k) = W[r][k], nonzero for k >= r)
  e = launch_gemm64<false, true, KR_A_UPPER>(c, npad, mpad, npad, W, ldw, V, mpad, nullptr, 0, S, mpad, 1.0, 0, P);
  if (e != hipSuccess) return e;
  const dim3 grid(q, m);
#define GPX_MG(D)                                                                                                    \
  moments_grad_kernel<D><<<grid, WG, 0, c->stream>>>(p, n, X, ldx, alpha, Xs, ldxs, q, S, mpad, mean, dmean, cov, \
                                                     dcov)
  if (p.d <= 4)
    GPX_MG(4);
  else if (p.d <= 8)
    GPX_MG(8);
  else if (p.d <= 16)
    GPX_MG(16);
  else
    GPX_MG(32);
#undef GPX_MG
  return hipGetLastError();
}

// ---- the baseline side of qNoisyExpectedImprovement (optimization/Bayesian1.py:118-140) ------------------------------
// mean_b[c] = const_mean + sum_i K*[i][c] alpha_i (thread c, i in order) and cov_bb (mb x mb, contiguous) out of its
// padded form Cp (row length mbpad).
__global__ void __launch_bounds__(WG) joint_finish_kernel(double const_mean, int n, int mb, int mbpad,
                                                          const double* __restrict__ Ks,
                                                          const double* __restrict__ alpha,
                                                          const double* __restrict__ Cp, double* __restrict__ mean_b,
                                                          double* __restrict__ cov_bb) {
  const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (e >= (int64_t)mb * mb) return;
  const int r = (int)(e / mb), c = (int)(e % mb);
  cov_bb[e] = Cp[(int64_t)r * mbpad + c];
  if (e < mb) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += Ks[(int64_t)i * mbpad + e] * alpha[i];
    mean_b[e] = const_mean + acc;
  }
}

static inline int pad_nb(int m) { return ((m + NB - 1) / NB) * NB; }

size_t joint_moments_ws_doubles(int npad, int mb) {
  const int mbpad = pad_nb(mb);
  const size_t blk = (size_t)npad * mbpad, sq = (size_t)mbpad * mbpad;
  const size_t p1 = gemm_split_doubles(npad, mbpad, npad), p2 = gemm_split_doubles(mbpad, mbpad, npad);
  return 2 * blk + 2 * sq + (p1 > p2 ? p1 : p2) + 64;
}

hipError_t launch_joint_moments(Context* c, const gpx_kernel_params& p, int n, int npad, const double* X, int64_t ldx,
                                const double* W, int64_t ldw, const double* alpha, const double* Xb, int mb,
                                int64_t ldxb, double* mean_b, double* cov_bb, double* Sb, int64_t ldsb, double* ws) {
  const int mbpad = pad_nb(mb);
  const size_t blk = (size_t)npad * mbpad, sq = (size_t)mbpad * mbpad;
  double* Ks = ws;
  double* V = Ks + blk;
  double* Kbb = V + blk;
  double* Cp = Kbb + sq;
  double* P = Cp + sq;
  const int64_t tot = (int64_t)npad * mbpad, totb = (int64_t)mbpad * mbpad;
  kstar_plain_kernel<<<(unsigned)((tot + WG - 1) / WG), WG, 0, c->stream>>>(p, n, npad, mb, mbpad, X, ldx, Xb, ldxb, Ks);
  kstar_plain_kernel<<<(unsigned)((totb + WG - 1) / WG), WG, 0, c->stream>>>(p, mb, mbpad, mb, mbpad, Xb, ldxb, Xb, ldxb,
                                                                            Kbb);
  // V = W^T K*, then K_bb - V^T V
  hipError_t e = launch_gemm64<true, true, KR_A_LOWER>(c, npad, mbpad, npad, W, ldw, Ks, mbpad, nullptr, 0, V, mbpad, 1.0,
                                                       0, P);
  if (e != hipSuccess) return e;
  e = launch_gemm64<true, true, KR_FULL>(c, mbpad, mbpad, npad, V, mbpad, V, mbpad, Kbb, mbpad, Cp, mbpad, -1.0, 0, P);
  if (e != hipSuccess) return e;
  if (Sb) {  // Sb = W V = K^{-1} K*
    e = launch_gemm64<false, true, KR_A_UPPER>(c, npad, mbpad, npad, W, ldw, V, mbpad, nullptr, 0, Sb, ldsb, 1.0, 0, P);
    if (e != hipSuccess) return e;
  }
  const int64_t out = (int64_t)mb * mb;
  joint_finish_kernel<<<(unsigned)((out + WG - 1) / WG), WG, 0, c->stream>>>(p.const_mean, n, mb, mbpad, Ks, alpha, Cp,
                                                                             mean_b, cov_bb);
  return hipGetLastError();
}

// One workgroup per (candidate a = blockIdx.y, baseline point b = blockIdx.x): cross[a][b] and its partials in x_a,
// contracting k(x_a, X_i) and d1k(x_a, X_i) against column b of Sb = K^{-1} K(X, Xb) (the L-BFGS-B evaluations: a few
// candidates).
template <int DMAX>
__global__ void __launch_bounds__(WG) cross_cov_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                       int64_t ldx, const double* __restrict__ Sb, int64_t ldsb,
                                                       const double* __restrict__ Xb, int64_t ldxb,
                                                       const double* __restrict__ Xs, int64_t ldxs, int nb,
                                                       double* __restrict__ cross, double* __restrict__ dcross) {
  constexpr int CNT = DMAX + 1;
  __shared__ double red[4 * CNT];
  const int a = blockIdx.y, b = blockIdx.x;
  const int d = p.d;
  double xa[DMAX], xb[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    xa[k] = (k < d) ? Xs[(int64_t)a * ldxs + k] : 0.0;
    xb[k] = (k < d) ? Xb[(int64_t)b * ldxb + k] : 0.0;
  }
  double acc[CNT];  // acc[0] = sum k s_ib, acc[1..d] = sum dk s_ib
#pragma unroll
  for (int t = 0; t < CNT; ++t) acc[t] = 0.0;
  for (int i = threadIdx.x; i < n; i += WG) {
    double xi[DMAX], g[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) xi[k] = (k < d) ? X[(int64_t)i * ldx + k] : 0.0;
    const double kv = cov_and_grad<DMAX>(p, xa, xi, g);
    const double s = Sb[(int64_t)i * ldsb + b];
    acc[0] += kv * s;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) acc[1 + k] += g[k] * s;
  }
  block_sum<CNT>(acc, red);
  if (threadIdx.x != 0) return;
  double gp[DMAX];
  const double kab = cov_and_grad<DMAX>(p, xa, xb, gp);
  cross[(int64_t)a * nb + b] = kab - acc[0];
  for (int k = 0; k < d; ++k) dcross[((int64_t)a * d + k) * nb + b] = gp[k] - acc[1 + k];
}

// Value-only cross-covariance (raw-sample scoring: thousands of candidates): one workgroup per CROSS_CA consecutive
// candidates, so that k(x_a, X_i) is evaluated once per pair and a row of Sb serves CROSS_CA candidates.  Tile by tile
// over the training points: thread t evaluates its point i = tile + t against the candidates into LDS; then thread
// (g = t / 64, b = t % 64) adds the tile's points r = g, g + 4, ... times Sb[r][b] in order.  The four partial sums
// per (candidate, b) are added in a fixed order.
constexpr int CROSS_CA = 4;
template <int DMAX>
__global__ void __launch_bounds__(WG) cross_value_kernel(gpx_kernel_params p, int n, const double* __restrict__ X,
                                                         int64_t ldx, const double* __restrict__ Sb, int64_t ldsb,
                                                         const double* __restrict__ Xb, int64_t ldxb,
                                                         const double* __restrict__ Xs, int64_t ldxs, int m, int nb,
                                                         double* __restrict__ cross) {
  __shared__ double xs[CROSS_CA][DMAX], xss[CROSS_CA][DMAX];  // the candidates, raw and divided by the lengthscales
  __shared__ double ks[CROSS_CA][WG];
  __shared__ double part[4][CROSS_CA][GPX_MAX_BASELINE];
  const int tid = threadIdx.x, g = tid >> 6, b = tid & 63;
  const int a0 = blockIdx.x * CROSS_CA;
  const int d = p.d;
  const bool lin = p.kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  if (tid < CROSS_CA * DMAX) {
    const int c = tid / DMAX, k = tid % DMAX;
    const double v = (k < d && a0 + c < m) ? Xs[(int64_t)(a0 + c) * ldxs + k] : 0.0;
    xs[c][k] = v;
    xss[c][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
  }
  __syncthreads();
  double acc[CROSS_CA];
#pragma unroll
  for (int c = 0; c < CROSS_CA; ++c) acc[c] = 0.0;
  for (int tile = 0; tile < n; tile += WG) {
    const int i = tile + tid;
    if (i < n) {
      double xi[DMAX], xis[DMAX];
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        xi[k] = (k < d) ? X[(int64_t)i * ldx + k] : 0.0;
        xis[k] = (k < d) ? xi[k] / p.lengthscale[k] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < CROSS_CA; ++c) {
        double r2 = 0.0, lv = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          if (k < d) {
            const double df = xis[k] - xss[c][k];
            r2 += df * df;
            if (lin) lv += xi[k] * p.linear_variance[k] * xs[c][k];
          }
        }
        ks[c][tid] = cov_from_r2(p.kind, p.outputscale, r2, lv);
      }
    }
    __syncthreads();
    if (b < nb) {
      const int cnt = min(WG, n - tile);
      for (int r = g; r < cnt; r += 4) {
        const double s = Sb[(int64_t)(tile + r) * ldsb + b];
#pragma unroll
        for (int c = 0; c < CROSS_CA; ++c) acc[c] += ks[c][r] * s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < CROSS_CA; ++c) part[g][c][b] = acc[c];
  __syncthreads();
  const int c = g;  // CROSS_CA == WG / 64: thread (c, b) finishes candidate a0 + c against baseline point b
  if (b >= nb || a0 + c >= m) return;
  double r2 = 0.0, lv = 0.0;
  for (int k = 0; k < d; ++k) {
    const double xb = Xb[(int64_t)b * ldxb + k];
    const double df = xb / p.lengthscale[k] - xss[c][k];
    r2 += df * df;
    if (lin) lv += xb * p.linear_variance[k] * xs[c][k];
  }
  const double sum = ((part[0][c][b] + part[1][c][b]) + part[2][c][b]) + part[3][c][b];
  cross[(int64_t)(a0 + c) * nb + b] = cov_from_r2(p.kind, p.outputscale, r2, lv) - sum;
}
static_assert(CROSS_CA == WG / 64, "cross_value_kernel finishes one candidate per wave");

hipError_t launch_cross_cov_grad(Context* c, const gpx_kernel_params& p, int n, const double* X, int64_t ldx,
                                 const double* Sb, int64_t ldsb, const double* Xb, int nb, int64_t ldxb,
                                 const double* Xs, int m, int64_t ldxs, double* cross, double* dcross) {
  const dim3 grid(nb, m);
  const unsigned vgrid = (unsigned)((m + CROSS_CA - 1) / CROSS_CA);
#define GPX_CC(D)                                                                                                      \
  do {                                                                                                                 \
    if (dcross)                                                                                                        \
      cross_cov_kernel<D><<<grid, WG, 0, c->stream>>>(p, n, X, ldx, Sb, ldsb, Xb, ldxb, Xs, ldxs, nb, cross, dcross); \
    else                                                                                                               \
      cross_value_kernel<D><<<vgrid, WG, 0, c->stream>>>(p, n, X, ldx, Sb, ldsb, Xb, ldxb, Xs, ldxs, m, nb, cross);   \
  } while (0)
  if (p.d <= 4)
    GPX_CC(4);
  else if (p.d <= 8)
    GPX_CC(8);
  else if (p.d <= 16)
    GPX_CC(16);
  else
    GPX_CC(32);
#undef GPX_CC
  return hipGetLastError();
}

}  // namespace gpx
