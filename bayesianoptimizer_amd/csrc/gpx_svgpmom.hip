// Posterior moments of q-batches of candidates under one task of an SVGP, and their derivatives w.r.t. the candidate
// inputs: what gpx_moments_grad_f64 (gpx_grad.hip) is to the exact GP, for the whitened variational posterior that
// gpx_svgp_prepare_f64 caches (optimize_acqf on the per-output SVGPs of optimization/Bayesian6.py:492-577, 896-919).
// With K_ZZ + jitter I = L L^T, W = L^{-T}, S = tril(chol_variational_covar), W2 = W S, alpha' = W m and
// k_a = K(Z, x_a), for candidates x_a (rows of Xs, consecutive q-batches) and c in a's batch:
//   v_c = W^T k_c,  u_c = W2^T k_c (= S^T v_c),  h_c = W v_c - W2 u_c        (= L^{-T} (I - S S^T) L^{-1} k_c)
//   mean[a]   = m + k_a^T alpha'                  dmean[a][j]   = sum_i d1k(x_a, z_i)/dx_aj alpha'_i
//   cov[a][c] = k(x_a, x_c) - k_a^T h_c           dcov[a][j][c] = d1k(x_a, x_c)/dx_aj - sum_i d1k(x_a, z_i)/dx_aj h_c[i]
// with d1k the partial derivative in the kernel's FIRST argument.  W (I - S S^T) W^T is symmetric, so the chain rule of
// gpx_grad.hip holds unchanged.  K* is projected first and contracted afterwards (four fp64-MFMA products over
// Mpad x mpad, gpx_gemm.h); W (I - S S^T) W^T is never formed, and nothing assumes S S^T <= I.  The covariance is the
// latent one: no likelihood noise, no variance floor.
//
// Workspace (doubles, mpad = m rounded up to 64, blk = Mpad * mpad):
//   [0, blk)        K* = K(Z, Xs), then H (K* is dead once V and U exist)
//   [blk, 2 blk)    V = W^T K*
//   [2 blk, 3 blk)  U = W2^T K*
//   [3 blk, ...)    the products' split-K partials (gemm_split_doubles(Mpad, mpad, Mpad))
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_gemm.h"

namespace gpx {

// One workgroup per candidate a.  Tile by tile over the inducing points: thread t evaluates k and d1k of its point
// z_{tile + t} against x_a once into LDS; then thread (g = t / 64, cc = t % 64) adds the tile's rows r = g, g + 4, ...
// times column cc of [H(:, batch) | alpha'] (cc < q: batch member cc; cc == q: the mean's column) into its 1 + d
// accumulators.  The four partial sums per (a, cc) are added in a fixed order.  GRAD = false: the values only, by the
// same operations in the same order, so mean and cov have the bits of the GRAD = true instantiation.
template <int DMAX, bool GRAD>
__global__ void __launch_bounds__(WG) svgp_moments_kernel(gpx_kernel_params p, int M, const double* __restrict__ Z,
                                                          int64_t ldz, const double* __restrict__ alpha,
                                                          const double* __restrict__ Xs, int64_t ldxs, int q,
                                                          const double* __restrict__ H, int mpad,
                                                          double* __restrict__ mean, double* __restrict__ dmean,
                                                          double* __restrict__ cov, double* __restrict__ dcov) {
  constexpr int CNT = GRAD ? DMAX + 1 : 1;  // values per (point, candidate): k, then d1k
  constexpr int COLS = GPX_MAX_Q + 1;       // column slots: the batch, then alpha'
  static_assert(COLS <= 64, "one column slot per lane");
  static_assert(4 * CNT * COLS <= CNT * WG, "the partial sums reuse the tile's LDS");
  __shared__ double xa[DMAX];
  __shared__ double ks[CNT * WG];  // ks[k * WG + r]; after the last tile: part[(g * CNT + k) * COLS + cc]
  const int tid = threadIdx.x, g = tid >> 6, cc = tid & 63;
  const int a = blockIdx.x;
  const int batch0 = (a / q) * q;
  const int d = p.d;
  if (tid < DMAX) xa[tid] = (tid < d) ? Xs[(int64_t)a * ldxs + tid] : 0.0;
  __syncthreads();
  double acc[CNT];
#pragma unroll
  for (int k = 0; k < CNT; ++k) acc[k] = 0.0;
  for (int tile = 0; tile < M; tile += WG) {
    const int i = tile + tid;
    if (i < M) {
      double zi[DMAX], gk[DMAX];
#pragma unroll
      for (int k = 0; k < DMAX; ++k) zi[k] = (k < d) ? Z[(int64_t)i * ldz + k] : 0.0;
      ks[tid] = cov_and_grad<DMAX>(p, xa, zi, gk);
      if constexpr (GRAD) {
#pragma unroll
        for (int k = 0; k < DMAX; ++k) ks[(1 + k) * WG + tid] = gk[k];
      }
    }
    __syncthreads();
    if (cc <= q) {
      const int cnt = min(WG, M - tile);
      for (int r = g; r < cnt; r += 4) {
        const double s = (cc < q) ? H[(int64_t)(tile + r) * mpad + batch0 + cc] : alpha[tile + r];
        acc[0] += ks[r] * s;
        if constexpr (GRAD) {
#pragma unroll
          for (int k = 1; k < CNT; ++k)
            if (k <= d) acc[k] += ks[k * WG + r] * s;
        }
      }
    }
    __syncthreads();
  }
  if (cc <= q) {
#pragma unroll
    for (int k = 0; k < CNT; ++k) ks[(g * CNT + k) * COLS + cc] = acc[k];
  }
  __syncthreads();
  if (g != 0 || cc > q) return;
  double sum[CNT];
#pragma unroll
  for (int k = 0; k < CNT; ++k)
    sum[k] = ((ks[k * COLS + cc] + ks[(CNT + k) * COLS + cc]) + ks[(2 * CNT + k) * COLS + cc]) +
             ks[(3 * CNT + k) * COLS + cc];
  if (cc == q) {
    mean[a] = p.const_mean + sum[0];
    if constexpr (GRAD) {
#pragma unroll
      for (int k = 1; k < CNT; ++k)
        if (k <= d) dmean[(int64_t)a * d + k - 1] = sum[k];
    }
    return;
  }
  double xc[DMAX], gp[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) xc[k] = (k < d) ? Xs[(int64_t)(batch0 + cc) * ldxs + k] : 0.0;
  const double kac = cov_and_grad<DMAX>(p, xa, xc, gp);
  {
    // k(x_a, x_c) rounded, then the difference: left to contract, the value-only instantiation (k has no other use
    // there) would fuse the outputscale's product into the subtraction and the gradient instantiation would not
#pragma clang fp contract(off)
    cov[(int64_t)a * q + cc] = kac - sum[0];
  }
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 1; k < CNT; ++k)
      if (k <= d) dcov[((int64_t)a * d + k - 1) * q + cc] = gp[k - 1] - sum[k];
  }
}

size_t svgp_moments_ws_doubles(int Mpad, int m) {
  const int mpad = ((m + NB - 1) / NB) * NB;
  return 3 * (size_t)Mpad * mpad + gemm_split_doubles(Mpad, mpad, Mpad) + 64;
}

hipError_t launch_svgp_moments(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                               const double* W, const double* W2, const double* alpha, const double* Xs, int64_t ldxs,
                               int m, int q, double* mean, double* dmean, double* cov, double* dcov, double* ws) {
  const int mpad = ((m + NB - 1) / NB) * NB;
  const size_t blk = (size_t)Mpad * mpad;
  double* Ks = ws;
  double* V = Ks + blk;
  double* U = V + blk;
  double* P = U + blk;
  double* H = Ks;
  const int64_t tot = (int64_t)Mpad * mpad;
  kstar_plain_kernel<<<(unsigned)((tot + WG - 1) / WG), WG, 0, c->stream>>>(p, M, Mpad, m, mpad, Z, ldz, Xs, ldxs, Ks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // V = W^T K*  (A(r, k) = W[k][r], nonzero for k <= r)
  e = launch_gemm64<true, true, KR_A_LOWER>(c, Mpad, mpad, Mpad, W, Mpad, Ks, mpad, nullptr, 0, V, mpad, 1.0, 0, P);
  if (e != hipSuccess) return e;
  // U = W2^T K*  (W2 = W S is full)
  e = launch_gemm64<true, true, KR_FULL>(c, Mpad, mpad, Mpad, W2, Mpad, Ks, mpad, nullptr, 0, U, mpad, 1.0, 0, P);
  if (e != hipSuccess) return e;
  // H = W V  (A(r, k) = W[r][k], nonzero for k >= r), over K*; then H -= W2 U, each element read and written by one thread
  e = launch_gemm64<false, true, KR_A_UPPER>(c, Mpad, mpad, Mpad, W, Mpad, V, mpad, nullptr, 0, H, mpad, 1.0, 0, P);
  if (e != hipSuccess) return e;
  e = launch_gemm64<false, true, KR_FULL>(c, Mpad, mpad, Mpad, W2, Mpad, U, mpad, H, mpad, H, mpad, -1.0, 0, P);
  if (e != hipSuccess) return e;
  const bool grad = dmean != nullptr;
  with_dmax(p.d, [&](auto D) {
    constexpr int DM = decltype(D)::value;
    if (grad)
      svgp_moments_kernel<DM, true><<<m, WG, 0, c->stream>>>(p, M, Z, ldz, alpha, Xs, ldxs, q, H, mpad, mean, dmean, cov,
                                                             dcov);
    else
      svgp_moments_kernel<DM, false><<<m, WG, 0, c->stream>>>(p, M, Z, ldz, alpha, Xs, ldxs, q, H, mpad, mean, nullptr,
                                                              cov, nullptr);
  });
  return hipGetLastError();
}

}  // namespace gpx
