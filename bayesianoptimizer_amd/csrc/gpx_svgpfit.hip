// Closed-form SVGP variational posterior (gpx_svgp_fit_collapsed_f64): the optimum of the whitened
// q(u) = N(m, S) of optimization/Bayesian7.py's model under the full-batch ELBO, for given hyperparameters and inducing
// points Z (Titsias' collapsed posterior; Bayesian7.py:451-538 descends towards it with Adam).
//
// Per task, with W = L_ZZ^{-T} (upper) from the SVGP preparation's Gram / potrf / trtri, the training inputs are streamed
// in chunks of columns, PROJECT FIRST, THEN SQUARE (conjugating an accumulated K_ZX K_XZ with W afterwards would multiply
// its rounding by |W|^2 ~ 1 / jitter):
//  * svgp_project_kernel  Phi_chunk = W^T K(Z, X_chunk): trmm_sumsq_kernel's product (128 x 128 fp64-MFMA tiles,
//                         triangular k range, the hand-placed k loop of gpx_trmm_asm.h) with a store epilogue.  The rows
//                         are stored in REVERSED order (row i at Mpad - 1 - i) and columns beyond the chunk's points as 0.
//  * svgp_resid_kernel    r_chunk = y - const_mean, and the chunk's share of sum_i k(x_i, x_i) and r^T r.
//  * svgp_rhs_kernel      b_acc += Phi_chunk r_chunk (one wave per row).
//  * svgp_syrk_kernel     B_acc (lower 128-tiles) += Phi_chunk Phi_chunk^T, all tasks of the chunk in one launch (each
//                         task keeps its own projected chunk until then).
// Everything after the projection therefore lives in reversed index order: B' = J B J = I + Phi' Phi'^T / s2 is what
// launch_potrf factors (B' = L' L'^T) and launch_trtri inverts (W' = L'^{-T}, upper), and C = J W' J is LOWER triangular
// with C C^T = J B'^{-1} J = B^{-1}: the variational Cholesky factor without a second factorisation.  m = J W' (W'^T b').
// Padded rows of Phi are exactly 0 (K's padded rows are 0, W's padding is the identity), so B' carries an identity block
// in front and the padding never mixes with the model.
//
// Determinism: chunks and tasks run in stream order, each accumulator element is owned by one thread of one workgroup per
// launch, and every reduction has a fixed order; there are no floating-point atomics.
#include <algorithm>
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_trmm_asm.h"

namespace gpx {

using FitTile = MfmaTile<128, 128, 16, true, true>;  // (the accumulator layout and LDS size of both products)
static_assert(FitTile::LDS_DOUBLES * 8 == trmm_asm::LDS_BYTES, "hand-placed tile uses MfmaTile's LDS image");

// Phi'[Mpad - 1 - (128 I + m)][128 cb + c] = sum_{k < 128 (I + 1)} W[k][128 I + m] K[k][128 cb + c], 0 for columns >= mc
// FULL (gpx_svgp_condition_f64: W is the full W2 = W C): the sum over every k < Mpad.  A compile-time variant, so each
// kernel holds one k loop.
template <bool FULL>
__global__ void __launch_bounds__(WG) svgp_project_kernel(int Mpad, const double* __restrict__ W,
                                                          const double* __restrict__ kc, int64_t ldk, int ncb, int mc,
                                                          double* __restrict__ phi) {
  __shared__ __attribute__((aligned(16))) double smem[FitTile::LDS_DOUBLES];
  const int nI = Mpad / 128;
  const int I = nI - 1 - (int)blockIdx.x / ncb, cb = (int)blockIdx.x % ncb;  // deepest row tiles first
  // A(m, k) = W[k][128 I + m], B(k, c) = K[k][128 cb + c]; W's diagonal 128-block is the last 8 k-tiles (run_tri)
  trmm_asm::TileT<true, true, false, FULL ? 2 : 0> tile;
  tile.zero();
  if constexpr (FULL)
    tile.run(W + (int64_t)I * 128, Mpad, kc + (int64_t)cb * 128, ldk, nI * 8, smem);
  else
    tile.run_tri(W + (int64_t)I * 128, Mpad, kc + (int64_t)cb * 128, ldk, (I + 1) * 8, smem);
#pragma unroll
  for (int i = 0; i < FitTile::WM; ++i)
#pragma unroll
    for (int j = 0; j < FitTile::WN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I * 128 + FitTile::row_of(i, r), col = cb * 128 + FitTile::col_of(j);
        phi[(int64_t)(Mpad - 1 - row) * ldk + col] = col < mc ? tile.acc[i][j][r] : 0.0;
      }
}

// B_acc tile (I, J), J <= I, += Phi'[128 I ..][0 .. ncols) Phi'[128 J ..][0 .. ncols)^T (ncols a multiple of 128), for
// task blockIdx.y (strides sp / sb): the lower tiles alone are 136 workgroups at Mpad = 2048, half of the 256 CUs, so
// the tasks of a chunk share one launch (179.2 -> 150.1 ms for the whole fit at T = 8, n = 100000).
__global__ void __launch_bounds__(WG) svgp_syrk_kernel(int Mpad, const double* __restrict__ phi, int64_t sp, int64_t ldp,
                                                       int ncols, double* __restrict__ Bacc, int64_t sb) {
  __shared__ __attribute__((aligned(16))) double smem[FitTile::LDS_DOUBLES];
  phi += blockIdx.y * sp;
  Bacc += blockIdx.y * sb;
  int I, J;
  tri_decode((int)blockIdx.x, I, J);
  trmm_asm::TileT<false, false, false, 1> tile;
  tile.zero();
  tile.run(phi + (int64_t)I * 128 * ldp, ldp, phi + (int64_t)J * 128 * ldp, ldp, ncols / 16, smem);
  double* O = Bacc + (int64_t)I * 128 * Mpad + J * 128;
#pragma unroll
  for (int i = 0; i < FitTile::WM; ++i)
#pragma unroll
    for (int j = 0; j < FitTile::WN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* o = O + (int64_t)FitTile::row_of(i, r) * Mpad + FitTile::col_of(j);
        *o += tile.acc[i][j][r];
      }
}

// sum of v over the workgroup's threads in a fixed order (tree over LDS); result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// k(x, x) of gpx_device.h's covariance: outputscale for the stationary kinds, outputscale (sum_k v_k x_k^2 + 1) with
// the linear part
__device__ __forceinline__ double cov_diag(const gpx_kernel_params& p, const double* __restrict__ x) {
  if (p.kind != GPX_KERNEL_SCALE_LINEAR_MATERN52) return p.outputscale;
  double lv = 0.0;
  for (int k = 0; k < p.d; ++k) lv += x[k] * p.linear_variance[k] * x[k];
  return p.outputscale * (lv + 1.0);
}

// one workgroup: r[c] = y_c - const_mean for the chunk's mc points; scal[0] += sum k(x_c, x_c), scal[1] += r^T r
__global__ void __launch_bounds__(WG) svgp_resid_kernel(gpx_kernel_params p, const double* __restrict__ X, int64_t ldx,
                                                        const double* __restrict__ Y, int64_t ldy, int mc,
                                                        double* __restrict__ r, double* __restrict__ scal) {
  __shared__ double red[WG];
  double kd = 0.0, rr = 0.0;
  for (int c = threadIdx.x; c < mc; c += WG) {
    const double v = Y[(int64_t)c * ldy] - p.const_mean;
    r[c] = v;
    rr += v * v;
    kd += cov_diag(p, X + (int64_t)c * ldx);
  }
  const double skd = block_sum(kd, red);
  __syncthreads();
  const double srr = block_sum(rr, red);
  if (threadIdx.x == 0) {
    scal[0] += skd;
    scal[1] += srr;
  }
}

// b_acc[row] += sum_{c < mc} Phi'[row][c] r[c]: one wave per row, lanes stride the columns, xor-tree over the lanes
__global__ void __launch_bounds__(WG) svgp_rhs_kernel(int Mpad, const double* __restrict__ phi, int64_t ldp, int mc,
                                                      const double* __restrict__ r, double* __restrict__ bacc) {
  const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Mpad) return;
  const double* P = phi + (int64_t)row * ldp;
  double v = 0.0;
  for (int c = lane; c < mc; c += 64) v += P[c] * r[c];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) bacc[row] += v;
}

// scal[2] = tr Phi Phi^T = the diagonal sum of B_acc (one workgroup)
__global__ void __launch_bounds__(WG) svgp_trace_kernel(int Mpad, const double* __restrict__ Bacc,
                                                        double* __restrict__ scal) {
  __shared__ double red[WG];
  double v = 0.0;
  for (int i = threadIdx.x; i < Mpad; i += WG) v += Bacc[(int64_t)i * Mpad + i];
  const double s = block_sum(v, red);
  if (threadIdx.x == 0) scal[2] = s;
}

// B' = I + B_acc / s2 on the lower 128-tiles (in place), b' = b_acc / s2.  A task whose K_ZZ failed (info != 0) gets
// B' = I, b' = 0, so that the launches behind work on finite numbers.
__global__ void __launch_bounds__(WG) svgp_bfinal_kernel(int Mpad, double s2, const int32_t* __restrict__ info,
                                                         double* __restrict__ B, double* __restrict__ bvec) {
  const bool bad = *info != 0;
  const int64_t e0 = (int64_t)blockIdx.x * WG + threadIdx.x, tot = (int64_t)Mpad * Mpad;
  for (int64_t e = e0; e < tot; e += (int64_t)gridDim.x * WG) {
    const int i = (int)(e / Mpad), j = (int)(e % Mpad);
    if ((j >> 7) > (i >> 7)) continue;
    const double id = i == j ? 1.0 : 0.0;
    B[e] = bad ? id : id + B[e] / s2;
  }
  if (e0 < Mpad) bvec[e0] = bad ? 0.0 : bvec[e0] / s2;
}

// u[j] = sum_{i <= j} W'[i][j] b'[i] (= L'^{-1} b'): one thread per column, rows in ascending order
__global__ void __launch_bounds__(WG) svgp_utvec_kernel(int Mpad, const double* __restrict__ Wp, int64_t sw,
                                                        const double* __restrict__ bvec, double* __restrict__ u,
                                                        int64_t sv) {
  Wp += blockIdx.y * sw;
  bvec += blockIdx.y * sv;
  u += blockIdx.y * sv;
  const int j = (int)blockIdx.x * WG + threadIdx.x;
  if (j >= Mpad) return;
  double v = 0.0;
  for (int i = 0; i <= j; ++i) v += Wp[(int64_t)i * Mpad + j] * bvec[i];
  u[j] = v;
}

// vchol[i][j] = W'[Mpad-1-i][Mpad-1-j] for j <= i < M and exactly 0 above the diagonal; vmean[i] = m'[Mpad-1-i]; and,
// by workgroup 0, the bound and its terms.
__global__ void __launch_bounds__(WG) svgp_finish_kernel(int M, int Mpad, int64_t n, double s2,
                                                         const double* __restrict__ Lp, const double* __restrict__ Wp,
                                                         const double* __restrict__ u, const double* __restrict__ mrev,
                                                         const double* __restrict__ scal, double* __restrict__ vmean,
                                                         double* __restrict__ vchol, int64_t ldc,
                                                         double* __restrict__ bound) {
  __shared__ double red[WG];
  const int64_t e0 = (int64_t)blockIdx.x * WG + threadIdx.x, tot = (int64_t)M * M;
  for (int64_t e = e0; e < tot; e += (int64_t)gridDim.x * WG) {
    const int i = (int)(e / M), j = (int)(e % M);
    vchol[(int64_t)i * ldc + j] = j <= i ? Wp[(int64_t)(Mpad - 1 - i) * Mpad + (Mpad - 1 - j)] : 0.0;
  }
  if (e0 < M) vmean[e0] = mrev[Mpad - 1 - e0];
  if (blockIdx.x != 0) return;
  double ld = 0.0, uu = 0.0;
  for (int i = threadIdx.x; i < Mpad; i += WG) {
    ld += log(Lp[(int64_t)i * Mpad + i]);
    uu += u[i] * u[i];
  }
  const double sld = block_sum(ld, red);
  __syncthreads();
  const double suu = block_sum(uu, red);
  if (threadIdx.x == 0) {
    const double t1 = -0.5 * (double)n * log(6.283185307179586476925286766559 * s2);
    const double t2 = -sld;  // -(1/2) log|B| = -sum log L'_ii
    const double t3 = -0.5 * scal[1] / s2;
    const double t4 = 0.5 * suu;
    const double t5 = -0.5 * (scal[0] - scal[2]) / s2;
    bound[GPX_SVGP_BOUND_F] = t1 + t2 + t3 + t4 + t5;
    bound[GPX_SVGP_BOUND_CONST] = t1;
    bound[GPX_SVGP_BOUND_LOGDET] = t2;
    bound[GPX_SVGP_BOUND_QUAD] = t3;
    bound[GPX_SVGP_BOUND_FIT] = t4;
    bound[GPX_SVGP_BOUND_TRACE] = t5;
  }
}

// One chunk of one task behind its covariance build: kc = K(Z, X_chunk) (Mpad x ldk, columns 0 .. mc - 1 valid).
hipError_t launch_svgp_fit_project(Context* c, const gpx_kernel_params& p, int Mpad, const double* W, const double* kc,
                                   double* phi, int64_t ldk, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                                   int mc, double* r, double* bacc, double* scal) {
  const int nI = Mpad / 128, ncb = (mc + 127) / 128;
  svgp_project_kernel<false><<<nI * ncb, WG, 0, c->stream>>>(Mpad, W, kc, ldk, ncb, mc, phi);
  svgp_resid_kernel<<<1, WG, 0, c->stream>>>(p, X, ldx, Y, ldy, mc, r, scal);
  svgp_rhs_kernel<<<(Mpad + 3) / 4, WG, 0, c->stream>>>(Mpad, phi, ldk, mc, r, bacc);
  return hipGetLastError();
}

// The conditioning call's projection (gpx_svgpcond.hip): U' = the row-reversed W2^T K chunk, W2 full, and
// b_acc += U' e with the chunk's residual e (already formed).
hipError_t launch_svgp_cond_project(Context* c, int Mpad, const double* W2, const double* kc, double* phi, int64_t ldk,
                                    int mc, const double* e, double* bacc) {
  const int nI = Mpad / 128, ncb = (mc + 127) / 128;
  svgp_project_kernel<true><<<nI * ncb, WG, 0, c->stream>>>(Mpad, W2, kc, ldk, ncb, mc, phi);
  svgp_rhs_kernel<<<(Mpad + 3) / 4, WG, 0, c->stream>>>(Mpad, phi, ldk, mc, e, bacc);
  return hipGetLastError();
}

// The chunk's rank update of every task: B_acc_t += Phi'_t Phi'_t^T (task strides sp / sb)
hipError_t launch_svgp_fit_syrk(Context* c, int ntask, int Mpad, const double* phi, int64_t sp, int64_t ldk, int mc,
                                double* Bacc, int64_t sb) {
  const int nI = Mpad / 128, ncb = (mc + 127) / 128;
  svgp_syrk_kernel<<<dim3(nI * (nI + 1) / 2, ntask), WG, 0, c->stream>>>(Mpad, phi, sp, ldk, ncb * 128, Bacc, sb);
  return hipGetLastError();
}

hipError_t launch_svgp_fit_system(Context* c, int Mpad, double s2, const int32_t* info, double* B, double* bvec,
                                  double* scal) {
  svgp_trace_kernel<<<1, WG, 0, c->stream>>>(Mpad, B, scal);
  const int blocks = (int)std::min<int64_t>(((int64_t)Mpad * Mpad + WG - 1) / WG, 2048);
  svgp_bfinal_kernel<<<std::max(blocks, (Mpad + WG - 1) / WG), WG, 0, c->stream>>>(Mpad, s2, info, B, bvec);
  return hipGetLastError();
}

hipError_t launch_svgp_fit_utvec(Context* c, int ntask, int Mpad, const double* Wp, int64_t sw, const double* bvec,
                                 double* u, int64_t sv) {
  svgp_utvec_kernel<<<dim3((Mpad + WG - 1) / WG, ntask), WG, 0, c->stream>>>(Mpad, Wp, sw, bvec, u, sv);
  return hipGetLastError();
}

hipError_t launch_svgp_fit_finish(Context* c, int M, int Mpad, int64_t n, double s2, const double* Lp, const double* Wp,
                                  const double* u, const double* mrev, const double* scal, double* vmean, double* vchol,
                                  int64_t ldc, double* bound) {
  const int blocks = (int)std::min<int64_t>(((int64_t)M * M + WG - 1) / WG, 2048);
  svgp_finish_kernel<<<blocks, WG, 0, c->stream>>>(M, Mpad, n, s2, Lp, Wp, u, mrev, scal, vmean, vchol, ldc, bound);
  return hipGetLastError();
}

// The bound alone (gpx_svgp_bound_grad_f64): svgp_finish_kernel's workgroup 0 with no rows of vmean / vchol to write,
// so the same arithmetic and the same bits as the fit's.
hipError_t launch_svgp_fit_bound(Context* c, int Mpad, int64_t n, double s2, const double* Lp, const double* u,
                                 const double* scal, double* bound) {
  svgp_finish_kernel<<<1, WG, 0, c->stream>>>(0, Mpad, n, s2, Lp, nullptr, u, nullptr, scal, nullptr, nullptr, 0, bound);
  return hipGetLastError();
}

}  // namespace gpx
