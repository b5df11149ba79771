// Conditioning the sparse model on new data (gpx_svgp_condition_f64): the exact Bayesian update of a task's
// whitened q(u) = N(m, C C^T) by Gaussian observations (X_n, y_n), in the basis of the current posterior u = m + C u~:
//   U = C^T Phi_n = W2^T K(Z, X_n)              (W2 = W C, the block the preparation stores)
//   e = y_n - (const_mean + K(Z, X_n)^T alpha')  (the residual against the current predictive mean)
//   P = I + U U^T / s2,  D lower with D D^T = P^-1,  g = D D^T U e / s2
//   m_new = m + C g,  C_new = C D,  W2_new = W2 D,  alpha'_new = alpha' + W2 g.
// From P on this is the collapsed fit's own system (gpx_svgpfit.hip) with U in Phi's place: the chunks of X_n go through
// the fit's covariance build (with the task's alpha', whose mean partials give e), svgp_project_kernel's full-range
// variant, the fit's rank update and the fit's tail (B' = I + ./s2, launch_potrf, launch_trtri, u, m'), all in reversed
// index order: the workspace then holds W' = L'^{-T} (upper) and m' with D = J W' J and g = J m'.
//
//  * svgp_cond_resid_kernel   e_chunk from the build's mean partials, summed in ascending block order.
//  * svgp_compose_kernel      Out = A D on fp64 MFMA, 128 x 128 tiles, D never materialised: in reversed indices
//                             Out[i][R - j'] = sum_{k' <= j'} A[i][R - k'] W'[k'][j'] (R = Mpad - 1), i.e. W' is the
//                             k-major right operand as it lies and A is read DOWN its rows (gpx_trmm_asm.h's reversed
//                             row-major operand); the epilogue mirrors the columns.  A = W2 (full) gives W2_out, A = the
//                             zero-padded tril(vchol) gives vchol_out.
//  * svgp_cond_finish_kernel  alpha'_new and m_new: one wave per row, lanes stride the columns, xor-tree over the lanes.
//  * svgp_cond_check_kernel   a task whose update is not finite (non-finite Y_n: P itself stays finite) gets info > 0.
//
// Determinism: as the fit's; every output element is owned by one thread and every reduction has a fixed order.
#include <algorithm>
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_trmm_asm.h"

namespace gpx {

using ComposeTile = MfmaTile<128, 128, 16, false, true>;  // (the accumulator layout and LDS size)
static_assert(ComposeTile::LDS_DOUBLES * 8 == trmm_asm::LDS_BYTES, "hand-placed tile uses MfmaTile's LDS image");

// e[c] = Y[c] - (const_mean + sum_jb mu[jb][c]) for the chunk's mc points (mu: the covariance build's mean partials of
// the task's alpha', nJB rows of ldk)
__global__ void __launch_bounds__(WG) svgp_cond_resid_kernel(double const_mean, const double* __restrict__ Y,
                                                             int64_t ldy, int mc, const double* __restrict__ mu,
                                                             int64_t ldk, int nJB, double* __restrict__ e) {
  const int c = (int)blockIdx.x * WG + threadIdx.x;
  if (c >= mc) return;
  double s = 0.0;
  for (int jb = 0; jb < nJB; ++jb) s += mu[(int64_t)jb * ldk + c];
  e[c] = Y[(int64_t)c * ldy] - (s + const_mean);
}

// spad = tril(vchol) zero-padded to Mpad x Mpad, per task (grid y): svgp_pad_kernel's matrix half
__global__ void __launch_bounds__(WG) svgp_cond_pad_kernel(int M, int Mpad, const double* __restrict__ vchol,
                                                           int64_t ldc, int64_t stride_c, double* __restrict__ spad,
                                                           int64_t sdst) {
  const double* V = vchol + blockIdx.y * stride_c;
  double* S = spad + blockIdx.y * sdst;
  const int64_t tot = (int64_t)Mpad * Mpad;
  for (int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x; e < tot; e += (int64_t)gridDim.x * WG) {
    const int i = (int)(e / Mpad), j = (int)(e % Mpad);
    S[e] = (i < M && j <= i) ? V[(int64_t)i * ldc + j] : 0.0;
  }
}

// Out[128 I + m][j] = sum_{k >= j} A[128 I + m][k] D[k][j], D[k][j] = W'[R - k][R - j], for the column tile J of j and
// task blockIdx.y (strides sa / sw / so doubles).  In reversed indices k' = R - k, j' = R - j the column tile is
// Jr = nT - 1 - J and k' runs over [k0, 128 (Jr + 1)): k0 = 0 for a full A; for a lower-triangular A (tri) row tile I
// is zero for k > 128 I + 127, so k0 = 128 (nT - 1 - I), and a tile above the diagonal (J > I) is all zero.
// The store: rows and columns >= M as exact zeros (full: the prepared blocks' padding) or not at all (tri: out is
// M x M with rows ldo apart, and the strict upper triangle is written as exactly 0).
__global__ void __launch_bounds__(WG) svgp_compose_kernel(int M, int Mpad, const double* __restrict__ A, int64_t sa,
                                                          const double* __restrict__ Wp, int64_t sw,
                                                          double* __restrict__ out, int64_t ldo, int64_t so, int tri) {
  __shared__ __attribute__((aligned(16))) double smem[ComposeTile::LDS_DOUBLES];
  const int nT = Mpad / 128;
  const int Jr = nT - 1 - (int)blockIdx.x / nT, I = (int)blockIdx.x % nT;  // the longest k ranges first
  A += blockIdx.y * sa;
  Wp += blockIdx.y * sw;
  out += blockIdx.y * so;
  const int k0 = tri ? (nT - 1 - I) * 128 : 0, k1 = (Jr + 1) * 128;
  // A(m, k') = A[128 I + m][R - k0 - k'] (row-major, read down the row from k-tile 0's lowest address),
  // B(k', n) = W'[k0 + k'][128 Jr + n] (k-major)
  trmm_asm::TileT<false, true, false, 0, true> tile;
  tile.zero();
  if (k1 > k0)
    tile.run(A + (int64_t)I * 128 * Mpad + (Mpad - 16 - k0), Mpad, Wp + (int64_t)k0 * Mpad + Jr * 128, Mpad,
             (k1 - k0) / 16, smem);
#pragma unroll
  for (int i = 0; i < ComposeTile::WM; ++i)
#pragma unroll
    for (int j = 0; j < ComposeTile::WN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I * 128 + ComposeTile::row_of(i, r), col = Mpad - 1 - (Jr * 128 + ComposeTile::col_of(j));
        const bool in = row < M && col < M;
        if (tri) {
          if (in) out[(int64_t)row * ldo + col] = col <= row ? tile.acc[i][j][r] : 0.0;
        } else {
          out[(int64_t)row * ldo + col] = in ? tile.acc[i][j][r] : 0.0;
        }
      }
}

// Row `row` of task blockIdx.y, one wave each, g[j] = mrev[Mpad - 1 - j]:
//   alpha_out[row] = alpha[row] + sum_j W2[row][j] g[j] for row < M, 0 for the padding;
//   vmean_out[row] = vmean[row] + sum_{j <= row} vchol[row][j] g[j] for row < M (vchol: null = not wanted).
__global__ void __launch_bounds__(WG) svgp_cond_finish_kernel(int M, int Mpad, const double* __restrict__ W2,
                                                              const double* __restrict__ alpha,
                                                              const double* __restrict__ mrev, int64_t smrev,
                                                              double* __restrict__ alpha_out,
                                                              const double* __restrict__ vmean, int64_t stride_m,
                                                              const double* __restrict__ vchol, int64_t ldc,
                                                              int64_t stride_c, double* __restrict__ vmean_out) {
  const int t = blockIdx.y, row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Mpad) return;
  const double* g = mrev + t * smrev + (Mpad - 1);  // g[j] = g[-j] of this pointer
  if (row >= M) {
    if (lane == 0) alpha_out[(int64_t)t * Mpad + row] = 0.0;
    return;
  }
  const double* P = W2 + ((int64_t)t * Mpad + row) * Mpad;
  double v = 0.0;
  for (int j = lane; j < M; j += 64) v += P[j] * g[-j];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) alpha_out[(int64_t)t * Mpad + row] = alpha[(int64_t)t * Mpad + row] + v;
  if (!vchol) return;
  const double* Cr = vchol + t * stride_c + (int64_t)row * ldc;
  double s = 0.0;
  for (int j = lane; j <= row; j += 64) s += Cr[j] * g[-j];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) vmean_out[t * stride_m + row] = vmean[t * stride_m + row] + s;
}

// One workgroup per task: if the factorisation went through (info == 0) but m' is not finite, info = 1 + the lowest
// index (in the caller's order) of a non-finite entry of g.
__global__ void __launch_bounds__(WG) svgp_cond_check_kernel(int Mpad, const double* __restrict__ mrev, int64_t smrev,
                                                             int32_t* __restrict__ info) {
  __shared__ int red[WG];
  const double* g = mrev + blockIdx.x * smrev + (Mpad - 1);
  int first = Mpad;
  for (int j = threadIdx.x; j < Mpad; j += WG)
    if (!isfinite(g[-j]) && j < first) first = j;
  red[threadIdx.x] = first;
  __syncthreads();
  for (int s = WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0] < Mpad && info[blockIdx.x] == 0) info[blockIdx.x] = red[0] + 1;
}

hipError_t launch_svgp_cond_resid(Context* c, double const_mean, const double* Y, int64_t ldy, int mc, const double* mu,
                                  int64_t ldk, int nJB, double* e) {
  svgp_cond_resid_kernel<<<(mc + WG - 1) / WG, WG, 0, c->stream>>>(const_mean, Y, ldy, mc, mu, ldk, nJB, e);
  return hipGetLastError();
}

hipError_t launch_svgp_cond_pad(Context* c, int ntask, int M, int Mpad, const double* vchol, int64_t ldc,
                                int64_t stride_c, double* spad, int64_t sdst) {
  const int blocks = (int)std::min<int64_t>(((int64_t)Mpad * Mpad + WG - 1) / WG, 2048);
  svgp_cond_pad_kernel<<<dim3(blocks, ntask), WG, 0, c->stream>>>(M, Mpad, vchol, ldc, stride_c, spad, sdst);
  return hipGetLastError();
}

hipError_t launch_svgp_compose(Context* c, int ntask, int M, int Mpad, const double* A, int64_t sa, const double* Wp,
                               int64_t sw, double* out, int64_t ldo, int64_t so, bool tri) {
  const int nT = Mpad / 128;
  svgp_compose_kernel<<<dim3(nT * nT, ntask), WG, 0, c->stream>>>(M, Mpad, A, sa, Wp, sw, out, ldo, so, tri ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_svgp_cond_finish(Context* c, int ntask, int M, int Mpad, const double* W2, const double* alpha,
                                   const double* mrev, int64_t smrev, double* alpha_out, const double* vmean,
                                   int64_t stride_m, const double* vchol, int64_t ldc, int64_t stride_c,
                                   double* vmean_out, int32_t* info) {
  svgp_cond_finish_kernel<<<dim3((Mpad + 3) / 4, ntask), WG, 0, c->stream>>>(
      M, Mpad, W2, alpha, mrev, smrev, alpha_out, vmean, stride_m, vchol, ldc, stride_c, vmean_out);
  svgp_cond_check_kernel<<<ntask, WG, 0, c->stream>>>(Mpad, mrev, smrev, info);
  return hipGetLastError();
}

}  // namespace gpx
