// Hyperparameter gradient of the collapsed SVGP bound (gpx_svgp_bound_grad_f64): F(theta) of gpx_svgpfit.hip
// with q(u) = N(m, S) already maximised out, differentiated with respect to the likelihood noise, the constant mean and
// the kernel's parameters.  An evaluation is the fit (pass 1, gpx_svgpfit.hip, with W = L_ZZ^{-T} and B' kept) and a
// second pass over X; S and m are known only after the first.  Per task, with r = y - c, s2 = noise, c_v = W m and
// e = r - K_u^T c_v (K_u = K(Z, X)):
//   dF/dK_u = G_u = (H K_u + c_v e^T) / s2,   H = A^{-1} - Sigma^{-1} = W (I - S) W^T          (M x n, never stored)
//   dF/dA   = G_A = W (2I - S - B - m m^T) W^T / 2                                             (M x M)
//   dF/dk(x_i, x_i) = -1 / (2 s2),   dF/dc = sum_i e_i / s2
//   dF/ds2  = -n / (2 s2) + (M - tr S) / (2 s2) + e^T e / (2 s2^2) + (sum_i k(x_i, x_i) - tr Phi Phi^T) / (2 s2^2)
//   dF/dtheta = sum G_u dK_u/dtheta + sum G_A dK_ZZ/dtheta - sum_i dk(x_i, x_i)/dtheta / (2 s2)
//
// Between the passes (O(M^3) per task, all tasks of a step in one launch; svgp_mm_kernel, a full 128 x 128 fp64-MFMA tile
// product C = A B^T of row-major operands whose k range starts at the triangular operand's first non-zero tile):
//   S' = W' W'^T lives in the fit's REVERSED index order (J . J); its epilogue un-reverses it on the way out, as
//   T1 = I - S and Q = 2I - S - B - m m^T in natural order.  Padding: B' carries an identity block there and m' is 0,
//   so T1's and Q's padded rows and columns are exactly 0, and so are H's and G_A's.
//   U = W T1, H = U W^T;  U = W Q, G_A = U W^T / 2  (T1 and Q are symmetric: read as their own transposes).
//   svgp_kzz_kernel contracts the materialised G_A with dK_ZZ/dtheta element by element (it is not the hot path).
// Pass 2, per chunk of columns and task: K(Z, X_chunk) again through launch_svgp_kchunk, whose mean partials with c_v as
// its "alpha" give K_chunk^T c_v, hence e (svgp_echunk_kernel, svgp_esum_kernel); svgp_grad_kernel forms one 128 x 128 tile of H K_chunk
// over all of Mpad on the MFMA and contracts G = (acc + c_v[a] e[i]) / s2 against dk(z_a, x_i)/dtheta recomputed from
// the tile's rows of Z and X in LDS: mll_grad_kernel's epilogue without its symmetry weights.  One partial row per
// workgroup, added in a fixed order by svgp_partsum_kernel into the task's accumulator row.
//
// Determinism as in the fit: chunks and tasks in stream order, one owner per accumulator element and launch, fixed-order
// reductions, no floating-point atomics.
#include <algorithm>
#include "gpx_internal.h"
#include "gpx_device.h"
#include "gpx_trmm_asm.h"

namespace gpx {

namespace {

using GTile = MfmaTile<128, 128, 16, true, true>;  // (the accumulator layout and LDS size of every product here)
static_assert(GTile::LDS_DOUBLES * 8 == trmm_asm::LDS_BYTES, "hand-placed tile uses MfmaTile's LDS image");
constexpr int MT = 128;
constexpr double SQRT5 = 2.23606797749978969640917366873128;
constexpr int NROW = GPX_MLL_NOUT;  // partial rows use the GPX_MLL_D_* slots

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// The running sums of a workgroup's contraction: gs (outputscale), gl[k] (lengthscales, still to be divided by l_k),
// gv[k] (linear variances, still to be multiplied by the outputscale).
template <int DMAX>
struct DkSums {
  double gs, gl[DMAX], gv[DMAX];
  __device__ __forceinline__ void zero() {
    gs = 0.0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) gl[k] = gv[k] = 0.0;
  }
};

// sums += G dk(x1, x2)/dtheta for one pair of points (rows of DMAX doubles, zero beyond d): mll_grad_kernel's element.
// KIND >= 0 is compile-time; KIND < 0 reads the kind at run time (the Scale(Linear + Matern) instantiation).
// Returns G kfac, the factor of -(x1_k - x2_k) / l_k^2 in G d1 k(x1, x2)_k (the inducing-location gradient's element).
template <int DMAX, int KIND>
__device__ __forceinline__ double dk_add(const gpx_kernel_params& p, int kind, const double (&il)[DMAX], double G,
                                         const double* __restrict__ x1, const double* __restrict__ x2,
                                         DkSums<DMAX>& a) {
  const int d = p.d;
  const bool lin = kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  double q[DMAX];
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    q[k] = 0.0;
    if (KIND >= 0 || k < d) {
      const double df = (x1[k] - x2[k]) * il[k];
      q[k] = df * df;
      r2 += q[k];
    }
  }
  double base, kfac;  // base = dk/d outputscale; kfac q_k / l_k = dk/dl_k
  if (kind == GPX_KERNEL_RBF) {
    base = exp(-0.5 * r2);
    kfac = p.outputscale * base;
  } else {
    const double rr = sqrt(r2);
    const double ex = exp(-SQRT5 * rr);
    base = (1.0 + SQRT5 * rr + (5.0 / 3.0) * r2) * ex;
    kfac = p.outputscale * (5.0 / 3.0) * (1.0 + SQRT5 * rr) * ex;
  }
  if (lin) {
    double lv = 0.0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
      if (k < d) {
        const double xx = x1[k] * x2[k];
        lv += p.linear_variance[k] * xx;
        a.gv[k] += G * xx;
      }
    }
    base += lv;
  }
  a.gs += G * base;
  const double gk = G * kfac;
#pragma unroll
  for (int k = 0; k < DMAX; ++k) a.gl[k] += gk * q[k];
  return gk;
}

// The inducing-location gradient (gpx_svgp_bound_grad_z_f64).  With G = dF/dk(z_a, x) for one pair of points,
//   G d1 k(z_a, x)_k = -il_k^2 [ (G kfac) (z_ak - x_k) + G cz_k x_k ],   cz_k = -outputscale v_k l_k^2 (linear kind; else 0)
// so a row's running sum gz[k] takes two FMAs per pair and dimension (one without the linear part) and is multiplied by
// -il_k^2 once, when the row leaves the workgroup.
template <int DMAX>
__device__ __forceinline__ void dz_consts(const gpx_kernel_params& p, bool lin, double (&cz)[DMAX]) {
#pragma unroll
  for (int k = 0; k < DMAX; ++k)
    cz[k] = (lin && k < p.d) ? -(p.outputscale * p.linear_variance[k]) * (p.lengthscale[k] * p.lengthscale[k]) : 0.0;
}

// The two column halves of a row (threads row and 128 + row) joined in a fixed order through LDS (buf: 128 x (DMAX + 1)
// doubles, free to overwrite), scaled, into dst[row][DMAX] (k >= d: 0).  Every thread of the workgroup calls it.
template <int DMAX>
__device__ __forceinline__ void dz_store(const gpx_kernel_params& p, const double (&gz)[DMAX], double scale,
                                         double* buf, double* __restrict__ dst) {
  constexpr int XP = DMAX + 1;
  const int row = threadIdx.x & (MT - 1), hh = threadIdx.x >> 7;
  if (hh == 1) {
#pragma unroll
    for (int k = 0; k < DMAX; ++k) buf[row * XP + k] = gz[k];
  }
  __syncthreads();
  if (hh == 0) {
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
      const double il = (k < p.d) ? 1.0 / p.lengthscale[k] : 0.0;
      dst[row * DMAX + k] = -scale * (il * il) * (gz[k] + buf[row * XP + k]);
    }
  }
  __syncthreads();
}

// the workgroup's sums, in a fixed order, into one partial row (red: 4 x NROW doubles of LDS, free to overwrite)
template <int DMAX>
__device__ __forceinline__ void dk_store(const gpx_kernel_params& p, int kind, const double (&il)[DMAX],
                                         const DkSums<DMAX>& a, double* red, double* __restrict__ dst) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = p.d;
  const bool lin = kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  auto put = [&](int slot, double v) {
    v = wave_sum(v);
    if (lane == 0) red[w * NROW + slot] = v;
  };
  put(GPX_MLL_D_OUTPUTSCALE, a.gs);
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    if (k < d) {
      put(GPX_MLL_D_LENGTHSCALE + k, a.gl[k] * il[k]);
      if (lin) put(GPX_MLL_D_LINVAR + k, a.gv[k] * p.outputscale);
    }
  }
  __syncthreads();
  for (int o = threadIdx.x; o < NROW; o += WG) {
    const bool used = o == GPX_MLL_D_OUTPUTSCALE || (o >= GPX_MLL_D_LENGTHSCALE && o < GPX_MLL_D_LENGTHSCALE + d) ||
                      (lin && o >= GPX_MLL_D_LINVAR && o < GPX_MLL_D_LINVAR + d);
    dst[o] = used ? ((red[o] + red[NROW + o]) + (red[2 * NROW + o] + red[3 * NROW + o])) : 0.0;
  }
}

}  // namespace

// C tile (I, J) = sum_{k >= kbeg} A[128 I + m][k] B[128 J + n][k] (row-major Mpad x Mpad operands of task blockIdx.y,
// task stride ts for every array), kbeg = 128 max(I, J) / 128 I / 128 J for kmode 0 / 1 / 2: the first k-tile in which
// the upper-triangular operand(s) are non-zero.  emode 0: out1 = scale C.  emode 1 (C = S' in reversed order):
// out1[P-1-i][P-1-j] = delta - C (T1 = I - S), out2[P-1-i][P-1-j] = 2 delta - C - B'[i][j] - m'[i] m'[j] (Q), with B'
// read from its lower 128-tiles.
__global__ void __launch_bounds__(WG) svgp_mm_kernel(int P, int64_t ts, const double* __restrict__ A,
                                                     const double* __restrict__ B, int kmode, int emode, double scale,
                                                     double* __restrict__ out1, double* __restrict__ out2,
                                                     const double* __restrict__ Bp, const double* __restrict__ mrev) {
  __shared__ __attribute__((aligned(16))) double smem[GTile::LDS_DOUBLES];
  const int nI = P / MT;
  const int I = (int)blockIdx.x / nI, J = (int)blockIdx.x % nI;
  const int64_t off = (int64_t)blockIdx.y * ts;
  A += off;
  B += off;
  out1 += off;
  const int kbeg = MT * (kmode == 0 ? max(I, J) : kmode == 1 ? I : J);
  trmm_asm::TileT<false, false, false, 1> tile;
  tile.zero();
  tile.run(A + (int64_t)I * MT * P + kbeg, P, B + (int64_t)J * MT * P + kbeg, P, (P - kbeg) / 16, smem);
  if (emode == 0) {
#pragma unroll
    for (int i = 0; i < GTile::WM; ++i)
#pragma unroll
      for (int j = 0; j < GTile::WN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = I * MT + GTile::row_of(i, r), col = J * MT + GTile::col_of(j);
          out1[(int64_t)row * P + col] = scale * tile.acc[i][j][r];
        }
    return;
  }
  out2 += off;
  Bp += off;
  mrev += off;
#pragma unroll
  for (int i = 0; i < GTile::WM; ++i)
#pragma unroll
    for (int j = 0; j < GTile::WN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = I * MT + GTile::row_of(i, r), col = J * MT + GTile::col_of(j);
        const double dl = row == col ? 1.0 : 0.0, s = tile.acc[i][j][r];
        const double b = I >= J ? Bp[(int64_t)row * P + col] : Bp[(int64_t)col * P + row];
        const int64_t o = (int64_t)(P - 1 - row) * P + (P - 1 - col);
        out1[o] = dl - s;
        out2[o] = 2.0 * dl - s - b - mrev[row] * mrev[col];
      }
}

// One workgroup per task: m in natural order (mnat[i] = m'[P - 1 - i]) and sc2[2] = tr T1 = M - tr S.
__global__ void __launch_bounds__(WG) svgp_unreverse_kernel(int P, int64_t ts, const double* __restrict__ mrev,
                                                            const double* __restrict__ T1, double* __restrict__ mnat,
                                                            double* __restrict__ sc2) {
  __shared__ double red[WG];
  const int64_t off = (int64_t)blockIdx.x * ts;
  double tr = 0.0;
  for (int i = threadIdx.x; i < P; i += WG) {
    mnat[off + i] = mrev[off + P - 1 - i];
    tr += T1[off + (int64_t)i * P + i];
  }
  const double s = block_sum(tr, red);
  if (threadIdx.x == 0) sc2[off + 2] = s;
}

// Partial row of tile (I, J) of sum_{a, b < M} G_A[a][b] dk(z_a, z_b)/dtheta (G_A materialised, Mpad x Mpad).
template <int DMAX>
__global__ void __launch_bounds__(WG) svgp_kzz_kernel(gpx_kernel_params p, int M, int P, const double* __restrict__ Z,
                                                      int64_t ldz, const double* __restrict__ GA,
                                                      double* __restrict__ part) {
  constexpr int XP = DMAX + 1;
  constexpr int SM = 2 * MT * XP > 4 * NROW ? 2 * MT * XP : 4 * NROW;
  __shared__ double smem[SM];
  const int nI = P / MT;
  const int I = (int)blockIdx.x / nI, J = (int)blockIdx.x % nI, i0 = I * MT, j0 = J * MT;
  const int d = p.d, kind = p.kind;
  double* zi = smem;
  double* zj = zi + MT * XP;
  for (int e = threadIdx.x; e < MT * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    zi[r * XP + k] = (k < d && i0 + r < M) ? Z[(int64_t)(i0 + r) * ldz + k] : 0.0;
    zj[r * XP + k] = (k < d && j0 + r < M) ? Z[(int64_t)(j0 + r) * ldz + k] : 0.0;
  }
  __syncthreads();
  double il[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) il[k] = (k < d) ? 1.0 / p.lengthscale[k] : 0.0;
  DkSums<DMAX> a;
  a.zero();
#pragma unroll 1
  for (int e = threadIdx.x; e < MT * MT; e += WG) {
    const int ri = e / MT, cj = e % MT;
    if (i0 + ri >= M || j0 + cj >= M) continue;
    dk_add<DMAX, -1>(p, kind, il, GA[(int64_t)(i0 + ri) * P + j0 + cj], zi + ri * XP, zj + cj * XP, a);
  }
  __syncthreads();
  dk_store<DMAX>(p, kind, il, a, smem, part + (int64_t)blockIdx.x * NROW);
}

// The K_ZZ part of the inducing-location gradient: zacc[a][k] = 2 sum_{b < M} G_A[a][b] d1 k(z_a, z_b)_k for the rows of
// tile I = blockIdx.x, the column tiles J in ascending order.  Thread (row, half) owns row a = 128 I + row and the
// columns 64 half .. 64 half + 63 of every tile; G_A is read through its transpose (it is symmetric), which the lanes'
// consecutive rows read coalesced.  b = a needs no special case: the stationary part is 0 there and the linear part's
// 2 G_A[a][a] outputscale v_k z_ak is the whole derivative of k(z_a, z_a).
template <int DMAX>
__global__ void __launch_bounds__(WG) svgp_kzz_z_kernel(gpx_kernel_params p, int M, int P, const double* __restrict__ Z,
                                                        int64_t ldz, const double* __restrict__ GA,
                                                        double* __restrict__ zacc) {
  constexpr int XP = DMAX + 1;
  __shared__ double zj[MT * XP];
  const int nI = P / MT, i0 = (int)blockIdx.x * MT;
  const int d = p.d, kind = p.kind;
  const bool lin = kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  const int row = threadIdx.x & (MT - 1), hh = threadIdx.x >> 7;
  const bool rowin = i0 + row < M;
  double il[DMAX], cz[DMAX], zr[DMAX], gz[DMAX];
  dz_consts<DMAX>(p, lin, cz);
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    il[k] = (k < d) ? 1.0 / p.lengthscale[k] : 0.0;
    zr[k] = (k < d && rowin) ? Z[(int64_t)(i0 + row) * ldz + k] : 0.0;
    gz[k] = 0.0;
  }
#pragma unroll 1
  for (int J = 0; J < nI; ++J) {
    const int j0 = J * MT;
    __syncthreads();
    for (int e = threadIdx.x; e < MT * DMAX; e += WG) {
      const int r = e / DMAX, k = e % DMAX;
      zj[r * XP + k] = (k < d && j0 + r < M) ? Z[(int64_t)(j0 + r) * ldz + k] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int c = hh * (MT / 2); c < (hh + 1) * (MT / 2); ++c) {
      if (!rowin || j0 + c >= M) continue;
      const double G = GA[(int64_t)(j0 + c) * P + i0 + row];
      const double* zb = zj + c * XP;
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        const double df = (zr[k] - zb[k]) * il[k];
        r2 += df * df;
      }
      double kfac;
      if (kind == GPX_KERNEL_RBF) {
        kfac = p.outputscale * exp(-0.5 * r2);
      } else {
        const double rr = sqrt(r2);
        kfac = p.outputscale * (5.0 / 3.0) * (1.0 + SQRT5 * rr) * exp(-SQRT5 * rr);
      }
      const double gk = G * kfac;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        gz[k] += gk * (zr[k] - zb[k]);
        if (lin) gz[k] += (G * cz[k]) * zb[k];
      }
    }
  }
  __syncthreads();
  dz_store<DMAX>(p, gz, 2.0, zj, zacc + (int64_t)i0 * DMAX);
}

// e[c] = y_c - const_mean - sum_jb mu[jb][c] (the covariance build's partials of K_chunk^T c_v) for the chunk's mc
// points, 0 up to the next multiple of 128: one column per thread.  Workgroup b leaves its sums in epart[b][ESUM]:
// {sum e, e^T e, sum_c x_ck^2 at 2 + k (linear kind)}; svgp_esum_kernel adds them in workgroup order into sc2.
constexpr int ESUM = 2 + GPX_MAX_DIM;
__global__ void __launch_bounds__(WG) svgp_echunk_kernel(gpx_kernel_params p, int njb, const double* __restrict__ mu,
                                                         int64_t ldk, const double* __restrict__ X, int64_t ldx,
                                                         const double* __restrict__ Y, int64_t ldy, int mc, int mcp,
                                                         double* __restrict__ ev, double* __restrict__ epart) {
  __shared__ double red[WG];
  const int c = (int)blockIdx.x * WG + threadIdx.x;
  double v = 0.0;
  if (c < mc) {
    double kc = 0.0;
    for (int jb = 0; jb < njb; ++jb) kc += mu[(int64_t)jb * ldk + c];
    v = (Y[(int64_t)c * ldy] - p.const_mean) - kc;
  }
  if (c < mcp) ev[c] = v;
  double* dst = epart + (int64_t)blockIdx.x * ESUM;
  const double se = block_sum(v, red), see = block_sum(v * v, red);
  if (threadIdx.x == 0) {
    dst[0] = se;
    dst[1] = see;
  }
  const bool lin = p.kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;  // (uniform)
  for (int k = 0; k < GPX_MAX_DIM; ++k) {
    double xx = 0.0;
    if (lin && k < p.d) {
      const double x = c < mc ? X[(int64_t)c * ldx + k] : 0.0;
      xx = block_sum(x * x, red);
    }
    if (threadIdx.x == 0) dst[2 + k] = xx;
  }
}

// sc2[0] += sum e, sc2[1] += e^T e, sc2[8 + k] += sum_c x_ck^2: the workgroups' sums in ascending order
__global__ void __launch_bounds__(WG) svgp_esum_kernel(const double* __restrict__ epart, int nb,
                                                       double* __restrict__ sc2) {
  const int o = threadIdx.x;
  if (o >= ESUM) return;
  double v = 0.0;
  for (int b = 0; b < nb; ++b) v += epart[(int64_t)b * ESUM + o];
  sc2[o < 2 ? o : 8 + o - 2] += v;
}

// Tile (I, cb) of H K_chunk (H symmetric, Mpad x Mpad; kc: Mpad x ldk, k over all of Mpad) and its contraction:
// part[blockIdx.x] = sum_{a in tile, a < M} sum_{i in tile, i < mc} (acc + c_v[a] e[i]) / s2 * dk(z_a, x_i)/dtheta.
//
// ZG (gpx_svgp_bound_grad_z_f64): the same tile is also contracted against d1 k(z_a, x_i), into zpart[blockIdx.x], the
// workgroup's 128 x DMAX row partial of dF/dZ.  The hyperparameter contraction keeps its thread mapping and order (its
// sums are the other instantiation's bit for bit); each thread leaves G kfac in the slab element it has just read (and G
// beside it for the linear kind), and a second loop over the slab, thread (row, half) = (tid % 128, tid / 128) owning
// one row and 8 of the slab's 16 columns, sums them into DMAX registers: no second exponential, one row per thread, and
// conflict-free LDS reads (KVP and XP are odd).  The slab's sums are added to the row's running sums in LDS (za), half
// 0 before half 1, so they are not live across the hyperparameter loop (with them the d > 16 linear kind would spill).
template <int DMAX, int KIND, bool ZG = false>
__global__ void __launch_bounds__(WG) svgp_grad_kernel(gpx_kernel_params p, int M, int Mpad,
                                                       const double* __restrict__ Z, int64_t ldz,
                                                       const double* __restrict__ H, const double* __restrict__ kc,
                                                       int64_t ldk, int ncb, const double* __restrict__ X, int64_t ldx,
                                                       int mc, const double* __restrict__ cv,
                                                       const double* __restrict__ ev, double* __restrict__ part,
                                                       double* __restrict__ zpart) {
  // Epilogue LDS: the tile's rows of Z and of X_chunk, c_v and e, and one 128 x SW slab of the product (ZG, linear kind:
  // a second slab for G)
  constexpr int SW = 16, KVP = SW + 1, XP = DMAX + 1;
  constexpr bool ZLIN = ZG && KIND < 0;
  constexpr bool CZS = ZLIN && DMAX > 16;  // the linear part's constants in LDS instead of registers
  constexpr int EPI = 2 * MT * XP + 2 * MT + MT * KVP + (ZLIN ? MT * KVP : 0) + (ZG ? MT * XP : 0) + (CZS ? DMAX : 0);
  constexpr int SMEM = EPI > GTile::LDS_DOUBLES ? EPI : GTile::LDS_DOUBLES;  // 73.7 KB for d <= 16
  __shared__ __attribute__((aligned(16))) double smem[SMEM];
  const int I = (int)blockIdx.x / ncb, cb = (int)blockIdx.x % ncb;
  const int a0 = I * MT, c0 = cb * MT;
  // A(m, k) = H[k][a0 + m] (H = H^T), B(k, c) = K[k][c0 + c]: both k-major, the projection's operand form
  trmm_asm::TileT<true, true, false, 16 * DMAX + KIND + 2 + (ZG ? 1024 : 0)> t;
  t.zero();
  t.run(H + a0, Mpad, kc + c0, ldk, Mpad / 16, smem);

  double* zi = smem;             // [MT][XP]
  double* xj = zi + MT * XP;     // [MT][XP]
  double* ci = xj + MT * XP;     // [MT]
  double* ej = ci + MT;          // [MT]
  double* kv = ej + MT;          // [MT][KVP]
  const int d = p.d;
  for (int e = threadIdx.x; e < MT * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    zi[r * XP + k] = (k < d && a0 + r < M) ? Z[(int64_t)(a0 + r) * ldz + k] : 0.0;
    xj[r * XP + k] = (k < d && c0 + r < mc) ? X[(int64_t)(c0 + r) * ldx + k] : 0.0;
  }
  for (int e = threadIdx.x; e < MT; e += WG) {
    ci[e] = cv[a0 + e];
    ej[e] = ev[c0 + e];
  }
  const int kind = KIND >= 0 ? KIND : p.kind;
  const double is2 = 1.0 / p.noise;
  double il[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) il[k] = (k < d) ? 1.0 / p.lengthscale[k] : 0.0;
  DkSums<DMAX> sums;
  sums.zero();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double* gb = kv + MT * KVP;                  // [MT][KVP] (ZLIN only)
  double* za = gb + (ZLIN ? MT * KVP : 0);     // [MT][XP]  (ZG only)
  [[maybe_unused]] double* czs = za + MT * XP; // [DMAX]    (CZS only)
  const int zrow = threadIdx.x & (MT - 1), zh = threadIdx.x >> 7;
  [[maybe_unused]] double cz[ZLIN && !CZS ? DMAX : 1];
  if constexpr (ZG) {
    for (int e = threadIdx.x; e < MT * XP; e += WG) za[e] = 0.0;
  }
  if constexpr (ZLIN && !CZS) dz_consts<DMAX>(p, true, cz);
  if constexpr (CZS) {
    if ((int)threadIdx.x < DMAX) {
      const int k = threadIdx.x;
      czs[k] = k < d ? -(p.outputscale * p.linear_variance[k]) * (p.lengthscale[k] * p.lengthscale[k]) : 0.0;
    }
  }
  // Eight 16-column slabs: the two waves owning the slab's columns park their accumulators in LDS, then all 256 threads
  // contract the slab element by element (a rolled loop keeps register pressure flat).
#pragma unroll
  for (int sl = 0; sl < MT / SW; ++sl) {
    if ((w & 1) == (sl >> 2)) {
#pragma unroll
      for (int a = 0; a < GTile::WM; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) kv[GTile::row_of(a, r) * KVP + (lane & 15)] = t.acc[a][sl & 3][r];
    }
    __syncthreads();
#pragma unroll 1
    for (int e = threadIdx.x; e < MT * SW; e += WG) {
      const int ri = e / SW, cj = sl * SW + e % SW;
      if (a0 + ri >= M || c0 + cj >= mc) {
        if constexpr (ZG) kv[ri * KVP + e % SW] = 0.0;
        if constexpr (ZLIN) gb[ri * KVP + e % SW] = 0.0;
        continue;
      }
      const double G = (kv[ri * KVP + e % SW] + ci[ri] * ej[cj]) * is2;
      const double gk = dk_add<DMAX, KIND>(p, kind, il, G, zi + ri * XP, xj + cj * XP, sums);
      if constexpr (ZG) kv[ri * KVP + e % SW] = gk;  // (this thread alone reads the element above)
      if constexpr (ZLIN) gb[ri * KVP + e % SW] = G;
    }
    __syncthreads();
    if constexpr (ZG) {
      constexpr int KB = DMAX > 16 ? 16 : DMAX;  // dimensions per sweep of the slab (two sweeps for d > 16)
#pragma unroll 1
      for (int kb = 0; kb < DMAX; kb += KB) {
        double zr[KB], gz[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          zr[k] = zi[zrow * XP + kb + k];
          gz[k] = 0.0;
        }
#pragma unroll 1
        for (int c = zh * (SW / 2); c < (zh + 1) * (SW / 2); ++c) {
          const double gk = kv[zrow * KVP + c];
          const double* xc = xj + (sl * SW + c) * XP + kb;
          if constexpr (ZLIN) {
            const double G = gb[zrow * KVP + c];
#pragma unroll
            for (int k = 0; k < KB; ++k) gz[k] += gk * (zr[k] - xc[k]) + (G * (CZS ? czs[kb + k] : cz[k])) * xc[k];
          } else {
#pragma unroll
            for (int k = 0; k < KB; ++k) gz[k] += gk * (zr[k] - xc[k]);
          }
        }
        if (zh == 0) {
#pragma unroll
          for (int k = 0; k < KB; ++k) za[zrow * XP + kb + k] += gz[k];
        }
        __syncthreads();
        if (zh == 1) {
#pragma unroll
          for (int k = 0; k < KB; ++k) za[zrow * XP + kb + k] += gz[k];
        }
        __syncthreads();
      }
    }
  }
  if constexpr (ZG) {  // the row partial: -il_k^2 times the running sums (dz_consts' arrangement)
    double* dst = zpart + (int64_t)blockIdx.x * MT * DMAX;
    for (int e = threadIdx.x; e < MT * DMAX; e += WG) {
      const int r = e / DMAX, k = e % DMAX;
      const double ilk = (k < d) ? 1.0 / p.lengthscale[k] : 0.0;
      dst[e] = -(ilk * ilk) * za[r * XP + k];
    }
    __syncthreads();  // (dk_store reuses the LDS image from its start)
  }
  dk_store<DMAX>(p, kind, il, sums, smem, part + (int64_t)blockIdx.x * NROW);
}

// acc[o] += sum over the partial rows, rows in ascending order within each of three stripes (mll_rowsum_kernel's scheme
// in one workgroup: at most a few thousand rows per launch)
__global__ void __launch_bounds__(WG) svgp_partsum_kernel(const double* __restrict__ part, int rows,
                                                          double* __restrict__ acc) {
  __shared__ double st[3][NROW];
  const int col = threadIdx.x % NROW, s = threadIdx.x / NROW;
  if (s < 3) {
    double v = 0.0;
    for (int r = s; r < rows; r += 3) v += part[(int64_t)r * NROW + col];
    st[s][col] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < NROW) acc[threadIdx.x] += (st[0][threadIdx.x] + st[1][threadIdx.x]) + st[2][threadIdx.x];
}

// zacc[128 I + r][k] += sum over the chunk's column blocks, ascending, of the row partials zpart[I ncb + cb][r][k]: one
// thread per element of row tile I = blockIdx.x (dmax: the row length the tile kernel was instantiated with)
__global__ void __launch_bounds__(WG) svgp_zsum_kernel(const double* __restrict__ zpart, int ncb, int dmax,
                                                       double* __restrict__ zacc) {
  const int64_t blk = (int64_t)MT * dmax;
  for (int e = threadIdx.x; e < blk; e += WG) {
    double v = 0.0;
    for (int cb = 0; cb < ncb; ++cb) v += zpart[((int64_t)blockIdx.x * ncb + cb) * blk + e];
    zacc[(int64_t)blockIdx.x * blk + e] += v;
  }
}

// dZ[a][k] = -zacc[a][k] = d(-F)/dz_ak for a < M, k < d (rows of dmax doubles in, of lddz out)
__global__ void __launch_bounds__(WG) svgp_zfinish_kernel(int M, int d, int dmax, const double* __restrict__ zacc,
                                                          double* __restrict__ dZ, int64_t lddz) {
  const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t a = e / d;
  const int k = (int)(e % d);
  if (a < M) dZ[a * lddz + k] = -zacc[a * dmax + k];
}

// The output vector of one task: the bound's six values, then the GPX_MLL_* block of -F and its gradient.
__global__ void __launch_bounds__(WG) svgp_grad_finish_kernel(gpx_kernel_params p, int M, int64_t n,
                                                              const double* __restrict__ bound,
                                                              const double* __restrict__ scal,
                                                              const double* __restrict__ sc2,
                                                              const double* __restrict__ gacc,
                                                              double* __restrict__ out) {
  const int o = threadIdx.x;
  if (o >= GPX_SVGP_GRAD_NOUT) return;
  const double s2 = p.noise, os = p.outputscale;
  const bool lin = p.kind == GPX_KERNEL_SCALE_LINEAR_MATERN52;
  if (o < GPX_SVGP_GRAD_MLL) {
    out[o] = o < GPX_SVGP_BOUND_NOUT ? bound[o] : 0.0;
    return;
  }
  const int q = o - GPX_SVGP_GRAD_MLL;
  double v = 0.0;  // dF/dtheta
  if (q == GPX_MLL_NLL) {
    v = bound[GPX_SVGP_BOUND_F];
  } else if (q == GPX_MLL_D_NOISE) {
    v = -0.5 * (double)n / s2 + 0.5 * sc2[2] / s2 + 0.5 * sc2[1] / (s2 * s2) + 0.5 * (scal[0] - scal[2]) / (s2 * s2);
  } else if (q == GPX_MLL_D_MEAN) {
    v = sc2[0] / s2;
  } else if (q == GPX_MLL_D_OUTPUTSCALE) {
    v = gacc[q] - 0.5 * (scal[0] / os) / s2;  // sum_i k(x_i, x_i) / outputscale = sum_i dk(x_i, x_i)/d outputscale
  } else if (q >= GPX_MLL_D_LENGTHSCALE && q < GPX_MLL_D_LENGTHSCALE + p.d) {
    v = gacc[q];
  } else if (lin && q >= GPX_MLL_D_LINVAR && q < GPX_MLL_D_LINVAR + p.d) {
    v = gacc[q] - 0.5 * os * sc2[8 + q - GPX_MLL_D_LINVAR] / s2;
  }
  out[o] = -v;
}

// T1 = I - S and Q = 2I - S - B - m m^T (natural order) from W', B' and m' (reversed), all tasks
hipError_t launch_svgp_grad_sq(Context* c, int ntask, int Mpad, int64_t ts, const double* Wp, const double* Bp,
                               const double* mrev, double* T1, double* Q) {
  const int nI = Mpad / MT;
  svgp_mm_kernel<<<dim3(nI * nI, ntask), WG, 0, c->stream>>>(Mpad, ts, Wp, Wp, 0, 1, 1.0, T1, Q, Bp, mrev);
  return hipGetLastError();
}

// out = scale W (T W^T ... ): U = W T (T symmetric) into tmp, then out = scale U W^T, all tasks
hipError_t launch_svgp_grad_conj(Context* c, int ntask, int Mpad, int64_t ts, const double* W, const double* T,
                                 double scale, double* tmp, double* out) {
  const int nI = Mpad / MT;
  svgp_mm_kernel<<<dim3(nI * nI, ntask), WG, 0, c->stream>>>(Mpad, ts, W, T, 1, 0, 1.0, tmp, nullptr, nullptr, nullptr);
  svgp_mm_kernel<<<dim3(nI * nI, ntask), WG, 0, c->stream>>>(Mpad, ts, tmp, W, 2, 0, scale, out, nullptr, nullptr,
                                                             nullptr);
  return hipGetLastError();
}

hipError_t launch_svgp_grad_unreverse(Context* c, int ntask, int Mpad, int64_t ts, const double* mrev, const double* T1,
                                      double* mnat, double* sc2) {
  svgp_unreverse_kernel<<<ntask, WG, 0, c->stream>>>(Mpad, ts, mrev, T1, mnat, sc2);
  return hipGetLastError();
}

// gacc += sum G_A dK_ZZ/dtheta of one task (part: (Mpad / 128)^2 rows of GPX_MLL_NOUT doubles)
hipError_t launch_svgp_grad_kzz(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                                const double* GA, double* part, double* gacc, double* zacc) {
  const int nI = Mpad / MT;
  with_dmax(p.d, [&](auto D) {
    svgp_kzz_kernel<decltype(D)::value><<<nI * nI, WG, 0, c->stream>>>(p, M, Mpad, Z, ldz, GA, part);
  });
  svgp_partsum_kernel<<<1, WG, 0, c->stream>>>(part, nI * nI, gacc);
  if (zacc)  // (writes every row of the task's accumulator: the chunks' sums are added to it)
    with_dmax(p.d, [&](auto D) {
      svgp_kzz_z_kernel<decltype(D)::value><<<nI, WG, 0, c->stream>>>(p, M, Mpad, Z, ldz, GA, zacc);
    });
  return hipGetLastError();
}

// One chunk of one task behind its covariance build (kc, and mu: that build's partials of K_chunk^T c_v): the residual
// e, the tile contractions and their sum into gacc.
hipError_t launch_svgp_grad_chunk(Context* c, const gpx_kernel_params& p, int M, int Mpad, const double* Z, int64_t ldz,
                                  const double* H, const double* kc, const double* mu, int64_t ldk, const double* X,
                                  int64_t ldx, const double* Y, int64_t ldy, int mc, const double* cv, double* ev,
                                  double* sc2, double* part, double* gacc, double* zpart, double* zacc) {
  const int nI = Mpad / MT, ncb = (mc + MT - 1) / MT;
  // (part is free until the tile contraction below writes it: the residual's per-workgroup sums pass through it)
  const int neb = (ncb * MT + WG - 1) / WG;
  svgp_echunk_kernel<<<neb, WG, 0, c->stream>>>(p, Mpad / NB, mu, ldk, X, ldx, Y, ldy, mc, ncb * MT, ev, part);
  svgp_esum_kernel<<<1, WG, 0, c->stream>>>(part, neb, sc2);
  const int grid = nI * ncb;
#define GPX_SG_K(D, K)                                                                                                \
  (zacc ? svgp_grad_kernel<D, K, true><<<grid, WG, 0, c->stream>>>(p, M, Mpad, Z, ldz, H, kc, ldk, ncb, X, ldx, mc,  \
                                                                   cv, ev, part, zpart)                              \
        : svgp_grad_kernel<D, K><<<grid, WG, 0, c->stream>>>(p, M, Mpad, Z, ldz, H, kc, ldk, ncb, X, ldx, mc, cv, ev, \
                                                             part, nullptr))
#define GPX_SG(D)                                                       \
  (p.kind == GPX_KERNEL_RBF        ? GPX_SG_K(D, GPX_KERNEL_RBF)        \
   : p.kind == GPX_KERNEL_MATERN52 ? GPX_SG_K(D, GPX_KERNEL_MATERN52)   \
                                   : GPX_SG_K(D, -1))
  int dmax;
  if (p.d <= 4)
    dmax = 4, GPX_SG(4);
  else if (p.d <= 8)
    dmax = 8, GPX_SG(8);
  else if (p.d <= 16)
    dmax = 16, GPX_SG(16);
  else
    dmax = 32, GPX_SG(32);
#undef GPX_SG
#undef GPX_SG_K
  svgp_partsum_kernel<<<1, WG, 0, c->stream>>>(part, grid, gacc);
  if (zacc) svgp_zsum_kernel<<<nI, WG, 0, c->stream>>>(zpart, ncb, dmax, zacc);
  return hipGetLastError();
}

hipError_t launch_svgp_grad_finish(Context* c, const gpx_kernel_params& p, int M, int64_t n, const double* bound,
                                   const double* scal, const double* sc2, const double* gacc, double* out,
                                   const double* zacc, double* dZ, int64_t lddz) {
  svgp_grad_finish_kernel<<<1, WG, 0, c->stream>>>(p, M, n, bound, scal, sc2, gacc, out);
  if (zacc) {
    const int dmax = p.d <= 4 ? 4 : p.d <= 8 ? 8 : p.d <= 16 ? 16 : 32;
    svgp_zfinish_kernel<<<(unsigned)(((int64_t)M * p.d + WG - 1) / WG), WG, 0, c->stream>>>(M, p.d, dmax, zacc, dZ,
                                                                                             lddz);
  }
  return hipGetLastError();
}

}  // namespace gpx
