// The pruned sweep's head phase: a bound of the posterior mean (RBF, fp64, d <= 16, one right-hand side).
// The rest of the library reaches this unit through sweep_mu_bound_ok and launch_mu_bound (gpx_internal.h): the lazy
// pruned sweep (gpx_sweep.hip) and gpx_debug_mu_bound_f64.
#include "gpx_internal.h"
#include "gpx_device.h"

namespace gpx {

// The pruned sweep's head needs the mean of every candidate only to bound its score from above, and every acquisition of
// the ABI is non-decreasing in the mean.  mu_bound_kernel gives, per candidate, mu_approx and mu_slack with
//     mu_approx - mu_slack <= mu <= mu_approx + mu_slack,
// mu being the value the exact path computes (sum_partials over the mean partials of KSTAR_FULL), at about a third of
// the exact build's instructions per entry: the exponential is v_exp_f32 with a first-order correction.
//
// Proof.  r2_j has the bits of the exact build's: same v / lengthscale, same centring by the mean of the row block's
// valid rows (mu_prep_kernel runs kstar_mfma_kernel's prologue once per row block), same MFMA sequence, same
// sqdist_expanded.  So with E_j = the exact path's exp(-r2_j / 2) and k_j = fl(outputscale * E_j) its K* entry,
// the two means differ by the exponential and by the summation only.
//  (a) exponential.  y = fl(r2 * (-log2(e) / 2)), yf = the fp32 nearest y, e = v_exp_f32(yf), rem = y - yf (exact in
//      fp64), e~ = fl(e + fl(e * rem) * ln 2).  2^y = 2^yf * 2^rem and 2^rem = 1 + rem ln 2 + O(rem^2) with |rem| <=
//      2^-24 |y| <= 2^-13.9 over the range where 2^y is not flushed (|y| < 127), so the second-order term is below 2^-29;
//      the roundings of y (|y| 2^-53 ln 2 relative), of the constant, of the two fp64 operations and the error of E_j
//      itself (1 ulp of fp64) are below 2^-40 together.  What is left is the instruction's error, documented as 1 ulp
//      (2^-23 relative), and its flush of results below 2^-126 to zero.  Hence
//          |e~ - E| <= eps1 e~ + eps2,    eps1 = MUB_EPS1 = 2^-20,  eps2 = MUB_EPS2 = 2^-120,
//      each constant at least 4 x the largest error measured over 2^22 arguments in [-760, 0] and every fp32 argument of
//      three binades (tests/test_gpu_sweep_mubound.py: at most 0.089 of eps1 e~ + eps2, 2^-23.5 relative).
//      NaN r2 gives NaN; r2 = +inf gives y = yf = -inf, e = 0, rem = NaN replaced by 1 (fmin), e~ = 0.
//  (b) sums.  The kernel forms S = sum_j alpha_j e~_j and A = sum_j |alpha_j| e~_j by fp64 FMAs, every term passing at
//      most npad / 4 + 2 additions: |S - sum alpha e~| <= (npad / 4 + 2) u A' with u = 2^-53 and A' = sum |alpha| e~ (exact),
//      A >= A' (1 - (npad / 4 + 2) u).  The exact path: |mu - sum alpha k| <= (npad / 64 + 18) u sum |alpha| k (16 FMAs and
//      two shuffles per partial, then sum_partials), and |k - outputscale E| <= u outputscale E.
//  (c) together, with mu_approx = fl(outputscale S):
//          |mu_approx - mu| <= outputscale (eps1 A' + eps2 |alpha|_1) + (npad / 4 + npad / 64 + 23) u outputscale (1 + eps1) A'
//                              + (npad / 64 + 19) u outputscale eps2 |alpha|_1
//      which lies below mu_slack = (eps1 A~ + eps2 outputscale |alpha|_1 + (n + 64) 2^-52 A~) (1 + 2^-30), A~ =
//      fl(outputscale A): (n + 64) 2^-52 = 2 (n + 64) u is more than twice the factor in front of u above (npad < n +
//      128), and the factor 1 + 2^-30 covers A~ against outputscale A', the last line's term ((npad / 64 + 19) u < 2^-30)
//      and the roundings of the slack's own operations.  Padded rows have alpha = 0: their terms are exact zeros (e~ is finite for a finite candidate).  With
//      alpha = 0 everywhere S = A = 0 and the slack is exactly 0.
//  (d) the head's bound pass scores mu_approx + mu_slack.  The rounded sum can fall below the real one by u |sum|; since
//      mu_slack >= eps1 |mu_approx|, the 2^-30 in (c) covers that too.  The y transform is monotone under rounding, and
//      acq_score's own rounding is what PRUNE_EPS is for, as with the variance bound.
constexpr double MUB_EPS1 = 0x1p-20, MUB_EPS2 = 0x1p-120;

__device__ __forceinline__ double exp_half_neg_fast(double r2) {  // ~ exp(-r2 / 2), r2 >= 0 (or NaN)
  const double y = r2 * -0.72134752044448170367996234050095;  // -log2(e) / 2
  const float yf = (float)y;
  const double e = (double)__builtin_amdgcn_exp2f(yf);
  const double rem = fmin(y - (double)yf, 1.0);  // (y = -inf: NaN -> 1 with e = 0)
  return fma(e * rem, 0.69314718055994530941723212145818, e);
}

// The factorised form (mu_fact_kernel).  With one centre c for every row block (the mean of the valid scaled
// rows), a_j = x_j / l - c and b = x* / l - c,
//     exp(-r2_j / 2) = exp(-|a_j|^2 / 2) exp(-|b|^2 / 2) exp(a_j . b):
// the row factor goes into alpha once per row (alpha'_j = alpha_j exp(-|a_j|^2 / 2), fp64, mu_prep_kernel), the candidate
// factor G = exp(-|b|^2 / 2) is applied once per candidate, and an entry costs v_cvt_f32_f64, v_exp_f32 and two v_fma_f32:
// the rows' fragments carry log2(e), so the MFMA sequence gives y = log2(e) a_j . b, e = v_exp_f32(fl32(y)),
// S += alpha"_j e, A += |alpha"_j| e in fp32 over the 16 rows a lane holds of a row block, the runs added in fp64.
// alpha" = fl32(alpha' / 2^k), 2^k >= max |alpha'| (exact scaling; |alpha"| <= 1, a run stays below 2^20).
//     mu_approx = outputscale 2^k S G,   A~ = |outputscale| 2^k A G.
// A workgroup takes this form only if every candidate c of it has
//     Y_c = log2(e) sqrt(M2 |b|^2) (1 + 2^-40) <= MUF_Y_LIMIT  and  Q_c = M2 + |b|^2 <= MUF_Q_LIMIT,  M2 = max_j |a_j|^2
// (written so that NaN fails); otherwise it flags itself (mu_slack = -1 for its candidates) and mu_bound_kernel, launched
// behind, runs it as before; mu_bound_kernel's other workgroups return at once.  |y| <= Y_c (Cauchy-Schwarz on the
// computed fragments, M2 being the maximum of the very values |a_j|^2 the row factors use).
//
// Proof of |mu_approx - mu| <= mu_slack on this path.  r2 no longer shares bits with the exact build, so both sides are
// compared with the real value R_j = outputscale alpha_j exp(-|s_j - s*|^2 / 2) of the fp64 scaled points s = x / l;
// u = 2^-53, v = 2^-24, D = DMAX.
//  (e) the exact path against R.  Its centred points carry u relative per coordinate, the norms D u, the MFMA dot
//      D u |a'||b'|, the two operations of sqdist_expanded u each: |r2 - real| <= 2 (D + 4) u (|a'|^2 + |b'|^2), the clamp
//      only helping; its block centre lies within sqrt(M2) of c, so |a'|^2 + |b'|^2 <= 6 Q_c.  With exp's and the
//      outputscale's ulp: |k_j - R_j / alpha_j| <= (6 (D + 4) Q_c + 4) u k_j <= (120 Q_c + 4) u k_j.
//  (f) this path against R, fp64 part.  |a - b|^2 = |a|^2 + |b|^2 - 2 a.b exactly for the rounded a, b, and differs from
//      the real r2 by <= 4 u Q_c; the two norms carry D u each (exponent error <= D u Q_c / 2), the fragments' scaling 2 u
//      and the MFMA D u (|y - log2(e) a.b| <= (D + 2) u Y_c <= 288 u), exp / products of alpha', G and the final
//      scalings <= 8 u: relative (12 Q_c + 210) u.
//      (e) + (f) + the sums of (b) (here npad / 64 + 6 fp64 additions per term) lie below
//          eps64 = (256 Q_c + 512 + 2 (n + 64)) u  <=  2^-29 + (n + 320) 2^-52.
//  (g) fp32 part, relative to |alpha"_j| e_j: rounding of y to fp32 <= v Y_c ln 2 (on 2^y), the instruction 2 v (1 ulp,
//      no flush: |y| <= 16), alpha"'s rounding v, the run of 16 FMAs 16 v: (19 + 0.6932 Y_c) v.  Second-order terms and
//      A against the true sum (A >= |S|: the two runs round monotonically in the same order) take the factor 1 + 2^-8:
//          eps1(c) = ((19 + 0.6932 Y_c) 2^-24 + eps64) (1 + 2^-8)  <=  2^-19.08 + 2^-28 < 2^-18  for Y_c <= 16.
//  (h) flushes.  alpha" below 2^-126 may flush (<= 2^-126 e <= 2^-110 each), so may an FMA's result (2^-126): less than
//      n 2^-109 2^k <= 2^-84 |alpha|_1 in all for n < 2^24 (2^k <= 2 max |alpha'| <= 2 |alpha|_1); alpha' or G below the
//      fp64 normal range lose at most 2^-1074 2^16 per term, which MUF_EPS2 |alpha|_1 covers because mu_prep_kernel sends
//      every workgroup to the other path when 0 < max |alpha'| < 2^-800 (or when it is not finite).  MUF_EPS2 = 2^-80.
//      mu_slack = (eps1(c) A~ + MUF_EPS2 |outputscale| |alpha|_1) (1 + 2^-30).
//  Zero alpha: alpha" = 0, S = A = 0, G finite: both values are exact zeros.  Padded rows have alpha" = 0 and zero
//  fragments (e = 1): exact zeros.  A NaN or infinite candidate fails the eligibility test and keeps the other path's
//  result (NaN stays NaN).  (d) holds as before: mu_slack >= eps1 |mu_approx|.
constexpr double MUF_Y_LIMIT = 16.0, MUF_Q_LIMIT = 65536.0, MUF_EPS2 = 0x1p-80;
constexpr double MUF_LOG2E = 1.44269504088896340735992468100189;

// The fp32 factorised form (mu_fact32_kernel; 4 < d <= 8, the DMAX = 8 instance).  The same factorisation, but
// y is never held in fp64: the fragments are A = fl32(fl(log2(e) a_j)) and B = fl32(b), the dot product runs on
// v_mfma_f32_16x16x4_f32 (KS = DMAX / 4 chained instructions on a zero accumulator) and e = v_exp_f32 of its result;
// everything behind e (alpha", the fp32 runs, the fp64 sums, G, the scalings) is mu_fact_kernel's, except that a run is
// MUF32_RUN = 8 rows of a lane, not 16.  Nothing downstream of y saw more than 24 bits of it before either; the price is the dot product's own fp32 rounding, which grows with d and Y_c, so the form is taken by
// eps1_32(c) itself: a workgroup eligible for a factorised form (Y_c <= MUF_Y_LIMIT, Q_c <= MUF_Q_LIMIT) runs here only
// if every candidate of it has eps1_32(c) <= MUF32_EPS1_MAX (1 - 2^-12) (written so that NaN fails); otherwise it flags
// itself (mu_slack = -2) for mu_fact_kernel.  So every candidate on either factorised form has eps1 < 2^-18.
//
// Proof of |mu_approx - mu| <= mu_slack here: (e), (f) and (h) stand (the fp64 MFMA's D u Y_c in (f) is no longer spent);
// (g) is replaced by (g32), with d = p.d the number of coordinates that are not padding.
//  (g32) fp32 part, relative to |alpha"_j| e_j.
//      fragments.  A_i = La_i (1 + t1), B_i = b_i (1 + t2), |t| <= v, La_i = fl(log2(e) a_i) (its u is in (f)).
//      the MFMA.  The arithmetic model assumed: the instruction takes f32 operands and returns an f32 accumulator, and
//      every product and every addition in it is rounded to nearest at worst once each, in any order (a fused or wider
//      internal sum only does better); a chain of KS instructions adds KS - 1 roundings inside the same count.  Then
//          |yhat - sum_i A_i B_i| <= gamma_d sum_i |A_i B_i|,   gamma_d = d v / (1 - d v),
//      d products and d - 1 additions (the first lands on a zero accumulator, exactly).  Padded coordinates have A_i =
//      B_i = 0: exact zeros under any model.  The result is the fp32 number v_exp_f32 reads: the old "y -> fp32" term
//      is part of this one.  tools/probes/mfma_f32_probe.hip measures the model on adversarial inputs (cancelling
//      pairs, one large and many small terms, magnitudes over 2^40, random signs, denormals): DESIGN §3 quotes the
//      largest error in units of v sum |A_i B_i|.
//      Cauchy-Schwarz on the rounded fragments: sum |A_i B_i| <= (1 + v)^2 sum |La_i b_i| <= (1 + v)^2 (1 + u) log2(e)
//      |a||b| <= Y_c (1 + 2^-22) (Y_c carries 1 + 2^-40 for its own roundings).  Together
//          |yhat - log2(e) a.b| <= (d + 2) v Y_c (1 + 2^-20)  (+ the fp64 roundings of (f)),
//      on 2^y relative ln 2 (d + 2) v Y_c (1 + 2^-16) (second order: ln 2 (d + 2) v Y_c <= 2^-17).
//      as in (g): the instruction 2 v (1 ulp), alpha"'s rounding v, the run of MUF32_RUN = 8 FMAs 8 v (two runs per row
//      block: npad / 32 + 6 fp64 additions per term instead of npad / 64 + 6, still inside eps64's 2 (n + 64) u with
//      the exact path's npad / 64 + 18).  With the factor 1 + 2^-8 as in (g):
//          eps1_32(c) = ((MUF32_RUN + 3 + 0.6932 (d + 2) Y_c) 2^-24 + eps64) (1 + 2^-8);
//      at d = 8 it is below 2^-18 for Y_c <= 7.6, at d = 5 for Y_c <= 10.8.  (Runs of 16 give 19 in place of 11 and Y_c
//      <= 6.45 at d = 8, which sends 20 of the bench step's 4096 workgroups to the fp64 form, where they run alone for
//      0.15 ms; runs of 8 cost 0.02 ms in this kernel: step 7.05 against 7.21 ms, profiles/r13_run_length_ab.jsonl.)
//      fp32 range.  |La_i| <= log2(e) sqrt(M2) and |b_i| <= |b| are at most 2^8.6 under Q_c <= 2^16, every product and
//      partial sum at most 2^17.2: no overflow.  A fragment, a product or a partial sum below 2^-126 may be flushed or
//      rounded as a denormal: an absolute error of at most 2^-126 each, times the other operand (<= 2^9) for a fragment;
//      over d <= 8 coordinates less than 2^-112 on y, so 2^-112 relative on 2^y: far inside the factor 1 + 2^-8 (which
//      leaves 11 v 2^-8 > 2^-29 unspent).  |yhat| <= Y_c (1 + (d + 2) v (1 + 2^-20)) < 16.001: v_exp_f32 returns a
//      normal number (>= 2^-17), no flush, and its 1 ulp holds.
//  The slack is mu_fact_kernel's expression with eps1_32(c).  MUF32_EPS1_MAX = 2^-18; the 2^-12 of margin in the
//  eligibility test covers the roundings of eps1_32 itself (a few u), A~ against the true sum |alpha_j| k_j (eps1
//  relative) and the slack's 1 + 2^-30, so the written slack is below 2^-18 sum |alpha_j| k_j + MUF_EPS2 |outputscale|
//  |alpha|_1 (1 + 2^-30).  Zero alpha, padded rows, NaN and infinite candidates: as on the fp64 form.
//  Only DMAX = 8 is built.  At DMAX = 16 the limit admits Y_c < 3.6 only, which unit-cube candidates do not meet; at
//  DMAX = 4 the form was built and tested (with runs of 16), but its looser bound let three more candidates of 45,000
//  through the head in a d = 4 call whose sweep_stats tests/test_gpu_sweep_narrow.py pins, so d <= 4 keeps the fp64 form.
// (mu_fp32_form(DMAX), gpx_sweep_layout.h: DMAX == 8)
constexpr double MUF32_EPS1_MAX = 0x1p-18;
constexpr int MUF32_RUN = 8;  // rows a lane sums in fp32 before the run goes to the fp64 sums (8 or 16; see (g32))
typedef float f4 __attribute__((ext_vector_type(4)));  // v_mfma_f32_16x16x4_f32's accumulator

// The buffer's head: MUF_HEAD doubles of call-wide values, then the row blocks' records (MuPrep), the factorised form's
// records (MuFact) and the row blocks' sums and maxima (MuStat).
constexpr int MUF_FALLBACK = 0;  // int64: workgroups of the last call that took mu_bound_kernel's path
constexpr int MUF_FP64FORM = 20;  // int64: workgroups of the last call that took mu_fact_kernel (the fp64 factorised form)
constexpr int MUF_M2 = 1, MUF_SCALE = 2, MUF_L1 = 3, MUF_CEN = 4;  // (MUF_HEAD: gpx_sweep_layout.h)

// Per row block of 64 training rows: kstar_mfma_kernel's prologue (scaled rows, centre = mean of the valid rows, centred
// rows, their norms), alpha with zeros for the padded rows, and sum |alpha| of the block.  Layout of a block's record:
template <int DMAX>
struct MuPrep {
  static constexpr int ROWS = 0, NA = NB * DMAX, AL = NA + NB, CEN = AL + NB, L1 = CEN + DMAX, STRIDE = L1 + 2;
};
// The factorised form's record of a row block: the fragments log2(e) a in the MFMA's own order (double FRAG + ((s KS +
// k) 64 + lane) = row 16 s + (lane & 15), coordinate 4 k + (lane >> 4)), then alpha" as 64 floats, row 16 s + kq + 4 r at
// float 16 kq + 4 s + r (the 16 rows of a lane in a row).
template <int DMAX>
struct MuFact {
  static constexpr int FRAG = 0, AL = NB * DMAX, STRIDE = AL + NB / 2;
};
// The fp32 form's record of a row block (DMAX = 8), after the MuStat records: the fragments fl32(log2(e) a) in the same
// MFMA order as floats, then alpha" as 64 floats in the order of the f32 accumulator (register r of lane 16 kq + m is row
// 4 kq + r of the 16 x 16 result, not kq + 4 r): row 16 s + 4 kq + r at float 16 kq + 4 s + r.  Offsets in floats.
template <int DMAX>
struct MuFact32 {
  static constexpr int FRAG = 0, AL = NB * DMAX, STRIDE_D = mu_fp32_form(DMAX) ? (NB * DMAX + NB) / 2 : 0;  // STRIDE_D in doubles
};
// A row block's column sums of the scaled rows, then max |a|^2, max |alpha'| and sum |alpha| over its valid rows.
template <int DMAX>
struct MuStat {
  static constexpr int SUM = 0, M2 = DMAX, AM = DMAX + 1, L1 = DMAX + 2, STRIDE = DMAX + 4;
};
// mu_prep_doubles (gpx_sweep_layout.h) is the sum of a row block's records
template <int D>
constexpr bool mu_prep_matches_layout =
    mu_prep_block_doubles(D) == MuPrep<D>::STRIDE + MuFact<D>::STRIDE + MuStat<D>::STRIDE + MuFact32<D>::STRIDE_D;
static_assert(mu_prep_matches_layout<4> && mu_prep_matches_layout<8> && mu_prep_matches_layout<16>, "mu_prep");
template <int DMAX>
__device__ __forceinline__ double* mu_stat(double* prep, int npad, int jb) {
  return prep + MUF_HEAD + (int64_t)(npad / NB) * (MuPrep<DMAX>::STRIDE + MuFact<DMAX>::STRIDE) +
         (int64_t)jb * MuStat<DMAX>::STRIDE;
}
template <int DMAX>
__device__ __forceinline__ const double* mu_fact_rec(const double* prep, int npad, int jb) {
  return prep + MUF_HEAD + (int64_t)(npad / NB) * MuPrep<DMAX>::STRIDE + (int64_t)jb * MuFact<DMAX>::STRIDE;
}
template <int DMAX>
__device__ __forceinline__ const float* mu_fact32_rec(const double* prep, int npad, int jb) {
  return reinterpret_cast<const float*>(prep + MUF_HEAD +
                                        (int64_t)(npad / NB) * (MuPrep<DMAX>::STRIDE + MuFact<DMAX>::STRIDE +
                                                                MuStat<DMAX>::STRIDE) +
                                        (int64_t)jb * MuFact32<DMAX>::STRIDE_D);
}

// |a|^2 of row j for the centre cen: the value the row factor, M2 and (through M2) the eligibility test all use.
template <int DMAX>
__device__ __forceinline__ double mu_row_norm(const gpx_kernel_params& p, const double* __restrict__ X, int64_t ldx,
                                              int j, const double* cen) {
  double u = 0.0;
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    const double a = k < p.d ? X[(int64_t)j * ldx + k] / p.lengthscale[k] - cen[k] : 0.0;
    u = fma(a, a, u);
  }
  return u;
}
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }  // a NaN stays

// The call-wide values of the factorised form (centre, M2, 2^k, |alpha|_1) in three small launches of one workgroup per
// row block, every sum and maximum in a fixed order: the blocks' column sums; from them the centre (every workgroup the
// same bits) and the blocks' maxima; from those M2 and 2^k in mu_prep_kernel.
template <int DMAX>
__global__ void __launch_bounds__(WG) mu_colsum_kernel(gpx_kernel_params p, int n, int npad,
                                                       const double* __restrict__ X, int64_t ldx,
                                                       double* __restrict__ prep) {
  __shared__ double red[WG];
  const int jb = blockIdx.x, j0 = jb * NB, d = p.d, t = threadIdx.x, k = t % DMAX;
  double s = 0.0;
  if (k < d)
    for (int r = t / DMAX; r < NB && j0 + r < n; r += WG / DMAX) s += X[(int64_t)(j0 + r) * ldx + k] / p.lengthscale[k];
  red[t] = s;
  __syncthreads();
  if (t < DMAX) {
    double v = 0.0;
    for (int i = t; i < WG; i += DMAX) v += red[i];
    mu_stat<DMAX>(prep, npad, jb)[MuStat<DMAX>::SUM + t] = v;
  }
}

template <int DMAX>
__global__ void __launch_bounds__(NB) mu_rowstat_kernel(gpx_kernel_params p, int n, int npad,
                                                        const double* __restrict__ X, int64_t ldx,
                                                        const double* __restrict__ alpha, double* __restrict__ prep) {
  using T = MuStat<DMAX>;
  __shared__ double cen[DMAX];
  const int jb = blockIdx.x, j = jb * NB + (int)threadIdx.x, t = threadIdx.x;
  if (t < DMAX) {
    double s = 0.0;
    for (int b = 0; b < npad / NB; ++b) s += mu_stat<DMAX>(prep, npad, b)[T::SUM + t];
    cen[t] = s / n;
    if (jb == 0) prep[MUF_CEN + t] = cen[t];
  }
  __syncthreads();
  double m2 = 0.0, am = 0.0, l1 = 0.0;
  if (j < n) {
    m2 = mu_row_norm<DMAX>(p, X, ldx, j, cen);
    am = fabs(alpha[j] * exp(-0.5 * m2));
    l1 = fabs(alpha[j]);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    m2 = max_nan(m2, __shfl_xor(m2, o));
    am = max_nan(am, __shfl_xor(am, o));
    l1 += __shfl_xor(l1, o);
  }
  if (t == 0) {
    double* st = mu_stat<DMAX>(prep, npad, jb);
    st[T::M2] = m2, st[T::AM] = am, st[T::L1] = l1;
  }
}

template <int DMAX>
__global__ void __launch_bounds__(WG) mu_prep_kernel(gpx_kernel_params p, int n, int npad, const double* __restrict__ X,
                                                     int64_t ldx, const double* __restrict__ alpha,
                                                     double* __restrict__ prep) {
  using P = MuPrep<DMAX>;
  using F = MuFact<DMAX>;
  using T = MuStat<DMAX>;
  constexpr int KS = DMAX / 4;
  __shared__ double sa[NB][DMAX + 1], cen[DMAX], inv_scale;
  const int jb = blockIdx.x, j0 = jb * NB, d = p.d, t = threadIdx.x;
  const int nv = n - j0 < NB ? n - j0 : NB;
  if (t < 64) {  // M2, 2^k and |alpha|_1 from the blocks' values (every workgroup the same bits; block 0 writes the head)
    double m2 = 0.0, am = 0.0, l1 = 0.0;
    for (int b = t; b < npad / NB; b += 64) {
      const double* st = mu_stat<DMAX>(prep, npad, b);
      m2 = max_nan(m2, st[T::M2]);
      am = max_nan(am, st[T::AM]);
      l1 += st[T::L1];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      m2 = max_nan(m2, __shfl_xor(m2, o));
      am = max_nan(am, __shfl_xor(am, o));
      l1 += __shfl_xor(l1, o);
    }
    if (t == 0) {
      double scale = 1.0;
      if (am > 0.0) {
        int e;
        (void)frexp(am, &e);
        scale = ldexp(1.0, e);  // am in [scale / 2, scale)
      }
      if (!(am <= 0x1p1000) || (am > 0.0 && am < 0x1p-800)) m2 = __builtin_nan("");  // every workgroup to the other path
      inv_scale = 1.0 / scale;
      if (jb == 0) {
        reinterpret_cast<unsigned long long*>(prep)[MUF_FALLBACK] = 0ull;
        reinterpret_cast<unsigned long long*>(prep)[MUF_FP64FORM] = 0ull;
        prep[MUF_M2] = m2;
        prep[MUF_SCALE] = scale;
        prep[MUF_L1] = l1;
      }
    }
  }
  __syncthreads();
  // the factorised forms' records (the centre is in the head: mu_rowstat_kernel); the fp32 form's holds the same
  // values, rounded once more
  auto record = [&](auto* frag, float* al, int kq_rows, int r_rows) {  // alpha" of row 16 s + kq_rows kq + r_rows r
    using E = std::remove_pointer_t<decltype(frag)>;
    const double* gc = prep + MUF_CEN;
    for (int e = t; e < NB * DMAX; e += WG) {
      const int lane = e & 63, k = (e >> 6) % KS, s = (e >> 6) / KS;
      const int j = j0 + 16 * s + (lane & 15), col = 4 * k + (lane >> 4);
      const double a = (col < d && j < n) ? X[(int64_t)j * ldx + col] / p.lengthscale[col] - gc[col] : 0.0;
      frag[e] = (E)(a * MUF_LOG2E);
    }
    if (t < NB) {
      const int kq = t >> 4, s = (t >> 2) & 3, r = t & 3, j = j0 + 16 * s + kq_rows * kq + r_rows * r;
      double ap = 0.0;
      if (j < n) ap = alpha[j] * exp(-0.5 * mu_row_norm<DMAX>(p, X, ldx, j, gc)) * inv_scale;
      al[t] = (float)ap;
    }
  };
  {
    double* fo = const_cast<double*>(mu_fact_rec<DMAX>(prep, npad, jb));
    record(fo + F::FRAG, reinterpret_cast<float*>(fo + F::AL), 1, 4);
  }
  if constexpr (mu_fp32_form(DMAX)) {
    float* go = const_cast<float*>(mu_fact32_rec<DMAX>(prep, npad, jb));
    record(go + MuFact32<DMAX>::FRAG, go + MuFact32<DMAX>::AL, 4, 1);
  }
  double* out = prep + MUF_HEAD + (int64_t)jb * P::STRIDE;
  for (int e = t; e < NB * DMAX; e += WG) {
    const int r = e / DMAX, k = e % DMAX;
    const double v = (k < d && j0 + r < n) ? X[(int64_t)(j0 + r) * ldx + k] : 0.0;
    sa[r][k] = (k < d) ? v / p.lengthscale[k] : 0.0;
  }
  __syncthreads();
  if (t < DMAX) {
    double s = 0.0;
    for (int r = 0; r < nv; ++r) s += sa[r][t];
    cen[t] = nv > 0 ? s / nv : 0.0;
  }
  __syncthreads();
  for (int e = t; e < NB * DMAX; e += WG) sa[e / DMAX][e % DMAX] -= cen[e % DMAX];
  __syncthreads();
  for (int e = t; e < NB * DMAX; e += WG) out[P::ROWS + e] = sa[e / DMAX][e % DMAX];
  if (t < NB) {
    double u = 0.0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) u = fma(sa[t][k], sa[t][k], u);
    out[P::NA + t] = u;
    out[P::AL + t] = j0 + t < n ? alpha[j0 + t] : 0.0;
  }
  if (t < DMAX) out[P::CEN + t] = cen[t];
  if (t == 0) {
    double s = 0.0;
    for (int r = 0; r < nv; ++r) s += fabs(alpha[j0 + r]);
    out[P::L1] = s;
  }
}

// Workgroup x: candidates 256 x .. 256 x + 255 against every row block.  The candidate tile is loaded and divided once
// (a thread keeps its own candidate's scaled coordinates in registers); per row block it is centred and its norms are
// taken (the bits of kstar_mfma_kernel's), then kstar_mfma_kernel's MFMA sequence and the fast exponential.
template <int DMAX>
__global__ void __launch_bounds__(WG) mu_bound_kernel(gpx_kernel_params p, int n, const double* __restrict__ prep,
                                                      const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                      double* __restrict__ mu_approx, double* __restrict__ mu_slack) {
  using P = MuPrep<DMAX>;
  constexpr int KS = DMAX / 4;
  __shared__ double sa[NB][DMAX + 1], sb[WG][DMAX + 1], na[NB], nb[WG], sal[NB];
  const int d = p.d, t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * WG;
  if (mu_slack[c0] != -1.0) return;  // mu_fact_kernel did this workgroup's candidates
  prep += MUF_HEAD;
  const int nblk = (n + NB - 1) / NB;  // row blocks with a valid row
  double xb[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    const double v = (k < d && c0 + t < m_chunk) ? Xs[(c0 + t) * ldxs + k] : 0.0;
    xb[k] = (k < d) ? v / p.lengthscale[k] : 0.0;
  }
  const int lane = t & 63, w = t >> 6, m = lane & 15, kq = lane >> 4;
  double S[4] = {0.0, 0.0, 0.0, 0.0}, A[4] = {0.0, 0.0, 0.0, 0.0}, l1 = 0.0;
#pragma unroll 1
  for (int jb = 0; jb < nblk; ++jb) {
    const double* __restrict__ in = prep + (int64_t)jb * P::STRIDE;
    __syncthreads();  // (the previous block's reads)
    for (int e = t; e < NB * DMAX; e += WG) sa[e / DMAX][e % DMAX] = in[P::ROWS + e];
    if (t < NB) {
      na[t] = in[P::NA + t];
      sal[t] = in[P::AL + t];
    }
    l1 += in[P::L1];
    {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        const double s = xb[k] - in[P::CEN + k];
        sb[t][k] = s;
        v = fma(s, s, v);
      }
      nb[t] = v;
    }
    __syncthreads();
    double nbc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) nbc[cb] = nb[64 * w + 16 * cb + m];
#pragma unroll 1
    for (int rs = 0; rs < NB; rs += 16) {
      d4 acc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        acc[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < KS; ++k)
          acc[cb] = mfma16x16x4(sa[rs + m][4 * k + kq], sb[64 * w + 16 * cb + m][4 * k + kq], acc[cb]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = rs + kq + 4 * r;
        const double naj = na[j], al = sal[j];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const double e = exp_half_neg_fast(sqdist_expanded(naj, nbc[cb], acc[cb][r]));
          S[cb] = fma(al, e, S[cb]);
          A[cb] = fma(fabs(al), e, A[cb]);
        }
      }
    }
  }
  const double os = fabs(p.outputscale);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    double s = S[cb], a = A[cb];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    a += __shfl_xor(a, 16);
    a += __shfl_xor(a, 32);
    const int64_t c = c0 + 64 * w + 16 * cb + m;
    if (kq == 0 && c < m_chunk) {
      const double at = os * a;
      mu_approx[c] = p.outputscale * s;
      mu_slack[c] = (MUB_EPS1 * at + MUB_EPS2 * os * l1 + ((double)(n + 64) * 0x1p-52) * at) * (1.0 + 0x1p-30);
    }
  }
}

// eps1(c) of (g) (the fp64 form) or eps1_32(c) of (g32) for the candidate with |b|^2 = nbq; its Y_c and Q_c in yc, q.
template <bool FP32>
__device__ __forceinline__ double mu_eps1(const gpx_kernel_params& p, int n, const double* __restrict__ prep, double nbq,
                                          double& yc, double& q) {
  const double m2 = prep[MUF_M2];
  yc = MUF_LOG2E * sqrt(m2 * nbq) * (1.0 + 0x1p-40), q = m2 + nbq;
  const double run = FP32 ? (double)(MUF32_RUN + 3) : 19.0, coef = FP32 ? 0.6932 * (double)(p.d + 2) : 0.6932;
  return ((run + coef * yc) * 0x1p-24 + (256.0 * q + 512.0 + 2.0 * (double)(n + 64)) * 0x1p-53) * (1.0 + 0x1p-8);
}

// The classification of a workgroup of 256 candidates, by the first kernel behind mu_prep_kernel (mu_fact32_kernel, or
// mu_class_kernel where the fp32 form is not built): not eligible for a factorised form -> mu_slack = -1 and the
// fallback counter (mu_bound_kernel runs it); eligible but not for the fp32 form (FP32 false, or some eps1_32(c) over the
// limit) -> mu_slack = -2 and the MUF_FP64FORM counter (mu_fact_kernel runs it); else true: the caller computes.
// nbq = |b|^2 of thread t's candidate; eps32 = eps1_32(c) is returned for it.
template <bool FP32>
__device__ __forceinline__ bool mu_classify(const gpx_kernel_params& p, int n, double* __restrict__ prep, double nbq,
                                            int64_t c, int64_t m_chunk, double* __restrict__ mu_slack, double& eps32) {
  double yc, q;
  eps32 = mu_eps1<true>(p, n, prep, nbq, yc, q);
  const bool ok = c >= m_chunk || (yc <= MUF_Y_LIMIT && q <= MUF_Q_LIMIT);  // (NaN fails)
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(prep);
  if (!__syncthreads_and(ok)) {
    if (c < m_chunk) mu_slack[c] = -1.0;
    if (threadIdx.x == 0) atomicAdd(cnt + MUF_FALLBACK, 1ull);
    return false;
  }
  const bool ok32 = FP32 && (c >= m_chunk || eps32 <= MUF32_EPS1_MAX * (1.0 - 0x1p-12));  // (NaN fails)
  if (!__syncthreads_and(ok32)) {
    if (c < m_chunk) mu_slack[c] = -2.0;
    if (threadIdx.x == 0) atomicAdd(cnt + MUF_FP64FORM, 1ull);
    return false;
  }
  return true;
}

template <int DMAX>
__device__ __forceinline__ double mu_cand_norm(const gpx_kernel_params& p, const double* __restrict__ prep,
                                               const double* __restrict__ Xs, int64_t ldxs, int64_t c, int64_t m_chunk) {
  const double* __restrict__ gc = prep + MUF_CEN;
  double nbq = 0.0;
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    const double v = (k < p.d && c < m_chunk) ? Xs[c * ldxs + k] : 0.0;
    const double b = k < p.d ? v / p.lengthscale[k] - gc[k] : 0.0;
    nbq = fma(b, b, nbq);
  }
  return nbq;
}

// d <= 4 and d > 8: the classification alone (every eligible workgroup to mu_fact_kernel).
template <int DMAX>
__global__ void __launch_bounds__(WG) mu_class_kernel(gpx_kernel_params p, int n, double* __restrict__ prep,
                                                      const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                      double* __restrict__ mu_slack) {
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  double eps32;
  (void)mu_classify<false>(p, n, prep, mu_cand_norm<DMAX>(p, prep, Xs, ldxs, c, m_chunk), c, m_chunk, mu_slack, eps32);
}

// What the two factorised forms do differently in mu_fact_body: the fragments' element and accumulator types, the row
// blocks' records, the rows a lane sums in fp32 before the run goes to the fp64 sums, the MFMA, and how y leaves it.
template <int DMAX, bool FP32>
struct MuForm;
template <int DMAX>
struct MuForm<DMAX, false> {  // fp64 fragments; register r of the accumulator is row kq + 4 r of the row step
  using Elem = double;
  using Acc = d4;
  using Rec = MuFact<DMAX>;
  static constexpr int RUN = 16;
  static __device__ __forceinline__ const Elem* rec(const double* prep, int npad, int jb) {
    return mu_fact_rec<DMAX>(prep, npad, jb);
  }
  static __device__ __forceinline__ Acc mfma(Elem a, Elem b, Acc c) { return mfma16x16x4(a, b, c); }
  static __device__ __forceinline__ float y(const Acc& acc, int r) { return (float)acc[r]; }
  template <class... T>
  static __device__ __forceinline__ void pin(T&...) {}
};
template <int DMAX>
struct MuForm<DMAX, true> {  // fp32 fragments (proof: (g32) above); register r is row 4 kq + r (MuFact32's order)
  using Elem = float;
  using Acc = f4;
  using Rec = MuFact32<DMAX>;
  static constexpr int RUN = MUF32_RUN;
  static __device__ __forceinline__ const Elem* rec(const double* prep, int npad, int jb) {
    return mu_fact32_rec<DMAX>(prep, npad, jb);
  }
  static __device__ __forceinline__ Acc mfma(Elem a, Elem b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float y(const Acc& acc, int r) { return acc[r]; }
  // (an empty asm on each loaded register: without it hipcc moves the loads into the next trip, next to their uses,
  // and the loop waits for memory eight times per row block)
  static __device__ __forceinline__ void pin(float& a) { asm volatile("" : "+v"(a)); }
  static __device__ __forceinline__ void pin(float& a, float& b, float& c, float& d) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  }
};

// The factorised forms' loop.  Workgroup x: candidates 256 x .. 256 x + 255 against every row block, no LDS: a lane keeps
// the fragments of its wave's 64 candidates in registers for the whole kernel (the centre is the same for every row
// block) and reads the row blocks' fragments and alpha" from their records (every wave reads the same lines; the next
// block's are loaded before the current block's work).  The MFMAs of a row step are issued before the exponentials of the
// step before it.  Thread t ends up with the sums of its own candidate c0 + t (16-lane row kq holds candidate block cb =
// kq); nbq = |b|^2 and eps1 = eps1(c) resp. eps1_32(c) of that candidate.
template <int DMAX, bool FP32>
__device__ __forceinline__ void mu_fact_body(const gpx_kernel_params& p, int n, int npad,
                                             const double* __restrict__ prep, const double* __restrict__ Xs,
                                             int64_t ldxs, int64_t m_chunk, double* __restrict__ mu_approx,
                                             double* __restrict__ mu_slack, double nbq, double eps1) {
  using F = MuForm<DMAX, FP32>;
  using Elem = typename F::Elem;
  using Acc = typename F::Acc;
  constexpr int KS = DMAX / 4;
  const int d = p.d, t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * WG, c = c0 + t;
  const int nblk = (n + NB - 1) / NB;  // row blocks with a valid row
  const double* __restrict__ gc = prep + MUF_CEN;
  const int lane = t & 63, w = t >> 6, m = lane & 15, kq = lane >> 4;
  Elem bf[4][KS];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int64_t cc = c0 + 64 * w + 16 * cb + m;
      const int col = 4 * k + kq;
      const double v = (col < d && cc < m_chunk) ? Xs[cc * ldxs + col] : 0.0;
      bf[cb][k] = col < d ? (Elem)(v / p.lengthscale[col] - gc[col]) : (Elem)0;
    }
  Elem af[4][KS], afn[4][KS];
  float4 al[4], aln[4];
  auto load = [&](int jb, Elem(&a)[4][KS], float4(&l)[4]) {
    const Elem* __restrict__ in = F::rec(prep, npad, jb);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int k = 0; k < KS; ++k) a[s][k] = in[F::Rec::FRAG + (s * KS + k) * 64 + lane];
    const float4* __restrict__ ap = reinterpret_cast<const float4*>(in + F::Rec::AL) + 4 * kq;
#pragma unroll
    for (int s = 0; s < 4; ++s) l[s] = ap[s];
  };
  auto mm = [&](const Elem(&a)[KS], Acc(&acc)[4]) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      acc[cb] = Acc{0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < KS; ++k) acc[cb] = F::mfma(a[k], bf[cb][k], acc[cb]);
    }
  };
  float Sf[4], Af[4];
  double S[4] = {0.0, 0.0, 0.0, 0.0}, A[4] = {0.0, 0.0, 0.0, 0.0};
  auto entries = [&](const Acc(&acc)[4], const float4 l) {  // the lane's four rows of the step, alpha" in l
    const float lr[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const float e = __builtin_amdgcn_exp2f(F::y(acc[cb], r));
        Sf[cb] = fmaf(lr[r], e, Sf[cb]);
        Af[cb] = fmaf(fabsf(lr[r]), e, Af[cb]);
      }
  };
  auto flush = [&](bool again) {  // the fp32 runs to the fp64 sums
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      S[cb] += (double)Sf[cb];
      A[cb] += (double)Af[cb];
      if (again) Sf[cb] = Af[cb] = 0.0f;
    }
  };
  Acc acc0[4], acc1[4];
  load(0, af, al);
  mm(af[0], acc0);
#pragma unroll 1
  for (int jb = 0; jb < nblk; ++jb) {
    load(jb + 1 < nblk ? jb + 1 : jb, afn, aln);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) Sf[cb] = Af[cb] = 0.0f;
    mm(af[1], acc1);
    entries(acc0, al[0]);
    mm(af[2], acc0);
    entries(acc1, al[1]);
    if constexpr (F::RUN == 8) flush(true);
    mm(af[3], acc1);
    entries(acc0, al[2]);
    mm(afn[0], acc0);  // (the last block's again after the last: unused)
    entries(acc1, al[3]);
    flush(false);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      F::pin(aln[s].x, aln[s].y, aln[s].z, aln[s].w);
      al[s] = aln[s];
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        F::pin(afn[s][k]);
        af[s][k] = afn[s][k];
      }
    }
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    S[cb] += __shfl_xor(S[cb], 16);
    S[cb] += __shfl_xor(S[cb], 32);
    A[cb] += __shfl_xor(A[cb], 16);
    A[cb] += __shfl_xor(A[cb], 32);
  }
  if (c < m_chunk) {
    const double s = kq == 0 ? S[0] : kq == 1 ? S[1] : kq == 2 ? S[2] : S[3];
    const double a = kq == 0 ? A[0] : kq == 1 ? A[1] : kq == 2 ? A[2] : A[3];
    const double g = exp(-0.5 * nbq), scale = prep[MUF_SCALE], os = fabs(p.outputscale);
    const double at = (os * (scale * a)) * g;
    mu_approx[c] = (p.outputscale * (scale * s)) * g;
    mu_slack[c] = (eps1 * at + MUF_EPS2 * os * prep[MUF_L1]) * (1.0 + 0x1p-30);
  }
}

// The fp32 factorised form.  It classifies every workgroup first (mu_classify) and computes only those whose candidates
// all pass the fp32 form's limit.
template <int DMAX>
__global__ void __launch_bounds__(WG) mu_fact32_kernel(gpx_kernel_params p, int n, int npad, double* __restrict__ prep,
                                                       const double* __restrict__ Xs, int64_t ldxs, int64_t m_chunk,
                                                       double* __restrict__ mu_approx, double* __restrict__ mu_slack) {
  const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
  const double nbq = mu_cand_norm<DMAX>(p, prep, Xs, ldxs, c, m_chunk);
  double eps1;
  if (!mu_classify<true>(p, n, prep, nbq, c, m_chunk, mu_slack, eps1)) return;
  mu_fact_body<DMAX, true>(p, n, npad, prep, Xs, ldxs, m_chunk, mu_approx, mu_slack, nbq, eps1);
}

// The fp64 factorised form: only the workgroups mu_classify sent here.
template <int DMAX>
__global__ void __launch_bounds__(WG) mu_fact_kernel(gpx_kernel_params p, int n, int npad,
                                                     const double* __restrict__ prep, const double* __restrict__ Xs,
                                                     int64_t ldxs, int64_t m_chunk, double* __restrict__ mu_approx,
                                                     double* __restrict__ mu_slack) {
  const int64_t c0 = (int64_t)blockIdx.x * WG, c = c0 + threadIdx.x;
  // (the barrier: thread 0 writes mu_slack[c0] at the end, after every wave has read the flag)
  if (!__syncthreads_and(mu_slack[c0] == -2.0)) return;
  const double nbq = mu_cand_norm<DMAX>(p, prep, Xs, ldxs, c, m_chunk);
  double yc, q;
  const double eps1 = mu_eps1<false>(p, n, prep, nbq, yc, q);
  mu_fact_body<DMAX, false>(p, n, npad, prep, Xs, ldxs, m_chunk, mu_approx, mu_slack, nbq, eps1);
}

// The head phase's mean bound of q.m candidates (mu_colsum_kernel, mu_rowstat_kernel and mu_prep_kernel, then
// mu_fact32_kernel for the workgroups inside the fp32 form's limit (4 < d <= 8), mu_fact_kernel for the other eligible ones
// and mu_bound_kernel for the rest); prep: mu_prep_doubles(npad, d) doubles of scratch.
bool sweep_mu_bound_ok(const gpx_kernel_params& p) { return p.kind == GPX_KERNEL_RBF && !p.cov_fp32 && p.d <= 16; }

hipError_t launch_mu_bound(const SweepModel& M, const SweepCands& q, double* prep, double* mu_approx, double* mu_slack) {
  LaunchTimer tm(M.c, GPX_TIMER_KSTAR);
  const gpx_kernel_params& p = M.p;
  const int n = M.n, npad = M.npad;
  hipStream_t stream = M.c->stream;
  const unsigned nwg = (unsigned)((q.m + WG - 1) / WG);
  with_dmax(p.d, [&](auto D) {
    constexpr int DM = decltype(D)::value;
    if constexpr (DM <= 16) {  // (sweep_mu_bound_ok)
      mu_colsum_kernel<DM><<<npad / NB, WG, 0, stream>>>(p, n, npad, M.X, M.ldx, prep);
      mu_rowstat_kernel<DM><<<npad / NB, NB, 0, stream>>>(p, n, npad, M.X, M.ldx, M.alpha, prep);
      mu_prep_kernel<DM><<<npad / NB, WG, 0, stream>>>(p, n, npad, M.X, M.ldx, M.alpha, prep);
      // the first kernel over the candidates classifies every workgroup and, for 4 < d <= 8, computes those on the fp32
      // form; the two kernels behind it run the workgroups it flagged -2 and -1, the others returning at once
      if constexpr (mu_fp32_form(DM))
        mu_fact32_kernel<DM><<<nwg, WG, 0, stream>>>(p, n, npad, prep, q.Xs, q.ldxs, q.m, mu_approx, mu_slack);
      else
        mu_class_kernel<DM><<<nwg, WG, 0, stream>>>(p, n, prep, q.Xs, q.ldxs, q.m, mu_slack);
      mu_fact_kernel<DM><<<nwg, WG, 0, stream>>>(p, n, npad, prep, q.Xs, q.ldxs, q.m, mu_approx, mu_slack);
      mu_bound_kernel<DM><<<nwg, WG, 0, stream>>>(p, n, prep, q.Xs, q.ldxs, q.m, mu_approx, mu_slack);
    }
  });
  return hipGetLastError();
}

}  // namespace gpx
