// Probe: the rounding of v_mfma_f32_16x16x4_f32 as mu_fact32_kernel uses it (gpx_mubound.hip, (g32)): a chain of KS = 1
// or 2 instructions on a zero accumulator, so a dot product of d = 4 KS fp32 pairs.  The proof assumes no more than the
// standard model, |yhat - sum a_i b_i| <= gamma_d sum |a_i b_i| with gamma_d = d v / (1 - d v), v = 2^-24.  This runs the
// chain on adversarial fp32 inputs, compares with the exact dot product of the same fp32 inputs (every product of two
// floats is exact in fp64; their sum is taken in long double) and prints, per family, the largest error in units of
// v sum |a_i b_i|: a figure above d would refute the model.  Denormal operands are measured against the bound the proof
// uses for them, 2^-126 (|a_i| + |b_i| + 1) per coordinate on top of the model's term.
//   hipcc --offload-arch=gfx950 -O2 -o tools/probes/mfma_f32_probe tools/probes/mfma_f32_probe.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n",hipGetErrorString(e),__LINE__); exit(1);}}while(0)

// Trial b: A is 16 x (4 KS) row-major, B is (4 KS) x 16 row-major, C 16 x 16 row-major.
// Lane l holds A[l & 15][4 k + (l >> 4)] and B[4 k + (l >> 4)][l & 15]; register r of lane l is C[4 (l >> 4) + r][l & 15].
template <int KS>
__global__ void __launch_bounds__(64) chain_k(const float* __restrict__ A, const float* __restrict__ B,
                                              float* __restrict__ C) {
  const int l = threadIdx.x;
  const float* a = A + (size_t)blockIdx.x * 16 * 4 * KS;
  const float* b = B + (size_t)blockIdx.x * 16 * 4 * KS;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < KS; ++k)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(l & 15) * 4 * KS + 4 * k + (l >> 4)],
                                               b[(4 * k + (l >> 4)) * 16 + (l & 15)], acc, 0, 0, 0);
  float* c = C + (size_t)blockIdx.x * 256;
  for (int r = 0; r < 4; ++r) c[(4 * (l >> 4) + r) * 16 + (l & 15)] = acc[r];
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static double unif() { return (double)(rnd() >> 11) * 0x1p-53; }
static float mant() { return (float)(1.0 + unif()); }  // [1, 2), a full 24-bit mantissa
static float sgn() { return (rnd() & 1) ? -1.0f : 1.0f; }

enum Family { CANCEL, ONE_LARGE, SPREAD, SIGNS, DENORMAL, NFAM };
static const char* NAMES[NFAM] = {"cancelling pairs", "one large, many small", "magnitudes over 2^40", "random signs",
                                  "denormal operands"};

// One row of A (d values) and the matching column of B (filled per family so that the d products have the pattern).
static void fill(Family f, int d, float* a, float* b) {
  switch (f) {
    case CANCEL:  // products in pairs of nearly opposite value: a_{2i+1} b_{2i+1} ~ -a_{2i} b_{2i}
      for (int i = 0; i < d; i += 2) {
        a[i] = mant() * sgn(), b[i] = mant();
        a[i + 1] = -a[i] * (1.0f + (float)((int)(rnd() % 5) - 2) * 0x1p-23f), b[i + 1] = b[i] * (1.0f + (float)(rnd() % 3) * 0x1p-23f);
      }
      break;
    case ONE_LARGE: {
      const int big = (int)(rnd() % d);
      for (int i = 0; i < d; ++i) {
        a[i] = mant() * sgn() * (i == big ? 1.0f : ldexpf(1.0f, -(int)(rnd() % 26)));
        b[i] = mant();
      }
    } break;
    case SPREAD:
      for (int i = 0; i < d; ++i) {
        a[i] = mant() * sgn() * ldexpf(1.0f, (int)(rnd() % 41) - 20);
        b[i] = mant() * ldexpf(1.0f, (int)(rnd() % 41) - 20);
      }
      break;
    case SIGNS:
      for (int i = 0; i < d; ++i) a[i] = mant() * sgn(), b[i] = mant() * sgn();
      break;
    default:  // denormal fragments, and normal ones whose product is denormal, beside ordinary terms
      for (int i = 0; i < d; ++i) {
        const int kind = (int)(rnd() % 4);
        if (kind == 0) a[i] = mant() * sgn() * ldexpf(1.0f, -127 - (int)(rnd() % 20)), b[i] = mant() * ldexpf(1.0f, (int)(rnd() % 9));
        else if (kind == 1) a[i] = mant() * sgn() * ldexpf(1.0f, -70), b[i] = mant() * ldexpf(1.0f, -60 - (int)(rnd() % 10));
        else if (kind == 2) a[i] = mant() * sgn() * ldexpf(1.0f, -120), b[i] = mant() * ldexpf(1.0f, -(int)(rnd() % 8));
        else a[i] = 0.0f, b[i] = mant();
      }
  }
}

template <int KS>
static void run(int trials) {
  const int d = 4 * KS;
  std::vector<float> A((size_t)trials * 16 * d), B((size_t)trials * 16 * d), C((size_t)trials * 256);
  float *dA, *dB, *dC;
  CK(hipMalloc(&dA, A.size() * 4)); CK(hipMalloc(&dB, B.size() * 4)); CK(hipMalloc(&dC, C.size() * 4));
  for (int f = 0; f < NFAM; ++f) {
    // rows of A and columns of B are filled as pairs (row i with column i); every (row i, column j) pair is measured, the
    // matched pairs i = j carry the family's pattern, the others are further random-sign cases of the same magnitudes
    std::vector<float> ra(d), cb(d);
    for (int tr = 0; tr < trials; ++tr)
      for (int i = 0; i < 16; ++i) {
        fill((Family)f, d, ra.data(), cb.data());
        for (int k = 0; k < d; ++k) {
          A[((size_t)tr * 16 + i) * d + k] = ra[k];
          B[((size_t)tr * d + k) * 16 + i] = cb[k];
        }
      }
    CK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
    chain_k<KS><<<trials, 64>>>(dA, dB, dC);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(C.data(), dC, C.size() * 4, hipMemcpyDeviceToHost));
    double worst_diag = 0.0, worst_all = 0.0;
    for (int tr = 0; tr < trials; ++tr)
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
          long double s = 0.0L;
          double sabs = 0.0, den = 0.0;
          for (int k = 0; k < d; ++k) {
            const double pa = A[((size_t)tr * 16 + i) * d + k], pb = B[((size_t)tr * d + k) * 16 + j];
            s += (long double)(pa * pb);
            sabs += fabs(pa * pb);
            den += 0x1p-126 * (fabs(pa) + fabs(pb) + 1.0);
          }
          const double err = fabs((double)((long double)C[(size_t)tr * 256 + i * 16 + j] - s));
          double ratio;
          if (f == DENORMAL) {
            const double gam = d * 0x1p-24 / (1.0 - d * 0x1p-24);
            ratio = err / (gam * sabs + den);  // against the proof's whole bound: must be <= 1
          } else {
            ratio = sabs > 0.0 ? err / (0x1p-24 * sabs) : 0.0;  // in units of v sum |a_i b_i|: the model says <= d
          }
          if (ratio > worst_all) worst_all = ratio;
          if (i == j && ratio > worst_diag) worst_diag = ratio;
        }
    printf("MFMA_F32 KS=%d d=%d %-24s max err = %.4f (patterned pairs), %.4f (all 256 pairs) %s\n", KS, d, NAMES[f],
           worst_diag, worst_all, f == DENORMAL ? "of gamma_d sum|ab| + 2^-126 sum(|a|+|b|+1)" : "x v sum|a_i b_i|");
  }
  CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dC));
}

int main() {
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  printf("device %s %s\n", p.name, p.gcnArchName);
  run<1>(2048);
  run<2>(2048);
  printf("PROBE DONE\n");
  return 0;
}
