// The IGSO(3) rows of utils/so3.py on the device, in fp64 (see include/ddk.h: ddk_so3_rows): for a noise level eps the truncated series
//   f(omega)      = sum_l (2l + 1) exp(-l (l + 1) eps^2) sin((l + 1/2) omega) / sin(omega / 2)                 _expansion, so3.py:21-25
//   pdf(omega)    = f (1 - cos omega) / pi                                                                     _density(marginal), :28-30
//   cdf           = cumsum(pdf) / 2000 * pi                                                                    :58
//   score(omega)  = (sum_l (2l + 1) exp(-l (l + 1) eps^2) (lo dhi - hi dlo) / lo^2) / f                        _score, :35-43
//   exp_score_norm = sqrt(sum(score^2 pdf) / sum(pdf) / pi)                                                    :61
// on the 2000 angles omega_j = pi (j + 1) / 2000, L = 2000 terms.  One workgroup per row.  Every (row, omega) element is accumulated by ONE thread with l
// ascending and every term as the reference writes it (no contraction into FMAs): that order reproduces the reference's tables bit for bit on the host,
// and here to the last bits of the device library's sin / cos / exp.  The weights (2l + 1) exp(-l (l + 1) eps^2) of the row sit in LDS; the cumulative sum
// and the two sums of the norm are serial loops of one thread each, in index order: 2000 additions against 4 million sine / cosine pairs per row.
// No atomics: the same bits on every run.
// Where the density vanishes f is what rounding leaves of 2000 cancelling terms, and score^2 pdf = dSigma^2 (1 - cos omega) / (pi f) of such an entry is
// unbounded as that remainder comes close to 0: one entry in a few hundred thousand outweighs 1e-10 of its row's sum (rows 44 and 55 of the reference's own
// _exp_score_norms carry such a term).  The norm therefore counts an entry only if its score is finite AND |f| > 2^-40 sum_l |term_l|, i.e. f stands a factor
// 1000 above the rounding noise of its own sum; the entries left out hold less than 1e-10 of the sum.
#include <math.h>

#include "model.h"

namespace ddk {

constexpr int SO3_N_EPS = 1000, SO3_X_N = 2000, SO3_L = 2000;
constexpr double SO3_MIN_EPS = 0.01, SO3_MAX_EPS = 2.0;
constexpr int SO3_THREADS = 1024;
constexpr int SO3_ROWS_PER_LAUNCH = 256;      // eps of a launch's rows travel as a kernel argument (the row list is a HOST array and the call allocates nothing)
constexpr int SO3_MAX_ROWS = 4096;
constexpr double SO3_NOISE_GUARD = 0x1p-40;      // an entry enters exp_score_norm only if |f| > this * sum_l |term_l|

struct So3Eps { double eps[SO3_ROWS_PER_LAUNCH]; };

// np.linspace(0, pi, 2001)[1:]: arange * step, the last entry set to the end point
__device__ inline double so3_omega(int j) { return j == SO3_X_N - 1 ? M_PI : (double)(j + 1) * (M_PI / SO3_X_N); }

__global__ __launch_bounds__(SO3_THREADS) void so3_rows_kernel(So3Eps E, int row0, double* __restrict__ cdf_out, double* __restrict__ score_out,
                                                               double* __restrict__ esn_out) {
#pragma clang fp contract(off)
  __shared__ double w[SO3_L], pdf[SO3_X_N], sc[SO3_X_N];
  __shared__ uint8_t counts[SO3_X_N];      // the entry enters the norm: f above the rounding noise of its sum (file comment)
  const int tid = threadIdx.x;
  const double eps = E.eps[blockIdx.x];
  const int64_t row = (int64_t)row0 + blockIdx.x;
  const double eps2 = eps * eps;
  for (int l = tid; l < SO3_L; l += SO3_THREADS) w[l] = (double)(2 * l + 1) * exp((double)(-l * (l + 1)) * eps2);
  __syncthreads();
  for (int j = tid; j < SO3_X_N; j += SO3_THREADS) {
    const double omega = so3_omega(j);
    const double lo = sin(omega / 2), dlo = 0.5 * cos(omega / 2), lo2 = lo * lo;
    double p = 0.0, ds = 0.0, amp = 0.0;
    for (int l = 0; l < SO3_L; ++l) {
      const double h = (double)l + 0.5, wl = w[l];
      double hi, c;
      sincos(omega * h, &hi, &c);
      const double dhi = h * c;
      const double term = wl * hi / lo;
      p += term;
      amp += fabs(term);
      ds += wl * (lo * dhi - hi * dlo) / lo2;
    }
    pdf[j] = p * (1.0 - cos(omega)) / M_PI;
    sc[j] = ds / p;      // inf / NaN where the expansion cancels to 0: the reference's dead tail, kept as it is
    counts[j] = fabs(p) > SO3_NOISE_GUARD * amp;
  }
  __syncthreads();
  if (tid == 0) {      // np.cumsum: serial, in index order; the weights are done with, their array takes the result
    double run = 0.0;
    for (int j = 0; j < SO3_X_N; ++j) {
      run += pdf[j];
      w[j] = run / SO3_X_N * M_PI;
    }
  } else if (tid == 64 && esn_out) {      // another wave: the norm over the entries that count
    double num = 0.0, den = 0.0;
    for (int j = 0; j < SO3_X_N; ++j) {
      const double s = sc[j], q = pdf[j];
      den += q;
      if (counts[j] && isfinite(s)) num += s * s * q;
    }
    esn_out[row] = sqrt(num / den / M_PI);
  }
  __syncthreads();
  for (int j = tid; j < SO3_X_N; j += SO3_THREADS) {
    if (cdf_out) cdf_out[row * SO3_X_N + j] = w[j];
    if (score_out) score_out[row * SO3_X_N + j] = sc[j];
  }
}

// 10 ** np.linspace(log10(MIN_EPS), log10(MAX_EPS), N_EPS)[i] in fp64 on the host
static double so3_eps(int i) {
  const double start = log10(SO3_MIN_EPS), stop = log10(SO3_MAX_EPS), step = (stop - start) / (SO3_N_EPS - 1);
  return pow(10.0, i == SO3_N_EPS - 1 ? stop : (double)i * step + start);
}

}  // namespace ddk

using namespace ddk;

extern "C" int ddk_so3_rows(ddk_ctx* ctx, int32_t n_rows, const int32_t* eps_idx, double* cdf_out, double* score_out, double* exp_score_norm_out,
                            void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (n_rows < 1 || n_rows > SO3_MAX_ROWS) return fail(ctx, DDK_ERR_INVALID, "ddk_so3_rows: n_rows must be in [1, " + std::to_string(SO3_MAX_ROWS) + "]");
  if (!eps_idx) return fail(ctx, DDK_ERR_INVALID, "ddk_so3_rows: null eps_idx");
  if (!cdf_out && !score_out && !exp_score_norm_out) return fail(ctx, DDK_ERR_INVALID, "ddk_so3_rows: at least one output must not be null");
  for (int i = 0; i < n_rows; ++i)
    if (eps_idx[i] < 0 || eps_idx[i] >= SO3_N_EPS)
      return fail(ctx, DDK_ERR_INVALID, "ddk_so3_rows: eps_idx[" + std::to_string(i) + "] must be in [0, " + std::to_string(SO3_N_EPS) + ")");
  for (int r0 = 0; r0 < n_rows; r0 += SO3_ROWS_PER_LAUNCH) {
    const int n = n_rows - r0 < SO3_ROWS_PER_LAUNCH ? n_rows - r0 : SO3_ROWS_PER_LAUNCH;
    So3Eps E;
    for (int i = 0; i < SO3_ROWS_PER_LAUNCH; ++i) E.eps[i] = i < n ? so3_eps(eps_idx[r0 + i]) : 0.0;
    hipLaunchKernelGGL(so3_rows_kernel, dim3(n), dim3(SO3_THREADS), 0, (hipStream_t)stream, E, r0, cdf_out, score_out, exp_score_norm_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "so3_rows launch");
  }
  return DDK_OK;
}
