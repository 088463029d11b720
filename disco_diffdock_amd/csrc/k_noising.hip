// The forward half of the diffusion: NoiseTransform.apply_noise's draws with their score targets, and loss_function (see include/ddk.h:
// ddk_torus_score, ddk_rng_perturbation, ddk_score_matching_loss; the IGSO(3) rows the rotation reads come from ddk_so3_rows, k_so3.hip):
//   torus_score_kernel          torus.score(x, sigma) (utils/torus.py:43-52) per element, the table entry evaluated on the spot in fp64
//   rng_perturbation_kernel     tr / rot / tor updates of one noising of B samples from the counter-based generator (k_philox.h, purposes 6-8 with the
//                               draw index in the step field) and data.tr_score / rot_score / tor_score (datasets_utils/pdbbind.py:47-56)
//   score_matching_loss_kernel  the six per-sample terms of loss_function(..., apply_mean=False) (utils/training.py:21-53), one wave per sample
// Every value is a pure function of its inputs: no state, no atomics, fixed reduction orders, so the same bits on every run and under any cut by samples.
#include <math.h>

#include "k_philox.h"
#include "model.h"

namespace ddk {

enum RngForwardPurpose : uint32_t { RNG_FWD_TRANSLATION = 6, RNG_FWD_ROTATION = 7, RNG_FWD_TORSION = 8 };      // DDK_RNG_LAYOUT 1, beside RngPurpose

constexpr int NOISING_THREADS = 256;
constexpr int64_t NOISING_MAX_GRID = 1 << 16;
constexpr int SO3_ROW = 2000;                     // angles of an IGSO(3) row: omega_j = pi (j + 1) / 2000
constexpr int TORUS_X_N = 5000, TORUS_SIGMA_N = 5000, TORUS_TERMS = 100;
constexpr double TORUS_X_MIN = 1e-5, TORUS_SIGMA_MIN = 3e-3, TORUS_SIGMA_MAX = 2.0;

// the host's part of torus.py's grids, in fp64: sigma of the chosen row, and the constants of the x grid 10 ** linspace(log10(X_MIN), 0, 5001) * pi
struct TorusGrid { double sigma, x_start, x_step, ln_x_min; };

static TorusGrid torus_grid(int sigma_idx) {
  const double s0 = log10(TORUS_SIGMA_MIN), s1 = log10(TORUS_SIGMA_MAX), sstep = (s1 - s0) / TORUS_SIGMA_N;
  TorusGrid T;
  T.sigma = pow(10.0, sigma_idx == TORUS_SIGMA_N ? s1 : (double)sigma_idx * sstep + s0) * M_PI;
  T.x_start = log10(TORUS_X_MIN);
  T.x_step = (0.0 - T.x_start) / TORUS_X_N;
  T.ln_x_min = log(TORUS_X_MIN);
  return T;
}

static unsigned noising_grid(int64_t items) {
  const int64_t g = (items + NOISING_THREADS - 1) / NOISING_THREADS;
  return (unsigned)(g < 1 ? 1 : (g > NOISING_MAX_GRID ? NOISING_MAX_GRID : g));
}

// -sign(x) * score_[sigma, x_idx] of torus.py, every operation in fp64 as written there: wrap to [-pi, pi), quantise |x| on the natural-log grid (clip, round
// half to even), grad / p with 201 terms in ascending i at that grid point.  x == 0: 0.  p underflows to 0: NaN, as in the reference's table.
__device__ inline double torus_score_f64(double x, const TorusGrid& T) {
#pragma clang fp contract(off)
  if (!isfinite(x)) return NAN;
  const double two_pi = 2 * M_PI;
  double y = fmod(x + M_PI, two_pi);      // Python's %: the result takes the divisor's sign
  if (y < 0) y += two_pi;
  x = y - M_PI;
  if (x == 0) return 0.0;
  const double sign = x > 0 ? 1.0 : -1.0;
  double q = (log(fabs(x) / M_PI) - T.ln_x_min) / (0 - T.ln_x_min) * TORUS_X_N;
  q = q < 0 ? 0 : (q > TORUS_X_N ? TORUS_X_N : q);
  const int idx = (int)rint(q);
  const double xg = pow(10.0, idx == TORUS_X_N ? 0.0 : (double)idx * T.x_step + T.x_start) * M_PI;
  const double s2 = T.sigma * T.sigma;
  double p = 0.0, g = 0.0;
  for (int i = -TORUS_TERMS; i <= TORUS_TERMS; ++i) {
    const double v = xg + two_pi * i;
    const double e = exp(-(v * v) / 2 / s2);
    p += e;
    g += v / s2 * e;
  }
  return -sign * (g / p);
}

__global__ __launch_bounds__(NOISING_THREADS) void torus_score_kernel(int64_t n, const float* __restrict__ x, TorusGrid T, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * NOISING_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NOISING_THREADS)
    out[i] = (float)torus_score_f64((double)x[i], T);
}

// np.interp(x, xp, fp) on n points with the bracket found by bisection for the first xp[j] >= x; clamped at both ends.  XP, FP: j -> xp[j], fp[j]
template <typename XP, typename FP>
__device__ inline double interp_f64(double x, XP xp, FP fp, int n) {
#pragma clang fp contract(off)
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xp(mid) >= x) hi = mid; else lo = mid + 1;
  }
  if (lo == 0) return fp(0);
  if (lo == n) return fp(n - 1);
  const int j = lo - 1;
  return (fp(j + 1) - fp(j)) / (xp(j + 1) - xp(j)) * (x - xp(j)) + fp(j);
}

struct PerturbArgs {
  RngStream S; uint32_t sample0; int B; uint32_t draw; int n_rot; float tr_sigma, tor_sigma; TorusGrid T;
  const double *cdf, *score; ddk_perturbation out;
};

// item = b * per + j with per = n_tor_blk + 2: j < n_tor_blk the torsion block j of sample b, j = n_tor_blk its rotation, j = n_tor_blk + 1 its translation
__global__ __launch_bounds__(NOISING_THREADS) void rng_perturbation_kernel(PerturbArgs A) {
  const int n_tor_blk = (A.n_rot + 3) >> 2;
  const int per = n_tor_blk + 2;
  const int64_t items = (int64_t)A.B * per;
  for (int64_t it = (int64_t)blockIdx.x * NOISING_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * NOISING_THREADS) {
    const int j = (int)(it % per);
    const int64_t b = it / per;
    const uint32_t sample = A.sample0 + (uint32_t)b;
    uint32_t w[4];
    float z[4];
    if (j < n_tor_blk) {
      rng_block(A.S, sample, RNG_FWD_TORSION, A.draw, (uint32_t)j, w);
      rng_normals(w, z);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 4 * j + q;
        if (r < A.n_rot) {
          const float upd = A.tor_sigma * z[q];
          A.out.tor_update[b * A.n_rot + r] = upd;
          if (A.out.tor_score) A.out.tor_score[b * A.n_rot + r] = (float)torus_score_f64((double)upd, A.T);
        }
      }
    } else if (j == n_tor_blk) {
      rng_block(A.S, sample, RNG_FWD_ROTATION, A.draw, 0, w);
      rng_normals(w, z);
      rng_block(A.S, sample, RNG_FWD_ROTATION, A.draw, 1, w);
      const double u = (double)rng_uniform(w[0]);
      const double a[3] = {(double)z[0], (double)z[1], (double)z[2]};
      const double n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
      double upd[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
      if (n2 >= 0x1p-60) {
        const auto omegas = [](int k) { return k == SO3_ROW - 1 ? M_PI : (double)(k + 1) * (M_PI / SO3_ROW); };
        const double *cdf = A.cdf, *score = A.score;
        const double omega = interp_f64(u, [cdf](int k) { return cdf[k]; }, omegas, SO3_ROW);      // so3.sample: np.interp(u, cdf row, omegas)
        const double norm = sqrt(n2);
#pragma unroll
        for (int e = 0; e < 3; ++e) upd[e] = a[e] / norm * omega;
        if (A.out.rot_score) {      // so3.score_vec: np.interp(omega, omegas, score row) * vec / omega
          const double s = interp_f64(omega, omegas, [score](int k) { return score[k]; }, SO3_ROW);
#pragma unroll
          for (int e = 0; e < 3; ++e) sc[e] = s * upd[e] / omega;
        }
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        A.out.rot_update[b * 3 + e] = (float)upd[e];
        if (A.out.rot_score) A.out.rot_score[b * 3 + e] = (float)sc[e];
      }
    } else {
      rng_block(A.S, sample, RNG_FWD_TRANSLATION, A.draw, 0, w);
      rng_normals(w, z);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float upd = A.tr_sigma * z[e];
        A.out.tr_update[b * 3 + e] = upd;
        if (A.out.tr_score) A.out.tr_score[b * 3 + e] = -upd / (A.tr_sigma * A.tr_sigma);
      }
    }
  }
}

struct LossArgs {
  int B, n_rot; const float *tr_pred, *rot_pred, *tor_pred, *tr_score, *rot_score, *tor_score; double tr_sigma, so3_norm, torus_norm2; float* out;
};

// one wave per sample, in fp64, each term rounded once to fp32: lane 0 the two means of three, all lanes the torsion sums (lane k takes torsions k, k + 64,
// ... in ascending order, then a shuffle tree of fixed shape)
__global__ __launch_bounds__(NOISING_THREADS) void score_matching_loss_kernel(LossArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (NOISING_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= A.B) return;      // whole waves leave: the shuffles below see full waves
  double tor = 0.0, tor_base = 0.0;
  if (A.tor_pred && A.n_rot > 0) {
    for (int r = lane; r < A.n_rot; r += 64) {
      const double s = (double)A.tor_score[b * A.n_rot + r], d = (double)A.tor_pred[b * A.n_rot + r] - s;
      tor += d * d / A.torus_norm2;
      tor_base += s * s / A.torus_norm2;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      tor += __shfl_down(tor, off, 64);
      tor_base += __shfl_down(tor_base, off, 64);
    }
    tor /= (double)A.n_rot + 1e-4;
    tor_base /= (double)A.n_rot + 1e-4;
  }
  if (lane != 0) return;
  double tr = 0.0, tr_base = 0.0, rot = 0.0, rot_base = 0.0;
  const double s2 = A.tr_sigma * A.tr_sigma;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double ts = (double)A.tr_score[b * 3 + e], td = (double)A.tr_pred[b * 3 + e] - ts;
    tr += td * td * s2;
    tr_base += ts * ts * s2;
    const double rs = (double)A.rot_score[b * 3 + e] / A.so3_norm, rd = ((double)A.rot_pred[b * 3 + e] - (double)A.rot_score[b * 3 + e]) / A.so3_norm;
    rot += rd * rd;
    rot_base += rs * rs;
  }
  float* o = A.out + b * 6;
  o[0] = (float)(tr / 3.0); o[1] = (float)(rot / 3.0); o[2] = (float)tor;
  o[3] = (float)(tr_base / 3.0); o[4] = (float)(rot_base / 3.0); o[5] = (float)tor_base;
}

}  // namespace ddk

using namespace ddk;

extern "C" {

int ddk_torus_score(ddk_ctx* ctx, int64_t n, const float* x, int32_t sigma_idx, float* score_out, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (n < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_torus_score: n must be >= 0");
  if (sigma_idx < 0 || sigma_idx > TORUS_SIGMA_N) return fail(ctx, DDK_ERR_INVALID, "ddk_torus_score: sigma_idx must be in [0, " + std::to_string(TORUS_SIGMA_N) + "]");
  if (n > 0 && (!x || !score_out)) return fail(ctx, DDK_ERR_INVALID, "ddk_torus_score: null argument");
  if (n == 0) return DDK_OK;
  hipLaunchKernelGGL(torus_score_kernel, dim3(noising_grid(n)), dim3(NOISING_THREADS), 0, (hipStream_t)stream, n, x, torus_grid(sigma_idx), score_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "torus_score launch");
  return DDK_OK;
}

int ddk_rng_perturbation(ddk_ctx* ctx, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t B, int32_t draw, int32_t n_rot, float tr_sigma,
                         float tor_sigma, int32_t torus_sigma_idx, const double* so3_cdf_row, const double* so3_score_row, const ddk_perturbation* out,
                         void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (B < 1) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: B must be >= 1");
  if (sample0 < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: sample0 must be >= 0");
  if ((int64_t)sample0 + B > (int64_t)INT32_MAX) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: sample0 + B must be <= 2^31 - 1");
  if (draw < 0 || draw >= RNG_MAX_STEPS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: draw must be in [0, " + std::to_string(RNG_MAX_STEPS) + ")");
  if (n_rot < 0 || n_rot > RNG_MAX_COLS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: n_rot must be in [0, " + std::to_string(RNG_MAX_COLS) + "]");
  if (!(tr_sigma > 0.f) || !(tor_sigma > 0.f) || !isfinite(tr_sigma) || !isfinite(tor_sigma))
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: tr_sigma and tor_sigma must be positive and finite");
  if (torus_sigma_idx < 0 || torus_sigma_idx > TORUS_SIGMA_N)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: torus_sigma_idx must be in [0, " + std::to_string(TORUS_SIGMA_N) + "]");
  if (!out || !out->tr_update || !out->rot_update || (!out->tor_update && n_rot > 0))
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: null output (only the score members, and tor_update with n_rot = 0, may be null)");
  if (!so3_cdf_row || (!so3_score_row && out->rot_score))
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation: null IGSO(3) row (so3_score_row may be null only without rot_score)");
  PerturbArgs A{rng_stream(seed, stream_id), (uint32_t)sample0, B, (uint32_t)draw, n_rot, tr_sigma, tor_sigma, torus_grid(torus_sigma_idx),
                so3_cdf_row, so3_score_row, *out};
  const int64_t items = (int64_t)B * (((n_rot + 3) >> 2) + 2);
  hipLaunchKernelGGL(rng_perturbation_kernel, dim3(noising_grid(items)), dim3(NOISING_THREADS), 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "rng_perturbation launch");
  return DDK_OK;
}

int ddk_score_matching_loss(ddk_ctx* ctx, int32_t B, int32_t n_rot, const float* tr_pred, const float* rot_pred, const float* tor_pred,
                            const float* tr_score, const float* rot_score, const float* tor_score, float tr_sigma, float so3_score_norm,
                            float torus_score_norm2, float* out, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (B < 1) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss: B must be >= 1");
  if (n_rot < 0 || n_rot > RNG_MAX_COLS) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss: n_rot must be in [0, " + std::to_string(RNG_MAX_COLS) + "]");
  if (!tr_pred || !rot_pred || !tr_score || !rot_score || !out) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss: null argument");
  if (tor_pred && n_rot > 0 && !tor_score) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss: tor_pred without tor_score");
  if (!(tr_sigma > 0.f) || !(so3_score_norm > 0.f) || !(torus_score_norm2 > 0.f))
    return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss: tr_sigma, so3_score_norm and torus_score_norm2 must be positive");
  LossArgs A{B, n_rot, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, (double)tr_sigma, (double)so3_score_norm, (double)torus_score_norm2, out};
  const int per = NOISING_THREADS / 64;
  hipLaunchKernelGGL(score_matching_loss_kernel, dim3((B + per - 1) / per), dim3(NOISING_THREADS), 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "score_matching_loss launch");
  return DDK_OK;
}

}  // extern "C"
