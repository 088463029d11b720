// The forward half of the diffusion: NoiseTransform.apply_noise's draws with their score targets, and loss_function (see include/ddk.h:
// ddk_torus_score, ddk_rng_perturbation, ddk_score_matching_loss; the IGSO(3) rows the rotation reads come from ddk_so3_rows, k_so3.hip):
//   torus_score_kernel          torus.score(x, sigma) (utils/torus.py:43-52) per element, the table entry evaluated on the spot in fp64
//   rng_perturbation_kernel     tr / rot / tor updates of one noising of B samples from the counter-based generator (k_philox.h, purposes 6-8 with the
//                               draw index in the step field) and data.tr_score / rot_score / tor_score (datasets_utils/pdbbind.py:47-56)
//   score_matching_loss_kernel  the six per-sample terms of loss_function(..., apply_mean=False) (utils/training.py:21-53), one wave per sample
// and their forms for a ragged batch of G different complexes at G noise levels (ddk_rng_perturbation_batch, ddk_score_matching_loss_batch and its backward;
// the per-graph scalars and prefix tables are device arrays), which call the same device functions and give a graph the bits of the per-sample call:
//   rng_perturbation_batch_kernel                one workgroup per graph
//   score_matching_loss_batch_kernel             one wave per graph
//   score_matching_loss_batch_backward_kernel    element-wise over the predictions
// ddk_rng_forward_times (purpose 11, the diffusion time of a complex) is computed on the host from k_philox.h.
// Every value is a pure function of its inputs: no state, no atomics, fixed reduction orders, so the same bits on every run and under any cut by samples.
#include <math.h>

#include <mutex>
#include <vector>

#include "k_philox.h"
#include "model.h"

namespace ddk {

enum RngForwardPurpose : uint32_t { RNG_FWD_TRANSLATION = 6, RNG_FWD_ROTATION = 7, RNG_FWD_TORSION = 8, RNG_FWD_TIME = 11 };      // DDK_RNG_LAYOUT 1, beside RngPurpose

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

// One sample's noising, as one item of it sees it: the generator's coordinates, the noise level, and the sample's OWN rows of the six outputs
// (tr / rot [3], tor [n_rot]).  rng_perturbation_kernel (B samples of one complex at one level) and rng_perturbation_batch_kernel (G graphs, each at its
// own level) both fill one and call perturbation_item, so that a graph of a batch gets the bits of the same sample noised alone.
struct PerturbSample {
  RngStream S; uint32_t sample, draw; int n_rot; float tr_sigma, tor_sigma; TorusGrid T; const double *cdf, *score;
  float *tr_update, *rot_update, *tor_update, *tr_score, *rot_score, *tor_score;
};

// item j of a sample, with n_tor_blk = ceil(n_rot / 4): j < n_tor_blk the torsion block j, j = n_tor_blk the rotation, j = n_tor_blk + 1 the translation
__device__ inline void perturbation_item(const PerturbSample& P, int j, int n_tor_blk) {
  uint32_t w[4];
  float z[4];
  if (j < n_tor_blk) {
    rng_block(P.S, P.sample, RNG_FWD_TORSION, P.draw, (uint32_t)j, w);
    rng_normals(w, z);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 4 * j + q;
      if (r < P.n_rot) {
        const float upd = P.tor_sigma * z[q];
        P.tor_update[r] = upd;
        if (P.tor_score) P.tor_score[r] = (float)torus_score_f64((double)upd, P.T);
      }
    }
  } else if (j == n_tor_blk) {
    rng_block(P.S, P.sample, RNG_FWD_ROTATION, P.draw, 0, w);
    rng_normals(w, z);
    rng_block(P.S, P.sample, RNG_FWD_ROTATION, P.draw, 1, w);
    const double u = (double)rng_uniform(w[0]);
    const double a[3] = {(double)z[0], (double)z[1], (double)z[2]};
    const double n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    double upd[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    if (n2 >= 0x1p-60) {
      const auto omegas = [](int k) { return k == SO3_ROW - 1 ? M_PI : (double)(k + 1) * (M_PI / SO3_ROW); };
      const double *cdf = P.cdf, *score = P.score;
      const double omega = interp_f64(u, [cdf](int k) { return cdf[k]; }, omegas, SO3_ROW);      // so3.sample: np.interp(u, cdf row, omegas)
      const double norm = sqrt(n2);
#pragma unroll
      for (int e = 0; e < 3; ++e) upd[e] = a[e] / norm * omega;
      if (P.rot_score) {      // so3.score_vec: np.interp(omega, omegas, score row) * vec / omega
        const double s = interp_f64(omega, omegas, [score](int k) { return score[k]; }, SO3_ROW);
#pragma unroll
        for (int e = 0; e < 3; ++e) sc[e] = s * upd[e] / omega;
      }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      P.rot_update[e] = (float)upd[e];
      if (P.rot_score) P.rot_score[e] = (float)sc[e];
    }
  } else {
    rng_block(P.S, P.sample, RNG_FWD_TRANSLATION, P.draw, 0, w);
    rng_normals(w, z);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float upd = P.tr_sigma * z[e];
      P.tr_update[e] = upd;
      if (P.tr_score) P.tr_score[e] = -upd / (P.tr_sigma * P.tr_sigma);
    }
  }
}

// item = b * per + j with per = n_tor_blk + 2: item j of sample b (perturbation_item)
__global__ __launch_bounds__(NOISING_THREADS) void rng_perturbation_kernel(PerturbArgs A) {
  const int n_tor_blk = (A.n_rot + 3) >> 2;
  const int per = n_tor_blk + 2;
  const int64_t items = (int64_t)A.B * per;
  for (int64_t it = (int64_t)blockIdx.x * NOISING_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * NOISING_THREADS) {
    const int j = (int)(it % per);
    const int64_t b = it / per;
    const auto row = [b](float* p, int w) { return p ? p + b * w : nullptr; };
    const PerturbSample P{A.S, A.sample0 + (uint32_t)b, A.draw, A.n_rot, A.tr_sigma, A.tor_sigma, A.T, A.cdf, A.score,
                          row(A.out.tr_update, 3), row(A.out.rot_update, 3), row(A.out.tor_update, A.n_rot),
                          row(A.out.tr_score, 3), row(A.out.rot_score, 3), row(A.out.tor_score, A.n_rot)};
    perturbation_item(P, j, n_tor_blk);
  }
}

// ddk_rng_perturbation_batch: graph g of the batch is the sample sample[g] of stream stream_id[g] at its own noise level, with R_g = tor_ptr[g + 1] -
// tor_ptr[g] torsions.  One workgroup per graph; its threads take the graph's items.  Every per-graph entry is checked before it becomes an address or a
// table index (the tables are device arrays the host never sees): a graph with a broken entry gets NaN updates and nothing else.
struct PerturbBatchArgs {
  uint32_t seed_lo, seed_hi, draw; int G, T, n_rows;
  const uint64_t* stream_id; const int32_t *sample, *tor_ptr, *torus_sigma_idx, *so3_row; const float *tr_sigma, *tor_sigma;
  const double *torus_sigma, *cdf_rows, *score_rows;      // torus_sigma: the grid's 5001 sigmas (torus_grid(i).sigma, computed on the host)
  TorusGrid T0;                                           // the grid's constants; sigma is the graph's own
  ddk_perturbation out;
};

__global__ __launch_bounds__(NOISING_THREADS) void rng_perturbation_batch_kernel(PerturbBatchArgs A) {
  const int g = blockIdx.x;
  const int t0 = A.tor_ptr[g], t1 = A.tor_ptr[g + 1], n_rot = t1 - t0, idx = A.torus_sigma_idx[g], row = A.so3_row[g], sample = A.sample[g];
  const float tr_sigma = A.tr_sigma[g], tor_sigma = A.tor_sigma[g];
  const bool ok = t0 >= 0 && t1 >= t0 && t1 <= A.T && n_rot <= RNG_MAX_COLS && idx >= 0 && idx <= TORUS_SIGMA_N && row >= 0 && row < A.n_rows &&
                  sample >= 0 && tr_sigma > 0.f && tor_sigma > 0.f && isfinite(tr_sigma) && isfinite(tor_sigma);
  if (!ok) {
    if (threadIdx.x < 3) { A.out.tr_update[3 * g + threadIdx.x] = NAN; A.out.rot_update[3 * g + threadIdx.x] = NAN; }
    return;
  }
  const uint64_t sid = A.stream_id[g];
  TorusGrid T = A.T0;
  T.sigma = A.torus_sigma[idx];
  const auto at = [](float* p, int64_t off) { return p ? p + off : nullptr; };
  const PerturbSample P{RngStream{A.seed_lo, A.seed_hi, (uint32_t)sid, (uint32_t)(sid >> 32)}, (uint32_t)sample, A.draw, n_rot, tr_sigma, tor_sigma, T,
                        A.cdf_rows + (size_t)row * SO3_ROW, A.score_rows ? A.score_rows + (size_t)row * SO3_ROW : nullptr,
                        A.out.tr_update + 3 * g, A.out.rot_update + 3 * g, at(A.out.tor_update, t0),
                        at(A.out.tr_score, 3 * g), at(A.out.rot_score, 3 * g), at(A.out.tor_score, t0)};
  const int n_tor_blk = (n_rot + 3) >> 2;
  for (int j = threadIdx.x; j < n_tor_blk + 2; j += NOISING_THREADS) perturbation_item(P, j, n_tor_blk);
}

struct LossArgs {
  int B, n_rot; const float *tr_pred, *rot_pred, *tor_pred, *tr_score, *rot_score, *tor_score; double tr_sigma, so3_norm, torus_norm2; float* out;
};

// one wave per sample, in fp64, each term rounded once to fp32: lane 0 the two means of three, all lanes the torsion sums (lane k takes torsions k, k + 64,
// ... in ascending order, then a shuffle tree of fixed shape)
// (one row = one sample of score_matching_loss_kernel or one graph of score_matching_loss_batch_kernel: the pointers are the row's own, so both give the
// same bits for the same operands.  Called by all 64 lanes of a wave.)
__device__ inline void score_matching_loss_row(int lane, int n_rot, const float* tr_pred, const float* rot_pred, const float* tor_pred, const float* tr_score,
                                               const float* rot_score, const float* tor_score, double tr_sigma, double so3_norm, double torus_norm2,
                                               float* o) {
  double tor = 0.0, tor_base = 0.0;
  if (tor_pred && n_rot > 0) {
    for (int r = lane; r < n_rot; r += 64) {
      const double s = (double)tor_score[r], d = (double)tor_pred[r] - s;
      tor += d * d / torus_norm2;
      tor_base += s * s / torus_norm2;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      tor += __shfl_down(tor, off, 64);
      tor_base += __shfl_down(tor_base, off, 64);
    }
    tor /= (double)n_rot + 1e-4;
    tor_base /= (double)n_rot + 1e-4;
  }
  if (lane != 0) return;
  double tr = 0.0, tr_base = 0.0, rot = 0.0, rot_base = 0.0;
  const double s2 = tr_sigma * tr_sigma;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double ts = (double)tr_score[e], td = (double)tr_pred[e] - ts;
    tr += td * td * s2;
    tr_base += ts * ts * s2;
    const double rs = (double)rot_score[e] / so3_norm, rd = ((double)rot_pred[e] - (double)rot_score[e]) / so3_norm;
    rot += rd * rd;
    rot_base += rs * rs;
  }
  o[0] = (float)(tr / 3.0); o[1] = (float)(rot / 3.0); o[2] = (float)tor;
  o[3] = (float)(tr_base / 3.0); o[4] = (float)(rot_base / 3.0); o[5] = (float)tor_base;
}

__global__ __launch_bounds__(NOISING_THREADS) void score_matching_loss_kernel(LossArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (NOISING_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= A.B) return;      // whole waves leave: the shuffles below see full waves
  const bool tor = A.tor_pred && A.n_rot > 0;
  score_matching_loss_row(lane, A.n_rot, A.tr_pred + b * 3, A.rot_pred + b * 3, tor ? A.tor_pred + b * A.n_rot : nullptr, A.tr_score + b * 3,
                          A.rot_score + b * 3, tor ? A.tor_score + b * A.n_rot : nullptr, A.tr_sigma, A.so3_norm, A.torus_norm2, A.out + b * 6);
}

// ddk_score_matching_loss_batch: row g is a graph with its own three scalars and its own R_g = tor_ptr[g + 1] - tor_ptr[g] torsions at tor_ptr[g] of the flat
// torsion arrays.  A graph whose tor_ptr entries are not a range inside [0, T], or that has a scalar that is not positive, gets a row of NaN.
struct LossBatchArgs {
  int G, T; const int32_t* tor_ptr; const float *tr_pred, *rot_pred, *tor_pred, *tr_score, *rot_score, *tor_score, *tr_sigma, *so3_norm, *torus_norm2; float* out;
};

__global__ __launch_bounds__(NOISING_THREADS) void score_matching_loss_batch_kernel(LossBatchArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (NOISING_THREADS / 64) + (threadIdx.x >> 6);
  if (g >= A.G) return;
  const int t0 = A.tor_ptr[g], t1 = A.tor_ptr[g + 1];
  const float tr_sigma = A.tr_sigma[g], so3_norm = A.so3_norm[g], torus_norm2 = A.torus_norm2[g];
  if (!(t0 >= 0 && t1 >= t0 && t1 <= A.T && t1 - t0 <= RNG_MAX_COLS && tr_sigma > 0.f && so3_norm > 0.f && torus_norm2 > 0.f)) {
    if (lane < 6) A.out[g * 6 + lane] = NAN;
    return;
  }
  const bool tor = A.tor_pred && t1 > t0;
  score_matching_loss_row(lane, t1 - t0, A.tr_pred + g * 3, A.rot_pred + g * 3, tor ? A.tor_pred + t0 : nullptr, A.tr_score + g * 3, A.rot_score + g * 3,
                          tor ? A.tor_score + t0 : nullptr, (double)tr_sigma, (double)so3_norm, (double)torus_norm2, A.out + g * 6);
}

// the derivative of the three loss columns by the predictions, times the incoming gradient g [G, 3] of those columns: element-wise, in fp64, rounded once
//   d tr_loss[g] / d tr_pred[g][k] = 2 (pred - score) tr_sigma^2 / 3      d rot_loss[g] / d rot_pred[g][k] = 2 (pred - score) / so3_norm^2 / 3
//   d tor_loss[g] / d tor_pred[r]  = 2 (pred - score) / torus_norm2 / (R_g + 1e-4)      (r a torsion of graph g, found by bisection in tor_ptr)
// items [0, 3G) translation, [3G, 6G) rotation, [6G, 6G + T) torsion; a destination that is NULL is not computed
struct LossBatchBwdArgs {
  int G, T; const int32_t* tor_ptr; const float *grad, *tr_pred, *rot_pred, *tor_pred, *tr_score, *rot_score, *tor_score, *tr_sigma, *so3_norm, *torus_norm2;
  float *grad_tr, *grad_rot, *grad_tor;
};

__global__ __launch_bounds__(NOISING_THREADS) void score_matching_loss_batch_backward_kernel(LossBatchBwdArgs A) {
  const int64_t items = 6 * (int64_t)A.G + A.T;
  for (int64_t it = (int64_t)blockIdx.x * NOISING_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * NOISING_THREADS) {
    if (it < 3 * (int64_t)A.G) {
      if (!A.grad_tr) continue;
      const int g = (int)(it / 3);
      const double s = (double)A.tr_sigma[g];
      A.grad_tr[it] = (float)(2.0 * ((double)A.tr_pred[it] - (double)A.tr_score[it]) * (s * s) / 3.0 * (double)A.grad[3 * g]);
    } else if (it < 6 * (int64_t)A.G) {
      if (!A.grad_rot) continue;
      const int64_t i = it - 3 * (int64_t)A.G;
      const int g = (int)(i / 3);
      const double n = (double)A.so3_norm[g];
      A.grad_rot[i] = (float)(2.0 * ((double)A.rot_pred[i] - (double)A.rot_score[i]) / (n * n) / 3.0 * (double)A.grad[3 * g + 1]);
    } else {
      if (!A.grad_tor) continue;
      const int r = (int)(it - 6 * (int64_t)A.G);
      int lo = 0, hi = A.G;      // the graph of torsion r: the last g with tor_ptr[g] <= r (empty graphs before it share that start and are passed over)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.tor_ptr[mid] <= r) lo = mid; else hi = mid;
      }
      const int n_rot = A.tor_ptr[lo + 1] - A.tor_ptr[lo];
      float out = NAN;      // a tor_ptr that is not the prefix the forward accepted
      if (A.tor_ptr[lo] <= r && r < A.tor_ptr[lo + 1])
        out = (float)(2.0 * ((double)A.tor_pred[r] - (double)A.tor_score[r]) / (double)A.torus_norm2[lo] / ((double)n_rot + 1e-4) * (double)A.grad[3 * lo + 2]);
      A.grad_tor[r] = out;
    }
  }
}

// the 5001 sigmas of the torus grid on the device: rng_perturbation_batch_kernel reads its graphs' sigma indices from device memory, and the sigma of an index
// must be the HOST's (torus_grid: the host's pow and log10), or a graph of a batch would not get the bits of ddk_rng_perturbation.  Filled by the first batch
// call on each device (40 kB, a blocking copy, once per process and device).
__device__ double g_torus_sigma[TORUS_SIGMA_N + 1];
constexpr int TORUS_TABLE_MAX_DEVICES = 64;
static std::mutex g_torus_sigma_mutex;
static bool g_torus_sigma_ready[TORUS_TABLE_MAX_DEVICES];

static hipError_t torus_sigma_table(int device, const double** out) {
  if (device < 0 || device >= TORUS_TABLE_MAX_DEVICES) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(g_torus_sigma_mutex);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess && !g_torus_sigma_ready[device]) {
    std::vector<double> host(TORUS_SIGMA_N + 1);
    for (int i = 0; i <= TORUS_SIGMA_N; ++i) host[i] = torus_grid(i).sigma;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_torus_sigma), host.data(), host.size() * sizeof(double));
    g_torus_sigma_ready[device] = e == hipSuccess;
  }
  if (e == hipSuccess) e = hipGetSymbolAddress((void**)out, HIP_SYMBOL(g_torus_sigma));
  return e;
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

int ddk_rng_perturbation_batch(ddk_ctx* ctx, uint64_t seed, int32_t G, const uint64_t* stream_id, const int32_t* sample, const int32_t* tor_ptr, int32_t T,
                               int32_t draw, const float* tr_sigma, const float* tor_sigma, const int32_t* torus_sigma_idx, const int32_t* so3_row,
                               int32_t n_rows, const double* so3_cdf_rows, const double* so3_score_rows, const ddk_perturbation* out, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (G < 1 || G > NOISE_BATCH_MAX_GRAPHS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: G must be in [1, " + std::to_string(NOISE_BATCH_MAX_GRAPHS) + "]");
  if (T < 0 || (int64_t)T > (int64_t)G * RNG_MAX_COLS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: T must be in [0, G * " + std::to_string(RNG_MAX_COLS) + "]");
  if (draw < 0 || draw >= RNG_MAX_STEPS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: draw must be in [0, " + std::to_string(RNG_MAX_STEPS) + ")");
  if (n_rows < 1 || n_rows > NOISE_BATCH_MAX_ROWS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: n_rows must be in [1, " + std::to_string(NOISE_BATCH_MAX_ROWS) + "]");
  if (!stream_id || !sample || !tor_ptr || !tr_sigma || !tor_sigma || !torus_sigma_idx || !so3_row)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: null per-graph table (stream_id, sample, tor_ptr, tr_sigma, tor_sigma, torus_sigma_idx, so3_row)");
  if (!out || !out->tr_update || !out->rot_update || (!out->tor_update && T > 0))
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: null output (only the score members, and tor_update with T = 0, may be null)");
  if (!so3_cdf_rows || (!so3_score_rows && out->rot_score))
    return fail(ctx, DDK_ERR_INVALID, "ddk_rng_perturbation_batch: null IGSO(3) rows (so3_score_rows may be null only without rot_score)");
  const double* sigmas = nullptr;
  hipError_t e = torus_sigma_table(ctx->cfg.device, &sigmas);
  if (e != hipSuccess) return hip_fail(ctx, e, "rng_perturbation_batch: the torus sigma grid");
  PerturbBatchArgs A{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, G, T, n_rows, stream_id, sample, tor_ptr, torus_sigma_idx, so3_row,
                     tr_sigma, tor_sigma, sigmas, so3_cdf_rows, so3_score_rows, torus_grid(0), *out};
  hipLaunchKernelGGL(rng_perturbation_batch_kernel, dim3(G), dim3(NOISING_THREADS), 0, (hipStream_t)stream, A);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "rng_perturbation_batch launch");
  return DDK_OK;
}

int ddk_rng_forward_times(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id, int32_t sample, int32_t draw, float* t_out) {
  if (!ctx) return DDK_ERR_INVALID;
  if (n < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_forward_times: n must be >= 0");
  if (sample < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_forward_times: sample must be >= 0");
  if (draw < 0 || draw >= RNG_MAX_STEPS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_forward_times: draw must be in [0, " + std::to_string(RNG_MAX_STEPS) + ")");
  if (n > 0 && (!stream_id || !t_out)) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_forward_times: null argument");
  for (int32_t i = 0; i < n; ++i) {
    uint32_t w[4];
    rng_block(rng_stream(seed, stream_id[i]), (uint32_t)sample, RNG_FWD_TIME, (uint32_t)draw, 0, w);
    t_out[i] = rng_uniform(w[0]);
  }
  return DDK_OK;
}

// what the forward and the backward of the ragged loss check alike
static int loss_batch_guard(ddk_ctx* ctx, const char* who, int32_t G, int32_t T, const int32_t* tor_ptr, const float* tr_pred, const float* rot_pred,
                            const float* tor_pred, const float* tr_score, const float* rot_score, const float* tor_score, const float* tr_sigma,
                            const float* so3_score_norm, const float* torus_score_norm2) {
  const std::string w = std::string(who) + ": ";
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (G < 1 || G > NOISE_BATCH_MAX_GRAPHS) return fail(ctx, DDK_ERR_INVALID, w + "G must be in [1, " + std::to_string(NOISE_BATCH_MAX_GRAPHS) + "]");
  if (T < 0 || (int64_t)T > (int64_t)G * RNG_MAX_COLS) return fail(ctx, DDK_ERR_INVALID, w + "T must be in [0, G * " + std::to_string(RNG_MAX_COLS) + "]");
  if (!tor_ptr || !tr_pred || !rot_pred || !tr_score || !rot_score || !tr_sigma || !so3_score_norm || !torus_score_norm2)
    return fail(ctx, DDK_ERR_INVALID, w + "null argument (tor_ptr, tr_pred, rot_pred, tr_score, rot_score, tr_sigma, so3_score_norm, torus_score_norm2)");
  if (tor_pred && T > 0 && !tor_score) return fail(ctx, DDK_ERR_INVALID, w + "tor_pred without tor_score");
  return DDK_OK;
}

int ddk_score_matching_loss_batch(ddk_ctx* ctx, int32_t G, const int32_t* tor_ptr, int32_t T, const float* tr_pred, const float* rot_pred,
                                  const float* tor_pred, const float* tr_score, const float* rot_score, const float* tor_score, const float* tr_sigma,
                                  const float* so3_score_norm, const float* torus_score_norm2, float* out, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  const int rc = loss_batch_guard(ctx, "ddk_score_matching_loss_batch", G, T, tor_ptr, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma,
                                  so3_score_norm, torus_score_norm2);
  if (rc != DDK_OK) return rc;
  if (!out) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss_batch: null output (out)");
  LossBatchArgs A{G, T, tor_ptr, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2, out};
  const int per = NOISING_THREADS / 64;
  hipLaunchKernelGGL(score_matching_loss_batch_kernel, dim3((G + per - 1) / per), dim3(NOISING_THREADS), 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "score_matching_loss_batch launch");
  return DDK_OK;
}

int ddk_score_matching_loss_batch_backward(ddk_ctx* ctx, int32_t G, const int32_t* tor_ptr, int32_t T, const float* grad, const float* tr_pred,
                                           const float* rot_pred, const float* tor_pred, const float* tr_score, const float* rot_score,
                                           const float* tor_score, const float* tr_sigma, const float* so3_score_norm, const float* torus_score_norm2,
                                           float* grad_tr_pred, float* grad_rot_pred, float* grad_tor_pred, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  const int rc = loss_batch_guard(ctx, "ddk_score_matching_loss_batch_backward", G, T, tor_ptr, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score,
                                  tr_sigma, so3_score_norm, torus_score_norm2);
  if (rc != DDK_OK) return rc;
  if (!grad) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss_batch_backward: null argument (grad)");
  if (grad_tor_pred && T > 0 && !tor_pred) return fail(ctx, DDK_ERR_INVALID, "ddk_score_matching_loss_batch_backward: grad_tor_pred without tor_pred");
  if (!grad_tr_pred && !grad_rot_pred && !(grad_tor_pred && T > 0)) return DDK_OK;      // nothing asked for
  LossBatchBwdArgs A{G, grad_tor_pred ? T : 0, tor_ptr, grad, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm,
                     torus_score_norm2, grad_tr_pred, grad_rot_pred, grad_tor_pred};
  hipLaunchKernelGGL(score_matching_loss_batch_backward_kernel, dim3(noising_grid(6 * (int64_t)G + A.T)), dim3(NOISING_THREADS), 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "score_matching_loss_batch_backward launch");
  return DDK_OK;
}

}  // extern "C"
