// The top eigenvalue of Horn's 4 x 4 matrix, which is all conformer matching's objective needs (csrc/k_match.hip): the Jacobi of csrc/k_geom.h
// (horn_top_eigenvalue) against a Newton iteration on the characteristic polynomial (Theobald 2005, "QCP").  Both in fp64, every lane of a wave on the
// same matrix, as match_eval calls it.  Prints, per class of point-set pair, the latency of one solve (one wave, 1024 dependent solves), the time per
// solve with the chip full (65536 waves), and what the two make of the RMSD.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I disco_diffdock_amd/csrc -I include tools/probes/horn_eigen_probe.hip -o tools/probes/horn_eigen_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "k_geom.h"

// lambda_max by Newton from (Ga + Gb) / 2 >= lambda_max on P(l) = l^4 + c2 l^2 + c1 l + c0, the characteristic polynomial of the traceless matrix:
// c2 = -2 sum S_ij^2, c1 = -8 det S, c0 = det N.  At most 50 steps.
__device__ inline double newton_top_eigenvalue(const double* S, double start) {
  const double N[4][4] = {
      {S[0] + S[4] + S[8], S[5] - S[7], S[6] - S[2], S[1] - S[3]},
      {S[5] - S[7], S[0] - S[4] - S[8], S[1] + S[3], S[6] + S[2]},
      {S[6] - S[2], S[1] + S[3], -S[0] + S[4] - S[8], S[5] + S[7]},
      {S[1] - S[3], S[6] + S[2], S[5] + S[7], -S[0] - S[4] + S[8]}};
  double c2 = 0;
  for (int i = 0; i < 9; ++i) c2 += S[i] * S[i];
  c2 *= -2.0;
  const double detS = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  const double c1 = -8.0 * detS;
  // det N by the 2 x 2 minors of its upper and lower row pairs
  const double s0 = N[0][0] * N[1][1] - N[1][0] * N[0][1], s1 = N[0][0] * N[1][2] - N[1][0] * N[0][2], s2 = N[0][0] * N[1][3] - N[1][0] * N[0][3];
  const double s3 = N[0][1] * N[1][2] - N[1][1] * N[0][2], s4 = N[0][1] * N[1][3] - N[1][1] * N[0][3], s5 = N[0][2] * N[1][3] - N[1][2] * N[0][3];
  const double t5 = N[2][2] * N[3][3] - N[3][2] * N[2][3], t4 = N[2][1] * N[3][3] - N[3][1] * N[2][3], t3 = N[2][1] * N[3][2] - N[3][1] * N[2][2];
  const double t2 = N[2][0] * N[3][3] - N[3][0] * N[2][3], t1 = N[2][0] * N[3][2] - N[3][0] * N[2][2], t0 = N[2][0] * N[3][1] - N[3][0] * N[2][1];
  const double c0 = s0 * t5 - s1 * t4 + s2 * t3 + s3 * t2 - s4 * t1 + s5 * t0;
  double l = start;
  for (int it = 0; it < 50; ++it) {
    const double l2 = l * l, p = (l2 + c2) * l2 + c1 * l + c0, dp = (4.0 * l2 + 2.0 * c2) * l + c1;
    if (dp == 0.0) break;
    const double nl = l - p / dp;
    const bool stop = fabs(nl - l) <= 1e-15 * fabs(nl);
    l = nl;
    if (stop) break;
  }
  return l;
}

// in [n][11]: S[9], Ga, Gb.  NEWTON selects the solver; `chain` solves run one after the other in every wave (each perturbed by the one before, so that
// they stay dependent); out[m] = the first solve's eigenvalue.
template <bool NEWTON>
__global__ __launch_bounds__(256) void solve_kernel(const double* in, int n, int chain, double* out) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= n) return;
  double S[9], first = 0, carry = 0;
  for (int k = 0; k < chain; ++k) {
    const double* row = in + (size_t)((wave + k) % n) * 11;
    for (int i = 0; i < 9; ++i) S[i] = row[i] + carry * 1e-300;
    const double lam = NEWTON ? newton_top_eigenvalue(S, 0.5 * (row[9] + row[10])) : ddk::horn_top_eigenvalue(S);
    if (k == 0) first = lam;
    carry = lam;
  }
  if ((threadIdx.x & 63) == 0) out[wave] = first + carry * 1e-300;
}

struct Pair { std::vector<double> a, b; };

static void covariance(const Pair& p, double* row) {
  const int n = (int)p.a.size() / 3;
  double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) { ca[c] += p.a[3 * i + c] / n; cb[c] += p.b[3 * i + c] / n; }
  for (int i = 0; i < 11; ++i) row[i] = 0;
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < 3; ++r) {
      const double x = p.a[3 * i + r] - ca[r], y = p.b[3 * i + r] - cb[r];
      row[9] += x * x; row[10] += y * y;
      for (int c = 0; c < 3; ++c) row[3 * r + c] += x * (p.b[3 * i + c] - cb[c]);
    }
}

int main() {
  const int n = 65536, atoms = 24;
  const char* names[] = {"unrelated sets", "noisy copy (0.15 per coordinate)", "exact rotated copy", "planar exact copy"};
  std::mt19937_64 gen(1);
  std::normal_distribution<double> nd(0.0, 1.0);
  double *d_in, *d_out;
  hipMalloc(&d_in, sizeof(double) * 11 * n);
  hipMalloc(&d_out, sizeof(double) * n);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int cls = 0; cls < 4; ++cls) {
    std::vector<double> in((size_t)n * 11);
    for (int m = 0; m < n; ++m) {
      Pair p;
      p.a.resize(3 * atoms); p.b.resize(3 * atoms);
      for (auto& v : p.a) v = 3.0 * nd(gen);
      if (cls == 3) for (int i = 0; i < atoms; ++i) p.a[3 * i + 2] = 0.0;
      double q[4] = {nd(gen), nd(gen), nd(gen), nd(gen)};
      const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (auto& v : q) v /= qn;
      const double w = q[0], x = q[1], y = q[2], z = q[3];
      const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                           2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
      for (int i = 0; i < atoms; ++i)
        for (int r = 0; r < 3; ++r) {
          double v = R[3 * r] * p.a[3 * i] + R[3 * r + 1] * p.a[3 * i + 1] + R[3 * r + 2] * p.a[3 * i + 2] + 5.0;
          if (cls == 0) v = 3.0 * nd(gen);
          if (cls == 1) v += 0.15 * nd(gen);
          p.b[3 * i + r] = v;
        }
      covariance(p, &in[(size_t)m * 11]);
    }
    hipMemcpy(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice);
    std::vector<double> lam[2] = {std::vector<double>(n), std::vector<double>(n)};
    float full_us[2], chain_us[2];
    for (int s = 0; s < 2; ++s) {
      for (int rep = 0; rep < 3; ++rep) {      // the last of three
        hipEventRecord(e0);
        if (s) hipLaunchKernelGGL(solve_kernel<true>, dim3(n / 4), dim3(256), 0, 0, d_in, n, 1, d_out);
        else hipLaunchKernelGGL(solve_kernel<false>, dim3(n / 4), dim3(256), 0, 0, d_in, n, 1, d_out);
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&full_us[s], e0, e1);
      }
      hipMemcpy(lam[s].data(), d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
      for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        if (s) hipLaunchKernelGGL(solve_kernel<true>, dim3(1), dim3(64), 0, 0, d_in, n, 1024, d_out);
        else hipLaunchKernelGGL(solve_kernel<false>, dim3(1), dim3(64), 0, 0, d_in, n, 1024, d_out);
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&chain_us[s], e0, e1);
      }
    }
    double worst_l = 0, worst_r = 0, res_j = 0, res_n = 0;
    for (int m = 0; m < n; ++m) {
      const double g = in[(size_t)m * 11 + 9] + in[(size_t)m * 11 + 10];
      const double rj = std::sqrt(std::fmax(0.0, (g - 2 * lam[0][m]) / atoms)), rn = std::sqrt(std::fmax(0.0, (g - 2 * lam[1][m]) / atoms));
      worst_l = std::fmax(worst_l, std::fabs(lam[0][m] - lam[1][m]) / std::fabs(lam[0][m]));
      worst_r = std::fmax(worst_r, std::fabs(rj - rn));
      res_j = std::fmax(res_j, rj); res_n = std::fmax(res_n, rn);
    }
    printf("%-34s latency per solve: Jacobi %.2f us, Newton %.2f us (1024 dependent solves, one wave); chip full: Jacobi %.1f ns, Newton %.1f ns per wave-solve; "
           "max |dlambda| / lambda %.1e, max |dRMSD| %.1e A", names[cls], chain_us[0] * 1e3 / 1024, chain_us[1] * 1e3 / 1024, full_us[0] * 1e6 / n,
           full_us[1] * 1e6 / n, worst_l, worst_r);
    if (cls >= 2) printf("; true RMSD 0: largest RMSD Jacobi %.2e A, Newton %.2e A", res_j, res_n);
    printf("\n");
  }
  return 0;
}
