// The pieces of rigid-body arithmetic that the pose update (k_se3.hip) and the conformer matching (k_match.hip) share: the rotation matrix of an
// axis-angle vector, the bond rotor step built on it (the update's rotor loop, randomize_kernel and match_eval) and the optimal rotation of a
// point-set pair from its 3 x 3 covariance (Horn 1987).
#pragma once
#include "model.h"

namespace ddk {

__device__ inline void axis_angle_to_matrix_dev(float ax, float ay, float az, float* R) {
  // utils/geometry.py:38-85 (quaternion route, small-angle series below 1e-6)
  const float ang = sqrtf(ax * ax + ay * ay + az * az);
  const float half = 0.5f * ang;
  const float s = fabsf(ang) < 1e-6f ? 0.5f - ang * ang / 48.0f : sinf(half) / ang;
  const float qr = cosf(half), qi = ax * s, qj = ay * s, qk = az * s;
  // the matrix of the fp32 quaternion assembled in fp64, one rounding per element: in fp32 (three to four roundings per element, as the reference does it)
  // |R R^T - I| reaches 10 * 2^-24 near a half turn (tests/test_gpu_geometry_adversarial.py), and the rotor loop multiplies such matrices R times per step
  const double r = qr, i = qi, j = qj, k = qk;
  const double two_s = 2.0 / (r * r + i * i + j * j + k * k);
  R[0] = (float)(1 - two_s * (j * j + k * k)); R[1] = (float)(two_s * (i * j - k * r)); R[2] = (float)(two_s * (i * k + j * r));
  R[3] = (float)(two_s * (i * j + k * r)); R[4] = (float)(1 - two_s * (i * i + k * k)); R[5] = (float)(two_s * (j * k - i * r));
  R[6] = (float)(two_s * (i * k - j * r)); R[7] = (float)(two_s * (j * k + i * r)); R[8] = (float)(1 - two_s * (i * i + j * j));
}

// The bond rotor step (utils/torsion.py:48-68) on the coordinates xyz [3 n]: the rotation by th about the axis xyz[u] - xyz[v] -> M [9], and its
// pivot xyz[v] -> piv [3].  A caller that skips zero angles tests th itself.
__device__ inline void bond_rotor(const float* xyz, int u, int v, float th, float* M, float* piv) {
  const float px = xyz[3 * v], py = xyz[3 * v + 1], pz = xyz[3 * v + 2];
  const float ax = xyz[3 * u] - px, ay = xyz[3 * u + 1] - py, az = xyz[3 * u + 2] - pz;
  const float nn = sqrtf(ax * ax + ay * ay + az * az);
  axis_angle_to_matrix_dev(ax / nn * th, ay / nn * th, az / nn * th, M);
  piv[0] = px; piv[1] = py; piv[2] = pz;
}

// (x, y, z) <- M ((x, y, z) - piv) + piv
__device__ inline void rotate_about(const float* M, const float* piv, float& x, float& y, float& z) {
  x -= piv[0]; y -= piv[1]; z -= piv[2];
  const float nx = M[0] * x + M[1] * y + M[2] * z + piv[0], ny = M[3] * x + M[4] * y + M[5] * z + piv[1], nz = M[6] * x + M[7] * y + M[8] * z + piv[2];
  x = nx; y = ny; z = nz;
}

// Horn 1987 for the covariance S[a][b] = sum a_i[a] b_i[b] of two centred point sets: the largest eigenvalue of a 4 x 4 symmetric matrix is
// sum_i (R a_i) . b_i at the rotation R minimising sum |R a_i - b_i|^2, and its eigenvector is that R as a quaternion.  Returns the eigenvalue; with VEC
// also writes R (row-major).  VEC = false runs the same sweeps without the eigenvector accumulation (R is not touched): all an RMSD needs,
// msd = (sum |a|^2 + sum |b|^2 - 2 lambda_max) / n.
template <bool VEC>
__device__ inline double horn_solve(const double* S, float* R) {
  double N[4][4] = {
      {S[0] + S[4] + S[8], S[5] - S[7], S[6] - S[2], S[1] - S[3]},
      {S[5] - S[7], S[0] - S[4] - S[8], S[1] + S[3], S[6] + S[2]},
      {S[6] - S[2], S[1] + S[3], -S[0] + S[4] - S[8], S[5] + S[7]},
      {S[1] - S[3], S[6] + S[2], S[5] + S[7], -S[0] - S[4] + S[8]}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  // Cyclic Jacobi.  A sweep costs six rotations of one sqrt + one rsqrt each on a single lane (the kernel's serial tail), so: the rotation
  // comes from (c, s) = (|r|, sgn(r) x) / sqrt(r^2 + x^2) with r = d + sgn(d) sqrt(d^2 + x^2), d = (N_qq - N_pp) / 2 - the textbook
  // t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) without its three divisions; an off-diagonal element below 2^-60 of its diagonal pair is left
  // alone (the rotation would be the identity in fp64); the sweeps end when the off-diagonal mass is below 1e-32 of the diagonal's.
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0, dg = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      dg += N[p][p] * N[p][p];
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off += N[p][q] * N[p][q];
    }
    if (off <= 1e-32 * dg || off < 1e-300) break;
    // (every index below is a compile-time constant after unrolling: N and V stay in registers - with rolled loops they lived in scratch memory)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double x = N[p][q];
        if (fabs(x) <= 8.7e-19 * (fabs(N[p][p]) + fabs(N[q][q]))) continue;
        const double d = 0.5 * (N[q][q] - N[p][p]);
        const double r = d + (d >= 0 ? 1.0 : -1.0) * sqrt(d * d + x * x);
        const double inv = rsqrt(r * r + x * x);
        const double c = fabs(r) * inv, s = (r >= 0 ? x : -x) * inv;
        // N <- G^T N G on the symmetric matrix: the two diagonal elements in closed form, the (p, q) element is zero by construction, the two
        // other rows / columns once (mirrored)
        const double app = N[p][p], aqq = N[q][q], cc = c * c, ss = s * s, cs2 = 2.0 * c * s * x;
        N[p][p] = cc * app - cs2 + ss * aqq;
        N[q][q] = ss * app + cs2 + cc * aqq;
        N[p][q] = 0.0; N[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k == p || k == q) continue;
          const double a = N[k][p], b = N[k][q];
          const double np_ = c * a - s * b, nq_ = s * a + c * b;
          N[k][p] = np_; N[p][k] = np_; N[k][q] = nq_; N[q][k] = nq_;
        }
        if constexpr (VEC) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double a = V[k][p], b = V[k][q];
            V[k][p] = c * a - s * b; V[k][q] = s * a + c * b;
          }
        }
      }
  }
  double top = N[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > top) { top = N[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
  if constexpr (VEC) {
    const double nn = w * w + x * x + y * y + z * z, s2 = 2.0 / nn;
    R[0] = (float)(1 - s2 * (y * y + z * z)); R[1] = (float)(s2 * (x * y - z * w)); R[2] = (float)(s2 * (x * z + y * w));
    R[3] = (float)(s2 * (x * y + z * w)); R[4] = (float)(1 - s2 * (x * x + z * z)); R[5] = (float)(s2 * (y * z - x * w));
    R[6] = (float)(s2 * (x * z - y * w)); R[7] = (float)(s2 * (y * z + x * w)); R[8] = (float)(1 - s2 * (x * x + y * y));
  }
  return top;
}

// rotation R minimising sum |R a_i - b_i|^2 given S
__device__ inline void horn_rotation(const double* S, float* R) { horn_solve<true>(S, R); }

__device__ inline double horn_top_eigenvalue(const double* S) { return horn_solve<false>(S, nullptr); }

}  // namespace ddk
