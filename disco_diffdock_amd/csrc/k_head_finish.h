// The finish of the two score heads from their accumulator rows (reference models/score_model.py:272-286, 302-307), element by element: the scalar
// pieces that heads_post_kernel (k_heads.hip, 64 threads per row) and the POST block of se3_update_kernel (k_se3.hip, 256 threads over chunks of 64 rows)
// both run.  Arithmetic only: each kernel keeps its own thread mapping, LDS rows and barriers.  Every accumulator that is read is cleared behind the read.
#pragma once
#include "model.h"

namespace ddk {

// tor_bond_conv: element c of a bond's row, mean over its ne neighbour atoms and BatchNorm
__device__ inline float tor_bn_element(const HeadArgs& H, float* row, int ne, int c) {
  const float s = row[c] / (float)(ne > 1 ? ne : 1);
  row[c] = 0.0f;
  return (s - H.md.tb_bn_mean[c]) * H.md.tb_bn_scale[c] + H.md.tb_bn_bias[c];
}

// tor_final_layer, Linear(48,24,no bias) -> tanh -> Linear(24,1,no bias): hidden unit k times its output weight, from the row's 48 elements v
__device__ inline float tor_hidden_unit(const HeadArgs& H, const float* v, int k) {
  float a = 0.0f;
  for (int j = 0; j < 2 * NS; ++j) a += H.md.tf_w0[k * 2 * NS + j] * v[j];
  return H.md.tf_w3[k] * tanhf(a);
}

// ... and the sum of the 24 weighted hidden units: the bond's torsion score
__device__ inline float tor_score_sum(const HeadArgs& H, const float* hid) {
  float o = 0.0f;
  for (int j = 0; j < NS; ++j) o += hid[j];
  if (H.scale_by_sigma) o *= H.sp.torus_norm_sqrt;
  return o;
}

// final_conv: element c < 12 of graph b's row, mean over the ligand atoms and BatchNorm scale
__device__ inline float center_element(const HeadArgs& H, float* row, int c) {
  const float g = (row[c] / (float)H.n_lig) * H.md.fc_bn_scale[c / 3];
  row[c] = 0.0f;
  return g;
}

// which = 0: the translation score of graph b from g12, which = 1: its rotation score (score_model.py:274-286): direction times the magnitude MLP of the norm.
// (H by value: through a reference heads_post_kernel needed 70 VGPRs instead of 64 and lost an occupancy step)
__device__ inline void tr_rot_score(const HeadArgs H, const float* g12, int which, int b) {
  const int o = 3 * which;
  const float px = g12[o] + g12[6 + o], py = g12[o + 1] + g12[7 + o], pz = g12[o + 2] + g12[8 + o];
  const float nrm = sqrtf(px * px + py * py + pz * pz);
  const float* w0n = which == 0 ? H.md.tr_w0n : H.md.rot_w0n;
  const float* w3 = which == 0 ? H.md.tr_w3 : H.md.rot_w3;
  const float* sb = which == 0 ? H.sp.tr_sigb : H.sp.rot_sigb;
  float s = which == 0 ? H.md.tr_b3 : H.md.rot_b3;
  for (int k = 0; k < NS; ++k) s += w3[k] * fmaxf(w0n[k] * nrm + sb[k], 0.0f);
  float f = s / nrm;
  if (H.scale_by_sigma) f = which == 0 ? f / H.sp.tr_sigma : f * H.sp.so3_norm;
  float* out = (which == 0 ? H.tr_out : H.rot_out) + 3 * (size_t)b;
  out[0] = px * f; out[1] = py * f; out[2] = pz * f;
}

}  // namespace ddk
