// The four FasterTensorProduct shapes of the score model's conv layers (models/tensor_layers.py:56-61), shared by the forward kernel (k_tp.hip) and
// its vector-Jacobian product (k_tp_bwd.hip): input multiplicities A, P, Q, C of 0e, 1o, 1e, 0o, output multiplicities O0 .. O3, the weight blocks'
// row counts R0 .. R3 and their offsets B0 .. B3 in the flat weight row of W floats.
#pragma once

namespace ddk {

template <int A_, int P_, int Q_, int C_, int O0_, int O1_, int O2_, int O3_>
struct TpShape {
  static constexpr int A = A_, P = P_, Q = Q_, C = C_, O0 = O0_, O1 = O1_, O2 = O2_, O3 = O3_;
  static constexpr int R0 = O0 ? A + P : 0, R1 = O1 ? A + P + Q : 0, R2 = O2 ? P + Q + C : 0, R3 = O3 ? Q + C : 0;      // tensor_layers.py:56-61
  static constexpr int B0 = 0, B1 = B0 + R0 * O0, B2 = B1 + R1 * O1, B3 = B2 + R2 * O2, W = B3 + R3 * O3;
  static constexpr int DIN = A + 3 * P + 3 * Q + C, DOUT = O0 + 3 * O1 + 3 * O2 + O3;
  static constexpr int NV = (W / 4 + 63) / 64;       // 16-B loads per lane and row
  static constexpr int XC = A + 3 * P + 3 * Q;       // first 0o input
  static_assert(A % 8 == 0 && C % 8 == 0 && (A == C || A == 0 || C == 0) && (C == 0 || XC % 4 == 0), "phase A is walked in two halves");
  static_assert(W % 4 == 0 && DIN <= 128 && O0 + O1 + O2 + O3 <= 64 && P <= 8 && Q <= 8, "shape outside the kernel's layout");
};
typedef float tp_f4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float tp_rl(float v, int k) {      // v_readlane_b32 on the bit pattern (the builtin is typed int: a plain call would convert the VALUE)
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

}  // namespace ddk
