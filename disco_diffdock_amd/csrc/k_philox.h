// The sampler's counter-based generator (include/ddk.h, DDK_RNG_LAYOUT 1): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) and the conversions from its words to the draws the sampler consumes.  Plain C++, host and device: a kernel that draws for itself (the pose
// update, one day) includes this header and gets the same numbers as rng_*_kernel of k_rng.hip, and tests/philox_ref.py restates it operation for operation.
// Every draw is a pure function of (seed, complex, sample, step, column); nothing here keeps state.
//   uniform   u = (x >> 8) * 2^-24: in [0, 1), exact in fp32
//   torsion   (float)pi * (2u - 1): 2u - 1 is exact (a multiple of 2^-23 in [-1, 1)), so ONE rounding
//   normals   Box-Muller, two pairs per block from words (0, 1) and (2, 3): u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (x1 >> 8) * 2^-24,
//             r = sqrtf(-2 logf(u1)), z0 = r cospif(2 u2), z1 = r sinpif(2 u2) with the accurate library functions.
//             |z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768 by construction; u1 = 1 gives r = 0 and a signed zero, never NaN (u1 > 0: the log is finite).
//   rotation  the four normals of a block are the quaternion (x, y, z, w): normalised, then scipy's Rotation.from_quat matrix; |q|^2 < 2^-60: identity
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DDK_HD __host__ __device__
#else
#define DDK_HD
#endif

namespace ddk {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl constants of the key schedule

// the purposes of DDK_RNG_LAYOUT 1 (bits 28..31 of counter word 3)
// (6-8 and 11 are the forward process, RngForwardPurpose of k_noising.hip; 9 and 10 the conformer matching's search, k_match.hip)
enum RngPurpose : uint32_t { RNG_NOISE = 0, RNG_INIT_TORSION = 1, RNG_INIT_ROTATION = 2, RNG_INIT_TRANSLATION = 3, RNG_AR_PICK = 4, RNG_AR_ROTATION = 5,
                             RNG_MATCH_POPULATION = 9, RNG_MATCH_GENERATION = 10 };
constexpr int RNG_MAX_STEPS = 1 << 20;      // step < 2^20
constexpr int RNG_MAX_COLS = 1024;          // block < 256, four words each

struct RngStream { uint32_t seed_lo, seed_hi, stream_lo, stream_hi; };

DDK_HD inline RngStream rng_stream(uint64_t seed, uint64_t stream_id) {
  return RngStream{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
}

DDK_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of block `block` of (purpose, step) for global sample `sample`: the counter layout of DDK_RNG_LAYOUT 1
DDK_HD inline void rng_block(const RngStream& S, uint32_t sample, uint32_t purpose, uint32_t step, uint32_t block, uint32_t out[4]) {
  const uint32_t ctr[4] = {S.stream_lo, S.stream_hi, sample, (purpose << 28) | (step << 8) | block};
  const uint32_t key[2] = {S.seed_lo, S.seed_hi};
  philox4x32_10(ctr, key, out);
}

DDK_HD inline float rng_uniform(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }

// The dropout masks of the training ops (include/ddk.h: DDK_RHID_MASK_LAYOUT, DDK_EEMB_MASK_LAYOUT): the keep flags of columns 4 q .. 4 q + 3 of edge e are
// rng_uniform(word) >= p of the four words of Philox(key = seed, counter = (e_lo, e_hi, q, tag)), and a kept element is relu(v) / (1 - p) = relu(v) * s
struct MaskKeep4 {      // (keep[i] compares where it is used: flags made ahead of their use cost a kernel vector registers)
  float u[4], p;
  DDK_HD bool operator[](int i) const { return u[i] >= p; }
};
DDK_HD inline MaskKeep4 mask_keep4(uint32_t seed_lo, uint32_t seed_hi, int64_t e, uint32_t q, uint32_t tag, float p) {
  const uint32_t ctr[4] = {(uint32_t)e, (uint32_t)((uint64_t)e >> 32), q, tag};
  const uint32_t key[2] = {seed_lo, seed_hi};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  return MaskKeep4{{rng_uniform(w[0]), rng_uniform(w[1]), rng_uniform(w[2]), rng_uniform(w[3])}, p};
}
DDK_HD inline float mask_relu(bool keep, float v, float s) {
  const float r = v < 0.f ? 0.f : v;      // (a NaN stays one, as torch's relu leaves it)
  return keep ? r * s : 0.f;
}

DDK_HD inline float rng_torsion(uint32_t x) {
  const float s = 2.0f * rng_uniform(x) - 1.0f;      // exact, contracted or not
  return 3.14159265358979323846f * s;
}

// cos(pi a), sin(pi a) for a in [0, 2).  The device has cospif / sinpif; a host libm need not, so the host folds a onto [-1/4, 1/4] exactly (a is a multiple of
// 2^-23) and calls cosf / sinf there: the same values to within the functions' last bits, which is what a host-side check of the device draws compares to.
DDK_HD inline void rng_cossinpi(float a, float& c, float& s) {
#if defined(__HIP_DEVICE_COMPILE__)
  c = cospif(a);
  s = sinpif(a);
#else
  const int k = (int)(2.0f * a + 0.5f);                     // nearest half-turn quarter: 0 .. 4
  const float f = 3.14159265358979323846f * (a - 0.5f * (float)k);
  const float cf = cosf(f), sf = sinf(f);
  switch (k & 3) {
    case 0: c = cf; s = sf; break;
    case 1: c = -sf; s = cf; break;
    case 2: c = -cf; s = -sf; break;
    default: c = sf; s = -cf; break;
  }
#endif
}

// one Box-Muller pair from two words
DDK_HD inline void rng_normal_pair(uint32_t x0, uint32_t x1, float& z0, float& z1) {
  const float u1 = (float)((x0 >> 8) + 1u) * 0x1p-24f;      // (0, 1]
  const float a = 2.0f * rng_uniform(x1);                   // [0, 2), exact
  const float r = sqrtf(-2.0f * logf(u1));
  float c, s;
  rng_cossinpi(a, c, s);
  z0 = r * c;
  z1 = r * s;
}

DDK_HD inline void rng_normals(const uint32_t w[4], float z[4]) {
  rng_normal_pair(w[0], w[1], z[0], z[1]);
  rng_normal_pair(w[2], w[3], z[2], z[3]);
}

// quaternion (x, y, z, w) -> row-major rotation matrix, the expressions of scipy's Rotation.from_quat(...).as_matrix()
DDK_HD inline void rng_rotation(const float q[4], float R[9]) {
  const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (!(n2 >= 0x1p-60f)) {
    R[0] = 1.f; R[1] = 0.f; R[2] = 0.f; R[3] = 0.f; R[4] = 1.f; R[5] = 0.f; R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
    return;
  }
  const float inv = 1.0f / sqrtf(n2);
  const float x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
  const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const float xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  R[0] = x2 - y2 - z2 + w2; R[1] = 2.f * (xy - zw);     R[2] = 2.f * (xz + yw);
  R[3] = 2.f * (xy + zw);   R[4] = -x2 + y2 - z2 + w2;  R[5] = 2.f * (yz - xw);
  R[6] = 2.f * (xz - yw);   R[7] = 2.f * (yz + xw);     R[8] = -x2 - y2 + z2 + w2;
}

}  // namespace ddk
