// The sampler's random draws, made on the device from the counter-based generator of k_philox.h (see include/ddk.h: DDK_RNG_LAYOUT, ddk_rng_noise,
// ddk_rng_initial, ddk_rng_uniform):
//   rng_noise_kernel    the N(0,1) rows ddk_sample's `noise` argument reads, [steps, B, n_cols]
//   rng_initial_kernel  the draws of randomize_position: torsion angles [B, n_rot], rotation matrices [B, 3, 3], translations [B, 3]
//   rng_uniform_kernel  the uniform of one AR pick per sample, [B]
// One thread per Philox block (four words): the arrays are tens of kilobytes and nothing here is worth more.  Every value is a pure function of
// (seed, complex, sample, step, column): no state, no atomics, no dependence on the grid, so any cut of the work into calls gives the same bits.
#include <math.h>

#include "k_philox.h"
#include "model.h"

namespace ddk {

constexpr int RNG_THREADS = 256;
constexpr int64_t RNG_MAX_GRID = 1 << 16;      // workgroups of a launch; the threads stride over what is left

static unsigned rng_grid(int64_t items) {
  const int64_t g = (items + RNG_THREADS - 1) / RNG_THREADS;
  return (unsigned)(g < 1 ? 1 : (g > RNG_MAX_GRID ? RNG_MAX_GRID : g));
}

// rows (k, b) of steps [step0, step0 + steps): item = (k * B + b) * n_blk + blk writes columns 4 blk .. 4 blk + 3 of its row; columns at or past
// n_active write 0 and a block that lies wholly there draws nothing
__global__ __launch_bounds__(RNG_THREADS) void rng_noise_kernel(RngStream S, uint32_t sample0, int B, uint32_t step0, int steps, int n_cols, int n_active,
                                                                 float* __restrict__ out) {
  const int n_blk = (n_cols + 3) >> 2;
  const int64_t items = (int64_t)steps * B * n_blk;
  for (int64_t it = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * RNG_THREADS) {
    const int blk = (int)(it % n_blk);
    const int64_t row = it / n_blk;
    const int b = (int)(row % B);
    const uint32_t k = (uint32_t)(row / B);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (4 * blk < n_active) {
      uint32_t w[4];
      rng_block(S, sample0 + (uint32_t)b, RNG_NOISE, step0 + k, (uint32_t)blk, w);
      rng_normals(w, z);
    }
    float* o = out + row * n_cols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * blk + j;
      if (c < n_cols) o[c] = c < n_active ? z[j] : 0.f;
    }
  }
}

// item = b * per + j with per = n_tor_blk + 2: j < n_tor_blk the torsion block j of sample b, j = n_tor_blk its rotation, j = n_tor_blk + 1 its translation
__global__ __launch_bounds__(RNG_THREADS) void rng_initial_kernel(RngStream S, uint32_t sample0, int B, int n_rot, float tr_sigma, uint32_t purpose_rot,
                                                                   float* __restrict__ tor_out, float* __restrict__ rot_out, float* __restrict__ tr_out) {
  const int n_tor_blk = tor_out ? (n_rot + 3) >> 2 : 0;
  const int per = n_tor_blk + 2;
  const int64_t items = (int64_t)B * per;
  for (int64_t it = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * RNG_THREADS) {
    const int j = (int)(it % per);
    const int64_t b = it / per;
    const uint32_t sample = sample0 + (uint32_t)b;
    uint32_t w[4];
    if (j < n_tor_blk) {
      rng_block(S, sample, RNG_INIT_TORSION, 0, (uint32_t)j, w);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 4 * j + q;
        if (r < n_rot) tor_out[b * n_rot + r] = rng_torsion(w[q]);
      }
    } else if (j == n_tor_blk) {
      float q[4], R[9];
      rng_block(S, sample, purpose_rot, 0, 0, w);
      rng_normals(w, q);
      rng_rotation(q, R);
#pragma unroll
      for (int e = 0; e < 9; ++e) rot_out[b * 9 + e] = R[e];
    } else if (tr_out) {
      float z[4];
      rng_block(S, sample, RNG_INIT_TRANSLATION, 0, 0, w);
      rng_normals(w, z);
#pragma unroll
      for (int e = 0; e < 3; ++e) tr_out[b * 3 + e] = tr_sigma * z[e];
    }
  }
}

__global__ __launch_bounds__(RNG_THREADS) void rng_uniform_kernel(RngStream S, uint32_t sample0, int B, uint32_t decoding_idx, float* __restrict__ out) {
  for (int64_t b = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x; b < B; b += (int64_t)gridDim.x * RNG_THREADS) {
    uint32_t w[4];
    rng_block(S, sample0 + (uint32_t)b, RNG_AR_PICK, decoding_idx, 0, w);
    out[b] = rng_uniform(w[0]);
  }
}

hipError_t launch_rng_noise(uint64_t seed, uint64_t stream_id, int sample0, int B, int step0, int steps, int n_cols, int n_active, float* out, hipStream_t s) {
  if (steps < 1) return hipSuccess;
  const int64_t items = (int64_t)steps * B * ((n_cols + 3) >> 2);
  hipLaunchKernelGGL(rng_noise_kernel, dim3(rng_grid(items)), dim3(RNG_THREADS), 0, s, rng_stream(seed, stream_id), (uint32_t)sample0, B, (uint32_t)step0,
                     steps, n_cols, n_active, out);
  return hipGetLastError();
}

hipError_t launch_rng_initial(uint64_t seed, uint64_t stream_id, int sample0, int B, int n_rot, float tr_sigma, int purpose_rot, float* tor_out,
                              float* rot_out, float* tr_out, hipStream_t s) {
  const int64_t items = (int64_t)B * ((tor_out ? (n_rot + 3) >> 2 : 0) + 2);
  hipLaunchKernelGGL(rng_initial_kernel, dim3(rng_grid(items)), dim3(RNG_THREADS), 0, s, rng_stream(seed, stream_id), (uint32_t)sample0, B, n_rot, tr_sigma,
                     (uint32_t)purpose_rot, tor_out, rot_out, tr_out);
  return hipGetLastError();
}

hipError_t launch_rng_uniform(uint64_t seed, uint64_t stream_id, int sample0, int B, int decoding_idx, float* out, hipStream_t s) {
  hipLaunchKernelGGL(rng_uniform_kernel, dim3(rng_grid(B)), dim3(RNG_THREADS), 0, s, rng_stream(seed, stream_id), (uint32_t)sample0, B, (uint32_t)decoding_idx, out);
  return hipGetLastError();
}

}  // namespace ddk
