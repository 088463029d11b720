// The edge embeddings in front of the conv stack at the op boundary, and their vector-Jacobian product for the four parameter tensors, WITHOUT any per-edge
// tensor besides the two outputs (models/score_model.py:191-225 of the reference: lig_edge_embedding, cross_edge_embedding, rec_edge_embedding and the
// first-order spherical harmonics of the edges).  For edge e of ONE edge group:
//   vec = pos_b[idx_b[e]] - pos_a[idx_a[e]]     d = |vec|     row = [ feat[e] (F = 0 or 4) | sig[sig_index[idx_a[e]]] (32) | exp(coeff (d - offset_j)^2) (32) ]
//   pre = W1 row + b1     hid = dropout(relu(pre))     emb[e] = W2 hid + b2     sh[e] = [1 | sqrt3 vec / max(d, 1e-12)]
// Every column of the row is a pure function of two coordinates, a graph index and the bond type: nothing of it carries a gradient, so the backward has the
// parameters alone to serve and RECOMPUTES row, pre and the mask from the coordinates and the seed; the forward keeps nothing per edge.  Exact fp32: every
// dot product is ONE fmaf chain in a written-out order (compiled with -ffp-contract=off, so that the only fused operations are the ones spelled fmaf):
//   pre[e, c]  = fmaf(W1[c, K - 1], row[K - 1], ... fmaf(W1[c, 0], row[0], b1[c]))          k ascending, the bias first (feat, then sig, then the smearing)
//   emb[e, o]  = fmaf(W2[o, 23], hid[23], ... fmaf(W2[o, 0], hid[0], b2[o]))                c ascending, the bias first
//   ghid[e, c] = fmaf(g[e, 23], W2[23, c], ... fmaf(g[e, 0], W2[0, c], 0))                  o ascending
//   d = sqrtf(fmaf(z, z, fmaf(y, y, x * x))), the smearing's argument t = d - offset_j, column = expf(coeff * (t * t))
// The forward and the backward share these expressions (eemb_geometry, eemb_smear, eemb_hidden): the recomputed hidden layer has the forward's bits.
//
// FORWARD.  One LANE owns one EDGE; a workgroup is two waves.  The lane's 24 accumulators start from b1 and a step adds FOUR columns of W1 (24 loads of 16
// bytes at the same address in every lane: scalar loads through the constant cache, W1 is 6.5 KB, W2 2.3 KB, and v_fmac_f32 takes them from the scalar
// registers).  The row is never stored: a step's four columns are made where they are used.  emb and sh leave as 16-byte stores of the lane's own row.
//
// THE MASK (include/ddk.h, DDK_EEMB_MASK_LAYOUT): keep(e, c) = rng_uniform(word c % 4 of Philox4x32-10(key = seed, counter = (e_lo, e_hi, c / 4,
// DDK_EEMB_MASK_TAG))) >= p, e the edge's position within the call: a pure function of (seed, edge id, column).
//
// BACKWARD.  eemb_param_kernel + the slice reduction of k_reduce.hip, as rhid_param_kernel: a workgroup of four waves owns a slice of rtp_slice_len(E)
// edges and walks it 64 edges at a time.  Per step the four waves share the 64 edges (lane = edge): wave w makes eight columns of sig and of the smearing
// and six of grad_emb into LDS; then six columns of pre / hid (the forward's chain over the whole row, read back from LDS); then six of
// gpre = ghid * (hid != 0 ? s : 0).  Then every thread adds the step's 64 edges, in ascending edge order, to its elements of the slice's image, which
// it holds in registers: grad_w1 [24][K] with grad_b1 as column K, grad_w2 [24][24] with grad_b2 as column 24.  Plain stores of the image; the second
// kernel adds the images in slice order.  No atomics; the images are the whole workspace, and everything is computed whichever outputs are asked for, so
// the bits do not depend on the subset, the run or the device.  A row of the LDS tiles has an odd stride: the lanes of an access hit different banks.
//
// THE LATENT VARIANT (DisCo: latent_dim = NL in 1..4; include/ddk.h, ddk_eemb_latent_*) is a compile-time flag of both kernels, as RtpIdx<S> is of the rtp
// kernels: the plain instantiations take EembArgs and are the code they were.  The row gains 2 NL columns behind the smearing, [lat_a[idx_a[e]] | lat_b[idx_b[e]]]
// (zeros with zero_latent: the cross group), the chain of pre runs on over them, and emb[e, o] = fmaf(unc_a[idx_a[e]], uemb[o], emb[e, o]) closes the forward
// where unc_a is given.  The latent carries a gradient, so the parameter pass has three more things to do per step of 64 edges: the latent columns ride in the
// row tile (grad_w1 is [24][K] with K up to 76, the tile's stride 77), grad_uemb is one more image column (the threads of grad_b2's row group, edges ascending),
// and glat[e, j] = fmaf(gpre[e, 23], W1[23, K0 + j], ... fmaf(gpre[e, 0], W1[0, K0 + j], 0)), K0 = F + 64, leaves as two planes [E, NL] of the workspace
// (idx_a's columns, idx_b's columns) that launch_seg_sum adds per node in ascending edge id from the caller's node-sorted lists.  No atomics.
#include <type_traits>

#include "ddk_internal.h"
#include "k_philox.h"

namespace ddk {

constexpr int EE_H = 24;             // hidden and output width (ns)
constexpr int EE_S = 32;             // sigma embedding columns
constexpr int EE_D = 32;             // Gaussians of the distance expansion
constexpr int EE_KMAX = 4 + EE_S + EE_D;
constexpr int EE_NLMAX = 4;          // latent columns per side (latent variant)
constexpr int EE_EPB = 128;          // edges per workgroup of the forward: two waves, one edge per lane
constexpr int EE_PT = 256;           // threads of eemb_param_kernel: four waves
constexpr int EE_LDR = EE_KMAX + 1;  // row stride of the LDS tile of rows
constexpr int EE_LDR_LAT = EE_KMAX + 2 * EE_NLMAX + 1;      // the same with the latent columns: 77, odd
constexpr int EE_LDH = EE_H + 1;     // row stride of the LDS tiles of grad_emb, hid and gpre
static_assert(EE_H == NS, "the edge embedding of ns = 24");

struct EembArgs {
  const float* pos_a; const float* pos_b; const int32_t* idx_a; const int32_t* idx_b;
  const float* feat; const float* sig; const int32_t* sig_index;
  const float* w1; const float* b1; const float* w2; const float* b2;
  const float* gemb;
  float* emb; float* sh; float* img;
  int64_t E, L;      // edges of the call; edges per slice (parameter pass)
  int F, K;          // bond-feature columns (0 or 4); K = F + 64
  float coeff, p, s;
  uint32_t seed_lo, seed_hi;
  float offset[EE_D];
};

// what the latent instantiations take on top (glat_a / glat_b: the planes [E, NL] of the parameter pass, null: not made; img_u: the images [slices][24] of grad_uemb)
struct EembLatArgs : EembArgs {
  const float* lat_a; const float* lat_b; const float* unc_a; const float* uemb;
  float* glat_a; float* glat_b; float* img_u;
  int NL, zero_latent;
};
template <bool LAT> using EembKernelArgs = std::conditional_t<LAT, EembLatArgs, EembArgs>;

struct EembEdge { float x, y, z, d; int64_t sig_row; };

// vec, d and the row of the sigma table of edge e (the indices are trusted)
__device__ __forceinline__ EembEdge eemb_geometry(const EembArgs& a, int64_t e) {
  const int64_t ia = a.idx_a[e], ib = a.idx_b[e];
  EembEdge g;
  g.x = a.pos_b[3 * ib] - a.pos_a[3 * ia];
  g.y = a.pos_b[3 * ib + 1] - a.pos_a[3 * ia + 1];
  g.z = a.pos_b[3 * ib + 2] - a.pos_a[3 * ia + 2];
  g.d = sqrtf(fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)));
  g.sig_row = a.sig_index[ia];
  return g;
}

__device__ __forceinline__ float eemb_smear(const EembArgs& a, float d, int j) {
  const float t = d - a.offset[j];
  return expf(a.coeff * (t * t));
}

// hid[c] of the dropout layout from the ReLU of pre[c]: columns c0 .. c0 + n - 1 (c0 a multiple of 2, n <= 8) of edge e
// (mask_keep4 / mask_relu of k_philox.h written out: through the helper eemb_param_kernel measured 1 % slower, with the text below it is the code it was)
template <int N>
__device__ __forceinline__ void eemb_hidden(const EembArgs& a, int64_t e, int c0, float* v) {
  if (a.p > 0.f) {
    const uint32_t key[2] = {a.seed_lo, a.seed_hi};
    const int q0 = c0 >> 2, q1 = (c0 + N - 1) >> 2;
    for (int q = q0; q <= q1; ++q) {
      const uint32_t ctr[4] = {(uint32_t)e, (uint32_t)((uint64_t)e >> 32), (uint32_t)q, DDK_EEMB_MASK_TAG};
      uint32_t w[4];
      philox4x32_10(ctr, key, w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 4 * q + i - c0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          if (j == c) {
            const float r = v[j] < 0.f ? 0.f : v[j];      // (a NaN stays one, as torch's relu leaves it)
            v[j] = rng_uniform(w[i]) >= a.p ? r * a.s : 0.f;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------------------------------
template <bool LAT>
__global__ __launch_bounds__(EE_EPB) void eemb_fwd_kernel(EembKernelArgs<LAT> a) {
  const int64_t e = (int64_t)blockIdx.x * EE_EPB + threadIdx.x;
  const bool ev = e < a.E;
  const int64_t el = ev ? e : 0;      // a lane past the end works on edge 0 and stores nothing
  const EembEdge g = eemb_geometry(a, el);
  float acc[EE_H];
#pragma unroll
  for (int c = 0; c < EE_H; ++c) acc[c] = a.b1[c];
  const int K = a.K;
  int k0 = 0;
  if (a.F) {      // the bond features: columns 0 .. 3
    const float4 f = reinterpret_cast<const float4*>(a.feat)[el];
    const float x[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int c = 0; c < EE_H; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c] = fmaf(a.w1[c * K + i], x[i], acc[c]);
    }
    k0 = 4;
  }
  const float4* srow = reinterpret_cast<const float4*>(a.sig + g.sig_row * EE_S);
#pragma unroll 1
  for (int j = 0; j < EE_S; j += 4) {      // the sigma embedding of the edge's graph
    const float4 f = srow[j >> 2];
    const float x[4] = {f.x, f.y, f.z, f.w};
    const float* w = a.w1 + k0 + j;
#pragma unroll
    for (int c = 0; c < EE_H; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c] = fmaf(w[c * K + i], x[i], acc[c]);
    }
  }
#pragma unroll 1
  for (int j = 0; j < EE_D; j += 4) {      // the Gaussian smearing of the edge length
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = eemb_smear(a, g.d, j + i);
    const float* w = a.w1 + k0 + EE_S + j;
#pragma unroll
    for (int c = 0; c < EE_H; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c] = fmaf(w[c * K + i], x[i], acc[c]);
    }
  }
  if constexpr (LAT) {      // the latent of the edge's two nodes: columns F + 64 .. K - 1 (zero_latent: the row holds zeros there)
    const int64_t ia = a.idx_a[el], ib = a.idx_b[el];
    const float* w = a.w1 + k0 + EE_S + EE_D;
#pragma unroll 1
    for (int j = 0; j < 2 * a.NL; ++j) {
      const float x = a.zero_latent ? 0.f : (j < a.NL ? a.lat_a[ia * a.NL + j] : a.lat_b[ib * a.NL + j - a.NL]);
#pragma unroll
      for (int c = 0; c < EE_H; ++c) acc[c] = fmaf(w[c * K + j], x, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < EE_H; c += 8) eemb_hidden<8>(a, el, c, acc + c);
  float out[EE_H];
#pragma unroll
  for (int o = 0; o < EE_H; ++o) {
    float v = a.b2[o];
#pragma unroll
    for (int c = 0; c < EE_H; ++c) v = fmaf(a.w2[o * EE_H + c], acc[c], v);
    out[o] = v;
  }
  if constexpr (LAT) {
    if (a.unc_a) {
      const float u = a.unc_a[a.idx_a[el]];
#pragma unroll
      for (int o = 0; o < EE_H; ++o) out[o] = fmaf(u, a.uemb[o], out[o]);
    }
  }
  if (ev) {
    float4* to = reinterpret_cast<float4*>(a.emb + e * EE_H);
#pragma unroll
    for (int q = 0; q < EE_H / 4; ++q) to[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    const float r = 1.7320508075688772f / fmaxf(g.d, 1e-12f);
    reinterpret_cast<float4*>(a.sh)[e] = make_float4(1.f, g.x * r, g.y * r, g.z * r);
  }
}

// ---- backward: the slice images ------------------------------------------------------------------------------------------------------------------------------
// image of a slice: [24][K + 1] (grad_w1, column K grad_b1), then [24][25] (grad_w2, column 24 grad_b2)
__host__ __device__ inline int eemb_img(int K) { return EE_H * (K + 1) + EE_H * (EE_H + 1); }

template <bool LAT>
__global__ __launch_bounds__(EE_PT) void eemb_param_kernel(EembKernelArgs<LAT> a) {
  constexpr int LDR = LAT ? EE_LDR_LAT : EE_LDR;
  __shared__ float rows[64 * LDR];
  constexpr int UC = EE_LDR_LAT - 1;      // latent variant: the tile's last column (K <= 76 never reaches it) holds unc_a of the edge
  __shared__ float gs[64 * EE_LDH];
  __shared__ float hs[64 * EE_LDH];
  __shared__ float ps[64 * EE_LDH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform in the wave: what it indexes W1 and W2 with goes through scalar loads)
  const int K = a.K, F = a.F;
  const int64_t slice = blockIdx.x;
  const int64_t begin = slice * a.L, end = begin + a.L < a.E ? begin + a.L : a.E;
  // the thread's elements of the image: rows 3 tc .. 3 tc + 2 of columns tk, tk + 32, tk + 64 (< K) of grad_w1; of column tk (< 24) of grad_w2;
  // tk == 24: of grad_b1; tk == 25: of grad_b2
  const int tc = tid & 7, tk = tid >> 3;
  float a1[3][3], a2[3], au[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a2[i] = 0.f; au[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) a1[i][j] = 0.f;
  }
  const bool third = tk + 64 < K;
  for (int64_t eb = begin; eb < end; eb += 64) {
    const int64_t e = eb + lane;
    const bool ev = e < end;
    const int64_t el = ev ? e : begin;
    // 1. the wave's columns of the row and of grad_emb; a lane past the end stages zeros, which leave every sum as it is
    {
      const EembEdge g = eemb_geometry(a, el);
      float* r = rows + lane * LDR;
      if (wave == 0 && F) {
        const float4 f = reinterpret_cast<const float4*>(a.feat)[el];
        r[0] = ev ? f.x : 0.f; r[1] = ev ? f.y : 0.f; r[2] = ev ? f.z : 0.f; r[3] = ev ? f.w : 0.f;
      }
      const float4* srow = reinterpret_cast<const float4*>(a.sig + g.sig_row * EE_S) + 2 * wave;
      const float4 s0 = srow[0], s1 = srow[1];
      const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        r[F + 8 * wave + i] = ev ? sv[i] : 0.f;
        const float x = eemb_smear(a, g.d, 8 * wave + i);
        r[F + EE_S + 8 * wave + i] = ev ? x : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) gs[lane * EE_LDH + 6 * wave + i] = ev ? a.gemb[el * EE_H + 6 * wave + i] : 0.f;
      if constexpr (LAT) {
        if (wave == 1) {      // the latent columns; wave 2: unc_a of the edge
          const int64_t ia = a.idx_a[el], ib = a.idx_b[el];
          for (int j = 0; j < 2 * a.NL; ++j) {
            const float x = a.zero_latent ? 0.f : (j < a.NL ? a.lat_a[ia * a.NL + j] : a.lat_b[ib * a.NL + j - a.NL]);
            r[F + EE_S + EE_D + j] = ev ? x : 0.f;
          }
        } else if (wave == 2) {
          rows[lane * LDR + UC] = (ev && a.unc_a) ? a.unc_a[a.idx_a[el]] : 0.f;
        }
      }
    }
    __syncthreads();
    // 2. six columns of pre and of hid: the forward's chain over the row
    {
      const float* r = rows + lane * LDR;
      const float* w = a.w1 + 6 * wave * K;
      float v[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) v[i] = a.b1[6 * wave + i];
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const float x = r[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = fmaf(w[i * K + k], x, v[i]);
      }
      eemb_hidden<6>(a, el, 6 * wave, v);
#pragma unroll
      for (int i = 0; i < 6; ++i) hs[lane * EE_LDH + 6 * wave + i] = ev ? v[i] : 0.f;
      // 3. six columns of gpre = ghid * (hid != 0 ? s : 0)
      float gh[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < EE_H; ++o) {
        const float go = gs[lane * EE_LDH + o];
#pragma unroll
        for (int i = 0; i < 6; ++i) gh[i] = fmaf(go, a.w2[o * EE_H + 6 * wave + i], gh[i]);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) ps[lane * EE_LDH + 6 * wave + i] = ev ? gh[i] * (v[i] != 0.f ? a.s : 0.f) : 0.f;
    }
    __syncthreads();
    if constexpr (LAT) {      // the latent's per-edge gradient rows: wave w makes columns w and w + 4 of [idx_a's NL | idx_b's NL], one chain over c ascending
      if (a.glat_a) {
        for (int j = wave; j < 2 * a.NL; j += 4) {
          const float* w = a.w1 + F + EE_S + EE_D + j;
          float v = 0.f;
#pragma unroll 4
          for (int c = 0; c < EE_H; ++c) v = fmaf(ps[lane * EE_LDH + c], w[c * K], v);
          if (ev) {
            if (j < a.NL) a.glat_a[e * a.NL + j] = v;
            else a.glat_b[e * a.NL + j - a.NL] = v;
          }
        }
      }
    }
    // 4. the step's 64 edges, ascending, into the thread's elements of the image
    if (tk < EE_H) {
#pragma unroll 4
      for (int l = 0; l < 64; ++l) {
        const float hv = hs[l * EE_LDH + tk];
        const float x0 = rows[l * LDR + tk], x1 = rows[l * LDR + tk + 32], x2 = third ? rows[l * LDR + tk + 64] : 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float gp = ps[l * EE_LDH + 3 * tc + i];
          a1[i][0] = fmaf(gp, x0, a1[i][0]); a1[i][1] = fmaf(gp, x1, a1[i][1]); a1[i][2] = fmaf(gp, x2, a1[i][2]);
          a2[i] = fmaf(gs[l * EE_LDH + 3 * tc + i], hv, a2[i]);
        }
      }
    } else {
      const float* from = tk == EE_H ? ps : gs;      // grad_b1 = the sum of gpre, grad_b2 = the sum of grad_emb (tk == 25; the threads behind add what they never store)
#pragma unroll 4
      for (int l = 0; l < 64; ++l) {
        const float x0 = rows[l * LDR + tk], x1 = rows[l * LDR + tk + 32];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float gp = ps[l * EE_LDH + 3 * tc + i];
          a1[i][0] = fmaf(gp, x0, a1[i][0]); a1[i][1] = fmaf(gp, x1, a1[i][1]);
          a2[i] += from[l * EE_LDH + 3 * tc + i];
          if constexpr (LAT) au[i] = fmaf(rows[l * LDR + UC], gs[l * EE_LDH + 3 * tc + i], au[i]);      // grad_uemb (tk == 25 stores it)
        }
      }
    }
    __syncthreads();      // (the next step overwrites the tiles)
  }
  float* img = a.img + slice * (int64_t)eemb_img(K);
  float* img2 = img + EE_H * (K + 1);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int c = 3 * tc + i;
    img[c * (K + 1) + tk] = a1[i][0];
    img[c * (K + 1) + tk + 32] = a1[i][1];
    if (third) img[c * (K + 1) + tk + 64] = a1[i][2];
    if (tk < EE_H) img2[c * (EE_H + 1) + tk] = a2[i];
    else if (tk == EE_H) img[c * (K + 1) + K] = a2[i];
    else if (tk == EE_H + 1) img2[c * (EE_H + 1) + EE_H] = a2[i];
    if constexpr (LAT) {
      if (tk == EE_H + 1) a.img_u[slice * EE_H + c] = au[i];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
// The plain op is the latent op with NL = 0 and no unconditional term: l == nullptr below.  It runs the <false> instantiations on the EembArgs part of the
// arguments.  workspace: [slices][eemb_img(K)], and with NL > 0 behind it [slices][24] (grad_uemb) | glat_a [E][NL] | glat_b [E][NL], every part on 16 bytes
int64_t eemb_workspace(int64_t E, int32_t K, int32_t NL) {
  if (E < 0 || E >= (int64_t)1 << 31 || NL < 0 || NL > EE_NLMAX || (K != EE_S + EE_D + 2 * NL && K != EE_KMAX + 2 * NL)) return -1;
  const int64_t ns = slice_bound(E, 1);
  return (NL ? ws_pad(ns * eemb_img(K)) + ws_pad(ns * EE_H) + 2 * ws_pad(E * NL) : ns * eemb_img(K)) * (int64_t)sizeof(float);
}

// offset as torch.linspace(start, stop, 32) makes it in fp32 (one fused multiply-add per centre, the upper half counted down from stop), coeff as GaussianSmearing: -0.5 / (offset[1] - offset[0])^2
static EembLatArgs eemb_args(const EembOperands& o, const EembLatent* l, int64_t E) {
  EembLatArgs a{};
  a.pos_a = o.pos_a; a.pos_b = o.pos_b; a.idx_a = o.idx_a; a.idx_b = o.idx_b; a.feat = o.feat; a.sig = o.sig; a.sig_index = o.sig_index;
  a.w1 = o.w1; a.b1 = o.b1; a.w2 = o.w2; a.b2 = o.b2;
  a.E = E; a.L = rtp_slice_len(E);
  a.F = o.F; a.K = a.F + EE_S + EE_D;
  const float step = (o.stop - o.start) / (float)(EE_D - 1);
  for (int j = 0; j < EE_D; ++j) a.offset[j] = j < EE_D / 2 ? fmaf(step, (float)j, o.start) : fmaf(-step, (float)(EE_D - 1 - j), o.stop);
  const double gap = (double)(a.offset[1] - a.offset[0]);
  a.coeff = (float)(-0.5 / (gap * gap));
  a.p = o.p;
  a.s = o.p > 0.f ? 1.0f / (1.0f - o.p) : 1.0f;
  a.seed_lo = (uint32_t)o.seed; a.seed_hi = (uint32_t)(o.seed >> 32);
  if (l) {
    a.K += 2 * l->NL;
    a.lat_a = l->lat_a; a.lat_b = l->lat_b; a.unc_a = l->unc_a; a.uemb = l->uemb;
    a.NL = l->NL; a.zero_latent = l->zero_latent;
  }
  return a;
}

hipError_t launch_eemb_forward(const EembOperands& o, const EembLatent* l, int64_t E, float* emb, float* sh, hipStream_t s) {
  if (E == 0) return hipSuccess;
  EembLatArgs a = eemb_args(o, l, E);
  a.emb = emb; a.sh = sh;
  const dim3 grid((unsigned)((E + EE_EPB - 1) / EE_EPB));      // E < 2^31: fewer than 2^31 workgroups
  if (l) hipLaunchKernelGGL(eemb_fwd_kernel<true>, grid, dim3(EE_EPB), 0, s, a);
  else hipLaunchKernelGGL(eemb_fwd_kernel<false>, grid, dim3(EE_EPB), 0, s, static_cast<const EembArgs&>(a));
  return hipGetLastError();
}

hipError_t launch_eemb_backward(const EembOperands& o, const EembLatent* l, const EembLatentGraph& gr, const float* grad_emb, int64_t E, float* grad_w1,
                                float* grad_b1, float* grad_w2, float* grad_b2, float* grad_uemb, float* grad_lat_a, float* grad_lat_b, float* workspace,
                                hipStream_t s) {
  const int NL = l ? l->NL : 0, K = o.F + EE_S + EE_D + 2 * NL;
  const bool nodes = l && !l->zero_latent && E > 0 && (grad_lat_a || grad_lat_b);
  hipError_t e = hipSuccess;
  if (!nodes) {      // no edges, or the cross group: the latent gets zeros (the plain op has no such output)
    e = zero_async(grad_lat_a, gr.n_a * NL, s);
    if (e == hipSuccess) e = zero_async(grad_lat_b, gr.n_b * NL, s);
  }
  if (E == 0) {
    if (e == hipSuccess) e = zero_async(grad_w1, EE_H * K, s);
    if (e == hipSuccess) e = zero_async(grad_b1, EE_H, s);
    if (e == hipSuccess) e = zero_async(grad_w2, EE_H * EE_H, s);
    if (e == hipSuccess) e = zero_async(grad_b2, EE_H, s);
    if (e == hipSuccess) e = zero_async(grad_uemb, EE_H, s);
    return e;
  }
  if (e != hipSuccess) return e;
  EembLatArgs a = eemb_args(o, l, E);
  a.gemb = grad_emb; a.img = workspace;
  const dim3 grid((unsigned)((E + a.L - 1) / a.L));      // the slices: at most 241
  float* glat_a = nullptr; float* glat_b = nullptr;
  if (l) {
    const int64_t ns = slice_bound(E, 1);
    a.img_u = workspace + ws_pad(ns * eemb_img(K));
    glat_a = a.img_u + ws_pad(ns * EE_H);
    glat_b = glat_a + ws_pad(E * NL);
    a.glat_a = nodes ? glat_a : nullptr; a.glat_b = nodes ? glat_b : nullptr;
    hipLaunchKernelGGL(eemb_param_kernel<true>, grid, dim3(EE_PT), 0, s, a);
  } else {
    hipLaunchKernelGGL(eemb_param_kernel<false>, grid, dim3(EE_PT), 0, s, static_cast<const EembArgs&>(a));
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const EdgeGroupTable t = group_table(E);
  if (grad_w1 || grad_b1 || grad_w2 || grad_b2)
    e = launch_slice_reduce(workspace, t, a.L, ReducePart{grad_w1, grad_b1, EE_H, K}, ReducePart{grad_w2, grad_b2, EE_H, EE_H}, s);
  if (e == hipSuccess && grad_uemb) e = launch_slice_reduce(a.img_u, t, a.L, ReducePart{nullptr, grad_uemb, EE_H, 0}, ReducePart{nullptr, nullptr, 0, 0}, s);
  if (e == hipSuccess && nodes && grad_lat_a) e = launch_seg_sum(glat_a, gr.order_a, gr.ptr_a, grad_lat_a, gr.n_a, NL, s);
  if (e == hipSuccess && nodes && grad_lat_b) e = launch_seg_sum(glat_b, gr.order_b, gr.ptr_b, grad_lat_b, gr.n_b, NL, s);
  return e;
}

}  // namespace ddk
