// Conformer matching (include/ddk.h: ddk_conformer_rmsd, ddk_conformer_match): fit the torsion angles of a conformer so that, after the optimal rigid
// fit, it lies as close as possible to a target pose (datasets_utils/conformer_matching.py through get_lig_graph_with_matching, process_mols.py:280-311).
// The objective is modify_conformer_torsion_angles (utils/torsion.py:48-68) followed by the Kabsch RMSD; the optimiser is the reference's differential
// evolution (best1bin, F in (0.5, 1), CR 0.8) made generation-synchronous, with wrap-around bounds, a seeded counter-based population and a compass polish.
//   match_validate_kernel   one workgroup: the bond indices, the two mask asserts of the reference, the kept-atom count and the finiteness of the coordinates,
//                           all before an index is used as an address; packs the rotor tables (mask rows as 256-bit rows, the centred coordinates, the target's
//                           sums) into the workspace and writes the status word every later launch of the call reads first.
//   match_generation_kernel one launch per generation over a fixed grid, one WAVE per member: generation 0 draws the population, generation g >= 1 builds the
//                           member's trial from generation g - 1 (double-buffered in the workspace), evaluates it and selects.  Every workgroup recomputes its
//                           island's best member and convergence test from the previous costs: no atomics, no reduction launch, and no workgroup waits for another;
//                           the boundary between two launches is the only ordering between workgroups.
//   match_select_kernel     one workgroup: the best member over the islands, the start of the polish.
//   match_polish_kernel     one launch per polish iteration, one wave per neighbour theta +- h e_d; every workgroup folds the previous iteration's costs into the
//                           state for itself, and once the polish is done the launches that are left return at once.
//   match_finish_kernel     one workgroup: the last fold, the final fit and the stores.
//   conformer_rmsd_kernel   the objective alone on caller-supplied torsion vectors; validates for itself (it has no workspace).
// One evaluation = one wave: the candidate's coordinates sit in 3 KB of LDS, the lanes work over the atoms (four each at 256), a rotor reads its two bond
// atoms, which it never moves (mask[u] = 0, and v is the pivot), so it rotates in place with wave-local ordering only; the centroid, the covariance and the squared norms are summed in
// fp64 and the RMSD comes from the top eigenvalue of Horn's matrix without the rotation.  Every loop has a bound known at launch.
#include "model.h"
#include "k_geom.h"
#include "k_philox.h"

namespace ddk {

namespace {

constexpr float MATCH_PI = 3.14159265358979323846f, MATCH_TWO_PI = 6.28318530717958647692f, MATCH_INV_TWO_PI = 0.15915494309189533577f;
constexpr float MATCH_CR = 0.8f;                 // recombination
constexpr float MATCH_H0 = 0.5f, MATCH_H_MIN = 1e-4f;      // the compass polish's first and smallest step

// what an evaluation reads, in LDS; match_validate_kernel leaves the same bytes in the workspace
struct MatchTables {
  float pos0[MAX_LIG * 3];               // the conformer minus c0 = fp32(mean over all atoms): the rotor chain runs on centred coordinates (k_se3.hip says why)
  float tgt[MAX_LIG * 3];                // the target minus ct = fp32(mean over the kept atoms)
  uint32_t bits[MATCH_MAX_ROT][8];       // mask_rotate's rows as bit rows: atom i is bit i & 31 of word i >> 5
  int2 uv[MATCH_MAX_ROT];                // (u, v) of the rotors: axis pos[u] - pos[v], pivot pos[v]
  uint32_t keep[8];                      // the kept atoms
  double tc[3];                          // what is left of the kept target atoms' mean after ct was subtracted, in fp64
  double Gb;                             // sum over the kept atoms of |tgt - tc|^2
  float ct[3];
  int m;                                 // the kept atoms
};
static_assert(sizeof(MatchTables) % 8 == 0, "copied as 4-byte words, read as doubles");

struct MatchHeader {      // the first 128 bytes of the workspace
  int status, pad;
  int gens[MATCH_MAX_ISLANDS];      // the last generation that changed island j
};
constexpr size_t MATCH_TABLES_AT = 128;

// the compass polish's state between two of its launches, double-buffered in the workspace like the populations
struct MatchPolish {
  float h, c_best;
  int done, pad;
  float th[MATCH_MAX_ROT];
};
struct MatchLayout { size_t polish[2], cand[2], pop[2], cost[2], total; };
inline MatchLayout match_layout(int n_rot, int NP, int n_islands) {
  MatchLayout L;
  const size_t members = (size_t)n_islands * NP, row = (size_t)(n_rot > 0 ? n_rot : 1);
  size_t at = (MATCH_TABLES_AT + sizeof(MatchTables) + 255) / 256 * 256;
  for (int k = 0; k < 2; ++k) { L.polish[k] = at; at += (sizeof(MatchPolish) + 255) / 256 * 256; }
  for (int k = 0; k < 2; ++k) { L.cand[k] = at; at += 2 * MATCH_MAX_ROT * sizeof(float); }
  for (int k = 0; k < 2; ++k) { L.pop[k] = at; at += (members * row * sizeof(float) + 255) / 256 * 256; }
  for (int k = 0; k < 2; ++k) { L.cost[k] = at; at += (members * sizeof(float) + 255) / 256 * 256; }
  L.total = at;
  return L;
}

__device__ inline bool bit_of(const uint32_t* row, int i) { return (row[i >> 5] >> (i & 31)) & 1u; }

__device__ inline double wave_sum(double v) {      // every lane gets the same total (a + b == b + a bit for bit)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline float wrap_angle(float t) {      // into [-pi, pi): the objective is 2 pi-periodic
  const float k = floorf((t + MATCH_PI) * MATCH_INV_TWO_PI);
  float w = fmaf(-MATCH_TWO_PI, k, t);
  if (w >= MATCH_PI) w -= MATCH_TWO_PI;
  if (w < -MATCH_PI) w += MATCH_TWO_PI;
  return w;
}

// Validates the problem and fills T from the caller's arrays.  Called by every thread of a workgroup of at least 128 threads (barriers inside); returns the
// status, the same in every thread: 0, 2 (a bond index outside the ligand, u == v, mask[u] set, mask[v] clear, fewer than 3 kept atoms) or 3 (a coordinate that
// is not finite).  No index is used as an address before it was checked.
__device__ int match_setup(MatchTables& T, const MatchProblem& P) {
  const int tid = threadIdx.x, nt = blockDim.x, n = P.n_lig, R = P.n_rot;
  bool bad = false, inf = false;
  for (int k = tid; k < R; k += nt) {
    const int u = P.rot_bonds[2 * k], v = P.rot_bonds[2 * k + 1];
    if (u < 0 || u >= n || v < 0 || v >= n || u == v) bad = true;
    else if (P.mask_rotate[(size_t)k * n + u] != 0 || P.mask_rotate[(size_t)k * n + v] == 0) bad = true;
    else T.uv[k] = make_int2(u, v);
  }
  for (int i = tid; i < 3 * n; i += nt) inf = inf || !isfinite(P.pos0[i]) || !isfinite(P.target[i]);
  for (int w = tid; w < 8; w += nt) {
    uint32_t b = 0;
    for (int j = 0; j < 32; ++j) {
      const int i = 32 * w + j;
      if (i < n && (P.atom_mask == nullptr || P.atom_mask[i] != 0)) b |= 1u << j;
    }
    T.keep[w] = b;
  }
  const int any_bad = __syncthreads_or(bad), any_inf = __syncthreads_or(inf);
  int m = 0;
  for (int w = 0; w < 8; ++w) m += __popc(T.keep[w]);
  if (any_bad || m < 3) return 2;
  if (any_inf) return 3;
  for (int e = tid; e < R * 8; e += nt) {
    const int k = e >> 3, w = e & 7;
    uint32_t b = 0;
    for (int j = 0; j < 32; ++j) {
      const int i = 32 * w + j;
      if (i < n && P.mask_rotate[(size_t)k * n + i] != 0) b |= 1u << j;
    }
    T.bits[k][w] = b;
  }
  __shared__ float c0[3];
  if (tid < 64) {      // the two centroids in fp64, rounded once (component_sum_wave0's reasoning, k_se3.hip)
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += 64) {
      const bool kept = bit_of(T.keep, i);
      for (int c = 0; c < 3; ++c) {
        s[c] += (double)P.pos0[3 * i + c];
        if (kept) s[3 + c] += (double)P.target[3 * i + c];
      }
    }
    for (int c = 0; c < 6; ++c) s[c] = wave_sum(s[c]);
    if (tid < 3) { c0[tid] = (float)(s[tid] / (double)n); T.ct[tid] = (float)(s[3 + tid] / (double)m); }
    if (tid == 0) T.m = m;
  }
  __syncthreads();
  for (int i = tid; i < 3 * n; i += nt) { T.pos0[i] = P.pos0[i] - c0[i % 3]; T.tgt[i] = P.target[i] - T.ct[i % 3]; }
  __syncthreads();
  if (tid < 64) {
    double s[3] = {0, 0, 0};
    for (int i = tid; i < n; i += 64)
      if (bit_of(T.keep, i))
        for (int c = 0; c < 3; ++c) s[c] += (double)T.tgt[3 * i + c];
    for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]) / (double)m;
    double g = 0;
    for (int i = tid; i < n; i += 64)
      if (bit_of(T.keep, i))
        for (int c = 0; c < 3; ++c) { const double d = (double)T.tgt[3 * i + c] - s[c]; g += d * d; }
    g = wave_sum(g);
    if (tid < 3) T.tc[tid] = s[tid];
    if (tid == 0) T.Gb = g;
  }
  __syncthreads();
  return 0;
}

__device__ inline void match_load_tables(MatchTables& T, const void* workspace) {
  const uint32_t* src = (const uint32_t*)((const char*)workspace + MATCH_TABLES_AT);
  uint32_t* dst = (uint32_t*)&T;
  for (int i = threadIdx.x; i < (int)(sizeof(MatchTables) / 4); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

struct MatchFit { double S[9], cF[3]; };

// Orders the LDS accesses of ONE wave: what its lanes wrote before is what any of its lanes reads after.  A wave's LDS operations complete in order, so
// this costs no wait on another wave; it keeps the compiler from moving or caching the accesses across it.
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The objective for one torsion vector, by one wave: `xyz` [3 n_lig] is the wave's own LDS, `theta` [n_rot] is read by every lane and may be shared with
// other waves (the caller puts a workgroup barrier between an evaluation and the next write to a shared theta).  Inside, only wave-local ordering: the waves
// of a workgroup are not coupled and need not call it together.  Returns the RMSD in every lane; fit != nullptr also gets the covariance of
// (conformer, target) and the conformer's centroid, which the final fit turns into a rotation.  xyz keeps the torsioned conformer.
__device__ inline float match_eval(const MatchTables& T, float* xyz, const float* theta, int n, int n_rot, int lane, MatchFit* fit) {
  for (int i = lane; i < 3 * n; i += 64) xyz[i] = T.pos0[i];
  wave_lds_sync();
  for (int k = 0; k < n_rot; ++k) {
    const float th = theta[k];
    if (th != 0.0f) {      // a rotor with a zero angle is skipped, as in the reference
      const int2 uv = T.uv[k];
      float Rl[9], piv[3];
      bond_rotor(xyz, uv.x, uv.y, th, Rl, piv);
      // in place: u is not in the mask and v, the pivot, maps to itself exactly, so the two atoms every lane has just read keep their values
      for (int i = lane; i < n; i += 64)
        if (bit_of(T.bits[k], i)) {
          float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
          rotate_about(Rl, piv, x, y, z);
          xyz[3 * i] = x; xyz[3 * i + 1] = y; xyz[3 * i + 2] = z;
        }
    }
    wave_lds_sync();
  }
  double c[3] = {0, 0, 0};
  for (int i = lane; i < n; i += 64)
    if (bit_of(T.keep, i)) { c[0] += (double)xyz[3 * i]; c[1] += (double)xyz[3 * i + 1]; c[2] += (double)xyz[3 * i + 2]; }
  const double inv_m = 1.0 / (double)T.m;
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = wave_sum(c[a]) * inv_m;
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Ga = 0;
  for (int i = lane; i < n; i += 64)
    if (bit_of(T.keep, i)) {
      const double a0 = (double)xyz[3 * i] - c[0], a1 = (double)xyz[3 * i + 1] - c[1], a2 = (double)xyz[3 * i + 2] - c[2];
      const double b0 = (double)T.tgt[3 * i] - T.tc[0], b1 = (double)T.tgt[3 * i + 1] - T.tc[1], b2 = (double)T.tgt[3 * i + 2] - T.tc[2];
      S[0] += a0 * b0; S[1] += a0 * b1; S[2] += a0 * b2;
      S[3] += a1 * b0; S[4] += a1 * b1; S[5] += a1 * b2;
      S[6] += a2 * b0; S[7] += a2 * b1; S[8] += a2 * b2;
      Ga += a0 * a0 + a1 * a1 + a2 * a2;
    }
#pragma unroll
  for (int a = 0; a < 9; ++a) S[a] = wave_sum(S[a]);
  Ga = wave_sum(Ga);
  if (fit != nullptr) {
#pragma unroll
    for (int a = 0; a < 9; ++a) fit->S[a] = S[a];
    fit->cF[0] = c[0]; fit->cF[1] = c[1]; fit->cF[2] = c[2];
  }
  const double msd = (Ga + T.Gb - 2.0 * horn_top_eigenvalue(S)) * inv_m;
  return (float)sqrt(msd < 0.0 ? 0.0 : msd);      // (a NaN stays a NaN)
}

// index draws by integer arithmetic on the 24-bit uniforms: floor(u k) without a float rounding
__device__ inline int draw_below(uint32_t x, int k) { return (int)(((uint64_t)(x >> 8) * (uint64_t)k) >> 24); }

struct MatchArgs {
  int n_lig, n_rot, NP, n_islands;
  float tol;
  uint64_t seed, stream_id;
  void* workspace;
  float* pop[2];      // [n_islands, NP, n_rot]
  float* cost[2];     // [n_islands, NP]
};

__global__ __launch_bounds__(256) void match_validate_kernel(MatchProblem P, void* workspace, int32_t* count_out) {
  __shared__ MatchTables T;
  MatchHeader* H = (MatchHeader*)workspace;
  const int status = match_setup(T, P);
  const int tid = threadIdx.x;
  if (tid == 0) { H->status = status; H->pad = 0; count_out[0] = 0; count_out[1] = status; }
  if (tid < MATCH_MAX_ISLANDS) H->gens[tid] = 0;
  if (status != 0) return;
  uint32_t* dst = (uint32_t*)((char*)workspace + MATCH_TABLES_AT);
  const uint32_t* src = (const uint32_t*)&T;
  // (rows of bits / uv past n_rot and coordinates past n_lig were never written: they are copied as they are and never read)
  for (int i = tid; i < (int)(sizeof(MatchTables) / 4); i += 256) dst[i] = src[i];
}

// generation g of every island; g = 0 draws and evaluates the population
__global__ __launch_bounds__(64 * MATCH_WAVES) void match_generation_kernel(MatchArgs A, int g) {
  __shared__ MatchTables T;
  __shared__ float xyz[MATCH_WAVES][MAX_LIG * 3], theta[MATCH_WAVES][MATCH_MAX_ROT];
  __shared__ double red[MATCH_WAVES];
  __shared__ float red_c[MATCH_WAVES];
  __shared__ int red_i[MATCH_WAVES];
  if (((const MatchHeader*)A.workspace)->status != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n_lig, R = A.n_rot, NP = A.NP;
  const int blocks_per_island = (NP + MATCH_WAVES - 1) / MATCH_WAVES;
  const int island = blockIdx.x / blocks_per_island, chunk = blockIdx.x - island * blocks_per_island;
  const int member = chunk * MATCH_WAVES + wave;
  const bool valid = member < NP;
  const int i = valid ? member : NP - 1;
  const size_t row0 = (size_t)island * NP;
  const float* pop_prev = A.pop[(g + 1) & 1] + row0 * R;
  const float* cost_prev = A.cost[(g + 1) & 1] + row0;
  float* pop_next = A.pop[g & 1] + row0 * R;
  float* cost_next = A.cost[g & 1] + row0;
  const RngStream rs = rng_stream(A.seed, A.stream_id);
  const uint32_t sample = (uint32_t)(row0 + i);
  int best = 0;
  if (g > 0) {
    // the island's state after generation g - 1, recomputed by every workgroup in one fixed order: mean, then the deviations, then the lowest cost
    double s = 0;
    for (int j = tid; j < NP; j += 256) s += (double)cost_prev[j];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const double mean = (red[0] + red[1] + red[2] + red[3]) / (double)NP;
    __syncthreads();
    double q = 0;
    float bc = INFINITY;
    int bi = NP;
    for (int j = tid; j < NP; j += 256) {
      const float cj = cost_prev[j];
      const double d = (double)cj - mean;
      q += d * d;
      if (cj < bc) { bc = cj; bi = j; }      // ascending j: ties stay with the lower index
    }
    q = wave_sum(q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float oc = __shfl_xor(bc, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (lane == 0) { red[wave] = q; red_c[wave] = bc; red_i[wave] = bi; }
    __syncthreads();
    const double sd = sqrt((red[0] + red[1] + red[2] + red[3]) / (double)NP);
    bc = red_c[0]; bi = red_i[0];
#pragma unroll
    for (int w = 1; w < MATCH_WAVES; ++w)
      if (red_c[w] < bc || (red_c[w] == bc && red_i[w] < bi)) { bc = red_c[w]; bi = red_i[w]; }
    best = bi < NP ? bi : 0;      // (every cost a NaN: member 0)
    if (sd <= (double)A.tol * fabs(mean)) {      // converged: the island stays as it is
      if (valid) {
        for (int d = lane; d < R; d += 64) pop_next[(size_t)i * R + d] = pop_prev[(size_t)i * R + d];
        if (lane == 0) cost_next[i] = cost_prev[i];
      }
      return;
    }
    if (chunk == 0 && tid == 0) ((MatchHeader*)A.workspace)->gens[island] = g;
  }
  match_load_tables(T, A.workspace);
  if (g == 0) {
    for (int d = lane; d < R; d += 64) {
      uint32_t w[4];
      rng_block(rs, sample, RNG_MATCH_POPULATION, 0, (uint32_t)(d >> 2), w);
      theta[wave][d] = (island == 0 && i == 0) ? 0.0f : rng_torsion(w[d & 3]);      // member 0 of island 0: the conformer as it is
    }
  } else {
    uint32_t w0[4], wf[4];
    rng_block(rs, sample, RNG_MATCH_GENERATION, (uint32_t)g, 0, w0);
    rng_block(rs, (uint32_t)row0, RNG_MATCH_GENERATION, (uint32_t)g, 0, wf);
    const float F = 0.5f + 0.5f * rng_uniform(wf[3]);
    int r1 = draw_below(w0[0], NP - 1);
    if (r1 >= i) ++r1;
    const int lo = r1 < i ? r1 : i, hi = r1 < i ? i : r1;
    int r2 = draw_below(w0[1], NP - 2);
    if (r2 >= lo) ++r2;
    if (r2 >= hi) ++r2;
    const int forced = draw_below(w0[2], R);
    for (int d = lane; d < R; d += 64) {
      uint32_t w[4];
      rng_block(rs, sample, RNG_MATCH_GENERATION, (uint32_t)g, (uint32_t)(1 + (d >> 2)), w);
      float t = pop_prev[(size_t)i * R + d];
      if (d == forced || rng_uniform(w[d & 3]) < MATCH_CR)
        t = wrap_angle(fmaf(F, pop_prev[(size_t)r1 * R + d] - pop_prev[(size_t)r2 * R + d], pop_prev[(size_t)best * R + d]));
      theta[wave][d] = t;
    }
  }
  __syncthreads();
  const float c = match_eval(T, xyz[wave], theta[wave], n, R, lane, nullptr);
  if (!valid) return;
  const bool take = g == 0 || c <= cost_prev[i];
  for (int d = lane; d < R; d += 64) pop_next[(size_t)i * R + d] = take ? theta[wave][d] : pop_prev[(size_t)i * R + d];
  if (lane == 0) cost_next[i] = take ? c : cost_prev[i];
}

struct MatchPolishArgs {
  MatchPolish* state[2];
  float* cand[2];      // [2 n_rot] costs of the neighbours theta +- h e_d, candidate 2 d is +, 2 d + 1 is -
};

// The state after a polish iteration from the state before it (`prev`) and that iteration's candidate costs (`cand`; nullptr: nothing was evaluated yet), by
// every thread of a workgroup, every workgroup the same: the best neighbour if it is strictly better (ties to the lowest candidate), otherwise half the
// step; h < 1e-4 ends the polish.  th [n_rot] is LDS.
__device__ inline void polish_fold(const MatchPolish* prev, const float* cand, int R, float* th, float& h, float& c_best, int& done) {
  __syncthreads();      // (th may still be read by a wave that is evaluating it)
  for (int d = threadIdx.x; d < R; d += blockDim.x) th[d] = prev->th[d];
  h = prev->h; c_best = prev->c_best; done = prev->done;
  __syncthreads();
  if (done || cand == nullptr) return;
  float bc = c_best;
  int bi = -1;
  for (int j = 0; j < 2 * R; ++j) {
    const float c = cand[j];
    if (c < bc) { bc = c; bi = j; }
  }
  if (bi >= 0) {
    if (threadIdx.x == 0) th[bi >> 1] = wrap_angle(th[bi >> 1] + ((bi & 1) ? -h : h));
    c_best = bc;
  } else {
    h *= 0.5f;
    if (h < MATCH_H_MIN) done = 1;
  }
  __syncthreads();
}

// one workgroup: the best member over the islands (ties to the lowest island, then member) becomes the polish's start; theta = 0 if no member beats it here
__global__ __launch_bounds__(64 * MATCH_POLISH_WAVES) void match_select_kernel(MatchArgs A, int fin, int polish_iters, MatchPolish* out) {
  constexpr int NW = MATCH_POLISH_WAVES, NT = 64 * NW;
  __shared__ MatchTables T;
  __shared__ float xyz[NW][MAX_LIG * 3], theta[NW][MATCH_MAX_ROT], th_best[MATCH_MAX_ROT];
  __shared__ float red_c[NW];
  __shared__ int red_i[NW];
  if (((const MatchHeader*)A.workspace)->status != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n_lig, R = A.n_rot;
  match_load_tables(T, A.workspace);
  for (int d = tid; d < R; d += NT) th_best[d] = 0.0f;
  __syncthreads();
  const float rigid = match_eval(T, xyz[wave], th_best, n, R, lane, nullptr);
  float c_best = rigid;
  const int total = A.n_islands * A.NP;
  const float* cost = A.cost[fin];
  float bc = INFINITY;
  int bi = total;
  for (int j = tid; j < total; j += NT) {
    const float cj = cost[j];
    if (cj < bc) { bc = cj; bi = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oc = __shfl_xor(bc, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
  }
  if (lane == 0) { red_c[wave] = bc; red_i[wave] = bi; }
  __syncthreads();
  bc = red_c[0]; bi = red_i[0];
#pragma unroll
  for (int w = 1; w < NW; ++w)
    if (red_c[w] < bc || (red_c[w] == bc && red_i[w] < bi)) { bc = red_c[w]; bi = red_i[w]; }
  // the search's cost of theta = 0 is `rigid` up to the roundings of another kernel's copy of match_eval: the member is taken only if it is not worse HERE
  if (bi < total) {
    for (int d = lane; d < R; d += 64) theta[wave][d] = A.pop[fin][(size_t)bi * R + d];
    __syncthreads();
    const float c = match_eval(T, xyz[wave], theta[wave], n, R, lane, nullptr);
    if (c <= rigid) {
      c_best = c;
      for (int d = tid; d < R; d += NT) th_best[d] = theta[0][d];
    }
    __syncthreads();
  }
  for (int d = tid; d < R; d += NT) out->th[d] = th_best[d];
  if (tid == 0) { out->h = MATCH_H0; out->c_best = c_best; out->done = polish_iters == 0; out->pad = 0; }
}

// polish iteration `it`: folds iteration it - 1, then one wave per neighbour of the new best vector.  Once the polish is done the launches that are left
// copy the state forward and return.
__global__ __launch_bounds__(64 * MATCH_WAVES) void match_polish_kernel(MatchArgs A, MatchPolishArgs P, int it) {
  __shared__ MatchTables T;
  __shared__ float xyz[MATCH_WAVES][MAX_LIG * 3], theta[MATCH_WAVES][MATCH_MAX_ROT], th[MATCH_MAX_ROT];
  if (((const MatchHeader*)A.workspace)->status != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n_lig, R = A.n_rot;
  float h, c_best;
  int done;
  polish_fold(P.state[(it + 1) & 1], it > 0 ? P.cand[(it + 1) & 1] : nullptr, R, th, h, c_best, done);
  if (blockIdx.x == 0) {
    MatchPolish* cur = P.state[it & 1];
    for (int d = tid; d < R; d += 64 * MATCH_WAVES) cur->th[d] = th[d];
    if (tid == 0) { cur->h = h; cur->c_best = c_best; cur->done = done; cur->pad = 0; }
  }
  if (done) return;
  match_load_tables(T, A.workspace);
  const int n_cand = 2 * R, cnd = blockIdx.x * MATCH_WAVES + wave, cc = cnd < n_cand ? cnd : n_cand - 1, dd = cc >> 1;
  for (int d = lane; d < R; d += 64) theta[wave][d] = d == dd ? wrap_angle(th[d] + ((cc & 1) ? -h : h)) : th[d];
  __syncthreads();
  const float c = match_eval(T, xyz[wave], theta[wave], n, R, lane, nullptr);
  if (lane == 0 && cnd < n_cand) P.cand[it & 1][cnd] = c;
}

struct MatchFinishArgs {
  MatchArgs A;
  MatchPolishArgs P;
  int polish_iters;
  float *torsions_out, *pos_out, *rmsd_out;
  int32_t* count_out;
};

// one workgroup: folds the last polish iteration, then the final fit and the stores
__global__ __launch_bounds__(64 * MATCH_WAVES) void match_finish_kernel(MatchFinishArgs F) {
  constexpr int NT = 64 * MATCH_WAVES;
  __shared__ MatchTables T;
  __shared__ float xyz[MATCH_WAVES][MAX_LIG * 3], th[MATCH_MAX_ROT];
  __shared__ float Rk[9], shift[6];
  const MatchArgs& A = F.A;
  const MatchHeader* H = (const MatchHeader*)A.workspace;
  if (H->status != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n_lig, R = A.n_rot;
  match_load_tables(T, A.workspace);
  for (int d = tid; d < R; d += NT) th[d] = 0.0f;
  __syncthreads();
  const float rigid = match_eval(T, xyz[wave], th, n, R, lane, nullptr);      // the conformer as it is: the rigid fit
  int gens = 0;
  if (R > 0) {
    float h, c_best;
    int done;
    polish_fold(F.P.state[(F.polish_iters + 1) & 1], F.polish_iters > 0 ? F.P.cand[(F.polish_iters + 1) & 1] : nullptr, R, th, h, c_best, done);
    for (int j = 0; j < A.n_islands; ++j) gens = H->gens[j] > gens ? H->gens[j] : gens;
  }
  // the matched conformer in the target's frame: rotation from the covariance (Horn), R (x - centroid) + the target's centroid
  MatchFit fit;
  float matched = match_eval(T, xyz[wave], th, n, R, lane, &fit);
  if (!(matched <= rigid)) {      // (only through the roundings of another kernel's copy of match_eval: rmsd_out[1] <= rmsd_out[0] is a guarantee)
    __syncthreads();
    for (int d = tid; d < R; d += NT) th[d] = 0.0f;
    __syncthreads();
    matched = match_eval(T, xyz[wave], th, n, R, lane, &fit);
  }
  if (tid == 0) {
    horn_rotation(fit.S, Rk);
    for (int a = 0; a < 3; ++a) { shift[a] = (float)fit.cF[a]; shift[3 + a] = (float)(T.tc[a] + (double)T.ct[a]); }
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) {
    const float x = xyz[0][3 * i] - shift[0], y = xyz[0][3 * i + 1] - shift[1], z = xyz[0][3 * i + 2] - shift[2];
    F.pos_out[3 * i] = Rk[0] * x + Rk[1] * y + Rk[2] * z + shift[3];
    F.pos_out[3 * i + 1] = Rk[3] * x + Rk[4] * y + Rk[5] * z + shift[4];
    F.pos_out[3 * i + 2] = Rk[6] * x + Rk[7] * y + Rk[8] * z + shift[5];
  }
  for (int d = tid; d < R; d += NT) F.torsions_out[d] = th[d];
  if (tid == 0) {
    F.rmsd_out[0] = rigid;
    F.rmsd_out[1] = matched;
    F.count_out[0] = gens;
    F.count_out[1] = 0;
  }
}

__global__ __launch_bounds__(64 * MATCH_WAVES) void conformer_rmsd_kernel(MatchProblem P, int M, int iters, const float* __restrict__ torsions,
                                                                           float* __restrict__ rmsd_out, int32_t* status_out) {
  __shared__ MatchTables T;
  __shared__ float xyz[MATCH_WAVES][MAX_LIG * 3], theta[MATCH_WAVES][MATCH_MAX_ROT];
  const int status = match_setup(T, P);
  if (blockIdx.x == 0 && threadIdx.x == 0) status_out[0] = status;
  if (status != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = P.n_lig, R = P.n_rot;
  for (int it = 0; it < iters; ++it) {
    const int64_t cnd = ((int64_t)it * gridDim.x + blockIdx.x) * MATCH_WAVES + wave;
    const int64_t row = cnd < M ? cnd : M - 1;
    for (int d = lane; d < R; d += 64) theta[wave][d] = torsions[row * R + d];
    __syncthreads();
    const float c = match_eval(T, xyz[wave], theta[wave], n, R, lane, nullptr);
    if (lane == 0 && cnd < M) rmsd_out[cnd] = c;
  }
}

}  // namespace

int64_t match_workspace_bytes(int n_lig, int n_rot, int popsize, int n_islands) {
  return (int64_t)match_layout(n_rot, match_members(popsize, n_rot), n_islands).total;
}

hipError_t launch_conformer_rmsd(const MatchProblem& P, int M, const float* torsions, float* rmsd_out, int32_t* status_out, hipStream_t s) {
  const int groups = (M + MATCH_WAVES - 1) / MATCH_WAVES, grid = groups < MATCH_RMSD_GRID ? groups : MATCH_RMSD_GRID;
  const int iters = (groups + grid - 1) / grid;
  hipLaunchKernelGGL(conformer_rmsd_kernel, dim3(grid), dim3(64 * MATCH_WAVES), 0, s, P, M, iters, torsions, rmsd_out, status_out);
  return hipGetLastError();
}

hipError_t launch_conformer_match(const MatchProblem& P, const MatchSearch& O, float* torsions_out, float* pos_out, float* rmsd_out, int32_t* count_out,
                                  void* workspace, hipStream_t s) {
  MatchArgs A;
  A.n_lig = P.n_lig; A.n_rot = P.n_rot; A.NP = match_members(O.popsize, P.n_rot); A.n_islands = O.n_islands;
  A.tol = O.tol; A.seed = O.seed; A.stream_id = O.stream_id; A.workspace = workspace;
  const MatchLayout L = match_layout(P.n_rot, A.NP, O.n_islands);
  for (int k = 0; k < 2; ++k) { A.pop[k] = (float*)((char*)workspace + L.pop[k]); A.cost[k] = (float*)((char*)workspace + L.cost[k]); }
  hipLaunchKernelGGL(match_validate_kernel, dim3(1), dim3(256), 0, s, P, workspace, count_out);
  MatchFinishArgs F;
  for (int k = 0; k < 2; ++k) { F.P.state[k] = (MatchPolish*)((char*)workspace + L.polish[k]); F.P.cand[k] = (float*)((char*)workspace + L.cand[k]); }
  if (P.n_rot > 0) {      // (no rotor: nothing to search or polish, the reference's `if rotable_bonds:`)
    const int grid = O.n_islands * ((A.NP + MATCH_WAVES - 1) / MATCH_WAVES);
    for (int g = 0; g <= O.maxiter; ++g) hipLaunchKernelGGL(match_generation_kernel, dim3(grid), dim3(64 * MATCH_WAVES), 0, s, A, g);
    // iteration 0 of the polish reads the buffer iteration -1 would have written
    hipLaunchKernelGGL(match_select_kernel, dim3(1), dim3(64 * MATCH_POLISH_WAVES), 0, s, A, O.maxiter & 1, O.polish_iters, F.P.state[1]);
    const int pgrid = (2 * P.n_rot + MATCH_WAVES - 1) / MATCH_WAVES;
    for (int it = 0; it < O.polish_iters; ++it) hipLaunchKernelGGL(match_polish_kernel, dim3(pgrid), dim3(64 * MATCH_WAVES), 0, s, A, F.P, it);
  }
  F.A = A; F.polish_iters = O.polish_iters;
  F.torsions_out = torsions_out; F.pos_out = pos_out; F.rmsd_out = rmsd_out; F.count_out = count_out;
  hipLaunchKernelGGL(match_finish_kernel, dim3(1), dim3(64 * MATCH_WAVES), 0, s, F);
  return hipGetLastError();
}

}  // namespace ddk
