// SE(3) x torus conformer update of one reverse-diffusion step, one workgroup per sample
// (reference utils/diffusion_utils.py:37-55 modify_conformer_batch, utils/geometry.py:6-85,126-156,
//  utils/torsion.py:71-86, and the perturbation arithmetic of utils/sampling.py:137-192):
//   upd   = score_coeff * score + noise_coeff * z                       (tr, rot, tor)
//   rigid = (pos - centroid) R(rot)^T + tr + centroid
//   flex  = sequential torsion rotations (in bond order, on already-updated coordinates)
//   out   = Kabsch-align(flex -> rigid)
// evaluated on centred coordinates: rigid and flex without "+ tr + centroid", which is added to the aligned pose at the end (same map, see the kernel)
// The 3x3 SVD of the reference is replaced by Horn's closed form (largest eigenvector of a 4x4 symmetric
// matrix, Jacobi in fp64 on one lane): same optimal proper rotation, reflection case included.
// One body, pose_update_body, runs from the centroid to the last store in se3_update_kernel<POST, REC> (the sampler) and in
// modify_conformer_batch_kernel (the ragged training batch); the heads' finish of the POST block is k_head_finish.h's, the rotor step k_geom.h's.
#include "model.h"
#include "k_geom.h"
#include "k_head_finish.h"
#include "k_philox.h"

namespace ddk {


// Sum of the n points p[3 i + c] per component c in fp64, called by the 64 lanes of the block's first wave: lane t < 48 sums every 16th point of component
// t % 3, four shuffle steps fold the 16 partial sums, lanes 0..2 return the totals of x, y, z.  fp64 with one rounding at the end because a sequential fp32
// sum of 256 coordinates near 150 A ends 1e-4 A off, five times the error of the fp32 reference's mean, and the centroid goes into every output atom
// (tests/test_gpu_geometry_adversarial.py); 16 lanes per component because one lane's chain of n dependent additions was the longest serial piece here.
__device__ inline double component_sum_wave0(const float* p, int n, int lane) {
  double s = 0.0;
  if (lane < 48) {
    const int c = lane % 3;
    for (int i = lane / 3; i < n; i += 16) s += (double)p[3 * i + c];
  }
  s += __shfl_down(s, 24); s += __shfl_down(s, 12); s += __shfl_down(s, 6); s += __shfl_down(s, 3);
  return s;
}

// rigid_transform_Kabsch_3D_torch_batch (utils/geometry.py:126-156) for one point-set pair held in LDS: R, t with R a + t ~ b, proper
// rotation also in the reflection case.  All threads of the block call it (barriers inside); cA, cB [3], S [9], Rk [9], tk [3] in LDS.
__device__ void kabsch_block(const float* a, const float* bpts, int n, float* cA, float* cB, double* S, float* Rk, float* tk) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const double sa = component_sum_wave0(a, n, tid), sb = component_sum_wave0(bpts, n, tid);
    if (tid < 3) { cA[tid] = (float)(sa / (double)n); cB[tid] = (float)(sb / (double)n); }
  }
  __syncthreads();
  if (tid < 9) {
    const int r = tid / 3, c = tid % 3;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)(a[3 * i + r] - cA[r]) * (double)(bpts[3 * i + c] - cB[c]);
    S[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    horn_rotation(S, Rk);
    for (int k = 0; k < 3; ++k) tk[k] = -(Rk[3 * k] * cA[0] + Rk[3 * k + 1] * cA[1] + Rk[3 * k + 2] * cA[2]) + cB[k];
  }
  __syncthreads();
}

// test hooks (include/ddk_debug.h): the device functions above on caller-supplied inputs
__global__ __launch_bounds__(256) void debug_kabsch_kernel(const float* A, const float* Bp, int n, float* R_out, float* t_out) {
  __shared__ float a[MAX_LIG * 3], bb[MAX_LIG * 3], cA[3], cB[3], Rk[9], tk[3];
  __shared__ double S[9];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < n * 3; i += 256) { a[i] = A[(size_t)b * n * 3 + i]; bb[i] = Bp[(size_t)b * n * 3 + i]; }
  __syncthreads();
  kabsch_block(a, bb, n, cA, cB, S, Rk, tk);
  if (tid < 9) R_out[9 * b + tid] = Rk[tid];
  if (tid < 3) t_out[3 * b + tid] = tk[tid];
}

__global__ void debug_axis_angle_kernel(const float* aa, int n, float* R_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) axis_angle_to_matrix_dev(aa[3 * i], aa[3 * i + 1], aa[3 * i + 2], R_out + 9 * i);
}

hipError_t launch_debug_kabsch(const float* A, const float* Bp, int B, int n, float* R_out, float* t_out, hipStream_t s) {
  hipLaunchKernelGGL(debug_kabsch_kernel, dim3(B), dim3(256), 0, s, A, Bp, n, R_out, t_out);
  return hipGetLastError();
}

hipError_t launch_debug_axis_angle(const float* aa, int n, float* R_out, hipStream_t s) {
  hipLaunchKernelGGL(debug_axis_angle_kernel, dim3((n + 63) / 64), dim3(64), 0, s, aa, n, R_out);
  return hipGetLastError();
}

// The LDS of one pose update: the rigid pose, the two buffers the rotor loop alternates between, and the small per-sample quantities.
struct PoseLds {
  float rig[MAX_LIG * 3], flx[2][MAX_LIG * 3];
  float upd[6], ctr[3], Rm[9], cA[3], cB[3], Rk[9], tk[3], rot_th[64];
  int2 rot_uv[64];
  double S[9];
};

// The pose update from the centroid to the last store, by all 256 threads of a workgroup (barriers inside).  The caller has filled L.rig with the n atoms
// of the pose and L.upd with (tr, rot), and has passed a barrier behind those stores.  flexible = the R rotors turn; mask_rotate [R, n] says
// which atoms.  What differs between the kernels comes in as two inlined callables: rotor(r, u, v, th) gives rotor r's bond (u, v) and angle, called
// once per rotor by one thread; store(i, x, y, z) puts atom i of the new pose where it belongs.  se3_update_kernel<POST, REC> and
// modify_conformer_batch_kernel are this one body, which is why a graph of the ragged batch gets the bits of the same ligand alone
// (tests/test_gpu_noise_batch.py, tests/test_gpu_pose_bits.py).
template <class Rotor, class Store>
__device__ __forceinline__ void pose_update_body(PoseLds& L, int n, int R, bool flexible, const uint8_t* mask_rotate, Rotor rotor, Store store) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const double s = component_sum_wave0(L.rig, n, tid);
    if (tid < 3) L.ctr[tid] = (float)(s / (double)n);
  }
  if (tid == 64) axis_angle_to_matrix_dev(L.upd[3], L.upd[4], L.upd[5], L.Rm);
  __syncthreads();
  if (tid < n) {
    const float x = L.rig[3 * tid] - L.ctr[0], y = L.rig[3 * tid + 1] - L.ctr[1], z = L.rig[3 * tid + 2] - L.ctr[2];
    // CENTRED coordinates from here to the last line: tr + centroid is added once, to the final pose.  With it added here the rotor
    // axes (differences of two atoms 1.5 A apart) and every rotated atom carry roundings of the DISTANCE FROM THE ORIGIN, and a chain of rotors amplifies
    // them by its lever arms: 150 A out a 129-rotor chain ended up to 5e-3 A from fp64 (tests/test_geometry_bound.py), centred it is as exact as at the origin
    const float rx = L.Rm[0] * x + L.Rm[1] * y + L.Rm[2] * z;
    const float ry = L.Rm[3] * x + L.Rm[4] * y + L.Rm[5] * z;
    const float rz = L.Rm[6] * x + L.Rm[7] * y + L.Rm[8] * z;
    // every thread owns its atom: safe to overwrite in place after the barrier above
    L.rig[3 * tid] = rx; L.rig[3 * tid + 1] = ry; L.rig[3 * tid + 2] = rz;
    L.flx[0][3 * tid] = rx; L.flx[0][3 * tid + 1] = ry; L.flx[0][3 * tid + 2] = rz;
  }
  __syncthreads();
  if (!flexible) {
    if (tid < n) store(tid, L.rig[3 * tid] + L.upd[0] + L.ctr[0], L.rig[3 * tid + 1] + L.upd[1] + L.ctr[1], L.rig[3 * tid + 2] + L.upd[2] + L.ctr[2]);
    return;
  }
  // Sequential torsion rotations, one barrier per rotor: the rotor table (u, v, angle) and every atom's mask bits are fetched for up to 64 rotors at
  // once (one exposed memory latency per chunk instead of three per rotor), every thread builds the rotor's matrix itself from the CURRENT
  // coordinates (same instruction sequence on every lane) and writes its atom into the other of two coordinate buffers.
  float* cur = L.flx[0];
  float* nxt = L.flx[1];
  for (int r0 = 0; r0 < R; r0 += 64) {
    const int chunk = min(64, R - r0);
    if (tid < chunk) {
      int u, v;
      float th;
      rotor(r0 + tid, u, v, th);
      L.rot_uv[tid] = make_int2(u, v);
      L.rot_th[tid] = th;
    }
    unsigned long long mbits = 0ull;
    if (tid < n)
      for (int k = 0; k < chunk; ++k) mbits |= (unsigned long long)(mask_rotate[(size_t)(r0 + k) * n + tid] != 0) << k;
    __syncthreads();
    for (int k = 0; k < chunk; ++k) {
      if (tid < n) {
        float x = cur[3 * tid], y = cur[3 * tid + 1], z = cur[3 * tid + 2];
        if ((mbits >> k) & 1ull) {
          float Rl[9], piv[3];
          bond_rotor(cur, L.rot_uv[k].x, L.rot_uv[k].y, L.rot_th[k], Rl, piv);
          rotate_about(Rl, piv, x, y, z);
        }
        nxt[3 * tid] = x; nxt[3 * tid + 1] = y; nxt[3 * tid + 2] = z;
      }
      __syncthreads();
      float* t_ = cur; cur = nxt; nxt = t_;
    }
  }
  kabsch_block(cur, L.rig, n, L.cA, L.cB, L.S, L.Rk, L.tk);
  if (tid < n) {
    const float x = cur[3 * tid], y = cur[3 * tid + 1], z = cur[3 * tid + 2];
    // Rk (x, y, z) + tk + upd + ctr with every multiply-add WRITTEN OUT: left to the compiler's contraction, which product of a row is rounded before
    // the others are fused onto it comes out differently in the recording and the plain instantiations (one body, two sets of bits).  These chains,
    // rows 1 and 2 starting from their middle product, are the ones tests/golden/pose_update_bits.json pins: do not reorder them.
    const float ox = fmaf(L.Rk[2], z, fmaf(L.Rk[1], y, L.Rk[0] * x)) + L.tk[0] + L.upd[0] + L.ctr[0];
    const float oy = fmaf(L.Rk[5], z, fmaf(L.Rk[3], x, L.Rk[4] * y)) + L.tk[1] + L.upd[1] + L.ctr[1];
    const float oz = fmaf(L.Rk[8], z, fmaf(L.Rk[6], x, L.Rk[7] * y)) + L.tk[2] + L.upd[2] + L.ctr[2];
    store(tid, ox, oy, oz);
  }
}

// POST: the workgroup of sample b first finishes the sample's scores from the heads' accumulators - heads_post_kernel's arithmetic, through the same
// functions (k_head_finish.h), on 256 threads over chunks of 64 bonds - so that a reverse step needs no launch between the head convolutions and the
// update (ddk_sample without classifier-free guidance)
// REC: the workgroup also stores what it consumed and produced into the step's rows of a ddk_trajectory (Se3Args::rec_*; ddk_sample_trajectory).  A template
// flag, not a run-time test: the <POST, false> instantiations carry no trace of it.
template <bool POST, bool REC>
__global__ __launch_bounds__(256) void se3_update_kernel(Se3Args A, HeadArgs H) {
  __shared__ PoseLds L;
  const int b = blockIdx.x, tid = threadIdx.x, n = A.n_lig, R = A.R;
  if constexpr (POST) {
    __shared__ float v48[64][2 * NS], hid[64][NS], g12[12];
    if (H.prof_out != nullptr && b == (int)gridDim.x - 1 && tid < PROF_INTS) H.prof_out[tid] = H.exec_info[tid];
    if (A.tor != nullptr && R > 0) {
      for (int r0 = 0; r0 < R; r0 += 64) {
        const int chunk = min(64, R - r0);
        for (int i = tid; i < chunk * 2 * NS; i += 256) {
          const int rr = i / (2 * NS), c = i - rr * 2 * NS;
          const int bond = b * R + r0 + rr;
          v48[rr][c] = tor_bn_element(H, H.h_sum + (size_t)(H.B + bond) * XW, H.h_deg[bond], c);
        }
        __syncthreads();
        for (int i = tid; i < chunk * NS; i += 256) {
          const int rr = i / NS, k = i - rr * NS;
          hid[rr][k] = tor_hidden_unit(H, v48[rr], k);
        }
        __syncthreads();
        if (tid < chunk) H.tor_out[(size_t)b * R + r0 + tid] = tor_score_sum(H, hid[tid]);
        __syncthreads();
      }
    }
    if (tid < 12) g12[tid] = center_element(H, H.h_sum + (size_t)b * XW, tid);
    __syncthreads();
    if (tid < 2) tr_rot_score(H, g12, tid, b);   // tid 0: translation, tid 1: rotation
    __syncthreads();      // the scores written above are read back through A.tr / A.rot / A.tor below (same workgroup)
  }
  const float* nz = A.noise ? A.noise + (size_t)b * (6 + R) : nullptr;
  for (int i = tid; i < n * 3; i += 256) L.rig[i] = A.pos[(size_t)b * n * 3 + i];
  if (tid < 6) {
    const int k = tid / 3;
    const float sc = (tid < 3 ? A.tr : A.rot)[3 * b + tid % 3];
    const float u = A.sc[k] * sc + (nz ? A.nc[k] * nz[tid] : 0.0f);
    L.upd[tid] = u;
    if constexpr (REC) {
      if (A.rec_scores != nullptr) A.rec_scores[(size_t)b * (6 + R) + tid] = sc;
      if (A.rec_perturb != nullptr) A.rec_perturb[(size_t)b * (6 + R) + tid] = u;
    }
  }
  if constexpr (REC) {      // batch totals of the four edge groups of the graph this step's forward ran on (ddk_last_graph_stats out[0..3])
    if (A.rec_edges != nullptr && b == 0 && tid < 4) A.rec_edges[tid] = A.info[I_GO + 1 + tid] - A.info[I_GO + tid];
  }
  __syncthreads();
  const bool flexible = A.tor != nullptr && R > 0;
  pose_update_body(
      L, n, R, flexible, A.mask_rotate,
      [&](int r, int& u, int& v, float& th) {
        u = A.rot_u[r]; v = A.rot_v[r];
        const float ts = A.tor[(size_t)b * R + r];
        th = A.sc[2] * ts + (nz ? A.nc[2] * nz[6 + r] : 0.0f);
        if constexpr (REC) {
          if (A.rec_scores != nullptr) A.rec_scores[(size_t)b * (6 + R) + 6 + r] = ts;
          if (A.rec_perturb != nullptr) A.rec_perturb[(size_t)b * (6 + R) + 6 + r] = th;
        }
      },
      [&](int i, float x, float y, float z) {
        float* o = A.pos_out + ((size_t)b * n + i) * 3;
        o[0] = x; o[1] = y; o[2] = z;
        if constexpr (REC)
          if (A.rec_pos != nullptr) {
            float* q = A.rec_pos + ((size_t)b * n + i) * 3;
            q[0] = x; q[1] = y; q[2] = z;
          }
      });
  if constexpr (REC)      // no_torsion: the torsion columns of the record's rows are zero
    if (!flexible)
      for (int r = tid; r < R; r += 256) {
        if (A.rec_scores != nullptr) A.rec_scores[(size_t)b * (6 + R) + 6 + r] = 0.0f;
        if (A.rec_perturb != nullptr) A.rec_perturb[(size_t)b * (6 + R) + 6 + r] = 0.0f;
      }
}

// modify_conformer (utils/diffusion_utils.py) for a RAGGED batch, one workgroup per graph (include/ddk.h: ddk_modify_conformer_batch): graph g has its own
// atom count, rotor table and mask block, found through node_ptr / tor_ptr / mask_ptr.  From the centroid on this is pose_update_body, as in
// se3_update_kernel<false, false> with B = 1, score_coeff = 1 and no noise; the update of component k is `score + 0.0f`, what 1 * score + 0 rounds to.  So a
// graph gets the bits ddk_se3_update gives the same ligand alone.  Before any table entry becomes an address the workgroup
// checks it; status_out[g]: 0 done; 2 a bond index outside [0, n_g) or u == v; 3 a coordinate that is not finite; 4 a node_ptr / tor_ptr / mask_ptr entry
// that is no range of the arrays or breaks a limit.  With a status other than 0 the graph's rows of pos_out are not written.
__global__ __launch_bounds__(256) void modify_conformer_batch_kernel(ConformerBatchArgs A) {
  __shared__ PoseLds L;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = A.node_ptr[g], n = A.node_ptr[g + 1] - n0;
  bool tables_ok = n0 >= 0 && n >= 1 && n <= MAX_LIG && n0 <= A.N - n;
  int R = 0, t0 = 0, m0 = 0;
  if (A.tor != nullptr) {
    t0 = A.tor_ptr[g]; R = A.tor_ptr[g + 1] - t0; m0 = A.mask_ptr[g];
    tables_ok = tables_ok && t0 >= 0 && R >= 0 && R <= NOISE_BATCH_MAX_ROT && t0 <= A.T - R && m0 >= 0 && A.mask_ptr[g + 1] - m0 == R * n &&
                m0 <= A.mask_bytes - R * n;
  }
  if (!tables_ok) {      // (the same in every thread: the block leaves as one)
    if (tid == 0) A.status_out[g] = 4;
    return;
  }
  const float* pos = A.pos + (size_t)n0 * 3;
  float* pos_out = A.pos_out + (size_t)n0 * 3;
  const int32_t* bonds = A.rot_bonds + (size_t)t0 * 2;
  const float* tor = A.tor != nullptr ? A.tor + t0 : nullptr;
  int bad_pos = 0, bad_bond = 0;
  for (int i = tid; i < n * 3; i += 256) {
    const float v = pos[i];
    L.rig[i] = v;
    bad_pos |= !isfinite(v);
  }
  for (int r = tid; r < R; r += 256) {
    const int u = bonds[2 * r], v = bonds[2 * r + 1];
    bad_bond |= u < 0 || u >= n || v < 0 || v >= n || u == v;
  }
  if (tid < 6) L.upd[tid] = (tid < 3 ? A.tr : A.rot)[3 * g + tid % 3] + 0.0f;
  bad_pos = __syncthreads_or(bad_pos);
  bad_bond = __syncthreads_or(bad_bond);
  if (bad_pos || bad_bond) {
    if (tid == 0) A.status_out[g] = bad_bond ? 2 : 3;
    return;
  }
  if (tid == 0) A.status_out[g] = 0;
  pose_update_body(
      L, n, R, tor != nullptr && R > 0, A.mask_rotate + m0,
      [&](int r, int& u, int& v, float& th) { u = bonds[2 * r]; v = bonds[2 * r + 1]; th = tor[r] + 0.0f; },
      [&](int i, float x, float y, float z) { pos_out[3 * i] = x; pos_out[3 * i + 1] = y; pos_out[3 * i + 2] = z; });
}

hipError_t launch_modify_conformer_batch(const ConformerBatchArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(modify_conformer_batch_kernel, dim3(A.G), dim3(256), 0, s, A);
  return hipGetLastError();
}

// randomize_position (utils/sampling.py:12-34) for B copies of one conformer, one workgroup per sample:
// sequential torsion updates in bond order (utils/torsion.py:48-68: axis pos_u - pos_v, pivot pos_v, zero updates skipped),
// then (pos - centroid) R^T + tr with the caller's rotation matrix and translation draw.
__global__ __launch_bounds__(256) void randomize_kernel(RandPosArgs A) {
  __shared__ float p[MAX_LIG * 3];
  __shared__ float Rt[9], piv[3], ctr[3];
  __shared__ int skip;
  const int b = blockIdx.x, tid = threadIdx.x, n = A.n_lig, R = A.R;
  for (int i = tid; i < n * 3; i += 256) p[i] = A.pos0[i];
  __syncthreads();
  if (A.tor != nullptr) {
    for (int r = 0; r < R; ++r) {
      if (tid == 0) {      // thread 0 builds the rotor, all apply it
        const float th = A.tor[(size_t)b * R + r];
        skip = th == 0.0f;
        bond_rotor(p, A.rot_u[r], A.rot_v[r], th, Rt, piv);
      }
      __syncthreads();
      if (!skip && tid < n && A.mask_rotate[(size_t)r * n + tid]) {
        float x = p[3 * tid], y = p[3 * tid + 1], z = p[3 * tid + 2];
        rotate_about(Rt, piv, x, y, z);
        p[3 * tid] = x; p[3 * tid + 1] = y; p[3 * tid + 2] = z;
      }
      __syncthreads();
    }
  }
  if (tid < 64) {
    const double s = component_sum_wave0(p, n, tid);
    if (tid < 3) ctr[tid] = (float)(s / (double)n);
  }
  __syncthreads();
  if (tid < n) {
    const float* M = A.rot + (size_t)b * 9;
    const float x = p[3 * tid] - ctr[0], y = p[3 * tid + 1] - ctr[1], z = p[3 * tid + 2] - ctr[2];
    float ox = M[0] * x + M[1] * y + M[2] * z, oy = M[3] * x + M[4] * y + M[5] * z, oz = M[6] * x + M[7] * y + M[8] * z;
    if (A.tr != nullptr) { ox += A.tr[3 * b]; oy += A.tr[3 * b + 1]; oz += A.tr[3 * b + 2]; }
    float* o = A.pos_out + ((size_t)b * n + tid) * 3;
    o[0] = ox; o[1] = oy; o[2] = oz;
  }
}

hipError_t launch_randomize(const RandPosArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(randomize_kernel, dim3(A.B), dim3(256), 0, s, A);
  return hipGetLastError();
}

// randomize_position for a RAGGED batch of G different ligands, one workgroup per graph (include/ddk.h: ddk_randomize_position_batch): graph g is the global
// sample sample[g] of stream stream_id[g]; its tables are found through node_ptr / tor_ptr / mask_ptr as in modify_conformer_batch_kernel, with that kernel's
// checks and status codes (a sample < 0 counts as a bad table entry).  The workgroup makes the graph's draws itself, with rng_initial_kernel's expressions
// (k_rng.hip; purposes 1, 2, 3 of DDK_RNG_LAYOUT 1) into LDS, and then runs randomize_kernel's arithmetic on them, statement for statement, so a graph gets the
// bits ddk_rng_initial + ddk_randomize_position give the same ligand alone.  Each draw goes through LDS before it is used: a product formed here is rounded
// as the one rng_initial_kernel stores, never fused into the addition that consumes it.
// rng_rotation (k_philox.h) with every multiply-add WRITTEN OUT as rng_initial_kernel's code object evaluates it: there the contraction of the quaternion's
// products was left to the compiler, which fuses some of them and not others, and a second kernel that inlines the same source need not get the same choice
// (this one did not).  The chains below are read off that code object: the norm starts from the unfused sum of the first two squares; R[3], R[7] and
// R[8] add rounded products; the other six fuse one product.  Doubling is exact either way.  Do not reorder them: the bit-for-bit contract with
// ddk_rng_initial rests on them (tests/test_gpu_randomize_batch.py).
__device__ __forceinline__ void rotation_as_rng_initial(const float q[4], float* R) {
#pragma clang fp contract(off)
  const float s01 = q[0] * q[0] + q[1] * q[1];
  const float n2 = fmaf(q[3], q[3], fmaf(q[2], q[2], s01));
  if (!(n2 >= 0x1p-60f)) {
    R[0] = 1.f; R[1] = 0.f; R[2] = 0.f; R[3] = 0.f; R[4] = 1.f; R[5] = 0.f; R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
    return;
  }
  const float inv = 1.0f / sqrtf(n2);
  const float x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
  const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const float xy = x * y, zw = z * w, yw = y * w, xw = x * w, yz = y * z;
  const float r1 = fmaf(x, y, -zw), r2 = fmaf(x, z, yw), r3 = xy + zw, r5 = fmaf(y, z, -xw), r6 = fmaf(x, z, -yw), r7 = yz + xw;
  R[0] = fmaf(w, w, (x2 - y2) - z2); R[1] = r1 + r1;                     R[2] = r2 + r2;
  R[3] = r3 + r3;                     R[4] = fmaf(w, w, (y2 - x2) - z2); R[5] = r5 + r5;
  R[6] = r6 + r6;                     R[7] = r7 + r7;                     R[8] = (z2 + (-x2 - y2)) + w2;
}

__global__ __launch_bounds__(256) void randomize_batch_kernel(RandPosBatchArgs A) {
  __shared__ float p[MAX_LIG * 3];
  __shared__ float tor[NOISE_BATCH_MAX_ROT];
  __shared__ float Rt[9], piv[3], ctr[3], M[9], trv[3];
  __shared__ int skip;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = A.node_ptr[g], n = A.node_ptr[g + 1] - n0;
  bool tables_ok = n0 >= 0 && n >= 1 && n <= MAX_LIG && n0 <= A.N - n && A.sample[g] >= 0;
  int R = 0, t0 = 0, m0 = 0;
  if (A.tor_ptr != nullptr) {
    t0 = A.tor_ptr[g]; R = A.tor_ptr[g + 1] - t0; m0 = A.mask_ptr[g];
    tables_ok = tables_ok && t0 >= 0 && R >= 0 && R <= NOISE_BATCH_MAX_ROT && t0 <= A.T - R && m0 >= 0 && A.mask_ptr[g + 1] - m0 == R * n &&
                m0 <= A.mask_bytes - R * n;
  }
  if (!tables_ok) {      // (the same in every thread: the block leaves as one)
    if (tid == 0) A.status_out[g] = 4;
    return;
  }
  const float* pos = A.pos + (size_t)n0 * 3;
  const int32_t* bonds = A.rot_bonds + (size_t)t0 * 2;
  const uint8_t* mask = A.mask_rotate + m0;
  int bad_pos = 0, bad_bond = 0;
  for (int i = tid; i < n * 3; i += 256) {
    const float v = pos[i];
    p[i] = v;
    bad_pos |= !isfinite(v);
  }
  for (int r = tid; r < R; r += 256) {
    const int u = bonds[2 * r], v = bonds[2 * r + 1];
    bad_bond |= u < 0 || u >= n || v < 0 || v >= n || u == v;
  }
  bad_pos = __syncthreads_or(bad_pos);
  bad_bond = __syncthreads_or(bad_bond);
  if (bad_pos || bad_bond) {
    if (tid == 0) A.status_out[g] = bad_bond ? 2 : 3;
    return;
  }
  if (tid == 0) A.status_out[g] = 0;
  // the draws: item j < n_tor_blk the torsion block j, j = n_tor_blk the rotation, j = n_tor_blk + 1 the translation
  const RngStream S = rng_stream(((uint64_t)A.seed_hi << 32) | A.seed_lo, A.stream_id[g]);
  const uint32_t sample = (uint32_t)A.sample[g];
  const int n_tor_blk = (R + 3) >> 2;
  for (int j = tid; j < n_tor_blk + 2; j += 256) {
    uint32_t w[4];
    if (j < n_tor_blk) {
      rng_block(S, sample, RNG_INIT_TORSION, 0, (uint32_t)j, w);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 4 * j + q;
        if (r < R) tor[r] = rng_torsion(w[q]);
      }
    } else if (j == n_tor_blk) {
      float q[4];
      rng_block(S, sample, RNG_INIT_ROTATION, 0, 0, w);
      rng_normals(w, q);
      rotation_as_rng_initial(q, M);
    } else {
      float z[4];
      rng_block(S, sample, RNG_INIT_TRANSLATION, 0, 0, w);
      rng_normals(w, z);
#pragma unroll
      for (int e = 0; e < 3; ++e) trv[e] = A.tr_sigma * z[e];
    }
  }
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    if (tid == 0) {      // thread 0 builds the rotor, all apply it
      const float th = tor[r];
      skip = th == 0.0f;
      bond_rotor(p, bonds[2 * r], bonds[2 * r + 1], th, Rt, piv);
    }
    __syncthreads();
    if (!skip && tid < n && mask[(size_t)r * n + tid]) {
      float x = p[3 * tid], y = p[3 * tid + 1], z = p[3 * tid + 2];
      rotate_about(Rt, piv, x, y, z);
      p[3 * tid] = x; p[3 * tid + 1] = y; p[3 * tid + 2] = z;
    }
    __syncthreads();
  }
  if (tid < 64) {
    const double s = component_sum_wave0(p, n, tid);
    if (tid < 3) ctr[tid] = (float)(s / (double)n);
  }
  __syncthreads();
  if (tid < n) {
    const float x = p[3 * tid] - ctr[0], y = p[3 * tid + 1] - ctr[1], z = p[3 * tid + 2] - ctr[2];
    float ox, oy, oz;
    {
      // randomize_kernel's three rows with every multiply-add WRITTEN OUT as that kernel's code object evaluates them (its contraction was left to the
      // compiler, which packs rows 0 and 1 and leaves row 2 on its own: row 1 starts from its middle product, row 2 adds its last product unfused).
      // These chains are what the bit-for-bit contract with ddk_randomize_position rests on (tests/test_gpu_randomize_batch.py): do not reorder them.
#pragma clang fp contract(off)
      ox = fmaf(M[2], z, fmaf(M[1], y, M[0] * x));
      oy = fmaf(M[5], z, fmaf(M[3], x, M[4] * y));
      const float oz_xy = fmaf(M[6], x, M[7] * y), oz_z = M[8] * z;
      oz = oz_xy + oz_z;
      ox += trv[0]; oy += trv[1]; oz += trv[2];
    }
    float* o = A.pos_out + ((size_t)n0 + tid) * 3;
    o[0] = ox; o[1] = oy; o[2] = oz;
  }
}

hipError_t launch_randomize_batch(const RandPosBatchArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(randomize_batch_kernel, dim3(A.G), dim3(256), 0, s, A);
  return hipGetLastError();
}

// pose metrics of evaluate.py:297-338, one workgroup per pose (see include/ddk.h: ddk_pose_metrics)
__global__ __launch_bounds__(256) void pose_metrics_kernel(const float* pos, const float* ref, const uint8_t* mask, const int32_t* perms, int n_perms,
                                                           const float* rec_pos, int n_lig, int n_rec, float* out) {
  __shared__ float p[MAX_LIG * 3], rf[MAX_LIG * 3];
  __shared__ unsigned char keep[MAX_LIG];
  __shared__ float red[4][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < n_lig * 3; i += 256) { p[i] = pos[(size_t)b * n_lig * 3 + i]; rf[i] = ref[i]; }
  for (int i = tid; i < n_lig; i += 256) keep[i] = mask ? (mask[i] != 0) : 1;
  __syncthreads();
  float cnt = 0.f, cx = 0.f, cy = 0.f, cz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
  float mcross = INFINITY, mself = INFINITY;
  for (int i = tid; i < n_lig; i += 256)
    if (keep[i]) {
      cnt += 1.f;
      cx += p[3 * i]; cy += p[3 * i + 1]; cz += p[3 * i + 2];
      rx += rf[3 * i]; ry += rf[3 * i + 1]; rz += rf[3 * i + 2];
      for (int j = 0; j < n_lig; ++j)
        if (j != i && keep[j]) {
          const float ex = p[3 * i] - p[3 * j], ey = p[3 * i + 1] - p[3 * j + 1], ez = p[3 * i + 2] - p[3 * j + 2];
          mself = fminf(mself, ex * ex + ey * ey + ez * ez);
        }
    }
  // RMSD: the symmetry-corrected one of evaluate.py:308-310 (spyrmsd symmrmsd without minimisation) = the minimum over the graph
  // automorphisms G of sqrt(mean_i |pos[G(i)] - ref[i]|^2); n_perms = 0 / perms = null: identity only (the fallback of :313).
  // One thread per permutation (each sum is n_lig terms in atom order: deterministic), then a block minimum.
  float best = INFINITY;
  const int K = perms ? n_perms : 1;
  for (int k = tid; k < K; k += 256) {
    float s2 = 0.f;
    for (int i = 0; i < n_lig; ++i)
      if (keep[i]) {
        const int j = perms ? perms[(size_t)k * n_lig + i] : i;
        if ((unsigned)j >= (unsigned)n_lig) { s2 = INFINITY; break; }      // not a ligand atom: this table row can never be the minimum (rmsd = inf if none is valid)
        const float dx = p[3 * j] - rf[3 * i], dy = p[3 * j + 1] - rf[3 * i + 1], dz = p[3 * j + 2] - rf[3 * i + 2];
        s2 += dx * dx + dy * dy + dz * dz;
      }
    best = fminf(best, s2);
  }
  for (int r = tid; r < n_rec; r += 256) {
    const float qx = rec_pos[3 * r], qy = rec_pos[3 * r + 1], qz = rec_pos[3 * r + 2];
    for (int i = 0; i < n_lig; ++i)
      if (keep[i]) {
        const float ex = qx - p[3 * i], ey = qy - p[3 * i + 1], ez = qz - p[3 * i + 2];
        mcross = fminf(mcross, ex * ex + ey * ey + ez * ez);
      }
  }
  // block reductions: sums of (cnt, centroid components) and the three minima
  float vals[7] = {cnt, cx, cy, cz, rx, ry, rz};
  float sums[7];
  for (int k = 0; k < 7; ++k) {
    red[0][tid] = vals[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[0][tid] += red[0][tid + o]; __syncthreads(); }
    sums[k] = red[0][0];
    __syncthreads();
  }
  red[1][tid] = mcross; red[2][tid] = mself; red[3][tid] = best;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[1][tid] = fminf(red[1][tid], red[1][tid + o]); red[2][tid] = fminf(red[2][tid], red[2][tid + o]);
      red[3][tid] = fminf(red[3][tid], red[3][tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float n = fmaxf(sums[0], 1.f);
    const float dx = (sums[1] - sums[4]) / n, dy = (sums[2] - sums[5]) / n, dz = (sums[3] - sums[6]) / n;
    out[4 * b + 0] = sqrtf(red[3][0] / n);
    out[4 * b + 1] = sqrtf(dx * dx + dy * dy + dz * dz);
    out[4 * b + 2] = sqrtf(red[1][0]);
    out[4 * b + 3] = sqrtf(red[2][0]);
  }
}

hipError_t launch_pose_metrics(const float* pos, const float* ref, const uint8_t* mask, const int32_t* perms, int n_perms, const float* rec_pos,
                               int B, int n_lig, int n_rec, float* out, hipStream_t s) {
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(B), dim3(256), 0, s, pos, ref, mask, perms, n_perms, rec_pos, n_lig, n_rec, out);
  return hipGetLastError();
}

// classifier-free guidance: score <- score + w * (score - score_unconditional)   (utils/sampling.py:131-133)
__global__ void cfg_combine_kernel(float* score, const float* uncond, float w, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) score[i] = score[i] + w * (score[i] - uncond[i]);
}

hipError_t launch_cfg_combine(float* score, const float* uncond, float weight, int64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(cfg_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, score, uncond, weight, n);
  return hipGetLastError();
}

hipError_t launch_se3(const Se3Args& A, hipStream_t s, const HeadArgs* post) {
  const bool rec = A.rec_pos != nullptr || A.rec_scores != nullptr || A.rec_perturb != nullptr || A.rec_edges != nullptr;
  HeadArgs H0 = {};
  const HeadArgs& H = post ? *post : H0;
  if (post && rec) hipLaunchKernelGGL((se3_update_kernel<true, true>), dim3(A.B), dim3(256), 0, s, A, H);
  else if (post) hipLaunchKernelGGL((se3_update_kernel<true, false>), dim3(A.B), dim3(256), 0, s, A, H);
  else if (rec) hipLaunchKernelGGL((se3_update_kernel<false, true>), dim3(A.B), dim3(256), 0, s, A, H);
  else hipLaunchKernelGGL((se3_update_kernel<false, false>), dim3(A.B), dim3(256), 0, s, A, H);
  return hipGetLastError();
}

}  // namespace ddk

extern "C" int ddk_modify_conformer_batch(ddk_ctx* ctx, int32_t G, int32_t N, const float* pos, const int32_t* node_ptr, int32_t T, const int32_t* rot_bonds,
                                          const uint8_t* mask_rotate, const int32_t* mask_ptr, int32_t mask_bytes, const int32_t* tor_ptr,
                                          const float* tr_update, const float* rot_update, const float* tor_update, float* pos_out, int32_t* status_out,
                                          void* stream) {
  using namespace ddk;
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (G < 1 || G > NOISE_BATCH_MAX_GRAPHS)
    return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: G must be in [1, " + std::to_string(NOISE_BATCH_MAX_GRAPHS) + "]");
  if (N < G || (int64_t)N > (int64_t)G * MAX_LIG)
    return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: N must be in [G, G * " + std::to_string(MAX_LIG) + "] (n_lig of a graph is in [1, " +
                                          std::to_string(MAX_LIG) + "])");
  if (T < 0 || (int64_t)T > (int64_t)G * NOISE_BATCH_MAX_ROT)
    return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: T must be in [0, G * " + std::to_string(NOISE_BATCH_MAX_ROT) + "]");
  if (mask_bytes < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: mask_bytes must be >= 0");
  if (!pos || !node_ptr || !tr_update || !rot_update) return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: null argument (pos, node_ptr, tr_update, rot_update)");
  if (!pos_out || !status_out) return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: null output (pos_out, status_out)");
  if (tor_update && (!tor_ptr || !mask_ptr || (T > 0 && (!rot_bonds || !mask_rotate))))
    return fail(ctx, DDK_ERR_INVALID, "ddk_modify_conformer_batch: tor_update without the rotor tables (tor_ptr, mask_ptr, and with T > 0 rot_bonds, mask_rotate)");
  ConformerBatchArgs A{pos, node_ptr, tor_ptr, mask_ptr, rot_bonds, mask_rotate, tr_update, rot_update, tor_update, G, N, T, mask_bytes, pos_out, status_out};
  hipError_t e = launch_modify_conformer_batch(A, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "modify_conformer_batch launch");
  return DDK_OK;
}

extern "C" int ddk_randomize_position_batch(ddk_ctx* ctx, uint64_t seed, int32_t G, int32_t N, const float* pos, const int32_t* node_ptr, int32_t T,
                                            const int32_t* rot_bonds, const uint8_t* mask_rotate, const int32_t* mask_ptr, int32_t mask_bytes,
                                            const int32_t* tor_ptr, const uint64_t* stream_id, const int32_t* sample, float tr_sigma_max, float* pos_out,
                                            int32_t* status_out, void* stream) {
  using namespace ddk;
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (G < 1 || G > NOISE_BATCH_MAX_GRAPHS)
    return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: G must be in [1, " + std::to_string(NOISE_BATCH_MAX_GRAPHS) + "]");
  if (N < G || (int64_t)N > (int64_t)G * MAX_LIG)
    return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: N must be in [G, G * " + std::to_string(MAX_LIG) + "] (n_lig of a graph is in [1, " +
                                          std::to_string(MAX_LIG) + "])");
  if (T < 0 || (int64_t)T > (int64_t)G * NOISE_BATCH_MAX_ROT)
    return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: T must be in [0, G * " + std::to_string(NOISE_BATCH_MAX_ROT) + "]");
  if (mask_bytes < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: mask_bytes must be >= 0");
  if (!(tr_sigma_max >= 0.f) || !(tr_sigma_max < INFINITY)) return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: tr_sigma_max must be finite and >= 0");
  if (!pos || !node_ptr || !stream_id || !sample) return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: null argument (pos, node_ptr, stream_id, sample)");
  if (!pos_out || !status_out) return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: null output (pos_out, status_out)");
  if (tor_ptr && (!mask_ptr || (T > 0 && (!rot_bonds || !mask_rotate))))
    return fail(ctx, DDK_ERR_INVALID, "ddk_randomize_position_batch: tor_ptr without the rotor tables (mask_ptr, and with T > 0 rot_bonds, mask_rotate)");
  RandPosBatchArgs A{pos, node_ptr, tor_ptr, mask_ptr, rot_bonds, mask_rotate, stream_id, sample, (uint32_t)seed, (uint32_t)(seed >> 32), tr_sigma_max,
                     G, N, T, mask_bytes, pos_out, status_out};
  hipError_t e = launch_randomize_batch(A, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "randomize_position_batch launch");
  return DDK_OK;
}
