// Host side of the fused conv kernels: everything that turns a state dict into a ConvLayerDev.  The tile table and weight-row map of a layer
// (build_layout), the BatchNorm fold, the fp32 MFMA fragments of the radial MLP (fill_gemm1 / fill_gemm2, fp32_records), the f16-limb records
// (pack_x3) and the two layer builders ddk_finalize_weights calls (build_conv_layer, build_head_layer).  All of it runs in host-only contexts too.
#include <math.h>
#include <algorithm>
#include <cmath>
#include <string.h>

#include "model.h"
#include "k_conv_common.h"

namespace ddk {

// row of the 32x32 MFMA D tile held by accumulator register r of lane-half hh
static inline int d_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
// hidden-unit index consumed by GEMM2 step s in lane-half hh (== D layout of GEMM1, see k_conv.hip)
static inline int hid_of(int s, int hh) { return s < 32 ? 32 * (s / 16) + d_row(s % 16, hh) : 64 + (s - 32) + 4 * hh; }
// input index consumed by GEMM1 step s in lane-half hh
static inline int kin_of(int s, int hh) { return 24 * (s / 12) + 12 * hh + (s % 12); }

// fp32 fragment arrays are [tile][9][64][4]: register s (0..35) of `lane` in tile t
constexpr int FRAG_FLOATS = 9 * 64 * 4;                                            // 2304: one 32-row tile
constexpr size_t W1_FLOATS = 3 * FRAG_FLOATS, B1_FLOATS = 3 * 2 * 16;              // GEMM1 of one group: three row tiles, b1 [3][2][16]
static inline size_t frag_index(int t, int s, int lane) { return (((size_t)t * 9 + s / 4) * 64 + lane) * 4 + (s & 3); }

struct RowSrc { int wbase; float scale; };           // weight of (row, channel k) = W2[wbase + k] * scale
struct Part { int kind, f_off, dot_which; std::vector<RowSrc> rows; };   // dot_which >= 0: rows live in the F_PQ layout

// Tile table + weight-row map of one conv layer.  mode 0: FasterTensorProduct (tensor_layers.py:58-63,72-92: blocks 0e,1o,1e,0o,
// weights [in_,out] row-major, 1/sqrt(in_)); mode 1: e3nn FullyConnectedTensorProduct(in, 0e+1o+2e, out, shared_weights=False)
// as all_atom_score_model.py:25 builds it: instructions in (in1, sh, out) loop order with 'uvw' weights [mul_in, 1, mul_out],
// path coefficient sqrt(dim_out / sum of mul_in over the paths into that output irrep), real wigner-3j with Frobenius norm 1
// (w3j(0,1,1)=w3j(1,0,1)=w3j(1,1,0)=delta/sqrt3, w3j(1,1,1)=eps/sqrt6, w3j(1,2,1).Y2 = sqrt(3/2) (v^ v^T - I/3)).
static int build_layout(ddk_ctx* ctx, int mode, int l, ConvLayerDev& L, std::vector<int>& rowmap, std::vector<float>& rowscale,
                        std::vector<TileDesc>& tiles) {
  const ddk_config& c = ctx->cfg;
  const int ns = c.ns, nv = c.nv;
  const int seq[4][4] = {{ns, 0, 0, 0}, {ns, nv, 0, 0}, {ns, nv, nv, 0}, {ns, nv, nv, ns}};
  // modes 2 / 3: the output heads as layouts of the same kernel (score_model.py:132-161: tor_bond_conv / final_conv read the full irreps);
  // their "out" multiplicities are per FasterTensorProduct-style block (0e, 1o, 1e, 0o), the output columns are set below
  const int head_out[2][4] = {{ns, 0, 0, ns}, {0, 2, 2, 0}};
  const int* in = seq[(mode >= 2 || l >= 3) ? 3 : l];
  const int* out = mode >= 2 ? head_out[mode - 2] : seq[l + 1 < 3 ? l + 1 : 3];
  for (int b = 0; b < 4; ++b) { L.in_mul[b] = in[b]; L.out_mul[b] = out[b]; }
  L.n_out[0] = out[0]; L.n_out[1] = out[1]; L.n_out[2] = out[2]; L.n_out[3] = out[3];
  L.din = in[0] + 3 * in[1] + 3 * in[2] + in[3];
  L.dout = out[0] + 3 * out[1] + 3 * out[2] + out[3];
  if (in[2] > 0 && in[1] == 0) return fail(ctx, DDK_ERR_INVALID, "unsupported irreps sequence");

  std::vector<Part> parts[4];
  auto rows_of = [](int wbase0, int stride, int n, float scale) {
    std::vector<RowSrc> r;
    for (int i = 0; i < n; ++i) r.push_back({wbase0 + i * stride, scale});
    return r;
  };
  auto cat = [](std::vector<RowSrc> a, const std::vector<RowSrc>& b) { a.insert(a.end(), b.begin(), b.end()); return a; };
  if (mode == 0) {
    L.n_in[0] = in[0] + in[1];
    L.n_in[1] = in[0] + in[1] + in[2];
    L.n_in[2] = in[1] + in[2] + in[3];
    L.n_in[3] = in[2] + in[3];
    int off = 0;
    for (int b = 0; b < 4; ++b) { L.blk_off[b] = off; off += L.n_in[b] * L.n_out[b]; }
    L.W = off;
    auto blk = [&](int b, int row0, int n) { return rows_of(L.blk_off[b] + row0 * L.n_out[b], L.n_out[b], n, 1.0f / sqrtf((float)L.n_in[b])); };
    parts[0].push_back({T_RA, F_A, -1, blk(0, 0, in[0])});                                        // a * s0
    if (in[1]) parts[0].push_back({T_RT, 0, 0, blk(0, in[0], in[1])});                            // (p.v)/sqrt3
    parts[1].push_back({T_RA, F_A, -1, blk(1, 0, in[0])});                                        // a (x) v
    if (in[1] + in[2]) parts[1].push_back({T_TV, F_T1O, -1, blk(1, in[0], in[1] + in[2])});       // p*s0 ; (q x v)/sqrt2
    if (in[1] + in[2]) parts[2].push_back({T_TV, F_T1E, -1, blk(2, 0, in[1] + in[2])});           // (p x v)/sqrt2 ; q*s0
    if (in[3]) parts[2].push_back({T_RA, F_C, -1, blk(2, in[1] + in[2], in[3])});                 // c (x) v
    if (in[2]) parts[3].push_back({T_RT, 0, 1, blk(3, 0, in[2])});                                // (q.v)/sqrt3
    if (in[3]) parts[3].push_back({T_RA, F_C, -1, blk(3, in[2], in[3])});                         // c * s0
  } else if (mode == 2) {
    // tor_bond_conv: e3nn FullyConnectedTensorProduct(84, sh (x) sh_2e, '24x0o + 24x0e') keeps two paths (score_model.py:152-156): 1o (x) T -> 0e
    // (weights [nv][ns] at 0) and 1e (x) T -> 0o (at nv*ns), T = the 1o block of the full tensor product, path coefficient sqrt(1/nv) and
    // w3j(1,1,0) = delta/sqrt3.  The kernel forms (p.v)/sqrt3 and (q.v)/sqrt3 with v := T (heads_pre_kernel puts T into the edge's sh), which
    // leaves 1/sqrt(nv) for the packed weights.  Output columns: [0o | 0e].
    for (int b = 0; b < 4; ++b) { L.n_in[b] = (b == 0 || b == 3) ? nv : 0; L.blk_off[b] = 0; }
    L.W = 2 * nv * ns;
    const float sc = 1.0f / sqrtf((float)nv);
    parts[0].push_back({T_RT, 0, 0, rows_of(0, ns, nv, sc)});
    parts[3].push_back({T_RT, 0, 1, rows_of(nv * ns, ns, nv, sc)});
  } else if (mode == 3) {
    // final_conv: FullyConnectedTensorProduct(84, 0e+1o, '2x1o + 2x1e'), weight blocks in instruction order (score_model.py:132-139):
    //   A 0e(x)1o->1o [ns][2] | B 1o(x)0e->1o [nv][2] | C 1o(x)1o->1e [nv][2] | D 1e(x)0e->1e [nv][2] | E 1e(x)1o->1o [nv][2] | F 0o(x)1o->1e [ns][2]
    // path coefficient sqrt(3 / (ns + 2 nv)) = 1/sqrt12 for both outputs; w3j(0,1,1) = w3j(1,0,1) = delta/sqrt3, w3j(1,1,1) = eps/sqrt6;
    // the kernel's rows are a (x) v, p*s0, (q x v)/sqrt2 | (p x v)/sqrt2, q*s0, c (x) v  with s0 = 1, v = sh[1:4]
    for (int b = 0; b < 4; ++b) { L.n_in[b] = (b == 1 || b == 2) ? ns + 2 * nv : 0; L.blk_off[b] = 0; }
    L.W = 2 * 2 * (ns + 2 * nv);
    const float pc = sqrtf(3.0f / (float)(ns + 2 * nv));
    const float cS = pc * 0.57735026918962576451f, cX = pc * 0.40824829046386301637f * 1.41421356237309504880f;
    const int oA = 0, oB = 2 * ns, oC = oB + 2 * nv, oD = oC + 2 * nv, oE = oD + 2 * nv, oF = oE + 2 * nv;
    parts[1].push_back({T_RA, F_A, -1, rows_of(oA, 2, ns, cS)});
    parts[1].push_back({T_TV, F_T1O, -1, cat(rows_of(oB, 2, nv, cS), rows_of(oE, 2, nv, cX))});
    parts[2].push_back({T_TV, F_T1E, -1, cat(rows_of(oC, 2, nv, cX), rows_of(oD, 2, nv, cS))});
    parts[2].push_back({T_RA, F_C, -1, rows_of(oF, 2, ns, cS)});
  } else {
    // irreps as (l, parity): node 0e,1o,1e,0o ; sh 0e,1o,2e
    const int nl[4] = {0, 1, 1, 0}, np_[4] = {+1, -1, +1, -1}, sl[3] = {0, 1, 2}, sp[3] = {+1, -1, +1};
    int inst_off[4][3][4];
    int fan[4] = {0, 0, 0, 0}, off = 0;
    for (int i1 = 0; i1 < 4; ++i1)
      for (int i2 = 0; i2 < 3; ++i2)
        for (int io = 0; io < 4; ++io) {
          inst_off[i1][i2][io] = -1;
          if (!in[i1] || !out[io]) continue;
          const bool tri = nl[io] >= abs(nl[i1] - sl[i2]) && nl[io] <= nl[i1] + sl[i2];
          if (!tri || np_[i1] * sp[i2] != np_[io]) continue;
          inst_off[i1][i2][io] = off;
          off += in[i1] * out[io];
          fan[io] += in[i1];
        }
    L.W = off;
    for (int b = 0; b < 4; ++b) { L.n_in[b] = fan[b]; L.blk_off[b] = 0; }
    const float is3 = 0.57735026918962576451f, kappa = 1.22474487139158904910f;
    auto coeff = [&](int io) { return sqrtf((float)(2 * nl[io] + 1) / (float)fan[io]); };
    auto inst = [&](int i1, int i2, int io, float k) { return rows_of(inst_off[i1][i2][io], out[io], in[i1], coeff(io) * k); };
    if (out[0]) {
      parts[0].push_back({T_RA, F_A, -1, inst(0, 0, 0, 1.0f)});                                   // 0e x Y0 -> 0e : a*s0
      if (in[1]) parts[0].push_back({T_RT, 0, 0, inst(1, 1, 0, 1.0f)});                           // 1o x Y1 -> 0e : (p.v)/sqrt3
    }
    if (out[1]) {
      parts[1].push_back({T_RA, F_A, -1, inst(0, 1, 1, is3)});                                    // 0e x Y1 -> 1o : a v / sqrt3
      if (in[1]) {
        std::vector<RowSrc> r = inst(1, 0, 1, is3);                                               // 1o x Y0 -> 1o : p*s0 / sqrt3
        if (in[2]) r = cat(r, inst(2, 1, 1, is3));                                                // 1e x Y1 -> 1o : (q x v)/sqrt6
        parts[1].push_back({T_TV, F_T1O, -1, r});
        parts[1].push_back({T_TV, F_T2O, -1, inst(1, 2, 1, kappa)});                              // 1o x Y2 -> 1o
      }
    }
    if (out[2]) {
      if (in[1]) {
        std::vector<RowSrc> r = inst(1, 1, 2, is3);                                               // 1o x Y1 -> 1e : (p x v)/sqrt6
        if (in[2]) r = cat(r, inst(2, 0, 2, is3));                                                // 1e x Y0 -> 1e : q*s0 / sqrt3
        parts[2].push_back({T_TV, F_T1E, -1, r});
      }
      if (in[3]) parts[2].push_back({T_RA, F_C, -1, inst(3, 1, 2, is3)});                         // 0o x Y1 -> 1e : c v / sqrt3
      if (in[2]) parts[2].push_back({T_TV, F_T2E, -1, inst(2, 2, 2, kappa)});                     // 1e x Y2 -> 1e
    }
    if (out[3]) {
      if (in[2]) parts[3].push_back({T_RT, 0, 1, inst(2, 1, 3, 1.0f)});                           // 1e x Y1 -> 0o : (q.v)/sqrt3
      if (in[3]) parts[3].push_back({T_RA, F_C, -1, inst(3, 0, 3, 1.0f)});                        // 0o x Y0 -> 0o : c*s0
    }
  }

  int oc[4] = {0, out[0], out[0] + 3 * out[1], out[0] + 3 * out[1] + 3 * out[2]};
  if (mode == 2) { oc[0] = ns; oc[3] = 0; L.dout = 2 * ns; }       // '24x0o + 24x0e': the 0o channels come first
  if (mode == 3) { oc[1] = 0; oc[2] = 6; L.dout = 12; }
  // per tile row j: the block it belongs to (the shared tail tile holds two); has_x: accumulator quad rq = 3 of a 6-channel column carries
  // the rows xr[] of ANOTHER row quad for the channel pair xpair (see pack_quads below)
  struct TRow { int blk[4], col; RowSrc r[4]; bool ok[4]; bool has_x = false; int xpair = 0; RowSrc xr[4]; };
  std::vector<TRow> trows;
  tiles.clear();
  L.n_cols = 0;
  auto chan0_of = [&](int b, int col) { return oc[b] + ((b == 1 || b == 2) ? 3 : 1) * 8 * col; };
  auto nch_of = [&](int b, int col) { return L.n_out[b] - 8 * col < 8 ? L.n_out[b] - 8 * col : 8; };
  auto emit = [&](int b, int col, const Part& p, int f_off, int row0, int jlo, int cnt) {
    tiles.push_back(make_tile(p.kind, f_off, FL_NONE, nch_of(b, col) / 2, chan0_of(b, col)));
    TRow t; t.col = col;
    for (int j = 0; j < 4; ++j) { t.blk[j] = b; t.ok[j] = j >= jlo && j < jlo + cnt; if (t.ok[j]) t.r[j] = p.rows[row0 + j - jlo]; }
    trows.push_back(t);
  };
  // all tiles of one part of one output column; a dot-product part's tail (rows 4, 5: the [pv4 pv5 qv4 qv5] quad) can be left to the caller
  auto emit_part = [&](int b, int col, const Part& p, bool with_tail) -> int {
    const int n = (int)p.rows.size();
    if (p.dot_which >= 0) {     // F_PQ = [pv0..3 | qv0..3 | pv4 pv5 qv4 qv5]
      if (n > 6) return fail(ctx, DDK_ERR_INVALID, "dot-product parts hold at most 6 rows");
      emit(b, col, p, F_PQ + 4 * p.dot_which, 0, 0, n < 4 ? n : 4);
      if (n > 4 && with_tail) emit(b, col, p, F_PQ + 8, 4, 2 * p.dot_which, n - 4);
    } else {
      for (int q = 0; 4 * q < n; ++q) emit(b, col, p, p.f_off + (p.kind == T_TV ? 12 * q : 4 * q), 4 * q, 0, n - 4 * q < 4 ? n - 4 * q : 4);
    }
    return DDK_OK;
  };
  auto dot_part = [&](int b) -> const Part* {
    for (const Part& p : parts[b]) if (p.dot_which >= 0 && p.rows.size() > 4) return &p;
    return nullptr;
  };
  // The 0e and 0o blocks' dot-product parts (p.v, q.v: 6 rows each) would each end in a half-empty tile (pv4 pv5 . . / . . qv4 qv5).  When both
  // exist with the same output width they share ONE tile (kind T_RTS): the two columns of the same channel slots are laid out back to back,
  // [0e column ... | shared tail: flushes the 0e column, opens the 0o column | 0o column ...]  (3 tiles less for W = 1872 and W = 1152).
  const Part *dp0 = dot_part(0), *dp3 = dot_part(3);
  const bool share = mode == 0 && dp0 && dp3 && dp0->rows.size() == 6 && dp3->rows.size() == 6 && L.n_out[0] == L.n_out[3] &&
                     L.n_out[0] % 2 == 0;
  bool done[4] = {false, false, false, false};
  if (share) {
    for (int col = 0; 8 * col < L.n_out[0]; ++col) {
      if (L.n_cols >= 16) return fail(ctx, DDK_ERR_INVALID, "too many output columns");
      L.col_start[L.n_cols++] = (int)tiles.size();            // (one split point per PAIR of columns: the shared tile binds them)
      for (const Part& p : parts[0])
        if (int rc = emit_part(0, col, p, false)) return rc;
      tiles.push_back(make_tile(T_RTS, F_PQ + 8, FL_S, nch_of(0, col) / 2, chan0_of(0, col)));
      TRow t; t.col = col;
      for (int j = 0; j < 4; ++j) { t.blk[j] = j < 2 ? 0 : 3; t.ok[j] = true; t.r[j] = j < 2 ? dp0->rows[4 + j] : dp3->rows[4 + j - 2]; }
      trows.push_back(t);
      for (const Part& p : parts[3])
        if (int rc = emit_part(3, col, p, false)) return rc;
      tiles.back().w0 |= FL_S << 2;
    }
    done[0] = done[3] = true;
  }
  // A column of 6 output channels (the vector blocks: nv = 6) fills only 3 of a tile's 4 accumulator quads.  The 4th quad of the column's
  // first tiles carries the (row quad, channel pair) units of the column's LAST a (x) v / c (x) v row quads instead, whose own tiles disappear:
  // Q row quads -> ceil(3Q/4) tiles (9 -> 7 for in = 36 rows, 8 -> 6, 6 -> 5).  Tile word: bit 7 = extra unit present, bits 8-9 = its channel
  // pair, bits 10-13 = its F offset / 4 (an a / c quad).
  const bool pack_quads = mode == 0 || mode == 1;
  for (int b = 0; b < 4; ++b) {
    if (done[b] || parts[b].empty() || L.n_out[b] == 0) continue;
    if (L.n_out[b] % 2) return fail(ctx, DDK_ERR_INVALID, "odd output multiplicity unsupported");
    const bool vec = (b == 1 || b == 2);
    for (int col = 0; 8 * col < L.n_out[b]; ++col) {
      if (L.n_cols >= 16) return fail(ctx, DDK_ERR_INVALID, "too many output columns");
      L.col_start[L.n_cols++] = (int)tiles.size();
      const int t_first = (int)tiles.size();
      for (const Part& p : parts[b])
        if (int rc = emit_part(b, col, p, true)) return rc;
      if (pack_quads && vec && nch_of(b, col) == 6) {
        const int Q = (int)tiles.size() - t_first, T = (3 * Q + 3) / 4, n_x = Q - T;
        // the extras: the last n_x full scalar-row quads (kind T_RA, rows a or c) of the column
        std::vector<int> xs;
        for (int t = (int)tiles.size() - 1; t >= t_first && (int)xs.size() < n_x; --t) {
          const TRow& tr = trows[t];
          if ((tiles[t].w0 & 3) == T_RA && tr.ok[0] && tr.ok[1] && tr.ok[2] && tr.ok[3] && (tiles[t].w0 >> 16) % 4 == 0 && (tiles[t].w0 >> 16) < 64) xs.push_back(t);
        }
        if (n_x > 0 && (int)xs.size() == n_x) {
          std::vector<TileDesc> keep_t; std::vector<TRow> keep_r, x_r; std::vector<int> x_off;
          for (int t = t_first; t < (int)tiles.size(); ++t) {
            if (std::find(xs.begin(), xs.end(), t) != xs.end()) { x_r.push_back(trows[t]); x_off.push_back(tiles[t].w0 >> 16); }
            else { keep_t.push_back(tiles[t]); keep_r.push_back(trows[t]); }
          }
          for (int u = 0; u < 3 * n_x; ++u) {       // unit u = (extra quad u / 3, channel pair u % 3) rides on the column's tile u
            keep_r[u].has_x = true; keep_r[u].xpair = u % 3;
            for (int j = 0; j < 4; ++j) keep_r[u].xr[j] = x_r[u / 3].r[j];
            keep_t[u].w0 |= 0x80 | ((u % 3) << 8) | ((x_off[u / 3] / 4) << 10);
          }
          tiles.resize(t_first); trows.resize(t_first);
          tiles.insert(tiles.end(), keep_t.begin(), keep_t.end());
          trows.insert(trows.end(), keep_r.begin(), keep_r.end());
        }
      }
      tiles.back().w0 |= (vec ? FL_V : FL_S) << 2;
    }
  }
  if (mode == 3 && !ctx->cfg.deterministic) {      // (the deterministic scatter STORES: every output channel must be flushed exactly once)
    // final_conv has a handful of edge blocks (B * n_lig edges): the kernel's short-queue split hands out COLUMNS, so cut its two 9-tile columns
    // into flush columns of two tiles (a flush adds the partial sums to the same output channels: the sum is what counts)
    L.n_cols = 0;
    for (int t = 0; t < (int)tiles.size(); ++t) {
      const bool prev_flushes = t > 0 && ((tiles[t - 1].w0 >> 2) & 3) != FL_NONE;
      if (t == 0 || prev_flushes || t - L.col_start[L.n_cols - 1] == 2) {
        if (L.n_cols >= 16) return fail(ctx, DDK_ERR_INVALID, "too many output columns");
        if (t > 0 && !prev_flushes) tiles[t - 1].w0 |= FL_V << 2;
        L.col_start[L.n_cols++] = t;
      }
    }
  }
  L.n_tiles = (int)tiles.size();
  L.col_start[L.n_cols] = L.n_tiles;
  L.h_tiles = tiles;

  // row map: tile row rho = 8*rq + 4*hh + j  ->  index into the reference weight vector (or -1 = zero row) and its scale
  rowmap.assign((size_t)L.n_tiles * 32, -1);
  rowscale.assign((size_t)L.n_tiles * 32, 0.f);
  for (int t = 0; t < L.n_tiles; ++t) {
    const TRow& tr = trows[t];
    for (int rq = 0; rq < 4; ++rq)
      for (int hh = 0; hh < 2; ++hh)
        for (int j = 0; j < 4; ++j) {
          if (tr.has_x && rq == 3) {      // the extra unit: rows of another quad, channel pair xpair of the same column
            rowmap[(size_t)t * 32 + 8 * rq + 4 * hh + j] = tr.xr[j].wbase + 8 * tr.col + 2 * tr.xpair + hh;
            rowscale[(size_t)t * 32 + 8 * rq + 4 * hh + j] = tr.xr[j].scale;
            continue;
          }
          const int k = 8 * tr.col + 2 * rq + hh;
          if (!tr.ok[j] || k >= L.n_out[tr.blk[j]]) continue;
          rowmap[(size_t)t * 32 + 8 * rq + 4 * hh + j] = tr.r[j].wbase + k;
          rowscale[(size_t)t * 32 + 8 * rq + 4 * hh + j] = tr.r[j].scale;
        }
  }
  // every weight row must be used exactly once
  std::vector<int> cnt(L.W, 0);
  for (int r : rowmap) if (r >= 0) cnt[r]++;
  for (int r = 0; r < L.W; ++r) if (cnt[r] != 1) return fail(ctx, DDK_ERR_INVALID, "internal: weight row map is not a bijection");
  return DDK_OK;
}

// e3nn BatchNorm (eval) folded to per-channel mean / scale / bias over the padded XW columns
static int fold_batch_norm(ddk_ctx* ctx, const std::string& pre, const int* out, float* mean, float* scale, float* bias) {
  for (int i = 0; i < XW; ++i) { mean[i] = 0.f; scale[i] = 1.f; bias[i] = 0.f; }
  const int nf = out[0] + out[1] + out[2] + out[3];
  const HostTensor* bw = find_w(ctx, pre + ".weight", {nf});
  const HostTensor* bb = find_w(ctx, pre + ".bias", {out[0]});
  const HostTensor* bm = find_w(ctx, pre + ".running_mean", {out[0]});
  const HostTensor* bv = find_w(ctx, pre + ".running_var", {nf});
  if (!bw || !bb || !bm || !bv) return DDK_ERR_INVALID;
  int ch = 0, f = 0;
  const int dims[4] = {1, 3, 3, 1};
  for (int b = 0; b < 4; ++b)
    for (int m = 0; m < out[b]; ++m, ++f) {
      const float sc = powf(bv->data[f] + 1e-5f, -0.5f) * bw->data[f];
      for (int d = 0; d < dims[b]; ++d, ++ch) {
        scale[ch] = sc;
        if (b == 0) { mean[ch] = bm->data[m]; bias[ch] = bb->data[m]; }
      }
    }
  return DDK_OK;
}

// GEMM1 of one radial MLP (W1 [kin][kin], B1 [kin]) as fp32 fragments w1 [3][9][64][4] and accumulator-init rows b1 [3][2][16].  The kernel's
// GEMMs are 72 wide: input columns and hidden units at or beyond kin are zero (kin = 72 for the conv layers and tor_bond_conv, 48 for final_conv).
static void fill_gemm1(const HostTensor& W1, const HostTensor& B1, int kin, float* w1, float* b1) {
  for (int T = 0; T < 3; ++T) {
    for (int s = 0; s < 36; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int hidden = 32 * T + (lane & 31), k = kin_of(s, lane >> 5);
        w1[frag_index(T, s, lane)] = (hidden < kin && k < kin) ? W1.data[(size_t)hidden * kin + k] : 0.f;
      }
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r) {
        const int hidden = 32 * T + d_row(r, hh);
        b1[(T * 2 + hh) * 16 + r] = hidden < kin ? B1.data[hidden] : 0.f;
      }
  }
}

// GEMM2 of one radial MLP (W2 [W][kin], B2 [W]) as fp32 fragments w2 [n_tiles][9][64][4] and bias rows b2 [n_tiles][2][16]: tile row rho of
// tile t is weight row rowmap[32 t + rho] times rowscale[32 t + rho] (-1: a zero row), hidden units at or beyond kin are zero
static void fill_gemm2(const HostTensor& W2, const HostTensor& B2, int kin, const std::vector<int>& rowmap, const std::vector<float>& rowscale,
                       int n_tiles, float* w2, float* b2) {
  for (int t = 0; t < n_tiles; ++t) {
    for (int s = 0; s < 36; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const size_t rho = (size_t)t * 32 + (lane & 31);
        const int row = rowmap[rho], hd = hid_of(s, lane >> 5);
        w2[frag_index(t, s, lane)] = (row >= 0 && hd < kin) ? W2.data[(size_t)row * kin + hd] * rowscale[rho] : 0.f;
      }
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r) {
        const size_t rho = (size_t)t * 32 + d_row(r, hh);
        b2[((size_t)t * 2 + hh) * 16 + r] = rowmap[rho] >= 0 ? B2.data[rowmap[rho]] * rowscale[rho] : 0.f;
      }
  }
}

// W2 ring records of the fp32 kernel, [group][n_tiles][W2_TILE_FLOATS]: per tile [2304 fragment floats | bias [2][16] | the two descriptor words | 0 0]
// from the group-major fragments w2 and bias rows b2
static std::vector<float> fp32_records(const std::vector<float>& w2, const std::vector<float>& b2, const std::vector<TileDesc>& tiles, int n_groups) {
  const size_t n_tiles = tiles.size();
  std::vector<float> rec((size_t)n_groups * n_tiles * W2_TILE_FLOATS);
  for (size_t i = 0; i < n_groups * n_tiles; ++i) {
    float* r = rec.data() + i * W2_TILE_FLOATS;
    memcpy(r, w2.data() + i * FRAG_FLOATS, FRAG_FLOATS * sizeof(float));
    memcpy(r + FRAG_FLOATS, b2.data() + i * 32, 32 * sizeof(float));
    memcpy(r + FRAG_FLOATS + 32, &tiles[i % n_tiles], 2 * sizeof(int32_t));   // descriptor rides with the record (bit pattern)
  }
  return rec;
}

// The f16-limb kernels keep the raw p / q rows once ([p0..p5 | q0..q5], quads of four): the l = 2 group of the q rows (T2E), whose two
// tiles are [q0 q1 q2 q3], [q4 q5 . .] in the table, reads raw quads 1 and 2 = [. . q0 q1], [q2 q3 q4 q5]: move its weight rows accordingly
// (accumulator quads 0..2 only: quad 3 of a 6-channel column is empty or carries a packed extra unit).  x_tile_word() gives the tiles their offsets.
// rmx / rsx: the moved copies of rowmap / rowscale (confidence model only: the score model has no l = 2 rows).
static int t2e_row_remap(ddk_ctx* ctx, const std::vector<TileDesc>& tiles, const std::vector<int>& rowmap, const std::vector<float>& rowscale,
                         std::vector<int>& rmx, std::vector<float>& rsx) {
  rmx = rowmap;
  rsx = rowscale;
  for (int t = 0; t + 1 < (int)tiles.size(); ++t) {
    if ((tiles[t].w0 & 3) != T_TV || (tiles[t].w0 >> 16) != F_T2E) continue;
    if ((tiles[t + 1].w0 & 3) != T_TV || (tiles[t + 1].w0 >> 16) != F_T2E + 12) return fail(ctx, DDK_ERR_INVALID, "internal: the two tiles of a T2E row group are not adjacent");
    for (int rq = 0; rq < 3; ++rq)
      for (int hh = 0; hh < 2; ++hh) {
        const size_t a = (size_t)t * 32 + 8 * rq + 4 * hh, b = (size_t)(t + 1) * 32 + 8 * rq + 4 * hh;
        if (rowmap[b + 2] >= 0 || rowmap[b + 3] >= 0) return fail(ctx, DDK_ERR_INVALID, "internal: a T2E row group holds more than six rows");
        for (int j = 0; j < 2; ++j) {
          rmx[a + j] = -1; rsx[a + j] = 0.f;
          rmx[a + 2 + j] = rowmap[a + j]; rsx[a + 2 + j] = rowscale[a + j];
          rmx[b + j] = rowmap[a + 2 + j]; rsx[b + j] = rowscale[a + 2 + j];
          rmx[b + 2 + j] = rowmap[b + j]; rsx[b + 2 + j] = rowscale[b + j];
        }
      }
  }
  return DDK_OK;
}

// One fp32 value as fp16 limbs at their own weight: hi = fp16(v) at dst, mid = fp16(v - hi) at dst + limb_stride and, with three limbs,
// lo = fp16(v - hi - mid) at dst + 2 limb_stride (fp16 subnormals included).  Returns whether the limbs stand for v as their form promises.
// Three limbs must reproduce v bit for bit (values below 0.5 - more than 2^-15 under the group's maximum - within 2^-25); two limbs must stay in the
// window |v - hi - mid| <= max(2^-22 |v|, 2^-25).
static bool store_limbs(float v, int limbs, uint8_t* dst, size_t limb_stride) {
  const _Float16 h = (_Float16)v;
  const float r1 = v - (float)h;
  const _Float16 m = (_Float16)r1;
  const _Float16 l = (_Float16)(r1 - (float)m);
  memcpy(dst, &h, 2); memcpy(dst + limb_stride, &m, 2);
  if (limbs == 3) {
    memcpy(dst + 2 * limb_stride, &l, 2);
    const double back = (double)(float)h + (double)(float)m + (double)(float)l;
    return !(std::fabs(v) >= 0.5f ? back != (double)v : std::fabs(back - (double)v) > 0x1p-25);
  }
  const double back = (double)(float)h + (double)(float)m;
  return !(std::fabs(back - (double)v) > std::max(0x1p-22 * std::fabs((double)v), 0x1p-25));
}

// f16-limb records of a layer's radial-MLP weights for k_conv_x.hip / k_conv_x2.hip: every (range-scaled) fp32 weight v becomes
// hi + mid + lo with hi = fp16(v), mid = fp16(v - hi), lo = fp16(v - hi - mid), each limb carrying its own weight (store_limbs).
// Three limbs are exact whenever the last bit of v is a multiple of the fp16 subnormal step 2^-24, i.e. for |v| >= 0.5 after scaling (the group's
// maximum is scaled into [2^14, 2^15)); smaller values are off by at most 2^-25 = 2^-39 of the maximum.  Checked here for every value.
// w1all / w2all: the fp32 fragment arrays [.][s/4][lane][s&3] (s = register of the lane half), b2all [t][2][16].
// A layer is packed in the form it runs: conv_kernel = 3 keeps the three-limb records (W2X_TILE_BYTES, W1X_TILE_BYTES); the default two-limb form
// (ConvLayerDev::limbs == 2, k_conv_x2.hip) gets the records without the lo limb it never reads (W2X2_TILE_BYTES, W1X2_TILE_BYTES): hi and mid are the same bits at
// the same offsets.  Two limbs are not exact: |v - hi - mid| <= 2^-22 |v| (mid = fp16(v - hi) rounds a remainder of <= 2^-11 |v| to 11 bits), or <= 2^-25
// where mid is an fp16 subnormal.  That window is checked here for every value instead of exactness.
// sender_k48: also pack the K = 48 GEMM1 records of the node-term split (score-model conv layers in the two-limb form: the only instantiations that read them)
static int pack_x3(ddk_ctx* ctx, ConvLayerDev& L, int NG, const std::vector<float>& w1all, const std::vector<float>& w2all,
                   const std::vector<float>& b2all, bool sender_k48 = false) {
  const size_t w2sz = (size_t)L.n_tiles * FRAG_FLOATS, b2sz = (size_t)L.n_tiles * 32;
  struct Form { int limbs, tile_bytes, bias_off, desc_off, w1_tile_bytes; };
  const Form F = ctx->cfg.conv_kernel == 3 ? Form{3, W2X_TILE_BYTES, W2X_BIAS_OFF, W2X_DESC_OFF, W1X_TILE_BYTES}
                                           : Form{2, W2X2_TILE_BYTES, W2X2_BIAS_OFF, W2X2_DESC_OFF, W1X2_TILE_BYTES};
  bool exact = true;
  // exact power-of-two range scaling: max|w| of a group is brought into [2^14, 2^15) so that no limb leaves the fp16 range whatever the
  // scale of the checkpoint (the kernel scales the activations per edge the same way)
  auto range_scale = [](const float* v, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(v[i]));
    int e = 0;
    std::frexp(std::max(m, 0x1p-40f), &e);      // m = f * 2^e, f in [0.5, 1)
    return std::ldexp(1.0f, 15 - e);
  };
  // (+ three zero records behind the last group: the kernel requests record t+3 without clamping at a group's last tile)
  std::vector<uint8_t> w2x((size_t)(NG * L.n_tiles + 4) * F.tile_bytes, 0), w1x((size_t)NG * 3 * F.w1_tile_bytes, 0), w1sx(F.limbs == 2 && sender_k48 ? (size_t)NG * W1L_BYTES : 0, 0);
  // tile t of the fp32 fragments src [.][9][64][4] -> the form's limbs x [4 x [64][8] | [64][4]]
  auto frags = [&](const float* src, int t, float sc, uint8_t* dst) {
    for (int r = 0; r < 36; ++r)
      for (int lane = 0; lane < 64; ++lane) {
        const int s_ = r / 8, i = r % 8;
        const size_t off = s_ < 4 ? (size_t)s_ * 1024 + lane * 16 + 2 * i : (size_t)4096 + lane * 8 + 2 * i;
        exact &= store_limbs(src[frag_index(t, r, lane)] * sc, F.limbs, dst + off, W2X_LIMB_BYTES);
      }
  };
  for (int g = 0; g < NG; ++g) {
    const float* w2 = w2all.data() + g * w2sz;
    const float* w1 = w1all.data() + g * W1_FLOATS;
    const float* b2 = b2all.data() + g * b2sz;
    const float sc1 = range_scale(w1, W1_FLOATS), sc2 = range_scale(w2, w2sz);
    L.w1s[g] = sc1; L.w2s[g] = sc2;
    for (int t = 0; t < L.n_tiles; ++t) {
      uint8_t* rec = w2x.data() + ((size_t)g * L.n_tiles + t) * F.tile_bytes;
      frags(w2, t, sc2, rec);
      memcpy(rec + F.bias_off, b2 + (size_t)t * 32, 128);       // fp32 as is: the kernel scales it like the products
      const int32_t dq[2] = {x_tile_word(L.h_tiles[t].w0), L.h_tiles[t].chan0};
      if (dq[0] < 0) return fail(ctx, DDK_ERR_INVALID, "internal: a vector tile of the conv layout does not sit on a T1O / T1E row quad");
      memcpy(rec + F.desc_off, dq, 8);
    }
    for (int T = 0; T < 3; ++T) frags(w1, T, sc1, w1x.data() + ((size_t)g * 3 + T) * F.w1_tile_bytes);
    // two-limb form: the K = 48 fragments of the node-term split (W1L_BYTES, ddk_internal.h): the edge_emb and x_dst columns of the K = 72 fragments as
    // three full K steps, under the group's range scale and the same window
    if (!w1sx.empty())
      for (int T = 0; T < 3; ++T)
        for (int r = 0; r < 24; ++r)
          for (int lane = 0; lane < 64; ++lane) {
            uint8_t* dst = w1sx.data() + (size_t)g * W1L_BYTES + (size_t)T * 2 * W1L_LIMB_BYTES + (size_t)(r / 8) * 1024 + lane * 16 + 2 * (r % 8);
            exact &= store_limbs(w1[frag_index(T, w1s_k72_register(r), lane)] * sc1, 2, dst, W1L_LIMB_BYTES);
          }
  }
  if (!exact)
    return fail(ctx, DDK_ERR_INVALID, F.limbs == 3 ? "internal: the three-limb fp16 split of a conv weight is not exact"
                                                   : "internal: the two-limb fp16 split of a conv weight leaves its 2^-22 window");
  L.h_w2x = w2x; L.h_w1x = w1x; L.h_w1sx = w1sx;
  L.sender_in_gemm1 = !w1sx.empty();      // the layer's split launches multiply the sender's columns themselves: its contexts form the receiver roles only
  L.epi_ok = conv_epilogue_shapes_ok(L.h_tiles);      // conv_select (conv_launch.hip) refuses the asm-epilogue instantiation otherwise
  L.limbs = F.limbs;      // 2: the default two-limb form, three products (k_conv_x2.hip); 3 (conv_kernel = 3): all three limbs, six products
  if (ctx->host_only) return DDK_OK;
  L.w2x = (uint8_t*)dev_alloc(ctx, w2x.size());
  L.w1x = (uint8_t*)dev_alloc(ctx, w1x.size());
  if (!w1sx.empty()) L.w1sx = (uint8_t*)dev_alloc(ctx, w1sx.size());
  if (!L.w2x || !L.w1x || (!w1sx.empty() && !L.w1sx)) return fail(ctx, DDK_ERR_NOMEM, "device allocation failed while packing conv weights (f16 limbs)");
  if (!w1sx.empty() && hipMemcpy(L.w1sx, w1sx.data(), w1sx.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, DDK_ERR_HIP, "f16-limb weight upload failed");
  if (hipMemcpy(L.w2x, w2x.data(), w2x.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(L.w1x, w1x.data(), w1x.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ctx, DDK_ERR_HIP, "f16-limb weight upload failed");
  return DDK_OK;
}

// mode 0: score-model layer l = conv_layers.{l} with 4 edge groups (fc.{g}.{0,4}) and one BatchNorm;
// mode 1: confidence-model layer l = the 9 convs conv_layers.{9l+g} (fc.{0,3}), each with its own BatchNorm.
int build_conv_layer(ddk_ctx* ctx, int mode, int l, ConvLayerDev& L) {
  const ddk_config& c = ctx->cfg;
  std::vector<int> rowmap;
  std::vector<float> rowscale;
  std::vector<TileDesc> tiles;
  int rc = build_layout(ctx, mode, l, L, rowmap, rowscale, tiles);
  if (rc) return rc;
  const int NG = mode == 0 ? 4 : 9;
  L.n_groups = NG;
  auto fc_name = [&](int g) { return mode == 0 ? "conv_layers." + std::to_string(l) + ".fc." + std::to_string(g) : "conv_layers." + std::to_string(9 * l + g) + ".fc"; };
  const std::string lin2 = mode == 0 ? ".4" : ".3";
  if (ctx->weights.find(fc_name(0) + ".0.weight") == ctx->weights.end()) {
    L.has_weights = false;     // shape-only layer: ddk_tp_forward works, ddk_conv_forward refuses
    return DDK_OK;
  }
  L.has_weights = true;
  const size_t w2sz = (size_t)L.n_tiles * FRAG_FLOATS, b2sz = (size_t)L.n_tiles * 32;
  std::vector<float> w1all(NG * W1_FLOATS, 0.f), b1all(NG * B1_FLOATS, 0.f), w2all(NG * w2sz, 0.f), b2all(NG * b2sz, 0.f);
  std::vector<const HostTensor*> W1(NG), B1(NG), W2(NG), B2(NG);
  for (int g = 0; g < NG; ++g) {
    const std::string f = fc_name(g);
    W1[g] = find_w(ctx, f + ".0.weight", {NE, NE});
    B1[g] = find_w(ctx, f + ".0.bias", {NE});
    W2[g] = find_w(ctx, f + lin2 + ".weight", {L.W, NE});
    B2[g] = find_w(ctx, f + lin2 + ".bias", {L.W});
    if (!W1[g] || !B1[g] || !W2[g] || !B2[g]) return DDK_ERR_INVALID;
    fill_gemm1(*W1[g], *B1[g], NE, w1all.data() + g * W1_FLOATS, b1all.data() + g * B1_FLOATS);
    fill_gemm2(*W2[g], *B2[g], NE, rowmap, rowscale, L.n_tiles, w2all.data() + g * w2sz, b2all.data() + g * b2sz);
  }
  // node terms of GEMM1 (score model): see ConvLayerDev::wn
  if (mode == 0) {
    L.h_wn.assign((size_t)2 * 4 * NE * NS, 0.f);
    L.h_bnp.assign((size_t)2 * 4 * NE, 0.f);
    const int recv_g[2][2] = {{0, 1}, {2, 3}}, send_g[2][2] = {{0, 3}, {1, 2}};     // [node type][slot]: ligand atom / residue
    for (int type = 0; type < 2; ++type)
      for (int slot = 0; slot < 4; ++slot) {
        const int g = slot < 2 ? recv_g[type][slot] : send_g[type][slot - 2];
        const int col0 = slot < 2 ? NS : 2 * NS;       // x[edge_src][:ns] columns (receiver) / x[edge_dst][:ns] columns (sender)
        for (int o = 0; o < NE; ++o) {
          const size_t row = ((size_t)(type * 4 + slot) * NE + pre_pos(o));
          for (int k = 0; k < NS; ++k) L.h_wn[row * NS + k] = W1[g]->data[(size_t)o * NE + col0 + k];
          L.h_bnp[row] = slot < 2 ? B1[g]->data[o] : 0.f;       // the bias rides with the receiver's term
        }
      }
  }
  // BatchNorm (e3nn, eval): per multiplicity channel; one per layer (mode 0) or one per conv (mode 1)
  const int n_bn = mode == 0 ? 1 : NG;
  L.h_bn_mean.assign((size_t)n_bn * XW, 0.f);
  L.h_bn_scale.assign((size_t)n_bn * XW, 1.f);
  L.h_bn_bias.assign((size_t)n_bn * XW, 0.f);
  if (c.batch_norm)
    for (int g = 0; g < n_bn; ++g) {
      const std::string pre = "conv_layers." + std::to_string(mode == 0 ? l : 9 * l + g) + ".batch_norm";
      if ((rc = fold_batch_norm(ctx, pre, L.out_mul, L.h_bn_mean.data() + (size_t)g * XW, L.h_bn_scale.data() + (size_t)g * XW,
                                L.h_bn_bias.data() + (size_t)g * XW)))
        return rc;
    }
  L.h_w1p.resize(NG); L.h_b1p.resize(NG); L.h_w2p.resize(NG); L.h_b2p.resize(NG);
  for (int g = 0; g < NG; ++g) {
    L.h_w1p[g].assign(w1all.begin() + g * W1_FLOATS, w1all.begin() + (g + 1) * W1_FLOATS);
    L.h_b1p[g].assign(b1all.begin() + g * B1_FLOATS, b1all.begin() + (g + 1) * B1_FLOATS);
    L.h_w2p[g].assign(w2all.begin() + g * w2sz, w2all.begin() + (g + 1) * w2sz);
    L.h_b2p[g].assign(b2all.begin() + g * b2sz, b2all.begin() + (g + 1) * b2sz);
  }
  if (mode == 0 && c.conv_kernel != 1 && (rc = pack_x3(ctx, L, NG, w1all, w2all, b2all, true))) return rc;
  if (mode == 1 && c.conv_kernel != 1) {      // the limb records take GEMM2 under the moved T2E rows; the fp32 fragments above keep the table's
    std::vector<int> rmx;
    std::vector<float> rsx;
    if ((rc = t2e_row_remap(ctx, tiles, rowmap, rowscale, rmx, rsx))) return rc;
    std::vector<float> w2x_all(NG * w2sz, 0.f), b2x_all(NG * b2sz, 0.f);
    for (int g = 0; g < NG; ++g) fill_gemm2(*W2[g], *B2[g], NE, rmx, rsx, L.n_tiles, w2x_all.data() + g * w2sz, b2x_all.data() + g * b2sz);
    if ((rc = pack_x3(ctx, L, NG, w1all, w2x_all, b2x_all))) return rc;
  }
  if (!ctx->host_only) {
    float* d1 = dev_upload(ctx, w1all);
    float* db1 = dev_upload(ctx, b1all);
    float* d2 = dev_upload(ctx, fp32_records(w2all, b2all, tiles, NG));
    if (mode == 0) { L.wn = dev_upload(ctx, L.h_wn); L.bnp = dev_upload(ctx, L.h_bnp); if (!L.wn || !L.bnp) return fail(ctx, DDK_ERR_NOMEM, "device allocation failed while packing conv weights"); }
    L.bn_mean = dev_upload(ctx, L.h_bn_mean);
    L.bn_scale = dev_upload(ctx, L.h_bn_scale);
    L.bn_bias = dev_upload(ctx, L.h_bn_bias);
    if (!d1 || !db1 || !d2 || !L.bn_mean || !L.bn_scale || !L.bn_bias)
      return fail(ctx, DDK_ERR_NOMEM, "device allocation failed while packing conv weights");
    for (int g = 0; g < 4; ++g) {      // group-major contiguous: group g at + g * stride
      L.w1p[g] = d1 + g * W1_FLOATS;
      L.b1p[g] = db1 + g * B1_FLOATS;
      L.w2r[g] = d2 + (size_t)g * L.n_tiles * W2_TILE_FLOATS;
    }
  }
  return DDK_OK;
}

// tor_bond_conv (mode 2, radial MLP 72 -> 72 -> 288) and final_conv (mode 3, 48 -> 48 -> 144, zero padded to the kernel's 72-wide GEMMs)
// packed like one edge group of a conv layer: the heads run through conv_fused_kernel<GATHER = false> on explicit edge attributes
int build_head_layer(ddk_ctx* ctx, int mode, ConvLayerDev& L) {
  std::vector<int> rowmap;
  std::vector<float> rowscale;
  std::vector<TileDesc> tiles;
  int rc = build_layout(ctx, mode, 3, L, rowmap, rowscale, tiles);
  if (rc) return rc;
  L.n_groups = 1;
  const std::string pre = mode == 2 ? "tor_bond_conv.fc" : "final_conv.fc";
  const int kin = mode == 2 ? NE : 2 * NS;          // true width of the MLP's input and hidden layer
  const HostTensor* W1 = find_w(ctx, pre + ".0.weight", {kin, kin});
  const HostTensor* B1 = find_w(ctx, pre + ".0.bias", {kin});
  const HostTensor* W2 = find_w(ctx, pre + ".4.weight", {L.W, kin});
  const HostTensor* B2 = find_w(ctx, pre + ".4.bias", {L.W});
  if (!W1 || !B1 || !W2 || !B2) return DDK_ERR_INVALID;
  L.has_weights = true;
  std::vector<float> w1(W1_FLOATS, 0.f), b1(B1_FLOATS, 0.f), w2((size_t)L.n_tiles * FRAG_FLOATS, 0.f), b2((size_t)L.n_tiles * 32, 0.f);
  fill_gemm1(*W1, *B1, kin, w1.data(), b1.data());
  fill_gemm2(*W2, *B2, kin, rowmap, rowscale, L.n_tiles, w2.data(), b2.data());
  L.h_w1p.assign(1, w1); L.h_b1p.assign(1, b1); L.h_w2p.assign(1, w2); L.h_b2p.assign(1, b2);
  L.h_bn_mean.assign(XW, 0.f); L.h_bn_scale.assign(XW, 1.f); L.h_bn_bias.assign(XW, 0.f);
  if (ctx->cfg.conv_kernel != 1 && (rc = pack_x3(ctx, L, 1, w1, w2, b2))) return rc;
  if (ctx->host_only) return DDK_OK;
  L.w1p[0] = dev_upload(ctx, w1); L.b1p[0] = dev_upload(ctx, b1); L.w2r[0] = dev_upload(ctx, fp32_records(w2, b2, tiles, 1));
  if (!L.w1p[0] || !L.b1p[0] || !L.w2r[0]) return fail(ctx, DDK_ERR_NOMEM, "device allocation failed while packing the head weights");
  return DDK_OK;
}

}  // namespace ddk
