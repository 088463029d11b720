"""Adversarial operands for the radial-MLP GEMMs of the fused conv layer (Linear(72,72) -> ReLU -> Linear(72,W), models/tensor_layers.py:140-143,154-155),
layer inputs that make every single GEMM dot product visible in the layer's output, the fp64 measures the bars are stated in, and the host restatement
of the default kernel's arithmetic.  Plain helper module (no fixtures): shared by tests/test_limb_bound.py (CPU) and tests/test_gpu_conv_adversarial.py.

Notation.  u = 2^-24 (unit roundoff of fp32).  The kernel range-scales every operand of a GEMM by an exact power of two that brings the maximum of its
RANGE-SCALING GROUP into [2^14, 2^15): the group of a weight is its whole fc.<g> matrix (W1 [72,72]; W2 [W,72] AFTER the tensor product's
fl32(1/sqrt(fan-in)) was folded into its rows: the `packed` W2 below), the group of an activation is one edge's 72 values (edge_attr, then the hidden vector).

THE BARS (imported by both tests; nothing here is a number measured on the kernel).
A layer input built by `make_case` makes every output element  kappa * w'[e, c]  with ONE packed weight column
    w'[e, c] = sum_k W'_ck h_ek + b'_c,      S = sum_k |W'_ck h_ek| + |b'_c|      (W' = W2 / sqrt(fan-in), h = relu(W1 edge_attr + b1))
and |kappa| in {1, 1/sqrt2, 1/sqrt3} (the tensor-product coefficient; the mean over one edge, the identity batch norm and the zero residual follow).

(a) the fp32 contract   |kernel - fp64| <= |kappa| GAMMA S,   GAMMA = 89 u (1 + 2^-10), term by term (first order, the factor covers the cross terms):
      3 u   the packed weight fl32(W fl32(1 / fl32(sqrt n))): one rounding of the product, two in the constant
     73 u   the K = 72 dot product plus the bias (73 terms) at u per term: the classical a-priori bound n u sum |terms|, which holds for ANY summation order
            (fp32 FMA chain, MFMA chain, the limb form: tests/test_limb_bound.py shows its truncation 3 * 2^-22 = 12 u plus 14 chain roundings stay under it)
      5 u   the pass-through GEMM: in the `gemm2` arrangement W1 = 2^p I, so h = 2^p edge_attr up to the two-limb truncation 2^-22 = 4 u of edge_attr (exact in
            kernels 1 and 3); in the `gemm1` arrangement W2 selects one hidden unit with a power of two, up to the truncation 4 u of h and - when that unit is
            more than 17 binades under the edge's largest - the absolute 2^-39 max h, which is <= 1 u S wherever S >= 2^-15 max_j S_j (asserted for the classes
            bar (a) is applied to)
      6 u   the coefficient: the constant's own rounding, the product with the one-hot feature / harmonic, the fma into the row accumulator, the
            cross-product / s0 factor and the add when the column is flushed (one rounding each; the power-of-two output scale is exact), one spare
      2 u   the mean over one edge (exact) and the batch norm: the scale powf(var + eps, -1/2) of the kernel against the oracle's, and the multiply
(b) the limb floor      |kernel - fp64| <= |kappa| (GAMMA S + FLOOR),  for operands further than 17 binades under their group's maximum.  After scaling
    |x - hi - mid| <= max(2^-22 |x|, 2^-25) and the group's maximum M is >= 2^14, so the absolute term is <= 2^-39 M per operand; the three kept products
    lose  a db + b da + da db + mid.mid  <=  2^-39 (M_W |h| + M_h |W|) (1 + 2^-9) + 2^-78 M_W M_h  per term beyond the relative part already in GAMMA:
      FLOOR = C_FLOOR (M_W sum_k |h_k| + N_H M_h sum_k |W_ck|) + 72 * 2^-78 M_W M_h (+ C_FLOOR M_hid: the selected hidden unit's own split, `gemm1`)
      C_FLOOR = 2^-39 (1 + 2^-9);  N_H = 2 in `gemm2` (edge_attr is split in the pass-through GEMM and h again in GEMM2), 1 in `gemm1`.
    Kernel 3's third limb removes the relative truncation but not the absolute term (lo rounds at the same fp16 subnormal step): the same FLOOR holds for it.
(c) against the fp32 chains on the same operands, in the 3- and 14-binade classes: max and p99 of error / (|kappa| S) of the default <= RATIO_C = 1.5 x kernel 1's
    (the project's own factor, tests/test_gpu_round6.py::test_two_limb_kernel_is_fp32_grade), no additive term."""
import numpy as np
import torch

from oracle import score_model_ref as smr

K = 72
U = 2.0 ** -24
GAMMA = 89 * U * (1 + 2.0 ** -10)
C_FLOOR = 2.0 ** -39 * (1 + 2.0 ** -9)
C_CROSS = K * 2.0 ** -78
RATIO_C = 1.5
ROW_SCALE_SPREAD = 2.0 ** -15        # bar (a) in `gemm1` needs S_j >= this * max_j S_j (see GAMMA's pass-through term)
CFG = smr.ScoreModelConfig()
GROUP_SIZES = (347, 401, 339, 365)   # all four groups non-empty, none a multiple of 32, each >= the 336 (channel, harmonic) configurations of the widest layer

CLASSES = ('hi_ties', 'mid_ties', 'pow2_neighbours', 'spread3', 'spread14', 'spread30', 'mixed_signs', 'cancelling', 'small_column', 'dominant_entry')
FLOOR_CLASSES = ('spread30', 'small_column', 'dominant_entry')      # operands further than 17 binades under their group's maximum: bar (b)
RATIO_CLASSES = ('spread3', 'spread14')                              # bar (c)
SMALL_DEPTHS = (20, 24, 28)          # binades under the group's maximum (20 and 28: the issue's; 24: where a truncating mid conversion is visible above GAMMA S)


# ------------------------------------------------------------------------------------------------------------------------------------
# the operand primitives of tests/test_limb_bound.py
# ------------------------------------------------------------------------------------------------------------------------------------
def adversarial(rng, n, binades):
    """fp32 values with every mantissa bit in play, values one ulp around powers of two and around fp16 rounding boundaries (hi ties, mid ties), mixed signs,
    spread over `binades` binades below the group's maximum"""
    m = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64)
    m[::7] = (1 << 23) + rng.integers(0, 3, size=m[::7].shape)
    m[1::7] = (1 << 24) - 1 - rng.integers(0, 3, size=m[1::7].shape)
    m[2::7] = ((rng.integers(1 << 10, 1 << 11, size=m[2::7].shape) << 13) | (1 << 12)) + rng.integers(-1, 2, size=m[2::7].shape)
    m[3::7] = (rng.integers(1 << 10, 1 << 11, size=m[3::7].shape) << 13) | ((1 << 12) + (1 << 1) - 1) | (rng.integers(0, 2, size=m[3::7].shape) << 1)
    e = rng.integers(-binades, 1, size=n)
    return (rng.choice([-1.0, 1.0], size=n) * m * np.exp2(e.astype(np.float64) - 23)).astype(np.float32)


def range_scale(x, group):
    """the kernel's exact power-of-two scaling: the maximum of every group of `group` values lands in [2^14, 2^15)"""
    g = np.abs(x.astype(np.float64)).reshape(-1, group).max(axis=1)
    e = np.floor(np.log2(np.maximum(g, 2.0 ** -40)))
    return np.repeat(np.exp2(14 - e), group)


def two_limbs(xs):
    hi = xs.astype(np.float32).astype(np.float16)
    mid = (xs.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)          # (the subtraction is exact in fp32: Sterbenz-like, hi is x rounded to 11 bits)
    return hi.astype(np.float64), mid.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------
# operand classes: positive magnitudes [rows, 72] as float64 that are exact fp32 numbers, significands below 2/sqrt3 where a pattern has to survive the packing
# ------------------------------------------------------------------------------------------------------------------------------------
def _mantissas(rng, shape, kind):
    """24-bit significands in [2^23, 2^24).  `low`: any low bits under random top bits < 150/1024 (reachable through every row scale, `preimage`)."""
    top = rng.integers(0, 150, size=shape) << 13                           # significand < 1 + 150/1024 < 2/sqrt3, the smallest row scale's (fan-in 12)
    if kind == 'any':
        return rng.integers(1 << 23, 1 << 24, size=shape)
    if kind == 'low':
        return (1 << 23) | top | rng.integers(0, 1 << 13, size=shape)
    if kind == 'hi_tie':                                                   # the 13 bits under hi's 11: exactly half, one ulp under, one ulp over
        return ((1 << 23) | top | (1 << 12)) + rng.integers(-1, 2, size=shape)
    if kind == 'mid_tie':                                                  # the remainder x - hi has 12 bits and its last one set: mid (11 bits) is a tie, both directions of hi
        down = (1 << 11) | (rng.integers(0, 1 << 10, size=shape) << 1) | 1
        up = (1 << 13) - down
        return (1 << 23) | top | np.where(rng.integers(0, 2, size=shape) == 1, up, down)
    if kind == 'pow2':                                                     # one-ulp neighbours of powers of two, from above and from below
        return np.where(rng.integers(0, 2, size=shape) == 1, (1 << 23) + rng.integers(0, 3, size=shape), (1 << 24) - 1 - rng.integers(0, 3, size=shape))
    raise ValueError(kind)


def _magnitudes(rng, shape, kind, binades):
    return _mantissas(rng, shape, kind).astype(np.float64) * np.exp2(rng.integers(-binades, 1, size=shape).astype(np.float64) - 23)


def _row_signs(rng, rows):
    """a third of the rows all positive, a third all negative (products of one sign: a biased rounding adds up), a third mixed"""
    s = rng.choice([-1.0, 1.0], size=(rows, K))
    s[0::3] = 1.0
    s[1::3] = -1.0
    return s


def _small_values(rng, n, depth):
    """`depth` binades under a group maximum of exactly 2^0 (scaled: 2^14), positive, built against a truncating mid conversion: after scaling hi rounds DOWN
    and the remainder sits 2^-5 of a step under the next multiple of mid's fp16 subnormal step 2^-24, so round-to-nearest loses 2^-29 where truncation loses
    31/32 of 2^-24.  (At depth 28 the remainder is under half a step either way: both conversions give mid = 0, the error is the remainder itself.)"""
    E = 14 - depth                                                         # binade of the scaled value
    top = rng.integers(0, 150, size=n) << 13
    per = 1 << (-E - 1)                                                    # ulps of the fp32 value per 2^-24 step of the scaled value
    if per < (1 << 12):
        low = (rng.integers(0, (1 << 12) // per, size=n) + 1) * per - max(per // 32, 1)
    else:
        low = rng.integers(0, 1 << 11, size=n) | 1
    return ((1 << 23) | top | low).astype(np.float64) * 2.0 ** (-depth - 23)


def class_operands(cls, rng, rows, E, signed_act):
    """(weights [rows, 72], activations [E, 72], special rows, special edges) of one class, float64 holding exact fp32 numbers.  The weights' group is the
    whole matrix, an activation's its edge; `signed_act` False: activations >= 0 (the `gemm2` arrangement needs relu(h) = h)."""
    kind, binades = {'hi_ties': ('hi_tie', 3), 'mid_ties': ('mid_tie', 3), 'pow2_neighbours': ('pow2', 3), 'spread3': ('low', 3), 'spread14': ('low', 14),
                     'spread30': ('low', 30), 'mixed_signs': ('any', 3), 'cancelling': ('low', 3), 'small_column': ('low', 3), 'dominant_entry': ('low', 3)}[cls]
    W = _magnitudes(rng, (rows, K), kind, binades)
    A = _magnitudes(rng, (E, K), kind, binades)
    sw = rng.choice([-1.0, 1.0], size=(rows, K)) if cls == 'mixed_signs' else np.ones((rows, K)) if cls in ('hi_ties', 'mid_ties', 'pow2_neighbours') else _row_signs(rng, rows)
    sa = np.ones((E, K))
    if signed_act:
        sa = rng.choice([-1.0, 1.0], size=(E, K))
        if cls != 'mixed_signs':
            sa[0::2] = 1.0
    special_rows, special_edges = {}, {}
    if cls == 'cancelling':                                                # pairs (x, -(x + 1..3 ulp)) against equal activations: sum ~ 1e-7 of sum |.|
        ulp = np.exp2(np.floor(np.log2(W[:, 0::2])) - 23)
        W[:, 1::2] = W[:, 0::2] + ulp * rng.integers(1, 4, size=W[:, 0::2].shape)
        sw[:, 1::2] = -sw[:, 0::2]
        A[:, 1::2] = A[:, 0::2]
        sa[:, 1::2] = sa[:, 0::2]
    if cls in ('small_column', 'dominant_entry'):
        # the group's maximum is EXACTLY a power of two (scaled: 2^14, where 2^-25 IS 2^-39 of the maximum), everything else at least a binade under it
        W *= 0.25
        A *= 0.25
    if cls == 'small_column':
        W[rows // 3, 5] = 1.0
        for i, d in enumerate(SMALL_DEPTHS):
            r = (1 + i * (rows - 3) // (len(SMALL_DEPTHS) - 1)) if rows > 8 else 1 + i
            r += (r == rows // 3)
            W[r] = _small_values(rng, K, d)
            sw[r] = 1.0
            special_rows[d] = r
        sa[:] = 1.0
        A[:, 0] = 1.0                                                       # (every edge's maximum a power of two as well: the activations' own floor at its exact constant)
    if cls == 'dominant_entry':
        W[rows // 3, 5] = 1.0
        W[0::2, 0] = 0.0                                                    # (half of the rows do not see the dominant entry: their S is the small entries' alone)
        sw[:] = np.where(sw[:, :1] == 0, 1.0, sw[:, :1])                    # single-signed rows
        for i, d in enumerate(SMALL_DEPTHS):
            for e in range(3 + i, E, 7):                                    # many edges with ONE dominant entry, the 71 others `d` binades under it
                A[e] = _small_values(rng, K, d)
                A[e, 0] = 1.0
                sa[e] = 1.0
                special_edges[e] = d
    return W * sw, A * sa, special_rows, special_edges


def preimage(target, rs32):
    """fp32 x with fl32(x * rs32) == target wherever one exists (always for significands below that of every row scale, the smallest being 2/sqrt3 at fan-in 12: there the product's ulp is coarser than x's), the
    nearest x otherwise.  target: float64 array of exact fp32 numbers, rs32: float32 row scales broadcastable to it.  Returns (x float32, hit mask)."""
    t32 = target.astype(np.float32)
    rs32 = np.broadcast_to(np.asarray(rs32, np.float32), t32.shape)
    c = (target / rs32.astype(np.float64)).astype(np.float32)
    best, hit = c.copy(), (c * rs32 == t32)
    for d in (1, -1, 2, -2):
        cand = (c.view(np.int32) + d).view(np.float32)
        ok = (cand * rs32 == t32) & ~hit
        best[ok] = cand[ok]
        hit |= ok
    best[t32 == 0] = 0.0
    return best, hit | (t32 == 0)


# ------------------------------------------------------------------------------------------------------------------------------------
# layer inputs that expose single weight columns
# ------------------------------------------------------------------------------------------------------------------------------------
_LAYOUT_CACHE = {}


def layout(l):
    """For layer l: every (input channel, harmonic component) pair as one configuration; J[n, o] = (column c, coefficient) such that for a one-hot sender
    feature and a one-hot sh the tensor product's output o is  coefficient * w[c]  - read off the fp64 oracle by differentiation, and CONFIRMED by its
    linearity on random weights here (not assumed).  Returns dict(din, dout, W, rs32 [W] the packed row scale fl32(1/fl32(sqrt(fan-in))), rs64, conf_ch,
    conf_sh, col [nconf, dout] (-1: the element depends on no column), coef [nconf, dout])."""
    if l in _LAYOUT_CACHE:
        return _LAYOUT_CACHE[l]
    i_irr, o_irr = CFG.conv_irreps(l)
    din, dout, W = smr.irreps_dim(i_irr), smr.irreps_dim(o_irr), smr.faster_tp_weight_numel(i_irr, o_irr)
    conf_ch, conf_sh = np.divmod(np.arange(din * 4), 4)
    n = len(conf_ch)
    x = torch.zeros(n, din, dtype=torch.float64)
    sh = torch.zeros(n, 4, dtype=torch.float64)
    x[torch.arange(n), torch.from_numpy(conf_ch)] = 1.0
    sh[torch.arange(n), torch.from_numpy(conf_sh)] = 1.0
    w = torch.randn(n, W, dtype=torch.float64, generator=torch.Generator().manual_seed(1000 + l), requires_grad=True)
    out = smr.faster_tensor_product(x, sh, w, i_irr, o_irr)
    col = np.full((n, dout), -1, np.int64)
    coef = np.zeros((n, dout))
    Jw = torch.zeros(n, dout, dtype=torch.float64)
    for o in range(dout):
        g, = torch.autograd.grad(out[:, o].sum(), w, retain_graph=True)
        nz = g != 0
        assert int(nz.sum(1).max()) <= 1, (l, o, 'an output element depends on more than one weight column')
        has = nz.any(1).numpy()
        col[has, o] = nz.int().argmax(1).numpy()[has]
        coef[:, o] = g.sum(1).numpy()
        Jw[:, o] = (g * w.detach()).sum(1)
    assert torch.allclose(Jw, out.detach(), rtol=0, atol=1e-13), (l, 'the oracle tensor product is not coefficient x one column on these inputs')
    rs32 = np.zeros(W, np.float32)
    start = 0
    for key in ('0e', '1o', '1e', '0o'):
        n_in, n_out = smr.faster_tp_weight_shapes(i_irr, o_irr)[key]
        rs32[start:start + n_in * n_out] = np.float32(1.0) / np.sqrt(np.float32(n_in)) if n_in else 0
        start += n_in * n_out
    rs64 = np.zeros(W)
    start = 0
    for key in ('0e', '1o', '1e', '0o'):
        n_in, n_out = smr.faster_tp_weight_shapes(i_irr, o_irr)[key]
        rs64[start:start + n_in * n_out] = 1.0 / np.sqrt(n_in) if n_in else 0
        start += n_in * n_out
    # the coefficient is kappa / sqrt(fan-in) with |kappa| in {1, 1/sqrt2, 1/sqrt3}
    kap = np.abs(coef[col >= 0]) / rs64[col[col >= 0]]
    assert np.all(np.min(np.abs(kap[:, None] - np.array([1.0, 2 ** -0.5, 3 ** -0.5])[None]), axis=1) < 1e-14)
    L = dict(din=din, dout=dout, W=W, rs32=rs32, rs64=rs64, conf_ch=conf_ch, conf_sh=conf_sh, col=col, coef=coef, i_irr=i_irr, o_irr=o_irr)
    _LAYOUT_CACHE[l] = L
    return L


def make_case(l, arrangement, cls, variant, seed=0):
    """One layer input (state dict of conv layer l, nodes, edges, edge_attr, sh) of operand class `cls` in arrangement
      'gemm2': fc.<g>.0 = 2^p I, bias 0, edge_attr >= 0; fc.<g>.4.weight adversarial (chosen so that its PACKED rows carry the class's bit patterns);
               variant 0: fc.<g>.4.bias = 0, variant 1: adversarial
      'gemm1': fc.<g>.4.weight rows one-hot powers of two (column c selects hidden unit c mod 72), bias 0; fc.<g>.0 and edge_attr adversarial;
               variant 0: W1, variant 1: -W1 (ReLU hides the other half)
    and the fp64 measures of every observed element.  Everything derives from (l, arrangement, cls, variant, seed)."""
    L = layout(l)
    W, din, dout = L['W'], L['din'], L['dout']
    rng = np.random.default_rng([seed, l, CLASSES.index(cls), variant, arrangement == 'gemm1'])
    sizes = GROUP_SIZES
    splits = np.concatenate([[0], np.cumsum(sizes)])
    E = int(splits[-1])
    nconf = din * 4
    P, ea = {}, np.zeros((E, K), np.float32)
    conf = np.zeros(E, np.int64)
    meas = dict(S=np.zeros((E, dout)), floor=np.zeros((E, dout)), scale_ok=True, hits=[])
    for g in range(4):
        a, b = int(splits[g]), int(splits[g + 1])
        n = b - a
        ascale = 2.0 ** int(rng.integers(-6, 7))
        conf[a:b] = (np.arange(n) + 17 * g) % nconf                         # every configuration in every group (n >= nconf), a different phase per group
        if arrangement == 'gemm2':
            Wt, A, srows, sedges = class_operands(cls, rng, W, n, signed_act=False)
            p = int(rng.integers(-3, 4))
            W2, hit = preimage(Wt, L['rs32'][:, None])
            meas['hits'].append(float(hit.mean()))
            if cls == 'small_column':
                assert all(hit[r].all() for r in srows.values()) and hit[W // 3, 5]
            W1 = (2.0 ** p * np.eye(K)).astype(np.float32)
            b1 = np.zeros(K, np.float32)
            b2 = np.zeros(W, np.float32)
            if variant == 1:
                bt = _magnitudes(rng, (W,), 'low', 3) * rng.choice([-1.0, 1.0], size=W) * np.abs(Wt).max() * 2.0 ** p * ascale * 4.0
                b2 = preimage(bt, L['rs32'])[0]
        else:
            W1t, A, srows, sedges = class_operands(cls, rng, K, n, signed_act=True)
            W1 = (W1t if variant == 0 else -W1t).astype(np.float32)
            b1 = (_magnitudes(rng, (K,), 'low', 3) * rng.choice([-1.0, 1.0], size=K) * np.abs(W1t).max() * ascale * (0.0 if cls == 'cancelling' else 2.0)).astype(np.float32)
            b1[list(srows.values())] = 0.0                                   # (a bias of the large rows' size would hide a small row's floor under GAMMA |b|)
            if cls == 'dominant_entry':
                b1[:] = 0.0
            W2 = np.zeros((W, K), np.float32)
            W2[np.arange(W), np.arange(W) % K] = np.exp2(-(np.arange(W) % 4)).astype(np.float32)
            b2 = np.zeros(W, np.float32)
        A = A * ascale
        ea[a:b] = A.astype(np.float32)
        assert np.array_equal(ea[a:b].astype(np.float64), A)
        P[f'fc.{g}.0.weight'], P[f'fc.{g}.0.bias'] = torch.from_numpy(W1), torch.from_numpy(b1)
        P[f'fc.{g}.4.weight'], P[f'fc.{g}.4.bias'] = torch.from_numpy(W2), torch.from_numpy(b2)
        # ---- fp64 measures, in PACKED units (w' = w / sqrt(fan-in)) ----
        A64, W1_64, W2p = ea[a:b].astype(np.float64), W1.astype(np.float64), W2.astype(np.float64) * L['rs64'][:, None]
        b2p = b2.astype(np.float64) * L['rs64']
        pre = A64 @ W1_64.T + b1
        h = np.maximum(pre, 0.0)
        S1 = np.abs(A64) @ np.abs(W1_64).T + np.abs(b1)                    # [n, 72]
        c_of = L['col'][conf[a:b]]                                         # [n, dout] observed column (or -1)
        cc = np.maximum(c_of, 0)
        if arrangement == 'gemm2':
            S = np.take_along_axis(h @ np.abs(W2p).T + np.abs(b2p), cc, 1)
            M_W, M_h = np.abs(W2p).max(), h.max(1, keepdims=True)
            sumW = np.abs(W2p).sum(1)[cc]
            fl = C_FLOOR * (M_W * h.sum(1, keepdims=True) + 2 * M_h * sumW) + C_CROSS * M_W * M_h
        else:
            j, q = cc % K, np.exp2(-(cc % 4).astype(np.float64)) * L['rs64'][cc]
            M_W, M_a = np.abs(W1_64).max(), np.abs(A64).max(1, keepdims=True)
            fl1 = C_FLOOR * (M_W * np.abs(A64).sum(1, keepdims=True) + M_a * np.abs(W1_64).sum(1)[None]) + C_CROSS * M_W * M_a       # [n, 72]
            M_hid = (h + GAMMA * S1 + fl1).max(1, keepdims=True)
            S = q * np.take_along_axis(S1, j, 1)
            fl = q * (np.take_along_axis(fl1, j, 1) + C_FLOOR * M_hid)
            if cls not in FLOOR_CLASSES:
                meas['scale_ok'] &= bool((S1.min(1) >= ROW_SCALE_SPREAD * S1.max(1)).all())
        kap = np.where(c_of >= 0, np.abs(L['coef'][conf[a:b]]) / np.where(c_of >= 0, L['rs64'][cc], 1.0), 0.0)
        meas['S'][a:b] = kap * S
        meas['floor'][a:b] = kap * fl
    # identity batch norm: mean 0, weight 1, bias 0, variance 1 - eps (the scale (var + eps)^-1/2 is 1 to a rounding: in GAMMA)
    spec = {}
    smr._bn_spec(spec, 'batch_norm', L['o_irr'])
    P['batch_norm.weight'] = torch.ones(spec['batch_norm.weight'])
    P['batch_norm.bias'] = torch.zeros(spec['batch_norm.bias'])
    P['batch_norm.running_mean'] = torch.zeros(spec['batch_norm.running_mean'])
    P['batch_norm.running_var'] = torch.full(spec['batch_norm.running_var'], 1.0 - 1e-5)
    # receivers 0..E-1: all-zero features, ONE edge each; senders E..E+din-1: the one-hot rows
    node = torch.zeros(E + din, din)
    node[E:] = torch.eye(din)
    src = torch.arange(E)
    dst = E + torch.from_numpy(L['conf_ch'][conf])
    sh = torch.zeros(E, 4)
    sh[torch.arange(E), torch.from_numpy(L['conf_sh'][conf])] = 1.0
    S_all, fl_all = np.zeros((E + din, dout)), np.zeros((E + din, dout))
    S_all[:E], fl_all[:E] = meas['S'], meas['floor']
    observed = [np.unique(L['col'][conf[int(splits[g]):int(splits[g + 1])]]) for g in range(4)]
    return dict(l=l, P=P, node=node, ei=torch.stack([src, dst]), ea=torch.from_numpy(ea), sh=sh, splits=[int(v) for v in splits], S=S_all, floor=fl_all,
                conf=conf, observed=observed, scale_ok=meas['scale_ok'], hits=meas['hits'], layout=L, cls=cls, arrangement=arrangement)


def oracle_output(case):
    """the fp64 oracle's tp_conv_layer on the case, as it stands"""
    L = case['layout']
    P = {'L.' + k: v.double() for k, v in case['P'].items()}
    s = case['splits']
    return smr.tp_conv_layer(P, 'L', case['node'].double(), case['ei'], [case['ea'].double()[s[i]:s[i + 1]] for i in range(4)], case['sh'].double(),
                             L['i_irr'], '1x0e+1x1o', L['o_irr'], residual=True, batch_norm=True, faster=True, edge_groups=4).numpy()


def bound(case, kernel):
    """[N, dout] bound of |kernel - oracle| for conv_kernel `kernel` (module docstring): (a) everywhere for kernel 1, (a) outside / (b) inside
    FLOOR_CLASSES for kernels 0 and 3.  Zero where an element depends on no weight column: those must be reproduced exactly."""
    b = GAMMA * case['S']
    if kernel != 1 and case['cls'] in FLOOR_CLASSES:
        b = b + case['floor']
    return b


# ------------------------------------------------------------------------------------------------------------------------------------
# the default kernel's GEMM arithmetic on the host (k_conv_x.hip under X3_TWO_LIMBS), with the mutants the bars must catch
# ------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = (None, 'drop_hi_mid_in_one_step', 'truncate_mid', 'scale_one_binade_up')
_f32 = lambda v: v.astype(np.float32).astype(np.float64)


def _limbs(xs, mutant):
    with np.errstate(over='ignore', invalid='ignore'):
        hi = xs.astype(np.float32).astype(np.float16)
        r = xs.astype(np.float32) - hi.astype(np.float32)
        mid = r.astype(np.float16)
        if mutant == 'truncate_mid':
            m64, r64 = mid.astype(np.float64), r.astype(np.float64)
            over = np.abs(m64) > np.abs(r64)                                # rounded away from zero: step back towards it
            mid = np.where(over, np.nextafter(mid, np.float16(0)), mid)
    return hi.astype(np.float64), mid.astype(np.float64)


def _scale_of(m, mutant):
    e = np.floor(np.log2(np.maximum(m, 2.0 ** -40)))
    return np.exp2((15 if mutant == 'scale_one_binade_up' else 14) - e)


def limb_gemm(Wm, sW, X, bias, mutant=None):
    """acc[e, r] = fp32 accumulator of the kernel for row r (Wm [E, R, 72] or [R, 72], range scale sW of its matrix) against the edge's X [E, 72] (scaled per
    edge here): seeded with the bias times both scales, per K step of 16 the MFMAs hi.mid, mid.hi, hi.hi (each adds its K range exactly and rounds once), the
    packed K = 8 tail's two; returned unscaled (exact powers of two)."""
    sx = _scale_of(np.abs(X).max(1, keepdims=True), mutant)                # [E, 1]
    xh, xm = _limbs(X * sx, mutant)
    wh, wm = _limbs(Wm * sW, mutant)
    if wh.ndim == 2:
        wh, wm = wh[None], wm[None]
    xh, xm = xh[:, None, :], xm[:, None, :]
    with np.errstate(over='ignore', invalid='ignore'):
        acc = _f32(bias * (sx * sW))
        for s in range(4):
            sl = slice(16 * s, 16 * s + 16)
            for i, (A, B) in enumerate(((wh, xm), (wm, xh), (wh, xh))):
                if mutant == 'drop_hi_mid_in_one_step' and s == 2 and i == 0:
                    continue
                acc = _f32(acc + (A[..., sl] * B[..., sl]).sum(-1))
        sl = slice(64, 72)
        acc = _f32(acc + (wh[..., sl] * xm[..., sl]).sum(-1) + (wm[..., sl] * xh[..., sl]).sum(-1))
        acc = _f32(acc + (wh[..., sl] * xh[..., sl]).sum(-1) + (wm[..., sl] * xm[..., sl]).sum(-1))
        return acc / (sx * sW)


def fma_chain_gemm(Wm, X, bias):
    """an fp32 FMA chain over the same operands, one rounding per step (what conv_kernel = 1 and the reference's CPU GEMM do)"""
    if Wm.ndim == 2:
        Wm = Wm[None]
    acc = _f32(np.broadcast_to(bias, np.broadcast_shapes(np.shape(bias), (X.shape[0], Wm.shape[1]))).copy())
    for k in range(K):
        acc = _f32(acc + Wm[..., k] * X[:, None, k])
    return acc


def host_restatement(case, mutant=None, chain=False):
    """The layer's output [N, dout] as the default kernel's two GEMMs would give it (chain=True: fp32 FMA chains), everything behind the GEMMs - coefficient,
    mean, batch norm - in fp64: the restated arithmetic is the GEMMs', the rest is covered by GAMMA's other terms."""
    L = case['layout']
    s = case['splits']
    E = s[-1]
    out = np.zeros((E + L['din'], L['dout']))
    out[E:, :L['din']] = np.eye(L['din'])
    bn = (float(np.float32(1.0 - 1e-5)) + 1e-5) ** -0.5
    for g in range(4):
        a, b = s[g], s[g + 1]
        X = case['ea'][a:b].numpy().astype(np.float64)
        W1 = case['P'][f'fc.{g}.0.weight'].numpy().astype(np.float64)
        b1 = case['P'][f'fc.{g}.0.bias'].numpy().astype(np.float64)
        W2p = (case['P'][f'fc.{g}.4.weight'].numpy() * L['rs32'][:, None]).astype(np.float64)          # fl32(W rs32): the packed rows
        b2p = (case['P'][f'fc.{g}.4.bias'].numpy() * L['rs32']).astype(np.float64)
        c_of = L['col'][case['conf'][a:b]]
        cc = np.maximum(c_of, 0)
        if chain:
            h = np.maximum(fma_chain_gemm(W1, X, b1[None]), 0.0)
            w = fma_chain_gemm(W2p[cc], h, b2p[cc])
        else:
            h = np.maximum(limb_gemm(W1, _scale_of(np.abs(W1).max(), mutant), X, b1[None], mutant), 0.0)
            h = _f32(h)
            w = limb_gemm(W2p[cc], _scale_of(np.abs(W2p).max(), mutant), h, b2p[cc], mutant)
        kap = np.where(c_of >= 0, L['coef'][case['conf'][a:b]] / np.where(c_of >= 0, L['rs64'][cc], 1.0), 0.0)
        with np.errstate(invalid='ignore'):
            out[a:b] = np.where(c_of >= 0, kap * w * bn, 0.0)
    return out


def figures(out, ref, case, kernel):
    """error / (|kappa| S) over the observed elements (max, p99) and the largest error / bound (<= 1: the bar holds; inf: a non-zero where exactly zero is due)"""
    err = np.abs(np.asarray(out, np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    bd = bound(case, kernel)
    obs = case['S'] > 0
    rel = err[obs] / case['S'][obs]
    with np.errstate(divide='ignore', invalid='ignore'):
        use = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))
    return dict(max=float(rel.max()), p99=float(np.quantile(rel, 0.99)) if np.isfinite(rel).all() else float('inf'), worst_over_bound=float(use.max()),
                gamma_headroom=float(GAMMA / max(rel.max(), 1e-300)))
