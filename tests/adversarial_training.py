"""Adversarial operands, per-element scales and bars for the training ops built on the tensor-product kernels (k_tp.hip, k_tp_bwd.hip, k_rtp.hip: the tensor
product, the radial tensor product, the radial conv; k_reduce.hip: the slice reduction and the segmented sum).  Plain helper module (no fixtures): shared
by tests/test_adversarial_training_host.py (CPU) and tests/test_gpu_training_adversarial.py.  Nothing here is a number measured on a kernel.

THE FORMS.  `forward`, `backward`, `rtp_forward`, `rtp_backward`, `rconv_forward`, `rconv_backward` restate tests/tp_backward_ref.py, radial_tp_ref.py and
radial_conv_ref.py for a shape dict (so that they serve the nv = 4 family, whose fp64 text is autograd of the oracle, tests/latent_encoder_ref.py) under an
arithmetic `Mode`: fp64 (the reference; the host test holds it to the three closed forms and to the oracle), fp32 in two summation orders (the reference
evaluations the bar is tried on) and ABSOLUTE: the same multilinear forms on |operands|, every coefficient positive and both products of a cross-product
component added.  The absolute form of an output element is S, the sum of the absolute values of all terms of its full expansion.

THE BAR.  For every element of every output, none exempt,     |device - fp64| <= n u (1 + 2^-10) S,     u = 2^-24,
n = the number of fp32 roundings on the longest path from the operands to the element, counted from the documented structure of the kernels (`counts`;
the first-order a-priori bound: it holds for any summation order, fused or not; n u < 2^-10 here, which the factor covers).  An element with S == 0 must be
an exact zero.  The counts, term by term (R_k rows and O_k <= 24 columns of weight block k, W weights, n_g edges in group g, deg the node's edge count):
    DOT  = 73   w_e[p] = sum_k W2[p, k] h[k] + b2[p]: the K = 72 dot plus the bias (0 for the tensor product, whose w is an operand)
    UROW =  5   a row of U, on its longest path: (p . v) / sqrt3 is a product, two adds, the constant's own rounding and the product with it
    RS   =  3   rs_k = 1 / sqrtf(R_k): the root, the division, the product with the row
    out          DOT + UROW + RS + 1 (the product with the accumulator) + R_k + 1 (the adds over a half-wave's rows and the add of the two halves)
                 = DOT + 10 + R_k;   out_nodes: + deg + 1 (the node's adds and the one division)
    grad_w       UROW + RS + 1 (product with g) + 2 (a vector column's two adds) + 1 spare = 12  (the tensor product's per-edge weight gradient: gw_e)
    G row        DOT + O_k (<= 24: one product, O_k - 1 adds over the columns) + RS + 1 spare = DOT + 28
    grad_x       G row + 8 (the fold: a cross product's two products, subtraction, constant and its rounding; up to three adds into the edge's image)
                 = DOT + 36;   grad_x_nodes: + 1 (g = grad_out / count) + deg
    grad_sh      G row + 4 (the product or cross product with x) + 3 sum_k R_k (the adds over every row, three components) + 8 (the add of the halves / the
                 wave's butterfly) = DOT + 40 + 3 sum_k R_k;   conv: + 1
    grad_h       12 (gw_e) + 1 (product) + W (terms)                      conv: + 1
    grad_w2[g]   12 (gw_e) + 1 (product with h) + n_g (the edges of the group) + ceil(n_g / 512) + 1 (its slices)      conv: + 1
    grad_b2[g]   as grad_w2 (the product with 1 is exact; counted all the same)

THE OPERAND CLASSES (`operands`).  Every nonzero magnitude lies in [2^-24, 2^4] (a Gaussian clipped to [2^-4, 4] times at most ONE power of two 2^-k,
k <= 20, per operand); a term is a product of at most five operands, so that nothing underflows or overflows in fp32: asserted in fp64 by the generator,
with the class's own claims.  CLASSES below; `zero_blocks` has the two variants 'x' and 'g'.

THE FIGURES of the reference evaluations (tests/test_adversarial_training_host.py prints them; the largest err / (u S) over all classes, tables, graphs and
the eight shapes, fp32 numpy in two summation orders; they are numbers of the reference evaluation, not of the kernel):
    tp:     out 9.1    grad_x 6.2    grad_sh 4.2    grad_w 4.7
    rtp:    out 9.0    grad_x 5.0    grad_sh 2.1    grad_h 7.5    grad_w2 10.2   grad_b2 7.9
    rconv:  out_nodes 2.4    grad_x_nodes 2.8    grad_sh 1.9    grad_h 6.7    grad_w2 10.7   grad_b2 9.2
and of the four mutants of that evaluation on 200 edges, shapes 0 and 3, as err / bar on the class built for them (each must exceed 1):
    a dropped slot in the smallest column (column_spread, out)          7.1e3, 4.6e3      (helpers.rel_err of its block: 1.2e-7, 3.7e-7: a pass at 1e-5)
    h rounded to fp16 (channel_spread, out)                             3.4e1, 3.0e1
    one edge left out of a group's grad_w2 (edge_spread)                2.0e5, 2.0e5
    a node's last row left out of its sum (degrees, out_nodes)          1.3e2, 1.9e2
"""
import numpy as np

import latent_encoder_ref as ler
import tp_backward_ref as tpr

U = 2.0 ** -24
SLACK = 1 + 2.0 ** -10
HIDDEN = 72
NV4 = 8                                       # DDK_TP_NV4: the ids of the second shape family
SHAPES = (0, 1, 2, 3, NV4, NV4 + 1, NV4 + 2, NV4 + 3)      # layer 4 shares shape 3
LO, HI = 2.0 ** -24, 2.0 ** 4
CLASSES = ('column_spread', 'channel_spread', 'edge_spread', 'relu_sparse', 'degenerate_sh', 'cancelling', 'zero_blocks')
TP_CLASSES = ('column_spread', 'channel_spread', 'edge_spread', 'degenerate_sh', 'cancelling', 'zero_blocks')      # (no h: relu_sparse does not apply)
CLASS_TABLE = [0, 1, 1, 34, 70]               # a one-edge group, an empty group, boundaries off the tile grid
GROUP_TABLES = ([0, 64], [0, 128, 256, 257, 384], [0, 512, 512, 1025, 1536], [0, 0, 0, 97], [0, 96, 96, 96, 96])
DOT, UROW, RS = 73, 5, 3


def shape(l):
    """the sizes of shape id l (tests/tp_backward_ref.py: shape): nv = 6 layers 0..3, nv = 4 layers NV4 + 0..3"""
    return tpr.shape(l) if l < NV4 else ler.shape(l - NV4, 4)


def out_offsets(s):
    O = s['O']
    return [0, O[0], O[0] + 3 * O[1], O[0] + 3 * O[1] + 3 * O[2], s['dout']]


def out_block_of_column(s):
    """[dout] the weight block that feeds each column of an out row"""
    o = out_offsets(s)
    return np.concatenate([np.full(o[k + 1] - o[k], k) for k in range(4)]).astype(np.int64)


def slot_index(s):
    """(block, row, column) [W] of every weight slot p = B_k + r O_k + c"""
    blk, row, col = (np.zeros(s['W'], np.int64) for _ in range(3))
    for k in range(4):
        n = s['R'][k] * s['O'][k]
        if n:
            r, c = np.divmod(np.arange(n), s['O'][k])
            blk[s['B'][k]:s['B'][k + 1]], row[s['B'][k]:s['B'][k + 1]], col[s['B'][k]:s['B'][k + 1]] = k, r, c
    return blk, row, col


def row_source(s, k, r):
    """the input irrep ('a', 'p', 'q', 'c') that makes row r of block k"""
    A, P, Q = s['A'], s['P'], s['Q']
    if k == 0:
        return 'a' if r < A else 'p'
    if k == 1:
        return 'a' if r < A else ('p' if r < A + P else 'q')
    if k == 2:
        return 'p' if r < P else ('q' if r < P + Q else 'c')
    return 'q' if r < Q else 'c'


def x_slices(s):
    A, P, Q = s['A'], s['P'], s['Q']
    return {'a': slice(0, A), 'p': slice(A, A + 3 * P), 'q': slice(A + 3 * P, A + 3 * P + 3 * Q), 'c': slice(A + 3 * P + 3 * Q, s['din'])}


# ------------------------------------------------------------------------------------------------------------------------------------
# the forms under an arithmetic mode
# ------------------------------------------------------------------------------------------------------------------------------------
class Mode:
    """How the forms are evaluated: `dt` float64 or float32; `absolute`: on |operands| with every subtraction an addition (S); `rev`: sums run sequentially
    from the last term to the first, one rounding per add (otherwise numpy's own order: pairwise sums, BLAS products)."""

    def __init__(self, dt=np.float64, absolute=False, rev=False):
        self.dt, self.absolute, self.rev = dt, absolute, rev

    def c(self, a):
        a = np.asarray(a, self.dt)
        return np.abs(a) if self.absolute else a

    def k(self, v):
        return self.dt(v)

    def sub(self, a, b):
        return a + b if self.absolute else a - b

    def sum(self, t, axis):
        if not self.rev or t.shape[axis] == 0:
            return t.sum(axis, dtype=self.dt)
        t = np.moveaxis(t, axis, 0)
        acc = t[-1].copy()
        for i in range(t.shape[0] - 2, -1, -1):
            acc = acc + t[i]
        return acc

    def mm(self, a, b):
        """a [n, K] @ b [K, m]"""
        if not self.rev or a.shape[1] == 0:
            return a @ b
        K = a.shape[1]
        acc = np.zeros((a.shape[0], b.shape[1]), self.dt)
        if K <= 128:
            for k in range(K - 1, -1, -1):
                acc = acc + a[:, k, None] * b[None, k, :]
        else:      # pieces of 32 by the product routine, added from the last piece to the first
            for k in range(32 * ((K - 1) // 32), -1, -32):
                acc = acc + a[:, k:k + 32] @ b[k:k + 32]
        return acc


FP64, ABS = Mode(), Mode(absolute=True)
FP32_ORDERS = (Mode(np.float32), Mode(np.float32, rev=True))


def _cross(m, t, v):
    t, v = np.broadcast_arrays(t, v)
    return np.stack([m.sub(t[..., 1] * v[..., 2], t[..., 2] * v[..., 1]), m.sub(t[..., 2] * v[..., 0], t[..., 0] * v[..., 2]),
                     m.sub(t[..., 0] * v[..., 1], t[..., 1] * v[..., 0])], -1)


def _split(m, s, x, sh, g):
    A, P, Q, O = s['A'], s['P'], s['Q'], s['O']
    x, sh = m.c(x), m.c(sh)
    E = x.shape[0]
    a, p = x[:, :A], x[:, A:A + 3 * P].reshape(E, P, 3)
    q, c = x[:, A + 3 * P:A + 3 * P + 3 * Q].reshape(E, Q, 3), x[:, A + 3 * P + 3 * Q:]
    gs = None
    if g is not None:
        g, o = m.c(g), out_offsets(s)
        gs = [g[:, :o[1]], g[:, o[1]:o[2]].reshape(E, O[1], 3), g[:, o[2]:o[3]].reshape(E, O[2], 3), g[:, o[3]:]]
    return a, p, q, c, sh[:, 0], sh[:, 1:4], gs


def _rows(m, a, p, q, c, s0, v):
    vv, ss = v[:, None, :], s0[:, None, None]
    k2, k3 = m.k(1 / np.sqrt(2.0)), m.k(1 / np.sqrt(3.0))
    U0 = np.concatenate([a * s0[:, None], m.sum(p * vv, -1) * k3], 1)
    U1 = np.concatenate([a[:, :, None] * vv, p * ss, _cross(m, q, vv) * k2], 1)
    U2 = np.concatenate([_cross(m, p, vv) * k2, q * ss, c[:, :, None] * vv], 1)
    U3 = np.concatenate([m.sum(q * vv, -1) * k3, c * s0[:, None]], 1)
    return U0, U1, U2, U3


def forward(m, s, x, sh, w):
    """out [E, Dout] of the tensor product (tests/tp_backward_ref.py: forward) under mode m"""
    a, p, q, c, s0, v, _ = _split(m, s, x, sh, None)
    w = m.c(w)
    Us, E, out = _rows(m, a, p, q, c, s0, v), a.shape[0], []
    for k in range(4):
        R, O = s['R'][k], s['O'][k]
        if R * O == 0:
            continue
        Wk = w[:, s['B'][k]:s['B'][k + 1]].reshape(E, R, O)
        Uk = Us[k] * m.k(1 / np.sqrt(R))
        out.append(m.sum(Uk[:, :, None] * Wk, 1) if k in (0, 3) else m.sum(Uk[:, :, None, :] * Wk[:, :, :, None], 1).reshape(E, -1))
    return np.concatenate(out, 1)


def backward(m, s, x, sh, w, grad_out):
    """(grad_x, grad_sh, grad_w, G) under mode m; G: the four blocks' rows, for the claims of `zero_blocks`.  w None: grad_w alone is meaningful"""
    a, p, q, c, s0, v, gs = _split(m, s, x, sh, grad_out)
    A, P, Q, C = s['A'], s['P'], s['Q'], s['C']
    E = a.shape[0]
    w = np.zeros((E, s['W']), m.dt) if w is None else m.c(w)
    Us = _rows(m, a, p, q, c, s0, v)
    grad_w = np.zeros((E, s['W']), m.dt)
    G = [np.zeros((E, A + P), m.dt), np.zeros((E, A + P + Q, 3), m.dt), np.zeros((E, P + Q + C, 3), m.dt), np.zeros((E, Q + C), m.dt)]
    for k in range(4):
        R, O = s['R'][k], s['O'][k]
        if R * O == 0:
            continue
        rs = m.k(1 / np.sqrt(R))
        Wk = w[:, s['B'][k]:s['B'][k + 1]].reshape(E, R, O)
        Uk = Us[k] * rs
        if k in (0, 3):
            grad_w[:, s['B'][k]:s['B'][k + 1]] = (Uk[:, :, None] * gs[k][:, None, :]).reshape(E, -1)
            G[k] = m.sum(Wk * gs[k][:, None, :], 2) * rs
        else:
            grad_w[:, s['B'][k]:s['B'][k + 1]] = m.sum(Uk[:, :, None, :] * gs[k][:, None, :, :], 3).reshape(E, -1)
            G[k] = m.sum(Wk[:, :, :, None] * gs[k][:, None, :, :], 2) * rs
    G0, G1, G2, G3 = G
    vv, ss = v[:, None, :], s0[:, None, None]
    k2, k3 = m.k(1 / np.sqrt(2.0)), m.k(1 / np.sqrt(3.0))
    grad_a = s0[:, None] * G0[:, :A] + m.sum(vv * G1[:, :A], -1)
    grad_p = vv * G0[:, A:A + P, None] * k3 + ss * G1[:, A:A + P] + _cross(m, vv, G2[:, :P]) * k2
    grad_q = _cross(m, vv, G1[:, A + P:A + P + Q]) * k2 + ss * G2[:, P:P + Q] + vv * G3[:, :Q, None] * k3
    grad_c = m.sum(vv * G2[:, P + Q:P + Q + C], -1) + s0[:, None] * G3[:, Q:Q + C]
    grad_x = np.concatenate([grad_a, grad_p.reshape(E, -1), grad_q.reshape(E, -1), grad_c], 1)
    grad_s0 = m.sum(a * G0[:, :A], 1) + m.sum((p * G1[:, A:A + P]).reshape(E, -1), 1) + m.sum((q * G2[:, P:P + Q]).reshape(E, -1), 1) + m.sum(c * G3[:, Q:Q + C], 1)
    grad_v = (m.sum(a[:, :, None] * G1[:, :A], 1) + m.sum(p * G0[:, A:A + P, None], 1) * k3 + m.sum(_cross(m, G2[:, :P], p), 1) * k2
              + m.sum(_cross(m, G1[:, A + P:A + P + Q], q), 1) * k2 + m.sum(q * G3[:, :Q, None], 1) * k3 + m.sum(c[:, :, None] * G2[:, P + Q:P + Q + C], 1))
    return grad_x, np.concatenate([grad_s0[:, None], grad_v], 1), grad_w, G


def weights(m, s, h, offsets, w2, b2):
    h, w2, b2 = m.c(h), m.c(w2), m.c(b2)
    w = np.zeros((h.shape[0], s['W']), m.dt)
    for g in range(len(offsets) - 1):
        sl = slice(offsets[g], offsets[g + 1])
        w[sl] = m.mm(h[sl], np.ascontiguousarray(w2[g].T)) + b2[g]
    return w


def rtp_forward(m, s, x, sh, h, offsets, w2, b2):
    return forward(m, s, x, sh, weights(m, s, h, offsets, w2, b2))      # (absolute: w is a sum of magnitudes already)


def rtp_backward(m, s, x, sh, h, offsets, w2, b2, grad_out):
    """(grad_x, grad_sh, grad_h, grad_w2, grad_b2) under mode m"""
    hm, w2m = m.c(h), m.c(w2)
    gx, gsh, gw, _ = backward(m, s, x, sh, weights(m, s, h, offsets, w2, b2), grad_out)
    gh, gw2, gb2 = np.zeros_like(hm), np.zeros_like(w2m), np.zeros(w2m.shape[:2], m.dt)
    for g in range(len(offsets) - 1):
        sl = slice(offsets[g], offsets[g + 1])
        gh[sl] = m.mm(gw[sl], w2m[g])
        gw2[g] = m.mm(np.ascontiguousarray(gw[sl].T), hm[sl])
        gb2[g] = m.sum(gw[sl], 0)
    return gx, gsh, gh, gw2, gb2


def node_counts(idx, n):
    return np.maximum(np.bincount(np.asarray(idx, np.int64), minlength=n)[:n], 1)


def _scatter(m, rows, idx, n):
    if m.dt is np.float64:
        out = np.zeros((n, rows.shape[1]))
        np.add.at(out, np.asarray(idx, np.int64), rows)
        return out
    if m.rev:      # the node's rows from the last edge to the first
        return seg_ref(rows[::-1], np.asarray(idx)[::-1], n)
    return seg_ref(rows, idx, n)


def rconv_forward(m, s, x_nodes, src, dst, n_out, sh, h, offsets, w2, b2):
    rows = rtp_forward(m, s, m.c(x_nodes)[np.asarray(dst, np.int64)], sh, h, offsets, w2, b2)
    return _scatter(m, rows, src, n_out) / node_counts(src, n_out).astype(m.dt)[:, None]


def rconv_backward(m, s, x_nodes, src, dst, n_out, sh, h, offsets, w2, b2, grad_out_nodes):
    """(grad_x_nodes, grad_sh, grad_h, grad_w2, grad_b2) under mode m"""
    xm = m.c(x_nodes)
    g = (m.c(grad_out_nodes) / node_counts(src, n_out).astype(m.dt)[:, None])[np.asarray(src, np.int64)]
    gx, gsh, gh, gw2, gb2 = rtp_backward(m, s, xm[np.asarray(dst, np.int64)], sh, h, offsets, w2, b2, g)
    return _scatter(m, gx, dst, xm.shape[0]), gsh, gh, gw2, gb2


# ------------------------------------------------------------------------------------------------------------------------------------
# the order-exact segmented sum
# ------------------------------------------------------------------------------------------------------------------------------------
def seg_ref(rows, idx, n, mean=False):
    """nodes [n, D] fp32 as the kernels promise them: node k's rows (those with idx == k) added in ascending edge id - the order of a stable argsort of the
    test's own indices - with separate fp32 adds, the first row STARTING the sum (a -0 stays -0, a node without rows is +0); mean: one fp32 division by
    max(count, 1)"""
    rows, idx = np.ascontiguousarray(rows, np.float32), np.asarray(idx, np.int64)
    order = np.argsort(idx, kind='stable')
    count = np.bincount(idx, minlength=n)[:n]
    ptr = np.concatenate([[0], np.cumsum(count)])
    out = np.zeros((n, rows.shape[1]), np.float32)
    for j in range(int(count.max()) if len(idx) else 0):
        on = np.nonzero(count > j)[0]
        r = rows[order[ptr[on] + j]]
        out[on] = r if j == 0 else (out[on] + r).astype(np.float32)
    if mean:
        out = (out / np.maximum(count, 1).astype(np.float32)[:, None]).astype(np.float32)
    return out


def node_scale(g, idx, n):
    """g / float32(max(count, 1)) per node, in fp32: the node-scale of the conv's backward"""
    return (np.asarray(g, np.float32) / np.maximum(np.bincount(np.asarray(idx, np.int64), minlength=n)[:n], 1).astype(np.float32)[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the counts of the bar
# ------------------------------------------------------------------------------------------------------------------------------------
def counts(s, op, offsets=None, src=None, dst=None, n_in=None, n_out=None):
    """{output name: n}, each broadcastable to its output (module docstring); op: 'tp', 'rtp' or 'rconv'.  From the shape, the group table and the test's
    own indices alone."""
    dot = 0 if op == 'tp' else DOT
    conv = 1 if op == 'rconv' else 0
    R = np.array(s['R'])
    n = {'out': (dot + UROW + RS + 2 + R[out_block_of_column(s)])[None, :].astype(np.float64),
         'grad_x': np.float64(dot + 36 + conv),
         'grad_sh': np.float64(dot + 40 + 3 * int(R.sum()) + conv)}
    if op == 'tp':
        n['grad_w'] = np.float64(12)
        return n
    ng = np.diff(np.asarray(offsets, np.int64))
    n['grad_h'] = np.float64(13 + s['W'] + conv)
    n['grad_w2'] = (13 + ng + (ng + 511) // 512 + 1 + conv).astype(np.float64)[:, None, None]
    n['grad_b2'] = n['grad_w2'][:, :, 0]
    if conv:
        n['out'] = n['out'] + (np.bincount(np.asarray(src, np.int64), minlength=n_out)[:n_out] + 1)[:, None]
        n['grad_x'] = n['grad_x'] + np.bincount(np.asarray(dst, np.int64), minlength=n_in)[:n_in][:, None]
    return n


def bar(n, S):
    return n * U * SLACK * S


def worst(got, ref, n, S):
    """(largest |got - ref| / bar over the elements, its index); an element whose bar is 0 must be exact (inf otherwise); a non-finite value is inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if got.size == 0:
        return 0.0, ()
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    b = np.broadcast_to(bar(n, S), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def locate(name, at, offsets=None, s=None):
    """where an element sits in the kernels' decomposition, for a failure's report: the edge's place in its group, workgroup, wave and slice; the weight
    slot's block, row, column and 32-slot tile; the out column's block"""
    if not at:
        return name
    text = f'{name}{list(at)}'
    if name in ('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w') and offsets is not None:
        e = at[0]
        g = int(np.searchsorted(np.asarray(offsets), e, side='right') - 1)
        r = e - offsets[g]
        text += f': edge {e} = group {g} + {r}: workgroup {r // 128} of its group, wave {(r % 128) // 32}, lane {r % 32}; slice {r // 512} + {r % 512}'
    if s is not None and name == 'out':
        k = int(out_block_of_column(s)[at[1]])
        c = at[1] - out_offsets(s)[k]
        text += f'; block {k}, column {c // 3 if k in (1, 2) else c}' + (f', component {c % 3}' if k in (1, 2) else '')
    if s is not None and name in ('grad_w', 'grad_w2', 'grad_b2'):
        blk, row, col = (int(v[at[1]]) for v in slot_index(s))
        text += f'; slot {at[1]} = block {blk}, row {row}, column {col} (row group {row // 4}, column group {col // 8}; fed by {row_source(s, blk, row)})'
        if name != 'grad_w':
            text += f', group {at[0]}' + (f', hidden unit {at[2]}' if name == 'grad_w2' else '')
    return text


# ------------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------------
def _base(rng, *shp, signed=True):
    """a Gaussian clipped to magnitudes in [2^-4, 4], as exact fp32 numbers"""
    z = np.clip(np.abs(rng.standard_normal(shp)), 2.0 ** -4, 4.0)
    if signed:
        z = z * rng.choice([-1.0, 1.0], size=shp)
    return z.astype(np.float32)


def _ks(rng, n, top=20):
    """n exponents that span 0..top (both ends present when n > 1), in random order"""
    return rng.permutation(np.round(np.linspace(0, top, n)).astype(np.int64)) if n > 1 else np.zeros(n, np.int64)


def _pow(k):
    return np.exp2(-np.asarray(k, np.float64)).astype(np.float32)


def column_scales(s, rng):
    """(per weight slot [W], per out column [dout], the k of every (block, column)): one 2^-k per output column of each block, a vector column's three
    components sharing it"""
    blk, _, col = slot_index(s)
    ws, gs, ks = np.ones(s['W'], np.float32), np.ones(s['dout'], np.float32), {}
    o = out_offsets(s)
    for k in range(4):
        if s['R'][k] * s['O'][k] == 0:
            continue
        kk = _ks(rng, s['O'][k])
        ks[k] = kk
        ws[blk == k] = _pow(kk)[col[blk == k]]
        gs[o[k]:o[k + 1]] = np.repeat(_pow(kk), 3 if k in (1, 2) else 1)
    return ws, gs, ks


def channel_scales(s, rng):
    """per column of an x row [din]: one 2^-k per input channel, a 3-vector sharing it"""
    A, P, Q, C = s['A'], s['P'], s['Q'], s['C']
    kk = _ks(rng, A + P + Q + C)
    return np.concatenate([_pow(kk[:A]), np.repeat(_pow(kk[A:A + P]), 3), np.repeat(_pow(kk[A + P:A + P + Q]), 3), _pow(kk[A + P + Q:])])


def _ulps(w, rng):
    """|w| moved up by one to three ulps"""
    w = np.abs(w).astype(np.float32)
    return (w.view(np.int32) + rng.integers(1, 4, size=w.shape).astype(np.int32)).view(np.float32)


def operands(cls, l, offsets, seed, variant='x', tp=False, n_in=None, n_out=None):
    """One case of class `cls` for shape id l on the group table `offsets`: dict of fp32 x, sh, g and h, w2, b2 (tp: the per-edge w instead), plus
    'claims': what the class promises (asserted here in fp64 where it is a property of the operands, by the tests where it is one of the outputs).
    n_in / n_out: x and g are node tables of the radial conv (the classes that scale per edge then scale per node)."""
    s = shape(l)
    E, G, W = int(offsets[-1]), len(offsets) - 1, s['W']
    rng = np.random.default_rng([seed, l, CLASSES.index(cls), int(variant == 'g'), int(tp)])
    nx, ng = (E if n_in is None else n_in), (E if n_out is None else n_out)
    x, sh, g = _base(rng, nx, s['din']), _base(rng, E, 4), _base(rng, ng, s['dout'])
    h = _base(rng, E, HIDDEN, signed=False) * (rng.random((E, HIDDEN)) < 0.5)      # what ReLU leaves: half of it zeros
    w2, b2 = _base(rng, G, W, HIDDEN), _base(rng, G, W)
    wt = _base(rng, E, W)
    blk, row, col = slot_index(s)
    claims = {}
    sizes = np.diff(np.asarray(offsets))
    if cls == 'column_spread':
        ws, gs, ks = column_scales(s, rng)
        w2, b2, wt, g = w2 * ws[None, :, None], b2 * ws[None, :], wt * ws[None, :], g * gs[None, :]
        c_small = int(np.argmax(ks[0]))
        claims.update(ks=ks, small_column=c_small, small_slot=int(s['B'][0] + 3 * s['O'][0] + c_small))      # row 3 of block 0's smallest column
        assert ks[0][c_small] == 20 and ks[0].min() == 0
    elif cls == 'channel_spread':
        x = x * channel_scales(s, rng)[None, :]
        h = h * _pow(_ks(rng, HIDDEN))[None, :]
    elif cls == 'edge_spread':
        assert n_in is None and n_out is None
        ke = _ks(rng, E)
        last = np.asarray(offsets[1:])[sizes > 0] - 1
        ke[last] = 1      # the last edge of every group is among the large ones: a lost tail row is visible in every element of the group's gradient
        x, h, g = x * _pow(ke)[:, None], h * _pow(ke)[:, None], g * _pow(ke)[:, None]
        claims['last_edges'] = last
    elif cls == 'relu_sparse':
        h = _base(rng, E, HIDDEN, signed=False) * (rng.random((E, HIDDEN)) < 0.15)
        dead = np.arange(2, E, 9)      # edges whose hidden row is all zero: the bias path alone
        h[dead] = 0
        full = [q for q in range(G) if sizes[q] > 1]
        zg = full[len(full) // 2] if len(full) > 1 else None      # one whole group without a hidden unit alive
        if zg is not None:
            h[offsets[zg]:offsets[zg + 1]] = 0
        claims.update(dead_edges=dead, zero_group=zg)
        assert E < 30 or 0.8 < (h == 0).mean() < 0.97
    elif cls == 'degenerate_sh':
        assert n_in is None
        sh[0::8, 1:4] = 0      # v = 0
        sh[1::8, 0] = 0      # s0 = 0
        sh[2::8, 1:3] = 0      # v along z
        sh[3::8, 2:4] = 0      # v along x
        par = np.arange(4, E, 8)      # v parallel to every input vector of the edge: each cross product cancels to exactly 0 while its S is not
        xv = x_slices(s)
        for key in ('p', 'q'):
            n = (xv[key].stop - xv[key].start) // 3
            if n:
                lam = np.exp2(rng.integers(-3, 3, size=(len(par), n))).astype(np.float32)
                x[par, xv[key]] = (lam[:, :, None] * sh[par, None, 1:4]).reshape(len(par), -1)
        claims['parallel_edges'] = par
    elif cls == 'cancelling':
        # (a) slots whose  sum_k W2[p, k] h[k] + b2[p]  cancels: hidden units in equal pairs, the slot's weights in pairs (y, -(y + 1..3 ulp)), no bias;
        # (b) an out column that cancels: block 0's column 1, whose rows r < A come in pairs with equal inputs (a_2i = a_2i+1) and weights (y, -(y + ulp)),
        #     the rows of the vector inputs without weight
        h[:, 1::2] = h[:, 0::2]
        slots = np.nonzero((col == 2) | ((blk == 1) & (col == 0)))[0]
        w2[:, slots, 1::2] = -np.sign(w2[:, slots, 0::2]) * _ulps(w2[:, slots, 0::2], rng)
        b2[:, slots] = 0
        x[:, 1:s['A']:2] = x[:, 0:s['A']:2]
        c0 = 1
        even = s['B'][0] + np.arange(0, s['A'], 2) * s['O'][0] + c0
        odd = even + s['O'][0]
        rest = s['B'][0] + np.arange(s['A'], s['R'][0]) * s['O'][0] + c0
        w2[:, odd, :] = -np.sign(w2[:, even, :]) * _ulps(w2[:, even, :], rng)
        b2[:, odd] = -np.sign(b2[:, even]) * _ulps(b2[:, even], rng)
        wt[:, odd] = -np.sign(wt[:, even]) * _ulps(wt[:, even], rng)
        w2[:, rest, :], b2[:, rest], wt[:, rest] = 0, 0, 0
        claims.update(slots=slots, out_column=c0)
    elif cls == 'zero_blocks':
        if variant == 'x':      # the last input irrep that is present
            key = [k for k in ('a', 'p', 'q', 'c') if x_slices(s)[k].stop > x_slices(s)[k].start][-1]
            x[:, x_slices(s)[key]] = 0
            zero = np.array([p for p in range(W) if row_source(s, int(blk[p]), int(row[p])) == key], np.int64)
            claims.update(zero_x=key)
        else:      # the last block of grad_out that is present
            kb = [k for k in range(4) if s['O'][k]][-1]
            o = out_offsets(s)
            g[:, o[kb]:o[kb + 1]] = 0
            zero = np.nonzero(blk == kb)[0]
            claims.update(zero_g=kb)
        claims['zero_slots'] = zero      # grad_w2[:, zero], grad_b2[:, zero] (grad_w[:, zero]) must be exactly zero
        assert len(zero)
    else:
        raise ValueError(cls)
    o = dict(x=x, sh=sh, g=g, claims=claims)
    o.update(dict(w=wt) if tp else dict(h=h, w2=w2, b2=b2))
    for key, a in o.items():
        if key == 'claims':
            continue
        assert a.dtype == np.float32
        mag = np.abs(a.astype(np.float64))
        assert np.all((mag == 0) | ((mag >= LO) & (mag <= HI))), (cls, key, mag[mag > 0].min(), mag.max())
    _assert_claims(cls, s, offsets, o, tp)
    return o


def _assert_claims(cls, s, offsets, o, tp):
    """the claims that are properties of the operands, in fp64"""
    cl = o['claims']
    if cls == 'degenerate_sh' and s['P'] + s['Q'] and len(cl['parallel_edges']):
        e = cl['parallel_edges']
        a, p, q, c, s0, v, _ = _split(FP64, s, o['x'][e], o['sh'][e], None)
        aa, pa, qa, ca, s0a, va, _ = _split(ABS, s, o['x'][e], o['sh'][e], None)
        for t, ta in ((p, pa), (q, qa)):
            if t.shape[1]:
                assert not _cross(FP64, t, v[:, None, :]).any() and _cross(ABS, ta, va[:, None, :]).max() > 0      # exactly 0 while S > 0
                assert not _cross(Mode(np.float32), t.astype(np.float32), v[:, None, :].astype(np.float32)).any()      # and in fp32, product by product
    if cls == 'cancelling':
        c0 = cl['out_column']
        if tp:
            ref, S = forward(FP64, s, o['x'], o['sh'], o['w']), forward(ABS, s, o['x'], o['sh'], o['w'])
        else:
            w, Sw = weights(FP64, s, o['h'], offsets, o['w2'], o['b2']), weights(ABS, s, o['h'], offsets, o['w2'], o['b2'])
            alive = Sw[:, cl['slots']] > 0
            assert alive.any() and np.all(np.abs(w[:, cl['slots']]) <= 2.0 ** -18 * Sw[:, cl['slots']])
            ref, S = forward(FP64, s, o['x'], o['sh'], w), forward(ABS, s, o['x'], o['sh'], Sw)
        assert (S[:, c0] > 0).all() and np.all(np.abs(ref[:, c0]) <= 2.0 ** -18 * S[:, c0])
    if cls == 'zero_blocks':
        w = o['w'] if tp else weights(FP64, s, o['h'], offsets, o['w2'], o['b2'])
        _, _, gw, G = backward(FP64, s, o['x'], o['sh'], w, o['g'])
        assert not gw[:, cl['zero_slots']].any()
        if 'zero_g' in cl:
            assert not G[cl['zero_g']].any()      # G of that block


# ------------------------------------------------------------------------------------------------------------------------------------
# graphs of the radial conv and the segmented sum
# ------------------------------------------------------------------------------------------------------------------------------------
GRAPHS = ('degrees', 'reversed', 'one_node')


def graph(name):
    """dict(src, dst, n_in, n_out, offsets) with its claims asserted.  Messages go from node dst[e] of the n_in input nodes to node src[e] of the n_out
    output nodes."""
    rng = np.random.default_rng(GRAPHS.index(name) + 40)
    if name == 'degrees':
        # src: node 0 a hub of 130 edges, nodes 1..9 one to nine edges, node 10 none.  dst: node 0 a hub of 110, nodes 1..9 one to nine, node 10 twenty, node 11 none
        n_out, n_in, offsets = 11, 12, [0, 60, 60, 120, 175]
        src = rng.permutation(np.concatenate([np.zeros(130, np.int64)] + [np.full(i, i) for i in range(1, 10)]))
        dst = rng.permutation(np.concatenate([np.zeros(110, np.int64), np.full(20, 10)] + [np.full(i, i) for i in range(1, 10)]))
        e, f = int(np.nonzero(src == 3)[0][0]), int(np.nonzero(dst == 3)[0][0])      # a self-loop away from the hub
        dst[e], dst[f] = dst[f], dst[e]
        ds, dd = np.bincount(src, minlength=n_out), np.bincount(dst, minlength=n_in)
        assert sorted(ds[1:]) == list(range(10)) and sorted(dd[1:10].tolist() + [dd[11]]) == list(range(10)) and ds[0] == 130
        assert ds[-1] == 0 and dd[-1] == 0 and (src == dst)[src != 0].any() and n_in != n_out
        pairs = src * n_in + dst
        assert len(np.unique(pairs)) < len(pairs)      # a duplicated (src, dst) pair
        hub = np.nonzero(src == 0)[0]
        assert len(np.unique(np.searchsorted(offsets, hub, side='right'))) == 3      # the hub's edges lie in three groups (each its own workgroups)
    elif name == 'reversed':
        n_out = n_in = 17
        offsets = [0, 50, 100, 150, 200]
        src = np.sort(rng.integers(0, n_out, 200))[::-1].copy()
        dst = rng.integers(0, n_in, 200)
        assert (np.diff(src) <= 0).all() and not np.array_equal(np.argsort(src, kind='stable'), np.arange(200))
    elif name == 'one_node':
        n_out = n_in = 2
        offsets = [0, 513]      # one group: the node's 513 rows cross a 512-edge slice
        src, dst = np.ones(513, np.int64), np.zeros(513, np.int64)
    else:
        raise ValueError(name)
    return dict(src=src, dst=dst, n_in=n_in, n_out=n_out, offsets=offsets)


# ------------------------------------------------------------------------------------------------------------------------------------
# one case: every output under a mode, and what the bar needs
# ------------------------------------------------------------------------------------------------------------------------------------
def evaluate(m, op, l, o, offsets=None, gr=None):
    """{output name: array} of op ('tp', 'rtp', 'rconv') on the operands o under mode m"""
    s = shape(l)
    if op == 'tp':
        gx, gsh, gw, _ = backward(m, s, o['x'], o['sh'], o['w'], o['g'])
        return dict(out=forward(m, s, o['x'], o['sh'], o['w']), grad_x=gx, grad_sh=gsh, grad_w=gw)
    if op == 'rtp':
        args = (m, s, o['x'], o['sh'], o['h'], offsets, o['w2'], o['b2'])
        return dict(zip(('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'), (rtp_forward(*args),) + tuple(rtp_backward(*args, o['g']))))
    args = (m, s, o['x'], gr['src'], gr['dst'], gr['n_out'], o['sh'], o['h'], offsets, o['w2'], o['b2'])
    return dict(zip(('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'), (rconv_forward(*args),) + tuple(rconv_backward(*args, o['g']))))


def measures(op, l, o, offsets=None, gr=None):
    """{output name: (fp64 reference, S, n)}: what `worst` takes"""
    ref, S = evaluate(FP64, op, l, o, offsets, gr), evaluate(ABS, op, l, o, offsets, gr)
    n = counts(shape(l), op, offsets, **({} if gr is None else {k: gr[k] for k in ('src', 'dst', 'n_in', 'n_out')}))
    return {k: (ref[k], S[k], n[k]) for k in ref}
