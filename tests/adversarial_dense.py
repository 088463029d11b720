"""Adversarial operands, per-element scales and bars for the three dense training ops: the radial hidden layer (k_rhid.hip: ddk_rhid_*), the edge embedding
and its latent variant (k_eemb.hip: ddk_eemb_*, ddk_eemb_latent_*) and the two head convs (k_hconv.hip: ddk_hconv_*), with the slice reduction and the segmented
sum that close them (k_reduce.hip).  Plain helper module (no fixtures, no GPU import): shared by tests/test_adversarial_dense_host.py (CPU) and
tests/test_gpu_dense_adversarial.py.  It continues tests/adversarial_training.py (Mode, the bar, `worst`, seg_ref, the graphs, the operand window) and takes its
closed forms from radial_hidden_ref.py, edge_embedding_ref.py, latent_embedding_ref.py and head_conv_ref.py.  Nothing here is a number measured on a kernel.

THE BAR.  For every element of every output, none exempt,     |device - fp64| <= n u (1 + 2^-10) S,     u = 2^-24,
S the element's own sum of |terms| (the same form under ABS: every subtraction an addition, both products of a cross-product component added) and n its count of
fp32 roundings.  n is the LARGER of two counts, both read from the kernels' text and the operands' shapes: the roundings on the element's longest path through
the kernel, and the roundings of a plain left-to-right evaluation of the same sum (a sum of T terms: T - 1 adds), so that the bound holds for any summation
order, fused or not (the host test tries two).  An element with S == 0 must be an exact zero.  n u < 2^-10 throughout, which the factor covers.

THE COUNTS, term by term.  E edges, n_g edges in group g, deg the node's edge count, L = rtp_slice_len(E) = 512 here, SL(n) = n + ceil(n / L) + 1: a slice's chain
over its edges (one fmaf or one add per edge), the adds of the slice images in slice order, one spare.
  rhid (K = 72)
    h            72 (pre: the chain of 72 fmaf over k, started from the bias) + 1 (the bias: counted as tests/adversarial_training.py's DOT does) + 1 (relu * s;
                 s = fp32(1) / (fp32(1) - p) is carried into the reference as the fp32 value it is) = 74
    grad_emb     1 (gpre = grad_h * s) + 72 (the chain over c) = 73;   the two gather rows the same
    grad_xs      73 + deg_src + deg_dst (seg_ref of the src rows: deg_src - 1 adds, of the dst rows: deg_dst - 1, one add of the two)
    grad_w1[g]   1 (gpre) + SL(n_g);   grad_b1[g] the same (acc += gpre: an add per edge)
  eemb (K = F + 64 + 2 NL)
    emb          K + 1 (pre: the chain and its bias) + 1 (relu * s) + 24 + 1 (the chain over the hidden units and b2) + 1 (fmaf(unc_a, uemb, .)) = K + 28
    sh           component 0 is the constant 1: exact.  Components 1..3 are x_i * (sqrt3f / fmaxf(d, 1e-12f)): 1 (the subtraction x_i) + 3.5 (d: below) + 1 (sqrt3f's own
                 rounding) + 1 (the division) + 1 (the product) = 7.5 -> 8, at S = |sh_i| (<= sqrt3: no weaker than scale 1); x_i == 0 gives an exact 0, a zero-length
                 edge exactly [1, 0, 0, 0]
    gpre         24 (ghid: the chain over o from 0) + 1 (* s) = 25
    grad_w1      25 + SL(E);   grad_b1 the same;   grad_w2   K + 2 (hid) + SL(E);   grad_b2   SL(E);   grad_uemb   SL(E) (fmaf(unc, g, .) per edge)
    grad_lat     25 + 24 (glat: the chain over c) + deg (the node's rows)
  hconv (K = 48, W = 144 centre; K = 72, W = 288 torsion); W_ = K + 1: w_e[p] = b2[p] + the chain over k
    u, centre    5 on its longest path, a cross row: two products, the subtraction, HC_S72's own rounding, the product with it (a row a v / 6 or p s0 / 6: 3)
    u, torsion   7: three products, two adds, HC_S18's own rounding, the product with it
    out, centre  W_ + 5 + 36 (o = fmaf(u, w, o) over the tile's 36 rows) + deg + 1 (the receiver's adds and the division by its count) = K + 43 + deg
    out, torsion W_ + 7 + 6 (the block's six rows) + deg + 1 = K + 15 + deg
    grad_x, centre   1 (g = grad_out / count) + W_ + 1 (d = w g) + 5 ((vx d0 + vy d1 + vz d2) * HC_S6: a product, two adds, the constant, the product; a cross
                 column has 4) + 4 (the tiles' parts added into the image in tile order) + deg = K + 12 + deg
    grad_x, torsion  1 (g) + W_ + 24 (du: the kernel chains six columns per tile and adds four tiles = 10; a plain sum over the block's 24 columns: 24) + 2 (* HC_S18)
                 + 1 (* v) + deg = K + 29 + deg
    grad_h       9 (gw_e: u (5 / 7), g (1), the product, two adds: centre 9, torsion 9) + W (the kernel: a chain over the tile's 36 weights and NT tiles added;
                 a plain sum over the W weights: W) = 9 + W
    grad_w2      9 (gw_e) + SL(E) (fmaf(gw, h, .) over the edges of a slice);   grad_b2 the same (h = 1)

THE TWO THINGS THAT ARE NOT MULTILINEAR.
  The ReLU.  Forward it is 1-Lipschitz: h and emb are held to the bar built from the pre-activation's S.  Backward, rhid differentiates through the pattern h != 0
  of the emulator below, to which the device is held bit for bit, so nothing is exempt.  eemb's hidden layer never leaves the device: `eemb_operands` produces only
  cases in which no (edge, unit) has |pre| under the fp32 margin of edge_embedding_ref.pre_activation (latent_embedding_ref's with latents) nor under this module's
  own bar of pre: the cap is 0.  An offending unit's b1 is drawn again from the case's generator; the count of re-draws is kept in the case.
  The Gaussian columns of eemb, column_j = expf(coeff * (t * t)), t = d - offset_j, d = sqrtf(fmaf(z, z, fmaf(y, y, x * x))), x = pos_b[.] - pos_a[.].  The reference
  takes the fp32 positions, offsets and coeff as the device receives them, carried in fp64.  To first order in u, with v the column's value and a = coeff t^2:
    x, y, z      one subtraction each: relative error u
    d            the operands of the sum of squares carry 2 u each, the sum (all terms positive) 3 roundings on its longest path (x * x and two fmaf): r2 has 5 u;
                 the root halves it and rounds once: |dd| <= 3.5 u d
    t            one subtraction: |dt| <= 3.5 u d + u |t|
    a            t * t: 2 |dt| / |t| + u, the product with coeff: + u:   |da| <= 2 |coeff t| (3.5 u d + u |t|) + 2 u |a| = 7 u |coeff t| d + 4 u |a|
    expf         v |da| from its argument, and 1 ulp <= 2 u v of its own (the bound the HIP math library documents for expf); below the smallest normal number an ulp is
                 absolute and a library may flush: + 2^-126
    delta_j(e) = v (7 u |coeff t| d + 4 u |a| + 2 u) + 2^-126
  An element that reads the row gets  n u (1 + 2^-10) S + (1 + 2^-10) sum_j |d element / d column_j| delta_j, the second term being the ABS form with delta in the
  columns' place (emb, grad_w1's smearing columns, grad_w2; nothing else reads the row's values once the ReLU pattern is fixed).

THE EMULATOR of rhid (`rhid_emulate`), written from the headers of k_rhid.hip and k_reduce.hip with `fma32`, a correctly rounded fp32 fused multiply-add in numpy
(product exact in fp64, TwoSum, the fp64 sum rounded to odd, one rounding to fp32), vectorised over edges:
    h            acc = b1[c]; acc = fmaf(w1[c, k], in[k], acc) for k ascending through [emb | xs[src] | xs[dst]]; acc < 0 ? 0 : acc at p == 0, keep ? relu * s : 0 otherwise
    grad_emb and the two gather rows: gpre = gh * (h != 0 ? s : 0); acc = 0; acc = fmaf(gpre[c], w1[c, k], acc) for c ascending
    grad_xs      seg_ref of the src rows, seg_ref of the dst rows, one add in that order
    grad_w1, grad_b1: per slice of 512 edges of a group acc = fmaf(gpre, in, acc) from +0 over the edges ascending (grad_b1: acc += gpre); then sum = 0; sum += image[s]

THE OPERAND CLASSES.  Every nonzero magnitude lies in [2^-24, 2^4] (a Gaussian clipped to [2^-4, 4] times at most ONE power of two 2^-k, k <= 20, per operand; s, the
receiver's count and the constants aside a term is a product of at most four operands): asserted in fp64 by the generators, with each class's own claims.  The
coordinates of eemb are geometry, not operands of a product, and are outside the window.  RHID_CLASSES, EEMB_CLASSES, HCONV_CLASSES below.

THE FIGURES of the reference evaluations (tests/test_adversarial_dense_host.py prints them: the largest err / (u S) over every class, table, graph and shape used on the
GPU; fp32 numpy in two summation orders, and for rhid the emulator; numbers of the reference evaluation, not of a kernel; elements that read the Gaussian columns are
measured against their whole bar instead, as err / bar):
    rhid        fp32: h 9.8   grad_emb 6.8   grad_xs 3.7   grad_w1 10.5   grad_b1 6.9;   the emulator: h 15.7   grad_emb 6.8   grad_xs 3.7   grad_w1 11.6   grad_b1 4.3
    hconv       centre: out 1.9   grad_x 5.9   grad_h 11.3   grad_w2 11.2   grad_b2 31.9;   torsion: out 4.3   grad_x 2.4   grad_h 9.6   grad_w2 7.8   grad_b2 28.1
    eemb        emb 0.05 (of its bar)   sh 3.6   grad_w1 0.30 (of its bar)   grad_b1 2.9   grad_w2 0.07 (of its bar)   grad_b2 5.3   grad_uemb 5.7   grad_lat 1.4
    (re-draws of b1 that brought a case's ambiguous ReLU branches to 0: one each in five of the 128 eemb cases, none in the others)
and of the mutants of that evaluation, as err / bar on the class built for them, with helpers.rel_err of the block the older tests judge:
    rhid    the smallest unit's bias dropped (unit_spread, h)                        5.1e3    (rel_err of h 1.2e-7: a pass at 1e-5)
            w1 rounded to fp16 (column_spread, h)                                    5.4e1    (rel_err 1.6e-4)
            one edge left out of a slice's grad_w1 (edge_spread)                     2.9e4    (rel_err 3.1e-1)
            the dst sum of one node left out (unit_spread, degrees, grad_xs)         8.0e4    (rel_err 5.3e-1)
    hconv   S72 in place of S6 on block B (column_spread, centre, out)               2.1e3    (rel_err of its block 1.4e-1)
            the cross product's sign in block C (column_spread, centre, out)         2.2e4    (rel_err 2.2)
            a dropped slot in the smallest channel (column_spread, torsion, out)     3.9e3    (rel_err of its block 3.6e-7: a pass at 1e-5)
            a receiver's last row left out of its mean (channel_spread, out)         4.3e2, 3.1e2 (centre, torsion; rel_err 6.2e-3, 3.4e-3)
            one edge left out of grad_w2 (edge_spread)                               3.0e3, 3.1e3 (rel_err 2.8e-1, 1.5e-1)
    eemb    the sigma row taken from idx_b (sig_spread, emb)                         4.1e4    (rel_err 5.3e-1)
            the latent columns of the two sides swapped (latent_spread, emb)         5.4e3    (rel_err 2.7e-1)
            the unc_a uemb term dropped (out_spread, emb)                            1.8e3    (rel_err 6.0e-2)
            the same term dropped in the smallest output column alone                1.5e2    (rel_err of emb 3.2e-7: a pass at 1e-5)
            the offsets shifted by one ulp (lengths; emb, grad_w1, grad_w2)          0.09: UNDER the bar.  An ulp of an offset is 2 u |offset|, no more than what the
            roundings of d (3.5 u d) and of t (u |t|) may move a column by already: no bar that admits an fp32 evaluation of the columns can tell this one (rel_err 5.9e-7)
"""
import numpy as np

import adversarial_training as at
import edge_embedding_ref as eer
import head_conv_ref as hcr
import latent_embedding_ref as lar
import radial_hidden_ref as rhr
from adversarial_training import ABS, FP32_ORDERS, FP64, GRAPHS, HI, LO, SLACK, U, Mode, _base, _ks, _pow, _ulps, bar, graph, node_scale, seg_ref, worst  # noqa: F401

F32 = np.float32
SLICE = 512      # rtp_slice_len(E) for every E used here (E <= 513 <= 240 * 512)


def slice_len(E):
    """rtp_slice_len of ddk_internal.h"""
    return max(512, ((E + 239) // 240 + 63) // 64 * 64)


def SL(n):
    """n + ceil(n / L) + 1 (module docstring)"""
    n = np.asarray(n, np.int64)
    return n + (n + SLICE - 1) // SLICE + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# a correctly rounded fp32 fused multiply-add
# ------------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise with broadcasting.  The product of two fp32 numbers is exact in fp64; TwoSum gives the fp64 sum and its
    exact error; the sum is rounded to odd (when the error is nonzero and the sum's last mantissa bit is even, one ulp towards the error), which makes the
    second rounding, to fp32, the only one that counts (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    p, c = np.broadcast_arrays(p, c)
    shape = p.shape
    s = np.array(p + c, ndmin=1)
    p, c = p.reshape(s.shape), c.reshape(s.shape)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    need = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    step = np.where((err > 0) == (s > 0), 1, -1)      # a float's magnitude grows with its bit pattern, whatever its sign
    out = np.where(need, bits + step, bits).view(np.float64).astype(F32)
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------------------
# shared pieces
# ------------------------------------------------------------------------------------------------------------------------------------
def _nodes(m, rows, idx, n):
    """node sums under mode m: fp64 exactly, fp32 in ascending edge id (rev: descending), one rounding per add"""
    if m.dt is np.float64:
        out = np.zeros((n, rows.shape[1]))
        np.add.at(out, np.asarray(idx, np.int64), rows)
        return out
    if m.rev:
        return seg_ref(rows[::-1], np.asarray(idx)[::-1], n)
    return seg_ref(rows, idx, n)


def _window(o, keys):
    for k in keys:
        a = o[k]
        if a is None:
            continue
        assert a.dtype == F32, k
        mag = np.abs(a.astype(np.float64))
        assert np.all((mag == 0) | ((mag >= LO) & (mag <= HI))), (k, mag[mag > 0].min(), mag.max())


def _groups(offsets):
    return [slice(int(offsets[g]), int(offsets[g + 1])) for g in range(len(offsets) - 1)]


def _large_last(ke, offsets):
    """the last edge of every group and of every 512-slice of a group is among the large ones"""
    last = []
    for sl in _groups(offsets):
        if sl.stop > sl.start:
            last += [min(b + SLICE, sl.stop) - 1 for b in range(sl.start, sl.stop, SLICE)]
    last = np.array(sorted(set(last)), np.int64)
    ke[last] = 1
    return last


# ====================================================================================================================================
# rhid
# ====================================================================================================================================
RH, RP = 72, 24
RHID_CLASSES = ('unit_spread', 'column_spread', 'edge_spread', 'cancelling', 'dead')
RHID_TABLES = ([0, 1, 1, 34, 70], [0, 513])      # a one-edge group, an empty group, ends off the 64 / 128 grid; one slice boundary
RHID_LAYOUTS = ('table0', 'table1') + GRAPHS
RHID_NAMES = ('h', 'grad_xs', 'grad_emb', 'grad_w1', 'grad_b1')
RHID_P = (0.0, 0.25)
RHID_SEED = 0xC0FFEE12345


def rhid_layout(name):
    """dict(src, dst, N, offsets): a group table with random indices over ten of eleven nodes, or one of adversarial_training.GRAPHS on max(n_in, n_out) nodes"""
    if name.startswith('table'):
        i = int(name[5:])
        offsets, N = RHID_TABLES[i], 11
        rng = np.random.default_rng(900 + i)
        src, dst = rng.integers(0, N - 1, offsets[-1]), rng.integers(0, N - 1, offsets[-1])      # node 10 is neither sender nor receiver
    else:
        gr = graph(name)
        src, dst, offsets, N = gr['src'], gr['dst'], gr['offsets'], max(gr['n_in'], gr['n_out'])
    return dict(src=np.asarray(src, np.int64), dst=np.asarray(dst, np.int64), N=N, offsets=list(offsets))


def rhid_rows(m, lay, o):
    xs = m.c(o['xs'])
    return np.concatenate([m.c(o['emb']), xs[lay['src']], xs[lay['dst']]], 1)


def rhid_pre(m, lay, o):
    a, w1, b1 = rhid_rows(m, lay, o), m.c(o['w1']), m.c(o['b1'])
    pre = np.zeros((a.shape[0], RH), m.dt)
    for g, sl in enumerate(_groups(lay['offsets'])):
        pre[sl] = m.mm(a[sl], np.ascontiguousarray(w1[g].T)) + b1[g]
    return pre


def rhid_evaluate(m, lay, o, keep, s, pattern):
    """{name: array} of the op under mode m (radial_hidden_ref.forward / backward restated); keep: the dropout mask; s: the fp64 value of the fp32 scale;
    pattern: bool [E, 72], the zero pattern the backward differentiates through"""
    a, w1 = rhid_rows(m, lay, o), m.c(o['w1'])
    pre = rhid_pre(m, lay, o)
    h = np.where(keep, (pre if m.absolute else np.maximum(pre, 0)) * m.k(s), m.k(0))
    gpre = m.c(o['g']) * np.where(pattern, m.k(s), m.k(0))
    G = len(lay['offsets']) - 1
    gin, gw1, gb1 = np.zeros_like(a), np.zeros((G, RH, RH), m.dt), np.zeros((G, RH), m.dt)
    for g, sl in enumerate(_groups(lay['offsets'])):
        gin[sl] = m.mm(gpre[sl], w1[g])
        gw1[g] = m.mm(np.ascontiguousarray(gpre[sl].T), a[sl])
        gb1[g] = m.sum(gpre[sl], 0)
    gxs = _nodes(m, gin[:, RP:2 * RP], lay['src'], lay['N']) + _nodes(m, gin[:, 2 * RP:], lay['dst'], lay['N'])
    return dict(h=h, grad_xs=gxs, grad_emb=gin[:, :RP].copy(), grad_w1=gw1, grad_b1=gb1)


def rhid_counts(lay):
    N = lay['N']
    deg = np.bincount(lay['src'], minlength=N)[:N] + np.bincount(lay['dst'], minlength=N)[:N]
    ng = np.diff(np.asarray(lay['offsets'], np.int64))
    return dict(h=np.float64(74), grad_emb=np.float64(73), grad_xs=(73 + deg).astype(np.float64)[:, None],
                grad_w1=(1 + SL(ng)).astype(np.float64)[:, None, None], grad_b1=(1 + SL(ng)).astype(np.float64)[:, None])


def rhid_measures(lay, o, p, seed, pattern):
    """{name: (fp64 reference, S, n)}"""
    keep, s = rhr.keep_mask(seed, len(lay['src']), p), rhr.scale(p)
    ref, S, n = rhid_evaluate(FP64, lay, o, keep, s, pattern), rhid_evaluate(ABS, lay, o, keep, s, pattern), rhid_counts(lay)
    return {k: (ref[k], S[k], n[k]) for k in ref}


def rhid_emulate(lay, o, p, seed, parts=False):
    """every output of ddk_rhid_forward / ddk_rhid_backward in the bits the headers of k_rhid.hip and k_reduce.hip promise (module docstring)"""
    src, dst, N, offsets = lay['src'], lay['dst'], lay['N'], lay['offsets']
    xs, emb, w1, b1, gh = (np.asarray(o[k], F32) for k in ('xs', 'emb', 'w1', 'b1', 'g'))
    E, G = len(src), len(offsets) - 1
    rows = np.concatenate([emb, xs[src], xs[dst]], 1)
    s = F32(1) / (F32(1) - F32(p)) if p > 0 else F32(1)
    keep = rhr.keep_mask(seed, E, p)
    h, gin = np.zeros((E, RH), F32), np.zeros((E, RH), F32)
    for g, sl in enumerate(_groups(offsets)):
        acc = np.broadcast_to(b1[g], (sl.stop - sl.start, RH)).copy()
        for k in range(RH):
            acc = fma32(w1[g][None, :, k], rows[sl, k, None], acc)
        relu = np.where(acc < 0, F32(0), acc)
        h[sl] = relu if p == 0 else np.where(keep[sl], (relu * s).astype(F32), F32(0))
    gpre = (gh * np.where(h != 0, s, F32(0)).astype(F32)).astype(F32)
    gw1, gb1 = np.zeros((G, RH, RH), F32), np.zeros((G, RH), F32)
    for g, sl in enumerate(_groups(offsets)):
        acc = np.zeros((sl.stop - sl.start, RH), F32)
        for c in range(RH):
            acc = fma32(gpre[sl, c, None], w1[g][None, c, :], acc)
        gin[sl] = acc
        sw, sb = np.zeros((RH, RH), F32), np.zeros(RH, F32)
        for b in range(sl.start, sl.stop, SLICE):
            iw, ib = np.zeros((RH, RH), F32), np.zeros(RH, F32)
            for e in range(b, min(b + SLICE, sl.stop)):
                iw = fma32(gpre[e][:, None], rows[e][None, :], iw)
                ib = (ib + gpre[e]).astype(F32)
            sw, sb = (sw + iw).astype(F32), (sb + ib).astype(F32)
        gw1[g], gb1[g] = sw, sb
    gxs = (seg_ref(gin[:, RP:2 * RP], src, N) + seg_ref(gin[:, 2 * RP:], dst, N)).astype(F32)
    out = dict(h=h, grad_xs=gxs, grad_emb=gin[:, :RP].copy(), grad_w1=gw1, grad_b1=gb1)
    if parts:
        out.update(gpre=gpre, gin=gin, rows=rows)
    return out


def rhid_operands(cls, layout, seed=5):
    """One case of class `cls` on layout `layout`: dict of fp32 xs [N, 24], emb [E, 24], w1 [G, 72, 72], b1 [G, 72], g = grad_h [E, 72] and 'claims'"""
    lay = rhid_layout(layout)
    src, dst, N, offsets = lay['src'], lay['dst'], lay['N'], lay['offsets']
    E, G = len(src), len(offsets) - 1
    rng = np.random.default_rng([seed, RHID_CLASSES.index(cls), RHID_LAYOUTS.index(layout)])
    xs, emb, w1, b1, g = _base(rng, N, RP), _base(rng, E, RP), _base(rng, G, RH, RH), _base(rng, G, RH), _base(rng, E, RH)
    claims = {}
    groups, sizes = _groups(offsets), np.diff(np.asarray(offsets))
    if cls == 'unit_spread':
        ku = _ks(rng, RH)
        w1, b1, g = w1 * _pow(ku)[None, :, None], b1 * _pow(ku)[None, :], g * _pow(ku)[None, :]
        claims.update(ku=ku, small_unit=int(np.argmax(ku)))
        assert ku.max() == 20 and ku.min() == 0
    elif cls == 'column_spread':
        kc = _ks(rng, RH)
        w1 = w1 * _pow(kc)[None, None, :]
        claims.update(kc=kc, small_column=int(np.argmax(kc)))
    elif cls == 'edge_spread':
        ke, kn = _ks(rng, E), _ks(rng, N)
        claims['last_edges'] = _large_last(ke, offsets)
        emb, g, xs = emb * _pow(ke)[:, None], g * _pow(ke)[:, None], xs * _pow(kn)[:, None]
        claims.update(ke=ke, kn=kn)
    elif cls == 'cancelling':      # inputs in equal pairs, weights (y, -(y + 1..3 ulp)), no bias
        emb[:, 1::2], xs[:, 1::2] = emb[:, 0::2], xs[:, 0::2]
        w1[:, :, 1::2] = -np.sign(w1[:, :, 0::2]) * _ulps(w1[:, :, 0::2], rng)
        b1[:] = 0
    elif cls == 'dead':
        full = [q for q in range(G) if sizes[q] > 1]
        zg, gl = (full[-1], full[-2]) if len(full) > 1 else (None, full[-1])
        if zg is not None:      # one whole group whose every unit is off: negative weights on a positive embedding, nothing from the node table, a negative bias
            w1[zg, :, :RP], w1[zg, :, RP:] = -np.abs(w1[zg, :, :RP]), 0
            b1[zg] = -np.abs(b1[zg])
            emb[groups[zg]] = np.abs(emb[groups[zg]])
        # group gl: edges with a single unit alive.  w1[gl][c, j] > 0 only for c == j < 24, nothing from the node table, a small negative bias; a lone edge's
        # embedding is one positive column j: unit j alone passes
        w1[gl, :, RP:] = 0
        w1[gl, :, :RP] = -np.abs(w1[gl, :, :RP])
        w1[gl, np.arange(RP), np.arange(RP)] = np.abs(w1[gl, np.arange(RP), np.arange(RP)])
        b1[gl] = -np.abs(b1[gl]) * _pow(11)
        emb[groups[gl]] = np.abs(emb[groups[gl]])
        lone = np.arange(groups[gl].start, groups[gl].stop, 3)
        units = lone % RP
        keepv = emb[lone, units].copy()
        emb[lone] = 0
        emb[lone, units] = keepv
        claims.update(zero_group=zg, lone_group=gl, lone_edges=lone, lone_units=units)
    else:
        raise ValueError(cls)
    o = dict(xs=xs, emb=emb, w1=w1, b1=b1, g=g, claims=claims)
    _window(o, ('xs', 'emb', 'w1', 'b1', 'g'))
    pre, Spre = rhid_pre(FP64, lay, o), rhid_pre(ABS, lay, o)
    if cls == 'cancelling':
        assert E == 0 or ((Spre > 0).all() and np.all(np.abs(pre) <= 2.0 ** -18 * Spre))
    if cls == 'dead':
        if claims['zero_group'] is not None:
            assert (pre[groups[claims['zero_group']]] < 0).all()
        on = pre[claims['lone_edges']] > 0
        assert (on.sum(1) == 1).all() and on[np.arange(len(on)), claims['lone_units']].all()
    return o


def rhid_locate(name, where, lay):
    """where an element sits in the kernels' decomposition, for a failure's report"""
    text = f'{name}{list(where)}'
    offsets = np.asarray(lay['offsets'])
    if name in ('h', 'grad_emb'):
        e = where[0]
        g = int(np.searchsorted(offsets, e, side='right') - 1)
        r = e - int(offsets[g])
        text += (f': edge {e} = group {g} + {r}: workgroup {r // 128} of its group, wave {(r % 128) // 64}, lane {r % 64}; slice {r // SLICE} + {r % SLICE}; '
                 + (f'unit {where[1]}' if name == 'h' else f'column {where[1]}'))
    elif name == 'grad_xs':
        n = where[0]
        text += f': node {n} ({int((lay["src"] == n).sum())} edges as src, {int((lay["dst"] == n).sum())} as dst), column {where[1]}'
    elif name in ('grad_w1', 'grad_b1'):
        g = where[0]
        n = int(offsets[g + 1] - offsets[g])
        text += f': group {g} ({n} edges, {(n + SLICE - 1) // SLICE} slices), unit {where[1]}'
        if name == 'grad_w1':
            text += f', column {where[2]} ({("emb", "xs[src]", "xs[dst]")[where[2] // RP]} + {where[2] % RP})'
    return text


# ====================================================================================================================================
# hconv
# ====================================================================================================================================
HCONV_CLASSES = ('column_spread', 'channel_spread', 'edge_spread', 'relu_sparse', 'degenerate_sh', 'cancelling', 'zero_blocks')
HCONV_NAMES = ('out', 'grad_x', 'grad_h', 'grad_w2', 'grad_b2')
HC_SOURCE = ({'A': '0e', 'B': '1o', 'C': '1o', 'D': '1e', 'E': '1e', 'F': '0o'}, {'P': '1o', 'Q': '1e'})      # the input irrep that makes a block's rows


def hc_slot_table(head):
    """per weight slot [W]: (block name, row, column, output channel, input irrep, output irrep).  Channels: the centre head's four vectors (2x1o, 2x1e: a
    channel owns three out columns), the torsion head's 48 scalars"""
    W = hcr.W[head]
    blk, row, col, ch, src, oir = [None] * W, np.zeros(W, np.int64), np.zeros(W, np.int64), np.zeros(W, np.int64), [None] * W, [None] * W
    for n, (off, r, c, io) in hcr.BLOCKS[head].items():
        for i in range(r * c):
            p = off + i
            blk[p], row[p], col[p], src[p], oir[p] = n, i // c, i % c, HC_SOURCE[head][n], io
            ch[p] = ({'1o': 0, '1e': 2}[io] + i % c) if head == 0 else (hcr.OUT_SLICES[1][io].start + i % c)
    return np.array(blk), row, col, ch, np.array(src), np.array(oir)


def hc_out_channel(head):
    """[dout] the channel of every out column"""
    return np.arange(12) // 3 if head == 0 else np.arange(48)


def _hc_parts(xe):
    return xe[:, :24], xe[:, 24:42].reshape(-1, 6, 3), xe[:, 42:60].reshape(-1, 6, 3), xe[:, 60:]


def hc_u(m, head, xe, sh, consts=None):
    """the scaled pre-weight rows per block (head_conv_ref._center_rows / tp_rows under mode m); consts: {block: constant} overrides (the mutants)"""
    a, p, q, c = _hc_parts(xe)
    k = lambda n, v: m.k((consts or {}).get(n, v))
    if head == 0:
        s0, v = sh[:, 0][:, None, None], sh[:, None, 1:4]
        return {'A': a[:, :, None] * v * k('A', hcr.S6), 'B': p * s0 * k('B', hcr.S6), 'C': at._cross(m, p, v) * k('C', hcr.S72),
                'D': q * s0 * k('D', hcr.S6), 'E': at._cross(m, q, v) * k('E', hcr.S72), 'F': c[:, :, None] * v * k('F', hcr.S6)}
    T = sh[:, None, 1:4]
    return {'P': m.sum(p * T, -1) * k('P', hcr.S18), 'Q': m.sum(q * T, -1) * k('Q', hcr.S18)}


def hc_weights(m, o):
    return m.mm(m.c(o['h']), np.ascontiguousarray(m.c(o['w2']).T)) + m.c(o['b2'])


def hc_rows(m, head, Us, w):
    """the tensor product per edge [E, dout]"""
    E = w.shape[0]
    if head == 0:
        acc = {'1o': np.zeros((E, 2, 3), m.dt), '1e': np.zeros((E, 2, 3), m.dt)}
        for n, (off, r, c, io) in hcr.CENTER_BLOCKS.items():
            acc[io] = acc[io] + m.sum(Us[n][:, :, None, :] * w[:, off:off + r * c].reshape(E, r, c)[:, :, :, None], 1)
        return np.concatenate([acc['1o'].reshape(E, 6), acc['1e'].reshape(E, 6)], 1)
    o0e = m.sum(Us['P'][:, :, None] * w[:, :144].reshape(E, 6, 24), 1)
    o0o = m.sum(Us['Q'][:, :, None] * w[:, 144:].reshape(E, 6, 24), 1)
    return np.concatenate([o0o, o0e], 1)


def hc_vjp_rows(m, head, xe, sh, Us, w, ge):
    """(grad_xe [E, 84], gw [E, W]) per edge (head_conv_ref.tp_vjp under mode m)"""
    E = w.shape[0]
    gxe, gw = np.zeros((E, hcr.DIN), m.dt), np.zeros((E, hcr.W[head]), m.dt)
    if head == 0:
        s0, v = sh[:, 0][:, None, None], sh[:, None, 1:4]
        g = {'1o': ge[:, :6].reshape(E, 2, 3), '1e': ge[:, 6:].reshape(E, 2, 3)}
        ga, gp, gq, gc = np.zeros((E, 24), m.dt), np.zeros((E, 6, 3), m.dt), np.zeros((E, 6, 3), m.dt), np.zeros((E, 24), m.dt)
        S6, S72 = m.k(hcr.S6), m.k(hcr.S72)
        for n, (off, r, c, io) in hcr.CENTER_BLOCKS.items():
            wb = w[:, off:off + r * c].reshape(E, r, c)
            gw[:, off:off + r * c] = m.sum(Us[n][:, :, None, :] * g[io][:, None, :, :], -1).reshape(E, r * c)
            gU = m.sum(wb[:, :, :, None] * g[io][:, None, :, :], 2)
            if n == 'A':
                ga = ga + m.sum(gU * v, -1) * S6
            elif n == 'F':
                gc = gc + m.sum(gU * v, -1) * S6
            elif n == 'B':
                gp = gp + gU * s0 * S6
            elif n == 'D':
                gq = gq + gU * s0 * S6
            elif n == 'C':
                gp = gp + at._cross(m, v, gU) * S72
            else:
                gq = gq + at._cross(m, v, gU) * S72
        gxe[:, :24], gxe[:, 24:42], gxe[:, 42:60], gxe[:, 60:] = ga, gp.reshape(E, 18), gq.reshape(E, 18), gc
        return gxe, gw
    T, S18 = sh[:, None, 1:4], m.k(hcr.S18)
    g0o, g0e = ge[:, :24], ge[:, 24:]
    gw[:, :144] = (Us['P'][:, :, None] * g0e[:, None, :]).reshape(E, 144)
    gw[:, 144:] = (Us['Q'][:, :, None] * g0o[:, None, :]).reshape(E, 144)
    gup = m.sum(w[:, :144].reshape(E, 6, 24) * g0e[:, None, :], 2)
    guq = m.sum(w[:, 144:].reshape(E, 6, 24) * g0o[:, None, :], 2)
    gxe[:, 24:42] = (gup[:, :, None] * T * S18).reshape(E, 18)
    gxe[:, 42:60] = (guq[:, :, None] * T * S18).reshape(E, 18)
    return gxe, gw


def hconv_evaluate(m, head, gr, o, consts=None):
    """{name: array} of ddk_hconv_forward / ddk_hconv_backward under mode m (head_conv_ref.forward / vjp restated)"""
    src, dst, n_in, n_out = np.asarray(gr['src'], np.int64), np.asarray(gr['dst'], np.int64), gr['n_in'], gr['n_out']
    x, sh, h, w2, g = m.c(o['x']), m.c(o['sh']), m.c(o['h']), m.c(o['w2']), m.c(o['g'])
    cnt = at.node_counts(src, n_out).astype(m.dt)[:, None]
    w = hc_weights(m, o)
    Us = hc_u(m, head, x[dst], sh, consts)
    out = _nodes(m, hc_rows(m, head, Us, w), src, n_out) / cnt
    gxe, gw = hc_vjp_rows(m, head, x[dst], sh, Us, w, (g / cnt)[src])
    return dict(out=out, grad_x=_nodes(m, gxe, dst, n_in), grad_h=m.mm(gw, w2), grad_w2=m.mm(np.ascontiguousarray(gw.T), h), grad_b2=m.sum(gw, 0))


def hconv_counts(head, gr):
    K, W, E = hcr.K[head], hcr.W[head], len(gr['src'])
    ds = np.bincount(np.asarray(gr['src'], np.int64), minlength=gr['n_out'])[:gr['n_out']].astype(np.float64)[:, None]
    dd = np.bincount(np.asarray(gr['dst'], np.int64), minlength=gr['n_in'])[:gr['n_in']].astype(np.float64)[:, None]
    n_out, n_x = ((K + 43, K + 12), (K + 15, K + 29))[head]
    return dict(out=n_out + ds, grad_x=n_x + dd, grad_h=np.float64(9 + W), grad_w2=np.float64(9 + SL(E)), grad_b2=np.float64(9 + SL(E)))


def hconv_measures(head, gr, o):
    ref, S, n = hconv_evaluate(FP64, head, gr, o), hconv_evaluate(ABS, head, gr, o), hconv_counts(head, gr)
    return {k: (ref[k], S[k], n[k]) for k in ref}


def hconv_operands(cls, head, gname, seed=7, variant='x'):
    """One case of class `cls` for head `head` on graph `gname`: dict of fp32 x [n_in, 84], sh [E, 4], h [E, K], w2 [W, K], b2 [W], g = grad_out [n_out, dout]
    and 'claims'.  The classes of adversarial_training.operands carried over: x and g are node tables, so what scales per edge there scales h per edge and
    x, g per node here."""
    gr = graph(gname)
    src, dst, n_in, n_out = np.asarray(gr['src'], np.int64), np.asarray(gr['dst'], np.int64), gr['n_in'], gr['n_out']
    E, K, W, dout = len(src), hcr.K[head], hcr.W[head], hcr.DOUT[head]
    rng = np.random.default_rng([seed, head, HCONV_CLASSES.index(cls), GRAPHS.index(gname), int(variant == 'g')])
    x, sh, g = _base(rng, n_in, hcr.DIN), _base(rng, E, 4), _base(rng, n_out, dout)
    h = _base(rng, E, K, signed=False) * (rng.random((E, K)) < 0.5)      # what ReLU leaves
    w2, b2 = _base(rng, W, K), _base(rng, W)
    blk, row, col, ch, isrc, oir = hc_slot_table(head)
    claims = {}
    if cls == 'column_spread':
        nch = 4 if head == 0 else 48
        kc = _ks(rng, nch)
        w2, b2, g = w2 * _pow(kc)[ch][:, None], b2 * _pow(kc)[ch], g * _pow(kc)[hc_out_channel(head)][None, :]
        claims.update(kc=kc, small_channel=int(np.argmax(kc)))
        assert kc.max() == 20 and kc.min() == 0
    elif cls == 'channel_spread':
        kk = _ks(rng, 60)
        x = x * np.concatenate([_pow(kk[:24]), np.repeat(_pow(kk[24:30]), 3), np.repeat(_pow(kk[30:36]), 3), _pow(kk[36:])])[None, :]
        h = h * _pow(_ks(rng, K))[None, :]
    elif cls == 'edge_spread':
        ke = _ks(rng, E)
        claims['last_edges'] = _large_last(ke, [0, E])
        h, x, g = h * _pow(ke)[:, None], x * _pow(_ks(rng, n_in))[:, None], g * _pow(_ks(rng, n_out))[:, None]
    elif cls == 'relu_sparse':
        h = _base(rng, E, K, signed=False) * (rng.random((E, K)) < 0.15)
        dead = np.arange(2, E, 9)
        h[dead] = 0
        claims['dead_edges'] = dead
        assert 0.8 < (h == 0).mean() < 0.97
    elif cls == 'degenerate_sh':
        sh[0::8, 1:4] = 0      # v = 0
        sh[1::8, 0] = 0      # s0 = 0
        sh[2::8, 1:3] = 0      # v along z
        sh[3::8, 2:4] = 0      # v along x
        # v parallel to every p and q of the edge: the even nodes' vectors all lie along one direction of their node, and every edge e % 8 >= 4 that reads such a
        # node has v along it too (scaled by powers of two: each cross product cancels to exactly 0, product by product, while its S does not)
        nodes = np.arange(0, n_in, 2)
        d = _base(rng, n_in, 3)
        lam = np.exp2(rng.integers(-3, 3, size=(len(nodes), 12))).astype(F32)
        x[nodes, 24:60] = (lam[:, :, None] * d[nodes, None, :]).reshape(len(nodes), 36)
        par = np.nonzero((np.arange(E) % 8 >= 4) & (dst % 2 == 0))[0]
        sh[par, 1:4] = np.exp2(rng.integers(-2, 2, size=(len(par), 1))).astype(F32) * d[dst[par]]
        claims['parallel_edges'] = par
        assert len(par)
    elif cls == 'cancelling':
        # (a) weight slots whose  sum_k W2[p, k] h[k] + b2[p]  cancels: hidden units in equal pairs, the slot's weights in pairs (y, -(y + 1..3 ulp)), no bias
        # (b) an out channel that cancels: its rows come in pairs with equal inputs and weights (y, -(y + ulp)); the other blocks that feed it carry no weight
        h[:, 1::2] = h[:, 0::2]
        if head == 0:      # channel 1 (the second 1o vector): block A's rows in pairs a_2i = a_2i+1; blocks B and E silent in it
            x[:, 1:24:2] = x[:, 0:24:2]
            even = np.nonzero((blk == 'A') & (col == 1) & (row % 2 == 0))[0]
            odd = even + 2
            rest = np.nonzero(((blk == 'B') | (blk == 'E')) & (col == 1))[0]
            cols = [3, 4, 5]
        else:      # out column 25 (block P, column 1): the six p vectors in equal pairs
            pv = x[:, 24:42].reshape(n_in, 6, 3)
            pv[:, 1::2] = pv[:, 0::2]
            x[:, 24:42] = pv.reshape(n_in, 18)
            even = np.nonzero((blk == 'P') & (col == 1) & (row % 2 == 0))[0]
            odd = even + 24
            rest = np.zeros(0, np.int64)
            cols = [25]
        assert (blk[odd] == blk[even]).all() and (row[odd] == row[even] + 1).all() and (col[odd] == 1).all()
        slots = np.setdiff1d(np.arange(0, W, 5), np.concatenate([even, odd, rest]))
        w2[slots, 1::2] = -np.sign(w2[slots, 0::2]) * _ulps(w2[slots, 0::2], rng)
        b2[slots] = 0
        w2[odd] = -np.sign(w2[even]) * _ulps(w2[even], rng)
        b2[odd] = -np.sign(b2[even]) * _ulps(b2[even], rng)
        w2[rest], b2[rest] = 0, 0
        claims.update(slots=slots, out_columns=cols)
    elif cls == 'zero_blocks':
        if variant == 'x':      # the 1e vectors of the node row
            x[:, hcr.X_SLICES['1e']] = 0
            zero = np.nonzero(isrc == '1e')[0]
            claims['zero_x'] = '1e'
        else:      # the second block of grad_out
            io = ('1e', '0e')[head]
            g[:, hcr.OUT_SLICES[head][io]] = 0
            zero = np.nonzero(oir == io)[0]
            claims['zero_g'] = io
        claims['zero_slots'] = zero      # grad_w2[zero], grad_b2[zero] must be exactly zero
        assert len(zero)
    else:
        raise ValueError(cls)
    o = dict(x=x, sh=sh, h=h, w2=w2, b2=b2, g=g, claims=claims)
    _window(o, ('x', 'sh', 'h', 'w2', 'b2', 'g'))
    if cls == 'degenerate_sh' and head == 0:
        e = claims['parallel_edges']
        _, p, q, _ = _hc_parts(x[dst[e]].astype(np.float64))
        v = sh[e, None, 1:4].astype(np.float64)
        for t in (p, q):
            assert not at._cross(FP64, t, v).any() and at._cross(ABS, np.abs(t), np.abs(v)).max() > 0
            assert not at._cross(Mode(F32), t.astype(F32), v.astype(F32)).any()
    if cls == 'cancelling':
        w, Sw = hc_weights(FP64, o), hc_weights(ABS, o)
        alive = Sw[:, claims['slots']] > 0
        assert alive.any() and np.all(np.abs(w[:, claims['slots']]) <= 2.0 ** -18 * Sw[:, claims['slots']])
        ref, S = hconv_evaluate(FP64, head, gr, o)['out'], hconv_evaluate(ABS, head, gr, o)['out']
        has = np.bincount(src, minlength=n_out)[:n_out] > 0
        c = claims['out_columns']
        assert (S[has][:, c] > 0).all() and np.all(np.abs(ref[:, c]) <= 2.0 ** -18 * S[:, c])
    if cls == 'zero_blocks':
        ev = hconv_evaluate(ABS, head, gr, o)
        assert not ev['grad_w2'][claims['zero_slots']].any() and not ev['grad_b2'][claims['zero_slots']].any()
    return o


def hconv_locate(name, where, head, gr):
    text = f'{name}{list(where)}'
    if name in ('out', 'grad_x'):
        idx = gr['src'] if name == 'out' else gr['dst']
        text += f': node {where[0]} ({int((np.asarray(idx) == where[0]).sum())} edges), column {where[1]}'
        if name == 'out':
            text += f' (channel {int(hc_out_channel(head)[where[1]])})'
    elif name == 'grad_h':
        e = where[0]
        text += f': edge {e}: workgroup {e // 64}, lane {e % 64} of every tile\'s wave; slice {e // SLICE} + {e % SLICE}; hidden unit {where[1]}'
    else:
        blk, row, col, ch, isrc, oir = hc_slot_table(head)
        p = where[0]
        text += f': slot {p} = block {blk[p]}, row {int(row[p])}, column {int(col[p])} (channel {int(ch[p])}, fed by {isrc[p]}, into {oir[p]})'
        if name == 'grad_w2':
            text += f', hidden unit {where[1]}'
    return text


# ====================================================================================================================================
# eemb
# ====================================================================================================================================
EH, ED = 24, 32
EEMB_CLASSES = ('hidden_spread', 'out_spread', 'sig_spread', 'latent_spread', 'edge_spread', 'out_cancelling', 'lengths')
# name -> F (bond features), L (latent columns per side; 0: the plain op), unc (unc_a / uemb given), zero (zero_latent)
EEMB_CONFIGS = {'plain64': dict(F=0, L=0, unc=False, zero=False), 'plain68': dict(F=4, L=0, unc=False, zero=False),
                'lat2': dict(F=4, L=2, unc=True, zero=False), 'lat4': dict(F=0, L=4, unc=False, zero=False), 'lat4zero': dict(F=0, L=4, unc=True, zero=True)}
EEMB_E = (1, 65, 130, 513)
EEMB_TABLES = {4: (0.0, 5.0), 0: (0.0, 30.0)}      # (start, stop) by F: the ligand group's expansion with bond features, the receptor's without
EEMB_NA, EEMB_NB = 7, 11
EEMB_SEED = 0x5EED0123456


def eemb_p(cls, E):
    """the dropout rate a case runs with (the mask is a function of the edge's position): 0.25 on the two odd sizes, none where hidden units must stay in pairs"""
    return 0.25 if E in (65, 513) and cls != 'out_cancelling' else 0.0


def eemb_cases():
    return [(cls, cfg, E) for cfg, c in EEMB_CONFIGS.items() for cls in EEMB_CLASSES for E in EEMB_E if c['L'] and not c['zero'] or cls != 'latent_spread']


def _ee_geometry(m, o):
    """(vec [E, 3], d [E]) under mode m; fp32: the device's expression, with separate products and adds (a bound that holds for them holds for the fused form)"""
    ia, ib = np.asarray(o['idx_a'], np.int64), np.asarray(o['idx_b'], np.int64)
    if m.dt is F32:
        vec = (o['pos_b'][ib] - o['pos_a'][ia]).astype(F32)
        return vec, np.sqrt(((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]).astype(F32) + vec[:, 2] * vec[:, 2]).astype(F32)).astype(F32)
    vec = o['pos_b'].astype(np.float64)[ib] - o['pos_a'].astype(np.float64)[ia]
    return vec, np.sqrt((vec * vec).sum(1))


def ee_smear(m, o, offsets=None):
    """the 32 Gaussian columns [E, 32]; fp32: every step rounded to fp32, the exponential correctly rounded"""
    _, d = _ee_geometry(m, o)
    off = eer.offsets(o['start'], o['stop']) if offsets is None else offsets
    k = eer.coeff(o['start'], o['stop'])
    if m.dt is F32:
        t = (d[:, None] - off[None, :]).astype(F32)
        a = (F32(k) * (t * t).astype(F32)).astype(F32)
        with np.errstate(under='ignore'):
            return np.exp(a.astype(np.float64)).astype(F32)
    t = d[:, None] - off.astype(np.float64)[None, :]
    return np.exp(k * t * t)


def ee_delta(o):
    """delta_j(e) [E, 32] (module docstring)"""
    _, d = _ee_geometry(FP64, o)
    k = eer.coeff(o['start'], o['stop'])
    t = d[:, None] - eer.offsets(o['start'], o['stop']).astype(np.float64)[None, :]
    a = np.abs(k * t * t)
    return np.exp(-a) * (7 * U * np.abs(k * t) * d[:, None] + 4 * U * a + 2 * U) + 2.0 ** -126


def ee_row(m, cfg, o, delta=None, mutate=None):
    """the row [E, K] under mode m; delta: that array in the Gaussian columns' place and zeros elsewhere"""
    c = EEMB_CONFIGS[cfg]
    ia, ib = np.asarray(o['idx_a'], np.int64), np.asarray(o['idx_b'], np.int64)
    E = len(ia)
    mutate = mutate or {}
    sig_of = (ib % len(o['sig_index'])) if mutate.get('sig_from_b') else ia
    parts = [m.c(o['feat'])] if c['F'] else []
    parts += [m.c(o['sig'])[np.asarray(o['sig_index'], np.int64)[sig_of]], ee_smear(m, o, mutate.get('offsets')).astype(m.dt)]
    if c['L']:
        if c['zero']:
            parts += [np.zeros((E, 2 * c['L']), m.dt)]
        else:
            la, lb = m.c(o['lat_a'])[ia], m.c(o['lat_b'])[ib]
            parts += [lb[:, :c['L']], la[:, :c['L']]] if mutate.get('swap_latent') else [la, lb]
    a = np.concatenate(parts, 1)
    if delta is not None:
        k0 = c['F'] + ED
        z = np.zeros_like(a)
        z[:, k0:k0 + ED] = delta
        return z
    return a


def eemb_evaluate(m, cfg, o, keep, s, on, delta=None, mutate=None):
    """{name: array} of ddk_eemb(_latent)_forward / _backward under mode m (edge_embedding_ref / latent_embedding_ref restated).  keep: the dropout mask; on: bool
    [E, 24], where ReLU and mask pass (the backward's pattern; the generator's cap of 0 makes it the same in every arithmetic); delta: the ABS form with delta in the
    Gaussian columns' place, every output that does not read the row's values zero."""
    c = EEMB_CONFIGS[cfg]
    mutate = mutate or {}
    ia, ib = np.asarray(o['idx_a'], np.int64), np.asarray(o['idx_b'], np.int64)
    E, L = len(ia), c['L']
    a = ee_row(m, cfg, o, delta, mutate)
    w1, w2, g = m.c(o['w1']), m.c(o['w2']), m.c(o['g'])
    b1, b2 = (m.c(o['b1']), m.c(o['b2'])) if delta is None else (np.zeros(EH, m.dt), np.zeros(EH, m.dt))
    pre = m.mm(a, np.ascontiguousarray(w1.T)) + b1
    hid_f = np.where(keep, (pre if m.absolute else np.maximum(pre, 0)) * m.k(s), m.k(0))
    emb = m.mm(hid_f, np.ascontiguousarray(w2.T)) + b2
    if c['unc'] and delta is None and not mutate.get('drop_unc'):
        emb = emb + m.c(o['unc_a'])[ia][:, None] * m.c(o['uemb'])[None, :]
    hid_b = np.where(on, pre * m.k(s), m.k(0))
    gpre = m.mm(g, w2) * np.where(on, m.k(s), m.k(0))
    out = dict(emb=emb, grad_w1=m.mm(np.ascontiguousarray(gpre.T), a), grad_b1=m.sum(gpre, 0), grad_w2=m.mm(np.ascontiguousarray(g.T), hid_b), grad_b2=m.sum(g, 0))
    vec, d = _ee_geometry(m, o)
    if m.dt is F32:
        out['sh'] = np.concatenate([np.ones((E, 1), F32), (vec * (F32(1.7320508075688772) / np.maximum(d, F32(1e-12))).astype(F32)[:, None]).astype(F32)], 1)
    else:
        sh = eer.spherical_harmonics(vec, d)
        out['sh'] = np.abs(sh) if m.absolute else sh
    if L:
        unc = m.c(o['unc_a']) if c['unc'] else np.zeros(EEMB_NA, m.dt)
        out['grad_uemb'] = m.sum(unc[ia][:, None] * g, 0)
        K0 = a.shape[1] - 2 * L
        if c['zero']:
            out['grad_w1'][:, K0:] = 0
            out['grad_lat_a'], out['grad_lat_b'] = np.zeros((EEMB_NA, L), m.dt), np.zeros((EEMB_NB, L), m.dt)
        else:
            glat = m.mm(gpre, w1[:, K0:])
            out['grad_lat_a'], out['grad_lat_b'] = _nodes(m, glat[:, :L], ia, EEMB_NA), _nodes(m, glat[:, L:], ib, EEMB_NB)
    if delta is not None:
        for k in out:
            if k not in ('emb', 'grad_w1', 'grad_w2'):
                out[k] = np.zeros_like(out[k])
    return out


def eemb_counts(cfg, o):
    c = EEMB_CONFIGS[cfg]
    E, K = len(o['idx_a']), c['F'] + 64 + 2 * c['L']
    sl = float(SL(E))
    n = dict(emb=np.float64(K + 28), sh=np.array([0.0, 8.0, 8.0, 8.0])[None, :], grad_w1=np.float64(25 + sl), grad_b1=np.float64(25 + sl),
             grad_w2=np.float64(K + 2 + sl), grad_b2=np.float64(sl))
    if c['L']:
        da = np.bincount(np.asarray(o['idx_a'], np.int64), minlength=EEMB_NA)[:EEMB_NA].astype(np.float64)[:, None]
        db = np.bincount(np.asarray(o['idx_b'], np.int64), minlength=EEMB_NB)[:EEMB_NB].astype(np.float64)[:, None]
        n.update(grad_uemb=np.float64(sl), grad_lat_a=49 + da, grad_lat_b=49 + db)
    return n


def eemb_pattern(cfg, o, p, seed):
    """(keep, s, on): the mask, the scale and the backward's pattern, from the fp64 pre-activation"""
    E = len(o['idx_a'])
    keep, s = eer.keep_mask(seed, E, p), eer.scale(p)
    pre = ee_row(FP64, cfg, o) @ o['w1'].astype(np.float64).T + o['b1'].astype(np.float64)
    return keep, s, keep & (pre > 0)


def eemb_measures(cfg, o, p, seed):
    """{name: (fp64 reference, S, n)}.  Where an element reads the Gaussian columns, S carries their term: S + extra / (n u (1 + 2^-10)), so that
    adversarial_training.bar(n, S) is  n u (1 + 2^-10) S + (1 + 2^-10) sum_j |d element / d column_j| delta_j  (the helper's `worst` then serves unchanged)"""
    keep, s, on = eemb_pattern(cfg, o, p, seed)
    ref, S, n = eemb_evaluate(FP64, cfg, o, keep, s, on), eemb_evaluate(ABS, cfg, o, keep, s, on), eemb_counts(cfg, o)
    extra = eemb_evaluate(ABS, cfg, o, keep, s, on, delta=ee_delta(o))
    S['sh'][:, 0] = 0      # the constant 1: exact
    M = {}
    for k in ref:
        Sk = S[k] + (SLACK * extra[k] / (n[k] * U * SLACK) if k in ('emb', 'grad_w1', 'grad_w2') else 0.0)
        M[k] = (ref[k], Sk, n[k])
    return M


def eemb_kinks(cfg, o):
    """bool [E, 24]: the (edge, unit)s whose |pre| is under the fp32 margin of edge_embedding_ref.pre_activation (latent_embedding_ref's with latents), or under
    this module's own bar of pre"""
    c = EEMB_CONFIGS[cfg]
    oo = dict(o, feat=o['feat'] if c['F'] else None, zero_latent=c['zero'])
    pre, margin = lar.pre_activation(oo, o['w1'], o['b1'], c['L']) if c['L'] else eer.pre_activation(oo, o['w1'], o['b1'])
    a, w1 = ee_row(ABS, cfg, o), np.abs(o['w1'].astype(np.float64))
    K = a.shape[1]
    own = (K + 2) * U * SLACK * (a @ w1.T + np.abs(o['b1'].astype(np.float64))) + SLACK * ee_row(ABS, cfg, o, ee_delta(o)) @ w1.T
    return np.abs(pre) < np.maximum(margin, own)


def eemb_operands(cls, cfg, E, seed=9):
    """One case: dict of pos_a [7, 3], pos_b [11, 3], idx_a, idx_b [E] int32, feat [E, 4] or None, sig [3, 32], sig_index [7] int32, start, stop, w1 [24, K], b1,
    w2 [24, 24], b2, g = grad_emb [E, 24] and, by the configuration, lat_a [7, L], lat_b [11, L], unc_a [7], uemb [24]; 'claims'; 'redraws': how many times a
    unit's b1 was drawn again to bring the case's ambiguous ReLU branches to 0"""
    c = EEMB_CONFIGS[cfg]
    F, L = c['F'], c['L']
    K = F + 64 + 2 * L
    rng = np.random.default_rng([seed, EEMB_CLASSES.index(cls), list(EEMB_CONFIGS).index(cfg), E])
    start, stop = EEMB_TABLES[F]
    f = lambda *shape: rng.standard_normal(shape).astype(F32)
    o = dict(pos_a=f(EEMB_NA, 3) * F32(stop / 4), pos_b=f(EEMB_NB, 3) * F32(stop / 4), idx_a=rng.integers(0, EEMB_NA, E).astype(np.int32),
             idx_b=rng.integers(0, EEMB_NB, E).astype(np.int32), feat=None, sig=_base(rng, 3, 32), sig_index=rng.integers(0, 3, EEMB_NA).astype(np.int32),
             start=start, stop=stop, w1=_base(rng, EH, K), b1=_base(rng, EH), w2=_base(rng, EH, EH), b2=_base(rng, EH), g=_base(rng, E, EH))
    if F:
        o['feat'] = np.eye(4, dtype=F32)[rng.integers(0, 4, E)] * (rng.random(E) < 0.7)[:, None].astype(F32)
    if L:
        o.update(lat_a=_base(rng, EEMB_NA, L), lat_b=_base(rng, EEMB_NB, L))
    if c['unc']:
        o.update(unc_a=_base(rng, EEMB_NA, signed=False) * (rng.random(EEMB_NA) < 0.6), uemb=_base(rng, EH))
        o['unc_a'][0] = 1      # (never all zero)
    claims, b1_scale, pairs = {}, np.ones(EH, F32), False
    if cls == 'hidden_spread':
        kh = _ks(rng, EH)
        b1_scale = _pow(kh)
        o['w1'], o['b1'] = o['w1'] * b1_scale[:, None], o['b1'] * b1_scale
        claims.update(kh=kh, small_unit=int(np.argmax(kh)))
    elif cls == 'out_spread':
        ko = _ks(rng, EH)
        o['w2'], o['b2'], o['g'] = o['w2'] * _pow(ko)[:, None], o['b2'] * _pow(ko), o['g'] * _pow(ko)[None, :]
        if c['unc']:
            o['uemb'] = o['uemb'] * _pow(ko)
        claims.update(ko=ko, small_column=int(np.argmax(ko)))
    elif cls == 'sig_spread':
        ks = _ks(rng, 32)
        o['sig'] = o['sig'] * _pow(ks)[None, :]
        claims.update(ks=ks)
    elif cls == 'latent_spread':
        assert L and not c['zero']
        ka, kb = _ks(rng, L), _ks(rng, L)
        o['lat_a'], o['lat_b'] = o['lat_a'] * _pow(ka)[None, :], o['lat_b'] * _pow(kb)[None, :]
        claims.update(ka=ka, kb=kb)
    elif cls == 'edge_spread':
        ke = _ks(rng, E)
        if E:
            claims['last_edges'] = _large_last(ke, [0, E])
        o['g'] = o['g'] * _pow(ke)[:, None]
    elif cls == 'out_cancelling':      # hidden units in equal pairs (equal rows of w1, equal b1, no dropout), w2 in pairs (y, -(y + 1..3 ulp)), no b2, no uemb
        pairs = True
        o['w1'][1::2], o['b1'][1::2] = o['w1'][0::2], o['b1'][0::2]
        o['w2'][:, 1::2] = -np.sign(o['w2'][:, 0::2]) * _ulps(o['w2'][:, 0::2], rng)
        o['b2'][:] = 0
        if c['unc']:
            o['uemb'][:] = 0
    elif cls == 'lengths':
        # lengths from 0 across the whole table and beyond it: pos_a a small cluster, pos_b on rays of growing length; edge 0 joins two coincident points, edge 1 a
        # pair exactly `stop` apart
        o['pos_a'] = f(EEMB_NA, 3) * F32(0.125)
        ray = f(EEMB_NB, 3)
        ray = ray / np.sqrt((ray.astype(np.float64) ** 2).sum(1))[:, None].astype(F32)
        o['pos_b'] = (ray * np.linspace(0.0, 1.5 * stop, EEMB_NB).astype(F32)[:, None]).astype(F32)
        o['pos_b'][0] = o['pos_a'][0]
        o['pos_a'][1] = (0.5, 1.0, -2.0)
        o['pos_b'][1] = (0.5 + stop, 1.0, -2.0)
        o['idx_a'][0], o['idx_b'][0] = 0, 0
        if E > 1:
            o['idx_a'][1], o['idx_b'][1] = 1, 1
    else:
        raise ValueError(cls)
    _window(o, ('feat', 'sig', 'w1', 'b1', 'w2', 'b2', 'g') + (('lat_a', 'lat_b') if L else ()) + (('unc_a', 'uemb') if c['unc'] else ()))
    redraws = 0
    while True:      # the cap of ambiguous ReLU branches is 0: an offending unit's b1 is drawn again from the case's generator
        bad = np.nonzero(eemb_kinks(cfg, o).any(0))[0]
        if not len(bad):
            break
        for u in (sorted(set(int(b) // 2 * 2 for b in bad)) if pairs else bad):
            o['b1'][u] = _base(rng, 1)[0] * b1_scale[u]
            if pairs:
                o['b1'][u + 1] = o['b1'][u]
            redraws += 1
        assert redraws < 1000
    _window(o, ('b1',))
    _, d = _ee_geometry(FP64, o)
    assert np.all((d == 0) | (d > 1e-6))
    if cls == 'lengths':
        smear = ee_smear(FP64, o)
        assert d[0] == 0 and (E < 2 or d[1] == stop) and (E < 65 or (d.max() > 1.2 * stop and smear.min() < 2.0 ** -149 and smear.max() > 0.99))
        claims.update(zero_edge=0, stop_edge=1 if E > 1 else None)
    if cls == 'out_cancelling':
        p = 0.0
        keep, s, on = eemb_pattern(cfg, o, p, 0)
        ref, S = eemb_evaluate(FP64, cfg, o, keep, s, on)['emb'], eemb_evaluate(ABS, cfg, o, keep, s, on)['emb']
        assert np.all(np.abs(ref) <= 2.0 ** -18 * S) and (S > 0).any()
    o.update(claims=claims, redraws=redraws)
    return o


def eemb_locate(name, where, cfg):
    c = EEMB_CONFIGS[cfg]
    text = f'{name}{list(where)}'
    if name in ('emb', 'sh'):
        e = where[0]
        text += f': edge {e}: workgroup {e // 128}, wave {(e % 128) // 64}, lane {e % 64}; slice {e // SLICE} + {e % SLICE}; column {where[1]}'
    elif name == 'grad_w1':
        k, F = where[1], c['F']
        part = 'feat' if k < F else ('sig' if k < F + 32 else ('smearing' if k < F + 64 else ('lat_a' if k < F + 64 + c['L'] else 'lat_b')))
        text += f': unit {where[0]}, column {k} ({part})'
    elif name == 'grad_w2':
        text += f': column {where[0]}, unit {where[1]}'
    elif name in ('grad_lat_a', 'grad_lat_b'):
        text += f': node {where[0]}, latent column {where[1]}'
    else:
        text += f': unit / column {where[0]}'
    return text
