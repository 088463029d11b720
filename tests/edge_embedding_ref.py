"""fp64 numpy restatement of one edge group's embedding in front of the conv stack and of its vector-Jacobian product for the four parameter tensors
(include/ddk.h: ddk_eemb_forward / ddk_eemb_backward; models/score_model.py:191-225 of the reference):

    vec[e] = pos_b[idx_b[e]] - pos_a[idx_a[e]]        d = |vec|
    row[e] = [ feat[e] (F = 0 or 4) | sig[sig_index[idx_a[e]]] (32) | exp(coeff (d - offset_j)^2) (32) ]
    hid[e, c] = keep[e, c] ? max(w1[c] . row[e] + b1[c], 0) * s : 0          s = fp32(1) / (fp32(1) - fp32(p)), 1 for p == 0
    emb[e] = w2 hid[e] + b2                             sh[e] = [1 | sqrt3 vec / max(d, 1e-12)]

``offset`` and ``coeff`` are the fp32 values the header states (torch.linspace's two-sided formula, GaussianSmearing's coeff), used in fp64.  The mask is
DDK_EEMB_MASK_LAYOUT 1 restated with tests/philox_ref.py."""
import numpy as np

import philox_ref

MASK_TAG = 0x45454D42      # DDK_EEMB_MASK_TAG
H = 24
D = 32
F32 = np.float32


def offsets(start, stop):
    """the 32 Gaussian centres as fp32 values: fmaf(step, j, start) below the middle, fmaf(-step, 31 - j, stop) above, step = (stop - start) / 31 in fp32
    (the product of two fp32 numbers is exact in fp64, so the fused operation is one fp64 sum rounded to fp32)"""
    start, stop = F32(start), F32(stop)
    step = np.float64((stop - start) / F32(D - 1))
    return np.array([F32(step * j + np.float64(start)) if j < D // 2 else F32(np.float64(stop) - step * (D - 1 - j)) for j in range(D)], F32)


def coeff(start, stop):
    off = offsets(start, stop)
    return float(F32(-0.5 / float(off[1] - off[0]) ** 2))


def scale(p):
    return 1.0 if p == 0 else float(F32(1) / (F32(1) - F32(p)))


def keep_mask(seed, E, p, e0=0):
    """keep[e, c] for edge positions e0 .. e0 + E - 1: word c % 4 of Philox4x32-10(key = seed, counter = (e_lo, e_hi, c / 4, MASK_TAG)), kept iff u >= p"""
    if p == 0:
        return np.ones((E, H), bool)
    seed = int(seed)
    e = (np.arange(E, dtype=np.uint64) + np.uint64(e0))[:, None]
    q = np.arange(H // 4, dtype=np.uint64)[None, :]
    words = philox_ref.philox4x32_10((e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), q, MASK_TAG), (seed & 0xFFFFFFFF, seed >> 32))      # [E, 6, 4]
    return philox_ref.uniform32(words).reshape(E, H) >= F32(p)


def geometry(pos_a, pos_b, idx_a, idx_b):
    vec = np.asarray(pos_b, np.float64)[np.asarray(idx_b)] - np.asarray(pos_a, np.float64)[np.asarray(idx_a)]
    return vec, np.sqrt((vec * vec).sum(1))


def spherical_harmonics(vec, d):
    return np.concatenate([np.ones((len(d), 1)), np.sqrt(3.0) * vec / np.maximum(d, 1e-12)[:, None]], 1)


def rows(o):
    """the row [E, K] in fp64 of the operands ``o`` (a dict: pos_a, pos_b, idx_a, idx_b, feat or None, sig, sig_index, start, stop)"""
    _, d = geometry(o['pos_a'], o['pos_b'], o['idx_a'], o['idx_b'])
    t = d[:, None] - offsets(o['start'], o['stop']).astype(np.float64)[None, :]
    parts = [np.asarray(o['sig'], np.float64)[np.asarray(o['sig_index'])[np.asarray(o['idx_a'])]], np.exp(coeff(o['start'], o['stop']) * t * t)]
    if o.get('feat') is not None:
        parts.insert(0, np.asarray(o['feat'], np.float64))
    return np.concatenate(parts, 1)


def smearing_uncertainty(o):
    """[E, 32]: what an fp32 evaluation may be off by in every smearing column: the edge length carries a few roundings of its own magnitude
    (4 * 2^-24 d: three differences, a sum of squares and a root), column j moves by |2 coeff t_j| exp(coeff t_j^2) per unit of d, the product
    coeff t^2 carries three roundings which the exponential turns into 3 * 2^-24 |coeff t^2| of the value, and expf adds 2^-22 of the value"""
    _, d = geometry(o['pos_a'], o['pos_b'], o['idx_a'], o['idx_b'])
    k = coeff(o['start'], o['stop'])
    t = d[:, None] - offsets(o['start'], o['stop']).astype(np.float64)[None, :]
    v = np.exp(k * t * t)
    return np.abs(2 * k * t) * v * (4 * 2.0 ** -24 * d)[:, None] + (3 * 2.0 ** -24 * np.abs(k * t * t) + 2.0 ** -22) * v


def pre_activation(o, w1, b1):
    """(pre [E, 24], margin [E, 24]): the pre-activation and a bound of what an fp32 chain may differ from it: the classical bound of a dot product of K
    terms and a bias, K * 2^-23 * (sum |w_i row_i| + |b|), plus the smearing columns' own uncertainty through their weights"""
    a = rows(o)
    w1, b1 = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    K = a.shape[1]
    pre = a @ w1.T + b1
    margin = K * 2.0 ** -23 * (np.abs(a) @ np.abs(w1).T + np.abs(b1)) + smearing_uncertainty(o) @ np.abs(w1[:, K - D:]).T
    return pre, margin


def forward(o, w1, b1, w2, b2, keep=None, s=1.0):
    """(emb [E, 24], sh [E, 4], hid [E, 24]) in fp64; keep: bool [E, 24] or None (everything kept)"""
    pre, _ = pre_activation(o, w1, b1)
    hid = np.maximum(pre, 0) * s
    if keep is not None:
        hid = np.where(keep, hid, 0.0)
    vec, d = geometry(o['pos_a'], o['pos_b'], o['idx_a'], o['idx_b'])
    return hid @ np.asarray(w2, np.float64).T + np.asarray(b2, np.float64), spherical_harmonics(vec, d), hid


def backward(o, w1, b1, w2, grad_emb, keep=None, s=1.0, passes=None):
    """(grad_w1 [24, K], grad_b1 [24], grad_w2 [24, 24], grad_b2 [24]) in fp64.  passes: bool [E, 24], where the ReLU passes (None: pre > 0, the fp64
    pattern; a caller overrides it on the elements within fp32 rounding of zero)"""
    a = rows(o)
    pre, _ = pre_activation(o, w1, b1)
    on = pre > 0 if passes is None else np.asarray(passes, bool)
    if keep is not None:
        on = on & keep
    hid = np.where(on, pre * s, 0.0)
    g = np.asarray(grad_emb, np.float64)
    gpre = (g @ np.asarray(w2, np.float64)) * np.where(on, s, 0.0)
    return gpre.T @ a, gpre.sum(0), g.T @ hid, g.sum(0)
