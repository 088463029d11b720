"""fp64 numpy restatement of the radial MLP's hidden layer from the edge embedding and the node table (include/ddk.h: ddk_rhid_forward /
ddk_rhid_backward; the cat of models/score_model.py:227-230 and fc[g][0..3] of models/tensor_layers.py:154):

    in[e]  = [ emb[e] | xs[src[e]] | xs[dst[e]] ]                    pre[e] = w1[g(e)] in[e] + b1[g(e)]
    h[e, c] = keep[e, c] ? max(pre[e, c], 0) * s : 0                 s = fp32(1) / (fp32(1) - fp32(p)), 1 for p == 0

and the mask layout DDK_RHID_MASK_LAYOUT 1 restated with tests/philox_ref.py.  The backward takes the zero pattern it differentiates through as an
argument (the device's own ``h != 0`` in the GPU tests: an fp32 pre-activation within rounding of zero may take the other branch than fp64)."""
import numpy as np

import philox_ref

MASK_TAG = 0x52484944      # DDK_RHID_MASK_TAG
H = 72
NS = 24


def scale(p):
    """s of include/ddk.h as the fp64 value of its fp32 expression"""
    return 1.0 if p == 0 else float(np.float32(1) / (np.float32(1) - np.float32(p)))


def keep_mask(seed, E, p, e0=0):
    """keep[e, c] for edges e0 .. e0 + E - 1: word c % 4 of Philox4x32-10(key = seed, counter = (e_lo, e_hi, c / 4, MASK_TAG)), kept iff its uniform >= p"""
    if p == 0:
        return np.ones((E, H), bool)
    seed = int(seed)
    e = (np.arange(E, dtype=np.uint64) + np.uint64(e0))[:, None]
    q = np.arange(H // 4, dtype=np.uint64)[None, :]
    words = philox_ref.philox4x32_10((e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), q, MASK_TAG), (seed & 0xFFFFFFFF, seed >> 32))      # [E, 18, 4]
    return philox_ref.uniform32(words).reshape(E, H) >= np.float32(p)


def rows(xs, src, dst, emb):
    """the concatenated row [E, 72] in fp64"""
    xs, emb = np.asarray(xs, np.float64), np.asarray(emb, np.float64)
    return np.concatenate([emb, xs[np.asarray(src)], xs[np.asarray(dst)]], axis=1)


def _groups(offsets):
    return [slice(int(offsets[g]), int(offsets[g + 1])) for g in range(len(offsets) - 1)]


def pre_activation(xs, src, dst, emb, offsets, w1, b1):
    """(pre [E, 72], margin [E, 72]): the pre-activation, and the classical bound of an fp32 dot product of 72 terms and a bias around it,
    72 * 2^-23 * (sum_i |w_i a_i| + |b|)"""
    a = rows(xs, src, dst, emb)
    w1, b1 = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    pre, mag = np.zeros((a.shape[0], H)), np.zeros((a.shape[0], H))
    for g, sl in enumerate(_groups(offsets)):
        pre[sl] = a[sl] @ w1[g].T + b1[g]
        mag[sl] = np.abs(a[sl]) @ np.abs(w1[g]).T + np.abs(b1[g])
    return pre, H * 2.0 ** -23 * mag


def forward(xs, src, dst, emb, offsets, w1, b1, keep=None, s=1.0):
    """h [E, 72] in fp64; keep: bool [E, 72] or None (everything kept)"""
    pre, _ = pre_activation(xs, src, dst, emb, offsets, w1, b1)
    h = np.maximum(pre, 0) * s
    return h if keep is None else np.where(keep, h, 0.0)


def backward(xs, src, dst, emb, offsets, w1, pattern, s, grad_h):
    """(grad_xs [N, 24], grad_emb [E, 24], grad_w1 [G, 72, 72], grad_b1 [G, 72]) in fp64 for the zero pattern ``pattern`` (bool [E, 72]: where h != 0)"""
    a = rows(xs, src, dst, emb)
    w1 = np.asarray(w1, np.float64)
    gpre = np.asarray(grad_h, np.float64) * np.where(pattern, s, 0.0)
    G = len(offsets) - 1
    gin, gw1, gb1 = np.zeros_like(a), np.zeros((G, H, H)), np.zeros((G, H))
    for g, sl in enumerate(_groups(offsets)):
        gin[sl] = gpre[sl] @ w1[g]
        gw1[g] = gpre[sl].T @ a[sl]
        gb1[g] = gpre[sl].sum(0)
    gxs = np.zeros((np.asarray(xs).shape[0], NS))
    np.add.at(gxs, np.asarray(src), gin[:, NS:2 * NS])
    np.add.at(gxs, np.asarray(dst), gin[:, 2 * NS:])
    return gxs, gin[:, :NS].copy(), gw1, gb1
