"""Restatements the latent-conditioned (DisCo) training ops are measured against (include/ddk.h: ddk_eemb_latent_forward / ddk_eemb_latent_backward,
ddk_gumbel_softmax_batch / ddk_gumbel_softmax_batch_backward, ddk_rng_latent_keep), on top of tests/edge_embedding_ref.py and tests/philox_ref.py.

The edge embedding with latent columns, for edge e with ia = idx_a[e], ib = idx_b[e]:

    row[e] = [ edge_embedding_ref.rows | lat_a[ia] (L) | lat_b[ib] (L) ]      (zeros with zero_latent)         K = F + 64 + 2 L
    hid, emb as edge_embedding_ref;   emb[e] += unc_a[ia] * uemb   where unc_a is given

``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` runs the same expressions on fp32 arrays (numpy's own summation order): the host's fp32
evaluation whose distance from fp64, err32, sets a test's bar.

The Gumbel softmax: per graph and latent dimension over the graph's ligand nodes followed by its receptor nodes, from the uniforms of DDK_GUMBEL_LAYOUT 1
(``gumbel_uniforms``, bit-exact)."""
import numpy as np

import edge_embedding_ref as ref
import philox_ref

GUMBEL_TAG = 0x47554D42      # DDK_GUMBEL_TAG
GUMBEL_PURPOSE, KEEP_PURPOSE = 13, 12
F32 = np.float32


# ---- the edge embedding with latent columns ----------------------------------------------------------------------------------------------------------------------
def rows(o, L, dtype=np.float64):
    """the row [E, K + 2 L]; ``o``: the operands of edge_embedding_ref.rows plus lat_a [Na, L], lat_b [Nb, L] (ignored with o['zero_latent'])"""
    base = ref.rows(o)
    E = base.shape[0]
    if o.get('zero_latent'):
        lat = np.zeros((E, 2 * L))
    else:
        lat = np.concatenate([np.asarray(o['lat_a'], np.float64)[np.asarray(o['idx_a'])], np.asarray(o['lat_b'], np.float64)[np.asarray(o['idx_b'])]], 1)
    assert lat.shape == (E, 2 * L)
    return np.concatenate([base, lat], 1).astype(dtype)


def pre_activation(o, w1, b1, L):
    """(pre [E, 24], margin [E, 24]) in fp64: edge_embedding_ref.pre_activation's bound with the latent columns in the dot product"""
    a = rows(o, L)
    w1, b1 = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    K = a.shape[1]
    pre = a @ w1.T + b1
    K0 = K - 2 * L
    margin = K * 2.0 ** -23 * (np.abs(a) @ np.abs(w1).T + np.abs(b1)) + ref.smearing_uncertainty(o) @ np.abs(w1[:, K0 - ref.D:K0]).T
    return pre, margin


def forward(o, P, L, keep=None, s=1.0, dtype=np.float64):
    """emb [E, 24] in ``dtype``; P: w1 [24, K + 2 L], b1, w2, b2 and, for the unconditional term, uemb [24] with o['unc_a'] [Na]"""
    c = lambda x: np.asarray(x, np.float64).astype(dtype)
    a = rows(o, L, dtype)
    pre = a @ c(P['w1']).T + c(P['b1'])
    hid = np.maximum(pre, 0) * dtype(s)
    if keep is not None:
        hid = np.where(keep, hid, dtype(0))
    emb = hid @ c(P['w2']).T + c(P['b2'])
    if o.get('unc_a') is not None:
        emb = emb + c(o['unc_a'])[np.asarray(o['idx_a'])][:, None] * c(P['uemb'])[None, :]
    return emb


def backward(o, P, L, grad_emb, keep=None, s=1.0, passes=None, dtype=np.float64):
    """dict(grad_w1 [24, K + 2 L], grad_b1, grad_w2, grad_b2, grad_uemb [24], grad_lat_a [Na, L], grad_lat_b [Nb, L]) in ``dtype``.  ``passes``: where the
    ReLU passes (None: this dtype's own pre > 0)"""
    c = lambda x: np.asarray(x, np.float64).astype(dtype)
    a = rows(o, L, dtype)
    w1 = c(P['w1'])
    pre = a @ w1.T + c(P['b1'])
    on = pre > 0 if passes is None else np.asarray(passes, bool)
    if keep is not None:
        on = on & keep
    hid = np.where(on, pre * dtype(s), dtype(0))
    g = c(grad_emb)
    gpre = (g @ c(P['w2'])) * np.where(on, dtype(s), dtype(0))
    ia, ib = np.asarray(o['idx_a']), np.asarray(o['idx_b'])
    n_a, n_b = len(o['pos_a']), len(o['pos_b'])
    out = dict(grad_w1=gpre.T @ a, grad_b1=gpre.sum(0), grad_w2=g.T @ hid, grad_b2=g.sum(0))
    unc = np.zeros(n_a, dtype) if o.get('unc_a') is None else c(o['unc_a'])
    out['grad_uemb'] = (unc[ia][:, None] * g).sum(0)
    K0 = a.shape[1] - 2 * L
    glat = gpre @ w1[:, K0:]      # [E, 2 L]
    ga, gb = np.zeros((n_a, L), dtype), np.zeros((n_b, L), dtype)
    if not o.get('zero_latent'):
        np.add.at(ga, ia, glat[:, :L])
        np.add.at(gb, ib, glat[:, L:])
    else:
        out['grad_w1'][:, K0:] = 0
    out['grad_lat_a'], out['grad_lat_b'] = ga, gb
    return out


NAMES = ('grad_w1', 'grad_b1', 'grad_w2', 'grad_b2', 'grad_uemb', 'grad_lat_a', 'grad_lat_b')


# ---- the noise of DDK_GUMBEL_LAYOUT 1 and the keep flag --------------------------------------------------------------------------------------------------------
def gumbel_uniforms(seed, stream, sample, draw, d, n):
    """u [n] in fp32, bit-exact: purpose 13 with counter (stream, sample, 13 << 28 | draw << 8 | d) yields four words, words 0 and 1 key a second
    Philox4x32-10 whose counter (pos / 4, 0, 0, GUMBEL_TAG) gives position pos the word pos % 4"""
    key = philox_ref.block(seed, stream, sample, GUMBEL_PURPOSE, draw, d)
    quads = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox_ref.philox4x32_10((quads, 0, 0, GUMBEL_TAG), (int(key[0]), int(key[1])))      # [quads, 4]
    return philox_ref.uniform32(words).reshape(-1)[:n]


def latent_keep(seed, streams, rate, draw=0, sample=0):
    """keep [n] as 1.0 / 0.0: purpose 12, step = draw, block 0, word 0, kept iff u >= rate in fp32"""
    u = np.array([philox_ref.uniform32(philox_ref.block(seed, st, sample, KEEP_PURPOSE, draw, 0))[0] for st in streams], F32)
    return (u >= F32(rate)).astype(F32)


def gumbel_noise(u, dtype=np.float64):
    """-log(-log(u + 1e-20) + 1e-20) from the fp32 uniforms, the additions in fp32 as on the device (u + 1e-20f is u unless u == 0)"""
    inner = (np.asarray(u, F32) + F32(1e-20)).astype(dtype)
    return -np.log(-np.log(inner) + dtype(1e-20))


def gumbel_forward(logits, u, T, dtype=np.float64):
    """one (graph, dimension): logits [n] over the graph's ligand then receptor nodes, u [n] -> (out [n], y [n], argmax): y = softmax((logits + gum) / T),
    out = (hard - y) + y with hard the one-hot at the lowest index of the maximum of y"""
    z = ((np.asarray(logits, np.float64).astype(dtype) + gumbel_noise(u, dtype)) / dtype(T)).astype(dtype)
    e = np.exp(z - z.max())
    y = (e / e.sum()).astype(dtype)
    k = int(np.argmax(y))      # (numpy's argmax: the first of equals)
    hard = np.zeros_like(y)
    hard[k] = 1
    return (hard - y) + y, y, k


def gumbel_backward(y, grad_out, T, dtype=np.float64):
    """grad_logit = y (g - sum g y) / T"""
    y, g = np.asarray(y, np.float64).astype(dtype), np.asarray(grad_out, np.float64).astype(dtype)
    return (y * (g - (g * y).sum()) / dtype(T)).astype(dtype)
