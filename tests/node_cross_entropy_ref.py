"""Host restatements of the AR model's ragged node cross-entropy (include/ddk.h: ddk_node_cross_entropy_batch; csrc/k_node_ce.hip) in numpy: per graph, over
the graph's ligand nodes followed by its receptor nodes,

    lse_s = m_s + log(sum exp(s_p - m_s))
    hard:  q = the lowest argmax of the teacher's column, loss = lse_s - s_q,             label_p = [p == q]
    soft:  p_t = softmax of the teacher's column,          loss = lse_s - sum p_t s_p,    label_p = p_t
    grad_logit_p = grad_g (exp(s_p - lse_s) - label_p)

``node_cross_entropy(..., dtype=np.float64)`` is the reference the device is measured against; ``dtype=np.float32`` evaluates the same expressions with every
intermediate in fp32 (numpy's own summation order), the host fp32 evaluation whose error against fp64 sets the bar.  Plain numpy, no torch, no device."""
import numpy as np


def graph_rows(table_l, table_r, lig_ptr, rec_ptr, g):
    """the rows of graph ``g``: its ligand rows followed by its receptor rows"""
    return np.concatenate([table_l[lig_ptr[g]:lig_ptr[g + 1]], table_r[rec_ptr[g]:rec_ptr[g + 1]]], axis=0)


def lowest_argmax(v):
    """the lowest position that holds the maximum (numpy's argmax returns the first occurrence)"""
    return int(np.argmax(v))


def graph_cross_entropy(s, t, soft, dtype=np.float64):
    """one graph: student logits ``s`` [n], teacher column ``t`` [n] -> (loss, softmax(s) - label [n], pick, target), every intermediate in ``dtype``"""
    s, t = np.asarray(s, dtype=dtype), np.asarray(t, dtype=dtype)
    pick, target = lowest_argmax(s), lowest_argmax(t)
    m = s.max()
    lse = m + np.log(np.exp(s - m).sum(dtype=dtype))
    if soft:
        mt = t.max()
        lse_t = mt + np.log(np.exp(t - mt).sum(dtype=dtype))
        label = np.exp(t - lse_t)
        loss = lse - (label * s).sum(dtype=dtype)
    else:
        label = np.zeros_like(s)
        label[target] = 1
        loss = lse - s[target]
    return dtype(loss), (np.exp(s - lse) - label).astype(dtype), pick, target


def node_cross_entropy(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft, grad=None, dtype=np.float64):
    """the collated batch: (loss [G], pick [G], target [G], grad_logit_l [n_lig], grad_logit_r [n_rec]) with ``grad`` [G] the upstream gradient of the
    losses (default: ones).  A graph without nodes keeps loss NaN and indices -1."""
    logit_l, logit_r = np.asarray(logit_l).reshape(-1), np.asarray(logit_r).reshape(-1)
    G = len(lig_ptr) - 1
    grad = np.ones(G, dtype) if grad is None else np.asarray(grad, dtype)
    loss = np.full(G, np.nan, dtype)
    pick, target = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    g_l, g_r = np.zeros(logit_l.shape[0], dtype), np.zeros(logit_r.shape[0], dtype)
    for g in range(G):
        s = graph_rows(logit_l, logit_r, lig_ptr, rec_ptr, g)
        if s.size == 0:
            continue
        t = graph_rows(teacher_l, teacher_r, lig_ptr, rec_ptr, g)[:, column[g]]
        loss[g], d, pick[g], target[g] = graph_cross_entropy(s, t, soft, dtype)
        d = (grad[g] * d).astype(dtype)
        n_l = lig_ptr[g + 1] - lig_ptr[g]
        g_l[lig_ptr[g]:lig_ptr[g + 1]], g_r[rec_ptr[g]:rec_ptr[g + 1]] = d[:n_l], d[n_l:]
    return loss, pick, target, g_l, g_r


def mask_input_latent(label_l, label_r, lig_ptr, rec_ptr, decoding_idx):
    """the input latent of an AR training item (autoregressive/dataset_ar.py:83-90): the label columns at or past the graph's decoding index are zeroed"""
    out_l, out_r = np.array(label_l, copy=True), np.array(label_r, copy=True)
    for g, k in enumerate(decoding_idx):
        out_l[lig_ptr[g]:lig_ptr[g + 1], k:] = 0
        out_r[rec_ptr[g]:rec_ptr[g + 1], k:] = 0
    return out_l, out_r
