"""The all-atom (confidence) family of the radial tensor product restated in numpy, fp64: the closed form that csrc/k_rtp.hip implements for the ids
DDK_TP_AA + l, read from ``runtime.tp_layer_shape_aa``'s table (blocks, instruction offsets, kinds, scales) and nothing else.  tests/test_confidence_conv_host.py
holds it against ``oracle.e3nn_lite.FullyConnectedTensorProduct``; the GPU tests hold the kernels against it.

A path (one e3nn instruction) takes the input irrep's rows I [E, mul_in, d_in], the sh row [E, 9] = [Y0 | Y1 | Y2] and its weight matrix
w [E, mul_in, mul_out] to  out[e, o, k] += scale * sum_u w[e, u, o] * U[e, u, k],  U[e, u, k] = sum_{a, j} T_kind[a, j, k] I[e, u, a] sh[e, j]:
every kind is one constant tensor T [d_in, 9, d_out], so the output and all gradients are einsums."""
import numpy as np

from disco_diffdock_amd.runtime import tp_layer_shape_aa

S3 = np.sqrt(3.0)


def _kind_tensors():
    T = {k: np.zeros((d_in, 9, d_out)) for k, (d_in, d_out) in dict(ss=(1, 1), sv=(1, 3), vs=(3, 3), vd=(3, 1), vx=(3, 3), v2=(3, 3)).items()}
    T['ss'][0, 0, 0] = 1.0                      # i Y0
    for k in range(3):
        T['sv'][0, 1 + k, k] = 1.0              # i Y1
        T['vs'][k, 0, k] = 1.0                  # i Y0
        T['vd'][k, 1 + k, 0] = 1.0              # i . Y1
    for a, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):      # i x Y1
        T['vx'][a, 1 + j, k], T['vx'][j, 1 + a, k] = 1.0, -1.0
    # M(Y2) i with M = [[-y2/sqrt3 - y4, y1, y0], [y1, 2 y2/sqrt3, y3], [y0, y3, -y2/sqrt3 + y4]], y = sh[4:9]; T[a, 4 + m, k] = dM[k, a] / dy_m
    M = np.zeros((5, 3, 3))
    M[0, 0, 2] = M[0, 2, 0] = M[1, 0, 1] = M[1, 1, 0] = M[3, 1, 2] = M[3, 2, 1] = 1.0
    M[2, 0, 0], M[2, 1, 1], M[2, 2, 2] = -1 / S3, 2 / S3, -1 / S3
    M[4, 0, 0], M[4, 2, 2] = -1.0, 1.0
    for m in range(5):
        T['v2'][:, 4 + m, :] = M[m].T
    return T


KIND = _kind_tensors()
DIMS = {'0e': 1, '1o': 3, '1e': 3, '0o': 1}


def shape(l):
    return tp_layer_shape_aa(l)


def in_slices(s):
    """the irrep slices of a node row [din] that exist, by name"""
    mul = dict(zip(('0e', '1o', '1e', '0o'), (s['A'], s['P'], s['Q'], s['C'])))
    out, off = {}, 0
    for ir, m in mul.items():
        if m:
            out[ir] = slice(off, off + m * DIMS[ir])
        off += m * DIMS[ir]
    return out


def out_slices(s):
    out, off = {}, 0
    for ir, m in zip(('0e', '1o', '1e', '0o'), s['O']):
        if m:
            out[ir] = slice(off, off + m * DIMS[ir])
        off += m * DIMS[ir]
    return out


def weight_slices(s):
    """each e3nn instruction's slice of the flat weight row, by name 'in.sh.out'"""
    return {f"{p['ir_in']}.{p['ir_sh']}.{p['ir_out']}": slice(p['offset'], p['offset'] + p['mul_in'] * p['mul_out']) for p in s['paths']}


def _path_views(p, x, w):
    E = x.shape[0]
    I = x[:, p['xoff']:p['xoff'] + p['mul_in'] * DIMS[p['ir_in']]].reshape(E, p['mul_in'], DIMS[p['ir_in']])
    wp = w[:, p['offset']:p['offset'] + p['mul_in'] * p['mul_out']].reshape(E, p['mul_in'], p['mul_out'])
    return I, wp


def tp(l, x, sh, w, g=None):
    """out [E, dout] of per-edge weights w [E, W]; with g [E, dout] also the gradients dict(x, sh, w).  fp64."""
    s = shape(l)
    x, sh, w = (np.asarray(a, np.float64) for a in (x, sh, w))
    E = x.shape[0]
    out = np.zeros((E, s['dout']))
    grads = None if g is None else dict(x=np.zeros_like(x), sh=np.zeros_like(sh), w=np.zeros_like(w))
    for p in s['paths']:
        T, d_out = KIND[p['kind']], DIMS[p['ir_out']]
        I, wp = _path_views(p, x, w)
        U = np.einsum('ajk,eua,ej->euk', T, I, sh)
        osl = slice(p['ooff'], p['ooff'] + p['mul_out'] * d_out)
        out[:, osl] += p['scale'] * np.einsum('euo,euk->eok', wp, U).reshape(E, -1)
        if g is not None:
            G = np.asarray(g, np.float64)[:, osl].reshape(E, p['mul_out'], d_out)
            grads['w'][:, p['offset']:p['offset'] + p['mul_in'] * p['mul_out']] += p['scale'] * np.einsum('euk,eok->euo', U, G).reshape(E, -1)
            gU = p['scale'] * np.einsum('euo,eok->euk', wp, G)
            grads['x'][:, p['xoff']:p['xoff'] + p['mul_in'] * DIMS[p['ir_in']]] += np.einsum('ajk,ej,euk->eua', T, sh, gU).reshape(E, -1)
            grads['sh'] += np.einsum('ajk,eua,euk->ej', T, I, gU)
    return (out, grads) if g is not None else out


def _groups(offsets):
    return [(k, offsets[k], offsets[k + 1]) for k in range(len(offsets) - 1)]


def rtp(l, x, sh, h, offsets, w2, b2, g):
    """the radial tensor product: w_e = w2[group(e)] h_e + b2[group(e)].  (out, dict(x, sh, h, w2, b2)), fp64"""
    x, sh, h, w2, b2, g = (np.asarray(a, np.float64) for a in (x, sh, h, w2, b2, g))
    w = np.zeros((x.shape[0], w2.shape[1]))
    for k, a, b in _groups(offsets):
        w[a:b] = h[a:b] @ w2[k].T + b2[k]
    out, gr = tp(l, x, sh, w, g)
    gh, gw2, gb2 = np.zeros_like(h), np.zeros_like(w2), np.zeros_like(b2)
    for k, a, b in _groups(offsets):
        gh[a:b] = gr['w'][a:b] @ w2[k]
        gw2[k] = gr['w'][a:b].T @ h[a:b]
        gb2[k] = gr['w'][a:b].sum(0)
    return out, dict(x=gr['x'], sh=gr['sh'], h=gh, w2=gw2, b2=gb2)


def rconv(l, x_nodes, src, dst, n_out, sh, h, offsets, w2, b2, g_nodes):
    """the radial conv: scatter-mean over src of rtp(x_nodes[dst]).  (out_nodes, dict(x, sh, h, w2, b2)), fp64"""
    x_nodes, g_nodes = np.asarray(x_nodes, np.float64), np.asarray(g_nodes, np.float64)
    src, dst = np.asarray(src), np.asarray(dst)
    cnt = np.maximum(np.bincount(src, minlength=n_out)[:n_out], 1).astype(np.float64)
    out_e, gr = rtp(l, x_nodes[dst], sh, h, offsets, w2, b2, (g_nodes / cnt[:, None])[src])
    out = np.zeros((n_out, out_e.shape[1]))
    np.add.at(out, src, out_e)
    gx = np.zeros_like(x_nodes)
    np.add.at(gx, dst, gr['x'])
    return out / cnt[:, None], dict(gr, x=gx)


def layer_fp64(params, l, bn, training, send, recv, ei, sh, emb=None, edge_attr=None):
    """The all-atom TensorProductConvLayer in fp64 torch autograd through this module's closed form (all_atom_score_model.py:36-50): ``params``: the
    layer's state dict as fp64 tensors (the parameters require grad), ``send`` [n_in, din] and ``recv`` [n_out, >= 24] fp64 tensors, ``ei`` [2, E] (row 0
    receivers), ``sh`` [E, 9].  ``emb`` [E, 24]: the embedded form, rows [emb | recv[ei[0], :24] | send[ei[1], :24]]; else ``edge_attr`` [E, 72].
    BatchNorm always (zero edges too), on the batch statistics in training.  Returns (out [n_out, dout], (mean, var) that move the buffers or None)."""
    import torch
    s = shape(l)
    E, n_out = ei.shape[1], recv.shape[0]
    if emb is not None:
        edge_attr = torch.cat([emb, recv[ei[0], :24], send[ei[1], :24]], 1)
    if E:
        hid = torch.relu(edge_attr @ params['fc.0.weight'].T + params['fc.0.bias'])
        w = hid @ params['fc.3.weight'].T + params['fc.3.bias']
        xg = send[ei[1]]
        outs = torch.zeros((E, s['dout']), dtype=torch.float64)
        for p in s['paths']:
            T, d_in, d_out = torch.from_numpy(KIND[p['kind']]), DIMS[p['ir_in']], DIMS[p['ir_out']]
            I = xg[:, p['xoff']:p['xoff'] + p['mul_in'] * d_in].reshape(E, p['mul_in'], d_in)
            wp = w[:, p['offset']:p['offset'] + p['mul_in'] * p['mul_out']].reshape(E, p['mul_in'], p['mul_out'])
            U = torch.einsum('ajk,eua,ej->euk', T, I, sh)
            piece = p['scale'] * torch.einsum('euo,euk->eok', wp, U).reshape(E, -1)
            outs = torch.cat([outs[:, :p['ooff']], outs[:, p['ooff']:p['ooff'] + p['mul_out'] * d_out] + piece, outs[:, p['ooff'] + p['mul_out'] * d_out:]], 1)
        cnt = torch.bincount(ei[0], minlength=n_out).clamp(min=1).double()
        out = torch.zeros((n_out, s['dout']), dtype=torch.float64).index_add(0, ei[0], outs) / cnt[:, None]
    else:
        out = torch.zeros((n_out, s['dout']), dtype=torch.float64)
    if not bn:
        return out, None
    pieces, stats_m, stats_v, iw, ib = [], [], [], 0, 0
    for ir, sl in out_slices(s).items():
        d = DIMS[ir]
        mul = (sl.stop - sl.start) // d
        f = out[:, sl].reshape(-1, mul, d)
        if ir == '0e':
            mean = f.mean(dim=(0, 2)) if training else params['batch_norm.running_mean'][ib:ib + mul]
            stats_m.append(mean.detach())
            f = f - mean.reshape(1, mul, 1)
        var = f.pow(2).mean(-1).mean(0) if training else params['batch_norm.running_var'][iw:iw + mul]
        stats_v.append(var.detach())
        f = f * ((var + 1e-5).pow(-0.5) * params['batch_norm.weight'][iw:iw + mul]).reshape(1, mul, 1)
        if ir == '0e':
            f = f + params['batch_norm.bias'][ib:ib + mul].reshape(1, mul, 1)
            ib += mul
        iw += mul
        pieces.append(f.reshape(-1, mul * d))
    return torch.cat(pieces, 1), (torch.cat(stats_m), torch.cat(stats_v))


def auc_pairs(y, score):
    """ROC AUC by brute-force pair counting: P(score_pos > score_neg) + P(tie) / 2; 0 with one class present (the reference's ``except``)"""
    y, score = np.asarray(y).astype(bool), np.asarray(score, np.float64)
    pos, neg = score[y], score[~y]
    if pos.size == 0 or neg.size == 0:
        return 0.0
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (pos.size * neg.size))
