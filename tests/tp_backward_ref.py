"""The vector-Jacobian product of FasterTensorProduct.forward (reference models/tensor_layers.py:65-116) in closed form, fp64 numpy: the
specification ddk_tp_backward is written against (tests/golden/faster_tp_backward_l*.npz, made by autograd of the unmodified reference class, decide
whether this text is right: tests/test_tp_backward_host.py).

Input multiplicities A, P, Q, C of 0e, 1o, 1e, 0o; output multiplicities O0..O3; weight block k has R_k rows, R = (A+P, A+P+Q, P+Q+C, Q+C), and is
scaled by rs_k = 1/sqrt(R_k); a block with O_k = 0 has no elements.  With s0, v = sh and the pre-weight rows

    U0 = [a s0 ; (p.v)/sqrt3]    U1 = [a v ; p s0 ; (q x v)/sqrt2]    U2 = [(p x v)/sqrt2 ; q s0 ; c v]    U3 = [(q.v)/sqrt3 ; c s0]

    grad_w block k [r, c] = rs_k U_k[r] . g_k[c]         G_k[r] = rs_k sum_c W_k[r, c] g_k[c]
    grad_a[i] = s0 G0[i] + v.G1[i]
    grad_p[i] = v G0[A+i]/sqrt3 + s0 G1[A+i] + (v x G2[i])/sqrt2
    grad_q[i] = (v x G1[A+P+i])/sqrt2 + s0 G2[P+i] + v G3[i]/sqrt3
    grad_c[i] = v.G2[P+Q+i] + s0 G3[Q+i]
    grad_s0, grad_v: the same products summed over i against a, p, q, c
"""
import numpy as np

# (A, P, Q, C) -> (O0, O1, O2, O3) of the score model's conv layers (ns = 24, nv = 6; layers 3 and 4 share a shape)
LAYER_MULS = [((24, 0, 0, 0), (24, 6, 0, 0)), ((24, 6, 0, 0), (24, 6, 6, 0)), ((24, 6, 6, 0), (24, 6, 6, 24)), ((24, 6, 6, 24), (24, 6, 6, 24)),
              ((24, 6, 6, 24), (24, 6, 6, 24))]


def shape(layer):
    """dict of the layer's sizes: multiplicities, rows R, block offsets B in the weight row, W, Din, Dout"""
    (A, P, Q, C), O = LAYER_MULS[layer]
    R = [A + P if O[0] else 0, A + P + Q if O[1] else 0, P + Q + C if O[2] else 0, Q + C if O[3] else 0]
    B = [0]
    for k in range(4):
        B.append(B[-1] + R[k] * O[k])
    return dict(A=A, P=P, Q=Q, C=C, O=O, R=R, B=B, W=B[4], din=A + 3 * P + 3 * Q + C, dout=O[0] + 3 * O[1] + 3 * O[2] + O[3])


def weight_blocks(layer):
    """[(name, slice of the weight row)] of the blocks that have elements"""
    s = shape(layer)
    return [(f'block{k}', slice(s['B'][k], s['B'][k + 1])) for k in range(4) if s['B'][k + 1] > s['B'][k]]


def input_slices(layer):
    """[(irrep name, slice of the node row)] of the input irreps that are present"""
    s = shape(layer)
    A, P, Q, C = s['A'], s['P'], s['Q'], s['C']
    out = [('0e', slice(0, A)), ('1o', slice(A, A + 3 * P)), ('1e', slice(A + 3 * P, A + 3 * P + 3 * Q)), ('0o', slice(A + 3 * P + 3 * Q, s['din']))]
    return [(n, sl) for n, sl in out if sl.stop > sl.start]


def _split(layer, x, sh, g):
    s = shape(layer)
    A, P, Q, C, O = s['A'], s['P'], s['Q'], s['C'], s['O']
    E = x.shape[0]
    a, p = x[:, :A], x[:, A:A + 3 * P].reshape(E, P, 3)
    q, c = x[:, A + 3 * P:A + 3 * P + 3 * Q].reshape(E, Q, 3), x[:, A + 3 * P + 3 * Q:]
    o1, o2 = O[0] + 3 * O[1], O[0] + 3 * O[1] + 3 * O[2]
    gs = [g[:, :O[0]], g[:, O[0]:o1].reshape(E, O[1], 3), g[:, o1:o2].reshape(E, O[2], 3), g[:, o2:]]
    return s, a, p, q, c, sh[:, 0], sh[:, 1:4], gs


def _rows(a, p, q, c, s0, v):
    """U0 [E, A+P], U1 [E, A+P+Q, 3], U2 [E, P+Q+C, 3], U3 [E, Q+C]"""
    vv, ss = v[:, None, :], s0[:, None, None]
    cr = lambda t: np.cross(t, np.broadcast_to(vv, t.shape)) / np.sqrt(2.0)
    U0 = np.concatenate([a * s0[:, None], (p * vv).sum(-1) / np.sqrt(3.0)], 1)
    U1 = np.concatenate([a[:, :, None] * vv, p * ss, cr(q)], 1)
    U2 = np.concatenate([cr(p), q * ss, c[:, :, None] * vv], 1)
    U3 = np.concatenate([(q * vv).sum(-1) / np.sqrt(3.0), c * s0[:, None]], 1)
    return U0, U1, U2, U3


def forward(layer, x, sh, w):
    """out [E, Dout] (fp64): the forward itself, for the adjoint identities"""
    x, sh, w = (np.asarray(t, np.float64) for t in (x, sh, w))
    s, a, p, q, c, s0, v, _ = _split(layer, x, sh, np.zeros((x.shape[0], shape(layer)['dout'])))
    U, E, out = _rows(a, p, q, c, s0, v), x.shape[0], []
    for k in range(4):
        R, O = s['R'][k], s['O'][k]
        if R * O == 0:
            continue
        Wk = w[:, s['B'][k]:s['B'][k + 1]].reshape(E, R, O) / np.sqrt(R)
        out.append(np.einsum('er,erc->ec', U[k], Wk) if k in (0, 3) else np.einsum('erx,erc->ecx', U[k], Wk).reshape(E, -1))
    return np.concatenate(out, 1)


def backward(layer, x, sh, w, grad_out):
    """(grad_x [E, Din], grad_sh [E, 4], grad_w [E, W]) in fp64"""
    x, sh, w, g = (np.asarray(t, np.float64) for t in (x, sh, w, grad_out))
    s, a, p, q, c, s0, v, gs = _split(layer, x, sh, g)
    A, P, Q, C = s['A'], s['P'], s['Q'], s['C']
    E = x.shape[0]
    U = _rows(a, p, q, c, s0, v)
    grad_w = np.zeros((E, s['W']))
    G = [np.zeros((E, A + P)), np.zeros((E, A + P + Q, 3)), np.zeros((E, P + Q + C, 3)), np.zeros((E, Q + C))]      # zero where the block is absent
    for k in range(4):
        R, O = s['R'][k], s['O'][k]
        if R * O == 0:
            continue
        rs = 1.0 / np.sqrt(R)
        Wk = w[:, s['B'][k]:s['B'][k + 1]].reshape(E, R, O)
        if k in (0, 3):
            grad_w[:, s['B'][k]:s['B'][k + 1]] = (rs * U[k][:, :, None] * gs[k][:, None, :]).reshape(E, -1)
            G[k] = rs * np.einsum('erc,ec->er', Wk, gs[k])
        else:
            grad_w[:, s['B'][k]:s['B'][k + 1]] = (rs * np.einsum('erx,ecx->erc', U[k], gs[k])).reshape(E, -1)
            G[k] = rs * np.einsum('erc,ecx->erx', Wk, gs[k])
    G0, G1, G2, G3 = G
    vv, ss = v[:, None, :], s0[:, None, None]
    s3, s2 = np.sqrt(3.0), np.sqrt(2.0)
    vx = lambda t: np.cross(np.broadcast_to(vv, t.shape), t)      # v x t
    grad_a = s0[:, None] * G0[:, :A] + (vv * G1[:, :A]).sum(-1)
    grad_p = vv * G0[:, A:A + P, None] / s3 + ss * G1[:, A:A + P] + vx(G2[:, :P]) / s2
    grad_q = vx(G1[:, A + P:A + P + Q]) / s2 + ss * G2[:, P:P + Q] + vv * G3[:, :Q, None] / s3
    grad_c = (vv * G2[:, P + Q:P + Q + C]).sum(-1) + s0[:, None] * G3[:, Q:Q + C]
    grad_x = np.concatenate([grad_a, grad_p.reshape(E, -1), grad_q.reshape(E, -1), grad_c], 1)
    grad_s0 = (a * G0[:, :A]).sum(1) + (p * G1[:, A:A + P]).sum((1, 2)) + (q * G2[:, P:P + Q]).sum((1, 2)) + (c * G3[:, Q:Q + C]).sum(1)
    grad_v = ((a[:, :, None] * G1[:, :A]).sum(1) + (p * G0[:, A:A + P, None]).sum(1) / s3 + np.cross(G2[:, :P], p).sum(1) / s2
              + np.cross(G1[:, A + P:A + P + Q], q).sum(1) / s2 + (q * G3[:, :Q, None]).sum(1) / s3 + (c[:, :, None] * G2[:, P + Q:P + Q + C]).sum(1))
    return grad_x, np.concatenate([grad_s0[:, None], grad_v], 1), grad_w
