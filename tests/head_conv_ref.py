"""fp64 numpy closed form of the two head convolutions of the score model and of their vector-Jacobian product (include/ddk.h: ddk_hconv_forward /
ddk_hconv_backward; csrc/k_hconv.hip), written out from the pre-weight rows and scales of e3nn's FullyConnectedTensorProduct for

* head 0, the centre head ``final_conv``:   in (x) '1x0e + 1x1o' -> '2x1o + 2x1e', W = 144, K = 48
* head 1, the torsion head ``tor_bond_conv``: in (x) (., T) -> '24x0o + 24x0e', W = 288, K = 72, T the 1o block of FullTensorProduct('1x0e + 1x1o', '2e')

with ``in`` = [a 24x0e | p 6x1o | q 6x1e | c 24x0o].  tests/test_head_conv_host.py checks it against fp64 autograd of oracle/e3nn_lite.py."""
import numpy as np

S6 = np.sqrt(3.0 / 36.0) / np.sqrt(3.0)       # path coefficient sqrt(3/36) times w3j(0,1,1) = w3j(1,0,1) = delta / sqrt3
S72 = np.sqrt(3.0 / 36.0) / np.sqrt(6.0)      # ... times w3j(1,1,1) = epsilon / sqrt6
S18 = np.sqrt(1.0 / 6.0) / np.sqrt(3.0)       # path coefficient sqrt(1/6) times w3j(1,1,0) = delta / sqrt3

K = (48, 72)
W = (144, 288)
DOUT = (12, 48)
DIN = 84
X_SLICES = {'0e': slice(0, 24), '1o': slice(24, 42), '1e': slice(42, 60), '0o': slice(60, 84)}
OUT_SLICES = ({'1o': slice(0, 6), '1e': slice(6, 12)}, {'0o': slice(0, 24), '0e': slice(24, 48)})
# the weight blocks in e3nn's instruction order: name -> (offset, rows, columns, output irrep)
CENTER_BLOCKS = {'A': (0, 24, 2, '1o'), 'B': (48, 6, 2, '1o'), 'C': (60, 6, 2, '1e'), 'D': (72, 6, 2, '1e'), 'E': (84, 6, 2, '1o'), 'F': (96, 24, 2, '1e')}
TORSION_BLOCKS = {'P': (0, 6, 24, '0e'), 'Q': (144, 6, 24, '0o')}
BLOCKS = (CENTER_BLOCKS, TORSION_BLOCKS)


def weight_slices(head):
    """name -> slice of the weight row, one per weight block"""
    return {n: slice(o, o + r * c) for n, (o, r, c, _) in BLOCKS[head].items()}


def _parts(xe):
    return xe[:, :24], xe[:, 24:42].reshape(-1, 6, 3), xe[:, 42:60].reshape(-1, 6, 3), xe[:, 60:]


def _center_rows(xe, sh):
    """name -> the pre-weight rows [E, rows, 3] of the block, scaled"""
    a, p, q, c = _parts(xe)
    s0, v = sh[:, 0][:, None, None], sh[:, None, 1:4]
    return {'A': a[:, :, None] * v * S6, 'B': p * s0 * S6, 'C': np.cross(p, v) * S72, 'D': q * s0 * S6, 'E': np.cross(q, v) * S72, 'F': c[:, :, None] * v * S6}


def tp_rows(head, xe, sh, w):
    """the tensor product per edge: xe [E, 84] (the gathered node rows), sh [E, 4], w [E, W] -> [E, dout]"""
    E = xe.shape[0]
    if head == 0:
        U = _center_rows(xe, sh)
        o = {'1o': np.zeros((E, 2, 3)), '1e': np.zeros((E, 2, 3))}
        for n, (off, r, c, io) in CENTER_BLOCKS.items():
            o[io] += np.einsum('erk,erc->eck', U[n], w[:, off:off + r * c].reshape(E, r, c))
        return np.concatenate([o['1o'].reshape(E, 6), o['1e'].reshape(E, 6)], 1)
    _, p, q, _ = _parts(xe)
    T = sh[:, 1:4]
    up, uq = np.einsum('erk,ek->er', p, T) * S18, np.einsum('erk,ek->er', q, T) * S18
    o0e = np.einsum('er,erc->ec', up, w[:, :144].reshape(E, 6, 24))
    o0o = np.einsum('er,erc->ec', uq, w[:, 144:].reshape(E, 6, 24))
    return np.concatenate([o0o, o0e], 1)


def tp_vjp(head, xe, sh, w, ge):
    """(grad_xe [E, 84], grad_w [E, W]) of tp_rows for the per-edge gradient rows ge [E, dout]"""
    E = xe.shape[0]
    gxe, gw = np.zeros((E, DIN)), np.zeros((E, W[head]))
    if head == 0:
        U = _center_rows(xe, sh)
        s0, v = sh[:, 0][:, None, None], sh[:, None, 1:4]
        g = {'1o': ge[:, :6].reshape(E, 2, 3), '1e': ge[:, 6:].reshape(E, 2, 3)}
        ga, gp, gq, gc = np.zeros((E, 24)), np.zeros((E, 6, 3)), np.zeros((E, 6, 3)), np.zeros((E, 24))
        for n, (off, r, c, io) in CENTER_BLOCKS.items():
            wb = w[:, off:off + r * c].reshape(E, r, c)
            gw[:, off:off + r * c] = np.einsum('erk,eck->erc', U[n], g[io]).reshape(E, r * c)
            gU = np.einsum('erc,eck->erk', wb, g[io])
            if n == 'A':
                ga += (gU * v).sum(-1) * S6
            elif n == 'F':
                gc += (gU * v).sum(-1) * S6
            elif n == 'B':
                gp += gU * s0 * S6
            elif n == 'D':
                gq += gU * s0 * S6
            elif n == 'C':      # u = p x v: the adjoint is v x gU
                gp += np.cross(v, gU) * S72
            else:
                gq += np.cross(v, gU) * S72
        gxe[:, :24], gxe[:, 24:42], gxe[:, 42:60], gxe[:, 60:] = ga, gp.reshape(E, 18), gq.reshape(E, 18), gc
        return gxe, gw
    _, p, q, _ = _parts(xe)
    T = sh[:, 1:4]
    up, uq = np.einsum('erk,ek->er', p, T) * S18, np.einsum('erk,ek->er', q, T) * S18
    g0o, g0e = ge[:, :24], ge[:, 24:]
    gw[:, :144] = (up[:, :, None] * g0e[:, None, :]).reshape(E, 144)
    gw[:, 144:] = (uq[:, :, None] * g0o[:, None, :]).reshape(E, 144)
    gup = np.einsum('erc,ec->er', w[:, :144].reshape(E, 6, 24), g0e)
    guq = np.einsum('erc,ec->er', w[:, 144:].reshape(E, 6, 24), g0o)
    gxe[:, 24:42] = (gup[:, :, None] * T[:, None, :] * S18).reshape(E, 18)
    gxe[:, 42:60] = (guq[:, :, None] * T[:, None, :] * S18).reshape(E, 18)
    return gxe, gw


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def forward(head, x, sh, h, w2, b2, src, dst, n_out):
    """out [n_out, dout]: the mean over the edges with src == r of the tensor product of (x[dst], sh, w2 h + b2); a receiver without edges: zeros"""
    x, sh, h, w2, b2 = _f64(x, sh, h, w2, b2)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    tp = tp_rows(head, x[dst], sh, h @ w2.T + b2)
    out = np.zeros((n_out, DOUT[head]))
    np.add.at(out, src, tp)
    return out / np.maximum(np.bincount(src, minlength=n_out), 1)[:, None]


def vjp(head, x, sh, h, w2, b2, src, dst, n_out, grad_out):
    """(grad_x [N, 84], grad_h [E, K], grad_w2 [W, K], grad_b2 [W]) of ``forward``"""
    x, sh, h, w2, b2, grad_out = _f64(x, sh, h, w2, b2, grad_out)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    cnt = np.maximum(np.bincount(src, minlength=n_out), 1)
    ge = grad_out[src] / cnt[src][:, None]
    gxe, gw = tp_vjp(head, x[dst], sh, h @ w2.T + b2, ge)
    gx = np.zeros_like(x)
    np.add.at(gx, dst, gxe)
    return gx, gw @ w2, gw.T @ h, gw.sum(0)
