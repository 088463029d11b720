"""The radial conv (ddk_rconv_forward / ddk_rconv_backward) and e3nn's BatchNorm in closed form, fp64 numpy: lines 153-162 of the reference's
TensorProductConvLayer.forward with reduce='mean', built from tests/radial_tp_ref.py.

    out_nodes[n] = (sum over e with src[e] == n of rtp_forward(x[dst], ...)[e]) / max(count[n], 1)

    backward: rtp_backward with g_e = grad_out_nodes[src[e]] / count[src[e]], then grad_x_nodes[n] = sum over e with dst[e] == n of grad_x[e]
"""
import numpy as np

import radial_tp_ref as ref


def counts(src, n_out):
    return np.maximum(np.bincount(np.asarray(src, np.int64), minlength=n_out)[:n_out], 1).astype(np.float64)


def forward(layer, x_nodes, src, dst, n_out, sh, h, offsets, w2, b2):
    """out_nodes [n_out, Dout] in fp64"""
    x64 = np.asarray(x_nodes, np.float64)
    rows = ref.forward(layer, x64[dst], sh, h, offsets, w2, b2)
    out = np.zeros((n_out, rows.shape[1]))
    np.add.at(out, src, rows)
    return out / counts(src, n_out)[:, None]


def backward(layer, x_nodes, src, dst, n_out, sh, h, offsets, w2, b2, grad_out_nodes):
    """(grad_x_nodes [n_in, Din], grad_sh [E, 4], grad_h [E, 72], grad_w2 [G, W, 72], grad_b2 [G, W]) in fp64"""
    x64 = np.asarray(x_nodes, np.float64)
    g = (np.asarray(grad_out_nodes, np.float64) / counts(src, n_out)[:, None])[src]
    gx, gsh, gh, gw2, gb2 = ref.backward(layer, x64[dst], sh, h, offsets, w2, b2, g)
    gxn = np.zeros_like(x64)
    np.add.at(gxn, dst, gx)
    return gxn, gsh, gh, gw2, gb2


# ---- e3nn.nn.BatchNorm with its defaults (eps 1e-5, momentum 0.1, affine, reduce 'mean', normalization 'component', not instance) --------------------
def bn_blocks(muls):
    """(mul, d, is_scalar) per irrep block of (0e, 1o, 1e, 0o) multiplicities: 0o is not a scalar for e3nn"""
    return [(m, d, k == 0) for k, (m, d) in enumerate(zip(muls, (1, 3, 3, 1))) if m]


def batch_norm(x, muls, weight, bias, running_mean, running_var, training, eps=1e-5, momentum=0.1):
    """(out, new_running_mean, new_running_var), fp64; in evaluation the buffers come back as they went in"""
    x = np.asarray(x, np.float64)
    rm, rv = np.array(running_mean, np.float64), np.array(running_var, np.float64)
    out, ix, iw, ib = [], 0, 0, 0
    for mul, d, scalar in bn_blocks(muls):
        f = x[:, ix:ix + mul * d].reshape(-1, mul, d).copy()
        ix += mul * d
        if scalar:
            if training:
                mean = f.mean(axis=(0, 2))
                rm[ib:ib + mul] = (1 - momentum) * rm[ib:ib + mul] + momentum * mean
            else:
                mean = rm[ib:ib + mul]
            f -= mean[None, :, None]
        if training:
            norm = (f ** 2).mean(axis=2).mean(axis=0)
            rv[iw:iw + mul] = (1 - momentum) * rv[iw:iw + mul] + momentum * norm
        else:
            norm = rv[iw:iw + mul]
        f *= ((norm + eps) ** -0.5 * np.asarray(weight, np.float64)[iw:iw + mul])[None, :, None]
        if scalar:
            f += np.asarray(bias, np.float64)[ib:ib + mul][None, :, None]
            ib += mul
        iw += mul
        out.append(f.reshape(-1, mul * d))
    return np.concatenate(out, axis=1), rm, rv
