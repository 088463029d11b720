"""The radial tensor product and its vector-Jacobian product in closed form, fp64 numpy: the specification ddk_rtp_forward / ddk_rtp_backward are
written against (tests/golden/radial_tp_l0.npz, made by autograd of the unmodified reference classes, decides whether this text is right:
tests/test_radial_tp_host.py).

    w_e = W2[g(e)] h_e + b2[g(e)]            out_e = FasterTensorProduct(x_e, sh_e, w_e)       (tests/tp_backward_ref.py: forward)

With gw_e = grad_w of tests/tp_backward_ref.py: backward (it needs no w), and grad_x, grad_sh of the same function at w_e:

    grad_h[e, j] = sum_p gw_e[p] W2[g(e)][p, j]      grad_w2[g][p, j] = sum_{e in g} gw_e[p] h_e[j]      grad_b2[g][p] = sum_{e in g} gw_e[p]
"""
import numpy as np

import tp_backward_ref as tpr

HIDDEN = 72


def weights(layer, h, offsets, w2, b2):
    """w [E, W] (fp64): the per-edge weights the device never stores"""
    h, w2, b2 = (np.asarray(t, np.float64) for t in (h, w2, b2))
    w = np.zeros((h.shape[0], tpr.shape(layer)['W']))
    for g in range(len(offsets) - 1):
        sl = slice(offsets[g], offsets[g + 1])
        w[sl] = h[sl] @ w2[g].T + b2[g]
    return w


def forward(layer, x, sh, h, offsets, w2, b2):
    """out [E, Dout] in fp64"""
    return tpr.forward(layer, x, sh, weights(layer, h, offsets, w2, b2))


def backward(layer, x, sh, h, offsets, w2, b2, grad_out):
    """(grad_x [E, Din], grad_sh [E, 4], grad_h [E, 72], grad_w2 [G, W, 72], grad_b2 [G, W]) in fp64"""
    h64, w264 = np.asarray(h, np.float64), np.asarray(w2, np.float64)
    gx, gsh, gw = tpr.backward(layer, x, sh, weights(layer, h, offsets, w2, b2), grad_out)
    G = len(offsets) - 1
    gh, gw2, gb2 = np.zeros_like(h64), np.zeros_like(w264), np.zeros(w264.shape[:2])
    for g in range(G):
        sl = slice(offsets[g], offsets[g + 1])
        gh[sl] = gw[sl] @ w264[g]
        gw2[g] = gw[sl].T @ h64[sl]
        gb2[g] = gw[sl].sum(0)
    return gx, gsh, gh, gw2, gb2
