#!/usr/bin/env python
"""Generate tests/golden/radial_tp_l0.npz by EXECUTING THE REFERENCE under torch autograd.

Like make_golden.py this runs only where the reference checkout is present (REF of make_golden.py); only the produced arrays are committed.  The unmodified
reference classes - the last Linear of models/layers.py:FCBlock per edge group, torch.cat, models/tensor_layers.py:FasterTensorProduct - are evaluated
in fp64 on fp32-representable inputs: conv layer 0, E = 24 edges in G = 2 groups [0, 11, 24], and autograd gives the vector-Jacobian product for a
random incoming gradient:

    x, sh, h, w2 [G, W, 72], b2 [G, W], grad_out   float32  (the operands; offsets int64)
    out, grad_x, grad_sh, grad_h, grad_w2, grad_b2   float64  (what ddk_rtp_forward / ddk_rtp_backward must reproduce)

The file has to stay below the largest golden of the suite, and grad_w2 alone is 2 x 720 x 72 doubles of noise.  So the operands are chosen to compress
without losing a case: h is what ReLU and Dropout leave, with 24 of the 72 hidden units alive per group (the columns of grad_w2 of a dead unit are
exact zeros), and w2 is drawn on a grid of 1/8.

    python tests/golden/make_golden_radial_tp.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
from oracle import score_model_ref as smr  # noqa: E402


def main():
    mg.install_standins()
    from models import tensor_layers      # the unmodified reference modules
    from models.layers import FCBlock
    cfg = smr.ScoreModelConfig()
    g = torch.Generator().manual_seed(40)
    l, E, offsets = 0, 24, [0, 11, 24]
    G = len(offsets) - 1
    i_irr, o_irr = cfg.conv_irreps(l)
    tp = tensor_layers.FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr).double()
    W = tp.weight_numel
    x = torch.randn(E, smr.irreps_dim(i_irr), generator=g)
    sh = torch.randn(E, 4, generator=g)
    h = torch.relu(torch.randn(E, 72, generator=g))
    for k in range(G):
        alive = torch.zeros(72)
        alive[torch.randperm(72, generator=g)[:24]] = 1.0
        h[offsets[k]:offsets[k + 1]] *= alive
    w2 = torch.round(torch.randn(G, W, 72, generator=g) * 8) / 8
    b2 = torch.randn(G, W, generator=g)
    grad_out = torch.randn(E, smr.irreps_dim(o_irr), generator=g)
    fc = [FCBlock(72, 72, W, 2, 0.0).double() for _ in range(G)]
    for k in range(G):
        fc[k][4].weight.data.copy_(w2[k].double())
        fc[k][4].bias.data.copy_(b2[k].double())
    xd, sd, hd = (t.double().requires_grad_(True) for t in (x, sh, h))
    w = torch.cat([fc[k][4](hd[offsets[k]:offsets[k + 1]]) for k in range(G)], dim=0)
    out = tp(xd, sd, w)
    assert out.dtype == torch.float64
    params = [fc[k][4].weight for k in range(G)] + [fc[k][4].bias for k in range(G)]
    grads = torch.autograd.grad(out, [xd, sd, hd] + params, grad_out.double())
    mg.save('radial_tp_l0', x=x, sh=sh, h=h, w2=w2, b2=b2, grad_out=grad_out, offsets=torch.tensor(offsets), out=out, grad_x=grads[0], grad_sh=grads[1],
            grad_h=grads[2], grad_w2=torch.stack(grads[3:3 + G]), grad_b2=torch.stack(grads[3 + G:]))


if __name__ == '__main__':
    main()
