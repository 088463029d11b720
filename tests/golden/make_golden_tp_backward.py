#!/usr/bin/env python
"""Generate tests/golden/faster_tp_backward_l{0..4}.npz by EXECUTING THE REFERENCE under torch autograd.

Like make_golden.py this runs only where the reference checkout is present (REF of make_golden.py); only the produced arrays are committed.  The unmodified
reference class models/tensor_layers.py:FasterTensorProduct is evaluated in fp64 on fp32-representable inputs (E = 16 edges per layer), and
autograd gives the vector-Jacobian product for a random incoming gradient:

    x, sh, w, grad_out   float32  (the operands)
    grad_x, grad_sh, grad_w   float64  (what ddk_tp_backward must reproduce)

    python tests/golden/make_golden_tp_backward.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
from oracle import score_model_ref as smr  # noqa: E402


def main():
    mg.install_standins()
    from models import tensor_layers      # the unmodified reference module
    cfg = smr.ScoreModelConfig()
    g = torch.Generator().manual_seed(20)
    E = 16
    for l in range(5):
        i_irr, o_irr = cfg.conv_irreps(l)
        tp = tensor_layers.FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr).double()
        x = torch.randn(E, smr.irreps_dim(i_irr), generator=g)
        sh = torch.randn(E, 4, generator=g)
        w = torch.randn(E, tp.weight_numel, generator=g)
        grad_out = torch.randn(E, smr.irreps_dim(o_irr), generator=g)
        xd, sd, wd = (t.double().requires_grad_(True) for t in (x, sh, w))
        out = tp(xd, sd, wd)
        assert out.dtype == torch.float64
        gx, gs, gw = torch.autograd.grad(out, (xd, sd, wd), grad_out.double())
        mg.save(f'faster_tp_backward_l{l}', x=x, sh=sh, w=w, grad_out=grad_out, grad_x=gx, grad_sh=gs, grad_w=gw)


if __name__ == '__main__':
    main()
