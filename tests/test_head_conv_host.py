"""CPU tests of the head convolutions' host side: the fp64 closed form tests/head_conv_ref.py against fp64 autograd of oracle/e3nn_lite.py (the
reference every GPU test of the heads leans on), runtime.head_tp_shape against the instruction table e3nn_lite builds, TensorProductConvLayer in
the two head configurations (state-dict keys and shapes of the reference), and _BatchNormParams for the torsion head's '24x0o + 24x0e'."""
import os
import re

import numpy as np
import pytest
import torch

import head_conv_ref as hcr
from oracle import e3nn_lite
from oracle import score_model_ref as smr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CFG = smr.ScoreModelConfig()
IN_IRREPS = '24x0e + 6x1o + 6x1e + 24x0o'
SH = e3nn_lite.Irreps.spherical_harmonics(1)
TOR_SH = e3nn_lite.FullTensorProduct(SH, '2e').irreps_out
OUT_IRREPS = ('2x1o + 2x1e', '24x0o + 24x0e')


def _relerr(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _e3nn_head(head, x, sh_edge, bond_sh, w):
    """the reference composition in torch: FullyConnectedTensorProduct on (x, sh or FullTensorProduct(sh, bond_sh), w)"""
    if head == 0:
        return e3nn_lite.FullyConnectedTensorProduct(IN_IRREPS, SH, OUT_IRREPS[0])(x, sh_edge, w)
    full = e3nn_lite.FullTensorProduct(SH, '2e')(sh_edge, bond_sh)
    return e3nn_lite.FullyConnectedTensorProduct(IN_IRREPS, TOR_SH, OUT_IRREPS[1])(x, full, w)


@pytest.mark.parametrize('head', [0, 1])
def test_closed_form_against_e3nn_autograd(head):
    """50 random edges, outputs and all four gradients, both sides fp64 evaluations of the same polynomial: 1e-12 relative"""
    E, N, n_out, K, W = 50, 17, 6, hcr.K[head], hcr.W[head]
    gen = torch.Generator().manual_seed(40 + head)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, h, w2, b2 = r(N, 84).requires_grad_(), torch.relu(r(E, K)).requires_grad_(), (r(W, K) / K ** 0.5).requires_grad_(), r(W).requires_grad_()
    vec, bond = r(E, 3), r(E, 3)
    sh_edge = e3nn_lite.spherical_harmonics(SH, vec, normalize=True, normalization='component')
    bond_sh = e3nn_lite.spherical_harmonics('2e', bond, normalize=True, normalization='component')
    src, dst = torch.randint(0, n_out, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    src[src == 3] = 0      # a receiver without edges
    tp = _e3nn_head(head, x[dst], sh_edge, bond_sh, h @ w2.T + b2)
    cnt = torch.bincount(src, minlength=n_out).clamp(min=1).double()
    out = torch.zeros(n_out, tp.shape[1], dtype=torch.float64).index_add(0, src, tp) / cnt[:, None]
    g = r(n_out, tp.shape[1])
    want = torch.autograd.grad(out, (x, h, w2, b2), g)
    if head == 0:
        sh4 = sh_edge
    else:      # the op takes (., T): T is the 1o block, the first three columns of the full tensor product
        sh4 = torch.cat([r(E, 1), e3nn_lite.FullTensorProduct(SH, '2e')(sh_edge, bond_sh)[:, :3]], 1)
        assert str(TOR_SH[0]) == '1x1o'
    n = lambda t: t.detach().numpy()
    args = (head, n(x), n(sh4), n(h), n(w2), n(b2), n(src), n(dst), n_out)
    errs = {'out': _relerr(hcr.forward(*args), n(out))}
    for name, a, b in zip(('grad_x', 'grad_h', 'grad_w2', 'grad_b2'), hcr.vjp(*args, n(g)), want):
        assert a.shape == tuple(b.shape)
        errs[name] = _relerr(a, n(b))
    print(head, {k: f'{v:.2e}' for k, v in errs.items()})
    assert max(errs.values()) < 1e-12, errs
    assert not hcr.forward(*args)[3].any()


@pytest.mark.parametrize('head', [0, 1])
def test_shape_table_is_e3nn_instruction_table(head):
    from disco_diffdock_amd.runtime import head_tp_shape
    s = head_tp_shape(head)
    tp = e3nn_lite.FullyConnectedTensorProduct(IN_IRREPS, SH if head == 0 else TOR_SH, OUT_IRREPS[head])
    assert s['W'] == tp.weight_numel == (144, 288)[head] == hcr.W[head]
    assert s['K'] == hcr.K[head] and s['din'] == tp.irreps_in1.dim == 84 and s['dout'] == tp.irreps_out.dim == hcr.DOUT[head]
    assert [b[1:] for b in s['blocks']] == [tuple(i) for i in tp.instructions]      # (i1, i2, io, offset, (mul1, mul2, mulo)) in instruction order
    assert list(s['out_off']) == [sl.start for sl in tp.irreps_out.slices()]
    for (name, *_), (ref_name, (off, rows, cols, _)) in zip(s['blocks'], hcr.BLOCKS[head].items()):      # the closed form's own table agrees
        blk = next(b for b in s['blocks'] if b[0] == name)
        assert name == ref_name and blk[4] == off and blk[5] == (rows, 1, cols)
    with pytest.raises(RuntimeError, match='head'):
        head_tp_shape(2)


def _head_layers(**kw):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    ns = CFG.ns
    final_conv = TensorProductConvLayer(in_irreps=IN_IRREPS, sh_irreps=SH, out_irreps='2x1o + 2x1e', n_edge_features=2 * ns, residual=False, dropout=0.1,
                                        batch_norm=True, **kw)
    tor_bond_conv = TensorProductConvLayer(in_irreps=IN_IRREPS, sh_irreps=TOR_SH, out_irreps=f'{ns}x0o + {ns}x0e', n_edge_features=3 * ns, residual=False,
                                           dropout=0.1, batch_norm=True, **kw)
    return final_conv, tor_bond_conv


def test_constructor_takes_the_two_head_configurations():
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    spec = smr.state_dict_spec(CFG)
    for prefix, layer in zip(('final_conv', 'tor_bond_conv'), _head_layers()):
        want = {k[len(prefix) + 1:]: tuple(v) for k, v in spec.items() if k.startswith(prefix + '.')}
        got = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
        assert got == want and 'fc.0.weight' in got and 'fc.4.bias' in got, prefix
        assert isinstance(layer.fc, torch.nn.Sequential) and not layer.residual and layer.edge_groups == 1
    msg = re.escape('ddk: the fused kernel implements faster=True, edge_groups=4, residual=True conv layers')
    with pytest.raises(RuntimeError, match=msg):
        TensorProductConvLayer(IN_IRREPS, SH, IN_IRREPS, 72, faster=False, edge_groups=4)
    with pytest.raises(RuntimeError, match=msg):      # a head's arguments with other output irreps
        TensorProductConvLayer(IN_IRREPS, SH, '4x1o + 2x1e', 48, residual=False)
    with pytest.raises(RuntimeError, match=msg):      # ... or another width of the radial MLP
        TensorProductConvLayer(IN_IRREPS, SH, '2x1o + 2x1e', 72, residual=False)
    # the conv layers are built as before
    layer = TensorProductConvLayer(IN_IRREPS, SH, IN_IRREPS, 72, hidden_features=72, faster=True, edge_groups=4)
    assert isinstance(layer.fc, torch.nn.ModuleList) and layer.head is None


def test_batch_norm_order_of_the_torsion_head():
    from disco_diffdock_amd.tensor_layers import _BatchNormParams
    bn = _BatchNormParams('24x0o + 24x0e').double()
    assert bn.blocks == [(24, 1, False), (24, 1, True)]      # the 24 scalars come second
    assert bn.weight.shape == bn.running_var.shape == (48,) and bn.bias.shape == bn.running_mean.shape == (24,)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(48, generator=gen, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(24, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(24, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(48, generator=gen, dtype=torch.float64) + 0.5)
    x = torch.randn(9, 48, generator=gen, dtype=torch.float64)
    bn.eval()
    want = e3nn_lite.batch_norm_eval(x, '24x0o + 24x0e', bn.weight, bn.bias, bn.running_mean, bn.running_var)
    assert torch.equal(bn(x), want) or float((bn(x) - want).abs().max()) < 1e-14
    # the centre head: no scalars at all
    bc = _BatchNormParams('2x1o + 2x1e')
    assert bc.blocks == [(2, 3, False), (2, 3, False)] and bc.bias.shape == (0,) and bc.weight.shape == (4,)
    # the conv layers' strings give the blocks they gave
    assert _BatchNormParams(IN_IRREPS).blocks == [(24, 1, True), (6, 3, False), (6, 3, False), (24, 1, False)]
    assert _BatchNormParams('24x0e + 6x1o').blocks == [(24, 1, True), (6, 3, False)]


def test_entry_points_are_declared_exported_and_bound():
    from disco_diffdock_amd import _lib, build
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    cdll = _lib.lib()
    for name in ('ddk_hconv_forward', 'ddk_hconv_backward', 'ddk_hconv_workspace', 'ddk_seg_sum'):
        assert re.search(r'\b' + name + r'\(', hdr), name
        assert name in _lib.SYMBOLS and hasattr(cdll, name), name
    assert re.search(r'#define DDK_HEAD_CENTER 0\b', hdr) and re.search(r'#define DDK_HEAD_TORSION 1\b', hdr)
    ws = cdll.ddk_hconv_workspace
    assert ws(0, 0, 5, 2, 0) == 0 and ws(1, 0, 5, 2, 0) == 0
    assert ws(0, 10, 5, 2, 0) == 10 * 12 * 4 and ws(1, 10, 5, 2, 0) == 10 * 48 * 4
    # backward: the per-edge rows of grad_x, and E / slice length + 1 parameter images [W][K + 1] (513 edges: two slices of 512)
    assert ws(0, 513, 5, 2, 1) == (513 * 84 + 2 * 144 * 49) * 4 and ws(1, 513, 5, 2, 1) == (513 * 84 + 2 * 288 * 73) * 4
    for bad in ((2, 1, 1, 1, 0), (-1, 1, 1, 1, 0), (0, -1, 1, 1, 0), (0, 1 << 31, 1, 1, 1), (0, 1, -1, 1, 0), (0, 1, 1, 1 << 31, 1)):
        assert ws(*bad) == -1, bad
