"""GPU parity tests (through the C ABI) of the two operator-level entry points:
ddk_tp_forward  == FasterTensorProduct.forward      (reference models/tensor_layers.py:65-116)
ddk_conv_forward == TensorProductConvLayer.forward  (reference models/tensor_layers.py:147-168)
against the golden vectors produced by the reference and against the oracle on larger seeded inputs.
Tolerance: 1e-4 relative (north star) is the bar; fp32 MFMA chains land around 1e-6."""
import numpy as np
import pytest
import torch

from oracle import score_model_ref as smr
from helpers import rel_err

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig()
T = torch.from_numpy


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.mark.parametrize('l', range(5))
def test_faster_tp_golden(dev, golden, l):
    from disco_diffdock_amd.tensor_layers import FasterTensorProduct
    z = golden(f'faster_tp_l{l}')
    i_irr, o_irr = CFG.conv_irreps(l)
    tp = FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr)
    assert tp.weight_numel == int(z['weight_numel'])
    out = tp(T(z['x']).to(dev), T(z['sh']).to(dev), T(z['w']).to(dev)).cpu()
    assert rel_err(out, z['out']) < 1e-5


@pytest.mark.parametrize('l', range(5))
@pytest.mark.parametrize('bn', [0, 1])
def test_conv_layer_golden(dev, golden, l, bn):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    z = golden(f'conv_layer_l{l}_bn{bn}')
    i_irr, o_irr = CFG.conv_irreps(l)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=bool(bn),
                                   dropout=0.1, faster=True, edge_groups=4).eval()
    layer.load_state_dict(smr.random_conv_layer_params(CFG, l, int(z['param_seed']), bool(bn)), strict=True)
    s = z['splits']
    ea = T(z['edge_attr']).to(dev)
    out = layer(T(z['node']).to(dev), T(z['edge_index']).to(dev), [ea[s[i]:s[i + 1]] for i in range(4)], T(z['sh']).to(dev)).cpu()
    assert rel_err(out, z['out']) < 1e-5


def _random_case(l, N, splits, seed, sort_src):
    g = torch.Generator().manual_seed(seed)
    i_irr, o_irr = CFG.conv_irreps(l)
    E = splits[-1]
    node = torch.randn(N, smr.irreps_dim(i_irr), generator=g)
    src = torch.randint(0, N, (E,), generator=g)
    if sort_src:
        for a, b in zip(splits[:-1], splits[1:]):
            src[a:b] = torch.sort(src[a:b]).values
    dst = torch.randint(0, N, (E,), generator=g)
    ea = torch.randn(E, 72, generator=g)
    sh = torch.randn(E, 4, generator=g)
    return node, torch.stack([src, dst]), ea, sh


@pytest.mark.parametrize('l,N,splits,sort_src', [
    (0, 50, [0, 100, 1000, 1777, 3001], True),
    (1, 300, [0, 0, 2049, 2049, 4100], False),      # empty groups
    (2, 7, [0, 1, 2, 3, 4], True),                   # one edge per group
    (3, 400, [0, 1500, 6000, 9000, 12345], True),
    (4, 400, [0, 33, 64, 4000, 4031], False),
    (3, 64, [0, 0, 0, 0, 0], True),                  # no edges at all
])
def test_conv_layer_vs_oracle(dev, l, N, splits, sort_src):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    i_irr, o_irr = CFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(CFG, l, 40 + l, True)
    node, ei, ea, sh = _random_case(l, N, splits, 7 + l, sort_src)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=True,
                                   faster=True, edge_groups=4).eval()
    layer.load_state_dict(Pl, strict=True)
    ea_d = ea.to(dev)
    out = layer(node.to(dev), ei.to(dev), [ea_d[splits[i]:splits[i + 1]] for i in range(4)], sh.to(dev)).cpu()
    P = {'L.' + k: v.double() for k, v in Pl.items()}
    ref = smr.tp_conv_layer(P, 'L', node.double(), ei, [ea.double()[splits[i]:splits[i + 1]] for i in range(4)], sh.double(),
                            i_irr, '1x0e+1x1o', o_irr, residual=True, batch_norm=True, faster=True, edge_groups=4)
    assert rel_err(out, ref) < 1e-5


def test_fused_conv_equals_unfused_boundary(dev):
    """size-independent property at a large size: the fused kernel == radial MLP (torch GEMM) -> ddk_tp_forward ->
    scatter_mean -> BN -> residual, i.e. the reference's own op boundary, on 200k edges."""
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    l, N = 3, 3000
    splits = [0, 20000, 90000, 150000, 200000]
    i_irr, o_irr = CFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(CFG, l, 99, True)
    node, ei, ea, sh = _random_case(l, N, splits, 11, True)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, batch_norm=True, faster=True, edge_groups=4).eval()
    layer.load_state_dict(Pl, strict=True)
    node_d, ei_d, ea_d, sh_d = node.to(dev), ei.to(dev), ea.to(dev), sh.to(dev)
    fused = layer(node_d, ei_d, [ea_d[splits[i]:splits[i + 1]] for i in range(4)], sh_d)
    w = torch.cat([torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(
        ea_d[splits[g]:splits[g + 1]], Pl[f'fc.{g}.0.weight'].to(dev), Pl[f'fc.{g}.0.bias'].to(dev))),
        Pl[f'fc.{g}.4.weight'].to(dev), Pl[f'fc.{g}.4.bias'].to(dev)) for g in range(4)])
    msg = layer.tp(node_d[ei_d[1]], sh_d, w)
    summed = torch.zeros(N, 84, device=dev).index_add_(0, ei_d[0], msg)
    cnt = torch.bincount(ei_d[0], minlength=N).clamp(min=1).unsqueeze(1)
    from oracle import e3nn_lite
    ref = e3nn_lite.batch_norm_eval((summed / cnt).cpu(), o_irr, Pl['batch_norm.weight'], Pl['batch_norm.bias'],
                                    Pl['batch_norm.running_mean'], Pl['batch_norm.running_var']) + node
    assert rel_err(fused.cpu(), ref) < 2e-5


@pytest.mark.parametrize('kernel', [0, 1, 3])
@pytest.mark.parametrize('l', range(5))
def test_confidence_conv_layer_vs_oracle(dev, l, kernel):
    """One conv of the all-atom confidence model (e3nn FCTP with sh 0e+1o+2e, BatchNorm, no residual)
    through ddk_conv_forward in an all-atom context == the oracle's conv layer; every conv kernel (0: two f16 limbs / three products, 1: fp32 MFMA, 3: three limbs / six products)."""
    from oracle import confidence_ref as cr, e3nn_lite as o3
    from disco_diffdock_amd.runtime import Context
    cfg = cr.ConfidenceModelConfig()
    P = {k: v for k, v in cr.random_state_dict(cfg, seed=60 + l).items() if k.startswith('conv_layers.')}
    ctx = Context(device=0, all_atoms=1, embedding_scale=10000.0, num_confidence_outputs=2, conv_kernel=kernel)
    ctx.load_state_dict(P)
    i_irr, o_irr = cfg.conv_irreps(l)
    din, dout = smr.irreps_dim(i_irr), smr.irreps_dim(o_irr)
    g = torch.Generator().manual_seed(l)
    N, E = 300, 5000
    node = torch.randn(N, din, generator=g)
    src = torch.sort(torch.randint(0, N, (E,), generator=g)).values
    dst = torch.randint(0, N, (E,), generator=g)
    ea = torch.randn(E, 72, generator=g)
    vec = torch.randn(E, 3, generator=g)
    vec[::7] = 0.0                      # zero-length edges (a C-alpha atom and its own residue): Y1 = Y2 = 0
    sh9 = o3.spherical_harmonics(cfg.sh_irreps, vec, normalize=True, normalization='component')
    for k in (0, 4, 8):
        want = cr.conv_layer(P, f'conv_layers.{9 * l + k}', cfg, l, node, torch.stack([src, dst]), ea, sh9, out_nodes=N)
        got = ctx.conv_forward(9 * l + k, node.to(dev), src.to(dev), dst.to(dev), [0, E, E, E, E], ea.to(dev), sh9[:, :4].contiguous().to(dev), dout)
        assert rel_err(got.cpu(), want) < 1e-5, (l, k)


@pytest.mark.parametrize('l,N,splits,sort_src', [
    (0, 50, [0, 100, 1000, 1777, 3001], True),
    (1, 300, [0, 0, 2049, 2049, 4100], False),
    (3, 400, [0, 1500, 6000, 9000, 12345], True),
    (4, 400, [0, 33, 64, 4000, 4031], False),
])
def test_conv_layer_fp32_kernel_vs_oracle(dev, l, N, splits, sort_src):
    """The fallback ddk_config.conv_kernel = 1 (radial-MLP GEMMs as fp32 MFMA chains; the default is the f16-limb product - two limbs, three products since round 6 - which
    every other test of this file runs) must meet the SAME bar against the fp64 oracle, and repeated launches must agree."""
    from disco_diffdock_amd.runtime import Context
    i_irr, o_irr = CFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(CFG, l, 40 + l, True)
    node, ei, ea, sh = _random_case(l, N, splits, 7 + l, sort_src)
    ctx = Context(device=0, conv_kernel=1)
    ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in Pl.items()})
    dout = smr.irreps_dim(o_irr)
    P = {'L.' + k: v.double() for k, v in Pl.items()}
    ref = smr.tp_conv_layer(P, 'L', node.double(), ei, [ea.double()[splits[i]:splits[i + 1]] for i in range(4)], sh.double(),
                            i_irr, '1x0e+1x1o', o_irr, residual=True, batch_norm=True, faster=True, edge_groups=4)
    args = (l, node.to(dev), ei[0].to(dev), ei[1].to(dev), splits, ea.to(dev), sh.to(dev), dout)
    for _ in range(5):
        out = ctx.conv_forward(*args).cpu()
        assert rel_err(out, ref) < 1e-5


@pytest.mark.parametrize('in_scale,w1_scale,w2_scale', [
    (1e4, 1e2, 1e-6),       # inputs and hidden units (~1e6) far above the fp16 maximum 65504, W2 far below the fp16 normal range 6.1e-5
    (1e-4, 1e-2, 1e6),      # tiny inputs, W1 and hidden units (~1e-6); W2 above the fp16 maximum
    (1.0, 1e6, 1e-6),       # W1 above, W2 below
])
def test_conv_layer_x3_range(dev, in_scale, w1_scale, w2_scale):
    """The f16-limb products (0: two limbs / three products, the default; 3: three limbs / six products) must not depend on the SCALE of a checkpoint or of
    the features: operands are range-scaled by exact powers of two (weights per group at pack time, activations per edge in the kernel), so operands far outside
    the fp16 range meet the same bar, and the error against the fp64 oracle is not larger than the fp32-MFMA kernel's (VERDICT r02 #3 ii; 2x for the default).
    (The three scales multiply to 1, so the messages stay O(1) next to the residual and the batch-norm statistics.)
    The additive terms stay: with ~18 edges per node the fp32 atomics of the scatter reorder from run to run, and against the largest output element the
    ratios to the fp32-MFMA kernel measured in two runs of the same build were 1.42 / 1.51 / 1.00 and 1.42 / 1.11 / 1.00 (default, bar 2.0) but
    1.91 / 0.95 / 1.00 and 1.14 / 0.95 / 1.00 (three limbs, bar 1.5) over the three cases: the factors alone do not hold run to run.  The ratios are kept in the drift
    file; the per-column bars without any additive term are tests/test_gpu_conv_adversarial.py's (one edge per node: no atomics noise)."""
    from disco_diffdock_amd.runtime import Context
    from test_gpu_round3 import _record_drift
    l, N, splits = 3, 300, [0, 700, 2500, 4000, 5555]
    i_irr, o_irr = CFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(CFG, l, 77, True)
    for k in list(Pl):
        if k.startswith('fc.') and k.endswith('.0.weight'):
            Pl[k] = Pl[k] * w1_scale
        if k.startswith('fc.') and k.endswith('.0.bias'):
            Pl[k] = Pl[k] * (w1_scale * in_scale)
        if k.startswith('fc.') and k.endswith('.4.weight'):     # (.4.bias stays O(0.1) like the W2 h it is added to)
            Pl[k] = Pl[k] * w2_scale
    node, ei, ea, sh = _random_case(l, N, splits, 11, True)
    ea = ea * in_scale
    P = {'L.' + k: v.double() for k, v in Pl.items()}
    ref = smr.tp_conv_layer(P, 'L', node.double(), ei, [ea.double()[splits[i]:splits[i + 1]] for i in range(4)], sh.double(),
                            i_irr, '1x0e+1x1o', o_irr, residual=True, batch_norm=True, faster=True, edge_groups=4)
    assert 0.05 < float(ref.abs().max()) < 1e3
    args = (l, node.to(dev), ei[0].to(dev), ei[1].to(dev), splits, ea.to(dev), sh.to(dev), smr.irreps_dim(o_irr))
    err = {}
    for kernel in (0, 1, 3):       # 0: two f16 limbs / three products (default), 1: fp32 MFMA, 3: three limbs / six products
        ctx = Context(device=0, conv_kernel=kernel)
        ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in Pl.items()})
        out = ctx.conv_forward(*args).cpu()
        assert torch.isfinite(out).all()
        err[kernel] = rel_err(out, ref)
    print(f'range test {in_scale:g}/{w1_scale:g}/{w2_scale:g}: two limbs / three products {err[0]:.2e}, fp32 MFMA {err[1]:.2e}, three limbs / six products {err[3]:.2e}')
    _record_drift(f'conv_layer_x3_range_{in_scale:g}_{w1_scale:g}_{w2_scale:g}', err[0], bar=1e-5, two_limbs_three_products=err[0], fp32_chains=err[1], six_products=err[3],
                  two_limbs_ratio_to_fp32=err[0] / err[1], six_products_ratio_to_fp32=err[3] / err[1])
    assert err[3] < 1e-5 and err[3] < 1.5 * err[1] + 2e-7, err
    assert err[0] < 1e-5 and err[0] < 2.0 * err[1] + 4e-7, err      # the same per-edge range scaling: no dependence on the magnitude of inputs / weights
