"""GPU tests of the second shape family of the tensor-product ops (ns = 24, nv = 4; the `layer` ids DDK_TP_NV4 + l): ddk_tp_*, ddk_rtp_*, ddk_rconv_* through
Context, and TensorProductConvLayer on nv = 4 irreps in .train() and .eval().

Reference: fp64 autograd through the oracle's faster_tensor_product / tp_conv_layer (tests/latent_encoder_ref.py).  Bar: helpers.rel_err < 1e-5 PER BLOCK
(each irrep slice of out and grad_x, grad_sh, grad_h, each group and weight block of grad_w2 / grad_b2), the bar of the nv = 6 tests of the same kernels
(tests/test_gpu_tp_backward.py, test_gpu_radial_tp.py, test_gpu_radial_conv.py): the arithmetic is the same fp32 fmaf / fp32-MFMA chains, over shorter
rows.  The graphs and group tables are those of tests/test_gpu_radial_conv.py, chosen for these kernels' boundaries."""
import numpy as np
import pytest
import torch

import latent_encoder_ref as ler
from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_radial_conv import _awkward_graph, _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
BAR = 1e-5
NV4 = 8      # DDK_TP_NV4
CFG4 = smr.ScoreModelConfig(nv=4)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.runtime import TP_NV4
    from disco_diffdock_amd.tensor_layers import _shape_context
    assert TP_NV4 == NV4
    return _shape_context(0)      # a shape-only context: no weights loaded


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _block_errors(s, offsets, got_out, got, want_out, want):
    """rel_err per block: out / grad_x per irrep slice, grad_sh, grad_h, grad_w (tp) per weight block, grad_w2 / grad_b2 per group and weight block"""
    errs = {}
    for name, sl in ler.out_slices(s).items():
        errs[f'out.{name}'] = rel_err(got_out[:, sl], want_out[:, sl])
    for name, sl in ler.in_slices(s).items():
        errs[f'grad_x.{name}'] = rel_err(got['x'][:, sl], want['x'][:, sl])
    for k in ('sh', 'h'):
        if k in want and want[k].size:
            errs[f'grad_{k}'] = rel_err(got[k], want[k])
    for name, sl in ler.weight_slices(s).items():
        if 'w' in want and want['w'].size:
            errs[f'grad_w.{name}'] = rel_err(got['w'][:, sl], want['w'][:, sl])
        if 'w2' in want:
            for g in range(len(offsets) - 1):
                if offsets[g + 1] > offsets[g]:
                    errs[f'grad_w2.g{g}.{name}'] = rel_err(got['w2'][g, sl], want['w2'][g, sl])
                    errs[f'grad_b2.g{g}.{name}'] = rel_err(got['b2'][g, sl], want['b2'][g, sl])
    return errs


def _assert_blocks(tag, errs):
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'tp_nv4.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


# ---- 1. the tensor product at the op boundary -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', range(4))
def test_tp_forward_and_backward(ctx, dev, l):
    s = ler.shape(l, 4)
    for E in (1, 63, 64, 65, 130):
        rng = np.random.default_rng(1000 + 10 * l + E)
        f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
        x, sh, w, g = f(E, s['din']), f(E, 4), f(E, s['W']), f(E, s['dout'])
        t = [_to(dev, a) for a in (x, sh, w, g)]
        out = ctx.tp_forward(NV4 + l, t[0], t[1], t[2], s['dout'])
        full = ctx.tp_backward(NV4 + l, *t)
        want_out, want = ler.tp(l, 4, x, sh, w, g)
        assert out.shape == (E, s['dout']) and [tuple(a.shape) for a in full] == [(E, s['din']), (E, 4), (E, s['W'])]
        _assert_blocks(f'tp.l{l}.E{E}', _block_errors(s, [0, E], _np(out), dict(zip(('x', 'sh', 'w'), map(_np, full))), want_out, want))
        # each gradient asked for alone, and two runs: the same bits
        assert torch.equal(_bits(out), _bits(ctx.tp_forward(NV4 + l, t[0], t[1], t[2], s['dout'])))
        again = ctx.tp_backward(NV4 + l, *t)
        for k in range(3):
            need = tuple(i == k for i in range(3))
            alone = ctx.tp_backward(NV4 + l, t[0], t[1], None if k == 2 else t[2], t[3], need)
            assert [a is not None for a in alone] == list(need)
            assert torch.equal(_bits(alone[k]), _bits(full[k])) and torch.equal(_bits(again[k]), _bits(full[k])), (E, k)


# ---- 2. the radial tensor product and the radial conv ---------------------------------------------------------------------------------------------------------
def _radial_operands(s, offsets, n_in, n_out, seed, per_edge):
    E, G = offsets[-1], len(offsets) - 1
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=f(E if per_edge else n_in, s['din']), sh=f(E, 4), h=np.maximum(f(E, 72), 0), w2=f(G, s['W'], 72) / np.float32(np.sqrt(72.0)), b2=f(G, s['W']),
                g=f(E if per_edge else n_out, s['dout']))


NAMES = ('x', 'sh', 'h', 'w2', 'b2')


def _check_rtp(ctx, dev, tag, l, offsets, seed):
    s = ler.shape(l, 4)
    o = _radial_operands(s, offsets, 0, 0, seed, True)
    t = {k: _to(dev, v) for k, v in o.items()}
    run = lambda: (ctx.rtp_forward(NV4 + l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], s['dout']),
                   ctx.rtp_backward(NV4 + l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g']))
    out, grads = run()
    want_out, want = ler.rtp(l, 4, o['x'], o['sh'], o['h'], offsets, o['w2'], o['b2'], o['g'])
    _assert_blocks(tag, _block_errors(s, offsets, _np(out), dict(zip(NAMES, map(_np, grads))), want_out, want))
    out2, grads2 = run()
    assert torch.equal(_bits(out), _bits(out2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, grads2))      # two runs: the same bits
    return _np(out), [_np(a) for a in grads]


def _check_rconv(ctx, dev, tag, l, src, dst, n_in, n_out, offsets, seed):
    s = ler.shape(l, 4)
    o = _radial_operands(s, offsets, n_in, n_out, seed, False)
    t = {k: _to(dev, v) for k, v in o.items()}
    graph = ctx.conv_graph(_to(dev, np.asarray(src)), _to(dev, np.asarray(dst)), n_in, n_out)
    run = lambda: (ctx.rconv_forward(NV4 + l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2']),
                   ctx.rconv_backward(NV4 + l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g']))
    out, grads = run()
    assert out.shape == (n_out, s['dout']) and grads[0].shape == (n_in, s['din'])
    want_out, want = ler.rconv(l, 4, o['x'], src, dst, n_out, o['sh'], o['h'], offsets, o['w2'], o['b2'], o['g'])
    _assert_blocks(tag, _block_errors(s, offsets, _np(out), dict(zip(NAMES, map(_np, grads))), want_out, want))
    out2, grads2 = run()
    assert torch.equal(_bits(out), _bits(out2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, grads2))
    return _np(out), [_np(a) for a in grads]


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_on_the_awkward_graph(ctx, dev, l):
    N, offs = 11, [0, 1, 1, 34, 70]      # a one-edge group, an empty group, boundaries off the tile grid
    src, dst = _awkward_graph(N, offs[-1], 5)      # a self-loop, a duplicated edge, a node that receives nothing, one that sends nothing
    _, grads = _check_rtp(ctx, dev, f'rtp.graph.l{l}', l, offs, 100 + l)
    assert not grads[3][1].any() and not grads[4][1].any()      # the empty group: exact zeros
    out, grads = _check_rconv(ctx, dev, f'rconv.graph.l{l}', l, src, dst, N, N, offs, 100 + l)
    assert not out[N - 1].any()      # the node that receives nothing: exact zeros
    assert not grads[0][N - 2].any()      # the node that sends nothing
    assert not grads[3][1].any() and not grads[4][1].any()      # the empty group


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_tails(ctx, dev, l):
    N = 5
    for E in (1, 31, 32, 33, 129):
        rng = np.random.default_rng(E)
        if E == 129:      # one node holds every edge, in and out: its sums cross the waves of a workgroup and two workgroups
            src, dst = np.full(E, 2), np.full(E, 4)
        else:
            src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
        _check_rtp(ctx, dev, f'rtp.tails.l{l}.E{E}', l, [0, E], 200 + 7 * l + E)
        _check_rconv(ctx, dev, f'rconv.tails.l{l}.E{E}', l, src, dst, N, N, [0, E], 200 + 7 * l + E)


@pytest.mark.parametrize('l', range(4))
def test_radial_conv_other_number_of_output_nodes(ctx, dev, l):
    n_in, n_out, offs = 9, 4, [0, 10, 25, 25, 50]
    rng = np.random.default_rng(31)
    src, dst = rng.integers(0, n_out, offs[-1]), rng.integers(0, n_in, offs[-1])
    dst[0], dst[1] = n_in - 1, n_out      # rows of x past n_out are read
    _check_rconv(ctx, dev, f'rconv.n_out_4.n_in_9.l{l}', l, src, dst, n_in, n_out, offs, 300 + l)


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_across_a_slice_of_the_parameter_pass(ctx, dev, l):
    N, offs = 40, [0, 600]      # one group of 600 edges: the parameter pass crosses a 512-edge slice
    rng = np.random.default_rng(60 + l)
    _check_rtp(ctx, dev, f'rtp.slices.l{l}', l, offs, 600 + l)
    _check_rconv(ctx, dev, f'rconv.slices.l{l}', l, rng.integers(0, N, 600), rng.integers(0, N, 600), N, N, offs, 600 + l)


def test_family_ids_outside_the_table_are_refused(ctx, dev):
    one = torch.zeros(4096, device=dev)
    for bad in (5, 7, 13):      # (the shape-only context has five conv layers)
        assert ctx.L.ddk_tp_forward(ctx.h, bad, one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, one.data_ptr(), None) != 0
        msg = ctx.L.ddk_last_error(ctx.h).decode()
        assert 'DDK_TP_NV4' in msg and '6x1o' in msg and '4x1o' in msg, msg      # the refusal names both families
    # a context that holds conv layers 8 and 9 refuses the ids that are also its own layers' indices (before the second family they ran ITS layer), serves the rest
    from disco_diffdock_amd.runtime import Context
    big = Context(device=0, num_conv_layers=10)
    big.finalize()
    s = ler.shape(0, 4)
    x, sh, w = torch.randn(3, s['din'], device=dev), torch.randn(3, 4, device=dev), torch.randn(3, s['W'], device=dev)
    with pytest.raises(RuntimeError, match='this context has a conv layer 8'):
        big.tp_forward(NV4, x, sh, w, s['dout'])
    s3 = ler.shape(3, 4)
    x3, w3 = torch.randn(3, s3['din'], device=dev), torch.randn(3, s3['W'], device=dev)
    assert torch.equal(_bits(big.tp_forward(NV4 + 3, x3, sh, w3, s3['dout'])), _bits(ctx.tp_forward(NV4 + 3, x3, sh, w3, s3['dout'])))


# ---- 3. TensorProductConvLayer on nv = 4 irreps -------------------------------------------------------------------------------------------------------------------
def _layer(l, dev, bn, seed, nv=4, dropout=0.0):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    cfg = smr.ScoreModelConfig(nv=nv)
    i_irr, o_irr = cfg.conv_irreps(l)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=bn, dropout=dropout, faster=True, edge_groups=4)
    layer.load_state_dict(smr.random_conv_layer_params(cfg, l, seed, bn), strict=True)
    return layer.to(dev)


def _layer_case(l, seed):
    offs, s, N = [0, 50, 131, 132, 300], ler.shape(l, 4), 40
    rng = np.random.default_rng(seed)
    E = offs[-1]
    x, sh, emb, g = (rng.standard_normal((n, c)).astype(np.float32) for n, c in ((N, s['din']), (E, 4), (E, 24), (N, s['dout'])))
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    return offs, s, N, x, sh, emb, g, src, dst


def _layer_fp64(layer, l, x, sh, emb, g, src, dst, offs, bn, training, embedded):
    """the oracle's layer in fp64: out, the gradients of node_attr and of every parameter, the statistics BatchNorm's buffers are moved by.  ``embedded``:
    the edge attributes are [emb | x[src, :24] | x[dst, :24]] of the node table (forward_embedded), else fixed rows (forward)"""
    P = {'L.' + k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    for k, _ in layer.named_parameters():
        P['L.' + k].requires_grad_(True)
    X = torch.from_numpy(x).double().requires_grad_(True)
    ei = torch.from_numpy(np.stack([src, dst]))
    ea = torch.cat([torch.from_numpy(emb).double(), X[ei[0], :24], X[ei[1], :24]], 1) if embedded else torch.from_numpy(_fixed_rows(x, emb, src, dst)).double()
    out, stats = ler.conv_layer(P, 'L', l, 4, X, ei, [ea[offs[k]:offs[k + 1]] for k in range(4)], torch.from_numpy(sh).double(), bn, training)
    out.backward(torch.from_numpy(g).double())
    want = {'out': out.detach().numpy(), 'node_attr': X.grad.numpy()}
    want.update({k: P['L.' + k].grad.numpy() for k, _ in layer.named_parameters()})
    return want, stats


def _fixed_rows(x, emb, src, dst):
    return np.concatenate([emb, x[src, :24], x[dst, :24]], 1)


def _layer_device(layer, dev, x, sh, emb, g, src, dst, offs, embedded):
    layer.zero_grad(set_to_none=True)
    X = _to(dev, x).requires_grad_(True)
    ei = _to(dev, np.stack([src, dst]))
    sizes = [offs[k + 1] - offs[k] for k in range(4)]
    if embedded:
        out = layer.forward_embedded(X, ei, _to(dev, emb), sizes, _to(dev, sh))
    else:
        ea = _to(dev, _fixed_rows(x, emb, src, dst))
        out = layer(X, ei, list(torch.split(ea, sizes)), _to(dev, sh))
    out.backward(_to(dev, g))
    got = {'out': out.detach(), 'node_attr': X.grad}
    got.update({k: p.grad for k, p in layer.named_parameters()})
    assert all(v is not None for v in got.values())
    return {k: _np(v) for k, v in got.items()}


@pytest.mark.parametrize('l,bn', [(0, False), (0, True), (2, False), (2, True)])
@pytest.mark.parametrize('embedded', [False, True])
def test_nv4_layer_in_training_against_fp64(dev, l, bn, embedded):
    offs, s, N, x, sh, emb, g, src, dst = _layer_case(l, 800 + l)
    layer = _layer(l, dev, bn, 80 + l).train()
    assert layer.layer == NV4 + l
    before = {k: v.detach().cpu().double().numpy() for k, v in layer.named_buffers()}
    got = _layer_device(layer, dev, x, sh, emb, g, src, dst, offs, embedded)
    want, stats = _layer_fp64(layer, l, x, sh, emb, g, src, dst, offs, bn, True, embedded)      # (reads the parameters alone: the buffers have moved)
    assert set(got) == set(want) and len(want) == 2 + 16 + (2 if bn else 0)
    errs = {k: rel_err(got[k], want[k]) for k in want}
    if bn:
        after = {k: _np(v) for k, v in layer.named_buffers()}
        for k, stat in zip(('batch_norm.running_mean', 'batch_norm.running_var'), stats):
            errs[k] = rel_err(after[k], 0.9 * before[k] + 0.1 * stat.numpy())
            assert not np.array_equal(after[k], before[k])
    _assert_blocks(f'layer_training.l{l}.bn{int(bn)}.embedded{int(embedded)}', errs)


@pytest.mark.parametrize('l,bn', [(0, False), (0, True), (2, False), (2, True)])
def test_nv4_layer_in_evaluation(dev, l, bn):
    """.eval() of an nv = 4 layer runs the training ops: BatchNorm on the running buffers, no dropout (the layer is built with rate 0.5), the same bits on
    two calls, the buffers untouched; against the oracle in fp64"""
    offs, s, N, x, sh, emb, g, src, dst = _layer_case(l, 850 + l)
    layer = _layer(l, dev, bn, 85 + l, dropout=0.5).eval()
    buffers = {k: v.detach().clone() for k, v in layer.named_buffers()}
    for embedded in (False, True):
        got = _layer_device(layer, dev, x, sh, emb, g, src, dst, offs, embedded)
        again = _layer_device(layer, dev, x, sh, emb, g, src, dst, offs, embedded)
        assert all(np.array_equal(got[k], again[k]) for k in got)      # bit-identical, every gradient too
        want, _ = _layer_fp64(layer, l, x, sh, emb, g, src, dst, offs, bn, False, embedded)
        if bn:      # the running buffers scale and shift; the affine parameters still get their gradient
            assert want['batch_norm.weight'].any()
        _assert_blocks(f'layer_eval.l{l}.bn{int(bn)}.embedded{int(embedded)}', {k: rel_err(got[k], want[k]) for k in want})
        with torch.no_grad():
            quiet = layer.forward_embedded(_to(dev, x), _to(dev, np.stack([src, dst])), _to(dev, emb), [offs[k + 1] - offs[k] for k in range(4)], _to(dev, sh)) \
                if embedded else None
        if quiet is not None:
            assert np.array_equal(_np(quiet), got['out'])
    assert all(torch.equal(v, buffers[k]) for k, v in layer.named_buffers())


def test_nv6_layer_in_evaluation_is_still_the_inference_kernel(dev):
    """the eval dispatch of the first family has not moved: ddk_conv_forward, the same bits as a direct call and on two calls.  On a graph whose nodes
    receive ONE message each: that kernel's scatter adds with float atomics"""
    from disco_diffdock_amd.runtime import Context
    l, offs = 3, [0, 50, 131, 132, 300]
    s = ler.shape(l, 6)
    layer = _layer(l, dev, True, 95, nv=6).eval()
    assert layer.layer == l
    rng = np.random.default_rng(951)
    E = offs[-1]
    X, SH, EA = (_to(dev, rng.standard_normal(shape).astype(np.float32)) for shape in ((E, s['din']), (E, 4), (E, 72)))
    ei = _to(dev, np.stack([rng.permutation(E), rng.integers(0, E, E)]))
    groups = list(torch.split(EA, [offs[k + 1] - offs[k] for k in range(4)]))
    with torch.no_grad():
        a, b = layer(X, ei, groups, SH), layer(X, ei, groups, SH)
    direct = Context(device=0, batch_norm=1)
    direct.load_state_dict(layer.state_dict(), prefix=f'conv_layers.{l}.')
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(direct.conv_forward(l, X, ei[0], ei[1], offs, EA, SH, s['dout'])))
