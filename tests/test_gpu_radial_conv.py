"""GPU tests of the radial conv (ddk_rconv_forward / ddk_rconv_backward): node features to aggregated node features with the gather inside the radial
tensor product's kernels and the scatter-mean a fixed-order segmented sum, through the C ABI, Context.rconv_forward / rconv_backward,
tensor_layers.fused_radial_conv and TensorProductConvLayer in training.

Reference: the fp64 closed form tests/radial_conv_ref.py (tests/radial_tp_ref.py on x[dst], np.add.at over src, the mean; e3nn's BatchNorm formulas).
Bar: helpers.rel_err < 1e-5 PER BLOCK, the bar of tests/test_gpu_radial_tp.py: each irrep slice of out and grad_x, grad_sh, grad_h, each group and weight
block of grad_w2 / grad_b2.  The sums over a node's edges are short fp32 sums in a fixed order (a few hundred terms at most here): their rounding is far
inside the bar.  The measured figures are kept in the suite's parity-drift record (test_gpu_round3._record_drift)."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import radial_conv_ref as rcr
import tp_backward_ref as tpr
from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_radial_tp import SENTINEL, _block_errors, _guarded, _modules, _to      # the helpers of the op this one is built on
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig()
BAR = 1e-5
NAMES = ('grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


def _operands(l, offsets, n_in, n_out, seed):
    """x_nodes, sh, h (what ReLU leaves), w2, b2, grad_out_nodes as fp32 numpy"""
    s, E, G = tpr.shape(l), offsets[-1], len(offsets) - 1
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=f(n_in, s['din']), sh=f(E, 4), h=np.maximum(f(E, 72), 0), w2=f(G, s['W'], 72) / np.float32(np.sqrt(72.0)), b2=f(G, s['W']), g=f(n_out, s['dout']))


def _graph(ctx, dev, src, dst, n_in, n_out):
    return ctx.conv_graph(torch.from_numpy(np.asarray(src)).to(dev), torch.from_numpy(np.asarray(dst)).to(dev), n_in, n_out)


def _device(ctx, dev, l, graph, offsets, o, need=(True,) * 5):
    t = {k: _to(dev, v) for k, v in o.items()}
    out = ctx.rconv_forward(l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'])
    grads = ctx.rconv_backward(l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'], need)
    return out.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _reference(l, src, dst, n_out, offsets, o):
    args = (l, o['x'], src, dst, n_out, o['sh'], o['h'], offsets, o['w2'], o['b2'])
    return rcr.forward(*args), rcr.backward(*args, o['g'])


def _assert_blocks(tag, l, offsets, got, want):
    assert got[0].shape == want[0].shape and [a.shape for a in got[1]] == [a.shape for a in want[1]]
    errs = _block_errors(l, offsets, got, want)
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_conv.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


def _check(ctx, dev, tag, l, src, dst, n_in, n_out, offsets, seed):
    o = _operands(l, offsets, n_in, n_out, seed)
    got = _device(ctx, dev, l, _graph(ctx, dev, src, dst, n_in, n_out), offsets, o)
    _assert_blocks(tag, l, offsets, got, _reference(l, src, dst, n_out, offsets, o))
    return got


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. all five layers on one graph ---------------------------------------------------------------------------------------------------
def _awkward_graph(N, E, seed):
    """random src / dst with a node that receives nothing, one that sends nothing, a self-loop and a duplicated (src, dst) pair"""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    src[src == N - 1] = 0
    dst[dst == N - 2] = 1
    src[5] = dst[5] = 3
    src[7], dst[7] = src[6], dst[6]
    assert (src != N - 1).all() and (dst != N - 2).all() and (src == dst).any() and (src[6], dst[6]) == (src[7], dst[7])
    return src, dst


@pytest.mark.parametrize('l', range(5))
def test_layers_on_one_graph(ctx, dev, l):
    N, offs = 11, [0, 1, 1, 34, 70]      # a one-edge group, an empty group, boundaries off the tile grid
    src, dst = _awkward_graph(N, offs[-1], 5)
    out, grads = _check(ctx, dev, f'graph.l{l}', l, src, dst, N, N, offs, 100 + l)
    assert not out[N - 1].any()      # the node that receives nothing: exact zeros
    assert not grads[0][N - 2].any()      # the node that sends nothing
    assert not grads[3][1].any() and not grads[4][1].any()      # the empty group


# ---- 2. tails and workgroup boundaries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l,E', [(l, E) for l in (0, 3) for E in (1, 31, 32, 33, 129)])
def test_tails(ctx, dev, l, E):
    N = 5
    rng = np.random.default_rng(E)
    if E == 129:      # one node holds every edge, in and out: its sums cross the waves of a workgroup and two workgroups
        src, dst = np.full(E, 2), np.full(E, 4)
    else:
        src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    _check(ctx, dev, f'tails.l{l}.E{E}', l, src, dst, N, N, [0, E], 200 + 7 * l + E)


# ---- 3. n_out != n_in --------------------------------------------------------------------------------------------------------------------------
def test_other_number_of_output_nodes(ctx, dev):
    l, n_in, n_out, offs = 1, 9, 4, [0, 10, 25, 25, 50]
    rng = np.random.default_rng(31)
    src, dst = rng.integers(0, n_out, offs[-1]), rng.integers(0, n_in, offs[-1])
    dst[0], dst[1] = n_in - 1, n_out      # rows of x past n_out are read
    out, grads = _check(ctx, dev, 'n_out_4.n_in_9', l, src, dst, n_in, n_out, offs, 300)
    assert out.shape == (n_out, tpr.shape(l)['dout']) and grads[0].shape == (n_in, tpr.shape(l)['din'])


# ---- 4. the identity graph: the indexed kernels are the tested ones --------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [1, 3])
def test_identity_graph_equals_the_radial_tensor_product_bit_for_bit(ctx, dev, l):
    offs = [0, 1, 1, 34, 70]
    E = offs[-1]
    o = _operands(l, offs, E, E, 400 + l)
    t = {k: _to(dev, v) for k, v in o.items()}
    graph = _graph(ctx, dev, np.arange(E), np.arange(E), E, E)
    out = ctx.rconv_forward(l, graph, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2'])
    grads = ctx.rconv_backward(l, graph, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2'], t['g'])
    want_out = ctx.rtp_forward(l, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2'], tpr.shape(l)['dout'])
    want = ctx.rtp_backward(l, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2'], t['g'])
    assert torch.equal(_bits(out), _bits(want_out))      # a mean over one term: a division by 1
    for name, a, b in zip(NAMES, grads, want):
        assert torch.equal(_bits(a), _bits(b)), name


# ---- 5. output subsets, repeatability, three slices of the parameter pass ---------------------------------------------------------------------
def test_output_subsets(ctx, dev):
    l, N, offs = 3, 40, [0, 1300]      # 1300 edges of one group: three slices of 512
    s = tpr.shape(l)
    E, G, W = offs[-1], 1, s['W']
    rng = np.random.default_rng(50)
    graph = _graph(ctx, dev, rng.integers(0, N, E), rng.integers(0, N, E), N, N)
    ops = {k: _to(dev, v) for k, v in _operands(l, offs, N, N, 500).items()}
    before = {k: v.clone() for k, v in ops.items()}
    ws = torch.empty(ctx.L.ddk_rconv_workspace(l, E, G, N, N, 1) // 4, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    coffs = (C.c_int64 * (G + 1))(*offs)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = ((N, s['din']), (E, 4), (E, 72), (G * W, 72), (G, W))

    def raw(need, w2=True, b2=True):
        bufs = [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        g = graph
        rc = ctx.L.ddk_rconv_backward(ctx.h, l, ptr(ops['x']), N, N, ptr(g.src), ptr(g.dst), ptr(g.src_order), ptr(g.src_ptr), ptr(g.dst_order), ptr(g.dst_ptr),
                                      ptr(ops['sh']), ptr(ops['h']), coffs, G, ptr(ops['w2']) if w2 else None, ptr(ops['b2']) if b2 else None, ptr(ops['g']), E,
                                      *[ptr(v) for _, v in bufs], ptr(ws), stream())
        return rc, bufs

    def call(need, **kw):
        rc, bufs = raw(need, **kw)
        assert rc == 0, ctx.L.ddk_last_error(ctx.h)
        torch.cuda.synchronize()
        for full, _ in bufs:
            if full is not None:      # the guard rows in front and behind still hold the sentinel
                assert bool((full[0] == SENTINEL).all()) and bool((full[-1] == SENTINEL).all())
        return [None if v is None else v.clone() for _, v in bufs]

    full = call((True,) * 5)
    assert all(bool((t != SENTINEL).all()) for t in full)      # every element was written
    again = call((True,) * 5)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, again))      # two full calls: the same bits
    for need in itertools.product((False, True), repeat=5):
        if not any(need):
            continue
        part = call(need, w2=any(need[:3]), b2=need[0] or need[1])      # w2 / b2 are passed only where the rules say they are read
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(_bits(a), _bits(b)), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(ops[k], before[k]) for k in ops)      # the operands are untouched
    err = lambda: ctx.L.ddk_last_error(ctx.h)
    assert raw((False,) * 5)[0] == -1 and b'no gradient' in err()
    assert raw((True, False, False, False, False), w2=False)[0] == -1 and b'w2' in err()
    assert raw((False, True, False, False, False), b2=False)[0] == -1 and b'b2' in err()
    torch.cuda.synchronize()


# ---- 6. no edges --------------------------------------------------------------------------------------------------------------------------------
def test_no_edges(ctx, dev):
    l, n_in, n_out = 3, 6, 4
    s = tpr.shape(l)
    graph = _graph(ctx, dev, np.zeros(0, np.int64), np.zeros(0, np.int64), n_in, n_out)
    for offs in ([0, 0], [0, 0, 0, 0, 0]):
        G = len(offs) - 1
        out, (gx, gsh, gh, gw2, gb2) = _device(ctx, dev, l, graph, offs, _operands(l, offs, n_in, n_out, 1))
        assert out.shape == (n_out, s['dout']) and not out.any()
        assert gx.shape == (n_in, s['din']) and not gx.any() and gsh.shape == (0, 4) and gh.shape == (0, 72)
        assert gw2.shape == (G, s['W'], 72) and gb2.shape == (G, s['W']) and not gw2.any() and not gb2.any()
    # the C entries themselves write the zeros, with no operands, no tables and no workspace
    full = lambda *shape: torch.full(shape, 7.0, device=dev)
    out, gx, gw2, gb2 = full(n_out, s['dout']), full(n_in, s['din']), full(s['W'], 72), full(s['W'])
    p = lambda t: C.c_void_p(t.data_ptr())
    offs, stream = (C.c_int64 * 2)(0, 0), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ctx.L.ddk_rconv_forward(ctx.h, l, None, n_in, n_out, None, None, None, None, None, None, offs, 1, None, None, 0, p(out), None, stream)
    assert rc == 0, ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_rconv_backward(ctx.h, l, None, n_in, n_out, None, None, None, None, None, None, None, None, offs, 1, None, None, None, 0,
                                  p(gx), None, None, p(gw2), p(gb2), None, stream)
    assert rc == 0, ctx.L.ddk_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not out.any() and not gx.any() and not gw2.any() and not gb2.any()


@pytest.mark.parametrize('bn', [False, True])
def test_layer_in_training_without_edges_returns_the_padded_input(dev, bn):
    layer = _layer(0, dev, bn, 60).train()
    s = tpr.shape(0)
    x = torch.randn(7, s['din'], device=dev)
    out = layer(x, torch.zeros(2, 0, dtype=torch.long, device=dev), [torch.zeros(0, 72, device=dev)] * 4, torch.zeros(0, 4, device=dev))
    assert out.shape == (7, s['dout']) and torch.equal(out[:, :s['din']], x) and not out[:, s['din']:].any()      # (reference: no BatchNorm without edges)


# ---- 7. fused_radial_conv against the composition it replaces --------------------------------------------------------------------------------------
def _fp64_fc(l, offs, fc, ea):
    """fp64 numpy: fc[k][0] -> ReLU; the parameters, the pre-activation z, h and the stacked last Linears"""
    P = [{n: p.detach().cpu().numpy().astype(np.float64) for n, p in blk.named_parameters()} for blk in fc]
    ea64 = ea.astype(np.float64)
    z = np.concatenate([ea64[offs[k]:offs[k + 1]] @ P[k]['0.weight'].T + P[k]['0.bias'] for k in range(4)])
    return P, ea64, z, np.maximum(z, 0), np.stack([p['4.weight'] for p in P]), np.stack([p['4.bias'] for p in P])


def _fp64_fc_grads(offs, P, ea64, z, gh, gw2, gb2):
    gz, want = gh * (z > 0), {}
    for k in range(4):
        sl = slice(offs[k], offs[k + 1])
        want[f'fc.{k}.4.weight'], want[f'fc.{k}.4.bias'] = gw2[k], gb2[k]
        want[f'fc.{k}.0.weight'], want[f'fc.{k}.0.bias'] = gz[sl].T @ ea64[sl], gz[sl].sum(0)
        want[f'edge_attr.{k}'] = gz[sl] @ P[k]['0.weight']
    return want


def _composition(tp, fc, X, SH, EA, src, dst, n_out):
    """what fused_radial_conv replaces: index_select + fused_radial_tp + index_add_ / count"""
    from disco_diffdock_amd.tensor_layers import fused_radial_tp
    rows = fused_radial_tp(tp, fc, X.index_select(0, dst), SH, EA)
    count = torch.bincount(src, minlength=n_out).clamp(min=1).to(rows.dtype)
    return torch.zeros(n_out, rows.shape[1], device=rows.device).index_add_(0, src, rows) / count[:, None]


@pytest.mark.parametrize('l', [1, 3])
def test_fused_radial_conv_against_the_composition(ctx, dev, l, monkeypatch):
    from disco_diffdock_amd.tensor_layers import fused_radial_conv
    offs, s, N = [0, 50, 131, 132, 300], tpr.shape(l), 40
    E = offs[-1]
    tp, fc = _modules(l, dev, 70 + l)
    rng = np.random.default_rng(700 + l)
    x, sh, ea, g = (rng.standard_normal((n, c)).astype(np.float32) for n, c in ((N, s['din']), (E, 4), (E, 72), (N, s['dout'])))
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    graph = ctx.conv_graph(ei[0], ei[1], N, N)
    leaves = lambda: (_to(dev, x).requires_grad_(True), _to(dev, sh).requires_grad_(True), [_to(dev, ea[offs[k]:offs[k + 1]]).requires_grad_(True) for k in range(4)])

    def run(fused):
        fc.zero_grad(set_to_none=True)
        X, SH, EA = leaves()
        out = fused_radial_conv(tp, fc, X, ei, SH, EA, graph=graph) if fused else _composition(tp, fc, X, SH, EA, ei[0], ei[1], N)
        assert out.shape == (N, s['dout']) and out.grad_fn is not None
        out.backward(_to(dev, g))
        got = {'out': out.detach(), 'node_attr': X.grad, 'edge_sh': SH.grad}
        got.update({f'edge_attr.{k}': EA[k].grad for k in range(4)})
        got.update({'fc.' + n: p.grad for n, p in fc.named_parameters()})
        assert all(v is not None for v in got.values())
        return {k: v.cpu().numpy() for k, v in got.items()}

    fused, plain = run(True), run(False)
    P, ea64, z, h, w2, b2 = _fp64_fc(l, offs, fc, ea)
    gxn, gsh, gh, gw2, gb2 = rcr.backward(l, x, src, dst, N, sh, h, offs, w2, b2, g)
    want = {'out': rcr.forward(l, x, src, dst, N, sh, h, offs, w2, b2), 'node_attr': gxn, 'edge_sh': gsh}
    want.update(_fp64_fc_grads(offs, P, ea64, z, gh, gw2, gb2))
    assert set(fused) == set(plain) == set(want) and len(want) == 3 + 4 + 16
    errs = {}
    for k in want:
        assert fused[k].shape == plain[k].shape == want[k].shape, k
        errs[k + '.vs_composition'] = rel_err(fused[k], plain[k])
        errs[k + '.vs_fp64'] = rel_err(fused[k], want[k])
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_conv.fused.l{l}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])
    again = run(True)
    assert all(np.array_equal(again[k], fused[k]) for k in fused)      # the same bits again, every gradient

    # the graph is built from edge_index when none is given: the same bits
    X, SH, EA = leaves()
    built = fused_radial_conv(tp, fc, X, ei, SH, EA)
    assert np.array_equal(built.detach().cpu().numpy(), fused['out'])

    # under no_grad only the forward runs, with the same bits
    with torch.no_grad():
        quiet = fused_radial_conv(tp, fc, _to(dev, x), ei, _to(dev, sh), [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)], graph=graph)
    assert quiet.grad_fn is None and not quiet.requires_grad and np.array_equal(quiet.cpu().numpy(), fused['out'])

    # a frozen last Linear: no parameter pass is asked of the kernel, the other gradients are the same bits
    asked = []
    real = ctx.rconv_backward
    monkeypatch.setattr(ctx, 'rconv_backward', lambda *a: asked.append(tuple(a[-1])) or real(*a))
    for blk in fc:
        blk[4].requires_grad_(False)
    fc.zero_grad(set_to_none=True)
    X, SH, EA = leaves()
    fused_radial_conv(tp, fc, X, ei, SH, EA, graph=graph).backward(_to(dev, g))
    assert asked == [(True, True, True, False, False)]
    assert all(blk[4].weight.grad is None and blk[4].bias.grad is None for blk in fc)
    assert np.array_equal(X.grad.cpu().numpy(), fused['node_attr']) and np.array_equal(SH.grad.cpu().numpy(), fused['edge_sh'])
    for k in range(4):
        assert np.array_equal(EA[k].grad.cpu().numpy(), fused[f'edge_attr.{k}']) and np.array_equal(fc[k][0].weight.grad.cpu().numpy(), fused[f'fc.{k}.0.weight'])
    monkeypatch.undo()
    for blk in fc:
        blk[4].requires_grad_(True)

    # a double backward raises instead of giving zeros
    X, SH, EA = leaves()
    (gx,) = torch.autograd.grad(fused_radial_conv(tp, fc, X, ei, SH, EA, graph=graph), X, _to(dev, g), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with pytest.raises(RuntimeError, match='GPU only'):
        fused_radial_conv(tp, fc, torch.from_numpy(x), ei.cpu(), torch.from_numpy(sh), [torch.from_numpy(ea[offs[k]:offs[k + 1]]) for k in range(4)])


# ---- 8. the layer in training -----------------------------------------------------------------------------------------------------------------
def _layer(l, dev, bn, seed):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    i_irr, o_irr = CFG.conv_irreps(l)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=bn, dropout=0.0, faster=True, edge_groups=4)
    layer.load_state_dict(smr.random_conv_layer_params(CFG, l, seed, bn), strict=True)
    return layer.to(dev)


def _bn_train_fp64(x, muls, weight, bias):
    """e3nn's BatchNorm on the batch statistics, written once more in torch fp64 for autograd: per block, scalars lose their mean and get the bias,
    every channel is divided by the root of its mean square over batch and components"""
    cols, ix, iw, ib = [], 0, 0, 0
    for k, (mul, d) in enumerate(zip(muls, (1, 3, 3, 1))):
        if not mul:
            continue
        f = x[:, ix:ix + mul * d].reshape(x.shape[0], mul, d)
        if k == 0:
            f = f - f.sum(dim=(0, 2), keepdim=True) / (x.shape[0] * d)
        ms = (f * f).sum(dim=(0, 2), keepdim=True) / (x.shape[0] * d)
        f = f / torch.sqrt(ms + 1e-5) * weight[iw:iw + mul].reshape(1, mul, 1)
        if k == 0:
            f = f + bias[ib:ib + mul].reshape(1, mul, 1)
            ib += mul
        ix, iw = ix + mul * d, iw + mul
        cols.append(f.reshape(x.shape[0], mul * d))
    return torch.cat(cols, dim=1)


def _layer_case(l, dev, seed):
    offs, s, N = [0, 50, 131, 132, 300], tpr.shape(l), 40
    rng = np.random.default_rng(seed)
    E = offs[-1]
    x, sh, ea, g = (rng.standard_normal((n, c)).astype(np.float32) for n, c in ((N, s['din']), (E, 4), (E, 72), (N, s['dout'])))
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    return offs, s, N, x, sh, ea, g, src, dst


@pytest.mark.parametrize('l,bn', [(0, False), (0, True), (3, False), (3, True)])
def test_layer_in_training_against_fp64(dev, l, bn):
    offs, s, N, x, sh, ea, g, src, dst = _layer_case(l, dev, 800 + l)
    layer = _layer(l, dev, bn, 80 + l).train()
    muls = s['O']
    buffers = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in layer.named_buffers()}
    X = _to(dev, x).requires_grad_(True)
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    out = layer(X, ei, [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)], _to(dev, sh))
    out.backward(_to(dev, g))
    got = {'out': out.detach(), 'node_attr': X.grad}
    got.update({n: p.grad for n, p in layer.named_parameters()})
    got.update({n: b.detach() for n, b in layer.named_buffers()})
    assert all(v is not None for v in got.values())
    got = {k: v.cpu().numpy() for k, v in got.items()}

    # fp64: the closed form, the BatchNorm formulas (their gradient by autograd of _bn_train_fp64), the residual
    P, ea64, z, h, w2, b2 = _fp64_fc(l, offs, layer.fc, ea)
    agg = rcr.forward(l, x, src, dst, N, sh, h, offs, w2, b2)
    g64, want = g.astype(np.float64), {}
    if bn:
        A = torch.from_numpy(agg).requires_grad_(True)
        Wt, Bt = (layer.batch_norm.weight.detach().cpu().double().requires_grad_(True), layer.batch_norm.bias.detach().cpu().double().requires_grad_(True))
        y = _bn_train_fp64(A, muls, Wt, Bt)
        y.backward(torch.from_numpy(g64))
        y, g_agg = y.detach().numpy(), A.grad.numpy()
        want['batch_norm.weight'], want['batch_norm.bias'] = Wt.grad.numpy(), Bt.grad.numpy()
        mine, want['batch_norm.running_mean'], want['batch_norm.running_var'] = rcr.batch_norm(
            agg, muls, Wt.detach().numpy(), Bt.detach().numpy(), buffers['batch_norm.running_mean'], buffers['batch_norm.running_var'], training=True)
        assert np.abs(mine - y).max() < 1e-10      # the two fp64 texts of the formulas agree
    else:
        y, g_agg = agg, g64
    want['out'] = y + np.pad(x.astype(np.float64), ((0, 0), (0, s['dout'] - s['din'])))
    gxn, _, gh, gw2, gb2 = rcr.backward(l, x, src, dst, N, sh, h, offs, w2, b2, g_agg)
    want['node_attr'] = gxn + g64[:, :s['din']]
    want.update({k: v for k, v in _fp64_fc_grads(offs, P, ea64, z, gh, gw2, gb2).items() if k.startswith('fc.')})
    assert set(got) == set(want) and len(want) == 2 + 16 + (4 if bn else 0)
    errs = {k: rel_err(got[k], want[k]) for k in want}
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_conv.layer_training.l{l}.bn{int(bn)}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])


@pytest.mark.parametrize('l', range(5))
def test_training_step_is_reproducible(dev, l):
    """layer.train(), forward, loss.backward(), optimizer.step() for every layer shape; two such steps from the same state: bit-identical parameters"""
    offs, s, N, x, sh, ea, g, src, dst = _layer_case(l, dev, 900 + l)
    start = _layer(l, dev, True, 90 + l)
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)

    def step():
        layer = copy.deepcopy(start).train()
        opt = torch.optim.SGD(layer.parameters(), lr=0.05)
        out = layer(_to(dev, x), ei, [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)], _to(dev, sh))
        (out * _to(dev, g)).sum().backward()
        opt.step()
        return {k: v.detach().clone() for k, v in layer.state_dict().items()}

    a, b = step(), step()
    assert a.keys() == b.keys() and len(a) == 20
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert not torch.equal(a[k], start.state_dict()[k]), k      # the step moved it


# ---- 9. the training path agrees with the inference kernel ----------------------------------------------------------------------------------------
def test_training_path_agrees_with_the_inference_kernel(dev):
    from disco_diffdock_amd.runtime import Context
    from disco_diffdock_amd.tensor_layers import fused_radial_conv
    l = 3
    offs, s, N, x, sh, ea, g, src, dst = _layer_case(l, dev, 950)
    layer = _layer(l, dev, True, 95).eval()      # random weights, running buffers that are not the initial ones
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    X, SH, EA = _to(dev, x), _to(dev, sh), [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)]
    with torch.no_grad():
        inference = layer(X, ei, EA, SH)
        trained_path = layer.batch_norm(fused_radial_conv(layer.tp, layer.fc, X, ei, SH, EA)) + torch.nn.functional.pad(X, (0, s['dout'] - s['din']))
    err = rel_err(trained_path.cpu().numpy(), inference.cpu().numpy())
    _record_drift('radial_conv.training_path_vs_inference.l3', err, bar=1e-4)
    assert err < 1e-4, err      # the bar of the conv goldens; the inference kernel carries its operands as f16 limbs, so not the same bits
    # eval mode itself returns what it returned: ddk_conv_forward, bit for bit.  On a graph whose nodes receive ONE message each: that kernel's scatter adds
    # with float atomics, so where a node's sum has several terms two of its own runs differ in the last bits
    rng = np.random.default_rng(951)
    E = offs[-1]
    X1 = _to(dev, rng.standard_normal((E, s['din'])).astype(np.float32))
    ei1 = torch.from_numpy(np.stack([rng.permutation(E), rng.integers(0, E, E)])).to(dev)
    with torch.no_grad():
        inference = layer(X1, ei1, EA, SH)
    ctx = Context(device=0, batch_norm=1)
    ctx.load_state_dict(layer.state_dict(), prefix=f'conv_layers.{l}.')
    direct = ctx.conv_forward(l, X1, ei1[0], ei1[1], offs, torch.cat(EA), SH, s['dout'])
    assert torch.equal(_bits(direct), _bits(inference))
    with pytest.raises(RuntimeError, match="reduce='mean'"):
        layer(X, ei, EA, SH, reduce='sum')
    with pytest.raises(RuntimeError, match="reduce='mean'"):
        layer(X, ei, EA, SH, out_nodes=N - 1)


# ---- 10. memory: neither x_dst nor the tensor product's rows are kept for the backward -----------------------------------------------------------
def test_peak_memory_is_below_the_composition(ctx, dev):
    from disco_diffdock_amd.tensor_layers import fused_radial_conv
    l, E, N = 3, 50000, 2000
    s = tpr.shape(l)
    offs = [0, 12500, 25000, 37500, E]
    tp, fc = _modules(l, dev, 80)
    gen = torch.Generator(device=dev).manual_seed(81)
    x, sh, ea, g = (torch.randn(n, c, device=dev, generator=gen) for n, c in ((N, s['din']), (E, 4), (E, 72), (N, s['dout'])))
    ei = torch.randint(0, N, (2, E), device=dev, generator=gen)
    graph = ctx.conv_graph(ei[0], ei[1], N, N)

    def peak(fused):
        fc.zero_grad(set_to_none=True)
        X, SH = x.clone().requires_grad_(True), sh.clone().requires_grad_(True)
        EA = [ea[offs[k]:offs[k + 1]].clone().requires_grad_(True) for k in range(4)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        out = fused_radial_conv(tp, fc, X, ei, SH, EA, graph=graph) if fused else _composition(tp, fc, X, SH, EA, ei[0], ei[1], N)
        out.backward(g)
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - live
        grad = X.grad.clone()
        del out, X, SH, EA
        return used, grad

    fused, gf = peak(True)
    plain, gp = peak(False)
    one_rows = 4 * E * s['dout']
    print(f'peak bytes over forward + backward: radial conv {fused}, composition {plain}, one [E, Dout] tensor {one_rows}')
    _record_drift('radial_conv.peak_memory.l3.E50000', fused / one_rows, composition=plain / one_rows, bar=plain / one_rows)
    assert fused < plain, (fused, plain)
    assert rel_err(gf.cpu().numpy(), gp.cpu().numpy()) < BAR
