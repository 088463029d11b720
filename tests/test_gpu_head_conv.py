"""GPU tests of the head convolutions (ddk_hconv_forward / ddk_hconv_backward; csrc/k_hconv.hip): final_conv and tor_bond_conv as differentiable device
ops, through the C ABI, Context.hconv_forward / hconv_backward, tensor_layers.fused_head_conv, TensorProductConvLayer in head configuration and
heads.ScoreHeads.

Reference: the fp64 closed form tests/head_conv_ref.py (checked against fp64 autograd of oracle/e3nn_lite.py by tests/test_head_conv_host.py).
Bar: helpers.rel_err < 1e-5 PER BLOCK, the bar of tests/test_gpu_radial_tp.py and test_gpu_radial_conv.py: each output irrep slice, each of the six / two
weight blocks of grad_w2 and grad_b2, grad_x per irrep slice, grad_h.  The kernels' sums are fp32 fmaf chains of 48 / 72 terms and fixed-order sums of at
most a few hundred rows here: their rounding is far inside the bar.  The tie to the inference path uses the project's end-to-end bar, 1e-4.  The measured
figures are kept in the suite's parity-drift record (test_gpu_round3._record_drift).

Edge counts: a wave holds 64 edges (lane = edge) and a workgroup is the waves of the same 64 edges, one per weight tile, so the sizes around the tiling's
edges are E = 63, 64, 65 (tails, first edge of a second workgroup) besides the issue's 1, 31, 33, 129 (129: the first edge of a third workgroup)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import head_conv_ref as hcr
from helpers import rel_err
from oracle import e3nn_lite
from oracle import score_model_ref as smr
from test_gpu_radial_tp import SENTINEL, _guarded, _to      # the guard rows of the op these are modelled on
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig()
BAR = 1e-5
NAMES = ('grad_x', 'grad_h', 'grad_w2', 'grad_b2')
IN_IRREPS = '24x0e + 6x1o + 6x1e + 24x0o'
SH = e3nn_lite.Irreps.spherical_harmonics(1)
TOR_SH = e3nn_lite.FullTensorProduct(SH, '2e').irreps_out


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


def _slice_len(E):
    """rtp_slice_len of csrc/ddk_internal.h"""
    return max(((E + 239) // 240 + 63) // 64 * 64, 512)


def _operands(head, E, n_in, n_out, seed):
    """x, sh, h (what ReLU leaves), w2, b2, grad_out as fp32 numpy"""
    K, W = hcr.K[head], hcr.W[head]
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=f(n_in, 84), sh=f(E, 4), h=np.maximum(f(E, K), 0), w2=f(W, K) / np.float32(np.sqrt(K)), b2=f(W), g=f(n_out, hcr.DOUT[head]))


def _graph(ctx, dev, src, dst, n_in, n_out):
    return ctx.conv_graph(torch.from_numpy(np.asarray(src)).to(dev), torch.from_numpy(np.asarray(dst)).to(dev), n_in, n_out)


def _device(ctx, dev, head, graph, o, need=(True,) * 4):
    t = {k: _to(dev, v) for k, v in o.items()}
    out = ctx.hconv_forward(head, graph, t['x'], t['sh'], t['h'], t['w2'], t['b2'])
    grads = ctx.hconv_backward(head, graph, t['x'], t['sh'], t['h'], t['w2'], t['b2'], t['g'], need)
    return out.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _reference(head, src, dst, n_out, o):
    args = (head, o['x'], o['sh'], o['h'], o['w2'], o['b2'], src, dst, n_out)
    return hcr.forward(*args), hcr.vjp(*args, o['g'])


def _block_errors(head, got, want):
    """{name: rel_err} per irrep slice of out and grad_x, of grad_h, and per weight block of grad_w2 / grad_b2"""
    (out, (gx, gh, gw2, gb2)), (rout, (rx, rh, rw2, rb2)) = got, want
    errs = {'grad_h': rel_err(gh, rh)}
    for name, sl in hcr.OUT_SLICES[head].items():
        errs['out.' + name] = rel_err(out[:, sl], rout[:, sl])
    for name, sl in hcr.X_SLICES.items():
        if np.abs(rx[:, sl]).max() > 0:
            errs['grad_x.' + name] = rel_err(gx[:, sl], rx[:, sl])
        else:      # the torsion head reads neither 0e nor 0o: exact zeros, not a relative figure
            assert not gx[:, sl].any(), name
    for name, sl in hcr.weight_slices(head).items():
        errs['grad_w2.' + name] = rel_err(gw2[sl], rw2[sl])
        errs['grad_b2.' + name] = rel_err(gb2[sl], rb2[sl])
    return errs


def _assert_blocks(tag, head, got, want):
    assert got[0].shape == want[0].shape and [a.shape for a in got[1]] == [a.shape for a in want[1]]
    errs = _block_errors(head, got, want)
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'head_conv.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. both heads against the closed form on an awkward graph ------------------------------------------------------------------------------------
def _awkward_graph(E, seed):
    """n_out = 7 receivers over N = 12 nodes: receiver 6 has no edge, node 11 is read by no edge, edges 0 and 1 are one (src, dst) pair twice (receivers
    with exactly 1, 32 and 33 edges: test_receiver_edge_counts_1_32_33)"""
    N, n_out = 12, 7
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n_out - 1, E), rng.integers(0, N - 1, E)
    if E >= 2:
        src[1], dst[1] = src[0], dst[0]
    return src, dst, N, n_out


@pytest.mark.parametrize('head,E', [(h, E) for h in (0, 1) for E in (1, 31, 33, 63, 64, 65, 129)])
def test_heads_against_the_closed_form(ctx, dev, head, E):
    src, dst, N, n_out = _awkward_graph(E, 10 * E + head)
    assert (src != 6).all() and (dst != 11).all() and (E < 2 or (src[0], dst[0]) == (src[1], dst[1]))
    o = _operands(head, E, N, n_out, 100 + E + head)
    got = _device(ctx, dev, head, _graph(ctx, dev, src, dst, N, n_out), o)
    _assert_blocks(f'closed_form.h{head}.E{E}', head, got, _reference(head, src, dst, n_out, o))
    out, grads = got
    assert out.shape == (n_out, hcr.DOUT[head]) and grads[0].shape == (N, 84)      # n_out != N
    assert not out[6].any()      # the receiver without edges: exact zeros
    assert not grads[0][11].any()      # the node no edge reads


def test_receiver_edge_counts_1_32_33(ctx, dev):
    """receivers with exactly 1, 32 and 33 edges, one with none, both heads"""
    E, N, n_out = 66, 9, 4
    src = np.concatenate([[0], np.full(32, 1), np.full(33, 2)])[np.random.default_rng(1).permutation(E)]
    dst = np.random.default_rng(2).integers(0, N, E)
    assert list(np.bincount(src, minlength=n_out)) == [1, 32, 33, 0]
    for head in (0, 1):
        o = _operands(head, E, N, n_out, 150 + head)
        got = _device(ctx, dev, head, _graph(ctx, dev, src, dst, N, n_out), o)
        _assert_blocks(f'counts.h{head}', head, got, _reference(head, src, dst, n_out, o))
        assert not got[0][3].any()


def test_no_edges(ctx, dev):
    for head in (0, 1):
        o = _operands(head, 0, 5, 3, 160 + head)
        g = _graph(ctx, dev, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 5, 3)
        out, grads = _device(ctx, dev, head, g, o)
        assert out.shape == (3, hcr.DOUT[head]) and not out.any()
        assert grads[1].shape == (0, hcr.K[head]) and all(not a.any() for a in grads)


# ---- 2. the slice boundary of the parameter reduction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head,n_slices', [(h, n) for h in (0, 1) for n in (1, 2)])
def test_parameter_gradients_across_slices(ctx, dev, head, n_slices):
    E = n_slices * _slice_len(513) + 1      # one edge into the second / third slice (513 and 1 025 with a slice of 512)
    assert _slice_len(E) == _slice_len(513)
    N, n_out = 40, 9
    rng = np.random.default_rng(E + head)
    src, dst = rng.integers(0, n_out, E), rng.integers(0, N, E)
    o = _operands(head, E, N, n_out, 200 + E + head)
    got = _device(ctx, dev, head, _graph(ctx, dev, src, dst, N, n_out), o)
    _assert_blocks(f'slices.h{head}.E{E}', head, got, _reference(head, src, dst, n_out, o))


# ---- 3. output subsets, guards, the stated workspace -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', [0, 1])
def test_output_subsets(ctx, dev, head):
    E, N, n_out = 600, 30, 11      # two slices
    K, W, dout = hcr.K[head], hcr.W[head], hcr.DOUT[head]
    rng = np.random.default_rng(50 + head)
    graph = _graph(ctx, dev, rng.integers(0, n_out, E), rng.integers(0, N, E), N, n_out)
    ops = {k: _to(dev, v) for k, v in _operands(head, E, N, n_out, 500 + head).items()}
    before = {k: v.clone() for k, v in ops.items()}
    nws = ctx.L.ddk_hconv_workspace(head, E, N, n_out, 1)
    assert nws > 0 and nws % 4 == 0
    ws_full = torch.full((nws // 4 + 64,), SENTINEL, dtype=torch.float32, device=dev)      # the stated size, a guard behind it
    ws = ws_full[:nws // 4]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = ((N, 84), (E, K), (W, K), (1, W))

    def raw(need, w2=True, b2=True):
        bufs = [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        g = graph
        rc = ctx.L.ddk_hconv_backward(ctx.h, head, ptr(ops['x']), N, n_out, ptr(g.src), ptr(g.dst), ptr(g.src_order), ptr(g.src_ptr), ptr(g.dst_order),
                                      ptr(g.dst_ptr), ptr(ops['sh']), ptr(ops['h']), ptr(ops['w2']) if w2 else None, ptr(ops['b2']) if b2 else None,
                                      ptr(ops['g']), E, *[ptr(v) for _, v in bufs], ptr(ws), stream())
        return rc, bufs

    def call(need, **kw):
        rc, bufs = raw(need, **kw)
        assert rc == 0, ctx.L.ddk_last_error(ctx.h)
        torch.cuda.synchronize()
        for full, _ in bufs:
            if full is not None:      # the guard rows in front and behind still hold the sentinel
                assert bool((full[0] == SENTINEL).all()) and bool((full[-1] == SENTINEL).all())
        assert bool((ws_full[nws // 4:] == SENTINEL).all())      # nothing was written behind the workspace
        return [None if v is None else v.clone() for _, v in bufs]

    full = call((True,) * 4)
    assert all(bool((t != SENTINEL).all()) for t in full)      # every element was written
    again = call((True,) * 4)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, again))
    for need in itertools.product((False, True), repeat=4):
        if not any(need):
            continue
        part = call(need, w2=need[0] or need[1], b2=need[0])      # w2 / b2 are passed only where the rules say they are read
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(_bits(a), _bits(b)), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(ops[k], before[k]) for k in ops)      # the operands are untouched
    err = lambda: ctx.L.ddk_last_error(ctx.h)
    assert raw((False,) * 4)[0] == -1 and b'no gradient' in err()
    assert raw((True, False, False, False), w2=False)[0] == -1 and b'w2' in err()
    assert raw((True, False, False, False), b2=False)[0] == -1 and b'b2' in err()
    # the forward: guards around the output, the stated workspace with a guard behind it
    nwf = ctx.L.ddk_hconv_workspace(head, E, N, n_out, 0)
    wf_full = torch.full((nwf // 4 + 64,), SENTINEL, dtype=torch.float32, device=dev)
    obuf, out = _guarded(n_out, dout, dev)
    g = graph
    rc = ctx.L.ddk_hconv_forward(ctx.h, head, ptr(ops['x']), N, n_out, ptr(g.src), ptr(g.dst), ptr(g.src_order), ptr(g.src_ptr), ptr(ops['sh']), ptr(ops['h']),
                                 ptr(ops['w2']), ptr(ops['b2']), E, ptr(out), ptr(wf_full), stream())
    assert rc == 0, err()
    torch.cuda.synchronize()
    assert bool((obuf[0] == SENTINEL).all()) and bool((obuf[-1] == SENTINEL).all()) and bool((wf_full[nwf // 4:] == SENTINEL).all())
    assert torch.equal(_bits(out), _bits(ctx.hconv_forward(head, graph, ops['x'], ops['sh'], ops['h'], ops['w2'], ops['b2'])))
    assert ctx.L.ddk_hconv_forward(ctx.h, 2, ptr(ops['x']), N, n_out, ptr(g.src), ptr(g.dst), ptr(g.src_order), ptr(g.src_ptr), ptr(ops['sh']), ptr(ops['h']),
                                   ptr(ops['w2']), ptr(ops['b2']), E, ptr(out), ptr(wf_full), stream()) == -1 and b'head' in err()
    torch.cuda.synchronize()


# ---- 4. determinism of the ops ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', [0, 1])
def test_two_runs_give_the_same_bits(ctx, dev, head):
    E, N, n_out = 1100, 50, 6      # long segments: 180 edges per receiver, 22 per node; three slices
    rng = np.random.default_rng(70 + head)
    graph = _graph(ctx, dev, rng.integers(0, n_out, E), rng.integers(0, N, E), N, n_out)
    t = {k: _to(dev, v) for k, v in _operands(head, E, N, n_out, 700 + head).items()}
    runs = []
    for _ in range(2):
        out = ctx.hconv_forward(head, graph, t['x'], t['sh'], t['h'], t['w2'], t['b2'])
        runs.append((out,) + ctx.hconv_backward(head, graph, t['x'], t['sh'], t['h'], t['w2'], t['b2'], t['g']))
    for name, a, b in zip(('out',) + NAMES, *runs):
        assert torch.equal(_bits(a), _bits(b)), name


# ---- 5. autograd plumbing -------------------------------------------------------------------------------------------------------------------------------------
def _head_layer(head, dev, seed, batch_norm, dropout=0.0):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    torch.manual_seed(seed)
    if head == 0:
        layer = TensorProductConvLayer(IN_IRREPS, SH, '2x1o + 2x1e', 48, residual=False, dropout=dropout, batch_norm=batch_norm)
    else:
        layer = TensorProductConvLayer(IN_IRREPS, TOR_SH, '24x0o + 24x0e', 72, residual=False, dropout=dropout, batch_norm=batch_norm)
    if batch_norm:
        with torch.no_grad():
            layer.batch_norm.weight.uniform_(0.5, 1.5)
            layer.batch_norm.bias.normal_()
    return layer.to(dev)


def _layer_inputs(head, E, N, n_out, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    sh_edge = e3nn_lite.spherical_harmonics(SH, r(E, 3), normalize=True, normalization='component')
    if head == 1:      # [E, 20], as the reference passes it
        sh_edge = e3nn_lite.FullTensorProduct(SH, '2e')(sh_edge, e3nn_lite.spherical_harmonics('2e', r(E, 3), normalize=True, normalization='component'))
    src, dst = torch.randint(0, n_out, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    src[src == n_out - 1] = 0
    return r(N, 84), torch.stack([src, dst]), r(E, hcr.K[head]), sh_edge, r(n_out, hcr.DOUT[head])


@pytest.mark.parametrize('head', [0, 1])
def test_layer_gradients_against_the_oracle(dev, head):
    """batch-norm off: TensorProductConvLayer (and fused_head_conv under it) against fp64 autograd of oracle.score_model_ref.tp_conv_layer(faster=False)"""
    E, N, n_out = 90, 14, 5
    layer = _head_layer(head, dev, 80 + head, batch_norm=False).train()
    x, ei, ea, sh, g = _layer_inputs(head, E, N, n_out, 800 + head)
    P = {f'L.{k}': v.detach().cpu().double().requires_grad_() for k, v in layer.state_dict().items()}
    x64, ea64 = x.clone().requires_grad_(), ea.clone().requires_grad_()
    want = smr.tp_conv_layer(P, 'L', x64, ei, ea64, sh, IN_IRREPS, SH if head == 0 else TOR_SH, ('2x1o + 2x1e', '24x0o + 24x0e')[head], residual=False,
                             batch_norm=False, faster=False, out_nodes=n_out)
    want.backward(g)
    xd, ead = x.float().to(dev).requires_grad_(), ea.float().to(dev).requires_grad_()
    out = layer(xd, ei.to(dev), ead, sh.float().to(dev), out_nodes=n_out)
    out.backward(g.float().to(dev))
    errs = {'out': rel_err(out.detach().cpu().numpy(), want.detach().numpy()), 'node_attr': rel_err(xd.grad.cpu().numpy(), x64.grad.numpy()),
            'edge_attr': rel_err(ead.grad.cpu().numpy(), ea64.grad.numpy())}
    for k, p in layer.named_parameters():
        errs[k] = rel_err(p.grad.cpu().numpy(), P[f'L.{k}'].grad.numpy())
    print(head, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'head_conv.layer.h{head}', errs[worst], worst_block=worst, bar=BAR)
    assert set(errs) >= {'fc.0.weight', 'fc.0.bias', 'fc.4.weight', 'fc.4.bias'} and errs[worst] < BAR, (worst, errs[worst])
    # evaluation runs the same kernel under no_grad
    layer.eval()
    with torch.no_grad():
        assert torch.equal(_bits(layer(xd, ei.to(dev), ead, sh.float().to(dev), out_nodes=n_out)), _bits(out))
    # sh that asks for a gradient is refused, not answered with zeros
    with pytest.raises(RuntimeError, match='edge_sh'):
        layer(xd, ei.to(dev), ead, sh.float().to(dev).requires_grad_(), out_nodes=n_out)


def _bn_training(x, blocks, weight, bias, gy, eps=1e-5):
    """e3nn.nn.BatchNorm on the batch statistics (the formulas of tests/radial_conv_ref.batch_norm) for blocks (mul, d, scalar) in the order given, and
    its gradient, written out in fp64: (out, grad_x, grad_weight, grad_bias)"""
    out, gx, gw, gb, ix, iw, ib = [], [], [], [], 0, 0, 0
    B = x.shape[0]
    for mul, d, scalar in blocks:
        f = x[:, ix:ix + mul * d].reshape(B, mul, d)
        gyb = gy[:, ix:ix + mul * d].reshape(B, mul, d)
        w = weight[iw:iw + mul][None, :, None]
        fc = f - f.mean(axis=(0, 2), keepdims=True) if scalar else f
        norm = (fc ** 2).mean(-1).mean(0)[None, :, None]
        s = (norm + eps) ** -0.5
        y = fc * s * w
        if scalar:
            y = y + bias[ib:ib + mul][None, :, None]
            gb.append(gyb.sum(axis=(0, 2)))
            ib += mul
        gw.append((gyb * fc * s).sum(axis=(0, 2)))
        gnorm = (gyb * fc * w).sum(axis=(0, 2), keepdims=True) * -0.5 * (norm + eps) ** -1.5
        gfc = gyb * s * w + gnorm * 2 * fc / (B * d)
        if scalar:
            gfc = gfc - gfc.mean(axis=(0, 2), keepdims=True)
        out.append(y.reshape(B, mul * d))
        gx.append(gfc.reshape(B, mul * d))
        ix, iw = ix + mul * d, iw + mul
    return np.concatenate(out, 1), np.concatenate(gx, 1), np.concatenate(gw), np.concatenate(gb) if gb else np.zeros(0)


@pytest.mark.parametrize('head', [0, 1])
def test_layer_with_batch_norm_in_training(dev, head):
    """batch-norm on, training: the closed form, then e3nn's BatchNorm on the batch statistics and its gradient as tests/radial_conv_ref.py writes them"""
    import radial_conv_ref as rcr
    E, N, n_out = 120, 14, 6
    layer = _head_layer(head, dev, 90 + head, batch_norm=True).train()
    x, ei, ea, sh, g = _layer_inputs(head, E, N, n_out, 900 + head)
    src = ei[0].clone()
    src[:n_out] = torch.arange(n_out)      # every receiver has an edge: the batch statistics are those of real rows
    ei = torch.stack([src, ei[1]])
    P = {k: v.detach().cpu().double().numpy() for k, v in layer.state_dict().items()}
    sh4 = sh.numpy() if head == 0 else np.concatenate([np.zeros((E, 1)), sh.numpy()[:, :3]], 1)
    z = ea.numpy() @ P['fc.0.weight'].T + P['fc.0.bias']
    h = np.maximum(z, 0)
    args = (head, x.numpy(), sh4, h, P['fc.4.weight'], P['fc.4.bias'], ei[0].numpy(), ei[1].numpy(), n_out)
    pre = hcr.forward(*args)
    blocks = [(2, 3, False), (2, 3, False)] if head == 0 else [(24, 1, False), (24, 1, True)]      # in the order the irreps are written
    want_out, gpre, gw, gb = _bn_training(pre, blocks, P['batch_norm.weight'], P['batch_norm.bias'], g.numpy())
    # the forward is radial_conv_ref's: its blocks come in (0e, 1o, 1e, 0o) order, so the torsion head's two halves are swapped for it
    muls, perm = ((0, 2, 2, 0), np.arange(12)) if head == 0 else ((24, 0, 0, 24), np.concatenate([np.arange(24, 48), np.arange(24)]))
    wperm = np.arange(4) if head == 0 else perm
    rcr_out, rm, rv = rcr.batch_norm(pre[:, perm], muls, P['batch_norm.weight'][wperm], P['batch_norm.bias'], P['batch_norm.running_mean'],
                                     P['batch_norm.running_var'][wperm], training=True)
    assert np.abs(rcr_out[:, np.argsort(perm)] - want_out).max() < 1e-12
    gx, gh, gw2, gb2 = hcr.vjp(*args, gpre)
    gz = gh * (z > 0)
    want = {'out': want_out, 'node_attr': gx, 'edge_attr': gz @ P['fc.0.weight'], 'fc.0.weight': gz.T @ ea.numpy(), 'fc.0.bias': gz.sum(0),
            'fc.4.weight': gw2, 'fc.4.bias': gb2, 'batch_norm.weight': gw, 'batch_norm.bias': gb,
            'running_mean': rm, 'running_var': rv[np.argsort(wperm)]}
    xd, ead = x.float().to(dev).requires_grad_(), ea.float().to(dev).requires_grad_()
    out = layer(xd, ei.to(dev), ead, sh.float().to(dev), out_nodes=n_out)
    out.backward(g.float().to(dev))
    got = {'out': out.detach(), 'node_attr': xd.grad, 'edge_attr': ead.grad, **{k: p.grad for k, p in layer.named_parameters()},
           'running_mean': layer.batch_norm.running_mean, 'running_var': layer.batch_norm.running_var}
    errs = {k: rel_err(got[k].cpu().numpy(), want[k]) for k in want if want[k].size}
    print(head, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'head_conv.layer_bn.h{head}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])


def test_gather_rows_backward_is_the_segmented_sum(ctx, dev):
    """x[index] forward; backward = the rows of a node added in ascending position (ddk_seg_sum): the fp64 sum to fp32 rounding, zero rows for nodes that
    are never read, the same bits on two runs and with the list taken from a ConvGraph; 200 columns go through in two pieces"""
    from disco_diffdock_amd.tensor_layers import gather_rows
    N, E = 40, 3000      # 75 rows per node on average: where float atomics would reorder
    rng = np.random.default_rng(9)
    idx = rng.integers(0, N - 2, E)      # rows N - 2 and N - 1 are never read
    for cols in (24, 200):
        x = _to(dev, rng.standard_normal((N, cols)).astype(np.float32)).requires_grad_()
        g = rng.standard_normal((E, cols)).astype(np.float32)
        index = torch.from_numpy(idx).to(dev)
        graph = ctx.conv_graph(torch.zeros(E, dtype=torch.long, device=dev), index, N, 1)
        grads = []
        for kw in ({}, {}, {'graph': graph, 'side': 'dst'}):
            out = gather_rows(x, index, **kw)
            assert torch.equal(out, x.detach()[index])
            grads.append(torch.autograd.grad(out, x, _to(dev, g))[0])
        assert torch.equal(_bits(grads[0]), _bits(grads[1])) and torch.equal(_bits(grads[0]), _bits(grads[2]))
        want = np.zeros((N, cols))
        np.add.at(want, idx, g.astype(np.float64))
        assert rel_err(grads[0].cpu().numpy(), want) < BAR and not grads[0][N - 2:].any()
    with torch.no_grad():
        assert torch.equal(gather_rows(x, index), x[index])
    with pytest.raises(RuntimeError, match='GPU only'):
        gather_rows(x.detach().cpu(), index.cpu())


# ---- ScoreHeads ---------------------------------------------------------------------------------------------------------------------------------------------
HEAD_PREFIXES = ('center_edge_embedding.', 'final_conv.', 'tr_final_layer.', 'rot_final_layer.', 'final_edge_embedding.', 'tor_bond_conv.',
                 'tor_final_layer.', 'center_distance_expansion.', 'lig_distance_expansion.')


def _complex_batch(dev, B, t, seed=12):
    """a small synthetic complex as tests/test_gpu_model.py builds them: B noised copies, the collated batch on the device with its times set"""
    from disco_diffdock_amd import synthetic
    from test_gpu_model import _dev_batch
    c = synthetic.make_complex(seed, n_res=40, n_lig=23)
    assert int(c['edge_mask'].sum()) >= 3      # at least three rotatable bonds
    rng = np.random.default_rng(seed)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 2.0, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(B)]).astype(np.float32)
    return c, _dev_batch(c, B, pos, dev, t)


def _heads_inputs(b):
    return (b['ligand'].pos, b['ligand'].batch, b['ligand', 'ligand'].edge_index, b['ligand'].edge_mask, b.complex_t)


def _score_heads(dev, state=None, dropout=0.0):
    from disco_diffdock_amd.heads import ScoreHeads
    heads = ScoreHeads(dropout=dropout)
    if state is not None:
        res = heads.load_state_dict(state, strict=False)      # a full reference checkpoint: the other prefixes are reported, nothing is missing
        assert not res.missing_keys and res.unexpected_keys and not any(k.startswith(HEAD_PREFIXES) for k in res.unexpected_keys)
        heads.load_state_dict({k: v for k, v in state.items() if k.startswith(HEAD_PREFIXES)}, strict=True)      # filtered: strict works
    return heads.to(dev)


def test_score_heads_reproduce_the_inference_path(dev):
    """the same checkpoint in the inference model (ddk_score_forward: conv_pack.hip modes 2 / 3, k_heads.hip) and in ScoreHeads, eval mode: from the
    model's own lig_node_attr the module gives the model's tr, rot, tor.  Bar: the project's end-to-end bar, 1e-4 relative."""
    from test_gpu_model import ARGS_S, CFG as MCFG
    from functools import partial
    from disco_diffdock_amd.model_utils import get_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    P = smr.random_state_dict(MCFG, seed=7)
    model = get_model(ARGS_S, dev, partial(t_to_sigma, args=ARGS_S), no_parallel=True)
    model.score_model.load_state_dict(P, strict=True)
    heads = _score_heads(dev, P).eval()
    assert set(heads.state_dict()) == {k for k in P if k.startswith(HEAD_PREFIXES)}
    for t in (0.6, 0.15):
        c, b = _complex_batch(dev, 2, t)
        lig = model.score_model.embed(b)[0]
        tr, rot, tor = model.score_model(b)
        with torch.no_grad():
            got = heads(lig, *_heads_inputs(b))
        assert got[2].shape == tor.shape == (2 * int(c['edge_mask'].sum()),)
        errs = {n: rel_err(a.cpu().numpy(), w.cpu().numpy()) for n, a, w in zip(('tr', 'rot', 'tor'), got, (tr, rot, tor))}
        print(t, {k: f'{v:.2e}' for k, v in errs.items()})
        worst = max(errs, key=errs.get)
        _record_drift(f'head_conv.score_heads.t{t}', errs[worst], worst_block=worst, bar=1e-4)
        assert errs[worst] < 1e-4, (t, worst, errs[worst])
    # no rotatable bond, and no_torsion: the empty tor_pred the reference returns
    from disco_diffdock_amd.heads import ScoreHeads
    pos, batch, bonds, mask, ct = _heads_inputs(b)
    with torch.no_grad():
        assert heads(lig, pos, batch, bonds, torch.zeros_like(mask), ct)[2].shape == (0,)
        nt = ScoreHeads(no_torsion=True).to(dev).eval()
        assert not any(k.startswith(('tor_', 'final_edge', 'lig_distance')) for k in nt.state_dict())
        assert nt(lig, pos, batch, bonds, mask, ct)[2].shape == (0,)


def _made_up_targets(dev, B, n_rot, t, seed):
    from disco_diffdock_amd import training
    from disco_diffdock_amd.tensor_layers import _shape_context
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    tr_sigma, rot_sigma, tor_sigma = training._sigmas(_shape_context(0), t)
    return training.Targets(r(B, 3), r(B, 3), r(B, n_rot), tr_sigma, rot_sigma, tor_sigma, t, None, None, None)


def test_score_heads_training_step_is_reproducible(dev):
    """two full training steps from one state (torch.manual_seed, dropout 0.1, one SGD step): identical parameter bits"""
    from disco_diffdock_amd import training
    from disco_diffdock_amd.tensor_layers import _shape_context
    t, B = 0.4, 2
    c, b = _complex_batch(dev, B, t, seed=14)
    n_rot = int(c['edge_mask'].sum())
    P = smr.random_state_dict(CFG, seed=3)
    lig0 = torch.randn(b['ligand'].pos.shape[0], 84, generator=torch.Generator().manual_seed(5)).to(dev)
    targets = _made_up_targets(dev, B, n_rot, t, 6)

    def step():
        torch.manual_seed(1234)
        heads = _score_heads(dev, P, dropout=0.1).train()
        opt = torch.optim.SGD(heads.parameters(), lr=1e-2)
        lig = lig0.clone().requires_grad_()
        tr, rot, tor = heads(lig, *_heads_inputs(b))
        loss = training.loss_function(tr, rot, tor, targets, _shape_context(0))[0]
        loss.backward()
        grads = {k: p.grad.clone() for k, p in heads.named_parameters() if p.numel()}      # (final_conv's BatchNorm has no scalars: an empty bias)
        opt.step()
        return loss.detach(), lig.grad, grads, {k: v.detach().clone() for k, v in heads.state_dict().items()}

    a, b2 = step(), step()
    assert torch.equal(_bits(a[0]), _bits(b2[0])) and torch.equal(_bits(a[1]), _bits(b2[1]))
    for k in a[2]:
        assert torch.equal(_bits(a[2][k]), _bits(b2[2][k])), k
    for k in a[3]:
        assert torch.equal(_bits(a[3][k].float()), _bits(b2[3][k].float())), k
    moved = [k for k, p in _score_heads(dev, P).named_parameters() if p.numel() and not torch.equal(p.detach(), a[3][k])]
    assert len(moved) == len(a[2])      # the step moved every parameter


def test_end_to_end_loss_reaches_every_parameter(dev):
    """conv_stack (two layers, training) -> ScoreHeads -> training.loss_function on made-up targets -> backward(): every parameter of both has a finite,
    non-zero gradient, and a second identical run gives the same loss bits"""
    from disco_diffdock_amd import training
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer, _shape_context, conv_stack
    t, B = 0.5, 2
    c, b = _complex_batch(dev, B, t, seed=16)
    n_rot, N = int(c['edge_mask'].sum()), b['ligand'].pos.shape[0]
    P = smr.random_state_dict(CFG, seed=4)
    rng = np.random.default_rng(17)
    # the ligand's own graph for the stack: every atom to its graph's other atoms within 5 A would do; random edges inside each graph are enough here
    n = N // B
    src = np.concatenate([g * n + rng.integers(0, n, 6 * n) for g in range(B)])
    dst = np.concatenate([g * n + rng.integers(0, n, 6 * n) for g in range(B)])
    E = src.shape[0]
    sizes = [E - 3 * (E // 4), E // 4, E // 4, E // 4]
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    x0, emb0, sh = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev) for s in ((N, 60), (E, 24), (E, 4)))
    targets = _made_up_targets(dev, B, n_rot, t, 18)

    def run():
        torch.manual_seed(99)
        layers = torch.nn.ModuleList()
        for l in (2, 3):      # 60 -> 84 -> 84 columns: the last one gives the heads' input irreps
            i_irr, o_irr = CFG.conv_irreps(l)
            layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=True, dropout=0.1, faster=True,
                                           edge_groups=4)
            layer.load_state_dict(smr.random_conv_layer_params(CFG, l, 40 + l, True), strict=True)
            layers.append(layer)
        layers = layers.to(dev).train()
        heads = _score_heads(dev, P, dropout=0.1).train()
        lig = conv_stack(layers, x0.clone().requires_grad_(), ei, emb0, sizes, sh, seed=77)
        tr, rot, tor = heads(lig, *_heads_inputs(b))
        loss = training.loss_function(tr, rot, tor, targets, _shape_context(0))[0]
        loss.backward()
        return loss.detach(), {**{'stack.' + k: p.grad for k, p in layers.named_parameters()}, **{'heads.' + k: p.grad for k, p in heads.named_parameters() if p.numel()}}

    (loss_a, grads), (loss_b, _) = run(), run()
    assert torch.equal(_bits(loss_a), _bits(loss_b)) and bool(torch.isfinite(loss_a).all())
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any()), k
