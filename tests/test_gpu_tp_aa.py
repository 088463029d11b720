"""GPU tests of the third shape family of the radial tensor product and the radial conv: the all-atom (confidence) model's conv layers, e3nn's
FullyConnectedTensorProduct(in, 1x0e + 1x1o + 1x2e, out) with the weights in e3nn's instruction order (the `layer` ids DDK_TP_AA + l, sh rows of 9 floats),
and TensorProductConvLayer in the all-atom configuration.

Reference: the closed form restated in fp64 numpy (tests/confidence_conv_ref.py), which tests/test_confidence_conv_host.py holds against
oracle.e3nn_lite.FullyConnectedTensorProduct to 1e-12.  Bar: helpers.rel_err < 1e-5 PER BLOCK (each irrep slice of out and grad_x, grad_h, each e3nn
instruction's slice of grad_w2 / grad_b2 per group), the bar of the nv = 6 and nv = 4 tests of the same kernels (tests/test_gpu_tp_nv4.py): the arithmetic
is the same fp32 fmaf / fp32-MFMA chains.  The graphs and group tables are those tests'.  The layer's bar is 1e-5 per tensor."""
import numpy as np
import pytest
import torch

import confidence_conv_ref as ccr
from helpers import rel_err
from test_gpu_radial_conv import _awkward_graph, _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
BAR = 1e-5
AA = 16      # DDK_TP_AA
IRREPS = ['24x0e', '24x0e+6x1o', '24x0e+6x1o+6x1e', '24x0e+6x1o+6x1e+24x0o']
SH = '1x0e+1x1o+1x2e'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.runtime import TP_AA
    from disco_diffdock_amd.tensor_layers import _shape_context
    assert TP_AA == AA
    return _shape_context(0)      # a shape-only context: no weights loaded


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _block_errors(s, offsets, got_out, got, want_out, want):
    """rel_err per block: out / grad_x per irrep slice, grad_h, grad_w2 / grad_b2 per group and e3nn instruction"""
    errs = {}
    for name, sl in ccr.out_slices(s).items():
        errs[f'out.{name}'] = rel_err(got_out[:, sl], want_out[:, sl])
    for name, sl in ccr.in_slices(s).items():
        errs[f'grad_x.{name}'] = rel_err(got['x'][:, sl], want['x'][:, sl])
    if want['h'].size:
        errs['grad_h'] = rel_err(got['h'], want['h'])
    for name, sl in ccr.weight_slices(s).items():
        for g in range(len(offsets) - 1):
            if offsets[g + 1] > offsets[g]:
                errs[f'grad_w2.g{g}.{name}'] = rel_err(got['w2'][g, sl], want['w2'][g, sl])
                errs[f'grad_b2.g{g}.{name}'] = rel_err(got['b2'][g, sl], want['b2'][g, sl])
    return errs


def _assert_blocks(tag, errs):
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'tp_aa.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


# ---- 1. the radial tensor product and the radial conv ---------------------------------------------------------------------------------------------------------
def _radial_operands(s, offsets, n_in, n_out, seed, per_edge, y2_only=False):
    E, G = offsets[-1], len(offsets) - 1
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    o = dict(x=f(E if per_edge else n_in, s['din']), sh=f(E, 9), h=np.maximum(f(E, 72), 0), w2=f(G, s['W'], 72) / np.float32(np.sqrt(72.0)), b2=f(G, s['W']),
             g=f(E if per_edge else n_out, s['dout']))
    if y2_only:      # only the two l = 2 paths act
        o['sh'][:, :4] = 0
    return o


NAMES = ('x', 'h', 'w2', 'b2')
NEED = (True, False, True, True, True)      # grad_sh is not implemented for this family


def _grads(full):
    assert full[1] is None
    return [full[0], full[2], full[3], full[4]]


def _same_bits_alone(full, alone_of):
    """each gradient asked for alone: the same bits as when all are asked for"""
    for k in (0, 2, 3, 4):
        need = tuple(i == k for i in range(5))
        alone = alone_of(need)
        assert [a is not None for a in alone] == list(need)
        assert torch.equal(_bits(alone[k]), _bits(full[k])), k


def _check_rtp(ctx, dev, tag, l, offsets, seed, y2_only=False):
    s = ccr.shape(l)
    o = _radial_operands(s, offsets, 0, 0, seed, True, y2_only)
    t = {k: _to(dev, v) for k, v in o.items()}
    back = lambda need: ctx.rtp_backward(AA + l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'], need)
    run = lambda: (ctx.rtp_forward(AA + l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], s['dout']), back(NEED))
    out, full = run()
    want_out, want = ccr.rtp(l, o['x'], o['sh'], o['h'], offsets, o['w2'], o['b2'], o['g'])
    _assert_blocks(tag, _block_errors(s, offsets, _np(out), dict(zip(NAMES, map(_np, _grads(full)))), want_out, want))
    out2, full2 = run()
    assert torch.equal(_bits(out), _bits(out2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_grads(full), _grads(full2)))      # two runs: the same bits
    _same_bits_alone(full, back)
    return _np(out), [_np(a) for a in _grads(full)]


def _check_rconv(ctx, dev, tag, l, src, dst, n_in, n_out, offsets, seed, y2_only=False):
    s = ccr.shape(l)
    o = _radial_operands(s, offsets, n_in, n_out, seed, False, y2_only)
    t = {k: _to(dev, v) for k, v in o.items()}
    graph = ctx.conv_graph(_to(dev, np.asarray(src)), _to(dev, np.asarray(dst)), n_in, n_out)
    back = lambda need: ctx.rconv_backward(AA + l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'], need)
    run = lambda: (ctx.rconv_forward(AA + l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2']), back(NEED))
    out, full = run()
    assert out.shape == (n_out, s['dout']) and full[0].shape == (n_in, s['din'])
    want_out, want = ccr.rconv(l, o['x'], src, dst, n_out, o['sh'], o['h'], offsets, o['w2'], o['b2'], o['g'])
    _assert_blocks(tag, _block_errors(s, offsets, _np(out), dict(zip(NAMES, map(_np, _grads(full)))), want_out, want))
    out2, full2 = run()
    assert torch.equal(_bits(out), _bits(out2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_grads(full), _grads(full2)))
    _same_bits_alone(full, back)
    return _np(out), [_np(a) for a in _grads(full)]


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_on_the_awkward_graph(ctx, dev, l):
    N, offs = 11, [0, 1, 1, 34, 70]      # a one-edge group, an empty group, boundaries off the tile grid
    src, dst = _awkward_graph(N, offs[-1], 5)      # a self-loop, a duplicated edge, a node that receives nothing, one that sends nothing
    _, grads = _check_rtp(ctx, dev, f'rtp.graph.l{l}', l, offs, 100 + l)
    assert not grads[2][1].any() and not grads[3][1].any()      # the empty group: exact zeros
    out, grads = _check_rconv(ctx, dev, f'rconv.graph.l{l}', l, src, dst, N, N, offs, 100 + l)
    assert not out[N - 1].any()      # the node that receives nothing: exact zeros
    assert not grads[0][N - 2].any()      # the node that sends nothing
    assert not grads[2][1].any() and not grads[3][1].any()      # the empty group


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_with_the_second_order_columns_alone(ctx, dev, l):
    """sh[:, :4] = 0: only 1o (x) 2e -> 1o and 1e (x) 2e -> 1e act (layer 0 has neither: exact zeros)"""
    N, offs = 11, [0, 1, 1, 34, 70]
    src, dst = _awkward_graph(N, offs[-1], 5)
    if l == 0:
        s = ccr.shape(0)
        o = {k: _to(dev, v) for k, v in _radial_operands(s, offs, 0, 0, 150, True, True).items()}
        assert not _np(ctx.rtp_forward(AA, o['x'], o['sh'], o['h'], offs, o['w2'], o['b2'], s['dout'])).any()
        return
    out, _ = _check_rtp(ctx, dev, f'rtp.y2.l{l}', l, offs, 150 + l, True)
    assert out.any()
    _check_rconv(ctx, dev, f'rconv.y2.l{l}', l, src, dst, N, N, offs, 150 + l, True)


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
    _check_rtp(ctx, dev, f'rtp.groups.l{l}', l, offs, 300 + l)
    _check_rconv(ctx, dev, f'rconv.n_out_4.n_in_9.l{l}', l, src, dst, n_in, n_out, offs, 300 + l)


@pytest.mark.parametrize('l', range(4))
def test_radial_ops_across_a_slice_of_the_parameter_pass(ctx, dev, l):
    N, offs = 40, [0, 600]      # one group of 600 edges: the parameter pass crosses a 512-edge slice
    rng = np.random.default_rng(60 + l)
    _check_rtp(ctx, dev, f'rtp.slices.l{l}', l, offs, 600 + l)
    _check_rconv(ctx, dev, f'rconv.slices.l{l}', l, rng.integers(0, N, 600), rng.integers(0, N, 600), N, N, offs, 600 + l)


def test_refusals_name_the_family(ctx, dev):
    from disco_diffdock_amd.runtime import Context
    s = ccr.shape(0)
    x, sh, h = torch.randn(3, s['din'], device=dev), torch.randn(3, 9, device=dev), torch.randn(3, 72, device=dev)
    w2, b2, w, g = torch.randn(1, s['W'], 72, device=dev), torch.randn(1, s['W'], device=dev), torch.randn(3, s['W'], device=dev), torch.randn(3, s['dout'], device=dev)
    # the per-edge-weight entries refuse the ids by name
    with pytest.raises(RuntimeError, match='all-atom family'):
        ctx.tp_forward(AA, x, sh[:, :4].contiguous(), w, s['dout'])
    with pytest.raises(RuntimeError, match='all-atom family'):
        ctx.tp_backward(AA, x, sh[:, :4].contiguous(), w, g)
    # grad_sh asked for
    with pytest.raises(RuntimeError, match='grad_sh is not implemented for the all-atom family'):
        ctx.rtp_backward(AA, x, sh, h, [0, 3], w2, b2, g)
    graph = ctx.conv_graph(torch.tensor([0, 1, 2], device=dev), torch.tensor([2, 1, 0], device=dev), 3, 3)
    with pytest.raises(RuntimeError, match='grad_sh is not implemented for the all-atom family'):
        ctx.rconv_backward(AA, graph, x, sh, h, [0, 3], w2, b2, g)
    # ids next to the table
    one = torch.zeros(4096, device=dev)
    import ctypes
    offs = (ctypes.c_int64 * 2)(0, 1)
    for bad in (15, 21):
        p = one.data_ptr()
        assert ctx.L.ddk_rtp_forward(ctx.h, bad, p, p, p, offs, 1, p, p, 1, p, None) != 0
        msg = ctx.L.ddk_last_error(ctx.h).decode()
        assert 'DDK_TP_AA' in msg and 'all-atom family' in msg, msg
    # the ids name a shape, not a context's layer.  A context holds at most 16 conv layers (indices 0..15: the all-atom model's 45 convs are nine groups
    # of each of its five), so no context that can be created has a layer 16: one of 45 is refused at creation, and the largest one serves the id as the shape
    with pytest.raises(RuntimeError, match='num_conv_layers must be in'):
        Context(device=0, num_conv_layers=45)
    big = Context(device=0, num_conv_layers=16)
    big.finalize()
    assert torch.equal(_bits(big.rtp_forward(AA, x, sh, h, [0, 3], w2, b2, s['dout'])), _bits(ctx.rtp_forward(AA, x, sh, h, [0, 3], w2, b2, s['dout'])))
    # sh rows of 4 floats with these ids
    with pytest.raises(RuntimeError, match=r'sh \[E, 9\]'):
        ctx.rtp_forward(AA, x, sh[:, :4].contiguous(), h, [0, 3], w2, b2, s['dout'])


# ---- 2. TensorProductConvLayer in the all-atom configuration --------------------------------------------------------------------------------------------------
def _layer(l, dev, bn, seed, dropout=0.0):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    layer = TensorProductConvLayer(IRREPS[l], SH, IRREPS[min(l + 1, 3)], 72, residual=False, batch_norm=bn, dropout=dropout, faster=False, edge_groups=1)
    want = {'fc.0.weight', 'fc.0.bias', 'fc.3.weight', 'fc.3.bias'} | ({'batch_norm.weight', 'batch_norm.bias', 'batch_norm.running_mean', 'batch_norm.running_var'} if bn else set())
    assert set(layer.state_dict()) == want and layer.layer == AA + l
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in layer.state_dict().items():      # parameters and buffers away from their initial values (running_var positive)
            r = torch.randn(p.shape, generator=g)
            p.copy_(0.5 + r.abs() if k.endswith('running_var') or k == 'batch_norm.weight' else r * (0.3 if 'fc.' in k else 1.0))
    return layer.to(dev)


def _layer_case(l, seed, n_in, n_out, E):
    s = ccr.shape(l)
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    ei = np.stack([rng.integers(0, n_out, E), rng.integers(0, n_in, E)])
    return dict(send=f(n_in, s['din']), recv=f(n_out, s['din']), sh=f(E, 9), emb=f(E, 24), ea=f(E, 72), g=f(n_out, s['dout']), ei=ei)


def _layer_fp64(layer, l, c, bn, training, embedded):
    P = {k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    for k, _ in layer.named_parameters():
        P[k].requires_grad_(True)
    send, recv = (torch.from_numpy(c[k]).double().requires_grad_(True) for k in ('send', 'recv'))
    out, stats = ccr.layer_fp64(P, l, bn, training, send, recv, torch.from_numpy(c['ei']), torch.from_numpy(c['sh']).double(),
                                emb=torch.from_numpy(c['emb']).double() if embedded else None, edge_attr=None if embedded else torch.from_numpy(c['ea']).double())
    out.backward(torch.from_numpy(c['g']).double())
    want = {'out': out.detach().numpy()}
    if c['ei'].shape[1]:
        want['send'] = send.grad.numpy()
        if embedded:
            want['recv'] = recv.grad.numpy()
        want.update({k: P[k].grad.numpy() for k, _ in layer.named_parameters() if P[k].grad is not None})
    return want, stats


def _layer_device(layer, dev, c, embedded):
    layer.zero_grad(set_to_none=True)
    send, recv = (_to(dev, c[k]).requires_grad_(True) for k in ('send', 'recv'))
    ei = _to(dev, c['ei'])
    if embedded:
        out = layer.forward_embedded_all_atom(recv, send, ei, _to(dev, c['emb']), _to(dev, c['sh']), seed=7)
    else:
        out = layer(send, ei, _to(dev, c['ea']), _to(dev, c['sh']), out_nodes=recv.shape[0])
    out.backward(_to(dev, c['g']))
    got = {'out': out.detach(), 'send': send.grad, 'recv': recv.grad}
    got.update({k: p.grad for k, p in layer.named_parameters()})
    return {k: _np(v) for k, v in got.items() if v is not None}


@pytest.mark.parametrize('l,bn', [(0, False), (0, True), (2, False), (2, True), (3, False), (3, True)])
@pytest.mark.parametrize('embedded', [False, True])
def test_all_atom_layer_in_training_against_fp64(dev, l, bn, embedded):
    """bipartite: 9 senders, 4 receivers; BatchNorm on the batch statistics, the buffers move"""
    c = _layer_case(l, 800 + l, 9, 4, 150)
    layer = _layer(l, dev, bn, 80 + l).train()
    before = {k: v.detach().cpu().double().numpy() for k, v in layer.named_buffers()}
    got = _layer_device(layer, dev, c, embedded)
    want, stats = _layer_fp64(layer, l, c, bn, True, embedded)      # (reads the parameters alone: the buffers have moved)
    assert set(got) == set(want) and len(want) == 2 + int(embedded) + 4 + (2 if bn else 0), (sorted(got), sorted(want))
    errs = {k: rel_err(got[k], want[k]) for k in want}
    if bn:
        after = {k: _np(v) for k, v in layer.named_buffers()}
        for k, stat in zip(('batch_norm.running_mean', 'batch_norm.running_var'), stats):
            errs[k] = rel_err(after[k], 0.9 * before[k] + 0.1 * stat.numpy())
            assert not np.array_equal(after[k], before[k])
    _assert_blocks(f'layer_training.l{l}.bn{int(bn)}.embedded{int(embedded)}', errs)


def test_all_atom_layer_without_edges_is_batch_norm_of_zeros(dev):
    """a ligand outside the receptor: the conv has no edges and BatchNorm still runs (the score model's layer returns the zeros); the buffers move"""
    l = 2
    c = _layer_case(l, 870, 9, 4, 0)
    for embedded in (False, True):
        layer = _layer(l, dev, True, 87).train()
        before = {k: v.detach().clone() for k, v in layer.named_buffers()}
        send, recv, ei = _to(dev, c['send']), _to(dev, c['recv']), _to(dev, c['ei'])
        if embedded:
            out = layer.forward_embedded_all_atom(recv, send, ei, _to(dev, c['emb']), _to(dev, c['sh']))
        else:
            out = layer(send, ei, _to(dev, c['ea']), _to(dev, c['sh']), out_nodes=4)
        want, stats = _layer_fp64(layer, l, c, True, True, embedded)
        assert out.shape == want['out'].shape and np.abs(want['out'][:, :24]).max() > 0      # the bias of the scalars
        assert rel_err(_np(out), want['out']) < BAR
        after = dict(layer.named_buffers())
        assert torch.equal(after['batch_norm.running_mean'], 0.9 * before['batch_norm.running_mean'])      # the batch mean and norm are zero
        assert torch.equal(after['batch_norm.running_var'], 0.9 * before['batch_norm.running_var'])
        assert not torch.equal(after['batch_norm.running_var'], before['batch_norm.running_var'])
    quiet = _layer(l, dev, False, 88).train()
    assert not _np(quiet(send, ei, _to(dev, c['ea']), _to(dev, c['sh']), out_nodes=4)).any()


@pytest.mark.parametrize('l,bn', [(0, True), (2, False), (3, True)])
def test_all_atom_layer_in_evaluation(dev, l, bn):
    """.eval() runs the training ops: BatchNorm on the running buffers, no dropout (the layer is built with rate 0.5), the same bits on two calls, the
    buffers untouched; against fp64"""
    c = _layer_case(l, 850 + l, 9, 4, 150)
    layer = _layer(l, dev, bn, 85 + l, dropout=0.5).eval()
    buffers = {k: v.detach().clone() for k, v in layer.named_buffers()}
    for embedded in (False, True):
        got, again = _layer_device(layer, dev, c, embedded), _layer_device(layer, dev, c, embedded)
        assert all(np.array_equal(got[k], again[k]) for k in got)      # bit-identical, every gradient too
        want, _ = _layer_fp64(layer, l, c, bn, False, embedded)
        assert set(got) == set(want)
        _assert_blocks(f'layer_eval.l{l}.bn{int(bn)}.embedded{int(embedded)}', {k: rel_err(got[k], want[k]) for k in want})
    assert all(torch.equal(v, buffers[k]) for k, v in layer.named_buffers())


def test_the_holder_refuses_per_edge_weights(dev):
    from disco_diffdock_amd.tensor_layers import FasterTensorProduct, FullyConnectedTensorProduct, fused_radial_tp
    tp = FullyConnectedTensorProduct(IRREPS[3], '1x0e + 1x1o + 1x2e', IRREPS[3])
    assert (tp.layer, tp.weight_numel, tp.out_size) == (AA + 3, 1944, 84)
    with pytest.raises(RuntimeError, match='fused_radial_tp'):
        tp(torch.zeros(1, 84, device=dev), torch.zeros(1, 9, device=dev), torch.zeros(1, 1944, device=dev))
    # the reference's 4-module Sequential through fused_radial_tp, against the closed form
    s = ccr.shape(3)
    fc = torch.nn.Sequential(torch.nn.Linear(72, 72), torch.nn.ReLU(), torch.nn.Dropout(0.0), torch.nn.Linear(72, 1944)).to(dev)
    rng = np.random.default_rng(5)
    x, sh, ea = (rng.standard_normal(shape).astype(np.float32) for shape in ((40, 84), (40, 9), (40, 72)))
    out = fused_radial_tp(tp, fc, _to(dev, x), _to(dev, sh), _to(dev, ea))
    with torch.no_grad():
        w = fc(_to(dev, ea)).double().cpu().numpy()
    assert rel_err(_np(out), ccr.tp(3, x, sh, w)) < BAR
    assert FasterTensorProduct(IRREPS[3], '1x0e+1x1o', IRREPS[3]).layer == 3      # the first family's holder has not moved
