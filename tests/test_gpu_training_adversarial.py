"""GPU tests of the training ops on adversarial operands, judged PER ELEMENT: the tensor product (ddk_tp_forward / ddk_tp_backward), the radial tensor product
(ddk_rtp_*), the radial conv (ddk_rconv_*) and the segmented sum (ddk_seg_sum), both shape families, through Context.

Reference, operands and bar: tests/adversarial_training.py (its docstring derives the bar; tests/test_adversarial_training_host.py shows on the CPU that
fp32 evaluations in two orders stay under it and that four mutants do not).  Every element of every output is held to
    |device - fp64| <= n u (1 + 2^-10) S,     S = the element's own sum of |terms|,     n = its count of fp32 roundings,
and an element whose S is 0 to an exact zero: no block maximum that a large column could hide a small one behind.  The node side of the conv is held to
the documented order bit for bit: a node's rows added in ascending edge id, then one true division (adversarial_training.seg_ref, an emulator written from
the kernels' headers, not from their output).  The largest err / bar per op and class goes to the suite's parity-drift record."""
import numpy as np
import pytest
import torch

import adversarial_training as at
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
RTP_NAMES = ('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2')
WORST = {}      # (op, class) -> the largest err / bar so far


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
    assert TP_NV4 == at.NV4
    return _shape_context(0)      # a shape-only context: no weights loaded


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _device(ctx, dev, op, l, o, offsets=None, graph=None):
    """{output name: numpy} of the op on the device"""
    s = at.shape(l)
    t = {k: _to(dev, v) for k, v in o.items() if k != 'claims'}
    if op == 'tp':
        out = ctx.tp_forward(l, t['x'], t['sh'], t['w'], s['dout'])
        grads = ctx.tp_backward(l, t['x'], t['sh'], t['w'], t['g'])
        return dict(zip(('out', 'grad_x', 'grad_sh', 'grad_w'), map(_np, (out,) + tuple(grads))))
    if op == 'rtp':
        out = ctx.rtp_forward(l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], s['dout'])
        grads = ctx.rtp_backward(l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'])
    else:
        out = ctx.rconv_forward(l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'])
        grads = ctx.rconv_backward(l, graph, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'])
    return dict(zip(RTP_NAMES, map(_np, (out,) + tuple(grads))))


def _judge(op, cls, tag, s, got, M, offsets=None):
    """every element of every output against its own bar; the figures are printed and recorded before they are asserted"""
    ratios = {}
    for k, (ref, S, n) in M.items():
        assert got[k].shape == ref.shape, (tag, k, got[k].shape, ref.shape)
        ratios[k] = at.worst(got[k], ref, n, S)
    print(tag, {k: f'{v[0]:.3f}' for k, v in ratios.items()})
    k = max(ratios, key=lambda name: ratios[name][0])
    if ratios[k][0] >= WORST.get((op, cls), (-1.0,))[0]:
        WORST[(op, cls)] = (ratios[k][0], tag, k)
        _record_drift(f'training_adversarial.{op}.{cls}', ratios[k][0], worst_case=tag, worst_output=k, bar=1.0, unit='err / (n u S)')
    for k, (ratio, where) in ratios.items():
        assert ratio <= 1, (tag, at.locate(k, where, None if op == 'rconv' and k in ('out', 'grad_x') else offsets, s), ratio,
                            float(got[k][where]), float(M[k][0][where]), float(M[k][1][where]))


def _exact_zeros(cls, op, o, got, ref):
    """the outputs the class lists as exactly zero"""
    cl = o['claims']
    if cls == 'zero_blocks':
        for k in (('grad_w',) if op == 'tp' else ('grad_w2', 'grad_b2')):
            assert (got[k][:, cl['zero_slots']] == 0).all(), (k, cl)
    if cls == 'relu_sparse' and cl['zero_group'] is not None:
        zg = cl['zero_group']
        assert (got['grad_w2'][zg] == 0).all() and got['grad_b2'][zg].any() and ref['grad_b2'][0][zg].any()


def _variants(cls):
    return ('x', 'g') if cls == 'zero_blocks' else ('x',)


# ---- 1. the per-element bar -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', at.SHAPES)
@pytest.mark.parametrize('cls', at.TP_CLASSES)
def test_tensor_product_per_element(ctx, dev, cls, l):
    for variant in _variants(cls):
        o = at.operands(cls, l, [0, 130], 11, variant=variant, tp=True)      # 130 edges
        got, M = _device(ctx, dev, 'tp', l, o), at.measures('tp', l, o)
        _judge('tp', cls, f'tp.{cls}.{variant}.l{l}', at.shape(l), got, M, [0, 130])
        _exact_zeros(cls, 'tp', o, got, M)


@pytest.mark.parametrize('l', at.SHAPES)
@pytest.mark.parametrize('cls', at.CLASSES)
def test_radial_tensor_product_per_element(ctx, dev, cls, l):
    offs = at.CLASS_TABLE
    for variant in _variants(cls):
        o = at.operands(cls, l, offs, 11, variant=variant)
        got, M = _device(ctx, dev, 'rtp', l, o, offs), at.measures('rtp', l, o, offs)
        _judge('rtp', cls, f'rtp.{cls}.{variant}.l{l}', at.shape(l), got, M, offs)
        _exact_zeros(cls, 'rtp', o, got, M)
        assert (got['grad_w2'][1] == 0).all() and (got['grad_b2'][1] == 0).all()      # the empty group


@pytest.mark.parametrize('l', (0, 3, at.NV4 + 1, at.NV4 + 3))
@pytest.mark.parametrize('table', range(len(at.GROUP_TABLES)))
def test_radial_tensor_product_group_tables(ctx, dev, table, l):
    offs = at.GROUP_TABLES[table]
    o = at.operands('column_spread', l, offs, 20 + table)
    got, M = _device(ctx, dev, 'rtp', l, o, offs), at.measures('rtp', l, o, offs)
    _judge('rtp', 'column_spread.tables', f'rtp.table{table}.l{l}', at.shape(l), got, M, offs)
    for g in np.nonzero(np.diff(offs) == 0)[0]:
        assert (got['grad_w2'][g] == 0).all() and (got['grad_b2'][g] == 0).all()


def _graph(ctx, dev, gr):
    return ctx.conv_graph(_to(dev, gr['src']), _to(dev, gr['dst']), gr['n_in'], gr['n_out'])


@pytest.mark.parametrize('l', (1, 3, at.NV4 + 2))
@pytest.mark.parametrize('cls', ('column_spread', 'relu_sparse'))
@pytest.mark.parametrize('name', at.GRAPHS)
def test_radial_conv_per_element(ctx, dev, name, cls, l):
    gr = at.graph(name)
    o = at.operands(cls, l, gr['offsets'], 30, n_in=gr['n_in'], n_out=gr['n_out'])
    got = _device(ctx, dev, 'rconv', l, o, gr['offsets'], _graph(ctx, dev, gr))
    M = at.measures('rconv', l, o, gr['offsets'], gr)
    _judge('rconv', cls, f'rconv.{name}.{cls}.l{l}', at.shape(l), got, M, gr['offsets'])
    _exact_zeros(cls, 'rconv', o, got, M)
    ds, dd = np.bincount(gr['src'], minlength=gr['n_out']), np.bincount(gr['dst'], minlength=gr['n_in'])
    assert (got['out'][ds == 0] == 0).all() and (got['grad_x'][dd == 0] == 0).all()      # nodes without edges


# ---- 2. the node side, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', at.GRAPHS)
def test_seg_sum_is_the_documented_sum_bit_for_bit(ctx, dev, name):
    gr = at.graph(name)
    graph = _graph(ctx, dev, gr)
    E = len(gr['src'])
    rng = np.random.default_rng(70 + at.GRAPHS.index(name))
    for D in (1, 5, 128):
        rows = (rng.standard_normal((E, D)) * np.exp2(-rng.integers(0, 21, (E, 1)))).astype(np.float32)
        rows[:, D - 1] = -0.0      # a column of -0: stays -0 where the node has rows
        rows[::3, D // 2] = -0.0
        for idx, n, order, ptr in ((gr['src'], gr['n_out'], graph.src_order, graph.src_ptr), (gr['dst'], gr['n_in'], graph.dst_order, graph.dst_ptr)):
            got = _np(ctx.seg_sum(_to(dev, rows), order, ptr))
            want = at.seg_ref(rows, idx, n)
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (name, D, np.argwhere(_bits(got) != _bits(want))[:5])


@pytest.mark.parametrize('l', (3, at.NV4 + 2))
@pytest.mark.parametrize('name', at.GRAPHS)
def test_radial_conv_node_side_bit_for_bit(ctx, dev, name, l):
    """the conv is the radial tensor product's rows (the device's own) under the documented node sums: the mean in ascending edge id with one fp32 division,
    the backward with g = grad_out / float32(count) formed once per node"""
    gr, s = at.graph(name), at.shape(l)
    src, dst, offs = gr['src'], gr['dst'], gr['offsets']
    o = at.operands('column_spread', l, offs, 31, n_in=gr['n_in'], n_out=gr['n_out'])
    graph = _graph(ctx, dev, gr)
    t = {k: _to(dev, v) for k, v in o.items() if k != 'claims'}
    x_rows = _to(dev, o['x'][dst])
    out = _np(ctx.rconv_forward(l, graph, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2']))
    rows = _np(ctx.rtp_forward(l, x_rows, t['sh'], t['h'], offs, t['w2'], t['b2'], s['dout']))
    want = at.seg_ref(rows, src, gr['n_out'], mean=True)
    diff = np.argwhere(_bits(out) != _bits(want))
    if len(diff):      # is it the division alone?
        sums = at.seg_ref(rows, src, gr['n_out'])
        n, c = diff[0]
        print(f'out[{n}, {c}]: device {out[n, c]!r}, emulator {want[n, c]!r}, the sum {sums[n, c]!r} over {np.bincount(src, minlength=gr["n_out"])[n]} rows')
    assert not len(diff), (name, l, diff[:5])
    grads = [_np(a) for a in ctx.rconv_backward(l, graph, t['x'], t['sh'], t['h'], offs, t['w2'], t['b2'], t['g'])]
    g_rows = at.node_scale(o['g'], src, gr['n_out'])[src]
    edge = [_np(a) for a in ctx.rtp_backward(l, x_rows, t['sh'], t['h'], offs, t['w2'], t['b2'], _to(dev, g_rows))]
    want_x = at.seg_ref(edge[0], dst, gr['n_in'])
    assert np.array_equal(_bits(grads[0]), _bits(want_x)), (name, l, np.argwhere(_bits(grads[0]) != _bits(want_x))[:5])
    for k, a, b in zip(RTP_NAMES[2:], grads[1:], edge[1:]):
        assert np.array_equal(_bits(a), _bits(b)), (name, l, k, np.argwhere(_bits(a) != _bits(b))[:5])
