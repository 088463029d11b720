"""CPU tests of tests/adversarial_training.py: the helper behind tests/test_gpu_training_adversarial.py is itself held to account here, without a GPU.

* its forms in fp64 are the project's closed forms (tp_backward_ref, radial_tp_ref, radial_conv_ref) and, for the nv = 4 family, autograd of the oracle
* every generator's claims hold (the generators assert them; the claims about outputs are asserted here on the fp64 reference)
* S >= |reference| everywhere, and S == |reference| on all-nonnegative operands of layer 0 (no cross rows: there S is tight)
* an fp32 numpy evaluation of every op in two summation orders stays under the bar on every class, table and graph, for all eight shapes; the largest
  err / (u S) per op is printed (and kept in the helper's docstring)
* teeth: four mutants of that evaluation exceed the bar on the class built for them; the first one passes the suite's older per-block bar
* seg_ref is within deg u S of the fp64 sum"""
import numpy as np
import pytest

import adversarial_training as at
import latent_encoder_ref as ler
import radial_conv_ref as rcr
import radial_tp_ref as rtr
import tp_backward_ref as tpr
from helpers import rel_err

RTP_NAMES = ('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2')
FIGURES = {}      # op.output -> largest err / (u S) of the fp32 evaluations


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return a.size == 0 or np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


def _variants(cls):
    return ('x', 'g') if cls == 'zero_blocks' else ('x',)


def _under_bar(tag, op, l, o, offsets=None, gr=None):
    M = at.measures(op, l, o, offsets, gr)
    for m in at.FP32_ORDERS:
        ev = at.evaluate(m, op, l, o, offsets, gr)
        for k, (ref, S, n) in M.items():
            assert ev[k].dtype == np.float32
            ratio, where = at.worst(ev[k], ref, n, S)
            assert ratio <= 1, (tag, k, where, ratio)
            if S.size and (S > 0).any():
                fig = float((np.abs(ev[k] - ref)[S > 0] / (at.U * S[S > 0])).max())
                FIGURES[f'{op}.{k}'] = max(FIGURES.get(f'{op}.{k}', 0.0), fig)
    return M


# ---- 1. the forms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', at.SHAPES)
def test_fp64_forms_are_the_closed_forms(l):
    s, offs, gr = at.shape(l), at.CLASS_TABLE, at.graph('reversed')
    o = at.operands('channel_spread', l, offs, 3)
    w = at.weights(at.FP64, s, o['h'], offs, o['w2'], o['b2'])
    oc = at.operands('column_spread', l, gr['offsets'], 3, n_in=gr['n_in'], n_out=gr['n_out'])
    tp = at.evaluate(at.FP64, 'tp', l, dict(o, w=w))
    rtp = at.evaluate(at.FP64, 'rtp', l, o, offs)
    rc = at.evaluate(at.FP64, 'rconv', l, oc, gr['offsets'], gr)
    if l < at.NV4:
        gx, gsh, gw = tpr.backward(l, o['x'], o['sh'], w, o['g'])
        assert _close(tp['out'], tpr.forward(l, o['x'], o['sh'], w)) and _close(tp['grad_x'], gx) and _close(tp['grad_sh'], gsh) and _close(tp['grad_w'], gw)
        args = (l, o['x'], o['sh'], o['h'], offs, o['w2'], o['b2'])
        assert _close(rtp['out'], rtr.forward(*args))
        assert all(_close(rtp[k], v) for k, v in zip(RTP_NAMES[1:], rtr.backward(*args, o['g'])))
        args = (l, oc['x'], gr['src'], gr['dst'], gr['n_out'], oc['sh'], oc['h'], gr['offsets'], oc['w2'], oc['b2'])
        assert _close(rc['out'], rcr.forward(*args))
        assert all(_close(rc[k], v) for k, v in zip(RTP_NAMES[1:], rcr.backward(*args, oc['g'])))
    else:
        k = l - at.NV4
        out, g = ler.tp(k, 4, o['x'], o['sh'], w, o['g'])
        assert _close(tp['out'], out) and _close(tp['grad_x'], g['x']) and _close(tp['grad_sh'], g['sh']) and _close(tp['grad_w'], g['w'])
        out, g = ler.rtp(k, 4, o['x'], o['sh'], o['h'], offs, o['w2'], o['b2'], o['g'])
        assert _close(rtp['out'], out) and all(_close(rtp[a], g[b]) for a, b in zip(RTP_NAMES[1:], ('x', 'sh', 'h', 'w2', 'b2')))
        out, g = ler.rconv(k, 4, oc['x'], gr['src'], gr['dst'], gr['n_out'], oc['sh'], oc['h'], gr['offsets'], oc['w2'], oc['b2'], oc['g'])
        assert _close(rc['out'], out) and all(_close(rc[a], g[b]) for a, b in zip(RTP_NAMES[1:], ('x', 'sh', 'h', 'w2', 'b2')))


# ---- 2. S ---------------------------------------------------------------------------------------------------------------------------------------
def test_S_is_tight_on_nonnegative_operands_of_layer_0():
    gr = at.graph('degrees')
    for l in (0, at.NV4):
        o = at.operands('column_spread', l, at.CLASS_TABLE, 5)
        o = {k: (np.abs(v) if k != 'claims' else v) for k, v in o.items()}
        w = at.weights(at.FP64, at.shape(l), o['h'], at.CLASS_TABLE, o['w2'], o['b2']).astype(np.float32)
        oc = at.operands('relu_sparse', l, gr['offsets'], 5, n_in=gr['n_in'], n_out=gr['n_out'])
        oc = {k: (np.abs(v) if k != 'claims' else v) for k, v in oc.items()}
        for op, ops, offs, g in (('tp', dict(o, w=w), None, None), ('rtp', o, at.CLASS_TABLE, None), ('rconv', oc, gr['offsets'], gr)):
            for k, (ref, S, n) in at.measures(op, l, ops, offs, g).items():
                assert (ref >= 0).all() and _close(S, ref), (l, op, k)


# ---- 3. the classes: claims, S >= |ref|, the fp32 evaluations under the bar ---------------------------------------------------------------------
@pytest.mark.parametrize('l', at.SHAPES)
@pytest.mark.parametrize('cls', at.CLASSES)
def test_classes(cls, l):
    offs, s = at.CLASS_TABLE, at.shape(l)
    for variant in _variants(cls):
        cases = [('rtp', at.operands(cls, l, offs, 11, variant=variant), offs)]
        if cls in at.TP_CLASSES:
            cases.append(('tp', at.operands(cls, l, [0, 130], 11, variant=variant, tp=True), None))
        for op, o, offsets in cases:
            M = _under_bar(f'{op}.{cls}.{variant}.l{l}', op, l, o, offsets)
            for k, (ref, S, n) in M.items():
                assert np.all(S >= np.abs(ref) * (1 - 1e-12)), (op, k)
            cl = o['claims']
            if cls == 'zero_blocks':
                for k in (('grad_w',) if op == 'tp' else ('grad_w2', 'grad_b2')):
                    assert not M[k][0][:, cl['zero_slots']].any() and not M[k][1][:, cl['zero_slots']].any()      # exact zeros, and a bar of zero
                    assert M[k][0].any() or (variant == 'x' and s['din'] == s['A'])      # (layer 0 has one input irrep: all of x is zero then)
            if cls == 'relu_sparse':
                zg = cl['zero_group']
                assert zg is not None and not M['grad_w2'][0][zg].any() and not M['grad_w2'][1][zg].any() and M['grad_b2'][0][zg].any()
            if cls == 'cancelling':
                ref, S, _ = M['out']
                assert np.all(np.abs(ref[:, cl['out_column']]) <= 2.0 ** -18 * S[:, cl['out_column']])


@pytest.mark.parametrize('l', at.SHAPES)
@pytest.mark.parametrize('table', range(len(at.GROUP_TABLES)))
def test_group_tables(table, l):
    offs = at.GROUP_TABLES[table]
    M = _under_bar(f'rtp.table{table}.l{l}', 'rtp', l, at.operands('column_spread', l, offs, 20 + table), offs)
    sizes = np.diff(offs)
    for g in np.nonzero(sizes == 0)[0]:
        assert not M['grad_w2'][1][g].any() and not M['grad_b2'][1][g].any()      # an empty group: S = 0, so exact zeros are due
    assert {64, 128, 1, 127, 512, 0, 513, 511, 97, 96} <= set(np.concatenate([np.diff(t) for t in at.GROUP_TABLES]).tolist())


@pytest.mark.parametrize('l', at.SHAPES)
@pytest.mark.parametrize('cls', ('column_spread', 'relu_sparse'))
@pytest.mark.parametrize('name', at.GRAPHS)
def test_graphs(name, cls, l):
    gr = at.graph(name)
    o = at.operands(cls, l, gr['offsets'], 30, n_in=gr['n_in'], n_out=gr['n_out'])
    M = _under_bar(f'rconv.{name}.{cls}.l{l}', 'rconv', l, o, gr['offsets'], gr)
    for k, (ref, S, n) in M.items():
        assert np.all(S >= np.abs(ref) * (1 - 1e-12)), k
    ds, dd = np.bincount(gr['src'], minlength=gr['n_out']), np.bincount(gr['dst'], minlength=gr['n_in'])
    assert not M['out'][1][ds == 0].any() and not M['grad_x'][1][dd == 0].any()      # a node without edges: S = 0


# ---- 4. teeth -------------------------------------------------------------------------------------------------------------------------------------
def _ratio(got, M, k):
    return at.worst(got, *[M[k][i] for i in (0, 2, 1)])[0]


@pytest.mark.parametrize('l', (0, 3))
def test_mutants_exceed_the_bar(l):
    s, fp32 = at.shape(l), at.FP32_ORDERS[0]
    offs = [0, 60, 60, 130, 200]      # 200 edges
    # a dropped slot in the smallest column
    o = at.operands('column_spread', l, offs, 41)
    M = at.measures('rtp', l, o, offs)
    p, c = o['claims']['small_slot'], o['claims']['small_column']
    w2, b2 = o['w2'].copy(), o['b2'].copy()
    w2[:, p], b2[:, p] = 0, 0
    out = at.rtp_forward(fp32, s, o['x'], o['sh'], o['h'], offs, w2, b2)
    good = at.rtp_forward(fp32, s, o['x'], o['sh'], o['h'], offs, o['w2'], o['b2'])
    r_slot, where = at.worst(out, *[M['out'][i] for i in (0, 2, 1)])
    old = rel_err(out[:, :s['O'][0]], M['out'][0][:, :s['O'][0]])
    assert r_slot > 1 and where[1] == c and _ratio(good, M, 'out') <= 1
    assert old < 1e-5      # the block bar of the older tests lets it through: the gap
    # h rounded to fp16
    o = at.operands('channel_spread', l, offs, 42)
    M = at.measures('rtp', l, o, offs)
    with np.errstate(under='ignore'):
        h16 = o['h'].astype(np.float16).astype(np.float32)
    r_h16 = _ratio(at.rtp_forward(fp32, s, o['x'], o['sh'], h16, offs, o['w2'], o['b2']), M, 'out')
    assert r_h16 > 1
    # one edge (a group's last) left out of the group's grad_w2
    o = at.operands('edge_spread', l, offs, 43)
    M = at.measures('rtp', l, o, offs)
    h = o['h'].copy()
    e = int(o['claims']['last_edges'][-1])
    assert h[e].any()
    h[e] = 0
    r_edge = _ratio(at.rtp_backward(fp32, s, o['x'], o['sh'], h, offs, o['w2'], o['b2'], o['g'])[3], M, 'grad_w2')
    assert r_edge > 1
    # a node's last row left out of its sum
    gr = at.graph('degrees')
    o = at.operands('column_spread', l, gr['offsets'], 44, n_in=gr['n_in'], n_out=gr['n_out'])
    M = at.measures('rconv', l, o, gr['offsets'], gr)
    rows = at.rtp_forward(fp32, s, o['x'][gr['dst']], o['sh'], o['h'], gr['offsets'], o['w2'], o['b2'])
    assert _ratio(at.seg_ref(rows, gr['src'], gr['n_out'], mean=True), M, 'out') <= 1
    rows[np.nonzero(gr['src'] == 0)[0][-1]] = 0      # the hub's last row
    r_row, where = at.worst(at.seg_ref(rows, gr['src'], gr['n_out'], mean=True), *[M['out'][i] for i in (0, 2, 1)])
    assert r_row > 1 and where[0] == 0
    print(f'mutants l{l}: dropped slot {r_slot:.2e} x bar (rel_err of its block {old:.2e}), h in fp16 {r_h16:.2e}, an edge left out {r_edge:.2e}, '
          f'a last row left out {r_row:.2e}')


# ---- 5. the order-exact segmented sum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', at.GRAPHS)
def test_seg_ref_against_fp64(name):
    gr = at.graph(name)
    rng = np.random.default_rng(7)
    E = len(gr['src'])
    rows = (rng.standard_normal((E, 5)) * np.exp2(-rng.integers(0, 21, (E, 1)))).astype(np.float32)
    rows[:, 4] = -0.0
    for idx, n in ((gr['src'], gr['n_out']), (gr['dst'], gr['n_in'])):
        want, S = np.zeros((n, 5)), np.zeros((n, 5))
        np.add.at(want, idx, rows.astype(np.float64))
        np.add.at(S, idx, np.abs(rows.astype(np.float64)))
        deg = np.bincount(idx, minlength=n)[:, None]
        got = at.seg_ref(rows, idx, n)
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= deg * at.U * S)
        assert np.array_equal(np.signbit(got[:, 4]), deg[:, 0] > 0)      # -0 stays -0; a node without rows is +0
        mean = at.seg_ref(rows, idx, n, mean=True)
        assert np.array_equal(mean, (got / np.maximum(deg, 1).astype(np.float32)).astype(np.float32))
    g = rng.standard_normal((gr['n_out'], 3)).astype(np.float32)
    assert np.array_equal(at.node_scale(g, gr['src'], gr['n_out']), g / np.maximum(np.bincount(gr['src'], minlength=gr['n_out']), 1).astype(np.float32)[:, None])


def test_zz_print_the_figures():
    """(last in the file: the figures the other tests gathered, as the helper's docstring keeps them)"""
    for k in sorted(FIGURES):
        print(f'{k}: {FIGURES[k]:.1f} u S')
