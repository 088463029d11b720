"""Host tests of the all-atom (confidence) family: the closed form the kernels implement (tests/confidence_conv_ref.py, read from
``runtime.tp_layer_shape_aa``) against fp64 ``oracle.e3nn_lite.FullyConnectedTensorProduct``, ``sh_second_order`` against e3nn's spherical harmonics, the
AUC against pair counting, the labels against confidence/dataset.py:162-166.  No GPU."""
import math

import numpy as np
import pytest
import torch

import confidence_conv_ref as ccr
from oracle import e3nn_lite as o3

IRREPS = ['24x0e', '24x0e+6x1o', '24x0e+6x1o+6x1e', '24x0e+6x1o+6x1e+24x0o']
SH = '1x0e+1x1o+1x2e'
W = (720, 972, 1224, 1944)


def _oracle(l, x, sh, w, g):
    tp = o3.FullyConnectedTensorProduct(IRREPS[l], SH, IRREPS[min(l + 1, 3)])
    X, S, Wt = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (x, sh, w))
    out = tp(X, S, Wt)
    out.backward(torch.from_numpy(np.asarray(g, np.float64)))
    return tp, out.detach().numpy(), dict(x=X.grad.numpy(), sh=S.grad.numpy(), w=Wt.grad.numpy())


def _operands(l, seed, E=9):
    s = ccr.shape(l)
    rng = np.random.default_rng(seed)
    return s, rng.standard_normal((E, s['din'])), rng.standard_normal((E, 9)), rng.standard_normal((E, s['W'])), rng.standard_normal((E, s['dout']))


@pytest.mark.parametrize('l', range(4))
def test_the_table_is_e3nns(l):
    s = ccr.shape(l)
    tp = o3.FullyConnectedTensorProduct(IRREPS[l], SH, IRREPS[min(l + 1, 3)])
    assert s['W'] == tp.weight_numel == W[l] and (s['din'], s['dout']) == ((24, 42, 60, 84)[l], (42, 60, 84, 84)[l])
    assert [(p['offset'], p['mul_in'], p['mul_out']) for p in s['paths']] == [(off, shape[0], shape[2]) for _, _, _, off, shape in tp.instructions]
    for p, (i1, i2, io, _, _), coeff in zip(s['paths'], tp.instructions, tp.coeffs):      # sqrt(dim_out / R_k), R_k the fan-in of the output
        assert (p['ir_in'], p['ir_sh'], p['ir_out']) == tuple(str(irr[i].ir) for irr, i in ((tp.irreps_in1, i1), (tp.irreps_in2, i2), (tp.irreps_out, io)))
        amp = {'ss': 1, 'sv': 3 ** -0.5, 'vs': 3 ** -0.5, 'vd': 3 ** -0.5, 'vx': 6 ** -0.5, 'v2': 10 ** -0.5}[p['kind']]
        assert abs(p['scale'] - coeff * amp) < 1e-15 and s['R'][p['block']] == round((3 if p['block'] in (1, 2) else 1) / coeff ** 2)
    if l == 3:
        assert [p['offset'] for p in s['paths']] == [0, 576, 720, 756, 900, 936, 972, 1008, 1044, 1188, 1224, 1800]
    # a block's rows, in the order the kernels walk them, tile the block
    for k in range(4):
        rows = sorted((p['row0'], p['mul_in']) for p in s['paths'] if p['block'] == k)
        assert sum(m for _, m in rows) == s['R'][k] and all(r0 == sum(m for _, m in rows[:i]) for i, (r0, _) in enumerate(rows))


@pytest.mark.parametrize('l', range(4))
def test_closed_form_equals_e3nn_in_fp64(l):
    s, x, sh, w, g = _operands(l, 10 + l)
    _, want_out, want = _oracle(l, x, sh, w, g)
    out, got = ccr.tp(l, x, sh, w, g)
    assert np.abs(out - want_out).max() < 1e-12
    for k in ('x', 'sh', 'w'):
        assert np.abs(got[k] - want[k]).max() < 1e-12, k


@pytest.mark.parametrize('l', range(4))
def test_second_order_columns_alone(l):
    """sh[:, :4] = 0: only 1o (x) 2e -> 1o and 1e (x) 2e -> 1e act"""
    s, x, sh, w, g = _operands(l, 20 + l)
    sh[:, :4] = 0
    _, want_out, want = _oracle(l, x, sh, w, g)
    out, got = ccr.tp(l, x, sh, w, g)
    assert np.abs(out - want_out).max() < 1e-12 and all(np.abs(got[k] - want[k]).max() < 1e-12 for k in ('x', 'sh', 'w'))
    assert (np.abs(out).max() > 0) == (l > 0)
    live = [n for n, sl in ccr.weight_slices(s).items() if np.abs(got['w'][:, sl]).max() > 0]
    assert live == [n for n in ccr.weight_slices(s) if '.2e.' in n]


@pytest.mark.parametrize('l', range(4))
def test_a_single_weight_pins_every_instruction_offset(l):
    s, x, sh, _, g = _operands(l, 30 + l, E=3)
    for p in s['paths']:
        for at in (p['offset'], p['offset'] + p['mul_in'] * p['mul_out'] - 1):
            w = np.zeros((3, s['W']))
            w[:, at] = 1.0
            _, want_out, want = _oracle(l, x, sh, w, g)
            out, got = ccr.tp(l, x, sh, w, g)
            assert np.abs(want_out).max() > 0 and np.abs(out - want_out).max() < 1e-12
            assert all(np.abs(got[k] - want[k]).max() < 1e-12 for k in ('x', 'sh', 'w'))


def test_radial_form_and_conv_are_consistent():
    """rtp / rconv of the restatement against autograd through the closed form's layer (one group, no BatchNorm)"""
    l, E, n_in, n_out = 2, 40, 7, 5
    s = ccr.shape(l)
    rng = np.random.default_rng(3)
    x, sh, ea, g = rng.standard_normal((n_in, s['din'])), rng.standard_normal((E, 9)), rng.standard_normal((E, 72)), rng.standard_normal((n_out, s['dout']))
    ei = np.stack([rng.integers(0, n_out, E), rng.integers(0, n_in, E)])
    P = {'fc.0.weight': rng.standard_normal((72, 72)) / 8, 'fc.0.bias': rng.standard_normal(72), 'fc.3.weight': rng.standard_normal((s['W'], 72)) / 8,
         'fc.3.bias': rng.standard_normal(s['W'])}
    Pt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in P.items()}
    X = torch.from_numpy(x).requires_grad_(True)
    out, _ = ccr.layer_fp64(Pt, l, False, True, X, torch.zeros(n_out, 24, dtype=torch.float64), torch.from_numpy(ei), torch.from_numpy(sh), edge_attr=torch.from_numpy(ea))
    out.backward(torch.from_numpy(g))
    h = np.maximum(ea @ P['fc.0.weight'].T + P['fc.0.bias'], 0)
    got_out, got = ccr.rconv(l, x, ei[0], ei[1], n_out, sh, h, [0, E], P['fc.3.weight'][None], P['fc.3.bias'][None], g)
    assert np.abs(got_out - out.detach().numpy()).max() < 1e-12 and np.abs(got['x'] - X.grad.numpy()).max() < 1e-12
    assert np.abs(got['w2'][0] - Pt['fc.3.weight'].grad.numpy()).max() < 1e-11 and np.abs(got['b2'][0] - Pt['fc.3.bias'].grad.numpy()).max() < 1e-11


def test_sh_second_order_equals_e3nn():
    from disco_diffdock_amd.tensor_layers import sh_second_order
    rng = np.random.default_rng(4)
    v = torch.from_numpy(rng.standard_normal((200, 3)) * 10 ** rng.uniform(-3, 2, (200, 1)))
    v[7] = 0      # a zero-length edge: a C-alpha atom and its own residue
    want = o3.spherical_harmonics(SH, v, normalize=True, normalization='component')
    sh4 = want[:, :4].float()      # what fused_edge_embedding hands over: [1 | sqrt3 u], zeros for a zero vector
    got = sh_second_order(sh4)
    assert got.shape == (200, 9) and got.dtype == torch.float32 and not got.requires_grad
    assert torch.equal(got[:, :4], sh4) and not got[7, 1:].any() and got[7, 0] == 1
    # Y2 is a quadratic of the fp32 unit vector: its rounding (6e-8 relative per component) enters twice, times the largest coefficient sqrt(15)
    assert (got.double() - want).abs().max() < 8 * math.sqrt(15.0) * 2 ** -24


def test_auc_equals_pair_counting():
    from disco_diffdock_amd.confidence_training import roc_auc
    rng = np.random.default_rng(5)
    for n, ties in ((2, False), (17, False), (64, True), (65, True)):
        y = rng.integers(0, 2, n)
        y[0], y[1] = 0, 1
        s = rng.integers(0, 6, n).astype(np.float32) if ties else rng.standard_normal(n).astype(np.float32)
        got = float(roc_auc(torch.from_numpy(y).float(), torch.from_numpy(s)))
        assert abs(got - ccr.auc_pairs(y, s)) < 1e-12, (n, ties)
    for y in (np.zeros(9), np.ones(9)):      # one class present: 0, as the reference's except
        assert float(roc_auc(torch.from_numpy(y).float(), torch.randn(9))) == 0.0 == ccr.auc_pairs(y, np.zeros(9))
    assert float(roc_auc(torch.tensor([0., 1.]), torch.tensor([1., 1.]))) == 0.5      # all tied
    # a list of cutoffs: sklearn's macro average over the columns, 0 when a column holds one class
    Y, S = rng.integers(0, 2, (30, 2)), rng.standard_normal((30, 2)).astype(np.float32)
    Y[0], Y[1] = (0, 1), (1, 0)
    want = np.mean([ccr.auc_pairs(Y[:, c], S[:, c]) for c in range(2)])
    assert abs(float(roc_auc(torch.from_numpy(Y).float(), torch.from_numpy(S))) - want) < 1e-12
    Y[:, 1] = 1
    assert float(roc_auc(torch.from_numpy(Y).float(), torch.from_numpy(S))) == 0.0


def test_labels_are_the_datasets():
    """confidence/dataset.py:162-166"""
    from disco_diffdock_amd.confidence_training import confidence_labels, pose_draw
    for rmsd in (0.0, 1.999, 2.0, 3.7, 5.0, 9.0):
        lab = confidence_labels(rmsd, 2.0)
        assert set(lab) == {'y', 'rmsd'} and lab['y'].shape == (1,) and lab['y'].item() == float(rmsd < 2.0) and abs(lab['rmsd'].item() - rmsd) < 1e-6
        cut = [2.0, 5.0]
        lab = confidence_labels(rmsd, cut)
        want = np.logical_and(rmsd < np.array(cut + [math.inf]), rmsd >= np.array([0] + cut)).astype(np.float32)
        assert lab['y_binned'].shape == (1, 3) and np.array_equal(lab['y_binned'][0].numpy(), want) and want.sum() == 1
        assert lab['y'].item() == float(rmsd < cut[0])
    # the draw: a pure function of (seed, complex, epoch), spread over the samples
    draws = [pose_draw('1abc', 40, 7, e) for e in range(200)]
    assert draws == [pose_draw('1abc', 40, 7, e) for e in range(200)] and len(set(draws)) > 25 and min(draws) >= 0 and max(draws) < 40
    assert draws != [pose_draw('2xyz', 40, 7, e) for e in range(200)] and draws != [pose_draw('1abc', 40, 8, e) for e in range(200)]
