"""ddk_node_cross_entropy_batch and its backward (csrc/k_node_ce.hip; tensor_layers.ragged_node_cross_entropy) against tests/node_cross_entropy_ref.py.

ONE launch holds five graphs, (n_lig, n_rec) =
    (1, 0)       a single node: loss 0 and gradient exactly 0
    (0, 5)       no ligand node; the target at the LAST position
    (3, 2)       not a multiple of four; the target in the ligand part; the student's maximum twice (positions 1 and 4): the lowest wins
    (7, 1018)    1025 positions, one past a full trip of 256 quads; the target in the receptor part, the teacher's maximum twice (600 and 900); student
                 logits spread over +-90 (an fp32 exponential without the maximum taken out overflows at 90)
    (30, 2129)   the largest timesplit receptor; the target at position 0
with D = 1 and D = 4 (a different teacher column per graph), in hard and in soft mode.  The loss and both gradient tables are measured ELEMENT-WISE
(helpers.elem_err) against the fp64 restatement and held to max(4 * err32, 1e-5), err32 the error of the host's fp32 restatement against fp64; the figures are
kept through _record_drift under node_ce.<case>.  pick and target are exact.  Bad tables are tested through the left-unwritten path only."""
import numpy as np
import pytest
import torch

import node_cross_entropy_ref as nref
from helpers import _bits, elem_err

pytestmark = pytest.mark.gpu
F32 = np.float32
FLOOR, K = 1e-5, 4.0
SHAPES = ((1, 0), (0, 5), (3, 2), (7, 1018), (30, 2129))
TARGET_AT = (0, 4, 1, 600, 0)      # position of the teacher's maximum in its graph's column: single node, last, ligand part, receptor part, first


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


def _record(key, value, **extra):
    from test_gpu_round3 import _record_drift
    _record_drift(f'node_ce.{key}', value, **extra)


_cases = {}


def _case(D):
    """per graph: the student's logits [n], the teacher's table [n, D], its column; and the upstream gradient [G].  Made once per D and never changed."""
    if D in _cases:
        return _cases[D]
    rng = np.random.default_rng(20 + D)
    graphs = []
    for g, ((n_l, n_r), at) in enumerate(zip(SHAPES, TARGET_AT)):
        n = n_l + n_r
        s = rng.normal(0, 3, n).astype(F32)
        t = rng.normal(0, 2, (n, D)).astype(F32)
        c = (g + 1) % D
        t[at, c] = t[:, c].max() + F32(1.5)
        if (n_l, n_r) == (3, 2):
            s[1] = s[4] = s.max() + F32(1.0)
        if (n_l, n_r) == (7, 1018):
            s = rng.uniform(-90, 90, n).astype(F32)
            s[17], s[800] = F32(90.0), F32(-90.0)
            t[900, c] = t[600, c]
        graphs.append(dict(s=s, t=t, c=c, n_l=n_l, n_r=n_r))
    _cases[D] = dict(graphs=graphs, grad=rng.normal(0, 1, len(SHAPES)).astype(F32))
    return _cases[D]


def _collate(case, order, scale=1.0):
    """the graphs of ``case`` in ``order`` as host tables: logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, grad"""
    gs = [case['graphs'][g] for g in order]
    D = gs[0]['t'].shape[1]
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, F32)
    logit_l, logit_r = cat([g['s'][:g['n_l']] for g in gs], (0,)), cat([g['s'][g['n_l']:] for g in gs], (0,))
    teacher_l, teacher_r = cat([g['t'][:g['n_l']] for g in gs], (0, D)) * F32(scale), cat([g['t'][g['n_l']:] for g in gs], (0, D)) * F32(scale)
    lig_ptr = np.concatenate([[0], np.cumsum([g['n_l'] for g in gs])]).astype(np.int64)
    rec_ptr = np.concatenate([[0], np.cumsum([g['n_r'] for g in gs])]).astype(np.int64)
    column = np.asarray([g['c'] for g in gs], np.int32)
    return logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, case['grad'][list(order)]


def _device(dev, host):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host]


def _run(dev, host, soft):
    """the op through autograd: (loss, pick, target, grad_logit_l, grad_logit_r) as host arrays"""
    from disco_diffdock_amd.tensor_layers import ragged_node_cross_entropy
    l, r, lp, rp, tl, tr, col, grad = _device(dev, host)
    l.requires_grad_(True)
    r.requires_grad_(True)
    loss, pick, target = ragged_node_cross_entropy(l, r, lp, rp, tl, tr, col, soft=soft)
    (loss * grad).sum().backward()
    return tuple(v.detach().cpu().numpy() for v in (loss, pick, target, l.grad, r.grad))


_refs = {}


def _reference(D, soft):
    """(host tables in the natural order, the fp64 restatement, the fp32 restatement): computed once, shared, never changed"""
    if (D, soft) not in _refs:
        host = _collate(_case(D), range(len(SHAPES)))
        _refs[D, soft] = (host, nref.node_cross_entropy(*host[:7], soft, grad=host[7], dtype=np.float64),
                          nref.node_cross_entropy(*host[:7], soft, grad=host[7], dtype=np.float32))
    return _refs[D, soft]


@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('D', [1, 4])
def test_node_cross_entropy_against_fp64(dev, ctx, D, soft):
    host, want, host32 = _reference(D, soft)
    loss, pick, target, g_l, g_r = _run(dev, host, soft)
    assert np.array_equal(pick, want[1]) and np.array_equal(target, want[2]), (pick, want[1], target, want[2])
    assert target.tolist() == list(TARGET_AT) and pick[2] == 1      # the lowest position of a two-way tie, student and teacher
    assert np.isfinite(loss).all() and np.isfinite(g_l).all() and np.isfinite(g_r).all()
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(host[1][host[3][3]:host[3][4]].max()))      # the +-90 graph: exp(90) in fp32 without the maximum taken out is inf
    mode = 'soft' if soft else 'hard'
    for name, got, ref, ref32 in (('loss', loss, want[0], host32[0]), ('grad_l', g_l, want[3], host32[3]), ('grad_r', g_r, want[4], host32[4])):
        err, err32 = elem_err(got, ref), elem_err(ref32, ref)
        bar = max(K * err32, FLOOR)
        print(f'node_ce.D{D}.{mode}.{name}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record(f'D{D}.{mode}.{name}', err, host_fp32=err32, bar=bar)
        assert err <= bar, (name, err, bar)
    # the single node: loss 0 and gradient exactly 0
    assert loss[0] == 0.0 and g_l[0] == 0.0, (loss[0], g_l[0])


def test_soft_with_a_sharp_teacher_agrees_with_hard(dev, ctx):
    """the teacher scaled by 100: its maximum leads by at least 1.5 * 100 except for the tie, whose two positions then share the label; on the graphs
    without a teacher tie softmax is the one-hot to within exp(-150), so the fp64 losses agree to 1e-60 and their fp32 roundings to an ulp"""
    case = _case(4)
    host = _collate(case, range(len(SHAPES)), scale=100.0)
    hard = _run(dev, host, False)
    soft = _run(dev, host, True)
    keep = [g for g in range(len(SHAPES)) if SHAPES[g] != (7, 1018)]      # (the tie graph: soft mode spreads the label over both positions)
    assert np.array_equal(hard[1], soft[1]) and np.array_equal(hard[2], soft[2])
    err = elem_err(soft[0][keep], hard[0][keep])
    print(f'node_ce.sharp_teacher.loss: soft against hard {err:.2e}')
    _record('sharp_teacher.loss', err, bar=2.0 ** -22)
    assert err <= 2.0 ** -22, err
    lp, rp = host[2], host[3]
    for g in keep:
        for got, ref, ptr in ((soft[3], hard[3], lp), (soft[4], hard[4], rp)):
            a, b = got[ptr[g]:ptr[g + 1]], ref[ptr[g]:ptr[g + 1]]
            assert elem_err(a, b) <= 2.0 ** -22, (g, elem_err(a, b))


@pytest.mark.parametrize('soft', [False, True])
def test_same_bits_twice_and_in_another_batch_order(dev, ctx, soft):
    case = _case(4)
    natural = list(range(len(SHAPES)))
    first = _run(dev, _collate(case, natural), soft)
    again = _run(dev, _collate(case, natural), soft)
    for a, b in zip(first, again):
        assert np.array_equal(np.asarray(a).view(np.int32 if a.dtype == F32 else a.dtype), np.asarray(b).view(np.int32 if b.dtype == F32 else b.dtype))
    order = [4, 2, 0, 3, 1]
    host_n, host_o = _collate(case, natural), _collate(case, order)
    other = _run(dev, host_o, soft)
    for k, g in enumerate(order):
        assert _bits(other[0][k]) == _bits(first[0][g]) and other[1][k] == first[1][g] and other[2][k] == first[2][g]
        for side, ptr in ((3, 2), (4, 3)):
            a = other[side][host_o[ptr][k]:host_o[ptr][k + 1]]
            b = first[side][host_n[ptr][g]:host_n[ptr][g + 1]]
            assert np.array_equal(_bits(a), _bits(b)), (g, side)


def test_bad_tables_leave_their_graph_unwritten(dev, ctx):
    """graph 4 gets a pointer pair that is no range of its table (its end lies one past the receptor table; a prefix entry is shared by two graphs, so
    only the last one can be broken alone), graph 2 a column outside 0 .. D - 1: their outputs keep the sentinel the test filled in, in both directions,
    and the other graphs are as in the clean batch.  No bad index is ever dereferenced: the kernels check the pair and the column first."""
    host, want, _ = _reference(4, False)
    clean = _run(dev, host, False)
    l, r, lp, rp, tl, tr, col, grad = _device(dev, host)
    rp_bad, col_bad = rp.clone(), col.clone()
    rp_bad[5] = r.shape[0] + 1
    col_bad[2] = 4
    G = len(SHAPES)
    sent = -7.0
    out = (torch.full((G,), sent, device=dev), torch.full((G,), -7, dtype=torch.int64, device=dev), torch.full((G,), -7, dtype=torch.int64, device=dev),
           torch.full((G, 2), sent, dtype=torch.float64, device=dev))
    loss, pick, target, saved = ctx.node_cross_entropy(l, r, lp, rp_bad, tl, tr, col_bad, False, out=out)
    g_out = (torch.full_like(l, sent), torch.full_like(r, sent))
    g_l, g_r = ctx.node_cross_entropy_backward(grad, l, r, lp, rp_bad, tl, tr, col_bad, target, saved, False, out=g_out)
    loss, pick, target, saved, g_l, g_r = (v.cpu().numpy() for v in (loss, pick, target, saved, g_l, g_r))
    hl, hr = host[2], host[3]
    for g in (2, 4):
        assert loss[g] == sent and pick[g] == -7 and target[g] == -7 and (saved[g] == sent).all(), g
        assert (g_l[hl[g]:hl[g + 1]] == sent).all() and (g_r[hr[g]:hr[g + 1]] == sent).all(), g
    for g in (0, 1, 3):
        assert _bits(loss[g]) == _bits(clean[0][g]) and pick[g] == clean[1][g] and target[g] == clean[2][g]
        assert np.array_equal(_bits(g_l[hl[g]:hl[g + 1]]), _bits(clean[3][hl[g]:hl[g + 1]]))
        assert np.array_equal(_bits(g_r[hr[g]:hr[g + 1]]), _bits(clean[4][hr[g]:hr[g + 1]]))
