"""The kernels that make or feed the DisCo path's discrete decision - gumbel_fwd_kernel / gumbel_bwd_kernel (csrc/k_gumbel.hip), ar_decode_kernel and
ar_logits_kernel (csrc/k_ar.hip) - at their edges (tests/adversarial_latent.py holds the generators and the numpy references; tests/test_latent_choice_host.py
checks on the CPU that the generators have the properties they claim and that every margin used here holds).

A wrong pick is a perfectly valid one-hot, so every expectation here is either EXACT BY CONSTRUCTION (a saturated logit that absorbs the noise, a temperature
at which every exponential is 1, sums of exact integers, NaN / inf / signed-zero rows whose winner the contract names) or protected by a margin that is
asserted on the CPU for every case: the fp64 argmax of logit + gum leads by more than 1e-4, a sampling target is at least 1e-5 of the total away from every
partial sum.  Continuous outputs (y, grad_logit, the predictor logits) are compared ELEMENT-WISE with helpers.elem_err against fp64 and held to the
project's measured bar: the same expressions in fp32 on the host give err32, the device passes under max(4 * err32, 1e-5).  No bar is taken from the device.

elem_err's floor (1e-3 of the largest element, its default, not tuned): at T = 0.01 the softmax's argument is (logit + gum) * 100 and all but a handful
of the y underflow towards 0; those entries are measured against 1e-3 * max y, where both the device and fp64 are 0 to that scale, so they neither pass nor
fail a case.  What the figures at T = 0.01 measure is the few y within e^-6.9 of the largest and the gradient rows that they feed.

Figures are kept through _record_drift under latent_choice.<kernel>.<case>...; the worst per group (elem_err against fp64), measured on an MI355X, `before`
on the kernel as it was (z and the exponential's argument in fp32):

    group                                   figures   worst at         device     host fp32   bar        device / bar
    gumbel two_trips  T = 1     y             32      D3 graph1 d2     2.21e-07   4.03e-07    1.00e-05   0.02     before 8.69e-07
    gumbel two_trips  T = 1     grad_logit    32      D3 graph0 d2     2.15e-06   1.19e-06    1.00e-05   0.21     before 1.46e-05 at graph4 d2 (bar 1.90e-05)
    gumbel two_trips  T = 0.01  y             32      graph0 d0        4.29e-08   4.29e-08    1.00e-05   0.00     before 6.52e-05 at graph4 d2 (bar 4.08e-05): FAILED
    gumbel two_trips  T = 0.01  grad_logit    32      graph5 d0        7.84e-07   6.44e-08    1.00e-05   0.08     before 3.06e-05: FAILED
                                                      graph4 d2        8.86e-08   9.07e-06    3.63e-05   0.00     before 5.80e-05: FAILED
    gumbel sharp      T = 0.01  y              4      d0               4.29e-08   4.29e-08    1.00e-05   0.00
    gumbel sharp      T = 0.01  grad_logit     4      d3               1.98e-06   1.98e-06    1.00e-05   0.20
    gumbel flat       T = 1e30  grad_logit     4      d2               7.84e-07   1.53e-07    1.00e-05   0.08
    ar_logits  H = 128, ns = 24                3      graph0           8.75e-07   8.75e-07    1.00e-05   0.09
    ar_logits  H =  96, ns = 16                3      graph2           4.94e-07   3.22e-07    1.00e-05   0.05
    ar_logits  H =  40, ns =  4, no BatchNorm  3      graph2           3.76e-07   2.93e-07    1.00e-05   0.04
    ar_decode  n = 37, 319, 540; argmax at T = 100 and 1e4 (11 rows each), sampling (53 rows each): 0 wrong rows in all nine launches
    gumbel saturated_ties, flat: y, hard and the losers' out exact in every (graph, d)
(two_trips at T = 0.01, graph0 d0, graph4 d1 and graph5 d3: err32 is 1.0 - the fp32 winner's 1 - y cancels - so the bar is 4 and says nothing there.)

WHAT THE TESTS FOUND, fixed in csrc/k_gumbel.hip in the same change.  gumbel_fwd_kernel formed z = (logit + gum) / T and the exponential's argument z - max z
in fp32.  z is 1 / T times a number of the order of 10; at T = 0.01 it is an fp32 number of 180 .. 700 whose ulp is 1.5e-5 .. 6.1e-5, and every y under the
winner's carries the ABSOLUTE error of z - max z as its RELATIVE error: 6.52e-5 at the runner-up of the 1024-node graph (2.19 under the winner; the host's fp32
chain happens to land 1.0e-5 off there), 3.06e-5 in the one gradient entry that gives the 9-node graph's row its scale.  test_gumbel_two_trips_against_fp64
failed on both at T = 0.01.  The pick was never in doubt (out was the exact one-hot at the fp64 argmax), but the soft sample is what the encoder's gradient
flows through.  The kernel now forms gum, z and z - max z in fp64 (z parked between the passes as an fp32 pair in y's and out's buffers) and rounds the
exponential once; the sums, y = e / sum and the backward stay in fp32 in their fixed order.  include/ddk.h states the new arithmetic: the contract text was the
side that changed, because no fp32 z can do better than half an ulp of 700.
"""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import adversarial_latent as al
import latent_embedding_ref as lref
from helpers import elem_err
from oracle import score_model_ref as smr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F32 = np.float32
FLOOR, K = 1e-5, 4.0


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
    _record_drift(f'latent_choice.{key}', value, **extra)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _measure(key, got, want, host32):
    """elem_err of the device and of the host's fp32 evaluation against fp64 -> (err, bar); printed and recorded"""
    err, err32 = elem_err(got, want), elem_err(host32, want)
    bar = max(K * err32, FLOOR)
    print(f'{key}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
    _record(key, err, host_fp32=err32, bar=bar)
    return err, bar


# ====================================================================================================================================
# Gumbel softmax
# ====================================================================================================================================
def _collate(dev, case, tables, order, pad=0, fill=0.0):
    """the two node tables of the graphs ``order`` (each graph's ligand rows, then ``pad`` rows of ``fill`` past the last pointer) and their pointer tables"""
    D = case['D']
    graphs = [case['graphs'][g] for g in order]
    l = np.concatenate([tables[g][:nl] for g, (nl, nr) in zip(order, graphs)] + [np.full((pad, D), fill, F32)]).reshape(-1, D)
    r = np.concatenate([tables[g][nl:] for g, (nl, nr) in zip(order, graphs)] + [np.full((pad, D), fill, F32)]).reshape(-1, D)
    lp = np.concatenate([[0], np.cumsum([nl for nl, _ in graphs])]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum([nr for _, nr in graphs])]).astype(np.int64)
    return [T(np.ascontiguousarray(a)).to(dev) for a in (l, r, lp, rp)]


def _split(t_l, t_r, graphs):
    out, al_, ar_ = [], 0, 0
    t_l, t_r = t_l.detach().cpu().numpy(), t_r.detach().cpu().numpy()
    for nl, nr in graphs:
        out.append(np.concatenate([t_l[al_:al_ + nl], t_r[ar_:ar_ + nr]]))      # [n, D]: the ligand's nodes first
        al_, ar_ = al_ + nl, ar_ + nr
    return out


def _run(ctx, dev, case, Tm, order=None):
    """Context.gumbel_softmax / gumbel_softmax_backward with explicit pointer tables -> per graph of ``order``: (out, y, grad_logit), each [n, D]"""
    order = list(range(len(case['graphs']))) if order is None else list(order)
    graphs = [case['graphs'][g] for g in order]
    l, r, lp, rp = _collate(dev, case, case['logits'], order)
    gl, gr, _, _ = _collate(dev, case, case['grads'], order)
    out_l, out_r, y_l, y_r = ctx.gumbel_softmax(l, r, lp, rp, Tm, al.GUMBEL_SEED, [case['streams'][g] for g in order], sample=al.GUMBEL_SAMPLE, draw=al.GUMBEL_DRAW)
    g_l, g_r = ctx.gumbel_softmax_backward(y_l, y_r, lp, rp, Tm, gl, gr)
    torch.cuda.synchronize()
    return list(zip(_split(out_l, out_r, graphs), _split(y_l, y_r, graphs), _split(g_l, g_r, graphs)))


@functools.lru_cache(maxsize=None)
def _gumbel_ref(name, g, d, Tm):
    """the references of one (case, graph, d, T), computed once and shared: (argmax, y64, y32, grad64, grad32)"""
    case = al.gumbel_case(name)
    u = al.gumbel_uniforms(case, g, d)
    lg, go = case['logits'][g][:, d], case['grads'][g][:, d]
    _, y, k = lref.gumbel_forward(lg, u, Tm)
    _, y32, _ = lref.gumbel_forward(lg, u, Tm, dtype=F32)
    assert k == al.gumbel_margin(case, g, d)[0]
    return k, y, y32, lref.gumbel_backward(y, go, Tm), lref.gumbel_backward(y32, go, Tm, dtype=F32)


def _assert_one_hot(out, k, who):
    """exactly 0 off the winner ((0 - y) + y), the winner within 2e-7 of 1 ((1 - y) + y: the bound of tests/test_gpu_gumbel.py)"""
    assert not np.delete(out, k).any(), (who, np.flatnonzero(out)[:8])
    assert abs(float(out[k]) - 1.0) < 2e-7, (who, out[k])


@pytest.mark.parametrize('Tm', [1.0, 0.01])
@pytest.mark.parametrize('D', [1, 3, 4])
def test_gumbel_two_trips_against_fp64(dev, ctx, D, Tm):
    """graphs of 1800, 1025, 1, 0, 1024 and 9 nodes (the second trip of all five loops, a single position in a second quad, every thread exactly once, an empty
    graph in the middle, two graphs without a ligand side) at D = 1, 3, 4: out is the exact one-hot at the fp64 argmax, y and grad_logit element-wise.

    Before the kernel formed z in fp64 this failed at T = 0.01, device / host fp32 / bar:  graph5 d0 grad_logit 3.06e-05 / 6.44e-08 / 1.00e-05; graph4 d2 y
    6.52e-05 / 1.02e-05 / 4.08e-05 and grad_logit 5.80e-05 / 9.07e-06 / 3.63e-05 (module docstring, WHAT THE TESTS FOUND); now 7.84e-07, 3.67e-08 and 8.86e-08."""
    case = al.gumbel_case('two_trips', D)
    got = _run(ctx, dev, case, Tm)
    bad = []
    for g, (nl, nr) in enumerate(case['graphs']):
        out, y, grad = got[g]
        assert out.shape == y.shape == grad.shape == (nl + nr, D)
        if nl + nr == 0:
            continue
        for d in range(D):
            k, y64, y32, g64, g32 = _gumbel_ref('two_trips', g, d, Tm)
            _assert_one_hot(out[:, d], k, (g, d))
            assert np.isfinite(y[:, d]).all() and np.isfinite(grad[:, d]).all()
            if nl + nr == 1:
                assert y[0, d] == 1.0 and grad[0, d] == 0.0      # one class: y = 1, the gradient is exactly 0
                continue
            for name, a, want, host in (('y', y[:, d], y64, y32), ('grad_logit', grad[:, d], g64, g32)):
                err, bar = _measure(f'gumbel.two_trips.D{D}.T{Tm}.graph{g}.d{d}.{name}', a, want, host)
                if not err < bar:
                    bad.append((g, d, name, err, bar))
    assert not bad, bad


def test_gumbel_two_trips_through_autograd(dev, ctx):
    """tensor_layers.ragged_gumbel_softmax on batch vectors (the empty graph owns no entry of either) and its autograd backward give the bits of the
    explicit-pointer calls"""
    from disco_diffdock_amd.tensor_layers import ragged_gumbel_softmax
    case = al.gumbel_case('two_trips', 3)
    want = _run(ctx, dev, case, 1.0)
    order = list(range(len(case['graphs'])))
    l, r, _, _ = _collate(dev, case, case['logits'], order)
    gl, gr, _, _ = _collate(dev, case, case['grads'], order)
    lb = torch.from_numpy(np.concatenate([np.full(nl, g) for g, (nl, nr) in enumerate(case['graphs'])]).astype(np.int64)).to(dev)
    rb = torch.from_numpy(np.concatenate([np.full(nr, g) for g, (nl, nr) in enumerate(case['graphs'])]).astype(np.int64)).to(dev)
    l.requires_grad_(), r.requires_grad_()
    out_l, out_r = ragged_gumbel_softmax(l, r, lb, rb, 1.0, al.GUMBEL_SEED, case['streams'], sample=al.GUMBEL_SAMPLE, draw=al.GUMBEL_DRAW)
    torch.autograd.backward([out_l, out_r], [gl, gr])
    outs, grads = _split(out_l, out_r, case['graphs']), _split(l.grad, r.grad, case['graphs'])
    for g in order:
        assert np.array_equal(_bits(outs[g]), _bits(want[g][0])) and np.array_equal(_bits(grads[g]), _bits(want[g][2])), g


def test_gumbel_saturated_ties_exact(dev, ctx):
    """logit 1e30f at k positions: 1e30f + gum == 1e30f, so z ties exactly whatever logf returns.  y is exactly 1 / k there and exactly 0 elsewhere, hard sits
    at the LOWEST tied position - through the per-thread scan (thread 1's second quad), the tree (thread 174 against 175, 250 and 1) and the
    ligand/receptor boundary (699 | 700); in the second graph the lowest tied position, 1000, sits in thread 250 and the other one in thread 1"""
    case = al.gumbel_case('saturated_ties')
    got = _run(ctx, dev, case, case['T'])
    for g, tied in enumerate(case['claims']['tied']):
        out, y, grad = got[g]
        want_y = np.zeros(1200, F32)
        want_y[list(tied)] = F32(1) / F32(len(tied))
        for d in range(case['D']):
            assert np.array_equal(_bits(y[:, d]), _bits(want_y)), (g, d, np.flatnonzero(y[:, d] != want_y)[:8])
            _assert_one_hot(out[:, d], case['claims']['hard'][g], (g, d))
            assert np.isfinite(grad[:, d]).all()


def test_gumbel_flat_all_way_tie(dev, ctx):
    """T = 1e30: every exponential is exactly 1, y exactly 1 / 1105 at all 1105 positions, hard at position 0 - the tie through every thread's scan and every
    level of the tree; the backward on this y element-wise against fp64"""
    case = al.gumbel_case('flat')
    (out, y, grad), = _run(ctx, dev, case, case['T'])
    y0 = case['claims']['y']
    bad = []
    for d in range(case['D']):
        assert np.array_equal(_bits(y[:, d]), _bits(np.full(1105, y0, F32))), (d, np.flatnonzero(y[:, d] != y0)[:8])
        _assert_one_hot(out[:, d], 0, d)
        go = case['grads'][0][:, d]
        want, host = lref.gumbel_backward(np.full(1105, y0), go, case['T']), lref.gumbel_backward(np.full(1105, y0), go, case['T'], dtype=F32)
        assert np.abs(want).max() > 1e-12      # (far above elem_err's absolute 1e-30: the figure measures the rows)
        err, bar = _measure(f'gumbel.flat.d{d}.grad_logit', grad[:, d], want, host)
        if not err < bar:
            bad.append((d, err, bar))
    assert not bad, bad


def test_gumbel_sharp_backward_elementwise(dev, ctx):
    """T = 0.01 on the 1800-node graph with grad_out entries of the scales 1e-20, 1 and 1e20: a global maximum would measure the 1e20 rows alone"""
    case = al.gumbel_case('sharp')
    (out, y, grad), = _run(ctx, dev, case, case['T'])
    bad = []
    for d in range(case['D']):
        k, y64, y32, g64, g32 = _gumbel_ref('sharp', 0, d, case['T'])
        _assert_one_hot(out[:, d], k, d)
        assert np.isfinite(grad[:, d]).all()
        for name, a, want, host in (('y', y[:, d], y64, y32), ('grad_logit', grad[:, d], g64, g32)):
            err, bar = _measure(f'gumbel.sharp.d{d}.{name}', a, want, host)
            if not err < bar:
                bad.append((d, name, err, bar))
    assert not bad, bad


@pytest.mark.parametrize('Tm', [1.0, 0.01])
def test_gumbel_two_trip_graphs_alone_and_inside_a_batch(dev, ctx, Tm):
    """the 1800-node graph has the same bits alone, first in two_trips and in THIRD place behind the empty graph; every graph has the same bits with and
    without the empty graph in the batch"""
    case = al.gumbel_case('two_trips')
    full = _run(ctx, dev, case, Tm)
    same = lambda a, b: all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    moved_order = [1, 3, 0, 2, 4, 5]
    moved = _run(ctx, dev, case, Tm, moved_order)
    alone = _run(ctx, dev, case, Tm, [0])
    assert same(alone[0], full[0]) and same(moved[2], full[0])
    for at, g in enumerate(moved_order):
        assert same(moved[at], full[g]), g
    no_empty = [0, 1, 2, 4, 5]
    without = _run(ctx, dev, case, Tm, no_empty)
    for at, g in enumerate(no_empty):
        assert same(without[at], full[g]), g
    assert all(a.shape == (0, al.D_MAX) for a in full[3])


def test_gumbel_leaves_the_rows_past_the_last_pointer_alone(dev, ctx):
    """logit, y, out and grad_logit tables with 8 sentinel rows past ptr[G] on both sides: untouched by the forward and by the backward (through the C ABI:
    Context.gumbel_softmax allocates its own outputs)"""
    from disco_diffdock_amd.runtime import _ptr, _stream
    case = al.gumbel_case('two_trips', 3)
    order, D, G, PAD, MARK = list(range(len(case['graphs']))), 3, len(case['graphs']), 8, 777.25
    l, r, lp, rp = _collate(dev, case, case['logits'], order, pad=PAD, fill=MARK)
    gl, gr, _, _ = _collate(dev, case, case['grads'], order, pad=PAD, fill=MARK)
    st = T(np.array(case['streams'], dtype=np.uint64).view(np.int64)).to(dev)
    marked = lambda t: torch.full_like(t, MARK)
    y_l, y_r, out_l, out_r, g_l, g_r = marked(l), marked(r), marked(l), marked(r), marked(l), marked(r)
    l0, r0 = l.clone(), r.clone()
    ctx._check(ctx.L.ddk_gumbel_softmax_batch(ctx.h, G, D, _ptr(l), l.shape[0], _ptr(r), r.shape[0], _ptr(lp), _ptr(rp), 1.0, C.c_uint64(al.GUMBEL_SEED), _ptr(st),
                                              al.GUMBEL_SAMPLE, al.GUMBEL_DRAW, _ptr(y_l), _ptr(y_r), _ptr(out_l), _ptr(out_r), _stream()), 'ddk_gumbel_softmax_batch')
    torch.cuda.synchronize()
    nl, nr = int(lp[-1]), int(rp[-1])
    assert l.shape[0] == nl + PAD and r.shape[0] == nr + PAD
    assert torch.equal(l, l0) and torch.equal(r, r0)
    for t, n in ((y_l, nl), (out_l, nl), (y_r, nr), (out_r, nr)):
        assert (t[n:] == MARK).all() and not (t[:n] == MARK).any()
    ctx._check(ctx.L.ddk_gumbel_softmax_batch_backward(ctx.h, G, D, _ptr(y_l), y_l.shape[0], _ptr(y_r), y_r.shape[0], _ptr(lp), _ptr(rp), 1.0, _ptr(gl), _ptr(gr),
                                                       _ptr(g_l), _ptr(g_r), _stream()), 'ddk_gumbel_softmax_batch_backward')
    torch.cuda.synchronize()
    for t, n in ((g_l, nl), (g_r, nr), (y_l, nl), (y_r, nr)):
        assert (t[n:] == MARK).all() and not (t[:n] == MARK).any()
    want = _run(ctx, dev, case, 1.0)      # and the padded tables give the bits of the unpadded ones
    outs, grads = _split(out_l[:nl], out_r[:nr], case['graphs']), _split(g_l[:nl], g_r[:nr], case['graphs'])
    for g in order:
        assert np.array_equal(_bits(outs[g]), _bits(want[g][0])) and np.array_equal(_bits(grads[g]), _bits(want[g][2])), g


# ====================================================================================================================================
# AR decode
# ====================================================================================================================================
@pytest.fixture(scope='module')
def complexes(dev, ctx):
    """one topology-only Complex per graph size (ddk_ar_decode needs no AR weights), created on first use"""
    from disco_diffdock_amd.runtime import Complex
    made = {}

    def get(n_lig, n_rec):
        if (n_lig, n_rec) not in made:
            made[n_lig, n_rec] = Complex(ctx, al.chain_complex(n_lig, n_rec), max_batch=4)
        return made[n_lig, n_rec]
    return get


def _decode(cx, dev, logits, Tm, u, latent_dim=3, idx=1):
    B = logits.shape[0]
    lat_l = torch.zeros(B * cx.n_lig, latent_dim, device=dev)
    lat_r = torch.zeros(B * cx.n_rec, latent_dim, device=dev)
    choices = torch.full((B, latent_dim), -1, dtype=torch.int32, device=dev)
    cx.ar_decode(T(logits).to(dev), Tm, None if u is None else T(u).to(dev), idx, lat_l, lat_r, choices)
    torch.cuda.synchronize()
    return choices.cpu().numpy(), lat_l.cpu().numpy().reshape(B, cx.n_lig, latent_dim), lat_r.cpu().numpy().reshape(B, cx.n_rec, latent_dim)


@pytest.mark.parametrize('mode', ['argmax_T100', 'argmax_T1e4', 'sample'])
@pytest.mark.parametrize('n_lig,n_rec', al.AR_SIZES)
def test_ar_decode_corner_rules(dev, complexes, n_lig, n_rec, mode):
    """ddk_ar_decode on n = 37, 319 and 540 logits (1, 2 and 3 per thread; at 319 the threads from 160 on own none), one launch per size and mode with one
    graph per row: unique maxima at both ends of both sides, ties across thread chunks and the ligand/receptor boundary, all -inf, NaN after +inf, two NaNs,
    products that overflow, -0.0 before 0.0; sampling with integer sums at u = 0, 0.5, k / n and 1 - 2^-24, leading zero mass, one +inf, two clamped overflows, an
    all-zero total, and 40 random rows whose margin the CPU test asserts.  choices, both latent arrays (one 1.0 per graph in column 1 on the right side of the
    boundary, exact zeros elsewhere), the untouched columns, and equal bits on a second call."""
    cx = complexes(n_lig, n_rec)
    assert (cx.n_lig, cx.n_rec) == (n_lig, n_rec)
    n = n_lig + n_rec
    cases = al.ar_decode_cases(n_lig, n_rec)
    rows = cases['sample'] if mode == 'sample' else cases['argmax']
    Tm = al.AR_SAMPLE_T if mode == 'sample' else al.AR_ARGMAX_T[mode == 'argmax_T1e4']
    logits = np.stack([r['logits'] for r in rows])
    u = np.array([r['u'] for r in rows], F32) if mode == 'sample' else None
    expect = np.array([r['expect'] for r in rows])
    B = len(rows)
    choices, lat_l, lat_r = _decode(cx, dev, logits, Tm, u)
    wrong = [(r['name'], int(c), r['expect']) for r, c in zip(rows, choices[:, 1]) if c != r['expect']]
    print(f'ar_decode n = {n} {mode}: {B} rows, {len(wrong)} wrong')
    _record(f'ar_decode.n{n}.{mode}.wrong_rows', len(wrong), rows=B, bar=0)
    assert not wrong, wrong
    assert (choices[:, 0] == -1).all() and (choices[:, 2] == -1).all()
    want_l, want_r = np.zeros((B, n_lig, 3), F32), np.zeros((B, n_rec, 3), F32)
    for b, c in enumerate(expect):
        if c < n_lig:
            want_l[b, c, 1] = 1.0
        else:
            want_r[b, c - n_lig, 1] = 1.0
    assert np.array_equal(_bits(lat_l), _bits(want_l)) and np.array_equal(_bits(lat_r), _bits(want_r))
    assert (expect < n_lig).any() and (expect >= n_lig).any()
    again = _decode(cx, dev, logits, Tm, u)
    assert all(np.array_equal(a, b) for a, b in zip((choices, _bits(lat_l), _bits(lat_r)), (again[0], _bits(again[1]), _bits(again[2]))))


# ====================================================================================================================================
# AR logits
# ====================================================================================================================================
SCORE_ARGS = dict(ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32, max_radius=5.0, cross_max_distance=80,
                  dynamic_max_cross=True, embedding_scale=1000, embedding_type='sinusoidal', scale_by_sigma=True, no_torsion=False, no_batch_norm=False, dropout=0.1,
                  sh_lmax=1, use_second_order_repr=False, use_old_atom_encoder=False, esm_embeddings_path='x', latent_dim=2, latent_vocab=1, latent_droprate=0.1,
                  latent_cross_attention=False, tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14)
AR_CFG = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)


@pytest.mark.parametrize('H,ns,no_bn,stats', al.AR_LOGITS_CASES)
def test_ar_logits_against_fp64_on_the_device_rows(dev, H, ns, no_bn, stats):
    """ddk_ar_logits at (H, ns) = (128, 24): the widest input; (96, 16): the zero-padded hidden units; (40, 4) without BatchNorm; the BatchNorm statistics with
    running_var down to 1e-6 (eps decides the scale), negative and zero weights, means of 3 sigma.  B = 3 copies of an 11-atom, 43-residue complex: 33 ligand
    rows (one tile plus one row) and 129 residue rows (four tiles plus one).  The reference reads the DEVICE's own last-layer rows, so the comparison isolates
    the predictor kernel and the fold of ddk_finalize_weights from the conv stack; per graph, so that a row written to another graph's place shows."""
    from disco_diffdock_amd.data import from_arrays, collate
    from disco_diffdock_amd.model_utils import get_ar_model
    from disco_diffdock_amd.score_model import complex_for_batch
    P, _ = al.ar_state_dict(AR_CFG, H, ns, no_bn, stats)
    ar_args = Namespace(use_pretrained_score=True, ns=ns, latent_no_batchnorm=no_bn, latent_dropout=0.0, latent_hidden_dim=H, esm_embeddings_path='x', no_randomness=False)
    ar = get_ar_model(ar_args, Namespace(**SCORE_ARGS), dev, training=False)
    ar.load_state_dict(P, strict=True)
    ar.eval()
    spec = al.AR_LOGITS_COMPLEX
    n_lig, n_rec, B = spec['n_lig'], spec['n_rec'], spec['B']
    c = al.chain_complex(n_lig, n_rec, spec['seed'])
    rng = np.random.default_rng(5)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 2.0, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(B)]).astype(F32)
    b = collate([from_arrays(c) for _ in range(B)])
    b['ligand'].pos = T(pos.reshape(-1, 3))
    b = b.to(dev)
    b['ligand'].input_latent = torch.zeros(B * n_lig, 2, device=dev)
    b['receptor'].input_latent = torch.zeros(B * n_rec, 2, device=dev)
    with torch.no_grad():
        logits = ar.logits(b)
    cx, _ = complex_for_batch(b, dev, ctx=ar.pretrained_score_model.ctx)
    lig, rec = [x.cpu().numpy() for x in cx.node_features(B, dev)]
    logits = logits.cpu().numpy()
    assert logits.shape == (B, 1, n_lig + n_rec) and lig.shape == (B * n_lig, 84) and rec.shape == (B * n_rec, 84)
    assert np.isfinite(logits).all() and np.isfinite(lig).all() and np.isfinite(rec).all() and np.abs(rec).max() > 0
    assert not np.array_equal(lig[:n_lig], lig[n_lig:2 * n_lig])      # the graphs differ (their poses do): a row in another graph's place shows
    want, host = al.ar_logits_ref(lig, rec, P, ns, B), al.ar_logits_ref(lig, rec, P, ns, B, dtype=F32)
    bad = []
    for g in range(B):
        err, bar = _measure(f'ar_logits.H{H}.ns{ns}.graph{g}', logits[g, 0], want[g], host[g])
        if not err < bar:
            bad.append((g, err, bar))
    assert not bad, bad
