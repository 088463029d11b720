"""GPU tests of the radial hidden layer (ddk_rhid_forward / ddk_rhid_backward): the cat of the embed loop and fc[g][0..3] of a conv layer as one op from
the edge embedding and the node table, through the C ABI, Context.rhid_forward / rhid_backward, tensor_layers.fused_radial_hidden,
TensorProductConvLayer.forward_embedded and tensor_layers.conv_stack.

Reference: the fp64 restatement tests/radial_hidden_ref.py, its mask from tests/philox_ref.py.  Bar: helpers.rel_err < 1e-5 PER BLOCK, the bar of
tests/test_gpu_radial_conv.py: h and grad_emb, grad_xs, and per group the three 24-column parts of grad_w1 and grad_b1.  Every device number is an fp32
fmaf chain of at most 72 terms, or a fixed-order fp32 sum over the edges of a node or a slice (a few hundred terms here): far inside the bar.

The ReLU kink: an fp32 pre-activation within rounding of zero may take the other branch than fp64.  The fp64 backward therefore differentiates through
the DEVICE's zero pattern (h != 0), and the pattern itself is compared with the fp64 one on every element whose |pre| is at least the classical bound of
the fp32 dot product, 72 * 2^-23 * (sum |w_i a_i| + |b|); at most 0.05 % of the elements (or one) may lie under that margin, which is asserted."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import radial_hidden_ref as ref
from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_radial_conv import _awkward_graph, _bits, _layer_case
from test_gpu_radial_tp import SENTINEL, _guarded, _to
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig()
BAR = 1e-5
NAMES = ('grad_xs', 'grad_emb', 'grad_w1', 'grad_b1')
PARTS = (('emb', slice(0, 24)), ('src', slice(24, 48)), ('dst', slice(48, 72)))


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


def _operands(N, offsets, seed):
    """xs, emb, w1 ~ N(0, 1/72), b1 and grad_h as fp32 numpy"""
    E, G = offsets[-1], len(offsets) - 1
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(xs=f(N, 24), emb=f(E, 24), w1=f(G, 72, 72) / np.float32(np.sqrt(72.0)), b1=f(G, 72), g=f(E, 72))


def _graph(ctx, dev, src, dst, N):
    return ctx.conv_graph(torch.from_numpy(np.asarray(src)).to(dev), torch.from_numpy(np.asarray(dst)).to(dev), N, N)


def _device(ctx, dev, graph, offsets, o, p=0.0, seed=0, need=(True,) * 4):
    t = {k: _to(dev, v) for k, v in o.items()}
    h = ctx.rhid_forward(graph, t['xs'], t['emb'], offsets, t['w1'], t['b1'], p, seed)
    grads = ctx.rhid_backward(graph, t['xs'], t['emb'], h, offsets, t['w1'], t['g'], p, need)
    return h.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _assert_pattern(tag, h, pre, margin, keep):
    """the device's zero pattern against the fp64 one wherever |pre| clears the fp32 bound; the exempt elements are counted and capped"""
    sure = np.abs(pre) >= margin
    exempt, cap = int((~sure).sum()), max(1, int(0.0005 * pre.size))
    print(tag, f'{exempt} of {pre.size} elements under the fp32 margin (cap {cap})')
    assert exempt <= cap, (tag, exempt, cap)
    assert np.array_equal((h != 0)[sure], (keep & (pre > 0))[sure]), tag


def _block_errors(offsets, got, want):
    (h, (gxs, gemb, gw1, gb1)), (rh, (rxs, remb, rw1, rb1)) = got, want
    errs = {'h': rel_err(h, rh), 'grad_xs': rel_err(gxs, rxs), 'grad_emb': rel_err(gemb, remb)}
    for g in range(len(offsets) - 1):
        errs[f'grad_b1.g{g}'] = rel_err(gb1[g], rb1[g])
        for name, sl in PARTS:
            errs[f'grad_w1.g{g}.{name}'] = rel_err(gw1[g][:, sl], rw1[g][:, sl])
    return errs


def _check(ctx, dev, tag, src, dst, N, offsets, seed, p=0.0, mask_seed=0):
    o = _operands(N, offsets, seed)
    h, grads = got = _device(ctx, dev, _graph(ctx, dev, src, dst, N), offsets, o, p, mask_seed)
    E, s = offsets[-1], ref.scale(p)
    keep = ref.keep_mask(mask_seed, E, p)
    pre, margin = ref.pre_activation(o['xs'], src, dst, o['emb'], offsets, o['w1'], o['b1'])
    _assert_pattern(tag, h, pre, margin, keep)
    want = (ref.forward(o['xs'], src, dst, o['emb'], offsets, o['w1'], o['b1'], keep, s),
            ref.backward(o['xs'], src, dst, o['emb'], offsets, o['w1'], h != 0, s, o['g']))      # through the device's own pattern
    assert h.shape == want[0].shape and [a.shape for a in grads] == [a.shape for a in want[1]]
    errs = _block_errors(offsets, got, want)
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_hidden.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])
    return got


# ---- 1. forward and the four gradients on an awkward graph -------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.25])
def test_awkward_graph(ctx, dev, p):
    N, offs = 11, [0, 1, 1, 34, 70]      # a one-edge group, an empty group, boundaries off the wave grid
    # over the first ten nodes: node 9 is never src, node 8 never dst, a self-loop, a duplicated pair; node 10 is neither sender nor receiver
    src, dst = _awkward_graph(N - 1, offs[-1], 5)
    assert (src == N - 2).sum() == 0 and (dst == N - 2).any() and (dst == N - 3).sum() == 0 and (src == N - 3).any()
    h, (gxs, gemb, gw1, gb1) = _check(ctx, dev, f'graph.p{p}', src, dst, N, offs, 100, p, mask_seed=0xC0FFEE12345)
    assert not gw1[1].any() and not gb1[1].any()      # the empty group: exact zeros
    assert not gxs[N - 1].any() and gxs[:N - 1].all(axis=1).all()      # neither sender nor receiver: exact zeros (and nobody else)


# ---- 2. tails and workgroup boundaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 31, 32, 33, 129])
def test_tails(ctx, dev, E):
    N = 5
    rng = np.random.default_rng(E)
    if E == 129:      # every edge shares one src and one dst node: the node sums cross the waves of a workgroup and two workgroups
        src, dst = np.full(E, 2), np.full(E, 4)
    else:
        src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    _check(ctx, dev, f'tails.E{E}', src, dst, N, [0, E], 200 + E, p=0.25 if E == 33 else 0.0, mask_seed=E)


# ---- 3. the mask ---------------------------------------------------------------------------------------------------------------------------------------
def test_mask(ctx, dev):
    N, offs, p = 7, [0, 40, 40, 150, 301], 0.25      # three workgroups' worth of edges, groups that end inside a wave
    E = offs[-1]
    rng = np.random.default_rng(30)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    graph = _graph(ctx, dev, src, dst, N)
    o = _operands(N, offs, 300)
    t = {k: _to(dev, v) for k, v in o.items()}
    pre, margin = ref.pre_activation(o['xs'], src, dst, o['emb'], offs, o['w1'], o['b1'])
    run = lambda seed: ctx.rhid_forward(graph, t['xs'], t['emb'], offs, t['w1'], t['b1'], p, seed)
    seeds = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    h = [run(s) for s in seeds]
    for s, hs in zip(seeds, h):
        keep, on = ref.keep_mask(s, E, p), pre > margin
        assert on.mean() > 0.4
        assert np.array_equal((hs.cpu().numpy() != 0)[on], keep[on])      # element for element, wherever the ReLU surely passes
        assert not (hs.cpu().numpy() != 0)[pre < -margin].any()
    assert not torch.equal(h[0] != 0, h[1] != 0)      # two seeds: two masks
    assert torch.equal(_bits(run(seeds[0])), _bits(h[0]))      # one seed: the same bits
    # the kept elements carry s = 1 / (1 - p) and nothing else: the same bits as the p = 0 run times s
    plain = ctx.rhid_forward(graph, t['xs'], t['emb'], offs, t['w1'], t['b1'], 0.0, 0)
    scaled = plain * torch.tensor(np.float32(1) / (np.float32(1) - np.float32(p)), device=dev)
    assert torch.equal(_bits(torch.where(h[0] != 0, scaled, torch.zeros_like(scaled))), _bits(h[0]))
    # a group table that cuts the same edges differently leaves the mask where it is
    one = ctx.rhid_forward(graph, t['xs'], t['emb'], [0, E], t['w1'][:1], t['b1'][:1], p, seeds[0]).cpu().numpy()
    pre1, margin1 = ref.pre_activation(o['xs'], src, dst, o['emb'], [0, E], o['w1'][:1], o['b1'][:1])
    on = pre1 > margin1
    assert np.array_equal((one != 0)[on], ref.keep_mask(seeds[0], E, p)[on])


# ---- 4. output subsets ---------------------------------------------------------------------------------------------------------------------------
def test_output_subsets(ctx, dev):
    N, offs, p = 40, [0, 700, 1300], 0.25      # 1300 edges: two slices of 512 in the first group, two in the second
    E, G = offs[-1], 2
    rng = np.random.default_rng(50)
    graph = _graph(ctx, dev, rng.integers(0, N, E), rng.integers(0, N, E), N)
    ops = {k: _to(dev, v) for k, v in _operands(N, offs, 500).items()}
    ops['h'] = ctx.rhid_forward(graph, ops['xs'], ops['emb'], offs, ops['w1'], ops['b1'], p, 77)
    before = {k: v.clone() for k, v in ops.items()}
    ws = torch.empty(ctx.L.ddk_rhid_workspace(E, G, N) // 4, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    coffs = (C.c_int64 * (G + 1))(*offs)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = ((N, 24), (E, 24), (G * 72, 72), (G, 72))

    def raw(need, w1=True, p=p):
        # guard rows of 24 / 72 floats keep the views 16-byte aligned or not; the entry asks alignment of its inputs only
        bufs = [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        g = graph
        rc = ctx.L.ddk_rhid_backward(ctx.h, ptr(ops['xs']), N, ptr(g.src), ptr(g.dst), ptr(g.src_order), ptr(g.src_ptr), ptr(g.dst_order), ptr(g.dst_ptr),
                                     ptr(ops['emb']), ptr(ops['h']), coffs, G, ptr(ops['w1']) if w1 else None, ptr(ops['g']), p, E,
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

    full = call((True,) * 4)
    assert all(bool((t != SENTINEL).all()) for t in full)      # every element was written
    again = call((True,) * 4)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, again))      # two full calls: the same bits
    subsets = [need for need in itertools.product((False, True), repeat=4) if any(need)]
    assert len(subsets) == 15
    for need in subsets:
        part = call(need, w1=need[0] or need[1])      # w1 is passed only where the rules say it is read
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(_bits(a), _bits(b)), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(ops[k], before[k]) for k in ops)      # the operands are untouched
    err = lambda: ctx.L.ddk_last_error(ctx.h)
    assert raw((False,) * 4)[0] == -1 and b'no gradient' in err()
    assert raw((True, False, False, False), w1=False)[0] == -1 and b'w1' in err()
    assert raw((False, True, False, False), w1=False)[0] == -1 and b'w1' in err()
    assert raw((True,) * 4, p=1.0)[0] == -1 and b'[0, 1)' in err()
    assert raw((True,) * 4, p=-0.5)[0] == -1 and b'[0, 1)' in err()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='at least one'):
        ctx.rhid_backward(graph, ops['xs'], ops['emb'], ops['h'], offs, ops['w1'], ops['g'], p, need=(False,) * 4)


# ---- 5. no edges, and what is refused ------------------------------------------------------------------------------------------------------------------
def test_no_edges(ctx, dev):
    N = 6
    graph = _graph(ctx, dev, np.zeros(0, np.int64), np.zeros(0, np.int64), N)
    for offs in ([0, 0], [0, 0, 0, 0, 0]):
        G = len(offs) - 1
        h, (gxs, gemb, gw1, gb1) = _device(ctx, dev, graph, offs, _operands(N, offs, 1))
        assert h.shape == (0, 72) and gemb.shape == (0, 24)
        assert gxs.shape == (N, 24) and not gxs.any() and gw1.shape == (G, 72, 72) and gb1.shape == (G, 72) and not gw1.any() and not gb1.any()
    # the C entries themselves write the zeros, with no operands, no tables and no workspace
    full = lambda *shape: torch.full(shape, 7.0, device=dev)
    gxs, gw1, gb1 = full(N, 24), full(72, 72), full(72)
    p = lambda t: C.c_void_p(t.data_ptr())
    offs, stream = (C.c_int64 * 2)(0, 0), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ctx.L.ddk_rhid_forward(ctx.h, None, N, None, None, None, offs, 1, None, None, 0.1, 5, 0, None, stream)
    assert rc == 0, ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_rhid_backward(ctx.h, None, N, None, None, None, None, None, None, None, None, offs, 1, None, None, 0.1, 0, p(gxs), None, p(gw1), p(gb1),
                                 None, stream)
    assert rc == 0, ctx.L.ddk_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not gxs.any() and not gw1.any() and not gb1.any()


def _fc(dev, seed, dropout=0.0, out=200):
    from disco_diffdock_amd.tensor_layers import FCBlock
    torch.manual_seed(seed)
    return torch.nn.ModuleList([FCBlock(72, 72, out, 2, dropout) for _ in range(4)]).to(dev)


def test_refusals(ctx, dev):
    from disco_diffdock_amd.tensor_layers import fused_radial_hidden
    N, offs = 8, [0, 5, 9, 9, 20]
    E = offs[-1]
    rng = np.random.default_rng(60)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    graph = _graph(ctx, dev, src, dst, N)
    o = _operands(N, offs, 600)
    t = {k: _to(dev, v) for k, v in o.items()}
    fwd = lambda graph=graph, p=0.0, **kw: ctx.rhid_forward(graph, kw.get('xs', t['xs']), kw.get('emb', t['emb']), offs, kw.get('w1', t['w1']), t['b1'], p, 0)
    with pytest.raises(RuntimeError, match='device tensors only'):
        fwd(xs=t['xs'].cpu())
    with pytest.raises(RuntimeError, match='device tensors only'):
        fwd(emb=t['emb'].cpu())
    with pytest.raises(RuntimeError, match='on the device'):
        fwd(graph=ctx.conv_graph(torch.from_numpy(src), torch.from_numpy(dst), N, N))      # a graph on another device (the host)
    with pytest.raises(RuntimeError, match='n_in == n_out'):
        fwd(graph=ctx.conv_graph(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), N, N + 1))
    with pytest.raises(RuntimeError, match='ConvGraph'):
        fwd(graph=(src, dst))
    with pytest.raises(RuntimeError, match='w1'):
        fwd(w1=t['w1'][:, :, :71])
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(RuntimeError, match=r'\[0, 1\)'):
            fwd(p=bad)
    h = fwd()
    with pytest.raises(RuntimeError, match='needs w1'):
        ctx.rhid_backward(graph, t['xs'], t['emb'], h, offs, None, t['g'], 0.0, need=(True, False, True, True))
    with pytest.raises(RuntimeError, match='device tensors only'):
        ctx.rhid_backward(graph, t['xs'], t['emb'], h.cpu(), offs, t['w1'], t['g'], 0.0)
    # the module level: the fc layout, the dropout rates
    X, EMB = torch.randn(N, 30, device=dev), t['emb']
    good = _fc(dev, 61)
    assert fused_radial_hidden(good, X, EMB, offs, graph).shape == (E, 72)
    with pytest.raises(RuntimeError, match='GPU only'):
        fused_radial_hidden(good, X.cpu(), EMB, offs, graph)
    wrong = copy.deepcopy(good)
    wrong[2][0] = torch.nn.Linear(72, 72, bias=False).to(dev)
    with pytest.raises(RuntimeError, match='2-layer FCBlocks'):
        fused_radial_hidden(wrong, X, EMB, offs, graph)
    wrong = copy.deepcopy(good)
    wrong[1] = torch.nn.Sequential(*list(good[1])[:4]).to(dev)
    with pytest.raises(RuntimeError, match='2-layer FCBlocks'):
        fused_radial_hidden(wrong, X, EMB, offs, graph)
    wrong = copy.deepcopy(good)
    wrong[0][0] = torch.nn.Linear(48, 72).to(dev)
    with pytest.raises(RuntimeError, match='2-layer FCBlocks'):
        fused_radial_hidden(wrong, X, EMB, offs, graph)
    uneven = _fc(dev, 62, dropout=0.1).train()
    uneven[3][3].p = 0.2
    with pytest.raises(RuntimeError, match='one dropout rate'):
        fused_radial_hidden(uneven, X, EMB, offs, graph)
    assert fused_radial_hidden(uneven.eval(), X, EMB, offs, graph).shape == (E, 72)      # in evaluation no block drops anything
    certain = _fc(dev, 63, dropout=1.0).train()
    with pytest.raises(RuntimeError, match=r'\[0, 1\)'):
        fused_radial_hidden(certain, X, EMB, offs, graph)
    with pytest.raises(RuntimeError, match='group offset'):
        fused_radial_hidden(good, X, EMB, offs[:-1], graph)


# ---- 6. fused_radial_hidden against the composition it replaces ------------------------------------------------------------------------------------
def _composition(fc, X, EMB, ei, offs):
    """the reference's lines: the cat, cut into the groups, through fc[g][:4]"""
    row = torch.cat([EMB, X[ei[0], :24], X[ei[1], :24]], -1)
    return torch.cat([fc[g][:4](row[offs[g]:offs[g + 1]]) for g in range(len(offs) - 1)])


def test_fused_radial_hidden_against_the_composition(ctx, dev, monkeypatch):
    from disco_diffdock_amd.tensor_layers import fused_radial_hidden
    N, offs = 40, [0, 50, 131, 132, 300]
    E = offs[-1]
    fc = _fc(dev, 70).train()      # dropout 0: p = 0
    rng = np.random.default_rng(700)
    x, emb, g = (rng.standard_normal((n, c)).astype(np.float32) for n, c in ((N, 48), (E, 24), (E, 72)))
    ei = torch.from_numpy(np.stack([rng.integers(0, N, E), rng.integers(0, N, E)])).to(dev)
    graph = ctx.conv_graph(ei[0], ei[1], N, N)

    def run(fused):
        fc.zero_grad(set_to_none=True)
        X, EMB = _to(dev, x).requires_grad_(True), _to(dev, emb).requires_grad_(True)
        h = fused_radial_hidden(fc, X, EMB, offs, graph) if fused else _composition(fc, X, EMB, ei, offs)
        assert h.shape == (E, 72) and h.grad_fn is not None
        h.backward(_to(dev, g))
        got = {'h': h.detach(), 'node_attr': X.grad, 'edge_emb': EMB.grad}
        got.update({f'fc.{k}.0.{n}': getattr(fc[k][0], n).grad for k in range(4) for n in ('weight', 'bias')})
        assert all(v is not None for v in got.values()) and all(blk[4].weight.grad is None for blk in fc)
        return {k: v.cpu().numpy() for k, v in got.items()}

    fused, plain = run(True), run(False)
    assert set(fused) == set(plain) and len(fused) == 3 + 8
    assert fused['node_attr'].shape == (N, 48) and not fused['node_attr'][:, 24:].any()      # the slice's backward pads the node row
    errs = {k: rel_err(fused[k], plain[k]) for k in fused}
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift('radial_hidden.fused_vs_composition', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])
    again = run(True)
    assert all(np.array_equal(again[k], fused[k]) for k in fused)      # the same bits again, every gradient

    # under no_grad only the forward runs, with the same bits
    asked = []
    real = ctx.rhid_backward
    monkeypatch.setattr(ctx, 'rhid_backward', lambda *a, **kw: asked.append(a) or real(*a, **kw))
    with torch.no_grad():
        quiet = fused_radial_hidden(fc, _to(dev, x), _to(dev, emb), offs, graph)
    assert quiet.grad_fn is None and not quiet.requires_grad and np.array_equal(quiet.cpu().numpy(), fused['h']) and not asked

    # frozen first Linears and a constant embedding: only grad_xs is asked of the kernel, with the same bits
    for blk in fc:
        blk[0].requires_grad_(False)
    X = _to(dev, x).requires_grad_(True)
    fused_radial_hidden(fc, X, _to(dev, emb), offs, graph).backward(_to(dev, g))
    assert len(asked) == 1 and tuple(asked[0][-1]) == (True, False, False, False)
    assert np.array_equal(X.grad.cpu().numpy(), fused['node_attr'])
    monkeypatch.undo()
    for blk in fc:
        blk[0].requires_grad_(True)

    # seed=None draws from torch's CPU generator: torch.manual_seed reproduces the mask
    drop = _fc(dev, 71, dropout=0.1).train()
    with torch.no_grad():
        torch.manual_seed(5)
        a = fused_radial_hidden(drop, _to(dev, x), _to(dev, emb), offs, graph)
        b = fused_radial_hidden(drop, _to(dev, x), _to(dev, emb), offs, graph)
        torch.manual_seed(5)
        c = fused_radial_hidden(drop, _to(dev, x), _to(dev, emb), offs, graph)
    assert torch.equal(_bits(a), _bits(c)) and not torch.equal(a != 0, b != 0)


# ---- 7. the layer from the edge embedding ----------------------------------------------------------------------------------------------------------
def _layer(l, dev, bn, seed, dropout=0.0):
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    i_irr, o_irr = CFG.conv_irreps(l)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, hidden_features=72, residual=True, batch_norm=bn, dropout=dropout, faster=True, edge_groups=4)
    layer.load_state_dict(smr.random_conv_layer_params(CFG, l, seed, bn), strict=True)
    return layer.to(dev)


@pytest.mark.parametrize('l,bn', [(0, False), (0, True), (3, False), (3, True)])
def test_forward_embedded_against_forward(dev, l, bn):
    offs, s, N, x, sh, ea, g, src, dst = _layer_case(l, dev, 800 + l)
    sizes = [b - a for a, b in zip(offs, offs[1:])]
    emb = ea[:, :24]
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    start = _layer(l, dev, bn, 80 + l)

    def run(embedded):
        layer = copy.deepcopy(start).train()
        X, EMB = _to(dev, x).requires_grad_(True), _to(dev, emb).requires_grad_(True)
        if embedded:
            out = layer.forward_embedded(X, ei, EMB, sizes, _to(dev, sh))
        else:
            row = torch.cat([EMB, X[ei[0], :24], X[ei[1], :24]], -1)
            out = layer(X, ei, list(torch.split(row, sizes)), _to(dev, sh))
        out.backward(_to(dev, g))
        got = {'out': out.detach(), 'node_attr': X.grad, 'edge_emb': EMB.grad}
        got.update({n: p.grad for n, p in layer.named_parameters()})
        got.update({n: b.detach() for n, b in layer.named_buffers()})
        assert all(v is not None for v in got.values())
        return {k: v.cpu().numpy() for k, v in got.items()}

    got, want = run(True), run(False)
    assert set(got) == set(want) and len(want) == 3 + 16 + (4 if bn else 0)
    errs = {k: rel_err(got[k], want[k]) for k in want}
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_hidden.forward_embedded.l{l}.bn{int(bn)}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])


def test_forward_embedded_in_eval_is_forward(dev):
    """on a graph whose nodes receive ONE message each: the inference kernel's scatter adds with float atomics, so with several terms per node two of its
    own runs differ in the last bits"""
    l = 3
    offs, s, N, x, sh, ea, g, src, dst = _layer_case(l, dev, 950)
    sizes = [b - a for a, b in zip(offs, offs[1:])]
    E = offs[-1]
    rng = np.random.default_rng(951)
    layer = _layer(l, dev, True, 95).eval()
    X, EMB, SH = _to(dev, rng.standard_normal((E, s['din'])).astype(np.float32)), _to(dev, ea[:, :24]), _to(dev, sh)
    ei = torch.from_numpy(np.stack([rng.permutation(E), rng.integers(0, E, E)])).to(dev)
    with torch.no_grad():
        row = torch.cat([EMB, X[ei[0], :24], X[ei[1], :24]], -1)
        want = layer(X, ei, list(torch.split(row, sizes)), SH)
        got = layer.forward_embedded(X, ei, EMB, sizes, SH)
    assert torch.equal(_bits(got), _bits(want))
    with pytest.raises(RuntimeError, match='group sizes'):
        layer.forward_embedded(X, ei, EMB, sizes[:3], SH)


# ---- 8. the stack trains with the same bits on every run ----------------------------------------------------------------------------------------------
def test_stack_is_reproducible(dev):
    from disco_diffdock_amd.tensor_layers import conv_stack
    N, sizes = 30, [200, 0, 150, 250]
    E = sum(sizes)
    rng = np.random.default_rng(1000)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    src[:180], dst[100:320] = 3, 3      # a node of degree 180 as src and 220 as dst: where float atomics would reorder
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    x, emb, sh = (rng.standard_normal((n, c)).astype(np.float32) for n, c in ((N, 24), (E, 24), (E, 4)))
    start = torch.nn.ModuleList([_layer(l, dev, True, 110 + l, dropout=0.1) for l in range(3)])

    def run(seed):
        layers = copy.deepcopy(start).train()
        X, EMB = _to(dev, x).requires_grad_(True), _to(dev, emb).requires_grad_(True)
        out = conv_stack(layers, X, ei, EMB, sizes, _to(dev, sh), seed=seed)
        assert out.shape == (N, 24 + 18 + 18 + 24)
        (out * torch.linspace(-1, 1, out.numel(), device=dev).reshape(out.shape)).sum().backward()
        got = {'out': out.detach(), 'node_attr': X.grad, 'edge_emb': EMB.grad}
        got.update({n: p.grad for n, p in layers.named_parameters()})
        assert all(v is not None for v in got.values()) and len(got) == 3 + 3 * 18
        return got

    a, b, c = run(2024), run(2024), run(2025)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k      # one state, one seed: the same bits, every gradient
        assert bool(torch.isfinite(a[k]).all()), k
    assert not torch.equal(a['out'], c['out']) and not torch.equal(a['node_attr'], c['node_attr'])      # another seed: another mask
    assert float((a['node_attr'] != 0).float().mean()) > 0.9


# ---- 9. memory: no [E, 72] tensor is kept but h ------------------------------------------------------------------------------------------------------
def test_peak_memory_is_below_the_composition(ctx, dev):
    from disco_diffdock_amd.tensor_layers import fused_radial_hidden
    E, N = 50000, 2000
    offs = [0, 12500, 25000, 37500, E]
    fc = _fc(dev, 90, dropout=0.1).train()
    gen = torch.Generator(device=dev).manual_seed(91)
    x, emb, g = (torch.randn(n, c, device=dev, generator=gen) for n, c in ((N, 48), (E, 24), (E, 72)))
    ei = torch.randint(0, N, (2, E), device=dev, generator=gen)
    graph = ctx.conv_graph(ei[0], ei[1], N, N)

    def peak(fused):
        fc.zero_grad(set_to_none=True)
        X, EMB = x.clone().requires_grad_(True), emb.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        h = fused_radial_hidden(fc, X, EMB, offs, graph, seed=9) if fused else _composition(fc, X, EMB, ei, offs)
        h.backward(g)
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - live
        del h, X, EMB
        return used

    fused, plain = peak(True), peak(False)
    one = 4 * E * 72
    print(f'peak bytes over forward + backward: radial hidden {fused}, composition {plain}, one [E, 72] tensor {one}')
    _record_drift('radial_hidden.peak_memory.E50000', fused / one, composition=plain / one, bar=plain / one)
    assert fused < plain, (fused, plain)
