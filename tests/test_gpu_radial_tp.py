"""GPU tests of the radial tensor product (ddk_rtp_forward / ddk_rtp_backward): the tensor product of a conv layer with its per-edge weights
w2[g] h + b2[g] formed inside the kernels, through the C ABI, Context.rtp_forward / rtp_backward and tensor_layers.fused_radial_tp.

Reference: autograd of the unmodified reference classes (tests/golden/radial_tp_l0.npz) and the fp64 closed form tests/radial_tp_ref.py (equal to the
former to 1e-12, tests/test_radial_tp_host.py).  Bar: helpers.rel_err < 1e-5, the bar of tests/test_gpu_tp_backward.py, taken PER BLOCK - each weight
block of grad_w2 / grad_b2 per group, each irrep slice of grad_x and out, grad_sh, grad_h.  (An fp32 evaluation with the worst, fully sequential summation
over 5000 random-normal edges stays at 2.6e-6 against fp64 on layers 0 and 3: the arithmetic alone is inside the bar at every size used here.)  The
measured figures are kept in the suite's parity-drift record (test_gpu_round3._record_drift)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import radial_tp_ref as ref
import tp_backward_ref as tpr
from helpers import rel_err
from oracle import score_model_ref as smr
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


def _operands(l, offsets, seed):
    """x, sh, h (what ReLU leaves), w2, b2, grad_out as fp32 numpy"""
    s, E, G = tpr.shape(l), offsets[-1], len(offsets) - 1
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=f(E, s['din']), sh=f(E, 4), h=np.maximum(f(E, 72), 0), w2=f(G, s['W'], 72) / np.float32(np.sqrt(72.0)), b2=f(G, s['W']), g=f(E, s['dout']))


def _to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device(ctx, dev, l, offsets, o, need=(True,) * 5):
    t = {k: _to(dev, v) for k, v in o.items()}
    out = ctx.rtp_forward(l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], tpr.shape(l)['dout'])
    grads = ctx.rtp_backward(l, t['x'], t['sh'], t['h'], offsets, t['w2'], t['b2'], t['g'], need)
    return out.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _reference(l, offsets, o):
    args = (o['x'], o['sh'], o['h'], offsets, o['w2'], o['b2'])
    return ref.forward(l, *args), ref.backward(l, *args, o['g'])


def _out_slices(l):
    O = tpr.shape(l)['O']
    edges = np.cumsum([0, O[0], 3 * O[1], 3 * O[2], O[3]])
    return [(n, slice(int(a), int(b))) for n, a, b in zip(('0e', '1o', '1e', '0o'), edges[:-1], edges[1:]) if b > a]


def _block_errors(l, offsets, got, want):
    """{name: rel_err} per irrep slice of out and grad_x, of grad_sh and grad_h, and per group and weight block of grad_w2 / grad_b2"""
    (out, (gx, gsh, gh, gw2, gb2)), (rout, (rx, rsh, rh, rw2, rb2)) = got, want
    errs = {'grad_sh': rel_err(gsh, rsh), 'grad_h': rel_err(gh, rh)}
    for name, sl in _out_slices(l):
        errs['out.' + name] = rel_err(out[:, sl], rout[:, sl])
    for name, sl in tpr.input_slices(l):
        errs['grad_x.' + name] = rel_err(gx[:, sl], rx[:, sl])
    for g in range(len(offsets) - 1):
        for name, sl in tpr.weight_blocks(l):
            errs[f'grad_w2.g{g}.{name}'] = rel_err(gw2[g, sl], rw2[g, sl])
            errs[f'grad_b2.g{g}.{name}'] = rel_err(gb2[g, sl], rb2[g, sl])
    return errs


def _assert_blocks(tag, l, offsets, got, want):
    assert got[0].shape == want[0].shape and [a.shape for a in got[1]] == [a.shape for a in want[1]]
    if offsets[-1] == 0:      # nothing per edge to compare (rel_err of two empty arrays has no maximum)
        return
    errs = _block_errors(l, offsets, got, want)
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_tp.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


# ---- 1. golden -----------------------------------------------------------------------------------
def test_golden(ctx, dev, golden):
    z = golden('radial_tp_l0')
    offs = [int(o) for o in z['offsets']]
    o = dict(x=z['x'], sh=z['sh'], h=z['h'], w2=z['w2'], b2=z['b2'], g=z['grad_out'])
    got = _device(ctx, dev, 0, offs, o)
    _assert_blocks('golden.l0', 0, offs, got, (z['out'], [z[k] for k in NAMES]))


# ---- 2. all five layers, groups ------------------------------------------------------------------
@pytest.mark.parametrize('l', range(5))
def test_layers_and_groups(ctx, dev, l):
    offs = [0, 1, 1, 34, 70]      # a one-edge group, an empty group, boundaries off the tile grid
    o = _operands(l, offs, 100 + l)
    got = _device(ctx, dev, l, offs, o)
    _assert_blocks(f'groups.l{l}', l, offs, got, _reference(l, offs, o))
    assert not got[1][3][1].any() and not got[1][4][1].any()      # the empty group: exact zeros


# ---- 3. tails ------------------------------------------------------------------------------------
@pytest.mark.parametrize('l,E', [(l, E) for l in (0, 3) for E in (1, 31, 32, 33)])
def test_tails(ctx, dev, l, E):
    offs = [0, E]
    o = _operands(l, offs, 200 + 7 * l + E)
    _assert_blocks(f'tails.l{l}.E{E}', l, offs, _device(ctx, dev, l, offs, o), _reference(l, offs, o))


@pytest.mark.parametrize('l', [0, 3])
def test_no_edges(ctx, dev, l):
    s = tpr.shape(l)
    for offs in ([0, 0], [0, 0, 0, 0, 0]):
        G = len(offs) - 1
        out, (gx, gsh, gh, gw2, gb2) = _device(ctx, dev, l, offs, _operands(l, offs, 1))
        assert out.shape == (0, s['dout']) and gx.shape == (0, s['din']) and gsh.shape == (0, 4) and gh.shape == (0, 72)
        assert gw2.shape == (G, s['W'], 72) and gb2.shape == (G, s['W']) and not gw2.any() and not gb2.any()
    # the C entry itself: E == 0 writes the parameter gradients that were asked for, with no workspace and no operands
    gw2 = torch.full((s['W'], 72), 7.0, device=dev)
    gb2 = torch.full((s['W'],), 7.0, device=dev)
    offs = (C.c_int64 * 2)(0, 0)
    rc = ctx.L.ddk_rtp_backward(ctx.h, l, None, None, None, offs, 1, None, None, None, 0, None, None, None, C.c_void_p(gw2.data_ptr()),
                                C.c_void_p(gb2.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, ctx.L.ddk_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not gw2.any() and not gb2.any()
    assert ctx.L.ddk_rtp_forward(ctx.h, l, None, None, None, offs, 1, None, None, 0, None, None) == 0


# ---- 4. / 5. reduction across slices and workgroups, repeatability ----------------------------------
@pytest.mark.parametrize('l', [0, 3])
def test_reduction_across_slices_and_repeatability(ctx, dev, l):
    offs = [0, 37, 2500, 2501, 5000]      # groups of 37, 2463, 1 and 2499 edges: 1 + 5 + 1 + 5 slices of 512
    o = _operands(l, offs, 400 + l)
    got = _device(ctx, dev, l, offs, o)
    _assert_blocks(f'slices.l{l}', l, offs, got, _reference(l, offs, o))
    again = _device(ctx, dev, l, offs, o)
    assert np.array_equal(got[0], again[0])
    for name, a, b in zip(NAMES, got[1], again[1]):
        assert np.array_equal(a, b), name      # bit for bit


# ---- 6. output subsets ---------------------------------------------------------------------------
SENTINEL = -12345.5


def _guarded(rows, cols, dev):
    buf = torch.full((rows + 2, cols), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[1:rows + 1]


@pytest.mark.parametrize('l', [1, 3])
def test_output_subsets(ctx, dev, l):
    offs, s = [0, 20, 20, 77], tpr.shape(l)
    E, G, W = offs[-1], len(offs) - 1, s['W']
    o = _operands(l, offs, 600 + l)
    ops = {k: _to(dev, v) for k, v in o.items()}
    before = {k: v.clone() for k, v in ops.items()}
    ws = torch.empty(ctx.L.ddk_rtp_backward_workspace(l, E, G) // 4, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    coffs = (C.c_int64 * (G + 1))(*offs)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = ((E, s['din']), (E, 4), (E, 72), (G * W, 72), (G, W))

    def raw(need, w2=True, b2=True, offsets=coffs, n_groups=G, layer=l, n_edges=E, bufs=None):
        bufs = bufs if bufs is not None else [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        rc = ctx.L.ddk_rtp_backward(ctx.h, layer, ptr(ops['x']), ptr(ops['sh']), ptr(ops['h']), offsets, n_groups, ptr(ops['w2']) if w2 else None,
                                    ptr(ops['b2']) if b2 else None, ptr(ops['g']), n_edges, *[ptr(v) for _, v in bufs], ptr(ws), stream())
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
    for need in itertools.product((False, True), repeat=5):
        if not any(need):
            continue
        per_edge = any(need[:3])
        part = call(need, w2=per_edge, b2=need[0] or need[1])      # w2 / b2 are passed only where the rules say they are read
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(a, b), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(ops[k], before[k]) for k in ops)
    # the refusals of the entry, each with a text
    err = lambda: ctx.L.ddk_last_error(ctx.h)
    assert raw((False,) * 5)[0] == -1 and b'no gradient' in err()
    assert raw((True, False, False, False, False), w2=False)[0] == -1 and b'w2' in err()
    assert raw((False, False, True, False, False), w2=False)[0] == -1 and b'w2' in err()
    assert raw((False, True, False, False, False), b2=False)[0] == -1 and b'b2' in err()
    one = (True, False, False, False, False)
    assert raw(one, n_groups=0)[0] == -1 and b'n_groups' in err()
    assert raw(one, n_groups=5)[0] == -1 and b'n_groups' in err()
    assert raw(one, offsets=(C.c_int64 * 4)(0, 30, 20, 77))[0] == -1 and b'monotone' in err()
    assert raw(one, offsets=(C.c_int64 * 4)(0, 20, 20, 76))[0] == -1 and b'last group offset' in err()
    assert raw(one, offsets=(C.c_int64 * 4)(1, 20, 20, 77))[0] == -1 and b'start at 0' in err()
    assert raw(one, layer=-1)[0] == -1 and b'layer' in err()
    assert raw(one, layer=99)[0] == -1 and b'layer' in err()
    assert raw(one, n_edges=-1)[0] == -1
    out = torch.empty(E, s['dout'], device=dev)
    fwd = lambda offsets, n_groups, layer=l: ctx.L.ddk_rtp_forward(ctx.h, layer, ptr(ops['x']), ptr(ops['sh']), ptr(ops['h']), offsets, n_groups, ptr(ops['w2']),
                                                                    ptr(ops['b2']), E, ptr(out), stream())
    assert fwd(coffs, 5) == -1 and b'n_groups' in err()
    assert fwd((C.c_int64 * 4)(0, 30, 20, 77), G) == -1 and b'monotone' in err()
    assert fwd((C.c_int64 * 4)(0, 20, 20, 78), G) == -1 and b'last group offset' in err()
    assert fwd(coffs, G, layer=99) == -1 and b'layer' in err()
    with pytest.raises(RuntimeError, match='needs w2'):
        ctx.rtp_backward(l, ops['x'], ops['sh'], ops['h'], offs, None, None, ops['g'], (True, False, False, True, False))
    torch.cuda.synchronize()


# ---- 7. fused_radial_tp against the unfused composition -------------------------------------------------
def _modules(l, dev, seed):
    from disco_diffdock_amd.tensor_layers import FasterTensorProduct, FCBlock
    i_irr, o_irr = CFG.conv_irreps(l)
    tp = FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr)
    torch.manual_seed(seed)
    fc = torch.nn.ModuleList([FCBlock(72, 72, tp.weight_numel, 2, 0.0) for _ in range(4)]).to(dev)
    return tp, fc


def _fp64_composition(l, offs, fc, x, sh, ea, g):
    """fp64 numpy: fc[k][0] -> ReLU -> the closed form; gradients of every tensor the device test compares, by name"""
    P = [{n: p.detach().cpu().numpy().astype(np.float64) for n, p in blk.named_parameters()} for blk in fc]
    ea64 = ea.astype(np.float64)
    z = np.concatenate([ea64[offs[k]:offs[k + 1]] @ P[k]['0.weight'].T + P[k]['0.bias'] for k in range(4)])
    h = np.maximum(z, 0)
    w2, b2 = np.stack([p['4.weight'] for p in P]), np.stack([p['4.bias'] for p in P])
    out = ref.forward(l, x, sh, h, offs, w2, b2)
    gx, gsh, gh, gw2, gb2 = ref.backward(l, x, sh, h, offs, w2, b2, g)
    gz = gh * (z > 0)
    want = {'out': out, 'x_dst': gx, 'edge_sh': gsh}
    for k in range(4):
        sl = slice(offs[k], offs[k + 1])
        want[f'fc.{k}.4.weight'], want[f'fc.{k}.4.bias'] = gw2[k], gb2[k]
        want[f'fc.{k}.0.weight'], want[f'fc.{k}.0.bias'] = gz[sl].T @ ea64[sl], gz[sl].sum(0)
        want[f'edge_attr.{k}'] = gz[sl] @ P[k]['0.weight']
    return want


@pytest.mark.parametrize('l', [1, 3])
def test_fused_radial_tp_against_the_unfused_composition(ctx, dev, l, monkeypatch):
    from disco_diffdock_amd.tensor_layers import fused_radial_tp
    offs, s = [0, 50, 131, 132, 300], tpr.shape(l)
    E = offs[-1]
    tp, fc = _modules(l, dev, 70 + l)
    rng = np.random.default_rng(700 + l)
    x, sh, ea, g = (rng.standard_normal((E, n)).astype(np.float32) for n in (s['din'], 4, 72, s['dout']))

    def run(fused):
        fc.zero_grad(set_to_none=True)
        X, SH = _to(dev, x).requires_grad_(True), _to(dev, sh).requires_grad_(True)
        EA = [_to(dev, ea[offs[k]:offs[k + 1]]).requires_grad_(True) for k in range(4)]
        out = fused_radial_tp(tp, fc, X, SH, EA) if fused else tp(X, SH, torch.cat([fc[k](EA[k]) for k in range(4)]))
        assert out.shape == (E, s['dout']) and out.grad_fn is not None
        out.backward(_to(dev, g))
        got = {'out': out.detach(), 'x_dst': X.grad, 'edge_sh': SH.grad}
        got.update({f'edge_attr.{k}': EA[k].grad for k in range(4)})
        got.update({'fc.' + n: p.grad for n, p in fc.named_parameters()})
        assert all(v is not None for v in got.values())
        return {k: v.cpu().numpy() for k, v in got.items()}, out

    fused, out = run(True)
    plain, _ = run(False)
    want = _fp64_composition(l, offs, fc, x, sh, ea, g)
    assert set(fused) == set(plain) == set(want) and len(want) == 3 + 4 + 16
    errs = {}
    for k in want:
        assert fused[k].shape == plain[k].shape == want[k].shape, k
        errs[k + '.vs_unfused'] = rel_err(fused[k], plain[k])
        errs[k + '.vs_fp64'] = rel_err(fused[k], want[k])
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'radial_tp.fused.l{l}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])

    # under no_grad only the forward runs, with the same bits
    with torch.no_grad():
        quiet = fused_radial_tp(tp, fc, _to(dev, x), _to(dev, sh), [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)])
    assert quiet.grad_fn is None and not quiet.requires_grad and np.array_equal(quiet.cpu().numpy(), fused['out'])

    # a frozen last Linear: no parameter pass is asked of the kernel, the other gradients are the same bits
    asked = []
    real = ctx.rtp_backward
    monkeypatch.setattr(ctx, 'rtp_backward', lambda *a: asked.append(tuple(a[-1])) or real(*a))
    for blk in fc:
        blk[4].requires_grad_(False)
    fc.zero_grad(set_to_none=True)
    X, SH = _to(dev, x).requires_grad_(True), _to(dev, sh).requires_grad_(True)
    EA = [_to(dev, ea[offs[k]:offs[k + 1]]).requires_grad_(True) for k in range(4)]
    fused_radial_tp(tp, fc, X, SH, EA).backward(_to(dev, g))
    assert asked == [(True, True, True, False, False)]
    assert all(blk[4].weight.grad is None and blk[4].bias.grad is None for blk in fc)
    assert np.array_equal(X.grad.cpu().numpy(), fused['x_dst']) and np.array_equal(SH.grad.cpu().numpy(), fused['edge_sh'])
    for k in range(4):
        assert np.array_equal(EA[k].grad.cpu().numpy(), fused[f'edge_attr.{k}']) and np.array_equal(fc[k][0].weight.grad.cpu().numpy(), fused[f'fc.{k}.0.weight'])
    monkeypatch.undo()
    for blk in fc:
        blk[4].requires_grad_(True)

    # a double backward raises instead of giving zeros
    X4 = _to(dev, x).requires_grad_(True)
    (gx,) = torch.autograd.grad(fused_radial_tp(tp, fc, X4, _to(dev, sh), [_to(dev, ea[offs[k]:offs[k + 1]]) for k in range(4)]), X4, _to(dev, g), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with pytest.raises(RuntimeError, match='GPU only'):
        fused_radial_tp(tp, fc, torch.from_numpy(x), torch.from_numpy(sh), [torch.from_numpy(ea[offs[k]:offs[k + 1]]) for k in range(4)])


def test_fused_radial_tp_single_group(ctx, dev):
    """edge_groups == 1: one FCBlock and one edge_attr tensor"""
    from disco_diffdock_amd.tensor_layers import fused_radial_tp
    l, E = 2, 45
    s = tpr.shape(l)
    tp, fc = _modules(l, dev, 90)
    rng = np.random.default_rng(900)
    x, sh, ea = (_to(dev, rng.standard_normal((E, n)).astype(np.float32)) for n in (s['din'], 4, 72))
    with torch.no_grad():
        got, want = fused_radial_tp(tp, fc[0], x, sh, ea), tp(x, sh, fc[0](ea))
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < BAR


# ---- 8. memory: the point of the feature ---------------------------------------------------------------
def test_peak_memory_stays_below_one_weight_tensor(ctx, dev):
    from disco_diffdock_amd.tensor_layers import fused_radial_tp
    l, E = 3, 50000
    s = tpr.shape(l)
    offs = [0, 12500, 25000, 37500, E]
    tp, fc = _modules(l, dev, 80)
    gen = torch.Generator(device=dev).manual_seed(81)
    x, sh, ea, g = (torch.randn(E, n, device=dev, generator=gen) for n in (s['din'], 4, 72, s['dout']))
    one_w = 4 * E * s['W']

    def peak(fused):
        fc.zero_grad(set_to_none=True)
        X, SH = x.clone().requires_grad_(True), sh.clone().requires_grad_(True)
        EA = [ea[offs[k]:offs[k + 1]].clone().requires_grad_(True) for k in range(4)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        out = fused_radial_tp(tp, fc, X, SH, EA) if fused else tp(X, SH, torch.cat([fc[k](EA[k]) for k in range(4)]))
        out.backward(g)
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - live
        grads = [X.grad.clone()]      # (per edge: no long sum whose order differs between the two paths)
        del out, X, SH, EA
        return used, grads

    fused, gf = peak(True)
    plain, gp = peak(False)
    print(f'peak bytes over forward + backward: fused {fused}, unfused {plain}, one [E, W] tensor {one_w}')
    _record_drift('radial_tp.peak_memory.l3.E50000', fused / one_w, unfused=plain / one_w, bar=1.0)
    assert fused < one_w, (fused, one_w)      # the workspace of the parameter gradients included
    assert plain >= 2 * one_w, (plain, one_w)      # the composition it replaces: the test discriminates
    for a, b in zip(gf, gp):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < BAR
