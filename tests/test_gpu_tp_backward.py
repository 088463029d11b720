"""GPU tests of ddk_tp_backward, the vector-Jacobian product of FasterTensorProduct.forward (reference models/tensor_layers.py:65-116), through the C ABI,
Context.tp_backward and the autograd Function of disco_diffdock_amd.tensor_layers.FasterTensorProduct.

Reference: autograd of the unmodified reference class (tests/golden/faster_tp_backward_l*.npz), the fp64 closed form tests/tp_backward_ref.py (equal to
the former to 1e-12, tests/test_tp_backward_host.py) and fp64 autograd of the oracle's conv layer.  Bar: helpers.rel_err < 1e-5, the forward's bar
(tests/test_gpu_ops.py; the sums are as long), taken PER BLOCK - each weight block of grad_w, each irrep slice of grad_x, grad_sh - so that a large
block cannot hide a small one.  The measured figures are kept in the suite's parity-drift record (test_gpu_round3._record_drift)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tp_backward_ref as ref
from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig()
BAR = 1e-5
GRID = 4096      # the kernel's persistent grid (csrc/k_tp_shape.h tp_persistent_grid)


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


def _operands(l, E, seed):
    s = ref.shape(l)
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((E, n)).astype(np.float32) for n in (s['din'], 4, s['W'], s['dout'])]


def _device_backward(ctx, dev, l, x, sh, w, g, need=(True, True, True)):
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, sh, w, g)]
    out = ctx.tp_backward(l, t[0], t[1], t[2], t[3], need)
    return [None if o is None else o.cpu().numpy() for o in out]


def _block_errors(l, got, want):
    """{name: rel_err} per weight block of grad_w, per irrep slice of grad_x, and of grad_sh"""
    gx, gsh, gw = got
    rx, rsh, rw = want
    errs = {'grad_sh': rel_err(gsh, rsh)}
    for name, sl in ref.input_slices(l):
        errs['grad_x.' + name] = rel_err(gx[:, sl], rx[:, sl])
    for name, sl in ref.weight_blocks(l):
        errs['grad_w.' + name] = rel_err(gw[:, sl], rw[:, sl])
    return errs


def _assert_blocks(tag, l, got, want):
    errs = _block_errors(l, got, want)
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'tp_backward.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])


# ---- 1. golden -----------------------------------------------------------------------------------
@pytest.mark.parametrize('l', range(5))
def test_golden(ctx, dev, golden, l):
    z = golden(f'faster_tp_backward_l{l}')
    got = _device_backward(ctx, dev, l, z['x'], z['sh'], z['w'], z['grad_out'])
    assert [a.shape for a in got] == [z[k].shape for k in ('grad_x', 'grad_sh', 'grad_w')]
    _assert_blocks(f'golden.l{l}', l, got, (z['grad_x'], z['grad_sh'], z['grad_w']))


# ---- 2. sizes and tails ----------------------------------------------------------------------------
@pytest.mark.parametrize('l,E', [(l, 65) for l in range(5)] + [(l, E) for l in (0, 3) for E in (1, 2, 2 * GRID + 809)])
def test_sizes_and_tails(ctx, dev, l, E):
    ops = _operands(l, E, 100 + 7 * l + E % 13)
    got = _device_backward(ctx, dev, l, *ops)
    _assert_blocks(f'sizes.l{l}.E{E}', l, got, ref.backward(l, *ops))


def test_no_edges(ctx, dev):
    for l in (0, 3):
        s = ref.shape(l)
        gx, gsh, gw = _device_backward(ctx, dev, l, *_operands(l, 0, 1))
        assert gx.shape == (0, s['din']) and gsh.shape == (0, 4) and gw.shape == (0, s['W'])
        z = torch.zeros(4, device=dev)      # the C entry itself: E == 0 is DDK_OK with any pointers
        p = C.c_void_p(z.data_ptr())
        assert ctx.L.ddk_tp_backward(ctx.h, l, p, p, p, p, 0, p, p, p, None) == 0


# ---- 3. output subsets -----------------------------------------------------------------------------
SENTINEL = -12345.5


def _guarded(E, cols, dev):
    buf = torch.full((E + 2, cols), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[1:E + 1]


@pytest.mark.parametrize('l', [1, 3])
def test_output_subsets(ctx, dev, l):
    E = 77
    s = ref.shape(l)
    ops = [torch.from_numpy(a).to(dev) for a in _operands(l, E, 300 + l)]
    before = [t.clone() for t in ops]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(need, with_w=True):
        bufs = [_guarded(E, n, dev) if on else (None, None) for on, n in zip(need, (s['din'], 4, s['W']))]
        rc = ctx.L.ddk_tp_backward(ctx.h, l, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]) if with_w else None, ptr(ops[3]), E,
                                   ptr(bufs[0][1]), ptr(bufs[1][1]), ptr(bufs[2][1]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, ctx.L.ddk_last_error(ctx.h)
        torch.cuda.synchronize()
        for full, _ in bufs:
            if full is not None:      # the guard rows in front and behind still hold the sentinel
                assert bool((full[0] == SENTINEL).all()) and bool((full[-1] == SENTINEL).all())
        return [None if v is None else v.clone() for _, v in bufs]

    full = call((True, True, True))
    assert all(bool((t != SENTINEL).all()) for t in full)      # every element was written
    for need, with_w in (((True, True, True), True), ((False, False, True), False), ((True, True, False), True), ((True, False, False), True),
                         ((False, True, False), True)):
        part = call(need, with_w)
        for on, a, b in zip(need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(a, b), (need, with_w)      # the same bits as the all-outputs call, and from one call to the next
    assert all(torch.equal(a, b) for a, b in zip(ops, before))
    # the refusals of the entry: nothing asked for; w missing where it is needed
    assert ctx.L.ddk_tp_backward(ctx.h, l, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), ptr(ops[3]), E, None, None, None, None) == -1
    gx = torch.empty(E, s['din'], device=dev)
    assert ctx.L.ddk_tp_backward(ctx.h, l, ptr(ops[0]), ptr(ops[1]), None, ptr(ops[3]), E, ptr(gx), None, None, None) == -1
    with pytest.raises(RuntimeError, match='needs w'):
        ctx.tp_backward(l, ops[0], ops[1], None, ops[3], (True, False, True))


# ---- 4. index exactness ----------------------------------------------------------------------------
@pytest.mark.parametrize('l', range(5))
def test_index_exactness(ctx, dev, l):
    """One-hot grad_out (edge e carries unit vector e) pins every column decode, one-hot x every row decode: where fp64 gives an exact 0 the device
    gives 0.0, elsewhere the bar applies."""
    s = ref.shape(l)
    for what, n, pos in (('grad_out', s['dout'], 3), ('x', s['din'], 0)):
        ops = _operands(l, n, 400 + l)
        ops[pos] = np.eye(n, dtype=np.float32)
        got, want = _device_backward(ctx, dev, l, *ops), ref.backward(l, *ops)
        for name, a, b in zip(('grad_x', 'grad_sh', 'grad_w'), got, want):
            zero = b == 0.0
            assert zero.any() or name != 'grad_w'      # all but one column (row class) of every weight block
            assert np.all(a[zero] == 0.0), (what, name, int(np.count_nonzero(a[zero])))
        _assert_blocks(f'onehot_{what}.l{l}', l, got, want)


# ---- 5. adjoint identities against the forward kernel ----------------------------------------------
@pytest.mark.parametrize('l', range(5))
def test_adjoint_identities(ctx, dev, l):
    """The op is linear in each of x, sh, w: per edge, sum g . out = sum grad_x . x = sum grad_sh . sh = sum grad_w . w.  Sums in fp64 on the host from
    device results of both kernels; no oracle."""
    E = 130
    ops = _operands(l, E, 500 + l)
    t = [torch.from_numpy(a).to(dev) for a in ops]
    out = ctx.tp_forward(l, t[0], t[1], t[2], ref.shape(l)['dout']).cpu().numpy().astype(np.float64)
    gx, gsh, gw = (a.astype(np.float64) for a in _device_backward(ctx, dev, l, *ops))
    x, sh, w, g = (a.astype(np.float64) for a in ops)
    sums = [(g * out).sum(1), (gx * x).sum(1), (gsh * sh).sum(1), (gw * w).sum(1)]
    scale = np.abs(gw * w).sum(1)
    worst = max(float((np.abs(a - sums[3]) / scale).max()) for a in sums[:3])
    print('adjoint', l, worst)
    _record_drift(f'tp_backward.adjoint.l{l}', worst, bar=BAR)
    assert worst < BAR


# ---- 6. operands -----------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [0, 2, 3])
def test_operand_classes(ctx, dev, l):
    E = 70
    x, sh, w, g = _operands(l, E, 600 + l)
    gx, gsh, gw = _device_backward(ctx, dev, l, x, sh, w, np.zeros_like(g))
    assert not gx.any() and not gsh.any() and not gw.any()
    gx, gsh, gw = _device_backward(ctx, dev, l, np.zeros_like(x), sh, w, g)
    assert not gsh.any() and not gw.any()
    assert rel_err(gx, ref.backward(l, np.zeros_like(x), sh, w, g)[0]) < BAR
    sh0 = sh.copy()
    sh0[::2] = (1.0, 0.0, 0.0, 0.0)      # the zero-length edge: v = 0, s0 = 1
    got = _device_backward(ctx, dev, l, x, sh0, w, g)
    assert np.isfinite(np.concatenate([a.reshape(-1) for a in got])).all()
    _assert_blocks(f'zero_length.l{l}', l, got, ref.backward(l, x, sh0, w, g))
    # powers of two: grad_w and grad_sh are linear in x, grad_x does not see it - bit for bit, so no reduced-precision path hides anywhere
    base = _device_backward(ctx, dev, l, x, sh, w, g)
    for k in (10, -10):
        f = np.float32(2.0 ** k)
        sx, ssh, sw = _device_backward(ctx, dev, l, x * f, sh, w, g)
        assert np.array_equal(sx, base[0]) and np.array_equal(ssh, base[1] * f) and np.array_equal(sw, base[2] * f)


# ---- 7. autograd -----------------------------------------------------------------------------------
def _tp_module(l):
    from disco_diffdock_amd.tensor_layers import FasterTensorProduct
    i_irr, o_irr = CFG.conv_irreps(l)
    return FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr)


def test_autograd_function(ctx, dev):
    l = 3
    s = ref.shape(l)
    tp = _tp_module(l)
    x, sh, w, g = _operands(l, 66, 700)
    lead = (2, 33)
    X, SH, Wt = (torch.from_numpy(a).to(dev).reshape(lead + (-1,)).requires_grad_(True) for a in (x, sh, w))
    G = torch.from_numpy(g).to(dev).reshape(lead + (-1,))
    out = tp(X, SH, Wt)
    assert out.shape == lead + (s['dout'],) and out.grad_fn is not None
    with torch.no_grad():
        plain = tp(X, SH, Wt)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, out.detach())
    assert torch.equal(plain.reshape(-1, s['dout']), ctx.tp_forward(l, X.detach().reshape(-1, s['din']), SH.detach().reshape(-1, 4), Wt.detach().reshape(-1, s['W']), s['dout']))
    out.backward(G)
    assert X.grad.shape == X.shape and SH.grad.shape == SH.shape and Wt.grad.shape == Wt.shape
    got = [t.grad.reshape(66, -1).cpu().numpy() for t in (X, SH, Wt)]
    _assert_blocks('autograd.l3', l, got, ref.backward(l, x, sh, w, g))

    # only the weight requires grad: the other two get nothing
    X2, SH2 = X.detach().clone(), SH.detach().clone()
    W2 = Wt.detach().clone().requires_grad_(True)
    tp(X2, SH2, W2).backward(G)
    assert X2.grad is None and SH2.grad is None and torch.equal(W2.grad, Wt.grad)

    # a strided grad_outputs, on a side stream
    side = torch.cuda.Stream(device=dev)
    Gs = torch.from_numpy(g).to(dev).reshape(lead + (-1,)).repeat_interleave(2, dim=-1)[..., ::2]
    assert not Gs.is_contiguous() and torch.equal(Gs, G)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        X3, SH3, W3 = (t.detach().clone().requires_grad_(True) for t in (X, SH, Wt))
        grads = torch.autograd.grad(tp(X3, SH3, W3), (X3, SH3, W3), Gs)
    side.synchronize()
    assert all(torch.equal(a, b.grad) for a, b in zip(grads, (X, SH, Wt)))

    # a double backward raises instead of giving zeros
    X4 = X.detach().clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(tp(X4, SH2, W2.detach()), X4, G, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()

    with pytest.raises(RuntimeError, match='GPU only'):
        tp(X.detach().cpu(), SH.detach().cpu(), Wt.detach().cpu())


# ---- 8. the reason for the feature -------------------------------------------------------------------
def test_radial_mlp_receives_gradients_through_the_op_boundary(dev):
    """The reference's op boundary in training: torch fc -> FasterTensorProduct -> index_add_ mean.  Every fc parameter of every edge group, and the
    node features, get a gradient, equal to fp64 autograd of the oracle's conv layer."""
    l, N, E = 3, 40, 600
    splits = [0, 100, 250, 450, E]
    i_irr, o_irr = CFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(CFG, l, 81, False)
    g = torch.Generator().manual_seed(82)
    node = torch.randn(N, smr.irreps_dim(i_irr), generator=g)
    ei = torch.randint(0, N, (2, E), generator=g)
    ea, sh = torch.randn(E, 72, generator=g), torch.randn(E, 4, generator=g)
    gout = torch.randn(N, smr.irreps_dim(o_irr), generator=g)
    names = [f'fc.{k}.{i}.{p}' for k in range(4) for i in (0, 4) for p in ('weight', 'bias')]

    # fp64 autograd of the oracle
    P64 = {'L.' + k: v.double().requires_grad_(k in names) for k, v in Pl.items()}
    node64 = node.double().requires_grad_(True)
    o64 = smr.tp_conv_layer(P64, 'L', node64, ei, [ea.double()[splits[i]:splits[i + 1]] for i in range(4)], sh.double(), i_irr, '1x0e+1x1o', o_irr,
                            residual=False, batch_norm=False, faster=True, edge_groups=4)
    o64.backward(gout.double())

    # the device path
    tp = _tp_module(l)
    Pd = {k: v.to(dev).requires_grad_(k in names) for k, v in Pl.items()}
    node_d = node.to(dev).requires_grad_(True)
    ei_d, ea_d, sh_d = ei.to(dev), ea.to(dev), sh.to(dev)
    lin = torch.nn.functional.linear
    w = torch.cat([lin(torch.relu(lin(ea_d[splits[k]:splits[k + 1]], Pd[f'fc.{k}.0.weight'], Pd[f'fc.{k}.0.bias'])), Pd[f'fc.{k}.4.weight'], Pd[f'fc.{k}.4.bias'])
                   for k in range(4)])
    msg = tp(node_d[ei_d[1]], sh_d, w)
    summed = torch.zeros(N, msg.shape[1], device=dev).index_add_(0, ei_d[0], msg)
    out = summed / torch.bincount(ei_d[0], minlength=N).clamp(min=1).unsqueeze(1)
    assert rel_err(out.detach().cpu(), o64.detach()) < BAR
    out.backward(gout.to(dev))

    errs = {'node': rel_err(node_d.grad.cpu(), node64.grad)}
    assert node_d.grad.abs().max() > 0
    for k in names:
        assert Pd[k].grad is not None and float(Pd[k].grad.abs().max()) > 0, k
        errs[k] = rel_err(Pd[k].grad.cpu(), P64['L.' + k].grad)
    print({k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift('tp_backward.op_boundary_training.l3', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (worst, errs[worst])
