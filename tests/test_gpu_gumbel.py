"""GPU tests of the ragged straight-through Gumbel softmax (ddk_gumbel_softmax_batch / ddk_gumbel_softmax_batch_backward, csrc/k_gumbel.hip) through
Context.gumbel_softmax and tensor_layers.ragged_gumbel_softmax: G = 3 graphs of (5 + 7), (1 + 0) and (16 + 300) ligand + receptor nodes, D = 2.

Reference: tests/latent_embedding_ref.py in fp64 from the host mirror's uniforms (DDK_GUMBEL_LAYOUT 1, bit-exact).  The bar of an output is MEASURED, as in
the sibling op tests: the same expressions in fp32 on the host against fp64 give err32, the device passes under 4 * err32 floored at 1e-5.  At T = 0.01 the
softmax's argument is (logit + gum) * 100: an fp32 rounding of the noise, 2^-24 * |gum| * 100, moves y by that relative amount, which err32 measures."""
import numpy as np
import pytest
import torch

import latent_embedding_ref as lref
from helpers import _bits, rel_err
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
GRAPHS = ((5, 7), (1, 0), (16, 300))
D, SEED, SAMPLE, DRAW = 2, 0x1234567890ABCDEF, 3, 17
FLOOR = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _streams(n=len(GRAPHS)):
    from disco_diffdock_amd.runtime import stream_id
    return [stream_id(f'gumbel_{i}') for i in range(n)]


def _case(graphs=GRAPHS, seed=1):
    rng = np.random.default_rng(seed)
    per = [(rng.standard_normal((nl, D)).astype(np.float32), rng.standard_normal((nr, D)).astype(np.float32)) for nl, nr in graphs]
    grads = [(rng.standard_normal((nl, D)).astype(np.float32), rng.standard_normal((nr, D)).astype(np.float32)) for nl, nr in graphs]
    return per, grads


def _collate(dev, per, order):
    """(table_l, table_r, lig_batch, rec_batch) of the graphs ``order`` of ``per``, in that order"""
    l = np.concatenate([per[g][0] for g in order]).reshape(-1, D)
    r = np.concatenate([per[g][1] for g in order]).reshape(-1, D)
    lb = np.concatenate([np.full(len(per[g][0]), i) for i, g in enumerate(order)]).astype(np.int64)
    rb = np.concatenate([np.full(len(per[g][1]), i) for i, g in enumerate(order)]).astype(np.int64)
    return [torch.from_numpy(a).to(dev) for a in (l, r, lb, rb)]


def _split(t_l, t_r, graphs):
    out, al, ar = [], 0, 0
    for nl, nr in graphs:
        out.append(np.concatenate([t_l[al:al + nl], t_r[ar:ar + nr]]))      # [n, D]: the ligand's nodes first
        al, ar = al + nl, ar + nr
    return out


def _run(dev, per, grads, T, order=None):
    from disco_diffdock_amd.tensor_layers import ragged_gumbel_softmax
    order = list(range(len(per))) if order is None else order
    st = _streams()
    l, r, lb, rb = _collate(dev, per, order)
    gl, gr, _, _ = _collate(dev, grads, order)
    l.requires_grad_(), r.requires_grad_()
    out_l, out_r = ragged_gumbel_softmax(l, r, lb, rb, T, SEED, [st[g] for g in order], sample=SAMPLE, draw=DRAW)
    torch.autograd.backward([out_l, out_r], [gl, gr])
    graphs = [(len(per[g][0]), len(per[g][1])) for g in order]
    c = lambda t: t.detach().cpu().numpy()
    return _split(c(out_l), c(out_r), graphs), _split(c(l.grad), c(r.grad), graphs)


@pytest.mark.parametrize('T', [1.0, 0.01])
def test_against_fp64_and_the_mirror(dev, T):
    per, grads = _case()
    st = _streams()
    out, glogit = _run(dev, per, grads, T)
    for g, (nl, nr) in enumerate(GRAPHS):
        n = nl + nr
        logits, gout = np.concatenate(per[g]), np.concatenate(grads[g])
        assert out[g].shape == (n, D)
        for d in range(D):
            u = lref.gumbel_uniforms(SEED, st[g], SAMPLE, DRAW, d, n)
            want_out, y, k = lref.gumbel_forward(logits[:, d], u, T)
            z = logits[:, d].astype(np.float64) + lref.gumbel_noise(u)
            assert k == int(np.argmax(z)) and (n == 1 or np.sort(z)[-1] - np.sort(z)[-2] > 1e-4)      # the argmax of logit + gum, by a margin fp32 cannot flip
            hard = np.zeros(n)
            hard[k] = 1
            assert np.array_equal(np.round(out[g][:, d]), hard) and abs(out[g][k, d] - 1.0) < 2e-7      # one-hot at that argmax; (0 - y) + y is exactly 0
            out32, y32, _ = lref.gumbel_forward(logits[:, d], u, T, dtype=np.float32)
            want_g = lref.gumbel_backward(y, gout[:, d], T)
            g32 = lref.gumbel_backward(y32, gout[:, d], T, dtype=np.float32)
            # out differs from the one-hot by the rounding of (hard - y) + y alone: measured on the scale of 1
            for name, got, want, host in (('out', out[g][:, d], want_out, out32), ('grad_logit', glogit[g][:, d], want_g, g32)):
                err, err32 = rel_err(got, want), rel_err(host, want)
                bar = max(4 * err32, FLOOR)
                print(f'T{T}.graph{g}.d{d} {name}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
                _record_drift(f'gumbel.T{T}.graph{g}.d{d}.{name}', err, host_fp32=err32, bar=bar)
                assert err < bar, (T, g, d, name, err, bar)
            if n == 1:
                assert not glogit[g][:, d].any()      # one class: y = 1, the gradient is exactly 0


@pytest.mark.parametrize('T', [1.0, 0.01])
def test_a_graph_alone_and_inside_a_batch(dev, T):
    """a graph's rows are bit-identical alone and inside the batch at another position: the noise is keyed by the complex, the sums by the graph"""
    per, grads = _case()
    out, glogit = _run(dev, per, grads, T, order=[2, 0, 1])
    for g in range(len(GRAPHS)):
        alone_out, alone_g = _run(dev, per, grads, T, order=[g])
        at = [2, 0, 1].index(g)
        assert np.array_equal(alone_out[0].view(np.int32), out[at].view(np.int32)), g
        assert np.array_equal(alone_g[0].view(np.int32), glogit[at].view(np.int32)), g
    again = _run(dev, per, grads, T, order=[2, 0, 1])      # two calls: equal bits
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(out + glogit, again[0] + again[1]))


def test_guards_and_draws(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context, ragged_gumbel_softmax
    ctx = _shape_context(0)
    per, _ = _case()
    l, r, lb, rb = _collate(dev, per, [0, 1, 2])
    st = _streams()
    base = ragged_gumbel_softmax(l, r, lb, rb, 1.0, SEED, st)
    assert not base[0].requires_grad and base[0].shape == l.shape and base[1].shape == r.shape
    for d in range(D):      # per graph and dimension exactly one node is chosen, on either side
        picks = torch.zeros(3, device=dev).index_add_(0, lb, base[0][:, d].round()) + torch.zeros(3, device=dev).index_add_(0, rb, base[1][:, d].round())
        assert picks.tolist() == [1.0, 1.0, 1.0]
    assert any(not torch.equal(_bits(a), _bits(b)) for kw in (dict(draw=1), dict(sample=1)) for a, b in zip(ragged_gumbel_softmax(l, r, lb, rb, 1.0, SEED, st, **kw), base))
    ptr = lambda b: torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(b, minlength=3), 0)])
    with pytest.raises(RuntimeError, match='D in 1..4'):
        ctx.gumbel_softmax(torch.zeros(12, 5, device=dev), torch.zeros(8, 5, device=dev), ptr(lb), ptr(rb), 1.0, 1, st)
    with pytest.raises(RuntimeError, match='temperature'):
        ctx.gumbel_softmax(l, r, ptr(lb), ptr(rb), 0.0, 1, st)
    with pytest.raises(RuntimeError, match='draw'):
        ctx.gumbel_softmax(l, r, ptr(lb), ptr(rb), 1.0, 1, st, draw=1 << 20)
    with pytest.raises(RuntimeError, match='sorted by graph'):
        ragged_gumbel_softmax(l, r, lb.flip(0), rb, 1.0, SEED, st)
    with pytest.raises(RuntimeError, match='GPU only'):
        ragged_gumbel_softmax(l.cpu(), r.cpu(), lb.cpu(), rb.cpu(), 1.0, SEED, st)
    # a pointer pair that is no range of its table leaves the graph unwritten and touches nothing else
    broken = ptr(lb).clone()
    broken[3] = l.shape[0] + 5
    out_l, out_r, _, _ = ctx.gumbel_softmax(l, r, broken, ptr(rb), 1.0, SEED, st)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_l[:6]), _bits(base[0][:6])) and torch.equal(_bits(out_r[:7]), _bits(base[1][:7]))
