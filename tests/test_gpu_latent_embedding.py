"""GPU tests of the edge embedding with latent columns (ddk_eemb_latent_forward / ddk_eemb_latent_backward, csrc/k_eemb.hip) through the C ABI,
Context.eemb_latent_forward / eemb_latent_backward and tensor_layers.fused_edge_embedding(latent_a=..., latent_b=...).

Reference: the fp64 restatement tests/latent_embedding_ref.py, its mask from tests/philox_ref.py.  The bar of an output is MEASURED: the same expressions
evaluated in fp32 on the host against fp64 give err32; the device passes under 4 * err32, floored at 1e-5.  Both are fp32 evaluations that differ only in
summation order between lanes and slices; 4 is the allowance for that.

The ReLU kink is handled as in tests/test_gpu_edge_embedding.py: the hidden layer never leaves the device, an element whose pre-activation lies within
fp32 rounding of zero may take either branch, at most AMBIGUOUS_CAP of them per case (asserted first), and the gradients must meet the bar for ONE
assignment of those few branches.  The host's fp32 evaluation is given the same branches, so err32 measures rounding alone."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import edge_embedding_ref as ref
import latent_embedding_ref as lref
from helpers import rel_err
from test_gpu_edge_embedding import _operands as _plain_operands
from test_gpu_radial_conv import _bits
from test_gpu_radial_tp import SENTINEL, _guarded, _to
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
FLOOR = 1e-5
AMBIGUOUS_CAP = 3
NAMES = lref.NAMES


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


def _params(K, seed):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(w1=f(24, K) / np.float32(np.sqrt(K)), b1=f(24) * np.float32(0.5), w2=f(24, 24) / np.float32(np.sqrt(24.0)), b2=f(24), uemb=f(24))


def _operands(E, F, L, seed, n_a=7, n_b=11, unc=True):
    """the plain op's operands (tables of 7 and 11 rows, the indices repeat) with DIFFERENT latent tables of different lengths on the two sides and an
    unconditional value per node of pos_a that is not just 0 / 1"""
    o, g = _plain_operands(E, F + 64, seed, n_a=n_a, n_b=n_b)
    rng = np.random.default_rng(seed + 17)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    o.update(lat_a=f(n_a, L), lat_b=f(n_b, L), unc_a=((rng.random(n_a) < 0.4) + np.float32(0.25) * f(n_a)).astype(np.float32) if unc else None)
    return o, g


def _dev_ops(dev, o):
    return [_to(dev, o[k]) for k in ('pos_a', 'pos_b', 'idx_a', 'idx_b', 'feat', 'sig', 'sig_index')] + [o['start'], o['stop']]


def _graph(dev, o):
    from disco_diffdock_amd.runtime import Context
    return Context.conv_graph(_to(dev, o['idx_a']), _to(dev, o['idx_b']), len(o['pos_b']), len(o['pos_a']))


def _device(ctx, dev, o, P, g, p=0.0, seed=0, need=(True,) * 7):
    ops, t = _dev_ops(dev, o), {k: _to(dev, v) for k, v in P.items()}
    zero = bool(o.get('zero_latent'))
    la, lb = (None, None) if zero else (_to(dev, o['lat_a']), _to(dev, o['lat_b']))
    unc, uemb = (None, None) if o.get('unc_a') is None else (_to(dev, o['unc_a']), t['uemb'])
    emb, sh = ctx.eemb_latent_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], la, lb, zero, unc, uemb, p, seed)
    graph = _graph(dev, o) if len(o['idx_a']) else None
    grads = ctx.eemb_latent_backward(*ops, t['w1'], t['b1'], t['w2'], la, lb, _to(dev, g), zero, unc, uemb, p, seed, graph, need)
    return emb.cpu().numpy(), sh.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _check(ctx, dev, tag, o, P, g, L, p=0.0, mask_seed=0):
    pre, margin = lref.pre_activation(o, P['w1'], P['b1'], L)
    amb = np.argwhere(np.abs(pre) < margin)
    print(tag, f'{len(amb)} of {pre.size} elements under the fp32 margin (cap {AMBIGUOUS_CAP})')
    assert len(amb) <= AMBIGUOUS_CAP, (tag, len(amb))
    passes = pre > 0
    E = len(o['idx_a'])
    keep, s = ref.keep_mask(mask_seed, E, p), ref.scale(p)
    emb, sh, grads = _device(ctx, dev, o, P, g, p, mask_seed)
    want_emb = lref.forward(o, P, L, keep, s)
    err32 = {'emb': rel_err(lref.forward(o, P, L, keep, s, dtype=np.float32), want_emb)}
    vec, d = ref.geometry(o['pos_a'], o['pos_b'], o['idx_a'], o['idx_b'])
    assert emb.shape == want_emb.shape and sh.shape == (E, 4)
    assert np.isfinite(emb).all() and np.isfinite(sh).all() and all(np.isfinite(a).all() for a in grads)
    assert rel_err(sh, ref.spherical_harmonics(vec, d)) < FLOOR
    best = None
    for choice in itertools.product((False, True), repeat=len(amb)):      # (one pass when nothing is ambiguous)
        for (e, c), v in zip(amb, choice):
            passes[e, c] = v
        want = lref.backward(o, P, L, g, keep, s, passes)
        host = lref.backward(o, P, L, g, keep, s, passes, dtype=np.float32)
        assert [a.shape for a in grads] == [want[n].shape for n in NAMES]
        errs = {n: rel_err(a, want[n]) if want[n].any() else float(np.abs(a).max()) for n, a in zip(NAMES, grads)}
        e32 = {n: rel_err(host[n], want[n]) if want[n].any() else 0.0 for n in NAMES}
        over = max(errs[n] / max(4 * e32[n], FLOOR) for n in NAMES)
        if best is None or over < best[0]:
            best = (over, errs, e32)
    _, errs, e32 = best
    errs['emb'] = rel_err(emb, want_emb)
    err32.update(e32)
    failures = []
    for n, v in errs.items():
        bar = max(4 * err32[n], FLOOR)
        print(f'{tag} {n}: device {v:.2e}, host fp32 {err32[n]:.2e}, bar {bar:.2e}')
        _record_drift(f'latent_embedding.{tag}.{n}', v, host_fp32=err32[n], bar=bar)
        if not v < bar:
            failures.append((n, v, err32[n], bar))
    assert not failures, (tag, failures)
    return emb, sh, grads


# ---- 1. forward and the seven gradients: wave boundaries (64) and the slice boundaries of rtp_slice_len (512); different tables on the two sides ------------
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('L', [1, 2, 4])
@pytest.mark.parametrize('F', [0, 4])
@pytest.mark.parametrize('E', [1, 63, 64, 65, 129, 511, 512, 513, 1025])
def test_against_closed_form(ctx, dev, E, F, L, p):
    o, g = _operands(E, F, L, 1000 * E + 10 * F + L)
    assert o['lat_a'].shape[0] != o['lat_b'].shape[0]
    # (the weights' seed: with 7 E + F + L + 400 no case has more than 2 elements under the fp32 margin, counted on the host; the offsets 0 and 100 gave
    # cases with 6 and 8, over the cap, which is a property of the input alone)
    _check(ctx, dev, f'E{E}.F{F}.L{L}.p{p}', o, _params(F + 64 + 2 * L, 7 * E + F + L + 400), g, L, p, mask_seed=0xC0FFEE0000 + E)


# ---- 2. zero_latent: the cross group --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [1, 2, 4])
def test_zero_latent(ctx, dev, L):
    E, F = 700, 0
    o, g = _operands(E, F, L, 31 + L)
    o['zero_latent'] = True
    P = _params(F + 64 + 2 * L, 32)
    emb, _, grads = _check(ctx, dev, f'zero_latent.L{L}', o, P, g, L, p=0.1, mask_seed=5)
    by = dict(zip(NAMES, grads))
    assert not by['grad_w1'][:, F + 64:].any() and by['grad_w1'][:, :F + 64].any()      # exact zeros in the latent columns
    assert by['grad_lat_a'].shape == (7, L) and by['grad_lat_b'].shape == (11, L) and not by['grad_lat_a'].any() and not by['grad_lat_b'].any()
    # the tables are not read: the same bits with tables of NaN handed to the op through the autograd wrapper's flag
    ops, t = _dev_ops(dev, o), {k: _to(dev, v) for k, v in P.items()}
    again, _ = ctx.eemb_latent_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], torch.full((7, L), float('nan'), device=dev),
                                       torch.full((11, L), float('nan'), device=dev), True, _to(dev, o['unc_a']), t['uemb'], 0.1, 5)
    assert np.array_equal(again.cpu().numpy().view(np.int32), emb.view(np.int32))


# ---- 3. all-zero latents, no unconditional term: the plain op's bits whatever W1's latent columns hold ------------------------------------------------------
@pytest.mark.parametrize('F,L', [(0, 1), (4, 2), (0, 4)])
def test_zero_latents_give_the_plain_bits(ctx, dev, F, L):
    """fmaf(w, 0, acc) == acc for every finite w: the chain over the 2 L new columns leaves the pre-activation's bits alone"""
    E, K, p, seed = 1300, F + 64, 0.1, 77
    o, g = _operands(E, F, L, 55, unc=False)
    o['lat_a'][:], o['lat_b'][:] = 0, 0
    P = _params(K + 2 * L, 56)
    P['w1'][:, K:] = (np.random.default_rng(1).standard_normal((24, 2 * L)) * 1e6).astype(np.float32)      # arbitrary finite values
    ops, t = _dev_ops(dev, o), {k: _to(dev, v) for k, v in P.items()}
    plain_w1 = t['w1'][:, :K].contiguous()
    want_emb, want_sh = ctx.eemb_forward(*ops, plain_w1, t['b1'], t['w2'], t['b2'], p, seed)
    for zero in (False, True):
        la, lb = (None, None) if zero else (_to(dev, o['lat_a']), _to(dev, o['lat_b']))
        emb, sh = ctx.eemb_latent_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], la, lb, zero, None, None, p, seed)
        assert torch.equal(_bits(emb), _bits(want_emb)) and torch.equal(_bits(sh), _bits(want_sh)), zero
    # and the parameter gradients the two ops share are the same images added in the same order
    gd = _to(dev, g)
    want = ctx.eemb_backward(*ops, plain_w1, t['b1'], t['w2'], gd, p, seed)
    got = ctx.eemb_latent_backward(*ops, t['w1'], t['b1'], t['w2'], None, None, gd, True, None, None, p, seed, None, (True,) * 5 + (False,) * 2)
    assert torch.equal(_bits(got[0][:, :K]), _bits(want[0])) and not bool(got[0][:, K:].any()) and not bool(got[4].any())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[1:4], want[1:]))


# ---- 4. one node owns every edge, and nodes without edges ------------------------------------------------------------------------------------------------------
def test_one_node_owns_all_edges(ctx, dev):
    E, F, L = 1025, 4, 2
    o, g = _operands(E, F, L, 91)
    o['idx_a'][:] = 3                       # node 3 of pos_a owns all 1025 edges (three slices); the six others own none
    o['idx_b'][o['idx_b'] == 5] = 6         # node 5 of pos_b owns none
    _, _, grads = _check(ctx, dev, 'one_node', o, _params(F + 64 + 2 * L, 92), g, L, p=0.1, mask_seed=9)
    by = dict(zip(NAMES, grads))
    others = np.arange(7) != 3
    assert by['grad_lat_a'][3].all() and not by['grad_lat_a'][others].any()      # exact zeros where a node has no edge
    assert not by['grad_lat_b'][5].any() and by['grad_lat_b'][6].all()


# ---- 5. identical bits, output subsets, guards (the C entries themselves) -----------------------------------------------------------------------------------
def test_guards_bits_and_subsets(ctx, dev):
    E, F, L, p, seed = 1300, 4, 2, 0.1, 0xFEDCBA9876543210      # three slices of 512 edges
    K = F + 64 + 2 * L
    o, g = _operands(E, F, L, 42)
    ops = _dev_ops(dev, o)
    P = {k: _to(dev, v) for k, v in _params(K, 43).items()}
    gd, la, lb, unc = _to(dev, g), _to(dev, o['lat_a']), _to(dev, o['lat_b']), _to(dev, o['unc_a'])
    graph = _graph(dev, o)
    tensors = [t for t in ops if torch.is_tensor(t)] + list(P.values()) + [gd, la, lb, unc]
    before = [t.clone() for t in tensors]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: ctx.L.ddk_last_error(ctx.h)

    def common(L_=L, lat_a=la, lat_b=lb, zero=0, unc_=unc, uemb=P['uemb']):
        return [ctx.h, ptr(ops[0]), 7, ptr(ops[1]), 11, ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), 4, ptr(ops[5]), 3, ptr(ops[6]), 0.0, 5.0, 32,
                ptr(P['w1']), ptr(P['b1']), ptr(P['w2']), ptr(P['b2']), p, seed, ptr(lat_a) if torch.is_tensor(lat_a) else lat_a,
                ptr(lat_b) if torch.is_tensor(lat_b) else lat_b, L_, zero, ptr(unc_), ptr(uemb)]

    def check_guards(bufs):
        torch.cuda.synchronize()
        for full, _ in bufs:
            if full is not None:      # the guard rows in front and behind still hold the sentinel
                assert bool((full[0] == SENTINEL).all()) and bool((full[-1] == SENTINEL).all())

    def fwd():
        bufs = [_guarded(E, 24, dev), _guarded(E, 4, dev)]
        assert ctx.L.ddk_eemb_latent_forward(*common(), E, ptr(bufs[0][1]), ptr(bufs[1][1]), stream()) == 0, err()
        check_guards(bufs)
        return [v.clone() for _, v in bufs]

    first, again = fwd(), fwd()
    assert all(bool((t != SENTINEL).all()) for t in first)      # every element was written
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    emb, sh = ctx.eemb_latent_forward(*ops, P['w1'], P['b1'], P['w2'], P['b2'], la, lb, False, unc, P['uemb'], p, seed)
    assert torch.equal(_bits(emb), _bits(first[0])) and torch.equal(_bits(sh), _bits(first[1]))

    ws = torch.empty(ctx.L.ddk_eemb_latent_workspace(E, K, L) // 4, device=dev)
    shapes = ((24, K), (1, 24), (24, 24), (1, 24), (1, 24), (7, L), (11, L))
    tables = [ptr(graph.src_order), ptr(graph.src_ptr), ptr(graph.dst_order), ptr(graph.dst_ptr)]

    def raw(need, **kw):
        bufs = [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        return ctx.L.ddk_eemb_latent_backward(*common(**kw), *tables, ptr(gd), E, *[ptr(v) for _, v in bufs], ptr(ws), stream()), bufs

    def bwd(need):
        rc, bufs = raw(need)
        assert rc == 0, err()
        check_guards(bufs)
        return [None if v is None else v.clone() for _, v in bufs]

    full = bwd((True,) * 7)
    assert all(bool((t != SENTINEL).all()) for t in full)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, bwd((True,) * 7)))      # two full calls: the same bits
    subsets = [need for need in itertools.product((False, True), repeat=7) if any(need)]
    assert len(subsets) == 127
    for need in subsets:
        part = bwd(need)
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(_bits(a), _bits(b)), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(a, b) for a, b in zip(tensors, before))      # the operands are untouched
    via = ctx.eemb_latent_backward(*ops, P['w1'], P['b1'], P['w2'], la, lb, gd, False, unc, P['uemb'], p, seed, graph)
    assert all(torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1))) for a, b in zip(via, full))
    # what is refused, with text
    assert raw((False,) * 7)[0] == -1 and b'no gradient' in err()
    for bad in (0, 5):
        assert raw((True,) * 7, L_=bad)[0] == -1 and b'1..4' in err()
    odd = torch.zeros(7 * L + 1, device=dev)[1:]      # a table 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4
    assert raw((True,) * 7, lat_a=odd)[0] == -1 and b'16-byte aligned' in err()
    assert raw((True,) * 7, lat_b=None)[0] == -1 and b'null latent table' in err()
    assert raw((True,) * 7, uemb=None)[0] == -1 and b'unc_a without uemb' in err()
    assert ctx.L.ddk_eemb_latent_forward(*common(L_=7), E, ptr(first[0]), ptr(first[1]), stream()) == -1 and b'1..4' in err()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='at least one'):
        ctx.eemb_latent_backward(*ops, P['w1'], P['b1'], P['w2'], la, lb, gd, False, unc, P['uemb'], p, seed, graph, need=(False,) * 7)
    with pytest.raises(RuntimeError, match=r'w1 \[24, 68 \+ 2 L\]'):      # K mismatch
        ctx.eemb_latent_forward(*ops, P['w1'][:, :K - 1].contiguous(), P['b1'], P['w2'], P['b2'], la, lb)
    with pytest.raises(RuntimeError, match='lat_a'):
        ctx.eemb_latent_forward(*ops, P['w1'], P['b1'], P['w2'], P['b2'], la[:, :1].contiguous(), lb)
    with pytest.raises(RuntimeError, match='conv_graph'):
        ctx.eemb_latent_backward(*ops, P['w1'], P['b1'], P['w2'], la, lb, gd, False, unc, P['uemb'], p, seed, None)


# ---- 6. no edges ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_no_edges(ctx, dev):
    for F, L in ((0, 1), (4, 4)):
        o, g = _operands(0, F, L, 1)
        emb, sh, grads = _device(ctx, dev, o, _params(F + 64 + 2 * L, 2), g, p=0.1, seed=5)
        assert emb.shape == (0, 24) and sh.shape == (0, 4)
        assert [a.shape for a in grads] == [(24, F + 64 + 2 * L), (24,), (24, 24), (24,), (24,), (7, L), (11, L)] and not any(a.any() for a in grads)
    # the C entries themselves write the zeros, with no operands and no workspace
    full = lambda *shape: torch.full(shape, 7.0, device=dev)
    outs = [full(24, 72), full(24), full(24, 24), full(24), full(24), full(7, 2), full(11, 2)]
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = [None, 7, None, 11, None, None, None, 4, None, 0, None, 0.0, 5.0, 32, None, None, None, None, 0.1, 5, None, None, 2, 0, None, None]
    assert ctx.L.ddk_eemb_latent_forward(ctx.h, *none, 0, None, None, stream) == 0, ctx.L.ddk_last_error(ctx.h)
    assert ctx.L.ddk_eemb_latent_backward(ctx.h, *none, None, None, None, None, None, 0, *[p(t) for t in outs], None, stream) == 0, ctx.L.ddk_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in outs)


# ---- 7. the autograd op: one table on both sides, the unconditional row, and the plain call path ------------------------------------------------------------
def test_fused_edge_embedding_with_latents(ctx, dev):
    from disco_diffdock_amd.tensor_layers import GaussianSmearing, fused_edge_embedding
    E, F, L = 300, 4, 2
    K = F + 64 + 2 * L
    o, g = _operands(E, F, L, 90, n_a=9, n_b=9)
    torch.manual_seed(3)
    mlp = torch.nn.Sequential(torch.nn.Linear(K, 24), torch.nn.ReLU(), torch.nn.Dropout(0.1), torch.nn.Linear(24, 24)).to(dev)
    uemb = torch.nn.Parameter(torch.randn(1, 24, device=dev))
    expansion = GaussianSmearing(0.0, 5.0, 32).to(dev)
    pos, _, ia, ib, feat, sig, sig_index = _dev_ops(dev, o)[:7]
    edge_index = torch.stack([ia, ib]).long()
    lat = _to(dev, o['lat_a']).requires_grad_()
    unc = _to(dev, o['unc_a'])
    gd = _to(dev, g)
    params = list(mlp.parameters()) + [uemb, lat]

    def step(seed=11):
        for q in params:
            q.grad = None
        emb, sh = fused_edge_embedding(mlp, expansion, pos, pos, edge_index, sig, sig_index, feat=feat, seed=seed, latent_a=lat, latent_b=lat,
                                       unconditional=unc, unconditional_embedding=uemb)
        assert not sh.requires_grad and emb.requires_grad
        emb.backward(gd)
        return emb.detach(), [q.grad.clone() for q in params]

    mlp.train()
    emb, grads = step()
    P = [mlp[0].weight.detach(), mlp[0].bias.detach(), mlp[3].weight.detach(), mlp[3].bias.detach()]
    ops = (pos, pos, ia, ib, feat, sig, sig_index, 0.0, 5.0)
    want = ctx.eemb_latent_forward(*ops, *P, lat.detach(), lat.detach(), False, unc, uemb.detach(), 0.1, 11)
    assert torch.equal(_bits(emb), _bits(want[0]))
    from disco_diffdock_amd.runtime import Context
    raw = ctx.eemb_latent_backward(*ops, *P[:3], lat.detach(), lat.detach(), gd, False, unc, uemb.detach(), 0.1, 11, Context.conv_graph(ia, ib, 9, 9))
    assert all(torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1))) for a, b in zip(grads[:5], raw[:5]))
    assert torch.equal(_bits(grads[5]), _bits(raw[5] + raw[6]))      # one table: the source sum + the destination sum
    again = step()
    assert torch.equal(_bits(again[0]), _bits(emb)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[1], grads))      # one seed: the same bits
    # evaluation: no dropout, and the plain composition in fp32 on the device (index_select, cat, Sequential, the unconditional add) agrees to fp32 accuracy
    mlp.eval()
    ev, gev = step()
    for q in params:
        q.grad = None
    with torch.no_grad():
        vec = pos[ib.long()] - pos[ia.long()]
        head = torch.cat([feat, sig[sig_index.long()[ia.long()]], expansion(vec.norm(dim=-1))], 1)
    plain = mlp(torch.cat([head, lat[ia.long()], lat[ib.long()]], 1)) + unc[ia.long()][:, None] * uemb
    plain.backward(gd)
    assert rel_err(ev.cpu().numpy(), plain.detach().cpu().numpy()) < 1e-5
    for a, q in zip(gev, params):
        assert rel_err(a.cpu().numpy(), q.grad.cpu().numpy()) < 1e-4
    # nothing per edge is saved but what the caller handed in (and the node-sorted lists of the indices)
    mlp.train()
    out, _ = fused_edge_embedding(mlp, expansion, pos, pos, edge_index, sig, sig_index, feat=feat, seed=1, latent_a=lat, latent_b=lat)
    given = {t.data_ptr() for t in (pos, ia, ib, feat, sig, sig_index, lat, *[q for q in mlp.parameters()])}
    assert all(t.data_ptr() in given or (t.dtype == torch.int32 and t.dim() == 1) for t in out.grad_fn.saved_tensors if t is not None)
    # what is refused, and the plain call path
    with pytest.raises(RuntimeError, match='unconditional'):
        fused_edge_embedding(mlp, expansion, pos, pos, edge_index, sig, sig_index, feat=feat, latent_a=lat, latent_b=lat, unconditional=unc.clone().requires_grad_(),
                             unconditional_embedding=uemb)
    with pytest.raises(RuntimeError, match='the row has 68'):
        fused_edge_embedding(mlp, expansion, pos, pos, edge_index, sig, sig_index, feat=feat)
    with pytest.raises(RuntimeError, match='the row has 76'):
        fused_edge_embedding(mlp, expansion, pos, pos, edge_index, sig, sig_index, feat=feat, latent_a=torch.zeros(9, 4, device=dev), latent_b=torch.zeros(9, 4, device=dev))
    small = torch.nn.Sequential(torch.nn.Linear(68, 24), torch.nn.ReLU(), torch.nn.Dropout(0.1), torch.nn.Linear(24, 24)).to(dev).train()
    a, _ = fused_edge_embedding(small, expansion, pos, pos, edge_index, sig, sig_index, feat=feat, seed=4)
    b, _ = ctx.eemb_forward(*ops, small[0].weight.detach(), small[0].bias.detach(), small[3].weight.detach(), small[3].bias.detach(), 0.1, 4)
    assert torch.equal(_bits(a.detach()), _bits(b)) and type(a.grad_fn).__name__.startswith('_EdgeEmbeddingFunction')
