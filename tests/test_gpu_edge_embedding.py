"""GPU tests of the edge embedding in front of the conv stack (ddk_eemb_forward / ddk_eemb_backward, csrc/k_eemb.hip) through the C ABI,
Context.eemb_forward / eemb_backward and tensor_layers.fused_edge_embedding.

Reference: the fp64 restatement tests/edge_embedding_ref.py, its mask from tests/philox_ref.py.  Bar: helpers.rel_err < 1e-5 per output (emb, sh) and per
parameter tensor (grad_w1, grad_b1, grad_w2, grad_b2), the bar of the sibling op tests.  Every device number is an fp32 fmaf chain of at most 68 terms over
columns that are exact (bond types, the sigma table) or an expf of an edge length, or a fixed-order fp32 sum over at most 1025 edges: far inside the bar.

The ReLU kink: the hidden layer is recomputed inside the backward and never leaves the device, so the fp64 reference differentiates through its OWN
zero pattern.  That is the device's pattern wherever |pre| clears what an fp32 evaluation can be off by (edge_embedding_ref.pre_activation's margin).
An element under that margin may take either branch on the device: at most AMBIGUOUS_CAP of them are allowed per case (asserted first), and the
gradients must meet the bar for ONE assignment of those few branches; every other element is held to the fp64 pattern."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import adversarial_edges as adv
import edge_embedding_ref as ref
from helpers import rel_err
from test_gpu_radial_conv import _bits
from test_gpu_radial_tp import SENTINEL, _guarded, _to
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
BAR = 1e-5
AMBIGUOUS_CAP = 3      # elements of a case whose ReLU branch fp32 rounding may decide (the gradients are tried with either branch)
NAMES = ('grad_w1', 'grad_b1', 'grad_w2', 'grad_b2')
TABLES = {68: (0.0, 5.0), 64: (0.0, 30.0)}      # the ligand group's expansion with bond features; the receptor's without


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
    return dict(w1=f(24, K) / np.float32(np.sqrt(K)), b1=f(24) * np.float32(0.5), w2=f(24, 24) / np.float32(np.sqrt(24.0)), b2=f(24))


def _operands(E, K, seed, n_a=7, n_b=11, T=3):
    """coordinate tables of 7 and 11 rows (the indices repeat), lengths over the whole expansion and beyond it, one-hot bond types for K = 68"""
    rng = np.random.default_rng(seed)
    start, stop = TABLES[K]
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    o = dict(pos_a=f(n_a, 3) * np.float32(stop / 4), pos_b=f(n_b, 3) * np.float32(stop / 4), idx_a=rng.integers(0, n_a, E).astype(np.int32),
             idx_b=rng.integers(0, n_b, E).astype(np.int32), feat=None, sig=f(T, 32), sig_index=rng.integers(0, T, n_a).astype(np.int32), start=start, stop=stop)
    if K == 68:
        o['feat'] = np.eye(4, dtype=np.float32)[rng.integers(0, 4, E)] * (rng.random(E) < 0.7)[:, None].astype(np.float32)      # (radius copies carry zeros)
    return o, f(E, 24)


def _dev_operands(dev, o):
    return [_to(dev, o[k]) for k in ('pos_a', 'pos_b', 'idx_a', 'idx_b', 'feat', 'sig', 'sig_index')] + [o['start'], o['stop']]


def _device(ctx, dev, o, P, g, p=0.0, seed=0, need=(True,) * 4):
    ops, t = _dev_operands(dev, o), {k: _to(dev, v) for k, v in P.items()}
    emb, sh = ctx.eemb_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], p, seed)
    grads = ctx.eemb_backward(*ops, t['w1'], t['b1'], t['w2'], _to(dev, g), p, seed, need)
    return emb.cpu().numpy(), sh.cpu().numpy(), [None if a is None else a.cpu().numpy() for a in grads]


def _ambiguous(tag, o, P):
    """the (edge, column) elements whose pre-activation lies within fp32 rounding of zero, and the fp64 pattern"""
    pre, margin = ref.pre_activation(o, P['w1'], P['b1'])
    amb = np.argwhere(np.abs(pre) < margin)
    print(tag, f'{len(amb)} of {pre.size} elements under the fp32 margin (cap {AMBIGUOUS_CAP})')
    assert len(amb) <= AMBIGUOUS_CAP, (tag, len(amb))
    return amb, pre > 0


def _check(ctx, dev, tag, o, P, g, p=0.0, mask_seed=0):
    amb, passes = _ambiguous(tag, o, P)
    E = len(o['idx_a'])
    keep, s = ref.keep_mask(mask_seed, E, p), ref.scale(p)
    emb, sh, grads = _device(ctx, dev, o, P, g, p, mask_seed)
    want_emb, want_sh, _ = ref.forward(o, P['w1'], P['b1'], P['w2'], P['b2'], keep, s)
    assert emb.shape == want_emb.shape and sh.shape == want_sh.shape
    assert np.isfinite(emb).all() and np.isfinite(sh).all() and all(np.isfinite(a).all() for a in grads)
    errs = None
    for choice in itertools.product((False, True), repeat=len(amb)):      # (one pass when nothing is ambiguous)
        for (e, c), v in zip(amb, choice):
            passes[e, c] = v
        want = ref.backward(o, P['w1'], P['b1'], P['w2'], g, keep, s, passes)
        assert [a.shape for a in grads] == [a.shape for a in want]
        these = {name: rel_err(a, b) for name, a, b in zip(NAMES, grads, want)}
        if errs is None or max(these.values()) < max(errs.values()):
            errs = these
    errs.update({'emb': rel_err(emb, want_emb), 'sh': rel_err(sh, want_sh)})
    print(tag, {k: f'{v:.2e}' for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    _record_drift(f'edge_embedding.{tag}', errs[worst], worst_block=worst, bar=BAR)
    assert errs[worst] < BAR, (tag, worst, errs[worst])
    return emb, sh, grads


# ---- 1. forward and the four gradients: wave boundaries (64) and the slice boundaries of rtp_slice_len (512) ------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('K', [64, 68])
@pytest.mark.parametrize('E', [1, 63, 64, 65, 129, 511, 512, 513, 1025])
def test_against_closed_form(ctx, dev, E, K, p):
    o, g = _operands(E, K, 1000 * E + K)
    _check(ctx, dev, f'E{E}.K{K}.p{p}', o, _params(K, 7 * E + K), g, p, mask_seed=0xC0FFEE0000 + E)


# ---- 2. adversarial geometry (the generators of tests/adversarial_edges.py) -----------------------------------------------------------------------------
def _all_pairs(n_a, n_b, same):
    ia, ib = np.meshgrid(np.arange(n_a), np.arange(n_b), indexing='ij')
    on = (ia != ib) if same else np.ones_like(ia, bool)
    return ia[on].astype(np.int32), ib[on].astype(np.int32)


def _geometry_case(name):
    rng = np.random.default_rng(5)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    if name == 'coincident':      # atoms 1 and 2 ON atom 0, atom 3 one ulp from atom 4: zero-length ligand edges, and every pair beyond the 5 A table
        cs = adv.case('coincident')
        pos = np.concatenate([cs.pos[0], np.array([[0, 0, 0], [3, 4, 0]], np.float32) + np.round(cs.pos[0][7])])      # + a pair on whole coordinates exactly 5 A apart: AT stop
        ia, ib = _all_pairs(len(pos), len(pos), True)
        o = dict(pos_a=pos, pos_b=pos, idx_a=ia, idx_b=ib, start=0.0, stop=5.0)
    elif name == 'binades':       # sample 2: the atoms on a ray from residue 0, 0.05 .. 77 A from it, and residues out to 100 A: across and beyond the 30 A table
        cs = adv.case('binades')
        ia, ib = _all_pairs(len(cs.pos[2]), len(cs.c['rec_pos']), False)
        o = dict(pos_a=cs.pos[2], pos_b=cs.c['rec_pos'], idx_a=ia, idx_b=ib, start=0.0, stop=30.0)
    else:                         # coordinates of magnitude 1e3: the shifted complex moved further out
        cs = adv.case('far_shift')
        shift = np.array([850.0, -920.0, 940.0])
        pa, pb = (cs.pos[1].astype(np.float64) + shift).astype(np.float32), (cs.c['rec_pos'].astype(np.float64) + shift).astype(np.float32)
        assert np.abs(pa).max() > 900 and np.abs(pb).max() > 900
        ia, ib = _all_pairs(len(pa), len(pb), False)
        o = dict(pos_a=pa, pos_b=pb, idx_a=ia, idx_b=ib, start=0.0, stop=30.0)
    E, n_a = len(o['idx_a']), len(o['pos_a'])
    same = name == 'coincident'
    o.update(feat=np.eye(4, dtype=np.float32)[rng.integers(0, 4, E)] if same else None, sig=f(2, 32), sig_index=rng.integers(0, 2, n_a).astype(np.int32))
    return o, _params(68 if same else 64, 11), f(E, 24)


@pytest.mark.parametrize('name', ['coincident', 'binades', 'far_1e3'])
def test_adversarial_geometry(ctx, dev, name):
    o, P, g = _geometry_case(name)
    _, d = ref.geometry(o['pos_a'], o['pos_b'], o['idx_a'], o['idx_b'])
    if name == 'coincident':
        assert (d == 0).sum() >= 6 and (d == 5.0).sum() >= 2 and (d > 5.0).any() and ((d > 0) & (d < 1e-5)).any()      # zero length, one ulp, AT stop, beyond
    if name == 'binades':
        assert d.min() < 0.1 and d.max() > 90 and (d > 30.0).mean() > 0.2
    emb, sh, _ = _check(ctx, dev, f'geometry.{name}', o, P, g, p=0.1, mask_seed=99)
    if name == 'coincident':
        assert np.array_equal(sh[d == 0], np.tile(np.array([1, 0, 0, 0], np.float32), (int((d == 0).sum()), 1)))      # a zero-length edge: finite, [1, 0, 0, 0]
    assert np.allclose(np.linalg.norm(sh[d > 0][:, 1:], axis=1), np.sqrt(3.0), rtol=1e-5)


# ---- 3. guard rows, identical bits, output subsets (the C entries themselves) -------------------------------------------------------------------------------
def test_guards_bits_and_subsets(ctx, dev):
    E, K, p, seed = 1300, 68, 0.1, 0xFEDCBA9876543210      # three slices of 512 edges
    o, g = _operands(E, K, 42)
    ops = [t for t in _dev_operands(dev, o)]
    P = {k: _to(dev, v) for k, v in _params(K, 43).items()}
    gd = _to(dev, g)
    tensors = [t for t in ops if torch.is_tensor(t)] + list(P.values()) + [gd]
    before = [t.clone() for t in tensors]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = lambda: [ctx.h, ptr(ops[0]), 7, ptr(ops[1]), 11, ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), 4, ptr(ops[5]), 3, ptr(ops[6]), 0.0, 5.0, 32,
                      ptr(P['w1']), ptr(P['b1']), ptr(P['w2']), ptr(P['b2']), p, seed]
    err = lambda: ctx.L.ddk_last_error(ctx.h)

    def check_guards(bufs):
        torch.cuda.synchronize()
        for full, _ in bufs:
            if full is not None:      # the guard rows in front and behind still hold the sentinel
                assert bool((full[0] == SENTINEL).all()) and bool((full[-1] == SENTINEL).all())

    def fwd():
        bufs = [_guarded(E, 24, dev), _guarded(E, 4, dev)]
        assert ctx.L.ddk_eemb_forward(*common(), E, ptr(bufs[0][1]), ptr(bufs[1][1]), stream()) == 0, err()
        check_guards(bufs)
        return [v.clone() for _, v in bufs]

    first, again = fwd(), fwd()
    assert all(bool((t != SENTINEL).all()) for t in first)      # every element was written
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    emb, sh = ctx.eemb_forward(*ops, P['w1'], P['b1'], P['w2'], P['b2'], p, seed)
    assert torch.equal(_bits(emb), _bits(first[0])) and torch.equal(_bits(sh), _bits(first[1]))

    ws = torch.empty(ctx.L.ddk_eemb_workspace(E, K) // 4, device=dev)
    shapes = ((24, K), (1, 24), (24, 24), (1, 24))

    def raw(need, b2=True):
        bufs = [_guarded(r, c, dev) if on else (None, None) for on, (r, c) in zip(need, shapes)]
        args = common()
        if not b2:
            args[18] = None      # (the backward does not read b2)
        return ctx.L.ddk_eemb_backward(*args, ptr(gd), E, *[ptr(v) for _, v in bufs], ptr(ws), stream()), bufs

    def bwd(need, **kw):
        rc, bufs = raw(need, **kw)
        assert rc == 0, err()
        check_guards(bufs)
        return [None if v is None else v.clone() for _, v in bufs]

    full = bwd((True,) * 4)
    assert all(bool((t != SENTINEL).all()) for t in full)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, bwd((True,) * 4)))      # two full calls: the same bits
    subsets = [need for need in itertools.product((False, True), repeat=4) if any(need)]
    assert len(subsets) == 15
    for need in subsets:
        part = bwd(need, b2=False)
        for name, on, a, b in zip(NAMES, need, part, full):
            assert (a is not None) == on
            if on:
                assert torch.equal(_bits(a), _bits(b)), (need, name)      # the same bits as the all-outputs call
    assert all(torch.equal(a, b) for a, b in zip(tensors, before))      # the operands are untouched
    via = ctx.eemb_backward(*ops, P['w1'], P['b1'], P['w2'], gd, p, seed)
    assert all(torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1))) for a, b in zip(via, full))
    assert raw((False,) * 4)[0] == -1 and b'no gradient' in err()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='at least one'):
        ctx.eemb_backward(*ops, P['w1'], P['b1'], P['w2'], gd, p, seed, need=(False,) * 4)
    with pytest.raises(RuntimeError, match='int32'):
        ctx.eemb_forward(ops[0], ops[1], ops[2].long(), *ops[3:], P['w1'], P['b1'], P['w2'], P['b2'])
    with pytest.raises(RuntimeError, match=r'\[0, 1\)'):
        ctx.eemb_forward(*ops, P['w1'], P['b1'], P['w2'], P['b2'], 1.0, 0)


# ---- 4. no edges -----------------------------------------------------------------------------------------------------------------------------------------------
def test_no_edges(ctx, dev):
    for K in (64, 68):
        o, g = _operands(0, K, 1)
        emb, sh, grads = _device(ctx, dev, o, _params(K, 2), g, p=0.1, seed=5)
        assert emb.shape == (0, 24) and sh.shape == (0, 4)
        assert [a.shape for a in grads] == [(24, K), (24,), (24, 24), (24,)] and not any(a.any() for a in grads)
    # the C entries themselves write the zeros, with no operands and no workspace
    full = lambda *shape: torch.full(shape, 7.0, device=dev)
    outs = [full(24, 68), full(24), full(24, 24), full(24)]
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = [None, 0, None, 0, None, None, None, 4, None, 0, None, 0.0, 5.0, 32, None, None, None, None, 0.1, 5]
    assert ctx.L.ddk_eemb_forward(ctx.h, *none, 0, None, None, stream) == 0, ctx.L.ddk_last_error(ctx.h)
    assert ctx.L.ddk_eemb_backward(ctx.h, *none, None, 0, *[p(t) for t in outs], None, stream) == 0, ctx.L.ddk_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in outs)


# ---- 5. the recomputed hidden layer's zero pattern is the host mask ------------------------------------------------------------------------------------------
def test_recomputed_mask(ctx, dev):
    """The hidden layer never leaves the device; grad_w1 shows its pattern.  Node a of probe edge j belongs to graph j, whose row of the sigma table is the
    unit vector j, every other edge's graph has a zero row: column F + j of grad_w1 is gpre of that ONE edge, gpre[c] = ghid[c] * (hid[c] != 0 ? s : 0).
    With w1 = 0 and b1 > 0 the ReLU passes everywhere, and ghid != 0 for random w2 and grad_emb: the zeros of the column are the mask's.  The probes sit
    at the first and last positions of a call of three slices, so the edge id is the position in the call, not in a workgroup or a slice."""
    E, K, p, seed = 1300, 64, 0.1, 0x0123456789ABCDEF
    o, g = _operands(E, K, 77, n_a=E, T=33)
    probes = np.concatenate([np.arange(16), np.arange(E - 16, E)])
    o['idx_a'] = np.arange(E, dtype=np.int32)
    o['sig_index'] = np.full(E, 32, np.int32)
    o['sig_index'][probes] = np.arange(32)
    o['sig'] = np.concatenate([np.eye(32, dtype=np.float32), np.zeros((1, 32), np.float32)])
    P = _params(K, 78)
    P['w1'][:] = 0
    P['b1'] = np.abs(P['b1']) + np.float32(0.5)
    ops, t = _dev_operands(dev, o), {k: _to(dev, v) for k, v in P.items()}
    gw1 = ctx.eemb_backward(*ops, t['w1'], t['b1'], t['w2'], _to(dev, g), p, seed, need=(True, False, False, False))[0].cpu().numpy()
    keep = ref.keep_mask(seed, E, p)
    assert 0.02 < 1 - keep[probes].mean() < 0.25
    assert np.array_equal(gw1[:, :32].T != 0, keep[probes])
    # and the forward draws the same mask: with w2 = I and b2 = 0 the embedding IS the hidden layer
    t['w2'], t['b2'] = torch.eye(24, device=dev), torch.zeros(24, device=dev)
    emb, _ = ctx.eemb_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], p, seed)
    assert np.array_equal(emb.cpu().numpy() != 0, keep)
    other, _ = ctx.eemb_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], p, seed + 1)
    assert not torch.equal(other != 0, emb != 0)      # another seed: another mask
    plain, _ = ctx.eemb_forward(*ops, t['w1'], t['b1'], t['w2'], t['b2'], 0.0, 0)
    scaled = plain * torch.tensor(np.float32(1) / (np.float32(1) - np.float32(p)), device=dev)
    assert torch.equal(_bits(torch.where(emb != 0, scaled, torch.zeros_like(scaled))), _bits(emb))      # the kept elements carry s and nothing else


# ---- 6. the autograd op ------------------------------------------------------------------------------------------------------------------------------------------
def test_fused_edge_embedding(ctx, dev):
    from disco_diffdock_amd.tensor_layers import GaussianSmearing, fused_edge_embedding
    E, K = 200, 68
    o, g = _operands(E, K, 90)
    torch.manual_seed(3)
    mlp = torch.nn.Sequential(torch.nn.Linear(K, 24), torch.nn.ReLU(), torch.nn.Dropout(0.1), torch.nn.Linear(24, 24)).to(dev)
    expansion = GaussianSmearing(0.0, 5.0, 32).to(dev)
    assert np.array_equal(expansion.offset.cpu().numpy(), ref.offsets(0.0, 5.0)) and np.float32(expansion.coeff) == np.float32(ref.coeff(0.0, 5.0))
    pos_a, pos_b, ia, ib, feat, sig, sig_index = _dev_operands(dev, o)[:7]
    edge_index = torch.stack([ia, ib]).long()
    call = lambda **kw: fused_edge_embedding(mlp, expansion, kw.get('pos_a', pos_a), pos_b, edge_index, sig, sig_index, feat=feat, seed=kw.get('seed', 11))
    gd = _to(dev, g)

    def step(seed=11):
        mlp.zero_grad()
        emb, sh = call(seed=seed)
        assert not sh.requires_grad and emb.requires_grad
        emb.backward(gd)
        return emb.detach(), sh, [q.grad.clone() for q in mlp.parameters()]

    mlp.train()
    emb, sh, grads = step()
    P = dict(w1=mlp[0].weight.detach(), b1=mlp[0].bias.detach(), w2=mlp[3].weight.detach(), b2=mlp[3].bias.detach())
    want = ctx.eemb_forward(pos_a, pos_b, ia, ib, feat, sig, sig_index, 0.0, 5.0, P['w1'], P['b1'], P['w2'], P['b2'], 0.1, 11)
    assert torch.equal(_bits(emb), _bits(want[0])) and torch.equal(_bits(sh), _bits(want[1]))
    raw = ctx.eemb_backward(pos_a, pos_b, ia, ib, feat, sig, sig_index, 0.0, 5.0, P['w1'], P['b1'], P['w2'], gd, 0.1, 11)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, raw))
    again = step()
    assert torch.equal(_bits(again[0]), _bits(emb)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[2], grads))      # one seed: the same bits
    assert not torch.equal(step(seed=12)[0], emb)      # another seed: another mask
    # evaluation: no dropout, and the plain composition in fp32 on the device agrees to fp32 accuracy
    mlp.eval()
    ev, _, gev = step()
    with torch.no_grad():
        vec = pos_b[ib.long()] - pos_a[ia.long()]
        row = torch.cat([feat, sig[sig_index.long()[ia.long()]], expansion(vec.norm(dim=-1))], 1)
    mlp.zero_grad()
    plain = mlp(row)
    plain.backward(gd)
    assert rel_err(ev.cpu().numpy(), plain.detach().cpu().numpy()) < 1e-5
    for a, q in zip(gev, mlp.parameters()):
        assert rel_err(a.cpu().numpy(), q.grad.cpu().numpy()) < 1e-4
    # what is refused
    with pytest.raises(RuntimeError, match='no gradient for the positions'):
        call(pos_a=pos_a.clone().requires_grad_())
    with pytest.raises(RuntimeError, match='GPU only'):
        fused_edge_embedding(mlp.cpu(), expansion, pos_a.cpu(), pos_b.cpu(), edge_index.cpu(), sig.cpu(), sig_index.cpu(), feat=feat.cpu())
    mlp.to(dev)
    with pytest.raises(RuntimeError, match='the row has 64'):
        fused_edge_embedding(mlp, expansion, pos_a, pos_b, edge_index, sig, sig_index, feat=None)
    # nothing per edge is saved but what the caller handed in: the saved tensors are the operands and the parameters
    mlp.train()
    emb, _ = call()
    saved = [t for t in emb.grad_fn.saved_tensors if t is not None]
    given = {t.data_ptr() for t in (pos_a, pos_b, ia, ib, feat, sig, sig_index, *[q for q in mlp.parameters()])}
    assert all(t.data_ptr() in given or (t.dtype == torch.int32 and t.dim() == 1) for t in saved)      # (edge_index's rows, converted to int32)
