"""GPU tests of disco_diffdock_amd.train_model.TrainableScoreModel: a collated batch of different complexes at different times through the graph build,
the node and edge embeddings, conv_stack and ScoreHeads.

(a) the gradient of EVERY parameter against autograd through the oracle (oracle.score_model_ref.score_model_forward) in fp64, same state dict, a fixed
    random linear functional of (tr, rot, tor) as the loss.  The bar of a parameter tensor is MEASURED: the same oracle run in fp32 on the host against
    its fp64 run gives err32; the device passes under 4 * err32, floored at 1e-5.  Both are fp32 evaluations that differ in summation order; 4 is the
    allowance for that.  Forward outputs: the project's 1e-4.
    The ReLU kink: a summation order decides the BRANCH of a hidden unit whose pre-activation lies within fp32 rounding of zero, and the two branches'
    gradients differ by a whole term, not by rounding.  With the weights of seed 5 the oracle's fp64 pre-activation of ONE unit of 1.9 million is
    1.4e-8 (conv layer 4, the ligand <- receptor group, an edge of residue 74; the host's fp32 run gives 6.0e-8, the rms difference of the two runs
    in that tensor is 7.9e-8): the device took the other branch, the gradient of that one residue's row was off by 4.2e-6 where every other row agreed
    to 4e-8, and the receptor-side parameters showed 2e-5 .. 9e-5 (ligand side: 3e-6 .. 5e-6) against host figures of 1e-6.  That comparison measures
    the input, not the model, so the test states what it needs of its input and asserts it FIRST, from the oracle alone: every pre-activation of
    the three edge embeddings and of the conv layers' radial MLPs is at least 8 times its tensor's rms fp32-against-fp64 difference away from zero.
    The weights of seed 9 meet that.  (The heads' MLPs, 1 % of the hidden units, are not covered by the assertion.)
(b) the round trip to the inference engine: .eval() against TensorProductScoreModel loaded from this module's state_dict, 1e-4.
(c) training: one loss_function(...).backward() reaches every parameter, and two Adam steps from one state and one seed give identical bits."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import rel_err, to_graph
from oracle import graph_lite
from oracle import score_model_ref as smr
from test_gpu_radial_conv import _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
TIMES = (0.2, 0.5, 0.75)
COMPLEXES = ((70, 22), (71, 28), (60, 35))      # (seed, residues): ligands of 16 atoms with four rotatable bonds each
MODEL = dict(sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, lm_embedding_type='esm')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _tables():
    d = os.path.join(os.path.dirname(__file__), '..', 'disco_diffdock_amd', 'data')
    return np.load(os.path.join(d, 'so3_exp_score_norms.npy')), np.load(os.path.join(d, 'torus_score_norm_seed0.npy'))


def _batch():
    """three different synthetic complexes, their ligands slightly off the true pose, collated as the reference's loader does, each at its own time"""
    from disco_diffdock_amd import synthetic
    cs = [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in COMPLEXES]
    rng = np.random.default_rng(8)
    for c in cs:
        assert 20 <= len(c['rec_pos']) <= 40 and 8 <= len(c['lig_pos']) <= 16 and int(c['edge_mask'].sum()) >= 1
        c['lig_pos'] = (c['lig_pos'] + rng.normal(0, 1.0, size=(1, 3)) + rng.normal(0, 0.2, size=c['lig_pos'].shape)).astype(np.float32)
    b = graph_lite.collate([to_graph(c) for c in cs])
    b.complex_t = {k: torch.tensor(TIMES) for k in ('tr', 'rot', 'tor')}
    for nt in ('ligand', 'receptor'):
        b[nt].node_t = {k: b.complex_t[k][b[nt].batch] for k in ('tr', 'rot', 'tor')}
    return cs, b


def _functional(n_tor, seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((3, 3), (3, 3), (n_tor,))]


def _oracle_gradients(cfg, P, batch, dtype):
    Pd = {k: (v.detach().to(dtype).requires_grad_() if v.is_floating_point() else v) for k, v in P.items()}
    so3, torus = _tables()
    out = smr.score_model_forward(Pd, cfg, copy.deepcopy(batch), so3, torus, dtype=dtype)
    loss = sum((o.double() * w).sum() for o, w in zip(out, _functional(out[2].shape[0])))
    loss.backward()
    return [o.detach().double().numpy() for o in out], {k: v.grad.double().numpy() for k, v in Pd.items() if v.is_floating_point() and v.grad is not None}


def _relu_preactivations(cfg, P, batch, dtype):
    """the oracle's pre-activations in front of the ReLUs of the three edge embeddings and of every conv layer's radial MLPs (name -> [E_g, 24 | 72])"""
    Pd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    b = copy.deepcopy(batch)
    for nt in ('ligand', 'receptor'):
        b[nt].pos = b[nt].pos.to(dtype)
    lig, rec = smr.build_lig_conv_graph(b, cfg, None, dtype), smr.build_rec_conv_graph(b, cfg, None, dtype)
    tr_sigma = smr.t_to_sigma(*[b.complex_t[k] for k in ('tr', 'rot', 'tor')], cfg)[0]
    cross = smr.build_cross_conv_graph(b, cfg, (tr_sigma * 3 + 20).unsqueeze(1).to(dtype), lig[4], None, dtype)
    lin = lambda row, name: row @ Pd[f'{name}.weight'].T + Pd[f'{name}.bias']
    out = {f'{name}_edge_embedding': lin(row, f'{name}_edge_embedding.0') for name, row in (('lig', lig[2]), ('rec', rec[2]), ('cross', cross[1]))}
    g = smr.embed(Pd, cfg, b, dtype, True)[-1]
    ei, offs = g['edge_index'], (0,) + tuple(g['splits']) + (g['edge_index'].shape[1],)
    for l in range(cfg.num_conv_layers):
        x = g['x0'] if l == 0 else g['layers'][l - 1]
        ea = torch.cat([g['edge_emb'], x[ei[0], :cfg.ns], x[ei[1], :cfg.ns]], -1)
        for grp in range(4):
            out[f'conv_layers.{l}.fc.{grp}'] = lin(ea[offs[grp]:offs[grp + 1]], f'conv_layers.{l}.fc.{grp}.0')
    return out


@pytest.fixture(scope='module')
def parity_reference():
    """computed once: the oracle's outputs and parameter gradients in fp64 and in fp32 (configuration (a): no BatchNorm, no dropout), and how far its
    hidden units stay from the ReLU's kink, in units of the tensor's rms fp32-against-fp64 difference"""
    cfg = smr.ScoreModelConfig(batch_norm=False)
    P = smr.random_state_dict(cfg, seed=9)
    _, b = _batch()
    out64, g64 = _oracle_gradients(cfg, P, b, torch.float64)
    out32, g32 = _oracle_gradients(cfg, P, b, torch.float32)
    p64, p32 = _relu_preactivations(cfg, P, b, torch.float64), _relu_preactivations(cfg, P, b, torch.float32)
    clearance = {k: float(p64[k].abs().min() / (p32[k].double() - p64[k]).pow(2).mean().sqrt()) for k in p64}
    return dict(cfg=cfg, P=P, out64=out64, g64=g64, out32=out32, g32=g32, clearance=clearance, hidden_units=sum(v.numel() for v in p64.values()))


def _model(dev, P=None, **kw):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    model = TrainableScoreModel(**dict(MODEL, **kw))
    if P is not None:
        model.load_state_dict({k: v for k, v in P.items() if k in model.state_dict()}, strict=True)
    return model.to(dev)


# ---- (a) gradient parity with the oracle ---------------------------------------------------------------------------------------------------------------------
def test_gradient_parity_with_the_oracle(dev, parity_reference):
    r = parity_reference
    tight = min(r['clearance'], key=r['clearance'].get)
    print(f"{r['hidden_units']} hidden units, the closest to the kink: {tight} at {r['clearance'][tight]:.1f} rms fp32 differences")
    assert r['clearance'][tight] >= 8, (tight, r['clearance'][tight])      # the input leaves every ReLU branch to the model, none to a summation order
    model = _model(dev, r['P'], batch_norm=False, dropout=0.0).train()
    assert set(model.state_dict()) == {k for k in r['P'] if '.batch_norm.' not in k}
    _, b = _batch()
    out = model(b.to(dev))
    loss = sum((o.double() * w.to(dev)).sum() for o, w in zip(out, _functional(out[2].shape[0])))
    loss.backward()
    assert out[2].shape == (sum(int(c['edge_mask'].sum()) for c in _batch()[0]),)
    for name, a, w, w32 in zip(('tr', 'rot', 'tor'), out, r['out64'], r['out32']):
        err, err32 = rel_err(a.detach().cpu().numpy(), w), rel_err(w32, w)
        print(f'forward {name}: device {err:.2e}, host fp32 {err32:.2e}')
        _record_drift(f'train_model.forward.{name}', err, host_fp32=err32, bar=1e-4)
        assert err < 1e-4, (name, err)
    failures = []
    for k, p in model.named_parameters():
        if p.numel() == 0:
            continue
        assert p.grad is not None, k
        want = r['g64'][k]
        if not want.any():      # (the last conv layer's receptor-side groups: nothing reads the receptor rows after it)
            assert not bool(p.grad.any()), k
            continue
        err, err32 = rel_err(p.grad.cpu().numpy(), want), rel_err(r['g32'][k], want)
        bar = max(4 * err32, 1e-5)
        print(f'{k}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record_drift(f'train_model.grad.{k}', err, host_fp32=err32, bar=bar)
        if not err < bar:
            failures.append((k, err, err32, bar))
    assert not failures, failures


# ---- (b) round trip to the inference engine ----------------------------------------------------------------------------------------------------------------------
def test_round_trip_to_the_inference_engine(dev):
    from functools import partial
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    from disco_diffdock_amd.model_utils import get_model
    from test_gpu_model import ARGS_S, CFG, _dev_batch
    trainable = _model(dev, smr.random_state_dict(CFG, seed=9), dropout=0.1).eval()
    engine = get_model(ARGS_S, dev, partial(t_to_sigma, args=ARGS_S), no_parallel=True).score_model
    engine.load_state_dict(trainable.state_dict(), strict=True)
    c = synthetic.make_complex(71, n_res=28, n_lig=12)
    rng = np.random.default_rng(3)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 1.5, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(4)]).astype(np.float32)
    for t in (0.7, 0.2):
        b = _dev_batch(c, 4, pos, dev, t)
        want = engine(b)
        with torch.no_grad():
            got = trainable(b)
        assert got[2].shape == want[2].shape == (4 * int(c['edge_mask'].sum()),)
        errs = {n: rel_err(a.cpu().numpy(), w.cpu().numpy()) for n, a, w in zip(('tr', 'rot', 'tor'), got, want)}
        print(t, {k: f'{v:.2e}' for k, v in errs.items()})
        worst = max(errs, key=errs.get)
        _record_drift(f'train_model.round_trip.t{t}', errs[worst], worst_block=worst, bar=1e-4)
        assert errs[worst] < 1e-4, (t, worst, errs[worst])


# ---- (c) training --------------------------------------------------------------------------------------------------------------------------------------------------
def _made_up_targets(dev, model, B, n_rot, t, seed):
    from disco_diffdock_amd import training
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    tr_sigma, rot_sigma, tor_sigma = training._sigmas(model.ctx, t)
    return training.Targets(r(B, 3), r(B, 3), r(B, n_rot), tr_sigma, rot_sigma, tor_sigma, t, None, None, None)


def test_training_step_reaches_every_parameter_and_is_reproducible(dev, parity_reference):
    """batch_norm=True, dropout 0.1, .train(): one loss_function(...).backward() reaches every parameter; two Adam steps from one state and one seed give
    identical parameter bits"""
    from disco_diffdock_amd import training
    cs, b = _batch()
    b = b.to(dev)
    n_rot = int(cs[0]['edge_mask'].sum())
    assert all(int(c['edge_mask'].sum()) == n_rot for c in cs)      # (loss_function takes [B, n_rot] torsion targets)
    P = smr.random_state_dict(smr.ScoreModelConfig(), seed=6)
    targets = None
    # Where the oracle's gradient is zero: without BatchNorm the receptor-side groups of the LAST conv layer (nothing reads the receptor rows after it).
    # With BatchNorm on batch statistics those rows enter the ligand rows' mean and variance, so here nothing is dead
    dead = {k for k, g in parity_reference['g64'].items() if not g.any()}
    assert dead and all(k.startswith(('conv_layers.4.fc.2.', 'conv_layers.4.fc.3.')) for k in dead)

    def run():
        nonlocal targets
        torch.manual_seed(4321)
        model = _model(dev, P, batch_norm=True, dropout=0.1).train()
        if targets is None:
            targets = _made_up_targets(dev, model, 3, n_rot, 0.5, 31)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        first = None
        for _ in range(2):
            opt.zero_grad()
            tr, rot, tor = model(b)
            loss = training.loss_function(tr, rot, tor, targets, model)[0]
            loss.backward()
            if first is None:
                first = {k: p.grad.clone() if p.grad is not None else None for k, p in model.named_parameters() if p.numel()}      # (final_conv's BatchNorm has no scalars: an empty bias)
            opt.step()
        return loss.detach(), first, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (loss_a, grads, state_a), (loss_b, _, state_b) = run(), run()
    assert bool(torch.isfinite(loss_a).all())
    for k, g in grads.items():
        assert g is not None, k
        assert bool(torch.isfinite(g).all()), k
        assert bool((g != 0).any()), k      # none all zero
    assert torch.equal(_bits(loss_a), _bits(loss_b))
    for k in state_a:
        assert torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())), k
    moved = [k for k, v in _model(dev, P).state_dict().items() if v.numel() and not torch.equal(v, state_a[k])]
    assert len(moved) >= len(grads)      # the steps moved every parameter (and BatchNorm's statistics)
