"""GPU tests of disco_diffdock_amd.latent_encoder.TPEncoder (ns 24, nv 4, 3 conv layers, latent_dim 2) on a collated batch of three synthetic complexes.

(a) logits and the gradient of EVERY parameter against the fp64 restatement tests/latent_encoder_ref.encoder_logits (no BatchNorm, no dropout, no Gumbel
    step; a fixed random linear functional of the logits as the loss).  Logits: the project's 1e-4.  Gradients: max(4 * err32, 1e-5), err32 the same
    restatement run in fp32 on the host against its fp64 run: the measured bar of tests/test_gpu_train_model.py, for its reason (both are fp32
    evaluations that differ in summation order).  Its ReLU-kink condition is asserted FIRST, from the restatement alone: every hidden pre-activation of the
    three edge embeddings and of the conv layers' radial MLPs is at least 8 rms fp32-against-fp64 differences from zero.  The weights of seed 11 meet that.
(b) the same with BatchNorm and BatchNorm1d on, in .train(): logits under max(4 * err32, 1e-4); the running buffers of every norm layer moved.
(c) BatchNorm off, .eval(): a graph's logits are bit-identical whether it is collated alone or as any member of the batch (the encoder runs its torch
    Linears graph by graph there: the receptor embedding's GEMM gave other last bits at 22 rows than at 85).
(d) the Gumbel wiring: the output is ragged_gumbel_softmax of the encoder's own logits, bit for bit, one-hot per (graph, dimension).
(e) LatentModelWrapper(TPEncoder, TrainableScoreModel): noise_batch -> forward -> loss_function -> backward reaches every parameter of both; two Adam steps
    from one state and one seed give identical bits, another seed does not.
(f) training.train_epoch runs and returns the same seven meters on two runs from one state."""
import copy

import numpy as np
import pytest
import torch

import latent_encoder_ref as ler
from helpers import rel_err, to_graph
from oracle import graph_lite
from test_gpu_radial_conv import _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
COMPLEXES = ((70, 22), (71, 28), (60, 35))      # (seed, residues): ligands of 16 atoms with four rotatable bonds each
ENCODER = dict(latent_dim=2, latent_vocab=1, sh_lmax=1, ns=24, nv=4, num_conv_layers=3, lig_max_radius=5.0, rec_max_radius=30.0, cross_max_distance=80.0,
               lm_embedding_type='esm')
SEED = 11      # of the weights; chosen on the host for the ReLU-kink condition of (a)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _complexes():
    from disco_diffdock_amd import synthetic
    cs = [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in COMPLEXES]
    for c in cs:
        assert 20 <= len(c['rec_pos']) <= 40 and 8 <= len(c['lig_pos']) <= 16 and int(c['edge_mask'].sum()) >= 1
    return cs


def _batch(cs):
    """the complexes collated as the reference's loader does, the true pose under the name the encoder reads"""
    b = graph_lite.collate([to_graph(c) for c in cs])
    b['ligand'].orig_pos_torch = b['ligand'].pos.clone()
    b.name = [c['name'] for c in cs]
    return b


def _encoder(seed=SEED, **kw):
    """a TPEncoder on the host with seeded weights; the norm layers' parameters and running buffers are moved off their initial values"""
    from disco_diffdock_amd.latent_encoder import TPEncoder
    torch.manual_seed(seed)
    enc = TPEncoder(None, **dict(ENCODER, **kw))
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            if 'batch_norm.' in k or k.split('.')[-2] in ('1', '5') and k.startswith('latent_'):
                if k.endswith(('weight', 'running_var')):
                    v.copy_(torch.rand(v.shape, generator=gen) + 0.5)
                elif k.endswith(('bias', 'running_mean')):
                    v.copy_(torch.randn(v.shape, generator=gen) * 0.1)
    return enc


def _cfg(enc, batch_norm, latent_batchnorm):
    return dict(nv=enc.nv, num_conv_layers=enc.num_conv_layers, lig_max_radius=enc.lig_max_radius, rec_max_radius=enc.rec_max_radius,
                cross_max_distance=enc.cross_max_distance, batch_norm=batch_norm, latent_batchnorm=latent_batchnorm)


def _functional(n_lig, n_rec, D, seed=21):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n_lig, D, generator=gen, dtype=torch.float64), torch.randn(n_rec, D, generator=gen, dtype=torch.float64)


def _restatement(state, cfg, batch, dtype, training):
    """logits, parameter gradients of the functional, hidden pre-activations, norm statistics of the restatement in ``dtype``"""
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    params = [k for k, v in P.items() if v.is_floating_point() and 'running_' not in k and not k.endswith('offset')]
    for k in params:
        P[k].requires_grad_(True)
    hidden = {}
    logit_l, logit_r, stats = ler.encoder_logits(P, cfg, copy.deepcopy(batch), dtype, training=training, hidden=hidden)
    wl, wr = _functional(logit_l.shape[0], logit_r.shape[0], logit_l.shape[1])
    ((logit_l.double() * wl).sum() + (logit_r.double() * wr).sum()).backward()
    grads = {k: P[k].grad.double().numpy() for k in params if P[k].grad is not None}
    return (logit_l.detach().double().numpy(), logit_r.detach().double().numpy()), grads, hidden, stats


@pytest.fixture(scope='module')
def reference():
    """computed once and left unchanged: the restatement in fp64 and in fp32 for configuration (a) (no norm layers) and (b) (all norm layers, training)"""
    b = _batch(_complexes())
    out = {}
    for tag, bn in (('a', False), ('b', True)):
        enc = _encoder(batch_norm=bn, latent_no_batchnorm=not bn)
        cfg = _cfg(enc, bn, bn)
        r64, r32 = (_restatement(enc.state_dict(), cfg, b, dt, training=bn) for dt in (torch.float64, torch.float32))
        clearance = {k: float(r64[2][k].abs().min() / (r32[2][k].double() - r64[2][k]).pow(2).mean().sqrt()) for k in r64[2]}
        out[tag] = dict(state=copy.deepcopy(enc.state_dict()), out64=r64[0], g64=r64[1], out32=r32[0], g32=r32[1], clearance=clearance,
                        hidden_units=sum(v.numel() for v in r64[2].values()), stats=r64[3])
    return out


def _device_run(enc, dev, b):
    enc.zero_grad(set_to_none=True)
    logit_l, logit_r, _, _ = enc.logits(copy.deepcopy(b).to(dev))
    wl, wr = _functional(logit_l.shape[0], logit_r.shape[0], logit_l.shape[1])
    ((logit_l.double() * wl.to(dev)).sum() + (logit_r.double() * wr.to(dev)).sum()).backward()
    return logit_l.detach().cpu().numpy(), logit_r.detach().cpu().numpy()


# ---- (a) accuracy against the fp64 restatement ---------------------------------------------------------------------------------------------------------------
def test_logits_and_gradients_against_fp64(dev, reference):
    r = reference['a']
    tight = min(r['clearance'], key=r['clearance'].get)
    print(f"{r['hidden_units']} hidden units, the closest to the kink: {tight} at {r['clearance'][tight]:.1f} rms fp32 differences")
    assert len(r['clearance']) == 3 + 3 * 4
    assert r['clearance'][tight] >= 8, (tight, r['clearance'][tight])      # the input leaves every ReLU branch to the model, none to a summation order
    enc = _encoder(batch_norm=False, latent_no_batchnorm=True, apply_gumbel_softmax=False)
    enc.load_state_dict(r['state'], strict=True)
    enc = enc.to(dev).train()
    got = _device_run(enc, dev, _batch(_complexes()))
    for name, a, w, w32 in zip(('ligand', 'receptor'), got, r['out64'], r['out32']):
        err, err32 = rel_err(a, w), rel_err(w32, w)
        print(f'logits {name}: device {err:.2e}, host fp32 {err32:.2e}')
        _record_drift(f'train_encoder.logits.{name}', err, host_fp32=err32, bar=1e-4)
        assert a.shape == w.shape and err < 1e-4, (name, err)
    failures, seen = [], 0
    for k, p in enc.named_parameters():
        assert p.grad is not None and k in r['g64'], k
        want = r['g64'][k]
        assert want.any(), k      # the encoder reads the ligand and the receptor rows of its last layer: no parameter is dead
        err, err32 = rel_err(p.grad.cpu().numpy(), want), rel_err(r['g32'][k], want)
        bar = max(4 * err32, 1e-5)
        print(f'{k}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record_drift(f'train_encoder.grad.{k}', err, host_fp32=err32, bar=bar)
        seen += 1
        if not err < bar:
            failures.append((k, err, err32, bar))
    assert seen == len(r['g64']) and not failures, failures


# ---- (b) with every norm layer on, in training --------------------------------------------------------------------------------------------------------------------
def test_logits_with_batch_norm_in_training(dev, reference):
    r = reference['b']
    enc = _encoder(batch_norm=True, latent_no_batchnorm=False, apply_gumbel_softmax=False)
    enc.load_state_dict(r['state'], strict=True)
    enc = enc.to(dev).train()
    got = _device_run(enc, dev, _batch(_complexes()))
    for name, a, w, w32 in zip(('ligand', 'receptor'), got, r['out64'], r['out32']):
        err, err32 = rel_err(a, w), rel_err(w32, w)
        bar = max(4 * err32, 1e-4)
        print(f'logits {name}, norm layers on: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record_drift(f'train_encoder.bn.logits.{name}', err, host_fp32=err32, bar=bar)
        assert err < bar, (name, err, bar)
    after = enc.state_dict()
    moved = [k for k in after if 'running_' in k or k.endswith('num_batches_tracked')]
    assert len(moved) == 2 * 3 + 2 * 2 * 3      # three conv layers, two norm layers in each predictor
    for k in moved:
        assert not torch.equal(after[k].cpu(), r['state'][k]), k
    for name, (mean, second) in r['stats'].items():      # and to where the restatement's batch statistics put them
        for key, stat in (('running_mean', mean), ('running_var', second)):
            want = 0.9 * r['state'][f'{name}.{key}'].double().numpy() + 0.1 * stat.numpy()
            assert rel_err(after[f'{name}.{key}'].cpu().numpy(), want) < 1e-4, (name, key)


# ---- (c) independence from the batch --------------------------------------------------------------------------------------------------------------------------------
def test_logits_do_not_depend_on_the_batch(dev, reference):
    cs = _complexes()
    enc = _encoder(batch_norm=False, latent_no_batchnorm=True, apply_gumbel_softmax=False, dropout=0.1, latent_dropout=0.1)
    enc.load_state_dict(reference['a']['state'], strict=True)
    enc = enc.to(dev).eval()
    with torch.no_grad():
        together = enc(_batch(cs).to(dev))
        assert len(together) == 3
        for g, c in enumerate(cs):
            (alone,) = enc(_batch([c]).to(dev))
            assert alone.shape == together[g].shape == (1, 2, len(c['lig_pos']) + len(c['rec_pos']))
            assert torch.equal(_bits(alone), _bits(together[g])), g


# ---- (d) the Gumbel wiring -------------------------------------------------------------------------------------------------------------------------------------------
def test_gumbel_output_is_the_ragged_op_on_the_encoders_logits(dev, reference):
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.tensor_layers import ragged_gumbel_softmax
    cs = _complexes()
    enc = _encoder(batch_norm=False, latent_no_batchnorm=True, apply_gumbel_softmax=True)
    enc.load_state_dict(reference['a']['state'], strict=True)
    enc = enc.to(dev).eval()
    enc.latent_temperature = 0.7
    b = _batch(cs).to(dev)
    with torch.no_grad():
        latent_l, latent_r = enc(b, seed=1234)
        logit_l, logit_r, lig_batch, rec_batch = enc.logits(b, seed=1234)
        want_l, want_r = ragged_gumbel_softmax(logit_l, logit_r, lig_batch, rec_batch, 0.7, enc.gumbel_seed(1234), [stream_id(c['name']) for c in cs])
    assert torch.equal(_bits(latent_l), _bits(want_l)) and torch.equal(_bits(latent_r), _bits(want_r))
    assert latent_l.shape == (logit_l.shape[0], 2) and latent_r.shape == (logit_r.shape[0], 2)
    for g in range(3):
        col = torch.cat([latent_l[lig_batch == g], latent_r[rec_batch == g]], 0)
        assert bool(((col == 0) | (col == 1)).all()) and bool((col.sum(0) == 1).all()), g      # one-hot per (graph, dimension)


# ---- (e) a training step of the wrapper -------------------------------------------------------------------------------------------------------------------------------
def _wrapper(dev, enc_state, score_state):
    from disco_diffdock_amd.train_model import LatentModelWrapper, TrainableScoreModel
    enc = _encoder(batch_norm=True, latent_no_batchnorm=False, dropout=0.1, latent_dropout=0.1)
    score = TrainableScoreModel(sh_lmax=1, ns=24, nv=6, num_conv_layers=3, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True,
                                lm_embedding_type='esm', latent_dim=2, latent_vocab=1, latent_droprate=0.1, batch_norm=True, dropout=0.1)
    if enc_state is not None:
        enc.load_state_dict(enc_state, strict=True)
        score.load_state_dict(score_state, strict=True)
    return LatentModelWrapper(enc, score, training_latent_temperature=1.0, latent_droprate=0.1).to(dev)


def test_training_step_reaches_every_parameter_and_is_reproducible(dev):
    from disco_diffdock_amd import training
    cs = _complexes()
    torch.manual_seed(11)
    start = _wrapper(dev, None, None)
    with torch.no_grad():      # the unconditional embeddings start at zero in the reference; off zero here, so that the edge rows' gradient reaches them
        for k, p in start.named_parameters():
            if 'unconditional_embedding' in k:
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(dev) * 0.1)
    enc_state, score_state = copy.deepcopy(start.encoder.state_dict()), copy.deepcopy(start.score_model.state_dict())
    keep = np.array([1.0, 0.0, 1.0], np.float32)      # both branches of the latent dropout are in the batch

    def run(seed):
        torch.manual_seed(4321)
        model = _wrapper(dev, enc_state, score_state).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        first = None
        for step in range(2):
            data, targets = training.noise_batch(model, cs, [0.2, 0.5, 0.75], seed=5, draw=step)
            assert torch.equal(data['ligand'].orig_pos_torch.cpu(), torch.cat([torch.as_tensor(c['lig_pos']).float() for c in cs]))
            opt.zero_grad()
            tr, rot, tor = model(data, seed=seed, keep=keep)
            loss = training.loss_function(tr, rot, tor, targets, model)[0]
            loss.sum().backward()
            if first is None:
                first = {k: p.grad.clone() if p.grad is not None else None for k, p in model.named_parameters() if p.numel()}
            opt.step()
        return first, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (grads, state_a), (_, state_b), (_, state_c) = run(99), run(99), run(100)
    assert sum(k.startswith('encoder.') for k in grads) == len(list(start.encoder.parameters())) and any(k.startswith('score_model.') for k in grads)
    for k, g in grads.items():
        assert g is not None, k
        assert bool(torch.isfinite(g).all()), k
        assert bool((g != 0).any()), k      # none all zero: the encoder behind the Gumbel step, the score model
    assert any(k.startswith('encoder.') and 'running_' in k for k in state_a) and any(k.startswith('score_model.') for k in state_a)
    for k in state_a:
        assert torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())), k      # one state, one seed: the same bits, both modules
    changed = [k for k in state_a if state_a[k].is_floating_point() and not torch.equal(state_a[k], state_c[k])]
    assert any(k.startswith('encoder.') for k in changed) and any(k.startswith('score_model.') for k in changed)      # another seed: other masks, another draw


# ---- (f) an epoch ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_train_epoch_with_the_encoder(dev):
    from disco_diffdock_amd import training
    cs = _complexes()
    torch.manual_seed(12)
    start = _wrapper(dev, None, None)
    enc_state, score_state = copy.deepcopy(start.encoder.state_dict()), copy.deepcopy(start.score_model.state_dict())

    def run():
        model = _wrapper(dev, enc_state, score_state)
        summary = training.train_epoch(model, cs, torch.optim.Adam(model.parameters(), lr=1e-3), 2, seed=7, epoch=1)
        return summary, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (sum_a, state_a), (sum_b, state_b) = run(), run()
    assert set(sum_a) == set(training.TRAIN_METERS) and len(sum_a) == 7 and all(np.isfinite(v) for v in sum_a.values()) and sum_a == sum_b
    assert all(torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())) for k in state_a)
    assert any(not torch.equal(state_a['encoder.' + k], v) for k, v in enc_state.items() if v.is_floating_point())      # the epoch moved the encoder
