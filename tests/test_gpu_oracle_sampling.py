"""Sampling with ORACLE latents (sampling(ar_model=None)), the encoder half of the inference ModelWrapper and compute_ar_accuracy, on deterministic = 1
contexts.  One synthetic complex (40 residues, 22 ligand atoms), a random-init score model (latent_dim 2) and a random-init TPEncoder of 3 layers at
ns 24 / nv 4 (tests/oracle_latents_ref.py), 4 steps, 8 samples."""
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

import oracle_latents_ref as olr
from oracle import ar_ref
from oracle import sampler_ref as spr
from oracle import score_model_ref as smr
from helpers import rel_err, to_graph
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ARGS = Namespace(ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                 max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, embedding_scale=1000, embedding_type='sinusoidal',
                 scale_by_sigma=True, no_torsion=False, no_batch_norm=False, dropout=0.1, sh_lmax=1, use_second_order_repr=False,
                 use_old_atom_encoder=False, esm_embeddings_path='data/esm2_3billion_embeddings.pt', latent_dim=2, latent_vocab=1, latent_droprate=0.1,
                 latent_cross_attention=False, tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55,
                 tor_sigma_min=0.03, tor_sigma_max=3.14, encoder_ns=24, encoder_nv=4, encoder_num_conv_layers=3, encoder_cross_max_distance=80,
                 training_latent_temperature=1.0)
CFG = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
STEPS, N, SEED = 4, olr.SAMPLES, olr.SAMPLING_SEED


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def det_env():
    mp = pytest.MonkeyPatch()
    mp.setenv('DDK_DETERMINISTIC', '1')
    yield
    mp.undo()


@pytest.fixture(scope='module')
def cplx():
    c = olr.sampling_complex()
    assert int(np.asarray(c['edge_mask']).sum()) >= 1
    return c


@pytest.fixture(scope='module')
def weights():
    """computed once and left unchanged: the score model's state dict and the encoder's, and both under the wrapper's keys"""
    P = smr.random_state_dict(CFG, seed=13)
    E = {k: v.detach().clone() for k, v in olr.host_encoder().state_dict().items()}
    full = {**{'score_model.' + k: v for k, v in P.items()}, **{'encoder.' + k: v for k, v in E.items()}}
    return dict(P=P, E=E, full=full)


def _new_model(dev):
    from disco_diffdock_amd.model_utils import get_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    return get_model(ARGS, dev, partial(t_to_sigma, args=ARGS), no_parallel=True)


@pytest.fixture(scope='module')
def model(dev, det_env, weights):
    m = _new_model(dev)
    assert m.encoder is None
    m.load_state_dict(weights['full'], strict=True)
    assert int(m.score_model.ctx.cfg.deterministic) == 1
    return m


def _graphs(c, lo, hi):
    """the copies with the global sample indices lo .. hi - 1, each at its own start pose (a fixed shift per global index), with the true pose"""
    from disco_diffdock_amd.data import from_arrays
    shifts = np.random.default_rng(2).normal(0, 4.0, size=(N, 1, 3)).astype(np.float32)
    dl = [from_arrays(c) for _ in range(lo, hi)]
    for d, i in zip(dl, range(lo, hi)):
        d['ligand'].pos = T(np.asarray(c['lig_pos'], np.float32) + shifts[i]).float()
        d['ligand'].ar_pos = d['ligand'].pos.clone()
        d['ligand'].orig_pos_torch = T(np.asarray(c['lig_pos'], np.float32).copy())
    return dl


def _run(model, c, dev, lo=0, hi=N, graphs=None, **kw):
    from disco_diffdock_amd.sampling import sampling
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    sched = get_t_schedule(STEPS)
    kw.setdefault('batch_size', hi - lo)
    kw.setdefault('seed', SEED)
    out, _ = sampling(_graphs(c, lo, hi) if graphs is None else graphs, model, STEPS, sched, sched, sched, dev, partial(t_to_sigma, args=ARGS), ARGS,
                      no_final_step_noise=True, gumbel_latent_temperature=olr.SAMPLING_T, **kw)
    return torch.stack([d['ligand'].pos for d in out]).cpu(), out


def _picks(lat):
    """[n] latent_str -> the picked positions [n, D] (ligand nodes first)"""
    out = []
    for s in lat:
        row, tok = [], s.replace('L', ' L').replace('R', ' R').split()
        for t in tok:
            row.append(int(t[1:]) + (olr.COMPLEX['n_lig'] if t[0] == 'R' else 0))
        out.append(row)
    return out


# ---- loading ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_checkpoint_fills_both_halves(dev, det_env, model, weights, cplx):
    from disco_diffdock_amd.latent_encoder import TPEncoder
    from disco_diffdock_amd.model_utils import get_trainable_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    assert isinstance(model.encoder, TPEncoder) and not model.encoder.training
    assert next(model.encoder.parameters()).is_cuda
    for k, v in model.encoder.state_dict().items():
        assert torch.equal(v.cpu(), weights['E'][k]), k
    # a checkpoint as this project's training writes it: LatentModelWrapper.state_dict()
    torch.manual_seed(3)
    trained = get_trainable_model(ARGS, dev, partial(t_to_sigma, args=ARGS))
    state = trained.state_dict()
    assert any(k.startswith('encoder.') for k in state) and any(k.startswith('score_model.') for k in state)
    m = _new_model(dev)
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in trained.encoder.state_dict().items():
        assert torch.equal(m.encoder.state_dict()[k], v), k
    assert torch.isfinite(_run(m, cplx, dev, 0, 2)[0]).all()
    # a missing encoder key raises with strict, and is reported without
    short = {k: v for k, v in state.items() if k != 'encoder.latent_s_predictor.8.bias'}
    with pytest.raises(RuntimeError, match='latent_s_predictor.8.bias'):
        _new_model(dev).load_state_dict(short, strict=True)
    assert 'encoder.latent_s_predictor.8.bias' in _new_model(dev).load_state_dict(short, strict=False).missing_keys
    with pytest.raises(RuntimeError, match='unexpected'):
        _new_model(dev).load_state_dict(dict(state, **{'decoder.weight': torch.zeros(1)}), strict=True)
    # attach_encoder takes a live encoder, by reference
    m2 = _new_model(dev)
    m2.load_state_dict(weights['P'], strict=True)
    assert m2.encoder is None
    assert m2.attach_encoder(trained.encoder).encoder is trained.encoder and not trained.encoder.training
    with pytest.raises(RuntimeError, match='TPEncoder'):
        m2.attach_encoder(torch.nn.Linear(1, 1))
    # an encoder configuration TPEncoder refuses still raises by name
    with pytest.raises(RuntimeError, match='latent_virtual_nodes'):
        from disco_diffdock_amd.model_utils import get_model
        get_model(Namespace(**dict(vars(ARGS), latent_virtual_nodes=True)), dev, partial(t_to_sigma, args=ARGS), no_parallel=True).load_state_dict(state)


def test_bare_checkpoint_leaves_no_encoder(dev, det_env, weights, cplx):
    m = _new_model(dev)
    m.load_state_dict(weights['P'], strict=True)
    assert m.encoder is None
    with pytest.raises(RuntimeError, match='no encoder'):
        _run(m, cplx, dev)
    m.load_state_dict({'score_model.' + k: v for k, v in weights['P'].items()}, strict=True)
    assert m.encoder is None
    from disco_diffdock_amd.sampling import oracle_latents
    from disco_diffdock_amd.data import collate
    with pytest.raises(RuntimeError, match='no encoder'):
        oracle_latents(m, collate(_graphs(cplx, 0, 2)), olr.SAMPLING_T, SEED)


# ---- sampling --------------------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_sampling_is_seeded_and_cut_invariant(dev, model, cplx):
    """fails on a tree without the feature: there sampling(ar_model=None) of a latent-conditioned model raises"""
    def go(lo=0, hi=N, **kw):
        pos, out = _run(model, cplx, dev, lo, hi, **kw)
        return pos, [d.latent_str for d in out]

    a, lat_a = go()
    assert torch.isfinite(a).all() and all(len(s) >= 4 for s in lat_a)
    b, lat_b = go()
    assert torch.equal(a, b) and lat_a == lat_b                                      # twice
    b, lat_b = go(batch_size=4)
    assert torch.equal(a, b) and lat_a == lat_b                                      # batch size 8 vs 4
    lo, lat_lo = go(0, 4, sample_offset=0)
    hi, lat_hi = go(4, 8, sample_offset=4)
    assert torch.equal(a, torch.cat([lo, hi])) and lat_lo + lat_hi == lat_a          # two calls on 4 copies each
    c, lat_c = go(seed=8)
    assert len(set(lat_a)) > 1 and lat_c != lat_a and not torch.equal(a, c)          # the picks are draws
    # the bookkeeping's strings are the device's choices
    from disco_diffdock_amd.sampling import oracle_latents
    from disco_diffdock_amd.data import collate
    _, _, choices = oracle_latents(model, collate(_graphs(cplx, 0, N)), olr.SAMPLING_T, SEED)
    assert _picks(lat_a) == choices.cpu().tolist()
    out = _run(model, cplx, dev)[1]
    want = torch.as_tensor(cplx['rec_pos'])
    for d, row in zip(out, choices.cpu().tolist()):
        assert tuple(d.latent_pos.shape) == (2, 3)
        for j, idx in enumerate(row):
            if idx >= olr.COMPLEX['n_lig']:
                assert torch.allclose(d.latent_pos[j], want[idx - olr.COMPLEX['n_lig']].float() + d.original_center.reshape(3), atol=1e-6)


def test_missing_pose_or_name_says_what_is_needed(dev, model, cplx):
    graphs = _graphs(cplx, 0, 2)
    del graphs[0]['ligand'].__dict__['orig_pos_torch']
    with pytest.raises(RuntimeError, match='orig_pos_torch'):
        _run(model, cplx, dev, 0, 2, graphs=graphs)
    from disco_diffdock_amd.sampling import oracle_latents
    from disco_diffdock_amd.data import collate
    graphs = _graphs(cplx, 0, 2)
    for g in graphs:
        g.name = None
    with pytest.raises(RuntimeError, match='name'):
        oracle_latents(model, collate(graphs), olr.SAMPLING_T, SEED, rng_stream=5)


# ---- the latents -----------------------------------------------------------------------------------------------------------------------------------------------
def test_latents_are_the_encoder_and_the_ragged_op(dev, model, cplx):
    from disco_diffdock_amd.data import collate
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.sampling import oracle_latents
    n_l, n_r = olr.COMPLEX['n_lig'], len(cplx['rec_pos'])
    lat_l, lat_r, choices = oracle_latents(model, collate(_graphs(cplx, 0, N)), olr.SAMPLING_T, SEED, None, 0)
    assert tuple(lat_l.shape) == (N * n_l, 2) and tuple(lat_r.shape) == (N * n_r, 2) and tuple(choices.shape) == (N, 2)
    assert model.encoder.latent_temperature == olr.SAMPLING_T and not model.encoder.training
    one = collate(_graphs(cplx, 0, 1)).to(dev)
    with torch.no_grad():
        logit_l, logit_r, _, _ = model.encoder.logits(one)
    ctx = model.score_model.ctx
    ptr = lambda n: torch.tensor([0, n], dtype=torch.int64, device=dev)
    for b in range(N):
        out_l, out_r, _, _ = ctx.gumbel_softmax(logit_l, logit_r, ptr(n_l), ptr(n_r), olr.SAMPLING_T, SEED, [stream_id(cplx['name'])], sample=b, draw=0)
        assert torch.equal(_bits(lat_l[b * n_l:(b + 1) * n_l]), _bits(out_l)) and torch.equal(_bits(lat_r[b * n_r:(b + 1) * n_r]), _bits(out_r)), b
    # sample0 and the stream move the draws; the default stream is the name's
    again = oracle_latents(model, collate(_graphs(cplx, 0, 3)), olr.SAMPLING_T, SEED, stream_id(cplx['name']), 5)
    assert torch.equal(again[2], choices[5:8])
    assert not torch.equal(oracle_latents(model, collate(_graphs(cplx, 0, N)), olr.SAMPLING_T, SEED, 12345, 0)[2], choices)
    # against the fp64 restatement of the encoder and of the draw
    logits = olr.logits64(olr.host_encoder(), cplx)
    dev_logits = torch.cat([logit_l, logit_r]).cpu().numpy()
    err = rel_err(dev_logits, logits)
    print(f'oracle encoder logits, device against fp64: {err:.2e}')
    _record_drift('oracle_sampling.encoder_logits', err, bar=1e-4)
    assert err < 1e-4
    want, gaps = olr.host_picks(logits, SEED, stream_id(cplx['name']), 0, N)
    assert (gaps > olr.SAMPLING_GAP).all()      # (every case is held; tests/test_oracle_sampling_host.py shows it on the CPU)
    assert (choices.cpu().numpy() == want).all()


# ---- the trajectory ------------------------------------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_the_oracle_sampler(dev, model, cplx, weights, tables):
    """the seeded call's final poses against oracle.sampler_ref.sampling handed the same latents and the rows of ctx.rng_noise(7, ...): the project's 1e-4"""
    from disco_diffdock_amd.data import collate
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.sampling import oracle_latents, step_coefficients
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    sched = get_t_schedule(STEPS)
    got, _ = _run(model, cplx, dev)
    n_l, n_r = olr.COMPLEX['n_lig'], len(cplx['rec_pos'])
    lat_l, lat_r, _ = oracle_latents(model, collate(_graphs(cplx, 0, N)), olr.SAMPLING_T, SEED)
    lat_l, lat_r = lat_l.cpu().round(), lat_r.cpu().round()      # ((hard - y) + y is the one-hot to an ulp; the engine reads it as it is)
    _, _, nc = step_coefficients(STEPS, sched, sched, sched, partial(t_to_sigma, args=ARGS), ARGS, False, False, True, 1.0, 0.0, 0.5)
    R = int(np.asarray(cplx['edge_mask']).sum())
    z = model.score_model.ctx.rng_noise(SEED, stream_id(cplx['name']), 0, N, STEPS, 6 + R, noise_coeff=nc).cpu()
    dl = []
    for i, d in enumerate(_graphs(cplx, 0, N)):
        g = to_graph(cplx)
        g['ligand'].pos = d['ligand'].pos.clone()
        g['ligand'].latent_h, g['receptor'].latent_h = lat_l[i * n_l:(i + 1) * n_l], lat_r[i * n_r:(i + 1) * n_r]
        g['ligand'].unconditional, g['receptor'].unconditional = torch.zeros(n_l, 1), torch.zeros(n_r, 1)
        dl.append(g)
    nf = lambda b, t, name, shape: {'tr': z[t, :, 0:3], 'rot': z[t, :, 3:6], 'tor': z[t, :, 6:].reshape(-1)}[name]
    ref, _ = spr.sampling(dl, weights['P'], CFG, tables[0], tables[1], STEPS, sched, sched, sched, noise_fn=nf, batch_size=N, no_final_step_noise=True)
    ref = torch.stack([g['ligand'].pos for g in ref])
    err = rel_err(got, ref)
    print(f'oracle-latent sampling, {STEPS} steps, {N} samples: final poses against the oracle sampler {err:.2e}')
    _record_drift('oracle_sampling.final_poses', err, bar=1e-4)
    assert err < 1e-4


# ---- compute_ar_accuracy ---------------------------------------------------------------------------------------------------------------------------------------
def test_compute_ar_accuracy(dev, det_env, model, cplx):
    from disco_diffdock_amd.data import collate
    from disco_diffdock_amd.model_utils import get_ar_model
    from disco_diffdock_amd.sampling import oracle_latents
    ar_args = Namespace(use_pretrained_score=True, ns=16, latent_no_batchnorm=False, latent_dropout=0.0, latent_hidden_dim=128,
                        esm_embeddings_path='x', no_randomness=False)
    ar = get_ar_model(ar_args, ARGS, dev, training=False)
    ar.load_state_dict(ar_ref.random_ar_state_dict(CFG, seed=14))
    ar.eval()
    kw = dict(ar_model=ar, ar_args=ar_args, softmax_latent_temperature=1.0)
    plain, out_plain = _run(model, cplx, dev, **kw)
    assert all('ar_accuracy' not in d.__dict__ for d in out_plain)
    lat_plain = [d.latent_str for d in out_plain]
    flagged, out = _run(model, cplx, dev, compute_ar_accuracy=True, **kw)
    ar_choices = ar.last_choices.cpu()
    _, _, true_choices = oracle_latents(model, collate(_graphs(cplx, 0, N)), olr.SAMPLING_T, SEED)
    want = float((ar_choices[:, 0] == true_choices.cpu()[:, 0]).double().mean())
    assert [d.ar_accuracy for d in out] == [want] * N and 0.0 <= want <= 1.0
    assert torch.equal(plain, flagged) and [d.latent_str for d in out] == lat_plain and _picks(lat_plain) == ar_choices.tolist()      # the AR latents sample
    # per batch: with two batches of four each graph carries its own batch's share
    _, out4 = _run(model, cplx, dev, compute_ar_accuracy=True, batch_size=4, **kw)
    same = (ar_choices[:, 0] == true_choices.cpu()[:, 0]).double()
    assert [d.ar_accuracy for d in out4] == [float(same[:4].mean())] * 4 + [float(same[4:].mean())] * 4
