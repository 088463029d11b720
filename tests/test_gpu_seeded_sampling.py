"""Seeded sampling end to end (sampling(seed=...), randomize_position(seed=...), the seeded AR picks) on deterministic = 1 contexts: with the draws a pure
function of (seed, complex, global sample index, step, column) and the arithmetic independent of the batch around a sample, the POSES are the same bits
whatever the batch size and however the samples of a complex are spread over calls.  A small synthetic complex (40 residues, 22 ligand atoms, at least one
rotatable bond), 3 steps, 8 samples, random weights through the reference's call surface (get_model / get_ar_model)."""
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

import philox_ref as pr
from oracle import ar_ref
from oracle import score_model_ref as smr
from helpers import rel_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy

ARGS = Namespace(ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                 max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, embedding_scale=1000, embedding_type='sinusoidal',
                 scale_by_sigma=True, no_torsion=False, no_batch_norm=False, dropout=0.1, sh_lmax=1, use_second_order_repr=False,
                 use_old_atom_encoder=False, esm_embeddings_path='data/esm2_3billion_embeddings.pt', latent_dim=0, latent_vocab=64,
                 latent_cross_attention=False, tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55,
                 tor_sigma_min=0.03, tor_sigma_max=3.14)
STEPS, N = 3, 8


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def det_env():
    """every context made inside this module's fixtures is deterministic = 1 (the process-wide switch runtime.Context reads when it is created)"""
    mp = pytest.MonkeyPatch()
    mp.setenv('DDK_DETERMINISTIC', '1')
    yield
    mp.undo()


@pytest.fixture(scope='module')
def cplx():
    from disco_diffdock_amd import synthetic
    c = synthetic.make_complex(31, n_res=40, n_lig=22)
    assert int(np.asarray(c['edge_mask']).sum()) >= 1
    return c


@pytest.fixture(scope='module')
def model(dev, det_env):
    from disco_diffdock_amd.model_utils import get_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    m = get_model(ARGS, dev, partial(t_to_sigma, args=ARGS), no_parallel=True)
    m.score_model.load_state_dict(smr.random_state_dict(smr.ScoreModelConfig(latent_vocab=64), seed=7), strict=True)
    assert int(m.score_model.ctx.cfg.deterministic) == 1
    return m


def _graphs(c, lo, hi):
    """the copies with the global sample indices lo .. hi - 1, each at its own start pose (a fixed shift per global index)"""
    from disco_diffdock_amd.data import from_arrays
    shifts = np.random.default_rng(2).normal(0, 4.0, size=(N, 1, 3)).astype(np.float32)
    dl = [from_arrays(c) for _ in range(lo, hi)]
    for d, i in zip(dl, range(lo, hi)):
        d['ligand'].pos = T(np.asarray(c['lig_pos'], np.float32) + shifts[i]).float()
        d['ligand'].ar_pos = d['ligand'].pos.clone()
    return dl


def _run(model, c, dev, lo=0, hi=N, args=ARGS, **kw):
    from disco_diffdock_amd.sampling import sampling
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    sched = get_t_schedule(STEPS)
    kw.setdefault('batch_size', hi - lo)
    out, _ = sampling(_graphs(c, lo, hi), model, STEPS, sched, sched, sched, dev, partial(t_to_sigma, args=args), args, no_final_step_noise=True, **kw)
    return torch.stack([d['ligand'].pos for d in out]).cpu(), out


def test_seeded_sampling_is_reproducible_and_cut_invariant(dev, model, cplx):
    a, _ = _run(model, cplx, dev, seed=7)
    assert torch.isfinite(a).all()
    assert torch.equal(a, _run(model, cplx, dev, seed=7)[0])                               # twice
    assert torch.equal(a, _run(model, cplx, dev, seed=7, batch_size=4)[0])                 # batch size 8 vs 4
    lo = _run(model, cplx, dev, 0, 4, seed=7, sample_offset=0)[0]                          # two calls on 4 copies each
    hi = _run(model, cplx, dev, 4, 8, seed=7, sample_offset=4)[0]
    assert torch.equal(a, torch.cat([lo, hi]))
    assert not torch.equal(a, _run(model, cplx, dev, seed=8)[0])                           # another seed
    b = _run(model, cplx, dev, seed=7, rng_stream=12345)[0]                                # another stream
    assert not torch.equal(a, b)
    from disco_diffdock_amd.runtime import stream_id
    assert torch.equal(a, _run(model, cplx, dev, seed=7, rng_stream=stream_id(cplx['name']))[0])      # the default stream is the name's hash


def test_seeded_noise_is_what_the_sampler_consumed(dev, model, cplx):
    """the seeded call equals the unseeded one fed the generator's rows through noise=: the seed changes where the draws come from and nothing else"""
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.sampling import step_coefficients
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    sched = get_t_schedule(STEPS)
    _, _, nc = step_coefficients(STEPS, sched, sched, sched, partial(t_to_sigma, args=ARGS), ARGS, False, False, True, 1.0, 0.0, 0.5)
    R = int(np.asarray(cplx['edge_mask']).sum())
    z = model.score_model.ctx.rng_noise(7, stream_id(cplx['name']), 0, N, STEPS, 6 + R, noise_coeff=nc)
    assert bool((z[STEPS - 1] == 0).all()) and bool((z[:STEPS - 1] != 0).all())             # no_final_step_noise: the last step draws nothing
    assert torch.equal(_run(model, cplx, dev, seed=7)[0], _run(model, cplx, dev, noise=[z])[0])


def test_noise_together_with_seed_raises(dev, model, cplx):
    with pytest.raises(ValueError, match='noise'):
        _run(model, cplx, dev, seed=7, noise=[torch.zeros(STEPS, N, 6)])


def _randomized(c, dev, lo=0, hi=N, **kw):
    from disco_diffdock_amd.data import from_arrays
    from disco_diffdock_amd.sampling import randomize_position
    dl = [from_arrays(c) for _ in range(lo, hi)]
    randomize_position(dl, False, False, 19.0, device=dev, **kw)
    assert all(d['ligand'].pos.is_cuda for d in dl)
    return torch.stack([d['ligand'].pos for d in dl]).cpu(), dl


def test_seeded_randomize_position(dev, cplx):
    a, _ = _randomized(cplx, dev, seed=7)
    assert torch.equal(a, _randomized(cplx, dev, seed=7)[0])
    lo, hi = _randomized(cplx, dev, 0, 4, seed=7, sample_offset=0)[0], _randomized(cplx, dev, 4, 8, seed=7, sample_offset=4)[0]
    assert torch.equal(a, torch.cat([lo, hi]))
    assert torch.equal(a[2:5], _randomized(cplx, dev, 2, 5, seed=7, sample_offset=2)[0])      # any slice of the samples
    assert not torch.equal(a, _randomized(cplx, dev, seed=8)[0]) and not torch.equal(a, _randomized(cplx, dev, seed=7, rng_stream=12345)[0])
    # the poses are ddk_randomize_position's on the restatement's draws (that kernel's tolerance, tests/test_gpu_model.py::test_randomize_position_device)
    from disco_diffdock_amd.runtime import Complex, stream_id
    from disco_diffdock_amd.tensor_layers import _shape_context
    n_rot = int(np.asarray(cplx['edge_mask']).sum())
    tor, rot, tr = pr.initial(7, stream_id(cplx['name']), 0, N, n_rot, 19.0)
    cx = Complex(_shape_context(0), cplx, max_batch=N)
    want = cx.randomize_position(T(np.asarray(cplx['lig_pos'], np.float32)).to(dev), T(rot.astype(np.float32)).to(dev), T(tor).to(dev),
                                 T(tr.astype(np.float32)).to(dev))
    assert rel_err(a, want.cpu()) < 2e-6


def test_seeded_ar_rotation_is_purpose_5(dev, cplx):
    """ar_args.no_randomness: the pose the AR model sees is the centred conformer under the rotation of purpose 5, per global sample"""
    from disco_diffdock_amd.data import from_arrays
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.sampling import randomize_position
    ar_args = Namespace(no_randomness=True)
    conf = np.asarray(cplx['lig_pos'], np.float32) + 3.0

    def go(lo, hi):
        dl = [from_arrays(cplx) for _ in range(lo, hi)]
        for d in dl:
            d['ligand'].orig_rdkit_pos = [conf]
        randomize_position(dl, False, False, 19.0, ar_args=ar_args, device=dev, seed=7, sample_offset=lo)
        return torch.stack([d['ligand'].ar_pos for d in dl]).cpu()

    a = go(0, N)
    assert torch.equal(a[3:6], go(3, 6))
    rot5 = pr.initial(7, stream_id(cplx['name']), 0, N, 0, purpose_rot=5)[1]
    rot2 = pr.initial(7, stream_id(cplx['name']), 0, N, 0, purpose_rot=2)[1]
    centred = (conf - conf.mean(0, keepdims=True)).astype(np.float64)
    assert rel_err(a, centred[None] @ rot5.transpose(0, 2, 1)) < 2e-6
    assert rel_err(a, centred[None] @ rot2.transpose(0, 2, 1)) > 1e-2


def test_seeded_latent_sampling_with_ar_model(dev, det_env, cplx):
    """latent-conditioned sampling with an AR model at a temperature that draws (T = 1 < 100): the picks and the poses do not depend on the batch split"""
    from disco_diffdock_amd.model_utils import get_model, get_ar_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    score_args = Namespace(**dict(vars(ARGS), latent_dim=2, latent_vocab=1, latent_droprate=0.1))
    ar_args = Namespace(use_pretrained_score=True, ns=16, latent_no_batchnorm=False, latent_dropout=0.0, latent_hidden_dim=128,
                        esm_embeddings_path='x', no_randomness=False)
    cfg = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    m = get_model(score_args, dev, partial(t_to_sigma, args=score_args), no_parallel=True)
    m.score_model.load_state_dict(smr.random_state_dict(cfg, seed=13))
    ar = get_ar_model(ar_args, score_args, dev, training=False)
    ar.load_state_dict(ar_ref.random_ar_state_dict(cfg, seed=14))
    ar.eval()
    assert int(m.score_model.ctx.cfg.deterministic) == 1 and int(ar.pretrained_score_model.ctx.cfg.deterministic) == 1
    kw = dict(args=score_args, ar_model=ar, ar_args=ar_args, softmax_latent_temperature=1.0, seed=7)

    def go(lo=0, hi=N, **extra):
        pos, out = _run(m, cplx, dev, lo, hi, **dict(kw, **extra))
        last = ar.last_choices.cpu()
        return pos, [d.latent_str for d in out], last

    a, lat_a, ch_a = go()
    assert tuple(ch_a.shape) == (N, 2) and int(ch_a.min()) >= 0
    b, lat_b, ch_b = go(batch_size=4)
    assert lat_a == lat_b and torch.equal(ch_a[4:], ch_b) and torch.equal(a, b)
    lo, lat_lo, ch_lo = go(0, 4, sample_offset=0)
    hi, lat_hi, ch_hi = go(4, 8, sample_offset=4)
    assert lat_lo + lat_hi == lat_a and torch.equal(torch.cat([ch_lo, ch_hi]), ch_a) and torch.equal(torch.cat([lo, hi]), a)
    assert len(set(lat_a)) > 1 or not torch.equal(a, go(seed=8)[0])      # the picks are draws: they differ between samples, or at least between seeds


def test_unseeded_paths_never_touch_the_generator(dev, model, cplx, monkeypatch):
    """seed=None: sampling(), randomize_position() and encode_ar() draw exactly as before; the new entry points are not called"""
    from disco_diffdock_amd.runtime import Context

    def boom(*a, **k):
        raise AssertionError('a ddk_rng_* call on an unseeded path')
    for name in ('rng_noise', 'rng_initial', 'rng_uniform'):
        monkeypatch.setattr(Context, name, boom)
    for name in ('ddk_rng_noise', 'ddk_rng_initial', 'ddk_rng_uniform'):
        monkeypatch.setattr(model.score_model.ctx.L, name, boom)
    torch.manual_seed(0)
    np.random.seed(0)
    a, _ = _run(model, cplx, dev)
    assert torch.isfinite(a).all()
    p, _ = _randomized(cplx, dev)
    assert torch.isfinite(p).all()
    with pytest.raises(AssertionError, match='unseeded'):
        _run(model, cplx, dev, seed=7)
