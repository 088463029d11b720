"""training.test_epoch and training.inference_epoch on the device: three synthetic complexes (30-40 residues, 12-22 ligand atoms), a
TrainableScoreModel of four conv layers with and without the oracle encoder in front (train_model.LatentModelWrapper), random-init weights.

The Gumbel draw of test_epoch's step k follows ``_step_seed(seed, epoch, k)``, so the wrapper's numbers are a function of the batch size as well (a complex
meets another step, hence another draw); the comparison of batch sizes 3 and 1 is therefore made on the plain score model, whose evaluation forward treats
every graph by itself: the two runs differ by the summation order of the library GEMMs inside the heads, 1e-5 relative at most."""
import copy
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ARGS = Namespace(ns=24, nv=6, num_conv_layers=4, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                 max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, embedding_scale=1000, embedding_type='sinusoidal',
                 scale_by_sigma=True, no_torsion=False, no_batch_norm=False, dropout=0.1, sh_lmax=1, use_second_order_repr=False,
                 use_old_atom_encoder=False, esm_embeddings_path='data/esm2_3billion_embeddings.pt', latent_dim=2, latent_vocab=1, latent_droprate=0.1,
                 latent_cross_attention=False, tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55,
                 tor_sigma_min=0.03, tor_sigma_max=3.14, encoder_ns=24, encoder_nv=4, encoder_num_conv_layers=3, encoder_cross_max_distance=80,
                 training_latent_temperature=1.0, inference_steps=2, sampling_latent_temperature=0.01)
PLAIN = Namespace(**dict(vars(ARGS), latent_dim=0, latent_droprate=0.0))
COMPLEXES = ((70, 32, 12), (71, 36, 16), (60, 40, 22))      # (seed, residues, ligand atoms)
SEED, EPOCH = 7, 3


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
def complexes():
    from disco_diffdock_amd import synthetic
    cs = [synthetic.make_complex(seed, n_res=n_res, n_lig=n_lig) for seed, n_res, n_lig in COMPLEXES]
    for c in cs:
        assert 20 <= len(c['rec_pos']) <= 40 and 8 <= len(c['lig_pos']) <= 22 and int(np.asarray(c['edge_mask']).sum()) >= 1
    assert len({c['name'] for c in cs}) == 3
    return cs


def _model(dev, args, seed=5):
    from disco_diffdock_amd.model_utils import get_trainable_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    torch.manual_seed(seed)
    return get_trainable_model(args, dev, partial(t_to_sigma, args=args))


@pytest.fixture(scope='module')
def models(dev, det_env):
    return dict(plain=_model(dev, PLAIN), latent=_model(dev, ARGS))


def _by_hand(model, cs, batch_size, seed, epoch, plain_forward=False):
    """the loop test_epoch stands for: -> (the seven means, the per-complex rows [n, 7], the times).  ``plain_forward``: the evaluation forward as
    ``model.eval()`` alone gives it (the conv layers on the fused inference kernel), without test_epoch's switch to the ops without atomics"""
    import contextlib
    from disco_diffdock_amd import training
    from disco_diffdock_amd.train_model import LatentModelWrapper
    model.eval()
    times = training.draw_times([c['name'] for c in cs], seed, draw=epoch)
    rows = []
    with torch.no_grad(), (contextlib.nullcontext() if plain_forward else training.reproducible_evaluation(model)):
        for k, at in enumerate(range(0, len(cs), batch_size)):
            part = cs[at:at + batch_size]
            data, targets = training.noise_batch(model, part, times[at:at + batch_size], seed, draw=epoch)
            kw = dict(seed=training._step_seed(seed, epoch, k))
            if isinstance(model, LatentModelWrapper) and model.latent_droprate > 0:
                kw['keep'] = training.draw_latent_keep(part, model.latent_droprate, seed, epoch)
            tr, rot, tor = model(data, **kw)
            out = training.loss_function(tr, rot, tor, targets, model, apply_mean=False)
            rows.append(torch.stack([v.double().reshape(-1) for v in out], dim=1).cpu().numpy())
    rows = np.concatenate(rows)
    return dict(zip(training.TRAIN_METERS, rows.mean(axis=0).tolist())), rows, np.asarray(times, np.float64)


@pytest.mark.parametrize('kind', ['plain', 'latent'])
def test_test_epoch_is_the_loop_by_hand(dev, models, complexes, kind):
    from disco_diffdock_amd import training
    model = models[kind].train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    got = training.test_epoch(model, complexes, 2, SEED, epoch=EPOCH)      # batches of two graphs and of one
    assert not model.training and all(p.grad is None for p in model.parameters())
    for k, v in model.state_dict().items():      # neither a parameter nor a BatchNorm statistic moved
        assert torch.equal(v, before[k]), k
    want, rows, _ = _by_hand(model, complexes, 2, SEED, EPOCH)
    assert list(got) == list(training.TRAIN_METERS) and got == want and all(np.isfinite(v) for v in got.values())
    assert got == training.test_epoch(model, complexes, 2, SEED, epoch=EPOCH) and want == _by_hand(model, complexes, 2, SEED, EPOCH)[0]      # twice
    assert got != training.test_epoch(model, complexes, 2, SEED, epoch=EPOCH + 1) and got != training.test_epoch(model, complexes, 2, SEED + 1, epoch=EPOCH)
    assert abs(got['loss'] - (got['tr_loss'] + got['rot_loss'] + got['tor_loss'])) < 1e-6 * abs(got['loss'])
    assert all(np.isnan(v) for v in training.test_epoch(model, [], 2, SEED).values())


@pytest.mark.parametrize('kind', ['plain', 'latent'])
def test_test_epoch_against_the_plain_evaluation_forward(dev, models, complexes, kind):
    """test_epoch's route (conv layers on the training ops in .eval()) against the loop on the plain .eval() forward, whose conv layers run the fused
    inference kernel: the same BatchNorm buffers, no dropout, the same Gumbel draw, so the two differ by arithmetic alone.  The inference kernel multiplies
    its radial-MLP GEMMs as two f16 limbs (<= 3 * 2^-22 = 7e-7 relative per product) where the training ops take fp32 inputs, and it
    scatters in the order of its atomics; over four layers that is a few 1e-6 on a prediction, and a loss term, a square of prediction minus target,
    carries twice that.  Bar: 1e-5 relative per meter, the bar the tensor-product ops carry per block.  The base losses do not read the predictions."""
    from disco_diffdock_amd import training
    from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures
    model = models[kind]
    layers = [m for m in model.modules() if hasattr(m, 'eval_with_training_ops')]
    assert layers and not any(m.eval_with_training_ops for m in layers)      # off by default, and put back by test_epoch
    got = training.test_epoch(model, complexes, 2, SEED, epoch=EPOCH)
    assert not any(m.eval_with_training_ops for m in layers)
    want, rows, _ = _by_hand(model, complexes, 2, SEED, EPOCH, plain_forward=True)
    sure, sure_rows, _ = _by_hand(model, complexes, 2, SEED, EPOCH)
    worst = 0.0
    for k in training.TRAIN_METERS:
        err = abs(got[k] - want[k]) / abs(want[k])
        print(f'{kind} {k}: test_epoch {got[k]:.9g}, plain evaluation forward {want[k]:.9g}, relative {err:.2e}')
        _record_drift(f'test_epoch.plain_forward.{kind}.{k}', err, bar=1e-5)
        worst = max(worst, err)
    assert worst < 1e-5
    assert np.abs(sure_rows - rows).max() <= 1e-5 * np.abs(rows).max()      # per complex too
    for k in ('tr_base_loss', 'rot_base_loss', 'tor_base_loss'):
        assert got[k] == want[k]


def test_wrapper_rows_do_not_depend_on_the_batch(dev, models, complexes):
    """test_epoch gives step k its own Gumbel seed, so its wrapper numbers move with the batch size by construction.  With ONE seed for every call (the
    Gumbel noise is then a function of the complex alone) and every latent kept, a complex's seven loss values are the same in a batch of three and alone,
    to the 1e-5 of test_batch_size_three_against_one"""
    from disco_diffdock_amd import training
    model = models['latent'].eval()
    times = training.draw_times([c['name'] for c in complexes], SEED, draw=EPOCH)

    def rows(part, t):
        data, targets = training.noise_batch(model, part, t, SEED, draw=EPOCH)
        tr, rot, tor = model(data, seed=12345, keep=np.ones(len(part), np.float32))
        out = training.loss_function(tr, rot, tor, targets, model, apply_mean=False)
        return torch.stack([v.double().reshape(-1) for v in out], dim=1).cpu().numpy()

    with torch.no_grad(), training.reproducible_evaluation(model):
        together = rows(complexes, times)
        alone = np.concatenate([rows([c], times[i:i + 1]) for i, c in enumerate(complexes)])
    err = np.abs(together - alone) / np.abs(alone)
    print('wrapper rows, batch of three against alone: relative', err.max())
    assert np.isfinite(alone).all() and err.max() <= 1e-5


def test_batch_size_three_against_one(dev, models, complexes):
    from disco_diffdock_amd import training
    a, b = (training.test_epoch(models['plain'], complexes, bs, SEED, epoch=EPOCH) for bs in (3, 1))
    for k in training.TRAIN_METERS:
        print(f'{k}: batch size 3 {a[k]:.9g}, 1 {b[k]:.9g}')
        assert abs(a[k] - b[k]) <= 1e-5 * abs(b[k]), k


@pytest.mark.parametrize('kind', ['plain', 'latent'])
def test_sigma_intervals(dev, models, complexes, kind):
    from disco_diffdock_amd import training
    got = training.test_epoch(models[kind], complexes, 2, SEED, epoch=EPOCH, test_sigma_intervals=True)
    want, rows, times = _by_hand(models[kind], complexes, 2, SEED, EPOCH)
    assert len(got) == 7 + 70 and {k: got[k] for k in training.TRAIN_METERS} == want
    interval = np.floor(10 * times).astype(int)
    for i in range(10):
        for j, name in enumerate(training.TRAIN_METERS):
            v = got[f'int{i}_{name}']
            if (interval == i).any():
                assert v == float(rows[interval == i, j].mean())
            else:
                assert np.isnan(v)
    assert sum((interval == i).any() for i in range(10)) >= 1


# ---- inference_epoch -------------------------------------------------------------------------------------------------------------------------------------------
def _sample_by_hand(engine, cs, args, seed, epoch, dev):
    from disco_diffdock_amd import training
    from disco_diffdock_amd.data import from_arrays
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    from disco_diffdock_amd.sampling import randomize_position, sampling
    sched = get_t_schedule(inference_steps=args.inference_steps)
    out, out64 = [], []
    for i, c in enumerate(cs):
        s = training._step_seed(seed, epoch, i)
        g = from_arrays(c)
        g['ligand'].orig_pos_torch = torch.as_tensor(np.asarray(c['lig_pos'], np.float32))
        dl = [g]
        randomize_position(dl, args.no_torsion, False, args.tr_sigma_max, device=dev, seed=s)
        dl, _ = sampling(dl, engine, args.inference_steps, sched, sched, sched, dev, partial(t_to_sigma, args=args), args, batch_size=1,
                         use_latent=args.latent_dim > 0, ar_model=None, seed=s, gumbel_latent_temperature=args.sampling_latent_temperature)
        pos = dl[0]['ligand'].pos
        true = torch.as_tensor(np.asarray(c['lig_pos'], np.float32)).to(dev)
        heavy = torch.as_tensor((np.asarray(c['lig_x'])[:, 0] != 0).astype(np.float32)).to(dev)
        out.append(float((((((pos - true) ** 2).sum(dim=1) * heavy).sum() / heavy.sum()).sqrt()).double()))
        keep = np.asarray(c['lig_x'])[:, 0] != 0
        out64.append(float(np.sqrt(((pos.cpu().numpy().astype(np.float64)[keep] - np.asarray(c['lig_pos'], np.float64)[keep]) ** 2).sum(1).mean())))
    return np.array(out), np.array(out64)


def test_inference_epoch(dev, det_env, models, complexes):
    from disco_diffdock_amd import training
    model = models['latent']
    start = copy.deepcopy(model.state_dict())
    engine = training.inference_engine(model, ARGS)
    assert int(engine.score_model.ctx.cfg.deterministic) == 1 and engine.encoder is not None and not engine.encoder.training
    for k, v in model.encoder.state_dict().items():
        assert torch.equal(engine.encoder.state_dict()[k], v), k
    first = training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH, engine=engine)
    r = first['rmsds']
    assert r.shape == (3,) and r.dtype == np.float64 and np.isfinite(r).all() and (r > 0).all()
    assert first['rmsds_lt2'] == 100 * (r < 2).sum() / 3 and first['rmsds_lt5'] == 100 * (r < 5).sum() / 3 and set(first) == {'rmsds_lt2', 'rmsds_lt5', 'rmsds'}
    hand, hand64 = _sample_by_hand(engine, complexes, ARGS, SEED, EPOCH, dev)
    print('rmsds', r, 'by hand', hand, 'fp64 on the host', hand64)
    assert (r == hand).all()                                            # the composition, bit for bit
    assert np.abs(r - hand64).max() <= 1e-5 * hand64.max()               # and the RMSD it is meant to be
    again = training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH, engine=engine)
    fresh = training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH)      # an engine of its own
    assert (again['rmsds'] == r).all() and (fresh['rmsds'] == r).all()
    assert not (training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH + 1, engine=engine)['rmsds'] == r).all()
    assert not (training.inference_epoch(model, complexes, ARGS, SEED + 1, epoch=EPOCH, engine=engine)['rmsds'] == r).all()
    # one Adam step: the SAME engine must sample with the new weights (an engine that kept the old ones, or complexes set up with them, repeats r)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    data, targets = training.noise_batch(model, complexes, [0.3, 0.5, 0.7], SEED, draw=0)
    opt.zero_grad()
    tr, rot, tor = model(data, seed=1, keep=np.ones(3, np.float32))
    training.loss_function(tr, rot, tor, targets, model)[0].sum().backward()
    opt.step()
    moved = training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH, engine=engine)['rmsds']
    assert np.isfinite(moved).all() and not (moved == r).any()
    model.load_state_dict(start, strict=True)
    back = training.inference_epoch(model, complexes, ARGS, SEED, epoch=EPOCH, engine=engine)['rmsds']
    assert (back == r).all()


def test_inference_epoch_without_latents(dev, det_env, models, complexes):
    from disco_diffdock_amd import training
    a = training.inference_epoch(models['plain'], complexes, PLAIN, SEED, epoch=EPOCH)
    assert np.isfinite(a['rmsds']).all() and a['rmsds'].shape == (3,)
    engine = training.inference_engine(models['plain'], PLAIN)
    assert getattr(engine, 'encoder', None) is None
    assert (training.inference_epoch(models['plain'], complexes, PLAIN, SEED, epoch=EPOCH, engine=engine)['rmsds'] == a['rmsds']).all()
