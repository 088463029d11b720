"""GPU tests of the trainable AR latent model (pretrained_score_encoder.TrainablePretrainedScoreEncoder, ar_training) on the three complexes of
tests/test_gpu_train_model.py, over the DisCo score model of tests/test_gpu_train_latent_model.py (latent_dim=2, latent_vocab=1, latent_droprate=0.1).

(a) the logits and the gradient of EVERY parameter against fp64 autograd through oracle.score_model_ref.embed (t = 1, unconditional = 1, latent_h =
    input_latent) plus the predictors restated here, without BatchNorm and dropout; the functional is sum(logits * w) with fixed random w.  The input latent
    is partially decoded: graph 0 at decoding index 0 (all zeros), graphs 1 and 2 at index 1 (column 0 holds a one-hot: a ligand atom in graph 1, a residue
    in graph 2).  Bars as in tests/test_gpu_train_latent_model.py (a): forward 1e-4; a gradient passes under max(4 * err32, 1e-5), err32 the oracle's own
    fp32 run against its fp64 run.  The ReLU clearance (the smallest |pre-activation| over the rms fp32-against-fp64 difference of its tensor) is asserted
    FIRST, from the oracle alone: >= 8, the predictors' two ReLUs per side included.  The weights are random_state_dict(cfg, seed=WEIGHT_SEED) and
    _predictor_weights(WEIGHT_SEED): a search on the CPU over seeds 1, 2, ... (clearance_of below) stops at seed 2 with a clearance of 16.4, tightest at
    conv_layers.1.fc.2 (the predictors' four ReLUs stay above 900); seed 1 reaches 5.7.  The oracle's fp32 run depends on the host's BLAS, so the figure
    moves a little between hosts.
(b) the round trip: .eval() logits on two copies of one complex with a partially decoded latent against get_ar_model(training=False) loaded from this
    module's state_dict (its logits()), 1e-4.
(c) with BatchNorm and dropout 0.1: two Adam steps of train_ar_epoch from one state and one seed give identical bits in every parameter and meter; the
    loss's gradient reaches both predictors and every score-model parameter; with the score model frozen only predictor parameters change.
(d) test_ar_epoch's accuracy equals a per-graph torch recomputation.
(e) make_latent_labels twice gives identical tables, each column a one-hot over the graph."""
import copy
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_radial_conv import _bits
from test_gpu_round3 import _record_drift
from test_gpu_train_model import COMPLEXES, MODEL, _batch

pytestmark = pytest.mark.gpu
LATENT = dict(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
AR_NS, HIDDEN = 16, 64
WEIGHT_SEED = 2      # clearance 16.4: see the module docstring
# every parameter the AR model's forward runs: the predictors and what TrainableScoreModel.embed runs of the score model (its heads stay unused, as in the reference)
EMBED_PARAMETERS = ('latent_s_predictor.', 'latent_r_predictor.') + tuple(
    'pretrained_score_model.' + k for k in ('lig_node_embedding.', 'rec_node_embedding.', 'lig_edge_embedding.', 'rec_edge_embedding.', 'cross_edge_embedding.',
                                            'conv_layers.', 'lig_node_unconditional', 'rec_node_unconditional', 'lig_edge_unconditional',
                                            'rec_edge_unconditional', 'cross_edge_unconditional'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _predictor_weights(seed, batchnorm):
    """the two predictors under the reference's keys: uniform(-1, 1) / sqrt(fan-in), and BatchNorm statistics away from the identity"""
    g = torch.Generator().manual_seed(1000 + seed)
    P = {}
    for name in ('latent_s_predictor', 'latent_r_predictor'):
        for i, (o, n_in) in ((0, (HIDDEN, 2 * AR_NS)), (4, (HIDDEN, HIDDEN)), (8, (1, HIDDEN))):
            P[f'{name}.{i}.weight'] = (torch.rand(o, n_in, generator=g) * 2 - 1) / math.sqrt(n_in)
            P[f'{name}.{i}.bias'] = (torch.rand(o, generator=g) * 2 - 1) / math.sqrt(n_in)
        if batchnorm:
            for i in (1, 5):
                P[f'{name}.{i}.weight'], P[f'{name}.{i}.bias'] = torch.rand(HIDDEN, generator=g) + 0.5, torch.randn(HIDDEN, generator=g) * 0.1
                P[f'{name}.{i}.running_mean'], P[f'{name}.{i}.running_var'] = torch.randn(HIDDEN, generator=g) * 0.1, torch.rand(HIDDEN, generator=g) + 0.5
                P[f'{name}.{i}.num_batches_tracked'] = torch.tensor(7)
    return P


def _input_latents(b):
    """graph 0: zeros (decoding index 0); graphs 1, 2: column 0 a one-hot, on ligand atom 3 of graph 1 and residue 5 of graph 2 (decoding index 1)"""
    lig_batch, rec_batch = b['ligand'].batch.long(), b['receptor'].batch.long()
    lat_l, lat_r = torch.zeros(lig_batch.shape[0], 2, dtype=torch.float64), torch.zeros(rec_batch.shape[0], 2, dtype=torch.float64)
    lat_l[int((lig_batch == 1).nonzero()[0]) + 3, 0] = 1
    lat_r[int((rec_batch == 2).nonzero()[0]) + 5, 0] = 1
    return lat_l, lat_r


def _prepared(batch, dtype):
    """the batch as PretrainedScoreEncoder.forward hands it to embed: latent_h = input_latent, unconditional = 1, t = 1 everywhere"""
    b = copy.deepcopy(batch)
    lat_l, lat_r = _input_latents(b)
    b['ligand'].latent_h, b['receptor'].latent_h = lat_l.to(dtype), lat_r.to(dtype)
    b['ligand'].unconditional, b['receptor'].unconditional = torch.ones(lat_l.shape[0], 1, dtype=dtype), torch.ones(lat_r.shape[0], 1, dtype=dtype)
    B = int(b.num_graphs)
    b.complex_t = {k: torch.ones(B) for k in ('tr', 'rot', 'tor')}
    for nt in ('ligand', 'receptor'):
        b[nt].node_t = {k: b.complex_t[k][b[nt].batch] for k in ('tr', 'rot', 'tor')}
        b[nt].pos = b[nt].pos.to(dtype)
    return b


def _oracle(cfg, P, Q, batch, dtype, grads=True):
    """fp autograd through the oracle's embed and the restated predictors (Linear, ReLU, Linear, ReLU, Linear): the logits, every gradient, and every
    pre-activation in front of a ReLU"""
    Pd = {k: (v.detach().to(dtype).requires_grad_(grads) if v.is_floating_point() else v) for k, v in P.items()}
    Qd = {k: v.detach().to(dtype).requires_grad_(grads) for k, v in Q.items()}
    b = _prepared(batch, dtype)
    out = smr.embed(Pd, cfg, b, dtype, True)
    lig, rec, g = out[0], out[1], out[-1]
    pre = {}
    lin = lambda row, name: row @ Pd[f'{name}.weight'].T + Pd[f'{name}.bias']
    latent_h = (b['ligand'].latent_h, b['receptor'].latent_h)
    lg, rc = smr.build_lig_conv_graph(b, cfg, latent_h, dtype), smr.build_rec_conv_graph(b, cfg, latent_h, dtype)
    tr_sigma = smr.t_to_sigma(*[b.complex_t[k] for k in ('tr', 'rot', 'tor')], cfg)[0]
    cross = smr.build_cross_conv_graph(b, cfg, (tr_sigma * 3 + 20).unsqueeze(1).to(dtype), lg[4], latent_h, dtype)
    for name, row in (('lig', lg[2]), ('rec', rc[2]), ('cross', cross[1])):
        pre[f'{name}_edge_embedding'] = lin(row, f'{name}_edge_embedding.0')
    ei, offs = g['edge_index'], (0,) + tuple(g['splits']) + (g['edge_index'].shape[1],)
    for l in range(cfg.num_conv_layers):
        x = g['x0'] if l == 0 else g['layers'][l - 1]
        ea = torch.cat([g['edge_emb'], x[ei[0], :cfg.ns], x[ei[1], :cfg.ns]], -1)
        for grp in range(4):
            pre[f'conv_layers.{l}.fc.{grp}'] = lin(ea[offs[grp]:offs[grp + 1]], f'conv_layers.{l}.fc.{grp}.0')
    logits = []
    for name, x in (('latent_s_predictor', lig), ('latent_r_predictor', rec)):
        h = torch.cat([x[:, :AR_NS], x[:, -AR_NS:]], 1)
        for i in (0, 4):
            p = h @ Qd[f'{name}.{i}.weight'].T + Qd[f'{name}.{i}.bias']
            pre[f'{name}.{i}'] = p
            h = torch.relu(p)
        logits.append(h @ Qd[f'{name}.8.weight'].T + Qd[f'{name}.8.bias'])
    got = dict(logits=[v.detach().double().numpy() for v in logits], pre={k: v.detach().double() for k, v in pre.items()})
    if grads:
        w = _functional(logits[0].shape[0], logits[1].shape[0])
        sum((o.double() * f).sum() for o, f in zip(logits, w)).backward()
        got['grads'] = {'pretrained_score_model.' + k: v.grad.double().numpy() for k, v in Pd.items() if v.is_floating_point() and v.grad is not None}
        got['grads'].update({k: v.grad.double().numpy() for k, v in Qd.items()})
    return got


def _functional(n_l, n_r, seed=23):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 1, generator=gen, dtype=torch.float64) for n in (n_l, n_r)]


def clearance_of(seed):
    """the ReLU clearance of weight seed ``seed``, from the oracle alone: name -> min |pre-activation| / rms(fp32 - fp64) of its tensor"""
    cfg = smr.ScoreModelConfig(batch_norm=False, **LATENT)
    P, Q = smr.random_state_dict(cfg, seed=seed), _predictor_weights(seed, False)
    _, b = _batch()
    p64, p32 = _oracle(cfg, P, Q, b, torch.float64, grads=False)['pre'], _oracle(cfg, P, Q, b, torch.float32, grads=False)['pre']
    return {k: float(p64[k].abs().min() / (p32[k] - p64[k]).pow(2).mean().sqrt()) for k in p64}


@pytest.fixture(scope='module')
def parity_reference():
    """computed once: the oracle in fp64 and in fp32, and the ReLU clearance"""
    cfg = smr.ScoreModelConfig(batch_norm=False, **LATENT)
    P, Q = smr.random_state_dict(cfg, seed=WEIGHT_SEED), _predictor_weights(WEIGHT_SEED, False)
    _, b = _batch()
    r64, r32 = _oracle(cfg, P, Q, b, torch.float64), _oracle(cfg, P, Q, b, torch.float32)
    clearance = {k: float(r64['pre'][k].abs().min() / (r32['pre'][k] - r64['pre'][k]).pow(2).mean().sqrt()) for k in r64['pre']}
    return dict(cfg=cfg, P=P, Q=Q, r64=r64, r32=r32, clearance=clearance, hidden_units=sum(v.numel() for v in r64['pre'].values()))


def _score_model(dev, P=None, **kw):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    model = TrainableScoreModel(**dict(MODEL, **LATENT, **kw))
    if P is not None:
        model.load_state_dict({k: v for k, v in P.items() if k in model.state_dict()}, strict=True)
    return model.to(dev)


def _ar_model(dev, P=None, Q=None, latent_no_batchnorm=False, latent_dropout=0.0, **kw):
    from disco_diffdock_amd.pretrained_score_encoder import TrainablePretrainedScoreEncoder
    ar = TrainablePretrainedScoreEncoder(_score_model(dev, P, **kw), ns=AR_NS, latent_dim=1, latent_vocab=1, latent_no_batchnorm=latent_no_batchnorm,
                                         latent_dropout=latent_dropout, latent_hidden_dim=HIDDEN, input_latent_dim=2, apply_gumbel_softmax=False)
    if Q is not None:
        missing, unexpected = ar.load_state_dict(Q, strict=False)
        assert not unexpected and all(k.startswith('pretrained_score_model.') for k in missing)
    return ar.to(dev)


# ---- (a) gradient parity with the oracle ---------------------------------------------------------------------------------------------------------------------
def test_gradient_parity_with_the_oracle(dev, parity_reference):
    r = parity_reference
    tight = min(r['clearance'], key=r['clearance'].get)
    print(f"{r['hidden_units']} hidden units, the closest to the kink: {tight} at {r['clearance'][tight]:.1f} rms fp32 differences")
    assert sum(k.startswith('latent_') for k in r['clearance']) == 4      # the predictors' two ReLUs per side are in the clearance
    assert r['clearance'][tight] >= 8, (tight, r['clearance'][tight])
    model = _ar_model(dev, r['P'], r['Q'], latent_no_batchnorm=True, batch_norm=False, dropout=0.0).train()
    _, b = _batch()
    lat_l, lat_r = _input_latents(b)
    b = b.to(dev)
    b['ligand'].input_latent, b['receptor'].input_latent = lat_l.float().to(dev), lat_r.float().to(dev)
    pred = model(b)
    assert tuple(pred.logit_l.shape) == (lat_l.shape[0], 1) and tuple(pred.logit_r.shape) == (lat_r.shape[0], 1)
    w = _functional(lat_l.shape[0], lat_r.shape[0])
    sum((o.double() * f.to(dev)).sum() for o, f in zip((pred.logit_l, pred.logit_r), w)).backward()
    for name, a, want, w32 in zip(('logit_l', 'logit_r'), (pred.logit_l, pred.logit_r), r['r64']['logits'], r['r32']['logits']):
        err, err32 = rel_err(a.detach().cpu().numpy(), want), rel_err(w32, want)
        print(f'forward {name}: device {err:.2e}, host fp32 {err32:.2e}')
        _record_drift(f'train_ar.forward.{name}', err, host_fp32=err32, bar=1e-4)
        assert err < 1e-4, (name, err)
    # the reference's list of per-graph [1, 1, n_g] tensors
    parts = model.logit_list(pred)
    n_l, n_r = torch.bincount(b['ligand'].batch).tolist(), torch.bincount(b['receptor'].batch).tolist()
    assert [tuple(p.shape) for p in parts] == [(1, 1, a + c) for a, c in zip(n_l, n_r)]
    assert torch.equal(parts[1][0, 0, :n_l[1]], pred.logit_l[n_l[0]:n_l[0] + n_l[1], 0])
    failures = []
    g64, g32 = r['r64']['grads'], r['r32']['grads']
    reached = 0
    for k, p in model.named_parameters():
        if not p.numel():
            continue
        if k not in g64:      # the score heads' parameters: embed() does not run them, in the oracle as here
            assert not k.startswith(EMBED_PARAMETERS) and p.grad is None, k
            continue
        assert k.startswith(EMBED_PARAMETERS) and p.grad is not None, k
        reached += 1
        want = g64[k]
        if not want.any():      # (what nothing downstream of the last conv layer's scalar columns reads)
            assert not bool(p.grad.any()), k
            continue
        err, err32 = rel_err(p.grad.cpu().numpy(), want), rel_err(g32[k], want)
        bar = max(4 * err32, 1e-5)
        print(f'{k}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record_drift(f'train_ar.grad.{k}', err, host_fp32=err32, bar=bar)
        if not err < bar:
            failures.append((k, err, err32, bar))
    assert not failures, failures
    assert reached == len(g64)      # every tensor the oracle differentiates is a parameter here


# ---- (b) round trip to the inference class ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_to_the_inference_class(dev):
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.model_utils import get_ar_model
    from test_gpu_model import ARGS_S, _dev_batch
    score_args = Namespace(**dict(vars(ARGS_S), **LATENT))
    ar_args = Namespace(use_pretrained_score=True, ns=AR_NS, latent_no_batchnorm=False, latent_dropout=0.1, latent_hidden_dim=HIDDEN)
    cfg = smr.ScoreModelConfig(**LATENT)
    trainable = _ar_model(dev, smr.random_state_dict(cfg, seed=9), _predictor_weights(9, True), latent_dropout=0.1, dropout=0.1).eval()
    engine = get_ar_model(ar_args, score_args, dev, training=False).eval()
    assert set(trainable.state_dict()) == {'pretrained_score_model.' + k for k in engine.pretrained_score_model.expected_state_dict_spec()} | set(engine.predictor_spec())
    engine.load_state_dict(trainable.state_dict(), strict=True)
    back = get_ar_model(ar_args, score_args, dev, training=True)      # and the reverse direction: the trainable class takes the same keys
    back.load_state_dict(trainable.state_dict(), strict=True)
    assert not back.apply_gumbel_softmax
    c = synthetic.make_complex(71, n_res=28, n_lig=12)
    n_lig, n_rec, B = len(c['lig_pos']), len(c['rec_pos']), 2
    rng = np.random.default_rng(3)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 1.5, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(B)]).astype(np.float32)
    lat = np.zeros((B, n_lig + n_rec, 2), np.float32)      # copy 0 decoded one latent on a ligand atom, copy 1 on a residue; the second column is still open
    lat[0, 2, 0] = lat[1, n_lig + 7, 0] = 1
    b = _dev_batch(c, B, pos, dev, 1.0)
    b['ligand'].input_latent = torch.from_numpy(lat[:, :n_lig].reshape(-1, 2).copy()).to(dev)
    b['receptor'].input_latent = torch.from_numpy(lat[:, n_lig:].reshape(-1, 2).copy()).to(dev)
    want = engine.logits(b)      # [B, 1, n_lig + n_rec]
    with torch.no_grad():
        pred = trainable(b)
    got = torch.stack([p[0] for p in trainable.logit_list(pred)])
    err = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print(f'round trip: {err:.2e}')
    _record_drift('train_ar.round_trip', err, bar=1e-4)
    assert err < 1e-4, err


# ---- (c), (d), (e): labels, epochs -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def complexes():
    from disco_diffdock_amd import synthetic
    return [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in COMPLEXES]


@pytest.fixture(scope='module')
def labels(dev, complexes):
    """the oracle encoder's latents of the three complexes, made twice: (e)"""
    from disco_diffdock_amd import ar_training
    from disco_diffdock_amd.latent_encoder import TPEncoder
    torch.manual_seed(5)
    enc = TPEncoder(None, 2, 1, sh_lmax=1, ns=24, nv=4, num_conv_layers=3, lm_embedding_type='esm', latent_hidden_dim=32).to(dev).train()
    first = ar_training.make_latent_labels(enc, complexes, temperature=0.01, seed=3)
    assert enc.training and enc.apply_gumbel_softmax and enc.latent_temperature == 1.0      # put back
    again = ar_training.make_latent_labels(enc, complexes, temperature=0.01, seed=3)
    logits = ar_training.make_latent_labels(enc, complexes, no_sampling=True, seed=3)
    return first, again, logits


def test_latent_labels_are_reproducible_one_hots(complexes, labels):
    first, again, logits = labels
    assert set(first) == {c['name'] for c in complexes}
    for c in complexes:
        (l, r), (l2, r2), (gl, gr) = first[c['name']], again[c['name']], logits[c['name']]
        assert not l.is_cuda and tuple(l.shape) == (len(c['lig_pos']), 2) and tuple(r.shape) == (len(c['rec_pos']), 2) and l.dtype == torch.float32
        assert torch.equal(l, l2) and torch.equal(r, r2)
        both = torch.cat([l, r])
        assert bool(((both == 0) | (both == 1)).all()) and both.sum(0).tolist() == [1.0, 1.0]      # each column a one-hot over the graph
        assert tuple(gl.shape) == tuple(l.shape) and bool(torch.isfinite(gl).all()) and not bool(((gl == 0) | (gl == 1)).all())


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_two_adam_steps_are_reproducible_and_reach_every_parameter(dev, complexes, labels):
    from disco_diffdock_amd import ar_training
    P, Q = smr.random_state_dict(smr.ScoreModelConfig(**LATENT), seed=6), _predictor_weights(6, True)

    def run(freeze=False):
        model = _ar_model(dev, P, Q, latent_dropout=0.1, batch_norm=True, dropout=0.1)
        if freeze:
            for p in model.pretrained_score_model.parameters():
                p.requires_grad = False
        before = _state(model)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        grads = {}
        hooks = [p.register_hook(lambda g, k=k: grads.setdefault(k, g.detach().clone())) for k, p in model.named_parameters() if p.requires_grad and p.numel()]
        meters = [ar_training.train_ar_epoch(model, complexes, labels[0], opt, 3, seed=11, epoch=e) for e in range(2)]      # one batch per epoch: two steps
        for h in hooks:
            h.remove()
        return meters, grads, before, _state(model)

    (meters_a, grads, before, state_a), (meters_b, _, _, state_b) = run(), run()
    assert all(np.isfinite(m['ar_loss']) and m['ar_loss'] > 0 for m in meters_a) and meters_a == meters_b
    for k in state_a:
        assert torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())), k
    parameters = [k for k, p in _ar_model(dev, P, Q).named_parameters() if p.numel()]
    names = [k for k in parameters if k.startswith(EMBED_PARAMETERS)]
    assert set(grads) == set(names) and sum(k.startswith('latent_') for k in names) == 20      # (2 predictors: 3 Linears and 2 BatchNorms, weight and bias)
    assert sum(k.startswith('pretrained_score_model.') for k in names) > 50
    for k in names:
        assert bool(torch.isfinite(grads[k]).all()) and bool((grads[k] != 0).any()), k      # both predictors and every score-model parameter embed() runs
    _, frozen_grads, before, after = run(freeze=True)
    assert frozen_grads and all(k.startswith('latent_') for k in frozen_grads)
    changed = {k for k in parameters if not torch.equal(after[k], before[k])}      # (parameters: the frozen conv layers' BatchNorm buffers still move in .train())
    assert changed and all(k.startswith('latent_') for k in changed), sorted(k for k in changed if not k.startswith('latent_'))


def test_test_epoch_accuracy_is_the_per_graph_recomputation(dev, complexes, labels):
    from disco_diffdock_amd import ar_training
    from disco_diffdock_amd.training import epoch_permutation
    P, Q = smr.random_state_dict(smr.ScoreModelConfig(**LATENT), seed=6), _predictor_weights(6, True)
    for no_sampling, lab in ((False, labels[0]), (True, labels[2])):
        model = _ar_model(dev, P, Q, batch_norm=True)
        out = ar_training.test_ar_epoch(model, complexes, lab, 2, seed=13, num_latents=2, no_sampling=no_sampling)
        assert set(out) == {'ar_loss', 'accuracy', 'accuracy0', 'accuracy1', 'int0_ar_loss', 'int0_accuracy', 'int1_ar_loss', 'int1_accuracy'}
        # per graph, in plain torch, as train_ar.py:169-177 computes it
        order = epoch_permutation(len(complexes), 13, 0)
        losses, hits, idxs = [], [], []
        model.eval()
        with torch.no_grad():
            for at in range(0, 3, 2):
                data = ar_training.ar_batch(model, [complexes[i] for i in order[at:at + 2]], lab, 13, 0, no_sampling)
                parts = model.logit_list(model(data))
                tl, tr = torch.split(data.teacher_l, (data.lig_ptr[1:] - data.lig_ptr[:-1]).tolist()), torch.split(data.teacher_r, (data.rec_ptr[1:] - data.rec_ptr[:-1]).tolist())
                for g, k in enumerate(data.decoding_idx.tolist()):
                    s, t = parts[g][0, 0].double(), torch.cat([tl[g][:, k], tr[g][:, k]]).double()
                    label = torch.softmax(t, 0)[None] if no_sampling else torch.argmax(t)
                    losses.append(float(torch.nn.functional.cross_entropy(s[None] if no_sampling else s, label)))
                    hits.append(float(torch.argmax(s) == torch.argmax(t)))
                    idxs.append(k)
                    # the input latent: the label's columns before k, zeros from k on
                    n_l = tl[g].shape[0]
                    il = data['ligand'].input_latent[data.lig_ptr[g]:data.lig_ptr[g + 1]]
                    assert not bool(il[:, k:].any()) and (no_sampling or torch.equal(il[:, :k], tl[g][:, :k])) and il.shape[0] == n_l
        assert out['accuracy'] == pytest.approx(np.mean(hits), abs=1e-12) and out['ar_loss'] == pytest.approx(np.mean(losses), rel=1e-5)
        for d in range(2):
            mine = [h for h, k in zip(hits, idxs) if k == d]
            if mine:
                assert out[f'accuracy{d}'] == out[f'int{d}_accuracy'] == pytest.approx(np.mean(mine), abs=1e-12)
            else:
                assert np.isnan(out[f'accuracy{d}'])
