"""GPU tests of confidence.TrainableConfidenceModel and confidence_training: a collated batch of all-atom complexes through the six edge embeddings, the
OldAtomEncoders, nine all-atom convs per layer (the third family of the radial tensor product), the segmented-sum pooling and the predictor.

(a) the gradient of every parameter the forward uses against fp64 autograd through oracle.confidence_ref.confidence_forward, the model in .eval() with
    randomised running buffers, a fixed random linear functional of the logits as the loss.  The bar of a tensor is MEASURED as in
    tests/test_gpu_train_model.py: the oracle's own fp32 host run against its fp64 run gives err32; the device passes under 4 * err32, floored at 1e-5.
    Asserted FIRST, from the oracle alone: every radial-MLP and edge-embedding pre-activation is at least 8 times its tensor's rms fp32-against-fp64
    difference away from zero.  The weight seed was chosen on the CPU so that this holds: seeds 9 and 5 leave a unit at 1.4 and 0.009 rms
    differences (conv_layers.27.fc, conv_layers.24.fc), seed 11 clears with 8.6.
(b) the round trip: .eval() against Context.confidence_forward from the same state dict on B = 3 poses of the golden complex, and the golden logits; 1e-4.
(c) one confidence_loss(...).backward() reaches every used parameter; two Adam steps from one state and one seed give identical bits, buffers included.
(d) train_confidence_epoch twice from one state gives identical state; test_confidence_epoch's AUC and accuracy equal the host computation."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

import confidence_conv_ref as ccr
from helpers import complex_from_npz, rel_err, to_graph
from oracle import confidence_ref as cr
from oracle import graph_lite
from test_gpu_radial_conv import _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures

pytestmark = pytest.mark.gpu
ARGS = Namespace(all_atoms=True, ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                 max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, embedding_type='sinusoidal', embedding_scale=10000,
                 scale_by_sigma=True, no_torsion=False, no_batch_norm=False, dropout=0.0, use_second_order_repr=False,
                 esm_embeddings_path='data/esm2_3billion_embeddings.pt', rmsd_classification_cutoff=[2.0], confidence_no_batchnorm=False,
                 tr_sigma_min=0.1, tr_sigma_max=34.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.0314, tor_sigma_max=3.14)
COMPLEXES = ((70, 22), (71, 28))      # (seed, residues); a third graph is the first one with its ligand 60 A away: no la and no lr edges there
WEIGHT_SEED = 11


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _graph(c):
    return graph_lite.add_atoms(to_graph(c), c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index'])


def _zero_times(b, B):
    b.complex_t = {k: torch.zeros(B) for k in ('tr', 'rot', 'tor')}
    for nt in ('ligand', 'receptor', 'atom'):
        b[nt].node_t = {k: torch.zeros(b[nt].num_nodes) for k in ('tr', 'rot', 'tor')}
    return b


def _complexes():
    from disco_diffdock_amd import synthetic
    cs = []
    for seed, n_res in COMPLEXES:
        c = synthetic.make_complex(seed, n_res=n_res, n_lig=12)
        synthetic.add_receptor_atoms(c, np.random.default_rng(seed + 1))
        cs.append(c)
    far = copy.deepcopy(cs[0])
    far['lig_pos'] = (far['lig_pos'] + np.array([[60.0, 0, 0]])).astype(np.float32)
    return cs + [far]


def _batch():
    cs = _complexes()
    rng = np.random.default_rng(8)
    for c in cs:
        c['lig_pos'] = (c['lig_pos'] + rng.normal(0, 0.3, size=c['lig_pos'].shape)).astype(np.float32)
    return _zero_times(graph_lite.collate([_graph(c) for c in cs]), len(cs))


def _functional(shape, seed=21):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _oracle_gradients(cfg, P, batch, dtype):
    Pd = {k: (v.detach().to(dtype).requires_grad_() if v.is_floating_point() and not k.endswith('.offset') else v) for k, v in P.items()}
    out = cr.confidence_forward(Pd, cfg, copy.deepcopy(batch), dtype=dtype)
    (out.double() * _functional(out.shape)).sum().backward()
    return out.detach().double().numpy(), {k: v.grad.double().numpy() for k, v in Pd.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}


def _relu_preactivations(cfg, P, batch, dtype):
    """the oracle's pre-activations in front of the ReLUs of the six edge embeddings and of every conv's radial MLP that the forward runs"""
    Pd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    lin = lambda row, name: row @ Pd[f'{name}.weight'].T + Pd[f'{name}.bias']
    ns, L = cfg.ns, cfg.num_conv_layers
    b = copy.deepcopy(batch)
    lig, rec, atom = b['ligand'], b['receptor'], b['atom']
    emb = lambda t: cr.sinusoidal_embedding(cfg.embedding_scale * t, cfg.sigma_embed_dim).to(dtype)
    sig = dict(l=emb(lig.node_t['tr']), r=emb(rec.node_t['tr']), a=emb(atom.node_t['tr']))
    _, inter = cr.confidence_forward(Pd, cfg, copy.deepcopy(b), dtype=dtype, return_intermediates=True)
    es = inter['edge_sets']
    out = {}
    bond = torch.cat([b['ligand', 'ligand'].edge_attr.to(dtype), torch.zeros(es['ll'][0].shape[1] - b['ligand', 'ligand'].edge_attr.shape[0], 4, dtype=dtype)], 0)
    out['lig_edge_embedding'] = lin(cr._intra_graph(lig.pos.to(dtype), es['ll'][0], sig['l'], cfg.lig_max_radius, cfg, dtype, extra=bond)[0], 'lig_edge_embedding.0')
    out['rec_edge_embedding'] = lin(cr._intra_graph(rec.pos.to(dtype), es['rr'][0], sig['r'], cfg.rec_max_radius, cfg, dtype)[0], 'rec_edge_embedding.0')
    out['atom_edge_embedding'] = lin(cr._intra_graph(atom.pos.to(dtype), es['aa'][0], sig['a'], cfg.lig_max_radius, cfg, dtype)[0], 'atom_edge_embedding.0')
    for k, pa, pb, s_, stop in (('lr', lig.pos, rec.pos, sig['l'], cfg.cross_max_distance), ('la', lig.pos, atom.pos, sig['l'], cfg.cross_max_distance),
                                ('ar', atom.pos, rec.pos, sig['a'], cfg.rec_max_radius)):
        idx = es[k][0]
        d = (pb[idx[1]] - pa[idx[0]]).norm(dim=-1)
        out[f'{k}_edge_embedding'] = lin(torch.cat([s_[idx[0]], cr.gaussian_smearing(d, stop, 32, dtype)], 1), f'{k}_edge_embedding.0')
    plan = (('l', 'l', 'll', False), ('l', 'r', 'lr', False), ('l', 'a', 'la', False), ('a', 'a', 'aa', False), ('a', 'l', 'la', True),
            ('a', 'r', 'ar', False), ('r', 'r', 'rr', False), ('r', 'l', 'lr', True), ('r', 'a', 'ar', True))
    for l in range(L):
        if l == 0:
            x = dict(l=inter['x0']['lig'], a=inter['x0']['atom'], r=inter['x0']['rec'])
        else:
            _, it = cr.confidence_forward(Pd, cfg, copy.deepcopy(b), dtype=dtype, return_intermediates=True, stop_after=l)
            x = dict(l=it['lig_node_attr'], a=it['atom_node_attr'], r=it['rec_node_attr'])
        for k, (rv, sn, e, flip) in enumerate(plan):
            if l == L - 1 and k >= 3:
                break
            idx = torch.flip(es[e][0], dims=[0]) if flip else es[e][0]
            if idx.shape[1]:
                out[f'conv_layers.{9 * l + k}.fc'] = lin(torch.cat([es[e][1], x[rv][idx[0], :ns], x[sn][idx[1], :ns]], 1), f'conv_layers.{9 * l + k}.fc.0')
    return out


@pytest.fixture(scope='module')
def parity_reference():
    """computed once, on the CPU: the oracle's logits and parameter gradients in fp64 and fp32, and how far its hidden units stay from the ReLU's kink in
    units of the tensor's rms fp32-against-fp64 difference"""
    cfg = cr.ConfidenceModelConfig(num_conv_layers=4)
    b = _batch()
    seed = WEIGHT_SEED
    P = cr.random_state_dict(cfg, seed=seed)
    p64, p32 = _relu_preactivations(cfg, P, b, torch.float64), _relu_preactivations(cfg, P, b, torch.float32)
    clearance = {k: float(p64[k].abs().min() / (p32[k].double() - p64[k]).pow(2).mean().sqrt()) for k in p64}
    out64, g64 = _oracle_gradients(cfg, P, b, torch.float64)
    out32, g32 = _oracle_gradients(cfg, P, b, torch.float32)
    return dict(cfg=cfg, P=P, seed=seed, out64=out64, g64=g64, out32=out32, g32=g32, clearance=clearance, hidden_units=sum(v.numel() for v in p64.values()))


def _model(dev, P=None, **kw):
    from disco_diffdock_amd.model_utils import get_trainable_model
    model = get_trainable_model(Namespace(**dict(vars(ARGS), **kw)), dev, confidence_mode=True)
    if P is not None:
        model.load_state_dict(P, strict=True)
    return model.to(dev)


# ---- (a) gradient parity with the oracle ---------------------------------------------------------------------------------------------------------------------
def test_gradient_parity_with_the_oracle(dev, parity_reference):
    r = parity_reference
    tight = min(r['clearance'], key=r['clearance'].get)
    print(f"weight seed {r['seed']}: {r['hidden_units']} hidden units, the closest to the kink: {tight} at {r['clearance'][tight]:.1f} rms fp32 differences")
    assert r['clearance'][tight] >= 8, (tight, r['clearance'][tight])      # the input leaves every ReLU branch to the model, none to a summation order
    model = _model(dev, r['P'], num_conv_layers=4).eval()
    assert set(model.state_dict()) == set(cr.state_dict_spec(r['cfg']))
    out = model(_batch().to(dev))
    assert out.shape == (3, 2)
    (out.double() * _functional(out.shape).to(dev)).sum().backward()
    err, err32 = rel_err(out.detach().cpu().numpy(), r['out64']), rel_err(r['out32'], r['out64'])
    print(f'forward: device {err:.2e}, host fp32 {err32:.2e}')
    _record_drift('train_confidence.forward', err, host_fp32=err32, bar=1e-4)
    assert err < 1e-4, err
    used, failures = set(model.used_parameters()), []
    unused = [n for n, _ in model.named_parameters() if n not in used]
    assert len(unused) == 6 * 6 and all(n.startswith(tuple(f'conv_layers.{27 + k}.' for k in range(3, 9))) for n in unused)
    for name, p in model.named_parameters():
        if name in unused:      # convs 3..8 of the last layer: no gradient, as in the reference
            assert p.grad is None and name not in r['g64'], name
            continue
        assert p.grad is not None and name in r['g64'], name
        err, err32 = rel_err(p.grad.cpu().numpy(), r['g64'][name]), rel_err(r['g32'][name], r['g64'][name])
        bar = max(4 * err32, 1e-5)
        _record_drift(f'train_confidence.grad.{name}', err, host_fp32=err32, bar=bar)
        if not err < bar:
            failures.append((name, err, err32))
    print('worst:', sorted(((rel_err(p.grad.cpu().numpy(), r['g64'][n]), n) for n, p in model.named_parameters() if n in used), reverse=True)[:5])
    assert not failures, failures


# ---- (b) the round trip to the inference engine ------------------------------------------------------------------------------------------------------------
def test_round_trip_to_the_inference_engine(dev, golden):
    from disco_diffdock_amd.confidence import ConfidenceModel
    from disco_diffdock_amd.runtime import Complex, Context
    z, c = golden('confidence_paper_model'), complex_from_npz(golden('complex_confidence'))
    cfg, B = cr.ConfidenceModelConfig(), 3
    P = cr.random_state_dict(cfg, seed=int(z['seed']))
    model = _model(dev, P, dropout=0.1).eval()
    assert set(model.state_dict()) == set(cr.state_dict_spec(cfg)) and all(model.state_dict()[k].shape == tuple(s) for k, s in cr.state_dict_spec(cfg).items())
    n = len(c['lig_pos'])
    pos = torch.as_tensor(z['pos']).float().reshape(-1, n, 3)[:B]
    b = _zero_times(graph_lite.collate([_graph(c) for _ in range(B)]), B)
    b['ligand'].pos = pos.reshape(-1, 3)
    with torch.no_grad():
        got = model(b.to(dev))
    want = np.asarray(z['confidence']).reshape(int(z['B']), -1)[:B]      # (.eval(): a graph's logits do not depend on the batch it is in)
    assert rel_err(got.cpu().numpy().reshape(B, -1), want) < 1e-4
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ctx = Context(device=0, all_atoms=1, embedding_scale=10000.0, num_confidence_outputs=2)
    ctx.load_state_dict(state)
    cx = Complex(ctx, c, max_batch=B)
    cx.set_atoms(c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index'])
    engine = cx.confidence_forward(pos.to(dev))
    assert rel_err(got.cpu().numpy().reshape(B, -1), engine.cpu().numpy().reshape(B, -1)) < 1e-4
    inference = ConfidenceModel(ARGS, dev)
    inference.load_state_dict(state, strict=True)      # and back: what was trained here loads into the inference class
    fresh = _model(dev)
    fresh.load_state_dict(state, strict=True)


def test_refused_configurations_use_the_inference_models_words(dev):
    from disco_diffdock_amd.model_utils import get_trainable_model
    for kw in (dict(use_second_order_repr=True), dict(use_old_atom_encoder=False), dict(latent_dim=2), dict(sh_lmax=1)):
        with pytest.raises(RuntimeError, match='only sh_lmax=2, first-order irreps, OldAtomEncoder, no latents are implemented'):
            get_trainable_model(Namespace(**dict(vars(ARGS), **kw)), dev, confidence_mode=True)
    with pytest.raises(RuntimeError, match='all_atoms'):
        get_trainable_model(Namespace(**dict(vars(ARGS), all_atoms=False)), dev, confidence_mode=True)


# ---- (c) training: every used parameter, the same bits -----------------------------------------------------------------------------------------------------
def _labelled_batch():
    b = _batch()
    b.y, b.rmsd = torch.tensor([1.0, 0.0, 0.0]), torch.tensor([1.2, 3.4, 60.0])
    b.y_binned = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]])
    return b


def test_training_reaches_every_used_parameter_with_the_same_bits(dev):
    from disco_diffdock_amd.confidence_training import confidence_loss
    cfg = cr.ConfidenceModelConfig(num_conv_layers=4)
    P = cr.random_state_dict(cfg, seed=3)
    states = []
    for _ in range(2):
        model = _model(dev, P, num_conv_layers=4, dropout=0.1, confidence_dropout=0.1).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        for step in range(2):
            opt.zero_grad()
            b = _labelled_batch()
            loss = confidence_loss(model(b.to(dev), seed=1234 + step), b, False, [2.0])
            loss.backward()
            if step == 0:
                used = set(model.used_parameters())
                for n, p in model.named_parameters():
                    assert (p.grad is not None and bool(p.grad.any())) == (n in used), n
            opt.step()
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    moved = [k for k in states[0] if not torch.equal(states[0][k].cpu(), P[k])]
    assert any('batch_norm.running_var' in k for k in moved) and any(k.startswith('confidence_predictor.1.running') for k in moved)
    assert all(torch.equal(_bits(states[0][k]) if states[0][k].dtype == torch.float32 else states[0][k], _bits(states[1][k]) if states[1][k].dtype == torch.float32 else states[1][k])
               for k in states[0])      # two Adam steps from one state and one seed: identical bits, BatchNorm buffers included


# ---- (d) epochs ------------------------------------------------------------------------------------------------------------------------------------------
def test_epochs_are_pure_functions_of_state_set_seed_and_epoch(dev):
    from disco_diffdock_amd import confidence_training as ct
    cs = {f'c{i}': c for i, c in enumerate(_complexes())}
    names = sorted(cs)
    rng = np.random.default_rng(12)
    conf_set = {n: (np.stack([cs[n]['lig_pos'] + rng.normal(0, s, size=(1, 3)) for s in (0.2, 0.5, 3.0, 6.0)]).astype(np.float32), np.array([0.4, 0.9, 5.2, 10.4]))
                for n in names}
    make = lambda n: _graph(cs[n])
    cfg = cr.ConfidenceModelConfig(num_conv_layers=4, num_confidence_outputs=1)
    P = cr.random_state_dict(cfg, seed=4)
    states = []
    for _ in range(2):
        model = _model(dev, P, num_conv_layers=4, dropout=0.1, rmsd_classification_cutoff=2.0)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        res = ct.train_confidence_epoch(model, opt, make, names, conf_set, graph_lite.collate, 2, seed=5, epoch=1, cutoff=2.0)
        assert res['batches'] == 1 and np.isfinite(res['confidence_loss'])      # three complexes in batches of two: the batch of one graph is skipped
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    assert all(torch.equal(states[0][k], states[1][k]) for k in states[0])
    ev = ct.test_confidence_epoch(model, make, names, conf_set, graph_lite.collate, 3, seed=5, epoch=1, cutoff=2.0, return_logits=True)
    logits, labels = torch.cat(ev['logits']).cpu().numpy(), torch.cat(ev['labels']).cpu().numpy()
    assert logits.shape == (3,) and abs(ev['roc_auc'] - ccr.auc_pairs(labels, logits)) < 1e-12
    assert abs(ev['accuracy'] - np.mean(labels == (logits > 0))) < 1e-7 and abs(ev['baseline_metric'] - labels.mean()) < 1e-7
    with pytest.raises(RuntimeError, match='balance is not implemented'):
        ct.refuse_options(Namespace(balance=True))
