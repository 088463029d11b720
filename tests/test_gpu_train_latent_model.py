"""GPU tests of the latent-conditioned (DisCo) TrainableScoreModel: latent_dim=2, latent_vocab=1, latent_droprate=0.1, the configuration of the reference's
disco_diffdockS_score_model, on the three complexes, times and functional of tests/test_gpu_train_model.py.

(a) the gradient of EVERY parameter and of latent_l / latent_r against autograd through the oracle (oracle.score_model_ref.score_model_forward) in fp64.
    Latents are SOFT and graph 1 is unconditional: with g = torch.Generator().manual_seed(4) and keep = (1, 0, 1), for graph i in order
    y = softmax(2 * randn(2, n_lig_i + n_rec_i, generator=g, dtype=float64), -1) * keep[i], the ligand's columns first; unconditional = 1 - keep[batch].
    Bars as in test (a) of tests/test_gpu_train_model.py: forward 1e-4; a gradient passes under max(4 * err32, 1e-5), err32 the oracle's own fp32 run
    against its fp64 run.  The ReLU clearance of that test's docstring is asserted FIRST, from the oracle alone: >= 8.  With the weights of
    random_state_dict(cfg, seed=29) and exactly this input the clearance is 10.3 on one host CPU and 11.0 on another (the oracle's fp32 run depends on
    the host's BLAS), tightest at conv_layers.1.fc.0 both times (seeds 1-28 do not reach 8).
    The cross MLP's latent columns get a gradient of exactly 0 (the cross rows hold zeros there).
(b) the round trip to the inference engine: .eval() against get_model(... latent_dim=2, latent_vocab=1, latent_droprate=0.1) loaded from this module's
    state_dict, 4 samples of one complex, with one-hot latents and unconditional = 0, and with zero latents and unconditional = 1.  1e-4.
(c) training: a stand-in encoder (one nn.Linear per side from the node features to D logits) -> ragged_gumbel_softmax -> LatentModelWrapper ->
    loss_function -> backward(), with batch_norm, dropout 0.1 and a seeded keep that holds both a 0 and a 1 (asserted first): the gradient reaches every
    parameter of the score model, all five unconditional rows and the encoder; two Adam steps from one state and one seed give identical bits everywhere.
(d) training.train_epoch with the wrapper: every batch gets keep = draw_latent_keep of ITS complexes in ITS order (the epoch's permutation is not the
    identity and one complex is dropped: asserted first), and two epochs from one state and one seed give identical bits and meters."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import rel_err
from oracle import score_model_ref as smr
from test_gpu_radial_conv import _bits
from test_gpu_round3 import _record_drift      # the suite's record of measured parity figures
from test_gpu_train_model import MODEL, _batch, _functional, _made_up_targets, _tables

pytestmark = pytest.mark.gpu
LATENT = dict(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
KEEP = (1.0, 0.0, 1.0)
WEIGHT_SEED = 29


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _soft_latents(b):
    """(latent_l [N_lig, 2], latent_r [N_rec, 2], unconditional_l [N_lig, 1], unconditional_r [N_rec, 1]) in fp64, as the module's docstring states them"""
    g = torch.Generator().manual_seed(4)
    lig_batch, rec_batch = b['ligand'].batch.long(), b['receptor'].batch.long()
    ls, rs = [], []
    for i, k in enumerate(KEEP):
        n_lig, n_rec = int((lig_batch == i).sum()), int((rec_batch == i).sum())
        y = torch.softmax(2 * torch.randn(2, n_lig + n_rec, generator=g, dtype=torch.float64), -1) * k
        ls.append(y[:, :n_lig].T)
        rs.append(y[:, n_lig:].T)
    keep = torch.tensor(KEEP, dtype=torch.float64)
    return torch.cat(ls).contiguous(), torch.cat(rs).contiguous(), (1 - keep[lig_batch])[:, None], (1 - keep[rec_batch])[:, None]


def _with_latents(b, dtype, grad):
    b = copy.deepcopy(b)
    lat_l, lat_r, unc_l, unc_r = _soft_latents(b)
    b['ligand'].latent_h, b['receptor'].latent_h = lat_l.to(dtype).requires_grad_(grad), lat_r.to(dtype).requires_grad_(grad)
    b['ligand'].unconditional, b['receptor'].unconditional = unc_l.to(dtype), unc_r.to(dtype)
    return b


def _oracle_gradients(cfg, P, batch, dtype):
    Pd = {k: (v.detach().to(dtype).requires_grad_() if v.is_floating_point() else v) for k, v in P.items()}
    so3, torus = _tables()
    b = _with_latents(batch, dtype, True)
    out = smr.score_model_forward(Pd, cfg, b, so3, torus, dtype=dtype)
    loss = sum((o.double() * w).sum() for o, w in zip(out, _functional(out[2].shape[0])))
    loss.backward()
    grads = {k: v.grad.double().numpy() for k, v in Pd.items() if v.is_floating_point() and v.grad is not None}
    grads['latent_l'], grads['latent_r'] = b['ligand'].latent_h.grad.double().numpy(), b['receptor'].latent_h.grad.double().numpy()
    return [o.detach().double().numpy() for o in out], grads


def _relu_preactivations(cfg, P, batch, dtype):
    """the oracle's pre-activations in front of the ReLUs of the three edge embeddings and of every conv layer's radial MLPs (name -> [E_g, 24 | 72])"""
    Pd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    b = _with_latents(batch, dtype, False)
    for nt in ('ligand', 'receptor'):
        b[nt].pos = b[nt].pos.to(dtype)
    latent_h = (b['ligand'].latent_h, b['receptor'].latent_h)
    lig, rec = smr.build_lig_conv_graph(b, cfg, latent_h, dtype), smr.build_rec_conv_graph(b, cfg, latent_h, dtype)
    tr_sigma = smr.t_to_sigma(*[b.complex_t[k] for k in ('tr', 'rot', 'tor')], cfg)[0]
    cross = smr.build_cross_conv_graph(b, cfg, (tr_sigma * 3 + 20).unsqueeze(1).to(dtype), lig[4], latent_h, dtype)
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
    """computed once: the oracle's outputs and gradients in fp64 and in fp32 (no BatchNorm, no dropout) and its hidden units' distance from the ReLU's kink"""
    cfg = smr.ScoreModelConfig(batch_norm=False, **LATENT)
    P = smr.random_state_dict(cfg, seed=WEIGHT_SEED)
    _, b = _batch()
    out64, g64 = _oracle_gradients(cfg, P, b, torch.float64)
    out32, g32 = _oracle_gradients(cfg, P, b, torch.float32)
    p64, p32 = _relu_preactivations(cfg, P, b, torch.float64), _relu_preactivations(cfg, P, b, torch.float32)
    clearance = {k: float(p64[k].abs().min() / (p32[k].double() - p64[k]).pow(2).mean().sqrt()) for k in p64}
    return dict(cfg=cfg, P=P, out64=out64, g64=g64, out32=out32, g32=g32, clearance=clearance, hidden_units=sum(v.numel() for v in p64.values()))


def _model(dev, P=None, **kw):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    model = TrainableScoreModel(**dict(MODEL, **LATENT, **kw))
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
    lat_l, lat_r, unc_l, unc_r = _soft_latents(b)
    b = b.to(dev)
    latent_l, latent_r = lat_l.float().to(dev).requires_grad_(), lat_r.float().to(dev).requires_grad_()
    b['ligand'].latent_h, b['receptor'].latent_h = latent_l, latent_r
    b['ligand'].unconditional, b['receptor'].unconditional = unc_l.float().to(dev), unc_r.float().to(dev)
    out = model(b)
    loss = sum((o.double() * w.to(dev)).sum() for o, w in zip(out, _functional(out[2].shape[0])))
    loss.backward()
    for name, a, w, w32 in zip(('tr', 'rot', 'tor'), out, r['out64'], r['out32']):
        err, err32 = rel_err(a.detach().cpu().numpy(), w), rel_err(w32, w)
        print(f'forward {name}: device {err:.2e}, host fp32 {err32:.2e}')
        _record_drift(f'train_latent_model.forward.{name}', err, host_fp32=err32, bar=1e-4)
        assert err < 1e-4, (name, err)
    cross = model.cross_edge_embedding[0].weight.grad
    assert not bool(cross[:, 64:].any()) and bool(cross[:, :64].any())      # the cross rows hold zeros in the latent columns: exactly no gradient
    assert not r['g64']['cross_edge_embedding.0.weight'][:, 64:].any()
    failures = []
    tensors = [(k, p.grad) for k, p in model.named_parameters() if p.numel()] + [('latent_l', latent_l.grad), ('latent_r', latent_r.grad)]
    assert sum('unconditional_embedding' in k for k, _ in tensors) == 5
    for k, grad in tensors:
        assert grad is not None, k
        want = r['g64'][k]
        if not want.any():      # (the last conv layer's receptor-side groups: nothing reads the receptor rows after it)
            assert not bool(grad.any()), k
            continue
        err, err32 = rel_err(grad.cpu().numpy(), want), rel_err(r['g32'][k], want)
        bar = max(4 * err32, 1e-5)
        print(f'{k}: device {err:.2e}, host fp32 {err32:.2e}, bar {bar:.2e}')
        _record_drift(f'train_latent_model.grad.{k}', err, host_fp32=err32, bar=bar)
        if not err < bar:
            failures.append((k, err, err32, bar))
    assert not failures, failures
    # a batch without its latents is refused by name
    del b['ligand'].__dict__['latent_h']
    with pytest.raises(RuntimeError, match=r"data\['ligand'\].latent_h"):
        model(b)
    b['ligand'].latent_h = latent_l.detach()
    del b['receptor'].__dict__['unconditional']
    with pytest.raises(RuntimeError, match=r"data\['receptor'\].unconditional"):
        model(b)


# ---- (b) round trip to the inference engine ----------------------------------------------------------------------------------------------------------------------
def test_round_trip_to_the_inference_engine(dev):
    from functools import partial
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    from disco_diffdock_amd.model_utils import get_model
    from test_gpu_model import ARGS_S, _dev_batch
    args = Namespace(**dict(vars(ARGS_S), **LATENT))
    cfg = smr.ScoreModelConfig(**LATENT)
    trainable = _model(dev, smr.random_state_dict(cfg, seed=9), dropout=0.1).eval()
    assert all(bool(getattr(trainable, f'{k}_unconditional_embedding').any()) for k in ('lig_node', 'rec_node', 'lig_edge', 'rec_edge', 'cross_edge'))
    engine = get_model(args, dev, partial(t_to_sigma, args=args), no_parallel=True).score_model
    engine.load_state_dict(trainable.state_dict(), strict=True)
    c = synthetic.make_complex(71, n_res=28, n_lig=12)
    n_lig, n_rec, B = len(c['lig_pos']), len(c['rec_pos']), 4
    rng = np.random.default_rng(3)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 1.5, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(B)]).astype(np.float32)
    one_hot = np.zeros((B, n_lig + n_rec, 2), np.float32)      # per sample and latent dimension one node of the complex, on either side
    picks = rng.integers(0, n_lig + n_rec, size=(B, 2))
    picks[0, 0], picks[1, 1] = 0, n_lig + n_rec - 1            # (a ligand atom and a residue for certain)
    for s in range(B):
        for d in range(2):
            one_hot[s, picks[s, d], d] = 1
    cases = {'one_hot': (one_hot, 0.0), 'unconditional': (np.zeros_like(one_hot), 1.0)}
    for tag, (lat, unc) in cases.items():
        for t in (0.7, 0.2):
            b = _dev_batch(c, B, pos, dev, t)
            b['ligand'].latent_h = torch.from_numpy(lat[:, :n_lig].reshape(-1, 2).copy()).to(dev)
            b['receptor'].latent_h = torch.from_numpy(lat[:, n_lig:].reshape(-1, 2).copy()).to(dev)
            b['ligand'].unconditional = torch.full((B * n_lig, 1), unc, device=dev)
            b['receptor'].unconditional = torch.full((B * n_rec, 1), unc, device=dev)
            want = engine(b)
            with torch.no_grad():
                got = trainable(b)
            assert got[2].shape == want[2].shape == (B * int(c['edge_mask'].sum()),)
            errs = {n: rel_err(a.cpu().numpy(), w.cpu().numpy()) for n, a, w in zip(('tr', 'rot', 'tor'), got, want)}
            print(tag, t, {k: f'{v:.2e}' for k, v in errs.items()})
            worst = max(errs, key=errs.get)
            _record_drift(f'train_latent_model.round_trip.{tag}.t{t}', errs[worst], worst_block=worst, bar=1e-4)
            assert errs[worst] < 1e-4, (tag, t, worst, errs[worst])


# ---- (c) training --------------------------------------------------------------------------------------------------------------------------------------------------
class _StandInEncoder(torch.nn.Module):
    """one Linear per side from the node features to D logits, then the ragged Gumbel softmax at the temperature the wrapper hands over"""

    def __init__(self, n_lig_features, n_rec_features, D, names, seed):
        super().__init__()
        self.lig, self.rec = torch.nn.Linear(n_lig_features, D), torch.nn.Linear(n_rec_features, D)
        self.names, self.seed, self.latent_temperature = names, seed, None      # names None: the batch's own (``data.name`` of a collated batch)

    def forward(self, data):
        from disco_diffdock_amd.runtime import stream_id
        from disco_diffdock_amd.tensor_layers import ragged_gumbel_softmax
        lig, rec = data['ligand'], data['receptor']
        streams = [stream_id(n) for n in (self.names if self.names is not None else data.name)]
        return ragged_gumbel_softmax(self.lig(lig.x.float()), self.rec(rec.x.float()), lig.batch, rec.batch, self.latent_temperature, self.seed, streams)


def test_training_step_reaches_every_parameter_and_is_reproducible(dev):
    from disco_diffdock_amd import training
    from disco_diffdock_amd.train_model import LatentModelWrapper
    cs, b = _batch()
    b = b.to(dev)
    n_rot = int(cs[0]['edge_mask'].sum())
    keep = training.draw_latent_keep(cs, LATENT['latent_droprate'], seed=6, draw=0)
    assert (keep == 0).any() and (keep == 1).any(), keep      # both branches of the latent dropout are in the batch
    P = smr.random_state_dict(smr.ScoreModelConfig(**LATENT), seed=6)
    targets = None

    def run():
        nonlocal targets
        torch.manual_seed(4321)
        score_model = _model(dev, P, batch_norm=True, dropout=0.1)
        encoder = _StandInEncoder(b['ligand'].x.shape[1], b['receptor'].x.shape[1], 2, [c['name'] for c in cs], seed=77).to(dev)
        model = LatentModelWrapper(encoder, score_model, training_latent_temperature=1.0, latent_droprate=LATENT['latent_droprate']).train()
        if targets is None:
            targets = _made_up_targets(dev, model, 3, n_rot, 0.5, 31)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        first = None
        for _ in range(2):
            opt.zero_grad()
            tr, rot, tor = model(b, seed=99, keep=keep)
            loss = training.loss_function(tr, rot, tor, targets, model)[0]
            loss.backward()
            if first is None:
                first = {k: p.grad.clone() if p.grad is not None else None for k, p in model.named_parameters() if p.numel()}
            opt.step()
        assert encoder.latent_temperature == 1.0
        return loss.detach(), first, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (loss_a, grads, state_a), (loss_b, _, state_b) = run(), run()
    assert bool(torch.isfinite(loss_a).all())
    assert sum('unconditional_embedding' in k for k in grads) == 5 and sum(k.startswith('encoder.') for k in grads) == 4
    for k, g in grads.items():
        assert g is not None, k
        assert bool(torch.isfinite(g).all()), k
        assert bool((g != 0).any()), k      # none all zero: the score model, the five unconditional rows, the encoder
    assert torch.equal(_bits(loss_a), _bits(loss_b))
    for k in state_a:
        assert torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())), k


# ---- (d) an epoch through training.train_epoch ---------------------------------------------------------------------------------------------------------------
def test_train_epoch_with_the_wrapper(dev):
    import latent_embedding_ref as lref
    from disco_diffdock_amd import synthetic, training
    from disco_diffdock_amd.runtime import stream_id
    from disco_diffdock_amd.train_model import LatentModelWrapper
    complexes = [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in ((70, 22), (71, 28), (60, 35), (67, 24))]
    seed, epoch, rate = 10, 0, LATENT['latent_droprate']
    order = training.epoch_permutation(len(complexes), seed, epoch)
    flags = training.draw_latent_keep(complexes, rate, seed, epoch)
    assert order != sorted(order) and (flags == 0).sum() == 1, (order, flags)      # batches are not in list order, and one complex trains unconditionally
    P = smr.random_state_dict(smr.ScoreModelConfig(**LATENT), seed=6)
    n_lig_features, n_rec_features = complexes[0]['lig_x'].shape[1], complexes[0]['rec_x'].shape[1]

    def run():
        torch.manual_seed(99)
        encoder = _StandInEncoder(n_lig_features, n_rec_features, 2, None, seed=77).to(dev)
        model = LatentModelWrapper(encoder, _model(dev, P, batch_norm=True, dropout=0.1), 1.0, rate)
        seen = []
        model.register_forward_pre_hook(lambda m, args, kwargs: seen.append((list(args[0].name), np.asarray(kwargs['keep']).copy())), with_kwargs=True)
        summary = training.train_epoch(model, complexes, torch.optim.Adam(model.parameters(), lr=1e-3), 2, seed, epoch)
        return summary, seen, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (sum_a, seen, state_a), (sum_b, _, state_b) = run(), run()
    assert [names for names, _ in seen] == [[complexes[i]['name'] for i in order[at:at + 2]] for at in (0, 2)]
    for names, keep in seen:      # the flags of the batch's own complexes, in the batch's order: the mirror by name
        assert np.array_equal(keep, lref.latent_keep(seed, [stream_id(n) for n in names], rate, draw=epoch))
    assert sum(int((keep == 0).sum()) for _, keep in seen) == 1
    assert set(sum_a) == set(training.TRAIN_METERS) and all(np.isfinite(v) for v in sum_a.values()) and sum_a == sum_b
    for k in state_a:
        assert torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())), k
