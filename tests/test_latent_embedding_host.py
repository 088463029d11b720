"""CPU tests of the host side of the latent-conditioned (DisCo) training ops: the fp64 restatements the kernels are measured against
(tests/latent_embedding_ref.py) equal torch autograd of the plain compositions they replace, the host mirror of DDK_GUMBEL_LAYOUT and ddk_rng_latent_keep
agree with the library's host function, ddk_eemb_latent_workspace states its ranges, and TrainableScoreModel(latent_dim=2, latent_droprate=0.1) holds the
inference spec's key set."""
import numpy as np
import pytest
import torch

import edge_embedding_ref as ref
import latent_embedding_ref as lref


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def _case(seed, E, F, L, stop, n_a=7, n_b=11, same=False):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape)
    T, K = 3, F + 64 + 2 * L
    if same:
        n_b = n_a
    o = dict(pos_a=f(n_a, 3) * stop / 4, pos_b=f(n_b, 3) * stop / 4, idx_a=rng.integers(0, n_a, E), idx_b=rng.integers(0, n_b, E),
             feat=np.eye(4)[rng.integers(0, 4, E)] if F else None, sig=f(T, 32), sig_index=rng.integers(0, T, n_a), start=0.0, stop=stop,
             lat_a=f(n_a, L), unc_a=(rng.random(n_a) < 0.4) * 1.0 + 0.25 * f(n_a))
    o['lat_b'] = o['lat_a'] if same else f(n_b, L)
    if same:
        o['pos_b'] = o['pos_a']
    P = dict(w1=f(24, K) / np.sqrt(K), b1=f(24) * 0.5, w2=f(24, 24) / np.sqrt(24.0), b2=f(24), uemb=f(24))
    return o, P, f(E, 24)


@pytest.mark.parametrize('zero_latent', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.25])
@pytest.mark.parametrize('F,L,stop,same', [(4, 2, 5.0, True), (0, 1, 30.0, False), (0, 4, 30.0, False)])
def test_restatement_equals_autograd_of_the_composition(F, L, stop, same, p, zero_latent):
    """cat -> Sequential -> + unc * uemb in torch fp64, gradients of both latent tables (of the ONE table where both sides index it) included"""
    E = 41
    o, P, g = _case(11 + F + L, E, F, L, stop, same=same)
    o['zero_latent'] = zero_latent
    keep, s = ref.keep_mask(99, E, p), ref.scale(p)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    T = lambda a: torch.as_tensor(np.asarray(a))
    la = torch.tensor(o['lat_a'], requires_grad=True)
    lb = la if same else torch.tensor(o['lat_b'], requires_grad=True)
    ia, ib = T(o['idx_a']), T(o['idx_b'])
    vec = T(o['pos_b'])[ib] - T(o['pos_a'])[ia]
    offset = torch.linspace(0.0, stop, 32)
    smear = torch.exp(ref.coeff(0.0, stop) * (vec.norm(dim=-1)[:, None] - offset.double()[None, :]) ** 2)
    lat = torch.zeros(E, 2 * L, dtype=torch.float64) if zero_latent else torch.cat([la[ia], lb[ib]], 1)
    row = torch.cat(([T(o['feat'])] if F else []) + [T(o['sig'])[T(o['sig_index'])[ia]], smear, lat], 1)
    hid = torch.relu(torch.nn.functional.linear(row, t['w1'], t['b1'])) * torch.from_numpy(keep) * s
    emb = torch.nn.functional.linear(hid, t['w2'], t['b2']) + T(o['unc_a'])[ia][:, None] * t['uemb'][None, :]
    emb.backward(torch.from_numpy(g))
    np.testing.assert_allclose(lref.forward(o, P, L, keep, s), emb.detach().numpy(), rtol=0, atol=1e-12)
    got = lref.backward(o, P, L, g, keep, s)
    for name in ('w1', 'b1', 'w2', 'b2', 'uemb'):
        np.testing.assert_allclose(got[f'grad_{name}'], t[name].grad.numpy(), rtol=0, atol=1e-11, err_msg=name)
    zeros = lambda x: np.zeros_like(x.detach().numpy())
    if zero_latent:
        assert la.grad is None and not got['grad_lat_a'].any() and not got['grad_lat_b'].any() and not got['grad_w1'][:, F + 64:].any()
    elif same:      # one table: the source sum + the destination sum
        np.testing.assert_allclose(got['grad_lat_a'] + got['grad_lat_b'], la.grad.numpy(), rtol=0, atol=1e-11)
    else:
        np.testing.assert_allclose(got['grad_lat_a'], la.grad.numpy() if la.grad is not None else zeros(la), rtol=0, atol=1e-11)
        np.testing.assert_allclose(got['grad_lat_b'], lb.grad.numpy() if lb.grad is not None else zeros(lb), rtol=0, atol=1e-11)
    # the fp32 evaluation of the same expressions is an fp32 distance away, not more
    e32 = np.abs(lref.forward(o, P, L, keep, s, dtype=np.float32) - emb.detach().numpy()).max()
    assert 0 < e32 < 1e-4


def _straight_through_gumbel(logits, temperature, u):
    """the straight-through Gumbel softmax in torch autograd from given uniforms u, [D, n] with the classes last (what models/layers.py:152-181 of the
    reference computes from its own torch.rand): the soft sample, and the one-hot of its argmax carrying the soft sample's gradient"""
    noise = -(-(u + 1e-20).log() + 1e-20).log()
    soft = ((logits + noise) / temperature).softmax(-1)
    hard = torch.nn.functional.one_hot(soft.argmax(-1), soft.shape[-1]).to(soft.dtype)
    return (hard - soft).detach() + soft, soft


@pytest.mark.parametrize('T', [1.0, 0.3])
def test_gumbel_restatement_equals_autograd_of_the_composition(T):
    """per graph the reference calls gumbel_softmax(cat([logit_l[mask], logit_r[mask]]).T, T): [D, n] with the nodes as classes"""
    rng = np.random.default_rng(5)
    D, n = 2, 23
    logits = rng.standard_normal((D, n))
    u = np.stack([lref.gumbel_uniforms(7, 0xABCDEF0123456789, 3, 11, d, n) for d in range(D)])
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == u.size
    lt = torch.tensor(logits, requires_grad=True)
    out, y = _straight_through_gumbel(lt, T, torch.tensor(u.astype(np.float64)))
    g = rng.standard_normal((D, n))
    out.backward(torch.tensor(g))
    for d in range(D):
        got_out, got_y, k = lref.gumbel_forward(logits[d], u[d], T)
        np.testing.assert_allclose(got_y, y[d].detach().numpy(), rtol=0, atol=1e-14)
        np.testing.assert_allclose(got_out, out[d].detach().numpy(), rtol=0, atol=1e-14)
        assert k == int(y[d].argmax()) and abs(got_out[k] - 1) < 1e-15
        np.testing.assert_allclose(lref.gumbel_backward(got_y, g[d], T), lt.grad[d].numpy(), rtol=0, atol=1e-13)
    # the noise of a graph does not depend on how many nodes are asked for, and every field of the counter matters
    base = lref.gumbel_uniforms(7, 1, 0, 0, 0, 9)
    assert np.array_equal(lref.gumbel_uniforms(7, 1, 0, 0, 0, 300)[:9], base)
    for other in ((8, 1, 0, 0, 0), (7, 2, 0, 0, 0), (7, 1, 1, 0, 0), (7, 1, 0, 1, 0), (7, 1, 0, 0, 1)):
        assert not np.array_equal(lref.gumbel_uniforms(*other, 9), base)


def test_key_set_and_oracle_weights_load():
    """the DisCo-DiffDock-S configuration: the inference spec's keys, and the oracle's random weights of that configuration load strict"""
    from types import SimpleNamespace
    from disco_diffdock_amd.runtime import DEFAULTS
    from disco_diffdock_amd.score_model import TensorProductScoreModel
    from disco_diffdock_amd.train_model import LatentModelWrapper, TrainableScoreModel
    from oracle import score_model_ref as smr

    def inference_spec(latent_droprate):
        cfg = dict(DEFAULTS, ns=24, nv=6, num_conv_layers=5, batch_norm=1, no_torsion=0, lm_embedding_dim=1280, latent_dim=2, latent_vocab=1,
                   latent_droprate=latent_droprate)
        return TensorProductScoreModel.expected_state_dict_spec(SimpleNamespace(cfg=cfg, confidence_mode=False))
    kw = dict(sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True, lm_embedding_type='esm',
              latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    model = TrainableScoreModel(**kw)
    spec = inference_spec(0.1)
    state = model.state_dict()
    assert set(state) == set(spec)
    assert all(tuple(state[k].shape) == tuple(spec[k]) for k in spec)
    assert model.lig_edge_embedding[0].in_features == 72 and model.rec_edge_embedding[0].in_features == 68 and model.cross_edge_embedding[0].in_features == 68
    for k in ('lig_node', 'rec_node', 'lig_edge', 'rec_edge', 'cross_edge'):
        q = getattr(model, f'{k}_unconditional_embedding')
        assert q.shape == (1, 24) and q.requires_grad and not bool(q.any())      # zeros at init, as in the reference
    cfg = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1, lm_embedding_dim=1280)
    model.load_state_dict(smr.random_state_dict(cfg, seed=3), strict=True)
    # without a drop rate the five rows do not exist
    plain = TrainableScoreModel(**dict(kw, latent_droprate=0.0))
    assert not any('unconditional' in k for k in plain.state_dict())
    assert set(plain.state_dict()) == set(inference_spec(0.0))
    # what stays refused, by name
    for bad, name in ((dict(latent_vocab=32), 'latent_vocab'), (dict(latent_dim=0, latent_droprate=0.1), 'latent_droprate'), (dict(latent_dim=5), 'latent_dim'),
                      (dict(latent_cross_attention=True), 'latent_cross_attention')):
        with pytest.raises(RuntimeError, match=name):
            TrainableScoreModel(**dict(kw, **bad))
    with pytest.raises(RuntimeError, match='latent_droprate'):
        LatentModelWrapper(torch.nn.Identity(), model, 1.0, 0.0)
    with pytest.raises(RuntimeError, match='latent_dim'):
        LatentModelWrapper(torch.nn.Identity(), TrainableScoreModel(**dict(kw, latent_dim=0, latent_droprate=0.0)), 1.0, 0.0)


def test_workspace_ranges(built):
    from disco_diffdock_amd import _lib
    L = _lib.lib()
    ws = L.ddk_eemb_latent_workspace
    for E in (0, 1, 512, 513, 200000):
        for F in (0, 4):
            for NL in (1, 2, 3, 4):
                K = F + 64 + 2 * NL
                n = ws(E, K, NL)
                slices = E // max(512, ((E + 239) // 240 + 63) // 64 * 64) + 1
                pad = lambda v: (v + 3) // 4 * 4
                assert n == 4 * (pad(slices * (24 * (K + 1) + 24 * 25)) + pad(slices * 24) + 2 * pad(E * NL)), (E, K, NL)
                assert n % 16 == 0
                assert n - 8 * pad(E * NL) <= 4 * 241 * (24 * 77 + 24 * 25 + 24) + 64      # besides the [E, 2 L] rows: the images alone
    for bad in ((-1, 68, 2), (1 << 31, 68, 2), (10, 68, 0), (10, 74, 5), (10, 64, 2), (10, 69, 2), (10, 73, 2), (10, 76, 2), (10, 66, 2)):
        assert ws(*bad) == -1, bad
    assert ws(10, 66, 1) > 0 and ws(10, 76, 4) > 0
    assert L.ddk_eemb_workspace(10, 72) == -1      # the plain query keeps its range


def test_latent_keep_against_the_mirror(built):
    from disco_diffdock_amd import runtime, training
    ctx = runtime.Context(device=-1)
    names = [f'complex_{i}' for i in range(64)]
    streams = [runtime.stream_id(n) for n in names]
    assert runtime.RNG_LATENT_KEEP_PURPOSE == lref.KEEP_PURPOSE and runtime.RNG_GUMBEL_PURPOSE == lref.GUMBEL_PURPOSE and runtime.GUMBEL_TAG == lref.GUMBEL_TAG
    taken = set(runtime.RNG_PURPOSES.values()) | set(runtime.RNG_FORWARD_PURPOSES.values()) | {runtime.RNG_TIME_PURPOSE, 9, 10}
    assert not {12, 13} & taken
    for rate, draw, sample in ((0.1, 0, 0), (0.5, 7, 3), (0.0, 1, 0), (1.0, 1, 0)):
        got = ctx.latent_keep(5, streams, rate, draw=draw, sample=sample)
        assert got.dtype == np.float32 and np.array_equal(got, lref.latent_keep(5, streams, rate, draw, sample))
    assert ctx.latent_keep(5, streams, 0.0).all() and not ctx.latent_keep(5, streams, 1.0).any()
    half = ctx.latent_keep(5, streams, 0.5)
    assert 16 < half.sum() < 48 and not np.array_equal(half, ctx.latent_keep(6, streams, 0.5)) and not np.array_equal(half, ctx.latent_keep(5, streams, 0.5, draw=1))
    # a complex's flag does not depend on the batch it sits in; training.draw_latent_keep is the same call by name
    assert np.array_equal(ctx.latent_keep(5, streams[10:20], 0.5), half[10:20])
    assert np.array_equal(training.draw_latent_keep([dict(name=n) for n in names], 0.5, 5, 0), half)
    mixed = training.draw_latent_keep([dict(name=n) for n in names[:4]], 0.5, 5, 2, samples=[0, 1, 0, 1])
    assert np.array_equal(mixed, [lref.latent_keep(5, [streams[i]], 0.5, 2, s)[0] for i, s in enumerate((0, 1, 0, 1))])
    with pytest.raises(RuntimeError, match='draw'):
        ctx.latent_keep(5, streams, 0.5, draw=1 << 20)
    with pytest.raises(RuntimeError, match='rate'):
        ctx.latent_keep(5, streams, 1.5)
    # the header states the layout
    import os
    import re
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'ddk.h')).read()
    assert '#define DDK_GUMBEL_LAYOUT 1' in header and re.search(r'#define DDK_GUMBEL_TAG 0x47554D42u', header) and '#define DDK_RNG_LAYOUT 1' in header
    assert re.search(r'^ \*\s+12 latent keep', header, re.M) and re.search(r'^ \*\s+13 Gumbel noise', header, re.M)
