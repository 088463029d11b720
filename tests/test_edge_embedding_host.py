"""CPU tests of the host side of the edge embedding and of the trainable score model: the fp64 restatement the kernels are measured against
(tests/edge_embedding_ref.py) equals torch autograd of the plain composition it replaces, the mask layout of include/ddk.h restated with
tests/philox_ref.py keeps what a dropout of rate p keeps, ddk_eemb_workspace states its ranges, the batched graph builder of
disco_diffdock_amd/train_model.py gives the oracle's edge lists, and TrainableScoreModel holds the reference's key set and refuses what it does not build."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import edge_embedding_ref as ref
from helpers import to_graph
from oracle import cluster_lite, graph_lite


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def _case(seed, E, K, start, stop):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape)
    n_a, n_b, T = 7, 11, 3
    o = dict(pos_a=f(n_a, 3) * stop / 4, pos_b=f(n_b, 3) * stop / 4, idx_a=rng.integers(0, n_a, E), idx_b=rng.integers(0, n_b, E),
             feat=np.eye(4)[rng.integers(0, 4, E)] if K == 68 else None, sig=f(T, 32), sig_index=rng.integers(0, T, n_a), start=start, stop=stop)
    P = dict(w1=f(24, K) / np.sqrt(K), b1=f(24) * 0.5, w2=f(24, 24) / np.sqrt(24.0), b2=f(24))
    return o, P, f(E, 24)


@pytest.mark.parametrize('p', [0.0, 0.25])
@pytest.mark.parametrize('K,stop', [(68, 5.0), (64, 30.0)])
def test_restatement_equals_autograd_of_the_composition(K, stop, p):
    E = 41
    o, P, g = _case(7 + K, E, K, 0.0, stop)
    keep, s = ref.keep_mask(1234, E, p), ref.scale(p)
    assert (p == 0 and s == 1.0 and keep.all()) or (p > 0 and abs(s - 1 / (1 - p)) < 1e-7 and not keep.all() and keep.any())
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    T = lambda a: torch.as_tensor(np.asarray(a))
    # the plain composition (models/score_model.py:310-344 for one group): gathers, norm, smearing, cat, Linear, ReLU, mask, Linear
    vec = T(o['pos_b'])[T(o['idx_b'])] - T(o['pos_a'])[T(o['idx_a'])]
    d = vec.norm(dim=-1)
    offset = torch.linspace(0.0, stop, 32)
    assert np.array_equal(offset.numpy(), ref.offsets(0.0, stop))      # the header's formula IS torch.linspace's, in fp32
    coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
    assert np.float32(coeff) == np.float32(ref.coeff(0.0, stop))
    smear = torch.exp(ref.coeff(0.0, stop) * (d[:, None] - offset.double()[None, :]) ** 2)
    row = torch.cat(([T(o['feat'])] if K == 68 else []) + [T(o['sig'])[T(o['sig_index'])[T(o['idx_a'])]], smear], 1)
    hid = torch.relu(torch.nn.functional.linear(row, t['w1'], t['b1'])) * torch.from_numpy(keep) * s
    emb = torch.nn.functional.linear(hid, t['w2'], t['b2'])
    emb.backward(torch.from_numpy(g))
    unit = vec / d.clamp_min(1e-12)[:, None]
    sh = torch.cat([torch.ones(E, 1, dtype=torch.float64), np.sqrt(3.0) * unit], 1)      # heads._sh1
    got_emb, got_sh, got_hid = ref.forward(o, P['w1'], P['b1'], P['w2'], P['b2'], keep, s)
    np.testing.assert_allclose(got_emb, emb.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_sh, sh.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_hid, hid.detach().numpy(), rtol=0, atol=1e-12)
    got = ref.backward(o, P['w1'], P['b1'], P['w2'], g, keep, s)
    for name, a in zip(('w1', 'b1', 'w2', 'b2'), got):
        np.testing.assert_allclose(a, t[name].grad.numpy(), rtol=0, atol=1e-11, err_msg=name)
    # the margin is a bound of an fp32 evaluation of the pre-activation
    pre, margin = ref.pre_activation(o, P['w1'], P['b1'])
    row32 = row.detach().float()
    d32 = (T(o['pos_b']).float()[T(o['idx_b'])] - T(o['pos_a']).float()[T(o['idx_a'])]).norm(dim=-1)
    row32[:, -32:] = torch.exp(np.float32(coeff) * (d32[:, None] - offset[None, :]) ** 2)
    pre32 = torch.nn.functional.linear(row32, t['w1'].detach().float(), t['b1'].detach().float()).double().numpy()
    pos32 = dict(o, pos_a=np.asarray(o['pos_a'], np.float32), pos_b=np.asarray(o['pos_b'], np.float32), sig=np.asarray(o['sig'], np.float32))
    pre_of_fp32_inputs, margin = ref.pre_activation(pos32, P['w1'].astype(np.float32), P['b1'].astype(np.float32))
    assert (np.abs(pre32 - pre_of_fp32_inputs) <= margin).all() and (margin < 1e-4).all()


def test_mask_layout():
    import philox_ref
    E, p = 4096, 0.1
    keep = ref.keep_mask(20240607, E, p)
    n = keep.size
    assert keep.shape == (E, 24)
    sigma = np.sqrt(n * p * (1 - p))
    assert abs(int(keep.sum()) - n * (1 - p)) < 4 * sigma      # the keep rate of a dropout of rate p, within 4 sigma of the binomial
    assert ref.keep_mask(20240607, E, 0.0).all()      # p == 0 keeps everything
    assert np.array_equal(ref.keep_mask(20240607, 50, p, e0=1000), keep[1000:1050])      # a pure function of (seed, edge position, column)
    other = ref.keep_mask(20240608, E, p)
    assert 0.1 < float((other != keep).mean()) < 0.3      # two independent masks differ on 2 p (1 - p) = 18 % of the elements
    # the layout itself, for one element, written out: counter (e_lo, e_hi, c / 4, tag), word c % 4, kept iff (word >> 8) * 2^-24 >= p
    e, c, seed = (1 << 32) + 5, 18, (7 << 32) | 9
    words = philox_ref.philox4x32_10((5, 1, c // 4, 0x45454D42), (9, 7))
    u = np.float32(int(words[c % 4]) >> 8) * np.float32(2.0 ** -24)
    assert bool(ref.keep_mask(seed, 1, p, e0=e)[0, c]) == bool(u >= np.float32(p))
    # a tag of its own: the radial hidden layer's mask of the same seed and edge is another one
    import radial_hidden_ref
    assert ref.MASK_TAG != radial_hidden_ref.MASK_TAG
    assert not np.array_equal(keep[:, :24], radial_hidden_ref.keep_mask(20240607, E, p)[:, :24])


def test_workspace_ranges(built):
    from disco_diffdock_amd import _lib
    ws = _lib.lib().ddk_eemb_workspace
    img = lambda K: 24 * (K + 1) + 24 * 25      # grad_w1 with grad_b1 as column K, grad_w2 with grad_b2 as column 24
    assert ws(0, 64) == img(64) * 4 and ws(0, 68) == img(68) * 4
    assert ws(511, 68) == img(68) * 4 and ws(1300, 64) == 3 * img(64) * 4      # slices of 512 edges: E / 512 + 1 images, never anything per edge
    assert ws(800000, 68) == (800000 // 3392 + 1) * img(68) * 4      # longer slices once E > 122 880: at most 241 images
    big = ws((1 << 31) - 1, 68)
    assert 0 < big <= 241 * img(68) * 4
    for bad in ((-1, 64), (1 << 31, 64), (10, 0), (10, 72), (10, 66)):
        assert ws(*bad) == -1, bad


# ---- the batched graph builder ------------------------------------------------------------------------------------------------------------------------
def _three_complexes():
    """three synthetic complexes of different sizes, collated as the reference's loader collates them, each with its own time"""
    from disco_diffdock_amd import synthetic
    cs = [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in ((43, 24), (47, 37), (42, 30))]      # ligands of 16, 17 and 18 atoms
    b = graph_lite.collate([to_graph(c) for c in cs])
    b.complex_t = {k: torch.tensor([0.15, 0.3, 0.45]) for k in ('tr', 'rot', 'tor')}
    return cs, b


@pytest.mark.parametrize('dynamic', [False, True])
def test_graph_builder_gives_the_oracles_edge_lists(dynamic):
    from disco_diffdock_amd import train_model as tm
    from oracle import score_model_ref as smr
    cs, b = _three_complexes()
    lig, rec, B = b['ligand'], b['receptor'], b.num_graphs
    lig.pos = lig.pos + torch.tensor([12.0, 9.0, 0.0])      # the ligands 15 A off their pockets: part of every small receptor is out of reach
    assert len({len(c['lig_pos']) for c in cs}) == 3 and len({len(c['rec_pos']) for c in cs}) == 3
    cfg = smr.ScoreModelConfig(dynamic_max_cross=dynamic, cross_max_distance=18.0)
    if dynamic:
        tr_sigma = smr.t_to_sigma(b.complex_t['tr'], b.complex_t['rot'], b.complex_t['tor'], cfg)[0]
        cutoff = tr_sigma * 3 + 20
        want_cross = cluster_lite.radius(rec.pos / cutoff.unsqueeze(1)[rec.batch], lig.pos / cutoff.unsqueeze(1)[lig.batch], 1, rec.batch, lig.batch,
                                         max_num_neighbors=10000)
    else:
        cutoff = cfg.cross_max_distance
        want_cross = cluster_lite.radius(rec.pos, lig.pos, cutoff, rec.batch, lig.batch, max_num_neighbors=10000)
    want_radius = cluster_lite.radius_graph(lig.pos, cfg.lig_max_radius, lig.batch)
    # no cap binds on these inputs: every centre has fewer than 32 neighbours, every atom fewer than 10000 residues in reach
    assert int(torch.bincount(want_radius[1], minlength=lig.pos.shape[0]).max()) < 32
    assert int(torch.bincount(want_cross[0], minlength=lig.pos.shape[0]).max()) < 10000
    pairs = [len(c['lig_pos']) * len(c['rec_pos']) for c in cs]
    per_graph = torch.bincount(lig.batch[want_cross[0]], minlength=B).tolist()
    assert want_radius.shape[1] > 50 and all(0 < n < full for n, full in zip(per_graph, pairs)), (per_graph, pairs)      # the cutoffs cut, in every graph
    bonds, rec_edges = b['ligand', 'ligand'].edge_index, b['receptor', 'receptor'].edge_index
    lig_ei, cross_ei, rec_ei, n_bond = tm.build_conv_edges(lig.pos, lig.batch, rec.pos, rec.batch, bonds, rec_edges, B, cfg.lig_max_radius, cutoff)
    assert n_bond == bonds.shape[1]
    assert torch.equal(lig_ei, torch.cat([bonds, want_radius], 1)) and torch.equal(cross_ei, want_cross) and torch.equal(rec_ei, rec_edges)
    # the oracle's cat order over the node table [ligand | receptor], and its group sizes
    n_lig = lig.pos.shape[0]
    edge_index, sizes = tm.combine_edges(lig_ei, cross_ei, rec_ei, n_lig)
    lr = torch.stack([want_cross[0], want_cross[1] + n_lig])
    want = torch.cat([torch.cat([bonds, want_radius], 1), lr, rec_edges + n_lig, torch.flip(lr, dims=[0])], dim=1)
    assert torch.equal(edge_index, want) and sizes == (lig_ei.shape[1], lr.shape[1], rec_edges.shape[1], lr.shape[1])
    # and against the oracle's embed itself: the graph it convolves over
    P = smr.random_state_dict(smr.ScoreModelConfig(dynamic_max_cross=dynamic, cross_max_distance=18.0, num_conv_layers=1), seed=1)
    for nt in ('ligand', 'receptor'):
        b[nt].node_t = {k: b.complex_t[k][b[nt].batch] for k in ('tr', 'rot', 'tor')}
    graph = smr.embed(P, smr.ScoreModelConfig(dynamic_max_cross=dynamic, cross_max_distance=18.0, num_conv_layers=1), b, return_graph=True)[-1]
    assert torch.equal(graph['edge_index'], edge_index) and graph['splits'] == (sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2])


def test_radius_caps_and_order():
    """the rules oracle/cluster_lite.py states, where they bind: strict <, ascending index, the first max_num_neighbors, per graph"""
    from disco_diffdock_amd import train_model as tm
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(0, 1.2, (60, 3))).float()
    batch = torch.cat([torch.zeros(45, dtype=torch.long), torch.ones(15, dtype=torch.long)])
    x[7] = x[3] + torch.tensor([2.0, 0.0, 0.0])      # a pair at exactly the radius: excluded by the strict comparison
    for cap in (5, 32):
        want = cluster_lite.radius_graph(x, 2.0, batch, max_num_neighbors=cap)
        assert torch.equal(tm.radius_graph(x, 2.0, batch, 2, cap), want)
        if cap == 5:      # the cap binds: cap + 1 go into radius, the centre among them or not
            assert int(torch.bincount(want[1]).max()) in (cap, cap + 1) and int((torch.bincount(want[1]) >= cap).sum()) > 20
    got = tm.radius_graph(x, 2.0, batch, 2, 32)
    assert not bool(((got[0] == 3) & (got[1] == 7)).any()) and bool(((x[3] - x[7]).pow(2).sum() == 4.0))
    y = torch.from_numpy(rng.normal(0, 1.2, (9, 3))).float()
    by = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert torch.equal(tm.radius(x, y, 1.5, batch, by, 2, 4), cluster_lite.radius(x, y, 1.5, batch, by, max_num_neighbors=4))
    assert tm.radius(x[:0], y, 1.5, batch[:0], by, 2).shape == (2, 0)
    with pytest.raises(RuntimeError, match='grouped by graph'):
        tm.radius(x, y, 1.5, batch.flip(0), by, 2)


# ---- the module's key set, and what it refuses ---------------------------------------------------------------------------------------------------------------
CONFIG = dict(sh_lmax=1, ns=24, nv=6, num_conv_layers=5)


@pytest.mark.parametrize('batch_norm,no_torsion,lm', list(itertools.product((True, False), (False, True), (None, 'esm'))))
def test_key_set_is_the_inference_models(batch_norm, no_torsion, lm):
    from disco_diffdock_amd.runtime import DEFAULTS
    from disco_diffdock_amd.score_model import TensorProductScoreModel
    from disco_diffdock_amd.train_model import TrainableScoreModel
    model = TrainableScoreModel(batch_norm=batch_norm, no_torsion=no_torsion, lm_embedding_type=lm, dynamic_max_cross=True, dropout=0.1, **CONFIG)
    cfg = dict(DEFAULTS, ns=24, nv=6, num_conv_layers=5, batch_norm=int(batch_norm), no_torsion=int(no_torsion), lm_embedding_dim=1280 if lm else 0,
               latent_dim=0, latent_droprate=0.0)
    spec = TensorProductScoreModel.expected_state_dict_spec(SimpleNamespace(cfg=cfg, confidence_mode=False))
    state = model.state_dict()
    assert set(state.keys()) == set(spec.keys())
    assert {k: tuple(v.shape) for k, v in state.items()} == {k: tuple(v) for k, v in spec.items()}
    params = {k for k, _ in model.named_parameters()}
    buffers = {k for k in state if k.endswith(('.offset', '.running_mean', '.running_var'))}
    assert params | buffers == set(state) and not params & buffers      # everything but the expansions' offsets and BatchNorm's statistics trains
    # the oracle's random checkpoint of the same configuration loads strictly
    from oracle import score_model_ref as smr
    P = smr.random_state_dict(smr.ScoreModelConfig(batch_norm=batch_norm, no_torsion=no_torsion, lm_embedding_dim=1280 if lm else 0), seed=2)
    P = {k: v for k, v in P.items() if k in spec}
    model.load_state_dict(P, strict=True)
    # train / eval reach the heads' modules, which sit at top level
    model.eval()
    assert not model.final_conv.training and not model._heads.training and not model.conv_layers[0].training
    model.train()
    assert model.final_conv.training and model._heads.training and model.lig_edge_embedding[2].training


@pytest.mark.parametrize('option,value', [('sh_lmax', 2), ('ns', 16), ('nv', 4), ('latent_dim', 2), ('latent_droprate', 0.1), ('latent_cross_attention', True),
                                          ('use_old_atom_encoder', True), ('use_second_order_repr', True), ('confidence_mode', True),
                                          ('in_lig_edge_features', 5), ('sigma_embed_dim', 64), ('distance_embed_dim', 16), ('cross_distance_embed_dim', 16),
                                          ('lm_embedding_type', 'other'), ('num_conv_layers', 2), ('conv_kernel', 1), ('dropout', 1.0), ('no_such_option', 1)])
def test_unsupported_options_raise_and_name_the_option(option, value):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    with pytest.raises(RuntimeError, match=option):
        TrainableScoreModel(**dict(CONFIG, **{option: value}))


def test_reference_defaults_are_refused():
    """the reference's constructor defaults (sh_lmax=2, ns=16, nv=4) are not the supported model: nothing is built silently"""
    from disco_diffdock_amd.train_model import TrainableScoreModel
    with pytest.raises(RuntimeError, match='sh_lmax'):
        TrainableScoreModel()


def test_forward_refuses_the_host():
    from disco_diffdock_amd.train_model import TrainableScoreModel
    _, b = _three_complexes()
    with pytest.raises(RuntimeError, match='GPU only'):
        TrainableScoreModel(**CONFIG)(b)
