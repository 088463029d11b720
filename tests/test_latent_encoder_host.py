"""Host tests of the second tensor-product shape family (ns = 24, nv = 4) and of latent_encoder.TPEncoder's constructor: the shapes, the family ids, the
state-dict keys of the reference's module (written out here from its constructor, models/latent_encoder.py:17-169), the refusals, the workspace functions."""
import pytest
import torch

from disco_diffdock_amd import _lib
from disco_diffdock_amd.runtime import TP_NV4, tp_id_shape, tp_layer_shape
from disco_diffdock_amd.tensor_layers import FasterTensorProduct, TensorProductConvLayer, layer_index

NV4_W = (672, 800, 928, 1600, 1600)
LIG_TABLES = (119, 4, 12, 12, 8, 10, 6, 6, 2, 8, 2, 2, 2, 2, 2, 2)      # datasets_utils/process_mols.py:62-79
REC_TABLES = (38,)


def _seq(nv, ns=24):
    return [f'{ns}x0e', f'{ns}x0e + {nv}x1o', f'{ns}x0e + {nv}x1o + {nv}x1e', f'{ns}x0e + {nv}x1o + {nv}x1e + {ns}x0o']


def test_nv4_shapes():
    assert TP_NV4 == 8
    assert tuple(tp_layer_shape(l, 24, 4)['W'] for l in range(5)) == NV4_W
    s = tp_layer_shape(2, 24, 4)
    assert (s['A'], s['P'], s['Q'], s['C']) == (24, 4, 4, 0) and s['O'] == (24, 4, 4, 24) and (s['din'], s['dout']) == (48, 72)
    for l in range(5):
        assert tp_id_shape(TP_NV4 + l) == tp_layer_shape(l, 24, 4) and tp_id_shape(l) == tp_layer_shape(l, 24, 6)


def test_layer_index_names_the_family():
    for nv, base in ((4, TP_NV4), (6, 0)):
        seq = _seq(nv)
        assert [layer_index(seq[min(l, 3)], seq[min(l + 1, 3)]) for l in range(5)] == [base, base + 1, base + 2, base + 3, base + 3]
    seq = _seq(5)
    for l in range(4):
        with pytest.raises(RuntimeError, match='no fused kernel'):
            layer_index(seq[l], seq[min(l + 1, 3)])
    with pytest.raises(RuntimeError, match='no fused kernel'):
        layer_index(_seq(4)[1], _seq(6)[2])      # the two families do not mix
    tp = FasterTensorProduct(_seq(4)[2], '1x0e+1x1o', _seq(4)[3])
    assert tp.layer == TP_NV4 + 2 and tp.weight_numel == 928 and tp.out_size == 72
    layer = TensorProductConvLayer(_seq(4)[3], '1x0e+1x1o', _seq(4)[3], 72, hidden_features=72, residual=True, batch_norm=True, faster=True, edge_groups=4)
    assert layer.layer == TP_NV4 + 3 and layer.fc[0][4].out_features == 1600 and layer.batch_norm.weight.shape == (56,)


def _expected_keys(L, nv, latent_dim, hidden, latent_batchnorm, batch_norm=True, esm=False):
    ns, spec = 24, {}

    def lin(name, o, i):
        spec[f'{name}.weight'], spec[f'{name}.bias'] = (o, i), (o,)

    for side, tables, extra in (('lig', LIG_TABLES, 0), ('rec', REC_TABLES, 1280 if esm else 0)):
        for i, n in enumerate(tables):
            spec[f'{side}_node_embedding.atom_embedding_list.{i}.weight'] = (n, ns)
        if extra:      # models/layers.py:137: the Linear exists only with additional features; the encoder has no sigma block, so that is ESM alone
            lin(f'{side}_node_embedding.additional_features_embedder', ns, ns + extra)
    for side, k in (('lig', 4 + 32), ('rec', 32), ('cross', 32)):
        lin(f'{side}_edge_embedding.0', ns, k)
        lin(f'{side}_edge_embedding.3', ns, ns)
        spec[f'{side}_distance_expansion.offset'] = (32,)
    seq = [(ns, 0, 0, 0), (ns, nv, 0, 0), (ns, nv, nv, 0), (ns, nv, nv, ns)]
    for l in range(L):
        (A, P, Q, C), O = seq[min(l, 3)], seq[min(l + 1, 3)]
        W = sum(r * o for r, o in zip((A + P, A + P + Q, P + Q + C, Q + C), O))
        for g in range(4):
            lin(f'conv_layers.{l}.fc.{g}.0', 72, 72)
            lin(f'conv_layers.{l}.fc.{g}.4', W, 72)
        if batch_norm:
            spec[f'conv_layers.{l}.batch_norm.weight'] = spec[f'conv_layers.{l}.batch_norm.running_var'] = (sum(O),)
            spec[f'conv_layers.{l}.batch_norm.bias'] = spec[f'conv_layers.{l}.batch_norm.running_mean'] = (O[0],)      # e3nn: the 0e scalars alone
    for p in ('latent_s_predictor', 'latent_r_predictor'):
        lin(f'{p}.0', hidden, 2 * ns if L >= 3 else ns)
        lin(f'{p}.4', hidden, hidden)
        lin(f'{p}.8', latent_dim, hidden)
        if latent_batchnorm:
            for i in (1, 5):
                for k in ('weight', 'bias', 'running_mean', 'running_var'):
                    spec[f'{p}.{i}.{k}'] = (hidden,)
                spec[f'{p}.{i}.num_batches_tracked'] = ()
    return spec


@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('no_bn', [False, True])
def test_state_dict_keys_are_the_references(L, no_bn):
    from disco_diffdock_amd.latent_encoder import TPEncoder
    enc = TPEncoder(None, 2, 1, sh_lmax=1, ns=24, nv=4, num_conv_layers=L, latent_no_batchnorm=no_bn, latent_hidden_dim=96)
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    want = _expected_keys(L, 4, 2, 96, not no_bn)
    assert got == want, (sorted(set(got) ^ set(want)), {k: (got[k], want[k]) for k in set(got) & set(want) if got[k] != want[k]})
    assert [l.layer for l in enc.conv_layers] == [TP_NV4 + min(l, 3) for l in range(L)]


def test_state_dict_keys_nv6_esm_and_the_wrapper_prefixes():
    from disco_diffdock_amd.latent_encoder import TPEncoder
    from disco_diffdock_amd.train_model import LatentModelWrapper, TrainableScoreModel
    enc = TPEncoder(None, 3, 1, sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lm_embedding_type='esm', batch_norm=False)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == _expected_keys(5, 6, 3, 128, True, batch_norm=False, esm=True)
    score = TrainableScoreModel(sh_lmax=1, ns=24, nv=6, num_conv_layers=3, latent_dim=3, latent_vocab=1)
    keys = set(LatentModelWrapper(enc, score).state_dict())
    assert keys == {'encoder.' + k for k in enc.state_dict()} | {'score_model.' + k for k in score.state_dict()}


REFUSED = [('sh_lmax', 2), ('ns', 16), ('nv', 5), ('num_conv_layers', 0), ('num_conv_layers', 6), ('latent_vocab', 32), ('latent_dim', 0), ('latent_dim', 5),
           ('input_latent_dim', 2), ('use_oracle', False), ('latent_virtual_nodes', True), ('latent_nodes_residual', True), ('use_second_order_repr', True),
           ('distance_embed_dim', 64), ('cross_distance_embed_dim', 16), ('in_lig_edge_features', 5), ('lm_embedding_type', 'other'), ('dropout', 1.0),
           ('latent_dropout', -0.1)]


@pytest.mark.parametrize('name,value', REFUSED)
def test_refused_arguments_are_named(name, value):
    from disco_diffdock_amd.latent_encoder import TPEncoder
    kw = dict(latent_dim=2, latent_vocab=1, sh_lmax=1, ns=24, nv=4, num_conv_layers=3)
    kw[name] = value
    with pytest.raises(RuntimeError, match=rf'TPEncoder: {name} '):
        TPEncoder(None, **kw)


def test_reference_defaults_out_of_range_are_refused():
    from disco_diffdock_amd.latent_encoder import TPEncoder
    with pytest.raises(RuntimeError, match='TPEncoder: sh_lmax'):
        TPEncoder(None, 2, 1)      # the reference's defaults are sh_lmax=2, ns=16


def test_workspace_functions_take_the_family_ids():
    L = _lib.lib()
    for l in range(5):
        w4, w6 = L.ddk_rtp_backward_workspace(TP_NV4 + l, 1000, 4), L.ddk_rtp_backward_workspace(l, 1000, 4)
        assert w4 > 0 and w4 * tp_layer_shape(l, 24, 6)['W'] == w6 * NV4_W[l]      # slices x W x 73 floats: proportional to W
        s = tp_layer_shape(l, 24, 4)
        fwd, bwd = L.ddk_rconv_workspace(TP_NV4 + l, 1000, 4, 50, 40, 0), L.ddk_rconv_workspace(TP_NV4 + l, 1000, 4, 50, 40, 1)
        assert 4 * 1000 * s['dout'] <= fwd < 4 * 1000 * s['dout'] + 4096
        assert bwd >= w4 + 4 * (40 * s['dout'] + 1000 * s['din'])
    for bad in (5, 6, 7, 13, -1):
        assert L.ddk_rtp_backward_workspace(bad, 1000, 4) == -1 and L.ddk_rconv_workspace(bad, 1000, 4, 50, 40, 1) == -1
    assert L.ddk_rtp_backward_workspace(TP_NV4, 1000, 5) == -1 and L.ddk_rtp_backward_workspace(TP_NV4, -1, 4) == -1


def test_get_trainable_model_builds_the_wrapper():
    from types import SimpleNamespace
    from disco_diffdock_amd.latent_encoder import TPEncoder
    from disco_diffdock_amd.model_utils import get_trainable_model
    from disco_diffdock_amd.train_model import LatentModelWrapper, TrainableScoreModel
    args = SimpleNamespace(no_torsion=False, num_conv_layers=3, max_radius=5.0, scale_by_sigma=True, sigma_embed_dim=32, ns=24, nv=6, distance_embed_dim=32,
                           cross_distance_embed_dim=32, no_batch_norm=False, dropout=0.1, sh_lmax=1, use_second_order_repr=False, cross_max_distance=80,
                           dynamic_max_cross=True, esm_embeddings_path='x', use_old_atom_encoder=False, embedding_scale=1000, tr_sigma_min=0.1,
                           tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14, embedding_type='sinusoidal')
    assert isinstance(get_trainable_model(args, torch.device('cpu')), TrainableScoreModel)
    lat = SimpleNamespace(**vars(args), latent_dim=2, latent_vocab=1, latent_droprate=0.1, encoder_ns=24, encoder_nv=4, encoder_num_conv_layers=3,
                          encoder_cross_max_distance=40.0, encoder_no_esm=True, latent_no_batchnorm=False, latent_dropout=0.05, latent_hidden_dim=64,
                          latent_virtual_nodes=False, latent_nodes_residual=False, training_latent_temperature=0.7)
    model = get_trainable_model(lat, torch.device('cpu'))
    assert isinstance(model, LatentModelWrapper) and isinstance(model.encoder, TPEncoder) and model.training_latent_temperature == 0.7
    enc = model.encoder
    assert (enc.nv, enc.num_conv_layers, enc.cross_max_distance, enc.latent_dim) == (4, 3, 40.0, 2)
    assert not hasattr(enc.rec_node_embedding, 'additional_features_embedder') and not hasattr(enc.lig_node_embedding, 'additional_features_embedder')      # encoder_no_esm
    assert not any('additional_features_embedder' in k for k in enc.state_dict())
    with_esm = get_trainable_model(SimpleNamespace(**dict(vars(lat), encoder_no_esm=False)), torch.device('cpu')).encoder
    assert with_esm.rec_node_embedding.additional_features_embedder.in_features == 24 + 1280 and not hasattr(with_esm.lig_node_embedding, 'additional_features_embedder')
    assert enc.latent_s_predictor[0].out_features == 64 and enc.latent_s_predictor[3].p == 0.05
    with pytest.raises(RuntimeError, match='latent_vocab'):
        get_trainable_model(SimpleNamespace(**dict(vars(lat), latent_vocab=32)), torch.device('cpu'))
    with pytest.raises(RuntimeError, match='TPEncoder: latent_virtual_nodes'):
        get_trainable_model(SimpleNamespace(**dict(vars(lat), latent_virtual_nodes=True)), torch.device('cpu'))
