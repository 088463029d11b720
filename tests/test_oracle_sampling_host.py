"""Host side of the oracle-latent tests: the fp64 restatement (tests/oracle_latents_ref.py) at the seeds the GPU tests use - no (sample, dimension) is
closer to a tie than the gap those tests exclude, so they leave no case out, and the statistics case passes its chi-square - and ModelWrapper's routing of
``encoder.*`` / ``score_model.*`` keys, on CPU tensors with a stand-in score model."""
import numpy as np
import pytest
import torch

import oracle_latents_ref as olr
import philox_ref


def test_kernel_cases_have_no_near_tie():
    stream = philox_ref.fnv1a64(olr.STREAM_NAME)
    for n_lig, n_rec in olr.SHAPES:
        for D in olr.DIMS:
            logits = olr.case_logits(n_lig, n_rec, D)
            n = n_lig + n_rec
            if n >= 2:
                assert np.isneginf(logits[n // 2]).all() and np.isfinite(np.delete(logits, n // 2, axis=0)).all()
            if n >= 8:
                assert len(np.unique(logits[np.isfinite(logits)])) < np.isfinite(logits).sum()      # equal logits: the noise decides between them
            for B in olr.BATCHES:
                for sample0 in olr.SAMPLE0S:
                    picks, gaps = olr.host_picks(logits, olr.SEED, stream, sample0, B, draw=olr.DRAW)
                    assert (gaps > olr.GAP).all(), (n_lig, n_rec, D, B, sample0, float(gaps.min()))
                    assert ((picks >= 0) & (picks < n)).all() and (n < 2 or (picks != n // 2).all())
    # a sample's pick is keyed by its global index
    logits = olr.case_logits(7, 23, 4)
    a, b = olr.host_picks(logits, olr.SEED, stream, 0, 5, draw=olr.DRAW)[0], olr.host_picks(logits, olr.SEED, stream, 3, 2, draw=olr.DRAW)[0]
    assert (a[3:] == b).all()


def test_vectorised_uniforms_are_the_per_sample_ones():
    import latent_embedding_ref as lref
    u = olr.uniforms(5, 0x1234, [3, 4, 70000], 2, 1, 9)
    for row, sample in zip(u, (3, 4, 70000)):
        assert (row == lref.gumbel_uniforms(5, 0x1234, sample, 2, 1, 9)).all()


def test_statistics_case():
    stream = philox_ref.fnv1a64(olr.STREAM_NAME)
    picks, gaps = olr.host_picks(olr.STAT_LOGITS[:, None], olr.STAT_SEED, stream, 0, olr.STAT_B)
    assert (gaps > olr.GAP).all()
    assert olr.chi_square(picks, olr.STAT_LOGITS) < olr.STAT_CHI2
    # what the bound is there to catch: one pick for every sample (a key without the sample index)
    assert olr.chi_square(np.repeat(picks[:1], olr.STAT_B, axis=0), olr.STAT_LOGITS) > olr.STAT_CHI2


def test_sampling_case_has_no_near_tie():
    c = olr.sampling_complex()
    logits = olr.logits64(olr.host_encoder(), c)
    assert logits.shape == (olr.COMPLEX['n_lig'] + len(c['rec_pos']), 2) and np.isfinite(logits).all()
    picks, gaps = olr.host_picks(logits, olr.SAMPLING_SEED, philox_ref.fnv1a64(c['name']), 0, olr.SAMPLES)
    assert (gaps > olr.SAMPLING_GAP).all(), float(gaps.min())
    assert len({tuple(p) for p in picks.tolist()}) > 1


class _StubScoreModel(torch.nn.Module):
    """records what ModelWrapper hands to the score model"""

    def __init__(self):
        super().__init__()
        self.cfg, self.seen = dict(latent_dim=2), None

    def load_state_dict(self, state_dict, strict=True):
        self.seen = (sorted(state_dict), strict)
        return torch.nn.modules.module._IncompatibleKeys([], [])


def test_model_wrapper_routes_the_keys():
    from disco_diffdock_amd.latent_encoder import TPEncoder
    from disco_diffdock_amd.score_model import ModelWrapper
    enc_state = olr.host_encoder().state_dict()
    built = []

    def factory():
        built.append(TPEncoder(None, **olr.ENCODER).train())
        return built[-1]

    full = {**{'score_model.a.weight': torch.zeros(2), 'score_model.b': torch.ones(1)}, **{'encoder.' + k: v for k, v in enc_state.items()}}
    # a bare state dict and a wrapped one without encoder keys: no encoder is built
    m = ModelWrapper(None, _StubScoreModel(), encoder_factory=factory)
    m.load_state_dict({'a.weight': torch.zeros(2), 'b': torch.ones(1)})
    assert m.encoder is None and not built and m.score_model.seen == (['a.weight', 'b'], True)
    m.load_state_dict({k: v for k, v in full.items() if k.startswith('score_model.')})
    assert m.encoder is None and not built and m.score_model.seen == (['a.weight', 'b'], True)
    # encoder keys: built once, in eval, loaded with the caller's strict; a second load goes into the same module
    res = m.load_state_dict(full, strict=True)
    assert len(built) == 1 and m.encoder is built[0] and not m.encoder.training and not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, enc_state[k]) for k, v in m.encoder.state_dict().items()) and m.score_model.seen == (['a.weight', 'b'], True)
    assert 'encoder.latent_s_predictor.0.weight' in m.state_dict()
    m.load_state_dict(full, strict=True)
    assert len(built) == 1
    short = {k: v for k, v in full.items() if k != 'encoder.latent_r_predictor.0.bias'}
    with pytest.raises(RuntimeError, match='latent_r_predictor.0.bias'):
        m.load_state_dict(short, strict=True)
    res = m.load_state_dict(short, strict=False)
    assert res.missing_keys == ['encoder.latent_r_predictor.0.bias'] and m.score_model.seen[1] is False
    with pytest.raises(RuntimeError, match='unexpected keys'):
        m.load_state_dict(dict(full, **{'other.weight': torch.zeros(1)}), strict=True)
    assert m.load_state_dict(dict(full, **{'other.weight': torch.zeros(1)}), strict=False).unexpected_keys == ['other.weight']
    # without a factory the keys cannot be placed; attach_encoder takes a live encoder of the model's latent_dim, nothing else
    bare = ModelWrapper(None, _StubScoreModel())
    with pytest.raises(RuntimeError, match='cannot build the encoder'):
        bare.load_state_dict(full)
    live = olr.host_encoder().train()
    assert bare.attach_encoder(live).encoder is live and not live.training
    bare.load_state_dict(full, strict=True)
    with pytest.raises(RuntimeError, match='TPEncoder'):
        bare.attach_encoder(torch.nn.Linear(1, 1))
    with pytest.raises(RuntimeError, match='latent_dim'):
        bare.attach_encoder(TPEncoder(None, **dict(olr.ENCODER, latent_dim=3)))
    # a configuration the encoder refuses raises by name when the checkpoint asks for the encoder
    refused = ModelWrapper(None, _StubScoreModel(), encoder_factory=lambda: TPEncoder(None, **dict(olr.ENCODER, latent_virtual_nodes=True)))
    with pytest.raises(RuntimeError, match='latent_virtual_nodes'):
        refused.load_state_dict(full)


def test_get_model_keeps_what_the_encoder_needs():
    """model_utils._oracle_encoder reads the Namespace as get_trainable_model always did: one constructor for both"""
    from argparse import Namespace
    from disco_diffdock_amd.latent_encoder import TPEncoder
    from disco_diffdock_amd.model_utils import _oracle_encoder
    args = Namespace(no_torsion=False, max_radius=5.0, distance_embed_dim=32, cross_distance_embed_dim=32, no_batch_norm=False, dropout=0.1, sh_lmax=1,
                     use_second_order_repr=False, esm_embeddings_path='x', latent_dim=2, latent_vocab=1, encoder_ns=24, encoder_nv=4,
                     encoder_num_conv_layers=3, encoder_cross_max_distance=80, latent_hidden_dim=64)
    enc = _oracle_encoder(args, None)
    assert isinstance(enc, TPEncoder) and (enc.nv, enc.num_conv_layers, enc.latent_dim, enc.cross_max_distance) == (4, 3, 2, 80.0)
    assert enc.latent_s_predictor[0].out_features == 64 and enc.rec_node_embedding.additional_features_dim == 1280
    assert _oracle_encoder(Namespace(**dict(vars(args), encoder_no_esm=True)), None).rec_node_embedding.additional_features_dim == 0
    with pytest.raises(RuntimeError, match='nv'):
        _oracle_encoder(Namespace(**dict(vars(args), encoder_nv=5)), None)
