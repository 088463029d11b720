"""Host tests of the AR latent model's training side (disco_diffdock_amd.ar_training, pretrained_score_encoder.TrainablePretrainedScoreEncoder,
model_utils.get_ar_model(training=True)): the cross-entropy restatement of tests/node_cross_entropy_ref.py against torch's F.cross_entropy, the decoding
index of generator purpose 14, the input-latent masking rule, the state-dict key set, the refusals by argument name."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import node_cross_entropy_ref as nref
import philox_ref as pr

SHAPES = ((1, 0), (0, 5), (3, 2), (7, 58), (30, 129))


def _batch(D, seed=3):
    rng = np.random.default_rng(seed)
    n_l, n_r = [s[0] for s in SHAPES], [s[1] for s in SHAPES]
    lig_ptr, rec_ptr = np.concatenate([[0], np.cumsum(n_l)]), np.concatenate([[0], np.cumsum(n_r)])
    logit_l, logit_r = rng.normal(0, 3, lig_ptr[-1]), rng.normal(0, 3, rec_ptr[-1])
    teacher_l, teacher_r = rng.normal(0, 2, (lig_ptr[-1], D)), rng.normal(0, 2, (rec_ptr[-1], D))
    column = np.asarray([(g + 1) % D for g in range(len(SHAPES))])
    return logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, rng.normal(0, 1, len(SHAPES))


@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('D', [1, 4])
def test_restatement_against_torch_cross_entropy(D, soft):
    """per graph, as train_ar.py:120-125 calls it: F.cross_entropy(logits [n], class index) in hard mode, F.cross_entropy(logits [1, n], probabilities
    [1, n]) with the label softmax(teacher) in soft mode; fp64 on the CPU, loss and gradient"""
    b = _batch(D)
    loss, pick, target, g_l, g_r = nref.node_cross_entropy(*b[:7], soft, grad=b[7])
    s_l, s_r = torch.tensor(b[0], requires_grad=True), torch.tensor(b[1], requires_grad=True)
    total = 0
    for g in range(len(SHAPES)):
        s = torch.cat([s_l[b[2][g]:b[2][g + 1]], s_r[b[3][g]:b[3][g + 1]]])
        t = torch.tensor(nref.graph_rows(b[4], b[5], b[2], b[3], g)[:, b[6][g]])
        want = F.cross_entropy(s[None], torch.softmax(t, 0)[None]) if soft else F.cross_entropy(s, torch.argmax(t))
        assert abs(want.item() - loss[g]) <= 1e-12 * max(1.0, abs(want.item())), (g, want.item(), loss[g])
        assert pick[g] == int(torch.argmax(s)) and target[g] == int(torch.argmax(t))
        total = total + want * b[7][g]
    total.backward()
    assert np.abs(s_l.grad.numpy() - g_l).max() <= 1e-12 and np.abs(s_r.grad.numpy() - g_r).max() <= 1e-12


def test_restatement_ties_and_fp32():
    s, t = np.asarray([0.0, 2.0, -1.0, 2.0]), np.asarray([1.0, 5.0, 5.0, 0.0])
    loss, d, pick, target = nref.graph_cross_entropy(s, t, False)
    assert (pick, target) == (1, 1) and abs(d.sum()) < 1e-15      # the lowest position of a tie; softmax - one-hot sums to 0
    loss32, d32, _, _ = nref.graph_cross_entropy(s, t, True, dtype=np.float32)
    assert loss32.dtype == np.float32 and d32.dtype == np.float32
    one = nref.graph_cross_entropy(np.asarray([3.5]), np.asarray([-2.0]), False)
    assert one[0] == 0.0 and one[1][0] == 0.0      # a single node: loss 0, gradient 0


def test_decoding_index_word_layout_and_range():
    """purpose 14, step = draw, block 0, word 0, sample 0: idx = ((word >> 8) * D) >> 24, against the Philox restatement; a pure function of (name, seed,
    draw); in 0 .. D - 1 for D = 1..4, every value taken over 64 names"""
    from disco_diffdock_amd import ar_training, runtime
    assert runtime.RNG_DECODING_INDEX_PURPOSE == 14
    taken = set(runtime.RNG_PURPOSES.values()) | set(runtime.RNG_FORWARD_PURPOSES.values()) | set(runtime.RNG_MATCH_PURPOSES.values()) | \
        {runtime.RNG_TIME_PURPOSE, runtime.RNG_LATENT_KEEP_PURPOSE, runtime.RNG_GUMBEL_PURPOSE}
    assert runtime.RNG_DECODING_INDEX_PURPOSE not in taken and runtime.RNG_LAYOUT == 1
    names = [f'complex_{i}' for i in range(64)]
    for D in (1, 2, 3, 4):
        for seed, draw in ((0, 0), (7, 3), ((1 << 64) - 1, (1 << 20) - 1)):
            idx = ar_training.draw_decoding_idx(names, D, seed, draw)
            assert idx.dtype == np.int32 and idx.shape == (64,)
            words = [int(pr.block(seed, pr.fnv1a64(n), np.array([0]), 14, draw, 0)[0, 0]) for n in names]
            assert idx.tolist() == [((w >> 8) * D) >> 24 for w in words]
            assert set(idx.tolist()) == set(range(D)), (D, seed, draw)
            assert np.array_equal(ar_training.draw_decoding_idx(names[::-1], D, seed, draw), idx[::-1])      # whatever the neighbours
            assert np.array_equal(ar_training.draw_decoding_idx(names[5:9], D, seed, draw), idx[5:9])
    assert not np.array_equal(ar_training.draw_decoding_idx(names, 4, 7, 3), ar_training.draw_decoding_idx(names, 4, 7, 4))
    assert not np.array_equal(ar_training.draw_decoding_idx(names, 4, 7, 3), ar_training.draw_decoding_idx(names, 4, 8, 3))
    assert ar_training.draw_decoding_idx([], 2, 1, 0).shape == (0,)
    for D in (0, 5):
        with pytest.raises(ValueError, match='D must be in 1..4'):
            ar_training.draw_decoding_idx(names, D, 1, 0)
    with pytest.raises(RuntimeError, match=r'ddk_rng_decoding_index: draw'):
        ar_training.draw_decoding_idx(names, 2, 1, 1 << 20)


def test_input_latent_masking_rule():
    """dataset_ar.py:117-119: the columns at or past the decoding index are zeroed, those before it kept; index 0 leaves nothing"""
    from disco_diffdock_amd import ar_training
    label = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    for k in range(4):
        got = ar_training.mask_input_latent(label, k)
        assert np.array_equal(got[:, :k], label[:, :k]) and (got[:, k:] == 0).all() and got is not label
    assert (label > 0).all()      # the label itself is left alone
    # the collated form of the reference module agrees
    lig_ptr, rec_ptr = [0, 2, 3], [0, 1, 3]
    l, r = np.ones((3, 4), np.float32), np.ones((3, 4), np.float32)
    ml, mr = nref.mask_input_latent(l, r, lig_ptr, rec_ptr, [1, 3])
    assert np.array_equal(ml[:2], ar_training.mask_input_latent(l[:2], 1)) and np.array_equal(ml[2:], ar_training.mask_input_latent(l[2:], 3))
    assert np.array_equal(mr[:1], ar_training.mask_input_latent(r[:1], 1)) and np.array_equal(mr[1:], ar_training.mask_input_latent(r[1:], 3))


SCORE = dict(sh_lmax=1, ns=24, nv=6, num_conv_layers=3, latent_dim=2, latent_vocab=1)


def _score(**kw):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    return TrainableScoreModel(**dict(SCORE, **kw))


@pytest.mark.parametrize('no_bn,ns,droprate', [(False, 24, 0.0), (True, 16, 0.1)])
def test_state_dict_keys_are_the_inference_class_keys(no_bn, ns, droprate):
    """state_dict().keys() == the pretrained_score_model.-prefixed key set of the inference spec plus PretrainedScoreEncoder.predictor_spec()"""
    from disco_diffdock_amd.pretrained_score_encoder import PretrainedScoreEncoder, TrainablePretrainedScoreEncoder
    from disco_diffdock_amd.score_model import TensorProductScoreModel
    sm = _score(latent_droprate=droprate, lm_embedding_type='esm')
    ar = TrainablePretrainedScoreEncoder(sm, ns=ns, latent_dim=1, latent_vocab=1, latent_no_batchnorm=no_bn, latent_hidden_dim=96, input_latent_dim=2,
                                         apply_gumbel_softmax=False)
    cfg = dict(ns=24, nv=6, num_conv_layers=3, sigma_embed_dim=32, distance_embed_dim=32, lm_embedding_dim=1280, latent_dim=2, latent_droprate=droprate,
               batch_norm=1, no_torsion=0)
    spec = {'pretrained_score_model.' + k: tuple(v) for k, v in
            TensorProductScoreModel.expected_state_dict_spec(SimpleNamespace(cfg=cfg, confidence_mode=False)).items()}
    spec.update({k: tuple(v) for k, v in
                 PretrainedScoreEncoder.predictor_spec(SimpleNamespace(hidden=96, ns=ns, latent_dim=1, no_bn=no_bn)).items()})
    got = {k: tuple(v.shape) for k, v in ar.state_dict().items()}
    assert set(got) == set(spec), sorted(set(got) ^ set(spec))
    assert got == spec, {k: (got[k], spec[k]) for k in got if got[k] != spec[k]}
    assert ar.latent_s_predictor[0].in_features == 2 * ns and not ar.apply_gumbel_softmax


REFUSED = [('latent_vocab', dict(latent_vocab=32)), ('latent_dim', dict(latent_dim=2)), ('input_latent_dim', dict(input_latent_dim=3)), ('ns', dict(ns=32)),
           ('latent_dropout', dict(latent_dropout=1.0)), ('latent_hidden_dim', dict(latent_hidden_dim=0))]


@pytest.mark.parametrize('name,change', REFUSED)
def test_refused_arguments_are_named(name, change):
    from disco_diffdock_amd.pretrained_score_encoder import TrainablePretrainedScoreEncoder
    kw = dict(ns=24, latent_dim=1, latent_vocab=1, input_latent_dim=2)
    kw.update(change)
    with pytest.raises(RuntimeError, match=rf'TrainablePretrainedScoreEncoder: {name} '):
        TrainablePretrainedScoreEncoder(_score(), **kw)


def test_refused_score_models():
    from disco_diffdock_amd.pretrained_score_encoder import TrainablePretrainedScoreEncoder
    with pytest.raises(RuntimeError, match='latent_dim >= 1'):
        TrainablePretrainedScoreEncoder(_score(latent_dim=0), ns=24, latent_dim=1, latent_vocab=1, input_latent_dim=1)
    with pytest.raises(RuntimeError, match='TrainableScoreModel'):
        TrainablePretrainedScoreEncoder(torch.nn.Linear(1, 1), ns=24, latent_dim=1, latent_vocab=1, input_latent_dim=1)


def test_get_ar_model_training_builds_the_trainable_class():
    from disco_diffdock_amd.model_utils import get_ar_model
    from disco_diffdock_amd.pretrained_score_encoder import TrainablePretrainedScoreEncoder
    score_args = SimpleNamespace(no_torsion=False, num_conv_layers=3, max_radius=5.0, scale_by_sigma=True, sigma_embed_dim=32, ns=24, nv=6, distance_embed_dim=32,
                                 cross_distance_embed_dim=32, no_batch_norm=False, dropout=0.1, sh_lmax=1, use_second_order_repr=False, cross_max_distance=80,
                                 dynamic_max_cross=True, esm_embeddings_path='x', use_old_atom_encoder=False, embedding_scale=1000, tr_sigma_min=0.1,
                                 tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14,
                                 embedding_type='sinusoidal', latent_dim=2, latent_vocab=1, latent_droprate=0.1)

    class Args(dict):      # (the reference tests `'use_pretrained_score' in args` on its Namespace)
        __getattr__ = dict.__getitem__

    ar_args = Args(use_pretrained_score=True, ns=16, latent_no_batchnorm=False, latent_dropout=0.05, latent_hidden_dim=64, original_model_dir='nowhere', ckpt='none.pt')
    ar = get_ar_model(ar_args, score_args, torch.device('cpu'), training=True)
    assert isinstance(ar, TrainablePretrainedScoreEncoder) and not ar.apply_gumbel_softmax and ar.input_latent_dim == 2 and ar.ns == 16
    assert ar.latent_r_predictor[3].p == 0.05 and ar.latent_r_predictor[8].out_features == 1 and ar.tr_sigma_max == 19.0
    # the warm-up freeze: only the predictors stay trainable
    for p in ar.pretrained_score_model.parameters():
        p.requires_grad = False
    assert {n.split('.')[0] for n, p in ar.named_parameters() if p.requires_grad} == {'latent_s_predictor', 'latent_r_predictor'}
    with pytest.raises(RuntimeError, match='use_pretrained_score'):
        get_ar_model(Args(use_pretrained_score=False), score_args, torch.device('cpu'), training=True)


def test_shim_checks_what_the_host_can_see():
    """shapes, dtypes, D, G and contiguity are refused before anything reaches the library (no device is needed to get that far, except for the device test)"""
    from disco_diffdock_amd.runtime import Context
    check = Context._node_ce_operands
    with pytest.raises(RuntimeError, match='on the GPU'):
        check(torch.zeros(3), torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, 1), torch.zeros(2, 1),
              torch.zeros(1, dtype=torch.int32), False, 'node_cross_entropy')
    from disco_diffdock_amd.tensor_layers import ragged_node_cross_entropy
    with pytest.raises(RuntimeError, match='GPU only'):
        ragged_node_cross_entropy(torch.zeros(3), torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, 1),
                                  torch.zeros(2, 1), torch.zeros(1, dtype=torch.int32))
