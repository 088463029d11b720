"""Host mirror of the reference's AR latent model at inference:
``PretrainedScoreEncoder`` (models/pretrained_score_encoder.py:9-89) and ``GenericEncoder.encode_ar``
(models/model_classes.py:9-49), latent_vocab == 1.  Everything runs in libddk.so: ``score_model.embed()`` at t = 1 with
unconditional = 1 and the partially decoded input latents is the ordinary score-model forward of the AR checkpoint's own
score-model copy (its own ddk context), the two predictor MLPs with BatchNorm1d(eval) are ``ddk_ar_logits`` and the per-graph
pick + one-hot write is ``ddk_ar_decode`` (csrc/k_ar.hip).  ``encode_ar`` never reads the device back."""
import collections

import torch
from torch import nn

from .score_model import complex_for_batch


class GenericEncoder(nn.Module):
    def encode_ar(self, data, sampling_temperature=1.0, choice_fn=None, uniforms=None, rng=None):
        """assumes graphs of the same complex as input (model_classes.py:10).  Returns the one-hot latents
        ``(latent_l [B*n_lig, D], latent_r [B*n_rec, D])`` on the device; ``self.last_choices`` [B, D] (int32, device) holds the
        picked node of every graph (ligand atoms first).
        Extras for the parity tests: ``uniforms`` [D, B] replaces the device draws of the inverse-CDF pick;
        ``choice_fn(idx, logits)`` replaces the pick altogether (host round trip).
        ``rng`` = (seed, stream id, sample0): the uniforms come from the counter-based generator instead of torch's (``ddk_rng_uniform``: graph b is the
        global sample sample0 + b, so its picks do not depend on the batch around it)."""
        if self.latent_vocab != 1:
            raise RuntimeError('ddk: AR decoding is implemented for latent_vocab == 1')
        sm = self.pretrained_score_model
        pos = data['ligand'].pos
        if not pos.is_cuda:
            raise RuntimeError('ddk AR model runs on the GPU only (no CPU fallback)')
        dev = pos.device
        cx, B = complex_for_batch(data, dev, ctx=sm.ctx)
        D = self.input_latent_dim
        latent_l = torch.zeros(B * cx.n_lig, D, device=dev)
        latent_r = torch.zeros(B * cx.n_rec, D, device=dev)
        choices = torch.full((B, D), -1, dtype=torch.int32, device=dev)
        T = float(sampling_temperature)
        p3 = pos.reshape(B, -1, 3)
        cx.keep_receptor_features(True)        # embed(): the predictors read the receptor rows of the last conv layer too
        try:
            for idx in range(D):
                logits = self._logits(cx, p3, latent_l, latent_r)
                if choice_fn is not None:
                    c = choice_fn(idx, logits * T)[:, 0].to(dev)
                    rows = torch.arange(B, device=dev)
                    in_lig = c < cx.n_lig
                    latent_l[(rows * cx.n_lig + c)[in_lig], idx] = 1
                    latent_r[(rows * cx.n_rec + c - cx.n_lig)[~in_lig], idx] = 1
                    choices[:, idx] = c.int()
                    continue
                u = None
                if T < 100:
                    if uniforms is not None:
                        u = uniforms[idx].to(dev).float().contiguous()
                    else:
                        u = torch.rand(B, device=dev) if rng is None else sm.ctx.rng_uniform(rng[0], rng[1], rng[2], B, idx)
                cx.ar_decode(logits, T, u, idx, latent_l, latent_r, choices)
        finally:
            cx.keep_receptor_features(False)
        self.last_choices = choices
        return latent_l, latent_r

    def _logits(self, cx, pos, latent_l, latent_r):
        """one embed() pass + the predictors: [B, n_lig + n_rec]"""
        cx.set_latents(latent_l, latent_r, 1.0)            # unconditional = 1 (pretrained_score_encoder.py:62-64)
        cx.score_forward(pos, 1.0, 1.0, 1.0)               # set_time(data, 1, 1, 1, ...) (:59-61)
        return cx.ar_logits(pos.shape[0])


class PretrainedScoreEncoder(GenericEncoder):
    def __init__(self, pretrained_score_model, ns, latent_dim, latent_vocab, latent_no_batchnorm=False, latent_dropout=0.0,
                 latent_hidden_dim=128, input_latent_dim=0, apply_gumbel_softmax=True):
        super().__init__()
        assert input_latent_dim > 0
        if latent_dim != 1:
            raise RuntimeError('ddk: the AR predictors emit one logit per node (latent_dim = 1, utils/model_utils.py:133-139)')
        if pretrained_score_model.cfg['num_conv_layers'] < 3:
            raise RuntimeError('ddk: AR predictors need the full irreps (num_conv_layers >= 3: inputs [x[:, :ns] | x[:, -ns:]])')
        self.ns, self.latent_dim, self.latent_vocab = ns, latent_dim, latent_vocab
        self.latent_temperature = 1.0
        self.input_latent_dim = input_latent_dim
        self.apply_gumbel_softmax = apply_gumbel_softmax
        self.pretrained_score_model = pretrained_score_model      # ddk-backed TensorProductScoreModel
        self.hidden, self.no_bn = latent_hidden_dim, bool(latent_no_batchnorm)
        self.last_choices = None

    def predictor_spec(self):
        """name -> shape of the predictor part of the AR checkpoint (models/pretrained_score_encoder.py:24-45)."""
        H, n_in, spec = self.hidden, 2 * self.ns, {}
        for name in ('latent_s_predictor', 'latent_r_predictor'):
            for i, shape in ((0, (H, n_in)), (4, (H, H)), (8, (self.latent_dim, H))):
                spec[f'{name}.{i}.weight'], spec[f'{name}.{i}.bias'] = shape, (shape[0],)
            if not self.no_bn:
                for i in (1, 5):
                    for k in ('weight', 'bias', 'running_mean', 'running_var'):
                        spec[f'{name}.{i}.{k}'] = (H,)
                    spec[f'{name}.{i}.num_batches_tracked'] = ()
        return spec

    def load_state_dict(self, state_dict, strict=True):
        pre = 'pretrained_score_model.'
        own = {k: v for k, v in state_dict.items() if not k.startswith(pre)}
        spec = self.predictor_spec()
        missing = [k for k in spec if k not in own and not k.endswith('num_batches_tracked')]
        unexpected = [k for k in own if k not in spec]
        bad = [k for k in spec if k in own and tuple(own[k].shape) != tuple(spec[k])]
        if missing or bad or (strict and unexpected):
            raise RuntimeError(f'AR state_dict mismatch: missing {missing}, unexpected {unexpected}, mis-shaped {bad}')
        # the predictors live in the SAME ddk context as the AR checkpoint's score-model copy (ddk_finalize_weights folds the BatchNorms)
        self.pretrained_score_model.load_state_dict({k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}, strict=strict,
                                                    extra={k: v for k, v in own.items() if k in spec})
        return torch.nn.modules.module._IncompatibleKeys([], unexpected)

    def logits(self, data):
        """[B, latent_dim, n_lig + n_rec] logits of PretrainedScoreEncoder.forward with apply_gumbel_softmax=False, for the input
        latents ``data[...].input_latent`` (the batch is left untouched)."""
        if self.training:
            raise RuntimeError('ddk: inference (eval mode) only')
        pos = data['ligand'].pos
        if not pos.is_cuda:
            raise RuntimeError('ddk AR model runs on the GPU only (no CPU fallback)')
        cx, B = complex_for_batch(data, pos.device, ctx=self.pretrained_score_model.ctx)
        cx.keep_receptor_features(True)
        try:
            lg = self._logits(cx, pos.reshape(B, -1, 3), data['ligand'].input_latent.to(pos.device), data['receptor'].input_latent.to(pos.device))
        finally:
            cx.keep_receptor_features(False)
        return lg[:, None, :]

    def forward(self, data):
        raise RuntimeError('ddk: use encode_ar() / logits(); the trainable class is TrainablePretrainedScoreEncoder (model_utils.get_ar_model(training=True))')


# what ``TrainablePretrainedScoreEncoder.forward`` returns with apply_gumbel_softmax=False: the per-node logits [N_lig, 1], [N_rec, 1] and the int64 [G + 1]
# prefixes of the graphs' rows, all on the device (what ``tensor_layers.ragged_node_cross_entropy`` takes)
ARLogits = collections.namedtuple('ARLogits', ('logit_l', 'logit_r', 'lig_ptr', 'rec_ptr'))

AR_GUMBEL_SEED_INDEX = 24      # the sub-seed of the AR model's Gumbel draw: the score model takes 0 .. num_conv_layers + 2 (at most 18), an oracle encoder 32 and up


class TrainablePretrainedScoreEncoder(nn.Module):
    """The reference's ``PretrainedScoreEncoder`` (models/pretrained_score_encoder.py) for training: a ``train_model.TrainableScoreModel`` with
    ``latent_dim >= 1`` and at least three conv layers under ``pretrained_score_model``, and the two predictors as real ``nn.Sequential`` modules under the
    reference's keys.  ``state_dict()`` has the keys of the inference class (the score model's under ``pretrained_score_model.`` plus
    ``PretrainedScoreEncoder.predictor_spec()``), so what is trained here loads into ``model_utils.get_ar_model(training=False)`` with ``strict=True`` and
    an AR checkpoint loads here.  ``ns``: the AR settings' (the predictors read ``[x[:, :ns] | x[:, -ns:]]`` of the score model's node rows; it may be
    smaller than the score model's 24).  Supported: latent_vocab=1, latent_dim=1 (one logit per node); anything else raises and names the argument."""

    def __init__(self, pretrained_score_model, ns, latent_dim, latent_vocab, latent_no_batchnorm=False, latent_dropout=0.0, latent_hidden_dim=128,
                 input_latent_dim=0, apply_gumbel_softmax=True):
        super().__init__()
        from .latent_encoder import _predictor
        from .train_model import TrainableScoreModel
        sm = pretrained_score_model
        if not isinstance(sm, TrainableScoreModel) or sm.latent_dim < 1:
            raise RuntimeError('ddk: TrainablePretrainedScoreEncoder: pretrained_score_model must be a TrainableScoreModel with latent_dim >= 1')
        refused = [('latent_vocab', latent_vocab != 1, 'must be 1: the equivariant one-hot-over-nodes latent only'),
                   ('latent_dim', latent_dim != 1, 'must be 1: the AR predictors emit one logit per node (utils/model_utils.py:133-139)'),
                   ('num_conv_layers', len(sm.conv_layers) < 3, 'of the score model must be >= 3: the predictors read [x[:, :ns] | x[:, -ns:]] of the full rows'),
                   ('input_latent_dim', int(input_latent_dim) != sm.latent_dim, f"must be the score model's latent_dim ({sm.latent_dim})"),
                   ('ns', not 1 <= int(ns) <= sm.ns, f"must be in 1..{sm.ns}, the score model's ns"),
                   ('latent_dropout', not 0.0 <= float(latent_dropout) < 1.0, 'must be in [0, 1)'),
                   ('latent_hidden_dim', int(latent_hidden_dim) < 1, 'must be positive')]
        for name, bad, why in refused:
            if bad:
                raise RuntimeError(f'ddk: TrainablePretrainedScoreEncoder: {name} {why}')
        self.ns, self.latent_dim, self.latent_vocab = int(ns), 1, 1
        self.latent_temperature = 1.0
        self.input_latent_dim = int(input_latent_dim)
        self.apply_gumbel_softmax = bool(apply_gumbel_softmax)
        self.pretrained_score_model = sm
        self.latent_s_predictor = _predictor(2 * self.ns, int(latent_hidden_dim), 1, not latent_no_batchnorm, latent_dropout)
        self.latent_r_predictor = _predictor(2 * self.ns, int(latent_hidden_dim), 1, not latent_no_batchnorm, latent_dropout)

    # what ``ar_training.ar_batch`` and ``training``'s helpers read off the model they are handed
    @property
    def ctx(self):
        return self.pretrained_score_model.ctx

    @property
    def no_torsion(self):
        return self.pretrained_score_model.no_torsion

    @property
    def tr_sigma_max(self):
        return self.pretrained_score_model.tr_sigma_max

    def logits(self, data, seed=None):
        """models/pretrained_score_encoder.py:56-72: ``latent_h = input_latent``, ``unconditional = 1`` and ``complex_t = 1`` for every graph, the score
        model's ``embed`` and the two predictors: :data:`ARLogits`.  The pointer tables are ``data.lig_ptr`` / ``data.rec_ptr`` where the batch has them
        (``ar_training.ar_batch`` sets them); otherwise they are made from the batch vectors, with one read-back that checks those."""
        from .tensor_layers import _graph_ptrs
        sm = self.pretrained_score_model
        lig, rec = data['ligand'], data['receptor']
        if not lig.pos.is_cuda:
            raise RuntimeError('ddk TrainablePretrainedScoreEncoder runs on the GPU only (no CPU fallback)')
        dev, B = lig.pos.device, int(data.num_graphs)
        for side in (lig, rec):
            if getattr(side, 'input_latent', None) is None:
                raise RuntimeError("ddk: TrainablePretrainedScoreEncoder reads data['ligand' | 'receptor'].input_latent; the batch has none "
                                   '(ar_training.ar_batch sets it)')
            side.latent_h = side.input_latent.to(dev).float()
            side.unconditional = torch.ones((side.latent_h.shape[0], 1), device=dev)
        data.complex_t = {k: torch.ones(B, device=dev) for k in ('tr', 'rot', 'tor')}
        lig_attr, rec_attr = sm.embed(data, seed)
        ns = self.ns
        logit_l = self.latent_s_predictor(torch.cat([lig_attr[:, :ns], lig_attr[:, -ns:]], dim=1))
        logit_r = self.latent_r_predictor(torch.cat([rec_attr[:, :ns], rec_attr[:, -ns:]], dim=1))
        lig_ptr, rec_ptr = getattr(data, 'lig_ptr', None), getattr(data, 'rec_ptr', None)
        if lig_ptr is None or rec_ptr is None:
            (lig_ptr, rec_ptr), probes = _graph_ptrs((lig.batch.to(dev), rec.batch.to(dev)), B)
            for what, (descent, first, last) in zip(("data['ligand'].batch", "data['receptor'].batch"), probes):
                if descent > 0 or first < 0 or last >= B:
                    raise RuntimeError(f'ddk: TrainablePretrainedScoreEncoder takes {what} sorted by graph with entries in [0, {B})')
        return ARLogits(logit_l, logit_r, lig_ptr, rec_ptr)

    @staticmethod
    def logit_list(pred):
        """:data:`ARLogits` -> the reference's list of per-graph [1, 1, n_lig_g + n_rec_g] tensors (one read-back of the two pointer tables)"""
        n_l, n_r = ((p[1:] - p[:-1]).tolist() for p in (pred.lig_ptr, pred.rec_ptr))
        return [torch.cat([l, r], dim=0).T.unsqueeze(0) for l, r in zip(torch.split(pred.logit_l, n_l), torch.split(pred.logit_r, n_r))]

    def forward(self, data, seed=None):
        """``apply_gumbel_softmax=False`` (training, as ``get_ar_model`` builds it): :data:`ARLogits`; True: (latent_l [N_lig, 1], latent_r [N_rec, 1]), per
        graph a straight-through one-hot over its nodes at ``self.latent_temperature`` (``ragged_gumbel_softmax``; the graphs' names in ``data.name``).
        ``seed``: of the device ops' dropout masks and the Gumbel noise (None: one draw from torch's default CPU generator where one is needed)."""
        from .runtime import stream_id
        from .tensor_layers import _draw_seed, _layer_seed, ragged_gumbel_softmax
        if seed is None and (self.training or self.apply_gumbel_softmax):
            seed = _draw_seed()
        pred = self.logits(data, seed)
        if not self.apply_gumbel_softmax:
            return pred
        B = int(data.num_graphs)
        names = getattr(data, 'name', None)
        names = [names] if isinstance(names, str) else names
        if names is None or len(names) != B:
            raise RuntimeError(f"ddk: TrainablePretrainedScoreEncoder takes the complexes' names in data.name ({B} of them): the Gumbel noise of a graph "
                               'is drawn from runtime.stream_id(name)')
        dev = pred.logit_l.device
        return ragged_gumbel_softmax(pred.logit_l, pred.logit_r, data['ligand'].batch.to(dev), data['receptor'].batch.to(dev), self.latent_temperature,
                                     _layer_seed(seed, AR_GUMBEL_SEED_INDEX), [stream_id(n) for n in names])
