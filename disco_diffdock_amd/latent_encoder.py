"""A trainable DisCo latent encoder: the reference's ``TPEncoder`` (models/latent_encoder.py) for the configuration DisCo trains with, with real
``nn.Parameter``s under the reference's keys, assembled from the differentiable device ops as ``train_model.TrainableScoreModel`` is:

    batch -> graph build on the TRUE pose (``data['ligand'].orig_pos_torch``; plain torch, no gradient) -> node embeddings (``AtomEncoder``)
          -> three ``fused_edge_embedding`` calls (``sig=None``: the encoder has no sigma block) -> ``conv_stack`` -> the scalar columns
          -> ``latent_s_predictor`` / ``latent_r_predictor`` (plain torch) -> per-node logits [N_lig, D], [N_rec, D]
          -> ``ragged_gumbel_softmax`` (``apply_gumbel_softmax=True``) or the per-graph logit list (False: the AR model's targets)

The oracle encoder reads the ground-truth pose: it runs in training, to make AR targets, and in front of the sampler (``sampling.oracle_latents``: once per
batch of copies of a complex, through ``logits`` in ``.eval()``).  It has no inference engine of its own behind the C ABI.  Its conv
layers are the ns = 24 / nv = 4 (or nv = 6) family of the tensor-product ops; an nv = 4 layer has no fused inference kernel and evaluates with the
training ops (``tensor_layers.TensorProductConvLayer``).

Seeding.  ``forward(data, seed=None)``: the dropout masks of the device ops and the Gumbel noise are pure functions of ``seed`` and of the graphs' stream
ids (``runtime.stream_id(name)`` of ``data.name``).  The sub-seeds are ``_layer_seed(seed, ENCODER_SEED_BASE + k)``: k = 0 .. L - 1 the conv layers, L .. L + 2
the three edge embeddings, L + 3 the Gumbel draw; a score model that is handed the same seed uses k below ENCODER_SEED_BASE.  The two predictors' ``nn.Dropout``
layers (``latent_dropout``) draw from torch's generators, which ``training.train_epoch`` seeds per step.

Not covered: the AR predictor variant (``input_latent_dim > 0``, ``use_oracle=False``), ``latent_vocab > 1``, virtual nodes / ``TransformerConv``,
``use_second_order_repr``, any other ns / nv / sh_lmax."""
import torch
from torch import nn

from .runtime import stream_id
from .synthetic import LIG_FEATURE_DIMS, REC_RESIDUE_FEATURE_DIMS
from .tensor_layers import GaussianSmearing, TensorProductConvLayer, _draw_seed, _layer_seed, conv_stack, ragged_gumbel_softmax
from .train_model import AtomEncoder, embed_edge_groups

ENCODER_SEED_BASE = 32      # the encoder's sub-seeds start here: a score model takes 0 .. num_conv_layers + 2 (at most 18) of the same seed


def _predictor(n_in, hidden, n_out, batchnorm, dropout):
    """models/latent_encoder.py:148-169: keys 0, (1,) 4, (5,) 8"""
    norm = lambda: nn.BatchNorm1d(hidden) if batchnorm else nn.Identity()
    return nn.Sequential(nn.Linear(n_in, hidden), norm(), nn.ReLU(), nn.Dropout(dropout), nn.Linear(hidden, hidden), norm(), nn.ReLU(), nn.Dropout(dropout),
                         nn.Linear(hidden, n_out))


def _rows_by_graph(module, sizes, *tensors):
    """``module(*tensors)``; with ``sizes`` (rows per graph) the module runs on each graph's rows by themselves, each part in storage of its own, so that
    a row's result is the same whatever else is in the batch"""
    if not sizes or len(sizes) == 1:
        return module(*tensors)
    parts = zip(*(torch.split(t, sizes) for t in tensors))
    return torch.cat([module(*(t.clone() for t in part)) for part in parts], 0)


class TPEncoder(nn.Module):
    """Constructor arguments follow the reference's ``TPEncoder`` (models/latent_encoder.py:17-23).  Supported: sh_lmax=1, ns=24, nv 4 or 6, 1..5 conv
    layers, latent_vocab=1, latent_dim 1..4, use_oracle=True with input_latent_dim=0, no virtual nodes, first-order irreps, 32-wide distance embeddings,
    batch_norm / dropout / lm_embedding_type / latent_no_batchnorm / latent_dropout / latent_hidden_dim / apply_gumbel_softmax as given; anything else
    raises and names the argument."""

    def __init__(self, device, latent_dim, latent_vocab, in_lig_edge_features=4, sh_lmax=2, ns=16, nv=4, num_conv_layers=2, lig_max_radius=5,
                 rec_max_radius=30, cross_max_distance=250, center_max_distance=30, distance_embed_dim=32, cross_distance_embed_dim=32, no_torsion=False,
                 use_second_order_repr=False, batch_norm=True, dropout=0.0, lm_embedding_type=None, latent_no_batchnorm=False, latent_dropout=0.0,
                 latent_hidden_dim=128, use_oracle=True, input_latent_dim=0, apply_gumbel_softmax=True, latent_virtual_nodes=False,
                 latent_nodes_residual=False):
        super().__init__()
        refused = [('sh_lmax', sh_lmax != 1, 'must be 1'), ('ns', ns != 24, 'must be 24'), ('nv', nv not in (4, 6), 'must be 4 or 6'),
                   ('num_conv_layers', not 1 <= num_conv_layers <= 5, 'must be in 1..5'),
                   ('latent_vocab', latent_vocab != 1, 'must be 1: the equivariant one-hot-over-nodes latent only'),
                   ('latent_dim', not 1 <= latent_dim <= 4, 'must be in 1..4'),
                   ('input_latent_dim', input_latent_dim != 0, 'must be 0: the AR predictor variant is not implemented'),
                   ('use_oracle', not use_oracle, 'must be True: the AR predictor variant, which reads the noised pose, is not implemented'),
                   ('latent_virtual_nodes', bool(latent_virtual_nodes), 'is not implemented (virtual nodes / TransformerConv)'),
                   ('latent_nodes_residual', bool(latent_nodes_residual), 'is not implemented (it belongs to latent_virtual_nodes)'),
                   ('use_second_order_repr', bool(use_second_order_repr), 'is not implemented'),
                   ('in_lig_edge_features', in_lig_edge_features != 4, 'must be 4'), ('distance_embed_dim', distance_embed_dim != 32, 'must be 32'),
                   ('cross_distance_embed_dim', cross_distance_embed_dim != 32, 'must be 32'),
                   ('lm_embedding_type', lm_embedding_type not in (None, 'esm'), "must be None or 'esm'"),
                   ('dropout', not 0.0 <= float(dropout) < 1.0, 'must be in [0, 1)'),
                   ('latent_dropout', not 0.0 <= float(latent_dropout) < 1.0, 'must be in [0, 1)'),
                   ('latent_hidden_dim', int(latent_hidden_dim) < 1, 'must be positive')]
        for name, bad, why in refused:
            if bad:
                raise RuntimeError(f'ddk: TPEncoder: {name} {why}')
        self.ns, self.nv, self.num_conv_layers, self.no_torsion = ns, nv, int(num_conv_layers), bool(no_torsion)
        self.lig_max_radius, self.rec_max_radius = float(lig_max_radius), float(rec_max_radius)
        self.cross_max_distance, self.center_max_distance = float(cross_max_distance), float(center_max_distance)
        self.latent_dim, self.latent_vocab, self.use_oracle, self.input_latent_dim = int(latent_dim), 1, True, 0
        self.apply_gumbel_softmax = bool(apply_gumbel_softmax)
        self.latent_temperature = 1.0      # reset by the training and evaluation routines (LatentModelWrapper sets it before every call)

        self.lig_node_embedding = AtomEncoder(ns, (LIG_FEATURE_DIMS, 0), 0)
        self.lig_edge_embedding = nn.Sequential(nn.Linear(in_lig_edge_features + distance_embed_dim, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.rec_node_embedding = AtomEncoder(ns, (REC_RESIDUE_FEATURE_DIMS, 0), 0, lm_embedding_type)
        self.rec_edge_embedding = nn.Sequential(nn.Linear(distance_embed_dim, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.cross_edge_embedding = nn.Sequential(nn.Linear(cross_distance_embed_dim, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.lig_distance_expansion = GaussianSmearing(0.0, lig_max_radius, distance_embed_dim)
        self.rec_distance_expansion = GaussianSmearing(0.0, rec_max_radius, distance_embed_dim)
        self.cross_distance_expansion = GaussianSmearing(0.0, cross_max_distance, cross_distance_embed_dim)

        seq = [f'{ns}x0e', f'{ns}x0e + {nv}x1o', f'{ns}x0e + {nv}x1o + {nv}x1e', f'{ns}x0e + {nv}x1o + {nv}x1e + {ns}x0o']
        self.conv_layers = nn.ModuleList([TensorProductConvLayer(in_irreps=seq[min(i, 3)], sh_irreps='1x0e+1x1o', out_irreps=seq[min(i + 1, 3)],
                                                                 n_edge_features=3 * ns, hidden_features=3 * ns, residual=True, batch_norm=batch_norm,
                                                                 dropout=dropout, faster=True, edge_groups=4) for i in range(self.num_conv_layers)])
        n_scalar = 2 * ns if self.num_conv_layers >= 3 else ns      # the 0o columns exist from the third layer on
        self.latent_s_predictor = _predictor(n_scalar, int(latent_hidden_dim), self.latent_dim, not latent_no_batchnorm, latent_dropout)
        self.latent_r_predictor = _predictor(n_scalar, int(latent_hidden_dim), self.latent_dim, not latent_no_batchnorm, latent_dropout)

    def _seeds(self, seed):
        """(the conv stack's seed, the three edge embeddings' seeds, the Gumbel seed) of a call's ``seed``"""
        L = self.num_conv_layers
        stack = _layer_seed(seed, ENCODER_SEED_BASE - 1)      # conv_stack gives layer l _layer_seed(stack, l) = _layer_seed(seed, ENCODER_SEED_BASE + l)
        return stack, [_layer_seed(stack, L + g) for g in range(3)], _layer_seed(stack, L + 3)

    def gumbel_seed(self, seed):
        """the seed ``forward(data, seed)`` hands to ``ragged_gumbel_softmax``"""
        return self._seeds(seed)[2]

    def logits(self, data, seed=None):
        """models/latent_encoder.py:171-323 without virtual nodes, vocab 1: (logit_l [N_lig, D], logit_r [N_rec, D], lig_batch, rec_batch) of a collated
        batch in the layout ``TrainableScoreModel.forward`` documents, with the true poses in ``data['ligand'].orig_pos_torch``."""
        lig, rec = data['ligand'], data['receptor']
        pos_e = getattr(lig, 'orig_pos_torch', None)
        if pos_e is None:
            raise RuntimeError("ddk: TPEncoder (use_oracle) reads the true pose in data['ligand'].orig_pos_torch; the batch has none "
                               '(training.noise_batch sets it)')
        if not pos_e.is_cuda:
            raise RuntimeError('ddk TPEncoder runs on the GPU only (no CPU fallback)')
        dev, B = pos_e.device, int(data.num_graphs)
        with torch.no_grad():
            lig_pos, rec_pos = pos_e.detach().float().reshape(-1, 3), rec.pos.to(dev).detach().float()
            lig_batch, rec_batch = lig.batch.to(dev).long(), rec.batch.to(dev).long()
            if lig_pos.shape[0] != lig_batch.shape[0]:
                raise RuntimeError(f"ddk: data['ligand'].orig_pos_torch must hold one row per ligand atom ({lig_batch.shape[0]}); got {lig_pos.shape[0]}")
            n_lig = lig_pos.shape[0]
            n_cat = self.rec_node_embedding.num_categorical_features
            rec_x = rec.x.to(dev)
        if seed is None and self.training:
            seed = _draw_seed()
        stack_seed, emb_seeds, _ = self._seeds(seed) if seed is not None else (None, [None] * 3, None)

        # In evaluation the torch Linears (node embeddings, predictors) run graph by graph: a library GEMM picks its algorithm, and with it the
        # summation order of a row, by the number of rows (measured: the receptor embedding's K = 1304 product differs in the last bits between 22 and
        # 85 rows), and a graph's logits must not depend on the batch it is collated in.  Training couples the graphs through BatchNorm anyway.
        # torch does not promise that equal row counts give equal bits either: it is what the library does, measured for these shapes, and the test holds it.
        sizes = None
        if not self.training:
            sizes = torch.stack([torch.bincount(lig_batch, minlength=B)[:B], torch.bincount(rec_batch, minlength=B)[:B]]).tolist()      # (one read-back)
        lig_node_attr = _rows_by_graph(self.lig_node_embedding, sizes and sizes[0], lig.x.to(dev).long(), lig_pos.new_zeros((n_lig, 0)))
        rec_node_attr = _rows_by_graph(self.rec_node_embedding, sizes and sizes[1], rec_x[:, :n_cat].long(), rec_x[:, n_cat:].float())
        edge_index, group_sizes, edge_emb, edge_sh = embed_edge_groups(self, lig_pos, lig_batch, rec_pos, rec_batch, data['ligand', 'ligand'],
                                                                       data['receptor', 'receptor'].edge_index, B, self.cross_max_distance, None,
                                                                       emb_seeds)      # (sig None: the encoder has no sigma block)
        node_attr = torch.cat([lig_node_attr, rec_node_attr], dim=0)
        node_attr = conv_stack(self.conv_layers, node_attr, edge_index, edge_emb, group_sizes, edge_sh, seed=stack_seed)
        ns = self.ns
        scalar = torch.cat([node_attr[:, :ns], node_attr[:, -ns:]], dim=1) if self.num_conv_layers >= 3 else node_attr[:, :ns]
        return (_rows_by_graph(self.latent_s_predictor, sizes and sizes[0], scalar[:n_lig]), _rows_by_graph(self.latent_r_predictor, sizes and sizes[1], scalar[n_lig:]),
                lig_batch, rec_batch)

    def forward(self, data, seed=None):
        """``apply_gumbel_softmax=True``: (latent_l [N_lig, D], latent_r [N_rec, D]), per graph and latent dimension a straight-through one-hot over the
        graph's ligand + receptor nodes at ``self.latent_temperature``; False: the reference's list of per-graph [1, D, n_lig + n_rec] logit tensors.
        ``seed``: of the dropout masks and the Gumbel noise (None: one draw from torch's default CPU generator)."""
        if seed is None and (self.training or self.apply_gumbel_softmax):
            seed = _draw_seed()
        logit_l, logit_r, lig_batch, rec_batch = self.logits(data, seed)
        B = int(data.num_graphs)
        if not self.apply_gumbel_softmax:
            n_l, n_r = (torch.bincount(b, minlength=B)[:B].tolist() for b in (lig_batch, rec_batch))      # (the AR targets' path: two read-backs)
            return [torch.cat([l, r], dim=0).T.unsqueeze(0) for l, r in zip(torch.split(logit_l, n_l), torch.split(logit_r, n_r))]
        names = getattr(data, 'name', None)
        names = [names] if isinstance(names, str) else names
        if names is None or len(names) != B:
            raise RuntimeError(f'ddk: TPEncoder takes the complexes\' names in data.name ({B} of them): the Gumbel noise of a graph is drawn from '
                               'runtime.stream_id(name)')
        return ragged_gumbel_softmax(logit_l, logit_r, lig_batch, rec_batch, self.latent_temperature, self.gumbel_seed(seed), [stream_id(n) for n in names])
