"""A trainable score model: the reference's ``TensorProductScoreModel`` (models/score_model.py) for the coarse-grained sh_lmax=1 configuration with real
``nn.Parameter``s under the reference's keys, assembled from the differentiable device ops:

    batch -> graph build (plain torch, no gradient) -> node embeddings (``gather_rows`` + Linear) -> three ``fused_edge_embedding`` calls
          -> ``conv_stack`` -> ``heads.ScoreHeads`` -> (tr_pred [B, 3], rot_pred [B, 3], tor_pred [sum R])

``state_dict()`` has the keys of ``score_model.TensorProductScoreModel(...).expected_state_dict_spec()`` for the same configuration, so a reference
checkpoint loads with ``strict=True`` and what was trained here loads into the inference class.  ``.train()`` / ``.eval()`` switch BatchNorm between batch
statistics and running buffers and switch dropout, as in the layers; in training every parameter gets the same gradient bits on every run for one seed.
The inference class stays the fast path for sampling: this module is for fine-tuning.

The latent-conditioned DisCo score model (``latent_dim`` in 1..4, ``latent_vocab=1``, ``latent_droprate >= 0``) reads ``data['ligand' |
'receptor'].latent_h`` (and ``.unconditional`` with a drop rate): the latent is appended to every node row and, as [source | destination], to every ligand
and receptor edge row (zeros on cross edges), inside ``fused_edge_embedding``; its gradient reaches whatever made it (``LatentModelWrapper`` puts an encoder
and ``ragged_gumbel_softmax`` in front), again without atomics.

The oracle latent encoder is ``latent_encoder.TPEncoder``.  Not covered: the AR predictor, ``latent_vocab > 1``, ``latent_cross_attention``, ``confidence_mode``, the all-atom
model, any other ns / nv / sh_lmax."""
import inspect

import torch
from torch import nn

from .diffusion_utils import get_timestep_embedding
from .heads import ScoreHeads
from .runtime import DEFAULTS
from .synthetic import LIG_FEATURE_DIMS, REC_RESIDUE_FEATURE_DIMS
from .tensor_layers import (GaussianSmearing, TensorProductConvLayer, _draw_seed, _layer_seed, _shape_context, conv_stack, fused_edge_embedding,
                            gather_rows)

LIG_RADIUS_CAP = 32        # radius_graph's max_num_neighbors default (the self loop rides on top of it)
CROSS_CAP = 10000          # max_num_neighbors of the cross graph (models/score_model.py:381, 384)


def radius(x, y, r, batch_x, batch_y, B, max_num_neighbors=32):
    """torch_cluster.radius as oracle/cluster_lite.py states it: for every query y_i the x_j of the same graph with |x_j - y_i|^2 < r^2 (strict), in
    ascending j, the first ``max_num_neighbors`` of them; returns [y index; x index], by y index, then x index.  One window of the query's own graph per
    query ([Ny, largest graph]), never an Ny x Nx matrix over the batch.  CPU or device tensors."""
    Nx, Ny = x.shape[0], y.shape[0]
    if Nx == 0 or Ny == 0:
        return torch.zeros((2, 0), dtype=torch.long, device=x.device)
    first, count = ScoreHeads._graph_ranges(batch_x, B)      # (first node, node count) per graph; refuses nodes that are not grouped by graph
    window = torch.arange(int(count.max()), device=x.device)
    valid = window[None, :] < count[batch_y][:, None]
    cand = (first[batch_y][:, None] + window[None, :]).clamp(max=Nx - 1)      # [Ny, largest graph]: the nodes of the query's graph, ascending
    d2 = ((y[:, None, :] - x[cand]) ** 2).sum(-1)
    inside = valid & (d2 < float(r) * float(r))
    keep = inside & (torch.cumsum(inside, 1) <= max_num_neighbors)
    yy, col = keep.nonzero(as_tuple=True)      # row-major: by query, then by node index
    return torch.stack([yy, cand[yy, col]])


def radius_graph(x, r, batch, B, max_num_neighbors=32):
    """torch_cluster.radius_graph (flow='source_to_target', no self loops) as oracle/cluster_lite.py states it: [neighbour; centre], by centre, then
    neighbour; the cap counts the centre itself, so ``max_num_neighbors + 1`` go into ``radius``"""
    ei = radius(x, x, r, batch, batch, B, max_num_neighbors + 1)
    row, col = ei[1], ei[0]
    mask = row != col
    return torch.stack([row[mask], col[mask]])


def build_conv_edges(lig_pos, lig_batch, rec_pos, rec_batch, bond_index, rec_edge_index, B, lig_max_radius, cross_cutoff):
    """The three edge lists of the reference's embed (models/score_model.py:310-408) for a collated batch, without gradient:
    ``lig_edge_index`` = [the bonds | radius_graph(lig_pos, lig_max_radius)], ``cross_edge_index`` = radius(rec_pos, lig_pos, cutoff) as [ligand atom;
    residue] (residue indices NOT yet offset), ``rec_edge_index`` as given.  ``cross_cutoff``: a float, or a [B] tensor of per-graph cutoffs (the
    reference's dynamic_max_cross: both coordinate sets are divided by their graph's cutoff and the radius is 1).  Returns (lig, cross, rec) edge
    indices [2, .] (int64) and the number of bond edges in front of the ligand list."""
    with torch.no_grad():
        lig_batch, rec_batch = lig_batch.long(), rec_batch.long()
        radius_edges = radius_graph(lig_pos, lig_max_radius, lig_batch, B, LIG_RADIUS_CAP)
        lig_ei = torch.cat([bond_index.long(), radius_edges], 1)
        if torch.is_tensor(cross_cutoff):
            cut = cross_cutoff.reshape(-1, 1).to(lig_pos.dtype)
            cross_ei = radius(rec_pos / cut[rec_batch], lig_pos / cut[lig_batch], 1, rec_batch, lig_batch, B, CROSS_CAP)
        else:
            cross_ei = radius(rec_pos, lig_pos, cross_cutoff, rec_batch, lig_batch, B, CROSS_CAP)
        return lig_ei, cross_ei, rec_edge_index.long(), bond_index.shape[1]


def combine_edges(lig_ei, cross_ei, rec_ei, n_lig):
    """the reference's cat order (models/score_model.py:219-225): ligand, cross, receptor, flipped cross over the node table [ligand | receptor];
    returns (edge_index [2, E], the four group sizes)"""
    lr = torch.stack([cross_ei[0], cross_ei[1] + n_lig])
    edge_index = torch.cat([lig_ei, lr, rec_ei + n_lig, torch.flip(lr, dims=[0])], dim=1)
    return edge_index, (lig_ei.shape[1], lr.shape[1], rec_ei.shape[1], lr.shape[1])


def embed_edge_groups(model, lig_pos, lig_batch, rec_pos, rec_batch, bonds, rec_edge_index, B, cross_cutoff, sig, seeds, latent=None):
    """What the score model and the latent encoder do alike between their node embeddings and ``conv_stack``: the three edge lists
    (``build_conv_edges`` at ``model.lig_max_radius`` and ``cross_cutoff``), the bond features padded with zero rows for the radius edges,
    ``combine_edges``, and one ``fused_edge_embedding`` per group through ``model``'s ``{lig,cross,rec}_edge_embedding`` / ``_distance_expansion``.
    ``bonds``: the batch's ``data['ligand', 'ligand']``; ``sig`` [B, 32] or None (a row without the sigma block); ``seeds``: of the three groups;
    ``latent``: per group the latent keywords of ``fused_edge_embedding`` (None: the plain op in all three).  Returns (edge_index [2, E], the four group sizes, edge_emb [E, 24],
    edge_sh [E, 4]) in the order of ``combine_edges``."""
    dev, latent = lig_pos.device, latent or ({}, {}, {})
    with torch.no_grad():
        lig_ei, cross_ei, rec_ei, n_bond = build_conv_edges(lig_pos, lig_batch, rec_pos, rec_batch, bonds.edge_index.to(dev), rec_edge_index.to(dev), B,
                                                            model.lig_max_radius, cross_cutoff)
        feat = torch.cat([bonds.edge_attr.to(dev).float(), torch.zeros((lig_ei.shape[1] - n_bond, 4), device=dev)], 0)
        edge_index, group_sizes = combine_edges(lig_ei, cross_ei, rec_ei, lig_pos.shape[0])
        lig_idx, rec_idx = (None, None) if sig is None else (lig_batch.to(torch.int32), rec_batch.to(torch.int32))
    lig_emb, lig_sh = fused_edge_embedding(model.lig_edge_embedding, model.lig_distance_expansion, lig_pos, lig_pos, lig_ei, sig, lig_idx, feat=feat,
                                           seed=seeds[0], **latent[0])
    lr_emb, lr_sh = fused_edge_embedding(model.cross_edge_embedding, model.cross_distance_expansion, lig_pos, rec_pos, cross_ei, sig, lig_idx, seed=seeds[1],
                                         **latent[1])
    rec_emb, rec_sh = fused_edge_embedding(model.rec_edge_embedding, model.rec_distance_expansion, rec_pos, rec_pos, rec_ei, sig, rec_idx, seed=seeds[2],
                                           **latent[2])
    edge_emb = torch.cat([lig_emb, lr_emb, rec_emb, lr_emb], dim=0)      # the cross embedding is computed once and serves both directions
    edge_sh = torch.cat([lig_sh, lr_sh, rec_sh, lr_sh], dim=0)
    return edge_index, group_sizes, edge_emb, edge_sh


class AtomEncoder(nn.Module):
    """models/layers.py:119-149 (the new AtomEncoder): one embedding table per categorical feature, summed, then a Linear over [sum | scalar features |
    sigma embedding] where there are any such columns (the latent encoder's ligand side, and its receptor side without ESM, have none: the sum is the output).  The tables are read through ``gather_rows``: their gradient is a fixed-order segmented sum, not index_add_'s atomics."""

    def __init__(self, emb_dim, feature_dims, sigma_embed_dim, lm_embedding_type=None, latent_dim=0):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList()
        self.num_categorical_features = len(feature_dims[0])
        lm = 1280 if lm_embedding_type == 'esm' else 0
        self.additional_features_dim = feature_dims[1] + sigma_embed_dim + lm + latent_dim      # (the latent rides behind the sigma embedding: plain torch, autograd)
        for dim in feature_dims[0]:
            emb = nn.Embedding(dim, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)
        if self.additional_features_dim > 0:      # (models/layers.py:137: without additional features the sum of the tables is the output, and there is no such key)
            self.additional_features_embedder = nn.Linear(self.additional_features_dim + emb_dim, emb_dim)

    def forward(self, x_cat, x_scalar):
        """``x_cat`` [N, categorical features] (integers), ``x_scalar`` [N, additional features] (floats)"""
        if x_cat.shape[1] != self.num_categorical_features or x_scalar.shape[1] != self.additional_features_dim:
            raise RuntimeError(f'ddk: AtomEncoder takes {self.num_categorical_features} categorical and {self.additional_features_dim} scalar columns; '
                               f'got {x_cat.shape[1]} and {x_scalar.shape[1]}')
        emb = 0
        for i, table in enumerate(self.atom_embedding_list):
            emb = emb + gather_rows(table.weight, x_cat[:, i])
        if self.additional_features_dim == 0:
            return emb
        return self.additional_features_embedder(torch.cat([emb, x_scalar], dim=1))


class TrainableScoreModel(nn.Module):
    """Constructor keywords follow ``score_model.TensorProductScoreModel`` (models/score_model.py:15-24 plus ``embedding_scale`` and ``sigma_limits``).
    Supported: sh_lmax=1, ns=24, nv=6, latent_dim 0..4 with latent_vocab=1 and latent_droprate in [0, 1), the new AtomEncoder, 32-wide sigma and distance embeddings, batch_norm / no_torsion /
    dynamic_max_cross on or off, lm_embedding_type None or 'esm', 3..16 conv layers; anything else raises and names the option."""

    def __init__(self, t_to_sigma=None, device=None, timestep_emb_func=None, in_lig_edge_features=4, sigma_embed_dim=32, sh_lmax=2, ns=16, nv=4,
                 num_conv_layers=2, lig_max_radius=5, rec_max_radius=30, cross_max_distance=250, center_max_distance=30, distance_embed_dim=32,
                 cross_distance_embed_dim=32, no_torsion=False, scale_by_sigma=True, use_second_order_repr=False, batch_norm=True,
                 dynamic_max_cross=False, dropout=0.0, lm_embedding_type=None, confidence_mode=False, use_old_atom_encoder=False, latent_dim=0,
                 latent_vocab=32, latent_cross_attention=False, latent_droprate=0.0, embedding_scale=1000.0, sigma_limits=None, conv_kernel=None,
                 confidence_dropout=0, confidence_no_batchnorm=False, num_confidence_outputs=1, new_cross_attention=False, **unused):
        super().__init__()
        refused = [('sh_lmax', sh_lmax != 1, 'must be 1'), ('ns', ns != 24, 'must be 24'), ('nv', nv != 6, 'must be 6'),
                   ('latent_dim', not 0 <= latent_dim <= 4, 'must be in 0..4'),
                   ('latent_vocab', latent_dim > 0 and latent_vocab != 1, 'must be 1 whenever latent_dim > 0: the equivariant one-hot-over-nodes latent only'),
                   ('latent_droprate', not 0.0 <= float(latent_droprate) < 1.0 or (latent_droprate > 0 and latent_dim == 0),
                    'must be in [0, 1), and > 0 needs latent_dim > 0'), ('latent_cross_attention', bool(latent_cross_attention), 'is not implemented'),
                   ('new_cross_attention', bool(new_cross_attention), 'is not implemented'),
                   ('use_old_atom_encoder', bool(use_old_atom_encoder), 'is not implemented: the new AtomEncoder only'),
                   ('use_second_order_repr', bool(use_second_order_repr), 'is not implemented'),
                   ('confidence_mode', bool(confidence_mode), 'is not implemented: the score heads only'),
                   ('in_lig_edge_features', in_lig_edge_features != 4, 'must be 4'), ('sigma_embed_dim', sigma_embed_dim != 32, 'must be 32'),
                   ('distance_embed_dim', distance_embed_dim != 32, 'must be 32'), ('cross_distance_embed_dim', cross_distance_embed_dim != 32, 'must be 32'),
                   ('lm_embedding_type', lm_embedding_type not in (None, 'esm'), "must be None or 'esm'"),
                   ('num_conv_layers', not 3 <= num_conv_layers <= 16, 'must be in 3..16: the heads read the full 0e + 1o + 1e + 0o rows'),
                   ('dropout', not 0.0 <= float(dropout) < 1.0, 'must be in [0, 1)'),
                   ('conv_kernel', conv_kernel is not None, 'selects an inference kernel: it is an option of score_model.TensorProductScoreModel')]
        for name, bad, why in refused:
            if bad:
                raise RuntimeError(f'ddk: TrainableScoreModel: {name} {why}')
        if unused:
            raise RuntimeError(f'ddk: TrainableScoreModel: unknown option(s) {sorted(unused)}')
        keys = ('tr_sigma_min', 'tr_sigma_max', 'rot_sigma_min', 'rot_sigma_max', 'tor_sigma_min', 'tor_sigma_max')
        lim = {k: float((sigma_limits or DEFAULTS)[k]) for k in keys}
        self.ns, self.no_torsion, self.dynamic_max_cross = ns, bool(no_torsion), bool(dynamic_max_cross)
        self.lig_max_radius, self.cross_max_distance = float(lig_max_radius), float(cross_max_distance)
        self.tr_sigma_min, self.tr_sigma_max = lim['tr_sigma_min'], lim['tr_sigma_max']
        self.timestep_emb_func = get_timestep_embedding('sinusoidal', sigma_embed_dim, embedding_scale)
        self.latent_dim, self.latent_droprate = int(latent_dim), float(latent_droprate)
        lat_e = 2 * self.latent_dim      # an edge row carries the latent of its source and of its destination (zeros on cross edges)

        self.lig_node_embedding = AtomEncoder(ns, (LIG_FEATURE_DIMS, 0), sigma_embed_dim, latent_dim=self.latent_dim)
        self.lig_edge_embedding = nn.Sequential(nn.Linear(in_lig_edge_features + sigma_embed_dim + distance_embed_dim + lat_e, ns), nn.ReLU(), nn.Dropout(dropout),
                                                nn.Linear(ns, ns))
        self.rec_node_embedding = AtomEncoder(ns, (REC_RESIDUE_FEATURE_DIMS, 0), sigma_embed_dim, lm_embedding_type, latent_dim=self.latent_dim)
        self.rec_edge_embedding = nn.Sequential(nn.Linear(sigma_embed_dim + distance_embed_dim + lat_e, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.cross_edge_embedding = nn.Sequential(nn.Linear(sigma_embed_dim + cross_distance_embed_dim + lat_e, ns), nn.ReLU(), nn.Dropout(dropout),
                                                  nn.Linear(ns, ns))
        if self.latent_droprate > 0:      # models/score_model.py:97-101: zeros at init
            for k in ('lig_node', 'rec_node', 'lig_edge', 'rec_edge', 'cross_edge'):
                setattr(self, f'{k}_unconditional_embedding', nn.Parameter(torch.zeros(1, ns)))
        self.rec_distance_expansion = GaussianSmearing(0.0, rec_max_radius, distance_embed_dim)
        self.cross_distance_expansion = GaussianSmearing(0.0, cross_max_distance, cross_distance_embed_dim)

        seq = [f'{ns}x0e', f'{ns}x0e + {nv}x1o', f'{ns}x0e + {nv}x1o + {nv}x1e', f'{ns}x0e + {nv}x1o + {nv}x1e + {ns}x0o']
        self.conv_layers = nn.ModuleList([TensorProductConvLayer(in_irreps=seq[min(i, 3)], sh_irreps='1x0e+1x1o', out_irreps=seq[min(i + 1, 3)],
                                                                 n_edge_features=3 * ns, hidden_features=3 * ns, residual=True, batch_norm=batch_norm,
                                                                 dropout=dropout, faster=True, edge_groups=4) for i in range(num_conv_layers)])

        # the heads' modules sit at top level, under the reference's keys; the ScoreHeads object that runs them is not a child (no second set of keys)
        heads = ScoreHeads(ns=ns, nv=nv, sigma_embed_dim=sigma_embed_dim, distance_embed_dim=distance_embed_dim, lig_max_radius=lig_max_radius,
                           center_max_distance=center_max_distance, dropout=dropout, batch_norm=batch_norm, no_torsion=no_torsion,
                           scale_by_sigma=scale_by_sigma, embedding_scale=embedding_scale, sigma_limits=lim)
        for name, module in heads.named_children():
            setattr(self, name, module)
        if self.no_torsion:      # (the torsion head owns the ligand's expansion otherwise: one module, one key)
            self.lig_distance_expansion = GaussianSmearing(0.0, lig_max_radius, distance_embed_dim)
        object.__setattr__(self, '_heads', heads)

    @property
    def ctx(self):
        """the device context the ops run in (what ``training.loss_function`` takes as its ``model``)"""
        dev = next(self.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('ddk TrainableScoreModel runs on the GPU only (no CPU fallback)')
        return _shape_context(dev.index or 0)

    def train(self, mode=True):
        super().train(mode)
        self._heads.training = mode      # (its children are this module's children and were switched with them)
        return self

    def _cross_cutoff(self, complex_t):
        if not self.dynamic_max_cross:
            return self.cross_max_distance
        tr_sigma = self.tr_sigma_min ** (1 - complex_t['tr']) * self.tr_sigma_max ** complex_t['tr']      # diffusion_utils.t_to_sigma
        return tr_sigma * 3 + 20

    def embed(self, data, seed=None):
        """models/score_model.py:169-257: (lig_node_attr [N_lig, 84], rec_node_attr [N_rec, 84]) after the conv stack, for a collated batch.  With
        ``latent_dim`` (models/score_model.py:191-215, 310-408 with latent_h) the node rows are [x | sig | latent] (+ unconditional *
        node_unconditional_embedding) and the edge rows carry [latent[src] | latent[dst]] inside the fused op"""
        lig, rec = data['ligand'], data['receptor']
        if not lig.pos.is_cuda:
            raise RuntimeError('ddk TrainableScoreModel runs on the GPU only (no CPU fallback)')
        dev, B = lig.pos.device, int(data.num_graphs)
        complex_t = {k: data.complex_t[k].to(dev).float() for k in ('tr', 'rot', 'tor')}
        with torch.no_grad():
            lig_pos, rec_pos = lig.pos.detach().float(), rec.pos.detach().float()
            lig_batch, rec_batch = lig.batch.to(dev).long(), rec.batch.to(dev).long()
            sig = self.timestep_emb_func(complex_t['tr'])      # [B, 32]: a node's sigma embedding is its graph's
            n_lig = lig_pos.shape[0]
            n_cat = self.rec_node_embedding.num_categorical_features
            rec_x = rec.x.to(dev)
        if self.training and seed is None:
            seed = _draw_seed()
        seeds = [None if seed is None else _layer_seed(seed, len(self.conv_layers) + g) for g in range(3)]      # (the conv layers take 0 .. L - 1)

        if self.latent_dim:
            lig_node_attr, rec_node_attr, latent = self._embed_latent(data, sig, lig_batch, rec_batch, rec_x, n_cat)
        else:
            lig_node_attr = self.lig_node_embedding(lig.x.to(dev).long(), sig[lig_batch])
            rec_node_attr = self.rec_node_embedding(rec_x[:, :n_cat].long(), torch.cat([rec_x[:, n_cat:].float(), sig[rec_batch]], 1))
            latent = None
        edge_index, group_sizes, edge_emb, edge_sh = embed_edge_groups(self, lig_pos, lig_batch, rec_pos, rec_batch, data['ligand', 'ligand'],
                                                                       data['receptor', 'receptor'].edge_index, B, self._cross_cutoff(complex_t), sig,
                                                                       seeds, latent)
        node_attr = torch.cat([lig_node_attr, rec_node_attr], dim=0)
        node_attr = conv_stack(self.conv_layers, node_attr, edge_index, edge_emb, group_sizes, edge_sh, seed=seed)
        return node_attr[:n_lig], node_attr[n_lig:]

    def _latent_inputs(self, data, dev):
        """(latent_l [N_lig, L], latent_r [N_rec, L], unconditional_l [N_lig, 1] or None, unconditional_r) of a batch; a missing one raises by name"""
        out = []
        for side in ('ligand', 'receptor'):
            h = getattr(data[side], 'latent_h', None)
            if h is None:
                raise RuntimeError(f"ddk: TrainableScoreModel(latent_dim={self.latent_dim}) reads data['{side}'].latent_h; the batch has none")
            h = h.to(dev).float()
            if h.dim() != 2 or h.shape != (data[side].pos.shape[0], self.latent_dim):
                raise RuntimeError(f"ddk: data['{side}'].latent_h must be [nodes, latent_dim] = {(data[side].pos.shape[0], self.latent_dim)}; got {tuple(h.shape)}")
            out.append(h)
        for side in ('ligand', 'receptor'):
            u = None
            if self.latent_droprate > 0:
                u = getattr(data[side], 'unconditional', None)
                if u is None:
                    raise RuntimeError(f"ddk: TrainableScoreModel(latent_droprate={self.latent_droprate}) reads data['{side}'].unconditional; the batch has none")
                u = u.to(dev).float().detach().reshape(-1, 1)
                if u.shape[0] != data[side].pos.shape[0]:
                    raise RuntimeError(f"ddk: data['{side}'].unconditional must hold one value per node; got {tuple(u.shape)}")
            out.append(u)
        return out

    def _embed_latent(self, data, sig, lig_batch, rec_batch, rec_x, n_cat):
        """what the latent-conditioned model embeds differently (models/score_model.py:191-215, 310-408 with latent_h): the node rows [x | sig | latent]
        (+ unconditional * node_unconditional_embedding), and per edge group the latent keywords of ``fused_edge_embedding``"""
        dev = sig.device
        lat_l, lat_r, unc_l, unc_r = self._latent_inputs(data, dev)
        lig_node_attr = self.lig_node_embedding(data['ligand'].x.to(dev).long(), torch.cat([sig[lig_batch], lat_l], 1))
        rec_node_attr = self.rec_node_embedding(rec_x[:, :n_cat].long(), torch.cat([rec_x[:, n_cat:].float(), sig[rec_batch], lat_r], 1))
        unc = lambda u, name: {} if u is None else dict(unconditional=u.reshape(-1), unconditional_embedding=getattr(self, f'{name}_unconditional_embedding'))
        if unc_l is not None:
            lig_node_attr = lig_node_attr + unc_l * self.lig_node_unconditional_embedding
            rec_node_attr = rec_node_attr + unc_r * self.rec_node_unconditional_embedding
        return lig_node_attr, rec_node_attr, (dict(latent_a=lat_l, latent_b=lat_l, **unc(unc_l, 'lig_edge')),
                                              dict(latent_a=self.latent_dim, zero_latent=True, **unc(unc_l, 'cross_edge')),
                                              dict(latent_a=lat_r, latent_b=lat_r, **unc(unc_r, 'rec_edge')))

    def forward(self, data, seed=None):
        """``data``: a collated batch in the reference's layout (``data['ligand'].x / .pos / .batch / .edge_mask``, ``data['ligand', 'ligand'].edge_index /
        .edge_attr``, ``data['receptor'].x / .pos / .batch``, ``data['receptor', 'receptor'].edge_index``, ``data.complex_t`` with the three [B] times,
        ``data.num_graphs``); the graphs may be different complexes at different times.  ``seed``: of the dropout masks of the device ops (None: one draw
        from torch's default CPU generator per call in training).  Returns (tr_pred [B, 3], rot_pred [B, 3], tor_pred [sum R])."""
        lig = data['ligand']
        lig_node_attr, _ = self.embed(data, seed)
        dev = lig_node_attr.device
        complex_t = {k: data.complex_t[k].to(dev).float() for k in ('tr', 'rot', 'tor')}
        edge_mask = None if self.no_torsion else lig.edge_mask.to(dev)
        return self._heads(lig_node_attr, lig.pos, lig.batch.to(dev), data['ligand', 'ligand'].edge_index.to(dev), edge_mask, complex_t)


class LatentModelWrapper(nn.Module):
    """The tuple branch of the reference's ``ModelWrapper.forward`` (models/model_classes.py:62-85) for training: ``encoder(data)`` -> (latent_l [N_lig, L],
    latent_r [N_rec, L]) (any module; ``tensor_layers.ragged_gumbel_softmax`` is the sampling step the reference's encoders end in), the per-graph keep mask
    of classifier-free guidance, then the score model on the batch with ``latent_h`` and ``unconditional`` set:

        latent *= keep[batch][:, None]        unconditional = 1 - keep[batch]            keep [B] in {0, 1}; latent_droprate == 0: all ones, no unconditional

    ``forward(data, seed=None, keep=None)``: ``seed`` goes to the score model and, where its ``forward`` has a ``seed`` parameter (``latent_encoder.TPEncoder``), to
    the encoder; ``keep`` as given (``training.draw_latent_keep`` makes a seeded one, ``training.train_epoch`` passes it), else
    drawn with ``torch.bernoulli(1 - latent_droprate)`` as the reference does, in ``.train()`` and in ``.eval()`` alike (pass ``keep=torch.ones(B)``
    for a conditional evaluation).  ``training_latent_temperature`` is set on the encoder as
    ``encoder.latent_temperature`` before every call, as the reference does.  ``ctx`` / ``no_torsion`` are the score model's, so ``training.noise_batch`` and ``loss_function`` take the
    wrapper where they take the model."""

    def __init__(self, encoder, score_model, training_latent_temperature=1.0, latent_droprate=0.0):
        super().__init__()
        if not isinstance(score_model, TrainableScoreModel) or score_model.latent_dim < 1:
            raise RuntimeError('ddk: LatentModelWrapper takes a TrainableScoreModel with latent_dim > 0')
        if float(latent_droprate) != score_model.latent_droprate:
            raise RuntimeError(f'ddk: LatentModelWrapper: latent_droprate = {latent_droprate}, the score model was built with {score_model.latent_droprate}')
        self.encoder, self.score_model = encoder, score_model
        self._encoder_takes_seed = 'seed' in inspect.signature(encoder.forward).parameters
        self.training_latent_temperature, self.latent_droprate = float(training_latent_temperature), float(latent_droprate)

    @property
    def ctx(self):
        return self.score_model.ctx

    @property
    def no_torsion(self):
        return self.score_model.no_torsion

    def forward(self, data, seed=None, keep=None):
        self.encoder.latent_temperature = self.training_latent_temperature      # (as the reference hands it over)
        if self._encoder_takes_seed:      # (latent_encoder.TPEncoder: its dropout masks and Gumbel noise follow the step's seed, on sub-seeds of its own)
            latent_l, latent_r = self.encoder(data, seed=seed)
        else:
            latent_l, latent_r = self.encoder(data)
        dev, B = latent_l.device, int(data.num_graphs)
        lig_batch, rec_batch = data['ligand'].batch.to(dev).long(), data['receptor'].batch.to(dev).long()
        if self.latent_droprate > 0:
            if keep is None:
                keep = torch.bernoulli(torch.full((B,), 1.0 - self.latent_droprate))      # (in .eval() too, as the reference's wrapper)
            keep = torch.as_tensor(keep, dtype=torch.float32).reshape(-1).to(dev)
            if keep.shape[0] != B:
                raise RuntimeError(f'ddk: LatentModelWrapper takes keep [B] = {B} values; got {keep.shape[0]}')
            latent_l, latent_r = latent_l * keep[lig_batch][:, None], latent_r * keep[rec_batch][:, None]
            data['ligand'].unconditional, data['receptor'].unconditional = (1 - keep[lig_batch])[:, None], (1 - keep[rec_batch])[:, None]
        data['ligand'].latent_h, data['receptor'].latent_h = latent_l, latent_r
        return self.score_model(data, seed=seed)
