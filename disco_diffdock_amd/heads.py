"""The score heads of the reference's ``TensorProductScoreModel.forward`` (models/score_model.py:259-308) from ``lig_node_attr`` on, as a trainable
module: ``ScoreHeads(lig_node_attr, pos, batch, bonds, edge_mask, complex_t) -> (tr_pred [B, 3], rot_pred [B, 3], tor_pred [sum R])`` with real
``nn.Parameter``s under the reference's names (``center_edge_embedding``, ``final_conv``, ``tr_final_layer``, ``rot_final_layer``,
``final_edge_embedding``, ``tor_bond_conv``, ``tor_final_layer``, and the ``offset`` buffers of the two distance expansions), so that
``load_state_dict(checkpoint, strict=False)`` takes the head keys of a full reference checkpoint.

The two convolutions are the device ops of csrc/k_hconv.hip (``tensor_layers.fused_head_conv``): no atomics, the same gradient bits on every run.  The
geometry (centre graph, bond graph, Gaussian smearing, spherical harmonics) is plain torch on the device without gradient: positions carry none in score
matching.  The gathers of node rows go through ``tensor_layers.gather_rows``, whose backward is a fixed-order segmented sum."""
import math
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from .diffusion_utils import get_timestep_embedding, t_to_sigma
from .runtime import DEFAULTS, Context
from .tensor_layers import GaussianSmearing, TensorProductConvLayer, _shape_context, gather_rows

BOND_CAP = 32      # neighbours of a bond centre (torch_cluster.radius' max_num_neighbors default; BOND_CAP of csrc/k_heads.hip)
_SQRT3, _SQRT5 = math.sqrt(3.0), math.sqrt(5.0)


def _sh1(vec):
    """o3.spherical_harmonics('1x0e + 1x1o', vec, normalize=True, normalization='component'): [1 | sqrt3 vec / |vec|]"""
    unit = vec / vec.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.cat([torch.ones_like(unit[:, :1]), _SQRT3 * unit], dim=-1)


def bond_tensor_block(edge_sh, bond_vec):
    """The 1o block T [E, 3] of ``FullTensorProduct('1x0e + 1x1o', '2e')(edge_sh, sh_2e(bond_vec))``, the only part of it tor_bond_conv reads:
    sqrt3 sum_jk w3j(1, 2, 1) s1_j y_k in closed form (csrc/k_heads.hip, heads_pre_kernel).  ``edge_sh`` [E, 4], ``bond_vec`` [E, 3] (any length)."""
    b = bond_vec / bond_vec.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    bx, by, bz = b.unbind(-1)
    s0, s1, s2 = edge_sh[:, 1], edge_sh[:, 2], edge_sh[:, 3]
    y0, y1, y2 = _SQRT5 * _SQRT3 * bx * bz, _SQRT5 * _SQRT3 * bx * by, _SQRT5 * (by * by - 0.5 * (bx * bx + bz * bz))
    y3, y4 = _SQRT5 * _SQRT3 * by * bz, _SQRT5 * (_SQRT3 * 0.5) * (bz * bz - bx * bx)
    ca, cb = 1.0 / math.sqrt(10.0), 1.0 / math.sqrt(30.0)
    return torch.stack([_SQRT3 * (-cb * s0 * y2 - ca * s0 * y4 + ca * s1 * y1 + ca * s2 * y0),
                        _SQRT3 * (ca * s0 * y1 + 2.0 * cb * s1 * y2 + ca * s2 * y3),
                        _SQRT3 * (ca * s0 * y0 + ca * s1 * y3 - cb * s2 * y2 + ca * s2 * y4)], dim=-1)


class ScoreHeads(nn.Module):
    """Constructor keywords follow models/score_model.py:15-24 as far as the heads read them; ``sigma_limits``: the six ``*_sigma_min`` / ``*_sigma_max``
    of the noise schedule (``runtime.DEFAULTS`` otherwise), read by ``scale_by_sigma``."""

    def __init__(self, ns=24, nv=6, sigma_embed_dim=32, distance_embed_dim=32, lig_max_radius=5.0, center_max_distance=30.0, dropout=0.0,
                 batch_norm=True, no_torsion=False, scale_by_sigma=True, embedding_scale=1000.0, sigma_limits=None):
        super().__init__()
        if ns != 24 or nv != 6:
            raise RuntimeError('ddk: the head kernels implement ns=24, nv=6')
        self.ns, self.no_torsion, self.scale_by_sigma = ns, bool(no_torsion), bool(scale_by_sigma)
        self.lig_max_radius = float(lig_max_radius)
        keys = ('tr_sigma_min', 'tr_sigma_max', 'rot_sigma_min', 'rot_sigma_max', 'tor_sigma_min', 'tor_sigma_max')
        self.cfg = SimpleNamespace(**{k: float((sigma_limits or DEFAULTS)[k]) for k in keys})      # (what training._sigmas reads of a context)
        self.timestep_emb_func = get_timestep_embedding('sinusoidal', sigma_embed_dim, embedding_scale)
        conv_out = f'{ns}x0e + {nv}x1o + {nv}x1e + {ns}x0o'
        self.center_distance_expansion = GaussianSmearing(0.0, center_max_distance, distance_embed_dim)
        self.center_edge_embedding = nn.Sequential(nn.Linear(distance_embed_dim + sigma_embed_dim, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.final_conv = TensorProductConvLayer(in_irreps=conv_out, sh_irreps='1x0e+1x1o', out_irreps='2x1o + 2x1e', n_edge_features=2 * ns,
                                                 residual=False, dropout=dropout, batch_norm=batch_norm)
        self.tr_final_layer = nn.Sequential(nn.Linear(1 + sigma_embed_dim, ns), nn.Dropout(dropout), nn.ReLU(), nn.Linear(ns, 1))
        self.rot_final_layer = nn.Sequential(nn.Linear(1 + sigma_embed_dim, ns), nn.Dropout(dropout), nn.ReLU(), nn.Linear(ns, 1))
        if not self.no_torsion:
            self.lig_distance_expansion = GaussianSmearing(0.0, lig_max_radius, distance_embed_dim)
            self.final_edge_embedding = nn.Sequential(nn.Linear(distance_embed_dim, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
            self.tor_bond_conv = TensorProductConvLayer(in_irreps=conv_out, sh_irreps='1x1o+1x2e+1x2o+1x3o', out_irreps=f'{ns}x0o + {ns}x0e',
                                                        n_edge_features=3 * ns, residual=False, dropout=dropout, batch_norm=batch_norm)
            self.tor_final_layer = nn.Sequential(nn.Linear(2 * ns, ns, bias=False), nn.Tanh(), nn.Dropout(dropout), nn.Linear(ns, 1, bias=False))

    # ---- geometry: no gradient ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _graph_ranges(batch, B):
        """(first atom, atom count) per graph; the atoms of a graph are contiguous, as a collated batch has them"""
        if batch.numel() > 1 and bool((batch[1:] < batch[:-1]).any()):
            raise RuntimeError('ddk: ScoreHeads takes the atoms grouped by graph (batch ascending), as a collated batch has them')
        count = torch.bincount(batch, minlength=B)
        return torch.cumsum(count, 0) - count, count

    def _center_graph(self, pos, batch, B, node_sigma_emb):
        """build_center_conv_graph (score_model.py:410-423): edge (graph <- atom), its attributes before the embedding and its spherical harmonics.  The
        centroid is a fixed-order sum over the graph's atoms (the reference's index_add_ uses atomics)."""
        N = pos.shape[0]
        edge_index = torch.stack([batch, torch.arange(N, device=pos.device)])
        graph = Context.conv_graph(edge_index[0], edge_index[1], N, B)
        center = _shape_context(pos.device.index or 0).seg_sum(pos, graph.src_order, graph.src_ptr) / graph.src_count.clamp(min=1).unsqueeze(1)
        edge_vec = pos - center[batch]
        edge_attr = torch.cat([self.center_distance_expansion(edge_vec.norm(dim=-1)), node_sigma_emb], 1)
        return edge_index, graph, edge_attr, _sh1(edge_vec)

    def _bond_graph(self, pos, batch, B, rot_bonds):
        """build_bond_conv_graph (score_model.py:425-438) with torch_cluster.radius' rule as heads_pre_kernel states it: the atoms of the bond's graph
        within lig_max_radius of the bond centre (squared distance below the squared radius), at most 32 per bond in ascending atom index."""
        u, v = rot_bonds
        R, N = u.shape[0], pos.shape[0]
        first, count = self._graph_ranges(batch, B)
        bond_pos = (pos[u] + pos[v]) / 2
        bb = batch[u]
        window = torch.arange(int(count.max()), device=pos.device)
        valid = window[None, :] < count[bb][:, None]
        cand = (first[bb][:, None] + window[None, :]).clamp(max=N - 1)      # [R, largest graph]: the atoms of the bond's graph, ascending
        d2 = (pos[cand] - bond_pos[:, None, :]).pow(2).sum(-1)
        inside = valid & (d2 < self.lig_max_radius ** 2)
        keep = inside & (torch.cumsum(inside, 1) <= BOND_CAP)
        src, col = keep.nonzero(as_tuple=True)      # row-major: by bond, then by atom index
        dst = cand[src, col]
        edge_vec = pos[dst] - bond_pos[src]
        edge_sh = _sh1(edge_vec)
        T = bond_tensor_block(edge_sh, (pos[v] - pos[u])[src])
        edge_sh4 = torch.cat([torch.ones_like(T[:, :1]), T], dim=1)      # (., T): what the torsion op reads of the full tensor product
        return torch.stack([src, dst]), Context.conv_graph(src, dst, N, R), self.lig_distance_expansion(edge_vec.norm(dim=-1)), edge_sh4

    def _score_norms(self, complex_t, batch, rot_bonds):
        """host lookups of scale_by_sigma: tr_sigma [B], so3.score_norm(rot_sigma) [B], sqrt(torus.score_norm(tor_sigma)) per rotatable bond"""
        from .training import _score_norm_tables, so3_eps_index, torus_sigma_index
        t = {k: complex_t[k].detach().double().cpu().numpy() for k in ('tr', 'rot', 'tor')}
        tr_sigma, rot_sigma, tor_sigma = t_to_sigma(t['tr'], t['rot'], t['tor'], self.cfg)
        so3_tab, torus_tab = _score_norm_tables(self)
        dev = batch.device
        f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)
        tor_norm = None
        if rot_bonds is not None:
            per_graph = f(np.sqrt(np.asarray(torus_tab)[torus_sigma_index(tor_sigma.astype(np.float32))]))
            tor_norm = per_graph[batch[rot_bonds[0]]]
        return f(tr_sigma), f(np.asarray(so3_tab)[so3_eps_index(rot_sigma.astype(np.float32))]), tor_norm

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------------
    def forward(self, lig_node_attr, pos, batch, bonds, edge_mask, complex_t):
        """``lig_node_attr`` [N, 84] (what ``conv_stack`` / ``embed`` return for the ligand atoms), ``pos`` [N, 3], ``batch`` [N] the graph of an atom
        (ascending), ``bonds`` [2, nb] the ligand's bond edges as global atom indices with ``edge_mask`` [nb] marking the rotatable ones
        (``data['ligand', 'ligand'].edge_index`` and ``data['ligand'].edge_mask``), ``complex_t``: dict of the three [B] times 'tr', 'rot', 'tor'."""
        if not lig_node_attr.is_cuda:
            raise RuntimeError('ddk ScoreHeads runs on the GPU only (no CPU fallback)')
        ns, B = self.ns, complex_t['tr'].shape[0]
        batch = batch.long()
        rot_bonds = None
        if not self.no_torsion and bonds is not None and edge_mask is not None:
            rot_bonds = bonds.long()[:, edge_mask.bool()]
            if rot_bonds.shape[1] == 0:
                rot_bonds = None
        with torch.no_grad():
            pos = pos.detach().float()
            graph_sigma_emb = self.timestep_emb_func(complex_t['tr'].float())
            c_index, c_graph, c_attr, c_sh = self._center_graph(pos, batch, B, graph_sigma_emb[batch])
            if rot_bonds is not None:
                t_index, t_graph, t_attr, t_sh = self._bond_graph(pos, batch, B, rot_bonds)
            if self.scale_by_sigma:
                tr_sigma, rot_norm_tab, tor_norm_tab = self._score_norms(complex_t, batch, rot_bonds)

        # translational and rotational score vectors: the centre graph's edge e reads atom e, so the "gather" is the slice itself
        c_attr = torch.cat([self.center_edge_embedding(c_attr), lig_node_attr[:, :ns]], -1)
        global_pred = self.final_conv._forward_head(lig_node_attr, c_index, c_attr, c_sh, B, 'mean', graph=c_graph)
        tr_pred = global_pred[:, :3] + global_pred[:, 6:9]
        rot_pred = global_pred[:, 3:6] + global_pred[:, 9:]
        tr_norm = torch.linalg.vector_norm(tr_pred, dim=1).unsqueeze(1)
        tr_pred = tr_pred / tr_norm * self.tr_final_layer(torch.cat([tr_norm, graph_sigma_emb], dim=1))
        rot_norm = torch.linalg.vector_norm(rot_pred, dim=1).unsqueeze(1)
        rot_pred = rot_pred / rot_norm * self.rot_final_layer(torch.cat([rot_norm, graph_sigma_emb], dim=1))
        if self.scale_by_sigma:
            tr_pred = tr_pred / tr_sigma.unsqueeze(1)
            rot_pred = rot_pred * rot_norm_tab.unsqueeze(1)
        if rot_bonds is None:
            return tr_pred, rot_pred, torch.empty(0, device=lig_node_attr.device)

        # torsional components
        xs = lig_node_attr[:, :ns]
        tor_bond_attr = gather_rows(xs, rot_bonds[0]) + gather_rows(xs, rot_bonds[1])
        t_attr = torch.cat([self.final_edge_embedding(t_attr), gather_rows(xs, t_index[1], t_graph, 'dst'), gather_rows(tor_bond_attr, t_index[0], t_graph, 'src')], -1)
        tor_pred = self.tor_bond_conv._forward_head(lig_node_attr, t_index, t_attr, t_sh, rot_bonds.shape[1], 'mean', graph=t_graph)
        tor_pred = self.tor_final_layer(tor_pred).squeeze(1)
        if self.scale_by_sigma:
            tor_pred = tor_pred * tor_norm_tab
        return tr_pred, rot_pred, tor_pred
