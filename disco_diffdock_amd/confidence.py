"""Host mirror of the reference's confidence model interface: what ``get_model(confidence_args, device,
t_to_sigma, no_parallel=True, confidence_mode=True)`` returns for ``all_atoms: true`` checkpoints (utils/model_utils.py:25-68 ->
models/all_atom_score_model.py), i.e. an object with ``load_state_dict(state_dict, strict=True)``, ``eval()`` and
``__call__(batch) -> confidence [B] or [B, k]``.  The forward runs in libddk.so (``ddk_confidence_forward``); there is no CPU
fallback.  Supported: the paper_confidence_model configuration family (ns=24, nv=6, sh_lmax=2, first-order irreps,
OldAtomEncoder, ESM features, BatchNorm); anything else raises."""
import numpy as np
import torch
from torch import nn

from .runtime import Context, Complex, config_from_args

import collections
_conf_cache = collections.OrderedDict()        # content key -> Complex (+ atoms), least recently used first


def confidence_config(args, device_index=0):
    g = lambda k, d: getattr(args, k, d)
    if not g('all_atoms', False):
        raise RuntimeError('ddk: the confidence model on the device is the all-atom model (all_atoms: true)')
    if g('sh_lmax', 2) != 2 or g('use_second_order_repr', False) or not g('use_old_atom_encoder', True) or g('latent_dim', 0):
        raise RuntimeError('ddk: confidence model: only sh_lmax=2, first-order irreps, OldAtomEncoder, no latents are implemented')
    import copy
    a = copy.copy(args)
    a.sh_lmax = 1                      # config_from_args validates the score-model family; the all-atom flag selects the l<=2 product
    d = config_from_args(a, device_index)
    cut = g('rmsd_classification_cutoff', None)
    d.update(all_atoms=1, num_confidence_outputs=len(cut) + 1 if isinstance(cut, list) else 1,
             confidence_no_batchnorm=int(bool(g('confidence_no_batchnorm', False))))
    return d


class ConfidenceModel(nn.Module):
    def __init__(self, args, device):
        super().__init__()
        dev_index = (device.index or 0) if isinstance(device, torch.device) and device.type == 'cuda' else 0
        self.device = torch.device('cuda', dev_index)
        self.cfg = confidence_config(args, dev_index)
        self.ctx = None
        self._loaded = False
        self.last_complex = None

    def load_state_dict(self, state_dict, strict=True):
        if self.ctx is not None:
            self.ctx.close()
        self.ctx = Context(**self.cfg)
        if strict:
            need = [k for k in ('lig_node_embedding.linear.weight', 'confidence_predictor.8.weight', 'conv_layers.0.fc.3.weight') if k not in state_dict]
            if need:
                raise RuntimeError(f'ddk confidence model: missing keys {need}')
        self.ctx.load_state_dict(state_dict)
        self._loaded = True
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def to(self, *a, **k):
        return self

    def complex_for(self, batch):
        """Complex (+ atoms) in this model's context for a batch of B copies of one all-atom complex graph."""
        from .score_model import arrays_from_batch, _fingerprint, _first_view
        B = batch.num_graphs
        g0, B00 = _first_view(batch, B)
        n_a0, E_aa0 = g0['atom'].num_nodes // B00, g0['atom', 'atom'].num_edges // B00
        import hashlib
        from .score_model import _bytes_of
        ha = hashlib.blake2b(digest_size=16)
        for a in (g0['atom'].x[:n_a0], g0['atom'].pos[:n_a0], g0['atom', 'atom'].edge_index[:, :E_aa0], g0['atom', 'receptor'].edge_index[:, :n_a0]):
            ha.update(_bytes_of(a))
            ha.update(b'|')
        key = (id(self.ctx),) + _fingerprint(batch, B) + (n_a0, ha.hexdigest())
        cx = _conf_cache.get(key)
        if cx is None or cx.max_batch < B:
            while len(_conf_cache) > 2:            # evicted complexes hand their device chunks back to the context's pool
                _conf_cache.popitem(last=False)
            arr = arrays_from_batch(batch, B)
            g, B0 = _first_view(batch, B)          # the first graph itself when the batch knows it (no concatenation of the 40 copies)
            n_a = g['atom'].num_nodes // B0
            E_aa = g['atom', 'atom'].num_edges // B0
            cx = Complex(self.ctx, arr, max_batch=B)
            cx.set_atoms(g['atom'].x[:n_a].cpu(), g['atom'].pos[:n_a].cpu(), g['atom', 'atom'].edge_index[:, :E_aa].cpu(),
                         g['atom', 'receptor'].edge_index[:, :n_a].cpu())
            _conf_cache[key] = cx
        _conf_cache.move_to_end(key)
        return cx, B

    def forward(self, data, check=True):
        """``check=False``: no host synchronisation here; the caller runs ``self.last_complex.confidence_counts()`` later (sampling()
        does it once per call, behind its own read-back)."""
        if not self._loaded:
            raise RuntimeError('ddk confidence model: load_state_dict() first')
        pos = data['ligand'].pos
        if not pos.is_cuda:
            raise RuntimeError('ddk confidence model runs on the GPU only (no CPU fallback)')
        t = data.complex_t['tr'] if hasattr(data, 'complex_t') else None
        # (check=False is sampling()'s own call, which has just set the times to 0 itself: reading a device tensor here would wait for the
        # whole reverse-diffusion loop queued in front of it)
        if check and t is not None and float(torch.as_tensor(t).abs().max()) != 0.0:
            raise RuntimeError('ddk confidence model: implemented for complex_t = 0 (utils/sampling.py:236)')
        cx, B = self.complex_for(data)
        self.last_complex = cx
        out = cx.confidence_forward(pos.reshape(B, -1, 3), check=check)
        return out.squeeze(dim=-1)


# ---- training: the all-atom confidence model with real parameters ------------------------------------------------------------------------------------------
from .synthetic import LIG_FEATURE_DIMS, REC_RESIDUE_FEATURE_DIMS      # noqa: E402

REC_ATOM_FEATURE_DIMS = (38, 119, 23, 38)      # datasets_utils/process_mols.py:81-86
CONVS = ('ll', 'lr', 'la', 'aa', 'al', 'ar', 'rr', 'rl', 'ra')      # the nine convs of a layer, in the order of conv_layers[9 l + k]


class OldAtomEncoder(nn.Module):
    """models/layers.py:91-116: one table per categorical feature, summed, plus a Linear over the 'scalar features' x[:, n_cat : n_cat + sigma_embed_dim];
    with language-model features a second Linear over [that | the LAST lm_dim columns of x].  With x = [ids | ESM | sigma embedding] the first slice is
    ESM[:32] and the second [ESM[32:] | sigma embedding], as the reference computes it.  The tables are read through ``gather_rows`` (no atomics)."""

    def __init__(self, emb_dim, feature_dims, sigma_embed_dim, lm_dim=0):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList()
        self.num_categorical_features, self.num_scalar_features, self.lm_dim = len(feature_dims), sigma_embed_dim, lm_dim
        for dim in feature_dims:
            emb = nn.Embedding(dim, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)
        self.linear = nn.Linear(sigma_embed_dim, emb_dim)
        if lm_dim:
            self.lm_embedding_layer = nn.Linear(lm_dim + emb_dim, emb_dim)

    def forward(self, x):
        from .tensor_layers import gather_rows
        n_cat = self.num_categorical_features
        emb = 0
        for i, table in enumerate(self.atom_embedding_list):
            emb = emb + gather_rows(table.weight, x[:, i].long())
        emb = emb + self.linear(x[:, n_cat:n_cat + self.num_scalar_features])
        if self.lm_dim:
            emb = self.lm_embedding_layer(torch.cat([emb, x[:, -self.lm_dim:]], dim=1))
        return emb


class _BatchNorm1d(nn.Module):
    """nn.BatchNorm1d with the four keys of the reference's checkpoints that the inference engine reads (no ``num_batches_tracked``)"""

    def __init__(self, n):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(n)), nn.Parameter(torch.zeros(n))
        self.register_buffer('running_mean', torch.zeros(n))
        self.register_buffer('running_var', torch.ones(n))

    def forward(self, x):
        return torch.nn.functional.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, self.training, 0.1, 1e-5)


class _SeededDropout(nn.Module):
    """Dropout whose mask is a pure function of the seed it is handed (a CPU generator: [B, ns] values per step)"""

    def __init__(self, p):
        super().__init__()
        self.p, self.seed = float(p), None

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        g = torch.Generator()
        g.manual_seed(int(self.seed if self.seed is not None else torch.randint(0, (1 << 62), (1,)).item()) & ((1 << 63) - 1))
        keep = (torch.rand(x.shape, generator=g) >= self.p).to(x.device, x.dtype)
        return x * keep / (1.0 - self.p)


class _SegMeanFunction(torch.autograd.Function):
    """mean of the rows of each graph (rows sorted by graph) through the fixed-order segmented sum; the backward is a gather"""

    @staticmethod
    def forward(fctx, x, batch, ptr):
        from .tensor_layers import _ctx_of
        count = (ptr[1:] - ptr[:-1]).clamp(min=1).to(x.dtype)
        order = torch.arange(x.shape[0], dtype=torch.int32, device=x.device)
        fctx.save_for_backward(batch, count)
        return _ctx_of(x).seg_sum(x, order, ptr) / count[:, None]

    @staticmethod
    def backward(fctx, grad):
        batch, count = fctx.saved_tensors
        return (grad / count[:, None])[batch], None, None


class TrainableConfidenceModel(nn.Module):
    """The reference's all-atom ``TensorProductScoreModel(confidence_mode=True)`` (models/all_atom_score_model.py) with real ``nn.Parameter``s, assembled
    from the differentiable device ops: six ``fused_edge_embedding`` calls, ``OldAtomEncoder`` through ``gather_rows``, nine all-atom convs per layer
    (``TensorProductConvLayer.forward_embedded_all_atom``: the third family of the radial tensor product, sh_lmax = 2), the pooled ligand mean through the
    segmented sum, the predictor in plain torch.  ``state_dict()`` has exactly the keys of the reference's checkpoint that ``ConfidenceModel`` reads, so
    a state dict goes to and from the inference engine with ``strict=True``.  Built from a model_parameters.yml Namespace; what ``confidence_config``
    refuses is refused here with the same words.  ``.train()`` / ``.eval()`` switch BatchNorm and dropout; both run the same kernels."""

    def __init__(self, args, device=None):
        super().__init__()
        cfg = confidence_config(args, 0)      # (the refusals)
        g = lambda k, d: getattr(args, k, d)
        ns = self.ns = int(cfg['ns'])
        self.num_conv_layers = int(cfg['num_conv_layers'])
        self.lig_max_radius, self.cross_max_distance = float(cfg['lig_max_radius']), float(cfg['cross_max_distance'])
        self.dynamic_max_cross = bool(cfg['dynamic_max_cross'])
        sd, dd, cd = int(cfg['sigma_embed_dim']), int(cfg['distance_embed_dim']), int(cfg['cross_distance_embed_dim'])
        if (ns, int(cfg['nv']), sd, dd, cd) != (24, 6, 32, 32, 32) or g('embedding_type', 'sinusoidal') != 'sinusoidal':
            raise RuntimeError('ddk: TrainableConfidenceModel: ns=24, nv=6 and 32-wide sinusoidal sigma and distance embeddings only')
        dropout, batch_norm = float(g('dropout', 0.0)), bool(cfg['batch_norm'])
        from .diffusion_utils import get_timestep_embedding
        from .tensor_layers import GaussianSmearing, TensorProductConvLayer
        self.timestep_emb_func = get_timestep_embedding('sinusoidal', sd, float(cfg['embedding_scale']))
        lm = int(cfg['lm_embedding_dim'])
        mlp = lambda k: nn.Sequential(nn.Linear(k, ns), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ns, ns))
        self.lig_node_embedding = OldAtomEncoder(ns, LIG_FEATURE_DIMS, sd)
        self.lig_edge_embedding = mlp(4 + sd + dd)
        self.rec_node_embedding = OldAtomEncoder(ns, REC_RESIDUE_FEATURE_DIMS, sd, lm)
        self.rec_edge_embedding = mlp(sd + dd)
        self.atom_node_embedding = OldAtomEncoder(ns, REC_ATOM_FEATURE_DIMS, sd)
        self.atom_edge_embedding = mlp(sd + dd)
        self.lr_edge_embedding, self.ar_edge_embedding, self.la_edge_embedding = mlp(sd + cd), mlp(sd + dd), mlp(sd + cd)
        self.lig_distance_expansion = GaussianSmearing(0.0, self.lig_max_radius, dd)
        self.rec_distance_expansion = GaussianSmearing(0.0, 30.0, dd)
        self.cross_distance_expansion = GaussianSmearing(0.0, self.cross_max_distance, cd)
        seq = [f'{ns}x0e', f'{ns}x0e + 6x1o', f'{ns}x0e + 6x1o + 6x1e', f'{ns}x0e + 6x1o + 6x1e + {ns}x0o']
        self.conv_layers = nn.ModuleList([TensorProductConvLayer(in_irreps=seq[min(l, 3)], sh_irreps='1x0e+1x1o+1x2e', out_irreps=seq[min(l + 1, 3)],
                                                                 n_edge_features=3 * ns, residual=False, batch_norm=batch_norm, dropout=dropout)
                                          for l in range(self.num_conv_layers) for _ in range(9)])
        k_out = int(cfg['num_confidence_outputs'])
        bn = (lambda: nn.Identity()) if cfg['confidence_no_batchnorm'] else (lambda: _BatchNorm1d(ns))
        p = float(g('confidence_dropout', 0.0))
        self.confidence_predictor = nn.Sequential(nn.Linear(2 * ns if self.num_conv_layers >= 3 else ns, ns), bn(), nn.ReLU(), _SeededDropout(p),
                                                  nn.Linear(ns, ns), bn(), nn.ReLU(), _SeededDropout(p), nn.Linear(ns, k_out))
        if device is not None:
            self.to(device)

    def used_parameters(self):
        """names of the parameters a forward reaches: all but convs 3..8 of the last layer (the reference's 'last layer optimisation')"""
        skip = tuple(f'conv_layers.{9 * (self.num_conv_layers - 1) + k}.' for k in range(3, 9))
        return [n for n, _ in self.named_parameters() if not n.startswith(skip)]

    def build_edges(self, data, B, tr_sigma):
        """the six edge lists, per graph, in plain torch without gradient (all_atom_score_model.py:329-428): ll = bonds + radius graph, lr at the dynamic
        cutoff 3 sigma_tr + 20 (or cross_max_distance), la at lig_max_radius; aa, ar and rr from the data"""
        from .train_model import CROSS_CAP, LIG_RADIUS_CAP, radius, radius_graph
        lig, rec, atom = data['ligand'], data['receptor'], data['atom']
        with torch.no_grad():
            dev = lig.pos.device
            lp, rp, ap = lig.pos.detach().float(), rec.pos.detach().float().to(dev), atom.pos.detach().float().to(dev)
            lb, rb, ab = lig.batch.to(dev).long(), rec.batch.to(dev).long(), atom.batch.to(dev).long()
            bonds = data['ligand', 'ligand'].edge_index.to(dev).long()
            ll = torch.cat([bonds, radius_graph(lp, self.lig_max_radius, lb, B, LIG_RADIUS_CAP)], 1)
            if self.dynamic_max_cross:
                cut = (tr_sigma * 3 + 20).reshape(-1, 1)
                lr = radius(rp / cut[rb], lp / cut[lb], 1, rb, lb, B, CROSS_CAP)
            else:
                lr = radius(rp, lp, self.cross_max_distance, rb, lb, B, CROSS_CAP)
            la = radius(ap, lp, self.lig_max_radius, ab, lb, B, CROSS_CAP)
            return dict(ll=ll, lr=lr, la=la, aa=data['atom', 'atom'].edge_index.to(dev).long(), ar=data['atom', 'receptor'].edge_index.to(dev).long(),
                        rr=data['receptor', 'receptor'].edge_index.to(dev).long()), bonds.shape[1], (lp, rp, ap), (lb, rb, ab)

    def forward(self, data, seed=None):
        """``data``: a collated batch of all-atom complex graphs in the reference's layout (different complexes, or copies of one); ``data.complex_t`` is
        used as sigma directly (all_atom_score_model.py:206-207).  ``seed``: of every dropout mask (None: one draw from torch's default CPU generator
        per call in training).  Returns the logits [B], or [B, k] with k confidence outputs."""
        from .runtime import Context
        from .tensor_layers import _draw_seed, _layer_seed, fused_edge_embedding, sh_second_order
        lig, rec, atom = data['ligand'], data['receptor'], data['atom']
        if not lig.pos.is_cuda:
            raise RuntimeError('ddk TrainableConfidenceModel runs on the GPU only (no CPU fallback)')
        dev, B, L, ns = lig.pos.device, int(data.num_graphs), self.num_conv_layers, self.ns
        tr_sigma = data.complex_t['tr'].to(dev).float()
        ei, n_bond, (lp, rp, ap), (lb, rb, ab) = self.build_edges(data, B, tr_sigma)
        if self.training and seed is None:
            seed = _draw_seed()
        sub = lambda i: None if seed is None else _layer_seed(seed, i)
        with torch.no_grad():
            sig = self.timestep_emb_func(tr_sigma)      # [B, 32]: a node's sigma embedding is its graph's (node_t = complex_t[batch])
            feat = torch.cat([data['ligand', 'ligand'].edge_attr.to(dev).float(), torch.zeros((ei['ll'].shape[1] - n_bond, 4), device=dev)], 0)
            li, ri, ai = lb.to(torch.int32), rb.to(torch.int32), ab.to(torch.int32)
        # 2. six edge embeddings; the atom graph's distances go through the LIGAND expansion
        E = {}
        for i, (k, mlp, exp, pa, pb, idx, ft) in enumerate((
                ('ll', self.lig_edge_embedding, self.lig_distance_expansion, lp, lp, li, feat),
                ('lr', self.lr_edge_embedding, self.cross_distance_expansion, lp, rp, li, None),
                ('la', self.la_edge_embedding, self.cross_distance_expansion, lp, ap, li, None),
                ('aa', self.atom_edge_embedding, self.lig_distance_expansion, ap, ap, ai, None),
                ('ar', self.ar_edge_embedding, self.rec_distance_expansion, ap, rp, ai, None),
                ('rr', self.rec_edge_embedding, self.rec_distance_expansion, rp, rp, ri, None))):
            emb, sh4 = fused_edge_embedding(mlp, exp, pa, pb, ei[k], sig, idx, feat=ft, seed=sub(9 * L + i))
            E[k] = (ei[k], emb, sh_second_order(sh4))
        # 3. node embeddings
        x = dict(l=self.lig_node_embedding(torch.cat([lig.x.to(dev).float(), sig[lb]], 1)),
                 r=self.rec_node_embedding(torch.cat([rec.x.to(dev).float(), sig[rb]], 1)),
                 a=self.atom_node_embedding(torch.cat([atom.x.to(dev).float(), sig[ab]], 1)))
        # 4. the convs: (receivers, senders, edge set, flipped) of [ll lr la aa al ar rr rl ra]; one pair of graphs per conv, shared by the layers
        plan = (('l', 'l', 'll', False), ('l', 'r', 'lr', False), ('l', 'a', 'la', False), ('a', 'a', 'aa', False), ('a', 'l', 'la', True),
                ('a', 'r', 'ar', False), ('r', 'r', 'rr', False), ('r', 'l', 'lr', True), ('r', 'a', 'ar', True))
        graphs = {}
        for k, (rv, sn, es, flip) in enumerate(plan):
            idx = torch.flip(E[es][0], dims=[0]) if flip else E[es][0]
            n_r, n_s = x[rv].shape[0], x[sn].shape[0]
            g = hg = None
            if idx.shape[1] > 0:
                g = Context.conv_graph(idx[0], idx[1], n_s, n_r)
                hg = g if rv == sn else Context.conv_graph(idx[0], idx[1] + n_r, n_r + n_s, n_r + n_s)
            graphs[k] = (idx, g, hg)
        for l in range(L):
            upd = {}
            for k, (rv, sn, es, flip) in enumerate(plan):
                if l == L - 1 and k >= 3:      # the last layer updates the ligand alone
                    break
                idx, g, hg = graphs[k]
                upd[k] = self.conv_layers[9 * l + k].forward_embedded_all_atom(x[rv], x[sn], idx, E[es][1], E[es][2], graph=g, hidden_graph=hg, seed=sub(9 * l + k))
            pad = lambda t, u: torch.nn.functional.pad(t, (0, u.shape[-1] - t.shape[-1]))
            new_l = pad(x['l'], upd[0]) + upd[0] + upd[2] + upd[1]
            if l != L - 1:
                x['a'] = pad(x['a'], upd[3]) + upd[3] + upd[4] + upd[5]
                x['r'] = pad(x['r'], upd[6]) + upd[6] + upd[8] + upd[7]
            x['l'] = new_l
        # 5. pooling and 6. the predictor
        scalar = torch.cat([x['l'][:, :ns], x['l'][:, -ns:]], dim=1) if L >= 3 else x['l'][:, :ns]
        ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(lb, minlength=B)[:B], 0)
        pooled = _SegMeanFunction.apply(scalar.contiguous(), lb, ptr)
        for j, m in enumerate(self.confidence_predictor):
            if isinstance(m, _SeededDropout):
                m.seed = sub(9 * L + 6 + j)
        return self.confidence_predictor(pooled).squeeze(dim=-1)
