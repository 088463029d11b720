"""fp64 (and host fp32) restatements for the tests of the ns = 24 / nv = 4 tensor-product ops and of latent_encoder.TPEncoder, composed from the project's
oracle (oracle.score_model_ref: faster_tensor_product, tp_conv_layer, gaussian_smearing, atom_encoder, mlp2; oracle.cluster_lite), which is general in
ns / nv and differentiable.  Everything here is torch on the host: gradients come from autograd, in the dtype asked for.

* ``irreps(l, nv)``: the in / out irreps of conv layer l of get_irrep_seq(24, nv, False)
* ``tp`` / ``rtp`` / ``rconv``: FasterTensorProduct, the radial tensor product (w_e = W2[g] h_e + b2[g]) and the radial conv (gather over dst, mean over
  src) with their vector-Jacobian products
* ``bn_train``: e3nn's BatchNorm on the batch statistics
* ``encoder_logits``: models/latent_encoder.py:171-323 without virtual nodes, vocab 1, on ``data['ligand'].orig_pos_torch``"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import e3nn_lite as o3
from oracle import score_model_ref as smr
from oracle.cluster_lite import radius, radius_graph

SH = '1x0e+1x1o'


def irreps(l, nv, ns=24):
    return smr.ScoreModelConfig(ns=ns, nv=nv).conv_irreps(l)


def shape(l, nv, ns=24):
    """A, P, Q, C, O, R, B, W, din, dout of conv layer l, from the oracle's own weight shapes"""
    i, o = irreps(l, nv, ns)
    mi, mo = smr._muls(i), smr._muls(o)
    ws = smr.faster_tp_weight_shapes(i, o)
    R = [ws[k][0] if ws[k][1] else 0 for k in ('0e', '1o', '1e', '0o')]
    O = [mo[k] for k in ('0e', '1o', '1e', '0o')]
    B = [sum(r * c for r, c in zip(R[:k], O)) for k in range(5)]
    return dict(A=mi['0e'], P=mi['1o'], Q=mi['1e'], C=mi['0o'], O=O, R=R, B=B, W=B[4], din=smr.irreps_dim(i), dout=smr.irreps_dim(o))


def out_slices(s):
    """the irrep slices of an out row / a node row of width dout"""
    O, at, out = s['O'], 0, {}
    for k, (name, d) in enumerate((('0e', 1), ('1o', 3), ('1e', 3), ('0o', 1))):
        if O[k]:
            out[name] = slice(at, at + O[k] * d)
            at += O[k] * d
    return out


def in_slices(s):
    at, out = 0, {}
    for name, m, d in (('0e', s['A'], 1), ('1o', s['P'], 3), ('1e', s['Q'], 3), ('0o', s['C'], 1)):
        if m:
            out[name] = slice(at, at + m * d)
            at += m * d
    return out


def weight_slices(s):
    return {name: slice(s['B'][k], s['B'][k + 1]) for k, name in enumerate(('0e', '1o', '1e', '0o')) if s['R'][k] * s['O'][k]}


def _leaves(arrays, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in arrays.items()}


def _vjp(out, leaves, g, dtype):
    out.backward(torch.as_tensor(np.asarray(g)).to(dtype))
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items()}


def tp(l, nv, x, sh, w, g, dtype=torch.float64):
    """(out, {x, sh, w: gradient}) of FasterTensorProduct for the incoming gradient g"""
    t = _leaves(dict(x=x, sh=sh, w=w), dtype)
    return _vjp(smr.faster_tensor_product(t['x'], t['sh'], t['w'], *irreps(l, nv)), t, g, dtype)


def _rtp_rows(l, nv, x_rows, t, offsets):
    w = torch.cat([t['h'][offsets[k]:offsets[k + 1]] @ t['w2'][k].T + t['b2'][k] for k in range(len(offsets) - 1)])
    return smr.faster_tensor_product(x_rows, t['sh'], w, *irreps(l, nv))


def rtp(l, nv, x, sh, h, offsets, w2, b2, g, dtype=torch.float64):
    """(out, {x, sh, h, w2, b2: gradient}) of the radial tensor product"""
    t = _leaves(dict(x=x, sh=sh, h=h, w2=w2, b2=b2), dtype)
    return _vjp(_rtp_rows(l, nv, t['x'], t, offsets), t, g, dtype)


def rconv(l, nv, x, src, dst, n_out, sh, h, offsets, w2, b2, g, dtype=torch.float64):
    """(out_nodes, {x, sh, h, w2, b2: gradient}) of the radial conv: rows of x gathered over dst, the mean over src (a node without edges: zeros)"""
    t = _leaves(dict(x=x, sh=sh, h=h, w2=w2, b2=b2), dtype)
    src, dst = torch.as_tensor(np.asarray(src)).long(), torch.as_tensor(np.asarray(dst)).long()
    rows = _rtp_rows(l, nv, t['x'][dst], t, offsets)
    count = torch.bincount(src, minlength=n_out).clamp(min=1).to(dtype)
    out = torch.zeros((n_out, rows.shape[1]), dtype=dtype).index_add(0, src, rows) / count[:, None]
    return _vjp(out, t, g, dtype)


def bn_train(x, muls, weight, bias, eps=1e-5):
    """e3nn's BatchNorm (affine, reduce='mean', normalization='component') on the batch statistics; returns (y, batch mean of the scalars, batch mean
    square per channel): scalars (0e) lose their mean and get the bias, every channel is divided by the root of its mean square"""
    cols, means, norms, ix, iw, ib = [], [], [], 0, 0, 0
    for k, (mul, d) in enumerate(zip(muls, (1, 3, 3, 1))):
        if not mul:
            continue
        f = x[:, ix:ix + mul * d].reshape(x.shape[0], mul, d)
        if k == 0:
            mean = f.mean(dim=(0, 2))
            means.append(mean)
            f = f - mean.reshape(1, mul, 1)
        ms = (f * f).mean(dim=(0, 2))
        norms.append(ms)
        f = f / torch.sqrt(ms + eps).reshape(1, mul, 1) * weight[iw:iw + mul].reshape(1, mul, 1)
        if k == 0:
            f = f + bias[ib:ib + mul].reshape(1, mul, 1)
            ib += mul
        ix, iw = ix + mul * d, iw + mul
        cols.append(f.reshape(x.shape[0], mul * d))
    return torch.cat(cols, dim=1), torch.cat(means), torch.cat(norms)


def conv_layer(P, prefix, l, nv, node_attr, edge_index, edge_attr, edge_sh, batch_norm, training):
    """TensorProductConvLayer.forward (models/tensor_layers.py:147-168) through the oracle's tp_conv_layer; BatchNorm on the batch statistics in training
    (also returns the (mean, mean square) the running buffers are moved by) or on the running buffers"""
    i, o = irreps(l, nv)
    stats = None
    if batch_norm and training:
        agg = smr.tp_conv_layer(P, prefix, node_attr, edge_index, edge_attr, edge_sh, i, SH, o, residual=False, batch_norm=False, faster=True, edge_groups=4)
        y, mean, ms = bn_train(agg, shape(l, nv)['O'], P[f'{prefix}.batch_norm.weight'], P[f'{prefix}.batch_norm.bias'])
        stats = (mean.detach(), ms.detach())
        out = y + F.pad(node_attr, (0, y.shape[-1] - node_attr.shape[-1]))
    else:
        out = smr.tp_conv_layer(P, prefix, node_attr, edge_index, edge_attr, edge_sh, i, SH, o, residual=True, batch_norm=batch_norm, faster=True,
                                edge_groups=4)
    return out, stats


def _predictor(x, P, prefix, batchnorm, training, stats):
    """Linear, [BatchNorm1d], ReLU, Linear, [BatchNorm1d], ReLU, Linear under keys 0, 1, 4, 5, 8 (dropout rate 0)"""
    for lin, bn in ((0, 1), (4, 5)):
        x = F.linear(x, P[f'{prefix}.{lin}.weight'], P[f'{prefix}.{lin}.bias'])
        if batchnorm:
            if training:
                stats[f'{prefix}.{bn}'] = (x.mean(0).detach(), x.var(0, unbiased=True).detach())
            x = F.batch_norm(x, P[f'{prefix}.{bn}.running_mean'].clone(), P[f'{prefix}.{bn}.running_var'].clone(), P[f'{prefix}.{bn}.weight'],
                             P[f'{prefix}.{bn}.bias'], training=training, momentum=0.1, eps=1e-5)
        x = torch.relu(x)
    return F.linear(x, P[f'{prefix}.8.weight'], P[f'{prefix}.8.bias'])


def atom_encoder(x, P, prefix, n_cat):
    """models/layers.py:140-149 (AtomEncoder.forward): the summed embedding tables, then the Linear over [sum | additional features] only where the module
    has additional features (the oracle's atom_encoder restates the score model's, which always has the sigma embedding)"""
    if x.shape[1] > n_cat:
        return smr.atom_encoder(x, P, prefix, n_cat)
    assert f'{prefix}.additional_features_embedder.weight' not in P
    emb = 0
    for i in range(n_cat):
        emb = emb + P[f'{prefix}.atom_embedding_list.{i}.weight'][x[:, i].long()]
    return emb


def encoder_logits(P, cfg, data, dtype=torch.float64, training=False, hidden=None):
    """models/latent_encoder.py:171-323 (no virtual nodes, latent_vocab 1, use_oracle): (logit_l [N_lig, D], logit_r [N_rec, D], stats).  ``cfg``: dict with
    nv, num_conv_layers, lig_max_radius, rec_max_radius, cross_max_distance, batch_norm, latent_batchnorm; ``P``: the encoder's state dict in ``dtype``
    (leaves that require grad get their gradient from the caller's backward); ``stats``: what the norm layers' running buffers are moved by in training.
    ``hidden``: a dict that receives every pre-activation in front of a ReLU of the three edge embeddings and of the conv layers' radial MLPs."""
    ns, nv, L = 24, cfg['nv'], cfg['num_conv_layers']
    lig, rec = data['ligand'], data['receptor']
    pos_e, rec_pos = lig.orig_pos_torch.to(dtype), rec.pos.to(dtype)
    lin = lambda row, name: row @ P[f'{name}.weight'].T + P[f'{name}.bias']

    def embedding(name, row):
        if hidden is not None:
            hidden[f'{name}_edge_embedding'] = lin(row, f'{name}_edge_embedding.0').detach()
        return smr.mlp2(row, P, f'{name}_edge_embedding', 0, 3)

    radius_edges = radius_graph(pos_e, cfg['lig_max_radius'], lig.batch)
    bonds = data['ligand', 'ligand']
    lig_ei = torch.cat([bonds.edge_index, radius_edges], 1).long()
    feat = torch.cat([bonds.edge_attr.to(dtype), torch.zeros(radius_edges.shape[-1], 4, dtype=dtype)], 0)
    vec = pos_e[lig_ei[1]] - pos_e[lig_ei[0]]
    lig_emb = embedding('lig', torch.cat([feat, smr.gaussian_smearing(vec.norm(dim=-1), cfg['lig_max_radius'], 32, dtype)], 1))
    lig_sh = smr._sh(vec, o3.Irreps.spherical_harmonics(1))
    lig_x = atom_encoder(lig.x.to(dtype), P, 'lig_node_embedding', len(smr.LIG_FEATURE_DIMS))

    rec_ei = data['receptor', 'receptor'].edge_index.long()
    vec = rec_pos[rec_ei[1]] - rec_pos[rec_ei[0]]
    rec_emb = embedding('rec', smr.gaussian_smearing(vec.norm(dim=-1), cfg['rec_max_radius'], 32, dtype))
    rec_sh = smr._sh(vec, o3.Irreps.spherical_harmonics(1))
    rec_x = atom_encoder(rec.x.to(dtype), P, 'rec_node_embedding', len(smr.REC_FEATURE_DIMS))

    lr_ei = radius(rec_pos, pos_e, cfg['cross_max_distance'], rec.batch, lig.batch, max_num_neighbors=10000)
    vec = rec_pos[lr_ei[1]] - pos_e[lr_ei[0]]
    lr_emb = embedding('cross', smr.gaussian_smearing(vec.norm(dim=-1), cfg['cross_max_distance'], 32, dtype))
    lr_sh = smr._sh(vec, o3.Irreps.spherical_harmonics(1))

    n_lig = lig_x.shape[0]
    node_attr = torch.cat([lig_x, rec_x], 0)
    lr = torch.stack([lr_ei[0], lr_ei[1] + n_lig])
    edge_index = torch.cat([lig_ei, lr, rec_ei + n_lig, torch.flip(lr, dims=[0])], 1)
    edge_emb, edge_sh = torch.cat([lig_emb, lr_emb, rec_emb, lr_emb], 0), torch.cat([lig_sh, lr_sh, rec_sh, lr_sh], 0)
    offs = np.cumsum([0, lig_ei.shape[1], lr.shape[1], rec_ei.shape[1], lr.shape[1]])
    stats = {}
    for l in range(L):
        ea = torch.cat([edge_emb, node_attr[edge_index[0], :ns], node_attr[edge_index[1], :ns]], -1)
        ea = [ea[offs[k]:offs[k + 1]] for k in range(4)]
        if hidden is not None:
            for k in range(4):
                hidden[f'conv_layers.{l}.fc.{k}'] = lin(ea[k], f'conv_layers.{l}.fc.{k}.0').detach()
        node_attr, st = conv_layer(P, f'conv_layers.{l}', l, nv, node_attr, edge_index, ea, edge_sh, cfg['batch_norm'], training)
        if st is not None:
            stats[f'conv_layers.{l}.batch_norm'] = st
    scalar = torch.cat([node_attr[:, :ns], node_attr[:, -ns:]], 1) if L >= 3 else node_attr[:, :ns]
    logit_l = _predictor(scalar[:n_lig], P, 'latent_s_predictor', cfg['latent_batchnorm'], training, stats)
    logit_r = _predictor(scalar[n_lig:], P, 'latent_r_predictor', cfg['latent_batchnorm'], training, stats)
    return logit_l, logit_r, stats
