"""Host-side mirror of the reference's models/tensor_layers.py interface for the hot path, backed by
libddk.so.  Same class names, constructor arguments, forward signatures and state_dict keys, so that the
parity tests read like tests of the reference modules:

* ``FasterTensorProduct(in_irreps, sh_irreps, out_irreps).forward(in_, sh, weight)``   tensor_layers.py:39-116
* ``TensorProductConvLayer(...).forward(node_attr, edge_index, edge_attr, edge_sh, out_nodes=None, reduce='mean')``
                                                                                          tensor_layers.py:119-168
* ``GaussianSmearing``                                                                   tensor_layers.py:171-181
* ``fused_radial_tp(tp, fc, x_dst, edge_sh, edge_attr)``: the radial MLP's last Linear, the cat and the tensor product
  of tensor_layers.py:154-156 as one differentiable op that never stores the per-edge weights (training)
* ``fused_radial_conv(tp, fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes=None, graph=None)``: lines 153-159, from the
  node features to the scatter-mean, as one differentiable op: the gather inside the kernels, the mean a fixed-order sum,
  no atomics (the same gradient bits on every run); ``hidden=`` takes the hidden activation made by ``fused_radial_hidden``
* ``fused_radial_hidden(fc, node_attr, edge_emb, group_offsets, graph, seed=None)``: the cat of the embed loop
  (score_model.py:227-230) and ``fc[g][:4]`` as one differentiable op from the edge embedding [E, ns]: no [E, 72] row, no
  atomics, a counter-based dropout mask
* ``TensorProductConvLayer.forward_embedded(...)`` and ``conv_stack(conv_layers, ...)``: one step of that loop, and the loop
* ``fused_head_conv(head, fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes, graph=None, hidden=None)``: lines 153-159 for the two score
  heads (final_conv, tor_bond_conv: ``faster=False``, e3nn's FullyConnectedTensorProduct, one FCBlock) as one differentiable op, no atomics
* ``gather_rows(x, index, graph=None, side='dst')``: a gather whose backward is a fixed-order segmented sum
* ``fused_edge_embedding(mlp, expansion, pos_a, pos_b, edge_index, sig, sig_index, feat=None, seed=None)``: one edge group of the embed in front of the
  conv stack (score_model.py:191-225): the edge embedding [E, ns] and the spherical harmonics from the coordinates, nothing kept per edge

Only the configurations the shipped models use are implemented on the device (ns=24, sh_lmax=1, 2-layer ReLU radial MLP; nv=6, the score model, and for the
conv layers nv=4, the DisCo latent encoder): the conv layers (faster=True, edge_groups=4, residual=True) and the two heads (nv=6; faster=False,
edge_groups=1, residual=False); anything else raises.

``TensorProductConvLayer`` trains: in ``.train()`` its forward is ``fused_radial_conv``, e3nn's BatchNorm on the batch
statistics (plain torch, ``_BatchNormParams.forward``) and the padded residual.  In ``.eval()`` it is the fused inference
kernel (``ddk_conv_forward``), unchanged; an nv=4 layer has no inference kernel and evaluates with the training ops.  ``conv_stack`` trains the whole stack of them from the edge embedding with the
same bits on every run.  In a head configuration the layer is ``fused_head_conv`` plus BatchNorm in training and in evaluation
(``heads.ScoreHeads`` is the module on top); ``train_model.TrainableScoreModel`` assembles the whole model.  The latent-conditioned (DisCo) score model trains
through ``fused_edge_embedding``'s latent columns and ``ragged_gumbel_softmax``; ``latent_encoder.TPEncoder`` is the encoder in front.  What still does not
train: the AR predictor, the all-atom SCORE model, any other ns / nv.  The all-atom CONFIDENCE model's conv layer (sh_lmax = 2, e3nn's
FullyConnectedTensorProduct: ``FullyConnectedTensorProduct``, ``sh_second_order``, ``TensorProductConvLayer`` with second-order sh_irreps) trains on the third
shape family of the radial ops; ``confidence.TrainableConfidenceModel`` is the model on top.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .runtime import HEAD_CENTER, HEAD_TORSION, TP_AA, TP_NV4, Context, head_tp_shape, tp_id_shape, tp_layer_shape

_ORDER = ('0e', '1o', '1e', '0o')
_DIM = {'0e': 1, '1o': 3, '1e': 3, '0o': 1}


def parse_irreps(irreps):
    """'24x0e + 6x1o' -> {'0e':24,'1o':6,'1e':0,'0o':0}; order must be the reference's (0e,1o,1e,0o)."""
    muls = {k: 0 for k in _ORDER}
    seen = []
    for chunk in str(irreps).split('+'):
        chunk = chunk.strip()
        if not chunk:
            continue
        mul, ir = chunk.split('x') if 'x' in chunk else ('1', chunk)
        ir = ir.strip()
        if ir not in muls:
            raise RuntimeError(f'ddk: unsupported irrep {ir!r} (sh_lmax=1 first-order model only)')
        muls[ir] = int(mul)
        seen.append(ir)
    if seen != [k for k in _ORDER if k in seen]:
        raise RuntimeError(f'ddk: irreps {irreps!r} are not in 0e,1o,1e,0o order')
    return muls


def _irreps_list(irreps):
    """'24x0o + 24x0e' -> [(24, '0o'), (24, '0e')]: the (mul, irrep) pairs in the order written, entries of multiplicity 0 left out"""
    out = []
    for chunk in str(irreps).split('+'):
        chunk = chunk.strip()
        if not chunk:
            continue
        mul, ir = chunk.split('x') if 'x' in chunk else ('1', chunk)
        ir = ir.strip()
        if ir not in _DIM:
            raise RuntimeError(f'ddk: unsupported irrep {ir!r} (sh_lmax=1 first-order model only)')
        if int(mul):
            out.append((int(mul), ir))
    return out


def irrep_to_size(irreps):
    return sum(m * _DIM[k] for k, m in parse_irreps(irreps).items())


SH_SECOND_ORDER = '1x0e+1x1o+1x2e'      # o3.Irreps.spherical_harmonics(2): the sh irreps of the all-atom (confidence) model


def _is_second_order_sh(sh_irreps):
    return sh_irreps is not None and str(sh_irreps).replace(' ', '') == SH_SECOND_ORDER


def layer_index(in_irreps, out_irreps, ns=24, nv=None, sh_irreps=None):
    """The `layer` argument of the tensor-product ops for these irreps (get_irrep_seq, tensor_layers.py:12-27): 0..3 for the score model's family
    (nv = 6), ``TP_NV4 + l`` for the latent encoder's (nv = 4).  ``nv``: one family alone (None: both are searched).  ``sh_irreps`` = '1x0e + 1x1o + 1x2e'
    names the all-atom family (e3nn's FullyConnectedTensorProduct on the nv = 6 irreps): ``TP_AA + l``."""
    i, o = tuple(parse_irreps(in_irreps).values()), tuple(parse_irreps(out_irreps).values())
    if _is_second_order_sh(sh_irreps):
        for l in range(4):
            s = tp_layer_shape(l, 24, 6)
            if ns == 24 and nv in (None, 6) and (s['A'], s['P'], s['Q'], s['C']) == i and s['O'] == o:
                return TP_AA + l
        raise RuntimeError(f'ddk: no fused kernel for irreps {in_irreps} (x) {sh_irreps} -> {out_irreps} (the all-atom family is compiled in for ns=24, nv=6)')
    for fam_nv, base in ((6, 0), (4, TP_NV4)):
        if nv not in (None, fam_nv) or ns != 24:
            continue
        for l in range(4):
            s = tp_layer_shape(l, ns, fam_nv)
            if (s['A'], s['P'], s['Q'], s['C']) == i and s['O'] == o:
                return base + l
    raise RuntimeError(f'ddk: no fused kernel for irreps {in_irreps} -> {out_irreps} (ns=24 with nv=6 or nv=4 are compiled in'
                       + (f'; asked for ns={ns}, nv={nv})' if nv is not None or ns != 24 else ')'))


_shape_ctx = {}


def _shape_context(device_index):
    """Context without weights: enough for ddk_tp_forward and ddk_tp_backward (shape-only layers)."""
    if device_index not in _shape_ctx:
        ctx = Context(device=device_index)
        ctx.finalize()
        _shape_ctx[device_index] = ctx
    return _shape_ctx[device_index]


def _ctx_of(t):
    """the shape context of the device of tensor ``t``"""
    return _shape_context(t.device.index or 0)


def _grad_rows(grad):
    """an incoming gradient [..., cols] as contiguous fp32 rows [E, cols]"""
    return _as_rows(grad, grad.shape[-1])


def _grads_like(grads, meta):
    """each gradient in the shape and dtype of its input (meta: their (shape, dtype)); None stays None"""
    return tuple(None if g is None else g.reshape(shape).to(dtype) for g, (shape, dtype) in zip(grads, meta))


def _as_rows(t, cols):
    """[..., cols] -> contiguous fp32 [E, cols]; the tensor itself when it already is that"""
    return t.reshape(-1, cols).contiguous().float()


class _FasterTPFunction(torch.autograd.Function):
    """ddk_tp_forward with ddk_tp_backward as its vector-Jacobian product (one launch each way).  Inputs keep their shapes and dtypes: the gradients
    come back in them."""

    @staticmethod
    def forward(fctx, in_, sh, weight, layer, weight_numel, out_size):
        ctx = _ctx_of(in_)
        x, s, w = _as_rows(in_, in_.shape[-1]), _as_rows(sh, 4), _as_rows(weight, weight_numel)
        out = ctx.tp_forward(layer, x, s, w, out_size)
        fctx.save_for_backward(x, s, w if (fctx.needs_input_grad[0] or fctx.needs_input_grad[1]) else None)      # grad_w alone does not read w
        fctx.layer, fctx.ddk = layer, ctx
        fctx.meta = [(t.shape, t.dtype) for t in (in_, sh, weight)]
        return out.reshape(in_.shape[:-1] + (out_size,))

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_out):
        x, s, w = fctx.saved_tensors
        need = tuple(fctx.needs_input_grad[:3])
        g = _grad_rows(grad_out)
        with torch.cuda.device(x.device):
            grads = fctx.ddk.tp_backward(fctx.layer, x, s, w, g, need)
        return _grads_like(grads, fctx.meta) + (None, None, None)


class FasterTensorProduct(nn.Module):
    def __init__(self, in_irreps, sh_irreps, out_irreps, **kwargs):
        super().__init__()
        if parse_irreps(sh_irreps) != {'0e': 1, '1o': 1, '1e': 0, '0o': 0}:
            raise AssertionError("sh_irreps don't look like 1st order spherical harmonics")
        self.in_irreps, self.out_irreps = str(in_irreps), str(out_irreps)
        self.layer = layer_index(in_irreps, out_irreps)
        s = tp_id_shape(self.layer)
        self.weight_shapes = dict(zip(_ORDER, zip(s['R'], s['O'])))      # (every block of these layers that has rows has columns)
        self.weight_numel, self.out_size = s['W'], s['dout']

    def forward(self, in_, sh, weight):
        if not in_.is_cuda:
            raise RuntimeError('ddk FasterTensorProduct runs on the GPU only (no CPU fallback)')
        if torch.is_grad_enabled() and (in_.requires_grad or sh.requires_grad or weight.requires_grad):
            return _FasterTPFunction.apply(in_, sh, weight, self.layer, self.weight_numel, self.out_size)
        lead = in_.shape[:-1]
        ctx = _ctx_of(in_)
        out = ctx.tp_forward(self.layer, in_.reshape(-1, in_.shape[-1]), sh.reshape(-1, 4),
                             weight.reshape(-1, self.weight_numel), self.out_size)
        return out.reshape(lead + (self.out_size,))


class FullyConnectedTensorProduct(nn.Module):
    """The holder of a conv layer's tensor product in the all-atom (confidence) model, e3nn's ``o3.FullyConnectedTensorProduct(in_irreps, '1x0e + 1x1o +
    1x2e', out_irreps, shared_weights=False)`` (all_atom_score_model.py:26), as ``FasterTensorProduct`` is for its families: ``.layer`` (``TP_AA + l``),
    ``.weight_numel`` and ``.out_size``, with the weights in e3nn's instruction order and normalisation (``runtime.tp_layer_shape_aa``).  It has no
    per-edge-weight form: ``fused_radial_tp`` / ``fused_radial_conv`` run it with the weights formed inside the kernels."""

    def __init__(self, in_irreps, sh_irreps, out_irreps, shared_weights=False, **kwargs):
        super().__init__()
        if shared_weights:
            raise RuntimeError('ddk: FullyConnectedTensorProduct takes per-edge weights from a radial MLP (shared_weights=False)')
        if not _is_second_order_sh(sh_irreps):
            raise RuntimeError(f'ddk: FullyConnectedTensorProduct is the all-atom family\'s, sh_irreps {SH_SECOND_ORDER}; got {sh_irreps} (the score heads are fused_head_conv)')
        self.in_irreps, self.sh_irreps, self.out_irreps = str(in_irreps), str(sh_irreps), str(out_irreps)
        self.layer = layer_index(in_irreps, out_irreps, sh_irreps=sh_irreps)
        s = tp_id_shape(self.layer)
        self.weight_numel, self.out_size = s['W'], s['dout']

    def forward(self, in_, sh, weight):
        raise RuntimeError(f'ddk: the all-atom family has no per-edge weight form [E, {self.weight_numel}]: use fused_radial_tp or fused_radial_conv, which form '
                           'the weights inside the kernels')


def sh_second_order(sh4):
    """The sh rows [E, 9] = [Y0 | Y1 | Y2] of the all-atom family (e3nn's component order and 'component' normalisation, normalize=True) from
    ``fused_edge_embedding``'s rows [E, 4] = [1 | sqrt3 u]: Y2 is a polynomial of the unit vector u that Y1 carries.  A zero-length edge (Y1 = 0: a C-alpha
    atom and its own residue) gives Y2 = 0, as e3nn does.  Plain torch, no gradient."""
    with torch.no_grad():
        sh4 = sh4.detach().float()
        x, y, z = (sh4[:, 1:4] * (3 ** -0.5)).unbind(-1)
        s15 = 15 ** 0.5
        y2 = torch.stack([s15 * x * z, s15 * x * y, (5 ** 0.5) * (y * y - 0.5 * (x * x + z * z)), s15 * y * z, (0.5 * s15) * (z * z - x * x)], -1)
        return torch.cat([sh4, y2], -1).contiguous()


def _fc_parts(blk):
    """(first Linear, ReLU, Dropout, last Linear) of a radial MLP: an FCBlock (Linear, Identity, ReLU, Dropout, Linear: keys 0 and 4) or the all-atom
    layer's ``Sequential(Linear, ReLU, Dropout, Linear)`` (keys 0 and 3); None for anything else"""
    if not isinstance(blk, nn.Sequential) or len(blk) not in (4, 5):
        return None
    parts = (blk[0], blk[-3], blk[-2], blk[-1])
    return parts if all(isinstance(m, t) for m, t in zip(parts, (nn.Linear, nn.ReLU, nn.Dropout, nn.Linear))) else None


class _RadialTPFunction(torch.autograd.Function):
    """ddk_rtp_forward with ddk_rtp_backward as its vector-Jacobian product: the tensor product with its weights w2[g] h + b2[g] formed inside the
    kernels, so that neither the per-edge weights [E, W] nor their gradient exist.  Inputs keep their shapes and dtypes: the gradients come back in them."""

    @staticmethod
    def forward(fctx, in_, sh, h, w2, b2, layer, offsets, out_size):
        ctx = _ctx_of(in_)
        x, s, hh = _as_rows(in_, in_.shape[-1]), _as_rows(sh, sh.shape[-1]), _as_rows(h, h.shape[-1])
        w, b = w2.contiguous().float(), b2.contiguous().float()
        out = ctx.rtp_forward(layer, x, s, hh, offsets, w, b, out_size)
        ng = fctx.needs_input_grad
        fctx.save_for_backward(x, s, hh, w if any(ng[:3]) else None, b if any(ng[:2]) else None)      # the parameter gradients read neither
        fctx.layer, fctx.ddk, fctx.offsets = layer, ctx, tuple(offsets)
        fctx.meta = [(t.shape, t.dtype) for t in (in_, sh, h, w2, b2)]
        return out.reshape(in_.shape[:-1] + (out_size,))

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_out):
        x, s, hh, w, b = fctx.saved_tensors
        need = tuple(fctx.needs_input_grad[:5])
        g = _grad_rows(grad_out)
        with torch.cuda.device(x.device):
            grads = fctx.ddk.rtp_backward(fctx.layer, x, s, hh, fctx.offsets, w, b, g, need)
        return _grads_like(grads, fctx.meta) + (None, None, None)


def _radial_operands(who, tp, fc, x, edge_attr, hidden=None):
    """What fused_radial_tp and fused_radial_conv share: the checks on ``tp`` and ``fc``, then ``fc[i][0..3]`` in torch.  Returns the group offsets, the
    hidden activation [E, 72] and the last Linears stacked, w2 [G, W, 72] and b2 [G, W].  With ``hidden`` given (fused_radial_hidden's output)
    ``fc[i][0..3]`` do not run, and ``edge_attr`` gives the groups alone: G + 1 integer offsets, or one tensor per group whose rows are counted."""
    if not isinstance(tp, (FasterTensorProduct, FullyConnectedTensorProduct)):
        raise RuntimeError(f'ddk: {who} takes a FasterTensorProduct (or the all-atom family\'s FullyConnectedTensorProduct)')
    if not x.is_cuda:
        raise RuntimeError(f'ddk {who} runs on the GPU only (no CPU fallback)')
    if hidden is not None and not torch.is_tensor(edge_attr) and len(edge_attr) and not torch.is_tensor(edge_attr[0]):
        offs = [int(o) for o in edge_attr]
        fc = [fc] if isinstance(fc, nn.Sequential) else list(fc)
        if len(offs) != len(fc) + 1 or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])):
            raise RuntimeError(f'ddk: {who} with hidden= takes G + 1 ascending group offsets that start at 0, G the number of FCBlocks')
        edge_attr = None
    else:
        if isinstance(fc, nn.Sequential):
            fc, edge_attr = [fc], ([edge_attr] if torch.is_tensor(edge_attr) else list(edge_attr))
        fc, edge_attr = list(fc), list(edge_attr)
        if len(fc) != len(edge_attr):
            raise RuntimeError(f'ddk: {who} takes one edge_attr tensor per FCBlock, 1..4 of them')
        offs = [0]
        for ea in edge_attr:
            offs.append(offs[-1] + ea.shape[0])
    if not 1 <= len(fc) <= 4:
        raise RuntimeError(f'ddk: {who} takes one edge_attr tensor per FCBlock, 1..4 of them')
    for blk in fc:      # an FCBlock, or the all-atom layer's Sequential(Linear, ReLU, Dropout, Linear): the last module is the Linear the kernels run
        if len(blk) not in (4, 5) or not isinstance(blk[-1], nn.Linear) or blk[-1].in_features != 72 or blk[-1].out_features != tp.weight_numel or blk[-1].bias is None:
            raise RuntimeError(f'ddk: {who} takes 2-layer FCBlocks whose last Linear maps 72 -> weight_numel')
    if hidden is not None:
        if hidden.dim() != 2 or hidden.shape != (offs[-1], 72):
            raise RuntimeError(f'ddk: {who} takes hidden [E, 72] with E = {offs[-1]}, the total of the edge groups; got {tuple(hidden.shape)}')
    else:
        hidden = torch.cat([blk[:-1](ea) for blk, ea in zip(fc, edge_attr)], dim=0) if len(fc) > 1 else fc[0][:-1](edge_attr[0])
    w2, b2 = torch.stack([blk[-1].weight for blk in fc]), torch.stack([blk[-1].bias for blk in fc])
    return offs, hidden, w2, b2


def fused_radial_tp(tp, fc, x_dst, edge_sh, edge_attr):
    """``tp(x_dst, edge_sh, torch.cat([fc[i](edge_attr[i]) for i in range(G)]))`` of the reference's TensorProductConvLayer.forward
    (models/tensor_layers.py:154-156) without the per-edge weights: ``fc[i][0..3]`` run in torch, the last Linear of every group runs inside the tensor
    product's kernels, forward and backward.  ``tp``: a FasterTensorProduct; ``fc``: the layer's ModuleList of FCBlocks, or one FCBlock (edge_groups == 1);
    ``edge_attr``: the per-group list (a tensor for one FCBlock).  Every parameter of ``fc``, ``x_dst``, ``edge_sh`` and ``edge_attr`` receive the gradients
    the unfused composition gives them."""
    offs, hidden, w2, b2 = _radial_operands('fused_radial_tp', tp, fc, x_dst, edge_attr)
    if x_dst.dim() != 2 or x_dst.shape[0] != offs[-1]:
        raise RuntimeError('ddk: fused_radial_tp takes x_dst [E, Din] with E the total of the edge groups')
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x_dst, edge_sh, hidden, w2, b2)):
        return _RadialTPFunction.apply(x_dst, edge_sh, hidden, w2, b2, tp.layer, tuple(offs), tp.out_size)
    ctx = _ctx_of(x_dst)
    return ctx.rtp_forward(tp.layer, x_dst, edge_sh.reshape(-1, edge_sh.shape[-1]), hidden, offs, w2, b2, tp.out_size)


class _RadialConvFunction(torch.autograd.Function):
    """ddk_rconv_forward with ddk_rconv_backward as its vector-Jacobian product: node features to aggregated node features.  Saved for the backward: the
    node table, sh, h, the graph, and w2 / b2 where a requested gradient reads them; never the gathered rows [E, Din], the tensor product's rows [E, Dout]
    or the per-edge weights.  No atomics: the gradients have the same bits on every run."""

    @staticmethod
    def forward(fctx, node_attr, sh, h, w2, b2, layer, offsets, graph):
        ctx = _ctx_of(node_attr)
        x, s, hh = _as_rows(node_attr, node_attr.shape[-1]), _as_rows(sh, sh.shape[-1]), _as_rows(h, h.shape[-1])
        w, b = w2.contiguous().float(), b2.contiguous().float()
        out = ctx.rconv_forward(layer, graph, x, s, hh, offsets, w, b)
        ng = fctx.needs_input_grad
        fctx.save_for_backward(x, s, hh, w if any(ng[:3]) else None, b if any(ng[:2]) else None)      # the parameter gradients read neither
        fctx.layer, fctx.ddk, fctx.offsets, fctx.graph = layer, ctx, tuple(offsets), graph
        fctx.meta = [(t.shape, t.dtype) for t in (node_attr, sh, h, w2, b2)]
        return out

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_out):
        x, s, hh, w, b = fctx.saved_tensors
        need = tuple(fctx.needs_input_grad[:5])
        g = _grad_rows(grad_out)
        with torch.cuda.device(x.device):
            grads = fctx.ddk.rconv_backward(fctx.layer, fctx.graph, x, s, hh, fctx.offsets, w, b, g, need)
        return _grads_like(grads, fctx.meta) + (None, None, None)


def fused_radial_conv(tp, fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes=None, graph=None, hidden=None):
    """Lines 153-159 of the reference's TensorProductConvLayer.forward with reduce='mean' (models/tensor_layers.py) as one differentiable op:
    ``scatter(tp(node_attr[edge_dst], edge_sh, torch.cat([fc[i](edge_attr[i]) ...])), edge_src, dim_size=out_nodes, reduce='mean')``.  ``fc[i][0..3]``
    (Dropout included) run in torch; the last Linear, the gather, the tensor product and the mean run in the kernels of the radial tensor product and a
    fixed-order segmented sum, forward and backward: no [E, W] weights, no gathered rows, no atomics, so the gradients of ``node_attr``, ``edge_sh``,
    ``edge_attr`` and every parameter of ``fc`` have the same bits on every run.  ``graph``: a ``runtime.ConvGraph`` made once for this
    ``edge_index`` (``Context.conv_graph(edge_index[0], edge_index[1], n_in=node_attr.shape[0], n_out=out_nodes)``); built here otherwise, which
    costs two sorts and one read-back per call.  ``hidden``: the hidden activation [E, 72] made elsewhere (``fused_radial_hidden``); ``fc[i][0..3]`` are
    skipped then, and ``edge_attr`` only names the groups: G + 1 integer offsets, or per-group tensors whose rows are counted.  [out_nodes or N, Dout], fp32."""
    offs, hidden, w2, b2 = _radial_operands('fused_radial_conv', tp, fc, node_attr, edge_attr, hidden)
    if node_attr.dim() != 2:
        raise RuntimeError('ddk: fused_radial_conv takes node_attr [N, Din]')
    n_out = out_nodes or node_attr.shape[0]
    if graph is None:
        graph = Context.conv_graph(edge_index[0], edge_index[1], node_attr.shape[0], n_out)
    if graph.n_in != node_attr.shape[0] or graph.n_out != n_out or graph.E != offs[-1]:
        raise RuntimeError(f'ddk: fused_radial_conv: the graph ({graph.n_in} -> {graph.n_out} nodes, {graph.E} edges) does not fit '
                           f'{node_attr.shape[0]} -> {n_out} nodes and {offs[-1]} edges in the groups')
    if torch.is_grad_enabled() and any(t.requires_grad for t in (node_attr, edge_sh, hidden, w2, b2)):
        return _RadialConvFunction.apply(node_attr, edge_sh, hidden, w2, b2, tp.layer, tuple(offs), graph)
    ctx = _ctx_of(node_attr)
    return ctx.rconv_forward(tp.layer, graph, node_attr, edge_sh.reshape(-1, edge_sh.shape[-1]), hidden, offs, w2, b2)


class _RadialHiddenFunction(torch.autograd.Function):
    """ddk_rhid_forward with ddk_rhid_backward as its vector-Jacobian product: the hidden activation of the radial MLP from the node scalars and the
    edge embedding.  Saved for the backward: xs [N, 24], emb [E, 24], h [E, 72] (the output, which carries the ReLU and Dropout pattern), the graph, and
    w1 where an input gradient reads it; never the concatenated row, the ReLU output or a mask.  No atomics: the same gradient bits on every run."""

    @staticmethod
    def forward(fctx, xs, emb, w1, b1, offsets, graph, p, seed):
        ctx = _ctx_of(xs)
        x, e = _as_rows(xs, 24), _as_rows(emb, 24)
        w, b = w1.contiguous().float(), b1.contiguous().float()
        h = ctx.rhid_forward(graph, x, e, offsets, w, b, p, seed)
        fctx.save_for_backward(x, e, h, w if any(fctx.needs_input_grad[:2]) else None)      # the parameter gradients do not read w1
        fctx.ddk, fctx.offsets, fctx.graph, fctx.p = ctx, tuple(offsets), graph, p
        fctx.meta = [(t.shape, t.dtype) for t in (xs, emb, w1, b1)]
        return h

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_h):
        x, e, h, w = fctx.saved_tensors
        need = tuple(fctx.needs_input_grad[:4])
        g = grad_h.reshape(-1, 72).contiguous().float()
        with torch.cuda.device(x.device):
            grads = fctx.ddk.rhid_backward(fctx.graph, x, e, h, fctx.offsets, w, g, fctx.p, need)
        return _grads_like(grads, fctx.meta) + (None, None, None, None)


def _draw_seed():
    """one 63-bit draw from torch's default CPU generator: torch.manual_seed reproduces it, and nothing waits for the device"""
    return int(torch.randint(0, (1 << 63) - 1, (1,), dtype=torch.int64).item())


def fused_radial_hidden(fc, node_attr, edge_emb, group_offsets, graph, seed=None):
    """``torch.cat([fc[g][:4](edge_attr_[g]) for g in range(G)])`` with ``edge_attr_ = torch.cat([edge_emb, node_attr[edge_index[0], :ns],
    node_attr[edge_index[1], :ns]], -1)`` cut into the groups (the reference's embed loop, models/score_model.py:227-230, and the first half of the
    conv layer's radial MLP) as one differentiable op: the hidden activation [E, 72] of all groups.  The gathers, the Linear, the ReLU and the Dropout
    run in one kernel; the backward adds the gathers' gradients per node in a fixed order (no atomics), so ``node_attr``, ``edge_emb`` and every
    ``fc[g][0]`` parameter get the same gradient bits on every run.  ``fc``: the layer's FCBlocks (or one); ``group_offsets``: G + 1 integers;
    ``graph``: the ``ConvGraph`` of ``edge_index`` over ``node_attr``'s rows.  Dropout: rate ``fc[g][3].p`` while that module is in training mode (the
    same in every group), else none; the mask is a pure function of (``seed``, edge, column), DDK_RHID_MASK_LAYOUT of include/ddk.h.  ``seed=None``
    takes one draw from torch's default CPU generator, so ``torch.manual_seed`` reproduces a step."""
    fc = [fc] if isinstance(fc, nn.Sequential) else list(fc)
    offs = [int(o) for o in group_offsets]
    if not 1 <= len(fc) <= 4 or len(offs) != len(fc) + 1:
        raise RuntimeError('ddk: fused_radial_hidden takes 1..4 FCBlocks and one more group offset than blocks')
    for blk in fc:
        parts = _fc_parts(blk)
        if (parts is None or parts[3].in_features != 72 or parts[3].bias is None or parts[0].in_features != 72 or parts[0].out_features != 72
                or parts[0].bias is None):
            raise RuntimeError('ddk: fused_radial_hidden takes 2-layer FCBlocks: Linear(72, 72) with bias, Identity, ReLU, Dropout, Linear(72, .) '
                               '(or the all-atom layer\'s Sequential without the Identity)')
    rates = {float(_fc_parts(blk)[2].p) if _fc_parts(blk)[2].training else 0.0 for blk in fc}
    if len(rates) != 1:
        raise RuntimeError(f'ddk: fused_radial_hidden takes one dropout rate for all groups; got {sorted(rates)}')
    p = rates.pop()
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f'ddk: fused_radial_hidden takes a dropout rate in [0, 1); got {p}')
    if not node_attr.is_cuda:
        raise RuntimeError('ddk fused_radial_hidden runs on the GPU only (no CPU fallback)')
    if node_attr.dim() != 2 or node_attr.shape[1] < 24 or edge_emb.dim() != 2 or edge_emb.shape[1] != 24:
        raise RuntimeError('ddk: fused_radial_hidden takes node_attr [N, >= 24] and edge_emb [E, 24]')
    if seed is None:
        seed = _draw_seed() if p > 0 else 0
    xs = node_attr[:, :24]      # (torch's slice: its backward pads the gradient back to the node row)
    w1, b1 = torch.stack([blk[0].weight for blk in fc]), torch.stack([blk[0].bias for blk in fc])
    if torch.is_grad_enabled() and any(t.requires_grad for t in (xs, edge_emb, w1, b1)):
        return _RadialHiddenFunction.apply(xs, edge_emb, w1, b1, tuple(offs), graph, p, int(seed))
    return _ctx_of(node_attr).rhid_forward(graph, xs, edge_emb, offs, w1, b1, p, int(seed))


def _layer_seed(seed, l):
    """the seed of layer ``l`` of a stack: the stack's seed moved by the layer's multiple of the 64-bit golden ratio (distinct Philox keys)"""
    return (int(seed) + (l + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def conv_stack(conv_layers, node_attr, edge_index, edge_emb, group_sizes, edge_sh, seed=None):
    """The conv loop of the reference's embed (models/score_model.py:227-230) over ``conv_layers``: every layer sees
    ``[edge_emb | node_attr[edge_index[0], :ns] | node_attr[edge_index[1], :ns]]`` of the current node features, cut into groups of ``group_sizes`` edges.
    One ``ConvGraph`` is built for all layers; layer l's dropout seed is derived from ``seed`` (``None``: one draw from torch's default CPU generator).
    In training the whole stack runs without atomics: two passes from one state and one seed give the same bits.  Returns ``node_attr``."""
    layers = list(conv_layers)
    graph = None
    if any(layer.training or getattr(layer, 'layer', 0) >= TP_NV4 or getattr(layer, 'eval_with_training_ops', False) for layer in layers) and edge_index.shape[1] > 0:      # (an nv = 4 layer evaluates with the training ops)
        graph = Context.conv_graph(edge_index[0], edge_index[1], node_attr.shape[0], node_attr.shape[0])
        if seed is None and any(layer.training for layer in layers):
            seed = _draw_seed()
    for l, layer in enumerate(layers):
        node_attr = layer.forward_embedded(node_attr, edge_index, edge_emb, group_sizes, edge_sh, graph=graph,
                                           seed=None if seed is None else _layer_seed(seed, l))
    return node_attr


def _edge_embedding_forward(scalars, w1, b1, w2, b2, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, *lat):
    """(emb, sh) of one edge group from the device op, without autograd.  ``scalars``: (start, stop, p, seed, zero_latent, graph); ``lat``: nothing for
    the plain op (ddk_eemb_forward), (uemb, lat_a, lat_b, unc_a) for the latent one (ddk_eemb_latent_forward)"""
    start, stop, p, seed, zero_latent, _ = scalars
    ctx, ops = _ctx_of(pos_a), (pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2)
    if lat:
        uemb, lat_a, lat_b, unc_a = lat
        return ctx.eemb_latent_forward(*ops, lat_a, lat_b, zero_latent, unc_a, uemb, p, seed)
    return ctx.eemb_forward(*ops, p, seed)


class _EdgeEmbeddingFunction(torch.autograd.Function):
    """``_edge_embedding_forward`` with ddk_eemb_backward / ddk_eemb_latent_backward as its vector-Jacobian product: one edge group's embedding [E, 24]
    and spherical harmonics [E, 4] from the coordinates.  Saved for the backward: the operands it was given (positions, index tensors, bond features,
    the sigma table, the parameters without b2; the latent op's four tensors behind them, its node-sorted edge lists in ``scalars``); nothing per edge
    that the op made itself.  The plain op has no latent inputs: it takes and saves no more than it did.  The backward recomputes the hidden layer and
    the mask from the seed.  Gradients: the four parameters, and for the latent op ``uemb`` and the two latent tables (where both are one tensor the
    caller adds the two), all without atomics: the same bits on every run."""

    @staticmethod
    def forward(fctx, scalars, w1, b1, w2, b2, *rest):      # rest: the seven geometry operands, then ``lat``
        emb, sh = _edge_embedding_forward(scalars, w1, b1, w2, b2, *rest)
        fctx.save_for_backward(w1, b1, w2, *rest)      # (b2 is not read by the backward)
        fctx.ddk, fctx.scalars = _ctx_of(rest[0]), scalars
        fctx.meta = [None if t is None else (t.shape, t.dtype) for t in (w1, b1, w2, b2, *rest[7:10])]
        fctx.mark_non_differentiable(sh)
        return emb, sh

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_emb, _grad_sh):
        w1, b1, w2, *rest = fctx.saved_tensors
        start, stop, p, seed, zero_latent, graph = fctx.scalars
        ops, lat, need = (*rest[:7], start, stop, w1, b1, w2), rest[7:], fctx.needs_input_grad
        with torch.cuda.device(rest[0].device):
            if lat:
                uemb, lat_a, lat_b, unc_a = lat
                grads = fctx.ddk.eemb_latent_backward(*ops, lat_a, lat_b, grad_emb, zero_latent, unc_a, uemb, p, seed, graph, need[1:5] + need[12:15])
            else:
                grads = fctx.ddk.eemb_backward(*ops, grad_emb, p, seed, need[1:5])
        out = tuple(None if (g is None or m is None) else g.reshape(m[0]).to(m[1]) for g, m in zip(grads, fctx.meta))
        return (None,) + out[:4] + (None,) * 7 + out[4:] + ((None,) if lat else ())


def _smearing_range(expansion):
    """(start, stop) of a GaussianSmearing of 32 Gaussians whose ``offset`` and ``coeff`` are what the kernels restate from them (include/ddk.h); read
    back once per buffer and kept on the module"""
    off = expansion.offset
    key = (off.data_ptr(), off._version, str(off.device))
    cached = getattr(expansion, '_ddk_range', None)
    if cached is None or cached[0] != key:
        host = off.detach().float().cpu()
        if host.shape != (32,):
            raise RuntimeError(f'ddk: fused_edge_embedding takes a distance expansion of 32 Gaussians; got {tuple(host.shape)}')
        start, stop = float(host[0]), float(host[-1])
        if not start < stop or not torch.allclose(host, torch.linspace(start, stop, 32), rtol=0, atol=4e-7 * max(abs(start), abs(stop))):
            raise RuntimeError('ddk: fused_edge_embedding takes a distance expansion whose offset is torch.linspace(start, stop, 32)')
        coeff = -0.5 / float(host[1] - host[0]) ** 2
        if abs(float(expansion.coeff) - coeff) > 1e-5 * abs(coeff):
            raise RuntimeError(f'ddk: fused_edge_embedding takes a distance expansion with coeff = -0.5 / (offset[1] - offset[0])^2 = {coeff}; got {expansion.coeff}')
        cached = (key, (start, stop))
        expansion._ddk_range = cached
    return cached[1]


def fused_edge_embedding(mlp, expansion, pos_a, pos_b, edge_index, sig, sig_index, feat=None, seed=None, latent_a=None, latent_b=None, zero_latent=False,
                         unconditional=None, unconditional_embedding=None, graph=None):
    """One edge group of the reference's embed in front of the conv stack (models/score_model.py:191-225) as one differentiable op:
    ``edge_emb = mlp(torch.cat([feat, sig[sig_index[edge_index[0]]], expansion(|vec|)], 1))`` and ``edge_sh`` = the first-order spherical harmonics of
    ``vec = pos_b[edge_index[1]] - pos_a[edge_index[0]]`` (component normalisation: ``[1 | sqrt3 vec / |vec|]``).  ``mlp``: the reference's
    ``nn.Sequential(Linear(K, 24), ReLU, Dropout, Linear(24, 24))``, K = 64, or 68 with ``feat`` [E, 4]; ``expansion``: a ``GaussianSmearing`` of 32
    Gaussians; ``sig`` [T, 32]: the sigma embedding per graph, ``sig_index`` [Na] the graph of a node of ``pos_a``; ``sig=None, sig_index=None``: a row without the
    sigma block (K = 32, or 36 with ``feat``: the latent encoder's), run by the same kernels on ``W1`` padded with 32 zero columns.  The positions carry no gradient in
    score matching: one that requires it raises.  Nothing wider than the outputs is stored per edge, forward or backward; the four parameters of ``mlp``
    get the same gradient bits on every run (no atomics).  Dropout: rate ``mlp[2].p`` while that module is in training mode, else none; the mask is a
    pure function of (``seed``, edge position, column), DDK_EEMB_MASK_LAYOUT of include/ddk.h; ``seed=None`` takes one draw from torch's default CPU
    generator.  Returns (edge_emb [E, 24], edge_sh [E, 4]), fp32.

    The latent-conditioned (DisCo) model: ``latent_a`` [Na, L] and ``latent_b`` [Nb, L], 1 <= L <= 4, append ``[latent_a[edge_index[0]] |
    latent_b[edge_index[1]]]`` to the row (the first Linear then takes K + 2 L columns); they may be one tensor and may require grad: their gradient is a
    fixed-order sum over a node's edges (no atomics), the source sum + the destination sum where both are one tensor.  ``zero_latent=True`` (the cross
    group, models/score_model.py:401) appends 2 L zero columns instead; it takes ``latent_a`` for L alone (or an int).  ``unconditional`` [Na] (no
    gradient) with ``unconditional_embedding`` [1, 24] or [24] (a parameter) adds ``unconditional[edge_index[0]][:, None] * unconditional_embedding``.
    ``graph``: ``Context.conv_graph(edge_index[0], edge_index[1], Nb, Na)`` where the caller has it (built here otherwise, when a latent needs its
    gradient).  With none of these given the call is the plain op's, call for call."""
    if (not isinstance(mlp, nn.Sequential) or len(mlp) != 4 or not isinstance(mlp[0], nn.Linear) or not isinstance(mlp[1], nn.ReLU)
            or not isinstance(mlp[2], nn.Dropout) or not isinstance(mlp[3], nn.Linear) or mlp[0].bias is None or mlp[3].bias is None
            or mlp[0].out_features != 24 or (mlp[3].in_features, mlp[3].out_features) != (24, 24)):
        raise RuntimeError('ddk: fused_edge_embedding takes nn.Sequential(Linear(K, 24), ReLU, Dropout, Linear(24, 24)) with biases')
    F_ = 0 if feat is None else 4
    K = F_ + (32 if sig is not None else 0) + 32
    latent = latent_a is not None or latent_b is not None or zero_latent or unconditional is not None or unconditional_embedding is not None
    L = 0
    if latent:
        if zero_latent:
            L = int(latent_a) if isinstance(latent_a, int) else (latent_a.shape[1] if torch.is_tensor(latent_a) else (mlp[0].in_features - K) // 2)
            latent_a = latent_b = None
        else:
            if not torch.is_tensor(latent_a) or not torch.is_tensor(latent_b) or latent_a.dim() != 2 or latent_b.dim() != 2 or latent_a.shape[1] != latent_b.shape[1]:
                raise RuntimeError('ddk: fused_edge_embedding takes latent_a [Na, L] and latent_b [Nb, L] together (or zero_latent)')
            L = latent_a.shape[1]
        if not 1 <= L <= 4:
            raise RuntimeError(f'ddk: fused_edge_embedding takes 1..4 latent columns per node; got {L}')
        if (unconditional is None) != (unconditional_embedding is None):
            raise RuntimeError('ddk: fused_edge_embedding takes unconditional and unconditional_embedding together')
        if unconditional is not None and unconditional.requires_grad:
            raise RuntimeError('ddk: fused_edge_embedding has no gradient for unconditional (a mask of graphs); detach it')
    if mlp[0].in_features != K + 2 * L:
        raise RuntimeError(f'ddk: fused_edge_embedding: the first Linear takes {mlp[0].in_features} columns, the row has {K + 2 * L} (4 bond features with feat, 32 + 32 (32 with sig=None)'
                           + (f', 2 x {L} latent columns)' if L else ')'))
    if not pos_a.is_cuda:
        raise RuntimeError('ddk fused_edge_embedding runs on the GPU only (no CPU fallback)')
    if pos_a.requires_grad or pos_b.requires_grad:
        raise RuntimeError('ddk: fused_edge_embedding has no gradient for the positions (they carry none in score matching); detach them')
    w1 = mlp[0].weight
    if sig is None:
        # no sigma block (the latent encoder): 32 zero columns where the kernel reads it, a one-row zero table that every node points at.  The zero columns
        # add exact zeros to each fmaf chain, and the cat's backward drops their gradient
        if sig_index is not None:
            raise RuntimeError('ddk: fused_edge_embedding takes sig and sig_index together (both None: a row without a sigma block)')
        w1 = torch.cat([w1[:, :F_], w1.new_zeros((w1.shape[0], 32)), w1[:, F_:]], 1)
        sig = torch.zeros((1, 32), dtype=torch.float32, device=pos_a.device)
        sig_index = torch.zeros(pos_a.shape[0], dtype=torch.int32, device=pos_a.device)
    if sig.requires_grad or (feat is not None and feat.requires_grad):
        raise RuntimeError('ddk: fused_edge_embedding has no gradient for sig or feat (times and bond types carry none); detach them')
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise RuntimeError(f'ddk: fused_edge_embedding takes edge_index [2, E]; got {tuple(edge_index.shape)}')
    p = float(mlp[2].p) if mlp[2].training else 0.0
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f'ddk: fused_edge_embedding takes a dropout rate in [0, 1); got {p}')
    if seed is None:
        seed = _draw_seed() if p > 0 else 0
    start, stop = _smearing_range(expansion)
    idx_a, idx_b = edge_index[0].to(torch.int32).contiguous(), edge_index[1].to(torch.int32).contiguous()
    operands = (pos_a.detach().float().contiguous(), pos_b.detach().float().contiguous(), idx_a, idx_b, None if feat is None else feat.float().contiguous(),
                sig.float().contiguous(), sig_index.to(torch.int32).contiguous())
    b1, w2, b2 = mlp[0].bias, mlp[3].weight, mlp[3].bias
    lat = ()      # (latent_a and latent_b may be one tensor: autograd adds the source sum and the destination sum, a commutative fp32 add)
    if latent:
        lat = (None if unconditional_embedding is None else unconditional_embedding.reshape(-1), latent_a, latent_b,
               None if unconditional is None else unconditional.detach().float().reshape(-1).contiguous())
    differentiable = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (w1, b1, w2, b2, *lat[:3]))
    if differentiable and latent and graph is None and latent_a is not None and (latent_a.requires_grad or latent_b.requires_grad) and idx_a.shape[0] > 0:
        graph = Context.conv_graph(idx_a, idx_b, pos_b.shape[0], pos_a.shape[0])
    args = ((start, stop, p, int(seed), bool(zero_latent), graph if latent else None), w1, b1, w2, b2, *operands, *lat)
    return _EdgeEmbeddingFunction.apply(*args) if differentiable else _edge_embedding_forward(*args)


class _RaggedGumbelFunction(torch.autograd.Function):
    """ddk_gumbel_softmax_batch with ddk_gumbel_softmax_batch_backward as its vector-Jacobian product; saved: the soft y of both sides and the two pointer
    tables.  No atomics: the same bits on every run."""

    @staticmethod
    def forward(fctx, logit_l, logit_r, lig_ptr, rec_ptr, T, seed, stream_ids, sample, draw):
        ctx = _ctx_of(logit_l)
        out_l, out_r, y_l, y_r = ctx.gumbel_softmax(logit_l, logit_r, lig_ptr, rec_ptr, T, seed, stream_ids, sample, draw)
        fctx.save_for_backward(y_l, y_r, lig_ptr, rec_ptr)
        fctx.ddk, fctx.T = ctx, T
        fctx.meta = [(t.shape, t.dtype) for t in (logit_l, logit_r)]
        return out_l, out_r

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_l, grad_r):
        y_l, y_r, lig_ptr, rec_ptr = fctx.saved_tensors
        with torch.cuda.device(y_l.device):
            grads = fctx.ddk.gumbel_softmax_backward(y_l, y_r, lig_ptr, rec_ptr, fctx.T, grad_l, grad_r)
        return _grads_like(grads, fctx.meta) + (None,) * 7


def _graph_ptrs(batches, G):
    """the [G + 1] int64 prefixes of node-to-graph vectors whose nodes are grouped by graph in ascending order, and ONE read-back for all of them: per
    vector (the largest descent between neighbours, the first entry, the last entry), as ``Context.conv_graph`` reads the extremes of its indices"""
    ptrs, probes = [], []
    for batch in batches:
        batch = batch.long()
        ptr = torch.zeros(G + 1, dtype=torch.int64, device=batch.device)
        if batch.numel():
            ptr[1:] = torch.cumsum(torch.bincount(batch.clamp(0, max(G - 1, 0)), minlength=G)[:G], 0)
            descent = (batch[:-1] - batch[1:]).max() if batch.numel() > 1 else torch.zeros((), dtype=torch.int64, device=batch.device)
            probes.append(torch.stack([descent, batch[0], batch[-1]]))
        else:
            probes.append(torch.zeros(3, dtype=torch.int64, device=batch.device))
        ptrs.append(ptr)
    return ptrs, torch.stack(probes).tolist()


def ragged_gumbel_softmax(logit_l, logit_r, lig_batch, rec_batch, temperature, seed, stream_ids, sample=0, draw=0):
    """The reference's per-graph straight-through Gumbel softmax over a graph's ligand and receptor nodes (latent_encoder.py:328-335,
    pretrained_score_encoder.py:74-81 over models/layers.py:152-181: ``gumbel_softmax(cat([logit_l[lig_batch == g], logit_r[rec_batch == g]]).T, hard=True)``)
    for the whole collated batch in one launch and with one read-back (the check of the two batch vectors), none per graph: ``logit_l`` [N_lig, D], ``logit_r`` [N_rec, D], D <= 4, ->
    (latent_l [N_lig, D], latent_r [N_rec, D]): per graph and latent dimension a one-hot over the graph's nodes that carries the soft sample's gradient.
    ``lig_batch`` / ``rec_batch``: the graph of a node, sorted; ``stream_ids`` [G]: ``runtime.stream_id`` of each graph's complex.  The noise is a pure
    function of (``seed``, complex, ``sample``, ``draw``, d, node position), DDK_GUMBEL_LAYOUT of include/ddk.h: a graph draws the same noise in any
    batch.  Differentiable in both logit tables, without atomics: the same bits on every run."""
    if not logit_l.is_cuda:
        raise RuntimeError('ddk ragged_gumbel_softmax runs on the GPU only (no CPU fallback)')
    G = len(stream_ids)
    if lig_batch.shape[0] != logit_l.shape[0] or rec_batch.shape[0] != logit_r.shape[0]:
        raise RuntimeError('ddk: ragged_gumbel_softmax takes one batch entry per row of its logit tables')
    (lig_ptr, rec_ptr), probes = _graph_ptrs((lig_batch.to(logit_l.device), rec_batch.to(logit_l.device)), G)      # the call's one read-back
    for what, (descent, first, last) in zip(('lig_batch', 'rec_batch'), probes):
        if descent > 0 or first < 0 or last >= G:
            raise RuntimeError(f'ddk: ragged_gumbel_softmax takes {what} sorted by graph with entries in [0, {G})')
    if not torch.is_tensor(stream_ids):
        stream_ids = torch.from_numpy(np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids], dtype=np.uint64).view(np.int64)).to(logit_l.device)
    args = (logit_l, logit_r, lig_ptr, rec_ptr, float(temperature), int(seed), stream_ids, int(sample), int(draw))
    if torch.is_grad_enabled() and (logit_l.requires_grad or logit_r.requires_grad):
        return _RaggedGumbelFunction.apply(*args)
    return _ctx_of(logit_l).gumbel_softmax(*args)[:2]


class _RaggedNodeCrossEntropyFunction(torch.autograd.Function):
    """ddk_node_cross_entropy_batch with ddk_node_cross_entropy_batch_backward as its vector-Jacobian product, for the two logit tables only; saved: the
    operands and per GRAPH the two log-sum-exps and the target.  No atomics: the same bits on every run."""

    @staticmethod
    def forward(fctx, logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft):
        ctx = _ctx_of(logit_l)
        loss, pick, target, saved = ctx.node_cross_entropy(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft)
        fctx.save_for_backward(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, target, saved)
        fctx.ddk, fctx.soft = ctx, soft
        fctx.mark_non_differentiable(pick, target)
        return loss, pick, target

    @staticmethod
    @once_differentiable
    def backward(fctx, grad, _pick, _target):
        logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, target, saved = fctx.saved_tensors
        with torch.cuda.device(logit_l.device):
            g_l, g_r = fctx.ddk.node_cross_entropy_backward(grad, logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, target, saved, fctx.soft)
        need = fctx.needs_input_grad
        return (g_l if need[0] else None, g_r if need[1] else None) + (None,) * 6


def ragged_node_cross_entropy(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft=False):
    """The AR model's loss: per graph, the cross-entropy of the student's logits over the graph's ligand nodes followed by its receptor nodes against
    column ``column[g]`` of the teacher's tables, the reference's loop of one ``F.cross_entropy`` per graph (autoregressive/train_ar.py:116-127, 152-177)
    in one launch and without a read-back.  ``logit_l`` [N_lig] or [N_lig, 1], ``logit_r`` [N_rec] or [N_rec, 1] (float32, contiguous); ``lig_ptr`` /
    ``rec_ptr``: int64 [G + 1] prefixes of the graphs' rows; ``teacher_l`` [N_lig, D], ``teacher_r`` [N_rec, D], D in 1..4; ``column``: int32 [G];
    all on one device.  ``soft=False``: the label is the teacher column's argmax (the sampled one-hot labels); ``soft=True``: softmax of the teacher
    column (``--no_sampling``).  Returns (loss [G], pick [G], target [G]): the student's and the teacher's argmax, the lowest position on a tie.  A graph
    with a pointer pair that is no range of its table or a column outside 0 .. D - 1 gets loss NaN, indices -1 and no gradient.  Differentiable in the
    two logit tables only; with neither asking for a gradient nothing is saved and no gradient is computed.  No atomics."""
    if not (torch.is_tensor(logit_l) and logit_l.is_cuda):
        raise RuntimeError('ddk ragged_node_cross_entropy runs on the GPU only (no CPU fallback)')
    args = (logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, bool(soft))
    if torch.is_grad_enabled() and (logit_l.requires_grad or logit_r.requires_grad):
        return _RaggedNodeCrossEntropyFunction.apply(*args)
    return _ctx_of(logit_l).node_cross_entropy(*args)[:3]


class _HeadConvFunction(torch.autograd.Function):
    """ddk_hconv_forward with ddk_hconv_backward as its vector-Jacobian product: node features to receiver rows through a head's
    FullyConnectedTensorProduct.  Saved for the backward: the node table, sh, h, the graph, and w2 / b2 where a requested gradient reads them; never the
    gathered rows, the tensor product's rows or the per-edge weights.  No atomics: the gradients have the same bits on every run.  sh gets no gradient."""

    @staticmethod
    def forward(fctx, node_attr, sh, h, w2, b2, head, graph):
        ctx = _ctx_of(node_attr)
        x, s, hh = _as_rows(node_attr, node_attr.shape[-1]), _as_rows(sh, 4), _as_rows(h, h.shape[-1])
        w, b = w2.contiguous().float(), b2.contiguous().float()
        out = ctx.hconv_forward(head, graph, x, s, hh, w, b)
        ng = fctx.needs_input_grad
        fctx.save_for_backward(x, s, hh, w if (ng[0] or ng[2]) else None, b if ng[0] else None)      # the parameter gradients read neither
        fctx.head, fctx.ddk, fctx.graph = head, ctx, graph
        fctx.meta = [(t.shape, t.dtype) for t in (node_attr, h, w2, b2)]
        return out

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_out):
        x, s, hh, w, b = fctx.saved_tensors
        ng = fctx.needs_input_grad
        need = (ng[0], ng[2], ng[3], ng[4])
        g = _grad_rows(grad_out)
        with torch.cuda.device(x.device):
            gx, gh, gw2, gb2 = _grads_like(fctx.ddk.hconv_backward(fctx.head, fctx.graph, x, s, hh, w, b, g, need), fctx.meta)
        return gx, None, gh, gw2, gb2, None, None


def fused_head_conv(head, fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes, graph=None, hidden=None):
    """Lines 153-159 of the reference's TensorProductConvLayer.forward (models/tensor_layers.py) for a score head, ``faster=False, edge_groups=1,
    reduce='mean'``, as one differentiable op: ``scatter(o3.FullyConnectedTensorProduct(...)(node_attr[edge_dst], edge_sh, fc(edge_attr)), edge_src,
    dim_size=out_nodes, reduce='mean')``.  ``head``: ``runtime.HEAD_CENTER`` (final_conv) or ``runtime.HEAD_TORSION`` (tor_bond_conv); ``fc``: ONE FCBlock
    whose Linears are K -> K and K -> W of ``runtime.head_tp_shape(head)``.  ``fc[:4]`` (Linear, ReLU, Dropout) runs in torch unless ``hidden`` [E, K] is
    given; the last Linear, the gather, the tensor product and the mean run in the kernels of csrc/k_hconv.hip, forward and backward: no [E, W] weights,
    no gathered rows, no atomics, so ``node_attr``, ``edge_attr`` and every parameter of ``fc`` get the same gradient bits on every run.  ``edge_sh``
    [E, 4]: (1x0e, 1x1o) for the centre head; (anything, T) for the torsion head, T the 1o block of ``FullTensorProduct(sh_irreps, '2e')``.  It gets
    no gradient (positions carry none in score matching): an ``edge_sh`` that requires one raises.  ``graph``: the ``ConvGraph`` of ``edge_index`` from
    ``node_attr``'s rows to ``out_nodes`` receivers, built here otherwise.  [out_nodes, dout], fp32."""
    s = head_tp_shape(head)
    K, W = s['K'], s['W']
    if (not isinstance(fc, nn.Sequential) or len(fc) != 5 or not isinstance(fc[0], nn.Linear) or not isinstance(fc[4], nn.Linear)
            or (fc[0].in_features, fc[0].out_features) != (K, K) or (fc[4].in_features, fc[4].out_features) != (K, W) or fc[4].bias is None):
        raise RuntimeError(f'ddk: fused_head_conv takes one 2-layer FCBlock whose Linears map {K} -> {K} and {K} -> {W} (edge_groups == 1)')
    if not node_attr.is_cuda:
        raise RuntimeError('ddk fused_head_conv runs on the GPU only (no CPU fallback)')
    if edge_sh.requires_grad:
        raise RuntimeError('ddk: fused_head_conv has no gradient for edge_sh (positions carry none in score matching); detach it')
    if node_attr.dim() != 2 or node_attr.shape[1] != s['din']:
        raise RuntimeError(f'ddk: fused_head_conv takes node_attr [N, {s["din"]}], the output of conv layer 3; got {tuple(node_attr.shape)}')
    n_out = int(out_nodes)
    if graph is None:
        graph = Context.conv_graph(edge_index[0], edge_index[1], node_attr.shape[0], n_out)
    if graph.n_in != node_attr.shape[0] or graph.n_out != n_out:
        raise RuntimeError(f'ddk: fused_head_conv: the graph ({graph.n_in} -> {graph.n_out} nodes) does not fit {node_attr.shape[0]} -> {n_out} nodes')
    if hidden is None:
        hidden = fc[:4](edge_attr)
    if hidden.dim() != 2 or hidden.shape != (graph.E, K) or edge_sh.shape != (graph.E, 4):
        raise RuntimeError(f'ddk: fused_head_conv takes edge_sh [E, 4] and a hidden activation [E, {K}] with E = {graph.E}, the edges of the graph; got '
                           f'{tuple(edge_sh.shape)} and {tuple(hidden.shape)}')
    w2, b2 = fc[4].weight, fc[4].bias
    if torch.is_grad_enabled() and any(t.requires_grad for t in (node_attr, hidden, w2, b2)):
        return _HeadConvFunction.apply(node_attr, edge_sh, hidden, w2, b2, head, graph)
    return _ctx_of(node_attr).hconv_forward(head, graph, node_attr, edge_sh, hidden, w2, b2)


class _GatherRowsFunction(torch.autograd.Function):
    """x[index] whose backward adds the rows of a node in ascending position (ddk_seg_sum over the node-sorted list), not with index_add_'s atomics."""

    @staticmethod
    def forward(fctx, x, index, order, ptr):
        fctx.save_for_backward(order, ptr)
        fctx.meta = (x.shape, x.dtype)
        return x.index_select(0, index)

    @staticmethod
    @once_differentiable
    def backward(fctx, grad):
        order, ptr = fctx.saved_tensors
        shape, dtype = fctx.meta
        with torch.cuda.device(grad.device):
            nodes = _ctx_of(grad).seg_sum(grad.reshape(grad.shape[0], -1), order, ptr)
        return nodes.reshape(shape).to(dtype), None, None, None


def gather_rows(x, index, graph=None, side='dst'):
    """``x[index]`` ([E, ...] rows of the node table ``x``) with a run-to-run reproducible backward: the gradient rows of a node are added in ascending
    position from a node-sorted list, where ``index_select``'s backward is ``index_add_`` with float atomics.  ``graph``: a ``ConvGraph`` whose
    ``side`` ('dst' or 'src') IS ``index`` over ``x``'s rows, so that its sorted list is reused; without it the list is made here (one stable sort).
    The backward is the device's segmented sum (``Context.seg_sum``): GPU tensors only."""
    if not x.is_cuda:
        raise RuntimeError('ddk gather_rows runs on the GPU only (no CPU fallback)')
    index = index.long()
    if graph is not None:
        order, ptr = (graph.dst_order, graph.dst_ptr) if side == 'dst' else (graph.src_order, graph.src_ptr)
        if order.shape[0] != index.shape[0] or ptr.shape[0] != x.shape[0] + 1:
            raise RuntimeError(f'ddk: gather_rows: the graph\'s {side} side ({order.shape[0]} edges, {ptr.shape[0] - 1} nodes) does not fit '
                               f'{index.shape[0]} indices into {x.shape[0]} rows')
    else:
        order = torch.sort(index, stable=True).indices.to(torch.int32)
        ptr = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=index.device)
        ptr[1:] = torch.cumsum(torch.bincount(index, minlength=x.shape[0])[:x.shape[0]], 0)
    if torch.is_grad_enabled() and x.requires_grad:
        return _GatherRowsFunction.apply(x, index, order, ptr)
    return x.index_select(0, index)


def FCBlock(in_dim, hidden_dim, out_dim, layers, dropout, activation='relu', batchnorm=False):
    """Same Sequential layout (indices 0 and 4 hold the Linears) as the reference models/layers.py:15-22."""
    if layers != 2 or activation != 'relu' or batchnorm:
        raise RuntimeError('ddk: only the 2-layer ReLU radial MLP is implemented')
    return nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.Identity(), nn.ReLU(), nn.Dropout(dropout), nn.Linear(hidden_dim, out_dim))


class _BatchNormParams(nn.Module):
    """Parameter holder with e3nn.nn.BatchNorm's state_dict keys (weight, bias, running_mean, running_var)."""

    def __init__(self, irreps):
        super().__init__()
        listed = _irreps_list(irreps)      # in the order written: the torsion head's '24x0o + 24x0e' puts its scalars second
        nf, nsc = sum(mul for mul, _ in listed), sum(mul for mul, ir in listed if ir == '0e')
        self.register_buffer('running_mean', torch.zeros(nsc))
        self.register_buffer('running_var', torch.ones(nf))
        self.weight = nn.Parameter(torch.ones(nf))
        self.bias = nn.Parameter(torch.zeros(nsc))
        self.blocks = [(mul, _DIM[ir], ir == '0e') for mul, ir in listed]      # (mul, d, scalar): 0o is not a scalar for e3nn (no mean, no bias)
        self.eps, self.momentum = 1e-5, 0.1

    def forward(self, x):
        """e3nn.nn.BatchNorm.forward with its defaults (affine, reduce='mean', normalization='component', not instance) in plain torch, so that autograd
        differentiates it: the batch statistics are not detached in the normalisation.  Training updates the running buffers; evaluation reads them."""
        out, ix, iw, ib = [], 0, 0, 0
        for mul, d, scalar in self.blocks:
            field = x[:, ix:ix + mul * d].reshape(-1, mul, d)
            ix += mul * d
            if scalar:
                if self.training:
                    mean = field.mean(dim=(0, 2))
                    with torch.no_grad():
                        self.running_mean[ib:ib + mul] = (1 - self.momentum) * self.running_mean[ib:ib + mul] + self.momentum * mean.detach()
                else:
                    mean = self.running_mean[ib:ib + mul]
                field = field - mean.reshape(1, mul, 1)
            if self.training:
                norm = field.pow(2).mean(-1).mean(0)      # the biased estimate, which also feeds the running average
                with torch.no_grad():
                    self.running_var[iw:iw + mul] = (1 - self.momentum) * self.running_var[iw:iw + mul] + self.momentum * norm.detach()
            else:
                norm = self.running_var[iw:iw + mul]
            field = field * ((norm + self.eps).pow(-0.5) * self.weight[iw:iw + mul]).reshape(1, mul, 1)
            if scalar:
                field = field + self.bias[ib:ib + mul].reshape(1, mul, 1)
                ib += mul
            iw += mul
            out.append(field.reshape(-1, mul * d))
        return torch.cat(out, dim=-1)


class TensorProductConvLayer(nn.Module):
    all_atom = False      # True on a conv layer of the all-atom (confidence) model: sh_irreps of second order

    def __init__(self, in_irreps, sh_irreps, out_irreps, n_edge_features, residual=True, batch_norm=True, dropout=0.0,
                 hidden_features=None, faster=False, edge_groups=1, tp_weights_layers=2, activation='relu'):
        super().__init__()
        self.head = self._head_configuration(in_irreps, sh_irreps, out_irreps, n_edge_features, residual, hidden_features, faster, edge_groups,
                                             tp_weights_layers, activation)
        if self.head is not None:
            # final_conv / tor_bond_conv (models/score_model.py:132-161): e3nn's FullyConnectedTensorProduct, one FCBlock, no residual
            s = head_tp_shape(self.head)
            self.in_irreps, self.out_irreps, self.sh_irreps = str(in_irreps), str(out_irreps), sh_irreps
            self.residual, self.edge_groups, self.out_size = residual, edge_groups, s['dout']
            self.fc = FCBlock(n_edge_features, s['K'], s['W'], tp_weights_layers, dropout, activation)      # a plain FCBlock: keys fc.0.weight, fc.4.bias
            self.batch_norm = _BatchNormParams(out_irreps) if batch_norm else None
            return
        self.all_atom = _is_second_order_sh(sh_irreps)
        if self.all_atom:
            # a conv layer of the all-atom (confidence) model (all_atom_score_model.py:15-50): e3nn's FullyConnectedTensorProduct with sh_lmax = 2, one radial
            # MLP WITHOUT the FCBlock's Identity (keys fc.0.*, fc.3.*), no residual, senders and receivers possibly different node tables
            if faster or edge_groups != 1 or residual or tp_weights_layers != 2 or activation != 'relu':
                raise RuntimeError('ddk: an all-atom conv layer (sh_irreps 1x0e + 1x1o + 1x2e) is faster=False, edge_groups=1, residual=False with a 2-layer ReLU radial MLP')
            if n_edge_features != 72 or hidden_features not in (None, 72):
                raise RuntimeError('ddk: radial MLP width must be 3*ns = 72')
            self.in_irreps, self.out_irreps, self.sh_irreps = str(in_irreps), str(out_irreps), sh_irreps
            self.residual, self.edge_groups = residual, edge_groups
            self.tp = FullyConnectedTensorProduct(in_irreps, sh_irreps, out_irreps)
            self.layer, self.out_size = self.tp.layer, self.tp.out_size
            self.fc = nn.Sequential(nn.Linear(72, 72), nn.ReLU(), nn.Dropout(dropout), nn.Linear(72, self.tp.weight_numel))
            self.batch_norm = _BatchNormParams(out_irreps) if batch_norm else None
            return
        if not faster or edge_groups != 4 or not residual:
            raise RuntimeError('ddk: the fused kernel implements faster=True, edge_groups=4, residual=True conv layers')
        self.in_irreps, self.out_irreps, self.sh_irreps = str(in_irreps), str(out_irreps), sh_irreps
        self.residual, self.edge_groups = residual, edge_groups
        self.out_size = irrep_to_size(out_irreps)
        hidden_features = n_edge_features if hidden_features is None else hidden_features
        self.tp = FasterTensorProduct(in_irreps, sh_irreps, out_irreps)
        self.layer = self.tp.layer
        if n_edge_features != 72 or hidden_features != 72:
            raise RuntimeError('ddk: radial MLP width must be 3*ns = 72')
        self.fc = nn.ModuleList([FCBlock(n_edge_features, hidden_features, self.tp.weight_numel, tp_weights_layers, dropout,
                                         activation) for _ in range(edge_groups)])
        self.batch_norm = _BatchNormParams(out_irreps) if batch_norm else None
        self._ctx, self._ctx_key = None, None
        # evaluation runs the fused inference kernel, whose scatter is an fp32 atomic add: the last bits of an evaluation forward then differ from run to
        # run.  True: evaluate with the training ops instead (no atomics; dropout rate 0 and BatchNorm on its running buffers, as an nv = 4 layer does)
        self.eval_with_training_ops = False

    @staticmethod
    def _head_configuration(in_irreps, sh_irreps, out_irreps, n_edge_features, residual, hidden_features, faster, edge_groups, tp_weights_layers,
                            activation):
        """HEAD_CENTER / HEAD_TORSION when the arguments are those models/score_model.py:132-161 passes to final_conv / tor_bond_conv, else None"""
        if faster or edge_groups != 1 or residual or tp_weights_layers != 2 or activation != 'relu':
            return None
        try:
            if tuple(parse_irreps(in_irreps).values()) != (24, 6, 6, 24):
                return None
            out = _irreps_list(out_irreps)
        except (RuntimeError, ValueError):
            return None
        sh = str(sh_irreps).replace(' ', '').split('+')
        # the torsion head's sh irreps: the 1o block first (the only one with a path to a scalar), then 2e, 2o, 3o in the order the caller's sort gives
        for head, sh_want, out_want in ((HEAD_CENTER, ['1x0e', '1x1o'], [(2, '1o'), (2, '1e')]),
                                        (HEAD_TORSION, ['1x1o', '1x2e', '1x2o', '1x3o'], [(24, '0o'), (24, '0e')])):
            K = head_tp_shape(head)['K']
            if sh[0] == sh_want[0] and sorted(sh) == sh_want and out == out_want and n_edge_features == K and hidden_features in (None, K):
                return head
        return None

    def _forward_head(self, node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce, graph=None):
        """The reference's forward (models/tensor_layers.py:147-168) of a head: fused_head_conv, then BatchNorm (batch statistics in training, the running
        buffers in evaluation), no residual.  Training and evaluation run the same kernels.  The torsion head takes ``edge_sh`` as the reference passes it,
        [E, 20] = FullTensorProduct(sh_irreps, '2e') whose first three columns are the 1o block, or as the op does, [E, 4] = (anything, 1o block)."""
        if reduce != 'mean':
            raise RuntimeError("ddk: conv layers aggregate with reduce='mean'")
        if not node_attr.is_cuda:
            raise RuntimeError('ddk TensorProductConvLayer runs on the GPU only (no CPU fallback)')
        if edge_index.shape[1] == 0:      # (as there: zeros on all nodes, no BatchNorm)
            return torch.zeros((node_attr.shape[0], self.out_size), dtype=node_attr.dtype, device=node_attr.device)
        if self.head == HEAD_TORSION and edge_sh.shape[-1] == 20:
            edge_sh = torch.nn.functional.pad(edge_sh[:, :3], (1, 0))
        out = fused_head_conv(self.head, self.fc, node_attr, edge_index, edge_sh, edge_attr, int(out_nodes or node_attr.shape[0]), graph=graph)
        return self.batch_norm(out) if self.batch_norm is not None else out

    def _context(self, device):
        key = (device.index or 0, tuple(int(p._version) for p in self.state_dict().values()))
        if self._ctx is None or self._ctx_key != key:
            ctx = Context(device=device.index or 0, batch_norm=int(self.batch_norm is not None))
            ctx.load_state_dict(self.state_dict(), prefix=f'conv_layers.{self.layer}.')
            self._ctx, self._ctx_key = ctx, key
        return self._ctx

    def _forward_all_atom(self, node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce, graph=None, hidden=None):
        """The all-atom layer's forward (all_atom_score_model.py:36-50): ``BN(scatter_mean(tp(node_attr[edge_dst], edge_sh, fc(edge_attr)), edge_src,
        out_nodes))`` through fused_radial_conv; ``edge_sh`` [E, 9].  BatchNorm is applied ALWAYS: a conv without edges gives BatchNorm of zeros (and moves
        the running buffers in training), where the score model's layer returns the zeros.  Training and evaluation run the same kernels (the modules' own
        mode gives dropout rate 0 and BatchNorm on its running buffers)."""
        if reduce != 'mean':
            raise RuntimeError("ddk: conv layers aggregate with reduce='mean'")
        if not node_attr.is_cuda:
            raise RuntimeError('ddk TensorProductConvLayer runs on the GPU only (no CPU fallback)')
        n_out = int(out_nodes or node_attr.shape[0])
        if edge_index.shape[1] == 0:
            out = torch.zeros((n_out, self.out_size), dtype=torch.float32, device=node_attr.device)
        elif hidden is not None:
            out = fused_radial_conv(self.tp, self.fc, node_attr, edge_index, edge_sh, [0, edge_index.shape[1]], out_nodes=n_out, graph=graph, hidden=hidden)
        else:
            out = fused_radial_conv(self.tp, self.fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes=n_out, graph=graph)
        return self.batch_norm(out) if self.batch_norm is not None else out

    def forward_embedded_all_atom(self, recv_attr, send_attr, edge_index, edge_emb, edge_sh, graph=None, hidden_graph=None, seed=None):
        """One conv of the all-atom model's loop (all_atom_score_model.py:232-268) from the edge EMBEDDING [E, ns]: what ``forward(send_attr, edge_index,
        [edge_emb | recv_attr[edge_index[0], :ns] | send_attr[edge_index[1], :ns]], edge_sh, out_nodes=recv_attr.shape[0])`` returns, without the row
        [E, 72]: ``fused_radial_hidden`` on the two scalar tables concatenated (receivers first, the senders' index shifted; torch's cat has a deterministic
        backward) -> ``fused_radial_conv(hidden=...)`` -> BatchNorm.  ``recv_attr is send_attr``: one table (ll, aa, rr).  ``graph``: the ``ConvGraph`` of
        ``edge_index`` from the senders to the receivers; ``hidden_graph``: that of the shifted index over the concatenated table (``graph`` itself for one
        table); both built here otherwise.  ``seed``: of the dropout mask."""
        if not self.all_atom:
            raise RuntimeError('ddk: forward_embedded_all_atom is a step of the all-atom model; this layer has forward_embedded')
        E, n_recv, n_send = edge_index.shape[1], recv_attr.shape[0], send_attr.shape[0]
        if edge_emb.shape[0] != E:
            raise RuntimeError(f'ddk: forward_embedded_all_atom takes one edge_emb row per edge; got {edge_emb.shape[0]} for {E} edges')
        if E == 0:
            return self._forward_all_atom(send_attr, edge_index, None, edge_sh, n_recv, 'mean')
        if graph is None:
            graph = Context.conv_graph(edge_index[0], edge_index[1], n_send, n_recv)
        if recv_attr is send_attr:
            table, hidden_graph = recv_attr, graph
        else:
            table = torch.cat([recv_attr[:, :24], send_attr[:, :24]], 0)
            if hidden_graph is None:
                hidden_graph = Context.conv_graph(edge_index[0], edge_index[1] + n_recv, n_recv + n_send, n_recv + n_send)
        hidden = fused_radial_hidden(self.fc, table, edge_emb, [0, E], hidden_graph, seed=seed)
        return self._forward_all_atom(send_attr, edge_index, None, edge_sh, n_recv, 'mean', graph=graph, hidden=hidden)

    def forward(self, node_attr, edge_index, edge_attr, edge_sh, out_nodes=None, reduce='mean'):
        if self.head is not None:
            return self._forward_head(node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce)
        if self.all_atom:
            return self._forward_all_atom(node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce)
        if self.training or self.layer >= TP_NV4 or self.eval_with_training_ops:      # the fused inference kernel is nv = 6 only: an nv = 4 layer evaluates with the training ops
            return self._forward_training(node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce)
        if reduce != 'mean' or (out_nodes is not None and out_nodes != node_attr.shape[0]):
            raise RuntimeError("ddk: conv layers aggregate with reduce='mean' onto all nodes")
        if not node_attr.is_cuda:
            raise RuntimeError('ddk TensorProductConvLayer runs on the GPU only (no CPU fallback)')
        offs = [0]
        for ea in edge_attr:
            offs.append(offs[-1] + ea.shape[0])
        ea = torch.cat(list(edge_attr), dim=0)
        ctx = self._context(node_attr.device)
        return ctx.conv_forward(self.layer, node_attr, edge_index[0], edge_index[1], offs, ea, edge_sh, self.out_size)


    def _forward_training(self, node_attr, edge_index, edge_attr, edge_sh, out_nodes, reduce):
        """The reference's forward (models/tensor_layers.py:147-168) in training: fused_radial_conv, BatchNorm on the batch statistics, the padded
        residual.  Without edges: zeros and no BatchNorm, as there.  An nv = 4 layer runs this in evaluation too: the modules' own mode then gives
        dropout rate 0 and BatchNorm on its running buffers."""
        if reduce != 'mean':
            raise RuntimeError("ddk: conv layers aggregate with reduce='mean'")
        if not node_attr.is_cuda:
            raise RuntimeError('ddk TensorProductConvLayer runs on the GPU only (no CPU fallback)')
        if edge_index.shape[1] == 0:
            out = torch.zeros((node_attr.shape[0], self.out_size), dtype=node_attr.dtype, device=node_attr.device)
        else:
            out = fused_radial_conv(self.tp, self.fc, node_attr, edge_index, edge_sh, edge_attr, out_nodes=out_nodes)
            if self.batch_norm is not None:
                out = self.batch_norm(out)
        return out + torch.nn.functional.pad(node_attr, (0, out.shape[-1] - node_attr.shape[-1]))

    def forward_embedded(self, node_attr, edge_index, edge_emb, group_sizes, edge_sh, graph=None, seed=None):
        """One step of the reference's embed loop (models/score_model.py:227-230) from the edge EMBEDDING [E, ns]: what ``forward`` returns for
        ``edge_attr = [edge_emb | node_attr[edge_index[0], :ns] | node_attr[edge_index[1], :ns]]`` cut into groups of ``group_sizes`` edges.  In
        training the row [E, 72] is never built: ``fused_radial_hidden`` -> ``fused_radial_conv(hidden=...)`` -> BatchNorm -> residual, without
        atomics.  ``graph``: the ``ConvGraph`` of ``edge_index`` over the nodes, built here otherwise; ``seed``: of the dropout mask
        (``fused_radial_hidden``).  In evaluation the cat is built and ``forward`` runs the inference kernel, unchanged; an nv = 4 layer, which has no inference
        kernel, runs the training ops there too (dropout rate 0, BatchNorm on its running buffers)."""
        if self.head is not None or self.all_atom:
            raise RuntimeError('ddk: forward_embedded is a step of the conv stack; a head layer has forward alone' if self.head is not None else
                               'ddk: forward_embedded is a step of the score model\'s conv stack; an all-atom layer has forward_embedded_all_atom')
        sizes = [int(n) for n in group_sizes]
        E = edge_index.shape[1]
        if len(sizes) != self.edge_groups or any(n < 0 for n in sizes) or sum(sizes) != E or edge_emb.shape[0] != E:
            raise RuntimeError(f'ddk: forward_embedded takes {self.edge_groups} group sizes that add up to the {E} edges of edge_index and edge_emb')
        if not self.training and self.layer < TP_NV4 and not self.eval_with_training_ops:
            ns = edge_emb.shape[1]
            edge_attr = torch.cat([edge_emb, node_attr[edge_index[0], :ns], node_attr[edge_index[1], :ns]], -1)
            return self.forward(node_attr, edge_index, list(torch.split(edge_attr, sizes)), edge_sh)
        if not node_attr.is_cuda:
            raise RuntimeError('ddk TensorProductConvLayer runs on the GPU only (no CPU fallback)')
        if E == 0:
            out = torch.zeros((node_attr.shape[0], self.out_size), dtype=node_attr.dtype, device=node_attr.device)
        else:
            offs = [0]
            for n in sizes:
                offs.append(offs[-1] + n)
            if graph is None:
                graph = Context.conv_graph(edge_index[0], edge_index[1], node_attr.shape[0], node_attr.shape[0])
            hidden = fused_radial_hidden(self.fc, node_attr, edge_emb, offs, graph, seed=seed)
            out = fused_radial_conv(self.tp, self.fc, node_attr, edge_index, edge_sh, offs, graph=graph, hidden=hidden)
            if self.batch_norm is not None:
                out = self.batch_norm(out)
        return out + torch.nn.functional.pad(node_attr, (0, out.shape[-1] - node_attr.shape[-1]))


class GaussianSmearing(nn.Module):
    """Distance embedding (tensor_layers.py:171-181); kept as a module so that state_dicts carry `offset`."""

    def __init__(self, start=0.0, stop=5.0, num_gaussians=50):
        super().__init__()
        offset = torch.linspace(start, stop, num_gaussians)
        self.coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
        self.register_buffer('offset', offset)

    def forward(self, dist):
        dist = dist.view(-1, 1) - self.offset.view(1, -1)
        return torch.exp(self.coeff * torch.pow(dist, 2))
