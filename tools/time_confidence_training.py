"""Timing of the all-atom confidence model's training ops (reported, not gated): prints markdown for profiles/confidence_training_kernel_stats.md.

    python tools/time_confidence_training.py [--edges 200000 800000] [--residues 300] [--batch 4]

1. One conv op of layer 3 (DDK_TP_AA + 3), forward + backward with all gradients, against the torch composition it replaces: ``index_select``, the radial
   MLP's last Linear ([E, 1944] per-edge weights), the einsum FullyConnectedTensorProduct, ``index_add_`` / count.  Same GPU, median of three runs, time
   (events around forward + backward) and peak memory above what the operands hold.
2. One whole training step (forward, BCE loss, backward, Adam) of ``TrainableConfidenceModel`` on a batch of synthetic complexes."""
import argparse
import os
import sys
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from disco_diffdock_amd import synthetic      # noqa: E402
from disco_diffdock_amd.runtime import Context, tp_layer_shape_aa      # noqa: E402
from disco_diffdock_amd.tensor_layers import FullyConnectedTensorProduct, fused_radial_conv      # noqa: E402

IRREPS = '24x0e+6x1o+6x1e+24x0o'
DIMS = {'0e': 1, '1o': 3, '1e': 3, '0o': 1}


def kind_tensors(dev):
    """the bilinear map of each path kind, T [d_in, 9, d_out] (runtime.tp_layer_shape_aa's kinds)"""
    T = {k: torch.zeros(a, 9, b) for k, (a, b) in dict(ss=(1, 1), sv=(1, 3), vs=(3, 3), vd=(3, 1), vx=(3, 3), v2=(3, 3)).items()}
    T['ss'][0, 0, 0] = 1
    for k in range(3):
        T['sv'][0, 1 + k, k] = T['vs'][k, 0, k] = T['vd'][k, 1 + k, 0] = 1
    for a, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        T['vx'][a, 1 + j, k], T['vx'][j, 1 + a, k] = 1, -1
    r = 3 ** -0.5
    for m, entries in enumerate((((0, 2, 1),), ((0, 1, 1),), ((0, 0, -r), (1, 1, 2 * r), (2, 2, -r)), ((1, 2, 1),), ((0, 0, -1), (2, 2, 1)))):
        for a, k, v in entries:
            T['v2'][a, 4 + m, k] = T['v2'][k, 4 + m, a] = v
    return {k: v.to(dev) for k, v in T.items()}


def composition(s, T, x, ei, sh, h, w2, b2, n_out):
    """the unfused layer: gather, per-edge weights, one einsum per e3nn instruction, scatter-mean with index_add_"""
    E = ei.shape[1]
    w = h @ w2.T + b2
    xg = x.index_select(0, ei[1])
    outs = []
    for ir in ('0e', '1o', '1e', '0o'):
        acc = 0
        for p in s['paths']:
            if p['ir_out'] != ir:
                continue
            I = xg[:, p['xoff']:p['xoff'] + p['mul_in'] * DIMS[p['ir_in']]].reshape(E, p['mul_in'], -1)
            wp = w[:, p['offset']:p['offset'] + p['mul_in'] * p['mul_out']].reshape(E, p['mul_in'], p['mul_out'])
            acc = acc + p['scale'] * torch.einsum('euo,ajk,eua,ej->eok', wp, T[p['kind']], I, sh).reshape(E, -1)
        outs.append(acc)
    rows = torch.cat(outs, 1)
    cnt = torch.bincount(ei[0], minlength=n_out).clamp(min=1).to(rows.dtype)
    return torch.zeros((n_out, rows.shape[1]), device=x.device).index_add_(0, ei[0], rows) / cnt[:, None]


def measure(fn, params, reps=3):
    times, peaks = [], []
    for _ in range(reps + 1):      # the first run warms up
        for p in params:
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        out.backward(torch.ones_like(out))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        peaks.append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        del out
    return float(np.median(times[1:])), float(np.median(peaks[1:]))


def conv_op(E, dev):
    s, T = tp_layer_shape_aa(3), kind_tensors(dev)
    n = max(E // 20, 1)
    g = torch.Generator(device='cpu').manual_seed(E)
    ei = torch.randint(0, n, (2, E), generator=g).to(dev)
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    x, h, w2, b2 = (mk(n, 84).requires_grad_(), mk(E, 72).relu().requires_grad_(), (mk(1944, 72) / 72 ** 0.5).requires_grad_(), mk(1944).requires_grad_())
    sh = mk(E, 9)
    tp = FullyConnectedTensorProduct(IRREPS, '1x0e+1x1o+1x2e', IRREPS)
    fc = torch.nn.Sequential(torch.nn.Linear(72, 72), torch.nn.ReLU(), torch.nn.Dropout(0.0), torch.nn.Linear(72, 1944)).to(dev)
    fc[3].weight, fc[3].bias = torch.nn.Parameter(w2.detach().clone()), torch.nn.Parameter(b2.detach().clone())
    graph = Context.conv_graph(ei[0], ei[1], n, n)
    fused = lambda: fused_radial_conv(tp, fc, x, ei, sh, [0, E], out_nodes=n, graph=graph, hidden=h)
    t_f, m_f = measure(fused, [x, h, fc[3].weight, fc[3].bias])
    t_c, m_c = measure(lambda: composition(s, T, x, ei, sh, h, w2, b2, n), [x, h, w2, b2])
    with torch.no_grad():
        err = float((fused() - composition(s, T, x, ei, sh, h, w2, b2, n)).abs().max())
    return t_f, m_f, t_c, m_c, err


def whole_step(n_res, B, dev):
    from disco_diffdock_amd.model_utils import get_trainable_model
    from oracle import graph_lite
    to_graph = lambda c: graph_lite.make_complex(c['lig_x'], c['lig_pos'], c['bond_index'], c['bond_attr'], c['edge_mask'], c['mask_rotate'], c['rec_x'],
                                                 c['rec_pos'], c['rec_edge_index'], c['original_center'])
    args = Namespace(all_atoms=True, ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32, max_radius=5.0,
                     cross_max_distance=80, dynamic_max_cross=True, embedding_type='sinusoidal', embedding_scale=10000, scale_by_sigma=True, no_torsion=False,
                     no_batch_norm=False, dropout=0.1, use_second_order_repr=False, esm_embeddings_path='esm', rmsd_classification_cutoff=2.0,
                     tr_sigma_min=0.1, tr_sigma_max=34.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.0314, tor_sigma_max=3.14)
    model = get_trainable_model(args, dev, confidence_mode=True).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    graphs = []
    for i in range(B):
        c = synthetic.make_complex(100 + i, n_res=n_res, n_lig=30)
        synthetic.add_receptor_atoms(c, np.random.default_rng(i))
        graphs.append(graph_lite.add_atoms(to_graph(c), c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index']))
    b = graph_lite.collate(graphs)
    b.complex_t = {k: torch.zeros(B) for k in ('tr', 'rot', 'tor')}
    b = b.to(dev)
    y = (torch.arange(B, device=dev) % 2).float()
    times = []
    for step in range(4):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(b, seed=step), y)
        loss.backward()
        opt.step()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e))
    sizes = (b['ligand'].num_nodes, b['receptor'].num_nodes, b['atom'].num_nodes, b['atom', 'atom'].edge_index.shape[1])
    return float(np.median(times[1:])), torch.cuda.max_memory_allocated() / 2 ** 20, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--edges', type=int, nargs='*', default=[200000, 800000])
    ap.add_argument('--residues', type=int, default=300)
    ap.add_argument('--batch', type=int, default=4)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    print('| layer 3 conv op, forward + backward | fused ms | fused peak MiB | composition ms | composition peak MiB | max abs difference of the outputs |')
    print('|---|---|---|---|---|---|')
    for E in a.edges:
        t_f, m_f, t_c, m_c, err = conv_op(E, dev)
        print(f'| E = {E} | {t_f:.2f} | {m_f:.0f} | {t_c:.2f} | {m_c:.0f} | {err:.1e} |', flush=True)
    t, peak, sizes = whole_step(a.residues, a.batch, dev)
    print(f'\nWhole training step (forward, loss, backward, Adam), {a.batch} complexes of {a.residues} residues ({sizes[0]} ligand atoms, {sizes[1]} residues, '
          f'{sizes[2]} receptor atoms, {sizes[3]} atom-atom edges): {t:.1f} ms, peak {peak:.0f} MiB (median of three steps after one warm-up)')


if __name__ == '__main__':
    main()
