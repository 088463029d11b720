"""BASELINE metric, second clause, at the REFERENCE's op boundary: FasterTensorProduct.forward (models/tensor_layers.py:65-116) with the per-edge
weights [E, W] resident in HBM (SURVEY.md 8(d) boundary (A): 8 184 B per edge at layers 3 / 4, 0.7 FLOP/B - HBM-bound).  Times ddk_tp_forward
(tp_stream_kernel, k_tp.hip) with events on the launch stream and checks a slice against the fp64 restatement below.

    python tools/bench_tp.py [--layer 3] [--edges 800000] [--json out.json]        (run it under rocprofv3 --kernel-trace / --pmc for the profile)

    python tools/bench_tp.py --backward [--edges 800000] [--json out.json]
times, for each of the four layer shapes, the forward, ddk_tp_backward (tp_bwd_kernel, k_tp_bwd.hip) with all outputs, with grad_w alone and with
grad_x + grad_sh alone, and in the same run what a user has without it: PyTorch autograd, forward plus backward, of a plain-torch fp32 restatement.
Every figure is the median of --repeats passes of --iters calls between two events, after warm-up; GB/s are the algorithmic bytes of each mode.

    python tools/bench_tp.py --radial [--edges 200000] [--iters 30] [--json out.json]
times, for each of the four layer shapes and four equal edge groups, one training step of the op with all gradients two ways in the same run:
tensor_layers.fused_radial_tp (ddk_rtp_forward / ddk_rtp_backward, k_rtp.hip: the per-edge weights [E, W] never exist) and the composition it replaces
(the fc Linears, torch.cat, FasterTensorProduct forward and backward, autograd through the Linears), with the peak device memory of each.

    python tools/bench_tp.py --conv [--edges 200000] [--nodes 8000] [--layers 0,3] [--iters 10] [--json out.json]
times one training step, forward + backward with all gradients, of the conv layer's lines 153-159 on one random graph (--nodes: default edges / 25) two
ways: (a) tensor_layers.fused_radial_conv (ddk_rconv_forward / ddk_rconv_backward: gather inside the kernels, fixed-order mean, no atomics) and (b) the
composition it replaces, index_select + fused_radial_tp + index_add_ / count.  The two paths alternate pass by pass; medians of --repeats passes, and the
peak device memory of one step of each.

    python tools/bench_tp.py --hidden [--edges 200000] [--nodes 8000] [--dropout 0.1] [--iters 10] [--json out.json]
times one training step, forward + backward with all gradients, of the radial MLP's hidden layer from the edge embedding two ways on one random graph:
(a) tensor_layers.fused_radial_hidden (ddk_rhid_forward / ddk_rhid_backward, k_rhid.hip: no [E, 72] row, no atomics, a counter-based dropout mask) and
(b) the composition it replaces, the reference's cat of [edge_emb | node_attr[src, :24] | node_attr[dst, :24]] and fc[g][:4] per group.  Same options,
alternation and medians as --conv; and the device passes of (a) on their own.

    python tools/bench_tp.py --heads [--iters 20] [--json out.json]
times one training step, forward + backward with all gradients, of the two head convolutions (final_conv, tor_bond_conv) two ways on the shapes of a
training batch, 1 200 and 12 000 ligand atoms in ligands of 30 atoms with 8 rotatable bonds each (20 neighbours per bond): (a)
tensor_layers.fused_head_conv (ddk_hconv_forward / ddk_hconv_backward, k_hconv.hip) and (b) a plain-torch restatement of the same composition, the radial
MLP, index_select, e3nn's FullyConnectedTensorProduct written out per weight block, index_add_ and the division.  Alternation and medians as --conv; the
device passes of (a) on their own; the launches per direction.

    python tools/bench_tp.py --embed [--iters 10] [--json out.json]
times one training step, forward + backward with all four parameter gradients, of one edge group's embedding in front of the conv stack two ways, at
E = 200 000 and 800 000 edges for K = 64 and K = 68 with dropout 0.1: (a) tensor_layers.fused_edge_embedding (ddk_eemb_forward / ddk_eemb_backward,
k_eemb.hip: nothing per edge but the outputs, a counter-based mask, no atomics) and (b) the plain-torch composition it replaces (two position gathers,
the norm, the Gaussian smearing, the gathered sigma embedding, the cat, Linear, ReLU, Dropout, Linear and the spherical harmonics).  Alternation and
medians as --conv; the peak device memory of one step of each; the device passes of (a) on their own.

    python tools/bench_tp.py --model [--iters 5] [--json out.json]
times forward + backward of train_model.TrainableScoreModel on a batch of 16 synthetic complexes, and its stages on their own (the graph build, the
node embeddings, the three edge embeddings, the conv stack, the heads).  Absolute times: there is nothing on the device to compare them with."""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from disco_diffdock_amd.tensor_layers import FasterTensorProduct

p = argparse.ArgumentParser()
p.add_argument('--layer', type=int, default=3)
p.add_argument('--edges', type=int, default=800000)
p.add_argument('--iters', type=int, default=10)
p.add_argument('--json', default=None)
p.add_argument('--backward', action='store_true')
p.add_argument('--radial', action='store_true')
p.add_argument('--conv', action='store_true')
p.add_argument('--hidden', action='store_true')
p.add_argument('--heads', action='store_true')
p.add_argument('--embed', action='store_true')
p.add_argument('--model', action='store_true')
p.add_argument('--dropout', type=float, default=0.1, help='--hidden: the dropout rate of the FCBlocks')
p.add_argument('--nodes', type=int, default=None, help='--conv, --hidden: nodes of the graph (default: edges / 25)')
p.add_argument('--layers', default='0,3', help='--conv: the layer shapes to time')
p.add_argument('--repeats', type=int, default=5)
p.add_argument('--baseline-edges', type=int, default=None, help='edges of the torch baseline (default: --edges; a smaller count is scaled and reported)')
a = p.parse_args()
dev = torch.device('cuda:0')
seq = ['24x0e', '24x0e+6x1o', '24x0e+6x1o+6x1e', '24x0e+6x1o+6x1e+24x0o']
MULS = [(24, 0, 0, 0), (24, 6, 0, 0), (24, 6, 6, 0), (24, 6, 6, 24)]


def tp_torch(x, sh, w, im, om):
    """tensor_layers.py:65-116 in plain torch, any dtype: the autograd baseline (fp32) and the check (fp64) of --backward"""
    n, (A, P, Q, C) = x.shape[0], im
    a_, p_ = x[:, :A], x[:, A:A + 3 * P].reshape(n, P, 3)
    q_, c_ = x[:, A + 3 * P:A + 3 * P + 3 * Q].reshape(n, Q, 3), x[:, A + 3 * P + 3 * Q:]
    s0, v = sh[:, :1], sh[:, None, 1:]
    cross = lambda t: torch.cross(t, v.expand_as(t), dim=-1) / 2 ** 0.5
    rows = [torch.cat([a_ * s0, (p_ * v).sum(-1) / 3 ** 0.5], 1)[..., None],
            torch.cat([a_[..., None] * v, p_ * s0[..., None], cross(q_)], 1),
            torch.cat([cross(p_), q_ * s0[..., None], c_[..., None] * v], 1),
            torch.cat([(q_ * v).sum(-1) / 3 ** 0.5, c_ * s0], 1)[..., None]]
    out, off = [], 0
    for r, n_out in zip(rows, om):
        n_in = r.shape[1]
        if n_out == 0 or n_in == 0:
            continue
        wk = w[:, off:off + n_in * n_out].reshape(n, n_in, n_out)
        off += n_in * n_out
        out.append((torch.einsum('eic,eio->eoc', r, wk) / n_in ** 0.5).reshape(n, -1))
    return torch.cat(out, 1)


def median_ms(fn, iters, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        times.append(st.elapsed_time(en) / iters)
    return sorted(times)[len(times) // 2]


def bench_backward():
    from disco_diffdock_amd.tensor_layers import _shape_context
    ctx = _shape_context(0)
    E, results = a.edges, []
    for layer in range(4):
        im, om = MULS[layer], MULS[min(layer + 1, 3)]
        tp = FasterTensorProduct(seq[layer], '1x0e+1x1o', seq[min(layer + 1, 3)])
        W, din, dout = tp.weight_numel, im[0] + 3 * im[1] + 3 * im[2] + im[3], om[0] + 3 * om[1] + 3 * om[2] + om[3]
        gen = torch.Generator(device=dev).manual_seed(layer)
        x, sh, w, g = (torch.randn(E, n, device=dev, generator=gen) for n in (din, 4, W, dout))
        # a slice against fp64 autograd of the restatement
        n = 2048
        xs, ss, ws = (t[:n].double().requires_grad_(True) for t in (x, sh, w))
        want = torch.autograd.grad(tp_torch(xs, ss, ws, im, om), (xs, ss, ws), g[:n].double())
        got = ctx.tp_backward(layer, x, sh, w, g)
        err = max(float((a_[:n].double() - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(got, want))
        assert err < 1e-5, (layer, err)
        del got, want, xs, ss, ws
        rd_all, wr_all = 4 * (W + din + dout + 4), 4 * (W + din + 4)
        modes = {'forward': (lambda: ctx.tp_forward(layer, x, sh, w, dout), 4 * (W + din + 4) + 4 * dout),
                 'backward_all': (lambda: ctx.tp_backward(layer, x, sh, w, g, (True, True, True)), rd_all + wr_all),
                 'backward_grad_w': (lambda: ctx.tp_backward(layer, x, sh, None, g, (False, False, True)), 4 * (din + dout + 4) + 4 * W),
                 'backward_grad_x_sh': (lambda: ctx.tp_backward(layer, x, sh, w, g, (True, True, False)), rd_all + 4 * (din + 4))}
        res = {'layer_shape': layer, 'edges': E, 'W': W, 'max_rel_err_vs_fp64': err}
        for name, (fn, nbytes) in modes.items():
            ms = median_ms(fn, a.iters, a.repeats)
            gbps = E * nbytes / ms / 1e6
            res[name] = {'ms': ms, 'bytes_per_edge': nbytes, 'GBps': gbps, 'frac_of_6300': gbps / 6300}
        for name in ('backward_all', 'backward_grad_w', 'backward_grad_x_sh'):
            res[name]['ratio_to_forward_ms'] = res[name]['ms'] / res['forward']['ms']
        # the baseline: torch autograd of the fp32 restatement, forward + backward, with the same inputs asking for a gradient
        Eb = a.baseline_edges or E
        xb, sb, wb, gb = x[:Eb], sh[:Eb], w[:Eb], g[:Eb]

        def torch_step(need):
            ins = [t.detach().requires_grad_(r) for t, r in zip((xb, sb, wb), need)]
            torch.autograd.grad(tp_torch(*ins, im, om), [t for t, r in zip(ins, need) if r], gb)

        base = {}
        for name, need in (('backward_all', (True, True, True)), ('backward_grad_w', (False, False, True)), ('backward_grad_x_sh', (True, True, False))):
            base[name] = median_ms(lambda: torch_step(need), max(1, a.iters // 3), a.repeats) * E / Eb
        with torch.no_grad():
            base['forward'] = median_ms(lambda: tp_torch(xb, sb, wb, im, om), max(1, a.iters // 3), a.repeats) * E / Eb
        res['torch_baseline'] = {'edges': Eb, 'forward_ms': base['forward'], 'forward_plus_backward_ms': {k: v for k, v in base.items() if k != 'forward'}}
        res['speedup_forward_plus_backward'] = {k: base[k] / (res['forward']['ms'] + res[k]['ms']) for k in ('backward_all', 'backward_grad_w', 'backward_grad_x_sh')}
        res['speedup_forward'] = base['forward'] / res['forward']['ms']
        res['faster_than_torch_in_every_mode'] = all(v > 1 for v in res['speedup_forward_plus_backward'].values()) and res['speedup_forward'] > 1
        print(json.dumps(res), flush=True)
        results.append(res)
        del x, sh, w, g, xb, sb, wb, gb
        torch.cuda.empty_cache()
    if a.json:
        json.dump(results, open(a.json, 'w'), indent=1)
    assert all(r['faster_than_torch_in_every_mode'] for r in results), 'a mode is slower than the torch baseline'


def bench_radial():
    from disco_diffdock_amd.tensor_layers import FCBlock, _shape_context, fused_radial_tp
    ctx = _shape_context(0)
    E, results = a.edges, []
    offs = [E * k // 4 for k in range(5)]
    for layer in range(4):
        im, om = MULS[layer], MULS[min(layer + 1, 3)]
        tp = FasterTensorProduct(seq[layer], '1x0e+1x1o', seq[min(layer + 1, 3)])
        W, din, dout = tp.weight_numel, im[0] + 3 * im[1] + 3 * im[2] + im[3], om[0] + 3 * om[1] + 3 * om[2] + om[3]
        torch.manual_seed(layer)
        fc = torch.nn.ModuleList([FCBlock(72, 72, W, 2, 0.0) for _ in range(4)]).to(dev)
        gen = torch.Generator(device=dev).manual_seed(layer)
        x, sh, ea, g = (torch.randn(E, n, device=dev, generator=gen) for n in (din, 4, 72, dout))
        X, SH = x.requires_grad_(True), sh.requires_grad_(True)
        EA = [ea[offs[k]:offs[k + 1]].clone().requires_grad_(True) for k in range(4)]

        def step(fused):
            for t in [X, SH] + EA + list(fc.parameters()):
                t.grad = None
            out = fused_radial_tp(tp, fc, X, SH, EA) if fused else tp(X, SH, torch.cat([fc[k](EA[k]) for k in range(4)]))
            out.backward(g)

        res = {'layer_shape': layer, 'edges': E, 'W': W, 'one_weight_tensor_bytes': 4 * E * W, 'workspace_bytes': ctx.L.ddk_rtp_backward_workspace(layer, E, 4)}
        grads = {}
        for name, fused in (('fused', True), ('unfused', False)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            live = torch.cuda.memory_allocated()
            step(fused)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - live
            grads[name] = [X.grad.clone()] + [p.grad.clone() for p in fc.parameters()]
            res[name] = {'ms': median_ms(lambda: step(fused), a.iters, a.repeats), 'peak_bytes': peak, 'peak_over_one_weight_tensor': peak / (4 * E * W)}
        res['max_rel_diff_of_gradients'] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(grads['fused'], grads['unfused']))
        res['fused_over_unfused_ms'] = res['fused']['ms'] / res['unfused']['ms']
        # the three device passes on their own (no torch around them)
        with torch.no_grad():
            hid = torch.cat([fc[k][:4](EA[k]) for k in range(4)])
            w2, b2 = torch.stack([b[4].weight for b in fc]), torch.stack([b[4].bias for b in fc])
            xd, sd = X.detach(), SH.detach()
            res['kernels_ms'] = {
                'forward': median_ms(lambda: ctx.rtp_forward(layer, xd, sd, hid, offs, w2, b2, dout), a.iters, a.repeats),
                'backward_per_edge': median_ms(lambda: ctx.rtp_backward(layer, xd, sd, hid, offs, w2, b2, g, (True, True, True, False, False)), a.iters, a.repeats),
                'backward_parameters': median_ms(lambda: ctx.rtp_backward(layer, xd, sd, hid, offs, None, None, g, (False, False, False, True, True)), a.iters, a.repeats)}
        print(json.dumps(res), flush=True)
        results.append(res)
        del x, sh, ea, g, X, SH, EA, grads, hid
        torch.cuda.empty_cache()
    if a.json:
        json.dump(results, open(a.json, 'w'), indent=1)


def bench_conv():
    from disco_diffdock_amd.tensor_layers import FCBlock, _shape_context, fused_radial_conv, fused_radial_tp
    ctx = _shape_context(0)
    E, results = a.edges, []
    N = a.nodes or max(1, E // 25)
    offs = [E * k // 4 for k in range(5)]
    for layer in [int(v) for v in a.layers.split(',')]:
        im, om = MULS[min(layer, 3)], MULS[min(layer + 1, 3)]
        tp = FasterTensorProduct(seq[min(layer, 3)], '1x0e+1x1o', seq[min(layer + 1, 3)])
        W, din, dout = tp.weight_numel, im[0] + 3 * im[1] + 3 * im[2] + im[3], om[0] + 3 * om[1] + 3 * om[2] + om[3]
        torch.manual_seed(layer)
        fc = torch.nn.ModuleList([FCBlock(72, 72, W, 2, 0.0) for _ in range(4)]).to(dev)
        gen = torch.Generator(device=dev).manual_seed(layer)
        x, sh, ea, g = (torch.randn(n, c, device=dev, generator=gen) for n, c in ((N, din), (E, 4), (E, 72), (N, dout)))
        ei = torch.randint(0, N, (2, E), device=dev, generator=gen)
        graph = ctx.conv_graph(ei[0], ei[1], N, N)
        count = graph.src_count.clamp(min=1).float()[:, None]
        X, SH = x.requires_grad_(True), sh.requires_grad_(True)
        EA = [ea[offs[k]:offs[k + 1]].clone().requires_grad_(True) for k in range(4)]

        def step(fused):
            for t in [X, SH] + EA + list(fc.parameters()):
                t.grad = None
            if fused:
                out = fused_radial_conv(tp, fc, X, ei, SH, EA, graph=graph)
            else:
                rows = fused_radial_tp(tp, fc, X.index_select(0, ei[1]), SH, EA)
                out = torch.zeros(N, dout, device=dev).index_add_(0, ei[0], rows) / count
            out.backward(g)

        res = {'layer_shape': layer, 'edges': E, 'nodes': N, 'W': W, 'one_row_tensor_bytes': 4 * E * dout,
               'workspace_bytes': {'forward': ctx.L.ddk_rconv_workspace(layer, E, 4, N, N, 0), 'backward': ctx.L.ddk_rconv_workspace(layer, E, 4, N, N, 1)}}
        grads = {}
        for name, fused in (('fused_conv', True), ('composition', False)):
            step(fused)      # (warm-up: the allocator's blocks, the kernels' code objects)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            live = torch.cuda.memory_allocated()
            step(fused)
            torch.cuda.synchronize()
            res[name] = {'peak_bytes': torch.cuda.max_memory_allocated() - live}
            grads[name] = [X.grad.clone(), SH.grad.clone()] + [p.grad.clone() for p in fc.parameters()]
        res['max_rel_diff_of_gradients'] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(grads['fused_conv'], grads['composition']))
        step(True)
        again = [X.grad.clone(), SH.grad.clone()] + [p.grad.clone() for p in fc.parameters()]
        res['fused_conv']['gradients_bit_identical_run_to_run'] = all(torch.equal(u, v) for u, v in zip(again, grads['fused_conv']))
        times = {'fused_conv': [], 'composition': []}
        for _ in range(a.repeats):      # the two paths alternate, so that a drift of the clocks meets both
            for name, fused in (('fused_conv', True), ('composition', False)):
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                for _ in range(a.iters):
                    step(fused)
                en.record()
                torch.cuda.synchronize()
                times[name].append(st.elapsed_time(en) / a.iters)
        for name, t in times.items():
            res[name]['ms'], res[name]['ms_passes'] = sorted(t)[len(t) // 2], t
        res['fused_over_composition_ms'] = res['fused_conv']['ms'] / res['composition']['ms']
        res['fused_over_composition_peak'] = res['fused_conv']['peak_bytes'] / res['composition']['peak_bytes']
        print(json.dumps(res), flush=True)
        results.append(res)
        del x, sh, ea, g, X, SH, EA, grads, again, graph, count
        torch.cuda.empty_cache()
    if a.json:
        json.dump(results, open(a.json, 'w'), indent=1)


def bench_hidden():
    from disco_diffdock_amd.tensor_layers import FCBlock, _shape_context, fused_radial_hidden
    ctx = _shape_context(0)
    E = a.edges
    N = a.nodes or max(1, E // 25)
    offs = [E * k // 4 for k in range(5)]
    torch.manual_seed(0)
    fc = torch.nn.ModuleList([FCBlock(72, 72, 72, 2, a.dropout) for _ in range(4)]).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    x, emb, g = (torch.randn(n, c, device=dev, generator=gen) for n, c in ((N, 48), (E, 24), (E, 72)))
    ei = torch.randint(0, N, (2, E), device=dev, generator=gen)
    graph = ctx.conv_graph(ei[0], ei[1], N, N)
    X, EMB = x.requires_grad_(True), emb.requires_grad_(True)
    first = [p for blk in fc for p in blk[0].parameters()]

    def step(fused, seed=None):
        for t in [X, EMB] + first:
            t.grad = None
        if fused:
            h = fused_radial_hidden(fc, X, EMB, offs, graph, seed=seed)
        else:
            row = torch.cat([EMB, X[ei[0], :24], X[ei[1], :24]], -1)
            h = torch.cat([fc[k][:4](row[offs[k]:offs[k + 1]]) for k in range(4)])
        h.backward(g)

    res = {'edges': E, 'nodes': N, 'dropout': a.dropout, 'one_hidden_tensor_bytes': 4 * E * 72, 'workspace_bytes': ctx.L.ddk_rhid_workspace(E, 4, N)}
    for name, fused in (('fused_hidden', True), ('composition', False)):
        step(fused)      # (warm-up: the allocator's blocks, the kernels' code objects)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        step(fused)
        torch.cuda.synchronize()
        res[name] = {'peak_bytes': torch.cuda.max_memory_allocated() - live}
    step(True, seed=1)
    one = [X.grad.clone(), EMB.grad.clone()] + [p.grad.clone() for p in first]
    step(True, seed=1)
    res['fused_hidden']['gradients_bit_identical_run_to_run'] = all(torch.equal(u, v) for u, v in zip(one, [X.grad, EMB.grad] + [p.grad for p in first]))
    if a.dropout == 0:      # (with dropout the two paths draw different masks)
        step(False)
        two = [X.grad.clone(), EMB.grad.clone()] + [p.grad.clone() for p in first]
        res['max_rel_diff_of_gradients'] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(one, two))
    times = {'fused_hidden': [], 'composition': []}
    for _ in range(a.repeats):      # the two paths alternate, so that a drift of the clocks meets both
        for name, fused in (('fused_hidden', True), ('composition', False)):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(a.iters):
                step(fused)
            en.record()
            torch.cuda.synchronize()
            times[name].append(st.elapsed_time(en) / a.iters)
    for name, t in times.items():
        res[name]['ms'], res[name]['ms_passes'] = sorted(t)[len(t) // 2], t
    res['fused_over_composition_ms'] = res['fused_hidden']['ms'] / res['composition']['ms']
    res['fused_over_composition_peak'] = res['fused_hidden']['peak_bytes'] / res['composition']['peak_bytes']
    # the device passes on their own (no torch around them)
    with torch.no_grad():
        w1, b1 = torch.stack([b[0].weight for b in fc]), torch.stack([b[0].bias for b in fc])
        xs, em = X.detach()[:, :24].contiguous(), EMB.detach()
        h = ctx.rhid_forward(graph, xs, em, offs, w1, b1, a.dropout, 1)
        res['kernels_ms'] = {
            'forward': median_ms(lambda: ctx.rhid_forward(graph, xs, em, offs, w1, b1, a.dropout, 1), a.iters, a.repeats),
            'backward_per_edge_and_node_sums': median_ms(lambda: ctx.rhid_backward(graph, xs, em, h, offs, w1, g, a.dropout, (True, True, False, False)), a.iters, a.repeats),
            'backward_parameters': median_ms(lambda: ctx.rhid_backward(graph, xs, em, h, offs, None, g, a.dropout, (False, False, True, True)), a.iters, a.repeats)}
    print(json.dumps(res), flush=True)
    if a.json:
        json.dump([res], open(a.json, 'w'), indent=1)


def head_tp_torch(head, xe, sh, w):
    """e3nn's FullyConnectedTensorProduct of a score head in plain torch, any dtype (the formulas of oracle/e3nn_lite.py written out per weight block,
    as tests/head_conv_ref.py does in numpy): xe [E, 84] gathered node rows, sh [E, 4], w [E, W] -> [E, 12] (centre) or [E, 48] (torsion)"""
    E = xe.shape[0]
    a_, p_, q_, c_ = xe[:, :24], xe[:, 24:42].reshape(E, 6, 3), xe[:, 42:60].reshape(E, 6, 3), xe[:, 60:]
    s0, v = sh[:, :1, None], sh[:, None, 1:]
    if head == 0:
        s6, s72 = (3.0 / 36.0) ** 0.5 / 3.0 ** 0.5, (3.0 / 36.0) ** 0.5 / 6.0 ** 0.5
        cross = lambda t: torch.cross(t, v.expand_as(t), dim=-1) * s72
        blocks = ((a_[..., None] * v * s6, 0, 0), (p_ * s0 * s6, 48, 0), (cross(p_), 60, 1), (q_ * s0 * s6, 72, 1), (cross(q_), 84, 0), (c_[..., None] * v * s6, 96, 1))
        out = [0, 0]
        for u, off, io in blocks:
            r = u.shape[1]
            out[io] = out[io] + torch.einsum('erk,erc->eck', u, w[:, off:off + 2 * r].reshape(E, r, 2))
        return torch.cat([out[0].reshape(E, 6), out[1].reshape(E, 6)], 1)
    s18 = (1.0 / 6.0) ** 0.5 / 3.0 ** 0.5
    up, uq = (p_ * v).sum(-1) * s18, (q_ * v).sum(-1) * s18
    o0e = torch.einsum('er,erc->ec', up, w[:, :144].reshape(E, 6, 24))
    o0o = torch.einsum('er,erc->ec', uq, w[:, 144:].reshape(E, 6, 24))
    return torch.cat([o0o, o0e], 1)


def bench_heads():
    """forward + backward of both head convs on the shapes of a training batch: ligands of 30 atoms with 8 rotatable bonds each"""
    from disco_diffdock_amd.runtime import head_tp_shape
    from disco_diffdock_amd.tensor_layers import FCBlock, _shape_context, fused_head_conv
    ctx = _shape_context(0)
    results = []
    for n_atoms in (1200, 12000):
        n_lig = n_atoms // 30
        for head, name in ((0, 'centre'), (1, 'torsion')):
            s = head_tp_shape(head)
            K, W, dout = s['K'], s['W'], s['dout']
            gen = torch.Generator(device=dev).manual_seed(head)
            if head == 0:      # one edge per atom, to its ligand
                src, dst, n_out = torch.arange(n_atoms, device=dev) // 30, torch.arange(n_atoms, device=dev), n_lig
            else:      # per bond 20 of its ligand's 30 atoms, ascending
                n_out = 8 * n_lig
                pick = torch.rand(n_out, 30, device=dev, generator=gen).argsort(1)[:, :20].sort(1).values
                src = torch.arange(n_out, device=dev).repeat_interleave(20)
                dst = (pick + 30 * (torch.arange(n_out, device=dev) // 8)[:, None]).reshape(-1)
            E = src.shape[0]
            torch.manual_seed(head)
            fc = FCBlock(K, K, W, 2, 0.0).to(dev)
            x, sh, ea, g = (torch.randn(n, c, device=dev, generator=gen) for n, c in ((n_atoms, 84), (E, 4), (E, K), (n_out, dout)))
            ei = torch.stack([src, dst])
            graph = ctx.conv_graph(src, dst, n_atoms, n_out)
            count = graph.src_count.clamp(min=1).float()[:, None]
            X, EA = x.requires_grad_(True), ea.requires_grad_(True)

            def step(fused):
                for t in [X, EA] + list(fc.parameters()):
                    t.grad = None
                if fused:
                    out = fused_head_conv(head, fc, X, ei, sh, EA, n_out, graph=graph)
                else:
                    rows = head_tp_torch(head, X.index_select(0, dst), sh, fc(EA))
                    out = torch.zeros(n_out, dout, device=dev).index_add_(0, src, rows) / count
                out.backward(g)

            res = {'head': name, 'atoms': n_atoms, 'ligands': n_lig, 'receivers': n_out, 'edges': E, 'W': W, 'K': K,
                   'launches': {'forward': 2, 'backward': 4},
                   'workspace_bytes': {'forward': ctx.L.ddk_hconv_workspace(head, E, n_atoms, n_out, 0), 'backward': ctx.L.ddk_hconv_workspace(head, E, n_atoms, n_out, 1)}}
            grads = {}
            for tag, fused in (('fused', True), ('torch', False)):
                step(fused)
                step(fused)
                torch.cuda.synchronize()
                grads[tag] = [X.grad.clone(), EA.grad.clone()] + [p.grad.clone() for p in fc.parameters()]
            res['max_rel_diff_of_gradients'] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(grads['fused'], grads['torch']))
            step(True)
            again = [X.grad.clone(), EA.grad.clone()] + [p.grad.clone() for p in fc.parameters()]
            res['gradients_bit_identical_run_to_run'] = all(torch.equal(u, v) for u, v in zip(again, grads['fused']))
            times = {'fused': [], 'torch': []}
            for _ in range(a.repeats):      # the two paths alternate, so that a drift of the clocks meets both
                for tag, fused in (('fused', True), ('torch', False)):
                    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    st.record()
                    for _ in range(a.iters):
                        step(fused)
                    en.record()
                    torch.cuda.synchronize()
                    times[tag].append(st.elapsed_time(en) / a.iters)
            for tag, t in times.items():
                res[tag] = {'ms': sorted(t)[len(t) // 2], 'ms_passes': t}
            res['fused_over_torch_ms'] = res['fused']['ms'] / res['torch']['ms']
            with torch.no_grad():      # the device passes on their own (no torch around them)
                hid, w2, b2, xd = fc[:4](EA), fc[4].weight, fc[4].bias, X.detach()
                res['kernels_ms'] = {
                    'forward': median_ms(lambda: ctx.hconv_forward(head, graph, xd, sh, hid, w2, b2), a.iters, a.repeats),
                    'backward_all': median_ms(lambda: ctx.hconv_backward(head, graph, xd, sh, hid, w2, b2, g), a.iters, a.repeats),
                    'backward_per_edge': median_ms(lambda: ctx.hconv_backward(head, graph, xd, sh, hid, w2, b2, g, (True, True, False, False)), a.iters, a.repeats),
                    'backward_parameters': median_ms(lambda: ctx.hconv_backward(head, graph, xd, sh, hid, None, None, g, (False, False, True, True)), a.iters, a.repeats)}
            print(json.dumps(res), flush=True)
            results.append(res)
    if a.json:
        json.dump(results, open(a.json, 'w'), indent=1)


def bench_embed():
    import math
    from disco_diffdock_amd.tensor_layers import GaussianSmearing, _shape_context, fused_edge_embedding
    ctx = _shape_context(0)
    results = []
    for E, K in ((200000, 64), (200000, 68), (800000, 64), (800000, 68)):
        stop = 5.0 if K == 68 else 30.0
        n_a, n_b, T = max(1, E // 25), max(1, E // 25), 16
        torch.manual_seed(0)
        mlp = torch.nn.Sequential(torch.nn.Linear(K, 24), torch.nn.ReLU(), torch.nn.Dropout(a.dropout), torch.nn.Linear(24, 24)).to(dev).train()
        expansion = GaussianSmearing(0.0, stop, 32).to(dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        pos_a, pos_b = (torch.randn(n, 3, device=dev, generator=gen) * (stop / 4) for n in (n_a, n_b))
        ei = torch.stack([torch.randint(0, n_a, (E,), device=dev, generator=gen), torch.randint(0, n_b, (E,), device=dev, generator=gen)])
        sig, sig_index = torch.randn(T, 32, device=dev, generator=gen), torch.randint(0, T, (n_a,), device=dev, generator=gen).to(torch.int32)
        feat = torch.nn.functional.one_hot(torch.randint(0, 4, (E,), device=dev, generator=gen), 4).float() if K == 68 else None
        g = torch.randn(E, 24, device=dev, generator=gen)
        params = list(mlp.parameters())

        def step(fused, seed=None):
            for t in params:
                t.grad = None
            if fused:
                emb, sh = fused_edge_embedding(mlp, expansion, pos_a, pos_b, ei, sig, sig_index, feat=feat, seed=seed)
            else:
                vec = pos_b[ei[1]] - pos_a[ei[0]]
                d = vec.norm(dim=-1)
                row = torch.cat(([feat] if feat is not None else []) + [sig[sig_index.long()[ei[0]]], expansion(d)], 1)
                emb = mlp(row)
                sh = torch.cat([torch.ones_like(d)[:, None], math.sqrt(3.0) * vec / d.clamp_min(1e-12)[:, None]], 1)
            emb.backward(g)
            return sh

        res = {'edges': E, 'K': K, 'dropout': a.dropout, 'outputs_bytes': 4 * E * 28, 'workspace_bytes': ctx.L.ddk_eemb_workspace(E, K)}
        for name, fused in (('fused_embedding', True), ('composition', False)):
            step(fused)      # (warm-up: the allocator's blocks, the kernels' code objects)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            live = torch.cuda.memory_allocated()
            step(fused)
            torch.cuda.synchronize()
            res[name] = {'peak_bytes': torch.cuda.max_memory_allocated() - live}
        step(True, seed=1)
        one = [t.grad.clone() for t in params]
        step(True, seed=1)
        res['fused_embedding']['gradients_bit_identical_run_to_run'] = all(torch.equal(u, t.grad) for u, t in zip(one, params))
        times = {'fused_embedding': [], 'composition': []}
        for _ in range(a.repeats):      # the two paths alternate, so that a drift of the clocks meets both
            for name, fused in (('fused_embedding', True), ('composition', False)):
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                for _ in range(a.iters):
                    step(fused)
                en.record()
                torch.cuda.synchronize()
                times[name].append(st.elapsed_time(en) / a.iters)
        for name, t in times.items():
            res[name]['ms'], res[name]['ms_passes'] = sorted(t)[len(t) // 2], t
        res['fused_over_composition_ms'] = res['fused_embedding']['ms'] / res['composition']['ms']
        res['fused_over_composition_peak'] = res['fused_embedding']['peak_bytes'] / res['composition']['peak_bytes']
        with torch.no_grad():      # the device passes on their own (no torch around them)
            ops = (pos_a, pos_b, ei[0].to(torch.int32), ei[1].to(torch.int32), feat, sig, sig_index, 0.0, stop)
            w = [t.detach() for t in params]
            res['kernels_ms'] = {'forward': median_ms(lambda: ctx.eemb_forward(*ops, *w, a.dropout, 1), a.iters, a.repeats),
                                 'backward': median_ms(lambda: ctx.eemb_backward(*ops, w[0], w[1], w[2], g, a.dropout, 1), a.iters, a.repeats)}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.json:
        json.dump(results, open(a.json, 'w'), indent=1)


def bench_model():
    import numpy as np
    from disco_diffdock_amd import synthetic, train_model
    from disco_diffdock_amd.data import collate, from_arrays
    from disco_diffdock_amd.tensor_layers import conv_stack
    B = 16
    cs = [synthetic.make_complex(100 + k, n_res=150 + 10 * k) for k in range(B)]
    b = collate([from_arrays(c) for c in cs]).to(dev)
    t = torch.linspace(0.1, 0.9, B, device=dev)
    b.complex_t = {k: t.clone() for k in ('tr', 'rot', 'tor')}
    torch.manual_seed(0)
    model = train_model.TrainableScoreModel(sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True,
                                            lm_embedding_type='esm', dropout=a.dropout).to(dev).train()
    lig, rec = b['ligand'], b['receptor']
    ct = {k: v.float() for k, v in b.complex_t.items()}

    def edges():
        return train_model.build_conv_edges(lig.pos, lig.batch, rec.pos, rec.batch, b['ligand', 'ligand'].edge_index, b['receptor', 'receptor'].edge_index, B,
                                            model.lig_max_radius, model._cross_cutoff(ct))

    lig_ei, cross_ei, rec_ei, _ = edges()
    edge_index, sizes = train_model.combine_edges(lig_ei, cross_ei, rec_ei, lig.pos.shape[0])

    def full():
        model.zero_grad(set_to_none=True)
        tr, rot, tor = model(b, seed=1)
        (tr.sum() + rot.sum() + tor.sum()).backward()

    def embed_only():
        model.zero_grad(set_to_none=True)
        l, r = model.embed(b, seed=1)
        (l.sum() + r.sum()).backward()

    res = {'complexes': B, 'ligand_atoms': int(lig.pos.shape[0]), 'residues': int(rec.pos.shape[0]), 'edges': dict(zip(('lig', 'cross', 'rec', 'cross_flipped'), sizes)),
           'dropout': a.dropout, 'parameters': sum(p.numel() for p in model.parameters())}
    full()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    full()
    torch.cuda.synchronize()
    res['peak_bytes_of_a_step'] = torch.cuda.max_memory_allocated() - live
    res['ms'] = {'forward_backward': median_ms(full, a.iters, a.repeats), 'graph_build': median_ms(edges, a.iters, a.repeats),
                 'embed_forward_backward (graph build, embeddings, conv stack)': median_ms(embed_only, a.iters, a.repeats)}
    res['ms']['heads_forward_backward (the difference)'] = res['ms']['forward_backward'] - res['ms']['embed_forward_backward (graph build, embeddings, conv stack)']
    # the edge embeddings and the conv stack on their own, on the batch's graph
    sig = model.timestep_emb_func(ct['tr'])
    feat = torch.cat([b['ligand', 'ligand'].edge_attr.float(), torch.zeros((lig_ei.shape[1] - b['ligand', 'ligand'].edge_attr.shape[0], 4), device=dev)], 0)
    from disco_diffdock_amd.tensor_layers import fused_edge_embedding
    li, ri = lig.batch.to(torch.int32), rec.batch.to(torch.int32)

    def edge_embeddings():
        model.zero_grad(set_to_none=True)
        e0, s0 = fused_edge_embedding(model.lig_edge_embedding, model.lig_distance_expansion, lig.pos, lig.pos, lig_ei, sig, li, feat=feat, seed=1)
        e1, s1 = fused_edge_embedding(model.cross_edge_embedding, model.cross_distance_expansion, lig.pos, rec.pos, cross_ei, sig, li, seed=2)
        e2, s2 = fused_edge_embedding(model.rec_edge_embedding, model.rec_distance_expansion, rec.pos, rec.pos, rec_ei, sig, ri, seed=3)
        (e0.sum() + e1.sum() + e2.sum()).backward()
        return torch.cat([e0, e1, e2, e1]).detach(), torch.cat([s0, s1, s2, s1])

    emb, sh = edge_embeddings()
    x0 = torch.randn(lig.pos.shape[0] + rec.pos.shape[0], 24, device=dev)

    def stack():
        model.zero_grad(set_to_none=True)
        conv_stack(model.conv_layers, x0, edge_index, emb, sizes, sh, seed=1).sum().backward()

    res['ms']['edge_embeddings_forward_backward'] = median_ms(edge_embeddings, a.iters, a.repeats)
    res['ms']['conv_stack_forward_backward'] = median_ms(stack, a.iters, a.repeats)
    print(json.dumps(res), flush=True)
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)


if a.heads:
    bench_heads()
    sys.exit(0)
if a.embed:
    bench_embed()
    sys.exit(0)
if a.model:
    bench_model()
    sys.exit(0)
if a.hidden:
    bench_hidden()
    sys.exit(0)
if a.backward:
    bench_backward()
    sys.exit(0)
if a.conv:
    bench_conv()
    sys.exit(0)
if a.radial:
    bench_radial()
    sys.exit(0)
i_irr, o_irr = seq[min(a.layer, 3)], seq[min(a.layer + 1, 3)]
tp = FasterTensorProduct(i_irr, '1x0e+1x1o', o_irr)
E, W = a.edges, tp.weight_numel
din = {0: 24, 1: 42, 2: 60, 3: 84, 4: 84}[a.layer]
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(E, din, device=dev, generator=g)
sh = torch.randn(E, 4, device=dev, generator=g)
w = torch.randn(E, W, device=dev, generator=g)
out = tp(x, sh, w)
torch.cuda.synchronize()
# fp64 restatement of tensor_layers.py:65-116 on a slice (the committed goldens of the unmodified class are checked by tests/test_gpu_ops.py)
n = 4096
xs, ss, ws = x[:n].double().cpu(), sh[:n].double().cpu(), w[:n].double().cpu()
import re
mul = {k: 0 for k in ('0e', '1o', '1e', '0o')}
for c in i_irr.split('+'):
    m, ir = c.split('x'); mul[ir] = int(m)
omul = {k: 0 for k in ('0e', '1o', '1e', '0o')}
for c in o_irr.split('+'):
    m, ir = c.split('x'); omul[ir] = int(m)
o = 0
A_ = xs[:, o:o + mul['0e']]; o += mul['0e']
P_ = xs[:, o:o + 3 * mul['1o']].reshape(n, -1, 3); o += 3 * mul['1o']
Q_ = xs[:, o:o + 3 * mul['1e']].reshape(n, -1, 3); o += 3 * mul['1e']
C_ = xs[:, o:o + mul['0o']]
s0, v = ss[:, :1], ss[:, 1:]
rows = {
    '0e': torch.cat([A_ * s0, (P_ * v[:, None]).sum(-1) / 3 ** 0.5], 1)[..., None],
    '1o': torch.cat([A_[..., None] * v[:, None], P_ * s0[..., None], torch.cross(Q_, v[:, None].expand_as(Q_), dim=-1) / 2 ** 0.5], 1),
    '1e': torch.cat([torch.cross(P_, v[:, None].expand_as(P_), dim=-1) / 2 ** 0.5, Q_ * s0[..., None], C_[..., None] * v[:, None]], 1),
    '0o': torch.cat([(Q_ * v[:, None]).sum(-1) / 3 ** 0.5, C_ * s0], 1)[..., None],
}
ref, off = [], 0
for k in ('0e', '1o', '1e', '0o'):
    n_in, n_out = rows[k].shape[1], omul[k]
    if n_out == 0:
        continue
    wk = ws[:, off:off + n_in * n_out].reshape(n, n_in, n_out); off += n_in * n_out
    if n_in:
        ref.append((torch.einsum('eic,eio->eoc', rows[k], wk) / n_in ** 0.5).reshape(n, -1))
ref = torch.cat(ref, 1)
err = float((out[:n].double().cpu() - ref).abs().max() / ref.abs().max())
assert off == W and err < 1e-5, (off, W, err)
st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(2):
    tp(x, sh, w)
torch.cuda.synchronize()
st.record()
for _ in range(a.iters):
    tp(x, sh, w)
en.record()
torch.cuda.synchronize()
ms = st.elapsed_time(en) / a.iters
bytes_per_edge = 4 * (W + din + 4) + 8 + 4 * out.shape[1]      # SURVEY.md 8(d) boundary (A) (incl. the two int32 indices of the gather the reference does first)
moved = 4 * (W + din + 4) + 4 * out.shape[1]                   # what this entry point really reads / writes (x_dst arrives gathered)
res = {'layer': a.layer, 'edges': E, 'W': W, 'ms_per_call': ms, 'algorithmic_bytes_per_edge': bytes_per_edge, 'bytes_moved_per_edge': moved,
       'achieved_GBps_algorithmic': E * bytes_per_edge / ms / 1e6, 'frac_of_8000': E * bytes_per_edge / ms / 1e6 / 8000, 'frac_of_6300': E * bytes_per_edge / ms / 1e6 / 6300,
       'Medges_per_s': E / ms / 1e3, 'max_rel_err_vs_fp64': err}
print(json.dumps(res))
if a.json:
    json.dump(res, open(a.json, 'w'), indent=1)
