#!/usr/bin/env python
"""Generate tests/golden/train_ops_bits.json: the SHA-256 of the raw bytes of every output of the training ops (the radial tensor product, the radial
conv, the radial hidden layer, the head convs, the edge embedding and the segmented sum) on the smallest shapes that reach every piece they share: the
group table, the slice reduction and the fixed-order segmented sum.

Unlike the other make_golden_*.py this needs no reference checkout: it EXECUTES THE DEVICE OPS through ``Context`` on a MI355X, at a commit whose
arithmetic is known to be good, and records what they give.  tests/test_gpu_train_ops_bits.py recomputes the same outputs with ``outputs`` below and
compares the digests, so a changed order of additions in a parameter gradient or a node sum shows as a changed digest where the fp64 tests at 1e-5
see nothing.  Inputs come from numpy.random.default_rng with fixed seeds.

    python tests/golden/make_golden_train_ops_bits.py [--commit HASH]

THE CASES.  rtp_slice_len is 512 for these sizes.
    groups   offsets [0, 0, 5, 650, 1300]: an empty group, a group that is one short tail, two groups of two slices each (512 + 133 and 512 + 138);
             and one group with E = 1
    graph    41 nodes; on each side the degrees include 0, 1, 4, 5 and hubs of more than 9 edges: the segmented kernel's first element, its block of
             four and its tail
    rtp, rconv     layers 0 and 3 on both group tables, forward and all five gradients
    rhid           both group tables, p = 0 and p = 0.25, forward and all four gradients
    hconv          the centre head with E = 1300 onto 3 receivers; the torsion head with E = 700 onto 17 receivers, one of them without edges
    eemb           E = 1300, F = 0 and F = 4, p = 0 and p = 0.25, forward and all four gradients
    eemb, latent   the same edges and operands with a last node on either side that has no edge, unc_a / uemb given: L = 1 with F = 0 and L = 4 with
                   F = 4, each at p = 0 and p = 0.25, and zero_latent with L = 2 (F = 0, p = 0.25); forward and all seven gradients
    seg_sum        D = 1 and D = 128 (column 0 of the latter is all -0: the first row starts the sum, so -0 stays -0)
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, 'train_ops_bits.json')

N_NODES = 41
GROUPS = {'g4': [0, 0, 5, 650, 1300], 'g1': [0, 1]}
SEED = 0x5EED0B175


def _edges(rng, E, n, special):
    """E node ids below n: ``special`` maps a node to its exact degree (0 included), every other node shares the rest"""
    fixed = [v for v, d in special.items() for _ in range(d)]
    others = np.array([v for v in range(n) if v not in special])
    idx = np.concatenate([np.array(fixed, dtype=np.int64), others[rng.integers(0, len(others), E - len(fixed))]])
    return rng.permutation(idx)


def graph_edges(E, n_in=N_NODES, n_out=N_NODES, seed=1):
    """(src [E] below n_out, dst [E] below n_in): a side of at least 8 nodes has nodes of degree 0, 1, 4 and 5, either side has a hub (64 edges or more)"""
    rng = np.random.default_rng(seed)
    if E < 64:
        return rng.integers(0, n_out, E), rng.integers(0, n_in, E)
    sp = lambda n: {} if n < 8 else {0: 0, 1: 1, 2: 4, 3: 5}
    src, dst = _edges(rng, E, n_out, sp(n_out)), _edges(rng, E, n_in, {n_in - 1 - v: d for v, d in sp(n_in).items()})
    for idx, n in ((src, n_out), (dst, n_in)):
        deg = np.bincount(idx, minlength=n)
        assert deg.max() >= 9 and (n < 8 or {0, 1, 4, 5} <= set(deg.tolist())), deg
    return src, dst


def outputs(ctx, dev):
    """every (name, device tensor) of every case, in a fixed order"""
    from disco_diffdock_amd.runtime import HEAD_CENTER, HEAD_TORSION, head_tp_shape, tp_layer_shape

    def rnd(seed):
        rng = np.random.default_rng(seed)
        return lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)

    def named(tag, names, tensors):
        return [(f'{tag}.{n}', t) for n, t in zip(names, tensors)]

    out = []
    graphs = {}
    for gname, offs in GROUPS.items():
        E = offs[-1]
        src, dst = graph_edges(E)
        graphs[gname] = graph = ctx.conv_graph(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), N_NODES, N_NODES)
        G = len(offs) - 1
        for layer in (0, 3):
            s = tp_layer_shape(layer)
            f = rnd(SEED + 100 * layer + G)
            x, xn, sh, h = f(E, s['din']), f(N_NODES, s['din']), f(E, 4), torch.relu(f(E, 72))
            w2, b2 = f(G, s['W'], 72) / 8, f(G, s['W'])
            g, gn = f(E, s['dout']), f(N_NODES, s['dout'])
            tag = f'rtp.l{layer}.{gname}'
            out += [(tag + '.out', ctx.rtp_forward(layer, x, sh, h, offs, w2, b2, s['dout']))]
            out += named(tag, ('grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'), ctx.rtp_backward(layer, x, sh, h, offs, w2, b2, g))
            tag = f'rconv.l{layer}.{gname}'
            out += [(tag + '.out', ctx.rconv_forward(layer, graph, xn, sh, h, offs, w2, b2))]
            out += named(tag, ('grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'), ctx.rconv_backward(layer, graph, xn, sh, h, offs, w2, b2, gn))
        for p in (0.0, 0.25):
            f = rnd(SEED + 1000 + G)
            xs, emb, w1, b1, gh = f(N_NODES, 24), f(E, 24), f(G, 72, 72) / 8, f(G, 72), f(E, 72)
            tag = f'rhid.p{p}.{gname}'
            h = ctx.rhid_forward(graph, xs, emb, offs, w1, b1, p, 0xC0FFEE)
            out += [(tag + '.h', h)]
            out += named(tag, ('grad_xs', 'grad_emb', 'grad_w1', 'grad_b1'), ctx.rhid_backward(graph, xs, emb, h, offs, w1, gh, p))

    for head, E, n_out in ((HEAD_CENTER, 1300, 3), (HEAD_TORSION, 700, 17)):
        s = head_tp_shape(head)
        src, dst = graph_edges(E, N_NODES, n_out, seed=2 + head)
        graph = ctx.conv_graph(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), N_NODES, n_out)
        f = rnd(SEED + 2000 + head)
        x, sh, h, w2, b2, g = f(N_NODES, s['din']), f(E, 4), torch.relu(f(E, s['K'])), f(s['W'], s['K']) / 8, f(s['W']), f(n_out, s['dout'])
        tag = f'hconv.head{head}'
        out += [(tag + '.out', ctx.hconv_forward(head, graph, x, sh, h, w2, b2))]
        out += named(tag, ('grad_x', 'grad_h', 'grad_w2', 'grad_b2'), ctx.hconv_backward(head, graph, x, sh, h, w2, b2, g))

    E, n_a, n_b, T = 1300, 7, 11, 3
    for F, (start, stop) in ((0, (0.0, 30.0)), (4, (0.0, 5.0))):
        rng = np.random.default_rng(SEED + 3000 + F)
        f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
        i32 = lambda hi, n: torch.from_numpy(rng.integers(0, hi, n).astype(np.int32)).to(dev)
        pos_a, pos_b, idx_a, idx_b = f(n_a, 3) * (stop / 4), f(n_b, 3) * (stop / 4), i32(n_a, E), i32(n_b, E)
        feat = torch.from_numpy(np.eye(4, dtype=np.float32)[rng.integers(0, 4, E)]).to(dev) if F else None
        sig, sig_index = f(T, 32), i32(T, n_a)
        K = F + 64
        w1, b1, w2, b2, g = f(24, K) / 8, f(24) / 2, f(24, 24) / 5, f(24), f(E, 24)
        for p in (0.0, 0.25):
            tag = f'eemb.F{F}.p{p}'
            ops = (pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop)
            out += named(tag, ('emb', 'sh'), ctx.eemb_forward(*ops, w1, b1, w2, b2, p, 0xBEEF))
            out += named(tag, ('grad_w1', 'grad_b1', 'grad_w2', 'grad_b2'), ctx.eemb_backward(*ops, w1, b1, w2, g, p, 0xBEEF))
        # the latent op on the same edges (drawn behind everything above, which keeps its bits).  Either node table gains a last node that no edge names
        pos_a, pos_b, sig_index = torch.cat([pos_a, f(1, 3)]), torch.cat([pos_b, f(1, 3)]), torch.cat([sig_index, i32(T, 1)])
        graph = ctx.conv_graph(idx_a, idx_b, n_b + 1, n_a + 1)
        assert int(graph.src_ptr[-1] - graph.src_ptr[-2]) == 0 and int(graph.dst_ptr[-1] - graph.dst_ptr[-2]) == 0
        unc_a, uemb = torch.from_numpy((rng.random(n_a + 1) < 0.5).astype(np.float32)).to(dev), f(24)
        ops = (pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop)
        for L, zero, ps in ((1 if F == 0 else 4, False, (0.0, 0.25)),) + (((2, True, (0.25,)),) if F == 0 else ()):
            w1l, lat_a, lat_b = torch.cat([w1, f(24, 2 * L) / 8], 1), f(n_a + 1, L), f(n_b + 1, L)
            for p in ps:
                tag = f'eemb.F{F}.L{L}.p{p}' + ('.zero_latent' if zero else '')
                out += named(tag, ('emb', 'sh'), ctx.eemb_latent_forward(*ops, w1l, b1, w2, b2, lat_a, lat_b, zero, unc_a, uemb, p, 0xBEEF))
                out += named(tag, ('grad_w1', 'grad_b1', 'grad_w2', 'grad_b2', 'grad_uemb', 'grad_lat_a', 'grad_lat_b'),
                             ctx.eemb_latent_backward(*ops, w1l, b1, w2, lat_a, lat_b, g, zero, unc_a, uemb, p, 0xBEEF, graph))

    graph = graphs['g4']
    for D in (1, 128):
        rows = rnd(SEED + 4000 + D)(graph.E, D)
        if D > 1:
            rows[:, 0] = -0.0
        out += [(f'seg_sum.D{D}.src', ctx.seg_sum(rows, graph.src_order, graph.src_ptr)), (f'seg_sum.D{D}.dst', ctx.seg_sum(rows, graph.dst_order, graph.dst_ptr))]
    torch.cuda.synchronize()
    return out


def digests(ctx, dev):
    d = {}
    for name, t in outputs(ctx, dev):
        assert name not in d and t.dtype == torch.float32, name
        d[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit the file is generated at (recorded in the file)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the digests come from the device ops: a MI355X is needed'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    d = digests(_shape_context(0), torch.device('cuda:0'))
    earlier = []      # where the file was generated before: kept, oldest first
    if os.path.exists(PATH):
        with open(PATH) as f:
            old = json.load(f)
        earlier = old.get('earlier', []) + [{k: old[k] for k in ('generated_at_commit', 'hip')}]
    with open(PATH, 'w') as f:
        json.dump({'generated_at_commit': a.commit, 'hip': torch.version.hip, 'earlier': earlier, 'sha256': d}, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{PATH}: {len(d)} digests')


if __name__ == '__main__':
    main()
