#!/usr/bin/env python
"""Generate tests/golden/latent_choice_bits.json: the SHA-256 of the raw bytes of every output of the latent-choice ops (the ragged Gumbel softmax and its
backward, the per-sample Gumbel pick, the ragged node cross-entropy and its backward) on the smallest shapes that reach every piece they share in
csrc/k_ragged.h: the pointer-pair rule, the position-to-row map, the quad walk and the three halving trees.

Like make_golden_train_ops_bits.py this needs no reference checkout: it EXECUTES THE DEVICE OPS through ``Context`` on a MI355X, at a commit whose
arithmetic is known to be good, and records what they give.  tests/test_gpu_latent_choice_bits.py recomputes the same outputs with ``digests`` below and
compares, so a changed order of additions, a changed first-of-equals rule or a graph that is no longer left alone shows as a changed digest.  Every
output is computed twice here; one that differs between the two runs is listed under ``unstable`` and not pinned.

    python tests/golden/make_golden_latent_choice_bits.py [--commit HASH]

THE CASES.  The six graphs of adversarial_latent.gumbel_case('two_trips'): (300, 1500), (0, 1025), (1, 0), (0, 0), (1024, 0), (3, 6) ligand and receptor
nodes - 1025 leaves one position alone in thread 0's second quad, 1024 fills every thread exactly once, 1 and 9 leave most threads idle, graphs 1 and 3
have no ligand nodes, graphs 2, 3 and 4 no receptor nodes.
    gumbel       D = 1 and 4, T = 1 and 0.01, (sample, draw) = (0, 0) and (3, 2): out, y and grad_logit on both sides.  At D = 4, T = 1, (3, 2) also:
                 ``descending``: graph 2's ligand pair is (1327, 0) - the ligand table holds the rows of graphs 3 .. 5 first, so that no row belongs to two
                 graphs; ``past_end``: the last ligand pointer is n_lig + 1.  Both into outputs filled with 7.0: the graph left alone shows in the digest;
                 ``nan``: column 1 of the logits is NaN;  ``flat``: gumbel_case('flat'), the all-way tie through the whole tree
    pick         B = 3, sample0 = 5 on a (6, 7) graph and on the (0, 1025) graph, D = 1 and 4, both temperatures: lig_latent, rec_latent, choices; and the
                 (6, 7) graph at D = 4 with a NaN column, whose choice is -1
    node_ce      D = 1 and 4, soft = 0 and 1, column[g] = g % D: loss, pick, target, saved and grad_logit on both sides.  The student ties at its
                 maximum at positions 10 and 1700 of graph 0 and the teacher at 0 and 1024 of graph 1 (the lowest wins).  ``neginf`` (D = 4): every logit
                 of the 9-node graph is -inf (position 0);  ``bad`` (D = 4, soft = 0): graph 0's column is D and the last receptor pointer is n_rec + 1,
                 into outputs filled with -7
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
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, 'latent_choice_bits.json')

SEED = 0x1A7E27C401CE
TEMPERATURES = ((1.0, 'T1'), (0.01, 'T1e-2'))
DRAWS = ((0, 0), (3, 2))
OPS = ('gumbel', 'pick', 'node_ce')


def _ptrs(graphs):
    return (np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64),
            np.concatenate([[0], np.cumsum([g[1] for g in graphs])]).astype(np.int64))


def _sides(per, graphs, order_l=None):
    """per graph [n, ...] arrays -> (ligand table, receptor table); ``order_l``: the order of the graphs' blocks in the ligand table"""
    order_l = range(len(graphs)) if order_l is None else order_l
    return (np.concatenate([per[g][:graphs[g][0]] for g in order_l]), np.concatenate([a[nl:] for a, (nl, _) in zip(per, graphs)]))


def outputs(ctx, dev):
    """every (name, device tensor) of every case, in a fixed order"""
    import adversarial_latent as al
    from disco_diffdock_amd.runtime import _ptr, _stream, stream_id
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = []

    def named(tag, names, tensors):
        out.extend((f'{tag}.{n}', t) for n, t in zip(names, tensors))

    def gumbel_into(l, r, lp, rp, T, st, sample, draw, g_l, g_r):
        """the two C entries on outputs filled with 7.0 (Context's wrappers allocate theirs)"""
        D, G = l.shape[1], lp.shape[0] - 1
        st = put(np.asarray(st, np.uint64).view(np.int64))
        y_l, y_r, o_l, o_r, d_l, d_r = (torch.full_like(t, 7.0) for t in (l, r, l, r, l, r))
        ctx._check(ctx.L.ddk_gumbel_softmax_batch(ctx.h, G, D, _ptr(l), l.shape[0], _ptr(r), r.shape[0], _ptr(lp), _ptr(rp), T, SEED, _ptr(st), sample, draw,
                                                  _ptr(y_l), _ptr(y_r), _ptr(o_l), _ptr(o_r), _stream()), 'ddk_gumbel_softmax_batch')
        ctx._check(ctx.L.ddk_gumbel_softmax_batch_backward(ctx.h, G, D, _ptr(y_l), l.shape[0], _ptr(y_r), r.shape[0], _ptr(lp), _ptr(rp), T, _ptr(g_l),
                                                           _ptr(g_r), _ptr(d_l), _ptr(d_r), _stream()), 'ddk_gumbel_softmax_batch_backward')
        return o_l, o_r, y_l, y_r, d_l, d_r

    GUMBEL_OUT = ('out_l', 'out_r', 'y_l', 'y_r', 'grad_logit_l', 'grad_logit_r')

    def gumbel(tag, l, r, lp, rp, T, st, sample, draw, g_l, g_r):
        o_l, o_r, y_l, y_r = ctx.gumbel_softmax(l, r, lp, rp, T, SEED, st, sample=sample, draw=draw)
        named(tag, GUMBEL_OUT, (o_l, o_r, y_l, y_r, *ctx.gumbel_softmax_backward(y_l, y_r, lp, rp, T, g_l, g_r)))

    # ---- the ragged Gumbel softmax ----
    for D in (1, 4):
        case = al.gumbel_case('two_trips', D)
        graphs, st = case['graphs'], case['streams']
        assert [sum(g) for g in graphs] == [1800, 1025, 1, 0, 1024, 9]
        assert any(nl == 0 and nr > 0 for nl, nr in graphs) and any(nr == 0 and nl > 0 for nl, nr in graphs)
        (l, r), (g_l, g_r) = (tuple(put(a) for a in _sides(case[k], graphs)) for k in ('logits', 'grads'))
        lp, rp = (put(a) for a in _ptrs(graphs))
        for T, tt in TEMPERATURES:
            for sample, draw in DRAWS:
                gumbel(f'gumbel.two_trips_D{D}_{tt}_s{sample}d{draw}', l, r, lp, rp, T, st, sample, draw, g_l, g_r)
        if D == 4:
            # graph 2's ligand pair descends: the ligand table holds the blocks of graphs 3, 4, 5, then 0, (1), then 2, so that no row has two owners
            order = (3, 4, 5, 0, 1, 2)
            (bl, _), (bg, _) = (_sides(case[k], graphs, order) for k in ('logits', 'grads'))
            bad = np.asarray([1027, 1327, 1327, 0, 0, 1024, 1027], np.int64)
            assert bl.shape[0] == 1328 and bad[2] > bad[3]
            named('gumbel.descending', GUMBEL_OUT, gumbel_into(put(bl), r, put(bad), rp, 1.0, st, 3, 2, put(bg), g_r))
            bad = _ptrs(graphs)[0]
            bad[-1] = l.shape[0] + 1
            named('gumbel.past_end', GUMBEL_OUT, gumbel_into(l, r, put(bad), rp, 1.0, st, 3, 2, g_l, g_r))
            nl, nr = l.clone(), r.clone()
            nl[:, 1], nr[:, 1] = float('nan'), float('nan')
            gumbel('gumbel.nan', nl, nr, lp, rp, 1.0, st, 3, 2, g_l, g_r)
    case = al.gumbel_case('flat', 4)
    graphs = case['graphs']
    (l, r), (g_l, g_r) = (tuple(put(a) for a in _sides(case[k], graphs)) for k in ('logits', 'grads'))
    lp, rp = (put(a) for a in _ptrs(graphs))
    gumbel('gumbel.flat', l, r, lp, rp, case['T'], case['streams'], 3, 2, g_l, g_r)

    # ---- B samples of one complex ----
    stream = stream_id('latent_choice_bits')
    PICK_OUT = ('lig_latent', 'rec_latent', 'choices')
    for n_l, n_r in ((6, 7), (0, 1025)):
        logits = np.random.default_rng(SEED % 1000 + n_l + n_r).standard_normal((n_l + n_r, 4)).astype(np.float32)
        for D in (1, 4):
            l, r = put(logits[:n_l, :D]), put(logits[n_l:, :D])
            for T, tt in TEMPERATURES:
                named(f'pick.n{n_l}_{n_r}_D{D}_{tt}', PICK_OUT, ctx.gumbel_pick_samples(l, r, 3, T, SEED, stream, sample0=5, draw=2))
        if n_l:
            l, r = l.clone(), r.clone()
            l[:, 1], r[:, 1] = float('nan'), float('nan')
            res = ctx.gumbel_pick_samples(l, r, 3, 1.0, SEED, stream, sample0=5, draw=2)
            assert res[2][:, 1].tolist() == [-1, -1, -1]
            named('pick.nan', PICK_OUT, res)

    # ---- the ragged node cross-entropy ----
    graphs = al.TWO_TRIPS
    G = len(graphs)
    lp, rp = _ptrs(graphs)
    NCE_OUT = ('loss', 'pick', 'target', 'saved', 'grad_logit_l', 'grad_logit_r')
    for D in (1, 4):
        rng = np.random.default_rng(SEED % 1000 + 50 + D)
        s = [(3 * rng.standard_normal(sum(g))).astype(np.float32) for g in graphs]
        t = [(2 * rng.standard_normal((sum(g), D))).astype(np.float32) for g in graphs]
        col = np.arange(G, dtype=np.int32) % D
        s[0][[10, 1700]] = s[0].max() + np.float32(1.0)
        t[1][[0, 1024], col[1]] = t[1][:, col[1]].max() + np.float32(1.0)
        grad = put(rng.standard_normal(G).astype(np.float32))

        def run(tag, s, t, col, soft, lp=lp, rp=rp, fill=False):
            (s_l, s_r), (t_l, t_r) = (tuple(put(a) for a in _sides(per, graphs)) for per in (s, t))
            ops = (s_l, s_r, put(lp), put(rp), t_l, t_r, put(col))
            o = o_g = None
            if fill:
                o = (torch.full((G,), -7.0, device=dev), torch.full((G,), -7, dtype=torch.int64, device=dev), torch.full((G,), -7, dtype=torch.int64, device=dev),
                     torch.full((G, 2), -7.0, dtype=torch.float64, device=dev))
                o_g = (torch.full_like(s_l, -7.0), torch.full_like(s_r, -7.0))
            loss, pick, target, saved = ctx.node_cross_entropy(*ops, soft, out=o)
            named(tag, NCE_OUT, (loss, pick, target, saved, *ctx.node_cross_entropy_backward(grad, *ops, target, saved, soft, out=o_g)))
            return pick, target

        for soft in (0, 1):
            pick, target = run(f'node_ce.two_trips_D{D}_soft{soft}', s, t, col, soft)
            assert pick[0].item() == 10 and target[1].item() == 0, (pick, target)
        if D == 4:
            s_inf, t_inf = [a.copy() for a in s], [a.copy() for a in t]
            s_inf[5][:], t_inf[5][:] = -np.inf, -np.inf
            for soft in (0, 1):
                pick, target = run(f'node_ce.neginf_soft{soft}', s_inf, t_inf, col, soft)
                assert pick[5].item() == 0 and target[5].item() == 0, (pick, target)
            col_bad, rp_bad = col.copy(), rp.copy()
            col_bad[0], rp_bad[-1] = D, rp[-1] + 1
            pick, _ = run('node_ce.bad', s, t, col_bad, 0, rp=rp_bad, fill=True)
            assert pick[0].item() == -7 and pick[5].item() == -7 and pick[1].item() >= 0, pick
    torch.cuda.synchronize()
    return out


def digests(ctx, dev):
    d = {}
    for name, t in outputs(ctx, dev):
        assert name not in d, name
        d[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit the file is generated at (recorded in the file)')
    ap.add_argument('--out', default=PATH)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the digests come from the device ops: a MI355X is needed'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    ctx, dev = _shape_context(0), torch.device('cuda:0')
    first, again = digests(ctx, dev), digests(ctx, dev)
    unstable = sorted(k for k in first if first[k] != again[k])
    d = {k: v for k, v in first.items() if k not in unstable}
    with open(a.out, 'w') as f:
        json.dump({'generated_at_commit': a.commit, 'hip': torch.version.hip, 'sha256': d, 'unstable': unstable}, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{a.out}: {len(d)} digests, {len(unstable)} unstable: {unstable}')


if __name__ == '__main__':
    main()
