#!/usr/bin/env python
"""Generate tests/golden/node_stage_bits.json: the SHA-256 of the raw bytes of the output of ddk_conv_forward on the three shapes in which it launches the
plain node finalize (node_finalize_kernel: scatter-mean divisor, BatchNorm, residual): a row stride of dout with the residual, no residual with a
BatchNorm offset (one conv of an all-atom layer), and dout = 0 (no edges: the residual alone, BatchNorm skipped).

Like make_golden_pose_bits.py this needs no reference checkout: it EXECUTES THE DEVICE ENTRY POINT on a MI355X, at a commit whose arithmetic is known to
be good, and records what it gives.  tests/test_gpu_node_stage_bits.py recomputes the same outputs with ``digests`` below and compares, so a finalize
expression that the compiler contracts differently shows as a changed digest where the fp64 tests see nothing.  Every case is computed twice; the
generator refuses to write a file if an output is not identical run to run.

    python tests/golden/make_golden_node_stage_bits.py [--commit HASH]

THE CASES.  The conv launch in front of the finalize accumulates with atomics, so the graphs are built for the order of additions not to matter: the
edges of a group fit one 32-edge tile (a receiver's messages of a group are summed inside the tile, in edge order) and no node receives in more than
two groups (two additions onto a zeroed accumulator commute exactly).  Every context names its conv_kernel and deterministic: the file means the same
under DDK_CONV_KERNEL / DDK_DETERMINISTIC.
    score.k{0,1}.l{0,3}    score-model context with conv_kernel 0 (two f16 limbs) and 1 (fp32 MFMA), layers 0 and 3: N = 5, group offsets [0, 2, 3, 5, 6],
                           receivers [0, 1 | 1 | 2, 2 | 3] (sorted per group; node 1 receives in two groups, node 2 twice in one, node 4 nothing:
                           the divisor max(deg, 1)), random weights with BatchNorm (oracle.score_model_ref.random_conv_layer_params)
    score.k{0,1}.l3.empty  layer 3, N = 3, offsets [0, 0, 0, 0, 0]: out = the input rows, BatchNorm skipped
    all_atom.l0.conv4      all-atom context, conv index 9 * 0 + 4: N = 5, E = 6 in one group, offsets [0, 6, 6, 6, 6], receivers [0, 0, 1, 2, 2, 2]: no
                           residual, the fifth BatchNorm of the layer
"""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, 'node_stage_bits.json')

SCORE_OFFSETS = [0, 2, 3, 5, 6]
SCORE_RECEIVERS = [0, 1, 1, 2, 2, 3]
ATOM_RECEIVERS = [0, 0, 1, 2, 2, 2]
CASES = tuple(f'score.k{k}.l{l}' for k in (0, 1) for l in (0, 3)) + tuple(f'score.k{k}.l3.empty' for k in (0, 1)) + ('all_atom.l0.conv4',)


def _edges(g, N, receivers, attr_dim=72):
    E = len(receivers)
    return (torch.tensor(receivers, dtype=torch.int32), torch.randint(0, N, (E,), generator=g).int(), torch.randn(E, attr_dim, generator=g),
            torch.randn(E, 4, generator=g))


def _score(dev, kernel):
    from oracle import score_model_ref as smr
    from disco_diffdock_amd.runtime import Context
    cfg = smr.ScoreModelConfig()
    out = []
    for l in (0, 3):
        i_irr, o_irr = cfg.conv_irreps(l)
        ctx = Context(device=0, conv_kernel=kernel, deterministic=0)
        ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in smr.random_conv_layer_params(cfg, l, 40 + l, True).items()})
        din, dout = smr.irreps_dim(i_irr), smr.irreps_dim(o_irr)
        g = torch.Generator().manual_seed(100 + l)
        src, dst, ea, sh = _edges(g, 5, SCORE_RECEIVERS)
        node = torch.randn(5, din, generator=g)
        out.append((f'score.k{kernel}.l{l}', ctx.conv_forward(l, node.to(dev), src.to(dev), dst.to(dev), SCORE_OFFSETS, ea.to(dev), sh.to(dev), dout)))
        if l == 3:
            node = torch.randn(3, din, generator=g)
            e = torch.zeros(0, dtype=torch.int32, device=dev)
            out.append((f'score.k{kernel}.l3.empty', ctx.conv_forward(l, node.to(dev), e, e, [0, 0, 0, 0, 0], torch.zeros(0, 72, device=dev),
                                                                      torch.zeros(0, 4, device=dev), dout)))
    return out


def _all_atom(dev):
    from oracle import confidence_ref as cr, score_model_ref as smr
    from disco_diffdock_amd.runtime import Context
    cfg = cr.ConfidenceModelConfig()
    ctx = Context(device=0, all_atoms=1, embedding_scale=10000.0, num_confidence_outputs=2, conv_kernel=0, deterministic=0)
    ctx.load_state_dict({k: v for k, v in cr.random_state_dict(cfg, seed=60).items() if k.startswith('conv_layers.')})
    i_irr, o_irr = cfg.conv_irreps(0)
    g = torch.Generator().manual_seed(200)
    src, dst, ea, sh = _edges(g, 5, ATOM_RECEIVERS)
    node = torch.randn(5, smr.irreps_dim(i_irr), generator=g)
    return [('all_atom.l0.conv4', ctx.conv_forward(9 * 0 + 4, node.to(dev), src.to(dev), dst.to(dev), [0, 6, 6, 6, 6], ea.to(dev), sh.to(dev),
                                                   smr.irreps_dim(o_irr)))]


def digests(dev):
    out = _score(dev, 0) + _score(dev, 1) + _all_atom(dev)
    torch.cuda.synchronize()
    d = {}
    for name, t in out:
        assert name not in d and t.dtype == torch.float32 and bool(torch.isfinite(t).all()), name
        d[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit the file is generated at (recorded in the file)')
    ap.add_argument('--out', default=PATH)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the digests come from the device entry point: a MI355X is needed'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    dev = torch.device('cuda:0')
    d, again = digests(dev), digests(dev)
    unstable = [k for k in d if d[k] != again[k]]
    assert not unstable, f'not identical run to run: {unstable}'
    with open(a.out, 'w') as f:
        json.dump({'generated_at_commit': a.commit, 'hip': torch.version.hip, 'sha256': d}, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{a.out}: {len(d)} digests')


if __name__ == '__main__':
    main()
