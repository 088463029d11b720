"""Time the edge embedding with latent columns (tensor_layers.fused_edge_embedding(latent_a=..., latent_b=...), forward + backward with every gradient: the
four MLP parameters, the unconditional row and the latent table) against the torch composition it replaces (two index_selects of the latent table, the cat,
the nn.Sequential, the unconditional add; the geometry columns are handed to it ready-made and are not timed), and the plain op on its own.

    python tools/time_latent_embedding.py latent [--out PATH]            both sides at E = 200 000 and 800 000, time and peak memory, in one process
    python tools/time_latent_embedding.py plain [--root DIR] [--out PATH]  the plain op (no latent operands) from the package under DIR (default: this
                                                                          tree): run it for two trees alternately on one card to compare two builds

Device events around REPS forward + backward steps after WARMUP steps; the median of ROUNDS such windows and their spread.  Peak memory: torch's allocator
high-water mark over one step, above what is held before it (operands and parameters).  Run on the GPU box."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('mode', choices=('latent', 'plain'))
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out', default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from disco_diffdock_amd.tensor_layers import GaussianSmearing, fused_edge_embedding   # noqa: E402

SIZES, N_NODES, T, L, F = (200_000, 800_000), 20_000, 16, 2, 4
WARMUP, REPS, ROUNDS = 5, 20, 5
dev = torch.device('cuda', 0)


def operands(E, seed=1):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    pos = f(N_NODES, 3) * 8
    ei = torch.from_numpy(rng.integers(0, N_NODES, (2, E))).to(dev)
    return dict(pos=pos, ei=ei, sig=f(T, 32), sig_index=torch.from_numpy(rng.integers(0, T, N_NODES).astype(np.int32)).to(dev),
                feat=torch.from_numpy(np.eye(4, dtype=np.float32)[rng.integers(0, 4, E)]).to(dev), gemb=f(E, 24), lat=f(N_NODES, L),
                unc=torch.from_numpy((rng.random(N_NODES) < 0.1).astype(np.float32)).to(dev))


def window(step):
    """median and spread (ms per step) of ROUNDS windows of REPS steps, and the peak bytes of one step above the standing allocation"""
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), peak_mib=peak / 2 ** 20)


def mlp(K):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(K, 24), torch.nn.ReLU(), torch.nn.Dropout(0.1), torch.nn.Linear(24, 24)).to(dev).train()


def run_latent(E):
    o = operands(E)
    net, expansion = mlp(F + 64 + 2 * L), GaussianSmearing(0.0, 5.0, 32).to(dev)
    uemb = torch.nn.Parameter(torch.randn(1, 24, device=dev))
    lat = o['lat'].clone().requires_grad_()
    leaves = list(net.parameters()) + [uemb, lat]
    ia, ib = o['ei'][0], o['ei'][1]
    from disco_diffdock_amd.runtime import Context
    graph = Context.conv_graph(ia, ib, N_NODES, N_NODES)      # built once per batch by the caller, as conv_stack builds its own

    def fused():
        for q in leaves:
            q.grad = None
        emb, _ = fused_edge_embedding(net, expansion, o['pos'], o['pos'], o['ei'], o['sig'], o['sig_index'], feat=o['feat'], seed=7, latent_a=lat, latent_b=lat,
                                      unconditional=o['unc'], unconditional_embedding=uemb, graph=graph)
        emb.backward(o['gemb'])

    with torch.no_grad():      # the columns that carry no gradient, made once: the composition is not charged for them
        vec = o['pos'][ib] - o['pos'][ia]
        head = torch.cat([o['feat'], o['sig'][o['sig_index'].long()[ia]], expansion(vec.norm(dim=-1))], 1)

    def composition():
        for q in leaves:
            q.grad = None
        row = torch.cat([head, lat.index_select(0, ia), lat.index_select(0, ib)], 1)
        emb = net(row) + o['unc'][ia][:, None] * uemb
        emb.backward(o['gemb'])

    out = dict(E=E, fused=window(fused), composition=window(composition))
    out['composition_over_fused'] = out['composition']['ms'] / out['fused']['ms']
    return out


def run_plain(E):
    o = operands(E)
    net, expansion = mlp(F + 64), GaussianSmearing(0.0, 5.0, 32).to(dev)

    def fused():
        for q in net.parameters():
            q.grad = None
        emb, _ = fused_edge_embedding(net, expansion, o['pos'], o['pos'], o['ei'], o['sig'], o['sig_index'], feat=o['feat'], seed=7)
        emb.backward(o['gemb'])

    return dict(E=E, plain=window(fused))


result = dict(mode=args.mode, root=os.path.abspath(args.root), device=torch.cuda.get_device_name(0), reps=REPS, rounds=ROUNDS,
              cases=[(run_latent if args.mode == 'latent' else run_plain)(E) for E in SIZES])
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
