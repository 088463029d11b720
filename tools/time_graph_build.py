"""Time the three table builders of csrc/k_build.hip (ddk_receptor_knn_graph, ddk_radius_graph, ddk_ligand_transformation_mask) with HIP events: receptors of
300 and 3000 residues (synthetic.make_receptor), their atoms (synthetic.add_receptor_atoms) and ligands of 30 and 80 atoms (synthetic.make_ligand); the
median of 20 calls after 5 warm-up calls, beside the host code of synthetic.py that builds the same tables (timed once; for the two receptor tables it is
the graph part of the generator alone, restated here, not the point sampling).  Prints the table of profiles/graph_build_timing.md; `--out PATH` also
writes it.  Run on the GPU box."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco_diffdock_amd import synthetic   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

WARMUP, CALLS = 5, 20
dev = torch.device('cuda', 0)
ctx = _shape_context(0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())


def device_us(call):
    times = []
    for k in range(WARMUP + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def host_knn(pos, cutoff=15.0, max_neighbor=24):
    """the graph part of synthetic.make_receptor"""
    t0 = time.perf_counter()
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    E = 0
    for i in range(len(pos)):
        nb = list(np.where(d[i] < cutoff)[0])
        nb.remove(i)
        if len(nb) > max_neighbor:
            nb = list(np.argsort(d[i]))[1:max_neighbor + 1]
        if len(nb) == 0:
            nb = list(np.argsort(d[i]))[1:2]
        E += len(nb)
    return time.perf_counter() - t0, E


def host_radius(pos, r=5.0, k=8):
    """the graph part of synthetic.add_receptor_atoms"""
    t0 = time.perf_counter()
    order = np.argsort(pos[:, 0], kind='stable')
    xs = pos[order, 0]
    for i in range(len(pos)):
        lo, hi = np.searchsorted(xs, pos[i, 0] - r), np.searchsorted(xs, pos[i, 0] + r)
        cand = np.sort(order[lo:hi])
        d = np.linalg.norm(pos[cand] - pos[i], axis=1)
        cand[(d < r) & (cand != i)][:k]
    return time.perf_counter() - t0


lines = ['| call | input | result | launches | device: one call, median of %d | host (synthetic.py) |' % CALLS, '|---|---|---|---|---|---|']
count = torch.empty(2, dtype=torch.int32, device=dev)
for n_res in (300, 3000):
    c = synthetic.make_receptor(np.random.default_rng(n_res), n_res, esm_dim=4)
    c = synthetic.add_receptor_atoms(c, np.random.default_rng(n_res + 1))
    pos = torch.from_numpy(c['rec_pos']).to(dev)
    n, K = n_res, 24
    out = torch.empty((2, n * K), dtype=torch.int32, device=dev)
    ws = torch.empty(ctx.L.ddk_receptor_knn_graph_workspace(n, K), dtype=torch.uint8, device=dev)
    us = device_us(lambda: ctx._check(ctx.L.ddk_receptor_knn_graph(ctx.h, n, ptr(pos), 15.0, K, ptr(out), n * K, ptr(count), ptr(ws), st), 'knn'))
    host_s, E = host_knn(c['rec_pos'].astype(np.float64))
    assert count.cpu().tolist() == [E, 0]
    lines.append('| ddk_receptor_knn_graph | %d residues | %d edges | 3 | %.1f us | %.1f ms |' % (n, E, us, host_s * 1e3))
    apos = torch.from_numpy(c['atom_pos']).to(dev)
    n, K = apos.shape[0], 8
    out = torch.empty((2, n * (K + 1)), dtype=torch.int32, device=dev)
    ws = torch.empty(ctx.L.ddk_radius_graph_workspace(n, K), dtype=torch.uint8, device=dev)
    us = device_us(lambda: ctx._check(ctx.L.ddk_radius_graph(ctx.h, n, ptr(apos), 5.0, K, ptr(out), n * (K + 1), ptr(count), ptr(ws), st), 'radius'))
    E, status = count.cpu().tolist()
    assert status == 0
    lines.append('| ddk_radius_graph | %d atoms (of %d residues) | %d edges | 3 | %.1f us | %.1f ms |' % (n, n_res, E, us, host_radius(c['atom_pos']) * 1e3))
for n_lig in (30, 80):
    lig = synthetic.make_ligand(np.random.default_rng(n_lig), n_lig)
    n, bi = len(lig['lig_x']), lig['bond_index']
    M = bi.shape[1]
    d_b = torch.from_numpy(np.ascontiguousarray(bi, np.int32)).to(dev)
    em, mr = torch.empty(M, dtype=torch.uint8, device=dev), torch.empty((M // 2, n), dtype=torch.uint8, device=dev)
    ws = torch.empty(ctx.L.ddk_ligand_transformation_mask_workspace(n, M), dtype=torch.uint8, device=dev)
    us = device_us(lambda: ctx._check(ctx.L.ddk_ligand_transformation_mask(ctx.h, n, ptr(d_b), M, ptr(em), ptr(mr), M // 2, ptr(count), ptr(ws), st), 'mask'))
    t0 = time.perf_counter()
    want_e, want_r = synthetic.transformation_mask(n, [tuple(p) for p in bi[:, 0::2].T.tolist()])
    host_s = time.perf_counter() - t0
    R, status = count.cpu().tolist()
    assert status == 0 and np.array_equal(em.cpu().numpy(), want_e) and np.array_equal(mr[:R].cpu().numpy(), want_r)
    lines.append('| ddk_ligand_transformation_mask | %d atoms, %d bonds | %d rotatable | 1 | %.1f us | %.2f ms |' % (n, M // 2, R, us, host_s * 1e3))
text = '\n'.join(lines)
print(text)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(text + '\n')
