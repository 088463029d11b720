"""Time one ddk_ligand_automorphisms call (csrc/k_autos.hip) with HIP events for the test ligands with K = 2 (toluene, 7 atoms), 1 296 (CF3 x 4, 22 atoms)
and 7 776 (CF3 x 5, 27 atoms) of tests/automorphism_ref.py, at the test's capacity 2 K and at the default capacity 65 536 of Complex.automorphisms: the
median of 20 calls after 5 warm-up calls, beside the host search it replaces on the same graph: networkx's GraphMatcher where networkx imports (the
INTEGRATION.md recipe), the pure-Python reference otherwise.  Prints the table of profiles/automorphism_timing.md; `--out PATH` also writes it.  Run on
the GPU box."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import automorphism_ref as ar   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

try:
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
except ImportError:
    nx = None

WARMUP, CALLS = 5, 20
dev = torch.device('cuda', 0)
ctx = _shape_context(0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())


def host_search(colour, bonds):
    """(seconds, rows, which) of the host search"""
    t0 = time.perf_counter()
    if nx is not None:
        G = nx.Graph()
        G.add_nodes_from((a, dict(colour=int(c))) for a, c in enumerate(colour))
        G.add_edges_from(bonds.T.tolist())
        rows = sum(1 for _ in GraphMatcher(G, G, node_match=lambda a, b: a['colour'] == b['colour']).isomorphisms_iter())
        return time.perf_counter() - t0, rows, 'networkx %s GraphMatcher' % nx.__version__
    rows = len(ar.automorphisms_ref(colour, bonds))
    return time.perf_counter() - t0, rows, 'tests/automorphism_ref.py'


lines = ['| ligand | atoms | K | cap | launches | device: one call, median of %d | host search | host time |' % CALLS, '|---|---|---|---|---|---|---|---|']
for name in ('toluene', 'cf3_x4', 'cf3_x5'):
    colour, bonds, K, want = ar.graph_and_table(name)
    n = len(colour)
    host_s, host_rows, which = host_search(colour, bonds)
    assert host_rows == K
    d_c, d_b = torch.from_numpy(colour.astype(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(bonds, np.int32)).to(dev)
    for cap in (2 * K, 65536):
        perms = torch.empty((cap, n), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(ctx.L.ddk_ligand_automorphisms_workspace(n, cap), dtype=torch.uint8, device=dev)
        times = []
        for k in range(WARMUP + CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx._check(ctx.L.ddk_ligand_automorphisms(ctx.h, n, ptr(d_c), ptr(d_b), bonds.shape[1], None, ptr(perms), cap, ptr(count), ptr(ws), st),
                       'ddk_ligand_automorphisms')
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                times.append(e0.elapsed_time(e1) * 1e3)
        assert count.cpu().tolist() == [K, 0] and ar.same_set(perms[:K].cpu().numpy(), want)
        launches = 2 if cap * n <= 16384 else 2 * n          # the walk and the emit, plus a pair per further level beyond the walk-only size
        lines.append('| %s | %d | %d | %d | %d | %.1f us | %s | %.2f ms |' % (name, n, K, cap, launches, statistics.median(times), which, host_s * 1e3))
text = '\n'.join(lines)
print(text)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(text + '\n')
