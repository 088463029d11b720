"""Time one ddk_pose_pairwise_rmsd + ddk_pose_cluster call (csrc/k_pairs.hip) with HIP events at the sampler's shape, B = 40 poses x 80 atoms, for
n_perms in {1, 1024}: the median of 20 calls after 5 warm-up calls, beside the numpy reference of tests/pairwise_ref.py on the host for the same input
(what the device call replaces).  Prints the table of profiles/pairwise_rmsd_timing.md; `--out PATH` also writes it.  Run on the GPU box."""
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
import pairwise_ref as pr   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

B, N_LIG, WARMUP, CALLS = 40, 80, 5, 20
dev = torch.device('cuda', 0)
ctx = _shape_context(0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())
pos = pr.typical(B, N_LIG, seed=0)
score = np.random.default_rng(0).normal(size=B).astype(np.float32)
d_pos, d_score = torch.from_numpy(pos).to(dev), torch.from_numpy(score).to(dev)
rmsd = torch.empty((B, B), device=dev)
cluster, leaders, n = (torch.empty(k, dtype=torch.int32, device=dev) for k in (B, B, 1))

lines = ['| n_perms | device: pairwise RMSD + clustering, median of %d calls | of which the RMSD matrix | host: numpy reference, fp64 | host: numpy reference, fp32 |' % CALLS,
         '|---|---|---|---|---|']
for n_perms in (1, 1024):
    table = pr.random_table(n_perms, N_LIG, seed=1)
    d_table = torch.from_numpy(table).to(dev)

    def pairs():
        ctx._check(ctx.L.ddk_pose_pairwise_rmsd(ctx.h, B, N_LIG, ptr(d_pos), None, ptr(d_table), n_perms, ptr(rmsd), st), 'ddk_pose_pairwise_rmsd')

    def both():
        pairs()
        ctx._check(ctx.L.ddk_pose_cluster(ctx.h, B, ptr(rmsd), ptr(d_score), 2.0, ptr(cluster), ptr(leaders), ptr(n), st), 'ddk_pose_cluster')

    med = {}
    for name, fn in (('both', both), ('pairs', pairs)):
        times = []
        for k in range(WARMUP + CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                times.append(e0.elapsed_time(e1) * 1e3)
        med[name] = statistics.median(times)
    host = {}
    for dt in (np.float64, np.float32):
        t0 = time.perf_counter()
        ref = pr.pairwise_rmsd_ref(pos, None, table, dtype=dt)
        pr.cluster_ref(ref, score, 2.0)
        host[dt] = (time.perf_counter() - t0) * 1e3
    assert np.abs(rmsd.cpu().numpy() - pr.pairwise_rmsd_ref(pos, None, table)).max() < 1e-4
    lines.append('| %d | %.1f us | %.1f us | %.1f ms | %.1f ms |' % (n_perms, med['both'], med['pairs'], host[np.float64], host[np.float32]))
text = '\n'.join(lines)
print(text)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(text + '\n')
