"""Time ddk_conformer_match (csrc/k_match.hip) with HIP events on the twelve yardstick cases of tests/golden/conformer_matching.npz and on one 80-atom /
29-rotor synthetic ligand, at (popsize, maxiter) = (15, 15), (20, 20) and (15, 500) with 1 and 8 islands (tol = 0, so every generation runs): the median of
CALLS warm calls, per call and per generation, beside scipy's differential_evolution on the numpy objective on this host's CPU (the optimiser the reference
calls; one run each, the 80-atom ligand at (15, 15) only).  The events bracket the C call alone: the arguments are converted and uploaded, and the outputs
and the workspace allocated, before the first event.  Prints the table of profiles/conformer_matching.md; `--out PATH` also writes it.  Run on the GPU box."""
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
import matching_ref as mr   # noqa: E402
from disco_diffdock_amd import _lib, synthetic   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

WARMUP, CALLS = 3, 9
SETTINGS = ((15, 15), (20, 20), (15, 500))


def device_us(ctx, dev, c, popsize, maxiter, n_islands):
    """median microseconds of one ddk_conformer_match call (polish included) and of the same call without polish"""
    n, R = len(c['pos0']), len(c['rot_bonds'])
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    d = [up(c['pos0'], np.float32), up(c['target'], np.float32), None, up(c['rot_bonds'], np.int32), up(c['mask_rotate'], np.uint8)]
    tor, pos = torch.empty(R, dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
    rmsd, count = torch.empty(2, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(ctx.L.ddk_conformer_match_workspace(n, R, popsize, n_islands), dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for polish in (128, 0):
        opt = _lib.ddk_match_options(popsize, maxiter, 0.0, polish, n_islands, 0, 0)
        times = []
        for k in range(WARMUP + CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx._check(ctx.L.ddk_conformer_match(ctx.h, n, *[ptr(t) for t in d], R, C.byref(opt), ptr(tor), ptr(pos), ptr(rmsd), ptr(count), ptr(ws), st),
                       'ddk_conformer_match')
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                times.append(e0.elapsed_time(e1) * 1e3)
        assert count.cpu().tolist()[1] == 0
        out.append(statistics.median(times))
    return out


def scipy_seconds(c, popsize, maxiter):
    from scipy.optimize import differential_evolution
    f = lambda x: mr.objective(c['pos0'], c['target'], c['rot_bonds'], c['mask_rotate'], x)
    t0 = time.perf_counter()
    res = differential_evolution(f, [(-np.pi, np.pi)] * len(c['rot_bonds']), maxiter=maxiter, popsize=popsize, mutation=(0.5, 1), recombination=0.8, seed=0)
    return time.perf_counter() - t0, res.fun


def main():
    dev = torch.device('cuda', 0)
    ctx = _shape_context(0)
    problems = [('case %d' % s, mr.golden_case(s)) for s in mr.GOLDEN_SEEDS]
    lig = synthetic.make_ligand(np.random.default_rng(80), 80)
    big = dict(pos0=np.asarray(lig['lig_pos'], np.float32), rot_bonds=mr.rotors(lig), mask_rotate=np.asarray(lig['mask_rotate'], bool))
    rng = np.random.default_rng(0)
    big['target'] = (mr.apply_torsions(big['pos0'], big['rot_bonds'], big['mask_rotate'], rng.uniform(-np.pi, np.pi, size=len(big['rot_bonds'])))
                     + 0.15 * rng.normal(size=big['pos0'].shape)).astype(np.float32)
    problems.append(('80 atoms', big))

    lines = ['| ligand | atoms | rotors | popsize, maxiter | islands | members | device call, median of %d | of which generations | per generation | scipy on this CPU |' % CALLS,
             '|---|---|---|---|---|---|---|---|---|---|']
    for name, c in problems:
        R = len(c['rot_bonds'])
        for popsize, maxiter in SETTINGS:
            if name != '80 atoms' and name != 'case 100' and (popsize, maxiter) != (20, 20):
                continue      # the twelve cases at the reference's defaults; the first of them and the large ligand at every setting
            host = ''
            if (popsize, maxiter) == (20, 20) and name != '80 atoms' or (name == '80 atoms' and (popsize, maxiter) == (15, 15)):
                s, fun = scipy_seconds(c, popsize, maxiter)
                host = '%.2f s (fun %.4f)' % (s, fun)
            for islands in (1, 8):
                full, search = device_us(ctx, dev, c, popsize, maxiter, islands)
                lines.append('| %s | %d | %d | %d, %d | %d | %d | %.0f us | %.0f us | %.1f us | %s |' % (
                    name, len(c['pos0']), R, popsize, maxiter, islands, islands * mr.members(popsize, R), full, search, search / (maxiter + 1), host))
    text = '\n'.join(lines)
    print(text)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
