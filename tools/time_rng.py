"""Time the sampler's draws with and without a seed (csrc/k_rng.hip against the host RNG streams / torch's device generator they replace) at the
sampler's shape: 40 samples, 20 steps, a ~30-atom ligand.  Two brackets, each the median of CALLS calls after WARMUP warm-up calls, a device
synchronise before the clock starts and before it stops (host wall time: the unseeded randomize_position is a host loop, so the host clock is the honest one):
  randomize_position   sampling.randomize_position on 40 copies, seeded (one ddk_rng_initial launch) vs unseeded (numpy + scipy + torch per copy, three uploads)
  noise fill           Context.rng_noise [20, 40, 6 + R] vs sampling.draw_noise (torch's device generator), both with the last step's noise off
Both sides run in the same process on the same build.  Prints the table of profiles/rng_timing.md; `--out PATH` also writes it.  Run on the GPU box."""
import os
import statistics
import sys
import time
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco_diffdock_amd import synthetic   # noqa: E402
from disco_diffdock_amd.data import from_arrays   # noqa: E402
from disco_diffdock_amd.diffusion_utils import get_t_schedule, t_to_sigma   # noqa: E402
from disco_diffdock_amd.runtime import stream_id   # noqa: E402
from disco_diffdock_amd.sampling import draw_noise, randomize_position, step_coefficients   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

SAMPLES, STEPS, N_LIG, WARMUP, CALLS = 40, 20, 30, 5, 30
dev = torch.device('cuda', 0)
ctx = _shape_context(0)
c = synthetic.make_complex(3, n_res=120, n_lig=N_LIG)
R = int(np.asarray(c['edge_mask']).sum())
stream = stream_id(c['name'])
args = SimpleNamespace(tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14, no_torsion=False)
sched = get_t_schedule(STEPS)
_, _, nc = step_coefficients(STEPS, sched, sched, sched, partial(t_to_sigma, args=args), args, False, False, True, 1.0, 0.0, 0.5)


def bracket(fn):
    times = []
    for k in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times), min(times), max(times)


def graphs():
    return [from_arrays(c) for _ in range(SAMPLES)]


lists = iter([graphs() for _ in range(2 * (WARMUP + CALLS))])      # built outside the brackets: every call gets fresh copies at the conformer
rows = [('randomize_position, %d copies, %d atoms, %d rotatable bonds' % (SAMPLES, len(c['lig_pos']), R),
         bracket(lambda: randomize_position(next(lists), False, False, 19.0, device=dev, seed=7)),
         bracket(lambda: randomize_position(next(lists), False, False, 19.0, device=dev))),
        ('noise fill [%d, %d, %d]' % (STEPS, SAMPLES, 6 + R),
         bracket(lambda: ctx.rng_noise(7, stream, 0, SAMPLES, STEPS, 6 + R, noise_coeff=nc)),
         bracket(lambda: draw_noise(STEPS, SAMPLES, R, R, nc, dev)))]
lines = ['| bracket (host wall time, synchronised on both sides; median of %d calls, min - max) | seeded | unseeded | unseeded / seeded |' % CALLS, '|---|---|---|---|']
for name, s, u in rows:
    lines.append('| %s | %.0f us (%.0f - %.0f) | %.0f us (%.0f - %.0f) | %.1f |' % ((name,) + s + u + (u[0] / s[0],)))
text = '\n'.join(lines)
print(text)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(text + '\n')
