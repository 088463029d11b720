"""Time the data half of a training step (training.noise_batch + training.loss_function on a BatchTargets) against the same work done with the per-complex
calls that existed before it (G noise_complex(B=1) calls and G loss_function(Targets) calls), for G = 32 different synthetic complexes (300 residues,
ligands of about 30 atoms) at 32 different times, and the share of one train_epoch step that is spent outside the model's forward and backward.

    python tools/time_noise_batch.py wall [--out PATH]      host wall time, a device synchronise before the clock starts and before it stops; median of 3
    python tools/time_noise_batch.py kernels                the three ops 50 times each, for `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own

Both sides of a comparison run in the same process on the same build.  Run on the GPU box."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco_diffdock_amd import data as ddk_data, synthetic, training   # noqa: E402
from disco_diffdock_amd.runtime import Complex   # noqa: E402
from disco_diffdock_amd.tensor_layers import _shape_context   # noqa: E402

G, SEED, REPEATS, WARMUP = 32, 5, 3, 2
dev = torch.device('cuda', 0)
ctx = _shape_context(0)
# (the kernel run never reads the receptors: small ones keep its 50 collations short)
complexes = [synthetic.make_complex(100 + g, n_res=20 if sys.argv[1:2] == ['kernels'] else 300, n_lig=30) for g in range(G)]
times = training.draw_times([c['name'] for c in complexes], SEED, 0)
rotors = [int(np.asarray(c['edge_mask']).sum()) for c in complexes]
T = sum(rotors)


def bracket(fn, repeats=REPEATS):
    out = []
    for k in range(WARMUP + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= WARMUP:
            out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def predictions(n, n_tor, grad=False):
    gen = torch.Generator().manual_seed(1)
    return [torch.randn(*s, generator=gen).to(dev).requires_grad_(grad) for s in ((n, 3), (n, 3), (n_tor,))]


def batch_path():
    _, tg = training.noise_batch(ctx, complexes, times, SEED)
    return training.loss_function(*predictions(G, T), tg, ctx)


def per_complex_path(cxs=None, rows=None):
    out = []
    for g, c in enumerate(complexes):
        _, tg = training.noise_complex(ctx, c, float(times[g]), 1, SEED, cx=None if cxs is None else cxs[g], so3_row=None if rows is None else rows[g])
        out.append(training.loss_function(*predictions(1, rotors[g]), tg, ctx))
    return out


def wall():
    res = dict(G=G, atoms=[len(c['lig_pos']) for c in complexes], rotors=rotors, residues=300, repeats=REPEATS, warmup=WARMUP)
    res['noise_batch_plus_loss'] = bracket(batch_path)
    res['collate_and_upload_alone'] = bracket(lambda: ddk_data.collate([ddk_data.from_arrays(c) for c in complexes]).to(dev))
    res['per_complex_calls'] = bracket(per_complex_path)
    cxs = [Complex(ctx, c, 1) for c in complexes]
    cdf, score, _ = ctx.so3_rows([int(training.so3_eps_index(training._sigmas(ctx, float(t))[1])) for t in times], exp_score_norm=False)
    rows = [(cdf[g], score[g]) for g in range(G)]
    res['per_complex_calls_complexes_and_rows_prepared'] = bracket(lambda: per_complex_path(cxs, rows))
    # one training step, split at the model: everything before the forward and after the backward against the forward and backward themselves
    from oracle import score_model_ref as smr
    from disco_diffdock_amd.train_model import TrainableScoreModel
    model = TrainableScoreModel(sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True,
                                lm_embedding_type='esm', batch_norm=True, dropout=0.1)
    P = smr.random_state_dict(smr.ScoreModelConfig(), seed=6)
    model.load_state_dict({k: v for k, v in P.items() if k in model.state_dict()}, strict=True)
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    state = {}

    def data_half():
        state['batch'] = training.noise_batch(model, complexes[:8], times[:8], SEED)

    def model_half():
        opt.zero_grad()
        data, tg = state['batch']
        pred = model(data, seed=3)
        state['pred'] = [p.detach() for p in pred]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = training.loss_function(*pred, tg, model)[0]
        torch.cuda.synchronize()
        state['loss_ms'] = (time.perf_counter() - t0) * 1e3
        loss.backward()
        opt.step()

    data_half()
    res['train_step_8_graphs'] = dict(noise_batch=bracket(data_half), forward_loss_backward_step=bracket(model_half), loss_forward_ms_last=None)
    res['train_step_8_graphs']['loss_forward_ms_last'] = state['loss_ms']
    d, m = res['train_step_8_graphs']['noise_batch']['median_ms'], res['train_step_8_graphs']['forward_loss_backward_step']['median_ms']
    res['train_step_8_graphs']['share_outside_model'] = (d + state['loss_ms']) / (d + m)
    text = json.dumps(res, indent=1)
    print(text)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(text + '\n')


def kernels():
    _, tg = training.noise_batch(ctx, complexes, times, SEED)
    pred = predictions(G, T, grad=True)
    for _ in range(50):
        _, tg = training.noise_batch(ctx, complexes, times, SEED)
        training.loss_function(*pred, tg, ctx)[0].sum().backward()
    torch.cuda.synchronize()


if __name__ == '__main__':
    {'wall': wall, 'kernels': kernels}[sys.argv[1]]()
