"""Time the AR model's loss op against the reference's per-graph loop, and one train_ar_epoch step (profiles/ar_training_kernel_stats.md).

    python tests/devtools/profile_ar_training.py [--out FILE.json]

Both sides run in ONE process on the same device and the same tables: ``ar_training.ar_loss`` forward + backward (one ddk_node_cross_entropy_batch launch each
way) against the reference's loop restated in plain torch (train_ar.py:116-127: per graph a boolean mask per side, ``l_idx.sum()``-style host read-backs
through the slicing, one ``F.cross_entropy``, the losses added up, one backward), at G = 5 and G = 32 with timesplit-shaped node counts (ligands of 20 to
60 atoms, receptors of 150 to 2129 residues; the largest graph holds the largest timesplit receptor).  Medians of repeated timed passes after warm-up, a
device synchronise inside every pass.  Then one ``train_ar_epoch`` step (batch of 3 synthetic complexes) of a TrainablePretrainedScoreEncoder."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path.insert(0, ROOT)

from disco_diffdock_amd import ar_training, build, synthetic      # noqa: E402
from disco_diffdock_amd.pretrained_score_encoder import ARLogits, TrainablePretrainedScoreEncoder      # noqa: E402
from disco_diffdock_amd.train_model import TrainableScoreModel      # noqa: E402

PASSES, WARMUP, INNER = 15, 5, 20


def _tables(G, D, dev, seed):
    rng = np.random.default_rng(seed)
    n_l = rng.integers(20, 61, G)
    n_r = rng.integers(150, 1200, G)
    n_r[-1] = 2129
    lig_ptr, rec_ptr = (torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int64)).to(dev) for n in (n_l, n_r))
    f = lambda *shape: torch.from_numpy(rng.normal(0, 2, shape).astype(np.float32)).to(dev)
    data = type('Batch', (), {})()
    data.lig_ptr, data.rec_ptr, data.teacher_l, data.teacher_r = lig_ptr, rec_ptr, f(int(n_l.sum()), D), f(int(n_r.sum()), D)
    data.decoding_idx = torch.from_numpy(rng.integers(0, D, G).astype(np.int32)).to(dev)
    data.lig_batch = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(n_l).to(dev))
    data.rec_batch = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(n_r).to(dev))
    return data, f(int(n_l.sum()), 1).requires_grad_(), f(int(n_r.sum()), 1).requires_grad_()


def _op(data, logit_l, logit_r, soft):
    logit_l.grad = logit_r.grad = None
    ar_training.ar_loss(ARLogits(logit_l, logit_r, data.lig_ptr, data.rec_ptr), data, soft)[0].backward()


def _loop(data, logit_l, logit_r, soft):
    """the reference's loop: per graph the nodes are found with boolean masks, the label is read per graph"""
    logit_l.grad = logit_r.grad = None
    G = data.decoding_idx.shape[0]
    idx = data.decoding_idx.tolist()
    total = 0
    for g in range(G):
        ml, mr = data.lig_batch == g, data.rec_batch == g
        s = torch.cat([logit_l[ml, 0], logit_r[mr, 0]])
        t = torch.cat([data.teacher_l[ml, idx[g]], data.teacher_r[mr, idx[g]]])
        label = torch.softmax(t, 0)[None] if soft else torch.argmax(t)
        total = total + torch.nn.functional.cross_entropy(s[None] if soft else s, label)
    (total / G).backward()


def _median_ms(fn, *args, inner=INNER):
    for _ in range(WARMUP):
        fn(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(PASSES):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn(*args)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / inner * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ar_training_timing.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no CPU path'
    build.build(verbose=False)
    dev = torch.device('cuda:0')
    out = {'passes': PASSES, 'calls_per_pass': INNER, 'loss': []}
    for G in (5, 32):
        for soft in (False, True):
            data, l, r = _tables(G, 2, dev, seed=G)
            a, b = _median_ms(_op, data, l, r, soft), _median_ms(_loop, data, l, r, soft)
            _op(data, l, r, soft)
            g_op = (l.grad.clone(), r.grad.clone())
            _loop(data, l, r, soft)
            err = max(float((x - y).abs().max()) for x, y in zip(g_op, (l.grad, r.grad)))
            row = dict(G=G, soft=soft, nodes=int(l.shape[0] + r.shape[0]), op_ms=a[0], op_min_max=a[1:], loop_ms=b[0], loop_min_max=b[1:], ratio=b[0] / a[0],
                       max_abs_grad_difference=err)
            print(row, flush=True)
            out['loss'].append(row)
    # one train_ar_epoch step: three synthetic complexes in one batch
    cs = [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in ((70, 22), (71, 28), (60, 35))]
    torch.manual_seed(1)
    sm = TrainableScoreModel(sh_lmax=1, ns=24, nv=6, num_conv_layers=5, lig_max_radius=5.0, cross_max_distance=80, dynamic_max_cross=True,
                             lm_embedding_type='esm', latent_dim=2, latent_vocab=1, latent_droprate=0.1, dropout=0.1)
    ar = TrainablePretrainedScoreEncoder(sm, ns=16, latent_dim=1, latent_vocab=1, latent_dropout=0.1, latent_hidden_dim=128, input_latent_dim=2,
                                         apply_gumbel_softmax=False).to(dev)
    rng = np.random.default_rng(0)
    labels = {}
    for c in cs:
        n_l, n_r = len(c['lig_pos']), len(c['rec_pos'])
        hot = np.zeros((n_l + n_r, 2), np.float32)
        hot[rng.integers(0, n_l + n_r, 2), [0, 1]] = 1
        labels[c['name']] = (torch.from_numpy(hot[:n_l].copy()), torch.from_numpy(hot[n_l:].copy()))
    opt = torch.optim.Adam(ar.parameters(), lr=1e-3)
    epoch = [0]

    def step():
        ar_training.train_ar_epoch(ar, cs, labels, opt, 3, seed=5, epoch=epoch[0])
        epoch[0] += 1

    m = _median_ms(step, inner=3)
    out['train_ar_epoch_step_ms'] = dict(median=m[0], min=m[1], max=m[2], graphs=3)
    print(out['train_ar_epoch_step_ms'], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
