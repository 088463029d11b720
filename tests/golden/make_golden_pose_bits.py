#!/usr/bin/env python
"""Generate tests/golden/pose_update_bits.json: the SHA-256 of the raw bytes of every output of the entry points that run the pose update
(se3_update_kernel<POST, REC>, modify_conformer_batch_kernel), the heads' finish (heads_post_kernel and the POST block of the update) and the bond
rotor step (the update's rotor loop, match_eval, randomize_kernel), on the smallest cases that reach every branch of the code these kernels share.

Like make_golden_train_ops_bits.py this needs no reference checkout: it EXECUTES THE DEVICE ENTRY POINTS on a MI355X, at a commit whose arithmetic is
known to be good, and records what they give.  tests/test_gpu_pose_bits.py recomputes the same outputs with ``outputs`` below and compares the digests,
so a multiply-add that the compiler contracts differently in one of the kernels that share a body shows as a changed digest where the fp64 tests see
nothing.  Inputs come from numpy.random.default_rng with fixed seeds; the generator computes everything twice and refuses to write a file if an
output is not identical run to run.

    python tests/golden/make_golden_pose_bits.py [--commit HASH]

THE CASES.  Ligands and update classes are those of tests/adversarial_geometry.py, B = 3.
    ligands       chain3 (R = 0, the rigid branch), chain4 (R = 1), chain68 (R = 65, one past the 64-rotor chunk), chain256 (n = MAX_LIG, R = 253, four
                  chunks), branched
    se3_update    Complex.se3_update on topology-only complexes (<false, false>): every ligand x typical / tiny (the series branch of the axis-angle
                  matrix inside the rotor loop) / half_turn / rigid (no torsion pointer), at offsets 0 and 150
    batch         Context.modify_conformer_batch: one ragged call with all five ligands (graph g takes update class g of typical, tiny, half_turn,
                  typical, tiny and sits at offset 0 or 150 in turn), and the same call without torsion updates; poses and statuses
    sample        Complex.sample on a deterministic context with random weights, a 40-residue complex, 4 steps, injected noise: plain (<true, false>)
                  and recorded (<true, true>, all four record arrays); once more on a no_torsion context (the rigid record)
    guided        the same on a latent-conditioned deterministic context with classifier-free guidance on steps 2 and 3 of 5 (the setup of
                  test_recorded_guided_steps_vs_oracle): those steps run heads_post_kernel, cfg_combine and <false, *>
    score         Complex.score_forward on the deterministic context: the three outputs heads_post_kernel writes
    randomize     Complex.randomize_position at n = 68 with torsions (an exact 0 among them: the skipped rotor) and without
    rmsd          Context.conformer_rmsd on chain68 with a typical and a zero torsion vector
    match         Context.match_conformer on chain4 and branched with popsize 1, maxiter 0, polish_iters 0 (the smallest the entry point accepts), and
                  with maxiter 1, polish_iters 2 (one generation and the polish kernel), seed 5
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.abspath(os.path.join(HERE, '..'))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, 'pose_update_bits.json')

B = 3
LIGANDS = ('chain3', 'chain4', 'chain68', 'chain256', 'branched')
CLASSES = ('typical', 'tiny', 'half_turn', 'rigid')
OFFSETS = (0.0, 150.0)
BATCH_CLASSES = ('typical', 'tiny', 'half_turn', 'typical', 'tiny')
TOR_KEYS = ('final_edge_embedding', 'tor_bond_conv', 'tor_final_layer')
MATCH = {'min': dict(popsize=1, maxiter=0, polish_iters=0), 'polish': dict(popsize=1, maxiter=1, polish_iters=2)}
T = torch.from_numpy


def _prefix(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _se3_update(dev, ctx):
    import adversarial_geometry as ag
    from disco_diffdock_amd.runtime import Complex
    out = []
    for lig in LIGANDS:
        c = ag.ligand(lig)
        cx = Complex(ctx, c, max_batch=B)
        for cls in CLASSES:
            tr, rot, tor = ag.updates(cls, cx.R, B, seed=7)
            for offset in OFFSETS:
                pos = ag.poses(c, B, offset)
                got = cx.se3_update(T(pos).to(dev), T(tr).to(dev), T(rot).to(dev), None if tor is None else T(tor).to(dev))
                out.append((f'se3_update.{lig}.{cls}.at{offset:g}', got))
    return out


def _batch(dev, ctx):
    import adversarial_geometry as ag
    cs = [ag.ligand(lig) for lig in LIGANDS]
    rot_counts = [len(ag.rotors(c)) for c in cs]
    pos = np.concatenate([ag.poses(c, 1, OFFSETS[g % 2])[0] for g, c in enumerate(cs)])
    ups = [ag.updates(cls, R, 1, seed=20 + g) for g, (cls, R) in enumerate(zip(BATCH_CLASSES, rot_counts))]
    tr, rot, tor = (np.concatenate([u[k].reshape(-1, 3) if k < 2 else u[k].reshape(-1) for u in ups]) for k in range(3))
    node_ptr, tor_ptr = _prefix([len(c['lig_pos']) for c in cs]), _prefix(rot_counts)
    bonds = np.concatenate([ag.rotors(c).reshape(-1, 2) for c in cs]).astype(np.int32)
    masks = np.concatenate([np.asarray(c['mask_rotate'], np.uint8).reshape(-1) for c in cs])
    mask_ptr = _prefix([r * len(c['lig_pos']) for r, c in zip(rot_counts, cs)])
    out = []
    for name, t in (('ragged', T(tor).to(dev)), ('no_torsion', None)):
        p, status = ctx.modify_conformer_batch(T(pos).to(dev), node_ptr, bonds, masks, mask_ptr, tor_ptr, T(tr).to(dev), T(rot).to(dev), t, return_status=True)
        out += [(f'batch.{name}.pos', p), (f'batch.{name}.status', status)]
    return out


def _sampled(tag, cx, pos0, t_arr, sc, nc, z):
    """the plain and the recorded call of one workload -> the final poses of both and the four record arrays"""
    plain = cx.sample(pos0.clone(), t_arr, sc, nc, z)
    p_rec = pos0.clone()
    rec = cx.sample(p_rec, t_arr, sc, nc, z, record=True)
    return [(f'{tag}.plain.pos', plain), (f'{tag}.recorded.pos', p_rec)] + [(f'{tag}.recorded.rec_{k}', v) for k, v in rec._asdict().items()]


def _sample(dev):
    from oracle import score_model_ref as smr
    from test_gpu_trajectory import CFG, _coefficients
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    c = synthetic.make_complex(3, n_res=40)
    P = smr.random_state_dict(CFG, seed=9)
    steps = 4
    _, t_arr, sc, nc = _coefficients(steps)
    rng = np.random.default_rng(77)
    pos0 = T(np.stack([c['lig_pos'] + rng.normal(0, 1.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)).to(dev)
    out = []
    for tag, kw, weights in (('sample', {}, P), ('sample_no_torsion', dict(no_torsion=1), {k: v for k, v in P.items() if not k.startswith(TOR_KEYS)})):
        ctx = Context(device=0, deterministic=1, **kw)
        ctx.load_state_dict(weights)
        cx = Complex(ctx, c, B)
        assert cx.R > 0
        z = T((0.3 * np.random.default_rng(3).standard_normal((steps, B, 6 + cx.R))).astype(np.float32)).to(dev)
        out += _sampled(tag, cx, pos0, t_arr, sc, nc, z)
        if not kw:
            out += [(f'score.{k}', v) for k, v in zip(('tr', 'rot', 'tor'), cx.score_forward(pos0, 0.5, 0.5, 0.5))]
    return out


def _guided(dev):
    from oracle import score_model_ref as smr
    from test_gpu_trajectory import _coefficients
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    cfg = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    c = synthetic.make_complex(31, n_res=40, n_lig=22)
    ctx = Context(device=0, deterministic=1, latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    ctx.load_state_dict(smr.random_state_dict(cfg, seed=13))
    steps = 5
    cx = Complex(ctx, c, B)
    n_l, n_r = cx.n_lig, cx.n_rec
    rng = np.random.default_rng(2)
    ll, lr = torch.zeros(B * n_l, 2), torch.zeros(B * n_r, 2)
    for s in range(B):
        lr[s * n_r + rng.integers(n_r), 0] = 1
        (ll if s == 1 else lr)[s * (n_l if s == 1 else n_r) + rng.integers(n_l if s == 1 else n_r), 1] = 1
    cx.set_latents(ll.to(dev), lr.to(dev), 0.0)
    cx.set_guidance(0.7, 0.7, 0.3)
    sched, t_arr, sc, nc = _coefficients(steps)
    assert [bool(0.3 <= t <= 0.7) for t in sched] == [False, False, True, True, False]
    pos0 = T(np.stack([c['lig_pos'] + rng.normal(0, 2.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)).to(dev)
    z = T((0.2 * rng.standard_normal((steps, B, 6 + cx.R))).astype(np.float32)).to(dev)
    return _sampled('guided', cx, pos0, t_arr, sc, nc, z)


def _rotations(rng, n):
    import adversarial_geometry as ag
    return np.stack([ag._rot64(v) for v in rng.normal(size=(n, 3))])


def _randomize(dev, ctx):
    import adversarial_geometry as ag
    from disco_diffdock_amd.runtime import Complex
    c = ag.ligand('chain68')
    cx = Complex(ctx, c, max_batch=B)
    rng = np.random.default_rng(68)
    tor = rng.uniform(-np.pi, np.pi, size=(B, cx.R)).astype(np.float32)
    for b in range(B):
        tor[b, 63 + b % 2] = 0.0          # a skipped rotor
    rot, tr = _rotations(rng, B).astype(np.float32), rng.normal(0, 19.0, size=(B, 3)).astype(np.float32)
    pos0 = T(np.asarray(c['lig_pos'], np.float32)).to(dev)
    return [(f'randomize.{name}', cx.randomize_position(pos0, T(rot).to(dev), t, T(tr).to(dev))) for name, t in (('full', T(tor).to(dev)), ('no_torsion', None))]


def _matching(dev, ctx):
    import adversarial_geometry as ag
    out = []
    c = ag.ligand('chain68')
    rb, mk, pos0 = ag.rotors(c), np.asarray(c['mask_rotate'], bool), np.asarray(c['lig_pos'], np.float32)
    rng = np.random.default_rng(11)
    target = (pos0.astype(np.float64) @ _rotations(rng, 1)[0].T + 0.3 * rng.normal(size=pos0.shape) + 5.0).astype(np.float32)
    tor = np.stack([rng.normal(size=len(rb)), np.zeros(len(rb))]).astype(np.float32)
    rmsd, status = ctx.conformer_rmsd(pos0, target, rb, mk, tor, return_status=True)
    out += [('rmsd.chain68.rmsd', rmsd), ('rmsd.chain68.status', status)]
    for lig in ('chain4', 'branched'):
        c = ag.ligand(lig)
        rb, mk, pos0 = ag.rotors(c), np.asarray(c['mask_rotate'], bool), np.asarray(c['lig_pos'], np.float32)
        rng = np.random.default_rng(len(pos0))
        turned = ag.host_update(c, pos0[None], np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), rng.uniform(-np.pi, np.pi, size=(1, len(rb))).astype(np.float32))[0]
        target = (turned.astype(np.float64) @ _rotations(rng, 1)[0].T + 0.15 * rng.normal(size=pos0.shape) + 5.0).astype(np.float32)
        for name, opt in MATCH.items():
            res = ctx.match_conformer(pos0, target, rb, mk, n_islands=1, seed=5, **opt)
            out += [(f'match.{lig}.{name}.{k}', v) for k, v in res.items()]
    return out


def outputs(dev):
    """every (name, device tensor) of every case, in a fixed order"""
    from disco_diffdock_amd.tensor_layers import _shape_context
    ctx = _shape_context(0)
    out = _se3_update(dev, ctx) + _batch(dev, ctx) + _sample(dev) + _guided(dev) + _randomize(dev, ctx) + _matching(dev, ctx)
    torch.cuda.synchronize()
    return out


def digests(dev):
    d = {}
    for name, t in outputs(dev):
        assert name not in d and t.dtype in (torch.float32, torch.int32), name
        d[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit the file is generated at (recorded in the file)')
    ap.add_argument('--out', default=PATH)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the digests come from the device entry points: a MI355X is needed'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    dev = torch.device('cuda:0')
    d, again = digests(dev), digests(dev)
    unstable = [k for k in d if d[k] != again[k]]
    assert not unstable, f'not identical run to run, to be left out of the cases: {unstable}'
    with open(a.out, 'w') as f:
        json.dump({'generated_at_commit': a.commit, 'hip': torch.version.hip, 'sha256': d}, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{a.out}: {len(d)} digests')


if __name__ == '__main__':
    main()
