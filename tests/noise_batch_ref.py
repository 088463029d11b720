"""fp64 restatement of the ragged batch forms of the forward diffusion and of the score-matching loss (include/ddk.h: ddk_rng_perturbation_batch,
ddk_modify_conformer_batch, ddk_score_matching_loss_batch and its backward; disco_diffdock_amd.training.noise_batch / loss_function), built on
tests/noising_ref.py (the draws, the targets and the per-sample loss), tests/adversarial_geometry.py (oracle.sampler_ref.modify_conformer_batch per ligand)
and a transcription of the reference's loss_function (utils/training.py:14-61) for a batch of different complexes at different times.

The semantics of the ragged loss, as the reference has them:
  apply_mean=False  per graph: tr / rot the mean over the graph's 3 components; the torsion term the sum of the graph's per-torsion terms divided by
                    R_g + 1e-4 (an index_add of the terms and of the counts, then c + 0.0001): a graph without torsions gets 0 / 1e-4 = 0
  apply_mean=True   tr / rot the mean over all (G, 3) entries, 0-d; the torsion term the mean over ALL T torsions of the batch (NOT the mean of the
                    per-graph values), shape [1]; with no_torsion zeros of shape [1] ([G] without apply_mean).  (With T = 0 the reference's mean of an
                    empty tensor is NaN; the project returns 0 there, as it does for no_torsion, and the transcription below does the same.)
Every torsion of graph g carries the graph's own tor_sigma (tor_sigma_edge), so the torus norm is one number per graph."""
import numpy as np
import torch

import noising_ref as nr

TIMES = (0.05, 0.3, 0.6, 0.95)
STANDING = ((70, 22, None), (0, 20, None), (60, 35, 0), (64, 30, 1))      # (seed, residues, rotors kept or None = all) of synthetic.make_complex(n_lig=12)


def with_rotors(c, keep):
    """a copy of the complex dict with only its first ``keep`` rotatable bonds left rotatable (0: a rigid ligand, an empty mask_rotate)"""
    c = dict(c)
    em = np.asarray(c['edge_mask']).astype(bool).copy()
    on = np.flatnonzero(em)
    em[on[keep:]] = False
    c['edge_mask'] = em
    c['mask_rotate'] = np.asarray(c['mask_rotate']).reshape(len(on), -1)[:keep].copy()
    c['name'] = f"{c['name']}_r{keep}"
    return c


def standing_batch():
    """the four complexes every test of the batch ops runs on: 20..40 residues, ligands of different atom counts, rotor counts 4, >= 5, 0 and 1"""
    from disco_diffdock_amd import synthetic
    cs = []
    for seed, n_res, keep in STANDING:
        c = synthetic.make_complex(seed, n_res=n_res, n_lig=12)
        cs.append(c if keep is None else with_rotors(c, keep))
    return cs


def rotor_counts(cs):
    return [int(np.asarray(c['edge_mask']).astype(bool).sum()) for c in cs]


def rot_bonds(c):
    return np.asarray(c['bond_index'])[:, np.asarray(c['edge_mask']).astype(bool)].T.reshape(-1, 2)


def prefix(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


_rows = {}


def so3_row(eps_idx):
    if eps_idx not in _rows:
        _rows[eps_idx] = nr.so3_row(eps_idx)
    return _rows[eps_idx]


def perturbation_batch(seed, streams, samples, draw, rotors, tr_sigma, tor_sigma, torus_idx, eps_idx):
    """graph g = nr.perturbation of the one sample samples[g] of stream streams[g] at g's own noise level: dict of fp64 arrays, tr / rot [G, 3], tor flat [T]"""
    out = {k: [] for k in ('tr_update', 'rot_update', 'tor_update', 'tr_score', 'rot_score', 'tor_score')}
    for g in range(len(streams)):
        row = so3_row(int(eps_idx[g]))
        p = nr.perturbation(*nr.perturbation_words(seed, streams[g], int(samples[g]), 1, draw, int(rotors[g])), tr_sigma[g], tor_sigma[g], int(torus_idx[g]),
                            row['cdf'], row['score'])
        for k in out:
            out[k].append(p[k].reshape(-1, 3) if not k.startswith('tor') else p[k].reshape(-1))
    return {k: np.concatenate(v) for k, v in out.items()}


def modify_conformer_batch(cs, tr, rot, tor, tor_ptr):
    """oracle.sampler_ref.modify_conformer_batch in fp64 per ligand on the given updates: list of [n_g, 3] arrays"""
    import adversarial_geometry as ag
    out = []
    for g, c in enumerate(cs):
        pos = np.asarray(c['lig_pos'], np.float32)[None]
        t = np.asarray(tor[tor_ptr[g]:tor_ptr[g + 1]])[None]
        out.append(ag.update_ref(c, pos, np.asarray(tr[g])[None], np.asarray(rot[g])[None], t if t.size else None)[0])
    return out


def loss_batch(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2, tor_ptr):
    """[G, 6] fp64: row g = nr.score_matching_loss of the one sample with g's scalars and g's torsions"""
    G = len(tr_sigma)
    rows = []
    for g in range(G):
        a, b = int(tor_ptr[g]), int(tor_ptr[g + 1])
        tp = None if tor_pred is None or a == b else np.asarray(tor_pred)[a:b][None]
        ts = np.zeros((1, 0)) if tor_score is None else np.asarray(tor_score)[a:b][None]
        rows.append(nr.score_matching_loss(np.asarray(tr_pred)[g:g + 1], np.asarray(rot_pred)[g:g + 1], tp, np.asarray(tr_score)[g:g + 1],
                                           np.asarray(rot_score)[g:g + 1], ts, tr_sigma[g], so3_norm[g], torus_norm2[g])[0])
    return np.stack(rows)


def loss_batch_torch(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2, tor_ptr):
    """the three loss columns [G, 3] of ``loss_batch`` as differentiable fp64 torch (the scalars rounded to fp32 first, as the device holds them)"""
    f = lambda v: torch.as_tensor(np.asarray(v, np.float32).astype(np.float64))
    s, n, n2 = f(tr_sigma), f(so3_norm), f(torus_norm2)
    tr = ((tr_pred - tr_score) ** 2 * s[:, None] ** 2).mean(dim=1)
    rot = (((rot_pred - rot_score) / n[:, None]) ** 2).mean(dim=1)
    tor = []
    for g in range(len(s)):
        a, b = int(tor_ptr[g]), int(tor_ptr[g + 1])
        tor.append(((tor_pred[a:b] - tor_score[a:b]) ** 2 / n2[g]).sum() / ((b - a) + 0.0001) if tor_pred is not None else torch.zeros((), dtype=torch.float64))
    return torch.stack([tr, rot, torch.stack(tor)], dim=1)


def reference_loss_function(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2, tor_ptr, apply_mean=True,
                            no_torsion=False, tr_weight=1, rot_weight=1, tor_weight=1):
    """utils/training.py:14-61 on a ragged batch, in fp64 torch on host arrays: the 7-tuple (loss, tr_loss, rot_loss, tor_loss, tr_base_loss,
    rot_base_loss, tor_base_loss).  Per-EDGE torus norms (the graph's, repeated over its torsions), an index_add of terms and counts for
    apply_mean=False, the mean over all torsions for apply_mean=True."""
    f = lambda v: torch.as_tensor(np.asarray(v, np.float64))
    f32 = lambda v: torch.as_tensor(np.asarray(v, np.float32).astype(np.float64))
    tr_pred, rot_pred, tr_score, rot_score = f(tr_pred), f(rot_pred), f(tr_score), f(rot_score)
    G = tr_score.shape[0]
    dims = (0, 1) if apply_mean else 1
    sigma = f32(tr_sigma).unsqueeze(-1)
    tr_loss = ((tr_pred - tr_score) ** 2 * sigma ** 2).mean(dim=dims)
    tr_base = (tr_score ** 2 * sigma ** 2).mean(dim=dims)
    norm = f32(so3_norm).unsqueeze(-1)
    rot_loss = (((rot_pred - rot_score) / norm) ** 2).mean(dim=dims)
    rot_base = ((rot_score / norm) ** 2).mean(dim=dims)
    counts = np.diff(np.asarray(tor_ptr))
    T = int(counts.sum())
    if no_torsion or tor_pred is None or T == 0:
        tor_loss = tor_base = torch.zeros(1 if apply_mean else G, dtype=torch.float64)
    else:
        edge_norm2 = f32(np.repeat(np.asarray(torus_norm2, np.float32), counts))
        tor_pred, tor_score = f(tor_pred).reshape(-1), f(tor_score).reshape(-1)
        per_edge, per_edge_base = (tor_pred - tor_score) ** 2 / edge_norm2, tor_score ** 2 / edge_norm2
        if apply_mean:
            tor_loss, tor_base = per_edge.mean() * torch.ones(1, dtype=torch.float64), per_edge_base.mean() * torch.ones(1, dtype=torch.float64)
        else:
            index = torch.as_tensor(np.repeat(np.arange(G), counts))
            c = torch.zeros(G, dtype=torch.float64).index_add_(0, index, torch.ones(T, dtype=torch.float64)) + 0.0001
            tor_loss = torch.zeros(G, dtype=torch.float64).index_add_(0, index, per_edge) / c
            tor_base = torch.zeros(G, dtype=torch.float64).index_add_(0, index, per_edge_base) / c
    loss = tr_loss * tr_weight + rot_loss * rot_weight + tor_loss * tor_weight
    return loss, tr_loss, rot_loss, tor_loss, tr_base, rot_base, tor_base


def batch_mean_from_rows(rows, tor_ptr):
    """what loss_function(apply_mean=True) makes of the [G, 6] rows: the means over G, and for the two torsion columns sum_g row * (R_g + 1e-4) / T (0 if T = 0)"""
    rows = np.asarray(rows, np.float64)
    counts = np.diff(np.asarray(tor_ptr)).astype(np.float64)
    T = counts.sum()
    out = rows.mean(axis=0)
    for k in (2, 5):
        out[k] = (rows[:, k] * (counts + 1e-4)).sum() / T if T else 0.0
    return out


def ema_update(shadow, params, decay, num_updates):
    """one update of utils/utils.py's ExponentialMovingAverage in fp64 numpy: (new shadow list, new num_updates)"""
    d = decay
    if num_updates is not None:
        num_updates += 1
        d = min(decay, (1 + num_updates) / (10 + num_updates))
    return [s - (1.0 - d) * (s - p) for s, p in zip(shadow, params)], num_updates
