"""The forward half of the diffusion and the score-matching validation loss: the reference's validation pass (test_epoch, utils/training.py) for a
loaded checkpoint, without training.  ``noise_complex`` is NoiseTransform.apply_noise (datasets_utils/pdbbind.py:40-57) for B copies of a complex at a
common t, ``loss_function`` is utils/training.py:14-61, ``validation_loss`` runs noise -> score model -> loss over complexes and noise levels.  Every draw
comes from the counter-based generator (ddk_rng_perturbation), so a validation number is a pure function of (checkpoint, complexes, seed).
All compute is in libddk.so (csrc/k_so3.hip, csrc/k_noising.hip and the score model); the host holds scalars."""
import collections
import os

import numpy as np
import torch

from .diffusion_utils import t_to_sigma
from .runtime import _DATA, LOSS_COLUMNS, Complex, stream_id

# utils/so3.py and utils/torus.py: the grids of the two noise-level tables
SO3_MIN_EPS, SO3_MAX_EPS, SO3_N_EPS = 0.01, 2, 1000
TORUS_SIGMA_MIN, TORUS_SIGMA_MAX, TORUS_SIGMA_N = 3e-3, 2, 5000

# what ``noise_complex`` hands to ``loss_function``: the score targets [B, 3], [B, 3], [B, n_rot] (device; tor_score None on a no_torsion model), the
# three sigmas and t (host floats), and the updates that made the poses
Targets = collections.namedtuple('Targets', ('tr_score', 'rot_score', 'tor_score', 'tr_sigma', 'rot_sigma', 'tor_sigma', 't',
                                             'tr_update', 'rot_update', 'tor_update'))


def so3_eps_index(eps):
    """Row of the IGSO(3) tables for the noise level ``eps``: utils/so3.py:70-71 in fp64 (the index is scaled by N_EPS, not N_EPS - 1, as there)."""
    idx = (np.log10(eps) - np.log10(SO3_MIN_EPS)) / (np.log10(SO3_MAX_EPS) - np.log10(SO3_MIN_EPS)) * SO3_N_EPS
    return np.clip(np.around(idx).astype(int), a_min=0, a_max=SO3_N_EPS - 1)


def torus_sigma_index(sigma):
    """Row of the torus tables for ``sigma``: utils/torus.py:49-51 in fp64."""
    s = np.log(np.asarray(sigma, np.float64) / np.pi)
    s = (s - np.log(TORUS_SIGMA_MIN)) / (np.log(TORUS_SIGMA_MAX) - np.log(TORUS_SIGMA_MIN)) * TORUS_SIGMA_N
    return np.round(np.clip(s, 0, TORUS_SIGMA_N)).astype(int)


def _ctx_of(model):
    return model.ctx if hasattr(model, 'ctx') else model


def _sigmas(ctx, t):
    return tuple(float(v) for v in t_to_sigma(t, t, t, ctx.cfg))


def _score_norm_tables(ctx):
    tables = getattr(ctx, 'score_norm_tables', None)
    if tables is None:      # a context that never loaded a checkpoint: the shipped tables
        tables = (np.load(os.path.join(_DATA, 'so3_exp_score_norms.npy')), np.load(os.path.join(_DATA, 'torus_score_norm_seed0.npy')))
    return tables


def noise_complex(model, c, t, B, seed, draw=0, sample_offset=0, cx=None, so3_row=None):
    """apply_noise for B copies of the true pose ``c['lig_pos']`` at the common time ``t``: returns (pos [B, n_lig, 3] device tensor, :data:`Targets`).
    ``model``: a score model (or its ``runtime.Context``); ``c``: the complex dict ``runtime.Complex`` takes, with 'lig_pos' and 'name'; ``cx``: its
    ``Complex`` if the caller already has one (max_batch >= B); ``so3_row``: (cdf [2000], score [2000]) of this t's rot_sigma if the caller already has them
    (``validation_loss`` computes the rows of all its noise levels in one call: a lone row keeps one workgroup busy for 3 ms).  Sample b is the global sample ``sample_offset + b`` of stream ``stream_id(c['name'])``
    under ``seed``; ``draw`` numbers independent noisings of the same sample.  One ddk_so3_rows call (the one row of this rot_sigma), one
    ddk_rng_perturbation, one ddk_se3_update; nothing is read back."""
    ctx = _ctx_of(model)
    name = c.get('name') if hasattr(c, 'get') else None
    if name is None:
        raise ValueError('ddk: noise_complex needs a complex with a name (its stream id is runtime.stream_id(name))')
    if cx is None:
        cx = Complex(ctx, c, B)
    dev = torch.device('cuda', ctx.device)
    tr_sigma, rot_sigma, tor_sigma = _sigmas(ctx, float(t))
    no_torsion = bool(ctx.cfg.no_torsion)
    n_rot = 0 if no_torsion else cx.R
    if so3_row is None:
        cdf, score, _ = ctx.so3_rows([int(so3_eps_index(rot_sigma))], exp_score_norm=False)
        so3_row = (cdf[0], score[0])
    p = ctx.rng_perturbation(seed, stream_id(name), sample_offset, B, n_rot, tr_sigma, tor_sigma, int(torus_sigma_index(tor_sigma)), so3_row[0], so3_row[1],
                             draw=draw)
    pos0 = torch.as_tensor(np.asarray(c['lig_pos'], dtype=np.float32)).to(dev).reshape(1, cx.n_lig, 3).expand(B, -1, -1).contiguous()
    pos = cx.se3_update(pos0, p.tr_update, p.rot_update, p.tor_update.reshape(-1) if n_rot else None)
    tor_score = None if no_torsion else p.tor_score
    return pos, Targets(p.tr_score, p.rot_score, tor_score, tr_sigma, rot_sigma, tor_sigma, float(t), p.tr_update, p.rot_update, p.tor_update)


class _ScoreMatchingLoss(torch.autograd.Function):
    """ddk_score_matching_loss for predictions that ask for a gradient: the forward is the kernel, the backward the derivative of its three loss columns
    (the base columns do not depend on the predictions), written out element-wise: plain torch without reductions, so the same bits on every run.
      tr_loss[b] = mean_k (tr_pred - tr_score)^2 tr_sigma^2      rot_loss[b] = mean_k ((rot_pred - rot_score) / so3_norm)^2
      tor_loss[b] = sum_r (tor_pred - tor_score)^2 / torus_norm2 / (n_rot + 1e-4)"""

    @staticmethod
    def forward(fctx, ctx, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2):
        fctx.save_for_backward(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score)
        fctx.scalars = (float(tr_sigma), float(so3_norm), float(torus_norm2))
        return ctx.score_matching_loss(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g):
        tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score = fctx.saved_tensors
        tr_sigma, so3_norm, torus_norm2 = fctx.scalars
        B = g.shape[0]
        like = lambda d, p: d.reshape(p.shape).to(p.dtype)
        g_tr = g_rot = g_tor = None
        if fctx.needs_input_grad[1]:
            g_tr = like((tr_pred.reshape(B, 3).float() - tr_score.reshape(B, 3).float()) * (2.0 * tr_sigma * tr_sigma / 3.0) * g[:, 0:1], tr_pred)
        if fctx.needs_input_grad[2]:
            g_rot = like((rot_pred.reshape(B, 3).float() - rot_score.reshape(B, 3).float()) * (2.0 / (so3_norm * so3_norm * 3.0)) * g[:, 1:2], rot_pred)
        if tor_pred is not None and fctx.needs_input_grad[3]:
            n_rot = tor_score.numel() // max(B, 1)
            d = tor_pred.reshape(B, n_rot).float() - tor_score.reshape(B, n_rot).float()
            g_tor = like(d * (2.0 / (torus_norm2 * (n_rot + 1e-4))) * g[:, 2:3], tor_pred)
        return None, g_tr, g_rot, g_tor, None, None, None, None, None, None


def loss_function(tr_pred, rot_pred, tor_pred, targets, model, apply_mean=True, tr_weight=1, rot_weight=1, tor_weight=1):
    """utils/training.py:14-61 for one batch of ``noise_complex``: the 7-tuple (loss, tr_loss, rot_loss, tor_loss, tr_base_loss, rot_base_loss,
    tor_base_loss) of device tensors, [B] each with ``apply_mean=False`` and [1] (the reference's shapes: 0-d for tr / rot) with it.  The score norms
    are looked up on the host in the context's tables at the targets' sigmas.  With ``apply_mean`` the torsion term is the mean over ALL torsions of the
    batch, as in the reference (the per-sample values divide by n_rot + 1e-4; the batch mean divides by the count)."""
    ctx = _ctx_of(model)
    so3_tab, torus_tab = _score_norm_tables(ctx)
    so3_norm = float(np.float32(so3_tab[int(so3_eps_index(targets.rot_sigma))]))
    torus_norm2 = float(np.float32(torus_tab[int(torus_sigma_index(targets.tor_sigma))]))
    no_tor = targets.tor_score is None or tor_pred is None or targets.tor_score.numel() == 0
    args = (tr_pred, rot_pred, None if no_tor else tor_pred, targets.tr_score, targets.rot_score, None if no_tor else targets.tor_score, targets.tr_sigma,
            so3_norm, torus_norm2)
    if torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad for p in args[:3]):      # training: the same kernel, with a backward
        per = _ScoreMatchingLoss.apply(ctx, *args)
    else:
        per = ctx.score_matching_loss(*args)
    cols = [per[:, k] for k in range(len(LOSS_COLUMNS))]
    if apply_mean:
        B = per.shape[0]
        n_rot = 0 if no_tor else targets.tor_score.numel() // B
        # the per-sample torsion sums were divided by n_rot + 1e-4; the batch mean of the reference divides their total by B * n_rot
        undo = (n_rot + 1e-4) / n_rot if n_rot else 0.0
        cols = [cols[0].mean(), cols[1].mean(), (cols[2].mean() * undo).reshape(1), cols[3].mean(), cols[4].mean(), (cols[5].mean() * undo).reshape(1)]
    tr_loss, rot_loss, tor_loss, tr_base, rot_base, tor_base = cols
    loss = tr_loss * tr_weight + rot_loss * rot_weight + tor_loss * tor_weight
    return loss, tr_loss, rot_loss, tor_loss, tr_base, rot_base, tor_base


def validation_loss(model, complexes, t_values=None, samples_per_complex=8, seed=0):
    """The validation loss of a loaded checkpoint: for every complex of ``complexes`` (dicts as ``runtime.Complex`` takes, with 'lig_pos' and 'name') and
    every t of ``t_values`` (None: the midpoints of ten equal intervals of [0, 1]), ``samples_per_complex`` noisings -> ``Complex.score_forward`` ->
    ``loss_function(apply_mean=False)``.  Returns a dict: 'loss' and the six LOSS_COLUMNS as means over everything, 'per_t' = {t: the same seven means at
    that t}, 'n' = the number of noised poses.  The t of index k uses draw k, so the noise levels are independent noisings of the same samples.  One
    read-back per (complex, t)."""
    ctx = _ctx_of(model)
    t_values = [(k + 0.5) / 10 for k in range(10)] if t_values is None else [float(t) for t in t_values]
    B = int(samples_per_complex)
    keys = ('loss',) + LOSS_COLUMNS
    rows = {t: [] for t in t_values}
    cdf, score, _ = ctx.so3_rows([int(so3_eps_index(_sigmas(ctx, t)[1])) for t in t_values], exp_score_norm=False)      # every noise level's row, once
    for c in complexes:
        cx = Complex(ctx, c, B)
        for k, t in enumerate(t_values):
            pos, targets = noise_complex(model, c, t, B, seed, draw=k, cx=cx, so3_row=(cdf[k], score[k]))
            tr, rot, tor = cx.score_forward(pos, t, t, t)
            out = loss_function(tr, rot, None if targets.tor_score is None else tor, targets, model, apply_mean=False)
            rows[t].append(torch.stack(out, dim=1).double().cpu().numpy())      # [B, 7]
        cx.close()
    per_t = {t: dict(zip(keys, np.concatenate(v).mean(axis=0).tolist())) for t, v in rows.items() if v}
    every = np.concatenate([np.concatenate(v) for v in rows.values() if v]) if per_t else np.zeros((0, 7))
    out = dict(zip(keys, every.mean(axis=0).tolist())) if len(every) else {k: float('nan') for k in keys}
    out.update(per_t=per_t, n=int(len(every)))
    return out
