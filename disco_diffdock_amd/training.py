"""The forward half of the diffusion, the score-matching loss and the training loop: the reference's validation pass (test_epoch, utils/training.py) for a
loaded checkpoint (``validation_loss``) and for the trainable classes (``test_epoch``), its sampling validation (``inference_epoch`` through
``inference_engine``), and its training pass (train_epoch) for a ``train_model.TrainableScoreModel``: ``noise_batch`` is NoiseTransform.apply_noise per complex
at its own time followed by collation, ``draw_times`` the times, ``train_epoch`` utils/training.py:96-135, ``ExponentialMovingAverage`` utils/utils.py:117-.
``noise_complex`` is NoiseTransform.apply_noise (datasets_utils/pdbbind.py:40-57) for B copies of a complex at a common t, ``loss_function`` is
utils/training.py:14-61, ``validation_loss`` runs noise -> score model -> loss over complexes and noise levels.  Every draw comes from the counter-based generator (ddk_rng_perturbation), so a validation number is a pure function of (checkpoint, complexes, seed).
All compute is in libddk.so (csrc/k_so3.hip, csrc/k_noising.hip and the score model); the host holds scalars."""
import collections
import contextlib
import os

import numpy as np
import torch

from .diffusion_utils import t_to_sigma
from . import data as _data
from .runtime import _DATA, LOSS_COLUMNS, NOISE_BATCH_MAX_LIG, NOISE_BATCH_MAX_ROT, Complex, Context, h2d_async, stream_id

# utils/so3.py and utils/torus.py: the grids of the two noise-level tables
SO3_MIN_EPS, SO3_MAX_EPS, SO3_N_EPS = 0.01, 2, 1000
TORUS_SIGMA_MIN, TORUS_SIGMA_MAX, TORUS_SIGMA_N = 3e-3, 2, 5000

# what ``noise_complex`` hands to ``loss_function``: the score targets [B, 3], [B, 3], [B, n_rot] (device; tor_score None on a no_torsion model), the
# three sigmas and t (host floats), and the updates that made the poses
Targets = collections.namedtuple('Targets', ('tr_score', 'rot_score', 'tor_score', 'tr_sigma', 'rot_sigma', 'tor_sigma', 't',
                                             'tr_update', 'rot_update', 'tor_update'))

# what ``noise_batch`` hands to ``loss_function``: G graphs, each at its own time.  tr_score / rot_score / tr_update / rot_update [G, 3]; tor_score / tor_update
# flat [T] with the prefix tor_ptr [G + 1] (int32) of the rotor counts (tor_score None on a no_torsion model); the three sigmas, t, so3_score_norm =
# so3.score_norm(rot_sigma) and torus_score_norm2 = torus.score_norm(tor_sigma) float32 [G]: all device tensors.  rotors: the R_g as a HOST tuple (shapes).
BatchTargets = collections.namedtuple('BatchTargets', ('tr_score', 'rot_score', 'tor_score', 'tr_sigma', 'rot_sigma', 'tor_sigma', 't', 'tor_ptr',
                                                       'tr_update', 'rot_update', 'tor_update', 'so3_score_norm', 'torus_score_norm2', 'rotors'))


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


_host_context = None


def _host_ctx():
    """a host-only context for the calls that launch nothing (ddk_rng_forward_times)"""
    global _host_context
    if _host_context is None:
        _host_context = Context(device=-1)
    return _host_context


def draw_times(names, seed, draw, alpha=1, beta=1):
    """The diffusion time t in [0, 1) of each complex of ``names`` for noising ``draw`` under ``seed``: a float32 host array, a pure function of (name, seed,
    draw) (generator purpose 11, ddk_rng_forward_times; computed on the host).  NoiseTransform draws t ~ Beta(alpha, beta); only the reference's default
    alpha = beta = 1, the uniform, is covered."""
    for option, v in (('alpha', alpha), ('beta', beta)):
        if float(v) != 1.0:
            raise NotImplementedError(f'ddk: draw_times covers sampling_{option} = 1 only (t uniform on [0, 1)), got {option} = {v}')
    return _host_ctx().forward_times(seed, [stream_id(n) for n in names], draw=draw)


def draw_latent_keep(complexes, rate, seed, draw, samples=None):
    """The keep flags of the latent dropout (classifier-free guidance training, models/model_classes.py:70-76) for one batch: a float32 host array [G] of
    1.0 / 0.0, complex g kept iff the uniform of generator purpose 12 for (seed, stream_id(name_g), samples[g], draw) is at or above ``rate``
    (ddk_rng_latent_keep; computed on the host): a pure function of (name, seed, draw, sample), whatever the batch."""
    names = [c.get('name') if hasattr(c, 'get') else c for c in complexes]
    if any(n is None for n in names):
        raise ValueError('ddk: draw_latent_keep needs complexes with a name (the stream id is runtime.stream_id(name))')
    samples = [0] * len(names) if samples is None else [int(s) for s in samples]
    if len(samples) != len(names):
        raise ValueError(f'ddk: draw_latent_keep: samples must hold one index per complex ({len(names)}), got {len(samples)}')
    ctx = _host_ctx()
    out = np.empty(len(names), np.float32)
    for s in sorted(set(samples)):      # (one call per distinct sample index: usually one)
        at = [i for i, v in enumerate(samples) if v == s]
        out[at] = ctx.latent_keep(seed, [stream_id(names[i]) for i in at], rate, draw=draw, sample=s)
    return out


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x, z ^ (z >> 31)


def epoch_permutation(n, seed, epoch):
    """The order in which ``train_epoch`` visits n complexes: a permutation of range(n) that is a pure function of (n, seed, epoch), in integer arithmetic
    only (a Fisher-Yates shuffle fed by splitmix64 from the state seed ^ splitmix64(epoch); the modulo bias of 64-bit words is below 2^-40 for any list
    that fits in memory), so it is the same on every host and library version."""
    state = (int(seed) ^ _splitmix64(int(epoch) & 0xFFFFFFFFFFFFFFFF)[1]) & 0xFFFFFFFFFFFFFFFF
    order = list(range(int(n)))
    for i in range(len(order) - 1, 0, -1):
        state, word = _splitmix64(state)
        j = word % (i + 1)
        order[i], order[j] = order[j], order[i]
    return order


def _pack(arrays):
    """host arrays -> one uint8 buffer with every array at a multiple of 16 bytes, and their (offset, dtype, shape)"""
    at, parts, where = 0, [], []
    for a in arrays:
        a = np.ascontiguousarray(a)
        where.append((at, a.dtype, a.shape, a.nbytes))
        pad = (-a.nbytes) % 16
        parts.append(a.reshape(-1).view(np.uint8))
        if pad:
            parts.append(np.zeros(pad, np.uint8))
        at += a.nbytes + pad
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), where


_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def noise_batch(model, complexes, t, seed, draw=0, samples=None):
    """NoiseTransform.apply_noise (datasets_utils/pdbbind.py:35-57) for G DIFFERENT complexes, complex g at its own time ``t[g]``, and their collation:
    returns (data, :data:`BatchTargets`).  ``complexes``: the dicts ``runtime.Complex`` takes, with 'name', 'lig_pos', 'edge_mask', 'mask_rotate'; ``t``:
    G host floats in [0, 1]; ``samples``: G global sample indices (default 0).  Graph g is sample ``samples[g]`` of stream ``stream_id(name_g)`` under
    ``seed`` and ``draw``, so its pose and targets do not depend on the rest of the batch, and a complex may appear twice with different samples.
    ``data`` is a ``data.collate`` batch on the model's device in the layout ``TrainableScoreModel.forward`` documents, with the noised ``data['ligand'].pos``,
    the true poses in ``data['ligand'].orig_pos_torch`` and ``data.complex_t`` (set_time's graph-level part).  Every per-graph table goes up in ONE copy; then ddk_rng_perturbation_batch and
    ddk_modify_conformer_batch, one launch each (the IGSO(3) table is computed once per context).  Nothing is read back: what the device would report as a
    status (a bond outside its ligand, a coordinate that is not finite, a ligand over a limit) is checked here on the host first and raises."""
    ctx = _ctx_of(model)
    G = len(complexes)
    if G < 1:
        raise ValueError('ddk: noise_batch needs at least one complex')
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if t.size != G:
        raise ValueError(f'ddk: noise_batch: t must hold one time per complex ({G}), got {t.size}')
    if not (np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all()):
        raise ValueError(f'ddk: noise_batch: every t must be in [0, 1], got {t.tolist()}')
    samples = np.zeros(G, np.int64) if samples is None else np.asarray(samples, dtype=np.int64).reshape(-1)
    if samples.size != G or (samples < 0).any() or (samples >= (1 << 31) - 1).any():
        raise ValueError(f'ddk: noise_batch: samples must hold one index in [0, 2^31 - 1) per complex ({G}), got {samples.tolist()}')
    no_torsion = bool(getattr(model, 'no_torsion', ctx.cfg.no_torsion))      # (a TrainableScoreModel says so itself; its context is shared)
    so3_tab, torus_tab = _score_norm_tables(ctx)
    streams, pos, bonds, masks, rotors, atoms, sig, idx, norms = [], [], [], [], [], [], [], [], []
    for g, c in enumerate(complexes):
        name = c.get('name') if hasattr(c, 'get') else None
        if name is None:
            raise ValueError(f'ddk: noise_batch needs complexes with a name (complex {g} has none; its stream id is runtime.stream_id(name))')
        p = np.asarray(c['lig_pos'], dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        if not 1 <= n <= NOISE_BATCH_MAX_LIG:
            raise ValueError(f'ddk: noise_batch: n_lig of complex {g} ({name!r}) must be in [1, {NOISE_BATCH_MAX_LIG}], got {n}')
        if not np.isfinite(p).all():
            raise ValueError(f'ddk: noise_batch: lig_pos of complex {g} ({name!r}) has a coordinate that is not finite')
        em = np.asarray(c['edge_mask']).astype(bool).reshape(-1)
        mr = np.asarray(c['mask_rotate']).astype(np.uint8).reshape(-1, n) if np.size(c['mask_rotate']) else np.zeros((0, n), np.uint8)
        uv = np.asarray(c['bond_index'], dtype=np.int64)[:, em].T.reshape(-1, 2)
        if mr.shape[0] != uv.shape[0]:
            raise ValueError(f'ddk: noise_batch: complex {g} ({name!r}) has {uv.shape[0]} rotatable bonds in edge_mask and {mr.shape[0]} rows in mask_rotate')
        if no_torsion:
            mr, uv = mr[:0], uv[:0]
        R = uv.shape[0]
        if R > NOISE_BATCH_MAX_ROT:
            raise ValueError(f'ddk: noise_batch: R_g of complex {g} ({name!r}) must be in [0, {NOISE_BATCH_MAX_ROT}], got {R}')
        if R and ((uv < 0).any() or (uv >= n).any() or (uv[:, 0] == uv[:, 1]).any()):
            raise ValueError(f'ddk: noise_batch: a rotatable bond of complex {g} ({name!r}) has an atom index outside [0, {n}) or joins an atom to itself')
        s3 = _sigmas(ctx, float(t[g]))
        e_idx, t_idx = int(so3_eps_index(s3[1])), int(torus_sigma_index(s3[2]))
        streams.append(stream_id(name)); pos.append(p); bonds.append(uv.astype(np.int32)); masks.append(mr.reshape(-1)); rotors.append(R); atoms.append(n)
        sig.append(s3); idx.append((e_idx, t_idx)); norms.append((so3_tab[e_idx], torus_tab[t_idx]))
    prefix = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    node_ptr, tor_ptr, mask_ptr = prefix(atoms), prefix(rotors), prefix([r * n for r, n in zip(rotors, atoms)])
    T = int(tor_ptr[-1])
    sig, idx, norms = np.asarray(sig, np.float32), np.asarray(idx, np.int32), np.asarray(norms, np.float32)
    host = [np.asarray(streams, np.uint64).view(np.int64), np.concatenate(pos), node_ptr, tor_ptr, mask_ptr, samples.astype(np.int32), idx[:, 0].copy(),
            idx[:, 1].copy(), sig[:, 0].copy(), sig[:, 1].copy(), sig[:, 2].copy(), t.astype(np.float32), norms[:, 0].copy(), norms[:, 1].copy(),
            np.concatenate(bonds).reshape(-1, 2), np.concatenate(masks)]
    buf, where = _pack(host)
    dev = torch.device('cuda', ctx.device)
    dbuf = h2d_async(torch.from_numpy(buf), dev)      # the one copy
    (d_streams, d_pos, d_node, d_tor, d_mask_ptr, d_samples, d_eps, d_tidx, d_tr_sigma, d_rot_sigma, d_tor_sigma, d_t, d_so3_norm, d_torus_norm2, d_bonds,
     d_masks) = (dbuf[at:at + nbytes].view(_TORCH_OF[dt]).reshape(shape) for at, dt, shape, nbytes in where)
    cdf, score = ctx.so3_table()
    p = ctx.rng_perturbation_batch(seed, d_streams, d_samples, d_tor, d_tr_sigma, d_tor_sigma, d_tidx, d_eps, cdf, score, draw=draw, T=T)
    noised = ctx.modify_conformer_batch(d_pos, d_node, d_bonds, d_masks, d_mask_ptr, d_tor, p.tr_update, p.rot_update, p.tor_update if T else None, T=T)
    batch = _data.collate([_data.from_arrays(c) for c in complexes]).to(dev)
    batch['ligand'].pos = noised
    batch['ligand'].orig_pos_torch = d_pos      # the true poses, as uploaded: what the oracle latent encoder reads (latent_encoder.TPEncoder)
    batch.complex_t = {k: d_t for k in ('tr', 'rot', 'tor')}
    targets = BatchTargets(p.tr_score, p.rot_score, None if no_torsion else p.tor_score, d_tr_sigma, d_rot_sigma, d_tor_sigma, d_t, d_tor, p.tr_update,
                           p.rot_update, p.tor_update, d_so3_norm, d_torus_norm2, tuple(rotors))
    return batch, targets


class _ScoreMatchingLossBatch(torch.autograd.Function):
    """ddk_score_matching_loss_batch for predictions that ask for a gradient; the backward is ddk_score_matching_loss_batch_backward, element-wise (the
    base columns do not depend on the predictions)."""

    @staticmethod
    def forward(fctx, ctx, tg, tr_pred, rot_pred, tor_pred):
        fctx.save_for_backward(tr_pred, rot_pred, tor_pred)
        fctx.ddk = (ctx, tg)
        return ctx.score_matching_loss_batch(tr_pred, rot_pred, tor_pred, tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_sigma, tg.so3_score_norm,
                                             tg.torus_score_norm2, tg.tor_ptr, sum(tg.rotors))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g):
        tr_pred, rot_pred, tor_pred = fctx.saved_tensors
        ctx, tg = fctx.ddk
        need = (fctx.needs_input_grad[2], fctx.needs_input_grad[3], tor_pred is not None and fctx.needs_input_grad[4])
        grads = ctx.score_matching_loss_batch_backward(g[:, :3], tr_pred, rot_pred, tor_pred, tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_sigma,
                                                       tg.so3_score_norm, tg.torus_score_norm2, tg.tor_ptr, sum(tg.rotors), need=need)
        like = lambda d, p: None if d is None else d.reshape(p.shape).to(p.dtype)
        return (None, None) + tuple(like(d, p) for d, p in zip(grads, (tr_pred, rot_pred, tor_pred)))


def _loss_function_batch(tr_pred, rot_pred, tor_pred, tg, ctx, apply_mean, tr_weight, rot_weight, tor_weight):
    """loss_function for a :data:`BatchTargets`: per graph, the torsion term divided by R_g + 1e-4 (the reference's index_add of the per-edge terms and of
    the counts); with ``apply_mean`` the tr / rot means over (G, 3) and the torsion mean over ALL T torsions of the batch, [1], 0 when T = 0"""
    T = sum(tg.rotors)
    no_tor = tg.tor_score is None or tor_pred is None or T == 0
    args = (tr_pred, rot_pred, None if no_tor else tor_pred)
    if torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad for p in args):
        per = _ScoreMatchingLossBatch.apply(ctx, tg, *args)
    else:
        per = ctx.score_matching_loss_batch(*args, tg.tr_score, tg.rot_score, None if no_tor else tg.tor_score, tg.tr_sigma, tg.so3_score_norm,
                                            tg.torus_score_norm2, tg.tor_ptr, T)
    cols = [per[:, k] for k in range(len(LOSS_COLUMNS))]
    if apply_mean:
        G = per.shape[0]
        if no_tor:
            tor = tor_base = torch.zeros(1, dtype=per.dtype, device=per.device)
        else:      # the per-graph sums were divided by R_g + 1e-4: multiply back, add up over the graphs, divide by the count of all torsions
            w = (tg.tor_ptr[1:] - tg.tor_ptr[:-1]).to(per.dtype) + 1e-4
            tor, tor_base = ((cols[2] * w).sum() / T).reshape(1), ((cols[5] * w).sum() / T).reshape(1)
        cols = [cols[0].sum() / G, cols[1].sum() / G, tor, cols[3].sum() / G, cols[4].sum() / G, tor_base]
    tr_loss, rot_loss, tor_loss, tr_base, rot_base, tor_base = cols
    loss = tr_loss * tr_weight + rot_loss * rot_weight + tor_loss * tor_weight
    return loss, tr_loss, rot_loss, tor_loss, tr_base, rot_base, tor_base


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
    batch, as in the reference (the per-sample values divide by n_rot + 1e-4; the batch mean divides by the count).
    With the :data:`BatchTargets` of ``noise_batch`` the batch is ragged: G graphs, each with its own sigmas and its own number of torsions; the tensors are
    [G] each with ``apply_mean=False`` (ddk_score_matching_loss_batch, the score norms taken from the targets)."""
    ctx = _ctx_of(model)
    if isinstance(targets, BatchTargets):
        return _loss_function_batch(tr_pred, rot_pred, tor_pred, targets, ctx, apply_mean, tr_weight, rot_weight, tor_weight)
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


class ExponentialMovingAverage:
    """The moving average of a model's trainable parameters that the reference trains with (utils/utils.py:117-, after score_sde_pytorch's ema.py), in plain
    torch: shadow <- shadow - (1 - d) (shadow - p) after every optimizer step, with d = min(decay, (1 + k) / (10 + k)) at update k when
    ``use_num_updates``.  ``store`` / ``copy_to`` / ``restore`` swap the average in for validation and back."""

    def __init__(self, parameters, decay, use_num_updates=True):
        if not 0.0 <= decay <= 1.0:
            raise ValueError('Decay must be between 0 and 1')
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow_params = [p.detach().clone() for p in parameters if p.requires_grad]
        self.collected_params = []

    def update(self, parameters):
        d = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            d = min(d, (1 + self.num_updates) / (10 + self.num_updates))
        with torch.no_grad():
            for shadow, p in zip(self.shadow_params, [p for p in parameters if p.requires_grad]):
                shadow.sub_((1.0 - d) * (shadow - p))

    def copy_to(self, parameters):
        for shadow, p in zip(self.shadow_params, [p for p in parameters if p.requires_grad]):
            p.data.copy_(shadow.data)

    def store(self, parameters):
        self.collected_params = [p.detach().clone() for p in parameters]

    def restore(self, parameters):
        for kept, p in zip(self.collected_params, parameters):
            p.data.copy_(kept.data)

    def state_dict(self):
        return dict(decay=self.decay, num_updates=self.num_updates, shadow_params=self.shadow_params)

    def load_state_dict(self, state_dict, device=None):
        self.decay, self.num_updates = state_dict['decay'], state_dict['num_updates']
        self.shadow_params = [v.detach().clone() if device is None else v.to(device) for v in state_dict['shadow_params']]


TRAIN_METERS = ('loss',) + LOSS_COLUMNS


def _step_seed(seed, epoch, step):
    """the dropout seed of one training step: distinct 63-bit values for distinct (seed, epoch, step)"""
    return _splitmix64((_splitmix64((int(seed) ^ _splitmix64(int(epoch) & 0xFFFFFFFFFFFFFFFF)[1]) & 0xFFFFFFFFFFFFFFFF)[1] + int(step)) & 0xFFFFFFFFFFFFFFFF)[1] >> 1


def train_epoch(model, complexes, optimizer, batch_size, seed, epoch, ema=None, tr_weight=1, rot_weight=1, tor_weight=1):
    """One training epoch of a ``TrainableScoreModel`` over ``complexes`` (dicts as ``noise_batch`` takes): utils/training.py:96-135.  The complexes are
    visited in the order ``epoch_permutation(len(complexes), seed, epoch)`` in batches of ``batch_size``; complex i is noised at ``draw_times(names, seed,
    draw=epoch)[i]`` with draw = epoch, so every epoch sees every complex at a new time and a new noise, and the whole epoch is a pure function of (the
    model's state, complexes, seed, epoch).  Per batch: ``noise_batch`` -> ``model(data, seed=...)`` -> ``loss_function`` -> ``backward`` ->
    ``optimizer.step()`` -> ``ema.update``.  A ``train_model.LatentModelWrapper`` with a drop rate gets ``keep=draw_latent_keep(batch, rate, seed, epoch)``.
    A batch of one graph is skipped, as in the reference (BatchNorm needs two).  The seven meters are added up on
    the device and read back ONCE at the end; returns the reference's summary, {'loss', 'tr_loss', ...: the mean over the batches run} (NaN if none ran).
    The reference's out-of-memory loop, which retries a batch at 0.8 of its size, is not reproduced: an out-of-memory error is raised."""
    ctx = _ctx_of(model)
    model.train()
    from .train_model import LatentModelWrapper      # (here: train_model imports the layers, which import nothing of this module)
    latent = isinstance(model, LatentModelWrapper) and model.latent_droprate > 0
    order = epoch_permutation(len(complexes), seed, epoch)
    times = draw_times([c.get('name') if hasattr(c, 'get') else None for c in complexes], seed, epoch) if complexes else np.zeros(0, np.float32)
    total, ran = torch.zeros(len(TRAIN_METERS), dtype=torch.float64, device=torch.device('cuda', ctx.device)), 0
    for step, at in enumerate(range(0, len(order), int(batch_size))):
        ids = order[at:at + int(batch_size)]
        if len(ids) == 1:
            continue
        data, targets = noise_batch(model, [complexes[i] for i in ids], times[ids], seed, draw=epoch)
        optimizer.zero_grad()
        step_seed = _step_seed(seed, epoch, step)
        with torch.random.fork_rng(devices=[ctx.device]):      # the heads' nn.Dropout layers draw from torch's generators: seeded per step, then put back
            torch.manual_seed(step_seed)
            if latent:
                tr_pred, rot_pred, tor_pred = model(data, seed=step_seed, keep=draw_latent_keep([complexes[i] for i in ids], model.latent_droprate, seed, epoch))
            else:
                tr_pred, rot_pred, tor_pred = model(data, seed=step_seed)
        out = loss_function(tr_pred, rot_pred, tor_pred, targets, model, tr_weight=tr_weight, rot_weight=rot_weight, tor_weight=tor_weight)
        out[0].sum().backward()
        optimizer.step()
        if ema is not None:
            ema.update(model.parameters())
        total += torch.stack([v.detach().double().reshape(()) for v in out])
        ran += 1
    values = (total / ran).tolist() if ran else [float('nan')] * len(TRAIN_METERS)      # the one read-back
    return dict(zip(TRAIN_METERS, values))


def _names(complexes):
    return [c.get('name') if hasattr(c, 'get') else None for c in complexes]


@contextlib.contextmanager
def reproducible_evaluation(model):
    """inside: the model's conv layers evaluate with the training ops (``TensorProductConvLayer.eval_with_training_ops``), which use no atomics"""
    layers = [m for m in model.modules() if hasattr(m, 'eval_with_training_ops')]
    was = [m.eval_with_training_ops for m in layers]
    for m in layers:
        m.eval_with_training_ops = True
    try:
        yield
    finally:
        for m, w in zip(layers, was):
            m.eval_with_training_ops = w


def test_epoch(model, complexes, batch_size, seed, epoch=0, test_sigma_intervals=False):
    """The validation loss of a ``TrainableScoreModel`` or ``train_model.LatentModelWrapper`` over ``complexes`` (dicts as ``noise_batch`` takes):
    utils/training.py:138-177.  The model is put in ``.eval()`` (and left there, as in the reference; ``train_epoch`` sets ``.train()`` itself) and runs under
    ``torch.no_grad()``.  The complexes are taken in list order in batches of ``batch_size``; complex i is noised at ``draw_times(names, seed,
    draw=epoch)[i]`` with draw = epoch; step k's forward gets ``_step_seed(seed, epoch, k)`` (the oracle encoder's Gumbel noise) and, for a wrapper with a
    drop rate, ``keep=draw_latent_keep(batch, rate, seed, epoch)`` (the reference's wrapper drops latents in evaluation too, from torch's generator; here
    the flags follow the seed), then ``loss_function(apply_mean=False)``.  A batch of one graph is run: evaluation needs no batch statistics.  The conv
    layers evaluate with the training ops (dropout off, BatchNorm on its running buffers): the fused inference kernel they would otherwise run scatters
    with fp32 atomics (``ddk_conv_forward`` at the op boundary never takes the deterministic scatter), and the last bits of a loss would differ from
    run to run.  The trade: this is not the forward ``model.eval()`` alone gives; ``TensorProductConvLayer`` reads one more flag
    (``eval_with_training_ops``, at three places in tensor_layers.py, off outside this function), and the validation pass runs the training ops, which
    are slower than the inference kernel (their [E, 72] hidden rows and node-sorted edge lists are built as in training).  What it buys is a number that is
    the same on every run, so ``best_model.pt`` does not flip on an atomic's order.  The two routes agree to 8e-8 relative on every meter where measured
    (tests/test_gpu_validation_epochs.py holds them to 1e-5).  The
    result is a pure function of (the model's state, complexes, seed, epoch) at a given ``batch_size``.  The per-complex values of the seven meters stay
    on the device ([n, 7], fp64) and are read back ONCE; returned: the reference's unpooled means over the complexes, {'loss', 'tr_loss', ...} (NaN
    for an empty list), formed on the host in fp64 in list order.  (The sums themselves are not formed on the device: its scatter-add is an atomic
    and would give the mean's last bits an order of its own.)

    ``test_sigma_intervals``: also 'int{i}_{name}', i = 0 .. 9, the means over the complexes with floor(10 t) == i, NaN for an interval without one.
    The reference creates this second meter and never adds to it (its summary is 0 / 0 everywhere); here it is filled as described.

    The reference's out-of-memory branch, which skips a batch, is not reproduced: the error is raised."""
    ctx = _ctx_of(model)
    model.eval()
    from .train_model import LatentModelWrapper
    latent = isinstance(model, LatentModelWrapper) and model.latent_droprate > 0
    n, bs = len(complexes), int(batch_size)
    if bs < 1:
        raise ValueError(f'ddk: test_epoch: batch_size must be positive, got {batch_size}')
    times = draw_times(_names(complexes), seed, epoch) if n else np.zeros(0, np.float32)
    rows = torch.zeros((n, len(TRAIN_METERS)), dtype=torch.float64, device=torch.device('cuda', ctx.device))
    with torch.no_grad(), reproducible_evaluation(model):
        for step, at in enumerate(range(0, n, bs)):
            part = complexes[at:at + bs]
            data, targets = noise_batch(model, part, times[at:at + bs], seed, draw=epoch)
            step_seed = _step_seed(seed, epoch, step)
            if latent:
                tr_pred, rot_pred, tor_pred = model(data, seed=step_seed, keep=draw_latent_keep(part, model.latent_droprate, seed, epoch))
            else:
                tr_pred, rot_pred, tor_pred = model(data, seed=step_seed)
            out = loss_function(tr_pred, rot_pred, tor_pred, targets, model, apply_mean=False)
            rows[at:at + len(part)] = torch.stack([v.detach().double().reshape(-1) for v in out], dim=1)
    host = rows.cpu().numpy()      # the one read-back
    mean = lambda a: a.mean(axis=0).tolist() if len(a) else [float('nan')] * len(TRAIN_METERS)
    result = dict(zip(TRAIN_METERS, mean(host)))
    if test_sigma_intervals:
        interval = np.floor(10.0 * np.asarray(times, np.float64)).astype(np.int64)
        for i in range(10):
            result.update({f'int{i}_{k}': v for k, v in zip(TRAIN_METERS, mean(host[interval == i]))})
    return result


def inference_engine(model, args, engine=None):
    """The inference model of a trainable one: ``model_utils.get_model(args, ...)`` (built once: pass the returned object back as ``engine`` and only the
    weights are loaded again, into the same context) with ``model.state_dict()`` loaded ``strict=True`` - for a ``train_model.LatentModelWrapper`` both
    halves, the oracle encoder included.  ``args``: the model_parameters.yml Namespace the model was built from.  A reload drops the engine's cached
    complexes (their node embeddings were made with the old weights).  The packed weights of the loads before stay allocated until the context goes
    (``ddk_finalize_weights`` packs anew and frees nothing): measured 18.8 MB of device memory per reload for five conv layers with latent_dim 2, so a run
    that validates 80 times on one engine ends 1.5 GB up.  An engine that is dropped gives everything back; make a new one (``engine=None``) every few
    dozen reloads where that matters."""
    from functools import partial
    from .model_utils import get_model
    if engine is None:
        engine = get_model(args, torch.device('cuda', _ctx_of(model).device), partial(t_to_sigma, args=args), no_parallel=True)
    engine.load_state_dict(model.state_dict(), strict=True)
    return engine


def inference_epoch(model, complexes, args, seed, epoch=0, engine=None):
    """utils/training.py:180-231: sample ONE pose per complex with the model as it is now and count the poses under 2 and 5 A.  ``complexes``: dicts as
    ``train_epoch`` takes ('lig_pos' is the true pose in the receptor-centred frame); ``args``: the model's Namespace with ``inference_steps`` and, for a
    latent model, ``sampling_latent_temperature``; ``engine``: what ``inference_engine(model, args)`` returned earlier (the weights are loaded again), None:
    a new one.  Per complex i, with s = ``_step_seed(seed, epoch, i)``: ``sampling.randomize_position(seed=s)``, ``sampling.sampling(batch_size=1,
    ar_model=None, seed=s)`` - a latent model samples with ORACLE latents at ``args.sampling_latent_temperature`` - and the heavy-atom RMSD
    (``lig_x[:, 0] != 0``) to the true pose, on the device.  One read-back at the end.  Returns {'rmsds_lt2', 'rmsds_lt5'} in percent and the RMSDs
    themselves, a float64 array, under 'rmsds': a pure function of (the model's state, complexes, seed, epoch) on a deterministic context.  Without
    latents (``latent_dim`` 0) the same minus the encoder.  The reference retries a complex whose Kabsch SVD "failed to converge"; there is no SVD on
    this path (the alignment is closed-form on the device), so there is nothing to retry."""
    from functools import partial
    from .diffusion_utils import get_t_schedule
    from .sampling import randomize_position, sampling
    engine = inference_engine(model, args, engine)
    dev = torch.device('cuda', _ctx_of(model).device)
    sched = get_t_schedule(inference_steps=args.inference_steps)
    use_latent = int(getattr(args, 'latent_dim', 0)) > 0
    rmsds = torch.zeros(len(complexes), dtype=torch.float64, device=dev)
    for i, c in enumerate(complexes):
        s = _step_seed(seed, epoch, i)
        true = np.asarray(c['lig_pos'], np.float32).reshape(-1, 3)
        g = _data.from_arrays(c)
        g['ligand'].orig_pos_torch = torch.from_numpy(true.copy())
        graphs = [g]
        randomize_position(graphs, args.no_torsion, False, args.tr_sigma_max, device=dev, seed=s)
        graphs, _ = sampling(graphs, engine, args.inference_steps, sched, sched, sched, dev, partial(t_to_sigma, args=args), args, batch_size=1,
                             use_latent=use_latent, ar_model=None, seed=s, gumbel_latent_temperature=getattr(args, 'sampling_latent_temperature', 0.01))
        heavy = (np.asarray(c['lig_x'])[:, 0] != 0).astype(np.float32)
        ref = h2d_async(torch.from_numpy(np.concatenate([true, heavy[:, None]], axis=1)), dev)      # one copy: the true pose and the heavy-atom flags
        d2 = ((graphs[0]['ligand'].pos.detach().float() - ref[:, :3]) ** 2).sum(dim=1)
        rmsds[i] = ((d2 * ref[:, 3]).sum() / ref[:, 3].sum()).sqrt()
    host = rmsds.cpu().numpy()      # the one read-back
    n = max(len(host), 1)
    return {'rmsds_lt2': 100.0 * float((host < 2).sum()) / n, 'rmsds_lt5': 100.0 * float((host < 5).sum()) / n, 'rmsds': host}
