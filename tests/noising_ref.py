"""fp64 NumPy restatement of the forward diffusion and the score-matching loss (csrc/k_so3.hip, csrc/k_noising.hip; include/ddk.h: ddk_so3_rows,
ddk_torus_score, ddk_rng_perturbation, ddk_score_matching_loss), written from the formulas of the reference's utils/so3.py, utils/torus.py,
NoiseTransform.apply_noise (datasets_utils/pdbbind.py:40-57) and loss_function (utils/training.py:14-61).  The draws come from tests/philox_ref.py.

The IGSO(3) series can be summed with l ascending (the reference's order: it reproduces the shipped so3_exp_score_norms.npy bit for bit) or descending;
the disagreement of the two is the yardstick the device rows are measured with."""
import numpy as np

import philox_ref as pr

# ---- utils/so3.py ------------------------------------------------------------------------------------------------------------------------------------
MIN_EPS, MAX_EPS, N_EPS = 0.01, 2, 1000
X_N = 2000
L = 2000
omegas = np.linspace(0, np.pi, X_N + 1)[1:]
eps_array = 10 ** np.linspace(np.log10(MIN_EPS), np.log10(MAX_EPS), N_EPS)


def so3_eps_index(eps):
    """so3.py:70-71 (scaled by N_EPS, not N_EPS - 1, as there)"""
    idx = (np.log10(eps) - np.log10(MIN_EPS)) / (np.log10(MAX_EPS) - np.log10(MIN_EPS)) * N_EPS
    return np.clip(np.around(idx).astype(int), a_min=0, a_max=N_EPS - 1)


NOISE_GUARD = 2.0 ** -40      # ddk_so3_rows counts an entry in exp_score_norm only if |_expansion| > this * sum_l |term_l|


def so3_series(eps, omega=omegas, descending=False, with_amp=False):
    """(_expansion, _score) of so3.py:21-43 at the angles ``omega`` for one eps, every term as written there, summed over l in the given order; with_amp adds
    sum_l |term_l| of the expansion"""
    omega = np.asarray(omega, np.float64)
    p, d_sigma, amp = 0, 0, 0
    lo = np.sin(omega / 2)
    dlo = 1 / 2 * np.cos(omega / 2)
    with np.errstate(all='ignore'):
        for l in (range(L - 1, -1, -1) if descending else range(L)):
            w = (2 * l + 1) * np.exp(-l * (l + 1) * eps ** 2)
            hi = np.sin(omega * (l + 1 / 2))
            dhi = (l + 1 / 2) * np.cos(omega * (l + 1 / 2))
            p = p + w * hi / lo
            amp = amp + np.abs(w * hi / lo)
            d_sigma = d_sigma + w * (lo * dhi - hi * dlo) / lo ** 2
        return (p, d_sigma / p, amp) if with_amp else (p, d_sigma / p)


def so3_row(eps_idx, descending=False):
    """dict(pdf, cdf, score [2000], exp_score_norm) of row ``eps_idx`` of the reference's tables (so3.py:56-61); ``exp_score_norm_finite`` sums only the
    entries whose score is finite, ``exp_score_norm_guarded`` of those only the ones whose expansion stands above the rounding noise of its own sum (the rule
    of ddk_so3_rows)"""
    eps = eps_array[eps_idx]
    exp, score, amp = so3_series(eps, omegas, descending, with_amp=True)
    pdf = exp * (1 - np.cos(omegas)) / np.pi
    cdf = pdf.cumsum() / X_N * np.pi
    with np.errstate(all='ignore'):
        esn = np.sqrt(np.sum(score ** 2 * pdf) / np.sum(pdf) / np.pi)
        ok = np.isfinite(score)
        esn_finite = np.sqrt(np.sum(score[ok] ** 2 * pdf[ok]) / np.sum(pdf) / np.pi)
        ok &= np.abs(exp) > NOISE_GUARD * amp
        esn_guarded = np.sqrt(np.sum(score[ok] ** 2 * pdf[ok]) / np.sum(pdf) / np.pi)
    return dict(eps=eps, pdf=pdf, cdf=cdf, score=score, exp_score_norm=esn, exp_score_norm_finite=esn_finite, exp_score_norm_guarded=esn_guarded)


def live_set(pdf, rel=1e-6):
    """the comparison set of a row: pdf >= rel * max(pdf) -> (mask, is it one contiguous run, its share of sum |pdf|)"""
    m = pdf >= rel * pdf.max()
    idx = np.flatnonzero(m)
    return m, bool(idx.size and idx[-1] - idx[0] + 1 == idx.size), float(np.abs(pdf[m]).sum() / np.abs(pdf).sum())


def interp(x, xp, fp):
    """np.interp's arithmetic with the bracket ddk_rng_perturbation finds: j = the first xp[j] >= x by bisection; clamped at both ends"""
    n = len(xp)
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if xp[mid] >= x:
            hi = mid
        else:
            lo = mid + 1
    if lo == 0:
        return fp[0]
    if lo == n:
        return fp[n - 1]
    j = lo - 1
    return (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]) + fp[j]


def so3_score_vec(eps, vec):
    """so3.py:83-88 with the one row it needs computed on the spot"""
    vec = np.asarray(vec, np.float64)
    om = np.linalg.norm(vec)
    return np.interp(om, omegas, so3_row(int(so3_eps_index(eps)))['score']) * vec / om


# ---- utils/torus.py ----------------------------------------------------------------------------------------------------------------------------------
T_X_MIN, T_X_N = 1e-5, 5000
T_SIGMA_MIN, T_SIGMA_MAX, T_SIGMA_N = 3e-3, 2, 5000
T_N = 100
torus_x = 10 ** np.linspace(np.log10(T_X_MIN), 0, T_X_N + 1) * np.pi
torus_sigma = 10 ** np.linspace(np.log10(T_SIGMA_MIN), np.log10(T_SIGMA_MAX), T_SIGMA_N + 1) * np.pi


def torus_sigma_index(sigma):
    """torus.py:49-51"""
    s = np.log(np.asarray(sigma, np.float64) / np.pi)
    s = (s - np.log(T_SIGMA_MIN)) / (np.log(T_SIGMA_MAX) - np.log(T_SIGMA_MIN)) * T_SIGMA_N
    return np.round(np.clip(s, 0, T_SIGMA_N)).astype(int)


def torus_table_entry(x_idx, sigma_idx):
    """score_[sigma_idx, x_idx] of torus.py:36-40: grad / p with N = 100, the 201 terms summed in ascending i"""
    x, sigma = torus_x[np.asarray(x_idx)], torus_sigma[np.asarray(sigma_idx)]
    p, g = 0, 0
    with np.errstate(all='ignore'):
        for i in range(-T_N, T_N + 1):
            e = np.exp(-(x + 2 * np.pi * i) ** 2 / 2 / sigma ** 2)
            p = p + e
            g = g + (x + 2 * np.pi * i) / sigma ** 2 * e
        return g / p


def torus_score(x, sigma_idx):
    """torus.py:43-52 with the sigma index given: fp64, NaN where the table has NaN; x == 0 gives 0"""
    x = np.asarray(x, np.float64)
    x = (x + np.pi) % (2 * np.pi) - np.pi
    sign = np.sign(x)
    with np.errstate(all='ignore'):
        xi = np.log(np.abs(x) / np.pi)
        xi = (xi - np.log(T_X_MIN)) / (0 - np.log(T_X_MIN)) * T_X_N
        xi = np.round(np.clip(xi, 0, T_X_N)).astype(int)
        out = -sign * torus_table_entry(xi, np.broadcast_to(np.asarray(sigma_idx), x.shape))
    return np.where(x == 0, 0.0, out)


# ---- the forward draws and their targets (ddk_rng_perturbation) -------------------------------------------------------------------------------------
FORWARD_PURPOSE = dict(forward_translation=6, forward_rotation=7, forward_torsion=8)


def perturbation_words(seed, stream, sample0, B, draw, n_rot):
    """the raw draws in fp64: (z_tr [B, 3], a [B, 3], u [B] fp32 bit-exact, z_tor [B, n_rot])"""
    b = np.arange(B) + sample0
    z_tr = pr.normals64(pr.block(seed, stream, b, FORWARD_PURPOSE['forward_translation'], draw, 0))[:, :3]
    a = pr.normals64(pr.block(seed, stream, b, FORWARD_PURPOSE['forward_rotation'], draw, 0))[:, :3]
    u = pr.uniform32(pr.block(seed, stream, b, FORWARD_PURPOSE['forward_rotation'], draw, 1)[:, 0])
    n_blk = (n_rot + 3) // 4
    z_tor = pr.normals64(pr.block(seed, stream, b[:, None], FORWARD_PURPOSE['forward_torsion'], draw, np.arange(n_blk)[None, :])).reshape(B, 4 * n_blk)[:, :n_rot]
    return z_tr, a, u, z_tor


def perturbation(z_tr, a, u, z_tor, tr_sigma, tor_sigma, torus_sigma_idx, cdf_row, score_row):
    """apply_noise's updates and targets from the given draws: dict of fp64 arrays (the device rounds each once to fp32)"""
    tr_sigma, tor_sigma = np.float64(np.float32(tr_sigma)), np.float64(np.float32(tor_sigma))
    tr_update = tr_sigma * z_tr
    tr_score = -tr_update / tr_sigma ** 2
    B = len(u)
    rot_update, rot_score = np.zeros((B, 3)), np.zeros((B, 3))
    for b in range(B):
        n2 = float((a[b] * a[b]).sum())
        if n2 < 2.0 ** -60:
            continue
        omega = interp(float(u[b]), cdf_row, omegas)
        rot_update[b] = a[b] / np.sqrt(n2) * omega
        rot_score[b] = interp(omega, omegas, score_row) * rot_update[b] / omega
    tor_update = tor_sigma * z_tor
    tor_score = torus_score(tor_update.astype(np.float32), torus_sigma_idx)
    return dict(tr_update=tr_update, rot_update=rot_update, tor_update=tor_update, tr_score=tr_score, rot_score=rot_score, tor_score=tor_score)


# ---- loss_function(..., apply_mean=False) ------------------------------------------------------------------------------------------------------------
def score_matching_loss(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2):
    """[B, 6] fp64: tr_loss, rot_loss, tor_loss, tr_base_loss, rot_base_loss, tor_base_loss per sample (utils/training.py:21-53)"""
    f = lambda v: np.asarray(v, np.float64)
    s, n, n2 = (np.float64(np.float32(v)) for v in (tr_sigma, so3_score_norm, torus_score_norm2))
    tr_pred, rot_pred, tr_score, rot_score = f(tr_pred), f(rot_pred), f(tr_score), f(rot_score)
    B = tr_score.shape[0]
    out = np.zeros((B, 6))
    out[:, 0] = ((tr_pred - tr_score) ** 2 * s ** 2).mean(axis=1)
    out[:, 3] = (tr_score ** 2 * s ** 2).mean(axis=1)
    out[:, 1] = (((rot_pred - rot_score) / n) ** 2).mean(axis=1)
    out[:, 4] = ((rot_score / n) ** 2).mean(axis=1)
    if tor_pred is not None and np.size(tor_score):
        tor_pred, tor_score = f(tor_pred).reshape(B, -1), f(tor_score).reshape(B, -1)
        c = tor_score.shape[1] + 0.0001
        out[:, 2] = ((tor_pred - tor_score) ** 2 / n2).sum(axis=1) / c
        out[:, 5] = (tor_score ** 2 / n2).sum(axis=1) / c
    return out
