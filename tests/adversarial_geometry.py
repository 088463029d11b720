"""Adversarial geometry for the pose-update kernels of csrc/k_se3.hip (axis_angle_to_matrix_dev, horn_rotation / kabsch_block, se3_update_kernel,
randomize_kernel, pose_metrics_kernel): seeded generators that return their inputs together with the properties they claim, the fp64 references,
the one definition of the tolerance, and a host restatement of the kernel's update in numpy fp32.  Plain helper module (no fixtures, no GPU import):
shared by tests/test_geometry_bound.py (CPU) and tests/test_gpu_geometry_adversarial.py.

THE BAR.  A fixed tolerance is blind on a 4-atom ligand at the origin (the fp32 reference is 3e-7 A from fp64 there) and false on a 256-atom chain
150 A out (9e-3 A), so every comparison is held to what fp32 can do ON THAT INPUT:

    bar(err32, scale) = max(K * err32, FLOOR * scale),      K = 4,  FLOOR = 8 * 2^-24

err32 is the error of the fp32 reference (oracle/sampler_ref.py on float tensors) against the same reference on double tensors, computed on the host for
the very inputs the kernel gets - never taken from the kernel.  scale is max |coordinate| for positions and 1 for rotation-matrix elements; the floor
keeps a class where the fp32 reference happens to be exact from asking more than fp32 holds (8 roundings of the largest coordinate: the centroid, the
centred coordinate, three products and two sums of the rotation, the translation).  K is a margin over ANOTHER fp32 evaluation of the same chain: the
kernel accumulates the centroid in fp64, builds the rotor matrix per lane and uses Horn's eigenvector where torch sums pairwise in fp32 and takes an SVD - a
different realisation of the same roundings, not a different order of error."""
import numpy as np
import torch

from oracle import sampler_ref as spr

U = 2.0 ** -24
K = 4.0
FLOOR = 8.0 * U
GAP_DEGENERATE = 1e-6                # relative gap of the two largest eigenvalues of Horn's matrix under which the optimal rotation is not unique
BRANCH = np.float32(1e-6)            # the small-angle branch point of axis_angle_to_matrix (utils/geometry.py:38-68)


def bar(err32, scale=1.0):
    """THE tolerance (module docstring): max(K * err32, FLOOR * scale)"""
    return max(K * float(err32), FLOOR * float(scale))


def max_err(a, b):
    """max |a - b| in fp64; a non-finite value anywhere counts as an infinite error (a NaN must never pass a comparison)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    d = np.abs(a - b)
    return float(np.inf) if not np.isfinite(d).all() else float(d.max())


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# axis-angle vectors
# ------------------------------------------------------------------------------------------------------------------------------------
AXES = np.concatenate([np.eye(3), -np.eye(3)])


def _on_axes(angles, rng, n_random):
    """every angle on the six signed coordinate axes and on n_random random axes"""
    a = np.asarray(angles, np.float64)
    ax = np.concatenate([np.broadcast_to(AXES[None], (len(a), 6, 3)), _unit(rng, len(a) * n_random).reshape(len(a), n_random, 3)], axis=1)
    return (ax * a[:, None, None]).reshape(-1, 3)


def axis_angle_vectors(seed=0):
    """-> (aa [N, 3] float32, classes {name: index array}), N ~ 4000.  Classes:
    log_small     angles log-spaced over 1e-30 .. 1e-5 (the series branch and a decade past it; below ~1e-19 the squares are subnormal, below ~1e-23 they vanish)
    branch        nextafter down / the value / nextafter up of fp32(1e-6): the neighbours of the branch point on both sides
    underflow     components of 0.3e-23 .. 2e-23: every square is under half the smallest subnormal, the computed angle is 0 for a non-zero vector
    pi            pi and 2 pi with 0, +-1, +-2 ulp (sin(half) / angle at the half turn, cos(half) = -1 at the full turn)
    large         angles uniform in [2 pi, 100]
    zero          exact zeros of both signs
    typical       angles uniform in [1e-5, 2 pi] on random axes"""
    rng = np.random.default_rng(seed)
    parts = {}
    parts['log_small'] = _on_axes(np.logspace(-30, -5, 150), rng, 6)
    b = BRANCH
    parts['branch'] = _on_axes([np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(1))] * 4, rng, 14)
    parts['underflow'] = rng.uniform(0.3e-23, 2e-23, size=(240, 3)) * rng.choice([-1.0, 1.0], size=(240, 3))
    near = []
    for base in (np.float32(np.pi), np.float32(2 * np.pi)):
        lo1, hi1 = np.nextafter(base, np.float32(0)), np.nextafter(base, np.float32(100))
        near += [np.nextafter(lo1, np.float32(0)), lo1, base, hi1, np.nextafter(hi1, np.float32(100))]
    parts['pi'] = _on_axes(near * 2, rng, 14)
    parts['large'] = _on_axes(rng.uniform(2 * np.pi, 100.0, size=100), rng, 4)
    parts['zero'] = np.array([[0.0, 0.0, 0.0]] * 4 + [[-0.0, 0.0, -0.0]] * 4)
    parts['typical'] = _unit(rng, 400) * rng.uniform(1e-5, 2 * np.pi, size=(400, 1))
    aa, classes, at = [], {}, 0
    for name, v in parts.items():
        aa.append(np.asarray(v, np.float32))
        classes[name] = np.arange(at, at + len(v))
        at += len(v)
    return np.concatenate(aa), classes


def angle_fp32(aa):
    """the angle as the kernel and the fp32 reference compute it: fp32 squares, fp32 sum, fp32 square root"""
    a = np.asarray(aa, np.float32)
    return np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2], dtype=np.float32)


def axis_angle_ref(aa, dtype=torch.float64):
    """utils/geometry.py:71-85 through the oracle on the fp32 vectors, in `dtype` -> numpy [N, 3, 3]"""
    return spr.axis_angle_to_matrix(torch.from_numpy(np.asarray(aa, np.float32)).to(dtype)).numpy()


def rotation_defect(R):
    """-> (max |R R^T - I|, max |det R - 1|) per matrix, in fp64"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    return np.abs(np.einsum('bij,bkj->bik', R, R) - np.eye(3)).max(axis=(1, 2)), np.abs(np.linalg.det(R) - 1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# point-set pairs for Kabsch
# ------------------------------------------------------------------------------------------------------------------------------------
KABSCH_N = (1, 2, 3, 4, 12, 255, 256)
KABSCH_CLASSES = ('generic', 'identical', 'planar', 'collinear', 'reflection', 'reflection_noise', 'rot_pi', 'rot_near_pi', 'offset150', 'scale_1e-3',
                  'scale_1e3', 'unrelated')
REFLECTION_CLASSES = ('reflection', 'reflection_noise')


def _rot64(v):
    return spr.axis_angle_to_matrix(torch.tensor(np.asarray(v, np.float64))[None])[0].numpy()


def horn_matrix(S):
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def horn_rotation(S):
    """Horn 1987 in fp64 by symmetric eigendecomposition -> (R [3, 3], relative gap of the two largest eigenvalues; 0 for S = 0)"""
    S = np.asarray(S, np.float64)
    if not np.isfinite(S).all():          # (a NaN input gives a NaN rotation, as the kernel's Jacobi sweeps would)
        return np.full((3, 3), np.nan), 0.0
    w, V = np.linalg.eigh(horn_matrix(S))
    a, x, y, z = V[:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * a), 2 * (x * z + y * a)],
                  [2 * (x * y + z * a), 1 - 2 * (x * x + z * z), 2 * (y * z - x * a)],
                  [2 * (x * z - y * a), 2 * (y * z + x * a), 1 - 2 * (x * x + y * y)]])
    top = np.abs(w).max()
    return R, (float((w[-1] - w[-2]) / top) if top > 0 else 0.0)


def kabsch_pairs(n, seed=0):
    """-> (A [C, n, 3], B [C, n, 3] float32 in the order of KABSCH_CLASSES, props): props[name] = dict(gap = relative gap of the two largest
    eigenvalues of Horn's matrix in fp64, det = determinant of the unconstrained optimum V U^T of the fp64 SVD).  The collinear A is k * (0.5, 1, 1.5)
    with half-integer k of exact zero mean: exactly collinear in fp32, so that S has rank one whatever B is."""
    rng = np.random.default_rng(1000 * seed + n)
    X = rng.normal(size=(n, 3)) * 3.0
    Rg = _rot64([0.3, 0.2, -0.5])
    noise = lambda s: rng.normal(size=(n, 3)) * s
    P = X.copy()
    P[:, 2] = 0.0
    L = np.outer(np.arange(n) - (n - 1) / 2.0, [0.5, 1.0, 1.5])
    ax = _unit(rng, 1)[0]
    pairs = {
        'generic': (X, X @ Rg.T + noise(0.05) + 1.0),
        'identical': (X, X.copy()),
        'planar': (P, P @ _rot64([1.0, 2.0, 0.5]).T + noise(0.05)),
        'collinear': (L, L @ _rot64([0.4, 0.0, 0.1]).T + noise(0.05)),
        'reflection': (X, X * [1.0, 1.0, -1.0]),
        'reflection_noise': (X, X * [1.0, 1.0, -1.0] + noise(0.05)),
        'rot_pi': (X, X @ _rot64(np.pi * ax).T + noise(0.01)),
        'rot_near_pi': (X, X @ _rot64((np.pi - 1e-4) * ax).T + noise(0.01)),
        'offset150': (X + 150.0, X @ Rg.T + noise(0.05) + [150.0, -150.0, 150.0]),
        'scale_1e-3': (X * 1e-3, (X @ Rg.T + noise(0.05)) * 1e-3),
        'scale_1e3': (X * 1e3, (X @ Rg.T + noise(0.05)) * 1e3),
        'unrelated': (X, noise(3.0)),
    }
    A = np.stack([pairs[k][0] for k in KABSCH_CLASSES]).astype(np.float32)
    B = np.stack([pairs[k][1] for k in KABSCH_CLASSES]).astype(np.float32)
    props = {}
    for i, name in enumerate(KABSCH_CLASSES):
        a, b = A[i].astype(np.float64), B[i].astype(np.float64)
        S = (a - a.mean(0)).T @ (b - b.mean(0))
        Uu, _, Vt = np.linalg.svd(S)
        props[name] = dict(gap=horn_rotation(S)[1], det=float(np.linalg.det(Vt.T @ Uu.T)))
    return A, B, props


def kabsch_ref(A, B, dtype=torch.float64):
    """the oracle's kabsch_batch on the fp32 point sets in `dtype` -> (R [C, 3, 3], t [C, 3]) numpy"""
    R, t = spr.kabsch_batch(torch.from_numpy(np.asarray(A, np.float32)).to(dtype), torch.from_numpy(np.asarray(B, np.float32)).to(dtype))
    return R.numpy(), t.numpy()[:, :, 0]


def aligned(A, R, t):
    """R a + t in fp64 for every point of every pair"""
    return np.einsum('bij,bnj->bni', np.asarray(R, np.float64), np.asarray(A, np.float64)) + np.asarray(t, np.float64)[:, None, :]


def host_centroid(x, mutant=None):
    """the kernels' centroid: fp64 accumulator, one rounding to fp32.  mutant 'fp32_centroid': the sequential fp32 sum the kernels had before"""
    if mutant == 'fp32_centroid':
        return np.cumsum(x, axis=0, dtype=np.float32)[-1] / np.float32(len(x))
    return (np.cumsum(x, axis=0, dtype=np.float64)[-1] / len(x)).astype(np.float32)


def host_kabsch(A, B, mutant=None):
    """kabsch_block restated: centroids by host_centroid, S in fp64 from the fp32 differences, Horn in fp64, R rounded to fp32, t = -R cA + cB in fp32.
    mutant 'no_reflection_fix': the plain SVD product V U^T without the diag(1, 1, -1) correction (what the reference computes before :149-153)."""
    f = np.float32
    A, B = np.asarray(A, f), np.asarray(B, f)
    n = A.shape[0]
    cA, cB = host_centroid(A, mutant), host_centroid(B, mutant)
    S = (A - cA).astype(np.float64).T @ (B - cB).astype(np.float64)
    if mutant == 'no_reflection_fix':
        Uu, _, Vt = np.linalg.svd(S)
        R = (Vt.T @ Uu.T).astype(f)
    else:
        R = horn_rotation(S)[0].astype(f)
    t = -(R[:, 0] * cA[0] + R[:, 1] * cA[1] + R[:, 2] * cA[2]) + cB
    return R, t.astype(f)


# ------------------------------------------------------------------------------------------------------------------------------------
# ligands
# ------------------------------------------------------------------------------------------------------------------------------------
CHAIN_N = (3, 4, 66, 67, 68, 131, 132, 256)          # R = n - 3 = 0, 1, 63, 64, 65, 128, 129, 253: both sides of the 64-rotor chunks, the largest ligand
LIGANDS = tuple(f'chain{n}' for n in CHAIN_N) + ('planar20', 'branched')
UPDATE_CLASSES = ('typical', 'zero', 'tiny', 'half_turn', 'wide', 'rigid')
OFFSETS = (0.0, 150.0)
BOND = 1.5
_cache = {}


def _chain_positions(n, rng, planar):
    pos, d = [np.zeros(3)], np.array([1.0, 0.0, 0.0])
    for _ in range(1, n):
        v = rng.normal(size=3)
        if planar:
            v[2] = 0.0
        v -= 0.5 * (v @ d) * d          # never folds straight back: no two atoms coincide
        v /= np.linalg.norm(v)
        d = v
        pos.append(pos[-1] + BOND * v)
    return np.asarray(pos)


def ligand(name):
    """-> complex dict (numpy arrays in the layout Complex takes; a 20-residue synthetic receptor, for the ligands of the sampler test a 40-residue one
    around the ligand).  chain<n>: bonds (i, i + 1) of length 1.5, R = n - 3 rotors by synthetic.transformation_mask; planar20: a chain in the plane z = 0;
    branched: synthetic.make_ligand's two rings, linker, tail and substituents."""
    if name in _cache:
        return _cache[name]
    from disco_diffdock_amd import synthetic
    if name == 'branched':
        c = synthetic.make_complex(41, n_res=40, n_lig=30)
    else:
        n = 20 if name == 'planar20' else int(name[5:])
        rng = np.random.default_rng(100 + n)
        c = synthetic.make_complex(1, n_res=40 if n == 68 else 20, n_lig=20)
        pos = _chain_positions(n, rng, planar=name == 'planar20')
        if n == 68:      # the sampler runs the score model on it: put it into the pocket the synthetic ligand had
            pos = pos - pos.mean(0) + c['lig_pos'].mean(0)
        bonds = [(i, i + 1) for i in range(n - 1)]
        edge_mask, mask_rotate = synthetic.transformation_mask(n, bonds)
        ei = np.zeros((2, 2 * len(bonds)), np.int64)
        for bi, (a, b) in enumerate(bonds):
            ei[:, 2 * bi], ei[:, 2 * bi + 1] = (a, b), (b, a)
        ea = np.zeros((2 * len(bonds), 4), np.float32)
        ea[:, 0] = 1
        c.update(lig_x=np.stack([rng.integers(0, d, size=n) for d in synthetic.LIG_FEATURE_DIMS], 1), lig_pos=pos.astype(np.float32), bond_index=ei, bond_attr=ea,
                 edge_mask=edge_mask, mask_rotate=mask_rotate)
    _cache[name] = c
    return c


def rotors(c):
    """-> [R, 2] (u, v) of the rotatable directed bonds in bond order: axis pos[u] - pos[v], pivot pos[v], the atoms of mask_rotate[r] turn"""
    return np.asarray(c['bond_index']).T[np.asarray(c['edge_mask'], bool)].reshape(-1, 2)


def bonds(c):
    return np.asarray(c['bond_index']).T[::2]


def updates(cls, R, B, seed=0):
    """-> (tr [B, 3], rot [B, 3], tor [B, R] or None) float32 of one update class (the table of tests/test_geometry_bound.py's docstring)"""
    rng = np.random.default_rng(seed)
    f = np.float32
    tr, rot, tor = rng.normal(size=(B, 3)), 0.3 * rng.normal(size=(B, 3)), rng.normal(size=(B, R))
    if cls == 'zero':
        tr, rot, tor = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, R))
    elif cls == 'tiny':
        tr, rot = np.zeros((B, 3)), 1e-8 * _unit(rng, B)
        tor = 1e-7 * rng.choice([-1.0, 1.0], size=(B, R))
        tor[:, 1::2] = 0.0
    elif cls == 'half_turn':
        rot, tor = np.pi * _unit(rng, B), np.pi * rng.choice([-1.0, 1.0], size=(B, R))
    elif cls == 'wide':
        rot, tor = 3.0 * rng.normal(size=(B, 3)), rng.uniform(-2 * np.pi, 2 * np.pi, size=(B, R))
    elif cls == 'rigid':
        tor = None
    elif cls != 'typical':
        raise ValueError(cls)
    return tr.astype(f), rot.astype(f), None if tor is None else tor.astype(f)


def poses(c, B, offset):
    """B copies of the conformer, shifted by (offset, -offset, offset) and by a different sub-Angstrom amount each -> [B, n, 3] float32"""
    p = np.asarray(c['lig_pos'], np.float64)
    p = p - p.mean(0) if offset else p
    return np.stack([p + np.array([offset, -offset, offset]) + 0.37 * b for b in range(B)]).astype(np.float32)


def _batch(c, B):
    key = ('batch', id(c), B)
    if key not in _cache:
        from helpers import batch_of
        _cache[key] = batch_of(c, B)
    return _cache[key]


def update_ref(c, pos, tr, rot, tor, dtype=torch.float64):
    """oracle.sampler_ref.modify_conformer_batch (with its axis_angle_to_matrix and kabsch_batch) on `dtype` tensors -> [B, n, 3] numpy.  A ligand
    without rotors takes the rigid branch like the kernel does (the reference cannot reshape an empty torsion vector)."""
    B, n = pos.shape[0], pos.shape[1]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    mr = torch.from_numpy(np.asarray(c['mask_rotate'], bool))
    flexible = tor is not None and mr.shape[0] > 0
    out = spr.modify_conformer_batch(t(pos).reshape(-1, 3), _batch(c, B), t(tr), t(rot), t(tor).reshape(-1) if flexible else None, mr)
    return out.reshape(B, n, 3).numpy()


def randomize_ref(c, pos0, tor, rot, tr, dtype=torch.float64):
    """randomize_position (utils/sampling.py:12-34 with utils/torsion.py:48-68) restated on the caller's draws in `dtype`: sequential torsion updates in bond
    order on the current coordinates, a rotor skipped only when its fp32 draw is exactly 0, then (pos - centroid) R^T (+ tr).  tor / tr may be None."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    mr, uv = np.asarray(c['mask_rotate'], bool), rotors(c)
    out = []
    for b in range(rot.shape[0]):
        p = t(pos0).clone()
        if tor is not None:
            for r, (u, v) in enumerate(uv):
                if tor[b, r] == 0:
                    continue
                axis = p[u] - p[v]
                M = spr.axis_angle_to_matrix((axis * t(tor[b, r:r + 1]) / torch.linalg.norm(axis))[None])[0]
                m = torch.from_numpy(mr[r])
                p[m] = (p[m] - p[v]) @ M.T + p[v]
        p = (p - p.mean(dim=0, keepdim=True)) @ t(rot[b]).T
        out.append(p + t(tr[b]) if tr is not None else p)
    return torch.stack(out).numpy()


def pose_metrics_ref(pos, ref, mask=None, perms=None, rec=None, dtype=np.float64):
    """evaluate.py:297-338 in numpy `dtype` -> [B, 4] = rmsd (minimum over the valid rows of perms; inf if none is valid), centroid distance, min cross
    distance, min self distance (inf for fewer than two kept atoms).  An empty mask divides by max(count, 1) like the kernel: rmsd 0, centroid distance 0."""
    pos, ref = np.asarray(pos, dtype), np.asarray(ref, dtype)
    n = ref.shape[0]
    keep = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    cnt = dtype(max(int(keep.sum()), 1))
    rows = [np.arange(n)] if perms is None else [np.asarray(r, np.int64) for r in perms]
    rows = [r for r in rows if not ((r[keep] < 0) | (r[keep] >= n)).any()]
    out = np.empty((len(pos), 4), dtype)
    for b, p in enumerate(pos):
        best = min([((p[r[keep]] - ref[keep]) ** 2).sum(dtype=dtype) for r in rows], default=dtype(np.inf))
        out[b, 0] = np.sqrt(best / cnt)
        d = (p[keep].sum(0, dtype=dtype) - ref[keep].sum(0, dtype=dtype)) / cnt
        out[b, 1] = np.sqrt((d * d).sum(dtype=dtype))
        out[b, 2] = np.inf if rec is None or not keep.any() else np.sqrt((((np.asarray(rec, dtype)[:, None] - p[keep][None]) ** 2).sum(-1, dtype=dtype)).min())
        dd = ((p[keep][:, None] - p[keep][None]) ** 2).sum(-1, dtype=dtype)
        dd[np.eye(len(dd), dtype=bool)] = np.inf
        out[b, 3] = np.sqrt(dd.min()) if dd.size else np.inf
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the host restatement of se3_update_kernel
# ------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ('stale_torsion', 'pivot_u', 'reversed_axis', 'no_kabsch', 'no_reflection_fix', 'no_small_angle', 'chunk_slip', 'fp32_centroid', 'uncentred')


def host_axis_angle(aa, small_angle_branch=True):
    """axis_angle_to_matrix_dev in numpy (fp32 up to the quaternion, the matrix assembled in fp64 and rounded once per element, as the kernel does), vectorised over the rows of aa [N, 3] -> [N, 3, 3]"""
    f = np.float32
    a = np.asarray(aa, f).reshape(-1, 3)
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    with np.errstate(all='ignore'):
        ang = np.sqrt(ax * ax + ay * ay + az * az, dtype=f)
        half = f(0.5) * ang
        series = f(0.5) - ang * ang / f(48.0)
        s = np.sin(half, dtype=f) / ang
        if small_angle_branch:
            s = np.where(np.abs(ang) < f(1e-6), series, s)
        qr, qi, qj, qk = [q.astype(np.float64) for q in (np.cos(half, dtype=f), ax * s, ay * s, az * s)]          # fp32 quaternion, matrix assembled in fp64, one rounding per element
        two_s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk)
        R = np.stack([1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                      two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                      two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)], axis=-1)
    return R.astype(f).reshape(-1, 3, 3)


def host_update(c, pos, tr, rot, tor, mutant=None):
    """se3_update_kernel restated in numpy fp32 (Horn's S in fp64 as in the kernel): centroid by host_centroid; CENTRED rigid = R (x - ctr); per rotor, in bond
    order, the matrix from the CURRENT coordinates with pivot v and axis u - v; Kabsch of the flexed onto the rigid pose by host_kabsch; + tr + ctr on the aligned pose.  -> [B, n, 3]
    float32.  `mutant` names one deliberate error (MUTANTS; tests/test_geometry_bound.py shows that each one that changes the mathematics breaks a bar)."""
    f = np.float32
    pos = np.asarray(pos, f)
    B, n = pos.shape[0], pos.shape[1]
    mr, uv = np.asarray(c['mask_rotate'], bool), rotors(c)
    branch = mutant != 'no_small_angle'
    out = np.empty_like(pos)
    for b in range(B):
        x = pos[b]
        ctr = host_centroid(x, mutant)
        Rm = host_axis_angle(rot[b], branch)[0]
        d = x - ctr
        shift = (np.asarray(tr[b], f), ctr)          # added once, to the final pose: everything in between is centred (mutant 'uncentred': added here, as the kernel did)
        rig = (Rm[:, 0] * d[:, 0:1] + Rm[:, 1] * d[:, 1:2] + Rm[:, 2] * d[:, 2:3]).astype(f)
        if mutant == 'uncentred':
            rig, shift = (rig + shift[0] + shift[1]).astype(f), (f(0), f(0))
        if tor is None or len(uv) == 0:
            out[b] = rig + shift[0] + shift[1]
            continue
        cur = rig.copy()
        for r, (u, v) in enumerate(uv):
            th = f(tor[b, r - 64 if (mutant == 'chunk_slip' and r >= 64) else r])
            src = rig if mutant == 'stale_torsion' else cur
            if mutant == 'reversed_axis':
                u, v = v, u
            piv = src[u if mutant == 'pivot_u' else v].copy()
            axis = src[u] - src[v]
            with np.errstate(all='ignore'):
                nn = np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2], dtype=f)
                Rl = host_axis_angle(axis / nn * th, branch)[0]
            m = mr[r]
            d = cur[m] - piv
            cur[m] = (Rl[:, 0] * d[:, 0:1] + Rl[:, 1] * d[:, 1:2] + Rl[:, 2] * d[:, 2:3] + piv).astype(f)
        if mutant == 'no_kabsch':
            out[b] = cur + shift[0] + shift[1]
            continue
        Rk, tk = host_kabsch(cur, rig, mutant)
        out[b] = (Rk[:, 0] * cur[:, 0:1] + Rk[:, 1] * cur[:, 1:2] + Rk[:, 2] * cur[:, 2:3] + tk + shift[0] + shift[1]).astype(f)
    return out


def update_figures(c, pos, tr, rot, tor, got, ref64=None, ref32=None):
    """The four comparisons every realisation of the update is held to, each as (error, bar, err32):
    pos       the poses against the fp64 reference; err32 = the fp32 reference's error, scale = max |coordinate|
    bond      every bond length of the output against the INPUT's (the update is an isometry of every bond); err32 = the fp32 reference's worst bond
              length change, scale = max |coordinate| (a length is a difference of two coordinates)
    centroid  the output centroid against centroid(pos) + tr (Kabsch alignment preserves it); err32 = the fp32 reference's
    zero      only for an all-zero update: the output against the input, same bar as pos"""
    ref64 = update_ref(c, pos, tr, rot, tor) if ref64 is None else ref64
    ref32 = update_ref(c, pos, tr, rot, tor, torch.float32) if ref32 is None else ref32
    p64 = np.asarray(pos, np.float64)
    scale = float(np.abs(ref64).max())
    bd = bonds(c)
    length = lambda p: np.linalg.norm(np.asarray(p, np.float64)[:, bd[:, 0]] - np.asarray(p, np.float64)[:, bd[:, 1]], axis=-1)
    cen = p64.mean(1) + np.asarray(tr, np.float64)
    fb = lambda err, err32: (err, bar(err32, scale), err32)
    fig = dict(pos=fb(max_err(got, ref64), max_err(ref32, ref64)),
               bond=fb(max_err(length(got), length(p64)), max_err(length(ref32), length(p64))),
               centroid=fb(max_err(np.asarray(got, np.float64).mean(1), cen), max_err(ref32.astype(np.float64).mean(1), cen)))
    if not np.any(tr) and not np.any(rot) and (tor is None or not np.any(tor)):
        fig['zero'] = fb(max_err(got, p64), fig['pos'][2])
    return fig


def ratio(err, the_bar):
    """error in units of the bar's own err32 term: K * err / bar, so a figure of K sits on the bar (inf for a non-finite error)"""
    return float(K * err / the_bar)
