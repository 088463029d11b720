"""The pose-update kernels of csrc/k_se3.hip on adversarial geometry against fp64 (tests/adversarial_geometry.py holds the generators, the references and the
bar; tests/test_geometry_bound.py checks on the CPU that the generators have the properties they claim and that the bars bite).

Every comparison is held to  bar(err32, scale) = max(K * err32, 8 * 2^-24 * scale),  K = 4:  err32 is the fp32 reference's own error against the fp64
reference on the SAME input, computed on the host at run time; scale is max |coordinate| for positions and 1 for rotation-matrix elements.  All through entry
points that exist: ddk_debug_axis_angle, ddk_debug_kabsch, ddk_se3_update, ddk_sample_trajectory (the <POST, REC> instantiations of the update, per step),
ddk_randomize_position, ddk_pose_metrics.  Inputs stay inside the documented limits (n_lig <= 256, B <= max_batch).

Figures are kept through _record_drift under geometry_<entry>_<class>_n<n>: value = K * error / bar, the kernel's error in units of err32 where K * err32 is
the bar (4 sits on the bar).  Measured on an MI355X (profiles/r08_parity_drift.json; `before_fixes` there is the same figure on the library before the three
changes below), worst figure per entry point:

    entry point         before                                        after
    axis_angle          1.00 elements; |R R^T - I| 5.85e-7 (FAILED)   1.00 elements; |R R^T - I| 8.0e-8, |det R - 1| 8.3e-8 (bound 4.77e-7)
    kabsch              4.04 offset150, n = 256 (FAILED)              0.86 rot_pi, n = 1  (offset150, n = 256: 0.44)
    se3_update          5.44 half_turn at 150 A, n = 256 (FAILED)     1.70 typical at the origin, n = 66; 0.90 at most 150 A out
    sample (per step)   1.52 chain68                                  0.9 .. 1.6 over four runs (the scores under it are atomic sums)
    randomize           0.98                                          1.95 n = 256
    pose_metrics        1.00 one_kept                                 1.00

WHAT THE TESTS FOUND, fixed in csrc/k_se3.hip in the same change.
1. kabsch_block, se3_update_kernel and randomize_kernel summed the centroid sequentially in fp32.  For 256 atoms 150 A from the origin the partial sums pass
   2^15 (ulp 2^-8), the centroid ends 1e-4 A off - five times the fp32 reference's error - and goes into every output atom.  fp64 accumulators now, one
   rounding at the end, 16 lanes per component so that the step is no slower.
2. se3_update_kernel ran the rotor loop on coordinates that already held tr + centroid, so 150 A out every rotor axis and rotated atom carried roundings of
   the distance from the origin, amplified by the chain's lever arms (up to 5e-3 A on a 129-rotor chain, 8.9 x the fp32 reference on one sample of the host
   restatement).  The loop and the Kabsch step run on centred coordinates now and tr + centroid is added to the aligned pose: 150 A out the error is below the
   fp32 reference's in every class.
3. axis_angle_to_matrix_dev assembled the matrix in fp32 like the reference: |R R^T - I| 5.85e-7 and |det R - 1| 5.32e-7 near a half turn, against the bound
   8 * 2^-24 = 4.77e-7 (the fp32 reference itself: 4.30e-7 / 4.96e-7).  The matrix of the fp32 quaternion is assembled in fp64 now, one rounding per element.
The restatement's `fp32_centroid` and `uncentred` forms keep the old arithmetic under test on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import adversarial_geometry as ag
from oracle import score_model_ref as smr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CFG = smr.ScoreModelConfig(latent_vocab=64)
B = 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def complexes(dev):
    """one topology-only Complex per ligand (max_batch 4), created on first use and shared by the tests of this module"""
    from disco_diffdock_amd.runtime import Complex
    from disco_diffdock_amd.tensor_layers import _shape_context
    made = {}

    def get(name):
        if name not in made:
            made[name] = Complex(_shape_context(0), ag.ligand(name), max_batch=4)
        return made[name]
    return get


def _record(entry, cls, n, value, **extra):
    from test_gpu_round3 import _record_drift
    _record_drift(f'geometry_{entry}_{cls}_n{n}', value, bar=ag.K, **extra)


def _tag(name):
    """ligand name -> (class suffix, n) of the drift key"""
    c = ag.ligand(name)
    return ('' if name.startswith('chain') else '_' + name.rstrip('0123456789')), len(c['lig_pos'])


def test_axis_angle_adversarial(dev):
    """~4000 vectors in ONE launch (angles 1e-30 .. 1e-5, the fp32 neighbours of the 1e-6 branch point, components whose squares underflow, pi and 2 pi +- 2
    ulp, angles up to 100, exact zeros; on the coordinate axes and on random axes): every element within the bar of the fp64 oracle per class, |R R^T - I| and
    |det R - 1| within 8 * 2^-24, no non-finite value."""
    from disco_diffdock_amd.tensor_layers import _shape_context
    ctx = _shape_context(0)
    aa, classes = ag.axis_angle_vectors()
    d_aa = T(aa).contiguous().to(dev)
    R = torch.empty((len(aa), 3, 3), device=dev)
    ctx._check(ctx.L.ddk_debug_axis_angle(ctx.h, len(aa), C.c_void_p(d_aa.data_ptr()), C.c_void_p(R.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               'ddk_debug_axis_angle')
    R = R.cpu().numpy()
    assert np.isfinite(R).all()
    R64, R32 = ag.axis_angle_ref(aa), ag.axis_angle_ref(aa, torch.float32)
    orth, det = ag.rotation_defect(R)
    bad = []
    for name, idx in classes.items():
        err, err32 = ag.max_err(R[idx], R64[idx]), ag.max_err(R32[idx], R64[idx])
        the_bar = ag.bar(err32)
        print(f'axis_angle {name:10s}: |R - fp64| {err:.2e} (fp32 oracle {err32:.2e}, bar {the_bar:.2e}), |R R^T - I| {orth[idx].max():.2e}, |det - 1| {det[idx].max():.2e} '
              f'(bar {ag.FLOOR:.2e})')
        _record('axis_angle', name, len(idx), ag.ratio(err, the_bar), err=err, err32=err32, orthogonality=float(orth[idx].max()), det=float(det[idx].max()))
        if not (err <= the_bar and orth[idx].max() <= ag.FLOOR and det[idx].max() <= ag.FLOOR):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize('n', ag.KABSCH_N)
def test_kabsch_adversarial(dev, n):
    """One launch per n over the twelve classes (generic, identical, planar, collinear, reflection (+ noise), rotation by pi and pi - 1e-4, both sets 150 out,
    coordinates * 1e-3 and * 1e3, unrelated sets): R within the bar where the optimum is unique (eigenvalue gap >= 1e-6), the aligned positions R a + t within
    the bar in EVERY class (collinear sets and n <= 2 have no unique R, but a unique image), det R > 0 and orthogonality to 8 * 2^-24 everywhere, nothing
    non-finite - n = 1 included, where S = 0."""
    from disco_diffdock_amd.tensor_layers import _shape_context
    ctx = _shape_context(0)
    A, Bp, props = ag.kabsch_pairs(n)
    nb = A.shape[0]
    dA, dB = T(A).contiguous().to(dev), T(Bp).contiguous().to(dev)
    R, t = torch.empty((nb, 3, 3), device=dev), torch.empty((nb, 3), device=dev)
    ctx._check(ctx.L.ddk_debug_kabsch(ctx.h, nb, n, C.c_void_p(dA.data_ptr()), C.c_void_p(dB.data_ptr()), C.c_void_p(R.data_ptr()), C.c_void_p(t.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ddk_debug_kabsch')
    R, t = R.cpu().numpy(), t.cpu().numpy()
    assert np.isfinite(R).all() and np.isfinite(t).all()
    (R64, t64), (R32, t32) = ag.kabsch_ref(A, Bp), ag.kabsch_ref(A, Bp, torch.float32)
    P, P64, P32 = ag.aligned(A, R, t), ag.aligned(A, R64, t64), ag.aligned(A, R32, t32)
    orth, _ = ag.rotation_defect(R)
    bad = []
    for i, name in enumerate(ag.KABSCH_CLASSES):
        scale = float(np.abs(Bp[i]).max())
        eP, barP = ag.max_err(P[i], P64[i]), ag.bar(ag.max_err(P32[i], P64[i]), scale)
        unique = props[name]['gap'] >= ag.GAP_DEGENERATE
        eR, barR = (ag.max_err(R[i], R64[i]), ag.bar(ag.max_err(R32[i], R64[i]))) if unique else (0.0, ag.FLOOR)
        det = float(np.linalg.det(R[i].astype(np.float64)))
        print(f'kabsch n = {n:3d} {name:17s}: gap {props[name]["gap"]:.1e}, aligned {eP:.2e} (bar {barP:.2e}), R {eR:.2e} (bar {barR:.2e}{"" if unique else ", not unique"}), '
              f'det {det:+.7f}, |R R^T - I| {orth[i]:.1e}')
        _record('kabsch', name, n, max(ag.ratio(eP, barP), ag.ratio(eR, barR)), aligned=ag.ratio(eP, barP), R=ag.ratio(eR, barR) if unique else None,
                err_aligned=eP, gap=props[name]['gap'])
        if not (eP <= barP and eR <= barR and det > 0 and orth[i] <= ag.FLOOR):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize('offset', ag.OFFSETS)
@pytest.mark.parametrize('cls', ag.UPDATE_CLASSES)
@pytest.mark.parametrize('lig', ag.LIGANDS)
def test_se3_update_adversarial(dev, complexes, lig, cls, offset):
    """ddk_se3_update on chains of R = 0, 1, 63, 64, 65, 128, 129, 253 rotors (both sides of the 64-rotor chunks), a planar chain and a branched ligand; update
    classes typical / zero / tiny (rot 1e-8, tor 1e-7 alternating with exact zeros: the series branch inside the rotor loop) / half_turn (|rot| = pi, tor = +-pi)
    / wide (rot sigma 3, tor in [-2 pi, 2 pi]) / rigid (no torsion pointer); at the origin and 150 A out.  Against the fp64 oracle within the bar; bond lengths
    of the output within the bar of the input's; centroid within the bar of centroid + tr; `zero` returns the input to the bar; `rigid` is the oracle's rigid
    branch (same comparison: the reference is called without torsions)."""
    c, cx = ag.ligand(lig), complexes(lig)
    pos = ag.poses(c, B, offset)
    tr, rot, tor = ag.updates(cls, cx.R, B, seed=7)
    got = cx.se3_update(T(pos).to(dev), T(tr).to(dev), T(rot).to(dev), None if tor is None else T(tor).to(dev)).cpu().numpy()
    assert np.isfinite(got).all()
    fig = ag.update_figures(c, pos, tr, rot, tor, got)
    assert ('zero' in fig) == (cls == 'zero')
    ratios = {k: ag.ratio(e, b) for k, (e, b, _) in fig.items()}
    print(f'se3_update {lig} R = {cx.R} {cls} at {offset:g}: ' + ', '.join(f'{k} {e:.2e} (fp32 oracle {e32:.2e}, bar {b:.2e})' for k, (e, b, e32) in fig.items()))
    suffix, n = _tag(lig)
    _record('se3_update', f'{cls}_at{offset:g}{suffix}', n, max(ratios.values()), **ratios, err_pos=fig['pos'][0], err32_pos=fig['pos'][2])
    assert all(e <= b for e, b, _ in fig.values()), ratios


@pytest.mark.parametrize('no_torsion', [False, True])
@pytest.mark.parametrize('lig', ['chain68', 'branched'])
def test_update_inside_sample_per_step(dev, lig, no_torsion):
    """The <POST, REC> instantiations ddk_sample launches (heads' post fused into the update), pinned PER STEP at fp32 grade instead of per trajectory at 1e-3:
    a 4-step recorded call with random weights, B = 3 and injected noise; for every step k the fp64 modify_conformer_batch of the recorded pos[k] and
    perturb[k] must give pos[k + 1] within the bar.  The 68-atom chain has R = 65: the POST torsion finish and the rotor table both cross their 64-bond chunk.
    On a no_torsion context the perturbation's torsion columns are zero and the reference takes its rigid branch.  (The scores stay with the existing tests.)"""
    from test_gpu_trajectory import _coefficients
    from disco_diffdock_amd.runtime import Context, Complex
    c = ag.ligand(lig)
    P = smr.random_state_dict(CFG, seed=11)
    if no_torsion:
        P = {k: v for k, v in P.items() if not k.startswith(('final_edge_embedding', 'tor_bond_conv', 'tor_final_layer'))}
    ctx = Context(device=0, no_torsion=int(no_torsion))
    ctx.load_state_dict(P)
    steps = 4
    cx = Complex(ctx, c, B)
    _, t_arr, sc, nc = _coefficients(steps)
    rng = np.random.default_rng(5)
    pos0 = np.stack([c['lig_pos'] + rng.normal(0, 1.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)
    z = 0.2 * torch.randn(steps, B, 6 + cx.R, generator=torch.Generator().manual_seed(3))
    rec = cx.sample(T(pos0.copy()).to(dev), t_arr, sc, nc, z.to(dev), record=('pos', 'perturb'))
    torch.cuda.synchronize()
    pos, pt = rec.pos.cpu().numpy(), rec.perturb.cpu().numpy()
    assert np.isfinite(pos).all() and np.isfinite(pt).all()
    assert cx.R > 0 and (np.abs(pt[:, :, 6:]).max() == 0.0) == no_torsion
    worst, ok = 0.0, True
    for k in range(steps):
        tor = None if no_torsion else pt[k][:, 6:]
        fig = ag.update_figures(c, pos[k], pt[k][:, 0:3], pt[k][:, 3:6], tor, pos[k + 1])
        print(f'sample {lig} no_torsion = {no_torsion} step {k}: ' + ', '.join(f'{n_} {e:.2e} (fp32 oracle {e32:.2e}, bar {b:.2e})' for n_, (e, b, e32) in fig.items()))
        worst = max(worst, max(ag.ratio(e, b) for e, b, _ in fig.values()))
        ok = ok and all(e <= b for e, b, _ in fig.values())
    suffix, n = _tag(lig)
    _record('sample', f'per_step{"_no_torsion" if no_torsion else ""}{suffix}', n, worst)
    assert ok, worst


@pytest.mark.parametrize('variant', ['full', 'no_torsion', 'no_translation'])
@pytest.mark.parametrize('n', [67, 68, 256])
def test_randomize_position_adversarial(dev, complexes, n, variant):
    """ddk_randomize_position on the chains with R = 64, 65 and 253: uniform(-pi, pi) draws with exact 0 (the skipped rotor), +-fp32(pi) and the fp32 neighbours of
    +-pi on both sides placed in every sample; with tor = None and with tr = None; against the fp64 restatement of randomize_position on the same draws."""
    from scipy.spatial.transform import Rotation
    lig = f'chain{n}'
    c, cx = ag.ligand(lig), complexes(lig)
    rng = np.random.default_rng(n)
    nb, Rn = 4, cx.R
    tor = rng.uniform(-np.pi, np.pi, size=(nb, Rn)).astype(np.float32)
    pi = np.float32(np.pi)
    special = [np.float32(0), pi, -pi, np.nextafter(pi, np.float32(0)), np.nextafter(pi, np.float32(4)), -np.nextafter(pi, np.float32(0)), -np.nextafter(pi, np.float32(4))]
    for b in range(nb):
        at = rng.choice(Rn, size=len(special), replace=False)
        tor[b, at] = special
        tor[b, min(63 + b % 2, Rn - 1)] = 0.0          # a skipped rotor on either side of a would-be 64 boundary
    rot = Rotation.random(nb, random_state=rng).as_matrix().astype(np.float32)
    tr = rng.normal(0, 19.0, size=(nb, 3)).astype(np.float32)
    if variant == 'no_torsion':
        tor = None
    if variant == 'no_translation':
        tr = None
    pos0 = np.asarray(c['lig_pos'], np.float32)
    got = cx.randomize_position(T(pos0).to(dev), T(rot).to(dev), None if tor is None else T(tor).to(dev), None if tr is None else T(tr).to(dev)).cpu().numpy()
    ref64, ref32 = ag.randomize_ref(c, pos0, tor, rot, tr), ag.randomize_ref(c, pos0, tor, rot, tr, torch.float32)
    err, err32 = ag.max_err(got, ref64), ag.max_err(ref32, ref64)
    the_bar = ag.bar(err32, np.abs(ref64).max())
    print(f'randomize_position n = {n} R = {Rn} {variant}: {err:.2e} (fp32 restatement {err32:.2e}, bar {the_bar:.2e})')
    _record('randomize', variant, n, ag.ratio(err, the_bar), err=err, err32=err32)
    assert err <= the_bar


def _pose_metrics_raw(cx, dev, pos, ref, mask=None, perms=None, rec=None):
    """ddk_pose_metrics through the C ABI (Complex.pose_metrics refuses a permutation table with an entry outside the ligand before the kernel sees it)"""
    ctx = cx.ctx
    p = lambda a, dt: None if a is None else T(np.ascontiguousarray(a, dt)).to(dev)
    d_pos, d_ref, d_m, d_pm, d_rec = p(pos, np.float32), p(ref, np.float32), p(mask, np.uint8), p(perms, np.int32), p(rec, np.float32)
    out = torch.empty((pos.shape[0], 4), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    ctx._check(ctx.L.ddk_pose_metrics(ctx.h, cx.h, pos.shape[0], ptr(d_pos), ptr(d_ref), ptr(d_m), ptr(d_pm), 0 if perms is None else len(perms), ptr(d_rec),
                                      0 if rec is None else len(rec), ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ddk_pose_metrics')
    return out.cpu().numpy()


def _metrics_ok(got, pos, ref, scale, **kw):
    """every metric against numpy fp64 within bar(err32, scale), err32 = the same restatement in numpy fp32; an infinite reference must be met by inf"""
    m64, m32 = ag.pose_metrics_ref(pos, ref, **kw), ag.pose_metrics_ref(pos, ref, dtype=np.float32, **kw)
    assert not np.isnan(got).any()
    inf = np.isinf(m64)
    ok = bool((np.isinf(got) == inf).all() and (got[inf] > 0).all())
    worst = 0.0
    for j in range(4):
        f = ~inf[:, j]
        the_bar = ag.bar(ag.max_err(m32[f, j], m64[f, j]), scale)
        err = ag.max_err(got[f, j], m64[f, j])
        worst, ok = max(worst, ag.ratio(err, the_bar)), ok and err <= the_bar
    return ok, worst


def test_pose_metrics_adversarial(dev, complexes):
    """ddk_pose_metrics on the 256-atom chain (and a one-atom ligand) against numpy fp64:
    shifted        poses and reference both 150 A out, true centroid distance ~0.3 A (cancels in the fp32 sums)
    one_kept       exactly one kept atom: min self distance inf, rmsd of that atom
    none_kept      an all-false mask: the kernel divides by max(count, 1) and returns rmsd 0, centroid distance 0, min cross inf, min self inf - finite or inf, never NaN
    one_atom       n_lig = 1
    last_row       a permutation table of 257 rows (past the 256 threads' first pass) whose only valid row is the last
    no_valid_row   a table whose every row holds an entry outside the ligand: rmsd inf"""
    from disco_diffdock_amd.runtime import Complex
    from disco_diffdock_amd.tensor_layers import _shape_context
    c, cx = ag.ligand('chain256'), complexes('chain256')
    n = 256
    rng = np.random.default_rng(2)
    shift = np.array([150.0, -150.0, 150.0])
    ref = (c['lig_pos'].astype(np.float64) - c['lig_pos'].mean(0) + shift).astype(np.float32)
    pos = np.stack([ref + np.float32(0.3 / np.sqrt(3)) + rng.normal(0, 0.05, size=(n, 3)) for _ in range(B)]).astype(np.float32)
    rec = np.asarray(c['rec_pos'], np.float32)
    scale = float(np.abs(pos).max())
    one = np.zeros(n, bool)
    one[137] = True
    table = np.stack([rng.permutation(n) for _ in range(257)]).astype(np.int32)
    table[np.arange(256), rng.integers(0, n, size=256)] = rng.choice([-1, n, 2 ** 31 - 1], size=256)
    invalid = table.copy()
    invalid[256, 5] = n
    results = {}
    cases = dict(shifted=dict(), one_kept=dict(mask=one), none_kept=dict(mask=np.zeros(n, bool)), last_row=dict(perms=table), no_valid_row=dict(perms=invalid))
    for name, kw in cases.items():
        got = _pose_metrics_raw(cx, dev, pos, ref, rec=rec, **kw)
        results[name] = (got,) + _metrics_ok(got, pos, ref, scale, rec=rec, **kw)
    # n_lig = 1 (no bonds, no rotors)
    c1 = dict(c)
    c1.update(lig_x=c['lig_x'][:1], lig_pos=c['lig_pos'][:1], bond_index=np.zeros((2, 0), np.int64), bond_attr=np.zeros((0, 4), np.float32),
              edge_mask=np.zeros(0, bool), mask_rotate=np.zeros((0, 1), bool))
    cx1 = Complex(_shape_context(0), c1, max_batch=B)
    got = _pose_metrics_raw(cx1, dev, pos[:, :1], ref[:1], rec=rec)
    results['one_atom'] = (got,) + _metrics_ok(got, pos[:, :1], ref[:1], scale, rec=rec)
    for name, (got, ok, worst) in results.items():
        print(f'pose_metrics {name:12s}: worst figure {worst:.2f}, first pose {got[0]}')
        _record('pose_metrics', name, 1 if name == 'one_atom' else n, worst)
    assert np.isinf(results['one_kept'][0][:, 3]).all() and np.isinf(results['one_atom'][0][:, 3]).all()
    assert np.array_equal(results['none_kept'][0], np.tile(np.array([0.0, 0.0, np.inf, np.inf], np.float32), (B, 1)))
    assert np.isinf(results['no_valid_row'][0][:, 0]).all() and np.isfinite(results['last_row'][0][:, 0]).all()
    assert abs(float(results['shifted'][0][0, 1]) - 0.3) < 0.05          # the premise of `shifted`: the centroid distance is the small difference of large sums
    assert all(ok for _, ok, _ in results.values()), {k: w for k, (_, _, w) in results.items()}
