"""CPU tests of tests/adversarial_geometry.py: every generator class has the property it claims, the host restatement of the pose update meets every bar
the GPU module (tests/test_gpu_geometry_adversarial.py) applies, the fp64 reference has the invariants the GPU module relies on, and the bars bite - each
deliberate error of the restatement that changes the mathematics breaks at least one of them.

Update classes (adversarial_geometry.updates), each with B = 3, at the origin and 150 A out:
    typical     tr sigma 1, rot sigma 0.3, tor sigma 1
    zero        every update exactly 0: the output must equal the input to the bar
    tiny        tr 0, |rot| = 1e-8, tor = +-1e-7 alternating with exact zeros (the series branch of the axis-angle map, inside the rotor loop too)
    half_turn   |rot| = pi on a random axis, tor = +-pi
    wide        rot sigma 3, tor uniform in [-2 pi, 2 pi]
    rigid       no torsion updates (the kernel's null pointer, the reference's rigid branch)"""
import numpy as np
import pytest
import torch

import adversarial_geometry as ag

B = 3


def _figures(lig, cls, offset, mutant=None):
    c = ag.ligand(lig)
    pos = ag.poses(c, B, offset)
    tr, rot, tor = ag.updates(cls, c['mask_rotate'].shape[0], B, seed=7)
    with np.errstate(all='ignore'):
        got = ag.host_update(c, pos, tr, rot, tor, mutant)
    return ag.update_figures(c, pos, tr, rot, tor, got), got


def _broken(fig):
    return [k for k, (e, b, _) in fig.items() if not e <= b]


# ---- the generators ------------------------------------------------------------------------------------------------------------------------
def test_axis_angle_classes_have_their_properties():
    aa, cl = ag.axis_angle_vectors()
    ang = ag.angle_fp32(aa)
    assert 3500 <= len(aa) <= 4500 and aa.dtype == np.float32 and sum(len(v) for v in cl.values()) == len(aa)
    on_axis = (aa != 0).sum(1) == 1
    for name in ('log_small', 'branch', 'pi', 'large'):          # every one of these angles sits on coordinate axes AND on random axes
        assert on_axis[cl[name]].any() and (~on_axis[cl[name]]).any(), name
    a = ang[cl['log_small']]
    assert (a < ag.BRANCH).sum() > 1000 and (a > ag.BRANCH).any() and a.max() < 1.001e-5          # mostly the series branch, up to a decade past it
    assert (a == 0).any() and ((a > 0) & (a < 1e-19)).any()                                          # vanishing and subnormal squares are both in
    assert np.abs(aa[cl['log_small']]).max(1).min() > 0
    lo, hi = np.nextafter(ag.BRANCH, np.float32(0)), np.nextafter(ag.BRANCH, np.float32(1))
    b = ang[cl['branch']][on_axis[cl['branch']]]
    assert set(b.tolist()) == {float(lo), float(ag.BRANCH), float(hi)}          # both sides of `angle < 1e-6f` and the value itself
    assert (b < ag.BRANCH).any() and (b >= ag.BRANCH).any()
    u = aa[cl['underflow']]
    assert (u != 0).all() and (ang[cl['underflow']] == 0).all()                  # a non-zero vector whose fp32 angle is exactly 0
    assert np.linalg.norm(u.astype(np.float64), axis=1).min() > 0
    p = ang[cl['pi']][on_axis[cl['pi']]]
    for base in (np.float32(np.pi), np.float32(2 * np.pi)):
        near = np.unique(p[np.abs(p - base) < 1e-3])
        assert len(near) == 5 and near[2] == base and np.all(np.diff(near) == np.spacing(near[:4]))          # base and +-1, +-2 ulp
    assert ang[cl['large']].min() >= np.float32(2 * np.pi) * (1 - 1e-6) and ang[cl['large']].max() <= 100.0 * (1 + 1e-6) and ang[cl['large']].max() > 90
    assert not aa[cl['zero']].any() and np.signbit(aa[cl['zero']]).any()


@pytest.mark.parametrize('n', ag.KABSCH_N)
def test_kabsch_classes_have_their_properties(n):
    A, Bp, props = ag.kabsch_pairs(n)
    assert A.shape == Bp.shape == (len(ag.KABSCH_CLASSES), n, 3) and A.dtype == np.float32
    for i, name in enumerate(ag.KABSCH_CLASSES):
        degenerate = props[name]['gap'] < ag.GAP_DEGENERATE
        assert degenerate == (name == 'collinear' or n <= 2), (name, props[name])          # collinear sets, n <= 2 and only those
        if not degenerate:
            assert props[name]['gap'] > 1e-3, (name, props[name])                          # nothing sits near the threshold
    k = ag.KABSCH_CLASSES.index
    if n >= 4:      # (three points are planar: their mirror image IS a rotation of them, the third singular value is 0 and the sign of det has no meaning)
        for name in ag.REFLECTION_CLASSES:
            assert props[name]['det'] < -0.99, (name, props[name])
        assert props['generic']['det'] > 0.99 and props['rot_pi']['det'] > 0.99
    assert not A[k('planar')][:, 2].any()
    L = A[k('collinear')].astype(np.float64)
    assert not np.cross(L, L[-1]).any() and not L.sum(0).any()                             # exactly collinear, exactly centred: S has rank one
    assert np.array_equal(A[k('identical')], Bp[k('identical')])
    assert np.abs(A[k('offset150')]).max() > 140 and np.abs(A[k('scale_1e-3')]).max() < 0.02 and np.abs(A[k('scale_1e3')]).max() > 1e3 or n <= 2
    Rpi = ag.kabsch_ref(A[k('rot_pi')][None], Bp[k('rot_pi')][None])[0][0]
    if n >= 3:
        assert abs(np.trace(Rpi) + 1) < 1e-2          # rotation angle pi: trace = 1 + 2 cos(pi)


def test_ligands_have_their_rotor_counts():
    for n in ag.CHAIN_N:
        c = ag.ligand(f'chain{n}')
        uv = ag.rotors(c)
        assert c['lig_pos'].shape == (n, 3) and c['mask_rotate'].shape == (n - 3, n) == (len(uv), n)          # R = n - 3: 0, 1, 63, 64, 65, 128, 129, 253
        assert all(not c['mask_rotate'][r, u] and c['mask_rotate'][r, v] for r, (u, v) in enumerate(uv))
        bd = ag.bonds(c)
        assert np.array_equal(bd, np.stack([np.arange(n - 1), np.arange(1, n)], 1))
        assert np.abs(np.linalg.norm(c['lig_pos'][bd[:, 0]] - c['lig_pos'][bd[:, 1]], axis=1) - ag.BOND).max() < 1e-5
    p = ag.ligand('planar20')
    assert not p['lig_pos'][:, 2].any() and p['mask_rotate'].shape == (17, 20)
    br = ag.ligand('branched')
    assert len(ag.bonds(br)) >= len(br['lig_pos']) and br['mask_rotate'].shape[0] >= 4          # rings: at least as many bonds as atoms
    assert sorted(r for r in (ag.ligand(f'chain{n}')['mask_rotate'].shape[0] for n in ag.CHAIN_N)) == [0, 1, 63, 64, 65, 128, 129, 253]


def test_update_classes_have_their_properties():
    R = 65
    for cls in ag.UPDATE_CLASSES:
        tr, rot, tor = ag.updates(cls, R, B, seed=7)
        assert tr.dtype == rot.dtype == np.float32 and tr.shape == rot.shape == (B, 3) and (tor is None) == (cls == 'rigid')
        assert tor is None or (tor.dtype == np.float32 and tor.shape == (B, R))
    tr, rot, tor = ag.updates('zero', R, B)
    assert not tr.any() and not rot.any() and not tor.any()
    tr, rot, tor = ag.updates('tiny', R, B)
    a = ag.angle_fp32(rot)
    assert (a > 0).all() and (a < ag.BRANCH).all()                                        # the rotation really enters the series branch ...
    assert (tor[:, 0::2] != 0).all() and (np.abs(tor) < ag.BRANCH).all() and not tor[:, 1::2].any()          # ... and so does every other rotor; the rest are exact zeros
    axis = np.float32([0.6, 0.0, 0.8])
    assert (ag.angle_fp32(axis[None] * tor[:, 0:1]) < ag.BRANCH).all()                    # (the angle the rotor loop computes from unit axis * theta)
    tr, rot, tor = ag.updates('half_turn', R, B)
    assert np.abs(ag.angle_fp32(rot) - np.float32(np.pi)).max() < 1e-6 and (np.abs(tor) == np.float32(np.pi)).all() and (tor > 0).any() and (tor < 0).any()
    tr, rot, tor = ag.updates('wide', R, B)
    assert np.abs(tor).max() > np.pi and np.abs(tor).max() <= 2 * np.pi and ag.angle_fp32(rot).max() > np.pi
    for offset in ag.OFFSETS:
        p = ag.poses(ag.ligand('chain68'), B, offset)
        assert p.shape == (B, 68, 3) and (np.abs(p).max() > 150) == (offset > 0)


# ---- the restatement meets every bar ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', ag.OFFSETS)
@pytest.mark.parametrize('cls', ag.UPDATE_CLASSES)
@pytest.mark.parametrize('lig', ag.LIGANDS)
def test_host_update_meets_every_bar(lig, cls, offset):
    fig, got = _figures(lig, cls, offset)
    assert np.isfinite(got).all() and not _broken(fig), {k: ag.ratio(e, b) for k, (e, b, _) in fig.items()}
    assert ('zero' in fig) == (cls == 'zero')


def test_host_axis_angle_meets_every_bar():
    aa, cl = ag.axis_angle_vectors()
    R, R64, R32 = ag.host_axis_angle(aa), ag.axis_angle_ref(aa), ag.axis_angle_ref(aa, torch.float32)
    assert np.isfinite(R).all()
    for name, idx in cl.items():
        assert ag.max_err(R[idx], R64[idx]) <= ag.bar(ag.max_err(R32[idx], R64[idx])), name


@pytest.mark.parametrize('n', ag.KABSCH_N)
def test_host_kabsch_meets_every_bar(n):
    A, Bp, props = ag.kabsch_pairs(n)
    (R64, t64), (R32, t32) = ag.kabsch_ref(A, Bp), ag.kabsch_ref(A, Bp, torch.float32)
    P64, P32 = ag.aligned(A, R64, t64), ag.aligned(A, R32, t32)
    for i, name in enumerate(ag.KABSCH_CLASSES):
        R, t = ag.host_kabsch(A[i], Bp[i])
        assert np.isfinite(R).all() and np.isfinite(t).all(), name
        assert ag.max_err(ag.aligned(A[i:i + 1], R[None], t[None])[0], P64[i]) <= ag.bar(ag.max_err(P32[i], P64[i]), np.abs(Bp[i]).max()), name
        if props[name]['gap'] >= ag.GAP_DEGENERATE:
            assert ag.max_err(R, R64[i]) <= ag.bar(ag.max_err(R32[i], R64[i])), name
        orth, _ = ag.rotation_defect(R)
        assert np.linalg.det(R.astype(np.float64)) > 0 and orth[0] <= ag.FLOOR, name


# ---- invariants of the fp64 reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lig', ['chain4', 'chain68', 'chain256', 'planar20', 'branched'])
def test_reference_invariants_in_fp64(lig):
    """what the GPU module's `bond` and `centroid` comparisons rest on: the update changes no bond length and moves the centroid by exactly tr (to 1e-10)"""
    c = ag.ligand(lig)
    bd = ag.bonds(c)
    for offset in ag.OFFSETS:
        pos = ag.poses(c, B, offset)
        for cls in ag.UPDATE_CLASSES:
            tr, rot, tor = ag.updates(cls, c['mask_rotate'].shape[0], B, seed=7)
            out = ag.update_ref(c, pos, tr, rot, tor)
            p64 = pos.astype(np.float64)
            length = lambda p: np.linalg.norm(p[:, bd[:, 0]] - p[:, bd[:, 1]], axis=-1)
            assert np.abs(length(out) - length(p64)).max() < 1e-10, (cls, offset)
            assert np.abs(out.mean(1) - (p64.mean(1) + tr.astype(np.float64))).max() < 1e-10, (cls, offset)


# ---- the bars bite ---------------------------------------------------------------------------------------------------------------------------
def test_mutant_torsions_on_the_original_coordinates():
    fig, _ = _figures('chain66', 'typical', 0.0, 'stale_torsion')
    assert 'pos' in _broken(fig) and 'bond' in _broken(fig)
    assert not _broken(_figures('chain4', 'typical', 0.0, 'stale_torsion')[0])          # one rotor: nothing has moved before it (why R = 1 alone pins nothing)


def test_mutant_pivot_at_u_is_the_same_rotation():
    """The axis of a rotor passes through BOTH of its atoms: R (x - v - a) + v + a = R (x - v) + v for a = u - v, because R a = a.  A pivot taken at u is the
    same map, not an error - no class can tell it apart and none must; the restatement with the pivot at u meets every bar like the one with the pivot at v.
    The neighbouring REAL error - u and v exchanged in the axis, which turns the rotor the other way - breaks the bars at every size."""
    for lig in ('chain68', 'branched'):
        for offset in ag.OFFSETS:
            assert not _broken(_figures(lig, 'wide', offset, 'pivot_u')[0])
            assert 'pos' in _broken(_figures(lig, 'wide', offset, 'reversed_axis')[0])
    assert 'pos' in _broken(_figures('chain4', 'typical', 0.0, 'reversed_axis')[0])


def test_mutant_kabsch_step_dropped():
    for lig in ('chain4', 'chain68', 'branched'):
        fig, _ = _figures(lig, 'typical', 0.0, 'no_kabsch')
        assert 'pos' in _broken(fig) and 'centroid' in _broken(fig) and 'bond' not in _broken(fig)          # (still an isometry of every bond)


def test_mutant_svd_product_without_reflection_correction():
    k = ag.KABSCH_CLASSES.index
    for n in (4, 12, 256):
        A, Bp, _ = ag.kabsch_pairs(n)
        (R64, t64), (R32, t32) = ag.kabsch_ref(A, Bp), ag.kabsch_ref(A, Bp, torch.float32)
        for name in ag.REFLECTION_CLASSES:
            i = k(name)
            R, t = ag.host_kabsch(A[i], Bp[i], 'no_reflection_fix')
            assert np.linalg.det(R.astype(np.float64)) < 0          # breaks det R > 0 ...
            P64, P32 = ag.aligned(A[i:i + 1], R64[i:i + 1], t64[i:i + 1]), ag.aligned(A[i:i + 1], R32[i:i + 1], t32[i:i + 1])
            assert ag.max_err(R, R64[i]) > ag.bar(ag.max_err(R32[i], R64[i]))          # ... the bar on R ...
            if name == 'reflection_noise':      # ... and the aligned positions (the exact mirror image is reached by the improper matrix, which is the point of the class)
                assert ag.max_err(ag.aligned(A[i:i + 1], R[None], t[None]), P64) > ag.bar(ag.max_err(P32, P64), np.abs(Bp[i]).max())
        R, t = ag.host_kabsch(A[k('generic')], Bp[k('generic')], 'no_reflection_fix')          # harmless where the optimum is proper
        assert ag.max_err(R, R64[k('generic')]) <= ag.bar(ag.max_err(R32[k('generic')], R64[k('generic')]))


def test_mutant_small_angle_branch_removed():
    for lig in ('chain4', 'chain68'):
        fig, got = _figures(lig, 'zero', 0.0, 'no_small_angle')
        assert not np.isfinite(got).all() and set(_broken(fig)) == {'pos', 'bond', 'centroid', 'zero'}          # NaN at angle 0 never passes
    fig, got = _figures('chain68', 'tiny', 0.0, 'no_small_angle')          # the exact zeros among the tiny torsions
    assert 'pos' in _broken(fig)
    R = ag.host_axis_angle(ag.axis_angle_vectors()[0], small_angle_branch=False)
    assert not np.isfinite(R).all()


def test_mutant_chunk_offset_slip():
    for lig in ('chain68', 'chain132', 'chain256'):          # R = 65, 129, 253
        assert 'pos' in _broken(_figures(lig, 'typical', 0.0, 'chunk_slip')[0]), lig
    a, b = _figures('chain67', 'typical', 0.0, 'chunk_slip')[1], _figures('chain67', 'typical', 0.0)[1]
    assert np.array_equal(a, b)          # R = 64: no rotor of a second chunk - why 65 is in the set


def test_mutant_sequential_fp32_centroid():
    """the form the kernels had: within the bars at the origin, outside the `centroid` bar for a half turn 150 A out, and outside the aligned-position bar of
    the `offset150` Kabsch pair of 256 points"""
    assert not _broken(_figures('chain256', 'wide', 0.0, 'fp32_centroid')[0])
    for lig in ('chain68', 'chain256'):          # (I - R) x the centroid's error reaches the output: largest for the half turn, where |I - R| = 2
        assert 'centroid' in _broken(_figures(lig, 'half_turn', 150.0, 'fp32_centroid')[0]), lig
    A, Bp, _ = ag.kabsch_pairs(256)
    i = ag.KABSCH_CLASSES.index('offset150')
    (R64, t64), (R32, t32) = ag.kabsch_ref(A[i:i + 1], Bp[i:i + 1]), ag.kabsch_ref(A[i:i + 1], Bp[i:i + 1], torch.float32)
    R, t = ag.host_kabsch(A[i], Bp[i], 'fp32_centroid')
    P64 = ag.aligned(A[i:i + 1], R64, t64)
    assert ag.max_err(ag.aligned(A[i:i + 1], R[None], t[None]), P64) > ag.bar(ag.max_err(ag.aligned(A[i:i + 1], R32, t32), P64), np.abs(Bp[i]).max())


def test_uncentred_form_loses_digits_far_from_the_origin():
    """the form the kernel had: tr + centroid added BEFORE the rotor loop, so that the rotor axes and every rotated atom carry roundings of the distance from the
    origin.  The same map, and indistinguishable at the origin; 150 A out its error on the long chains is that of the fp32 reference (up to 8.9 x of it on one
    ill-conditioned sample of the 129-rotor chain, where half an ulp on the input already moves the fp64 result by 1.5e-3 A: two fp32 evaluations of such a
    chain can differ by a decade), while the centred form stays below the fp32 reference's error there and at least 3 x below the uncentred form's"""
    assert not _broken(_figures('chain132', 'typical', 0.0, 'uncentred')[0])
    for lig in ('chain68', 'chain132', 'chain256'):
        for cls in ('typical', 'half_turn', 'wide'):
            e, _, e32 = _figures(lig, cls, 150.0)[0]['pos']
            eu = _figures(lig, cls, 150.0, 'uncentred')[0]['pos'][0]
            assert e < e32 and 3 * e < eu, (lig, cls, e, e32, eu)
