"""The pairwise pose RMSD and the pose clustering on the device (csrc/k_pairs.hip) through the C ABI: ddk_pose_pairwise_rmsd against numpy fp64,
ddk_pose_cluster integer for integer against the plain loop, the two Python entries end to end, and the refusals.  tests/pairwise_ref.py holds the
references and generators (tests/test_pairwise_host.py checks them on the CPU).

Values are held to the project's bar, adversarial_geometry.bar(err32, scale) = max(4 * err32, 8 * 2^-24 * scale): err32 is the error of the numpy fp32
restatement against fp64 on the SAME input, computed at run time, scale is max |coordinate|.  Shapes sit on the kernel's edges: B in {1, 2, 3, TJ, TJ + 1,
2 TJ + 1} (no pair, an odd count, the tile edges of the TJ = 8 partner poses of a workgroup), n_lig in {1, 63, 65, 256} (one atom, both sides of a wave,
the limit), n_perms in {0, 1, 5, 17} (no table, one row, a few, one more than the 16 rows of the kernel's first pass).

Figures are kept through _record_drift under pairwise_rmsd_<class>_n<n_lig>_B<B>: the worst K * error / bar over the table sizes (4 sits on the bar).
Measured on an MI355X (profiles/pairwise_rmsd_drift.json), worst figure per class over every n_lig and B: typical 1.13, one_kept 1.13, last_row 1.13 (all at
n_lig = 1, where a pair is three differences and one square root: the kernel's error is the fp32 restatement's; 0.4 - 0.8 at 256 atoms), far 0.005 (the
floor 8 * 2^-24 * 150 A rules there and the differences of nearby coordinates are exact), none_kept and no_valid_row 0 (exact zeros / +inf)."""
import ctypes as C

import numpy as np
import pytest
import torch

import adversarial_geometry as ag
import pairwise_ref as pr

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(a, dt, dev):
    return None if a is None else T(np.ascontiguousarray(a, dt)).to(dev)


def _pairs_raw(ctx, dev, pos, mask=None, perms=None):
    """ddk_pose_pairwise_rmsd through the C ABI (Context.pairwise_rmsd refuses a table with an entry outside the ligand before the kernel sees it)"""
    d_pos, d_m, d_pm = _up(pos, np.float32, dev), _up(mask, np.uint8, dev), _up(perms, np.int32, dev)
    B, n = pos.shape[0], pos.shape[1]
    out = torch.full((B, B), float('nan'), dtype=torch.float32, device=dev)
    ctx._check(ctx.L.ddk_pose_pairwise_rmsd(ctx.h, B, n, _ptr(d_pos), _ptr(d_m), _ptr(d_pm), 0 if perms is None else len(perms), _ptr(out), _stream()),
               'ddk_pose_pairwise_rmsd')
    return out.cpu().numpy()


def _cluster_raw(ctx, dev, rmsd, score, cutoff):
    """ddk_pose_cluster through the C ABI -> (cluster, leaders, n_clusters) on the host"""
    B = rmsd.shape[0]
    d_r = rmsd if torch.is_tensor(rmsd) else _up(rmsd, np.float32, dev)
    d_s = _up(score, np.float32, dev)
    cluster, leaders = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ctx._check(ctx.L.ddk_pose_cluster(ctx.h, B, _ptr(d_r), _ptr(d_s), float(cutoff), _ptr(cluster), _ptr(leaders), _ptr(n), _stream()), 'ddk_pose_cluster')
    return cluster.cpu().numpy(), leaders.cpu().numpy(), int(n.cpu()[0])


def _figure(got, pos, mask, perms):
    """(ok, K * error / bar) of a device matrix against numpy fp64; an infinite reference entry must be met by +inf, nothing may be NaN"""
    d64, d32 = pr.pairwise_rmsd_ref(pos, mask, perms), pr.pairwise_rmsd_ref(pos, mask, perms, dtype=np.float32)
    if np.isnan(got).any():
        return False, float('inf')
    inf = np.isinf(d64)
    if not ((np.isinf(got) == inf).all() and (got[inf] > 0).all()):
        return False, float('inf')
    the_bar = ag.bar(ag.max_err(d32[~inf], d64[~inf]), np.abs(pos).max())
    err = ag.max_err(got[~inf], d64[~inf])
    return err <= the_bar, ag.ratio(err, the_bar)


CLASSES = ('typical', 'far', 'one_kept', 'none_kept', 'last_row', 'no_valid_row')
BATCHES = (1, 2, 3, 8, 9, 17)
TABLES = (0, 1, 5, 17)


def test_shapes_sit_on_the_kernel_edges():
    from disco_diffdock_amd import runtime
    TJ = runtime.PAIRS_TJ
    assert BATCHES == (1, 2, 3, TJ, TJ + 1, 2 * TJ + 1) and TABLES == (0, 1, 5, runtime.PAIRS_ROWS_PER_PASS + 1)


def _case(cls, B, n, n_perms, seed):
    """(pos, mask, perms) of one class; masks carry entries outside the ligand at masked-out atoms of the table (they must be ignored)"""
    rng = np.random.default_rng(seed)
    pos = pr.far(B, n, seed) if cls == 'far' else pr.typical(B, n, seed)
    mask, perms = None, (pr.random_table(n_perms, n, seed) if n_perms else None)
    if cls == 'typical' and n > 2:
        mask = rng.random(n) < 0.7
        mask[:2] = (True, False)
    if cls == 'one_kept':
        mask = np.zeros(n, bool)
        mask[(137 * n) // 256] = True
    if cls == 'none_kept':
        mask = np.zeros(n, bool)
    if perms is not None and mask is not None:
        perms[:, ~mask] = rng.choice([-1, n, 2 ** 31 - 1], size=(n_perms, int((~mask).sum())))
    if cls == 'last_row':
        perms = pr.spoil_rows(perms, range(n_perms - 1), seed=seed)
    if cls == 'no_valid_row':
        perms = pr.spoil_rows(perms, range(n_perms), seed=seed)
    return pos, mask, perms


@pytest.mark.parametrize('n', (1, 63, 65, 256))
def test_pairwise_rmsd_against_fp64(dev, ctx, n):
    """every class x B x table size at one ligand size: values within the bar of numpy fp64, exact symmetry, an exactly zero diagonal, bit-identical
    results from two runs; an all-false mask gives exactly zeros; no valid row gives +inf off the diagonal and 0 on it, never NaN"""
    from test_gpu_round3 import _record_drift
    bad = []
    for cls in CLASSES:
        worst_of_class = 0.0
        for B in BATCHES:
            worst = 0.0
            for n_perms in TABLES:
                if n_perms == 0 and cls in ('last_row', 'no_valid_row'):
                    continue
                pos, mask, perms = _case(cls, B, n, n_perms, seed=1000 * n + 10 * B + n_perms)
                got = _pairs_raw(ctx, dev, pos, mask, perms)
                again = _pairs_raw(ctx, dev, pos, mask, perms)
                ok, fig = _figure(got, pos, mask, perms)
                ok = ok and np.array_equal(got, got.T) and (np.diag(got) == 0).all() and got.tobytes() == again.tobytes()
                off = ~np.eye(B, dtype=bool)
                if cls == 'none_kept':
                    ok = ok and np.array_equal(got, np.zeros((B, B), np.float32))
                if cls == 'no_valid_row':
                    ok = ok and np.isposinf(got[off]).all()
                if cls in ('typical', 'far', 'one_kept', 'last_row'):
                    ok = ok and np.isfinite(got).all()
                worst = max(worst, fig)
                if not ok:
                    bad.append((cls, B, n_perms, fig))
            _record_drift(f'pairwise_rmsd_{cls}_n{n}_B{B}', worst, bar=ag.K)
            worst_of_class = max(worst_of_class, worst)
        print(f'pairwise_rmsd n = {n} {cls:12s}: worst figure over B and the table sizes {worst_of_class:.2f} (the bar is {ag.K:.0f})')
    assert not bad, bad


def test_pairwise_rmsd_on_a_symmetric_ligand(dev, ctx):
    """poses that differ by an automorphism only: exactly 0 with the table (differences of equal numbers), more than 0 with the identity alone"""
    x, table = pr.symmetric_ligand(20, seed=6)
    pos = np.stack([x[g] for g in table]).astype(np.float32)
    assert np.array_equal(_pairs_raw(ctx, dev, pos, perms=table), np.zeros((8, 8), np.float32))
    assert (_pairs_raw(ctx, dev, pos)[~np.eye(8, dtype=bool)] > 0.1).all()


def test_pairwise_rmsd_agrees_with_pose_metrics(dev, ctx):
    """out[i][j] = the rmsd of Complex.pose_metrics(pos[i], ref_pos = pos[j]) within the same bar, with and without mask and table"""
    from disco_diffdock_amd.runtime import Complex
    lig = ag.ligand('chain66')
    n = len(lig['lig_pos'])
    cx = Complex(ctx, lig, max_batch=4)
    pos = pr.typical(9, n, seed=3)
    mask = np.arange(n) % 4 != 1
    table = pr.random_table(5, n, seed=4)
    d_pos = T(pos).to(dev)
    for kw in (dict(), dict(mask=mask), dict(perms=table), dict(mask=mask, perms=table)):
        got = _pairs_raw(ctx, dev, pos, **kw)
        d64, d32 = pr.pairwise_rmsd_ref(pos, **kw), pr.pairwise_rmsd_ref(pos, dtype=np.float32, **kw)
        the_bar = ag.bar(ag.max_err(d32, d64), np.abs(pos).max())
        for i, j in ((0, 1), (0, 8), (3, 4), (7, 8), (2, 6)):
            m = cx.pose_metrics(d_pos[i:i + 1], d_pos[j], atom_mask=None if 'mask' not in kw else T(mask), perms=kw.get('perms'))[0, 0].item()
            assert abs(float(got[i, j]) - m) <= the_bar, (kw.keys(), i, j, got[i, j], m, the_bar)


def _cluster_poses(B, seed):
    """B poses of a 5-atom ligand scattered so that a 2 A cutoff finds many clusters of several poses"""
    rng = np.random.default_rng(seed)
    base = pr.conformer(5, seed)
    sites = rng.uniform(-6, 6, size=(max(B // 8, 1), 3))
    return np.stack([base + sites[rng.integers(len(sites))] + rng.normal(0, 0.4, size=(5, 3)) for _ in range(B)]).astype(np.float32)


@pytest.mark.parametrize('B', (1, 2, 40, 1024))
def test_cluster_is_the_plain_loop_exactly(dev, ctx, B):
    """ddk_pose_cluster on the device's own fp32 matrix against cluster_ref, integer for integer: scores with ties, a NaN score, score = NULL, a matrix with
    inf entries, cutoff = 0 (only exact duplicates join), cutoff = inf (one cluster), and a cutoff equal bit for bit to an entry (which must join)"""
    rng = np.random.default_rng(B)
    pos = _cluster_poses(B, seed=B)
    if B >= 4:
        pos[B // 2], pos[B - 1] = pos[1], pos[1]          # exact duplicates of pose 1: distance 0 to it and to each other
    d_dev = _up(pos, np.float32, dev)
    rmsd = torch.empty((B, B), dtype=torch.float32, device=dev)
    ctx._check(ctx.L.ddk_pose_pairwise_rmsd(ctx.h, B, 5, _ptr(d_dev), None, None, 0, _ptr(rmsd), _stream()), 'ddk_pose_pairwise_rmsd')
    d = rmsd.cpu().numpy()
    ties = np.round(rng.normal(size=B) * 2).astype(np.float32) / 2          # a handful of distinct values: ties everywhere
    with_nan = rng.normal(size=B).astype(np.float32)
    with_nan[rng.integers(B)] = np.nan
    with_nan[0] = -np.inf if B > 1 and not np.isnan(with_nan[0]) else with_nan[0]
    holes = d.copy()
    if B > 1:
        i, j = rng.integers(B, size=(2, 4 * B))
        off = i != j
        holes[i[off], j[off]] = np.inf
        holes[j[off], i[off]] = np.inf
    equal = float(d[0, B // 3]) if B > 2 else 2.0                          # leader 0 under score = NULL: sample B // 3 sits exactly on the cutoff
    cases = [('ties', d, ties, 2.0), ('nan', d, with_nan, 2.0), ('null', d, None, 2.0), ('inf entries', holes, ties, 2.0),
             ('inf entries, cutoff inf', holes, None, np.inf), ('cutoff 0', d, with_nan, 0.0), ('cutoff inf', d, ties, np.inf), ('on the cutoff', d, None, equal)]
    for name, mat, score, cutoff in cases:
        got = _cluster_raw(ctx, dev, rmsd if mat is d else mat, score, cutoff)
        want = pr.cluster_ref(mat, score, cutoff)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, got[2], want[2])
        if name == 'cutoff inf':
            assert got[2] == 1 and (got[0] == 0).all()
        if name == 'cutoff 0' and B >= 4:
            assert got[2] == B - 2 and got[0][1] == got[0][B // 2] == got[0][B - 1]
        if name == 'on the cutoff' and B > 2:
            assert got[0][B // 3] == 0
    if B == 40:
        assert 1 < pr.cluster_ref(d, ties, 2.0)[2] < B          # the premise: several clusters of several poses


def _planted(dev):
    x, table = pr.symmetric_ligand(24, seed=0)
    moved = (table != np.arange(24)).any(0)
    mask = np.ones(24, bool)
    mask[np.flatnonzero(~moved)[::3]] = False                  # 'hydrogens': atoms that no row of the table moves
    pos, labels = pr.modes(M=3, per_mode=13, outliers=1, n_lig=24, seed=0, mask=mask, perms=table)
    score = np.random.default_rng(5).normal(size=len(pos)).astype(np.float32)
    want = pr.cluster_ref(pr.pairwise_rmsd_ref(pos, mask, table), score, pr.CUTOFF)
    assert want[2] == 4 and pr.same_partition(want[0], labels)
    return pos, mask, table, score, want


def test_cluster_poses_end_to_end(dev, ctx):
    """Context.cluster_poses and sampling.cluster_poses on 3 modes x 13 poses + 1 outlier (B = 40) with a permutation table, a mask and random scores:
    the planted partition, as the fp64 reference clusters it"""
    from disco_diffdock_amd import sampling
    from disco_diffdock_amd.data import HeteroData
    pos, mask, table, score, want = _planted(dev)
    d_pos, d_score = T(pos).to(dev), T(score).to(dev)
    res = ctx.cluster_poses(d_pos, scores=d_score, cutoff=pr.CUTOFF, atom_mask=T(mask), perms=table)
    assert all(t.is_cuda for t in res) and res.rmsd.shape == (40, 40) and res.n_clusters.shape == (1,)
    assert np.array_equal(res.cluster.cpu().numpy(), want[0]) and np.array_equal(res.leaders.cpu().numpy(), want[1]) and int(res.n_clusters.cpu()[0]) == 4
    assert torch.equal(res.rmsd, ctx.pairwise_rmsd(d_pos, atom_mask=T(mask), perms=table))
    # the list sampling() returns: one graph per pose, ['ligand'].pos on the device, the element column of ['ligand'].x zero for hydrogens
    x = torch.zeros((24, 3), dtype=torch.long)
    x[:, 0] = T(mask.astype(np.int64)) * 5
    data_list = []
    for p in d_pos:
        g = HeteroData()
        g['ligand'].pos, g['ligand'].x = p, x
        data_list.append(g)
    conf = torch.stack([d_score, -d_score], dim=1)           # [B, k]: column 0 ranks
    res2 = sampling.cluster_poses(data_list, confidence=conf, cutoff=pr.CUTOFF, perms=table, ctx=ctx)
    assert all(torch.equal(a, b) for a, b in zip(res, res2))
    res3 = sampling.cluster_poses(data_list, confidence=d_score.cpu(), perms=table)          # the default context; a host confidence is uploaded
    assert all(torch.equal(a, b) for a, b in zip(res, res3))
    # all atoms and no table: the relabelled poses of a mode fall apart
    assert int(sampling.cluster_poses(data_list, confidence=conf, heavy_atoms_only=False, ctx=ctx).n_clusters.cpu()[0]) > 4


def test_refusals_leave_the_context_usable(dev, ctx):
    """B = 0, n_lig = 257, B = 1025 for the cluster call, a CPU tensor, n_perms > 0 with perms = NULL: RuntimeError with the ddk_last_error text"""
    pos = T(pr.typical(3, 7, seed=1)).to(dev)
    with pytest.raises(RuntimeError, match=r'B must be in \[1, 4096\]'):
        ctx.pairwise_rmsd(pos[:0])
    with pytest.raises(RuntimeError, match=r'n_lig must be in \[1, 256\]'):
        ctx.pairwise_rmsd(torch.zeros((2, 257, 3), device=dev))
    big = torch.zeros((1025, 1025), device=dev)
    out = torch.zeros(1025, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r'ddk_pose_cluster: B must be in \[1, 1024\]'):
        ctx._check(ctx.L.ddk_pose_cluster(ctx.h, 1025, _ptr(big), None, 2.0, _ptr(out), _ptr(out), _ptr(out), _stream()), 'ddk_pose_cluster')
    with pytest.raises(RuntimeError, match=r'B must be in \[1, 1024\]'):
        ctx.cluster_poses(torch.zeros((1025, 2, 3), device=dev))
    with pytest.raises(RuntimeError, match='device tensors only'):
        ctx.pairwise_rmsd(pos.cpu())
    with pytest.raises(RuntimeError, match='device tensors only'):
        ctx.cluster_poses(pos, scores=torch.zeros(3))
    res = torch.zeros((3, 3), device=dev)
    with pytest.raises(RuntimeError, match='perms / n_perms come in a pair'):
        ctx._check(ctx.L.ddk_pose_pairwise_rmsd(ctx.h, 3, 7, _ptr(pos), None, None, 2, _ptr(res), _stream()), 'ddk_pose_pairwise_rmsd')
    with pytest.raises(RuntimeError, match='ligand atom indices'):
        ctx.pairwise_rmsd(pos, perms=np.array([[0, 1, 2, 3, 4, 5, 7]]))
    got = ctx.cluster_poses(pos, cutoff=np.inf)
    assert got.cluster.cpu().tolist() == [0, 0, 0] and got.leaders.cpu().tolist() == [0, -1, -1] and got.n_clusters.cpu().tolist() == [1]
