"""CPU checks of tests/pairwise_ref.py: the references of the pairwise pose RMSD and the pose clustering have the properties they claim, the generators
deliver what they promise, and the bar that tests/test_gpu_pairwise.py holds the kernel to bites on the `far` class."""
import numpy as np

import adversarial_geometry as ag
import pairwise_ref as pr


def test_matrix_is_symmetric_with_zero_diagonal():
    pos = pr.typical(7, 21, seed=1)
    mask = np.arange(21) % 3 != 0
    for kw in (dict(), dict(mask=mask), dict(perms=pr.random_table(5, 21)), dict(mask=mask, perms=pr.random_table(5, 21))):
        d = pr.pairwise_rmsd_ref(pos, **kw)
        assert np.array_equal(d, d.T) and (np.diag(d) == 0).all() and (d[~np.eye(7, dtype=bool)] > 0).all()
    assert np.array_equal(pr.pairwise_rmsd_ref(pos[:1]), np.zeros((1, 1)))
    assert np.array_equal(pr.pairwise_rmsd_ref(pos, mask=np.zeros(21, bool)), np.zeros((7, 7)))


def test_matrix_is_the_plain_definition():
    """against the definition written as loops, entry by entry (the lower-indexed pose is the permuted one)"""
    pos = pr.typical(4, 9, seed=2).astype(np.float64)
    mask = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    table = pr.random_table(3, 9, seed=3)
    d = pr.pairwise_rmsd_ref(pos, mask, table)
    for i in range(4):
        for j in range(i + 1, 4):
            want = min(np.sqrt(sum(((pos[i][row[a]] - pos[j][a]) ** 2).sum() for a in range(9) if mask[a]) / mask.sum()) for row in table)
            assert abs(d[i, j] - want) < 1e-12 and d[j, i] == d[i, j]


def test_invariant_under_a_common_rigid_motion():
    rng = np.random.default_rng(0)
    pos = pr.typical(6, 30, seed=4).astype(np.float64)
    R, t = pr._rotation(rng, 2.1), np.array([31.0, -7.0, 12.5])
    table = pr.random_table(4, 30, seed=5)
    assert np.abs(pr.pairwise_rmsd_ref(pos @ R.T + t, perms=table) - pr.pairwise_rmsd_ref(pos, perms=table)).max() < 1e-12


def test_automorphic_poses_are_at_zero_only_with_the_table():
    x, table = pr.symmetric_ligand(20, seed=6)
    pos = np.stack([x[g] for g in table])            # the same pose under every relabelling of the group
    assert np.array_equal(pr.pairwise_rmsd_ref(pos, perms=table), np.zeros((8, 8)))
    ident = pr.pairwise_rmsd_ref(pos, perms=table[:1])
    assert np.array_equal(ident, pr.pairwise_rmsd_ref(pos)) and (ident[~np.eye(8, dtype=bool)] > 0.1).all()


def test_invalid_rows_never_win():
    pos = pr.typical(3, 12, seed=7)
    table = pr.random_table(4, 12, seed=8)
    only_last = pr.spoil_rows(table, [0, 1, 2])
    assert np.array_equal(pr.pairwise_rmsd_ref(pos, perms=only_last), pr.pairwise_rmsd_ref(pos, perms=table[3:]))
    none = pr.pairwise_rmsd_ref(pos, perms=pr.spoil_rows(table, [0, 1, 2, 3]))
    off = ~np.eye(3, dtype=bool)
    assert np.isposinf(none[off]).all() and (np.diag(none) == 0).all()
    # an entry outside the ligand at a masked-out atom does not count
    keep = np.ones(12, bool)
    keep[5] = False
    t = table.copy()
    t[:, 5] = -1
    assert np.array_equal(pr.pairwise_rmsd_ref(pos, keep, t), pr.pairwise_rmsd_ref(pos, keep, table))


def test_cluster_ref_recovers_the_planted_modes_with_leaders_in_score_order():
    x, table = pr.symmetric_ligand(24, seed=0)
    pos, labels = pr.modes(perms=table)
    assert len(pos) == 40
    rng = np.random.default_rng(1)
    score = rng.normal(size=40).astype(np.float32)
    d = pr.pairwise_rmsd_ref(pos, perms=table)
    cluster, leaders, n = pr.cluster_ref(d, score, pr.CUTOFF)
    assert n == 4 and pr.same_partition(cluster, labels)
    lead = leaders[:n]
    assert (leaders[n:] == -1).all() and (np.diff(score[lead]) <= 0).all()
    for k in range(n):            # a leader is the best-scored pose of its mode, and cluster ordinals follow the leaders
        members = np.flatnonzero(cluster == k)
        assert lead[k] == members[np.argmax(score[members])] and cluster[lead[k]] == k
    # without the table the relabelled poses of a mode fall apart
    assert pr.cluster_ref(pr.pairwise_rmsd_ref(pos), score, pr.CUTOFF)[2] > 4


def test_tie_and_nan_ordering():
    nan, inf = np.nan, np.inf
    assert pr.rank_order(None, 3) == [0, 1, 2]
    assert pr.rank_order([1.0, 2.0, 2.0, 1.0], 4) == [1, 2, 0, 3]
    assert pr.rank_order([nan, -inf, 0.0, nan, inf, -0.0], 6) == [4, 2, 5, 1, 0, 3]
    # the ranking decides the leaders: two poses far apart, the NaN one is never first
    d = np.array([[0, 9], [9, 0]], np.float32)
    assert pr.cluster_ref(d, [nan, -inf], 2.0)[1].tolist() == [1, 0]
    assert pr.cluster_ref(d, [0.5, 0.5], 2.0)[1].tolist() == [0, 1]


def test_cluster_ref_edges():
    inf = np.inf
    d = np.array([[0, 1, 2, inf], [1, 0, 1, 5], [2, 1, 0, 5], [inf, 5, 5, 0]], np.float32)
    assert pr.cluster_ref(d, None, 1.0)[0].tolist() == [0, 0, 1, 2]          # an entry equal to the cutoff joins; 2 is not within 1 of leader 0
    assert pr.cluster_ref(d, None, 0.0)[2] == 4
    c, lead, n = pr.cluster_ref(d, None, np.inf)                              # an infinite distance never joins
    assert c.tolist() == [0, 0, 0, 1] and lead.tolist() == [0, 3, -1, -1] and n == 2
    assert pr.cluster_ref(np.zeros((1, 1), np.float32), None, 2.0)[0].tolist() == [0]


def test_the_bar_bites_on_far():
    """150 A out the numpy fp32 restatement is off by a non-zero amount that stays far below the bar's floor (8 * 2^-24 * 150 A = 7e-5 A): the bar
    leaves room for fp32 roundings of the coordinates' size and for nothing else - the expanded form |a|^2 + |b|^2 - 2ab is three orders outside it."""
    pos = pr.far()
    assert np.abs(pos).min() > 140
    d64, d32 = pr.pairwise_rmsd_ref(pos), pr.pairwise_rmsd_ref(pos, dtype=np.float32)
    off = ~np.eye(len(pos), dtype=bool)
    assert 0.1 < d64[off].min() and d64[off].max() < 1.5
    err32 = ag.max_err(d32, d64)
    the_bar = ag.bar(err32, np.abs(pos).max())
    assert 0 < err32 < the_bar < 1e-4
    p = pos.astype(np.float32)
    sq = (p * p).sum(-1, dtype=np.float32)                                    # [B, n]
    expanded = sq[:, None] + sq[None] - np.float32(2) * np.einsum('iak,jak->ija', p, p)
    bad = np.sqrt(np.maximum(expanded.mean(-1, dtype=np.float32), 0))
    assert ag.max_err(bad[off], d64[off]) > 10 * the_bar
