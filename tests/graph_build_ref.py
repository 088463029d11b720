"""The specification of the three table builders of csrc/k_build.hip (ddk_receptor_knn_graph, ddk_radius_graph, ddk_ligand_transformation_mask in
include/ddk.h) in numpy, with the tie rules spelled out, and the inputs their tests run on.

Distances: the fp32 coordinates are converted to float64, subtracted, d2 = dx*dx + dy*dy + dz*dz in float64, compared with float64(float32(r)) ** 2,
strictly below; neighbours are ordered by a stable sort on (d2, j).  On the lattices below (coordinates that are multiples of 3) every step is exact, so
the ties and the pairs exactly at the cutoff are decided the same way everywhere; the random inputs are checked to stay away from both
(``knn_margins`` / ``radius_margins``), and then the comparison with the device and with the generators of synthetic.py is exact, not tolerant."""
import numpy as np

STATUS_OK, STATUS_OVERFLOW, STATUS_BAD_INPUT, STATUS_DISCONNECTED = 0, 1, 2, 3


def d2_rows(pos, lo, hi):
    """d2 [hi - lo, n] of the rows lo..hi in float64, the sum in the order dx*dx + dy*dy + dz*dz"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    d = p[None, :, :] - p[lo:hi, None, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _r2(r):
    return float(np.float32(r)) * float(np.float32(r))


def knn_graph_ref(pos, cutoff=15.0, max_neighbor=24):
    """-> (edge_index [2, E] int64 columns [i; j] grouped by i, status)"""
    pos = np.asarray(pos, np.float32)
    n, c2 = len(pos), _r2(cutoff)
    if not np.isfinite(pos).all():
        return np.zeros((2, 0), np.int64), STATUS_BAD_INPUT
    src, dst = [], []
    for lo in range(0, n, 512):
        D = d2_rows(pos, lo, min(lo + 512, n))
        for r, d2 in enumerate(D):
            i = lo + r
            others = np.delete(np.arange(n), i)          # self leaves by its index
            nb = others[d2[others] < c2]                 # ascending j
            if len(nb) > max_neighbor or len(nb) == 0:
                order = np.lexsort((others, d2[others]))          # stable on (d2, j): nearest first, ties to the lower index
                nb = others[order[:max_neighbor if len(nb) else 1]]
            src += [i] * len(nb)
            dst += nb.tolist()
    return np.asarray([src, dst], np.int64).reshape(2, -1), STATUS_OK


def radius_graph_ref(pos, r=5.0, max_num_neighbors=8):
    """-> (edge_index [2, E] int64 columns [neighbour; centre] grouped by centre, status); E is what the graph needs (the caller compares it with cap)"""
    pos = np.asarray(pos, np.float32)
    n, r2 = len(pos), _r2(r)
    if not np.isfinite(pos).all():
        return np.zeros((2, 0), np.int64), STATUS_BAD_INPUT
    row, col = [], []
    for lo in range(0, n, 512):
        D = d2_rows(pos, lo, min(lo + 512, n))
        for k, d2 in enumerate(D):
            i = lo + k
            nb = np.nonzero(d2 < r2)[0][:max_num_neighbors + 1]          # self is one of them; dropped afterwards
            nb = nb[nb != i]
            row += nb.tolist()
            col += [i] * len(nb)
    return np.asarray([row, col], np.int64).reshape(2, -1), STATUS_OK


def transformation_mask_ref(n_lig, bond_index):
    """-> (edge_mask [M] uint8, mask_rotate [R, n_lig] uint8, status).  Status 2 / 3: the masks are all 0 and R = 0."""
    bi = np.asarray(bond_index, np.int64).reshape(2, -1)
    M = bi.shape[1]
    none = (np.zeros(M, np.uint8), np.zeros((0, n_lig), np.uint8))
    seen = set()
    for k in range(M // 2):
        u, v = int(bi[0, 2 * k]), int(bi[1, 2 * k])
        if not (0 <= u < n_lig and 0 <= v < n_lig) or u == v or (int(bi[0, 2 * k + 1]), int(bi[1, 2 * k + 1])) != (v, u) or frozenset((u, v)) in seen:
            return none + (STATUS_BAD_INPUT,)
        seen.add(frozenset((u, v)))
    adj = [set() for _ in range(n_lig)]
    for k in range(M // 2):
        u, v = int(bi[0, 2 * k]), int(bi[1, 2 * k])
        adj[u].add(v)
        adj[v].add(u)

    def side(start, cut):
        got, stack = {start}, [start]
        while stack:
            a = stack.pop()
            for b in adj[a]:
                if {a, b} != cut and b not in got:
                    got.add(b)
                    stack.append(b)
        return got

    if len(side(0, set())) != n_lig:
        return none + (STATUS_DISCONNECTED,)
    edge_mask, rows = np.zeros(M, np.uint8), []
    for k in range(M // 2):
        u, v = int(bi[0, 2 * k]), int(bi[1, 2 * k])
        su = side(u, {u, v})
        if v in su:
            continue                      # a ring bond
        sv = set(range(n_lig)) - su
        # the smaller side; of two equal sides the one with the lowest atom index (atom 0: the graph is connected)
        l = su if (len(su) < len(sv) or (len(su) == len(sv) and 0 in su)) else sv
        if len(l) > 1:
            edge_mask[2 * k + 1 if u in l else 2 * k] = 1
            row = np.zeros(n_lig, np.uint8)
            row[sorted(l)] = 1
            rows.append(row)
    return edge_mask, np.asarray(rows, np.uint8).reshape(-1, n_lig), STATUS_OK


# ---- margins: a random input must not sit on a decision ------------------------------------------------------------------------------------------
REL = 1e-6


def knn_margins(pos, cutoff, max_neighbor, interior=False):
    """(no pair within REL relative of the cutoff, no two distances within REL relative of each other at a selected row's boundary: its m-th and
    (m + 1)-th nearest).  interior: nor anywhere among its first m + 1, for a comparison with a generator that orders them in another arithmetic"""
    pos = np.asarray(pos, np.float32)
    n, far, apart = len(pos), True, True
    for lo in range(0, n, 512):
        D = np.sqrt(d2_rows(pos, lo, min(lo + 512, n)))
        far &= bool((np.abs(D / float(np.float32(cutoff)) - 1.0) > REL).all())
        for r, d in enumerate(D):
            d = np.delete(d, lo + r)
            under = int((d < cutoff).sum())
            if under > max_neighbor or under == 0:
                m = max_neighbor if under else 1
                s = np.sort(d)[(0 if interior else m - 1):m + 1]
                apart &= bool((np.diff(s) > REL * s[1:]).all())
    return far, apart


def radius_margins(pos, r):
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    return all(bool((np.abs(np.sqrt(d2_rows(pos, lo, min(lo + 512, n))) / float(np.float32(r)) - 1.0) > REL).all()) for lo in range(0, n, 512))


# ---- point sets ----------------------------------------------------------------------------------------------------------------------------------
def lattice(side=5, spacing=3.0):
    """integer lattice, spacing 3: distance ties everywhere; (0,0,0)-(9,12,0) is exactly 15 apart and with spacing 1 (3,4,0) exactly 5"""
    g = np.arange(side) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


def dense_ball(n=1500, radius=7.0, seed=11):
    """n points inside a ball whose diameter is below the cutoff 15: every row selects max_neighbor of n - 1"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(size=(n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


def with_isolated_point(pos, where=7):
    """a copy with one more point 100 A away at index `where`: its row has no candidate and takes the single nearest point"""
    far = np.asarray(pos).max(0) + np.float32(100.0)
    return np.insert(np.asarray(pos, np.float32), where, far, axis=0)


def two_points(gap=40.0):
    return np.asarray([[0, 0, 0], [gap, 0, 0]], np.float32)


def coincident_cluster():
    """12 atoms at one place, max_num_neighbors = 4: atoms 0..4 find themselves among their first five in-radius points and keep 4 neighbours,
    atoms 5..11 do not and keep 5"""
    return np.full((12, 3), 1.5, np.float32)


def protein_atoms(n, seed):
    """n points at the heavy-atom density of a protein (about 17 A^3 per atom), at least 1.2 A apart, in random index order"""
    rng = np.random.default_rng(seed)
    side = (17.0 * n) ** (1.0 / 3.0)
    cell = 1.2
    pts, grid = [], {}
    while len(pts) < n:
        p = rng.uniform(0, side, size=3)
        k = tuple((p // cell).astype(int))
        near = [q for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) for q in grid.get((k[0] + dx, k[1] + dy, k[2] + dz), ())]
        if all(((pts[q] - p) ** 2).sum() >= cell * cell for q in near):
            grid.setdefault(k, []).append(len(pts))
            pts.append(p)
    return np.asarray(pts, np.float32)


def random_residues(n, seed):
    """n C-alpha-like points at protein density (135 A^3 per residue), at least 3.8 A apart: synthetic.make_receptor's point set without its graph"""
    rng = np.random.default_rng(seed)
    side = (135.0 * n) ** (1.0 / 3.0)
    cell = 3.8
    pts, grid = [], {}
    while len(pts) < n:
        p = rng.uniform(0, side, size=3)
        k = tuple((p // cell).astype(int))
        near = [q for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) for q in grid.get((k[0] + dx, k[1] + dy, k[2] + dz), ())]
        if all(((pts[q] - p) ** 2).sum() >= cell * cell for q in near):
            grid.setdefault(k, []).append(len(pts))
            pts.append(p)
    return np.asarray(pts, np.float32)


# name -> (pos, cutoff, max_neighbor) of ddk_receptor_knn_graph
def knn_cases():
    lat = lattice()
    return {
        'lattice_k24': (lat, 15.0, 24),                              # pairs exactly at 15 (9, 12, 0) are not candidates; ties inside every selection
        'lattice_k6': (lat, 15.0, 6),                                # the cap binds on six equidistant neighbours and on fewer at faces and corners
        'lattice_all_kept': (lattice(3), 4.0, 24),                   # <= 6 candidates per row: all kept in index order
        'dense_ball': (dense_ball(), 15.0, 24),                      # 24 of 1499: rows far above a wave's 64 lanes and above 1024 items
        'isolated': (with_isolated_point(lattice(3)), 15.0, 24),     # the fallback row
        'two_points': (two_points(), 15.0, 24),                      # n = 2, both rows fall back
        'two_points_close': (two_points(3.0), 15.0, 1),
        'coincident': (np.concatenate([coincident_cluster(), lattice(2)]), 15.0, 4),      # distance 0 between different indices: neighbours like any other
    }


# name -> (pos, r, max_num_neighbors) of ddk_radius_graph
def radius_cases():
    return {
        'lattice_r5': (lattice(5, 1.0), 5.0, 8),                     # (3, 4, 0) exactly at 5 is out; the cap binds everywhere
        'lattice_r5_wide': (lattice(5, 3.0), 5.0, 8),                # 18 points within 5 (3 and 3 sqrt 2 away): the cap binds on tied distances, index order decides
        'coincident': (coincident_cluster(), 5.0, 4),
        'one_point': (np.zeros((1, 3), np.float32), 5.0, 8),
        'cap_1024': (dense_ball(1100, 2.0, 5), 5.0, 1024),           # every centre sees 1100 points: quota 1025, rows across the 1024 boundary
        'atoms_300': (protein_atoms(300, 3), 5.0, 8),
    }


# ---- ligand graphs: name -> (n_lig, bond_index [2, M]) -------------------------------------------------------------------------------------------
def directed(pairs):
    bi = np.zeros((2, 2 * len(pairs)), np.int64)
    for k, (u, v) in enumerate(pairs):
        bi[:, 2 * k], bi[:, 2 * k + 1] = (u, v), (v, u)
    return bi


def path(n):
    return n, directed([(a, a + 1) for a in range(n - 1)])


def ring6():
    return 6, directed([(a, (a + 1) % 6) for a in range(6)])


def star(leaves=5):
    return leaves + 1, directed([(0, a) for a in range(1, leaves + 1)])


def two_rings_on_a_bridge(flip=False):
    """two six-rings joined by one bond: both sides have six atoms, the side with atom 0 is l.  flip: the bond is stored from the other ring"""
    pairs = [(a, (a + 1) % 6) for a in range(6)] + [(6 + a, 6 + (a + 1) % 6) for a in range(6)]
    return 12, directed(pairs + [(9, 3) if flip else (3, 9)])


def project_ligand(seed):
    from disco_diffdock_amd import synthetic
    lig = synthetic.make_ligand(np.random.default_rng(seed))
    return len(lig['lig_x']), lig['bond_index']


def ligand_cases():
    cases = {'path2': path(2), 'path3': path(3), 'path4': path(4), 'path256': path(256), 'ring6': ring6(), 'star': star(),
             'bridge': two_rings_on_a_bridge(), 'bridge_flipped': two_rings_on_a_bridge(True), 'one_atom': (1, np.zeros((2, 0), np.int64)),
             'path4_reversed': (4, directed([(3, 2), (2, 1), (1, 0)]))}
    for seed in range(8):
        cases[f'make_ligand_{seed}'] = project_ligand(seed)
    return cases


def broken_ligands():
    """name -> (n_lig, bond_index, status)"""
    n, good = path(6)
    out = {}
    for name, (col, row, val) in {'index_high': (2, 0, 6), 'index_negative': (5, 1, -1), 'unpaired': (3, 0, 5), 'self_bond': (4, 1, 2)}.items():
        b = good.copy()
        b[row, col] = val
        if name == 'self_bond':
            b[:, 4], b[:, 5] = (2, 2), (2, 2)
        out[name] = (n, b, STATUS_BAD_INPUT)
    out['repeated'] = (n, np.concatenate([good, good[:, 2:4]], axis=1), STATUS_BAD_INPUT)
    out['repeated_reversed'] = (n, np.concatenate([good, good[:, [3, 2]]], axis=1), STATUS_BAD_INPUT)
    out['counter_ion'] = (7, good, STATUS_DISCONNECTED)                                   # atom 6 has no bond
    out['two_fragments'] = (8, directed([(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)]), STATUS_DISCONNECTED)
    return out


def with_nan(pos, where=3):
    p = np.array(pos, np.float32)
    p[where, 1] = np.nan
    return p


def with_inf(pos, where=0):
    p = np.array(pos, np.float32)
    p[where, 2] = np.inf
    return p
