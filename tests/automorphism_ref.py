"""The specification of ddk_ligand_automorphisms (include/ddk.h, csrc/k_autos.hip) in plain Python, and the graphs its tests run on.

A graph is (colour [n] int, bonds [2, E] int, mask [n] bool or None).  The kept atoms (mask != 0, None: all) and the bonds between two distinct kept atoms
form G; an automorphism is a bijection p of the kept atoms with colour[p(a)] == colour[a] and {a, b} in E <=> {p(a), p(b)} in E.  A table row holds p(a) at
a kept atom a and a itself at a masked-out one.

    automorphisms_ref   depth-first backtracking over the matching order, no parallelism: the table [K, n] int32, row 0 the identity
    peak_frontier       the same search level by level: the largest number of partial maps any level holds (the `cap` the device call needs)
Both use the four rules of the device search and nothing else: a candidate is unused, has the atom's colour and degree, and is adjacent to the image of u
exactly when the atom is adjacent to u, for every mapped u.  tests/test_automorphism_host.py checks both against networkx and against each other."""
import functools

import numpy as np


def _graph(colour, bonds, mask):
    colour = np.asarray(colour).reshape(-1)
    n = len(colour)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    adj = np.zeros((n, n), bool)
    if bonds is not None:
        for a, b in np.asarray(bonds).reshape(2, -1).T:
            if not (0 <= a < n and 0 <= b < n):
                raise ValueError('bond index outside the ligand')
            if a != b and keep[a] and keep[b]:
                adj[a, b] = adj[b, a] = True
    return colour, keep, adj


def matching_order(keep, adj):
    """breadth-first from the lowest unvisited kept atom, component by component, neighbours ascending -> (order, parent position or -1)"""
    n = len(keep)
    seen, order, parent = np.zeros(n, bool), [], []
    for r in range(n):
        if not keep[r] or seen[r]:
            continue
        seen[r] = True
        head = len(order)
        order.append(r)
        parent.append(-1)
        while head < len(order):
            for q in np.flatnonzero(adj[order[head]]):
                if not seen[q]:
                    seen[q] = True
                    order.append(int(q))
                    parent.append(head)
            head += 1
    return order, parent


def _candidates(d, image, order, parent, keep, adj):
    return np.flatnonzero(keep) if parent[d] < 0 else np.flatnonzero(adj[image[parent[d]]])


def _survives(c, d, image, order, colour, deg, adj):
    v = order[d]
    if c in image[:d] or colour[c] != colour[v] or deg[c] != deg[v]:
        return False
    return all(adj[order[u], v] == adj[image[u], c] for u in range(d))


def automorphisms_ref(colour, bonds, mask=None):
    colour, keep, adj = _graph(colour, bonds, mask)
    n, deg = len(colour), adj.sum(1)
    order, parent = matching_order(keep, adj)
    m, rows, image = len(order), [], []

    def extend(d):
        if d == m:
            row = np.arange(n, dtype=np.int32)
            row[order] = image
            rows.append(row)
            return
        for c in _candidates(d, image, order, parent, keep, adj):
            if _survives(int(c), d, image, order, colour, deg, adj):
                image.append(int(c))
                extend(d + 1)
                image.pop()

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, m + 200))
    try:
        extend(0)
    finally:
        sys.setrecursionlimit(old)
    return np.stack(rows)


def peak_frontier(colour, bonds, mask=None):
    """(largest frontier over the levels 0 .. m, the last level's size = K)"""
    colour, keep, adj = _graph(colour, bonds, mask)
    deg = adj.sum(1)
    order, parent = matching_order(keep, adj)
    frontier, peak = [[]], 1
    for d in range(len(order)):
        frontier = [image + [int(c)] for image in frontier for c in _candidates(d, image, order, parent, keep, adj)
                    if _survives(int(c), d, image, order, colour, deg, adj)]
        peak = max(peak, len(frontier))
    return peak, len(frontier)


def sort_rows(table):
    """the rows in lexicographic order: tables are compared as sets"""
    table = np.asarray(table)
    return table[np.lexsort(table.T[::-1])]


def same_set(a, b):
    a, b = sort_rows(a), sort_rows(b)
    return a.shape == b.shape and np.array_equal(a, b)


def conjugate(table, relabel):
    """the table of the graph whose atom relabel[a] is this graph's atom a: row' [relabel[a]] = relabel[row[a]]"""
    table, relabel = np.asarray(table), np.asarray(relabel)
    out = np.empty_like(table)
    out[:, relabel] = relabel[table]
    return out


def relabelled(colour, bonds, mask, relabel):
    relabel = np.asarray(relabel)
    c2 = np.empty_like(np.asarray(colour))
    c2[relabel] = colour
    m2 = None
    if mask is not None:
        m2 = np.empty(len(relabel), bool)
        m2[relabel] = np.asarray(mask) != 0
    return c2, relabel[np.asarray(bonds)].astype(np.int32), m2


# ---- the graphs: name -> (colour, bonds [2, E] one direction each, K) --------------------------------------------------------------------------------------
def _g(colour, pairs):
    return np.asarray(colour, np.int32), np.asarray(pairs, np.int32).reshape(-1, 2).T.copy()


def _ring(k, first=0):
    return [(first + i, first + (i + 1) % k) for i in range(k)]


def cf3_chain(k):
    """N - (C(-CF3))_k - O: 5 k + 2 atoms, every CF3 turns by itself, K = 6^k"""
    colour, pairs, prev = [1], [], 0            # colours: N 1, C 2, O 3, F 4
    for _ in range(k):
        c = len(colour)
        colour += [2, 2, 4, 4, 4]
        pairs += [(prev, c), (c, c + 1), (c + 1, c + 2), (c + 1, c + 3), (c + 1, c + 4)]
        prev = c
    colour.append(3)
    pairs.append((prev, len(colour) - 1))
    return _g(colour, pairs)


def hexagon_with_hydrogens(odd=False):
    """a one-colour hexagon (atoms 0-5) with a hydrogen (colour 0) on every atom (6-11); odd: atom 8 is of another colour instead"""
    colour = [2] * 6 + [0] * 6
    if odd:
        colour[8] = 5
    return _g(colour, _ring(6) + [(i, 6 + i) for i in range(6)])


GRAPHS = {
    'one_atom': lambda: _g([3], []) + (1,),
    'toluene': lambda: _g([2] * 7, _ring(6) + [(0, 6)]) + (2,),
    'hexagon': lambda: _g([2] * 6, _ring(6)) + (12,),
    'star': lambda: _g([1, 2, 2, 2, 2], [(0, i) for i in range(1, 5)]) + (24,),
    'no_bonds': lambda: _g([2] * 5, []) + (120,),
    'cubane': lambda: _g([2] * 8, [(a, a ^ b) for a in range(8) for b in (1, 2, 4) if a < a ^ b]) + (48,),
    'c6_c3_c3': lambda: _g([2] * 12, _ring(6) + _ring(3, 6) + _ring(3, 9)) + (864,),
    'cf3_x4': lambda: cf3_chain(4) + (1296,),
    'cf3_x5': lambda: cf3_chain(5) + (7776,),
    'path256': lambda: _g([2] * 256, [(i, i + 1) for i in range(255)]) + (2,),
}
ATOMS = {'one_atom': 1, 'toluene': 7, 'hexagon': 6, 'star': 5, 'no_bonds': 5, 'cubane': 8, 'c6_c3_c3': 12, 'cf3_x4': 22, 'cf3_x5': 27, 'path256': 256}


@functools.lru_cache(maxsize=None)
def graph_and_table(name):
    """(colour, bonds, K, the reference table) of a named graph, computed once per process; treat the arrays as read-only"""
    colour, bonds, K = GRAPHS[name]()
    table = automorphisms_ref(colour, bonds)
    for a in (colour, bonds, table):
        a.setflags(write=False)
    return colour, bonds, K, table
