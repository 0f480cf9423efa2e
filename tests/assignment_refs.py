"""References, case tables and fixtures for the device assignment solver (csrc/fvit_assign.hip).

``exact`` restates the kernel's algorithm in numpy fp64: shortest augmenting paths with dual variables over the short side of the block, ties to the lowest
path cost, then an unassigned column, then the lowest index.  fp32 costs are exact in fp64, so on a case with ONE optimum ``exact``, the kernel and scipy
must agree index for index as soon as the optimum is separated from the runner-up by more than fp64 rounding: ``margin`` measures that separation, and the
unique-optimum cases are drawn so that it is at least ``MIN_MARGIN`` = 1e-6, six orders above the rounding error of sums of a few hundred fp64 terms of
size ~10.  On the tie cases only the total is defined, and it is compared exactly: integer costs add without error.

The fixtures (tests/golden/assignment_cases.npz, written by tests/golden/make_assignment_golden.py) hold scipy's indices, totals and margins and a
checksum of every cost matrix; the matrices themselves are drawn again from their seeds.  The keyword switches of ``exact`` (``greedy``, ``no_dual``,
``swap_output``, ``unsorted``) produce the wrong answers tests/test_assignment_refs_cpu.py shows to fail.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assignment_cases.npz")
MIN_MARGIN = 1e-6
FORBID = 1.0e6      # added to a cost to forbid its pair: far above any cost here, far below where fp64 would lose the 1e-6

# (Q, n_b) of the unique-optimum cases, one image each; "dup" is the near-duplicate 900 x 20
UNIQUE_CASES = [(1, 1), (1, 3), (3, 1), (7, 5), (5, 7), (63, 64), (64, 64), (65, 3), (257, 20), (300, 257), (900, 20), (900, 100)]
DUP_CASE = (900, 20)
# batches: name -> (Q, targets per image); their T is the sum, wider than any image's block
BATCH_CASES = {"hole": (7, [3, 0, 5]), "none": (7, [0, 0]), "mixed": (33, [4, 9, 2])}
# ties: name -> (Q, n_b)
TIE_CASES = {"int33": (33, 33), "int40x17": (40, 17), "equal65x8": (65, 8)}


def case_names():
    return [f"u{q}x{n}" for q, n in UNIQUE_CASES] + ["dup"] + list(BATCH_CASES) + list(TIE_CASES)


def _seed(name):
    return 7700 + case_names().index(name)


def draw(name):
    """(cost fp32 (B, Q, T), sizes) of a case, drawn from its seed."""
    g = np.random.default_rng(_seed(name))
    if name == "dup":
        Q, n = DUP_CASE
        base = g.standard_normal((30, n)) * 2
        cost = base[g.integers(0, 30, Q)] + 1e-3 * g.standard_normal((Q, n))
        return cost.astype(np.float32)[None], [n]
    if name in BATCH_CASES:
        Q, sizes = BATCH_CASES[name]
        return (g.standard_normal((len(sizes), Q, sum(sizes))) * 2).astype(np.float32), list(sizes)
    if name in TIE_CASES:
        Q, n = TIE_CASES[name]
        cost = np.full((Q, n), 3.0) if name.startswith("equal") else g.integers(0, 10, (Q, n)).astype(np.float64)
        return cost.astype(np.float32)[None], [n]
    Q, n = UNIQUE_CASES[[f"u{q}x{m}" for q, m in UNIQUE_CASES].index(name)]
    return (g.standard_normal((1, Q, n)) * 2).astype(np.float32), [n]


def blocks(cost, sizes):
    """The (Q, n_b) block of every image."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return [cost[b][:, off[b]:off[b + 1]] for b in range(len(sizes))]


def checksum(cost):
    return float(np.asarray(cost, dtype=np.float64).sum()) + float(np.abs(np.asarray(cost, dtype=np.float64)).sum())


def load_golden():
    return dict(np.load(GOLDEN).items())


# --------------------------------------------------------------------------------------------------------------------------------------- the solver
def exact(cost, greedy=False, no_dual=False, swap_output=False, unsorted=False):
    """(src, tgt) int64 of one (Q, n) block: min(Q, n) pairs, src ascending -- what linear_sum_assignment returns as (row_ind, col_ind)."""
    c = np.asarray(cost, dtype=np.float64)
    Q, n = c.shape
    if min(Q, n) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if greedy:                                       # every query's cheapest target, the k cheapest queries: no assignment problem is solved
        q = np.argsort(c.min(1), kind="stable")[:min(Q, n)]
        q.sort()
        return q.astype(np.int64), c[q].argmin(1).astype(np.int64)
    q_long = n < Q
    w = c.T if q_long else c                         # rows: the short side
    nr, nc = w.shape
    u, v = np.zeros(nr), np.zeros(nc)
    row4col, col4row = np.full(nc, -1), np.full(nr, -1)
    cols = np.arange(nc)
    for cur in range(nr):
        shortest, path, visited = np.full(nc, np.inf), np.full(nc, -1), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        for _ in range(nr + 1):
            r = min_val + w[i] - u[i] - v
            better = ~visited & (r < shortest)
            shortest[better], path[better] = r[better], i
            low = np.where(visited, np.inf, shortest).min()
            assert low < np.inf
            tied = cols[~visited & (shortest == low)]
            free = tied[row4col[tied] < 0]
            j = int(free[0] if free.size else tied[0])
            min_val, visited[j] = low, True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        assert sink >= 0, "the column visits ran into their bound"
        if not no_dual:
            d = min_val - shortest[visited]
            v[visited] -= d
            behind = row4col[visited]
            u[behind[behind >= 0]] += d[behind >= 0]
            u[cur] += min_val
        j = sink
        while True:
            r = path[j]
            row4col[j] = r
            col4row[r], j = j, col4row[r]
            if r == cur:
                break
    if q_long:
        src = cols[row4col >= 0]
        tgt = row4col[src]
    else:
        src, tgt = np.arange(nr), col4row.copy()
    if unsorted:
        src, tgt = src[::-1].copy(), tgt[::-1].copy()
    if swap_output:
        src, tgt = tgt, src
    return src.astype(np.int64), tgt.astype(np.int64)


def total(cost, src, tgt):
    """The assignment's cost, summed in fp64."""
    return float(np.asarray(cost, dtype=np.float64)[np.asarray(src, dtype=np.int64), np.asarray(tgt, dtype=np.int64)].sum())


def is_assignment(src, tgt, Q, n):
    src, tgt = np.asarray(src), np.asarray(tgt)
    k = min(Q, n)
    if src.shape != (k,) or tgt.shape != (k,):
        return False
    if k == 0:
        return True
    return bool((np.diff(src) > 0).all() and src[0] >= 0 and src[-1] < Q and np.unique(tgt).size == k and tgt.min() >= 0 and tgt.max() < n)


def margin(cost, solve=None):
    """The smallest increase of the optimum when one of its pairs is forbidden, found by solving again (inf for a block with a single cell a side)."""
    if solve is None:
        from scipy.optimize import linear_sum_assignment as solve
    c = np.asarray(cost, dtype=np.float64)
    src, tgt = solve(c)
    best, out = total(c, src, tgt), np.inf
    for i, j in zip(src, tgt):
        if c.shape[0] == 1 and c.shape[1] == 1:
            break
        d = c.copy()
        d[i, j] += FORBID
        out = min(out, total(d, *solve(d)) - best)
    return out
