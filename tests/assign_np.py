"""The definition of the least-cost assignment restated in numpy int64: what csrc/rdgan_assign.hip.h must equal
bit for bit in perm, u and v.  Shortest augmenting paths with dual potentials (the Hungarian method in Jonker-Volgenant form): rows
inserted in the order 0 .. S - 1 from u = v = 0, each by a Dijkstra search over the columns from a virtual column S; the next column
is the unused one of the smallest (minv[j], j) -- value first, then the smaller index.  There is no initialisation pass."""
import itertools

import numpy as np

MAX_COST = 1 << 40
INF = 1 << 62


def assign(C):
    """C (S, S) int64 with 0 <= C < 2^40 -> (perm (S,) int32, u (S,) int64, v (S,) int64, search steps)"""
    C = np.asarray(C, dtype=np.int64)
    S = C.shape[0]
    assert C.shape == (S, S) and S >= 1
    u, v = np.zeros(S, np.int64), np.zeros(S, np.int64)
    p = np.full(S + 1, -1, np.int64)                                                      # column -> row; p[S]: the row being inserted
    way = np.zeros(S, np.int64)
    steps = 0
    for r in range(S):
        minv = np.full(S, INF, np.int64)
        used = np.zeros(S, bool)
        p[S] = r
        j0 = S
        for _ in range(r + 1):                                                            # r columns are matched: a free one is met by then
            i0 = p[j0]
            free = ~used
            cur = C[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            j1 = int(np.argmin(np.where(free, minv, INF)))                                # the first of equals: the smaller index
            delta = minv[j1]
            assert 0 <= delta < S * MAX_COST and free[j1]
            u[p[:S][used]] += delta
            u[r] += delta                                                                 # the virtual column
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            used[j0] = True
            steps += 1
            if p[j0] < 0:
                break
        assert p[j0] < 0
        for _ in range(S):
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == S:
                break
        assert j0 == S
    perm = np.empty(S, np.int32)
    perm[p[:S]] = np.arange(S)
    return perm, u, v, steps


def optimal_matching(costs):
    """costs (B, S, S) -> (perm (B, S) int32, total (B,), u (B, S), v (B, S) int64, steps (B,))"""
    costs = np.asarray(costs, dtype=np.int64)
    out = [assign(C) for C in costs]
    perm = np.stack([o[0] for o in out])
    total = np.array([int(C[np.arange(len(q)), q].sum()) for C, q in zip(costs, perm)], np.int64)
    return perm, total, np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), np.array([o[3] for o in out], np.int64)


def check_certificate(C, perm, u, v):
    """asserts that perm is a permutation, that the duals are feasible on all pairs and tight on the matched ones, and that they sum
    to the total: together a proof that perm is optimal, with no reference.  -> total"""
    C, perm = np.asarray(C, dtype=np.int64), np.asarray(perm).astype(np.int64)
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    S = C.shape[0]
    assert C.shape == (S, S) and perm.shape == u.shape == v.shape == (S,)
    assert sorted(perm.tolist()) == list(range(S)), "perm is not a permutation"
    slack = C - u[:, None] - v[None, :]
    assert slack.min() >= 0, f"duals infeasible: least slack {slack.min()}"
    assert not slack[np.arange(S), perm].any(), "duals not tight on the matched pairs"
    total = int(C[np.arange(S), perm].sum())
    assert int(u.sum()) + int(v.sum()) == total
    return total


def brute_force(C):
    """the least total over all S! permutations"""
    C = np.asarray(C, dtype=np.int64)
    S = C.shape[0]
    perms = np.array(list(itertools.permutations(range(S))))
    return int(C[np.arange(S)[None, :], perms].sum(axis=1).min())
