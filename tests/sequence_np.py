"""The definitions of pr_disagg_radar_gan_amd/sequence.py restated in numpy, as plainly as they read: edge
features, seam masks and costs (a double loop), the min-plus recurrence with its tie rules, the greedy matching as the sorted walk
over all pairs -- and, beside it, the rounds of locally dominant pairs the device runs, which must give the same matching -- and the
series order.  Test infrastructure only."""
import numpy as np

UNIT = 32
FEATMAX = 65535
MAX_DEPTH = 2048
MAX_MEMBERS = 4096


def edge_features(hourly, first_hour=0, last_hour=23):
    """hourly (S, D, 24, ny, nx) -> (features (S, D, 2, P) uint16, bad (D, 2, P) bool): edge 0 is first_hour, edge 1 last_hour"""
    x = np.asarray(hourly, dtype=np.float32)
    S, D = x.shape[:2]
    e = x[:, :, [first_hour, last_hour]].reshape(S, D, 2, -1)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(e) & (e >= 0) & (e < np.float32(MAX_DEPTH))
        q = np.rint(np.where(good, e, np.float32(0)) * np.float32(UNIT))            # the fp32 product, rint to even
    feat = np.minimum(q, FEATMAX).astype(np.uint16)
    return feat, (~good).any(axis=0)


def seam_costs(feat_a, bad_a, shift=1, feat_b=None, bad_b=None):
    """-> (costs (B, S_a, S_b) int64, n_valid (B,) int64): boundary b joins edge 1 of day b (rows) to edge 0 of day b + shift"""
    if feat_b is None:
        feat_b, bad_b = feat_a, bad_a
    Sa, D, Sb = feat_a.shape[0], feat_a.shape[1], feat_b.shape[0]
    B = D - shift
    costs, n_valid = np.zeros((B, Sa, Sb), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        keep = ~(bad_a[b, 1] | bad_b[b + shift, 0])
        n_valid[b] = keep.sum()
        for i in range(Sa):
            for j in range(Sb):
                d = np.abs(feat_a[i, b, 1].astype(np.int64) - feat_b[j, b + shift, 0].astype(np.int64))
                costs[b, i, j] = d[keep].sum()
    return costs, n_valid


def min_plus(costs):
    """costs (B, S, S) -> (acc (B + 1, S), back (B, S)): the smallest i among equals"""
    costs = np.asarray(costs, dtype=np.int64)
    B, S = costs.shape[:2]
    acc, back = np.zeros((B + 1, S), np.int64), np.zeros((B, S), np.int32)
    for b in range(B):
        for j in range(S):
            v = acc[b] + costs[b, :, j]
            back[b, j] = int(np.argmin(v))                                          # (the first of equals)
            acc[b + 1, j] = v[back[b, j]]
    return acc, back


def best_path(costs):
    """-> (path (B + 1,) ints, total): the end member is the smallest j among equals"""
    acc, back = min_plus(costs)
    B = back.shape[0]
    path = [int(np.argmin(acc[B]))]
    for b in range(B - 1, -1, -1):
        path.append(int(back[b, path[-1]]))
    return np.array(path[::-1], dtype=np.int64), int(acc[B].min())


def keys(C):
    C = np.asarray(C, dtype=np.int64)
    S = C.shape[0]
    assert C.shape == (S, S) and S <= MAX_MEMBERS and C.min() >= 0 and C.max() < 1 << 40
    i, j = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(S, dtype=np.uint64), indexing="ij")
    return (C.astype(np.uint64) << np.uint64(24)) | (i << np.uint64(12)) | j                # 64 bits, unsigned: C < 2^40


def greedy_sorted(C):
    """the definition: all S^2 pairs by ascending key, a pair taken when neither its row nor its column is taken"""
    k = keys(C)
    S = k.shape[0]
    perm, col_taken = np.full(S, -1, np.int32), np.zeros(S, bool)
    for key in np.sort(k.ravel()):
        i, j = (int(key) >> 12) & 0xFFF, int(key) & 0xFFF
        if perm[i] < 0 and not col_taken[j]:
            perm[i], col_taken[j] = j, True
    return perm


def greedy_rounds(C, max_rounds=None):
    """the device's form: per round every free pair whose key is the minimum of its row over the free columns and of its column over
    the free rows is taken.  -> (perm, rounds used)"""
    k = keys(C)
    S = k.shape[0]
    perm, row_free, col_free = np.full(S, -1, np.int32), np.ones(S, bool), np.ones(S, bool)
    rounds = 0
    big = np.uint64(np.iinfo(np.uint64).max)
    while row_free.any():
        assert rounds < (S if max_rounds is None else max_rounds), "a round takes at least the smallest free pair"
        free = np.where(row_free[:, None] & col_free[None, :], k, big)
        rowmin, colmin = free.min(axis=1), free.min(axis=0)
        took = 0
        for i in np.flatnonzero(row_free):
            j = int(rowmin[i]) & 0xFFF
            if colmin[j] == rowmin[i]:
                perm[i], row_free[i], col_free[j] = j, False, False
                took += 1
        assert took >= 1
        rounds += 1
    return perm, rounds


def greedy_matching(costs):
    """costs (B, S, S) -> perm (B, S) int32; the two forms are asserted equal, as the contract demands"""
    out = []
    for C in np.asarray(costs, dtype=np.int64):
        a, (b, _) = greedy_sorted(C), greedy_rounds(C)
        assert np.array_equal(a, b)
        out.append(a)
    return np.stack(out)


def series_order(perm):
    """perm (B, S) -> order (B + 1, S): order[0][s] = s, order[d + 1][s] = perm[d][order[d][s]]"""
    perm = np.asarray(perm)
    B, S = perm.shape
    order = np.zeros((B + 1, S), np.int64)
    order[0] = np.arange(S)
    for d in range(B):
        order[d + 1] = perm[d][order[d]]
    return order


def reorder(x, order):
    """x (S, D, ...) -> the series: out[s, d] = x[order[d][s], d]"""
    x = np.asarray(x)
    return np.stack([x[order[d], d] for d in range(x.shape[1])], axis=1)
