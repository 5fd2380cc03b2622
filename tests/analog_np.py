"""The yardstick of the analog tests: the definitions of DESIGN.md section 22 restated in numpy by brute force -- features, keys,
the k nearest days (a sort of all keys, and a running top-k as a second form), the picks with the counter RNG's words on stream
9, and the apply step in fp64.  No code is shared with the module, and the reference project has no analog method, so this file
is the definition.  tests/test_analog_host.py checks the two forms against each other and against answers worked out by hand."""
import numpy as np

from oracle import rng as orng
from tests.hourly_np import quantise

NHOURS = 24
STREAM_ANALOG = 9
NONE = np.int64(1) << np.int64(62)                                           # above every key


def isqrt(D):
    """floor(sqrt(D)) of non-negative int64, exact: a floating estimate corrected by comparing squares"""
    D = np.asarray(D, dtype=np.int64)
    r = np.floor(np.sqrt(D.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > D, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= D, r + 1, r)
    assert np.all(r * r <= D) and np.all((r + 1) * (r + 1) > D)
    return r


def library_features(lib):
    """lib (N, 24, ny, nx) -> (e (N, P) int64, void (N,) bool, total (N,) int64)"""
    lib = np.asarray(lib, dtype=np.float32)
    N = lib.shape[0]
    q, bad = quantise(lib.reshape(N, NHOURS, -1), 2048)
    D = q.sum(axis=1)
    total = D.sum(axis=1)
    return isqrt(D), bad.any(axis=(1, 2)) | (total == 0), total


def query_features(cond):
    """cond (Q, ny, nx) -> (e (Q, P) int64, masked (Q, P) bool)"""
    cond = np.asarray(cond, dtype=np.float32)
    q, masked = quantise(cond.reshape(cond.shape[0], -1), 2048 * NHOURS)
    return isqrt(q), masked


def all_keys(lib, cond, lib_groups=None, query_groups=None):
    """(Q, N) int64: dist 2^24 + j, NONE for a day that is void or of the query's group"""
    e, void, _ = library_features(lib)
    eq, masked = query_features(cond)
    Q, N = eq.shape[0], e.shape[0]
    keys = np.empty((Q, N), np.int64)
    for i in range(Q):
        d = np.where(masked[i][None, :], 0, eq[i][None, :] - e)
        keys[i] = (d * d).sum(axis=1) * (1 << 24) + np.arange(N)
        keys[i][void] = NONE
        if lib_groups is not None and query_groups is not None and query_groups[i] >= 0:
            keys[i][np.asarray(lib_groups) == query_groups[i]] = NONE
    return keys


def _unpack(best, Q, k):
    nb = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), -1, np.int64)
    found = np.zeros(Q, np.int32)
    for i in range(Q):
        for r, key in enumerate(best[i]):
            nb[i, r], dist[i, r] = key & ((1 << 24) - 1), key >> 24
        found[i] = len(best[i])
    return nb, dist, found


def search(lib, cond, k, lib_groups=None, query_groups=None):
    """the sort of all keys -> (neighbours (Q, k) int32, distances (Q, k) int64, found (Q,) int32)"""
    keys = all_keys(lib, cond, lib_groups, query_groups)
    best = [[int(v) for v in np.sort(row) if v != NONE][:k] for row in keys]
    return _unpack(best, keys.shape[0], k)


def search_running(lib, cond, k, lib_groups=None, query_groups=None, order=None):
    """the same by a running list of the k smallest keys, the days met in `order` (default: as they lie)"""
    keys = all_keys(lib, cond, lib_groups, query_groups)
    Q, N = keys.shape
    best = []
    for i in range(Q):
        top = []
        for j in (range(N) if order is None else order):
            key = int(keys[i, j])
            if key == NONE or (len(top) == k and key > top[-1]):
                continue
            pos = 0
            while pos < len(top) and top[pos] < key:
                pos += 1
            top.insert(pos, key)
            del top[k:]
        best.append(top)
    return _unpack(best, Q, k)


def member_key(seed, member):
    """rd_member_key(rd_make_key(seed, 9), member) of csrc/rdgan_rng.h"""
    member = int(member)
    inner = orng.mix32(np.uint32(member >> 32) ^ np.uint32(0x9E3779B9))
    return orng.mix32(orng.make_key(seed, STREAM_ANALOG) ^ orng.mix32(np.uint32(member & 0xFFFFFFFF) ^ inner))


def pick_bits(seed, member, query):
    return int(orng.mix32(orng.mix32(np.uint32(query & 0xFFFFFFFF)) ^ member_key(seed, member)))


def rank_table(f):
    """c[r] = sum over s <= r of floor(2^20 / (s + 1)), r = 0 .. f - 1"""
    return np.cumsum([(1 << 20) // (s + 1) for s in range(f)])


def pick_rank(bits, f, weights):
    if weights == "uniform":
        return (bits * f) >> 32
    c = rank_table(f)
    target = (bits * int(c[-1])) >> 32
    return int(np.argmax(c > target))


def picks(neighbours, found, n_members, seed, weights="rank", first_member=0, first_query=0):
    """(Q, S) int32: the library index member first_member + m picks for query first_query + i, -1 without a neighbour"""
    Q = neighbours.shape[0]
    out = np.full((Q, n_members), -1, np.int32)
    for i in range(Q):
        for m in range(n_members):
            if found[i] > 0:
                out[i, m] = neighbours[i, pick_rank(pick_bits(seed, first_member + m, first_query + i), int(found[i]), weights)]
    return out


def apply(lib, cond, picked):
    """-> (out (Q, S, 24, ny, nx) float64, profile_path (Q, S, ny, nx) bool: where the donor's pixel is dry and its areal profile
    stands in).  NaN at masked pixels and for a pick of -1."""
    lib64 = np.asarray(lib, dtype=np.float32).astype(np.float64)
    cond32 = np.asarray(cond, dtype=np.float32)
    Q, S = picked.shape
    ny, nx = cond32.shape[1:]
    out = np.full((Q, S, NHOURS, ny, nx), np.nan)
    dry = np.zeros((Q, S, ny, nx), bool)
    with np.errstate(invalid="ignore"):
        masked = ~((cond32 >= 0) & (cond32 < 2048 * NHOURS))
    for i in range(Q):
        for m in range(S):
            j = picked[i, m]
            if j < 0:
                continue
            day = lib64[j]
            d = day.sum(axis=0)
            profile = day.sum(axis=(1, 2)) / day.sum()
            with np.errstate(invalid="ignore", divide="ignore"):
                frac = np.where(d > 0, day / d, profile[:, None, None])
            out[i, m] = np.where(masked[i], np.nan, cond32[i].astype(np.float64) * frac)
            dry[i, m] = (d == 0) & ~masked[i]
    return out, dry
