"""The yardstick of the cascade tests: the definitions of DESIGN.md section 24 restated in numpy -- the state a calibration counts,
the thresholds a model is built from (Python ints), and the generation with the counter RNG's words on stream 10.  No code is shared
with the module, and the reference project has no cascade, so this file is the definition.  The counting exists twice, over arrays
(accumulate) and pixel-day by pixel-day in plain Python (accumulate_scalar); tests/test_cascade_host.py checks the two against each
other and against counts written out by hand.

The tree of a pixel-day: node 0 is the day, split into thirds of 8 h; nodes 1 .. 3 the 8 h boxes (level 0), 4 .. 9 the 4 h boxes
(level 1), 10 .. 21 the 2 h boxes (level 2), each split into halves.  Node 22 names no box: it holds the draws of the second split of
a day whose three thirds are wet.

Flat state, NV = len(edges) + 1 volume classes, int64:
    type    [3 levels][4 positions][NV][3]        at 0         0/1 (first half dry), 1/0, x/(1-x)
    weight  [3 levels][4 positions][NV][32]       at 36 NV     bin (V1 * 32) // V of an x/(1-x) split
    pattern [NV][8]                               at 420 NV    wet mask of the thirds, bit t for third t
    w2      [NV][8][32]                           at 428 NV    two wet thirds: bin of the first wet one, by pattern (3, 5, 6)
    w3a     [NV][32]                              at 684 NV    three wet thirds: bin (V1 * 32) // V
    w3b     [NV][32]                              at 716 NV    three wet thirds: bin (V2 * 32) // (V - V1)
    n_days, n_bad, n_dry                          at 748 NV    pixel-days seen, left out for a bad hour, without rain
Positions: 0 isolated, 1 starting (previous dry, next wet), 2 enclosed, 3 ending.  The model table has the same layout without the
last three words and holds, per row, cumulative 24-bit thresholds."""
import numpy as np

from oracle import rng as orng
from tests.hourly_np import UNIT, levels_q, quantise

NHOURS = 24
NB = 32
NP = 4
NL = 3
NT = 3
MAX_EDGES = 7
PER_CLASS = 748
TAIL = 3
STREAM_CASCADE = 10
LEVEL_HOURS = (8, 4, 2)
LEVEL_NODE0 = (1, 4, 10)
NODE_DAY2 = 22
MAX_COND = 16384
ONE = 1 << 24
ISOLATED, STARTING, ENCLOSED, ENDING = range(4)


def offsets(NV):
    return {"type": 0, "weight": 36 * NV, "pattern": 420 * NV, "w2": 428 * NV, "w3a": 684 * NV, "w3b": 716 * NV, "tail": 748 * NV}


def state_size(n_edges):
    return PER_CLASS * (n_edges + 1) + TAIL


def edge_units(edges):
    """the integer thresholds per hour: rint(e * 1024), the product in fp64"""
    return levels_q(edges)


def vclass(V, eq, hours):
    """the number of edges e with V >= e * hours"""
    V = np.asarray(V, dtype=np.int64)
    c = np.zeros(V.shape, np.int64)
    for e in eq:
        c += V >= e * hours
    return c


def positions(wet):
    """wet (M, nb) bool -> (M, nb) position classes; a box beyond the day's ends is dry"""
    prev = np.zeros_like(wet)
    nxt = np.zeros_like(wet)
    prev[:, 1:] = wet[:, :-1]
    nxt[:, :-1] = wet[:, 1:]
    return np.where(prev, np.where(nxt, ENCLOSED, ENDING), np.where(nxt, STARTING, ISOLATED))


def accumulate(hourly, edges=(0.1, 1.0)):
    """hourly (..., 24, ny, nx) -> the flat state, int64"""
    eq = edge_units(edges)
    NV, off = len(eq) + 1, offsets(len(eq) + 1)
    x = np.asarray(hourly, dtype=np.float32)
    x = np.moveaxis(x.reshape((-1, NHOURS) + x.shape[-2:]), 1, -1).reshape(-1, NHOURS)        # pixel-days
    state = np.zeros(state_size(len(eq)), np.int64)
    q, bad = quantise(x, 2048)
    badday = bad.any(axis=1)
    q = q[~badday]
    D = q.sum(axis=1)
    state[off["tail"]:] = len(x), badday.sum(), (D == 0).sum()
    q, D = q[D > 0], D[D > 0]
    # the day
    v8 = q.reshape(-1, 3, 8).sum(axis=2)
    vc = vclass(D, eq, NHOURS)
    mask = (v8[:, 0] > 0) + 2 * (v8[:, 1] > 0) + 4 * (v8[:, 2] > 0)
    np.add.at(state, off["pattern"] + vc * 8 + mask, 1)
    for pat, first in ((3, 0), (5, 0), (6, 1)):
        s = mask == pat
        np.add.at(state, off["w2"] + (vc[s] * 8 + pat) * NB + (v8[s, first] * NB) // D[s], 1)
    s = mask == 7
    np.add.at(state, off["w3a"] + vc[s] * NB + (v8[s, 0] * NB) // D[s], 1)
    np.add.at(state, off["w3b"] + vc[s] * NB + (v8[s, 1] * NB) // (D[s] - v8[s, 0]), 1)
    # the binary levels
    for L, hours in enumerate(LEVEL_HOURS):
        nb = NHOURS // hours
        box = q.reshape(-1, nb, hours).sum(axis=2)
        V1 = q.reshape(-1, nb, 2, hours // 2).sum(axis=3)[:, :, 0]
        wet = box > 0
        row = (L * NP + positions(wet)) * NV + vclass(box, eq, hours)
        kind = np.where(V1 == 0, 0, np.where(V1 == box, 1, 2))
        np.add.at(state, off["type"] + row[wet] * NT + kind[wet], 1)
        s = wet & (kind == 2)
        np.add.at(state, off["weight"] + row[s] * NB + (V1[s] * NB) // box[s], 1)
    return state


def accumulate_scalar(hourly, edges=(0.1, 1.0)):
    """the same counts pixel-day by pixel-day in plain Python: the second form"""
    eq = edge_units(edges)
    NV, off = len(eq) + 1, offsets(len(eq) + 1)
    x = np.asarray(hourly, dtype=np.float32)
    x = np.moveaxis(x.reshape((-1, NHOURS) + x.shape[-2:]), 1, -1).reshape(-1, NHOURS)
    state = np.zeros(state_size(len(eq)), np.int64)
    vcl = lambda V, hours: sum(1 for e in eq if V >= e * hours)
    for day in x:
        state[off["tail"]] += 1
        if any(not (0 <= v < 2048) for v in day):                                       # (a NaN fails both)
            state[off["tail"] + 1] += 1
            continue
        q = [int(np.rint(np.float32(v) * np.float32(1024))) for v in day]
        D = sum(q)
        if D == 0:
            state[off["tail"] + 2] += 1
            continue
        third = [sum(q[8 * t:8 * t + 8]) for t in range(3)]
        vc = vcl(D, 24)
        mask = sum(1 << t for t in range(3) if third[t] > 0)
        state[off["pattern"] + vc * 8 + mask] += 1
        wet = [t for t in range(3) if third[t] > 0]
        if len(wet) == 2:
            state[off["w2"] + (vc * 8 + mask) * NB + third[wet[0]] * NB // D] += 1
        if len(wet) == 3:
            state[off["w3a"] + vc * NB + third[0] * NB // D] += 1
            state[off["w3b"] + vc * NB + third[1] * NB // (D - third[0])] += 1
        for L, hours in enumerate(LEVEL_HOURS):
            nb = NHOURS // hours
            box = [sum(q[hours * j:hours * (j + 1)]) for j in range(nb)]
            for j in range(nb):
                if box[j] == 0:
                    continue
                prev, nxt = j > 0 and box[j - 1] > 0, j + 1 < nb and box[j + 1] > 0
                pos = (ENCLOSED if nxt else ENDING) if prev else (STARTING if nxt else ISOLATED)
                row = (L * NP + pos) * NV + vcl(box[j], hours)
                V1 = sum(q[hours * j:hours * j + hours // 2])
                kind = 0 if V1 == 0 else (1 if V1 == box[j] else 2)
                state[off["type"] + row * NT + kind] += 1
                if kind == 2:
                    state[off["weight"] + row * NB + V1 * NB // box[j]] += 1
    return state


# ---------------------------------------------------------------------------------------------------------------------------------
# the model: exact integer arithmetic on Python ints
# ---------------------------------------------------------------------------------------------------------------------------------
def cumulative(counts):
    """c[j] = (cum[j] << 24) // total; the last one is 2^24"""
    total, cum, out = sum(counts), 0, []
    for c in counts:
        cum += c
        out.append((cum << 24) // total)
    return out


def one_hot(n, j):
    return [0] * j + [1] + [0] * (n - 1 - j)


def _first_nonempty(*rows):
    for r in rows:
        if sum(r) > 0:
            return r
    raise AssertionError("the fixed rule is never empty")


def _add(rows):
    return [sum(col) for col in zip(*rows)]


def build_model(state, n_edges):
    """-> (table (748 NV,) uint32, fallbacks: {(table name, row indices): 1, 2 or 3, the step of the chain an empty row took}).
    An empty row falls back to (1) the row pooled over the position classes, (2) pooled over the volume classes as well, (3) the
    fixed rule: x/(1-x) for a type row, bin 16 for a weight row, pattern 7 for the day.  The day's rows have no position class: step
    1 is step 2 there.  ValueError for a state without a wet pixel-day."""
    NV, off = n_edges + 1, offsets(n_edges + 1)
    s = [int(v) for v in np.asarray(state).ravel()]
    if len(s) != state_size(n_edges):
        raise ValueError(f"a state of {n_edges} edges has {state_size(n_edges)} words, got {len(s)}")
    if sum(s[off["pattern"]:off["w2"]]) == 0:
        raise ValueError("the state holds no wet pixel-day")
    table, fallbacks = [0] * (PER_CLASS * NV), {}

    def put(name, at, idx, chain):
        for step, r in enumerate(chain):
            if sum(r) > 0:
                if step:
                    fallbacks[(name, idx)] = step
                table[at:at + len(r)] = cumulative(r)
                return

    for name, width, fixed in (("type", NT, one_hot(NT, 2)), ("weight", NB, one_hot(NB, NB // 2))):
        row = lambda L, pos, v: s[off[name] + ((L * NP + pos) * NV + v) * width:off[name] + ((L * NP + pos) * NV + v + 1) * width]
        for L in range(NL):
            for pos in range(NP):
                for v in range(NV):
                    over_pos = _add([row(L, p, v) for p in range(NP)])
                    over_all = _add([row(L, p, w) for p in range(NP) for w in range(NV)])
                    put(name, off[name] + ((L * NP + pos) * NV + v) * width, (L, pos, v), (row(L, pos, v), over_pos, over_all, fixed))
    for name, width, rows_per_class, fixed in (("pattern", 8, 1, one_hot(8, 7)), ("w2", NB, 8, one_hot(NB, NB // 2)),
                                               ("w3a", NB, 1, one_hot(NB, NB // 2)), ("w3b", NB, 1, one_hot(NB, NB // 2))):
        row = lambda v, k: s[off[name] + (v * rows_per_class + k) * width:off[name] + (v * rows_per_class + k + 1) * width]
        for v in range(NV):
            for k in range(rows_per_class):
                over_all = _add([row(w, k) for w in range(NV)])
                put(name, off[name] + (v * rows_per_class + k) * width, (v, k), (row(v, k), over_all, over_all, fixed))
    return np.array(table, dtype=np.uint32), fallbacks


def probabilities(table, n_edges):
    """the thresholds as probabilities, float64, by table name"""
    NV, off = n_edges + 1, offsets(n_edges + 1)
    t = np.asarray(table, dtype=np.float64) / ONE
    cut = lambda name, end, shape: np.diff(t[off[name]:end].reshape(shape), axis=-1, prepend=0.0)
    return {"type": cut("type", off["weight"], (NL, NP, NV, NT)), "weight": cut("weight", off["pattern"], (NL, NP, NV, NB)),
            "pattern": cut("pattern", off["w2"], (NV, 8)), "w2": cut("w2", off["w3a"], (NV, 8, NB)),
            "w3a": cut("w3a", off["w3b"], (NV, NB)), "w3b": cut("w3b", off["tail"], (NV, NB))}


# ---------------------------------------------------------------------------------------------------------------------------------
# generation
# ---------------------------------------------------------------------------------------------------------------------------------
def member_key(seed, member, query):
    """rd_member_key(rd_member_key(rd_make_key(seed, 10), member), query) of csrc/rdgan_rng.h"""
    key = orng.make_key(seed, STREAM_CASCADE)
    for m in (int(member), int(query)):
        inner = orng.mix32(np.uint32(m >> 32) ^ np.uint32(0x9E3779B9))
        key = orng.mix32(key ^ orng.mix32(np.uint32(m & 0xFFFFFFFF) ^ inner))
    return np.uint32(key)


def pick(rows, r):
    """the first j with rows[:, j] > r"""
    return (rows > r[:, None]).argmax(axis=1)


def split(V, b, u, most):
    """clamp((V * ((b << 24) + u)) >> 29, 1, most): V < 2^24, the product below 2^53"""
    return np.clip((V * ((b << 24) + u)) >> 29, 1, most)


def generate(table, edges, cond, n_members, seed=0, first_member=0, first_query=0, patch=1):
    """cond (Q, ny, nx) daily sums in mm -> (out (Q, S, 24, ny, nx) float32, units (Q, S, 24, ny, nx) int32): units in 1 / 1024 mm,
    out = units * 2^-10; NaN and -1 at a masked pixel (NaN, +-inf, negative or >= 16384 mm).

    Rules beyond the tables.  A draw is bits(key, (block * 32 + node) * 4 + draw) >> 8 with block = (y // patch) * ceil(nx / patch)
    + x // patch; draw 0 picks the type or pattern, draw 1 the weight bin, draw 2 the 24 bits u inside the bin.  The day: the pattern
    from pattern[vclass]; while it has more wet thirds than V has units, its highest wet third is dropped.  Two wet thirds: the first
    gets split(V, b, u, V - 1) with b from w2[vclass][pattern].  Three: V1 = split(V, b1, u1, V - 2) with b1 from w3a, and of the rest R
    = V - V1, V2 = split(R, b2, u2, R - 1) with b2 from w3b and the draws 1 and 2 of node 22.  A binary node of V >= 2: the type from
    type[level][pos][vclass]; x/(1-x) gives the first half split(V, b, u, V - 1).  A binary node of V = 1 cannot split x/(1-x): with
    (c0, c1, 2^24) its type thresholds and r the draw, it is 0/1 where (r * c1) >> 24 < c0 and 1/0 otherwise -- the two other types
    in their own proportion -- and where c1 = 0, 0/1 for r < 2^23."""
    table = np.asarray(table, dtype=np.int64)
    eq = edge_units(edges)
    NV, off = len(eq) + 1, offsets(len(eq) + 1)
    cond = np.asarray(cond, dtype=np.float32)
    Q, ny, nx = cond.shape
    S, plane = int(n_members), ny * nx
    V0, masked = quantise(cond.reshape(Q, plane), MAX_COND)
    nbx = -(-nx // patch)
    p = np.arange(plane)
    block = ((p // nx) // patch) * nbx + (p % nx) // patch
    keys = np.array([[member_key(seed, first_member + m, first_query + i) for m in range(S)] for i in range(Q)], dtype=np.uint32)
    N = Q * S * plane
    key = np.broadcast_to(keys[:, :, None], (Q, S, plane)).reshape(N)
    blk = np.broadcast_to(block[None, None, :], (Q, S, plane)).reshape(N).astype(np.int64)
    V = np.broadcast_to(V0[:, None, :], (Q, S, plane)).reshape(N).copy()

    def draw(node, d):
        idx = (((blk * 32 + node) * 4 + d) & 0xFFFFFFFF).astype(np.uint32)
        return (orng.mix32(orng.mix32(idx) ^ key) >> np.uint32(8)).astype(np.int64)

    rows = lambda name, width, row: table[off[name] + row[:, None] * width + np.arange(width)[None, :]]
    # the day
    vc = vclass(V, eq, NHOURS)
    pat = pick(rows("pattern", 8, vc), draw(0, 0))
    pat = np.where(V == 1, pat & -pat, np.where((V == 2) & (pat == 7), 3, pat))
    pat = np.where(V == 0, 0, pat)
    nwet = (pat & 1) + ((pat >> 1) & 1) + ((pat >> 2) & 1)
    b2w = pick(rows("w2", NB, vc * 8 + pat), draw(0, 1))
    b3a = pick(rows("w3a", NB, vc), draw(0, 1))
    u = draw(0, 2)
    first2 = split(V, b2w, u, np.maximum(V - 1, 1))
    V1 = split(V, b3a, u, np.maximum(V - 2, 1))
    R = V - V1
    V2 = split(R, pick(rows("w3b", NB, vc), draw(NODE_DAY2, 1)), draw(NODE_DAY2, 2), np.maximum(R - 1, 1))
    third = np.zeros((N, 3), np.int64)
    for t in range(3):
        third[:, t] = np.where((nwet == 1) & (pat == 1 << t), V, third[:, t])
    for p2, (a, b) in ((3, (0, 1)), (5, (0, 2)), (6, (1, 2))):
        s = pat == p2
        third[s, a], third[s, b] = first2[s], V[s] - first2[s]
    s = pat == 7
    third[s, 0], third[s, 1], third[s, 2] = V1[s], V2[s], R[s] - V2[s]
    assert np.array_equal(third.sum(axis=1), V)
    # the binary levels
    box = third
    for L, hours in enumerate(LEVEL_HOURS):
        nb = NHOURS // hours
        wet = box > 0
        row = (L * NP + positions(wet)) * NV + vclass(box, eq, hours)
        half = np.zeros((N, 2 * nb), np.int64)
        for j in range(nb):
            node, Vj = LEVEL_NODE0[L] + j, box[:, j]
            thr = rows("type", NT, row[:, j])
            r = draw(node, 0)
            kind = pick(thr, r)
            c0, c1 = thr[:, 0], thr[:, 1]
            kind1 = np.where(c1 == 0, r >> 23, ((r * c1) >> 24) >= c0).astype(np.int64)
            kind = np.where(Vj == 1, kind1, kind)
            b = pick(rows("weight", NB, row[:, j]), draw(node, 1))
            x = split(Vj, b, draw(node, 2), np.maximum(Vj - 1, 1))
            first = np.where(kind == 0, 0, np.where(kind == 1, Vj, x))
            first = np.where(Vj == 0, 0, first)
            half[:, 2 * j], half[:, 2 * j + 1] = first, Vj - first
        assert np.array_equal(half.reshape(N, nb, 2).sum(axis=2), box) and half.min() >= 0
        box = half
    units = box.reshape(Q, S, plane, NHOURS)
    units = np.where(masked[:, None, :, None], -1, units)
    units = np.moveaxis(units, 3, 2).reshape(Q, S, NHOURS, ny, nx).astype(np.int32)
    out = np.where(units < 0, np.float32(np.nan), units.astype(np.float32) * np.float32(2.0 ** -10)).astype(np.float32)
    return out, units
