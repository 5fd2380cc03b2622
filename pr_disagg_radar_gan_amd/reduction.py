"""Scenario reduction (csrc/rdgan_reduce.hip.h): which k members of an ensemble of S hourly scenarios to hand to
a model that can afford k, and what each is worth.  The other modules describe, score or re-order a whole ensemble; this one picks a
small weighted subset that stays close to it, by fast forward selection (Heitsch & Roemisch 2003, Algorithm 2.4; Dupacova,
Groewe-Kuska & Roemisch 2003): members are picked greedily so that the Kantorovich distance between the reduced weighted set and the
full, equally weighted ensemble is smallest, and the weight of each left-out member goes to its nearest representative.

Everything is an integer.  A member is ([D,] 24, ny, nx).  A value x is good when it is finite and 0 <= x < 2048; a good value has
e = min(rint(32 x), 65535), rint to even -- the unit and clamp of sequence.py.  With pool = p in {1, 2, 4, 8} a feature position is a
p x p block of one plane (rim blocks are smaller and use their own pixel count n); its feature is (sum e + n / 2) // n, and it is
bad when any of its pixels is.  A member has Pf = D 24 ceil(ny / p) ceil(nx / p) positions, stored as uint16 and padded to a multiple
of 8 with zeros that are never bad.  A position is masked when it is bad in any member added so far -- the bad bits are ORed, and the
mask is applied when distances are formed, so members added before a bad one are treated as those after it.  n_valid = Pf - masked.
Dist[i][j] is the sum over the unmasked positions of |e_i - e_j|, int64, symmetric with a zero diagonal.

Forward selection, k steps: m[j] = +inf; step t computes z[u] = sum over j of min(m[j], Dist[u][j]) for every u not yet selected and
picks the u of the smallest z[u] << 12 | u (ties to the smaller index): chosen[t] = u, cost[t] = z[u], m[j] = min(m[j], Dist[u][j]).
A selected member is skipped explicitly: a duplicate of it has z equal to the current total and would otherwise tie with it.
assign[j] is the chosen u of the smallest Dist[u][j] << 12 | u and counts[t] the members assigned to chosen[t], so sum(counts) = S;
a chosen exact duplicate of a smaller-indexed chosen member gets count 0 (every member it could serve ties with the smaller index,
itself included), and weight 0 -- it can be dropped.

Out of scope: non-uniform input probabilities, backward reduction, PAM swap refinement, other norms, plots.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import MAX_ELEMS, MAX_MEMBERS, MAX_PLANE, admit_array, dense_member_layout, to_state_device
from .engine import require_gpu

UNIT = 32                                                                    # RD_SEQ_UNIT: features are integers in 1 / UNIT mm
FEATMAX = 65535                                                              # RD_SEQ_FEATMAX
POOLS = (1, 2, 4, 8)
KEY_BITS = 52                                                                # RD_RED_KEYBITS: z < 2^52, key = z << 12 | u


def n_positions(shape, pool):
    """Pf of a member of shape ([D,] 24, ny, nx)"""
    ny, nx = shape[-2:]
    return int(np.prod(shape[:-2], dtype=np.int64)) * (-(-ny // pool)) * (-(-nx // pool))


def padded_positions(pf):
    return (int(pf) + 7) // 8 * 8


def bad_words(pf):
    return (padded_positions(pf) + 31) // 32


def check_pool(pool):
    if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)) or int(pool) not in POOLS:
        raise ValueError(f"pool must be one of {POOLS}, got {pool!r}")
    return int(pool)


def check_admission(n_members, pf, max_feature_bytes):
    """the limits of an ensemble of n_members members of pf positions, before any device call"""
    if not 1 <= n_members <= MAX_MEMBERS:
        raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {n_members}")
    if pf * FEATMAX * n_members >= 1 << KEY_BITS:
        raise ValueError(f"{n_members} members of {pf} positions: positions x 65535 x members must stay below 2^{KEY_BITS}; use a larger pool")
    nbytes = 2 * n_members * padded_positions(pf)
    if nbytes > max_feature_bytes:
        raise ValueError(f"the features of {n_members} members of {pf} positions would take {nbytes} bytes, max_feature_bytes is {max_feature_bytes}")


class ScenarioFeatures:
    """The pooled integer features of an ensemble on the device.  pool: 1, 2, 4 or 8, the width of the block of pixels behind a feature
    position; max_feature_bytes: a ValueError, before the device, if the features (2 bytes per member and padded position) would
    exceed it.  add(members) appends members; adding in several calls equals adding at once.  n_positions: Pf.  features (S, Ppad) uint16, bad
    (W,) int32 words, bit f % 32 of word f / 32 set when any member is bad at position f."""

    def __init__(self, pool=1, max_feature_bytes=8 << 30, device=None):
        self.pool = check_pool(pool)
        self.max_feature_bytes = whole_number(max_feature_bytes, 1, 1 << 62, "max_feature_bytes")
        self.device = None if device is None else torch.device(device)
        self.member_shape = self.n_positions = self.lib = self.bad = self._features = None
        self._chunks = []
        self.n_members = 0

    def add(self, members):
        """members (s, [D,] 24, ny, nx) float32: a CUDA tensor, whose member axis may have any stride >= the size of a member (a view
        of a wider buffer), or a numpy array.  The day and plane shape is fixed by the first call; at most 4096 members in all.
        Returns self."""
        members, from_host, shape = admit_array(members, "members")
        if len(shape) not in (4, 5):
            raise ValueError(f"members: expected shape (s, 24, ny, nx) or (s, D, 24, ny, nx), got {shape}")
        if self.member_shape is not None and shape[1:] != self.member_shape:
            raise ValueError(f"members: the shape of a member is {self.member_shape} since the first call, got {shape[1:]}")
        s, mshape = shape[0], shape[1:]
        ny, nx = mshape[-2:]
        P = int(np.prod(mshape, dtype=np.int64))
        if ny * nx > MAX_PLANE or P > MAX_ELEMS:
            raise ValueError(f"members: a plane of {ny * nx} pixels and a member of {P} values; the limits are {MAX_PLANE} and {MAX_ELEMS}")
        pf = n_positions(mshape, self.pool)
        check_admission(self.n_members + s, pf, self.max_feature_bytes)
        members, _, _, stride, _ = dense_member_layout(members, from_host)
        if self.lib is None:
            require_gpu()
            self.lib = _lib.load()
            self.device = (self.device or torch.device("cuda")) if from_host else members.device
        members = to_state_device(members, from_host, self.device, "members")
        self.device = members.device                                         # ("cuda" has become the device it names)
        D = P // (W.NHOURS * ny * nx)
        ppad = padded_positions(pf)
        with torch.cuda.device(self.device):
            if self.bad is None:
                self.bad = torch.zeros(bad_words(pf), dtype=torch.int32, device=self.device)
            feat = torch.empty((s, ppad), dtype=torch.int16, device=self.device)
            rc = self.lib.rdgan_red_features(_p(members), s, stride, D, ny, nx, self.pool, _p(feat), ppad, _p(self.bad), _stream(feat))
        _lib.check(rc, None, "rdgan_red_features")
        self.member_shape, self.n_positions = mshape, pf
        self._chunks.append(feat)
        self._features = None
        self.n_members += s
        return self

    @property
    def features(self):
        """(S, Ppad) uint16, CUDA (its bits live in an int16 tensor viewed as uint16)"""
        if not self._chunks:
            raise ValueError("nothing has been added")
        if self._features is None:
            self._chunks = [self._chunks[0] if len(self._chunks) == 1 else torch.cat(self._chunks)]
            self._features = self._chunks[0].view(torch.uint16)
        return self._features

    def bad_mask(self):
        """the bad bits unpacked: (Pf,) bool, CUDA"""
        self.features
        bits = (self.bad[:, None] >> torch.arange(32, device=self.device, dtype=torch.int32)) & 1
        return bits.reshape(-1)[:self.n_positions].bool()

    @property
    def n_valid(self):
        """Pf - the masked positions, an int (read from the device)"""
        return self.n_positions - int(self.bad_mask().sum())


def member_distances(features, position_splits=None):
    """-> (Dist (S, S) int64 CUDA, n_valid, a 0-d int64 CUDA tensor) of a ScenarioFeatures that has its members.  position_splits: None,
    or into how many ranges the positions of a tile of pairs are cut, one workgroup each (at most one per 128 positions); the result
    does not depend on it."""
    if not isinstance(features, ScenarioFeatures):
        raise ValueError("features: expected a ScenarioFeatures")
    if features.n_members < 1:
        raise ValueError("features: nothing has been added")
    splits = 0 if position_splits is None else whole_number(position_splits, 1, (1 << 31) - 1, "position_splits, unless None,")
    S, pf, dev = features.n_members, features.n_positions, features.device
    feat = features.features
    with torch.cuda.device(dev):
        dist = torch.empty((S, S), dtype=torch.int64, device=dev)
        n_valid = torch.empty(1, dtype=torch.int64, device=dev)
        rc = features.lib.rdgan_red_distances(_p(feat), _p(features.bad), S, int(feat.shape[1]), pf, splits, _p(dist), _p(n_valid), _stream(dist))
    _lib.check(rc, None, "rdgan_red_distances")
    return dist, n_valid.view(())


def _assign(rows, chosen, S):
    """assignment and counts on the host from rows = Dist[chosen] (k, S): the smallest Dist[u][j] << 12 | u"""
    keys = (rows.astype(np.uint64) << np.uint64(12)) | chosen.astype(np.uint64)[:, None]
    t = np.argmin(keys, axis=0)                                              # (the keys of a column are distinct unless u repeats)
    return chosen[t].astype(np.int32), np.bincount(t, minlength=len(chosen)).astype(np.int32)


@dataclass
class Reduction:
    """What select() found, numpy on the host.  chosen (k,) int32: the members in the order they were picked; cost (k,) int64:
    cost[t] = sum over all members of the distance to the nearest of the first t + 1 picks (non-increasing in t); assign (S,)
    int32: the pick each member goes to; counts (k,) int32: how many go to chosen[t], sum S -- 0 for a pick that duplicates a
    smaller-indexed pick exactly.  dist_chosen (k, S) int64: the rows Dist[chosen], from which prefix() re-assigns.  n_valid: the
    unmasked positions behind the distances, or None for a distance of the caller's.  reduce_field adds latent (k, ...), the latent
    vectors of the picks, and with return_hourly hourly (k, [D,] 24, ny, nx) on the device."""
    chosen: np.ndarray
    cost: np.ndarray
    assign: np.ndarray
    counts: np.ndarray
    dist_chosen: np.ndarray
    n_members: int
    n_valid: int = None
    latent: object = None
    hourly: object = None

    @property
    def weights(self):
        """(k,) the probability of each pick: counts / S"""
        return self.counts / float(self.n_members)

    @property
    def mean_distance_mm(self):
        """(k,) cost / (32 S n_valid): the mean distance of a member to its pick in mm/h per valid position, after 1 .. k picks -- the
        curve on which k is chosen.  NaN without n_valid"""
        if not self.n_valid:
            return np.full(len(self.cost), np.nan)
        return self.cost / (float(UNIT) * self.n_members * self.n_valid)

    def prefix(self, k):
        """The reduction to the first k picks.  Forward selection is nested: chosen[:k] and cost[:k] are those of select(dist, k);
        assign and counts are formed again, on the host."""
        k = whole_number(k, 1, len(self.chosen), "k")
        chosen, rows = self.chosen[:k], self.dist_chosen[:k]
        assign, counts = _assign(rows, chosen, self.n_members)
        return Reduction(chosen, self.cost[:k], assign, counts, rows, self.n_members, self.n_valid,
                         None if self.latent is None else self.latent[:k], None if self.hourly is None else self.hourly[:k])


def _check_dist(dist, k):
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.int64:
        raise ValueError("dist: expected an int64 tensor, as member_distances returns it")
    if dist.dim() != 2 or dist.shape[0] != dist.shape[1] or dist.shape[0] < 1:
        raise ValueError(f"dist: expected shape (S, S) with S >= 1, got {tuple(dist.shape)}")
    S = int(dist.shape[0])
    if S > MAX_MEMBERS:
        raise ValueError(f"dist: at most {MAX_MEMBERS} members, got {S}")
    k = whole_number(k, 1, S, "k")
    if not dist.is_cuda:
        raise ValueError("dist: expected a CUDA tensor")
    return dist.contiguous(), S, k


def select(dist, k, n_valid=None):
    """Fast forward selection of k of the S members behind dist (S, S) int64 CUDA -> Reduction.  dist: what member_distances
    returns, or any symmetric matrix with 0 <= entries < 2^52 / S -- a precondition, not checked (it would cost a reduction and a
    wait on the device): the catchment hyetographs of CatchmentRainfall can be reduced through a distance the caller forms.  All k
    steps are enqueued at once; the host waits only for the result.  n_valid: what member_distances returned beside dist, for
    Reduction.mean_distance_mm."""
    dist, S, k = _check_dist(dist, k)
    require_gpu()
    lib = _lib.load()
    dev = dist.device
    with torch.cuda.device(dev):
        nbytes = workspace_bytes(lib, "rdgan_red_workspace_bytes", S, k)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        chosen = torch.empty(k, dtype=torch.int32, device=dev)
        cost = torch.empty(k, dtype=torch.int64, device=dev)
        assign = torch.empty(S, dtype=torch.int32, device=dev)
        counts = torch.empty(k, dtype=torch.int32, device=dev)
        rc = lib.rdgan_red_select(_p(dist), S, k, _p(chosen), _p(cost), _p(assign), _p(counts), _p(ws), nbytes, _stream(dist))
        _lib.check(rc, None, "rdgan_red_select")
        rows = dist.index_select(0, chosen.long()).cpu().numpy()
    return Reduction(chosen.cpu().numpy(), cost.cpu().numpy(), assign.cpu().numpy(), counts.cpu().numpy(), rows, S,
                     None if n_valid is None else int(n_valid))


def reduce_features(features, k):
    """select() on the distances of a ScenarioFeatures that has its members"""
    dist, n_valid = member_distances(features)
    return select(dist, k, n_valid)


def reduce_hourly(ens, k, pool=1, max_feature_bytes=8 << 30):
    """One call for an ensemble that is held: ens (S, [D,] 24, ny, nx), a float32 CUDA tensor or a numpy array -> Reduction"""
    pool = check_pool(pool)
    shape = tuple(int(n) for n in getattr(ens, "shape", ()))
    if len(shape) in (4, 5):
        whole_number(k, 1, shape[0], "k")
    return reduce_features(ScenarioFeatures(pool, max_feature_bytes).add(ens), k)


def reduce_field(gen, daily, n_scenarios, k, pool=1, return_hourly=False, scenario_chunk=16, overlap=4, latent_mode="shared", seed=None,
                 latent=None, chunk=1024, norm_scale=W.NORM_SCALE, max_feature_bytes=8 << 30):
    """Disaggregate the daily map ([D,] ny, nx) into n_scenarios scenarios and reduce them to k without holding the fp32 ensemble:
    the scenario stream of field._stream_scenarios with ScenarioFeatures.add as the sink.  The latent array z is drawn once here,
    exactly as field._draw_latent draws it for the same seed, latent and numpy RNG state -- and, as there, not at all for a field
    without a wet tile, whose distances are all 0 and whose picks are 0 .. k - 1.  -> Reduction with .latent = z[chosen] (numpy;
    None when none was drawn): disaggregate(gen, daily, k, latent=result.latent) makes the picks again.  return_hourly: the
    scenarios are streamed a second time with the same z and scenario_chunk -- the same disaggregate calls as the first pass, so the
    features of the returned members equal the stored features of the picks bit for bit -- and the picks copied out as .hourly
    (k, [D,] 24, ny, nx) on the device.  Against reduce_hourly(disaggregate(...all scenarios...)[0], k) the integers are equal when
    the batches are the same, as _hourly.evaluate_field says."""
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    k, pool = whole_number(k, 1, S, "k"), check_pool(pool)
    req = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    _, squeeze_day, D, ny, nx, plan, z_shape = req
    mshape = (W.NHOURS, ny, nx) if squeeze_day else (D, W.NHOURS, ny, nx)
    if ny * nx > MAX_PLANE or D * W.NHOURS * ny * nx > MAX_ELEMS:
        raise ValueError(f"daily: at most {MAX_PLANE} pixels a plane and {MAX_ELEMS} hourly values a scenario")
    feats = ScenarioFeatures(pool, max_feature_bytes)
    check_admission(S, n_positions(mshape, pool), feats.max_feature_bytes)
    dd, info, _ = F._scan_request(req[0], D, ny, nx, plan)
    with torch.cuda.device(dd.device):
        z = F._draw_latent(latent, seed, z_shape, dd.device) if info.n_active else None
    stream = lambda sink: F._stream_scenarios(gen, req, dd, S, step, sink, overlap, latent_mode, None, z, chunk, norm_scale)
    stream(feats.add)
    result = reduce_features(feats, k)
    if z is not None:
        result.latent = z.cpu().numpy()[result.chosen]
    if return_hourly:
        out = torch.empty((k,) + mshape, dtype=torch.float32, device=dd.device)
        seen = [0]

        def keep(buf):
            s0, n = seen[0], int(buf.shape[0])
            for t, u in enumerate(result.chosen):
                if s0 <= u < s0 + n:
                    out[t].copy_(buf[int(u) - s0])
            seen[0] = s0 + n

        stream(keep)
        result.hourly = out
    return result
