"""Multivariate rank histograms (csrc/rdgan_mvrank.hip.h): is an ensemble of whole hourly days CALIBRATED as a
joint forecast?  multivariate.py scores such an ensemble; a proper score does not say which way it fails.  A rank histogram does:
under-dispersed, over-dispersed, biased, or wrong dependence between pixels and hours.  Three pre-ranks after Thorarinsdottir,
Scheuerer & Heinz (2016) and Smith & Hansen / Wilks (2004); all are integers.

One case is a day (24, ny, nx): z_0 = the observation, z_1 .. z_m = the members, N = m + 1 <= 4096.  A position is valid when the
observation and every member are finite there (members may hold NaN, unlike in multivariate.py); all members are in the call, so the
result does not depend on their order.  Per valid position p and per i, comparing in fp32 (-0.0 == 0.0):
lt_i = #{j : z_j[p] < z_i[p]}, gt_i = #{j : z_j[p] > z_i[p]}.

average rank   avg_i = sum over p of (lt_i - gt_i + N + 1): twice the mid-rank, so ties -- most of a precipitation field -- cost nothing
               and need no randomness.
band depth     depth_i = sum over p of ((N - 1)(N - 2) - lt_i (lt_i - 1) - gt_i (gt_i - 1)): twice the number of pairs of the OTHER
               vectors whose closed interval holds z_i[p].  Low means outlying.
MST            mst_i = the length of the minimum spanning tree of the set WITHOUT z_i under the L1 distance of reduction.py's uint16
               features at the chosen pool.  This route alone quantises to 1/32 mm and treats a value < 0 or >= 2048 as bad (the bad
               positions of the observation and of every member are ORed, as ScenarioFeatures does); the two rank routes use the raw
               fp32 values and only leave non-finite positions out.  The weights are integers, so the length is unique whatever the
               order of equal edges.  N = 2 gives 0.

The observation's rank for a pre-rank rho: below = #{i >= 1 : rho_i < rho_0}, equal = #{i >= 1 : rho_i == rho_0}, rank = below + U
with U uniform on 0 .. equal from numpy.random.default_rng(seed) on the host; the histogram is over the cases.  A case without a
valid position is left out of the histograms and counted.

Out of scope: the Euclidean MST, the multivariate rank of Gneiting et al. 2008 (dominance counting), members streamed across calls
(a rank needs all members at once), plots.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from . import reduction as R
from ._dev import device_f32, flag, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._experiment import competing_methods, for_each_day
from ._hourly import MAX_ELEMS, MAX_PLANE, NHOURS, admit_ensemble, ensemble_on_device, shape_of  # noqa: F401 (the limits are public here)
from .engine import require_gpu

MAX_VECTORS = 4096                                                           # RD_MVR_MAXN: the observation and the members
MAX_MEMBERS = MAX_VECTORS - 1                                                # RD_MVR_MAXM
MAX_DAYS = 1 << 20                                                           # RD_MVR_MAXDAYS
MAX_DIST = 1 << 40                                                           # RD_MVR_MAXDIST: an MST edge lies below it
KINDS = ("average", "band_depth", "mst")


# ---------------------------------------------------------------------------------------------------------------------------------
# host: arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def admit(ens, obs):
    """_hourly.admit_ensemble with the limits of the ranks: at most 4095 members, 2^20 days, N 24 ny nx <= 2^40.  -> (m, D, ny, nx, shared)"""
    return admit_ensemble(ens, obs, MAX_MEMBERS, MAX_DAYS, obs_is_a_vector=True)


def check_kinds(kinds, by_hour=False):
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    if not kinds or len(set(kinds)) != len(kinds) or any(k not in KINDS for k in kinds):
        raise ValueError(f"kinds: expected distinct names out of {KINDS}, got {kinds!r}")
    if by_hour and "mst" in kinds:
        raise ValueError("the MST pre-rank is of the whole day: by_hour=True cannot be combined with kind 'mst'")
    return kinds


# ---------------------------------------------------------------------------------------------------------------------------------
# the pre-ranks
# ---------------------------------------------------------------------------------------------------------------------------------
def prerank_sums(ens, obs, by_hour=False, position_runs=None):
    """-> (sums, n_valid), int64 CUDA tensors.  sums (D, N, 2), or (D, 24, N, 2) with by_hour: index 0 of N is the observation, the
    last axis is (avg, depth) as defined above; n_valid (D,) or (D, 24): the valid positions.  ens (m, 24, ny, nx) -- one ensemble
    for every day of obs -- or (D, m, 24, ny, nx); obs (24, ny, nx) (D = 1) or (D, 24, ny, nx); numpy or CUDA; members may hold NaN.
    position_runs: None, or into how many runs the tiles of positions of a plane are cut, one workgroup each; the result does not
    depend on it."""
    by_hour = flag(by_hour, "by_hour")
    runs = 0 if position_runs is None else whole_number(position_runs, 1, (1 << 31) - 1, "position_runs, unless None,")
    m, D, ny, nx, shared = admit(ens, obs)
    ens, obs = ensemble_on_device(ens, obs)
    lib, dev = _lib.load(), ens.device
    with torch.cuda.device(dev):
        sums = torch.empty((D, NHOURS, m + 1, 2), dtype=torch.int64, device=dev)
        n_valid = torch.empty((D, NHOURS), dtype=torch.int64, device=dev)
        nbytes = workspace_bytes(lib, "rdgan_mvr_ranks_workspace_bytes", m, D, int(shared))
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
        rc = lib.rdgan_mvr_ranks(_p(ens), _p(obs), m, D, ny, nx, int(shared), runs, _p(sums), _p(n_valid), _p(ws), nbytes, _stream(ens))
    _lib.check(rc, None, "rdgan_mvr_ranks")
    return (sums, n_valid) if by_hour else (sums.sum(dim=1), n_valid.sum(dim=1))


def _check_dist(dist):
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.int64:
        raise ValueError("dist: expected an int64 tensor, as reduction.member_distances returns it")
    if dist.dim() != 2 or dist.shape[0] != dist.shape[1] or not 1 <= dist.shape[0] <= MAX_VECTORS:
        raise ValueError(f"dist: expected shape (N, N) with 1 <= N <= {MAX_VECTORS}, got {tuple(dist.shape)}")
    if not dist.is_cuda:
        raise ValueError("dist: expected a CUDA tensor")
    return dist.contiguous(), int(dist.shape[0])


def mst_leave_one_out(dist, check=True):
    """dist (N, N) int64 CUDA, symmetric, 0 <= entries < 2^40 -> (N,) int64 CUDA: entry i is the length of the minimum spanning tree of
    the vertices other than i; 0 for N <= 2.  check: the range of the entries is read back from the device first and a ValueError
    raised outside it; mst_preranks, whose features bound the distances by arithmetic, turns it off."""
    check = flag(check, "check")
    dist, N = _check_dist(dist)
    require_gpu()
    lib, dev = _lib.load(), dist.device
    with torch.cuda.device(dev):
        if check:
            lo, hi = int(dist.min()), int(dist.max())
            if lo < 0 or hi >= MAX_DIST:
                raise ValueError(f"dist: entries must lie in 0 .. 2^40 - 1, found {lo} .. {hi}")
        out = torch.empty(N, dtype=torch.int64, device=dev)
        rc = lib.rdgan_mvr_mst(_p(dist), N, _p(out), _stream(dist))
    _lib.check(rc, None, "rdgan_mvr_mst")
    return out


def check_mst_admission(n_vectors, pf):
    """before any device call: N <= 4096 and a distance below 2^40, by the rule of reduction.check_admission (positions x 65535)"""
    if not 2 <= n_vectors <= MAX_VECTORS:
        raise ValueError(f"the observation and the members must number 2 .. {MAX_VECTORS}, got {n_vectors}")
    if pf * R.FEATMAX >= MAX_DIST:
        raise ValueError(f"{pf} positions: positions x {R.FEATMAX} must stay below 2^40; use a larger pool")


def mst_preranks(ens_day, obs_day, pool=1):
    """One case: ens_day (m, 24, ny, nx), obs_day (24, ny, nx), numpy or float32 CUDA -> (lengths (N,) int64 CUDA, index 0 the
    observation; n_valid, a 0-d int64 CUDA tensor).  The members and then the observation go through reduction.ScenarioFeatures at
    this pool (the observation is added last and read back as index 0), reduction.member_distances and the MST kernel."""
    pool = R.check_pool(pool)
    es, os_ = shape_of(ens_day, "ens_day"), shape_of(obs_day, "obs_day")
    if len(es) != 4 or es[1] != NHOURS or min(es) < 1 or os_ != es[1:]:
        raise ValueError(f"ens_day (m, {NHOURS}, ny, nx) and obs_day ({NHOURS}, ny, nx) expected, got {es} and {os_}")
    m = es[0]
    check_mst_admission(m + 1, R.n_positions(es[1:], pool))
    if isinstance(ens_day, torch.Tensor) != isinstance(obs_day, torch.Tensor):           # (ScenarioFeatures pins the device by its first call)
        require_gpu()
        ens_day = device_f32(ens_day, "ens_day", obs_day.device if isinstance(obs_day, torch.Tensor) else None)
        obs_day = device_f32(obs_day, "obs_day", ens_day.device)
    feats = R.ScenarioFeatures(pool).add(ens_day).add(obs_day[None])
    dist, n_valid = R.member_distances(feats)
    order = torch.cat([torch.tensor([m], device=dist.device), torch.arange(m, device=dist.device)])
    dist = dist.index_select(0, order).index_select(1, order)
    return mst_leave_one_out(dist, check=False), n_valid


def observation_ranks(preranks):
    """preranks (..., N), index 0 the observation; a tensor or an array -> (below, equal), numpy int64 (...): the members whose pre-rank
    lies below the observation's, and those that equal it"""
    if isinstance(preranks, torch.Tensor):
        preranks = preranks.detach().cpu().numpy()
    r = np.asarray(preranks)
    if r.ndim < 1 or r.shape[-1] < 2 or not (np.issubdtype(r.dtype, np.integer) or np.issubdtype(r.dtype, np.floating)):
        raise ValueError(f"preranks: expected numbers of shape (..., N) with N >= 2, got {r.dtype} {r.shape}")
    return (r[..., 1:] < r[..., :1]).sum(axis=-1).astype(np.int64), (r[..., 1:] == r[..., :1]).sum(axis=-1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class MultivariateRanks:
    """The observation's place among n_members members, per case and kind, numpy on the host.  kinds: the kinds held, out of
    ("average", "band_depth", "mst").  below[kind], equal[kind], n_valid[kind]: int64 (cases,) -- or (cases, 24) for a by_hour
    result, every (day, hour) a case; n_valid is the valid positions behind the pre-rank (the MST's count is of feature positions).
    A case with n_valid = 0 is left out of every histogram and counted by n_empty."""
    kinds: Tuple[str, ...]
    n_members: int
    below: Dict[str, np.ndarray] = field(default_factory=dict)
    equal: Dict[str, np.ndarray] = field(default_factory=dict)
    n_valid: Dict[str, np.ndarray] = field(default_factory=dict)

    def _kind(self, kind):
        if kind not in self.kinds:
            raise ValueError(f"kind: expected one of {self.kinds}, got {kind!r}")
        return kind

    def n_cases(self, kind):
        return int((self.n_valid[self._kind(kind)] > 0).sum())

    def n_empty(self, kind):
        """the cases without a valid position"""
        return int((self.n_valid[self._kind(kind)] <= 0).sum())

    def ranks(self, kind, seed=0):
        """(cases used,) int64 in 0 .. n_members: below + U, U uniform on 0 .. equal from numpy.random.default_rng(seed)"""
        kind, seed = self._kind(kind), whole_number(seed, 0, 1 << 62, "seed")
        keep = self.n_valid[kind].reshape(-1) > 0
        below, equal = self.below[kind].reshape(-1)[keep], self.equal[kind].reshape(-1)[keep]
        return below + np.random.default_rng(seed).integers(0, equal + 1)

    def histogram(self, kind, n_bins=None, seed=0):
        """(n_bins,) int64 counts of the cases' ranks.  n_bins: None for the n_members + 1 ranks, or a divisor of n_members + 1:
        neighbouring ranks are merged into bins of equal width."""
        n_ranks = self.n_members + 1
        n_bins = n_ranks if n_bins is None else whole_number(n_bins, 1, n_ranks, "n_bins")
        if n_ranks % n_bins:
            raise ValueError(f"n_bins must divide the {n_ranks} ranks, got {n_bins}")
        return np.bincount(self.ranks(kind, seed) // (n_ranks // n_bins), minlength=n_bins).astype(np.int64)

    def reliability_index(self, kind, n_bins=None, seed=0):
        """sum over the bins of |f_k - 1 / n_bins|, f the relative frequencies (Delle Monache et al. 2006): 0 for a flat histogram;
        NaN without a case"""
        h = self.histogram(kind, n_bins, seed)
        return float(np.abs(h / h.sum() - 1.0 / len(h)).sum()) if h.sum() else float("nan")

    def summary(self, n_bins=None, seed=0):
        """{kind: {"cases", "empty", "histogram", "reliability_index", "low", "high"}}: low and high are the shares of the cases in
        the lowest and the highest bin -- both high under an average-rank histogram: under-dispersed; the lowest under band depth or
        MST: the observation is an outlier too often"""
        out = {}
        for kind in self.kinds:
            h = self.histogram(kind, n_bins, seed)
            total = int(h.sum())
            out[kind] = {"cases": total, "empty": self.n_empty(kind), "histogram": h.tolist(),
                         "reliability_index": self.reliability_index(kind, n_bins, seed),
                         "low": h[0] / total if total else float("nan"), "high": h[-1] / total if total else float("nan")}
        return out


def compare(a, b, n_bins=None, seed=0):
    """Two results side by side: {kind: {"a": ..., "b": ..., "reliability_index_difference": a - b}} for the kinds both hold, each
    side its summary() entry; the two must agree on n_members + 1 being divisible by n_bins, not on n_members."""
    if not isinstance(a, MultivariateRanks) or not isinstance(b, MultivariateRanks):
        raise ValueError("compare: expected two MultivariateRanks")
    sa, sb = a.summary(n_bins, seed), b.summary(n_bins, seed)
    return {k: {"a": sa[k], "b": sb[k], "reliability_index_difference": sa[k]["reliability_index"] - sb[k]["reliability_index"]}
            for k in a.kinds if k in b.kinds}


def _collect(kinds, m, parts):
    """parts: [{kind: (below, equal, n_valid)}] per call, concatenated along the cases"""
    res = MultivariateRanks(kinds, m)
    for k in kinds:
        res.below[k], res.equal[k], res.n_valid[k] = (np.concatenate([p[k][i] for p in parts]) for i in range(3))
    return res


def _case_ranks(ens, obs, kinds, by_hour, pool, m, D, shared):
    """{kind: (below, equal, n_valid)} of one call's D cases; ens and obs on the device"""
    out = {}
    if "average" in kinds or "band_depth" in kinds:
        sums, n_valid = prerank_sums(ens, obs, by_hour=by_hour)
        sums, n_valid = sums.cpu().numpy(), n_valid.cpu().numpy()
        for q, k in enumerate(("average", "band_depth")):
            if k in kinds:
                out[k] = observation_ranks(sums[..., q]) + (n_valid,)
    if "mst" in kinds:
        obs4 = obs.reshape((D,) + tuple(obs.shape[-3:]))
        rows = [mst_preranks(ens if shared else ens[d], obs4[d], pool) for d in range(D)]
        below, equal = observation_ranks(torch.stack([r[0] for r in rows]))
        out["mst"] = (below, equal, torch.stack([r[1] for r in rows]).cpu().numpy())
    return out


def multivariate_ranks(ens, obs, kinds=KINDS, by_hour=False, pool=1):
    """The observation's ranks for the D cases of a call -> MultivariateRanks.  ens and obs as prerank_sums.  by_hour: every (day,
    hour) is a case of its own (below, equal, n_valid of shape (D, 24)); the MST is of the whole day only, and asking for it with
    by_hour is a ValueError.  pool: of the MST's features."""
    by_hour = flag(by_hour, "by_hour")
    kinds, pool = check_kinds(kinds, by_hour), R.check_pool(pool)
    m, D, ny, nx, shared = admit(ens, obs)
    if "mst" in kinds:
        check_mst_admission(m + 1, R.n_positions((NHOURS, ny, nx), pool))
    ens, obs = ensemble_on_device(ens, obs)
    return _collect(kinds, m, [_case_ranks(ens, obs, kinds, by_hour, pool, m, D, shared)])


def ranks_for_days(make_ensemble, reals, kinds=KINDS, by_hour=False, pool=1):
    """reals (D, 24, ny, nx), numpy or CUDA; make_ensemble(d) -> day d's (m, 24, ny, nx) ensemble, which is ranked against reals[d]
    and dropped before the next one is made, as multivariate.scores_for_days does: one ensemble is alive at a time.  Every day
    must bring the same number of members.  -> MultivariateRanks."""
    by_hour = flag(by_hour, "by_hour")
    kinds, pool = check_kinds(kinds, by_hour), R.check_pool(pool)
    members = []

    def per_day(d, ens, real):
        one = multivariate_ranks(ens, real, kinds, by_hour, pool)
        if members and one.n_members != members[-1]:
            raise ValueError(f"make_ensemble({d}) brought {one.n_members} members, the days before it {members[-1]}")
        members.append(one.n_members)
        return {k: (one.below[k], one.equal[k], one.n_valid[k]) for k in kinds}

    parts = for_each_day(make_ensemble, reals, per_day)
    return _collect(kinds, members[0], parts)


def multivariate_rank_experiment(gen, reals_precip, climatology, slopes=None, library=None, n_members=1000, seed=0, kinds=KINDS,
                                 by_hour=False, pool=1, k=10, analog_weights="rank", query_groups=None, cascade=None, cascade_patch=1):
    """The rank histograms of the competing methods over the real days: {method: MultivariateRanks} with "gan", "random" (the fixed
    climatological ensemble, ranked in the shared form) and "rainfarm" / "analog" / "cascade" where the experiment has slopes / a
    library / a cascade model.  The competitors, their arguments and their seed rules are those of _experiment.competing_methods, as in
    multivariate.multivariate_experiment: the two experiments see the same members.  n_members and the climatology: at most 4095."""
    by_hour = flag(by_hour, "by_hour")
    rank = dict(kinds=check_kinds(kinds, by_hour), by_hour=by_hour, pool=R.check_pool(pool))
    roster = competing_methods(gen, reals_precip, climatology, max_members=MAX_MEMBERS, slopes=slopes, library=library, n_members=n_members,
                               seed=seed, k=k, analog_weights=analog_weights, query_groups=query_groups, cascade=cascade, cascade_patch=cascade_patch)
    return roster.run(lambda make: ranks_for_days(make, roster.reals, **rank), lambda clim, reals: multivariate_ranks(clim, reals, **rank))
