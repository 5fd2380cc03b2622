"""Chaining scenarios across midnight (csrc/rdgan_sequence.hip.h).  Every other module here treats a day as an
independent unit: member s of day d has nothing to do with member s of day d + 1, and a user who concatenates them pairs independent
draws.  This module does not make the generator aware of the previous day; it makes the best use of the ensemble there is: it
measures how well every member of one day continues every member of the next (seam_costs), picks continuous series from that --
the cheapest single one (best_path) and a matching that uses every member of every day exactly once (greedy_matching, series_order,
reorder) -- and reports how far the seams are from observed ones (chain, compare).

Everything is an integer.  A value x of an hourly array is good when it is finite and 0 <= x < 2048; a good value has the feature
e = min(rint(x * 32), 65535), a uint16 in 1/32 mm (rint to even), a bad one the feature 0 and the bad bit of its (day, edge, pixel).
A day has two edges, its first_hour (0) and its last_hour (23).  Boundary b joins the last edge of day b to the first edge of day
b + shift (1: a seam; 0: two hours of the same day, a yardstick).  A pixel is masked at b when the bad bit of either edge is set for
any member; n_valid[b] counts the others.  C[b][i][j] is the sum over the unmasked pixels of |e_i - e_j|, an int64 below 2^40, and
key = C << 24 | i << 12 | j orders the pairs strictly.  The greedy matching walks all pairs by ascending key and takes a pair when
neither its row nor its column is taken; it is NOT the assignment of least total cost: that is optimal_matching (DESIGN.md section
32, csrc/rdgan_assign.hip.h), shortest augmenting paths with dual potentials, which chain* use with matching="optimal".

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass, replace

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import MAX_MEMBERS, MAX_PLANE, NHOURS, admit, to_state_device
from .engine import require_gpu

UNIT = 32                                                                    # RD_SEQ_UNIT: features are integers in 1 / UNIT mm
MAX_DAYS = 65535                                                             # RD_SEQ_MAXDAYS
MAX_COSTS = 1 << 31                                                          # RD_SEQ_MAXCOSTS: elements of one call's cost array
MAX_COST = 1 << 40                                                           # a cost lies below it: RD_SEQ_FEATMAX + 1 times MAX_PLANE
YARDSTICK_HOURS = (11, 12)                                                   # the within-day pair compare() sets beside the seams
_FIRST_BATCH = 8                                                             # rounds of the first batch of a matching; then doubled
MATCHINGS = ("greedy", "optimal")                                            # what chain* accept as `matching`


def padded_plane(plane):
    """Ppad: the pixels of a plane rounded up to whole groups of 8 (rd_seq_ppad)"""
    return (int(plane) + 7) // 8 * 8


def bad_words(plane):
    """W: the 32-bit words of one edge's bad bits (rd_seq_words)"""
    return (padded_plane(plane) + 31) // 32


def check_hour(hour, what):
    return whole_number(hour, 0, NHOURS - 1, what)


class SeamEdges:
    """The two edge hours of an ensemble of hourly days on the device, as integer features.  add(hourly) appends members; adding in
    several calls equals adding at once.  features (S, D, 2, Ppad) uint16 -- edge 0 the first_hour, edge 1 the last_hour, padding
    pixels 0 -- and bad (D, 2, W) int32 words, bit p % 32 of word p / 32 set when any member is bad at pixel p of that (day, edge)."""

    def __init__(self, first_hour=0, last_hour=23, device=None):
        self.first_hour, self.last_hour = check_hour(first_hour, "first_hour"), check_hour(last_hour, "last_hour")
        self.device = None if device is None else torch.device(device)
        self.plane_shape = self.n_days = self.lib = self.bad = self._features = None
        self._chunks = []
        self.n_members = 0

    def add(self, hourly):
        """hourly (n, D, 24, ny, nx), n members of D days, or (D, 24, ny, nx), one member: float32, a CUDA tensor (the leading axes as
        _hourly.tensor_layout admits them) or a numpy array.  D and the plane are fixed by the first call; at most 4096 members.
        Only the two edge hours are read.  Returns self."""
        hourly, from_host, shape, n, stride = admit(hourly, self.plane_shape)
        if len(shape) not in (4, 5):
            raise ValueError(f"hourly: expected shape (n, D, 24, ny, nx) or (D, 24, ny, nx), got {shape}")
        D, ny, nx = shape[-4], shape[-2], shape[-1]
        members = n // D
        if ny * nx > MAX_PLANE:
            raise ValueError(f"hourly: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
        if D > MAX_DAYS or (self.n_days is not None and D != self.n_days):
            raise ValueError(f"hourly: {D} days; at most {MAX_DAYS}" + (f", and {self.n_days} since the first call" if self.n_days else ""))
        if self.n_members + members > MAX_MEMBERS:
            raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {self.n_members + members}")
        if self.lib is None:
            require_gpu()
            self.lib = _lib.load()
            self.device = (self.device or torch.device("cuda")) if from_host else hourly.device
        hourly = to_state_device(hourly, from_host, self.device)
        plane = ny * nx
        with torch.cuda.device(self.device):
            if self.bad is None:
                self.bad = torch.zeros((D, 2, bad_words(plane)), dtype=torch.int32, device=self.device)
            feat = torch.empty((members, D, 2, padded_plane(plane)), dtype=torch.int16, device=self.device)
            rc = self.lib.rdgan_seq_edges(_p(hourly), n, stride, ny, nx, D, self.first_hour, self.last_hour, _p(feat), _p(self.bad),
                                          _stream(feat))
        _lib.check(rc, None, "rdgan_seq_edges")
        self.plane_shape, self.n_days = (ny, nx), D
        self._chunks.append(feat)
        self._features = None
        self.n_members += members
        return self

    @property
    def features(self):
        """(S, D, 2, Ppad) uint16, CUDA (its bits live in an int16 tensor viewed as uint16)"""
        if not self._chunks:
            raise ValueError("nothing has been added")
        if self._features is None:
            self._chunks = [self._chunks[0] if len(self._chunks) == 1 else torch.cat(self._chunks)]
            self._features = self._chunks[0].view(torch.uint16)
        return self._features

    def bad_mask(self):
        """the bad bits unpacked: (D, 2, P) bool, CUDA"""
        self.features
        P = self.plane_shape[0] * self.plane_shape[1]
        bits = (self.bad[..., None] >> torch.arange(32, device=self.device, dtype=torch.int32)) & 1
        return bits.reshape(self.n_days, 2, -1)[..., :P].bool()


def _check_edges(edges, what):
    if not isinstance(edges, SeamEdges):
        raise ValueError(f"{what}: expected a SeamEdges")
    if edges.n_members < 1:
        raise ValueError(f"{what}: nothing has been added")
    return edges


def seam_costs(edges, shift=1, other=None, pixel_splits=None):
    """-> (costs (B, S_a, S_b) int64 CUDA, n_valid (B,) int64 CUDA), B = D - shift: costs[b][i][j] joins the last edge of day b of
    member i of `edges` to the first edge of day b + shift of member j of `other` (default: of `edges` itself; observed days are an
    ensemble of one member).  shift 1 is a seam, shift 0 pairs two hours of the same day.  Both ensembles must have the same days
    and plane.  pixel_splits: None, or into how many ranges the pixels of a tile of pairs are cut, one workgroup each (at most one
    per 128 pixels); the result does not depend on it."""
    a = _check_edges(edges, "edges")
    b = a if other is None else _check_edges(other, "other")
    if (b.n_days, b.plane_shape) != (a.n_days, a.plane_shape):
        raise ValueError(f"other holds {b.n_days} days of {b.plane_shape}, edges {a.n_days} of {a.plane_shape}")
    if b.device != a.device:
        raise ValueError(f"other lies on {b.device}, edges on {a.device}")
    D = a.n_days
    shift = whole_number(shift, 0, D - 1, "shift")
    splits = 0 if pixel_splits is None else whole_number(pixel_splits, 1, MAX_PLANE, "pixel_splits, unless None,")
    B, Sa, Sb = D - shift, a.n_members, b.n_members
    if B * Sa * Sb > MAX_COSTS:
        raise ValueError(f"{B} boundaries of {Sa} x {Sb} pairs, the limit is {MAX_COSTS} costs a call")
    fa, fb = a.features, b.features
    dev = a.device
    with torch.cuda.device(dev):
        costs = torch.empty((B, Sa, Sb), dtype=torch.int64, device=dev)
        n_valid = torch.empty(B, dtype=torch.int64, device=dev)
        rc = a.lib.rdgan_seq_costs(_p(fa), _p(a.bad), Sa, _p(fb), _p(b.bad), Sb, D, a.plane_shape[0] * a.plane_shape[1], shift, splits, _p(costs),
                                   _p(n_valid), _stream(costs))
    _lib.check(rc, None, "rdgan_seq_costs")
    return costs, n_valid


def _check_costs(costs):
    """a cost array for best_path and greedy_matching: (B, S, S) int64 on the device, contiguous; host code"""
    if not isinstance(costs, torch.Tensor) or costs.dtype != torch.int64:
        raise ValueError("costs: expected an int64 tensor, as seam_costs returns it")
    if costs.dim() != 3 or costs.shape[1] != costs.shape[2] or min(costs.shape) < 1:
        raise ValueError(f"costs: expected shape (B, S, S) with B, S >= 1, got {tuple(costs.shape)}")
    B, S = int(costs.shape[0]), int(costs.shape[1])
    if S > MAX_MEMBERS or B > MAX_DAYS or B * S * S > MAX_COSTS:
        raise ValueError(f"costs: at most {MAX_MEMBERS} members, {MAX_DAYS} boundaries and {MAX_COSTS} costs, got {tuple(costs.shape)}")
    if not costs.is_cuda:
        raise ValueError("costs: expected a CUDA tensor")
    return costs.contiguous(), B, S


def min_plus(costs):
    """costs (B, S, S) -> (acc (B + 1, S) int64, back (B, S) int32), CUDA: acc[0] = 0, acc[b + 1][j] = min over i of acc[b][i] +
    costs[b][i][j], back[b][j] the smallest i that attains it"""
    costs, B, S = _check_costs(costs)
    require_gpu()
    lib = _lib.load()
    with torch.cuda.device(costs.device):
        acc = torch.empty((B + 1, S), dtype=torch.int64, device=costs.device)
        back = torch.empty((B, S), dtype=torch.int32, device=costs.device)
        rc = lib.rdgan_seq_minplus(_p(costs), B, S, _p(acc), _p(back), _stream(costs))
    _lib.check(rc, None, "rdgan_seq_minplus")
    return acc, back


def best_path(costs):
    """The cheapest single series: -> (path (B + 1,) int64 numpy, total int), path[d] the member of day d.  Ties go to the smaller
    member, at every step and at the end; the recurrence runs on the device, the backtracking on the host."""
    acc, back = min_plus(costs)
    last, back = acc[-1].cpu().numpy(), back.cpu().numpy()
    path = [int(np.argmin(last))]                                            # (the first of equals)
    for b in range(back.shape[0] - 1, -1, -1):
        path.append(int(back[b, path[-1]]))
    return np.array(path[::-1], dtype=np.int64), int(last.min())


def greedy_matching(costs, return_rounds=False):
    """costs (B, S, S) int64 -> perm (B, S) int32 CUDA.  Precondition, not checked (it would cost two reductions and a wait on the
    device): 0 <= C < 2^40, which every result of seam_costs meets; outside it the keys overlap and the matching is not the
    defined one, though still a permutation.  perm[b] is the matching that walking all S^2 pairs of
    boundary b by ascending key = C << 24 | i << 12 | j gives, a pair taken when neither its row nor its column is taken.  It is
    computed as rounds of locally dominant pairs (a free pair is taken iff its key is the minimum of its row over the free columns
    and of its column over the free rows), which yields the same matching because the keys are distinct; a round takes at least
    the smallest free pair, so S rounds suffice.  Rounds are launched in batches and the counters of free rows read in between;
    RdganError if one is not 0 after S rounds.  Not the assignment of least total cost.  return_rounds: also the rounds launched."""
    costs, B, S = _check_costs(costs)
    require_gpu()
    lib = _lib.load()
    dev = costs.device
    with torch.cuda.device(dev):
        nbytes = workspace_bytes(lib, "rdgan_seq_workspace_bytes", S, B)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        perm = torch.empty((B, S), dtype=torch.int32, device=dev)
        free = torch.empty(B, dtype=torch.int32, device=dev)
        done, batch, left = 0, _FIRST_BATCH, S
        while done < S and left:
            n = min(batch, S - done)
            rc = lib.rdgan_seq_match(_p(costs), B, S, 1 if done == 0 else 0, n, _p(perm), _p(free), _p(ws), nbytes, _stream(costs))
            _lib.check(rc, None, "rdgan_seq_match")
            done, batch = done + n, batch * 2
            left = int(free.max())
    if left:
        raise _lib.RdganError(f"greedy_matching: {left} rows are free after {done} rounds of {S} members")
    return (perm, done) if return_rounds else perm


def optimal_matching(costs, return_duals=False):
    """costs (B, S, S) int64 -> perm (B, S) int32 CUDA, for every boundary a permutation of least total cost sum_i C[b][i][perm[b][i]];
    with return_duals (perm, total (B,), u (B, S), v (B, S)), int64 CUDA: u[i] + v[j] <= C[i][j] for all pairs with equality on the
    matched ones, so sum u + sum v == total proves the optimum.  The precondition of greedy_matching, 0 <= C < 2^40, again not
    checked.  Optimal permutations are not unique; the algorithm (rows inserted in the order 0 .. S - 1 by
    shortest augmenting paths, the next column the unused one of the smallest (minv[j], j)) is the definition.  One asynchronous
    launch, one workgroup per boundary, no host wait."""
    costs, B, S = _check_costs(costs)
    require_gpu()
    lib = _lib.load()
    dev = costs.device
    with torch.cuda.device(dev):
        perm = torch.empty((B, S), dtype=torch.int32, device=dev)
        duals = torch.empty((2, B, S), dtype=torch.int64, device=dev)
        total = torch.empty(B, dtype=torch.int64, device=dev)
        rc = lib.rdgan_assign(_p(costs), B, S, _p(perm), _p(duals[0]), _p(duals[1]), _p(total), _stream(costs))
    _lib.check(rc, None, "rdgan_assign")
    return (perm, total, duals[0], duals[1]) if return_duals else perm


def check_matching(matching):
    if matching not in MATCHINGS:
        raise ValueError(f"matching: expected one of {MATCHINGS}, got {matching!r}")
    return matching


def series_order(perm):
    """perm (B, S) -> order (B + 1, S) int64, on perm's device (or numpy for an array): order[0][s] = s, order[d + 1][s] =
    perm[d][order[d][s]]; series s consists of member order[d][s] on day d, and every member of every day is used exactly once"""
    if isinstance(perm, torch.Tensor):
        if perm.dim() != 2 or perm.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"perm: expected whole numbers of shape (B, S), got {perm.dtype} {tuple(perm.shape)}")
        p = perm.long()
        rows = [torch.arange(p.shape[1], device=p.device)]
        for d in range(p.shape[0]):
            rows.append(p[d][rows[-1]])
        return torch.stack(rows)
    p = np.asarray(perm)
    if p.ndim != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"perm: expected whole numbers of shape (B, S), got {p.dtype} {p.shape}")
    rows = [np.arange(p.shape[1], dtype=np.int64)]
    for d in range(p.shape[0]):
        rows.append(p[d].astype(np.int64)[rows[-1]])
    return np.stack(rows)


def reorder(x, order):
    """x (S, D, ...) CUDA tensor, order (D, S) -> the series: out[s, d] = x[order[d][s], d], by torch.gather.  x may be the hourly
    ensemble (S, D, 24, ny, nx) or anything else per member and day, the hyetographs of CatchmentRainfall for one."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() < 2:
        raise ValueError("x: expected a CUDA tensor of shape (S, D, ...)")
    S, D = int(x.shape[0]), int(x.shape[1])
    order = torch.as_tensor(order)
    if tuple(order.shape) != (D, S) or order.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"order: expected whole numbers of shape ({D}, {S}), got {order.dtype} {tuple(order.shape)}")
    idx = order.to(device=x.device, dtype=torch.int64).t().reshape((S, D) + (1,) * (x.dim() - 2)).expand(x.shape)
    return torch.gather(x, 0, idx)


@dataclass
class ChainResult:
    """What chain() found.  order (D, S) int64 and perm (D - 1, S) int32: the matched series (series_order; greedy_matching, or
    optimal_matching when `matching` is "optimal", and then greedy_matched (D - 1,) is what the greedy matching would have given); path
    (D,) and path_total: the cheapest single series and its cost in 1/32 mm; n_valid (D - 1,); and per boundary, in mm/h per valid
    pixel (cost / (32 n_valid), NaN where n_valid is 0): random -- the mean over all pairs, what pairing at random expects;
    diagonal -- the mean over the pairs (s, s), the pairing by index of a plain concatenation; matched -- the mean over the matched
    pairs; path_cost -- the pairs of the path.  compare() adds observed (D - 1,), the seams of the observed days (NaN where they do
    not follow each other), and observed_within (D,), the observed step between the hours 11 and 12 of every day.  All numpy."""
    order: np.ndarray
    perm: np.ndarray
    path: np.ndarray
    path_total: int
    n_valid: np.ndarray
    random: np.ndarray
    diagonal: np.ndarray
    matched: np.ndarray
    path_cost: np.ndarray
    first_hour: int = 0
    last_hour: int = 23
    plane_shape: tuple = ()
    observed: np.ndarray = None
    observed_within: np.ndarray = None
    matching: str = "greedy"
    greedy_matched: np.ndarray = None


def _per_pixel(cost, n_valid):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n_valid > 0, np.asarray(cost, dtype=np.float64) / (UNIT * n_valid.astype(np.float64)), np.nan)


def chain_edges(edges, matching="greedy"):
    """chain() for a SeamEdges that has its members: costs, matching, series order, path and the four seam statistics.  matching:
    "greedy" (greedy_matching) or "optimal" (optimal_matching: least total seam cost per boundary; the result then also holds
    greedy_matched, the matched mean of the greedy matching, so the gain is read off one result)"""
    _check_edges(edges, "edges")
    check_matching(matching)
    if edges.n_days < 2:
        raise ValueError("chaining needs at least 2 days")
    costs, n_valid = seam_costs(edges)
    greedy = greedy_matching(costs)
    perm = optimal_matching(costs) if matching == "optimal" else greedy
    path, total = best_path(costs)
    order = series_order(perm)
    B, S = perm.shape
    with torch.cuda.device(costs.device):
        c = costs.double()
        matched = torch.gather(c, 2, perm.long()[..., None]).mean(dim=(1, 2))
        steps = torch.from_numpy(np.stack([np.arange(B), path[:-1], path[1:]])).to(costs.device)
        rows = [c.mean(dim=(1, 2)), c.diagonal(dim1=1, dim2=2).mean(dim=1), matched,
                costs[steps[0], steps[1], steps[2]].double(), n_valid.double()]
        if matching == "optimal":
            rows.append(torch.gather(c, 2, greedy.long()[..., None]).mean(dim=(1, 2)))
        host = torch.stack(rows).cpu().numpy()
    nv = host[4].astype(np.int64)
    return ChainResult(order=order.cpu().numpy(), perm=perm.cpu().numpy(), path=path, path_total=total, n_valid=nv,
                       random=_per_pixel(host[0], nv), diagonal=_per_pixel(host[1], nv), matched=_per_pixel(host[2], nv),
                       path_cost=_per_pixel(host[3], nv), first_hour=edges.first_hour, last_hour=edges.last_hour,
                       plane_shape=edges.plane_shape, matching=matching,
                       greedy_matched=_per_pixel(host[5], nv) if matching == "optimal" else None)


def chain(hourly, first_hour=0, last_hour=23, matching="greedy"):
    """One call for an ensemble that is held: hourly (S, D, 24, ny, nx), D >= 2 -> ChainResult.  reorder(hourly, result.order) is
    the ensemble as S continuous series.  matching: as for chain_edges."""
    check_matching(matching)
    return chain_edges(SeamEdges(first_hour, last_hour).add(hourly), matching)


def compare(result, observed_hourly, consecutive=None):
    """Set the seams of a ChainResult beside observed ones: observed_hourly (D, 24, ny, nx), the observed days as an ensemble of one
    member; consecutive: None, or D - 1 bools, which neighbouring days really follow each other (the others get NaN).  Adds
    result.observed (D - 1,), the observed seam per boundary, and result.observed_within (D,), the observed step between the hours
    11 and 12 of each day -- what one hour's change costs where no midnight lies between -- in mm/h per valid pixel.  -> a new
    ChainResult"""
    if not isinstance(result, ChainResult):
        raise ValueError("result: expected a ChainResult")
    shape = tuple(int(v) for v in getattr(observed_hourly, "shape", ()))
    D = len(result.path)
    if len(shape) != 4 or shape[0] != D or shape[2:] != tuple(result.plane_shape):
        raise ValueError(f"observed_hourly: expected shape ({D}, 24, {result.plane_shape[0]}, {result.plane_shape[1]}), got {shape}")
    if consecutive is not None:
        consecutive = np.asarray(consecutive)
        if consecutive.shape != (D - 1,) or consecutive.dtype != np.bool_:
            raise ValueError(f"consecutive: expected {D - 1} bools, got {consecutive.dtype} of shape {consecutive.shape}")
    seam = SeamEdges(result.first_hour, result.last_hour).add(observed_hourly)
    c, nv = seam_costs(seam)
    within = SeamEdges(first_hour=YARDSTICK_HOURS[1], last_hour=YARDSTICK_HOURS[0], device=seam.device).add(observed_hourly)
    cw, nw = seam_costs(within, shift=0)
    observed = _per_pixel(c.view(-1).cpu().numpy(), nv.cpu().numpy())
    if consecutive is not None:
        observed = np.where(consecutive, observed, np.nan)
    return replace(result, observed=observed, observed_within=_per_pixel(cw.view(-1).cpu().numpy(), nw.cpu().numpy()))


def chain_field(gen, daily, n_scenarios, scenario_chunk=16, first_hour=0, last_hour=23, overlap=4, latent_mode="shared", seed=None,
                latent=None, chunk=1024, norm_scale=W.NORM_SCALE, matching="greedy"):
    """Disaggregate the daily maps (D, ny, nx), D >= 2, into n_scenarios scenarios and chain them without holding the hourly
    ensemble: the scenario stream of field._stream_scenarios with SeamEdges.add as the sink, which keeps two hours of every day.
    -> ChainResult.  The latent array is drawn once for all scenarios, exactly as field.disaggregate draws it for the same seed,
    latent and numpy RNG state, so member s of day d -- order[d][s'] names it -- is reproduced by disaggregate with the same seed or
    latent (row s of it), and the series themselves by reorder() on that output.  The generator's fp32 output depends in its last
    bits on the batch of tiles it runs in, so against chain(disaggregate(...all scenarios...)[0]) the integers are equal when the
    batches are the same (`chunk` at most one unit's wet tiles, or one scenario chunk), as _hourly.evaluate_field says.  matching: as
    for chain_edges."""
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    first_hour, last_hour = check_hour(first_hour, "first_hour"), check_hour(last_hour, "last_hour")
    check_matching(matching)
    req = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    if req[1] or req[2] < 2:
        raise ValueError("daily: chaining needs daily maps (D, ny, nx) of at least 2 days")
    if req[2] > MAX_DAYS or req[3] * req[4] > MAX_PLANE:
        raise ValueError(f"daily: at most {MAX_DAYS} days of {MAX_PLANE} pixels")
    edges = SeamEdges(first_hour, last_hour)
    F._stream_scenarios(gen, req, req[0], S, step, edges.add, overlap, latent_mode, seed, latent, chunk, norm_scale)
    return chain_edges(edges, matching)
