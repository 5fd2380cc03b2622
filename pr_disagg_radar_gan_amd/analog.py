"""Analog baseline, the method of fragments (csrc/rdgan_analog.hip.h): "daily sum -> 24 hourly fields" the
way a hydrologist would try first.  Among a library of observed days, find the k whose daily field most resembles the condition,
pick one of them per member, and scale its hourly fractions to the condition's daily amounts.  Unlike the climatological day and
RainFARM, this baseline looks at the condition's spatial pattern.

The search is defined in integers: q = rint(x * 1024) in units of 2^-10 mm; a library pixel-hour is bad when x is NaN, +-inf,
negative or >= 2048; D[p] is the day's sum of q and the feature e[p] = floor(sqrt(D[p])), the square-root transform usual for
rain.  A library day with a bad pixel-hour or no rain at all is void and never a neighbour.  A query pixel that is NaN, +-inf,
negative or >= 2048 * 24 is masked: it adds nothing to a distance and is NaN in every generated hour.  dist(i, j) is the sum of
(e_i - e_j)^2 over the query's unmasked pixels; ties go to the smaller library index.  Library days of the query's own group
(its calendar day, say) are skipped: the leave-one-day-out exclusion an experiment needs whose queries come from the library's own
data set, where overlapping tiles of the same day would leak the answer.

The pick of member m for query i comes from the counter RNG (stream 9) and depends on (seed, member, query) only; weights="rank"
is Lall and Sharma's 1 / rank kernel, "uniform" draws among the neighbours evenly.  The hourly fields are fp32.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
import numpy as np
import torch

from . import _lib
from ._dev import device_f32, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import NHOURS, UNIT, admit, to_state_device
from .engine import require_gpu
from .ensemble import crps_ensemble_device

MAX_PLANE = 4096                                                             # RD_AN_MAXP
MAX_LIBRARY = (1 << 24) - 1                                                  # RD_AN_MAXN
MAX_QUERIES = 1 << 18                                                        # RD_AN_MAXQ
MAX_K = 32                                                                   # RD_AN_MAXK
MAX_MEMBERS = 65535                                                          # RD_AN_MAXS
BLOCK = 64                                                                   # RD_AN_BLOCK: library days of a block
WAVES = 8                                                                    # RD_AN_WAVES: lists a slice writes per query
STREAM_ANALOG = 9                                                            # RD_STREAM_ANALOG
WEIGHTS = {"uniform": 0, "rank": 1}                                          # RD_AN_UNIFORM, RD_AN_RANK
_TARGET_WORKGROUPS = 1024                                                    # of a search by default: four per compute unit


def padded_plane(plane):
    """Ppad: the pixels of a plane rounded up to whole chunks of 8"""
    return (int(plane) + 7) // 8 * 8


def query_tile(plane):
    """the queries a workgroup of the search holds in LDS (rd_an_query_tile)"""
    return 16 if padded_plane(plane) <= 2048 else 8


def check_k(k):
    return whole_number(k, 1, MAX_K, "k")


def check_weights(weights):
    if not isinstance(weights, str) or weights not in WEIGHTS:
        raise ValueError(f"weights must be one of {tuple(WEIGHTS)}, got {weights!r}")
    return WEIGHTS[weights]


def check_workspace_bytes(nbytes):
    return None if nbytes is None else whole_number(nbytes, 1, 1 << 50, "workspace_bytes, unless None,")


def _check_groups(groups, n, what):
    """None, or n whole numbers in the int32 range -> int32 numpy array or CUDA tensor"""
    if groups is None:
        return None
    if isinstance(groups, torch.Tensor):
        if groups.dtype not in (torch.int32, torch.int64) or tuple(groups.shape) != (n,):
            raise ValueError(f"{what}: expected {n} whole numbers, got a {groups.dtype} tensor of shape {tuple(groups.shape)}")
        return groups
    g = np.asarray(groups)
    if g.shape != (n,) or not np.issubdtype(g.dtype, np.integer) or g.dtype == np.bool_:
        raise ValueError(f"{what}: expected {n} whole numbers, got shape {g.shape} of {g.dtype}")
    if n and (g.min() < -(1 << 31) or g.max() >= 1 << 31):
        raise ValueError(f"{what}: a group lies outside the int32 range")
    return g.astype(np.int32)


def _groups_to(groups, device):
    if groups is None:
        return None
    if isinstance(groups, torch.Tensor):
        return groups.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(groups).to(device)


def _check_plane(ny, nx, what):
    if ny * nx > MAX_PLANE:
        raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")


def gather_tiles(dataset, ixs):
    """the raw mm/h tiles (n, 24, nd, nd) of the valid-tile rows ixs, as rainfarm.random_tiles gathers them, and their day indices"""
    nd, dev = dataset.ndomain, dataset.data.device
    ar, hours = torch.arange(nd, device=dev), torch.arange(NHOURS, device=dev)
    idx = dataset.indices[torch.from_numpy(np.asarray(ixs, dtype=np.int64)).to(dev)].long()
    days, ys, xs = idx[:, 0], idx[:, 1:2] + ar, idx[:, 2:3] + ar
    batch = dataset.data[days[:, None, None, None], hours[None, :, None, None], ys[:, None, :, None], xs[:, None, None, :]]
    return batch.contiguous(), days.to(torch.int32)


class AnalogLibrary:
    """The library of an analog search on the device.  hourly (N, 24, ny, nx) float32 in mm/h, a CUDA tensor (kept as it is; the
    leading axis may have any stride >= 24 ny nx) or a numpy array (uploaded to `device`, default "cuda"); ny nx <= 4096 and
    N < 2^24.  groups: None, or N whole numbers -- a library day whose group equals a query's, and is >= 0, is skipped for that
    query.  The features are built once, here; n_void is the number of days that can never be a neighbour."""

    def __init__(self, hourly, groups=None, device=None):
        hourly, from_host, shape, n, stride = admit(hourly)
        ny, nx = shape[-2:]
        _check_plane(ny, nx, "hourly")
        if not 1 <= n <= MAX_LIBRARY:
            raise ValueError(f"hourly: a library holds 1 .. {MAX_LIBRARY} days, got {n}")
        groups = _check_groups(groups, n, "groups")
        require_gpu()
        self.lib = _lib.load()
        dev = torch.device(device or "cuda") if from_host else hourly.device
        self.hourly = to_state_device(hourly, from_host, dev)
        self.n, self.day_stride, self.plane_shape = n, stride, (ny, nx)
        self.device = self.hourly.device
        self.groups = _groups_to(groups, self.device)
        plane = ny * nx
        self.features = torch.empty((n + BLOCK - 1) // BLOCK * BLOCK * padded_plane(plane), dtype=torch.int16, device=self.device)
        self.totals = torch.empty(n, dtype=torch.int64, device=self.device)
        self.void = torch.empty(n, dtype=torch.uint8, device=self.device)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.rdgan_analog_features(_p(self.hourly), n, stride, ny, nx, 1, _p(self.features), _p(None), _p(self.totals),
                                                _p(self.void), _p(count), _stream(self.hourly))
        _lib.check(rc, None, "rdgan_analog_features")
        self.n_void = int(count.item())
        self._ws = None

    @classmethod
    def from_dataset(cls, dataset, n=None):
        """The valid tiles of a DeviceDataset as a library: all of them, or n drawn with np.random.randint(n_samples, size=n) as
        rainfarm.random_tiles draws.  The group of a tile is its day index, so a query of the same calendar day skips it."""
        if getattr(dataset, "indices", None) is None:
            raise ValueError("dataset has no valid-tile indices (set_indices)")
        nd = int(dataset.ndomain)
        _check_plane(nd, nd, "dataset")
        if n is None:
            ixs = np.arange(dataset.n_samples)
        else:
            ixs = np.random.randint(dataset.n_samples, size=whole_number(n, 1, MAX_LIBRARY, "n, unless None,"))
        if len(ixs) > MAX_LIBRARY:
            raise ValueError(f"the data set has {len(ixs)} valid tiles, a library holds {MAX_LIBRARY}")
        tiles, days = gather_tiles(dataset, ixs)
        return cls(tiles, groups=days)

    # ---- queries
    def _admit_cond(self, cond, query_groups):
        """-> (cond as given, Q, query groups checked): host code"""
        shape = tuple(int(v) for v in getattr(cond, "shape", ()))
        if isinstance(cond, torch.Tensor) and not cond.is_cuda:
            raise ValueError("cond: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
        if len(shape) != 3 or shape[1:] != self.plane_shape or shape[0] < 1:
            raise ValueError(f"cond: expected shape (Q, {self.plane_shape[0]}, {self.plane_shape[1]}) with Q >= 1, got {shape}")
        if shape[0] > MAX_QUERIES:
            raise ValueError(f"cond: at most {MAX_QUERIES} queries per call, got {shape[0]}")
        if isinstance(cond, torch.Tensor) and cond.device != self.device:
            raise ValueError(f"cond lies on {cond.device}, the library on {self.device}")
        qg = _check_groups(query_groups, shape[0], "query_groups")
        if qg is not None and self.groups is None:
            raise ValueError("query_groups given, but the library has no groups")
        return shape[0], qg

    def _default_slices(self, Q):
        ny, nx = self.plane_shape
        tiles = -(-Q // query_tile(ny * nx))
        nblocks = -(-self.n // BLOCK)
        return max(1, min(-(-_TARGET_WORKGROUPS // tiles), -(-nblocks // WAVES)))

    def _search(self, cond, Q, k, qg, workspace_nbytes):
        ny, nx = self.plane_shape
        plane, ppad = ny * nx, padded_plane(ny * nx)
        dev = self.device
        qfeat = torch.empty(Q * ppad, dtype=torch.int16, device=dev)
        qmask = torch.empty(Q * ppad, dtype=torch.int16, device=dev)
        neighbours = torch.empty((Q, k), dtype=torch.int32, device=dev)
        distances = torch.empty((Q, k), dtype=torch.int64, device=dev)
        found = torch.empty(Q, dtype=torch.int32, device=dev)
        qg = _groups_to(qg, dev)
        with torch.cuda.device(dev):
            nbytes = workspace_nbytes
            if nbytes is None:
                nbytes = workspace_bytes(self.lib, "rdgan_analog_workspace_bytes", Q, k, self._default_slices(Q))
            nbytes = max(nbytes // 8, 1) * 8
            if self._ws is None or self._ws.numel() * 8 != nbytes:
                self._ws = None
                self._ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            st = _stream(cond)
            rc = self.lib.rdgan_analog_features(_p(cond), Q, plane, ny, nx, 0, _p(qfeat), _p(qmask), _p(None), _p(None), _p(None), st)
            _lib.check(rc, None, "rdgan_analog_features")
            rc = self.lib.rdgan_analog_search(_p(self.features), _p(self.void), _p(self.groups if qg is not None else None), self.n, plane,
                                              _p(qfeat), _p(qmask), _p(qg), Q, k, _p(neighbours), _p(distances), _p(found), _p(self._ws),
                                              nbytes, st)
        _lib.check(rc, None, "rdgan_analog_search")
        return neighbours, distances, found

    def search(self, cond, k=10, query_groups=None, workspace_bytes=None):
        """cond (Q, ny, nx) daily sums in mm, numpy or CUDA -> (neighbours (Q, k) int32, distances (Q, k) int64, found (Q,) int32),
        CUDA tensors: the library indices and integer distances of the k nearest admissible days by ascending (distance, index),
        -1 in the slots behind the `found` admissible ones.  workspace_bytes: None, or the size of the workspace, which fixes into
        how many slices the library is cut (at least 512 k bytes per query); the result does not depend on it."""
        k, nbytes = check_k(k), check_workspace_bytes(workspace_bytes)
        Q, qg = self._admit_cond(cond, query_groups)
        if nbytes is not None and nbytes < Q * WAVES * k * 8:
            raise ValueError(f"workspace_bytes: one slice of {Q} queries needs {Q * WAVES * k * 8} bytes, got {nbytes}")
        return self._search(device_f32(cond, "cond", self.device), Q, k, qg, nbytes)

    def generate(self, cond, n_members, k=10, seed=0, weights="rank", query_groups=None, first_member=0, return_picks=False,
                 first_query=0):
        """cond (Q, ny, nx) -> (Q, S, 24, ny, nx) float32 CUDA tensor, S = n_members hourly days per query in mm/h whose 24 hours
        sum to the condition: member first_member + m of query first_query + i picks one of the query's k nearest library days
        (weights "rank": with probability proportional to 1 / rank; "uniform": evenly) and scales its hourly fractions; where the
        picked day is dry and the condition is not, the day's areal profile stands in.  NaN at masked pixels, and throughout for a
        query without an admissible day.  return_picks: also the picked library indices (Q, S) int32, -1 for none."""
        k, w = check_k(k), check_weights(weights)
        S = whole_number(n_members, 1, MAX_MEMBERS, "n_members")
        seed = whole_number(seed, 0, (1 << 64) - 1, "seed")
        first_member = whole_number(first_member, 0, 1 << 62, "first_member")
        Q, qg = self._admit_cond(cond, query_groups)
        first_query = whole_number(first_query, 0, (1 << 32) - Q, "first_query")
        cond = device_f32(cond, "cond", self.device)
        neighbours, _, found = self._search(cond, Q, k, qg, None)
        ny, nx = self.plane_shape
        out = torch.empty((Q, S, NHOURS, ny, nx), dtype=torch.float32, device=self.device)
        picks = torch.empty((Q, S), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.rdgan_analog_apply(_p(self.hourly), self.n, self.day_stride, ny, nx, _p(cond), Q, first_query, _p(neighbours),
                                             _p(found), k, S, first_member, seed, w, _p(out), _p(picks), _stream(out))
        _lib.check(rc, None, "rdgan_analog_apply")
        return (out, picks) if return_picks else out


def _check_days(real, library, query_groups=None):
    if not isinstance(library, AnalogLibrary):
        raise ValueError("library: expected an AnalogLibrary")
    shape = tuple(int(v) for v in getattr(real, "shape", ()))
    if len(shape) != 4 or shape[1] != NHOURS or shape[2:] != library.plane_shape or shape[0] < 1:
        raise ValueError(f"real: expected shape (n, {NHOURS}, {library.plane_shape[0]}, {library.plane_shape[1]}) with n >= 1, got {shape}")
    if isinstance(real, torch.Tensor) and not real.is_cuda:
        raise ValueError("real: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
    if _check_groups(query_groups, shape[0], "query_groups") is not None and library.groups is None:
        raise ValueError("query_groups given, but the library has no groups")
    return shape[0]


def generate_one_per_day(real, library, k=10, seed=0, weights="rank", query_groups=None):
    """One analog day per real day from its daily sum, as rainfarm.generate_one_per_day: real (n, 24, ny, nx) mm/h, numpy or CUDA
    -> (n, 24, ny, nx) CUDA tensor, the layout spectral.lsd_evaluation takes.  The condition is the day's own hourly sum; member 0
    of query i.  query_groups (n,): the days' groups, to leave the library's tiles of the same day out."""
    _check_days(real, library, query_groups)
    check_k(k), check_weights(weights)
    whole_number(seed, 0, (1 << 64) - 1, "seed")
    real = device_f32(real, "real", library.device)
    return library.generate(real.sum(1), 1, k=k, seed=seed, weights=weights, query_groups=query_groups)[:, 0]


def crps_for_days(real, library, n_members=1000, k=10, seed=0, weights="rank", query_groups=None):
    """rainfarm.crps_for_day for n days at once: n_members analog days from each real day's daily sum, their CRPS against the real
    hourly fields per grid point (mm/h: no scale), the area mean per hour.  real (n, 24, ny, nx) -> numpy (n, 24)."""
    n = _check_days(real, library, query_groups)
    check_k(k), check_weights(weights)
    whole_number(n_members, 1, MAX_MEMBERS, "n_members")
    whole_number(seed, 0, (1 << 64) - 1, "seed")
    real = device_f32(real, "real", library.device)
    ens = library.generate(real.sum(1), n_members, k=k, seed=seed, weights=weights, query_groups=query_groups)
    crps = torch.stack([crps_ensemble_device(ens[i], real[i]) for i in range(n)])
    return crps.mean(dim=(2, 3)).cpu().numpy()
