"""Random-cascade baseline (csrc/rdgan_cascade.hip.h): the microcanonical multiplicative random cascade every
temporal-disaggregation paper is measured against (Olsson 1998; Guentner et al. 2001; Mueller & Haberlandt 2015 for the three-way
first split of a 24-hour day).  It learns from observed hourly data how a wet box of rain splits into its parts -- all in one part,
or x/(1-x) -- given the box's position in a wet spell and its volume, and applies those splits recursively to a daily sum:
24 h -> 3 x 8 h -> 4 h -> 2 h -> 1 h.  Unlike the analog baseline it copies no observed day, and unlike RainFARM it knows nothing of
space: each pixel (or each patch x patch block of pixels, see `patch`) is disaggregated on its own.

Everything is an integer: depths are counted in 1 / 1024 mm, the calibration is a table of counts, the model a table of 24-bit
cumulative thresholds built from it with Python ints, and a generated hour is units * 2^-10, exact in fp32.  A pixel's 24 generated
hours therefore sum to rint(cond * 1024) / 1024 -- the one difference from the other baselines, whose hours sum to cond.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
import numpy as np
import torch

from . import _lib
from ._dev import device_f32, flag, host_ptr, ptr as _p, stream as _stream, whole_number
from .analog import gather_tiles
from ._hourly import MAX_ELEMS, MAX_PLANE, NHOURS, UNIT, HourlyAccumulator, admit, to_state_device
from .engine import require_gpu
from .ensemble import crps_ensemble_device

NB = 32                                                                      # RD_CS_NB: weight bins
NP = 4                                                                       # RD_CS_NP: position classes
NL = 3                                                                       # RD_CS_NL: binary levels, boxes of 8, 4 and 2 hours
NT = 3                                                                       # RD_CS_NT: 0/1, 1/0, x/(1-x)
MAX_EDGES = 7                                                                # RD_CS_MAXE
PER_CLASS = 748                                                              # RD_CS_PER_CLASS: counters per volume class
TAIL = 3                                                                     # RD_CS_TAIL: n_days, n_bad, n_dry
MAX_EDGE = 1 << 21                                                           # RD_CS_MAXEDGE
MAX_QUERIES = 1 << 18                                                        # RD_CS_MAXQ
MAX_MEMBERS = 65535                                                          # RD_CS_MAXS
MAX_COND = 16384                                                             # RD_CS_MAXCOND
STREAM_CASCADE = 10                                                          # RD_STREAM_CASCADE
DEFAULT_EDGES = (0.1, 1.0)
ONE = 1 << 24
POSITIONS = ("isolated", "starting", "enclosed", "ending")
TYPES = ("0/1", "1/0", "x/(1-x)")


def state_size(n_edges):
    return PER_CLASS * (n_edges + 1) + TAIL


def offsets(NV):
    """where the tables start in the flat state and in the model table (include/rdgan.h)"""
    return {"type": 0, "weight": 36 * NV, "pattern": 420 * NV, "w2": 428 * NV, "w3a": 684 * NV, "w3b": 716 * NV, "tail": 748 * NV}


def check_edges(edges):
    """edges in mm/h -> (the edges as floats, their integer thresholds per hour rint(e * 1024)): at most 7, finite, and strictly
    increasing in 1 .. 2^21 as integers"""
    if isinstance(edges, (str, bytes)) or not hasattr(edges, "__iter__"):
        raise ValueError(f"edges: expected a list of numbers, got {edges!r}")
    edges = list(edges)
    if len(edges) > MAX_EDGES:
        raise ValueError(f"edges: at most {MAX_EDGES}, got {len(edges)}")
    units = []
    for e in edges:
        if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not np.isfinite(e):
            raise ValueError(f"edges: expected finite numbers, got {e!r}")
        u = int(np.rint(np.float64(e) * UNIT))
        if not 1 <= u <= MAX_EDGE or (units and u <= units[-1]):
            raise ValueError(f"edges: expected strictly increasing values in 1/1024 .. 2048 mm/h, got {edges!r}")
        units.append(u)
    return tuple(float(e) for e in edges), np.array(units, dtype=np.int32)


def _check_plane(ny, nx, what):
    if ny * nx > MAX_PLANE:
        raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the model: exact integer arithmetic on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _cumulative(counts):
    total, cum, out = sum(counts), 0, []
    for c in counts:
        cum += c
        out.append((cum << 24) // total)
    return out


def _pooled(rows):
    return [sum(col) for col in zip(*rows)]


def thresholds_from_state(state, n_edges):
    """the flat state (748 NV + 3 integers) -> the model table (748 NV,) uint32: every row as 24-bit cumulative thresholds c[j] =
    (cum[j] << 24) // total, the last one 2^24, in Python ints.  An empty row falls back to (1) the row pooled over the position
    classes, (2) pooled over the volume classes as well, (3) a fixed rule: x/(1-x) for a type row, bin 16 for a weight row, pattern 7
    for the day (whose rows have no position class: step 1 is step 2 there).  ValueError for a state without a wet pixel-day."""
    NV = n_edges + 1
    off = offsets(NV)
    s = [int(v) for v in np.asarray(state).ravel()]
    if len(s) != state_size(n_edges):
        raise ValueError(f"state: {n_edges} edges give {state_size(n_edges)} words, got {len(s)}")
    if min(s) < 0:
        raise ValueError("state: a count is negative")
    if sum(s[off["pattern"]:off["w2"]]) == 0:
        raise ValueError("state: no wet pixel-day has been counted; a cascade cannot be calibrated on it")
    table = [0] * (PER_CLASS * NV)

    def put(at, chain):
        row = next(r for r in chain if sum(r) > 0)
        table[at:at + len(row)] = _cumulative(row)

    hot = lambda n, j: [int(i == j) for i in range(n)]
    for name, width, fixed in (("type", NT, hot(NT, 2)), ("weight", NB, hot(NB, NB // 2))):
        at = lambda L, pos, v: off[name] + ((L * NP + pos) * NV + v) * width
        row = lambda L, pos, v: s[at(L, pos, v):at(L, pos, v) + width]
        for L in range(NL):
            over_all = _pooled([row(L, p, w) for p in range(NP) for w in range(NV)])
            for v in range(NV):
                over_pos = _pooled([row(L, p, v) for p in range(NP)])
                for pos in range(NP):
                    put(at(L, pos, v), (row(L, pos, v), over_pos, over_all, fixed))
    for name, width, per_class, fixed in (("pattern", 8, 1, hot(8, 7)), ("w2", NB, 8, hot(NB, NB // 2)), ("w3a", NB, 1, hot(NB, NB // 2)),
                                          ("w3b", NB, 1, hot(NB, NB // 2))):
        at = lambda v, k: off[name] + (v * per_class + k) * width
        row = lambda v, k: s[at(v, k):at(v, k) + width]
        for k in range(per_class):
            over_all = _pooled([row(w, k) for w in range(NV)])
            for v in range(NV):
                put(at(v, k), (row(v, k), over_all, fixed))
    return np.array(table, dtype=np.uint32)


class CascadeModel:
    """A calibrated cascade: the state it was counted from (host, int64), the edges of its volume classes in mm/h, and the table of
    thresholds, uploaded to a device at the first generate.  Build one with calibrate(), CascadeCalibrator.result(),
    CascadeModel.from_dataset() or CascadeModel.load()."""

    def __init__(self, state, edges=DEFAULT_EDGES):
        self.edges, self.edge_units = check_edges(edges)
        self.state = np.array(state, dtype=np.int64).ravel()
        self.table = thresholds_from_state(self.state, len(self.edges))
        self._device_table = None

    n_classes = property(lambda self: len(self.edges) + 1)
    n_days = property(lambda self: int(self.state[-3]))
    n_bad = property(lambda self: int(self.state[-2]))
    n_dry = property(lambda self: int(self.state[-1]))

    @classmethod
    def from_dataset(cls, dataset, n=None, edges=DEFAULT_EDGES):
        """The valid tiles of a DeviceDataset as the calibration set, as AnalogLibrary.from_dataset takes them: all of them, or n
        drawn with np.random.randint(n_samples, size=n).  Overlapping tiles count their shared pixels once per tile."""
        check_edges(edges)
        if getattr(dataset, "indices", None) is None:
            raise ValueError("dataset has no valid-tile indices (set_indices)")
        if n is None:
            ixs = np.arange(dataset.n_samples)
        else:
            ixs = np.random.randint(dataset.n_samples, size=whole_number(n, 1, 1 << 40, "n, unless None,"))
        cal = CascadeCalibrator(edges)
        for i in range(0, len(ixs), 1 << 16):                                # (the gathered tiles of a chunk are held at once)
            cal.add(gather_tiles(dataset, ixs[i:i + (1 << 16)])[0])
        return cal.result()

    def save(self, path):
        """np.savez of the state and the edges"""
        np.savez(path, state=self.state, edges=np.array(self.edges, dtype=np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            return cls(f["state"], tuple(float(e) for e in f["edges"]))

    def probabilities(self):
        """the tables as probabilities, float64, for inspection and plots: "type" (3, 4, NV, 3) by level (boxes of 8, 4, 2 h),
        position (POSITIONS), volume class and type (TYPES); "weight" (3, 4, NV, 32) over the bins of x; "pattern" (NV, 8) over the
        wet masks of the thirds; "w2" (NV, 8, 32), "w3a" and "w3b" (NV, 32) over the bins of the day's splits"""
        NV = self.n_classes
        off = offsets(NV)
        t = self.table.astype(np.float64) / ONE
        cut = lambda name, end, shape: np.diff(t[off[name]:off[end]].reshape(shape), axis=-1, prepend=0.0)
        return {"type": cut("type", "weight", (NL, NP, NV, NT)), "weight": cut("weight", "pattern", (NL, NP, NV, NB)),
                "pattern": cut("pattern", "w2", (NV, 8)), "w2": cut("w2", "w3a", (NV, 8, NB)), "w3a": cut("w3a", "w3b", (NV, NB)),
                "w3b": cut("w3b", "tail", (NV, NB))}

    def _check_cond(self, cond):
        shape = tuple(int(v) for v in getattr(cond, "shape", ()))
        if isinstance(cond, torch.Tensor) and not cond.is_cuda:
            raise ValueError("cond: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"cond: expected shape (Q, ny, nx) with no empty axis, got {shape}")
        if shape[0] > MAX_QUERIES:
            raise ValueError(f"cond: at most {MAX_QUERIES} queries per call, got {shape[0]}")
        _check_plane(shape[1], shape[2], "cond")
        return shape

    def generate(self, cond, n_members, seed=0, first_member=0, first_query=0, patch=1, return_units=False, out=None):
        """cond (Q, ny, nx) daily sums in mm, numpy or CUDA -> (Q, S, 24, ny, nx) float32 CUDA tensor, S = n_members hourly days per
        query in mm/h.  The 24 hours of a pixel sum to rint(cond * 1024) / 1024, not to cond: the cascade splits whole units of
        1 / 1024 mm.  A pixel that is NaN, +-inf, negative or >= 16384 mm is masked: 24 NaNs.  Member first_member + m of query
        first_query + i depends on (seed, member, query) only, not on how members or queries are split into calls.  patch: the
        pixels of a patch x patch block, anchored at (0, 0), share their draws -- 1: every pixel on its own, the classic per-gauge
        cascade (salt-and-pepper fields); >= max(ny, nx): one set of draws for the tile, so wet and dry hours are coherent while the
        amounts follow each pixel's volume class.  return_units: also the hours as int32 in 1 / 1024 mm (-1 where masked).  out:
        None, or a contiguous float32 CUDA tensor (Q, S, 24, ny, nx) to write into."""
        S = whole_number(n_members, 1, MAX_MEMBERS, "n_members")
        seed = whole_number(seed, 0, (1 << 64) - 1, "seed")
        first_member = whole_number(first_member, 0, 1 << 62, "first_member")
        patch = whole_number(patch, 1, MAX_PLANE, "patch")
        return_units = flag(return_units, "return_units")
        Q, ny, nx = self._check_cond(cond)
        first_query = whole_number(first_query, 0, (1 << 32) - Q, "first_query")
        if Q * S * NHOURS * ny * nx > MAX_ELEMS:
            raise ValueError(f"{Q} queries of {S} members hold more than {MAX_ELEMS} values; split the call")
        shape = (Q, S, NHOURS, ny, nx)
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                    and tuple(out.shape) == shape):
            raise ValueError(f"out: expected a contiguous float32 CUDA tensor of shape {shape}")
        require_gpu()
        lib = _lib.load()
        cond = device_f32(cond, "cond", out.device if out is not None else None)
        dev = cond.device
        if out is not None and out.device != dev:
            raise ValueError(f"cond lies on {dev}, out on {out.device}")
        if self._device_table is None or self._device_table.device != dev:
            self._device_table = torch.from_numpy(self.table.astype(np.int32)).to(dev)                     # (thresholds <= 2^24)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        units = torch.empty(shape, dtype=torch.int32, device=dev) if return_units else None
        with torch.cuda.device(dev):
            rc = lib.rdgan_cascade_generate(_p(self._device_table), host_ptr(self.edge_units), len(self.edges), _p(cond), Q, first_query, ny,
                                            nx, S, first_member, seed, patch, _p(out), _p(units), _stream(out))
        _lib.check(rc, None, "rdgan_cascade_generate")
        return (out, units) if return_units else out


class CascadeCalibrator(HourlyAccumulator):
    """The counts of a cascade calibration on the device.  edges: the edges of the volume classes in mm/h (at most 7; the class of a
    box is the number of edges its mean intensity reaches); device: where a numpy input goes (None: "cuda"; a tensor input fixes
    it).  add() grows the state call by call; it does not depend on how the days are grouped into calls.  state(): (748 NV + 3,)
    int64 in the flat order of include/rdgan.h.  The entry needs no workspace."""
    entry = "rdgan_cascade_accumulate"

    def __init__(self, edges=DEFAULT_EDGES, device=None):
        self.edges, self.edge_units = check_edges(edges)
        self.device = device
        self.reset()

    def _state_tensors(self, device):
        self.counts = torch.zeros(state_size(len(self.edges)), dtype=torch.int64, device=device)

    def _check_plane(self, ny, nx, what):
        _check_plane(ny, nx, what)

    def add(self, hourly):
        """hourly (..., 24, ny, nx) float32 in mm/h: a CUDA tensor or a numpy array, admitted as HourlyAccumulator.add admits it.
        The plane shape is fixed by the first call.  Returns self."""
        hourly, from_host, shape, n, stride = admit(hourly, self.plane_shape)
        ny, nx = shape[-2:]
        self._check_plane(ny, nx, "hourly")
        if n * NHOURS * ny * nx > MAX_ELEMS:
            raise ValueError(f"hourly: at most {MAX_ELEMS} values per call, got {n * NHOURS * ny * nx}")
        if self.counts is None:
            self._start((self.device or "cuda") if from_host else hourly.device)
        device = self.counts.device
        hourly = to_state_device(hourly, from_host, device)
        self.plane_shape = shape[-2:]
        with torch.cuda.device(device):
            rc = getattr(self.lib, self.entry)(_p(hourly), n, stride, ny, nx, host_ptr(self.edge_units), len(self.edges), _p(self.counts),
                                               _stream(self.counts))
        _lib.check(rc, None, self.entry)
        return self

    def result(self):
        """-> CascadeModel (ValueError while no wet pixel-day has been counted)"""
        return CascadeModel(self.state().cpu().numpy(), self.edges)


def calibrate(hourly, edges=DEFAULT_EDGES):
    """One call for an array that is held: hourly (..., 24, ny, nx), numpy or CUDA -> CascadeModel"""
    return CascadeCalibrator(edges).add(hourly).result()


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry points the other baselines have
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_days(real, model):
    if not isinstance(model, CascadeModel):
        raise ValueError("model: expected a CascadeModel")
    shape = tuple(int(v) for v in getattr(real, "shape", ()))
    if len(shape) != 4 or shape[1] != NHOURS or min(shape) < 1:
        raise ValueError(f"real: expected shape (n, {NHOURS}, ny, nx) with n >= 1, got {shape}")
    if isinstance(real, torch.Tensor) and not real.is_cuda:
        raise ValueError("real: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
    _check_plane(shape[2], shape[3], "real")
    return shape[0]


def generate_one_per_day(real, model, seed=0, patch=1):
    """One cascade day per real day from its daily sum, as rainfarm.generate_one_per_day: real (n, 24, ny, nx) mm/h, numpy or CUDA
    -> (n, 24, ny, nx) CUDA tensor, the layout spectral.lsd_evaluation takes.  The condition is the day's own hourly sum; member 0
    of query i."""
    _check_days(real, model)
    whole_number(seed, 0, (1 << 64) - 1, "seed")
    whole_number(patch, 1, MAX_PLANE, "patch")
    real = device_f32(real, "real")
    return model.generate(real.sum(1), 1, seed=seed, patch=patch)[:, 0]


def crps_for_days(real, model, n_members=1000, seed=0, patch=1):
    """rainfarm.crps_for_day for n days at once: n_members cascade days from each real day's daily sum, their CRPS against the real
    hourly fields per grid point (mm/h: no scale), the area mean per hour.  real (n, 24, ny, nx) -> numpy (n, 24)."""
    n = _check_days(real, model)
    whole_number(n_members, 1, MAX_MEMBERS, "n_members")
    whole_number(seed, 0, (1 << 64) - 1, "seed")
    whole_number(patch, 1, MAX_PLANE, "patch")
    real = device_f32(real, "real")
    ens = model.generate(real.sum(1), n_members, seed=seed, patch=patch)
    crps = torch.stack([crps_ensemble_device(ens[i], real[i]) for i in range(n)])
    return crps.mean(dim=(2, 3)).cpu().numpy()
