"""What the evaluations of hourly arrays share on the host: how an array (..., 24, ny, nx) is admitted -- kind, shape, layout --
before any device call, the accumulator the single-array ones are (HourlyAccumulator) with its driver for whole daily fields
(evaluate_field), the base of those that hold members against an observation (ObservedVerifier) with theirs (ObservedRequest), how an ensemble of
whole days is admitted against observed days (admit_ensemble, the joint-field scores and ranks), and the small quotients and
summaries their statistics use."""
import warnings

import numpy as np
import torch

from . import _lib
from . import field as F
from ._dev import device_f32, ptr as _p, stream as _stream, workspace_bytes
from .engine import require_gpu

NHOURS = 24                                                                  # RD_HOURS
UNIT = 1024                                                                  # RD_DEPTH_UNIT: depths are integers in 1 / UNIT mm
MAX_DEPTH = 2048                                                             # RD_DEPTH_MAX: mm an hour, from which a value is bad
MAX_PLANE = 1 << 24                                                          # RD_HOURLY_MAXPLANE: pixels of a plane
MAX_ELEMS = 1 << 40                                                          # RD_HOURLY_MAXELEMS: values of one call's array
MAX_MEMBERS = 4096                                                           # RD_MS_MAXS, RD_VF_MAXS


def hourly_shape(shape, what="hourly"):
    shape = tuple(int(n) for n in shape)
    if len(shape) < 3 or shape[-3] != NHOURS or min(shape) < 1:
        raise ValueError(f"{what}: expected shape (..., 24, ny, nx) with no empty axis, got {shape}")
    return shape


def tensor_layout(shape, strides):
    """(n, day_stride) of a tensor of shape (..., 24, ny, nx) with these strides (in elements), as rdgan_temporal_accumulate reads
    it: the last three axes must be dense, whatever the rank; the leading axes must flatten to one axis of stride day_stride >= 24
    ny nx, which a single leading axis does with any stride (a view of a wider buffer) and several do only when they are dense
    among themselves.  Anything a stride argument cannot express -- a crop, a step, a transposed plane -- is a ValueError."""
    shape, strides = tuple(int(m) for m in shape), tuple(int(st) for st in strides)
    expect = 1
    for m, st in zip(reversed(shape[-3:]), reversed(strides[-3:])):
        if m != 1 and st != expect:
            raise ValueError("hourly: the hour, row and column axes must be contiguous (a crop, a step or a transpose is not)")
        expect *= m
    day = expect
    lead = [(m, st) for m, st in zip(shape[:-3], strides[:-3]) if m != 1]
    n = int(np.prod(shape[:-3], dtype=np.int64))
    if not lead:
        return n, day
    stride = lead[-1][1]
    if stride < day:
        raise ValueError(f"hourly: the leading stride {stride} is below the size of a day {day}")
    expect = stride
    for m, st in reversed(lead):
        if st != expect:
            raise ValueError("hourly: several leading axes must be contiguous among themselves")
        expect *= m
    return n, stride


def member_layout(x):
    """(S, P, member_stride, shape) of x (S, *shape): every axis behind the first must be contiguous, the first may have any stride
    >= P (a view of a wider buffer)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("x: expected a tensor of shape (S, *shape)")
    S, shape = int(x.shape[0]), tuple(int(n) for n in x.shape[1:])
    P = int(np.prod(shape, dtype=np.int64))
    if not 1 <= S <= MAX_MEMBERS:
        raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {S}")
    if P < 1:
        raise ValueError(f"x holds no position: shape {tuple(x.shape)}")
    expect = 1
    for n, st in zip(reversed(shape), reversed(x.stride()[1:])):
        if n != 1 and st != expect:
            raise ValueError("x: the axes behind the member axis must be contiguous")
        expect *= n
    stride = int(x.stride(0)) if S > 1 else P
    if stride < P:
        raise ValueError(f"x: the member stride {stride} is below the number of positions {P}")
    return S, P, stride, shape


def dense_member_layout(members, from_host):
    """members (S, *shape) behind admit_array: a host array becomes dense float32 (member stride P), a tensor stays as it is
    -> (members, S, P, member_stride, shape)"""
    if from_host:
        members = np.ascontiguousarray(members, dtype=np.float32)
    return (members,) + member_layout(torch.from_numpy(members) if from_host else members)


def check_pair(ens_shape, obs_shape, what="ens"):
    """ValueError unless ens_shape is (S,) + obs_shape with 1 .. MAX_MEMBERS members"""
    if len(ens_shape) < 4:
        raise ValueError(f"{what}: expected an array or tensor of shape (S, ..., 24, ny, nx)")
    if not 1 <= int(ens_shape[0]) <= MAX_MEMBERS:
        raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {int(ens_shape[0])}")
    if tuple(ens_shape[1:]) != tuple(obs_shape):
        raise ValueError(f"{what}: expected shape (S,) + {tuple(obs_shape)}, got {tuple(ens_shape)}")


def admit_array(a, what="hourly"):
    """Kind and shape of an hourly input, host code: a float32 CUDA tensor is taken as it is, anything else as a numpy array of
    numbers; a torch tensor on the host is refused.  -> (the tensor or array, from_host, shape)"""
    from_host = not isinstance(a, torch.Tensor)
    if from_host:
        a = np.asarray(a)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what}: expected an array of numbers")
    elif not a.is_cuda:                                # (a host view's strides would not survive the copy to the device)
        raise ValueError(f"{what}: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
    elif a.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32")
    return a, from_host, hourly_shape(a.shape, what)


def admit(hourly, plane_shape=None):
    """admit_array, the plane shape an accumulator has pinned (None: not yet), and the layout the accumulate entries read: a
    numpy array will be uploaded dense, a tensor must pass tensor_layout.  -> (hourly, from_host, shape, n, day_stride)"""
    hourly, from_host, shape = admit_array(hourly)
    if plane_shape is not None and shape[-2:] != tuple(plane_shape):
        raise ValueError(f"hourly: the plane shape is {tuple(plane_shape)} since the first call, got {shape[-2:]}")
    if from_host:
        n, day_stride = int(np.prod(shape[:-3], dtype=np.int64)), NHOURS * shape[-2] * shape[-1]
    else:
        n, day_stride = tensor_layout(shape, hourly.stride())
    return hourly, from_host, shape, n, day_stride


def to_state_device(a, from_host, device, what="hourly"):
    """The step behind admission once the state exists: a host array goes to the state's device as dense float32, a tensor must
    lie there already"""
    if from_host:
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    if a.device != device:
        raise ValueError(f"{what} lies on {a.device}, the state on {device}")
    return a


def observation_on_device(obs, from_host):
    """the first device step of a verification: a host array goes to "cuda" as dense float32, a tensor is used where it lies"""
    require_gpu()
    return to_state_device(obs, True, "cuda") if from_host else obs.detach().contiguous()


def shape_of(a, name):
    """the shape of an input device_f32 will convert: a floating-point CUDA tensor or a numpy array of numbers (admit_array asks more)"""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError(f"{name}: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
        if not a.dtype.is_floating_point:
            raise ValueError(f"{name}: expected floating-point values")
        return tuple(int(v) for v in a.shape)
    a = np.asarray(a)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{name}: expected an array of numbers")
    return tuple(int(v) for v in a.shape)


def check_reals(reals, name="reals"):
    """-> the shape of the observed days (D, 24, ny, nx) that a per-day loop runs over"""
    shape = shape_of(reals, name)
    if len(shape) != 4 or shape[1] != NHOURS or min(shape) < 1:
        raise ValueError(f"{name}: expected shape (D, {NHOURS}, ny, nx) with no empty axis, got {shape}")
    return shape


def admit_ensemble(ens, obs, max_members, max_days, obs_is_a_vector=False):
    """The shapes of an ensemble of whole days against observed days, host code: ens (m, 24, ny, nx) with obs (24, ny, nx) or
    (D, 24, ny, nx) -- one shared ensemble -- or ens (D, m, 24, ny, nx) with obs (D, 24, ny, nx).  obs_is_a_vector: m + 1 vectors and
    the call's members must stay within MAX_ELEMS values (otherwise the entry alone holds the members to it).  -> (m, D, ny, nx, shared)"""
    es, os_ = shape_of(ens, "ens"), shape_of(obs, "obs")
    if len(es) not in (4, 5) or es[-3] != NHOURS or min(es) < 1:
        raise ValueError(f"ens: expected shape (m, {NHOURS}, ny, nx) or (D, m, {NHOURS}, ny, nx) with no empty axis, got {es}")
    if len(os_) not in (3, 4) or min(os_) < 1 or os_[-3:] != es[-3:]:
        raise ValueError(f"obs: expected shape ({NHOURS}, {es[-2]}, {es[-1]}) or (D, {NHOURS}, {es[-2]}, {es[-1]}), got {os_}")
    m, ny, nx = es[-4], es[-2], es[-1]
    D, shared = os_[0] if len(os_) == 4 else 1, len(es) == 4
    if not shared and (len(os_) != 4 or es[0] != D):
        raise ValueError(f"ens holds {es[0]} days, obs must have shape ({es[0]}, {NHOURS}, {ny}, {nx}), got {os_}")
    if m > max_members:
        raise ValueError(f"at most {max_members} members, got {m}")
    if ny * nx > MAX_PLANE:
        raise ValueError(f"a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
    if D > max_days:
        raise ValueError(f"at most {max_days} days per call, got {D}")
    if obs_is_a_vector and max(m + 1, (1 if shared else D) * m) * NHOURS * ny * nx > MAX_ELEMS:
        raise ValueError(f"{m} members of {NHOURS} x {ny} x {nx} values: at most {MAX_ELEMS} values per call")
    return m, D, ny, nx, shared


def ensemble_on_device(ens, obs):
    """the first device step behind admit_ensemble: both as float32 on one device, a numpy array going where the other lies"""
    require_gpu()
    ens = device_f32(ens, "ens", obs.device if isinstance(obs, torch.Tensor) else None)
    obs = device_f32(obs, "obs", ens.device)
    if obs.device != ens.device:
        raise ValueError(f"ens lies on {ens.device}, obs on {obs.device}")
    return ens, obs


def grow_workspace(owner, nbytes, device):
    """-> owner._ws if it holds nbytes, else a new int64 buffer of that size in its place.  It takes the owner, not the buffer: only
    the owner can drop the old buffer before the new one is allocated, so that the two never coexist."""
    if owner._ws is None or owner._ws.numel() * 8 < nbytes:
        owner._ws = None
        owner._ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    return owner._ws


def check_out_tensor(t, name, dtype, shape):
    """an optional output of an accumulate entry: None, or a contiguous CUDA tensor of this dtype and shape"""
    if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                              and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous {str(dtype).split('.')[-1]} CUDA tensor of shape {tuple(shape)}")


class HourlyAccumulator:
    """What the accumulators of hourly arrays share: an integer state `counts` on the device that add() grows call by call, the
    plane shape the first call pins, and one workspace.  A subclass names its two library entries and supplies what differs:

      _state_tensors(device)            allocate the zeroed state: self.counts (temporal: and self.sums)
      _check_plane(ny, nx, what)        ValueError for a plane the evaluation cannot take
      _check_args(shape, n, out, ...)   ValueError for a bad out tensor or extra argument of add; -> the extra arguments, normalised
      _pass_units(n, ny, nx)            how many of the entry's units (planes or days) one pass takes; None where there are no passes
      _workspace_args(n, ny, nx)        the arguments of workspace_entry, (ny, nx, _pass_units) unless overridden
      _entry_args(ny, nx, out, ...)     the arguments of `entry` between (x, n, day_stride) and the workspace
      result()                          the state as statistics on the host

    The workspace only grows, and the entry is told the bytes this call needs, not the size of the buffer: the entries take as many
    units per pass as the bytes they are told hold, so a buffer left larger by an earlier call changes nothing (and the state does
    not depend on the pass size in any case)."""
    entry = workspace_entry = None
    out_name = None                              # how add's optional out tensor is called in messages
    device = None                                # where a numpy input goes (None: "cuda"); a tensor input fixes it

    def reset(self):
        """forget the days added so far (and the plane shape); returns self"""
        self.plane_shape = None
        self.lib = None
        self.counts = self._ws = None
        return self

    def _start(self, device):
        require_gpu()
        self.lib = _lib.load()
        self._state_tensors(device)

    def _check_plane(self, ny, nx, what):
        pass

    def _check_args(self, shape, n, out):
        return ()

    def _pass_units(self, n, ny, nx):
        return None

    def _workspace_args(self, n, ny, nx):
        return ny, nx, self._pass_units(n, ny, nx)

    def add(self, hourly, out=None, *extra):
        """hourly (..., 24, ny, nx) float32: a CUDA tensor, whose leading axis may have any stride >= the size of one of its
        entries (a view of a wider buffer; tensor_layout has the rule, and refuses a crop, a step or a transpose at any rank), or
        a numpy array.  The plane shape is fixed by the first call.  Returns self."""
        hourly, from_host, shape, n, stride = admit(hourly, self.plane_shape)
        ny, nx = shape[-2:]
        self._check_plane(ny, nx, "hourly")
        extra = self._check_args(shape, n, out, *extra)
        if self.counts is None:
            self._start((self.device or "cuda") if from_host else hourly.device)
        device = self.counts.device
        hourly = to_state_device(hourly, from_host, device)
        if out is not None:
            to_state_device(out, False, device, self.out_name)
        self.plane_shape = shape[-2:]
        with torch.cuda.device(device):
            nbytes = workspace_bytes(self.lib, self.workspace_entry, *self._workspace_args(n, ny, nx))
            ws = grow_workspace(self, nbytes, device)
            rc = getattr(self.lib, self.entry)(_p(hourly), n, stride, *self._entry_args(ny, nx, out, *extra), _p(ws), nbytes,
                                               _stream(self.counts))
        _lib.check(rc, None, self.entry)
        return self

    def state(self):
        """the state tensor itself, on the device, in the flat order of include/rdgan.h"""
        if self.counts is None:
            raise ValueError("nothing has been added")
        return self.counts


def evaluate_field(acc, gen, daily, n_scenarios, scenario_chunk, overlap, latent_mode, seed, latent, chunk, norm_scale):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and add them to the accumulator `acc` without holding
    them; -> acc.result().  The latent array is drawn once for all scenarios, exactly as field.disaggregate draws it for the same
    seed, latent and numpy RNG state; disaggregate then runs for scenario_chunk scenarios at a time into one reused buffer and each
    result is added.  The result is the evaluation of the hourly values those disaggregate calls produce.  The generator's fp32
    output depends in its last bits on the batch of tiles it runs in, so against the evaluation of
    disaggregate(...all scenarios...)[0] the integer states are equal (and temporal's sums within the reordering bound) when the
    batches are the same (`chunk` at most one unit's wet tiles, or one scenario chunk); otherwise the two differ as disaggregate's
    own outputs differ between values of `chunk`."""
    S, step = F._check_scenarios(n_scenarios, scenario_chunk)
    req = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    acc._check_plane(req[3], req[4], "daily")
    F._stream_scenarios(gen, req, req[0], S, step, acc.add, overlap, latent_mode, seed, latent, chunk, norm_scale)
    return acc.result()


class ObservedVerifier:
    """What the verifiers of members against an observation share: the observation (..., 24, ny, nx) on the device, and the head of
    add(members).  A subclass calls _admit_obs in its __init__, _admit_members first in its add, and overrides _check_members."""
    _ws = None                                   # the workspace of a subclass that has one (grow_workspace)

    def _admit_obs(self, obs, check_obs=lambda shape: None):
        """sets shape, ny, nx, P, n_days, then runs the subclass's host checks check_obs(shape), and only then the device: obs, lib"""
        obs, from_host, self.shape = admit_array(obs, "obs")
        self.ny, self.nx = self.shape[-2:]
        self.P = int(np.prod(self.shape, dtype=np.int64))
        self.n_days = self.P // (NHOURS * self.ny * self.nx)
        check_obs(self.shape)
        self.obs = observation_on_device(obs, from_host)
        self.lib = _lib.load()

    def _check_members(self, s):
        """ValueError if s more members cannot be taken; host code that must not need the device state"""

    def _admit_members(self, members):
        """the head of add(members): every step before the last, the move to the observation's device, reads self.shape alone (and
        what _check_members reads).  -> (members on the device, s, member_stride)"""
        members, from_host, _ = admit_array(members, "members")
        members, s, P, stride, shape = dense_member_layout(members, from_host)
        if shape != self.shape:
            raise ValueError(f"members: expected shape (s,) + {self.shape}, got {tuple(members.shape)}")
        if s * P > MAX_ELEMS:
            raise ValueError(f"members: more than {MAX_ELEMS} values in one call")
        self._check_members(s)
        return to_state_device(members, from_host, self.obs.device, "members"), s, stride


class ObservedRequest:
    """The host half of a `*_field` verification against the observed hours: every check of `observed`, `daily` and the scenario
    arguments, before any device call.  observed ([D,] 24, ny, nx): a numpy array, a float32 CUDA tensor or a DeviceDataset (its
    hourly tensor and daily plane are used where they lie); daily: the condition ([D,] ny, nx) or None; check_obs(shape): the
    module's own ValueErrors for the observation; S: the scenarios.  Holds obs and from_host, what admit_array made of `observed`."""

    def __init__(self, gen, observed, daily, check_obs, S, overlap, latent_mode, latent, chunk, norm_scale):
        self._dataset = observed if hasattr(observed, "daily_plane") else None
        self.obs, self.from_host, shape = admit_array(observed if self._dataset is None else observed.data, "observed")
        if len(shape) not in (3, 4):
            raise ValueError(f"observed must have shape (24, ny, nx) or (n_days, 24, ny, nx), got {shape}")
        check_obs(shape)
        day_shape = shape[:-3] + shape[-2:]
        if daily is not None and not isinstance(daily, torch.Tensor):
            daily = np.asarray(daily)
        if daily is not None and tuple(daily.shape) != day_shape:
            raise ValueError(f"daily: expected shape {day_shape}, got {tuple(daily.shape)}")
        # the checks of disaggregate on a stand-in of the daily map's shape: nothing has touched the device so far
        self._req = F._check_request(gen, np.broadcast_to(np.float32(0), day_shape), S, overlap, latent_mode, latent, chunk, norm_scale)
        self._daily, self._args = daily, (gen, S, overlap, latent_mode, latent, chunk, norm_scale)

    def stream(self, obs, scenario_chunk, sink, seed):
        """Disaggregate under the device of obs, the observation once it lies there, and hand every chunk of scenarios to sink
        (field._stream_scenarios).  The default daily is the dataset's daily plane, or the sum of the observed hours."""
        gen, S, overlap, latent_mode, latent, chunk, norm_scale = self._args
        with torch.cuda.device(obs.device):
            daily = self._daily
            if daily is None:
                daily = obs.sum(dim=-3) if self._dataset is None else self._dataset.daily_plane()
            F._stream_scenarios(gen, self._req, daily, S, scenario_chunk, sink, overlap, latent_mode, seed, latent, chunk, norm_scale)


def div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.asarray(b) != 0, np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64), np.nan)


def quantile_summary(a, axis, mean_abs=False):
    """dict of median, q25, q75 and undefined (the share of NaN) of a over the pairs along axis -- with mean_abs, the mean of |a|
    too; NaN where nothing is defined"""
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                      # (an all-NaN slice: its quantile is NaN, as wanted)
        q25, med, q75 = np.nanquantile(a, [0.25, 0.5, 0.75], axis=axis)
        out = dict(median=med, q25=q25, q75=q75, undefined=np.mean(np.isnan(a), axis=axis))
        if mean_abs:
            out["mean_abs"] = np.nanmean(np.abs(a), axis=axis)
    return out


def summary_differences(a, b, names):
    """{name: {k: a[name][k] - b[name][k]}} of two summaries, dicts of dicts of arrays"""
    return {name: {k: a[name][k] - b[name][k] for k in a[name]} for name in names}


def tv(a, b):
    with np.errstate(invalid="ignore"):
        return 0.5 * np.abs(a - b).sum(axis=-1)
