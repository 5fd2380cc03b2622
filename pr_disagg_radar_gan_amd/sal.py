"""Object-based verification of hourly fields against the observed hours (csrc/rdgan_sal.hip.h): SAL of
Wernli, Paulat, Hagen and Frei (2008) -- per pair of (day, hour) planes the structure S (too peaked < 0 < too flat), the amplitude A
(too dry < 0 < too wet) and the location L = L1 + L2 (the distance of the centres of mass, and the difference in how far the objects
lie from the centre), at fixed thresholds.

The device work is plane_records: the objects of a plane at threshold t are its cells (cells.label_cells has the labels), and per
plane the library returns integers -- n_bad, the mass moments M0, Mx, My of the whole field, and per threshold n_objects, n_wet, R --
and two fp64 values, the weighted scaled volume V and the weighted distance r.  The mass of a valid pixel is its value clamped
into 0 .. 2048 - 1/1024 mm and counted in 1/1024 mm.  Every record of a plane is bitwise the same however the planes are grouped
into passes or calls.  sal_from_records is host code on numpy and needs no GPU.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream, workspace_bytes
from ._hourly import (MAX_MEMBERS, MAX_PLANE, NHOURS, ObservedRequest, admit, check_pair, div, observation_on_device,
                      quantile_summary, summary_differences, to_state_device)
from .cells import MAX_PASS, check_connectivity, check_planes_per_pass
from .engine import require_gpu
from .verification import check_event_thresholds

MAX_MOMENT = 1 << 42                                                         # RD_SAL_MAXMOMENT: max(ny, nx) ny nx stays below it
CHUNK = 4096                                                                 # RD_SAL_CHUNK
_DEFAULT_PASS_PIXELS = 1 << 23                                               # 403 MB of workspace at most by default
COMPONENTS = ("S", "A", "L1", "L2", "L")


def check_plane(ny, nx, what="hourly"):
    """ValueError for a plane the entry refuses: more than 2^24 pixels, or 2^21 max(ny, nx) ny nx >= 2^63 (a moment could wrap)"""
    if ny * nx > MAX_PLANE:
        raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
    if max(ny, nx) * ny * nx >= MAX_MOMENT:
        raise ValueError(f"{what}: a plane of {ny} x {nx} pixels could overflow its 64-bit moments (max(ny, nx) ny nx must stay below 2^42)")


@dataclass
class PlaneRecords:
    """What plane_records returns, for hourly (..., 24, ny, nx) and T thresholds: plane (..., 24, 4) int64 = (n_bad, M0, Mx, My);
    objects (..., 24, T, 3) int64 = (n_objects, n_wet, R); vr (..., 24, T, 2) float64 = (V, r).  Device tensors, or numpy arrays
    after cpu()."""
    plane: object
    objects: object
    vr: object
    ny: int
    nx: int
    thresholds: tuple
    connectivity: int

    def cpu(self):
        """the same records as numpy arrays on the host"""
        host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return PlaneRecords(host(self.plane), host(self.objects), host(self.vr), self.ny, self.nx, self.thresholds, self.connectivity)

    n_bad = property(lambda self: self.plane[..., 0])
    M0 = property(lambda self: self.plane[..., 1])
    Mx = property(lambda self: self.plane[..., 2])
    My = property(lambda self: self.plane[..., 3])
    n_objects = property(lambda self: self.objects[..., 0])
    n_wet = property(lambda self: self.objects[..., 1])
    R = property(lambda self: self.objects[..., 2])
    V = property(lambda self: self.vr[..., 0])
    r = property(lambda self: self.vr[..., 1])


def _check_request(thresholds, connectivity, planes_per_pass):
    return check_event_thresholds(thresholds), check_connectivity(connectivity), check_planes_per_pass(planes_per_pass)


def plane_records(hourly, thresholds, connectivity=8, planes_per_pass=None):
    """The records of every plane of hourly (..., 24, ny, nx) float32: a CUDA tensor, whose leading axis may have any stride (a
    view of a wider buffer; _hourly.tensor_layout has the rule), or a numpy array.  thresholds: the wet-pixel events in the unit
    of the data; connectivity: 4 or 8; planes_per_pass: how many planes the workspace holds at a time, 48 bytes per pixel -- None:
    up to 2^23 pixels.  The records do not depend on it.  -> PlaneRecords on the device"""
    thr, connectivity, planes_per_pass = _check_request(thresholds, connectivity, planes_per_pass)
    hourly, from_host, shape, n, stride = admit(hourly)
    ny, nx = shape[-2:]
    check_plane(ny, nx)
    require_gpu()
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if from_host else hourly.device
    hourly = to_state_device(hourly, from_host, device)
    T, lead = len(thr), shape[:-2]
    per_pass = min(planes_per_pass or max(1, _DEFAULT_PASS_PIXELS // (ny * nx)), n * NHOURS, MAX_PASS)
    with torch.cuda.device(device):
        plane = torch.empty(lead + (4,), dtype=torch.int64, device=device)
        objects = torch.empty(lead + (T, 3), dtype=torch.int64, device=device)
        vr = torch.empty(lead + (T, 2), dtype=torch.float64, device=device)
        nbytes = workspace_bytes(lib, "rdgan_sal_workspace_bytes", ny, nx, per_pass)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        rc = lib.rdgan_sal_records(_p(hourly), n, stride, ny, nx, _hp(thr), T, connectivity, _p(plane), _p(objects), _p(vr), _p(ws),
                                   nbytes, _stream(plane))
    _lib.check(rc, None, "rdgan_sal_records")
    return PlaneRecords(plane, objects, vr, ny, nx, tuple(float(t) for t in thr), connectivity)


@dataclass
class SAL:
    """What sal_from_records returns, numpy on the host: S, A, L1, L2, L float64 and mask_mismatch bool, each of shape
    broadcast(model, obs) + (T,) = (..., 24, T).  NaN where a component is undefined."""
    thresholds: tuple
    connectivity: int
    ny: int
    nx: int
    S: np.ndarray
    A: np.ndarray
    L1: np.ndarray
    L2: np.ndarray
    L: np.ndarray
    mask_mismatch: np.ndarray

    def summary(self):
        """dict: thresholds, and per component c in S, A, L1, L2, L a dict of median, q25, q75, mean_abs, undefined (the share of
        pairs where c is NaN), each (T,) over all pairs, and by_hour (24, T), the median over the pairs of an hour; NaN where
        nothing is defined"""
        out = dict(thresholds=self.thresholds, mask_mismatch=float(np.mean(self.mask_mismatch)))
        for c in COMPONENTS:
            a = getattr(self, c)
            T = a.shape[-1]
            flat, hours = a.reshape(-1, T), np.moveaxis(a, -2, 0).reshape(NHOURS, -1, T)
            out[c] = dict(quantile_summary(flat, 0, mean_abs=True), by_hour=quantile_summary(hours, 1)["median"])
        return out


def sal_from_records(model, obs):
    """SAL of the model planes against the observed ones.  model, obs: PlaneRecords (device or numpy) of the same plane shape,
    thresholds and connectivity, whose leading shapes (..., 24) broadcast (an ensemble (S, D, 24) against (D, 24)).  With
    d = sqrt(ny^2 + nx^2), D = M0 / n_valid, the centre c = (Mx, My) / M0:
        A = 2 (D_m - D_o) / (D_m + D_o)      S = 2 (V_m - V_o) / (V_m + V_o)
        L1 = |c_m - c_o| / d                 L2 = 2 |r_m - r_o| / d              L = L1 + L2
    A component is NaN where a denominator is 0: A when both planes are dry (or one has no valid pixel), L1 when either M0 is 0, S
    and L2 when either plane has no object at that threshold (S also when both V are 0).  mask_mismatch: n_bad differs.  -> SAL"""
    if not (isinstance(model, PlaneRecords) and isinstance(obs, PlaneRecords)):
        raise ValueError("sal_from_records takes two PlaneRecords")
    if (model.ny, model.nx) != (obs.ny, obs.nx):
        raise ValueError(f"the two records have different plane shapes: {(model.ny, model.nx)} and {(obs.ny, obs.nx)}")
    if tuple(model.thresholds) != tuple(obs.thresholds):
        raise ValueError(f"the two records have different thresholds: {model.thresholds} and {obs.thresholds}")
    if model.connectivity != obs.connectivity:
        raise ValueError(f"the two records have different connectivities: {model.connectivity} and {obs.connectivity}")
    m, o = model.cpu(), obs.cpu()
    try:
        lead = np.broadcast_shapes(m.plane.shape[:-1], o.plane.shape[:-1])
    except ValueError:
        raise ValueError(f"the two records do not broadcast: {m.plane.shape[:-1]} and {o.plane.shape[:-1]}") from None
    ny, nx = m.ny, m.nx
    d = np.sqrt(np.float64(ny * ny + nx * nx))
    Dm, Do = div(m.M0, ny * nx - m.n_bad), div(o.M0, ny * nx - o.n_bad)
    A = 2.0 * div(Dm - Do, Dm + Do)
    L1 = np.hypot(div(m.Mx, m.M0) - div(o.Mx, o.M0), div(m.My, m.M0) - div(o.My, o.M0)) / d
    both = (m.n_objects > 0) & (o.n_objects > 0)
    S = np.where(both, 2.0 * div(m.V - o.V, m.V + o.V), np.nan)
    L2 = np.where(both, 2.0 * np.abs(m.r - o.r) / d, np.nan)
    T = len(m.thresholds)
    wide = lambda a: np.broadcast_to(a[..., None], lead + (T,)).copy()
    A, L1 = wide(A), wide(L1)
    return SAL(tuple(m.thresholds), m.connectivity, ny, nx, S=np.broadcast_to(S, lead + (T,)).copy(), A=A, L1=L1,
               L2=np.broadcast_to(L2, lead + (T,)).copy(), L=L1 + L2, mask_mismatch=wide(m.n_bad != o.n_bad))


def compare(a, b):
    """Two SAL (or two of their summaries) with the same thresholds -- two generators against the same observation -> dict: per
    component the differences a - b of median, q25, q75, mean_abs, undefined (T,) and by_hour (24, T)"""
    a, b = (s.summary() if isinstance(s, SAL) else s for s in (a, b))
    if not (isinstance(a, dict) and isinstance(b, dict) and "thresholds" in a and "thresholds" in b):
        raise ValueError("compare takes two SAL or two summaries")
    if tuple(a["thresholds"]) != tuple(b["thresholds"]):
        raise ValueError(f"the two summaries have different thresholds: {a['thresholds']} and {b['thresholds']}")
    return dict(thresholds=tuple(a["thresholds"]), **summary_differences(a, b, COMPONENTS))


def sal_hourly(ens, obs, thresholds, connectivity=8, planes_per_pass=None):
    """One call for an ensemble that is held: ens (S,) + obs.shape, obs (..., 24, ny, nx), each a float32 CUDA tensor or a numpy
    array.  -> SAL of shape (S, ..., 24, T)"""
    thr, connectivity, planes_per_pass = _check_request(thresholds, connectivity, planes_per_pass)
    obs_shape, ens_shape = admit(obs)[2], admit(ens)[2]
    check_pair(ens_shape, obs_shape)
    check_plane(*obs_shape[-2:])
    return sal_from_records(plane_records(ens, thr, connectivity, planes_per_pass).cpu(),
                            plane_records(obs, thr, connectivity, planes_per_pass).cpu())


def sal_field(gen, observed, n_scenarios, thresholds, connectivity=8, planes_per_pass=None, daily=None, scenario_chunk=16, overlap=4,
              latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a day and take the SAL of every scenario against its observed hours without holding the scenarios.  observed
    ([D,] 24, ny, nx): a numpy array, a float32 CUDA tensor or a DeviceDataset; daily: the condition, ([D,] ny, nx), by default the
    sum of the observed hours.  The latent array is drawn once for all n_scenarios (<= 4096) scenarios, exactly as field.disaggregate
    draws it for the same seed, latent and numpy RNG state; disaggregate then runs for scenario_chunk scenarios at a time into one
    reused buffer, and only the records of each chunk are kept.  The result equals sal_hourly(disaggregate(...all scenarios...)[0],
    observed, ...) bit for bit where the hourly values are the same (_hourly.evaluate_field says when they are).
    -> SAL of shape (S, [D,] 24, T)"""
    thr, connectivity, planes_per_pass = _check_request(thresholds, connectivity, planes_per_pass)
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    request = ObservedRequest(gen, observed, daily, lambda shape: check_plane(shape[-2], shape[-1], "observed"), S, overlap, latent_mode,
                              latent, chunk, norm_scale)
    obs = observation_on_device(request.obs, request.from_host)
    obs_rec = plane_records(obs, thr, connectivity, planes_per_pass).cpu()
    parts = []
    request.stream(obs, step, lambda buf: parts.append(plane_records(buf, thr, connectivity, planes_per_pass).cpu()), seed)
    model = PlaneRecords(*(np.concatenate([getattr(p, k) for p in parts], axis=0) for k in ("plane", "objects", "vr")), obs_rec.ny, obs_rec.nx,
                         obs_rec.thresholds, connectivity)
    return sal_from_records(model, obs_rec)
