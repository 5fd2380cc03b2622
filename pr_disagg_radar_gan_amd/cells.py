"""Rain cells of hourly fields (csrc/rdgan_cells.hip.h): threshold an hour, take the connected wet areas
("cells") and look at how many there are, how large they are, how much water they carry and how that changes over the day -- the
object-based diagnostic that sees speckle, cells cut or fused along tile seams, and a missing tail of large cells.

A plane is one (day, hour) map; a pixel is wet at threshold t when x > thr[t] in fp32, bad when it is NaN or +-inf (never wet).
A cell is a maximal set of wet pixels of one plane connected under 4- or 8-connectivity; cells never link across hours.  A
CellStructure accumulates, over any number of add() calls, the integer state include/rdgan.h lists for rdgan_cells_accumulate;
the array is read on the device and never copied to the host, and the state does not depend on how the planes were split into
calls or on planes_per_pass.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, whole_number
from ._hourly import MAX_PLANE, NHOURS, HourlyAccumulator, admit, check_out_tensor, div as _div, evaluate_field, tv as _tv
from .engine import require_gpu
from .verification import check_event_thresholds

N_COUNTS = 317                                                               # RD_CL_NC: counters per threshold
N_BINS = 25                                                                  # RD_CL_NBINS: floor(log2(area)) = 0 .. 24
N_KPP = 65                                                                   # RD_CL_NKP: cells_per_plane[0 .. 64], the last bin open
MAX_PASS = 65535                                                             # RD_CL_MAXPASS
VOLUME_UNIT = 2.0 ** -16                                                     # a volume counts 2^-16 of the data's unit
# offsets of a threshold's counters (RD_CL_WET ..)
_WET, _CELLS, _HIST, _ASUM, _ASQ, _VBA, _KPP, _LARGEST, _DRY, _ABA = 0, 24, 72, 122, 124, 126, 176, 241, 266, 267
_DEFAULT_PASS_PIXELS = 1 << 24                                               # 256 MB of workspace at most by default


def check_connectivity(connectivity):
    if whole_number(connectivity, 4, 8, "connectivity") not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def check_planes_per_pass(planes_per_pass):
    return None if planes_per_pass is None else whole_number(planes_per_pass, 1, MAX_PASS, "planes_per_pass, unless None,")


def split_state(counts, n_thresholds):
    """the flat state of rdgan_cells_accumulate (numpy) -> dict of named int64 arrays"""
    T = n_thresholds
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (T * N_COUNTS + 2,):
        raise ValueError(f"expected {T * N_COUNTS + 2} counts, got {c.shape}")
    per = c[:T * N_COUNTS].reshape(T, N_COUNTS)
    return dict(wet_pixels=per[:, _WET:_CELLS].copy(), cells=per[:, _CELLS:_HIST].reshape(T, 2, NHOURS).copy(),
                area_hist=per[:, _HIST:_ASUM].reshape(T, 2, N_BINS).copy(), area_sum=per[:, _ASUM:_ASQ].copy(),
                area_sq_sum=per[:, _ASQ:_VBA].copy(), volume_by_area=per[:, _VBA:_KPP].reshape(T, 2, N_BINS).copy(),
                cells_per_plane=per[:, _KPP:_LARGEST].copy(), largest_area=per[:, _LARGEST:_DRY].copy(), dry_planes=per[:, _DRY].copy(),
                area_by_area=per[:, _ABA:].reshape(T, 2, N_BINS).copy(),
                n_planes=int(c[-2]), n_bad_pixels=int(c[-1]))


@dataclass
class CellStats:
    """What CellStructure.result returns, numpy on the host, int64; T thresholds, edge class c = 1 for a cell the rim of the plane
    or a bad pixel cuts off, area bin b = floor(log2(area)).  wet_pixels (T, 24); cells (T, 2, 24) = [c][hour]; area_hist,
    volume_by_area, area_by_area (T, 2, 25) = [c][b]; area_sum, area_sq_sum (T, 2); cells_per_plane (T, 65), the last bin open; largest_area
    (T, 25); dry_planes (T,).  n_pixels is the size of a plane."""
    thresholds: tuple
    connectivity: int
    n_pixels: int
    n_planes: int
    n_bad_pixels: int
    wet_pixels: np.ndarray
    cells: np.ndarray
    area_hist: np.ndarray
    area_sum: np.ndarray
    area_sq_sum: np.ndarray
    volume_by_area: np.ndarray
    cells_per_plane: np.ndarray
    largest_area: np.ndarray
    dry_planes: np.ndarray
    area_by_area: np.ndarray

    def _by_class(self, a, interior_only):
        return a[:, 0] if interior_only else a.sum(axis=1)

    def cell_count_by_hour(self, interior_only=False):
        """(T, 24): cells in the planes of hour h"""
        return self._by_class(self.cells, interior_only)

    def mean_cells_per_plane(self):
        """(T,): NaN without a plane"""
        return _div(self.cells.sum(axis=(1, 2)), self.n_planes)

    def cells_per_plane_distribution(self):
        """(T, 65): the share of planes with k cells, the last bin 64 or more"""
        return _div(self.cells_per_plane, self.cells_per_plane.sum(axis=1, keepdims=True))

    def area_distribution(self, interior_only=False):
        """(T, 25): the share of cells with floor(log2(area)) = b; interior_only leaves out the cells that are cut off"""
        h = self._by_class(self.area_hist, interior_only)
        return _div(h, h.sum(axis=1, keepdims=True))

    def mean_area(self, interior_only=False):
        """(T,): pixels per cell, NaN without a cell"""
        return _div(self._by_class(self.area_sum, interior_only), self._by_class(self.area_hist, interior_only).sum(axis=-1))

    def area_weighted_mean_area(self, interior_only=False):
        """(T,): the area of the cell a wet pixel lies in, averaged over the wet pixels: area_sq_sum / area_sum"""
        return _div(self._by_class(self.area_sq_sum, interior_only), self._by_class(self.area_sum, interior_only))

    def speckle_fraction(self):
        """(T,): the share of wet pixels that are single-pixel cells"""
        return _div(self.area_hist[:, :, 0].sum(axis=1), self.area_sum.sum(axis=1))

    def mean_intensity_by_area(self, interior_only=False):
        """(T, 25): the mean amount per pixel, in the unit of the data, of the cells of area bin b: volume_by_area over
        area_by_area; NaN for a bin without a cell"""
        return _div(self._by_class(self.volume_by_area, interior_only) * VOLUME_UNIT, self._by_class(self.area_by_area, interior_only))

    def largest_cell_distribution(self):
        """(T, 26): the share of planes whose largest cell falls in bin b, the last entry the planes without a cell"""
        a = np.concatenate([self.largest_area, self.dry_planes[:, None]], axis=1)
        return _div(a, a.sum(axis=1, keepdims=True))

    def wet_fraction_by_hour(self):
        """(T, 24): wet pixels of hour h over all its pixels, the bad ones included; NaN without a plane.  Planes come in whole
        days, so every hour has n_planes / 24 of them."""
        return _div(self.wet_pixels, self.n_planes // NHOURS * self.n_pixels)


def compare(a, b):
    """Two CellStats with the same thresholds and connectivity (real days against generated days) -> dict, per threshold: the
    total-variation distances of the area, cells-per-plane and largest-cell distributions (tv_area, tv_area_interior,
    tv_cells_per_plane, tv_largest_cell, each (T,)); and the differences a - b of mean cells per plane, mean area, area-weighted
    mean area and speckle fraction (T,), and of the wet fraction by hour (T, 24)"""
    if not (isinstance(a, CellStats) and isinstance(b, CellStats)):
        raise ValueError("compare takes two CellStats")
    if tuple(a.thresholds) != tuple(b.thresholds):
        raise ValueError(f"the two statistics have different thresholds: {a.thresholds} and {b.thresholds}")
    if a.connectivity != b.connectivity:
        raise ValueError(f"the two statistics have different connectivities: {a.connectivity} and {b.connectivity}")
    return dict(thresholds=tuple(a.thresholds),
                tv_area=_tv(a.area_distribution(), b.area_distribution()),
                tv_area_interior=_tv(a.area_distribution(True), b.area_distribution(True)),
                tv_cells_per_plane=_tv(a.cells_per_plane_distribution(), b.cells_per_plane_distribution()),
                tv_largest_cell=_tv(a.largest_cell_distribution(), b.largest_cell_distribution()),
                mean_cells_per_plane=a.mean_cells_per_plane() - b.mean_cells_per_plane(), mean_area=a.mean_area() - b.mean_area(),
                area_weighted_mean_area=a.area_weighted_mean_area() - b.area_weighted_mean_area(),
                speckle_fraction=a.speckle_fraction() - b.speckle_fraction(),
                wet_fraction_by_hour=a.wet_fraction_by_hour() - b.wet_fraction_by_hour())


def stats_from_state(counts, thresholds, connectivity, n_pixels):
    """the flat state (numpy) -> CellStats"""
    thr = check_event_thresholds(thresholds)
    return CellStats(thresholds=tuple(float(t) for t in thr), connectivity=check_connectivity(connectivity), n_pixels=int(n_pixels),
                     **split_state(counts, len(thr)))


class LabelAccumulator(HourlyAccumulator):
    """An accumulator whose add() can also write the canonical labels at one of its thresholds (cells, storms)"""
    out_name = "labels_out"

    def add(self, hourly, labels_out=None, label_threshold=0):
        """hourly (..., 24, ny, nx) float32: a CUDA tensor or a numpy array, admitted as HourlyAccumulator.add admits it.  The
        plane shape is fixed by the first call.  labels_out: None, or a contiguous int32 CUDA tensor of hourly's shape that
        receives the canonical labels at thresholds[label_threshold].  Returns self."""
        return super().add(hourly, labels_out, label_threshold)

    def _check_args(self, shape, n, labels_out, label_threshold):
        label_threshold = whole_number(label_threshold, 0, len(self.thr) - 1, "label_threshold")
        check_out_tensor(labels_out, self.out_name, torch.int32, shape)
        return (label_threshold,)

    def _state_tensors(self, device):
        self.counts = torch.zeros(len(self.thr) * self.n_counts + 2, dtype=torch.int64, device=device)


class CellStructure(LabelAccumulator):
    """The state of a cell evaluation on the device.  thresholds: the wet-pixel events in the unit of the data; connectivity: 4
    (edges) or 8 (edges and corners); planes_per_pass: how many (day, hour) planes the workspace holds at a time, 16 bytes per
    pixel -- None: up to 2^24 pixels, 256 MB.  The result does not depend on it.  state(): counts (T * 317 + 2,) int64."""
    entry, workspace_entry, n_counts = "rdgan_cells_accumulate", "rdgan_cells_workspace_bytes", N_COUNTS

    def __init__(self, thresholds, connectivity=8, planes_per_pass=None):
        self.thr = check_event_thresholds(thresholds)
        self.connectivity = check_connectivity(connectivity)
        self.planes_per_pass = check_planes_per_pass(planes_per_pass)
        self.reset()

    def _check_plane(self, ny, nx, what):
        if ny * nx > MAX_PLANE:
            raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")

    def _pass_units(self, n, ny, nx):
        per_pass = self.planes_per_pass or max(1, _DEFAULT_PASS_PIXELS // (ny * nx))
        return min(per_pass, n * NHOURS, MAX_PASS)

    def _entry_args(self, ny, nx, labels_out, label_threshold):
        return ny, nx, _hp(self.thr), len(self.thr), self.connectivity, _p(self.counts), _p(labels_out), label_threshold

    def result(self):
        """-> CellStats"""
        return stats_from_state(self.state().cpu().numpy(), self.thr, self.connectivity, self.plane_shape[0] * self.plane_shape[1])


def cell_structure(hourly, thresholds, connectivity=8, planes_per_pass=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> CellStats"""
    return CellStructure(thresholds, connectivity, planes_per_pass).add(hourly).result()


def label_cells(hourly, threshold, connectivity=8):
    """The canonical labels of the cells of hourly (..., 24, ny, nx; a float32 CUDA tensor or numpy) at one threshold: an int32
    CUDA tensor of the same shape, every pixel of a cell holding the smallest flat index y nx + x of the cell, -1 elsewhere"""
    cs = CellStructure((threshold,), connectivity)
    hourly, from_host, shape, _, _ = admit(hourly)
    require_gpu()
    labels = torch.empty(shape, dtype=torch.int32, device="cuda" if from_host else hourly.device)
    cs.add(hourly, labels_out=labels)
    return labels


def cell_structure_field(gen, daily, n_scenarios, thresholds, connectivity=8, planes_per_pass=None, scenario_chunk=16, overlap=4,
                         latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their cells without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a CellStructure.  -> CellStats"""
    return evaluate_field(CellStructure(thresholds, connectivity, planes_per_pass), gen, daily, n_scenarios, scenario_chunk, overlap,
                          latent_mode, seed, latent, chunk, norm_scale)
