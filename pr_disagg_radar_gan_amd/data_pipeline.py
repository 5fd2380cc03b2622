"""Device-side input pipeline: the radar array lives in HBM (288 GB per MI355X hold the
reference's 8-year, hourly data set), tiles are gathered and normalised by a HIP kernel straight into the
tensors the training step consumes.  Replaces, for the hot loop, the reference's view_as_windows fancy-index
gather from a disk memmap, its per-sample Python divide loop and the multiprocessing queues
(gan_train_cwgangp_pixelnorm.py:143-193, :440-449), and compute_valid_indices.py's numba scan.

The array itself can be built on the device from raw radar frames: radar_lut /
hourly_from_radar_codes / DeviceDataset.from_radar_codes replace convert_smhi_radardata.py:38-44, reformat_data.py:72-91 and
revision1/additional_inputs/reformat_data_make_timelist.py:56-62; the float32 array never exists on the host."""
import ctypes
import pickle

import numpy as np
import torch

from . import _lib
from . import weights as W
from ._dev import ptr as _p
from .engine import require_gpu


FRAMES_PER_HOUR = (1, 2, 3, 4, 6, 12)          # what rdgan_data_radar_hourly accepts; SMHI: 12 (5-minute frames)
CHUNK_BYTES = 256 << 20                        # default size of one staged range of days of a host code array


def radar_lut(scale=0.4, offset=-30.0, missing=255, a=200.0, b=1.5, minutes=5):
    """float32[256]: radar code -> mm per frame, convert_smhi_radardata.py:38-44 in the reference's operation order and in float32
    (xarray's where() promotes the uint8 codes to float32): NaN at `missing`, dbz = code * scale + offset, mm/h =
    (10 ** (dbz / 10) / a) ** (1 / b), times minutes / 60.  Host only."""
    f = np.float32
    v = np.arange(256, dtype=np.uint8).astype(np.float32)
    if missing is not None:
        v[int(missing)] = np.nan                                       # res.where(res != 255)
    dbz = v * f(scale) + f(offset)                                      # res * 0.4 - 30
    mmperh = ((f(10) ** (dbz / f(10))) / f(a)) ** f(1 / b)              # ((10 ** (dbz / 10)) / 200) ** (1 / 1.5)
    return (mmperh * f(minutes) / f(60)).astype(np.float32)             # mmperh * 5/60


def day_of_year(dates):
    """one datetime.date or numpy.datetime64[D] per day -> int64 day of year, 1..366 (pandas dayofyear,
    reformat_data_make_timelist.py:58-60)"""
    d = np.asarray(dates, dtype="datetime64[D]")
    if d.ndim != 1:
        raise ValueError("dates must be a sequence with one date per day")
    return (d - d.astype("datetime64[Y]")).astype(np.int64) + 1


def _codes_as_days(codes, frames_per_hour):
    """(n_days, 24 fph, ny, nx) view of a code array given in either accepted shape; ValueError otherwise (reformat_data.py:83-84
    asserts a whole number of days)"""
    fph = int(frames_per_hour)
    if fph not in FRAMES_PER_HOUR:
        raise ValueError(f"frames_per_hour must be one of {FRAMES_PER_HOUR}")
    is_t = isinstance(codes, torch.Tensor)
    if not is_t and not isinstance(codes, np.ndarray):
        raise ValueError("codes must be a uint8 numpy array / memmap or a uint8 device tensor")
    if codes.dtype != (torch.uint8 if is_t else np.uint8):
        raise ValueError("codes must be uint8 radar codes")
    fpd = 24 * fph
    if codes.ndim == 3:
        if codes.shape[0] == 0 or codes.shape[0] % fpd:
            raise ValueError(f"{codes.shape[0]} frames are not a whole number of days of {fpd} frames")
        codes = codes.reshape((codes.shape[0] // fpd, fpd) + tuple(codes.shape[1:]))
    elif codes.ndim != 4 or codes.shape[1] != fpd or codes.shape[0] == 0:
        raise ValueError(f"codes must have shape (n_days, {fpd}, ny, nx) or (n_days * {fpd}, ny, nx)")
    if codes.shape[2] < 1 or codes.shape[3] < 1:
        raise ValueError("empty frames")
    return codes, fph


def hourly_from_radar_codes(codes, frames_per_hour=12, lut=None, chunk_days=None, device=None):
    """uint8 radar codes -> (hourly (n_days, 24, ny, nx), daily (n_days, ny, nx), n_missing): float32 device tensors and the number
    of NaN pixel-hours.  codes: numpy array / memmap (n_days, 24 fph, ny, nx) or (n_days 24 fph, ny, nx), or a contiguous device
    tensor of either shape.  A host array is streamed in ranges of chunk_days whole days through two pinned buffers: the upload of
    range k + 1 runs on a side stream beside the kernel of range k, ordered by events; the only full-size device allocations are
    the two outputs."""
    codes, fph = _codes_as_days(codes, frames_per_hour)
    require_gpu()
    lib = _lib.load()
    on_device = isinstance(codes, torch.Tensor)
    if on_device:
        if not codes.is_cuda or not codes.is_contiguous():
            raise ValueError("a tensor of codes must be a contiguous device tensor")
        dev = codes.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lut = radar_lut() if lut is None else np.ascontiguousarray(lut, dtype=np.float32)
    if lut.shape != (256,):
        raise ValueError("lut must hold 256 values")
    n_days, fpd, ny, nx = (int(v) for v in codes.shape)
    day_bytes = fpd * ny * nx
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        lut_d = torch.from_numpy(lut).to(dev)
        hourly = torch.empty((n_days, 24, ny, nx), dtype=torch.float32, device=dev)
        daily = torch.empty((n_days, ny, nx), dtype=torch.float32, device=dev)
        missing = torch.zeros(1, dtype=torch.int64, device=dev)

        def run(src, d0, n):
            rc = lib.rdgan_data_radar_hourly(_p(src), _p(lut_d), n, fph, ny, nx, _p(hourly[d0:]), _p(daily[d0:]), _p(missing),
                                             ctypes.c_void_p(main.cuda_stream))
            _lib.check(rc, None, "rdgan_data_radar_hourly")

        if on_device:
            run(codes, 0, n_days)
        else:
            cd = max(1, CHUNK_BYTES // day_bytes) if chunk_days is None else int(chunk_days)
            if cd < 1:
                raise ValueError("chunk_days must be at least 1")
            cd = min(cd, n_days)
            side = torch.cuda.Stream(dev)
            pinned = [torch.empty(cd * day_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            staged = [torch.empty(cd * day_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
            uploaded = [torch.cuda.Event() for _ in range(2)]      # the copy out of pinned[b] into staged[b] has finished
            consumed = [torch.cuda.Event() for _ in range(2)]      # the kernel that read staged[b] has finished
            for k, d0 in enumerate(range(0, n_days, cd)):
                b, n = k & 1, min(cd, n_days - d0)
                if k >= 2:
                    uploaded[b].synchronize()                      # (host waits for ONE earlier copy, not for the device)
                np.copyto(pinned[b].numpy()[:n * day_bytes], np.asarray(codes[d0:d0 + n]).reshape(-1))
                if k >= 2:
                    side.wait_event(consumed[b])
                with torch.cuda.stream(side):
                    staged[b][:n * day_bytes].copy_(pinned[b][:n * day_bytes], non_blocking=True)
                    uploaded[b].record(side)
                main.wait_event(uploaded[b])
                run(staged[b], d0, n)
                consumed[b].record(main)
        n_missing = int(missing.item())                            # (waits for the stream: the staging buffers are done with)
    return hourly, daily, n_missing


def write_npy(path, data, chunk_days=16):
    """The reference's `{start}-{end}_tres1.npy` (reformat_data.py:91): a float32 .npy that np.load(mmap_mode='r') opens, written
    in ranges of days so that no second full copy is held.  data: device / host tensor or array (n_days, 24, ny, nx)."""
    path = str(path)
    if not path.endswith(".npy"):
        path += ".npy"                                             # (np.save appends it too)
    out = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=tuple(int(v) for v in data.shape))
    for d0 in range(0, data.shape[0], chunk_days):
        part = data[d0:d0 + chunk_days]
        out[d0:d0 + chunk_days] = part.cpu().numpy() if isinstance(part, torch.Tensor) else part
    out.flush()
    del out
    return path


def save_valid_indices(path, indices):
    """The reference's valid-index file (compute_valid_indices.py:99): a pickled list of (tidx, yidx, xidx) tuples."""
    with open(str(path), "wb") as f:
        pickle.dump([(int(t), int(y), int(x)) for t, y, x in indices], f)
    return str(path)


class DeviceDataset:
    def __init__(self, data, indices=None, ndomain=16, norm_scale=W.NORM_SCALE, device=None):
        """data: float32 array (n_days, 24, ny, nx) (numpy / memmap); indices: (n_samples, 3) (tidx, yidx, xidx)."""
        require_gpu()
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if data.ndim != 4 or data.shape[1] != W.NHOURS or data.dtype != np.float32:
            raise ValueError("data must be float32 with shape (n_days, 24, ny, nx)")       # reference :131-138
        self.n_days, _, self.ny, self.nx = data.shape
        self.ndomain, self.norm_scale = int(ndomain), float(norm_scale)
        self.data = torch.from_numpy(np.ascontiguousarray(data)).to(self.device)
        self.daily = None                  # (n_days, ny, nx) daily sums: from_radar_codes / ensure_daily
        self.timelist = None               # day of year per day: from_radar_codes(dates=...)
        self.n_missing = None
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.indices = None
        self.extra = None
        if indices is not None:
            self.set_indices(indices)

    @classmethod
    def from_radar_codes(cls, codes, dates=None, ndomain=16, frames_per_hour=12, norm_scale=W.NORM_SCALE, lut=None, chunk_days=None,
                         device=None):
        """The data set straight from uint8 radar codes (hourly_from_radar_codes): `data` is the hourly tensor, the daily plane is
        kept for valid_indices, no float32 host copy exists at any point.  dates: one datetime.date / numpy.datetime64[D] per day ->
        self.timelist, the day of year set_extra_condition('doy') then uses by default."""
        codes, _ = _codes_as_days(codes, frames_per_hour)
        timelist = None
        if dates is not None:
            timelist = day_of_year(dates)
            if timelist.shape != (codes.shape[0],):
                raise ValueError("dates must hold one date per day of the codes")
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.data, self.daily, self.n_missing = hourly_from_radar_codes(codes, frames_per_hour, lut, chunk_days, device)
        self.device = self.data.device
        self.n_days, _, self.ny, self.nx = self.data.shape
        self.ndomain, self.norm_scale = int(ndomain), float(norm_scale)
        self.timelist = timelist
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.indices = None
        self.extra = None
        return self

    def ensure_daily(self):
        """Build the daily-sum plane (np.sum(data[t], axis=0), sequential over the hours) if the data set has none: valid_indices
        then reads 1 float per pixel of a box instead of 24."""
        if self.daily is None:
            daily = torch.empty((self.n_days, self.ny, self.nx), dtype=torch.float32, device=self.device)
            rc = self.lib.rdgan_data_daily_sum(_p(self.data), self.n_days, self.ny, self.nx, _p(daily), self._stream())
            _lib.check(rc, None, "rdgan_data_daily_sum")
            self.daily = daily
        return self.daily

    def daily_plane(self):
        """The (n_days, ny, nx) daily sums on the device (built on first use): what field.disaggregate takes without a host copy."""
        return self.ensure_daily()

    def save_npy(self, path):
        """write self.data as the reference's `{start}-{end}_tres1.npy` (write_npy)"""
        return write_npy(path, self.data)

    save_valid_indices = staticmethod(save_valid_indices)

    def set_extra_condition(self, kind, timelist=None, min_lonidx=0, max_lonidx=1):
        """Extra condition channels of the revision-1 variants, appended behind the daily sum by gather():
        'lon' -> (xidx - min_lonidx) / max_lonidx (…_lon.py:175-184); 'doy' -> sin, cos of 2 pi doy / 365 with
        doy = timelist[tidx] (…_doy.py:173-186; timelist defaults to the dates given to from_radar_codes); None -> the one-channel
        condition."""
        if kind is None:
            self.extra = None
        elif kind == 'lon':
            self.extra = ('lon', float(min_lonidx), float(max_lonidx))
        elif kind == 'doy':
            tl = np.asarray(self.timelist if timelist is None else timelist, dtype=np.float64)
            if tl.shape != (self.n_days,):
                raise ValueError("timelist must hold one day-of-year value per day of the data array")
            self.extra = ('doy', torch.from_numpy(tl).to(self.device))
        else:
            raise ValueError("extra condition kind must be None, 'lon' or 'doy'")

    @property
    def n_cond_channels(self):
        return 1 if self.extra is None else (2 if self.extra[0] == 'lon' else 3)

    def _extra_channels(self, sel, cond):
        nd = self.ndomain
        if self.extra[0] == 'lon':
            vals = [(sel[:, 2].double() - self.extra[1]) / self.extra[2]]
        else:
            ang = 2 * np.pi * self.extra[1][sel[:, 0].long()] / 365
            vals = [torch.sin(ang), torch.cos(ang)]
        planes = [v.float().view(-1, 1, 1, 1).expand(-1, nd, nd, 1) for v in vals]
        return torch.cat([cond] + planes, dim=-1).contiguous()

    def set_indices(self, indices):
        """(n_samples, 3) rows (tidx, yidx, xidx) of tile origins, checked here because the gather kernel does not: every tile must lie
        inside the array (yidx <= ny - ndomain, xidx <= nx - ndomain), no component negative, at least one row.  ValueError otherwise,
        before anything is uploaded."""
        raw = np.asarray(indices)
        if raw.ndim != 2 or raw.shape[1] != 3:
            raise ValueError("indices must have shape (n_samples, 3)")
        if raw.shape[0] == 0:
            raise ValueError("indices are empty: no tile to sample from")
        if raw.min() < 0:                  # (checked before the cast to int32: the gather would read in front of the array)
            raise ValueError("negative index: tidx, yidx and xidx count from 0")
        if raw[:, 0].max() >= self.n_days or raw[:, 1].max() + self.ndomain > self.ny or raw[:, 2].max() + self.ndomain > self.nx:
            raise ValueError("index outside the data array")
        idx = np.ascontiguousarray(raw, dtype=np.int32)
        self.indices = torch.from_numpy(idx).to(self.device)
        self.n_samples = idx.shape[0]

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def gather(self, ixs, with_batch=True):
        """tiles at self.indices[ixs] -> (fractions (n,24,nd,nd,1) or None, cond (n,nd,nd,n_cond_channels)) device tensors"""
        ixs = torch.as_tensor(ixs, dtype=torch.long, device=self.device)
        sel = self.indices[ixs].contiguous()
        n, nd = sel.shape[0], self.ndomain
        batch = torch.empty((n, W.NHOURS, nd, nd, 1), dtype=torch.float32, device=self.device) if with_batch else None
        cond = torch.empty((n, nd, nd, 1), dtype=torch.float32, device=self.device)
        rc = self.lib.rdgan_data_gather(_p(self.data), self.n_days, self.ny, self.nx, _p(sel), n, nd, self.norm_scale,
                                        _p(batch if with_batch else None), _p(cond), _p(self.flags), self._stream())
        _lib.check(rc, None, "rdgan_data_gather")
        if self.extra is not None:
            cond = self._extra_channels(sel, cond)
        return batch, cond

    def check_flags(self):
        """The reference's asserts (T:169-172), checked once per call site instead of per batch element.  The flag word on the device
        accumulates over every gather since the last check (rdgan_data_gather only ORs into it; it starts at zero): this reads it,
        clears it on the device, then raises AssertionError if a bit was set -- so one check after several sample_real / sample_latent
        calls covers all of them, and the check after a raise starts from a clean word."""
        f = int(self.flags.item())
        if f:
            self.flags.zero_()
        if f & 1:
            raise AssertionError("NaN/Inf in gathered batch or condition (daily sum of zero or missing data)")
        if f & 2:
            raise AssertionError("hourly fraction outside [0, 1]")

    def sample_real(self, n_batch):
        """generate_real_samples (T:143-174): random valid tiles -> [fractions, normalised daily sums]"""
        ixs = np.random.randint(self.n_samples, size=n_batch)
        return self.gather(ixs, True)

    def sample_latent(self, n_batch, latent_dim=W.LATENT_DIM):
        """generate_latent_points (T:177-193): latent noise and the conditions of random real tiles"""
        latent = torch.from_numpy(np.random.normal(size=(n_batch, latent_dim)).astype(np.float32)).to(self.device)
        ixs = np.random.randint(0, self.n_samples, size=n_batch)
        _, cond = self.gather(ixs, False)
        return latent, cond

    def valid_indices(self, stride=16, tp_thresh_daily=5, n_thresh=20):
        """compute_valid_indices.py:74-92 -> list of (tidx, ii, jj) in the reference's order"""
        nd = self.ndomain
        nbi, nbj = len(range(0, self.ny - nd, stride)), len(range(0, self.nx - nd, stride))
        if nbi < 1 or nbj < 1:
            return []
        valid = torch.empty((self.n_days, nbi, nbj), dtype=torch.int32, device=self.device)
        if self.n_days * nbi * nbj > 0xFFFFFF:
            self.ensure_daily()            # more boxes than one launch of the per-box kernel holds
        if self.daily is not None:         # the box test on the daily plane: same verdicts, 1/24 of the bytes per box
            rc = self.lib.rdgan_data_valid_tiles_daily(_p(self.daily), self.n_days, self.ny, self.nx, nd, int(stride),
                                                       float(tp_thresh_daily), int(n_thresh), _p(valid), self._stream())
            _lib.check(rc, None, "rdgan_data_valid_tiles_daily")
        else:
            rc = self.lib.rdgan_data_valid_tiles(_p(self.data), self.n_days, self.ny, self.nx, nd, int(stride),
                                                 float(tp_thresh_daily), int(n_thresh), _p(valid), self._stream())
            _lib.check(rc, None, "rdgan_data_valid_tiles")
        t, i, j = np.nonzero(valid.cpu().numpy())
        return [(int(a), int(b) * stride, int(c) * stride) for a, b, c in zip(t, i, j)]
