"""The yardstick of the SAL tests: the definitions of DESIGN.md section 28 restated in numpy and plain Python, no scipy.  The labels
are cells_np.label_plane's; the integer records are int64 sums checked against Python ints; V, r and S, A, L are fp64, the objects
summed one after the other in ascending canonical label.  The reference project has no such code."""
import math

import numpy as np

from tests import cells_np as cn

UNIT, MAX_DEPTH = 1024, 2048


def mass(v):
    """q of finite fp32 values: rint(clamp(v, 0, 2048 - 1/1024) * 1024) in fp32, half to even -> int64"""
    v = np.asarray(v, np.float32)
    hi = np.float32(MAX_DEPTH) - np.float32(1.0) / np.float32(UNIT)
    return np.rint(np.clip(v, np.float32(0), hi) * np.float32(UNIT)).astype(np.int64)


def plane_record(v, thresholds, connectivity=8):
    """v (ny, nx) fp32 -> ((n_bad, M0, Mx, My), [(n_objects, n_wet, R)] * T, [(V, r)] * T), Python ints and floats"""
    v = np.asarray(v, np.float32)
    ny, nx = v.shape
    fin = np.isfinite(v)
    q = np.where(fin, mass(np.where(fin, v, np.float32(0))), 0)
    yy, xx = np.indices((ny, nx))
    M0, Mx, My = int(q.sum()), int((q * xx).sum()), int((q * yy).sum())
    assert M0 == sum(int(a) for a in q.ravel()) or ny * nx > 4096           # (the int64 sums against Python ints on small planes)
    objs, vrs = [], []
    for thr in np.asarray(thresholds, np.float64).astype(np.float32):
        with np.errstate(invalid="ignore"):
            wet = fin & (v > thr)
        if not wet.any():
            objs.append((0, 0, 0))
            vrs.append((0.0, 0.0))
            continue
        lab = cn.label_plane(wet, connectivity)
        names, inv = np.unique(lab[wet], return_inverse=True)               # ascending canonical label
        n = len(names)
        Rn, Rmax, Sx, Sy = (np.zeros(n, np.int64) for _ in range(4))
        np.add.at(Rn, inv, q[wet])
        np.maximum.at(Rmax, inv, q[wet])
        np.add.at(Sx, inv, (q * xx)[wet])
        np.add.at(Sy, inv, (q * yy)[wet])
        R = int(Rn.sum())
        sv = sr = 0.0
        for k in range(n):
            if Rn[k] == 0:
                continue
            rn = float(int(Rn[k]))
            sv += rn * (rn / float(int(Rmax[k])))
            sr += rn * math.hypot(float(int(Sx[k])) / rn - float(Mx) / float(M0), float(int(Sy[k])) / rn - float(My) / float(M0))
        objs.append((n, int(wet.sum()), R))
        vrs.append((sv / float(R), sr / float(R)) if R else (0.0, 0.0))
    return (int((~fin).sum()), M0, Mx, My), objs, vrs


def records_np(x, thresholds, connectivity=8):
    """x (..., 24, ny, nx) -> dict(plane (..., 24, 4) int64, objects (..., 24, T, 3) int64, vr (..., 24, T, 2) float64)"""
    p = cn.planes_of(x)
    T = len(thresholds)
    plane, objects, vr = np.zeros((len(p), 4), np.int64), np.zeros((len(p), T, 3), np.int64), np.zeros((len(p), T, 2), np.float64)
    for i, v in enumerate(p):
        plane[i], objects[i], vr[i] = plane_record(v, thresholds, connectivity)
    lead = np.shape(x)[:-2]
    return dict(plane=plane.reshape(lead + (4,)), objects=objects.reshape(lead + (T, 3)), vr=vr.reshape(lead + (T, 2)))


def sal_pair(m, o, ny, nx):
    """one pair of plane records at one threshold, each (n_bad, M0, Mx, My, n_objects, V, r) -> (S, A, L1, L2, L, mask_mismatch),
    in plain Python floats, NaN where a denominator is 0"""
    nan = float("nan")
    d = math.sqrt(ny * ny + nx * nx)
    nbm, M0m, Mxm, Mym, nom, Vm, rm = m
    nbo, M0o, Mxo, Myo, noo, Vo, ro = o
    nvm, nvo = ny * nx - nbm, ny * nx - nbo
    if nvm == 0 or nvo == 0:
        A = nan
    else:
        Dm, Do = M0m / nvm, M0o / nvo
        A = 2.0 * (Dm - Do) / (Dm + Do) if Dm + Do != 0 else nan
    L1 = math.hypot(Mxm / M0m - Mxo / M0o, Mym / M0m - Myo / M0o) / d if M0m and M0o else nan
    if nom and noo:
        S = 2.0 * (Vm - Vo) / (Vm + Vo) if Vm + Vo != 0 else nan
        L2 = 2.0 * abs(rm - ro) / d
    else:
        S = L2 = nan
    return S, A, L1, L2, L1 + L2, nbm != nbo
