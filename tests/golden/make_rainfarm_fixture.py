"""Generates tests/golden/rainfarm_reference.npz by executing the reference's own RainFARM functions.

    python tests/golden/make_rainfarm_fixture.py /path/to/reference/rainfarm/rainfarm_temporal_downscaling.py

The reference module uses `np.complex`, which numpy removed in 1.24, so this parses it with `ast`, keeps only the definitions
named in KEEP and executes them against a copy of the numpy namespace that also has `complex = complex` (the builtin the alias
stood for).  Nothing of the reference's text is stored in this repository: the .npz holds the inputs, the seeds and what those
functions returned for them.

Calibration batches (nd 8 and 16): days made by the reference's own downscale_spatiotemporal from known slopes, so that the batch
has a non-trivial spectrum (white noise would give slopes near 0), from smooth daily sums with dry pixels (all-dry pixel series),
with a few hour planes set to 0 (all-dry hours).  They are stored as float32 and the reference's estimate_alpha / estimate_beta are
evaluated on their float64 copies.  Generation cases (nd 8 and 16): (precip, alpha, beta, seed) -> the reference's day after
np.random.seed(seed), stored as float32; beta below and above 1 (the branch of the negative frequencies), dry pixels in precip.
"""
import ast
import os
import sys
import types
import warnings

import numpy as np

KEEP = ("_log_slope", "estimate_beta", "estimate_alpha", "downscale_spatiotemporal")
SEED = 20261016
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rainfarm_reference.npz")
CALIB = {8: (16, 2.5, 1.3), 16: (8, 3.0, 1.6)}        # nd: (samples, alpha, beta) of the days in the batch
GEN = [(8, 1.5, 0.7, 11), (8, 2.2, 1.6, 12), (16, 1.9, 0.8, 13), (16, 1.4, 1.45, 14), (16, 2.6, 2.3, 15)]


def load_reference_functions(path):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in KEEP]
    if sorted(d.name for d in defs) != sorted(KEEP):
        raise SystemExit(f"{path}: expected definitions {KEEP}, found {[d.name for d in defs]}")
    npx = types.ModuleType("numpy")
    npx.__dict__.update(np.__dict__)
    npx.complex = complex
    ns = {"np": npx, "warnings": warnings}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def daily_sums(rng, nd, n):
    p = rng.gamma(0.6, 12.0, (n, nd, nd))
    p[rng.random(p.shape) < 0.25] = 0.0
    return p.astype(np.float32)


def smooth_sums(rng, nd, n):
    """n smooth daily sums (a Gaussian blob, dry below 3 mm): the spatial spectrum of the days then comes from the generator
    rather than from pixel-to-pixel noise in the sums, which flattens it"""
    yy, xx = np.mgrid[0:nd, 0:nd] / nd
    out = []
    for _ in range(n):
        c = rng.random(2)
        w = 0.2 + 0.3 * rng.random()
        f = 30.0 * np.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / w ** 2)
        f[f < 3.0] = 0.0
        out.append(f)
    return np.array(out, dtype=np.float32)


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference_functions(argv[1])
    rng = np.random.default_rng(SEED)
    out = {}
    for nd, (n, alpha, beta) in CALIB.items():
        sums = smooth_sums(rng, nd, n)
        np.random.seed(SEED + nd)
        days = np.array([ref["downscale_spatiotemporal"](s.astype(np.float64), alpha, beta, 24) for s in sums])
        days[0, 5] = 0.0
        days[1, 17:20] = 0.0
        days[2] = 0.0                                      # one sample dry all day
        x = days.astype(np.float32)
        xd = x.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)     # log(0) of the dry series: -inf, filtered by the reference
            a, b = ref["estimate_alpha"](xd), ref["estimate_beta"](xd)
        out[f"calib_nd{nd}"] = x
        out[f"calib_alpha_nd{nd}"] = np.float64(a)
        out[f"calib_beta_nd{nd}"] = np.float64(b)
        print(f"calibration nd {nd}: {n} samples, alpha {a:.6f}, beta {b:.6f}")
    for i, (nd, alpha, beta, seed) in enumerate(GEN):
        precip = daily_sums(rng, nd, 1)[0]
        np.random.seed(seed)
        day = ref["downscale_spatiotemporal"](precip.astype(np.float64), alpha, beta, 24)
        out[f"gen{i}_precip"] = precip
        out[f"gen{i}_params"] = np.array([nd, alpha, beta, seed], dtype=np.float64)
        out[f"gen{i}_day"] = day.astype(np.float32)
        print(f"generation {i}: nd {nd}, alpha {alpha}, beta {beta}, seed {seed}, {int((precip == 0).sum())} dry pixels")
    out["n_gen"] = np.int64(len(GEN))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main(sys.argv)
