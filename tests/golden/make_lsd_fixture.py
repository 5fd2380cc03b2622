"""Generates tests/golden/lsd_reference.npz by executing the reference's own spectrum and distance functions.

    python tests/golden/make_lsd_fixture.py /path/to/reference/log_spectral_distance.py

The reference script cannot be imported (it loads its data files and plots at module level), so this parses it with `ast`,
keeps only the definitions named in KEEP, drops their decorators (the numba JIT, absent here and irrelevant to the result)
and executes them against numpy and scipy.fftpack.  Nothing of the reference's text is stored in this repository: the .npz
holds the seeded input fields and what those functions returned for them.

The fields are stored as float32 (the hourly mm/h fields the evaluation feeds in); the reference is evaluated on their
float64 copies, so that the stored spectra are the exact float64 answer for the stored fp32 inputs.  The distance matrices
follow the pair loop of the reference's compute_dists: every ordered pair i != j, and the diagonal left at 0.
"""
import ast
import os
import sys
import warnings

import numpy as np

KEEP = ("azimuthal_average", "compute_radial_spectrum", "log_spectral_distance")
NDS = (8, 16, 64)
NFIELDS = {8: 32, 16: 32, 64: 20}
SEED = 20261016
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lsd_reference.npz")


def load_reference_functions(path):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in KEEP]
    if sorted(d.name for d in defs) != sorted(KEEP):
        raise SystemExit(f"{path}: expected definitions {KEEP}, found {[d.name for d in defs]}")
    for d in defs:
        d.decorator_list = []
    from scipy import fftpack
    ns = {"np": np, "fftpack": fftpack}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def fields(nd, n, rng):
    """n seeded (nd, nd) float32 precipitation fields: gamma with dry pixels, then the four special cases last."""
    x = rng.gamma(0.5, 1.5, (n, nd, nd))
    x[rng.random(x.shape) < 0.4] = 0.0
    x[-4] = 0.0                                        # all dry
    x[-3] = 0.75                                       # constant
    x[-2] = 0.0
    x[-2, nd // 3, nd // 5] = 2.5                      # single wet pixel
    x[-1] = rng.gamma(2.0, 25.0, (nd, nd)).clip(0.0, 100.0)   # heavy, up to 100 mm/h
    return x.astype(np.float32)


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference_functions(argv[1])
    rng = np.random.default_rng(SEED)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # 0/0 and x/0 of the dry fields: NaN and inf are the result
        for nd in NDS:
            f = fields(nd, NFIELDS[nd], rng)
            spec = np.array([ref["compute_radial_spectrum"](a.astype(np.float64)) for a in f])
            n = len(f)
            mat = np.zeros((n, n))
            for i in range(n):
                for j in range(n):
                    if i != j:
                        mat[i, j] = ref["log_spectral_distance"](spec[i], spec[j])
            out[f"fields_nd{nd}"] = f
            out[f"spectra_nd{nd}"] = spec
            out[f"lsd_nd{nd}"] = mat
            print(f"nd {nd}: {n} fields, K = {spec.shape[1]}, {np.isnan(mat).sum()} NaN / {np.isinf(mat).sum()} inf distances")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main(sys.argv)
