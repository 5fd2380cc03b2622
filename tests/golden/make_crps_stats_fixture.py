"""Generates tests/golden/crps_stats_reference.npz by executing the reference's own bootstrap function and scipy's t-test.

    python tests/golden/make_crps_stats_fixture.py /path/to/reference/analyze_crps_results.py

The reference script cannot be imported (it loads its pickled results at module level), so this parses it with `ast`, keeps only
the definition of bootstrapped_difference_onesample and executes it against numpy.  The one-sample t-test of the reference is
scipy.stats.ttest_1samp, called here directly.  Nothing of the reference's text is stored in this repository: the .npz holds the
seeded input vectors and what those functions returned for them.

Vectors x0 .. x3: (0) 2 400 differences of two gamma samples (the shape of gan - random for 100 days); (1) 50 values; (2) mean far
above the spread, so the p-value underflows to exactly 0; (3) half-integers symmetric about 0, whose sums are exact: mean 0, t 0,
p 1.  Per vector: t and p of ttest_1samp(x, popmean=0); for x0 and x1 the reference's [mean, lower, upper] after
np.random.seed(BOOT_SEED), N = 10 000, perc = 1.  Grid: one-sided tail scipy.stats.t.sf(t, df) over T_GRID x DF_GRID."""
import ast
import os
import sys

import numpy as np

KEEP = ("bootstrapped_difference_onesample",)
SEED = 20261016
BOOT_SEED = 7
T_GRID = (0.0, 1e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0, 20.0, 37.0)
DF_GRID = (1, 2, 5, 49, 2399, 239999)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crps_stats_reference.npz")


def load_reference_functions(path):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in KEEP]
    if sorted(d.name for d in defs) != sorted(KEEP):
        raise SystemExit(f"{path}: expected definitions {KEEP}, found {[d.name for d in defs]}")
    ns = {"np": np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    from scipy import stats
    ref = load_reference_functions(argv[1])
    rng = np.random.default_rng(SEED)
    xs = [rng.gamma(0.5, 0.2, 2400) - rng.gamma(0.5, 0.23, 2400),
          rng.gamma(0.5, 0.2, 50) - 0.08,
          5.0 + 1e-3 * rng.standard_normal(2400),
          np.arange(-32, 32) + 0.5]
    out = {"n_vectors": len(xs), "boot_seed": BOOT_SEED, "boot_N": 10000, "boot_perc": 1}
    for i, x in enumerate(xs):
        t, p = stats.ttest_1samp(x, popmean=0)
        out[f"x{i}"] = x
        out[f"tp{i}"] = np.array([t, p])
        print(f"x{i}: n {len(x)}, t {t!r}, p {p!r}")
    assert out["tp2"][1] == 0.0 and out["tp3"][0] == 0.0 and out["tp3"][1] == 1.0
    for i in (0, 1):
        np.random.seed(BOOT_SEED)
        out[f"boot{i}"] = ref["bootstrapped_difference_onesample"](xs[i], perc=1, N=10000)
        print(f"boot{i}: {out[f'boot{i}']!r}")
    tt, dd = np.meshgrid(np.array(T_GRID), np.array(DF_GRID, dtype=np.float64), indexing="ij")
    out["grid_t"], out["grid_df"], out["grid_sf"] = tt.ravel(), dd.ravel(), stats.t.sf(tt.ravel(), dd.ravel())
    assert np.all(out["grid_sf"] > 1e-300)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main(sys.argv)
