"""Generates tests/golden/ks_pvalues_reference.npz and ks_samples_reference_NN.npz from the RECORDED OUTPUTS of the reference's own
evaluation run (generate_and_evaluate.py:548-585):

    python tests/golden/make_ks_fixture.py /path/to/reference

Under <reference>/plots_generated_wgancp_pixelnorm lie, for 20 pairs of conditions, check_conditional_dist_samenoise_<params>_0020_00NN.csv
(48 000 rows: the hourly area-mean fractions of two ensembles of 1 000 days, float32 printed in shortest form, written at :579) and
check_conditional_dist_samenoise_KSpval<params>_0020_00NN.txt (the 24 p-values scipy.stats.ks_2samp gave the authors, :585).  They
are data the reference's program wrote; nothing of its program text is read or stored here.

ks_pvalues_reference.npz: p (20, 24) float64 as parsed from the text files; h (20, 24), n |D| of scipy.stats.ks_2samp on the recorded
samples (n = m = 1 000, so an integer); asymp_*: for seeded samples of unequal sizes the D and p-value of
scipy.stats.ks_2samp(method='asymp'), and scipy.special.kolmogorov(sqrt(n m / (n + m)) D); csv_head / pval_head: the first lines of
pair 0000's two files, quoted as data for the writers' format tests.
ks_samples_reference_NN.npz, NN in 0000 (ordinary), 0010 (D = 0.008, the largest recorded p), 0016 (the smallest, 2e-54): samples
(2, 1000, 24) float32 and box (2, 24, 12): matplotlib.cbook.boxplot_stats of the float64-cast column in the order n, mean, q1, med,
q3, iqr, whislo, whishi, cilo, cihi, n_fliers_lo, n_fliers_hi."""
import glob
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SUBDIR = "plots_generated_wgancp_pixelnorm"
SAMPLE_PAIRS = (0, 10, 16)
ASYMP_SIZES = ((1000, 1001), (7, 1000), (10000, 16384), (2, 7), (300, 5000), (16384, 1000))
SEED = 20261016


def read_pair(csv_path):
    """-> (2, 1000, 24) float32: [cond - 1][member][hour - 1]"""
    rows = np.loadtxt(csv_path, delimiter=",", skiprows=1, dtype=np.float64)
    assert rows.shape == (48000, 4), rows.shape
    out = np.full((2, 1000, 24), np.nan, np.float32)
    out[rows[:, 2].astype(int) - 1, rows[:, 0].astype(int), rows[:, 3].astype(int) - 1] = rows[:, 1].astype(np.float32)
    assert not np.isnan(out).any()
    return out


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    from matplotlib.cbook import boxplot_stats
    from scipy import special, stats
    d = os.path.join(argv[1], SUBDIR)
    csvs = sorted(f for f in glob.glob(os.path.join(d, "check_conditional_dist_samenoise_*.csv")))
    assert len(csvs) == 20, len(csvs)
    p_all, h_all, worst = np.zeros((20, 24)), np.zeros((20, 24), np.int64), 0.0
    for k, path in enumerate(csvs):
        assert path.endswith(f"_0020_{k:04d}.csv"), path
        txt = re.sub(r"samenoise_", "samenoise_KSpval", os.path.basename(path))[:-4] + ".txt"
        p_all[k] = np.loadtxt(os.path.join(d, txt))
        x = read_pair(path)
        for hour in range(24):
            res = stats.ks_2samp(x[0, :, hour].astype(np.float64), x[1, :, hour].astype(np.float64))
            h_all[k, hour] = int(round(res.statistic * 1000))
            assert abs(res.statistic * 1000 - h_all[k, hour]) < 1e-9
            worst = max(worst, abs(res.pvalue / p_all[k, hour] - 1))
        if k in SAMPLE_PAIRS:
            box = np.zeros((2, 24, 12))
            for c in range(2):
                for hour in range(24):
                    col = x[c, :, hour].astype(np.float64)
                    s = boxplot_stats(col, whis=1.5)[0]
                    box[c, hour] = [len(col), s["mean"], s["q1"], s["med"], s["q3"], s["iqr"], s["whislo"], s["whishi"], s["cilo"],
                                    s["cihi"], (s["fliers"] < s["whislo"]).sum(), (s["fliers"] > s["whishi"]).sum()]
                    assert len(s["fliers"]) == box[c, hour, 10] + box[c, hour, 11]
            out = os.path.join(HERE, f"ks_samples_reference_{k:04d}.npz")
            np.savez_compressed(out, samples=x, box=box)
            print(f"wrote {out} ({os.path.getsize(out)} bytes)")
    print(f"this scipy against the 480 recorded p-values: worst relative difference {worst:.2e}; p from {p_all.min():.3e} to "
          f"{p_all.max()!r}, h from {h_all.min()} to {h_all.max()}")
    rng = np.random.default_rng(SEED)
    asymp = []
    for n, m in ASYMP_SIZES:
        for shift in (0.0, 0.05, 0.3):
            a, b = rng.standard_normal(n), rng.standard_normal(m) + shift
            res = stats.ks_2samp(a, b, method="asymp")
            en = n * m / (n + m)
            asymp.append([n, m, res.statistic, res.pvalue, special.kolmogorov(np.sqrt(en) * res.statistic)])
    asymp = np.array(asymp)
    with open(csvs[0]) as f:
        csv_head = [next(f).rstrip("\n") for _ in range(4)]
    with open(os.path.join(d, re.sub(r"samenoise_", "samenoise_KSpval", os.path.basename(csvs[0]))[:-4] + ".txt")) as f:
        pval_head = [next(f).rstrip("\n") for _ in range(3)]
    out = os.path.join(HERE, "ks_pvalues_reference.npz")
    np.savez_compressed(out, p=p_all, h=h_all, n=1000, asymp_n=asymp[:, 0].astype(np.int64), asymp_m=asymp[:, 1].astype(np.int64),
                        asymp_d=asymp[:, 2], asymp_p_scipy=asymp[:, 3], asymp_p_kolmogorov=asymp[:, 4], csv_head=np.array(csv_head),
                        pval_head=np.array(pval_head))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv)
