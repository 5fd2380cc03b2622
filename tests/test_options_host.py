"""The option table of librdgan_hip.so (csrc/rdgan_options.h: one RD_OPTIONS row per rdgan_set_option name) checked without a
GPU: (1) the rows and the option comment of include/rdgan.h name the same options; (2) tests/host/options_check.cpp, built by the
host C++ compiler from that header alone, prints rd_option_normalise of every row at eight probe values, and the output equals
the table below, which was written from the strcmp ladder rdgan_set_option used to be (not from the new code); (3) every row's
default equals the default-constructed RdOptions field and the value the ladder's struct initialised; (4) the rows flagged as
shaping cached weight forms include every option the hand-packed masks and set-time invalidations covered."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS_H = os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_options.h")
RDGAN_H = os.path.join(ROOT, "include", "rdgan.h")

PROBES = (-5, -1, 0, 1, 2, 3, 9, 100)
X = "x"                                   # refused
BOOL = [1, 1, 0, 1, 1, 1, 1, 1]           # value ? 1 : 0
TRI = [-1, -1, 0, 1, 1, 1, 1, 1]          # value < 0 ? -1 : (value ? 1 : 0)
CLAMP2 = [0, 0, 0, 1, 2, 2, 2, 2]         # value < 0 ? 0 : (value > 2 ? 2 : value)
# name: (default, normalised value at each of PROBES)
LADDER = {
    "collapse": (1, BOOL),
    "wave_specialized": (1, CLAMP2),
    "bf16": (0, BOOL),
    "g9_direct": (1, BOOL),
    "fast_fwd": (-1, TRI),
    "fast_bwd": (-1, TRI),
    "tapgather": (1, BOOL),
    "resident": (1, BOOL),
    "upconv_slab": (1, BOOL),
    "upconv_slab_t": (1, BOOL),
    "upconv2_slab": (1, BOOL),
    "g9_fused": (1, BOOL),
    "d1_fwd_sample": (1, BOOL),
    "g9_bwd_mfma": (1, BOOL),
    "dense16": (1, BOOL),
    "dense_skinny": (1, BOOL),
    "wgrad_boxes": (1, BOOL),
    "border_boxes": (1, CLAMP2),
    "d3_wgrad_slab": (1, BOOL),
    "d2_wgrad_slab": (1, BOOL),
    "upwgrad_slab": (1, BOOL),
    "d1_dgrad_fused": (1, BOOL),
    "combine_dx_fused": (1, BOOL),
    "d1_wgrad16": (1, BOOL),
    "wgrad_wide": (0, BOOL),
    "conv_f16": (1, [X, X, 0, 1, 2, X, X, X]),                 # 0, 1 or 2; refused outside
    "d2_fwd_slab": (0, BOOL),
    "d2_gate_bits": (1, BOOL),
    "d2_slab": (1, BOOL),
    "dense_wgrad_slices": (0, list(PROBES)),                   # stored as given
    "keep_gates": (0, BOOL),
    "split3": (0, BOOL),
    "side_stream": (1, BOOL),                                  # (and off without a side stream: a hook beside the table)
    "gen_fwd_ahead": (-1, TRI),
    "edge_kernels": (1, CLAMP2),
    "sample_offset": (0, [X, X, 0, 1, 2, 3, 9, 100]),          # refused below 0
    "ws_ksplit": (1, [0, 0, 0, 1, 2, 3, 8, 8]),                # value < 0 ? 0 : (value > 8 ? 8 : value)
}
ALIASES = {"bf16": "mfma_bf16"}
# what the generator's nine-term mask, the critic's three-term mask and the invalidations in the ladder covered
FORMS_GEN = {"collapse", "fast_fwd", "bf16", "upconv_slab", "upconv2_slab", "g9_fused", "tapgather", "dense16", "upconv_slab_t",
             "dense_skinny", "conv_f16"}
FORMS_CRITIC = {"bf16", "d2_slab", "d2_fwd_slab", "conv_f16"}


def _table_rows():
    """(name, alias or None) of every RD_OPTIONS row, read from the header's text"""
    text = open(OPTIONS_H).read()
    body = text[text.index("RD_OPTIONS[] = {"):]
    body = body[:body.index("\n};")]
    rows = re.findall(r'^\s*\{"(\w+)",\s*(nullptr|"\w+"),', body, flags=re.M)
    return [(n, None if a == "nullptr" else a.strip('"')) for n, a in rows]


def test_option_names_match_the_header_comment():
    rows = _table_rows()
    names = [n for n, _ in rows]
    assert len(names) == len(set(names)) and set(names) == set(LADDER)
    assert {n: a for n, a in rows if a} == ALIASES
    text = open(RDGAN_H).read()
    end = text.index("int rdgan_set_option(")
    comment = text[text.rindex("/* Options.", 0, end):end]
    # an entry opens a comment line with its quoted name ("a" / "b" for two options documented together)
    documented = set()
    for first, second in re.findall(r'^(?:/\* Options\.\s+| \* )"(\w+)"(?: / "(\w+)")?', comment, flags=re.M):
        documented.update(x for x in (first, second) if x)
    assert documented - set(ALIASES.values()) == set(names)


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("options") / "options_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "host", "options_check.cpp"), "-o", exe],
                   check=True, cwd=ROOT)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.split("\n")
    rows = {}
    for line in lines:
        f = line.split()
        if len(f) == 5 + len(PROBES) and f[0] not in ("keys", "clashes"):
            rows[f[0]] = dict(alias=None if f[1] == "-" else f[1], default=int(f[2]), field_default=int(f[3]), forms=int(f[4]),
                              values=[X if v == X else int(v) for v in f[5:]])
    return rows, res.stdout


def test_normalisation_reproduces_the_ladder(checked):
    rows, out = checked
    assert set(rows) == set(LADDER), out
    for name, (_, want) in LADDER.items():
        assert rows[name]["values"] == want, (name, rows[name]["values"], want)
        assert rows[name]["alias"] == ALIASES.get(name)


def test_defaults_agree(checked):
    rows, _ = checked
    for name, (default, _) in LADDER.items():
        assert rows[name]["default"] == rows[name]["field_default"] == default, name


def test_form_flags_cover_what_the_masks_and_invalidations_covered(checked):
    rows, out = checked
    gen = {n for n, r in rows.items() if r["forms"] & 1}
    critic = {n for n, r in rows.items() if r["forms"] & 2}
    assert gen >= FORMS_GEN and critic >= FORMS_CRITIC, (gen, critic)
    assert "clashes 0" in out           # two values of any flagged option give two keys
