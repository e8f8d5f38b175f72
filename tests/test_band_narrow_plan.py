"""The narrow tier of the paired banded forward pass, on the CPU: the narrow plan of the headline graph and the rule that decides
who runs the tier (band_narrow_class / band_narrow_pairs in poasta_amd/csrc/poa_dense_plan.cpp, compiled for the host by
tests/band_narrow_host).

The narrow plan is plan_band of poasta_amd/csrc/poa_band_plan.cpp with a window of 384 columns and the 512 plan's segments and base
alignment: what tests/test_band_plan.py's Plan computes for (64, 384).  For the headline graph the plan must certify every
headline read: the largest optimal score of the 10 000 reads of 1 kbp is 518 under the default costs (mismatch 4, open 6, extend
2) - the oracle's A* (min-gap heuristic, pruning) over all of them, figure taken from the issue that introduced the tier - so
T_n = e * (D_n - 4) has to reach it at L = 1000."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder
from band_model import fork_graph
from test_band_plan import Plan, _check_band_columns, harness   # noqa: F401  (the host build of the band plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_ROWS, WINDOW, NARROW = 64, 512, 384
HEADLINE_MAX_SCORE, E = 518, 2
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def rule():
    src = os.path.join(ROOT, "tests", "band_narrow_host", "band_narrow_host.cpp")
    out = os.path.join(ROOT, "tests", "band_narrow_host", "libband_narrow_host.so")
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    deps = [src, os.path.join(csrc, "poa_dense_plan.cpp"), os.path.join(csrc, "poa_dense_plan.hpp"), os.path.join(ROOT, "include", "poasta_amd.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src, os.path.join(csrc, "poa_dense_plan.cpp")])
    X = C.CDLL(out)
    X.band_narrow_host_class.argtypes = [C.c_uint32] * 2
    X.band_narrow_host_class.restype = C.c_uint32
    X.band_narrow_host_pairs.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    X.band_narrow_host_pairs.restype = None
    return X


def _pairs(X, tune_value, pair_by_rule, n_rule, n_any):
    """tune_value: what POA_TUNE_BAND_PAIR holds (None: not set) -> (band_pair, band_narrow, pairs of the narrow tier)"""
    out = (C.c_int32 * 3)()
    X.band_narrow_host_pairs(0 if tune_value is None else tune_value + 1, int(pair_by_rule), n_rule, n_any, out)
    return tuple(out)


def test_headline_narrow_plan(harness, rule):
    g, _ = W.config2(n_queries=4)
    for L in (900, 1000, 1100):
        pl, wide = Plan(harness, g, L, SEG_ROWS, NARROW), Plan(harness, g, L, SEG_ROWS, WINDOW)
        assert 4 <= pl.D < wide.D, (L, pl.D, wide.D)
        assert (np.diff(pl.bases) >= 0).all() and pl.bases[0] == 0, pl.bases      # the windows are monotone
        _check_band_columns(pl)      # band(D_n) lies inside the windows, band(D_n + 1) does not fit
        assert rule.band_narrow_host_class(pl.D, L) == 0, (L, pl.D)      # the rule takes the class: D_n - 4 >= L / 4
        if L == 1000:
            # every headline read is certified, with room: the issue's figure for alignment 8 is D_n = 295, T_n = 582
            assert E * (pl.D - 4) >= HEADLINE_MAX_SCORE + 32, pl.D


def test_class_rule_from_both_sides(harness, rule):
    for L in (512, 1000, 1023):
        edge = 4 + (L + 3) // 4      # the smallest D_n with D_n - 4 >= L / 4
        assert rule.band_narrow_host_class(edge, L) == 0 and rule.band_narrow_host_class(edge - 1, L) == 1, L
    for d in (0, 3):
        assert rule.band_narrow_host_class(d, 512) == 2
    assert rule.band_narrow_host_class(4, 512) == 1
    # A class whose 512 plan has a band and whose narrow plan has none (D_n = 0): two branches of 420 nodes - the segment that
    # holds the end of the first branch and the start of the second spans 420 columns of band(0) alone.
    g, walks = fork_graph(100, 420, 420, 100, seed=3)
    L = len(walks[0])
    assert Plan(harness, g, L, SEG_ROWS, WINDOW).D >= 4
    d_n = Plan(harness, g, L, SEG_ROWS, NARROW).D
    assert d_n == 0 and rule.band_narrow_host_class(d_n, L) == 2
    # (The four-row graph of tests/test_band_pairs.py's test_default_rule_from_both_sides is no such class: with 512-base reads
    # its band(D) is empty up to D = 507 under either window, so both plans have that D and certify nothing.)
    gb = GraphBuilder()
    gb.add_path(ACGT[[0, 1, 2, 3]])
    four = gb.finish()
    assert Plan(harness, four, 512, SEG_ROWS, NARROW).D == Plan(harness, four, 512, SEG_ROWS, WINDOW).D >= 500


def test_override_table(rule):
    # POA_TUNE_BAND_PAIR: bits 0..1 the pairing (0 never, 1 always, 2 by the rule), bits 2..3 the tier (0 rule, 1 never, 2 whenever paired)
    n_rule, n_any = 5, 9
    for pair_bits, band_pair in ((None, -1), (0, 0), (1, 1), (2, -1)):
        for narrow_bits, band_narrow in ((0, -1), (1, 0), (2, 1)):
            if pair_bits is None and narrow_bits:
                continue
            value = None if pair_bits is None else pair_bits | (narrow_bits << 2)
            for by_rule in (False, True):
                got = _pairs(rule, value, by_rule, n_rule, n_any)
                want = 0 if band_narrow == 0 else (n_any if band_narrow == 1 else (n_rule if by_rule else 0))
                assert got == (band_pair, band_narrow, want), (pair_bits, narrow_bits, by_rule, got)
    # a forced POA_BAND_PAIR=1 alone: a chunk below the pair rule's count runs exactly as before the tier existed
    assert _pairs(rule, 1, False, n_rule, n_any) == (1, -1, 0)


def test_environment_reaches_the_entry():
    from poasta_amd import _lib
    i = _lib.TUNE_KEYS.index("BAND_PAIR")
    for pair, narrow, value in ((None, "1", 2 | (2 << 2)), ("1", "1", 1 | (2 << 2)), ("1", "0", 1 | (1 << 2)), ("0", None, 0), ("1", None, 1)):
        kw = {k: v for k, v in (("band_pair", pair), ("band_narrow", narrow)) if v is not None}
        old = {k: os.environ.pop(k, None) for k in ("POA_BAND_PAIR", "POA_BAND_NARROW")}
        try:
            cfg = _lib.tune_from_env(**kw)
        finally:
            os.environ.update({k: v for k, v in old.items() if v is not None})
        assert cfg.tune[i] == value + 1, (pair, narrow, cfg.tune[i])
