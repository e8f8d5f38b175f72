"""The host side of best-of score-set runs (poa_scoreset_run_best): the launch order and the query-to-pairs lists under the address
and undefined-behaviour sanitizers (tests/scoreset_best_host), and the ABI, all without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1
BEST_SYMBOLS = ("poa_scoreset_run_best", "poa_scoreset_run_2piece_best", "poa_scoreset_fetch_best", "poa_scoreset_device_best",
                "poa_score_best", "poa_score_best_2piece")


def test_scoreset_best_host_plan_under_sanitizers(tmp_path):
    """tests/scoreset_best_host: every best-of range is a permutation of the same range of class_list, ranks do not decrease along
    it, the pair index ascends within a rank, the CSR lists each pair once under its query — a program of its own, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "scoreset_best_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "scoreset_best_host", "scoreset_best_host.cpp"), os.path.join(csrc, "poa_scoreset_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"scoreset_best_host ok" in r.stdout


def test_scoreset_best_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    best_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd_scoreset_best.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", best_h)))
    assert declared == sorted(BEST_SYMBOLS) == sorted(_lib.EXPORTS_SCORESET_BEST)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in BEST_SYMBOLS:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert getattr(_lib.lib(), name).argtypes is not None, name
    # poasta_amd.h includes it at its end, behind the cap header
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    assert main_h.index('#include "poasta_amd_scoreset_cap.h"') < main_h.index('#include "poasta_amd_scoreset_best.h"')
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*poa_best_t\s*;", best_h)
    # the ctypes mirror of poa_best_t: 32 bytes, five words and three reserved ones
    assert C.sizeof(_lib.PoaBest) == 32
    assert [f[0] for f in _lib.PoaBest._fields_] == ["pair", "score", "flags", "second_score", "n_within", "reserved"]
    assert re.findall(r"uint32_t\s+([a-z_]+)", re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*poa_best_t", best_h).group(1)) == \
        ["pair", "score", "flags", "second_score", "n_within", "reserved"]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in BEST_SYMBOLS + ("poa_best_t",):
        assert name in integration, name


def test_scoreset_best_null_arguments_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    p = aligner._p
    c, c2 = _lib.PoaCosts(4, 6, 2, 0), _lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    best = np.zeros((4, 8), np.uint32)
    fake = C.c_void_p(1)   # never dereferenced: the other argument is refused first
    ptr = C.c_void_p()
    assert L.poa_scoreset_run_best(None, C.byref(c), None, 0, None, None) == ERR_INVALID_ARG and L.poa_last_error() != b""
    assert L.poa_scoreset_run_2piece_best(None, C.byref(c2), None, 0, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_best(fake, None, None, 0, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_2piece_best(fake, None, None, 0, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_fetch_best(None, p(best)) == ERR_INVALID_ARG
    assert L.poa_scoreset_fetch_best(fake, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_device_best(None, C.byref(ptr)) == ERR_INVALID_ARG
    assert L.poa_scoreset_device_best(fake, None) == ERR_INVALID_ARG
    # the one-shots: costs and the result array
    g = aligner.DeviceGraph(W.random_dag(1, n_nodes=8, p_edge=0.3))
    handles = (C.c_void_p * 1)(g.handle)
    qseq, qoff = np.frombuffer(b"ACGT", np.uint8), np.array([0, 4], np.uint64)
    for fn, cc in ((L.poa_score_best, c), (L.poa_score_best_2piece, c2)):
        assert fn(handles, 1, None, None, 1, p(qseq), p(qoff), 1, None, None, 0, None, p(best), None, None, None, 0) == ERR_INVALID_ARG
        assert fn(handles, 1, C.byref(cc), None, 1, p(qseq), p(qoff), 1, None, None, 0, None, None, None, None, None, 0) == ERR_INVALID_ARG
        assert L.poa_last_error() != b""
    bad2 = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)
    assert L.poa_score_best_2piece(handles, 1, C.byref(bad2), None, 1, p(qseq), p(qoff), 1, None, None, 0, None, p(best), None, None, None,
                                   0) == ERR_INVALID_ARG
    assert b"gap_extend1" in L.poa_last_error()
