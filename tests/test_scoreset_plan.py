"""The host side of score sets (poa_scoreset_*): the footprint, the argument errors and the ABI, all without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
SCORESET_SYMBOLS = ("poa_scoreset_footprint", "poa_scoreset_create", "poa_scoreset_run", "poa_scoreset_run_2piece", "poa_scoreset_fetch",
                    "poa_scoreset_stats", "poa_scoreset_device_results", "poa_scoreset_workspace_bytes", "poa_scoreset_destroy",
                    "poa_score_pairs", "poa_score_pairs_2piece")


def _case():
    rng = np.random.default_rng(3)
    graphs = [W.random_dag(s, n_nodes=n, p_edge=0.3) for s, n in ((1, 12), (2, 30), (3, 5))]
    g, _ = W.scaled_linearish(300, 15, 8, 1, 50)
    graphs += [g, GraphBuilder().finish(), graphs[1]]
    seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), l) for l in (0, 1, 63, 64, 5, 200, 1100, 30, 1023, 1024)]
    return graphs, seqs


def _pitch(length):
    # the rule of a single-graph batch, poasta_amd/csrc/poa_engine.hip batch_create_impl:
    #     const uint32_t pitch = (uint32_t)(((L + 1 + 63) / 64) * 64);
    return ((length + 1 + 63) // 64) * 64


def _term(aligner, g, q):
    # a pair holds max(n_slots(graph), 1) x pitch 4-byte cells of M and of D, plus 256 bytes
    _, n_slots = aligner.DeviceGraph(g).sweep_slots()
    return 2 * max(n_slots, 1) * _pitch(len(q)) * 4 + 256


def test_scoreset_footprint_is_the_sum_over_pairs():
    from poasta_amd import aligner
    graphs, seqs = _case()
    matrix = [(qi, gi) for qi in range(len(seqs)) for gi in range(len(graphs))]
    terms = [_term(aligner, graphs[gi], seqs[qi]) for qi, gi in matrix]
    assert len(set(terms)) > 4
    total, largest = aligner.scoreset_footprint(graphs, seqs)
    assert total == sum(terms) and largest == max(terms)
    # the matrix form is the explicit list
    assert aligner.scoreset_footprint(graphs, seqs, pairs=matrix) == (total, largest)
    assert aligner.scoreset_footprint(graphs, seqs, config=aligner.make_config("score")) == (total, largest)
    # an unsorted list with repeats; a graph and a query without a pair
    pairs = [(6, 3), (0, 1), (6, 3), (9, 0), (2, 5), (2, 1), (8, 4), (6, 2)]
    terms = [_term(aligner, graphs[gi], seqs[qi]) for qi, gi in pairs]
    assert aligner.scoreset_footprint(graphs, seqs, pairs=pairs) == (sum(terms), max(terms))
    # packed queries; a set without pairs, without queries, without graphs
    qseq, qoff = pack_queries(seqs)
    assert aligner.scoreset_footprint(graphs, qseq=qseq, qoff=qoff, pairs=pairs) == (sum(terms), max(terms))
    assert aligner.scoreset_footprint(graphs, seqs, pairs=np.zeros((0, 2), np.int64)) == (0, 0)
    assert aligner.scoreset_footprint(graphs, []) == (0, 0)
    assert aligner.scoreset_footprint([], seqs) == (0, 0)


def test_scoreset_handle_listed_twice_counts_twice():
    from poasta_amd import aligner
    graphs, seqs = _case()
    assert graphs[5] is graphs[1]
    once = aligner.scoreset_footprint([graphs[1]], seqs)
    twice = aligner.scoreset_footprint([graphs[1], graphs[5]], seqs)
    assert twice == (2 * once[0], once[1])
    pairs = [(5, 0), (5, 1), (6, 1)]
    terms = [_term(aligner, graphs[1], seqs[qi]) for qi, _ in pairs]
    assert aligner.scoreset_footprint([graphs[1], graphs[5]], seqs, pairs=pairs) == (sum(terms), max(terms))


def test_scoreset_argument_errors_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner.DeviceGraph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries(seqs)
    nq, ng = len(seqs), len(graphs)
    pq = np.array([6, 0, 6, 9], np.uint32)
    pg = np.array([3, 1, 3, 0], np.uint32)
    total, largest = C.c_uint64(0), C.c_uint64(0)
    c = _lib.PoaCosts(4, 6, 2, 0)
    p = aligner._p

    def footprint(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        return L.poa_scoreset_footprint(hs, ng, nq, p(off), n, p(q), p(g), C.byref(cfg) if cfg is not None else None, C.byref(total), C.byref(largest))

    def create(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        h = C.c_void_p()
        rc = L.poa_scoreset_create(hs, ng, 0, nq, p(qseq), p(off), n, p(q), p(g), C.byref(cfg) if cfg is not None else None, 0, C.byref(h))
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_scoreset_destroy(h)
        return rc

    def one_shot(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        s, f = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        rc = L.poa_score_pairs(hs, ng, C.byref(c), C.byref(cfg) if cfg is not None else None, nq, p(qseq), p(off), n, p(q), p(g), p(s), p(f), None, 0)
        assert rc != 0 or L.poa_device_count() > 0
        return rc

    assert footprint() == 0 and total.value > 0
    assert footprint(n=nq * ng, q=None, g=None) == 0
    assert footprint(n=0) == 0 and footprint(n=0, q=None, g=None) == 0 and total.value == 0   # no pairs: valid, nothing to hold
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    bad_q, bad_g = pq.copy(), pg.copy()
    bad_q[2], bad_g[1] = nq, ng
    cases = (("null graph", dict(hs=hole)), ("query index out of range", dict(q=bad_q)), ("graph index out of range", dict(g=bad_g)),
             ("null qoff", dict(off=None)), ("pair_query alone is null", dict(q=None)), ("pair_graph alone is null", dict(g=None)),
             ("matrix count too small", dict(n=nq * ng - 1, q=None, g=None)), ("matrix count too large", dict(n=nq * ng + 1, q=None, g=None)))
    for what, kw in cases:
        for call in (footprint, create, one_shot):
            L.poa_scoreset_footprint(handles, ng, nq, p(qoff), 4, p(pq), p(pg), None, C.byref(total), C.byref(largest))   # (a good call in between)
            assert call(**kw) == ERR_INVALID_ARG, (what, call.__name__)
            assert L.poa_last_error() != b"", what
    for mode in ("dense", "exact", "hybrid", "checkpoint", "checkpoint2"):
        for call in (footprint, create, one_shot):
            assert call(cfg=aligner.make_config(mode)) == ERR_UNSUPPORTED, (mode, call.__name__)
            assert L.poa_last_error() != b""
    ef = aligner.make_config("score", aln_type=aligner.AlignmentType.EndsFree())
    for call in (footprint, create, one_shot):
        assert call(cfg=ef) == ERR_UNSUPPORTED, call.__name__
    # the two-piece one-shot refuses extend1 < extend2 before anything else
    c2 = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)
    s = np.zeros(4, np.uint32)
    assert L.poa_score_pairs_2piece(handles, ng, C.byref(c2), None, nq, p(qseq), p(qoff), 4, p(pq), p(pg), p(s), None, None, 0) == ERR_INVALID_ARG
    assert b"gap_extend1" in L.poa_last_error()
    # null handles of the set itself
    st = _lib.PoaStats()
    assert L.poa_scoreset_run(None, C.byref(c), None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_2piece(None, C.byref(c2), None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_fetch(None, None, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_stats(None, C.byref(st)) == ERR_INVALID_ARG
    assert L.poa_scoreset_workspace_bytes(None, C.byref(total)) == ERR_INVALID_ARG
    assert L.poa_scoreset_device_results(None, None, None) == ERR_INVALID_ARG
    L.poa_scoreset_destroy(None)
    # the binding checks pair indices before the call
    for bad in ([(0, ng)], [(nq, 0)], [(-1, 0)]):
        try:
            aligner.scoreset_footprint(graphs, seqs, pairs=bad)
            raise AssertionError("pair %r was accepted" % (bad,))
        except ValueError:
            pass


def test_scoreset_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_(?:scoreset_[a-z_0-9]+|score_pairs[a-z_0-9]*))\s*\(", hdr)))
    assert declared == sorted(SCORESET_SYMBOLS)
    for name in SCORESET_SYMBOLS:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+poa_scoreset\s+poa_scoreset_t\s*;", hdr)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SCORESET_SYMBOLS:
        assert name in integration, name


CPP_MIRROR = r"""
#include <cstdio>
#include "poasta_amd.hpp"
using namespace poasta;
int main() {
    graphs::POAGraph a, b;
    a.add_alignment_with_weights("a", "ACGTACGTTTGA", nullptr, std::vector<size_t>(12, 1));
    b.add_alignment_with_weights("b", "ACGAACGATTGA", nullptr, std::vector<size_t>(12, 1));
    const std::vector<std::string> seqs = {"ACGTACGTTTGA", "ACGAACGATTGA", "ACG"};
    try {
        aligner::ScoreSet full({&a, &b}, seqs);
        aligner::ScoreSet some({&a, &b}, seqs, {{2, 1}, {0, 0}, {2, 1}});
        full.run(aligner::GapAffine(4, 2, 6));
        some.run(aligner::GapAffine2Piece(4, 2, 6, 1, 24));
        const auto r = full.fetch();
        const auto q = some.fetch();
        if (full.size() != 6 || r.score.size() != 6 || q.score.size() != 3) return 2;
        if (r.score[0] != 0 || r.score[3] != 0 || r.score[1] == 0 || q.score[0] != q.score[2] || q.score[1] != 0) return 3;
        std::printf("scoreset mirror ok\n");
    } catch (const PoastaError& e) {
        std::printf("PoastaError: %s\n", e.what());
    }
    return 0;
}
"""


def test_scoreset_cpp_mirror(tmp_path):
    """include/poasta_amd.hpp: aligner::ScoreSet compiles the way the host drivers are built, links and — where a device is
    visible — scores; without one the engine's refusal arrives as a PoastaError."""
    from poasta_amd import _lib
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    src, exe = os.path.join(str(tmp_path), "scoreset_mirror.cpp"), os.path.join(str(tmp_path), "scoreset_mirror")
    with open(src, "w") as f:
        f.write(CPP_MIRROR)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + libdir, "-lpoasta_amd", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], stdout=subprocess.PIPE)
    assert r.returncode == 0, r.stdout.decode()
    if _lib.lib().poa_device_count() > 0:
        assert b"scoreset mirror ok" in r.stdout
    else:
        assert b"PoastaError" in r.stdout and b"no HIP device" in r.stdout
