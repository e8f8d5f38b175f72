"""The host side of dense two-piece multi-graph batches (poa_multi_*_dense_2piece): the footprint, the chunks, the refusals, the
ABI and the binding, all without a device, and the stand-alone plan check of tests/multi_dense2_host under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -3, -7
ACGT = np.frombuffer(b"ACGT", np.uint8)
PAD_BYTES = 256


def _pitch(length):
    return ((length + 1 + 63) // 64) * 64


def _term(g, length):
    """The formula of include/poasta_amd_multi_dense2.h: five planes of rows x pitch two-byte cells, and the padding."""
    return 2 * 5 * g.n * _pitch(length) + PAD_BYTES


def _case():
    """Six listings: a 12-node DAG, a 30-node DAG, a graph without queries, a graph without real nodes, the 30-node handle again,
    the 12-node handle again.  Lengths at the 512-column pass edge, the 1024-column register edge, beyond it, and one of 5 000
    symbols that is its graph's last query."""
    rng = np.random.default_rng(5)
    small, big = W.random_dag(1, n_nodes=12, p_edge=0.3), W.random_dag(2, n_nodes=30, p_edge=0.3)
    b = GraphBuilder()
    b.add_path(rng.choice(ACGT, 9))
    idle = b.finish()
    graphs = [small, big, idle, GraphBuilder().finish(), big, small]
    lens = [[0, 1, 63, 64], [511, 512, 1023, 1024, 1100], [], [4, 0], [17, 5000], [2]]
    seqs = [[rng.choice(ACGT, l) for l in ls] for ls in lens]
    return graphs, seqs


def _terms(graphs, seqs):
    return [(gi, _term(g, len(q))) for gi, (g, qs) in enumerate(zip(graphs, seqs)) for q in qs]


def _greedy(terms, cap):
    """A Python restatement of the chunk rule: greedy in query order under max(cap, largest term); a chunk is closed in front of
    the first query that no longer fits.  Returns the first query of every chunk."""
    budget = max(cap, max(t for _, t in terms))
    firsts, used = [0], 0
    for i, (_, t) in enumerate(terms):
        if i > firsts[-1] and used + t > budget:
            firsts.append(i)
            used = 0
        used += t
    return firsts


def test_multi_dense2_footprint_is_the_formula_query_by_query():
    from poasta_amd import aligner
    graphs, seqs = _case()
    terms = [t for _, t in _terms(graphs, seqs)]
    # query by query through the library: a batch of that one query on its graph
    k = 0
    for g, qs in zip(graphs, seqs):
        for q in qs:
            assert aligner.multi_footprint([g], [[q]], dense2=True) == (terms[k], terms[k]), (g.n, len(q))
            k += 1
    total, largest = aligner.multi_footprint(graphs, seqs, dense2=True)
    assert total == sum(terms) and largest == max(terms)
    assert largest == _term(graphs[1], 5000)   # the query of 5 000 symbols is accepted, on the handle listed twice
    assert aligner.multi_footprint(graphs, seqs, dense2=True, config=aligner.make_config("dense")) == (total, largest)
    # POA_CFG_WIDE_QUERIES is not read
    assert aligner.multi_footprint(graphs, seqs, dense2=True, config=aligner.make_config("dense", wide_queries=True)) == (total, largest)
    # graph_qoff + packed queries, and a batch without queries
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert aligner.multi_footprint(graphs, graph_qoff=gq, qseq=qseq, qoff=qoff, dense2=True) == (total, largest)
    assert aligner.multi_footprint(graphs, [[] for _ in graphs], dense2=True) == (0, 0)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/multi_dense2_host built against the plan under the address and undefined-behaviour sanitizers."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path_factory.mktemp("multi_dense2_host")), "multi_dense2_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_dense2_host", "multi_dense2_host.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    return exe


def test_multi_dense2_greedy_chunks_restated(host_exe):
    """The plan's chunks against the restatement above, on the listings of _case() as chains of the same row counts: under a cap
    that ends one chunk inside a graph's range and one between two graphs, a cap below the largest query (raised to it), the
    largest query itself, and no cap.  The host program checks every offset of the same plans on the way."""
    graphs, seqs = _case()
    terms = _terms(graphs, seqs)
    total, largest = sum(t for _, t in terms), max(t for _, t in terms)
    first_listing = {}
    specs = []
    for gi, (g, qs) in enumerate(zip(graphs, seqs)):
        head = "=%d" % first_listing[id(g)] if id(g) in first_listing else "%d" % g.n
        first_listing.setdefault(id(g), gi)
        specs.append(head + ":" + ",".join(str(len(q)) for q in qs))
    assert sum(s.startswith("=") for s in specs) == 2 and any(s.endswith(":") for s in specs)   # handles listed twice, a graph without queries

    def planned(cap):
        r = subprocess.run([host_exe, "chunks", str(cap)] + specs, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        v = [int(x) for x in r.stdout.split()]
        return v[0], v[1], v[2], v[3:]

    cap = largest + PAD_BYTES
    firsts = _greedy(terms, cap)
    inside = [f for f in firsts[1:] if terms[f][0] == terms[f - 1][0]]
    between = [f for f in firsts[1:] if terms[f][0] != terms[f - 1][0]]
    assert len(firsts) >= 3 and inside and between, firsts
    for c in (cap, 1, largest, total // 2, total - 1, total, 0):
        want = _greedy(terms, c if c else total)
        ends = want[1:] + [len(terms)]
        ws = max(sum(t for _, t in terms[a:b]) for a, b in zip(want, ends))
        assert planned(c) == (total, largest, ws, want), c
    assert len(_greedy(terms, 1)) >= len(firsts) and _greedy(terms, 0 + total) == [0]


def test_multi_dense2_refusals_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner._device_graph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)

    def footprint(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        return L.poa_multi_footprint_dense_2piece(hs, len(dgs), aligner._p(gqoff), aligner._p(qo), C.byref(cfg) if cfg is not None else None,
                                                  C.byref(total) if outs else None, C.byref(largest) if outs else None)

    def create(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        h = C.c_void_p()
        rc = L.poa_multi_create_dense_2piece(hs, len(dgs), aligner._p(gqoff), 0, aligner._p(qseq), aligner._p(qo),
                                             C.byref(cfg) if cfg is not None else None, 0, C.byref(h) if outs else None)
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    assert footprint() == 0 and total.value > 0
    if L.poa_device_count() <= 0:
        refused(create(), ERR_NO_DEVICE, "create without a device")
        refused(create(cfg=aligner.make_config("dense")), ERR_NO_DEVICE, "create without a device, dense cfg")
    for mode in ("exact", "hybrid", "score", "checkpoint", "checkpoint2"):
        for call in (footprint, create):
            refused(call(cfg=aligner.make_config(mode)), ERR_UNSUPPORTED, (mode, call.__name__))
    ef = aligner.make_config("dense", aln_type=aligner.AlignmentType.EndsFree())
    for call in (footprint, create):
        refused(call(cfg=ef), ERR_UNSUPPORTED, ("ends-free", call.__name__))
    # the argument errors of poa_multi_create
    bad0 = gq.copy(); bad0[0] = 1
    down = gq.copy(); down[1], down[2] = gq[2], gq[1]
    assert down[2] < down[1]
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    for what, kw in (("graph_qoff[0] != 0", dict(gqoff=bad0)), ("graph_qoff decreasing", dict(gqoff=down)), ("null graph", dict(hs=hole)),
                     ("null outputs", dict(outs=False))):
        for call in (footprint, create):
            refused(call(**kw), ERR_INVALID_ARG, (what, call.__name__))
    # null handles and null costs
    c2 = _lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    buf = np.zeros(4, np.uint32)
    p = aligner._p(buf)
    refused(L.poa_multi_run_dense_2piece(None, C.byref(c2), None, None), ERR_INVALID_ARG, "run, null batch")
    refused(L.poa_multi_fetch_planes_2piece(None, 0, p, p, p, p, p), ERR_INVALID_ARG, "fetch planes, null batch")
    refused(L.poa_align_multi_dense_2piece(handles, len(dgs), aligner._p(gq), None, None, aligner._p(qseq), aligner._p(qoff), None, None, None, 0,
                                           None, None, 0), ERR_INVALID_ARG, "one-shot, null costs")
    bad = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)   # extend1 < extend2
    refused(L.poa_align_multi_dense_2piece(handles, len(dgs), aligner._p(gq), C.byref(bad), None, aligner._p(qseq), aligner._p(qoff), None, None,
                                           None, 0, None, None, 0), ERR_INVALID_ARG, "one-shot, extend1 < extend2")


def test_multi_dense2_binding_value_errors():
    from poasta_amd import aligner
    graphs, seqs = _case()
    two = aligner.PoastaAligner(aligner.Affine2PieceMinGapCost(aligner.GapAffine2Piece(4, 2, 6, 1, 24)))
    one = aligner.PoastaAligner(aligner.AffineMinGapCost(aligner.GapAffine(4, 2, 6)))
    reads = [q for s in seqs for q in s][:3]
    calls = [lambda kw=kw: aligner.multi_footprint(graphs, seqs, dense2=True, **kw)
             for kw in (dict(dense=True), dict(exact=True), dict(two_piece=True), dict(wide=True))]
    calls += [lambda kw=kw: aligner.MultiGraphBatch(graphs, seqs, dense2=True, **kw)
              for kw in (dict(dense=True), dict(exact=True), dict(two_piece=True), dict(wide=True))]
    calls += [
        # what the older tests pin: the one-piece spellings keep raising under a two-piece model
        lambda: aligner.multi_footprint(graphs, seqs, dense=True, two_piece=True),
        lambda: aligner.MultiGraphBatch(graphs, seqs, dense=True, two_piece=True),
        lambda: two.align_multi(graphs, seqs, mode="dense"),
        lambda: two.assign_and_align(graphs, reads, mode="dense"),
        # the new mode under a one-piece config
        lambda: one.align_multi(graphs, seqs, mode="dense2"),
        lambda: one.assign_and_align(graphs, reads, mode="dense2"),
        lambda: two.align_multi(graphs, seqs, mode="dense3"),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            raise AssertionError("call %d was accepted" % k)
    assert hasattr(aligner.MultiGraphBatch, "planes_2piece")


def test_multi_dense2_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd_multi_dense2.h")).read(), flags=re.S)
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    assert '#include "poasta_amd_multi_dense2.h"' in main_h
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(_lib.EXPORTS_MULTI_DENSE2) and len(declared) == 5
    others = (_lib.EXPORTS, _lib.EXPORTS_MULTI_DENSE, _lib.EXPORTS_MULTI_EXACT, _lib.EXPORTS_SCORESET_CAP, _lib.EXPORTS_SCORESET_BEST, _lib.EXPORTS_TB)
    for other in others:
        assert not set(_lib.EXPORTS_MULTI_DENSE2) & set(other)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in _lib.EXPORTS_MULTI_DENSE2:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert getattr(_lib.lib(), name).argtypes is not None, name
        assert name in integration, name
    # the argument lists are the _2piece namesakes'
    assert re.search(r"poa_multi_run_dense_2piece\(poa_multi_t\* m, const poa_costs2_t\* costs, const poa_config_t\* cfg, void\* stream\);", hdr)


def test_multi_dense2_host_plan_under_sanitizers(host_exe):
    """tests/multi_dense2_host: the footprint formula, planes aligned and in bounds, regions disjoint, chunk coverage exact and
    greedy, one table copy per handle, a 5 000-symbol query — a program of its own, address and undefined-behaviour sanitizers
    on, on the CPU."""
    r = subprocess.run([host_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_dense2_host ok" in r.stdout
