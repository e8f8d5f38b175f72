"""The two gap-state traceback flags that the compact format of poa_forward_px_kernel<3> no longer stores
(poasta_amd/csrc/poa_tb_derive.hpp): compiled for the host and run over EVERY cell of the oracle's dense planes, given only
what that format keeps — the M plane, the flags I == M and D == M, the D rows flagged ROW_STORE_D.  The derived flag must
equal the one the full I / D planes give for every cell with a finite I (any row) resp. a finite D (chain rows): no cell
is left out, and the test counts the cells itself to say so.  On the GPU: the format against the bit-plane format and
the oracle's dense batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
INF = 0xFFFFFFFF


def _p(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(ROOT, "tests", "derive_host", "derive_host.cpp")
    out = os.path.join(ROOT, "tests", "derive_host", "libderive_host.so")
    deps = [src] + [os.path.join(ROOT, "poasta_amd", "csrc", f) for f in ("poa_tb_derive.hpp", "poa_graph.cpp", "poa_graph.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src,
                               os.path.join(ROOT, "poasta_amd", "csrc", "poa_graph.cpp")])
    X = C.CDLL(out)
    X.derive_host_check.argtypes = [C.c_uint32] * 3 + [vp] * 5 + [C.c_uint8] * 2 + [vp, C.c_uint32, vp, vp, vp, vp]
    X.derive_host_check_clamped.argtypes = [C.c_uint32] * 3 + [vp] * 5 + [C.c_uint8] * 2 + [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    X.derive_host_chain_nodes.argtypes = [C.c_uint32] * 3 + [vp] * 5 + [vp]
    return X


def _check_every_cell(X, oracle, g, qs, costs):
    """-> (cells checked for B, for D).  costs = (mismatch, open, extend)."""
    og = oracle.OracleGraph.from_csr(g.as_dict())
    orank = og.export_csr()["rank"]
    d = g.as_dict()
    arrs = [np.ascontiguousarray(d[k], dtype=(np.uint8 if k == "symbol" else np.uint32)) for k in ("symbol", "succ_off", "succ", "pred_off", "pred")]
    head = (int(d["n"]), int(d["start"]), int(d["end"]))
    is_chain = np.zeros(head[0], np.uint8)
    assert X.derive_host_chain_nodes(*head, *[_p(a) for a in arrs], _p(is_chain)) == 0
    nb = nd = 0
    for q in qs:
        q = np.ascontiguousarray(q, np.uint8)
        od = og.dense_align(q, oracle.Costs(*costs), planes=True)
        m, i, dd = (np.ascontiguousarray(od[k][orank]) for k in ("M", "I", "D"))    # by node
        out = np.zeros(8, np.uint64)
        assert X.derive_host_check(*head, *[_p(a) for a in arrs], costs[1], costs[2], _p(q), len(q), _p(m), _p(i), _p(dd), _p(out)) == 0
        assert int(out[2]) == 0 and int(out[3]) == 0, "derived flag differs: state %d row %d column %d (B: %d, D: %d cells differ), costs %r, len %d" % (
            int(out[5]), int(out[6]), int(out[7]), int(out[2]), int(out[3]), costs, len(q))
        assert int(out[4]) == 0, "the derivation read a D row the compact layout does not keep"
        # the share of cells left out is zero: every finite I cell right of column 0 (column 0 has no insertion state at all)
        # and every finite D cell of a chain row
        assert (i[:, 0] == INF).all()
        assert int(out[0]) == int((i != INF).sum())
        assert int(out[1]) == int((dd[is_chain != 0] != INF).sum())
        nb += int(out[0]); nd += int(out[1])
    return nb, nd


COSTS = [(4, 6, 2), (2, 8, 1), (1, 10, 2), (3, 1, 1), (4, 4, 2), (4, 0, 2), (4, 0, 1), (255, 3, 1), (255, 6, 2), (1, 0, 1)]


def test_random_dags(harness, oracle):
    nb = nd = 0
    for seed in range(60):
        rng = np.random.Generator(np.random.PCG64(5000 + seed))
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 30)), p_edge=float(rng.uniform(0.1, 0.4)), alphabet=alpha)
        qs = [W.random_walk_query(rng, g, 0.3, alpha) for _ in range(6)]
        qs += [np.zeros(0, np.uint8), qs[0][:1], np.concatenate([qs[1]] * 3)]      # empty, one base, longer than the graph
        b, d = _check_every_cell(harness, oracle, g, qs, COSTS[seed % len(COSTS)])
        nb += b; nd += d
    assert nb > 5000 and nd > 2000


def test_linearish_graph(harness, oracle):
    g, (qseq, qoff) = W.scaled_linearish(300, 15, 8, 6, 320, p_sub=0.05, p_ins=0.03, p_del=0.03)
    qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(6)]
    qs = [qs[0], qs[1][:40], qs[2][:200], np.concatenate([qs[3], qs[4][:150]]), qs[5][100:]]   # shorter and longer than the graph
    for costs in ((4, 6, 2), (4, 0, 2), (2, 8, 1), (255, 3, 1)):
        nb, nd = _check_every_cell(harness, oracle, g, qs, costs)
        assert nb > 100000 and nd > 100000


def test_msa_and_bubble_graphs(harness, oracle):
    rows = [b"ACGT-ACGTTGCA--ACGTAC", b"ACGTTACG-TGCAGGACGTAC", b"AC-T-ACGTTGAA--ACG-AC", b"ACGTTACCTTGCAG-ACGTAC"]
    g = W.msa_to_graph(rows)
    qs = [np.frombuffer(r.replace(b"-", b""), np.uint8) for r in rows] + [np.frombuffer(b"ACGTACGTGGGGACGTAC", np.uint8), np.frombuffer(b"TTTT", np.uint8)]
    for costs in COSTS:
        _check_every_cell(harness, oracle, g, qs, costs)
    poa = W.PangenomePOA(ref_len=300, n_hap=6, p_snp=0.02, p_indel=0.01, max_indel=6, seed=4)
    _check_every_cell(harness, oracle, poa.graph, poa.queries(4, length=120) + poa.queries(2, length=330, seed=9), (4, 6, 2))
    lay = W.LayeredPOA(n_layers=50, width=4, indeg=4, seed=5)
    for costs in ((4, 6, 2), (3, 0, 1)):
        _check_every_cell(harness, oracle, lay.graph, lay.queries(4, length=0) + [lay.queries(1, length=0, seed=8)[0][:20]], costs)


def test_symbols_outside_acgt(harness, oracle):
    rng = np.random.default_rng(21)
    alpha = np.frombuffer(b"ACGTNacgtRYKM", np.uint8)
    backbone = rng.choice(alpha, 200)
    b = GraphBuilder()
    ids = b.add_path(backbone)
    for _ in range(20):
        i = int(rng.integers(1, 190))
        v = b.add_node(int(rng.choice(alpha)))
        b.add_edge(ids[i - 1], v); b.add_edge(v, ids[i + 1])
        j = int(rng.integers(1, 190))
        b.add_edge(ids[j], ids[j + int(rng.integers(2, 6))])
    g = b.finish()
    qs = []
    for _ in range(4):
        q = backbone.copy()
        pos = rng.choice(len(q), 20, replace=False)
        q[pos] = rng.choice(alpha, 20)
        qs.append(q[:int(rng.integers(100, 200))])
    qs.append(np.concatenate([backbone, backbone[:60]]))
    for costs in ((4, 6, 2), (3, 9, 1), (4, 0, 1)):
        _check_every_cell(harness, oracle, g, qs, costs)


# ---- GPU: the format itself ---------------------------------------------------------------------------------------------

def _run(engine, g, qseq, qoff, costs, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rb = engine.ResidentBatch(g, qseq, qoff)
        rb.run(engine.GapAffine(costs[0], costs[2], costs[1]))
        r = rb.fetch()
        layout = rb.layout()
        rb.close()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return r, layout


def _same(a, b):
    return (np.array_equal(a.score, b.score) and np.array_equal(a.flags, b.flags) and np.array_equal(a.pair_off, b.pair_off)
            and np.array_equal(a.pairs, b.pairs))


def _gpu_case(engine, oracle, g, qs, costs=(4, 6, 2)):
    qseq, qoff = pack_queries(qs)
    ref, _ = _run(engine, g, qseq, qoff, costs, {"POA_MF": "0"})
    og = oracle.OracleGraph.from_csr(g.as_dict())
    D = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)
    for env in ({"POA_TB_GROUP": "16", "POA_TB_DEPTH": "1"}, {"POA_TB_GROUP": "64", "POA_TB_DEPTH": "64"},
                {"POA_TB_GROUP": "16", "POA_TB_DEPTH": "16"}, {}):
        r, _ = _run(engine, g, qseq, qoff, costs, dict(env, POA_MF="3"))
        assert _same(r, ref), env
        assert np.array_equal(r.score, D["score"]) and np.array_equal(r.flags, D["flags"]), env
        for i in range(len(qs)):
            assert r.raw_alignment(i) == oracle.batch_alignment(D, i), (env, i)
    return _run(engine, g, qseq, qoff, costs, {})   # what the engine picks itself


@pytest.mark.gpu
def test_gpu_shapes_of_the_flag_encoding_test(engine, oracle):
    g, (qseq, qoff) = W.scaled_linearish(600, 30, 15, 40, 700)
    qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(40)]
    r, layout = _gpu_case(engine, oracle, g, qs)
    if not any(k in os.environ for k in ("POA_MF", "POA_PX", "POA_PLANES", "POA_COMPACT", "POA_PACKED", "POA_RELATIVE", "POA_FWD_QUADS", "POA_FUSE_TB")):
        assert "derived_gaps" in layout     # one strip, bound below 0x3FFF: the engine picks the new format by itself


@pytest.mark.gpu
def test_gpu_one_strip_kernel_shapes(engine, oracle):
    g, (qseq, qoff) = W.scaled_linearish(880, 40, 20, 6, 1000, p_sub=0.04, p_ins=0.02, p_del=0.02)
    full = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(6)]
    qs = [full[0], full[1][:513], full[2][:600], full[3][:777], full[4][:900], full[5][:100], full[0][:1023], full[1][:64], full[2][:960]]
    for costs in ((4, 6, 2), (9, 40, 12), (3, 1, 1)):
        _gpu_case(engine, oracle, g, qs, costs)
    poa = W.LayeredPOA(n_layers=800, width=4, indeg=4, seed=3)
    qs = poa.queries(5, length=0) + [q[:600] for q in poa.queries(2, length=0, seed=8)]
    _gpu_case(engine, oracle, poa.graph, qs)


@pytest.mark.gpu
def test_gpu_symbols_beyond_acgt(engine, oracle):
    rng = np.random.default_rng(21)
    alpha = np.frombuffer(b"ACGTNacgtRYKM", np.uint8)
    probs = np.array([6, 6, 6, 6, 2, 1, 1, 1, 1, .5, .5, .5, .5]); probs = probs / probs.sum()
    backbone = rng.choice(alpha, 820, p=probs)
    b = GraphBuilder()
    ids = b.add_path(backbone)
    for _ in range(40):
        i = int(rng.integers(1, 800))
        v = b.add_node(int(rng.choice(alpha, p=probs)))
        b.add_edge(ids[i - 1], v); b.add_edge(v, ids[i + 1])
        j = int(rng.integers(1, 790))
        b.add_edge(ids[j], ids[j + int(rng.integers(2, 6))])
    g = b.finish()
    qs = []
    for k in range(8):
        q = backbone.copy()
        pos = rng.choice(len(q), 40, replace=False)
        q[pos] = rng.choice(alpha, 40, p=probs)
        cut = sorted(rng.choice(len(q), 2, replace=False))
        qs.append(np.concatenate([q[:cut[0]], q[cut[0] + int(rng.integers(0, 4)):]])[:int(rng.integers(530, 820))])
    for costs in ((4, 6, 2), (3, 9, 1)):
        _gpu_case(engine, oracle, g, qs, costs)


@pytest.mark.gpu
def test_gpu_deep_bubbles(engine, oracle):
    # (padded to more than 512 columns with one long query so that the batch runs in the one-strip kernel)
    poa = W.LayeredPOA(n_layers=60, width=4, indeg=4, seed=5)
    qs = poa.queries(10, length=0)
    qs.append(np.concatenate([qs[0]] * 10)[:600])
    _gpu_case(engine, oracle, poa.graph, qs)


@pytest.mark.gpu
def test_gpu_config2_reads_with_long_insertion_tails(engine, oracle):
    g, (qseq, qoff) = W.config2(n_queries=600)
    qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(600)]
    r, layout = _gpu_case(engine, oracle, g, qs)
    assert int((r.pairs[:, 0] == 0xFFFFFFFF).sum()) > 20000   # the insertion runs are there
