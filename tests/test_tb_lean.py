"""The lean walk kernel (poa_traceback_mf_kernel<GW>, poasta_amd/csrc/poa_traceback_mf.hpp) against the generic one
(poa_traceback_kernel<u16, true, GW>) and the oracle's sequential restatement of the reference's backtrace.

CPU part: tb_lean_eligible / plan_dense_chunk of poa_dense_plan.cpp against the rule restated here, over the launch-matrix cases
and the POA_TB_LEAN override (tests/tb_lean_host, also run as a program of its own under the sanitizers).

GPU part: every case runs one resident batch under POA_TB_LEAN=0 and =1, asserts through poa_batch_tb_info which kernel ran,
and compares score, flags, pair_off and pairs of the two runs with each other and with the oracle.  What a planted read is there
for (a deletion run of k rows, an insertion run of k bases, a tie, ...) is asserted from the oracle's output first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import _lib
from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries
import test_dense_launch_matrix as LM
from test_band_plan import harness   # noqa: F401  (the host build of the band plan, for the tiers of test_band_tiers_in_one_batch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poasta_amd", "csrc")
HOST_DIR = os.path.join(ROOT, "tests", "tb_lean_host")
HOST_SRC = os.path.join(HOST_DIR, "tb_lean_host.cpp")
NONE = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
COSTS = (4, 6, 2)
AMBIGUOUS, START_QUIRK, REF_PANIC, SHORT_QUERY, TRUNCATED = 1, 2, 4, 8, 16
TB_LEAN_SHIFT = 4


# ---- CPU: the rule ------------------------------------------------------------------------------------------------------------------
def lean_of(pred, mode="dense", tb_lean=None, plane_elems=0):
    """the walk kernel of a chunk whose launch record is `pred` (test_dense_launch_matrix.predict): the rule restated"""
    eligible = (mode == "dense" and pred["tb_lanes"] != 0 and "compact" in pred["layout"] and pred["code_fmt"] == 4
                and "relative" not in pred["layout"] and plane_elems < 2 ** 32)
    return eligible and tb_lean != 0


def _pair_word(tb_lean, band_pair=None, band_narrow=None):
    """tune[POA_TUNE_BAND_PAIR] as tune_from_env encodes the three overrides (0: entry not set, else value + 1)"""
    kw = {k: v for k, v in (("tb_lean", tb_lean), ("band_pair", band_pair), ("band_narrow", band_narrow)) if v is not None}
    old = {k: os.environ.pop(k, None) for k in ("POA_TB_LEAN", "POA_BAND_PAIR", "POA_BAND_NARROW")}
    try:
        cfg = _lib.tune_from_env(None, **kw)
    finally:
        os.environ.update({k: v for k, v in old.items() if v is not None})
    return 0 if cfg is None else int(cfg.tune[_lib.TUNE_KEYS.index("BAND_PAIR")])


def test_override_rides_in_the_band_pair_entry():
    hdr = open(os.path.join(ROOT, "include", "poasta_amd_tb.h")).read()
    assert "#define POA_TB_LEAN_SHIFT %d" % TB_LEAN_SHIFT in hdr and _lib.TB_LEAN_SHIFT == TB_LEAN_SHIFT
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    assert '#include "poasta_amd_tb.h"' in main_h
    import re
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(_lib.EXPORTS_TB)
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, s) for s in declared)
    # nothing set: the entry stays unset; the override alone: pairing "by the rule" (2), narrow tier "by the rule" (0)
    assert _pair_word(None) == 0
    assert _pair_word(0) == (2 | 1 << TB_LEAN_SHIFT) + 1 and _pair_word(1) == (2 | 2 << TB_LEAN_SHIFT) + 1
    # beside the other two riders
    assert _pair_word(1, band_pair=1) == (1 | 2 << TB_LEAN_SHIFT) + 1
    assert _pair_word(0, band_pair=0, band_narrow=1) == (0 | 2 << 2 | 1 << TB_LEAN_SHIFT) + 1
    assert _pair_word(None, band_pair=1, band_narrow=0) == (1 | 1 << 2) + 1     # as before the override existed


@pytest.fixture(scope="module")
def lean_host():
    out = os.path.join(HOST_DIR, "libtb_lean_host.so")
    deps = [HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp"), os.path.join(CSRC, "poa_dense_plan.hpp"),
            os.path.join(ROOT, "include", "poasta_amd.h"), os.path.join(ROOT, "include", "poasta_amd_tb.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp")])
    X = C.CDLL(out)
    X.tb_lean_host.argtypes = [C.c_uint32] * 2 + [C.c_uint64] * 2 + [C.c_uint32] * 2 + [C.c_void_p] + [C.c_uint32] * 2 + [C.c_uint64, C.c_void_p]
    X.tb_lean_host.restype = None
    return X


def _cxx(X, costs, max_len, mpn, mode, full, words, count, max_pitch, plane_elems):
    out = (C.c_uint32 * 9)()
    X.tb_lean_host(costs[1], costs[2], max_len, mpn, mode, int(full), words, count, max_pitch, plane_elems, out)
    return tuple(out)


def test_cxx_rule_equals_restatement(lean_host):
    """over every launch-matrix case x {unset, POA_TB_LEAN=0, =1} x {dense, hybrid} x planes of {0, 2^32 - 1, 2^32} elements: the record
    v[0..7] is what it was (predict) and the trailing member is lean_of"""
    i_pair = _lib.TUNE_KEYS.index("BAND_PAIR")
    n_lean = n_generic = 0
    for c in LM.CASES:
        g, lengths = LM._graph(c.kind), LM._lengths(c)
        pred = LM._predict_itself(g, lengths, c.costs, tune=dict(c.tune), full_planes=c.full)
        want8 = LM._words_of(pred)[:8]
        for tb_lean in (None, 0, 1):
            for mode_name, mode in (("dense", 0), ("hybrid", 2)):
                for elems in (0, 2 ** 32 - 1, 2 ** 32):
                    words = LM._tune_words(dict(c.tune))
                    assert words[i_pair] == 0      # no case of the matrix sets the entry
                    words[i_pair] = _pair_word(tb_lean)
                    got = _cxx(lean_host, c.costs, max(lengths), LM.min_path_nodes(g), mode, c.full, words, pred["queries"],
                               max(LM.pitch_of(L) for L in lengths), elems)
                    want = lean_of(pred, mode_name, tb_lean, elems)
                    if mode == 0:
                        assert got[:8] == want8, (c.name, tb_lean, got, want8)
                    assert got[8] == int(want), (c.name, tb_lean, mode_name, elems, got)
                    n_lean += want
                    n_generic += not want
    assert n_lean > 20 and n_generic > 20


def test_tb_lean_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tb_lean_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tb_lean_host ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(a.score, b.score) and np.array_equal(a.flags, b.flags) and np.array_equal(a.pair_off, b.pair_off)
            and np.array_equal(a.pairs, b.pairs))


class Batch:
    """a graph, its reads and the oracle's dense batch, computed once and left unchanged"""
    def __init__(self, oracle, g, qs, costs=COSTS):
        self.g, self.qs, self.costs = g, [np.asarray(q, np.uint8) for q in qs], costs
        self.qseq, self.qoff = pack_queries(self.qs)
        self.oracle = oracle
        self.og = og = oracle.OracleGraph.from_csr(g.as_dict())
        self.D = og.dense_batch(self.qseq, self.qoff, oracle.Costs(*costs), threads=8)
        self._planes = {}

    def planes(self, i):
        """the oracle's M, I, D planes of read i, by node"""
        if i not in self._planes:
            orank = self.og.export_csr()["rank"]
            od = self.og.dense_align(self.qs[i], self.oracle.Costs(*self.costs), planes=True)
            self._planes[i] = tuple(od[k][orank].astype(np.int64) for k in ("M", "I", "D"))
        return self._planes[i]

    def pairs(self, i):
        o, n = int(self.D["pair_off"][i]), int(self.D["n_pairs"][i])
        return self.D["pairs"][o:o + n]

    def runs(self, i, col):
        """lengths of the maximal runs of pairs whose column `col` (0: node, 1: query position) is NONE, in walk order"""
        gap = self.pairs(i)[:, col] == NONE
        edges = np.flatnonzero(np.diff(np.concatenate(([0], gap.astype(np.int8), [0]))))
        return (edges[1::2] - edges[::2]).tolist()

    def check(self, engine, tune=None, workspace_bytes=0, kernels=("generic", "lean"), mode="dense", lanes=None):
        """the batch under POA_TB_LEAN=0 and =1: which kernel ran, the two results against each other and against the oracle"""
        rb = engine.ResidentBatch(self.g, self.qseq, self.qoff, workspace_bytes=workspace_bytes)
        try:
            res = []
            for lean, kernel in zip((0, 1), kernels):
                rb.run(engine.GapAffine(self.costs[0], self.costs[2], self.costs[1]), None, engine.make_config(mode, tb_lean=lean, **(tune or {})))
                info = rb.tb_info()
                assert info["kernel"] == kernel and info["walks"] == len(self.qs), (lean, info)
                if lanes is not None:
                    assert (info["lanes"], info["depth"]) == lanes, info
                res.append(rb.fetch())
            n = len(self.qs)
            assert _same(res[0], res[1]), ("lean != generic", tune, np.flatnonzero(res[0].flags != res[1].flags)[:8].tolist(),
                                           np.flatnonzero(np.diff(res[0].pair_off.astype(np.int64)) != np.diff(res[1].pair_off.astype(np.int64)))[:8].tolist())
            if mode == "dense":
                LM._assert_equals_oracle(res[1], self.D, n, "lean vs oracle %r" % (tune,))
            return rb.launches() if mode == "dense" else None, res[1]
        finally:
            rb.close()


def _walk_events(b, engine, i):
    """What the reference's backtrace meets on read i, restated from the oracle's planes and pairs alone -> {event: count}.
    The walk's position before every pair follows from the pairs (walk order, from the end cell): a pair (node, NONE) is a
    Deletion-state step in the node's row, a pair (NONE, qpos) an Insertion-state step at column qpos + 1 in the row of the next
    pair that names a node, a pair (node, qpos) a Match-state step.  Rows, chain rows and kept D rows are the engine's
    (poa_graph_node_rows) restated as tests/test_compact_planes.py does.
      d_phantom / i_phantom   a step whose opening predecessor lies BELOW the open target where no gap can open (phantom test)
      sic_bad                 an Insertion step that only extends and whose hop lands on an M value that is not that I value
      openi_always, child_eq  an Insertion step on a ROW_OPENI_ALWAYS row / on a row whose only child's symbol is the read's
      dext_kept, dext_flagc, dext_multi, dext_open, dext_above   the exit tbd_d_extends takes for a Deletion step on a chain row
      m_chain_run             the longest run of consecutive Match steps over chain rows (one diagonal)
      m_first_run             the Match steps over chain rows before the walk's first gap step
      m_at_row, m_at_col      (row, column) of the last Match step of the walk; m_last_run: the run of chain-row Match steps it ends"""
    from test_compact_planes import _kept_rows
    g, q, (x, o, e) = b.g, b.qs[i], b.costs
    L, INF = len(q), NONE
    rows = engine._device_graph(g).node_rows().astype(np.int64)
    node_of_row, kept = np.argsort(rows), _kept_rows(g, rows)
    preds = lambda v: g.predecessors(v).astype(np.int64)
    chain = lambda v: len(preds(v)) == 1 and rows[preds(v)[0]] + 1 == rows[v]
    M, I, D = b.planes(i)
    pairs = b.pairs(i).astype(np.int64)[::-1]      # the oracle stores an alignment front to back
    ev = {}
    hit = lambda k: ev.__setitem__(k, ev.get(k, 0) + 1)

    def dext(v, j, cs):
        if cs < e:
            return "under"
        tt, r = cs - e, rows[v] - 1
        while True:
            n = node_of_row[r]
            if M[n][j] > tt:
                return "above"
            if kept[r]:
                return "kept"
            if D[n][j] == M[n][j]:
                return "flagc"
            if not chain(n):
                return "multi"
            up = node_of_row[r - 1]
            if (j >= L or g.symbol[n] != q[j]) and M[up][j] != INF and M[up][j] + o + e == tt:
                return "open"
            if tt < e:
                return "under"
            tt, r = tt - e, r - 1

    j, run, best = L, 0, 0
    for k, (n, p) in enumerate(pairs):
        if n != NONE and p != NONE:
            run = run + 1 if chain(n) else 0
            best = max(best, run)
            ev["m_at_row"], ev["m_at_col"], ev["m_last_run"] = int(rows[n]), j, run
            j -= 1
            continue
        ev.setdefault("m_first_run", run)
        run = 0
        if n != NONE:
            cs = D[n][j]
            t_open = cs - o - e
            if j < L and g.symbol[n] == q[j] and any(M[pr][j] < t_open for pr in preds(n)):
                hit("d_phantom")
            if chain(n):
                hit("dext_" + dext(n, j, cs))
            continue
        later = pairs[k + 1:, 0]
        later = later[later != NONE]
        if len(later):
            v = later[0]
            cs, pm = I[v][j], M[v][j - 1]
            succ = g.successors(v).astype(np.int64)
            always = g.end in succ or len({int(g.symbol[s]) for s in succ}) >= 2
            open_i = always or (len(succ) > 0 and g.symbol[succ[0]] != q[j - 1])
            if always:
                hit("openi_always")
            elif len(succ) and g.symbol[succ[0]] == q[j - 1]:
                hit("child_eq")
            if pm != cs - o - e:
                if not open_i and pm < cs - o - e:
                    hit("i_phantom")
                if I[v][j - 1] == cs - e and pm != cs - e:
                    hit("sic_bad")
        j -= 1
    ev["m_chain_run"] = best
    return ev


def _plant_graph():
    """160 backbone nodes; SNP bubbles (one-node alleles) at 20 and 60; a two-node insertion branch after 40; sites whose next
    backbone node has 4, 5 and 8 predecessors (3, 4 and 7 one-node alleles beside the backbone's) at 80, 100, 120; a skip edge over
    130..133 (a deletion the graph knows)"""
    rng = np.random.default_rng(11)
    backbone = ACGT[rng.integers(0, 4, 160)]
    backbone[70:76] = ord("A")                     # a homopolymer: ties
    gb = GraphBuilder()
    ids = gb.add_path(backbone)
    alleles, nodes = {}, {"backbone": ids, "allele": {}}
    for p, k in ((20, 1), (60, 1), (80, 3), (100, 4), (120, 7)):
        alleles[p] = []
        nodes["allele"][p] = []
        for a in range(k):
            sym = int(ACGT[(int(np.searchsorted(ACGT, backbone[p])) + 1 + a) % 4]) if a < 3 else ord("N") + (a - 3)
            v = gb.add_node(sym)
            gb.add_edge(ids[p - 1], v)
            gb.add_edge(v, ids[p + 1])
            alleles[p].append(sym)
            nodes["allele"][p].append(v)
    b1, b2 = gb.add_node(ord("G")), gb.add_node(ord("T"))
    gb.add_edge(ids[40], b1); gb.add_edge(b1, b2); gb.add_edge(b2, ids[41])
    gb.add_edge(ids[129], ids[134])
    nodes["branch"] = (b1, b2)
    return gb.finish(), backbone, alleles, nodes


DEPTHS = (2, 7, 8, 15, 16, 31, 32, 63, 64)


def _plant_reads(backbone, alleles):
    """name -> read.  Deletions are cut out of, insertions put into the backbone's own sequence far from the bubbles."""
    B = backbone
    rng = np.random.default_rng(12)
    reads = {"plain": B.copy(), "empty": B[:0], "L1": B[:1], "L2": B[:2], "L3": B[:3], "L4": B[:4],
             "L3_foreign": np.frombuffer(b"NNN", np.uint8), "L1_foreign": np.frombuffer(b"N", np.uint8),
             "non_acgt": np.where(np.arange(160) % 17 == 5, ord("N"), B).astype(np.uint8)}
    for k in (1, 2, 3) + tuple(d + 1 for d in DEPTHS if d + 1 < 60):
        reads["del_%d" % k] = np.concatenate((B[:85], B[85 + k:]))
    ins = lambda k: ACGT[rng.integers(0, 4, k)]
    for k in (1, 2, 3, 9, 17, 33, 65, 75):
        reads["ins_%d" % k] = np.concatenate((B[:50], ins(k), B[50:]))
        reads["ins_tail_%d" % k] = np.concatenate((B, ins(k)))
    reads["ins_start_5"] = np.concatenate((ins(5), B))
    reads["ins_start_12"] = np.concatenate((B[:1], ACGT[np.random.default_rng(14).integers(0, 4, 12)], B[1:]))      # the run ends at column 1, in the graph's first row
    reads["ins_start_40"] = np.concatenate((ins(40), B[30:]))
    reads["ins_same_symbol"] = np.concatenate((B[:50], np.full(4, B[50], np.uint8), B[50:]))      # the child symbol equals the inserted one
    reads["ins_homopolymer"] = np.concatenate((B[:72], np.full(3, ord("A"), np.uint8), B[72:]))   # ties along the A run
    for p in (20, 60, 80, 100, 120):                 # through the last allele of each site, and through the backbone's
        r = B.copy(); r[p] = alleles[p][-1]
        reads["allele_%d" % p] = r
    r = B.copy(); r[20] = ord("N")
    reads["snp_tie_20"] = r                          # neither allele matches: two predecessors tie
    reads["branch"] = np.concatenate((B[:41], np.frombuffer(b"GT", np.uint8), B[41:]))
    reads["skip"] = np.concatenate((B[:130], B[134:]))
    reads["del_into_bubble"] = np.concatenate((B[:76], B[82:]))     # a deletion run across the site at 80 (a non-chain row, kept D rows)
    reads["del_at_end"] = B[:150]
    reads["del_at_start"] = B[12:]
    reads["start_quirk"] = B[5:]                    # the walk reaches column 0 on the row of B[4], whose symbol is the read's first
    reads["start_quirk_17"] = B[17:]
    # found with the oracle on the CPU among random edits of the backbone: walks on which tbd_d_extends leaves by an open, and
    # walks whose only ambiguity is the "sic" hop landing on an M value that is not the I value (asserted below)
    e = lambda *parts: np.concatenate([np.frombuffer(x, np.uint8) if isinstance(x, bytes) else x for x in parts])
    reads["dext_open_a"] = e(B[:7], b"TGAGATTTGTCAGCGTCTACTAGCGTTTGTTAACGTCTCTGGAGTTTTATCGCTAATTAAAGTTAGAAACCGCCTGGGCTACAATACTGTAGTGACAATTCATAGACTCCATACAATACCAGGTATAAGTTGACTGAGAGACCTGGCCTTAAC")
    reads["dext_open_b"] = e(B[:16], b"CTTGTCAGCGTCTACTAGCGTTTGTTAACGTCTCTGGAGTTTTATCGCAACCAAAGTTAGAAACCGCCTGGGCTACAATACTGTACAATAGACTCCATACAATACCAGGTATAAGTTGACTGAGAGACCTGGCCTTAAC")
    reads["sic_bad_a"] = e(b"AATCAACGGGACACTGAGATTTGTCAGCGTCTACTAGCGTTTGTTATACACACGTCTCTGGAGTTTTATCGCAATTCCAAAAAAGTTAGAAAGCGCCTGGGCTACAATACTGTACAATAGACTCCATACAAGGTATAAGTTGACTGAGAGACCTGGCCTTAAC")
    reads["sic_bad_b"] = e(b"AATCGGGACACTGAGATTTGTCAGCGTTAGTCTAGCGTTTGTTAACGTCTCTGGAGTTTTATCGCAATTCCAAAAAAGTTAGAAACCGCCTGGGCTACAATACTGTACACGATAGACTCCATACAATACCAGGTATAAGTTGACTGAGCGACCTGGCCTTAAC")
    return reads


_cache = {}


def _plants(oracle, costs=COSTS):
    if ("plants", costs) not in _cache:
        g, backbone, alleles, _ = _plant_graph()
        plain = _plant_reads(backbone, alleles)
        # cells of code_fmt 4 are those of the one-strip kernel, which runs where the chunk's widest plane row has more than 512
        # columns: a read with a tail of 400 inserted bases after every sixth read, so that every chunk of a split run has one
        rng = np.random.default_rng(13)
        reads = {}
        for k, (name, q) in enumerate(plain.items()):
            if k % 6 == 0:
                reads["wide_%d" % k] = np.concatenate((backbone[:100 + k], ACGT[rng.integers(0, 4, 400 + k)], backbone[100 + k:]))
            reads[name] = q
        _cache["plants", costs] = (Batch(oracle, g, list(reads.values()), costs), list(reads))
    return _cache["plants", costs]


@pytest.mark.gpu
def test_plants_do_what_their_names_say(engine, oracle):
    b, names = _plants(oracle)
    at = {n: i for i, n in enumerate(names)}
    fl = lambda n: int(b.D["flags"][at[n]])
    for k in (1, 2, 3) + tuple(d + 1 for d in DEPTHS if d + 1 < 60):
        assert k in b.runs(at["del_%d" % k], 1), (k, b.runs(at["del_%d" % k], 1))
    for k in (1, 2, 3, 9, 17, 33, 65, 75):
        assert max(b.runs(at["ins_%d" % k], 0)) == k and b.runs(at["ins_tail_%d" % k], 0)[0] == k, k     # (the tail run is walked first)
    assert sum(b.runs(at["ins_start_40"], 0)) >= 5 and b.D["score"][at["ins_start_5"]] > 0
    assert sum(b.runs(at["ins_same_symbol"], 0)) == 4 and sum(b.runs(at["ins_homopolymer"], 0)) == 3
    assert fl("snp_tie_20") & AMBIGUOUS and fl("del_into_bubble") & AMBIGUOUS
    assert b.D["score"][at["plain"]] == 0 and fl("plain") == 0
    for p in (20, 60, 80, 100, 120):
        assert b.D["score"][at["allele_%d" % p]] == 0, p          # the walk goes through the planted allele, not the backbone's
    assert b.D["score"][at["branch"]] == 0 and b.D["score"][at["skip"]] == 0
    assert 6 in b.runs(at["del_into_bubble"], 1) or sum(b.runs(at["del_into_bubble"], 1)) >= 5
    assert b.runs(at["del_at_end"], 1)[0] == 10 and b.runs(at["del_at_start"], 1)[-1] == 12
    assert fl("L1") & SHORT_QUERY and fl("L1_foreign") & SHORT_QUERY and b.D["n_pairs"][at["empty"]] == 0
    assert fl("start_quirk") == START_QUIRK and fl("start_quirk_17") == START_QUIRK
    flags = np.bitwise_or.reduce(b.D["flags"])
    assert flags & AMBIGUOUS and flags & SHORT_QUERY
    assert max(b.runs(at["wide_0"], 0)) >= 390 and max(len(q) for q in b.qs) + 1 > 512
    # ---- from the walk's positions and the oracle's planes (_walk_events)
    _, _, _, nodes = _plant_graph()
    ev = {n: _walk_events(b, engine, at[n]) for n in names if not n.startswith("wide_")}
    has = lambda n, k: ev[n].get(k, 0) > 0
    # the four exits of tbd_d_extends (and the plain "no": the M value above the target), each on a Deletion step of the walk
    for exit_, reads in (("kept", ("del_into_bubble", "del_17")), ("flagc", ("del_2", "del_3", "del_9")), ("multi", ("del_at_start",)),
                         ("open", ("dext_open_a", "dext_open_b")), ("above", ("del_1", "del_at_end"))):
        for n in reads:
            assert has(n, "dext_" + exit_), (exit_, n, ev[n])
    assert fl("dext_open_a") == 0      # ... on a walk that nothing else flags
    # insertion runs: on a ROW_OPENI_ALWAYS row (the last backbone row has the edge to the end), on a row whose only child's symbol
    # is the inserted base, and one whose "sic" hop sets `bad` with nothing else ambiguous on the walk
    for k in (1, 2, 3, 9, 17, 33, 65, 75):
        assert ev["ins_tail_%d" % k]["openi_always"] == k, (k, ev["ins_tail_%d" % k])
    assert all(has("ins_%d" % k, "child_eq") for k in (9, 17, 33, 65, 75))
    for n in ("sic_bad_a", "sic_bad_b"):
        assert has(n, "sic_bad") and fl(n) == AMBIGUOUS and not has(n, "d_phantom") and not has(n, "i_phantom"), (n, ev[n], fl(n))
    assert not any(has(n, "sic_bad") for n in ev if fl(n) == 0)          # the restatement agrees with the oracle's flags
    # an insertion run at the start of the read: twelve inserted bases after the first one to three, so that the cycle ramp (2, 2, 4, 8
    # cycles) is cut by the column (cj < idepth) before the run ends at column 1 to 3
    first = b.pairs(at["ins_start_12"])
    k0 = int(np.flatnonzero(first[:, 0] == NONE)[0])
    assert 1 <= k0 <= 3 and b.runs(at["ins_start_12"], 0) == [12] and first[k0, 1] == k0 and first[k0 + 12, 0] != NONE, first[:16]
    # ... and after it the Match run reaches the first row at column 6: crow + 1 < cj + 1, the row bound cuts the last prefixes
    assert ev["ins_start_5"]["m_at_row"] <= 2 and ev["ins_start_5"]["m_at_col"] == 6 and ev["ins_start_5"]["m_last_run"] >= 8
    # a Match run that reaches column 0 twelve rows below the start: cj + 1 < crow + 1, the column bound cuts the last prefixes
    assert ev["del_at_start"]["m_at_col"] == 1 and ev["del_at_start"]["m_at_row"] >= 13 and ev["del_at_start"]["m_last_run"] >= 8
    assert ev["plain"]["m_at_col"] == 1 and ev["plain"]["m_at_row"] <= 2       # both at once
    # bubbles: the walk names the planted allele's node, the plain read the backbone's, and of the two one lies one row and the
    # other two rows above the row they merge into
    rows = engine._device_graph(b.g).node_rows().astype(np.int64)
    on_walk = lambda n: set(b.pairs(at[n])[:, 0].tolist())
    for p in (20, 60, 80, 100, 120):
        allele, back, merge = nodes["allele"][p][-1], nodes["backbone"][p], nodes["backbone"][p + 1]
        assert allele in on_walk("allele_%d" % p) and back not in on_walk("allele_%d" % p), p
        assert back in on_walk("plain") and allele not in on_walk("plain"), p
        assert len(b.g.predecessors(merge)) == {20: 2, 60: 2, 80: 4, 100: 5, 120: 8}[p]
    for p in (20, 60):
        allele, back, merge = nodes["allele"][p][-1], nodes["backbone"][p], nodes["backbone"][p + 1]
        assert {int(rows[merge] - rows[allele]), int(rows[merge] - rows[back])} == {1, 2}, p
    assert set(nodes["branch"]) <= on_walk("branch") and not set(nodes["branch"]) & on_walk("plain")
    assert not {nodes["backbone"][k] for k in (130, 131, 132, 133)} & on_walk("skip") and b.runs(at["skip"], 1) == []
    # the tie: both alleles of the site mismatch, the first predecessor in trait order is taken
    merge = nodes["backbone"][21]
    assert int(b.g.predecessors(merge)[0]) in on_walk("snp_tie_20") and int(b.g.predecessors(merge)[1]) not in on_walk("snp_tie_20")


@pytest.mark.gpu
@pytest.mark.parametrize("gw", [8, 16, 32, 64])
@pytest.mark.parametrize("depth", ["1", "2", "gw-1", "gw"])
def test_every_instantiation_and_depth(engine, oracle, gw, depth):
    b, _ = _plants(oracle)
    d = {"1": 1, "2": 2, "gw-1": gw - 1, "gw": gw}[depth]
    launches, _ = b.check(engine, dict(tb_group=gw, tb_depth=d, band=0), lanes=(gw, d))
    assert len(launches) == 1 and launches[0]["code_fmt"] == 4 and launches[0]["tb_lanes"] == gw and launches[0]["kernel"] == "px"
    # the chain runs of depth - 1, depth and depth + 1 rows (test_chain_runs_are_what_their_names_say)
    launches, _ = _chain(oracle).check(engine, dict(tb_group=gw, tb_depth=d, band=0), lanes=(gw, d))
    assert len(launches) == 1 and launches[0]["code_fmt"] == 4


@pytest.mark.gpu
def test_default_rule_takes_the_lean_kernel(engine, oracle):
    b, _ = _plants(oracle)
    rb = engine.ResidentBatch(b.g, b.qseq, b.qoff)
    # the rule is what runs with no override: every POA_* selection variable of the session is set aside for this run
    aside = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("POA_") and k != "POA_LIB_PATH"}
    try:
        rb.run(engine.GapAffine(4, 2, 6))
        assert rb.tb_info() == {"kernel": "lean", "lanes": 64, "depth": 32, "walks": len(b.qs)}
        LM._assert_equals_oracle(rb.fetch(), b.D, len(b.qs), "default rule")
    finally:
        os.environ.update(aside)
        rb.close()


PANIC_COSTS = (3, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("gw,depth", [(64, 32), (32, 32), (16, 16), (16, 1)])
def test_reference_panic_mid_walk(engine, oracle, gw, depth):
    """mismatch 3, open 1, extend 1: a cell the walk enters with score 2 = one inserted base on a row whose symbol is not the
    read's wraps `score - mismatch` onto u32::MAX, where the reference dies: the steps before it stand, REF_PANIC | TRUNCATED.
    Cells of score 2 off the path meet speculating lanes in the same batch: they must not count."""
    b, names = _plants(oracle, PANIC_COSTS)
    fl = b.D["flags"]
    n_panic = int(((fl & REF_PANIC) != 0).sum())
    assert 3 <= n_panic < len(names) - 10, n_panic                          # some walks die, most do not
    assert any((fl[i] & REF_PANIC) and b.D["n_pairs"][i] > 40 for i in range(len(names)))     # ... mid-walk, after many steps
    assert all(fl[i] & TRUNCATED for i in range(len(names)) if fl[i] & REF_PANIC)
    b.check(engine, dict(tb_group=gw, tb_depth=depth, band=0), lanes=(gw, depth))


def _headline_like(n, seed=2):
    """reads of the headline's kind (1 kbp, ~75 inserted bases at the tail) on its graph, scaled down"""
    return W.scaled_linearish(560, 28, 14, n, 600, query_seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("gw,n", [(32, 1), (32, 7), (16, 1), (16, 13), (16, 33), (8, 9)])
def test_groups_that_diverge(engine, oracle, gw, n):
    """several walks per wave in different states: plain reads next to reads with long planted deletion and insertion runs and to
    very short ones (walks that finish hundreds of rounds apart); n = 1 and n = 4k + 1 leave the last wave partly empty"""
    b = _diverge_batch(oracle, n)
    b.check(engine, dict(tb_group=gw, band=0), lanes=(gw, 16 if gw == 16 else 32))


def _diverge_batch(oracle, n):
    key = ("diverge", n)
    if key not in _cache:
        g, (qseq, qoff) = _headline_like(max(n, 4))
        base = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(max(n, 4))]
        rng = np.random.default_rng(7)
        qs = []
        for i in range(n):
            q = base[i % len(base)]
            kind = i % 4
            if kind == 1:
                q = np.concatenate((q[:100], q[160:]))                           # a deletion run of ~60 rows
            elif kind == 2:
                q = np.concatenate((q[:150], ACGT[rng.integers(0, 4, 70)], q[150:]))   # an insertion run of 70 bases
            elif kind == 3:
                q = q[:3 + i % 5] if i % 8 == 3 else q[:520 + i]                   # a few bases: the walk is one long deletion run, done in a few rounds
            qs.append(q)
        if n == 1:
            qs = [np.concatenate((base[0][:100], base[0][160:400], ACGT[rng.integers(0, 4, 70)], base[0][400:]))]
        assert max(len(q) for q in qs) + 1 > 512
        _cache[key] = Batch(oracle, g, qs)
    b = _cache[key]
    if n >= 4:
        assert max(b.runs(1, 1)) >= 50 and max(b.runs(2, 0)) >= 50 and max(b.runs(3, 1)) >= 300 and max(b.runs(0, 1)) < 10    # the states are there
    else:
        assert max(b.runs(0, 1)) >= 50 and max(b.runs(0, 0)) >= 50
    return b


CHAIN_RUNS = sorted({k for d in DEPTHS for k in (d - 1, d, d + 1) if k >= 1})


def _chain(oracle):
    """a 600-row chain; the whole read, two reads with one deleted row, a read that stops 70 rows early, and for every depth
    tested a read whose walk matches exactly depth - 1, depth and depth + 1 chain rows before its one deviation (a deleted row)"""
    if "chain" not in _cache:
        rng = np.random.default_rng(5)
        seq = ACGT[np.cumsum(rng.integers(1, 4, 600)) % 4]      # no two neighbours alike: a deleted row has one place
        gb = GraphBuilder()
        gb.add_path(seq)
        qs = [seq, seq[:530], np.concatenate((seq[:64], seq[65:])), np.concatenate((seq[:535], seq[536:]))]
        qs += [np.concatenate((seq[:600 - k - 1], seq[600 - k:])) for k in CHAIN_RUNS]
        _cache["chain"] = Batch(oracle, gb.finish(), qs)
    return _cache["chain"]


@pytest.mark.gpu
def test_chain_runs_are_what_their_names_say(engine, oracle):
    b = _chain(oracle)
    assert b.D["score"][0] == 0 and b.D["n_pairs"][0] == 600 and b.runs(2, 1) == [1] and b.runs(3, 1) == [1]
    assert _walk_events(b, engine, 0)["m_chain_run"] == 600          # one diagonal over 600 chain rows: p == GW at every width
    for i, k in enumerate(CHAIN_RUNS, 4):
        ev = _walk_events(b, engine, i)
        assert ev["m_first_run"] == k and b.runs(i, 1) == [1] and b.D["flags"][i] == 0, (k, ev, b.runs(i, 1))


@pytest.mark.gpu
def test_whole_group_accepted(engine, oracle):
    """p == GW == 64: a read that matches a chain of more than 64 rows, at depth 64 (the sentinel of the prefix count)"""
    b = _chain(oracle)
    assert b.D["score"][0] == 0 and b.D["n_pairs"][0] == 600
    b.check(engine, dict(tb_group=64, tb_depth=64), lanes=(64, 64))


def _band_batch(engine, oracle):
    from test_band_narrow import NarrowBatch
    if "band" not in _cache:
        g, (qseq, qoff) = W.scaled_linearish(560, 28, 14, 8, 600)
        full = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(8)]
        assert min(len(q) for q in full) >= 540
        rng = np.random.default_rng(3)
        sub = lambda q, k: _substituted(rng, q, k)
        qs = [full[0][:540], full[1][:540], sub(full[2][:540], 40), full[3][:540], sub(full[4][:540], 40), sub(full[5][:540], 150),
              sub(full[6][:540], 420), full[7][:540]]
        _cache["band"] = NarrowBatch(engine, oracle, g, qs)
    return _cache["band"]


@pytest.mark.gpu
def test_band_tiers_in_one_batch(engine, oracle, harness):
    """reads the narrow tier certifies, reads the 512 pass certifies and reads the full pass recomputes, in one chunk under
    POA_BAND_PAIR=1 POA_BAND_NARROW=1: outside the windows of the first two kinds lies whatever the workspace held.  Which tier
    certifies a read is restated from the two band plans' D and the oracle's score (tests/test_band_narrow.py::_tiers), the pairs
    from the lengths (tests/test_band_pairs.py::_pairing)"""
    from test_band_narrow import ENV, _tiers
    from test_band_pairs import _pairing
    b = _band_batch(engine, oracle)
    tiers, _, _ = _tiers(b, harness, COSTS, 1 << 30)
    pairs, singles = _pairing([len(q) for q in b.qs], {len(q): b.plan(harness, len(q)).D for q in b.qs})
    assert {"narrow", "wide", "full"} <= set(tiers) and singles == [], (tiers, singles)
    assert any(tiers[a] != tiers[c] for a, c in pairs), (tiers, pairs)          # a pair whose members differ in tier
    rb = b.open()
    try:
        res = {}
        for lean in (0, 1):
            # other costs first: the workspace then holds stale values of another run everywhere
            b.run(rb, (3, 1, 1), {"POA_BAND": "0", "POA_TB_LEAN": str(lean)})
            res[lean] = b.run(rb, COSTS, dict(ENV, POA_TB_LEAN=str(lean)))
            assert rb.tb_info()["kernel"] == ("generic", "lean")[lean]
            b.check_results()
        assert _same(res[0], res[1])
    finally:
        rb.close()


def _substituted(rng, q, n):
    q = q.copy()
    at = rng.choice(len(q), n, replace=False)
    q[at] = ACGT[(np.searchsorted(ACGT, q[at]) + rng.integers(1, 4, n)) % 4]
    return q


@pytest.mark.gpu
def test_second_chunk(engine, oracle):
    """a workspace that holds a third of the batch: chunks with first_query != 0"""
    b, _ = _plants(oracle)
    # a compact query holds between 2.5 and 4.5 bytes per row and pitch column (test_dense_launch_matrix.test_gpu_mixed_chunks)
    cols = [LM.pitch_of(len(q)) for q in b.qs]
    assert sum(cols) // 3 > 2 * max(cols)
    launches, _ = b.check(engine, dict(tb_group=16, band=0), workspace_bytes=int(b.g.n * 3.5 * (sum(cols) // 3)))
    assert len(launches) >= 2 and sum(l["queries"] for l in launches) == len(b.qs)


@pytest.mark.gpu
@pytest.mark.parametrize("name,tune,mode", [("mf1", dict(mf=1), "dense"), ("mf2", dict(mf=2), "dense"), ("mf0", dict(mf=0), "dense"),
                                            ("u32", dict(planes=32), "dense"), ("relative", dict(relative=1), "dense"), ("hybrid", {}, "hybrid")])
def test_ineligible_runs_keep_the_generic_kernel(engine, oracle, name, tune, mode):
    b, _ = _plants(oracle)
    b.check(engine, tune, kernels=("generic", "generic"), mode=mode)
