"""Dense and exact multi-graph batches with queries of more than 1023 symbols (POA_CFG_WIDE_QUERIES): a chunk with such a query
runs the strip loop of the packed forward pass (poa_forward_packed_multi_wide_kernel), every other chunk what it always ran.

Every comparison is equal, not close, on score, flags, pair_off and pairs, and has the three references of test_multi_dense:
the oracle's dense restatement, poa_align_batch_ex in POA_MODE_DENSE per graph, and the checkpointed MultiGraphBatch on the same
inputs (the exact kind: poa_align_batch_ex in the same mode per graph and the oracle's search, counters included)."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

import test_multi_dense as TMD
import test_multi_exact as TME
from test_multi_graph import ACGT, EMPTY_GRAPH, ERR_UNSUPPORTED, _bubble_graph, _costs, _oracle_case

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
STRIP = 1024   # columns of one strip; column j holds the query prefix of j symbols, so query position p sits in column p + 1


def _wide_record(queries):
    return dict(TMD._record(2, queries), strips=True)


def _chain(rng, n):
    b = GraphBuilder()
    seq = rng.choice(ACGT, n)
    b.add_path(seq)
    return b.finish(), seq


def _other(rng, base):
    return int(rng.choice([int(b) for b in ACGT if int(b) != int(base)]))


# ---- 1. strip edges ---------------------------------------------------------------------------------------------------------------
def test_multi_wide_strip_edges(engine, oracle):
    rng = np.random.default_rng(51)
    chain, chain_seq = _chain(rng, 118)
    bubble = _bubble_graph()
    assert chain.n == 120
    lens = (1023, 1024, 1025, 1535, 1536, 2047, 2048, 2100, 0, 1, 63)

    def query(seq, length):
        """random, with the graph's own sequence laid over the last strip boundary the query crosses (matches on both sides of it)"""
        q = rng.choice(ACGT, length)
        if length > 200 and seq is not None:
            at = min(max(length // STRIP, 1) * STRIP - len(seq) // 2, length - len(seq))
            q[at:at + len(seq)] = seq
        return q

    graphs = [chain, bubble]
    seqs = [[query(chain_seq, length) for length in lens], [query(None, length) for length in lens]]
    assert [len(q) for q in seqs[0]] == list(lens) and [len(q) for q in seqs[1]] == list(lens)
    costs = (4, 6, 2)
    res = TMD._run(engine, graphs, seqs, costs)
    assert res.launches == [_wide_record(2 * len(lens))]
    TMD._check(engine, oracle, res, "wide-edges", graphs, seqs, costs, "strip edges")
    # the one-shot entry point sets the flag by itself
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
    TMD._same(al.align_multi(graphs, seqs, mode="dense"), res, "one-shot")


# ---- 2. what crosses a strip boundary ---------------------------------------------------------------------------------------------
def _runs(aln, gap_side):
    """Maximal runs of gap pairs of one side (0: rpos is NONE, an insertion; 1: qpos is NONE, a deletion) in an alignment:
    (index of the first pair, length, query position of the last pair before the run that has one)."""
    out, i, last_q = [], 0, -1
    while i < len(aln):
        if aln[i][gap_side] == NONE:
            j = i
            while j < len(aln) and aln[j][gap_side] == NONE:
                j += 1
            out.append((i, j - i, last_q))
            for k in range(i, j):
                if aln[k][1] != NONE:
                    last_q = aln[k][1]
            i = j
        else:
            if aln[i][1] != NONE:
                last_q = aln[i][1]
            i += 1
    return out


def test_multi_wide_boundary_crossings(engine, oracle):
    rng = np.random.default_rng(52)
    chain, base = _chain(rng, 1150)
    # an insertion of 60 bases after query position 999: columns 1001 - 1060
    ins = np.concatenate([base[:1000], rng.choice(ACGT, 60), base[1000:1100]])
    # deletions of 30 nodes: one taken in column 1023 (the last of strip 0), one in column 1024 (the first of strip 1)
    del_a = np.concatenate([base[:1023], base[1053:1150]])
    del_b = np.concatenate([base[:1024], base[1054:1150]])
    # mismatches at query positions 1022 and 1023: columns 1023 and 1024
    mis = base[:1120].copy()
    mis[1022], mis[1023] = _other(rng, base[1022]), _other(rng, base[1023])
    graphs, seqs = [chain], [[ins, del_a, del_b, mis]]
    costs = (4, 6, 2)
    case = _oracle_case(oracle, "dense/wide-cross", graphs, seqs, costs)
    # each case covers its edge, by the oracle's own alignment
    aln = case[0][1]
    runs = [(aln[i][1], n) for i, n, _ in _runs(aln, 0)]   # (first query position, length)
    # (the run may slide by a base or two where the inserted bases equal their neighbours: columns 1001 - 1060, give or take)
    assert any(n >= 40 and q0 + 1 <= 1005 and q0 + n >= 1055 for q0, n in runs), ("the insertion run spans columns 1000 - 1060", runs)
    for k, column in ((1, 1023), (2, 1024)):
        runs = [(last_q + 1, n) for _, n, last_q in _runs(case[k][1], 1)]   # (column the deletions are taken in, length)
        assert (column, 30) in runs, ("the deletion run lies in column %d" % column, runs)
    sym = {int(r): int(q) for r, q in case[3][1] if r != NONE and q != NONE}
    by_q = {q: r for r, q in sym.items()}
    for p in (1022, 1023):
        assert p in by_q and chain.symbol[by_q[p]] != mis[p] and chain.symbol[by_q[p]] == base[p], ("a mismatch at column %d" % (p + 1), p)
    res = TMD._run(engine, graphs, seqs, costs)
    assert res.launches == [_wide_record(4)]
    TMD._check(engine, oracle, res, "wide-cross", graphs, seqs, costs, "boundary crossings")


# ---- 3. rows that read the edge column back from the plane ------------------------------------------------------------------------
def _far_graph(rng):
    """A backbone of 1150 nodes; three branches of 1, 2 and 4 nodes leave node 1012 and join at node 1026, which then has four
    predecessors, and an edge from node 1008 skips to node 1034.  Returns the graph, the backbone's sequence and node ids, and
    the sequence of the two-node branch."""
    b = GraphBuilder()
    seq = rng.choice(ACGT, 1150)
    back = b.add_path(seq)
    branch = {}
    for length in (1, 2, 4):
        branch[length] = rng.choice(ACGT, length)
        br = b.add_path(branch[length])
        b.add_edge(back[1012], br[0])
        b.add_edge(br[-1], back[1026])
    b.add_edge(back[1008], back[1034])
    return b.finish(), seq, back, branch[2]


def _msa_graph(rng):
    """Four haplotypes of 1160 columns from the MSA import: SNPs in the adjacent columns 1020 and 1021 in all four combinations
    (the two nodes of column 1021 are siblings: both have both nodes of column 1020 as predecessors), a deletion of columns
    1030 - 1039 in one haplotype, and an SNP in the last column (the end node has two predecessors)."""
    ref = rng.choice(ACGT, 1160)
    alt = lambda base, k: ACGT[(int(np.flatnonzero(ACGT == base)[0]) + k) % 4]
    rows = []
    for k in range(4):
        row = ref.copy()
        if k & 1:
            row[1020] = alt(ref[1020], 1)
        if k & 2:
            row[1021] = alt(ref[1021], 1)
        if k == 3:
            row[1030:1040] = ord("-")
        if k >= 2:
            row[-1] = alt(ref[-1], 2)
        rows.append(row)
    return W.msa_to_graph(rows), [r[r != ord("-")] for r in rows]


def test_multi_wide_rows_that_read_the_edge_column(engine, oracle):
    rng = np.random.default_rng(53)
    far, far_seq, back, branch2 = _far_graph(rng)
    msa, haps = _msa_graph(rng)
    empty = GraphBuilder().finish()
    # the structure the case is about, in terms of the engine's rows
    rows = engine._device_graph(far).node_rows()
    join, land = back[1026], back[1034]
    preds = [int(p) for p in far.predecessors(join)]
    assert len(preds) == 4 and min(int(rows[p]) for p in preds) < int(rows[join]) - 1, "a multi-predecessor row with predecessors more than one row back"
    assert len(far.predecessors(land)) == 2 and int(rows[land]) - int(rows[back[1008]]) > 1
    mrows = engine._device_graph(msa).node_rows()
    two = [v for v in range(msa.n) if v != msa.end and len(msa.predecessors(v)) == 2]
    sibs = [(a, b) for a in two for b in two if int(mrows[b]) == int(mrows[a]) + 1 and sorted(msa.predecessors(a)) == sorted(msa.predecessors(b))]
    assert len(sibs) == 1, "one sibling pair on adjacent rows with the same two predecessors (ROW_SAME_PREDS)"
    assert len(msa.predecessors(msa.end)) == 2, "a two-predecessor end row"
    # reads that reach those rows in column 1024, the first of strip 1 (query position 1023): a few extra bases in front
    mut = lambda s: W.mutate(rng, s, 0.01, 0.004, 0.004)
    via_branch = np.concatenate([rng.choice(ACGT, 8), far_seq[:1013], branch2, far_seq[1026:]])
    via_skip = np.concatenate([rng.choice(ACGT, 14), far_seq[:1009], far_seq[1034:]])
    via_sib = [np.concatenate([rng.choice(ACGT, 2), h]) for h in haps]
    graphs = [far, msa, empty]
    seqs = [[via_branch, via_skip, mut(far_seq)], via_sib + [mut(haps[3])], [rng.choice(ACGT, 1100), rng.choice(ACGT, 7)]]
    assert all(len(q) >= 1100 for qs in seqs[:2] for q in qs) and len(seqs[2][0]) == 1100
    costs = (4, 6, 2)
    case = _oracle_case(oracle, "dense/wide-rows", graphs, seqs, costs)
    at = lambda i, p: [int(r) for r, q in case[i][1] if q == p and r != NONE]
    assert at(0, 1023) == [join] and at(1, 1023) == [land], (at(0, 1023), at(1, 1023))
    hit = {at(3 + k, 1023)[0] for k in range(4)}
    assert hit == set(sibs[0]), ("both siblings are reached in column 1024", hit, sibs)
    res = TMD._run(engine, graphs, seqs, costs)
    n = sum(len(s) for s in seqs)
    assert res.launches == [_wide_record(n)]
    TMD._check(engine, oracle, res, "wide-rows", graphs, seqs, costs, "edge column read back")
    for i, q in zip((n - 2, n - 1), seqs[2]):
        assert res.flags[i] == EMPTY_GRAPH and res.score[i] == 4 * len(q) and res.raw_alignment(i) == []


# ---- 4. mixed chunks --------------------------------------------------------------------------------------------------------------
def test_multi_wide_mixed_chunks_and_reruns(engine, oracle):
    rng = np.random.default_rng(54)
    chain, chain_seq = _chain(rng, 118)
    bubble = _bubble_graph()
    rep = lambda length: np.resize(chain_seq, length)   # the chain's sequence over and over
    graphs = [chain, bubble, chain]
    seqs = [[W.mutate(rng, rep(1300), 0.05, 0.02, 0.02)[:1300]],
            [rng.choice(ACGT, 600), W.random_walk_query(rng, bubble, 0.2), rng.choice(ACGT, 600), rng.choice(ACGT, 580), rng.choice(ACGT, 0)],
            [rng.choice(ACGT, 590), W.mutate(rng, rep(1100), 0.05, 0.02, 0.02)[:1100], rep(30), W.mutate(rng, rep(1030), 0.1, 0.0, 0.0), rep(1023)]]
    costs = (4, 6, 2)
    terms = TMD._terms(engine, graphs, seqs)
    total, largest = engine.multi_footprint(graphs, seqs, dense=True)
    assert total == sum(t for _, t in terms) and largest == max(t for _, t in terms)
    cap = largest + 256
    firsts, used = [0], 0
    for i, (_, t) in enumerate(terms):
        if used + t > cap and i > firsts[-1]:
            firsts.append(i)
            used = 0
        used += t
    ends = firsts[1:] + [len(terms)]
    lens = [len(q) for s in seqs for q in s]
    wide = [max(lens[a:b]) > 1023 for a, b in zip(firsts, ends)]
    assert len(firsts) >= 3 and wide.count(False) >= 1 and wide.count(True) >= 2, (firsts, wide)
    expect = [_wide_record(b - a) if w else TMD._record(2 if max(lens[a:b]) + 1 > 512 else 1, b - a) for w, a, b in zip(wide, firsts, ends)]
    mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=cap, dense=True)
    try:
        assert mb.wide
        # the same flagged batch under three costs
        for cs in (costs, (1, 1, 1), (8, 3, 1)):
            mb.run(_costs(engine, *cs))
            res = mb.fetch()
            assert res.stats["n_chunks"] == len(firsts)
            assert mb.launches() == expect   # a chunk of short queries: today's record exactly, no "strips" key
            TMD._check(engine, oracle, res, "wide-mixed", graphs, seqs, cs, ("chunked", cs))
        assert mb.workspace_bytes() == max(sum(t for _, t in terms[a:b]) for a, b in zip(firsts, ends)) <= cap
    finally:
        mb.close()
    whole = TMD._run(engine, graphs, seqs, costs)
    assert whole.launches == [_wide_record(len(terms))]
    TMD._check(engine, oracle, whole, "wide-mixed", graphs, seqs, costs, "one chunk")


def test_multi_wide_flag_on_short_queries_changes_nothing(engine):
    graphs, seqs = TMD._mixed_dense()
    costs = (4, 6, 2)
    _, largest = engine.multi_footprint(graphs, seqs, dense=True)
    for ws in (0, largest + 256):
        out = []
        for wide in (None, True):
            mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=ws, dense=True, wide=wide)
            try:
                assert mb.wide == bool(wide)
                mb.run(_costs(engine, *costs))
                out.append((mb.fetch(), mb.launches(), mb.workspace_bytes()))
            finally:
                mb.close()
        TMD._same(out[0][0], out[1][0], ("wide=True, short queries", ws))
        assert out[0][1] == out[1][1] and out[0][2] == out[1][2]
        assert all("strips" not in rec for rec in out[1][1])


# ---- 5. the exact kind ------------------------------------------------------------------------------------------------------------
_EXACT = None


def _exact_case():
    """Three graphs with paths of about 1200 nodes (a chain, an SNP ladder, an MSA import) and reads of 1030 - 1200 symbols at
    1 - 2 % divergence from a path of their graph; one read per graph is an exact copy of a path."""
    global _EXACT
    if _EXACT is None:
        rng = np.random.default_rng(55)
        chain, chain_seq = _chain(rng, 1200)
        ladder, lpath = TME._ladder(rng, 590)
        msa, haps = _msa_graph(rng)
        mut = lambda s, length: W.mutate(rng, s, 0.01, 0.003, 0.003)[:length]
        graphs = [chain, ladder, msa]
        seqs = [[mut(chain_seq, 1200), chain_seq[:1030].copy()], [mut(lpath, 1100), lpath[:1181].copy()], [mut(haps[1], 1150), haps[2][:1040].copy()]]
        seqs = [[np.ascontiguousarray(q, np.uint8) for q in qs] for qs in seqs]
        assert all(1030 <= len(q) <= 1200 for qs in seqs for q in qs), [len(q) for qs in seqs for q in qs]
        _EXACT = (graphs, seqs)
    return _EXACT


@pytest.mark.parametrize("mode", ["exact", "hybrid"])
def test_multi_wide_exact_kind(engine, oracle, mode):
    graphs, seqs = _exact_case()
    costs = (4, 6, 2)
    n = sum(len(s) for s in seqs)
    res = TME._run(engine, graphs, seqs, costs, mode, "mingap", True)
    assert res.stats["n_chunks"] == 1
    assert len(res.launches) == 1 and res.launches[0]["strips"] is True and res.launches[0]["replay"] in ("lds", "generic")
    assert dict(res.launches[0], replay=None, strips=None) == dict(TMD._record(2, n), replay=None, strips=None)
    replayed = TME._check(engine, oracle, res, "wide-exact", graphs, seqs, costs, mode, "mingap", True, ("wide", mode))
    if mode == "exact":
        assert replayed == n
    else:
        assert 0 < replayed < n, "under hybrid the replayed set is neither empty nor everything"


# ---- 6. without the flag ----------------------------------------------------------------------------------------------------------
def test_multi_wide_is_an_opt_in(engine):
    from poasta_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(56)
    chain, _ = _chain(rng, 28)
    qseq, qoff = pack_queries([rng.choice(ACGT, 40), rng.choice(ACGT, 1024)])
    gq = np.array([0, 2], np.uint64)
    handles = (C.c_void_p * 1)(engine._device_graph(chain).handle)
    c = _lib.PoaCosts(4, 6, 2, 0)
    for create, one_shot, cfgs in ((L.poa_multi_create_dense, L.poa_align_multi_dense, (None, engine.make_config("dense"))),
                                   (L.poa_multi_create_exact, L.poa_align_multi_exact, (None, engine.make_config("exact"), engine.make_config("hybrid")))):
        for cfg in cfgs:
            ref = C.byref(cfg) if cfg is not None else None
            h = C.c_void_p()
            assert create(handles, 1, engine._p(gq), 0, engine._p(qseq), engine._p(qoff), ref, 0, C.byref(h)) == ERR_UNSUPPORTED
            assert b"1023 symbols" in L.poa_last_error() and not h.value
            score, flags, pair_off = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(3, np.uint64)
            pairs = np.zeros((2 * chain.n + 1100, 2), np.uint32)
            assert one_shot(handles, 1, engine._p(gq), C.byref(c), ref, engine._p(qseq), engine._p(qoff), engine._p(score), engine._p(pairs),
                            engine._p(pair_off), len(pairs), engine._p(flags), None, 0) == ERR_UNSUPPORTED
