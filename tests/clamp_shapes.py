"""Graphs and reads whose dense planes hold FINITE values at and above the limit of the narrow cell format the launcher picks
for them, and the conditions a case must meet, from the oracle's planes alone, before any engine result is looked at.

The launcher bounds only the optimal score: ub = [o + e * L] + [o + e * min_path_nodes].  A cell exceeds ub only on a row whose
shortest-path depth is far above min_path_nodes: a long arm beside a short way through (a POA graph that has absorbed a read
with a large deletion).  arm_graph is that shape: a backbone of B nodes and, from backbone node a, a chain of A nodes that
rejoins at backbone node a + 1.  min_path_nodes stays B, so ub is that of the backbone alone, while the arm's rows are up to
a + A nodes deep: on them every cell is at least o + e * (depth - column), far above the format's limit.

The limits: 0xFFFF for u16 cells, 0x3FFF for the flags-in-score formats code_fmt 2 and 4, 0x0FFF for code_fmt 3.  Under each,
a value below the limit is stored exactly (with its flag bits); a value at or above it, or INF, reads as the limit."""
import functools
from collections import namedtuple

import numpy as np

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder

INF = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
LIMIT_U16, LIMIT_14, LIMIT_12 = 0xFFFF, 0x3FFF, 0x0FFF
# the launcher's bound on ub for each limit (poa_dense_plan.cpp): u16 cells, two flags beside the score, three flags
UB_BOUND = {LIMIT_U16: 65534, LIMIT_14: 16382, LIMIT_12: 4094}

Arm = namedtuple("Arm", "graph backbone ids arm_ids rejoin feeders")


@functools.lru_cache(maxsize=None)
def arm_graph(B, A, a, seed, into_end=False, arm_first=False, snp_every=0):
    """-> Arm(graph, backbone symbols, backbone node ids, arm node ids, rejoin node, (backbone feeder, arm feeder)).
    snp_every = k > 0: every k-th arm node gets a one-node SNP bubble beside it.  The bare arm is one chain, of which the compact
    layouts keep no D row but its last; the bubbles' rows have predecessors that are not the row above, so D rows all along the
    arm are kept (three per bubble) and the kept D rows hold clamped values too.
    into_end: the arm's last node gets no edge to backbone node a + 1; finish() makes it a second predecessor of the end node,
    whose deletion costs the plain e.  arm_first: the arm's edge into the rejoin node is listed before the backbone's in the
    predecessor order of the trait (GraphBuilder lists the most recently added edge first)."""
    assert 0 <= a < B - 1 and A >= 1
    rng = np.random.default_rng(seed)
    backbone = ACGT[rng.integers(0, 4, B)]
    arm = ACGT[rng.integers(0, 4, A)]
    gb = GraphBuilder()
    ids = [gb.add_node(int(c)) for c in backbone]
    arm_ids = [gb.add_node(int(c)) for c in arm]
    for k in range(B - 1):
        if k != a:
            gb.add_edge(ids[k], ids[k + 1])
    gb.add_edge(ids[a], arm_ids[0])
    for k in range(A - 1):
        gb.add_edge(arm_ids[k], arm_ids[k + 1])
    for p in range(snp_every, A - 1, snp_every) if snp_every else ():
        v = gb.add_node(int(ACGT[(int(np.searchsorted(ACGT, arm[p])) + 1 + int(rng.integers(0, 3))) % 4]))
        gb.add_edge(arm_ids[p - 1], v)
        gb.add_edge(v, arm_ids[p + 1])
    if into_end:
        gb.add_edge(ids[a], ids[a + 1])
        g = gb.finish()
        # finish() scans in ascending node index and lists the later edge first: the arm's last node comes first by itself
        rejoin, feeders = g.end, (ids[B - 1], arm_ids[-1])
        if not arm_first:      # list the backbone's edge first instead
            lo, hi = int(g.pred_off[g.end]), int(g.pred_off[g.end + 1])
            assert g.pred[lo:hi].tolist() == [arm_ids[-1], ids[B - 1]]
            g.pred[lo:hi] = g.pred[lo:hi][::-1]
    else:
        for s in ((ids[a], arm_ids[-1]) if arm_first else (arm_ids[-1], ids[a])):
            gb.add_edge(s, ids[a + 1])
        g = gb.finish()
        rejoin, feeders = ids[a + 1], (ids[a], arm_ids[-1])
    want = [feeders[1], feeders[0]] if arm_first else [feeders[0], feeders[1]]
    assert g.predecessors(rejoin).tolist() == want, (g.predecessors(rejoin).tolist(), want)
    return Arm(g, backbone, tuple(ids), tuple(arm_ids), rejoin, feeders)


VARIANTS = {"rejoin": {}, "into_end": {"into_end": True}, "arm_first": {"arm_first": True}}


WRAP_ARM = (880, 2100, 800)      # (B, A, a) of the variant "wrap"


def headline_arm(variant="rejoin"):
    """backbone 600, an arm of 2 500 nodes from backbone node 300 with a SNP bubble at every 25th: 3 201 rows, min_path_nodes 600.
    variant "wrap": backbone 880, an arm of 2 100 nodes from backbone node 800.  A value that wraps by 65 536 instead of
    saturating changes a RESULT only if the wrapped value is below what the backbone offers at the rejoin row, e * A < 65 536 + e,
    while the arm still passes the top of u16, e * (a + A) >= 65 536.  At e = 30 the headline arm (A = 2 500) is too long for that:
    its wrapped values stay above the backbone's.  This one is not: 30 * 2 100 = 63 000 (wrap_margin asserts it from the planes)."""
    if variant == "wrap":
        B, A, a = WRAP_ARM
        return arm_graph(B, A, a, 17, snp_every=25)
    return arm_graph(600, 2500, 300, 17, snp_every=25, **VARIANTS[variant])


def wrap_margin(M, feeders):
    """columns of the rejoin row's two predecessor rows (backbone feeder, arm feeder) of the oracle's M plane where the arm's value
    is finite, at least 65 536, and less 65 536 BELOW the backbone's: a value wrapped instead of saturated would win the minimum"""
    fb, fa = (np.asarray(M[r], np.int64) for r in feeders)
    return int(((fa != INF) & (fa >= 65536) & (fa - 65536 < fb)).sum())


# name: (arm length A, costs, read length): ub above 65534, 2 (o + e L) within it, and e * A just above 65535, so that an edge cost
# that wrapped instead of saturating would be a small number: the arm-tail read would then look cheaper through the arm
RELATIVE_SHAPES = {
    "one-strip": (1093, (4, 6, 60), 300),      # ub = 108 012, 2 (6 + 60 * 300) = 36 012, e * pred_k = 65 580
    "strips": (2622, (4, 6, 25), 1300),        # ub = 70 012, 2 (6 + 25 * 1300) = 65 012, e * pred_k = 65 550; two strips of 1024 columns
}


def relative_arm(shape="one-strip"):
    """backbone 1 500, an arm of A nodes from backbone node 700: the rejoin edge's offset in the relative encoding is pred_k = A"""
    return arm_graph(1500, RELATIVE_SHAPES[shape][0], 700, 19)


def relative_reads(shape):
    """a read along the backbone; a read that follows the arm's last L / 2 nodes and then the backbone from the rejoin node on (it
    matches the arm, but the way through the arm costs e * A more in deletions than the way past it); the empty read; one symbol"""
    arm = relative_arm(shape)
    L = RELATIVE_SHAPES[shape][2]
    rng = np.random.default_rng(29)
    read = np.concatenate([W.mutate(rng, arm.backbone[1500 - L - 100:], 0.05, 0.03, 0.03), ACGT[rng.integers(0, 4, L)]])[:L]
    tail = np.concatenate([arm.graph.symbol[np.array(arm.arm_ids[-(L // 2):])], arm.backbone[701:701 + L - L // 2]])
    return [read, tail, np.zeros(0, np.uint8), arm.backbone[:1].copy()]


@functools.lru_cache(maxsize=None)
def reads(variant="rejoin"):
    """the reads of the headline arm graph by name"""
    arm = headline_arm(variant)
    rng = np.random.default_rng(23)

    def read(n):      # the backbone with 5 % substitutions, 3 % insertions, 3 % deletions, random bases behind it, cut to n symbols
        return np.concatenate([W.mutate(rng, arm.backbone, 0.05, 0.03, 0.03), ACGT[rng.integers(0, 4, n)]])[:n]

    out = {
        "r600": read(600), "r600b": read(600), "r400": read(400), "r1300": read(1300),
        "n600": np.full(600, ord("N"), np.uint8),
        "empty": np.zeros(0, np.uint8),
        "one": arm.backbone[:1].copy(),
    }
    assert [len(out[k]) for k in ("r600", "r600b", "r400", "r1300")] == [600, 600, 400, 1300]
    return out


def score_ub(o, e, max_len, mpn):
    return (o + e * max_len if max_len else 0) + (o + e * mpn if mpn else 0)


def kept_rows(g, rows):
    """the D rows the compact layouts keep: the end row, and every predecessor of a non-chain row (a chain row has exactly
    one predecessor and it is the row right above); by engine row"""
    kept = np.zeros(g.n, bool)
    kept[rows[g.end]] = True
    for v in range(g.n):
        prs = rows[g.predecessors(v).astype(np.int64)]
        if not (len(prs) == 1 and prs[0] + 1 == rows[v]):
            kept[prs] = True
    return kept


Profile = namedtuple("Profile", "ub finite_m m_over d_over m_near mixed_rows rejoin_cols max_m score")


def clamp_profile(planes, limit, x, *, ub, kept, feeders, score):
    """planes: the oracle's (M, I, D) of one query, uint32 [row][column 0..L] with INF = 0xFFFFFFFF, in any row order; kept:
    bool per row, the D rows the format stores; feeders: the two predecessor rows of the rejoin row; x: the mismatch
    cost; ub and score: the launcher's bound and the optimal score.  Asserts the conditions of a clamped-cell case and returns
    the counts."""
    M, _, D = (np.asarray(p, np.int64) for p in planes)
    fin_m, fin_d = M != INF, (D != INF) & np.asarray(kept, bool)[:, None]
    m_over = int((fin_m & (M >= limit)).sum())
    d_over = int((fin_d & (D >= limit)).sum())
    m_near = int((fin_m & (M < limit) & (M + x >= limit)).sum())
    mixed = int(((fin_m & (M < limit)).any(axis=1) & (fin_m & (M >= limit)).any(axis=1)).sum())
    fa, fb = M[feeders[0]], M[feeders[1]]
    rejoin_cols = int((((fa >= limit) & (fb < limit)) | ((fb >= limit) & (fa < limit))).sum())
    prof = Profile(ub, int(fin_m.sum()), m_over, d_over, m_near, mixed, rejoin_cols, int(M[fin_m].max()), int(score))
    assert ub <= UB_BOUND[limit], prof
    assert m_over >= 10000, prof
    assert d_over >= 10000, prof
    assert m_near >= 50, prof
    assert mixed >= 1, prof
    assert rejoin_cols >= 1, prof
    assert score < limit, prof
    return prof


def expected_u16(plane):
    """what a u16 plane holds and reads back as, for the oracle's plane: the value if it is at most 65534, else INF"""
    plane = np.asarray(plane, np.uint32)
    return np.where(plane <= 65534, plane, np.uint32(INF))
