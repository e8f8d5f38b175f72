"""The dense one-piece pass (poa_batch_run_ex in poasta_amd/csrc/poa_engine.hip, which launches what plan_dense_run and
plan_dense_chunk of poasta_amd/csrc/poa_dense_plan.cpp decide) at every kernel the rule can pick: the forward instantiations
(poa_forward_kernel, poa_forward_packed_kernel, poa_forward_px_kernel, poa_forward_pxmw_kernel, the banded pair) and the
traceback instantiations (u32 / u16 full planes, the compact one at 64 / 32 / 16 / 8 lanes per walk over every cell encoding).

CPU: the rule restated in plain Python (`predict`), held against hand-computed shapes; a case table (`CASES`) and a
test that the table reaches every launch site of REQUIRED_SITES, every (cell encoding, lanes per walk) pair of REQUIRED_TB and
the column edges of every kernel, so a trimmed table fails here rather than passing silently; the multi-wave hand-over graph
is checked for the edges it exists for (32 and 33 rows back, hundreds of rows back, more rows than the LDS ring holds).
The C++ rule itself, compiled for the host (tests/dense_plan_host), gives `predict`'s record, layout and band on the case
table, on the hand-computed shapes and on a grid over costs, path lengths, pitches, counts and overrides; the same harness
runs as a program of its own under the address and undefined-behaviour sanitizers.

GPU: one test per case.  Overrides travel as keyword arguments of make_config (poa_config_t.tune), never through os.environ.
What ran is read back with ResidentBatch.launches() (poa_batch_last_launch) and must equal `predict`; layout() and band_info()
must agree with it.  If the environment itself carries a POA_* selection variable (scripts/variant_sweep.sh), only those
launch-record assertions are skipped.  Score, flags and the full (rpos, qpos) list of every query equal
oracle.OracleGraph.dense_batch bit for bit.  Full-plane cases compare every M / I / D cell of chosen queries with
dense_align(..., planes=True) through node_rows; for u16 planes the test asserts, from the oracle alone, that every finite
cell is at most 65534, so no cell is exempt.

Every batch carries an empty, a one-base and a 100-base query and L + 1 in {63, 64, 65} beside the lengths at its kernel's own
column-group and strip width, so short rows run under the long kernel the chunk's widest pitch selects.

The two `count * strips >= 8192` rules (packed multi-wave quads with pxmw refused; u32 `wide`) are checked by count from both
sides, 4 095 and 4 096 two-strip queries, on a 7-row graph (30 M cells); the kernels they select are also reached by override
(fwd_quads) on the larger graphs."""
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd._lib import TUNE_KEYS
from poasta_amd.aligner import LAUNCH_KERNELS
from poasta_amd.graph import GraphBuilder, pack_queries

from test_two_piece_shapes import min_path_nodes

INF = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
MW_MAX_WAVES, ROW_NEAR, MW_RING = 16, 32, 64      # poa_kernels.hpp
SELECTION_KEYS = ("PLANES", "COMPACT", "PACKED", "RELATIVE", "PX", "MF", "MW", "PXMW", "FWD_QUADS", "FUSE_TB", "TB_GROUP", "TB_DEPTH",
                  "BAND", "BAND_DELTA")


def _ambient():
    """a POA_* selection variable is set for the whole session (scripts/variant_sweep.sh): the launcher may pick another kernel"""
    return any("POA_" + k in os.environ for k in SELECTION_KEYS)


# ---- the selection rule (plan_dense_run / plan_dense_chunk, poa_dense_plan.cpp), in plain Python ------------------------------
def pitch_of(L):
    return (L + 1 + 63) // 64 * 64


def mw_waves(strips):
    groups = (strips + MW_MAX_WAVES - 1) // MW_MAX_WAVES
    return (strips + groups - 1) // groups


def predict(g, lengths, costs, n_chunk_queries=None, tune=None, max_len=None, full_planes=False, mpn=None):
    """What poa_batch_run_ex launches for one chunk: `lengths` are the chunk's query lengths (their widest pitch decides),
    n_chunk_queries its query count (default len(lengths)), max_len the longest query of the whole BATCH (default
    max(lengths)): the score bound is the batch's.  costs = (mismatch, open, extend); tune = make_config's keyword overrides.
    mpn: the nodes on the graph's shortest start -> end path, where there is no graph object (g is None).
    Returns the dict ResidentBatch.launches() gives for the chunk plus "layout" (ResidentBatch.layout()), "band" (the banded
    pair ran), "cells" ("u16" / "u32"), "strip" (columns per strip) and "strips" (of the widest query)."""
    _, o, e = costs
    T = dict(tune or {})
    count = len(lengths) if n_chunk_queries is None else n_chunk_queries
    max_len = max(lengths) if max_len is None else max_len
    mpn = min_path_nodes(g) if mpn is None else mpn
    ub = (o + e * max_len if max_len else 0) + (o + e * mpn if mpn else 0)
    narrow = ub <= 65534 and T.get("planes") != 32
    compact = narrow and not full_planes
    if T.get("compact") == 0:
        compact = False
    packed = T.get("packed", 1) != 0
    rel_ub = 2 * (o + e * max_len)
    relative = (not narrow) and rel_ub <= 65534 and not full_planes and packed and "planes" not in T and "compact" not in T
    if "relative" in T:
        relative = T["relative"] != 0 and rel_ub <= 65534 and not full_planes and packed
    if relative:
        narrow = compact = True
    spec_depth = T["tb_depth"] if 1 <= T.get("tb_depth", 0) <= 64 else 12
    fuse = T.get("fuse_tb", 0) != 0
    qo = T.get("fwd_quads", 0)
    want_band = e > 0 and T.get("band", 1) != 0
    max_pitch = max(pitch_of(L) for L in lengths)
    out = dict(fuse=False, mw=False, waves=4, code_fmt=0, queries=count)
    band = derived = False
    if narrow:
        quads = 1 if max_pitch <= 512 else 2
        if qo in (1, 2):
            quads = qo
        if relative:
            quads = 2
        if compact and packed:
            mw = max_pitch > 512 * quads
            if "mw" in T:
                mw = mw and (T["mw"] != 0 or relative)
            px = max_pitch <= 1024 and quads == 2 and (not fuse or relative)
            if "px" in T:
                px = px and (T["px"] != 0 or relative)
            if px:
                mf = 0 if relative else (2 if ub <= 4094 else (1 if ub <= 16382 else 0))
                if "mf" in T:
                    mf = (3 if mf >= 1 else 0) if T["mf"] == 3 else min(mf, max(0, T["mf"]))
                elif mf >= 1:
                    mf = 3
                out["code_fmt"] = {3: 4, 2: 3, 1: 2, 0: 1}[mf]
                derived = mf == 3
                band = mf == 3 and want_band and max_pitch > 512
                out.update(kernel="band" if band else "px", quads=2)
                strip = 1024
            elif mw and (relative or (T["pxmw"] != 0 if "pxmw" in T else count * ((max_pitch + 1023) // 1024) >= 1024)):
                strip = 1024
                out.update(kernel="pxmw", quads=2, mw=True, code_fmt=1, waves=mw_waves((max_pitch + 1023) // 1024))
            elif mw:
                if not qo:
                    quads = 2 if count * ((max_pitch + 1023) // 1024) >= 8192 else 1
                strip = 512 * quads
                out.update(kernel="packed", quads=quads, mw=True, waves=mw_waves((max_pitch + strip - 1) // strip))
            else:
                strip = 512 * quads
                out.update(kernel="packed", quads=quads, fuse=fuse)
        elif compact:
            strip = 512 * quads
            out.update(kernel="forward", quads=quads)
        else:
            strip = 512 * quads
            out.update(kernel="forward", quads=quads, fuse=fuse)
    else:
        quads = 1 if max_pitch <= 256 else (2 if max_pitch <= 512 else 4)
        if qo in (1, 2, 4):
            quads = qo
        mw = max_pitch > 1024
        if "mw" in T:
            mw = mw and T["mw"] != 0
        if mw:
            s2, s4 = (max_pitch + 511) // 512, (max_pitch + 1023) // 1024
            g2, g4 = (s2 + MW_MAX_WAVES - 1) // MW_MAX_WAVES, (s4 + 9) // 10
            wide = 14 * g4 < 10 * g2 or count * s4 >= 8192
            if qo == 4:
                wide = True
            if qo == 2:
                wide = False
            quads = 4 if wide else 2
            strip = 256 * quads
            out.update(kernel="forward", quads=quads, mw=True, waves=(s4 + g4 - 1) // g4 if wide else (s2 + g2 - 1) // g2)
        else:
            strip = 256 * quads
            out.update(kernel="forward", quads=quads, fuse=fuse)
    if fuse and not relative and max_pitch <= 1024 and (not compact or packed):
        out.update(tb_lanes=0, tb_depth=spec_depth)
    else:
        tbg = 64 if count <= 6144 else (32 if count <= 12288 else 16)
        if T.get("tb_group") in (8, 16, 32, 64):
            tbg = T["tb_group"]
        depth = spec_depth if "tb_depth" in T else (16 if tbg == 16 else (32 if compact else spec_depth))
        out.update(tb_lanes=tbg if compact else 64, tb_depth=depth if compact else spec_depth)
    layout = set()
    if narrow:
        layout.add("u16")
    if compact:
        layout.add("compact")
    if relative:
        layout.add("relative")
    if derived:
        layout.add("derived_gaps")
    out.update(layout=layout, band=band, cells="u16" if narrow else "u32", strip=strip, strips=(max_pitch + strip - 1) // strip)
    return out


_predict_itself = predict       # (a test below runs test_selection_rule_restated with `predict` wrapped)
LAUNCH_KEYS = ("kernel", "quads", "fuse", "mw", "waves", "code_fmt", "tb_lanes", "tb_depth", "queries")


def launch_of(pred):
    return {k: pred[k] for k in LAUNCH_KEYS}


def site_of(p):
    """the launch of launch_forward / launch_band (poa_engine.hip) a prediction stands for, under the name it had as a site of poa_batch_run_ex"""
    if p["kernel"] == "forward":
        if p["mw"]:
            return "forward<%d,u32,MW>" % p["quads"]
        if "compact" in p["layout"]:
            return "forward<%d,u16,compact>" % p["quads"]
        return "LAUNCH_FWD(%d,%s)%s" % (p["quads"], p["cells"], ",fuse" if p["fuse"] else "")
    if p["kernel"] == "packed":
        return "packed<%d,%s,%s>" % (p["quads"], "true" if p["fuse"] else "false", "true" if p["mw"] else "false")
    if p["kernel"] == "px":
        return "px<%d>%s" % ({1: 0, 2: 1, 3: 2, 4: 3}[p["code_fmt"]], ",relative" if "relative" in p["layout"] else "")
    if p["kernel"] == "pxmw":
        return "pxmw" + (",relative" if "relative" in p["layout"] else "")
    return "band"


def tb_site_of(p):
    if p["tb_lanes"] == 0:
        return None
    if "compact" in p["layout"]:
        return "tb<u16,true,%d>" % p["tb_lanes"]
    return "tb<%s,false>" % p["cells"]


def tb_format_of(p):
    """the storage format the separate traceback reads"""
    if "relative" in p["layout"]:
        return "relative"
    if "compact" in p["layout"]:
        return p["code_fmt"]
    return p["cells"] + "-full"


REQUIRED_SITES = (
    {"LAUNCH_FWD(%d,u16)%s" % (q, f) for q in (1, 2) for f in ("", ",fuse")}
    | {"LAUNCH_FWD(%d,u32)%s" % (q, f) for q in (1, 2, 4) for f in ("", ",fuse")}
    | {"forward<1,u16,compact>", "forward<2,u16,compact>", "forward<2,u32,MW>", "forward<4,u32,MW>"}
    | {"packed<%d,%s>" % (q, v) for q in (1, 2) for v in ("false,false", "true,false", "false,true")}
    | {"px<0>", "px<1>", "px<2>", "px<3>", "px<0>,relative", "pxmw", "pxmw,relative", "band"})
REQUIRED_TB_SITES = {"tb<u32,false>", "tb<u16,false>", "tb<u16,true,64>", "tb<u16,true,32>", "tb<u16,true,16>", "tb<u16,true,8>"}
REQUIRED_TB = ({(f, lanes) for f in (0, 1, 2, 3, 4, "relative") for lanes in (64, 32, 16, 8)}
               | {("u16-full", 64), ("u32-full", 64)})


# ---- graphs and queries -----------------------------------------------------------------------------------------------------
MWG_N = 1160
MWG_SKIP_A = tuple(range(508, 516)) + tuple(range(1019, 1028))
MWG_FAR = ((10, 700), (510, 950), (1022, 1100))
MWG_SKIP_COLS = (511, 512, 513, 1023, 1024, 1025)    # s * W - 1, s * W, s * W + 1 for W = 512 (s = 1, 2) and W = 1024 (s = 1)


@functools.lru_cache(maxsize=None)
def _mw_graph():
    """(graph, backbone, ids): a Hamiltonian chain of MWG_N random bases (row distance == node distance) with edges of exactly
    32 and 33 rows (the first row the LDS ring does not serve, ROW_NEAR = 32), three far edges, and rows with two predecessors
    directly behind their targets."""
    rng = np.random.default_rng(7)
    backbone = ACGT[rng.integers(0, 4, MWG_N)]
    # no base around the skips' targets equals the base 31, 32 or 33 rows before it: a walk that takes the edge a -> a + d could
    # otherwise take the neighbouring edge (from a - 1, or from a + 1) at the same score, and the skip would not be on THE path
    for k in list(range(520, 570)) + list(range(1030, 1080)):
        backbone[k] = [c for c in ACGT.tolist() if c not in backbone[k - 33:k - 30].tolist()][0]
    b = GraphBuilder()
    ids = b.add_path(backbone)
    for a in MWG_SKIP_A:
        b.add_edge(ids[a], ids[a + 32])
        b.add_edge(ids[a], ids[a + 33])
    for s, t in MWG_FAR:
        b.add_edge(ids[s], ids[t])
    for t in (549, 550, 1061, 1062, 701, 951, 1101):
        b.add_edge(ids[t - 2], ids[t])
    return b.finish(), backbone, tuple(ids)


@functools.lru_cache(maxsize=None)
def _mw_queries():
    """-> (queries, [(query index, (source node, qpos), (target node, qpos))]): walks that take one skip edge each so that the
    target row's cell lies in column c of MWG_SKIP_COLS (the source's in c - 1: the edge column of a strip that starts at c),
    one walk per far edge (targets in columns 12, 512, 1024), plain walks of 1 160 and 2 160 bases, and the short queries."""
    _, bb, ids = _mw_graph()
    rng = np.random.default_rng(8)

    def noisy(q, keep):
        q = q.copy()
        for p in rng.choice(len(q), len(q) // 100, replace=False).tolist():
            if all(abs(p - k) > 6 for k in keep):
                q[p] = ACGT[(int(np.searchsorted(ACGT, q[p])) + 1 + int(rng.integers(0, 3))) % 4]
        return q

    qs, marks = [np.zeros(0, np.uint8), bb[:1].copy(), bb[300:400].copy()], []
    for c in MWG_SKIP_COLS:
        a = c - 2                                     # bases 0..a are columns 1..a + 1 = c - 1; the skip's target is column c
        assert a in MWG_SKIP_A
        for d in (32, 33):
            marks.append((len(qs), (ids[a], a), (ids[a + d], a + 1)))
            qs.append(noisy(np.concatenate([bb[:a + 1], bb[a + d:]]), (a,)))
    for s, t in MWG_FAR:
        marks.append((len(qs), (ids[s], s), (ids[t], s + 1)))
        qs.append(noisy(np.concatenate([bb[:s + 1], bb[t:]]), (s,)))
    qs.append(W.mutate(rng, bb, 0.02, 0.01, 0.01))
    qs.append(np.concatenate([W.mutate(rng, bb, 0.01, 0.005, 0.005), ACGT[rng.integers(0, 4, 1000)]])[:2160])
    return tuple(qs), tuple(marks)


@functools.lru_cache(maxsize=None)
def _tb_graph():
    """about 600 rows: SNP bubbles, two-node branches and edges that skip two to six backbone nodes (deletions)"""
    rng = np.random.default_rng(11)
    n = 520
    backbone = ACGT[rng.integers(0, 4, n)]
    b = GraphBuilder()
    ids = b.add_path(backbone)
    for i in range(4, n - 8, 9):
        kind = (i // 9) % 3
        if kind == 0:
            v = b.add_node(int(ACGT[rng.integers(0, 4)]))
            b.add_edge(ids[i - 1], v)
            b.add_edge(v, ids[i + 1])
        elif kind == 1:
            v1, v2 = b.add_node(int(ACGT[rng.integers(0, 4)])), b.add_node(int(ACGT[rng.integers(0, 4)]))
            b.add_edge(ids[i], v1)
            b.add_edge(v1, v2)
            b.add_edge(v2, ids[i + 1])
        else:
            b.add_edge(ids[i], ids[i + int(rng.integers(2, 7))])
    return b.finish(), backbone


@functools.lru_cache(maxsize=None)
def _tb_queries():
    """reads with substitutions, insertions and deletions that end in an insertion tail of 60 to 140 random bases; pitch 704"""
    _, bb = _tb_graph()
    rng = np.random.default_rng(12)
    qs = [np.zeros(0, np.uint8), bb[:1].copy(), bb[200:300].copy()]
    for k in range(9):
        q = W.mutate(rng, bb, 0.03, 0.01, 0.01)
        qs.append(np.concatenate([q, ACGT[rng.integers(0, 4, 60 + 10 * k)]])[:690])
    return tuple(qs)


@functools.lru_cache(maxsize=None)
def _poa(kind):
    if kind == "lin":      # 202 rows
        return W.LinearishPOA(180, 10, 5, seed=3)
    if kind == "small":    # 62 rows
        return W.LinearishPOA(54, 4, 1, seed=4)
    if kind == "tiny":     # 32 rows
        return W.LinearishPOA(26, 2, 1, seed=5)
    if kind == "seven":    # 7 rows: four backbone nodes and one SNP bubble
        return W.LinearishPOA(4, 1, 0, seed=6)
    raise KeyError(kind)


def _graph(kind):
    if kind == "mw":
        return _mw_graph()[0]
    if kind == "tb":
        return _tb_graph()[0]
    return _poa(kind).graph


@functools.lru_cache(maxsize=None)
def _queries(kind, lengths):
    """lengths: a tuple of query lengths, or None for the graph's own query set"""
    if kind == "mw":
        return _mw_queries()[0]
    if kind == "tb":
        return _tb_queries()
    poa = _poa(kind)
    return tuple(poa.queries(1, length=L, first=i)[0] if L else np.zeros(0, np.uint8) for i, L in enumerate(lengths))


# ---- the case table ---------------------------------------------------------------------------------------------------------
COSTS = (4, 6, 2)
SHORT = (0, 1, 100, 62, 63, 64)     # empty, one base, ~100 bases, L + 1 in {63, 64, 65}


def lens(*cols):
    """SHORT plus the queries whose L + 1 are `cols`"""
    return SHORT + tuple(c - 1 for c in cols)


Case = namedtuple("Case", "name kind lengths costs tune full planes")


def C_(name, kind, lengths, tune=None, full=False, planes=(), costs=COSTS):
    return Case(name, kind, lengths, costs, tuple(sorted((tune or {}).items())), full, tuple(planes))


def _cases():
    out = []
    u32 = {"planes": 32}
    # --- column edges: every kernel at its own column-group / strip width W: L + 1 in {W - 1, W, W + 1, 2W, 2W + 1} as far as the
    # kernel takes them.  planes: L + 1 of the queries whose M / I / D cells are compared
    out += [
        C_("fwd1-u16", "lin", lens(255, 256, 257, 511, 512), full=True, planes=(1, 64, 512)),
        C_("fwd1-u16-strips", "lin", lens(511, 512, 513, 1024, 1025, 1300), {"fwd_quads": 1}, full=True, planes=(513, 1025, 1300)),
        C_("fwd2-u16-strips", "lin", lens(511, 512, 513, 1023, 1024, 1025, 2048, 2049, 3100), full=True, planes=(1024, 1025, 2049, 3100)),
        C_("fwd1-u16-fuse", "lin", lens(511, 512), {"fuse_tb": 1}, full=True, planes=(512,)),
        C_("fwd2-u16-fuse", "lin", lens(511, 512, 513, 1023, 1024), {"fuse_tb": 1}, full=True, planes=(1024,)),
        C_("fwd2-u16-fuse-strips", "lin", lens(1024, 1025, 2048, 2049), {"fuse_tb": 1}, full=True, planes=(2049,)),
        C_("fwd1-u32", "lin", lens(255, 256), u32, planes=(1, 64, 256)),
        C_("fwd2-u32", "lin", lens(255, 256, 257, 511, 512), u32, planes=(257, 512)),
        C_("fwd4-u32", "lin", lens(511, 512, 513, 1023, 1024), u32, planes=(513, 1024)),
        C_("fwd1-u32-strips", "lin", lens(255, 256, 257, 512, 513, 700), {"planes": 32, "fwd_quads": 1, "mw": 0}, planes=(257, 513, 700)),
        C_("fwd2-u32-strips", "lin", lens(511, 512, 513, 1024, 1025, 1300), {"planes": 32, "fwd_quads": 2, "mw": 0}, planes=(1025, 1300)),
        C_("fwd4-u32-strips", "lin", lens(1023, 1024, 1025, 2048, 2049, 3100), {"planes": 32, "mw": 0}, planes=(1025, 2049, 3100)),
        C_("fwd1-u32-fuse", "lin", lens(255, 256), {"planes": 32, "fuse_tb": 1}, planes=(256,)),
        C_("fwd2-u32-fuse", "lin", lens(257, 511, 512), {"planes": 32, "fuse_tb": 1}, planes=(512,)),
        C_("fwd4-u32-fuse", "lin", lens(513, 1023, 1024), {"planes": 32, "fuse_tb": 1}, planes=(1024,)),
        C_("fwd4-u32-fuse-strips", "lin", lens(1024, 1025, 2048, 2049), {"planes": 32, "fuse_tb": 1, "mw": 0}, planes=(2049,)),
        C_("fwdc1", "lin", lens(255, 256, 511, 512), {"packed": 0}),
        C_("fwdc1-strips", "lin", lens(511, 512, 513, 1024, 1025, 1300), {"packed": 0, "fwd_quads": 1}),
        C_("fwdc2-strips", "lin", lens(511, 512, 513, 1023, 1024, 1025, 2048, 2049), {"packed": 0}),
        C_("fwd2-u32-mw", "lin", lens(511, 512, 513, 1024, 1025), u32, planes=(513, 1025)),
        C_("fwd4-u32-mw", "lin", lens(1023, 1024, 1025, 2048, 2049), {"planes": 32, "fwd_quads": 4}, planes=(1025, 2049)),
        C_("packed1", "lin", lens(255, 256, 511, 512)),
        C_("packed2", "lin", lens(511, 512, 513, 1023, 1024), {"px": 0}),
        C_("packed1-strips", "lin", lens(511, 512, 513, 1024, 1025, 1500), {"fwd_quads": 1, "mw": 0}),
        C_("packed2-strips", "lin", lens(1023, 1024, 1025, 2048, 2049, 3100), {"mw": 0}),
        C_("packed1-fuse", "lin", lens(511, 512), {"fuse_tb": 1}),
        C_("packed2-fuse", "lin", lens(511, 512, 513, 1023, 1024), {"fuse_tb": 1}),
        C_("packed2-fuse-strips", "lin", lens(1024, 1025, 2048, 2049), {"fuse_tb": 1, "mw": 0}),
        C_("packed1-mw", "lin", lens(511, 512, 513, 1024, 1025)),
        C_("packed2-mw", "lin", lens(1023, 1024, 1025, 2048, 2049), {"fwd_quads": 2, "pxmw": 0}),
        C_("px0", "lin", lens(511, 512, 513, 1023, 1024), {"mf": 0}),
        C_("px1", "lin", lens(511, 512, 513, 1023, 1024), {"mf": 1}),
        C_("px2", "lin", lens(511, 512, 513, 1023, 1024), {"mf": 2}),
        C_("px3", "lin", lens(511, 512, 513, 1023, 1024), {"band": 0}),
        C_("band", "lin", lens(511, 512, 513, 1023, 1024)),
        C_("px0-relative", "lin", lens(511, 512, 513, 1023, 1024), {"relative": 1}),
        C_("pxmw", "lin", lens(1023, 1024, 1025, 2048, 2049), {"pxmw": 1}),
        C_("pxmw-relative", "lin", lens(1023, 1024, 1025, 2048, 2049), {"relative": 1}),
    ]
    # --- the second workgroup group of the multi-wave kernels: strips = limit, limit + 1, and two even groups
    for name, tune, strip, limit, sizes in (
            ("packed1-mw", {}, 512, 16, (16, 17, 20)), ("pxmw", {"pxmw": 1}, 1024, 16, (16, 17, 20)),
            ("fwd2-u32-mw", {"planes": 32, "fwd_quads": 2}, 512, 16, (16, 17, 20)),
            ("fwd4-u32-mw", {"planes": 32, "fwd_quads": 4}, 1024, 10, (10, 11, 14))):
        for s in sizes:
            top = (s - 1) * strip + 1 if s == limit + 1 else s * strip       # L + 1: limit + 1 strips by one column
            out.append(C_("%s-%dstrips" % (name, s), "lin", (0, 1, 100, 63, top - 1001, top - 1), tune,
                          planes=(top,) if "planes" in tune else ()))
    # --- the u32 `wide` rule by pitch, no quads override: 8 192 columns run <2,u32,MW> (16 waves), 8 193 run <4,u32,MW> (9)
    out.append(C_("u32-wide-8192", "lin", (0, 1, 100, 63, 8191), u32))
    out.append(C_("u32-wide-8193", "lin", (0, 1, 100, 63, 8191, 8192), u32))
    # --- the multi-wave hand-over graph through every multi-wave kernel, and through the strip loops that read the same edges
    for name, tune, full in (("packed1-mw", {}, False), ("packed2-mw", {"fwd_quads": 2, "pxmw": 0}, False), ("pxmw", {"pxmw": 1}, False),
                             ("pxmw-relative", {"relative": 1}, False), ("fwd2-u32-mw", {"planes": 32, "fwd_quads": 2}, False),
                             ("fwd4-u32-mw", {"planes": 32, "fwd_quads": 4}, False), ("packed2-strips", {"mw": 0}, False),
                             ("fwd2-u16-strips", {}, True), ("fwd4-u32-strips", {"planes": 32, "mw": 0}, False)):
        out.append(C_("handover-" + name, "mw", None, tune, full, planes=("far",) if (full or "planes" in tune) else ()))
    # --- the traceback matrix: every storage format x lanes per walk x speculation depth
    fmts = (("fmt0", {"px": 0}, False), ("fmt1", {"mf": 0}, False), ("fmt2", {"mf": 1}, False), ("fmt3", {"mf": 2}, False),
            ("fmt4", {"band": 0}, False), ("relative", {"relative": 1}, False))
    for fname, tune, full in fmts:
        for lanes in (64, 32, 16, 8):
            for depth in (1, None, 64):
                t = dict(tune, tb_group=lanes)
                if depth:
                    t["tb_depth"] = depth
                out.append(C_("tb-%s-%dlanes-depth%s" % (fname, lanes, depth or "default"), "tb", None, t, full))
    for fname, tune, full in (("u16full", {}, True), ("u32full", {"planes": 32}, False)):
        for depth in (1, None, 64):
            out.append(C_("tb-%s-depth%s" % (fname, depth or "default"), "tb", None, dict(tune, **({"tb_depth": depth} if depth else {})), full))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _lengths(case):
    return tuple(len(q) for q in _queries(case.kind, case.lengths))


def _predict(case):
    return predict(_graph(case.kind), _lengths(case), case.costs, tune=dict(case.tune), full_planes=case.full)


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_selection_rule_restated():
    """`predict` on shapes worked out by hand from plan_dense_run / plan_dense_chunk (poasta_amd/csrc/poa_dense_plan.cpp)."""
    g = _graph("lin")
    assert min_path_nodes(g) == 180
    assert [pitch_of(L) for L in (0, 62, 63, 64, 511, 512, 1023, 1024)] == [64, 64, 64, 128, 512, 576, 1024, 1088]
    assert [mw_waves(s) for s in (1, 3, 16, 17, 20, 32, 33)] == [1, 3, 16, 9, 10, 16, 11]
    # ub = 6 + 2 * 511 + 6 + 2 * 180 = 1394: u16, compact, one column group: the packed kernel, 64 lanes per walk at depth 32
    p = predict(g, [0, 511], COSTS)
    assert launch_of(p) == dict(kernel="packed", quads=1, fuse=False, mw=False, waves=4, code_fmt=0, tb_lanes=64, tb_depth=32, queries=2)
    assert p["layout"] == {"u16", "compact"} and not p["band"]
    # one more column: pitch 576, pairs across quads; ub <= 4094: flags ride in M, derived gaps, banded (e > 0, pitch > 512)
    p = predict(g, [0, 512], COSTS)
    assert (p["kernel"], p["quads"], p["code_fmt"], p["band"], p["layout"]) == ("band", 2, 4, True, {"u16", "compact", "derived_gaps"})
    assert predict(g, [512], COSTS, tune={"band": 0})["kernel"] == "px" and predict(g, [512], (4, 6, 0))["kernel"] == "px"
    assert [predict(g, [512], COSTS, tune={"mf": m})["code_fmt"] for m in (0, 1, 2, 3)] == [1, 2, 3, 4]
    # ub = 12 + 30 * (1000 + 180) = 35412 > 16382: no flags beside the score
    assert predict(g, [1000], (4, 6, 30))["code_fmt"] == 1 and predict(g, [1000], (4, 6, 30), tune={"mf": 3})["code_fmt"] == 1
    # ub = 12 + 8 * 1180 = 9452: two flags at most
    assert predict(g, [1000], (4, 6, 8), tune={"mf": 2})["code_fmt"] == 2 and predict(g, [1000], (4, 6, 8))["code_fmt"] == 4
    # past one strip: multi-wave; 3 strips of 512 for a small chunk, the 1024-column kernel once count * 2 strips reach 1024
    p = predict(g, [1024], COSTS)
    assert (p["kernel"], p["quads"], p["mw"], p["waves"], p["code_fmt"]) == ("packed", 1, True, 3, 0)
    assert predict(g, [1024], COSTS, n_chunk_queries=511)["kernel"] == "packed"
    p = predict(g, [1024], COSTS, n_chunk_queries=512)
    assert (p["kernel"], p["quads"], p["mw"], p["waves"], p["code_fmt"]) == ("pxmw", 2, True, 2, 1)
    p = predict(g, [1024], COSTS, n_chunk_queries=4096, tune={"pxmw": 0})
    assert (p["kernel"], p["quads"], p["waves"]) == ("packed", 2, 2)
    assert predict(g, [1024], COSTS, n_chunk_queries=4095, tune={"pxmw": 0})["quads"] == 1
    # overrides the launcher overrides: px = 0 and mw = 0 under the relative encoding, fuse_tb under px
    p = predict(g, [600], COSTS, tune={"relative": 1, "px": 0})
    assert (p["kernel"], p["code_fmt"], p["layout"]) == ("px", 1, {"u16", "compact", "relative"})
    assert predict(g, [1500], COSTS, tune={"relative": 1, "mw": 0})["kernel"] == "pxmw"
    p = predict(g, [600], COSTS, tune={"fuse_tb": 1})
    assert (p["kernel"], p["quads"], p["fuse"], p["tb_lanes"], p["tb_depth"]) == ("packed", 2, True, 0, 12)
    p = predict(g, [600], COSTS, tune={"fuse_tb": 1, "relative": 1})
    assert (p["kernel"], p["fuse"], p["tb_lanes"]) == ("px", False, 64)
    # the relative encoding by the rule: ub = 12 + 255 * (100 + 180) = 71 412 > 65534, 2 * (6 + 255 * 100) = 51 012 fits
    p = predict(g, [100], (4, 6, 255))
    assert p["layout"] == {"u16", "compact", "relative"} and p["kernel"] == "px"
    assert predict(g, [100], (4, 6, 255), tune={"relative": 0})["cells"] == "u32"
    # u32: 256 columns per group; multi-wave past 1024; wide = 14 * g4 < 10 * g2 or count * s4 >= 8192
    assert [predict(g, [L], COSTS, tune={"planes": 32})["quads"] for L in (255, 256, 511, 512, 1023)] == [1, 2, 2, 4, 4]
    p = predict(g, [8191], COSTS, tune={"planes": 32})
    assert (p["kernel"], p["quads"], p["mw"], p["waves"]) == ("forward", 2, True, 16)
    p = predict(g, [8192], COSTS, tune={"planes": 32})          # s2 = 17: two groups of 512-column strips, one of 1024-column ones
    assert (p["quads"], p["waves"]) == (4, 9)
    p = predict(g, [10240], COSTS, tune={"planes": 32})         # s4 = 11, g4 = 2; s2 = 21, g2 = 2: 28 < 20 fails
    assert (p["quads"], p["waves"]) == (2, 11)
    assert predict(g, [10240], COSTS, tune={"planes": 32, "fwd_quads": 4})["waves"] == 6
    assert predict(g, [1024], COSTS, n_chunk_queries=4096, tune={"planes": 32})["quads"] == 4
    assert predict(g, [1024], COSTS, n_chunk_queries=4095, tune={"planes": 32})["quads"] == 2
    # reads of 33 kbp at e = 2: 2 * (6 + 2 * 33000) > 65534 and ub > 65534: u32 by the rule
    assert predict(g, [33000], COSTS)["cells"] == "u32"
    # traceback lanes by the chunk's count, depth to match; full planes: 64 lanes at depth 12
    assert [(predict(g, [40], COSTS, n_chunk_queries=n)["tb_lanes"], predict(g, [40], COSTS, n_chunk_queries=n)["tb_depth"])
            for n in (6144, 6145, 12288, 12289)] == [(64, 32), (32, 32), (32, 32), (16, 16)]
    p = predict(g, [40], COSTS, tune={"tb_group": 16, "planes": 32})
    assert (p["tb_lanes"], p["tb_depth"]) == (64, 12)
    p = predict(g, [40], COSTS, tune={"tb_group": 8, "tb_depth": 64})
    assert (p["tb_lanes"], p["tb_depth"]) == (8, 64)
    assert predict(g, [40], COSTS, tune={"tb_group": 16})["tb_depth"] == 16
    # the bound is the batch's, the pitch the chunk's
    p = predict(g, [300], (4, 6, 30), max_len=3000)             # ub = 12 + 30 * 3180 > 65534 and no relative encoding either
    assert (p["cells"], p["quads"]) == ("u32", 2)


def test_case_table_reaches_every_launch_site():
    """Every launch site the issue lists, every (storage format, lanes per walk) pair the launcher can produce, the three depths,
    and for every forward site the column edges of its own width; names are unique and every batch carries the short queries."""
    assert len(BY_NAME) == len(CASES)
    sites, tb_sites, tb_pairs, depths, edge = {}, set(), set(), {}, {}
    for c in CASES:
        p = _predict(c)
        L = _lengths(c)
        assert {0, 1, 100} <= set(L), c.name
        if c.kind == "lin":
            assert 63 in L, c.name
        sites.setdefault(site_of(p), []).append(c.name)
        if tb_site_of(p):
            tb_sites.add(tb_site_of(p))
            tb_pairs.add((tb_format_of(p), p["tb_lanes"]))
            depths.setdefault((tb_format_of(p), p["tb_lanes"]), set()).add(p["tb_depth"])
        family = site_of(p).replace(",fuse", "").replace("true,false", "false,false")      # a fused variant shares its family's edges
        edge.setdefault(family, (p["strip"], set()))[1].update(x + 1 for x in L)
        assert edge[family][0] == p["strip"]
        for want in c.planes:
            assert "compact" not in p["layout"], c.name        # planes are fetched from full planes only
            assert want == "far" or want - 1 in L, (c.name, want)
    assert REQUIRED_SITES <= set(sites), sorted(REQUIRED_SITES - set(sites))
    assert REQUIRED_TB_SITES <= tb_sites, sorted(REQUIRED_TB_SITES - tb_sites)
    assert REQUIRED_TB <= tb_pairs, sorted(map(str, REQUIRED_TB - tb_pairs))
    for pair in REQUIRED_TB:
        default = 12 if str(pair[0]).endswith("full") else (16 if pair[1] == 16 else 32)
        assert {1, default, 64} <= depths[pair], (pair, depths[pair])
    for family, (Wd, cols) in edge.items():
        one_strip = family.startswith("px<") or family == "band"
        assert {63, 64, 65, Wd - 1, Wd} <= cols, (family, Wd)
        if not one_strip:
            assert {Wd + 1, 2 * Wd, 2 * Wd + 1} <= cols, (family, Wd, sorted(cols))
    # full planes, cell for cell: the u16 and u32 strip loops, both u32 multi-wave kernels, at 2, 3 and more strips
    for name, site, strips in (("fwd2-u16-strips", "LAUNCH_FWD(2,u16)", 4), ("fwd4-u32-strips", "LAUNCH_FWD(4,u32)", 4),
                               ("fwd2-u32-mw", "forward<2,u32,MW>", 3), ("fwd4-u32-mw", "forward<4,u32,MW>", 3)):
        p = _predict(BY_NAME[name])
        assert site_of(p) == site and p["strips"] == strips and BY_NAME[name].planes
        assert {(w + p["strip"] - 1) // p["strip"] for w in BY_NAME[name].planes} >= {2, 3}, name
    # the second group of every multi-wave kernel: limit, limit + 1, two even groups
    for name, site, want in (("packed1-mw", "packed<1,false,true>", {16: 16, 17: 9, 20: 10}), ("pxmw", "pxmw", {16: 16, 17: 9, 20: 10}),
                             ("fwd2-u32-mw", "forward<2,u32,MW>", {16: 16, 17: 9, 20: 10}),
                             ("fwd4-u32-mw", "forward<4,u32,MW>", {10: 10, 11: 6, 14: 7})):
        for strips, waves in want.items():
            p = _predict(BY_NAME["%s-%dstrips" % (name, strips)])
            assert (site_of(p), p["strips"], p["waves"]) == (site, strips, waves), (name, strips, p)
    assert (site_of(_predict(BY_NAME["u32-wide-8192"])), site_of(_predict(BY_NAME["u32-wide-8193"]))) == ("forward<2,u32,MW>", "forward<4,u32,MW>")
    assert not BY_NAME["u32-wide-8192"].tune[1:] and not BY_NAME["u32-wide-8193"].tune[1:]       # planes = 32 and nothing else
    # the hand-over graph runs through all six multi-wave launches and the three strip loops
    hand = {site_of(_predict(c)) for c in CASES if c.kind == "mw"}
    assert hand == {"packed<1,false,true>", "packed<2,false,true>", "pxmw", "pxmw,relative", "forward<2,u32,MW>", "forward<4,u32,MW>",
                    "packed<2,false,false>", "LAUNCH_FWD(2,u16)", "LAUNCH_FWD(4,u32)"}, hand
    # the fused walk above one strip is followed by the separate launch
    for name in ("fwd2-u16-fuse-strips", "fwd4-u32-fuse-strips", "packed2-fuse-strips"):
        p = _predict(BY_NAME[name])
        assert p["fuse"] and p["tb_lanes"] == 64, name


# ---- CPU: the C++ rule (poasta_amd/csrc/poa_dense_plan.cpp) against `predict` ------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poasta_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "dense_plan_host", "dense_plan_host.cpp")
KERNEL_ID = {"forward": 1, "packed": 2, "px": 3, "pxmw": 4, "band": 5}                # POA_KERNEL_*
LAYOUT_BIT = {"u16": 1, "compact": 2, "relative": 4, "derived_gaps": 8}               # POA_LAYOUT_*


@pytest.fixture(scope="module")
def plan_host():
    """tests/dense_plan_host and the product's poa_dense_plan.cpp as a shared library, built with g++"""
    out = os.path.join(ROOT, "tests", "dense_plan_host", "libdense_plan_host.so")
    deps = [HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp"), os.path.join(CSRC, "poa_dense_plan.hpp"), os.path.join(ROOT, "include", "poasta_amd.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp")])
    X = C.CDLL(out)
    X.dense_plan_host.argtypes = [C.c_uint32] * 3 + [C.c_uint64] * 2 + [C.c_uint32] * 3 + [C.c_void_p] + [C.c_uint32] * 2 + [C.c_void_p]
    X.dense_plan_host.restype = None
    return X


def _tune_words(tune):
    """poa_config_t.tune of make_config's keyword overrides: 0 not set, else value + 1"""
    t = (C.c_uint32 * 32)()
    for k, v in dict(tune).items():
        t[TUNE_KEYS.index(k.upper())] = v + 1
    return t


def _words_of(pred):
    """a prediction as dense_plan_host writes it: the eight launch words, the layout bits, the banded pair"""
    return (KERNEL_ID[pred["kernel"]], pred["quads"], int(pred["fuse"]) | int(pred["mw"]) << 1, pred["waves"], pred["code_fmt"], pred["tb_lanes"],
            pred["tb_depth"], pred["queries"], sum(LAYOUT_BIT[k] for k in pred["layout"]), int(pred["band"]))


def _cxx_words(X, costs, max_len, mpn, count, max_pitch, tune_words, full_planes, plan16_same=False):
    out = (C.c_uint32 * 11)()
    X.dense_plan_host(costs[0], costs[1], costs[2], max_len, mpn, 0, int(full_planes), int(plan16_same), tune_words, count, max_pitch, out)
    return tuple(out)


def _assert_cxx_equals_predict(X, g, lengths, costs, n_chunk_queries=None, tune=None, max_len=None, full_planes=False, mpn=None):
    """-> the prediction, after the C++ rule gave the same record, layout, band and chunk plan for the same chunk"""
    pred = _predict_itself(g, lengths, costs, n_chunk_queries, tune, max_len, full_planes, mpn)
    mpn = min_path_nodes(g) if mpn is None else mpn
    args = (costs, max(lengths) if max_len is None else max_len, mpn, pred["queries"], max(pitch_of(L) for L in lengths), _tune_words(tune or {}), full_planes)
    got = _cxx_words(X, *args)
    assert got[:10] == _words_of(pred), (lengths, costs, n_chunk_queries, tune, max_len, full_planes, got, _words_of(pred))
    assert launch_of(pred) == dict(zip(LAUNCH_KEYS, (LAUNCH_KERNELS[got[0]], got[1], bool(got[2] & 1), bool(got[2] & 2)) + got[3:8]))
    # the chunk plan of the run: 2-byte elements (compact: 2, full planes: 1) unless the batch fits one chunk anyway
    assert got[10] == ((2 if "compact" in pred["layout"] else 1) if pred["cells"] == "u16" else 0)
    assert _cxx_words(X, *args, plan16_same=True)[:10] == got[:10] and _cxx_words(X, *args, plan16_same=True)[10] == 0
    return pred


def test_cxx_rule_equals_predict_on_cases_and_restated_shapes(plan_host, monkeypatch):
    """plan_dense_run / plan_dense_chunk give launch_of(predict), predict's layout and band for every entry of CASES, and for
    every shape of test_selection_rule_restated: that test runs once more with each predict() it makes held against the C++ rule"""
    for c in CASES:
        _assert_cxx_equals_predict(plan_host, _graph(c.kind), _lengths(c), c.costs, tune=dict(c.tune), full_planes=c.full)
    seen = []

    def both(*args, **kwargs):
        seen.append(_assert_cxx_equals_predict(plan_host, *args, **kwargs))
        return seen[-1]

    monkeypatch.setitem(globals(), "predict", both)
    try:
        test_selection_rule_restated()
    finally:
        monkeypatch.undo()
    assert len(seen) >= 47 and predict is _predict_itself       # (the 47 predictions that test made when this one was written)


GRID_COSTS = ((6, 2), (6, 0), (0, 1), (6, 8), (6, 30), (6, 255))                     # (open, extend)
GRID_MPN = (0, 1, 180, 5000)
GRID_MAX_LEN = (None, 3000, 33000)                                                  # None: the chunk's own
GRID_COLS = (1, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 8192, 8193, 10241)      # L + 1
# The count axis of (1, 511, 512, 1023, 1024, 4095, 4096, 6144, 6145, 12288, 12289) took 40 s here, so it is halved: the last count
# below each threshold (count * strips >= 1024 and >= 8192 at one and two strips, 6 144 and 12 288 walks) and, with the next
# value, one above it; the counts right at the thresholds are among the shapes of test_selection_rule_restated.
GRID_COUNT = (511, 1023, 4095, 6144, 12288, 12289)
GRID_VALUES = dict(planes=(32,), compact=(0, 1), packed=(0, 1), px=(0, 1), mw=(0, 1), pxmw=(0, 1), band=(0, 1), relative=(0, 1), mf=(0, 1, 2, 3),
                   fwd_quads=(1, 2, 4), fuse_tb=(1,), tb_group=(8, 16, 32, 64, 7), tb_depth=(1, 64, 65), band_delta=(0, 5))


def _grid_tunes():
    """no override, every key of SELECTION_KEYS alone at each value the rule distinguishes, every distinct tune of CASES"""
    assert set(GRID_VALUES) == {k.lower() for k in SELECTION_KEYS}
    tunes = [()] + [((k.lower(), v),) for k in SELECTION_KEYS for v in GRID_VALUES[k.lower()]]
    for c in CASES:
        if c.tune not in tunes:
            tunes.append(c.tune)
    return tunes


def test_cxx_rule_equals_predict_on_the_grid(plan_host):
    """The full product of GRID_* x full planes off / on x _grid_tunes(): the C++ record, layout and band equal predict's.  Only
    the combinations whose batch max_len is below the chunk's own query are left out, and at least 90 % are compared."""
    tunes = [(dict(t), _tune_words(t)) for t in _grid_tunes()]
    total = compared = 0
    for L1 in GRID_COLS:
        L, pitch = L1 - 1, pitch_of(L1 - 1)
        for costs in GRID_COSTS:
            x_costs = (4,) + costs
            for mpn in GRID_MPN:
                for ml in GRID_MAX_LEN:
                    n = len(GRID_COUNT) * 2 * len(tunes)
                    total += n
                    max_len = L if ml is None else ml
                    if max_len < L:
                        continue
                    compared += n
                    for count in GRID_COUNT:
                        for full in (False, True):
                            for tune, words in tunes:
                                want = _words_of(predict(None, (L,), x_costs, count, tune, max_len, full, mpn))
                                got = _cxx_words(plan_host, x_costs, max_len, mpn, count, pitch, words, full)
                                assert got[:10] == want, (L, costs, mpn, max_len, count, full, tune, got, want)
    assert total == len(GRID_COLS) * len(GRID_COSTS) * len(GRID_MPN) * len(GRID_MAX_LEN) * len(GRID_COUNT) * 2 * len(tunes)
    assert compared >= 0.9 * total, (compared, total)


def test_dense_plan_host_under_sanitizers(tmp_path):
    """tests/dense_plan_host as a program of its own, address and undefined-behaviour sanitizers on, on the CPU: every record of
    its grid names a kernel, column groups the cell type has, 1 to 16 waves that cover the widest row, and lanes the traceback has."""
    exe = os.path.join(str(tmp_path), "dense_plan_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           HOST_SRC, os.path.join(CSRC, "poa_dense_plan.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"dense_plan_host ok" in r.stdout


def test_handover_graph_has_the_edges_it_exists_for(oracle):
    """Edges of exactly 32 and 33 rows and far ones on a Hamiltonian chain longer than ring + look-back; every marked query's
    optimal alignment (the oracle's) steps from the edge's source straight to its target, whose cell lies in the column meant."""
    from poasta_amd import aligner
    g, _, ids = _mw_graph()
    rows = aligner.DeviceGraph(g).node_rows().astype(np.int64)
    assert g.n >= MW_RING + ROW_NEAR + 2
    assert np.array_equal(rows[np.array(ids)], np.arange(1, MWG_N + 1))      # a Hamiltonian chain: row distance == node distance
    dist = {}
    for v in range(g.n):
        for p in g.predecessors(v).tolist():
            dist.setdefault(int(rows[v] - rows[p]), []).append(int(rows[v]))
    assert len(dist[ROW_NEAR]) >= len(MWG_SKIP_A) and len(dist[ROW_NEAR + 1]) >= len(MWG_SKIP_A)
    assert any(d >= 300 for d in dist) and 690 in dist
    assert len(dist[2]) >= 4                                                 # two-predecessor rows directly behind the targets
    qs, marks = _mw_queries()
    assert 1100 <= max(len(q) for q in qs) <= 2200 and sum(1100 <= len(q) for q in qs) >= 14
    cols = sorted({t[1] + 1 for _, _, t in marks})                           # column of the target's cell
    assert cols == [12, 511, 512, 513, 1023, 1024, 1025]
    for i, (sn, sq), (tn, tq) in marks:
        assert tq == sq + 1 and rows[tn] - rows[sn] >= ROW_NEAR and qs[i][sq] == g.symbol[sn] and qs[i][tq] == g.symbol[tn]
    both = {(int(rows[tn] - rows[sn]), tq + 1) for _, (sn, _), (tn, tq) in marks}
    assert {(d, c) for d in (32, 33) for c in MWG_SKIP_COLS} <= both
    _, D = _oracle(oracle, "mw", None, COSTS)
    for i, src, tgt in marks:
        al = oracle.batch_alignment(D, i)
        assert src in al and tgt in al and al.index(tgt) == al.index(src) + 1, (i, src, tgt)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _oracle(oracle, kind, lengths, costs):
    """(OracleGraph, dense_batch of the query set), computed once per (graph, queries, costs) and shared"""
    key = (kind, lengths, costs)
    if key not in _oracle_cache:
        og = oracle.OracleGraph.from_csr(_graph(kind).as_dict())
        qseq, qoff = pack_queries(_queries(kind, lengths))
        _oracle_cache[key] = (og, og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=8))
    return _oracle_cache[key]


def _assert_equals_oracle(res, D, n, tag):
    """score, flags and every (rpos, qpos) of the first n queries of D, bit for bit"""
    assert np.array_equal(res.score, D["score"][:n]), (tag, "score", np.flatnonzero(res.score != D["score"][:n])[:8].tolist())
    assert np.array_equal(res.flags, D["flags"][:n]), (tag, "flags", np.flatnonzero(res.flags != D["flags"][:n])[:8].tolist())
    npairs = D["n_pairs"][:n].astype(np.int64)
    got_n = np.diff(res.pair_off.astype(np.int64))
    assert np.array_equal(got_n, npairs), (tag, "n_pairs", np.flatnonzero(got_n != npairs)[:8].tolist())
    start = np.cumsum(npairs) - npairs
    idx = np.repeat(D["pair_off"][:n].astype(np.int64) - start, npairs) + np.arange(int(npairs.sum()))
    want, got = D["pairs"][idx], res.pairs[:int(npairs.sum())]
    if not np.array_equal(got, want):
        k = int(np.flatnonzero((got != want).any(axis=1))[0])
        i = int(np.searchsorted(start, k, side="right")) - 1
        pytest.fail("%s: alignment of query %d differs at pair %d: got %s, want %s" % (tag, i, k - int(start[i]), got[k].tolist(), want[k].tolist()))


def _run(engine, g, qs, costs, tune, full=False, workspace_bytes=0):
    qseq, qoff = pack_queries(qs)
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=workspace_bytes)
    rb.run(engine.GapAffine(costs[0], costs[2], costs[1]), None, engine.make_config(full_planes=full, **tune))
    return rb, rb.fetch()


def _assert_planes(rb, engine, oracle, og, g, q, i, costs, pred, tag):
    """every M / I / D cell of query i against the oracle's planes, rows mapped through node_rows on both sides"""
    rows, orank = rb.dg.node_rows(), og.export_csr()["rank"]
    od = og.dense_align(q, oracle.Costs(*costs), planes=True)
    got3 = rb.planes(i)
    for name, gp, op in zip("MID", got3, (od["M"], od["I"], od["D"])):
        want = op[orank]
        if pred["cells"] == "u16":
            finite = want[want != INF]
            assert finite.size == 0 or int(finite.max()) <= 65534, (tag, name)      # from the oracle alone: u16 holds every finite cell
        got = gp[rows]
        if not np.array_equal(got, want):
            v, c = (int(t) for t in np.argwhere(got != want)[0])
            pytest.fail("%s plane %s of query %d (%d columns): first difference at row %d (node %d) column %d, strip %d of %d columns: got %d, "
                        "want %d; %d cells differ" % (tag, name, i, len(q) + 1, int(rows[v]), v, c, c // pred["strip"], pred["strip"],
                                                      int(got[v, c]), int(want[v, c]), int((got != want).sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gpu_dense_launch(engine, oracle, case):
    g, qs = _graph(case.kind), _queries(case.kind, case.lengths)
    L = _lengths(case)
    pred = _predict(case)
    rb, res = _run(engine, g, qs, case.costs, dict(case.tune), case.full)
    try:
        launches, layout, band = rb.launches(), rb.layout(), rb.band_info()
        print(case.name, site_of(pred), tb_site_of(pred), launches)
        checked = not _ambient()
        if checked:
            assert launches == [launch_of(pred)], (launches, launch_of(pred))
            assert layout == pred["layout"], (layout, pred["layout"])
            assert band["used"] == pred["band"] and (not band["used"] or band["banded"] + band["fell_back"] == len(qs)), band
        og, D = _oracle(oracle, case.kind, case.lengths, case.costs)
        _assert_equals_oracle(res, D, len(qs), case.name)
        if case.kind == "mw":
            for i, src, tgt in _mw_queries()[1]:
                al = res.raw_alignment(i)
                assert src in al and tgt in al and al.index(tgt) == al.index(src) + 1, (case.name, i, src, tgt)
        if "compact" not in layout and (checked or layout == pred["layout"]):
            for want in case.planes:
                i = max(range(len(L)), key=lambda k: L[k]) if want == "far" else L.index(want - 1)
                if want == "far":                    # the far edge's query and the longest one
                    _assert_planes(rb, engine, oracle, og, g, qs[_mw_queries()[1][-3][0]], _mw_queries()[1][-3][0], case.costs, pred, case.name)
                _assert_planes(rb, engine, oracle, og, g, qs[i], i, case.costs, pred, case.name)
    finally:
        rb.close()


def _short_reads(kind, n, length, seed=21):
    poa = _poa(kind)
    return poa.queries(n, length=length, seed=seed)


@pytest.mark.gpu
def test_gpu_default_traceback_lanes_both_sides(engine, oracle):
    """6 144 / 6 145 and 12 288 / 12 289 reads of 40 bases on a 32-row graph, no override: 64, 32, 32 and 16 lanes per walk
    (packed<1>, code_fmt 0); the shorter batches are prefixes of the longest, so the shared queries must come out identical, and
    every one equals the oracle."""
    g = _graph("tiny")
    qs = [np.zeros(0, np.uint8)] + _short_reads("tiny", 12288, 40)
    for k in range(1, 12289, 97):
        qs[k] = qs[k][:int(k % 41)]            # lengths 0 .. 40 among them
    qseq, qoff = pack_queries(qs)
    D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*COSTS), threads=8)
    for n, lanes, depth in ((6144, 64, 32), (6145, 32, 32), (12288, 32, 32), (12289, 16, 16)):
        pred = predict(g, [len(q) for q in qs[:n]], COSTS)
        assert (site_of(pred), pred["tb_lanes"], pred["tb_depth"], pred["code_fmt"]) == ("packed<1,false,false>", lanes, depth, 0)
        rb, res = _run(engine, g, qs[:n], COSTS, {})
        try:
            print(n, rb.launches())
            if not _ambient():
                assert rb.launches() == [launch_of(pred)], (n, rb.launches())
            _assert_equals_oracle(res, D, n, "%d reads" % n)
        finally:
            rb.close()


@pytest.mark.gpu
def test_gpu_default_pxmw_rule_both_sides(engine, oracle):
    """511 and 512 queries of two 1024-column strips on a 62-row graph, no override: count * strips = 1 022 runs packed<1,MW>,
    1 024 runs pxmw; the first 511 queries are shared and every result equals the oracle."""
    g = _graph("small")
    qs = _short_reads("small", 512, 1030)
    qs[0], qs[1], qs[2] = qs[0][:0], qs[1][:1], qs[2][:100]
    qseq, qoff = pack_queries(qs)
    D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*COSTS), threads=8)
    for n, site in ((511, "packed<1,false,true>"), (512, "pxmw")):
        pred = predict(g, [len(q) for q in qs[:n]], COSTS)
        assert site_of(pred) == site
        rb, res = _run(engine, g, qs[:n], COSTS, {})
        try:
            print(n, rb.launches())
            if not _ambient():
                assert rb.launches() == [launch_of(pred)], (n, rb.launches())
            _assert_equals_oracle(res, D, n, "%d queries" % n)
        finally:
            rb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["packed-quads", "u32-wide"])
def test_gpu_default_8192_rules_both_sides(engine, oracle, rule):
    """4 095 and 4 096 queries of two 1024-column strips on a 7-row graph, no quads override: count * strips = 8 190 keeps the
    512-column strips (packed<1,MW> with pxmw refused; <2,u32,MW>), 8 192 takes the 1024-column ones (packed<2,MW>; <4,u32,MW>).
    The first 4 095 queries are shared and every result equals the oracle."""
    g = _graph("seven")
    assert g.n == 7
    qs = _short_reads("seven", 4096, 1030)
    qs[0], qs[1], qs[2] = qs[0][:0], qs[1][:1], qs[2][:100]
    tune, sites = {"packed-quads": ({"pxmw": 0}, ("packed<1,false,true>", "packed<2,false,true>")),
                   "u32-wide": ({"planes": 32}, ("forward<2,u32,MW>", "forward<4,u32,MW>"))}[rule]
    key = ("seven-8192", COSTS)
    if key not in _oracle_cache:
        qseq, qoff = pack_queries(qs)
        _oracle_cache[key] = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*COSTS), threads=8)
    D = _oracle_cache[key]
    for n, site, waves in ((4095, sites[0], 3), (4096, sites[1], 2)):
        pred = predict(g, [len(q) for q in qs[:n]], COSTS, tune=tune)
        assert (site_of(pred), pred["waves"]) == (site, waves)
        rb, res = _run(engine, g, qs[:n], COSTS, tune)
        try:
            print(rule, n, rb.launches())
            if not _ambient():
                assert rb.launches() == [launch_of(pred)], (n, rb.launches())
            _assert_equals_oracle(res, D, n, "%s, %d queries" % (rule, n))
        finally:
            rb.close()


def _mixed_batch():
    """64 reads of 300 bases, 24 of 800, 12 of 1 500, shortest first (and the three short queries in front)"""
    poa = _poa("lin")
    qs = [np.zeros(0, np.uint8), poa.queries(1, length=1, first=900)[0], poa.queries(1, length=100, first=901)[0]]
    for n, length, first in ((64, 300, 1000), (24, 800, 2000), (12, 1500, 3000)):
        qs += poa.queries(n, length=length, first=first)
    return qs


@pytest.mark.gpu
@pytest.mark.parametrize("relative", [False, True], ids=["absolute", "relative"])
def test_gpu_mixed_chunks(engine, oracle, relative):
    """A workspace cap that cuts a length-sorted batch into chunks that pick different kernels in one run: the first chunk (300-base
    reads only) runs packed<1>, the chunk with the first 800-base read a one-strip kernel (banded / px), the last chunk (1 500-base
    reads, first_query > 0) a multi-wave kernel.  launches() per chunk equals `predict` for that chunk's queries; the results equal
    the uncapped run's and the oracle's.  relative: the same under the relative encoding (px<0> and pxmw)."""
    g, qs = _graph("lin"), _mixed_batch()
    L = [len(q) for q in qs]
    tune = {"relative": 1} if relative else {}
    # a compact query holds between 2.5 and 4.5 bytes per row and pitch column: a cap of 12 000 columns at 3.5 bytes holds fewer
    # columns than the 300-base reads have together (20 480) and than the 800-base reads have (19 968), more than any one query
    ws = int(g.n * 3.5 * 12000)
    rb, res = _run(engine, g, qs, COSTS, tune, workspace_bytes=ws)
    try:
        launches = rb.launches()
        print(launches)
        assert res.stats["n_chunks"] == len(launches) >= 3
        counts = [l["queries"] for l in launches]
        assert sum(counts) == len(qs)
        if not _ambient():
            first, kinds = 0, []
            for l in launches:
                pred = predict(g, L[first:first + l["queries"]], COSTS, tune=tune, max_len=max(L))
                assert l == launch_of(pred), (first, l, launch_of(pred))
                kinds.append(site_of(pred))
                first += l["queries"]
            if relative:
                assert kinds[0] == "px<0>,relative" and kinds[-1] == "pxmw,relative", kinds
            else:
                assert kinds[0] == "packed<1,false,false>" and "band" in kinds and kinds[-1] == "packed<1,false,true>", kinds
            assert rb.layout() >= ({"u16", "compact", "relative"} if relative else {"u16", "compact"})
        qseq, qoff = pack_queries(qs)
        D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*COSTS), threads=8)
        _assert_equals_oracle(res, D, len(qs), "capped")
    finally:
        rb.close()
    rb2, whole = _run(engine, g, qs, COSTS, tune)
    try:
        assert len(rb2.launches()) == 1
        assert (np.array_equal(whole.score, res.score) and np.array_equal(whole.flags, res.flags) and np.array_equal(whole.pair_off, res.pair_off)
                and np.array_equal(whole.pairs, res.pairs))
    finally:
        rb2.close()


@pytest.mark.gpu
def test_gpu_launch_record_errors(engine):
    """poa_batch_last_launch: POA_ERR_INVALID_ARG before a run and for a chunk past the last, POA_ERR_UNSUPPORTED after a two-piece
    run and after a run in another mode."""
    import ctypes as C
    lib = engine._lib.lib()
    g, qs = _graph("small"), _short_reads("small", 4, 50)
    qseq, qoff = pack_queries(qs)
    rb = engine.ResidentBatch(g, qseq, qoff)
    out = (C.c_uint32 * 8)()
    try:
        assert lib.poa_batch_last_launch(rb.handle, 0, out) == -1
        rb.run(engine.GapAffine(4, 2, 6))
        assert lib.poa_batch_last_launch(rb.handle, 0, out) == 0 and out[7] == 4
        assert lib.poa_batch_last_launch(rb.handle, 1, out) == -1 and lib.poa_batch_last_launch(rb.handle, 0, None) == -1
        assert len(rb.launches()) == 1
        rb.run(engine.GapAffine2Piece(4, 2, 6, 1, 24))
        assert lib.poa_batch_last_launch(rb.handle, 0, out) == -7
        rb.run(engine.GapAffine(4, 2, 6), None, engine.make_config("exact"))
        assert lib.poa_batch_last_launch(rb.handle, 0, out) == -7
        rb.run(engine.GapAffine(4, 2, 6))
        assert rb.launches()[0]["kernel"] == "packed"
        rb.fetch()
    finally:
        rb.close()
