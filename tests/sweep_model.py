"""What the one-wavefront-per-query paths launch, restated in plain Python from poasta_amd/csrc/poa_engine.hip (run_sweep, run_ckpt,
run_ckpt2, poa_multi_run, poa_multi_run_2piece, scoreset_run), launch_by_pitch, u16_cells_suffice (poa_dense_plan.cpp) and
scoreset_class (poa_scoreset_plan.hpp).  Used by tests/test_sweep_matrix.py; no engine, no device."""
from collections import namedtuple

U16_BOUND = 65534
STRIP = {("u16", 1): 512, ("u16", 2): 1024, ("u32", 1): 256, ("u32", 2): 512, ("u32", 4): 1024}   # 64 lanes x K x Q columns


def pitch_of(L):
    return (L + 1 + 63) // 64 * 64


def score_bound(o, e, max_len, mpn):
    """open * n_open + extend * n_extend: insert the longest query, delete the shortest start -> end path"""
    return o * ((1 if max_len else 0) + (1 if mpn else 0)) + e * (max_len + mpn)


def reduced(costs2):
    """(m, e1, o1, e2, o2) -> the one-piece costs (m, o, e) the score-only sweeps run a two-piece model under"""
    m, e1, o1, e2, _ = costs2
    return (m, o1 + e1 - e2, e2)


def cells_of(o, e, per_graph, planes32=False):
    """per_graph: [(mpn, longest query)] of the graphs that have queries; u16 only if every graph's own bound allows it"""
    return "u16" if (not planes32 and all(score_bound(o, e, ml, mpn) <= U16_BOUND for mpn, ml in per_graph)) else "u32"


def quads_of(cells, max_pitch):
    """launch_by_pitch"""
    if cells == "u16":
        return 1 if max_pitch <= 512 else 2
    return 1 if max_pitch <= 256 else (2 if max_pitch <= 512 else 4)


def scoreset_class(cells, px, pitch):
    """scoreset_class: "PX", or the Q of the general kernel"""
    if cells == "u32":
        return 1 if pitch <= 256 else (2 if pitch <= 512 else 4)
    if pitch <= 512:
        return 1
    if px and pitch <= 1024:
        return "PX"
    return 2


Launch = namedtuple("Launch", "site cells quads px strip lengths")     # lengths: the queries that run under this launch


def _planes32(tune):
    return (tune or {}).get("planes") == 32


def predict_chunk(path, groups, costs, tune=None, wide=False):
    """What one chunk launches.  path: "score" / "score2" (run_sweep), "ckpt" (run_ckpt), "ckpt2" (run_ckpt2), "multi" / "multi2"
    (poa_multi_run / _2piece), "ss" / "ss_cap" / "ss_best" / "ss2" (scoreset_run: the plain, capped, best-of and two-piece plain
    forms).  groups: [(mpn, lengths)] per graph (one entry for the single-graph paths).  costs: (m, o, e), or (m, e1, o1, e2, o2)
    on the two-piece paths; wide: poa_costs2_t.wide_planes.  Returns the list of Launch records, one per kernel launched."""
    tune = dict(tune or {})
    two = path in ("score2", "ckpt2", "multi2", "ss2")
    if two:
        m, e1, o1, e2, o2 = costs
        o, e = reduced(costs)[1:] if path in ("score2", "ss2") else (o1, e1)     # the checkpointed passes: the first piece's costs
    else:
        m, o, e = costs
    groups = [(mpn, tuple(lengths)) for mpn, lengths in groups if len(lengths)]
    # run_ckpt2 never sees the tunables: only wide_planes widens its cells; poa_multi_run_2piece honours both; the sweeps read
    # the tunable alone
    p32 = (_planes32(tune) and path != "ckpt2") or (wide and path in ("ckpt2", "multi2"))
    cells = cells_of(o, e, [(mpn, max(ls)) for mpn, ls in groups], p32)
    lengths = tuple(L for _, ls in groups for L in ls)
    pitches = [pitch_of(L) for L in lengths]
    max_pitch = max(pitches)
    want_px = tune.get("px", 1) != 0
    if path in ("score", "score2"):
        px = cells == "u16" and want_px and 512 < max_pitch <= 1024 and sum(pitches) >= 512 * len(pitches)
        if px:
            return [Launch("poa_sweep_px_kernel", cells, 2, True, 1024, lengths)]
        q = quads_of(cells, max_pitch)
        return [Launch("poa_sweep_kernel<%d,%s>" % (q, cells), cells, q, False, STRIP[cells, q], lengths)]
    if path == "ckpt":
        q = quads_of(cells, max_pitch)
        return [Launch("poa_ckpt<%d,%s>" % (q, cells), cells, q, False, STRIP[cells, q], lengths)]
    if path == "ckpt2":
        q = 2 if cells == "u16" else 4
        return [Launch("poa2_ckpt<%s,%d>" % (cells, q), cells, q, False, 1024, lengths)]
    if path in ("multi", "multi2"):
        q = quads_of(cells, max_pitch)
        name = "poa_ckpt_multi<%d,%s>" % (q, cells) if path == "multi" else "poa2_ckpt_multi<%s,%d>" % (cells, q)
        return [Launch(name, cells, q, False, STRIP[cells, q], lengths)]
    form = {"ss": "scoreset", "ss2": "scoreset", "ss_cap": "scoreset_capped", "ss_best": "scoreset_best"}[path]
    by_class = {}
    for L in lengths:
        by_class.setdefault(scoreset_class(cells, want_px, pitch_of(L)), []).append(L)
    out = []
    for c in ("PX", 1, 2, 4):
        if c in by_class:
            if c == "PX":
                out.append(Launch(form + "<PX>", cells, 2, True, 1024, tuple(by_class[c])))
            else:
                out.append(Launch("%s<%d,%s>" % (form, c, cells), cells, c, False, STRIP[cells, c], tuple(by_class[c])))
    return out


def strips_of(launch):
    """the strip counts of the queries of a launch"""
    return {(pitch_of(L) + launch.strip - 1) // launch.strip for L in launch.lengths}


def sweep_plane_bytes(launches):
    """poa_stats_t.plane_bytes of a score-only run: kept rows x 2 planes x (2048 bytes in the packed kernel's register layout, else
    the pitch in cells).  launches: [(Launch, n_slotted of the graph its queries run on)]"""
    total = 0
    for la, n_slotted in launches:
        elem = 2 if la.cells == "u16" else 4
        total += sum(2 * n_slotted * (2048 if la.px else pitch_of(L) * elem) for L in la.lengths)
    return total


def ckpt_plane_bytes(cells, stored_rows, lengths):
    """... of a checkpointed run: (kept + snapshot rows) x planes kept + rows x window planes, per column of pitch"""
    return stored_rows * sum(pitch_of(L) for L in lengths) * (2 if cells == "u16" else 4)
