"""The exactness proof of the banded one-strip kernel ("Banded one-strip kernel") as a test, on the CPU: the
WINDOWED pass itself (tests/band_model.py: the recurrences with every cell outside its row's window read as INF, the left edge of the
window dropped), under the plans of poasta_amd/csrc/poa_band_plan.cpp, against the oracle's true planes.

  * model check: one window over the whole row, all bases 0  =>  the model IS the oracle, every cell of M, I and D;
  * for every query whose plan has D >= 4, with T = e * (D - 4) (the kernel's certificate):
      (a) model >= true in every cell and state;
      (b) every cell with a finite true value and value + e * de <= T + 2e is exact in M, I and D (claim (2) at D' = D - 2);
      (c) S_w <= T exactly when S* <= T, and then S_w == S*.

The graphs are small and the plans run with small windows and short segments - the same code as for 512 columns and 64 rows.  Fork
graphs (two parallel branches) make the plans move a window to the LEFT; the test counts its own coverage and asserts it."""
import numpy as np

from poasta_amd import workloads as W
from band_model import INF, fork_graph, windowed_planes
from test_band_plan import Plan, harness   # noqa: F401  (the host build of the band plan)

PLANS = [(16, 64), (8, 48)]                              # (seg_rows, window)
COSTS = [(4, 6, 2), (4, 0, 1), (255, 3, 1), (1, 0, 1)]
FORKS = [(40, 25, 25, 40), (30, 20, 35, 30), (50, 18, 18, 20)]
ERR = [(0.0, 0.0, 0.0), (0.02, 0.01, 0.01), (0.06, 0.03, 0.03), (0.15, 0.08, 0.08)]   # (p_sub, p_ins, p_del) of the four reads


def _fork_cases():
    for shape in FORKS:
        for seed in range(6):
            g, walks = fork_graph(*shape, seed=100 * seed + shape[0])
            rng = np.random.default_rng(7000 + seed)
            yield g, [W.mutate(rng, walks[k % 2], *ERR[k]) for k in range(4)]   # alternating branches, rising error rates


def _other_cases():
    lay = W.LayeredPOA(n_layers=40, width=3, indeg=3, seed=5)     # 3 divides neither 16 nor 8: layers straddle segment starts
    yield lay.graph, [lay.queries(1, length=0, seed=6 + k, p_err=p)[0] for k, p in enumerate((0.0, 0.03, 0.12, 0.3))]
    g, (qseq, qoff) = W.scaled_linearish(110, 8, 5, 4, 0, graph_seed=3, p_sub=0.05, p_ins=0.03, p_del=0.03)
    yield g, [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(4)]


def _true_planes(oracle, og, orank, node_of_row, q, costs):
    od = og.dense_align(q, oracle.Costs(*costs), planes=True)
    return [np.ascontiguousarray(od[name][orank])[node_of_row] for name in ("M", "I", "D")]     # by engine row


def test_whole_row_window_is_the_oracle(harness, oracle):
    cells = 0
    cases = list(_fork_cases())[::6] + list(_other_cases())
    for g, qs in cases:
        og = oracle.OracleGraph.from_csr(g.as_dict())
        orank = og.export_csr()["rank"]
        for q in qs[1:3]:
            q = np.ascontiguousarray(q, np.uint8)
            pl = Plan(harness, g, len(q), 16, 64)
            node_of_row = np.argsort(pl.node_row)
            for costs in COSTS:
                true = _true_planes(oracle, og, orank, node_of_row, q, costs)
                model = windowed_planes(g, pl.node_row, q, costs, g.n, len(q) + 1, [0])
                for name, t, m in zip("MID", true, model):
                    assert np.array_equal(t, m), (name, costs, len(q))
                    cells += t.size
    assert cells > 500000


def _check_windowed(harness, oracle, cases, count):
    for g, qs in cases:
        og = oracle.OracleGraph.from_csr(g.as_dict())
        orank = og.export_csr()["rank"]
        for q in qs:
            q = np.ascontiguousarray(q, np.uint8)
            L = len(q)
            for seg_rows, window in PLANS:
                pl = Plan(harness, g, L, seg_rows, window)
                count["plans"] += 1
                count["left_moves"] += int((np.diff(pl.bases) < 0).sum())
                if pl.D < 4:
                    count["no_band"] += 1
                    continue
                node_of_row = np.argsort(pl.node_row)
                end_row = int(pl.node_row[g.end])
                for costs in COSTS:
                    e = costs[2]
                    T = e * (pl.D - 4)
                    true = _true_planes(oracle, og, orank, node_of_row, q, costs)
                    model = windowed_planes(g, pl.node_row, q, costs, seg_rows, window, pl.bases)
                    for name, t, m in zip("MID", true, model):
                        t, m = t.astype(np.int64), m.astype(np.int64)
                        assert (m >= t).all(), ("a", name, costs, L, seg_rows)
                        must = (t != INF) & (t + e * pl.de <= T + 2 * e)
                        assert np.array_equal(m[must], t[must]), ("b", name, costs, L, seg_rows, pl.D)
                        count["exact_cells"] += int(must.sum())
                    s_true, s_w = int(true[0][end_row, L]), int(model[0][end_row, L])
                    assert (s_w <= T) == (s_true <= T), ("c", costs, L, seg_rows, pl.D, s_true, s_w)
                    if s_true <= T:
                        assert s_w == s_true, ("c", costs, L, seg_rows, pl.D)
                    count["certified" if s_true <= T else "uncertified"] += 1


def test_windowed_pass_on_fork_graphs(harness, oracle):
    count = dict.fromkeys(("plans", "left_moves", "no_band", "certified", "uncertified", "exact_cells"), 0)
    _check_windowed(harness, oracle, _fork_cases(), count)
    print(count)
    assert count["left_moves"] >= 1, count
    assert count["certified"] >= 1 and count["uncertified"] >= 1, count
    assert count["exact_cells"] > 100000, count


def test_windowed_pass_on_layered_and_linearish_graphs(harness, oracle):
    count = dict.fromkeys(("plans", "left_moves", "no_band", "certified", "uncertified", "exact_cells"), 0)
    _check_windowed(harness, oracle, _other_cases(), count)
    print(count)
    assert count["certified"] >= 1 and count["exact_cells"] > 10000, count
