"""A numpy model of what poa_forward_band_kernel<false> (poasta_amd/csrc/poa_forward_band.hpp) computes: the recurrences of
oracle/dense.hpp over the engine's rows, with these rules and nothing else:

  * row r owns the columns [b, min(b + window, L + 1)), b = bases[r // seg_rows]; every other cell of the row is INF, for
    every reader (predecessor rows read from memory and rows carried in registers across a window move alike);
  * the diagonal source of column b itself is INF (the dropped left edge: lane 0 of shr_lane);
  * the insertion chain starts at INF at column b;
  * H[start][0] = 0 only when b == 0.

With one window that covers every column and all bases 0 this is the oracle's dense pass (tests/test_band_model.py checks that
cell by cell).  Also here: the fork graphs both band test files use, and the words the compact derived-gaps layout stores for
given planes."""
import numpy as np

from poasta_amd.graph import GraphBuilder

INF = 0xFFFFFFFF
_BIG = 1 << 40          # INF of the int64 arithmetic: every sum of a finite value and costs stays far below it
ACGT = np.frombuffer(b"ACGT", np.uint8)


def windowed_planes(g, node_row, q, costs, seg_rows, window, bases):
    """-> (M, I, D), uint32 [engine row][column 0..L], INF = 0xFFFFFFFF.  g: FlatGraph; node_row[node] = engine row;
    costs = (mismatch, open, extend)."""
    x, o, e = (int(c) for c in costs)
    oe = o + e
    q = np.asarray(q, np.uint8)
    L = len(q)
    n = g.n
    node_row = np.asarray(node_row, np.int64)
    node_of_row = np.argsort(node_row)
    M = np.full((n, L + 1), _BIG, np.int64)
    I = np.full((n, L + 1), _BIG, np.int64)
    D = np.full((n, L + 1), _BIG, np.int64)
    qpad = np.concatenate([q, np.zeros(1, np.uint8)]).astype(np.int64)     # q[L] = 0: no symbol
    for r in range(n):
        v = int(node_of_row[r])
        b = int(bases[r // seg_rows])
        hi = min(b + window, L + 1)
        if b >= hi:
            continue
        j = np.arange(b, hi)
        w = hi - b
        prs = node_row[g.predecessors(v).astype(np.int64)]
        if len(prs):
            pm = M[prs, b:hi].min(axis=0)
            pd = D[prs, b:hi].min(axis=0)
        else:
            pm = np.full(w, _BIG, np.int64)
            pd = np.full(w, _BIG, np.int64)
        pml = np.full(w, _BIG, np.int64)      # M[p][j - 1]; column b has no diagonal source
        pml[1:] = pm[:-1]
        if v == g.end:
            d = np.minimum(pd + e, _BIG)
            D[r, b:hi] = d
            M[r, b:hi] = np.minimum(pm, d)
            continue
        sym = int(g.symbol[v])
        differs = (qpad[j] != sym) | (j >= L) | (sym == 0)                   # open_d: q[j] mismatches, or j == L
        d = pd + e
        d = np.where(differs, np.minimum(d, pm + oe), d)
        d = np.minimum(d, _BIG)
        left = qpad[np.maximum(j - 1, 0)]
        diag = np.minimum(pml + np.where((left != sym) | (sym == 0), x, 0), _BIG)
        h = np.minimum(diag, d)
        if v == g.start and b == 0:
            h[0] = 0
        # open_i(v, j), j < L: an edge to the end, or a non-end child that mismatches q[j]
        succ = g.successors(v)
        real = [int(c) for c in succ if int(c) != g.end]
        if len(real) < len(succ):
            can_open = j < L
        elif not real:
            can_open = np.zeros(w, bool)
        else:
            syms = {int(g.symbol[c]) for c in real}
            if len(syms) > 1 or 0 in syms:
                can_open = j < L
            else:
                can_open = (j < L) & (qpad[j] != next(iter(syms)))
        a = np.where(can_open, np.minimum(h + oe, _BIG), _BIG)
        # I[j + 1] = min(I[j] + e, a[j]), I[b] = INF  ==  e * j + min over k <= j of (a[k] - e * k)
        k = np.arange(w, dtype=np.int64)
        chain = np.minimum.accumulate(a - e * k) + e * k
        i = np.full(w, _BIG, np.int64)
        i[1:] = np.minimum(chain[:-1], _BIG)
        D[r, b:hi] = d
        I[r, b:hi] = i
        M[r, b:hi] = np.minimum(h, i)

    def out(p):
        return np.where(p >= _BIG, INF, p).astype(np.uint32)
    return out(M), out(I), out(D)


def in_window(n, L, seg_rows, window, bases):
    """bool [row][column]: the cells the windowed pass owns (and the banded kernel writes)"""
    b = np.asarray(bases, np.int64)[np.arange(n) // seg_rows][:, None]
    j = np.arange(L + 1, dtype=np.int64)[None, :]
    return (j >= b) & (j < b + window)


def fork_graph(pre, a, b, post, seed):
    """a backbone of `pre` nodes, two parallel branches of `a` and `b` nodes, a tail of `post` nodes.  The engine's
    chain-following row order puts the second branch's rows after the first's, so a band plan over it moves a window LEFT.
    -> (graph, [the walk through branch A, the walk through branch B])"""
    rng = np.random.default_rng(seed)
    s_pre, s_a, s_b, s_post = (ACGT[rng.integers(0, 4, k)] for k in (pre, a, b, post))
    gb = GraphBuilder()
    i_pre, i_a, i_b, i_post = (gb.add_path(s) for s in (s_pre, s_a, s_b, s_post))
    for br in (i_a, i_b):
        gb.add_edge(i_pre[-1], br[0])
        gb.add_edge(br[-1], i_post[0])
    return gb.finish(), [np.concatenate([s_pre, s_a, s_post]), np.concatenate([s_pre, s_b, s_post])]


def stored_words(M, I, D):
    """The u16 words of the compact derived-gaps layout (TbParams::code_fmt 4) for planes (M, I, D) with INF = 0xFFFFFFFF:
    -> (m_exact, m_word, d_exact, d_word).  Where m_exact, the stored M word is m_word: the score with bit 14 = (I == M) and bit 15 =
    (D == M).  Elsewhere (INF, or >= 0x3FFF) only the score field is defined: it is 0x3FFF.  The same for D against 0x3FFF:
    where d_exact the stored D is d_word, elsewhere it is >= 0x3FFF."""
    M, I, D = (np.asarray(p, np.int64) for p in (M, I, D))
    m_exact = M < 0x3FFF
    m_word = (np.minimum(M, 0x3FFF) | ((I == M).astype(np.int64) << 14) | ((D == M).astype(np.int64) << 15)).astype(np.uint16)
    d_exact = D < 0x3FFF
    d_word = np.minimum(D, 0xFFFF).astype(np.uint16)
    return m_exact, m_word, d_exact, d_word
