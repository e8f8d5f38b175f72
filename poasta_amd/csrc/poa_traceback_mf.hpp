// The traceback walk of poa_kernels.hpp (traceback_wave) written out for the one case the dense one-piece pass runs by default:
// u16 cells, compact layout, TbParams::code_fmt 4 (score in bits 0..13, 0x3FFF = INF, flag A: I == M in bit 14, flag C: D == M in
// bit 15, the two gap-state flags derived by poa_tb_derive.hpp), kept D rows behind the M plane and the quarter-plane gap, absolute
// encoding, no exact pass, no tiled table.  plan_dense_chunk (poa_dense_plan.cpp) selects it; every other layout keeps the
// generic kernel.
//
// Same walk, same bytes: the rounds, the speculation (diagonal prefix, deletion-run ramp, insertion-cycle ramp), the candidate
// order Match / Deletion / Insertion, n_cand and `bad`, the phantom test, the "sic" hop, the start quirk, the panic of a wrapped
// subtraction and the special cases of short reads are those of traceback_wave, statement by statement; what differs is what a
// step costs.  The walk is bound by instruction issue, and the generic routine decides the layout again in
// every load of every lane of every round.  Here
//   * the layout is the code: one load per cell, the flags taken from the loaded word;
//   * a query's planes are addressed by a base pointer and 32-bit element offsets (the host checks that they fit);
//   * a chain row has one candidate load and no predecessor loop, and its predecessor is the row above (no pred_rows load); the
//     row record, the cell and the candidate are requested together: one memory round trip per round on a chain;
//   * the state of the walk selects one of three step routines, each inlined once for the rounds and once for the cycle of an
//     insertion run; the end row's Match-state rules live in the first hop alone (rows are in topological order: no later
//     Match or Insertion step stands in the end row), a Deletion step tests the row's ROW_END flag as the generic one does;
//   * the ambiguity and start-quirk flags are gathered per lane (a lane inside the accepted prefix keeps its own) and reduced
//     once per walk instead of two ballots per round; the panic ballot is taken wave-wide first and almost never needed.
// Properties (a) and (b) of DESIGN.md §6 hold as before: a lane past the accepted prefix contributes nothing, and no address is
// formed from a loaded plane value (rows come from the graph tables and the walk's position, columns from the position).
#pragma once
#include "poa_kernels.hpp"

namespace poa_amd {

// what the steps and poa_tb_derive.hpp read of one query
struct MfCtx {
    const RowMeta* rows;
    const uint32_t* pred_rows;
    const uint16_t* M;          // the query's M plane
    const uint16_t* D;          // its kept D rows
    const uint32_t* d_slot;     // nullptr: the D rows are stored by row
    const uint32_t* pred_dslot;
    const uint8_t* q;
    uint32_t L, pitch, x, o, e;
    __device__ __forceinline__ uint32_t raw(uint32_t row, uint32_t j) const { return (uint32_t)M[row * pitch + j]; }
    __device__ __forceinline__ void cell(uint32_t row, uint32_t j, uint32_t& v, uint32_t& a, uint32_t& cf) const {
        const uint32_t r = raw(row, j);
        v = mf_value(r); a = (r >> 14) & 1u; cf = (r >> 15) & 1u;
    }
    __device__ __forceinline__ uint32_t m(uint32_t row, uint32_t j) const { return mf_value(raw(row, j)); }
    __device__ __forceinline__ uint32_t d_at(uint32_t slot, uint32_t j) const { return PlaneIO<uint16_t>::widen((uint32_t)D[slot * pitch + j]); }
    __device__ __forceinline__ uint32_t d_kept(uint32_t row, uint32_t j) const { return d_at(d_slot ? d_slot[row] : row, j); }
    __device__ __forceinline__ uint32_t pred(uint32_t k) const { return pred_rows[k]; }
    __device__ __forceinline__ uint32_t pred_d(uint32_t k, uint32_t j) const { return d_at(pred_dslot ? pred_dslot[k] : pred_rows[k], j); }
};

__device__ __forceinline__ void mf_cand(TbStep& f, uint32_t& n_cand, uint32_t row, uint32_t j, uint32_t st) {
    if (!f.found) { f.row = row; f.j = j; f.st = st; f.found = true; }
    n_cand++;
}
// a - b as the reference's Score subtraction: landing on u32::MAX is its panic
__device__ __forceinline__ uint32_t mf_sub(uint32_t a, uint32_t b, bool& panic) {
    const uint32_t r = a - b;
    if (r == INF) panic = true;
    return r;
}

// Match state at (row, j), m = rows[row].  raw: the cell's stored word; up: the score of M[row-1][j-1] (INF where row or j is 0) —
// the caller loads both beside the row record, so that a chain row's step is one memory round trip.  END: the end row (first hop
// only) — it equals every symbol and reads its predecessors at the same column.
template <bool END>
__device__ __forceinline__ TbStep mf_step_m(const MfCtx& c, const RowMeta& m, uint32_t row, uint32_t j, uint32_t raw, uint32_t up,
                                            uint32_t& n_cand, bool& panic) {
    TbStep f{0, 0, 0, false, 0, m.node};
    n_cand = 0;
    const uint32_t cs = mf_value(raw);
    f.cs = cs;
    if (cs == INF) return f;
    if (j > 0) {
        const bool moe = END || (uint32_t)m.sym == (uint32_t)c.q[j - 1];
        const uint32_t pj = END ? j : j - 1;
        // the reference evaluates `curr_score - mismatch` per predecessor: never for a row without predecessors
        const uint32_t target = (moe || m.pred_count == 0) ? cs : mf_sub(cs, c.x, panic);
        if (!END && (m.flags & ROW_CHAIN)) {
            if (up == target) mf_cand(f, n_cand, row - 1, pj, 0);
        } else {
            for (uint32_t k = 0; k < m.pred_count; ++k) {   // trait order
                const uint32_t pr = c.pred_rows[m.pred_begin + k];
                if (c.m(pr, pj) == target) mf_cand(f, n_cand, pr, pj, 0);
            }
        }
    }
    if (raw & 0x8000u) mf_cand(f, n_cand, row, j, 1);
    if (raw & 0x4000u) mf_cand(f, n_cand, row, j, 2);
    return f;
}
// the two loads of a Match-state step at (row, j)
__device__ __forceinline__ void mf_load_m(const MfCtx& c, uint32_t row, uint32_t j, uint32_t& raw, uint32_t& up) {
    const uint32_t off = row * c.pitch + j;
    raw = (uint32_t)c.M[off];
    up = (row > 0 && j > 0) ? mf_value((uint32_t)c.M[off - c.pitch - 1u]) : INF;
}

// Deletion state at (row, j) with the carried score cs of the D cell; above: the score of M[row-1][j] (read by chain rows only; the
// caller loads it beside the row record)
template <bool END>
__device__ __forceinline__ TbStep mf_step_d(const MfCtx& c, const RowMeta& m, uint32_t row, uint32_t j, uint32_t cs, uint32_t above,
                                            uint32_t& n_cand, bool& bad, bool& panic) {
    TbStep f{0, 0, 0, false, cs, m.node};
    n_cand = 0;
    if (cs == INF) return f;
    if (m.pred_count == 0) return f;
    const uint32_t t_open = mf_sub(mf_sub(cs, c.o, panic), c.e, panic), t_ext = mf_sub(cs, c.e, panic);
    // (a Deletion step of the rounds can stand in the end row: the first hop's Match step may take flag C at the end cell)
    const bool is_end = END || (m.flags & ROW_END) != 0;
    const bool real_open = !is_end && (j >= c.L || (uint32_t)m.sym != (uint32_t)c.q[j]);
    if (m.flags & ROW_CHAIN) {   // one predecessor, the row above
        const uint32_t v = above;
        if (v == t_open) mf_cand(f, n_cand, row - 1, j, 0);
        else if (!real_open && v < t_open) bad = true;  // phantom edge the reference does not re-check
        if (tbd_d_extends(c, row, j, cs)) mf_cand(f, n_cand, row - 1, j, 1);
    } else {
        for (uint32_t k = 0; k < m.pred_count; ++k) {
            const uint32_t pr = c.pred_rows[m.pred_begin + k];
            const uint32_t v = c.m(pr, j);
            if (v == t_open) mf_cand(f, n_cand, pr, j, 0);
            else if (!real_open && v < t_open) bad = true;
        }
        for (uint32_t k = 0; k < m.pred_count; ++k)   // predecessors of a non-chain row keep their D row
            if (c.pred_d(m.pred_begin + k, j) == t_ext) mf_cand(f, n_cand, c.pred_rows[m.pred_begin + k], j, 1);
    }
    return f;
}

// Insertion state at (row, j) with the carried score cs of the I cell
__device__ __forceinline__ TbStep mf_step_i(const MfCtx& c, const RowMeta& m, uint32_t row, uint32_t j, uint32_t cs, uint32_t& n_cand,
                                            bool& bad, bool& panic) {
    TbStep f{0, 0, 0, false, cs, m.node};
    n_cand = 0;
    if (cs == INF) return f;
    if (j > 0) {
        const uint32_t t_open = mf_sub(mf_sub(cs, c.o, panic), c.e, panic), t_ext = mf_sub(cs, c.e, panic);
        const uint32_t pm = c.m(row, j - 1);
        if (pm == t_open) mf_cand(f, n_cand, row, j - 1, 0);
        else if (!tbd_open_i(c, m, j - 1) && pm < t_open) bad = true;
        if (tbd_i_extends(c, m, row, j, cs)) {
            const bool only = (n_cand == 0);
            mf_cand(f, n_cand, row, j - 1, 0);  // sic: the reference returns Match here (gap_affine.rs:649)
            if (only && pm != t_ext) bad = true;  // the hop lands on M[row][j-1] which is not that I value
        }
    }
    return f;
}

// GW lanes per walk; `lane` is the lane within the group.  The comments of traceback_wave apply; only what differs is said here.
template <int GW>
__device__ __forceinline__ void traceback_mf_walk(const TbParams& P, const uint32_t qi, const uint32_t lane) {
    const uint32_t gbase = (threadIdx.x & 63u) - lane;  // first lane of my group within the wave
    // the group's bits of a ballot, bit i = lane i of the group
    auto gballot = [&](bool pred) -> uint64_t {
        const uint64_t b = __ballot(pred);
        if (GW == 64) return b;
        const uint32_t w = (gbase & 32u) ? (uint32_t)(b >> 32) : (uint32_t)b;
        return (uint64_t)((w >> (gbase & 31u)) & (uint32_t)((1ull << (GW & 63)) - 1ull));
    };
    auto ones = [](uint64_t b) -> uint32_t { return (b == ~0ull) ? 64u : (uint32_t)__builtin_ctzll(~b); };   // trailing ones
    auto bc = [&](uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)(gbase + src)); };

    const uint64_t qbeg = P.qoff[qi];
    MfCtx c;
    c.rows = P.rows; c.pred_rows = P.pred_rows;
    c.L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    c.q = P.qseq + qbeg;
    c.pitch = P.pitch[qi];
    const uint64_t RP = (uint64_t)P.n_rows * c.pitch;
    c.M = reinterpret_cast<const uint16_t*>(P.planes) + P.plane_off[qi];
    c.D = c.M + RP + RP / 4;   // compact_plane_elems
    c.d_slot = P.d_slot; c.pred_dslot = P.pred_dslot;
    c.x = P.cost_x; c.o = P.cost_o; c.e = P.cost_e;
    const uint32_t L = c.L, start_row = P.start_row, end_row = P.end_row;

    uint2* out = P.scratch + P.scratch_off[qi];
    const uint32_t cap = (uint32_t)(P.scratch_off[qi + 1] - P.scratch_off[qi]);
    uint32_t cnt = 0;     // group-uniform
    uint32_t flags = 0;   // group-uniform
    uint32_t lflags = 0;  // this lane's own: AMBIGUOUS / START_QUIRK of steps it evaluated inside an accepted prefix
    auto emit_at = [&](uint32_t pos, uint32_t rpos, uint32_t qpos) {
        if (pos < cap) out[cap - 1 - pos] = make_uint2(rpos, qpos);
    };

    if (lane == 0) P.score[qi] = c.m(end_row, L);
    const uint32_t end_node = c.rows[end_row].node;

    bool done = false;
    uint32_t crow = 0, cj = 0, cst = 0;
    uint32_t gcs = INF;
    if (L == 0) done = true;
    if (!done && L == 1) {   // "single nucleotide perfect match": the end node equals every symbol
        flags |= POA_FLAG_SHORT_QUERY;
        if (lane == 0) emit_at(0, end_node, 0);
        cnt = 1;
        done = true;
    }
    if (!done) {
        // first hop from the end cell: Match, .or_else(Insertion), .or_else(Deletion).  The end row has no insertion state
        // (I = INF: that step finds nothing and cannot panic) and keeps its D row
        uint32_t f0 = 0, fr = 0, fj = 0, fs = 0, fallback = 0, fg = INF;
        if (lane == 0) {
            uint32_t nc; bool bad = false, pn = false;
            const RowMeta me = c.rows[end_row];
            TbStep cur = mf_step_m<true>(c, me, end_row, L, c.raw(end_row, L), INF, nc, pn);
            fg = cur.cs;
            if (cur.found && !pn && nc != 1) f0 |= POA_FLAG_AMBIGUOUS;
            if (!cur.found && !pn) {
                cur = mf_step_d<true>(c, me, end_row, L, c.d_kept(end_row, L), end_row > 0 ? c.m(end_row - 1, L) : INF, nc, bad, pn);
                fg = cur.cs;
                if (!pn) {
                    if (!cur.found) { f0 |= POA_FLAG_REF_PANIC; fallback = 1; }
                    else f0 |= POA_FLAG_AMBIGUOUS;
                    if (cur.found && cur.st == 1) fg = cur.cs - c.e;  // stepped D -> D
                }
            }
            if (pn) { f0 |= POA_FLAG_REF_PANIC; fallback = 2; }
            fr = cur.row; fj = cur.j; fs = cur.st;
        }
        flags |= bc(f0, 0);
        const uint32_t fb = bc(fallback, 0);
        if (fb) {
            if (fb == 2) flags |= POA_FLAG_TRUNCATED;
            if (fb == 1 && L <= 3) {
                if (lane == 0) for (uint32_t i = 0; i < L; ++i) emit_at(i, end_node, L - 1 - i);
                cnt = L;
            }
            done = true;
        } else {
            crow = bc(fr, 0); cj = bc(fj, 0); cst = bc(fs, 0); gcs = bc(fg, 0);
        }
    }
    bool reached_start = done;
    uint32_t d_run = 0, i_run = 0;
    const uint32_t max_depth = P.spec_depth < (uint32_t)GW ? P.spec_depth : (uint32_t)GW;
    while (!done) {
        uint32_t depth = 1;
        if (cst == 2 && crow != start_row && max_depth > 1 && cj > 1) {
            uint32_t idepth = i_run < max_depth ? (i_run ? i_run : 1u) : max_depth;
            if (idepth < 2) idepth = 2;
            if (cj < idepth) idepth = cj;
            const bool iact = lane < idepth;
            const uint32_t jj = cj - lane;
            TbStep sI{0, 0, 0, false, 0, 0}, sM{0, 0, 0, false, 0, 0};
            uint32_t ncI = 0, ncM = 0;
            bool badI = false, pnI = false, pnM = false;
            RowMeta mi{};
            if (iact) {
                // an Insertion step stays in its row and lands one column to the left: the Match step of the cycle reads the same
                // row record, and its two cells are requested now, beside those of the Insertion step (jj >= 1)
                mi = c.rows[crow];
                uint32_t rawL, upL;
                mf_load_m(c, crow, jj - 1, rawL, upL);
                const uint32_t gcs_i = lane == 0 ? gcs : c.m(crow, jj);
                sI = mf_step_i(c, mi, crow, jj, gcs_i, ncI, badI, pnI);
                if (sI.found && !pnI) sM = mf_step_m<false>(c, mi, crow, sI.j, rawL, upL, ncM, pnM);
            }
            const bool cyc = iact && sI.found && !pnI && sI.j + 1 == jj && sM.found && !pnM && sM.st == 2 && sM.row == crow && sM.j == sI.j;
            const uint32_t ip = ones(gballot(cyc));   // accepted cycles, <= idepth
            if (ip > 0) {
                if (lane < ip) {
                    if (ncI != 1 || badI || ncM != 1) lflags |= POA_FLAG_AMBIGUOUS;
                    if (sI.j == 0 && (uint32_t)mi.sym == (uint32_t)c.q[0]) lflags |= POA_FLAG_START_QUIRK;   // (crow is not the start row here)
                    emit_at(cnt + lane, POA_NONE, jj - 1);
                }
                cnt += ip;
                cj -= ip;
                gcs = bc(sM.cs, ip - 1);
                i_run += ip;
                continue;
            }
            const uint32_t w0 = bc(((sI.found && !pnI) ? 1u : 0u) | ((ncI != 1 || badI) ? 2u : 0u), 0);
            if (w0 & 1u) {
                if (w0 & 2u) flags |= POA_FLAG_AMBIGUOUS;
                if (lane == 0) emit_at(cnt, POA_NONE, cj - 1);
                cnt += 1;
                const uint32_t n_row = crow, n_j = bc(sI.j, 0);   // an Insertion step lands in Match state, in its own row
                if (n_j == 0 && (uint32_t)c.rows[n_row].sym == (uint32_t)c.q[0]) flags |= POA_FLAG_START_QUIRK;
                cj = n_j; cst = 0;
                i_run = 0;
                continue;
            }
        }
        if (cst != 2) i_run = 0;
        if (cst == 0) {
            depth = max_depth;
            if (crow + 1 < depth) depth = crow + 1;
            if (cj + 1 < depth) depth = cj + 1;
        } else if (cst == 1) {
            depth = d_run < max_depth ? (d_run ? d_run : 1u) : max_depth;
            if (crow + 1 < depth) depth = crow + 1;
        }
        if (cst != 1) d_run = 0;
        const bool active = lane < depth;
        const uint32_t my_row = crow - lane, my_j = (cst == 0) ? cj - lane : cj;
        TbStep bt{0, 0, 0, false, 0, 0};
        uint32_t nc = 0;
        bool bad = false, pn = false;
        if (active) {
            const RowMeta m = c.rows[my_row];
            if (cst == 0) {
                uint32_t raw, up;
                mf_load_m(c, my_row, my_j, raw, up);
                bt = mf_step_m<false>(c, m, my_row, my_j, raw, up, nc, pn);
            } else if (cst == 1) {
                const uint32_t above = my_row > 0 ? c.m(my_row - 1, my_j) : INF;
                bt = mf_step_d<false>(c, m, my_row, my_j, gcs - lane * c.e, above, nc, bad, pn);
            } else bt = mf_step_i(c, m, my_row, my_j, gcs, nc, bad, pn);
        }
        const bool amb = active && bt.found && (nc != 1 || bad);
        const bool quirk = active && bt.found && bt.st == 0 && bt.j == 0 && bt.row != start_row && cst != 1 &&
                           (uint32_t)c.rows[bt.row].sym == (uint32_t)c.q[0];
        const bool regular = active && bt.found && bt.row + 1 == my_row && bt.row != start_row &&
                             ((cst == 0 && bt.st == 0 && bt.j + 1 == my_j) || (cst == 1 && bt.st == 1 && bt.j == my_j));
        uint32_t p = ones(gballot(regular));  // accepted prefix, <= depth
        bool dies = false;
        if (__ballot(active && pn)) {   // some walk of the wave wrapped a subtraction: rare
            const uint64_t pnb = gballot(active && pn);
            const uint32_t first_pn = pnb ? (uint32_t)__builtin_ctzll(pnb) : 64u;
            dies = pnb != 0 && first_pn <= p;
            if (dies) p = first_pn;
        }
        if (lane < p) {
            if (amb) lflags |= POA_FLAG_AMBIGUOUS;
            if (quirk) lflags |= POA_FLAG_START_QUIRK;
            emit_at(cnt + lane, bt.node, cst == 0 ? my_j - 1 : POA_NONE);
        }
        cnt += p;
        if (dies) {
            flags |= POA_FLAG_REF_PANIC;
            break;
        }
        if (p == depth) {
            crow -= depth;
            if (cst == 0) cj -= depth;
            else { gcs -= depth * c.e; d_run += depth; }
            continue;
        }
        // lane p deviates: replay the sequential rule with its results
        const uint32_t dw = bc((bt.found ? 1u : 0u) | (amb ? 2u : 0u) | (quirk ? 4u : 0u) | (bt.st << 3), p);
        const uint32_t d_row = bc(bt.row, p), d_j = bc(bt.j, p), d_cs = bc(bt.cs, p), d_node = bc(bt.node, p);
        const uint32_t d_st = dw >> 3;
        const uint32_t cur_j = (cst == 0) ? cj - p : cj, cur_st = cst;
        if (!(dw & 1u)) break;
        if (dw & 2u) flags |= POA_FLAG_AMBIGUOUS;
        if (cur_st == 0 && d_st != 0) {  // zero-cost gap close: no pair
            crow = d_row; cj = d_j; cst = d_st;
            gcs = d_cs;
            continue;
        }
        if (lane == 0) {
            if (cur_st == 0) emit_at(cnt, d_node, cur_j - 1);
            else if (cur_st == 2) emit_at(cnt, POA_NONE, cur_j - 1);
            else emit_at(cnt, d_node, POA_NONE);
        }
        cnt += 1;
        if (dw & 4u) flags |= POA_FLAG_START_QUIRK;
        if (d_row == start_row) { reached_start = true; break; }
        if (cur_st == 1 && d_st == 1) gcs = d_cs - c.e;
        if (cur_st == 1) d_run += p + 1;
        crow = d_row; cj = d_j; cst = d_st;
    }
    if (!reached_start) flags |= POA_FLAG_TRUNCATED;
    if (gballot((lflags & POA_FLAG_AMBIGUOUS) != 0)) flags |= POA_FLAG_AMBIGUOUS;
    if (gballot((lflags & POA_FLAG_START_QUIRK) != 0)) flags |= POA_FLAG_START_QUIRK;
    if (lane == 0) {
        P.flags[qi] = flags;
        P.n_pairs[qi] = cnt < cap ? cnt : cap;
    }
}

// same grid as poa_traceback_kernel<uint16_t, true, GW>: 256 / GW walks per 256-thread block
template <int GW>
__global__ __launch_bounds__(256) void poa_traceback_mf_kernel(TbParams P) {
    const uint32_t lane = threadIdx.x & (uint32_t)(GW - 1);
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) / (uint32_t)GW;  // uniform over the group
    if (wq >= P.n_queries) return;
    traceback_mf_walk<GW>(P, P.first_query + wq, lane);
}

}  // namespace poa_amd
