// fs2_align_tree.hip — the forced aligner's triphone stage: the likelihood gain of every question at every open node of the
// decision tree, in fp64 over the item table that stays on the device.  The specification is the "Triphones" paragraph of
// fastspeech2_amd/align.py's docstring (mirrored in DESIGN.md); tests/align_tri_ref.py restates it in numpy.
//
// Shapes.  The item table is [n_items][lds] with 1 + 2 D columns {n, a[0..D), q[0..D)} per row; left / right [n_items] int32 are the
// context symbols of the items, member [n_sets][n_symbols] uint8 the question sets.  Node m owns the items list[offs[m] .. offs[m + 1]).
// Question qi < n_sets asks whether left[item] is in set qi, question n_sets + qi whether right[item] is.  Only listed rows of the
// table are read (the tests poison the others with NaN).  An item index outside [0, n_items) is skipped and a symbol outside
// [0, n_symbols) answers no, so nothing out of bounds is read whatever the lists hold.
//
//   fs2_align_tree_gains   one workgroup (four waves) per node.  First the node's own likelihood: n in every thread, a_d and q_d one
//                          thread per d, items ascending; the D terms are added by one thread, d ascending.  Then every wave takes
//                          tiles of 16 questions (tile = wave, wave + 4, ...).  For a tile the yes-sums and the no-sums are 0/1
//                          matrices times the item table: v_mfma_f64_16x16x4_f64 with A[i = question][k = item] = the answer (1 - the
//                          answer for the no side), B[k = item][j = column] = the table, items ascending in steps of four; the last
//                          step is padded with zeros in both operands.  One pass with n broadcast to all 16 columns gives n_yes and
//                          n_no in the lanes that need them; then 16 columns of a and the matching 16 of q are accumulated together
//                          (four accumulators), the 16 x 16 terms log(2 pi v) + 1 go through LDS and lane i adds question i's terms
//                          d ascending.  Nothing per (node, question, column) leaves the chip.  Both sides are accumulated directly:
//                          no subtraction from the node's sums.  The order of every sum depends on the node's item count and D alone,
//                          and a question's arithmetic does not depend on its place in a tile: identical sets give identical bits,
//                          and so do two sets that part a node's items the same way or the other way round (yes and no go through
//                          the same instructions and L(yes) + L(no) is formed without a fused multiply-add).
#include "fs2_common.h"

#define TREE_MAX_SETS 1024          // question sets (2048 questions): generated sets number twice the phones
#define TREE_WAVES 4
#define TREE_QT 16                  // questions per tile, the instruction's i
#define TREE_DT 16                  // dimensions per tile, the instruction's j

typedef double tree_f64x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ double tree_term(double a, double q, double n, double fl) {
    const double mu = a / n;
    const double v = fmax(q / n - mu * mu, fl);
    return log(2.0 * M_PI * v) + 1.0;
}

__global__ void __launch_bounds__(TREE_WAVES * 64) align_tree_gains_kernel(
    const double* __restrict__ sums, long lds, int n_items, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
    const int32_t* __restrict__ offs, const int32_t* __restrict__ items, int n_list, const uint8_t* __restrict__ member, int n_sets,
    int n_sym, const double* __restrict__ floor_, int D, double min_occ, int32_t* __restrict__ best_q, double* __restrict__ best_gain,
    double* __restrict__ gains, double* __restrict__ n_yes, long ldq) {
    __shared__ double term_s[TREE_WAVES * 64];
    __shared__ double node_s;
    __shared__ double ty_s[TREE_WAVES][TREE_QT][TREE_DT + 1], tn_s[TREE_WAVES][TREE_QT][TREE_DT + 1];
    __shared__ double ny_s[TREE_WAVES][TREE_QT], nn_s[TREE_WAVES][TREE_QT];
    __shared__ double bg_s[TREE_WAVES][TREE_QT];
    __shared__ int bq_s[TREE_WAVES][TREE_QT];
    const int node = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int o0 = min(max(offs[node], 0), n_list), o1 = min(max(offs[node + 1], o0), n_list);
    const int cnt = o1 - o0;
    const int32_t* __restrict__ list = items + o0;

    // ---- L(node)
    double n_all = 0.0;
    for (int k = 0; k < cnt; ++k) {
        const int it = list[k];
        if (it >= 0 && it < n_items) n_all += sums[(size_t)it * lds];
    }
    double s_all = 0.0;
    for (int d0 = 0; d0 < D; d0 += TREE_WAVES * 64) {
        const int d = d0 + tid;
        double term = 0.0;
        if (d < D && n_all > 0.0) {
            double a = 0.0, q = 0.0;
            for (int k = 0; k < cnt; ++k) {
                const int it = list[k];
                if (it >= 0 && it < n_items) {
                    a += sums[(size_t)it * lds + 1 + d];
                    q += sums[(size_t)it * lds + 1 + D + d];
                }
            }
            term = tree_term(a, q, n_all, floor_[d]);
        }
        term_s[tid] = term;
        __syncthreads();
        if (tid == 0) {
            const int nd = min(TREE_WAVES * 64, D - d0);
            for (int t = 0; t < nd; ++t) s_all += term_s[t];
        }
        __syncthreads();
    }
    if (tid == 0) node_s = n_all > 0.0 ? -0.5 * n_all * s_all : 0.0;
    __syncthreads();
    const double l_node = node_s;

    // ---- the questions
    const int Q = 2 * n_sets, ntile = (Q + TREE_QT - 1) / TREE_QT, ndt = (D + TREE_DT - 1) / TREE_DT;
    const int ai = lane & 15, ak = lane >> 4;
    double bg = -INFINITY;
    int bq = -1;
    for (int t0 = 0; t0 < ntile; t0 += TREE_WAVES) {
        const int tile = t0 + w;
        const bool active = tile < ntile;                                  // the same for the whole wave
        const int qa = tile * TREE_QT + ai;                                // the question of this lane's row of A
        const bool qok = active && qa < Q;
        const int side = qa >= n_sets ? 1 : 0;
        const int32_t* __restrict__ ctx = side ? right : left;
        const uint8_t* __restrict__ row = member + (size_t)(qok ? qa - side * n_sets : 0) * n_sym;

        tree_f64x4 cy = {0.0, 0.0, 0.0, 0.0}, cn = {0.0, 0.0, 0.0, 0.0};
        if (active) {
            for (int g = 0; g < cnt; g += 4) {
                const int k = g + ak;
                const int it = k < cnt ? list[k] : -1;
                double ay = 0.0, an = 0.0, b = 0.0;
                if (it >= 0 && it < n_items) {
                    const int c = ctx[it];
                    const bool m = qok && c >= 0 && c < n_sym && row[c] != 0;
                    ay = m ? 1.0 : 0.0;
                    an = m ? 0.0 : 1.0;
                    b = sums[(size_t)it * lds];
                }
                cy = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, b, cy, 0, 0, 0);
                cn = __builtin_amdgcn_mfma_f64_16x16x4f64(an, b, cn, 0, 0, 0);
            }
        }
        bool el[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                      // D[i = ak + 4 r][j = ai]: n of question ak + 4 r in every column
            el[r] = cy[r] >= min_occ && cn[r] >= min_occ;
            if (ai == 0) {
                ny_s[w][ak + 4 * r] = cy[r];
                nn_s[w][ak + 4 * r] = cn[r];
            }
        }
        double sy = 0.0, sn = 0.0;                                         // lanes 0..15: the sums over d of question `lane`
        for (int dt = 0; dt < ndt; ++dt) {
            const int col = dt * TREE_DT + ai;
            const bool cok = col < D;
            tree_f64x4 aY = {0.0, 0.0, 0.0, 0.0}, qY = aY, aN = aY, qN = aY;
            if (active) {
                for (int g = 0; g < cnt; g += 4) {
                    const int k = g + ak;
                    const int it = k < cnt ? list[k] : -1;
                    double ay = 0.0, an = 0.0, ba = 0.0, bq2 = 0.0;
                    if (it >= 0 && it < n_items) {
                        const int c = ctx[it];
                        const bool m = qok && c >= 0 && c < n_sym && row[c] != 0;
                        ay = m ? 1.0 : 0.0;
                        an = m ? 0.0 : 1.0;
                        if (cok) {
                            ba = sums[(size_t)it * lds + 1 + col];
                            bq2 = sums[(size_t)it * lds + 1 + D + col];
                        }
                    }
                    aY = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, ba, aY, 0, 0, 0);
                    qY = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, bq2, qY, 0, 0, 0);
                    aN = __builtin_amdgcn_mfma_f64_16x16x4f64(an, ba, aN, 0, 0, 0);
                    qN = __builtin_amdgcn_mfma_f64_16x16x4f64(an, bq2, qN, 0, 0, 0);
                }
            }
            const double fl = cok ? floor_[col] : 1.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double ty = 0.0, tn = 0.0;
                if (cok && el[r]) {                                        // no variance is formed for an ineligible split
                    ty = tree_term(aY[r], qY[r], cy[r], fl);
                    tn = tree_term(aN[r], qN[r], cn[r], fl);
                }
                ty_s[w][ak + 4 * r][ai] = ty;
                tn_s[w][ak + 4 * r][ai] = tn;
            }
            __syncthreads();
            if (lane < TREE_QT) {
                const int nd = min(TREE_DT, D - dt * TREE_DT);
                for (int dl = 0; dl < nd; ++dl) {
                    sy += ty_s[w][lane][dl];
                    sn += tn_s[w][lane][dl];
                }
            }
            __syncthreads();
        }
        if (active && lane < TREE_QT) {
            const int q = tile * TREE_QT + lane;
            if (q < Q) {
                const double ny = ny_s[w][lane], nn = nn_s[w][lane];
                const bool e = ny >= min_occ && nn >= min_occ;
                double gain = -INFINITY;
                if (e) {
#pragma clang fp contract(off)                                             // no fused multiply-add: the two sides may change places
                    const double ly = -0.5 * ny * sy, ln = -0.5 * nn * sn;
                    gain = (ly + ln) - l_node;
                }
                if (gains) gains[(size_t)node * ldq + q] = gain;
                if (n_yes) n_yes[(size_t)node * ldq + q] = ny;
                if (gain > bg) {
                    bg = gain;
                    bq = q;
                }
            }
        }
    }
    if (lane < TREE_QT) {
        bg_s[w][lane] = bg;
        bq_s[w][lane] = bq;
    }
    __syncthreads();
    if (tid == 0) {
        double g = -INFINITY;
        int q = -1;
        for (int ww = 0; ww < TREE_WAVES; ++ww)
            for (int l = 0; l < TREE_QT; ++l) {
                const double cg = bg_s[ww][l];
                const int cq = bq_s[ww][l];
                if (cq >= 0 && (cg > g || (cg == g && cq < q))) {
                    g = cg;
                    q = cq;
                }
            }
        best_q[node] = q;
        best_gain[node] = g;
    }
}

extern "C" int fs2_align_max_tree_sets(void) { return TREE_MAX_SETS; }

extern "C" int fs2_align_tree_gains(const double* sums, long lds, int n_items, const int32_t* left, const int32_t* right,
                                    const int32_t* offs, const int32_t* items, int n_list, int n_nodes, const uint8_t* member,
                                    int n_sets, int n_symbols, const double* floor, int D, double min_occ, int32_t* best_q,
                                    double* best_gain, double* gains, double* n_yes, long ldq, hipStream_t stream) {
    FS2_CHECK_ARG(sums && left && right && offs && items && member && floor && best_q && best_gain, "align_tree_gains: null pointer");
    FS2_CHECK_ARG(n_sets >= 1 && n_sets <= TREE_MAX_SETS, "align_tree_gains: %d question sets, supported are 1..%d", n_sets, TREE_MAX_SETS);
    FS2_CHECK_ARG(min_occ >= 1.0, "align_tree_gains: tri_min_occ must be at least 1, got %g", min_occ);
    FS2_CHECK_ARG(D >= 1 && n_items >= 0 && n_list >= 0 && n_nodes >= 0 && n_symbols >= 1 && lds >= 1 + 2 * (long)D,
                  "align_tree_gains: bad shape D=%d n_items=%d n_list=%d n_nodes=%d n_symbols=%d lds=%ld", D, n_items, n_list, n_nodes,
                  n_symbols, lds);
    FS2_CHECK_ARG((!gains && !n_yes) || ldq >= 2 * (long)n_sets, "align_tree_gains: ldq=%ld below the %d questions", ldq, 2 * n_sets);
    if (n_nodes == 0) return FS2_OK;
    align_tree_gains_kernel<<<n_nodes, TREE_WAVES * 64, 0, stream>>>(sums, lds, n_items, left, right, offs, items, n_list, member, n_sets,
                                                                    n_symbols, floor, D, min_occ, best_q, best_gain, gains, n_yes, ldq);
    FS2_CHECK_LAUNCH("align_tree_gains");
    return FS2_OK;
}
