// fs2_align_loop.hip — Viterbi over a free loop of all phones on the aligner's acoustic model: the phone sequence the model hears.
// The specification is the docstring of fastspeech2_amd/recognize.py (mirrored in DESIGN.md); tests/align_loop_ref.py restates it
// in numpy.
//
// Layout.  P phones of S states; state j = p S + s is emission class j, C = P S of them.  E [B][Tmax][>= C] fp64 (strides lde_b,
// lde_t) comes from fs2_align_emit / fs2_align_emit_gmm with sid = 0 .. C - 1.  Costs, fp64, finite or -inf: self_[C], next_[C] (the
// arc s - 1 -> s, unused at s = 0), link[P][ldl] (leave the last state of p, enter the first state of q), init[P], final_[P].
//
//   fs2_align_loop_viterbi    one workgroup per utterance, one state per lane, the previous frame's row double-buffered in LDS, the
//                             next frame's E loaded one frame ahead: the scan of align_viterbi_kernel.  The lane of a phone's first
//                             state takes the maximum over the P exit scores (the last states of all phones, read from the LDS row)
//                             plus link[p][q], p ascending; link itself is staged in LDS when it fits beside the rows, else read
//                             from global memory (lanes of consecutive q read consecutive doubles either way).
//   fs2_align_loop_backtrack  backpointers -> the segments (phone, first frame) in time order, one lane per utterance
//
// Backpointer codes: 0 self, 1 next, 2 + p entry from phone p; a later candidate replaces an earlier one only when strictly larger.
// Only adds and compares of the oracle's operands: results are exact.  Nothing at t >= lens[b] is read or written.  No atomics.
#include "fs2_common.h"

#define ALP_MAX_PHONES 253          // the backpointer 2 + p is one byte
#define ALP_MAX_STATES 1024         // fs2_align_max_states(): one state per lane of the largest workgroup
#define ALP_LDS_BYTES 65536         // what one workgroup takes at most: the rows and, when it fits beside them, link

static __device__ __forceinline__ int alp_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }
static __device__ __forceinline__ double alp_ninf() { return -__builtin_huge_val(); }

// row[.][j + 1] holds the previous frame's value of state j and row[.][0] = -inf, as in align_viterbi_kernel; the exit score of
// phone p is row[.][p S + S].  Frame t reads buffer (t - 1) & 1 and writes buffer t & 1; the barrier at the top of frame t + 1 orders
// those writes before their readers and frame t's reads before frame t + 1's overwrites.  LINK_LDS: lk holds link as [P][P].
template <int NT>
__global__ void __launch_bounds__(NT) align_loop_viterbi_kernel(const double* __restrict__ E, long lde_b, long lde_t,
                                                                const int32_t* __restrict__ lens, const double* __restrict__ self_,
                                                                const double* __restrict__ next_, const double* __restrict__ link,
                                                                long ldl, const double* __restrict__ init,
                                                                const double* __restrict__ final_, uint8_t* __restrict__ bp, long ldp_b,
                                                                long ldp_t, int32_t* __restrict__ end, double* __restrict__ score,
                                                                int Tmax, int P, int S, int link_lds) {
    __shared__ double row[2][NT + 1];
    extern __shared__ double lk[];
    const int b = blockIdx.x, j = threadIdx.x, T = alp_len(lens, b, Tmax), C = P * S;
    if (T == 0) {
        if (j == 0) {
            end[b] = -1;
            score[b] = alp_ninf();
        }
        return;
    }
    const bool on = j < C;
    const int q = j / S, s = j - q * S;
    if (link_lds) {
        for (int k = j; k < P * P; k += NT) {
            const int p = k / P;
            lk[k] = link[(size_t)p * ldl + (k - p * P)];
        }
    }
    const double* L = link_lds ? lk + q : link + q;                        // L[p * ldL] = link[p][q]
    const long ldL = link_lds ? P : ldl;
    const double* Eb = E + (size_t)b * lde_b + j;
    uint8_t* Pb = bp + (size_t)b * ldp_b + j;
    const double w0 = on ? self_[j] : 0.0, w1 = (on && s > 0) ? next_[j] : 0.0;
    if (j == 0) row[0][0] = row[1][0] = alp_ninf();
    double a = alp_ninf();
    if (on && s == 0) a = init[q] + Eb[0];
    if (on) Pb[0] = 0;
    row[0][j + 1] = a;
    double e_next = (on && T > 1) ? Eb[lde_t] : 0.0;
    for (int t = 1; t < T; ++t) {
        __syncthreads();                                                   // the first one also orders the staging of link
        const double e = e_next;
        if (on && t + 1 < T) e_next = Eb[(size_t)(t + 1) * lde_t];
        const double* p = row[(t - 1) & 1];
        if (on) {
            double best = p[j + 1] + w0;
            int code = 0;
            if (s > 0) {
                const double nx = p[j] + w1;
                if (nx > best) { best = nx; code = 1; }
            } else {
                const double* ex = p + S;                                  // ex[pp * S] = the last state of phone pp
                for (int pp = 0; pp < P; ++pp) {
                    const double v = ex[pp * S] + L[(size_t)pp * ldL];
                    if (v > best) { best = v; code = 2 + pp; }
                }
            }
            a = e + best;
            Pb[(size_t)t * ldp_t] = (uint8_t)code;
        }
        row[t & 1][j + 1] = a;
    }
    __syncthreads();
    if (j == 0) {
        const double* p = row[(T - 1) & 1];
        double best = alp_ninf();
        int best_j = -1;
        for (int pp = 0; pp < P; ++pp) {
            const double v = p[pp * S + S] + final_[pp];
            if (v > best) { best = v; best_j = pp * S + S - 1; }
        }
        end[b] = best_j;
        score[b] = best;
    }
}

extern "C" int fs2_align_max_loop_phones(void) { return ALP_MAX_PHONES; }

extern "C" int fs2_align_loop_viterbi(const double* E, long lde_b, long lde_t, const int32_t* lens, const double* self_,
                                      const double* next_, const double* link, long ldl, const double* init, const double* final_,
                                      uint8_t* bp, long ldp_b, long ldp_t, int32_t* end, double* score, int B, int Tmax, int P, int S,
                                      hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && self_ && next_ && link && init && final_ && bp && end && score, "align_loop_viterbi: null pointer");
    FS2_CHECK_ARG(P >= 1 && P <= ALP_MAX_PHONES, "align_loop_viterbi: %d phones, supported are 1..%d", P, ALP_MAX_PHONES);
    FS2_CHECK_ARG(S >= 1 && S <= 3, "align_loop_viterbi: %d states per phone, supported are 1..3", S);
    FS2_CHECK_ARG(P * S <= ALP_MAX_STATES, "align_loop_viterbi: %d states exceed the supported maximum of %d", P * S, ALP_MAX_STATES);
    const int C = P * S;
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && lde_t >= C && lde_b >= (long)Tmax * lde_t && ldp_t >= C && ldp_b >= (long)Tmax * ldp_t && ldl >= P,
                  "align_loop_viterbi: bad shape B=%d Tmax=%d C=%d lde_b=%ld lde_t=%ld ldp_b=%ld ldp_t=%ld ldl=%ld", B, Tmax, C, lde_b,
                  lde_t, ldp_b, ldp_t, ldl);
    if (B == 0) return FS2_OK;
    const int NT = C <= 256 ? 256 : (C <= 512 ? 512 : 1024);
    const size_t rows = 2 * (size_t)(NT + 1) * sizeof(double), table = (size_t)P * P * sizeof(double);
    const int link_lds = rows + table <= ALP_LDS_BYTES;
    const size_t dyn = link_lds ? table : 0;
#define ALP_VIT(N)                                                                                                                  \
    align_loop_viterbi_kernel<N><<<B, N, dyn, stream>>>(E, lde_b, lde_t, lens, self_, next_, link, ldl, init, final_, bp, ldp_b, ldp_t, \
                                                        end, score, Tmax, P, S, link_lds)
    if (NT == 256) ALP_VIT(256); else if (NT == 512) ALP_VIT(512); else ALP_VIT(1024);
#undef ALP_VIT
    FS2_CHECK_LAUNCH("align_loop_viterbi");
    return FS2_OK;
}

// One lane per utterance walks its backpointers twice from the end state: the first walk checks the chain and counts the
// segments (frame 0 and every frame entered with a code >= 2 start one), the second writes them from the last to the first, so
// they stand in time order.  A chain that leaves the table (a state outside [0, C), code 1 at a first state, an entry code at any
// other state or from a phone >= P) writes n_seg = -1 and no segment.
__global__ void align_loop_backtrack_kernel(const uint8_t* __restrict__ bp, long ldp_b, long ldp_t, const int32_t* __restrict__ lens,
                                            const int32_t* __restrict__ end, int32_t* __restrict__ seg_phone,
                                            int32_t* __restrict__ seg_start, long lds_b, int32_t* __restrict__ n_seg, int B, int Tmax,
                                            int P, int S) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int T = alp_len(lens, b, Tmax), C = P * S, j_end = end[b];
    if (T == 0 || j_end < 0) {
        n_seg[b] = 0;
        return;
    }
    if (j_end >= C) {
        n_seg[b] = -1;
        return;
    }
    const uint8_t* Pb = bp + (size_t)b * ldp_b;
    int n = 1, j = j_end;
    for (int t = T - 1; t > 0; --t) {
        const int code = Pb[(size_t)t * ldp_t + j], s = j % S;
        if (code == 1) {
            if (s == 0) { n = -1; break; }
            j -= 1;
        } else if (code >= 2) {
            if (s != 0 || code - 2 >= P) { n = -1; break; }
            j = (code - 2) * S + S - 1;
            ++n;
        }
    }
    n_seg[b] = n;
    if (n < 0) return;
    int32_t* ph = seg_phone + (size_t)b * lds_b;
    int32_t* st = seg_start + (size_t)b * lds_b;
    int k = n - 1;
    j = j_end;
    for (int t = T - 1; t > 0; --t) {
        const int code = Pb[(size_t)t * ldp_t + j];
        if (code == 1) {
            j -= 1;
        } else if (code >= 2) {
            ph[k] = j / S;
            st[k] = t;
            --k;
            j = (code - 2) * S + S - 1;
        }
    }
    ph[0] = j / S;
    st[0] = 0;
}

extern "C" int fs2_align_loop_backtrack(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* end,
                                        int32_t* seg_phone, int32_t* seg_start, long lds_b, int32_t* n_seg, int B, int Tmax, int P,
                                        int S, hipStream_t stream) {
    FS2_CHECK_ARG(bp && lens && end && seg_phone && seg_start && n_seg, "align_loop_backtrack: null pointer");
    FS2_CHECK_ARG(P >= 1 && P <= ALP_MAX_PHONES, "align_loop_backtrack: %d phones, supported are 1..%d", P, ALP_MAX_PHONES);
    FS2_CHECK_ARG(S >= 1 && S <= 3, "align_loop_backtrack: %d states per phone, supported are 1..3", S);
    FS2_CHECK_ARG(P * S <= ALP_MAX_STATES, "align_loop_backtrack: %d states exceed the supported maximum of %d", P * S, ALP_MAX_STATES);
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && ldp_t >= P * S && ldp_b >= (long)Tmax * ldp_t && lds_b >= Tmax,
                  "align_loop_backtrack: bad shape B=%d Tmax=%d C=%d ldp_b=%ld ldp_t=%ld lds_b=%ld", B, Tmax, P * S, ldp_b, ldp_t, lds_b);
    if (B == 0) return FS2_OK;
    align_loop_backtrack_kernel<<<fs2_cdiv(B, 64), 64, 0, stream>>>(bp, ldp_b, ldp_t, lens, end, seg_phone, seg_start, lds_b, n_seg, B,
                                                                   Tmax, P, S);
    FS2_CHECK_LAUNCH("align_loop_backtrack");
    return FS2_OK;
}
