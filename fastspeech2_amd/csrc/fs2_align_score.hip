// fs2_align_score.hip — alignment confidence: the Viterbi path as per-frame states and classes, and every frame scored against
// every class of the model with the maximum taken on the chip (the "Confidence" paragraph of fastspeech2_amd/align.py; the numpy
// restatement is tests/align_score_ref.py).
//
//   fs2_align_path          backpointers -> state[b][t], cls[b][t] = sid[b][state]: the walk of fs2_align_backtrack, one lane per
//                           utterance; frames a broken chain does not reach get -1
//   fs2_align_frame_scores  F[t][c] for all C classes of the tables, never stored: own[t] = F[t][cls[t]], best[t] = max_c F[t][c],
//                           arg[t] = the lowest c that attains it
//
// The hot kernel.  F is the direct form sum_d (x_d - mu_d)^2 * (1 / var_d): not bilinear, so it runs on the fp64 vector ALU.  A
// 256-lane workgroup owns SC_FT = 64 frames and walks all classes in tiles of SC_CT = 64; lane (rg = tid & 15, fg = tid >> 4) owns
// the 4 x 4 outputs of frames fg + 16 i and classes c0 + rg + 16 k, so one feature value read from LDS feeds 4 and one table pair
// (mu, 1 / var) feeds 4 frames: 8 LDS reads per 16 outputs x 3 operations.  The feature dimension is staged SC_DC = 16 columns at a
// time, rows padded to 17 doubles: the 16 class rows a half-wave reads lie on 16 different bank pairs (34 rg mod 64), the two
// frame rows are broadcasts.  LDS: 3 x 64 x 17 x 8 B = 26 112 B per workgroup.  A lane keeps 16 accumulators and, with mixtures,
// 16 running (maximum, sum) pairs: 162 vector registers with M = 1 (3 waves per SIMD), 254 with mixtures (2 waves per SIMD), no
// scratch, which is why the frame tile stops at 64.
//
// What does not depend on the frame is computed once per call by score_prep_kernel into the workspace: iv = 1 / var and, per
// component, k = log w - 1/2 sum_d log(2 pi var_d) (d ascending).  So N[t][c][m] = k - 1/2 sum_d (x_d - mu_d)^2 iv_d, d ascending.
// Mixtures: a class's components are folded in ascending m with a running maximum, F = mx + log(sum_m exp(N_m - mx)); a component
// of weight 0 has k = -inf and is skipped; with M = 1 and w = 1, F = N.  Every class goes through the same instructions whatever
// its index or its place in a tile, so equal table rows give equal bits; a lane meets its classes in ascending order and replaces
// its maximum only by a strictly larger value, and the 16 lanes of a frame are combined by (larger value, then lower index): the
// lowest class wins ties.  own is the F of the one lane whose class is cls[t], taken from the same register as the maximum: own <=
// best always, own == best bit for bit where arg == cls.  No atomics.
#include "fs2_common.h"

#define SC_FT 64                    // frames per workgroup
#define SC_CT 64                    // classes per tile
#define SC_DC 16                    // feature columns per staging step
#define SC_MAX_MIX 8                // fs2_align_max_mixtures()
#define SC_MAX_STATES 1024          // fs2_align_max_states()

static __device__ __forceinline__ int sc_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }
static __device__ __forceinline__ double sc_ninf() { return -__builtin_huge_val(); }

// ------------------------------------------------------------------ path
__global__ void align_path_kernel(const uint8_t* __restrict__ bp, long ldp_b, long ldp_t, const int32_t* __restrict__ lens,
                                  const int32_t* __restrict__ jlens, const int32_t* __restrict__ skip, const int32_t* __restrict__ sid,
                                  long ldg, const int32_t* __restrict__ end, int32_t* __restrict__ state, long lds_b,
                                  int32_t* __restrict__ cls, long ldc_b, int B, int Tmax, int Jmax) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int T = sc_len(lens, b, Tmax), J = sc_len(jlens, b, Jmax);
    int32_t* st = state + (size_t)b * lds_b;
    int32_t* cl = cls + (size_t)b * ldc_b;
    const uint8_t* P = bp + (size_t)b * ldp_b;
    const int32_t* sk = skip + (size_t)b * ldg;
    const int32_t* sd = sid + (size_t)b * ldg;
    int j = end[b];
    if (j < 0 || j >= J) j = -1;
    for (int t = T - 1; t >= 0; --t) {
        st[t] = j;
        cl[t] = j >= 0 ? sd[j] : -1;
        if (t > 0 && j >= 0) {
            const int code = P[(size_t)t * ldp_t + j];
            const int nj = code == 0 ? j : (code == 1 ? j - 1 : sk[j]);
            j = (nj < 0 || nj >= J) ? -1 : nj;                             // not a path of this graph: the rest stays -1
        }
    }
}
extern "C" int fs2_align_path(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* jlens, const int32_t* skip,
                              const int32_t* sid, long ldg, const int32_t* end, int32_t* state, long lds_b, int32_t* cls, long ldc_b,
                              int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(bp && lens && jlens && skip && sid && end && state && cls, "align_path: null pointer");
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && Jmax >= 0 && ldp_t >= Jmax && ldp_b >= (long)Tmax * ldp_t && ldg >= Jmax && lds_b >= Tmax &&
                      ldc_b >= Tmax,
                  "align_path: bad shape B=%d Tmax=%d Jmax=%d ldp_b=%ld ldp_t=%ld ldg=%ld lds_b=%ld ldc_b=%ld", B, Tmax, Jmax, ldp_b, ldp_t,
                  ldg, lds_b, ldc_b);
    FS2_CHECK_ARG(Jmax <= SC_MAX_STATES, "align_path: %d states exceed the supported maximum of %d", Jmax, SC_MAX_STATES);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_path_kernel<<<fs2_cdiv(B, 64), 64, 0, stream>>>(bp, ldp_b, ldp_t, lens, jlens, skip, sid, ldg, end, state, lds_b, cls, ldc_b, B,
                                                          Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_path");
    return FS2_OK;
}

// ------------------------------------------------------------------ frame scores
// workspace: iv [R][D], then k [R], R = n_classes * M rows
__global__ void score_prep_kernel(const double* __restrict__ w, const double* __restrict__ var, int R, int D, double* __restrict__ iv,
                                  double* __restrict__ kk) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const double* v = var + (size_t)r * D;
    double* o = iv + (size_t)r * D;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const double x = v[d];
        o[d] = 1.0 / x;
        s += log(6.283185307179586476925286766559 * x);
    }
    const double wr = w[r];
    kk[r] = (wr == 0.0 ? sc_ninf() : log(wr)) + -0.5 * s;
}

template <bool MIX>
__global__ void __launch_bounds__(256) align_frame_scores_kernel(const double* __restrict__ f, long ldf_b, long ldf_t,
                                                                 const int32_t* __restrict__ lens, const int32_t* __restrict__ cls,
                                                                 long ldc_b, const double* __restrict__ mu,
                                                                 const double* __restrict__ iv, const double* __restrict__ kk, int C,
                                                                 int M, int D, double* __restrict__ own, long ldo_b,
                                                                 double* __restrict__ best, long ldb_b, int32_t* __restrict__ arg,
                                                                 long lda_b, int Tmax) {
    __shared__ double xs[SC_FT][SC_DC + 1], ms[SC_CT][SC_DC + 1], vs[SC_CT][SC_DC + 1];
    const int b = blockIdx.y, T = sc_len(lens, b, Tmax);
    const long t0 = (long)blockIdx.x * SC_FT;
    if (t0 >= T) return;
    const int tid = threadIdx.x, rg = tid & 15, fg = tid >> 4;
    const int sr = tid >> 4, sc = tid & 15;                                // staging: rows sr + 16 i, column sc
    const double* fb = f + (size_t)b * ldf_b;

    int want[4];                                                           // the path's class of this lane's frames
    double bst[4], mine[4];
    int ag[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long t = t0 + fg + 16 * i;
        want[i] = t < T ? cls[(size_t)b * ldc_b + t] : -1;
        bst[i] = sc_ninf();
        mine[i] = __builtin_nan("");
        ag[i] = 0x7fffffff;
    }

    for (int c0 = 0; c0 < C; c0 += SC_CT) {
        double mx[4][4], sm[4][4], F[4][4];
        if constexpr (MIX) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    mx[i][k] = sc_ninf();
                    sm[i][k] = 0.0;
                }
        }
        for (int m = 0; m < M; ++m) {
            double acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[i][k] = 0.0;
            for (int d0 = 0; d0 < D; d0 += SC_DC) {
                __syncthreads();
                const int d = d0 + sc;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = sr + 16 * i;
                    const long t = t0 + r;
                    xs[r][sc] = (t < T && d < D) ? fb[(size_t)t * ldf_t + d] : 0.0;
                    const int c = c0 + r;
                    double mm = 0.0, vv = 0.0;
                    if (c < C && d < D) {
                        const size_t at = ((size_t)c * M + m) * D + d;
                        mm = mu[at];
                        vv = iv[at];
                    }
                    ms[r][sc] = mm;
                    vs[r][sc] = vv;
                }
                __syncthreads();
#pragma unroll 4
                for (int dd = 0; dd < SC_DC; ++dd) {
                    double xv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) xv[i] = xs[fg + 16 * i][dd];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double mm = ms[rg + 16 * k][dd], vv = vs[rg + 16 * k][dd];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const double df = xv[i] - mm;
                            acc[i][k] += df * df * vv;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + rg + 16 * k;
                const double kc = c < C ? kk[(size_t)c * M + m] : sc_ninf();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double n = kc + -0.5 * acc[i][k];
                    if constexpr (MIX) {
                        if (n != sc_ninf()) {                              // a component of weight 0 contributes nothing
                            const double hi = fmax(mx[i][k], n), lo = fmin(mx[i][k], n);
                            const double e = exp(lo - hi);                 // exp(-inf) = 0 at the first component
                            sm[i][k] = n > mx[i][k] ? sm[i][k] * e + 1.0 : sm[i][k] + e;
                            mx[i][k] = hi;
                        }
                    } else {
                        F[i][k] = n;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // ascending classes: only a strictly larger value replaces
            const int c = c0 + rg + 16 * k;
            if (c >= C) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (MIX) F[i][k] = mx[i][k] == sc_ninf() ? mx[i][k] : mx[i][k] + log(sm[i][k]);
                if (F[i][k] > bst[i]) {
                    bst[i] = F[i][k];
                    ag[i] = c;
                }
                if (c == want[i]) mine[i] = F[i][k];
            }
        }
    }
    // the 16 lanes of a frame (consecutive lanes of one wave): larger value, then lower class; own from the one lane that has it
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const double b2 = __shfl_xor(bst[i], o, 64), m2 = __shfl_xor(mine[i], o, 64);
            const int a2 = __shfl_xor(ag[i], o, 64);
            if (b2 > bst[i] || (b2 == bst[i] && a2 < ag[i])) {
                bst[i] = b2;
                ag[i] = a2;
            }
            if (mine[i] != mine[i]) mine[i] = m2;
        }
        const long t = t0 + fg + 16 * i;
        if (rg == 0 && t < T) {
            own[(size_t)b * ldo_b + t] = mine[i];
            best[(size_t)b * ldb_b + t] = bst[i];
            arg[(size_t)b * lda_b + t] = ag[i] == 0x7fffffff ? 0 : ag[i];
        }
    }
}

static bool sc_rows_ok(int n_classes, int M, int D) {
    return n_classes > 0 && M >= 1 && M <= SC_MAX_MIX && D > 0 && (long)n_classes * M * ((long)D + 1) < (1L << 31);
}
extern "C" int fs2_align_frame_scores_ws(int n_classes, int M, int D) {
    return sc_rows_ok(n_classes, M, D) ? (int)((long)n_classes * M * ((long)D + 1)) : 0;
}

extern "C" int fs2_align_frame_scores(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const int32_t* cls, long ldc_b,
                                      const double* w, const double* mu, const double* var, int n_classes, int M, int D, double* ws,
                                      long ws_doubles, double* own, long ldo_b, double* best, long ldb_b, int32_t* arg, long lda_b, int B,
                                      int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(f && lens && cls && w && mu && var && ws && own && best && arg, "align_frame_scores: null pointer");
    FS2_CHECK_ARG(M >= 1 && M <= SC_MAX_MIX, "align_frame_scores: %d mixture components, supported are 1..%d", M, SC_MAX_MIX);
    FS2_CHECK_ARG(sc_rows_ok(n_classes, M, D), "align_frame_scores: bad tables classes=%d M=%d D=%d", n_classes, M, D);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && ldf_t >= D && ldf_b >= (long)Tmax * ldf_t && ldc_b >= Tmax && ldo_b >= Tmax &&
                      ldb_b >= Tmax && lda_b >= Tmax,
                  "align_frame_scores: bad shape B=%d Tmax=%d D=%d ldf_b=%ld ldf_t=%ld ldc_b=%ld ldo_b=%ld ldb_b=%ld lda_b=%ld", B, Tmax, D,
                  ldf_b, ldf_t, ldc_b, ldo_b, ldb_b, lda_b);
    FS2_CHECK_ARG(ws_doubles >= fs2_align_frame_scores_ws(n_classes, M, D), "align_frame_scores: workspace of %ld doubles, %d needed",
                  ws_doubles, fs2_align_frame_scores_ws(n_classes, M, D));
    if (B == 0 || Tmax == 0) return FS2_OK;
    const int R = n_classes * M;
    double* iv = ws;
    double* kk = ws + (size_t)R * D;
    score_prep_kernel<<<fs2_cdiv(R, 64), 64, 0, stream>>>(w, var, R, D, iv, kk);
    const dim3 grid(fs2_cdiv(Tmax, SC_FT), B);
    if (M == 1)
        align_frame_scores_kernel<false><<<grid, 256, 0, stream>>>(f, ldf_b, ldf_t, lens, cls, ldc_b, mu, iv, kk, n_classes, M, D, own, ldo_b,
                                                                    best, ldb_b, arg, lda_b, Tmax);
    else
        align_frame_scores_kernel<true><<<grid, 256, 0, stream>>>(f, ldf_b, ldf_t, lens, cls, ldc_b, mu, iv, kk, n_classes, M, D, own, ldo_b,
                                                                   best, ldb_b, arg, lda_b, Tmax);
    FS2_CHECK_LAUNCH("align_frame_scores");
    return FS2_OK;
}
