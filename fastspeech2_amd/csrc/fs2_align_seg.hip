// fs2_align_seg.hip — segmental goodness of pronunciation: every block of the Viterbi path scored as a whole left-to-right HMM of
// every phone of the table (the "Segmental scores" paragraph of fastspeech2_amd/align.py; the numpy restatement is
// tests/align_seg_ref.py).
//
//   fs2_align_segment_scores  V[b][k][q] = the best score of phone q's S states over the frames [start, start + frames) of block k,
//                             every state occupied, the exit arc included; the candidate classes come through cand[b][k][q S + s]
//
// The one-kernel form.  One 256-lane workgroup per (utterance, block): after `triphones` the table row of a candidate column
// depends on the block, so a tile's frames belong to one block.  The candidate phones are walked in tiles of SG_PT(S) = 64 / S
// phones (64, 32, 21: at most SG_CT = 64 columns, a phone's states never straddle two tiles), the segment's frames in sub-tiles of
// SG_FT = 16.  For a (phone tile, frame sub-tile) the class scores F[16][64] are computed as fs2_align_score.hip computes them: the
// same preparation into the workspace (iv = 1 / var, k = log w - 1/2 sum_d log(2 pi var_d), once per call), the feature dimension
// staged SG_DC = 16 columns at a time into rows padded to 17 doubles, the same statements per (frame, class, component) in
// ascending d, the same fold over ascending m with a running maximum.  Lane (rg = tid & 15, fg = tid >> 4) owns frame fg and the
// columns rg + 16 k, k < 4: one feature value from LDS feeds 4 outputs.  The tile goes to LDS (rows of 80 doubles: the two frame
// rows a half-wave writes lie on disjoint banks), then lane p < SG_PT(S) advances the S <= 3 running values of its phone over the
// sub-tile's frames in ascending t and keeps them in registers across the sub-tiles; V is written once, after the last.  Every
// column goes through the same instructions whatever its phone, its tile or its lane, so two phones with identical table rows
// get bit-identical V.  No atomics; max is order-free and every sum ascends in t and d: two runs are bit-identical.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): LDS 31 360 B per workgroup (staging 19 584, the F tile 10 240, the
// tile's classes and arcs 1 280); 108 / 114 / 118 vector registers with M = 1 and S = 1 / 2 / 3, 122 / 126 / 128 with mixtures, 4 waves
// per SIMD in every variant, no scratch.  Nothing of this has been timed.  The tile sizes (16 frames, 64
// columns, one workgroup per block) are unmeasured choices: phone segments are short (5 to 20 frames at hop 256 / 22 050 Hz), which
// is why the frame tile is a quarter of fs2_align_frame_scores's; the table rows of a phone tile are staged again for every frame
// sub-tile of a long segment.
#include "fs2_common.h"

#define SG_FT 16                    // frames per sub-tile
#define SG_CT 64                    // candidate columns per tile
#define SG_DC 16                    // feature columns per staging step
#define SG_FLD 80                   // row length of the F tile in LDS
#define SG_MAX_MIX 8                // fs2_align_max_mixtures()
#define SG_MAX_PHONES 256           // fs2_align_max_seg_phones()
#define SG_MAX_SEG_STATES 3         // the graph's states per phone

static __device__ __forceinline__ double sg_ninf() { return -__builtin_huge_val(); }

// workspace: iv [R][D], then k [R], R = n_classes * M rows: the preparation step of fs2_align_score.hip, statement for statement
__global__ void seg_prep_kernel(const double* __restrict__ w, const double* __restrict__ var, int R, int D, double* __restrict__ iv,
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
    kk[r] = (wr == 0.0 ? sg_ninf() : log(wr)) + -0.5 * s;
}

template <bool MIX, int S>
__global__ void __launch_bounds__(256) align_segment_scores_kernel(const double* __restrict__ f, long ldf_b, long ldf_t,
                                                                   const int32_t* __restrict__ lens, const int32_t* __restrict__ seg,
                                                                   long lds_b, const int32_t* __restrict__ cand, long ldc_b, long ldc_k,
                                                                   const double* __restrict__ mu, const double* __restrict__ iv,
                                                                   const double* __restrict__ kk, const double* __restrict__ arc, int C,
                                                                   int M, int D, double* __restrict__ V, long ldv_b, long ldv_k, int Tmax,
                                                                   int P) {
    constexpr int PT = SG_CT / S;                                          // phones per tile
    __shared__ double xs[SG_FT][SG_DC + 1], ms[SG_CT][SG_DC + 1], vs[SG_CT][SG_DC + 1], Fs[SG_FT][SG_FLD], stay[SG_CT], leave[SG_CT];
    __shared__ int cl[SG_CT];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int T = min(max(lens[b], 0), Tmax);
    const int32_t* sg = seg + (size_t)b * lds_b + 2 * (size_t)k;
    const long a = sg[0], n = sg[1];
    if (n <= 0 || a < 0 || a + n > T) return;                              // an absent segment: nothing is written (uniform)
    const int32_t* cd = cand + (size_t)b * ldc_b + (size_t)k * ldc_k;
    const int PS = P * S;
    int absent = 0;
    for (int j = tid; j < PS; j += 256) absent |= cd[j] < 0;
    if (__syncthreads_or(absent)) return;                                  // a row holding -1 is absent (uniform)

    const int rg = tid & 15, fg = tid >> 4;
    const int sr = tid >> 4, sc = tid & 15;                                // staging: rows sr (+ 16 i), column sc
    const double* fb = f + (size_t)b * ldf_b;
    double* vo = V + (size_t)b * ldv_b + (size_t)k * ldv_k;

    for (int q0 = 0; q0 < P; q0 += PT) {
        __syncthreads();                                                   // the scan of the tile before is done with stay / leave / Fs
        if (tid < SG_CT) {
            const int col = q0 * S + tid;
            int c = (tid < PT * S && col < PS) ? cd[col] : -1;
            if (c >= C) c = -1;                                            // outside the table: the column scores -inf, nothing is read
            cl[tid] = c;
            stay[tid] = c >= 0 ? arc[2 * (size_t)c] : 0.0;
            leave[tid] = c >= 0 ? arc[2 * (size_t)c + 1] : 0.0;
        }
        double v[S];                                                       // the running values of phone q0 + tid (lanes tid < PT)
#pragma unroll
        for (int s = 0; s < S; ++s) v[s] = sg_ninf();

        for (long t0 = a; t0 < a + n; t0 += SG_FT) {
            double mx[4], sm[4], F[4];
            if constexpr (MIX) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    mx[j] = sg_ninf();
                    sm[j] = 0.0;
                }
            }
            for (int m = 0; m < M; ++m) {
                double acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = 0.0;
                for (int d0 = 0; d0 < D; d0 += SG_DC) {
                    __syncthreads();
                    const int d = d0 + sc;
                    const long t = t0 + sr;
                    xs[sr][sc] = (t < a + n && d < D) ? fb[(size_t)t * ldf_t + d] : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = sr + 16 * i;
                        const int c = cl[r];
                        double mm = 0.0, vv = 0.0;
                        if (c >= 0 && d < D) {
                            const size_t at = ((size_t)c * M + m) * D + d;
                            mm = mu[at];
                            vv = iv[at];
                        }
                        ms[r][sc] = mm;
                        vs[r][sc] = vv;
                    }
                    __syncthreads();
#pragma unroll 4
                    for (int dd = 0; dd < SG_DC; ++dd) {
                        const double xv = xs[fg][dd];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double mm = ms[rg + 16 * j][dd], vv = vs[rg + 16 * j][dd];
                            const double df = xv - mm;
                            acc[j] += df * df * vv;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = cl[rg + 16 * j];
                    const double kc = c >= 0 ? kk[(size_t)c * M + m] : sg_ninf();
                    const double nn = kc + -0.5 * acc[j];
                    if constexpr (MIX) {
                        if (nn != sg_ninf()) {                             // a component of weight 0 contributes nothing
                            const double hi = fmax(mx[j], nn), lo = fmin(mx[j], nn);
                            const double e = exp(lo - hi);                 // exp(-inf) = 0 at the first component
                            sm[j] = nn > mx[j] ? sm[j] * e + 1.0 : sm[j] + e;
                            mx[j] = hi;
                        }
                    } else {
                        F[j] = nn;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (MIX) F[j] = mx[j] == sg_ninf() ? mx[j] : mx[j] + log(sm[j]);
                Fs[fg][rg + 16 * j] = F[j];
            }
            __syncthreads();
            if (tid < PT && q0 + tid < P) {                                // one lane per candidate phone, ascending t
                const int cnt = (int)min((long)SG_FT, a + n - t0);
                for (int i = 0; i < cnt; ++i) {
                    if (t0 + i == a) {
                        v[0] = Fs[i][tid * S];
                    } else {
#pragma unroll
                        for (int s = S - 1; s > 0; --s)
                            v[s] = Fs[i][tid * S + s] + fmax(v[s] + stay[tid * S + s], v[s - 1] + leave[tid * S + s - 1]);
                        v[0] = Fs[i][tid * S] + (v[0] + stay[tid * S]);
                    }
                }
            }
        }
        if (tid < PT && q0 + tid < P) vo[q0 + tid] = n < S ? sg_ninf() : v[S - 1] + leave[tid * S + S - 1];
    }
}

static bool sg_rows_ok(int n_classes, int M, int D) {
    return n_classes > 0 && M >= 1 && M <= SG_MAX_MIX && D > 0 && (long)n_classes * M * ((long)D + 1) < (1L << 31);
}
extern "C" int fs2_align_max_seg_phones(void) { return SG_MAX_PHONES; }
extern "C" int fs2_align_segment_scores_ws(int n_classes, int M, int D) {
    return sg_rows_ok(n_classes, M, D) ? (int)((long)n_classes * M * ((long)D + 1)) : 0;
}

template <bool MIX>
static void sg_launch(int S, dim3 grid, hipStream_t stream, const double* f, long ldf_b, long ldf_t, const int32_t* lens,
                      const int32_t* seg, long lds_b, const int32_t* cand, long ldc_b, long ldc_k, const double* mu, const double* iv,
                      const double* kk, const double* arc, int C, int M, int D, double* V, long ldv_b, long ldv_k, int Tmax, int P) {
#define SG_GO(S_)                                                                                                                     \
    align_segment_scores_kernel<MIX, S_><<<grid, 256, 0, stream>>>(f, ldf_b, ldf_t, lens, seg, lds_b, cand, ldc_b, ldc_k, mu, iv, kk, arc, \
                                                                   C, M, D, V, ldv_b, ldv_k, Tmax, P)
    if (S == 1) SG_GO(1);
    else if (S == 2) SG_GO(2);
    else SG_GO(3);
#undef SG_GO
}

extern "C" int fs2_align_segment_scores(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const int32_t* seg, long lds_b,
                                        const int32_t* cand, long ldc_b, long ldc_k, const double* w, const double* mu, const double* var,
                                        int n_classes, int M, int D, const double* arc, double* ws, long ws_doubles, double* V, long ldv_b,
                                        long ldv_k, int B, int Tmax, int Kmax, int P, int S, hipStream_t stream) {
    FS2_CHECK_ARG(f && lens && seg && cand && w && mu && var && arc && ws && V, "align_segment_scores: null pointer");
    FS2_CHECK_ARG(M >= 1 && M <= SG_MAX_MIX, "align_segment_scores: %d mixture components, supported are 1..%d", M, SG_MAX_MIX);
    FS2_CHECK_ARG(sg_rows_ok(n_classes, M, D), "align_segment_scores: bad tables classes=%d M=%d D=%d", n_classes, M, D);
    FS2_CHECK_ARG(P >= 1 && P <= SG_MAX_PHONES, "align_segment_scores: %d candidate phones, supported are 1..%d", P, SG_MAX_PHONES);
    FS2_CHECK_ARG(S >= 1 && S <= SG_MAX_SEG_STATES, "align_segment_scores: %d states per phone, supported are 1..%d", S, SG_MAX_SEG_STATES);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Kmax >= 0 && ldf_t >= D && ldf_b >= (long)Tmax * ldf_t && lds_b >= 2L * Kmax &&
                      ldc_k >= (long)P * S && ldc_b >= (long)Kmax * ldc_k && ldv_k >= P && ldv_b >= (long)Kmax * ldv_k,
                  "align_segment_scores: bad shape B=%d Tmax=%d Kmax=%d D=%d P=%d S=%d ldf_b=%ld ldf_t=%ld lds_b=%ld ldc_b=%ld ldc_k=%ld "
                  "ldv_b=%ld ldv_k=%ld",
                  B, Tmax, Kmax, D, P, S, ldf_b, ldf_t, lds_b, ldc_b, ldc_k, ldv_b, ldv_k);
    FS2_CHECK_ARG(ws_doubles >= fs2_align_segment_scores_ws(n_classes, M, D), "align_segment_scores: workspace of %ld doubles, %d needed",
                  ws_doubles, fs2_align_segment_scores_ws(n_classes, M, D));
    if (B == 0 || Tmax == 0 || Kmax == 0) return FS2_OK;
    const int R = n_classes * M;
    double* iv = ws;
    double* kk = ws + (size_t)R * D;
    seg_prep_kernel<<<fs2_cdiv(R, 64), 64, 0, stream>>>(w, var, R, D, iv, kk);
    const dim3 grid(Kmax, B);
    if (M == 1)
        sg_launch<false>(S, grid, stream, f, ldf_b, ldf_t, lens, seg, lds_b, cand, ldc_b, ldc_k, mu, iv, kk, arc, n_classes, M, D, V, ldv_b,
                         ldv_k, Tmax, P);
    else
        sg_launch<true>(S, grid, stream, f, ldf_b, ldf_t, lens, seg, lds_b, cand, ldc_b, ldc_k, mu, iv, kk, arc, n_classes, M, D, V, ldv_b,
                        ldv_k, Tmax, P);
    FS2_CHECK_LAUNCH("align_segment_scores");
    return FS2_OK;
}
