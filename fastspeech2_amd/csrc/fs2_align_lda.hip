// fs2_align_lda.hip — the forced aligner's LDA stage: spliced frames, their first and second moments over the corpus, and the
// projection of every frame, in fp64 on ragged batches.  The specification is the "LDA" paragraph of fastspeech2_amd/align.py's
// docstring (mirrored in DESIGN.md); tests/align_lda_ref.py restates it in numpy.
//
// Shapes.  Utterance b has T = lens[b] frames; x, y and z are [B][Tmax][.] with explicit batch and frame strides.  Nothing at
// t >= T is read (the tests poison it with NaN) and nothing there is written.  D_s = n_mel (2 c + 1) <= 720.
//
//   fs2_align_splice     y[b][t][(p + c) n_mel + m] = x[b][clamp(t + p, 0, T - 1)][m], one lane per element
//   fs2_align_scatter    s += sum y, S += sum y y^T over the valid frames.  The padded rows r = b Tmax + t are cut into at most 32
//                        chunks of equal length (a multiple of 16), a function of (B, Tmax) alone.  One workgroup per (64 x 64
//                        tile of the lower triangle, chunk): four waves, each a 32 x 32 quarter as 2 x 2 v_mfma_f64_16x16x4_f64
//                        accumulators, 16 frames staged in LDS at a time ([frame][dimension], rows padded to 80 doubles so that
//                        the two frame rows a half-wave reads fall on disjoint banks), frames in ascending order.  Partial tiles
//                        go to the caller's workspace; a second kernel adds them in ascending chunk order, adds the total to the
//                        caller's table and writes each value to (i, j) and (j, i): S is exactly symmetric, no atomics anywhere.
//   fs2_align_project    z[b][t][q] = sum_d P[q][d] y[b][t][d] - o[q]: 64 frames x 64 outputs per workgroup with the same wave
//                        layout, 16 dimensions of y and of P staged at a time ([row][dimension], rows padded to 17 doubles)
#include "fs2_common.h"

#define LDA_MAX_DIM 720             // D_s: 80 mel channels, c = 4
#define LDA_MAX_CONTEXT 4
#define LDA_TILE 64
#define LDA_SLAB 16
#define LDA_LD 80                   // LDS row of the scatter slabs, doubles
#define LDA_MAX_CHUNKS 32

typedef double lda_f64x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ int lda_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }

// ------------------------------------------------------------------ splice
__global__ void align_splice_kernel(const double* __restrict__ x, long ldx_b, long ldx_t, const int32_t* __restrict__ lens, int n_mel,
                                    int c, double* __restrict__ y, long ldy_b, long ldy_t, int Tmax) {
    const int b = blockIdx.y, T = lda_len(lens, b, Tmax), Ds = n_mel * (2 * c + 1);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * Ds) return;
    const int t = (int)(i / Ds), d = (int)(i - (long)t * Ds);
    const int q = d / n_mel, m = d - q * n_mel;
    const int ts = min(max(t + q - c, 0), T - 1);
    y[(size_t)b * ldy_b + (size_t)t * ldy_t + d] = x[(size_t)b * ldx_b + (size_t)ts * ldx_t + m];
}
extern "C" int fs2_align_max_splice_dim(void) { return LDA_MAX_DIM; }

extern "C" int fs2_align_splice(const double* x, long ldx_b, long ldx_t, const int32_t* lens, int n_mel, int c, double* y, long ldy_b,
                                long ldy_t, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && y, "align_splice: null pointer");
    FS2_CHECK_ARG(c >= 0 && c <= LDA_MAX_CONTEXT, "align_splice: context %d, supported are 0..%d", c, LDA_MAX_CONTEXT);
    FS2_CHECK_ARG(n_mel > 0 && (long)n_mel * (2 * c + 1) <= LDA_MAX_DIM, "align_splice: %d channels x %d frames exceed the supported %d",
                  n_mel, 2 * c + 1, LDA_MAX_DIM);
    const int Ds = n_mel * (2 * c + 1);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && ldx_t >= n_mel && ldx_b >= (long)Tmax * ldx_t && ldy_t >= Ds &&
                      ldy_b >= (long)Tmax * ldy_t && (long)Tmax * Ds < (1L << 31) * 256,
                  "align_splice: bad shape B=%d Tmax=%d n_mel=%d ldx_b=%ld ldx_t=%ld ldy_b=%ld ldy_t=%ld", B, Tmax, n_mel, ldx_b, ldx_t,
                  ldy_b, ldy_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_splice_kernel<<<dim3(fs2_cdiv((long)Tmax * Ds, 256), B), 256, 0, stream>>>(x, ldx_b, ldx_t, lens, n_mel, c, y, ldy_b, ldy_t,
                                                                                    Tmax);
    FS2_CHECK_LAUNCH("align_splice");
    return FS2_OK;
}

// ------------------------------------------------------------------ scatter
// The chunk split: rows per chunk = ceil(R / 32) rounded up to a multiple of 16, R = B Tmax padded rows.
static void lda_plan(long R, long* rows_per, int* n_chunks) {
    long rp = (R + LDA_MAX_CHUNKS - 1) / LDA_MAX_CHUNKS;
    rp = (rp + LDA_SLAB - 1) / LDA_SLAB * LDA_SLAB;
    if (rp < LDA_SLAB) rp = LDA_SLAB;
    *rows_per = rp;
    *n_chunks = (int)((R + rp - 1) / rp);
}
static long lda_chunk_doubles(int Ds) {
    const long nt = (Ds + LDA_TILE - 1) / LDA_TILE;
    return nt * (nt + 1) / 2 * LDA_TILE * LDA_TILE + nt * LDA_TILE;
}

// Workspace of chunk ch: ntri tiles [64][64] (tile p = I (I + 1) / 2 + J, J <= I, rows are dimensions of block I), then nt x 64 sums.
// Lane map of v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[i = (lane >> 4) + 4 reg][j =
// lane & 15].  Here k is the frame and both operands are read from [frame][dimension] slabs.
__global__ void __launch_bounds__(256) align_scatter_kernel(const double* __restrict__ y, long ldy_b, long ldy_t,
                                                            const int32_t* __restrict__ lens, int Ds, double* __restrict__ ws,
                                                            long chunk_doubles, int ntri, long rows_per, long R, int Tmax) {
    __shared__ double ya[LDA_SLAB][LDA_LD], yb[LDA_SLAB][LDA_LD];
    const int p = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= p) ++I;
    const int J = p - I * (I + 1) / 2;
    const long r_begin = (long)ch * rows_per, r_end = min(R, r_begin + rows_per);
    const int lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int rr = tid >> 4, cc = (tid & 15) * 4;                          // staging: row rr of the slab, four dimensions from cc
    lda_f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (lda_f64x4){0.0, 0.0, 0.0, 0.0};
    double ssum = 0.0;
    for (long r0 = r_begin; r0 < r_end; r0 += LDA_SLAB) {
        const long r = r0 + rr;
        bool ok = r < r_end;
        const double* src = y;
        if (ok) {
            const int b = (int)(r / Tmax), t = (int)(r - (long)b * Tmax);
            ok = t < lda_len(lens, b, Tmax);
            src = y + (size_t)b * ldy_b + (size_t)t * ldy_t;
        }
        double va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int da = I * LDA_TILE + cc + q, db = J * LDA_TILE + cc + q;
            va[q] = (ok && da < Ds) ? src[da] : 0.0;
            vb[q] = (ok && db < Ds) ? src[db] : 0.0;
        }
        __syncthreads();                                                   // the previous slab has been consumed
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ya[rr][cc + q] = va[q];
            yb[rr][cc + q] = vb[q];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < LDA_SLAB / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            const double a0 = ya[kk][wi * 32 + (lane & 15)], a1 = ya[kk][wi * 32 + 16 + (lane & 15)];
            const double b0 = yb[kk][wj * 32 + (lane & 15)], b1 = yb[kk][wj * 32 + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (J == 0 && tid < LDA_TILE) {
#pragma unroll
            for (int k = 0; k < LDA_SLAB; ++k) ssum += ya[k][tid];
        }
    }
    double* out = ws + (size_t)ch * chunk_doubles;
    double* tile = out + (size_t)p * LDA_TILE * LDA_TILE;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = wi * 32 + m * 16 + (lane >> 4) + 4 * reg, j = wj * 32 + n * 16 + (lane & 15);
                tile[i * LDA_TILE + j] = acc[m][n][reg];
            }
    if (J == 0 && tid < LDA_TILE) out[(size_t)ntri * LDA_TILE * LDA_TILE + I * LDA_TILE + tid] = ssum;
}

// The partial tiles of every chunk, in ascending chunk order, then onto the caller's table; (i, j) and (j, i) get the same value.
__global__ void __launch_bounds__(256) align_scatter_finish_kernel(const double* __restrict__ ws, long chunk_doubles, int n_chunks,
                                                                   int ntri, int Ds, double* __restrict__ s, double* __restrict__ S,
                                                                   long lds) {
    const int p = blockIdx.x, tid = threadIdx.x;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= p) ++I;
    const int J = p - I * (I + 1) / 2;
    const double* tile = ws + (size_t)p * LDA_TILE * LDA_TILE;
    for (int e = tid; e < LDA_TILE * LDA_TILE; e += 256) {
        const int gi = I * LDA_TILE + (e >> 6), gj = J * LDA_TILE + (e & 63);
        if (gi >= Ds || gj > gi) continue;
        double tot = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) tot += tile[(size_t)ch * chunk_doubles + e];
        const double v = S[(size_t)gi * lds + gj] + tot;
        S[(size_t)gi * lds + gj] = v;
        S[(size_t)gj * lds + gi] = v;
    }
    if (J == 0 && tid < LDA_TILE && I * LDA_TILE + tid < Ds) {
        const double* part = ws + (size_t)ntri * LDA_TILE * LDA_TILE + I * LDA_TILE + tid;
        double tot = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) tot += part[(size_t)ch * chunk_doubles];
        s[I * LDA_TILE + tid] += tot;
    }
}

extern "C" int fs2_align_scatter_ws(int B, int Tmax, int Ds) {
    if (B <= 0 || Tmax <= 0 || Ds <= 0 || Ds > LDA_MAX_DIM) return 0;
    long rows_per;
    int n_chunks;
    lda_plan((long)B * Tmax, &rows_per, &n_chunks);
    return (int)(n_chunks * lda_chunk_doubles(Ds));
}

extern "C" int fs2_align_scatter(const double* y, long ldy_b, long ldy_t, const int32_t* lens, int Ds, double* s, double* S, long lds,
                                 double* ws, long ws_doubles, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(y && lens && s && S, "align_scatter: null pointer");
    FS2_CHECK_ARG(Ds >= 1 && Ds <= LDA_MAX_DIM, "align_scatter: %d dimensions, supported are 1..%d", Ds, LDA_MAX_DIM);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && ldy_t >= Ds && ldy_b >= (long)Tmax * ldy_t && lds >= Ds,
                  "align_scatter: bad shape B=%d Tmax=%d Ds=%d ldy_b=%ld ldy_t=%ld lds=%ld", B, Tmax, Ds, ldy_b, ldy_t, lds);
    if (B == 0 || Tmax == 0) return FS2_OK;
    long rows_per;
    int n_chunks;
    lda_plan((long)B * Tmax, &rows_per, &n_chunks);
    const long chunk = lda_chunk_doubles(Ds);
    FS2_CHECK_ARG(ws && ws_doubles >= n_chunks * chunk, "align_scatter: workspace of %ld doubles, %ld needed (fs2_align_scatter_ws)",
                  ws_doubles, n_chunks * chunk);
    const int nt = fs2_cdiv(Ds, LDA_TILE), ntri = nt * (nt + 1) / 2;
    align_scatter_kernel<<<dim3(ntri, n_chunks), 256, 0, stream>>>(y, ldy_b, ldy_t, lens, Ds, ws, chunk, ntri, rows_per, (long)B * Tmax,
                                                                   Tmax);
    FS2_CHECK_LAUNCH("align_scatter");
    align_scatter_finish_kernel<<<ntri, 256, 0, stream>>>(ws, chunk, n_chunks, ntri, Ds, s, S, lds);
    FS2_CHECK_LAUNCH("align_scatter (finish)");
    return FS2_OK;
}

// ------------------------------------------------------------------ project
// A[i = frame][k = dimension] = y, B[k = dimension][j = output] = P[j][k]: both operands are contiguous in k in memory and are staged
// as [row][16 dimensions]; the sum over d ascends in steps of four (the instruction's k), o is subtracted at the end.
__global__ void __launch_bounds__(256) align_project_kernel(const double* __restrict__ y, long ldy_b, long ldy_t,
                                                            const int32_t* __restrict__ lens, const double* __restrict__ P,
                                                            const double* __restrict__ o, int K, int Ds, double* __restrict__ z,
                                                            long ldz_b, long ldz_t, int Tmax) {
    __shared__ double ys[LDA_TILE][LDA_SLAB + 1], ps[LDA_TILE][LDA_SLAB + 1];
    const int b = blockIdx.z, T = lda_len(lens, b, Tmax);
    const int t0 = blockIdx.y * LDA_TILE, n0 = blockIdx.x * LDA_TILE, tid = threadIdx.x;
    if (t0 >= T) return;
    const int lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int rr = tid >> 2, cc = (tid & 3) * 4;                           // staging: row rr, four dimensions from cc
    const bool y_ok = t0 + rr < T, p_ok = n0 + rr < K;
    const double* ysrc = y + (size_t)b * ldy_b + (size_t)(y_ok ? t0 + rr : 0) * ldy_t;
    const double* psrc = P + (size_t)(p_ok ? n0 + rr : 0) * Ds;
    lda_f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (lda_f64x4){0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < Ds; d0 += LDA_SLAB) {
        double va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = d0 + cc + q;
            va[q] = (y_ok && d < Ds) ? ysrc[d] : 0.0;
            vb[q] = (p_ok && d < Ds) ? psrc[d] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ys[rr][cc + q] = va[q];
            ps[rr][cc + q] = vb[q];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < LDA_SLAB / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            const double a0 = ys[wi * 32 + (lane & 15)][kk], a1 = ys[wi * 32 + 16 + (lane & 15)][kk];
            const double b0 = ps[wj * 32 + (lane & 15)][kk], b1 = ps[wj * 32 + 16 + (lane & 15)][kk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* zb = z + (size_t)b * ldz_b;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int q = n0 + wj * 32 + n * 16 + (lane & 15);
            if (q >= K) continue;
            const double off = o[q];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int t = t0 + wi * 32 + m * 16 + (lane >> 4) + 4 * reg;
                if (t < T) zb[(size_t)t * ldz_t + q] = acc[m][n][reg] - off;
            }
        }
}
extern "C" int fs2_align_project(const double* y, long ldy_b, long ldy_t, const int32_t* lens, const double* P, const double* o, int K,
                                 int Ds, double* z, long ldz_b, long ldz_t, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(y && lens && P && o && z, "align_project: null pointer");
    FS2_CHECK_ARG(Ds >= 1 && Ds <= LDA_MAX_DIM && K >= 1 && K <= Ds, "align_project: %d outputs of %d dimensions, supported are 1 <= k <= D_s <= %d",
                  K, Ds, LDA_MAX_DIM);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Tmax <= 65535 * LDA_TILE && ldy_t >= Ds && ldy_b >= (long)Tmax * ldy_t &&
                      ldz_t >= K && ldz_b >= (long)Tmax * ldz_t,
                  "align_project: bad shape B=%d Tmax=%d ldy_b=%ld ldy_t=%ld ldz_b=%ld ldz_t=%ld", B, Tmax, ldy_b, ldy_t, ldz_b, ldz_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_project_kernel<<<dim3(fs2_cdiv(K, LDA_TILE), fs2_cdiv(Tmax, LDA_TILE), B), 256, 0, stream>>>(y, ldy_b, ldy_t, lens, P, o, K, Ds,
                                                                                                     z, ldz_b, ldz_t, Tmax);
    FS2_CHECK_LAUNCH("align_project");
    return FS2_OK;
}
