// fs2_align_fmllr.hip — the forced aligner's speaker adaptation (constrained MLLR): the frame weights, the per-speaker statistics
// and the application of the transforms, in fp64 on ragged batches.  The specification is the "fMLLR" paragraph of
// fastspeech2_amd/align.py's docstring (mirrored in DESIGN.md); tests/align_fmllr_ref.py restates it in numpy.  Nothing here has been
// timed.
//
// Shapes.  Utterance b has T = lens[b] frames and J = jlens[b] states; f, c, h and the output are [B][Tmax][D], gamma is
// [B][Tmax][Jmax], all with explicit batch and frame strides.  Nothing at t >= T or j >= J is read (the tests poison it with NaN) and
// nothing there is written.  1 <= D <= 64; xi = (f, 1) has P = D + 1 entries.
//
//   fs2_align_fmllr_weights  c[b][t][i] = sum_j gamma / var[sid_j][i], h = sum_j gamma mu / var, j ascending; one lane per (t, i)
//   fs2_align_fmllr_accum    beta[s] += frames, G[s][i] += sum_t c[t][i] xi xi^T, k[s][i] += sum_t h[t][i] xi over the utterances the
//                            CSR (offs, rows) lists for speaker s, in list order.  A speaker's padded rows l Tmax + t (l its l-th
//                            utterance) are cut into chunks of `rows_per` rows, the split of fs2_align_scatter: a function of
//                            (B, Tmax) alone, so the whole batch has at most 32 + B chunks and the speakers of more than one
//                            chunk own fewer than 64 between them.  A small kernel turns the CSR into that list of chunks on the
//                            device.  One workgroup per (chunk, dimension i): 16 frames at a time go to LDS twice, as c[t][i] xi[t]
//                            and as xi[t] ([frame][entry], 80 entries, rows padded to 112 doubles: 112 = 16 mod 32, so the two
//                            frame rows a half-wave reads with ds_read_b64 fall on disjoint banks, as in fs2_align_lda.hip); the
//                            16 x 16 tiles of the lower triangle of the 80 x 80 product are dealt to the four waves, each tile one
//                            v_mfma_f64_16x16x4_f64 accumulator with the frame as the instruction's k, frames ascending.  The chunk
//                            of a one-chunk speaker is added to the tables directly; the others go to the caller's workspace and
//                            a third kernel adds them in ascending chunk order.  Every value is written to (p, q) and (q, p): G is
//                            exactly symmetric.  No atomics; the tables of a speaker without rows are not touched.
//   fs2_align_fmllr_apply    out[b][t] = W[spk[b]] xi[b][t]: the speaker's W transposed in LDS, 64 frames per workgroup, the sum
//                            over the entries of f ascending, the offset last
#include "fs2_common.h"

#define FM_MAX_DIM 64
#define FM_SLAB 16
#define FM_LD 112                   // LDS row of the slabs, doubles: D + 1 <= 65 padded to 80, whole 16-tiles, and on to 16 mod 32
#define FM_MAX_CHUNKS 32
#define FM_MAX_SLOTS 64             // chunks of the speakers that have more than one
#define FM_MAX_MULTI 32             // such speakers
#define FM_MAX_BATCH (1 << 24)      // utterances per batch
#define FM_PLAN_HEAD 4              // ints: n_items, n_multi, 0, 0

typedef double fm_f64x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ int fm_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }

extern "C" int fs2_align_max_fmllr_dim(void) { return FM_MAX_DIM; }

// ------------------------------------------------------------------ weights
__global__ void __launch_bounds__(256) align_fmllr_weights_kernel(const double* __restrict__ gamma, long ldg_b, long ldg_t,
                                                                  const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                                  const int32_t* __restrict__ sid, long ldsid,
                                                                  const double* __restrict__ mu, const double* __restrict__ var, int C,
                                                                  int D, double* __restrict__ c, double* __restrict__ h, long ldc_b,
                                                                  long ldc_t, int Tmax, int Jmax) {
    const int b = blockIdx.y, T = fm_len(lens, b, Tmax), J = fm_len(jlens, b, Jmax);
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), i = threadIdx.x & 63;
    if (t >= T || i >= D) return;
    const double* g = gamma + (size_t)b * ldg_b + (size_t)t * ldg_t;
    const int32_t* cls = sid + (size_t)b * ldsid;
    double cs = 0.0, hs = 0.0;
    for (int j = 0; j < J; ++j) {
        const double gj = g[j];
        const int k = cls[j];
        if (gj == 0.0 || k < 0 || k >= C) continue;                        // a zero posterior adds nothing
        const double iv = 1.0 / var[(size_t)k * D + i];
        cs += gj * iv;
        hs += gj * (mu[(size_t)k * D + i] * iv);
    }
    c[(size_t)b * ldc_b + (size_t)t * ldc_t + i] = cs;
    h[(size_t)b * ldc_b + (size_t)t * ldc_t + i] = hs;
}

extern "C" int fs2_align_fmllr_weights(const double* gamma, long ldg_b, long ldg_t, const int32_t* lens, const int32_t* jlens,
                                       const int32_t* sid, long ldsid, const double* mu, const double* var, int n_classes, int D,
                                       double* c, double* h, long ldc_b, long ldc_t, int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(gamma && lens && jlens && sid && mu && var && c && h, "align_fmllr_weights: null pointer");
    FS2_CHECK_ARG(D >= 1 && D <= FM_MAX_DIM, "align_fmllr_weights: %d dimensions, supported are 1..%d", D, FM_MAX_DIM);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Jmax >= 0 && n_classes >= 1 && ldg_t >= Jmax && ldg_b >= (long)Tmax * ldg_t &&
                      ldsid >= Jmax && ldc_t >= D && ldc_b >= (long)Tmax * ldc_t,
                  "align_fmllr_weights: bad shape B=%d Tmax=%d Jmax=%d C=%d ldg_b=%ld ldg_t=%ld ldsid=%ld ldc_b=%ld ldc_t=%ld", B, Tmax,
                  Jmax, n_classes, ldg_b, ldg_t, ldsid, ldc_b, ldc_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_fmllr_weights_kernel<<<dim3(fs2_cdiv(Tmax, 4), B), 256, 0, stream>>>(gamma, ldg_b, ldg_t, lens, jlens, sid, ldsid, mu, var,
                                                                               n_classes, D, c, h, ldc_b, ldc_t, Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_fmllr_weights");
    return FS2_OK;
}

// ------------------------------------------------------------------ accumulate
// The chunk length of fs2_align_scatter: ceil(R / 32) rounded up to a multiple of 16, R = B Tmax padded rows.
static long fm_rows_per(long R) {
    long rp = (R + FM_MAX_CHUNKS - 1) / FM_MAX_CHUNKS;
    rp = (rp + FM_SLAB - 1) / FM_SLAB * FM_SLAB;
    return rp < FM_SLAB ? FM_SLAB : rp;
}
static long fm_plan_ints(int B) { return FM_PLAN_HEAD + 4L * (FM_MAX_CHUNKS + B) + 4L * FM_MAX_MULTI; }
static long fm_plan_doubles(int B) { return (fm_plan_ints(B) + 1) / 2; }
static long fm_part_doubles(int D) { return (long)(D + 1) * (D + 1) + (D + 1); }       // one (chunk, i): G then k

// plan: ints [n_items, n_multi, 0, 0], then items {speaker, chunk, workspace slot or -1, 0} in speaker order, chunks ascending, then
// the speakers of more than one chunk {speaker, first slot, chunks, 0}.  Also beta.  A list that is no CSR of the batch's rows (an
// offset or a row outside the batch) is skipped where it is wrong, so that nothing is read or written out of bounds.
__global__ void __launch_bounds__(256) align_fmllr_plan_kernel(const int32_t* __restrict__ lens, const int32_t* __restrict__ offs,
                                                               const int32_t* __restrict__ rows, int n_spk, double* __restrict__ beta,
                                                               int32_t* __restrict__ plan, int max_items, long rows_per, int B, int Tmax) {
    for (int s = threadIdx.x; s < n_spk; s += 256) {
        const int o0 = offs[s], o1 = offs[s + 1];
        if (o0 < 0 || o1 > B || o1 <= o0) continue;
        double n = 0.0;
        for (int e = o0; e < o1; ++e) {
            const int b = rows[e];
            if (b >= 0 && b < B) n += (double)fm_len(lens, b, Tmax);
        }
        beta[s] += n;
    }
    if (threadIdx.x != 0) return;
    int32_t* items = plan + FM_PLAN_HEAD;
    int32_t* multi = items + 4L * max_items;
    int n_items = 0, n_multi = 0, n_slots = 0;
    for (int s = 0; s < n_spk; ++s) {
        const int o0 = offs[s], o1 = offs[s + 1];
        if (o0 < 0 || o1 > B || o1 <= o0) continue;
        const long cnt = ((long)(o1 - o0) * Tmax + rows_per - 1) / rows_per;
        if (n_items + cnt > max_items) break;
        if (cnt > 1 && (n_multi >= FM_MAX_MULTI || n_slots + cnt > FM_MAX_SLOTS)) break;
        for (int ch = 0; ch < (int)cnt; ++ch) {
            int32_t* it = items + 4L * n_items++;
            it[0] = s;
            it[1] = ch;
            it[2] = cnt > 1 ? n_slots + ch : -1;
            it[3] = 0;
        }
        if (cnt > 1) {
            int32_t* m = multi + 4L * n_multi++;
            m[0] = s;
            m[1] = n_slots;
            m[2] = (int)cnt;
            m[3] = 0;
            n_slots += (int)cnt;
        }
    }
    plan[0] = n_items;
    plan[1] = n_multi;
    plan[2] = plan[3] = 0;
}

// Lane map of v_mfma_f64_16x16x4_f64 (see fs2_align_lda.hip): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[i = (lane >> 4) + 4 reg][j = lane & 15].  Here k is the frame, A is read from the slab of c xi and B from the slab of xi.
__global__ void __launch_bounds__(256) align_fmllr_accum_kernel(const double* __restrict__ f, long ldf_b, long ldf_t,
                                                                const double* __restrict__ c, const double* __restrict__ h, long ldc_b,
                                                                long ldc_t, const int32_t* __restrict__ lens,
                                                                const int32_t* __restrict__ offs, const int32_t* __restrict__ rows, int D,
                                                                double* __restrict__ G, double* __restrict__ kt, double* __restrict__ parts,
                                                                const int32_t* __restrict__ plan, long rows_per, int B, int Tmax) {
    __shared__ double xa[FM_SLAB][FM_LD], xb[FM_SLAB][FM_LD], hsl[FM_SLAB];
    const int item = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    if (item >= plan[0]) return;
    const int32_t* it = plan + FM_PLAN_HEAD + 4L * item;
    const int s = it[0], ch = it[1], slot = it[2];
    const int P = D + 1, o0 = offs[s];
    const long Rs = (long)(offs[s + 1] - o0) * Tmax, r_begin = (long)ch * rows_per, r_end = min(Rs, r_begin + rows_per);
    const int lane = tid & 63, w = tid >> 6;
    const int nt = (P + 15) >> 4, ntri = nt * (nt + 1) / 2;
    int tI[4], tJ[4];                                                      // tile w + 4 q of the lower triangle, at most 15 of them
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = w + 4 * q;
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= p) ++I;
        tI[q] = p < ntri ? I : -1;
        tJ[q] = p - I * (I + 1) / 2;
    }
    const int rr = tid >> 4, c0 = (tid & 15) * 5;                          // staging: frame rr of the slab, five entries from c0
    fm_f64x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = (fm_f64x4){0.0, 0.0, 0.0, 0.0};
    double ksum = 0.0;
    for (long r0 = r_begin; r0 < r_end; r0 += FM_SLAB) {
        const long r = r0 + rr;
        bool ok = r < r_end;
        const double* src = f;
        double cv = 0.0, hv = 0.0;
        if (ok) {
            const int l = (int)(r / Tmax), t = (int)(r - (long)l * Tmax), b = rows[o0 + l];
            ok = b >= 0 && b < B && t < fm_len(lens, b, Tmax);
            if (ok) {
                src = f + (size_t)b * ldf_b + (size_t)t * ldf_t;
                cv = c[(size_t)b * ldc_b + (size_t)t * ldc_t + i];
                hv = h[(size_t)b * ldc_b + (size_t)t * ldc_t + i];
            }
        }
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int p = c0 + q;
            v[q] = !ok ? 0.0 : p < D ? src[p] : p == D ? 1.0 : 0.0;
        }
        __syncthreads();                                                   // the previous slab has been consumed
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            xa[rr][c0 + q] = cv * v[q];
            xb[rr][c0 + q] = v[q];
        }
        if ((tid & 15) == 0) hsl[rr] = hv;
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < FM_SLAB / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (tI[q] >= 0)                                            // the same for the whole wave
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[kk][tI[q] * 16 + (lane & 15)], xb[kk][tJ[q] * 16 + (lane & 15)],
                                                                  acc[q], 0, 0, 0);
        }
        if (tid < P) {
#pragma unroll
            for (int k = 0; k < FM_SLAB; ++k) ksum += hsl[k] * xb[k][tid];
        }
    }
    const bool direct = slot < 0;
    double* dG = direct ? G + ((size_t)s * D + i) * P * P : parts + ((size_t)slot * D + i) * ((size_t)P * P + P);
    double* dk = direct ? kt + ((size_t)s * D + i) * P : dG + (size_t)P * P;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (tI[q] < 0) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int p = tI[q] * 16 + (lane >> 4) + 4 * reg, j = tJ[q] * 16 + (lane & 15);
            if (p >= P || j > p) continue;
            if (direct) {
                const double val = dG[(size_t)p * P + j] + acc[q][reg];
                dG[(size_t)p * P + j] = val;
                dG[(size_t)j * P + p] = val;
            } else {
                dG[(size_t)p * P + j] = acc[q][reg];
            }
        }
    }
    if (tid < P) dk[tid] = direct ? dk[tid] + ksum : ksum;
}

// The chunks of a speaker that has more than one, in ascending order, then onto the tables; (p, q) and (q, p) get the same value.
__global__ void __launch_bounds__(256) align_fmllr_finish_kernel(const double* __restrict__ parts, const int32_t* __restrict__ plan,
                                                                 int max_items, int D, double* __restrict__ G, double* __restrict__ kt) {
    const int m = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    if (m >= plan[1]) return;
    const int32_t* mm = plan + FM_PLAN_HEAD + 4L * max_items + 4L * m;
    const int s = mm[0], slot0 = mm[1], cnt = mm[2], P = D + 1;
    const size_t part = (size_t)P * P + P, step = (size_t)D * part;
    const double* first = parts + ((size_t)slot0 * D + i) * part;
    double* dG = G + ((size_t)s * D + i) * P * P;
    for (int e = tid; e < P * P; e += 256) {
        const int p = e / P, j = e - p * P;
        if (j > p) continue;
        double tot = 0.0;
        for (int ch = 0; ch < cnt; ++ch) tot += first[(size_t)ch * step + e];
        const double val = dG[e] + tot;
        dG[e] = val;
        dG[(size_t)j * P + p] = val;
    }
    if (tid < P) {
        double tot = 0.0;
        for (int ch = 0; ch < cnt; ++ch) tot += first[(size_t)ch * step + (size_t)P * P + tid];
        kt[((size_t)s * D + i) * P + tid] += tot;
    }
}

extern "C" int fs2_align_fmllr_accum_ws(int B, int Tmax, int D) {
    if (B <= 0 || B > FM_MAX_BATCH || Tmax <= 0 || D <= 0 || D > FM_MAX_DIM) return 0;
    return (int)(fm_plan_doubles(B) + (long)FM_MAX_SLOTS * D * fm_part_doubles(D));
}

extern "C" int fs2_align_fmllr_accum(const double* f, long ldf_b, long ldf_t, const double* c, const double* h, long ldc_b, long ldc_t,
                                     const int32_t* lens, const int32_t* offs, const int32_t* rows, int n_spk, int D, double* beta,
                                     double* G, double* k, double* ws, long ws_doubles, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(f && c && h && lens && offs && rows && beta && G && k, "align_fmllr_accum: null pointer");
    FS2_CHECK_ARG(D >= 1 && D <= FM_MAX_DIM, "align_fmllr_accum: %d dimensions, supported are 1..%d", D, FM_MAX_DIM);
    FS2_CHECK_ARG(B >= 0 && B <= FM_MAX_BATCH && Tmax >= 0 && n_spk >= 1 && ldf_t >= D && ldf_b >= (long)Tmax * ldf_t && ldc_t >= D &&
                      ldc_b >= (long)Tmax * ldc_t,
                  "align_fmllr_accum: bad shape B=%d Tmax=%d n_spk=%d ldf_b=%ld ldf_t=%ld ldc_b=%ld ldc_t=%ld", B, Tmax, n_spk, ldf_b, ldf_t,
                  ldc_b, ldc_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    const long need = fs2_align_fmllr_accum_ws(B, Tmax, D);
    FS2_CHECK_ARG(ws && ws_doubles >= need, "align_fmllr_accum: workspace of %ld doubles, %ld needed (fs2_align_fmllr_accum_ws)",
                  ws_doubles, need);
    const long rows_per = fm_rows_per((long)B * Tmax);
    const int max_items = FM_MAX_CHUNKS + B;
    int32_t* plan = (int32_t*)ws;
    double* parts = ws + fm_plan_doubles(B);
    align_fmllr_plan_kernel<<<1, 256, 0, stream>>>(lens, offs, rows, n_spk, beta, plan, max_items, rows_per, B, Tmax);
    FS2_CHECK_LAUNCH("align_fmllr_accum (plan)");
    align_fmllr_accum_kernel<<<dim3(max_items, D), 256, 0, stream>>>(f, ldf_b, ldf_t, c, h, ldc_b, ldc_t, lens, offs, rows, D, G, k, parts,
                                                                     plan, rows_per, B, Tmax);
    FS2_CHECK_LAUNCH("align_fmllr_accum");
    align_fmllr_finish_kernel<<<dim3(FM_MAX_MULTI, D), 256, 0, stream>>>(parts, plan, max_items, D, G, k);
    FS2_CHECK_LAUNCH("align_fmllr_accum (finish)");
    return FS2_OK;
}

// ------------------------------------------------------------------ apply
__global__ void __launch_bounds__(256) align_fmllr_apply_kernel(const double* __restrict__ f, long ldf_b, long ldf_t,
                                                                const int32_t* __restrict__ lens, const double* __restrict__ W,
                                                                const int32_t* __restrict__ spk, int n_spk, int D,
                                                                double* __restrict__ out, long ldo_b, long ldo_t, int Tmax) {
    __shared__ double wt[FM_MAX_DIM + 1][FM_MAX_DIM];                      // [entry of xi][output]
    const int b = blockIdx.y, T = fm_len(lens, b, Tmax), t0 = blockIdx.x * 64, tid = threadIdx.x;
    const int s = spk[b], P = D + 1;
    if (t0 >= T || s < 0 || s >= n_spk) return;
    const double* ws = W + (size_t)s * D * P;
    for (int e = tid; e < D * P; e += 256) {
        const int r = e / P;
        wt[e - r * P][r] = ws[e];
    }
    __syncthreads();
    const int r = tid & 63;
    if (r >= D) return;
    for (int t = t0 + (tid >> 6); t < min(T, t0 + 64); t += 4) {
        const double* src = f + (size_t)b * ldf_b + (size_t)t * ldf_t;
        double a = 0.0;
        for (int p = 0; p < D; ++p) a += wt[p][r] * src[p];
        out[(size_t)b * ldo_b + (size_t)t * ldo_t + r] = a + wt[D][r];
    }
}

extern "C" int fs2_align_fmllr_apply(const double* f, long ldf_b, long ldf_t, const int32_t* lens, const double* W, const int32_t* spk,
                                     int n_spk, int D, double* out, long ldo_b, long ldo_t, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(f && lens && W && spk && out, "align_fmllr_apply: null pointer");
    FS2_CHECK_ARG(D >= 1 && D <= FM_MAX_DIM, "align_fmllr_apply: %d dimensions, supported are 1..%d", D, FM_MAX_DIM);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && n_spk >= 1 && ldf_t >= D && ldf_b >= (long)Tmax * ldf_t && ldo_t >= D &&
                      ldo_b >= (long)Tmax * ldo_t,
                  "align_fmllr_apply: bad shape B=%d Tmax=%d n_spk=%d ldf_b=%ld ldf_t=%ld ldo_b=%ld ldo_t=%ld", B, Tmax, n_spk, ldf_b, ldf_t,
                  ldo_b, ldo_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_fmllr_apply_kernel<<<dim3(fs2_cdiv(Tmax, 64), B), 256, 0, stream>>>(f, ldf_b, ldf_t, lens, W, spk, n_spk, D, out, ldo_b, ldo_t,
                                                                              Tmax);
    FS2_CHECK_LAUNCH("align_fmllr_apply");
    return FS2_OK;
}
