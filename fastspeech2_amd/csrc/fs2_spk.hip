// fs2_spk.hip — the GMM-UBM speaker-similarity score: cepstral features with deltas, the log-likelihood of packed frames under
// groups of diagonal Gaussian mixtures, the sufficient statistics of a mixture and the per-utterance mean log-likelihood ratio, all
// in fp64.  The specification is fastspeech2_amd/speaker.py's docstring (mirrored in DESIGN.md); tests/spk_ref.py restates it in
// numpy.
//
//   fs2_spk_feats      one workgroup per utterance: the largest c0, the frames within energy_floor of it, their mean and variance
//                      per dimension (one lane per dimension, frames ascending, mean first and the squares about it second), then
//                      the kept frames normalised and packed in time order by a prefix sum over blocks of 256 frames
//   fs2_spk_loglik     L[n][m] = c[m] + sum_d (x_d a[m][d] + x_d^2 b[m][d]) as a [64 frames x 2D] x [2D x 64 components] product
//                      on v_mfma_f64_16x16x4_f64: four waves, each a 32 x 32 quarter as 2 x 2 accumulators.  The A operand [x, x^2]
//                      of the 64 frames is built once in LDS (row stride Kp + 2 doubles: 2 x odd, so the 16 rows and two k of a
//                      half-wave's read fall on 32 different 8-byte banks); the tables are staged 16 k at a time.  The workgroup
//                      walks the M / 64 column tiles of every group of its range and folds them into a running (max, sum) per
//                      lane; 16 lanes and then the two column waves are combined in a fixed order.  With posteriors (G = 1) the
//                      tiles are computed a second time, by the same instructions, and exp(L - lse) is stored.
//   fs2_spk_accum      stats[m][j] += sum_n post[n][m] f[n][j], f = (1, x, x^2): fs2_align_scatter's plan: at most 32 row chunks
//                      whose length depends on N alone, 64 x 64 tiles per chunk with the frame as the MFMA's k, partial tiles in
//                      the caller's workspace, a second kernel adding them in ascending chunk order
//   fs2_spk_mean_rows  out[u][g] = mean over the utterance's packed rows of lse[n][g] - ubm[n], one lane per (u, g), rows ascending
//
// Lane map of v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[i = (lane >> 4) + 4 reg][j =
// lane & 15].  No atomics anywhere; every sum's order depends on the shape alone.
#include "fs2_common.h"
#include <math.h>

#define SPK_MAX_DIM 64
#define SPK_MAX_CEP 32
#define SPK_MAX_MIX 2048
#define SPK_TILE 64
#define SPK_SLAB 16
#define SPK_LDB 18                  // LDS row of the table slab, doubles (2 x odd)
#define SPK_LD 80                   // LDS row of the accumulate slabs, doubles (as fs2_align_lda.hip)
#define SPK_MAX_CHUNKS 32

typedef double spk_f64x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ features
// feature j of frame t: j < n_cep the cepstrum j + 1, else the regression over +-2 frames of cepstrum j - n_cep + 1, clamped indices
static __device__ __forceinline__ double spk_feature(const double* __restrict__ c, long ldc_t, int T, int t, int j, int n_cep) {
    if (j < n_cep) return c[(size_t)t * ldc_t + j + 1];
    const int q = j - n_cep + 1;
    const int p1 = min(t + 1, T - 1), m1 = max(t - 1, 0), p2 = min(t + 2, T - 1), m2 = max(t - 2, 0);
    const double d1 = c[(size_t)p1 * ldc_t + q] - c[(size_t)m1 * ldc_t + q];
    const double d2 = c[(size_t)p2 * ldc_t + q] - c[(size_t)m2 * ldc_t + q];
    return (d1 + 2.0 * d2) / 10.0;
}

__global__ void __launch_bounds__(256) spk_feats_kernel(const double* __restrict__ cep, long ldc_b, long ldc_t,
                                                        const int32_t* __restrict__ lens, const int32_t* __restrict__ offs, int n_cep,
                                                        double energy_floor, double* __restrict__ feat, long ldf,
                                                        int32_t* __restrict__ n_kept, double* __restrict__ mean,
                                                        double* __restrict__ var, long ldm, int Tmax) {
    __shared__ double red[256];
    __shared__ int32_t scan[256];
    __shared__ double mu_s[SPK_MAX_DIM], sd_s[SPK_MAX_DIM];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x, D = 2 * n_cep;
    const int T = min(max(lens[b], 0), Tmax);
    const double* c = cep + (size_t)b * ldc_b;
    // the largest c0
    double mx = -INFINITY;
    for (int t = tid; t < T; t += 256) mx = fmax(mx, c[(size_t)t * ldc_t]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double thr = red[0] - energy_floor;
    // how many frames pass
    int cnt = 0;
    for (int t = tid; t < T; t += 256) cnt += c[(size_t)t * ldc_t] >= thr;
    scan[tid] = cnt;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) scan[tid] += scan[tid + s];
        __syncthreads();
    }
    const int n = scan[0];
    __syncthreads();
    if (n < 2) {
        if (tid == 0) n_kept[b] = 0;
        if (tid < D) mean[(size_t)b * ldm + tid] = var[(size_t)b * ldm + tid] = NAN;
        return;
    }
    // moments, one lane per dimension, frames ascending
    if (tid < D) {
        double s1 = 0.0;
        for (int t = 0; t < T; ++t)
            if (c[(size_t)t * ldc_t] >= thr) s1 += spk_feature(c, ldc_t, T, t, tid, n_cep);
        const double mu = s1 / (double)n;
        double s2 = 0.0;
        for (int t = 0; t < T; ++t)
            if (c[(size_t)t * ldc_t] >= thr) {
                const double e = spk_feature(c, ldc_t, T, t, tid, n_cep) - mu;
                s2 += e * e;
            }
        const double v = s2 / (double)n;
        mean[(size_t)b * ldm + tid] = mu;
        var[(size_t)b * ldm + tid] = v;
        mu_s[tid] = mu;
        sd_s[tid] = sqrt(v);
        if (!(v > 0.0)) bad = 1;                                           // only ever set: no race on the value
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) n_kept[b] = 0;
        return;
    }
    if (tid == 0) n_kept[b] = n;
    // ordered compaction, 256 frames at a time
    double* dst = feat + (size_t)offs[b] * ldf;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + tid;
        const int keep = t < T && c[(size_t)t * ldc_t] >= thr;
        scan[tid] = keep;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                                // inclusive scan
            const int v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (keep) {
            double* row = dst + (size_t)(base + scan[tid] - 1) * ldf;
            for (int j = 0; j < D; ++j) row[j] = (spk_feature(c, ldc_t, T, t, j, n_cep) - mu_s[j]) / sd_s[j];
        }
        base += scan[255];
        __syncthreads();
    }
}

extern "C" int fs2_spk_max_dim(void) { return SPK_MAX_DIM; }
extern "C" int fs2_spk_max_components(void) { return SPK_MAX_MIX; }

extern "C" int fs2_spk_feats(const double* cep, long ldc_b, long ldc_t, const int32_t* lens, const int32_t* offs, int n_cep,
                             double energy_floor, double* feat, long ldf, int32_t* n_kept, double* mean, double* var, long ldm, int B,
                             int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(n_cep >= 1 && n_cep <= SPK_MAX_CEP, "spk_feats: %d cepstra, supported are 1..%d", n_cep, SPK_MAX_CEP);
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && ldc_t >= n_cep + 1 && ldc_b >= (long)Tmax * ldc_t && ldf >= 2 * n_cep && ldm >= 2 * n_cep &&
                      energy_floor >= 0.0,
                  "spk_feats: bad shape B=%d Tmax=%d n_cep=%d ldc_b=%ld ldc_t=%ld ldf=%ld ldm=%ld energy_floor=%g", B, Tmax, n_cep, ldc_b,
                  ldc_t, ldf, ldm, energy_floor);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(lens && offs && n_kept && mean && var && (Tmax == 0 || (cep && feat)), "spk_feats: null pointer");
    spk_feats_kernel<<<B, 256, 0, stream>>>(cep, ldc_b, ldc_t, lens, offs, n_cep, energy_floor, feat, ldf, n_kept, mean, var, ldm, Tmax);
    FS2_CHECK_LAUNCH("spk_feats");
    return FS2_OK;
}

// ------------------------------------------------------------------ log-likelihood
// One 64 x 64 tile of x a^T + x^2 b^T: components j0 .. j0 + 64 of the table rows at `ta` / `tb` (row stride ldt), accumulated over
// Kp = 2 D rounded up to 4.  Every wave passes the same barriers.
static __device__ __forceinline__ void spk_tile(const double* __restrict__ As, int S, double (*Bs)[SPK_LDB],
                                                const double* __restrict__ ta, const double* __restrict__ tb, long ldt, int j0, int M,
                                                int D, int Kp, int tid, spk_f64x4 (&acc)[2][2]) {
    const int lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int rr = tid >> 2, cc = (tid & 3) * 4;                           // staging: component rr of the tile, four k from cc
    const bool ok = j0 + rr < M;
    const size_t row = (size_t)(ok ? j0 + rr : 0) * ldt;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (spk_f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Kp; k0 += SPK_SLAB) {
        double vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + cc + q;
            vb[q] = (ok && k < 2 * D) ? (k < D ? ta[row + k] : tb[row + k - D]) : 0.0;
        }
        __syncthreads();                                                   // the previous slab has been consumed
#pragma unroll
        for (int q = 0; q < 4; ++q) Bs[rr][cc + q] = vb[q];
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SPK_SLAB / 4; ++ks) {
            if (k0 + ks * 4 >= Kp) break;                                  // uniform: A holds Kp columns only
            const int kb = ks * 4 + (lane >> 4), ka = k0 + kb;
            const double a0 = As[(wi * 32 + (lane & 15)) * S + ka], a1 = As[(wi * 32 + 16 + (lane & 15)) * S + ka];
            const double b0 = Bs[wj * 32 + (lane & 15)][kb], b1 = Bs[wj * 32 + 16 + (lane & 15)][kb];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// (m, s) <- the log-sum-exp pair of (m, s) and (mo, so); symmetric in its arguments bit for bit
static __device__ __forceinline__ void spk_merge(double& m, double& s, double mo, double so) {
    const double t = fmax(m, mo);
    if (t > -INFINITY) {
        s = s * exp(m - t) + so * exp(mo - t);
        m = t;
    }
}

__global__ void __launch_bounds__(256) spk_loglik_kernel(const double* __restrict__ x, long ldx, const double* __restrict__ a,
                                                         const double* __restrict__ b, long ldt, const double* __restrict__ c,
                                                         double* __restrict__ lse, long ldl, double* __restrict__ post, long ldp, int N,
                                                         int D, int M, int G, int Kp) {
    extern __shared__ double As[];                                         // [64][Kp + 2]
    __shared__ double Bs[SPK_TILE][SPK_LDB];
    __shared__ double mx_s[SPK_TILE], sm_s[SPK_TILE], lse_s[SPK_TILE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1, S = Kp + 2;
    const int n0 = blockIdx.x * SPK_TILE;
    for (int e = tid; e < SPK_TILE * Kp; e += 256) {
        const int r = e / Kp, k = e - r * Kp;
        double v = 0.0;
        if (n0 + r < N && k < 2 * D) {
            const double xv = x[(size_t)(n0 + r) * ldx + (k < D ? k : k - D)];
            v = k < D ? xv : xv * xv;
        }
        As[r * S + k] = v;
    }
    __syncthreads();
    spk_f64x4 acc[2][2];
    for (int g = blockIdx.y; g < G; g += gridDim.y) {
        const double *ta = a + (size_t)g * M * ldt, *tb = b + (size_t)g * M * ldt, *tc = c + (size_t)g * M;
        double rm[2][4], rs[2][4];                                         // this lane's running pair for its eight frames
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) rm[m][reg] = -INFINITY, rs[m][reg] = 0.0;
        for (int j0 = 0; j0 < M; j0 += SPK_TILE) {
            spk_tile(As, S, Bs, ta, tb, ldt, j0, M, D, Kp, tid, acc);
            const int ja = j0 + wj * 32 + (lane & 15), jb = ja + 16;
            const double ca = ja < M ? tc[ja] : -INFINITY, cb = jb < M ? tc[jb] : -INFINITY;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const double va = ja < M ? acc[m][0][reg] + ca : -INFINITY, vb = jb < M ? acc[m][1][reg] + cb : -INFINITY;
                    const double t = fmax(fmax(va, vb), rm[m][reg]);
                    if (t > -INFINITY) {
                        rs[m][reg] = rs[m][reg] * exp(rm[m][reg] - t) + exp(va - t) + exp(vb - t);
                        rm[m][reg] = t;
                    }
                }
        }
        // the 16 lanes of a row, then the two column waves
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const double mo = __shfl_xor(rm[m][reg], o, 64), so = __shfl_xor(rs[m][reg], o, 64);
                    spk_merge(rm[m][reg], rs[m][reg], mo, so);
                }
        __syncthreads();                                                   // the previous group's exchange has been read
        if (wj == 1 && (lane & 15) == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = wi * 32 + m * 16 + (lane >> 4) + 4 * reg;
                    mx_s[i] = rm[m][reg];
                    sm_s[i] = rs[m][reg];
                }
        }
        __syncthreads();
        if (wj == 0 && (lane & 15) == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = wi * 32 + m * 16 + (lane >> 4) + 4 * reg;
                    double mm = rm[m][reg], ss = rs[m][reg];
                    spk_merge(mm, ss, mx_s[i], sm_s[i]);
                    const double v = mm > -INFINITY ? mm + log(ss) : -INFINITY;
                    lse_s[i] = v;
                    if (n0 + i < N) lse[(size_t)(n0 + i) * ldl + g] = v;
                }
        }
        if (post == nullptr) continue;                                     // uniform
        __syncthreads();
        for (int j0 = 0; j0 < M; j0 += SPK_TILE) {
            spk_tile(As, S, Bs, ta, tb, ldt, j0, M, D, Kp, tid, acc);
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) {
                const int j = j0 + wj * 32 + nn * 16 + (lane & 15);
                if (j >= M) continue;
                const double cj = tc[j];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = wi * 32 + m * 16 + (lane >> 4) + 4 * reg;
                        if (n0 + i >= N) continue;
                        const double l = lse_s[i];
                        post[(size_t)(n0 + i) * ldp + j] = l > -INFINITY ? exp(acc[m][nn][reg] + cj - l) : 0.0;
                    }
            }
        }
    }
}

extern "C" int fs2_spk_loglik(const double* x, long ldx, const double* a, const double* b, long ldt, const double* c, double* lse,
                              long ldl, double* post, long ldp, int N, int D, int M, int G, hipStream_t stream) {
    FS2_CHECK_ARG(D >= 1 && D <= SPK_MAX_DIM, "spk_loglik: %d dimensions, supported are 1..%d", D, SPK_MAX_DIM);
    FS2_CHECK_ARG(M >= 1 && M <= SPK_MAX_MIX, "spk_loglik: %d components, supported are 1..%d", M, SPK_MAX_MIX);
    FS2_CHECK_ARG(G >= 1 && (long)G * M < (1L << 31), "spk_loglik: %d groups of %d components, supported are G >= 1 and G M < 2^31", G, M);
    FS2_CHECK_ARG(post == nullptr || G == 1, "spk_loglik: posteriors are written for one group only, got G=%d", G);
    FS2_CHECK_ARG(N >= 0 && ldx >= D && ldt >= D && ldl >= G && (post == nullptr || ldp >= M),
                  "spk_loglik: bad shape N=%d D=%d M=%d G=%d ldx=%ld ldt=%ld ldl=%ld ldp=%ld", N, D, M, G, ldx, ldt, ldl, ldp);
    FS2_CHECK_ARG(a && b && c, "spk_loglik: null pointer");
    if (N == 0) return FS2_OK;
    FS2_CHECK_ARG(x && lse, "spk_loglik: null pointer");
    const int Kp = (2 * D + 3) / 4 * 4;
    const size_t lds = (size_t)SPK_TILE * (Kp + 2) * sizeof(double);       // at most 66560 bytes: above the 64 KiB a kernel gets unasked
    static Fs2DevOnce once;
    once.run([&] {
        (void)hipFuncSetAttribute((const void*)spk_loglik_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  SPK_TILE * (2 * SPK_MAX_DIM + 2) * (int)sizeof(double));
    });
    spk_loglik_kernel<<<dim3(fs2_cdiv(N, SPK_TILE), G < 65535 ? G : 65535), 256, lds, stream>>>(x, ldx, a, b, ldt, c, lse, ldl, post, ldp,
                                                                                                N, D, M, G, Kp);
    FS2_CHECK_LAUNCH("spk_loglik");
    return FS2_OK;
}

// ------------------------------------------------------------------ statistics
static void spk_plan(long N, long* rows_per, int* n_chunks) {
    long rp = (N + SPK_MAX_CHUNKS - 1) / SPK_MAX_CHUNKS;
    rp = (rp + SPK_SLAB - 1) / SPK_SLAB * SPK_SLAB;
    if (rp < SPK_SLAB) rp = SPK_SLAB;
    *rows_per = rp;
    *n_chunks = (int)((N + rp - 1) / rp);
}

// Workspace of chunk ch: nmt x njt tiles [64][64], tile p = I njt + J: rows are components of block I, columns statistics of block J.
// k is the frame; both operands are read from [frame][.] slabs.
__global__ void __launch_bounds__(256) spk_accum_kernel(const double* __restrict__ post, long ldp, const double* __restrict__ x,
                                                        long ldx, int D, int M, double* __restrict__ ws, long chunk_doubles, int njt,
                                                        long rows_per, int N) {
    __shared__ double pa[SPK_SLAB][SPK_LD], fb[SPK_SLAB][SPK_LD];
    const int p = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    const int I = p / njt, J = p - I * njt, W = 1 + 2 * D;
    const long r_begin = (long)ch * rows_per, r_end = min((long)N, r_begin + rows_per);
    const int lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int rr = tid >> 4, cc = (tid & 15) * 4;                          // staging: row rr of the slab, four columns from cc
    spk_f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (spk_f64x4){0.0, 0.0, 0.0, 0.0};
    for (long r0 = r_begin; r0 < r_end; r0 += SPK_SLAB) {
        const long r = r0 + rr;
        const bool ok = r < r_end;
        const double *ps = post + (size_t)(ok ? r : 0) * ldp, *xs = x + (size_t)(ok ? r : 0) * ldx;
        double va[4], vb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = I * SPK_TILE + cc + q, j = J * SPK_TILE + cc + q;
            va[q] = (ok && m < M) ? ps[m] : 0.0;
            double f = 0.0;
            if (ok && j < W) {
                if (j == 0) f = 1.0;
                else if (j <= D) f = xs[j - 1];
                else {
                    const double xv = xs[j - 1 - D];
                    f = xv * xv;
                }
            }
            vb[q] = f;
        }
        __syncthreads();                                                   // the previous slab has been consumed
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pa[rr][cc + q] = va[q];
            fb[rr][cc + q] = vb[q];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SPK_SLAB / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            const double a0 = pa[kk][wi * 32 + (lane & 15)], a1 = pa[kk][wi * 32 + 16 + (lane & 15)];
            const double b0 = fb[kk][wj * 32 + (lane & 15)], b1 = fb[kk][wj * 32 + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* tile = ws + (size_t)ch * chunk_doubles + (size_t)p * SPK_TILE * SPK_TILE;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = wi * 32 + m * 16 + (lane >> 4) + 4 * reg, j = wj * 32 + n * 16 + (lane & 15);
                tile[i * SPK_TILE + j] = acc[m][n][reg];
            }
}

__global__ void __launch_bounds__(256) spk_accum_finish_kernel(const double* __restrict__ ws, long chunk_doubles, int n_chunks, int njt,
                                                               int D, int M, double* __restrict__ stats, long lds) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int I = p / njt, J = p - I * njt, W = 1 + 2 * D;
    const double* tile = ws + (size_t)p * SPK_TILE * SPK_TILE;
    for (int e = tid; e < SPK_TILE * SPK_TILE; e += 256) {
        const int m = I * SPK_TILE + (e >> 6), j = J * SPK_TILE + (e & 63);
        if (m >= M || j >= W) continue;
        double tot = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) tot += tile[(size_t)ch * chunk_doubles + e];
        stats[(size_t)m * lds + j] += tot;
    }
}

extern "C" int fs2_spk_accum_ws(int N, int D, int M) {
    if (N <= 0 || D < 1 || D > SPK_MAX_DIM || M < 1 || M > SPK_MAX_MIX) return 0;
    long rows_per;
    int n_chunks;
    spk_plan(N, &rows_per, &n_chunks);
    return n_chunks * fs2_cdiv(M, SPK_TILE) * fs2_cdiv(1 + 2 * D, SPK_TILE) * SPK_TILE * SPK_TILE;
}

extern "C" int fs2_spk_accum(const double* post, long ldp, const double* x, long ldx, double* stats, long lds, double* ws,
                             long ws_doubles, int N, int D, int M, hipStream_t stream) {
    FS2_CHECK_ARG(D >= 1 && D <= SPK_MAX_DIM, "spk_accum: %d dimensions, supported are 1..%d", D, SPK_MAX_DIM);
    FS2_CHECK_ARG(M >= 1 && M <= SPK_MAX_MIX, "spk_accum: %d components, supported are 1..%d", M, SPK_MAX_MIX);
    FS2_CHECK_ARG(N >= 0 && ldp >= M && ldx >= D && lds >= 1 + 2 * D, "spk_accum: bad shape N=%d D=%d M=%d ldp=%ld ldx=%ld lds=%ld", N, D,
                  M, ldp, ldx, lds);
    FS2_CHECK_ARG(stats, "spk_accum: null pointer");
    if (N == 0) return FS2_OK;
    FS2_CHECK_ARG(post && x, "spk_accum: null pointer");
    long rows_per;
    int n_chunks;
    spk_plan(N, &rows_per, &n_chunks);
    const int nmt = fs2_cdiv(M, SPK_TILE), njt = fs2_cdiv(1 + 2 * D, SPK_TILE);
    const long chunk = (long)nmt * njt * SPK_TILE * SPK_TILE;
    FS2_CHECK_ARG(ws && ws_doubles >= n_chunks * chunk, "spk_accum: workspace of %ld doubles, %ld needed (fs2_spk_accum_ws)", ws_doubles,
                  n_chunks * chunk);
    spk_accum_kernel<<<dim3(nmt * njt, n_chunks), 256, 0, stream>>>(post, ldp, x, ldx, D, M, ws, chunk, njt, rows_per, N);
    FS2_CHECK_LAUNCH("spk_accum");
    spk_accum_finish_kernel<<<nmt * njt, 256, 0, stream>>>(ws, chunk, n_chunks, njt, D, M, stats, lds);
    FS2_CHECK_LAUNCH("spk_accum (finish)");
    return FS2_OK;
}

// ------------------------------------------------------------------ mean log-likelihood ratio
__global__ void spk_mean_rows_kernel(const double* __restrict__ lse, long ldl, const double* __restrict__ ubm,
                                     const int32_t* __restrict__ offs, const int32_t* __restrict__ n_kept, double* __restrict__ out,
                                     long ldo, int U, int G) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)U * G) return;
    const int u = (int)(e / G), g = (int)(e - (long)u * G);
    const int n = n_kept[u];
    if (n <= 0) {
        out[(size_t)u * ldo + g] = NAN;
        return;
    }
    const size_t r0 = (size_t)offs[u];
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += lse[(r0 + r) * ldl + g] - ubm[r0 + r];
    out[(size_t)u * ldo + g] = s / (double)n;
}

extern "C" int fs2_spk_mean_rows(const double* lse, long ldl, const double* ubm, const int32_t* offs, const int32_t* n_kept, double* out,
                                 long ldo, int U, int G, hipStream_t stream) {
    FS2_CHECK_ARG(U >= 0 && G >= 1 && ldl >= G && ldo >= G && (long)U * G < (1L << 31) * 256, "spk_mean_rows: bad shape U=%d G=%d ldl=%ld ldo=%ld",
                  U, G, ldl, ldo);
    if (U == 0) return FS2_OK;
    FS2_CHECK_ARG(lse && ubm && offs && n_kept && out, "spk_mean_rows: null pointer");
    spk_mean_rows_kernel<<<fs2_cdiv((long)U * G, 256), 256, 0, stream>>>(lse, ldl, ubm, offs, n_kept, out, ldo, U, G);
    FS2_CHECK_LAUNCH("spk_mean_rows");
    return FS2_OK;
}
