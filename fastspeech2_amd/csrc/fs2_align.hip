// fs2_align.hip — forced alignment with a left-to-right monophone HMM: features, diagonal-Gaussian emissions, forward / backward
// (Baum-Welch occupancies), class statistics and Viterbi decoding on ragged batches, all in fp64.
// The specification is the docstring of fastspeech2_amd/align.py (mirrored in DESIGN.md); tests/align_ref.py restates it in numpy.
//
// Shapes.  Utterance b has T = lens[b] frames and J = jlens[b] states; buffers are [B][Tmax][Jmax] with explicit batch and frame
// strides, graphs are [B][Jmax] int32 rows (stride ldg).  Nothing at t >= T or j >= J is read (the tests poison it with NaN) and
// nothing there is written.  alt[b] = {alternative start state or -1, alternative end state or -1}: a path starts in state 0 or
// alt[b][0] and ends in state J - 1 or alt[b][1].
//
//   fs2_align_feats      log-mel [B][n_mel][frames] f32 -> x [B][Tmax][2 n_mel] f64: per-utterance mean removed, central differences
//   fs2_align_emit       E[b][t][j] = -1/2 sum_d ((x_d - mu_d)^2 / var_d + log(2 pi var_d)) for class sid[b][j]; 32 x 32 tiles of
//                        (t, j), the class rows staged in LDS as mu, 1 / var and log(2 pi var)
//   fs2_align_emit_gmm   the same with up to 8 mixture components per class: E = log sum_m exp(N_m), optional responsibilities
//   fs2_align_forward    the three scans: one workgroup per utterance, one state per lane, the previous frame's row in LDS,
//   fs2_align_backward   double-buffered, so a frame costs one barrier; E / alpha / gamma rows are read and written as
//   fs2_align_viterbi    consecutive f64 (bytes for the backpointers), the next frame's operands are loaded one frame ahead
//   fs2_align_*_arcs     the same three scans with a cost on every arc and edge; the backward scan also sums the arc posteriors
//   fs2_align_*_arcs     the same three scans with a cost on every arc and edge; the backward scan also sums the arc posteriors
//   fs2_align_stats      P[b][j] = sum_t gamma[t][j] [1, x_t, x_t^2]: gamma^T [1 x x^2] per utterance, 32 x 32 tiles of (j, d), frames
//                        staged in LDS 32 at a time, summed in ascending t
//   fs2_align_stats_gmm  the same over rows (j, m) with g = gamma[t][j] r[t][j][m], multiplied while a frame block is staged
//   fs2_align_reduce     class sums from the partial rows a host-built CSR index lists, in list order (no atomics anywhere)
//   fs2_align_backtrack  backpointers -> frames per block, one lane per utterance
#include "fs2_common.h"

#define AL_MAX_STATES 1024          // one state per lane of the largest workgroup
#define AL_TILE 32
#define AL_MAX_MIX 8                // mixture components per class: a lane keeps its 4 x 8 component scores in registers

static __device__ __forceinline__ int al_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }
static __device__ __forceinline__ double al_ninf() { return -__builtin_huge_val(); }

// log(exp(a) + exp(b) + exp(c)), the terms added in argument order; -inf when all three are (an absent arc is -inf)
static __device__ __forceinline__ double al_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == al_ninf()) return m;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}
static __device__ __forceinline__ double al_lse2(double a, double b) {
    const double m = fmax(a, b);
    if (m == al_ninf()) return m;
    return m + log(exp(a - m) + exp(b - m));
}

// ------------------------------------------------------------------ features
__global__ void align_mean_kernel(const float* __restrict__ mel, long ldm_b, long ldm_c, const int32_t* __restrict__ lens,
                                  double* __restrict__ mean, int n_mel, int Tmax) {
    __shared__ double red[256];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, T = al_len(lens, b, Tmax);
    const float* r = mel + (size_t)b * ldm_b + (size_t)c * ldm_c;
    double s = 0.0;
    for (int t = tid; t < T; t += 256) s += (double)r[t];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                                   // fixed tree: the same sum on every run
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) mean[(size_t)b * n_mel + c] = T > 0 ? red[0] / (double)T : 0.0;
}
__global__ void align_feats_kernel(const float* __restrict__ mel, long ldm_b, long ldm_c, const int32_t* __restrict__ lens,
                                   const double* __restrict__ mean, double* __restrict__ x, long ldx_b, long ldx_t, int n_mel,
                                   int Tmax) {
    const int b = blockIdx.y, T = al_len(lens, b, Tmax), D = 2 * n_mel;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * D) return;
    const int t = (int)(i / D), d = (int)(i - (long)t * D);
    const int c = d < n_mel ? d : d - n_mel;
    const float* r = mel + (size_t)b * ldm_b + (size_t)c * ldm_c;
    const double mu = mean[(size_t)b * n_mel + c];
    double v;
    if (d < n_mel) {
        v = (double)r[t] - mu;
    } else {
        const double hi = (double)r[min(t + 1, T - 1)] - mu, lo = (double)r[max(t - 1, 0)] - mu;
        v = (hi - lo) / 2.0;
    }
    x[(size_t)b * ldx_b + (size_t)t * ldx_t + d] = v;
}
extern "C" int fs2_align_feats(const float* mel, long ldm_b, long ldm_c, const int32_t* lens, double* mean, double* x, long ldx_b,
                               long ldx_t, int B, int n_mel, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(mel && lens && mean && x, "align_feats: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && n_mel > 0 && n_mel <= 65535 && Tmax >= 0 && ldm_c >= Tmax && ldx_t >= 2 * n_mel &&
                      ldx_b >= (long)Tmax * ldx_t && (long)Tmax * 2 * n_mel < (1L << 31) * 256,
                  "align_feats: bad shape B=%d n_mel=%d Tmax=%d ldm_c=%ld ldx_b=%ld ldx_t=%ld", B, n_mel, Tmax, ldm_c, ldx_b, ldx_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    align_mean_kernel<<<dim3(n_mel, B), 256, 0, stream>>>(mel, ldm_b, ldm_c, lens, mean, n_mel, Tmax);
    align_feats_kernel<<<dim3(fs2_cdiv((long)Tmax * 2 * n_mel, 256), B), 256, 0, stream>>>(mel, ldm_b, ldm_c, lens, mean, x, ldx_b,
                                                                                          ldx_t, n_mel, Tmax);
    FS2_CHECK_LAUNCH("align_feats");
    return FS2_OK;
}

// ------------------------------------------------------------------ emissions
// Tile of 32 frames x 32 states per 256-lane workgroup, the feature dimension in chunks of 32.  Lane (jj = tid & 31, tg = tid >> 5)
// owns frames tg, tg + 8, tg + 16, tg + 24 of state jj: a class value is read from LDS once per four outputs.  Rows are padded to
// 33 doubles so that the 32 states of a wave read 32 different bank pairs.
__global__ void __launch_bounds__(256) align_emit_kernel(const double* __restrict__ x, long ldx_b, long ldx_t,
                                                         const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                         const int32_t* __restrict__ sid, long ldg, const double* __restrict__ mu,
                                                         const double* __restrict__ var, int n_classes, int D, double* __restrict__ E,
                                                         long lde_b, long lde_t, int Tmax, int Jmax) {
    __shared__ double xs[AL_TILE][AL_TILE + 1], ms[AL_TILE][AL_TILE + 1], vs[AL_TILE][AL_TILE + 1], ls[AL_TILE][AL_TILE + 1];
    __shared__ int cls[AL_TILE];
    const int b = blockIdx.z, T = al_len(lens, b, Tmax), J = al_len(jlens, b, Jmax);
    const int t0 = blockIdx.y * AL_TILE, j0 = blockIdx.x * AL_TILE, tid = threadIdx.x;
    if (t0 >= T || j0 >= J) return;
    if (tid < AL_TILE) {
        const int j = j0 + tid;
        const int c = j < J ? sid[(size_t)b * ldg + j] : -1;
        cls[tid] = (c >= 0 && c < n_classes) ? c : -1;                     // a class outside the table yields NaN, never a wild read
    }
    const int jj = tid & 31, tg = tid >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* xb = x + (size_t)b * ldx_b;
    for (int d0 = 0; d0 < D; d0 += AL_TILE) {
        __syncthreads();
        for (int k = tid; k < AL_TILE * AL_TILE; k += 256) {
            const int r = k >> 5, dd = k & 31, d = d0 + dd;
            const int t = t0 + r;
            xs[r][dd] = (t < T && d < D) ? xb[(size_t)t * ldx_t + d] : 0.0;
            const int c = cls[r];
            double m = 0.0, iv = 0.0, lg = 0.0;
            if (d < D) {
                if (c >= 0) {
                    const double v = var[(size_t)c * D + d];
                    m = mu[(size_t)c * D + d];
                    iv = 1.0 / v;
                    lg = log(6.283185307179586476925286766559 * v);
                } else if (j0 + r < J) {
                    lg = __builtin_nan("");
                }
            }
            ms[r][dd] = m;
            vs[r][dd] = iv;
            ls[r][dd] = lg;
        }
        __syncthreads();
#pragma unroll 4
        for (int dd = 0; dd < AL_TILE; ++dd) {
            const double m = ms[jj][dd], iv = vs[jj][dd], lg = ls[jj][dd];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double df = xs[tg + 8 * q][dd] - m;
                acc[q] += df * df * iv + lg;
            }
        }
    }
    const int j = j0 + jj;
    if (j < J) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = t0 + tg + 8 * q;
            if (t < T) E[(size_t)b * lde_b + (size_t)t * lde_t + j] = -0.5 * acc[q];
        }
    }
}
extern "C" int fs2_align_emit(const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens, const int32_t* sid,
                              long ldg, const double* mu, const double* var, int n_classes, int D, double* E, long lde_b, long lde_t,
                              int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && jlens && sid && mu && var && E, "align_emit: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Tmax <= 65535 * AL_TILE && Jmax >= 0 && D > 0 && n_classes > 0 && ldx_t >= D &&
                      ldx_b >= (long)Tmax * ldx_t && lde_t >= Jmax && lde_b >= (long)Tmax * lde_t && ldg >= Jmax,
                  "align_emit: bad shape B=%d Tmax=%d Jmax=%d D=%d classes=%d", B, Tmax, Jmax, D, n_classes);
    FS2_CHECK_ARG(Jmax <= AL_MAX_STATES, "align_emit: %d states exceed the supported maximum of %d", Jmax, AL_MAX_STATES);
    if (B == 0 || Tmax == 0 || Jmax == 0) return FS2_OK;
    align_emit_kernel<<<dim3(fs2_cdiv(Jmax, AL_TILE), fs2_cdiv(Tmax, AL_TILE), B), 256, 0, stream>>>(
        x, ldx_b, ldx_t, lens, jlens, sid, ldg, mu, var, n_classes, D, E, lde_b, lde_t, Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_emit");
    return FS2_OK;
}

// Mixture emissions.  The tile and the lane map of align_emit_kernel; the components are the outer loop, so the D-chunks of x are
// staged once per component (they come from L2 after the first) and LDS stays at the single-Gaussian kernel's 34 KiB for any D,
// where a whole 32-frame tile of x would take 40 KiB at D = 160 and grow with D.  Component m of class c is row c * M + m of the
// tables.  A lane keeps N[m][q] = log w_m - 1/2 sum_d (...) of its four outputs in registers (the loop over m is unrolled), then
// takes the maximum and the sum over ascending m.  log 0 = -inf: a component of weight 0 has responsibility exp(-inf) = 0.
template <int M>
__global__ void __launch_bounds__(256) align_emit_gmm_kernel(const double* __restrict__ x, long ldx_b, long ldx_t,
                                                             const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                             const int32_t* __restrict__ sid, long ldg, const double* __restrict__ w,
                                                             const double* __restrict__ mu, const double* __restrict__ var,
                                                             int n_classes, int D, double* __restrict__ E, long lde_b, long lde_t,
                                                             double* __restrict__ resp, long ldr_b, long ldr_t, long ldr_j, int Tmax,
                                                             int Jmax) {
    __shared__ double xs[AL_TILE][AL_TILE + 1], ms[AL_TILE][AL_TILE + 1], vs[AL_TILE][AL_TILE + 1], ls[AL_TILE][AL_TILE + 1];
    __shared__ double lw[AL_TILE];
    __shared__ int cls[AL_TILE];
    const int b = blockIdx.z, T = al_len(lens, b, Tmax), J = al_len(jlens, b, Jmax);
    const int t0 = blockIdx.y * AL_TILE, j0 = blockIdx.x * AL_TILE, tid = threadIdx.x;
    if (t0 >= T || j0 >= J) return;
    if (tid < AL_TILE) {
        const int j = j0 + tid;
        const int c = j < J ? sid[(size_t)b * ldg + j] : -1;
        cls[tid] = (c >= 0 && c < n_classes) ? c : -1;                     // a class outside the table yields NaN, never a wild read
    }
    const int jj = tid & 31, tg = tid >> 5;
    const double* xb = x + (size_t)b * ldx_b;
    double N[M][4];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < D; d0 += AL_TILE) {
            __syncthreads();
            if (d0 == 0 && tid < AL_TILE) {
                const int c = cls[tid];
                lw[tid] = c >= 0 ? log(w[(size_t)c * M + m]) : 0.0;
            }
            for (int k = tid; k < AL_TILE * AL_TILE; k += 256) {
                const int r = k >> 5, dd = k & 31, d = d0 + dd;
                const int t = t0 + r;
                xs[r][dd] = (t < T && d < D) ? xb[(size_t)t * ldx_t + d] : 0.0;
                const int c = cls[r];
                double mm = 0.0, iv = 0.0, lg = 0.0;
                if (d < D) {
                    if (c >= 0) {
                        const size_t at = ((size_t)c * M + m) * D + d;
                        const double v = var[at];
                        mm = mu[at];
                        iv = 1.0 / v;
                        lg = log(6.283185307179586476925286766559 * v);
                    } else if (j0 + r < J) {
                        lg = __builtin_nan("");
                    }
                }
                ms[r][dd] = mm;
                vs[r][dd] = iv;
                ls[r][dd] = lg;
            }
            __syncthreads();
#pragma unroll 4
            for (int dd = 0; dd < AL_TILE; ++dd) {
                const double mm = ms[jj][dd], iv = vs[jj][dd], lg = ls[jj][dd];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double df = xs[tg + 8 * q][dd] - mm;
                    acc[q] += df * df * iv + lg;
                }
            }
        }
        const double l = lw[jj];                                           // rewritten only after the next component's first barrier
#pragma unroll
        for (int q = 0; q < 4; ++q) N[m][q] = l + -0.5 * acc[q];
    }
    const int j = j0 + jj;
    if (j >= J) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = t0 + tg + 8 * q;
        if (t >= T) continue;
        double mx = N[0][q];
#pragma unroll
        for (int m = 1; m < M; ++m) mx = fmax(mx, N[m][q]);
        double e = mx;
        if (mx != al_ninf()) {
            double s = exp(N[0][q] - mx);
#pragma unroll
            for (int m = 1; m < M; ++m) s += exp(N[m][q] - mx);
            e = mx + log(s);
        }
        E[(size_t)b * lde_b + (size_t)t * lde_t + j] = e;
        if (resp) {
            double* rr = resp + (size_t)b * ldr_b + (size_t)t * ldr_t + (size_t)j * ldr_j;
#pragma unroll
            for (int m = 0; m < M; ++m) rr[m] = mx != al_ninf() ? exp(N[m][q] - e) : 0.0;
        }
    }
}
extern "C" int fs2_align_max_mixtures(void) { return AL_MAX_MIX; }

extern "C" int fs2_align_emit_gmm(const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens,
                                  const int32_t* sid, long ldg, const double* w, const double* mu, const double* var, int n_classes,
                                  int M, int D, double* E, long lde_b, long lde_t, double* resp, long ldr_b, long ldr_t, long ldr_j,
                                  int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && jlens && sid && w && mu && var && E, "align_emit_gmm: null pointer");
    FS2_CHECK_ARG(M >= 1 && M <= AL_MAX_MIX, "align_emit_gmm: %d mixture components, supported are 1..%d", M, AL_MAX_MIX);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Tmax <= 65535 * AL_TILE && Jmax >= 0 && D > 0 && n_classes > 0 && ldx_t >= D &&
                      ldx_b >= (long)Tmax * ldx_t && lde_t >= Jmax && lde_b >= (long)Tmax * lde_t && ldg >= Jmax,
                  "align_emit_gmm: bad shape B=%d Tmax=%d Jmax=%d D=%d classes=%d", B, Tmax, Jmax, D, n_classes);
    FS2_CHECK_ARG(!resp || (ldr_j >= M && ldr_t >= (long)Jmax * ldr_j && ldr_b >= (long)Tmax * ldr_t),
                  "align_emit_gmm: bad responsibility strides %ld %ld %ld", ldr_b, ldr_t, ldr_j);
    FS2_CHECK_ARG(Jmax <= AL_MAX_STATES, "align_emit_gmm: %d states exceed the supported maximum of %d", Jmax, AL_MAX_STATES);
    if (B == 0 || Tmax == 0 || Jmax == 0) return FS2_OK;
    const dim3 grid(fs2_cdiv(Jmax, AL_TILE), fs2_cdiv(Tmax, AL_TILE), B);
#define AL_GMM(MM)                                                                                                                  \
    case MM:                                                                                                                        \
        align_emit_gmm_kernel<MM><<<grid, 256, 0, stream>>>(x, ldx_b, ldx_t, lens, jlens, sid, ldg, w, mu, var, n_classes, D, E, lde_b, \
                                                            lde_t, resp, ldr_b, ldr_t, ldr_j, Tmax, Jmax);                          \
        break
    switch (M) {
        AL_GMM(1); AL_GMM(2); AL_GMM(3); AL_GMM(4); AL_GMM(5); AL_GMM(6); AL_GMM(7); AL_GMM(8);
    }
#undef AL_GMM
    FS2_CHECK_LAUNCH("align_emit_gmm");
    return FS2_OK;
}

// ------------------------------------------------------------------ the scans
// Lane j owns state j.  prev[j + 1] holds the previous frame's value of state j and prev[0] = -inf, so the "next" arc of state 0
// needs no branch; the skip predecessor is one more LDS read.  Frame t reads buffer (t - 1) & 1 and writes buffer t & 1; the barrier
// at the top of frame t + 1 orders those writes before their readers and frame t's reads before frame t + 1's overwrites.
// ARCS (the *_arcs entry points): lane j keeps the costs w[0..2][j] of its three incoming arcs in registers and adds each to the
// predecessor's value before the lse (the max); the start states take edge[0] / edge[1], the end states edge[2] / edge[3].  Without
// ARCS none of that is compiled: the code, and with it every bit, is what it was before the costs existed.
template <int NT, bool ARCS>
__global__ void __launch_bounds__(NT) align_forward_kernel(const double* __restrict__ E, long lde_b, long lde_t,
                                                           const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                           const int32_t* __restrict__ skip, long ldg, const int32_t* __restrict__ alt,
                                                           const double* __restrict__ w, long ldw, const double* __restrict__ edge,
                                                           double* __restrict__ alpha, long lda_b, long lda_t,
                                                           double* __restrict__ loglik, int Tmax, int Jmax) {
    __shared__ double row[2][NT + 1];
    const int b = blockIdx.x, j = threadIdx.x, T = al_len(lens, b, Tmax), J = al_len(jlens, b, min(Jmax, NT));
    if (T == 0 || J == 0) {
        if (j == 0) loglik[b] = al_ninf();
        return;
    }
    const bool on = j < J;
    const int s_alt = alt[2 * b], e_alt = alt[2 * b + 1];
    int sk = on ? skip[(size_t)b * ldg + j] : -1;
    if (sk < 0 || sk >= J) sk = -1;
    const double* Eb = E + (size_t)b * lde_b + j;
    double* Ab = alpha + (size_t)b * lda_b + j;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if constexpr (ARCS) {
        if (on) {
            const double* Wb = w + (size_t)b * 3 * ldw + j;
            w0 = Wb[0];
            w1 = Wb[ldw];
            w2 = Wb[2 * ldw];
        }
    }
    if (j == 0) row[0][0] = row[1][0] = al_ninf();
    double a = al_ninf();
    if (on && (j == 0 || j == s_alt)) {
        if constexpr (ARCS) a = edge[4 * b + (j == 0 ? 0 : 1)] + Eb[0];
        else a = Eb[0];
    }
    if (on) Ab[0] = a;
    row[0][j + 1] = a;
    double e_next = (on && T > 1) ? Eb[lde_t] : 0.0;
    for (int t = 1; t < T; ++t) {
        __syncthreads();
        const double e = e_next;
        if (on && t + 1 < T) e_next = Eb[(size_t)(t + 1) * lde_t];
        const double* p = row[(t - 1) & 1];
        if (on) {
            if constexpr (ARCS) a = e + al_lse3(p[j + 1] + w0, p[j] + w1, sk >= 0 ? p[sk + 1] + w2 : al_ninf());
            else a = e + al_lse3(p[j + 1], p[j], sk >= 0 ? p[sk + 1] : al_ninf());
            Ab[(size_t)t * lda_t] = a;
        }
        row[t & 1][j + 1] = a;
    }
    __syncthreads();
    if (j == 0) {
        const double* p = row[(T - 1) & 1];
        if constexpr (ARCS) {
            const double last = p[J] + edge[4 * b + 2];
            loglik[b] = (e_alt >= 0 && e_alt < J - 1) ? al_lse2(p[e_alt + 1] + edge[4 * b + 3], last) : last;
        } else {
            const double last = p[J];
            loglik[b] = (e_alt >= 0 && e_alt < J - 1) ? al_lse2(p[e_alt + 1], last) : last;
        }
    }
}

// beta never leaves the chip: buffer row t holds E[t][k] + beta[t][k], what the predecessors of k add up.  Successors of state j
// are j, j + 1 and the one state whose skip predecessor is j (to[j], built in LDS from skip).  gamma may be written over alpha.
// ARCS: the successor arcs carry their costs (lane j keeps w[0][j], w[1][j + 1] and w[2][to[j]] for them) and beta[T - 1] is the end
// edge.  The arc posteriors xi[j][a] = sum_t exp(alpha[t - 1][pred_a(j)] + w[a][j] + E[t][j] + beta[t][j] - loglik) need the
// predecessors' alpha[t - 1]: in frame t every lane publishes the alpha[t][j] it prefetched a frame earlier in arow[t & 1][j + 1]
// (arow[.][0] = -inf, the "next" arc of state 0), beside row[t & 1][j], and in frame t - 1, after that frame's barrier, lane j adds
// the three terms of the transition into frame t + 1 from arow[t & 1] and from its own E + beta of frame t + 1, kept in a register
// (two frames back).  arow follows row's argument: frame t writes buffer t & 1 and reads buffer (t + 1) & 1, the barrier at the top of
// frame t orders frame t + 1's writes before these reads, the barrier at the top of frame t - 1 orders these reads before frame
// t - 1's overwrites of buffer (t + 1) & 1.  The last transition, into frame 1, is added after one more barrier behind the loop.  So
// xi is summed in descending t.  alpha[t][.] is read from memory by its own lane only, a frame before that lane writes gamma[t][.]:
// gamma over alpha stays legal.  Columns 3 and 4 of xi are gamma[0][j] and gamma[T - 1][j].
template <int NT, bool ARCS>
__global__ void __launch_bounds__(NT) align_backward_kernel(const double* __restrict__ E, long lde_b, long lde_t,
                                                            const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                            const int32_t* __restrict__ skip, long ldg, const int32_t* __restrict__ alt,
                                                            const double* __restrict__ w, long ldw, const double* __restrict__ edge,
                                                            const double* alpha, long lda_b, long lda_t,
                                                            const double* __restrict__ loglik, double* gamma, long ldo_b, long ldo_t,
                                                            double* __restrict__ xi, long ldx_b, long ldx_j, int Tmax, int Jmax) {
    __shared__ double row[2][NT + 1];
    __shared__ double arow[ARCS ? 2 : 1][ARCS ? NT + 1 : 1];
    __shared__ int to[NT];
    const int b = blockIdx.x, j = threadIdx.x, T = al_len(lens, b, Tmax), J = al_len(jlens, b, min(Jmax, NT));
    if (T == 0 || J == 0) return;
    const bool on = j < J;
    const int e_alt = alt[2 * b + 1];
    const double ll = loglik[b];
    int sk = on ? skip[(size_t)b * ldg + j] : -1;
    if (sk < 0 || sk >= J) sk = -1;
    to[j] = -1;
    row[0][j] = row[1][j] = al_ninf();                                     // states >= J stay -inf: the "next" arc of state J - 1
    if (j == 0) row[0][NT] = row[1][NT] = al_ninf();
    if constexpr (ARCS) {
        if (j == 0) arow[0][0] = arow[1][0] = al_ninf();
    }
    __syncthreads();
    if (sk >= 0) to[sk] = j;                                               // at most one state skips from sk
    __syncthreads();
    const int st = to[j];
    const double* Eb = E + (size_t)b * lde_b + j;
    const double* Ab = alpha + (size_t)b * lda_b + j;
    double* Gb = gamma + (size_t)b * ldo_b + j;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0, w1n = 0.0, w2s = 0.0;           // incoming self / next / skip, outgoing next / skip
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0, eb1 = al_ninf(), eb2 = al_ninf();
    double beta = (on && (j == J - 1 || j == e_alt)) ? 0.0 : al_ninf();
    if constexpr (ARCS) {
        if (on) {
            const double* Wb = w + (size_t)b * 3 * ldw;
            w0 = Wb[j];
            w1 = Wb[ldw + j];
            w2 = Wb[2 * ldw + j];
            if (j + 1 < J) w1n = Wb[ldw + j + 1];
            if (st >= 0) w2s = Wb[2 * ldw + st];
            if (j == J - 1 || j == e_alt) beta = edge[4 * b + (j == J - 1 ? 2 : 3)];
        }
    }
    if (on) {
        const double al = Ab[(size_t)(T - 1) * lda_t];
        const double g = exp(al + beta - ll);
        Gb[(size_t)(T - 1) * ldo_t] = g;
        const double eb = Eb[(size_t)(T - 1) * lde_t] + beta;
        row[(T - 1) & 1][j] = eb;
        if constexpr (ARCS) {
            x4 = g;
            if (T == 1) x3 = g;
            eb1 = eb;
        }
    }
    double e_next = 0.0, a_next = 0.0;
    if (on && T > 1) {
        e_next = Eb[(size_t)(T - 2) * lde_t];
        a_next = Ab[(size_t)(T - 2) * lda_t];
    }
    for (int t = T - 2; t >= 0; --t) {
        __syncthreads();
        const double e = e_next, al = a_next;
        if (on && t > 0) {
            e_next = Eb[(size_t)(t - 1) * lde_t];
            a_next = Ab[(size_t)(t - 1) * lda_t];
        }
        if (on) {
            const double* p = row[(t + 1) & 1];
            if constexpr (ARCS) {
                if (t + 2 < T) {                                           // the transition into frame t + 2: eb2 = (E + beta)[t + 2][j]
                    const double* pa = arow[(t + 1) & 1];
                    x0 += exp(pa[j + 1] + w0 + eb2 - ll);
                    x1 += exp(pa[j] + w1 + eb2 - ll);
                    if (sk >= 0) x2 += exp(pa[sk + 1] + w2 + eb2 - ll);
                }
                beta = al_lse3(p[j] + w0, p[j + 1] + w1n, st >= 0 ? p[st] + w2s : al_ninf());
            } else {
                beta = al_lse3(p[j], p[j + 1], st >= 0 ? p[st] : al_ninf());
            }
            const double g = exp(al + beta - ll);
            Gb[(size_t)t * ldo_t] = g;
            row[t & 1][j] = e + beta;
            if constexpr (ARCS) {
                arow[t & 1][j + 1] = al;
                eb2 = eb1;
                eb1 = e + beta;
                if (t == 0) x3 = g;
            }
        }
    }
    if constexpr (ARCS) {
        __syncthreads();
        if (on) {
            if (T > 1) {                                                   // the transition into frame 1: eb2 = (E + beta)[1][j]
                const double* pa = arow[0];
                x0 += exp(pa[j + 1] + w0 + eb2 - ll);
                x1 += exp(pa[j] + w1 + eb2 - ll);
                if (sk >= 0) x2 += exp(pa[sk + 1] + w2 + eb2 - ll);
            }
            double* X = xi + (size_t)b * ldx_b + (size_t)j * ldx_j;
            X[0] = x0;
            X[1] = x1;
            X[2] = x2;
            X[3] = x3;
            X[4] = x4;
        }
    }
}

// Backpointer code 0 self, 1 next, 2 skip; a later candidate replaces an earlier one only when strictly larger, so the lowest code
// wins ties; among the end states the lower index wins.  Only adds and compares of the oracle's operands: results are exact.
// ARCS: every candidate carries its arc cost, the start and end states their edge, as in align_forward_kernel.
template <int NT, bool ARCS>
__global__ void __launch_bounds__(NT) align_viterbi_kernel(const double* __restrict__ E, long lde_b, long lde_t,
                                                           const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                           const int32_t* __restrict__ skip, long ldg, const int32_t* __restrict__ alt,
                                                           const double* __restrict__ w, long ldw, const double* __restrict__ edge,
                                                           uint8_t* __restrict__ bp, long ldp_b, long ldp_t, int32_t* __restrict__ end,
                                                           double* __restrict__ score, int Tmax, int Jmax) {
    __shared__ double row[2][NT + 1];
    const int b = blockIdx.x, j = threadIdx.x, T = al_len(lens, b, Tmax), J = al_len(jlens, b, min(Jmax, NT));
    if (T == 0 || J == 0) {
        if (j == 0) {
            end[b] = -1;
            score[b] = al_ninf();
        }
        return;
    }
    const bool on = j < J;
    const int s_alt = alt[2 * b], e_alt = alt[2 * b + 1];
    int sk = on ? skip[(size_t)b * ldg + j] : -1;
    if (sk < 0 || sk >= J) sk = -1;
    const double* Eb = E + (size_t)b * lde_b + j;
    uint8_t* Pb = bp + (size_t)b * ldp_b + j;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if constexpr (ARCS) {
        if (on) {
            const double* Wb = w + (size_t)b * 3 * ldw + j;
            w0 = Wb[0];
            w1 = Wb[ldw];
            w2 = Wb[2 * ldw];
        }
    }
    if (j == 0) row[0][0] = row[1][0] = al_ninf();
    double a = al_ninf();
    if (on && (j == 0 || j == s_alt)) {
        if constexpr (ARCS) a = edge[4 * b + (j == 0 ? 0 : 1)] + Eb[0];
        else a = Eb[0];
    }
    if (on) Pb[0] = 0;
    row[0][j + 1] = a;
    double e_next = (on && T > 1) ? Eb[lde_t] : 0.0;
    for (int t = 1; t < T; ++t) {
        __syncthreads();
        const double e = e_next;
        if (on && t + 1 < T) e_next = Eb[(size_t)(t + 1) * lde_t];
        const double* p = row[(t - 1) & 1];
        if (on) {
            double best = ARCS ? p[j + 1] + w0 : p[j + 1];
            int code = 0;
            const double nx = ARCS ? p[j] + w1 : p[j];
            if (nx > best) { best = nx; code = 1; }
            if (sk >= 0) {
                const double sv = ARCS ? p[sk + 1] + w2 : p[sk + 1];
                if (sv > best) { best = sv; code = 2; }
            }
            a = e + best;
            Pb[(size_t)t * ldp_t] = (uint8_t)code;
        }
        row[t & 1][j + 1] = a;
    }
    __syncthreads();
    if (j == 0) {
        const double* p = row[(T - 1) & 1];
        int best_j = J - 1;
        if constexpr (ARCS) {
            double best = p[J] + edge[4 * b + 2];
            if (e_alt >= 0 && e_alt < J - 1 && p[e_alt + 1] + edge[4 * b + 3] >= best) {
                best_j = e_alt;
                best = p[e_alt + 1] + edge[4 * b + 3];
            }
            end[b] = best_j;
            score[b] = best;
        } else {
            double best = p[J];
            if (e_alt >= 0 && e_alt < J - 1 && p[e_alt + 1] >= best) {
                best_j = e_alt;
                best = p[e_alt + 1];
            }
            end[b] = best_j;
            score[b] = best;
        }
    }
}

#define AL_SCAN_ARGS(name)                                                                                                         \
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && Jmax >= 0 && lde_t >= Jmax && lde_b >= (long)Tmax * lde_t && ldg >= Jmax,                \
                  name ": bad shape B=%d Tmax=%d Jmax=%d lde_b=%ld lde_t=%ld ldg=%ld", B, Tmax, Jmax, lde_b, lde_t, ldg);          \
    FS2_CHECK_ARG(Jmax <= AL_MAX_STATES, name ": %d states exceed the supported maximum of %d", Jmax, AL_MAX_STATES)

extern "C" int fs2_align_max_states(void) { return AL_MAX_STATES; }

extern "C" int fs2_align_forward(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                 const int32_t* skip, long ldg, const int32_t* alt, double* alpha, long lda_b, long lda_t,
                                 double* loglik, int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && alpha && loglik, "align_forward: null pointer");
    AL_SCAN_ARGS("align_forward");
    FS2_CHECK_ARG(lda_t >= Jmax && lda_b >= (long)Tmax * lda_t, "align_forward: bad alpha strides %ld %ld", lda_b, lda_t);
    if (B == 0) return FS2_OK;
#define AL_FWD(NT, ARCS, w, ldw, edge)                                                                                             \
    align_forward_kernel<NT, ARCS><<<B, NT, 0, stream>>>(E, lde_b, lde_t, lens, jlens, skip, ldg, alt, w, ldw, edge, alpha, lda_b,  \
                                                         lda_t, loglik, Tmax, Jmax)
    if (Jmax <= 256) AL_FWD(256, false, nullptr, 0, nullptr); else if (Jmax <= 512) AL_FWD(512, false, nullptr, 0, nullptr);
    else AL_FWD(1024, false, nullptr, 0, nullptr);
    FS2_CHECK_LAUNCH("align_forward");
    return FS2_OK;
}

// The scans with arc costs: w [B][3][ldw] (self, next, skip into state j), edge [B][4] (start in 0, start in alt[0], end in J - 1,
// end in alt[1]); everything else as above.
#define AL_ARC_ARGS(name)                                                                                                          \
    FS2_CHECK_ARG(w && edge, name ": null arc costs");                                                                            \
    FS2_CHECK_ARG(ldw >= Jmax, name ": bad arc cost stride %ld for %d states", ldw, Jmax)

extern "C" int fs2_align_forward_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                      const int32_t* skip, long ldg, const int32_t* alt, const double* w, long ldw, const double* edge,
                                      double* alpha, long lda_b, long lda_t, double* loglik, int B, int Tmax, int Jmax,
                                      hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && alpha && loglik, "align_forward_arcs: null pointer");
    AL_SCAN_ARGS("align_forward_arcs");
    AL_ARC_ARGS("align_forward_arcs");
    FS2_CHECK_ARG(lda_t >= Jmax && lda_b >= (long)Tmax * lda_t, "align_forward_arcs: bad alpha strides %ld %ld", lda_b, lda_t);
    if (B == 0) return FS2_OK;
    if (Jmax <= 256) AL_FWD(256, true, w, ldw, edge); else if (Jmax <= 512) AL_FWD(512, true, w, ldw, edge);
    else AL_FWD(1024, true, w, ldw, edge);
#undef AL_FWD
    FS2_CHECK_LAUNCH("align_forward_arcs");
    return FS2_OK;
}

extern "C" int fs2_align_backward(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                  const int32_t* skip, long ldg, const int32_t* alt, const double* alpha, long lda_b, long lda_t,
                                  const double* loglik, double* gamma, long ldo_b, long ldo_t, int B, int Tmax, int Jmax,
                                  hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && alpha && loglik && gamma, "align_backward: null pointer");
    AL_SCAN_ARGS("align_backward");
    FS2_CHECK_ARG(lda_t >= Jmax && lda_b >= (long)Tmax * lda_t && ldo_t >= Jmax && ldo_b >= (long)Tmax * ldo_t,
                  "align_backward: bad alpha / gamma strides %ld %ld %ld %ld", lda_b, lda_t, ldo_b, ldo_t);
    FS2_CHECK_ARG(gamma != alpha || (lda_b == ldo_b && lda_t == ldo_t), "align_backward: gamma over alpha needs equal strides");
    if (B == 0) return FS2_OK;
#define AL_BWD(NT, ARCS, w, ldw, edge, xi, ldx_b, ldx_j)                                                                           \
    align_backward_kernel<NT, ARCS><<<B, NT, 0, stream>>>(E, lde_b, lde_t, lens, jlens, skip, ldg, alt, w, ldw, edge, alpha, lda_b, \
                                                          lda_t, loglik, gamma, ldo_b, ldo_t, xi, ldx_b, ldx_j, Tmax, Jmax)
    if (Jmax <= 256) AL_BWD(256, false, nullptr, 0, nullptr, nullptr, 0, 0);
    else if (Jmax <= 512) AL_BWD(512, false, nullptr, 0, nullptr, nullptr, 0, 0);
    else AL_BWD(1024, false, nullptr, 0, nullptr, nullptr, 0, 0);
    FS2_CHECK_LAUNCH("align_backward");
    return FS2_OK;
}

// xi [B][Jmax][5] (strides ldx_b, ldx_j): the arc posteriors self, next, skip summed in descending t, then gamma[0][j], gamma[T - 1][j]
extern "C" int fs2_align_backward_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                       const int32_t* skip, long ldg, const int32_t* alt, const double* w, long ldw,
                                       const double* edge, const double* alpha, long lda_b, long lda_t, const double* loglik,
                                       double* gamma, long ldo_b, long ldo_t, double* xi, long ldx_b, long ldx_j, int B, int Tmax,
                                       int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && alpha && loglik && gamma && xi, "align_backward_arcs: null pointer");
    AL_SCAN_ARGS("align_backward_arcs");
    AL_ARC_ARGS("align_backward_arcs");
    FS2_CHECK_ARG(lda_t >= Jmax && lda_b >= (long)Tmax * lda_t && ldo_t >= Jmax && ldo_b >= (long)Tmax * ldo_t,
                  "align_backward_arcs: bad alpha / gamma strides %ld %ld %ld %ld", lda_b, lda_t, ldo_b, ldo_t);
    FS2_CHECK_ARG(gamma != alpha || (lda_b == ldo_b && lda_t == ldo_t), "align_backward_arcs: gamma over alpha needs equal strides");
    FS2_CHECK_ARG(ldx_j >= 5 && ldx_b >= (long)Jmax * ldx_j, "align_backward_arcs: bad xi strides %ld %ld", ldx_b, ldx_j);
    if (B == 0) return FS2_OK;
    if (Jmax <= 256) AL_BWD(256, true, w, ldw, edge, xi, ldx_b, ldx_j);
    else if (Jmax <= 512) AL_BWD(512, true, w, ldw, edge, xi, ldx_b, ldx_j);
    else AL_BWD(1024, true, w, ldw, edge, xi, ldx_b, ldx_j);
#undef AL_BWD
    FS2_CHECK_LAUNCH("align_backward_arcs");
    return FS2_OK;
}

extern "C" int fs2_align_viterbi(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                 const int32_t* skip, long ldg, const int32_t* alt, uint8_t* bp, long ldp_b, long ldp_t, int32_t* end,
                                 double* score, int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && bp && end && score, "align_viterbi: null pointer");
    AL_SCAN_ARGS("align_viterbi");
    FS2_CHECK_ARG(ldp_t >= Jmax && ldp_b >= (long)Tmax * ldp_t, "align_viterbi: bad backpointer strides %ld %ld", ldp_b, ldp_t);
    if (B == 0) return FS2_OK;
#define AL_VIT(NT, ARCS, w, ldw, edge)                                                                                             \
    align_viterbi_kernel<NT, ARCS><<<B, NT, 0, stream>>>(E, lde_b, lde_t, lens, jlens, skip, ldg, alt, w, ldw, edge, bp, ldp_b, ldp_t, \
                                                         end, score, Tmax, Jmax)
    if (Jmax <= 256) AL_VIT(256, false, nullptr, 0, nullptr); else if (Jmax <= 512) AL_VIT(512, false, nullptr, 0, nullptr);
    else AL_VIT(1024, false, nullptr, 0, nullptr);
    FS2_CHECK_LAUNCH("align_viterbi");
    return FS2_OK;
}

extern "C" int fs2_align_viterbi_arcs(const double* E, long lde_b, long lde_t, const int32_t* lens, const int32_t* jlens,
                                      const int32_t* skip, long ldg, const int32_t* alt, const double* w, long ldw, const double* edge,
                                      uint8_t* bp, long ldp_b, long ldp_t, int32_t* end, double* score, int B, int Tmax, int Jmax,
                                      hipStream_t stream) {
    FS2_CHECK_ARG(E && lens && jlens && skip && alt && bp && end && score, "align_viterbi_arcs: null pointer");
    AL_SCAN_ARGS("align_viterbi_arcs");
    AL_ARC_ARGS("align_viterbi_arcs");
    FS2_CHECK_ARG(ldp_t >= Jmax && ldp_b >= (long)Tmax * ldp_t, "align_viterbi_arcs: bad backpointer strides %ld %ld", ldp_b, ldp_t);
    if (B == 0) return FS2_OK;
    if (Jmax <= 256) AL_VIT(256, true, w, ldw, edge); else if (Jmax <= 512) AL_VIT(512, true, w, ldw, edge);
    else AL_VIT(1024, true, w, ldw, edge);
#undef AL_VIT
    FS2_CHECK_LAUNCH("align_viterbi_arcs");
    return FS2_OK;
}

// ------------------------------------------------------------------ backtrack
// One lane per utterance walks its T backpointers from the end state; the path is monotone in the block index, so frames per block
// are run lengths.  Rows of `frames` are zero-filled up to nbmax first (a skipped optional block keeps 0).
__global__ void align_backtrack_kernel(const uint8_t* __restrict__ bp, long ldp_b, long ldp_t, const int32_t* __restrict__ lens,
                                       const int32_t* __restrict__ jlens, const int32_t* __restrict__ skip,
                                       const int32_t* __restrict__ block, long ldg, const int32_t* __restrict__ end,
                                       int32_t* __restrict__ frames, int nbmax, int B, int Tmax, int Jmax) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int32_t* fr = frames + (size_t)b * nbmax;
    for (int k = 0; k < nbmax; ++k) fr[k] = 0;
    const int T = al_len(lens, b, Tmax), J = al_len(jlens, b, Jmax);
    int j = end[b];
    if (T == 0 || j < 0 || j >= J) return;
    const uint8_t* P = bp + (size_t)b * ldp_b;
    const int32_t* sk = skip + (size_t)b * ldg;
    const int32_t* bl = block + (size_t)b * ldg;
    int cur = bl[j], cnt = 0;
    for (int t = T - 1; t >= 0; --t) {
        const int k = bl[j];
        if (k != cur) {
            if (cur >= 0 && cur < nbmax) fr[cur] = cnt;
            cur = k;
            cnt = 0;
        }
        ++cnt;
        if (t > 0) {
            const int code = P[(size_t)t * ldp_t + j];
            const int nj = code == 0 ? j : (code == 1 ? j - 1 : sk[j]);
            if (nj < 0 || nj >= J) break;                                   // not a path of this graph: stop rather than read outside
            j = nj;
        }
    }
    if (cur >= 0 && cur < nbmax) fr[cur] = cnt;
}
extern "C" int fs2_align_backtrack(const uint8_t* bp, long ldp_b, long ldp_t, const int32_t* lens, const int32_t* jlens,
                                   const int32_t* skip, const int32_t* block, long ldg, const int32_t* end, int32_t* frames,
                                   int nbmax, int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(bp && lens && jlens && skip && block && end && frames, "align_backtrack: null pointer");
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0 && Jmax >= 0 && nbmax >= 0 && ldp_t >= Jmax && ldp_b >= (long)Tmax * ldp_t && ldg >= Jmax,
                  "align_backtrack: bad shape B=%d Tmax=%d Jmax=%d nbmax=%d", B, Tmax, Jmax, nbmax);
    FS2_CHECK_ARG(Jmax <= AL_MAX_STATES, "align_backtrack: %d states exceed the supported maximum of %d", Jmax, AL_MAX_STATES);
    if (B == 0) return FS2_OK;
    align_backtrack_kernel<<<fs2_cdiv(B, 64), 64, 0, stream>>>(bp, ldp_b, ldp_t, lens, jlens, skip, block, ldg, end, frames, nbmax, B,
                                                             Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_backtrack");
    return FS2_OK;
}

// ------------------------------------------------------------------ statistics
// P[b][j][0] = sum_t g, P[b][j][1 + d] = sum_t g x_d, P[b][j][1 + D + d] = sum_t g x_d^2, with g = gamma[b][t][j], in ascending t.
// Lane (dd = tid & 31, jg = tid >> 5) owns dimension d0 + dd of states j0 + jg + 8 q, q < 4.
__global__ void __launch_bounds__(256) align_stats_kernel(const double* __restrict__ gamma, long ldo_b, long ldo_t,
                                                          const double* __restrict__ x, long ldx_b, long ldx_t,
                                                          const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens, int D,
                                                          double* __restrict__ P, long ldp_b, long ldp_j, int Tmax, int Jmax) {
    __shared__ double gs[AL_TILE][AL_TILE + 1], xs[AL_TILE][AL_TILE + 1];
    const int b = blockIdx.z, T = al_len(lens, b, Tmax), J = al_len(jlens, b, Jmax);
    const int d0 = blockIdx.x * AL_TILE, j0 = blockIdx.y * AL_TILE, tid = threadIdx.x;
    if (j0 >= J) return;
    const int dd = tid & 31, jg = tid >> 5;
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const double* gb = gamma + (size_t)b * ldo_b;
    const double* xb = x + (size_t)b * ldx_b;
    for (int t0 = 0; t0 < T; t0 += AL_TILE) {
        __syncthreads();
        for (int k = tid; k < AL_TILE * AL_TILE; k += 256) {
            const int r = k >> 5, c = k & 31, t = t0 + r;
            gs[r][c] = (t < T && j0 + c < J) ? gb[(size_t)t * ldo_t + j0 + c] : 0.0;
            xs[r][c] = (t < T && d0 + c < D) ? xb[(size_t)t * ldx_t + d0 + c] : 0.0;
        }
        __syncthreads();
        const int n = min(AL_TILE, T - t0);
        for (int r = 0; r < n; ++r) {
            const double xv = xs[r][dd], x2 = xv * xv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double g = gs[r][jg + 8 * q];
                s0[q] += g;
                s1[q] += g * xv;
                s2[q] += g * x2;
            }
        }
    }
    const int d = d0 + dd;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + jg + 8 * q;
        if (j >= J) continue;
        double* pr = P + (size_t)b * ldp_b + (size_t)j * ldp_j;
        if (blockIdx.x == 0 && dd == 0) pr[0] = s0[q];
        if (d < D) {
            pr[1 + d] = s1[q];
            pr[1 + D + d] = s2[q];
        }
    }
}
extern "C" int fs2_align_stats(const double* gamma, long ldo_b, long ldo_t, const double* x, long ldx_b, long ldx_t, const int32_t* lens,
                               const int32_t* jlens, int D, double* partials, long ldp_b, long ldp_j, int B, int Tmax, int Jmax,
                               hipStream_t stream) {
    FS2_CHECK_ARG(gamma && x && lens && jlens && partials, "align_stats: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Jmax >= 0 && D > 0 && ldo_t >= Jmax && ldo_b >= (long)Tmax * ldo_t && ldx_t >= D &&
                      ldx_b >= (long)Tmax * ldx_t && ldp_j >= 1 + 2 * D && ldp_b >= (long)Jmax * ldp_j,
                  "align_stats: bad shape B=%d Tmax=%d Jmax=%d D=%d", B, Tmax, Jmax, D);
    FS2_CHECK_ARG(Jmax <= AL_MAX_STATES, "align_stats: %d states exceed the supported maximum of %d", Jmax, AL_MAX_STATES);
    if (B == 0 || Jmax == 0) return FS2_OK;
    align_stats_kernel<<<dim3(fs2_cdiv(D, AL_TILE), fs2_cdiv(Jmax, AL_TILE), B), 256, 0, stream>>>(
        gamma, ldo_b, ldo_t, x, ldx_b, ldx_t, lens, jlens, D, partials, ldp_b, ldp_j, Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_stats");
    return FS2_OK;
}

// The mixture statistics: rows are (j, m) = row / M, row % M, up to 8 x 1024 of them, and g = gamma[b][t][j] resp[b][t][j][m] is
// formed while a frame block is staged, so no product of the two ever lies in HBM.  A lane stages the same row of every frame
// (k & 31 = tid & 31), so its (j, m) is computed once.  Tiles, lane map and the ascending-t sums are align_stats_kernel's.
__global__ void __launch_bounds__(256) align_stats_gmm_kernel(const double* __restrict__ gamma, long ldo_b, long ldo_t,
                                                              const double* __restrict__ resp, long ldr_b, long ldr_t, long ldr_j,
                                                              const double* __restrict__ x, long ldx_b, long ldx_t,
                                                              const int32_t* __restrict__ lens, const int32_t* __restrict__ jlens,
                                                              int M, int D, double* __restrict__ P, long ldp_b, long ldp_r, int Tmax,
                                                              int Jmax) {
    __shared__ double gs[AL_TILE][AL_TILE + 1], xs[AL_TILE][AL_TILE + 1];
    const int b = blockIdx.z, T = al_len(lens, b, Tmax), J = al_len(jlens, b, Jmax), R = J * M;
    const int d0 = blockIdx.x * AL_TILE, r0 = blockIdx.y * AL_TILE, tid = threadIdx.x;
    if (r0 >= R) return;
    const int dd = tid & 31, jg = tid >> 5;
    const int srow = r0 + dd, sj = srow / M, sm = srow - sj * M;           // the row this lane stages
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const double* gb = gamma + (size_t)b * ldo_b + sj;
    const double* rb = resp + (size_t)b * ldr_b + (size_t)sj * ldr_j + sm;
    const double* xb = x + (size_t)b * ldx_b;
    for (int t0 = 0; t0 < T; t0 += AL_TILE) {
        __syncthreads();
        for (int k = tid; k < AL_TILE * AL_TILE; k += 256) {
            const int r = k >> 5, t = t0 + r;
            gs[r][dd] = (t < T && srow < R) ? gb[(size_t)t * ldo_t] * rb[(size_t)t * ldr_t] : 0.0;
            xs[r][dd] = (t < T && d0 + dd < D) ? xb[(size_t)t * ldx_t + d0 + dd] : 0.0;
        }
        __syncthreads();
        const int n = min(AL_TILE, T - t0);
        for (int r = 0; r < n; ++r) {
            const double xv = xs[r][dd], x2 = xv * xv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double g = gs[r][jg + 8 * q];
                s0[q] += g;
                s1[q] += g * xv;
                s2[q] += g * x2;
            }
        }
    }
    const int d = d0 + dd;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = r0 + jg + 8 * q;
        if (row >= R) continue;
        double* pr = P + (size_t)b * ldp_b + (size_t)row * ldp_r;
        if (blockIdx.x == 0 && dd == 0) pr[0] = s0[q];
        if (d < D) {
            pr[1 + d] = s1[q];
            pr[1 + D + d] = s2[q];
        }
    }
}
extern "C" int fs2_align_stats_gmm(const double* gamma, long ldo_b, long ldo_t, const double* resp, long ldr_b, long ldr_t, long ldr_j,
                                   const double* x, long ldx_b, long ldx_t, const int32_t* lens, const int32_t* jlens, int M, int D,
                                   double* partials, long ldp_b, long ldp_r, int B, int Tmax, int Jmax, hipStream_t stream) {
    FS2_CHECK_ARG(gamma && resp && x && lens && jlens && partials, "align_stats_gmm: null pointer");
    FS2_CHECK_ARG(M >= 1 && M <= AL_MAX_MIX, "align_stats_gmm: %d mixture components, supported are 1..%d", M, AL_MAX_MIX);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && Jmax >= 0 && D > 0 && ldo_t >= Jmax && ldo_b >= (long)Tmax * ldo_t && ldx_t >= D &&
                      ldx_b >= (long)Tmax * ldx_t && ldp_r >= 1 + 2 * D && ldp_b >= (long)Jmax * M * ldp_r && ldr_j >= M &&
                      ldr_t >= (long)Jmax * ldr_j && ldr_b >= (long)Tmax * ldr_t,
                  "align_stats_gmm: bad shape B=%d Tmax=%d Jmax=%d M=%d D=%d", B, Tmax, Jmax, M, D);
    FS2_CHECK_ARG((long)Jmax * M <= (long)AL_MAX_STATES * AL_MAX_MIX, "align_stats_gmm: %ld rows exceed the supported maximum of %d",
                  (long)Jmax * M, AL_MAX_STATES * AL_MAX_MIX);
    if (B == 0 || Jmax == 0) return FS2_OK;
    align_stats_gmm_kernel<<<dim3(fs2_cdiv(D, AL_TILE), fs2_cdiv(Jmax * M, AL_TILE), B), 256, 0, stream>>>(
        gamma, ldo_b, ldo_t, resp, ldr_b, ldr_t, ldr_j, x, ldx_b, ldx_t, lens, jlens, M, D, partials, ldp_b, ldp_r, Tmax, Jmax);
    FS2_CHECK_LAUNCH("align_stats_gmm");
    return FS2_OK;
}

// sums[c][col] (+)= partial rows items[offs[c] .. offs[c + 1]) added in list order; rows index partials as [n_rows][ldp_j]
__global__ void align_reduce_kernel(const double* __restrict__ P, long ldp_j, long n_rows, const int32_t* __restrict__ offs,
                                    const int32_t* __restrict__ items, int cols, double* __restrict__ sums, int accumulate) {
    const int c = blockIdx.y, col = blockIdx.x * 64 + threadIdx.x;
    if (col >= cols) return;
    double acc = accumulate ? sums[(size_t)c * cols + col] : 0.0;
    const int i1 = offs[c + 1];
    for (int i = offs[c]; i < i1; ++i) {
        const long r = items[i];
        if (r >= 0 && r < n_rows) acc += P[(size_t)r * ldp_j + col];
    }
    sums[(size_t)c * cols + col] = acc;
}
extern "C" int fs2_align_reduce(const double* partials, long ldp_j, long n_rows, const int32_t* offs, const int32_t* items,
                                int n_classes, int cols, double* sums, int accumulate, hipStream_t stream) {
    FS2_CHECK_ARG(partials && offs && items && sums, "align_reduce: null pointer");
    FS2_CHECK_ARG(n_classes >= 0 && n_classes <= 65535 && cols > 0 && ldp_j >= cols && n_rows >= 0,
                  "align_reduce: bad shape classes=%d cols=%d ldp_j=%ld rows=%ld", n_classes, cols, ldp_j, n_rows);
    if (n_classes == 0) return FS2_OK;
    align_reduce_kernel<<<dim3(fs2_cdiv(cols, 64), n_classes), 64, 0, stream>>>(partials, ldp_j, n_rows, offs, items, cols, sums,
                                                                                accumulate);
    FS2_CHECK_LAUNCH("align_reduce");
    return FS2_OK;
}
