// fs2_stoi.hip — short-time objective intelligibility (STOI, Taal et al. 2011) and its extended form (ESTOI, Jensen & Taal 2016) of
// ragged batches of time-aligned pairs at 10 kHz.  The specification is the docstring of fastspeech2_amd/stoi.py (mirrored in
// DESIGN.md); tests/stoi_ref.py restates it in numpy.  Everything after the float32 load is fp64.
//
// The constants are the papers': frames of ST_N = 256 samples at hop ST_H = 128, zero-padded to ST_K = 512 for the transform,
// ST_J = 15 one-third octave bands, segments of ST_L = 30 frames.  The framing rule, used twice: frame starts s = 0, H, 2H, .. with
// s < len - N, so ST_FRAMES(len) = ceil((len - N) / H) for len > N and 0 otherwise.  One kernel per concern:
//
//   stoi_energy_kernel    one wave per frame of the clean row: e[j] = sum_n (x[s_j + n] w[n])^2
//   stoi_keep_kernel      one workgroup per row: the maximum of e, the keep mask e[j] > 1e-4 max (and max > 0), and the compaction
//                         map of the kept frames by an ordered integer scan: map[i] = the frame that becomes frame i
//   stoi_ola_kernel       both signals, one thread per output sample: a GATHER of the at most two kept frames that cover it, in
//                         ascending frame order, through the map; len' = (n_kept - 1) H + N
//   stoi_bands_kernel     one workgroup per frame of the compacted signal: window, direct DFT of the bins the bands use against an
//                         LDS copy of the caller's twiddle table (no sine is evaluated here), power, 15 band magnitudes
//   stoi_segment_kernel   one workgroup per (row, segment): the 2 x 15 x 30 values in LDS, both segment scores
//   stoi_mean_kernel      one workgroup per row: the ordered mean of the segment scores and the row's counts
//
// No atomics and no order that depends on timing: the same input gives the same bytes.  Samples at or beyond lens[b] are never
// loaded (a row's padding may hold anything).  Every count read back from device memory (n_kept, map) is clamped to its buffer
// before it is used as an index.
#include "fs2_common.h"

#define ST_N 256
#define ST_H 128
#define ST_K 512
#define ST_J 15
#define ST_L 30
#define ST_EPS 2.220446049250313e-16            // 2^-52
#define ST_FRAMES(len) ((len) > ST_N ? ((len) - ST_N + ST_H - 1) / ST_H : 0)

static __device__ __forceinline__ int st_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }
static __device__ __forceinline__ int st_kept(const int32_t* n_kept, int b, int cap) { return min(max(n_kept[b], 0), cap); }
static __device__ __forceinline__ double st_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ------------------------------------------------------------------ frame energies
__global__ void __launch_bounds__(256) stoi_energy_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ lens,
                                                          const double* __restrict__ w, double* __restrict__ e, long lde, int Nmax) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int F = ST_FRAMES(st_len(lens, b, Nmax));
    if (j >= F) return;                                                 // wave-uniform
    const float* xr = x + (size_t)b * ldx + (size_t)j * ST_H;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < ST_N / 64; ++q) {
        const int n = q * 64 + lane;
        const double v = (double)xr[n] * w[n];
        acc = fma(v, v, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) e[(size_t)b * lde + j] = acc;
}
extern "C" int fs2_stoi_frame_energy(const float* x, long ldx, const int32_t* lens, const double* w, double* e, long lde, int B,
                                     int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && w, "stoi_frame_energy: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldx >= Nmax, "stoi_frame_energy: bad shape B=%d Nmax=%d ldx=%ld", B, Nmax, ldx);
    const int Fmax = ST_FRAMES(Nmax);
    FS2_CHECK_ARG(Fmax == 0 || (e && lde >= Fmax), "stoi_frame_energy: e must hold %d frames per row (lde=%ld)", Fmax, lde);
    if (B == 0 || Fmax == 0) return FS2_OK;
    stoi_energy_kernel<<<dim3(fs2_cdiv(Fmax, 4), B), 256, 0, stream>>>(x, ldx, lens, w, e, lde, Nmax);
    FS2_CHECK_LAUNCH("stoi_frame_energy");
    return FS2_OK;
}

// ------------------------------------------------------------------ keep mask and compaction map
__global__ void __launch_bounds__(256) stoi_keep_kernel(const double* __restrict__ e, long lde, const int32_t* __restrict__ lens,
                                                        int32_t* __restrict__ mask, int32_t* __restrict__ map, long ldm,
                                                        int32_t* __restrict__ n_kept, int Nmax) {
    __shared__ double red[4];
    __shared__ int cnt[256];
    const int b = blockIdx.x, tid = threadIdx.x, F = ST_FRAMES(st_len(lens, b, Nmax));
    if (F == 0) {
        if (tid == 0) n_kept[b] = 0;
        return;
    }
    const double* er = e + (size_t)b * lde;
    double m = 0.0;                                                     // energies are >= 0; the maximum is exact in any order
    for (int j = tid; j < F; j += 256) m = fmax(m, er[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const double thr = 1e-4 * m;
    // thread t owns the frames [t C, (t + 1) C): counts, an inclusive scan of the counts, then the ordered writes
    const int C = (F + 255) / 256, j0 = min(tid * C, F), j1 = min(j0 + C, F);
    int c = 0;
    for (int j = j0; j < j1; ++j) c += (m > 0.0 && er[j] > thr) ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = tid >= o ? cnt[tid - o] : 0;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    int i = cnt[tid] - c;
    for (int j = j0; j < j1; ++j) {
        const int k = (m > 0.0 && er[j] > thr) ? 1 : 0;
        mask[(size_t)b * ldm + j] = k;
        if (k) map[(size_t)b * ldm + i++] = j;
    }
    if (tid == 255) n_kept[b] = cnt[255];
}
extern "C" int fs2_stoi_keep(const double* e, long lde, const int32_t* lens, int32_t* mask, int32_t* map, long ldm, int32_t* n_kept,
                             int B, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(lens && n_kept, "stoi_keep: null pointer");
    FS2_CHECK_ARG(B >= 0 && Nmax >= 0, "stoi_keep: bad shape B=%d Nmax=%d", B, Nmax);
    const int Fmax = ST_FRAMES(Nmax);
    FS2_CHECK_ARG(Fmax == 0 || (e && mask && map && lde >= Fmax && ldm >= Fmax),
                  "stoi_keep: e, mask and map must hold %d frames per row (lde=%ld ldm=%ld)", Fmax, lde, ldm);
    if (B == 0) return FS2_OK;
    stoi_keep_kernel<<<B, 256, 0, stream>>>(e, lde, lens, mask, map, ldm, n_kept, Nmax);
    FS2_CHECK_LAUNCH("stoi_keep");
    return FS2_OK;
}

// ------------------------------------------------------------------ overlap-add of the kept frames, as a gather
__global__ void __launch_bounds__(256) stoi_ola_kernel(const float* __restrict__ x, const float* __restrict__ y, long ldx,
                                                       const int32_t* __restrict__ lens, const double* __restrict__ w,
                                                       const int32_t* __restrict__ map, long ldm, const int32_t* __restrict__ n_kept,
                                                       double* __restrict__ xo, double* __restrict__ yo, long ldo, int Nmax) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int F = ST_FRAMES(st_len(lens, b, Nmax)), nk = st_kept(n_kept, b, F);
    if (nk == 0 || t >= (nk - 1) * ST_H + ST_N) return;
    const int i1 = t / ST_H;
    double ax = 0.0, ay = 0.0;
#pragma unroll
    for (int i = i1 - 1; i <= i1; ++i) {                                // ascending frame order, as the scatter loop adds them
        if (i < 0 || i >= nk) continue;
        const int j = min(max(map[(size_t)b * ldm + i], 0), F - 1), n = t - i * ST_H;
        const size_t at = (size_t)b * ldx + (size_t)j * ST_H + n;       // j H + n <= (F - 1) H + N - 1 < len
        ax += (double)x[at] * w[n];
        ay += (double)y[at] * w[n];
    }
    xo[(size_t)b * ldo + t] = ax;
    yo[(size_t)b * ldo + t] = ay;
}
extern "C" int fs2_stoi_ola(const float* x, const float* y, long ldx, const int32_t* lens, const double* w, const int32_t* map, long ldm,
                            const int32_t* n_kept, double* xo, double* yo, long ldo, int B, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && y && lens && w && n_kept, "stoi_ola: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldx >= Nmax, "stoi_ola: bad shape B=%d Nmax=%d ldx=%ld", B, Nmax, ldx);
    const int Fmax = ST_FRAMES(Nmax);
    const long Lmax = Fmax ? (long)(Fmax - 1) * ST_H + ST_N : 0;
    FS2_CHECK_ARG(Fmax == 0 || (map && xo && yo && ldm >= Fmax && ldo >= Lmax),
                  "stoi_ola: map must hold %d frames and xo, yo %ld samples per row (ldm=%ld ldo=%ld)", Fmax, Lmax, ldm, ldo);
    if (B == 0 || Fmax == 0) return FS2_OK;
    stoi_ola_kernel<<<dim3(fs2_cdiv(Lmax, 256), B), 256, 0, stream>>>(x, y, ldx, lens, w, map, ldm, n_kept, xo, yo, ldo, Nmax);
    FS2_CHECK_LAUNCH("stoi_ola");
    return FS2_OK;
}

// ------------------------------------------------------------------ framed DFT -> 15 band magnitudes
struct StEdges { int e[ST_J + 1]; };

__global__ void __launch_bounds__(256) stoi_bands_kernel(const double* __restrict__ xo, long ldo, const int32_t* __restrict__ n_kept,
                                                         const double* __restrict__ w, const double* __restrict__ twiddle, StEdges ed,
                                                         double* __restrict__ X, long ldx_b, long ldx_k, int Fmax) {
    __shared__ double f[ST_N];
    __shared__ double2 tw[ST_K];
    __shared__ double pw[256];
    const int b = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
    if (m >= st_kept(n_kept, b, Fmax) - 1) return;                      // M = n_kept - 1 frames
    f[tid] = xo[(size_t)b * ldo + (size_t)m * ST_H + tid] * w[tid];
    tw[tid] = reinterpret_cast<const double2*>(twiddle)[tid];
    tw[tid + 256] = reinterpret_cast<const double2*>(twiddle)[tid + 256];
    __syncthreads();
    const int k0 = ed.e[0], k = k0 + tid;
    if (k < ed.e[ST_J]) {
        // bin k of the frame zero-padded to 512: four interleaved partial sums, each ascending in n, added pairwise
        double re[4] = {0.0, 0.0, 0.0, 0.0}, im[4] = {0.0, 0.0, 0.0, 0.0};
        for (int n = 0; n < ST_N; n += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double2 c = tw[(k * (n + q)) & (ST_K - 1)];
                re[q] = fma(f[n + q], c.x, re[q]);
                im[q] = fma(f[n + q], c.y, im[q]);
            }
        }
        const double r = (re[0] + re[1]) + (re[2] + re[3]), i = (im[0] + im[1]) + (im[2] + im[3]);
        pw[tid] = r * r + i * i;
    }
    __syncthreads();
    if (tid < ST_J) {
        double s = 0.0;
        for (int q = ed.e[tid]; q < ed.e[tid + 1]; ++q) s += pw[q - k0];
        X[(size_t)b * ldx_b + (size_t)tid * ldx_k + m] = sqrt(s);
    }
}
extern "C" int fs2_stoi_bands(const double* xo, long ldo, const int32_t* n_kept, const double* w, const double* twiddle,
                              const int32_t* edges, double* X, long ldx_b, long ldx_k, int B, int Fmax, hipStream_t stream) {
    FS2_CHECK_ARG(n_kept && w && twiddle && edges, "stoi_bands: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Fmax >= 0 && Fmax <= (1 << 23), "stoi_bands: bad shape B=%d Fmax=%d", B, Fmax);
    StEdges ed;                                                         // edges is HOST memory: the 16 bins travel as a kernel argument
    for (int k = 0; k <= ST_J; ++k) ed.e[k] = edges[k];
    bool ok = ed.e[0] >= 0 && ed.e[ST_J] <= ST_K / 2 + 1 && ed.e[ST_J] - ed.e[0] <= 256;
    for (int k = 0; k < ST_J; ++k) ok = ok && ed.e[k] <= ed.e[k + 1];
    FS2_CHECK_ARG(ok, "stoi_bands: the band edges must ascend within [0, %d] and span at most 256 bins", ST_K / 2 + 1);
    const int Mmax = Fmax > 0 ? Fmax - 1 : 0;
    const long Lmax = Fmax ? (long)(Fmax - 1) * ST_H + ST_N : 0;
    FS2_CHECK_ARG(Mmax == 0 || (xo && X && ldo >= Lmax && ldx_k >= Mmax && ldx_b >= ST_J * ldx_k),
                  "stoi_bands: xo must hold %ld samples and X 15 x %d magnitudes per row (ldo=%ld ldx_b=%ld ldx_k=%ld)", Lmax, Mmax, ldo,
                  ldx_b, ldx_k);
    if (B == 0 || Mmax == 0) return FS2_OK;
    stoi_bands_kernel<<<dim3(Mmax, B), 256, 0, stream>>>(xo, ldo, n_kept, w, twiddle, ed, X, ldx_b, ldx_k, Fmax);
    FS2_CHECK_LAUNCH("stoi_bands");
    return FS2_OK;
}

// ------------------------------------------------------------------ segment scores
__global__ void __launch_bounds__(64) stoi_segment_kernel(const double* __restrict__ X, const double* __restrict__ Y, long ld_b, long ld_k,
                                                          const int32_t* __restrict__ n_kept, double clip, double* __restrict__ seg,
                                                          long lds_b, long lds_k, int Fmax) {
    __shared__ double xs[ST_J][ST_L], ys[ST_J][ST_L];                  // the segment as it is
    __shared__ double xr[ST_J][ST_L], yr[ST_J][ST_L];                  // ESTOI: after the row normalisation
    __shared__ double dk[ST_J], dn[ST_L];
    const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    if (s >= st_kept(n_kept, b, Fmax) - ST_L) return;                   // M - 29 segments, M = n_kept - 1
    for (int q = tid; q < ST_J * ST_L; q += 64) {
        const int k = q / ST_L, n = q % ST_L;
        const size_t at = (size_t)b * ld_b + (size_t)k * ld_k + s + n;
        xs[k][n] = X[at];
        ys[k][n] = Y[at];
    }
    __syncthreads();
    if (tid < ST_J) {                                                   // STOI: one band per thread, every sum ascending in the frame
        const int k = tid;
        double sx = 0.0, sy = 0.0;
        for (int n = 0; n < ST_L; ++n) { sx = fma(xs[k][n], xs[k][n], sx); sy = fma(ys[k][n], ys[k][n], sy); }
        const double alpha = sqrt(sx) / (sqrt(sy) + ST_EPS);
        double mx = 0.0, my = 0.0;
        for (int n = 0; n < ST_L; ++n) { mx += xs[k][n]; my += fmin(alpha * ys[k][n], clip * xs[k][n]); }
        mx /= (double)ST_L;
        my /= (double)ST_L;
        double nx = 0.0, ny = 0.0;
        for (int n = 0; n < ST_L; ++n) {
            const double u = xs[k][n] - mx, v = fmin(alpha * ys[k][n], clip * xs[k][n]) - my;
            nx = fma(u, u, nx);
            ny = fma(v, v, ny);
        }
        nx = sqrt(nx) + ST_EPS;
        ny = sqrt(ny) + ST_EPS;
        double d = 0.0;
        for (int n = 0; n < ST_L; ++n) {
            const double u = (xs[k][n] - mx) / nx, v = (fmin(alpha * ys[k][n], clip * xs[k][n]) - my) / ny;
            d = fma(u, v, d);
        }
        dk[k] = d;
    }
    if (tid >= 32 && tid < 32 + 2 * ST_J) {                             // ESTOI rows, on the second half-wave: X then Y
        const int k = (tid - 32) % ST_J;
        const double* src = tid - 32 < ST_J ? xs[k] : ys[k];
        double* dst = tid - 32 < ST_J ? xr[k] : yr[k];
        double mu = 0.0;
        for (int n = 0; n < ST_L; ++n) mu += src[n];
        mu /= (double)ST_L;
        double nn = 0.0;
        for (int n = 0; n < ST_L; ++n) { const double u = src[n] - mu; nn = fma(u, u, nn); }
        nn = sqrt(nn) + ST_EPS;
        for (int n = 0; n < ST_L; ++n) dst[n] = (src[n] - mu) / nn;
    }
    __syncthreads();
    if (tid < ST_L) {                                                   // ESTOI columns: one frame per thread
        const int n = tid;
        double mx = 0.0, my = 0.0;
        for (int k = 0; k < ST_J; ++k) { mx += xr[k][n]; my += yr[k][n]; }
        mx /= (double)ST_J;
        my /= (double)ST_J;
        double nx = 0.0, ny = 0.0;
        for (int k = 0; k < ST_J; ++k) {
            const double u = xr[k][n] - mx, v = yr[k][n] - my;
            nx = fma(u, u, nx);
            ny = fma(v, v, ny);
        }
        nx = sqrt(nx) + ST_EPS;
        ny = sqrt(ny) + ST_EPS;
        double d = 0.0;
        for (int k = 0; k < ST_J; ++k) d = fma((xr[k][n] - mx) / nx, (yr[k][n] - my) / ny, d);
        dn[n] = d;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, c = 0.0;
        for (int k = 0; k < ST_J; ++k) a += dk[k];
        for (int n = 0; n < ST_L; ++n) c += dn[n];
        seg[(size_t)b * lds_b + s] = a / (double)ST_J;
        seg[(size_t)b * lds_b + lds_k + s] = c / (double)ST_L;
    }
}
extern "C" int fs2_stoi_segments(const double* X, const double* Y, long ld_b, long ld_k, const int32_t* n_kept, double clip, double* seg,
                                 long lds_b, long lds_k, int B, int Fmax, hipStream_t stream) {
    FS2_CHECK_ARG(n_kept, "stoi_segments: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Fmax >= 0 && Fmax <= (1 << 23) && clip >= 1.0, "stoi_segments: bad arguments B=%d Fmax=%d clip=%g (>= 1)",
                  B, Fmax, clip);
    const int Mmax = Fmax > 0 ? Fmax - 1 : 0, Smax = Mmax >= ST_L ? Mmax - ST_L + 1 : 0;
    FS2_CHECK_ARG(Smax == 0 || (X && Y && seg && ld_k >= Mmax && ld_b >= ST_J * ld_k && lds_k >= Smax && lds_b >= 2 * lds_k),
                  "stoi_segments: X, Y must hold 15 x %d magnitudes and seg 2 x %d scores per row (ld_b=%ld ld_k=%ld lds_b=%ld lds_k=%ld)",
                  Mmax, Smax, ld_b, ld_k, lds_b, lds_k);
    if (B == 0 || Smax == 0) return FS2_OK;
    stoi_segment_kernel<<<dim3(Smax, B), 64, 0, stream>>>(X, Y, ld_b, ld_k, n_kept, clip, seg, lds_b, lds_k, Fmax);
    FS2_CHECK_LAUNCH("stoi_segments");
    return FS2_OK;
}

// ------------------------------------------------------------------ the row's scores
// fixed-shape sum over the workgroup: strided per thread, xor tree per wave, waves in ascending order
static __device__ __forceinline__ double st_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ void __launch_bounds__(256) stoi_mean_kernel(const double* __restrict__ seg, long lds_b, long lds_k,
                                                        const int32_t* __restrict__ lens, const int32_t* __restrict__ n_kept,
                                                        double* __restrict__ out, int Nmax) {
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x, F = ST_FRAMES(st_len(lens, b, Nmax)), nk = st_kept(n_kept, b, F);
    const int S = nk - ST_L > 0 ? nk - ST_L : 0;
    double a = 0.0, c = 0.0;
    for (int s = tid; s < S; s += 256) {
        a += seg[(size_t)b * lds_b + s];
        c += seg[(size_t)b * lds_b + lds_k + s];
    }
    a = st_sum(a, red);
    c = st_sum(c, red);
    if (tid == 0) {
        double* o = out + (size_t)b * 6;
        o[0] = S ? a / (double)S : st_nan();
        o[1] = S ? c / (double)S : st_nan();
        o[2] = (double)F;
        o[3] = (double)nk;
        o[4] = (double)S;
        o[5] = S ? 0.0 : 1.0;
    }
}
extern "C" int fs2_stoi_mean(const double* seg, long lds_b, long lds_k, const int32_t* lens, const int32_t* n_kept, double* out, int B,
                             int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(lens && n_kept && out, "stoi_mean: null pointer");
    FS2_CHECK_ARG(B >= 0 && Nmax >= 0, "stoi_mean: bad shape B=%d Nmax=%d", B, Nmax);
    const int Fmax = ST_FRAMES(Nmax), Smax = Fmax - 1 >= ST_L ? Fmax - ST_L : 0;
    FS2_CHECK_ARG(Smax == 0 || (seg && lds_k >= Smax && lds_b >= 2 * lds_k), "stoi_mean: seg must hold 2 x %d scores per row (lds_b=%ld lds_k=%ld)",
                  Smax, lds_b, lds_k);
    if (B == 0) return FS2_OK;
    stoi_mean_kernel<<<B, 256, 0, stream>>>(seg, lds_b, lds_k, lens, n_kept, out, Nmax);
    FS2_CHECK_LAUNCH("stoi_mean");
    return FS2_OK;
}
