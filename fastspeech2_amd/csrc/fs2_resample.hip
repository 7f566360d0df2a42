// fs2_resample.hip — rational polyphase sample-rate conversion, peak and peak-normalised int16 PCM on ragged batches.
// The specification is the docstring of fastspeech2_amd/resample.py (mirrored in DESIGN.md); tests/resample_ref.py restates it in
// numpy.  With half = 10 max(up, down) and the 2 half + 1 fp64 taps h of scipy.signal.resample_poly's default filter,
//     y[j] = sum over i of x[i] * h[j down - i up + half],      0 <= j down - i up + half <= 2 half,
// the i outside the row's slice [in_begin, in_begin + in_len) counting as zero.  Output j uses only the taps of one phase,
// p = (j down + half) mod up; with q = (j down + half) div up they are h[p + t up] against x[q - t].  The host lays the taps out
// phase-major and in ASCENDING input index: tab[p][s] = h[p + (T - 1 - s) up] (0 where that index exceeds 2 half), T even, so
//     y[j] = sum_{s < T} tab[p][s] * x[q - T + 1 + s]
// is a dot product of two contiguous runs: the taps stream from global memory (L2-resident: up * T doubles) as 16-byte loads, the
// samples come from an LDS tile that the workgroup's 256 consecutive outputs share.  fp64 taps, fp64 fma in ascending input index,
// one rounding to float32 at the store; no atomics, and nothing but the row's own samples enters a row's result.
//
//   fs2_resample_poly   one output per thread, 256 outputs per workgroup; LDS tile of (up - 1 + 255 down) / up + T input samples,
//                       or, where that tile would not fit 64 KiB, the same sum with the samples read from global memory
//   fs2_peak_abs        peak[b] = max |y[b][0, len[b])| on the magnitude bits (integer max: exact in any order, NaN propagates)
//   fs2_peaknorm_pcm    pcm = int16(y / peak * max_wav_value): two float32 operations, truncation toward zero to int32, low 16 bits
#include "fs2_common.h"

#define RS_T 256                    // outputs per workgroup
#define RS_LDS_MAX 65536            // largest staged tile in bytes (no dynamic-LDS opt-in needed up to here)

static __device__ __forceinline__ int rs_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }

// ------------------------------------------------------------------ polyphase resampler
template <bool STAGE>
__global__ void resample_poly_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ in_begin,
                                     const int32_t* __restrict__ in_len, const double* __restrict__ tab, int up, int down, int half,
                                     int T, const int32_t* __restrict__ out_begin, const int32_t* __restrict__ out_len,
                                     float* __restrict__ y, float* __restrict__ yc, long ldy, int Nin, int Nout, int span) {
    extern __shared__ float xs[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n_out = rs_len(out_len, b, Nout), n_in = rs_len(in_len, b, Nin);
    const int t0 = blockIdx.x * RS_T;
    if (t0 >= n_out) return;
    const long ib = in_begin ? (long)in_begin[b] : 0L;
    // first output of the tile: 64-bit once per workgroup, 32-bit per thread ((RS_T - 1) down + up < 2^31 is checked on the host)
    const long jd0 = ((long)(out_begin ? out_begin[b] : 0) + t0) * down + half;
    const long q0 = jd0 / up;
    const int r0 = (int)(jd0 - q0 * up);
    const long rel0 = q0 - T + 1 - ib;                              // row-relative index of the tile's first staged sample
    const float* xr = x + (size_t)b * ldx;
    if (STAGE) {
        for (int k = tid; k < span; k += RS_T) {
            const long n = rel0 + k;
            xs[k] = (n >= 0 && n < n_in) ? xr[n] : 0.0f;
        }
        __syncthreads();
    }
    const int t = t0 + tid;
    if (t >= n_out) return;
    const int v = r0 + tid * down;
    const int dq = v / up, p = v - dq * up;
    const double2* tp = reinterpret_cast<const double2*>(tab + (size_t)p * T);
    double acc = 0.0;
    if (STAGE) {
        const float* xp = xs + dq;
        for (int s = 0; s < T; s += 2) {
            const double2 h = tp[s >> 1];
            acc = fma(h.x, (double)xp[s], acc);
            acc = fma(h.y, (double)xp[s + 1], acc);
        }
    } else {
        const long n0 = rel0 + dq;
        for (int s = 0; s < T; s += 2) {
            const double2 h = tp[s >> 1];
            const long n = n0 + s;
            acc = fma(h.x, (n >= 0 && n < n_in) ? (double)xr[n] : 0.0, acc);
            acc = fma(h.y, (n + 1 >= 0 && n + 1 < n_in) ? (double)xr[n + 1] : 0.0, acc);
        }
    }
    const float r = (float)acc;
    y[(size_t)b * ldy + t] = r;
    if (yc) yc[(size_t)b * ldy + t] = r < -1.0f ? -1.0f : (r > 1.0f ? 1.0f : r);     // numpy.clip: NaN stays NaN
}
extern "C" int fs2_resample_poly(const float* x, long ldx, const int32_t* in_begin, const int32_t* in_len, const double* tab, int up,
                                 int down, int half, int T, const int32_t* out_begin, const int32_t* out_len, float* y, float* yc,
                                 long ldy, int B, int Nin, int Nout, hipStream_t stream) {
    FS2_CHECK_ARG(x && in_len && tab && out_len && y, "resample_poly: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nin >= 0 && Nout >= 0 && ldx >= Nin && ldy >= Nout,
                  "resample_poly: bad shape B=%d Nin=%d Nout=%d ldx=%ld ldy=%ld", B, Nin, Nout, ldx, ldy);
    FS2_CHECK_ARG(up > 0 && down > 0 && half >= 0 && T > 0 && T % 2 == 0 && (long)up * T >= 2L * half + 1 &&
                      (long)(RS_T - 1) * down + up < (1L << 31) && ((uintptr_t)tab & 15) == 0,
                  "resample_poly: bad filter up=%d down=%d half=%d T=%d (T even, up * T taps cover 2 half + 1, table 16-byte aligned)",
                  up, down, half, T);
    if (B == 0 || Nout == 0) return FS2_OK;
    const long span = ((long)up - 1 + (long)(RS_T - 1) * down) / up + T;
    const dim3 grid(fs2_cdiv(Nout, RS_T), B);
    if (span * (long)sizeof(float) <= RS_LDS_MAX)
        resample_poly_kernel<true><<<grid, RS_T, span * sizeof(float), stream>>>(x, ldx, in_begin, in_len, tab, up, down, half, T,
                                                                                out_begin, out_len, y, yc, ldy, Nin, Nout, (int)span);
    else
        resample_poly_kernel<false><<<grid, RS_T, 0, stream>>>(x, ldx, in_begin, in_len, tab, up, down, half, T, out_begin, out_len,
                                                              y, yc, ldy, Nin, Nout, 0);
    FS2_CHECK_LAUNCH("resample_poly");
    return FS2_OK;
}

// ------------------------------------------------------------------ peak
// |y| as its 31 magnitude bits: for floats of one sign the integer order is the float order (and every NaN sorts above infinity, so
// a NaN in the row comes out as NaN, as numpy.max does), which makes the maximum exact whatever the reduction shape.
#define PK_PER_BLOCK 4096
__global__ void peak_abs_kernel(const float* __restrict__ y, long ldy, const int32_t* __restrict__ lens, uint32_t* __restrict__ peak,
                                int Nmax) {
    __shared__ uint32_t red[256 / 64];
    const int b = blockIdx.y, tid = threadIdx.x, N = rs_len(lens, b, Nmax);
    const int n0 = blockIdx.x * PK_PER_BLOCK;
    if (n0 >= N) return;
    const float* yr = y + (size_t)b * ldy;
    uint32_t m = 0;
    const int n1 = min(n0 + PK_PER_BLOCK, N);
    for (int n = n0 + tid; n < n1; n += 256) m = max(m, __float_as_uint(yr[n]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) atomicMax(peak + b, max(max(red[0], red[1]), max(red[2], red[3])));
}
extern "C" int fs2_peak_abs(const float* y, long ldy, const int32_t* lens, float* peak, int B, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(y && lens && peak, "peak_abs: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldy >= Nmax, "peak_abs: bad shape B=%d Nmax=%d ldy=%ld", B, Nmax, ldy);
    if (B == 0) return FS2_OK;
    if (hipMemsetAsync(peak, 0, (size_t)B * sizeof(float), stream) != hipSuccess) {
        fs2_set_error("peak_abs: hipMemsetAsync failed");
        return FS2_ELAUNCH;
    }
    if (Nmax == 0) return FS2_OK;
    peak_abs_kernel<<<dim3(fs2_cdiv(Nmax, PK_PER_BLOCK), B), 256, 0, stream>>>(y, ldy, lens, reinterpret_cast<uint32_t*>(peak), Nmax);
    FS2_CHECK_LAUNCH("peak_abs");
    return FS2_OK;
}

// ------------------------------------------------------------------ peak-normalise + PCM cast
// pcm[b][n] = int16(y[b][n] / peak[b] * max_wav): correctly rounded float32 division, then the float32 product, then the cast of
// fs2_vocoder.hip (numpy astype('int16') of float32 on x86): truncate toward zero to int32, keep the low 16 bits - so a positive
// peak sample times 32768 wraps to -32768, as in the reference.  peak == 0: zeros.  [len[b], Nmax) of a row is zero-filled.
__global__ void peaknorm_pcm_kernel(const float* __restrict__ y, long ldy, const int32_t* __restrict__ lens,
                                    const float* __restrict__ peak, float max_wav, int16_t* __restrict__ pcm, long ldp, int Nmax) {
    const int b = blockIdx.y, N = rs_len(lens, b, Nmax);
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Nmax) return;
    int16_t o = 0;
    const float pk = peak[b];
    if (n < N && pk != 0.0f) {
        const float s = y[(size_t)b * ldy + n] / pk * max_wav;
        o = (int16_t)((int32_t)s & 0xffff);
    }
    pcm[(size_t)b * ldp + n] = o;
}
extern "C" int fs2_peaknorm_pcm(const float* y, long ldy, const int32_t* lens, const float* peak, float max_wav_value, int16_t* pcm,
                                long ldp, int B, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(y && lens && peak && pcm, "peaknorm_pcm: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldy >= Nmax && ldp >= Nmax, "peaknorm_pcm: bad shape B=%d Nmax=%d ldy=%ld ldp=%ld",
                  B, Nmax, ldy, ldp);
    if (B == 0 || Nmax == 0) return FS2_OK;
    peaknorm_pcm_kernel<<<dim3(fs2_cdiv(Nmax, 256), B), 256, 0, stream>>>(y, ldy, lens, peak, max_wav_value, pcm, ldp, Nmax);
    FS2_CHECK_LAUNCH("peaknorm_pcm");
    return FS2_OK;
}
