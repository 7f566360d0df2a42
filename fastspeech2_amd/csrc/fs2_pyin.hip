// fs2_pyin.hip — probabilistic YIN (Mauch & Dixon 2014) in fp64 on ragged batches, in three stages.
// The specification every kernel here implements is the docstring of fastspeech2_amd/pyin.py (mirrored in DESIGN.md);
// tests/pyin_ref.py restates it in numpy.  Input rows are float32 x[b][0, lens[b]) (row stride ldx); nothing at or beyond lens[b]
// is read.  Every sum has a fixed order that depends on the row alone and there are no atomics, so one utterance's F0 is bitwise
// the same whatever else shares its batch.
//
//   fs2_pyin_cmnd     one wave per frame, FR consecutive frames of a row per workgroup: their span of samples is staged once in LDS
//                     as doubles; lane l takes the lags l, l + 64, ... (R per pass), so at step j the wave reads one broadcast sample
//                     x[s0 + j] and R runs of 64 consecutive doubles: conflict-free.  d(tau) goes to LDS, the wave scans it.
//   fs2_pyin_observe  one wave per frame: troughs of d' flagged and compacted in lag order (ballot), exclusive prefix minimum of
//                     their heights, the 100 threshold weights summed per trough, run leaders add the masses of one bin in lag order;
//                     a frame whose d' is flat over the range (digital silence) gets no voiced mass
//   fs2_pyin_viterbi  one workgroup per row: log-domain Viterbi over 2 nb states with a banded transition, delta ping-pongs in LDS,
//                     one byte of backpointer per (frame, state); one lane backtracks
#include "fs2_common.h"
#include <math.h>

#define PYIN_LDS_MAX 65536            // dynamic LDS every kernel here stays under (no opt-in needed)
#define PYIN_VT 1024                  // threads of the Viterbi workgroup

static __device__ __forceinline__ int pyin_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }

// ------------------------------------------------------------------ difference function + cumulative-mean normalisation
// grid (ceil(Fmax / FR), B), block 64 FR.  LDS: span[(FR - 1) hop + L] doubles, then FR rows of tmax + 1 doubles.
template <int R>
__global__ void __launch_bounds__(512) pyin_cmnd_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ lens,
                                                        const int32_t* __restrict__ frames, int hop, int L, int W, int tmax,
                                                        double* __restrict__ out, int Fmax, int Nmax) {
    extern __shared__ double pyin_sm[];
    const int FR = blockDim.x >> 6, b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f0 = blockIdx.x * FR, f = f0 + wave;
    const int N = pyin_len(lens, b, Nmax), F = min(max(frames[b], 0), Fmax);
    const int span = (FR - 1) * hop + L, nl = tmax + 1;
    double* xs = pyin_sm;
    double* dd = pyin_sm + span + (size_t)wave * nl;
    const float* xr = x + (size_t)b * ldx;
    const long base = (long)f0 * hop - L / 2;                       // sample index of xs[0]
    for (int i = threadIdx.x; i < span; i += blockDim.x) {
        const long n = base + i;
        xs[i] = (n >= 0 && n < N) ? (double)xr[n] : 0.0;
    }
    __syncthreads();
    if (f >= Fmax) return;                                          // whole waves leave; no barrier follows
    double* o = out + ((size_t)b * Fmax + f) * nl;
    if (f >= F) {
        for (int t = lane; t < nl; t += 64) o[t] = 0.0;
        return;
    }
    const double* xf = xs + wave * hop;                             // this frame's first sample
    for (int t0 = 0; t0 < nl; t0 += 64 * R) {
        double acc[R];
        int tau[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r] = 0.0;
            tau[r] = min(t0 + 64 * r + lane, tmax);                 // lanes past tmax repeat it (in bounds) and store nothing
        }
#pragma unroll 4
        for (int j = 0; j < W; ++j) {
            const double a = xf[j];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double d = a - xf[j + tau[r]];
                acc[r] = fma(d, d, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = t0 + 64 * r + lane;
            if (t <= tmax) dd[t] = acc[r];
        }
    }
    // d'(0) = 1; d'(tau) = d(tau) tau / sum_{j=1..tau} d(j), 1 where that sum is 0: inclusive scan in runs of 64 lags
    double carry = 0.0;
    for (int t0 = 0; t0 < nl; t0 += 64) {
        const int t = t0 + lane;
        const double d = (t >= 1 && t < nl) ? dd[t] : 0.0;
        double s = d;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const double u = __shfl_up(s, k, 64);
            if (lane >= k) s += u;
        }
        s += carry;
        carry = __shfl(s, 63, 64);
        if (t < nl) o[t] = (t == 0 || s == 0.0) ? 1.0 : d * (double)t / s;
    }
}

template <int R>
static void pyin_cmnd_launch(dim3 grid, int threads, size_t lds, hipStream_t stream, const float* x, long ldx, const int32_t* lens,
                             const int32_t* frames, int hop, int L, int W, int tmax, double* out, int Fmax, int Nmax) {
    pyin_cmnd_kernel<R><<<grid, threads, lds, stream>>>(x, ldx, lens, frames, hop, L, W, tmax, out, Fmax, Nmax);
}

extern "C" int fs2_pyin_cmnd(const float* x, long ldx, const int32_t* lens, const int32_t* frames, int hop, int frame_length, int tmax,
                             double* dprime, int B, int Fmax, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && frames && dprime, "pyin_cmnd: null pointer");
    const int L = frame_length, W = L / 2;
    FS2_CHECK_ARG(B >= 0 && Fmax >= 0 && Nmax >= 0 && ldx >= Nmax && hop >= 1 && L >= 4 && L % 2 == 0 && tmax >= 1 && tmax <= L - W - 1,
                  "pyin_cmnd: bad shape B=%d Fmax=%d Nmax=%d ldx=%ld hop=%d frame_length=%d tmax=%d", B, Fmax, Nmax, ldx, hop, L, tmax);
    if (B == 0 || Fmax == 0) return FS2_OK;
    int FR = 8;                                                     // frames per workgroup: the most whose span fits
    auto bytes = [&](int fr) { return ((size_t)(fr - 1) * hop + L + (size_t)fr * (tmax + 1)) * sizeof(double); };
    while (FR > 1 && bytes(FR) > PYIN_LDS_MAX) FR >>= 1;
    FS2_CHECK_ARG(bytes(FR) <= PYIN_LDS_MAX, "pyin_cmnd: frame_length %d with tmax %d needs %zu B of LDS", L, tmax, bytes(FR));
    const dim3 grid(fs2_cdiv(Fmax, FR), B);
    const int R = min(8, fs2_cdiv(tmax + 1, 64));
    switch (R) {
#define PYIN_CASE(r) case r: pyin_cmnd_launch<r>(grid, 64 * FR, bytes(FR), stream, x, ldx, lens, frames, hop, L, W, tmax, dprime, Fmax, Nmax); break;
        PYIN_CASE(1) PYIN_CASE(2) PYIN_CASE(3) PYIN_CASE(4) PYIN_CASE(5) PYIN_CASE(6) PYIN_CASE(7) PYIN_CASE(8)
#undef PYIN_CASE
    }
    FS2_CHECK_LAUNCH("pyin_cmnd");
    return FS2_OK;
}

// ------------------------------------------------------------------ troughs -> observation row
static __device__ __forceinline__ double pyin_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (Fmax, B), block 64.  LDS: voiced[nb], height[cap], mass[cap] doubles, then tau[cap], bin[cap] ints; cap = (tmax - tmin) / 2 + 1.
__global__ void __launch_bounds__(64) pyin_observe_kernel(const double* __restrict__ dprime, const int32_t* __restrict__ frames,
                                                          int tmin, int tmax, const double* __restrict__ beta, int nthr,
                                                          double no_trough, double fs, double f_floor, double bins_per_octave, int nb,
                                                          double* __restrict__ obs, double* __restrict__ pv, int Fmax) {
    extern __shared__ double pyin_sm[];
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, nl = tmax + 1, cap = (tmax - tmin) / 2 + 1;
    double* voiced = pyin_sm;
    double* th = voiced + nb;
    double* tm = th + cap;
    int* tt = (int*)(tm + cap);
    int* tbin = tt + cap;
    double* orow = obs + ((size_t)b * Fmax + f) * (2 * (size_t)nb);
    if (f >= min(max(frames[b], 0), Fmax)) {
        for (int i = lane; i < 2 * nb; i += 64) orow[i] = 0.0;
        if (lane == 0) pv[(size_t)b * Fmax + f] = 0.0;
        return;
    }
    const double* d = dprime + ((size_t)b * Fmax + f) * nl;
    for (int i = lane; i < nb; i += 64) voiced[i] = 0.0;
    // troughs in lag order; the global minimum of the range (lowest lag on ties)
    int n = 0, gt = tmin;
    double gv = INFINITY, hv = -INFINITY;
    for (int t0 = tmin; t0 <= tmax; t0 += 64) {
        const int t = t0 + lane;
        bool is = false;
        double v = 0.0;
        if (t <= tmax) {
            v = d[t];
            const bool left = t == tmin || v < d[t - 1];
            const bool right = t == tmax ? true : (t == tmin ? v < d[t + 1] : v <= d[t + 1]);
            is = left && right;
            if (v < gv) { gv = v; gt = t; }                          // a lane's lags ascend: the first of equal values stays
            hv = fmax(hv, v);
        }
        const unsigned long long m = __ballot(is);
        if (is) {
            const int p = n + __popcll(m & ((1ull << lane) - 1ull));
            tt[p] = t;
            th[p] = v;
        }
        n += __popcll(m);
    }
    const double gmin = pyin_wave_min(gv);
    const bool flat = -pyin_wave_min(-hv) == gmin;                   // d' the same at every lag (digital silence): no candidate
    int gcand = gv == gmin ? gt : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gcand = min(gcand, __shfl_xor(gcand, o, 64));
    __syncthreads();
    // shift, bin and threshold mass per trough; entry n is the global minimum
    auto bin_of = [&](int t) {
        double shift = 0.0;
        if (t > tmin && t < tmax) {
            const double a = d[t - 1], c = d[t + 1], den = a - 2.0 * d[t] + c;
            if (den > 0.0) shift = (a - c) / (2.0 * den);
        }
        const double freq = fs / ((double)t + shift);
        const int k = (int)floor(bins_per_octave * log2(freq / f_floor) + 0.5);
        return min(max(k, 0), nb - 1);
    };
    double carry = INFINITY;                                         // minimum height of the troughs before this run of 64
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const double h = i < n ? th[i] : INFINITY;
        double s = h;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const double u = __shfl_up(s, k, 64);
            if (lane >= k) s = fmin(s, u);
        }
        double pm = __shfl_up(s, 1, 64);                             // exclusive: the troughs at lower lags
        pm = lane == 0 ? carry : fmin(pm, carry);
        carry = fmin(carry, __shfl(s, 63, 64));
        if (i < n) {
            double mass = 0.0;
            for (int k = 1; k <= nthr; ++k) {
                const double sk = (double)k / (double)nthr;
                if (h < sk && !(pm < sk)) mass += beta[k - 1];
            }
            tm[i] = mass;
            tbin[i] = bin_of(tt[i]);
        }
    }
    double gmass = 0.0;                                              // thresholds no trough is below (carry = the lowest height)
    for (int k = 1; k <= nthr; ++k) {
        const double sk = (double)k / (double)nthr;
        if (!(carry < sk)) gmass += no_trough * beta[k - 1];
    }
    if (flat) gmass = 0.0;
    const int gbin = bin_of(gcand);
    __syncthreads();
    // troughs of one bin are neighbours in lag order: the first of each run adds the run's masses in that order
    for (int i = lane; i < n; i += 64) {
        const int k = tbin[i];
        if (i == 0 || tbin[i - 1] != k) {
            double s = 0.0;
            for (int q = i; q < n && tbin[q] == k; ++q) s += tm[q];
            voiced[k] = s;
        }
    }
    __syncthreads();
    double total = 0.0;
    if (lane == 0) {
        voiced[gbin] += gmass;
        for (int i = 0; i < n; ++i) total += tm[i];
        total += gmass;
    }
    __syncthreads();
    total = __shfl(total, 0, 64);
    const double p = fmin(total, 1.0), unv = (1.0 - p) / (double)nb;
    for (int i = lane; i < nb; i += 64) {
        orow[i] = voiced[i];
        orow[nb + i] = unv;
    }
    if (lane == 0) pv[(size_t)b * Fmax + f] = p;
}

extern "C" int fs2_pyin_observe(const double* dprime, const int32_t* frames, int tmin, int tmax, const double* beta, int nthr,
                                double no_trough_prob, double fs, double fmin, int bins_per_octave, int nb, double* obs, double* pv,
                                int B, int Fmax, hipStream_t stream) {
    FS2_CHECK_ARG(dprime && frames && beta && obs && pv, "pyin_observe: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax >= 0 && tmin >= 1 && tmax > tmin && nthr >= 1 && nb >= 1 && bins_per_octave >= 1 && fs > 0 && fmin > 0 &&
                  no_trough_prob >= 0, "pyin_observe: bad shape B=%d Fmax=%d tmin=%d tmax=%d nthr=%d nb=%d", B, Fmax, tmin, tmax, nthr, nb);
    const size_t cap = (size_t)(tmax - tmin) / 2 + 1, lds = ((size_t)nb + 2 * cap) * sizeof(double) + 2 * cap * sizeof(int);
    FS2_CHECK_ARG(lds <= PYIN_LDS_MAX, "pyin_observe: nb=%d with %zu lags needs %zu B of LDS", nb, 2 * cap, lds);
    if (B == 0 || Fmax == 0) return FS2_OK;
    pyin_observe_kernel<<<dim3(Fmax, B), 64, lds, stream>>>(dprime, frames, tmin, tmax, beta, nthr, no_trough_prob, fs, fmin,
                                                            (double)bins_per_octave, nb, obs, pv, Fmax);
    FS2_CHECK_LAUNCH("pyin_observe");
    return FS2_OK;
}

// ------------------------------------------------------------------ Viterbi
// grid B, block PYIN_VT.  LDS: two vectors of 2 nb doubles and the 2 h + 1 log weights.  State s = v nb + bin, v = 0 voiced, 1 unvoiced.  A buffer holds
// delta(s) - logz[bin] (what the next frame adds its band weights to) except after the last frame, where it holds delta itself.
__global__ void __launch_bounds__(PYIN_VT) pyin_viterbi_kernel(const double* __restrict__ obs, const int32_t* __restrict__ frames,
                                                               int nb, int h, const double* __restrict__ logw,
                                                               const double* __restrict__ logz, double log_keep, double log_flip,
                                                               double f_floor, double bins_per_octave, uint8_t* __restrict__ bp,
                                                               int32_t* __restrict__ states, double* __restrict__ f0, int Fmax) {
    extern __shared__ double pyin_sm[];
    const int b = blockIdx.x, tid = threadIdx.x, S = 2 * nb;
    const int F = min(max(frames[b], 0), Fmax);
    int32_t* srow = states + (size_t)b * Fmax;
    double* frow = f0 + (size_t)b * Fmax;
    for (int t = F + tid; t < Fmax; t += PYIN_VT) {
        srow[t] = 0;
        frow[t] = 0.0;
    }
    if (F == 0) return;
    const double* orow = obs + (size_t)b * Fmax * S;
    uint8_t* brow = bp + (size_t)b * Fmax * S;
    double* cur = pyin_sm;
    double* nxt = pyin_sm + S;
    double* lw = pyin_sm + 2 * S;                                              // the band's log weights: every lane reads one address
    for (int o = tid; o <= 2 * h; o += PYIN_VT) lw[o] = logw[o];
    const double logpi = -log((double)S);
    for (int s = tid; s < S; s += PYIN_VT) {
        const double o = orow[s], v = logpi + (o > 0.0 ? log(o) : -INFINITY);
        cur[s] = F == 1 ? v : v - logz[s < nb ? s : s - nb];
    }
    __syncthreads();
    for (int t = 1; t < F; ++t) {
        const double* ot = orow + (size_t)t * S;
        uint8_t* bt = brow + (size_t)t * S;
        for (int s = tid; s < S; s += PYIN_VT) {
            const int v1 = s >= nb, j = s - v1 * nb;
            const int lo = max(0, h - j), hi = min(2 * h, nb - 1 - j + h);      // offsets o: predecessor bin i = j - h + o in [0, nb)
            double best = -INFINITY;
            int code = 2 * lo + v1;                                             // the first candidate: voiced half, lowest bin
            for (int v0 = 0; v0 < 2; ++v0) {
                const double sw = v0 == v1 ? log_keep : log_flip;
                const int off = v0 * nb + j - h;
                for (int o = lo; o <= hi; ++o) {
                    const double c = (cur[off + o] + lw[o]) + sw;
                    if (c > best) { best = c; code = 2 * o + (v0 ^ v1); }
                }
            }
            const double o = ot[s], val = (o > 0.0 ? log(o) : -INFINITY) + best;
            nxt[s] = t == F - 1 ? val : val - logz[j];
            bt[s] = (uint8_t)code;
        }
        __syncthreads();
        double* sw = cur; cur = nxt; nxt = sw;
    }
    __threadfence_block();
    __syncthreads();
    if (tid >= 64) return;
    // the best final state, lowest index on ties; then one lane walks the backpointers
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int s = tid; s < S; s += 64) {
        const double v = cur[s];
        if (bi == 0x7fffffff || v > bv) { bv = v; bi = s; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (tid == 0) {
        int s = bi;
        for (int t = F - 1; t >= 0; --t) {
            const int v1 = s >= nb, j = s - v1 * nb;
            srow[t] = s;
            frow[t] = v1 ? 0.0 : f_floor * exp2((double)j / bins_per_octave);
            if (t > 0) {
                const int code = brow[(size_t)t * S + s];
                s = ((code & 1) ^ v1) * nb + min(max(j - h + (code >> 1), 0), nb - 1);
            }
        }
    }
}

extern "C" int fs2_pyin_viterbi(const double* obs, const int32_t* frames, int nb, int half_width, const double* logw, const double* logz,
                                double switch_prob, double fmin, int bins_per_octave, uint8_t* backptr, int32_t* states, double* f0,
                                int B, int Fmax, hipStream_t stream) {
    FS2_CHECK_ARG(obs && frames && logw && logz && backptr && states && f0, "pyin_viterbi: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax >= 0 && nb >= 1 && half_width >= 0 && bins_per_octave >= 1 && fmin > 0 && switch_prob >= 0 &&
                  switch_prob <= 1, "pyin_viterbi: bad shape B=%d Fmax=%d nb=%d half_width=%d", B, Fmax, nb, half_width);
    FS2_CHECK_ARG(2 * (2 * half_width + 1) <= 255, "pyin_viterbi: a band of %d offsets does not fit a one-byte backpointer",
                  2 * half_width + 1);
    const size_t lds = (4 * (size_t)nb + 2 * (size_t)half_width + 1) * sizeof(double);
    FS2_CHECK_ARG(lds <= PYIN_LDS_MAX, "pyin_viterbi: nb=%d needs %zu B of LDS", nb, lds);
    if (B == 0 || Fmax == 0) return FS2_OK;
    pyin_viterbi_kernel<<<B, PYIN_VT, lds, stream>>>(obs, frames, nb, half_width, logw, logz,
                                                     switch_prob < 1 ? log1p(-switch_prob) : -INFINITY,
                                                     switch_prob > 0 ? log(switch_prob) : -INFINITY, fmin, (double)bins_per_octave,
                                                     backptr, states, f0, Fmax);
    FS2_CHECK_LAUNCH("pyin_viterbi");
    return FS2_OK;
}
