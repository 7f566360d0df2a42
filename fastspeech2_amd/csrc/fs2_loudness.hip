// fs2_loudness.hip — ITU-R BS.1770-4 programme loudness of ragged float32 batches, and the gain + int16 cast that goes with it.
// The specification is the docstring of fastspeech2_amd/loudness.py (mirrored in DESIGN.md); tests/loudness_ref.py restates it in
// numpy / scipy.  Everything after the float32 load is fp64.
//
// K-weighting is two biquads in cascade (high shelf, then the RLB high-pass), each in transposed direct form II, the form of
// scipy.signal.lfilter:   y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y.   The four states make a linear recursion
// S' = A S + B x.  A row is cut into chunks of KW_L samples, KW_T chunks to a tile, one thread per chunk and one workgroup per tile:
//
//   kw_chunk_kernel   every chunk runs the cascade from ZERO state and keeps its end state e0; a Hillis-Steele scan over the tile,
//                     v[c] += A^(L 2^d) v[c - 2^d] with the host-computed powers pw[d], leaves the tile's zero-state end state T0
//   kw_energy_kernel  the tile's true start state is T0[j] + A^(L T) S over the tiles j before it (a few dozen 4 x 4 products);
//                     the same scan, seeded with it, gives every chunk's true start state; the chunk runs the cascade again from
//                     there and sums y^2 into PIECES: hop i = [i h, (i + 1) h) split at i h + (n mod h), so that block
//                     [i h, i h + n) is a run of whole pieces whatever n and h are (4 h != n at 11 025 Hz).  Per piece the chunks'
//                     partial sums are added in ascending chunk order by one thread; a piece that straddles two tiles has two slots.
//   kw_block_kernel   z[b][i] = (sum of the pieces of block i, ascending, slot 0 then slot 1) / n
//
// No atomics on floating-point data and no order that depends on timing: the same input gives the same bytes.  Samples at or beyond
// lens[b] are never loaded (a row's padding may hold anything).
//
//   fs2_gated_loudness   one workgroup per utterance: the two gates of BS.1770-4 over z
//   fs2_loudness_gain    per-utterance linear gain from loudness, sample peak, target and ceiling
//   fs2_gain_pcm         int16(rint(x g 32768)) saturated, round-half-even, with a count of saturated samples
#include "fs2_common.h"

#define KW_L 64                     // samples per chunk
#define KW_T 128                    // chunks (threads) per tile
#define KW_TILE (KW_L * KW_T)       // samples per tile
#define KW_LOG_T 7
#define KW_PAD (KW_L + 1)           // LDS row stride of a chunk: lane c reads xs[c * 65 + k], conflict-free

static __device__ __forceinline__ int kw_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }

struct KwCoef { double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2; };

// one sample through the cascade; s[0..1] the shelf's states, s[2..3] the high-pass's
static __device__ __forceinline__ double kw_step(const KwCoef& k, double x, double* s) {
    const double y1 = fma(k.b0, x, s[0]);
    s[0] = fma(k.b1, x, s[1]) - k.a1 * y1;
    s[1] = fma(k.b2, x, -k.a2 * y1);
    const double y = fma(k.c0, y1, s[2]);
    s[2] = fma(k.c1, y1, s[3]) - k.d1 * y;
    s[3] = fma(k.c2, y1, -k.d2 * y);
    return y;
}

// coalesced load of the tile's samples into xs[chunk][KW_PAD]; zero at and beyond the row's length N
static __device__ __forceinline__ void kw_stage(const float* __restrict__ xr, int t0, int N, float* xs) {
    for (int k = threadIdx.x; k < KW_TILE; k += KW_T) {
        const int m = t0 + k;
        xs[(k / KW_L) * KW_PAD + (k % KW_L)] = m < N ? xr[m] : 0.0f;
    }
    __syncthreads();
}

// inclusive scan of the chunk end states along the tile: v[c] = sum_{j <= c} A^(L (c - j)) v0[j]
static __device__ __forceinline__ void kw_scan(double* v, const double* __restrict__ pw, double (*st)[4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 0; d < KW_LOG_T; ++d) {
        const int o = 1 << d;
        for (int j = 0; j < 4; ++j) st[tid][j] = v[j];
        __syncthreads();
        if (tid >= o) {
            const double* P = pw + 16 * d;
            const double u0 = st[tid - o][0], u1 = st[tid - o][1], u2 = st[tid - o][2], u3 = st[tid - o][3];
            for (int j = 0; j < 4; ++j) v[j] += fma(P[4 * j], u0, fma(P[4 * j + 1], u1, fma(P[4 * j + 2], u2, P[4 * j + 3] * u3)));
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(KW_T) kw_chunk_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ lens,
                                                        KwCoef co, const double* __restrict__ pw, double* __restrict__ e0,
                                                        double* __restrict__ T0, int tiles, int Nmax) {
    __shared__ float xs[KW_T * KW_PAD];
    __shared__ double st[KW_T][4];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, N = kw_len(lens, b, Nmax), t0 = tile * KW_TILE;
    if (t0 >= N) return;
    kw_stage(x + (size_t)b * ldx, t0, N, xs);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const float* xp = xs + tid * KW_PAD;
    for (int k = 0; k < KW_L; ++k) kw_step(co, (double)xp[k], s);
    double* e = e0 + ((size_t)b * tiles + tile) * KW_T * 4 + tid * 4;
    for (int j = 0; j < 4; ++j) e[j] = s[j];
    kw_scan(s, pw, st);
    if (tid == KW_T - 1)
        for (int j = 0; j < 4; ++j) T0[((size_t)b * tiles + tile) * 4 + j] = s[j];
}

// piece of row sample m: 2 (m / h) + (m mod h >= r), r = n mod h (with r == 0 every even piece is empty)
__global__ void __launch_bounds__(KW_T) kw_energy_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ lens,
                                                         KwCoef co, const double* __restrict__ pw, const double* __restrict__ e0,
                                                         const double* __restrict__ T0, double* __restrict__ pieces, int tiles,
                                                         int NP, int h, int r, int Nmax) {
    __shared__ float xs[KW_T * KW_PAD];
    __shared__ double st[KW_T][4];
    __shared__ double part[KW_T][4];
    __shared__ int p0s[KW_T];
    __shared__ double S0[4];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, N = kw_len(lens, b, Nmax), t0 = tile * KW_TILE;
    if (t0 >= N) return;
    if (tid == 0) {                                                  // the tile's start state, tiles in ascending order
        const double* P = pw + 16 * KW_LOG_T;
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < tile; ++j) {
            const double* t = T0 + ((size_t)b * tiles + j) * 4;
            double n4[4];
            for (int q = 0; q < 4; ++q) n4[q] = t[q] + fma(P[4 * q], S[0], fma(P[4 * q + 1], S[1], fma(P[4 * q + 2], S[2], P[4 * q + 3] * S[3])));
            for (int q = 0; q < 4; ++q) S[q] = n4[q];
        }
        for (int q = 0; q < 4; ++q) S0[q] = S[q];
    }
    kw_stage(x + (size_t)b * ldx, t0, N, xs);                        // its barrier publishes S0 too
    double s[4];
    const double* e = e0 + ((size_t)b * tiles + tile) * KW_T * 4 + tid * 4;
    for (int j = 0; j < 4; ++j) s[j] = e[j];
    if (tid == 0)
        for (int j = 0; j < 4; ++j) s[j] += fma(pw[4 * j], S0[0], fma(pw[4 * j + 1], S0[1], fma(pw[4 * j + 2], S0[2], pw[4 * j + 3] * S0[3])));
    kw_scan(s, pw, st);
    for (int j = 0; j < 4; ++j) st[tid][j] = s[j];
    for (int j = 0; j < 4; ++j) part[tid][j] = 0.0;
    __syncthreads();
    for (int j = 0; j < 4; ++j) s[j] = tid ? st[tid - 1][j] : S0[j];
    // the chunk again, from its true start state; y^2 into the pieces it crosses (at most 4 as KW_L <= h)
    const int m0 = t0 + tid * KW_L;
    const int off = m0 % h;
    bool first = off < r;
    int next = first ? r - off : h - off;                            // chunk-relative index of the next piece boundary
    int slot = 0;
    p0s[tid] = 2 * (m0 / h) + (first ? 0 : 1);
    double acc = 0.0;
    const float* xp = xs + tid * KW_PAD;
    for (int k = 0; k < KW_L; ++k) {
        if (k == next) {
            part[tid][slot] = acc;
            acc = 0.0;
            if (first) { first = false; next += h - r; slot += 1; }
            else if (r > 0) { first = true; next += r; slot += 1; }
            else { next += h; slot += 2; }
        }
        const double y = kw_step(co, (double)xp[k], s);
        acc = fma(y, y, acc);
    }
    part[tid][slot] = acc;
    __syncthreads();
    // one thread per piece of the tile: its chunks' partial sums in ascending order
    const int pf = p0s[0];
    const long tend = (long)t0 + KW_TILE;
    const int m_last = (int)min(tend, (long)N) - 1;
    const int pl = 2 * (m_last / h) + (m_last % h >= r ? 1 : 0);
    for (int p = pf + tid; p <= pl; p += KW_T) {
        const long hop = (long)(p >> 1) * h;
        const long start = (p & 1) ? hop + r : hop, end = (p & 1) ? hop + h : hop + r;
        const long lo = max(start, (long)t0), hi = min(end, tend);
        if (lo >= hi || start >= N) continue;
        double sum = 0.0;
        const int c_hi = (int)((hi - 1 - t0) / KW_L);
        for (int c = (int)((lo - t0) / KW_L); c <= c_hi; ++c) sum += part[c][p - p0s[c]];
        double* out = pieces + ((size_t)b * NP + p) * 2;
        if (start >= t0) {
            out[0] = sum;
            if (end <= tend || tend >= N) out[1] = 0.0;                  // no later tile holds the rest
        } else {
            out[1] = sum;
        }
    }
}

__global__ void kw_block_kernel(const double* __restrict__ pieces, const int32_t* __restrict__ lens, double* __restrict__ z, long ldz,
                                int32_t* __restrict__ n_blocks, int NP, int n, int h, int Nmax) {
    const int b = blockIdx.y, N = kw_len(lens, b, Nmax);
    const int nb = N >= n ? (N - n) / h + 1 : 0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) n_blocks[b] = nb;
    if (i >= nb) return;
    const int q = n / h, r = n % h;
    const double* pc = pieces + (size_t)b * NP * 2;
    double sum = 0.0;
    const int p1 = 2 * (i + q) + (r > 0 ? 1 : 0);                        // one past the block's last piece
    for (int p = 2 * i; p < p1; ++p) {
        if (r == 0 && !(p & 1)) continue;
        sum += pc[2 * p];
        sum += pc[2 * p + 1];
    }
    z[(size_t)b * ldz + i] = sum / (double)n;
}

extern "C" int fs2_kweight_chunk(void) { return KW_L; }
extern "C" int fs2_kweight_chunks_per_tile(void) { return KW_T; }

static long kw_tiles(int Nmax) { return ((long)Nmax + KW_TILE - 1) / KW_TILE; }
static long kw_pieces(int Nmax, int h) { return 2L * (Nmax / h + 1); }

extern "C" int fs2_kweight_energy_ws(int B, int Nmax, int h) {
    if (B <= 0 || Nmax <= 0 || h <= 0) return 0;
    const long d = (long)B * (kw_tiles(Nmax) * (KW_T * 4 + 4) + kw_pieces(Nmax, h) * 2);
    return d < (1L << 31) ? (int)d : -1;                                  // -1: the batch is too large for one call
}

extern "C" int fs2_kweight_energy(const float* x, long ldx, const int32_t* lens, const double* coef, const double* pw, int L, int n,
                                  int h, double* z, long ldz, int32_t* n_blocks, double* ws, long ws_doubles, int B, int Nmax,
                                  hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && coef && pw && n_blocks, "kweight_energy: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldx >= Nmax, "kweight_energy: bad shape B=%d Nmax=%d ldx=%ld", B, Nmax, ldx);
    FS2_CHECK_ARG(L == KW_L && h >= KW_L && h <= KW_TILE && n >= h, "kweight_energy: bad blocks L=%d n=%d h=%d (L = %d <= h <= %d, h <= n)",
                  L, n, h, KW_L, KW_TILE);
    if (B == 0) return FS2_OK;
    const long max_blocks = Nmax >= n ? (Nmax - n) / h + 1 : 0;
    FS2_CHECK_ARG(max_blocks == 0 || (z && ldz >= max_blocks), "kweight_energy: z must hold %ld blocks per row (ldz=%ld)", max_blocks, ldz);
    const int need = fs2_kweight_energy_ws(B, Nmax, h);
    FS2_CHECK_ARG(max_blocks == 0 || (need >= 0 && ws && ws_doubles >= need), "kweight_energy: workspace of %ld doubles, %d needed (-1: batch too large)",
                  ws_doubles, need);
    const int tiles = (int)kw_tiles(Nmax), NP = (int)kw_pieces(Nmax, h);
    if (max_blocks > 0) {
        // coef is HOST memory, read here: the ten coefficients travel as kernel arguments
        const KwCoef co = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
        double* e0 = ws;
        double* T0 = e0 + (size_t)B * tiles * KW_T * 4;
        double* pieces = T0 + (size_t)B * tiles * 4;
        const dim3 grid(tiles, B);
        kw_chunk_kernel<<<grid, KW_T, 0, stream>>>(x, ldx, lens, co, pw, e0, T0, tiles, Nmax);
        FS2_CHECK_LAUNCH("kweight_energy (chunks)");
        kw_energy_kernel<<<grid, KW_T, 0, stream>>>(x, ldx, lens, co, pw, e0, T0, pieces, tiles, NP, h, n % h, Nmax);
        FS2_CHECK_LAUNCH("kweight_energy (pieces)");
        kw_block_kernel<<<dim3(fs2_cdiv(max_blocks, 256), B), 256, 0, stream>>>(pieces, lens, z, ldz, n_blocks, NP, n, h, Nmax);
        FS2_CHECK_LAUNCH("kweight_energy (blocks)");
    } else {
        if (hipMemsetAsync(n_blocks, 0, (size_t)B * sizeof(int32_t), stream) != hipSuccess) {
            fs2_set_error("kweight_energy: hipMemsetAsync failed");
            return FS2_ELAUNCH;
        }
    }
    return FS2_OK;
}

// ------------------------------------------------------------------ gating
// fixed-shape sum and maximum over the workgroup: strided per thread, xor tree per wave, waves in ascending order
static __device__ __forceinline__ double gl_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
#define GL_LOUD(z) (-0.691 + 10.0 * log10(z))
__global__ void __launch_bounds__(256) gated_loudness_kernel(const double* __restrict__ z, long ldz, const int32_t* __restrict__ n_blocks,
                                                             double* __restrict__ out, int max_blocks) {
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x, nb = min(max(n_blocks[b], 0), max_blocks);
    const double* zr = z + (size_t)b * ldz;
    double* o = out + (size_t)b * 5;
    if (nb == 0) {
        if (tid == 0) { o[0] = o[1] = __longlong_as_double(0x7ff8000000000000LL); o[2] = o[3] = o[4] = 0.0; }
        return;
    }
    double s = 0.0, c = 0.0, m = 0.0;
    for (int i = tid; i < nb; i += 256) {
        const double v = zr[i];
        m = fmax(m, v);
        if (GL_LOUD(v) > -70.0) { s += v; c += 1.0; }
    }
    const double s_abs = gl_sum(s, red), c_abs = gl_sum(c, red);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmax(m, __shfl_xor(m, k, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const double gamma = GL_LOUD(s_abs / c_abs) - 10.0;                  // NaN when nothing passed: no block passes below either
    s = 0.0, c = 0.0;
    for (int i = tid; i < nb; i += 256) {
        const double v = zr[i], l = GL_LOUD(v);
        if (l > -70.0 && l > gamma) { s += v; c += 1.0; }
    }
    const double s_rel = gl_sum(s, red), c_rel = gl_sum(c, red);
    if (tid == 0) {
        o[0] = c_abs > 0.0 ? GL_LOUD(s_rel / c_rel) : -__longlong_as_double(0x7ff0000000000000LL);
        o[1] = GL_LOUD(m);
        o[2] = (double)nb;
        o[3] = c_abs;
        o[4] = c_rel;
    }
}
extern "C" int fs2_gated_loudness(const double* z, long ldz, const int32_t* n_blocks, double* out, int B, int max_blocks,
                                  hipStream_t stream) {
    FS2_CHECK_ARG(n_blocks && out && (z || max_blocks == 0), "gated_loudness: null pointer");
    FS2_CHECK_ARG(B >= 0 && max_blocks >= 0 && ldz >= max_blocks, "gated_loudness: bad shape B=%d max_blocks=%d ldz=%ld", B, max_blocks, ldz);
    if (B == 0) return FS2_OK;
    gated_loudness_kernel<<<B, 256, 0, stream>>>(z, ldz, n_blocks, out, max_blocks);
    FS2_CHECK_LAUNCH("gated_loudness");
    return FS2_OK;
}

// ------------------------------------------------------------------ gain
__global__ void loudness_gain_kernel(const double* __restrict__ loud, long ld_loud, const float* __restrict__ peak, double target,
                                     double ceiling_db, double* __restrict__ g, int32_t* __restrict__ flags, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double L = loud[(size_t)b * ld_loud], pk = (double)peak[b];
    const double cap = pk > 0.0 ? pow(10.0, ceiling_db / 20.0) / pk : 0.0;   // an all-zero row: gain 0, zeros out
    const bool fallback = !(fabs(L) <= 1.7976931348623157e308);             // NaN or infinite loudness
    double gain = fallback ? cap : pow(10.0, (target - L) / 20.0);
    const bool limited = !fallback && gain > cap;
    if (limited) gain = cap;
    g[b] = gain;
    flags[b] = (limited ? 1 : 0) | (fallback ? 2 : 0);
}
extern "C" int fs2_loudness_gain(const double* loud, long ld_loud, const float* peak, double target, double ceiling_db, double* g,
                                 int32_t* flags, int B, hipStream_t stream) {
    FS2_CHECK_ARG(loud && peak && g && flags, "loudness_gain: null pointer");
    FS2_CHECK_ARG(B >= 0 && ld_loud >= 1 && target >= -70.0 && target <= 0.0 && ceiling_db <= 0.0,
                  "loudness_gain: bad arguments B=%d ld=%ld target=%g (in [-70, 0]) ceiling=%g (<= 0)", B, ld_loud, target, ceiling_db);
    if (B == 0) return FS2_OK;
    loudness_gain_kernel<<<fs2_cdiv(B, 256), 256, 0, stream>>>(loud, ld_loud, peak, target, ceiling_db, g, flags, B);
    FS2_CHECK_LAUNCH("loudness_gain");
    return FS2_OK;
}

// ------------------------------------------------------------------ gain + PCM cast
// pcm[b][k] = int16(clamp(rint(x g 32768), -32768, 32767)): fp64 product (the power of two is exact), rint is round-half-even;
// saturated[b] counts the samples the clamp changed (an integer count: exact in any order).  [len[b], Nmax) is zero-filled.
#define GP_PER_THREAD 4
__global__ void __launch_bounds__(256) gain_pcm_kernel(const float* __restrict__ x, long ldx, const int32_t* __restrict__ lens,
                                                       const double* __restrict__ g, int16_t* __restrict__ pcm, long ldp,
                                                       int32_t* __restrict__ saturated, int Nmax) {
    __shared__ int red[4];
    const int b = blockIdx.y, tid = threadIdx.x, N = kw_len(lens, b, Nmax);
    const int k0 = blockIdx.x * (256 * GP_PER_THREAD);
    const double gain = g[b] * 32768.0;
    int sat = 0;
#pragma unroll
    for (int u = 0; u < GP_PER_THREAD; ++u) {
        const int k = k0 + u * 256 + tid;
        if (k >= Nmax) break;
        int16_t o = 0;
        if (k < N) {
            double v = rint((double)x[(size_t)b * ldx + k] * gain);
            if (v > 32767.0) { v = 32767.0; ++sat; }
            else if (v < -32768.0) { v = -32768.0; ++sat; }
            o = v == v ? (int16_t)(int)v : (int16_t)0;
        }
        pcm[(size_t)b * ldp + k] = o;
    }
    if (k0 >= N) return;                                                 // uniform: nothing of this workgroup is inside the row
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sat += __shfl_xor(sat, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sat;
    __syncthreads();
    if (tid == 0 && red[0] + red[1] + red[2] + red[3]) atomicAdd(saturated + b, red[0] + red[1] + red[2] + red[3]);
}
extern "C" int fs2_gain_pcm(const float* x, long ldx, const int32_t* lens, const double* g, int16_t* pcm, long ldp, int32_t* saturated,
                            int B, int Nmax, hipStream_t stream) {
    FS2_CHECK_ARG(x && lens && g && pcm && saturated, "gain_pcm: null pointer");
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Nmax >= 0 && ldx >= Nmax && ldp >= Nmax, "gain_pcm: bad shape B=%d Nmax=%d ldx=%ld ldp=%ld", B,
                  Nmax, ldx, ldp);
    if (B == 0) return FS2_OK;
    if (hipMemsetAsync(saturated, 0, (size_t)B * sizeof(int32_t), stream) != hipSuccess) {
        fs2_set_error("gain_pcm: hipMemsetAsync failed");
        return FS2_ELAUNCH;
    }
    if (Nmax == 0) return FS2_OK;
    gain_pcm_kernel<<<dim3(fs2_cdiv(Nmax, 256 * GP_PER_THREAD), B), 256, 0, stream>>>(x, ldx, lens, g, pcm, ldp, saturated, Nmax);
    FS2_CHECK_LAUNCH("gain_pcm");
    return FS2_OK;
}
