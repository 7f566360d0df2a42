// fs2_cwt.hip — the wavelet prosody scores: the interpolated, normalised continuous ln F0 of an F0 track, its continuous wavelet
// transform (Mexican hat, ten scales one octave apart) and the correlation sums of the ten scales and five levels of two such
// transforms along a DTW path.  fp64, ragged batches of rows of at most 2048 frames.  The specification is the docstring of
// fastspeech2_amd/cwt.py; tests/cwt_ref.py restates it in numpy (explicit loops, an FFT convolution).
//
// Every sum here is a compensated sum of fs2_comp.h, per lane in ascending order and then over the 256 lanes by its fixed tree.  No
// atomics; nothing at a frame >= lens[b] is read or written; the same input gives the same bytes, and a row's bytes do not depend
// on the rows beside it (a workgroup sees one row only).
//
//   fs2_cwt_contour    one workgroup per row, the row in LDS.  x = ln f0 at the voiced frames (f0 > 0).  The previous and the next
//                      voiced frame of every frame are an inclusive forward max-scan of (voiced ? t : -1) and a backward min-scan of
//                      (voiced ? t : T), both by doubling (11 steps at T = 2048) between two LDS buffers.  An unvoiced frame is
//                      x[t0] + (x[t1] - x[t0]) * ((t - t0) / (t1 - t0)) evaluated as written, or the nearest voiced value at the
//                      ends.  Then the mean, the deviation about it in a second pass, and z = (x - m) / sd.
//   fs2_cwt_transform  one workgroup per (row, scale): z and the scale's table in LDS (32 KiB).  Lane l owns frame t = t0 + l of a
//                      tile of 256 and walks d = u - t ascending over the table's support clipped to the tile: the z read is
//                      unit-stride across the lanes, the table read a broadcast, both conflict-free.  A u outside [0, T) adds an
//                      exact zero, so every frame sums its terms in ascending u.  About 8 fp64 operations per term: the loop is
//                      bound by arithmetic, which the four waves of a workgroup (several workgroups fit a CU) keep issued.
//   fs2_cwt_on_path    one workgroup per (pair, component): component c < 10 is scale c, component 10 + j the level W_2j + W_2j+1
//                      (0-based), formed at every path cell.  A first pass for the two means, a second for Sxx, Syy, Sxy, Sd2.
#include "fs2_comp.h"

#define CW_MAX_FRAMES 2048          // = fs2_dtw_max_frames()
#define CW_NT 256
#define CW_SCALES 10
#define CW_LEVELS 5
#define CW_COMP (CW_SCALES + CW_LEVELS)
#define CW_FLAT_SD 1e-12

struct CwSupport {
    int n[CW_SCALES];               // the table of scale i holds d = 0 .. n[i] - 1
};

#pragma clang fp contract(off)

static __device__ __forceinline__ int cw_len(const int32_t* lens, int b, int Tmax) { return min(lens[b], min(Tmax, CW_MAX_FRAMES)); }

// ------------------------------------------------------------------ the continuous, normalised ln F0
__global__ void __launch_bounds__(CW_NT) cwt_contour_kernel(const double* __restrict__ f0, long ldf, const int32_t* __restrict__ lens,
                                                            double* __restrict__ z, long ldz, double* __restrict__ stats, long lds,
                                                            int Tmax) {
    __shared__ double x[CW_MAX_FRAMES];
    __shared__ int prv[2][CW_MAX_FRAMES];
    __shared__ int nxt[2][CW_MAX_FRAMES];
    __shared__ double rs[CW_NT], re[CW_NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = cw_len(lens, b, Tmax);
    if (T < 1) return;                                                      // the whole workgroup: no barrier is skipped by a part of it
    const double* f = f0 + (size_t)b * ldf;
    double count = 0.0;
    for (int t = tid; t < T; t += CW_NT) {
        const double v = f[t];
        const bool voiced = v > 0.0;
        x[t] = voiced ? log(v) : 0.0;
        prv[0][t] = voiced ? t : -1;
        nxt[0][t] = voiced ? t : T;
        count += voiced ? 1.0 : 0.0;
    }
    __syncthreads();
    int c = 0;
    for (int off = 1; off < T; off <<= 1, c ^= 1) {
        for (int t = tid; t < T; t += CW_NT) {
            int p = prv[c][t], n = nxt[c][t];
            if (t >= off) p = max(p, prv[c][t - off]);
            if (t + off < T) n = min(n, nxt[c][t + off]);
            prv[c ^ 1][t] = p;
            nxt[c ^ 1][t] = n;
        }
        __syncthreads();
    }
    const double nv = cs_block_sum<CW_NT>(count, 0.0, rs, re, tid);         // small integers: exact
    double m = 0.0, sd = 0.0;
    if (nv > 0.0) {                                                         // the same for every lane
        for (int t = tid; t < T; t += CW_NT) {
            const int t0 = prv[c][t], t1 = nxt[c][t];
            if (t0 == t) continue;                                          // voiced: written once, above, and only read from here on
            double v;
            if (t0 < 0) {
                v = x[t1];
            } else if (t1 >= T) {
                v = x[t0];
            } else {
                const double x0 = x[t0], x1 = x[t1];
                const double frac = (double)(t - t0) / (double)(t1 - t0);
                v = x0 + (x1 - x0) * frac;
            }
            x[t] = v;
        }
        __syncthreads();
        double s = 0.0, e = 0.0;
        for (int t = tid; t < T; t += CW_NT) cs_add(s, e, x[t]);
        m = cs_block_sum<CW_NT>(s, e, rs, re, tid) / (double)T;
        s = 0.0, e = 0.0;
        for (int t = tid; t < T; t += CW_NT) {
            const double d = x[t] - m;
            cs_fma(s, e, d, d);
        }
        sd = sqrt(cs_block_sum<CW_NT>(s, e, rs, re, tid) / (double)T);
    }
    const bool flat = !(nv > 0.0) || !(sd > CW_FLAT_SD);
    double* zr = z + (size_t)b * ldz;
    for (int t = tid; t < T; t += CW_NT) zr[t] = flat ? 0.0 : (x[t] - m) / sd;
    if (tid == 0) {
        double* q = stats + (size_t)b * lds;
        q[0] = nv;
        q[1] = m;
        q[2] = sd;
        q[3] = flat ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------ the transform
__global__ void __launch_bounds__(CW_NT) cwt_transform_kernel(const double* __restrict__ z, long ldz, const int32_t* __restrict__ lens,
                                                              const double* __restrict__ tab, long ldt, CwSupport sup,
                                                              double* __restrict__ W, long ldw_b, long ldw_i,
                                                              double* __restrict__ power, long ldp, int Tmax) {
    __shared__ double zs[CW_MAX_FRAMES];
    __shared__ double ts[CW_MAX_FRAMES];
    __shared__ double rs[CW_NT], re[CW_NT];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int T = cw_len(lens, b, Tmax);
    if (T < 1) return;
    const int n = min(max(sup.n[i], 1), CW_MAX_FRAMES), R = n - 1;
    const double* zr = z + (size_t)b * ldz;
    const double* tr = tab + (size_t)i * ldt;
    for (int t = tid; t < T; t += CW_NT) zs[t] = zr[t];
    for (int d = tid; d < n; d += CW_NT) ts[d] = tr[d];
    __syncthreads();
    double* wr = W + (size_t)b * ldw_b + (size_t)i * ldw_i;
    double ps = 0.0, pe = 0.0;
    for (int t0 = 0; t0 < T; t0 += CW_NT) {
        const int t = t0 + tid;
        const int dlo = max(-R, -min(t0 + CW_NT - 1, T - 1)), dhi = min(R, T - 1 - t0);     // the d at which some frame of the tile has a u in [0, T)
        double s = 0.0, e = 0.0;
        for (int d = dlo; d <= dhi; ++d) {
            const int u = t + d;
            const double zv = (u >= 0 && u < T) ? zs[u] : 0.0;
            cs_fma(s, e, zv, ts[d < 0 ? -d : d]);
        }
        if (t < T) {
            const double w = s + e;
            wr[t] = w;
            cs_fma(ps, pe, w, w);
        }
    }
    const double total = cs_block_sum<CW_NT>(ps, pe, rs, re, tid);
    if (tid == 0) power[(size_t)b * ldp + i] = total;
}

// ------------------------------------------------------------------ the sums along the path
__global__ void __launch_bounds__(CW_NT) cwt_on_path_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, long ldq,
                                                            const int32_t* __restrict__ plen, const double* __restrict__ wr, long ldr_b,
                                                            long ldr_i, const double* __restrict__ ws, long lds_b, long lds_i,
                                                            const int32_t* __restrict__ alens, const int32_t* __restrict__ blens,
                                                            double* __restrict__ sums, long ldo_b, long ldo_c, int T1max, int T2max) {
    __shared__ double rs[CW_NT], re[CW_NT];
    const int comp = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int T1 = cw_len(alens, p, T1max), T2 = cw_len(blens, p, T2max);
    const int P = (int)min((long)max(plen[p], 0), ldq);
    const bool level = comp >= CW_SCALES;
    const int c0 = level ? 2 * (comp - CW_SCALES) : comp;
    const int32_t* qi = pi + (size_t)p * ldq;
    const int32_t* qj = pj + (size_t)p * ldq;
    const double* a0 = wr + (size_t)p * ldr_b + (size_t)c0 * ldr_i;
    const double* b0 = ws + (size_t)p * lds_b + (size_t)c0 * lds_i;
    const double* a1 = a0 + (level ? ldr_i : 0);
    const double* b1 = b0 + (level ? lds_i : 0);
    double sx = 0.0, ex = 0.0, sy = 0.0, ey = 0.0, count = 0.0;
    for (int k = tid; k < P; k += CW_NT) {
        const int i = qi[k], j = qj[k];
        if (i < 0 || i >= T1 || j < 0 || j >= T2) continue;                 // a path entry outside the pair is skipped, never followed
        const double x = level ? a0[i] + a1[i] : a0[i], y = level ? b0[j] + b1[j] : b0[j];
        cs_add(sx, ex, x);
        cs_add(sy, ey, y);
        count += 1.0;
    }
    const double n = cs_block_sum<CW_NT>(count, 0.0, rs, re, tid);
    double* o = sums + (size_t)p * ldo_b + (size_t)comp * ldo_c;
    if (!(n > 0.0)) {                                                       // the same for every lane
        if (tid < 4) o[tid] = 0.0;
        return;
    }
    const double xm = cs_block_sum<CW_NT>(sx, ex, rs, re, tid) / n, ym = cs_block_sum<CW_NT>(sy, ey, rs, re, tid) / n;
    double sxx = 0.0, exx = 0.0, syy = 0.0, eyy = 0.0, sxy = 0.0, exy = 0.0, sd2 = 0.0, ed2 = 0.0;
    for (int k = tid; k < P; k += CW_NT) {
        const int i = qi[k], j = qj[k];
        if (i < 0 || i >= T1 || j < 0 || j >= T2) continue;
        const double x = level ? a0[i] + a1[i] : a0[i], y = level ? b0[j] + b1[j] : b0[j];
        const double dx = x - xm, dy = y - ym, dd = x - y;
        cs_fma(sxx, exx, dx, dx);
        cs_fma(syy, eyy, dy, dy);
        cs_fma(sxy, exy, dx, dy);
        cs_fma(sd2, ed2, dd, dd);
    }
    const double r0 = cs_block_sum<CW_NT>(sxx, exx, rs, re, tid), r1 = cs_block_sum<CW_NT>(syy, eyy, rs, re, tid);
    const double r2 = cs_block_sum<CW_NT>(sxy, exy, rs, re, tid), r3 = cs_block_sum<CW_NT>(sd2, ed2, rs, re, tid);
    if (tid == 0) {
        o[0] = r0;
        o[1] = r1;
        o[2] = r2;
        o[3] = r3;
    }
}

// ------------------------------------------------------------------ the C ABI
extern "C" int fs2_cwt_scales(void) { return CW_SCALES; }

extern "C" int fs2_cwt_contour(const double* f0, long ldf, const int32_t* lens, double* z, long ldz, double* stats, long lds, int B,
                               int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && Tmax >= 1 && Tmax <= CW_MAX_FRAMES, "cwt_contour: bad shape B=%d Tmax=%d (1..%d frames)", B, Tmax, CW_MAX_FRAMES);
    FS2_CHECK_ARG(ldf >= Tmax && ldz >= Tmax && lds >= 4, "cwt_contour: bad strides f0 %ld z %ld stats %ld", ldf, ldz, lds);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(f0 && lens && z && stats, "cwt_contour: null pointer");
    FS2_CHECK_ARG(f0 != z, "cwt_contour: the contour cannot be written over the track");
    cwt_contour_kernel<<<B, CW_NT, 0, stream>>>(f0, ldf, lens, z, ldz, stats, lds, Tmax);
    FS2_CHECK_LAUNCH("cwt_contour");
    return FS2_OK;
}

extern "C" int fs2_cwt_transform(const double* z, long ldz, const int32_t* lens, const double* tab, long ldt, const int32_t* support,
                                 double* w, long ldw_b, long ldw_i, double* power, long ldp, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && Tmax >= 1 && Tmax <= CW_MAX_FRAMES, "cwt_transform: bad shape B=%d Tmax=%d (1..%d frames)", B, Tmax, CW_MAX_FRAMES);
    FS2_CHECK_ARG(B <= 65535, "cwt_transform: %d rows, supported are at most 65535 per launch", B);
    FS2_CHECK_ARG(support, "cwt_transform: null pointer");
    CwSupport sup;
    for (int i = 0; i < CW_SCALES; ++i) {
        sup.n[i] = support[i];
        FS2_CHECK_ARG(sup.n[i] >= 1 && sup.n[i] <= CW_MAX_FRAMES && sup.n[i] <= ldt, "cwt_transform: the table of scale %d has %d entries, not 1..%ld",
                      i + 1, sup.n[i], ldt < CW_MAX_FRAMES ? ldt : (long)CW_MAX_FRAMES);
    }
    FS2_CHECK_ARG(ldz >= Tmax && ldw_i >= Tmax && ldw_b >= (long)CW_SCALES * ldw_i && ldp >= CW_SCALES,
                  "cwt_transform: bad strides z %ld w %ld %ld power %ld", ldz, ldw_b, ldw_i, ldp);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(z && lens && tab && w && power, "cwt_transform: null pointer");
    cwt_transform_kernel<<<dim3(CW_SCALES, B), CW_NT, 0, stream>>>(z, ldz, lens, tab, ldt, sup, w, ldw_b, ldw_i, power, ldp, Tmax);
    FS2_CHECK_LAUNCH("cwt_transform");
    return FS2_OK;
}

extern "C" int fs2_cwt_on_path(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* w_ref, long ldr_b,
                               long ldr_i, const double* w_syn, long lds_b, long lds_i, const int32_t* alens, const int32_t* blens,
                               double* sums, long ldo_b, long ldo_c, int B, int T1max, int T2max, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && T1max >= 1 && T2max >= 1 && T1max <= CW_MAX_FRAMES && T2max <= CW_MAX_FRAMES,
                  "cwt_on_path: bad shape B=%d T1max=%d T2max=%d (1..%d frames)", B, T1max, T2max, CW_MAX_FRAMES);
    FS2_CHECK_ARG(B <= 65535, "cwt_on_path: %d pairs, supported are at most 65535 per launch", B);
    FS2_CHECK_ARG(ldq >= 0 && ldr_i >= T1max && ldr_b >= (long)CW_SCALES * ldr_i && lds_i >= T2max && lds_b >= (long)CW_SCALES * lds_i &&
                      ldo_c >= 4 && ldo_b >= (long)CW_COMP * ldo_c,
                  "cwt_on_path: bad strides path %ld w_ref %ld %ld w_syn %ld %ld sums %ld %ld", ldq, ldr_b, ldr_i, lds_b, lds_i, ldo_b, ldo_c);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(pi && pj && plen && w_ref && w_syn && alens && blens && sums, "cwt_on_path: null pointer");
    cwt_on_path_kernel<<<dim3(CW_COMP, B), CW_NT, 0, stream>>>(pi, pj, ldq, plen, w_ref, ldr_b, ldr_i, w_syn, lds_b, lds_i, alens, blens,
                                                               sums, ldo_b, ldo_c, T1max, T2max);
    FS2_CHECK_LAUNCH("cwt_on_path");
    return FS2_OK;
}
