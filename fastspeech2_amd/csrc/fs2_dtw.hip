// fs2_dtw.hip — objective synthesis scoring: cepstra of the log-mel (a DCT-II), dynamic time warping between two cepstral
// sequences and the F0 sums along the warping path, on ragged batches of pairs, all in fp64.
// The specification is the docstring of fastspeech2_amd/metrics.py (summarised in DESIGN.md); tests/dtw_ref.py restates it in numpy.
//
// Shapes.  Pair p has T1 = alens[p] reference frames (index i) and T2 = blens[p] synthesized frames (index j), both in [1, 2048].
// Cepstra are [B][Tmax][K] with explicit batch and frame strides.  The local costs and the backpointers of a pair are stored SKEWED:
// cell (i, j) lives at row (i + j) mod T2, column i of a [T2max][>= T1max] matrix.  Anti-diagonal s = i + j holds i in
// [max(0, s - T2 + 1), min(s, T1 - 1)] and anti-diagonal s + T2 holds i >= s + 1, so the two share a row without meeting: the
// mapping is a bijection onto the pair's own T2 x T1 corner, every anti-diagonal is contiguous in i, and the buffer is no larger
// than the unskewed one.  Nothing at a row >= T2 or a column >= T1 is read (the tests poison it with NaN) and nothing there is written.
//
//   fs2_mcep           log-mel [B][n_mel][frames] f32 -> c [B][Tmax][K] f64, c_k = sum_m x_m C[k][m] in ascending m; the host-built
//                      table C is staged in LDS, no cosine is evaluated here
//   fs2_dtw_cost       d(i, j) = sqrt(sum_k (a_k[i] - b_k[j])^2), k ascending, no fused multiply-add; 32 x 32 tiles of (i, s) with the
//                      32 rows of a and the 63 rows of b they touch staged in LDS, written in the skewed order
//   fs2_dtw_scan       one workgroup per pair, lanes over i, one anti-diagonal per step.  A lane keeps its own row's last two values
//                      in registers; the only value that crosses lanes, D(i - 1, s - 1), goes through LDS, double-buffered: one
//                      barrier per step.  Local costs are prefetched DT_PF anti-diagonals ahead into a register ring.  Backpointers
//                      leave as bytes; the accumulated cost never goes to HBM except D(T1 - 1, T2 - 1).
//   fs2_dtw_backtrack  one wave per pair: lane 0 walks the backpointers from (T1 - 1, T2 - 1), writing the path backwards into the
//                      tail of the pair's rows; the wave then moves it to the front, so the path reads from (0, 0)
//   fs2_dtw_f0         per pair the V/UV mismatches, the both-voiced count and the squared cents along the path, each lane over
//                      k = lane, lane + 256, ... ascending, then a fixed tree
//   fs2_dtw_prosody    per pair the gross pitch errors, the central sums of ln F0 on both sides (mean first, then a second pass) and
//                      the absolute energy differences along the path, summed like fs2_dtw_f0
#include "fs2_common.h"

#define DT_MAX_FRAMES 2048          // two rows per lane of the largest workgroup
#define DT_MAX_MCEP 40
#define DT_MAX_MEL 128
#define DT_TILE 32
#define DT_PF 8                     // anti-diagonals of local cost in flight per lane

static __device__ __forceinline__ int dt_len(const int32_t* lens, int b, int cap) { return min(max(lens[b], 0), cap); }
static __device__ __forceinline__ double dt_inf() { return __builtin_huge_val(); }

// ------------------------------------------------------------------ cepstra
// One frame per lane; the K rows of the table in groups of 8 accumulators (rows up to the next multiple of 8 are zero in LDS), so
// the mel column is re-read K / 8 times from cache and every table value is one LDS broadcast.
__global__ void __launch_bounds__(256) mcep_kernel(const float* __restrict__ mel, long ldm_b, long ldm_c, const int32_t* __restrict__ lens,
                                                   const double* __restrict__ table, int K, double* __restrict__ c, long ldc_b,
                                                   long ldc_t, int n_mel, int Tmax) {
    __shared__ double Cs[DT_MAX_MCEP * DT_MAX_MEL];
    const int b = blockIdx.y, tid = threadIdx.x, T = dt_len(lens, b, Tmax);
    if ((int)blockIdx.x * 256 >= T) return;
    const int Kp = (K + 7) & ~7;
    for (int k = tid; k < Kp * n_mel; k += 256) Cs[k] = k < K * n_mel ? table[k] : 0.0;
    __syncthreads();
    const int t = blockIdx.x * 256 + tid;
    if (t >= T) return;
    const float* x = mel + (size_t)b * ldm_b + t;
    double* o = c + (size_t)b * ldc_b + (size_t)t * ldc_t;
    for (int k0 = 0; k0 < K; k0 += 8) {
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const double* row = Cs + (size_t)k0 * n_mel;
        for (int m = 0; m < n_mel; ++m) {
            const double v = (double)x[(size_t)m * ldm_c];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += v * row[q * n_mel + m];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k0 + q < K) o[k0 + q] = acc[q];
    }
}
extern "C" int fs2_mcep(const float* mel, long ldm_b, long ldm_c, const int32_t* lens, const double* table, int K, double* c, long ldc_b,
                        long ldc_t, int B, int n_mel, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(mel && lens && table && c, "mcep: null pointer");
    FS2_CHECK_ARG(K >= 1 && K <= DT_MAX_MCEP && n_mel >= 1 && n_mel <= DT_MAX_MEL, "mcep: K=%d (1..%d) n_mel=%d (1..%d)", K,
                  DT_MAX_MCEP, n_mel, DT_MAX_MEL);
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && Tmax >= 0 && ldm_c >= Tmax && ldm_b >= 0 && ldc_t >= K && ldc_b >= (long)Tmax * ldc_t,
                  "mcep: bad shape B=%d Tmax=%d ldm_c=%ld ldc_b=%ld ldc_t=%ld", B, Tmax, ldm_c, ldc_b, ldc_t);
    if (B == 0 || Tmax == 0) return FS2_OK;
    mcep_kernel<<<dim3(fs2_cdiv(Tmax, 256), B), 256, 0, stream>>>(mel, ldm_b, ldm_c, lens, table, K, c, ldc_b, ldc_t, n_mel, Tmax);
    FS2_CHECK_LAUNCH("mcep");
    return FS2_OK;
}

// ------------------------------------------------------------------ local costs
// Tile of 32 rows i x 32 anti-diagonals s per 256-lane workgroup: lane (ii = tid & 31, sg = tid >> 5) owns s0 + sg + 8 q, q < 4, of
// row i0 + ii, so a wave writes two runs of 32 consecutive doubles.  j = s - i spans 63 values over the tile.  LDS rows are padded
// to an odd number of doubles.
__global__ void __launch_bounds__(256) dtw_cost_kernel(const double* __restrict__ a, long lda_b, long lda_t,
                                                       const int32_t* __restrict__ alens, const double* __restrict__ bq, long ldb_b,
                                                       long ldb_t, const int32_t* __restrict__ blens, int K, double* __restrict__ cost,
                                                       long ldd_b, long ldd_s, int T1max, int T2max) {
#pragma clang fp contract(off)
    __shared__ double as[DT_TILE][DT_MAX_MCEP + 1], bs[2 * DT_TILE - 1][DT_MAX_MCEP + 1];
    const int p = blockIdx.z, T1 = dt_len(alens, p, T1max), T2 = dt_len(blens, p, T2max);
    const int i0 = blockIdx.x * DT_TILE, s0 = blockIdx.y * DT_TILE, tid = threadIdx.x;
    const int jlo = s0 - i0 - (DT_TILE - 1);                               // j of (i0 + 31, s0); the tile's largest is jlo + 62
    if (i0 >= T1 || s0 > T1 + T2 - 2 || jlo + 2 * DT_TILE - 2 < 0 || jlo >= T2) return;
    const double* ap = a + (size_t)p * lda_b;
    const double* bp = bq + (size_t)p * ldb_b;
    for (int k = tid; k < DT_TILE * K; k += 256) {
        const int r = k / K, kk = k - r * K, i = i0 + r;
        as[r][kk] = i < T1 ? ap[(size_t)i * lda_t + kk] : 0.0;
    }
    for (int k = tid; k < (2 * DT_TILE - 1) * K; k += 256) {
        const int r = k / K, kk = k - r * K, j = jlo + r;
        bs[r][kk] = (j >= 0 && j < T2) ? bp[(size_t)j * ldb_t + kk] : 0.0;
    }
    __syncthreads();
    const int ii = tid & 31, sg = tid >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) {
        const double av = as[ii][k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double df = av - bs[sg + 8 * q - ii + DT_TILE - 1][k];
            acc[q] += df * df;
        }
    }
    const int i = i0 + ii;
    if (i >= T1) return;
    double* cp = cost + (size_t)p * ldd_b + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = s0 + sg + 8 * q, j = s - i;
        if (j >= 0 && j < T2) cp[(size_t)(s >= T2 ? (s >= 2 * T2 ? s % T2 : s - T2) : s) * ldd_s] = __dsqrt_rn(acc[q]);
    }
}

#define DT_PAIR_ARGS(name)                                                                                                        \
    FS2_CHECK_ARG(B >= 0 && B <= 65535 && T1max >= 0 && T2max >= 0, name ": bad shape B=%d T1max=%d T2max=%d", B, T1max, T2max);   \
    FS2_CHECK_ARG(T1max <= DT_MAX_FRAMES && T2max <= DT_MAX_FRAMES, name ": %d x %d frames exceed the supported maximum of %d",    \
                  T1max, T2max, DT_MAX_FRAMES)

extern "C" int fs2_dtw_max_frames(void) { return DT_MAX_FRAMES; }

extern "C" int fs2_dtw_cost(const double* a, long lda_b, long lda_t, const int32_t* alens, const double* b, long ldb_b, long ldb_t,
                            const int32_t* blens, int K, double* cost, long ldd_b, long ldd_s, int B, int T1max, int T2max,
                            hipStream_t stream) {
    FS2_CHECK_ARG(a && alens && b && blens && cost, "dtw_cost: null pointer");
    DT_PAIR_ARGS("dtw_cost");
    FS2_CHECK_ARG(K >= 1 && K <= DT_MAX_MCEP, "dtw_cost: K=%d outside 1..%d", K, DT_MAX_MCEP);
    FS2_CHECK_ARG(lda_t >= K && lda_b >= (long)T1max * lda_t && ldb_t >= K && ldb_b >= (long)T2max * ldb_t && ldd_s >= T1max &&
                      ldd_b >= (long)T2max * ldd_s,
                  "dtw_cost: bad strides a %ld %ld b %ld %ld cost %ld %ld", lda_b, lda_t, ldb_b, ldb_t, ldd_b, ldd_s);
    if (B == 0 || T1max == 0 || T2max == 0) return FS2_OK;
    dtw_cost_kernel<<<dim3(fs2_cdiv(T1max, DT_TILE), fs2_cdiv(T1max + T2max - 1, DT_TILE), B), 256, 0, stream>>>(
        a, lda_b, lda_t, alens, b, ldb_b, ldb_t, blens, K, cost, ldd_b, ldd_s, T1max, T2max);
    FS2_CHECK_LAUNCH("dtw_cost");
    return FS2_OK;
}

// ------------------------------------------------------------------ the scan
// Lane l owns rows i = l R + r, r < R.  At step s row i is at j = s - i.  With own[r] = D(i, s - 1) and own2[r] = D(i, s - 2) in
// registers, up = D(i - 1, s - 1) is own[r - 1], or for r = 0 the one LDS read edge[(s - 1) & 1][l] (slot l holds lane l - 1's last
// row, slot 0 is +inf); diag = D(i - 1, s - 2) is own2[r - 1], or the up value read one step earlier.  A cell outside the matrix is
// +inf.  Step s writes buffer s & 1 and reads (s - 1) & 1: the barrier at the top of step s + 1 orders step s's write before its
// reader and step s's read before step s + 1's overwrite of that buffer.  Code 0 diagonal, 1 (i - 1, j), 2 (i, j - 1); a later
// candidate wins only when strictly smaller, so the lowest code wins ties.  Only adds and compares of the stored costs: exact.
template <int NT, int R>
__global__ void __launch_bounds__(NT) dtw_scan_kernel(const double* __restrict__ cost, long ldd_b, long ldd_s,
                                                      const int32_t* __restrict__ alens, const int32_t* __restrict__ blens,
                                                      uint8_t* __restrict__ bp, long ldp_b, long ldp_s, double* __restrict__ total,
                                                      int T1max, int T2max) {
    __shared__ double edge[2][NT + 1];
    const int p = blockIdx.x, l = threadIdx.x;
    const int T1 = dt_len(alens, p, min(T1max, NT * R)), T2 = dt_len(blens, p, T2max);
    if (T1 == 0 || T2 == 0) {
        if (l == 0) total[p] = __builtin_nan("");
        return;
    }
    const double INF = dt_inf();
    const int i0 = l * R, nsteps = T1 + T2 - 1;
    const double* Cb = cost + (size_t)p * ldd_b + i0;
    uint8_t* Pb = bp + (size_t)p * ldp_b + i0;
    edge[0][l + 1] = edge[1][l + 1] = INF;
    if (l == 0) edge[0][0] = edge[1][0] = INF;

    double own[R], own2[R], c[DT_PF][R];
    double up2 = l == 0 ? 0.0 : INF;                                       // D(-1, -1) = 0 makes D(0, 0) = d(0, 0) by the general rule
#pragma unroll
    for (int r = 0; r < R; ++r) own[r] = own2[r] = INF;
#pragma unroll
    for (int u = 0; u < DT_PF; ++u) {
        const int row = u % T2;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r, j = u - i;
            c[u][r] = (i < T1 && j >= 0 && j < T2) ? Cb[(size_t)row * ldd_s + r] : 0.0;
        }
    }
    int row_now = 0, row_pf = DT_PF % T2;                                  // s mod T2 and (s + DT_PF) mod T2
    for (int sb = 0; sb < nsteps; sb += DT_PF) {
#pragma unroll
        for (int u = 0; u < DT_PF; ++u) {
            const int s = sb + u;                                          // steps >= nsteps have no cell inside: no load, no store
            __syncthreads();
            const double up_edge = edge[(s - 1) & 1][l];
            double nw[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = i0 + r, j = s - i;
                const bool in = i < T1 && j >= 0 && j < T2;
                const double up = r == 0 ? up_edge : own[r > 0 ? r - 1 : 0];
                const double dg = r == 0 ? up2 : own2[r > 0 ? r - 1 : 0];
                double best = dg;
                int code = 0;
                if (up < best) { best = up; code = 1; }
                if (own[r] < best) { best = own[r]; code = 2; }
                nw[r] = in ? c[u][r] + best : INF;
                if (in) {
                    Pb[(size_t)row_now * ldp_s + r] = (uint8_t)code;
                    if (i == T1 - 1 && j == T2 - 1) total[p] = nw[r];
                }
                const int jn = j + DT_PF;
                c[u][r] = (i < T1 && jn >= 0 && jn < T2) ? Cb[(size_t)row_pf * ldd_s + r] : 0.0;
            }
            up2 = up_edge;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                own2[r] = own[r];
                own[r] = nw[r];
            }
            edge[s & 1][l + 1] = nw[R - 1];
            row_now = row_now + 1 == T2 ? 0 : row_now + 1;
            row_pf = row_pf + 1 == T2 ? 0 : row_pf + 1;
        }
    }
}

extern "C" int fs2_dtw_scan(const double* cost, long ldd_b, long ldd_s, const int32_t* alens, const int32_t* blens, uint8_t* bp,
                            long ldp_b, long ldp_s, double* total, int B, int T1max, int T2max, hipStream_t stream) {
    FS2_CHECK_ARG(cost && alens && blens && bp && total, "dtw_scan: null pointer");
    DT_PAIR_ARGS("dtw_scan");
    FS2_CHECK_ARG(ldd_s >= T1max && ldd_b >= (long)T2max * ldd_s && ldp_s >= T1max && ldp_b >= (long)T2max * ldp_s,
                  "dtw_scan: bad strides cost %ld %ld bp %ld %ld", ldd_b, ldd_s, ldp_b, ldp_s);
    if (B == 0) return FS2_OK;
#define DT_SCAN(NT, R) dtw_scan_kernel<NT, R><<<B, NT, 0, stream>>>(cost, ldd_b, ldd_s, alens, blens, bp, ldp_b, ldp_s, total, T1max, T2max)
    if (T1max <= 256) DT_SCAN(256, 1); else if (T1max <= 512) DT_SCAN(512, 1); else if (T1max <= 1024) DT_SCAN(1024, 1); else DT_SCAN(1024, 2);
#undef DT_SCAN
    FS2_CHECK_LAUNCH("dtw_scan");
    return FS2_OK;
}

// ------------------------------------------------------------------ backtrack
// Lane 0 walks at most T1 + T2 - 1 cells back from (T1 - 1, T2 - 1) and writes cell number k of the walk at L - 1 - k, L = T1 + T2 - 1;
// the wave then moves the P cells from [L - P, L) to [0, P), 64 at a time (a chunk is read whole before it is written, and a later
// chunk reads only above what an earlier one wrote), and sets [P, L) to -1.  Nothing at k >= L is written.  A code that would leave
// the matrix ends the walk (not a path of this scan: stop rather than read outside).
__global__ void __launch_bounds__(64) dtw_backtrack_kernel(const uint8_t* __restrict__ bp, long ldp_b, long ldp_s,
                                                           const int32_t* __restrict__ alens, const int32_t* __restrict__ blens,
                                                           int32_t* pi, int32_t* pj, long ldq, int32_t* __restrict__ plen, int T1max,
                                                           int T2max) {
    __shared__ int P_sh;
    const int p = blockIdx.x, lane = threadIdx.x, T1 = dt_len(alens, p, T1max), T2 = dt_len(blens, p, T2max);
    if (T1 == 0 || T2 == 0) {
        if (lane == 0) plen[p] = 0;
        return;
    }
    const int L = T1 + T2 - 1;
    int32_t* qi = pi + (size_t)p * ldq;
    int32_t* qj = pj + (size_t)p * ldq;
    if (lane == 0) {
        const uint8_t* Pb = bp + (size_t)p * ldp_b;
        int i = T1 - 1, j = T2 - 1, k = 0, row = (i + j) % T2;
        for (;;) {
            qi[L - 1 - k] = i;
            qj[L - 1 - k] = j;
            ++k;
            if ((i == 0 && j == 0) || k >= L) break;
            const int code = Pb[(size_t)row * ldp_s + i];
            const int ni = code == 2 ? i : i - 1, nj = code == 1 ? j : j - 1;
            if (ni < 0 || nj < 0) break;
            row -= (i - ni) + (j - nj);
            if (row < 0) row += T2;
            if (row < 0) row += T2;                                        // T2 = 1 and a diagonal step
            i = ni;
            j = nj;
        }
        P_sh = k;
    }
    __syncthreads();
    const int P = P_sh, off = L - P;
    if (off > 0) {
        for (int k0 = 0; k0 < P; k0 += 64) {
            const int k = k0 + lane;
            int vi = 0, vj = 0;
            if (k < P) {
                vi = qi[off + k];
                vj = qj[off + k];
            }
            __syncthreads();
            if (k < P) {
                qi[k] = vi;
                qj[k] = vj;
            }
            __syncthreads();
        }
        for (int k = P + lane; k < L; k += 64) qi[k] = qj[k] = -1;
    }
    if (lane == 0) plen[p] = P;
}
extern "C" int fs2_dtw_backtrack(const uint8_t* bp, long ldp_b, long ldp_s, const int32_t* alens, const int32_t* blens, int32_t* pi,
                                 int32_t* pj, long ldq, int32_t* plen, int B, int T1max, int T2max, hipStream_t stream) {
    FS2_CHECK_ARG(bp && alens && blens && pi && pj && plen, "dtw_backtrack: null pointer");
    DT_PAIR_ARGS("dtw_backtrack");
    FS2_CHECK_ARG(pi != pj && ldp_s >= T1max && ldp_b >= (long)T2max * ldp_s && ldq >= (long)T1max + T2max - 1,
                  "dtw_backtrack: bad strides bp %ld %ld path %ld", ldp_b, ldp_s, ldq);
    if (B == 0) return FS2_OK;
    dtw_backtrack_kernel<<<B, 64, 0, stream>>>(bp, ldp_b, ldp_s, alens, blens, pi, pj, ldq, plen, T1max, T2max);
    FS2_CHECK_LAUNCH("dtw_backtrack");
    return FS2_OK;
}

// ------------------------------------------------------------------ F0 along the path
// sums[p] = {pairs where exactly one of r, s is 0, pairs with r > 0 and s > 0, sum over those of (1200 log2(s / r))^2} with
// r = f0_ref[pi[k]], s = f0_syn[pj[k]].  A path entry outside the pair's frames is skipped, never followed.
__global__ void __launch_bounds__(256) dtw_f0_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, long ldq,
                                                     const int32_t* __restrict__ plen, const double* __restrict__ f0r, long ldr,
                                                     const double* __restrict__ f0s, long lds, const int32_t* __restrict__ alens,
                                                     const int32_t* __restrict__ blens, double* __restrict__ sums, long ldo,
                                                     int T1max, int T2max) {
    __shared__ double red[3][256];
    const int p = blockIdx.x, tid = threadIdx.x, T1 = dt_len(alens, p, T1max), T2 = dt_len(blens, p, T2max);
    const int P = (int)min((long)max(plen[p], 0), ldq);
    const int32_t* qi = pi + (size_t)p * ldq;
    const int32_t* qj = pj + (size_t)p * ldq;
    const double* fr = f0r + (size_t)p * ldr;
    const double* fs = f0s + (size_t)p * lds;
    double mism = 0.0, voiced = 0.0, sq = 0.0;
    for (int k = tid; k < P; k += 256) {
        const int i = qi[k], j = qj[k];
        if (i < 0 || i >= T1 || j < 0 || j >= T2) continue;
        const double r = fr[i], s = fs[j];
        if ((r == 0.0) != (s == 0.0)) mism += 1.0;
        if (r > 0.0 && s > 0.0) {
            const double cents = 1200.0 * log2(s / r);
            voiced += 1.0;
            sq += cents * cents;
        }
    }
    red[0][tid] = mism;
    red[1][tid] = voiced;
    red[2][tid] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                                   // fixed tree: the same sums on every run
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
            red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
    }
    if (tid < 3) sums[(size_t)p * ldo + tid] = red[tid][0];
}
extern "C" int fs2_dtw_f0(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* f0_ref, long ldr,
                          const double* f0_syn, long lds, const int32_t* alens, const int32_t* blens, double* sums, long ldo, int B,
                          int T1max, int T2max, hipStream_t stream) {
    FS2_CHECK_ARG(pi && pj && plen && f0_ref && f0_syn && alens && blens && sums, "dtw_f0: null pointer");
    DT_PAIR_ARGS("dtw_f0");
    FS2_CHECK_ARG(ldq >= 0 && ldr >= T1max && lds >= T2max && ldo >= 3, "dtw_f0: bad strides path %ld f0 %ld %ld sums %ld", ldq, ldr,
                  lds, ldo);
    if (B == 0) return FS2_OK;
    dtw_f0_kernel<<<B, 256, 0, stream>>>(pi, pj, ldq, plen, f0_ref, ldr, f0_syn, lds, alens, blens, sums, ldo, T1max, T2max);
    FS2_CHECK_LAUNCH("dtw_f0");
    return FS2_OK;
}

// ------------------------------------------------------------------ prosody along the path
// Over the path cells with r = f0_ref[pi[k]], s = f0_syn[pj[k]], V the cells with r > 0 and s > 0, x = ln r, y = ln s over V, and
// er = e_ref[pi[k]], es = e_syn[pj[k]] (float32 promoted):
//   sums[p] = {gross = cells of V with fabs(s - r) > 0.2 r, n = |V|, cells where exactly one of r, s is 0,
//              Sxx = sum (x - xm)^2, Syy = sum (y - ym)^2, Sxy = sum (x - xm)(y - ym), sum |er - es|, sum er}
// with xm = (sum x) / n and ym = (sum y) / n from a first pass; the second pass evaluates the logarithms again rather than keep up
// to 4095 pairs of them.  The comparison is one subtraction and one product, unfused.  A path entry outside the pair is skipped.
#define DT_PROSODY_SUMS 8
static __device__ __forceinline__ void dt_tree(double (*red)[256], int rows, int tid) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                                   // fixed tree: the same sums on every run
        if (tid < o)
            for (int q = 0; q < rows; ++q) red[q][tid] += red[q][tid + o];
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) dtw_prosody_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, long ldq,
                                                          const int32_t* __restrict__ plen, const double* __restrict__ f0r, long ldr,
                                                          const double* __restrict__ f0s, long lds, const float* __restrict__ er,
                                                          long lder, const float* __restrict__ es, long ldes,
                                                          const int32_t* __restrict__ alens, const int32_t* __restrict__ blens,
                                                          double* __restrict__ sums, long ldo, int T1max, int T2max) {
#pragma clang fp contract(off)
    __shared__ double red[7][256];
    const int p = blockIdx.x, tid = threadIdx.x, T1 = dt_len(alens, p, T1max), T2 = dt_len(blens, p, T2max);
    const int P = (int)min((long)max(plen[p], 0), ldq);
    const int32_t* qi = pi + (size_t)p * ldq;
    const int32_t* qj = pj + (size_t)p * ldq;
    const double* fr = f0r + (size_t)p * ldr;
    const double* fs = f0s + (size_t)p * lds;
    const float* pr = er + (size_t)p * lder;
    const float* ps = es + (size_t)p * ldes;
    double gross = 0.0, voiced = 0.0, mism = 0.0, sx = 0.0, sy = 0.0, de = 0.0, se = 0.0;
    for (int k = tid; k < P; k += 256) {
        const int i = qi[k], j = qj[k];
        if (i < 0 || i >= T1 || j < 0 || j >= T2) continue;
        const double r = fr[i], s = fs[j], a = (double)pr[i], b = (double)ps[j];
        if ((r == 0.0) != (s == 0.0)) mism += 1.0;
        if (r > 0.0 && s > 0.0) {
            const double diff = s - r, bound = 0.2 * r;
            if (fabs(diff) > bound) gross += 1.0;
            voiced += 1.0;
            sx += log(r);
            sy += log(s);
        }
        de += fabs(a - b);
        se += a;
    }
    red[0][tid] = gross;
    red[1][tid] = voiced;
    red[2][tid] = mism;
    red[3][tid] = sx;
    red[4][tid] = sy;
    red[5][tid] = de;
    red[6][tid] = se;
    dt_tree(red, 7, tid);
    const double n = red[1][0];
    const double xm = n > 0.0 ? red[3][0] / n : 0.0, ym = n > 0.0 ? red[4][0] / n : 0.0;
    double* o = sums + (size_t)p * ldo;
    if (tid == 0) {
        o[0] = red[0][0];
        o[1] = n;
        o[2] = red[2][0];
        o[6] = red[5][0];
        o[7] = red[6][0];
    }
    __syncthreads();                                                       // everyone has read the means before red is reused
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = tid; k < P; k += 256) {
        const int i = qi[k], j = qj[k];
        if (i < 0 || i >= T1 || j < 0 || j >= T2) continue;
        const double r = fr[i], s = fs[j];
        if (r > 0.0 && s > 0.0) {
            const double dx = log(r) - xm, dy = log(s) - ym;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
        }
    }
    red[0][tid] = sxx;
    red[1][tid] = syy;
    red[2][tid] = sxy;
    dt_tree(red, 3, tid);
    if (tid < 3) o[3 + tid] = red[tid][0];
}
extern "C" int fs2_dtw_prosody(const int32_t* pi, const int32_t* pj, long ldq, const int32_t* plen, const double* f0_ref, long ldr,
                               const double* f0_syn, long lds, const float* e_ref, long lder, const float* e_syn, long ldes,
                               const int32_t* alens, const int32_t* blens, double* sums, long ldo, int B, int T1max, int T2max,
                               hipStream_t stream) {
    FS2_CHECK_ARG(pi && pj && plen && f0_ref && f0_syn && e_ref && e_syn && alens && blens && sums, "dtw_prosody: null pointer");
    DT_PAIR_ARGS("dtw_prosody");
    FS2_CHECK_ARG(ldq >= 0 && ldr >= T1max && lds >= T2max && lder >= T1max && ldes >= T2max && ldo >= DT_PROSODY_SUMS,
                  "dtw_prosody: bad strides path %ld f0 %ld %ld energy %ld %ld sums %ld", ldq, ldr, lds, lder, ldes, ldo);
    if (B == 0) return FS2_OK;
    dtw_prosody_kernel<<<B, 256, 0, stream>>>(pi, pj, ldq, plen, f0_ref, ldr, f0_syn, lds, e_ref, lder, e_syn, ldes, alens, blens, sums,
                                              ldo, T1max, T2max);
    FS2_CHECK_LAUNCH("dtw_prosody");
    return FS2_OK;
}
