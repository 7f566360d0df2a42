// fs2_prosody.hip — the per-side half of the prosody scores: the voiced frames of an F0 track compacted to the front of a row, and
// their count, mean and central sums.  fp64, ragged batches, one workgroup per utterance.  The specification is the docstring of
// fastspeech2_amd/metrics.py ('Prosody'); tests/prosody_ref.py restates it in numpy.  The sums along the warping path are
// fs2_dtw_prosody in fs2_dtw.hip; the pitch-contour DTW reuses fs2_dtw_cost / _scan / _backtrack with K = 1.
//
//   fs2_prosody_voiced  row b has T = lens[b] <= 2048 frames.  The row is taken in chunks of 256 frames, one per lane.  Within a
//                       chunk the exclusive scan of the voiced flags (f0 > 0) is a ballot and a population count per wave, plus the
//                       totals of the waves in front, which go through LDS (double-buffered: one barrier per chunk); the carry of
//                       the chunks in front is a register every lane keeps.  Frame t goes to position carry + scan: the order of the
//                       frames is kept.  The contour is written to the output row and to LDS, from where the two passes of the
//                       moments read it: lane l sums the values l, l + 256, ... ascending, then a fixed tree over the 256 lanes.
//                       Nothing at a frame >= T is read; the output row is written at [0, n_v) only.  No atomics.
#include "fs2_common.h"

#define PR_MAX_FRAMES 2048          // = fs2_dtw_max_frames(): the contour of a row fits in LDS
#define PR_NT 256

// The sum of v over the workgroup by a fixed tree, the same on every run.  Every lane gets it; `red` may be reused after the call.
static __device__ __forceinline__ double pr_block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int o = PR_NT / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(PR_NT) prosody_voiced_kernel(const double* __restrict__ f0, long ldf, const int32_t* __restrict__ lens,
                                                               double* __restrict__ out, long ldo, int32_t* __restrict__ nv,
                                                               double* __restrict__ stats, long lds, int Tmax) {
    __shared__ double u[PR_MAX_FRAMES];
    __shared__ double red[PR_NT];
    __shared__ int wtot[2][PR_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = min(max(lens[b], 0), min(Tmax, PR_MAX_FRAMES));
    const double* x = f0 + (size_t)b * ldf;
    double* o = out + (size_t)b * ldo;
    int carry = 0;
    for (int t0 = 0, c = 0; t0 < T; t0 += PR_NT, c ^= 1) {
        const int t = t0 + tid;
        const double v = t < T ? x[t] : 0.0;
        const bool voiced = v > 0.0;
        const unsigned long long mask = __ballot(voiced);
        if (lane == 0) wtot[c][wave] = __popcll(mask);
        __syncthreads();                                                   // the next chunk writes the other buffer: one barrier
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PR_NT / 64; ++w) {
            const int n = wtot[c][w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (voiced) {
            const int k = carry + before + __popcll(mask & ((1ull << lane) - 1ull));
            u[k] = v;
            o[k] = v;
        }
        carry += total;
    }
    __syncthreads();
    const int n = carry;
    double s = 0.0;
    for (int k = tid; k < n; k += PR_NT) s += u[k];
    s = pr_block_sum(s, red, tid);
    const double mean = n > 0 ? s / (double)n : 0.0;
    double m2 = 0.0, m3 = 0.0, m4 = 0.0;
    for (int k = tid; k < n; k += PR_NT) {
        const double d = u[k] - mean, d2 = d * d;
        m2 += d2;
        m3 += d2 * d;
        m4 += d2 * d2;
    }
    m2 = pr_block_sum(m2, red, tid);
    m3 = pr_block_sum(m3, red, tid);
    m4 = pr_block_sum(m4, red, tid);
    if (tid == 0) {
        double* q = stats + (size_t)b * lds;
        nv[b] = n;
        q[0] = (double)n;
        q[1] = mean;
        q[2] = m2;
        q[3] = m3;
        q[4] = m4;
    }
}

extern "C" int fs2_prosody_voiced(const double* f0, long ldf, const int32_t* lens, double* out, long ldo, int32_t* nv, double* stats,
                                  long lds, int B, int Tmax, hipStream_t stream) {
    FS2_CHECK_ARG(f0 && lens && out && nv && stats, "prosody_voiced: null pointer");
    FS2_CHECK_ARG(B >= 0 && Tmax >= 0, "prosody_voiced: bad shape B=%d Tmax=%d", B, Tmax);
    FS2_CHECK_ARG(Tmax <= PR_MAX_FRAMES, "prosody_voiced: %d frames exceed the supported maximum of %d", Tmax, PR_MAX_FRAMES);
    FS2_CHECK_ARG(ldf >= Tmax && ldo >= Tmax && lds >= 5, "prosody_voiced: bad strides f0 %ld out %ld stats %ld", ldf, ldo, lds);
    FS2_CHECK_ARG(f0 != out, "prosody_voiced: the contour cannot be compacted in place");
    if (B == 0) return FS2_OK;
    prosody_voiced_kernel<<<B, PR_NT, 0, stream>>>(f0, ldf, lens, out, ldo, nv, stats, lds, Tmax);
    FS2_CHECK_LAUNCH("prosody_voiced");
    return FS2_OK;
}
