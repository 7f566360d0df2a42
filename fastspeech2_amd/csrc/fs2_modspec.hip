// fs2_modspec.hip — the over-smoothing scores of a cepstral trajectory: its mean and central sum of squares over time (global
// variance) and the log power spectrum of the mean-removed trajectory over time (modulation spectrum), full resolution and
// averaged over bands of bins.  fp64, ragged batches c [B][Tmax][K] with strides in elements and unit stride in k.  The
// specification is the docstring of fastspeech2_amd/modspec.py; tests/modspec_ref.py restates it in numpy with an FFT.
//
// Every sum here is a compensated sum of fs2_comp.h over its terms in ascending order in one thread.  No atomics, no cross-lane
// reduction: the same input gives the same bytes.  The transform's sizes are those of fs2_modspec.h, which the postfilter
// (fs2_msfilter.hip) shares.
//
//   fs2_traj_moments  one thread per (b, k), lanes along k so that a wave reads contiguous coefficients of one frame.  Two passes
//                     over t < lens[b]: the sum, then the squared differences from mean = sum / T.
//   fs2_modspec       one workgroup of 256 lanes per (b, k).  The table of cos / sin(2 pi j / 4096) (64 KiB) and the mean-removed
//                     trajectory (16 KiB) are copied to LDS; lane l owns the bins l, l + 256, .. <= 2048 and walks t ascending with
//                     the table index (f t) mod 4096 kept by an integer addition.  ln(|X|^2 / T + floor) goes to LDS (and to
//                     logms, when asked for); then lane j sums the bins of band j.  The table is in LDS and not left to the L2:
//                     at 98 KiB of LDS one workgroup fits a CU whichever way, the loop is bound by its ~20 fp64 operations per
//                     term and not by the 16-byte table read, and an LDS read has a fixed short latency that the one wave per
//                     SIMD this leaves can cover, where a gather through the 32 KiB vector L1 of a 64 KiB table could not.  A lane's
//                     reads are t entries apart, so an even t costs bank conflicts (a factor of about 3 averaged over t), hidden
//                     under the arithmetic.  Chosen from the code; neither placement has been timed.
#include "fs2_modspec.h"

#define MS_MAX_BANDS 16
#define MS_LDS ((2 * MS_NFFT + MS_MAX_FRAMES + MS_HALF + 8) * (int)sizeof(double))

struct MsBands {
    int n;
    int lo[MS_MAX_BANDS], hi[MS_MAX_BANDS];     // band j is the bins [lo, hi)
};

#pragma clang fp contract(off)

__global__ void __launch_bounds__(MS_MAX_K) traj_moments_kernel(const double* __restrict__ c, long ldc_b, long ldc_t,
                                                                const int32_t* __restrict__ lens, double* __restrict__ mom, long ldm_b,
                                                                long ldm_k, int Tmax, int K) {
    const int b = blockIdx.x, k = threadIdx.x;
    const int T = min(lens[b], min(Tmax, MS_MAX_FRAMES));
    if (k >= K || T < 1) return;
    const double* x = c + (size_t)b * ldc_b + k;
    double s = 0.0, e = 0.0;
    for (int t = 0; t < T; ++t) cs_add(s, e, x[(size_t)t * ldc_t]);
    const double mean = (s + e) / (double)T;
    double m2 = 0.0, e2 = 0.0;
    for (int t = 0; t < T; ++t) {
        const double d = x[(size_t)t * ldc_t] - mean;
        cs_fma(m2, e2, d, d);
    }
    double* q = mom + (size_t)b * ldm_b + (size_t)k * ldm_k;
    q[0] = mean;
    q[1] = m2 + e2;
}

__global__ void __launch_bounds__(MS_NT) modspec_kernel(const double* __restrict__ c, long ldc_b, long ldc_t, const int32_t* __restrict__ lens,
                                                        const double* __restrict__ mean, long ldm_b, long ldm_k,
                                                        const double2* __restrict__ twiddle, MsBands bands, double floor_,
                                                        double* __restrict__ out, long ldo_b, long ldo_k, double* __restrict__ logms,
                                                        long ldl_b, long ldl_k, int Tmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* tw = reinterpret_cast<double2*>(smem);                        // [4096] {cos, sin}
    double* x = reinterpret_cast<double*>(smem) + 2 * MS_NFFT;              // [2048] the mean-removed trajectory
    double* ms = x + MS_MAX_FRAMES;                                         // [2049]
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int T = min(lens[b], min(Tmax, MS_MAX_FRAMES));
    if (T < 1) return;                                                      // the whole workgroup: no barrier is skipped by a part of it
    for (int j = tid; j < MS_NFFT; j += MS_NT) tw[j] = twiddle[j];
    const double mu = mean[(size_t)b * ldm_b + (size_t)k * ldm_k];
    const double* cx = c + (size_t)b * ldc_b + k;
    for (int t = tid; t < T; t += MS_NT) x[t] = cx[(size_t)t * ldc_t] - mu;
    __syncthreads();
    double* lm = logms ? logms + (size_t)b * ldl_b + (size_t)k * ldl_k : nullptr;
    for (int f = tid; f <= MS_HALF; f += MS_NT) {
        double re = 0.0, ree = 0.0, im = 0.0, ime = 0.0;
        int idx = 0;                                                        // (f t) mod 4096
        for (int t = 0; t < T; ++t) {
            const double2 w = tw[idx];
            const double v = x[t];
            cs_fma(re, ree, v, w.x);
            cs_fma(im, ime, v, w.y);                                        // the sign of the imaginary part does not reach the power
            idx = (idx + f) & (MS_NFFT - 1);
        }
        re += ree;
        im += ime;
        double p = 0.0, pe = 0.0;
        cs_fma(p, pe, re, re);
        cs_fma(p, pe, im, im);
        const double v = log((p + pe) / (double)T + floor_);
        ms[f] = v;
        if (lm) lm[f] = v;
    }
    __syncthreads();
    if (tid < bands.n) {
        const int lo = bands.lo[tid], hi = bands.hi[tid];
        double s = 0.0, e = 0.0;
        for (int f = lo; f < hi; ++f) cs_add(s, e, ms[f]);
        out[(size_t)b * ldo_b + (size_t)k * ldo_k + tid] = (s + e) / (double)(hi - lo) * (10.0 / 2.302585092994045684);
    }
}

extern "C" int fs2_modspec_nfft(void) { return MS_NFFT; }

extern "C" int fs2_traj_moments(const double* c, long ldc_b, long ldc_t, const int32_t* lens, double* mom, long ldm_b, long ldm_k, int B,
                                int Tmax, int K, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && Tmax >= 1 && Tmax <= MS_MAX_FRAMES, "traj_moments: bad shape B=%d Tmax=%d (1..%d frames)", B, Tmax, MS_MAX_FRAMES);
    FS2_CHECK_ARG(K >= 1 && K <= MS_MAX_K, "traj_moments: %d coefficients, supported are 1..%d", K, MS_MAX_K);
    FS2_CHECK_ARG(ldc_t >= K && ldc_b >= (long)Tmax * ldc_t && ldm_k >= 2 && ldm_b >= (long)K * ldm_k,
                  "traj_moments: bad strides c %ld %ld mom %ld %ld", ldc_b, ldc_t, ldm_b, ldm_k);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(c && lens && mom, "traj_moments: null pointer");
    traj_moments_kernel<<<B, MS_MAX_K, 0, stream>>>(c, ldc_b, ldc_t, lens, mom, ldm_b, ldm_k, Tmax, K);
    FS2_CHECK_LAUNCH("traj_moments");
    return FS2_OK;
}

extern "C" int fs2_modspec(const double* c, long ldc_b, long ldc_t, const int32_t* lens, const double* mean, long ldm_b, long ldm_k,
                           const double* twiddle, const int32_t* bins, int n_bands, double floor_, double* bands, long ldo_b, long ldo_k,
                           double* logms, long ldl_b, long ldl_k, int B, int Tmax, int K, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && Tmax >= 1 && Tmax <= MS_MAX_FRAMES, "modspec: bad shape B=%d Tmax=%d (1..%d frames)", B, Tmax, MS_MAX_FRAMES);
    FS2_CHECK_ARG(K >= 1 && K <= MS_MAX_K, "modspec: %d coefficients, supported are 1..%d", K, MS_MAX_K);
    FS2_CHECK_ARG(B <= 65535, "modspec: %d rows, supported are at most 65535 per launch", B);
    FS2_CHECK_ARG(n_bands >= 1 && n_bands <= MS_MAX_BANDS && bins, "modspec: %d bands, supported are 1..%d", n_bands, MS_MAX_BANDS);
    FS2_CHECK_ARG(floor_ > 0.0, "modspec: the floor must be positive");
    MsBands mb;
    mb.n = n_bands;
    for (int j = 0; j < n_bands; ++j) {
        mb.lo[j] = bins[2 * j];
        mb.hi[j] = bins[2 * j + 1];
        FS2_CHECK_ARG(mb.lo[j] >= (j ? mb.hi[j - 1] : 0) && mb.lo[j] < mb.hi[j] && mb.hi[j] <= MS_HALF + 1,
                      "modspec: band bins must be non-empty, ascending and disjoint ranges within [0, %d], band %d is [%d, %d)", MS_HALF + 1, j,
                      mb.lo[j], mb.hi[j]);
    }
    for (int j = n_bands; j < MS_MAX_BANDS; ++j) mb.lo[j] = mb.hi[j] = 0;
    FS2_CHECK_ARG(ldc_t >= K && ldc_b >= (long)Tmax * ldc_t && ldm_k >= 1 && ldm_b >= (long)(K - 1) * ldm_k + 1 && ldo_k >= n_bands &&
                      ldo_b >= (long)K * ldo_k,
                  "modspec: bad strides c %ld %ld mean %ld %ld bands %ld %ld", ldc_b, ldc_t, ldm_b, ldm_k, ldo_b, ldo_k);
    FS2_CHECK_ARG(logms == nullptr || (ldl_k >= MS_HALF + 1 && ldl_b >= (long)K * ldl_k), "modspec: bad strides logms %ld %ld", ldl_b, ldl_k);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(c && lens && mean && twiddle && bands, "modspec: null pointer");
    static Fs2DevOnce once;                                                 // 98 KiB: above the 64 KiB a kernel gets unasked
    once.run([&] { (void)hipFuncSetAttribute((const void*)modspec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MS_LDS); });
    modspec_kernel<<<dim3(K, B), MS_NT, MS_LDS, stream>>>(c, ldc_b, ldc_t, lens, mean, ldm_b, ldm_k, reinterpret_cast<const double2*>(twiddle),
                                                          mb, floor_, bands, ldo_b, ldo_k, logms, ldl_b, ldl_k, Tmax);
    FS2_CHECK_LAUNCH("modspec");
    return FS2_OK;
}
