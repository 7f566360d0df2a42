// fs2_msfilter.hip — the modulation-spectrum postfilter of Takamichi et al. 2016 on generated parameter trajectories: running
// statistics of the log modulation spectrum over utterances, and the filter that moves a trajectory's log modulation spectrum from
// the statistics of generated speech to those of natural speech and keeps its phase.  The specification is the docstring of
// fastspeech2_amd/postfilter.py; tests/postfilter_ref.py restates it in numpy with an FFT.  The log modulation spectrum that the
// statistics fold comes from fs2_modspec (csrc/fs2_modspec.hip), which is not repeated here.
//
// The arithmetic is fp64: every sum is a compensated sum of fs2_comp.h over its terms in ascending order in one thread.  No atomics,
// no cross-lane reduction: the same input gives the same bytes.  The transform's sizes are those of fs2_modspec.h, shared with
// fs2_modspec.
//
//   fs2_ms_stats_update  one thread per (k, f), lanes along f.  Welford's update of (mean, M2) over the rows b = 0 .. B - 1 of a logms
//                        batch in ascending b; rows whose keep flag is 0 are skipped; the count of rows folded before comes in.
//   fs2_ms_filter        one workgroup of 256 lanes per (b, k), float32 or float64 trajectories.  LDS holds the table of
//                        cos / sin(2 pi j / 4096) (64 KiB), the mean-removed trajectory (16 KiB) and the filtered half spectrum
//                        (2049 complex, 32 KiB + 16 B): 112 KiB of the 160 KiB of a CDNA4 compute unit, one workgroup per CU as
//                        fs2_modspec has it.  The four statistics rows of k (another 64 KiB) would not fit beside them; they stay
//                        in global memory, where each entry is read once, by consecutive lanes at consecutive f.  Phase 1: lane l
//                        owns the bins l, l + 256, .. <= 2048, walks t ascending with the table index (f t) mod 4096 kept by an
//                        integer addition, forms X[f], ms[f] (the operations of fs2_modspec in its order: the same bytes) and
//                        g[f], and leaves w g X in LDS, w = 2 for 0 < f < N / 2 and 1 at the two real bins.  Phase 2: lane l owns
//                        the frames l, l + 256, .. < T and walks f = 0 .. 2048 ascending with the same index.  A row shorter than
//                        min_frames is copied; a row with lens[b] < 1 is left alone.  Placement chosen from the code, not timed.
#include "fs2_modspec.h"

#define MF_LDS ((2 * MS_NFFT + MS_MAX_FRAMES + 2 * (MS_HALF + 1)) * (int)sizeof(double))

#pragma clang fp contract(off)

__global__ void __launch_bounds__(MS_NT) ms_stats_update_kernel(const double* __restrict__ logms, long ldl_b, long ldl_k,
                                                                const int32_t* __restrict__ keep, double* __restrict__ state, long lds_k,
                                                                long n_before, int B) {
    const int f = blockIdx.x * MS_NT + threadIdx.x, k = blockIdx.y;
    if (f > MS_HALF) return;
    double* st = state + (size_t)k * lds_k + 2 * (size_t)f;
    double mean = 0.0, m2 = 0.0;
    if (n_before > 0) {
        mean = st[0];
        m2 = st[1];
    }
    long n = n_before;
    const double* x = logms + (size_t)k * ldl_k + f;
    for (int b = 0; b < B; ++b) {
        if (keep[b] == 0) continue;
        const double v = x[(size_t)b * ldl_b];
        n += 1;
        const double d = v - mean;
        mean += d / (double)n;
        m2 += d * (v - mean);
    }
    st[0] = mean;
    st[1] = m2;
}

template <typename T>
__global__ void __launch_bounds__(MS_NT) ms_filter_kernel(const T* __restrict__ c, long ldc_b, long ldc_t, const int32_t* __restrict__ lens,
                                                          const double* __restrict__ mean, long ldm_b, long ldm_k,
                                                          const double2* __restrict__ twiddle, const double* __restrict__ mu_n,
                                                          const double* __restrict__ sd_n, const double* __restrict__ mu_g,
                                                          const double* __restrict__ sd_g, long lds_k, double kk, double floor_,
                                                          double max_ln_gain, int min_frames, T* __restrict__ y, long ldy_b, long ldy_t,
                                                          int Tmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* tw = reinterpret_cast<double2*>(smem);                        // [4096] {cos, sin}
    double* x = reinterpret_cast<double*>(smem) + 2 * MS_NFFT;              // [2048] the mean-removed trajectory
    double2* sp = reinterpret_cast<double2*>(x + MS_MAX_FRAMES);            // [2049] w g X: {re, the sine sum}
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int T_ = min(lens[b], min(Tmax, MS_MAX_FRAMES));
    if (T_ < 1) return;                                                     // the whole workgroup: no barrier is skipped by a part of it
    const T* cx = c + (size_t)b * ldc_b + k;
    T* yx = y + (size_t)b * ldy_b + k;
    if (T_ < min_frames) {                                                  // too short to filter: the row goes through as it is
        for (int t = tid; t < T_; t += MS_NT) yx[(size_t)t * ldy_t] = cx[(size_t)t * ldc_t];
        return;
    }
    for (int j = tid; j < MS_NFFT; j += MS_NT) tw[j] = twiddle[j];
    const double mu = mean[(size_t)b * ldm_b + (size_t)k * ldm_k];
    for (int t = tid; t < T_; t += MS_NT) x[t] = (double)cx[(size_t)t * ldc_t] - mu;
    __syncthreads();
    const size_t row = (size_t)k * lds_k;
    for (int f = tid; f <= MS_HALF; f += MS_NT) {
        double re = 0.0, ree = 0.0, im = 0.0, ime = 0.0;
        int idx = 0;                                                        // (f t) mod 4096
        for (int t = 0; t < T_; ++t) {
            const double2 w = tw[idx];
            const double v = x[t];
            cs_fma(re, ree, v, w.x);
            cs_fma(im, ime, v, w.y);                                        // X = re - i im
            idx = (idx + f) & (MS_NFFT - 1);
        }
        re += ree;
        im += ime;
        double p = 0.0, pe = 0.0;
        cs_fma(p, pe, re, re);
        cs_fma(p, pe, im, im);
        const double ms = log((p + pe) / (double)T_ + floor_);
        const double sg = sd_g[row + f];
        const double r = sg > 0.0 ? sd_n[row + f] / sg : 1.0;
        const double target = r * (ms - mu_g[row + f]) + mu_n[row + f];
        double lg = 0.5 * kk * (target - ms);
        lg = fmin(fmax(lg, -max_ln_gain), max_ln_gain);
        const bool edge = f == 0 || f == MS_HALF;                           // the two real bins: weight 1, no imaginary part
        const double g = f == 0 ? 1.0 : exp(lg);
        const double w = edge ? 1.0 : 2.0;
        sp[f] = make_double2(w * (g * re), edge ? 0.0 : w * (g * im));
    }
    __syncthreads();
    for (int t = tid; t < T_; t += MS_NT) {
        double s = 0.0, e = 0.0;
        int idx = 0;                                                        // (f t) mod 4096
        for (int f = 0; f <= MS_HALF; ++f) {
            const double2 w = tw[idx];
            const double2 v = sp[f];
            cs_fma(s, e, v.x, w.x);                                         // Re((re - i im)(cos + i sin)) = re cos + im sin
            cs_fma(s, e, v.y, w.y);
            idx = (idx + t) & (MS_NFFT - 1);
        }
        yx[(size_t)t * ldy_t] = (T)(mu + (s + e) / (double)MS_NFFT);
    }
}

extern "C" int fs2_ms_stats_update(const double* logms, long ldl_b, long ldl_k, const int32_t* keep, double* state, long lds_k,
                                   long n_before, int B, int K, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && n_before >= 0, "ms_stats_update: bad counts B=%d n_before=%ld", B, n_before);
    FS2_CHECK_ARG(K >= 1 && K <= MS_MAX_K, "ms_stats_update: %d coefficients, supported are 1..%d", K, MS_MAX_K);
    FS2_CHECK_ARG(ldl_k >= MS_HALF + 1 && ldl_b >= (long)K * ldl_k && lds_k >= 2 * (MS_HALF + 1),
                  "ms_stats_update: bad strides logms %ld %ld state %ld", ldl_b, ldl_k, lds_k);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(logms && keep && state, "ms_stats_update: null pointer");
    ms_stats_update_kernel<<<dim3((MS_HALF + MS_NT) / MS_NT, K), MS_NT, 0, stream>>>(logms, ldl_b, ldl_k, keep, state, lds_k, n_before, B);
    FS2_CHECK_LAUNCH("ms_stats_update");
    return FS2_OK;
}

extern "C" int fs2_ms_filter(const void* c, long ldc_b, long ldc_t, const int32_t* lens, const double* mean, long ldm_b, long ldm_k,
                             const double* twiddle, const double* mu_n, const double* sd_n, const double* mu_g, const double* sd_g,
                             long lds_k, double k_emph, double floor_, double max_gain_db, int min_frames, void* y, long ldy_b,
                             long ldy_t, int is_f64, int B, int Tmax, int K, hipStream_t stream) {
    FS2_CHECK_ARG(B >= 0 && Tmax >= 1 && Tmax <= MS_MAX_FRAMES, "ms_filter: bad shape B=%d Tmax=%d (1..%d frames)", B, Tmax, MS_MAX_FRAMES);
    FS2_CHECK_ARG(K >= 1 && K <= MS_MAX_K, "ms_filter: %d coefficients, supported are 1..%d", K, MS_MAX_K);
    FS2_CHECK_ARG(B <= 65535, "ms_filter: %d rows, supported are at most 65535 per launch", B);
    FS2_CHECK_ARG(k_emph >= 0.0 && k_emph <= 1.0, "ms_filter: the emphasis coefficient must lie in [0, 1]");
    FS2_CHECK_ARG(floor_ > 0.0 && max_gain_db >= 0.0 && max_gain_db <= 200.0 && min_frames >= 1,
                  "ms_filter: the floor must be positive, the gain bound within [0, 200] dB, min_frames at least 1");
    FS2_CHECK_ARG(is_f64 == 0 || is_f64 == 1, "ms_filter: is_f64 must be 0 (float32) or 1 (float64)");
    FS2_CHECK_ARG(ldc_t >= K && ldc_b >= (long)Tmax * ldc_t && ldy_t >= K && ldy_b >= (long)Tmax * ldy_t && ldm_k >= 1 &&
                      ldm_b >= (long)(K - 1) * ldm_k + 1 && lds_k >= MS_HALF + 1,
                  "ms_filter: bad strides c %ld %ld y %ld %ld mean %ld %ld stats %ld", ldc_b, ldc_t, ldy_b, ldy_t, ldm_b, ldm_k, lds_k);
    if (B == 0) return FS2_OK;
    FS2_CHECK_ARG(c && lens && mean && twiddle && mu_n && sd_n && mu_g && sd_g && y, "ms_filter: null pointer");
    const double max_ln_gain = max_gain_db * (2.302585092994045684 / 20.0);
    const double2* tw = reinterpret_cast<const double2*>(twiddle);
    if (is_f64) {
        static Fs2DevOnce once;                                             // 112 KiB: above the 64 KiB a kernel gets unasked
        once.run([&] { (void)hipFuncSetAttribute((const void*)ms_filter_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, MF_LDS); });
        ms_filter_kernel<double><<<dim3(K, B), MS_NT, MF_LDS, stream>>>(static_cast<const double*>(c), ldc_b, ldc_t, lens, mean, ldm_b, ldm_k, tw,
                                                                        mu_n, sd_n, mu_g, sd_g, lds_k, k_emph, floor_, max_ln_gain, min_frames,
                                                                        static_cast<double*>(y), ldy_b, ldy_t, Tmax);
    } else {
        static Fs2DevOnce once;
        once.run([&] { (void)hipFuncSetAttribute((const void*)ms_filter_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, MF_LDS); });
        ms_filter_kernel<float><<<dim3(K, B), MS_NT, MF_LDS, stream>>>(static_cast<const float*>(c), ldc_b, ldc_t, lens, mean, ldm_b, ldm_k, tw,
                                                                       mu_n, sd_n, mu_g, sd_g, lds_k, k_emph, floor_, max_ln_gain, min_frames,
                                                                       static_cast<float*>(y), ldy_b, ldy_t, Tmax);
    }
    FS2_CHECK_LAUNCH("ms_filter");
    return FS2_OK;
}
