// fs2_griffin_lim.hip — the HBM-bound passes of Griffin-Lim mel inversion (reference audio/stft.py:52-122 STFT.transform /
// inverse, audio/audio_processing.py:7-82 window_sumsquare / griffin_lim, audio/tools.py:18-34 inv_mel_spec).
// Both contractions of an iteration run in fs2_conv_gemm on the exact-fp32 MFMA:
//   forward   ft[B*S][2*NF]  = 4-tap framed DFT of the reflect-padded signal rows (as mel extraction does)
//   inverse   seg[B*F][filt] = G[B*F][ld] . inverse_basis          (one tap; the overlap-add is fs2_gl_ola's)
// One iteration = forward GEMM -> fs2_gl_project -> inverse GEMM -> fs2_gl_ola, all on the caller's stream.
// Layout: frame-major rows; G rows are [m cos(phi) (NF) | m sin(phi) (NF) | 0 ...] of ldg >= 2 NF floats.  Utterance b has
// frames[b] frames of the Fmax rows it owns; every padding entry (rows f >= frames[b], columns >= 2 NF) is WRITTEN as 0 on
// every pass, so no GEMM ever reads stale memory (garbage x 0 weight is NaN when the garbage is Inf / NaN).
#include "fs2_common.h"

static __device__ __forceinline__ int gl_frames(const int32_t* frames, int b, int Fmax) {
    return frames ? min(max(frames[b], 0), Fmax) : Fmax;
}

// ------------------------------------------------------------------ log-mel -> linear magnitude (inv_mel_spec, tools.py:19-26)
// mag[b][f][k] = 1000 * sum_j exp(mel[b][j][f]) * mel_basis[j][k] over the filters j whose non-zero band [lo_j, hi_j) holds k
// (bins no filter reaches are 0), for f < frames[b] = mel_lens[b] - 1 (the reference drops the last frame); 0 beyond.
// One 256-thread block per (frame, utterance): exp(mel) of the frame goes to LDS once.
__global__ void gl_mel_to_mag_kernel(const float* __restrict__ mel, long sb, long sj, long st, const int32_t* __restrict__ mel_lens,
                                     const float* __restrict__ melb, const int32_t* __restrict__ span, float* __restrict__ mag,
                                     long ldm, int Fmax, int n_mel, int NF) {
    __shared__ float e[256];
    const int b = blockIdx.y, f = blockIdx.x;
    const int F = min(max(mel_lens[b] - 1, 0), Fmax);
    float* out = mag + ((size_t)b * Fmax + f) * ldm;
    if (f >= F) {
        for (int k = threadIdx.x; k < NF; k += blockDim.x) out[k] = 0.f;
        return;
    }
    for (int j = threadIdx.x; j < n_mel; j += blockDim.x) e[j] = expf(mel[(size_t)b * sb + (size_t)j * sj + (size_t)f * st]);
    __syncthreads();
    for (int k = threadIdx.x; k < NF; k += blockDim.x) {
        float acc = 0.f;
        for (int j = 0; j < n_mel; ++j)
            if (k >= span[2 * j] && k < span[2 * j + 1]) acc = fmaf(e[j], melb[(size_t)j * NF + k], acc);
        out[k] = acc * 1000.f;
    }
}
extern "C" int fs2_gl_mel_to_mag(const float* mel, long sb, long sj, long st, const int32_t* mel_lens, const float* mel_basis,
                                 const int32_t* span, float* mag, long ldm, int B, int Fmax, int n_mel, int NF, hipStream_t stream) {
    FS2_CHECK_ARG(mel && mel_lens && mel_basis && span && mag, "gl_mel_to_mag: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax > 0 && n_mel > 0 && n_mel <= 256 && NF > 0 && ldm >= NF,
                  "gl_mel_to_mag: bad shape B=%d Fmax=%d n_mel=%d NF=%d ldm=%ld", B, Fmax, n_mel, NF, ldm);
    if (B == 0) return FS2_OK;
    gl_mel_to_mag_kernel<<<dim3(Fmax, B), 256, 0, stream>>>(mel, sb, sj, st, mel_lens, mel_basis, span, mag, ldm, Fmax, n_mel, NF);
    FS2_CHECK_LAUNCH("gl_mel_to_mag");
    return FS2_OK;
}

// ------------------------------------------------------------------ [m cos(phi) ; m sin(phi)] (stft.py:84-86)
// Strided magnitude / phase (element (b, f, k) at b*sb + f*sf + k*sk): the reference's (B, NF, F) tensors as well as the loop's
// frame-major magnitude.  One thread per G column; the row is grid x (B * Fmax passes the 65535 of grid y at a synthesis batch).
__global__ void gl_recombine_kernel(const float* __restrict__ mag, long msb, long msf, long msk, const float* __restrict__ ph,
                                    long psb, long psf, long psk, const int32_t* __restrict__ frames, float* __restrict__ G,
                                    long ldg, int Fmax, int NF) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= ldg) return;
    const int row = blockIdx.x, b = row / Fmax, f = row - b * Fmax;
    float v = 0.f;
    if (f < gl_frames(frames, b, Fmax) && c < 2 * NF) {
        const int k = c < NF ? c : c - NF;
        const float m = mag[(size_t)b * msb + (size_t)f * msf + (size_t)k * msk];
        const float p = ph[(size_t)b * psb + (size_t)f * psf + (size_t)k * psk];
        v = m * (c < NF ? cosf(p) : sinf(p));
    }
    G[(size_t)row * ldg + c] = v;
}
extern "C" int fs2_gl_recombine(const float* mag, long msb, long msf, long msk, const float* phase, long psb, long psf, long psk,
                                const int32_t* frames, float* G, long ldg, int B, int Fmax, int NF, hipStream_t stream) {
    FS2_CHECK_ARG(mag && phase && G, "gl_recombine: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax > 0 && NF > 0 && ldg >= 2L * NF, "gl_recombine: bad shape B=%d Fmax=%d NF=%d ldg=%ld", B, Fmax, NF, ldg);
    if (B == 0) return FS2_OK;
    gl_recombine_kernel<<<dim3(B * Fmax, fs2_cdiv(ldg, 256)), 256, 0, stream>>>(mag, msb, msf, msk, phase, psb, psf, psk, frames, G,
                                                                               ldg, Fmax, NF);
    FS2_CHECK_LAUNCH("gl_recombine");
    return FS2_OK;
}

// ------------------------------------------------------------------ phase projection (audio_processing.py:77-79)
// angles = atan2(Im, Re) of the forward DFT (stft.py:79, atan2(0, 0) = 0), next inverse input = [m cos(angles) ; m sin(angles)]
// with m the TARGET magnitude: transform()'s magnitude is never formed.  Thread k < NF writes columns k and NF + k; the threads
// past NF zero the padding columns [2 NF, ldg).
__global__ void gl_project_kernel(const float* __restrict__ ft, long ldft, int S, const float* __restrict__ mag, long msb, long msf,
                                  long msk, const int32_t* __restrict__ frames, float* __restrict__ G, long ldg, int Fmax, int NF) {
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    const int npad = (int)(ldg - 2L * NF);
    if (k >= NF + npad) return;
    const int row = blockIdx.x, b = row / Fmax, f = row - b * Fmax;
    float* g = G + (size_t)row * ldg;
    if (k >= NF) { g[NF + k] = 0.f; return; }
    float vr = 0.f, vi = 0.f;
    if (f < gl_frames(frames, b, Fmax)) {
        const float* r = ft + ((size_t)b * S + f) * ldft;
        const float p = atan2f(r[NF + k], r[k]);
        const float m = mag[(size_t)b * msb + (size_t)f * msf + (size_t)k * msk];
        vr = m * cosf(p);
        vi = m * sinf(p);
    }
    g[k] = vr;
    g[NF + k] = vi;
}
extern "C" int fs2_gl_project(const float* ft, long ldft, int S, const float* mag, long msb, long msf, long msk, const int32_t* frames,
                              float* G, long ldg, int B, int Fmax, int NF, hipStream_t stream) {
    FS2_CHECK_ARG(ft && mag && G, "gl_project: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax > 0 && S >= Fmax && NF > 0 && ldft >= 2L * NF && ldg >= 2L * NF,
                  "gl_project: bad shape B=%d Fmax=%d S=%d NF=%d ldft=%ld ldg=%ld", B, Fmax, S, NF, ldft, ldg);
    if (B == 0) return FS2_OK;
    const long nthr = ldg - NF;
    gl_project_kernel<<<dim3(B * Fmax, fs2_cdiv(nthr, 256)), 256, 0, stream>>>(ft, ldft, S, mag, msb, msf, msk, frames, G, ldg, Fmax, NF);
    FS2_CHECK_LAUNCH("gl_project");
    return FS2_OK;
}

// ------------------------------------------------------------------ overlap-add + window envelope (stft.py:88-120)
// Sample s of utterance b (N_b = hop (F_b - 1) samples after the trim) is t = s + filt/2 of the untrimmed conv_transpose1d
// output: the sum of seg[f][t - f hop] over the frames f that cover t, in increasing f, so a row's result depends on no other
// row of the batch.  The envelope is window_sumsquare's float32 array entry, rebuilt bit-exactly: frames added in increasing
// order, each add done in double and rounded to float32 (numpy: float32 array += float64 window^2).  Then the reference's
// `/= env where env > tiny(float32)` and `*= filt / hop`.
__device__ __forceinline__ float gl_ola_sample(const float* __restrict__ seg, long lds, const double* __restrict__ win_sq, int b,
                                               int Fmax, int F, int filt, int hop, long s, float scale) {
    const long t = s + filt / 2;
    const long f_lo = t >= filt ? (t - filt) / hop + 1 : 0;
    const long f_hi = min((long)F - 1, t / hop);
    float acc = 0.f, env = 0.f;
    for (long f = f_lo; f <= f_hi; ++f) {
        const long o = t - f * hop;
        acc += seg[((size_t)b * Fmax + f) * lds + o];
        env = (float)((double)env + win_sq[o]);
    }
    if (env > 1.17549435e-38f) acc = acc / env;
    return acc * scale;
}

// Thread i of row b writes xp[b][i] (the reflect-padded signal rows the next forward DFT reads: reflected at the utterance's
// OWN end as fs2_reflect_pad_ragged does, zero beyond N_b + filt) and, when y is given, y[b][i] for i < ldy (0 beyond N_b).
__global__ void gl_ola_kernel(const float* __restrict__ seg, long lds, const int32_t* __restrict__ frames, const double* __restrict__ win_sq,
                              float* __restrict__ xp, long row_len, float* __restrict__ y, long ldy, int Fmax, int filt, int hop, float scale) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int F = gl_frames(frames, b, Fmax);
    const long N = (long)hop * (F - 1), P = filt / 2;
    if (xp && i < row_len) {
        float v = 0.f;
        if (N > P && i < N + 2 * P) {
            long s = i - P;
            if (s < 0) s = -s;
            if (s >= N) s = 2 * (N - 1) - s;
            v = gl_ola_sample(seg, lds, win_sq, b, Fmax, F, filt, hop, s, scale);
        }
        xp[(size_t)b * row_len + i] = v;
    }
    if (y && i < ldy) y[(size_t)b * ldy + i] = i < N ? gl_ola_sample(seg, lds, win_sq, b, Fmax, F, filt, hop, i, scale) : 0.f;
}
extern "C" int fs2_gl_ola(const float* seg, long lds, const int32_t* frames, const double* win_sq, float* xp, long row_len, float* y,
                          long ldy, int B, int Fmax, int filter_length, int hop_length, hipStream_t stream) {
    FS2_CHECK_ARG(seg && win_sq && (xp || y), "gl_ola: null pointer");
    FS2_CHECK_ARG(B >= 0 && Fmax > 0 && hop_length > 0 && filter_length >= hop_length && filter_length % 2 == 0 && lds >= filter_length,
                  "gl_ola: bad shape B=%d Fmax=%d filter=%d hop=%d lds=%ld", B, Fmax, filter_length, hop_length, lds);
    FS2_CHECK_ARG(!xp || row_len >= (long)hop_length * (Fmax - 1) + filter_length, "gl_ola: xp rows of %ld < %ld samples", row_len,
                  (long)hop_length * (Fmax - 1) + filter_length);
    FS2_CHECK_ARG(!y || ldy >= (long)hop_length * (Fmax - 1), "gl_ola: y rows of %ld < %ld samples", ldy, (long)hop_length * (Fmax - 1));
    if (B == 0) return FS2_OK;
    const long n = max(xp ? row_len : 0L, y ? ldy : 0L);
    if (n == 0) return FS2_OK;
    gl_ola_kernel<<<dim3(fs2_cdiv(n, 256), B), 256, 0, stream>>>(seg, lds, frames, win_sq, xp, row_len, y, ldy, Fmax, filter_length,
                                                                 hop_length, (float)filter_length / (float)hop_length);
    FS2_CHECK_LAUNCH("gl_ola");
    return FS2_OK;
}

// ------------------------------------------------------------------ STFT.transform's outputs (stft.py:74-81)
// ft rows [B*S][2 NF] -> magnitude = sqrt(re^2 + im^2) (each product and the sum rounded, as the reference's separate tensor ops),
// phase = atan2(im, re); both (B, NF, F) channel-major like the reference.
__global__ void gl_mag_phase_kernel(const float* __restrict__ ft, long ldft, int S, float* __restrict__ mag, float* __restrict__ phase,
                                    int F, int NF) {
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= NF) return;
    const int f = blockIdx.x, b = blockIdx.z;
    const float* r = ft + ((size_t)b * S + f) * ldft;
    const float re = r[k], im = r[NF + k];
    const size_t o = ((size_t)b * NF + k) * F + f;
    mag[o] = sqrtf(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)));
    phase[o] = atan2f(im, re);
}
extern "C" int fs2_gl_mag_phase(const float* ft, long ldft, int S, float* mag, float* phase, int B, int F, int NF, hipStream_t stream) {
    FS2_CHECK_ARG(ft && mag && phase, "gl_mag_phase: null pointer");
    FS2_CHECK_ARG(B >= 0 && F > 0 && S >= F && NF > 0 && ldft >= 2L * NF, "gl_mag_phase: bad shape B=%d F=%d S=%d NF=%d", B, F, S, NF);
    if (B == 0) return FS2_OK;
    gl_mag_phase_kernel<<<dim3(F, fs2_cdiv(NF, 256), B), 256, 0, stream>>>(ft, ldft, S, mag, phase, F, NF);
    FS2_CHECK_LAUNCH("gl_mag_phase");
    return FS2_OK;
}
