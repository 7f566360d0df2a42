// fs2_melgan.hip - MelGAN generator kernels (gfx950): reflection guard rows for the contraction kernels, and the three ResnetBlocks of
// a narrow up-sampling stage (C = 32 / 64 channels, bf16) in ONE launch.
//
//   ResnetBlock_d(x) = shortcut(x) + conv4(lrelu(conv3_d(reflect_pad_d(lrelu(x)))))        slope 0.2, d = 1 / 3 / 9
//   conv3_d: k = 3, dilation d;  shortcut, conv4: k = 1  ->  one contraction over K = 2C:  [x | t] . [W_shortcut ; W_4] + (b_shortcut + b_4)
//
// (1) fs2_melgan_guard_rows.  The contraction kernels zero-pad; MelGAN reflects.  Instead of a reflection branch in their operand path an
// activation buffer carries G guard rows in front of and behind every batch item ([B][G + S + G][C]), this kernel fills them - by
// reflection at the ends of [0, S) (F.pad(mode="reflect"): the edge row is not repeated), or with zeros in front of a transposed
// convolution, whose own padding IS zero - and the existing kernels then run over S + 2G rows per item: what they compute for the guard
// rows is never read.  With src != dst the interior rows are copied as well (a compact buffer into a guarded one of another row stride).
//
// (2) fs2_melgan_stage_fwd.  At C = 64 / 32 the blocks are HBM-bound one convolution at a time (the case fs2_resblock.hip's header
// makes for HiFi-GAN).  A workgroup of 8 waves owns a tile of E rows of one batch item and runs all three blocks on it:
//   * x is read once, the stage's output written once; a lane owns a row, the running value lives in fp32 MFMA accumulators
//     (transposed product D[cout][row], as in fs2_resblock.hip) and is never stored between blocks;
//   * only what a DILATED convolution reads goes through LDS: lrelu(value) as bf16 rows [GUARD + E + GUARD][C + 8] (padded rows, one
//     16-byte chunk: conflict-free ds_read_b128).  The two k = 1 convolutions read nothing but the lane's own row, and after
//     v_permlane32_swap the accumulator layout IS the B-operand layout of a k-slice: their operands (raw value for the shortcut,
//     lrelu(t) for conv4) go from registers into the MFMA without touching LDS;
//   * reflection: a block reflects ITS input at the ends of [0, S), so tile rows outside the sequence cannot be carried along - after
//     every block they are rewritten: the lane that owns row t in [1, 9] also stores it at row -t, the owner of t in [S - 10, S - 2] at
//     2 (S - 1) - t (LDS rows only; the x loader clamps its global row index and nothing is read from a neighbouring item);
//   * halo by recomputation: H = d0 + d1 + d2 = 13 rows per side; a tile outputs its central R = E - 2H rows.  A tile edge that lies
//     outside the sequence costs no validity (its rows are reflections of valid ones), an edge inside loses d rows per block;
//   * weights: one block's [5C][C] bf16 image (conv3's three taps, shortcut, conv4: 40 KiB at C = 64) in LDS, XOR-swizzled rows; the NEXT
//     block's image is fetched into registers (5 x 16 bytes per thread) before the current block's MFMAs and stored behind the
//     barrier that ends them.  fs2_resblock.hip's LDS-DMA ring is not used: the whole stream is 120 KiB per workgroup.
// The stage's output is stored leaky-ReLU'd when out_slope > 0 (the next consumer - the following transposed convolution, or the
// final conv 24 - reads lrelu(value) only).  bf16 only; fp32 compute and any other C run the chain of single launches.
#include "fs2_gemm.h"

typedef unsigned mg_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned mg_u32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ guard rows
// one thread per 16-byte chunk of a destination row; src / dst strides in 16-byte chunks
__global__ void melgan_guard_rows_kernel(const uint4* __restrict__ src, long lds_, long src_bs, uint4* __restrict__ dst, long ldd, long dst_bs,
                                         int S, int G, int cpr, int reflect, int interior) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nrows = interior ? (long)S + 2 * G : 2L * G;
    if (i >= nrows * cpr) return;
    const int jr = (int)(i / cpr), c = (int)(i - (long)jr * cpr);
    const int j = interior ? jr : (jr < G ? jr : S + jr);        // guard rows only: [0, G) and [G + S, S + 2G)
    const int t = j - G;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const bool inside = t >= 0 && t < S;
    if (inside || reflect) {
        const int s = t < 0 ? -t : (t >= S ? 2 * (S - 1) - t : t);
        v = src[(size_t)b * src_bs + (size_t)s * lds_ + c];
    }
    dst[(size_t)b * dst_bs + (size_t)j * ldd + c] = v;
}

extern "C" int fs2_melgan_guard_rows(const void* src, long ld_src, long src_bstride, void* dst, long ld_dst, long dst_bstride, int B, int S,
                                     int G, int C, int reflect, int interior, int dtype, hipStream_t stream) {
    FS2_CHECK_ARG(src && dst, "melgan_guard_rows: null pointer");
    FS2_CHECK_ARG(dtype == FS2_F32 || dtype == FS2_BF16, "melgan_guard_rows: dtype %d", dtype);
    const int epc = dtype == FS2_F32 ? 4 : 8;
    FS2_CHECK_ARG(B >= 0 && S > 0 && G >= 0 && C > 0 && C % epc == 0, "melgan_guard_rows: bad shape B=%d S=%d G=%d C=%d", B, S, G, C);
    FS2_CHECK_ARG(!reflect || S > G, "melgan_guard_rows: a reflection of %d rows needs more than %d rows", G, S);
    FS2_CHECK_ARG(ld_src % epc == 0 && ld_dst % epc == 0 && src_bstride % epc == 0 && dst_bstride % epc == 0 && ld_src >= C && ld_dst >= C &&
                  (((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "melgan_guard_rows: rows must be 16-byte addressable");
    const long nrows = interior ? (long)S + 2 * G : 2L * G;
    if (B == 0 || nrows == 0) return FS2_OK;
    const int cpr = C / epc;
    dim3 grid(fs2_cdiv(nrows * cpr, 256), B);
    melgan_guard_rows_kernel<<<grid, 256, 0, stream>>>(reinterpret_cast<const uint4*>(src), ld_src / epc, src_bstride / epc,
                                                       reinterpret_cast<uint4*>(dst), ld_dst / epc, dst_bstride / epc, S, G, cpr, reflect, interior);
    FS2_CHECK_LAUNCH("melgan_guard_rows");
    return FS2_OK;
}

// ------------------------------------------------------------------ a narrow stage's three ResnetBlocks in one launch
struct MelganStageArgs {
    const bf16_t* X; long ldx, x_bs;        // row t of item b: X + b * x_bs + t * ldx   (elements)
    const bf16_t* W;                        // [3 blocks][5C rows][C]: conv3 tap 0 / 1 / 2 (cout-major), shortcut, conv4
    const float* bias;                      // [3][2][C]: conv3's, shortcut's + conv4's
    bf16_t* Y; long ldy, y_bs;
    float slope, out_slope;
    int S, d[3], R, tiles_per_seq;
};

template <int C> struct MgCfg {
    static constexpr int E = C == 32 ? 512 : 256;             // tile rows: 8 waves x MB x 32
    static constexpr int GUARD = 9;                           // largest dilation: rows a shifted read may touch outside the tile
    static constexpr int MB = E / 256, NB = C / 32, KS = C / 16, CPR = C / 8;
    static constexpr int STRIDE = C * 2 + 16;                 // activation rows padded by one chunk (an odd number of chunks per row)
    static constexpr int ROWB = C * 2;
    static constexpr int WROWS = 5 * C;
    static constexpr int ACT_BYTES = (E + 2 * GUARD) * STRIDE;
    static constexpr int W_OFF = ACT_BYTES;
    static constexpr int LDS = W_OFF + WROWS * ROWB;          // C = 64: 39456 + 40960, C = 32: 42400 + 10240
    static constexpr int NWCH = WROWS * ROWB / 16;            // 16-byte chunks of one block's weight image
    static constexpr int WPT = (NWCH + 511) / 512;            // ... per thread
};
// swizzle key of weight row r: chunk c is stored at chunk c ^ key (16 consecutive rows x one chunk -> 16 distinct 16-byte slots)
template <int C> __device__ __forceinline__ unsigned mg_wkey(unsigned r) { return C == 32 ? ((r >> 2) & 3u) : ((r >> 1) & 7u); }

template <int C>
__global__ void __launch_bounds__(512, 2) melgan_stage_kernel(MelganStageArgs a) {
    typedef MgCfg<C> K;
    constexpr int E = K::E, GUARD = K::GUARD, MB = K::MB, NB = K::NB, KS = K::KS, STRIDE = K::STRIDE, ROWB = K::ROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, fl = lane & 31, fh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = blockIdx.x / a.tiles_per_seq, tile = blockIdx.x - seq * a.tiles_per_seq;
    const int H = (E - a.R) >> 1;
    const int t_first = tile * a.R - H;                       // sequence row of tile row 0
    const int S = a.S;
    const bf16_t* X = a.X + (size_t)seq * a.x_bs;
    bf16_t* Y = a.Y + (size_t)seq * a.y_bs;

    // ---- weights: block j's image global -> registers (fetch_w) -> LDS (store_w)
    mg_u32x4 wreg[K::WPT];
    auto fetch_w = [&](int j) {
        const mg_u32x4* src = reinterpret_cast<const mg_u32x4*>(a.W) + (size_t)j * K::NWCH;
#pragma unroll
        for (int i = 0; i < K::WPT; ++i) {
            wreg[i] = src[min(i * 512 + tid, K::NWCH - 1)];      // (the last thread's surplus chunk is fetched, never stored)
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int i = 0; i < K::WPT; ++i) {
            const int g = i * 512 + tid;
            if (g < K::NWCH) {
                const unsigned row = (unsigned)g / K::CPR, c = (unsigned)g % K::CPR;
                *reinterpret_cast<mg_u32x4*>(smem + K::W_OFF + row * ROWB + ((c ^ mg_wkey<C>(row)) << 4)) = wreg[i];
            }
        }
    };
    fetch_w(0);

    // ---- x -> y in the accumulator layout (lane = row, registers = couts 4 fh + (r & 3) + 8 (r >> 2)); the row index is clamped:
    // rows outside [0, S) are never used from here, they are rewritten by reflection below
    f32x16 y[MB][NB], tacc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int t = min(max(t_first + wave * (MB * 32) + mb * 32 + fl, 0), S - 1);
        const bf16_t* row = X + (size_t)t * a.ldx;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 x4 = ld4<bf16_t>(row + nb * 32 + 8 * q + 4 * fh);
                y[mb][nb][4 * q + 0] = x4.x; y[mb][nb][4 * q + 1] = x4.y; y[mb][nb][4 * q + 2] = x4.z; y[mb][nb][4 * q + 3] = x4.w;
            }
    }
    // accumulator layout -> a lane's 2 x 8 consecutive couts (chunks nb * 4 + ch * 2 + fh) of its row
    auto to_rows = [&](const f32x16& v, float (&c)[2][8]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mg_u32x2 s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[e]), __float_as_uint(v[4 + e]), false, false);
            mg_u32x2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[8 + e]), __float_as_uint(v[12 + e]), false, false);
            c[0][e] = __uint_as_float(s0[0]); c[0][4 + e] = __uint_as_float(s0[1]);
            c[1][e] = __uint_as_float(s1[0]); c[1][4 + e] = __uint_as_float(s1[1]);
        }
    };
    // this lane's LDS rows: its own (live: inside the sequence) and the two it writes as the reflection of its own (-1: none)
    int lr_own[MB], lr_m0[MB], lr_m1[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int tr = wave * (MB * 32) + mb * 32 + fl, t = t_first + tr;
        lr_own[mb] = (t >= 0 && t < S) ? GUARD + tr : -1;
        const int m0 = GUARD - t - t_first;                    // LDS row of sequence row -t
        const int m1 = GUARD + 2 * (S - 1) - t - t_first;      // ... of 2 (S - 1) - t
        lr_m0[mb] = (t >= 1 && t <= GUARD && t < S && m0 >= 0) ? m0 : -1;
        lr_m1[mb] = (t <= S - 2 && t >= S - 1 - GUARD && t >= 0 && m1 < E + 2 * GUARD) ? m1 : -1;
    }
    // loop-invariant fragment addresses: weights (swizzled image: per cout block and k-slice), activation rows (padded)
    unsigned wa[NB][KS], xbase[MB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            wa[nb][ks] = (unsigned)(K::W_OFF + (nb * 32 + fl) * ROWB) + ((((unsigned)(2 * ks + fh)) ^ mg_wkey<C>((unsigned)(nb * 32 + fl))) << 4);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) xbase[mb] = (unsigned)((GUARD + wave * (MB * 32) + mb * 32 + fl) * STRIDE + fh * 16);

    auto init_bias = [&](f32x16 (&acc)[MB][NB], const float* bias) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bv = *reinterpret_cast<const float4*>(bias + nb * 32 + 8 * q + 4 * fh);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) { acc[mb][nb][4 * q] = bv.x; acc[mb][nb][4 * q + 1] = bv.y; acc[mb][nb][4 * q + 2] = bv.z; acc[mb][nb][4 * q + 3] = bv.w; }
            }
    };
    // a k = 1 convolution whose operand is in registers: pk[mb][ks] = the lane's 8 channels of k-slice ks (= nb * 2 + ch)
    auto mma_regs = [&](f32x16 (&acc)[MB][NB], const mg_u32x4 (&pk)[MB][KS], int wrow0) {
        const unsigned woff = (unsigned)(wrow0 * ROWB);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            mg_u32x4 wf[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) wf[nb] = *reinterpret_cast<const mg_u32x4*>(smem + woff + wa[nb][ks]);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[nb]), __builtin_bit_cast(bf16x8, pk[mb][ks]),
                                                                          acc[mb][nb], 0, 0, 0);
        }
    };
    auto pack8 = [&](const float (&c)[8], float slope) {
        mg_u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float lo = c[2 * e], hi = c[2 * e + 1];
            if (slope > 0.f) { lo = fmaxf(lo, lo * slope); hi = fmaxf(hi, hi * slope); }       // 0 < slope < 1
            o[e] = pack_bf16x2(lo, hi);
        }
        return o;
    };

    mg_u32x4 pk[MB][KS];
    for (int j = 0; j < 3; ++j) {
        const int d = j == 0 ? a.d[0] : (j == 1 ? a.d[1] : a.d[2]);       // (a dynamic index would put the argument block into scratch)
        __syncthreads();                       // every wave has finished the previous block's reads of the weight image and the tile
        store_w();
        // the tile <- lrelu(y) (own row when inside the sequence, and its reflections); pk <- raw y, the shortcut's operand
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float c[2][8];
                to_rows(y[mb][nb], c);
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    pk[mb][nb * 2 + ch] = pack8(c[ch], 0.f);
                    const mg_u32x4 o = pack8(c[ch], a.slope);
                    const unsigned coff = (unsigned)((nb * 4 + ch * 2 + fh) << 4);
                    if (lr_own[mb] >= 0) *reinterpret_cast<mg_u32x4*>(smem + (unsigned)lr_own[mb] * STRIDE + coff) = o;
                    if (lr_m0[mb] >= 0) *reinterpret_cast<mg_u32x4*>(smem + (unsigned)lr_m0[mb] * STRIDE + coff) = o;
                    if (lr_m1[mb] >= 0) *reinterpret_cast<mg_u32x4*>(smem + (unsigned)lr_m1[mb] * STRIDE + coff) = o;
                }
            }
        if (j < 2) fetch_w(j + 1);             // lands while this block multiplies
        __syncthreads();
        const float* bj = a.bias + j * 2 * C;
        // y <- b_shortcut + b_4 + W_shortcut . raw y
        init_bias(y, bj + C);
        mma_regs(y, pk, 3 * C);
        // t <- b_3 + conv3 (dilation d) over the tile
        init_bias(tacc, bj);
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int xoff = (tap - 1) * d * STRIDE;
            const unsigned woff = (unsigned)(tap * C * ROWB);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                mg_u32x4 wf[NB], xf[MB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) wf[nb] = *reinterpret_cast<const mg_u32x4*>(smem + woff + wa[nb][ks]);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) xf[mb] = *reinterpret_cast<const mg_u32x4*>(smem + (int)xbase[mb] + xoff + ks * 32);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        tacc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[nb]), __builtin_bit_cast(bf16x8, xf[mb]),
                                                                               tacc[mb][nb], 0, 0, 0);
            }
        }
        // y += W_4 . lrelu(t): the operand straight from the accumulators
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float c[2][8];
                to_rows(tacc[mb][nb], c);
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) pk[mb][nb * 2 + ch] = pack8(c[ch], a.slope);
            }
        mma_regs(y, pk, 4 * C);
    }

    // ---- store the tile's central R rows (leaky-ReLU'd when the consumer wants that)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int tr = wave * (MB * 32) + mb * 32 + fl;
        const int t = t_first + tr;
        const bool store = tr >= H && tr < H + a.R && t < S;         // (t >= 0 follows from tr >= H)
        bf16_t* row = Y + (size_t)(store ? t : 0) * a.ldy;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float c[2][8];
            to_rows(y[mb][nb], c);
            if (store) {
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) *reinterpret_cast<mg_u32x4*>(row + nb * 32 + ch * 16 + fh * 8) = pack8(c[ch], a.out_slope);
            }
        }
    }
}

template <int C>
static void launch_melgan_stage(const MelganStageArgs& a, int B, hipStream_t stream) {
    static Fs2DevOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)melgan_stage_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, MgCfg<C>::LDS); });
    melgan_stage_kernel<C><<<(unsigned)(B * a.tiles_per_seq), 512, MgCfg<C>::LDS, stream>>>(a);
}

extern "C" int fs2_melgan_stage_supported(int C, int dtype) { return dtype == FS2_BF16 && (C == 32 || C == 64) ? 1 : 0; }

extern "C" int fs2_melgan_stage_fwd(const void* x, long ldx, long x_bstride, const void* w, const float* bias, void* y, long ldy,
                                    long y_bstride, float slope, float out_slope, int B, int S, int C, int d0, int d1, int d2, int dtype,
                                    hipStream_t stream) {
    FS2_CHECK_ARG(x && w && bias && y, "melgan_stage_fwd: null pointer");
    FS2_CHECK_ARG(fs2_melgan_stage_supported(C, dtype), "melgan_stage_fwd: unsupported (C in {32, 64}, bf16)");
    const int G = MgCfg<32>::GUARD;
    FS2_CHECK_ARG(d0 >= 1 && d1 >= 1 && d2 >= 1 && d0 <= G && d1 <= G && d2 <= G, "melgan_stage_fwd: dilations in [1, %d]", G);
    // one reflection must land inside the sequence for every row a tile holds: S > GUARD + halo
    FS2_CHECK_ARG(B > 0 && S >= 32, "melgan_stage_fwd: bad shape B=%d S=%d (S >= 32)", B, S);
    FS2_CHECK_ARG(ldx % 8 == 0 && ldy % 8 == 0 && x_bstride % 8 == 0 && y_bstride % 8 == 0 && ldx >= C && ldy >= C &&
                  (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w | (uintptr_t)bias) & 15) == 0, "melgan_stage_fwd: rows must be 16-byte addressable");
    FS2_CHECK_ARG(slope > 0.f && slope < 1.f && out_slope >= 0.f && out_slope < 1.f, "melgan_stage_fwd: leaky-ReLU slope in (0, 1)");
    MelganStageArgs a = {};
    a.X = reinterpret_cast<const bf16_t*>(x); a.ldx = ldx; a.x_bs = x_bstride;
    a.W = reinterpret_cast<const bf16_t*>(w); a.bias = bias;
    a.Y = reinterpret_cast<bf16_t*>(y); a.ldy = ldy; a.y_bs = y_bstride;
    a.slope = slope; a.out_slope = out_slope; a.S = S; a.d[0] = d0; a.d[1] = d1; a.d[2] = d2;
    const int E = C == 32 ? MgCfg<32>::E : MgCfg<64>::E;
    a.R = E - 2 * (d0 + d1 + d2);
    a.tiles_per_seq = fs2_cdiv(S, a.R);
    if (C == 32) launch_melgan_stage<32>(a, B, stream);
    else launch_melgan_stage<64>(a, B, stream);
    FS2_CHECK_LAUNCH("melgan_stage_fwd");
    return FS2_OK;
}
