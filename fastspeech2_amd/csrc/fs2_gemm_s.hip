// fs2_gemm_s.hip - STREAMING kernel for the one-tap bf16 contractions with K = 256 (gfx950, round 4): the weights live in REGISTERS.
//
//   Y[m][n] = epilogue( sum_k X[m][k] * W[n][k] ),  K = Cin = 256, N a multiple of 256
//   nn.Linear / Conv1d(k = 1) of the FFT blocks with d_model on the reduction side: transformer/SubLayers.py:39-41 (w_qs / w_ks /
//   w_vs as one N = 768 matrix), :54 (fc) and its data gradient, and the data gradient of :88 (w_2: N = 1024, ReLU gate).
//
// Why another kernel.  These launches are HBM streams with almost no arithmetic (fc: 22.7 MB in, 22.7 MB out, 5.8 GFLOP), and
// round 3's wide kernel (fs2_gemm_w.hip, 256 x 256 tiles) runs them at 1.4-2.8 TB/s: 174 tiles for 256 CUs, ONE tile per
// workgroup - its operand loads, its MFMAs and its 128 KB of stores happen one after the other, nothing to pipeline against
// (profiles/r03w: 0.37 of the HBM roof, "every workgroup's first tile spends 57 k cycles in store back-pressure").  With K = 256 a
// wave can hold its whole weight slice in registers: 64 output columns x 256 k = 32 fragments of 4 registers = 128 VGPRs.  So:
//   * a workgroup owns 256 output columns (EIGHT consumer waves x 32 columns: 64 registers of weights each) and walks 64-row tiles
//     of X: the weights are fetched ONCE per workgroup, straight into registers, and never touch LDS; X goes through a 4-deep LDS
//     ring (32 KB per tile) by LDS-DMA;
//   * per tile a consumer wave reads 32 activation fragments and issues 32 MFMAs (no weight reads at all), then stores its
//     64 x 32 outputs from registers.  Two consumer waves share a SIMD: one's epilogue (residual / bias loads, stores) runs under
//     the other's MFMAs - the first cut, four 64-column waves alone on their SIMDs, paid every epilogue load's latency on the
//     tile's critical path and was slower than the wide kernel (r04t_bench_w.log);
//   * the LDS-DMA is issued by TWO loader waves that do nothing else: global stores share vmcnt with loads and may retire out
//     of order with them, so a wave that both prefetches with counted vmcnt and stores every tile cannot count (round 4's tall-tile kernel
//     drains once per tile; here a tile is too short for that).  One raw barrier per tile.
// LDS rows are 512 bytes (256 channels); the 32 16-byte chunks of a row are XOR-swizzled with (row & 15), which puts the 16 lanes of
// every ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...) on 16 different 16-byte bank groups.
// Lengths: with `lens` the epilogue zeroes padded rows, but every 64-row tile is still fetched and multiplied - this kernel takes no tile
// map (the loaders run three tiles ahead of the consumers on a counted vmcnt; a skip list would have to be shared between them before
// the first barrier).  The engine passes lens only to batches with >= 10 % wholly padded 256-row tiles (Engine._lens_pays); for those
// the K = 256 launches (qkv, fc, w_2 data gradient: 0.65 of the 8.4 ms LJSpeech step) do not shrink with the padding, the
// convolutions and the weight gradients do.
#include "fs2_gemm.h"
#include "fs2_gemm_epi.h"

static constexpr int S_TM = 64, S_K = 256, S_NBUF = 4;
static constexpr int S_TILE_BYTES = S_TM * S_K * 2;      // 32 KB
static constexpr int S_MAXB = 1024;                      // lens[] staged in LDS
static constexpr int S_AUX = S_MAXB * 4 + 3 * 256 * 4 + 2 * 8 * 64 * 4;               // lengths, bias / gamma / beta lines, row-sum exchange
static constexpr int S_LDS = S_NBUF * S_TILE_BYTES + S_AUX;                           // 139 KB
static constexpr int S_NLOAD = 2;                        // loader waves
static constexpr int S_CONS = 8;                         // consumer waves (32 output columns each)
static constexpr int S_THREADS = (S_CONS + S_NLOAD) * 64;

template <int N> __device__ __forceinline__ void s_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void s_barrier_mem() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// epilogue of one wave: 64 rows x 32 columns from the transposed accumulators (layout as p_epilogue, one column block)
// No global LOAD may sit behind the previous tile's stores on a tile's critical path (the compiler waits with vmcnt(0) for a
// loaded value once stores are pending too - loads and stores can retire out of order - so every tile would pay the store latency:
// the first cut of this epilogue ran 5 us per 64-row tile, waves parked 66 %, r04v_s_pmc_mfma.md): the bias line sits in registers
// (bb), the lengths in LDS (lens_s), and the residual / gate operand of THIS tile (rr) was requested before the tile's MFMAs.
//
// EPI: what the epilogue has to do, decided by the LAUNCHER and compiled in - bit 0 residual add, bit 1 ReLU gate on the residual
// operand, bit 2 lengths (padded rows zero), bit 3 "anything" (accumulate / out_scale != 1: every feature behind run-time flags, the
// first cut's form).  A wave issues about one instruction per 5 cycles and the run-time-flag form is 12 VALU per output element
// (selects for flags that are off, a multiply by 1.0, the unpacking of a residual that is not there): the epilogue, not the MFMAs or
// the stream, was the longest phase of a tile (r04x_s_abl.log).  Compiled for what the launch needs it is 3-6.
enum { S_EPI_RES = 1, S_EPI_GATE = 2, S_EPI_LENS = 4, S_EPI_ANY = 8, S_EPI_LN = 16 };
// gemm_res_ln on this kernel (EPI = S_EPI_LN; N = 256, so the workgroup's eight waves hold whole rows): the epilogue of fs2_gemm_w.hip's
// w_epilogue_resln in this kernel's layout - z = dropout(acc + bias) + res stored bf16 (saved for backward), statistics on the values
// AS STORED, two passes (mean, then squared deviations), each row's eight per-wave partial sums exchanged through LDS behind one
// barrier per pass (the loader waves pass the same barriers), out = mask(LN(z) gamma + beta), mean / rstd saved.
// transformer/SubLayers.py:54-55 + Layers.py:25 (fc -> dropout -> + residual -> LayerNorm -> masked_fill).
__device__ __forceinline__ void s_epilogue_ln(const ConvGemmArgs& a, const WLn& ln, f32x16 (&acc)[2][1], int m0, int nbase, int wave, int fl, int fh,
                                              const float* bias_s, const float* gamma_s, const float* beta_s, const int32_t* lens_s,
                                              const uint4 (&rr)[2][2], float* red, uint64_t seed, float ik) {
    bf16_t* Z = reinterpret_cast<bf16_t*>(a.Y);
    bf16_t* O = reinterpret_cast<bf16_t*>(ln.out);
    float rsum[2] = {0.f, 0.f};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int m = m0 + mb * 32 + fl;
        const bool rowok = m < a.M;
        float v[16];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u32x2 s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mb][0][e]), __float_as_uint(acc[mb][0][4 + e]), false, false);
            u32x2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mb][0][8 + e]), __float_as_uint(acc[mb][0][12 + e]), false, false);
            v[e] = __uint_as_float(s0[0]); v[4 + e] = __uint_as_float(s0[1]);
            v[8 + e] = __uint_as_float(s1[0]); v[12 + e] = __uint_as_float(s1[1]);
        }
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const int n = nbase + ch * 16 + fh * 8;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = v[ch * 8 + e] + bias_s[ch * 8 + e];
            if (ln.p_pre > 0.f) {
                const uint32_t e0 = (uint32_t)m * 256u + (uint32_t)n;
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] *= fs2_drop_scale(seed, e0 + e, ln.p_pre, ik);
            }
            if (a.R) {
                const uint32_t* u = reinterpret_cast<const uint32_t*>(&rr[mb][ch]);
#pragma unroll
                for (int e = 0; e < 4; ++e) { x[2 * e] += __uint_as_float(u[e] << 16); x[2 * e + 1] += __uint_as_float(u[e] & 0xffff0000u); }
            }
            uint4 zq;
            uint32_t* zu = reinterpret_cast<uint32_t*>(&zq);
#pragma unroll
            for (int e = 0; e < 4; ++e) zu[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
            if (rowok) *reinterpret_cast<uint4*>(Z + (size_t)m * a.ldy + n) = zq;
#pragma unroll
            for (int e = 0; e < 4; ++e) {                // statistics on the values as stored: backward sees the same z
                const float lo = __uint_as_float(zu[e] << 16), hi = __uint_as_float(zu[e] & 0xffff0000u);
                acc[mb][0][ch * 8 + 2 * e] = lo; acc[mb][0][ch * 8 + 2 * e + 1] = hi;
                rsum[mb] += lo + hi;
            }
        }
    }
    // ---- row means: lane pair, then the eight waves through LDS
    float mean[2], rstd[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        rsum[mb] += __shfl_xor(rsum[mb], 32, 64);
        if (fh == 0) red[wave * 64 + mb * 32 + fl] = rsum[mb];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += red[w * 64 + mb * 32 + fl];         // (same order in every wave: one mean per row)
        mean[mb] = t * (1.f / 256.f);
    }
    float rsq[2] = {0.f, 0.f};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float d = acc[mb][0][r] - mean[mb]; rsq[mb] += d * d; }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        rsq[mb] += __shfl_xor(rsq[mb], 32, 64);
        if (fh == 0) red[512 + wave * 64 + mb * 32 + fl] = rsq[mb];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += red[512 + w * 64 + mb * 32 + fl];
        rstd[mb] = rsqrtf(t * (1.f / 256.f) + ln.eps);
    }
    // ---- normalise, scale, mask, store
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int m = m0 + mb * 32 + fl;
        if (m >= a.M) continue;
        bool padrow = false;
        if (a.lens) { const int b = m / a.S; padrow = (m - b * a.S) >= lens_s[b]; }
        if (wave == 0 && fh == 0) { ln.mean[m] = mean[mb]; ln.rstd[m] = rstd[mb]; }
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const int n = nbase + ch * 16 + fh * 8;
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = padrow ? 0.f : (acc[mb][0][ch * 8 + e] - mean[mb]) * rstd[mb] * gamma_s[ch * 8 + e] + beta_s[ch * 8 + e];
            uint4 oq;
            uint32_t* ou = reinterpret_cast<uint32_t*>(&oq);
#pragma unroll
            for (int e = 0; e < 4; ++e) ou[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
            *reinterpret_cast<uint4*>(O + (size_t)m * ln.ldo + n) = oq;
        }
    }
}

template <int ACT, int EPI>
__device__ __forceinline__ void s_epilogue(const ConvGemmArgs& a, f32x16 (&acc)[2][1], int m0, int nbase, int fl, int fh,
                                           const float* bias_s, const int32_t* lens_s, const uint4 (&rr)[2][2]) {
    constexpr bool ANY = (EPI & S_EPI_ANY) != 0;
    bf16_t* Y = reinterpret_cast<bf16_t*>(a.Y);
    const bool has_r = ANY ? a.R != nullptr : (EPI & (S_EPI_RES | S_EPI_GATE)) != 0;
    const bool gate = ANY ? a.act == FS2_ACT_GATE : (EPI & S_EPI_GATE) != 0;
    const bool has_lens = ANY ? a.lens != nullptr : (EPI & S_EPI_LENS) != 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int m = m0 + mb * 32 + fl;
        const bool rowok = m < a.M;
        bool padrow = false;
        if (has_lens && rowok) { const int b = m / a.S; padrow = (m - b * a.S) >= lens_s[b]; }
        bf16_t* yrow = Y + (size_t)m * a.ldy;
#pragma unroll
        for (int nb = 0; nb < 1; ++nb) {
            float c[2][8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                u32x2 s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mb][nb][e]), __float_as_uint(acc[mb][nb][4 + e]), false, false);
                u32x2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mb][nb][8 + e]), __float_as_uint(acc[mb][nb][12 + e]), false, false);
                c[0][e] = __uint_as_float(s0[0]); c[0][4 + e] = __uint_as_float(s0[1]);
                c[1][e] = __uint_as_float(s1[0]); c[1][4 + e] = __uint_as_float(s1[1]);
            }
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const int n = nbase + nb * 32 + ch * 16 + fh * 8;
                if (!rowok) continue;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = act_ct<ACT>(c[ch][e] + bias_s[ch * 8 + e], a.slope);   // (zeros without a bias)
                if (has_r) {
                    const uint32_t* u = reinterpret_cast<const uint32_t*>(&rr[mb][ch]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r0 = __uint_as_float(u[e] << 16), r1 = __uint_as_float(u[e] & 0xffff0000u);
                        v[2 * e] = gate ? (r0 > 0.f ? v[2 * e] : 0.f) : v[2 * e] + r0;
                        v[2 * e + 1] = gate ? (r1 > 0.f ? v[2 * e + 1] : 0.f) : v[2 * e + 1] + r1;
                    }
                }
                if (ANY) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= a.out_scale;
                }
                if (has_lens) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (padrow) v[e] = 0.f;
                }
                if (ANY && a.accumulate) {
                    const uint4 yy = *reinterpret_cast<const uint4*>(yrow + n);
                    const uint32_t* u = reinterpret_cast<const uint32_t*>(&yy);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[2 * e] += __uint_as_float(u[e] << 16); v[2 * e + 1] += __uint_as_float(u[e] & 0xffff0000u); }
                }
                uint4 o;
                uint32_t* ou = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
                for (int e = 0; e < 4; ++e) ou[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                *reinterpret_cast<uint4*>(yrow + n) = o;
            }
        }
    }
}

// grid stripes * (N / 256), 1-D: a workgroup walks the 64-row tiles stripe, stripe + stripes, ... of one 256-column group
// Measured and not kept: the second wave of each SIMD (waves 4..7) running its epilogue one barrier LATE, so that on every SIMD one
// wave's MFMAs overlap the other's epilogue VALU work (r04x_s_skew.log; wave i sits on SIMD {3,0,2,1}[i % 4], so waves w and w + 4
// do share one): no gain from any pairing - the kernel is bound by bytes moved per CU, not by issue slots.
template <int EPI>
__global__ void __launch_bounds__(S_THREADS) conv_gemm_s_kernel(ConvGemmArgs a, WLn ln, int ntiles, int stripes, int groups) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 1-D grid, XCD-aware: workgroups are dealt round-robin over the 8 XCDs, and the `groups` workgroups that stream the SAME rows
    // (one per 256-column group) must share an L2, or every X tile crosses the fabric `groups` times: id -> (xcd = id % 8,
    // slot = id / 8), column group = slot % groups, row stripe = (slot / groups) * 8 + xcd.  (stripes is a multiple of 8, or
    // groups == 1, by the launcher.)
    const int bid = (int)blockIdx.x;
    const int slot = bid >> 3;
    const int col_group = groups == 1 ? 0 : slot % groups;
    const int stripe = groups == 1 ? bid : (slot / groups) * 8 + (bid & 7);
    const int my_tiles = (ntiles - stripe + stripes - 1) / stripes;
    if (my_tiles <= 0) return;                               // (whole workgroup: a stripe past the last tile)
    const unsigned smem_u = lds_addr(smem);

    if (wave >= S_CONS) {
        // ------------------------------------------------------------------ loader waves: LDS-DMA only, counted vmcnt
        const int lw = wave - S_CONS;
        const unsigned char* Xb = reinterpret_cast<const unsigned char*>(a.X);
        const unsigned ldx2 = (unsigned)(a.ldx * 2);
        const int hi = lane >> 5, pos = lane & 31;
        auto issue = [&](int t) {                            // tile t of this workgroup -> buffer t % S_NBUF (4); 16 pieces of 2 rows
            const int m0 = (stripe + t * stripes) * S_TM;
            const unsigned dst0 = smem_u + (unsigned)((t % S_NBUF) * S_TILE_BYTES);
#pragma unroll
            for (int i = 0; i < 32 / S_NLOAD; ++i) {
                const int j = lw + S_NLOAD * i;              // piece: rows 2j, 2j + 1
                const int row = 2 * j + hi;
                const int g = min(m0 + row, a.M - 1);
                const unsigned voff = (unsigned)g * ldx2 + (unsigned)((pos ^ (row & 15)) << 4);
                glds16_sbase(voff, Xb, __builtin_amdgcn_readfirstlane(dst0 + (unsigned)(j * 1024)));
            }
        };
        issue(0);
        if (my_tiles > 1) issue(1);
        if (my_tiles > 2) issue(2);
        for (int t = 0; t < my_tiles; ++t) {
            // my pieces of tile t have landed: at most the tiles behind it (two, one or none) may still be in flight
            if (t + 2 < my_tiles) s_wait_vm<2 * (32 / S_NLOAD)>();
            else if (t + 1 < my_tiles) s_wait_vm<32 / S_NLOAD>();
            else s_wait_vm<0>();
            s_barrier_mem();                                 // tile t published; the buffer of tile t - 1 released
            if (t + 3 < my_tiles) issue(t + 3);
            if (EPI & S_EPI_LN) { s_barrier_mem(); s_barrier_mem(); }        // (the consumers' two row-sum exchanges)
        }
        return;
    }

    // ------------------------------------------------------------------ consumer waves
    const int fl = lane & 31, fh = lane >> 5;
    const int nbase = col_group * 256 + wave * 32;
    // the wave's weight slice, once, straight into registers: B fragment ks = rows nbase + fl, k = 16 ks + 8 fh .. + 8
    u32x4 Wf[16];
    {
        const unsigned char* wrow = reinterpret_cast<const unsigned char*>(a.W) + (size_t)(nbase + fl) * (size_t)(a.ldw * 2) + fh * 16;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) Wf[ks] = *reinterpret_cast<const u32x4*>(wrow + ks * 32);
    }
    // the workgroup's bias line and the lengths in LDS (written before the first barrier, which every wave passes before any epilogue).
    // bias layout: [wave][half][run][8] so that a lane reads its two 8-column runs as 16 consecutive floats
    int32_t* lens_s = reinterpret_cast<int32_t*>(smem + S_NBUF * S_TILE_BYTES);
    float* bias_all = reinterpret_cast<float*>(smem + S_NBUF * S_TILE_BYTES + S_MAXB * 4);
    float* gamma_all = bias_all + 256;
    float* beta_all = bias_all + 512;
    float* red = bias_all + 768;                             // [2][8 waves][64 rows]
    if (tid < 256) {
        const int w_ = tid >> 5, r_ = tid & 31, ch_ = r_ >> 4, fh_ = (r_ >> 3) & 1, e_ = r_ & 7;
        const int slot = w_ * 32 + fh_ * 16 + ch_ * 8 + e_;
        bias_all[slot] = a.bias ? a.bias[col_group * 256 + tid] : 0.f;
        if (EPI & S_EPI_LN) { gamma_all[slot] = ln.gamma[tid]; beta_all[slot] = ln.beta[tid]; }
    }
    if (a.lens) {
        const int Bq = a.M / a.S;
        for (int i = tid; i < Bq; i += S_CONS * 64) lens_s[i] = a.lens[i];
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const float* bias_s = bias_all + wave * 32 + fh * 16;
    const float* gamma_s = gamma_all + wave * 32 + fh * 16;
    const float* beta_s = beta_all + wave * 32 + fh * 16;
    const uint64_t ln_seed = (EPI & S_EPI_LN) ? ln.seed_pre + (ln.seed_dev ? *ln.seed_dev : 0ull) : 0ull;
    const float ln_ik = ((EPI & S_EPI_LN) && ln.p_pre > 0.f) ? 1.f / (1.f - ln.p_pre) : 1.f;
    const bf16_t* Rb = reinterpret_cast<const bf16_t*>(a.R);
    const unsigned arow = (unsigned)(fl * 512);              // byte offset of the lane's row (second row block: + 32 rows)
    unsigned akey = (unsigned)(fl & 15);
    f32x16 acc[2][1];
    uint4 rr[2][2];
    int m0 = 0;
    for (int t = 0; t < my_tiles; ++t) {
        s_barrier_mem();                                     // tile t has landed (all loader pieces)
        asm volatile("" : "+v"(akey));                       // (keeps the 16 swizzled column offsets from being hoisted into 16 registers:
                                                             //  the budget is 168 with 10 waves, and a spill is a scratch LOAD per tile)
        const unsigned char* buf = smem + (t % S_NBUF) * S_TILE_BYTES;
        m0 = (stripe + t * stripes) * S_TM;
        // this tile's residual / gate operand: requested NOW, used after the MFMAs
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int m = min(m0 + mb * 32 + fl, a.M - 1);
#pragma unroll
            for (int ch = 0; ch < 2; ++ch)
                rr[mb][ch] = ((EPI & (S_EPI_ANY | S_EPI_LN)) ? Rb != nullptr : (EPI & (S_EPI_RES | S_EPI_GATE)) != 0)
                                 ? *reinterpret_cast<const uint4*>(Rb + (size_t)m * a.ldr + nbase + ch * 16 + fh * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const unsigned coff = ((unsigned)(2 * ks + fh) ^ akey) << 4;
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(buf + arow + coff);
            const u32x4 a1 = *reinterpret_cast<const u32x4*>(buf + arow + 32 * 512 + coff);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, Wf[ks]), __builtin_bit_cast(bf16x8, a0), acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, Wf[ks]), __builtin_bit_cast(bf16x8, a1), acc[1][0], 0, 0, 0);
        }
        if (EPI & S_EPI_LN) {
            s_epilogue_ln(a, ln, acc, m0, nbase, wave, fl, fh, bias_s, gamma_s, beta_s, lens_s, rr, red, ln_seed, ln_ik);
        } else if (EPI & S_EPI_ANY) {
            FS2_ACT_DISPATCH(a.act, (s_epilogue<ACT, EPI>(a, acc, m0, nbase, fl, fh, bias_s, lens_s, rr)));
        } else if (a.act == FS2_ACT_RELU) {                  // (tanh / leaky ReLU launches take the S_EPI_ANY kernel)
            s_epilogue<FS2_ACT_RELU, EPI>(a, acc, m0, nbase, fl, fh, bias_s, lens_s, rr);
        } else {
            s_epilogue<FS2_ACT_NONE, EPI>(a, acc, m0, nbase, fl, fh, bias_s, lens_s, rr);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launcher
static int s_cu_count() {
    static int cus[64] = {0};
    int d = 0;
    (void)hipGetDevice(&d);
    d &= 63;
    if (!cus[d]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
        cus[d] = n;
    }
    return cus[d];
}

// Eligibility (pure function of the launch description): one tap, K = 256 exactly, N a multiple of 256, 16-byte rows; at least as
// many 64-row tiles as would give every CU one (fewer: the small-M kernels keep the launch)
bool fs2_conv_gemm_s_ok(const ConvGemmArgs& a, int dtype) {
    if (dtype != FS2_BF16 || a.taps != 1 || a.in_act != FS2_ACT_NONE) return false;
    if (a.Cin != S_K || a.N % 256 != 0 || a.N > 256 * 64 || !a.vec_ok || a.ldx % 8 != 0) return false;
    if (a.lens && a.M / a.S > S_MAXB) return false;
    if ((double)a.M * a.ldx * 2 >= 4.0e9) return false;
    return (long)fs2_cdiv(a.M, S_TM) * (a.N / 256) >= s_cu_count();
}

template <int EPI>
static void s_launch_one(const ConvGemmArgs& a, dim3 grid, int ntiles, int stripes, int groups, hipStream_t stream, const WLn& ln = WLn{}) {
    static Fs2DevOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)conv_gemm_s_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, S_LDS); });
    conv_gemm_s_kernel<EPI><<<grid, S_THREADS, S_LDS, stream>>>(a, ln, ntiles, stripes, groups);
}

void fs2_conv_gemm_s_launch(const ConvGemmArgs& a, hipStream_t stream) {
    const int ntiles = fs2_cdiv(a.M, S_TM), groups = a.N / 256;
    // one workgroup per CU (133 KB of LDS); with several column groups the stripe count is a multiple of 8 (see the kernel's map)
    int stripes = s_cu_count() / groups;
    if (groups > 1) stripes = stripes / 8 * 8;
    if (stripes > ntiles) stripes = groups > 1 ? ntiles / 8 * 8 : ntiles;
    if (stripes < 8) { stripes = 8; }                        // (tiles past ntiles: a stripe with no tile returns at once)
    const dim3 grid((unsigned)(stripes * groups));
    // the epilogue this launch needs (see s_epilogue): accumulate / a scale fall back to the run-time-flag form
    const bool gate = a.act == FS2_ACT_GATE;
    const bool odd_act = a.act == FS2_ACT_TANH || a.act == FS2_ACT_LRELU;
    int epi = (a.accumulate || a.out_scale != 1.0f || (gate && !a.R) || odd_act) ? S_EPI_ANY
              : ((a.R ? (gate ? S_EPI_GATE : S_EPI_RES) : 0) | (a.lens ? S_EPI_LENS : 0));
    switch (epi) {
        case 0: s_launch_one<0>(a, grid, ntiles, stripes, groups, stream); break;
        case S_EPI_RES: s_launch_one<S_EPI_RES>(a, grid, ntiles, stripes, groups, stream); break;
        case S_EPI_GATE: s_launch_one<S_EPI_GATE>(a, grid, ntiles, stripes, groups, stream); break;
        case S_EPI_LENS: s_launch_one<S_EPI_LENS>(a, grid, ntiles, stripes, groups, stream); break;
        case S_EPI_RES | S_EPI_LENS: s_launch_one<S_EPI_RES | S_EPI_LENS>(a, grid, ntiles, stripes, groups, stream); break;
        case S_EPI_GATE | S_EPI_LENS: s_launch_one<S_EPI_GATE | S_EPI_LENS>(a, grid, ntiles, stripes, groups, stream); break;
        default: s_launch_one<S_EPI_ANY>(a, grid, ntiles, stripes, groups, stream); break;
    }
}

// ---- gemm_res_ln on the streaming kernel (called by fs2_gemm_res_ln_fwd, fs2_gemm_w.hip)
bool fs2_conv_gemm_s_ln_ok(const ConvGemmArgs& a, int dtype) {
    return a.N == 256 && a.act == FS2_ACT_NONE && !a.accumulate && a.out_scale == 1.0f && fs2_conv_gemm_s_ok(a, dtype);
}

void fs2_conv_gemm_s_ln_launch(const ConvGemmArgs& a, const WLn& ln, hipStream_t stream) {
    const int ntiles = fs2_cdiv(a.M, S_TM);
    int stripes = s_cu_count();
    if (stripes > ntiles) stripes = ntiles;
    s_launch_one<S_EPI_LN>(a, dim3((unsigned)stripes), ntiles, stripes, 1, stream, ln);
}
