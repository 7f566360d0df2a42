// fs2_g2p.hip — grapheme-to-phoneme conversion by a joint-sequence (graphone) n-gram: the many-to-many EM alignment of a lexicon's
// spellings with its pronunciations, and the beam search that pronounces a new word, on ragged batches of words, all in fp64.
// The specification is the docstring of fastspeech2_amd/g2p.py (summarised in DESIGN.md); tests/g2p_ref.py restates it in numpy.
//
// Shapes.  Word w has Lg = glens[w] letters (index i) and Lp = plens[w] phones (index j), ids in int32 rows letters[w][0..Lg) and
// phones[w][0..Lp); an id outside [0, A) / [0, P) makes every arc over it absent.  The lattice has the cells (i, j), i <= Lg, j <= Lp,
// and four arcs per cell, code c consuming (dl, dp) = (1,0), (1,1), (1,2), (2,1) letters and phones.  The graphone type of an arc is
// an index into the dense table log theta[A NQ + A A P], NQ = 1 + P + P P:
//     codes 0..2   a NQ + q        a the letter, q = 0 | 1 + p | 1 + P + p0 P + p1 the phone chunk
//     code 3       A NQ + (a0 A + a1) P + p
// so the kernels need the padded id rows alone.  Nothing at i >= Lg or j >= Lp of a row is read and nothing outside a word's own
// cells is written (the tests poison both).  No atomics; every sum has one order.
//
//   fs2_g2p_m2m_expect   one wave per word, lane i, one anti-diagonal s = i + j per step.  A lane keeps its own last three values;
//                        the four predecessors alpha(i-1, j), alpha(i-1, j-1), alpha(i-1, j-2), alpha(i-2, j-1) are lane i-1's values
//                        of one, two and three steps ago and lane i-2's of three steps ago: four wave shuffles, no barrier.  alpha
//                        goes to LDS, written and read back by the same lane; the backward pass mirrors the forward one and forms
//                        the posteriors of the arcs that leave its cell on the way
//   fs2_g2p_m2m_viterbi  the forward pass with max and a byte of backpointer per cell (the host walks them)
//   fs2_g2p_ngram_score  log P(token | history) of a back-off n-gram held as sorted packed keys: binary searches down the orders
//   fs2_g2p_decode       one workgroup per word: beam search, synchronous in the letter position, candidates scored with the same
//                        device function into a scratch row, the K best taken by K rounds of arg-max (ties to the lower index)
#include "fs2_common.h"

#define G2P_MAX_LETTERS 64
#define G2P_MAX_PHONES 128
#define G2P_MAX_LG 32               // letters per word: Lg + 1 lanes of one wave
#define G2P_MAX_LP 48
#define G2P_MAX_BEAM 256
#define G2P_MAX_ORDER 4             // four 16-bit ids in one key
#define G2P_WPB 4                   // words per workgroup, one wave each
#define G2P_NT 256

static __device__ __forceinline__ int g2p_len(const int32_t* lens, int w, int cap) { return min(max(lens[w], 0), cap); }
static __device__ __forceinline__ double g2p_ninf() { return -__builtin_huge_val(); }

// the dense index of an arc's type, -1 when an id is outside the alphabets: a1 / p1 the arc's last letter / phone, a0 / p0 the one before
static __device__ __forceinline__ long g2p_type(int code, int a0, int a1, int p0, int p1, int A, int P) {
    const long NQ = 1 + P + (long)P * P;
    const bool la = (unsigned)a1 < (unsigned)A, lp = (unsigned)p1 < (unsigned)P;
    if (code == 0) return la ? a1 * NQ : -1;
    if (code == 1) return la && lp ? a1 * NQ + 1 + p1 : -1;
    if (code == 2) return la && lp && (unsigned)p0 < (unsigned)P ? a1 * NQ + 1 + P + (long)p0 * P + p1 : -1;
    return la && lp && (unsigned)a0 < (unsigned)A ? A * NQ + ((long)a0 * A + a1) * P + p1 : -1;
}
static __device__ __forceinline__ double g2p_arc(const double* __restrict__ lt, bool exists, long type) {
    return exists && type >= 0 ? lt[type] : g2p_ninf();
}
// log(sum of exp) of the four terms in arc-code order; -inf when all four are
static __device__ __forceinline__ double g2p_lse4(double t0, double t1, double t2, double t3) {
    const double m = fmax(fmax(t0, t1), fmax(t2, t3));
    if (m == g2p_ninf()) return m;
    return m + log(exp(t0 - m) + exp(t1 - m) + exp(t2 - m) + exp(t3 - m));
}

// The log weights of the four arcs that ENTER cell (i, j): l1 = letters[i - 1], l0 = letters[i - 2], phones from the LDS row.
static __device__ __forceinline__ void g2p_in_arcs(const double* __restrict__ lt, const int* ph, int i, int j, int l0, int l1, int A,
                                                   int P, double t[4]) {
    const int p1 = j >= 1 ? ph[j - 1] : -1, p0 = j >= 2 ? ph[j - 2] : -1;
    t[0] = g2p_arc(lt, i >= 1, g2p_type(0, l0, l1, p0, p1, A, P));
    t[1] = g2p_arc(lt, i >= 1 && j >= 1, g2p_type(1, l0, l1, p0, p1, A, P));
    t[2] = g2p_arc(lt, i >= 1 && j >= 2, g2p_type(2, l0, l1, p0, p1, A, P));
    t[3] = g2p_arc(lt, i >= 2 && j >= 1, g2p_type(3, l0, l1, p0, p1, A, P));
}

#define G2P_STAGE_WORD()                                                                                          \
    const int wv = threadIdx.x >> 6, i = threadIdx.x & 63, w = blockIdx.x * G2P_WPB + wv;                         \
    const bool live = w < W;                                                                                      \
    const int Lg = live ? g2p_len(glens, w, Lgmax) : 0, Lp = live ? g2p_len(plens, w, Lpmax) : 0;                 \
    for (int j = i; j < Lp; j += 64) ph[wv][j] = phones[(size_t)w * ldp + j];                                     \
    __syncthreads();                                                                                              \
    const double NINF = g2p_ninf();                                                                               \
    const int32_t* lw = letters + (size_t)(live ? w : 0) * ldl

// ------------------------------------------------------------------ E-step
// post[w][i][j][c], i < Lg, j <= Lp: the posterior of the arc of code c that LEAVES cell (i, j),
// exp((alpha(i, j) + (log theta + beta(i', j'))) - loglik), exactly 0 for an arc that does not exist or lies on no path.
__global__ void __launch_bounds__(G2P_NT) g2p_expect_kernel(const int32_t* __restrict__ letters, long ldl, const int32_t* __restrict__ phones,
                                                            long ldp, const int32_t* __restrict__ glens, const int32_t* __restrict__ plens,
                                                            const double* __restrict__ lt, int A, int P, double* __restrict__ loglik,
                                                            double* __restrict__ post, long ldo_w, long ldo_i, int W, int Lgmax,
                                                            int Lpmax) {
    __shared__ double alpha[G2P_WPB][G2P_MAX_LP + 1][G2P_MAX_LG + 1];
    __shared__ int ph[G2P_WPB][G2P_MAX_LP];
    G2P_STAGE_WORD();
    const int l1 = (i >= 1 && i <= Lg) ? lw[i - 1] : -1, l0 = (i >= 2 && i <= Lg) ? lw[i - 2] : -1;
    const int nsteps = Lg + Lp;
    double d1 = NINF, d2 = NINF, d3 = NINF;
    for (int s = 0; s <= nsteps; ++s) {
        const double a1 = __shfl_up(d1, 1, 64), a2 = __shfl_up(d2, 1, 64), a3 = __shfl_up(d3, 1, 64), a4 = __shfl_up(d3, 2, 64);
        const int j = s - i;
        double v = NINF;
        if (live && i <= Lg && j >= 0 && j <= Lp) {
            if (s == 0) {
                v = 0.0;
            } else {
                double t[4];
                g2p_in_arcs(lt, ph[wv], i, j, l0, l1, A, P, t);
                v = g2p_lse4(i >= 1 ? a1 + t[0] : NINF, i >= 1 ? a2 + t[1] : NINF, i >= 1 ? a3 + t[2] : NINF, i >= 2 ? a4 + t[3] : NINF);
            }
            alpha[wv][j][i] = v;
        }
        d3 = d2;
        d2 = d1;
        d1 = v;
    }
    const double ll = __shfl(d1, Lg, 64);                                  // alpha(Lg, Lp), lane Lg's last value
    if (live && i == 0) loglik[w] = ll;
    // backward: e1..e3 are this lane's beta one, two and three anti-diagonals later
    const int n1 = i + 1 <= Lg ? lw[i] : -1, n2 = i + 2 <= Lg ? lw[i + 1] : -1;
    double e1 = NINF, e2 = NINF, e3 = NINF;
    for (int s = nsteps; s >= 0; --s) {
        const double b1 = __shfl_down(e1, 1, 64), b2 = __shfl_down(e2, 1, 64), b3 = __shfl_down(e3, 1, 64), b4 = __shfl_down(e3, 2, 64);
        const int j = s - i;
        double v = NINF;
        if (live && i <= Lg && j >= 0 && j <= Lp) {
            const int q1 = j + 1 <= Lp ? ph[wv][j] : -1, q2 = j + 2 <= Lp ? ph[wv][j + 1] : -1;
            const bool x0 = i + 1 <= Lg, x1 = x0 && j + 1 <= Lp, x2 = x0 && j + 2 <= Lp, x3 = i + 2 <= Lg && j + 1 <= Lp;
            const double u0 = x0 ? g2p_arc(lt, true, g2p_type(0, -1, n1, -1, -1, A, P)) + b1 : NINF;
            const double u1 = x1 ? g2p_arc(lt, true, g2p_type(1, -1, n1, -1, q1, A, P)) + b2 : NINF;
            const double u2 = x2 ? g2p_arc(lt, true, g2p_type(2, -1, n1, q1, q2, A, P)) + b3 : NINF;
            const double u3 = x3 ? g2p_arc(lt, true, g2p_type(3, n1, n2, -1, q1, A, P)) + b4 : NINF;
            v = (i == Lg && j == Lp) ? 0.0 : g2p_lse4(u0, u1, u2, u3);
            if (i < Lg) {
                const double a = alpha[wv][j][i];
                double* o = post + (size_t)w * ldo_w + (size_t)i * ldo_i + (size_t)j * 4;
                const bool path = ll != NINF;
                o[0] = path && x0 ? exp((a + u0) - ll) : 0.0;
                o[1] = path && x1 ? exp((a + u1) - ll) : 0.0;
                o[2] = path && x2 ? exp((a + u2) - ll) : 0.0;
                o[3] = path && x3 ? exp((a + u3) - ll) : 0.0;
            }
        }
        e3 = e2;
        e2 = e1;
        e1 = v;
    }
}

// ------------------------------------------------------------------ Viterbi
// bp[w][i][j], i <= Lg, j <= Lp: the code of the best arc into (i, j), 255 for (0, 0) and for a cell no path reaches; a later code
// wins only when strictly larger, so the lowest code wins ties.  Only adds and compares of the table's values: exact.
__global__ void __launch_bounds__(G2P_NT) g2p_viterbi_kernel(const int32_t* __restrict__ letters, long ldl, const int32_t* __restrict__ phones,
                                                             long ldp, const int32_t* __restrict__ glens, const int32_t* __restrict__ plens,
                                                             const double* __restrict__ lt, int A, int P, double* __restrict__ score,
                                                             uint8_t* __restrict__ bp, long ldb_w, long ldb_i, int W, int Lgmax,
                                                             int Lpmax) {
    __shared__ int ph[G2P_WPB][G2P_MAX_LP];
    G2P_STAGE_WORD();
    const int l1 = (i >= 1 && i <= Lg) ? lw[i - 1] : -1, l0 = (i >= 2 && i <= Lg) ? lw[i - 2] : -1;
    const int nsteps = Lg + Lp;
    double d1 = NINF, d2 = NINF, d3 = NINF;
    for (int s = 0; s <= nsteps; ++s) {
        const double a1 = __shfl_up(d1, 1, 64), a2 = __shfl_up(d2, 1, 64), a3 = __shfl_up(d3, 1, 64), a4 = __shfl_up(d3, 2, 64);
        const int j = s - i;
        double v = NINF;
        if (live && i <= Lg && j >= 0 && j <= Lp) {
            int code = 255;
            if (s == 0) {
                v = 0.0;
            } else {
                double t[4];
                g2p_in_arcs(lt, ph[wv], i, j, l0, l1, A, P, t);
                const double c0 = i >= 1 ? a1 + t[0] : NINF, c1 = i >= 1 ? a2 + t[1] : NINF, c2 = i >= 1 ? a3 + t[2] : NINF,
                             c3 = i >= 2 ? a4 + t[3] : NINF;
                v = c0;
                code = 0;
                if (c1 > v) { v = c1; code = 1; }
                if (c2 > v) { v = c2; code = 2; }
                if (c3 > v) { v = c3; code = 3; }
                if (v == NINF) code = 255;
            }
            bp[(size_t)w * ldb_w + (size_t)i * ldb_i + j] = (uint8_t)code;
        }
        d3 = d2;
        d2 = d1;
        d1 = v;
    }
    const double best = __shfl(d1, Lg, 64);
    if (live && i == 0) score[w] = best;
}

extern "C" int fs2_g2p_max_letters(void) { return G2P_MAX_LETTERS; }
extern "C" int fs2_g2p_max_phones(void) { return G2P_MAX_PHONES; }
extern "C" int fs2_g2p_max_word_letters(void) { return G2P_MAX_LG; }
extern "C" int fs2_g2p_max_word_phones(void) { return G2P_MAX_LP; }
extern "C" int fs2_g2p_max_beam(void) { return G2P_MAX_BEAM; }
extern "C" int fs2_g2p_max_order(void) { return G2P_MAX_ORDER; }
extern "C" int fs2_g2p_max_table_mib(void) { return 64; }

static long g2p_table_size(int A, int P) { return (long)A * (1 + P + (long)P * P) + (long)A * A * P; }

#define G2P_LATTICE_ARGS(name)                                                                                                     \
    FS2_CHECK_ARG(A >= 1 && A <= G2P_MAX_LETTERS && P >= 1 && P <= G2P_MAX_PHONES, name ": %d letters (1..%d), %d phones (1..%d)", A, \
                  G2P_MAX_LETTERS, P, G2P_MAX_PHONES);                                                                             \
    FS2_CHECK_ARG(n_table == g2p_table_size(A, P) && n_table * 8 <= ((long)fs2_g2p_max_table_mib() << 20),                          \
                  name ": table of %ld entries, expected %ld (at most %d MiB)", n_table, g2p_table_size(A, P), fs2_g2p_max_table_mib()); \
    FS2_CHECK_ARG(W >= 0 && Lgmax >= 0 && Lgmax <= G2P_MAX_LG && Lpmax >= 0 && Lpmax <= G2P_MAX_LP,                                 \
                  name ": bad shape W=%d Lgmax=%d (<= %d) Lpmax=%d (<= %d)", W, Lgmax, G2P_MAX_LG, Lpmax, G2P_MAX_LP);              \
    FS2_CHECK_ARG(ldl >= Lgmax && ldp >= Lpmax, name ": bad id strides %ld %ld", ldl, ldp)

extern "C" int fs2_g2p_m2m_expect(const int32_t* letters, long ldl, const int32_t* phones, long ldp, const int32_t* glens,
                                  const int32_t* plens, const double* logtheta, long n_table, int A, int P, double* loglik, double* post,
                                  long ldo_w, long ldo_i, int W, int Lgmax, int Lpmax, hipStream_t stream) {
    FS2_CHECK_ARG(letters && phones && glens && plens && logtheta && loglik && post, "g2p_m2m_expect: null pointer");
    G2P_LATTICE_ARGS("g2p_m2m_expect");
    FS2_CHECK_ARG(ldo_i >= 4l * (Lpmax + 1) && ldo_w >= (long)Lgmax * ldo_i, "g2p_m2m_expect: bad strides post %ld %ld", ldo_w, ldo_i);
    if (W == 0) return FS2_OK;
    g2p_expect_kernel<<<fs2_cdiv(W, G2P_WPB), G2P_NT, 0, stream>>>(letters, ldl, phones, ldp, glens, plens, logtheta, A, P, loglik, post,
                                                                  ldo_w, ldo_i, W, Lgmax, Lpmax);
    FS2_CHECK_LAUNCH("g2p_m2m_expect");
    return FS2_OK;
}

extern "C" int fs2_g2p_m2m_viterbi(const int32_t* letters, long ldl, const int32_t* phones, long ldp, const int32_t* glens,
                                   const int32_t* plens, const double* logtheta, long n_table, int A, int P, double* score, uint8_t* bp,
                                   long ldb_w, long ldb_i, int W, int Lgmax, int Lpmax, hipStream_t stream) {
    FS2_CHECK_ARG(letters && phones && glens && plens && logtheta && score && bp, "g2p_m2m_viterbi: null pointer");
    G2P_LATTICE_ARGS("g2p_m2m_viterbi");
    FS2_CHECK_ARG(ldb_i >= Lpmax + 1 && ldb_w >= (long)(Lgmax + 1) * ldb_i, "g2p_m2m_viterbi: bad strides bp %ld %ld", ldb_w, ldb_i);
    if (W == 0) return FS2_OK;
    g2p_viterbi_kernel<<<fs2_cdiv(W, G2P_WPB), G2P_NT, 0, stream>>>(letters, ldl, phones, ldp, glens, plens, logtheta, A, P, score, bp,
                                                                   ldb_w, ldb_i, W, Lgmax, Lpmax);
    FS2_CHECK_LAUNCH("g2p_m2m_viterbi");
    return FS2_OK;
}

// ------------------------------------------------------------------ the n-gram
// Order n holds the entries [offs[n - 1], offs[n]) of keys / logp / bow, keys ascending; a key packs n ids of 16 bits, the oldest in
// the highest place.  hist packs the last three ids of a history the same way (the newest in bits 0..15).
struct G2pLm {
    const uint64_t* keys;
    const double* logp;
    const double* bow;
    const int32_t* offs;
    int n_keys, N;
};
static __device__ __forceinline__ int g2p_find(const G2pLm& lm, int n, uint64_t key) {
    int lo = min(max(lm.offs[n - 1], 0), lm.n_keys);
    const int end = min(max(lm.offs[n], lo), lm.n_keys);
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lm.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < end && lm.keys[lo] == key) ? lo : -1;
}
// found at order n: its log-probability; else the back-off weight of the order's history (0 when that history is unseen) plus the
// score under the history without its oldest id.  The weights are added from the longest history down, the log-probability last.
static __device__ double g2p_lm_score(const G2pLm& lm, uint64_t hist, uint32_t tok) {
    double acc = 0.0;
    for (int n = lm.N; n >= 1; --n) {
        const uint64_t ctx = n > 1 ? hist & ((1ull << (16 * (n - 1))) - 1) : 0;
        const int idx = g2p_find(lm, n, (ctx << 16) | tok);
        if (idx >= 0) return acc + lm.logp[idx];
        if (n == 1) break;
        const int h = g2p_find(lm, n - 1, ctx);
        if (h >= 0) acc += lm.bow[h];
    }
    return g2p_ninf();
}

__global__ void __launch_bounds__(G2P_NT) g2p_ngram_score_kernel(const int32_t* __restrict__ hist, long ldh, const int32_t* __restrict__ tok,
                                                                 G2pLm lm, double* __restrict__ out, int n) {
    const int q = blockIdx.x * G2P_NT + threadIdx.x;
    if (q >= n) return;
    uint64_t h = 0;
    bool ok = (unsigned)tok[q] < 65536u;
    for (int k = 0; k < lm.N - 1; ++k) {                                   // oldest first
        const int id = hist[(size_t)q * ldh + k];
        ok = ok && (unsigned)id < 65536u;
        h = (h << 16) | (uint64_t)(id & 0xffff);
    }
    out[q] = ok ? g2p_lm_score(lm, h, (uint32_t)tok[q]) : g2p_ninf();
}

#define G2P_LM_ARGS(name)                                                                                                  \
    FS2_CHECK_ARG(keys && logp && bow && order_offs, name ": null model pointer");                                         \
    FS2_CHECK_ARG(N >= 1 && N <= G2P_MAX_ORDER && n_keys >= 0, name ": order %d (1..%d), %d keys", N, G2P_MAX_ORDER, n_keys)

extern "C" int fs2_g2p_ngram_score(const int32_t* hist, long ldh, const int32_t* tok, const uint64_t* keys, const double* logp,
                                   const double* bow, const int32_t* order_offs, int n_keys, int N, double* out, int n,
                                   hipStream_t stream) {
    FS2_CHECK_ARG(hist && tok && out, "g2p_ngram_score: null pointer");
    G2P_LM_ARGS("g2p_ngram_score");
    FS2_CHECK_ARG(n >= 0 && ldh >= N - 1, "g2p_ngram_score: bad shape n=%d ldh=%ld", n, ldh);
    if (n == 0) return FS2_OK;
    const G2pLm lm = {keys, logp, bow, order_offs, n_keys, N};
    g2p_ngram_score_kernel<<<fs2_cdiv(n, G2P_NT), G2P_NT, 0, stream>>>(hist, ldh, tok, lm, out, n);
    FS2_CHECK_LAUNCH("g2p_ngram_score");
    return FS2_OK;
}

// ------------------------------------------------------------------ decoding
// (value, index) arg-max over the workgroup by a fixed tree: the larger value, on ties the lower index.  The result is in rs[0], ri[0].
static __device__ __forceinline__ void g2p_argmax(double v, int e, double* rs, int* ri, int tid) {
    rs[tid] = v;
    ri[tid] = e;
    __syncthreads();
    for (int o = G2P_NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double v2 = rs[tid + o];
            const int e2 = ri[tid + o];
            if (v2 > rs[tid] || (v2 == rs[tid] && e2 < ri[tid])) {
                rs[tid] = v2;
                ri[tid] = e2;
            }
        }
        __syncthreads();
    }
}

struct G2pRow { int beg, n; };
// the types that spell chunk c, cut at the stated fan-out and at the list's end
static __device__ __forceinline__ G2pRow g2p_row(const int32_t* __restrict__ offs, int c, int n_spell, int fan) {
    G2pRow r = {0, 0};
    if (c < 0) return r;
    r.beg = min(max(offs[c], 0), n_spell);
    r.n = min(min(max(offs[c + 1] - r.beg, 0), fan), n_spell - r.beg);
    return r;
}

// Hypothesis k of position i is slot (i K + k) of the word's beam rows: its score, its last three ids (hist, BOS-padded) and
// bp = 2 (parent slot) + (letters consumed - 1).  Candidate e of position i: e < n(i-1) f1 is parent e / f1 at i - 1 with the
// (e % f1)-th type that spells letters[i-1:i]; the rest are parents at i - 2 with the types that spell letters[i-2:i], in the same way.
__global__ void __launch_bounds__(G2P_NT) g2p_decode_kernel(const int32_t* __restrict__ letters, long ldl, const int32_t* __restrict__ glens,
                                                            int A, const int32_t* __restrict__ spell_offs,
                                                            const int32_t* __restrict__ spell_types, int n_spell, int fan1, int fan2,
                                                            const int32_t* __restrict__ type_phones, int T, G2pLm lm, int K,
                                                            double* __restrict__ beam_score, uint64_t* __restrict__ beam_hist,
                                                            int32_t* __restrict__ beam_bp, int32_t* __restrict__ beam_n,
                                                            double* __restrict__ cand_all, long ldc, int32_t* __restrict__ out_phones,
                                                            long ldo, int32_t* __restrict__ out_n, double* __restrict__ out_score,
                                                            int Lgmax) {
    __shared__ double rs[G2P_NT];
    __shared__ int ri[G2P_NT];
    __shared__ int toks[G2P_MAX_LG];
    const int w = blockIdx.x, tid = threadIdx.x, Lg = g2p_len(glens, w, Lgmax);
    const double NINF = g2p_ninf();
    const int32_t* lw = letters + (size_t)w * ldl;
    double* bs = beam_score + (size_t)w * (Lgmax + 1) * K;
    uint64_t* bh = beam_hist + (size_t)w * (Lgmax + 1) * K;
    int32_t* bb = beam_bp + (size_t)w * (Lgmax + 1) * K;
    int32_t* bn = beam_n + (size_t)w * (Lgmax + 1);
    double* cand = cand_all + (size_t)w * ldc;
    const uint64_t bos = (uint64_t)T;
    if (tid == 0) {
        bs[0] = 0.0;
        bh[0] = bos | (bos << 16) | (bos << 32);
        bb[0] = -1;
        bn[0] = 1;
    }
    __syncthreads();
    for (int i = 1; i <= Lg; ++i) {
        const int a1 = lw[i - 1], a0 = i >= 2 ? lw[i - 2] : -1;
        const bool v1 = (unsigned)a1 < (unsigned)A, v0 = (unsigned)a0 < (unsigned)A;
        const G2pRow r1 = g2p_row(spell_offs, v1 ? a1 : -1, n_spell, fan1);
        const G2pRow r2 = g2p_row(spell_offs, v1 && v0 ? A + a0 * A + a1 : -1, n_spell, fan2);
        const int np1 = min(max(bn[i - 1], 0), K), np2 = i >= 2 ? min(max(bn[i - 2], 0), K) : 0;
        const int C1 = np1 * r1.n, C = C1 + np2 * r2.n;
        for (int e = tid; e < C; e += G2P_NT) {
            const bool first = e < C1;
            const int ee = first ? e : e - C1, f = first ? r1.n : r2.n;
            const int k = ee / f, slot = (first ? i - 1 : i - 2) * K + k;
            const int tok = spell_types[(first ? r1.beg : r2.beg) + (ee - k * f)];
            cand[e] = (unsigned)tok < (unsigned)T ? bs[slot] + g2p_lm_score(lm, bh[slot], (uint32_t)tok) : NINF;
        }
        __syncthreads();
        int kept = 0;
        for (int r = 0; r < K; ++r) {
            double bv = NINF;
            int be = 0x7fffffff;
            for (int e = tid; e < C; e += G2P_NT) {
                const double v = cand[e];
                if (v > bv) { bv = v; be = e; }
            }
            g2p_argmax(bv, be, rs, ri, tid);
            if (rs[0] == NINF) break;                                      // the same answer in every lane
            if (tid == 0) {
                const int e = ri[0];
                const bool first = e < C1;
                const int ee = first ? e : e - C1, f = first ? r1.n : r2.n;
                const int k = ee / f, slot = (first ? i - 1 : i - 2) * K + k;
                const int tok = spell_types[(first ? r1.beg : r2.beg) + (ee - k * f)];
                bs[i * K + r] = rs[0];
                bh[i * K + r] = ((bh[slot] << 16) | (uint64_t)tok) & 0xffffffffffffull;
                bb[i * K + r] = 2 * k + (first ? 0 : 1);
                cand[e] = NINF;
            }
            ++kept;
            __syncthreads();
        }
        if (tid == 0) bn[i] = kept;
        __syncthreads();
    }
    // the end of the word: + log P(</s> | history), the best (the lower slot on ties), the walk back
    const int nl = Lg >= 1 ? min(max(bn[Lg], 0), K) : 0;
    double bv = NINF;
    int be = 0x7fffffff;
    for (int k = tid; k < nl; k += G2P_NT) {
        const double v = bs[Lg * K + k] + g2p_lm_score(lm, bh[Lg * K + k], (uint32_t)T + 1);
        if (v > bv) { bv = v; be = k; }
    }
    g2p_argmax(bv, be, rs, ri, tid);
    if (tid != 0) return;
    if (rs[0] == NINF) {
        out_n[w] = -1;
        out_score[w] = NINF;
        return;
    }
    int pos = Lg, slot = ri[0], m = 0;
    while (pos > 0 && m < G2P_MAX_LG) {
        toks[m++] = (int)(bh[pos * K + slot] & 0xffff);
        const int b = bb[pos * K + slot];
        pos -= (b & 1) + 1;
        slot = min(max(b >> 1, 0), K - 1);
    }
    int n = 0;
    int32_t* o = out_phones + (size_t)w * ldo;
    for (int q = m - 1; q >= 0; --q)
        for (int z = 0; z < 2; ++z) {
            const int p = (unsigned)toks[q] < (unsigned)T ? type_phones[2 * toks[q] + z] : -1;
            if (p >= 0 && n < ldo) o[n++] = p;
        }
    out_n[w] = n;
    out_score[w] = rs[0];
}

extern "C" int fs2_g2p_decode(const int32_t* letters, long ldl, const int32_t* glens, int A, const int32_t* spell_offs,
                              const int32_t* spell_types, int n_spell, int max_fan1, int max_fan2, const int32_t* type_phones, int T,
                              const uint64_t* keys, const double* logp, const double* bow, const int32_t* order_offs, int n_keys, int N,
                              int K, double* beam_score, uint64_t* beam_hist, int32_t* beam_bp, int32_t* beam_n, double* cand, long ldc,
                              int32_t* out_phones, long ldo, int32_t* out_n, double* out_score, int W, int Lgmax, hipStream_t stream) {
    FS2_CHECK_ARG(letters && glens && spell_offs && spell_types && type_phones && beam_score && beam_hist && beam_bp && beam_n && cand &&
                      out_phones && out_n && out_score,
                  "g2p_decode: null pointer");
    G2P_LM_ARGS("g2p_decode");
    FS2_CHECK_ARG(A >= 1 && A <= G2P_MAX_LETTERS && T >= 1 && T < 65534, "g2p_decode: %d letters (1..%d), %d graphone types (1..65533)", A,
                  G2P_MAX_LETTERS, T);
    FS2_CHECK_ARG(K >= 1 && K <= G2P_MAX_BEAM, "g2p_decode: beam %d outside 1..%d", K, G2P_MAX_BEAM);
    FS2_CHECK_ARG(W >= 0 && Lgmax >= 0 && Lgmax <= G2P_MAX_LG && ldl >= Lgmax && ldo >= 2l * Lgmax,
                  "g2p_decode: bad shape W=%d Lgmax=%d (<= %d) ldl=%ld ldo=%ld", W, Lgmax, G2P_MAX_LG, ldl, ldo);
    FS2_CHECK_ARG(n_spell >= 0 && max_fan1 >= 0 && max_fan2 >= 0 && (long)K * ((long)max_fan1 + max_fan2) < (1l << 31) &&
                      ldc >= (long)K * ((long)max_fan1 + max_fan2),
                  "g2p_decode: candidate row of %ld for K=%d and fan-outs %d + %d", ldc, K, max_fan1, max_fan2);
    if (W == 0) return FS2_OK;
    const G2pLm lm = {keys, logp, bow, order_offs, n_keys, N};
    g2p_decode_kernel<<<W, G2P_NT, 0, stream>>>(letters, ldl, glens, A, spell_offs, spell_types, n_spell, max_fan1, max_fan2, type_phones,
                                               T, lm, K, beam_score, beam_hist, beam_bp, beam_n, cand, ldc, out_phones, ldo, out_n,
                                               out_score, Lgmax);
    FS2_CHECK_LAUNCH("g2p_decode");
    return FS2_OK;
}
