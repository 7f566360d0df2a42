// fs2_comp.h - the compensated fp64 sums of the scoring kernels (fs2_hnr.hip, fs2_cwt.hip, fs2_modspec.hip, fs2_msfilter.hip): a sum
// is a pair (s, e) whose second word carries the rounding errors (the two-sum of Knuth for the additions, an fma for the error of
// each product), so that s + e is the sum of the exactly evaluated terms rounded once, except in cases too rare to meet.  Terms go
// in per lane in the caller's order and the lanes' pairs are added by a fixed tree: the same input gives the same bytes.
//
// Every function switches contraction off in its own body: a fused a * b + c would drop the error that the second word is there to
// keep.  The including file's floating-point mode is left as it was.
#pragma once
#include "fs2_common.h"

// (s, e) += p, the rounding error of the addition into e
static __device__ __forceinline__ void cs_add(double& s, double& e, double p) {
#pragma clang fp contract(off)
    const double t = s + p, bb = t - s;
    e += (s - (t - bb)) + (p - bb);
    s = t;
}

// (s, e) += a b, the product taken exactly
static __device__ __forceinline__ void cs_fma(double& s, double& e, double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    e += __builtin_fma(a, b, -p);
    cs_add(s, e, p);
}

// The sum of the NT lanes' (s, e) by a fixed tree, the same on every run.  Every lane gets it; rs / re [NT] may be reused after
// the call.
template <int NT>
static __device__ __forceinline__ double cs_block_sum(double s, double e, double* rs, double* re, int tid) {
#pragma clang fp contract(off)
    rs[tid] = s;
    re[tid] = e;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
            double a = rs[tid], b = re[tid];
            cs_add(a, b, rs[tid + o]);
            b += re[tid + o];
            rs[tid] = a;
            re[tid] = b;
        }
        __syncthreads();
    }
    const double r = rs[0] + re[0];
    __syncthreads();
    return r;
}
