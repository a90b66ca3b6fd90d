// amq_sample_body.cuh -- the sampler of ONE row of fp16 logits by ONE workgroup of SMP_THREADS threads: the device code sample_kernel
// (amq_sample.hip) and decode_tail_lookup_sample_kernel (amq_lookup.hip) share.  What it computes and why every step is integer work is written
// at the top of amq_sample.hip.
#pragma once
#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

typedef unsigned long long u64;
typedef unsigned short us8 __attribute__((ext_vector_type(8)));

constexpr int SMP_THREADS = 1024;
constexpr int SMP_BINS = 4096;                 // upper 12 bits of the key
constexpr float SMP_FIX = 1099511627776.0f;    // 2^40: fixed-point scale of a weight in (0, 1]

__device__ __forceinline__ unsigned smp_key(unsigned b) {
    if ((b & 0x7fffu) > 0x7c00u) return 0;                     // NaN: not a candidate
    if (b == 0x8000u) b = 0;                                   // -0 == +0: one tie class
    if (b == 0x7c00u) b = 0x7bffu;                             // +inf counts as the largest finite value (keeps the weights finite)
    const unsigned k = (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
    return k <= 0x03ffu ? 0 : k;                               // -inf (key 0x03ff): probability 0, never kept
}

__device__ __forceinline__ float smp_val(unsigned k) {
    const unsigned short b = (unsigned short)((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xffffu));
    return (float)__builtin_bit_cast(_Float16, b);
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// sum of v over the threads with a HIGHER index (reverse = true) or a LOWER index (reverse = false); *total = the sum over all threads
__device__ __forceinline__ u64 smp_block_scan_excl(u64 v, bool reverse, u64* swave, u64* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    u64 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = reverse ? (u64)__shfl_down((long long)incl, off) : (u64)__shfl_up((long long)incl, off);
        if (reverse ? lane + off < 64 : lane >= off) incl += o;
    }
    if (lane == (reverse ? 0 : 63)) swave[w] = incl;
    __syncthreads();
    u64 other = 0, all = 0;
#pragma unroll
    for (int ww = 0; ww < SMP_THREADS / 64; ++ww) {
        const u64 s = swave[ww];
        all += s;
        if (reverse ? ww > w : ww < w) other += s;
    }
    __syncthreads();                                           // swave is reused by the next scan
    *total = all;
    return other + incl - v;
}

// Row `row` of a.logits [rows, a.vocab] -> *s_tok (a word of the caller's LDS), valid for every thread of the workgroup when the call returns (it
// ends in a barrier).  A: SampleArgs, or anything with its members logits, vocab, suppress, state, u_in, kept (taken by reference so that a kernel
// argument is read where it is used).  The generator's counter words of this row are (the state block's draw counter + draw_add as one 64-bit
// number, seq).  Every thread of the workgroup must call it.
template <class A>
__device__ __forceinline__ void smp_sample_row(const A& a, int row, unsigned draw_add, unsigned seq, unsigned* s_tok) {
    __shared__ u64 m12[SMP_BINS];                              // fixed-point mass per 12-bit key prefix
    __shared__ unsigned c12[SMP_BINS];                         // candidates per 12-bit key prefix
    __shared__ u64 m16[16];
    __shared__ unsigned c16[16];
    __shared__ u64 swave[SMP_THREADS / 64];
    __shared__ unsigned smaxw[SMP_THREADS / 64];
    __shared__ unsigned s_bin, s_key;
    __shared__ u64 s_above;

    const int tid = threadIdx.x, V = a.vocab;
    const unsigned short* lg = (const unsigned short*)a.logits + (size_t)row * V;
    const bool aligned = ((uintptr_t)lg & 15) == 0;
    const int nch = (V + 7) >> 3;                              // groups of 8 logits

    const int* st = a.state;
    const float temperature = __int_as_float(st[SMP_TEMPERATURE]);
    const int top_k = st[SMP_TOP_K];
    const float top_p = __int_as_float(st[SMP_TOP_P]);
    const unsigned seed0 = (unsigned)st[SMP_SEED], seed1 = (unsigned)st[SMP_SEED + 1];
    unsigned draw0 = (unsigned)st[SMP_DRAW], draw1 = (unsigned)st[SMP_DRAW + 1];
    if (draw_add != 0u) {                                      // (a 64-bit add: the carry goes into the second word)
        const u64 d = (((u64)draw1 << 32) | draw0) + draw_add;
        draw0 = (unsigned)d;
        draw1 = (unsigned)(d >> 32);
    }

    int sup[8], supc[8];
    bool anysup = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sup[j] = a.suppress ? a.suppress[j] : -1;
        supc[j] = sup[j] >> 3;                                 // (-1 stays -1: no group has that index)
        anysup = anysup || sup[j] >= 0;
    }

    // keys of logits 8c .. 8c + 7 (0 past the end of the row and for suppressed ids)
    auto get_keys = [&](int c, unsigned (&k)[8]) {
        const int i0 = 8 * c;
        if (aligned && i0 + 8 <= V) {
            const us8 v = *(const us8*)(lg + i0);
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = smp_key(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = i0 + e < V ? smp_key(lg[i0 + e]) : 0;
        }
        if (anysup) {
            bool hit = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) hit = hit || supc[j] == c;
            if (hit) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (i0 + e == sup[j]) k[e] = 0;
            }
        }
    };

    // ---- the largest key
    unsigned mk = 0;
    for (int c = tid; c < nch; c += SMP_THREADS) {
        unsigned k[8];
        get_keys(c, k);
#pragma unroll
        for (int e = 0; e < 8; ++e) mk = k[e] > mk ? k[e] : mk;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)mk, off);
        mk = o > mk ? o : mk;
    }
    if ((tid & 63) == 0) smaxw[tid >> 6] = mk;
    for (int b = tid; b < SMP_BINS; b += SMP_THREADS) { m12[b] = 0; c12[b] = 0; }
    __syncthreads();
    unsigned maxkey = 0;
#pragma unroll
    for (int w = 0; w < SMP_THREADS / 64; ++w) maxkey = smaxw[w] > maxkey ? smaxw[w] : maxkey;

    if (maxkey == 0) {                                         // no candidate at all (every logit NaN / -inf / suppressed): token 0, like the greedy tail
        if (tid == 0) *s_tok = 0;
        if (a.kept)
            for (int i = tid; i < V; i += SMP_THREADS) a.kept[(size_t)row * V + i] = 0;
        __syncthreads();
    } else {
        const float vmax = smp_val(maxkey);
        const float inv_t = 1.0f / temperature;
        auto wfix = [&](unsigned k) -> u64 { return (u64)(expf((smp_val(k) - vmax) * inv_t) * SMP_FIX); };

        // candidates and mass of the keys with 12-bit prefix `bin`, by their lower 4 bits -> c16 / m16
        auto low_hist = [&](unsigned bin) {
            if (tid < 16) { c16[tid] = 0; m16[tid] = 0; }
            __syncthreads();
            for (int c = tid; c < nch; c += SMP_THREADS) {
                unsigned k[8];
                get_keys(c, k);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k[e] != 0 && (k[e] >> 4) == bin) {
                        atomicAdd(&c16[k[e] & 15], 1u);
                        atomicAdd(&m16[k[e] & 15], wfix(k[e]));
                    }
            }
            __syncthreads();
        };

        // ---- histogram of candidates and mass over the 12-bit prefixes
        for (int c = tid; c < nch; c += SMP_THREADS) {
            unsigned k[8];
            get_keys(c, k);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (k[e] != 0) {
                    atomicAdd(&c12[k[e] >> 4], 1u);
                    atomicAdd(&m12[k[e] >> 4], wfix(k[e]));
                }
        }
        __syncthreads();

        // ---- top-k: kth = key of the k-th largest logit (ties with it are kept: key >= kth)
        unsigned kth = 1;
        if (top_k > 0) {
            const u64 k = (u64)top_k;
            u64 ct = 0, total;
#pragma unroll
            for (int j = 0; j < 4; ++j) ct += c12[4 * tid + j];
            const u64 above = smp_block_scan_excl(ct, true, swave, &total);
            if (k < total) {                                   // (k >= the number of candidates: nothing to cut)
                if (above < k && k <= above + ct) {            // exactly one thread: its four bins hold the k-th largest
                    u64 r = above;
                    for (int b = 4 * tid + 3; b >= 4 * tid; --b) {
                        if (r + c12[b] >= k) { s_bin = (unsigned)b; s_above = r; break; }
                        r += c12[b];
                    }
                }
                __syncthreads();
                const unsigned bk = s_bin;
                low_hist(bk);
                if (tid == 0) {
                    u64 r = s_above;
                    int j = 15;
                    for (; j > 0; --j) {
                        if (r + c16[j] >= k) break;
                        r += c16[j];
                    }
                    s_key = (bk << 4) | (unsigned)j;
                    u64 pm = 0;
                    for (int jj = j; jj < 16; ++jj) pm += m16[jj];
                    m12[bk] = pm;                              // what top-k leaves of this prefix
                }
                __syncthreads();
                kth = s_key;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned)(4 * tid + j) < bk) m12[4 * tid + j] = 0;     // (own bins: read back by this thread only)
            }
        }

        // ---- top-p over what top-k left: keep a token iff the mass of the strictly larger keys < top_p * total
        unsigned thr = kth;
        if (top_p < 1.0f) {
            u64 mt = 0, Z;
#pragma unroll
            for (int j = 0; j < 4; ++j) mt += m12[4 * tid + j];
            const u64 above = smp_block_scan_excl(mt, true, swave, &Z);
            const double pz = (double)top_p * (double)Z;
            if ((double)above < pz && (double)(above + mt) >= pz) {             // exactly one thread: the threshold is in its four bins
                u64 r = above;
                for (int b = 4 * tid + 3; b >= 4 * tid; --b) {
                    if ((double)r < pz && c12[b] != 0 && m12[b] != 0) { s_bin = (unsigned)b; s_above = r; }
                    r += m12[b];
                }
            }
            __syncthreads();
            const unsigned bs = s_bin;
            low_hist(bs);
            if (tid == 0) {
                u64 r = s_above;
                unsigned vp = kth;
                for (int j = 15; j >= 0; --j) {
                    const unsigned key = (bs << 4) | (unsigned)j;
                    if (key < kth) break;
                    if (c16[j] != 0) {
                        if ((double)r < pz) vp = key;
                        r += m16[j];
                    }
                }
                s_key = vp > kth ? vp : kth;
            }
            __syncthreads();
            thr = s_key;
        }

        // ---- the draw, in ascending token index: thread t owns tokens [t * per, (t + 1) * per)
        const int cpt = (((V + SMP_THREADS - 1) / SMP_THREADS) + 7) >> 3;      // groups of 8 per thread
        const int c_lo = tid * cpt;
        u64 mt = 0;
        for (int c = c_lo; c < c_lo + cpt && c < nch; ++c) {
            unsigned k[8];
            get_keys(c, k);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool keep = k[e] >= thr && k[e] != 0;
                if (keep) mt += wfix(k[e]);
                if (a.kept && 8 * c + e < V) a.kept[(size_t)row * V + 8 * c + e] = keep ? 1 : 0;
            }
        }
        u64 K;
        const u64 before = smp_block_scan_excl(mt, false, swave, &K);
        float u;
        if (st[SMP_FIRST_KEPT] != 0) {
            u = 0.0f;
        } else if (a.u_in) {
            u = a.u_in[row];
        } else {
            unsigned r4[4];
            philox4x32_10(draw0, draw1, seq, 0u, seed0, seed1, r4);
            u = (float)(r4[0] >> 8) * 5.9604644775390625e-8f;                  // 2^-24
        }
        u = u >= 0.0f ? u : 0.0f;
        u64 target = (u64)((double)u * (double)K);
        if (target >= K) target = K - 1;                                       // (K >= 2^40: the largest logit weighs exactly 1)
        if (before <= target && target < before + mt) {                       // exactly one thread
            u64 cum = before;
            bool found = false;
            for (int c = c_lo; c < c_lo + cpt && c < nch && !found; ++c) {
                unsigned k[8];
                get_keys(c, k);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (!found && k[e] >= thr && k[e] != 0) {
                        cum += wfix(k[e]);
                        if (cum > target) { *s_tok = (unsigned)(8 * c + e); found = true; }
                    }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace amq
