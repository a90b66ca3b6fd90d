// amq_eval.hip -- the two evaluation metrics of the deployed model as row reductions over fp16 logits: per-row negative log-likelihood
// (+ log-sum-exp and arg-max) and per-row Jensen-Shannon divergence against a second (dense) model's logits.  What the reference's search loop
// computes with a dozen framework passes over an fp32 copy of [S, vocab] (amq/utils/eval.py, amq/utils/loss.py) is here one launch over the
// fp16 rows as the lm_head wrote them.
//
// One workgroup of 512 threads per row.  A row is walked in LOGICAL chunks of 8 values, chunk c = values 8c .. 8c + 7 of the row whatever its
// address; thread t owns chunks t, t + 512, ...  The summation order is fixed by that map alone:
//   * a thread keeps one partial sum per slot of a chunk (8 of them, each a serial sum over the thread's chunks in ascending order) and folds
//     them as one binary tree;
//   * the 64 threads of a wave are folded by DPP inside the four 16-lane rows and four lane reads, ((r0 + r1) + (r2 + r3));
//   * the 8 wave sums go through LDS and are added in wave order by every thread.
// No atomics, nothing depends on the row's index, its neighbours or its alignment: a row has the same bits launched alone or among others.
//
// Loads: a chunk of a 16-byte aligned row is one 16-byte load (two for fp32 values).  A row that is not (odd vocabularies: rows 2 bytes aligned)
// is read through the ALIGNED 16-byte vectors that cover the chunk, shifted into place; the chunks whose covering vectors would reach outside the
// row -- the first one and the last one or two -- are read value by value, guarded by the row's length.  Rows are read two (NLL) or three
// (JSD) times; the later passes of a row come from L2 (a 152064-wide row pair is 608 KB).  Plain loads, the compiler's own waits.
#include <limits.h>

#include "amq_common.cuh"
#include "amq_kernels.h"

namespace amq {

constexpr int EV_THREADS = 512;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr float EV_NEG_INF = -__builtin_huge_valf();

__device__ __forceinline__ float ev_dpp(float v, int ctrl) {
    switch (ctrl) {      // (the control word of a DPP move is an immediate)
        case 0: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
        case 1: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
        case 2: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));   // row_half_mirror
        default: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));  // row_mirror
    }
}
__device__ __forceinline__ float ev_lane(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }

// whole-wave maximum / integer minimum, the shape of wave_sum_dpp (amq_common.cuh): every lane gets the result
__device__ __forceinline__ float ev_wave_max(float v) {
#pragma unroll
    for (int s = 0; s < 4; ++s) v = fmaxf(v, ev_dpp(v, s));
    return fmaxf(fmaxf(ev_lane(v, 0), ev_lane(v, 16)), fmaxf(ev_lane(v, 32), ev_lane(v, 48)));
}
__device__ __forceinline__ int ev_wave_min(int v) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int o = __builtin_bit_cast(int, ev_dpp(__builtin_bit_cast(float, v), s));
        v = o < v ? o : v;
    }
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

__device__ __forceinline__ float ev_tree8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

// sum over the workgroup, the same bits in every thread: DPP wave sums, then the waves in order.  s: EV_WAVES floats of LDS (reused call to call)
__device__ __forceinline__ float ev_block_sum(float v, float* s) {
    v = wave_sum_dpp(v);
    __syncthreads();                                           // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) t += s[w];
    return t;
}
__device__ __forceinline__ float ev_block_max(float v, float* s) {
    v = ev_wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = EV_NEG_INF;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) t = fmaxf(t, s[w]);
    return t;
}

__device__ __forceinline__ float ev_value(const uint32_t* o, int e, _Float16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)((e & 1) ? o[e >> 1] >> 16 : o[e >> 1] & 0xffffu));
}
__device__ __forceinline__ float ev_value(const uint32_t* o, int e, float) { return __builtin_bit_cast(float, o[e]); }

// o = d shifted down by Q dwords and, with `half`, two more bytes (the register indices are compile-time: nothing is indexed in memory)
template <int Q, int NW>
__device__ __forceinline__ void ev_shift(const uint32_t (&d)[NW + 4], bool half, uint32_t (&o)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) o[j] = half ? (d[j + Q] >> 16) | (d[j + Q + 1] << 16) : d[j + Q];
}

// one row of V values of type T (_Float16 or float) at any alignment of its type
template <typename T>
struct EvRow {
    static constexpr int NW = (int)sizeof(T) * 2;              // dwords of a chunk of 8 values
    const T* p;
    int V;
    int b0;                                                    // bytes from the 16-byte boundary below the row to the row: uniform over the workgroup

    __device__ __forceinline__ EvRow(const T* p_, int V_) : p(p_), V(V_), b0((int)((uintptr_t)p_ & 15)) {}
    __device__ __forceinline__ int chunks() const { return (V + 7) >> 3; }

    // values 8c .. 8c + 7 as fp32; -inf past the end of the row
    __device__ __forceinline__ void load(int c, float (&v)[8]) const {
        const int i0 = 8 * c;
        const long long first = (long long)i0 * (long long)sizeof(T) - b0;                 // byte offset (from the row) of the first covering vector
        const long long row_bytes = (long long)V * (long long)sizeof(T);
        const bool vec = b0 == 0 ? i0 + 8 <= V : (c > 0 && first + NW * 4 + 16 <= row_bytes);
        if (vec) {
            const u4* a = (const u4*)((const char*)p + first);
            uint32_t o[NW];
            if (b0 == 0) {
#pragma unroll
                for (int k = 0; k < NW / 4; ++k) {
                    const u4 t = a[k];
                    o[4 * k] = t.x; o[4 * k + 1] = t.y; o[4 * k + 2] = t.z; o[4 * k + 3] = t.w;
                }
            } else {
                uint32_t d[NW + 4];
#pragma unroll
                for (int k = 0; k < NW / 4 + 1; ++k) {
                    const u4 t = a[k];
                    d[4 * k] = t.x; d[4 * k + 1] = t.y; d[4 * k + 2] = t.z; d[4 * k + 3] = t.w;
                }
                const bool half = (b0 & 2) != 0;
                switch (b0 >> 2) {                             // whole dwords to skip (0 .. 3), then 0 or 2 bytes; a uniform branch
                    case 0: ev_shift<0, NW>(d, half, o); break;
                    case 1: ev_shift<1, NW>(d, half, o); break;
                    case 2: ev_shift<2, NW>(d, half, o); break;
                    default: ev_shift<3, NW>(d, half, o); break;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = ev_value(o, e, T());
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = i0 + e < V ? (float)p[i0 + e] : EV_NEG_INF;
        }
    }
};

// max of the row and sum of exp(value - max): the two passes both kernels start with.  *amax (when asked for): index of the first maximum.
template <typename T>
__device__ __forceinline__ void ev_max_sumexp(const EvRow<T>& r, float* sred, int* sidx, float* mx_out, float* sum_out, int* amax) {
    const int tid = threadIdx.x, nch = r.chunks();
    float best = EV_NEG_INF;
    int bi = INT_MAX;
    for (int c = tid; c < nch; c += EV_THREADS) {
        float v[8];
        r.load(c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (v[e] > best) { best = v[e]; bi = 8 * c + e; }  // ascending index, strict: a thread's first maximum
    }
    float mx;
    if (amax) {
        const float wm = ev_wave_max(best);
        const int wi = ev_wave_min(best == wm ? bi : INT_MAX);
        __syncthreads();
        if ((tid & 63) == 0) { sred[tid >> 6] = wm; sidx[tid >> 6] = wi; }
        __syncthreads();
        mx = EV_NEG_INF;
        int ai = INT_MAX;
#pragma unroll
        for (int w = 0; w < EV_WAVES; ++w) {
            const float m = sred[w];
            const int i = sidx[w];
            if (m > mx || (m == mx && i < ai)) { mx = m; ai = i; }
        }
        *amax = ai;
    } else {
        mx = ev_block_max(best, sred);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < nch; c += EV_THREADS) {
        float v[8];
        r.load(c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += expf(v[e] - mx);                             // (past the row: exp(-inf) = +0)
    }
    *mx_out = mx;
    *sum_out = ev_block_sum(ev_tree8(acc), sred);
}

__global__ __launch_bounds__(EV_THREADS) void logit_nll_kernel(const _Float16* logits, long long row_stride, const long long* labels, int V,
                                                               float* nll_out, float* lse_out, int* argmax_out) {
    __shared__ float sred[EV_WAVES];
    __shared__ int sidx[EV_WAVES];
    const size_t row = blockIdx.x;
    const EvRow<_Float16> r(logits + row * (size_t)row_stride, V);
    float mx, sum;
    int am;
    ev_max_sumexp(r, sred, sidx, &mx, &sum, &am);
    if (threadIdx.x == 0) {
        const float lse = mx + logf(sum);
        const long long label = labels ? labels[row] : -100;
        float nll = 0.f;                                       // -100: HF's ignore_index, the caller counts the row out
        if (label != -100) nll = (label >= 0 && label < (long long)V) ? lse - (float)r.p[label] : __builtin_nanf("");
        nll_out[row] = nll;
        if (lse_out) lse_out[row] = lse;
        if (argmax_out) argmax_out[row] = am;
    }
}

// row = 0.5 * sum_v [ e^lp (lp - m) + e^lq (lq - m) ],  lp = p - lse_p, lq = q - lse_q,  m = log(max(0.5 (e^lp + e^lq), eps)): the reference's
// JSD (KLDivLoss with log_target, the mixture clamped at eps before its log) on fp32 values.
// lp and m are both about -log V, each known to half an fp32 ulp THERE (5e-7 at 16): formed as written, lp - m carries that error into every
// term.  Where the mixture is not clamped the two differences are functions of d = lq - lp = (q - p) - (lse_q - lse_p) alone,
//     lp - m = -log(0.5 (1 + e^d)),     lq - m = d - log(0.5 (1 + e^d)),
// and d is small and exact to a few 1e-8 (q - p is exact in fp32): with g0 = log(0.5 + 0.5 e^-|d|) <= 0 they are (-d - g0, -g0) for d >= 0 and
// (-g0, d - g0) for d < 0.  A clamped entry (weights under 2 eps) keeps lp - log(eps), lq - log(eps).  The same function, evaluated where fp32
// can hold it: the kernel stays inside four fp32 ulp of log 2 of the fp64 value.
template <typename QT>
__global__ __launch_bounds__(EV_THREADS) void logit_jsd_kernel(const _Float16* p, long long p_stride, const QT* q, long long q_stride, int V, float eps,
                                                               float* jsd_out) {
    __shared__ float sred[EV_WAVES];
    const size_t row = blockIdx.x;
    const EvRow<_Float16> rp(p + row * (size_t)p_stride, V);
    const EvRow<QT> rq(q + row * (size_t)q_stride, V);
    float mp, sp, mq, sq;
    ev_max_sumexp(rp, sred, nullptr, &mp, &sp, nullptr);
    ev_max_sumexp(rq, sred, nullptr, &mq, &sq, nullptr);
    // lse = max + log(sum) is never rounded as one number: (value - max) is exact in fp32 for fp16 values, so lp = (p - mp) - log(sp) and
    // d = ((q - p) - (mq - mp)) - (log(sq) - log(sp)) keep their accuracy whatever the magnitude of the logits
    const float ls_p = logf(sp), ls_q = logf(sq);
    const float dmax = mq - mp, dls = ls_q - ls_p, log_eps = logf(eps);      // (eps = 0: nothing is clamped, log_eps is not used)
    const int tid = threadIdx.x, nch = rp.chunks();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < nch; c += EV_THREADS) {
        float vp[8], vq[8];
        rp.load(c, vp);
        rq.load(c, vq);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (8 * c + e < V) {
                const float lp = (vp[e] - mp) - ls_p, lq = (vq[e] - mq) - ls_q;
                const float ep = expf(lp), eq = expf(lq);
                float tp, tq;                                  // lp - m, lq - m
                if (0.5f * (ep + eq) >= eps) {
                    const float d = ((vq[e] - vp[e]) - dmax) - dls;
                    const float g0 = logf(0.5f + 0.5f * expf(-fabsf(d)));
                    tp = d >= 0.f ? -d - g0 : -g0;
                    tq = d >= 0.f ? -g0 : d - g0;
                } else {
                    tp = lp - log_eps;
                    tq = lq - log_eps;
                }
                acc[e] += ep * tp + eq * tq;
            }
        }
    }
    const float total = ev_block_sum(ev_tree8(acc), sred);
    if (tid == 0) jsd_out[row] = 0.5f * total;
}

hipError_t launch_logit_nll(const void* logits, long long row_stride, const void* labels, int M, int V, float* nll_out, float* lse_out,
                            int* argmax_out, hipStream_t st) {
    hipLaunchKernelGGL(logit_nll_kernel, dim3(M), dim3(EV_THREADS), 0, st, (const _Float16*)logits, row_stride, (const long long*)labels, V,
                       nll_out, lse_out, argmax_out);
    return hipGetLastError();
}

hipError_t launch_logit_jsd(const void* p, long long p_stride, const void* q, long long q_stride, bool q_is_f32, int M, int V, float eps,
                            float* jsd_out, hipStream_t st) {
    if (q_is_f32)
        hipLaunchKernelGGL(logit_jsd_kernel<float>, dim3(M), dim3(EV_THREADS), 0, st, (const _Float16*)p, p_stride, (const float*)q, q_stride, V, eps, jsd_out);
    else
        hipLaunchKernelGGL(logit_jsd_kernel<_Float16>, dim3(M), dim3(EV_THREADS), 0, st, (const _Float16*)p, p_stride, (const _Float16*)q, q_stride, V, eps, jsd_out);
    return hipGetLastError();
}

}  // namespace amq
