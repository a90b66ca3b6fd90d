// amq_quantize.hip -- fp16 W[N,K] -> HQQ Format A (W_q, scale, zero): Quantizer.quantize with its proximal solver
// (hqq/core/quantize.py:76-180, hqq/core/optimize.py:96-108, 201-255) in the fp32 arithmetic of the reference's CPU path.
//
// Three launches, no host read, no atomics:
//   hqq_solve_kernel<G>   one 64-lane wave owns a group (two groups of 32): W is read ONCE into registers and all 20 iterations run there.  The
//                         stop decision needs the error of the WHOLE tensor, so no wave can stop: every iteration leaves its zero in Z[i][group]
//                         and its sum of |W - W_r| in the wave's accumulator -- the trace that lets one pass over W replace twenty.
//   hqq_stop_kernel       one workgroup: adds the workgroups' partial errors per iteration in index order, walks the stop rule, writes the info
//                         block {int32 stop, int32 nonfinite, float mean_err[20]}.
//   hqq_emit_kernel<BITS> one thread per Format A word (amq_quant.cuh format_a_store): re-forms the codes from W, s and Z[stop] and packs them.
// Every operation is its own fp32 rounding (-ffp-contract=off, IEEE division); sums are fixed trees, so a layer quantizes to the
// same bits on every run.  tests/hqq_solver_ref.py restates the whole of it in torch.
#include "amq_quant.cuh"

namespace amq {

template <bool HALVES>
__device__ __forceinline__ float group_sum(float v, int lane) { return HALVES ? half_sum_dpp(v, lane) : wave_sum_dpp(v); }
template <bool HALVES>
__device__ __forceinline__ float group_max(float v, int lane) { return HALVES ? half_max_dpp(v, lane) : wave_max_dpp(v); }

// sum of a lane's V values as the low levels of the group's tree
template <int V>
__device__ __forceinline__ float lane_tree(const float (&x)[V]) {
    if constexpr (V == 1) return x[0];
    else if constexpr (V == 2) return x[0] + x[1];
    else return (x[0] + x[1]) + (x[2] + x[3]);
}

template <int G>
__global__ __launch_bounds__(64 * HQQ_WAVES) void hqq_solve_kernel(const _Float16* __restrict__ W, size_t P, size_t R, int T, float maxv, int round_zero,
                                                                   float* __restrict__ S, float* __restrict__ Z, float* __restrict__ Epart,
                                                                   int* __restrict__ NF) {
    constexpr int V = G >= 64 ? G / 64 : 1;          // values per lane: the lane's are consecutive, so lane tree + DPP tree = one tree over the index
    constexpr bool HALVES = G == 32;
    __shared__ float accE[HQQ_WAVES][HQQ_ITERS];
    __shared__ int accBad[HQQ_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < HQQ_ITERS) accE[wave][lane] = 0.0f;
    bool bad = false;
    const size_t pass0 = ((size_t)blockIdx.x * HQQ_WAVES + wave) * (size_t)T;
    for (int t = 0; t < T; ++t) {
        const size_t pass = pass0 + t;
        if (pass >= P) break;                        // (wave-uniform)
        float w[V];
        const _Float16* src = W + (pass * 64 + lane) * V;
        if constexpr (V == 1) w[0] = (float)src[0];
        else if constexpr (V == 2) { const h2 v = *(const h2*)src; w[0] = (float)v.x; w[1] = (float)v.y; }
        else { const h4 v = *(const h4*)src; w[0] = (float)v.x; w[1] = (float)v.y; w[2] = (float)v.z; w[3] = (float)v.w; }
        float mx = w[0], mn = w[0];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            bad = bad || !finite(w[v]);
            mx = fmaxf(mx, w[v]);
            mn = fminf(mn, w[v]);
        }
        mx = group_max<HALVES>(mx, lane);
        mn = -group_max<HALVES>(-mn, lane);
        const float den = mx - mn;
        float s = (1.0f / den) * maxv;               // the reference's `max_v / tensor` is torch's reciprocal() * max_v: two roundings, kept
        if (fabsf(den) <= 1e-4f) s = 1.0f;
        s = fminf(s, 2e4f);
        float z = (-mn) * s;
        if (round_zero) z = rintf(z);
        const size_t group = HALVES ? 2 * pass + (lane >> 5) : pass;
        const bool writer = HALVES ? (lane & 31) == 0 : lane == 0;
        if (writer) S[group] = s;
        for (int i = 0; i < HQQ_ITERS; ++i) {
            float a[V], u[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float q = fminf(fmaxf(rintf(w[v] * s + z), 0.0f), maxv);
                const float r = (q - z) / s;
                const float e = w[v] - r;
                a[v] = fabsf(e);
                const float sgn = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
                const float sh = fmaxf(a[v] - 0.1f * powf(a[v], -0.3f), 0.0f) * sgn;      // a = 0: 0 - inf clamps to 0
                u[v] = q - (w[v] - sh) * s;
            }
            const float ea = wave_sum_dpp(lane_tree<V>(a));                  // the whole pass (both groups of 32)
            z = group_sum<HALVES>(lane_tree<V>(u), lane) / (float)G;
            if (writer) Z[(size_t)i * R + group] = z;
            if (lane == 0) accE[wave][i] += ea;
        }
    }
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if (lane == 0) accBad[wave] = anybad ? 1 : 0;
    __syncthreads();
    if (threadIdx.x < HQQ_ITERS) {
        float e = 0.0f;
#pragma unroll
        for (int k = 0; k < HQQ_WAVES; ++k) e += accE[k][threadIdx.x];
        Epart[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = e;
    }
    if (threadIdx.x == 0) {
        int b = 0;
#pragma unroll
        for (int k = 0; k < HQQ_WAVES; ++k) b |= accBad[k];
        NF[blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(256) void hqq_stop_kernel(const float* __restrict__ Epart, const int* __restrict__ NF, int wgs, float count,
                                                       int* __restrict__ info) {
    __shared__ float buf[256][HQQ_ITERS + 1];
    __shared__ int sbad[256];
    __shared__ float mean[HQQ_ITERS];
    const int tid = threadIdx.x;
    float run = 0.0f;
    int bad = 0;
    for (int base = 0; base < wgs; base += 256) {
        const int w = base + tid;
#pragma unroll
        for (int i = 0; i < HQQ_ITERS; ++i) buf[tid][i] = w < wgs ? Epart[(size_t)i * wgs + w] : 0.0f;
        if (w < wgs) bad |= NF[w];
        __syncthreads();
        if (tid < HQQ_ITERS) {
            const int n = wgs - base < 256 ? wgs - base : 256;
            for (int j = 0; j < n; ++j) run += buf[j][tid];
        }
        __syncthreads();
    }
    sbad[tid] = bad;
    if (tid < HQQ_ITERS) mean[tid] = run / count;
    __syncthreads();
    if (tid == 0) {
        // first i with not (mean_i < best), best the running minimum from +inf (optimize.py:236-247); the last iteration if none
        float best = __builtin_inff();
        int stop = HQQ_ITERS - 1;
        for (int i = 0; i < HQQ_ITERS; ++i) {
            if (mean[i] < best) best = mean[i];
            else { stop = i; break; }
        }
        int any = 0;
        for (int j = 0; j < 256; ++j) any |= sbad[j];
        info[0] = stop;
        info[1] = any;
    }
    if (tid < HQQ_ITERS) ((float*)info)[2 + tid] = mean[tid];
}

template <int BITS>
__global__ __launch_bounds__(256) void hqq_emit_kernel(const _Float16* __restrict__ W, const float* __restrict__ S, const float* __restrict__ Z,
                                                       const int* __restrict__ info, size_t R, int G, void* __restrict__ Wq,
                                                       _Float16* __restrict__ scale, _Float16* __restrict__ zero) {
    constexpr float maxv = (float)((1 << BITS) - 1);
    int stop = info[0];
    stop = stop < 0 ? 0 : (stop >= HQQ_ITERS ? HQQ_ITERS - 1 : stop);
    const float* Zs = Z + (size_t)stop * R;
    format_a_store<BITS>(Wq, R, G, [&](size_t r, int col) {
        const float s = S[r], z = Zs[r];
        const float w = (float)W[r * G + col];
        if (col == 0) {
            scale[r] = (_Float16)(1.0f / s);
            zero[r] = (_Float16)z;
        }
        return fminf(fmaxf(rintf(w * s + z), 0.0f), maxv);
    });
}

hipError_t launch_hqq_quantize(const void* W, int N, int K, int bits, int group, int round_zero, void* W_q, void* scale, void* zero,
                               void* info, void* workspace, hipStream_t st) {
    const HqqGeom g = hqq_geometry(N, K, group);
    float* S = (float*)workspace;
    float* Z = S + g.R;
    float* Epart = Z + (size_t)HQQ_ITERS * g.R;
    int* NF = (int*)(Epart + (size_t)HQQ_ITERS * g.wgs);
    const float maxv = (float)((1 << bits) - 1);
    if (hipError_t e = dispatch<32, 64, 128, 256>(group, [&](auto G) {
            hipLaunchKernelGGL((hqq_solve_kernel<G()>), dim3(g.wgs), dim3(64 * HQQ_WAVES), 0, st, (const _Float16*)W, g.P, g.R, g.T, maxv, round_zero, S, Z,
                               Epart, NF);
            return hipGetLastError();
        }))
        return e;
    hipLaunchKernelGGL(hqq_stop_kernel, dim3(1), dim3(256), 0, st, Epart, NF, g.wgs, (float)((size_t)N * K), (int*)info);
    if (hipError_t e = hipGetLastError()) return e;
    return dispatch_bits(bits, [&](auto B) {
        hipLaunchKernelGGL((hqq_emit_kernel<B()>), dim3(format_a_blocks(g.R, group, bits)), dim3(256), 0, st, (const _Float16*)W, S, Z, (const int*)info,
                           g.R, group, W_q, (_Float16*)scale, (_Float16*)zero);
        return hipGetLastError();
    });
}

}  // namespace amq
