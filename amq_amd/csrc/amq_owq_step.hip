// amq_owq_step.hip -- the few-row stage of OWQ layers in the token step (DESIGN.md 3.12 "In the runner", include/amq_hip.h amq_owq_stage_f16): ONE
// launch in front of the unchanged packed GEMVs of a sibling set (q/k/v, o, gate/up, down).  For 1 .. 8 rows of x and the activation
//   a = x | gamma * fp16(x * rstd) (rmsnorm_kernel) | fp16(silu(x)) * x2 (silu_mul_kernel)
// it leaves, per part (one sibling linear): xg = a[:, perm] (0 where perm < 0: owq_gather_kernel) and y = fp16(acc) or fp16(fp32(residual) + acc),
// acc the fmaf chain over j ascending of fp32(a[r, out_ids[j]]) * fp32(W_out[n, j]) from 0 (owq_outlier_add_kernel) -- the packed GEMV then adds its
// product through its residual epilogue.  A part without outliers only gets a itself in xg.
//
//   grid   per part, in order: ceil(Kp / 512) gather workgroups (a thread owns two columns of xg for all rows: perm is read once), then -- with
//          outliers -- ceil(N / 256) workgroups that own 256 outputs n for all rows, the rows' outlier activations in LDS in tiles of OWQ_ADD_J
//          (every lane reads the same address: a broadcast), so a weight is read once per launch.
//   a      is formed where it is read, element by element, straight from global x (<= 16 KiB a row: L2).  With RMSNorm every workgroup takes the
//          rows' statistic itself, in rmsnorm_kernel's order: thread t adds the squares of chunks t, t + 256, .. of 8, element by element; the wave's
//          64 sums meet in the xor 32, 16, .. 1 butterfly; rstd = rsqrt(((w0 + w1) + w2) + w3) / K + eps).
// Every operation is its own rounding (-ffp-contract=off).  No atomics, no host read, no allocation: the same bits on every run, capturable.
#include "amq_quant.cuh"

namespace amq {

struct OwqStagePart {
    const int* perm;            // [Kp], nullptr for a part without outliers (identity over K)
    const int* out_ids;         // [n_out]
    const _Float16* W_out;      // [N, n_out]
    _Float16* xg;               // [R, Kp]
    _Float16* y;                // [R, N]
    const _Float16* residual;   // [R, N] or nullptr; may be y
    int N, n_out, Kp;
    int wg_gather, wg_out;      // workgroups of the part's two kinds
};
struct OwqStageArgs {
    const _Float16* x;
    const _Float16* x2;
    const _Float16* gamma;
    float eps;
    int R, K, n_parts;
    OwqStagePart part[OWQ_STAGE_PARTS];
};

enum { STAGE_NONE = 0, STAGE_RMSNORM = 1, STAGE_SILU_MUL = 2 };

// a[r, c]: the expressions of rmsnorm_kernel / silu_mul_kernel on one element
template <int ACT>
__device__ __forceinline__ _Float16 owq_stage_act(const _Float16* x, const _Float16* x2, const _Float16* gamma, const float* rstd, int K, int r, int c) {
    const _Float16 v = x[(size_t)r * K + c];
    if (ACT == STAGE_RMSNORM) {
        const _Float16 n = (_Float16)((float)v * rstd[r]);
        return gamma[c] * n;
    }
    if (ACT == STAGE_SILU_MUL) {
        const float gf = (float)v;
        const _Float16 sg = (_Float16)(gf / (1.0f + __expf(-gf)));
        return sg * x2[(size_t)r * K + c];
    }
    return v;
}

template <int ACT>
__global__ __launch_bounds__(256) void owq_stage_kernel(const OwqStageArgs a) {
    constexpr int RMAX = OWQ_STAGE_ROWS, J = OWQ_ADD_J;
    __shared__ float red[RMAX][4];
    __shared__ float rstd[RMAX];
    __shared__ float xs[J][RMAX];
    const int tid = threadIdx.x, R = a.R, K = a.K;
    const _Float16* x = a.x;
    const _Float16* x2 = a.x2;
    const _Float16* gamma = a.gamma;

    // which part, which kind, which chunk (workgroup-uniform; the parts' fields are picked by unrolled selects, never by a runtime index)
    const int* perm = nullptr;
    const int* out_ids = nullptr;
    const _Float16* W_out = nullptr;
    _Float16* xg = nullptr;
    _Float16* y = nullptr;
    const _Float16* res = nullptr;
    int N = 0, n_out = 0, Kp = 0, chunk = 0;
    bool gather = false, found = false;
    int wg = blockIdx.x;
#pragma unroll
    for (int i = 0; i < OWQ_STAGE_PARTS; ++i) {
        const OwqStagePart& p = a.part[i];
        const int total = i < a.n_parts ? p.wg_gather + p.wg_out : 0;
        if (!found && wg < total) {
            found = true;
            gather = wg < p.wg_gather;
            chunk = gather ? wg : wg - p.wg_gather;
            perm = p.perm;
            out_ids = p.out_ids;
            W_out = p.W_out;
            xg = p.xg;
            y = p.y;
            res = p.residual;
            N = p.N;
            n_out = p.n_out;
            Kp = p.Kp;
        }
        if (!found) wg -= total;
    }
    if (!found) return;

    if (ACT == STAGE_RMSNORM) {
        for (int r = 0; r < R; ++r) {
            const _Float16* xr = x + (size_t)r * K;
            float ss = 0.f;
            for (int c = tid; c < (K >> 3); c += 256) {
                const h8 v = *(const h8*)(xr + 8 * c);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float f = (float)v[i];
                    ss += f * f;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
            if ((tid & 63) == 0) red[r][tid >> 6] = ss;
        }
        __syncthreads();
        if (tid < R) rstd[tid] = rsqrtf((red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3]) / (float)K + a.eps);
        __syncthreads();
    }

    if (gather) {
        const int c = 2 * (chunk * 256 + tid);
        if (c >= Kp) return;
        const int p0 = perm ? perm[c] : c, p1 = perm ? perm[c + 1] : c + 1;
        const bool in0 = p0 >= 0 && p0 < K, in1 = p1 >= 0 && p1 < K;
        for (int r = 0; r < R; ++r) {
            h2 v;
            v.x = in0 ? owq_stage_act<ACT>(x, x2, gamma, rstd, K, r, p0) : (_Float16)0.0f;
            v.y = in1 ? owq_stage_act<ACT>(x, x2, gamma, rstd, K, r, p1) : (_Float16)0.0f;
            *(h2*)(xg + (size_t)r * Kp + c) = v;
        }
        return;
    }

    // 256 outputs of the part: owq_outlier_add_kernel's scheme over a
    const int n = chunk * 256 + tid;
    const _Float16* wr = W_out + (size_t)(n < N ? n : 0) * n_out;
    float acc[RMAX];
#pragma unroll
    for (int t = 0; t < RMAX; ++t) acc[t] = 0.0f;
    for (int j0 = 0; j0 < n_out; j0 += J) {
        const int nj = n_out - j0 < J ? n_out - j0 : J;
        __syncthreads();        // the previous tile has been used
        for (int e = tid; e < J * RMAX; e += 256) {
            const int jj = e / RMAX, t = e % RMAX;
            float v = 0.0f;
            if (jj < nj && t < R) {
                const int p = out_ids[j0 + jj];
                if (p >= 0 && p < K) v = (float)owq_stage_act<ACT>(x, x2, gamma, rstd, K, t, p);
            }
            xs[jj][t] = v;
        }
        __syncthreads();
        if (n < N)
            for (int jj = 0; jj < nj; ++jj) {
                const float w = (float)wr[j0 + jj];
#pragma unroll
                for (int t = 0; t < RMAX; ++t) acc[t] = fmaf(xs[jj][t], w, acc[t]);
            }
    }
    if (n < N)
#pragma unroll
        for (int t = 0; t < RMAX; ++t)
            if (t < R) {
                const size_t at = (size_t)t * N + n;
                y[at] = res ? (_Float16)((float)res[at] + acc[t]) : (_Float16)acc[t];
            }
}

hipError_t launch_owq_stage(const void* x, int R, int K, int act, const void* gamma, float eps, const void* x2, const OwqStageLaunchPart* parts,
                            int n_parts, hipStream_t st) {
    OwqStageArgs a = {};
    a.x = (const _Float16*)x;
    a.x2 = (const _Float16*)x2;
    a.gamma = (const _Float16*)gamma;
    a.eps = eps;
    a.R = R;
    a.K = K;
    a.n_parts = n_parts;
    unsigned wgs = 0;
    for (int i = 0; i < n_parts; ++i) {
        OwqStagePart& p = a.part[i];
        const OwqStageLaunchPart& s = parts[i];
        const bool plain = s.n_out == 0;
        p.perm = plain ? nullptr : (const int*)s.perm;
        p.out_ids = (const int*)s.out_ids;
        p.W_out = (const _Float16*)s.W_out;
        p.xg = (_Float16*)s.xg;
        p.y = (_Float16*)s.y;
        p.residual = (const _Float16*)s.residual;
        p.N = plain ? 0 : s.N;
        p.n_out = s.n_out;
        p.Kp = plain ? K : s.Kp;
        p.wg_gather = (p.Kp + 511) / 512;
        p.wg_out = plain ? 0 : (s.N + 255) / 256;
        wgs += (unsigned)(p.wg_gather + p.wg_out);
    }
    if (act == STAGE_RMSNORM)
        hipLaunchKernelGGL(owq_stage_kernel<STAGE_RMSNORM>, dim3(wgs), dim3(256), 0, st, a);
    else if (act == STAGE_SILU_MUL)
        hipLaunchKernelGGL(owq_stage_kernel<STAGE_SILU_MUL>, dim3(wgs), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(owq_stage_kernel<STAGE_NONE>, dim3(wgs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace amq
