// amq_owq.hip -- OWQ (include/amq_hip.h): a few input columns per linear stay fp16 and absorb the error feedback of the quantized
// ones, and every 128-column group of the rest takes its range from a search over num x 2^bits (delta, zero-point) candidates under an lp-2.4 loss.
//
//   owq_range_kernel<BITS>   one workgroup (4 waves) per row: the segment W[n, col0 .. col0 + L) is staged ONCE in LDS as fp16 (2 L bytes: 22 KiB at
//                            K = 11008, 56 KiB at 28672; L <= OWQ_RANGE_MAX_L keeps two workgroups of the longest row on a CU); per delta candidate
//                            one pass over LDS forms r = rint(v / d16) once and adds the element's term to all 2^bits zero-point sums in registers.
//   owq_colerr_kernel<BITS>  one thread per column: frob_c = the sum over the rows, ascending, of (w - w^)^2 for the rows' chosen (scale, zero).
//   owq_range_flag_kernel    one workgroup: a row without a winner (a non-finite value in it) sets the info word.
//   solve_kernel<SOLVE_OWQ, 128, BITS> (amq_solve_body.cuh, which also holds the candidate arithmetic the range search here shares): the group's
//                            (d16, zp) from the candidate search over the lane's 8 registers + a 16-lane butterfly per candidate; the columns
//                            >= n_nonout are never quantized: they only receive the updates and leave as fp16 W_out.
//   quant_flag_kernel, quant_pack_kernel<BITS> (amq_quant_pack.hip) end the solve.
//   owq_gather_kernel, owq_outlier_add_kernel   the deployment side of HIPOWQLinear: xg = x[:, perm], and y += x[:, out_ids] . W_out^T.
// Every operation is its own fp32 rounding (-ffp-contract=off, IEEE division, rintf) except the score's |d|^2.4 = v_exp_f32(2.4f * v_log_f32(|d|)),
// the one place whose bits a host restatement may miss; the sums' orders are stated at their loops.  No host read, no allocation, no atomics.
#include "amq_solve_body.cuh"

namespace amq {

// ---------------------------------------------------------------------------------------------------------------- the range search of row segments
template <int BITS>
__global__ __launch_bounds__(64 * OWQ_RANGE_WAVES) void owq_range_kernel(const _Float16* __restrict__ W, int K, int col0, int L, int num,
                                                                         _Float16* __restrict__ scale, _Float16* __restrict__ zero,
                                                                         int* __restrict__ choice, float* __restrict__ score) {
    constexpr int NZ = 1 << BITS, THREADS = 64 * OWQ_RANGE_WAVES;
    constexpr float maxq = (float)(NZ - 1);
    extern __shared__ _Float16 seg[];                               // the row's segment, L values
    __shared__ float red[OWQ_RANGE_WAVES][NZ];
    __shared__ float ext[OWQ_RANGE_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    const _Float16* src = W + row * (size_t)K + col0;
    float mn = 0.0f, mx = 0.0f;                                     // (0 is in the range by the rule: xmin = min(min v, 0), xmax = max(max v, 0))
    for (int c = tid; c < L; c += THREADS) {
        const _Float16 h = src[c];
        seg[c] = h;
        const float v = (float)h;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        if (!finite(v)) {                                           // fminf / fmaxf drop a NaN: a non-finite value makes the range infinite,
            mn = -__builtin_inff();                                 // every score NaN or inf, and the row ends without a winner (flagged)
            mx = __builtin_inff();
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        mn = fminf(mn, __shfl_xor(mn, m));
        mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    if (lane == 0) {
        ext[wave][0] = mn;
        ext[wave][1] = mx;
    }
    __syncthreads();
    float xmin = ext[0][0], xmax = ext[0][1];
#pragma unroll
    for (int w = 1; w < OWQ_RANGE_WAVES; ++w) {
        xmin = fminf(xmin, ext[w][0]);
        xmax = fmaxf(xmax, ext[w][1]);
    }
    const float xrange = xmax - xmin, numf = (float)num, Lf = (float)L;
    float best = 1e10f, bd = 0.0f;
    int bi = 0, bz = 0;
#pragma unroll 1
    for (int i = 1; i <= num; ++i) {
        const float d16 = owq_step(xrange, numf, i, maxq);
        // the sum's order: thread t adds its elements c = t, t + 256, ... in ascending c from 0; the wave's 64 sums meet in a butterfly (xor 1, 2,
        // 4, 8, 16, 32: s = s + the partner's s); the workgroup's four are (w0 + w1) + (w2 + w3); the score is that sum / L
        float acc[NZ];
#pragma unroll
        for (int z = 0; z < NZ; ++z) acc[z] = 0.0f;
        for (int c = tid; c < L; c += THREADS) {
            const float v = (float)seg[c];
            const float r = rintf(v / d16);
#pragma unroll
            for (int z = 0; z < NZ; ++z) acc[z] = acc[z] + owq_pow24(fabsf(v - owq_what<BITS>(r, (float)z, d16)));
        }
#pragma unroll
        for (int z = 0; z < NZ; ++z) {
            float s = acc[z];
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);
            if (lane == 0) red[wave][z] = s;
        }
        __syncthreads();
#pragma unroll
        for (int z = 0; z < NZ; ++z) {
            const float s = (red[0][z] + red[1][z]) + (red[2][z] + red[3][z]);
            const float sc = s / Lf;
            if (sc < best) {
                best = sc;
                bd = d16;
                bi = i;
                bz = z;
            }
        }
        __syncthreads();        // red is rewritten by the next candidate
    }
    if (tid == 0) {
        scale[row] = (_Float16)bd;
        zero[row] = (_Float16)(float)bz;
        choice[2 * row] = bi;
        choice[2 * row + 1] = bz;
        score[row] = best;
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void owq_colerr_kernel(const _Float16* __restrict__ W, int N, int K, const _Float16* __restrict__ scale,
                                                         const _Float16* __restrict__ zero, float* __restrict__ wq_err) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    float acc = 0.0f;
    for (int n = 0; n < N; ++n) {                                   // rows ascending, one chain per column
        const float s = (float)scale[n], z = (float)zero[n];
        const float v = (float)W[(size_t)n * K + c];
        const float d = v - owq_what<BITS>(rintf(v / s), z, s);
        acc = acc + d * d;
    }
    wq_err[c] = acc;
}

__global__ __launch_bounds__(256) void owq_range_flag_kernel(const int* __restrict__ choice, int N, int* __restrict__ info) {
    __shared__ int sbad[256];
    int bad = 0;
    for (int n = threadIdx.x; n < N; n += 256) bad |= choice[2 * n] == 0;
    sbad[threadIdx.x] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any = 0;
        for (int j = 0; j < 256; ++j) any |= sbad[j];
        info[0] = any != 0;
    }
}

hipError_t launch_owq_range(const void* W, int N, int K, int col0, int L, int bits, int num, void* scale, void* zero, void* choice, void* score,
                            void* wq_err, void* info, hipStream_t st) {
    if (hipError_t e = dispatch_bits(bits, [&](auto B) {
            hipLaunchKernelGGL((owq_range_kernel<B()>), dim3(N), dim3(64 * OWQ_RANGE_WAVES), (size_t)L * sizeof(_Float16), st, (const _Float16*)W, K,
                               col0, L, num, (_Float16*)scale, (_Float16*)zero, (int*)choice, (float*)score);
            if (hipError_t e2 = hipGetLastError()) return e2;
            if (wq_err)
                hipLaunchKernelGGL((owq_colerr_kernel<B()>), dim3((K + 255) / 256), dim3(256), 0, st, (const _Float16*)W, N, K,
                                   (const _Float16*)scale, (const _Float16*)zero, (float*)wq_err);
            return hipGetLastError();
        }))
        return e;
    hipLaunchKernelGGL(owq_range_flag_kernel, dim3(1), dim3(256), 0, st, (const int*)choice, N, (int*)info);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- the solve
hipError_t launch_owq_quantize(const void* W, const void* U, int N, int K, int n_out, int bits, int num, void* W_q, void* scale, void* zero,
                               void* W_out, void* choice, void* row_loss, void* info, void* workspace, hipStream_t st) {
    const int nq = K - n_out, Kp = owq_packed_columns(K, n_out);
    return launch_solve(workspace, N, Kp, GPTQ_BLOCK, bits, W_q, info, st, [&](float* E, int* NF, uint8_t* Q) {
        return dispatch_bits(bits, [&](auto B) {
            hipLaunchKernelGGL((solve_kernel<SOLVE_OWQ, GPTQ_BLOCK, B()>), dim3(gptq_workgroups(N)), dim3(64 * GPTQ_WAVES), 0, st, (const _Float16*)W,
                               (const float*)U, K, E, Q, (_Float16*)scale, (_Float16*)zero, (float*)row_loss, NF, (const int*)nullptr, nq, Kp, num,
                               (_Float16*)W_out, (int*)choice);
            return hipGetLastError();
        });
    });
}

// ---------------------------------------------------------------------------------------------------------------- the layer's two own launches
// xg[m, c] = x[m, perm[c]], 0 where perm[c] is not a column of x (the padding: its weight is 0, and 0 must not meet an inf); two columns per thread
__global__ __launch_bounds__(256) void owq_gather_kernel(const _Float16* __restrict__ x, int M, int K, const int* __restrict__ perm, int Kp,
                                                         _Float16* __restrict__ xg) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, half = (size_t)(Kp / 2);
    if (gid >= (size_t)M * half) return;
    const size_t m = gid / half;
    const int c = 2 * (int)(gid % half);
    const int p0 = perm[c], p1 = perm[c + 1];
    h2 v;
    v.x = (p0 >= 0 && p0 < K) ? x[m * (size_t)K + p0] : (_Float16)0.0f;
    v.y = (p1 >= 0 && p1 < K) ? x[m * (size_t)K + p1] : (_Float16)0.0f;
    *(h2*)(xg + m * (size_t)Kp + c) = v;
}

// y[m, n] = fp16(fp32(y[m, n]) + acc), acc = the fmaf chain over j ascending of fp32(x[m, out_ids[j]]) * fp32(W_out[n, j]) from 0.  A thread owns one
// output column n and OWQ_ADD_ROWS rows of x, so that a weight is read once for 16 rows; the rows' outlier activations go through LDS in tiles of
// OWQ_ADD_J columns (every lane reads the same address: a broadcast).  Each (m, n) keeps its own chain in ascending j whatever the tiling.
__global__ __launch_bounds__(256) void owq_outlier_add_kernel(const _Float16* __restrict__ x, int M, int K, const int* __restrict__ out_ids,
                                                              int n_out, const _Float16* __restrict__ Wout, _Float16* __restrict__ y, int N) {
    constexpr int R = OWQ_ADD_ROWS, J = OWQ_ADD_J;
    __shared__ float xs[J][R];
    const int n = blockIdx.x * 256 + threadIdx.x;
    const size_t m0 = (size_t)blockIdx.y * R;
    const int rows = (size_t)M - m0 < (size_t)R ? (int)((size_t)M - m0) : R;
    const _Float16* wr = Wout + (size_t)(n < N ? n : 0) * n_out;
    float acc[R];
#pragma unroll
    for (int t = 0; t < R; ++t) acc[t] = 0.0f;
    for (int j0 = 0; j0 < n_out; j0 += J) {
        const int nj = n_out - j0 < J ? n_out - j0 : J;
        __syncthreads();        // the previous tile has been used
        for (int e = threadIdx.x; e < J * R; e += 256) {
            const int jj = e / R, t = e % R;
            float v = 0.0f;
            if (jj < nj && t < rows) {
                const int p = out_ids[j0 + jj];
                if (p >= 0 && p < K) v = (float)x[(m0 + t) * (size_t)K + p];
            }
            xs[jj][t] = v;
        }
        __syncthreads();
        if (n < N)
            for (int jj = 0; jj < nj; ++jj) {
                const float w = (float)wr[j0 + jj];
#pragma unroll
                for (int t = 0; t < R; ++t) acc[t] = fmaf(xs[jj][t], w, acc[t]);
            }
    }
    if (n < N)
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < rows) {
                _Float16* at = y + (m0 + t) * (size_t)N + n;
                *at = (_Float16)((float)*at + acc[t]);
            }
}

hipError_t launch_owq_gather(const void* x, int M, int K, const void* perm, int Kp, void* xg, hipStream_t st) {
    const size_t threads = (size_t)M * (Kp / 2);
    hipLaunchKernelGGL(owq_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const _Float16*)x, M, K, (const int*)perm, Kp,
                       (_Float16*)xg);
    return hipGetLastError();
}

hipError_t launch_owq_outlier_add(const void* x, int M, int K, const void* out_ids, int n_out, const void* W_out, void* y, int N, hipStream_t st) {
    hipLaunchKernelGGL(owq_outlier_add_kernel, dim3((N + 255) / 256, (M + OWQ_ADD_ROWS - 1) / OWQ_ADD_ROWS), dim3(256), 0, st, (const _Float16*)x, M, K, (const int*)out_ids, n_out,
                       (const _Float16*)W_out, (_Float16*)y, N);
    return hipGetLastError();
}

}  // namespace amq
