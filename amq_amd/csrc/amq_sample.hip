// amq_sample.hip -- temperature / top-k / top-p sampling and EOS stop: the second tail of a token step (the greedy one is decode_tail_kernel,
// amq_decode.hip), and the same device code over any number of logits rows (first token after a prompt pass, tests).
//
// One workgroup of 1024 threads per row of fp16 logits.  Everything that decides WHICH tokens are kept and WHICH one is drawn is integer work:
//   * an fp16 logit maps to an ordered 16-bit key (larger logit = larger key; -0 = +0; NaN, -inf and suppressed ids = key 0 = "not a candidate"),
//     so the top-k threshold is an exact radix select: a 4096-bin histogram of the keys' upper 12 bits, then 16 bins of the lower 4 bits;
//   * a token's weight exp((logit - max) / temperature) is rounded ONCE to 2^-40 fixed point (<= 2^40; 2^18 of them sum below 2^58), and every
//     sum of weights is a 64-bit integer sum: the result does not depend on the order the adds happen in (LDS integer atomics included), so the
//     same inputs give the same kept set and the same token on every run, in a captured graph or not.  The top-p threshold is a key as well
//     (the same two-level walk over per-bin masses), so whole tie classes are kept or dropped together;
//   * the draw walks the kept tokens in ascending token index: thread t owns a contiguous slice of the vocabulary, an exclusive prefix sum over
//     the threads' kept masses finds the slice, the owning thread finds the token.
// The uniform number is Philox4x32-10 of (seed; draw counter, sequence index): a pure function of the three.
// The sampler of one row is smp_sample_row (amq_sample_body.cuh): this kernel and the sampled lookup tail (amq_lookup.hip) call the one copy.
#include "amq_sample_body.cuh"

namespace amq {

// SEQ (amq_decode_tail_sample_seq_f16): a.pos / a.rope_cur are those of block 0 of an array of step-state blocks STEP_STRIDE bytes apart; every row's
// workgroup advances ITS block's position and writes ITS cos/sin row.  Draws and EOS bookkeeping are the same.  The !SEQ instantiation is the
// shared-position kernel as it was.
template <bool SEQ>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(SampleArgs a) {
    __shared__ unsigned s_tok;
    __shared__ int spos;

    const int tid = threadIdx.x, row = blockIdx.x, V = a.vocab;
    int* st = a.state;
    const unsigned draw0 = (unsigned)st[SMP_DRAW], draw1 = (unsigned)st[SMP_DRAW + 1];
    smp_sample_row(a, row, 0u, (unsigned)(a.seq0 + row), &s_tok);

    // ---- EOS bookkeeping, the token, the shared state words
    if (tid == 0) {
        int tok = (int)s_tok;
        if ((a.flags & SMP_FLAG_EOS) && row < 8) {
            if (__hip_atomic_load(&st[SMP_FINISHED + row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                tok = st[SMP_PAD_ID];                                          // a finished sequence emits the pad id and stays finished
            } else {
                bool is_eos = false;
#pragma unroll
                for (int j = 0; j < 8; ++j) is_eos = is_eos || tok == st[SMP_EOS + j];      // (unused slots hold -1)
                if (is_eos) __hip_atomic_store(&st[SMP_FINISHED + row], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;                        // (a pad id outside the vocabulary must not become an out-of-bounds gather)
        }
        s_tok = (unsigned)tok;
        a.token[row] = (long long)tok;
        // every workgroup has read the draw counter and written its flag before the last one to arrive advances the shared words
        const int arrived = __hip_atomic_fetch_add(&st[SMP_ARRIVE], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == (int)gridDim.x - 1) {
            if (a.flags & SMP_FLAG_ADVANCE) {
                st[SMP_DRAW] = (int)(draw0 + 1u);
                if (draw0 + 1u == 0u) st[SMP_DRAW + 1] = (int)(draw1 + 1u);
            }
            if (a.flags & SMP_FLAG_EOS) {
                int n = 0;
                for (int r = 0; r < (int)gridDim.x && r < 8; ++r)
                    n += __hip_atomic_load(&st[SMP_FINISHED + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 ? 1 : 0;
                st[SMP_UNFINISHED] = n;
            }
            __hip_atomic_store(&st[SMP_ARRIVE], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (a.embed && (SEQ || row == 0)) {
            int* const pp = SEQ ? (int*)((char*)a.pos + (size_t)row * STEP_STRIDE) : a.pos;
            spos = pp[0] + 1;
            if (a.rope_table && spos > a.rope_rows) spos = a.rope_rows;        // saturating, as in the greedy tail
            pp[0] = spos;
        }
    }
    if (!a.embed) return;
    // ---- the greedy tail's duties: x = embed[token], the next position's cos/sin row
    __syncthreads();
    if ((SEQ || row == 0) && a.rope_cur && tid < 128) {
        const int rr = spos < a.rope_rows ? spos : a.rope_rows - 1;
        _Float16* const rc = SEQ ? (_Float16*)((char*)a.rope_cur + (size_t)row * STEP_STRIDE) : a.rope_cur;
        rc[tid] = a.rope_table[(size_t)rr * 128 + tid];
    }
    const _Float16* erow = a.embed + (size_t)s_tok * a.hidden;
    _Float16* x = a.x + (size_t)row * a.hidden;
    for (int c = tid; c < (a.hidden >> 3); c += SMP_THREADS) *(h8*)(x + 8 * c) = *(const h8*)(erow + 8 * c);
}

hipError_t launch_sample(const SampleArgs& a, int rows, hipStream_t st, bool seq) {
    hipLaunchKernelGGL(seq ? sample_kernel<true> : sample_kernel<false>, dim3(rows), dim3(SMP_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace amq
