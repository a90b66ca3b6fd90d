// amq_lookup.hip -- the verify-and-propose tail of a prompt-lookup speculative decode step: the third tail of a token step (greedy: decode_tail_kernel,
// amq_decode.hip; sampled: amq_sample.hip).
//
// The step ran R = D + 1 rows of ONE sequence: row 0 the current token, rows 1 .. D guessed continuations (drafts).  One launch, one workgroup of 1024
// threads per row:
//   * every workgroup takes the arg-max of its logits row (first maximum, suppressed ids left out: decode_tail_kernel's code), leaves it in the state
//     block and takes a ticket; the LAST one to arrive -- nobody waits -- does the rest:
//   * acceptance: n = the longest prefix of drafts with draft[i] == argmax[i - 1]; the step emits argmax[0 .. n];
//   * history: the n + 1 tokens are appended to the sequence's token history (prompt + everything emitted), counters advanced;
//   * proposal (mode 0): for g = ngram_max .. 1 the MOST RECENT earlier occurrence of the history's last g tokens that is followed by at least one token;
//     the drafts are the up to D tokens behind it.  Every thread walks candidate continuation starts e and keeps (match length << 24 | e); one max-reduce
//     over the workgroup picks the longest match and, among those, the latest -- an integer maximum, so the result does not depend on scheduling.  The
//     history is read once per step (each candidate reads the <= 4 words in front of it: L2 / L1 hits), so it is not staged in LDS: a stage would read
//     every word once as well and add the LDS round trip;
//   * the next step's inputs: token[0] = argmax[n], token[j] = draft j (clamped into the vocabulary; the unclamped value stays in the state block for
//     the comparison), x[j] = embed[token[j]], block j's position = new position + j (saturating at rope_rows) and its cos/sin row.
// Everything that changes between replays lives in device memory.  Vector stores and ordinary atomics only.
//
// decode_tail_lookup_sample_kernel is the same tail under sampling: every workgroup DRAWS its row's token with the sampler of amq_sample_body.cuh
// (row j: draw counter c + j, sequence 0) in the place of the arg-max, and the last arriver -- the same device function, lk_last_arriver -- also
// advances the 64-bit draw counter by n + 1: the token emitted at index i of the sequence is drawn with counter i whichever row of whichever step
// computes it, so the output is what one-row sampled decoding draws from the same logits.
#include "amq_sample_body.cuh"

namespace amq {

constexpr int LK_THREADS = 1024;
constexpr int LK_MAX_ROWS = 8;
constexpr int LK_MAX_SUPPRESS = 8;
constexpr int LK_E_BITS = 24;                   // a continuation start fits 24 bits (history_cap <= 2^24: checked by the C ABI)

// What the last workgroup to arrive does once every row's chosen token is in LK_ARGMAX + row: acceptance, history, counters, proposal and the next
// step's inputs.  SAMPLED: the chosen tokens are draws -- the draw counter (draw0, draw1: what this workgroup read before its ticket, as every other
// one did) moves on by n + 1.  Every thread of the workgroup must call it.
template <bool SAMPLED>
__device__ __forceinline__ void lk_last_arriver(const LookupArgs& a, int R, int* smp, unsigned draw0, unsigned draw1) {
    __shared__ unsigned skey[LK_THREADS / 64];
    __shared__ int s_n, s_len, s_len0, s_pos;
    __shared__ int s_emit[LK_MAX_ROWS], s_tok[LK_MAX_ROWS], s_posj[LK_MAX_ROWS];
    const int tid = threadIdx.x;
    int* const st = a.state;

    // ---- the last arriver: acceptance, history, counters
    int D = st[LK_DRAFTS];
    D = D < 0 ? 0 : D > R - 1 ? R - 1 : D;
    int gmax = st[LK_NGRAM];
    gmax = gmax < 1 ? 1 : gmax > 4 ? 4 : gmax;
    const int mode = st[LK_MODE];
    int* const pos0 = (int*)((char*)a.step_states + 256);
    if (tid == 0) {
        int am[LK_MAX_ROWS];
        for (int j = 0; j < R; ++j) am[j] = __hip_atomic_load(&st[LK_ARGMAX + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int n = 0;
        while (n < D) {                                         // draft[i] is the token row i ran with; -1 = no draft, never matches
            const int d = st[LK_DRAFT + n + 1];
            if (d < 0 || d != am[n]) break;
            ++n;
        }
        const int len0 = st[LK_COUNT];
        for (int i = 0; i <= n; ++i) {
            s_emit[i] = am[i];
            if (len0 >= 0 && len0 + i < a.history_cap) a.history[len0 + i] = am[i];
        }
        st[LK_COUNT] = len0 + n + 1;
        st[LK_STEPS] = st[LK_STEPS] + 1;
        st[LK_ACCEPTED] = n;
        if (SAMPLED) {
            const unsigned long long c = (((unsigned long long)draw1 << 32) | draw0) + (unsigned)(n + 1);
            smp[SMP_DRAW] = (int)(unsigned)c;
            smp[SMP_DRAW + 1] = (int)(unsigned)(c >> 32);
        }
        s_n = n;
        s_len0 = len0;
        s_len = len0 + n + 1;
        s_pos = pos0[0] + n + 1;                                // the position of the next step's row 0
    }
    __syncthreads();
    const int n = s_n, len0 = s_len0, len = s_len;
    // (this step's tokens from LDS: their stores may still be in flight.  Both loads unconditional at clamped indices and the VALUE selected: a select
    //  between the two addresses would become a flat load)
    auto hist = [&](int i) {
        const int d = i - len0;
        const int fresh = s_emit[d < 0 ? 0 : d > LK_MAX_ROWS - 1 ? LK_MAX_ROWS - 1 : d];
        const int old = a.history[d < 0 ? i : len0 > 0 ? len0 - 1 : 0];
        return d >= 0 ? fresh : old;
    };

    // ---- proposal: key = (match length << 24) | continuation start, maximum over the candidates
    unsigned key = 0;
    if (mode == 0 && len0 >= 0 && len <= a.history_cap && len >= 2) {
        int tl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tl[k] = (k < gmax && len - 1 - k >= 0) ? hist(len - 1 - k) : -2;
        for (int e = 1 + tid; e <= len - 1; e += LK_THREADS) {   // the occurrence ends in front of e; history[e] exists: at least one token follows
            int m = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (m == k && k < gmax && e - 1 - k >= 0 && hist(e - 1 - k) == tl[k]) m = k + 1;
            if (m > 0) {
                const unsigned kk = ((unsigned)m << LK_E_BITS) | (unsigned)e;
                key = kk > key ? kk : key;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)key, off);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) skey[tid >> 6] = key;
    __syncthreads();
    key = 0;
#pragma unroll
    for (int w = 0; w < LK_THREADS / 64; ++w) key = skey[w] > key ? skey[w] : key;

    // ---- the next step's tokens, drafts and positions
    if (tid < LK_MAX_ROWS) {
        const int j = tid;
        int d = -1;
        if (j >= 1 && j <= D && key != 0) {
            const int idx = (int)(key & ((1u << LK_E_BITS) - 1)) + j - 1;
            if (idx < len) d = hist(idx);
        }
        if (j >= 1) st[LK_DRAFT + j] = d;                      // (mode 1: -1 everywhere; the host fills its own)
        if (j < R) {
            int t = j == 0 ? s_emit[n] : d;
            t = t < 0 ? 0 : t >= a.vocab ? a.vocab - 1 : t;
            s_tok[j] = t;
            a.token[j] = (long long)t;
            int p = s_pos + j;
            p = p < 0 ? 0 : p > a.rope_rows ? a.rope_rows : p;  // saturating: the attention kernel treats pos == max_seq as out of range
            s_posj[j] = p;
            *(int*)((char*)a.step_states + (size_t)j * STEP_STRIDE + 256) = p;
        }
    }
    __syncthreads();
    if (tid < 128 * R) {                                        // cos/sin rows of the new positions (last row once the cache is full)
        const int j = tid >> 7, c = tid & 127;
        const int rr = s_posj[j] < a.rope_rows ? s_posj[j] : a.rope_rows - 1;
        ((_Float16*)((char*)a.step_states + (size_t)j * STEP_STRIDE))[c] = a.rope_table[(size_t)rr * 128 + c];
    }
    const int hc = a.hidden >> 3;
    for (int c = tid; c < R * hc; c += LK_THREADS) {
        const int j = c / hc, cc = c - j * hc;
        *(h8*)(a.x + (size_t)j * a.hidden + 8 * cc) = *(const h8*)(a.embed + (size_t)s_tok[j] * a.hidden + 8 * cc);
    }
}

__global__ __launch_bounds__(LK_THREADS) void decode_tail_lookup_kernel(LookupArgs a) {
    __shared__ float smax[LK_THREADS / 64];
    __shared__ int sidx[LK_THREADS / 64];
    __shared__ int s_last;
    const int tid = threadIdx.x, row = blockIdx.x, R = (int)gridDim.x;
    const _Float16* logits = a.logits + (size_t)row * a.vocab;
    int* const st = a.state;

    // ---- arg-max of this row (decode_tail_kernel: first maximum, suppressed ids never chosen)
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int sup[LK_MAX_SUPPRESS];
#pragma unroll
    for (int j = 0; j < LK_MAX_SUPPRESS; ++j) sup[j] = a.suppress ? a.suppress[j] : -1;
    auto allowed = [&](int idx) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < LK_MAX_SUPPRESS; ++j) ok = ok && idx != sup[j];
        return ok;
    };
    const int chunks = a.vocab >> 3;
    for (int c = tid; c < chunks; c += LK_THREADS) {
        const h8 v = *(const h8*)(logits + 8 * c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
            if (f > best && (!a.suppress || allowed(8 * c + e))) { best = f; bi = 8 * c + e; }
        }
    }
    for (int i = 8 * chunks + tid; i < a.vocab; i += LK_THREADS) {
        const float f = (float)logits[i];
        if ((f > best || (f == best && i < bi)) && (!a.suppress || allowed(i))) { best = f; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if ((tid & 63) == 0) { smax[tid >> 6] = best; sidx[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        float b = smax[0];
        int ix = sidx[0];
        for (int w = 1; w < LK_THREADS / 64; ++w)
            if (smax[w] > b || (smax[w] == b && sidx[w] < ix)) { b = smax[w]; ix = sidx[w]; }
        if (ix == 0x7fffffff) ix = 0;
        // the row's result, then the ticket (release); the last arriver's ticket (acquire) sees every row's
        __hip_atomic_store(&st[LK_ARGMAX + row], ix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int arrived = __hip_atomic_fetch_add(&st[LK_TICKET], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == R - 1;
        if (last) __hip_atomic_store(&st[LK_TICKET], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // zero before and after every launch
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    lk_last_arriver<false>(a, R, nullptr, 0u, 0u);
}

// one workgroup per row as above, the row's token drawn instead of its arg-max
__global__ __launch_bounds__(LK_THREADS) void decode_tail_lookup_sample_kernel(LookupSampleArgs s) {
    static_assert(LK_THREADS == SMP_THREADS, "the sampler's workgroup");
    __shared__ unsigned s_draw;
    __shared__ int s_last;
    const LookupArgs& a = s.lk;
    const int tid = threadIdx.x, row = blockIdx.x, R = (int)gridDim.x;
    int* const st = a.state;
    int* const smp = s.sample_state;
    // the draw counter c of this step: read by every workgroup before its ticket, advanced by the last arriver behind all of them
    const unsigned draw0 = (unsigned)smp[SMP_DRAW], draw1 = (unsigned)smp[SMP_DRAW + 1];
    if (tid == 0) s_draw = 0;                                  // (the sampler's first barrier is behind this)
    struct { const _Float16* logits; int vocab; const int* suppress; int* state; const float* u_in; unsigned char* kept; }
        r{a.logits, a.vocab, a.suppress, smp, s.u_in, s.kept};
    smp_sample_row(r, row, (unsigned)row, 0u, &s_draw);        // row j draws with counter c + j, sequence 0
    if (tid == 0) {
        // the row's result, then the ticket (release); the last arriver's ticket (acquire) sees every row's
        __hip_atomic_store(&st[LK_ARGMAX + row], (int)s_draw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int arrived = __hip_atomic_fetch_add(&st[LK_TICKET], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == R - 1;
        if (last) __hip_atomic_store(&st[LK_TICKET], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // zero before and after every launch
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    lk_last_arriver<true>(a, R, smp, draw0, draw1);
}

hipError_t launch_decode_tail_lookup(const LookupArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(decode_tail_lookup_kernel, dim3(rows), dim3(LK_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_decode_tail_lookup_sample(const LookupSampleArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(decode_tail_lookup_sample_kernel, dim3(rows), dim3(LK_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace amq
