// amq_gemv_keyed1.hip -- the other one-row launches of a decode step with their bit-widths fixed at compile time (gemv_kernel_keyed,
// amq_gemv_body.cuh): PRO_RMSNORM with two segments (gate/up) or one, PRO_NONE with one (o_proj) on 8 waves and K <= 4096; PRO_MUL and
// PRO_SILU_MUL with one (down_proj) on 16 waves and K <= 16384.  q/k/v: amq_gemv_keyed0.hip.
#include "amq_gemv_body.cuh"
namespace amq {
hipError_t launch_keyed(const GemvKArgs& a, int prologue, int total_wg, size_t lds, hipStream_t st) {
    switch (prologue) {
        case PRO_RMSNORM:
            if (a.nseg == 3) return launch_keyed_qkv(a, total_wg, lds, st);
            if (a.nseg == 2) return launch_keyed_2<PRO_RMSNORM, 8, XCfg<8>::XC>(a, total_wg, lds, st);
            if (a.nseg == 1) return launch_keyed_1<PRO_RMSNORM, 8, XCfg<8>::XC>(a, total_wg, lds, st);
            break;
        case PRO_NONE:
            if (a.nseg == 1) return launch_keyed_1<PRO_NONE, 8, XCfg<8>::XC>(a, total_wg, lds, st);
            break;
        case PRO_MUL:
            if (a.nseg == 1) return launch_keyed_1<PRO_MUL, 16, XCfg<16>::XC>(a, total_wg, lds, st);
            break;
        case PRO_SILU_MUL:
            if (a.nseg == 1) return launch_keyed_1<PRO_SILU_MUL, 16, XCfg<16>::XC>(a, total_wg, lds, st);
            break;
    }
    return hipErrorInvalidValue;       // (gemv_route sends nothing else here)
}
}
