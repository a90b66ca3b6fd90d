// amq_gemv_keyed0.hip -- the one-row q/k/v launch (PRO_RMSNORM, three segments, 8 waves, K <= 4096) with the segments' bit-widths fixed at compile
// time: the ten ascending triples of gemv_kernel_keyed (amq_gemv_body.cuh)
#include "amq_gemv_body.cuh"
namespace amq {
hipError_t launch_keyed_qkv(const GemvKArgs& a, int total_wg, size_t lds, hipStream_t st) {
    return launch_keyed_3<PRO_RMSNORM, 8, XCfg<8>::XC>(a, total_wg, lds, st);
}
}
