// fp32 kernels of the fused backend, check degree 6, fixed-point min-sum (q-bit saturating messages, ldpc_cn.hpp): one sibling of every
// min-sum shape of ldpc_fused_shapes_f32_dc6.hip, in that table's order (see there for what each shape is for).  No exact-in-fp32 variants:
// every value is a small integer already, fixed-point decoders refuse LDPC_FLAG_PRIOR_GRID.
#include "ldpc_fused_kernels.hpp"

namespace ldpc {

const ShapeEntry* fused_shapes_qmsa_f32_dc6(int* count) {
    static const ShapeEntry k[] = {
        shape_entry<ALG_QMSA, 6, 3, 4, 8, 1>(),                       // m <= 256, n <= 512
        shape_entry<ALG_QMSA, 6, 3, 5, 10, 2>(),                      // m <= 640, n <= 1280, 2 waves/frame
        shape_entry<ALG_QMSA, 6, 3, 10, 19, 1>(),                     // m <= 640, n <= 1216, 1 wave/frame
        shape_entry<ALG_QMSA, 6, 3, 5, 10, 2, vrx_arg(2, 6), 8>(),    // irregular, two waves per frame, pair rounds
        shape_entry<ALG_QMSA, 6, 3, 5, 10, 2, 2, 8>(),                // irregular, two waves per frame
        shape_entry<ALG_QMSA, 6, 3, 10, 19, 1, 4, 8>(),               // irregular, one wave per frame
        shape_entry<ALG_QMSA, 6, 3, 6, 11, 4>(),                      // four waves per frame: m <= 1536, n <= 2816
        shape_entry<ALG_QMSA, 6, 3, 5, 10, 16, vrx_arg(2, 6), 8>(),   // sixteen waves per frame, pair rounds
        shape_entry<ALG_QMSA, 6, 3, 5, 10, 16, 3, 8>(),               // sixteen waves per frame
    };
    *count = (int)(sizeof(k) / sizeof(k[0]));
    return k;
}

}  // namespace ldpc
