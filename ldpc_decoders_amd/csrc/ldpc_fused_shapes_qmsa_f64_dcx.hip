// fp64 kernels of the fused backend for check degrees other than 6, fixed-point min-sum: the siblings of the min-sum shapes of
// ldpc_fused_shapes_f64_dcx.hip, in that table's order.
#include "ldpc_fused_kernels.hpp"

namespace ldpc {

const ShapeEntry* fused_shapes_qmsa_f64_dcx(int* count) {
    static const ShapeEntry k[] = {
        shape_entry64<ALG_QMSA, 4, 3, 8, 10, 2>(),         // (3,4)-regular
        shape_entry64<ALG_QMSA, 8, 4, 5, 10, 2>(),         // (4,8)-regular
        shape_entry64<ALG_QMSA, 5, 3, 6, 10, 2, 2, 4>(),   // check degrees <= 5, variable degrees <= 4
        shape_entry64<ALG_QMSA, 7, 3, 5, 10, 2, 3, 16>(),  // check degrees <= 7, variable degrees <= 16
    };
    *count = (int)(sizeof(k) / sizeof(k[0]));
    return k;
}

}  // namespace ldpc
