// fp64 kernels of the fused backend, check degree 6, fixed-point min-sum: the siblings of the min-sum shapes of
// ldpc_fused_shapes_f64_dc6.hip, in that table's order.
#include "ldpc_fused_kernels.hpp"

namespace ldpc {

const ShapeEntry* fused_shapes_qmsa_f64_dc6(int* count) {
    static const ShapeEntry k[] = {
        shape_entry64<ALG_QMSA, 6, 3, 3, 5, 4>(),                     // (3,6)-regular, n <= 1248: four waves per frame on ten check rows
        shape_entry64<ALG_QMSA, 6, 3, 5, 10, 2>(),                    // (3,6)-regular, n <= 1216, two waves per frame (LDPC_FUSED_NW=2)
        shape_entry64<ALG_QMSA, 6, 3, 5, 10, 2, vrx_arg(2, 6), 8>(),  // irregular n <= 1215, pair rounds
        shape_entry64<ALG_QMSA, 6, 3, 5, 10, 2, 2, 8>(),              // irregular n <= 1215
        shape_entry64<ALG_QMSA, 6, 3, 3, 6, 8>(),                     // (3,6)-regular n <= 3008 (Margulis n = 2640)
    };
    *count = (int)(sizeof(k) / sizeof(k[0]));
    return k;
}

}  // namespace ldpc
