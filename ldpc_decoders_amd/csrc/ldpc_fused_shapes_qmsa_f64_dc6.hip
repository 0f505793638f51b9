// Kernels of the fused backend -- fp64, check degree 6: fixed-point min-sum.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(qmsa_f64_dc6, LDPC_MINSUM_SHAPES_F64_DC6, LDPC_ROW_QMSA_F64)
