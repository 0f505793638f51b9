// Kernels of the fused backend -- fp64, other check degrees: min-sum and sum-product.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(f64_dcx, LDPC_MINSUM_SHAPES_F64_DCX, LDPC_ROW_BASE_F64)
