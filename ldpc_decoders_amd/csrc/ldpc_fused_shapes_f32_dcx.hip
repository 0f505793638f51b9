// Kernels of the fused backend -- fp32, other check degrees: min-sum and sum-product.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(f32_dcx, LDPC_MINSUM_SHAPES_F32_DCX, LDPC_ROW_BASE_F32)
