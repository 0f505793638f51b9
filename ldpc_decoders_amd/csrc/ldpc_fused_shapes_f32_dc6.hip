// Kernels of the fused backend -- fp32, check degree 6: min-sum (with the exact-in-fp32 variants) and sum-product.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(f32_dc6, LDPC_MINSUM_SHAPES_F32_DC6, LDPC_ROW_BASE_F32)
