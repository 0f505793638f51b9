// Kernels of the fused backend -- fp64, check degree 6: min-sum and sum-product.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(f64_dc6, LDPC_MINSUM_SHAPES_F64_DC6, LDPC_ROW_BASE_F64)
