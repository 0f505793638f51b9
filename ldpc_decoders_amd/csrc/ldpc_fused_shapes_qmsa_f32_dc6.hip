// Kernels of the fused backend -- fp32, check degree 6: fixed-point min-sum.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(qmsa_f32_dc6, LDPC_MINSUM_SHAPES_F32_DC6, LDPC_ROW_QMSA_F32)
