// Kernels of the fused backend -- fp32, other check degrees: fixed-point min-sum.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(qmsa_f32_dcx, LDPC_MINSUM_SHAPES_F32_DCX, LDPC_ROW_QMSA_F32)
