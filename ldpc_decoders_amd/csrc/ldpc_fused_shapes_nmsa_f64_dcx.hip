// Kernels of the fused backend -- fp64, other check degrees: corrected (normalised / offset) min-sum.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(nmsa_f64_dcx, LDPC_MINSUM_SHAPES_F64_DCX, LDPC_ROW_NMSA_F64)
