// Kernels of the fused backend -- fp64, check degree 6: corrected (normalised / offset) min-sum.  The shapes: ldpc_fused_shapes.hpp.
#include "ldpc_fused_shapes.hpp"

LDPC_SHAPE_TABLE(nmsa_f64_dc6, LDPC_MINSUM_SHAPES_F64_DC6, LDPC_ROW_NMSA_F64)
