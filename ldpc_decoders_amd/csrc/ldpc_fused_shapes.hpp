// The min-sum shapes of the fused backend, stated ONCE per table class (arithmetic x check degree), and what expands them into the shape
// tables: per class one table of min-sum + sum-product, one of corrected min-sum (ALG_NMSA) and one of fixed-point min-sum (ALG_QMSA),
// each in a translation unit of its own (ldpc_fused_shapes_*.hip, built in parallel).  All three list the same tuples in the same order --
// preference order = table order -- so a decoder never changes shape because a correction is on.
//
// A row is ROW(kind, DC, DV, CRW, VRW, NW[, VRX, DVX]) (the template arguments of shape_entry / shape_entry64); kind says what the
// min-sum + sum-product table holds for the tuple beside plain min-sum:
//   PLAIN   its sum-product sibling
//   GRID    likewise, and the min-sum kernels also exist as exact-in-fp32 variants (priors on a 2^-k grid, exactness guard: shape_entry_grid).
//           The variants have none: a scale takes values off the prior grid, fixed-point min-sum quantises its priors itself.
//   NO_SPA  nothing: sum-product has no kernel of this tuple
#pragma once
#include "ldpc_fused_kernels.hpp"

// fp32, check degree 6 (the reference's code files).  Two waves per frame for n <= 1280 (fully regular codes only: no room for the zero
// row), else one wave per frame.
#define LDPC_MINSUM_SHAPES_F32_DC6(ROW)                                                                                                  \
    ROW(PLAIN, 6, 3, 4, 8, 1)  /* m <= 256, n <= 512 */                                                                                  \
    ROW(GRID, 6, 3, 5, 10, 2)  /* m <= 640, n <= 1280, 2 waves/frame */                                                                  \
    ROW(PLAIN, 6, 3, 10, 19, 1) /* m <= 640, n <= 1216, 1 wave/frame */                                                                  \
    /* irregular: check degrees <= 6 (short rows padded by a "certain" variable), variable degrees <= 8 (at most 256 above 3); two waves  \
       per frame (n <= 1215, system row) preferred, one wave per frame otherwise.  First choice: the same with six PAIR rounds per wave   \
       -- most variables of the reference's irregular ensembles have two edges: 34 instead of 40 gathers per wave and sweep -- for codes  \
       with at most 256 variables above degree 3 and at most 512 above 2 */                                                              \
    ROW(GRID, 6, 3, 5, 10, 2, vrx_arg(2, 6), 8)                                                                                          \
    ROW(GRID, 6, 3, 5, 10, 2, 2, 8)                                                                                                      \
    ROW(PLAIN, 6, 3, 10, 19, 1, 4, 8)                                                                                                    \
    /* four waves per frame: m <= 1536, n <= 2816 (48 KB of LDS per frame, 3 frames per CU) -- e.g. the (3,6) Margulis code n = 2640 */   \
    ROW(PLAIN, 6, 3, 6, 11, 4)                                                                                                           \
    /* sixteen waves per frame, the whole LDS of a CU (160 KB) for one frame: m <= 5120, n <= 10 175, check degrees <= 6, variable       \
       degrees <= 8 (at most 3072 above 3) -- the rate-1/2 irregular n = 10 000 ensemble.  First choice: two wide and six pair rounds     \
       per wave, 34 instead of 45 gathers per wave and sweep -- at most 2048 variables above degree 3 and 4096 above 2 */                \
    ROW(GRID, 6, 3, 5, 10, 16, vrx_arg(2, 6), 8)                                                                                         \
    ROW(GRID, 6, 3, 5, 10, 16, 3, 8)

// fp32, check degrees other than 6 -- the reference's generators take any (l, r) (src/codes.py:108-120,165-171) and any rho
// (src/ldpc.py:149-155, check degree rho + 1): two waves per frame, n around 1200.
#define LDPC_MINSUM_SHAPES_F32_DCX(ROW)                                                                                                  \
    ROW(PLAIN, 4, 3, 8, 10, 2)        /* (3,4)-regular: m <= 1024, n <= 1280 */                                                          \
    ROW(PLAIN, 8, 4, 5, 10, 2)        /* (4,8)-regular: m <= 640, n <= 1280 */                                                           \
    ROW(PLAIN, 5, 3, 6, 10, 2, 2, 4)  /* check degrees <= 5, variable degrees <= 4 (at most 256 above 3): (3,5)-regular, rho = x^4       \
                                         (src/ldpc.py); m <= 768, n <= 1215 */                                                           \
    ROW(PLAIN, 7, 3, 5, 10, 2, 3, 16) /* check degrees <= 7, variable degrees <= 16 (at most 384 above 3): rho = x^6, rate 1/2;          \
                                         m <= 640, n <= 1215 */

// fp64 (the reference's own arithmetic), check degree 6.
#define LDPC_MINSUM_SHAPES_F64_DC6(ROW)                                                                                                  \
    /* (3,6)-regular, n <= 1248: FOUR waves per frame on the same 40 KB (10 check rows: fused_check_rows), 16 waves per CU at <= 128     \
       VGPRs.  Same-footprint experiment (8 + 16 rows, n = 960): 4.36 ms with four waves per frame, 4.84 ms with two.  Sum-product (246  \
       VGPRs) has no room for four waves per SIMD */                                                                                     \
    ROW(NO_SPA, 6, 3, 3, 5, 4)                                                                                                           \
    /* (3,6)-regular, n <= 1216 (one marginal row reserved), two waves per frame: sum-product's shape, and the min-sum sibling of the    \
       shape above (LDPC_FUSED_NW=2).  Four waves on TWELVE check rows (46 KB, 3 frames per CU) were slower than this one: 6.87 vs 6.66  \
       ms per 65 536 frames (round 2) */                                                                                                 \
    ROW(PLAIN, 6, 3, 5, 10, 2)                                                                                                           \
    ROW(PLAIN, 6, 3, 5, 10, 2, vrx_arg(2, 6), 8) /* irregular n <= 1215, first choice: two wide and six pair rounds per wave (see fp32) */ \
    ROW(PLAIN, 6, 3, 5, 10, 2, 2, 8)             /* irregular n <= 1215: two wide variable rounds per wave, short check rows padded */    \
    ROW(PLAIN, 6, 3, 3, 6, 8)                    /* (3,6)-regular n <= 3008 (Margulis n = 2640): 96 KB per frame, one frame = 8 waves per CU */

// fp64, check degrees other than 6 (see the fp32 list).
#define LDPC_MINSUM_SHAPES_F64_DCX(ROW)                                                                                                  \
    ROW(PLAIN, 4, 3, 8, 10, 2)        /* (3,4)-regular: m <= 1024, n <= 1216; 43 KB per frame */                                         \
    ROW(PLAIN, 8, 4, 5, 10, 2)        /* (4,8)-regular: m <= 640, n <= 1216; 51 KB per frame */                                          \
    ROW(PLAIN, 5, 3, 6, 10, 2, 2, 4)  /* check degrees <= 5, variable degrees <= 4: (3,5)-regular, rho = x^4; 41 KB per frame */         \
    ROW(PLAIN, 7, 3, 5, 10, 2, 3, 16) /* check degrees <= 7, variable degrees <= 16: rho = x^6; 46 KB per frame */

// ---- what a table makes of a row: ENTRY is shape_entry (fp32 kernels) or shape_entry64 ----
#define LDPC_BASE_ROW_PLAIN(ENTRY, ...) ENTRY<ALG_MSA, __VA_ARGS__>(), ENTRY<ALG_SPA, __VA_ARGS__>(),
#define LDPC_BASE_ROW_GRID(ENTRY, ...) shape_entry_grid<__VA_ARGS__>(), ENTRY<ALG_SPA, __VA_ARGS__>(),
#define LDPC_BASE_ROW_NO_SPA(ENTRY, ...) ENTRY<ALG_MSA, __VA_ARGS__>(),
#define LDPC_ROW_BASE_F32(kind, ...) LDPC_BASE_ROW_##kind(shape_entry, __VA_ARGS__)
#define LDPC_ROW_BASE_F64(kind, ...) LDPC_BASE_ROW_##kind(shape_entry64, __VA_ARGS__)
#define LDPC_ROW_NMSA_F32(kind, ...) shape_entry<ALG_NMSA, __VA_ARGS__>(),
#define LDPC_ROW_NMSA_F64(kind, ...) shape_entry64<ALG_NMSA, __VA_ARGS__>(),
#define LDPC_ROW_QMSA_F32(kind, ...) shape_entry<ALG_QMSA, __VA_ARGS__>(),
#define LDPC_ROW_QMSA_F64(kind, ...) shape_entry64<ALG_QMSA, __VA_ARGS__>(),

// the table function of one translation unit: LDPC_SHAPE_TABLE(nmsa_f32_dc6, LDPC_MINSUM_SHAPES_F32_DC6, LDPC_ROW_NMSA_F32)
#define LDPC_SHAPE_TABLE(name, LIST, ROW)                  \
    namespace ldpc {                                       \
    const ShapeEntry* fused_shapes_##name(int* count) {    \
        static const ShapeEntry k[] = {LIST(ROW)};         \
        *count = (int)(sizeof(k) / sizeof(k[0]));          \
        return k;                                          \
    }                                                      \
    }
