/*
 * qkv_forms.h -- a layer's stored Q|K|V read back as fp32, piece by piece, in the three forms a plan leaves it in
 * (include/kernelHandler.h, VH_QKV_*).  Shared by the kernels that read the buffer beside the forward: attn_map.hip (the
 * class token's attention row) and rollout.hip (the whole head-mean attention matrix).
 *
 * A piece is 16 bytes per part of one row:
 *   fp32 rows          [rows][3E]            4 columns
 *   three-part planes  [3E/32][3][rows][32]  8 columns, three 16-byte loads, value = (p0 + p1) + p2 exactly
 *   one-part fp16      [3E/32][rows][32]     8 columns
 * LPK adjacent lanes on one key cover 256 contiguous bytes of an fp32 row, or one 64-byte segment of a plane (16 adjacent
 * keys per wave are then 16 adjacent segments).  A head that starts mid-chunk (head_dim 80, odd h) is a matter of piece
 * indices: piece p of the head is piece (E + hD)/8 + p of the row, chunk = that / 4.
 */
#ifndef VIT_HIP_QKV_FORMS_H
#define VIT_HIP_QKV_FORMS_H

#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"

constexpr int AM_MAX_HEAD_DIM = KL_CLS_ATTN_MAX_HEAD_DIM;

typedef _Float16 am_half8 __attribute__((ext_vector_type(8)));
typedef __bf16 am_bf16x8 __attribute__((ext_vector_type(8)));

/* per form: columns per piece, lanes per key, pieces a lane can own at head_dim 128 */
template <int FORM> struct AmForm { static constexpr int PIECE = 8, LPK = 4, MAXP = AM_MAX_HEAD_DIM / 8 / 4; };
template <> struct AmForm<VH_QKV_ROWS_F32> { static constexpr int PIECE = 4, LPK = 16, MAXP = AM_MAX_HEAD_DIM / 4 / 16; };

/* PIECE columns of row `row` from column `col` (a multiple of PIECE), decoded exactly to fp32 */
template <int FORM>
__device__ __forceinline__ void load_piece(const char *__restrict__ qkv, size_t rows, int row_floats, size_t row, int col, float *out)
{
    if constexpr (FORM == VH_QKV_ROWS_F32) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(qkv + (row * (size_t)row_floats + (size_t)col) * sizeof(float));
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[e] = v[e];
    } else if constexpr (FORM == VH_QKV_PLANES3) {
        const char *src = qkv + ((size_t)(col >> 5) * 3 * rows + row) * 64 + (size_t)(col & 31) * 2;
        am_bf16x8 part[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            part[pl] = __builtin_bit_cast(am_bf16x8, *reinterpret_cast<const f32x4 *>(src + (size_t)pl * rows * 64));
#pragma unroll
        for (int e = 0; e < 8; ++e)   /* exact: the parts are disjoint slices of one 24-bit significand */
            out[e] = ((float)part[0][e] + (float)part[1][e]) + (float)part[2][e];
    } else {
        const char *src = qkv + ((size_t)(col >> 5) * rows + row) * 64 + (size_t)(col & 31) * 2;
        const am_half8 v = __builtin_bit_cast(am_half8, *reinterpret_cast<const f32x4 *>(src));
#pragma unroll
        for (int e = 0; e < 8; ++e)
            out[e] = (float)v[e];
    }
}

#endif
