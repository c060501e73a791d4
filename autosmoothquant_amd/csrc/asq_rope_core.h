// The per-vector rotation of the rotary embedding (HF "rotate_half" / NeoX convention): shared by the stand-alone pass (asq_rope.hip) and by the pass that
// quantises what it rotates (asq_rope_q8.hip) -- ONE statement of the arithmetic, so rotate + quantise in one launch is bit-identical to asq_rope followed by
// asq_quantize_act by construction.
//   w1 = dt(f32(dt(x1 * cos)) - x2 * sin)        w2 = dt(f32(dt(x2 * cos)) + x1 * sin)        per element of one 16-byte vector from each half of a head
// -- what torch computes for  addcmul(x1 * cos, x2, sin, value=-1)  /  addcmul(x2 * cos, x1, sin): fp16 bit for bit (the second rounding is the mixed-precision fma's
// single one, see fma_mix_f16x2); bf16 / fp32: the same operations at fp32 width (tests/test_hip_harness.py compares with the torch composition).
#pragma once
#include "asq_common.h"

namespace asq {

// d = f16(c +- a * b) with ONE rounding, per half of packed fp16 words: v_fma_mixlo_f16 / v_fma_mixhi_f16 evaluate the fma on the fp16 sources at fp32 width and round
// the exact result once to fp16 -- the instruction torch's own addcmul kernel compiles to on this platform (fptrunc(a + alpha * (b * c)) folded into it), so the two
// agree on every bit, also where the fp32 sum lands on an fp16 tie (19 of 1.3 M elements differ from a round-to-fp32-then-fp16 form).
template <bool NEG> __device__ __forceinline__ uint32_t fma_mix_f16x2(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d = 0;
    if constexpr (NEG) {
        asm("v_fma_mixlo_f16 %0, -%1, %2, %3 op_sel_hi:[1,1,1]" : "+v"(d) : "v"(a), "v"(b), "v"(c));
        asm("v_fma_mixhi_f16 %0, -%1, %2, %3 op_sel:[1,1,1] op_sel_hi:[1,1,1]" : "+v"(d) : "v"(a), "v"(b), "v"(c));
    } else {
        asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,1,1]" : "+v"(d) : "v"(a), "v"(b), "v"(c));
        asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,1,1] op_sel_hi:[1,1,1]" : "+v"(d) : "v"(a), "v"(b), "v"(c));
    }
    return d;
}

// a1 / a2: the same 16 bytes' worth of elements from the first / second half of a head, cw / sw: the matching cos / sin vectors; w1 / w2: the rotated halves, in DT
template <int DT> __device__ __forceinline__ void rope_vec(const v4i &a1, const v4i &a2, const v4i &cw, const v4i &sw, v4i &w1, v4i &w2)
{
    constexpr int VEC = ElemT<DT>::VEC;
    if constexpr (DT == ASQ_F16) {
        typedef _Float16 v2h __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // (element copies first: __builtin_bit_cast applied to a vector-element expression `a1[i]` reads element 0 for every i with this hipcc)
            const int x1w = a1[i], x2w = a2[i], cwi = cw[i], swi = sw[i];
            const uint32_t t1 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(v2h, x1w) * __builtin_bit_cast(v2h, cwi));   // dt(x1 * cos): v_pk_mul_f16
            const uint32_t t2 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(v2h, x2w) * __builtin_bit_cast(v2h, cwi));
            w1[i] = (int)fma_mix_f16x2<true>((uint32_t)x2w, (uint32_t)swi, t1);    // dt(t1 - x2 * sin)
            w2[i] = (int)fma_mix_f16x2<false>((uint32_t)x1w, (uint32_t)swi, t2);   // dt(t2 + x1 * sin)
        }
    } else {
        float x1[VEC], x2[VEC], cs[VEC], sn[VEC], o1[VEC], o2[VEC];
        vec_unpack<DT>(a1, x1);
        vec_unpack<DT>(a2, x2);
        vec_unpack<DT>(cw, cs);
        vec_unpack<DT>(sw, sn);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float t1 = ElemT<DT>::round(__fmul_rn(x1[j], cs[j])), t2 = ElemT<DT>::round(__fmul_rn(x2[j], cs[j]));
            o1[j] = __fadd_rn(t1, __fmul_rn(-x2[j], sn[j]));   // self + (value * tensor1) * tensor2, value = -1
            o2[j] = __fadd_rn(t2, __fmul_rn(x1[j], sn[j]));
        }
        if constexpr (DT == ASQ_F32) {
            w1 = (v4i){__float_as_int(o1[0]), __float_as_int(o1[1]), __float_as_int(o1[2]), __float_as_int(o1[3])};
            w2 = (v4i){__float_as_int(o2[0]), __float_as_int(o2[1]), __float_as_int(o2[2]), __float_as_int(o2[3])};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w1[i] = (int)((uint32_t)ElemT<DT>::store(o1[2 * i]) | ((uint32_t)ElemT<DT>::store(o1[2 * i + 1]) << 16));
                w2[i] = (int)((uint32_t)ElemT<DT>::store(o2[2 * i]) | ((uint32_t)ElemT<DT>::store(o2[2 * i + 1]) << 16));
            }
        }
    }
}

}  // namespace asq
