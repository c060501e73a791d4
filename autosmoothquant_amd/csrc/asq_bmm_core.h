// What the batched int8 matmuls (asq_bmm.hip) and the decode attention kernel (asq_attn_decode.hip) share below the kernel level: the byte transpose and the
// guarded dword load of a row-major ([K, N]) B operand, and the constants of the softmax -> int8 formulation.
#pragma once
#include "asq_gemm_kernels.h"

namespace asq {

// 4 x 4 byte transpose: byte c of r[i] -> byte i of d[c]  (r[i] = 4 consecutive n of k row i  ->  d[c] = 4 consecutive k of column c)
__device__ __forceinline__ void bmm_transpose4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&d)[4])
{
    const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);   // r0.b0 r1.b0 r0.b1 r1.b1 | .b2 .b3
    const uint32_t u0 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), u1 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    d[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u), d[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
    d[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u), d[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

// 4 consecutive columns n .. n + 3 of row k of a [K, N] operand with row pitch ld, zero outside
__device__ __forceinline__ uint32_t load4_kn(const int8_t *base, int64_t ld, int64_t N, int64_t k, int64_t K, int64_t n, bool fast)
{
    if (k >= K || n >= N) return 0;
    const int8_t *p = base + k * ld + n;
    if (fast) return *(const uint32_t *)p;   // N % 16 == 0 (so is the row pitch ld), n % 4 == 0, base 16-B aligned
    uint32_t w = 0;
    for (int i = 0; i < 4; ++i)
        if (n + i < N) w |= (uint32_t)(uint8_t)p[i] << (8 * i);
    return w;
}

constexpr float SM_LOG2E = 1.44269502162933349609375f, SM_MAGIC = 12582912.0f;   // 1.5 * 2^23: the low mantissa bits of (x + SM_MAGIC) are rne(x)

}  // namespace asq
