// The reference's int8 linears with a fused bias epilogue (csrc/kernels/linear.cu:13-491, bindings.cpp:5-15): one GEMM launch through
// launch_gemm with an [N] bias read in its own dtype -- no [M, N] bias image, no second pass over the output.
//
//   acc[m, n] = sum_k x[m, k] * w[n, k]                                   exact int32, two's-complement wrap (as asq_gemm_i8_i32)
//   v         = fl(fl(alpha * float(acc)) + fl(beta * float(bias[n])))    the add skipped when beta == 0 (CUTLASS is_source_needed(), EpiI8::one)
//   ASQ_LIN_B32_O32        int32 bias -> int32  acc + bias[n] (wraps; alpha, beta ignored)
//   ASQ_LIN_B32_O32_SCALED int32 bias -> int32  sat_i32(rne(v))
//   ASQ_LIN_BF32_OF32      f32 bias   -> f32    v
//   ASQ_LIN_B8_O8          int8 bias  -> int8   sat_i8(rne(v))            (EpiI8::one with c = bias[n])
//   ASQ_LIN_RELU_B8_O8     int8 bias  -> int8   sat_i8(rne(max(v, 0)))
// Two roundings (multiply, then add) as EpiI8::one / EpiDequant::one, not a contracted fma: b8_o8 equals I8CUGEMM.linear_a8_w8_b8_o8_ and bfp32_ofp32
// with beta = 1 equals asq_linear_w8a8(F32, s_scalar = alpha, bias) bit for bit.
//
// One epilogue functor per output width (EpiBias<4> int32, EpiBias<5> f32, EpiBias<1> int8); the kind's remaining choices (wrap / scaled, ReLU) and
// alpha / beta are wave-uniform runtime values.  cols() hands the per-column bias term to the store as a v4f: fl(beta * float(bias)) for the
// scaled forms, and for ASQ_LIN_B32_O32 the int32 bias BITS (|bias| may reach 2^31: a float would round it).
#include "asq_gemm_kernels.h"

namespace asq {

template <int OUT> struct EpiBias {  // OUT: 4 = int32, 5 = fp32 (4-byte outputs), 1 = int8
    using Mma = MmaI8;
    static constexpr bool kHasRow = false, kHasCol = false, kHasBias = true;
    static constexpr int kOutBytes = OUT == 1 ? 1 : 4;
    static constexpr int kBiasBytes = OUT == 1 ? 1 : 4;  // int8 bias for int8 outputs, int32 / fp32 otherwise
    void *out;
    const void *bias;  // [N] in the kind's bias dtype
    int64_t N;         // row stride of out
    float alpha, beta;
    int mode;          // OUT == 4: 1 = scaled (sat_i32(rne(v))), 0 = acc + bias with wrap;  OUT == 1: 1 = ReLU
    bool vec_ok;       // N % 4 == 0, out and bias aligned to 4 elements: 16-B (4-B for int8) vector loads and stores

    __device__ __forceinline__ EpiBias rebased(int, int, int64_t, int64_t) const { return *this; }
    static constexpr bool kColView = true;
    EpiBias col_view(int64_t n0) const  // host side: the sub-problem starting at output column n0 (n0 % 256 == 0 keeps every alignment)
    {
        return EpiBias{(char *)out + n0 * kOutBytes, (const char *)bias + n0 * kBiasBytes, N, alpha, beta, mode, vec_ok};
    }
    __device__ __forceinline__ float row(int64_t) const { return 1.0f; }
    __device__ __forceinline__ bool wraps() const { return OUT == 4 && mode == 0; }

    // b[i] = the bias term of column n + i: the int32 bits for the wrapping form, fl(beta * float(bias)) otherwise (0 when beta == 0: never added)
    __device__ __forceinline__ void cols(int64_t n, int64_t Ncols, v4f &sc, v4f &b) const
    {
        sc = (v4f){0.f, 0.f, 0.f, 0.f};
        b = (v4f){0.f, 0.f, 0.f, 0.f};
        if (!wraps() && beta == 0.0f) return;
        v4i raw = {0, 0, 0, 0};
        if constexpr (OUT == 1) {
            const int8_t *p = (const int8_t *)bias + n;
            if (vec_ok && n + 3 < Ncols) {
                const uint32_t u = *(const uint32_t *)p;
                raw = (v4i){(int)(int8_t)u, (int)(int8_t)(u >> 8), (int)(int8_t)(u >> 16), (int)(int8_t)(u >> 24)};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < Ncols) raw[i] = p[i];
            }
        } else {
            const int32_t *p = (const int32_t *)bias + n;
            if (vec_ok && n + 3 < Ncols) {
                raw = *(const v4i *)p;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < Ncols) raw[i] = p[i];
            }
        }
        if (wraps()) {
            b = __builtin_bit_cast(v4f, raw);
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = __fmul_rn(beta, OUT == 5 ? __int_as_float(raw[i]) : (float)raw[i]);
    }

    __device__ __forceinline__ float value(int acc, float b) const
    {
        float v = __fmul_rn(alpha, (float)acc);  // v_cvt_f32_i32: round-to-nearest-even
        if (beta != 0.0f) v = __fadd_rn(v, b);
        return v;
    }
    __device__ __forceinline__ static int sat_i32(float v)  // sat_i32(rne(v)); NaN -> 0 (as quant_i8)
    {
        const float r = rintf(v);
        return r >= 2147483648.0f ? 0x7FFFFFFF : r >= -2147483648.0f ? (int)r : r != r ? 0 : (int)0x80000000u;
    }
    // one output in its storage encoding (the 32-bit pattern for 4-byte outputs, the int8 value otherwise)
    __device__ __forceinline__ int one(int acc, float b) const
    {
        if constexpr (OUT == 4) return mode == 0 ? (int)((uint32_t)acc + __float_as_uint(b)) : sat_i32(value(acc, b));
        if constexpr (OUT == 5) return __float_as_int(value(acc, b));
        float v = value(acc, b);
        if (mode == 1) v = (v < 0.0f) ? 0.0f : v;  // ReLU
        return quant_i8(v);
    }
    __device__ __forceinline__ v4i pack(const v4i &a, float, const v4f &, const v4f &b) const
    {
        static_assert(OUT != 1, "pack: 4-byte outputs");
        return (v4i){one(a[0], b[0]), one(a[1], b[1]), one(a[2], b[2]), one(a[3], b[3])};
    }
    __device__ __forceinline__ void store4(int64_t m, int64_t n, const v4i &a, float, const v4f &, const v4f &b, int64_t Ncols) const
    {
        if constexpr (OUT == 1) {
            int8_t *p = (int8_t *)out + m * N + n;
            if (vec_ok && n + 3 < Ncols) {
                *(uint32_t *)p = (uint32_t)(one(a[0], b[0]) & 0xFF) | ((uint32_t)(one(a[1], b[1]) & 0xFF) << 8) | ((uint32_t)(one(a[2], b[2]) & 0xFF) << 16) |
                                 ((uint32_t)(one(a[3], b[3]) & 0xFF) << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < Ncols) p[i] = (int8_t)one(a[i], b[i]);
            }
        } else {
            int32_t *p = (int32_t *)out + m * N + n;
            if (vec_ok && n + 3 < Ncols) {
                *(v4i *)p = pack(a, 1.0f, b, b);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < Ncols) p[i] = one(a[i], b[i]);
            }
        }
    }
};

static inline bool lin_mul(int64_t x, int64_t y, int64_t &r) { return !__builtin_mul_overflow(x, y, &r); }

}  // namespace asq

using namespace asq;

extern "C" int asq_linear_i8_bias(const int8_t *x, const int8_t *w, const void *bias, void *out, int kind, int64_t M, int64_t N, int64_t K, float alpha,
                                  float beta, void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_linear_i8_bias");
    int64_t mn = 0, bytes = 0, mk = 0, nk = 0;
    ASQ_REQUIRE(M >= 0 && N >= 0 && K >= 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), ASQ_ERR_DIM, "asq_linear_i8_bias: bad dims M=%lld N=%lld K=%lld",
                (long long)M, (long long)N, (long long)K);
    ASQ_REQUIRE(lin_mul(M, N, mn) && lin_mul(mn, 4, bytes) && lin_mul(M, K, mk) && lin_mul(N, K, nk), ASQ_ERR_DIM,
                "asq_linear_i8_bias: size overflows 64 bits (M=%lld N=%lld K=%lld)", (long long)M, (long long)N, (long long)K);
    ASQ_REQUIRE(kind >= ASQ_LIN_B32_O32 && kind <= ASQ_LIN_RELU_B8_O8, ASQ_ERR_DTYPE, "asq_linear_i8_bias: bad kind %d", kind);
    if (mn == 0) return ASQ_OK;
    ASQ_REQUIRE(out != nullptr && bias != nullptr, ASQ_ERR_NULL, "asq_linear_i8_bias: NULL out / bias");
    ASQ_REQUIRE(K == 0 || (x != nullptr && w != nullptr), ASQ_ERR_NULL, "asq_linear_i8_bias: NULL x / w");
    const bool i8 = kind == ASQ_LIN_B8_O8 || kind == ASQ_LIN_RELU_B8_O8;
    ASQ_REQUIRE(i8 || ((((uintptr_t)out | (uintptr_t)bias) & 3) == 0), ASQ_ERR_ALIGN, "asq_linear_i8_bias: out / bias misaligned for their element");
    const uintptr_t vmask = i8 ? 3 : 15;
    const bool vec_ok = (N % 4 == 0) && ((((uintptr_t)out | (uintptr_t)bias) & vmask) == 0);
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
    case ASQ_LIN_B32_O32:
    case ASQ_LIN_B32_O32_SCALED:
        return launch_gemm(x, w, M, N, K, EpiBias<4>{out, bias, N, alpha, beta, kind == ASQ_LIN_B32_O32_SCALED ? 1 : 0, vec_ok}, s, "asq_linear_i8_bias", workspace,
                           workspace_bytes);
    case ASQ_LIN_BF32_OF32:
        return launch_gemm(x, w, M, N, K, EpiBias<5>{out, bias, N, alpha, beta, 0, vec_ok}, s, "asq_linear_i8_bias", workspace, workspace_bytes);
    default:
        return launch_gemm(x, w, M, N, K, EpiBias<1>{out, bias, N, alpha, beta, kind == ASQ_LIN_RELU_B8_O8 ? 1 : 0, vec_ok}, s, "asq_linear_i8_bias", workspace,
                           workspace_bytes);
    }
}
