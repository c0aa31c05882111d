// bayhunter_amd/csrc/bh_okey.h -- the order-preserving key of a float or a double, and its inverse: the one statement of the rule
// that makes a radix pass over unsigned keys order values the way `<` does.
//
// The bits of a value with its sign bit set are inverted, those of any other value get the sign bit: keys compare as unsigned
// integers in the order of the values (-inf < .. < -0 < +0 < .. < +inf; a NaN lies beyond the infinity of its sign).  The radix
// selects of chain_diag_kernel.hip and posterior_select.h and the radix sort of chain_rank_kernel.hip all count digits of these keys.
#ifndef BH_OKEY_H
#define BH_OKEY_H

#include <hip/hip_runtime.h>

// The bits of a value and the value of bits, host and device alike.  Plain inline functions like the device library's
// __float_as_uint and its kin, which the kernels called here before: the compiler inlines them when it inlined those, and the
// kernels' instructions stay what they were (as always-inline functions they do not: profiles/chain_diag_kit_refactor.txt).
__host__ __device__ static inline unsigned okey_bits(float v)
{
    unsigned u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}
__host__ __device__ static inline unsigned long long okey_bits(double v)
{
    unsigned long long u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}
__host__ __device__ static inline float okey_float(unsigned u)
{
    float v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}
__host__ __device__ static inline double okey_double(unsigned long long u)
{
    double v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

__host__ __device__ __forceinline__ unsigned okey32(float v)
{
    const unsigned u = okey_bits(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float okey32_value(unsigned k) { return okey_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }
__host__ __device__ __forceinline__ unsigned long long okey64(double v)
{
    const unsigned long long u = okey_bits(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double okey64_value(unsigned long long k)
{
    return okey_double((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k);
}

// ... by the type of the value, for code that is a template on it: okey_t<T> is the key type of T
__host__ __device__ __forceinline__ unsigned okey_of(float v) { return okey32(v); }
__host__ __device__ __forceinline__ unsigned long long okey_of(double v) { return okey64(v); }
__host__ __device__ __forceinline__ double okey_value(unsigned k) { return (double)okey32_value(k); }
__host__ __device__ __forceinline__ double okey_value(unsigned long long k) { return okey64_value(k); }
template <typename T> using okey_t = decltype(okey_of(T()));

#endif
