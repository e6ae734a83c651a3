// The operand split: the library's arithmetic contract, once.  Every dense kernel multiplies fp32 values on
// the 16-bit matrix pipe by splitting each operand into NP 16-bit pieces; the kernels differ only in WHICH block they scale
// over, and say so themselves.
//
//   NP = 3  bf16 pieces, exact: hi = bf16(v), mi = bf16(v - hi), lo = bf16(v - hi - mi), and hi + mi + lo == v in fp32 (three
//           8-bit significands cover fp32's 24; holds while lo is a normal bf16 number, i.e. for |v| >= 2^-110 or so).  Six
//           products per multiply (the pairs with i + j <= 4), fp32 accumulation.
//   NP = 2  fp16 pieces of S v, S a power of two chosen per block: hi = fp16(S v), lo = fp16(S v - hi).  Three products per
//           multiply (hi hi' + hi lo' + lo hi') into one fp32 accumulator.  The caller scales so that the block's largest
//           magnitude lies in [2^8, 2^15) -- block_scale puts it in [2^14, 2^15) --: an element within 2^16 of that maximum
//           has a normal low piece and keeps 22 significand bits (relative error <= 2^-22); a smaller one keeps an absolute
//           error of at most 2^-25 (half a unit of fp16's denormal grid), 2^-39 of a maximum at 2^14.
//   Scales  S = 2^k with m S in [2^TOP, 2^(TOP + 1)), and 1 / S, both exact powers of two, from the biased exponent eb of the
//           maximum m.  TOP = 14 for activations (block_scale), TOP = 12 for weights and for tensors whose pieces of many
//           rows are summed (weight_scale: |w| of any magnitude; r04 packed 64 w and overflowed to inf from |w| >= 2^9).
//           Outside 16 <= eb <= 250 -- a zero, denormal-range, huge or non-finite maximum -- S = 1 / S = 1: no scale is
//           invented for a block that has none, and both factors stay normal numbers.
// The splits and scales are __host__ __device__: tests/test_operand_split_host.py holds them to these bounds on the CPU.
#pragma once
#include "ms_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte access at any 4-byte aligned address
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int NP> __host__ __device__ constexpr int xrs() { return NP * 32 + 16; }   // bytes per LDS column of a 16-channel chunk

// (a, b) -> packed 16-bit pairs, a's pieces in the low halves, b's in the high halves: three words = NP 3 (bf16), two = NP 2 (fp16)
__host__ __device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    const f32x2 v = {a, b};
    const bf16x2 hi = __builtin_convertvector(v, bf16x2);
    const f32x2 r1 = v - __builtin_convertvector(hi, f32x2);
    const bf16x2 mi = __builtin_convertvector(r1, bf16x2);
    const f32x2 r2 = r1 - __builtin_convertvector(mi, f32x2);
    const bf16x2 lo = __builtin_convertvector(r2, bf16x2);
    h = __builtin_bit_cast(unsigned, hi);
    m = __builtin_bit_cast(unsigned, mi);
    l = __builtin_bit_cast(unsigned, lo);
}
__host__ __device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& l) {
    const f32x2 v = {a, b};
    const f16x2 hi = __builtin_convertvector(v, f16x2);
    const f16x2 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x2), f16x2);
    h = __builtin_bit_cast(unsigned, hi);
    l = __builtin_bit_cast(unsigned, lo);
}
// the same into NP words, for the kernels templated on the scheme
template <int NP>
__host__ __device__ __forceinline__ void split_pair(float a, float b, unsigned (&o)[NP]) {
    if constexpr (NP == 3) split_pair(a, b, o[0], o[1], o[2]);
    else split_pair(a, b, o[0], o[1]);
}

// 4 consecutive values -> one 8-byte group per piece: two split_pair calls, piece for piece.  (The two branches hold their
// temporaries differently -- names, arrays -- because each is the spelling its kernels were compiled from: the values are the
// same either way, the compiler's instruction order in k_conv_rows3 and k_stack_fwd is not.)
template <int NP>
__host__ __device__ __forceinline__ void split_quad(const float (&e)[4], uint2 (&o)[NP]) {
    if constexpr (NP == 3) {
        unsigned h0, m0, l0, h1, m1, l1;
        split_pair(e[0], e[1], h0, m0, l0);
        split_pair(e[2], e[3], h1, m1, l1);
        o[0] = make_uint2(h0, h1);
        o[1] = make_uint2(m0, m1);
        o[2] = make_uint2(l0, l1);
    } else {
        unsigned a[2], b[2];
        split_pair(e[0], e[1], a[0], a[1]);
        split_pair(e[2], e[3], b[0], b[1]);
        o[0] = make_uint2(a[0], b[0]);
        o[1] = make_uint2(a[1], b[1]);
    }
}

// m -> S = 2^(TOP - floor(log2 m)) and 1 / S, or 1 and 1 (see above)
template <int TOP>
__host__ __device__ __forceinline__ void pow2_scale(float m, float& S, float& invS) {
    const unsigned eb = (__builtin_bit_cast(unsigned, m) >> 23) & 0xFFu;
    const bool ok = eb >= 16u && eb <= 250u;
    S = ok ? __builtin_bit_cast(float, (254u + TOP - eb) << 23) : 1.f;
    invS = ok ? __builtin_bit_cast(float, (eb - TOP) << 23) : 1.f;
}
__host__ __device__ __forceinline__ void block_scale(float m, float& S, float& invS) { pow2_scale<14>(m, S, invS); }
__host__ __device__ __forceinline__ void weight_scale(float m, float& S, float& invS) { pow2_scale<12>(m, S, invS); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// A weight tensor's largest magnitude from the partial maxima its pack left in the image's tail: 16 read by the calling thread ...
__device__ __forceinline__ float weight_max16(const float* __restrict__ pm) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) m = fmaxf(m, pm[i]);
    return m;
}
// ... or 256 (called by ALL 256 threads of a pack workgroup, before any of them returns: the first wave reduces the partials,
// LDS broadcasts)
__device__ __forceinline__ float weight_max256(const float* __restrict__ pm) {
    __shared__ float wmax_s;
    if (threadIdx.x < 64) {
        const float m = wave_max(fmaxf(fmaxf(pm[threadIdx.x], pm[threadIdx.x + 64]), fmaxf(pm[threadIdx.x + 128], pm[threadIdx.x + 192])));
        if (threadIdx.x == 0) wmax_s = m;
    }
    __syncthreads();
    return wmax_s;
}

// Byte offset that every buffer descriptor of the library rejects: a load returns 0.0, a store is dropped
constexpr unsigned OOB = 0xF0000000u;

// 4 consecutive samples t .. t+3 of the row that starts at element `row_elems` (length L) of a tensor read through rs: one
// (possibly unaligned) 16-byte load; samples outside [0, L) read 0.0.  t must be a multiple of 4: the vector then lies wholly
// in front of the row or starts inside it, and only the one across the row END needs clearing.
__device__ __forceinline__ f32x4 load_row4(__amdgpu_buffer_rsrc_t rs, unsigned row_elems, int t, int L) {
    const bool any = t >= 0 && t < L;
    f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, any ? (row_elems + (unsigned)t) * 4u : OOB, 0, 0));
#pragma unroll
    for (int e = 1; e < 4; ++e) v[e] = t + e < L ? v[e] : 0.f;
    return v;
}

}  // namespace
