// Shared device/host helpers for libkvpress_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#pragma GCC visibility push(default)   // the C ABI: the only symbols the library exports on purpose (besides KVP_INTERNAL_API, kvp_host.h)
#include "../../include/kvpress_hip.h"
#include "../../include/kvpress_hip_lab.h"
#pragma GCC visibility pop

#include "kvp_host.h"

// ---- element access ---------------------------------------------------------------------------
template <int DT> struct Elem;
template <> struct Elem<KVP_F32> {
    using T = float;
    static constexpr int PER16 = 4;  // elements per 16-byte vector
    static __device__ __forceinline__ float ld(const T* p) { return *p; }
};
template <> struct Elem<KVP_F16> {
    using T = _Float16;
    static constexpr int PER16 = 8;
    static __device__ __forceinline__ float ld(const T* p) { return (float)*p; }
};
template <> struct Elem<KVP_BF16> {
    using T = uint16_t;
    static constexpr int PER16 = 8;
    static __device__ __forceinline__ float ld(const T* p) { return __uint_as_float(((uint32_t)*p) << 16); }
};

// the two 16-bit halves of a dword as floats
template <int DT> __device__ __forceinline__ float lo16(uint32_t w);
template <int DT> __device__ __forceinline__ float hi16(uint32_t w);
template <> __device__ __forceinline__ float lo16<KVP_BF16>(uint32_t w) { return __uint_as_float(w << 16); }
template <> __device__ __forceinline__ float hi16<KVP_BF16>(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }
template <> __device__ __forceinline__ float lo16<KVP_F16>(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu)); }
template <> __device__ __forceinline__ float hi16<KVP_F16>(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }

// unpack a 16-byte vector into floats (4 for f32, 8 for f16/bf16)
template <int DT> __device__ __forceinline__ void unpack16(const uint4& v, float* f);
template <> __device__ __forceinline__ void unpack16<KVP_F32>(const uint4& v, float* f) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
}
template <> __device__ __forceinline__ void unpack16<KVP_BF16>(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = lo16<KVP_BF16>(w[i]); f[2 * i + 1] = hi16<KVP_BF16>(w[i]);
    }
}
template <> __device__ __forceinline__ void unpack16<KVP_F16>(const uint4& v, float* f) {   // (a packed conversion per dword: not lo16 / hi16's scalar ones)
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h2 p = __builtin_bit_cast(h2, w[i]);
        f[2 * i] = (float)p.x; f[2 * i + 1] = (float)p.y;
    }
}
// sum of the squares of the elements of a 16-byte vector (one fma chain, element order)
template <int DT> __device__ __forceinline__ float sumsq16(const uint4& v) {
    float f[Elem<DT>::PER16];
    unpack16<DT>(v, f);
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < Elem<DT>::PER16; ++i) a = fmaf(f[i], f[i], a);
    return a;
}

// ---- rounding to the model dtype (round to nearest even) ---------------------------------------------------------------------------
// Two families.  round_dt / to_dt / st_dt / pack2 use the hardware conversions through inline asm.  NEVER apply them directly to an
// MFMA accumulator: the asm reads the accumulator registers with no wait states after the MFMA that writes them (the compiler pads
// hazards around its own instructions, not inside asm), which read partly written accumulators on hardware.  After an MFMA use the
// asm-free round_acc / to_dt_acc.
// bf16 by integer arithmetic: fin() receives the rounded pattern in the upper 16 bits (the lower ones are whatever the carry left; NaN
// stays a quiet NaN) and masks or shifts it -- inside each branch, which is the shape both users were compiled from
template <typename F> __device__ __forceinline__ auto bf16_rne(float x, F fin) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return fin(u | 0x00400000u);
    return fin(u + 0x7FFFu + ((u >> 16) & 1u));
}
template <int DT> __device__ __forceinline__ float round_acc(float x);
template <> __device__ __forceinline__ float round_acc<KVP_F16>(float x) { return (float)(_Float16)x; }
template <> __device__ __forceinline__ float round_acc<KVP_BF16>(float x) {
    return bf16_rne(x, [](uint32_t r) { return __uint_as_float(r & 0xFFFF0000u); });
}
template <int DT> __device__ __forceinline__ typename Elem<DT>::T to_dt_acc(float x);
template <> __device__ __forceinline__ float to_dt_acc<KVP_F32>(float x) { return x; }
template <> __device__ __forceinline__ _Float16 to_dt_acc<KVP_F16>(float x) { return (_Float16)x; }
template <> __device__ __forceinline__ uint16_t to_dt_acc<KVP_BF16>(float x) {
    return bf16_rne(x, [](uint32_t r) { return (uint16_t)(r >> 16); });
}

// value rounded to the storage dtype and back (torch's eager ops round after every mul / add in the model dtype)
template <int DT> __device__ __forceinline__ float round_dt(float x);
template <> __device__ __forceinline__ float round_dt<KVP_F32>(float x) { return x; }
template <> __device__ __forceinline__ float round_dt<KVP_F16>(float x) {
    // opaque to the optimiser: written as (float)(_Float16)x, hipcc demotes the surrounding mul / add to f16 and then
    // contracts them into v_fma_f16 -- one rounding where torch's separate half ops have two
    float r;
    asm("v_cvt_f16_f32 %0, %1\n\tv_cvt_f32_f16 %0, %0" : "=v"(r) : "v"(x));
    return r;
}
template <> __device__ __forceinline__ float round_dt<KVP_BF16>(float x) {  // round-to-nearest-even to bf16
    // the hardware conversion (gfx950): one instruction + a shift instead of the 7-instruction integer emulation with its
    // inf / nan branch -- the RoPE / re-rotation kernels round six times per output pair and were bound by exactly that
#if defined(__gfx950__)
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(x));
    return __uint_as_float(r << 16);
#else   // any other target of a stray --offload-arch: the integer round-to-nearest-even (NaN stays a quiet NaN)
    return round_acc<KVP_BF16>(x);
#endif
}
// float -> a stored element of the model dtype (torch's .to(dtype))
template <int DT> __device__ __forceinline__ typename Elem<DT>::T to_dt(float x);
template <> __device__ __forceinline__ float to_dt<KVP_F32>(float x) { return x; }
template <> __device__ __forceinline__ _Float16 to_dt<KVP_F16>(float x) { return (_Float16)x; }
template <> __device__ __forceinline__ uint16_t to_dt<KVP_BF16>(float x) { return (uint16_t)(__float_as_uint(round_dt<KVP_BF16>(x)) >> 16); }
template <int DT> __device__ __forceinline__ void st_dt(typename Elem<DT>::T* p, float x) { *p = to_dt<DT>(x); }
// two floats -> one dword of 16-bit values, low half = lo: one conversion instruction
template <int DT> __device__ __forceinline__ uint32_t pack2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack2<KVP_BF16>(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
template <> __device__ __forceinline__ uint32_t pack2<KVP_F16>(float lo, float hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 p = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, p);
}
// the same dword from two round_dt conversions: the form the RoPE kernels were built and measured with (pack2 computes the same bits
// with fewer instructions, but it is another kernel: switching needs a timing of its own)
template <int DT> __device__ __forceinline__ uint32_t join2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t join2<KVP_BF16>(float lo, float hi) {
    return (__float_as_uint(round_dt<KVP_BF16>(lo)) >> 16) | (__float_as_uint(round_dt<KVP_BF16>(hi)) & 0xFFFF0000u);
}
template <> __device__ __forceinline__ uint32_t join2<KVP_F16>(float lo, float hi) { return pack2<KVP_F16>(lo, hi); }
// one RoPE output element with torch's rounding: round(round(a * ca) + round(b * sb)); __fmul_rn / __fadd_rn keep the
// ops separately rounded as in torch's eager mul, mul, add (never contracted to an fma)
template <int DT> __device__ __forceinline__ float rope_elem(float a, float ca, float b, float sb) {
    return round_dt<DT>(__fadd_rn(round_dt<DT>(__fmul_rn(a, ca)), round_dt<DT>(__fmul_rn(b, sb))));
}

// 16-byte loads/stores with an optional non-temporal (streaming, read/write-once) hint
typedef uint32_t kvp_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ uint4 ld16(const void* p) {
    if (NT) {
        const kvp_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const kvp_u32x4*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4*>(p);
}
template <bool NT> __device__ __forceinline__ void st16(void* p, const uint4& v) {
    if (NT) {
        kvp_u32x4 w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<kvp_u32x4*>(p));
    } else {
        *reinterpret_cast<uint4*>(p) = v;
    }
}

// ---- wave / block reductions -----------------------------------------------------------------
// butterflies over the wave's 64 lanes: every lane ends with the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// a value that every lane holds identically, moved to scalar registers: branches on it are scalar branches (no saved exec masks), and
// values handed to an asm block through "s" constraints must sit in SGPRs
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ float uni(float x) { return __uint_as_float(uni(__float_as_uint(x))); }
template <typename T> __device__ __forceinline__ T* uni(T* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    return (T*)(uintptr_t)(((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v));
}

// float <-> order-preserving uint32 (larger float <=> larger key; atomicMax / radix select over floats of any sign); -0.0 is canonicalised to +0.0
__device__ __forceinline__ uint32_t float_to_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(u);
}
