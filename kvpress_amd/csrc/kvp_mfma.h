// Device helpers of the matrix-core kernels (snapkv_mfma, ea_mfma, qproj, merge, compactor): the MFMA builtins, the LDS-DMA request
// and the wait counts that go with it, the geometry of a swizzled 16-bit key tile.  gfx950 only.
#pragma once
#include "kvp_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- MFMA --------------------------------------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x16: a lane holds 8 consecutive k of row / column lane & 31 (k group lane >> 5); C/D layout: col = lane & 31,
// row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  The accumulator is taken by const reference: by value the register allocation
// of the larger kernels (compactor.hip's ncattn_mfma_kernel) changes.
template <int DT> __device__ __forceinline__ f32x16 mma32(const uint4& a, const uint4& b, const f32x16& c);
template <> __device__ __forceinline__ f32x16 mma32<KVP_BF16>(const uint4& a, const uint4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16 mma32<KVP_F16>(const uint4& a, const uint4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// v_mfma_f32_16x16x32: a lane holds 8 consecutive k of row / column lane & 15 (k group lane >> 4); C/D: col = lane & 15, row = 4 * (lane >> 4) + reg
template <int DT> __device__ __forceinline__ f32x4 mma16(const uint4& a, const uint4& b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mma16<KVP_BF16>(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mma16<KVP_F16>(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- LDS-DMA -----------------------------------------------------------------------------------------------------------------------
// The instruction.  global_load_lds_dwordx4: every lane names a 16-byte global chunk, and the wave's 64 chunks land contiguously (1 KiB,
// in lane order) at the LDS byte address held in M0.  No VGPRs hold the data in transit and there is no ds_write phase.
//
// The M0 rule.  M0 is one register per wave, so the LDS address (`la` below) must be wave-uniform, and M0 is set OUTSIDE any divergent
// region.  M0 is a reserved register that hipcc never keeps values in, and nothing else in these kernels uses it.
//
// readfirstlane stays at the call.  The caller passes la = __builtin_amdgcn_readfirstlane(address), written out at the call site: wrapped
// in a function (uni() included) it changes the code of the surrounding kernel.
//
// Why asm, and the waits.  With the builtin form of the request hipcc makes every ds_read wait for vmcnt(0).  As inline asm the compiler
// does not count the requests, so the kernels wait for them by hand: dma_wait below.

// LDS byte address of a pointer into a __shared__ array.  (A macro: through a function parameter the pointer's address space is inferred
// later and the surrounding kernel compiles to other code.)
#define KVP_LDS_ADDR(p) ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)(p))

// nt: non-temporal (a stream that is read once)
__device__ __forceinline__ void lds_dma16(uint32_t la, const void* g, bool nt = false) {
    if (nt) asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off nt" ::"s"(la), "v"(g) : "memory");
    else asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(la), "v"(g) : "memory");
}
// the same for a wave in which only some lanes own a chunk (rows narrower than their LDS row): M0 is set by the whole wave, the request is
// made inside the branch; the other lanes request nothing and their LDS slots keep what they held.  Still ONE request of the wave for
// the wait counts.  lds_dma16_if is the two steps with the condition as an argument.
__device__ __forceinline__ void lds_dma_set_m0(uint32_t la) { asm volatile("s_mov_b32 m0, %0" ::"s"(la) : "memory"); }
__device__ __forceinline__ void lds_dma16_at_m0(const void* g, bool nt = false) {
    if (nt) asm volatile("global_load_lds_dwordx4 %0, off nt" ::"v"(g) : "memory");
    else asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(g) : "memory");
}
__device__ __forceinline__ void lds_dma16_if(bool has_chunk, uint32_t la, const void* g, bool nt = false) {
    lds_dma_set_m0(la);
    if (has_chunk) lds_dma16_at_m0(g, nt);
}
// the same with a wave-uniform 64-bit base (scalar registers; both halves through readfirstlane) plus a per-lane 32-bit byte offset: no
// vector address arithmetic per request.  (A macro: as a function it changes the scalar code around the one kernel that uses it.)
#define KVP_LDS_DMA16_SBASE(la, sbase, lane_off) asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(la), "v"(lane_off), "s"(sbase) : "memory")

// s_waitcnt through the builtin: unlike an asm string, hipcc's own wait-count bookkeeping sees it (it stops re-waiting for earlier
// loads inside the tile loop).  simm16 on gfx9: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14; a field at its maximum
// does not wait.  dma_wait<N>(): at most N of this wave's requests (and other vector-memory loads) still in flight, N <= 15 --
// requests complete in order, so the older ones have landed; the workgroup barrier that follows covers the other waves.
// LGKM = true also waits for every LDS read of the wave (lgkmcnt(0)).
template <int N, bool LGKM = false> __device__ __forceinline__ void dma_wait() {
    static_assert(N >= 0 && N <= 15, "vmcnt's low four bits");
    __builtin_amdgcn_s_waitcnt((LGKM ? 0x0070 : 0x0F70) | N);
}

// ---- a 128-key tile of 16-bit keys in LDS, XOR-swizzled, filled by the requests of a workgroup of THREADS -----------------------------
// DK = k-steps of 16 elements of a head: 4 / 6 / 8 / 16 for D = 64 / 96 / 128 / 256.  D = 96 keeps the 256-byte LDS rows of D = 128 and the
// lanes whose chunk lies beyond the 192-byte key row request nothing (lds_dma16_if).
template <int DK, int THREADS> struct KTileGeo {
    static constexpr int TILE = 128;                // keys per tile
    static constexpr int ROWB = DK == 6 ? 256 : DK * 32;   // bytes per key row IN LDS
    static constexpr int NCH = DK * 2;              // 16-byte chunks a key row really has
    static constexpr int CPR = ROWB / 16;           // 16-byte slots per LDS row
    static constexpr int RPW = 1024 / ROWB;         // rows one wave's request moves (64 lanes x 16 bytes)
    static constexpr int RPR = (THREADS / 64) * RPW;   // rows one request of the workgroup moves
    static constexpr int NREQ = TILE / RPR;         // requests per thread and tile
    static constexpr int TILEB = TILE * ROWB;
    static_assert(RPR % 16 == 0 && TILE % RPR == 0, "the swizzle of a row (period: 16 rows) depends on its index inside a request only");
    // XOR swizzle of a tile row's 16-byte slots, applied on the GLOBAL side of the DMA (slot p of row r holds chunk p ^ sw(r): the key row
    // stays coalesced): 16 consecutive rows of a fragment read must hit 16 distinct slots of the 256-byte bank line -- rows of 256 bytes:
    // the row's low four bits; rows of 128 bytes (two per bank line): bits 1 .. 3
    static __device__ __forceinline__ uint32_t sw(uint32_t row) { return DK == 4 ? ((row >> 1) & 7u) : (row & 15u); }
};
