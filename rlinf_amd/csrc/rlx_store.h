// rlx_store.h -- write-through global stores for data that the NEXT launch reads (gfx950).
//
// A plain store leaves its line dirty in the storing XCD's L2; the end of the launch then has to write every such line back
// before the dependent launch may start.  Data that no workgroup of the SAME launch reads again gains nothing from staying
// in L2 (the reader runs behind a launch boundary, usually on another XCD), so these stores carry `sc1`: the bytes go through
// to memory while the launch still computes, and the line is dropped instead of kept dirty.
// Users (measured per site): the bf16 fused launch's h / dz / states images and head partials, and the gradient
// slabs of every weight-gradient launch.  The f32x fused launch and the optimizer measured no gain and keep plain stores.
//
// All of them are VECTOR stores in forms the compiler counts in its vmcnt accounting (no inline assembly):
//   4 / 8 bytes   a relaxed agent-scope atomic store on a global pointer   -> global_store_dword[x2] ... sc1
//   16 bytes      a raw buffer store with aux = sc1 through a Span         -> buffer_store_dwordx4 ... sc1
// They order nothing: the kernel boundary stays the only synchronisation.  NEVER use them for bytes that the storing launch
// loads again (a plain load could be served from a stale L1 line).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rlx {
namespace wt {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// 4 or 8 bytes per lane.
template <typename T>
__device__ __forceinline__ void store(T* p, T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "wt::store: 4 or 8 bytes per lane");
    if constexpr (sizeof(T) == 4) {
        __hip_atomic_store((__attribute__((address_space(1))) unsigned*)(uintptr_t)p, __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)(uintptr_t)p, __builtin_bit_cast(unsigned long long, v),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The destination of 16-byte stores: a WAVE-UNIFORM base and its real extent in bytes.  The buffer resource drops a store that
// reaches past `bytes` silently, so the extent is the array's own, never a guess.  An extent that does not fit the resource's
// 32-bit range falls back to plain 16-byte stores (wave-uniform branch).
struct Span {
    char* base;
    size_t bytes;
};
__device__ __forceinline__ Span span(void* base, size_t bytes) {
    const uintptr_t b = (uintptr_t)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return Span{(char*)(((uintptr_t)hi << 32) | lo), bytes};
}
template <typename V>
__device__ __forceinline__ void store16(const Span& s, size_t byte_off, V v) {
    static_assert(sizeof(V) == 16, "wt::store16: 16 bytes per lane");
    if (s.bytes > 0xffffffffull) {
        *reinterpret_cast<V*>(s.base + byte_off) = v;
        return;
    }
    // raw buffer, stride 0; word 3 = DATA_FORMAT 32 (gfx9 family); aux 16 = sc1
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(s.base, 0, (int)(unsigned)s.bytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, (int)(unsigned)byte_off, 0, 16);
}

}  // namespace wt
}  // namespace rlx
