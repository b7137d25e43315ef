// lgm_amd/csrc/cdna4.h -- the gfx950 device idioms that more than one kernel file uses: the 16-bit MFMA, LDS DMA with
// its counted wait, the ballot prefix mask and the transposing LDS read. Everything is inlined; tile layouts, swizzles
// and address arithmetic stay with the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgm_attn.h"
#include "work_split.h"

namespace lgm {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef short s4v __attribute__((__vector_size__(8)));
typedef __attribute__((ext_vector_type(8))) short s8v;

// The 16-bit operand types by dtype code (LGM_ATTN_BF16 / LGM_ATTN_F16): the 8-element MFMA operand and the bit
// pattern of 1.0 (ONE2: two of them in a dword), for the ones operand that makes an MFMA sum rows.
template <int DT> struct Op16;
template <> struct Op16<LGM_ATTN_BF16> {
    using V8 = bf16x8;
    static constexpr short ONE = 0x3f80;
    static constexpr unsigned ONE2 = 0x3f803f80u;
};
template <> struct Op16<LGM_ATTN_F16> {
    using V8 = f16x8;
    static constexpr short ONE = 0x3c00;
    static constexpr unsigned ONE2 = 0x3c003c00u;
};

// v_mfma_f32_16x16x32_{bf16,f16}: c += a b, on typed operands or on their raw bits
template <int DT>
__device__ __forceinline__ f32x4 mfma16(typename Op16<DT>::V8 a, typename Op16<DT>::V8 b, f32x4 c) {
    if constexpr (DT == LGM_ATTN_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
template <int DT> __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    using V8 = typename Op16<DT>::V8;
    return mfma16<DT>(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c);
}

// The LDS address of a shared-memory pointer as a 32-bit offset (an address-space cast, not the 64-bit flat pointer:
// kept live across a staging loop, flat pointers were spilled and each reload's vmcnt(0) serialised the DMAs).
__device__ __forceinline__ unsigned lds_offset(const void *p) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// LDS DMA, global_load_lds_dword{,x3,x4}: each lane's BYTES bytes go from src straight to LDS, no staging registers.
// Lane i's bytes land at lds_base + 16 i in the 12- and 16-byte forms (one wave-instruction fills 1 KiB) and at
// lds_base + 4 i in the 4-byte form; lds_base is wave-uniform.
// Inline asm on purpose: the compiler's waitcnt pass treats any later LDS access that may alias a pending DMA as
// dependent on it and would wait for a prefetch right after issuing it. Hidden from the pass, the DMA only makes the
// pass's own vmcnt waits more conservative (still correct); the caller orders its completion with vm_wait<n>() in every
// issuing wave plus a barrier (the pass does not track LDS written by DMA). The compiler owns M0 and does not
// preserve it around a statement, so M0 is saved, written and restored inside the one statement that reads it; the
// s_nop 0 is the M0 write -> LDS-DMA wait state, which nothing checks.
#define LGM_LDS_DMA(width)                                                                                     \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_" width " %2, off\n\t"    \
                 "s_mov_b32 m0, %0"                                                                            \
                 : "=&s"(saved)                                                                                \
                 : "s"(m), "v"(src)                                                                            \
                 : "memory")
template <int BYTES> __device__ __forceinline__ void lds_dma(const void *src, unsigned lds_base) {
    static_assert(BYTES == 4 || BYTES == 12 || BYTES == 16, "global_load_lds widths");
    const unsigned m = __builtin_amdgcn_readfirstlane(lds_base);
    unsigned saved;
    if constexpr (BYTES == 16) LGM_LDS_DMA("dwordx4");
    else if constexpr (BYTES == 12) LGM_LDS_DMA("dwordx3");
    else LGM_LDS_DMA("dword");
}
#undef LGM_LDS_DMA

// s_waitcnt vmcnt(N), leaving lgkmcnt / expcnt alone: at most N of this wave's vector-memory operations (its LDS DMA
// included) are still pending. A hard wait that the compiler's waitcnt pass sees. The count is six bits wide, its
// upper two at bits 15:14 of the immediate.
template <int N = 0> __device__ __forceinline__ void vm_wait() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit count");
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}

// The lanes below `lane` as a ballot mask (a compaction's prefix: __popcll(ballot & lanemask_lt(lane))).
__device__ __forceinline__ unsigned long long lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// Two transposing reads (ds_read_b64_tr_b16) joined into one 8-element MFMA operand: p_lo supplies elements 0 .. 3 and
// p_hi 4 .. 7. The read moves 16-bit elements whatever their type, so the i16 form serves bf16 and f16.
__device__ __forceinline__ s8v tr16_pair(const void *p_lo, const void *p_hi) {
    const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v *)(p_lo));
    const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v *)(p_hi));
    return s8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace lgm
