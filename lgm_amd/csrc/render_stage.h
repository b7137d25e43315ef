// lgm_amd/csrc/render_stage.h -- what the forward and the backward compositing (render_fwd.hip, render_bwd.hip) share:
// the LDS image of a staged chunk of a tile's sorted list (StageT), its LDS-DMA staging, the read side of the per-wave
// entry lists, the sentinel row, the alpha cap, the chunk and batch sizes, and the diagnostic builds' stamp macros.
#pragma once
#include "cdna4.h"
#include "render_common.h"

namespace lgm {

// Section stamps of the diagnostic builds (shares only: the stamps' waits change the schedule), as statements: a source
// turns them on for its own kernel by defining LGM_SEC_STAMPS before this header (render_fwd.hip under LGM_FWD_STAMPS,
// render_bwd.hip under LGM_BWD_STAMPS); everywhere else each SEC_* line expands to nothing.
__device__ __forceinline__ unsigned long long sec_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#ifdef LGM_SEC_STAMPS
#define SEC_ON(...) __VA_ARGS__
#else
#define SEC_ON(...)
#endif
#define SEC_VAR(v) SEC_ON(unsigned long long v = 0)                // a cycle accumulator
#define SEC_DECL(a, n) SEC_ON(unsigned long long a[n] = {})        // an array of n accumulators
#define SEC_T(t) SEC_ON(const unsigned long long t = sec_stamp())  // t: the shader clock now
#define SEC_ADD(acc, a, b) SEC_ON(acc += (b) - (a))                // the cycles from stamp a to stamp b
#define SEC_SUB(acc, x) SEC_ON(acc -= (x))
#define SEC_FLUSH(cond, dst, a, n) /* if (cond): dst[q] += a[q] for q < n, by atomics */ \
    SEC_ON(if (cond) _Pragma("unroll") for (int q_ = 0; q_ < (n); q_++) atomicAdd(&(dst)[q_], (a)[q_]))

// min(0.99, e) for e = exp2(.) >= 0 as an integer min on the bits (ordered like the floats for e >= 0; NaN -> 0.99
// as fminf): one VALU, where fminf on an exp result costs a canonicalising v_max first
__device__ __forceinline__ float alpha_cap(float e) {
    return __uint_as_float(min(__float_as_uint(e), 0x3f7d70a4u));
}

constexpr int WU_LD = 68;  // row stride of the per-wave [16 columns][64 pixels] gradient image (16-B aligned rows)
// Columns 4..11 of that image hold pixel p at p ^ 8 (WU_SWZ): with the 17-slot row stride this puts the 16 lanes of
// every ds_read_b128 group of the batch reads (lanes {0-3, 12-15, 20-27}, ... : MI355X_MICROARCH.md §LDS) on 16
// distinct 16-B slots; unswizzled, columns 10, 11 and 12, 13 of one group shared two slots (2-way).
__device__ __forceinline__ int wu_swz(int col) { return (col >= 4 && col < 12) ? 8 : 0; }
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;
typedef __attribute__((ext_vector_type(2))) float f32x2v;
constexpr int MB = 8;      // entries per moment-MFMA batch (columns 0..7: w, 8..15: u)

// One staged chunk (256 entries in the forward, 64 in the backward), written by LDS DMA (global_load_lds: 16-B lane
// stride for both the 16-B and the 12-B form): P from gP, Q from gQ, R.xyz from the Gaussian row's colour; R.w holds
// the Gaussian id (written by the backward's chunk head, for its flush). The backward alternates two of these: chunk
// c + 1 streams into one while chunk c is composited from the other.
template <int ROWS>  // entries per chunk; row ROWS is the sentinel
struct StageBufT {
    float4 P[ROWS + 1];  // x, y, A, B
    float4 Q[ROWS + 1];  // C, opacity, tau, depth
    float4 R[ROWS + 1];  // r, g, b, id bits
};
template <int NB, int PAD, int ROWS = TILE_PIX>  // NB 2: double-buffered, 1: synchronous staging
struct StageT {                                   // PAD: list padding = entries evaluated per step (multiple of 4)
    static constexpr int kRows = ROWS;
    using Buf = StageBufT<ROWS>;
    Buf buf[NB];
    // (forward-only: the backward reads the forward's masks, and keeps the array so that its later LDS arrays stay put)
    unsigned char mask[ROWS];                 // quadrant mask of the current chunk's entries
    unsigned short list[4][ROWS + PAD];       // per-wave compacted entry indices, padded with the sentinel (ROWS)
};
// Forward: staged synchronously, chunk by chunk (double-buffered staging measured +20 us on the pool: most tiles
// saturate within a chunk or two, and the prefetch costs LDS and registers); FWD_FU = 4 entries evaluated per step
// (8 per step spilled). Backward: 64-entry chunks, double-buffered.
constexpr int FWD_FU = 4;
#ifndef LGM_FWD_SMALL_TILES
#define LGM_FWD_SMALL_TILES 256
#endif
constexpr int FWD_SMALL_TILES = LGM_FWD_SMALL_TILES;  // launches of at most this many tiles take k_render_fwd<., 8>
constexpr int BWD_CHUNK = 64;
// backward lists are padded to MB with the sentinel: every list position is one MFMA batch column (k_render_bwd)
using StageBwd = StageT<2, MB, BWD_CHUNK>;

// Issue the LDS DMA of one entry (this lane's row of wave w's 64-row slice; lds_dma, cdna4.h). Asynchronous: the
// rows are valid after vm_wait() in every issuing wave followed by a barrier.
// SH (LGM_RENDER_SH_MASK): the colour comes from the view's own record in `gauss` = Dims::sh_col [BV, N, 3] (12-B
// stride, 4-B aligned like the row's RGB) instead of the scene's 14-wide row.
template <bool SH = false, class Buf>
__device__ __forceinline__ void stage_dma(Buf &B, int w, unsigned gid, size_t gbase, int b, int N,
                                          const float4 *__restrict__ gP, const float4 *__restrict__ gQ,
                                          const float *__restrict__ gauss) {
    // one 32-bit LDS base, the three rows at constant offsets from it
    const unsigned base = lds_offset(&B) + (unsigned)(w * 64 * 16);
    lds_dma<16>(gP + gbase + gid, base + (unsigned)offsetof(Buf, P));
    lds_dma<16>(gQ + gbase + gid, base + (unsigned)offsetof(Buf, Q));
    if constexpr (SH) lds_dma<12>(gauss + (gbase + gid) * 3, base + (unsigned)offsetof(Buf, R));
    else lds_dma<12>(gauss + ((size_t)b * N + gid) * 14 + 11, base + (unsigned)offsetof(Buf, R));
}

// U (a multiple of 4) consecutive list entries from kk (a multiple of 4): list_raw reads them (an LDS read that can
// be issued a step ahead), list_decode makes them wave-uniform (scalar) indices.
template <int U, class Stage>
__device__ __forceinline__ void list_raw(const Stage &S, int w, int kk, uint2 (&raw)[U / 4]) {
    static_assert(U % 4 == 0, "list reads are 8-B words");
#pragma unroll
    for (int h = 0; h < U / 4; h++) raw[h] = *reinterpret_cast<const uint2 *>(&S.list[w][kk + 4 * h]);
}
template <int U>
__device__ __forceinline__ void list_decode(const uint2 (&raw)[U / 4], int (&jj)[U]) {
#pragma unroll
    for (int h = 0; h < U / 4; h++) {
        const unsigned lo = __builtin_amdgcn_readfirstlane(raw[h].x), hi = __builtin_amdgcn_readfirstlane(raw[h].y);
        jj[4 * h + 0] = lo & 0xffffu;
        jj[4 * h + 1] = lo >> 16;
        jj[4 * h + 2] = hi & 0xffffu;
        jj[4 * h + 3] = hi >> 16;
    }
}
template <class Stage>
__device__ __forceinline__ void init_sentinel(Stage &S) {
    if (threadIdx.x < sizeof(S.buf) / sizeof(S.buf[0])) {
        auto &B = S.buf[threadIdx.x];
        B.P[Stage::kRows] = make_float4(0.f, 0.f, 0.f, 0.f);
        B.Q[Stage::kRows] = make_float4(0.f, -INFINITY, 0.f, 0.f);  // L = -inf: alpha 0
        B.R[Stage::kRows] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace lgm
