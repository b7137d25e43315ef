// lgm_amd/csrc/render_layout.h -- where every byte of the render path's caller-owned workspace lives: the regions
// make_layout carves up, the gradient-accumulator block inside it, the words of the misc block, and the map of the
// diagnostics counter buffer. Plain C++ (no HIP header), so a host compiler can include and test it
// (tests/test_render_layout.py). render_common.h includes it and adds the typed pointers and the device math.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "lgm_render.h"

#ifdef __HIPCC__
#define LGM_HD __host__ __device__ __forceinline__
#else
#define LGM_HD inline
#endif

namespace lgm {

constexpr int BX = 16, BY = 16, TILE_PIX = BX * BY;  // 256 pixels per tile = 4 wavefronts (8x8 quadrants)
constexpr int NACC = 10;  // gradient partials per (view, Gaussian): mean2D(2) conic(3) opacity rgb(3) depth
constexpr int NACC_V = 6, NACC_S = 4;  // of them per (view, Gaussian) / per (scene, Gaussian): AccumLayout

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

struct Region {  // bytes [off, off + bytes)
    size_t off, bytes;
    LGM_HD size_t end() const { return off + bytes; }
};

// ---- The gradient-accumulator block (Layout::accum; every offset below is relative to it) ----------------------
// Four regions, in this order:
//   main    the view-dependent partials (mean2D 2, conic 3, depth) per (view, Gaussian) in records of NACC_V, then
//           the view-independent ones (opacity, colour) per (scene, Gaussian) in records of NACC_S -- the views of
//           a scene add into one record, so the forward zeroes and k_preproc_bwd reads 24 + 16 / V bytes per (view,
//           Gaussian) instead of 40. Elements are fp32, or int64 fixed point in deterministic mode (`elem` bytes).
//   needle  float mode only: fp64 sums of the conic partials of NEEDLE records, 3 per (view, Gaussian), 8-B aligned
//           (so up to 4 bytes of padding precede it). A needle is a record whose conic condition (A + C)^2 /
//           (AC - B^2) exceeds ACC_NEEDLE (or is not positive definite), decided on the stored record (rec_needle)
//           identically by the binning, the backward's flush and the preprocess backward (via bit 31 of the rect).
//   aa_part LGM_RENDER_ANTIALIAS only: the opacity partial per (view, Gaussian) instead of per scene (the preprocess
//           backward needs dL/do^ of each view: lgm_render.h), one element each.
//   aa_s    LGM_RENDER_ANTIALIAS only: the factors s themselves, one fp32 per (view, Gaussian). k_aa_factor writes
//           them ahead of the binning; the binning and the preprocess backward read them. Not an accumulator.
// Who zeroes what, and when (a backward adds into zeroed accumulators):
//   main    k_render_fwd's epilogue, every forward: fwd_zero(), the region rounded up to whole 16-B stores. The
//           overrun (< 16 B) lands on the needle block's first entry or in the padding that ends the block's
//           256-B-aligned reservation, never beyond it.
//   needle  k_bin, record by record, as it flags a record as a needle (unflagged entries are never read).
//   aa_part a memset in launch_binning, every forward with the bit.
//   all three again: launch_render_bwd's memset of clear() under LGM_RENDER_BACKWARD_AGAIN, which clears what the
//           previous backward of the same forward left. The factors stay.
// Spherical harmonics (the LGM_RENDER_SH_MASK bits, degree 1..3: lgm_render.h) append five more regions, each 16-B
// aligned; without the bits they are empty and the block is byte for byte what it was:
//   sh_part the colour partials per (view, Gaussian) instead of per scene, 3 elements each (fp32, or int64 with the
//           per-view flush bound in deterministic mode): the SH backward needs G_v = dL/dcolour of each view. The
//           scene records' colour elements are then never added to (they stay zero). Zeroed by a memset in
//           launch_sh_pack, every forward with the bits, and again by launch_render_bwd's memset of sh_part under
//           LGM_RENDER_BACKWARD_AGAIN.
//   sh_col  the colours the basis gives, fp32 [B, V, N, 3]: k_sh_colour writes the visible records' after the
//           binning, k_render_fwd and k_render_bwd stage them in place of the row's RGB. An invisible record's is
//           never written nor read (it is in no tile list). Not an accumulator.
//   sh_mask one byte per (view, Gaussian), bit c = channel c's unclamped colour is positive (upstream's `clamped`,
//           inverted). Written beside sh_col, read by k_sh_bwd. Not an accumulator.
//   sh_g14  [B, N, 14] fp32: columns 0:14 of the caller's wider rows, copied by k_sh_pack ahead of the binning, so
//           that every kernel written for 14-wide rows (k_bin, k_aa_factor, k_preproc_bwd) runs unchanged on them.
//   sh_dg14 [B, N, 14] fp32: what k_preproc_bwd writes as d_gaussians; k_sh_bwd then writes the caller's wide rows
//           from its columns 0:11, the position term and dL/dsh. Overwritten by every backward, never accumulated.
struct AccumLayout {
    int elem;  // bytes per accumulator element: 4 (fp32), 8 (int64, deterministic mode)
    Region main, needle, aa_part, aa_s, sh_part, sh_col, sh_mask, sh_g14, sh_dg14;
    size_t total;
    LGM_HD Region clear() const { return {0, aa_s.off}; }  // every accumulator (and the padding between them)
    LGM_HD Region fwd_zero() const { return {0, (main.bytes + 15) / 16 * 16}; }
};
constexpr int NEEDLE_DBL = 3;  // fp64 needle sums per (view, Gaussian): the conic partials
LGM_HD size_t accum_main_elems(size_t B, size_t V, size_t N) { return B * V * N * NACC_V + B * N * NACC_S; }
// elements from the block's start to the needle region in float mode (the main region, padded to 8 B), and to what
// follows the needle region
LGM_HD size_t accum_needle_elem0(size_t B, size_t V, size_t N) { return (accum_main_elems(B, V, N) + 1) & ~(size_t)1; }
LGM_HD size_t accum_needle_elem1(size_t B, size_t V, size_t N) {
    return accum_needle_elem0(B, V, N) + B * V * N * (NEEDLE_DBL * sizeof(double) / sizeof(float));
}
LGM_HD AccumLayout accum_layout(size_t B, size_t V, size_t N, bool det, bool aa, int sh_degree = 0) {
    AccumLayout a;
    a.elem = det ? 8 : 4;
    a.main = {0, accum_main_elems(B, V, N) * a.elem};
    a.needle = det ? Region{a.main.end(), 0}
                   : Region{accum_needle_elem0(B, V, N) * 4, B * V * N * NEEDLE_DBL * sizeof(double)};
    a.aa_part = {a.needle.end(), aa ? B * V * N * a.elem : 0};
    a.aa_s = {a.aa_part.end(), aa ? B * V * N * sizeof(float) : 0};
    a.total = a.aa_s.end();
    const size_t sh = sh_degree > 0 ? 1 : 0;
    auto next = [&](size_t bytes) {  // (16-B aligned; an empty region sits where the block ended)
        const Region r{sh ? (a.total + 15) / 16 * 16 : a.total, sh * bytes};
        a.total = r.end();
        return r;
    };
    a.sh_part = next(B * V * N * 3 * a.elem);
    a.sh_col = next(B * V * N * 3 * sizeof(float));
    a.sh_mask = next(B * V * N);
    a.sh_g14 = next(B * N * 14 * sizeof(float));
    a.sh_dg14 = next(B * N * 14 * sizeof(float));
    return a;
}
// the SH degree of a call's options (0: plain RGB rows) and the row width it implies
LGM_HD int sh_degree_of(int options) { return (options & LGM_RENDER_SH_MASK) >> LGM_RENDER_SH_SHIFT; }
LGM_HD int sh_row_width(int degree) { return degree > 0 ? 11 + 3 * (degree + 1) * (degree + 1) : 14; }
// Device code keeps no AccumLayout live across its hot loops (hoisted addresses spilled in k_render_bwd): it calls
// these at the point of use. Indices into the block as an array of its elements (fp32 / int64), or of doubles.
// k = (b V + v) N + i: the (view, Gaussian) record; (b, i): the (scene, Gaussian) record; BV = B V.
LGM_HD size_t accum_view_elem(size_t k, int q) { return k * NACC_V + q; }  // q: mean2D 0..1, conic 2..4, depth 5
LGM_HD size_t accum_scene_elem(size_t BV, size_t N, size_t b, size_t i, int q) {  // q: opacity 0, colour 1..3
    return BV * N * NACC_V + (b * N + i) * NACC_S + q;
}
LGM_HD size_t accum_needle_dbl(size_t B, size_t V, size_t N, size_t k, int c) {  // (float mode) c: conic 0..2
    return accum_needle_elem0(B, V, N) / 2 + k * NEEDLE_DBL + c;
}
// (antialias) the opacity partial of record k is element accum_aa_elem0 + k: the kernels add the workgroup-uniform
// and the per-lane parts of k one after the other
LGM_HD size_t accum_aa_elem0(size_t B, size_t V, size_t N, bool det) {
    return det ? accum_main_elems(B, V, N) : accum_needle_elem1(B, V, N);
}

// Deterministic mode's per-flush overflow bound (k_render_bwd): in that mode an accumulator takes at most one flush
// per tile list its Gaussian appears in -- one work item per tile, an entry once per list. A per-view record (mean2D,
// conic, depth) sees the T tiles of its view; a per-scene record (opacity, colour: accum_scene_elem) the V * T
// tiles of all views of its scene. With every flush |a| <= 2^62 / 2^ceil(log2 flushes), no sum of them reaches 2^62,
// whatever their signs, so int64 cannot wrap. (The design value of a flush is <= ~2^51: DET_BITS.)
LGM_HD int det_flush_limit_log2(int V, int T, bool scene_record) {
    const long long f = scene_record ? (long long)V * T : (long long)T;
    int c = 0;
    while ((1ll << c) < f) c++;  // ceil(log2 f)
    return 62 - c;
}

// ---- The misc block: MISC_BYTES of counters right after tile_count --------------------------------------------
constexpr int MISC_BYTES = 64;
constexpr int MISC_PAIRS = 0;      // u64 [0..1]: emitted and reference (Gaussian, tile) pair counts (k_bin, STATS)
constexpr int MISC_CK_REGION = 4;  // u32 [4..11]: the 8 backward-checkpoint region counters (k_render_fwd)
constexpr int MISC_LOSS_ARRIVAL = 12;  // u32: the fused loss reduction's arrival counter (k_loss_reduce)
constexpr int MISC_DET_SAT = 13;       // u32: deterministic mode's saturated flushes (k_render_bwd)
constexpr int MISC_PAIRS_N = 2, MISC_CK_REGIONS = 8;
static_assert((MISC_PAIRS + MISC_PAIRS_N) * 8 <= MISC_CK_REGION * 4 &&
                  MISC_CK_REGION + MISC_CK_REGIONS <= MISC_LOSS_ARRIVAL && MISC_LOSS_ARRIVAL < MISC_DET_SAT &&
                  (MISC_DET_SAT + 1) * 4 <= MISC_BYTES,
              "the misc words overlap or leave the block");

// ---- The diagnostics counter buffer (lgm_diag.render_counters: include/lgm_render.h documents the words) --------
// u64 words: 8 aggregate words, one record of 8 per (view, tile), one of 8 per binning workgroup (room for B V
// ceil(N / 512); k_bin uses the first B ceil(V / 3) ceil(N / 512)), one of 4 per backward work item (room for 3 B V T
// + 16 >= round8(B V T) + the checkpoint slots).
// Tile record t = bv T + tile starts at cnt_tile(t); binning record g at cnt_bin0 + CNT_BIN g; backward item i at
// cnt_item0 + CNT_ITEM i (k_render_bwd receives cnt_item0 as an argument).
constexpr int CNT_HEAD = 8, CNT_TILE = 8, CNT_BIN = 8, CNT_ITEM = 4, CNT_BIN_G = 512;
LGM_HD size_t cnt_tile(size_t t) { return CNT_HEAD + CNT_TILE * t; }
LGM_HD size_t cnt_bin0(size_t BV, size_t T) { return cnt_tile(BV * T); }
LGM_HD size_t cnt_item0(size_t BV, size_t T, size_t N) {
    return cnt_bin0(BV, T) + CNT_BIN * BV * ((N + CNT_BIN_G - 1) / CNT_BIN_G);
}
LGM_HD size_t cnt_words(size_t B, size_t V, size_t N, size_t H, size_t W) {
    const size_t T = ((W + BX - 1) / BX) * ((H + BY - 1) / BY);
    return cnt_item0(B * V, T, N) + CNT_ITEM * (3 * B * V * T + 16);
}

// ---- Backward work items and their checkpoints ------------------------------------------------------------------
// Backward work items span 2^ck_shift staged forward chunks (of TILE_PIX entries): 2 chunks for launches of at least
// CK_LONG_TILES tiles, where the many short checkpoint items run at the end of k_render_bwd at about half its slots
// (each workgroup hand-over idles a slot for a few us); one for smaller launches, whose head items already exceed
// one residency round. Pool (12,288 tiles): k_render_bwd 599 -> 588 us and k_render_fwd -6 us (fewer checkpoints);
// one cfg3 scene (1,536 tiles) with 2: bwd 92.7 -> 102.8 us (profiles/r06/ab_bwd_cks).
#ifndef LGM_CK_LONG_TILES
#define LGM_CK_LONG_TILES 4096
#endif
constexpr size_t CK_LONG_TILES = LGM_CK_LONG_TILES;
#ifdef LGM_CK_SHIFT0  // (A/B: one chunk per item at every size)
LGM_HD int ck_shift_for(size_t) { return 0; }
#else
LGM_HD int ck_shift_for(size_t tiles) { return tiles >= CK_LONG_TILES ? 1 : 0; }
#endif

// ---- The workspace --------------------------------------------------------------------------------------------
// Every region starts 256-B aligned. Pair storage `pairs` holds one u64 key (depth_bits << 32 | gaussian id) per
// (Gaussian, tile) pair; after sorting, the tile's u32 ids are written in place at the start of its range.
//   slot mode   (pair_capacity <= 0): tile (bv, t) owns pairs[(bv*T + t) * N, +N): no counting pass, no scan.
//   packed mode (pair_capacity  > 0): tiles are packed by an exclusive scan of exact counts.
// The options change the sizes of ck, cklist and accum only: everything ahead of ck -- all that the inspection
// entry points read -- sits at the same offset whatever the options.
struct Layout {
    size_t gP, gQ, rects, tile_count, tile_start, order, pairs, final_T, n_contrib, wlast, cfin, ck, cklist, nck, cmask,
        accum, lossp, lossw, detmax, misc, total;
    long long cap;
    int ck_region;  // backward checkpoint slots per region (8 regions; the forward shards tiles over them)
    int ck_slots;   // checkpoint slots in all: 8 ck_region (none in deterministic mode)
    bool slot;
    AccumLayout acc;  // the block at `accum`
    // tile_count and misc are adjacent: the binning clears both with one memset of this range
    Region bin_clear() const { return {tile_count, misc + MISC_BYTES - tile_count}; }
};

// options: the call's LGM_RENDER_* bits. Two of them shape the workspace.
// LGM_RENDER_DETERMINISTIC: the gradient accumulators are int64 fixed point (data-scaled units, see render_common.h
// det_norm) instead of fp32 -- integer atomics commute, so the backward's sums do not depend on the order of its work
// items -- and there are no backward checkpoints: one backward work item per tile, so how a tile's walk splits into
// work items cannot depend on which tiles won the shared pool's slot counters (a racing split changes the backward's
// per-chunk partials in their last bits). A per-tile checkpoint quota was measured (profiles/r03/ab_det):
// deterministic k_render_bwd 1950 / 1306 / 955 / 787 / 685 / 650 us at quota 16 / 8 / 4 / 2 / 1 / 0 (float mode
// 626) -- in the fixed-point mode the split costs more than its load balance returns.
// LGM_RENDER_ANTIALIAS: the accumulator block carries the per-view opacity partials and the factors (AccumLayout).
// LGM_RENDER_SH_MASK: it carries the per-view colours, masks and colour partials and the 14-wide row copies.
inline Layout make_layout(int B, int V, int N, int H, int W, long long pair_capacity, int options) {
    const bool det = (options & LGM_RENDER_DETERMINISTIC) != 0, aa = (options & LGM_RENDER_ANTIALIAS) != 0;
    const size_t BV = (size_t)B * V, T = (size_t)((W + BX - 1) / BX) * ((H + BY - 1) / BY), P = (size_t)H * W;
    Layout L;
    L.slot = pair_capacity <= 0;
    L.cap = L.slot ? (long long)(BV * T * (size_t)N) : pair_capacity;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes); return r; };
    L.gP = take(BV * N * 16);  // (x, y, A, B): centre and conic A, B (one 16-B row per (view, Gaussian))
    L.gQ = take(BV * N * 16);  // (C, opacity, tau, depth)
    L.rects = take(BV * N * 8);
    L.tile_count = take(BV * T * 4);
    L.misc = take(MISC_BYTES);  // right after tile_count (bin_clear); its words: MISC_*
    L.tile_start = take((BV * T + 1) * 4);
    L.order = take(T * 4);  // k_sort's centre-first tile table (center_order)
    L.pairs = take((size_t)L.cap * 8);
    L.final_T = take(BV * P * 4);
    L.n_contrib = take(BV * P * 4);
    L.wlast = take(BV * T * 16);  // per tile: the four waves' largest last contributor (forward -> backward)
    L.cfin = take(BV * P * 16);  // per-pixel pre-background colour and depth totals (forward -> backward)
    // backward checkpoints (k_render_fwd -> k_render_bwd), 5 planes of 256 floats each, in 8 regional pools (a
    // region is one eighth of the launch's tiles). k_render_bwd launches one workgroup per slot, and an unused slot's
    // workgroup still pays a dispatch and a counter round trip before it exits: at 2 slots per tile the pool (8 scenes,
    // ~0.53 used per tile) left 18k such workgroups and cost k_render_bwd ~15 us. A region holds min(2 per tile,
    // 0.75 / 2^ck_shift per tile + 257): the 8-scene pool (12,288 tiles, ck_shift 1) 833 per region, one cfg3 scene
    // keeps 2 per tile (384: its central regions need ~1 per tile), BASELINE config 2 keeps 64
    // (profiles/r06/ab_bwd_ckcap, abfull_cap). A full region leaves the rest of a tile's walk to its last
    // checkpointed item (slower, same result).
    L.ck_region = (int)std::min((2 * BV * T + 7) / 8, ((3 * BV * T / 4) >> ck_shift_for(BV * T)) / 8 + 1 + 256);
    L.ck_slots = det ? 0 : 8 * L.ck_region;
    L.ck = take((size_t)L.ck_slots * 5 * TILE_PIX * 4);
    L.cklist = take((size_t)L.ck_slots * 8);
    L.nck = take(BV * T * 4);
    L.cmask = take(BV * P);
    L.acc = accum_layout(B, V, N, det, aa, sh_degree_of(options));
    L.accum = take(L.acc.total);
    L.lossp = take(BV * T * 2 * 4);  // per-tile sums of squared image / alpha residuals (fused loss)
    L.lossw = take(((BV * T + 2047) / 2048) * 16);  // their per-workgroup double2 partials (k_loss_reduce)
    L.detmax = take(64 * 4);  // deterministic mode: max |dL/dpixel| over the seeds, in 64 atomicMax slots
    L.total = o;
    return L;
}

}  // namespace lgm

#undef LGM_HD
