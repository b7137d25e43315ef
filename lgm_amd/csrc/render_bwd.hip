// lgm_amd/csrc/render_bwd.hip -- the gradient pass of the per-tile alpha compositing (SURVEY.md §2.3 rows 7-8 up to
// the per-(view, Gaussian) partials; render_preproc_bwd.hip takes them from there).
//
// k_render_bwd: one 256-thread workgroup per work item (a tile's list head, or the chunks behind one of the forward's
// checkpoints), wavefront w on the 8x8 quadrant (w & 1, w >> 1). The list is walked front to back in 64-entry chunks,
// double-buffered (wave 0 streams chunk c + 1 in by LDS DMA while chunk c is composited). No entry test here: each wave
// compacts a chunk by its quadrant's bit of the masks the forward stored per list position (k_render_fwd's qmask, read
// a chunk ahead). The arithmetic, the moment MFMAs and the flush are described at the kernel.
// k_det_seed_max (deterministic mode) runs ahead of it and shares pixel_seed with it, so both see the same seeds.
#ifdef LGM_BWD_STAMPS  // the diagnostic build's section stamps (render_stage.h), for this source's kernel only
#define LGM_SEC_STAMPS
#endif
#include "render_stage.h"

namespace lgm {
namespace {

// The per-pixel seeds of the backward: dL/dpixel (colour, depth, alpha) after the fused loss's MSE terms and the
// clamp's gradient mask, and the forward's pre-background totals. Shared by k_render_bwd and (deterministic mode)
// k_det_seed_max, so both see the same values.
struct PixelSeed {
    float dp0, dp1, dp2, dpd, dpa;
    float4 cf;
};
template <bool DEPTH, bool LOSS>
__device__ __forceinline__ void pixel_seed(const Dims &d, bool inside, int bv, size_t P, size_t pid, float T_final,
                                           const float *__restrict__ bg, const float4 *__restrict__ cfin,
                                           const float *__restrict__ d_img, const float *__restrict__ d_depth,
                                           const float *__restrict__ d_alpha, const unsigned char *__restrict__ cmask,
                                           PixelSeed &o) {
    float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, dpd = 0.f, dpa = 0.f;
    float4 cf = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) {
        cf = cfin[bv * P + pid];
        if (d_img) {
            const float *di = d_img + (size_t)bv * 3 * P;
            dp0 = di[pid];
            dp1 = di[P + pid];
            dp2 = di[2 * P + pid];
        }
        unsigned cm = 7u;
        float dd = 0.f, da = 0.f;
        if (d.options & LGM_RENDER_CLAMP_IMAGE) cm = cmask[bv * P + pid];
        if (DEPTH) dd = d_depth[bv * P + pid];
        if (d_alpha) da = d_alpha[bv * P + pid];
        if (LOSS) {
            // the MSE seeds (core/models.py:148): dL/dimage += 2 (image - gt) dL/dmse_image / numel, likewise alpha;
            // image recomputed from the forward's totals exactly as the forward formed it
            const float s_img = 2.f * d.d_loss[0] / (float)(3.0 * d.BV * (double)P);
            const float s_a = 2.f * d.d_loss[1] / (float)((double)d.BV * P);
            const float m = d.gt_mask[bv * P + pid];
            const float *gi = d.gt_img + (size_t)bv * 3 * P;
            float c0 = fmaf(T_final, bg[0], cf.x), c1 = fmaf(T_final, bg[1], cf.y), c2 = fmaf(T_final, bg[2], cf.z);
            if (d.options & LGM_RENDER_CLAMP_IMAGE) {
                c0 = fminf(fmaxf(c0, 0.f), 1.f);
                c1 = fminf(fmaxf(c1, 0.f), 1.f);
                c2 = fminf(fmaxf(c2, 0.f), 1.f);
            }
            dp0 += s_img * (c0 - (gi[pid] * m + bg[0] * (1.f - m)));
            dp1 += s_img * (c1 - (gi[P + pid] * m + bg[1] * (1.f - m)));
            dp2 += s_img * (c2 - (gi[2 * P + pid] * m + bg[2] * (1.f - m)));
            dpa = s_a * ((1 - T_final) - m);
        }
        // (the loads are all issued above, in the blocks that only load: each use waits for the one round trip
        // they share -- with the loads next to their uses, the clamp mask and d_alpha were two serial trips)
        if (d.options & LGM_RENDER_CLAMP_IMAGE) {  // torch clamp gradient: passes where 0 <= x <= 1
            dp0 = (cm & 1u) ? dp0 : 0.f;
            dp1 = (cm & 2u) ? dp1 : 0.f;
            dp2 = (cm & 4u) ? dp2 : 0.f;
        }
        if (DEPTH) dpd = dd;
        dpa += da;
    }
    o.dp0 = dp0; o.dp1 = dp1; o.dp2 = dp2; o.dpd = dpd; o.dpa = dpa;
    o.cf = cf;
}

// k_det_seed_max: grid (min(B*V*T, DET_MAX_WGS)), block 256, each workgroup striding over tiles: max |dL/dpixel|
// over every seed of the call -> det_max[DET_SLOTS] (float bits, atomicMax on the non-negative bit pattern, slot
// blockIdx % DET_SLOTS; zeroed by the caller; readers take the max of the slots). One atomic per workgroup, spread
// over 64 words: same-address atomics serialise (one per wave on one word over 12,288 tiles took 564 us).
constexpr int DET_MAX_WGS = 4096;
template <bool DEPTH, bool LOSS>
__global__ __launch_bounds__(256) void k_det_seed_max(Dims d, const float *__restrict__ final_T,
                                                      const float *__restrict__ bg, const float4 *__restrict__ cfin,
                                                      const float *__restrict__ d_img, const float *__restrict__ d_depth,
                                                      const float *__restrict__ d_alpha,
                                                      const unsigned char *__restrict__ cmask,
                                                      unsigned *__restrict__ det_max, unsigned *__restrict__ det_sat) {
    __shared__ unsigned s_m[4];
    // the call's overflow count starts at zero here, ahead of every k_render_bwd flush of the call (a repeated
    // backward of the same forward, LGM_RENDER_BACKWARD_AGAIN, must not inherit an earlier backward's count)
    if (blockIdx.x == 0 && threadIdx.x == 0) *det_sat = 0u;
    int lx, ly;
    tile_pixel(threadIdx.x, lx, ly);
    const size_t P = (size_t)d.H * d.W;
    float m = 0.f;
    for (int tile = blockIdx.x; tile < d.BV * d.T; tile += gridDim.x) {
        const int bv = tile / d.T, t = tile - bv * d.T;
        const int px = (t % d.gx) * BX + lx, py = (t / d.gx) * BY + ly;
        const bool inside = px < d.W && py < d.H;
        const size_t pid = inside ? (size_t)d.W * py + px : 0;
        PixelSeed sd;
        pixel_seed<DEPTH, LOSS>(d, inside, bv, P, pid, inside ? final_T[bv * P + pid] : 0.f, bg, cfin, d_img, d_depth,
                                d_alpha, cmask, sd);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(sd.dp0), fabsf(sd.dp1)),
                           fmaxf(fmaxf(fabsf(sd.dp2), fabsf(sd.dpd)), fabsf(sd.dpa))));
    }
    unsigned mb = __float_as_uint(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, o, 64));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mb;
    __syncthreads();
    if (threadIdx.x == 0) {
        mb = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
        if (mb) atomicMax(det_max + blockIdx.x % DET_SLOTS, mb);
    }
}

// k_render_bwd: grid (B*V*T + CK slots), block 256. DEPTH: an upstream depth gradient is present (LGM passes none).
//
// The gradient pass walks each tile's list FRONT TO BACK, the forward's order. Upstream's reverse recurrence (suffix
// colour accumulators) is replaced by the equivalent prefix form: with T_i the transmittance in front of entry i,
// D_i = sum_{j <= i} alpha_j T_j (c_j . dL/dC) and the forward's per-pixel totals Dfin = C . dL/dC, T_final,
//     dL/dalpha_i = T_i (c_i . dL/dC) - (Dfin - K - D_i) / (1 - alpha_i),    K = (dL/dA - bg . dL/dC) T_final,
// so the per-pixel state is just (T, D). That state is what the forward checkpoints at each 256-entry chunk
// boundary it crosses (k_render_fwd: T and the prefix colour/depth sums; D = prefix . dL/dC), so the backward work
// item is one CHUNK, not one tile: workgroup g < B*V*T takes chunk 0 of LPT tile g, workgroup B*V*T + s takes the
// chunk of checkpoint slot s (cklist), and runs to the next checkpoint (or the tile's end if the pool ran out).
// Long tiles no longer bound the launch.
//
// Per-entry gradient sums over a wave's 64 pixels are pixel moments on the MFMA: w = G dL/dG and u = alpha T give
// sum_p w f(p) for f in {1, x, y, x^2, xy, y^2} (tile-centred pixel coordinates; the mean2D and conic partials
// follow from these and the Gaussian centre) and sum_p u dL/dC_c(p): a [features x pixels] . [pixels x entries]
// product: the wave walks its list MB = 8 entries per step (list padded with the sentinel), writes their w
// (columns 0..MB-1) and u (columns MB..) to a per-wave LDS image and sums them with v_mfma_f32_16x16x32_bf16 (the
// geometric features are exact in bf16; w, u and dL/dC as hi + lo bf16 pairs, ~2^-16 relative per product). Moments are combined over the tile's four waves in LDS, turned into gradient partials per
// entry and flushed once per (chunk, entry) to the per-view accumulators.
// Occupancy: at least 4 waves per SIMD for the register allocation (<= 128 VGPRs; the 64-entry chunks' LDS admits 4
// workgroups per CU); 2 for the depth-gradient instantiation, which LGM never runs.
// AA: LGM_RENDER_ANTIALIAS -- the opacity partial is flushed per (view, Gaussian) (accum_aa_elem0) instead of into the
// scene's record: k_preproc_bwd needs dL/do^ of each view. Compile-time, so the other instantiations are unchanged.
// SH: LGM_RENDER_SH_MASK -- `gauss` is the per-view colour buffer (stage_dma) and the colour partials are flushed per
// (view, Gaussian) to Dims::sh_part (k_sh_bwd needs dL/dcolour of each view), with the per-view flush bound.
// Compile-time likewise.
template <bool DEPTH, bool LOSS, bool DET, bool AA = false, bool SH = false>  // DET: LGM_RENDER_DETERMINISTIC (int64 fixed-point flush)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DEPTH ? 2 : 4))) void k_render_bwd(
    Dims d, long long slot_stride, const int *__restrict__ tile_start,
    const int *__restrict__ tile_count, const unsigned long long *__restrict__ pairs, const float4 *__restrict__ gP,
    const float4 *__restrict__ gQ, const float *__restrict__ gauss, const float *__restrict__ bg,
    const float *__restrict__ final_T, const int *__restrict__ n_contrib, const int *__restrict__ wlast_fwd,
    const float4 *__restrict__ cfin, const float *__restrict__ ck, const int2 *__restrict__ cklist,
    const int *__restrict__ nck,
    const unsigned *__restrict__ ckctr, int ck_region, const float *__restrict__ d_img,
    const float *__restrict__ d_depth, const float *__restrict__ d_alpha, const unsigned char *__restrict__ cmask,
    float *__restrict__ accum, const unsigned *__restrict__ det_max, unsigned *__restrict__ det_sat,
    long long item_stamps) {
    constexpr int NV = DEPTH ? NACC : NACC - 1;  // partials per (pixel, Gaussian): mean2D(2) conic(3) op rgb(3) [depth]
    // entries per staged chunk; LDS row stride of the moment slots: LS = 4 (mod 32) puts the rows a moment store
    // writes at once (4 qk + rr, qk = 0, 1 in a 32-lane store group: rows rr and rr + 4) 16 banks apart, so a batch's
    // 8 consecutive entry columns land on distinct banks (ds_write_b32 banks are (a / 4) mod 32)
    // (the depth-gradient instantiation keeps stride 65 and one shared junk row: its larger slots would not leave
    // room for a fourth workgroup per CU otherwise)
    constexpr int CH = BWD_CHUNK, LS = CH + 4;
    __shared__ StageBwd S;
    // per-wave moment slots (plain stores: each wave writes an entry's moments once; no LDS atomics), combined over
    // the entry's quadrant waves after the entries loop. Rows 0..5 geometric (w columns), then one row per colour
    // [+ depth] channel (u columns): the A operand holds each channel's dL/dpixel hi and lo bf16 parts in adjacent
    // rows (6 + 2c, 7 + 2c: one lane's accumulator pair), so a lane adds the pair before storing and the slot keeps
    // NC colour rows, not 2 NC. The MFMA results a lane does not keep go to a junk word after the rows (JB + lane +
    // the batch column; never read), so the stores need no exec-masked branches.
    constexpr int NC = DEPTH ? 4 : 3, NROW = 6 + NC, NROWA = 6 + 2 * NC;
    constexpr int JB = (LS * NROW + 3) & ~3;
    constexpr int SLOT = JB + 64 + CH + 4;        // junk words JB + lane + column; 16-B aligned slots
    constexpr int ZSLOT = JB;                     // the part zeroed per chunk (the junk words are never read)
    __shared__ __attribute__((aligned(16))) float sAccW[4][SLOT];
    __shared__ __attribute__((aligned(16))) float sWU[4][16 * WU_LD];  // read as float4: keep 16-B aligned
    // the chunk's gradient partials (rows q * LS + j; a needle's conic partials in rows NV .. NV + 2 for the fp64
    // flush) and its Gaussian ids, written by the conversion and read by the flush. Their own buffer (not a dead WU
    // image) lets a wave start the next chunk's compaction and entries right after its share of the flush, while
    // other waves still flush: one barrier less per chunk
    __shared__ __attribute__((aligned(16))) float sO[(NV + 3) * LS];
    __shared__ unsigned sId[CH];
    __shared__ int s_ndl[2];  // chunk parity: the chunk holds a needle-like record (conic partials to the fp64 block)

    // ---- work item: (tile, chunk c, checkpoint slot)
    const int M = d.BV * d.T, Mp = round8(M);  // head items, then the checkpoint items (none in deterministic mode)
    int tile, c = 0, slot = -1;
    if ((int)blockIdx.x < M) {
        tile = xcd_item(blockIdx.x, M);
    } else {
        if ((int)blockIdx.x < Mp) return;  // padding: the checkpoint items start at a multiple of 8
        slot = (int)blockIdx.x - Mp;
        if ((int)(slot >> 3) >= (int)ckctr[slot & 7]) return;  // an unused slot of region slot & 7 (workgroup-uniform)
        const int2 e = cklist[slot];
        if (e.x < 0) return;  // reserved, never written
        tile = e.x;
        c = e.y;
    }
    const int bv = tile / d.T, t = tile - bv * d.T, b = bv / d.V;
    const int tx0 = (t % d.gx) * BX, ty0 = (t / d.gx) * BY;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int lx, ly;
    tile_pixel(tid, lx, ly);
    const int px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < d.W && py < d.H;
    const float pfx = (float)px, pfy = (float)py;
    long long base;
    int n;
    tile_range(tile, slot_stride, tile_start, tile_count, base, n);
    const unsigned *ids = reinterpret_cast<const unsigned *>(pairs + base);
    // the first chunk's ids and LDS DMA go out before the per-pixel state loads (bounded by the list length n, a
    // superset of [s0, s1): rows past s1 are staged but never listed or flushed), so their two dependent memory
    // round trips overlap the pixel loads instead of following them
    const bool stager = w == 0;  // (wave 3 staging, with waves 0-2 flushing and never waiting for their atomics, measured
                                 // slower: pool k_render_bwd 608 -> 620 us, profiles/r06/ab_bwd_w3)
    const int s0e = (c * TILE_PIX) << d.ck_shift;
    unsigned id_cur = stager && s0e + lane < n ? ids[s0e + lane] : 0u;
    if (stager && s0e + lane < n) stage_dma<SH>(S.buf[0], 0, id_cur, (size_t)bv * d.N, b, d.N, gP, gQ, gauss);
    unsigned id_next = stager && s0e + BWD_CHUNK + lane < n ? ids[s0e + BWD_CHUNK + lane] : 0u;
    const size_t P = (size_t)d.H * d.W;
    const size_t pid = inside ? (size_t)d.W * py + px : 0;
    const float T_final = inside ? final_T[bv * P + pid] : 0.f;
    const int last = inside ? n_contrib[bv * P + pid] : 0;
    // the checkpoint's loads go out before the seeds' (one shared round trip instead of a third serial one)
    float ckT = 1.0f, ck1 = 0.f, ck2 = 0.f, ck3 = 0.f, ck4 = 0.f;
    if (slot >= 0) {
        const float *cp = ck + (size_t)slot * 5 * TILE_PIX;
        ckT = cp[tid];
        ck1 = cp[TILE_PIX + tid];
        ck2 = cp[2 * TILE_PIX + tid];
        ck3 = cp[3 * TILE_PIX + tid];
        if (DEPTH) ck4 = cp[4 * TILE_PIX + tid];
    }
    PixelSeed sd;
    pixel_seed<DEPTH, LOSS>(d, inside, bv, P, pid, T_final, bg, cfin, d_img, d_depth, d_alpha, cmask, sd);
    const float dp0 = sd.dp0, dp1 = sd.dp1, dp2 = sd.dp2, dpd = sd.dpd, dpa = sd.dpa;
    const float4 cf = sd.cf;
    // per-pixel state entering the chunk: the forward's checkpoint (or the list head)
    float Tr = 1.0f, Dup = 0.f;
    if (slot >= 0) {
        Tr = ckT;
        Dup = fmaf(ck1, dp0, fmaf(ck2, dp1, ck3 * dp2));
        if (DEPTH) Dup = fmaf(ck4, dpd, Dup);
    }
    init_sentinel(S);  // (published by the first barrier of the chunk loop)
    // the forward's per-wave maxima of the last contributors: positions >= wlast touch no pixel of this wave, and
    // entries behind every pixel's last contributor are never visited
    const int4 wl4 = reinterpret_cast<const int4 *>(wlast_fwd)[tile];
    const int wlast = w == 0 ? wl4.x : w == 1 ? wl4.y : w == 2 ? wl4.z : wl4.w;
    const int nlist = min(n, max(max(wl4.x, wl4.y), max(wl4.z, wl4.w)));
    const int s0 = (c * TILE_PIX) << d.ck_shift;
    if (s0 >= nlist) {  // workgroup-uniform (the early DMA must land before the workgroup retires)
        vm_wait();
        return;
    }
    const int s1 = (c + 1 <= nck[tile]) ? min(nlist, s0 + (TILE_PIX << d.ck_shift)) : nlist;
    if (s0 >= s1) {  // (nothing to do; likewise)
        vm_wait();
        return;
    }
    // Quadrant masks from the forward (k_render_fwd's qmask: byte 4 n + p of the tile's pair range for list position
    // p), one chunk ahead in a register like the ids. Only positions < min(s1, wlast) are loaded: all of them lie in
    // chunks the forward staged (wlast is a position it composited), so every byte read was written by this forward.
    // Why the forward's verdict serves: a pixel took a contribution only from an entry the forward listed for the
    // pixel's quadrant, so the masks cover every (entry, quadrant) with a non-zero gradient; an entry a wave does
    // not list adds exact zeros (its moment slot stays zeroed), and each listed entry's moments sit in an MFMA column
    // of their own, whatever else shares the batch. The float-mode gradients therefore keep their values up to the
    // order of the atomics, and the deterministic ones are bitwise those of the backward's own retest.
    const unsigned char *qmask = reinterpret_cast<const unsigned char *>(pairs + base) + 4 * (size_t)n;
    const int qend = min(s1, wlast);  // (per wave)
    unsigned qm = s0 + lane < qend ? qmask[(unsigned)(s0 + lane)] : 0u;
    const unsigned long long t_item = d.counters ? __builtin_amdgcn_s_memrealtime() : 0ull;
    // section cycles of this wave (LGM_BWD_STAMPS build only; counters [0..7], scripts/diag_bwd_stamps.py):
    // [0] prologue, [1] the lane's quadrant verdict, [2] rest of the chunk head (compaction, next DMA issue), [3] entries
    // loop, [4] the post-entries barrier + moments -> partials, [5] the DMA wait (vmcnt 0), [6] the pre-flush
    // barrier, [7] the gradient atomics
    SEC_DECL(sec, 8);
    SEC_T(ts_item);
    const float bg_dot = bg[0] * dp0 + bg[1] * dp1 + bg[2] * dp2;
    float cdpf = fmaf(cf.x, dp0, fmaf(cf.y, dp1, cf.z * dp2));
    if (DEPTH) cdpf = fmaf(cf.w, dpd, cdpf);
    const float DK = cdpf - (dpa - bg_dot) * T_final;  // Dfin - K
    float Erem = DK - Dup;  // Dfin - K - D_i, kept directly (one subtraction less per entry)
    const float ddelx_dx = 0.5f * d.W, ddely_dy = 0.5f * d.H;
    const int det_s = DET ? det_seed_shift(det_max) : 0;
    // per-flush bounds of the per-view and the per-scene records (render_common.h det_flush_limit_log2)
    const float det_lim_v = ldexpf(1.f, d.det_lim_log2 ? d.det_lim_log2 : det_flush_limit_log2(d.V, d.T, false));
    const float det_lim_s = ldexpf(1.f, d.det_lim_log2 ? d.det_lim_log2 : det_flush_limit_log2(d.V, d.T, true));
    const size_t gbase = (size_t)bv * d.N;
    // MFMA operands: A (features) lane (ql, qk) holds feature ql of wave pixels 32 t + 8 qk + j, j = 0..7
    const int ql = lane & 15, qk = lane >> 4;
    const float cxT = (float)tx0 + 7.5f, cyT = (float)ty0 + 7.5f;
    // the slot offset of this lane's r-th stored value: w columns (ql < MB) keep D rows 4 qk + r <= 5 (the geometric
    // moments); u columns keep the sums of the accumulator pairs (r = 0: D rows 4 qk, 4 qk + 1; r = 1: 4 qk + 2, + 3)
    // that are a colour channel's hi / lo rows 6 + 2c, 7 + 2c -> slot row 6 + c. Everything else: the junk word.
    int mrow[4];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        int row = -1;
        if (ql < MB) {
            if (4 * qk + rr <= 5) row = 4 * qk + rr;
        } else if (rr < 2) {
            const int a = 4 * qk + 2 * rr;  // the pair's first D row
            if (a >= 6 && a < NROWA) row = 6 + (a - 6) / 2;
        }
        mrow[rr] = row >= 0 ? row * LS : JB + lane;
    }
    float *myAcc = sAccW[w];
    float *myWU = sWU[w];
    const int lane_x = lane ^ 8;  // this lane's pixel in the swizzled image columns (wu_swz)
    myWU[lane] = dp0;
    myWU[64 + lane] = dp1;
    myWU[128 + lane] = dp2;
    myWU[192 + lane] = dpd;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // A operand: lane (ql, qk) holds row ql at the wave pixels p = 32 t2 + 8 qk + j, j = 0..7, i.e. tile-centred
    // fx = fx0 + j and fy = fy0 + 4 t2 + qk. Rows 0..5, the geometric features, are a + b j + c j^2 with per-lane
    // coefficients, exact in bf16 (small integers and halves); rows 6..6+NC-1 are dL/dpixel rounded to bf16 and rows
    // 6+NC.. the remainders, so A . (B_hi + B_lo) -- two MFMAs -- carries every product but lo x lo (~2^-16).
    bf16x8 Ah[2];
    {
        const float fx0 = (float)((w & 1) << 3) - 7.5f, fy0 = (float)((w >> 1) << 3) - 7.5f;
        const bool isdp = ql >= 6 && ql < NROWA, islo = isdp && ((ql - 6) & 1);
        const int qd = isdp ? (ql - 6) >> 1 : 0;  // the dL/dpixel channel of rows 6..NROWA-1 (hi, lo per channel)
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            const float fy = fy0 + (float)(4 * t2 + qk);
            const float ca = ql == 0 ? 1.f : ql == 1 ? fx0 : ql == 2 ? fy : ql == 3 ? fx0 * fx0
                           : ql == 4 ? fx0 * fy : ql == 5 ? fy * fy : 0.f;
            const float cb = ql == 1 ? 1.f : ql == 3 ? 2.f * fx0 : ql == 4 ? fy : 0.f;
            const float cc2 = ql == 3 ? 1.f : 0.f;
            const float4 *src = reinterpret_cast<const float4 *>(myWU + qd * 64 + 32 * t2 + 8 * qk);
            const float4 d0 = src[0], d1 = src[1];
            const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float geo = fmaf(fmaf(cc2, (float)j, cb), (float)j, ca);
                const __bf16 dh = (__bf16)dv[j];
                const float dlo = dv[j] - (float)dh;
                Ah[t2][j] = ql <= 5 ? (__bf16)geo : !isdp ? (__bf16)0.f : islo ? (__bf16)dlo : dh;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int myj = 0;  // the chunk row of this lane's batch column (ql & 7)
    // Moment precision. On needle-like footprints (conic condition > ~1e3) the cov2D inverse amplifies any rounding
    // of the conic gradients into their scale / rotation gradients. A two-term split with a TRUNCATED hi part biases
    // every product's rounding one way (~2^-16, coherent over a tile's pixels): at 512^2 it left mean / scale / rot
    // at ~2x the fp32 oracle's own error vs fp64. A round-to-nearest hi part (same instruction count: <= 2^-17 per
    // product, unbiased) and an exact three-term split (+2 MFMAs and +40 VALU per 8-entry batch, k_render_bwd +7 %
    // on the pool) both put them at 0.5-0.8x the oracle's (profiles/r03/diag_float_spread), so the two-term
    // round-to-nearest split is used in both modes.
    // B operand of the current batch: lane (ql, qk) takes column ql at pixels 32 t + 8 qk + j (two 16-B reads per t)
    auto read_batch = [&](float (&xs)[2][8]) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            const float *row = myWU + ql * WU_LD;
            const int p0 = 32 * t2 + 8 * qk, sw = wu_swz(ql);
            const float4 x0 = *reinterpret_cast<const float4 *>(row + (p0 ^ sw));
            const float4 x1 = *reinterpret_cast<const float4 *>(row + ((p0 + 4) ^ sw));
            xs[t2][0] = x0.x; xs[t2][1] = x0.y; xs[t2][2] = x0.z; xs[t2][3] = x0.w;
            xs[t2][4] = x1.x; xs[t2][5] = x1.y; xs[t2][6] = x1.z; xs[t2][7] = x1.w;
        }
    };
    // split hi + lo, the moment MFMAs, and the lane's (at most 4) live results into this wave's slots
    auto mfma_batch = [&](const float (&xs)[2][8], int col) {
        f32x4 a2[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            // hi = x rounded to bf16 (|x - hi| <= 2^-9 |x|), lo = the exact remainder rounded: <= 2^-17 |x| per
            // product (per pair: two packed conversions, the two hi halves back to fp32 by a shift and a mask, two
            // subtractions)
            bf16x8 bh, bl;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const bf16x2v hp = __builtin_convertvector((f32x2v){xs[t2][j], xs[t2][j + 1]}, bf16x2v);
                const unsigned hb = __builtin_bit_cast(unsigned, hp);
                const float h0 = __builtin_bit_cast(float, hb << 16), h1 = __builtin_bit_cast(float, hb & 0xffff0000u);
                const bf16x2v lp = __builtin_convertvector((f32x2v){xs[t2][j] - h0, xs[t2][j + 1] - h1}, bf16x2v);
                bh[j] = hp[0];
                bh[j + 1] = hp[1];
                bl[j] = lp[0];
                bl[j + 1] = lp[1];
            }
            f32x4 cacc = {0.f, 0.f, 0.f, 0.f};
            cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[t2], bh, cacc, 0, 0, 0);
            cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[t2], bl, cacc, 0, 0, 0);
            a2[t2] = cacc;
        }
        const f32x4 acc = a2[0] + a2[1];
        // D[row = 4 qk + r][col = ql]: moments 0..5 in the w columns; in the u columns each colour channel's hi and lo
        // rows are one lane's pair (r, r + 1), added here (the same sum the conversion formed before: bitwise equal);
        // each lane stores its values at per-lane offsets fixed for the kernel (mrow; dead ones to its junk word)
        const bool ucol = ql >= MB;
        const float v0 = ucol ? acc[0] + acc[1] : acc[0], v1 = ucol ? acc[2] + acc[3] : acc[1];
        myAcc[mrow[0] + col] = v0;  // (sentinel columns: row CH, all zero)
        myAcc[mrow[1] + col] = v1;
        myAcc[mrow[2] + col] = acc[2];
        myAcc[mrow[3] + col] = acc[3];
    };

    // Staging pipeline (front to back over [s0, s1)): chunk b0 + CH streams into the other buffer by LDS DMA
    // during chunk b0's compositing and is complete (vm_wait_all) before chunk b0's gradient atomics are issued,
    // so no staging load queues behind them; the sorted ids run one chunk further ahead in a register.
    // Two barriers per chunk: P (after the entries loop: every wave's moments are in its slot) and F (before the
    // flush: the partials are in sO, and the stager's next chunk has landed). The chunk-top barrier of rounds 1-5 is
    // gone: a wave goes from its share of chunk c's flush straight into chunk c + 1's compaction and entries
    // while the others still flush. That is safe because nothing the flush reads is written before the next P:
    // the partials and ids live in sO / sId (rewritten only by the next conversion, after P), the needle flag has one
    // word per chunk parity, and the next chunk's DMA overwrites the buffer of chunk c - 1, whose last reader (the
    // conversion of c - 1) finished before F of c - 1. Each wave zeroes its own moment slot at the top of a chunk,
    // after the conversion that read it (before F).
    vm_wait();
    __syncthreads();  // the first chunk's rows and the sentinel rows
    int cur = 0;
    SEC_T(ts_loop);
    SEC_ADD(sec[0], ts_item, ts_loop);  // prologue: pixel state, seeds, MFMA operands, first staging
    for (int b0 = s0, ci = 0; b0 < s1; b0 += CH, cur ^= 1, ci++) {
        SEC_T(ts_c0b);
        auto &B = S.buf[cur];
        // one row per lane: every wave takes its OWN quadrant's bit of the forward's mask for each of the CH entries
        // (qm, loaded a chunk ahead) and the ballot is its compaction mask (no shared mask, no barrier, and neither the
        // rows' LDS reads, the two IEEE divisions nor the ellipse test the retest cost at the top of every chunk)
        if (stager) reinterpret_cast<unsigned *>(&B.R[lane])[3] = id_cur;  // for the gradient flush
        if (!DET && tid == 0) s_ndl[ci & 1] = 0;  // (published by P; the flush of chunk ci - 2 read it before P of ci - 1)
        {  // every wave zeroes its own slot (an entry it skips, or never lists, adds nothing): wave-private, so the
           // entries loop follows the compaction without a barrier (with the conversion over three waves below:
           // pool k_render_bwd 642 -> 635 us, bitwise equal, profiles/r04/ab_bwd_conv)
            float4 *z = reinterpret_cast<float4 *>(myAcc);
            for (int q = lane; q < ZSLOT / 4; q += 64) z[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        int cnt;
        SEC_VAR(sec1_chunk);
        {
            SEC_T(ts_c0p);
            bool hit = (qm >> w) & 1u;  // (0 beyond min(s1, wlast): never loaded)
            qm = b0 + CH + lane < qend ? qmask[(unsigned)(b0 + CH + lane)] : 0u;  // the next chunk's
#ifdef LGM_BWD_STAMPS
            int hit_v = hit;
            asm volatile("" : "+v"(hit_v));  // (the lane's verdict exists before the stamp)
            hit = hit_v != 0;
#endif
            SEC_T(ts_c0q);
            SEC_ADD(sec1_chunk, ts_c0p, ts_c0q);
            SEC_ADD(sec[1], ts_c0p, ts_c0q);  // the lane's quadrant verdict alone ([2] keeps the rest of the head)
            const unsigned long long bal = __ballot(hit);
            if (hit) S.list[w][__popcll(bal & lanemask_lt(lane))] = (unsigned short)lane;
            cnt = __popcll(bal);
            constexpr int PAD = (int)(sizeof(S.list[0]) / sizeof(S.list[0][0])) - CH;
            if (lane < PAD) S.list[w][cnt + lane] = (unsigned short)CH;
        }
        if (stager && b0 + lane + CH < s1) stage_dma<SH>(S.buf[cur ^ 1], 0, id_next, gbase, b, d.N, gP, gQ, gauss);
        id_cur = id_next;
        id_next = stager && b0 + lane + 2 * CH < s1 ? ids[b0 + lane + 2 * CH] : 0u;
        static_assert(MB == 8, "one batch = two 4-entry list words");
        SEC_T(ts_c1);
        SEC_ADD(sec[2], ts_c0b, ts_c1);  // chunk head: slot zeroing, compaction, next DMA issue ...
        SEC_SUB(sec[2], sec1_chunk);     // ... without the quadrant verdict, which [1] holds
        const int lastrel = last - b0;  // this pixel's last contributor, relative to the chunk
        uint2 lraw[2];  // the next step's list words, read one step ahead
        list_raw<MB>(S, w, 0, lraw);
        // one batch: MB list entries evaluated per pixel, their w and u written to this wave's WU image
        auto eval_batch = [&](int kk) {
            int jj8[MB];
            list_decode<MB>(lraw, jj8);
            myj = S.list[w][kk + (lane & (MB - 1))];  // the entry of this lane's batch column
            list_raw<MB>(S, w, kk + MB, lraw);        // in bounds: the list rows hold kRows + MB words
#pragma unroll
            for (int h = 0; h < 2; h++) {
                // a batch with <= 4 listed entries (often a chunk's last) skips its second half, all padding: the
                // stale w / u columns it leaves multiply into the sentinel column CH only (pool k_render_bwd 634 ->
                // 614 us, bitwise equal: profiles/r04/ab_session_f)
                if (h == 1 && kk + 4 >= cnt) break;  // (wave-uniform)
                float al[4], Gw[4];
                float4 cc[4], Pv[4], Qv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {  // the LDS reads first, one wait (see k_render_fwd)
                    const int j = jj8[4 * h + u];
                    Pv[u] = B.P[j];
                    Qv[u] = B.Q[j];
                    const float4 Rj = B.R[j];
                    cc[u] = make_float4(Rj.x, Rj.y, Rj.z, 0.f);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool before_last = jj8[4 * h + u] < lastrel;  // position b0 + jj < last
                    const float4 Pj = Pv[u], Q = Qv[u];
                    cc[u].w = Q.w;
                    const float dx = Pj.x - pfx, dy = Pj.y - pfy;
                    const float lp = fmaf(Q.x * dy, dy, fmaf(fmaf(Pj.w, dy, Pj.z * dx), dx, Q.y));  // as k_render_fwd
                    const float e = __builtin_amdgcn_exp2f(lp);  // opacity G
                    const bool ok = before_last && lp <= Q.y && e >= 1.0f / 255.0f;
                    Gw[u] = ok ? e : 0.f;  // dL/dG = opacity dL/dalpha (0: the entry adds nothing here)
                    al[u] = alpha_cap(Gw[u]);  // (= ok ? alpha_cap(e) : 0, one select less: alpha_cap(0) = 0)
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {  // the prefix recurrences in list order
                    const float alpha = al[u];
                    const float4 cu = cc[u];
                    float cdp = fmaf(cu.x, dp0, fmaf(cu.y, dp1, cu.z * dp2));
                    if (DEPTH) cdp = fmaf(cu.w, dpd, cdp);
                    const float aT = alpha * Tr;
                    const float om = 1.f - alpha;
                    const float inv = __builtin_amdgcn_rcpf(om);  // 1 / (1 - alpha), 1 ulp
                    Erem = fmaf(-aT, cdp, Erem);
                    const float dL_dalpha = fmaf(Tr, cdp, -Erem * inv);
                    Tr = Tr - aT;
                    // w (columns 0..7) and u (8..15), pixel lane at lane ^ wu_swz(column): the swizzled
                    // columns 4..7 and 8..11 are h = 1 for w, h = 0 for u
                    myWU[(4 * h + u) * WU_LD + (h == 1 ? lane_x : lane)] = Gw[u] * dL_dalpha;
                    myWU[(MB + 4 * h + u) * WU_LD + (h == 0 ? lane_x : lane)] = aT;  // (dchannel_dcolor)
                }
            }
        };
        // software-pipelined: batch k's B operand is read from the WU image BEFORE batch k + 1 overwrites it (a
        // wave's LDS operations complete in issue order), so batch k's LDS round trip and moment MFMAs overlap batch
        // k + 1's evaluations instead of stalling the wave between batches
        if (cnt > 0) {
            eval_batch(0);
            for (int kk = 0; kk < cnt; kk += MB) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                float xs[2][8];
                read_batch(xs);
                const int col = myj;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the reads issue before the next writes)
                if (kk + MB < cnt) eval_batch(kk + MB);
                mfma_batch(xs, col);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        SEC_T(ts_c2);
        SEC_ADD(sec[3], ts_c1, ts_c2);  // the entries loop (evaluation, moments)
        __syncthreads();
        // moments -> gradient partials, an entry's three groups on three waves at once (thread 64 g + j, entry j):
        // g = 0 mean2D + opacity (moment rows 0..2) and the entry's Gaussian id, g = 1 conic (rows 0..5; a needle's go
        // to rows NV..NV+2 for the fp64 flush), g = 2 colour [+ depth] (the summed hi + lo rows). The partials go to
        // sO, rows q * LS + j.
        float *o = sO;
        if (w < 3 && b0 + lane < s1) {  // (w: wave-uniform)
            const int j = lane;
            auto msum = [&](int row) {
                float v = 0.f;
#pragma unroll
                for (int ww = 0; ww < 4; ww++) v += sAccW[ww][row * LS + j];
                return v;
            };
            if (w == 2) {
#pragma unroll
                for (int qq = 6; qq < NV; qq++) {
                    float v = 0.f;
#pragma unroll
                    for (int ww = 0; ww < 4; ww++) v += sAccW[ww][qq * LS + j];  // (each term: that wave's hi + lo)
                    o[qq * LS + j] = DET ? ldexpf(v, det_s) : v;
                }
            } else {
                const float4 Pj = B.P[j];
                const float4 Qj = B.Q[j];
                float cA, cB, cC, op;  // the upstream conic and opacity
                rec_conic(Pj, Qj, cA, cB, cC, op);
                const float xg = Pj.x - cxT, yg = Pj.y - cyT;
                const float q0 = msum(0), q1 = msum(1), q2 = msum(2);
                DetNorm nm;
                if (DET) nm = det_norm(Pj.z, Pj.w, Qj.x, d.W, d.H);
                if (w == 0) {
                    sId[j] = reinterpret_cast<const unsigned *>(&B.R[j])[3];
                    const float Sx = fmaf(xg, q0, -q1), Sy = fmaf(yg, q0, -q2);
                    float p0 = -ddelx_dx * (cA * Sx + cB * Sy);
                    float p1 = -ddely_dy * (cC * Sy + cB * Sx);
                    float p5 = op > 0.f ? q0 / op : 0.f;
                    if (DET) {
                        p0 = ldexpf(p0, det_s + nm.k[0]);
                        p1 = ldexpf(p1, det_s + nm.k[1]);
                        p5 = ldexpf(p5, det_s + (AA ? det_norm_opacity(Qj.y) : 0));
                    }
                    o[0 * LS + j] = p0;
                    o[1 * LS + j] = p1;
                    o[5 * LS + j] = p5;
                } else {
                    const float q3 = msum(3), q4 = msum(4), q5 = msum(5);
                    const float Sxx = fmaf(xg, fmaf(xg, q0, -2.f * q1), q3);
                    const float Sxy = fmaf(xg, fmaf(yg, q0, -q2), fmaf(-yg, q1, q4));
                    const float Syy = fmaf(yg, fmaf(yg, q0, -2.f * q2), q5);
                    float pc[3] = {-0.5f * Sxx, -0.5f * Sxy, -0.5f * Syy};
                    if (DET) {
#pragma unroll
                        for (int qq = 0; qq < 3; qq++) pc[qq] = ldexpf(pc[qq], det_s + nm.k[2 + qq]);
                    }
                    const bool ndl = !DET && rec_needle(Pj.z, Pj.w, Qj.x);
#pragma unroll
                    for (int qq = 0; qq < 3; qq++) {
                        o[(2 + qq) * LS + j] = ndl ? 0.f : pc[qq];
                        if (!DET) o[(NV + qq) * LS + j] = ndl ? pc[qq] : 0.f;
                    }
                    if (ndl) s_ndl[ci & 1] = 1;  // (benign race: every writer stores 1)
                }
            }
        }
        SEC_T(ts_c3);
        SEC_ADD(sec[4], ts_c2, ts_c3);  // barrier + moments -> partials
        // the next chunk's DMA and ids have landed before the atomics below go out (they cannot delay it)
        vm_wait();
        SEC_T(ts_c3a);
        SEC_ADD(sec[5], ts_c3, ts_c3a);  // DMA wait (and any earlier outstanding vector-memory op of this wave)
        __syncthreads();
        SEC_T(ts_c3b);
        SEC_ADD(sec[6], ts_c3a, ts_c3b);  // pre-flush barrier
        // flush: lane -> (entry, value) flat, so one global-atomic wave-instruction covers ~6 contiguous 40-B
        // gradient records instead of 64 scattered rows
        constexpr int FT = 256, FQ = NACC;  // flushing threads; items per entry in the lane mapping
        {
        int ft = tid;
        // the lane's (entry, partial) indices recomputed per chunk: hoisted out of the chunk loop, their 64-bit
        // per-scene accumulator offsets were spilled, and each reload's vmcnt(0) waited for this flush's earlier atomics
        asm volatile("" : "+v"(ft));
#pragma unroll
        for (int it = 0; it < (CH * FQ + FT - 1) / FT; it++) {
            const int f = it * FT + ft;
            const int j = f / FQ, q = f - j * FQ;
            if (q < NV && j < CH && b0 + j < s1) {
                const float a = o[q * LS + j];
                const unsigned gid = sId[j];
                // NACC order: mean2D 0..1 and conic 2..4 (per view), opacity 5 and colour 6..8 (per scene: ks is the
                // scene record's first element), depth 9
                const size_t k = gbase + gid, ks = accum_scene_elem(d.BV, d.N, b, gid, 0);
                size_t ai = q < 5 ? accum_view_elem(k, q) : q < 9 ? ks + (q - 5) : accum_view_elem(k, 5);
                if (AA && q == 5) ai = accum_aa_elem0(d.B, d.V, d.N, DET) + gbase + gid;  // per view, not per scene
                // (SH) the colour partials go to the view's own record in Dims::sh_part, outside `accum`'s main region
                const bool shq = SH && q >= 6 && q < 9;
                if (shq) ai = (gbase + gid) * 3 + (q - 6);
                if (a != 0.f) {
                    if (DET) {  // integer adds commute: order-independent sums (a is already in fixed-point units)
                        // (a per-view record takes at most T flushes, a per-scene one (q = 5..8) V * T: with |a|
                        // below the record's bound no sum reaches 2^62 whatever the flushes' signs; the design value
                        // is |a| <= ~2^51 per flush. A flush beyond the bound is counted and k_preproc_bwd then
                        // poisons the call's gradients with NaN instead of returning possibly wrapped sums)
                        if (!(fabsf(a) <= (q >= 5 + (AA ? 1 : 0) && q < (SH ? 6 : 9) ? det_lim_s : det_lim_v)))
                            atomicAdd(det_sat, 1u);
                        atomicAdd(reinterpret_cast<unsigned long long *>(shq ? d.sh_part : (void *)accum) + ai,
                                  (unsigned long long)__float2ll_rn(fminf(fmaxf(a, -9.0e18f), 9.0e18f)));
                    } else {
                        atomicAdd((shq ? reinterpret_cast<float *>(d.sh_part) : accum) + ai, a);
                    }
                }
            }
        }
        if (!DET && s_ndl[ci & 1]) {  // (workgroup-uniform) the chunk's needle conic partials, fp64
            int tt = tid;
            asm volatile("" : "+v"(tt));  // (recomputed here: lane indices hoisted out of the chunk loop spilled)
            for (; tt < 3 * CH; tt += FT) {  // (one pass)
                const int j = tt % CH, c3 = tt / CH;
                const float a = o[(NV + c3) * LS + j];
                if (a != 0.f && b0 + j < s1) {
                    const unsigned gid = sId[j];
                    // (the needle block's offset recomputed here from the SGPR dims: a pointer hoisted out of the
                    // chunk loop was kept in VGPRs and spilled)
                    atomicAdd(reinterpret_cast<double *>(accum) + accum_needle_dbl(d.B, d.V, d.N, gbase + gid, c3),
                              (double)a);
                }
            }
        }
        }  // (flushing waves)
        SEC_T(ts_c4);
        SEC_ADD(sec[7], ts_c3b, ts_c4);  // gradient atomics (issue)
    }
    SEC_FLUSH(d.counters && lane == 0, d.counters, sec, 8);
    if (d.counters && tid == 0) {  // work-item timeline (lgm_diag.render_counters): start, end, (length | chunk | tile)
        unsigned long long *o = d.counters + item_stamps + CNT_ITEM * (size_t)blockIdx.x;
        o[0] = t_item;
        o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = (unsigned long long)(s1 - s0) | ((unsigned long long)c << 20) | ((unsigned long long)tile << 40);
        o[3] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) |        // XCC_ID (the XCD)
               ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8);  // HW_ID
    }
}

}  // namespace

int launch_render_bwd(const Dims &d, const float *gaussians, const float *cam_view, const float *cam_view_proj,
                      const float *bg, const float *d_image, const float *d_depth, const float *d_alpha,
                      float *d_gaussians, float *d_means2D, const Workspace &w, const Layout &L, hipStream_t st) {
    auto zero = [&](void *p, size_t bytes) {
        if (hipMemsetAsync(p, 0, bytes, st) == hipSuccess) return true;
        set_error("hipMemsetAsync failed");
        return false;
    };
    // the accumulators were zeroed by the forward (AccumLayout: who zeroes what); a repeated backward of the same
    // forward clears what the previous one left ((SH) the per-view colour partials too)
    const bool again = (d.options & LGM_RENDER_BACKWARD_AGAIN) != 0;
    if (again && !zero(w.accum_range(L.acc.clear()), L.acc.clear().bytes)) return LGM_E_HIP;
    if (again && L.acc.sh_part.bytes && !zero(w.accum_range(L.acc.sh_part), L.acc.sh_part.bytes)) return LGM_E_HIP;
    const bool loss = (d.options & LGM_RENDER_FUSED_LOSS) != 0, det = (d.options & LGM_RENDER_DETERMINISTIC) != 0;
    if (det) {  // the call's fixed-point scale: max |dL/dpixel| over every seed (k_det_seed_max)
        if (!zero(w.detmax, DET_SLOTS * 4)) return LGM_E_HIP;
        auto smax = with_flags([](auto DEPTH, auto LOSS) { return k_det_seed_max<DEPTH.value, LOSS.value>; },
                               d_depth != nullptr, loss);
        LGM_LAUNCH("k_det_seed_max", st, (smax<<<(unsigned)min(d.BV * d.T, DET_MAX_WGS), 256, 0, st>>>(
                                             d, w.final_T, bg, w.cfin, d_image, d_depth, d_alpha, w.cmask, w.detmax,
                                             w.det_sat)));
    }
    const bool aa = (d.options & LGM_RENDER_ANTIALIAS) != 0;
    const bool sh = d.sh_col != nullptr;  // LGM_RENDER_SH_MASK
    auto bwd = with_flags(
        [](auto DEPTH, auto LOSS, auto DET, auto AA, auto SH) {
            return k_render_bwd<DEPTH.value, LOSS.value, DET.value, AA.value, SH.value>;
        },
        d_depth != nullptr, loss, det, aa, sh);
    // work items: chunk 0 of every tile, then one per checkpoint slot (unused slots exit at once)
    const int M = d.BV * d.T, Mp = round8(M);
    LGM_LAUNCH("k_render_bwd", st, (bwd<<<(unsigned)(Mp + L.ck_slots), 256, 0, st>>>(
                                       d, L.slot ? (long long)d.N : -1LL, w.tile_start, w.tile_count, w.pairs, w.gP,
                                       w.gQ, sh ? d.sh_col : gaussians, bg, w.final_T, w.n_contrib, w.wlast, w.cfin,
                                       w.ck, w.cklist, w.nck, w.ck_counters, L.ck_region, d_image, d_depth, d_alpha,
                                       w.cmask, w.accum, w.detmax, w.det_sat, (long long)cnt_item0(d.BV, d.T, d.N))));
    return launch_preproc_bwd(d, gaussians, cam_view, cam_view_proj, d_gaussians, d_means2D, w, st);
}

}  // namespace lgm
