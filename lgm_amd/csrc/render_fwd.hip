// lgm_amd/csrc/render_fwd.hip -- per-tile alpha compositing, forward, and the fused loss's
// final reduction.
//
// k_render_fwd: one 256-thread workgroup per 16x16 tile; wavefront w owns the 8x8 quadrant (w & 1, w >> 1). The tile's
// sorted Gaussians are staged synchronously, 256 at a time, in LDS (LDS DMA); the loader thread of each entry tests its
// alpha >= 1/255 ellipse (render_common.h) against the four quadrants (stage_commit), and every wavefront compacts the
// chunk to the entries that can touch its quadrant (compact_wave), so it only iterates over Gaussians for which some
// of its pixels pass upstream's `alpha >= 1/255` test. The masks are kept, one byte per list position, for k_render_bwd,
// which reads them instead of testing again. Per-pixel arithmetic, thresholds and the early termination are upstream's;
// alpha is v_exp_f32 of the pre-scaled quadratic form plus log2(opacity) (render_common.h's compositing records).
// k_loss_reduce: LGM_RENDER_FUSED_LOSS's sum over the per-tile partials k_render_fwd<LOSS = true> leaves.
#ifdef LGM_FWD_STAMPS  // the diagnostic build's section stamps (render_stage.h), for this source's kernel only
#define LGM_SEC_STAMPS
#endif
#include "render_stage.h"

namespace lgm {
namespace {

// Entry j of a landed chunk: its quadrant mask (the alpha >= 1/255 ellipse against the four 8x8 quadrants), which
// is also returned (k_render_fwd keeps it for the backward).
// The reciprocals are v_rcp_f32 (1 ulp): they only place the 1-D minimiser on a rectangle edge, and the minimum
// found is compared with a threshold inflated by 1e-3 relative (tau, render_common.h), orders of magnitude more
// than a 1-ulp shift of the minimiser moves a quadratic at its minimum.
template <class Stage>
__device__ __forceinline__ unsigned char stage_commit(Stage &S, typename Stage::Buf &B, int j, bool have, int tx0,
                                                      int ty0) {
    unsigned char mask = 0;
    if (have) {
        const float4 p = B.P[j], q = B.Q[j];
        const float A = -p.z, Bc = -0.5f * p.w, C = -q.x;  // KQ-scaled (render_common.h)
        const float iA = __builtin_amdgcn_rcpf(A), iC = __builtin_amdgcn_rcpf(C);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float qx = (float)(tx0 + ((k & 1) << 3)), qy = (float)(ty0 + ((k >> 1) << 3));
            if (ellipse_hits_rect(p.x, p.y, A, Bc, C, iA, iC, q.z, qx, qx + 7.0f, qy, qy + 7.0f))
                mask |= (unsigned char)(1u << k);
        }
    }
    S.mask[j] = mask;
    return mask;
}

template <class Stage>
__device__ __forceinline__ int compact_wave(Stage &S, int w, int lane, int jmin = 0, int jend = Stage::kRows) {
    constexpr int PAD = (int)(sizeof(S.list[0]) / sizeof(S.list[0][0])) - Stage::kRows;
    int cnt = 0;
    const unsigned long long lt = lanemask_lt(lane);
#pragma unroll
    for (int c = 0; c < Stage::kRows / 64; c++) {
        const int j = c * 64 + lane;
        const bool bit = ((S.mask[j] >> w) & 1u) && j >= jmin && j < jend;
        const unsigned long long bal = __ballot(bit);
        if (bit) S.list[w][cnt + __popcll(bal & lt)] = (unsigned short)j;
        cnt += __popcll(bal);
    }
    if (lane < PAD) S.list[w][cnt + lane] = (unsigned short)Stage::kRows;  // pad to the next multiple of PAD
    return cnt;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// k_render_fwd: grid (B*V*T), block 256, tile xcd_item(blockIdx). 7 waves per SIMD: <= 72 VGPRs (spills outside
// the compositing loop only): 327 vs 336 us at 6, 411 at 8 (pool).
// FU: entries evaluated per step. 4 for every launch that fills the chip; launches of at most one tile per CU
// (FWD_SMALL_TILES: a single 256^2 view, BASELINE config 2) run one wave per SIMD, where nothing hides a wave's own
// dependency chains, and take FU = 8 at 2 waves per SIMD (more registers: twice the independent evaluations in flight).
// The serial T / colour chain is in list order either way: the outputs are bitwise the same.
// SH: LGM_RENDER_SH_MASK -- `gauss` is the per-view colour buffer (stage_dma). Compile-time, so the plain
// instantiations are the code they were.
template <bool LOSS, int FU, bool SH = false>  // LOSS: LGM_RENDER_FUSED_LOSS compiled in (its epilogue registers stay out otherwise)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FU == FWD_FU ? 7 : 2))) void k_render_fwd(Dims d, long long slot_stride,
                                                    const int *__restrict__ tile_start,
                                                    const int *__restrict__ tile_count,
                                                    unsigned long long *__restrict__ pairs,
                                                    const float4 *__restrict__ gP, const float4 *__restrict__ gQ,
                                                    const float *__restrict__ gauss,
                                                    const float *__restrict__ bg, float *__restrict__ out_img,
                                                    float *__restrict__ out_depth, float *__restrict__ out_alpha,
                                                    float *__restrict__ final_T, int *__restrict__ n_contrib,
                                                    int *__restrict__ wlast_out,
                                                    unsigned char *__restrict__ cmask, float4 *__restrict__ cfin,
                                                    float *__restrict__ ck, int2 *__restrict__ cklist,
                                                    int *__restrict__ nck, unsigned *__restrict__ ckctr,
                                                    int ck_region, float4 *__restrict__ zero_base,
                                                    long long zero_n16) {
    __shared__ StageT<1, FU> S;
    __shared__ int s_ck[2];
    const int tile = xcd_item(blockIdx.x, d.BV * d.T);
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
    // The quadrant masks of every chunk staged here are kept for k_render_bwd, one byte per list position, in the dead
    // half of the tile's own pair range: k_sort leaves the n sorted ids as u32 in the first 4 n of its 8 n bytes (every
    // path: msd_sort's ids_out, the LSD passes' and sort_oversized's in-place ids, a single id in the low half of
    // its key; slot and packed ranges alike) and nothing reads the rest again. Position p's mask is byte 4 n + p.
    unsigned char *qmask = reinterpret_cast<unsigned char *>(pairs + base) + 4 * (size_t)n;
    const size_t gbase = (size_t)bv * d.N;
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    init_sentinel(S);
    // Tr < 0 marks a saturated pixel (|Tr| its final transmittance): outside pixels start saturated
    float Tr = inside ? 1.0f : -1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f;
    int last = 0;
    unsigned c_iter = 0, c_list = 0;  // diagnostic work counters (Dims::counters)
    // Staging: chunk c's entries land by LDS DMA, synchronously; the sorted ids run two chunks ahead in registers.
    // Each lane tests its own entry as soon as its row has landed, so one barrier publishes rows and masks together.
    unsigned id_a = tid < n ? ids[tid] : 0u;                        // chunk c
    unsigned id_b = TILE_PIX + tid < n ? ids[TILE_PIX + tid] : 0u;  // chunk c + 1
    // Backward checkpoints: entering every chunk c >= 1 the per-pixel state (T and the prefix colour / depth sums)
    // goes to a pool slot, reserved one chunk ahead from the region's counter (thread 0), so that k_render_bwd can
    // take the chunk as a work item of its own. The pool is sharded by tile over ckctr's 8 counters; a full region
    // just leaves the rest of the tile to the previous chunk's item.
    // (the region is the tile's XCD block group and its slots are interleaved by region, so the backward's
    // checkpoint items run on the XCD that composited the tile). Deterministic mode takes none (render_common.h).
    const int ck_reg = xcd_group(tile, d.BV * d.T);
    const bool det_ck = (d.options & LGM_RENDER_DETERMINISTIC) != 0;
    int ck_slot = -1, ck_written = 0;  // thread 0: slot reserved for the next boundary; checkpoints written
    // wave cycles per section (LGM_FWD_STAMPS build only; per-tile counters +2..+5, scripts/diag_fwd_stamps.py)
    SEC_VAR(fs_head); SEC_VAR(fs_mid); SEC_VAR(fs_comp);
    SEC_T(fs_t0);
    for (int b0 = 0, c = 0; b0 < n; b0 += TILE_PIX, c++) {
        SEC_T(fs_a);
        if (tid == 0) s_ck[c & 1] = ck_slot;  // reserved during chunk c - 1 (its atomic has long returned)
        if (__syncthreads_count(Tr < 0.f) == TILE_PIX) break;  // also: every wave is done with the previous chunk
        c_list += min(TILE_PIX, n - b0);
        const int k = b0 + tid;
        auto &B = S.buf[0];
        if (k < n) stage_dma<SH>(B, w, id_a, gbase, b, d.N, gP, gQ, gauss);
        vm_wait();
        const unsigned char qm = stage_commit(S, B, tid, k < n, tx0, ty0);
        __syncthreads();
        if (k < n) qmask[k] = qm;  // (one coalesced 256-B store per chunk; drains during the compositing)
        SEC_T(fs_b);
        SEC_ADD(fs_head, fs_a, fs_b);
        // checkpoint stores and the next reservation go out after this chunk's DMA wait, so they have the whole
        // chunk's compositing to complete before the next wait
        if (tid == 0) {
            ck_slot = -1;
            if (b0 + TILE_PIX < n && !det_ck && ((c + 1) & ((1 << d.ck_shift) - 1)) == 0) {
                const unsigned l = atomicAdd(&ckctr[ck_reg], 1u);
                if (l < (unsigned)ck_region) ck_slot = (int)l * 8 + ck_reg;
            }
        }
        if (c >= 1) {
            const int sl = s_ck[c & 1];  // workgroup-uniform
            if (sl >= 0) {
                int ctid = tid;
                // (the lane's checkpoint address recomputed here: hoisted out of the chunk loop, ck + tid was spilled
                // and its reload's vmcnt(0) waited for the chunk's outstanding loads)
                asm volatile("" : "+v"(ctid));
                float *cp = ck + (size_t)sl * 5 * TILE_PIX + ctid;
                cp[0] = fabsf(Tr);
                cp[TILE_PIX] = C0;
                cp[2 * TILE_PIX] = C1;
                cp[3 * TILE_PIX] = C2;
                cp[4 * TILE_PIX] = D;
                if (tid == 0) {
                    cklist[sl] = make_int2(tile, c >> d.ck_shift);
                    ck_written = c >> d.ck_shift;
                }
            }
        }
        id_a = id_b;
        id_b = k + 2 * TILE_PIX < n ? ids[k + 2 * TILE_PIX] : 0u;
        const int cnt = compact_wave(S, w, lane);
        SEC_T(fs_c);
        SEC_ADD(fs_mid, fs_b, fs_c);
        // FU = 4 entries per step: their alphas are independent of the running transmittance, so they are evaluated
        // together (ILP, branch-free: list padded with the opacity-0 sentinel); only the short T / colour update
        // chain stays serial, in list order, as upstream.
        uint2 lraw[FU / 4];  // the next step's list words, read one step ahead (the list is fixed for the chunk)
        list_raw<FU>(S, w, 0, lraw);
        for (int kk = 0; kk < cnt; kk += FU) {
            if (__ballot(Tr > 0.f) == 0ull) break;
            c_iter += min(FU, cnt - kk);
            int jj[FU];
            list_decode<FU>(lraw, jj);
            float al[FU];
            float4 cc[FU], Pv[FU], Qv[FU];
            // all the batch's LDS reads first, then one wait: the scheduler would otherwise interleave them with the
            // arithmetic entry by entry (its register-pressure heuristics) and expose the LDS latency FU times
#pragma unroll
            for (int u = 0; u < FU; u++) {
                Pv[u] = B.P[jj[u]];
                Qv[u] = B.Q[jj[u]];
                const float4 R = B.R[jj[u]];
                cc[u] = make_float4(R.x, R.y, R.z, 0.f);
            }
            list_raw<FU>(S, w, kk + FU, lraw);  // in bounds: the list rows hold kRows + FU words
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < FU; u++) {
                const float4 P = Pv[u], Q = Qv[u];
                cc[u].w = Q.w;
                // pre-scaled records (render_common.h): lp = power log2(e) + log2(opacity), e = opacity G
                const float dx = P.x - pfx, dy = P.y - pfy;
                const float lp = fmaf(Q.x * dy, dy, fmaf(fmaf(P.w, dy, P.z * dx), dx, Q.y));
                const float e = __builtin_amdgcn_exp2f(lp);
                const float alpha = alpha_cap(e);
                al[u] = (lp > Q.y || e < 1.0f / 255.0f) ? 0.f : alpha;  // 0 == skipped (power > 0 <=> lp > L)
            }
            // the serial chain as selects (no per-lane branches for the compiler to sink the alpha evaluations into,
            // so the FU evaluations above stay independent): upstream's test_T = T (1 - alpha) and T < 1e-4
            // termination, with the termination kept in Tr's sign -- a skipped entry (alpha 0) leaves test_T = T,
            // a saturated pixel (Tr < 0) has test_T <= 0, so one compare decides both
#pragma unroll
            for (int u = 0; u < FU; u++) {
                const float alpha = al[u];
                const float test_T = Tr * (1 - alpha);
                const bool keep = test_T >= 0.0001f;
                const float aw = keep ? alpha * Tr : 0.f;
                C0 = fmaf(cc[u].x, aw, C0);
                C1 = fmaf(cc[u].y, aw, C1);
                C2 = fmaf(cc[u].z, aw, C2);
                D = fmaf(cc[u].w, aw, D);
                Tr = keep ? test_T : -fabsf(Tr);
                const bool acc = keep && alpha != 0.f;
                last = acc ? b0 + jj[u] + 1 : last;
            }
        }
        SEC_T(fs_d);
        SEC_ADD(fs_comp, fs_c, fs_d);
    }
#ifdef LGM_FWD_STAMPS  // (stores to the tile's own slots, and a last stamp that only the storing thread takes)
    if (d.counters && tid == 0) {
        d.counters[cnt_tile(tile) + 2] = fs_head;  // (wave 0: termination count + staging + entry tests + barrier)
        d.counters[cnt_tile(tile) + 3] = fs_mid;   // (checkpoint stores + compaction)
        d.counters[cnt_tile(tile) + 4] = fs_comp;  // (the compositing loop)
        d.counters[cnt_tile(tile) + 5] = sec_stamp() - fs_t0;  // (the whole chunk loop)
    }
#endif
    if (zero_n16 > 0) {
        // this workgroup's slice of the backward's gradient accumulators (per-view and per-scene records, fp32 or
        // int64): zeroed here, at the end of the compositing, where the stores have the rest of the launch to drain,
        // instead of in the binning's critical path (pool / single scene -8 / -2 us, profiles/r04/ab_zf)
        const long long per = (zero_n16 + gridDim.x - 1) / gridDim.x, z0 = per * blockIdx.x;
        const long long z1 = min(zero_n16, z0 + per);
        for (long long q = z0 + tid; q < z1; q += TILE_PIX) zero_base[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid == 0) {
        if (ck_slot >= 0) cklist[ck_slot] = make_int2(-1, 0);  // reserved for a boundary never reached
        nck[tile] = ck_written;  // checkpoints c = 1 .. ck_written exist (a prefix: the counters only grow)
    }
    {  // the wave's largest last contributor (outside pixels: 0), for the backward's list bounds
        const int wl = wave_max_i32(last);
        if (lane == 0) wlast_out[4 * (size_t)tile + w] = wl;
    }
    if (d.counters) {
        // per-workgroup timeline (100 MHz s_memrealtime ticks): [8 + 8 tile] start, +1 end, +7 entries staged (low
        // 32 bits) and this wave's 4-entry steps (high 32 bits, wave 0). No aggregate atomics on shared words here:
        // 4 same-address atomics per wave over every tile serialise in L2 and stretched the forward's timeline ~7x.
        if (tid == 0) {
            // where it ran: HW_ID (SE / CU / SIMD / wave slot) in the high half of [+6] (the list length stays in the
            // low half), the XCD (XCC_ID) in the top byte of [+7]
            const unsigned hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
            d.counters[cnt_tile(tile)] = t_start;
            d.counters[cnt_tile(tile) + 1] = __builtin_amdgcn_s_memrealtime();
            d.counters[cnt_tile(tile) + 6] = (unsigned long long)(unsigned)n | ((unsigned long long)hw_id << 32);
            d.counters[cnt_tile(tile) + 7] = (unsigned long long)c_list | ((unsigned long long)c_iter << 32) |
                                                   ((unsigned long long)xcc << 56);
        }
    }
    float lsq_img = 0.f, lsq_a = 0.f;  // fused loss: this pixel's squared residuals
    if (inside) {
        Tr = fabsf(Tr);  // (the sign only marked saturation)
        const size_t P = (size_t)d.H * d.W;
        const size_t pid = (size_t)d.W * py + px;
        final_T[bv * P + pid] = Tr;
        n_contrib[bv * P + pid] = last;
        float *img = out_img + (size_t)bv * 3 * P;
        // explicit FMAs: the fused loss's backward recomputes these values bit for bit from cfin and final_T
        float c0 = fmaf(Tr, bg[0], C0), c1 = fmaf(Tr, bg[1], C1), c2 = fmaf(Tr, bg[2], C2);
        if (d.options & LGM_RENDER_CLAMP_IMAGE) {  // core/gs.py:87, gradient mask kept for the backward
            auto in01 = [](float v) { return (v >= 0.f && v <= 1.f) ? 1u : 0u; };
            cmask[bv * P + pid] = (unsigned char)(in01(c0) | (in01(c1) << 1) | (in01(c2) << 2));
            c0 = fminf(fmaxf(c0, 0.f), 1.f);
            c1 = fminf(fmaxf(c1, 0.f), 1.f);
            c2 = fminf(fmaxf(c2, 0.f), 1.f);
        }
        img[pid] = c0;
        img[P + pid] = c1;
        img[2 * P + pid] = c2;
        out_depth[bv * P + pid] = D;
        out_alpha[bv * P + pid] = 1 - Tr;
        cfin[bv * P + pid] = make_float4(C0, C1, C2, D);  // pre-background totals for the backward
        if (LOSS) {
            // core/models.py:145-148: gt composited over the background, squared residuals of image and alpha
            const float m = d.gt_mask[bv * P + pid];
            const float *gi = d.gt_img + (size_t)bv * 3 * P;
            const float r0 = c0 - (gi[pid] * m + bg[0] * (1.f - m));
            const float r1 = c1 - (gi[P + pid] * m + bg[1] * (1.f - m));
            const float r2 = c2 - (gi[2 * P + pid] * m + bg[2] * (1.f - m));
            const float ra = (1 - Tr) - m;
            lsq_img = r0 * r0 + r1 * r1 + r2 * r2;
            lsq_a = ra * ra;
        }
    }
    if (LOSS) {  // per-tile partial sums, fixed order
        __shared__ float sL[2][4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lsq_img += __shfl_xor(lsq_img, o, 64);
            lsq_a += __shfl_xor(lsq_a, o, 64);
        }
        if (lane == 0) { sL[0][w] = lsq_img; sL[1][w] = lsq_a; }
        __syncthreads();
        if (tid < 2) d.loss_part[2 * (size_t)tile + tid] = ((sL[tid][0] + sL[tid][1]) + sL[tid][2]) + sL[tid][3];
    }
}

// Fused loss, final reduction over the per-tile (image, alpha) partials, fixed order, one launch: workgroup g sums
// tiles [g * LR_TILES, +LR_TILES) (each thread LR_PER independent loads, then a fixed tree), writes its double2
// partial, and the workgroup that arrives last (a counter in the workspace, zeroed by the forward's memset and
// reset by that workgroup) sums the partials in workgroup order and writes
// out = (loss_mse, mse_image, mse_alpha, psnr) as core/models.py:148 (F.mse_loss twice) and :167 (psnr).
// (Was one workgroup looping over every tile: 38.8 us at cfg5's 26,624 tiles, now a few us.)
constexpr int LR_THREADS = 256, LR_PER = 8, LR_TILES = LR_THREADS * LR_PER;
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(LR_THREADS) void k_loss_reduce(int M, const float2 *__restrict__ part, double n_img,
                                                           double n_a, double2 *__restrict__ wg_part,
                                                           unsigned *__restrict__ counter, float *__restrict__ out) {
    __shared__ double s[2][LR_THREADS / 64];
    __shared__ bool s_last;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int k0 = blockIdx.x * LR_TILES + t;
    float2 v[LR_PER];
#pragma unroll
    for (int u = 0; u < LR_PER; u++) {
        const int k = k0 + u * LR_THREADS;
        v[u] = k < M ? part[k] : make_float2(0.f, 0.f);
    }
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int u = 0; u < LR_PER; u++) {
        a += (double)v[u].x;
        b += (double)v[u].y;
    }
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    if (lane == 0) { s[0][w] = a; s[1][w] = b; }
    __syncthreads();
    if (t == 0) {
        double2 r = make_double2(0.0, 0.0);
        for (int q = 0; q < LR_THREADS / 64; q++) { r.x += s[0][q]; r.y += s[1][q]; }
        wg_part[blockIdx.x] = r;
        __threadfence();  // the partial is visible device-wide before the arrival is counted
        s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();  // acquire: the other workgroups' partials (written back from their XCDs' L2s)
    double2 r = make_double2(0.0, 0.0);  // the last workgroup: partials in workgroup order (lanes, then a tree)
    for (int g = t; g < (int)gridDim.x; g += LR_THREADS) {
        const double2 x = wg_part[g];
        r.x += x.x;
        r.y += x.y;
    }
    r.x = wave_sum_f64(r.x);
    r.y = wave_sum_f64(r.y);
    if (lane == 0) { s[0][w] = r.x; s[1][w] = r.y; }
    __syncthreads();
    if (t == 0) {
        double si = 0.0, sa = 0.0;
        for (int q = 0; q < LR_THREADS / 64; q++) { si += s[0][q]; sa += s[1][q]; }
        const float mi = (float)(si / n_img), ma = (float)(sa / n_a);
        out[0] = mi + ma;
        out[1] = mi;
        out[2] = ma;
        out[3] = -10.f * log10f(mi);
        *counter = 0u;  // ready for the next launch on this workspace
    }
}

}  // namespace

int launch_render_fwd(const Dims &d, const float *gaussians, const float *bg, float *image, float *depth,
                      float *alpha, const Workspace &w, const Layout &L, hipStream_t st) {
    const bool small = d.BV * d.T <= FWD_SMALL_TILES;
    const bool sh = d.sh_col != nullptr;  // LGM_RENDER_SH_MASK: the colours are staged from the per-view buffer
    auto fwd = with_flags(
        [](auto LOSS, auto SMALL, auto SH) { return k_render_fwd<LOSS.value, SMALL.value ? 8 : FWD_FU, SH.value>; },
        (d.options & LGM_RENDER_FUSED_LOSS) != 0, small, sh);
    if (sh) gaussians = d.sh_col;
    LGM_LAUNCH("k_render_fwd", st, (fwd<<<(unsigned)(d.BV * d.T), 256, 0, st>>>(
                                       d, L.slot ? (long long)d.N : -1LL, w.tile_start, w.tile_count, w.pairs, w.gP,
                                       w.gQ, gaussians, bg, image, depth, alpha, w.final_T, w.n_contrib, w.wlast,
                                       w.cmask, w.cfin, w.ck, w.cklist, w.nck, w.ck_counters, L.ck_region, w.accum16,
                                       (long long)(L.acc.fwd_zero().bytes / 16))));
    return LGM_OK;
}

int launch_loss_reduce(const Dims &d, const Workspace &w, hipStream_t st) {
    const double P = (double)d.H * d.W;
    const int M = d.BV * d.T, G = (M + LR_TILES - 1) / LR_TILES;
    LGM_LAUNCH("k_loss_reduce", st, (k_loss_reduce<<<G, LR_THREADS, 0, st>>>(
                                        M, w.lossp, 3.0 * d.BV * P, d.BV * P, w.lossw, w.loss_arrival, d.loss_out)));
    return LGM_OK;
}

}  // namespace lgm
