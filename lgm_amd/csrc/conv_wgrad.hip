// lgm_amd/csrc/conv_wgrad.hip -- the weight / bias gradient of the UNet's stride-1 3 x 3 and 1 x 1 convolutions
// (include/lgm_conv.h): dw[co][ci][ky][kx] = sum over n, y, x of dy[n][co][y][x] * X[n][ci][y + ky - p][x + kx - p] and
// db[co] = sum of dy[n][co][y][x], the K = N * H * W long reduction of core/unet.py's nn.Conv2d layers under 16-bit
// autocast. k_wgrad's plan (wgrad.hip) on NCHW operands:
//   * the reduction runs over a padded pixel space: image row (n, y) takes Wp = ceil(W / 8) * 8 slots, the slots past W
//     hold zeros in dy and in x. A group of 8 slots (one lane's MFMA operand, 16 B) then never crosses a row, so the tap
//     ky is a whole-row offset and every LDS fragment read is a 16-byte aligned ds_read_b128, whatever W is;
//   * 64 x 64 output tiles over (Cout, Cin) with all taps in one workgroup (4 waves in 2 x 2, each 32 x 32 x 9 taps =
//     36 accumulator fragments); the slot range split S ways so that tiles * S fills the chip; fp32 partials;
//     k_conv_wgrad_reduce sums them in split order and scatters into dw / db;
//   * a stage is 64 slots: the dy strip and, per ky, the x strip of the rows y + ky - 1 (zeros where that row is outside
//     the image: masked at staging time per 8-slot group, so planes adjacent in memory never leak into each other).
//     The taps kx = 0 / 2 are the centre fragment shifted by one element in registers (v_alignbit) with the element
//     before / after the group (zero at x = 0 / x = W - 1) shifted in from a side array staged with the strip: no
//     misaligned LDS read and no second copy of the strip;
//   * staged through registers, the next stage's global loads in flight during the current stage's MFMAs. A group is
//     one 16-byte load where it is whole and 16-byte aligned and eight 2-byte loads otherwise: the same values land in
//     the same LDS slots, so both forms give the same bits;
//   * LDS images are [group][channel] chunks of 16 B, the channel XORed with the group: conflict-free for the
//     ds_read_b128 lane groups and for the ds_write_b128 of the staging threads;
//   * db on the same MFMAs (dy fragment times ones) in the workgroups of the first Cin tile only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdna4.h"
#include "common.h"
#include "lgm_conv.h"

namespace lgm {
namespace cw {

constexpr int BM = 64, BN = 64;    // output tile (Cout x Cin) of one workgroup
constexpr int BK = 64;             // slots per stage: two 32-slot MFMA K steps
constexpr int KG = BK / 8;         // 8-slot groups per stage
constexpr int THREADS = 256;
constexpr int WPE = 2;             // workgroups (= waves per SIMD) per CU: 254 VGPRs and 40 KB of LDS each at 3 x 3
constexpr int IMG = KG * 64 * 16;  // bytes of one strip image (KG groups x 64 channels x 16 B)
constexpr int SIDE = KG * 80;      // dwords of one strip's side array ((before | after << 16) per group and channel)
constexpr int SLOTS = 256 * WPE;   // workgroup slots per round at 3 x 3 (2 per CU)
constexpr int SLOTS_1 = 256 * 4;   // at 1 x 1 (98 VGPRs, 16 KB of LDS: 4 per CU)
constexpr int MIN_STAGES = 8;      // stages per split at least
constexpr int MAX_ROUNDS = 4;      // rounds of SLOTS workgroups at most (where the tiles alone are not more)
constexpr int DBT = 8;             // k_conv_wgrad_reduce lanes per bias-gradient row

struct Geo {
    int N, Cin, Cout, H, W, Wp;
    long long NR;         // image rows N * H
    int dq, dr, dqn, dqy; // one stage = dq rows + dr slots; dq rows = dqn planes + dqy rows
};

// 8 consecutive elements from p (the first cnt of them; the rest zero): one 16-byte load where the address allows it
__device__ __forceinline__ u32x4 load8(const uint16_t *p, int cnt) {
    if (cnt == 8 && ((uintptr_t)p & 15) == 0) return *reinterpret_cast<const u32x4 *>(p);
    unsigned e[8];
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = k < cnt ? (unsigned)p[k] : 0u;
    return u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}

// byte offset of (group kg, channel ch) in a strip image
__device__ __forceinline__ int chunk(int kg, int ch) { return ((kg << 6) + (ch ^ kg)) << 4; }

template <int KS> struct Pre {
    u32x4 a[2], b[KS][2];
    unsigned side[KS][2];
};

// k_conv_wgrad: grid (tiles * S), block 256. Workgroup item xcd_item(blockIdx) (work_split.h) -> (split s, tile
// (mt, nt)): the workgroups of one XCD take a contiguous range of the items, so the tiles that read the same dy / x
// strips share an L2. Split s covers its split_range of the nst_all stages.
template <int DT, int KS>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(WPE))) void k_conv_wgrad(
    Geo G, const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x, int S, int NT, long long nst_all,
    f32x4 *__restrict__ part, float *__restrict__ dbpart, int Mp) {
    constexpr int TAPS = KS * KS, PAD = (KS - 1) / 2;
    __shared__ __attribute__((aligned(16))) unsigned char sA[IMG];
    __shared__ __attribute__((aligned(16))) unsigned char sB[KS][IMG];
    __shared__ unsigned sS[KS][SIDE];
    const int tiles = gridDim.x / S;
    const int item = xcd_item(blockIdx.x, gridDim.x);
    const int s = item / tiles, tile = item - s * tiles, mt = tile / NT, nt = tile - mt * NT;
    const int m0 = mt * BM, n0c = nt * BN;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, wm = w >> 1, wn = w & 1;
    const int wn_u = __builtin_amdgcn_readfirstlane(w) & 1;
    const int g = lane >> 4, i = lane & 15;
    long long st0, nst_ll;
    split_range(nst_all, S, s, st0, nst_ll);
    const int nst = (int)nst_ll;
    const bool want_db = dbpart != nullptr && nt == 0 && wn_u == 0;
    const int H = G.H, W = G.W, Wp = G.Wp;

    // the stage's first slot as (plane n0, row y0, slot s00 of that row); row0 = n0 * H + y0
    long long row0 = st0 * BK / Wp;
    int s00 = (int)(st0 * BK - row0 * Wp);
    int n0 = (int)(row0 / H), y0 = (int)(row0 - (long long)n0 * H);

    const int kg = threadIdx.x & 7, crow = threadIdx.x >> 3;  // this thread's group and channels (crow, crow + 32)
    auto load = [&]() {
        Pre<KS> P;
        const unsigned sl = (unsigned)(s00 + 8 * kg);
        const unsigned drow = sl / (unsigned)Wp;
        const int sx = (int)(sl - drow * (unsigned)Wp);
        const unsigned yy = (unsigned)y0 + drow, dn = yy / (unsigned)H;
        const int y = (int)(yy - dn * (unsigned)H), n = n0 + (int)dn;
        const bool valid = row0 + drow < G.NR;
        const int cnt = valid ? min(8, W - sx) : 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int c = m0 + crow + 32 * h;
            P.a[h] = u32x4{0u, 0u, 0u, 0u};
            if (valid && c < G.Cout) P.a[h] = load8(dy + (((long long)n * G.Cout + c) * H + y) * W + sx, cnt);
        }
#pragma unroll
        for (int ky = 0; ky < KS; ky++) {
            const int yk = y + ky - PAD;
            const bool ok = valid && yk >= 0 && yk < H;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int c = n0c + crow + 32 * h;
                P.b[ky][h] = u32x4{0u, 0u, 0u, 0u};
                P.side[ky][h] = 0u;
                if (ok && c < G.Cin) {
                    const uint16_t *p = x + (((long long)n * G.Cin + c) * H + yk) * W + sx;
                    P.b[ky][h] = load8(p, cnt);
                    if (KS == 3) {
                        const unsigned before = sx > 0 ? (unsigned)p[-1] : 0u;
                        const unsigned after = sx + 8 < W ? (unsigned)p[8] : 0u;
                        P.side[ky][h] = before | (after << 16);
                    }
                }
            }
        }
        // the next stage's first slot
        s00 += G.dr;
        row0 += G.dq;
        y0 += G.dqy;
        n0 += G.dqn;
        if (s00 >= Wp) {
            s00 -= Wp;
            row0++;
            y0++;
        }
        if (y0 >= H) {
            y0 -= H;
            n0++;
        }
        return P;
    };
    auto store = [&](const Pre<KS> &P) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int ch = crow + 32 * h;
            *reinterpret_cast<u32x4 *>(sA + chunk(kg, ch)) = P.a[h];
#pragma unroll
            for (int ky = 0; ky < KS; ky++) {
                *reinterpret_cast<u32x4 *>(sB[ky] + chunk(kg, ch)) = P.b[ky][h];
                if (KS == 3) sS[ky][kg * 80 + ch] = P.side[ky][h];
            }
        }
    };

    f32x4 acc[4 * TAPS], dbacc[2];
#pragma unroll
    for (int f = 0; f < 4 * TAPS; f++) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    dbacc[0] = dbacc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u32x4 ones = u32x4{Op16<DT>::ONE2, Op16<DT>::ONE2, Op16<DT>::ONE2, Op16<DT>::ONE2};

    Pre<KS> P;
    if (nst > 0) P = load();
    for (int j = 0; j < nst; j++) {
        store(P);
        __syncthreads();
        if (j + 1 < nst) P = load();  // in flight during this stage's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK / 32; kk++) {
            const int kgr = 4 * kk + g;
            u32x4 fa[2];
#pragma unroll
            for (int a = 0; a < 2; a++) fa[a] = *reinterpret_cast<const u32x4 *>(sA + chunk(kgr, 32 * wm + 16 * a + i));
            if (want_db) {
                dbacc[0] = mfma16<DT>(fa[0], ones, dbacc[0]);
                dbacc[1] = mfma16<DT>(fa[1], ones, dbacc[1]);
            }
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int ch = 32 * wn + 16 * b + i;
#pragma unroll
                for (int ky = 0; ky < KS; ky++) {
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(sB[ky] + chunk(kgr, ch));
                    if constexpr (KS == 3) {
                        const unsigned sd = sS[ky][kgr * 80 + ch];
                        const unsigned m01 = __builtin_amdgcn_alignbit(v.y, v.x, 16);
                        const unsigned m12 = __builtin_amdgcn_alignbit(v.z, v.y, 16);
                        const unsigned m23 = __builtin_amdgcn_alignbit(v.w, v.z, 16);
                        const u32x4 vl = u32x4{(v.x << 16) | (sd & 0xffffu), m01, m12, m23};           // X[slot - 1]
                        const u32x4 vr = u32x4{m01, m12, m23, (v.w >> 16) | (sd & 0xffff0000u)};       // X[slot + 1]
#pragma unroll
                        for (int a = 0; a < 2; a++) {
                            const int t = (a * 2 + b) * TAPS + ky * 3;
                            acc[t] = mfma16<DT>(fa[a], vl, acc[t]);
                            acc[t + 1] = mfma16<DT>(fa[a], v, acc[t + 1]);
                            acc[t + 2] = mfma16<DT>(fa[a], vr, acc[t + 2]);
                        }
                    } else {
#pragma unroll
                        for (int a = 0; a < 2; a++) acc[a * 2 + b] = mfma16<DT>(fa[a], v, acc[a * 2 + b]);
                    }
                }
            }
        }
        __syncthreads();  // every wave has read the stage: the images are free
    }
    // fp32 partials in fragment order: one float4 per lane per fragment
    f32x4 *pp = part + ((size_t)((long long)s * tiles + tile) * 4 + w) * (4 * TAPS) * 64 + lane;
#pragma unroll
    for (int f = 0; f < 4 * TAPS; f++) pp[f * 64] = acc[f];
    if (want_db && i == 0) {  // lane (g, 0) holds the sums of rows 4g .. 4g + 3 of each 16-row block
        float *dp = dbpart + (size_t)s * Mp + m0 + 32 * wm + 4 * g;
#pragma unroll
        for (int a = 0; a < 2; a++) *reinterpret_cast<f32x4 *>(dp + 16 * a) = dbacc[a];
    }
}

// k_conv_wgrad_reduce: grid (ceil(npos / 256) + [ceil(Cout * DBT / 256)]), block 256. One thread per (tile, wave,
// fragment, lane) float4 position: the S partials summed in split order (up to 16 loads in flight), the 4 values
// scattered to dw; then (db) DBT threads per row: the S column-sum partials in a fixed order. S = 0 writes zeros.
__global__ __launch_bounds__(256) void k_conv_wgrad_reduce(int Cout, int Cin, int TAPS, int S, int NT, long long tiles,
                                                           const f32x4 *__restrict__ part,
                                                           const float *__restrict__ dbpart, int Mp,
                                                           float *__restrict__ dw, float *__restrict__ db) {
    const int FR = 4 * TAPS;
    const long long npos = tiles * 4 * FR * 64;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < npos) {
        f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; s += 16) {
            f32x4 v[16];
#pragma unroll
            for (int u = 0; u < 16; u++)
                v[u] = s + u < S ? part[(size_t)(s + u) * npos + p] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (s + u < S) sum += v[u];  // (split order)
        }
        const int lane = (int)(p & 63), f = (int)((p >> 6) % FR), w = (int)((p / (64 * FR)) & 3);
        const long long tile = p / (256 * FR);
        const int mt = (int)(tile / NT), nt = (int)(tile - (long long)mt * NT);
        const int ab = f / TAPS, tap = f - ab * TAPS, a = ab >> 1, b = ab & 1, g = lane >> 4, i = lane & 15;
        const int co = mt * BM + 32 * (w >> 1) + 16 * a + 4 * g, ci = nt * BN + 32 * (w & 1) + 16 * b + i;
        if (ci < Cin) {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (co + e < Cout) dw[((size_t)(co + e) * Cin + ci) * TAPS + tap] = sum[e];
        }
        return;
    }
    if (!db) return;
    // db: DBT adjacent lanes per row, each summing a contiguous part of the S partials in order, then a fixed xor
    // tree over the DBT lanes: deterministic
    const long long qd = p - ((npos + 255) / 256) * 256;
    const int m = (int)(qd / DBT), part8 = (int)(qd % DBT);
    const int per = (S + DBT - 1) / DBT, q0 = min(S, part8 * per), q1 = min(S, q0 + per);
    float v = 0.f;
    if (m < Cout) {
        for (int qq = q0; qq < q1; qq += 16) {
            float t[16];
#pragma unroll
            for (int u = 0; u < 16; u++) t[u] = qq + u < q1 ? dbpart[(size_t)(qq + u) * Mp + m] : 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++) v += t[u];
        }
    }
#pragma unroll
    for (int o = 1; o < DBT; o <<= 1) v += __shfl_xor(v, o, 64);  // (the same tree in every lane)
    if (m < Cout && part8 == 0) db[m] = v;
}

struct Plan {
    int MT, NT, S, Mp, Wp;
    long long tiles, nst;
    size_t part_bytes, db_bytes;
};
inline Plan plan(int N, int Cin, int Cout, int H, int W, int ksize, bool want_db) {
    Plan P;
    P.MT = (Cout + BM - 1) / BM;
    P.NT = (Cin + BN - 1) / BN;
    P.tiles = (long long)P.MT * P.NT;
    P.Wp = (W + 7) / 8 * 8;
    P.nst = ((long long)N * H * P.Wp + BK - 1) / BK;
    // S: the chip runs the tiles * S workgroups in rounds of `slots` (2 workgroups per CU at 3 x 3, 4 at 1 x 1: their
    // registers and LDS), so the time goes as rounds / S. For r = 1 .. MAX_ROUNDS rounds the largest S that fits them
    // (and leaves MIN_STAGES stages per split); of these the fewest rounds within 7 % of the best (more splits are more
    // partials to write and to sum: 3 rounds measured slower than 1 at equal fill). E.g. 384 tiles at 3 x 3: S = 1
    // fills 384 of 512 slots, S = 4 is three full rounds.
    const long long slots = ksize == 1 ? SLOTS_1 : SLOTS, by_stages = P.nst / MIN_STAGES;
    long long Sr[MAX_ROUNDS + 1], best = 0;
    for (int r = 1; r <= MAX_ROUNDS; r++) {
        Sr[r] = r * slots / P.tiles < by_stages ? r * slots / P.tiles : by_stages;
        if (Sr[r] > 0 && (best == 0 || r * Sr[best] < best * Sr[r])) best = r;  // r / Sr[r] < best / Sr[best]
    }
    long long pick = 1;
    for (int r = MAX_ROUNDS; r >= 1; r--)
        if (best && Sr[r] > 0 && r * Sr[best] * 100 <= best * Sr[r] * 107) pick = Sr[r];
    P.S = P.nst == 0 ? 0 : (int)pick;
    P.Mp = P.MT * BM;
    P.part_bytes = (size_t)P.S * P.tiles * 4 * (4 * ksize * ksize) * 64 * 16;
    P.db_bytes = want_db ? (size_t)P.S * P.Mp * 4 : 0;
    return P;
}

template <int DT, int KS>
inline void launch(const Geo &G, const Plan &P, const void *dy, const void *x, f32x4 *part, float *dbpart,
                   hipStream_t st) {
    k_conv_wgrad<DT, KS><<<(int)(P.tiles * P.S), THREADS, 0, st>>>(G, (const uint16_t *)dy, (const uint16_t *)x, P.S,
                                                                  P.NT, P.nst, part, dbpart, P.Mp);
}

}  // namespace cw
}  // namespace lgm

extern "C" size_t lgm_conv_wgrad_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize, int want_db) {
    if (N < 0 || H < 0 || W < 0 || Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return 0;
    const lgm::cw::Plan P = lgm::cw::plan(N, Cin, Cout, H, W, ksize, want_db != 0);
    return ((P.part_bytes + 255) & ~(size_t)255) + P.db_bytes;
}

extern "C" int lgm_conv_wgrad(int dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *dy,
                              const void *x, float *dw, float *db, void *workspace, size_t workspace_bytes,
                              void *stream, const lgm_diag *diag) {
    using namespace lgm::cw;
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (int rc = lgm::check_dtype16("lgm_conv_wgrad", dtype)) return rc;
    if (ksize != 1 && ksize != 3) {
        lgm::set_error("lgm_conv_wgrad: ksize must be 1 or 3 (got %d)", ksize);
        return LGM_E_INVALID;
    }
    if (N < 0 || Cin < 0 || Cout < 0 || H < 0 || W < 0) {
        lgm::set_error("lgm_conv_wgrad: negative size N=%d Cin=%d Cout=%d H=%d W=%d", N, Cin, Cout, H, W);
        return LGM_E_INVALID;
    }
    if (Cin == 0 || Cout == 0) return LGM_OK;
    const bool work = (long long)N * H * W > 0;
    if (!dw || (work && (!dy || !x))) {
        lgm::set_error("lgm_conv_wgrad: null pointer");
        return LGM_E_INVALID;
    }
    const Plan P = plan(N, Cin, Cout, H, W, ksize, db != nullptr);
    const int TAPS = ksize * ksize;
    const long long npos = P.tiles * 4 * (4 * TAPS) * 64;
    const long long rgrid = (npos + 255) / 256 + (db ? ((long long)Cout * DBT + 255) / 256 : 0);
    if (P.tiles * (P.S > 0 ? P.S : 1) > 2147483647LL || rgrid > 2147483647LL || (long long)N * H > 2147483647LL) {
        lgm::set_error("lgm_conv_wgrad: grid beyond 2^31 - 1 workgroups (Cout=%d Cin=%d N=%d H=%d)", Cout, Cin, N, H);
        return LGM_E_INVALID;
    }
    const size_t need = lgm_conv_wgrad_workspace_size(N, Cin, Cout, H, W, ksize, db != nullptr);
    if (int rc = lgm::check_workspace("lgm_conv_wgrad", workspace, workspace_bytes, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    lgm::f32x4 *part = (lgm::f32x4 *)workspace;
    float *dbpart = db && P.S ? (float *)((char *)workspace + ((P.part_bytes + 255) & ~(size_t)255)) : nullptr;
    if (P.S > 0) {
        Geo G;
        G.N = N, G.Cin = Cin, G.Cout = Cout, G.H = H, G.W = W, G.Wp = P.Wp;
        G.NR = (long long)N * H;
        G.dq = BK / P.Wp, G.dr = BK % P.Wp;
        G.dqn = G.dq / H, G.dqy = G.dq % H;
        lgm::prof_begin("k_conv_wgrad", st);
        if (dtype == LGM_ATTN_BF16) {
            if (ksize == 3) launch<LGM_ATTN_BF16, 3>(G, P, dy, x, part, dbpart, st);
            else launch<LGM_ATTN_BF16, 1>(G, P, dy, x, part, dbpart, st);
        } else {
            if (ksize == 3) launch<LGM_ATTN_F16, 3>(G, P, dy, x, part, dbpart, st);
            else launch<LGM_ATTN_F16, 1>(G, P, dy, x, part, dbpart, st);
        }
        lgm::prof_end(st);
        LGM_LAUNCH_CHECK("k_conv_wgrad");
    }
    LGM_LAUNCH("k_conv_wgrad_reduce", st,
               (k_conv_wgrad_reduce<<<(int)rgrid, 256, 0, st>>>(Cout, Cin, TAPS, P.S, P.NT, P.tiles, part, dbpart, P.Mp,
                                                                dw, db)));
    return LGM_OK;
}
