// lgm_amd/csrc/conv_fwd.hip -- the forward and the input gradient of the UNet's stride-1 3 x 3 and 1 x 1 convolutions
// (include/lgm_conv.h): out[n][co][y][x] = bias[co] + sum over ci, ky, kx of wE[co][ci][ky][kx] * IN[n][ci][y + ky - p][x + kx - p]
// as an implicit GEMM on v_mfma_f32_16x16x32: rows = output channels, columns = pixels, K = (tap, input channel). The
// input gradient is the same kernel on wE[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], an index map of the packing pass.
//   * the pixels run over a padded slot space: image row (n, y) takes Wp = W + 1 slots at 3 x 3 (Wp = W at 1 x 1), the
//     slot past W holds zero: it is the column after x = W - 1 of its row and the column before x = 0 of the next, so the
//     taps kx = 0 / 2 are the neighbouring slots, whatever W is. A workgroup owns 128 consecutive slots x 64 output
//     channels; the K range (32 channels per step, all taps of them) may be split S ways, fp32 partials summed in split
//     order by k_conv_fwd_reduce;
//   * the operand of a pixel column is 8 consecutive channels of one pixel, and the activations are NCHW: the strip is
//     transposed while it is staged. A thread owns one slot and 16 channels: element loads (lanes = consecutive pixels of a
//     plane: coalesced, any alignment), packed in registers, two ds_write_b128 per ky into a channel-innermost image.
//     One image per ky (the rows y + ky - 1 of the same slots; zeros where that row is outside the image, masked per
//     slot, so planes adjacent in memory never leak into each other) plus the slot before and after the strip;
//   * a lane's 4 pixel columns are the slots 4 i + f (f = 0 .. 3): the kx shifts of fragment f are the fragments f - 1
//     and f + 1 (lane i -+ 1 at the ends, a neighbouring chunk of the image), so 6 ds_read_b128 serve the 12 operands of
//     one ky, and a lane's 4 results of one channel are 4 consecutive pixels: one 8-byte store where they are in one row
//     and 8-byte aligned, four 2-byte stores otherwise (the same bits);
//   * images are [channel group of 8][position] chunks of 16 B, the positions of a fragment consecutive in the lane
//     index and the group stride a multiple of 16 chunks: conflict-free for every ds_read_b128 lane group;
//   * the weights are packed once per call (k_conv_wpack: rounded to the operand type, zero-filled to whole tiles) in
//     exactly the order of the LDS image, so their staging is 16-byte copies;
//   * staged through registers: the next step's global loads are in flight during this step's MFMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdna4.h"
#include "common.h"
#include "lgm_conv.h"

namespace lgm {
namespace cf {

constexpr int BM = 64;             // output channels of one workgroup (2 waves x 2 fragments of 16)
constexpr int BN = 128;            // slots of one workgroup (2 waves x 4 fragments of 16)
constexpr int KC = 32;             // input channels per K step: one MFMA K per tap
constexpr int THREADS = 256;
constexpr int FS = 36;             // chunks per fragment index f of a strip image: positions 0 .. 33
constexpr int GS = 4 * FS;         // chunks per channel group: a multiple of 16
constexpr int SLOTS = 512;         // workgroup slots of the chip (2 per CU at 3 x 3)
constexpr int MIN_STEPS = 4;       // K steps per split at least
constexpr int MAX_SPLIT = 16;

// fp32 -> the 16-bit type, round to nearest even (as tensor.to(dt))
template <int DT> __device__ __forceinline__ unsigned rnd(float v) {
    if constexpr (DT == LGM_ATTN_BF16) return __builtin_bit_cast(unsigned short, (__bf16)v);
    else return __builtin_bit_cast(unsigned short, (_Float16)v);
}
template <int DT> __device__ __forceinline__ float widen(unsigned short b) {
    if constexpr (DT == LGM_ATTN_BF16) return __builtin_bit_cast(float, (unsigned)b << 16);
    else return (float)__builtin_bit_cast(_Float16, b);
}
// bias[c] as fp32 (bdt: LGM_ATTN_F32 or the 16-bit type DT; an fp32 bias is rounded to DT first, as autocast's cast of
// it does, so both forms add the same value); NULL: 0
template <int DT> __device__ __forceinline__ float bias_at(const void *bias, int bdt, int c) {
    if (!bias) return 0.f;
    return widen<DT>(bdt == LGM_ATTN_F32 ? (unsigned short)rnd<DT>(((const float *)bias)[c]) : ((const uint16_t *)bias)[c]);
}

struct Geo {
    int Ci, Co, H, W, Wp;  // reduction / output channels, image, slots per image row
    long long NR, HW;      // image rows N * H, plane size
};

// k_conv_wpack: grid (MT * KCN * 4), block 256. One workgroup per 16 output channels of a (mt, kc) tile of the packed
// weight [mt][kc][tap][g][row] (a 16-byte chunk = the 8 channels kc * 32 + g * 8 .. of output channel mt * 64 + row at
// one tap; zeros past the channel counts). In w that is 16 runs of 32 * TAPS consecutive elements (one per output
// channel), or with flip -- the input gradient's map: transposed, taps reversed -- 32 runs of 16 * TAPS: read in that
// order (coalesced, every load of a thread in flight at once), rounded, placed in LDS in the packed order, written out
// as whole chunks.
constexpr int RQ = 16;
template <int DT, int KS>
__global__ __launch_bounds__(256) void k_conv_wpack(const void *__restrict__ w, int wdt, int Cout, int Cin, int flip,
                                                    int KCN, u32x4 *__restrict__ out) {
    constexpr int TAPS = KS * KS, PER = RQ * KC * TAPS / 256;
    __shared__ __attribute__((aligned(16))) uint16_t sW[TAPS * 4 * RQ * 8];
    const int tile = blockIdx.x >> 2, rq = blockIdx.x & 3;
    const int mt = tile / KCN, kc = tile - mt * KCN;
    const int Co = flip ? Cin : Cout, Ci = flip ? Cout : Cin;
    unsigned v[PER];
    int at[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = u * 256 + threadIdx.x;
        int rl, c, tap;
        size_t src;
        if (!flip) {
            rl = e / (KC * TAPS);
            const int r = e - rl * (KC * TAPS);
            c = r / TAPS;
            tap = r - c * TAPS;
            src = ((size_t)(mt * BM + rq * RQ + rl) * Cin + kc * KC + c) * TAPS + tap;
        } else {
            c = e / (RQ * TAPS);
            const int r = e - c * (RQ * TAPS);
            rl = r / TAPS;
            const int ts = r - rl * TAPS;
            tap = TAPS - 1 - ts;
            src = ((size_t)(kc * KC + c) * Cin + mt * BM + rq * RQ + rl) * TAPS + ts;
        }
        v[u] = 0u;
        if (mt * BM + rq * RQ + rl < Co && kc * KC + c < Ci)
            v[u] = wdt == LGM_ATTN_F32 ? rnd<DT>(((const float *)w)[src]) : (unsigned)((const uint16_t *)w)[src];
        at[u] = (((tap * 4 + (c >> 3)) * RQ + rl) << 3) + (c & 7);
    }
#pragma unroll
    for (int u = 0; u < PER; u++) sW[at[u]] = (uint16_t)v[u];
    __syncthreads();
    u32x4 *dst = out + (size_t)tile * (TAPS * 256) + rq * RQ;
#pragma unroll
    for (int q = threadIdx.x; q < TAPS * 4 * RQ; q += 256)
        dst[(q >> 4) * BM + (q & 15)] = reinterpret_cast<const u32x4 *>(sW)[q];
}

template <int KS> struct Pre {
    u32x4 a[KS * KS];
    unsigned b[KS][8];
    unsigned hb[KS];
};

// k_conv: grid (tiles * S), block 256. Workgroup -> (split s, pixel tile pt, channel tile mt); split s covers the K
// steps of its split_range (work_split.h) of the KCN steps. S == 1 writes out (bias added, one rounding);
// S > 1 writes the fp32 partial of split s at the output's own element offsets.
template <int DT, int KS>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_conv(
    Geo G, const uint16_t *__restrict__ x, const u32x4 *__restrict__ wp, const void *__restrict__ bias, int bdt,
    uint16_t *__restrict__ out, float *__restrict__ part, long long total, int S, int MT, int KCN) {
    constexpr int TAPS = KS * KS, PAD = (KS - 1) / 2, NF = 4 + 2 * PAD;
    __shared__ __attribute__((aligned(16))) unsigned char sA[TAPS * 4 * BM * 16];
    __shared__ __attribute__((aligned(16))) unsigned char sB[KS * 4 * GS * 16];
    const int tiles = gridDim.x / S;
    const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles, pt = tile / MT, mt = tile - pt * MT;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, wm = w >> 1, wn = w & 1;
    const int g = lane >> 4, i = lane & 15;
    int kc0, nk;
    split_range(KCN, S, s, kc0, nk);
    const int H = G.H, W = G.W, Wp = G.Wp, Ci = G.Ci;
    const long long HW = G.HW;

    // element offset of (slot, channel 0) in x and the mask of the ky whose row is inside the image (0: a zero slot)
    auto slot_geo = [&](long long sl, long long &off) -> unsigned {
        off = 0;
        if (sl < 0) return 0u;
        const long long row = sl / Wp;
        const int sx = (int)(sl - row * Wp);
        if (row >= G.NR || sx >= W) return 0u;
        const long long n = row / H;
        const int y = (int)(row - n * H);
        off = (n * Ci * H + y) * W + sx;
        unsigned m = 0u;
#pragma unroll
        for (int ky = 0; ky < KS; ky++)
            if (y + ky - PAD >= 0 && y + ky - PAD < H) m |= 1u << ky;
        return m;
    };
    // staging: this thread's slot j and channels 16 ch .. 16 ch + 15 of the step; threads 0 .. 63 also one channel of
    // the slot before / after the strip
    const int j = tid & 127, ch = tid >> 7;
    long long off, hoff = 0;
    const unsigned mask = slot_geo((long long)pt * BN + j, off);
    const int hs = tid >> 5, hc = tid & 31;
    unsigned hmask = 0u;
    if (KS == 3 && tid < 64) hmask = slot_geo((long long)pt * BN + (hs ? BN : -1), hoff);

    auto load = [&](int kc) {
        Pre<KS> P;
        const u32x4 *wsrc = wp + (((size_t)mt * KCN + kc) * TAPS) * 256 + tid;
#pragma unroll
        for (int t = 0; t < TAPS; t++) P.a[t] = wsrc[t * 256];
        const int c0 = kc * KC + ch * 16;
#pragma unroll
        for (int ky = 0; ky < KS; ky++) {
            const bool rk = (mask >> ky) & 1u;
            const uint16_t *p = x + (off + (long long)(ky - PAD) * W + c0 * HW);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const unsigned lo = rk && c0 + 2 * e < Ci ? (unsigned)*p : 0u;
                p += HW;
                const unsigned hi = rk && c0 + 2 * e + 1 < Ci ? (unsigned)*p : 0u;
                p += HW;
                P.b[ky][e] = lo | (hi << 16);
            }
            if (KS == 3) {
                const int c = kc * KC + hc;
                P.hb[ky] = ((hmask >> ky) & 1u) && c < Ci ? (unsigned)x[hoff + (long long)(ky - PAD) * W + c * HW] : 0u;
            }
        }
        return P;
    };
    auto store = [&](const Pre<KS> &P) {
#pragma unroll
        for (int t = 0; t < TAPS; t++) *reinterpret_cast<u32x4 *>(sA + (t * 256 + tid) * 16) = P.a[t];
        const int pos = (j & 3) * FS + (j >> 2) + 1;
#pragma unroll
        for (int ky = 0; ky < KS; ky++) {
#pragma unroll
            for (int h = 0; h < 2; h++)
                *reinterpret_cast<u32x4 *>(sB + (((ky * 4 + ch * 2 + h) * GS + pos) << 4)) =
                    u32x4{P.b[ky][4 * h], P.b[ky][4 * h + 1], P.b[ky][4 * h + 2], P.b[ky][4 * h + 3]};
            if (KS == 3 && tid < 64) {  // slot -1: (f 3, position 0); slot BN: (f 0, position 33)
                const int hpos = hs ? BN / 4 + 1 : 3 * FS;
                *reinterpret_cast<uint16_t *>(sB + (((ky * 4 + (hc >> 3)) * GS + hpos) << 4) + (hc & 7) * 2) =
                    (uint16_t)P.hb[ky];
            }
        }
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int f = 0; f < 4; f++) acc[a][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    Pre<KS> P;
    if (nk > 0) P = load(kc0);
    for (int k = 0; k < nk; k++) {
        store(P);
        __syncthreads();
        if (k + 1 < nk) P = load(kc0 + k + 1);  // in flight during this step's MFMAs
#pragma unroll
        for (int ky = 0; ky < KS; ky++) {
            u32x4 bf[NF];  // the slots 4 i + f' of this wave's 64, f' = -PAD .. 3 + PAD
#pragma unroll
            for (int n = 0; n < NF; n++) {
                const int fp = n - PAD;
                const int pos = (fp & 3) * FS + wn * 16 + i + 1 + (fp < 0 ? -1 : fp > 3 ? 1 : 0);
                bf[n] = *reinterpret_cast<const u32x4 *>(sB + (((ky * 4 + g) * GS + pos) << 4));
            }
#pragma unroll
            for (int kx = 0; kx < KS; kx++) {
                const int t = ky * KS + kx;
                u32x4 fa[2];
#pragma unroll
                for (int a = 0; a < 2; a++)
                    fa[a] = *reinterpret_cast<const u32x4 *>(sA + (((t * 4 + g) * BM + wm * 32 + a * 16 + i) << 4));
#pragma unroll
                for (int f = 0; f < 4; f++)
#pragma unroll
                    for (int a = 0; a < 2; a++) acc[a][f] = mfma16<DT>(fa[a], bf[f + kx], acc[a][f]);
            }
        }
        __syncthreads();  // every wave has read the step: the images are free
    }

    // this lane's 4 slots -> element offsets of channel 0 in out (-1: a padding slot)
    long long oo[4];
    {
        const long long sl = (long long)pt * BN + wn * 64 + 4 * i;
        long long row = sl / Wp;
        int sx = (int)(sl - row * Wp);
        long long n = row / H;
        int y = (int)(row - n * H);
#pragma unroll
        for (int f = 0; f < 4; f++) {
            oo[f] = row < G.NR && sx < W ? (n * G.Co * H + y) * W + sx : -1;
            if (++sx == Wp) {
                sx = 0;
                row++;
                if (++y == H) y = 0, n++;
            }
        }
    }
    const bool whole = oo[0] >= 0 && oo[3] == oo[0] + 3;  // 4 pixels of one row
#pragma unroll
    for (int a = 0; a < 2; a++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int co = mt * BM + wm * 32 + a * 16 + 4 * g + e;
            if (co >= G.Co) continue;
            const long long cb = co * HW;
            if (S == 1) {
                const float b = bias_at<DT>(bias, bdt, co);
                unsigned v[4];
#pragma unroll
                for (int f = 0; f < 4; f++) v[f] = rnd<DT>(acc[a][f][e] + b);
                uint16_t *p = out + oo[0] + cb;
                if (whole && ((uintptr_t)p & 7) == 0) {
                    *reinterpret_cast<u32x2 *>(p) = u32x2{v[0] | (v[1] << 16), v[2] | (v[3] << 16)};
                } else {
#pragma unroll
                    for (int f = 0; f < 4; f++)
                        if (oo[f] >= 0) out[oo[f] + cb] = (uint16_t)v[f];
                }
            } else {
                float *pp = part + (size_t)s * total + cb;
#pragma unroll
                for (int f = 0; f < 4; f++)
                    if (oo[f] >= 0) pp[oo[f]] = acc[a][f][e];
            }
        }
    }
}

// k_conv_fwd_reduce: grid ceil(total / 256), block 256. One thread per output element: the S partials in split order,
// the bias, one rounding.
template <int DT>
__global__ __launch_bounds__(256) void k_conv_fwd_reduce(const float *__restrict__ part, long long total, int S, int Co,
                                                         long long HW, const void *__restrict__ bias, int bdt,
                                                         uint16_t *__restrict__ out) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    float sum = 0.f;
    for (int s = 0; s < S; s += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = s + u < S ? part[(size_t)(s + u) * total + o] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (s + u < S) sum += v[u];  // (split order)
    }
    out[o] = (uint16_t)rnd<DT>(sum + bias_at<DT>(bias, bdt, (int)((o / HW) % Co)));
}

struct Plan {
    int MT, KCN, S, Wp;
    long long PT, tiles, total, wchunks;
    size_t w_bytes, part_bytes;
};
// Ci / Co: the reduction and the output channels of this direction
inline Plan plan(int N, int Ci, int Co, int H, int W, int ksize) {
    Plan P;
    P.MT = (Co + BM - 1) / BM;
    P.KCN = (Ci + KC - 1) / KC;
    P.Wp = ksize == 3 ? W + 1 : W;
    P.PT = ((long long)N * H * P.Wp + BN - 1) / BN;
    P.tiles = P.PT * P.MT;
    P.total = (long long)N * Co * H * W;
    // S: as many splits as fill the chip's workgroup slots once, each at least MIN_STEPS K steps long
    long long S = P.tiles > 0 ? SLOTS / P.tiles : 1;
    if (S > P.KCN / MIN_STEPS) S = P.KCN / MIN_STEPS;
    if (S > MAX_SPLIT) S = MAX_SPLIT;
    P.S = S < 1 ? 1 : (int)S;
    P.wchunks = (long long)P.MT * P.KCN * ksize * ksize * 256;
    P.w_bytes = (size_t)P.wchunks * 16;
    P.part_bytes = P.S > 1 ? (size_t)P.S * P.total * 4 : 0;
    return P;
}
inline size_t ws_size(int N, int Ci, int Co, int H, int W, int ksize) {
    if (N <= 0 || H <= 0 || W <= 0 || Ci < 0 || Co <= 0 || (ksize != 1 && ksize != 3)) return 0;
    const Plan P = plan(N, Ci, Co, H, W, ksize);
    return ((P.w_bytes + 255) & ~(size_t)255) + P.part_bytes;
}

template <int DT>
int run_t(const char *who, bool dgrad, int wdt, int N, int Cin, int Cout, int H, int W, int ksize, const void *x,
          const void *w, const void *bias, int bdt, void *y, void *workspace, const Plan &P, hipStream_t st) {
    const int Ci = dgrad ? Cout : Cin, Co = dgrad ? Cin : Cout;
    u32x4 *wp = (u32x4 *)workspace;
    float *part = P.S > 1 ? (float *)((char *)workspace + ((P.w_bytes + 255) & ~(size_t)255)) : nullptr;
    if (P.wchunks > 0) {
        const int wgrid = P.MT * P.KCN * 4, flip = dgrad ? 1 : 0;
        lgm::prof_begin("k_conv_wpack", st);
        if (ksize == 3) k_conv_wpack<DT, 3><<<wgrid, 256, 0, st>>>(w, wdt, Cout, Cin, flip, P.KCN, wp);
        else k_conv_wpack<DT, 1><<<wgrid, 256, 0, st>>>(w, wdt, Cout, Cin, flip, P.KCN, wp);
        lgm::prof_end(st);
        LGM_LAUNCH_CHECK("k_conv_wpack");
    }
    Geo G;
    G.Ci = Ci, G.Co = Co, G.H = H, G.W = W, G.Wp = P.Wp;
    G.NR = (long long)N * H, G.HW = (long long)H * W;
    const int grid = (int)(P.tiles * P.S);
    lgm::prof_begin(dgrad ? "k_conv_dgrad" : "k_conv_fwd", st);
    if (ksize == 3)
        k_conv<DT, 3><<<grid, THREADS, 0, st>>>(G, (const uint16_t *)x, wp, bias, bdt, (uint16_t *)y, part, P.total, P.S,
                                               P.MT, P.KCN);
    else
        k_conv<DT, 1><<<grid, THREADS, 0, st>>>(G, (const uint16_t *)x, wp, bias, bdt, (uint16_t *)y, part, P.total, P.S,
                                               P.MT, P.KCN);
    lgm::prof_end(st);
    LGM_LAUNCH_CHECK(who);
    if (P.S > 1)
        LGM_LAUNCH("k_conv_fwd_reduce", st,
                   (k_conv_fwd_reduce<DT><<<(int)((P.total + 255) / 256), 256, 0, st>>>(part, P.total, P.S, Co, G.HW, bias,
                                                                                       bdt, (uint16_t *)y)));
    return LGM_OK;
}

int run(const char *who, bool dgrad, int dtype, int wdt, int N, int Cin, int Cout, int H, int W, int ksize, const void *x,
        const void *w, const void *bias, int bdt, void *y, void *workspace, size_t workspace_bytes, void *stream,
        const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (int rc = lgm::check_dtype16(who, dtype)) return rc;
    if (wdt != LGM_ATTN_F32 && wdt != dtype) {
        lgm::set_error("%s: weight dtype must be fp32 or the operand dtype %d (got %d)", who, dtype, wdt);
        return LGM_E_INVALID;
    }
    if (bias && bdt != LGM_ATTN_F32 && bdt != dtype) {
        lgm::set_error("%s: bias dtype must be fp32 or the operand dtype %d (got %d)", who, dtype, bdt);
        return LGM_E_INVALID;
    }
    if (ksize != 1 && ksize != 3) {
        lgm::set_error("%s: ksize must be 1 or 3 (got %d)", who, ksize);
        return LGM_E_INVALID;
    }
    if (N < 0 || Cin < 0 || Cout < 0 || H < 0 || W < 0) {
        lgm::set_error("%s: negative size N=%d Cin=%d Cout=%d H=%d W=%d", who, N, Cin, Cout, H, W);
        return LGM_E_INVALID;
    }
    const int Ci = dgrad ? Cout : Cin, Co = dgrad ? Cin : Cout;
    if ((long long)N * H * W == 0 || Co == 0) return LGM_OK;
    if (!y || (Ci > 0 && (!x || !w))) {
        lgm::set_error("%s: null pointer", who);
        return LGM_E_INVALID;
    }
    const Plan P = plan(N, Ci, Co, H, W, ksize);
    if (P.tiles * P.S > 2147483647LL || P.wchunks / 256 > 2147483647LL || (long long)P.MT * P.KCN * 4 > 2147483647LL || (P.total + 255) / 256 > 2147483647LL) {
        lgm::set_error("%s: grid beyond 2^31 - 1 workgroups (N=%d Cin=%d Cout=%d H=%d W=%d)", who, N, Cin, Cout, H, W);
        return LGM_E_INVALID;
    }
    const size_t need = ws_size(N, Ci, Co, H, W, ksize);
    if (int rc = lgm::check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LGM_ATTN_BF16)
        return run_t<LGM_ATTN_BF16>(who, dgrad, wdt, N, Cin, Cout, H, W, ksize, x, w, bias, bdt, y, workspace, P, st);
    return run_t<LGM_ATTN_F16>(who, dgrad, wdt, N, Cin, Cout, H, W, ksize, x, w, bias, bdt, y, workspace, P, st);
}

}  // namespace cf
}  // namespace lgm

extern "C" size_t lgm_conv_forward_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize) {
    return lgm::cf::ws_size(N, Cin, Cout, H, W, ksize);
}

extern "C" int lgm_conv_forward(int dtype, int w_dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *x,
                                const void *w, const void *bias, int bias_dtype, void *y, void *workspace,
                                size_t workspace_bytes, void *stream, const lgm_diag *diag) {
    return lgm::cf::run("lgm_conv_forward", false, dtype, w_dtype, N, Cin, Cout, H, W, ksize, x, w, bias, bias_dtype, y,
                        workspace, workspace_bytes, stream, diag);
}

extern "C" size_t lgm_conv_dgrad_workspace_size(int N, int Cin, int Cout, int H, int W, int ksize) {
    return lgm::cf::ws_size(N, Cout, Cin, H, W, ksize);
}

extern "C" int lgm_conv_dgrad(int dtype, int w_dtype, int N, int Cin, int Cout, int H, int W, int ksize, const void *dy,
                              const void *w, void *dx, void *workspace, size_t workspace_bytes, void *stream,
                              const lgm_diag *diag) {
    return lgm::cf::run("lgm_conv_dgrad", true, dtype, w_dtype, N, Cin, Cout, H, W, ksize, dy, w, nullptr, 0, dx, workspace,
                        workspace_bytes, stream, diag);
}
