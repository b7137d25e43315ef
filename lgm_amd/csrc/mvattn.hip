// lgm_amd/csrc/mvattn.hip -- the token layout changes around MVAttention's attention core (core/unet.py:35-49),
// fused with the GroupNorm before and the residual after:
//   k_mva_gn_reg (slab in registers; else k_mva_gn_tok with the slab in LDS, or for slabs beyond LDS k_mva_stats +
//   k_mva_norm)  GroupNorm(x) of [B*F, C, H, W]
//                (core/unet.py:40, fp32 statistics), written straight into the [B, F*H*W, C] token layout of :41-42
//                in the qkv Linear's input dtype (bf16 under autocast): one launch instead of torch's moments /
//                fused-params / normalise launches + the permute copy + the cast.
//   k_mva_out    the [B, F*H*W, C] -> [B*F, C, H, W] permute of :45-46 fused with (x + res) * skip_scale of :47-48.
// and the backward's mirror of both (k_mva_out_bwd, k_mva_gn_part / k_mva_gn_coef / k_mva_gn_dx, below).
// All are HBM-bound layout kernels. The tiled passes (k_mva_out, k_mva_out_bwd, k_mva_gn_part, k_mva_gn_dx) are
// 64 x 64 LDS-tiled transposes, so global reads and writes run along rows; each is ONE kernel with a `bool VEC`
// parameter, written on the two tile fragments ChanFrag / TokFrag: VEC reads channel rows 4 pixels and token rows
// 8 channels per lane (C % 8 == 0, HW % 4 == 0, 16-B aligned tensors: mva_vec_ok; every LGM shape), the scalar form
// takes single elements and serves ragged shapes. The two forms share the tile, the arithmetic and the summation
// order: bitwise equal (tests/test_mva_forms_gpu.py).
#include <initializer_list>
#include <type_traits>

#include "elemwise.h"

namespace lgm {
namespace {

// GroupNorm statistics in two launches, all deterministic:
// k_mva_stats  grid (S, G, B*F): chunk s of group g of sample bf (the group's Cg*HW elements are contiguous) ->
//              its mean and centred sum of squares (two passes over the chunk, which stays in L1/L2).
// k_mva_norm   grid (ceil(HW/64), ceil(C/64), B*F): merges the chunk statistics of the groups its 64 channels
//              belong to (Chan's parallel formula, fixed order), then normalises a 64-channel x 64-pixel tile
//              through LDS: reads along hw, writes token rows along c. y = x (rstd gamma) + (beta - mean rstd gamma),
//              torch's fused GroupNorm parameters.
constexpr int MVA_CHUNK = 4096;  // elements per statistics workgroup

__device__ __forceinline__ int mva_chunks(int n) { return (n + MVA_CHUNK - 1) / MVA_CHUNK; }

template <class TI>
__global__ __launch_bounds__(256) void k_mva_stats(int C, int HW, int G, const TI *__restrict__ x,
                                                   float2 *__restrict__ part) {
    __shared__ float red[4];
    const int s = blockIdx.x, g = blockIdx.y, bf = blockIdx.z, Cg = C / G, tid = threadIdx.x;
    const int n = Cg * HW, S = mva_chunks(n);
    const int i0 = s * MVA_CHUNK, i1 = min(n, i0 + MVA_CHUNK), m = i1 - i0;
    const TI *xg = x + ((size_t)bf * C + (size_t)g * Cg) * HW;
    float v[MVA_CHUNK / 256];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < MVA_CHUNK / 256; k++) {
        const int i = i0 + k * 256 + tid;
        const float t = to_f(xg[i < i1 ? i : i0]);  // unconditional loads (clamped index): all in flight at once
        v[k] = i < i1 ? t : 0.f;
        sum += v[k];
    }
    const float mean = block_sum256(sum, red) / (float)m;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MVA_CHUNK / 256; k++) {
        const float d = i0 + k * 256 + tid < i1 ? v[k] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    q = block_sum256(q, red);
    if (tid == 0) part[((size_t)bf * G + g) * S + s] = make_float2(mean, q);
}

template <class TI, class TO>
__global__ __launch_bounds__(256) void k_mva_norm(int F, int C, int HW, int G, float eps, const TI *__restrict__ x,
                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                  const float2 *__restrict__ part, TO *__restrict__ tok,
                                                  float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    __shared__ float tile[64][65];  // [pixel][channel]
    __shared__ float sa[64], sb[64];
    const int hw0 = blockIdx.x * 64, c0 = blockIdx.y * 64, bf = blockIdx.z, tid = threadIdx.x;
    const int Cg = C / G, n = Cg * HW, S = mva_chunks(n);
    if (tid < 64 && c0 + tid < C) {  // this channel's group statistics (Chan merge of the chunks, in order)
        const int c = c0 + tid, g = c / Cg;
        const float2 *pg = part + ((size_t)bf * G + g) * S;
        float mean = 0.f, M2 = 0.f;
        int cnt = 0;
        for (int s2 = 0; s2 < S; s2++) {
            const float2 p = pg[s2];
            const int m = min(n, (s2 + 1) * MVA_CHUNK) - s2 * MVA_CHUNK;
            const int tot = cnt + m;
            const float d = p.x - mean;
            mean = fmaf(d, (float)m / (float)tot, mean);
            M2 += p.y + d * d * ((float)cnt * (float)m / (float)tot);
            cnt = tot;
        }
        const float rstd = rsqrtf(fmaxf(M2 / (float)n, 0.f) + eps);  // biased variance, as torch
        const float a = rstd * (gamma ? gamma[c] : 1.f);
        sa[tid] = a;
        sb[tid] = (beta ? beta[c] : 0.f) - mean * a;
        if (blockIdx.x == 0 && c % Cg == 0) {  // one writer per (sample, group)
            mean_out[(size_t)bf * G + g] = mean;
            rstd_out[(size_t)bf * G + g] = rstd;
        }
    }
    __syncthreads();
    const TI *xb = x + (size_t)bf * C * HW;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {  // all 16 loads issued before the first use (clamped, unconditional addresses)
        const int i = tid + 256 * k, r = i >> 6, h = i & 63;  // channel r, pixel h
        const bool ok = hw0 + h < HW && c0 + r < C;
        v[k] = to_f(xb[ok ? (size_t)(c0 + r) * HW + hw0 + h : 0]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int i = tid + 256 * k, r = i >> 6, h = i & 63;
        tile[h][r] = fmaf(v[k], sa[r], sb[r]);
    }
    __syncthreads();
    const int b = bf / F, f = bf - b * F;
    TO *tb = tok + ((size_t)b * F * HW + (size_t)f * HW) * C;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int i = tid + 256 * k, r = i >> 6, c = i & 63;  // token row r, channel c
        if (hw0 + r < HW && c0 + c < C) tb[(size_t)(hw0 + r) * C + c0 + c] = from_f<TO>(tile[r][c]);
    }
}

// k_mva_gn_tok  grid (G, B*F), block 512: the same GroupNorm -> tokens in ONE launch where a group's Cg x HW slab
//               fits in LDS (every LGM level: <= 100 KB): the slab is read once into LDS (float4 loads for fp32
//               input), its mean and centred sum of squares reduced in a fixed order (two passes over LDS), then
//               written normalised along the token rows (Cg / 8 x 16-B stores per token). Replaces the chunked
//               statistics launch + the tiled normalise launch (their fixed launch latency dominated LGM's small
//               levels: 600 and 2,400 tokens at C = 1024). cfg4's 16 blocks: GPU span per pass 2.43 -> 2.38 ms
//               (profiles/r05/ab_mva_gn_fused). The slab loads go 8 per thread at a time (the plain loop waited for
//               each before issuing the next): bench level 34.2 -> 32.2 us, cfg4 190.8 -> 182.9 us per pass
//               (profiles/r05/ab_mva_batch); the same for k_mva_gn_coef's tile partials (13.8 -> 11.5 us).
constexpr int GN_THREADS = 512;
constexpr size_t GN_LDS_MAX = 144 * 1024;  // bytes of dynamic LDS the fused form may take

// 8 consecutive channels of a token row: one 16-B store at 16 bits; fp32 stays 8 scalar stores (the token pointer's
// 32-B alignment is not checked on the forward GroupNorm paths)
template <class TO>
__device__ __forceinline__ void store_tok8(TO *dst, const float (&v)[8]) {
    if constexpr (sizeof(TO) == 2) {
        store8<TO>(dst, v);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = v[j];
    }
}

template <class TI, class TO>
__global__ __launch_bounds__(GN_THREADS) void k_mva_gn_tok(int F, int C, int HW, int G, float eps,
                                                            const TI *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, TO *__restrict__ tok,
                                                            float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    extern __shared__ __attribute__((aligned(16))) float slab[];  // [Cg][HW], then a[Cg], b[Cg]
    __shared__ float red[8];
    const int g = blockIdx.x, bf = blockIdx.y, Cg = C / G, n = Cg * HW, tid = threadIdx.x;
    const TI *xg = x + ((size_t)bf * C + (size_t)g * Cg) * HW;
    float s = 0.f;
    if constexpr (sizeof(TI) == 4) {
        if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(xg) & 15) == 0) {
            const float4 *x4 = reinterpret_cast<const float4 *>(xg);
            int i = tid;
            // 8 loads in flight per thread, then their LDS stores and sums in the same order (the plain loop waited
            // for each load before issuing the next)
            for (; i + 7 * GN_THREADS < n / 4; i += 8 * GN_THREADS) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = x4[i + u * GN_THREADS];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    reinterpret_cast<float4 *>(slab)[i + u * GN_THREADS] = v[u];
                    s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
                }
            }
            for (; i < n / 4; i += GN_THREADS) {
                const float4 v = x4[i];
                reinterpret_cast<float4 *>(slab)[i] = v;
                s += (v.x + v.y) + (v.z + v.w);
            }
        } else {
            for (int i = tid; i < n; i += GN_THREADS) { const float v = to_f(xg[i]); slab[i] = v; s += v; }
        }
    } else {
        int i = tid;
        for (; i + 7 * GN_THREADS < n; i += 8 * GN_THREADS) {  // (as above, 16-bit elements)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = to_f(xg[i + u * GN_THREADS]);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                slab[i + u * GN_THREADS] = v[u];
                s += v[u];
            }
        }
        for (; i < n; i += GN_THREADS) { const float v = to_f(xg[i]); slab[i] = v; s += v; }
    }
    const float mean = block_sum512(s, red) / (float)n;
    float q = 0.f;
    for (int i = tid; i < n; i += GN_THREADS) {
        const float d = slab[i] - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = rsqrtf(block_sum512(q, red) / (float)n + eps);  // biased variance, as torch
    float *sa = slab + n, *sb = sa + Cg;
    for (int c = tid; c < Cg; c += GN_THREADS) {
        const float a = rstd * (gamma ? gamma[g * Cg + c] : 1.f);
        sa[c] = a;
        sb[c] = (beta ? beta[g * Cg + c] : 0.f) - mean * a;
    }
    if (tid == 0) {
        mean_out[(size_t)bf * G + g] = mean;
        rstd_out[(size_t)bf * G + g] = rstd;
    }
    __syncthreads();
    const int b = bf / F, f = bf - b * F;
    TO *tb = tok + ((size_t)b * F * HW + (size_t)f * HW) * C + (size_t)g * Cg;
    if ((Cg & 7) == 0) {  // 8 channels per thread: one 16-B (bf16) / 32-B (fp32) store
        const int c8n = Cg / 8;
        for (int p = tid; p < HW * c8n; p += GN_THREADS) {
            const int hw = p / c8n, c0 = (p - hw * c8n) * 8;
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = fmaf(slab[(c0 + j) * HW + hw], sa[c0 + j], sb[c0 + j]);
            store_tok8<TO>(tb + (size_t)hw * C + c0, o);
        }
    } else {
        for (int p = tid; p < HW * Cg; p += GN_THREADS) {
            const int hw = p / Cg, c = p - hw * Cg;
            tb[(size_t)hw * C + c] = from_f<TO>(fmaf(slab[c * HW + hw], sa[c], sb[c]));
        }
    }
}

// k_mva_gn_reg  grid (G, B*F), block 512: the one-launch GroupNorm -> tokens with the group's slab in REGISTERS
//               instead of LDS, for Cg % 8 == 0 channels, HW % 4 == 0 and <= GNR_K * 512 items (every LGM level). An
//               item is 8 channel rows x 4 pixels: thread t holds items t + 512 k (channel block fastest, so the lanes
//               of one pixel quad write adjacent 16 B of each token row), loaded as one 4-pixel vector per channel row,
//               all in flight at once; the statistics are
//               reduced in a fixed order (two passes over the registers); each pixel of an item is written as one
//               token-row store of 8 channels. No LDS slab, so LDS does not cap the launch at two workgroups per CU.
//               Against k_mva_gn_tok: bench level 31.8 -> 29.5 us, cfg4 184.4 -> 153.3 us per pass (its C = 512 level
//               has 192 workgroups: all loads in flight at once matters most there; profiles/r05/ab_mva_gn_reg).
constexpr int GNR_K = 2;  // items per thread (64 registers of slab)
template <class TI, class TO>
__global__ __launch_bounds__(GN_THREADS) void k_mva_gn_reg(int F, int C, int HW, int G, float eps,
                                                            const TI *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, TO *__restrict__ tok,
                                                            float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    __shared__ float red[8];
    __shared__ float sab[2][256];  // per channel of the group: a = rstd gamma, b = beta - mean a (Cg <= 256)
    const int g = blockIdx.x, bf = blockIdx.y, Cg = C / G, tid = threadIdx.x;
    const int nCB = Cg / 8, nit = nCB * (HW / 4);  // items (channel block fastest: lane pairs share a pixel quad)
    const TI *xg = x + ((size_t)bf * C + (size_t)g * Cg) * HW;
    float v[GNR_K][8][4];
#pragma unroll
    for (int k = 0; k < GNR_K; k++) {
        const int it = tid + GN_THREADS * k;
        const int p4 = it / nCB, cb = it - p4 * nCB;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (it < nit) load4<TI>(xg + (size_t)(8 * cb + j) * HW + 4 * p4, v[k][j]);
            else v[k][j][0] = v[k][j][1] = v[k][j][2] = v[k][j][3] = 0.f;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < GNR_K; k++)
#pragma unroll
        for (int j = 0; j < 8; j++) s += (v[k][j][0] + v[k][j][1]) + (v[k][j][2] + v[k][j][3]);  // (past nit: 0)
    const float n = (float)Cg * (float)HW;
    const float mean = block_sum512(s, red) / n;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < GNR_K; k++) {
        if (tid + GN_THREADS * k < nit) {
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float d = v[k][j][e] - mean;
                    q = fmaf(d, d, q);
                }
        }
    }
    const float rstd = rsqrtf(block_sum512(q, red) / n + eps);  // biased variance, as torch
    for (int c = tid; c < Cg; c += GN_THREADS) {
        const float a = rstd * (gamma ? gamma[g * Cg + c] : 1.f);
        sab[0][c] = a;
        sab[1][c] = (beta ? beta[g * Cg + c] : 0.f) - mean * a;
    }
    if (tid == 0) {
        mean_out[(size_t)bf * G + g] = mean;
        rstd_out[(size_t)bf * G + g] = rstd;
    }
    __syncthreads();
    const int b = bf / F, f = bf - b * F;
    TO *tb = tok + ((size_t)b * F * HW + (size_t)f * HW) * C + (size_t)g * Cg;
#pragma unroll
    for (int k = 0; k < GNR_K; k++) {
        const int it = tid + GN_THREADS * k;
        if (it < nit) {
            const int p4 = it / nCB, cb = it - p4 * nCB;
            float a8[8], b8[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                a8[j] = sab[0][8 * cb + j];
                b8[j] = sab[1][8 * cb + j];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] = fmaf(v[k][j][e], a8[j], b8[j]);
                store_tok8<TO>(tb + (size_t)(4 * p4 + e) * C + 8 * cb, o);
            }
        }
    }
}

// ---- the tiled passes: grid (ceil(HW/64), ceil(C/64), B*F), block 256, one 64-channel x 64-pixel tile per workgroup.
// A fragment is a thread's 16 elements of that tile in the order of its global accesses: ChanFrag along hw (the
// [B*F, C, HW] tensors), TokFrag along c (the [B, F*HW, C] tokens). at(n, t) places element v[n]; load only issues
// loads, every one unconditional (lanes outside the tensor on a clamped in-range address, their values never used:
// masking happens at put / store), so all loads of a kernel go out before its first wait; put writes the fragment to
// the [64][65] LDS tile in its own orientation, zero outside the tensor; store is masked.
struct Tile {
    int F, C, HW, bf, hw0, c0;
};
__device__ __forceinline__ Tile this_tile(int F, int C, int HW) {
    return {F, C, HW, (int)blockIdx.z, (int)blockIdx.x * 64, (int)blockIdx.y * 64};
}
struct Pos {
    int r, j;  // row of the fragment's orientation, position along it
    bool ok;   // inside the tensor
};

// VEC: 4 accesses of 4 pixels (channel row i >> 4, pixels 4 (i & 15) ..); scalar: 16 of 1 (row i >> 6, pixel i & 63)
template <bool VEC>
struct ChanFrag {
    static constexpr int W = VEC ? 4 : 1;
    float v[16];
    static __device__ __forceinline__ Pos at(int n, const Tile &t) {  // r: channel, j: pixel
        const int i = threadIdx.x + 256 * (n / W);
        const int r = VEC ? i >> 4 : i >> 6, h = VEC ? 4 * (i & 15) + n % W : i & 63;
        return {r, h, t.c0 + r < t.C && t.hw0 + h < t.HW};
    }
    static __device__ __forceinline__ size_t offset(const Pos &p, const Tile &t) {
        return ((size_t)t.bf * t.C + t.c0 + p.r) * t.HW + t.hw0 + p.j;
    }
    template <class T>
    __device__ __forceinline__ void load(const T *__restrict__ x, const Tile &t) {
#pragma unroll
        for (int n = 0; n < 16; n += W) {
            const Pos p = at(n, t);
            const T *src = x + (p.ok ? offset(p, t) : 0);
            if constexpr (VEC) load4<T>(src, v + n);
            else v[n] = to_f(*src);
        }
    }
    template <class T>
    __device__ __forceinline__ void store1(T *__restrict__ x, const Tile &t, int n) const {  // the access at v[n]
        const Pos p = at(n, t);
        if (!p.ok) return;
        if constexpr (VEC) store4<T>(x + offset(p, t), v + n);
        else x[offset(p, t)] = from_f<T>(v[n]);
    }
    template <class T>
    __device__ __forceinline__ void store(T *__restrict__ x, const Tile &t) const {
#pragma unroll
        for (int n = 0; n < 16; n += W) store1(x, t, n);
    }
    __device__ __forceinline__ void put(float (&tile)[64][65], const Tile &t) const {  // [channel][pixel]
#pragma unroll
        for (int n = 0; n < 16; n++) {
            const Pos p = at(n, t);
            tile[p.r][p.j] = p.ok ? v[n] : 0.f;
        }
    }
};

// VEC: 2 accesses of 8 channels (token row i >> 3, channels 8 (i & 7) ..); scalar: 16 of 1 (row i >> 6, channel i & 63)
template <bool VEC>
struct TokFrag {
    static constexpr int W = VEC ? 8 : 1;
    float v[16];
    static __device__ __forceinline__ Pos at(int n, const Tile &t) {  // r: token row (pixel), j: channel
        const int i = threadIdx.x + 256 * (n / W);
        const int r = VEC ? i >> 3 : i >> 6, c = VEC ? 8 * (i & 7) + n % W : i & 63;
        return {r, c, t.hw0 + r < t.HW && t.c0 + c < t.C};
    }
    static __device__ __forceinline__ size_t offset(const Pos &p, const Tile &t) {
        const int b = t.bf / t.F, f = t.bf - b * t.F;
        return ((size_t)b * t.F * t.HW + (size_t)f * t.HW + t.hw0 + p.r) * t.C + t.c0 + p.j;
    }
    template <class T>
    __device__ __forceinline__ void load(const T *__restrict__ tok, const Tile &t) {
#pragma unroll
        for (int n = 0; n < 16; n += W) {
            const Pos p = at(n, t);
            const T *src = tok + (p.ok ? offset(p, t) : 0);
            if constexpr (VEC) load8<T>(src, v + n);
            else v[n] = to_f(*src);
        }
    }
    template <class T>
    __device__ __forceinline__ void store(T *__restrict__ tok, const Tile &t) const {
#pragma unroll
        for (int n = 0; n < 16; n += W) {
            const Pos p = at(n, t);
            if (!p.ok) continue;
            if constexpr (VEC) store8<T>(tok + offset(p, t), v + n);
            else tok[offset(p, t)] = from_f<T>(v[n]);
        }
    }
    __device__ __forceinline__ void put(float (&tile)[64][65], const Tile &t) const {  // [pixel][channel]
#pragma unroll
        for (int n = 0; n < 16; n++) {
            const Pos p = at(n, t);
            tile[p.r][p.j] = p.ok ? v[n] : 0.f;
        }
    }
};

// k_mva_out: out[bf][c][hw] = (y[b][f HW + hw][c] + res[bf][c][hw]) * skip (reads along c, writes along hw); the
// residual's loads go out with the tokens' (one round trip). In a lower-precision output the sum is rounded before
// the scale, as torch's two ops do. Vector against scalar accesses: bench level 37.0 -> 31.2 us, cfg4 171.6 ->
// 141.0 us per pass (profiles/r05/ab_mva_vec).
template <class TY, class TR, class TO, bool VEC>
__global__ __launch_bounds__(256) void k_mva_out(int F, int C, int HW, const TY *__restrict__ y,
                                                 const TR *__restrict__ res, float skip, TO *__restrict__ out) {
    __shared__ float tile[64][65];  // [channel][pixel]
    const Tile t = this_tile(F, C, HW);
    TokFrag<VEC> yv;
    ChanFrag<VEC> ov;  // the residual, then the output
    yv.load(y, t);
    if (res) ov.load(res, t);
#pragma unroll
    for (int n = 0; n < 16; n++) {
        const Pos p = TokFrag<VEC>::at(n, t);
        tile[p.j][p.r] = yv.v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 16; n++) {
        const Pos p = ChanFrag<VEC>::at(n, t);
        float s = tile[p.r][p.j];
        if (res) {
            s += ov.v[n];
            s = to_f(from_f<TO>(s));  // (exact for an fp32 output)
            s *= skip;
        }
        ov.v[n] = s;
    }
    ov.store(out, t);
}

// ---- backward (core/unet.py:40-48 backward), the mirror of the two passes above:
// k_mva_out_bwd   g = dL/dout * scale (rounded to out's dtype, as torch's `d_out * skip`), written to d_res
//                 [B*F, C, H, W] along hw and, through the LDS tile, to the tokens' gradient d_y [B, F*H*W, C] along c.
// k_mva_gn_part   per (sample, channel, 64-pixel tile) partial sums of dy * x and dy (dy = the token gradient read
//                 back through the LDS tile) -> part2
// k_mva_gn_coef   grid (G): per (sample, channel) ds = sum dy x, db = sum dy (fixed order over the tiles), then per
//                 (sample, group) torch's fused backward parameters c2, c3 and per channel dgamma, dbeta (fixed
//                 order over the samples): deterministic
// k_mva_gn_dx     dx = rstd gamma dy + c2 x + c3 (+ d_res), one rounding to x's dtype: the GroupNorm backward and
//                 autograd's sum with the residual's gradient in one pass.
// Vector against scalar accesses, bench level (C = 512, 32 x 32, 32 samples): k_mva_out_bwd 36.0 -> 31.8 us,
// k_mva_gn_part 25.3 -> 23.3 us, k_mva_gn_dx 40.8 -> 40.2 us (profiles/r05/ab_mva_vecb).
template <class TD, class TY, class TR, bool VEC>
__global__ __launch_bounds__(256) void k_mva_out_bwd(int F, int C, int HW, const TD *__restrict__ dout, float scale,
                                                     TY *__restrict__ dy, TR *__restrict__ dres) {
    __shared__ float tile[64][65];  // [channel][pixel]
    const Tile t = this_tile(F, C, HW);
    ChanFrag<VEC> g;
    g.load(dout, t);
#pragma unroll
    for (int n0 = 0; n0 < 16; n0 += ChanFrag<VEC>::W) {  // per access: its d_res store goes out once its load is back
#pragma unroll
        for (int n = n0; n < n0 + ChanFrag<VEC>::W; n++) {
            const Pos p = ChanFrag<VEC>::at(n, t);
            g.v[n] = to_f(from_f<TD>(g.v[n] * scale));  // (exact: scale 1 and an fp32 gradient)
            tile[p.r][p.j] = g.v[n];
        }
        if (dres) g.store1(dres, t, n0);
    }
    __syncthreads();
    TokFrag<VEC> dv;
#pragma unroll
    for (int n = 0; n < 16; n++) {
        const Pos p = TokFrag<VEC>::at(n, t);
        dv.v[n] = tile[p.j][p.r];
    }
    dv.store(dy, t);
}

template <class TI, class TT, bool VEC>
__global__ __launch_bounds__(256) void k_mva_gn_part(int F, int C, int HW, const TI *__restrict__ x,
                                                     const TT *__restrict__ dtok, float2 *__restrict__ part) {
    __shared__ float tile[64][65];  // dy [pixel][channel]
    __shared__ float xs[64][65];    // x [channel][pixel]
    __shared__ float2 red[4][64];
    const Tile t = this_tile(F, C, HW);
    const int tid = threadIdx.x, nT = gridDim.x;
    {
        ChanFrag<VEC> xv;
        TokFrag<VEC> dv;
        xv.load(x, t);
        dv.load(dtok, t);
        xv.put(xs, t);
        dv.put(tile, t);
    }
    __syncthreads();
    // thread: channel c = tid & 63, pixels 16 q .. 16 q + 15 (q = the wave); the four quarters summed in order
    const int c = tid & 63, q = tid >> 6;
    float sdx = 0.f, sd = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int h = 16 * q + k;
        const float g = tile[h][c];
        sd += g;
        sdx = fmaf(g, xs[c][h], sdx);
    }
    red[q][c] = make_float2(sdx, sd);
    __syncthreads();
    if (tid < 64 && t.c0 + tid < C) {
        const float2 a = red[0][tid], b2 = red[1][tid], c2 = red[2][tid], d2 = red[3][tid];
        part[((size_t)t.bf * C + t.c0 + tid) * nT + blockIdx.x] =
            make_float2((a.x + b2.x) + (c2.x + d2.x), (a.y + b2.y) + (c2.y + d2.y));
    }
}

constexpr int GN_NMAX = 2048;  // (sample, channel) pairs of one group held in LDS at a time
constexpr int GN_CPT = GN_NMAX / 256;  // channels per thread of k_mva_gn_coef (any Cg <= GN_NMAX)
__global__ __launch_bounds__(256) void k_mva_gn_coef(int BF, int C, int HW, int G, int nT,
                                                     const float2 *__restrict__ part, const float *__restrict__ gamma,
                                                     const float *__restrict__ mean, const float *__restrict__ rstd,
                                                     float2 *__restrict__ coef, float *__restrict__ dgamma,
                                                     float *__restrict__ dbeta) {
    __shared__ float2 sdb[GN_NMAX];  // (ds, db) of the chunk's (sample, channel) pairs
    const int g = blockIdx.x, Cg = C / G, tid = threadIdx.x;
    const float s = 1.f / ((float)Cg * (float)HW);
    const int nchunk = max(1, GN_NMAX / Cg);  // samples per LDS chunk
    // this thread's channels tid + 256 k (k < GN_CPT, Cg <= GN_NMAX), each summed over the samples in order
    float dg[GN_CPT], dbt[GN_CPT];
#pragma unroll
    for (int k = 0; k < GN_CPT; k++) dg[k] = dbt[k] = 0.f;
    for (int n0 = 0; n0 < BF; n0 += nchunk) {
        const int n1 = min(BF, n0 + nchunk), items = (n1 - n0) * Cg;
        for (int it = tid; it < items; it += 256) {
            const int n = n0 + it / Cg, c = g * Cg + it % Cg;
            const float2 *pp = part + ((size_t)n * C + c) * nT;
            float a = 0.f, b = 0.f;
            int t = 0;
            for (; t + 8 <= nT; t += 8) {  // 8 loads in flight, then the sums in the same fixed order
                float2 p[8];
#pragma unroll
                for (int u = 0; u < 8; u++) p[u] = pp[t + u];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    a += p[u].x;
                    b += p[u].y;
                }
            }
            for (; t < nT; t++) {  // fixed order over the pixel tiles
                const float2 p = pp[t];
                a += p.x;
                b += p.y;
            }
            sdb[it] = make_float2(a, b);
        }
        __syncthreads();
        for (int n = n0 + tid; n < n1; n += 256) {  // per sample: torch's fused backward parameters
            float sum1 = 0.f, sum2 = 0.f;
            for (int cc = 0; cc < Cg; cc++) {
                const float ga = gamma ? gamma[g * Cg + cc] : 1.f;
                const float2 v = sdb[(n - n0) * Cg + cc];
                sum1 = fmaf(v.x, ga, sum1);
                sum2 = fmaf(v.y, ga, sum2);
            }
            const float mu = mean[(size_t)n * G + g], rs = rstd[(size_t)n * G + g];
            const float c2 = (sum2 * mu - sum1) * rs * rs * rs * s;
            const float c3 = -c2 * mu - sum2 * rs * s;
            coef[(size_t)n * G + g] = make_float2(c2, c3);
        }
#pragma unroll
        for (int k = 0; k < GN_CPT; k++) {  // per channel: dgamma, dbeta over this chunk's samples, in order
            const int c = tid + 256 * k;
            if (c < Cg) {
                for (int n = n0; n < n1; n++) {
                    const float2 v = sdb[(n - n0) * Cg + c];
                    const float mu = mean[(size_t)n * G + g], rs = rstd[(size_t)n * G + g];
                    dg[k] = fmaf(v.x - v.y * mu, rs, dg[k]);
                    dbt[k] += v.y;
                }
            }
        }
        __syncthreads();  // (sdb is rewritten by the next chunk)
    }
#pragma unroll
    for (int k = 0; k < GN_CPT; k++) {
        const int c = tid + 256 * k;
        if (c < Cg) {
            if (dgamma) dgamma[g * Cg + c] = dg[k];
            if (dbeta) dbeta[g * Cg + c] = dbt[k];
        }
    }
}

template <class TI, class TT, class TR, bool VEC>
__global__ __launch_bounds__(256) void k_mva_gn_dx(int F, int C, int HW, int G, const TI *__restrict__ x,
                                                   const TT *__restrict__ dtok, const TR *__restrict__ dres,
                                                   const float *__restrict__ gamma, const float *__restrict__ rstd,
                                                   const float2 *__restrict__ coef, TI *__restrict__ dx) {
    __shared__ float tile[64][65];  // [pixel][channel]
    __shared__ float sa[64], sb[64], sc[64];
    const Tile t = this_tile(F, C, HW);
    const int tid = threadIdx.x, Cg = C / G;
    TokFrag<VEC> dv;
    ChanFrag<VEC> xv, rv;  // xv: x, then dx
    dv.load(dtok, t);
    xv.load(x, t);
    if (dres) {
        rv.load(dres, t);
    } else {
#pragma unroll
        for (int n = 0; n < 16; n++) rv.v[n] = 0.f;
    }
    if (tid < 64 && t.c0 + tid < C) {
        const int c = t.c0 + tid, g = c / Cg;
        const float2 k = coef[(size_t)t.bf * G + g];
        sa[tid] = rstd[(size_t)t.bf * G + g] * (gamma ? gamma[c] : 1.f);
        sb[tid] = k.x;
        sc[tid] = k.y;
    }
    dv.put(tile, t);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 16; n++) {
        const Pos p = ChanFrag<VEC>::at(n, t);
        xv.v[n] = fmaf(sa[p.r], tile[p.j][p.r], fmaf(sb[p.r], xv.v[n], sc[p.r])) + rv.v[n];
    }
    xv.store(dx, t);
}

// ---- host side
// the one predicate of the vector forms: rows of whole accesses, every tensor 16-B aligned (null: not used)
bool mva_vec_ok(int C, int HW, std::initializer_list<const void *> ps) {
    if (C % 8 || HW % 4) return false;
    for (const void *p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}
template <class Fn>
int with_vec(bool vec, Fn &&fn) {  // fn(std::bool_constant<vec>{})
    return vec ? fn(std::true_type{}) : fn(std::false_type{});
}

template <class TI, class TO>
int launch_norm(int B, int F, int C, int HW, int G, float eps, const void *x, const float *gamma, const float *beta,
                void *tok, float *mean, float *rstd, float2 *part, hipStream_t st) {
    const int Cg = C / G;
    if (Cg % 8 == 0 && Cg <= 256 && HW % 4 == 0 &&
        (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (long long)(Cg / 8) * (HW / 4) <= (long long)GNR_K * GN_THREADS) {
        LGM_LAUNCH("k_mva_gn_reg", st, (k_mva_gn_reg<TI, TO><<<dim3(G, B * F), GN_THREADS, 0, st>>>(
                                           F, C, HW, G, eps, (const TI *)x, gamma, beta, (TO *)tok, mean, rstd)));
        return LGM_OK;
    }
    const size_t lds = ((size_t)(C / G) * HW + 2 * (C / G)) * sizeof(float);
    if (lds <= GN_LDS_MAX) {  // one launch: the group's slab in LDS
        // the kernel's dynamic LDS limit is raised on every launch of this path: the attribute belongs to the current
        // device, and a process-wide "already set" flag would skip it on a second device (and race between threads);
        // the call is a host-side table update, no device work (include/lgm_attn.h, threading note)
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mva_gn_tok<TI, TO>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GN_LDS_MAX) != hipSuccess) {
            set_error("hipFuncSetAttribute(k_mva_gn_tok) failed");
            return LGM_E_HIP;
        }
        LGM_LAUNCH("k_mva_gn_tok", st, (k_mva_gn_tok<TI, TO><<<dim3(G, B * F), GN_THREADS, lds, st>>>(
                                           F, C, HW, G, eps, (const TI *)x, gamma, beta, (TO *)tok, mean, rstd)));
        return LGM_OK;
    }
    const int S = (C / G * HW + MVA_CHUNK - 1) / MVA_CHUNK;  // larger slabs: chunked statistics + tiled normalise
    LGM_LAUNCH("k_mva_stats", st,
               (k_mva_stats<TI><<<dim3(S, G, B * F), 256, 0, st>>>(C, HW, G, (const TI *)x, part)));
    const dim3 grid((HW + 63) / 64, (C + 63) / 64, B * F);
    LGM_LAUNCH("k_mva_norm", st, (k_mva_norm<TI, TO><<<grid, 256, 0, st>>>(F, C, HW, G, eps, (const TI *)x, gamma,
                                                                            beta, part, (TO *)tok, mean, rstd)));
    return LGM_OK;
}

size_t gn_part_bytes(int BF, int C, int HW) { return (((size_t)BF * C * ((HW + 63) / 64) * sizeof(float2)) + 255) & ~(size_t)255; }

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_mva_backward_workspace_size(int B, int F, int C, int HW, int groups) {
    if (B <= 0 || F <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups) return 0;
    return lgm::gn_part_bytes(B * F, C, HW) + (size_t)B * F * groups * sizeof(float2);
}

extern "C" int lgm_mva_tokens_out_backward(int dtype_dout, int dtype_dy, int dtype_dres, int B, int F, int C, int HW,
                                           const void *d_out, float scale, void *d_y, void *d_res, void *stream,
                                           const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (B < 0 || F <= 0 || C <= 0 || HW < 0) {
        lgm::set_error("lgm_mva_tokens_out_backward: bad shape B=%d F=%d C=%d HW=%d", B, F, C, HW);
        return LGM_E_INVALID;
    }
    if (B == 0 || HW == 0) return LGM_OK;
    if (!d_out || !d_y) {
        lgm::set_error("lgm_mva_tokens_out_backward: null pointer");
        return LGM_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((HW + 63) / 64, (C + 63) / 64, B * F);
    const char *who = "lgm_mva_tokens_out_backward";
    return lgm::with_type(who, dtype_dout, [&](auto td) {
        using TD = decltype(td);
        return lgm::with_type(who, dtype_dy, [&](auto ty) {
            using TY = decltype(ty);
            return lgm::with_type(who, d_res ? dtype_dres : LGM_ATTN_F32, [&](auto tr) {  // (no d_res: not used)
                using TR = decltype(tr);
                return lgm::with_vec(lgm::mva_vec_ok(C, HW, {d_out, d_y, d_res}), [&](auto vec) {
                    LGM_LAUNCH("k_mva_out_bwd", st,
                               (lgm::k_mva_out_bwd<TD, TY, TR, decltype(vec)::value><<<grid, 256, 0, st>>>(
                                   F, C, HW, (const TD *)d_out, scale, (TY *)d_y, (TR *)d_res)));
                    return LGM_OK;
                });
            });
        });
    });
}

extern "C" int lgm_mva_norm_tokens_backward(int dtype_x, int dtype_tok, int B, int F, int C, int HW, int groups,
                                            const void *x, const float *gamma, const float *mean, const float *rstd,
                                            const void *d_tokens, const void *d_res, void *dx, float *dgamma,
                                            float *dbeta, void *workspace, size_t workspace_bytes, void *stream,
                                            const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (B < 0 || F <= 0 || C <= 0 || HW < 0 || groups <= 0 || C % groups || C / groups > lgm::GN_NMAX) {
        lgm::set_error("lgm_mva_norm_tokens_backward: bad shape B=%d F=%d C=%d HW=%d groups=%d (channels per group "
                       "<= %d)", B, F, C, HW, groups, lgm::GN_NMAX);
        return LGM_E_INVALID;
    }
    if (B == 0 || HW == 0) return LGM_OK;
    if (!x || !mean || !rstd || !d_tokens || !workspace) {
        lgm::set_error("lgm_mva_norm_tokens_backward: null pointer");
        return LGM_E_INVALID;
    }
    if (workspace_bytes < lgm_mva_backward_workspace_size(B, F, C, HW, groups)) {
        lgm::set_error("lgm_mva_norm_tokens_backward: workspace too small");
        return LGM_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int BF = B * F, nT = (HW + 63) / 64;
    float2 *part = (float2 *)workspace;
    float2 *coef = (float2 *)((char *)workspace + lgm::gn_part_bytes(BF, C, HW));
    const dim3 grid(nT, (C + 63) / 64, BF);
    const char *who = "lgm_mva_norm_tokens_backward";
    return lgm::with_type(who, dtype_x, [&](auto tx) {
        using TI = decltype(tx);
        return lgm::with_type(who, dtype_tok, [&](auto tt) {
            using TT = decltype(tt);
            return lgm::with_vec(lgm::mva_vec_ok(C, HW, {x, d_tokens, d_res, dx}), [&](auto vec) {
                constexpr bool VEC = decltype(vec)::value;
                LGM_LAUNCH("k_mva_gn_part", st, (lgm::k_mva_gn_part<TI, TT, VEC><<<grid, 256, 0, st>>>(
                                                     F, C, HW, (const TI *)x, (const TT *)d_tokens, part)));
                LGM_LAUNCH("k_mva_gn_coef", st,
                           (lgm::k_mva_gn_coef<<<groups, 256, 0, st>>>(BF, C, HW, groups, nT, part, gamma, mean, rstd,
                                                                       coef, dgamma, dbeta)));
                if (dx)
                    LGM_LAUNCH("k_mva_gn_dx", st, (lgm::k_mva_gn_dx<TI, TT, TI, VEC><<<grid, 256, 0, st>>>(
                                                       F, C, HW, groups, (const TI *)x, (const TT *)d_tokens,
                                                       (const TI *)d_res, gamma, rstd, coef, (TI *)dx)));
                return LGM_OK;
            });
        });
    });
}

extern "C" size_t lgm_mva_workspace_size(int B, int F, int C, int HW, int groups) {
    if (B <= 0 || F <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups) return 0;
    const size_t S = ((size_t)(C / groups) * HW + lgm::MVA_CHUNK - 1) / lgm::MVA_CHUNK;
    return (size_t)B * F * groups * S * sizeof(float2);
}

extern "C" int lgm_mva_norm_tokens(int dtype_x, int dtype_tok, int B, int F, int C, int HW, int groups, float eps,
                                   const void *x, const float *gamma, const float *beta, void *tokens, float *mean,
                                   float *rstd, void *workspace, size_t workspace_bytes, void *stream,
                                   const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (B < 0 || F <= 0 || C <= 0 || HW < 0 || groups <= 0 || C % groups) {
        lgm::set_error("lgm_mva_norm_tokens: bad shape B=%d F=%d C=%d HW=%d groups=%d", B, F, C, HW, groups);
        return LGM_E_INVALID;
    }
    if (B == 0 || HW == 0) return LGM_OK;
    if (!x || !tokens || !mean || !rstd || !workspace) {
        lgm::set_error("lgm_mva_norm_tokens: null pointer");
        return LGM_E_INVALID;
    }
    if (workspace_bytes < lgm_mva_workspace_size(B, F, C, HW, groups)) {
        lgm::set_error("lgm_mva_norm_tokens: workspace too small");
        return LGM_E_WORKSPACE;
    }
    float2 *part = (float2 *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const char *who = "lgm_mva_norm_tokens";
    return lgm::with_type(who, dtype_x, [&](auto tx) {
        return lgm::with_type(who, dtype_tok, [&](auto tt) {
            return lgm::launch_norm<decltype(tx), decltype(tt)>(B, F, C, HW, groups, eps, x, gamma, beta, tokens, mean,
                                                                rstd, part, st);
        });
    });
}

extern "C" int lgm_mva_tokens_out(int dtype_y, int dtype_res, int dtype_out, int B, int F, int C, int HW,
                                  const void *y, const void *res, float skip, void *out, void *stream,
                                  const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    if (B < 0 || F <= 0 || C <= 0 || HW < 0) {
        lgm::set_error("lgm_mva_tokens_out: bad shape B=%d F=%d C=%d HW=%d", B, F, C, HW);
        return LGM_E_INVALID;
    }
    if (B == 0 || HW == 0) return LGM_OK;
    if (!y || !out) {
        lgm::set_error("lgm_mva_tokens_out: null pointer");
        return LGM_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((HW + 63) / 64, (C + 63) / 64, B * F);
    const char *who = "lgm_mva_tokens_out";
    return lgm::with_type(who, dtype_y, [&](auto ty) {
        using TY = decltype(ty);
        return lgm::with_type(who, res ? dtype_res : LGM_ATTN_F32, [&](auto tr) {  // (no residual: not used)
            using TR = decltype(tr);
            return lgm::with_type(who, dtype_out, [&](auto to) {
                using TO = decltype(to);
                return lgm::with_vec(lgm::mva_vec_ok(C, HW, {y, res, out}), [&](auto vec) {
                    LGM_LAUNCH("k_mva_out", st, (lgm::k_mva_out<TY, TR, TO, decltype(vec)::value><<<grid, 256, 0, st>>>(
                                                    F, C, HW, (const TY *)y, (const TR *)res, skip, (TO *)out)));
                    return LGM_OK;
                });
            });
        });
    });
}
