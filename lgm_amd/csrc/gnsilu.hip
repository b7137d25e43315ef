// lgm_amd/csrc/gnsilu.hip -- GroupNorm -> SiLU (-> 2x nearest upsample | 2x2 average pool) of the UNet's ResnetBlocks
// and norm_out (core/unet.py:89-98, :315-316) in NCHW, one pass per direction (include/lgm_norm.h).
//
// Forward, two regimes (as mvattn.hip):
//   k_gns_slab   grid (N*G), block 256: one (sample, group)'s Cg x HW slab is read once into LDS as fp32 (<= GNS_SLAB_MAX
//                elements), its statistics reduced in a fixed order (mean, then centred sums), and the activation written.
//                Taken when the slab fits and the launch fills the chip (>= GNS_FILL workgroups) or the slab is no
//                larger than one chunk (the chunked path would launch no more workgroups for it).
//   k_gns_stats  grid (N*G*S), block 256: chunk s (GNS_CHUNK elements, held in registers) of a group's contiguous slab ->
//                its mean and centred sum of squares;
//   k_gns_norm   block 256: a team of LP lanes merges its group's chunk statistics (Chan's formula, in order, in fp64: a
//                few scalar operations) and writes one tile (4 LP items) of one channel plane.
// Backward (the plan of k_mva_gn_part / k_mva_gn_coef / k_mva_gn_dx):
//   k_gns_bwd_part  per (plane, tile): dz of its items -> partial sums of dz (x - mean) and dz;
//   k_gns_bwd_coef  grid (G): the partials summed per (sample, channel) in tile order, then per (sample, group) the
//                   coefficients of dx and per channel dgamma, dbeta over the samples in order;
//   k_gns_bwd_dx    per (plane, tile): dx = rstd gamma dz + c2 (x - mean) + c3, one rounding.
// The elementwise passes run in teams of LP = 16, 64 or 256 lanes per (plane, tile), chosen by the plane's item count
// (<= 64, <= 256, more): the 8 x 8 and 16 x 16 planes of LGM's inner levels share a workgroup, 16 or 4 planes each.
// An item is what one thread handles at a time: with vector accesses (16-byte aligned tensors, rows of 4 / 8 elements)
// 4 input pixels (NONE, UP2: 2 x 8 outputs) or 2 x 8 input pixels (DOWN2: 4 outputs); otherwise 1 input pixel or one
// 2 x 2 input block. The _v / _s suffix of the kernel names (and 16 / 64 after it, the team) tells which form ran. Everything is written about
// (x - mean): a large mean costs no precision (no E[x^2] - E[x]^2, no a x + b with b ~ -mean a).
#include <type_traits>

#include "elemwise.h"
#include "lgm_norm.h"

namespace lgm {
namespace {

constexpr int GNS_THREADS = 256;
constexpr int GNS_CHUNK = 4096;     // elements per statistics workgroup (16 per thread, in registers)
constexpr int GNS_SLAB_MAX = 8192;  // elements of a (sample, group) slab the one-launch form holds in LDS (32 KB)
constexpr int GNS_FILL = 256;       // workgroups that fill the chip (one per CU)
constexpr int GNS_UNROLL = 4;       // items per thread of the elementwise passes
constexpr int GNS_TILE = GNS_THREADS * GNS_UNROLL;  // items per workgroup of the elementwise passes

// the sum over a team of LP consecutive lanes (16 or 64: shuffles inside the wave; 256: the workgroup), fixed order
template <int LP>
__device__ __forceinline__ float team_sum(float v, float *red) {
    if constexpr (LP == GNS_THREADS) {
        return block_sum256(v, red);
    } else {
#pragma unroll
        for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
}

// WN consecutive elements: 4-element vectors where WN is a multiple of 4 (the caller guarantees the alignment)
template <class T, int WN>
__device__ __forceinline__ void ld_row(const T *p, float *o) {
    if constexpr (WN % 4 == 0) {
#pragma unroll
        for (int q = 0; q < WN / 4; q++) load4<T>(p + 4 * q, o + 4 * q);
    } else {
#pragma unroll
        for (int j = 0; j < WN; j++) o[j] = to_f(p[j]);
    }
}
template <class T, int WN>
__device__ __forceinline__ void st_row(T *p, const float *v) {
    if constexpr (WN % 4 == 0) {
#pragma unroll
        for (int q = 0; q < WN / 4; q++) store4<T>(p + 4 * q, v + 4 * q);
    } else {
#pragma unroll
        for (int j = 0; j < WN; j++) p[j] = from_f<T>(v[j]);
    }
}

// The items of one channel plane: input footprint R rows x WN pixels, output footprint OR rows x OW pixels.
template <int RS, bool VEC>
struct Geo {
    static constexpr int R = RS == LGM_GN_RESAMPLE_DOWN2 ? 2 : 1;
    static constexpr int WN = (RS == LGM_GN_RESAMPLE_DOWN2 ? 2 : 1) * (VEC ? 4 : 1);
    static constexpr int OR = RS == LGM_GN_RESAMPLE_UP2 ? 2 : 1;
    static constexpr int OW = RS == LGM_GN_RESAMPLE_UP2 ? 2 * WN : RS == LGM_GN_RESAMPLE_DOWN2 ? WN / 2 : WN;
    __host__ __device__ static long long items(int H, int W) {
        if (RS == LGM_GN_RESAMPLE_NONE) return (long long)H * W / WN;  // (the plane flattened)
        if (RS == LGM_GN_RESAMPLE_UP2) return (long long)H * (W / WN);
        return (long long)(H / 2) * (W / WN);
    }
    // element offsets, within the input and the output plane, of item `it`; ostride: the output's row stride
    __device__ static void locate(long long it, int W, size_t &in0, size_t &out0, size_t &ostride) {
        if (RS == LGM_GN_RESAMPLE_NONE) {
            in0 = out0 = (size_t)it * WN;
            ostride = 0;
        } else {
            const long long wq = W / WN, h = it / wq, j = it - h * wq;
            if (RS == LGM_GN_RESAMPLE_UP2) {
                in0 = (size_t)h * W + (size_t)j * WN;
                ostride = 2 * (size_t)W;
                out0 = 2 * (size_t)h * ostride + 2 * (size_t)j * WN;
            } else {
                in0 = 2 * (size_t)h * W + (size_t)j * WN;
                ostride = (size_t)(W / 2);
                out0 = (size_t)h * ostride + (size_t)j * (WN / 2);
            }
        }
    }
};

__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

template <class TI, int RS, bool VEC>
__device__ __forceinline__ void load_x(const TI *xp, size_t in0, int W, float (&v)[Geo<RS, VEC>::R][Geo<RS, VEC>::WN]) {
#pragma unroll
    for (int r = 0; r < Geo<RS, VEC>::R; r++) ld_row<TI, Geo<RS, VEC>::WN>(xp + in0 + (size_t)r * W, v[r]);
}

// y = resample(silu((x - mean) a + b)) of one item, rounded once
template <class TO, int RS, bool VEC>
__device__ __forceinline__ void fwd_store(TO *yp, size_t out0, size_t ostride, float mean, float a, float b,
                                          const float (&v)[Geo<RS, VEC>::R][Geo<RS, VEC>::WN]) {
    using GE = Geo<RS, VEC>;
    float act[GE::R][GE::WN];
#pragma unroll
    for (int r = 0; r < GE::R; r++)
#pragma unroll
        for (int j = 0; j < GE::WN; j++) {
            const float z = fmaf(v[r][j] - mean, a, b);
            act[r][j] = z * sigmoidf(z);
        }
    float o[GE::OW];
    if constexpr (RS == LGM_GN_RESAMPLE_NONE) {
        st_row<TO, GE::OW>(yp + out0, act[0]);
    } else if constexpr (RS == LGM_GN_RESAMPLE_UP2) {
#pragma unroll
        for (int j = 0; j < GE::WN; j++) o[2 * j] = o[2 * j + 1] = act[0][j];
        st_row<TO, GE::OW>(yp + out0, o);
        st_row<TO, GE::OW>(yp + out0 + ostride, o);
    } else {
#pragma unroll
        for (int j = 0; j < GE::OW; j++)
            o[j] = ((act[0][2 * j] + act[0][2 * j + 1]) + (act[1][2 * j] + act[1][2 * j + 1])) * 0.25f;
        st_row<TO, GE::OW>(yp + out0, o);
    }
}

// da = resample^T(d_y) over an item's input footprint
template <class TO, int RS, bool VEC>
__device__ __forceinline__ void load_da(const TO *dyp, size_t out0, size_t ostride,
                                        float (&da)[Geo<RS, VEC>::R][Geo<RS, VEC>::WN]) {
    using GE = Geo<RS, VEC>;
    if constexpr (RS == LGM_GN_RESAMPLE_NONE) {
        ld_row<TO, GE::OW>(dyp + out0, da[0]);
    } else if constexpr (RS == LGM_GN_RESAMPLE_UP2) {
        float d0[GE::OW], d1[GE::OW];
        ld_row<TO, GE::OW>(dyp + out0, d0);
        ld_row<TO, GE::OW>(dyp + out0 + ostride, d1);
#pragma unroll
        for (int j = 0; j < GE::WN; j++) da[0][j] = (d0[2 * j] + d0[2 * j + 1]) + (d1[2 * j] + d1[2 * j + 1]);
    } else {
        float d[GE::OW];
        ld_row<TO, GE::OW>(dyp + out0, d);
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < GE::WN; j++) da[r][j] = d[j / 2] * 0.25f;
    }
}

// dz = da s (1 + z (1 - s)), z = (x - mean) a + b
__device__ __forceinline__ float silu_bwd(float xc, float a, float b, float da) {
    const float z = fmaf(xc, a, b), s = sigmoidf(z);
    return da * (s * fmaf(z, 1.f - s, 1.f));
}

// ---- forward
template <class TI, class TO, int RS, bool VEC>
__global__ __launch_bounds__(GNS_THREADS) void k_gns_slab(int C, int H, int W, int G, float eps,
                                                          const TI *__restrict__ x, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, TO *__restrict__ y,
                                                          float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    using GE = Geo<RS, VEC>;
    __shared__ __attribute__((aligned(16))) float slab[GNS_SLAB_MAX];  // [Cg][HW]
    __shared__ float red[4];
    const int tid = threadIdx.x, Cg = C / G, HW = H * W, n = Cg * HW;  // n <= GNS_SLAB_MAX
    const size_t ng = blockIdx.x, smp = ng / G;
    const int g = (int)(ng - smp * G);
    const TI *xg = x + ng * (size_t)n;  // (sample, group) slabs are contiguous
    float s = 0.f;
    if constexpr (VEC) {  // n % 4 == 0, 16-byte aligned
        for (int i = tid; i < n / 4; i += GNS_THREADS) {
            float v[4];
            load4<TI>(xg + 4 * i, v);
            *reinterpret_cast<float4 *>(slab + 4 * i) = make_float4(v[0], v[1], v[2], v[3]);
            s += (v[0] + v[1]) + (v[2] + v[3]);
        }
    } else {
        for (int i = tid; i < n; i += GNS_THREADS) {
            const float v = to_f(xg[i]);
            slab[i] = v;
            s += v;
        }
    }
    const float m0 = block_sum256(s, red) / (float)n;  // (its barriers also publish the slab)
    float sd = 0.f, q = 0.f;
    for (int i = tid; i < n; i += GNS_THREADS) {
        const float d = slab[i] - m0;
        sd += d;
        q = fmaf(d, d, q);
    }
    // the centred sums about m0 give the correction of m0 and the sum of squares about the corrected mean
    const float dm = block_sum256(sd, red) / (float)n;
    const float M2 = block_sum256(q, red) - dm * dm * (float)n;
    const float mean = m0 + dm;
    const float rstd = 1.f / sqrtf(fmaxf(M2 / (float)n, 0.f) + eps);  // biased variance, as torch
    if (tid == 0) {
        mean_out[ng] = mean;
        rstd_out[ng] = rstd;
    }
    const long long ipp = GE::items(H, W);
    const size_t OHW = RS == LGM_GN_RESAMPLE_UP2 ? 4 * (size_t)HW : RS == LGM_GN_RESAMPLE_DOWN2 ? (size_t)HW / 4 : (size_t)HW;
    const int total = (int)(ipp * Cg);  // <= n
    for (int it = tid; it < total; it += GNS_THREADS) {
        const int cl = it / (int)ipp, pit = it - cl * (int)ipp, c = g * Cg + cl;
        const float a = rstd * (gamma ? gamma[c] : 1.f), b = beta ? beta[c] : 0.f;
        size_t in0, out0, ostride;
        GE::locate(pit, W, in0, out0, ostride);
        float v[GE::R][GE::WN];
        load_x<float, RS, VEC>(slab + (size_t)cl * HW, in0, W, v);
        fwd_store<TO, RS, VEC>(y + (smp * C + c) * OHW, out0, ostride, mean, a, b, v);
    }
}

template <class TI, bool VEC>
__global__ __launch_bounds__(GNS_THREADS) void k_gns_stats(size_t n, int S, const TI *__restrict__ x,
                                                           float2 *__restrict__ part) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const size_t ng = blockIdx.x / (unsigned)S;
    const int s = (int)(blockIdx.x - ng * S);
    const size_t i0 = (size_t)s * GNS_CHUNK;
    const int m = (int)((n - i0 < (size_t)GNS_CHUNK) ? n - i0 : (size_t)GNS_CHUNK);  // elements of this chunk
    const TI *xc = x + ng * n + i0;
    float v[GNS_CHUNK / GNS_THREADS];
    // unconditional loads on clamped in-range addresses: all in flight at once
    if constexpr (VEC) {  // n % 4 == 0: m % 4 == 0
#pragma unroll
        for (int k = 0; k < GNS_CHUNK / GNS_THREADS / 4; k++) {
            const int i = 4 * (k * GNS_THREADS + tid);
            load4<TI>(xc + (i < m ? i : 0), v + 4 * k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < GNS_CHUNK / GNS_THREADS; k++) {
            const int i = k * GNS_THREADS + tid;
            v[k] = to_f(xc[i < m ? i : 0]);
        }
    }
    bool ok[GNS_CHUNK / GNS_THREADS];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < GNS_CHUNK / GNS_THREADS; k++) {
        ok[k] = (VEC ? 4 * ((k / 4) * GNS_THREADS + tid) : k * GNS_THREADS + tid) < m;
        sum += ok[k] ? v[k] : 0.f;
    }
    const float m0 = block_sum256(sum, red) / (float)m;
    float sd = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < GNS_CHUNK / GNS_THREADS; k++) {
        const float d = ok[k] ? v[k] - m0 : 0.f;
        sd += d;
        q = fmaf(d, d, q);
    }
    const float dm = block_sum256(sd, red) / (float)m;  // (as k_gns_slab)
    const float M2 = block_sum256(q, red) - dm * dm * (float)m;
    if (tid == 0) part[blockIdx.x] = make_float2(m0 + dm, fmaxf(M2, 0.f));
}

// mean / rstd of a group from its S chunk statistics: Chan's merge in chunk order, in fp64 (S scalar steps)
__device__ __forceinline__ void merge_stats(const float2 *__restrict__ pg, int S, size_t n, float eps, float &mean,
                                            float &rstd) {
    double mu = 0.0, M2 = 0.0, cnt = 0.0;
    for (int s = 0; s < S; s++) {
        const float2 p = pg[s];
        const size_t i0 = (size_t)s * GNS_CHUNK;
        const double m = (double)((n - i0 < (size_t)GNS_CHUNK) ? n - i0 : (size_t)GNS_CHUNK);
        const double tot = cnt + m, d = (double)p.x - mu;
        mu += d * (m / tot);
        M2 += (double)p.y + d * d * (cnt * m / tot);
        cnt = tot;
    }
    mean = (float)mu;
    rstd = 1.f / sqrtf((float)(M2 / (double)n) + eps);  // biased variance, as torch
}

template <class TI, class TO, int RS, bool VEC, int LP>
__global__ __launch_bounds__(GNS_THREADS) void k_gns_norm(int C, int H, int W, int G, int S, int nT, size_t units,
                                                          float eps,
                                                          const TI *__restrict__ x, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta,
                                                          const float2 *__restrict__ part, TO *__restrict__ y,
                                                          float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    using GE = Geo<RS, VEC>;
    const int tid = threadIdx.x, Cg = C / G, l = tid % LP;
    const size_t un = (size_t)blockIdx.x * (GNS_THREADS / LP) + tid / LP;  // this team's (plane, tile)
    if (un >= units) return;
    const size_t nc = un / (unsigned)nT, smp = nc / C, HW = (size_t)H * W;
    const int t = (int)(un - nc * nT), c = (int)(nc - smp * C), g = c / Cg;
    float mean, rstd;
    merge_stats(part + (smp * G + g) * S, S, (size_t)Cg * HW, eps, mean, rstd);
    if (t == 0 && c == g * Cg && l == 0) {  // one writer per (sample, group)
        mean_out[smp * G + g] = mean;
        rstd_out[smp * G + g] = rstd;
    }
    const float a = rstd * (gamma ? gamma[c] : 1.f), b = beta ? beta[c] : 0.f;
    const long long ipp = GE::items(H, W);
    const size_t OHW = RS == LGM_GN_RESAMPLE_UP2 ? 4 * HW : RS == LGM_GN_RESAMPLE_DOWN2 ? HW / 4 : HW;
    const TI *xp = x + nc * HW;
    TO *yp = y + nc * OHW;
    float v[GNS_UNROLL][GE::R][GE::WN];
    size_t out0[GNS_UNROLL], ostride = 0;
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {  // loads of all items first (clamped, unconditional)
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        size_t in0;
        GE::locate(it < ipp ? it : ipp - 1, W, in0, out0[u], ostride);
        load_x<TI, RS, VEC>(xp, in0, W, v[u]);
    }
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        if (it < ipp) fwd_store<TO, RS, VEC>(yp, out0[u], ostride, mean, a, b, v[u]);
    }
}

// ---- backward
template <class TI, class TO, int RS, bool VEC, int LP>
__global__ __launch_bounds__(GNS_THREADS) void k_gns_bwd_part(int C, int H, int W, int G, int nT, size_t units,
                                                              const TI *__restrict__ x,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta,
                                                              const float *__restrict__ mean_in,
                                                              const float *__restrict__ rstd_in,
                                                              const TO *__restrict__ dy, float2 *__restrict__ part) {
    using GE = Geo<RS, VEC>;
    __shared__ float red[4];
    const int tid = threadIdx.x, Cg = C / G, l = tid % LP;
    const size_t un = (size_t)blockIdx.x * (GNS_THREADS / LP) + tid / LP;  // this team's (plane, tile)
    if (un >= units) return;  // (teams of LP < 256 lanes only: whole teams leave, and no barrier follows)
    const size_t nc = un / (unsigned)nT, smp = nc / C, HW = (size_t)H * W;
    const int t = (int)(un - nc * nT), c = (int)(nc - smp * C), g = c / Cg;
    const float mean = mean_in[smp * G + g], rstd = rstd_in[smp * G + g];
    const float a = rstd * (gamma ? gamma[c] : 1.f), b = beta ? beta[c] : 0.f;
    const long long ipp = GE::items(H, W);
    const size_t OHW = RS == LGM_GN_RESAMPLE_UP2 ? 4 * HW : RS == LGM_GN_RESAMPLE_DOWN2 ? HW / 4 : HW;
    const TI *xp = x + nc * HW;
    const TO *dp = dy + nc * OHW;
    float v[GNS_UNROLL][GE::R][GE::WN], da[GNS_UNROLL][GE::R][GE::WN];
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        size_t in0, out0, ostride;
        GE::locate(it < ipp ? it : ipp - 1, W, in0, out0, ostride);
        load_x<TI, RS, VEC>(xp, in0, W, v[u]);
        load_da<TO, RS, VEC>(dp, out0, ostride, da[u]);
    }
    float sdx = 0.f, sd = 0.f;
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        if (it < ipp) {
#pragma unroll
            for (int r = 0; r < GE::R; r++)
#pragma unroll
                for (int j = 0; j < GE::WN; j++) {
                    const float xc = v[u][r][j] - mean, dz = silu_bwd(xc, a, b, da[u][r][j]);
                    sdx = fmaf(dz, xc, sdx);
                    sd += dz;
                }
        }
    }
    sdx = team_sum<LP>(sdx, red);
    sd = team_sum<LP>(sd, red);
    if (l == 0) part[un] = make_float2(sdx, sd);
}

// part [N*C][nT] -> sdb [N*C] = (sum dz (x - mean), sum dz) per (sample, channel), in tile order; then with
// s = 1 / (Cg HW): coef [N*G] = (c2, c3) = (-rstd^3 s sum_c gamma ds, -rstd s sum_c gamma db), and
// dgamma_c = sum_n ds rstd, dbeta_c = sum_n db, over the samples in order.
__global__ __launch_bounds__(GNS_THREADS) void k_gns_bwd_coef(int N, int C, float inv_count, int G, int nT,
                                                              const float2 *__restrict__ part, float2 *sdb,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ rstd, float2 *__restrict__ coef,
                                                              float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int g = blockIdx.x, Cg = C / G, tid = threadIdx.x;
    for (long long it = tid; it < (long long)N * Cg; it += GNS_THREADS) {
        const long long n = it / Cg;
        const int c = g * Cg + (int)(it - n * Cg);
        const float2 *pp = part + ((size_t)n * C + c) * nT;
        float a = 0.f, b = 0.f;
        for (int t = 0; t < nT; t++) {  // fixed order over the tiles
            const float2 p = pp[t];
            a += p.x;
            b += p.y;
        }
        sdb[(size_t)n * C + c] = make_float2(a, b);
    }
    __syncthreads();  // this workgroup wrote, and now reads, its own group's entries of sdb
    for (int n = tid; n < N; n += GNS_THREADS) {
        float sum1 = 0.f, sum2 = 0.f;
        for (int cc = 0; cc < Cg; cc++) {
            const float ga = gamma ? gamma[g * Cg + cc] : 1.f;
            const float2 v = sdb[(size_t)n * C + g * Cg + cc];
            sum1 = fmaf(v.x, ga, sum1);
            sum2 = fmaf(v.y, ga, sum2);
        }
        const float rs = rstd[(size_t)n * G + g];
        coef[(size_t)n * G + g] = make_float2(-sum1 * rs * rs * rs * inv_count, -sum2 * rs * inv_count);
    }
    if (dgamma || dbeta) {
        for (int cc = tid; cc < Cg; cc += GNS_THREADS) {
            float dg = 0.f, db = 0.f;
            for (int n = 0; n < N; n++) {
                const float2 v = sdb[(size_t)n * C + g * Cg + cc];
                dg = fmaf(v.x, rstd[(size_t)n * G + g], dg);
                db += v.y;
            }
            if (dgamma) dgamma[g * Cg + cc] = dg;
            if (dbeta) dbeta[g * Cg + cc] = db;
        }
    }
}

template <class TI, class TO, int RS, bool VEC, int LP>
__global__ __launch_bounds__(GNS_THREADS) void k_gns_bwd_dx(int C, int H, int W, int G, int nT, size_t units,
                                                            const TI *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta,
                                                            const float *__restrict__ mean_in,
                                                            const float *__restrict__ rstd_in,
                                                            const float2 *__restrict__ coef, const TO *__restrict__ dy,
                                                            TI *__restrict__ dx) {
    using GE = Geo<RS, VEC>;
    const int tid = threadIdx.x, Cg = C / G, l = tid % LP;
    const size_t un = (size_t)blockIdx.x * (GNS_THREADS / LP) + tid / LP;  // this team's (plane, tile)
    if (un >= units) return;
    const size_t nc = un / (unsigned)nT, smp = nc / C, HW = (size_t)H * W;
    const int t = (int)(un - nc * nT), c = (int)(nc - smp * C), g = c / Cg;
    const float mean = mean_in[smp * G + g], rstd = rstd_in[smp * G + g];
    const float2 k = coef[smp * G + g];
    const float a = rstd * (gamma ? gamma[c] : 1.f), b = beta ? beta[c] : 0.f;
    const long long ipp = GE::items(H, W);
    const size_t OHW = RS == LGM_GN_RESAMPLE_UP2 ? 4 * HW : RS == LGM_GN_RESAMPLE_DOWN2 ? HW / 4 : HW;
    const TI *xp = x + nc * HW;
    const TO *dp = dy + nc * OHW;
    TI *dxp = dx + nc * HW;
    float v[GNS_UNROLL][GE::R][GE::WN], da[GNS_UNROLL][GE::R][GE::WN];
    size_t in0[GNS_UNROLL];
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        size_t out0, ostride;
        GE::locate(it < ipp ? it : ipp - 1, W, in0[u], out0, ostride);
        load_x<TI, RS, VEC>(xp, in0[u], W, v[u]);
        load_da<TO, RS, VEC>(dp, out0, ostride, da[u]);
    }
#pragma unroll
    for (int u = 0; u < GNS_UNROLL; u++) {
        const long long it = (long long)t * (GNS_UNROLL * LP) + u * LP + l;
        if (it < ipp) {
#pragma unroll
            for (int r = 0; r < GE::R; r++) {
                float o[GE::WN];
#pragma unroll
                for (int j = 0; j < GE::WN; j++) {
                    const float xc = v[u][r][j] - mean, dz = silu_bwd(xc, a, b, da[u][r][j]);
                    o[j] = fmaf(a, dz, fmaf(k.x, xc, k.y));
                }
                st_row<TI, GE::WN>(dxp + in0[u] + (size_t)r * W, o);
            }
        }
    }
}

// ---- host side
constexpr long long GRID_MAX = 2147483647LL;

bool use_slab(long long N, int G, long long n) {
    return n <= GNS_SLAB_MAX && (n <= GNS_CHUNK || N * G >= GNS_FILL);
}

bool vec_ok(int rs, int H, int W, const void *a, const void *b, const void *c) {
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
        return false;
    if (rs == LGM_GN_RESAMPLE_NONE) return ((long long)H * W) % 4 == 0;
    return W % (rs == LGM_GN_RESAMPLE_UP2 ? 4 : 8) == 0;
}

long long items_of(int rs, bool vec, int H, int W) {
    if (rs == LGM_GN_RESAMPLE_NONE) return vec ? Geo<0, true>::items(H, W) : Geo<0, false>::items(H, W);
    if (rs == LGM_GN_RESAMPLE_UP2) return vec ? Geo<1, true>::items(H, W) : Geo<1, false>::items(H, W);
    return vec ? Geo<2, true>::items(H, W) : Geo<2, false>::items(H, W);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Lanes per (plane, tile) team of the elementwise passes, GNS_UNROLL items per lane: small planes (LGM's 8 x 8 and
// 16 x 16 levels have 16 and 64 vector items) share a workgroup, 16 or 4 planes each, instead of idling most of one.
constexpr int GNS_TEAM_S = 16, GNS_TEAM_M = 64;
int team_of(long long ipp) {
    return ipp <= GNS_UNROLL * GNS_TEAM_S ? GNS_TEAM_S : ipp <= GNS_UNROLL * GNS_TEAM_M ? GNS_TEAM_M : GNS_THREADS;
}
// kernel names by form: [vector][team]
const char *form_name(const char *const (&names)[2][3], bool vec, int lp) {
    return names[vec ? 1 : 0][lp == GNS_TEAM_S ? 0 : lp == GNS_TEAM_M ? 1 : 2];
}
constexpr const char *NORM_NAMES[2][3] = {{"k_gns_norm_s16", "k_gns_norm_s64", "k_gns_norm_s"},
                                          {"k_gns_norm_v16", "k_gns_norm_v64", "k_gns_norm_v"}};
constexpr const char *PART_NAMES[2][3] = {{"k_gns_bwd_part_s16", "k_gns_bwd_part_s64", "k_gns_bwd_part_s"},
                                          {"k_gns_bwd_part_v16", "k_gns_bwd_part_v64", "k_gns_bwd_part_v"}};
constexpr const char *DX_NAMES[2][3] = {{"k_gns_bwd_dx_s16", "k_gns_bwd_dx_s64", "k_gns_bwd_dx_s"},
                                        {"k_gns_bwd_dx_v16", "k_gns_bwd_dx_v64", "k_gns_bwd_dx_v"}};

// the supported (x, y) dtype pairs: y's == x's, or fp32 x with any y
bool pair_ok(int dtx, int dty) {
    const bool vy = dty == LGM_ATTN_F32 || dty == LGM_ATTN_BF16 || dty == LGM_ATTN_F16;
    return vy && (dtx == LGM_ATTN_F32 || (dtx == dty));
}
template <class Fn>
int with_pair(const char *who, int dtx, int dty, Fn &&fn) {
    if (!pair_ok(dtx, dty)) {
        set_error("%s: unsupported dtype pair x=%d y=%d (y's dtype must equal x's, or x be f32)", who, dtx, dty);
        return LGM_E_INVALID;
    }
    return with_type(who, dty, [&](auto ty) { return dtx == LGM_ATTN_F32 ? fn(float{}, ty) : fn(ty, ty); });
}

template <class Fn>
int with_geo(int rs, bool vec, Fn &&fn) {
    switch (rs * 2 + (vec ? 1 : 0)) {
        case 0: return fn(std::integral_constant<int, 0>{}, std::false_type{});
        case 1: return fn(std::integral_constant<int, 0>{}, std::true_type{});
        case 2: return fn(std::integral_constant<int, 1>{}, std::false_type{});
        case 3: return fn(std::integral_constant<int, 1>{}, std::true_type{});
        case 4: return fn(std::integral_constant<int, 2>{}, std::false_type{});
        default: return fn(std::integral_constant<int, 2>{}, std::true_type{});
    }
}

template <class Fn>
int with_team(int lp, Fn &&fn) {
    if (lp == GNS_TEAM_S) return fn(std::integral_constant<int, GNS_TEAM_S>{});
    if (lp == GNS_TEAM_M) return fn(std::integral_constant<int, GNS_TEAM_M>{});
    return fn(std::integral_constant<int, GNS_THREADS>{});
}

// shape checks shared by the two entry points; returns LGM_OK, and *empty = true where there is nothing to do
int check_shape(const char *who, int dtx, int dty, int N, int C, int H, int W, int G, int rs, bool *empty) {
    *empty = false;
    if (N < 0 || C <= 0 || H < 0 || W < 0 || G <= 0) {
        set_error("%s: bad shape N=%d C=%d H=%d W=%d groups=%d", who, N, C, H, W, G);
        return LGM_E_INVALID;
    }
    if (C % G) {
        set_error("%s: C=%d is not a multiple of groups=%d", who, C, G);
        return LGM_E_INVALID;
    }
    if (rs != LGM_GN_RESAMPLE_NONE && rs != LGM_GN_RESAMPLE_UP2 && rs != LGM_GN_RESAMPLE_DOWN2) {
        set_error("%s: bad resample %d", who, rs);
        return LGM_E_INVALID;
    }
    if (!pair_ok(dtx, dty)) {
        set_error("%s: unsupported dtype pair x=%d y=%d (y's dtype must equal x's, or x be f32)", who, dtx, dty);
        return LGM_E_INVALID;
    }
    if (rs == LGM_GN_RESAMPLE_DOWN2 && ((H | W) & 1)) {
        set_error("%s: DOWN2 needs even H and W, got %d x %d", who, H, W);
        return LGM_E_INVALID;
    }
    // 64-bit element offsets: the larger of the two tensors (UP2's output, 4x the input) stays below 2^60 elements, so
    // no product of the sizes formed later can wrap
    if ((double)N * (double)C * (double)H * (double)W * 4.0 >= 1152921504606846976.0) {
        set_error("%s: N=%d C=%d H=%d W=%d is beyond 2^60 elements", who, N, C, H, W);
        return LGM_E_INVALID;
    }
    if (N == 0 || H == 0 || W == 0) *empty = true;
    return LGM_OK;
}

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_gn_silu_workspace_size(int N, int C, int H, int W, int groups) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || groups <= 0 || C % groups) return 0;
    const long long n = (long long)(C / groups) * H * W;
    if (lgm::use_slab(N, groups, n)) return 0;
    const size_t S = (size_t)((n + lgm::GNS_CHUNK - 1) / lgm::GNS_CHUNK);
    return (size_t)N * groups * S * sizeof(float2);
}

extern "C" int lgm_gn_silu_forward(int dtype_x, int dtype_y, int N, int C, int H, int W, int groups, float eps,
                                   int resample, const void *x, const float *gamma, const float *beta, void *y,
                                   float *mean, float *rstd, void *workspace, size_t workspace_bytes, void *stream,
                                   const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    bool empty;
    const int rc = check_shape("lgm_gn_silu_forward", dtype_x, dtype_y, N, C, H, W, groups, resample, &empty);
    if (rc != LGM_OK || empty) return rc;
    const int G = groups, Cg = C / G;
    const long long HW = (long long)H * W, n = Cg * HW;
    const bool slab = use_slab(N, G, n);
    const bool vec = vec_ok(resample, H, W, x, y, nullptr);
    const long long S = (n + GNS_CHUNK - 1) / GNS_CHUNK;
    const long long ipp = items_of(resample, vec, H, W);
    const int lp = team_of(ipp);
    const long long nT = (ipp + GNS_UNROLL * lp - 1) / (GNS_UNROLL * lp), units = (long long)N * C * nT;
    const long long blocks = (units + GNS_THREADS / lp - 1) / (GNS_THREADS / lp);
    if ((long long)N * G > GRID_MAX || (!slab && ((long long)N * G * S > GRID_MAX || blocks > GRID_MAX))) {
        set_error("lgm_gn_silu_forward: N=%d C=%d H=%d W=%d groups=%d needs a launch grid beyond %lld workgroups", N,
                  C, H, W, G, GRID_MAX);
        return LGM_E_INVALID;
    }
    if (!x || !y || !mean || !rstd) {
        set_error("lgm_gn_silu_forward: null pointer");
        return LGM_E_INVALID;
    }
    const size_t need = lgm_gn_silu_workspace_size(N, C, H, W, G);
    if (need && (!workspace || workspace_bytes < need)) {
        set_error("lgm_gn_silu_forward: workspace too small (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0,
                  need);
        return LGM_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    return with_pair("lgm_gn_silu_forward", dtype_x, dtype_y, [&](auto tx, auto ty) {
        using TI = decltype(tx);
        using TO = decltype(ty);
        if (!slab) {
            float2 *part = (float2 *)workspace;
            if (vec)
                LGM_LAUNCH("k_gns_stats_v", st, (k_gns_stats<TI, true><<<(unsigned)(N * G * S), GNS_THREADS, 0, st>>>(
                                                    (size_t)n, (int)S, (const TI *)x, part)));
            else
                LGM_LAUNCH("k_gns_stats_s", st, (k_gns_stats<TI, false><<<(unsigned)(N * G * S), GNS_THREADS, 0, st>>>(
                                                    (size_t)n, (int)S, (const TI *)x, part)));
        }
        return with_geo(resample, vec, [&](auto rs_, auto vec_) {
            constexpr int RS = decltype(rs_)::value;
            constexpr bool VEC = decltype(vec_)::value;
            if (slab) {
                LGM_LAUNCH(VEC ? "k_gns_slab_v" : "k_gns_slab_s", st,
                           (k_gns_slab<TI, TO, RS, VEC><<<(unsigned)(N * G), GNS_THREADS, 0, st>>>(
                               C, H, W, G, eps, (const TI *)x, gamma, beta, (TO *)y, mean, rstd)));
                return LGM_OK;
            }
            return with_team(lp, [&](auto lp_) {
                constexpr int LP = decltype(lp_)::value;
                LGM_LAUNCH(form_name(NORM_NAMES, VEC, LP), st,
                           (k_gns_norm<TI, TO, RS, VEC, LP><<<(unsigned)blocks, GNS_THREADS, 0, st>>>(
                               C, H, W, G, (int)S, (int)nT, (size_t)units, eps, (const TI *)x, gamma, beta,
                               (const float2 *)workspace, (TO *)y, mean, rstd)));
                return LGM_OK;
            });
        });
    });
}

extern "C" size_t lgm_gn_silu_backward_workspace_size(int N, int C, int H, int W, int groups) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || groups <= 0 || C % groups) return 0;
    // the partial sums are sized for the most tiles any form takes (one item per input pixel)
    const size_t nT = (size_t)(((long long)H * W + lgm::GNS_TILE - 1) / lgm::GNS_TILE);
    return lgm::align256((size_t)N * C * nT * sizeof(float2)) + lgm::align256((size_t)N * C * sizeof(float2)) +
           (size_t)N * groups * sizeof(float2);
}

extern "C" int lgm_gn_silu_backward(int dtype_x, int dtype_y, int N, int C, int H, int W, int groups, int resample,
                                    const void *x, const float *gamma, const float *beta, const float *mean,
                                    const float *rstd, const void *d_y, void *dx, float *dgamma, float *dbeta,
                                    void *workspace, size_t workspace_bytes, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    bool empty;
    const int rc = check_shape("lgm_gn_silu_backward", dtype_x, dtype_y, N, C, H, W, groups, resample, &empty);
    if (rc != LGM_OK) return rc;
    const int G = groups, Cg = C / G;
    const long long HW = (long long)H * W;
    if (!dx && !dgamma && !dbeta) return LGM_OK;
    const bool vec = vec_ok(resample, H, W, x, d_y, dx);
    const long long ipp = empty ? 0 : items_of(resample, vec, H, W);
    const int lp = team_of(ipp);
    const long long nT = (ipp + GNS_UNROLL * lp - 1) / (GNS_UNROLL * lp), units = (long long)N * C * nT;
    const long long blocks = (units + GNS_THREADS / lp - 1) / (GNS_THREADS / lp);
    const long long nTmax = (HW + GNS_TILE - 1) / GNS_TILE;  // (nT <= nTmax: teams below 256 lanes have nT = 1)
    if ((long long)N * C > GRID_MAX || (long long)N * C * nTmax > GRID_MAX) {
        set_error("lgm_gn_silu_backward: N=%d C=%d H=%d W=%d needs a launch grid beyond %lld workgroups", N, C, H, W,
                  GRID_MAX);
        return LGM_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (empty) {  // no elements: the parameter gradients are zero
        if (dgamma && hipMemsetAsync(dgamma, 0, (size_t)C * sizeof(float), st) != hipSuccess) return LGM_E_HIP;
        if (dbeta && hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), st) != hipSuccess) return LGM_E_HIP;
        return LGM_OK;
    }
    if (!x || !mean || !rstd || !d_y) {
        set_error("lgm_gn_silu_backward: null pointer");
        return LGM_E_INVALID;
    }
    const size_t need = lgm_gn_silu_backward_workspace_size(N, C, H, W, G);
    if (!workspace || workspace_bytes < need) {
        set_error("lgm_gn_silu_backward: workspace too small (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0,
                  need);
        return LGM_E_WORKSPACE;
    }
    float2 *part = (float2 *)workspace;
    float2 *sdb = (float2 *)((char *)workspace + align256((size_t)N * C * nTmax * sizeof(float2)));
    float2 *coef = (float2 *)((char *)sdb + align256((size_t)N * C * sizeof(float2)));
    const float inv_count = 1.f / ((float)Cg * (float)HW);
    const unsigned grid = (unsigned)blocks;
    return with_pair("lgm_gn_silu_backward", dtype_x, dtype_y, [&](auto tx, auto ty) {
        using TI = decltype(tx);
        using TO = decltype(ty);
        return with_geo(resample, vec, [&](auto rs_, auto vec_) {
            constexpr int RS = decltype(rs_)::value;
            constexpr bool VEC = decltype(vec_)::value;
            return with_team(lp, [&](auto lp_) {
                constexpr int LP = decltype(lp_)::value;
                LGM_LAUNCH(form_name(PART_NAMES, VEC, LP), st,
                           (k_gns_bwd_part<TI, TO, RS, VEC, LP><<<grid, GNS_THREADS, 0, st>>>(
                               C, H, W, G, (int)nT, (size_t)units, (const TI *)x, gamma, beta, mean, rstd,
                               (const TO *)d_y, part)));
                LGM_LAUNCH("k_gns_bwd_coef", st, (k_gns_bwd_coef<<<G, GNS_THREADS, 0, st>>>(
                                                     N, C, inv_count, G, (int)nT, part, sdb, gamma, rstd, coef, dgamma,
                                                     dbeta)));
                if (dx)
                    LGM_LAUNCH(form_name(DX_NAMES, VEC, LP), st,
                               (k_gns_bwd_dx<TI, TO, RS, VEC, LP><<<grid, GNS_THREADS, 0, st>>>(
                                   C, H, W, G, (int)nT, (size_t)units, (const TI *)x, gamma, beta, mean, rstd, coef,
                                   (const TO *)d_y, (TI *)dx)));
                return LGM_OK;
            });
        });
    });
}
