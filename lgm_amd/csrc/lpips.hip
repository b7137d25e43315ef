// lgm_amd/csrc/lpips.hip -- the elementwise side of the LPIPS (VGG16) loss (include/lgm_lpips.h): the per-tap
// distance, forward and backward, and the input pass (composite, bilinear resize, LPIPS's affine map) of
// core/models.py:156-165. The trunk's convolutions stay torch's.
//
// Distance: features are NCHW, so a pixel's channels are HW elements apart: lanes run along pixels and loop over
// channels. A workgroup of 256 threads is a tile of LP pixel items x CS = 256 / LP channel slices: slice s takes the
// channels s, s + CS, ...; the per-slice sums meet in LDS and are added in slice order by every thread of the pixel.
//   k_lpips_dist      sweep 1: sum_c f0^2, sum_c f1^2 (fp64) -> the two norms (stored for the backward); sweep 2 (the tile
//                     again, from cache): sum_c w_c (f0 / A0 - f1 / A1)^2; the workgroup's sum -> part[workgroup];
//   k_lpips_dist_sum  grid (N): out[n] = (sum of the sample's partials, in a fixed order) / HW;
//   k_lpips_dist_bwd  sweep 1: t0, t1 = sum_c w_c d_c f0^_c, sum_c w_c d_c f1^_c; sweep 2: df0, df1, one rounding.
// An item is 4 consecutive pixels (16-byte aligned tensors, HW % 4 == 0: the _v kernels) or one pixel (_s). LP is
// chosen by the plane's item count and C (lp_of): small planes and many channels take 16 items x 16 slices, so that
// the 16^2 and 32^2 taps at C = 512 spread over 4 and 16 workgroups per image and the tile that sweep 2 re-reads
// (LP items x C channels x 2 tensors) stays small; few channels take the whole workgroup along pixels.
// Precision, for pairs that are nearly identical (d ~ 1e-3 |f^|, where training ends up): the sums of squares run in
// fp64 and the norm is rounded to fp32 once (an error of the norm is common to all channels of a pixel and does not
// average out over them); the normalised feature f / A (A = |f| + eps) is kept as q + e, q = f r with r = 1 / A formed
// once per pixel and e = (f - q A) r its correction (nrm: no division per element), and d = (q0 - q1) + (e0 - e1),
// each difference formed on its own under `fp contract(off)`, never folded into an fma: the leading parts cancel
// exactly, and
// bitwise identical inputs give d = 0 exactly.
//
// Input pass: k_lpips_prep, one thread per destination pixel (3 channels, pred and gt); k_lpips_prep_bwd, one thread
// per source texel, summing over the destination rows and columns whose two taps include it (a superset of that range
// in closed form -- the source coordinate is monotone in the destination's --, weights from the forward's own
// function, zero outside): a gather in a fixed order.
#include <type_traits>

#include "elemwise.h"
#include "lgm_lpips.h"

namespace lgm {
namespace {

constexpr int LPI_THREADS = 256;
constexpr long long LPI_GRID_MAX = 2147483647LL;
constexpr int LPI_SIZE_MAX = 32768;  // S, R of the input pass (the range estimates of its backward are fp32)

template <class T, bool VEC>
__device__ __forceinline__ void ld_item(const T *p, float *o) {
    if constexpr (VEC) load4<T>(p, o);
    else o[0] = to_f(p[0]);
}
template <class T, bool VEC>
__device__ __forceinline__ void st_item(T *p, const float *v) {
    if constexpr (VEC) store4<T>(p, v);
    else p[0] = from_f<T>(v[0]);
}

// v[q] (q < NQ) summed over the CS channel slices of this thread's pixel item, in slice order; sl: NQ * 256 elements
template <int NQ, int LP, class E>
__device__ __forceinline__ void slice_sum(E (&v)[NQ], E *sl, int l, int cs) {
    constexpr int CS = LPI_THREADS / LP;
    if constexpr (CS > 1) {
        __syncthreads();  // sl is reused between calls
#pragma unroll
        for (int q = 0; q < NQ; q++) sl[(q * CS + cs) * LP + l] = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            E s = 0;
#pragma unroll 4  // (not all CS at once: with every load of every q in flight the fp64 sums take 246 VGPRs)
            for (int k = 0; k < CS; k++) s += sl[(q * CS + k) * LP + l];
            v[q] = s;
        }
    }
}

// f / A from r = 1 / A as an unevaluated sum q + e: q = f r, e = (f - q A) r (see the head of the file)
struct Quot {
    float q, e;
    __device__ __forceinline__ float value() const { return q + e; }
};
__device__ __forceinline__ Quot nrm(float f, float A, float r) {
#pragma clang fp contract(off)  // (the products must stay products: __fmul_rn alone does not keep them from an fma)
    const float q = f * r, t = fmaf(-q, A, f);
    return {q, t * r};
}
// the difference of two normalised features: the leading parts (exact when they are within a factor 2) plus the
// corrections, each difference formed on its own and never contracted
__device__ __forceinline__ float nd(const Quot &a, const Quot &b) {
#pragma clang fp contract(off)
    const float dq = a.q - b.q, de = a.e - b.e;
    return dq + de;
}

// sqrt of a sum of squares held in fp64, rounded to fp32: the fp32 rsqrt of it and one correction step in fp64 (relative
// error about 1e-14 before the rounding); sums outside fp32's comfortable range (and 0) take fp64's sqrt
__device__ __forceinline__ float norm_of(double ss) {
    const float sf = (float)ss;
    if (!(sf >= 1e-30f && sf <= 1e30f)) return (float)sqrt(ss);
    const double y = (double)rsqrtf(sf), s = ss * y;
    return (float)fma(0.5 * y, fma(-s, s, ss), s);
}

template <class T, bool VEC, int LP>
__global__ __launch_bounds__(LPI_THREADS) void k_lpips_dist(int C, size_t HW, long long ipp, int nT, float eps,
                                                            const T *__restrict__ f0, const T *__restrict__ f1,
                                                            const float *__restrict__ w, float *__restrict__ norm0,
                                                            float *__restrict__ norm1, float *__restrict__ part) {
    constexpr int WN = VEC ? 4 : 1, CS = LPI_THREADS / LP;
    __shared__ float red[4];
    __shared__ double sl[CS > 1 ? 2 * WN * LPI_THREADS : 1];
    const int tid = threadIdx.x, l = tid % LP, cs = tid / LP;
    const size_t n = blockIdx.x / (unsigned)nT;
    const long long it = (long long)(blockIdx.x - n * nT) * LP + l;
    const bool live = it < ipp;
    const size_t off = (size_t)(live ? it : ipp - 1) * WN;  // (clamped: loads stay in range, nothing is stored)
    const T *p0 = f0 + n * C * HW + off, *p1 = f1 + n * C * HW + off;
    double ss[2 * WN];  // the sums of squares in fp64: the norm is common to all channels of a pixel, see norm_of
#pragma unroll
    for (int j = 0; j < 2 * WN; j++) ss[j] = 0.0;
#pragma unroll 4
    for (int c = cs; c < C; c += CS) {
        float a[WN], b[WN];
        ld_item<T, VEC>(p0 + (size_t)c * HW, a);
        ld_item<T, VEC>(p1 + (size_t)c * HW, b);
#pragma unroll
        for (int j = 0; j < WN; j++) {
            ss[j] = fma((double)a[j], (double)a[j], ss[j]);
            ss[WN + j] = fma((double)b[j], (double)b[j], ss[WN + j]);
        }
    }
    slice_sum<2 * WN, LP>(ss, sl, l, cs);
    float na[WN], nb[WN], Aa[WN], Ab[WN], ra[WN], rb[WN];
#pragma unroll
    for (int j = 0; j < WN; j++) {
        na[j] = norm_of(ss[j]);
        nb[j] = norm_of(ss[WN + j]);
        Aa[j] = na[j] + eps;
        Ab[j] = nb[j] + eps;
        ra[j] = 1.f / Aa[j];
        rb[j] = 1.f / Ab[j];
    }
    if (norm0 && cs == 0 && live) {
        st_item<float, VEC>(norm0 + n * HW + off, na);
        st_item<float, VEC>(norm1 + n * HW + off, nb);
    }
    float d[WN];
#pragma unroll
    for (int j = 0; j < WN; j++) d[j] = 0.f;
#pragma unroll 4
    for (int c = cs; c < C; c += CS) {
        float a[WN], b[WN];
        ld_item<T, VEC>(p0 + (size_t)c * HW, a);
        ld_item<T, VEC>(p1 + (size_t)c * HW, b);
        const float wc = w[c];
#pragma unroll
        for (int j = 0; j < WN; j++) {
            const float e = nd(nrm(a[j], Aa[j], ra[j]), nrm(b[j], Ab[j], rb[j]));
            d[j] = fmaf(wc * e, e, d[j]);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < WN; j++) s += d[j];
    s = block_sum256(live ? s : 0.f, red);
    if (tid == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(LPI_THREADS) void k_lpips_dist_sum(int nT, float hw, const float *__restrict__ part,
                                                                float *__restrict__ out) {
    __shared__ float red[4];
    const float *p = part + (size_t)blockIdx.x * nT;
    float s = 0.f;
    for (int t = threadIdx.x; t < nT; t += LPI_THREADS) s += p[t];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s / hw;
}

template <class T, bool VEC, int LP>
__global__ __launch_bounds__(LPI_THREADS) void k_lpips_dist_bwd(int C, size_t HW, long long ipp, int nT, float eps,
                                                                const T *__restrict__ f0, const T *__restrict__ f1,
                                                                const float *__restrict__ w,
                                                                const float *__restrict__ norm0,
                                                                const float *__restrict__ norm1,
                                                                const float *__restrict__ g, T *__restrict__ df0,
                                                                T *__restrict__ df1) {
    constexpr int WN = VEC ? 4 : 1, CS = LPI_THREADS / LP;
    __shared__ float sl[CS > 1 ? 2 * WN * LPI_THREADS : 1];
    const int tid = threadIdx.x, l = tid % LP, cs = tid / LP;
    const size_t n = blockIdx.x / (unsigned)nT;
    const long long it = (long long)(blockIdx.x - n * nT) * LP + l;
    const bool live = it < ipp;
    const size_t off = (size_t)(live ? it : ipp - 1) * WN;
    const size_t base = n * C * HW + off;
    const T *p0 = f0 + base, *p1 = f1 + base;
    float na[WN], nb[WN], Aa[WN], Ab[WN], ra[WN], rb[WN], ia[WN], ib[WN];
    ld_item<float, VEC>(norm0 + n * HW + off, na);
    ld_item<float, VEC>(norm1 + n * HW + off, nb);
#pragma unroll
    for (int j = 0; j < WN; j++) {
        Aa[j] = na[j] + eps;
        Ab[j] = nb[j] + eps;
        ra[j] = 1.f / Aa[j];
        rb[j] = 1.f / Ab[j];
        ia[j] = na[j] > 0.f ? 1.f / na[j] : 0.f;  // a zero norm drops the second term
        ib[j] = nb[j] > 0.f ? 1.f / nb[j] : 0.f;
    }
    float tt[2 * WN];
#pragma unroll
    for (int j = 0; j < 2 * WN; j++) tt[j] = 0.f;
#pragma unroll 4
    for (int c = cs; c < C; c += CS) {
        float a[WN], b[WN];
        ld_item<T, VEC>(p0 + (size_t)c * HW, a);
        ld_item<T, VEC>(p1 + (size_t)c * HW, b);
        const float wc = w[c];
#pragma unroll
        for (int j = 0; j < WN; j++) {
            const Quot qa = nrm(a[j], Aa[j], ra[j]), qb = nrm(b[j], Ab[j], rb[j]);
            const float ah = qa.value(), bh = qb.value(), we = wc * nd(qa, qb);
            tt[j] = fmaf(we, ah, tt[j]);
            tt[WN + j] = fmaf(we, bh, tt[WN + j]);
        }
    }
    slice_sum<2 * WN, LP>(tt, sl, l, cs);
    const float k = 2.f * g[n] / (float)HW;
    if (!live) return;  // (no barrier follows)
#pragma unroll 4
    for (int c = cs; c < C; c += CS) {
        float a[WN], b[WN], o0[WN], o1[WN];
        ld_item<T, VEC>(p0 + (size_t)c * HW, a);
        ld_item<T, VEC>(p1 + (size_t)c * HW, b);
        const float wc = w[c];
#pragma unroll
        for (int j = 0; j < WN; j++) {
            const Quot qa = nrm(a[j], Aa[j], ra[j]), qb = nrm(b[j], Ab[j], rb[j]);
            const float ah = qa.value(), bh = qb.value(), we = wc * nd(qa, qb);
            o0[j] = k * (we * ra[j] - tt[j] * ah * ia[j]);
            o1[j] = k * (tt[WN + j] * bh * ib[j] - we * rb[j]);
        }
        if (df0) st_item<T, VEC>(df0 + base + (size_t)c * HW, o0);
        if (df1) st_item<T, VEC>(df1 + base + (size_t)c * HW, o1);
    }
}

// ---- input pass
// LPIPS's scaling layer composed with [0, 1] -> [-1, 1]: v -> (2 v - 1 - shift_c) / scale_c
__device__ __forceinline__ float lp_shift(int c) { return c == 0 ? -.030f : c == 1 ? -.088f : -.188f; }
__device__ __forceinline__ float lp_scale(int c) { return c == 0 ? .458f : c == 1 ? .448f : .450f; }

// the two source taps of destination index d and the weight of the upper one (torch, align_corners = False)
__device__ __forceinline__ void taps(int d, float scale, int S, int &i0, int &i1, float &l1) {
    const float s = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
    i0 = min((int)s, S - 1);
    i1 = i0 + (i0 < S - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

template <class T>
__global__ __launch_bounds__(LPI_THREADS) void k_lpips_prep(int S, int R, size_t total, float scale,
                                                            const float *__restrict__ pred,
                                                            const float *__restrict__ gt,
                                                            const float *__restrict__ mask,
                                                            const float *__restrict__ bg, T *__restrict__ xp,
                                                            T *__restrict__ xg) {
    const size_t idx = (size_t)blockIdx.x * LPI_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t RR = (size_t)R * R, SS = (size_t)S * S, m = idx / RR, rem = idx - m * RR;
    const int y = (int)(rem / R), x = (int)(rem - (size_t)y * R);
    int y0, y1, x0, x1;
    float ly, lx;
    taps(y, scale, S, y0, y1, ly);
    taps(x, scale, S, x0, x1, lx);
    const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
    const size_t s00 = (size_t)y0 * S + x0, s01 = (size_t)y0 * S + x1, s10 = (size_t)y1 * S + x0,
                 s11 = (size_t)y1 * S + x1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *p = pred + (m * 3 + c) * SS;
        const float v = (w00 * p[s00] + w01 * p[s01]) + (w10 * p[s10] + w11 * p[s11]);
        xp[(m * 3 + c) * RR + rem] = from_f<T>((2.f * v - 1.f - lp_shift(c)) / lp_scale(c));
    }
    if (!gt) return;
    float m00 = 1.f, m01 = 1.f, m10 = 1.f, m11 = 1.f;
    if (mask) {
        const float *mk = mask + m * SS;
        m00 = mk[s00], m01 = mk[s01], m10 = mk[s10], m11 = mk[s11];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *p = gt + (m * 3 + c) * SS;
        const float b = mask ? bg[c] : 0.f;
        const float v = (w00 * (p[s00] * m00 + b * (1.f - m00)) + w01 * (p[s01] * m01 + b * (1.f - m01))) +
                        (w10 * (p[s10] * m10 + b * (1.f - m10)) + w11 * (p[s11] * m11 + b * (1.f - m11)));
        xg[(m * 3 + c) * RR + rem] = from_f<T>((2.f * v - 1.f - lp_shift(c)) / lp_scale(c));
    }
}

// the weight with which destination index d taps source index s
__device__ __forceinline__ float tap_weight(int d, int s, float scale, int S) {
    int i0, i1;
    float l1;
    taps(d, scale, S, i0, i1, l1);
    return (i0 == s ? 1.f - l1 : 0.f) + (i1 == s ? l1 : 0.f);
}

template <class T>
__global__ __launch_bounds__(LPI_THREADS) void k_lpips_prep_bwd(int S, int R, size_t total, float scale,
                                                                const T *__restrict__ dxp,
                                                                float *__restrict__ dpred) {
    const size_t idx = (size_t)blockIdx.x * LPI_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t RR = (size_t)R * R, SS = (size_t)S * S, m = idx / SS, rem = idx - m * SS;
    const int sy = (int)(rem / S), sx = (int)(rem - (size_t)sy * S);
    // destination d taps source s iff its source coordinate lies in [s - 1, s + 1): d in [(s - .5) / scale - .5,
    // (s + 1.5) / scale - .5), widened by one on each side against the rounding of these estimates
    const int ylo = max((int)floorf(((float)sy - 0.5f) / scale - 0.5f) - 1, 0);
    const int yhi = min((int)ceilf(((float)sy + 1.5f) / scale - 0.5f) + 1, R - 1);
    const int xlo = max((int)floorf(((float)sx - 0.5f) / scale - 0.5f) - 1, 0);
    const int xhi = min((int)ceilf(((float)sx + 1.5f) / scale - 0.5f) + 1, R - 1);
    float acc[3] = {0.f, 0.f, 0.f};
    const T *q = dxp + m * 3 * RR;
    for (int y = ylo; y <= yhi; y++) {
        const float wy = tap_weight(y, sy, scale, S);
        if (wy == 0.f) continue;
        for (int x = xlo; x <= xhi; x++) {
            const float wgt = wy * tap_weight(x, sx, scale, S);
            const size_t o = (size_t)y * R + x;
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] = fmaf(wgt, to_f(q[c * RR + o]), acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) dpred[(m * 3 + c) * SS + rem] = acc[c] * (2.f / lp_scale(c));
}

// ---- host side
constexpr int LPI_TEAM_S = 16, LPI_TEAM_M = 64;
// pixel items per workgroup (the other 256 / LP-fold of the workgroup slices the channels)
int lp_of(long long ipp, int C) {
    if (ipp <= 64 || C >= 256) return LPI_TEAM_S;
    if (ipp <= 256 || C >= 32) return LPI_TEAM_M;
    return LPI_THREADS;
}

bool aligned16(const void *a, const void *b, const void *c, const void *d) {
    return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
              reinterpret_cast<uintptr_t>(d)) & 15);
}

struct DistPlan {
    bool vec;
    int lp;
    long long ipp, nT, blocks;
};
DistPlan plan_of(int N, int C, long long HW, bool vec) {
    DistPlan p;
    p.vec = vec;
    p.ipp = vec ? HW / 4 : HW;
    p.lp = lp_of(p.ipp, C);
    p.nT = (p.ipp + p.lp - 1) / p.lp;
    p.blocks = (long long)N * p.nT;
    return p;
}

template <class Fn>
int with_form(bool vec, int lp, Fn &&fn) {
    if (vec) {
        if (lp == LPI_TEAM_S) return fn(std::true_type{}, std::integral_constant<int, LPI_TEAM_S>{});
        if (lp == LPI_TEAM_M) return fn(std::true_type{}, std::integral_constant<int, LPI_TEAM_M>{});
        return fn(std::true_type{}, std::integral_constant<int, LPI_THREADS>{});
    }
    if (lp == LPI_TEAM_S) return fn(std::false_type{}, std::integral_constant<int, LPI_TEAM_S>{});
    if (lp == LPI_TEAM_M) return fn(std::false_type{}, std::integral_constant<int, LPI_TEAM_M>{});
    return fn(std::false_type{}, std::integral_constant<int, LPI_THREADS>{});
}
constexpr const char *DIST_NAMES[2][3] = {{"k_lpips_dist_s16", "k_lpips_dist_s64", "k_lpips_dist_s"},
                                          {"k_lpips_dist_v16", "k_lpips_dist_v64", "k_lpips_dist_v"}};
constexpr const char *DIST_BWD_NAMES[2][3] = {{"k_lpips_dist_bwd_s16", "k_lpips_dist_bwd_s64", "k_lpips_dist_bwd_s"},
                                              {"k_lpips_dist_bwd_v16", "k_lpips_dist_bwd_v64", "k_lpips_dist_bwd_v"}};
const char *form_name(const char *const (&names)[2][3], bool vec, int lp) {
    return names[vec ? 1 : 0][lp == LPI_TEAM_S ? 0 : lp == LPI_TEAM_M ? 1 : 2];
}

// shape and dtype checks shared by the two distance entry points; *empty = true where there is nothing to do
int check_dist(const char *who, int dt0, int dt1, int N, int C, int H, int W, bool *empty) {
    *empty = false;
    if (N < 0 || C <= 0 || H < 0 || W < 0) {
        set_error("%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
        return LGM_E_INVALID;
    }
    if (dt0 != dt1) {
        set_error("%s: f0 and f1 must have one dtype, got %d and %d", who, dt0, dt1);
        return LGM_E_INVALID;
    }
    if (dt0 != LGM_ATTN_F32 && dt0 != LGM_ATTN_BF16 && dt0 != LGM_ATTN_F16) {
        set_error("%s: bad dtype %d", who, dt0);
        return LGM_E_INVALID;
    }
    // 64-bit element offsets: below 2^60 elements no product of the sizes formed later can wrap
    if ((double)N * (double)C * (double)H * (double)W >= 1152921504606846976.0) {
        set_error("%s: N=%d C=%d H=%d W=%d is beyond 2^60 elements", who, N, C, H, W);
        return LGM_E_INVALID;
    }
    // the scalar form launches the most workgroups
    if (plan_of(N, C, (long long)H * W, false).blocks > LPI_GRID_MAX) {
        set_error("%s: N=%d C=%d H=%d W=%d needs a launch grid beyond %lld workgroups", who, N, C, H, W, LPI_GRID_MAX);
        return LGM_E_INVALID;
    }
    if (N == 0 || H == 0 || W == 0) *empty = true;
    return LGM_OK;
}

int check_prep(const char *who, int dt, int M, int S, int R) {
    if (M < 0 || S <= 0 || R <= 0 || S > LPI_SIZE_MAX || R > LPI_SIZE_MAX) {
        set_error("%s: bad shape M=%d S=%d R=%d (S, R in 1 .. %d)", who, M, S, R, LPI_SIZE_MAX);
        return LGM_E_INVALID;
    }
    if (dt != LGM_ATTN_F32 && dt != LGM_ATTN_BF16 && dt != LGM_ATTN_F16) {
        set_error("%s: bad dtype %d", who, dt);
        return LGM_E_INVALID;
    }
    const long long big = S > R ? S : R;
    if (((long long)M * big * big + LPI_THREADS - 1) / LPI_THREADS > LPI_GRID_MAX) {
        set_error("%s: M=%d S=%d R=%d needs a launch grid beyond %lld workgroups", who, M, S, R, LPI_GRID_MAX);
        return LGM_E_INVALID;
    }
    return LGM_OK;
}

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_lpips_dist_workspace_size(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const long long HW = (long long)H * W;
    long long b = lgm::plan_of(N, C, HW, false).blocks;
    if (HW % 4 == 0) {
        const long long bv = lgm::plan_of(N, C, HW, true).blocks;
        b = bv > b ? bv : b;
    }
    return (size_t)b * sizeof(float);
}

extern "C" int lgm_lpips_dist_forward(int dtype_f0, int dtype_f1, int N, int C, int H, int W, float eps,
                                      const void *f0, const void *f1, const float *w, float *out, float *norm0,
                                      float *norm1, void *workspace, size_t workspace_bytes, void *stream,
                                      const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    bool empty;
    const int rc = check_dist("lgm_lpips_dist_forward", dtype_f0, dtype_f1, N, C, H, W, &empty);
    if (rc != LGM_OK || N == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!out) {
        set_error("lgm_lpips_dist_forward: null pointer");
        return LGM_E_INVALID;
    }
    if (empty) {  // no pixels: the mean over none is taken as 0
        if (hipMemsetAsync(out, 0, (size_t)N * sizeof(float), st) != hipSuccess) return LGM_E_HIP;
        return LGM_OK;
    }
    if (!f0 || !f1 || !w || (norm0 == nullptr) != (norm1 == nullptr)) {
        set_error("lgm_lpips_dist_forward: null pointer (f0, f1, w, out; norm0 and norm1 both or neither)");
        return LGM_E_INVALID;
    }
    const size_t need = lgm_lpips_dist_workspace_size(N, C, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("lgm_lpips_dist_forward: workspace too small (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0,
                  need);
        return LGM_E_WORKSPACE;
    }
    const long long HW = (long long)H * W;
    const DistPlan p = plan_of(N, C, HW, HW % 4 == 0 && aligned16(f0, f1, norm0, norm1));
    float *part = (float *)workspace;
    return with_type("lgm_lpips_dist_forward", dtype_f0, [&](auto ty) {
        using T = decltype(ty);
        return with_form(p.vec, p.lp, [&](auto vec_, auto lp_) {
            constexpr bool VEC = decltype(vec_)::value;
            constexpr int LP = decltype(lp_)::value;
            LGM_LAUNCH(form_name(DIST_NAMES, VEC, LP), st,
                       (k_lpips_dist<T, VEC, LP><<<(unsigned)p.blocks, LPI_THREADS, 0, st>>>(
                           C, (size_t)HW, p.ipp, (int)p.nT, eps, (const T *)f0, (const T *)f1, w, norm0, norm1, part)));
            LGM_LAUNCH("k_lpips_dist_sum", st,
                       (k_lpips_dist_sum<<<(unsigned)N, LPI_THREADS, 0, st>>>((int)p.nT, (float)HW, part, out)));
            return LGM_OK;
        });
    });
}

extern "C" int lgm_lpips_dist_backward(int dtype_f0, int dtype_f1, int N, int C, int H, int W, float eps,
                                       const void *f0, const void *f1, const float *w, const float *norm0,
                                       const float *norm1, const float *g, void *df0, void *df1, void *stream,
                                       const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    bool empty;
    const int rc = check_dist("lgm_lpips_dist_backward", dtype_f0, dtype_f1, N, C, H, W, &empty);
    if (rc != LGM_OK || empty || (!df0 && !df1)) return rc;
    if (!f0 || !f1 || !w || !norm0 || !norm1 || !g) {
        set_error("lgm_lpips_dist_backward: null pointer");
        return LGM_E_INVALID;
    }
    const long long HW = (long long)H * W;
    const bool al = aligned16(f0, f1, norm0, norm1) && aligned16(df0, df1, nullptr, nullptr);
    const DistPlan p = plan_of(N, C, HW, HW % 4 == 0 && al);
    hipStream_t st = (hipStream_t)stream;
    return with_type("lgm_lpips_dist_backward", dtype_f0, [&](auto ty) {
        using T = decltype(ty);
        return with_form(p.vec, p.lp, [&](auto vec_, auto lp_) {
            constexpr bool VEC = decltype(vec_)::value;
            constexpr int LP = decltype(lp_)::value;
            LGM_LAUNCH(form_name(DIST_BWD_NAMES, VEC, LP), st,
                       (k_lpips_dist_bwd<T, VEC, LP><<<(unsigned)p.blocks, LPI_THREADS, 0, st>>>(
                           C, (size_t)HW, p.ipp, (int)p.nT, eps, (const T *)f0, (const T *)f1, w, norm0, norm1, g,
                           (T *)df0, (T *)df1)));
            return LGM_OK;
        });
    });
}

extern "C" int lgm_lpips_prep_forward(int dtype_x, int M, int S, int R, const float *pred, const float *gt,
                                      const float *mask, const float *bg, void *x_pred, void *x_gt, void *stream,
                                      const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const int rc = check_prep("lgm_lpips_prep_forward", dtype_x, M, S, R);
    if (rc != LGM_OK || M == 0) return rc;
    if (!pred || !x_pred || (gt && !x_gt) || (mask && (!gt || !bg))) {
        set_error("lgm_lpips_prep_forward: null pointer (pred, x_pred; x_gt with gt; gt and bg with mask)");
        return LGM_E_INVALID;
    }
    const size_t total = (size_t)M * R * R;
    const unsigned grid = (unsigned)((total + LPI_THREADS - 1) / LPI_THREADS);
    const float scale = (float)S / (float)R;
    hipStream_t st = (hipStream_t)stream;
    return with_type("lgm_lpips_prep_forward", dtype_x, [&](auto ty) {
        using T = decltype(ty);
        LGM_LAUNCH("k_lpips_prep", st, (k_lpips_prep<T><<<grid, LPI_THREADS, 0, st>>>(S, R, total, scale, pred, gt, mask,
                                                                                      bg, (T *)x_pred, (T *)x_gt)));
        return LGM_OK;
    });
}

extern "C" int lgm_lpips_prep_backward(int dtype_x, int M, int S, int R, const void *d_x_pred, float *d_pred,
                                       void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const int rc = check_prep("lgm_lpips_prep_backward", dtype_x, M, S, R);
    if (rc != LGM_OK || M == 0) return rc;
    if (!d_x_pred || !d_pred) {
        set_error("lgm_lpips_prep_backward: null pointer");
        return LGM_E_INVALID;
    }
    const size_t total = (size_t)M * S * S;
    const unsigned grid = (unsigned)((total + LPI_THREADS - 1) / LPI_THREADS);
    const float scale = (float)S / (float)R;
    hipStream_t st = (hipStream_t)stream;
    return with_type("lgm_lpips_prep_backward", dtype_x, [&](auto ty) {
        using T = decltype(ty);
        LGM_LAUNCH("k_lpips_prep_bwd", st, (k_lpips_prep_bwd<T><<<grid, LPI_THREADS, 0, st>>>(
                                               S, R, total, scale, (const T *)d_x_pred, d_pred)));
        return LGM_OK;
    });
}
