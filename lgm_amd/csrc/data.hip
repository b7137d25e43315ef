// lgm_amd/csrc/data.hip -- the training-batch assembly of include/lgm_data.h: what a provider does after the PNG
// decode (core/provider_lvis.py:166-213, core/utils.py), from decoded RGBA views and raw poses to LGM.forward's `data`.
//
//   k_data_cameras  one lane per view, fp64: pose normalisation, the orbit jitter of the input poses, the COLMAP flip
//                   and cam_view / cam_view_proj / cam_pos by the adjugate of the 3x3 block; each output rounded once.
//   k_data_out      images_output and masks_output: one thread per 4 consecutive destination pixels of a row; per
//                   pixel four RGBA texels (one 4-byte load each for u8), composited on white per texel and blended.
//   k_data_in       input: a workgroup stays inside one view, so the view's pose, knot count (a launch argument) and
//                   resize scales are uniform; the knots sit in LDS. One thread per 4 consecutive pixels of a row:
//                   the three image planes (the resize sample, or for a distorted view the four grid_sample taps,
//                   each a resize sample of the source: the h x h view is never stored) and the six Pluecker planes.
// The pass is bandwidth-bound: the source is read as it was decoded (u8: 4 bytes per texel, neighbouring pixels'
// taps meet in cache), no fp32 intermediate is stored, and every plane is written once, as float4 when the row
// length and the pointer allow. Sample coordinates are fp64 (a handful of operations per thread): the tap index and
// weight are then exact to fp32 rounding at any size, where an fp32 coordinate loses 2^-24 * S of the weight.
// No atomics; one thread owns each output element.
#include "common.h"
#include "lgm_data.h"

namespace lgm {
namespace {

constexpr int DAT_THREADS = 256;
constexpr long long DAT_GRID_MAX = 2147483647LL;
constexpr int DAT_SIZE_MAX = 32768;
constexpr int DAT_CHUNK = 256;  // views per k_data_in launch: their knot counts travel as launch arguments
constexpr int KN = LGM_DATA_MAX_KNOTS;

struct KnotCounts {
    unsigned w[DAT_CHUNK / 4];  // one byte per view
};

// ---------------------------------------------------------------- cameras

struct Pose {
    double R[3][3], t[3];
};

__device__ __forceinline__ Pose load_pose(const float *m) {
    Pose p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) p.R[i][j] = (double)m[i * 4 + j];
        p.t[i] = (double)m[i * 4 + 3];
    }
    return p;
}

__device__ __forceinline__ void store_pose(float *m, const Pose &p) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) m[i * 4 + j] = (float)p.R[i][j];
        m[i * 4 + 3] = (float)p.t[i];
    }
    m[12] = 0.f, m[13] = 0.f, m[14] = 0.f, m[15] = 1.f;
}

// the values of the pose as fp32 holds them
__device__ __forceinline__ void round_pose(Pose &p) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) p.R[i][j] = (double)(float)p.R[i][j];
        p.t[i] = (double)(float)p.t[i];
    }
}

// inverse of a 3x3 block: adjugate / determinant (row i of the inverse = c_{i+1} x c_{i+2} / det, c_k the columns)
__device__ __forceinline__ void inv3(const double (&R)[3][3], double (&I)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        I[i][0] = R[1][a] * R[2][b] - R[2][a] * R[1][b];
        I[i][1] = R[2][a] * R[0][b] - R[0][a] * R[2][b];
        I[i][2] = R[0][a] * R[1][b] - R[1][a] * R[0][b];
    }
    const double det = R[0][0] * I[0][0] + R[1][0] * I[0][1] + R[2][0] * I[0][2];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) I[i][j] /= det;
}

__device__ __forceinline__ void mul33(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}

__device__ __forceinline__ double sinc(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// I + a K + b K^2 with K = [r]_x: exactly the identity at r = 0
__device__ __forceinline__ void rodrigues(const double (&r)[3], double (&M)[3][3]) {
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const double a = sinc(th), h = sinc(0.5 * th), b = 0.5 * h * h;
    const double K[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
    double K2[3][3];
    mul33(K, K, K2);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * K2[i][j];
}

__global__ __launch_bounds__(64) void k_data_cameras(int B, int V, int Vi, const float *__restrict__ c2w,
                                                     const float *__restrict__ jitter, double strength, double radius,
                                                     double p00, double p22, double p32, float *__restrict__ pose_in,
                                                     float *__restrict__ cam_view, float *__restrict__ cam_view_proj,
                                                     float *__restrict__ cam_pos, float *__restrict__ c2w_colmap) {
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (long long)B * V) return;
    const int b = (int)(idx / V), v = (int)(idx - (long long)b * V);
    const Pose A0 = load_pose(c2w + (size_t)b * V * 16), A = load_pose(c2w + (size_t)idx * 16);
    // P = T(0, 0, radius) inv(A0) A = [R0^-1 R, R0^-1 (t - t0) + (0, 0, radius)]
    double R0i[3][3];
    inv3(A0.R, R0i);
    Pose P;
    mul33(R0i, A.R, P.R);
    const double dt[3] = {A.t[0] - A0.t[0], A.t[1] - A0.t[1], A.t[2] - A0.t[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) P.t[i] = R0i[i][0] * dt[0] + R0i[i][1] * dt[1] + R0i[i][2] * dt[2];
    P.t[2] += radius;
    round_pose(P);

    if (v < Vi) {
        const size_t iv = (size_t)b * Vi + v;
        Pose J = P;
        if (jitter) {
            const double PI = 3.14159265358979323846;
            const double u0 = (double)jitter[iv * 2], u1 = (double)jitter[iv * 2 + 1];
            const double sx = strength * PI * u0, sy = strength * PI / 2 * u1;
            const double rx[3] = {P.R[0][1] * sx, P.R[1][1] * sx, P.R[2][1] * sx};
            const double ry[3] = {P.R[0][0] * sy, P.R[1][0] * sy, P.R[2][0] * sy};
            double Mx[3][3], My[3][3], rot[3][3];
            rodrigues(rx, Mx);
            rodrigues(ry, My);
            mul33(Mx, My, rot);
            mul33(rot, P.R, J.R);
#pragma unroll
            for (int i = 0; i < 3; i++) J.t[i] = rot[i][0] * P.t[0] + rot[i][1] * P.t[1] + rot[i][2] * P.t[2];
        }
        store_pose(pose_in + iv * 16, J);
    }

    // OpenGL -> COLMAP: up and forward flipped
#pragma unroll
    for (int i = 0; i < 3; i++) P.R[i][1] = -P.R[i][1], P.R[i][2] = -P.R[i][2];
    if (c2w_colmap && v < Vi) store_pose(c2w_colmap + ((size_t)b * Vi + v) * 16, P);
    double Ri[3][3], ti[3];
    inv3(P.R, Ri);
#pragma unroll
    for (int i = 0; i < 3; i++) ti[i] = -(Ri[i][0] * P.t[0] + Ri[i][1] * P.t[1] + Ri[i][2] * P.t[2]);
    // cam_view = inv(P')^T: rows 0..2 hold R^-T, row 3 the translation
    float *cv = cam_view + (size_t)idx * 16, *cvp = cam_view_proj + (size_t)idx * 16;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double c0 = i < 3 ? Ri[0][i] : ti[0], c1 = i < 3 ? Ri[1][i] : ti[1], c2 = i < 3 ? Ri[2][i] : ti[2];
        const double c3 = i < 3 ? 0.0 : 1.0;
        cv[i * 4 + 0] = (float)c0, cv[i * 4 + 1] = (float)c1, cv[i * 4 + 2] = (float)c2, cv[i * 4 + 3] = (float)c3;
        cvp[i * 4 + 0] = (float)(c0 * p00), cvp[i * 4 + 1] = (float)(c1 * p00);
        cvp[i * 4 + 2] = (float)(c2 * p22 + c3 * p32), cvp[i * 4 + 3] = (float)c2;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) cam_pos[(size_t)idx * 3 + i] = (float)(-P.t[i]);
}

// ---------------------------------------------------------------- views

// u / 255 for a byte u, correctly rounded (equal to the fp32 division for all 256 values, which
// tests/test_data_gpu.py checks): the product with fl(1 / 255) and one residual correction -- three operations where
// the IEEE division is a dozen, in a pass whose forward is otherwise a handful of operations per texel
__device__ __forceinline__ float unorm8(float u) {
#pragma clang fp contract(off)  // (the product must stay a product: the residual is taken from it as rounded)
    const float rc = 1.f / 255.f, q = u * rc;
    return fmaf(fmaf(-q, 255.f, u), rc, q);
}

// one RGBA texel as four values in [0, 1]
__device__ __forceinline__ float4 ld_texel(const uchar4 *p, size_t i) {
    const uchar4 t = p[i];
    return make_float4(unorm8((float)t.x), unorm8((float)t.y), unorm8((float)t.z), unorm8((float)t.w));
}
__device__ __forceinline__ float4 ld_texel(const float4 *p, size_t i) { return p[i]; }

// the two source taps of destination index d and the weight of the upper one (torch, align_corners = False);
// scale = S / R
struct Tap {
    int i0, i1;
    float l;
};
__device__ __forceinline__ Tap tap_of(int d, double scale, int S) {
    const double s = fmax(((double)d + 0.5) * scale - 0.5, 0.0);
    Tap t;
    t.i0 = min((int)s, S - 1);
    t.i1 = min(t.i0 + 1, S - 1);
    t.l = (float)(s - (double)t.i0);
    return t;
}

// composite on white: (r, g, b, a) -> (r a + 1 - a, ..., a)
__device__ __forceinline__ float4 on_white(float4 t, bool swap) {
    const float a = t.w, w = 1.f - a;
    const float r = swap ? t.z : t.x, b = swap ? t.x : t.z;
    return make_float4(r * a + w, t.y * a + w, b * a + w, a);
}

__device__ __forceinline__ float blend(float f00, float f01, float f10, float f11, float lx, float ly) {
    return (1.f - ly) * ((1.f - lx) * f00 + lx * f01) + ly * ((1.f - lx) * f10 + lx * f11);
}

// the resize sample of the view `img` (Hs x Ws texels) at taps ty, tx: composited colour and alpha
template <class S>
__device__ __forceinline__ float4 resize_sample(const S *__restrict__ img, int Ws, const Tap &ty, const Tap &tx,
                                                bool swap) {
    const size_t r0 = (size_t)ty.i0 * Ws, r1 = (size_t)ty.i1 * Ws;
    const float4 f00 = on_white(ld_texel(img, r0 + tx.i0), swap), f01 = on_white(ld_texel(img, r0 + tx.i1), swap);
    const float4 f10 = on_white(ld_texel(img, r1 + tx.i0), swap), f11 = on_white(ld_texel(img, r1 + tx.i1), swap);
    return make_float4(blend(f00.x, f01.x, f10.x, f11.x, tx.l, ty.l), blend(f00.y, f01.y, f10.y, f11.y, tx.l, ty.l),
                       blend(f00.z, f01.z, f10.z, f11.z, tx.l, ty.l), blend(f00.w, f01.w, f10.w, f11.w, tx.l, ty.l));
}

// four consecutive values of a row at p (x0 .. x0 + 3, those below W): one float4 when VEC
template <bool VEC>
__device__ __forceinline__ void st_row4(float *p, const float (&v)[4], int x0, int W) {
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (x0 + k < W) p[k] = v[k];
    }
}

// images_output [M, 3, So, So], masks_output [M, 1, So, So] from src [M, Hs, Ws] texels; W4 = ceil(So / 4)
template <class S, bool VEC>
__global__ __launch_bounds__(DAT_THREADS) void k_data_out(int Hs, int Ws, int So, int W4, size_t total, int swap,
                                                          double sy, double sx, const S *__restrict__ src,
                                                          float *__restrict__ images, float *__restrict__ masks) {
    const size_t idx = (size_t)blockIdx.x * DAT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t per = (size_t)So * W4, m = idx / per, rem = idx - m * per;
    const int y = (int)(rem / W4), x0 = (int)(rem - (size_t)y * W4) * 4;
    const S *img = src + m * (size_t)Hs * Ws;
    const Tap ty = tap_of(y, sy, Hs);
    float o[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = min(x0 + k, So - 1);  // (a lane past the row's end repeats the last pixel and stores nothing)
        const float4 c = resize_sample(img, Ws, ty, tap_of(x, sx, Ws), (swap & LGM_DATA_SWAP_RB) != 0);
        o[0][k] = c.x, o[1][k] = c.y, o[2][k] = c.z, o[3][k] = c.w;
    }
    const size_t SS = (size_t)So * So, at = (size_t)y * So + x0;
#pragma unroll
    for (int c = 0; c < 3; c++) st_row4<VEC>(images + (m * 3 + c) * SS + at, o[c], x0, So);
    st_row4<VEC>(masks + m * SS + at, o[3], x0, So);
}

// the grid coordinate in [-1, 1] of destination index j under the knots k[0 .. n - 1] (include/lgm_data.h)
__device__ __forceinline__ double grid_coord(const int *k, int n, int j) {
    int i = n - 2;
    for (int q = 0; q < n - 1; q++)
        if (k[q] <= j && j < k[q + 1]) {
            i = q;
            break;
        }
    const double g0 = -1.0 + 2.0 * (double)i / (double)(n - 1), g1 = -1.0 + 2.0 * (double)(i + 1) / (double)(n - 1);
    return g0 + (g1 - g0) * (double)(j - k[i]) / (double)max(k[i + 1] - k[i] - 1, 1);
}

// grid_sample's two taps of a coordinate in [-1, 1] on an axis of h pixels (align_corners = False, zeros padding):
// index i0 (may be -1 .. h - 1, tap i0 + 1), weight of the upper tap
__device__ __forceinline__ void warp_taps(double g, int h, int &i0, float &l) {
    const double ix = ((g + 1.0) * (double)h - 1.0) * 0.5, f = floor(ix);
    i0 = (int)f;
    l = (float)(ix - f);
}

// input [*, Vi views, 9, h, h]: this launch covers the views view0 .. view0 + gridDim.x / bpv - 1 of the flattened
// [B * Vi] list; cnt their knot counts. src is indexed by source view: b * V + v.
template <class S, bool VEC>
__global__ __launch_bounds__(DAT_THREADS) void k_data_in(int V, int Vi, int Hs, int Ws, int h, int W4, int bpv,
                                                         int view0, int swap, double sy, double sx, float focal,
                                                         KnotCounts cnt, const S *__restrict__ src,
                                                         const float *__restrict__ pose_in,
                                                         const int *__restrict__ knots, float *__restrict__ input) {
    __shared__ int sk[2 * KN];
    const int lv = blockIdx.x / bpv, blk = blockIdx.x - lv * bpv;
    const int view = view0 + lv, b = view / Vi, v = view - b * Vi;
    const int n = (int)((cnt.w[lv >> 2] >> ((lv & 3) * 8)) & 0xffu);  // uniform over the workgroup
    if (n > 0) {
        if (threadIdx.x < 2 * KN) sk[threadIdx.x] = knots[(size_t)view * (2 * KN) + threadIdx.x];
        __syncthreads();
    }
    const int item = blk * DAT_THREADS + threadIdx.x;
    if (item >= h * W4) return;
    const int y = item / W4, x0 = (item - y * W4) * 4;
    const S *img = src + ((size_t)b * V + v) * (size_t)Hs * Ws;
    const float *P = pose_in + (size_t)view * 16;

    float o[9][4];
    int wy0 = 0;
    float wly = 0.f;
    Tap ty = tap_of(y, sy, Hs);
    if (n > 0) warp_taps(grid_coord(sk + KN, n, y), h, wy0, wly);
    const float hh = 0.5f * (float)h;
    const float dy = -(((float)y - hh + 0.5f) / focal);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = min(x0 + k, h - 1);  // (a lane past the row's end repeats the last pixel and stores nothing)
        float r, g, bl;
        if (n == 0) {
            const float4 c = resize_sample(img, Ws, ty, tap_of(x, sx, Ws), (swap & LGM_DATA_SWAP_RB) != 0);
            r = c.x, g = c.y, bl = c.z;
        } else {
            int wx0;
            float wlx;
            warp_taps(grid_coord(sk, n, x), h, wx0, wlx);
            float4 t[2][2];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const int yy = wy0 + a, xx = wx0 + c;
                    const float w = (a ? wly : 1.f - wly) * (c ? wlx : 1.f - wlx);
                    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (yy >= 0 && yy < h && xx >= 0 && xx < h)
                        s = resize_sample(img, Ws, tap_of(yy, sy, Hs), tap_of(xx, sx, Ws), (swap & LGM_DATA_SWAP_RB) != 0);
                    t[a][c] = make_float4(w * s.x, w * s.y, w * s.z, 0.f);
                }
            r = (t[0][0].x + t[0][1].x) + (t[1][0].x + t[1][1].x);
            g = (t[0][0].y + t[0][1].y) + (t[1][0].y + t[1][1].y);
            bl = (t[0][0].z + t[0][1].z) + (t[1][0].z + t[1][1].z);
        }
        const bool nrm_img = !(swap & LGM_DATA_NO_NORMALIZE);
        o[0][k] = nrm_img ? __fdiv_rn(r - 0.485f, 0.229f) : r;
        o[1][k] = nrm_img ? __fdiv_rn(g - 0.456f, 0.224f) : g;
        o[2][k] = nrm_img ? __fdiv_rn(bl - 0.406f, 0.225f) : bl;
        // the ray through the pixel: d = normalize(R dir), Pluecker (o x d, d)
        const float dx = ((float)x - hh + 0.5f) / focal;
        float d0 = P[0] * dx + P[1] * dy - P[2], d1 = P[4] * dx + P[5] * dy - P[6], d2 = P[8] * dx + P[9] * dy - P[10];
        const float nrm = sqrtf(fmaxf(d0 * d0 + d1 * d1 + d2 * d2, 1e-20f));
        d0 = __fdiv_rn(d0, nrm), d1 = __fdiv_rn(d1, nrm), d2 = __fdiv_rn(d2, nrm);
        const float ox = P[3], oy = P[7], oz = P[11];
        o[3][k] = oy * d2 - oz * d1;
        o[4][k] = oz * d0 - ox * d2;
        o[5][k] = ox * d1 - oy * d0;
        o[6][k] = d0, o[7][k] = d1, o[8][k] = d2;
    }
    const size_t hw = (size_t)h * h;
    float *dst = input + (size_t)view * 9 * hw + (size_t)y * h + x0;
#pragma unroll
    for (int c = 0; c < 9; c++) st_row4<VEC>(dst + c * hw, o[c], x0, h);
}

bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }

template <class S>
int launch_views(int swap, int B, int V, int Vi, int Hs, int Ws, int h, int So, const S *src,
                 const float *pose_in, const int *knots, const int *nknots, double fovy_deg, float *input,
                 float *images, float *masks, hipStream_t st) {
    if (images) {
        const int W4 = (So + 3) / 4;
        const size_t total = (size_t)B * V * So * W4;
        const unsigned grid = (unsigned)((total + DAT_THREADS - 1) / DAT_THREADS);
        const double sy = (double)Hs / So, sx = (double)Ws / So;
        if (So % 4 == 0 && aligned16(images) && aligned16(masks))
            LGM_LAUNCH("k_data_out", st, (k_data_out<S, true><<<grid, DAT_THREADS, 0, st>>>(
                                             Hs, Ws, So, W4, total, swap, sy, sx, src, images, masks)));
        else
            LGM_LAUNCH("k_data_out", st, (k_data_out<S, false><<<grid, DAT_THREADS, 0, st>>>(
                                             Hs, Ws, So, W4, total, swap, sy, sx, src, images, masks)));
    }
    if (input) {
        const int W4 = (h + 3) / 4, bpv = (h * W4 + DAT_THREADS - 1) / DAT_THREADS;
        const double sy = (double)Hs / h, sx = (double)Ws / h;
        const double PI = 3.14159265358979323846;
        const float focal = (float)((double)h * 0.5 / tan(0.5 * fovy_deg * PI / 180.0));
        const bool vec = h % 4 == 0 && aligned16(input);
        const long long views = (long long)B * Vi;
        for (long long v0 = 0; v0 < views; v0 += DAT_CHUNK) {
            const int nv = (int)(views - v0 < DAT_CHUNK ? views - v0 : DAT_CHUNK);
            KnotCounts cnt = {};
            if (knots)
                for (int i = 0; i < nv; i++) cnt.w[i >> 2] |= (unsigned)nknots[v0 + i] << ((i & 3) * 8);
            const unsigned grid = (unsigned)nv * (unsigned)bpv;
            if (vec)
                LGM_LAUNCH("k_data_in", st, (k_data_in<S, true><<<grid, DAT_THREADS, 0, st>>>(
                                                V, Vi, Hs, Ws, h, W4, bpv, (int)v0, swap, sy, sx, focal, cnt, src,
                                                pose_in, knots, input)));
            else
                LGM_LAUNCH("k_data_in", st, (k_data_in<S, false><<<grid, DAT_THREADS, 0, st>>>(
                                                V, Vi, Hs, Ws, h, W4, bpv, (int)v0, swap, sy, sx, focal, cnt, src,
                                                pose_in, knots, input)));
        }
    }
    return LGM_OK;
}

}  // namespace
}  // namespace lgm

extern "C" int lgm_data_cameras(int B, int V, int Vi, const float *c2w, const float *jitter, double jitter_strength,
                                double cam_radius, double fovy_deg, double znear, double zfar, float *pose_in,
                                float *cam_view, float *cam_view_proj, float *cam_pos, float *c2w_colmap, void *stream,
                                const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    if (B < 0 || V <= 0 || Vi <= 0 || Vi > V) {
        set_error("lgm_data_cameras: bad sizes B=%d V=%d Vi=%d (0 < Vi <= V)", B, V, Vi);
        return LGM_E_INVALID;
    }
    if (!(fovy_deg > 0.0 && fovy_deg < 180.0) || !(zfar > znear)) {
        set_error("lgm_data_cameras: bad projection fovy=%g znear=%g zfar=%g", fovy_deg, znear, zfar);
        return LGM_E_INVALID;
    }
    if (B == 0) return LGM_OK;
    if (!c2w || !pose_in || !cam_view || !cam_view_proj || !cam_pos) {
        set_error("lgm_data_cameras: null pointer (c2w, pose_in, cam_view, cam_view_proj, cam_pos)");
        return LGM_E_INVALID;
    }
    const long long blocks = ((long long)B * V + 63) / 64;
    if (blocks > DAT_GRID_MAX) {
        set_error("lgm_data_cameras: B=%d V=%d needs a launch grid beyond %lld workgroups", B, V, DAT_GRID_MAX);
        return LGM_E_INVALID;
    }
    // proj as the fp32 matrix of core/provider_lvis.py:59-65 holds it
    const double PI = 3.14159265358979323846;
    const double p00 = (double)(float)(1.0 / tan(0.5 * fovy_deg * PI / 180.0));
    const double p22 = (double)(float)((zfar + znear) / (zfar - znear));
    const double p32 = (double)(float)(-(zfar * znear) / (zfar - znear));
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_data_cameras", st, (k_data_cameras<<<(unsigned)blocks, 64, 0, st>>>(
                                         B, V, Vi, c2w, jitter, jitter_strength, cam_radius, p00, p22, p32, pose_in,
                                         cam_view, cam_view_proj, cam_pos, c2w_colmap)));
    return LGM_OK;
}

extern "C" int lgm_data_views(int dtype_src, int swap_rb, int B, int V, int Vi, int Hs, int Ws, int h, int So,
                              const void *src, const float *pose_in, const int *knots, const int *nknots,
                              double fovy_deg, float *input, float *images_output, float *masks_output, void *stream,
                              const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_data_views";
    if (B < 0 || V <= 0 || Vi <= 0 || Vi > V || Hs <= 0 || Ws <= 0 || h <= 0 || So <= 0 || Hs > DAT_SIZE_MAX ||
        Ws > DAT_SIZE_MAX || h > DAT_SIZE_MAX || So > DAT_SIZE_MAX) {
        set_error("%s: bad sizes B=%d V=%d Vi=%d Hs=%d Ws=%d h=%d So=%d (0 < Vi <= V; sizes in 1 .. %d)", who, B, V, Vi,
                  Hs, Ws, h, So, DAT_SIZE_MAX);
        return LGM_E_INVALID;
    }
    if (dtype_src != LGM_DATA_U8 && dtype_src != LGM_ATTN_F32) {
        set_error("%s: bad dtype %d (LGM_DATA_U8 or LGM_ATTN_F32)", who, dtype_src);
        return LGM_E_INVALID;
    }
    if (!(fovy_deg > 0.0 && fovy_deg < 180.0)) {
        set_error("%s: bad fovy %g", who, fovy_deg);
        return LGM_E_INVALID;
    }
    if (B == 0) return LGM_OK;
    if (!src || (input && !pose_in) || (input && knots && !nknots) || (!images_output != !masks_output)) {
        set_error("%s: null pointer (src; pose_in with input; nknots with knots; images_output and masks_output both "
                  "or neither)", who);
        return LGM_E_INVALID;
    }
    if ((size_t)src & (dtype_src == LGM_DATA_U8 ? 3 : 15)) {
        set_error("%s: src is not aligned to its texel", who);
        return LGM_E_INVALID;
    }
    if (input && knots)
        for (long long i = 0; i < (long long)B * Vi; i++)
            if (nknots[i] != 0 && (nknots[i] < 2 || nknots[i] > LGM_DATA_MAX_KNOTS)) {
                set_error("%s: nknots[%lld] = %d is not 0 or 2 .. %d", who, i, nknots[i], LGM_DATA_MAX_KNOTS);
                return LGM_E_INVALID;
            }
    const long long out_blocks = ((long long)B * V * So * ((So + 3) / 4) + DAT_THREADS - 1) / DAT_THREADS;
    const long long in_bpv = ((long long)h * ((h + 3) / 4) + DAT_THREADS - 1) / DAT_THREADS;
    if (out_blocks > DAT_GRID_MAX || in_bpv * DAT_CHUNK > DAT_GRID_MAX || (long long)B * Vi > DAT_GRID_MAX) {
        set_error("%s: B=%d V=%d h=%d So=%d needs a launch grid beyond %lld workgroups", who, B, V, h, So, DAT_GRID_MAX);
        return LGM_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype_src == LGM_DATA_U8)
        return launch_views(swap_rb, B, V, Vi, Hs, Ws, h, So, (const uchar4 *)src, pose_in, knots, nknots,
                            fovy_deg, input, images_output, masks_output, st);
    return launch_views(swap_rb, B, V, Vi, Hs, Ws, h, So, (const float4 *)src, pose_in, knots, nknots, fovy_deg,
                        input, images_output, masks_output, st);
}
