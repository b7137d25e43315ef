// lgm_amd/csrc/render_sh.hip -- view-dependent colour from spherical harmonics (LGM_RENDER_SH_MASK: lgm_render.h
// states the basis, the colour and its gradients; render_layout.h the workspace regions and who zeroes them).
//
// Three passes around the kernels that only know 14-wide rows, none of which changes:
//   k_sh_pack    ahead of the binning: columns 0:14 of the caller's [B,N,11+3K] rows -> the workspace's [B,N,14] copy,
//                which k_bin, k_aa_factor and k_preproc_bwd then read as `gaussians`.
//   k_sh_colour  after the binning (it reads the rects for visibility), ahead of the compositing: one thread per
//                Gaussian keeps its 3K coefficients in registers and walks the scene's views, writing the colour and
//                the clamp mask of every visible (view, Gaussian). k_render_fwd / k_render_bwd stage that colour.
//   k_sh_bwd     after k_preproc_bwd: one thread (the only writer) per Gaussian walks the views in order, turns the
//                per-view colour partials into dL/dsh and the position term, and writes the caller's wide gradient row
//                from them and k_preproc_bwd's 14-wide row. No atomics; the sums run in a fixed order.
#include "render_common.h"

namespace lgm {
namespace {

constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f,
                            0.5462742152960396f};
constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                            -0.4570457994644658f, 1.445305721320277f,  -0.5900435899266435f};
constexpr int SH_VCHUNK = 64;  // views whose camera positions a workgroup holds in LDS at a time

constexpr int sh_k(int D) { return (D + 1) * (D + 1); }

// Y_0 .. Y_{K-1} at the unit vector (x, y, z): the 3DGS rasteriser's real basis
template <int D>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float (&Y)[sh_k(D)]) {
    Y[0] = SH_C0;
    Y[1] = -SH_C1 * y;
    Y[2] = SH_C1 * z;
    Y[3] = -SH_C1 * x;
    if constexpr (D > 1) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = SH_C2[0] * (x * y);
        Y[5] = SH_C2[1] * (y * z);
        Y[6] = SH_C2[2] * (2.f * zz - xx - yy);
        Y[7] = SH_C2[3] * (x * z);
        Y[8] = SH_C2[4] * (xx - yy);
        if constexpr (D > 2) {
            Y[9] = SH_C3[0] * y * (3.f * xx - yy);
            Y[10] = SH_C3[1] * (x * y) * z;
            Y[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
            Y[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
            Y[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
            Y[14] = SH_C3[5] * z * (xx - yy);
            Y[15] = SH_C3[6] * x * (xx - 3.f * yy);
        }
    }
}

// g = sum_k w[k] dY_k/d(x, y, z), the basis polynomials differentiated as written (k = 0 is constant)
template <int D>
__device__ __forceinline__ void sh_basis_grad(float x, float y, float z, const float (&w)[sh_k(D)], float (&g)[3]) {
    g[0] = -SH_C1 * w[3];
    g[1] = -SH_C1 * w[1];
    g[2] = SH_C1 * w[2];
    if constexpr (D > 1) {
        g[0] += SH_C2[0] * y * w[4] + SH_C2[2] * -2.f * x * w[6] + SH_C2[3] * z * w[7] + SH_C2[4] * 2.f * x * w[8];
        g[1] += SH_C2[0] * x * w[4] + SH_C2[1] * z * w[5] + SH_C2[2] * -2.f * y * w[6] + SH_C2[4] * -2.f * y * w[8];
        g[2] += SH_C2[1] * y * w[5] + SH_C2[2] * 4.f * z * w[6] + SH_C2[3] * x * w[7];
        if constexpr (D > 2) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
            g[0] += SH_C3[0] * 6.f * xy * w[9] + SH_C3[1] * yz * w[10] + SH_C3[2] * -2.f * xy * w[11] +
                    SH_C3[3] * -6.f * xz * w[12] + SH_C3[4] * (4.f * zz - 3.f * xx - yy) * w[13] +
                    SH_C3[5] * 2.f * xz * w[14] + SH_C3[6] * 3.f * (xx - yy) * w[15];
            g[1] += SH_C3[0] * 3.f * (xx - yy) * w[9] + SH_C3[1] * xz * w[10] +
                    SH_C3[2] * (4.f * zz - xx - 3.f * yy) * w[11] + SH_C3[3] * -6.f * yz * w[12] +
                    SH_C3[4] * -2.f * xy * w[13] + SH_C3[5] * -2.f * yz * w[14] + SH_C3[6] * -6.f * xy * w[15];
            g[2] += SH_C3[1] * xy * w[10] + SH_C3[2] * 8.f * yz * w[11] +
                    SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy) * w[12] + SH_C3[4] * 8.f * xz * w[13] +
                    SH_C3[5] * (xx - yy) * w[14];
        }
    }
}

// campos = -t M^-1 of view matrix `m` (row-vector convention: M = rows 0..2, t = row 3), the inverse in fp64
__device__ __forceinline__ void sh_campos(const float *__restrict__ m, float (&c)[3]) {
    const double a = m[0], b = m[1], cc = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double A = e * i - f * h, B = cc * h - b * i, C = b * f - cc * e;  // the adjugate, row by row
    const double Dd = f * g - d * i, E = a * i - cc * g, F = cc * d - a * f;
    const double G = d * h - e * g, H = b * g - a * h, I = a * e - b * d;
    const double id = 1.0 / (a * A + b * Dd + cc * G);
    const double tx = m[12], ty = m[13], tz = m[14];
    c[0] = (float)(-(tx * A + ty * Dd + tz * G) * id);
    c[1] = (float)(-(tx * B + ty * E + tz * H) * id);
    c[2] = (float)(-(tx * C + ty * F + tz * I) * id);
}

// the camera positions of views [v0, v0 + SH_VCHUNK) of scene b -> LDS, once per workgroup (barriers inside: every
// thread of the workgroup calls it)
__device__ __forceinline__ void sh_stage_campos(const Dims &d, const float *__restrict__ views, int b, int v0,
                                                float (*s_cam)[3]) {
    __syncthreads();  // the previous chunk's readers are done
    const int v = v0 + (int)threadIdx.x;
    if (threadIdx.x < SH_VCHUNK && v < d.V) {
        float c[3];
        sh_campos(views + 16 * ((size_t)b * d.V + v), c);
        s_cam[threadIdx.x][0] = c[0];
        s_cam[threadIdx.x][1] = c[1];
        s_cam[threadIdx.x][2] = c[2];
    }
    __syncthreads();
}

__device__ __forceinline__ bool sh_visible(uint2 r) { return (r.x & 0xffff) != (r.y & 0xffff); }

// the unit direction from the camera to p, and 1 / |p - campos|
__device__ __forceinline__ void sh_dir(const float (&p)[3], const float *cam, float (&dir)[3], float &ilen) {
    const float dx = p[0] - cam[0], dy = p[1] - cam[1], dz = p[2] - cam[2];
    ilen = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    dir[0] = dx * ilen;
    dir[1] = dy * ilen;
    dir[2] = dz * ilen;
}

// k_sh_pack: grid (ceil(B N 14 / 256)), block 256. wide [B N, WD] -> g14 [B N, 14] (columns 0:14)
__global__ __launch_bounds__(256) void k_sh_pack(long long n14, int WD, const float *__restrict__ wide,
                                                 float *__restrict__ g14) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n14) return;
    const long long r = e / 14;
    g14[e] = wide[r * WD + (e - r * 14)];
}

// k_sh_colour: grid (ceil(N / 256), B), block 256.
template <int D>
__global__ __launch_bounds__(256) void k_sh_colour(Dims d, const float *__restrict__ wide,
                                                   const float *__restrict__ views, const uint2 *__restrict__ rects,
                                                   float *__restrict__ col, unsigned char *__restrict__ mask) {
    constexpr int K = sh_k(D), WD = 11 + 3 * K;
    __shared__ float s_cam[SH_VCHUNK][3];
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const bool live = i < d.N;
    float p[3] = {0.f, 0.f, 0.f}, sh[3 * K];
    if (live) {  // the row's 3K coefficients: read once, used for every view of the scene
        const float *row = wide + ((size_t)b * d.N + i) * WD;
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = row[c];
#pragma unroll
        for (int e = 0; e < 3 * K; e++) sh[e] = row[11 + e];
    }
    for (int v0 = 0; v0 < d.V; v0 += SH_VCHUNK) {
        sh_stage_campos(d, views, b, v0, s_cam);
        if (!live) continue;
        const int nv = min(SH_VCHUNK, d.V - v0);
        for (int vv = 0; vv < nv; vv++) {
            const size_t k = ((size_t)b * d.V + v0 + vv) * d.N + i;
            if (!sh_visible(rects[k])) continue;  // cut by the preprocess: no colour from this view
            float dir[3], ilen, Y[K];
            sh_dir(p, s_cam[vv], dir, ilen);
            sh_basis<D>(dir[0], dir[1], dir[2], Y);
            unsigned m = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float s = 0.f;
#pragma unroll
                for (int kk = 0; kk < K; kk++) s = fmaf(Y[kk], sh[3 * kk + c], s);
                s += 0.5f;
                m |= s > 0.f ? 1u << c : 0u;
                col[3 * k + c] = fmaxf(s, 0.f);
            }
            mask[k] = (unsigned char)m;
        }
    }
}

// k_sh_bwd: grid (ceil(N / 256), B), block 256. dg14: k_preproc_bwd's [B,N,14] gradient rows; d_wide: the caller's
// [B,N,11+3K] (overwritten).
template <int D>
__global__ __launch_bounds__(256) void k_sh_bwd(Dims d, const float *__restrict__ wide,
                                                const float *__restrict__ views, const uint2 *__restrict__ rects,
                                                const unsigned char *__restrict__ mask,
                                                const float *__restrict__ dg14, float *__restrict__ d_wide,
                                                const unsigned *__restrict__ det_max,
                                                const unsigned *__restrict__ det_sat) {
    constexpr int K = sh_k(D), WD = 11 + 3 * K;
    __shared__ float s_cam[SH_VCHUNK][3];
    const bool det = (d.options & LGM_RENDER_DETERMINISTIC) != 0;
    const int det_s = det ? det_seed_shift(det_max) : 0;
    const bool det_bad = det && *det_sat != 0u;  // a fixed-point flush overflowed (k_render_bwd): poison the call
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const bool live = i < d.N;
    float p[3] = {0.f, 0.f, 0.f}, sh[3 * K], dsh[3 * K], dp[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 3 * K; e++) dsh[e] = 0.f;
    if (live) {
        const float *row = wide + ((size_t)b * d.N + i) * WD;
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = row[c];
#pragma unroll
        for (int e = 0; e < 3 * K; e++) sh[e] = row[11 + e];
    }
    for (int v0 = 0; v0 < d.V; v0 += SH_VCHUNK) {
        sh_stage_campos(d, views, b, v0, s_cam);
        if (!live) continue;
        const int nv = min(SH_VCHUNK, d.V - v0);
        for (int vv = 0; vv < nv; vv++) {  // the scene's views, in order
            const size_t k = ((size_t)b * d.V + v0 + vv) * d.N + i;
            if (!sh_visible(rects[k])) continue;  // no gradient from a view that cut the record
            const unsigned m = mask[k];
            float G[3];  // m_vc G_vc
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float g = det ? (float)ldexp((double)reinterpret_cast<const long long *>(d.sh_part)[3 * k + c],
                                                   -det_s)
                                    : reinterpret_cast<const float *>(d.sh_part)[3 * k + c];
                G[c] = (m >> c) & 1u ? g : 0.f;
            }
            float dir[3], ilen, Y[K], wk[K];
            sh_dir(p, s_cam[vv], dir, ilen);
            sh_basis<D>(dir[0], dir[1], dir[2], Y);
#pragma unroll
            for (int kk = 0; kk < K; kk++) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    dsh[3 * kk + c] = fmaf(Y[kk], G[c], dsh[3 * kk + c]);
                    s = fmaf(G[c], sh[3 * kk + c], s);
                }
                wk[kk] = s;
            }
            float g[3];
            sh_basis_grad<D>(dir[0], dir[1], dir[2], wk, g);
            // through dir = v / |v|: (g - dir (dir . g)) / |v|
            const float dg = dir[0] * g[0] + dir[1] * g[1] + dir[2] * g[2];
#pragma unroll
            for (int c = 0; c < 3; c++) dp[c] += (g[c] - dir[c] * dg) * ilen;
        }
    }
    if (!live) return;
    const float *src = dg14 + ((size_t)b * d.N + i) * 14;
    float *o = d_wide + ((size_t)b * d.N + i) * WD;
    const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int c = 0; c < 11; c++) o[c] = src[c] + (c < 3 ? dp[c] : 0.f);  // (k_preproc_bwd wrote NaN if det_bad)
#pragma unroll
    for (int e = 0; e < 3 * K; e++) o[11 + e] = det_bad ? qnan : dsh[e];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
int launch_sh_pack(const Dims &d, int degree, const float *wide, const Workspace &w, const Layout &L,
                   hipStream_t st) {
    if (d.N == 0) return LGM_OK;
    // the per-view colour partials start at zero here (AccumLayout: who zeroes what)
    if (hipMemsetAsync(w.sh_part, 0, L.acc.sh_part.bytes, st) != hipSuccess) {
        set_error("hipMemsetAsync failed");
        return LGM_E_HIP;
    }
    const long long n14 = (long long)d.B * d.N * 14;
    LGM_LAUNCH("k_sh_pack", st, (k_sh_pack<<<(unsigned)((n14 + 255) / 256), 256, 0, st>>>(
                                    n14, sh_row_width(degree), wide, w.sh_g14)));
    return LGM_OK;
}

int launch_sh_colour(const Dims &d, int degree, const float *wide, const float *cam_view, const Workspace &w,
                     hipStream_t st) {
    if (d.N == 0) return LGM_OK;
    auto k = degree == 1 ? k_sh_colour<1> : degree == 2 ? k_sh_colour<2> : k_sh_colour<3>;
    LGM_LAUNCH("k_sh_colour", st, (k<<<dim3((d.N + 255) / 256, d.B), 256, 0, st>>>(d, wide, cam_view, w.rects, w.sh_col,
                                                                                  w.sh_mask)));
    return LGM_OK;
}

int launch_sh_bwd(const Dims &d, int degree, const float *wide, const float *cam_view, float *d_wide,
                  const Workspace &w, hipStream_t st) {
    auto k = degree == 1 ? k_sh_bwd<1> : degree == 2 ? k_sh_bwd<2> : k_sh_bwd<3>;
    LGM_LAUNCH("k_sh_bwd", st, (k<<<dim3((d.N + 255) / 256, d.B), 256, 0, st>>>(d, wide, cam_view, w.rects, w.sh_mask,
                                                                               w.sh_dg14, d_wide, w.detmax,
                                                                               w.det_sat)));
    return LGM_OK;
}

}  // namespace lgm
