// lgm_amd/csrc/render_preproc_bwd.hip -- the per-Gaussian projection backward, the last
// launch of the render backward.
//
// k_preproc_bwd: one thread per Gaussian, summing over its scene's views in order. It decodes the partials k_render_bwd
// flushed to the accumulators (fp32 with fp64 needle sums, or the deterministic mode's int64 fixed point), recomputes
// the forward's projection (make_proj_bwd / cov2d_bwd) and carries them through cov2D, the perspective divide and
// cov3D to the 14-wide Gaussian rows.
#include "render_common.h"

namespace lgm {
namespace {

// The preprocess backward's recomputation of the forward's projection (make_proj / cov2d / the homogeneous
// divide): FP contraction on and 1-ulp v_rcp_f32 reciprocals. The forward keeps the oracle's bit-exact operation
// order because its integer outputs (radii, tile rects, sort keys) depend on it; here the values only feed
// gradients, and each IEEE division is ~10 VALU of a single thread's serial view chain (k_preproc_bwd 61.1 -> 55.5 us
// on the pool, gradients as accurate or more: profiles/r03/ab_preproc_fast).
__device__ __forceinline__ ProjCtx make_proj_bwd(const float *Vw, float mx, float my, float mz, float fx, float fy,
                                                 float tanx, float tany) {
    ProjCtx P;
    P.t[0] = Vw[0] * mx + Vw[4] * my + Vw[8] * mz + Vw[12];
    P.t[1] = Vw[1] * mx + Vw[5] * my + Vw[9] * mz + Vw[13];
    P.t[2] = Vw[2] * mx + Vw[6] * my + Vw[10] * mz + Vw[14];
    const float limx = 1.3f * tanx, limy = 1.3f * tany, rtz = __builtin_amdgcn_rcpf(P.t[2]);
    const float txtz = P.t[0] * rtz, tytz = P.t[1] * rtz;
    P.t[0] = fminf(limx, fmaxf(-limx, txtz)) * P.t[2];
    P.t[1] = fminf(limy, fmaxf(-limy, tytz)) * P.t[2];
    P.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    P.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    const float J00 = fx * rtz, J02 = -(fx * P.t[0]) * rtz * rtz;
    const float J11 = fy * rtz, J12 = -(fy * P.t[1]) * rtz * rtz;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        P.T0[r] = Vw[4 * r + 0] * J00 + Vw[4 * r + 2] * J02;
        P.T1[r] = Vw[4 * r + 1] * J11 + Vw[4 * r + 2] * J12;
    }
    return P;
}
__device__ __forceinline__ void cov2d_bwd(const ProjCtx &P, const float c3[6], float &a, float &b, float &c, float &a0,
                                          float &c0) {  // (a0, c0: before the dilation, for LGM_RENDER_ANTIALIAS)
    const float S[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float s0[3], s1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s0[k] = S[k][0] * P.T0[0] + S[k][1] * P.T0[1] + S[k][2] * P.T0[2];
        s1[k] = S[k][0] * P.T1[0] + S[k][1] * P.T1[1] + S[k][2] * P.T1[2];
    }
    a0 = P.T0[0] * s0[0] + P.T0[1] * s0[1] + P.T0[2] * s0[2];
    b = s1[0] * P.T0[0] + s1[1] * P.T0[1] + s1[2] * P.T0[2];
    c0 = P.T1[0] * s1[0] + P.T1[1] * s1[1] + P.T1[2] * s1[2];
    a = a0 + 0.3f;
    c = c0 + 0.3f;
}

// k_preproc_bwd: grid (ceil(N/256), B), block 256. Sums over the scene's views in order (deterministic; the
// order must not depend on the launch's size: a batched pool equals its scenes rendered alone, bit for bit).
// LDSV (scenes of up to PRE_MAXV views): the view / projection matrices staged in LDS once per workgroup, the
// Gaussian, its first view's rect + accumulator row and its scene partials loaded before that staging, and view
// v + 1's rect + row loaded while view v is processed. Without it each view paid its global round trip and then two
// scalar-load round trips for the matrices, in series: pool 57.4 -> 52.3 us, one scene 16.5 -> 14.2 us, outputs
// bitwise equal (profiles/r05/ab_preproc_lds).
constexpr int PRE_MAXV = 32;
// AA: LGM_RENDER_ANTIALIAS compiled in (the opacity partial per view, the factor s_v and its derivative: lgm_render.h);
// compile-time, so the plain instantiations keep their registers (as a runtime branch: 91 -> 104 and 106 -> 119 VGPRs).
template <bool LDSV, bool AA = false>
__global__ __launch_bounds__(256) void k_preproc_bwd(Dims d, const float *__restrict__ gauss,
                                                     const float *__restrict__ views,
                                                     const float *__restrict__ projs, const uint2 *__restrict__ rects,
                                                     float *__restrict__ accum, float *__restrict__ d_gauss,
                                                     float *__restrict__ d_means2D, const float4 *__restrict__ gP,
                                                     const float4 *__restrict__ gQ,
                                                     const unsigned *__restrict__ det_max,
                                                     const unsigned *__restrict__ det_sat) {
    const bool det = (d.options & LGM_RENDER_DETERMINISTIC) != 0;
    const int det_s = det ? det_seed_shift(det_max) : 0;
    const bool det_bad = det && *det_sat != 0u;  // a fixed-point flush overflowed (k_render_bwd): poison the call
    // LGM_RENDER_ANTIALIAS: the opacity partial arrives per view (G_v = dL/do^, accum_aa_elem0), not per scene
    constexpr bool aa = AA;
    const size_t aa_off = aa ? accum_aa_elem0(d.B, d.V, d.N, det) : 0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    // diagnostics: workgroup g's start / end in slots [2], [3] of per-tile record g (unused by the other kernels)
    const size_t g_diag = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const bool stamp = d.counters && threadIdx.x == 0 && g_diag < (size_t)d.BV * d.T;
    if (stamp) d.counters[cnt_tile(g_diag) + 2] = __builtin_amdgcn_s_memrealtime();
    const bool live = i < d.N;
    const float fx = d.fx, fy = d.fy, mod = d.mod;
    // float mode: the accumulator row is loaded beside the rect, not after it (one memory round trip per view
    // instead of two; an invisible view's row is uninitialised workspace, loaded and dropped); LDSV: view v + 1's
    // rect and row are loaded while view v is processed
    uint2 r_nx = make_uint2(0u, 0u);
    float2 acc_nx[NACC_V / 2];
    float aa_nx = 0.f, aa_snx = 0.f;  // (antialias) the view's opacity partial (float mode) and factor s_v
    auto load_view = [&](int v) {
        const size_t k = ((size_t)b * d.V + v) * d.N + i;
        r_nx = rects[k];
        if (!det) {
            const float2 *acc2 = reinterpret_cast<const float2 *>(accum + accum_view_elem(k, 0));
#pragma unroll
            for (int q = 0; q < NACC_V / 2; q++) acc_nx[q] = acc2[q];
            if (aa) aa_nx = accum[aa_off + k];
        }
        if (aa) aa_snx = d.aa_s[k];  // (k_aa_factor: the forward's own s_v)
    };
    float g[14];
    const size_t ks = accum_scene_elem(d.BV, d.N, b, i, 0);  // view-independent partials
    float4 acc_s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (LDSV && live) {  // the Gaussian, its first view and its scene partials in flight during the staging
        load_gaussian(gauss + ((size_t)b * d.N + i) * 14, g);
        if (d.V > 0) load_view(0);
        if (!det) acc_s = *reinterpret_cast<const float4 *>(accum + ks);
    }
    // LDSV: the scene's view and projection matrices in LDS, loaded once by the workgroup, so the view loop's reads
    // of them are LDS round trips instead of scalar loads issued after each view's global loads
    __shared__ float s_vp[LDSV ? PRE_MAXV : 1][32];
    if constexpr (LDSV) {
        for (int t = threadIdx.x; t < 32 * d.V; t += blockDim.x) {
            const int v = t >> 5, e = t & 31, bv = b * d.V + v;
            s_vp[v][e] = e < 16 ? views[16 * bv + e] : projs[16 * bv + e - 16];
        }
        __syncthreads();
    }
    if (!live) return;
    if (!LDSV) load_gaussian(gauss + ((size_t)b * d.N + i) * 14, g);
    float R[3][3];
    const float q4[4] = {g[7], g[8], g[9], g[10]};
    quat_rot(q4, R);
    const float s[3] = {mod * g[4], mod * g[5], mod * g[6]};
    float c3[6];
    cov3d(s, R, c3);
    const float Sg[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float dmean[3] = {0, 0, 0}, dcov[6] = {0, 0, 0, 0, 0, 0}, dop = 0, dcol[3] = {0, 0, 0};
    for (int v = 0; v < d.V; v++) {
        const int bv = b * d.V + v;
        const size_t k = (size_t)bv * d.N + i;
        if (!LDSV) load_view(v);
        const uint2 r = r_nx;
        float2 acc_e[NACC_V / 2];
#pragma unroll
        for (int q = 0; q < NACC_V / 2; q++) acc_e[q] = acc_nx[q];
        const float aa_e = aa_nx, sv = aa_snx;
        if (LDSV && v + 1 < d.V) load_view(v + 1);
        const bool vis = (r.x & 0xffff) != (r.y & 0xffff);
        if (!vis) {
            if (d_means2D) { d_means2D[2 * k] = 0.f; d_means2D[2 * k + 1] = 0.f; }
            continue;
        }
        float acc[NACC_V];
        if (det) {  // back from fixed point: the same normalisers k_render_bwd derived from this record
            const longlong2 *acc2 = reinterpret_cast<const longlong2 *>(reinterpret_cast<const long long *>(accum) +
                                                                        accum_view_elem(k, 0));
            const float4 rp = gP[k];
            const DetNorm nm = det_norm(rp.z, rp.w, gQ[k].x, d.W, d.H);
#pragma unroll
            for (int q = 0; q < NACC_V / 2; q++) {
                const longlong2 a = acc2[q];
                acc[2 * q] = (float)ldexp((double)a.x, -(det_s + nm.k[2 * q]));
                acc[2 * q + 1] = (float)ldexp((double)a.y, -(det_s + nm.k[2 * q + 1]));
            }
        } else {  // (zeroed by the forward's epilogue; see LGM_RENDER_BACKWARD_AGAIN)
#pragma unroll
            for (int q = 0; q < NACC_V / 2; q++) {
                acc[2 * q] = acc_e[q].x;
                acc[2 * q + 1] = acc_e[q].y;
            }
        }
        if (!det && (r.y >> 31)) {  // a needle: its conic partials were summed in fp64
            const double *sd = reinterpret_cast<const double *>(accum) + accum_needle_dbl(d.B, d.V, d.N, k, 0);
            acc[2] = (float)sd[0];
            acc[3] = (float)sd[1];
            acc[4] = (float)sd[2];
        }
        const float dm2x = acc[0], dm2y = acc[1];
        const float dcx = acc[2], dcy = acc[3], dcz = acc[4];
        const float ddep = acc[5];
        if (d_means2D) { d_means2D[2 * k] = dm2x; d_means2D[2 * k + 1] = dm2y; }
        const float *Vw = LDSV ? s_vp[v] : views + 16 * bv;
        const float *Pm = LDSV ? s_vp[v] + 16 : projs + 16 * bv;
        // ---- cov2D backward
        const ProjCtx Pc = make_proj_bwd(Vw, g[0], g[1], g[2], fx, fy, d.tanx, d.tany);
        float a, bb, c, a0, c0;
        cov2d_bwd(Pc, c3, a, bb, c, a0, c0);
        const float denom = a * c - bb * bb;
        const float denom2inv = __builtin_amdgcn_rcpf((denom * denom) + 0.0000001f);
        float aa_da = 0, aa_db = 0, aa_dc = 0;
        if (aa) {  // o^ = o s_v, s_v = sqrt(clamp(det0 / det)) (lgm_render.h): dL/do, and dL/ds_v -> a0, b, c0
            float Gv = aa_e;  // dL/do^ of this view
            if (det)
                Gv = (float)ldexp((double)(reinterpret_cast<const long long *>(accum) + aa_off)[k],
                                  -(det_s + det_norm_opacity(gQ[k].y)));
            // s_v is the forward's (fp64-evaluated) factor: at the floor 0.005 or at 1 it is a constant
            const float rdet = __builtin_amdgcn_rcpf(denom);
            const bool open = sv * sv > AA_RMIN && sv < 1.0f;
            dop += sv * Gv;
            if (open) {
                // dL/dr / det^2, and det^2 dr/d(a0, b, c0) with a - a0 = c - c0 = 0.3 put in: (c0 det - det0 c) =
                // 0.3 (c0 c + b^2), (a0 det - det0 a) = 0.3 (a0 a + b^2), det0 - det = -(0.3 (a0 + c0) + 0.09) --
                // the same derivative without the differences of products that cancel for a large splat
                const float dr = 0.5f * g[3] * Gv * __builtin_amdgcn_rcpf(sv) * rdet * rdet;
                aa_da = dr * 0.3f * (c0 * c + bb * bb);
                aa_dc = dr * 0.3f * (a0 * a + bb * bb);
                aa_db = -dr * 2 * bb * (0.3f * (a0 + c0) + 0.09f);
            }
        }
        float dL_da = 0, dL_db = 0, dL_dc = 0;
        if (denom2inv != 0) {
            dL_da = denom2inv * (-c * c * dcx + 2 * bb * c * dcy + (denom - a * c) * dcz);
            dL_dc = denom2inv * (-a * a * dcz + 2 * a * bb * dcy + (denom - a * c) * dcx);
            dL_db = denom2inv * 2 * (bb * c * dcx - (denom + 2 * bb * bb) * dcy + a * bb * dcz);
            if (aa) {  // the opacity factor's share (not added at all without the bit: x + 0 may change a zero's sign)
                dL_da += aa_da;
                dL_db += aa_db;
                dL_dc += aa_dc;
            }
            const float *t0 = Pc.T0, *t1 = Pc.T1;
            dcov[0] += (t0[0] * t0[0] * dL_da + t0[0] * t1[0] * dL_db + t1[0] * t1[0] * dL_dc);
            dcov[3] += (t0[1] * t0[1] * dL_da + t0[1] * t1[1] * dL_db + t1[1] * t1[1] * dL_dc);
            dcov[5] += (t0[2] * t0[2] * dL_da + t0[2] * t1[2] * dL_db + t1[2] * t1[2] * dL_dc);
            dcov[1] += 2 * t0[0] * t0[1] * dL_da + (t0[0] * t1[1] + t0[1] * t1[0]) * dL_db + 2 * t1[0] * t1[1] * dL_dc;
            dcov[2] += 2 * t0[0] * t0[2] * dL_da + (t0[0] * t1[2] + t0[2] * t1[0]) * dL_db + 2 * t1[0] * t1[2] * dL_dc;
            dcov[4] += 2 * t0[2] * t0[1] * dL_da + (t0[1] * t1[2] + t0[2] * t1[1]) * dL_db + 2 * t1[1] * t1[2] * dL_dc;
        }
        float dT0[3], dT1[3];
#pragma unroll
        for (int kk = 0; kk < 3; kk++) {
            const float s0 = Pc.T0[0] * Sg[kk][0] + Pc.T0[1] * Sg[kk][1] + Pc.T0[2] * Sg[kk][2];
            const float s1 = Pc.T1[0] * Sg[kk][0] + Pc.T1[1] * Sg[kk][1] + Pc.T1[2] * Sg[kk][2];
            dT0[kk] = 2 * s0 * dL_da + s1 * dL_db;
            dT1[kk] = 2 * s1 * dL_dc + s0 * dL_db;
        }
        const float dJ00 = Vw[0] * dT0[0] + Vw[4] * dT0[1] + Vw[8] * dT0[2];
        const float dJ02 = Vw[2] * dT0[0] + Vw[6] * dT0[1] + Vw[10] * dT0[2];
        const float dJ11 = Vw[1] * dT1[0] + Vw[5] * dT1[1] + Vw[9] * dT1[2];
        const float dJ12 = Vw[2] * dT1[0] + Vw[6] * dT1[1] + Vw[10] * dT1[2];
        const float tz = __builtin_amdgcn_rcpf(Pc.t[2]), tz2 = tz * tz, tz3 = tz2 * tz;
        const float dtx = Pc.xmul * -fx * tz2 * dJ02;
        const float dty = Pc.ymul * -fy * tz2 * dJ12;
        const float dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2 * fx * Pc.t[0]) * tz3 * dJ02 +
                          (2 * fy * Pc.t[1]) * tz3 * dJ12;
        dmean[0] += Vw[0] * dtx + Vw[1] * dty + Vw[2] * dtz;
        dmean[1] += Vw[4] * dtx + Vw[5] * dty + Vw[6] * dtz;
        dmean[2] += Vw[8] * dtx + Vw[9] * dty + Vw[10] * dtz;
        // ---- perspective-divide backward
        float hom[4];
        hom[0] = Pm[0] * g[0] + Pm[4] * g[1] + Pm[8] * g[2] + Pm[12];
        hom[1] = Pm[1] * g[0] + Pm[5] * g[1] + Pm[9] * g[2] + Pm[13];
        hom[3] = Pm[3] * g[0] + Pm[7] * g[1] + Pm[11] * g[2] + Pm[15];
        const float m_w = __builtin_amdgcn_rcpf(hom[3] + 0.0000001f);
        const float mul1 = hom[0] * m_w * m_w;
        const float mul2 = hom[1] * m_w * m_w;
        dmean[0] += (Pm[0] * m_w - Pm[3] * mul1) * dm2x + (Pm[1] * m_w - Pm[3] * mul2) * dm2y;
        dmean[1] += (Pm[4] * m_w - Pm[7] * mul1) * dm2x + (Pm[5] * m_w - Pm[7] * mul2) * dm2y;
        dmean[2] += (Pm[8] * m_w - Pm[11] * mul1) * dm2x + (Pm[9] * m_w - Pm[11] * mul2) * dm2y;
        // ---- depth backward (exact row 2 of the view matrix)
        dmean[0] += Vw[2] * ddep;
        dmean[1] += Vw[6] * ddep;
        dmean[2] += Vw[10] * ddep;
    }
    {  // the scene's view-independent partials (opacity, colour), summed over its views by the backward's atomics
        if (det) {
            const long long *a = reinterpret_cast<const long long *>(accum) + ks;
            if (!aa) dop = (float)ldexp((double)a[0], -det_s);
#pragma unroll
            for (int q = 0; q < 3; q++) dcol[q] = (float)ldexp((double)a[1 + q], -det_s);
        } else {
            const float4 a = LDSV ? acc_s : *reinterpret_cast<const float4 *>(accum + ks);
            if (!aa) dop = a.x;
            dcol[0] = a.y; dcol[1] = a.z; dcol[2] = a.w;
        }
    }
    // ---- cov3D backward, once on the view-summed dL/dcov3D (linear, so equal to the per-view sum)
    const float dS[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                            {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                            {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
    float dM[3][3];  // dM[c][r] = 2 s_r sum_k R[k][r] dS[c][k]   (glm M = S*R, M[k][r] = s_r R[k][r])
#pragma unroll
    for (int cc = 0; cc < 3; cc++)
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
            dM[cc][rr] = 2.0f * s[rr] * (R[0][rr] * dS[cc][0] + R[1][rr] * dS[cc][1] + R[2][rr] * dS[cc][2]);
    float dscale[3], dd[3][3];
#pragma unroll
    for (int ii = 0; ii < 3; ii++) {
        dscale[ii] = (R[0][ii] * dM[0][ii] + R[1][ii] * dM[1][ii] + R[2][ii] * dM[2][ii]) * mod;
#pragma unroll
        for (int rr = 0; rr < 3; rr++) dd[ii][rr] = dM[rr][ii] * s[ii];  // dL_dMt[ii][rr] * s_ii
    }
    const float r_ = g[7], x = g[8], y = g[9], z = g[10];
    float dq[4];
    dq[0] = 2 * z * (dd[0][1] - dd[1][0]) + 2 * y * (dd[2][0] - dd[0][2]) + 2 * x * (dd[1][2] - dd[2][1]);
    dq[1] = 2 * y * (dd[1][0] + dd[0][1]) + 2 * z * (dd[2][0] + dd[0][2]) + 2 * r_ * (dd[1][2] - dd[2][1]) -
            4 * x * (dd[2][2] + dd[1][1]);
    dq[2] = 2 * x * (dd[1][0] + dd[0][1]) + 2 * r_ * (dd[2][0] - dd[0][2]) + 2 * z * (dd[1][2] + dd[2][1]) -
            4 * y * (dd[2][2] + dd[0][0]);
    dq[3] = 2 * r_ * (dd[0][1] - dd[1][0]) + 2 * x * (dd[2][0] + dd[0][2]) + 2 * y * (dd[1][2] + dd[2][1]) -
            4 * z * (dd[1][1] + dd[0][0]);
    float *o = d_gauss + ((size_t)b * d.N + i) * 14;
    const float out[14] = {dmean[0], dmean[1], dmean[2], dop, dscale[0], dscale[1], dscale[2],
                           dq[0], dq[1], dq[2], dq[3], dcol[0], dcol[1], dcol[2]};
    float2 *o2 = reinterpret_cast<float2 *>(o);
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int kk = 0; kk < 7; kk++)
        o2[kk] = det_bad ? make_float2(qnan, qnan) : make_float2(out[2 * kk], out[2 * kk + 1]);
    if (stamp) d.counters[cnt_tile(g_diag) + 3] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace

int launch_preproc_bwd(const Dims &d, const float *gaussians, const float *cam_view, const float *cam_view_proj,
                       float *d_gaussians, float *d_means2D, const Workspace &w, hipStream_t st) {
    auto pre = with_flags([](auto LDSV, auto AA) { return k_preproc_bwd<LDSV.value, AA.value>; }, d.V <= PRE_MAXV,
                          (d.options & LGM_RENDER_ANTIALIAS) != 0);
    dim3 grid((d.N + 255) / 256, d.B);
    LGM_LAUNCH("k_preproc_bwd", st, (pre<<<grid, 256, 0, st>>>(d, gaussians, cam_view, cam_view_proj, w.rects, w.accum,
                                                               d_gaussians, d_means2D, w.gP, w.gQ, w.detmax,
                                                               w.det_sat)));
    return LGM_OK;
}

}  // namespace lgm
