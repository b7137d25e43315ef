// lgm_amd/csrc/render_common.h -- shared constants, the typed view of the workspace and device math of the render
// path. (Where the workspace's bytes live: render_layout.h.)
//
// Numerics restate SURVEY.md §2.3 (the upstream algorithm behind core/gs.py:58-85; CPU restatement in
// oracle/raster_oracle.c): 0.3 dilation, 1.3 tanfov clamp inside J, depth cull 0.2, radius = ceil(3 sqrt(lmax))
// with max(0.1, mid^2 - det), ndc2Pix in double, integer tile-rect math, alpha cap 0.99 / floor 1/255,
// transmittance floor 1e-4 tested before accumulation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "lgm_render.h"
#include "render_layout.h"
#include "work_split.h"

namespace lgm {

constexpr int LDS_HIST_MAX = 8192;                   // tiles per view for the LDS-histogram binning path
constexpr float LOG2E = 1.4426950408889634f;

// Float mode's gradient accumulators: fp32, and fp64 for the conic partials of needle-like records. A needle's conic
// partials from different tiles and views largely cancel and the cov2D inverse amplifies what is left (conditions
// 1e3-2e4), so fp32 atomic sums made its scale / rotation gradients a draw of the atomic order (single runs up to ~3x
// the fp32 oracle's error vs fp64 at 512^2, profiles/r03/diag_float_spread); fp64 sums of the same fp32 partials are
// order-independent to ~2^-50 of the partials (the deterministic mode's int64 sums are exact). Measured: all
// accumulators fp64 +37 us per pool step, the needle side accumulators +24 us (profiles/r03/ab_acc_side).
constexpr float ACC_NEEDLE = 300.0f;  // conic condition above which a record's conic partials are summed in fp64

struct Dims {
    int B, V, N, H, W, gx, gy, T, BV;
    float tanx, tany, fx, fy, mod;
    unsigned long long *counters;  // this call's device work counters (lgm_diag.render_counters), or null
    int det_lim_log2;              // lgm_diag.det_limit_log2 (test hook; 0 = the derived bound)
    int options;                   // per-call LGM_RENDER_* bits (NO_CULL, CLAMP_IMAGE, FUSED_LOSS, DETERMINISTIC,
                                   // ANTIALIAS, the SH degree)
    int ck_shift;                  // backward work items span 2^ck_shift forward chunks (ck_shift_for(BV * T))
    // LGM_RENDER_FUSED_LOSS (core/models.py:138-160): ground truth [BV,3,P] / [BV,P], the per-tile loss partials
    // (forward) and the gradients of the two MSE terms (backward)
    const float *gt_img, *gt_mask;
    float *loss_part;  // workspace: per-tile (image, alpha) sums of squared residuals
    float *loss_out;   // DEVICE float[4]: loss_mse, mse_image, mse_alpha, psnr
    const float *d_loss;  // DEVICE float[2]: dL/dmse_image, dL/dmse_alpha
    // LGM_RENDER_ANTIALIAS: the workspace's opacity factors s [BV, N] (Workspace::aa_s; k_aa_factor writes them ahead
    // of the binning), else null
    const float *aa_s;
    // LGM_RENDER_SH_MASK: the workspace's per-view colours [BV, N, 3] (AccumLayout::sh_col) and colour partials
    // [BV, N, 3] (AccumLayout::sh_part; fp32 or int64), else null
    const float *sh_col;
    void *sh_part;
};

// The workspace as typed pointers, built once per call: the one place that casts into it. (The kernels take the
// pointers one by one: a struct argument would change their kernarg layout and drop the __restrict__ information.)
struct Workspace {
    char *base;
    float4 *gP, *gQ;
    uint2 *rects;
    int *tile_count, *tile_start, *order;
    unsigned long long *pairs;
    float *final_T;
    int *n_contrib, *wlast;
    float4 *cfin;
    float *ck;
    int2 *cklist;
    int *nck;
    unsigned char *cmask;
    float *accum;      // the accumulator block (AccumLayout) as fp32 elements; the kernels recast it per region
    float4 *accum16;   // the same block as the 16-B units k_render_fwd's epilogue zeroes (AccumLayout::fwd_zero)
    float2 *lossp;
    double2 *lossw;
    unsigned *detmax;
    unsigned long long *pair_counts;                  // misc: MISC_PAIRS
    unsigned *ck_counters, *loss_arrival, *det_sat;  // misc: MISC_CK_REGION, MISC_LOSS_ARRIVAL, MISC_DET_SAT
    float *aa_s;  // LGM_RENDER_ANTIALIAS: the factors (AccumLayout::aa_s), else null
    // LGM_RENDER_SH_MASK: AccumLayout::sh_col, sh_part, sh_mask, sh_g14, sh_dg14, else null
    float *sh_col, *sh_g14, *sh_dg14;
    void *sh_part;
    unsigned char *sh_mask;
    Workspace(char *ws, const Layout &L) : base(ws) {
        auto at = [ws](auto *&p, size_t off) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(ws + off); };
        at(gP, L.gP); at(gQ, L.gQ); at(rects, L.rects);
        at(tile_count, L.tile_count); at(tile_start, L.tile_start); at(order, L.order); at(pairs, L.pairs);
        at(final_T, L.final_T); at(n_contrib, L.n_contrib); at(wlast, L.wlast); at(cfin, L.cfin);
        at(ck, L.ck); at(cklist, L.cklist); at(nck, L.nck); at(cmask, L.cmask);
        at(accum, L.accum); at(accum16, L.accum);
        at(lossp, L.lossp); at(lossw, L.lossw); at(detmax, L.detmax);
        at(pair_counts, L.misc + MISC_PAIRS * 8); at(ck_counters, L.misc + MISC_CK_REGION * 4);
        at(loss_arrival, L.misc + MISC_LOSS_ARRIVAL * 4); at(det_sat, L.misc + MISC_DET_SAT * 4);
        aa_s = nullptr;
        if (L.acc.aa_s.bytes) at(aa_s, L.accum + L.acc.aa_s.off);
        sh_col = sh_g14 = sh_dg14 = nullptr;
        sh_part = nullptr;
        sh_mask = nullptr;
        if (L.acc.sh_g14.bytes) {
            at(sh_part, L.accum + L.acc.sh_part.off); at(sh_col, L.accum + L.acc.sh_col.off);
            at(sh_mask, L.accum + L.acc.sh_mask.off); at(sh_g14, L.accum + L.acc.sh_g14.off);
            at(sh_dg14, L.accum + L.acc.sh_dg14.off);
        }
    }
    char *range(const Region &r) const { return base + r.off; }  // a range of the workspace (Layout::bin_clear)
    char *accum_range(const Region &r) const { return reinterpret_cast<char *>(accum) + r.off; }  // of AccumLayout
};

// ------------------------------------------------------------------------------------------------------------
// Camera helpers: the 4x4 matrices are the row-major torch tensors of core/gs.py:54-55 read column-major.
//
// Every helper of the forward preprocess runs with FP contraction OFF and in the oracle's operation order
// (oracle/raster_oracle.c: glm-order matrix products, left-to-right sums): the integer results derived from it
// -- radii, tile rects, (Gaussian, tile) pair counts and the depth sort keys -- are then bit-identical to the
// restatement (tests/test_render_parity_gpu.py), not merely close.
__device__ __forceinline__ void xf43(const float *M, float x, float y, float z, float o[3]) {
#pragma clang fp contract(off)
    o[0] = M[0] * x + M[4] * y + M[8] * z + M[12];
    o[1] = M[1] * x + M[5] * y + M[9] * z + M[13];
    o[2] = M[2] * x + M[6] * y + M[10] * z + M[14];
}
__device__ __forceinline__ void xf44(const float *M, float x, float y, float z, float o[4]) {
#pragma clang fp contract(off)
    o[0] = M[0] * x + M[4] * y + M[8] * z + M[12];
    o[1] = M[1] * x + M[5] * y + M[9] * z + M[13];
    o[2] = M[2] * x + M[6] * y + M[10] * z + M[14];
    o[3] = M[3] * x + M[7] * y + M[11] * z + M[15];
}

// glm-convention rotation matrix R[col][row] from the un-normalised quaternion (r,x,y,z) (upstream semantics).
__device__ __forceinline__ void quat_rot(const float q[4], float R[3][3]) {
#pragma clang fp contract(off)
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z); R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y); R[2][1] = 2.f * (y * z + r * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// Sigma = M^T M with M = S*R (glm): M[c][k] = s_k R[c][k], Sigma[c][r] = sum_k M[r][k] M[c][k] (the oracle's
// m3_mul order); stored (00,01,02,11,12,22).
__device__ __forceinline__ void cov3d(const float s[3], const float R[3][3], float c3[6]) {
#pragma clang fp contract(off)
    float M[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) M[c][k] = s[k] * R[c][k];
#define LGM_SIG(c, r) (M[r][0] * M[c][0] + M[r][1] * M[c][1] + M[r][2] * M[c][2])
    c3[0] = LGM_SIG(0, 0); c3[1] = LGM_SIG(0, 1); c3[2] = LGM_SIG(0, 2);
    c3[3] = LGM_SIG(1, 1); c3[4] = LGM_SIG(1, 2); c3[5] = LGM_SIG(2, 2);
#undef LGM_SIG
}

// The two non-zero glm columns of T = W*J (with the 1.3 tanfov clamp on t), SURVEY §2.3 row 1.
struct ProjCtx {
    float T0[3], T1[3];  // glm T[0][*], T[1][*]
    float t[3];          // clamped view-space mean
    float xmul, ymul;    // 0 where the clamp was active (gradient cut, as upstream)
};
__device__ __forceinline__ ProjCtx make_proj(const float *Vw, float mx, float my, float mz, float fx, float fy,
                                             float tanx, float tany) {
#pragma clang fp contract(off)
    ProjCtx P;
    xf43(Vw, mx, my, mz, P.t);
    const float limx = 1.3f * tanx, limy = 1.3f * tany;
    const float txtz = P.t[0] / P.t[2], tytz = P.t[1] / P.t[2];
    P.t[0] = fminf(limx, fmaxf(-limx, txtz)) * P.t[2];
    P.t[1] = fminf(limy, fmaxf(-limy, tytz)) * P.t[2];
    P.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    P.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    const float tz = P.t[2];
    const float J00 = fx / tz, J02 = -(fx * P.t[0]) / (tz * tz);
    const float J11 = fy / tz, J12 = -(fy * P.t[1]) / (tz * tz);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        P.T0[r] = Vw[4 * r + 0] * J00 + Vw[4 * r + 2] * J02;
        P.T1[r] = Vw[4 * r + 1] * J11 + Vw[4 * r + 2] * J12;
    }
    return P;
}
// cov = T^T Sigma^T T (glm order, as the oracle's cov2d): with s0 = Sigma T0 and s1 = Sigma T1 (T0, T1 the
// non-zero columns of T), a = T0 . s0, b = T0 . s1, c = T1 . s1, each summed left to right.
__device__ __forceinline__ void cov2d(const ProjCtx &P, const float c3[6], float &a, float &b, float &c) {
#pragma clang fp contract(off)
    const float S[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float s0[3], s1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s0[k] = S[k][0] * P.T0[0] + S[k][1] * P.T0[1] + S[k][2] * P.T0[2];
        s1[k] = S[k][0] * P.T1[0] + S[k][1] * P.T1[1] + S[k][2] * P.T1[2];
    }
    a = P.T0[0] * s0[0] + P.T0[1] * s0[1] + P.T0[2] * s0[2] + 0.3f;
    b = s1[0] * P.T0[0] + s1[1] * P.T0[1] + s1[2] * P.T0[2];
    c = P.T1[0] * s1[0] + P.T1[1] * s1[1] + P.T1[2] * s1[2] + 0.3f;
}
constexpr float AA_RMIN = 2.5e-5f;  // LGM_RENDER_ANTIALIAS: the floor of det0 / det (lgm_render.h)

__device__ __forceinline__ float ndc2pix(float v, int S) { return (float)((((double)v + 1.0) * S - 1.0) * 0.5); }

// Can any integer pixel of [rx0, rx1] x [ry0, ry1] reach q = A dx^2 + 2B dx dy + C dy^2 <= tau around (x, y)?
// Exact minimum of the (convex) quadratic over the rectangle: 0 if the centre is inside, else the minimum over the
// four edges (1-D minimiser clamped to the edge). Conservative for the integer pixels it contains.
// invA = 1/A, invC = 1/C (precomputed once per Gaussian).
__device__ __forceinline__ bool ellipse_hits_rect(float x, float y, float A, float B, float C, float invA,
                                                  float invC, float tau, float rx0, float rx1, float ry0, float ry1) {
    if (tau >= 3.0e38f) return true;
    if (x >= rx0 && x <= rx1 && y >= ry0 && y <= ry1) return true;
    float best = 3.0e38f;
    const float ex[2] = {rx0, rx1}, ey[2] = {ry0, ry1};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const float dx = x - ex[e];
        const float dy = fminf(fmaxf(-B * dx * invC, y - ry1), y - ry0);
        best = fminf(best, A * dx * dx + 2.f * B * dx * dy + C * dy * dy);
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const float dy = y - ey[e];
        const float dx = fminf(fmaxf(-B * dy * invA, x - rx1), x - rx0);
        best = fminf(best, A * dx * dx + 2.f * B * dx * dy + C * dy * dy);
    }
    return best <= tau;
}

// Compositing records (k_bin -> k_render_fwd / k_render_bwd), two float4 per (view, Gaussian):
//   P = (x, y, A', B'),  Q = (C', L, tau', depth)
// with the conic pre-scaled so that one (entry, pixel) evaluation is 5 VALU + exp2:
//   power * log2(e) + log2(opacity) = A' dx^2 + B' dx dy + C' dy^2 + L,   alpha = min(0.99, exp2(that)),
//   A' = -KQ A, B' = -2 KQ B, C' = -KQ C (KQ = log2(e) / 2), L = log2(opacity) (-inf for opacity <= 0).
// Upstream's `power > 0` skip is `that > L`; dL/dG = opacity dL/dalpha uses exp2(that) = opacity G directly.
// The culling threshold tau (on q = A dx^2 + 2B dx dy + C dy^2) is stored as tau' = KQ tau, so the quadrant tests
// run ellipse_hits_rect on (-A', -B'/2, -C', tau') = KQ (A, B, C, tau): the same test scaled by a positive constant
// (within tau's inflation). tau >= 3e38 (never cull) is kept as is.
constexpr float KQ = 0.5f * LOG2E;
__device__ __forceinline__ float4 rec_p(float x, float y, float A, float B) {
    return make_float4(x, y, -KQ * A, -LOG2E * B);
}
__device__ __forceinline__ float4 rec_q(float C, float opacity, float tau, float depth) {
    return make_float4(-KQ * C, opacity > 0.f ? log2f(opacity) : -INFINITY, tau >= 3.0e38f ? tau : KQ * tau, depth);
}
// Needle-like record (see AccumLayout::needle): on the stored pre-scaled conic A', B', C' (the condition is
// scale-invariant: (A' + C')^2 / (A'C' - B'^2 / 4) = (A + C)^2 / (AC - B^2)).
// FP contraction OFF: k_bin evaluates it on the record still in registers (right after the multiplications that
// form A', B', C'), k_render_bwd on the record loaded back from memory; with contraction a fused multiply-add could
// round differently in one of them and flip the decision for a record at the threshold. Evaluated as
// separately rounded IEEE operations it is a pure function of the stored bits in both (tests/test_render_gpu.py
// test_needle_flag_is_a_function_of_the_stored_record).
__device__ __forceinline__ bool rec_needle(float Ap, float Bp, float Cp) {
#pragma clang fp contract(off)
    const float sac = Ap + Cp, dq = Ap * Cp - 0.25f * Bp * Bp;
    return !(sac * sac <= ACC_NEEDLE * dq);  // (dq <= 0 or NaN: flagged)
}
// the upstream conic and opacity back from a record (the backward's per-entry gradient conversion)
__device__ __forceinline__ void rec_conic(const float4 &p, const float4 &q, float &A, float &B, float &C, float &op) {
    A = p.z * (-1.0f / KQ);
    B = p.w * (-1.0f / LOG2E);
    C = q.x * (-1.0f / KQ);
    op = exp2f(q.y);
}

struct Geo {
    float x, y, depth, A, B, C, opacity;  // pixel centre, view depth, conic (A, B, C), opacity
    float hx, hy;                         // half-extents of the alpha >= 1/255 ellipse's bounding box (pixels)
    float tau;                            // inflated alpha >= 1/255 threshold on q (3e38: never cull)
    int x0, y0, x1, y1;                   // reference tile rect (3-sigma)
    int cx0, cy0, cx1, cy1;               // emitted tile rect: reference rect ∩ tiles the alpha ellipse can reach
    int radius;
};

// Per-Gaussian forward preprocess. Returns false if culled (radius 0 upstream).
//
// Exact opacity-aware tile culling: upstream keeps every tile of the 3-sigma rect, but a tile in which
// alpha = min(0.99, o exp(-q/2)) < 1/255 for every pixel is skipped by every pixel (`continue`), changing
// nothing but the internal contributor counter. alpha >= 1/255 <=> q <= tau = 2 ln(255 o); the ellipse
// {q <= tau} lies inside |dx| <= sqrt(tau a), |dy| <= sqrt(tau c) (a, c: the dilated 2D covariance), which
// bounds the candidate tiles; the emitter then keeps a tile only if ellipse_hits_rect() says some pixel of it
// can reach q <= tau. tau is inflated (below) so fp32 rounding of q can never re-admit a culled pixel.
//
// In two parts: gaussian_cov3d is the part no view enters (Sigma from the scales and the quaternion), computed once
// per Gaussian; preprocess_view takes g[0..3] (mean, opacity) and Sigma for one view. Together they are the same
// operations on the same operands in the same order as the one-piece form.
__device__ __forceinline__ void gaussian_cov3d(const float *g, float mod, float c3[6]) {
#pragma clang fp contract(off)
    float R[3][3];
    const float q[4] = {g[7], g[8], g[9], g[10]};
    quat_rot(q, R);
    const float s[3] = {mod * g[4], mod * g[5], mod * g[6]};
    cov3d(s, R, c3);
}
__device__ __forceinline__ bool preprocess_view(const float *g, const float c3[6], const float *Vw, const float *Pm,
                                                const Dims &d, Geo &o, const float *aa_row, int i) {
#pragma clang fp contract(off)
    float hom[4], pv[3];
    xf44(Pm, g[0], g[1], g[2], hom);
    const float pw = 1.0f / (hom[3] + 0.0000001f);
    const float ppx = hom[0] * pw, ppy = hom[1] * pw;
    xf43(Vw, g[0], g[1], g[2], pv);
    if (pv[2] <= 0.2f) return false;
    const ProjCtx P = make_proj(Vw, g[0], g[1], g[2], d.fx, d.fy, d.tanx, d.tany);
    float a, b, c;
    cov2d(P, c3, a, b, c);
    const float det = a * c - b * b;
    if (det == 0.0f) return false;
    const float det_inv = 1.f / det;
    const float mid = 0.5f * (a + c);
    const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
    const float rad = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
    const float px = ndc2pix(ppx, d.W), py = ndc2pix(ppy, d.H);
    const int r = (int)rad;
    const int x0 = min(d.gx, max(0, (int)((px - r) / BX)));
    const int y0 = min(d.gy, max(0, (int)((py - r) / BY)));
    const int x1 = min(d.gx, max(0, (int)((px + r + BX - 1) / BX)));
    const int y1 = min(d.gy, max(0, (int)((py + r + BY - 1) / BY)));
    if ((x1 - x0) * (y1 - y0) == 0) return false;
    o.x = px; o.y = py; o.depth = pv[2];
    o.A = c * det_inv; o.B = -b * det_inv; o.C = a * det_inv;
    // the opacity every later step consumes: o, or o^ = o s with LGM_RENDER_ANTIALIAS (a runtime branch: k_bin's
    // instantiations and their register budget stay as they are). s of Gaussian i in this view (aa_row: the view's
    // row of Dims::aa_s) was written by k_aa_factor: det0 = a0 c0 - b^2 cancels for an elongated splat -- a0 c0 / det0
    // reaches hundreds -- and in fp32 that amplification of the operands' rounding is in log2 o^ (1e-5..1e-4)
    float op = g[3];
    if (d.options & LGM_RENDER_ANTIALIAS) {
        // (the index tied to the rect just computed: a load hoisted to the top of the preprocess would hold a register
        // across it, and k_bin has none to spare)
        int ii = i;
        asm volatile("" : "+v"(ii) : "v"(y1));
        op *= aa_row[ii];
    }
    o.opacity = op;
    o.x0 = x0; o.y0 = y0; o.x1 = x1; o.y1 = y1; o.radius = r;
    // --- exact opacity-aware cull of the emitted rect
    if (d.options & LGM_RENDER_NO_CULL) {
        o.hx = o.hy = 3.0e38f;
        o.tau = 3.0e38f;
        o.cx0 = x0; o.cx1 = x1; o.cy0 = y0; o.cy1 = y1;
        return true;
    }
    if (!(op * 255.0f > 1.0f)) {  // o <= 1/255: alpha < 1/255 everywhere (and NaN-safe)
        o.hx = o.hy = -1.f;
        o.tau = -1.f;
        o.cx0 = o.cx1 = x0; o.cy0 = o.cy1 = y0;
        return true;
    }
    // fp32 evaluation of q = A dx^2 + 2B dx dy + C dy^2 loses ~eps * kappa relative accuracy on elongated
    // ellipses; cond = (a + c)^2 / det ~ kappa. Inflate tau by 1e-3 + 2e-5 * cond (>= 80x the rounding bound) and
    // do not cull ill-conditioned or non-positive-definite ones at all (keep upstream's full rect).
    const float cond = (a + c) * (a + c) * __builtin_amdgcn_rcpf(det);  // (a threshold: 1 ulp is immaterial)
    if (!(det > 0.f) || !(cond < 4e4f)) {
        o.hx = o.hy = 3.0e38f;
        o.tau = 3.0e38f;
        o.cx0 = x0; o.cx1 = x1; o.cy0 = y0; o.cy1 = y1;
        return true;
    }
    // 2 ln(255 o) by v_log_f32 (log2, ~1 ulp): the 1e-3 inflation dwarfs it
    const float tau = (2.0f * 0.6931471805599453f) * __builtin_amdgcn_logf(255.0f * op) * (1.001f + 2e-5f * cond) + 1e-3f;
    o.tau = tau;
    o.hx = sqrtf(tau * fmaxf(a, 0.f));
    o.hy = sqrtf(tau * fmaxf(c, 0.f));
    const float lx = fmaxf(-1.0f, fminf((float)d.gx, (px - o.hx - (BX - 1)) / BX));
    const float hxt = fmaxf(-1.0f, fminf((float)d.gx, (px + o.hx) / BX));
    const float ly = fmaxf(-1.0f, fminf((float)d.gy, (py - o.hy - (BY - 1)) / BY));
    const float hyt = fmaxf(-1.0f, fminf((float)d.gy, (py + o.hy) / BY));
    o.cx0 = max(x0, (int)ceilf(lx));
    o.cx1 = min(x1, (int)floorf(hxt) + 1);
    o.cy0 = max(y0, (int)ceilf(ly));
    o.cy1 = min(y1, (int)floorf(hyt) + 1);
    if (o.cx1 < o.cx0) o.cx1 = o.cx0;
    if (o.cy1 < o.cy0) o.cy1 = o.cy0;
    return true;
}

__device__ __forceinline__ void load_gaussian(const float *__restrict__ src, float g[14]) {
    // rows are 56 B, always 8-B aligned: 7 x dwordx2
    const float2 *p = reinterpret_cast<const float2 *>(src);
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const float2 v = p[k];
        g[2 * k] = v.x;
        g[2 * k + 1] = v.y;
    }
}

// ---- Deterministic mode (LGM_RENDER_DETERMINISTIC): int64 fixed-point accumulators with scales that follow the
// data, so neither tiny nor huge gradients lose their meaning.
//  * a per-call scale 2^s with s = DET_BITS - exponent(max |dL/dpixel| over every seed): the accumulators' unit is
//    2^-DET_BITS of the largest per-pixel seed, whatever the loss normalisation (LGM's mean-MSE gives dL/dpixel
//    ~1e-9 at 8 x 8 views of 512^2: a fixed 2^-32 unit would leave its partials only tens of units);
//  * per (view, Gaussian) power-of-two normalisers of the view-dependent partials, from the compositing record (so
//    k_render_bwd and k_preproc_bwd derive bitwise the same exponents): dL/dmean2D by (W/2) sqrt(A) (resp. (H/2)
//    sqrt(C)) and dL/dconic by 1 / Sigma_xx, 1 / sqrt(Sigma_xx Sigma_yy), 1 / Sigma_yy (Sigma = conic^-1): with
//    alpha >= 1/255 only where q <= 2 ln 255, each normalised per-pixel term is bounded by a small constant times
//    |dL/dG|, so a large, elongated Gaussian's conic partials (pixel offsets of hundreds) cannot overflow int64 and a
//    small one's keep their resolution.
// Every power-of-two scaling is exact, so the only rounding is each flush's conversion to an integer (nearest).
// (k_render_bwd encodes with these, k_preproc_bwd and the SH backward decode.)
constexpr int DET_BITS = 30;  // seed max -> 2^30 units: per flush |value| <= ~2^51, sums of 2^11 flushes < 2^63
__device__ __forceinline__ int f32_exp(float x) { return (int)((__float_as_uint(x) >> 23) & 0xffu) - 127; }
constexpr int DET_SLOTS = 64;  // k_det_seed_max spreads its atomics over this many words (same-address atomics serialise)
__device__ __forceinline__ int det_seed_shift(const unsigned *det_max) {  // s: the call's global scale exponent
    const uint4 *p = reinterpret_cast<const uint4 *>(det_max);
    unsigned mb = 0u;
#pragma unroll
    for (int i = 0; i < DET_SLOTS / 4; i++) {
        const uint4 v = p[i];
        mb = max(max(mb, max(v.x, v.y)), max(v.z, v.w));
    }
    const float m = __uint_as_float(mb);
    return (m > 0.f && m < 3.0e38f) ? DET_BITS - f32_exp(m) : 0;
}

struct DetNorm {
    int k[6];  // exponents of the view record's slots: mean2D x, y, conic A, B, C, depth
};
__device__ __forceinline__ DetNorm det_norm(float Ap, float Bp, float Cp, int W, int H) {
#pragma clang fp contract(off)
    DetNorm n;
    const float detp = Ap * Cp - 0.25f * (Bp * Bp);  // KQ^2 det(conic): the record holds -KQ A, -2 KQ B, -KQ C
    if (!(detp > 0.f) || !(detp < 3.0e38f) || !(Ap < 0.f) || !(Cp < 0.f)) {
        for (int q = 0; q < 6; q++) n.k[q] = 0;
        return n;
    }
    const int ea = f32_exp(-Ap), ec = f32_exp(-Cp), ed = f32_exp(detp);
    auto cl = [](int x) { return min(60, max(-60, x)); };
    n.k[0] = cl(-(f32_exp(0.5f * (float)W) + (ea >> 1)));
    n.k[1] = cl(-(f32_exp(0.5f * (float)H) + (ec >> 1)));
    n.k[2] = cl(ed - ec);              // 1 / Sigma_xx ~ det / C
    n.k[3] = cl(ed - ((ea + ec) >> 1));  // 1 / sqrt(Sigma_xx Sigma_yy)
    n.k[4] = cl(ed - ea);              // 1 / Sigma_yy ~ det / A
    n.k[5] = 0;
    return n;
}
// LGM_RENDER_ANTIALIAS's per-view opacity partial dL/do^ = (sum_p w) / o^: normalised by o^'s own power of two, from
// the record's L = log2(o^) (<= 0; so k_render_bwd and k_preproc_bwd derive bitwise the same exponent): the
// normalised flush is the plain pixel sum of w = G dL/dG, bounded like the other per-view partials, however small
// the compensated opacity of a sub-pixel splat is.
__device__ __forceinline__ int det_norm_opacity(float L) { return (int)fminf(0.f, fmaxf(-60.f, floorf(L))); }

// Tile bucket of one (view, tile): base offset into `pairs` and entry count.
// slot_stride < 0 selects packed mode; slot mode uses stride N (possibly 0: then every bucket is empty).
__device__ __forceinline__ void tile_range(int tile, long long slot_stride, const int *__restrict__ tile_start,
                                           const int *__restrict__ tile_count, long long &base, int &n) {
    if (slot_stride >= 0) {
        base = (long long)tile * slot_stride;
        n = tile_count[tile];
    } else {
        base = tile_start[tile];
        n = tile_start[tile + 1] - tile_start[tile];
    }
}

// (The XCD-grouped order of the (view, tile) items in the sort and both compositing kernels, xcd_item / xcd_group:
// work_split.h.)
__host__ __device__ __forceinline__ int round8(int x) { return (x + 7) & ~7; }

// Pixel of thread t inside a 16x16 tile: wavefront w owns the 8x8 quadrant (w & 1, w >> 1).
__device__ __forceinline__ void tile_pixel(int t, int &lx, int &ly) {
    const int w = t >> 6, l = t & 63;
    lx = ((w & 1) << 3) + (l & 7);
    ly = ((w >> 1) << 3) + (l >> 3);
}

// Runtime flags as compile-time ones, for a launcher that picks a kernel instantiation: with_flags(f, a, b, ...) calls
// f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...), a generic lambda that returns the kernel's address.
template <class F>
auto with_flags(F f) { return f(); }
template <class F, class... Rest>
auto with_flags(F f, bool flag, Rest... rest) {
    auto bind = [&](auto tag) { return with_flags([&](auto... tags) { return f(tag, tags...); }, rest...); };
    return flag ? bind(std::true_type{}) : bind(std::false_type{});
}

// ---- host launchers (render_bin.hip, render_fwd.hip, render_bwd.hip, render_preproc_bwd.hip)
int launch_binning(const Dims &d, const float *gaussians, const float *cam_view, const float *cam_view_proj,
                   const Workspace &w, const Layout &L, int *radii_out, long long *stats_out, bool count_only,
                   hipStream_t st);
int launch_render_fwd(const Dims &d, const float *gaussians, const float *bg, float *image, float *depth,
                      float *alpha, const Workspace &w, const Layout &L, hipStream_t st);
// the fused loss's final reduction (after launch_render_fwd with LGM_RENDER_FUSED_LOSS): d.loss_out receives
// (loss_mse, mse_image, mse_alpha, psnr)
int launch_loss_reduce(const Dims &d, const Workspace &w, hipStream_t st);
int launch_render_bwd(const Dims &d, const float *gaussians, const float *cam_view, const float *cam_view_proj,
                      const float *bg, const float *d_image, const float *d_depth, const float *d_alpha,
                      float *d_gaussians, float *d_means2D, const Workspace &w, const Layout &L, hipStream_t st);
// the per-Gaussian projection backward over the accumulators k_render_bwd filled (launch_render_bwd ends with it)
int launch_preproc_bwd(const Dims &d, const float *gaussians, const float *cam_view, const float *cam_view_proj,
                       float *d_gaussians, float *d_means2D, const Workspace &w, hipStream_t st);
// LGM_RENDER_SH_MASK (render_sh.hip): `wide` / `d_wide` are the caller's [B,N,11+3K] rows. launch_sh_pack runs ahead
// of the binning (the 14-wide copy, the colour partials' zeroing), launch_sh_colour between the binning and
// launch_render_fwd, launch_sh_bwd after launch_render_bwd.
int launch_sh_pack(const Dims &d, int degree, const float *wide, const Workspace &w, const Layout &L, hipStream_t st);
int launch_sh_colour(const Dims &d, int degree, const float *wide, const float *cam_view, const Workspace &w,
                     hipStream_t st);
int launch_sh_bwd(const Dims &d, int degree, const float *wide, const float *cam_view, float *d_wide,
                  const Workspace &w, hipStream_t st);

}  // namespace lgm
