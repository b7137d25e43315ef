// lgm_amd/csrc/meshraster.hip -- the triangle-mesh rasteriser of include/lgm_meshraster.h: a mesh of lgm_mesh.h drawn
// from the Gaussian renderer's cameras, and the gradient of the image to its texture or vertex colours.
//
//   k_mr_project   per (view, vertex): pixel position, w and view depth into the workspace (w = 0: cut)
//   k_mr_vis       per (view, face): a box of at most LGM_MESHRASTER_SMALL_BOX pixels is walked by the thread itself
//                  (the workload: a 256^3 surface-nets mesh at 512^2 has triangles about a pixel across); a larger one is
//                  appended to a list (one integer atomic; the list's order does not matter)
//   k_mr_vis_big   one workgroup per listed face at a time, its 256 threads striding over the box together
//   k_mr_shade     per pixel: the winning face's beta recomputed, texture fetch or colour interpolation, all outputs
//   k_mr_absmax    backward: the largest |d_image| (bits through an integer atomicMax)
//   k_mr_scatter   backward, per covered pixel: d_image times its weights into int64 fixed-point accumulators
//   k_mr_convert   backward: accumulators to fp32
//
// Integer atomics only (64-bit min for visibility, 64-bit add for the gradient): two calls are bitwise equal.
#include "lgm_meshraster.h"
#include "render_common.h"

namespace lgm {
namespace {

constexpr int THREADS = 256;
constexpr int BIG_GRID = 2048;  // workgroups of k_mr_vis_big (a grid-stride loop over the list)
constexpr long long I31 = 2147483648LL;
constexpr unsigned long long NO_HIT = ~0ull;

struct MrLayout {
    size_t proj, vis, head, queue, acc, total;  // head: u32 [0] the list's length, u32 [1] the bits of amax
};

MrLayout mr_layout(int V, long long Nv, long long Nf, int H, int W, int Ht, int Wt) {
    MrLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes); return r; };
    L.proj = take((size_t)V * Nv * 16);  // (X, Y, w, z) per (view, vertex)
    L.vis = take((size_t)V * H * W * 8);  // depth bits << 32 | face per pixel (forward -> backward)
    L.head = take(16);
    L.queue = take((size_t)V * Nf * 4);  // (view, face) items of k_mr_vis_big
    L.acc = take(std::max((size_t)Nv, (size_t)Ht * Wt) * 3 * 8);  // the backward's int64 sums
    L.total = o;
    return L;
}

bool mr_sizes_ok(int V, long long Nv, long long Nf, int H, int W) {
    return V >= 1 && H >= 1 && W >= 1 && Nv >= 0 && Nf >= 0 && 3 * Nv < I31 && 3 * Nf < I31 &&
           3LL * V * H < I31 && 3LL * V * H * W < I31 && V * Nv < I31 && V * Nf < I31;
}

int unit_log2(int V, int H, int W) {
    const long long p = (long long)V * H * W;
    int c = 0;
    while ((1ll << c) < p) c++;  // ceil(log2 p)
    return 61 - c;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028235e38f; }  // (false for NaN)

// The face's three projected vertices in view v, or false if the face is dropped there (an index out of range, in
// texture mode (face_uvs given) a face_uvs entry out of range, a cut vertex).
__device__ __forceinline__ bool mr_face(const int *__restrict__ faces, const int *__restrict__ face_uvs, long long Nu,
                                        const float4 *__restrict__ proj, long long Nv, int v, int f, float4 p[3]) {
    if (face_uvs)
        for (int k = 0; k < 3; k++)
            if ((unsigned)face_uvs[3 * (size_t)f + k] >= (unsigned long long)Nu) return false;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned long long)Nv || (unsigned)i1 >= (unsigned long long)Nv ||
        (unsigned)i2 >= (unsigned long long)Nv)
        return false;
    const float4 *pv = proj + (size_t)v * Nv;
    p[0] = pv[i0], p[1] = pv[i1], p[2] = pv[i2];
    return p[0].z > 0.2f && p[1].z > 0.2f && p[2].z > 0.2f;
}

// The face's pixel box [xa, xb] x [ya, yb], clipped to the image (empty: xa > xb or ya > yb). X and Y are finite.
__device__ __forceinline__ void mr_box(const float4 p[3], int H, int W, int &xa, int &xb, int &ya, int &yb) {
    const float x0 = fminf(fminf(p[0].x, p[1].x), p[2].x), x1 = fmaxf(fmaxf(p[0].x, p[1].x), p[2].x);
    const float y0 = fminf(fminf(p[0].y, p[1].y), p[2].y), y1 = fmaxf(fmaxf(p[0].y, p[1].y), p[2].y);
    xa = (int)fminf(fmaxf(ceilf(x0), 0.f), (float)W);
    xb = (int)fmaxf(fminf(floorf(x1), (float)(W - 1)), -1.f);
    ya = (int)fminf(fmaxf(ceilf(y0), 0.f), (float)H);
    yb = (int)fmaxf(fminf(floorf(y1), (float)(H - 1)), -1.f);
}

// Coverage, beta and depth of the header at the pixel centre (px, py). One function for both visibility paths, the
// shading and the backward, with contraction off: a pure function of its operands' bits wherever it is inlined.
__device__ __forceinline__ bool mr_hit(const float4 p[3], float px, float py, float beta[3], float &depth) {
#pragma clang fp contract(off)
    const float x0 = p[0].x - px, y0 = p[0].y - py, x1 = p[1].x - px, y1 = p[1].y - py, x2 = p[2].x - px,
                y2 = p[2].y - py;
    const float e0 = x1 * y2 - x2 * y1, e1 = x2 * y0 - x0 * y2, e2 = x0 * y1 - x1 * y0;
    const float A = (e0 + e1) + e2;
    if (A == 0.f) return false;
    const float b0 = e0 / A, b1 = e1 / A, b2 = e2 / A;
    if (!(b0 >= 0.f && b1 >= 0.f && b2 >= 0.f)) return false;  // (a NaN: not covered)
    const float q0 = b0 / p[0].z, q1 = b1 / p[1].z, q2 = b2 / p[2].z;
    const float iw = (q0 + q1) + q2;
    beta[0] = q0 / iw, beta[1] = q1 / iw, beta[2] = q2 / iw;
    depth = (beta[0] * p[0].w + beta[1] * p[1].w) + beta[2] * p[2].w;
    return depth > 0.f && finite_f(depth);
}

__device__ __forceinline__ void mr_vote(unsigned long long *__restrict__ vis, size_t pix, float depth, int f) {
    atomicMin(vis + pix, ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)f);
}

__global__ __launch_bounds__(THREADS) void k_mr_project(const float *__restrict__ vertices, long long Nv, int V,
                                                        const float *__restrict__ cam_view,
                                                        const float *__restrict__ cam_view_proj, int H, int W,
                                                        float4 *__restrict__ proj) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= V * Nv) return;
    const int v = (int)(i / Nv);
    const long long n = i - v * Nv;
    const float x = vertices[3 * n], y = vertices[3 * n + 1], z = vertices[3 * n + 2];
    float hom[4], pv[3];
    xf44(cam_view_proj + 16 * v, x, y, z, hom);
    xf43(cam_view + 16 * v, x, y, z, pv);
    const float w = hom[3];
    const float X = ndc2pix(hom[0] / w, W), Y = ndc2pix(hom[1] / w, H);
    const bool ok = w > 0.2f && finite_f(w) && finite_f(X) && finite_f(Y) && finite_f(pv[2]);
    proj[i] = ok ? make_float4(X, Y, w, pv[2]) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(THREADS) void k_mr_vis(const int *__restrict__ faces, const int *__restrict__ face_uvs,
                                                    long long Nu, long long Nf, long long Nv, int V,
                                                    const float4 *__restrict__ proj, int H, int W,
                                                    unsigned long long *__restrict__ vis, unsigned *__restrict__ head,
                                                    int *__restrict__ queue) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= V * Nf) return;
    const int v = (int)(i / Nf), f = (int)(i - v * Nf);
    float4 p[3];
    if (!mr_face(faces, face_uvs, Nu, proj, Nv, v, f, p)) return;
    int xa, xb, ya, yb;
    mr_box(p, H, W, xa, xb, ya, yb);
    if (xa > xb || ya > yb) return;
    if ((long long)(xb - xa + 1) * (yb - ya + 1) > LGM_MESHRASTER_SMALL_BOX) {
        queue[atomicAdd(head, 1u)] = (int)i;  // (at most V Nf items: the queue's size)
        return;
    }
    const size_t base = (size_t)v * H * W;
    for (int y = ya; y <= yb; y++)
        for (int x = xa; x <= xb; x++) {
            float beta[3], depth;
            if (mr_hit(p, (float)x, (float)y, beta, depth)) mr_vote(vis, base + (size_t)y * W + x, depth, f);
        }
}

__global__ __launch_bounds__(THREADS) void k_mr_vis_big(const int *__restrict__ faces,
                                                        const int *__restrict__ face_uvs, long long Nu, long long Nf,
                                                        long long Nv, int V, const float4 *__restrict__ proj, int H, int W,
                                                        unsigned long long *__restrict__ vis,
                                                        const unsigned *__restrict__ head,
                                                        const int *__restrict__ queue) {
    const unsigned n = min(head[0], (unsigned)(V * Nf));
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const long long i = queue[e];
        if (i < 0 || i >= V * Nf) continue;
        const int v = (int)(i / Nf), f = (int)(i - v * Nf);
        float4 p[3];
        if (!mr_face(faces, face_uvs, Nu, proj, Nv, v, f, p)) continue;
        int xa, xb, ya, yb;
        mr_box(p, H, W, xa, xb, ya, yb);
        if (xa > xb || ya > yb) continue;
        const int bw = xb - xa + 1, npix = bw * (yb - ya + 1);
        const size_t base = (size_t)v * H * W;
        for (int k = threadIdx.x; k < npix; k += THREADS) {
            const int y = ya + k / bw, x = xa + k % bw;
            float beta[3], depth;
            if (mr_hit(p, (float)x, (float)y, beta, depth)) mr_vote(vis, base + (size_t)y * W + x, depth, f);
        }
    }
}

// The four texels and weights of the header's bilinear fetch at (u, v). Indices are clamped in float first, so a
// non-finite or huge uv reads inside the texture (and gives a non-finite colour through the weights).
__device__ __forceinline__ void mr_bilinear(float u, float v, int Ht, int Wt, int idx[4], float wgt[4]) {
#pragma clang fp contract(off)
    const float tx = u * (float)Wt - 0.5f, ty = (1.f - v) * (float)Ht - 0.5f;
    const float flx = floorf(tx), fly = floorf(ty);
    const float fx = tx - flx, fy = ty - fly;
    const int ix = (int)fminf(fmaxf(flx, -1.f), (float)Wt), iy = (int)fminf(fmaxf(fly, -1.f), (float)Ht);
    const int x0 = min(max(ix, 0), Wt - 1), x1 = min(max(ix + 1, 0), Wt - 1);
    const int y0 = min(max(iy, 0), Ht - 1), y1 = min(max(iy + 1, 0), Ht - 1);
    idx[0] = y0 * Wt + x0, idx[1] = y0 * Wt + x1, idx[2] = y1 * Wt + x0, idx[3] = y1 * Wt + x1;
    wgt[0] = (1.f - fx) * (1.f - fy), wgt[1] = fx * (1.f - fy), wgt[2] = (1.f - fx) * fy, wgt[3] = fx * fy;
}

// What a covered pixel reads: in texture mode the four texels idx (element index / 3) and weights, in colour mode the
// three vertices and beta (n = 4 or 3). false: no face, or one that the guards reject.
struct MrTaps {
    int idx[4];
    float wgt[4];
    int n;
};
__device__ __forceinline__ bool mr_taps(unsigned long long key, const int *__restrict__ faces, long long Nf, long long Nv,
                                        const float4 *__restrict__ proj, int v, int x, int y,
                                        const float *__restrict__ uvs, long long Nu, const int *__restrict__ face_uvs,
                                        int Ht, int Wt, bool textured, MrTaps &t) {
#pragma clang fp contract(off)
    if (key == NO_HIT) return false;
    const unsigned f = (unsigned)key;
    if (f >= (unsigned long long)Nf) return false;  // (a workspace that is not the forward's)
    float4 p[3];
    if (!mr_face(faces, textured ? face_uvs : nullptr, Nu, proj, Nv, v, (int)f, p)) return false;
    float beta[3], depth;
    if (!mr_hit(p, (float)x, (float)y, beta, depth)) return false;
    if (!textured) {
        t.n = 3;
#pragma unroll
        for (int k = 0; k < 3; k++) t.idx[k] = faces[3 * (size_t)f + k], t.wgt[k] = beta[k];
        t.idx[3] = 0, t.wgt[3] = 0.f;
        return true;
    }
    float uv[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int j = face_uvs[3 * (size_t)f + k];  // (in range: mr_face)
        uv[k][0] = uvs[2 * (size_t)j], uv[k][1] = uvs[2 * (size_t)j + 1];
    }
    const float u = (beta[0] * uv[0][0] + beta[1] * uv[1][0]) + beta[2] * uv[2][0];
    const float w = (beta[0] * uv[0][1] + beta[1] * uv[1][1]) + beta[2] * uv[2][1];
    t.n = 4;
    mr_bilinear(u, w, Ht, Wt, t.idx, t.wgt);
    return true;
}

__global__ __launch_bounds__(THREADS) void k_mr_shade(const int *__restrict__ faces, long long Nf, long long Nv, int V,
                                                      const float4 *__restrict__ proj, int H, int W,
                                                      const unsigned long long *__restrict__ vis,
                                                      const float *__restrict__ uvs, long long Nu,
                                                      const int *__restrict__ face_uvs,
                                                      const float *__restrict__ texture, int Ht, int Wt,
                                                      const float *__restrict__ colors, const float *__restrict__ bg,
                                                      float *__restrict__ image, float *__restrict__ alpha,
                                                      float *__restrict__ depth, int *__restrict__ face_id) {
#pragma clang fp contract(off)
    const size_t P = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)V * P) return;
    const int v = (int)(i / P);
    const size_t pix = i - (size_t)v * P;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const unsigned long long key = vis[i];
    const bool textured = texture != nullptr;
    const float *src = textured ? texture : colors;
    MrTaps t;
    // (a face that entered the buffer passed mr_face's guards in k_mr_vis; mr_taps applies them again)
    const bool hit = mr_taps(key, faces, Nf, Nv, proj, v, x, y, uvs, Nu, face_uvs, Ht, Wt, textured, t);
    float c[3] = {bg[0], bg[1], bg[2]};
    if (hit) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float s = t.wgt[0] * src[3 * (size_t)t.idx[0] + ch];
#pragma unroll
            for (int k = 1; k < 4; k++)
                if (k < t.n) s = s + t.wgt[k] * src[3 * (size_t)t.idx[k] + ch];
            c[ch] = s;
        }
    }
    for (int ch = 0; ch < 3; ch++) image[((size_t)v * 3 + ch) * P + pix] = c[ch];
    alpha[i] = hit ? 1.f : 0.f;
    if (depth) depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
    if (face_id) face_id[i] = hit ? (int)(unsigned)key : -1;
}

__global__ __launch_bounds__(THREADS) void k_mr_absmax(const float *__restrict__ d_image, size_t n,
                                                       unsigned *__restrict__ amax) {
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS)
        m = max(m, __float_as_uint(d_image[i]) & 0x7fffffffu);  // (bits of |d|: they order like the value, NaN on top)
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(amax, m);
}

// E with 2^(E - 1) <= amax < 2^E from amax's bits; false: amax is 0 (nothing to add) or not finite
__device__ __forceinline__ bool mr_exponent(unsigned bits, int &E) {
    if (bits == 0 || bits >= 0x7f800000u) return false;
    (void)frexpf(__uint_as_float(bits), &E);
    return true;
}

__global__ __launch_bounds__(THREADS) void k_mr_scatter(const int *__restrict__ faces, long long Nf, long long Nv, int V,
                                                        const float4 *__restrict__ proj, int H, int W,
                                                        const unsigned long long *__restrict__ vis,
                                                        const float *__restrict__ uvs, long long Nu,
                                                        const int *__restrict__ face_uvs, int Ht, int Wt, bool textured,
                                                        const float *__restrict__ d_image,
                                                        const unsigned *__restrict__ amax, int S,
                                                        unsigned long long *__restrict__ acc) {
#pragma clang fp contract(off)
    const size_t P = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (size_t)V * P) return;
    int E;
    if (!mr_exponent(amax[0], E)) return;
    const int v = (int)(i / P);
    const size_t pix = i - (size_t)v * P;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    MrTaps t;
    if (!mr_taps(vis[i], faces, Nf, Nv, proj, v, x, y, uvs, Nu, face_uvs, Ht, Wt, textured, t)) return;
    const double scale = ldexp(1.0, S - E);
    for (int ch = 0; ch < 3; ch++) {
        const float d = d_image[((size_t)v * 3 + ch) * P + pix];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k >= t.n) continue;
            const long long q = __double2ll_rn((double)(d * t.wgt[k]) * scale);
            if (q) atomicAdd(acc + 3 * (size_t)t.idx[k] + ch, (unsigned long long)q);
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_mr_convert(const unsigned long long *__restrict__ acc, size_t n,
                                                        const unsigned *__restrict__ amax, int S,
                                                        float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned bits = amax[0];
    int E;
    if (!mr_exponent(bits, E)) {
        out[i] = bits ? __uint_as_float(0x7fc00000u) : 0.f;
        return;
    }
    out[i] = (float)((double)(long long)acc[i] * ldexp(1.0, E - S));
}

unsigned blocks_for(size_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_meshraster_workspace_size(int V, long long Nv, long long Nf, int H, int W, int Ht, int Wt) {
    using namespace lgm;
    if (!mr_sizes_ok(V, Nv, Nf, H, W) || Ht < 0 || Wt < 0 || 3LL * Ht * Wt >= I31) return 0;
    return mr_layout(V, Nv, Nf, H, W, Ht, Wt).total;
}

extern "C" int lgm_meshraster_unit_log2(int V, int H, int W) {
    if (V < 1 || H < 1 || W < 1 || 3LL * V * H >= lgm::I31 || 3LL * V * H * W >= lgm::I31) return -1;
    return lgm::unit_log2(V, H, W);
}

extern "C" int lgm_meshraster_forward(const float *vertices, long long Nv, const int *faces, long long Nf,
                                      const float *uvs, long long Nu, const int *face_uvs, const float *texture, int Ht,
                                      int Wt, const float *colors, const float *cam_view, const float *cam_view_proj,
                                      int V, const float *bg, int H, int W, float *image, float *alpha, float *depth,
                                      int *face_id, void *ws, size_t ws_bytes, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_meshraster_forward";
    const bool textured = texture != nullptr;
    if (!textured) Nu = 0, Ht = 0, Wt = 0;
    if (!mr_sizes_ok(V, Nv, Nf, H, W) || Nu < 0 || 2 * Nu >= I31) {
        set_error("%s: V=%d Nv=%lld Nf=%lld Nu=%lld H=%d W=%d: V, H, W >= 1, counts >= 0, every element count (3 Nv, 3 Nf, "
                  "2 Nu, 3 V H W, V Nv, V Nf) below 2^31", who, V, Nv, Nf, Nu, H, W);
        return LGM_E_INVALID;
    }
    if (textured && (Ht < 1 || Wt < 1 || 3LL * Ht * Wt >= I31)) {
        set_error("%s: texture %d x %d: each dimension >= 1, 3 Ht Wt below 2^31", who, Ht, Wt);
        return LGM_E_INVALID;
    }
    if (!cam_view || !cam_view_proj || !bg || !image || !alpha || !ws || (Nv > 0 && !vertices) || (Nf > 0 && !faces) ||
        (Nf > 0 && (textured ? (!uvs || !face_uvs) : !colors))) {
        set_error("%s: null pointer (cam_view, cam_view_proj, bg, image, alpha, ws, vertices, faces, and uvs and face_uvs "
                  "with a texture or colors without)", who);
        return LGM_E_INVALID;
    }
    const MrLayout L = mr_layout(V, Nv, Nf, H, W, Ht, Wt);
    if (int rc = check_workspace(who, ws, ws_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    const size_t P = (size_t)V * H * W;
    if (hipMemsetAsync(w + L.vis, 0xff, P * 8, st) != hipSuccess || hipMemsetAsync(w + L.head, 0, 16, st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return LGM_E_HIP;
    }
    float4 *proj = (float4 *)(w + L.proj);
    unsigned long long *vis = (unsigned long long *)(w + L.vis);
    unsigned *head = (unsigned *)(w + L.head);
    int *queue = (int *)(w + L.queue);
    if (Nf > 0 && Nv > 0) {
        LGM_LAUNCH("k_mr_project", st,
                   (k_mr_project<<<blocks_for((size_t)V * Nv), THREADS, 0, st>>>(vertices, Nv, V, cam_view,
                                                                                 cam_view_proj, H, W, proj)));
        LGM_LAUNCH("k_mr_vis", st,
                   (k_mr_vis<<<blocks_for((size_t)V * Nf), THREADS, 0, st>>>(faces, textured ? face_uvs : nullptr, Nu, Nf,
                                                                             Nv, V, proj, H, W, vis, head, queue)));
        LGM_LAUNCH("k_mr_vis_big", st,
                   (k_mr_vis_big<<<(unsigned)std::min<long long>(BIG_GRID, V * Nf), THREADS, 0, st>>>(
                       faces, textured ? face_uvs : nullptr, Nu, Nf, Nv, V, proj, H, W, vis, head, queue)));
    }
    LGM_LAUNCH("k_mr_shade", st,
               (k_mr_shade<<<blocks_for(P), THREADS, 0, st>>>(faces, Nf, Nv, V, proj, H, W, vis, uvs, Nu, face_uvs,
                                                              texture, Ht, Wt, colors, bg, image, alpha, depth,
                                                              face_id)));
    return LGM_OK;
}

extern "C" int lgm_meshraster_backward(long long Nv, const int *faces, long long Nf, const float *uvs, long long Nu,
                                       const int *face_uvs, int Ht, int Wt, int V, int H, int W, const float *d_image,
                                       float *d_texture, float *d_colors, void *ws, size_t ws_bytes, void *stream,
                                       const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_meshraster_backward";
    const bool textured = d_texture != nullptr;
    if (!textured) Nu = 0, Ht = 0, Wt = 0;
    if (!mr_sizes_ok(V, Nv, Nf, H, W) || Nu < 0 || 2 * Nu >= I31) {
        set_error("%s: V=%d Nv=%lld Nf=%lld Nu=%lld H=%d W=%d: V, H, W >= 1, counts >= 0, every element count (3 Nv, 3 Nf, "
                  "2 Nu, 3 V H W, V Nv, V Nf) below 2^31", who, V, Nv, Nf, Nu, H, W);
        return LGM_E_INVALID;
    }
    if (textured && (Ht < 1 || Wt < 1 || 3LL * Ht * Wt >= I31)) {
        set_error("%s: texture %d x %d: each dimension >= 1, 3 Ht Wt below 2^31", who, Ht, Wt);
        return LGM_E_INVALID;
    }
    if (!d_image || !ws || (!textured && Nv > 0 && !d_colors) || (Nf > 0 && !faces) ||
        (Nf > 0 && textured && (!uvs || !face_uvs))) {
        set_error("%s: null pointer (d_image, ws, d_texture or d_colors, faces, and uvs and face_uvs with a texture)", who);
        return LGM_E_INVALID;
    }
    const MrLayout L = mr_layout(V, Nv, Nf, H, W, Ht, Wt);
    if (int rc = check_workspace(who, ws, ws_bytes, L.total)) return rc;
    const size_t n = 3 * (textured ? (size_t)Ht * Wt : (size_t)Nv);
    if (n == 0) return LGM_OK;
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    const size_t P = (size_t)V * H * W;
    unsigned *amax = (unsigned *)(w + L.head) + 1;
    unsigned long long *acc = (unsigned long long *)(w + L.acc);
    if (hipMemsetAsync(amax, 0, 4, st) != hipSuccess || hipMemsetAsync(acc, 0, n * 8, st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return LGM_E_HIP;
    }
    const int S = unit_log2(V, H, W);
    LGM_LAUNCH("k_mr_absmax", st,
               (k_mr_absmax<<<std::min(blocks_for(3 * P), 1024u), THREADS, 0, st>>>(d_image, 3 * P, amax)));
    if (Nf > 0 && Nv > 0)
        LGM_LAUNCH("k_mr_scatter", st,
                   (k_mr_scatter<<<blocks_for(P), THREADS, 0, st>>>(
                       faces, Nf, Nv, V, (const float4 *)(w + L.proj), H, W, (const unsigned long long *)(w + L.vis), uvs,
                       Nu, face_uvs, Ht, Wt, textured, d_image, amax, S, acc)));
    LGM_LAUNCH("k_mr_convert", st,
               (k_mr_convert<<<blocks_for(n), THREADS, 0, st>>>(acc, n, amax, S, textured ? d_texture : d_colors)));
    return LGM_OK;
}
