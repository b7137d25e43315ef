// lgm_amd/csrc/render_api.hip -- extern "C" entry points of include/lgm_render.h.
//
// lgm_render_forward  replaces the B*V calls of _C.rasterize_gaussians made by core/gs.py:73-85;
// lgm_render_backward replaces the B*V calls of _C.rasterize_gaussians_backward plus autograd's sum over views
// through the slices of core/gs.py:45-49. Kernels: render_bin.hip (preprocess, binning, sort),
// render_fwd.hip / render_bwd.hip (compositing forward / backward), render_preproc_bwd.hip (projection backward).
#include "render_common.h"

namespace {

int check_common(int B, int V, int N, int H, int W, const void *g, const void *cv, const void *cvp, float tanx,
                 float tany, float mod, lgm::Dims &d) {
    if (B <= 0 || V <= 0 || N < 0 || H <= 0 || W <= 0 || H > lgm::BY * 65535 || W > lgm::BX * 65535) {
        lgm::set_error("invalid sizes (B=%d V=%d N=%d H=%d W=%d)", B, V, N, H, W);
        return LGM_E_INVALID;
    }
    if ((N > 0 && !g) || !cv || !cvp) {
        lgm::set_error("null input pointer");
        return LGM_E_INVALID;
    }
    if (!(tanx > 0.f) || !(tany > 0.f)) {
        lgm::set_error("tanfov must be positive");
        return LGM_E_INVALID;
    }
    d.B = B; d.V = V; d.N = N; d.H = H; d.W = W;
    d.gx = (W + lgm::BX - 1) / lgm::BX;
    d.gy = (H + lgm::BY - 1) / lgm::BY;
    d.T = d.gx * d.gy;
    d.BV = B * V;
    d.ck_shift = lgm::ck_shift_for((size_t)d.BV * d.T);
    d.tanx = tanx; d.tany = tany;
    d.fx = W / (2.0f * tanx);
    d.fy = H / (2.0f * tany);
    d.mod = mod;
    const lgm_diag *diag = lgm::call_diag();  // this call's diagnostics (DiagScope), or none
    d.counters = diag ? diag->render_counters : nullptr;
    d.det_lim_log2 = diag ? diag->det_limit_log2 : 0;
    d.options = 0;
    d.gt_img = d.gt_mask = nullptr;
    d.loss_part = d.loss_out = nullptr;
    d.d_loss = nullptr;
    d.aa_s = nullptr;
    d.sh_col = nullptr;
    d.sh_part = nullptr;
    return LGM_OK;
}

bool capacity_ok(long long cap) { return cap <= 0x7fffffffLL; }

// lgm_render_needle_flags: render_common.h rec_needle (the decision the binning and the backward's flush both take
// on a stored record) evaluated on caller-given (A', B', C')
__global__ __launch_bounds__(256) void k_needle_flags(long long n, const float *__restrict__ abc,
                                                      unsigned char *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = lgm::rec_needle(abc[3 * i], abc[3 * i + 1], abc[3 * i + 2]) ? 1 : 0;
}

// Inspection kernels (lgm_render_tile_lists / lgm_render_pixel_state): plain copies out of the workspace.
__global__ __launch_bounds__(256) void k_tile_counts(int M, long long slot_stride, const int *__restrict__ tile_start,
                                                     const int *__restrict__ tile_count, int *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M) return;
    long long base;
    int n;
    lgm::tile_range(t, slot_stride, tile_start, tile_count, base, n);
    out[t] = n;
}
// one workgroup per (view, tile): its sorted ids (u32, in place at the start of its pair range) -> ids_out
__global__ __launch_bounds__(256) void k_tile_ids(long long slot_stride, const int *__restrict__ tile_start,
                                                  const int *__restrict__ tile_count,
                                                  const unsigned long long *__restrict__ pairs,
                                                  const long long *__restrict__ offsets, unsigned *__restrict__ ids_out) {
    const int t = blockIdx.x;
    long long base;
    int n;
    lgm::tile_range(t, slot_stride, tile_start, tile_count, base, n);
    const unsigned *ids = reinterpret_cast<const unsigned *>(pairs + base);
    unsigned *dst = ids_out + offsets[t];
    for (int e = threadIdx.x; e < n; e += 256) dst[e] = ids[e];
}

int check_ws(int B, int V, int N, int H, int W, const void *ws, size_t ws_bytes, long long cap, lgm::Layout &L) {
    if (B <= 0 || V <= 0 || N < 0 || H <= 0 || W <= 0) {
        lgm::set_error("invalid sizes (B=%d V=%d N=%d H=%d W=%d)", B, V, N, H, W);
        return LGM_E_INVALID;
    }
    // (without the call's options: every region the inspection entry points read sits ahead of the ones the options
    // resize -- render_layout.h, checked by tests/test_render_layout.py)
    L = lgm::make_layout(B, V, N, H, W, cap, 0);
    if (!ws || ws_bytes < L.total) {
        lgm::set_error("workspace too small (%zu < %zu)", ws_bytes, L.total);
        return LGM_E_WORKSPACE;
    }
    return LGM_OK;
}
// (the inspection entry points only read through the view)
lgm::Workspace read_view(const void *ws, const lgm::Layout &L) { return lgm::Workspace((char *)ws, L); }

// The part of a call's set-up that forward_impl and backward_impl share: the options, the antialias factors and the
// fused loss's ground truth. `third` is the loss's third pointer (loss_out / d_loss): the three come together or not
// at all.
int setup_call(lgm::Dims &d, int options, const lgm::Workspace &w, const float *gt_images, const float *gt_masks,
               const void *third, const char *pass, const char *third_name) {
    d.options = options & ~LGM_RENDER_FUSED_LOSS;
    d.aa_s = w.aa_s;
    d.sh_col = w.sh_col;
    d.sh_part = w.sh_part;
    if (gt_images || gt_masks || third) {
        if (!gt_images || !gt_masks || !third) {
            lgm::set_error("fused loss%s needs gt_images, gt_masks and %s", pass, third_name);
            return LGM_E_INVALID;
        }
        d.options |= LGM_RENDER_FUSED_LOSS;
        d.gt_img = gt_images;
        d.gt_mask = gt_masks;
    }
    return LGM_OK;
}

}  // namespace

extern "C" {

size_t lgm_render_workspace_size(int B, int V, int N, int H, int W, long long pair_capacity) {
    return lgm_render_workspace_size_opts(B, V, N, H, W, pair_capacity, 0);
}

size_t lgm_render_workspace_size_opts(int B, int V, int N, int H, int W, long long pair_capacity, int options) {
    if (B <= 0 || V <= 0 || N < 0 || H <= 0 || W <= 0) return 0;
    return lgm::make_layout(B, V, N, H, W, pair_capacity, options).total;
}

int lgm_render_count_pairs(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                           const float *cam_view_proj, float tanfovx, float tanfovy, float scale_modifier,
                           void *workspace, size_t workspace_bytes, long long *pairs_out, void *stream,
                           const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    lgm::Dims d;
    int rc = check_common(B, V, N, H, W, gaussians, cam_view, cam_view_proj, tanfovx, tanfovy, scale_modifier, d);
    if (rc) return rc;
    if (!pairs_out) {
        lgm::set_error("null pairs_out");
        return LGM_E_INVALID;
    }
    const lgm::Layout L = lgm::make_layout(B, V, N, H, W, 1, 0);
    if (!workspace || workspace_bytes < L.total) {
        lgm::set_error("workspace too small for counting (%zu < %zu)", workspace_bytes, L.total);
        return LGM_E_WORKSPACE;
    }
    return lgm::launch_binning(d, gaussians, cam_view, cam_view_proj, lgm::Workspace((char *)workspace, L), L, nullptr,
                               pairs_out, true, (hipStream_t)stream);
}

}  // extern "C"

static int forward_impl(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                        const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                        float scale_modifier, float *image, float *depth, float *alpha, int *radii_out,
                        const float *gt_images, const float *gt_masks, float *loss_out, void *workspace,
                        size_t workspace_bytes, long long pair_capacity, long long *stats_out, int options,
                        void *stream, const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    lgm::Dims d;
    int rc = check_common(B, V, N, H, W, gaussians, cam_view, cam_view_proj, tanfovx, tanfovy, scale_modifier, d);
    if (rc) return rc;
    if (!bg || !image || !depth || !alpha) {
        lgm::set_error("null output pointer");
        return LGM_E_INVALID;
    }
    const lgm::Layout L = lgm::make_layout(B, V, N, H, W, pair_capacity, options);
    if (!L.slot && !capacity_ok(L.cap)) {  // packed tile offsets are int32; slot offsets are 64-bit
        lgm::set_error("pair capacity %lld exceeds 2^31", L.cap);
        return LGM_E_INVALID;
    }
    if (!workspace || workspace_bytes < L.total) {
        lgm::set_error("workspace too small (%zu < %zu)", workspace_bytes, L.total);
        return LGM_E_WORKSPACE;
    }
    const lgm::Workspace w((char *)workspace, L);
    rc = setup_call(d, options, w, gt_images, gt_masks, loss_out, "", "loss_out");
    if (rc) return rc;
    if (d.options & LGM_RENDER_FUSED_LOSS) {
        d.loss_part = &w.lossp->x;
        d.loss_out = loss_out;
    }
    hipStream_t st = (hipStream_t)stream;
    // LGM_RENDER_SH_MASK: `gaussians` has rows of 11 + 3K; the kernels that know 14-wide rows run on the workspace's
    // copy of columns 0:14, and the compositing stages the colours k_sh_colour wrote (render_sh.hip)
    const int sh = N > 0 ? lgm::sh_degree_of(options) : 0;
    if (sh && (rc = lgm::launch_sh_pack(d, sh, gaussians, w, L, st))) return rc;
    const float *g14 = sh ? w.sh_g14 : gaussians;
    rc = lgm::launch_binning(d, g14, cam_view, cam_view_proj, w, L, radii_out, stats_out, false, st);
    if (rc) return rc;
    if (sh && (rc = lgm::launch_sh_colour(d, sh, gaussians, cam_view, w, st))) return rc;
    rc = lgm::launch_render_fwd(d, g14, bg, image, depth, alpha, w, L, st);
    if (rc || !(d.options & LGM_RENDER_FUSED_LOSS)) return rc;
    return lgm::launch_loss_reduce(d, w, st);
}

static int backward_impl(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                         const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                         float scale_modifier, const float *d_image, const float *d_depth, const float *d_alpha,
                         const float *gt_images, const float *gt_masks, const float *d_loss, float *d_gaussians,
                         float *d_means2D, void *workspace, size_t workspace_bytes, long long pair_capacity,
                         int options, void *stream, const lgm_diag *diag) {
    lgm::clear_error();
    lgm::DiagScope ds(diag);
    lgm::Dims d;
    int rc = check_common(B, V, N, H, W, gaussians, cam_view, cam_view_proj, tanfovx, tanfovy, scale_modifier, d);
    if (rc) return rc;
    if (!bg || (N > 0 && !d_gaussians)) {
        lgm::set_error("null pointer in backward");
        return LGM_E_INVALID;
    }
    const lgm::Layout L = lgm::make_layout(B, V, N, H, W, pair_capacity, options);
    if (!workspace || workspace_bytes < L.total) {
        lgm::set_error("workspace too small (%zu < %zu)", workspace_bytes, L.total);
        return LGM_E_WORKSPACE;
    }
    if (N == 0) return LGM_OK;
    const lgm::Workspace w((char *)workspace, L);
    rc = setup_call(d, options, w, gt_images, gt_masks, d_loss, " backward", "d_loss");
    if (rc) return rc;
    d.d_loss = d_loss;
    // LGM_RENDER_SH_MASK: k_preproc_bwd writes 14-wide rows to the workspace; k_sh_bwd then writes the caller's
    const int sh = lgm::sh_degree_of(options);
    rc = lgm::launch_render_bwd(d, sh ? w.sh_g14 : gaussians, cam_view, cam_view_proj, bg, d_image, d_depth, d_alpha,
                                sh ? w.sh_dg14 : d_gaussians, d_means2D, w, L, (hipStream_t)stream);
    if (rc || !sh) return rc;
    return lgm::launch_sh_bwd(d, sh, gaussians, cam_view, d_gaussians, w, (hipStream_t)stream);
}

extern "C" {

int lgm_render_forward(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                       const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                       float scale_modifier, float *image, float *depth, float *alpha, int *radii_out,
                       void *workspace, size_t workspace_bytes, long long pair_capacity, long long *stats_out,
                       int options, void *stream, const lgm_diag *diag) {
    return forward_impl(B, V, N, H, W, gaussians, cam_view, cam_view_proj, bg, tanfovx, tanfovy, scale_modifier,
                        image, depth, alpha, radii_out, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                        pair_capacity, stats_out, options, stream, diag);
}

int lgm_render_forward_loss(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                            const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                            float scale_modifier, float *image, float *depth, float *alpha, const float *gt_images,
                            const float *gt_masks, float *loss_out, void *workspace, size_t workspace_bytes,
                            long long pair_capacity, int options, void *stream, const lgm_diag *diag) {
    if (!gt_images || !gt_masks || !loss_out) {
        lgm::set_error("null gt_images / gt_masks / loss_out");
        return LGM_E_INVALID;
    }
    return forward_impl(B, V, N, H, W, gaussians, cam_view, cam_view_proj, bg, tanfovx, tanfovy, scale_modifier,
                        image, depth, alpha, nullptr, gt_images, gt_masks, loss_out, workspace, workspace_bytes,
                        pair_capacity, nullptr, options, stream, diag);
}

int lgm_render_backward_loss(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                             const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                             float scale_modifier, const float *d_image, const float *d_alpha,
                             const float *gt_images, const float *gt_masks, const float *d_loss,
                             float *d_gaussians, void *workspace, size_t workspace_bytes, long long pair_capacity,
                             int options, void *stream, const lgm_diag *diag) {
    if (!gt_images || !gt_masks || !d_loss) {
        lgm::set_error("null gt_images / gt_masks / d_loss");
        return LGM_E_INVALID;
    }
    return backward_impl(B, V, N, H, W, gaussians, cam_view, cam_view_proj, bg, tanfovx, tanfovy, scale_modifier,
                         d_image, nullptr, d_alpha, gt_images, gt_masks, d_loss, d_gaussians, nullptr, workspace,
                         workspace_bytes, pair_capacity, options, stream, diag);
}

int lgm_render_tile_lists(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                          long long pair_capacity, int *tile_counts_out, const long long *offsets,
                          unsigned *ids_out, void *stream) {
    lgm::clear_error();
    lgm::Layout L;
    int rc = check_ws(B, V, N, H, W, workspace, workspace_bytes, pair_capacity, L);
    if (rc) return rc;
    if (!tile_counts_out || (ids_out && !offsets)) {
        lgm::set_error("null tile_counts_out / offsets");
        return LGM_E_INVALID;
    }
    const int T = ((W + lgm::BX - 1) / lgm::BX) * ((H + lgm::BY - 1) / lgm::BY), M = B * V * T;
    const lgm::Workspace w = read_view(workspace, L);
    const long long stride = L.slot ? (long long)N : -1LL;
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_tile_counts", st, (k_tile_counts<<<(M + 255) / 256, 256, 0, st>>>(M, stride, w.tile_start, w.tile_count,
                                                                                    tile_counts_out)));
    if (ids_out && N > 0)
        LGM_LAUNCH("k_tile_ids", st, (k_tile_ids<<<M, 256, 0, st>>>(stride, w.tile_start, w.tile_count, w.pairs, offsets,
                                                                    ids_out)));
    return LGM_OK;
}

int lgm_render_pixel_state(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                           long long pair_capacity, int *n_contrib_out, float *final_T_out, void *stream) {
    lgm::clear_error();
    lgm::Layout L;
    int rc = check_ws(B, V, N, H, W, workspace, workspace_bytes, pair_capacity, L);
    if (rc) return rc;
    const size_t P = (size_t)B * V * H * W;
    const lgm::Workspace w = read_view(workspace, L);
    hipStream_t st = (hipStream_t)stream;
    if (n_contrib_out && hipMemcpyAsync(n_contrib_out, w.n_contrib, P * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        lgm::set_error("hipMemcpyAsync failed");
        return LGM_E_HIP;
    }
    if (final_T_out && hipMemcpyAsync(final_T_out, w.final_T, P * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        lgm::set_error("hipMemcpyAsync failed");
        return LGM_E_HIP;
    }
    return LGM_OK;
}

int lgm_render_records(int B, int V, int N, int H, int W, const void *workspace, size_t workspace_bytes,
                       long long pair_capacity, float *P_out, float *Q_out, unsigned *rects_out, void *stream) {
    lgm::clear_error();
    lgm::Layout L;
    int rc = check_ws(B, V, N, H, W, workspace, workspace_bytes, pair_capacity, L);
    if (rc) return rc;
    const size_t BVN = (size_t)B * V * N;
    const lgm::Workspace w = read_view(workspace, L);
    hipStream_t st = (hipStream_t)stream;
    const struct { void *dst; const void *src; size_t bytes; } cp[3] = {
        {P_out, w.gP, BVN * 16}, {Q_out, w.gQ, BVN * 16}, {rects_out, w.rects, BVN * 8}};
    for (const auto &c : cp) {
        if (c.dst && c.bytes && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            lgm::set_error("hipMemcpyAsync failed");
            return LGM_E_HIP;
        }
    }
    return LGM_OK;
}

int lgm_render_needle_flags(long long n, const float *abc, unsigned char *flags_out, void *stream) {
    lgm::clear_error();
    if (n < 0 || (n > 0 && (!abc || !flags_out))) {
        lgm::set_error("invalid needle-flag arguments");
        return LGM_E_INVALID;
    }
    if (n == 0) return LGM_OK;
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_needle_flags", st, (k_needle_flags<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, abc, flags_out)));
    return LGM_OK;
}

int lgm_render_det_flush_limit_log2(int views, int tiles, int scene_record) {
    lgm::clear_error();
    if (views <= 0 || tiles <= 0) {
        lgm::set_error("lgm_render_det_flush_limit_log2: views and tiles must be positive");
        return LGM_E_INVALID;
    }
    return lgm::det_flush_limit_log2(views, tiles, scene_record != 0);
}

int lgm_render_backward(int B, int V, int N, int H, int W, const float *gaussians, const float *cam_view,
                        const float *cam_view_proj, const float *bg, float tanfovx, float tanfovy,
                        float scale_modifier, const float *d_image, const float *d_depth, const float *d_alpha,
                        float *d_gaussians, float *d_means2D, void *workspace, size_t workspace_bytes,
                        long long pair_capacity, int options, void *stream, const lgm_diag *diag) {
    return backward_impl(B, V, N, H, W, gaussians, cam_view, cam_view_proj, bg, tanfovx, tanfovy, scale_modifier,
                         d_image, d_depth, d_alpha, nullptr, nullptr, nullptr, d_gaussians, d_means2D, workspace,
                         workspace_bytes, pair_capacity, options, stream, diag);
}

}  // extern "C"
