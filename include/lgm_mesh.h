/*
 * lgm_mesh.h -- C ABI of the mesh-export kernels in liblgm_amd.so (lgm_amd/csrc/mesh.hip): Gaussians to a coloured
 * triangle mesh. The reference's convert.py fits a NeRF to renders of the Gaussians, samples it on a 256^3 grid over
 * [-1, 1]^3 (convert.py:263-289) and runs marching cubes; here the Gaussians themselves are the density field: they
 * are sampled on the same grid, the iso-surface is extracted by naive surface nets and coloured from the Gaussians
 * (a deviation from the reference's algorithm). Nothing is fitted and nothing is random: two calls on
 * the same input give the same bits. This header is the specification the tests evaluate in fp64.
 *
 * ---- Density pass: lgm_mesh_density_count, lgm_mesh_density ------------------------------------------------------
 * g [N, 14] fp32, the layout GaussianRenderer takes: position 0:3, opacity 3, scale 4:7, rotation quaternion
 * (r, x, y, z) 7:11, rgb 11:14. Grid: Gx, Gy, Gz nodes (each >= 3, Gx Gy Gz < 2^31), node (i, j, k) at
 * x = lo + (i, j, k) h (lo, h: HOST float[3], per axis; h > 0). Outputs sigma [Gx][Gy][Gz] and rgb [Gx][Gy][Gz][3], fp32, k fastest (the
 * index order of the reference's sigmas[x, y, z]). cutoff eps > 0 (LGM_MESH_CUTOFF by default).
 * For Gaussian n, with o its opacity and c its rgb:
 *   s   = scale * scale_modifier
 *   q^  = q / |q|,  (r, x, y, z) = q^,  R = the rotation the render preprocess builds (render_common.h quat_rot read
 *         row by row), here of the normalised quaternion:
 *           [ 1 - 2(yy + zz)   2(xy - rz)       2(xz + ry)     ]
 *           [ 2(xy + rz)       1 - 2(xx + zz)   2(yz - rx)     ]
 *           [ 2(xz - ry)       2(yz + rx)       1 - 2(xx + yy) ]
 *         so that the Gaussian's covariance is R diag(s)^2 R^T, the renderer's.
 *   y   = diag(s)^-1 R^T (x - mu),  d2 = y . y          (no 3x3 inverse covariance is formed: it is ill-conditioned
 *                                                        on needles)
 *   rho2 = 2 ln(o / eps)
 *   w   = o exp(-d2 / 2) at the nodes where d2 <= rho2, nothing elsewhere (at the cut the term equals eps).
 * A Gaussian is skipped when o <= eps, when any of its 14 fields is not finite, when a scale component (after
 * scale_modifier) is <= 0 or when its quaternion is zero.
 *   sigma = sum_n w_n,   rgb = sum_n w_n c_n / sum_n w_n,   (0, 0, 0) where sigma = 0;
 * both sums run in ascending n in fp32 (no float atomics: the result does not depend on launch order).
 * The kernels evaluate d2 in fp32 from a per-Gaussian record computed in fp64 (the nine entries of diag(s)^-1 R^T,
 * pre-scaled so that the weight is one v_exp_f32: w = 2^(log2 o - d2'), kept where that exponent is >= log2 eps), with
 * x - mu taken relative to the node's brick in fp64; a term within fp32 rounding of the cut may fall on either side
 * of it (the tests allow eps per such term).
 *
 * Kernels: the grid is cut into bricks of LGM_MESH_BRICK^3 nodes (the last one of an axis ragged). k_mesh_bin_count
 * (per Gaussian: the record, the axis-aligned box of half extent rho sqrt(sum_k (R_ak s_k)^2) on axis a, one integer
 * atomic per brick the box touches), k_mesh_scan_reduce / _top / _add (exclusive scan of the brick counts),
 * k_mesh_bin_fill (the per-brick lists), k_mesh_density (one workgroup per brick: sorts its list in LDS, or, past
 * LGM_MESH_SORT_CAP entries, walks all N boxes in order; two nodes per thread).
 * The lists' total length is data dependent: lgm_mesh_density_count runs the count and the scan alone and writes the
 * total to DEVICE memory (*npairs); the caller reads it (one host sync) and passes a capacity >= it to
 * lgm_mesh_density with a workspace of lgm_mesh_density_workspace_size(N, Gx, Gy, Gz, capacity) bytes (the count
 * call takes capacity 0). lgm_mesh_density repeats the count itself; a capacity below the total cannot be reported
 * by the host half of the library (it never reads device memory): nothing is written out of bounds and every sigma
 * and rgb is NaN. rgb may be NULL (sigma alone). N == 0 is valid: a zero grid (g may then be NULL).
 *
 * ---- Extraction pass: lgm_mesh_count, lgm_mesh_emit --------------------------------------------------------------
 * Naive surface nets on sigma (and optionally rgb) of the layout above, iso > 0.
 *   - A sample on the outermost node layer of the grid, or one that is not finite, is read as 0: every surface closes.
 *   - A node is inside iff its sample is >= iso.
 *   - A cell is indexed by its lowest corner (i, j, k), linear index (i (Gy - 1) + j)(Gz - 1) + k; it is active iff its
 *     8 corners are neither all inside nor all outside. Each active cell has one vertex; vertices are numbered by
 *     ascending cell index.
 *   - Vertex position: corner c = 4 di + 2 dj + dk of the cell is node (i + di, j + dj, k + dk); the 12 edges, in
 *     this order, are (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7), each from its lower
 *     node a to its upper node b. An edge whose endpoints differ (one inside, one not) crosses at a + t (b - a),
 *     t = (iso - s_a) / (s_b - s_a). In fp32, every operation rounded on its own: the crossings' offsets from the
 *     cell's lowest corner ((da) + t e_axis, components in [0, 1]) are summed in edge order and divided by their
 *     number m; p = (i, j, k) + that mean (grid units); vertex = lo + p h.
 *   - Vertex colour (rgb given): the sum, over the same edges in the same order, of rgb at the edge's inside endpoint
 *     (sigma >= iso > 0 there, so it is defined), divided by m. Without rgb no colours are written.
 *   - Faces: nodes n in ascending linear order (i Gy + j) Gz + k, per node the axes a = 0, 1, 2, every grid edge
 *     n -> n + e_a (inside the grid) whose endpoints differ. With b = (a + 1) mod 3, c = (a + 2) mod 3 the quad is the
 *     vertices of the cells q0 = n - e_b - e_c, q1 = n - e_c, q2 = n, q3 = n - e_b (the forced boundary layer
 *     guarantees all four exist). n inside and n + e_a outside: triangles (q0, q1, q2), (q0, q2, q3); otherwise
 *     (q0, q2, q1), (q0, q3, q2). Normals point from inside to outside.
 * Outputs: vertices [Nv, 3] fp32, colors [Nv, 3] fp32, faces [Nf, 3] int32.
 * lgm_mesh_count (k_mesh_classify: per-cell active flag and per-node triangle count; k_mesh_scan_*: plain multi-pass
 * exclusive scans of both) leaves the scans in the workspace and writes counts[0] = Nv, counts[1] = Nf to DEVICE
 * memory; the caller reads them (the one host sync, the packed render workspace's policy), allocates, and calls
 * lgm_mesh_emit (k_mesh_emit) with the same sigma, grid, iso and workspace, the counts it read (nv, nf) and the
 * capacities of its buffers (cap_v vertices, cap_f faces). Nothing is ever written past a capacity.
 *
 * ---- Sampling pass: lgm_mesh_sample_count, lgm_mesh_sample ---------------------------------------------------------
 * The same field at M arbitrary points [M, 3] fp32: sigma [M], rgb [M, 3] (or NULL). For a point p, sigma(p) and rgb(p)
 * are exactly the density pass's formulas with x = p: the same skip rules, the cut d2 <= rho2, both sums in ascending
 * n in fp32, rgb = 0 where sigma = 0. The grid (G, lo, h) is only the acceleration structure and the domain: a point
 * is sampled iff its three coordinates are finite and lo - h / 2 <= p <= lo + (G - 1/2) h on every axis, compared in
 * fp64 (the half-cell margin: a mesh vertex rounded an ulp past the box is still sampled); every other point gets
 * sigma = 0, rgb = 0. Two calls are bitwise equal; no float atomics.
 * Kernels: k_mesh_sample_bin_count is k_mesh_bin_count with boxes over continuous intervals: in node units brick b of
 * an axis owns [b BRICK, (b + 1) BRICK), the first brick from -1/2 and the last one to G - 1/2, and a Gaussian enters
 * every brick its [c - ext, c + ext] meets (the density pass's boxes are node ranges: a cut that ends between two
 * nodes of different bricks leaves the lower brick's list, where a point may still lie). k_mesh_scan_*, k_mesh_bin_fill
 * as above. k_mesh_point_count (per point: the test above, its brick = floor of its fp64 node coordinate, clamped,
 * over BRICK; one integer atomic; the outputs of a point that is not sampled), k_mesh_scan_*, k_mesh_point_fill (the
 * bricks' point lists, any order: a point's sum is its own), k_mesh_sample (one workgroup per brick with points, 256
 * points at a time, one per thread, against the brick's list ordered and staged as in k_mesh_density; the point and mu
 * are both taken relative to the brick's first node in fp64 before rounding).
 * lgm_mesh_sample_count is lgm_mesh_density_count for these lists (its workspace:
 * lgm_mesh_sample_workspace_size(N, 0, Gx, Gy, Gz, 0)); lgm_mesh_sample takes a capacity >= that total and a workspace
 * of lgm_mesh_sample_workspace_size(N, M, Gx, Gy, Gz, capacity) bytes. A capacity below the total: every sigma and rgb
 * is NaN (the points that are not sampled too), nothing is written out of bounds. M == 0 and N == 0 are valid.
 *
 * ---- Atlas: lgm_mesh_atlas ------------------------------------------------------------------------------------------
 * A per-quad texture atlas for a mesh of the extraction pass, whose faces 2q and 2q + 1 are the quad q: outward
 * (q0, q1, q2), (q0, q2, q3) or flipped (q0, q2, q1), (q0, q3, q2) (read off the pair: the second face starts with the
 * first one's q0; outward iff the first face's last index is the second one's middle index). Quad q gets the block of
 * T x T texels (T >= 2) at column q mod cols, row q / cols of a texture of W = cols T by H = rows T texels
 * (cols rows >= the number of quads, W and H at most LGM_MESH_ATLAS_MAX).
 *   - points [nq][T][T][3], texel (i, j) at [q][j][i]: s = i / (T - 1), t = j / (T - 1) (i runs along q0 -> q1, j along
 *     q1 -> q2); s >= t: (1 - s) v0 + (s - t) v1 + t v2, otherwise (1 - t) v0 + (t - s) v3 + s v2: the point of the
 *     triangle that is drawn there. fp32, every operation rounded on its own, the three products summed left to right.
 *     Texel (0, 0) is v0 and texel (T - 1, T - 1) is v2.
 *   - uvs [nq][4][2]: entry k of quad q is the corner of q_k, (a, b) = (0, 0), (1, 0), (1, 1), (0, 1), at the pixel
 *     centre x = x0 + 1/2 + a (T - 1), y = y0 + 1/2 + b (T - 1) with (x0, y0) = (T (q mod cols), T (q / cols)):
 *     u = x / W, v = 1 - y / H (fp32, as above). Bilinear filtering inside a quad never leaves its block.
 *   - face_uvs [nf][3] int32: for every face corner the index into uvs (4 q + k) of the vertex faces names there.
 * A pair without that structure, or with an index outside [0, nv): its block's points are NaN (callers validate
 * first: lgm_amd.mesh.bake_texture raises).
 *
 * ---- Errors --------------------------------------------------------------------------------------------------------
 * rc < 0 (and lgm_last_error), with nothing launched, on: a required pointer that is null (g with N > 0, lo, h, ws,
 * npairs / counts, sigma, vertices with nv > 0, faces with nf > 0, colors with rgb given and nv > 0), N < 0 or
 * N >= 2^31, a grid axis < 3, Gx Gy Gz >= 2^31, a non-finite lo or scale_modifier, a non-finite or non-positive h, iso
 * or cutoff, a negative capacity or count, a capacity or count whose element count (3 per vertex or face, 1 per list
 * entry) is >= 2^31, a workspace shorter than the *_workspace_size, cap_v < nv or cap_f < nf. Sampling: the density
 * pass's rules, and M < 0, 3 M >= 2^31, points or sigma null with M > 0. Atlas: nv or nf negative, nf odd, 3 nv, 3 nf
 * or 3 nq T T >= 2^31, T < 2, cols or rows < 1, cols rows < nq, cols T or rows T > LGM_MESH_ATLAS_MAX, a null pointer
 * with nq > 0.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises. The library keeps
 * no state: what lgm_mesh_count leaves for lgm_mesh_emit lives in the caller's workspace.
 */
#ifndef LGM_MESH_H
#define LGM_MESH_H
#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_MESH_CUTOFF 1e-4f  /* default eps: a Gaussian's term is dropped where it falls below this */
#define LGM_MESH_BRICK 8       /* nodes per brick edge: one workgroup per brick */
#define LGM_MESH_SORT_CAP 4096 /* longest brick list sorted in LDS; longer ones walk all N boxes in order */
#define LGM_MESH_ATLAS_MAX 16384 /* widest and tallest atlas texture, in texels */

/* bytes of the density workspace for N Gaussians on the grid with room for `capacity` list entries (0: the count
 * call); 0 on invalid sizes */
size_t lgm_mesh_density_workspace_size(long long N, int Gx, int Gy, int Gz, long long capacity);

int lgm_mesh_density_count(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz, const float *lo,
                           const float *h, float cutoff, void *ws, size_t ws_bytes, long long *npairs, void *stream,
                           const lgm_diag *diag);

int lgm_mesh_density(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz, const float *lo,
                     const float *h, float cutoff, long long capacity, float *sigma, float *rgb, void *ws,
                     size_t ws_bytes, void *stream, const lgm_diag *diag);

/* bytes of the sampling workspace for N Gaussians and M points (the count call: M = 0, capacity = 0); 0 on invalid
 * sizes */
size_t lgm_mesh_sample_workspace_size(long long N, long long M, int Gx, int Gy, int Gz, long long capacity);

int lgm_mesh_sample_count(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz, const float *lo,
                          const float *h, float cutoff, void *ws, size_t ws_bytes, long long *npairs, void *stream,
                          const lgm_diag *diag);

int lgm_mesh_sample(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz, const float *lo,
                    const float *h, float cutoff, long long capacity, const float *points, long long M, float *sigma,
                    float *rgb, void *ws, size_t ws_bytes, void *stream, const lgm_diag *diag);

int lgm_mesh_atlas(const float *vertices, long long nv, const int *faces, long long nf, int T, int cols, int rows,
                   float *points, float *uvs, int *face_uvs, void *stream, const lgm_diag *diag);

/* bytes of the extraction workspace (shared by lgm_mesh_count and lgm_mesh_emit); 0 on invalid sizes */
size_t lgm_mesh_extract_workspace_size(int Gx, int Gy, int Gz);

int lgm_mesh_count(const float *sigma, int Gx, int Gy, int Gz, float iso, void *ws, size_t ws_bytes, long long *counts,
                   void *stream, const lgm_diag *diag);

int lgm_mesh_emit(const float *sigma, const float *rgb, int Gx, int Gy, int Gz, const float *lo, const float *h,
                  float iso, const void *ws, size_t ws_bytes, long long nv, long long nf, float *vertices, float *colors,
                  int *faces, long long cap_v, long long cap_f, void *stream, const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
