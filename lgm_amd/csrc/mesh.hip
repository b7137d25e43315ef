// lgm_amd/csrc/mesh.hip -- mesh export of include/lgm_mesh.h: the Gaussians' density and colour on a regular grid, and
// naive surface nets on that grid.
//
//   k_mesh_bin_count   per Gaussian: its 64-byte record (fp64 arithmetic, rounded once), its box in bricks, one integer
//                      atomic per brick the box touches
//   k_mesh_scan_reduce / k_mesh_scan_top / k_mesh_scan_add
//                      plain three-pass exclusive scan of an int array in place (tile sums, one workgroup over the tile
//                      sums, tiles again); no workgroup waits for another
//   k_mesh_bin_fill    per Gaussian: its index into the list of every brick of its box (atomic cursor: any order)
//   k_mesh_density     one workgroup per brick of 8^3 nodes, two nodes per thread: puts the brick's list in ascending
//                      order in LDS (rank sort up to 256 entries, bitonic up to LGM_MESH_SORT_CAP; longer lists are not
//                      read: the workgroup walks all N boxes in order instead), stages 64 records at a time through
//                      LDS and accumulates sum w and sum w c in fp32 in that order
//   k_mesh_sample_bin_count / k_mesh_point_count / k_mesh_point_fill / k_mesh_sample
//                      the same field at arbitrary points: the Gaussians binned over continuous brick intervals, the
//                      points binned into bricks, one workgroup per brick walking its points 256 at a time against
//                      its list (the list ordering and record staging are the device functions k_mesh_density uses)
//   k_mesh_atlas       per texel of a per-quad T x T atlas: its point on the drawn triangle; per quad: its uvs
//   k_mesh_classify    per node: the active flag of the cell it is the lowest corner of, and its triangle count
//   k_mesh_emit        per node: the vertex and colour of its cell and the triangles of its three grid edges
//
// Integer atomics only; every float sum has a fixed order, so two calls are bitwise equal.
#include "common.h"
#include "lgm_mesh.h"

namespace lgm {
namespace {

constexpr int BR = LGM_MESH_BRICK;
constexpr int THREADS = 256;
#ifdef LGM_MESH_SCAN_ALL  // A/B build: no brick reads its list, every brick walks all boxes
constexpr int SORT_CAP = -1;
#else
constexpr int SORT_CAP = LGM_MESH_SORT_CAP;
#endif
constexpr int SORT_LDS = LGM_MESH_SORT_CAP;
constexpr int RANK_CAP = 256;   // lists up to this length: one rank-sort step instead of the bitonic network
constexpr int REC_CHUNK = 64;   // records staged per step: 64 x 64 B
constexpr int REC_F4 = 4;       // float4 per record
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = THREADS * SCAN_ITEMS;
constexpr int TOP_THREADS = 1024;
constexpr long long I31 = 2147483648LL;
static_assert(BR == 8 && THREADS == BR * BR * BR / 2, "two nodes per thread");
static_assert(RANK_CAP <= THREADS && 2 * RANK_CAP <= SORT_LDS, "rank sort: one entry per thread, staged in the upper half");

struct Grid {
    int G[3];   // nodes per axis
    int nb[3];  // bricks per axis
    float lo[3], h[3];
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028235e38f; }  // (false for NaN)

// ---------------------------------------------------------------------------------------------------- binning
// record: mu (3), A' = sqrt(log2(e) / 2) diag(s)^-1 R^T row-major (9), log2 o, rgb (3).  box: brick ranges
// [x0, x1, y0, y1, z0, z1, -, -], inclusive; x0 > x1: touches nothing.
// SAMPLE: the boxes of the sampling pass, over continuous intervals (brick b owns [b BR, (b + 1) BR) in node units, the
// first one from -1/2 and the last one to G - 1/2), so that a point between two nodes finds every Gaussian that reaches it
template <bool SAMPLE>
__device__ __forceinline__ void bin_count(const float *__restrict__ g, int N, float mod, const Grid &gr, float cutoff,
                                          float4 *__restrict__ rec, int4 *__restrict__ box, int *__restrict__ cnt) {
    const int n = blockIdx.x * THREADS + threadIdx.x;
    if (n >= N) return;
    float f[14];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        f[i] = g[(size_t)n * 14 + i];
        ok = ok && finite_f(f[i]);
    }
    const double o = f[3];
    const double s[3] = {(double)mod * f[4], (double)mod * f[5], (double)mod * f[6]};
    const double qn2 = (double)f[7] * f[7] + (double)f[8] * f[8] + (double)f[9] * f[9] + (double)f[10] * f[10];
    ok = ok && f[3] > cutoff && s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0 && qn2 > 0.0;
    int b0[3] = {1, 1, 1}, b1[3] = {0, 0, 0};
    float4 r4[REC_F4] = {};
    if (ok) {
        const double qi = 1.0 / sqrt(qn2);
        const double r = f[7] * qi, x = f[8] * qi, y = f[9] * qi, z = f[10] * qi;
        const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)},
                                {2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)},
                                {2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)}};
        const double pre = 0.84932180028801904272;  // sqrt(log2(e) / 2): d2' = d2 log2(e) / 2
        float A[9];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int a = 0; a < 3; a++) A[k * 3 + a] = (float)(pre * R[a][k] / s[k]);
        r4[0] = make_float4(f[0], f[1], f[2], A[0]);
        r4[1] = make_float4(A[1], A[2], A[3], A[4]);
        r4[2] = make_float4(A[5], A[6], A[7], A[8]);
        r4[3] = make_float4((float)log2(o), f[11], f[12], f[13]);
        // the box, a little wide (it only has to contain the ellipsoid d2 <= rho2: the kernel tests every node)
        const double rho = sqrt(2.0 * log(o / (double)cutoff));
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double e0 = R[a][0] * s[0], e1 = R[a][1] * s[1], e2 = R[a][2] * s[2];
            const double ext = rho * sqrt(e0 * e0 + e1 * e1 + e2 * e2) * (1.0 + 1e-6);
            const double c = (double)f[a] - (double)gr.lo[a], hh = gr.h[a], top = gr.G[a] - 1;
            const double edge = SAMPLE ? 0.5 : 0.0;
            const double i0 = fmax((c - ext) / hh - 1e-3, -edge), i1 = fmin((c + ext) / hh + 1e-3, top + edge);
            if (SAMPLE && i0 <= i1) {  // (false for NaN too)
                b0[a] = (int)floor(fmax(i0, 0.0)) / BR;
                b1[a] = (int)floor(fmax(i1, 0.0)) / BR;  // (i1 <= G - 1/2: at most the last brick)
            } else if (!SAMPLE && i0 <= i1 && ceil(i0) <= floor(i1)) {
                b0[a] = (int)ceil(i0) / BR;
                b1[a] = (int)floor(i1) / BR;
            } else {
                b0[0] = 1, b1[0] = 0;
                break;
            }
        }
        if (b0[0] > b1[0] || b0[1] > b1[1] || b0[2] > b1[2]) b0[0] = 1, b1[0] = 0;
    }
#pragma unroll
    for (int q = 0; q < REC_F4; q++) rec[(size_t)n * REC_F4 + q] = r4[q];
    box[2 * (size_t)n] = make_int4(b0[0], b1[0], b0[1], b1[1]);
    box[2 * (size_t)n + 1] = make_int4(b0[2], b1[2], 0, 0);
    if (b0[0] > b1[0]) return;
    for (int bx = b0[0]; bx <= b1[0]; bx++)
        for (int by = b0[1]; by <= b1[1]; by++)
            for (int bz = b0[2]; bz <= b1[2]; bz++) atomicAdd(&cnt[(bx * gr.nb[1] + by) * gr.nb[2] + bz], 1);
}

__global__ __launch_bounds__(THREADS) void k_mesh_bin_count(const float *__restrict__ g, int N, float mod, Grid gr,
                                                            float cutoff, float4 *__restrict__ rec,
                                                            int4 *__restrict__ box, int *__restrict__ cnt) {
    bin_count<false>(g, N, mod, gr, cutoff, rec, box, cnt);
}

__global__ __launch_bounds__(THREADS) void k_mesh_sample_bin_count(const float *__restrict__ g, int N, float mod, Grid gr,
                                                                   float cutoff, float4 *__restrict__ rec,
                                                                   int4 *__restrict__ box, int *__restrict__ cnt) {
    bin_count<true>(g, N, mod, gr, cutoff, rec, box, cnt);
}

__global__ __launch_bounds__(THREADS) void k_mesh_bin_fill(int N, Grid gr, const int4 *__restrict__ box,
                                                           const int *__restrict__ offs, int *__restrict__ cur,
                                                           int *__restrict__ lists, long long capacity) {
    const int n = blockIdx.x * THREADS + threadIdx.x;
    if (n >= N) return;
    const int4 bxy = box[2 * (size_t)n], bz_ = box[2 * (size_t)n + 1];
    if (bxy.x > bxy.y) return;
    for (int bx = bxy.x; bx <= bxy.y; bx++)
        for (int by = bxy.z; by <= bxy.w; by++)
            for (int bz = bz_.x; bz <= bz_.y; bz++) {
                const int b = (bx * gr.nb[1] + by) * gr.nb[2] + bz;
                const long long at = (long long)offs[b] + atomicAdd(&cur[b], 1);
                if (offs[b] >= 0 && at < capacity) lists[at] = n;  // (a short capacity: k_mesh_density poisons)
            }
}

// ---------------------------------------------------------------------------------------------------- scan
// exclusive scan over the workgroup (shuffles up inside a wave, wave totals through LDS); total: the sum of all
template <int T>
__device__ __forceinline__ long long block_excl_scan(long long v, long long *red, long long &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    __syncthreads();  // (red may still be read from the previous use)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < T / 64; w++) {
        const long long s = red[w];
        if (w < wave) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(THREADS) void k_mesh_scan_reduce(const int *__restrict__ a, long long n,
                                                              long long *__restrict__ bsum) {
    __shared__ long long red[THREADS / 64];
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    long long s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++)
        if (base + i < n) s += a[base + i];
    long long total;
    block_excl_scan<THREADS>(s, red, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(TOP_THREADS) void k_mesh_scan_top(long long *__restrict__ bsum, long long nb,
                                                               long long *__restrict__ total_out) {
    __shared__ long long red[TOP_THREADS / 64];
    long long carry = 0;
    for (long long base = 0; base < nb; base += TOP_THREADS) {
        const long long i = base + threadIdx.x;
        const long long v = i < nb ? bsum[i] : 0;
        long long total;
        const long long ex = block_excl_scan<TOP_THREADS>(v, red, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(THREADS) void k_mesh_scan_add(int *__restrict__ a, long long n,
                                                           const long long *__restrict__ bsum) {
    __shared__ long long red[THREADS / 64];
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    long long s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        v[i] = base + i < n ? a[base + i] : 0;
        s += v[i];
    }
    long long total;
    long long run = bsum[blockIdx.x] + block_excl_scan<THREADS>(s, red, total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        if (base + i < n) a[base + i] = (int)run;  // (meaningful while the grand total is below 2^31: the host checks)
        run += v[i];
    }
}

// ---------------------------------------------------------------------------------------------------- density
struct NodeAcc {
    float w, r, g, b;
};

// The three steps k_mesh_density and k_mesh_sample share. Every thread of the workgroup calls them (barriers inside).
//
// s_list[0 .. L) = src[0 .. L) in ascending order, L <= LGM_MESH_SORT_CAP. Returns without a barrier: for_each_record
// begins with one.
__device__ __forceinline__ void order_list(const int *__restrict__ src, int L, int *s_list) {
    const int tid = threadIdx.x;
    if (L <= RANK_CAP) {
        // rank sort: the indices of a list are distinct, so the number of smaller ones is the place
        int *tmp = s_list + RANK_CAP;
        const int v = tid < L ? src[tid] : 0x7fffffff;
        tmp[tid] = v;
        __syncthreads();
        if (tid < L) {
            int rank = 0;
            for (int i = 0; i < L; i++) rank += tmp[i] < v;
            s_list[rank] = v;
        }
    } else {
        int P = RANK_CAP * 2;
        while (P < L) P <<= 1;
        for (int i = tid; i < P; i += THREADS) s_list[i] = i < L ? src[i] : 0x7fffffff;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const int u = s_list[i], v = s_list[p];
                        if ((u > v) == ((i & k) == 0)) s_list[i] = v, s_list[p] = u;
                    }
                }
                __syncthreads();
            }
    }
}

// a list longer than LDS: of the 256 boxes from `base` on, those that touch brick (bx, by, bz) go to s_list in
// ascending order; returns their number
__device__ __forceinline__ int gather_window(const int4 *__restrict__ box, int N, int base, int bx, int by, int bz,
                                             int *s_list, int *s_wcnt) {
    const int tid = threadIdx.x;
    const int n = base + tid;
    bool hit = false;
    if (n < N) {
        const int4 bxy = box[2 * (size_t)n], bz_ = box[2 * (size_t)n + 1];
        hit = bxy.x <= bx && bx <= bxy.y && bxy.z <= by && by <= bxy.w && bz_.x <= bz && bz <= bz_.y;
    }
    const unsigned long long mask = __ballot(hit);
    __syncthreads();  // (s_wcnt and s_list of the previous window are no longer read)
    if ((tid & 63) == 0) s_wcnt[tid >> 6] = __popcll(mask);
    __syncthreads();
    int before = 0, count = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) {
        const int c = s_wcnt[w];
        if (w < (tid >> 6)) before += c;
        count += c;
    }
    if (hit) s_list[before + __popcll(mask & ((1ull << (tid & 63)) - 1ull))] = n;
    return count;
}

// term(p0, p1, p2, p3) for the records of the Gaussians s_list[0 .. count), in that order, staged 64 at a time through
// s_rec with mu replaced by (ox, oy, oz) - mu, taken in fp64 and rounded once
template <class Term>
__device__ __forceinline__ void for_each_record(const float4 *__restrict__ rec, const int *s_list, int count, double ox,
                                                double oy, double oz, float4 *s_rec, Term &&term) {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < count; c0 += REC_CHUNK) {
        const int m = min(REC_CHUNK, count - c0);
        __syncthreads();  // s_list is written; the previous chunk's records are consumed
        if ((tid >> 2) < m) {
            const int q = tid & 3;
            float4 v = rec[(size_t)s_list[c0 + (tid >> 2)] * REC_F4 + q];
            if (q == 0) {
                v.x = (float)(ox - (double)v.x);
                v.y = (float)(oy - (double)v.y);
                v.z = (float)(oz - (double)v.z);
            }
            s_rec[(tid >> 2) * REC_F4 + q] = v;
        }
        __syncthreads();
        for (int r = 0; r < m; r++)
            term(s_rec[r * REC_F4], s_rec[r * REC_F4 + 1], s_rec[r * REC_F4 + 2], s_rec[r * REC_F4 + 3]);
    }
}

__global__ __launch_bounds__(THREADS) void k_mesh_density(Grid gr, int N, const float4 *__restrict__ rec,
                                                          const int4 *__restrict__ box, const int *__restrict__ offs,
                                                          const int *__restrict__ cur, const int *__restrict__ lists,
                                                          const long long *__restrict__ total, long long capacity,
                                                          float log2eps, float *__restrict__ sigma,
                                                          float *__restrict__ rgb) {
    __shared__ int s_list[SORT_LDS];
    __shared__ float4 s_rec[REC_CHUNK * REC_F4];
    __shared__ int s_wcnt[THREADS / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int bz = b % gr.nb[2], by = (b / gr.nb[2]) % gr.nb[1], bx = b / (gr.nb[2] * gr.nb[1]);
    const int li = tid >> 6, lj = (tid >> 3) & 7, lk = tid & 7;  // this thread's nodes: (li, lj, lk) and (li + 4, lj, lk)
    // the brick's first node, in fp64 (a record's mu is subtracted from it before anything is rounded to fp32)
    const double ox = (double)gr.lo[0] + (double)(bx * BR) * (double)gr.h[0];
    const double oy = (double)gr.lo[1] + (double)(by * BR) * (double)gr.h[1];
    const double oz = (double)gr.lo[2] + (double)(bz * BR) * (double)gr.h[2];
    const float fi0 = (float)li, fi1 = (float)(li + 4), fj = (float)lj, fk = (float)lk;
    NodeAcc acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const bool poison = *total > capacity;  // (uniform)

    // one Gaussian's term at the thread's two nodes
    auto term = [&](const float4 p0, const float4 p1, const float4 p2, const float4 p3) {
        const float dy = fmaf(fj, gr.h[1], p0.y), dz = fmaf(fk, gr.h[2], p0.z);
        // the part of y that the thread's two nodes share
        const float c0y = fmaf(p1.y, dz, p1.x * dy);  // row 0: A01 dy + A02 dz
        const float c1y = fmaf(p2.x, dz, p1.w * dy);  // row 1: A11 dy + A12 dz
        const float c2y = fmaf(p2.w, dz, p2.z * dy);  // row 2: A21 dy + A22 dz
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const float dx = fmaf(k ? fi1 : fi0, gr.h[0], p0.x);
            const float y0 = fmaf(p0.w, dx, c0y), y1 = fmaf(p1.z, dx, c1y), y2 = fmaf(p2.y, dx, c2y);
            const float e = p3.x - fmaf(y2, y2, fmaf(y1, y1, y0 * y0));
            if (e >= log2eps) {
                const float w = __builtin_amdgcn_exp2f(e);
                acc[k].w += w;
                acc[k].r = fmaf(w, p3.y, acc[k].r);
                acc[k].g = fmaf(w, p3.z, acc[k].g);
                acc[k].b = fmaf(w, p3.w, acc[k].b);
            }
        }
    };

    const int L = cur[b];
    if (poison || L == 0) {
        // nothing to accumulate
    } else if (L <= SORT_CAP) {
        order_list(lists + (long long)offs[b], L, s_list);
        for_each_record(rec, s_list, L, ox, oy, oz, s_rec, term);
    } else {
        // walk all boxes in ascending order, 256 at a time, and keep those that touch this brick
        for (int base = 0; base < N; base += THREADS) {
            const int count = gather_window(box, N, base, bx, by, bz, s_list, s_wcnt);
            for_each_record(rec, s_list, count, ox, oy, oz, s_rec, term);
        }
    }

    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = bx * BR + li + 4 * k, j = by * BR + lj, kk = bz * BR + lk;
        if (i >= gr.G[0] || j >= gr.G[1] || kk >= gr.G[2]) continue;
        const size_t at = ((size_t)i * gr.G[1] + j) * gr.G[2] + kk;
        const float s = acc[k].w;
        sigma[at] = poison ? qnan : s;
        if (rgb) {
            const bool has = s > 0.f;
            rgb[3 * at] = poison ? qnan : has ? acc[k].r / s : 0.f;
            rgb[3 * at + 1] = poison ? qnan : has ? acc[k].g / s : 0.f;
            rgb[3 * at + 2] = poison ? qnan : has ? acc[k].b / s : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- sampling
struct Domain {
    double lo[3], hi[3];  // lo - h / 2 and lo + (G - 1/2) h in fp64: the points that are sampled
};

// per point: its brick (-1: not sampled; such a point's outputs are written here), one integer atomic on that brick
__global__ __launch_bounds__(THREADS) void k_mesh_point_count(const float *__restrict__ pts, int M, Grid gr, Domain dom,
                                                              const long long *__restrict__ total, long long capacity,
                                                              int *__restrict__ pbrick, int *__restrict__ pcnt,
                                                              float *__restrict__ sigma, float *__restrict__ rgb) {
    const long long m = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    int bi[3];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float p = pts[3 * m + a];
        in = in && finite_f(p) && (double)p >= dom.lo[a] && (double)p <= dom.hi[a];
        const double u = ((double)p - (double)gr.lo[a]) / (double)gr.h[a];  // the fp64 node coordinate
        bi[a] = in ? min((int)floor(fmax(u, 0.0)), gr.G[a] - 1) / BR : 0;
    }
    int b = -1;
    if (in) {
        b = (bi[0] * gr.nb[1] + bi[1]) * gr.nb[2] + bi[2];
        atomicAdd(&pcnt[b], 1);
    } else {
        const float v = *total > capacity ? __builtin_nanf("") : 0.f;
        sigma[m] = v;
        if (rgb) rgb[3 * m] = v, rgb[3 * m + 1] = v, rgb[3 * m + 2] = v;
    }
    pbrick[m] = b;
}

__global__ __launch_bounds__(THREADS) void k_mesh_point_fill(int M, const int *__restrict__ pbrick,
                                                             const int *__restrict__ poffs, int *__restrict__ pcur,
                                                             int *__restrict__ plist) {
    const long long m = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    const int b = pbrick[m];
    if (b < 0) return;
    const long long at = (long long)poffs[b] + atomicAdd(&pcur[b], 1);
    if (at >= 0 && at < M) plist[at] = (int)m;  // (the sampled points are at most M: always true)
}

// one workgroup per brick: its points, 256 at a time and one per thread, against its list in ascending order
__global__ __launch_bounds__(THREADS) void k_mesh_sample(Grid gr, int N, const float4 *__restrict__ rec,
                                                         const int4 *__restrict__ box, const int *__restrict__ offs,
                                                         const int *__restrict__ cur, const int *__restrict__ lists,
                                                         const long long *__restrict__ total, long long capacity,
                                                         float log2eps, const float *__restrict__ pts,
                                                         const int *__restrict__ poffs, const int *__restrict__ pcur,
                                                         const int *__restrict__ plist, float *__restrict__ sigma,
                                                         float *__restrict__ rgb) {
    __shared__ int s_list[SORT_LDS];
    __shared__ float4 s_rec[REC_CHUNK * REC_F4];
    __shared__ int s_wcnt[THREADS / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int P = pcur[b];
    if (P == 0) return;  // (uniform)
    const int bz = b % gr.nb[2], by = (b / gr.nb[2]) % gr.nb[1], bx = b / (gr.nb[2] * gr.nb[1]);
    // the brick's first node, in fp64: a point and a record's mu are both subtracted from it before rounding to fp32
    const double ox = (double)gr.lo[0] + (double)(bx * BR) * (double)gr.h[0];
    const double oy = (double)gr.lo[1] + (double)(by * BR) * (double)gr.h[1];
    const double oz = (double)gr.lo[2] + (double)(bz * BR) * (double)gr.h[2];
    const bool poison = *total > capacity;  // (uniform)
    const int L = cur[b];
    const bool walk = !poison && L > 0 && L > SORT_CAP;
    if (!poison && L > 0 && !walk) order_list(lists + (long long)offs[b], L, s_list);
    const long long first = poffs[b];
    const float qnan = __builtin_nanf("");

    for (int p0 = 0; p0 < P; p0 += THREADS) {
        const int m = p0 + tid < P ? plist[first + p0 + tid] : -1;
        float lx = 0.f, ly = 0.f, lz = 0.f;
        if (m >= 0) {
            lx = (float)((double)pts[3 * (size_t)m] - ox);
            ly = (float)((double)pts[3 * (size_t)m + 1] - oy);
            lz = (float)((double)pts[3 * (size_t)m + 2] - oz);
        }
        NodeAcc acc = {0.f, 0.f, 0.f, 0.f};
        // one Gaussian's term at the thread's point: k_mesh_density's, with the point in the place of the node
        auto term = [&](const float4 q0, const float4 q1, const float4 q2, const float4 q3) {
            const float dx = lx + q0.x, dy = ly + q0.y, dz = lz + q0.z;
            const float y0 = fmaf(q0.w, dx, fmaf(q1.y, dz, q1.x * dy));
            const float y1 = fmaf(q1.z, dx, fmaf(q2.x, dz, q1.w * dy));
            const float y2 = fmaf(q2.y, dx, fmaf(q2.w, dz, q2.z * dy));
            const float e = q3.x - fmaf(y2, y2, fmaf(y1, y1, y0 * y0));
            if (e >= log2eps) {
                const float w = __builtin_amdgcn_exp2f(e);
                acc.w += w;
                acc.r = fmaf(w, q3.y, acc.r);
                acc.g = fmaf(w, q3.z, acc.g);
                acc.b = fmaf(w, q3.w, acc.b);
            }
        };
        if (walk) {
            for (int base = 0; base < N; base += THREADS) {
                const int count = gather_window(box, N, base, bx, by, bz, s_list, s_wcnt);
                for_each_record(rec, s_list, count, ox, oy, oz, s_rec, term);
            }
        } else if (!poison && L > 0) {
            for_each_record(rec, s_list, L, ox, oy, oz, s_rec, term);
        }
        if (m < 0) continue;
        const float s = acc.w;
        sigma[m] = poison ? qnan : s;
        if (rgb) {
            const bool has = s > 0.f;
            rgb[3 * (size_t)m] = poison ? qnan : has ? acc.r / s : 0.f;
            rgb[3 * (size_t)m + 1] = poison ? qnan : has ? acc.g / s : 0.f;
            rgb[3 * (size_t)m + 2] = poison ? qnan : has ? acc.b / s : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- atlas
// one thread per texel: block q of T x T texels for the quad of faces 2q and 2q + 1
__global__ __launch_bounds__(THREADS) void k_mesh_atlas(const float *__restrict__ vertices, long long nv,
                                                        const int *__restrict__ faces, long long nq, int T, int cols,
                                                        int rows, float *__restrict__ points, float *__restrict__ uvs,
                                                        int *__restrict__ face_uvs) {
// every fp32 operation is rounded on its own (include/lgm_mesh.h)
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (n >= nq * T * T) return;
    const long long q = n / (T * T);
    const int r = (int)(n % (T * T)), j = r / T, i = r % T;
    const int *f = faces + 6 * q;
    const int a = f[0], b = f[1], c = f[2], a2 = f[3], d = f[4], e = f[5];
    // outward (q0, q1, q2), (q0, q2, q3): c == d; flipped (q0, q2, q1), (q0, q3, q2): b == e
    const bool outward = c == d, flipped = !outward && b == e;
    const int q0 = a, q1 = outward ? b : c, q2 = outward ? c : b, q3 = outward ? e : d;
    const bool ok = a == a2 && (outward || flipped) && q0 >= 0 && q0 < nv && q1 >= 0 && q1 < nv && q2 >= 0 &&
                    q2 < nv && q3 >= 0 && q3 < nv;
    const float s = (float)i / (float)(T - 1), t = (float)j / (float)(T - 1);
    float *out = points + 3 * n;
    if (ok) {
        const bool up = s >= t;
        const float w0 = up ? 1.f - s : 1.f - t, w1 = up ? s - t : t - s, w2 = up ? t : s;
        const float *v0 = vertices + 3 * (size_t)q0, *v1 = vertices + 3 * (size_t)(up ? q1 : q3),
                    *v2 = vertices + 3 * (size_t)q2;
#pragma unroll
        for (int k = 0; k < 3; k++) out[k] = w0 * v0[k] + w1 * v1[k] + w2 * v2[k];
    } else {
        out[0] = out[1] = out[2] = __builtin_nanf("");
    }
    if (r != 0) return;
    const float x0 = (float)((q % cols) * T), y0 = (float)((q / cols) * T), W = (float)(cols * T), H = (float)(rows * T);
#pragma unroll
    for (int k = 0; k < 4; k++) {  // q0, q1, q2, q3: corners (0, 0), (1, 0), (1, 1), (0, 1)
        const int ca = (k == 1 || k == 2), cb = k >> 1;
        const float x = x0 + 0.5f + (float)(ca * (T - 1)), y = y0 + 0.5f + (float)(cb * (T - 1));
        uvs[8 * q + 2 * k] = x / W;
        uvs[8 * q + 2 * k + 1] = 1.f - y / H;
    }
    const int u0 = (int)(4 * q);
    int *fu = face_uvs + 6 * q;
    if (!flipped) {
        fu[0] = u0, fu[1] = u0 + 1, fu[2] = u0 + 2, fu[3] = u0, fu[4] = u0 + 2, fu[5] = u0 + 3;
    } else {
        fu[0] = u0, fu[1] = u0 + 2, fu[2] = u0 + 1, fu[3] = u0, fu[4] = u0 + 3, fu[5] = u0 + 2;
    }
}

// ---------------------------------------------------------------------------------------------------- extraction
// the sample at node (i, j, k) as the extraction reads it
__device__ __forceinline__ float sample(const float *__restrict__ sigma, const Grid &gr, int i, int j, int k) {
    if (i <= 0 || j <= 0 || k <= 0 || i >= gr.G[0] - 1 || j >= gr.G[1] - 1 || k >= gr.G[2] - 1) return 0.f;
    const float v = sigma[((size_t)i * gr.G[1] + j) * gr.G[2] + k];
    return finite_f(v) ? v : 0.f;
}

__global__ __launch_bounds__(THREADS) void k_mesh_classify(const float *__restrict__ sigma, Grid gr, float iso,
                                                           int *__restrict__ vflag, int *__restrict__ fcnt) {
    const long long n = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (n >= (long long)gr.G[0] * gr.G[1] * gr.G[2]) return;
    const int k = (int)(n % gr.G[2]), j = (int)((n / gr.G[2]) % gr.G[1]), i = (int)(n / ((long long)gr.G[2] * gr.G[1]));
    const bool in0 = sample(sigma, gr, i, j, k) >= iso;
    const bool inx = i + 1 < gr.G[0] && sample(sigma, gr, i + 1, j, k) >= iso;
    const bool iny = j + 1 < gr.G[1] && sample(sigma, gr, i, j + 1, k) >= iso;
    const bool inz = k + 1 < gr.G[2] && sample(sigma, gr, i, j, k + 1) >= iso;
    // (a node past the grid counts as outside, and so does the boundary layer: an edge leaving the grid never differs)
    fcnt[n] = 2 * ((int)(in0 != inx) + (int)(in0 != iny) + (int)(in0 != inz));
    if (i < gr.G[0] - 1 && j < gr.G[1] - 1 && k < gr.G[2] - 1) {
        int m = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) m += sample(sigma, gr, i + (c >> 2), j + ((c >> 1) & 1), k + (c & 1)) >= iso;
        vflag[((size_t)i * (gr.G[1] - 1) + j) * (gr.G[2] - 1) + k] = m != 0 && m != 8;
    }
}

__global__ __launch_bounds__(THREADS) void k_mesh_emit(const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                       Grid gr, float iso, const int *__restrict__ vpre,
                                                       const int *__restrict__ fpre, float *__restrict__ vertices,
                                                       float *__restrict__ colors, int *__restrict__ faces,
                                                       long long cap_v, long long cap_f) {
// every fp32 operation of the vertex and colour means is rounded on its own (include/lgm_mesh.h)
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (n >= (long long)gr.G[0] * gr.G[1] * gr.G[2]) return;
    const int k = (int)(n % gr.G[2]), j = (int)((n / gr.G[2]) % gr.G[1]), i = (int)(n / ((long long)gr.G[2] * gr.G[1]));
    const int C1 = gr.G[1] - 1, C2 = gr.G[2] - 1;
    float s[8];
    int m = 0;
    const bool cell = i < gr.G[0] - 1 && j < C1 && k < C2;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        s[c] = sample(sigma, gr, i + (c >> 2), j + ((c >> 1) & 1), k + (c & 1));  // (0 past the grid)
        m += s[c] >= iso;
    }
    if (cell && m != 0 && m != 8) {
        const long long vid = vpre[((size_t)i * C1 + j) * C2 + k];
        // the 12 edges in the header's order: lower corner, axis (upper corner = lower + (4 >> axis))
        constexpr int EA[12] = {0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6};
        constexpr int EX[12] = {2, 1, 0, 1, 0, 2, 0, 0, 2, 1, 1, 2};
        float p[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < 12; e++) {
            const int a = EA[e], ax = EX[e], bq = a + (4 >> ax);
            const bool ia = s[a] >= iso, ib = s[bq] >= iso;
            if (ia == ib) continue;
            const float t = (iso - s[a]) / (s[bq] - s[a]);
            float off[3] = {(float)(a >> 2), (float)((a >> 1) & 1), (float)(a & 1)};
            off[ax] = t;  // (the lower corner's offset on its edge's axis is 0)
            p[0] += off[0], p[1] += off[1], p[2] += off[2];
            if (rgb) {
                const int q = ia ? a : bq;
                const size_t at = ((size_t)(i + (q >> 2)) * gr.G[1] + (j + ((q >> 1) & 1))) * gr.G[2] + (k + (q & 1));
                col[0] += rgb[3 * at], col[1] += rgb[3 * at + 1], col[2] += rgb[3 * at + 2];
            }
            cnt++;
        }
        if (vid >= 0 && vid < cap_v) {
            const float fc = (float)cnt;
            const float px = (float)i + p[0] / fc, py = (float)j + p[1] / fc, pz = (float)k + p[2] / fc;
            vertices[3 * vid] = gr.lo[0] + px * gr.h[0];
            vertices[3 * vid + 1] = gr.lo[1] + py * gr.h[1];
            vertices[3 * vid + 2] = gr.lo[2] + pz * gr.h[2];
            if (rgb) colors[3 * vid] = col[0] / fc, colors[3 * vid + 1] = col[1] / fc, colors[3 * vid + 2] = col[2] / fc;
        }
    }
    // the triangles of the grid edges n -> n + e_a. A differing edge has an endpoint off the boundary layer, so n is
    // at least 1 and at most G - 2 on the two other axes, and at most G - 2 on a: the four cells exist.
    const bool in0 = s[0] >= iso;
    long long f = fpre[n];
    const int nn[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (nn[a] + 1 >= gr.G[a]) continue;
        const bool in1 = sample(sigma, gr, i + (a == 0), j + (a == 1), k + (a == 2)) >= iso;
        if (in0 == in1) continue;
        const int bA = (a + 1) % 3, cA = (a + 2) % 3;
        int q[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            int c[3] = {i, j, k};
            if (v == 0 || v == 3) c[bA] -= 1;
            if (v == 0 || v == 1) c[cA] -= 1;
            q[v] = vpre[((size_t)c[0] * C1 + c[1]) * C2 + c[2]];
        }
        if (f >= 0 && f + 1 < cap_f) {
            int *o = faces + 3 * f;
            if (in0) {
                o[0] = q[0], o[1] = q[1], o[2] = q[2], o[3] = q[0], o[4] = q[2], o[5] = q[3];
            } else {
                o[0] = q[0], o[1] = q[2], o[2] = q[1], o[3] = q[0], o[4] = q[3], o[5] = q[2];
            }
        }
        f += 2;
    }
}

// ---------------------------------------------------------------------------------------------------- host
bool fin(double x) { return x - x == 0.0; }
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
long long tiles_of(long long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

bool grid_ok(int Gx, int Gy, int Gz) {
    return Gx >= 3 && Gy >= 3 && Gz >= 3 && (double)Gx * Gy * Gz < 2147483648.0;
}

// 0 and gr filled, or < 0 with the error set
int make_grid(const char *who, int Gx, int Gy, int Gz, const float *lo, const float *h, bool need_geometry, Grid &gr) {
    if (!grid_ok(Gx, Gy, Gz)) {
        set_error("%s: grid %d x %d x %d: every axis must be >= 3 and the node count below 2^31", who, Gx, Gy, Gz);
        return LGM_E_INVALID;
    }
    gr.G[0] = Gx, gr.G[1] = Gy, gr.G[2] = Gz;
    for (int a = 0; a < 3; a++) {
        gr.nb[a] = (gr.G[a] + BR - 1) / BR;
        gr.lo[a] = 0.f, gr.h[a] = 1.f;
    }
    if (!need_geometry) return LGM_OK;
    if (!lo || !h) {
        set_error("%s: null pointer (lo, h)", who);
        return LGM_E_INVALID;
    }
    for (int a = 0; a < 3; a++) {
        if (!fin(lo[a]) || !fin(h[a]) || !(h[a] > 0.f)) {
            set_error("%s: lo[%d]=%g h[%d]=%g: lo must be finite, h finite and positive", who, a, lo[a], a, h[a]);
            return LGM_E_INVALID;
        }
        gr.lo[a] = lo[a], gr.h[a] = h[a];
    }
    return LGM_OK;
}

// (M >= 0: the sampling pass's workspace, with the arrays of its M points after the lists)
struct DensityLayout {
    size_t rec, box, cnt, cur, bsum, total, lists, pcnt, pcur, pbsum, ptotal, pbrick, plist, bytes;
    long long nbricks;
};
DensityLayout density_layout(long long N, const Grid &gr, long long capacity, long long M = -1) {
    DensityLayout L;
    L.nbricks = (long long)gr.nb[0] * gr.nb[1] * gr.nb[2];
    size_t at = 0;
    L.rec = at, at += up256((size_t)N * REC_F4 * sizeof(float4));
    L.box = at, at += up256((size_t)N * 2 * sizeof(int4));
    L.cnt = at, at += up256((size_t)L.nbricks * sizeof(int));
    L.cur = at, at += up256((size_t)L.nbricks * sizeof(int));
    L.bsum = at, at += up256((size_t)tiles_of(L.nbricks) * sizeof(long long));
    L.total = at, at += 256;
    L.lists = at, at += up256((size_t)capacity * sizeof(int));
    L.pcnt = L.pcur = L.pbsum = L.ptotal = L.pbrick = L.plist = at;
    if (M >= 0) {
        L.pcnt = at, at += up256((size_t)L.nbricks * sizeof(int));
        L.pcur = at, at += up256((size_t)L.nbricks * sizeof(int));
        L.pbsum = at, at += up256((size_t)tiles_of(L.nbricks) * sizeof(long long));
        L.ptotal = at, at += 256;
        L.pbrick = at, at += up256((size_t)M * sizeof(int));
        L.plist = at, at += up256((size_t)M * sizeof(int));
    }
    L.bytes = at;
    return L;
}

int scan_in_place(int *a, long long n, long long *bsum, long long *total, hipStream_t st) {
    const long long nt = tiles_of(n);
    LGM_LAUNCH("k_mesh_scan_reduce", st, (k_mesh_scan_reduce<<<(unsigned)nt, THREADS, 0, st>>>(a, n, bsum)));
    LGM_LAUNCH("k_mesh_scan_top", st, (k_mesh_scan_top<<<1, TOP_THREADS, 0, st>>>(bsum, nt, total)));
    LGM_LAUNCH("k_mesh_scan_add", st, (k_mesh_scan_add<<<(unsigned)nt, THREADS, 0, st>>>(a, n, bsum)));
    return LGM_OK;
}

// the checks and the passes lgm_mesh_density_count and lgm_mesh_density share: records, boxes, brick counts, scan
// (the total goes to total_dst, or into the workspace when that is null). M >= 0: the sampling pass, whose boxes are
// k_mesh_sample_bin_count's
int density_front(const char *who, const float *g, long long N, float mod, int Gx, int Gy, int Gz, const float *lo,
                  const float *h, float cutoff, long long capacity, void *ws, size_t ws_bytes, Grid &gr,
                  DensityLayout &L, long long *total_dst, hipStream_t st, long long M = -1) {
    const int rc = make_grid(who, Gx, Gy, Gz, lo, h, true, gr);
    if (rc) return rc;
    if (N < 0 || N >= I31 || capacity < 0 || capacity >= I31) {
        set_error("%s: N=%lld capacity=%lld: both must be in [0, 2^31)", who, N, capacity);
        return LGM_E_INVALID;
    }
    if (!fin(mod) || !fin(cutoff) || !(cutoff > 0.f)) {
        set_error("%s: scale_modifier=%g cutoff=%g: both must be finite, cutoff positive", who, mod, cutoff);
        return LGM_E_INVALID;
    }
    if ((N > 0 && !g) || !ws) {
        set_error("%s: null pointer (g, ws)", who);
        return LGM_E_INVALID;
    }
    L = density_layout(N, gr, capacity, M);
    if (ws_bytes < L.bytes) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.bytes);
        return LGM_E_WORKSPACE;
    }
    char *w = (char *)ws;
    if (hipMemsetAsync(w + L.cnt, 0, L.bsum - L.cnt, st) != hipSuccess) {  // (the counts and the cursors)
        set_error("%s: hipMemsetAsync failed", who);
        return LGM_E_HIP;
    }
    if (N > 0 && M < 0)
        LGM_LAUNCH("k_mesh_bin_count", st,
                   (k_mesh_bin_count<<<(unsigned)((N + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                       g, (int)N, mod, gr, cutoff, (float4 *)(w + L.rec), (int4 *)(w + L.box), (int *)(w + L.cnt))));
    if (N > 0 && M >= 0)
        LGM_LAUNCH("k_mesh_sample_bin_count", st,
                   (k_mesh_sample_bin_count<<<(unsigned)((N + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                       g, (int)N, mod, gr, cutoff, (float4 *)(w + L.rec), (int4 *)(w + L.box), (int *)(w + L.cnt))));
    return scan_in_place((int *)(w + L.cnt), L.nbricks, (long long *)(w + L.bsum),
                         total_dst ? total_dst : (long long *)(w + L.total), st);
}

struct ExtractLayout {
    size_t vpre, fpre, bsumv, bsumf, bytes;
    long long ncells, nnodes;
};
ExtractLayout extract_layout(const Grid &gr) {
    ExtractLayout L;
    L.ncells = (long long)(gr.G[0] - 1) * (gr.G[1] - 1) * (gr.G[2] - 1);
    L.nnodes = (long long)gr.G[0] * gr.G[1] * gr.G[2];
    size_t at = 0;
    L.vpre = at, at += up256((size_t)L.ncells * sizeof(int));
    L.fpre = at, at += up256((size_t)L.nnodes * sizeof(int));
    L.bsumv = at, at += up256((size_t)tiles_of(L.ncells) * sizeof(long long));
    L.bsumf = at, at += up256((size_t)tiles_of(L.nnodes) * sizeof(long long));
    L.bytes = at;
    return L;
}

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_mesh_density_workspace_size(long long N, int Gx, int Gy, int Gz, long long capacity) {
    using namespace lgm;
    if (N < 0 || N >= I31 || capacity < 0 || capacity >= I31 || !grid_ok(Gx, Gy, Gz)) return 0;
    Grid gr;
    gr.G[0] = Gx, gr.G[1] = Gy, gr.G[2] = Gz;
    for (int a = 0; a < 3; a++) gr.nb[a] = (gr.G[a] + BR - 1) / BR;
    return density_layout(N, gr, capacity).bytes;
}

extern "C" int lgm_mesh_density_count(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz,
                                      const float *lo, const float *h, float cutoff, void *ws, size_t ws_bytes,
                                      long long *npairs, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    hipStream_t st = (hipStream_t)stream;
    Grid gr;
    DensityLayout L;
    if (!npairs) {
        set_error("lgm_mesh_density_count: null pointer (npairs)");
        return LGM_E_INVALID;
    }
    return density_front("lgm_mesh_density_count", g, N, scale_modifier, Gx, Gy, Gz, lo, h, cutoff, 0, ws, ws_bytes, gr,
                         L, npairs, st);
}

extern "C" int lgm_mesh_density(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz,
                                const float *lo, const float *h, float cutoff, long long capacity, float *sigma,
                                float *rgb, void *ws, size_t ws_bytes, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    hipStream_t st = (hipStream_t)stream;
    Grid gr;
    DensityLayout L;
    if (!sigma) {
        set_error("lgm_mesh_density: null pointer (sigma)");
        return LGM_E_INVALID;
    }
    const int rc = density_front("lgm_mesh_density", g, N, scale_modifier, Gx, Gy, Gz, lo, h, cutoff, capacity, ws,
                                 ws_bytes, gr, L, nullptr, st);
    if (rc) return rc;
    char *w = (char *)ws;
    if (N > 0)
        LGM_LAUNCH("k_mesh_bin_fill", st,
                   (k_mesh_bin_fill<<<(unsigned)((N + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                       (int)N, gr, (const int4 *)(w + L.box), (const int *)(w + L.cnt), (int *)(w + L.cur),
                       (int *)(w + L.lists), capacity)));
    LGM_LAUNCH("k_mesh_density", st,
               (k_mesh_density<<<(unsigned)L.nbricks, THREADS, 0, st>>>(
                   gr, (int)N, (const float4 *)(w + L.rec), (const int4 *)(w + L.box), (const int *)(w + L.cnt),
                   (const int *)(w + L.cur), (const int *)(w + L.lists), (const long long *)(w + L.total), capacity,
                   log2f(cutoff), sigma, rgb)));
    return LGM_OK;
}

extern "C" size_t lgm_mesh_sample_workspace_size(long long N, long long M, int Gx, int Gy, int Gz, long long capacity) {
    using namespace lgm;
    if (N < 0 || N >= I31 || M < 0 || 3 * M >= I31 || capacity < 0 || capacity >= I31 || !grid_ok(Gx, Gy, Gz)) return 0;
    Grid gr;
    gr.G[0] = Gx, gr.G[1] = Gy, gr.G[2] = Gz;
    for (int a = 0; a < 3; a++) gr.nb[a] = (gr.G[a] + BR - 1) / BR;
    return density_layout(N, gr, capacity, M).bytes;
}

extern "C" int lgm_mesh_sample_count(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz,
                                     const float *lo, const float *h, float cutoff, void *ws, size_t ws_bytes,
                                     long long *npairs, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    hipStream_t st = (hipStream_t)stream;
    Grid gr;
    DensityLayout L;
    if (!npairs) {
        set_error("lgm_mesh_sample_count: null pointer (npairs)");
        return LGM_E_INVALID;
    }
    return density_front("lgm_mesh_sample_count", g, N, scale_modifier, Gx, Gy, Gz, lo, h, cutoff, 0, ws, ws_bytes, gr, L,
                         npairs, st, 0);
}

extern "C" int lgm_mesh_sample(const float *g, long long N, float scale_modifier, int Gx, int Gy, int Gz,
                               const float *lo, const float *h, float cutoff, long long capacity, const float *points,
                               long long M, float *sigma, float *rgb, void *ws, size_t ws_bytes, void *stream,
                               const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_mesh_sample";
    hipStream_t st = (hipStream_t)stream;
    Grid gr;
    DensityLayout L;
    if (M < 0 || 3 * M >= I31) {
        set_error("%s: M=%lld: must be >= 0 with 3 M below 2^31", who, M);
        return LGM_E_INVALID;
    }
    if (M > 0 && (!points || !sigma)) {
        set_error("%s: null pointer (points, sigma)", who);
        return LGM_E_INVALID;
    }
    const int rc = density_front(who, g, N, scale_modifier, Gx, Gy, Gz, lo, h, cutoff, capacity, ws, ws_bytes, gr, L,
                                 nullptr, st, M);
    if (rc || M == 0) return rc;
    char *w = (char *)ws;
    if (hipMemsetAsync(w + L.pcnt, 0, L.pbsum - L.pcnt, st) != hipSuccess) {  // (the points' counts and cursors)
        set_error("%s: hipMemsetAsync failed", who);
        return LGM_E_HIP;
    }
    if (N > 0)
        LGM_LAUNCH("k_mesh_bin_fill", st,
                   (k_mesh_bin_fill<<<(unsigned)((N + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                       (int)N, gr, (const int4 *)(w + L.box), (const int *)(w + L.cnt), (int *)(w + L.cur),
                       (int *)(w + L.lists), capacity)));
    Domain dom;
    for (int a = 0; a < 3; a++) {
        dom.lo[a] = (double)gr.lo[a] - (double)gr.h[a] / 2.0;
        dom.hi[a] = (double)gr.lo[a] + ((double)gr.G[a] - 0.5) * (double)gr.h[a];
    }
    const unsigned pblocks = (unsigned)((M + THREADS - 1) / THREADS);
    LGM_LAUNCH("k_mesh_point_count", st,
               (k_mesh_point_count<<<pblocks, THREADS, 0, st>>>(points, (int)M, gr, dom, (const long long *)(w + L.total),
                                                                capacity, (int *)(w + L.pbrick), (int *)(w + L.pcnt),
                                                                sigma, rgb)));
    const int rs = scan_in_place((int *)(w + L.pcnt), L.nbricks, (long long *)(w + L.pbsum),
                                 (long long *)(w + L.ptotal), st);
    if (rs) return rs;
    LGM_LAUNCH("k_mesh_point_fill", st,
               (k_mesh_point_fill<<<pblocks, THREADS, 0, st>>>((int)M, (const int *)(w + L.pbrick),
                                                               (const int *)(w + L.pcnt), (int *)(w + L.pcur),
                                                               (int *)(w + L.plist))));
    LGM_LAUNCH("k_mesh_sample", st,
               (k_mesh_sample<<<(unsigned)L.nbricks, THREADS, 0, st>>>(
                   gr, (int)N, (const float4 *)(w + L.rec), (const int4 *)(w + L.box), (const int *)(w + L.cnt),
                   (const int *)(w + L.cur), (const int *)(w + L.lists), (const long long *)(w + L.total), capacity,
                   log2f(cutoff), points, (const int *)(w + L.pcnt), (const int *)(w + L.pcur),
                   (const int *)(w + L.plist), sigma, rgb)));
    return LGM_OK;
}

extern "C" int lgm_mesh_atlas(const float *vertices, long long nv, const int *faces, long long nf, int T, int cols,
                              int rows, float *points, float *uvs, int *face_uvs, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_mesh_atlas";
    const long long nq = nf / 2;
    if (nv < 0 || nf < 0 || (nf & 1) || 3 * nv >= I31 || 3 * nf >= I31) {
        set_error("%s: nv=%lld nf=%lld: counts must be >= 0 with 3 x count below 2^31, nf even", who, nv, nf);
        return LGM_E_INVALID;
    }
    if (T < 2 || cols < 1 || rows < 1 || (long long)cols * T > LGM_MESH_ATLAS_MAX ||
        (long long)rows * T > LGM_MESH_ATLAS_MAX || (long long)cols * rows < nq) {
        set_error("%s: T=%d cols=%d rows=%d for %lld quads: T >= 2, cols rows >= the quads, cols T and rows T <= %d",
                  who, T, cols, rows, nq, LGM_MESH_ATLAS_MAX);
        return LGM_E_INVALID;
    }
    if (3 * nq * T * T >= I31) {
        set_error("%s: %lld quads of %d x %d texels: 3 x texels must be below 2^31", who, nq, T, T);
        return LGM_E_INVALID;
    }
    if (nq > 0 && (!vertices || !faces || !points || !uvs || !face_uvs)) {
        set_error("%s: null pointer (vertices, faces, points, uvs, face_uvs)", who);
        return LGM_E_INVALID;
    }
    if (nq == 0) return LGM_OK;
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_mesh_atlas", st,
               (k_mesh_atlas<<<(unsigned)((nq * T * T + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                   vertices, nv, faces, nq, T, cols, rows, points, uvs, face_uvs)));
    return LGM_OK;
}

extern "C" size_t lgm_mesh_extract_workspace_size(int Gx, int Gy, int Gz) {
    using namespace lgm;
    if (!grid_ok(Gx, Gy, Gz)) return 0;
    Grid gr;
    gr.G[0] = Gx, gr.G[1] = Gy, gr.G[2] = Gz;
    return extract_layout(gr).bytes;
}

extern "C" int lgm_mesh_count(const float *sigma, int Gx, int Gy, int Gz, float iso, void *ws, size_t ws_bytes,
                              long long *counts, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_mesh_count";
    Grid gr;
    int rc = make_grid(who, Gx, Gy, Gz, nullptr, nullptr, false, gr);
    if (rc) return rc;
    if (!fin(iso) || !(iso > 0.f)) {
        set_error("%s: iso=%g must be finite and positive", who, iso);
        return LGM_E_INVALID;
    }
    if (!sigma || !ws || !counts) {
        set_error("%s: null pointer (sigma, ws, counts)", who);
        return LGM_E_INVALID;
    }
    const ExtractLayout L = extract_layout(gr);
    if (ws_bytes < L.bytes) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.bytes);
        return LGM_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    LGM_LAUNCH("k_mesh_classify", st,
               (k_mesh_classify<<<(unsigned)((L.nnodes + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                   sigma, gr, iso, (int *)(w + L.vpre), (int *)(w + L.fpre))));
    rc = scan_in_place((int *)(w + L.vpre), L.ncells, (long long *)(w + L.bsumv), counts, st);
    if (rc) return rc;
    return scan_in_place((int *)(w + L.fpre), L.nnodes, (long long *)(w + L.bsumf), counts + 1, st);
}

extern "C" int lgm_mesh_emit(const float *sigma, const float *rgb, int Gx, int Gy, int Gz, const float *lo,
                             const float *h, float iso, const void *ws, size_t ws_bytes, long long nv, long long nf,
                             float *vertices, float *colors, int *faces, long long cap_v, long long cap_f, void *stream,
                             const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_mesh_emit";
    Grid gr;
    const int rc = make_grid(who, Gx, Gy, Gz, lo, h, true, gr);
    if (rc) return rc;
    if (!fin(iso) || !(iso > 0.f)) {
        set_error("%s: iso=%g must be finite and positive", who, iso);
        return LGM_E_INVALID;
    }
    if (nv < 0 || nf < 0 || cap_v < 0 || cap_f < 0 || 3 * nv >= I31 || 3 * nf >= I31 || cap_v >= I31 || cap_f >= I31) {
        set_error("%s: nv=%lld nf=%lld cap_v=%lld cap_f=%lld: counts must be >= 0 with 3 x count below 2^31", who, nv, nf,
                  cap_v, cap_f);
        return LGM_E_INVALID;
    }
    if (cap_v < nv || cap_f < nf) {
        set_error("%s: capacity of %lld vertices and %lld faces, %lld and %lld counted", who, cap_v, cap_f, nv, nf);
        return LGM_E_INVALID;
    }
    if (!sigma || !ws || (nv > 0 && !vertices) || (nv > 0 && rgb && !colors) || (nf > 0 && !faces)) {
        set_error("%s: null pointer (sigma, ws, vertices, colors, faces)", who);
        return LGM_E_INVALID;
    }
    const ExtractLayout L = extract_layout(gr);
    if (ws_bytes < L.bytes) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.bytes);
        return LGM_E_WORKSPACE;
    }
    if (nv == 0 && nf == 0) return LGM_OK;
    hipStream_t st = (hipStream_t)stream;
    const char *w = (const char *)ws;
    LGM_LAUNCH("k_mesh_emit", st,
               (k_mesh_emit<<<(unsigned)((L.nnodes + THREADS - 1) / THREADS), THREADS, 0, st>>>(
                   sigma, rgb, gr, iso, (const int *)(w + L.vpre), (const int *)(w + L.fpre), vertices, colors, faces,
                   nv, nf)));
    return LGM_OK;
}
