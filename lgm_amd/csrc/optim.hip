// lgm_amd/csrc/optim.hip -- the optimizer step of include/lgm_optim.h: the global-norm gradient clip and the AdamW
// update of the reference's training iteration (main.py:73, 105-109) over a whole parameter list per launch.
//
//   k_optim_sqnorm  one fp64 partial sum of g^2 per chunk, fixed order
//   k_optim_reduce  one workgroup: the fixed-order fp64 sum of the partials -> norm and clip coefficient (device)
//   k_optim_adamw   the update with the coefficient applied to g in registers (the scaled gradient is never stored)
//   k_optim_scale   g <- g coef (the stand-alone clip)
//
// One workgroup of 256 threads owns one chunk of LGM_OPTIM_CHUNK = 4096 elements of one tensor and finds it with one
// load of chunk_tensor[] and one of its table row (both uniform over the workgroup). Every thread holds four quads
// of four consecutive elements: with p, g, m, v that is sixteen independent 16-byte loads per thread issued ahead of
// the arithmetic, 64 KiB per workgroup. The passes are bandwidth-bound streams (4 B read for the norm, 16 B read and
// 12 B written per element for the update); the default model's list is ~100k chunks, several hundred per CU, and 234
// of its 344 tensors are a single short chunk, where the lanes past the end do nothing.
// A tensor with a pointer that is not 16-byte aligned (a view into a flat bucket) takes element loads and stores:
// in the norm with the same element-to-thread assignment (the sum's order is the same), in the elementwise passes one
// element per lane and pass (contiguous 256-byte wave accesses). Results do not depend on alignment. Plain vector
// stores only; no atomics.
#include "common.h"
#include "lgm_optim.h"

// every fp32 operation of the update is rounded on its own (include/lgm_optim.h)
#pragma clang fp contract(off)

namespace lgm {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = LGM_OPTIM_CHUNK;
constexpr int OPT_QUADS = OPT_CHUNK / (4 * OPT_THREADS);  // quads per thread
constexpr int RED_THREADS = 1024;
constexpr long long OPT_GRID_MAX = 2147483647LL;
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is a whole number of quads per thread");

struct AdamArgs {
    float decay, step_size, rbc2, w1, w2, beta2, eps;
};

// the chunk of this workgroup: its tensor's row, the offset of the chunk in the tensor and its length
__device__ __forceinline__ lgm_optim_tensor locate(const lgm_optim_tensor *__restrict__ table,
                                                   const int *__restrict__ chunk_tensor, long long chunk, int &off,
                                                   int &n) {
    const lgm_optim_tensor T = table[chunk_tensor[chunk]];
    off = (int)(chunk - T.chunk0) * OPT_CHUNK;
    n = min(OPT_CHUNK, T.numel - off);
    return T;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }

// The tensors' pointers come out of the table, so the compiler cannot tell that they point to global memory and
// would emit flat accesses: the loads and stores below go through global address-space pointers.
#define OPT_GLOBAL __attribute__((address_space(1)))
typedef float opt_f4 __attribute__((ext_vector_type(4)));

// elements i .. i + 3 of the chunk at p (those below n; the others read as 0)
template <bool VEC>
__device__ __forceinline__ float4 ld_quad(const float *p_, int i, int n) {
    const OPT_GLOBAL float *p = (const OPT_GLOBAL float *)p_;
    if (VEC && i + 3 < n) {
        const opt_f4 r = *(const OPT_GLOBAL opt_f4 *)(p + i);
        return make_float4(r.x, r.y, r.z, r.w);
    }
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) r.x = p[i];
    if (i + 1 < n) r.y = p[i + 1];
    if (i + 2 < n) r.z = p[i + 2];
    if (i + 3 < n) r.w = p[i + 3];
    return r;
}

template <bool VEC>
__device__ __forceinline__ void st_quad(float *p_, int i, int n, float4 r) {
    OPT_GLOBAL float *p = (OPT_GLOBAL float *)p_;
    if (VEC && i + 3 < n) {
        opt_f4 q;
        q.x = r.x, q.y = r.y, q.z = r.z, q.w = r.w;
        *(OPT_GLOBAL opt_f4 *)(p + i) = q;
        return;
    }
    if (i < n) p[i] = r.x;
    if (i + 1 < n) p[i + 1] = r.y;
    if (i + 2 < n) p[i + 2] = r.z;
    if (i + 3 < n) p[i + 3] = r.w;
}

// sum over the workgroup in a fixed order: xor butterfly inside each wave, then the wave sums in wave order
// (valid in thread 0). red: one double per wave.
template <int THREADS>
__device__ __forceinline__ double block_sum(double s, double *red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / 64; w++) total += red[w];
    return total;
}

template <bool VEC>
__device__ __forceinline__ double sqnorm_chunk(const float *__restrict__ g, int n) {
    float4 x[OPT_QUADS];
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) x[k] = ld_quad<VEC>(g, (k * OPT_THREADS + (int)threadIdx.x) * 4, n);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) {
        s += (double)x[k].x * (double)x[k].x;
        s += (double)x[k].y * (double)x[k].y;
        s += (double)x[k].z * (double)x[k].z;
        s += (double)x[k].w * (double)x[k].w;
    }
    return s;
}

__global__ __launch_bounds__(OPT_THREADS) void k_optim_sqnorm(const lgm_optim_tensor *__restrict__ table,
                                                              const int *__restrict__ chunk_tensor,
                                                              double *__restrict__ partials) {
    __shared__ double red[OPT_THREADS / 64];
    int off, n;
    const lgm_optim_tensor T = locate(table, chunk_tensor, blockIdx.x, off, n);
    const float *g = T.g + off;
    const double s = aligned16(T.g) ? sqnorm_chunk<true>(g, n) : sqnorm_chunk<false>(g, n);
    const double total = block_sum<OPT_THREADS>(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(RED_THREADS) void k_optim_reduce(const double *__restrict__ partials, int nchunks,
                                                              double max_norm, float *__restrict__ out) {
    __shared__ double red[RED_THREADS / 64];
    double s = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < nchunks; i += RED_THREADS) s += partials[i];
    const double S = block_sum<RED_THREADS>(s, red);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(S), c = max_norm / (nrm + 1e-6);
        out[0] = (float)nrm;
        out[1] = isfinite(S) ? (float)(c < 1.0 ? c : 1.0) : __builtin_nanf("");
    }
}

__device__ __forceinline__ void adamw_elem(float &p, float g, float &m, float &v, float coef, const AdamArgs &a) {
    g = g * coef;
    p = p * a.decay;
    m = m + (g - m) * a.w1;
    v = a.beta2 * v + a.w2 * (g * g);
    // sqrtf and / are the correctly rounded forms under this build's flags (__fsqrt_rn is the hardware's 1-ulp root)
    const float denom = __builtin_sqrtf(v) / a.rbc2 + a.eps;
    p = p - a.step_size * (m / denom);
}

// one element per thread and pass: what a tensor with a pointer that is only 4-byte aligned takes. Consecutive lanes
// take consecutive elements, so every wave instruction is one contiguous 256-byte access (the update is elementwise:
// which thread holds an element does not change its result).
constexpr int OPT_ELEMS = OPT_CHUNK / OPT_THREADS;  // elements per thread

__device__ __forceinline__ void adamw_chunk_elems(float *p_, const float *g_, float *m_, float *v_, int n, float coef,
                                                  const AdamArgs &a) {
    OPT_GLOBAL float *p = (OPT_GLOBAL float *)p_, *m = (OPT_GLOBAL float *)m_, *v = (OPT_GLOBAL float *)v_;
    const OPT_GLOBAL float *g = (const OPT_GLOBAL float *)g_;
    float P[OPT_ELEMS], G[OPT_ELEMS], M[OPT_ELEMS], V[OPT_ELEMS];
#pragma unroll
    for (int k = 0; k < OPT_ELEMS; k++) {
        const int i = k * OPT_THREADS + (int)threadIdx.x;
        const bool in = i < n;
        P[k] = in ? p[i] : 0.f, G[k] = in ? g[i] : 0.f, M[k] = in ? m[i] : 0.f, V[k] = in ? v[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < OPT_ELEMS; k++) {
        const int i = k * OPT_THREADS + (int)threadIdx.x;
        if (i >= n) break;
        adamw_elem(P[k], G[k], M[k], V[k], coef, a);
        p[i] = P[k], m[i] = M[k], v[i] = V[k];
    }
}

__device__ __forceinline__ void scale_chunk_elems(float *g_, int n, float coef) {
    OPT_GLOBAL float *g = (OPT_GLOBAL float *)g_;
    float G[OPT_ELEMS];
#pragma unroll
    for (int k = 0; k < OPT_ELEMS; k++) {
        const int i = k * OPT_THREADS + (int)threadIdx.x;
        G[k] = i < n ? g[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < OPT_ELEMS; k++) {
        const int i = k * OPT_THREADS + (int)threadIdx.x;
        if (i >= n) break;
        g[i] = G[k] * coef;
    }
}

__device__ __forceinline__ void adamw_chunk(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                            float *__restrict__ v, int n, float coef, const AdamArgs &a) {
    float4 P[OPT_QUADS], G[OPT_QUADS], M[OPT_QUADS], V[OPT_QUADS];
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) {
        const int i = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        P[k] = ld_quad<true>(p, i, n), G[k] = ld_quad<true>(g, i, n);
        M[k] = ld_quad<true>(m, i, n), V[k] = ld_quad<true>(v, i, n);
    }
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) {
        const int i = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        if (i >= n) break;  // (lanes past the end hold zeros and store nothing)
        adamw_elem(P[k].x, G[k].x, M[k].x, V[k].x, coef, a);
        adamw_elem(P[k].y, G[k].y, M[k].y, V[k].y, coef, a);
        adamw_elem(P[k].z, G[k].z, M[k].z, V[k].z, coef, a);
        adamw_elem(P[k].w, G[k].w, M[k].w, V[k].w, coef, a);
        st_quad<true>(p, i, n, P[k]);
        st_quad<true>(m, i, n, M[k]);
        st_quad<true>(v, i, n, V[k]);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void k_optim_adamw(const lgm_optim_tensor *__restrict__ table,
                                                             const int *__restrict__ chunk_tensor, long long chunk_begin,
                                                             const float *__restrict__ coef_ptr, AdamArgs a) {
    int off, n;
    const lgm_optim_tensor T = locate(table, chunk_tensor, chunk_begin + blockIdx.x, off, n);
    const float coef = coef_ptr ? *coef_ptr : 1.f;
    if (aligned16(T.p) && aligned16(T.g) && aligned16(T.m) && aligned16(T.v))
        adamw_chunk(T.p + off, T.g + off, T.m + off, T.v + off, n, coef, a);
    else
        adamw_chunk_elems(T.p + off, T.g + off, T.m + off, T.v + off, n, coef, a);
}

__device__ __forceinline__ void scale_chunk(float *__restrict__ g, int n, float coef) {
    float4 G[OPT_QUADS];
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) G[k] = ld_quad<true>(g, (k * OPT_THREADS + (int)threadIdx.x) * 4, n);
#pragma unroll
    for (int k = 0; k < OPT_QUADS; k++) {
        const int i = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        if (i >= n) break;
        st_quad<true>(g, i, n, make_float4(G[k].x * coef, G[k].y * coef, G[k].z * coef, G[k].w * coef));
    }
}

__global__ __launch_bounds__(OPT_THREADS) void k_optim_scale(const lgm_optim_tensor *__restrict__ table,
                                                             const int *__restrict__ chunk_tensor,
                                                             const float *__restrict__ coef_ptr) {
    int off, n;
    const lgm_optim_tensor T = locate(table, chunk_tensor, blockIdx.x, off, n);
    const float coef = *coef_ptr;
    if (aligned16(T.g))
        scale_chunk(T.g + off, n, coef);
    else
        scale_chunk_elems(T.g + off, n, coef);
}

bool is_fin(double x) { return x - x == 0.0; }

// the checks the three entry points share; 1: nothing to do, 0: go on, < 0: error
int check_lists(const char *who, const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor,
                long long chunk_begin, long long nchunks) {
    if (ntensors < 0 || nchunks < 0 || chunk_begin < 0) {
        set_error("%s: negative count (ntensors=%d chunk_begin=%lld nchunks=%lld)", who, ntensors, chunk_begin, nchunks);
        return LGM_E_INVALID;
    }
    if (ntensors == 0) return 1;
    if (!table || (nchunks > 0 && !chunk_tensor)) {
        set_error("%s: null pointer (table, chunk_tensor)", who);
        return LGM_E_INVALID;
    }
    if (nchunks > OPT_GRID_MAX || chunk_begin > OPT_GRID_MAX - nchunks) {
        set_error("%s: chunk_begin=%lld nchunks=%lld needs a launch grid beyond %lld workgroups", who, chunk_begin,
                  nchunks, OPT_GRID_MAX);
        return LGM_E_INVALID;
    }
    return 0;
}

}  // namespace
}  // namespace lgm

extern "C" size_t lgm_optim_workspace_size(long long nchunks) {
    return nchunks > 0 ? (size_t)nchunks * sizeof(double) : 0;
}

extern "C" int lgm_optim_grad_norm(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor,
                                   long long nchunks, double max_norm, double *partials, size_t partials_bytes,
                                   float *out, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_optim_grad_norm";
    const int c = check_lists(who, table, ntensors, chunk_tensor, 0, nchunks);
    if (c) return c < 0 ? c : LGM_OK;
    if (!(max_norm >= 0.0)) {
        set_error("%s: bad max_norm %g", who, max_norm);
        return LGM_E_INVALID;
    }
    if (!out || (nchunks > 0 && !partials)) {
        set_error("%s: null pointer (partials, out)", who);
        return LGM_E_INVALID;
    }
    if (partials_bytes < lgm_optim_workspace_size(nchunks)) {
        set_error("%s: partials buffer of %zu bytes, %zu needed", who, partials_bytes,
                  lgm_optim_workspace_size(nchunks));
        return LGM_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (nchunks > 0)
        LGM_LAUNCH("k_optim_sqnorm", st,
                   (k_optim_sqnorm<<<(unsigned)nchunks, OPT_THREADS, 0, st>>>(table, chunk_tensor, partials)));
    LGM_LAUNCH("k_optim_reduce", st, (k_optim_reduce<<<1, RED_THREADS, 0, st>>>(partials, (int)nchunks, max_norm, out)));
    return LGM_OK;
}

extern "C" int lgm_optim_adamw(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor,
                               long long chunk_begin, long long nchunks, const float *coef, double lr, double beta1,
                               double beta2, double eps, double weight_decay, double step, void *stream,
                               const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_optim_adamw";
    const int c = check_lists(who, table, ntensors, chunk_tensor, chunk_begin, nchunks);
    if (c) return c < 0 ? c : LGM_OK;
    if (!is_fin(lr) || !is_fin(eps) || !is_fin(weight_decay) || !(beta1 >= 0.0 && beta1 < 1.0) ||
        !(beta2 >= 0.0 && beta2 < 1.0) || !(step >= 1.0) || !is_fin(step)) {
        set_error("%s: bad hyperparameters lr=%g betas=(%g, %g) eps=%g weight_decay=%g step=%g", who, lr, beta1, beta2,
                  eps, weight_decay, step);
        return LGM_E_INVALID;
    }
    if (nchunks == 0) return LGM_OK;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    AdamArgs a;
    a.decay = (float)(1.0 - lr * weight_decay);
    a.step_size = (float)(lr / bc1);
    a.rbc2 = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - beta1);
    a.w2 = (float)(1.0 - beta2);
    a.beta2 = (float)beta2;
    a.eps = (float)eps;
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_optim_adamw", st,
               (k_optim_adamw<<<(unsigned)nchunks, OPT_THREADS, 0, st>>>(table, chunk_tensor, chunk_begin, coef, a)));
    return LGM_OK;
}

extern "C" int lgm_optim_scale(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor, long long nchunks,
                               const float *coef, void *stream, const lgm_diag *diag) {
    using namespace lgm;
    clear_error();
    DiagScope ds(diag);
    const char *who = "lgm_optim_scale";
    const int c = check_lists(who, table, ntensors, chunk_tensor, 0, nchunks);
    if (c) return c < 0 ? c : LGM_OK;
    if (!coef) {
        set_error("%s: null pointer (coef)", who);
        return LGM_E_INVALID;
    }
    if (nchunks == 0) return LGM_OK;
    hipStream_t st = (hipStream_t)stream;
    LGM_LAUNCH("k_optim_scale", st,
               (k_optim_scale<<<(unsigned)nchunks, OPT_THREADS, 0, st>>>(table, chunk_tensor, coef)));
    return LGM_OK;
}
