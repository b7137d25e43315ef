/*
 * lgm_optim.h -- C ABI of the optimizer-step kernels in liblgm_amd.so (lgm_amd/csrc/optim.hip): the tail of the
 * reference's training iteration (main.py:105-109 with the optimizer of main.py:73): the global-norm gradient clip
 * (accelerator.clip_grad_norm_, torch.nn.utils.clip_grad_norm_ with norm_type 2) and the AdamW update
 * (torch.optim.AdamW), over a whole parameter list per launch. This header is the specification the tests evaluate
 * in fp64.
 *
 * Data model. All tensors are fp32 and dense; a tensor is its numel elements in memory order (the layout does not
 * matter to an elementwise update as long as p, g, m and v of a tensor share it). The caller keeps, in DEVICE memory,
 *   table        [ntensors] lgm_optim_tensor: the pointers p (parameter), g (gradient), m (exp_avg), v (exp_avg_sq),
 *                the numel (0 <= numel < 2^31) and chunk0, the index of the tensor's first chunk;
 *   chunk_tensor [nchunks] int32: the index in `table` of the tensor each chunk belongs to.
 * Tensor i is cut into ceil(numel_i / LGM_OPTIM_CHUNK) chunks of LGM_OPTIM_CHUNK consecutive elements (the last one
 * shorter); the chunks of all tensors are numbered consecutively in table order: chunk0_0 = 0,
 * chunk0_{i+1} = chunk0_i + ceil(numel_i / LGM_OPTIM_CHUNK), nchunks = chunk0 past the last tensor (below 2^31). A
 * tensor of 0 elements has a row and no chunk. One workgroup owns one chunk; no chunk spans two tensors. The kernels
 * trust table and chunk_tensor (they are device memory: the host half of the library cannot read them); the caller
 * builds both from the same list of numels. Pointers need only be 4-byte aligned: a tensor takes 16-byte loads and
 * stores when every pointer the kernel uses of it is 16-byte aligned, and element loads and stores otherwise; the
 * norm's summation order (below) is the same on both paths and the other passes are elementwise, so the results are
 * the same bit for bit.
 *
 * lgm_optim_grad_norm (kernels k_optim_sqnorm, k_optim_reduce). Reads g of every row (p, m, v are not touched and
 * may be NULL).
 *   partials[c] = sum over the chunk's elements of (double)g * (double)g                      (fp64, one per chunk)
 *     in a fixed order: thread t of 256 takes the element quads q = t, t + 256, ... (elements 4q .. 4q + 3 of the
 *     chunk), ascending, into one fp64 accumulator; the 64 accumulators of a wave are summed by an xor butterfly
 *     (distances 32, 16, .. 1) and the four wave sums are added in wave order.
 *   S = sum of partials[0 .. nchunks - 1]: thread t of 1024 sums partials t, t + 1024, ... ascending, the same butterfly
 *     per wave, the 16 wave sums added in wave order.
 *   out[0] = norm = fl32(sqrt(S))
 *   out[1] = coef = fl32(min(1, max_norm / (sqrt(S) + 1e-6))), evaluated in fp64 and rounded once; a non-finite S
 *     (a NaN or an infinity among the gradients) gives coef = NaN.
 * No float atomics: two calls on the same inputs are bitwise equal. The host never sees the norm.
 * partials: DEVICE scratch of at least lgm_optim_workspace_size(nchunks) bytes, 8-byte aligned. out: DEVICE float[2].
 * With nchunks == 0 (every tensor empty) S = 0: norm 0, coef 1.
 *
 * lgm_optim_adamw (kernel k_optim_adamw): the update of the chunks chunk_begin .. chunk_begin + nchunks - 1 (a set
 * of whole tensors that share their hyperparameters and their step count t >= 1; the caller orders the table so
 * that such a set is a contiguous range of chunks, and makes one call per set). coef: DEVICE pointer to one float
 * (out + 1 of lgm_optim_grad_norm), or NULL for 1. Host, in fp64, each rounded to fp32 once:
 *   decay = 1 - lr wd,  step_size = lr / bc1,  rbc2 = sqrt(bc2),  w1 = 1 - beta1,  w2 = 1 - beta2,  beta2,  eps
 *   with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.
 * Per element, in fp32, every operation rounded on its own (no contraction into fused multiply-adds), division and
 * square root correctly rounded, in this order:
 *   g' = g coef
 *   p  <- p decay
 *   m  <- m + (g' - m) w1                                   (torch's lerp form)
 *   v  <- beta2 v + w2 (g' g')
 *   p  <- p - step_size (m / (sqrt(v) / rbc2 + eps))
 * p, m and v are written; g is not.
 *
 * lgm_optim_scale (kernel k_optim_scale): g <- g coef for every chunk 0 .. nchunks - 1, the stand-alone clip
 * (coef: DEVICE pointer to one float, required). p, m, v are not touched and may be NULL.
 *
 * rc < 0 (and lgm_last_error), with nothing launched, on: a null table or chunk_tensor with work to do, negative
 * counts, nchunks or chunk_begin + nchunks beyond 2^31 - 1 (the launch grid), a partials buffer shorter than
 * lgm_optim_workspace_size(nchunks), a null out or coef where it is required, non-finite or out-of-range
 * hyperparameters (lr, eps, wd finite, 0 <= beta < 1, t >= 1). ntensors == 0: rc 0, nothing to do.
 * All work is enqueued on `stream` (a hipStream_t, NULL = default stream); nothing synchronises.
 */
#ifndef LGM_OPTIM_H
#define LGM_OPTIM_H
#include "lgm_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGM_OPTIM_CHUNK 4096 /* elements per chunk = per workgroup */

typedef struct lgm_optim_tensor {
    float *p, *g, *m, *v;
    int numel;
    int chunk0;
} lgm_optim_tensor;

/* bytes of the partials buffer for nchunks chunks (0 when nchunks <= 0) */
size_t lgm_optim_workspace_size(long long nchunks);

int lgm_optim_grad_norm(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor, long long nchunks,
                        double max_norm, double *partials, size_t partials_bytes, float *out, void *stream,
                        const lgm_diag *diag);

int lgm_optim_adamw(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor, long long chunk_begin,
                    long long nchunks, const float *coef, double lr, double beta1, double beta2, double eps,
                    double weight_decay, double step, void *stream, const lgm_diag *diag);

int lgm_optim_scale(const lgm_optim_tensor *table, int ntensors, const int *chunk_tensor, long long nchunks,
                    const float *coef, void *stream, const lgm_diag *diag);

#ifdef __cplusplus
}
#endif
#endif
