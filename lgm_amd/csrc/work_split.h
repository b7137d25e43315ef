// lgm_amd/csrc/work_split.h -- index arithmetic that deals work to workgroups: the XCD-grouped item order and the
// split-K ranges. Plain C++ (no HIP header), so a host compiler can include and test it (tests/test_work_split.py).
#pragma once

#ifdef __HIPCC__
#define LGM_HD __host__ __device__ __forceinline__
#else
#define LGM_HD inline
#endif

namespace lgm {

// XCD-grouped work order of M items (the render's (view, tile) items in the sort and both compositing kernels, the
// (split, tile) items of the weight-gradient GEMMs). Workgroups are dealt round-robin over the 8 XCDs
// (MI355X_MICROARCH.md: blocks b and b + 8 share an XCD and its 4 MB L2), so block b takes item xcd_item(b): the
// blocks of group g = b % 8 walk one contiguous eighth of the items in order, and neighbouring items -- tiles that
// gather mostly the same Gaussians, output tiles that read the same rows of one K range -- run on one L2 at about the
// same time. (The render's previous LPT order dealt neighbouring tiles to all eight L2s: 5-17 % L2 hit rates in the
// compositing kernels.) Bijective on [0, M) for any M (group sizes q + 1 for g < r, else q). Speed only, never
// correctness.
LGM_HD int xcd_item(int b, int M) {
    const int q = M >> 3, r = M & 7, g = b & 7, i = b >> 3;
    return (g < r ? g * (q + 1) : r * (q + 1) + (g - r) * q) + i;
}
LGM_HD int xcd_group(int t, int M) {  // the block group (b % 8) that runs item t
    const int q = M >> 3, r = M & 7;
    return t < r * (q + 1) ? t / (q + 1) : r + (t - r * (q + 1)) / (q > 0 ? q : 1);
}

// Split s of S over n steps: the steps [first, first + count). With q, r = divmod(n, S) the first r splits take
// q + 1 steps and the others q, so the ranges tile [0, n) in order and their lengths differ by at most one.
template <typename I>
LGM_HD void split_range(I n, int S, int s, I &first, I &count) {
    const I q = n / S, r = n - q * S;
    first = s * q + (s < r ? s : r);
    count = q + (s < r ? 1 : 0);
}

}  // namespace lgm

#undef LGM_HD
