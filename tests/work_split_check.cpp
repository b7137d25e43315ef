// Host check of lgm_amd/csrc/work_split.h (built and run by tests/test_work_split.py with the address and
// undefined-behaviour sanitizers): xcd_item is a bijection whose inverse group map is xcd_group, and split_range tiles
// [0, n) in order with lengths that differ by at most one, the longer ones first.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "work_split.h"

#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            fprintf(stderr, "FAILED: %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);   \
            fprintf(stderr, "\n");          \
            exit(1);                        \
        }                                   \
    } while (0)

template <typename I> static void check_split_range() {
    for (int n = 0; n <= 70; n++)
        for (int S = 1; S <= 17; S++) {
            I next = 0, prev = 0, lo = n, hi = 0;
            for (int s = 0; s < S; s++) {
                I first = -1, count = -1;
                lgm::split_range<I>((I)n, S, s, first, count);
                CHECK(first == next, "n=%d S=%d s=%d first=%lld, expected %lld", n, S, s, (long long)first,
                      (long long)next);
                CHECK(count >= 0, "n=%d S=%d s=%d count=%lld", n, S, s, (long long)count);
                CHECK(s == 0 || count <= prev, "n=%d S=%d s=%d: a longer range after a shorter one", n, S, s);
                next = first + count;
                prev = count;
                lo = count < lo ? count : lo;
                hi = count > hi ? count : hi;
            }
            CHECK(next == n, "n=%d S=%d: the ranges end at %lld", n, S, (long long)next);
            CHECK(hi - lo <= 1, "n=%d S=%d: counts from %lld to %lld", n, S, (long long)lo, (long long)hi);
        }
}

int main() {
    for (int M = 1; M <= 300; M++) {
        std::vector<int> seen(M, 0);
        for (int b = 0; b < M; b++) {
            const int t = lgm::xcd_item(b, M);
            CHECK(t >= 0 && t < M, "M=%d b=%d item=%d", M, b, t);
            CHECK(seen[t]++ == 0, "M=%d: item %d dealt twice", M, t);
            CHECK(lgm::xcd_group(t, M) == b % 8, "M=%d b=%d item=%d group=%d", M, b, t, lgm::xcd_group(t, M));
        }
    }
    check_split_range<int>();
    check_split_range<long long>();
    puts("work_split ok");
    return 0;
}
