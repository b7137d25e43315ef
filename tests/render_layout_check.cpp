// Host check of lgm_amd/csrc/render_layout.h (built and run by tests/test_render_layout.py with the address and
// undefined-behaviour sanitizers): the accumulator block's regions and the device index functions that address them,
// the workspace's regions, the workspace sizes against recorded values, and the diagnostics counter map.
// `render_layout_check words B V N H W` prints cnt_words for the Python side's comparison.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "render_layout.h"

#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            fprintf(stderr, "FAILED: %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);   \
            fprintf(stderr, "\n");          \
            exit(1);                        \
        }                                   \
    } while (0)

using lgm::Region;

// marks bytes [off, off + n) of the block with `tag`; every byte is marked at most once and lies inside `r`
static void mark(std::vector<char> &bytes, const Region &r, size_t off, size_t n, char tag, const char *what) {
    CHECK(off >= r.off && off + n <= r.end(), "%s: bytes [%zu, %zu) leave the region [%zu, %zu)", what, off, off + n,
          r.off, r.end());
    for (size_t i = off; i < off + n; i++) {
        CHECK(bytes[i] == 0, "%s: byte %zu addressed twice", what, i);
        bytes[i] = tag;
    }
}
static void covered(const std::vector<char> &bytes, const Region &r, char tag, const char *what) {
    for (size_t i = r.off; i < r.end(); i++) CHECK(bytes[i] == tag, "%s: byte %zu of the region not addressed", what, i);
}

static void check_accum(int B, int V, int N, bool det, bool aa) {
    const lgm::AccumLayout a = lgm::accum_layout(B, V, N, det, aa);
    const size_t BVN = (size_t)B * V * N, e = a.elem;
    CHECK(a.elem == (det ? 8 : 4), "elem %d", a.elem);
    // in order, disjoint, aligned to their elements, ending at the total
    const Region *reg[4] = {&a.main, &a.needle, &a.aa_part, &a.aa_s};
    const size_t align[4] = {e, 8, e, 4};
    size_t prev = 0;
    for (int r = 0; r < 4; r++) {
        CHECK(reg[r]->off >= prev, "region %d starts at %zu, the one before ends at %zu", r, reg[r]->off, prev);
        CHECK(reg[r]->off % align[r] == 0, "region %d at %zu is not %zu-B aligned", r, reg[r]->off, align[r]);
        prev = reg[r]->end();
    }
    CHECK(prev == a.total, "regions end at %zu, total %zu", prev, a.total);
    CHECK(a.main.bytes == (BVN * lgm::NACC_V + (size_t)B * N * lgm::NACC_S) * e, "main %zu", a.main.bytes);
    CHECK(a.needle.bytes == (det ? 0 : BVN * 3 * 8), "needle %zu", a.needle.bytes);
    CHECK(a.aa_part.bytes == (aa ? BVN * e : 0) && a.aa_s.bytes == (aa ? BVN * 4 : 0), "antialias regions");
    // every index function is a bijection from its index set onto exactly its region
    std::vector<char> bytes(a.total, 0);
    for (size_t k = 0; k < BVN; k++)
        for (int q = 0; q < lgm::NACC_V; q++) mark(bytes, a.main, lgm::accum_view_elem(k, q) * e, e, 1, "view");
    for (int b = 0; b < B; b++)
        for (int i = 0; i < N; i++)
            for (int q = 0; q < lgm::NACC_S; q++)
                mark(bytes, a.main, lgm::accum_scene_elem((size_t)B * V, N, b, i, q) * e, e, 1, "scene");
    covered(bytes, a.main, 1, "main");
    if (!det) {
        for (size_t k = 0; k < BVN; k++)
            for (int c = 0; c < lgm::NEEDLE_DBL; c++)
                mark(bytes, a.needle, lgm::accum_needle_dbl(B, V, N, k, c) * 8, 8, 2, "needle");
        covered(bytes, a.needle, 2, "needle");
    }
    if (aa) {
        for (size_t k = 0; k < BVN; k++) mark(bytes, a.aa_part, (lgm::accum_aa_elem0(B, V, N, det) + k) * e, e, 3, "aa");
        covered(bytes, a.aa_part, 3, "aa_part");
    }
    // the repeated backward's clear range: the three accumulator regions and the padding between them (less than one
    // double), none of the factors
    const Region c = a.clear();
    CHECK(c.off == 0 && c.end() == a.aa_part.end() && c.end() == a.aa_s.off, "clear range [%zu, %zu)", c.off, c.end());
    size_t pad = 0;
    for (size_t i = c.off; i < c.end(); i++) pad += bytes[i] == 0;
    CHECK(pad == a.needle.off - a.main.end() && pad < 8, "%zu unaddressed bytes in the clear range", pad);
    // the forward's zero range: from the block's start over the main records, in whole 16-B stores, less than one
    // store beyond them and inside what make_layout reserves for the block
    const Region z = a.fwd_zero();
    CHECK(z.off == 0 && z.bytes % 16 == 0 && z.bytes >= a.main.bytes && z.bytes - a.main.bytes < 16, "zero range %zu for %zu",
          z.bytes, a.main.bytes);
    const int opt = (det ? LGM_RENDER_DETERMINISTIC : 0) | (aa ? LGM_RENDER_ANTIALIAS : 0);
    const lgm::Layout L = lgm::make_layout(B, V, N, 40, 24, 0, opt);
    CHECK(L.acc.total == a.total && z.bytes <= L.lossp - L.accum, "zero range %zu, reserved %zu", z.bytes, L.lossp - L.accum);
}

static void check_workspace(int B, int V, int N, int H, int W, long long cap) {
    lgm::Layout L4[4];
    for (int o = 0; o < 4; o++) {
        const int opt = (o & 1 ? LGM_RENDER_DETERMINISTIC : 0) | (o & 2 ? LGM_RENDER_ANTIALIAS : 0);
        const lgm::Layout L = L4[o] = lgm::make_layout(B, V, N, H, W, cap, opt);
        const size_t BV = (size_t)B * V, T = (size_t)((W + 15) / 16) * ((H + 15) / 16), P = (size_t)H * W;
        // the regions in their order in memory, with the bytes their users address
        const struct { const char *name; size_t off, bytes; } reg[] = {
            {"gP", L.gP, BV * N * 16}, {"gQ", L.gQ, BV * N * 16}, {"rects", L.rects, BV * N * 8},
            {"tile_count", L.tile_count, BV * T * 4}, {"misc", L.misc, (size_t)lgm::MISC_BYTES},
            {"tile_start", L.tile_start, (BV * T + 1) * 4}, {"order", L.order, T * 4},
            {"pairs", L.pairs, (size_t)L.cap * 8}, {"final_T", L.final_T, BV * P * 4},
            {"n_contrib", L.n_contrib, BV * P * 4}, {"wlast", L.wlast, BV * T * 16}, {"cfin", L.cfin, BV * P * 16},
            {"ck", L.ck, (size_t)L.ck_slots * 5 * 256 * 4}, {"cklist", L.cklist, (size_t)L.ck_slots * 8},
            {"nck", L.nck, BV * T * 4}, {"cmask", L.cmask, BV * P}, {"accum", L.accum, L.acc.total},
            {"lossp", L.lossp, BV * T * 8}, {"lossw", L.lossw, (BV * T + 2047) / 2048 * 16}, {"detmax", L.detmax, 256}};
        size_t prev = 0;
        for (const auto &r : reg) {
            CHECK(r.off % 256 == 0, "%s at %zu is not 256-B aligned", r.name, r.off);
            CHECK(r.off >= prev, "%s at %zu overlaps the region before it (ends at %zu)", r.name, r.off, prev);
            prev = r.off + r.bytes;
        }
        CHECK(L.total == lgm::align_up(prev) && L.total >= prev, "total %zu, last end %zu", L.total, prev);
        CHECK(L.slot == (cap <= 0) && L.cap == (cap <= 0 ? (long long)(BV * T * N) : cap), "cap %lld", L.cap);
        CHECK(L.ck_slots == (o & 1 ? 0 : 8 * L.ck_region), "ck_slots %d", L.ck_slots);
        // the binning's one memset: tile_count through misc, and nothing of the region after them
        const Region bc = L.bin_clear();
        CHECK(bc.off == L.tile_count && bc.end() == L.misc + lgm::MISC_BYTES && bc.end() <= L.tile_start &&
                  L.misc == lgm::align_up(L.tile_count + BV * T * 4),
              "bin_clear [%zu, %zu)", bc.off, bc.end());
    }
    // what the inspection entry points read sits at the same offsets whatever the options
    for (int o = 1; o < 4; o++) {
        const lgm::Layout &a = L4[0], &b = L4[o];
        CHECK(a.gP == b.gP && a.gQ == b.gQ && a.rects == b.rects && a.tile_count == b.tile_count &&
                  a.tile_start == b.tile_start && a.pairs == b.pairs && a.final_T == b.final_T &&
                  a.n_contrib == b.n_contrib && a.slot == b.slot && a.cap == b.cap,
              "options %d move a region the inspection entry points read", o);
    }
}

// lgm_render_workspace_size_opts of commit 276c0ff (the last one before this header), recorded by calling it:
// (B, V, N, H, W, pair_capacity, options) -> bytes
static const struct { int B, V, N, H, W; long long cap; int options; unsigned long long bytes; } SIZES[] = {
    {1, 6, 100000, 256, 256, 0, 0, 1308840960ull},
    {8, 6, 100000, 256, 256, 0, 0, 10378860800ull},
    {1, 1, 50000, 256, 256, 0, 0, 111875328ull},
    {1, 20, 65536, 512, 512, 0, 2, 11035550976ull},
    {2, 13, 16384, 512, 512, 0, 16, 3699553280ull},
    {1, 6, 100000, 256, 256, 1000000, 0, 88040960ull},
    {1, 6, 100000, 256, 256, 0, 48, 1301887744ull},
    {1, 2, 1, 16, 16, 0, 0, 57600ull},
    {1, 3, 3, 40, 24, 0, 32, 282112ull},
    {1, 3, 3, 40, 24, 0, 48, 76800ull},
    {2, 2, 7, 33, 17, 5, 32, 308992ull},
    {1, 1, 0, 16, 16, 0, 0, 49920ull},
};

static void check_counters(int B, int V, int N, int H, int W) {
    const size_t BV = (size_t)B * V, T = (size_t)((W + 15) / 16) * ((H + 15) / 16);
    const size_t nbin = BV * ((N + 511) / 512), nitem = 3 * BV * T + 16;
    // aggregate words, then the three record ranges back to back, ending at the word count
    CHECK(lgm::cnt_tile(0) == 8, "tile records start at %zu", lgm::cnt_tile(0));
    for (size_t t = 0; t < BV * T; t++)
        CHECK(lgm::cnt_tile(t + 1) == lgm::cnt_tile(t) + lgm::CNT_TILE, "tile record %zu", t);
    CHECK(lgm::cnt_bin0(BV, T) == lgm::cnt_tile(BV * T), "binning records start at %zu", lgm::cnt_bin0(BV, T));
    CHECK(lgm::cnt_item0(BV, T, N) == lgm::cnt_bin0(BV, T) + lgm::CNT_BIN * nbin, "items start at %zu", lgm::cnt_item0(BV, T, N));
    CHECK(lgm::cnt_words(B, V, N, H, W) == lgm::cnt_item0(BV, T, N) + lgm::CNT_ITEM * nitem, "%zu words",
          lgm::cnt_words(B, V, N, H, W));
    // the documented size (include/lgm_render.h)
    CHECK(lgm::cnt_words(B, V, N, H, W) == 8 + 8 * BV * T + 8 * nbin + 4 * nitem, "%zu words", lgm::cnt_words(B, V, N, H, W));
    // room for every record the kernels write: k_bin's workgroups, k_render_bwd's work items
    const lgm::Layout L = lgm::make_layout(B, V, N, H, W, 0, 0);
    CHECK((size_t)B * ((V + 2) / 3) * ((N + 511) / 512) <= nbin, "binning workgroups exceed %zu records", nbin);
    CHECK(((BV * T + 7) & ~(size_t)7) + L.ck_slots <= nitem, "backward items exceed %zu records", nitem);
}

int main(int argc, char **argv) {
    if (argc == 7 && argv[1][0] == 'w') {
        printf("%zu\n", lgm::cnt_words(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])));
        return 0;
    }
    const int Ns[5] = {0, 1, 2, 3, 5};
    const struct { int H, W; long long cap; } shapes[4] = {{16, 16, 0}, {40, 24, 0}, {33, 17, 5}, {256, 256, 1000}};
    for (int B = 1; B <= 2; B++)
        for (int V = 1; V <= 3; V++)
            for (int N : Ns) {
                for (int o = 0; o < 4; o++) check_accum(B, V, N, o & 1, o & 2);
                for (const auto &s : shapes) check_workspace(B, V, N, s.H, s.W, s.cap);
            }
    for (const auto &s : SIZES) {
        const size_t got = lgm::make_layout(s.B, s.V, s.N, s.H, s.W, s.cap, s.options).total;
        CHECK(got == s.bytes, "(%d, %d, %d, %d, %d, %lld, %d): %zu bytes, recorded %llu", s.B, s.V, s.N, s.H, s.W, s.cap,
              s.options, got, s.bytes);
    }
    check_counters(1, 2, 1, 16, 16);
    check_counters(2, 3, 1000, 40, 24);
    check_counters(8, 6, 100000, 256, 256);
    puts("render_layout ok");
    return 0;
}
