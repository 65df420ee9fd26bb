// csrc/identity_plan.h -- the LDS, the grid and the rule by which an align call counts the in-place family identity --
// against plain arithmetic, as a stand-alone program: tests/test_identity_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "identity_plan.h"

using namespace sina_hip;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// The tables laid out one after the other, as the kernel's builder places them: a bitmap word per 32 columns, a 16-bit
// count per word and two more, a mask byte per base.  Every byte the builder touches lies below the planned size.
static void check_layout(uint32_t width, uint32_t max_l) {
    const size_t bytes = identity_lds_bytes(width, max_l);
    const size_t nwords = ((size_t)width + 31) / 32;
    std::vector<unsigned char> lds(bytes, 0);
    const size_t bitmap_end = 4 * nwords;
    const size_t wrank_end = bitmap_end + 2 * (nwords + 2);
    const size_t amask_end = wrank_end + max_l;
    EXPECT(nwords * 32 >= width && (nwords == 0 || (nwords - 1) * 32 < width));
    EXPECT(amask_end <= bytes);
    EXPECT(bytes - amask_end >= 16 && bytes - amask_end < 64);  // (slack, and no more than that)
    if (width > 0) lds[4 * ((width - 1) / 32) + 3] = 1;          // the last column's bitmap word
    lds[bitmap_end + 2 * nwords + 1] = 1;                        // wrank[nwords]: the total
    if (max_l > 0) lds[wrank_end + max_l - 1] = 1;               // the last base's mask
    EXPECT(bytes <= kIdentityMaxLds || width > 524288u || max_l > 10240u);
}

int main() {
    // ---- LDS bytes at the widths where the word count steps
    EXPECT(identity_lds_bytes(1, 1) == 4 + 2 * 3 + 16 + 16);
    EXPECT(identity_lds_bytes(31, 1) == identity_lds_bytes(1, 1));
    EXPECT(identity_lds_bytes(32, 1) == identity_lds_bytes(31, 1));
    EXPECT(identity_lds_bytes(33, 1) == identity_lds_bytes(32, 1) + 6);
    EXPECT(identity_lds_bytes(524288, 10240) == 65536 + 2 * 16386 + 10255 + 16);
    EXPECT(identity_lds_bytes(524288, 10240) == 108579 && identity_lds_bytes(524288, 10240) > 64 * 1024);
    EXPECT(identity_lds_bytes(524288, 10240) <= kIdentityMaxLds && kIdentityMaxLds <= 160 * 1024);
    EXPECT(identity_lds_bytes(3200, 300) == 400 + 204 + 315 + 16);
    for (uint32_t w : {1u, 31u, 32u, 33u, 524288u})
        for (uint32_t l : {0u, 1u, 15u, 16u, 17u, 300u, 10240u}) check_layout(w, l);
    // (monotone in both)
    for (uint32_t w = 1; w < 200; w++) EXPECT(identity_lds_bytes(w + 1, 50) >= identity_lds_bytes(w, 50));
    for (uint32_t l = 0; l < 200; l++) EXPECT(identity_lds_bytes(100, l + 1) == identity_lds_bytes(100, l) + 1);

    // ---- the grid: one workgroup per query
    EXPECT(identity_grid(0) == 0);
    EXPECT(identity_grid(1) == 1);
    EXPECT(identity_grid(3072) == 3072);
    EXPECT(identity_grid(0xFFFFFFFFu) == 0xFFFFFFFFu);
    EXPECT(kIdentityThreads == 256);

    // ---- the rows
    EXPECT(identity_row_bytes(0) == 0 && identity_row_bytes(1) == 8);
    EXPECT(identity_row_bytes(0xFFFFFFFFu) == 8ull * 0xFFFFFFFFull);  // (no 32-bit overflow)

    // ---- whether a call counts: all four, nothing less
    for (int m = 0; m < 16; m++) {
        const bool on = m & 1, assemble = m & 2, fam = m & 4, some = m & 8;
        EXPECT(identity_call_counts(on, assemble, fam, some ? 7u : 0u) == (m == 15));
    }

    if (fails) {
        printf("identity_plan_check: %d checks failed\n", fails);
        return 1;
    }
    printf("identity_plan_check: ok\n");
    return 0;
}
