// plan_search_inplace (sina_amd/csrc/host/align_plan.h): whether a group's align call ranks the search stage's
// candidates in place -- every precondition's truth table, and the limits at their edges.  Stand-alone, no GPU;
// tests/test_search_inplace_cpu.py builds it with the address sanitizer and runs it.
#include <cstdio>
#include <cstdlib>

#include "host/align_plan.h"

using namespace sina;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static search_stage_facts good() {
    search_stage_facts f;
    f.correction_none = true;
    f.ignore_super = false;
    f.search_all = false;
    f.max_result = 10;
    f.candidates = 1000;
    f.name_order = f.same_store = f.index_matches = true;
    return f;
}

int main() {
    align_switches on;
    on.device_search = true;
    const align_switches off;
    CHECK(!off.device_search);  // off by default
    // everything in place: both fast routes rank, the long route never does
    CHECK(plan_search_inplace(on, route_device, true, good()));
    CHECK(plan_search_inplace(on, route_host_graphs, true, good()));
    CHECK(!plan_search_inplace(on, route_long, true, good()));
    // the truth table: eleven conditions, a group ranks if and only if all hold
    int ranked = 0;
    for (unsigned bits = 0; bits < (1u << 11); bits++) {
        align_switches s;
        s.device_search = bits & 1u;
        const align_route route = (bits & 2u) ? route_device : route_long;
        const bool assembles = bits & 4u;
        search_stage_facts f;
        f.correction_none = bits & 8u;
        f.ignore_super = !(bits & 16u);
        f.search_all = !(bits & 32u);
        f.max_result = (bits & 64u) ? 10 : 65;
        f.candidates = (bits & 128u) ? 4096 : 4097;
        f.name_order = bits & 256u;
        f.same_store = bits & 512u;
        f.index_matches = bits & 1024u;
        const bool want = bits == (1u << 11) - 1;
        CHECK(plan_search_inplace(s, route, assembles, f) == want);
        ranked += plan_search_inplace(s, route, assembles, f) ? 1 : 0;
    }
    CHECK(ranked == 1);
    // every condition alone switches it off
    {
        search_stage_facts f = good();
        f.correction_none = false;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        f = good(), f.ignore_super = true;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        f = good(), f.search_all = true;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        f = good(), f.name_order = false;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        f = good(), f.same_store = false;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        f = good(), f.index_matches = false;
        CHECK(!plan_search_inplace(on, route_device, true, f));
        CHECK(!plan_search_inplace(on, route_device, false, good()));
        CHECK(!plan_search_inplace(off, route_device, true, good()));
    }
    // the limits at their edges: search-max-result in 1..64, at most 4096 candidates after clamping to the store
    for (int n : {-1, 0, 1, 64, 65, 1000}) {
        search_stage_facts f = good();
        f.max_result = n;
        CHECK(plan_search_inplace(on, route_device, true, f) == (n >= 1 && n <= 64));
    }
    for (uint64_t c : {uint64_t(0), uint64_t(1), uint64_t(4096), uint64_t(4097), uint64_t(1) << 40}) {
        search_stage_facts f = good();
        f.candidates = c;
        CHECK(plan_search_inplace(on, route_device, true, f) == (c <= 4096));
    }
    CHECK(kSearchInplaceMaxResult == 64 && kSearchInplaceMaxCandidates == 4096);
    // the other switches do not matter, and the new one leaves the counting plan alone
    align_switches all = on;
    all.device_bps = all.device_idty = all.calc_idty = all.device_shift = all.fs_no_graph = all.device_profile = true;
    CHECK(plan_search_inplace(all, route_device, true, good()));
    CHECK(align_assemble_mode(on) == 1 && align_assemble_mode(all) == SINA_ASSEMBLE_SHIFT);
    const align_counting c = plan_counting(on, route_device, true, true, true);
    CHECK(!c.count_pairs && !c.count_idty);
    if (failures) return 1;
    std::printf("search_plan_check: ok\n");
    return 0;
}
