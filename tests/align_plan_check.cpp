// csrc/host/align_plan.h -- which DP jobs of a batch go to the device in which call: routes, groups and their order,
// weight sets, the in-place counting switches -- as a stand-alone program: tests/test_align_plan_cpu.py builds it with
// the address and undefined-behaviour sanitizers and runs it once.
//
// Two parts.  The hand-written cases carry their expected groups literally; they are what pins the behaviour.  The
// sweep compares the plan, over the combinations of the switches and every batch of up to four jobs out of a dozen
// kinds (see sweep()), with `restated` below -- which is a TRANSCRIPTION of the loop aligner::align_batch had before the plan was
// taken out of it (a std::map over tuples, bare numbers and all), not an independent oracle: it shows that nothing
// changed on the way, and the properties asserted beside it (a partition, in job order, keys ascending) hold whatever
// the rules are.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "host/align_plan.h"

using namespace sina;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            fails++;                                                  \
        }                                                             \
    } while (0)

// two filters' identities (the plan compares the pointers and never reads through them), and two widths
static const char filter_a = 'a', filter_b = 'b';
static const void *const A = &filter_a, *const B = &filter_b;
static const size_t W1 = 100, W2 = 200;
static const size_t LMAX = SINA_HIP_MAX_QUERY_LEN;

static align_job_facts job(size_t family_size, size_t query_len, size_t weight_width = 0, const void *filter = nullptr) {
    align_job_facts j;
    j.family_size = family_size;
    j.query_len = query_len;
    j.weight_width = weight_width;
    j.filter = filter;
    return j;
}

// the groups as text, "(width,filter,route)[members] ..." in the order of the device calls
static std::string show(const std::vector<align_group> &groups) {
    std::string s;
    for (const align_group &g : groups) {
        if (!s.empty()) s += " ";
        s += "(" + std::to_string(g.key.weight_width) + "," + std::to_string(g.key.filter) + "," + std::to_string((int)g.key.route) + ")[";
        for (size_t x = 0; x < g.members.size(); x++) s += (x ? "," : "") + std::to_string(g.members[x]);
        s += "]";
    }
    return s;
}
static std::string plan(const align_switches &s, const std::vector<align_job_facts> &jobs) {
    return show(plan_groups(s, jobs.data(), jobs.size()));
}
#define EXPECT_PLAN(switches, jobs, want)                                                          \
    do {                                                                                           \
        const std::string got_ = plan(switches, jobs);                                             \
        if (got_ != (want)) {                                                                      \
            printf("FAILED line %d: got %s, want %s\n", __LINE__, got_.c_str(), want);             \
            fails++;                                                                               \
        }                                                                                          \
    } while (0)

static void constants_and_order() {
    EXPECT(kDeviceFamilyMax == 128);
    EXPECT(kAnyFilter == -2 && kNoFilter == -1);
    EXPECT(route_host_graphs == 0 && route_device == 1 && route_long == 2);
    // width first, then the filter (any < none < numbered), then the route
    const align_group_key a{0, kNoFilter, route_long}, b{100, kAnyFilter, route_host_graphs}, c{100, kNoFilter, route_host_graphs},
        d{100, 0, route_host_graphs}, e{100, 0, route_device}, f{100, 1, route_host_graphs};
    EXPECT(a < b && b < c && c < d && d < e && e < f);
    EXPECT(!(b < a) && !(e < d) && !(d < d) && d == d && !(d == e));
}

static void directed_groups() {
    const align_switches dflt;  // device-graph and weight-sets on, everything else off: the aligner's defaults
    EXPECT(dflt.device_graph && dflt.weight_sets && !dflt.fs_no_graph && !dflt.device_profile && !dflt.wide_fallback);
    EXPECT(!dflt.device_bps && !dflt.device_idty && !dflt.calc_idty);

    EXPECT_PLAN(dflt, {}, "");  // the empty batch: no groups

    // the family limit of device-built DAGs
    EXPECT_PLAN(dflt, {job(128, 1500)}, "(0,-1,1)[0]");
    EXPECT_PLAN(dflt, {job(129, 1500)}, "(0,-1,0)[0]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(128, 1500), job(129, 1500), job(1, 1500)}), "(0,-1,0)[1] (0,-1,1)[0,2]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(128, 1500, W1, A), job(129, 1500, W1, A)}), "(100,-2,1)[0] (100,0,0)[1]");

    // device-graph off: everything over host graphs, weighted jobs by their filter
    align_switches host = dflt;
    host.device_graph = false;
    EXPECT_PLAN(host, (std::vector<align_job_facts>{job(40, 1500), job(40, 1500, W1, A), job(129, 1500), job(40, 1500, W1, B)}),
                "(0,-1,0)[0,2] (100,0,0)[1] (100,1,0)[3]");

    // the query limit: at it a job stays in its group, one base over it takes the long route -- also when it is
    // weighted and weight-sets is on (the long group is its filter's own)
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, LMAX), job(40, LMAX + 1)}), "(0,-1,1)[0] (0,-1,2)[1]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, LMAX, W1, A), job(40, LMAX + 1, W1, A)}), "(100,-2,1)[0] (100,0,2)[1]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(129, LMAX + 1, W1, A), job(129, LMAX, W1, A)}), "(100,0,0)[1] (100,0,2)[0]");
    EXPECT_PLAN(host, (std::vector<align_job_facts>{job(40, LMAX + 1)}), "(0,-1,2)[0]");
    align_switches wide = dflt;
    wide.wide_fallback = true;
    EXPECT_PLAN(wide, (std::vector<align_job_facts>{job(40, LMAX, W1, A), job(40, LMAX + 1, W1, A)}), "(100,0,1)[0] (100,0,2)[1]");

    // fs-no-graph: no positional weights whatever the filters, and the device route only with device-profile
    align_switches prof = dflt;
    prof.fs_no_graph = true;
    const std::vector<align_job_facts> weighted{job(128, 1500, W1, A), job(129, 1500, W1, B), job(40, 1500, W2, B), job(40, LMAX + 1, W1, A)};
    EXPECT_PLAN(prof, weighted, "(0,-1,0)[0,1,2] (0,-1,2)[3]");
    prof.device_profile = true;
    EXPECT_PLAN(prof, weighted, "(0,-1,0)[1] (0,-1,1)[0,2] (0,-1,2)[3]");
    prof.device_graph = false;
    EXPECT_PLAN(prof, weighted, "(0,-1,0)[0,1,2] (0,-1,2)[3]");
    align_switches dev_prof = dflt;  // device-profile without fs-no-graph changes nothing
    dev_prof.device_profile = true;
    EXPECT_PLAN(dev_prof, weighted, "(100,-2,1)[0] (100,0,0)[1] (100,1,2)[3] (200,-2,1)[2]");

    // two filters of one width: one any-filter group with weight-sets, one group per filter -- numbered by first
    // appearance -- without it or with wide-fallback; two widths: two groups either way
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, 1500, W1, A), job(40, 1500, W1, B)}), "(100,-2,1)[0,1]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, 1500, W1, A), job(40, 1500, W2, B)}), "(100,-2,1)[0] (200,-2,1)[1]");
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, 1500, W2, A), job(40, 1500, W1, B)}), "(100,-2,1)[1] (200,-2,1)[0]");
    align_switches per_filter = dflt;
    per_filter.weight_sets = false;
    const std::vector<align_job_facts> bab{job(40, 1500, W1, B), job(40, 1500, W1, A), job(40, 1500, W1, B)};
    EXPECT_PLAN(dflt, bab, "(100,-2,1)[0,1,2]");
    EXPECT_PLAN(per_filter, bab, "(100,0,1)[0,2] (100,1,1)[1]");
    EXPECT_PLAN(wide, bab, "(100,0,1)[0,2] (100,1,1)[1]");
    EXPECT_PLAN(per_filter, (std::vector<align_job_facts>{job(40, 1500, W1, A), job(40, 1500, W2, B)}), "(100,0,1)[0] (200,1,1)[1]");
    // (a number is given when a job needs one: the any-filter job of filter A brings none, so B is 0 and A is 1)
    EXPECT_PLAN(dflt, (std::vector<align_job_facts>{job(40, 1500, W1, A), job(129, 1500, W1, B), job(129, 1500, W1, A)}),
                "(100,-2,1)[0] (100,0,0)[1] (100,1,0)[2]");

    // a mixed batch: simple, weighted, long and oversize families, in the order of the device calls
    const std::vector<align_job_facts> mixed{job(40, 1500),          job(40, 1500, W1, A), job(40, LMAX + 1), job(129, 1500),
                                             job(40, 1500, W1, B),   job(40, LMAX + 1, W1, A), job(200, 1500, W1, A)};
    EXPECT_PLAN(wide, mixed, "(0,-1,0)[3] (0,-1,1)[0] (0,-1,2)[2] (100,0,0)[6] (100,0,1)[1] (100,0,2)[5] (100,1,1)[4]");
    EXPECT_PLAN(dflt, mixed, "(0,-1,0)[3] (0,-1,1)[0] (0,-1,2)[2] (100,-2,1)[1,4] (100,0,0)[6] (100,0,2)[5]");
    EXPECT_PLAN(host, mixed, "(0,-1,0)[0,3] (0,-1,2)[2] (100,0,0)[1,6] (100,0,2)[5] (100,1,0)[4]");
}

static void directed_weight_sets() {
    auto numbered = [](const std::vector<const void *> &filters) {
        return number_weight_sets(filters.size(), [&](size_t u) { return filters[u]; });
    };
    weight_sets w = numbered({A, B, A});
    EXPECT(w.set_of == (std::vector<uint32_t>{0, 1, 0}) && w.n_sets() == 2 && w.first_slot == (std::vector<uint32_t>{0, 1}));
    w = numbered({B, B, A, A, B});
    EXPECT(w.set_of == (std::vector<uint32_t>{0, 0, 1, 1, 0}) && w.n_sets() == 2 && w.first_slot == (std::vector<uint32_t>{0, 2}));
    w = numbered({A, A, A});  // one filter after all: the call without sets
    EXPECT(w.set_of.empty() && w.n_sets() == 1 && w.first_slot == (std::vector<uint32_t>{0}));
    w = numbered({B});
    EXPECT(w.set_of.empty() && w.n_sets() == 1 && w.first_slot == (std::vector<uint32_t>{0}));
}

// the two counting switches over everything they read -- and over the switches they do not
static void counting_truth_table() {
    align_switches on;
    on.device_bps = on.device_idty = on.calc_idty = true;
    align_counting c = plan_counting(on, route_device, true, true, true);
    EXPECT(c.count_pairs && c.count_idty);
    c = plan_counting(on, route_host_graphs, true, true, true);
    EXPECT(c.count_pairs && !c.count_idty);  // host-built graphs bring no families to the device
    c = plan_counting(on, route_long, true, true, true);
    EXPECT(!c.count_pairs && !c.count_idty);  // the wide path assembles nothing
    c = plan_counting(on, route_device, false, true, true);
    EXPECT(!c.count_pairs && c.count_idty);  // a single tray: its sink walks; its identity is counted all the same
    c = plan_counting(on, route_device, true, false, true);
    EXPECT(!c.count_pairs && c.count_idty);  // no helix map
    c = plan_counting(on, route_device, true, true, false);
    EXPECT(!c.count_pairs && !c.count_idty);  // a call that does not assemble
    c = plan_counting(align_switches(), route_device, true, true, true);
    EXPECT(!c.count_pairs && !c.count_idty);  // the defaults count nothing
    unsigned n = 0, n_pairs = 0, n_idty = 0;
    for (unsigned bits = 0; bits < 256; bits++)
        for (int route = 0; route < 3; route++)
            for (unsigned rest = 0; rest < 8; rest++) {
                align_switches s;
                s.fs_no_graph = bits & 1, s.device_graph = bits & 2, s.device_profile = bits & 4, s.wide_fallback = bits & 8;
                s.weight_sets = bits & 16, s.device_bps = bits & 32, s.device_idty = bits & 64, s.calc_idty = bits & 128;
                const bool batch_driver = rest & 1, has_map = rest & 2, assembles = rest & 4;
                c = plan_counting(s, (align_route)route, batch_driver, has_map, assembles);
                EXPECT(c.count_pairs == ((bits & 32) && batch_driver && has_map && assembles && route != 2));
                EXPECT(c.count_idty == ((bits & 64) && (bits & 128) && assembles && route == 1));
                n++, n_pairs += c.count_pairs, n_idty += c.count_idty;
            }
    // (of 256 x 3 x 8 rows: device-bps halves them, two of three routes, one of eight of the rest; device-idty and
    // calc-idty quarter them, one of three routes, assembling halves the rest)
    EXPECT(n == 6144 && n_pairs == 128 * 2 * 1 && n_idty == 64 * 1 * 4);
}

// The loop of the parent commit's aligner::align_batch, transcribed: jobs[i] for its dp_job, o for its options.
using old_key = std::tuple<size_t, int, int>;
static std::map<old_key, std::vector<uint32_t>> restated(const align_switches &o, const std::vector<align_job_facts> &jobs) {
    enum route { route_host_graphs = 0, route_device = 1, route_long = 2 };
    std::vector<const void *> filters_seen;
    auto filter_no = [&](const void *a) {
        for (size_t x = 0; x < filters_seen.size(); x++)
            if (filters_seen[x] == a) return (int)x;
        filters_seen.push_back(a);
        return (int)filters_seen.size() - 1;
    };
    std::map<old_key, std::vector<uint32_t>> groups;
    for (size_t i = 0; i < jobs.size(); i++) {
        const bool on_device = o.device_graph && jobs[i].family_size <= 128;
        const bool is_long = jobs[i].query_len > SINA_HIP_MAX_QUERY_LEN;
        const size_t w = jobs[i].weight_width;
        if (o.fs_no_graph || w == 0) {
            const int r = is_long ? route_long : on_device && (!o.fs_no_graph || o.device_profile) ? route_device : route_host_graphs;
            groups[{0, -1, r}].push_back((uint32_t)i);
        } else {
            const int r = is_long ? route_long : on_device ? route_device : route_host_graphs;
            const bool any = r == route_device && o.weight_sets && !o.wide_fallback;
            groups[{w, any ? -2 : filter_no(jobs[i].filter), r}].push_back((uint32_t)i);
        }
    }
    return groups;
}

static uint64_t sweep_one(const align_switches &s, const std::vector<align_job_facts> &jobs) {
    const std::vector<align_group> got = plan_groups(s, jobs.data(), jobs.size());
    const std::map<old_key, std::vector<uint32_t>> want = restated(s, jobs);
    bool same = got.size() == want.size();
    size_t x = 0;
    for (auto it = want.begin(); same && it != want.end(); ++it, ++x)
        same = old_key(got[x].key.weight_width, got[x].key.filter, (int)got[x].key.route) == it->first && got[x].members == it->second;
    // every job in exactly one group, members in job order, keys strictly ascending
    std::vector<int> seen(jobs.size(), 0);
    bool partition = true, ordered = true;
    for (size_t g = 0; g < got.size(); g++) {
        if (got[g].members.empty()) partition = false;
        for (size_t m = 0; m < got[g].members.size(); m++) {
            if (got[g].members[m] >= jobs.size()) {
                partition = false;
                continue;
            }
            seen[got[g].members[m]]++;
            if (m && got[g].members[m - 1] >= got[g].members[m]) ordered = false;
        }
        if (g && !(got[g - 1].key < got[g].key)) ordered = false;
    }
    for (int n : seen) partition = partition && n == 1;
    if (!(same && partition && ordered)) {
        if (fails < 20) printf("FAILED sweep: %zu jobs, same %d partition %d ordered %d: %s\n", jobs.size(), same, partition, ordered, show(got).c_str());
        fails++;
    }
    return got.size();
}

// Every combination of the switches x every batch of zero to four jobs out of twelve kinds: family size at and over
// the family limit, length at and over the query limit, no weights or one of two widths, filter A or B.  Batches of up
// to two jobs take all 256 combinations of the eight switches; those of three and four jobs -- 22 464 of them -- take
// the 32 combinations of the five switches the grouping reads, the three counting switches going through their eight
// values from batch to batch: the full product is six million plans, a minute under the sanitizers.
static void sweep() {
    const align_job_facts kinds[12] = {
        job(128, LMAX),        job(129, LMAX),        job(128, LMAX + 1),        job(129, LMAX + 1),
        job(128, LMAX, W1, A), job(128, LMAX, W1, B), job(129, LMAX, W1, A),     job(128, LMAX + 1, W1, B),
        job(128, LMAX, W2, A), job(129, LMAX, W2, B), job(128, LMAX + 1, W2, A), job(129, LMAX + 1, W1, B),
    };
    uint64_t batches = 0, groups = 0;
    std::vector<align_job_facts> jobs;
    for (unsigned bits = 0; bits < 256; bits++) {
        align_switches s;
        s.fs_no_graph = bits & 1, s.device_graph = bits & 2, s.device_profile = bits & 4, s.wide_fallback = bits & 8;
        s.weight_sets = bits & 16, s.device_bps = bits & 32, s.device_idty = bits & 64, s.calc_idty = bits & 128;
        for (size_t n = 0; n <= (bits < 32 ? 4 : 2); n++) {
            size_t total = 1;
            for (size_t k = 0; k < n; k++) total *= 12;
            for (size_t code = 0; code < total; code++) {
                jobs.clear();
                for (size_t k = 0, c = code; k < n; k++, c /= 12) jobs.push_back(kinds[c % 12]);
                if (n > 2) s.device_bps = code & 1, s.device_idty = code & 2, s.calc_idty = code & 4;
                groups += sweep_one(s, jobs);
                batches++;
            }
        }
    }
    EXPECT(batches == 256ull * (1 + 12 + 144) + 32ull * (1728 + 20736));
    EXPECT(groups > batches);  // (most batches have more than one group)
}

int main() {
    constants_and_order();
    directed_groups();
    directed_weight_sets();
    counting_truth_table();
    sweep();
    if (fails) {
        printf("align_plan_check: %d FAILED\n", fails);
        return 1;
    }
    printf("align_plan_check: ok\n");
    return 0;
}
