// What the aligner sends to the device in which call: the route of a DP job, the groups of a batch and their order,
// the weight sets of a several-filter group, and whether a group's call counts or ranks in place.  Header-only; no HIP, no
// stages.h, no cseq.h, no globals, no environment: a stand-alone program can include it (tests/align_plan_check.cpp).
// aligner.cpp fills the switches and the jobs' facts and runs one device call per group, in the order given here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "sina_hip.h"  // SINA_HIP_MAX_QUERY_LEN

// (hidden: a shared library that includes this exports none of it)
namespace sina __attribute__((visibility("hidden"))) {

// the aligner's options as far as the plan reads them (aligner::options; filled in one place, aligner.cpp)
struct align_switches {
    bool fs_no_graph = false, device_graph = true, device_profile = false, wide_fallback = false, weight_sets = true;
    bool device_bps = false, device_idty = false, calc_idty = false;
    bool device_shift = false;  // the align call runs with assemble = SINA_ASSEMBLE_SHIFT: see align_assemble_mode
    bool device_search = false;  // the align call ranks the search stage's candidates where it assembles: see plan_search_inplace
};

// What sina_hip_align_params::assemble is for a group's call: the device finishes the insertions that shift their
// neighbours too where the option asks for it.  Every route takes the value (the wide path assembles nothing either way);
// plan_counting's `assembles` input is this != 0, so device-bps and device-idty score shifted trays from the same call.
inline int align_assemble_mode(const align_switches &s) { return s.device_shift ? SINA_ASSEMBLE_SHIFT : 1; }

// what the plan reads of one DP job
struct align_job_facts {
    size_t family_size = 0;
    size_t query_len = 0;
    size_t weight_width = 0;       // of its filter's positional weights; 0: none (the simple scheme)
    const void *filter = nullptr;  // the filter's IDENTITY (the trays point at the store's filters): compared, never read
};

// Where a family's DAG is built: on the device (families of up to kDeviceFamilyMax members: the DAG-build kernel's LDS
// tables) or, for the rare larger family (--fs-max beyond 128), by the host twin of that kernel (build_family_graph)
// and handed over as a graph (sina_hip_align_graphs).
constexpr size_t kDeviceFamilyMax = 128;

// ... and, with wide-fallback, the long route: a query beyond the fast DP path's SINA_HIP_MAX_QUERY_LEN is taken out of
// its group up front -- size alone decides it -- into a group of host-built graphs that go one by one through
// sina_hip_align_graphs_any (the wide kernel).  Left in a device-built group, the limit refusal of
// sina_hip_align_families / _profiles would send the whole group, thousands of ordinary queries, back over host-built
// graphs.  (Only wide-fallback lets such a query reach the plan: prepare_tray.)
enum align_route { route_host_graphs = 0, route_device = 1, route_long = 2 };

// (--fs-no-graph: the family as a profile, built by build_family_profile on the host or -- with device-profile on,
// under the conditions a DAG is built on the device -- by sina_hip_align_profiles)
inline align_route route_of(const align_switches &s, const align_job_facts &j) {
    if (j.query_len > SINA_HIP_MAX_QUERY_LEN) return route_long;
    const bool on_device = s.device_graph && j.family_size <= kDeviceFamilyMax;
    return on_device && (!s.fs_no_graph || s.device_profile) ? route_device : route_host_graphs;
}

// A group's key: the scheme -- the width of the positional weights, 0 = simple (default-constructed astats,
// src/align.cpp:404-416; scoring_scheme_profile takes none either, :428-433) --, the filter and the route.  The filter
// is numbered by first appearance in the batch, or one of the two constants.  Groups go to the device in ascending
// order of (weight_width, filter, route).
constexpr int kAnyFilter = -2;  // the weighted jobs of this width whatever their filter (weight sets)
constexpr int kNoFilter = -1;   // no positional weights
struct align_group_key {
    size_t weight_width = 0;
    int filter = kNoFilter;
    align_route route = route_host_graphs;
    bool operator<(const align_group_key &o) const {
        return std::tie(weight_width, filter, route) < std::tie(o.weight_width, o.filter, o.route);
    }
    bool operator==(const align_group_key &o) const {
        return weight_width == o.weight_width && filter == o.filter && route == o.route;
    }
};

struct align_group {
    align_group_key key;
    std::vector<uint32_t> members;  // indices into the jobs, ascending
};

// Takes the DP jobs of a batch; gives its groups in the order of their device calls, every job in exactly one.
// weight-sets: the weighted jobs on the device route whose filters have the same width are ONE group whatever the
// filter (kAnyFilter) -- one DAG build and one DP launch for a batch whose queries chose several
// (sina_hip_align_families_wsets).  Not with wide-fallback, whose second route (host-built graphs after a limit
// refusal) takes one vector per call.  Every other weighted job is grouped by its filter, the filters numbered as the
// jobs that need a number bring them up.
inline std::vector<align_group> plan_groups(const align_switches &s, const align_job_facts *jobs, size_t n_jobs) {
    std::vector<uint32_t> numbered;  // [filter number] the job that brought the filter up
    auto filter_no = [&](size_t i) {
        for (size_t x = 0; x < numbered.size(); x++)
            if (jobs[numbered[x]].filter == jobs[i].filter) return (int)x;
        numbered.push_back((uint32_t)i);
        return (int)numbered.size() - 1;
    };
    std::map<align_group_key, std::vector<uint32_t>> by_key;
    for (size_t i = 0; i < n_jobs; i++) {
        const align_job_facts &j = jobs[i];
        align_group_key key;
        key.route = route_of(s, j);
        if (!s.fs_no_graph && j.weight_width != 0) {
            const bool any = key.route == route_device && s.weight_sets && !s.wide_fallback;
            key.weight_width = j.weight_width;
            key.filter = any ? kAnyFilter : filter_no(i);
        }
        by_key[key].push_back((uint32_t)i);
    }
    std::vector<align_group> groups;
    groups.reserve(by_key.size());
    for (auto &g : by_key) groups.push_back({g.first, std::move(g.second)});
    return groups;
}

// The weight sets of a several-filter group, from the filters of its slots filter_of(u) in slot order: set_of[u] =
// number of slot u's filter among the distinct ones, numbered by first appearance, and first_slot[x] = the slot that
// brought set x up.  One filter after all: set_of is empty (the call without sets).
struct weight_sets {
    std::vector<uint32_t> set_of;
    std::vector<uint32_t> first_slot;
    uint32_t n_sets() const { return (uint32_t)first_slot.size(); }
};
template <class FilterOf> weight_sets number_weight_sets(size_t n_slots, FilterOf &&filter_of) {
    weight_sets w;
    w.set_of.resize(n_slots);
    for (size_t u = 0; u < n_slots; u++) {
        size_t x = 0;
        while (x < w.first_slot.size() && filter_of(w.first_slot[x]) != filter_of(u)) x++;
        if (x == w.first_slot.size()) w.first_slot.push_back((uint32_t)u);
        w.set_of[u] = (uint32_t)x;
    }
    if (w.first_slot.size() <= 1) w.set_of.clear();
    return w;
}

// Whether a group's align call counts in place (the switches are set on the leased context either way: it keeps the
// switch of whoever had it before).
//   count_pairs (device-bps): the helix base pairs of the queries the call assembles.  Never for the one-slot calls of
//     the long route (the wide path assembles nothing) or a single tray (batch_driver false: its sink takes the host
//     walk, as before), and only if the store has a helix map.
//   count_idty (device-idty): the queries the call assembles scored against their families.  Only a group whose
//     families go to the device can count (the batch driver's and a single tray's alike), and without calc-idty
//     nothing is launched.
struct align_counting {
    bool count_pairs = false, count_idty = false;
};
inline align_counting plan_counting(const align_switches &s, align_route route, bool batch_driver, bool has_pair_map, bool assembles) {
    align_counting c;
    c.count_pairs = s.device_bps && batch_driver && route != route_long && has_pair_map && assembles;
    c.count_idty = s.calc_idty && s.device_idty && route == route_device && assembles;
    return c;
}

// Whether a group's align call also ranks the search stage's k-mer candidates against the words it assembles
// (device-search; sina_hip_align_rank).  What the aligner reads of the search stage and of the store, in one place:
struct search_stage_facts {
    bool correction_none = false;  // search-correction none (Jukes-Cantor: rounding can merge ratios into ties)
    bool ignore_super = false;     // search-ignore-super
    bool search_all = false;       // search-all (every reference is a candidate: sina_hip_compare_rank serves it)
    int max_result = 0;            // search-max-result
    uint64_t candidates = 0;       // min(search-kmer-candidates, references of the store)
    bool name_order = false;       // the store's name order is on the device (no two references share a name)
    bool same_store = false;       // search-db names the aligner's store
    bool index_matches = false;    // that store's index is the one search-kmer-len / search-no-fast ask for
};
constexpr int kSearchInplaceMaxResult = 64;            // rows of a query's staged row (rank_plan.h, kRankMaxResult)
constexpr uint64_t kSearchInplaceMaxCandidates = 4096;  // what the k-mer search's LDS select sorts (kmer_plan.h, kKmerSelMax)
// The stage's options are those its own device ranking accepts (search_filter.cpp, device_rank), the candidates and
// the comparison must be over the aligner's store, and the call must assemble: the rows are of finished words.  Never
// for the one-slot calls of the long route (the wide path assembles nothing).  A group that does not rank leaves
// its trays to the search stage's own path, as does every tray of a ranking group whose row says "not ranked".
inline bool plan_search_inplace(const align_switches &s, align_route route, bool assembles, const search_stage_facts &f) {
    return s.device_search && route != route_long && assembles && f.correction_none && !f.ignore_super && !f.search_all &&
           f.max_result >= 1 && f.max_result <= kSearchInplaceMaxResult && f.candidates <= kSearchInplaceMaxCandidates &&
           f.name_order && f.same_store && f.index_matches;
}

}  // namespace sina
