// Host side of the boundary: cseq_comparator, search_filter and the helix base-pair score of a batch.
// Behaviour follows the reference (citations inline); the comparisons go through the C ABI (include/sina_hip.h).
#include "stages_internal.h"
#include "../kmer_plan.h"
#include "../rank_plan.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <map>

namespace sina {

// ================================================================ cseq_comparator (src/cseq_comparator.cpp)

// The six counters cseq_comparator derives its score from (behaviour of src/cseq_comparator.cpp:
// 56-111,165-206), stated by column membership like compare_kernel (search.hip) states them: a
// filtered (lower-case, with filter_lowercase) base is as good as absent; a base outside the column
// range of the other sequence's remaining bases is "overhang"; inside it, it has a partner in the
// same column (match / mismatch by the IUPAC rule) or it has none.  A side without any remaining
// base gives all-zero counters.  Host version for single pairs and the CPU-side tests; batches go
// through sina_hip_compare.
void cseq_comparator::counts(const cseq &A, const cseq &B, CMP_IUPAC_TYPE iupac, bool filter_lc,
                             sina_hip_match_counts *m) {
    memset(m, 0, sizeof(*m));
    auto remaining = [&](const cseq &s) {
        std::vector<aligned_base> v;
        v.reserve(s.size());
        for (const aligned_base &x : s.getAlignedBases())
            if (!(filter_lc && x.getBase().isLowerCase())) v.push_back(x);
        return v;
    };
    const std::vector<aligned_base> a = remaining(A), b = remaining(B);
    if (a.empty() || b.empty()) return;
    auto same = [&](const aligned_base &x, const aligned_base &y) {
        const base_iupac p = x.getBase(), q = y.getBase();
        return iupac == CMP_IUPAC_OPTIMISTIC ? p.comp(q) : (iupac == CMP_IUPAC_PESSIMISTIC ? p.comp_pessimistic(q) : p.comp_exact(q));
    };
    const uint32_t a_lo = a.front().getPosition(), a_hi = a.back().getPosition();
    const uint32_t b_lo = b.front().getPosition(), b_hi = b.back().getPosition();
    size_t i = 0, j = 0;  // columns ascend on both sides: one merge
    while (i < a.size() || j < b.size()) {
        const uint32_t pa = i < a.size() ? a[i].getPosition() : 0xFFFFFFFFu;
        const uint32_t pb = j < b.size() ? b[j].getPosition() : 0xFFFFFFFFu;
        if (pa == pb) {
            if (same(a[i], b[j])) m->match++;
            else m->mismatch++;
            i++;
            j++;
        } else if (pa < pb) {
            if (pa < b_lo || pa > b_hi) m->only_a_overhang++;
            else m->only_a++;
            i++;
        } else {
            if (pb < a_lo || pb > a_hi) m->only_b_overhang++;
            else m->only_b++;
            j++;
        }
    }
}

// match fraction over the cover rule's denominator, optionally Jukes-Cantor corrected (behaviour of
// src/cseq_comparator.cpp:240-296, :42-44)
float cseq_comparator::score(const sina_hip_match_counts &m) const {
    const int paired = m.match + m.mismatch;
    const int a_alone = m.only_a + m.only_a_overhang, b_alone = m.only_b + m.only_b_overhang;
    int denom = 0;
    switch (cover_rule) {
    case CMP_COVER_ABS: denom = 1; break;
    case CMP_COVER_QUERY: denom = paired + a_alone; break;
    case CMP_COVER_TARGET: denom = paired + b_alone; break;
    case CMP_COVER_OVERLAP: denom = paired + m.only_a + m.only_b; break;
    case CMP_COVER_ALL: denom = paired + m.only_a + m.only_b + m.only_a_overhang + m.only_b_overhang; break;
    case CMP_COVER_AVERAGE: denom = paired + (m.only_a + m.only_b + m.only_a_overhang + m.only_b_overhang) / 2; break;
    case CMP_COVER_MIN: denom = paired + std::min(a_alone, b_alone); break;
    case CMP_COVER_MAX: denom = paired + std::max(a_alone, b_alone); break;
    case CMP_COVER_NOGAP: denom = paired; break;
    default: throw std::logic_error("unknown cover rule");
    }
    const float identity = (float)m.match / denom;
    if (dist_rule != CMP_DIST_JC) return identity;
    return (float)(-3.0 / 4 * log(1.0 - 4.0 / 3 * identity));
}
float cseq_comparator::operator()(const cseq &query, const cseq &target) const {
    sina_hip_match_counts m;
    counts(query, target, iupac_rule, filter_lc_rule, &m);
    return score(m);
}

// ================================================================ search_filter (src/search_filter.cpp)

const char *search_filter::fn_nearest = "nearest_slv";

struct search_filter::options {
    std::string pt_database;
    bool search_all;
    bool fs_no_fast;
    int fs_kmer_len;
    int kmer_candidates;
    float min_sim;
    bool ignore_super;
    int max_result;
    std::string lca_fields;
    std::vector<std::string> v_lca_fields;
    float lca_quorum;
    std::string copy_fields;
    std::vector<std::string> v_copy_fields;
    cseq_comparator comparator;
    bool device_rank;  // the candidates scored and ranked on the device, only the max_result best coming down (default off)
};
search_filter::options *search_filter::opts = nullptr;

static search_filter::options sf_defaults() {  // src/search_filter.cpp:91-126, cseq_comparator.cpp:434-464
    search_filter::options o;
    o.search_all = false;
    o.fs_no_fast = false;
    o.fs_kmer_len = 10;
    o.kmer_candidates = 1000;
    o.min_sim = .7f;
    o.ignore_super = false;
    o.max_result = 10;
    o.lca_quorum = .7f;
    o.device_rank = false;
    return o;
}
static search_filter::options &sf_opts() {
    if (!search_filter::opts) search_filter::opts = new search_filter::options(sf_defaults());
    return *search_filter::opts;
}
void search_filter::reset_options() { sf_opts() = sf_defaults(); }
std::string search_filter_database() { return sf_opts().pt_database; }
search_stage_request search_filter_request() {
    const search_filter::options &o = sf_opts();
    return {o.pt_database, o.search_all, o.fs_no_fast, o.ignore_super, o.comparator.dist_rule == CMP_DIST_NONE, o.comparator.filter_lc_rule,
            o.fs_kmer_len, o.kmer_candidates, o.max_result, (int)o.comparator.iupac_rule, (int)o.comparator.cover_rule};
}

void search_filter::set_option(const std::string &name, const std::string &value) {
    options &o = sf_opts();
    const std::string v = lower(value);
    if (name == "search-db" || (name == "db" && o.pt_database.empty())) o.pt_database = value;
    else if (name == "db") {}
    else if (name == "search-min-sim") o.min_sim = std::stof(value);
    else if (name == "search-max-result") o.max_result = std::stoi(value);
    else if (name == "lca-fields") o.lca_fields = value;
    else if (name == "lca-quorum") o.lca_quorum = std::stof(value);
    else if (name == "search-all") o.search_all = to_bool(value);
    else if (name == "search-no-fast") o.fs_no_fast = to_bool(value);
    else if (name == "search-kmer-candidates") o.kmer_candidates = std::stoi(value);
    else if (name == "search-kmer-len") o.fs_kmer_len = std::stoi(value);
    else if (name == "search-ignore-super") o.ignore_super = to_bool(value);
    else if (name == "search-copy-fields") o.copy_fields = value;
    else if (name == "device-rank") o.device_rank = to_bool(value);
    else if (name == "search-iupac") {  // validate(), cseq_comparator.cpp:301-318: istarts_with(name, value)
        auto starts = [&](const char *full) { return !v.empty() && std::string(full).compare(0, v.size(), v) == 0; };
        if (starts("optimistic")) o.comparator.iupac_rule = CMP_IUPAC_OPTIMISTIC;
        else if (starts("pessimistic")) o.comparator.iupac_rule = CMP_IUPAC_PESSIMISTIC;
        else if (starts("exact")) o.comparator.iupac_rule = CMP_IUPAC_EXACT;
        else throw std::logic_error("iupac matching must be either optimistic or pessimistic");
    } else if (name == "search-correction") {
        if (v == "none") o.comparator.dist_rule = CMP_DIST_NONE;
        else if (v == "jc") o.comparator.dist_rule = CMP_DIST_JC;
        else throw std::logic_error("distance correction must be either none or jc");
    } else if (name == "search-cover") {
        static const char *names[] = {"abs", "query", "target", "overlap", "all", "average", "min", "max", "nogap"};
        int found = -1;
        for (int i = 0; i < 9; i++)
            if (v == names[i]) found = i;
        if (found < 0)
            throw std::logic_error("coverage type must be one of abs, query, target, overlap,"
                                   "average, nogap, min or max");
        o.comparator.cover_rule = (CMP_COVER_TYPE)found;
    } else if (name == "search-filter-lowercase") o.comparator.filter_lc_rule = to_bool(value);
    else if (name == "search-engine") {
        if (v != "internal" && v != "sina_kmer" && v != "kmer")
            throw std::logic_error("search: only the internal k-mer engine is accelerated");
    } else if (name == "search-kmer-mm") {
        if (std::stoi(value) != 0) throw std::logic_error("search: --search-kmer-mm is a PT-server option");
    } else if (name == "search-kmer-norel") {
        if (to_bool(value)) throw std::logic_error("search: --search-kmer-norel is a PT-server option");
    } else throw std::logic_error("search: unknown option " + name);
}

void search_filter::validate_options() {  // src/search_filter.cpp:130-168
    options &o = sf_opts();
    if (o.pt_database.empty()) throw std::logic_error("need search-db to search");
    if (o.comparator.cover_rule == CMP_COVER_ABS && o.comparator.dist_rule != CMP_DIST_NONE)
        throw std::logic_error("only fractional identity can be distance corrected");  // cseq_comparator.cpp:476-479
    auto split = [](const std::string &s, std::vector<std::string> &out) {  // boost::split on ":,"
        out.clear();
        std::string cur;
        for (char ch : s) {
            if (ch == ':' || ch == ',') {
                out.push_back(cur);
                cur.clear();
            } else {
                cur += ch;
            }
        }
        out.push_back(cur);
        if (out.back().empty()) out.pop_back();
    };
    split(o.lca_fields, o.v_lca_fields);
    split(o.copy_fields, o.v_copy_fields);
}

struct search_filter::priv_data {
    std::shared_ptr<reference_store> arb;
    kmer_search *index = nullptr;
};

search_filter::search_filter() : data(new priv_data) {
    options &o = sf_opts();
    if (o.pt_database.empty()) throw std::logic_error("need search-db to search");
    data->arb = reference_store::get(o.pt_database);
    if (!o.search_all) data->index = kmer_search::get_kmer_search(o.pt_database, o.fs_kmer_len, o.fs_no_fast);
    // device-rank: the store's name order, computed and uploaded once (a store filled by broadcast: by the first batch)
    if (o.device_rank && !data->arb->filled_by_broadcast()) data->arb->name_order_ready();
}
search_filter::search_filter(const search_filter &) = default;
search_filter &search_filter::operator=(const search_filter &) = default;
search_filter::~search_filter() = default;

tray search_filter::operator()(tray t) {
    std::vector<tray> b{t};
    (*this)(b);
    return b[0];
}

namespace {
// most pairs of one comparison launch: a batch with more is compared in slices of whole queries
constexpr uint64_t kComparePairsPerSlice = 8u << 20;

// boost::algorithm::contains(ref aligned bases, query aligned bases, a.comp(b)), search_filter.cpp:264-268
bool contains_query(const cseq &ref, const cseq &q) {
    const auto &h = ref.getAlignedBases();
    const auto &n = q.getAlignedBases();
    if (n.empty()) return true;
    if (n.size() > h.size()) return false;
    for (size_t i = 0; i + n.size() <= h.size(); i++) {
        size_t j = 0;
        while (j < n.size() && h[i + j].getBase().comp(n[j].getBase())) j++;
        if (j == n.size()) return true;
    }
    return false;
}

// LCA classification (behaviour of src/search_filter.cpp:374-409): the taxonomy paths of the search
// results, in result order, vote level by level.  The first path still in the vote names the group
// of the current level; the first path that cannot follow it (it has ended, or names another group)
// is dropped from the vote -- as is the leading path itself once it has ended -- and every drop
// uses up one of the `n_results * (1 - quorum)` allowed outliers.  The vote ends when the outliers
// are used up or no path is left; what all remaining paths agreed on so far is the classification.
std::string lca_vote(const std::vector<std::vector<std::string>> &paths, size_t n_results, float quorum) {
    int outliers_left = n_results * (1 - quorum) + .5;
    std::vector<size_t> voting(paths.size());
    for (size_t i = 0; i < voting.size(); i++) voting[i] = i;
    std::string agreed;
    for (size_t level = 0; outliers_left >= 0 && !voting.empty();) {
        const std::vector<std::string> &lead = paths[voting[0]];
        size_t dissenter = voting.size();
        if (level >= lead.size()) {
            dissenter = 0;
        } else {
            for (size_t k = 1; k < voting.size() && dissenter == voting.size(); k++) {
                const std::vector<std::string> &p = paths[voting[k]];
                if (level >= p.size() || p[level] != lead[level]) dissenter = k;
            }
        }
        if (dissenter < voting.size()) {
            voting.erase(voting.begin() + (std::ptrdiff_t)dissenter);
            outliers_left--;
        } else {
            agreed += lead[level] + ";";
            level++;
        }
    }
    const bool nothing = agreed.empty() || agreed == ";" ||
                         (agreed.size() > 1 && agreed.compare(agreed.size() - 2, 2, ";;") == 0);
    return nothing ? "Unclassified;" : agreed;
}

// What the steps of a search-stage call share: the options, the store, the k-mer index (none: search-all), the batch.
struct search_call {
    const search_filter::options &o;
    reference_store &st;
    kmer_search *index;
    std::vector<tray> &batch;
    const cseq &query(size_t i) const { return *batch[i].aligned_sequence; }
};

// Takes the batch; gives the indices of the trays that are searched, each with an empty search_result -- a tray
// without a sequence, or with one of fewer than 20 bases, gets a log line instead.
std::vector<size_t> searched_trays(std::vector<tray> &batch) {
    std::vector<size_t> idx;
    for (size_t i = 0; i < batch.size(); i++) {
        tray &t = batch[i];
        if (t.aligned_sequence == nullptr) {
            t.log << "search: no sequence?!;";
            continue;
        }
        if (t.aligned_sequence->size() < 20) {
            t.log << "search:sequence too short (<20 bases);";
            continue;
        }
        t.search_result = new search::result_vector();
        idx.push_back(i);
    }
    return idx;
}

// Takes trays `sub` (indices into the batch); gives each its k-mer candidates, unscored: one find_batch for all, then
// --search-ignore-super keeps those that contain the query.
std::vector<search::result_vector> host_candidates(const search_call &s, const std::vector<size_t> &sub) {
    scoped_phase ph("sf.find_batch");
    const size_t nq = sub.size();
    std::vector<search::result_vector> cand(nq);
    std::vector<const cseq *> qs(nq);
    for (size_t x = 0; x < nq; x++) qs[x] = &s.query(sub[x]);
    s.index->find_batch(qs, cand, (unsigned)s.o.kmer_candidates);
    if (s.o.ignore_super) {  // sic: partition() moves the containing ones to the front and the REST is erased
        parallel_for(nq, [&](size_t x) {
            search::result_vector kept;
            for (auto &r : cand[x])
                if (contains_query(*r.sequence, s.query(sub[x]))) kept.push_back(r);
            cand[x].swap(kept);
        });
    }
    return cand;
}

// Takes trays `sub` and their candidates; gives every candidate its score -- search-all: fills cand[x] with every
// reference of the store, scored.  One comparison launch per slice of kComparePairsPerSlice pairs.
void host_scores(const search_call &s, const std::vector<size_t> &sub, std::vector<search::result_vector> &cand) {
    scoped_phase ph("sf.compare(C-ABI)");
    const search_filter::options &o = s.o;
    const unsigned n_refs = s.st.size();
    const size_t nq = sub.size();
    auto dev = s.st.worker_device(reference_store::dev_compare);
    for (size_t x0 = 0, x1; x0 < nq; x0 = x1) {
        uint64_t pairs = 0;
        x1 = x0;
        while (x1 < nq) {
            const uint64_t k = o.search_all ? n_refs : cand[x1].size();
            if (x1 > x0 && pairs + k > kComparePairsPerSlice) break;
            pairs += k;
            x1++;
        }
        if (pairs) {  // (a slice without a single candidate is not sent -- and has no scores to take)
            const pair_counts pc = compare_packed(
                dev.get(), x1 - x0, [&](size_t x) -> const cseq & { return s.query(sub[x0 + x]); },
                [&](size_t x) { return o.search_all ? (size_t)n_refs : cand[x0 + x].size(); },
                [&](size_t x, uint32_t *dst) {
                    if (o.search_all) {
                        for (unsigned r = 0; r < n_refs; r++) dst[r] = r;
                    } else {
                        for (size_t r = 0; r < cand[x0 + x].size(); r++) dst[r] = s.st.id_of(cand[x0 + x][r].sequence);
                    }
                },
                (int)o.comparator.iupac_rule, o.comparator.filter_lc_rule ? 1 : 0);
            for (size_t x = x0; x < x1; x++) {
                const sina_hip_match_counts *m = pc.counts.data() + pc.coff[x - x0];
                if (o.search_all) {
                    cand[x].clear();
                    cand[x].reserve(n_refs);
                    for (unsigned r = 0; r < n_refs; r++) cand[x].emplace_back(o.comparator.score(m[r]), &s.st.getCseq(r));
                } else {
                    for (size_t r = 0; r < cand[x].size(); r++) cand[x][r].score = o.comparator.score(m[r]);
                }
            }
        }
    }
}

// Search-all.  Takes query c and every reference of the store, scored (`all`, reordered); appends the result rows to vc.
void rank_all(const search_filter::options &o, const cseq &c, search::result_vector &all, search::result_vector &vc) {
    // every reference was compared: the `max_result` best that are not super-strings of the
    // query (--search-ignore-super), if above --search-min-sim (behaviour of src/
    // search_filter.cpp:271-296).  The sequence of libstdc++ calls is the contract here:
    // the window is re-sorted from the first kept candidate to the PREVIOUS window end, then
    // widened again, so std::partition also sees entries std::partial_sort left unordered.
    const auto stop = all.end();
    auto first_kept = all.begin();
    auto window_end = first_kept + (std::ptrdiff_t)std::min<size_t>((size_t)o.max_result, all.size());
    for (;;) {
        std::partial_sort(first_kept, window_end, stop, std::greater<search::result_item>());
        if (o.ignore_super) {
            window_end = first_kept + (std::ptrdiff_t)std::min<size_t>((size_t)o.max_result, (size_t)(stop - first_kept));
            first_kept = std::partition(first_kept, window_end, [&](search::result_item &item) {
                return contains_query(*item.sequence, c);
            });
        }
        const bool window_full = first_kept + o.max_result <= window_end;
        if (window_end == stop || window_full) break;
    }
    for (auto it = first_kept; it != window_end && it->score > o.min_sim; ++it) vc.push_back(*it);
}

// src/search_filter.cpp:297-331.  Takes a query's scored k-mer candidates (taken over); gives vc the `max_result` best
// in order, cut at the first not above --search-min-sim.
void rank_candidates(const search_filter::options &o, search::result_vector &cand, search::result_vector &vc) {
    vc.swap(cand);
    auto it = vc.begin();
    auto middle = vc.begin() + std::min<size_t>((size_t)o.max_result, vc.size());
    auto end = vc.end();
    std::partial_sort(it, middle, end, std::greater<search::result_item>());
    while (it != middle && it->score > o.min_sim) ++it;
    vc.erase(it, vc.end());
}

// Candidates, scores and ranking on the host: fills the search_result of trays `sub` (indices into the batch).
void host_rank(const search_call &s, const std::vector<size_t> &sub) {
    const size_t nq = sub.size();
    if (nq == 0) return;
    std::vector<search::result_vector> cand = s.o.search_all ? std::vector<search::result_vector>(nq) : host_candidates(s, sub);
    host_scores(s, sub, cand);
    scoped_phase ph("sf.rank+lca");
    parallel_for(nq, [&](size_t x) {
        search::result_vector &vc = *s.batch[sub[x]].search_result;
        if (s.o.search_all) rank_all(s.o, s.query(sub[x]), cand[x], vc);
        else rank_candidates(s.o, cand[x], vc);
    });
}

// What comes back from the device's ranking, per distinct query u: cnt[u] rows at ids / sc [u * N], best first, and
// flag[u] (bit 0: a 0 / 0 among its candidates, or a query the device cannot take as it is).
struct device_rows {
    std::vector<uint32_t> ids, cnt, flag;
    std::vector<float> sc;
    device_rows(size_t nu, uint32_t N) : ids(nu * N + 1), cnt(nu + 1), flag(nu + 1), sc(nu * N + 1) {}
};

// Takes the distinct queries as packed words (slot u at uab + d.off[u]) and ranks them on the device: one call of
// sina_hip_kmer_topk_rank for all, or -- search-all -- sina_hip_compare_rank per slice as the host path cuts them.
// Gives the rows, and false if the device refused as a limit (anything else it reports is an error).
bool device_rank_calls(const search_call &s, const distinct_items &d, const uint32_t *uab, uint32_t N, device_rows &rows) {
    const search_filter::options &o = s.o;
    const size_t nu = d.n;
    auto ok = [](int rc, const char *what) {  // a limit sends the stage back to the host path; anything else is an error
        if (rc != 0 && sina_hip_last_error_is_limit() != 1) hip_check(rc, what);
        return rc == 0;
    };
    if (nu == 0) return true;
    scoped_phase ph("sf.device_rank(C-ABI)");
    if (!o.search_all) {
        s.st.ensure_index((unsigned)o.fs_kmer_len, o.fs_no_fast);
        auto dev = s.st.worker_device(reference_store::dev_search);
        return ok(sina_hip_kmer_topk_rank(dev.get(), uab, d.off.data(), (uint32_t)nu, (uint32_t)o.kmer_candidates,
                                          (int)o.comparator.iupac_rule, o.comparator.filter_lc_rule ? 1 : 0, (int)o.comparator.cover_rule,
                                          N, rows.ids.data(), rows.sc.data(), rows.cnt.data(), rows.flag.data()),
                  "sina_hip_kmer_topk_rank");
    }
    auto dev = s.st.worker_device(reference_store::dev_compare);
    const size_t per = (size_t)std::max<uint64_t>(1, kComparePairsPerSlice / std::max(s.st.size(), 1u));
    for (size_t u0 = 0; u0 < nu; u0 += per) {
        const size_t u1 = std::min(nu, u0 + per);
        if (!ok(sina_hip_compare_rank(dev.get(), uab, d.off.data() + u0, (uint32_t)(u1 - u0), nullptr, nullptr,
                                      (int)o.comparator.iupac_rule, o.comparator.filter_lc_rule ? 1 : 0, (int)o.comparator.cover_rule,
                                      N, rows.ids.data() + u0 * N, rows.sc.data() + u0 * N, rows.cnt.data() + u0, rows.flag.data() + u0),
                "sina_hip_compare_rank"))
            return false;
    }
    return true;
}

// device-rank: score and rank on the device, the rows above min-sim into search_result.  Takes the searched trays;
// fills their results and gives true -- or false, with nothing filled: the whole stage then keeps the host path, for
// what the device does not rank as the host does (Jukes-Cantor: rounding can merge ratios into ties; ignore-super;
// more rows than a wave has lanes; names that repeat; more k-mer candidates than the LDS select sorts) and when the
// device refuses as a limit.  A query goes back to the host path, alone, when its columns do not ascend strictly, it
// has more than 65535 bases, or the device flags it.  Nothing of this reaches a tray's log.
bool device_rank(const search_call &s, const std::vector<size_t> &idx) {
    const search_filter::options &o = s.o;
    if (!(o.device_rank && o.comparator.dist_rule == CMP_DIST_NONE && !o.ignore_super && o.max_result >= 1 &&
          o.max_result <= (int)sina_hip::kRankMaxResult &&
          (o.search_all || std::min<uint64_t>((uint64_t)std::max(o.kmer_candidates, 0), s.st.size()) <= sina_hip::kKmerSelMax) &&
          s.st.name_order_ready()))
        return false;
    std::vector<size_t> dev_trays, host_trays;
    for (size_t i : idx) {
        const cseq &c = s.query(i);
        (c.size() <= 65535 && columns_ascend(c) ? dev_trays : host_trays).push_back(i);
    }
    const size_t nd = dev_trays.size();
    const uint32_t N = (uint32_t)s.o.max_result;
    auto seq_of = [&](size_t x) -> const cseq & { return s.query(dev_trays[x]); };
    const std::vector<uint64_t> qoff = offsets_of(nd, seq_of);
    batch_scratch<uint32_t> qab_buf, uab_buf;
    uint32_t *const qab = qab_buf.get(qoff.back() + 1);
    pack_words(nd, seq_of, qoff.data(), qab);
    // rows of the distinct queries (identical queries are sent once, as find_batch sends them)
    const distinct_items d = distinct_spans(dedup_enabled(), parallel_for, qab, qoff.data(), nd);
    const uint32_t *const uab = gather_distinct(d, parallel_for, qab, qoff.data(), uab_buf);
    device_rows rows(d.n, N);
    if (!device_rank_calls(s, d, uab, N, rows)) return false;
    uint64_t ranked = 0;
    for (size_t x = 0; x < nd; x++) {
        const size_t u = d.slot_of[x];
        if (rows.flag[u] & 1u) {
            host_trays.push_back(dev_trays[x]);
            continue;
        }
        auto &vc = *s.batch[dev_trays[x]].search_result;
        for (uint32_t r = 0; r < rows.cnt[u] && rows.sc[u * N + r] > s.o.min_sim; r++)
            vc.emplace_back(rows.sc[u * N + r], &s.st.getCseq(rows.ids[u * N + r]));
        ranked++;
    }
    s.st.count_ranked(ranked, host_trays.size());
    // (a flagged query "alone, in a call of its own": its candidates hold the NaN the host orders as it does)
    std::sort(host_trays.begin(), host_trays.end());
    for (size_t i : host_trays) host_rank(s, std::vector<size_t>{i});
    return true;
}

// device-search: a tray whose row says "ranked" and "every candidate had a score" takes its rows from the row, cut at
// --search-min-sim; it is never packed, uploaded or searched again.  Takes the searched trays; gives the others, in
// order -- copy-shortcut trays, trays the host finished, the long route's, flagged ones, trays that lost a base, and
// every tray when the aligner did not rank (align_plan.h, plan_search_inplace).  Nothing of this reaches a tray's log.
std::vector<size_t> rows_in_place(const search_call &s, const std::vector<size_t> &idx) {
    std::vector<size_t> rest;
    uint64_t taken = 0;
    for (size_t i : idx) {
        const tray &t = s.batch[i];
        const std::vector<uint32_t> *row = t.search_row.get();
        if (row == nullptr || row->size() < 2 || ((*row)[1] & 3u) != 2u || row->size() < 2 + 2 * (size_t)(*row)[0]) {
            rest.push_back(i);
            continue;
        }
        const uint32_t n = (*row)[0];
        auto &vc = *t.search_result;
        for (uint32_t r = 0; r < n; r++) {
            float score;
            memcpy(&score, row->data() + 2 + n + r, 4);
            if (!(score > s.o.min_sim)) break;
            vc.emplace_back(score, &s.st.getCseq((*row)[2 + r]));
        }
        taken++;
    }
    s.st.count_search_inplace(taken);
    return rest;
}

// boost::split(..., is_any_of(";")) of a taxonomy path, without the empty (or " ") group after the last ';'
void split_tax_path(const std::string &tax_path, std::vector<std::string> &group_names) {
    std::string cur;
    for (char ch : tax_path) {
        if (ch == ';') {
            group_names.push_back(cur);
            cur.clear();
        } else {
            cur += ch;
        }
    }
    group_names.push_back(cur);
    if (group_names.back().empty() || group_names.back() == " ") group_names.pop_back();
}

// Takes a searched tray with its result rows; gives its sequence nearest_slv, the copied fields of every row's
// reference and the LCA classification per --lca-fields field (src/search_filter.cpp:333-411).
void annotate_tray(const search_filter::options &o, reference_store &st, tray &t) {
    cseq *c = t.aligned_sequence;
    auto &vc = *t.search_result;
    std::string nearest;
    std::map<std::string, std::vector<std::vector<std::string>>> group_names_map;
    for (auto &i : vc) {
        const cseq &r = *i.sequence;
        for (const char *key : {"acc", "version", "start", "stop"}) st.loadKey(r, key);
        for (const std::string &s : o.v_lca_fields) {
            st.loadKey(r, s);
            std::string tax_path = r.get_attr<std::string>(s);
            if (tax_path == "Unclassified;") continue;
            std::vector<std::string> group_names;
            split_tax_path(tax_path, group_names);
            group_names_map[s].push_back(group_names);
        }
        char buf[64];
        snprintf(buf, sizeof buf, "~%.3f ", (double)i.score);  // fmt "{}.{}.{}.{}~{:.3f} "
        nearest += r.get_attr<std::string>("acc") + "." + r.get_attr<std::string>("version") + "." +
                   r.get_attr<std::string>("start") + "." + r.get_attr<std::string>("stop") + buf;
        const std::string acc = r.get_attr<std::string>("acc");
        for (const std::string &s : o.v_copy_fields) {
            st.loadKey(r, s);
            c->set_attr<std::string>(std::string("copy_") + acc + std::string("_") + s, r.get_attr<std::string>(s));
        }
    }
    c->set_attr<std::string>(search_filter::fn_nearest, nearest);
    for (const std::string &s : o.v_lca_fields)
        c->set_attr<std::string>(std::string("lca_") + s, lca_vote(group_names_map[s], vc.size(), o.lca_quorum));
}
}  // namespace

// src/search_filter.cpp:244-412 for a batch of trays: the k-mer search and the comparisons of the
// whole batch are one GPU call each (sina_hip_kmer_topk, sina_hip_compare) -- or, with device-rank, one call for
// both that brings down the max_result best only (sina_hip_kmer_topk_rank; search-all: sina_hip_compare_rank).
// -- or, for a tray the aligner's device-search has ranked, no call at all: its rows came back with its alignment.
void search_filter::operator()(std::vector<tray> &batch) {
    const search_call s{sf_opts(), *data->arb, data->index, batch};
    const std::vector<size_t> idx = searched_trays(batch);
    if (idx.empty()) return;
    const std::vector<size_t> rest = rows_in_place(s, idx);
    if (!rest.empty() && !device_rank(s, rest)) {
        if (s.o.device_rank) s.st.count_ranked(0, rest.size());
        host_rank(s, rest);
    }
    scoped_phase ph("sf.rank+lca");
    parallel_for(idx.size(), [&](size_t x) { annotate_tray(s.o, s.st, batch[idx[x]]); });
}

// ================================================================ helix base-pair score (align_bp_score_slv)

reference_store::pair_map aligner_pair_map() {
    if (aligner::opts == nullptr || aligner::opts->database.empty()) return nullptr;
    const std::shared_ptr<reference_store> st = reference_store::find(aligner::opts->database);
    return st ? st->pairs() : nullptr;
}

float tray_pair_score(const tray &t, const reference_store::pair_map &map) {
    if (t.aligned_sequence == nullptr) return 0.f;
    if (t.bp_score_set) return t.bp_score;
    return map ? t.aligned_sequence->calcPairScore(*map) : 0.f;
}

void pair_score_batch(std::vector<tray> &batch) {
    if (aligner::opts == nullptr || aligner::opts->database.empty()) return;
    const std::shared_ptr<reference_store> st = reference_store::find(aligner::opts->database);
    if (!st) return;
    const reference_store::pair_map map = st->pairs();
    if (!map) return;
    // the trays the device takes (columns ascending: the kernel finds a column by bisection), and the others
    std::vector<size_t> dev;
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> words;
    {
        scoped_phase ph("bp.pack");
        std::vector<char> kind(batch.size(), 0);  // 1: device, 2: host walk
        parallel_for(batch.size(), [&](size_t i) {
            tray &t = batch[i];
            if (t.aligned_sequence == nullptr || t.bp_score_set) return;  // (set: the aligner's device-bps has scored it)
            if (columns_ascend(*t.aligned_sequence)) kind[i] = 1;
            else {
                t.bp_score = t.aligned_sequence->calcPairScore(*map);
                t.bp_score_set = true;
            }
        });
        for (size_t i = 0; i < batch.size(); i++)
            if (kind[i] == 1) {
                dev.push_back(i);
                off.push_back(off.back() + batch[i].aligned_sequence->size());
            }
        words.resize((size_t)off.back());
        parallel_for(dev.size(), [&](size_t x) {
            const cseq &c = *batch[dev[x]].aligned_sequence;
            if (c.size()) memcpy(words.data() + off[x], c.packed(), 4 * (size_t)c.size());
        });
    }
    if (dev.empty()) return;
    std::vector<uint32_t> counts(6 * dev.size(), 0);
    {
        scoped_phase ph("bp.pair_counts(C-ABI)");
        reference_store::lease dv = st->worker_device(reference_store::dev_compare);
        hip_check(sina_hip_pair_counts(dv.get(), words.data(), off.data(), (uint32_t)dev.size(), counts.data()), "sina_hip_pair_counts");
    }
    for (size_t x = 0; x < dev.size(); x++) {
        tray &t = batch[dev[x]];
        t.bp_score = pair_score_from_counts(counts.data() + 6 * x);
        t.bp_score_set = true;
    }
}

}  // namespace sina
