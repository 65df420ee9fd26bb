// Host side of the boundary: the aligner.  Behaviour follows the reference (src/align.cpp, citations inline); what
// goes to the device in which call is decided in align_plan.h, the DP itself goes through the C ABI
// (include/sina_hip.h).  No CPU fallback: if the HIP library reports an error, the stage throws.
#include "stages_internal.h"
#include "align_plan.h"
#include "../kmer_plan.h"
#include "../rank_plan.h"
#include "../contain_plan.h"
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstring>
#include <ctime>

namespace sina {

// ================================================================ aligner

aligner::options *aligner::opts = nullptr;

static aligner::options al_defaults() {  // src/align.cpp:231-274
    aligner::options o;
    o.realign = false;
    o.overhang = OVERHANG_ATTACH;
    o.lowercase = LOWERCASE_NONE;
    o.insertion = INSERTION_SHIFT;
    o.calc_idty = false;
    o.fs_no_graph = false;
    o.fs_weight = 1;
    o.match_score = 2;
    o.mismatch_score = -1;
    o.gap_penalty = 5.0f;
    o.gap_ext_penalty = 2.0f;
    o.debug_graph = o.write_used_rels = o.use_subst_matrix = false;
    o.device_graph = true;  // family DAGs are built on the GPU (sina_hip_align_families)
    // the weighted trays of a batch go to the device in one call whatever filters they chose (--auto-filter-field):
    // sina_hip_align_families_wsets; off: one call per filter
    o.weight_sets = true;
    // --fs-no-graph profiles are built on the GPU (sina_hip_align_profiles) only on request: the device route gives the
    // host route's bytes, but the two have not been timed against each other yet (tools/perf_profile.py), so the
    // route that has always been taken stays the default
    o.device_profile = false;
    // families beyond the fast DP path's limits (sina_hip.h) through sina_hip_align_graphs_any and its wide kernel:
    // on request
    o.wide_fallback = false;
    // the helix base-pair score from the align call itself (sina_hip_align_count_pairs) instead of a second trip with
    // the finished alignments (pair_score_batch): on request, until it has been decided on measurements
    o.device_bps = false;
    // calc-idty from the align call itself (sina_hip_align_count_identity) instead of a second trip with the finished
    // alignments (set_family_identity): on request, until it has been decided on measurements
    o.device_idty = false;
    // the device also finishes alignments whose insertions shift their neighbours (assemble = 2): on request, until it
    // has been decided on measurements
    o.device_shift = false;
    // the search stage's rows from the align call itself (sina_hip_align_rank) instead of a second trip with the
    // finished sequences (default off)
    o.device_search = false;
    // --show-dist's comparisons in one device call per batch (sina_hip_show_dist, show_dist_batch) instead of the
    // sink's walks: on request, until it has been decided on measurements
    o.device_dist = false;
    // the exact-relative test of a batch's suspects in one device call (sina_hip_find_bases, find_on_device) instead of
    // the host's substring searches: on request, until it has been decided on measurements
    o.device_copy = false;
    return o;
}
static aligner::options &al_opts() {
    if (!aligner::opts) aligner::opts = new aligner::options(al_defaults());
    return *aligner::opts;
}
void aligner::reset_options() { al_opts() = al_defaults(); }

void aligner::set_option(const std::string &name, const std::string &value) {
    options &o = al_opts();
    const std::string v = lower(value);
    if (name == "realign") o.realign = to_bool(value);
    else if (name == "overhang") {
        if (v == "attach") o.overhang = OVERHANG_ATTACH;
        else if (v == "remove") o.overhang = OVERHANG_REMOVE;
        else if (v == "edge") o.overhang = OVERHANG_EDGE;
        else throw std::logic_error("invalid value for --overhang: " + value);
    } else if (name == "lowercase") {
        if (v == "none") o.lowercase = LOWERCASE_NONE;
        else if (v == "original") o.lowercase = LOWERCASE_ORIGINAL;
        else if (v == "unaligned") o.lowercase = LOWERCASE_UNALIGNED;
        else throw std::logic_error("invalid value for --lowercase: " + value);
    } else if (name == "insertion") {
        if (v == "shift") o.insertion = INSERTION_SHIFT;
        else if (v == "forbid") o.insertion = INSERTION_FORBID;
        else if (v == "remove") o.insertion = INSERTION_REMOVE;
        else throw std::logic_error("invalid value for --insertion: " + value);
    } else if (name == "fs-weight") o.fs_weight = std::stof(value);
    else if (name == "match-score") o.match_score = std::stof(value);
    else if (name == "mismatch-score") o.mismatch_score = std::stof(value);
    else if (name == "pen-gap") o.gap_penalty = std::stof(value);
    else if (name == "pen-gapext") o.gap_ext_penalty = std::stof(value);
    else if (name == "write-used-rels") o.write_used_rels = to_bool(value);
    else if (name == "calc-idty") o.calc_idty = to_bool(value);
    else if (name == "fs-no-graph") o.fs_no_graph = to_bool(value);
    else if (name == "use-subst-matrix" || name == "debug-graph") {
        if (to_bool(value)) throw std::logic_error("aligner: --" + name + " is outside the accelerated path");
    } else if (name == "device-graph") o.device_graph = to_bool(value);
    else if (name == "device-profile") o.device_profile = to_bool(value);
    else if (name == "wide-fallback") o.wide_fallback = to_bool(value);
    else if (name == "weight-sets") o.weight_sets = to_bool(value);
    else if (name == "device-bps") o.device_bps = to_bool(value);
    else if (name == "device-idty") o.device_idty = to_bool(value);
    else if (name == "device-shift") o.device_shift = to_bool(value);
    else if (name == "device-search") o.device_search = to_bool(value);
    else if (name == "device-dist") o.device_dist = to_bool(value);
    else if (name == "device-copy") o.device_copy = to_bool(value);
    else if (name == "db") o.database = value;
    else throw std::logic_error("aligner: unknown option " + name);
}
void aligner::validate_options() {}

aligner::aligner() { al_opts(); }
aligner::~aligner() = default;
aligner::aligner(const aligner &) = default;
aligner &aligner::operator=(const aligner &) = default;

static const std::string &make_datetime() {  // src/align.cpp:287-299 (formatted once per second and thread)
    thread_local time_t last = (time_t)-1;
    thread_local std::string text;
    const time_t t = time(nullptr);
    if (t != last) {
        struct tm tmv;
        char buf[50];
        gmtime_r(&t, &tmv);
        strftime(buf, 50, "%F %T", &tmv);
        text = buf;
        last = t;
    }
    return text;
}

namespace {
// case-insensitive substring search on base strings (boost::algorithm::icontains /
// ifind_first as used at src/align.cpp:329-333,364-369)
std::string upper_copy(const std::string &s) {
    std::string r(s);
    for (auto &c : r) c = (char)toupper((unsigned char)c);
    return r;
}

// First occurrence of `needle` in `hay` (std::string::find's answer).  Exact relatives are the common case of an
// amplicon run -- every member of a family may hold the query -- and std::string::find, a memchr for the first
// character and a memcmp at each hit, stops at every fourth position of a four-letter text: 2.5 us per member of
// 1500 bases, 100 us per query (tools/hoststub, --window 250).  Here: the needle's first four bytes against 32
// positions at a time (four shifted loads; a candidate every 256 positions), the scalar twin compares its first
// eight bytes as one word.
static size_t find_bases_scalar(const char *p, size_t from, size_t last, const std::string &needle) {
    const size_t n = needle.size();
    uint64_t first;
    memcpy(&first, needle.data(), 8);
    for (size_t i = from; i <= last; i++) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        if (w == first && memcmp(p + i + 8, needle.data() + 8, n - 8) == 0) return i;
    }
    return std::string::npos;
}
__attribute__((target("avx2"))) static size_t find_bases_avx2(const char *p, size_t last, const std::string &needle) {
    const size_t n = needle.size();
    const char *nd = needle.data();
    const __m256i c0 = _mm256_set1_epi8(nd[0]), c1 = _mm256_set1_epi8(nd[1]), c2 = _mm256_set1_epi8(nd[2]), c3 = _mm256_set1_epi8(nd[3]);
    size_t i = 0;
    // (a block reads bytes i .. i + 34: inside the text while i + 31 <= last, the needle being 8 or longer)
    for (; i + 31 <= last; i += 32) {
        const __m256i e = _mm256_and_si256(
            _mm256_and_si256(_mm256_cmpeq_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i)), c0),
                             _mm256_cmpeq_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i + 1)), c1)),
            _mm256_and_si256(_mm256_cmpeq_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i + 2)), c2),
                             _mm256_cmpeq_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i + 3)), c3)));
        uint32_t m = (uint32_t)_mm256_movemask_epi8(e);
        while (m) {
            const unsigned b = (unsigned)__builtin_ctz(m);
            if (memcmp(p + i + b + 4, nd + 4, n - 4) == 0) return i + b;
            m &= m - 1;
        }
    }
    return find_bases_scalar(p, i, last, needle);
}
}  // namespace
size_t find_bases(const std::string &hay, const std::string &needle, int force_scalar) {
    const size_t n = needle.size(), h = hay.size();
    if (n < 8 || h < n) return hay.find(needle);
    static const bool avx2 = __builtin_cpu_supports("avx2");
    return (avx2 && !force_scalar) ? find_bases_avx2(hay.data(), h - n, needle) : find_bases_scalar(hay.data(), 0, h - n, needle);
}
namespace {

struct dp_job {
    tray *t = nullptr;
    cseq *c = nullptr;  // working copy (becomes aligned_sequence)
    // the family in mseq input order IS the tray's alignment_reference as the preparation left it (a list of its
    // own per job was 9216 heap blocks per batch)
    const search::result_vector *fam = nullptr;
    size_t family_size() const { return fam->size(); }
    const cseq *member(size_t y) const { return (*fam)[y].sequence; }
    std::vector<const cseq *> family() const {
        std::vector<const cseq *> v;
        v.reserve(fam->size());
        for (const auto &r : *fam) v.push_back(r.sequence);
        return v;
    }
};

// |K(q)|: windows of k unambiguous bases ending before the last base, first base A in "fast" mode
// (src/kmer.h:69-83,122-124,188-201) -- for a family whose scores famfinder stamped as
// raw k-mer counts (tray::family_scores_kmer_k: k, negative = no-fast)
static unsigned query_kmer_count(const cseq &c, int stamp) {
    const unsigned k = (unsigned)(stamp < 0 ? -stamp : stamp);
    const bool nofast = stamp < 0;
    const auto &b = c.getAlignedBases();
    unsigned run = 0, n = 0;
    for (size_t e = 0; e + 1 < b.size(); e++) {
        const unsigned m = (b[e].raw >> 24) & 0xfu;
        run = (m & (m - 1)) == 0 && m != 0 ? run + 1 : 0;  // exactly one base bit
        if (run >= k && (nofast || ((b[e + 1 - k].raw >> 24) & 0xfu) == 1u)) n++;
    }
    return n;
}

// Whether prepare_tray looks at the tray's family at all, and the longest query it does that for (device limit: soft
// failure of the tray.  With wide-fallback a query beyond the fast DP path's length is aligned by the wide kernel -- up to
// the length the k-mer search can have found its family for)
static bool tray_is_complete(const tray &t) { return t.input_sequence != nullptr && t.alignment_reference != nullptr && t.astats != nullptr; }
static unsigned max_query_len(const aligner::options &o) { return o.wide_fallback ? SINA_HIP_MAX_LONG_QUERY_LEN : SINA_HIP_MAX_QUERY_LEN; }
// A family member can only contain the query's bases if it has every one of the query's
// k-mers, i.e. if its k-mer score (what famfinder ranked it by) is the query's k-mer count --
// which spares the string search for all but exact relatives.  Gives that count; -1: the scores are no k-mer counts.
static float all_kmers_of(const tray &t) {
    return t.family_scores_kmer_k == 0 ? -1.f
                                       : (float)(t.query_kmer_count >= 0 ? (unsigned)t.query_kmer_count
                                                                         : query_kmer_count(*t.input_sequence, t.family_scores_kmer_k));
}

// device-copy: where the suspects of one tray -- the family members that pass the k-mer-count test -- hold the query's
// bases, as sina_hip_find_bases answered for the batch (find_on_device): the start, or kContainNone.  A member without
// an entry is searched on the host.
struct copy_answers {
    std::vector<std::pair<const cseq *, uint32_t>> at;
    const uint32_t *find(const cseq *r) const {
        for (const auto &e : at)
            if (e.first == r) return &e.second;
        return nullptr;
    }
};

// Takes a tray as famfinder left it (prep_store: the reference store, if there is one, for its cached upper-case bases;
// dev: the device's answers for the tray's suspects, or null); gives true if it needs the DP, false if it is done:
// nothing to align, too long, or its alignment copied from a relative.
static bool prepare_tray(tray &t, const aligner::options &o, reference_store *prep_store, const copy_answers *dev) {
    if (!tray_is_complete(t)) return false;  // :310-318
    const unsigned max_len = max_query_len(o);
    if (t.input_sequence->size() > max_len) {
        t.log << "unable to align: sequence of " << t.input_sequence->size() << " bases (device limit "
              << max_len << ");";
        return false;
    }
    uint64_t tk = host_tsc();
    // (the working copy -- src/align.cpp:320-326 -- is made where its bases are known: below for a copied
    // alignment, when the DP is back for the rest; it never holds the query's own bases)
    search::result_vector &vc = *t.alignment_reference;
    // (the query's upper-case base string: only built if a family member passes the k-mer-count
    // test below and has to be searched for it -- exact relatives only)
    std::string ubases_store;
    bool have_ubases = false;
    const size_t n_bases = t.input_sequence->size();
    auto ubases_of_query = [&]() -> const std::string & {
        if (!have_ubases) {
            ubases_store = upper_copy(t.input_sequence->getBases());
            have_ubases = true;
        }
        return ubases_store;
    };
    // upper-case bases of a family member: cached per store (40 members x every query)
    auto ref_ubases = [&](const cseq *r, std::string &tmp) -> const std::string & {
        if (prep_store && prep_store->owns(r)) return prep_store->upper_bases(prep_store->id_of(r));
        tmp = upper_copy(r->getBases());
        return tmp;
    };
    const float all_kmers = all_kmers_of(t);
    // (the device's answer for a member, where the batch's pre-pass has one)
    auto device_at = [&](const cseq *r) -> const uint32_t * { return dev != nullptr ? dev->find(r) : nullptr; };
    auto lacks_query = [&](search::result_item &item) {
        if (item.score < all_kmers) return true;
        if (const uint32_t *at = device_at(item.sequence)) return *at == sina_hip::kContainNone;
        std::string tmp;
        return find_bases(ref_ubases(item.sequence, tmp), ubases_of_query()) == std::string::npos;
    };
    tk = host_tick("prepare: kmer count", tk);
    // (the order this leaves the family in is the member order its DAG is built from)
    auto holders = std::partition(vc.begin(), vc.end(), lacks_query);
    tk = host_tick("prepare: partition", tk);
    if (holders != vc.end()) {
        if (o.realign) {  // :337-348
            t.log << "sequences ";
            for (auto it = holders; it != vc.end(); ++it)
                t.log << it->sequence->get_attr<std::string>(fn::acc) << " ";
            t.log << "containing exact candidate removed from family;";
            vc.erase(holders, vc.end());
            if (vc.empty()) {
                t.log << "that's ALL of them. skipping sequence;";
                return false;
            }
        } else {  // :349-388 steal the alignment
            auto is_query_itself = [&](search::result_item &item) {
                if (const uint32_t *at = device_at(item.sequence)) return *at == 0 && item.sequence->size() == n_bases;
                std::string tmp;
                return ref_ubases(item.sequence, tmp) == ubases_of_query();
            };
            auto exact = std::find_if(holders, vc.end(), is_query_itself);
            cseq &c = *object_cache<cseq, cache_aligned_seq>::take();
            c.copy_meta(*t.input_sequence);
            if (exact != vc.end()) {
                c.setAlignedBases(exact->sequence->getAlignedBases());
                t.log << "copied alignment from identical template sequence "
                      << exact->sequence->get_attr<std::string>(fn::acc) << ":"
                      << exact->sequence->get_attr<std::string>(fn::start, "0") << "; ";
            } else {
                const auto &refal = holders->sequence->getAlignedBases();
                std::string tmp;
                const uint32_t *const dev_at = device_at(holders->sequence);
                const size_t at = dev_at ? (size_t)*dev_at : find_bases(ref_ubases(holders->sequence, tmp), ubases_of_query());
                c.setAlignedBases(refal.data() + at, n_bases);
                t.log << "copied alignment from (longer) template sequence "
                      << holders->sequence->get_attr<std::string>(fn::acc) << ":"
                      << holders->sequence->get_attr<std::string>(fn::start, "0") << "; ";
            }
            c.setWidth(holders->sequence->getWidth());
            c.set_attr(fn::date, make_datetime());
            c.set_attr(fn::qual, 100);
            if (o.calc_idty) c.set_attr(fn::idty, 100.f);
            c.set_attr(fn::head, 0);
            c.set_attr(fn::tail, 0);
            c.set_attr(fn::filter, "");
            t.aligned_sequence = &c;
            return false;
        }
    }
    host_tick("prepare: family list", tk);
    return true;
}

// Takes the options and a group's positional weights (none: simple scheme; they outlive the result; a group of several
// filters: their vectors of n_weights floats one after the other); gives the device call's parameters.
static sina_hip_align_params make_align_params(const aligner::options &o, const align_switches &sw, const float *weights, size_t n_weights) {
    sina_hip_align_params p;
    sina_hip_align_params_default(&p);
    p.match_score = o.match_score;
    p.mismatch_score = o.mismatch_score;
    p.gap_penalty = o.gap_penalty;
    p.gap_ext_penalty = o.gap_ext_penalty;
    p.fs_weight = o.fs_weight;
    p.overhang = (int)o.overhang;
    p.lowercase = (int)o.lowercase;
    p.insertion = (int)o.insertion;
    p.weights = n_weights == 0 ? nullptr : weights;
    p.n_weights = (uint32_t)n_weights;
    p.assemble = align_assemble_mode(sw);  // (the device finishes what it can: sina_hip_align_out::assembled)
    return p;
}

// What the device is given of a group: one SLOT per distinct (query, ordered family, filter); every member reads one slot's results.
struct device_slots {
    size_t dnq = 0;                   // number of slots
    std::vector<uint32_t> slot_of;    // [members] slot of group member x
    std::vector<uint64_t> dqoff;      // [dnq + 1] slot u's mask bytes -- and its aligned columns coming back -- start at dqoff[u]
    const uint8_t *dqmask = nullptr;  // the slots' mask bytes (a thread's scratch buffer: distinct_slots)
    const std::vector<dp_job *> *members = nullptr;
    std::vector<uint32_t> first;  // [dnq] first member of slot u; empty if nothing repeats (slot u is member u)
    const dp_job &job(size_t u) const { return *(*members)[first.empty() ? u : first[u]]; }  // the job slot u is aligned for
    // a group of several filters (sina_hip_align_families_wsets): the vector of slot u among the call's; empty: one for all
    std::vector<uint32_t> set_of;
    uint32_t n_sets = 1;
    // slot u alone, as the one slot of a call of its own (the long route); reads this one's mask bytes in place
    device_slots only(size_t u) const {
        device_slots one;
        one.dnq = 1;
        one.members = members;
        one.first.assign(1, first.empty() ? (uint32_t)u : first[u]);
        one.dqoff = {0, dqoff[u + 1] - dqoff[u]};
        one.dqmask = dqmask + dqoff[u];
        return one;
    }
};

// Repeated queries -- the same bases in the same case against the same ordered family under the same filter: amplicon
// runs are full of them -- are aligned ONCE (one DAG, one DP, one walk); every tray then finishes from the device results of its first
// occurrence, with its own name, log and attributes (distinct.h).  Takes a group, packs its queries' mask bytes (the DP
// looks at the four base bits only: case does not matter); gives the slots.  Where nothing repeats the packing is
// handed on as it is: nothing is copied.
static device_slots distinct_slots(const std::vector<dp_job *> &members) {
    scoped_phase ph("al.pack_queries");
    const size_t nq = members.size();
    auto seq_of = [&](size_t x) -> const cseq & { return *members[x]->t->input_sequence; };
    const std::vector<uint64_t> qoff = offsets_of(nq, seq_of);
    thread_local batch_scratch<uint8_t> qmask_buf;
    uint8_t *const qmask = qmask_buf.get(qoff.back() + 1);
    pack_masks(nq, seq_of, qoff.data(), qmask);
    distinct_items d = distinct_spans(
        dedup_enabled(), parallel_for, qmask, qoff.data(), nq,
        [&](size_t x) {
            const dp_job &jb = *members[x];
            uint64_t hf = 0xcbf29ce484222325ull ^ jb.family_size();
            for (size_t y = 0; y < jb.family_size(); y++) {
                hf = (hf ^ (uint64_t)reinterpret_cast<uintptr_t>(jb.member(y))) * 0x100000001b3ull;
                hf ^= hf >> 29;
            }
            return (hf ^ (uint64_t)reinterpret_cast<uintptr_t>(jb.t->astats)) * 0x100000001b3ull;  // (a group may hold several filters)
        },
        [&](size_t a, size_t b) {
            const dp_job &ja = *members[a], &jb = *members[b];
            if (ja.family_size() != jb.family_size() || ja.t->astats != jb.t->astats) return false;
            for (size_t y = 0; y < ja.family_size(); y++)
                if (ja.member(y) != jb.member(y)) return false;
            return true;
        });
    thread_local batch_scratch<uint8_t> dqmask_buf;  // (not the packing's buffer: that one is being read)
    device_slots s;
    s.members = &members;
    s.dqmask = gather_distinct(d, parallel_for, qmask, qoff.data(), dqmask_buf);
    s.dnq = d.n;
    s.slot_of = std::move(d.slot_of);
    s.dqoff = std::move(d.off);
    s.first = std::move(d.first);
    return s;
}

// The host-graph route: the slots' families as DAGs (--fs-no-graph: profiles) built by the host twins of the device
// builders and handed over as graphs -- with wide-fallback through sina_hip_align_graphs_any, which takes a DAG of
// any size.  Fills out[slot] and the context's staged columns; gives the graphs' width.  max_cells (if asked for, and
// before the device is called): the largest wide mesh among the slots, in cells as SINA_HIP_WIDE_CELLS counts them.
static uint32_t align_host_graphs(sina_hip_ctx *ctx, const aligner::options &o, const sina_hip_align_params &p,
                                  const device_slots &s, sina_hip_align_out *out, uint64_t *max_cells = nullptr) {
    const size_t n = s.dnq;
    std::vector<host_graph> gs(n);
    {
        scoped_phase ph("al.host_graph_build");
        parallel_for(n, [&](size_t u) {
            if (o.fs_no_graph) build_family_profile(s.job(u).family(), -o.match_score, -o.mismatch_score, o.gap_penalty, o.gap_ext_penalty, &gs[u]);
            else build_family_graph(s.job(u).family(), o.fs_weight, &gs[u]);
        });
    }
    if (max_cells)
        for (size_t u = 0; u < n; u++) {
            const uint64_t N = gs[u].pos.size(), L = s.dqoff[u + 1] - s.dqoff[u];
            *max_cells = std::max(*max_cells, (N + L - 1) * std::min(N, L));
        }
    sina_hip_graph_batch gb;
    std::vector<uint64_t> node_off(n + 1, 0), edge_off(n + 1, 0);
    std::vector<uint32_t> npos, pred, poff, smin;
    std::vector<uint8_t> nmask;
    std::vector<float> nw, nscore;  // (all sized below, under the phase that pays for them)
    float self16[16];
    {
        scoped_phase ph("al.host_graph_concat");
        for (size_t u = 0; u < n; u++) {
            node_off[u + 1] = node_off[u] + gs[u].pos.size();
            edge_off[u + 1] = edge_off[u] + gs[u].pred.size();
        }
        npos.resize(node_off.back()), pred.resize(edge_off.back() ? edge_off.back() : 1), poff.resize(node_off.back() + n);
        smin.resize(node_off.back()), nmask.resize(node_off.back()), nw.resize(node_off.back());
        nscore.resize(o.fs_no_graph ? 16 * (size_t)node_off.back() : 0);
        if (o.fs_no_graph) profile_self_scores(-o.match_score, -o.mismatch_score, o.gap_penalty, o.gap_ext_penalty, self16);
        parallel_for(n, [&](size_t u) {
            const host_graph &g = gs[u];
            std::copy(g.pos.begin(), g.pos.end(), npos.begin() + node_off[u]);
            std::copy(g.mask.begin(), g.mask.end(), nmask.begin() + node_off[u]);
            std::copy(g.weight.begin(), g.weight.end(), nw.begin() + node_off[u]);
            std::copy(g.succ_minpos.begin(), g.succ_minpos.end(), smin.begin() + node_off[u]);
            std::copy(g.pred_off.begin(), g.pred_off.end(), poff.begin() + node_off[u] + u);
            std::copy(g.pred.begin(), g.pred.end(), pred.begin() + edge_off[u]);
            if (o.fs_no_graph) std::copy(g.score16.begin(), g.score16.end(), nscore.begin() + 16 * node_off[u]);
        });
        gb.nq = (uint32_t)n;
        gb.node_off = node_off.data();
        gb.edge_off = edge_off.data();
        gb.node_pos = npos.data();
        gb.node_mask = nmask.data();
        gb.node_weight = nw.data();
        gb.pred_off = poff.data();
        gb.pred = pred.data();
        gb.succ_minpos = smin.data();
        gb.width = gs[0].width;
        gb.node_score16 = o.fs_no_graph ? nscore.data() : nullptr;
        gb.self_score16 = o.fs_no_graph ? self16 : nullptr;
    }
    scoped_phase ph("al.align_graphs(C-ABI)");
    // (out_pos == nullptr: the aligned columns are read where the device copied them, sina_hip_staged_out_pos)
    if (o.wide_fallback)
        hip_check(sina_hip_align_graphs_any(ctx, &gb, s.dqmask, s.dqoff.data(), &p, out, nullptr), "align_graphs_any");
    else
        hip_check(sina_hip_align_graphs(ctx, &gb, s.dqmask, s.dqoff.data(), &p, out, nullptr), "align_graphs");
    return gb.width;
}

// The family-id route: the slots' families as lists of reference ids, their DAGs (--fs-no-graph: profiles) built on
// the device.  wide-fallback: a group the device builders refuse because a family exceeds one of their documented
// limits is redone once over host-built graphs; any other failure propagates.  Fills out[slot] and the context's
// staged columns; gives the alignment's width.
static uint32_t align_family_ids(sina_hip_ctx *ctx, reference_store &store, const aligner::options &o,
                                 const sina_hip_align_params &p, const device_slots &s, sina_hip_align_out *out) {
    const size_t n = s.dnq;
    std::vector<uint64_t> foff(n + 1, 0);
    std::vector<uint32_t> fids;
    {
        scoped_phase ph("al.pack_queries");  // (the families' ids are packed under the phase the queries were)
        for (size_t u = 0; u < n; u++) foff[u + 1] = foff[u] + s.job(u).family_size();
        fids.resize(foff.back() ? foff.back() : 1);
        parallel_for(n, [&](size_t u) {
            const dp_job &jb = s.job(u);
            for (size_t y = 0; y < jb.family_size(); y++) fids[foff[u] + y] = store.id_of(jb.member(y));
        });
    }
    int rc;
    // (out_pos == nullptr: the aligned columns are read where the device copied them, sina_hip_staged_out_pos)
    if (o.fs_no_graph) {
        scoped_phase ph("al.align_profiles(C-ABI)");
        rc = sina_hip_align_profiles(ctx, fids.data(), foff.data(), (uint32_t)n, s.dqmask, s.dqoff.data(), &p, out, nullptr);
    } else if (!s.set_of.empty()) {
        scoped_phase ph("al.align_families(C-ABI)");
        rc = sina_hip_align_families_wsets(ctx, fids.data(), foff.data(), (uint32_t)n, s.dqmask, s.dqoff.data(), &p, s.set_of.data(), s.n_sets,
                                           out, nullptr);
        hip_check(rc, "align_families_wsets");  // (a group of several filters is not formed with wide-fallback: no second route)
    } else {
        scoped_phase ph("al.align_families(C-ABI)");
        rc = sina_hip_align_families(ctx, fids.data(), foff.data(), (uint32_t)n, s.dqmask, s.dqoff.data(), &p, out, nullptr);
    }
    if (rc != 0 && o.wide_fallback && sina_hip_last_error_is_limit() == 1) return align_host_graphs(ctx, o, p, s, out);
    hip_check(rc, o.fs_no_graph ? "align_profiles" : "align_families");
    return store.getAlignmentWidth();
}

// The bases a walk emits, in its order -- `tail` overhang bases from the query's end, the aligned bases back from
// end_s, `head` overhang bases -- as emit(column as the device gave it, base bits of that query base): upper-cased
// unless --lowercase=original (src/align.cpp:324-326), overhang bases lower-cased with --lowercase=unaligned.
template <class Emit>
static void for_each_emission(const cseq &query, const sina_hip_align_out &r, uint32_t tail, uint32_t head, LOWERCASE_TYPE lowercase,
                              const uint32_t *pos, Emit &&emit) {
    const uint32_t *qraw = query.packed();
    const uint32_t L = (uint32_t)query.size();
    const uint32_t keep_case = lowercase == LOWERCASE_ORIGINAL ? 0xFFFFFFFFu : ~((uint32_t)16 << 24);
    const uint32_t lower_bit = lowercase == LOWERCASE_UNALIGNED ? (uint32_t)16 << 24 : 0u;
    auto qbase = [&](uint32_t i, bool overhang_base) -> uint32_t {  // base bits of query base i, in place
        return ((qraw[i] & keep_case) & 0xFF000000u) | (overhang_base ? lower_bit : 0u);
    };
    uint32_t n = 0;
    for (uint32_t k = 0; k < tail; k++) emit(pos[n++], qbase(L - 1 - k, true));
    for (int k = 0; k < r.aligned_bases; k++) emit(pos[n++], qbase((uint32_t)r.end_s - (uint32_t)k, false));
    for (uint32_t k = 0; k < head; k++) emit(pos[n++], qbase((uint32_t)r.cutoff_head - 1 - k, true));
}

// Takes the result and emitted columns of a walk the device did not assemble; gives the working copy `c` its bases: the
// container steps of backtrack() (src/mesh.h:603-726) and the NAST fix-up with its log line.  Gives the tick to go on from.
static uint64_t assemble_on_host(tray &t, cseq &c, const sina_hip_align_out &r, const uint32_t *pos, uint32_t width,
                                 const aligner::options &o, uint64_t tk) {
    const bool keep_over = (o.overhang != OVERHANG_REMOVE);
    const uint32_t tail = keep_over ? (uint32_t)r.cutoff_tail : 0;
    const uint32_t head = keep_over ? (uint32_t)r.cutoff_head : 0;
    const uint32_t n_out = tail + (uint32_t)r.aligned_bases + head;
    // The container steps in one pass: every emitted base is appended under the container rule (a column left of
    // the current width is moved up to it, src/cseq.cpp:79-95), then the sequence is reversed (order and columns,
    // :283-289).  The columns after the rule never decrease, so the result is written back to front directly.
    c.clearSequence();
    base_vector &fin = c.mutableAlignedBases();  // (a recycled sequence: no allocation)
    fin.resize(n_out);
    uint32_t reach = 0;  // alignment_width while appending (clearSequence: 0)
    bool direct = true;
    uint32_t n = 0;
    for_each_emission(*t.input_sequence, r, tail, head, o.lowercase, pos, [&](uint32_t column, uint32_t base_bits) {
        if (column >= reach) reach = column;
        else column = reach;
        if (column >= width) direct = false;  // (setWidth would have to repack: the general way below)
        fin[n_out - 1 - n] = aligned_base::from_raw(((width - 1 - column) & 0xFFFFFFu) | base_bits);
        n++;
    });
    if (direct) {
        c.setWidth(width);
    } else {  // the same through the container's own operations
        c.clearSequence();
        for_each_emission(*t.input_sequence, r, tail, head, o.lowercase, pos, [&](uint32_t column, uint32_t base_bits) {
            c.append(aligned_base::from_raw((column & 0xFFFFFFu) | base_bits));
        });
        c.setWidth(width);
        c.reverse();
    }
    tk = host_tick("finish: assemble", tk);
    c.fix_duplicate_positions(t.log, o.lowercase == LOWERCASE_UNALIGNED, o.insertion == INSERTION_REMOVE);
    return host_tick("finish: NAST fix-up", tk);
}

// Takes a job, its slot's device result `r` and aligned columns `pos`; gives the tray its aligned sequence, attributes and log
// (backtrack()'s container steps, src/mesh.h:603-736, + do_align's attributes, src/align.cpp:507-509).  Throws on a failed query.
// pair_row (device-bps; else null): the six helix base-pair counters the align call counted for the slot -- the tray's
// score if the device assembled the alignment (only then the counters are of the finished words); gives whether it was taken.
// shift_row (device-shift; else null): the slot's row of the call's shift log -- its events become the log's
// "shifting bases to fit in ...;" texts, in order, in front of the totals, where the host's fix-up writes them.
static bool finish_tray(dp_job &jb, const sina_hip_align_out &r, const uint32_t *pos, uint32_t width, const aligner::options &o,
                        bool defer_score_line, const uint32_t *pair_row = nullptr, const uint32_t *shift_row = nullptr) {
    tray &t = *jb.t;
    if (r.status != 0) throw std::runtime_error("device alignment failed for " + t.input_sequence->getName());
    uint64_t tk = host_tsc();
    // the working copy: name and attributes of the input plus do_align's own (src/align.cpp:507-509,455-457),
    // made in one pass (cseq.h copy_meta_with); its bases follow
    const float score_q = r.raw / r.sum_weight;
    const std::string &date_text = make_datetime();
    const std::string &filter_name = t.astats->getName();
    struct keys_t {
        const std::string *head = cseq::attr_key(fn::head), *tail = cseq::attr_key(fn::tail), *filter = cseq::attr_key(fn::filter),
                          *qual = cseq::attr_key(fn::qual), *date = cseq::attr_key(fn::date);
    };
    static const keys_t keys;  // ("align_cutoff_head_slv" < "align_cutoff_tail_slv" < "align_filter_slv" < "align_quality_slv" < "aligned_slv")
    const cseq::attr_init extra[5] = {
        cseq::attr_init::of(keys.head, (int)r.cutoff_head),
        cseq::attr_init::of(keys.tail, (int)r.cutoff_tail),
        cseq::attr_init::of(keys.filter, std::string_view(filter_name)),
        cseq::attr_init::of(keys.qual, (int)std::min(100.f, std::max(0.f, 100.f * score_q))),
        cseq::attr_init::of(keys.date, std::string_view(date_text)),
    };
    cseq &c = *object_cache<cseq, cache_aligned_seq>::take();
    jb.c = &c;
    c.copy_meta_with(*t.input_sequence, extra, 5);
    tk = host_tick("finish: working copy + attributes", tk);
    if (r.assembled) {
        // the device did the container steps (append rule, setWidth, reverse) and the NAST fix-up -- one in which
        // every insertion fitted its gap, or (device-shift) its shifted runs too: the finished bases, and the
        // fix-up's log texts
        c.clearSequence();
        base_vector &fin = c.mutableAlignedBases();  // (a recycled sequence: no allocation)
        // (one pass, past the cache: base lists are not zeroed by resize() -- cseq.h, base_block_allocator -- and
        // nobody reads the finished list before a sink takes it)
        fin.resize(r.n_out);
        stream_copy(static_cast<void *>(fin.data()), pos, sizeof(aligned_base) * (size_t)r.n_out);
        c.setWidth(width);
        tk = host_tick("finish: assemble", tk);
        if (o.insertion == INSERTION_REMOVE) t.log << "insertion=remove not implemented, using shift; ";
        if (shift_row != nullptr)
            for (uint32_t e = 0; e < shift_row[0]; e++)
                t.log << "shifting bases to fit in " << shift_row[1 + 3 * e] << " bases at pos " << shift_row[2 + 3 * e] << " to "
                      << shift_row[3 + 3 * e] << ";";
        if (r.nast_total > 0)
            t.log << "total inserted bases=" << r.nast_total << ";"
                  << "longest insertion=" << r.nast_longest << ";"
                  << "total inserted bases before shifting=" << r.nast_last_run << ";";
        if (pair_row != nullptr) {
            t.bp_score = pair_score_from_counts(pair_row);
            t.bp_score_set = true;
        }
    } else {
        tk = assemble_on_host(t, c, r, pos, width, o, tk);
    }
    if (c.getWidth() > width) t.log << "warning: result sequence too wide!";
    // (the line itself is rendered when the log is read: tray::score_note -- or at once, for a caller that
    // reads the stream itself)
    const tray::score_note note{r.raw, r.sum_weight, score_q, (uint32_t)t.input_sequence->size(), (int32_t)r.aligned_bases,
                                (uint32_t)t.log.view().size(), true};
    if (defer_score_line) {
        t.pending_score = note;
    } else {
        char line[192];
        t.log.write(line, (std::streamsize)note.render(line, sizeof line));
    }
    tk = host_tick("finish: score log text", tk);
    if (o.write_used_rels) {
        std::string s;
        for (size_t y = 0; y < jb.family_size(); y++) s += jb.member(y)->getName() + " ";
        c.set_attr(fn::used_rels, s);
    }
    t.aligned_sequence = &c;
    host_tick("finish: attributes", tk);
    return r.assembled && pair_row != nullptr;
}

// --calc-idty (src/align.cpp:443-453): takes a finished group; gives every aligned query its best overlap identity with a
// member of its family as an attribute -- one comparison launch for the group (sina_hip_compare).
static void set_family_identity(const std::vector<dp_job *> &members, reference_store &store) {
    scoped_phase ph("al.calc_idty(C-ABI)");
    auto dev = store.worker_device(reference_store::dev_compare);
    const pair_counts pc = compare_packed(
        dev.get(), members.size(), [&](size_t x) -> const cseq & { return *members[x]->c; },
        [&](size_t x) { return members[x]->family_size(); },
        [&](size_t x, uint32_t *dst) {
            for (size_t y = 0; y < members[x]->family_size(); y++) dst[y] = store.id_of(members[x]->member(y));
        },
        SINA_CMP_IUPAC_OPTIMISTIC, 0);
    const cseq_comparator calc_id(CMP_IUPAC_OPTIMISTIC, CMP_DIST_NONE, CMP_COVER_OVERLAP, false);
    for (size_t x = 0; x < members.size(); x++) {
        float idty = 0;
        for (uint64_t y = pc.coff[x]; y < pc.coff[x + 1]; y++) idty = std::max(idty, calc_id.score(pc.counts[y]));
        members[x]->c->set_attr(fn::idty, 100.f * idty);
    }
}

// the plan's switches (align_plan.h) as the options have them
static align_switches plan_switches(const aligner::options &o) {
    align_switches s;
    s.fs_no_graph = o.fs_no_graph;
    s.device_graph = o.device_graph;
    s.device_profile = o.device_profile;
    s.wide_fallback = o.wide_fallback;
    s.weight_sets = o.weight_sets;
    s.device_bps = o.device_bps;
    s.device_idty = o.device_idty;
    s.calc_idty = o.calc_idty;
    s.device_shift = o.device_shift;
    s.device_search = o.device_search;
    return s;
}

// device-copy: the exact-relative test of a whole batch in ONE sina_hip_find_bases call on a leased
// worker context, before the trays are prepared.  Takes the batch as famfinder left it; gives, per tray, the answers for
// its suspects: the members of its family the store owns whose score is not below the query's k-mer count (what
// prepare_tray's lacks_query tests before it searches; scores that are no k-mer counts: every member).  Kept with the
// host walk, silently: members the store does not own; trays beyond the call's length limit; the whole batch if the
// call fails or is refused (the table stays empty).  A batch without suspects launches nothing.  walks: whether some
// suspect the store owns is left to the host walk (which reads the store's upper-case cache).
static std::vector<copy_answers> find_on_device(std::vector<tray> &batch, const aligner::options &o, reference_store &store, bool *walks) {
    scoped_phase ph("al.prepare(device-copy)");
    std::vector<copy_answers> table(batch.size());
    const unsigned max_len = max_query_len(o);
    std::vector<size_t> dev;  // the trays with suspects
    uint64_t too_long = 0;
    *walks = false;
    for (size_t i = 0; i < batch.size(); i++) {
        const tray &t = batch[i];
        if (!tray_is_complete(t) || t.input_sequence->size() > max_len || t.input_sequence->size() == 0) continue;
        const bool fits = t.input_sequence->size() <= sina_hip::kContainMaxBases;
        const float all_kmers = all_kmers_of(t);
        for (const search::result_item &item : *t.alignment_reference) {
            if (item.score < all_kmers || !store.owns(item.sequence)) continue;
            if (fits) table[i].at.emplace_back(item.sequence, sina_hip::kContainNone);
            else *walks = true;
        }
        if (!table[i].at.empty()) dev.push_back(i);
        else if (!fits && *walks) too_long++;
    }
    if (dev.empty()) {
        store.count_copy(0, too_long);
        return table;
    }
    const size_t n = dev.size();
    auto seq_of = [&](size_t x) -> const cseq & { return *batch[dev[x]].input_sequence; };
    const std::vector<uint64_t> qoff = offsets_of(n, seq_of);
    std::vector<uint64_t> coff(n + 1, 0);
    for (size_t x = 0; x < n; x++) coff[x + 1] = coff[x] + table[dev[x]].at.size();
    std::vector<uint8_t> qmask(qoff.back() + 1);
    pack_masks(n, seq_of, qoff.data(), qmask.data());
    std::vector<uint32_t> ids(coff.back()), at(coff.back(), sina_hip::kContainNone);
    for (size_t x = 0; x < n; x++)
        for (size_t y = 0; y < table[dev[x]].at.size(); y++) ids[coff[x] + y] = store.id_of(table[dev[x]].at[y].first);
    bool answered = false;
    try {
        scoped_phase call("al.find_bases(C-ABI)");
        reference_store::lease dv = store.worker_device(reference_store::dev_compare);
        answered = sina_hip_find_bases(dv.get(), qmask.data(), qoff.data(), (uint32_t)n, ids.data(), coff.data(), at.data()) == 0;
    } catch (const std::exception &) {  // (no context to be had: the walk)
    }
    if (!answered) {
        for (size_t i : dev) table[i].at.clear();
        *walks = true;
        store.count_copy(0, n + too_long);
        return table;
    }
    for (size_t x = 0; x < n; x++)
        for (size_t y = 0; y < table[dev[x]].at.size(); y++) table[dev[x]].at[y].second = at[coff[x] + y];
    store.count_copy(n, too_long);
    return table;
}

// Takes the batch (and the store's name; gives the store, if it can be had: a batch without DP jobs does without);
// prepares every tray.  Gives one job per tray: a tray that needs the DP has its job's `t` set.
static std::vector<dp_job> prepare_jobs(std::vector<tray> &batch, const aligner::options &o, const std::string &db,
                                        std::shared_ptr<reference_store> &store) {
    scoped_phase ph("al.prepare(partition)");
    std::vector<dp_job> jobs(batch.size());
    if (!db.empty()) {
        try {
            store = reference_store::get(db);
        } catch (const std::exception &) {  // (a batch without DP jobs does without the store)
        }
    }
    // (device-copy: the suspects' answers from one call; the store's upper-case cache only if a tray has to walk)
    bool walks = true;
    const std::vector<copy_answers> dev = o.device_copy && store ? find_on_device(batch, o, *store, &walks) : std::vector<copy_answers>();
    if (store && !batch.empty() && store->size() > 0 && walks) store->upper_bases(0);  // (fills the cache outside the loop)
    parallel_for(batch.size(), [&](size_t i) {
        if (!prepare_tray(batch[i], o, store.get(), dev.empty() || dev[i].at.empty() ? nullptr : &dev[i])) return;
        jobs[i].t = &batch[i];
        jobs[i].fam = batch[i].alignment_reference;
    });
    return jobs;
}

// What the steps of one group's trip to the device share.
struct group_call {
    const aligner::options &o;
    const align_switches &sw;
    reference_store &store;
    bool batch_driver;
    bool defer_score_line;
};

// Takes a group's key and slots; gives the group's positional weights (null: none): its one filter's, in place -- or,
// where its slots chose several, the distinct ones copied one after the other into `several`, with every slot's number
// among them in slots.set_of.
static const float *gather_weights(const aligner::options &o, const align_group_key &key, device_slots &slots, std::vector<float> &several) {
    const size_t n_weights = key.weight_width;
    if (n_weights == 0 || o.fs_no_graph) return nullptr;
    const float *weights = (*slots.members)[0]->t->astats->getWeights().data();
    if (key.filter != kAnyFilter) return weights;
    weight_sets sets = number_weight_sets(slots.dnq, [&](size_t u) { return slots.job(u).t->astats; });
    slots.n_sets = sets.n_sets();
    slots.set_of = std::move(sets.set_of);
    if (slots.n_sets > 1) {
        several.resize(slots.n_sets * n_weights);
        for (size_t x = 0; x < slots.n_sets; x++)
            memcpy(several.data() + x * n_weights, slots.job(sets.first_slot[x]).t->astats->getWeights().data(), 4 * n_weights);
        weights = several.data();
    }
    return weights;
}

// Sets the two in-place counting switches of the leased context as the plan has them for this group (either way: the
// context keeps the switches of whoever had it before); gives them.
static align_counting set_counting(sina_hip_ctx *ctx, const group_call &g, align_route route, const sina_hip_align_params &p) {
    const align_counting c = plan_counting(g.sw, route, g.batch_driver, g.sw.device_bps && g.store.pairs() != nullptr, p.assemble != 0);
    hip_check(sina_hip_align_count_pairs(ctx, c.count_pairs ? 1 : 0), "sina_hip_align_count_pairs");
    hip_check(sina_hip_align_count_identity(ctx, c.count_idty ? 1 : 0), "sina_hip_align_count_identity");
    return c;
}

static_assert(kSearchInplaceMaxResult == (int)sina_hip::kRankMaxResult && kSearchInplaceMaxCandidates == sina_hip::kKmerSelMax,
              "align_plan.h disagrees with rank_plan.h / kmer_plan.h");
// Sets the ranking switch of the leased context as the plan has it for this group (either way, as set_counting); gives
// whether the group's call ranks.  The store's name order is looked at -- and, the first time, uploaded -- only when
// everything else holds.
static bool set_search_inplace(sina_hip_ctx *ctx, const group_call &g, align_route route, const sina_hip_align_params &p) {
    bool ranks = false;
    search_stage_request rq{};
    if (g.sw.device_search) {
        rq = search_filter_request();
        search_stage_facts f;
        f.correction_none = rq.correction_none;
        f.ignore_super = rq.ignore_super;
        f.search_all = rq.search_all;
        f.max_result = rq.max_result;
        f.candidates = std::min<uint64_t>((uint64_t)std::max(rq.kmer_candidates, 0), g.store.size());
        f.same_store = !rq.database.empty() && rq.database == g.store.getFileName();
        f.index_matches = f.same_store && rq.kmer_len >= 1 && g.store.index_is((unsigned)rq.kmer_len, rq.no_fast);
        f.name_order = true;  // (asked last: the store's first answer computes and uploads the order)
        if (f.candidates >= 1 && plan_search_inplace(g.sw, route, p.assemble != 0, f)) {
            f.name_order = g.store.name_order_ready();
            ranks = plan_search_inplace(g.sw, route, p.assemble != 0, f);
        }
    }
    if (ranks)
        hip_check(sina_hip_align_rank(ctx, 1, (unsigned)rq.kmer_len, rq.no_fast ? 1 : 0, (uint32_t)rq.kmer_candidates, rq.iupac_rule,
                                      rq.filter_lowercase ? 1 : 0, rq.cover_rule, (uint32_t)rq.max_result),
                  "sina_hip_align_rank");
    else
        hip_check(sina_hip_align_rank(ctx, 0, 0, 0, 0, 0, 0, 0, 0), "sina_hip_align_rank");
    return ranks;
}

// The long route.  One call per slot: a wide mesh of this size fills a launch of the wide kernel nearly alone anyway,
// and a query whose mesh exceeds SINA_HIP_WIDE_CELLS -- the one thing a call refuses a well-formed query for -- then
// fails alone, softly, with the call's message in its log.  The trays of a slot are finished before the next call
// reuses the context's staged columns.
static void align_long_slots(sina_hip_ctx *ctx, const group_call &g, const sina_hip_align_params &p, const std::vector<dp_job *> &members,
                             const device_slots &slots, sina_hip_align_out *out) {
    std::vector<dp_job *> aligned;
    for (size_t u = 0; u < slots.dnq; u++) {
        const device_slots one = slots.only(u);
        uint64_t cells = 0;
        uint32_t width = 0;
        std::string refused;
        try {
            width = align_host_graphs(ctx, g.o, p, one, &out[u], &cells);
        } catch (const std::runtime_error &e) {
            if (cells <= SINA_HIP_WIDE_CELLS) throw;
            refused = e.what();
        }
        const uint32_t *const pos = sina_hip_staged_out_pos(ctx);
        // (a slot the call routed to the fast path may come back assembled, shifted runs included: its row is the call's first)
        const uint32_t *const shift_row = refused.empty() && p.assemble == SINA_ASSEMBLE_SHIFT ? sina_hip_staged_shift_log(ctx) : nullptr;
        uint64_t fin[2] = {0, 0};  // trays the host finished, trays the device had assembled
        for (size_t x = 0; x < members.size(); x++) {
            if (slots.slot_of[x] != u) continue;
            if (!refused.empty()) {
                members[x]->t->log << "unable to align: " << refused << ";";
                continue;
            }
            finish_tray(*members[x], out[u], pos, width, g.o, g.defer_score_line, nullptr, shift_row);
            fin[out[u].assembled ? 1 : 0]++;
            aligned.push_back(members[x]);
        }
        g.store.count_finished(fin[1], fin[0]);
    }
    if (g.o.calc_idty && !aligned.empty()) set_family_identity(aligned, g.store);
}

// Finishes the group's trays from out[slot] and the aligned columns where the device copied them, in the context's
// pinned staging buffer (sina_hip_staged_out_pos -- the context stays leased until the group's last tray is finished).
static void finish_group(sina_hip_ctx *ctx, const group_call &g, const std::vector<dp_job *> &members, const device_slots &slots,
                         const sina_hip_align_out *out, uint32_t width, bool counted_pairs, bool shifted, bool ranked) {
    const uint32_t *const staged_pos = sina_hip_staged_out_pos(ctx);
    // (null unless the call ran with assemble = 2; a slot's row: its shifted runs)
    const uint32_t *const staged_shift = shifted ? sina_hip_staged_shift_log(ctx) : nullptr;
    constexpr size_t shift_row_words = 1 + 3 * (size_t)SINA_HIP_SHIFT_LOG;
    // (null unless this call counted; the trays of a slot share its row)
    const uint32_t *const staged_pairs = counted_pairs ? sina_hip_staged_pair_counts(ctx) : nullptr;
    // (null unless this call ranked -- a call the device found a precondition missing for has not; a slot's row, cut to
    // its length, goes to the slot's trays: the search stage reads it, search_filter.cpp)
    const uint32_t *const staged_rank = ranked ? sina_hip_staged_rank(ctx) : nullptr;
    constexpr size_t rank_row_words = 2 + 2 * (size_t)kSearchInplaceMaxResult;
    scoped_phase ph("al.finish(NAST,log)");
    std::atomic<uint64_t> scored{0}, by_device{0};
    parallel_for(members.size(), [&](size_t x) {
        const uint32_t u = slots.slot_of[x];
        if (finish_tray(*members[x], out[u], staged_pos + slots.dqoff[u], width, g.o, g.defer_score_line,
                        staged_pairs ? staged_pairs + 6 * (size_t)u : nullptr, staged_shift ? staged_shift + shift_row_words * u : nullptr))
            scored.fetch_add(1, std::memory_order_relaxed);
        if (out[u].assembled) by_device.fetch_add(1, std::memory_order_relaxed);
        const uint32_t *const row = staged_rank ? staged_rank + rank_row_words * u : nullptr;
        if (row != nullptr && (row[1] & 2u) && row[0] <= (uint32_t)kSearchInplaceMaxResult) {
            auto cut = std::make_shared<std::vector<uint32_t>>(2 + 2 * (size_t)row[0]);
            (*cut)[0] = row[0], (*cut)[1] = row[1];
            std::copy(row + 2, row + 2 + row[0], cut->begin() + 2);
            std::copy(row + 2 + kSearchInplaceMaxResult, row + 2 + kSearchInplaceMaxResult + row[0], cut->begin() + 2 + row[0]);
            members[x]->t->search_row = std::move(cut);
        }
    });
    if (staged_pairs) g.store.count_pairs_inplace(scored.load());
    g.store.count_finished(by_device.load(), members.size() - by_device.load());
}

// --calc-idty for a finished group: from the rows the align call staged where it counted (device-idty), and by
// set_family_identity -- one comparison launch on a context of its own, while this group's is still leased -- for the rest.
static void set_group_identity(sina_hip_ctx *ctx, const group_call &g, const std::vector<dp_job *> &members, const device_slots &slots,
                               const sina_hip_align_out *out, bool counted_idty) {
    // (null unless this call counted -- a group redone over host-built graphs after a limit refusal has not)
    const uint32_t *const staged_idty = counted_idty ? sina_hip_staged_identity(ctx) : nullptr;
    if (staged_idty == nullptr) return set_family_identity(members, g.store);
    // device-idty: a tray whose slot the device assembled takes 100 x its slot's score (the trays of a slot share
    // the row); the trays the host finished go the old way
    std::vector<dp_job *> rest;
    uint64_t scored = 0;
    for (size_t x = 0; x < members.size(); x++) {
        const uint32_t u = slots.slot_of[x];
        if (!out[u].assembled) {
            rest.push_back(members[x]);
            continue;
        }
        float score;
        memcpy(&score, staged_idty + 2 * (size_t)u, 4);
        members[x]->c->set_attr(fn::idty, 100.f * score);
        scored++;
    }
    g.store.count_identity_inplace(scored);
    if (!rest.empty()) set_family_identity(rest, g.store);
}

// One group's trip: pack the queries and find the distinct ones, gather the weights, lease a context and set its
// counting switches, align the slots by the group's route, finish every tray and -- on request -- its identity.
static void align_group_members(const group_call &g, const align_group_key &key, const std::vector<dp_job *> &members) {
    device_slots slots = distinct_slots(members);
    std::vector<float> several;
    const float *weights = gather_weights(g.o, key, slots, several);
    const sina_hip_align_params p = make_align_params(g.o, g.sw, weights, key.weight_width);
    std::vector<sina_hip_align_out> out(slots.dnq);
    auto dev = g.store.worker_device(reference_store::dev_align);
    const align_counting counting = set_counting(dev.get(), g, key.route, p);
    const bool ranks = set_search_inplace(dev.get(), g, key.route, p);
    if (key.route == route_long) return align_long_slots(dev.get(), g, p, members, slots, out.data());
    // out[u] = slot u's result, its aligned columns at sina_hip_staged_out_pos + dqoff[u] while the context stays leased
    const uint32_t width = key.route == route_device ? align_family_ids(dev.get(), g.store, g.o, p, slots, out.data())
                                                     : align_host_graphs(dev.get(), g.o, p, slots, out.data());
    finish_group(dev.get(), g, members, slots, out.data(), width, counting.count_pairs, p.assemble == SINA_ASSEMBLE_SHIFT, ranks);
    if (g.o.calc_idty) set_group_identity(dev.get(), g, members, slots, out.data(), counting.count_idty);
}
}  // namespace

// src/align.cpp:307-460 for a batch of trays: prepare every tray, group those that need the DP (align_plan.h), then
// per group pack the queries, find the distinct ones, align them on the device, finish every tray and -- on request --
// its identity.
void aligner::operator()(std::vector<tray> &batch) { align_batch(batch, true); }

void aligner::align_batch(std::vector<tray> &batch, bool batch_driver) {
    const options &o = al_opts();
    const std::string db = o.database.empty() ? famfinder_database() : o.database;
    std::shared_ptr<reference_store> store;
    std::vector<dp_job> jobs = prepare_jobs(batch, o, db, store);
    std::vector<dp_job *> dp;
    std::vector<align_job_facts> facts;
    for (dp_job &jb : jobs)
        if (jb.t != nullptr) {
            dp.push_back(&jb);
            facts.push_back({jb.family_size(), jb.t->input_sequence->size(), jb.t->astats->getWeights().size(), jb.t->astats});
        }
    const align_switches sw = plan_switches(o);
    const std::vector<align_group> groups = plan_groups(sw, facts.data(), facts.size());
    if (!groups.empty() && !store) store = reference_store::get(db);  // (the DP needs the store: this throws what the lookup above met)
    for (const align_group &grp : groups) {
        std::vector<dp_job *> members(grp.members.size());
        for (size_t x = 0; x < members.size(); x++) members[x] = dp[grp.members[x]];
        align_group_members(group_call{o, sw, *store, batch_driver, defer_score_line}, grp.key, members);
    }
}

tray aligner::operator()(tray t) {
    std::vector<tray> b{t};
    align_batch(b, false);
    return b[0];
}

}  // namespace sina
