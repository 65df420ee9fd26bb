// Host side of the boundary: famfinder (its options, --turn, the auto-filter vote, the filter cascade over the
// k-mer search's candidates).  Behaviour follows the reference (citations inline).
#include "stages_internal.h"
#include "../family_plan.h"
#include <charconv>

#include <algorithm>
#include <cctype>
#include <cstdio>

namespace sina {

// ================================================================ famfinder

namespace {
struct ff_options {
    TURN_TYPE turn_which;
    ENGINE_TYPE engine;
    std::string posvar_filter;
    std::string posvar_autofilter_field;  // --auto-filter-field: empty = off
    float posvar_autofilter_thres;        // --auto-filter-threshold
    unsigned int fs_min, fs_max;
    float fs_msc, fs_msc_max;
    bool fs_leave_query_out;
    unsigned int fs_req, fs_req_full, fs_full_len, fs_req_gaps;
    bool fs_no_fast;
    unsigned int fs_kmer_len, fs_min_len, fs_cover_gene;
    std::string database;
    bool long_queries;  // search queries of up to SINA_HIP_MAX_LONG_QUERY_LEN bases (default off: SINA_HIP_MAX_QUERY_LEN)
    bool device_msc;    // fs-msc-max < 1: the candidates' identities from the device's match counts (default off: the host walk)
    bool device_cascade;  // the filter cascade on the device, behind the search (default off: match_pass below)
    bool device_turn;     // --turn: the device makes, searches and chooses the orientations (default off: best_orientations below)
};
ff_options ff_defaults() {  // src/famfinder.cpp:144-203
    ff_options o;
    o.turn_which = TURN_NONE;
    o.engine = ENGINE_SINA_KMER;
    o.fs_min = 40;
    o.fs_max = 40;
    o.fs_msc = .7f;
    o.fs_msc_max = 2;
    o.fs_leave_query_out = false;
    o.fs_req = 1;
    o.fs_req_full = 1;
    o.fs_full_len = 1400;
    o.fs_req_gaps = 10;
    o.fs_no_fast = false;
    o.fs_kmer_len = 10;
    o.fs_min_len = 150;
    o.fs_cover_gene = 0;
    o.long_queries = false;
    o.device_msc = false;
    o.device_cascade = false;
    o.device_turn = false;
    o.posvar_autofilter_thres = 0.8f;  // src/famfinder.cpp:205-208
    return o;
}
ff_options ff_opts = ff_defaults();

// cseq_comparator(CMP_IUPAC_OPTIMISTIC, CMP_DIST_NONE, CMP_COVER_QUERY, false)
// (src/cseq_comparator.cpp:59-117,211-295): column-wise merge walk
float identity_cover_query(const cseq &A, const cseq &B) {
    const auto &a = A.getAlignedBases();
    const auto &b = B.getAlignedBases();
    size_t i = 0, j = 0;
    const size_t ae = a.size(), be = b.size();
    if (ae == 0 || be == 0) return 0.f;
    int match = 0, mismatch = 0, only_a = 0, only_a_over = 0;
    if (a[0].getPosition() < b[0].getPosition()) {
        while (i != ae && a[i].getPosition() < b[j].getPosition()) { ++only_a_over; ++i; }
    } else {
        while (j != be && a[i].getPosition() > b[j].getPosition()) ++j;
    }
    while (i != ae && j != be) {
        const int diff = (int)a[i].getPosition() - (int)b[j].getPosition();
        if (diff > 0) ++j;
        else if (diff < 0) { ++only_a; ++i; }
        else {
            if (a[i].getBase().comp(b[j].getBase())) ++match; else ++mismatch;
            ++i; ++j;
        }
    }
    only_a_over += (int)(ae - i);
    const int base = match + mismatch + only_a + only_a_over;
    return (float)match / base;
}
}  // namespace

bool to_bool(const std::string &v) { return !(v.empty() || v == "0" || v == "false" || v == "no" || v == "off"); }
std::string lower(std::string s) {
    for (auto &c : s) c = (char)tolower((unsigned char)c);
    return s;
}
const std::string &famfinder_database() { return ff_opts.database; }

void famfinder::reset_options() { ff_opts = ff_defaults(); }

void famfinder::set_option(const std::string &name, const std::string &value) {
    ff_options &o = ff_opts;
    if (name == "db" || name == "ptdb") o.database = value;
    else if (name == "turn") {
        const std::string v = lower(value);
        if (v == "none") o.turn_which = TURN_NONE;
        else if (v == "revcomp" || v.empty()) o.turn_which = TURN_REVCOMP;
        else if (v == "all") o.turn_which = TURN_ALL;
        else throw std::logic_error("invalid value for --turn: " + value);
    } else if (name == "fs-engine") {
        if (lower(value) == "internal") o.engine = ENGINE_SINA_KMER;
        else throw std::logic_error("only the internal k-mer engine is available");
    } else if (name == "fs-kmer-len") o.fs_kmer_len = (unsigned)std::stoul(value);
    else if (name == "fs-req") o.fs_req = (unsigned)std::stoul(value);
    else if (name == "fs-min") o.fs_min = (unsigned)std::stoul(value);
    else if (name == "fs-max") o.fs_max = (unsigned)std::stoul(value);
    else if (name == "fs-msc") o.fs_msc = std::stof(value);
    else if (name == "fs-req-full") o.fs_req_full = (unsigned)std::stoul(value);
    else if (name == "fs-full-len") o.fs_full_len = (unsigned)std::stoul(value);
    else if (name == "fs-req-gaps") o.fs_req_gaps = (unsigned)std::stoul(value);
    else if (name == "fs-min-len") o.fs_min_len = (unsigned)std::stoul(value);
    else if (name == "fs-kmer-no-fast") o.fs_no_fast = to_bool(value);
    else if (name == "fs-msc-max") o.fs_msc_max = std::stof(value);
    else if (name == "fs-leave-query-out") o.fs_leave_query_out = to_bool(value);
    else if (name == "fs-cover-gene") o.fs_cover_gene = (unsigned)std::stoul(value);
    else if (name == "filter") o.posvar_filter = value;
    else if (name == "auto-filter-field") o.posvar_autofilter_field = value;
    else if (name == "auto-filter-threshold") o.posvar_autofilter_thres = std::stof(value);
    else if (name == "long-queries") o.long_queries = to_bool(value);
    else if (name == "device-msc") o.device_msc = to_bool(value);
    else if (name == "device-cascade") o.device_cascade = to_bool(value);
    else if (name == "device-turn") o.device_turn = to_bool(value);
    else throw std::logic_error("famfinder: unknown option " + name);
}

void famfinder::validate_options() {  // src/famfinder.cpp:213-239
    if (ff_opts.database.empty()) throw std::logic_error("Family Finder: Must have reference database (--db/-r)");
    if (ff_opts.fs_req < 1) throw std::logic_error("Family Finder: fs-req must be >= 1");
    if (ff_opts.fs_kmer_len < 1 || ff_opts.fs_kmer_len > 12)
        throw std::logic_error("Family Finder: fs-kmer-len must be in 1..12 on this engine");
}
ENGINE_TYPE famfinder::get_engine() { return ff_opts.engine; }
float famfinder::auto_filter_threshold() { return ff_opts.posvar_autofilter_thres; }

class famfinder::impl {
public:
    kmer_search *index{nullptr};
    std::shared_ptr<reference_store> arb;
    impl() : arb(reference_store::get(ff_opts.database)) {
        index = kmer_search::get_kmer_search(ff_opts.database, (int)ff_opts.fs_kmer_len, ff_opts.fs_no_fast);
    }
    ~impl() { delete index; }
    int turn_check(const cseq &query, bool all);
    std::vector<int> best_orientations(const std::vector<const cseq *> &queries, bool all);
    void orient_batch(std::vector<tray *> &batch);
    bool orient_on_device(std::vector<tray *> &batch, unsigned max, std::vector<search::result_vector> *found, std::vector<uint32_t> *nk);
    void select_astats(tray &t);
    void run(std::vector<tray *> &batch);
};

famfinder::famfinder() : pimpl(new impl()) {}
famfinder::famfinder(const famfinder &o) = default;
famfinder &famfinder::operator=(const famfinder &o) = default;
famfinder::~famfinder() = default;

int famfinder::turn_check(const cseq &query, bool all) { return pimpl->turn_check(query, all); }

// --turn (behaviour of src/famfinder.cpp:312-378): a query may arrive reversed and / or
// complemented.  Orientation o = (bit 0: reversed) | (bit 1: complemented); each candidate
// orientation gets one top-1 k-mer search and the strictly best-scoring one wins, the lowest o on
// ties and o = 0 when nothing scores above zero.  "revcomp" only tries o = 0 and o = 3, "all" tries
// the four.  All orientation variants of a whole batch go to the GPU as ONE top-1 search.
namespace {
cseq oriented(const cseq &q, int o) {
    cseq v(q);
    if (o & 1) v.reverse();
    if (o & 2) v.complement();
    return v;
}
const char *const orientation_names[4] = {"none", "reversed", "complemented", "reversed and complemented"};
}  // namespace

std::vector<int> famfinder::impl::best_orientations(const std::vector<const cseq *> &queries, bool all) {
    const int tried[4] = {0, 3, 1, 2};
    const int n_tried = all ? 4 : 2;
    std::vector<cseq> variants;
    variants.reserve(queries.size() * (size_t)n_tried);
    for (const cseq *q : queries)
        for (int x = 0; x < n_tried; x++) variants.push_back(oriented(*q, tried[x]));
    std::vector<const cseq *> vp;
    for (const cseq &v : variants) vp.push_back(&v);
    std::vector<search::result_vector> top1;
    index->find_batch(vp, top1, 1);
    std::vector<int> best(queries.size(), 0);
    for (size_t i = 0; i < queries.size(); i++) {
        float by_orientation[4] = {0, 0, 0, 0};
        for (int x = 0; x < n_tried; x++) {
            const search::result_vector &r = top1[i * (size_t)n_tried + x];
            if (!r.empty()) by_orientation[tried[x]] = r[0].score;
        }
        float top = 0;
        for (int o = 0; o < 4; o++)
            if (by_orientation[o] > top) {
                top = by_orientation[o];
                best[i] = o;
            }
    }
    return best;
}

int famfinder::impl::turn_check(const cseq &query, bool all) {
    return best_orientations(std::vector<const cseq *>{&query}, all)[0];
}

// turns the input sequences of a batch in place and records what was done (fn::turn)
void famfinder::impl::orient_batch(std::vector<tray *> &batch) {
    if (ff_opts.turn_which == TURN_NONE) {
        for (tray *t : batch) t->input_sequence->set_attr(fn::turn, "turn-check disabled");
        return;
    }
    std::vector<const cseq *> qs;
    for (tray *t : batch) qs.push_back(t->input_sequence);
    const std::vector<int> o = best_orientations(qs, ff_opts.turn_which == TURN_ALL);
    for (size_t i = 0; i < batch.size(); i++) {
        cseq &c = *batch[i]->input_sequence;
        c.set_attr(fn::turn, orientation_names[o[i]]);
        if (o[i]) c = oriented(c, o[i]);
    }
}

// device-turn: the batch's inputs go to the device as they are, once; it makes the orientations,
// searches them and chooses as turn_check does (sina_hip_kmer_topk_turn).  The inputs are then turned in place and
// fn::turn is set, as orient_batch does.  found (or null): the `max` best of every input AS TURNED -- a first round's
// rows -- with their k-mer counts in nk.  false: the call failed or was refused, nothing was done.
bool famfinder::impl::orient_on_device(std::vector<tray *> &batch, unsigned max, std::vector<search::result_vector> *found,
                                       std::vector<uint32_t> *nk) {
    std::vector<const cseq *> qs;
    for (tray *t : batch) qs.push_back(t->input_sequence);
    kmer_search::turn_request turn{ff_opts.turn_which == TURN_ALL, {}, false};
    std::vector<search::result_vector> top1;
    {
        scoped_phase ph_find("ff.find_batch");
        index->find_batch(qs, found ? *found : top1, max, found ? nk : nullptr, nullptr, nullptr, &turn);
    }
    if (!turn.done) {
        if (found) found->clear();
        return false;
    }
    for (size_t i = 0; i < batch.size(); i++) {
        cseq &c = *batch[i]->input_sequence;
        c.set_attr(fn::turn, orientation_names[turn.o[i]]);
        if (turn.o[i]) c = oriented(c, turn.o[i]);
    }
    return true;
}

int autofilter_vote(const std::vector<std::string> &filter_names, const std::vector<std::string> &field_texts,
                    const std::string &prefix, float threshold) {
    auto istarts_with = [](const std::string &text, const std::string &head) {
        if (head.size() > text.size()) return false;
        for (size_t i = 0; i < head.size(); i++)
            if (tolower((unsigned char)text[i]) != tolower((unsigned char)head[i])) return false;
        return true;
    };
    std::vector<std::string> texts;
    texts.reserve(field_texts.size());
    for (const std::string &f : field_texts) texts.push_back(prefix + ":" + f);
    int best_count = 0, best = -1;
    for (size_t x = 0; x < filter_names.size(); x++) {
        int n = 0;
        for (const std::string &f : texts)
            if (istarts_with(f, filter_names[x])) ++n;
        if (n > best_count) {  // (strictly: the first registered of equals stays -- the reference's "fixme")
            best_count = n;
            best = (int)x;
        }
    }
    // (int > size_t * float in the reference: both sides as float, the product rounded to float)
    const float quorum = (float)field_texts.size() * threshold;
    return (float)best_count > quorum ? best : -1;
}

// src/famfinder.cpp:381-436.  The tray points at the store's filter (stages.h, tray::astats); the fields the
// auto-filter reads are the store's per-reference database fields (reference_store::set_attr), a relative without
// the field contributing the empty string.
void famfinder::impl::select_astats(tray &t) {
    alignment_stats *astats = nullptr;
    std::deque<alignment_stats> &vastats = arb->getAlignmentStats();
    if (!ff_opts.posvar_filter.empty()) {
        for (alignment_stats &as : vastats) {
            if (as.getName() == ff_opts.posvar_filter || as.getName() == ff_opts.posvar_filter + ":ALL" ||
                as.getName() == ff_opts.posvar_filter + ":all")
                astats = &as;
        }
    }
    if (!ff_opts.posvar_autofilter_field.empty() && t.alignment_reference != nullptr) {
        std::vector<std::string> names, fields;
        names.reserve(vastats.size());
        for (const alignment_stats &as : vastats) names.push_back(as.getName());
        fields.reserve(t.alignment_reference->size());
        for (const auto &r : *t.alignment_reference) {
            arb->loadKey(*r.sequence, ff_opts.posvar_autofilter_field);
            fields.push_back(r.sequence->get_attr<std::string>(ff_opts.posvar_autofilter_field));
        }
        const int best = autofilter_vote(names, fields, ff_opts.posvar_filter, ff_opts.posvar_autofilter_thres);
        if (best >= 0) {
            t.log << "autofilter: " << vastats[(size_t)best].getName() << ";";
            astats = &vastats[(size_t)best];
        } else {
            t.log << "autofilter: no match;";
        }
    }
    if (astats == nullptr) astats = alignment_stats::shared_default();
    t.astats = astats;
}

// One pass of the filter cascade of famfinder::impl::match over ranked candidates
// (src/famfinder.cpp:497-612). Returns true when the loop condition
// says "enough".
namespace {
struct match_state {
    size_t have = 0, have_full = 0, have_cover_left = 0, have_cover_right = 0;
};
// match_row (device-msc; else null): the device's match count of every candidate, by its rank in the list as it came
// from the search -- the identity is then match / |query| instead of the walk
bool match_pass(search::result_vector &results, const cseq &query, match_state &st, const reference_store *store,
                const uint16_t *match_row = nullptr) {
    const ff_options &o = ff_opts;
    const size_t range_begin = 0, range_end = 0;
    st = match_state();
    const float query_bases = (float)query.size();
    auto remove_ranked = [&](const search::result_item &r, const uint16_t *match) {
        const cseq &s = *r.sequence;
        // (size, first and last column: out of the store's table for its own sequences)
        reference_store::ref_meta m;
        if (store && store->owns(r.sequence)) m = store->meta(store->id_of(r.sequence));
        else m = reference_store::ref_meta{(uint32_t)s.size(), s.size() ? s.begin()->getPosition() : 0u,
                                           s.size() ? s.getById(s.size() - 1).getPosition() : 0u};
        const bool is_full = m.size >= o.fs_full_len;
        const bool is_left = m.size && m.first_pos <= range_begin;
        const bool is_right = m.size && m.last_pos >= range_end;
        if (m.size < o.fs_min_len) return true;
        if (o.fs_leave_query_out && query.name_ref() == s.name_ref()) return true;
        if (o.fs_msc_max <= 2 && o.fs_msc_max < 1) {
            const float identity = match ? (query.size() ? (float)*match / query_bases : 0.f) : identity_cover_query(query, s);
            if (identity > o.fs_msc_max) return true;
        }
        const bool min_reached = st.have >= o.fs_min, max_reached = st.have >= o.fs_max;
        const bool score_good = r.score < o.fs_msc;  // sic (src/famfinder.cpp:565-567)
        const bool adds_to_full = o.fs_req_full && st.have_full < o.fs_req_full && is_full;
        const bool adds_to_range = (o.fs_cover_gene && st.have_cover_right < o.fs_cover_gene && is_right) ||
                                   (o.fs_cover_gene && st.have_cover_left < o.fs_cover_gene && is_left);
        if (min_reached && (max_reached || !score_good) && !adds_to_full && !adds_to_range) return true;
        ++st.have;
        if (o.fs_req_full && is_full) ++st.have_full;
        if (o.fs_cover_gene && is_right) ++st.have_cover_right;
        if (o.fs_cover_gene && is_left) ++st.have_cover_left;
        return false;
    };
    // (41 candidates out of a 100 000-sequence store: their records are asked for ahead of the pass)
    if (store)
        for (const auto &r : results)
            if (store->owns(r.sequence)) __builtin_prefetch(&store->meta(store->id_of(r.sequence)));
    if (match_row) {  // (the row is indexed by the rank before anything was removed: an explicit loop)
        size_t kept = 0;
        for (size_t i = 0; i < results.size(); i++) {
            if (remove_ranked(results[i], match_row + i)) continue;
            if (kept != i) results[kept] = std::move(results[i]);
            ++kept;
        }
        results.erase(results.begin() + (std::ptrdiff_t)kept, results.end());
    } else {
        auto remove = [&](const search::result_item &r) { return remove_ranked(r, nullptr); };
        results.erase(std::remove_if(results.begin(), results.end(), remove), results.end());
    }
    return !(st.have < o.fs_max || st.have_full < o.fs_req_full || st.have_cover_left < o.fs_cover_gene ||
             st.have_cover_right < o.fs_cover_gene);
}
}  // namespace

// The text of align_family_slv from the list famfinder left in its place (cseq.h lazy_text): items are
// reference id << 32 | whole-number score, owner the store.  The text is sized first and then written through a
// pointer (forty relatives were eighty checked appends).
void render_family_list(const void *owner, const uint64_t *items, size_t n, std::string &out) {
    reference_store *st = const_cast<reference_store *>(static_cast<const reference_store *>(owner));
    size_t total = 0;
    for (size_t x = 0; x < n; x++) {
        const uint32_t v = (uint32_t)items[x];
        const size_t digits = v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : 8;
        total += st->family_label((uint32_t)(items[x] >> 32)).size() + 1 + digits + 4;
    }
    out.resize(total);
    char *w = out.data();
    for (size_t x = 0; x < n; x++) {
        const std::string &label = st->family_label((uint32_t)(items[x] >> 32));
        memcpy(w, label.data(), label.size());
        w += label.size();
        *w++ = ':';
        w = std::to_chars(w, w + 10, (uint32_t)items[x]).ptr;
        memcpy(w, ".00 ", 4);
        w += 4;
    }
}

// src/famfinder.cpp:439-494 for a batch; the k-mer search of every escalation
// round is ONE launch over all queries still looking for relatives.
void famfinder::impl::run(std::vector<tray *> &batch) {
    const ff_options &o = ff_opts;
    std::vector<tray *> todo;
    // (the device takes queries of up to SINA_HIP_MAX_QUERY_LEN bases -- with long-queries, which lets the k-mer search
    // send the longer ones to its long count kernel, SINA_HIP_MAX_LONG_QUERY_LEN; a longer one fails alone, softly,
    // like a sequence without relatives -- not the whole batch)
    const unsigned max_len = o.long_queries ? SINA_HIP_MAX_LONG_QUERY_LEN : SINA_HIP_MAX_QUERY_LEN;
    std::vector<tray *> searchable;
    for (tray *t : batch) {
        if (t->input_sequence->size() > max_len) {
            t->log << "unable to align: sequence longer than " << max_len << " bases;";
            t->input_sequence->set_attr(fn::turn, "turn-check disabled");
        } else {
            searchable.push_back(t);
        }
    }
    // device-cascade: the cascade runs behind the search and a query's family comes back -- unless the
    // rule allows a family beyond the device's row, or the identity limit meets a store too wide for the match count
    // device-msc: every candidate's match count comes with the ids
    const bool device_cascade = o.device_cascade && o.engine == ENGINE_SINA_KMER &&
                                sina_hip::family_plan(o.fs_min, o.fs_max, o.fs_req_full, o.fs_cover_gene, 0).ok &&
                                !(o.fs_msc_max < 1 && arb->match_counts_too_wide());
    const bool device_msc = o.device_msc && o.fs_msc_max < 1 && !device_cascade;
    size_t max_results = (size_t)o.fs_max + 1;
    const unsigned isize = index->size();
    // device-turn: where the first round is the plain search its rows come with the orientation; where it rides with
    // match counts or the cascade only the orientation is taken (max = 1) and the round runs as ever on the turned input
    std::vector<search::result_vector> turn_found;
    std::vector<uint32_t> turn_nk;
    bool first_round_found = false;
    {
        scoped_phase ph_orient("ff.orient");
        if (o.device_turn && o.turn_which != TURN_NONE && o.engine == ENGINE_SINA_KMER && !searchable.empty()) {
            const bool rows = !device_msc && !device_cascade;
            if (orient_on_device(searchable, rows ? (unsigned)std::min<size_t>(max_results, isize) : 1u, rows ? &turn_found : nullptr, &turn_nk)) {
                first_round_found = rows;
                arb->count_turn(rows ? searchable.size() : 0, rows ? 0 : searchable.size(), 0);
            } else {
                arb->count_turn(0, 0, searchable.size());
                orient_batch(searchable);
            }
        } else {
            orient_batch(searchable);
        }
    }
    for (tray *t : searchable) {
        t->alignment_reference = object_cache<search::result_vector>::take();
        // (what the scores below are: raw k-mer counts of this engine -- the aligner's containment pre-filter asks)
        t->family_scores_kmer_k = o.engine == ENGINE_SINA_KMER ? (o.fs_no_fast ? -(int)o.fs_kmer_len : (int)o.fs_kmer_len) : 0;
        t->query_kmer_count = -1;
        todo.push_back(t);
    }
    while (!todo.empty()) {
        std::vector<const cseq *> qs;
        for (tray *t : todo) qs.push_back(t->input_sequence);
        std::vector<search::result_vector> found(todo.size());
        for (size_t i = 0; i < todo.size(); i++) found[i].swap(*todo[i]->alignment_reference);  // (their heap blocks, recycled)
        std::vector<uint32_t> nk;
        // device-msc: an empty row: that query keeps the walk; device-cascade: for a query the device cannot take,
        // match_pass below
        kmer_search::family_request family{
            sina_hip_family_rule{o.fs_min, o.fs_max, o.fs_req_full, o.fs_full_len, o.fs_min_len, o.fs_cover_gene, o.fs_msc, o.fs_msc_max},
            o.fs_leave_query_out, {}};
        std::vector<std::vector<uint16_t>> match_rows;
        if (first_round_found) {  // (device-turn searched the turned inputs with this round's max already)
            first_round_found = false;
            found.swap(turn_found);
            nk.swap(turn_nk);
        } else {
            scoped_phase ph_find("ff.find_batch");
            index->find_batch(qs, found, (unsigned)std::min<size_t>(max_results, isize),
                              o.engine == ENGINE_SINA_KMER ? &nk : nullptr, device_msc ? &match_rows : nullptr,
                              device_cascade ? &family : nullptr);
        }
        for (size_t i = 0; i < nk.size(); i++) todo[i]->query_kmer_count = (int)nk[i];
        std::vector<char> done(todo.size(), 0);
        scoped_phase ph_match("ff.match_pass");
        parallel_for(todo.size(), [&](size_t i) {
            search::result_vector &res = *todo[i]->alignment_reference;
            res.swap(found[i]);
            if (device_cascade && (family.state[i] & kmer_search::family_request::on_device)) {  // (res is the family)
                const uint8_t state = family.state[i];
                done[i] = ((state & (kmer_search::family_request::enough | kmer_search::family_request::empty_list)) || max_results >= isize) ? 1 : 0;
                return;
            }
            if (res.empty()) {
                done[i] = 1;
                return;
            }
            match_state st;
            const uint16_t *row = device_msc && match_rows[i].size() == res.size() ? match_rows[i].data() : nullptr;
            const bool enough = match_pass(res, *todo[i]->input_sequence, st, arb.get(), row);
            done[i] = (enough || max_results >= isize) ? 1 : 0;
        });
        std::vector<tray *> next;
        for (size_t i = 0; i < todo.size(); i++)
            if (!done[i]) next.push_back(todo[i]);
        todo.swap(next);
        max_results *= 10;
    }
    scoped_phase ph_post("ff.post");
    parallel_for(batch.size(), [&](size_t i) {
        tray &t = *batch[i];
        if (t.alignment_reference == nullptr) {  // (not searched, see above)
            select_astats(t);
            return;
        }
        auto &vc = *t.alignment_reference;
        cseq &c = *t.input_sequence;
        uint64_t tk = host_tsc();
        // "<acc>.<start>:<score> " per relative (famfinder.cpp:462-470), ":%.2f " for the score.  Where every
        // relative is of the store and has a whole-number score (k-mer counts are) the attribute is kept as the
        // list of (id, score) and the text made when it is read (cseq.h lazy_text, render_family_list below).
        bool plain = true;
        for (auto &r : vc) {
            const float sc = r.score;
            if (!(arb->owns(r.sequence) && sc >= 0.f && sc < 16777216.f && sc == (float)(uint32_t)sc)) {
                plain = false;
                break;
            }
        }
        if (plain) {
            std::vector<uint64_t> &items = c.set_lazy_attr(fn::family, arb.get(), &render_family_list);
            items.resize(vc.size());
            for (size_t x = 0; x < vc.size(); x++) items[x] = ((uint64_t)arb->id_of(vc[x].sequence) << 32) | (uint32_t)vc[x].score;
        } else {
            std::string &fam = c.string_slot(fn::family);  // (written in place, into the sequence's recycled block)
            char buf[64];
            fam.reserve(vc.size() * 24);
            for (auto &r : vc) {
                snprintf(buf, sizeof(buf), ":%.2f ", (double)r.score);
                if (arb->owns(r.sequence)) {
                    fam += arb->family_label(arb->id_of(r.sequence));  // (the "<acc>.<start>" part, cached per reference)
                } else {
                    arb->loadKey(*r.sequence, fn::acc);
                    arb->loadKey(*r.sequence, fn::start);
                    fam += r.sequence->get_attr<std::string>(fn::acc) + "." + r.sequence->get_attr<std::string>(fn::start, "0");
                }
                fam += buf;
            }
        }
        tk = host_tick("ff.post: family string", tk);
        if (o.fs_req_gaps != 0) {  // :472-480
            auto too_few_gaps = [&](search::result_item &it) {
                if (arb->owns(it.sequence)) {
                    const reference_store::ref_meta &m = arb->meta(arb->id_of(it.sequence));
                    return 0 == m.size || m.last_pos - m.size + 1 < o.fs_req_gaps;
                }
                return 0 == it.sequence->size() ||
                       it.sequence->rbegin()->getPosition() - it.sequence->size() + 1 < o.fs_req_gaps;
            };
            vc.erase(std::remove_if(vc.begin(), vc.end(), too_few_gaps), vc.end());
        }
        select_astats(t);
        host_tick("ff.post: gaps filter + astats", tk);
        if (vc.size() < o.fs_req) {  // :486-491
            t.log << "unable to align: too few relatives (" << vc.size() << ");";
            object_cache<search::result_vector>::give(t.alignment_reference);
            t.alignment_reference = nullptr;
        }
    });
}

tray famfinder::operator()(const tray &t) {
    tray r(t);
    std::vector<tray *> b{&r};
    pimpl->run(b);
    return r;
}
void famfinder::operator()(std::vector<tray> &batch) {
    std::vector<tray *> b;
    for (auto &t : batch) b.push_back(&t);
    pimpl->run(b);
}

}  // namespace sina
