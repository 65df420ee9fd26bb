// Plain-C driver over the C++ stage mirror, for pytest / bench.py (ctypes).
// Not part of the drop-in boundary (that is include/sina_hip.h below the stages
// and the famfinder/aligner classes above it); this only lets Python feed trays
// through the stages and read the results back.
#include <malloc.h>
#include <sys/mman.h>
#include <atomic>
#include <charconv>
#include <chrono>
#include <cstring>

#include "stages.h"
#include "flow.h"
#include "id_order.h"

#include <fstream>
#include <map>
#include <sstream>
#include <thread>
#include <memory>

using namespace sina;

namespace {
thread_local std::string g_err;
std::atomic<double> g_last_avg_bps{0.0};  // avg_bps of the last finished FASTA run (sina_host_last_avg_bps)
int fail(const std::exception &e) {
    g_err = e.what();
    return 1;
}
// The exception boundary of an exported function: f(), then 0 -- or 1, with what f threw kept for sina_host_last_error
template <class F>
int guarded(F &&f) {
    try {
        f();
        return 0;
    } catch (const std::exception &e) {
        return fail(e);
    }
}

struct result {
    // (between runs a result keeps its heap blocks: fresh memory per query is a page fault per query)
    void reset() {
        status = 2;
        head = tail = qual = 0;
        width = 0;
        ab = nullptr;
        n_ab = 0;
        own.clear();
        log.clear();
        note.set = false;
        family.clear();
        family_items.clear();
        family_render = nullptr;
        idty = -1.f;
        bps = 0.f;
        searched = false;
        sr_ids.clear();
        sr_scores.clear();
        attrs.clear();
    }
    int status = 2;  // 0 aligned by DP, 1 alignment copied from a reference, 2 not aligned
    int head = 0, tail = 0, qual = 0;
    uint32_t width = 0;
    const aligned_base *ab = nullptr;  // the aligned bases: own.data()
    uint32_t n_ab = 0;
    // The aligned bases, TAKEN from the tray's aligned sequence (the two exchange their base lists: the sequence
    // goes back to its cache with this record's previous block, so neither allocates in steady state).  Until
    // round 5 the sink copied them into an arena of the pipeline's -- the fifth time a query's 6 KB went through
    // a core; what a real sink does with them (format, write) it does from the sequence itself.
    base_vector own;
    mutable std::string log;          // (the tray's log; its score line is put in when the log is asked for)
    mutable tray::score_note note;
    // align_family_slv: as text, or as the list famfinder left (rendered by sina_host_result_family; the store is
    // kept alive by the pipeline's stages)
    mutable std::string family;
    std::vector<uint64_t> family_items;
    const void *family_owner = nullptr;
    void (*family_render)(const void *, const uint64_t *, size_t, std::string &) = nullptr;
    float idty = -1.f;              // align_ident_slv (--calc-idty), -1 if not computed
    // --show-dist (host option show-dist): sps, idty, cpm and the closest relative's id where the report has one
    float dist[3] = {0.f, 0.f, 0.f};
    uint32_t dist_closest = 0xFFFFFFFFu;
    bool have_dist = false;
    float bps = 0.f;                // the helix base-pair score (align_bp_score_slv = (int)(100 * bps)); 0 without a helix map
    bool searched = false;          // search stage ran and produced a result vector
    std::vector<uint32_t> sr_ids;   // search results, best first
    std::vector<float> sr_scores;
    // turn, nearest_slv, lca_*, copy_*: a handful per query.  A flat list whose strings keep their blocks from
    // one query to the next (a std::map was two heap blocks per attribute and query, freed by reset())
    struct attr_list {
        std::vector<std::pair<std::string, std::string>> v;
        size_t n = 0;
        void clear() { n = 0; }
        std::string &operator[](std::string_view key) {
            for (size_t i = 0; i < n; i++)
                if (v[i].first == key) return v[i].second;
            if (n == v.size()) v.emplace_back();
            v[n].first.assign(key);
            v[n].second.clear();
            return v[n++].second;
        }
        const std::string *find(std::string_view key) const {
            for (size_t i = 0; i < n; i++)
                if (v[i].first == key) return &v[i].second;
            return nullptr;
        }
    } attrs;
};

struct pipeline {
    famfinder ff;
    aligner al;
    pipeline() { al.defer_score_line = true; }  // (this driver's sink reads a tray's log through log_text())
    std::unique_ptr<search_filter> sf;  // only with sina_host_pipeline_create_search()
    std::shared_ptr<reference_store> search_store;
    double sf_s = 0;
    // The results of a run, batch by batch: chunk b holds the results of queries [b * chunk_q, (b + 1) * chunk_q)
    // (each with its aligned bases).  A chunk is sized and reset by the sink when its batch arrives
    // (and kept between runs) -- sizing everything before the first batch was 17 ms of every run's start.
    struct result_chunk {
        std::vector<result> results;
        uint64_t run = 0;  // the run (pipeline::run_no) whose sink filled it: an older one's results are not this run's
    };
    uint64_t run_no = 0;
    std::vector<result_chunk> chunks;
    uint32_t chunk_q = 1, n_results = 0;
    result &result_of(uint32_t q) { return chunks[q / chunk_q].results[q % chunk_q]; }
    double wall_s = 0, ff_s = 0, al_s = 0;
    // A batch's trays (6144 objects with a stringstream each) travel from the source to the sink and come
    // back here, emptied, for the next batch -- and the next run: constructing and destroying them per batch
    // was 1.5 us per query on the two driver threads that did it, and 6 ms before a run's first GPU call.
    std::mutex spare_mu;
    std::vector<std::vector<tray>> spare_trays;
    std::vector<tray> take_trays() {
        std::lock_guard<std::mutex> lk(spare_mu);
        if (spare_trays.empty()) return {};
        std::vector<tray> v = std::move(spare_trays.back());
        spare_trays.pop_back();
        return v;
    }
    void give_trays(std::vector<tray> &&v) {
        std::lock_guard<std::mutex> lk(spare_mu);
        if (spare_trays.size() < 16) spare_trays.push_back(std::move(v));
    }
};
// The sink's work for one tray (what SINA's writer stage does per sequence): log, family, attributes and the
// aligned bases go into the result record (a DP alignment has exactly the query's bases, a copied one its
// reference's: never more than the query, which the copy short-cut requires to be contained in it) -- and the
// tray gives its objects back.
// (helix: the store's helix map, for a tray that no pair step has scored -- or null)
void extract_tray(pipeline *p, tray &t, result &r, uint32_t query_bases, const reference_store::pair_map &helix) {
    r.reset();
    uint64_t tk = host_tsc();
    r.log.assign(t.log.view());  // (no temporary: the result's string keeps its block between runs)
    r.note = t.pending_score;
    if (const cseq::lazy_text *lz = t.input_sequence->lazy_attr(fn::family)) {  // (the list; the text when it is asked for)
        r.family_items.assign(lz->items.begin(), lz->items.end());
        r.family_owner = lz->owner;
        r.family_render = lz->render;
    } else if (const std::string *fam = t.input_sequence->string_attr(fn::family)) r.family.assign(*fam);
    else r.family = t.input_sequence->get_attr<std::string>(fn::family);
    if (const std::string *turn = t.input_sequence->string_attr(fn::turn)) r.attrs[fn::turn].assign(*turn);
    else if (t.input_sequence->has_attr(fn::turn)) r.attrs[fn::turn] = t.input_sequence->get_attr<std::string>(fn::turn);
    tk = host_tick("extract: log + family + turn", tk);
    if (t.aligned_sequence) {
        cseq &c = *t.aligned_sequence;
        r.bps = tray_pair_score(t, helix);
        if (show_dist_wanted()) {  // (the metric alone: the report's text is the FASTA drivers')
            log_printer::report rep;
            show_dist_of_tray(t, rep);
            if (rep.has_closest) {
                r.dist[0] = rep.sps;
                r.dist[1] = rep.idty;
                r.dist[2] = rep.cpm;
                r.dist_closest = rep.closest_id;
                if (rep.closest_seq != nullptr)
                    for (const std::string &key : {aligner::opts->database, search_filter_database()})
                        if (const std::shared_ptr<reference_store> st = key.empty() ? nullptr : reference_store::find(key))
                            if (st->owns(rep.closest_seq)) {
                                r.dist_closest = st->id_of(rep.closest_seq);
                                break;
                            }
                r.have_dist = true;
            }
        }
        r.width = c.getWidth();
        r.status = (r.log.find("copied alignment from") != std::string::npos) ? 1 : 0;
        // one walk over the attributes, the stages' own keys told by their interned addresses
        struct keys_t {
            const std::string *qual = cseq::attr_key(fn::qual), *head = cseq::attr_key(fn::head), *tail = cseq::attr_key(fn::tail),
                              *idty = cseq::attr_key(fn::idty), *nearest = cseq::attr_key(search_filter::fn_nearest),
                              *filter = cseq::attr_key(fn::filter);
        };
        static const keys_t keys;
        r.idty = -1.f;
        for (const auto &kv : c.attrs_unsettled()) {
            const int *iv = std::get_if<int>(&kv.second);
            if (kv.name == keys.qual) r.qual = iv ? *iv : c.get_attr<int>(fn::qual);
            else if (kv.name == keys.head) r.head = iv ? *iv : c.get_attr<int>(fn::head);
            else if (kv.name == keys.tail) r.tail = iv ? *iv : c.get_attr<int>(fn::tail);
            else if (kv.name == keys.idty) r.idty = c.get_attr<float>(fn::idty);
            else if (kv.name == keys.filter) {  // (align_filter_slv: kept where a filter was chosen; absent reads as "")
                const std::string *f = std::get_if<std::string>(&kv.second);
                if (f && !f->empty()) r.attrs[fn::filter].assign(*f);
            } else {
                const std::string &k = kv.key();
                if (kv.name == keys.nearest || k.compare(0, 4, "lca_") == 0 || k.compare(0, 5, "copy_") == 0)
                    r.attrs[k] = c.get_attr<std::string>(k);
            }
        }
        (void)query_bases;
        r.own.swap(c.mutableAlignedBases());
        r.n_ab = (uint32_t)r.own.size();
        r.ab = r.own.data();
    }
    if (t.search_result) {
        r.searched = true;
        for (const auto &sr : *t.search_result) {
            r.sr_ids.push_back(p->search_store->id_of(sr.sequence));
            r.sr_scores.push_back(sr.score);
        }
    }
    tk = host_tick("extract: aligned attrs + bases", tk);
    t.destroy();
    host_tick("extract: tray.destroy", tk);
}

// An unaligned query as the reader stage would hand it over: base i in column i.
void fill_query_tray(tray &t, uint32_t q, const uint8_t *qmask, const uint64_t *qoff) {
    uint64_t tk = host_tsc();
    t.seqno = q;
    // (trays are reused from batch to batch: a fresh log -- destroy() frees the sequences but leaves the
    // text, and the previous occupant's would lead this one's)
    t.clear_log();
    t.input_sequence = object_cache<cseq, cache_query_seq>::take();
    {
        char name[24] = "query";
        char *e = std::to_chars(name + 5, name + sizeof name, q).ptr;
        t.input_sequence->setName(std::string_view(name, (size_t)(e - name)));
    }
    tk = host_tick("build: log reset + new cseq", tk);
    // (base i in column i: the sequence keeps the mask bytes, cseq.h "dense" -- the packed words are made if a
    // stage asks for them)
    const uint32_t n_bases = (uint32_t)(qoff[q + 1] - qoff[q]);
    t.input_sequence->setDenseMasks(qmask + qoff[q], n_bases);
    host_tick("build: bases", tk);
}

// An ALIGNED query under its own name: packed aligned bases (column | mask << 24) as a reader of aligned input hands
// them over -- what the identity filter (--fs-msc-max) and --fs-leave-query-out look at.
void fill_aligned_query_tray(tray &t, uint32_t q, const uint32_t *q_ab, const uint64_t *q_off, const char *name, uint32_t width) {
    t.seqno = q;
    t.clear_log();
    t.input_sequence = object_cache<cseq, cache_query_seq>::take();
    t.input_sequence->setName(std::string_view(name));
    static_assert(sizeof(aligned_base) == 4, "packed words");
    t.input_sequence->setAlignedBases(reinterpret_cast<const aligned_base *>(q_ab + q_off[q]), (size_t)(q_off[q + 1] - q_off[q]));
    uint32_t cols = width;  // (a base beyond the store's alignment stays where it is)
    for (uint64_t i = q_off[q]; i < q_off[q + 1]; i++) cols = std::max(cols, (q_ab[i] & 0xFFFFFFu) + 1u);
    t.input_sequence->setWidth(cols);
}

// ---- what the staged drivers below share (the runner itself: flow.h)
// what a queue does with a batch nobody will take any more
void destroy_trays(std::vector<tray> &trays) {
    for (auto &t : trays) t.destroy();
}
// f(), its wall time added to ns
template <class F>
void timed(std::atomic<uint64_t> &ns, F &&f) {
    const auto a = std::chrono::steady_clock::now();
    f();
    ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - a).count();
}
// The device contexts that n_find famfinder threads and n_align aligner (+ search) threads will lease, made and
// warmed before any of them starts.  search_store(): the search stage's store, or null without that stage.
template <class SearchStore>
void reserve_workers(SearchStore &&search_store, unsigned n_find, unsigned n_align) {
    try {
        const auto store = reference_store::get(aligner::opts->database);
        const std::shared_ptr<reference_store> sstore = search_store();
        store->reserve_workers(reference_store::dev_search, n_find + (sstore == store ? n_align : 0));
        store->reserve_workers(reference_store::dev_align, n_align);
        // (the pair step; the aligner's device-copy pre-pass)
        if ((store->pairs() || aligner::opts->device_copy) && sstore != store) store->reserve_workers(reference_store::dev_compare, n_align);
        if (sstore) {
            if (sstore != store) sstore->reserve_workers(reference_store::dev_search, n_align);
            sstore->reserve_workers(reference_store::dev_compare, n_align);
        }
    } catch (const std::exception &) {
        // (a store that cannot be opened yet, or no room to warm: the stage that needs it will say so itself)
    }
}
}  // namespace

extern "C" {
static void tune_allocator();

const char *sina_host_last_error(void) { return g_err.c_str(); }

int sina_host_store_from_packed(const char *key, const uint32_t *ab, const uint64_t *off, uint32_t n, uint32_t width,
                                int device) {
    return guarded([&] {
        auto s = reference_store::from_packed(key, ab, off, n, width);
        s->set_device(device);
    });
}

// A store of a rank other than 0: its device buffers are allocated like rank 0's
// (sina_hip_store_alloc_like) and filled by the start-up broadcast instead of an upload of its own.
int sina_host_store_expect_broadcast(const char *key) {
    return guarded([&] {
        reference_store::get(key)->expect_broadcast();
    });
}

int sina_host_store_close(const char *key) {
    return guarded([&] {
        for (int k = 1; k <= 12; k++)
            for (int nf = 0; nf < 2; nf++) kmer_search::release_kmer_search(key, k, nf != 0);
        reference_store::close(key);
    });
}

int sina_host_add_filter(const char *key, const char *name, const float *weights, uint32_t n) {
    return guarded([&] {
        reference_store::get(key)->getAlignmentStats().emplace_back(std::string(name),
                                                                    std::vector<float>(weights, weights + n));
    });
}

// Test hook, no device involved: the --auto-filter-field vote (autofilter_vote, stages.h) of a family given as
// reference ids over the store's registered filters and its references' `field`.  *chosen: the filter's number in
// registration order, or -1 (no match); its name goes to name_out (if given; empty for no match).  A negative
// threshold stands for famfinder's --auto-filter-threshold as it is set.
int sina_host_autofilter_vote(const char *key, const uint32_t *ids, uint32_t n, const char *field, const char *prefix,
                              float threshold, int *chosen, char *name_out, uint32_t name_cap) {
    return guarded([&] {
        auto st = reference_store::get(key);
        std::vector<std::string> names, fields;
        for (const alignment_stats &as : st->getAlignmentStats()) names.push_back(as.getName());
        for (uint32_t x = 0; x < n; x++) {
            if (ids[x] >= st->size()) throw std::logic_error("autofilter_vote: no such reference");
            fields.push_back(st->getCseq(ids[x]).get_attr<std::string>(field));
        }
        const int best = autofilter_vote(names, fields, prefix, threshold < 0.f ? famfinder::auto_filter_threshold() : threshold);
        if (chosen) *chosen = best;
        if (name_out && name_cap) snprintf(name_out, name_cap, "%s", best >= 0 ? names[(size_t)best].c_str() : "");
    });
}

// Device context of a store (creates it and uploads the references on first use): lets a
// launcher reach sina_hip_store_view_get / sina_hip_store_alloc_like for the start-up
// broadcast of the index over RCCL.
void *sina_host_store_ctx(const char *key) {
    try {
        return reference_store::get(key)->device();
    } catch (const std::exception &e) {
        fail(e);
        return nullptr;
    }
}
int sina_host_store_slow_path_queries(const char *key, uint64_t *wide, uint64_t *long_kmer) {
    return guarded([&] {
        reference_store::get(key)->slow_path_queries(wide, long_kmer);
    });
}
int sina_host_store_big_select_queries(const char *key, uint64_t *n) {
    return guarded([&] {
        reference_store::get(key)->big_select_queries(n);
    });
}
int sina_host_store_match_stats(const char *key, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches) {
    return guarded([&] {
        reference_store::get(key)->match_stats(kernel_ms, pairs, cand_bases, launches);
    });
}
// famfinder's device-cascade on this store: the cascade kernel's time and volume (sina_hip_family_stats) on its contexts
int sina_host_store_family_stats(const char *key, double *kernel_ms, uint64_t *queries, uint64_t *candidates_listed,
                                 uint64_t *candidates_scanned, uint64_t *launches) {
    return guarded([&] {
        reference_store::get(key)->family_stats(kernel_ms, queries, candidates_listed, candidates_scanned, launches);
    });
}
// search_filter's device-rank on this store: queries ranked on the device, queries sent back to the host path, and the
// rank kernel's time and volume (sina_hip_rank_stats) on its contexts -- between runs, like the counters above
int sina_host_store_rank_stats(const char *key, uint64_t *ranked, uint64_t *fallen_back, double *kernel_ms, uint64_t *pairs,
                               uint64_t *cand_bases, uint64_t *launches) {
    return guarded([&] {
        reference_store::get(key)->rank_stats(ranked, fallen_back, kernel_ms, pairs, cand_bases, launches);
    });
}
// The helix map of a store (reference_store::set_pairs): pairs[i] = partner column of column i, 0 = unpaired; n == 0 or
// all zero removes it.  Before the stages run, like sina_host_add_filter.
int sina_host_store_set_pairs(const char *key, const uint32_t *pairs, uint32_t n) {
    return guarded([&] {
        if (!pairs && n) throw std::logic_error("store_set_pairs: null argument");
        reference_store::get(key)->set_pairs(pairs, n);
    });
}
// ... and the pair-count kernel's time and volume on the store's contexts (sina_hip_pair_stats) -- between runs
int sina_host_store_pair_stats(const char *key, double *kernel_ms, uint64_t *sequences, uint64_t *entries_visited, uint64_t *launches) {
    return guarded([&] {
        reference_store::get(key)->pair_stats(kernel_ms, sequences, entries_visited, launches);
    });
}
// the aligner's device-bps on this store: trays scored from the counters their align call brought back, and the
// in-place kernel's time and volume (sina_hip_pair_inplace_stats) on its contexts -- between runs
int sina_host_store_pair_inplace_stats(const char *key, uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *launches) {
    return guarded([&] {
        if (!trays || !kernel_ms || !sequences || !launches) throw std::logic_error("store_pair_inplace_stats: null argument");
        reference_store::get(key)->pair_inplace_stats(trays, kernel_ms, sequences, launches);
    });
}
// the aligner's device-idty on this store: trays that took their identity from the row their align call brought back,
// and the in-place kernel's time and volume (sina_hip_identity_inplace_stats) on its contexts -- between runs
int sina_host_store_identity_inplace_stats(const char *key, uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs,
                                           uint64_t *launches) {
    return guarded([&] {
        if (!trays || !kernel_ms || !sequences || !pairs || !launches) throw std::logic_error("store_identity_inplace_stats: null argument");
        reference_store::get(key)->identity_inplace_stats(trays, kernel_ms, sequences, pairs, launches);
    });
}
// the aligner's device-search on this store: trays whose search rows came from the row their align call brought back,
// and the in-place ranking's time and volume (sina_hip_rank_inplace_stats) on its contexts -- between runs
int sina_host_store_search_inplace_stats(const char *key, uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs,
                                         uint64_t *launches) {
    return guarded([&] {
        if (!trays || !kernel_ms || !sequences || !pairs || !launches) throw std::logic_error("store_search_inplace_stats: null argument");
        reference_store::get(key)->search_inplace_stats(trays, kernel_ms, sequences, pairs, launches);
    });
}
// the aligner's device-dist on this store: trays whose --show-dist counters came from the device, and the show-dist
// kernel's time and volume (sina_hip_show_dist_stats) on its contexts -- between runs
int sina_host_store_show_dist_stats(const char *key, uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs,
                                    uint64_t *launches) {
    return guarded([&] {
        if (!trays || !kernel_ms || !sequences || !pairs || !launches) throw std::logic_error("store_show_dist_stats: null argument");
        reference_store::get(key)->show_dist_stats(trays, kernel_ms, sequences, pairs, launches);
    });
}
// the aligner's device-copy on this store: (query, suspect) pairs the containment kernel answered, its time and launches
// (sina_hip_find_bases_stats) on the store's contexts, trays answered by the device and trays with suspects that kept
// the host walk -- between runs
int sina_host_store_copy_stats(const char *key, uint64_t *pairs, double *kernel_ms, uint64_t *launches, uint64_t *trays,
                               uint64_t *fallback_trays) {
    return guarded([&] {
        if (!pairs || !kernel_ms || !launches || !trays || !fallback_trays) throw std::logic_error("store_copy_stats: null argument");
        reference_store::get(key)->copy_stats(pairs, kernel_ms, launches, trays, fallback_trays);
    });
}
// famfinder's device-turn on this store: queries the orient and pick kernels took and those of them they turned, the
// kernels' time and launches (sina_hip_turn_stats) on the store's contexts; trays whose first round's rows came with
// the orientation, trays of which only the orientation was taken, and trays of batches that fell back to the host's
// searches -- between runs
int sina_host_store_turn_stats(const char *key, uint64_t *queries, uint64_t *turned, double *kernel_ms, uint64_t *launches,
                               uint64_t *rows_trays, uint64_t *orient_trays, uint64_t *fallback_trays) {
    return guarded([&] {
        if (!queries || !turned || !kernel_ms || !launches || !rows_trays || !orient_trays || !fallback_trays)
            throw std::logic_error("store_turn_stats: null argument");
        reference_store::get(key)->turn_stats(queries, turned, kernel_ms, launches, rows_trays, orient_trays, fallback_trays);
    });
}
// show_dist_report alone (no device), for tests: nq (orig, aligned) pairs as packed words of the store's width, their
// relatives as reference ids of the store; rows: null -- the host walk -- or [nq][20] counters to take instead
// (sina_hip_show_dist's rows).  out [nq][3]: sps, idty, cpm; flags [nq]: bit 0 has_sps, bit 1 has_closest; closest [nq];
// text (optional): the reports' lines, truncated at cap.
int sina_host_show_dist_reports(const char *key, const uint32_t *orig_ab, const uint64_t *orig_off, const uint32_t *al_ab,
                                const uint64_t *al_off, uint32_t nq, const uint32_t *ref_ids, const uint64_t *ref_off,
                                const uint32_t *rows, float *out, uint32_t *flags, uint32_t *closest, char *text, uint32_t cap) {
    return guarded([&] {
        if (!orig_ab || !orig_off || !al_ab || !al_off || !ref_off || !out || !flags || !closest)
            throw std::logic_error("show_dist_reports: null argument");
        const std::shared_ptr<reference_store> st = reference_store::get(key);
        std::string all;
        for (uint32_t q = 0; q < nq; q++) {
            cseq orig("orig"), aligned("aligned");
            orig.setAlignedBases(reinterpret_cast<const aligned_base *>(orig_ab + orig_off[q]), (size_t)(orig_off[q + 1] - orig_off[q]));
            aligned.setAlignedBases(reinterpret_cast<const aligned_base *>(al_ab + al_off[q]), (size_t)(al_off[q + 1] - al_off[q]));
            orig.setWidth(st->getAlignmentWidth());
            aligned.setWidth(st->getAlignmentWidth());
            search::result_vector ref;
            for (uint64_t i = ref_off[q]; i < ref_off[q + 1]; i++) {
                if (ref_ids[i] >= st->size()) throw std::logic_error("show_dist_reports: reference id out of range");
                ref.emplace_back(0.f, &st->getCseq(ref_ids[i]));
            }
            log_printer::report rep;
            show_dist_report(orig, aligned, ref, rows ? rows + 20 * (size_t)q : nullptr, rep);
            out[3 * (size_t)q] = rep.sps;
            out[3 * (size_t)q + 1] = rep.idty;
            out[3 * (size_t)q + 2] = rep.cpm;
            flags[q] = (rep.has_sps ? 1u : 0u) | (rep.has_closest ? 2u : 0u);
            closest[q] = rep.closest_seq ? st->id_of(rep.closest_seq) : rep.closest_id;
            all += rep.text;
        }
        if (text && cap) snprintf(text, cap, "%s", all.c_str());
    });
}
// the aligner's finish step on this store: trays the device had assembled / the host finished, and the device
// assembly's volume (sina_hip_assemble_stats) on its contexts -- between runs
int sina_host_store_assemble_stats(const char *key, uint64_t *trays_device, uint64_t *trays_host, uint64_t *queries, uint64_t *assembled,
                                   uint64_t *shifted_queries, uint64_t *shifted_runs) {
    return guarded([&] {
        if (!trays_device || !trays_host || !queries || !assembled || !shifted_queries || !shifted_runs)
            throw std::logic_error("store_assemble_stats: null argument");
        reference_store::get(key)->assemble_stats(trays_device, trays_host, queries, assembled, shifted_queries, shifted_runs);
    });
}
// The host walk (cseq_base::calcPairScore), no device involved, of an aligned string.  counts6 (optional): num, AG,
// AU, CG, GG, GU.
int sina_host_pair_score(const char *aligned_text, const uint32_t *pairs, uint32_t n, float *score, uint32_t *counts6) {
    return guarded([&] {
        if (!aligned_text || (!pairs && n) || !score) throw std::logic_error("pair_score: null argument");
        const cseq c("", aligned_text);
        *score = c.calcPairScore(std::vector<uint32_t>(pairs, pairs + n), counts6);
    });
}
// ... and of a batch of sequences as packed words, taken as they are (mask 0, equal or descending columns included; q_ab /
// q_off as sina_hip_pair_counts takes them), one after the other on the calling thread; counts6 (optional): [nq][6];
// seconds (optional): the walk's wall time, the map already in place (tools/perf_bps.py)
int sina_host_pair_scores_packed(const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, const uint32_t *pairs, uint32_t n,
                                 float *scores, uint32_t *counts6, double *seconds) {
    return guarded([&] {
        if (!q_ab || !q_off || (!pairs && n) || !scores) throw std::logic_error("pair_scores_packed: null argument");
        const std::vector<uint32_t> map(pairs, pairs + n);
        std::vector<cseq> seqs(nq);
        for (uint32_t q = 0; q < nq; q++)
            seqs[q].setAlignedBases(reinterpret_cast<const aligned_base *>(q_ab + q_off[q]), (size_t)(q_off[q + 1] - q_off[q]));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t q = 0; q < nq; q++) scores[q] = seqs[q].calcPairScore(map, counts6 ? counts6 + 6 * (size_t)q : nullptr);
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    });
}
// pair_score_from_counts and the attribute made of it, for tests
float sina_host_pair_score_from_counts(const uint32_t *counts6, int *attr) {
    const float s = pair_score_from_counts(counts6);
    if (attr) *attr = pair_score_attr(s);
    return s;
}
// Log::printer alone (no device): n aligned strings as trays seq0, seq1, ... through one log_printer, in order; the
// reports' text into out (truncated at cap), the run's avg_bps.  The helix map is the one of the aligner's "db".
int sina_host_log_reports(const char *const *aligned_texts, uint32_t n, char *out, uint32_t cap, double *avg_bps) {
    return guarded([&] {
        log_printer lp(false);
        std::ostringstream text;
        for (uint32_t i = 0; i < n; i++) {
            tray t;
            t.seqno = i;
            const std::string name = "seq" + std::to_string(i);
            t.input_sequence = new cseq(name.c_str(), aligned_texts[i]);
            t.aligned_sequence = new cseq(*t.input_sequence);
            t = lp(t, text);
            t.destroy();
        }
        if (out && cap) snprintf(out, cap, "%s", text.str().c_str());
        if (avg_bps) *avg_bps = lp.totals().avg_bps;
    });
}
int sina_host_store_build_index(const char *key, unsigned k, int nofast) {
    return guarded([&] {
        reference_store::get(key)->ensure_index(k, nofast != 0);
    });
}
// sina -i in.fasta -o out.fasta --db <key> [--search] [--show-dist]: FASTA reader -> famfinder -> aligner
// [-> search_filter] -> log printer -> FASTA writer, in batches of `batch` sequences.  The stage
// options are whatever sina_host_set_option set.  summary: n_read, n_aligned, n_written, n_skipped,
// then avg_sps, avg_cpm, avg_idty (as Log::printer prints them at exit).
//
// sina_host_run_fasta_serial: one batch at a time, stage after stage, tray after tray (rounds 1-3: parity runs).
// sina_host_run_fasta: the same stages as CONCURRENT nodes, as SINA's flow graph has them (src/sina.cpp:452-586:
// a serial source, the stages, serial ordered sinks): a reader thread cuts and parses the next batch while the
// batch before it is searched (famfinder thread) and the one before that aligned (aligner thread); the sink
// takes the batches in input order, renders the trays' log reports and composes their FASTA records on the loop
// pool, and only the hand-over of the finished text -- running totals, csv rows, the write itself -- stays
// serial.  Output, log and summary are byte for byte those of the serial driver.
namespace {
struct fasta_run {
    famfinder ff;
    aligner al;
    std::unique_ptr<search_filter> sf;
    std::unique_ptr<rw_fasta::reader> rd;
    std::unique_ptr<rw_fasta::writer> wr;
    std::unique_ptr<log_printer> lp;
    std::ofstream logf;
    std::ostringstream devnull;
    bool log_to_file = false;
    int n_read = 0, n_aligned = 0;
    std::ostream &log() { return log_to_file ? static_cast<std::ostream &>(logf) : devnull; }
    fasta_run(const char *in_path, const char *out_path, const char *log_path, int do_search, int show_dist) {
        famfinder::validate_options();
        aligner::validate_options();
        if (do_search) search_filter::validate_options();
        if (do_search) sf.reset(new search_filter());
        rd.reset(new rw_fasta::reader(in_path));
        wr.reset(new rw_fasta::writer(out_path));
        lp.reset(new log_printer(show_dist != 0));
        if (log_path && *log_path) {
            logf.open(log_path);
            log_to_file = logf.is_open();
        }
    }
    bool read_batch(std::vector<tray> &trays, uint32_t batch) {
        trays.clear();
        while (trays.size() < batch) {
            tray t;
            if (!(*rd)(t)) break;
            trays.push_back(t);
        }
        return !trays.empty();
    }
    void finish(double *summary7) {
        wr->flush();
        const log_printer::summary sm = lp->totals();
        summary7[0] = n_read;
        summary7[1] = n_aligned;
        summary7[2] = wr->written();
        summary7[3] = rd->skipped();
        summary7[4] = sm.avg_sps;
        summary7[5] = sm.avg_cpm;
        summary7[6] = sm.avg_idty;
        g_last_avg_bps.store(sm.avg_bps);
    }
};
}  // namespace

// One run of either kind.  The stages are the same four; what differs is how they are driven (staged: a thread
// each, so one batch is read while the one before it is searched and the one before that aligned; serial: batch
// after batch on this thread) and the sink: the staged one renders and composes on the loop pool and keeps only
// the hand-over serial, the serial one is SINA's node after node, which the tests compare the staged one with.
static int run_fasta(const char *in_path, const char *out_path, const char *log_path, int do_search, int show_dist,
                     uint32_t batch, double *summary7, bool staged) {
    return guarded([&] {
        fasta_run r(in_path, out_path, log_path, do_search, show_dist);
        const show_dist_scope dist_scope(show_dist != 0);  // (what show_dist_batch asks; the host option is the pipeline's)
        show_dist_prepare();
        if (batch == 0) batch = 1024;
        std::vector<log_printer::report> reports;
        auto sink_serial = [&](std::vector<tray> &trays) {
            for (auto &t : trays) {  // serial, in input order (Log::printer and the writer are serial nodes)
                if (t.aligned_sequence) r.n_aligned++;
                t = (*r.lp)(t, r.log());
                t = (*r.wr)(t);
                t.destroy();
                r.devnull.str("");
            }
        };
        auto sink_staged = [&](std::vector<tray> &trays) {
            reports.resize(trays.size());
            {
                host_phase hp("sink.report");  // (the log reports, --show-dist's walks among them: tools/perf_showdist.py)
                parallel_for(trays.size(), [&](size_t i) { r.lp->render(trays[i], reports[i]); });
            }
            r.wr->precompose(trays);  // (after render: the reports' attributes are part of the records' meta data)
            for (size_t i = 0; i < trays.size(); i++) {
                tray &t = trays[i];
                if (t.aligned_sequence) r.n_aligned++;
                r.lp->commit(reports[i], r.log());
                t = (*r.wr)(t);
                r.devnull.str("");
            }
            parallel_for(trays.size(), [&](size_t i) { trays[i].destroy(); });
        };
        // one thread per node and FIFO queues: the batches stay in input order
        flow::runner<std::vector<tray>> run(destroy_trays);
        run.source("reader", 1, [&](std::vector<tray> &trays) {
               if (!r.read_batch(trays, batch)) return false;
               r.n_read += (int)trays.size();
               return true;
           })
            .then(2, "famfinder", 1, [&](std::vector<tray> &trays) { r.ff(trays); })
            .then(2, "aligner", 1, [&](std::vector<tray> &trays) {
                r.al(trays);
                if (r.sf) (*r.sf)(trays);
                pair_score_batch(trays);
                show_dist_batch(trays);  // (nothing unless the run shows dist and the aligner's device-dist is on)
            });
        if (staged) {
            tune_allocator();
            reserve_workers([&] { return do_search ? reference_store::get(search_filter_database()) : nullptr; }, 1, 1);
            run.then(2, "sink", 1, sink_staged).staged();
        } else run.then(2, "sink", 1, sink_serial).inline_();
        r.finish(summary7);
    });
}

int sina_host_run_fasta_serial(const char *in_path, const char *out_path, const char *log_path, int do_search,
                               int show_dist, uint32_t batch, double *summary7) {
    return run_fasta(in_path, out_path, log_path, do_search, show_dist, batch, summary7, false);
}
int sina_host_run_fasta(const char *in_path, const char *out_path, const char *log_path, int do_search,
                        int show_dist, uint32_t batch, double *summary7) {
    return run_fasta(in_path, out_path, log_path, do_search, show_dist, batch, summary7, true);
}

// avg_bps of the last sina_host_run_fasta / _serial that finished: the sum of the aligned trays' base-pair scores, in
// tray order, over their number (Log::printer's avg_bps, src/log.cpp:358).  The summary array keeps its seven values.
double sina_host_last_avg_bps(void) { return g_last_avg_bps.load(); }

// FASTA reader + writer alone (no GPU): reads every sequence of in_path and writes it back, the
// input sequence standing in for the aligned one; returns the counts.  For CPU tests of the I/O rules.
int sina_host_fasta_roundtrip(const char *in_path, const char *out_path, int *n_read, int *n_skipped) {
    return guarded([&] {
        rw_fasta::reader rd(in_path);
        rw_fasta::writer wr(out_path);
        int n = 0;
        for (;;) {
            tray t;
            if (!rd(t)) break;
            n++;
            t.aligned_sequence = new cseq(*t.input_sequence);
            t = wr(t);
            t.destroy();
        }
        wr.flush();
        *n_read = n;
        *n_skipped = rd.skipped();
    });
}

// .sidx <-> CSR without a GPU (tests): load into caller buffers / store from caller arrays
int sina_host_sidx_load(const char *path, unsigned k, int nofast, uint32_t *n_sequences, uint32_t *offsets,
                        uint32_t *ids, uint64_t ids_cap, uint64_t *n_ids) {
    return guarded([&] {
        std::vector<std::string> names;
        std::vector<uint32_t> off, id;
        std::string why;
        if (!sidx_load(path, k, nofast != 0, &names, &off, &id, &why)) throw std::runtime_error("sidx_load: " + why);
        *n_sequences = (uint32_t)names.size();
        *n_ids = id.size();
        if (id.size() > ids_cap) throw std::runtime_error("sidx_load: ids buffer too small");
        memcpy(offsets, off.data(), 4 * off.size());
        if (!id.empty()) memcpy(ids, id.data(), 4 * id.size());
    });
}
int sina_host_sidx_store(const char *path, unsigned k, int nofast, uint32_t n_sequences, const uint32_t *offsets,
                         const uint32_t *ids, uint64_t n_ids) {
    return guarded([&] {
        std::vector<std::string> names;
        for (uint32_t i = 0; i < n_sequences; i++) names.push_back("ref" + std::to_string(i));
        sidx_store(path, k, nofast != 0, names, std::vector<uint32_t>(offsets, offsets + ((size_t)1 << (2 * k)) + 1),
                   std::vector<uint32_t>(ids, ids + n_ids));
    });
}
// opens an aligned-FASTA database by path (its index is cached in <path minus extension>.sidx)
int sina_host_store_open(const char *path, int device) {
    return guarded([&] {
        auto s = reference_store::get(path);
        s->set_device(device);
    });
}
// the same with the sequences numbered as the reference numbers an ARB database's (host/id_order.h)
int sina_host_store_open_arb_order(const char *path, int device) {
    return guarded([&] {
        auto s = reference_store::open(path, true);
        s->set_device(device);
    });
}
// order[i] = database position of the sequence the reference gives id i (query_arb.cpp:160,470-474,732-739);
// hashes[j] (optional) = boost::hash<std::string> of names[j]; returns the number of ids (distinct names)
uint32_t sina_host_reference_order(const char *const *names, uint32_t n, uint32_t *order, uint64_t *hashes,
                                   uint64_t *bucket_count) {
    std::vector<std::string> v(names, names + n);
    std::size_t buckets = 0;
    const std::vector<uint32_t> o = arb_name_order(v, &buckets);
    std::copy(o.begin(), o.end(), order);
    if (hashes)
        for (uint32_t i = 0; i < n; i++) hashes[i] = (uint64_t)arb_name_hash(v[i]);
    if (bucket_count) *bucket_count = buckets;
    return (uint32_t)o.size();
}
// name of reference `id` of a store (empty string: no such id)
const char *sina_host_store_name(const char *key, uint32_t id) {
    static thread_local std::string s;
    try {
        auto st = reference_store::get(key);
        s = id < st->size() ? st->getCseq(id).getName() : std::string();
    } catch (const std::exception &) {
        s.clear();
    }
    return s.c_str();
}
const char *sina_host_store_index_origin(const char *key) {
    static thread_local std::string s;
    try {
        s = reference_store::get(key)->index_origin();
    } catch (const std::exception &e) {
        fail(e);
        s.clear();
    }
    return s.c_str();
}
// After the index arrived by broadcast (sina_hip_store_alloc_like + RCCL): tell the store
// not to rebuild it.
int sina_host_store_index_ready(const char *key, unsigned k, int nofast) {
    return guarded([&] {
        reference_store::get(key)->adopt_index(k, nofast != 0);
    });
}

int sina_host_reset_options(void) {
    famfinder::reset_options();
    aligner::reset_options();
    search_filter::reset_options();
    rw_fasta::reset_options();
    set_show_dist(false);
    return 0;
}

// field of a reference sequence (stands in for the ARB database fields the search stage loads)
int sina_host_store_set_attr(const char *key, uint32_t id, const char *field, const char *value) {
    return guarded([&] {
        reference_store::get(key)->set_attr(id, field, value);
    });
}

int sina_host_set_option(const char *stage, const char *name, const char *value) {
    return guarded([&] {
        if (!strcmp(stage, "famfinder")) famfinder::set_option(name, value);
        else if (!strcmp(stage, "aligner")) aligner::set_option(name, value);
        else if (!strcmp(stage, "search")) search_filter::set_option(name, value);
        else if (!strcmp(stage, "fasta")) rw_fasta::set_option(name, value);
        else if (!strcmp(stage, "host") && !strcmp(name, "threads")) set_host_threads((unsigned)atoi(value));
        else if (!strcmp(stage, "host") && !strcmp(name, "dedup")) set_batch_dedup(atoi(value) != 0);
        else if (!strcmp(stage, "host") && !strcmp(name, "show-dist")) set_show_dist(atoi(value) != 0);
        else throw std::logic_error(std::string("unknown stage ") + stage);
    });
}

// The driver allocates and frees tens of MB of trays per batch: keep what the allocator got from the
// kernel (no trimming, no per-vector mmap) so that steady-state batches do not page-fault their
// memory in again.  Process-wide; a host that sets SINA_HIP_NO_RUNTIME_DEFAULTS (the library's "leave my process
// alone" switch, include/sina_hip.h) keeps its allocator settings too.
static void tune_allocator() {
    static const bool once = [] {
        const char *v = getenv("SINA_HIP_NO_RUNTIME_DEFAULTS");
        if (v && *v && !(v[0] == '0' && v[1] == 0)) return false;
        mallopt(M_TRIM_THRESHOLD, 1 << 30);
        mallopt(M_TOP_PAD, 64 << 20);
        mallopt(M_MMAP_THRESHOLD, 256 << 20);
        return true;
    }();
    (void)once;
}

void *sina_host_pipeline_create(void) {
    try {
        tune_allocator();
        famfinder::validate_options();
        aligner::validate_options();
        return new pipeline();
    } catch (const std::exception &e) {
        fail(e);
        return nullptr;
    }
}
// the same with the search stage behind the aligner (sina --search)
void *sina_host_pipeline_create_search(void) {
    try {
        tune_allocator();
        famfinder::validate_options();
        aligner::validate_options();
        search_filter::validate_options();
        std::unique_ptr<pipeline> p(new pipeline());
        p->sf.reset(new search_filter());
        p->search_store = reference_store::get(search_filter_database());
        return p.release();
    } catch (const std::exception &e) {
        fail(e);
        return nullptr;
    }
}
void sina_host_pipeline_destroy(void *p) { delete (pipeline *)p; }

// marks of the bench in the SINA_HOST_TRACE file: 0 = timed region starts, 1 = ends
void sina_host_profile_mark(int which) { host_profile_mark(which == 0 ? "MARK:timed-start" : "MARK:timed-end"); }
}  // extern "C"

// Feeds nq queries through famfinder -> aligner in batches of `batch`, with `inflight` batches being worked on
// concurrently (host stages of one batch overlap GPU work of another).  fill(tray, q): the source's part -- query q
// as the reader stage would hand it over.
template <class Fill>
static int run_queries(pipeline *p, uint32_t nq, const uint64_t *qoff, uint32_t batch, uint32_t inflight, Fill &&fill) {
    return guarded([&] {
        host_profile_mark("MARK:run-entered");
        show_dist_prepare();
        if (batch == 0) batch = nq ? nq : 1;
        if (p->chunk_q != batch) p->chunks.clear();  // (chunks follow the batch size)
        p->chunk_q = batch;
        p->n_results = nq;
        const size_t n_chunks = ((size_t)nq + batch - 1) / batch;
        if (p->chunks.size() < n_chunks) p->chunks.resize(n_chunks);
        // (a chunk keeps its records -- their heap blocks -- between runs, but not their meaning: only a chunk
        // the sink of THIS run has filled is served by result_at(); a batch that fails early leaves "not aligned")
        ++p->run_no;
        if (inflight == 0) inflight = 1;
        std::atomic<uint32_t> next{0};
        std::atomic<uint64_t> ff_ns{0}, al_ns{0}, sf_ns{0};
        const auto t0 = std::chrono::steady_clock::now();
        host_profile_mark("MARK:run-threads-start");
        // One batch travelling through the stages (what a tray is in SINA's TBB flow graph, times `batch`).
        struct item {
            uint32_t b0 = 0, b1 = 0;
            std::vector<tray> trays;
        };
        auto take = [&](item &it) -> bool {
            it.b0 = next.fetch_add(batch);
            if (it.b0 >= nq) return false;
            it.b1 = std::min(nq, it.b0 + batch);
            return true;
        };
        auto build_and_find = [&](item &it) {  // source + famfinder node
            it.trays = p->take_trays();
            it.trays.resize(it.b1 - it.b0);
            {
                host_phase hp("drv.build_trays");
                parallel_for(it.b1 - it.b0, [&](size_t i) {  // (what SINA's reader stage does per sequence)
                    fill(it.trays[i], it.b0 + (uint32_t)i);
                });
            }
            timed(ff_ns, [&] { p->ff(it.trays); });
        };
        auto align_and_search = [&](item &it) {  // aligner node (+ search node)
            timed(al_ns, [&] { p->al(it.trays); });
            if (p->sf) timed(sf_ns, [&] { (*p->sf)(it.trays); });
            pair_score_batch(it.trays);  // (nothing without a helix map)
            show_dist_batch(it.trays);   // (nothing without the host option show-dist and the aligner's device-dist)
        };
        auto extract = [&](item &it) {  // sink
            {
                host_phase hp("drv.extract");
                pipeline::result_chunk &chunk = p->chunks[it.b0 / batch];
                chunk.results.resize(it.b1 - it.b0);
                chunk.run = p->run_no;
                const reference_store::pair_map helix = aligner_pair_map();
                parallel_for(it.b1 - it.b0, [&](size_t i) {  // (what SINA's writer stage does per sequence)
                    const uint32_t q = it.b0 + (uint32_t)i;
                    extract_tray(p, it.trays[i], chunk.results[i], (uint32_t)(qoff[q + 1] - qoff[q]), helix);
                });
            }
            p->give_trays(std::move(it.trays));
        };
        // The stages as nodes with their own threads and bounded hand-over queues, as SINA wires them
        // (src/sina.cpp:452-586: source -> famfinder -> aligner -> search -> sink).  `inflight` aligner threads
        // keep the GPU's DP slot busy (graph build of one batch beside the DP of another); the famfinder threads
        // run ahead by at most `n_find` finished batches, so an aligner thread never waits for a k-mer search to
        // start.  inflight == 1: one batch at a time, stage after stage on this thread (kernel timings taken this
        // way are undisturbed).
        const uint32_t n_find = inflight >= 4 ? 3 : (inflight >= 3 ? 2 : 1), n_align = inflight;
        flow::runner<item> run([](item &it) { destroy_trays(it.trays); });
        run.source("finder", n_find, [&](item &it) {
               if (!take(it)) return false;
               build_and_find(it);
               return true;
           }, [] { host_profile_thread_exit("thread: finder (whole run)"); })
            .then(n_find, "aligner", n_align, align_and_search, [] { host_profile_thread_exit("thread: aligner (whole run)"); })
            .then(2, "sink", 1, extract, [] { host_profile_thread_exit("thread: sink (whole run)"); });
        std::exception_ptr err;
        try {
            if (inflight == 1) run.inline_();
            else {
                reserve_workers([&] { return p->sf ? p->search_store : nullptr; }, n_find, n_align);
                run.staged();
            }
        } catch (...) {
            err = std::current_exception();
        }
        p->wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        p->ff_s = ff_ns.load() * 1e-9;
        p->al_s = al_ns.load() * 1e-9;
        p->sf_s = sf_ns.load() * 1e-9;
        if (err) std::rethrow_exception(err);
    });
}

extern "C" {
// nq unaligned queries (iupac masks): base i in column i, named queryN
int sina_host_pipeline_run(void *pp, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq, uint32_t batch,
                           uint32_t inflight) {
    return run_queries((pipeline *)pp, nq, qoff, batch, inflight,
                       [&](tray &t, uint32_t q) { fill_query_tray(t, q, qmask, qoff); });
}

// The same run for ALIGNED queries under their own names: q_ab / q_off the packed aligned bases (column | mask << 24),
// names[q] the sequence's name.  What reaches --fs-msc-max and --fs-leave-query-out (a leave-out run: queries taken from
// the references themselves).  Results through sina_host_result(q) as ever.
int sina_host_pipeline_run_aligned(void *pp, const uint32_t *q_ab, const uint64_t *q_off, const char *const *names,
                                   uint32_t nq, uint32_t batch, uint32_t inflight) {
    pipeline *p = (pipeline *)pp;
    uint32_t width = 0;
    try {
        if (!q_ab || !q_off || !names) throw std::logic_error("pipeline_run_aligned: null argument");
        width = reference_store::get(aligner::opts->database)->getAlignmentWidth();
    } catch (const std::exception &e) {
        return fail(e);
    }
    return run_queries(p, nq, q_off, batch, inflight,
                       [&](tray &t, uint32_t q) { fill_aligned_query_tray(t, q, q_ab, q_off, names[q], width); });
}

// The boundary as INTEGRATION.md binds it (src/sina.cpp:497-519): `n_threads` callers -- TBB workers of
// unlimited-concurrency function_nodes in SINA -- each push ONE tray at a time through
// batched<famfinder> -> batched<aligner> (-> batched<search_filter> for a search pipeline), and the shim
// groups whoever is waiting into one GPU batch.  Results land where sina_host_pipeline_run puts them.
// poison_q >= 0: that query's family gets a member that is not of the store before the aligner sees it -- the
// device rejects the batch it travels in, the stage throws (std::runtime_error) and every
// caller of that batch gets the exception: failed[q] = 1 for those, the first message in err / err_cap.
int sina_host_pipeline_run_single_trays(void *pp, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq,
                                        uint32_t n_threads, uint32_t max_batch, uint32_t linger_us, int32_t poison_q,
                                        uint8_t *failed, char *err, uint32_t err_cap) {
    pipeline *p = (pipeline *)pp;
    try {
        if (n_threads == 0) n_threads = 1;
        ++p->run_no;
        p->chunk_q = nq ? nq : 1;
        p->n_results = nq;
        p->chunks.clear();
        p->chunks.resize(1);
        pipeline::result_chunk &chunk = p->chunks[0];
        chunk.results.resize(nq);
        chunk.run = p->run_no;
        if (failed) memset(failed, 0, nq);
        if (err && err_cap) err[0] = 0;
        batched<famfinder> bff(p->ff, max_batch, linger_us);
        aligner whole_log = p->al;  // (the callers of the shim read their trays' logs themselves)
        whole_log.defer_score_line = false;
        batched<aligner> bal(whole_log, max_batch, linger_us);
        std::unique_ptr<batched<search_filter>> bsf;
        if (p->sf) bsf.reset(new batched<search_filter>(*p->sf, max_batch, linger_us));
        // (a sequence of the store's width that is not one of the store's: what a stale tray would carry)
        cseq foreign("not-in-this-store");
        if (poison_q >= 0) {
            const auto store = reference_store::get(aligner::opts->database);
            foreign.append("ACGU");
            foreign.setWidth(store->getAlignmentWidth());
        }
        // (trays that come one at a time meet no pair step: their base-pair score is the host walk's, in the sink)
        const reference_store::pair_map helix = aligner_pair_map();
        std::atomic<uint32_t> next{0};
        std::mutex err_mu;
        std::exception_ptr fatal;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (uint32_t w = 0; w < n_threads; w++)
            th.emplace_back([&] {
                for (;;) {
                    const uint32_t q = next.fetch_add(1);
                    if (q >= nq) return;
                    try {
                        tray t;
                        fill_query_tray(t, q, qmask, qoff);
                        t = bff(std::move(t));
                        if ((int32_t)q == poison_q && t.alignment_reference && !t.alignment_reference->empty())
                            t.alignment_reference->back().sequence = &foreign;
                        tray keep = t;  // (the pointers: a stage that throws hands nothing back)
                        try {
                            t = bal(std::move(t));
                            if (bsf) t = (*bsf)(std::move(t));
                        } catch (const std::exception &e) {
                            if (failed) failed[q] = 1;
                            {
                                std::lock_guard<std::mutex> lk(err_mu);
                                if (err && err_cap && err[0] == 0) snprintf(err, err_cap, "%s", e.what());
                            }
                            keep.destroy();
                            continue;
                        }
                        extract_tray(p, t, chunk.results[q], (uint32_t)(qoff[q + 1] - qoff[q]), helix);
                    } catch (...) {
                        std::lock_guard<std::mutex> lk(err_mu);
                        if (!fatal) fatal = std::current_exception();
                        next.store(nq);
                        return;
                    }
                }
            });
        for (auto &t : th) t.join();
        p->wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (fatal) std::rethrow_exception(fatal);
        return 0;
    } catch (const std::exception &e) {
        return fail(e);
    }
}

namespace {
const result &result_at(void *pp, uint32_t q) {
    static const result none;  // (out of range, or a batch that never reached the sink: "not aligned")
    pipeline *p = (pipeline *)pp;
    if (q >= p->n_results) return none;
    const auto &chunk = p->chunks[q / p->chunk_q];
    if (chunk.run != p->run_no) return none;
    return (q % p->chunk_q) < chunk.results.size() ? chunk.results[q % p->chunk_q] : none;
}
}  // namespace

int sina_host_result(void *pp, uint32_t q, int *status, int *head, int *tail, int *qual, uint32_t *width,
                     uint32_t *n_bases) {
    pipeline *p = (pipeline *)pp;
    if (q >= p->n_results) return 1;
    const result &r = result_at(pp, q);
    *status = r.status;
    *head = r.head;
    *tail = r.tail;
    *qual = r.qual;
    *width = r.width;
    *n_bases = r.n_ab;
    return 0;
}
const uint32_t *sina_host_result_bases(void *pp, uint32_t q) {
    return reinterpret_cast<const uint32_t *>(result_at(pp, q).ab);
}
const char *sina_host_result_log(void *pp, uint32_t q) {
    const result &r = result_at(pp, q);
    if (r.note.set) {  // (rendered once, in place)
        r.note.merge_into(r.log);
        r.note.set = false;
    }
    return r.log.c_str();
}
const char *sina_host_result_family(void *pp, uint32_t q) {
    const result &r = result_at(pp, q);
    if (r.family_render && r.family.empty()) r.family_render(r.family_owner, r.family_items.data(), r.family_items.size(), r.family);
    return r.family.c_str();
}
// search stage: number of results (-1: stage did not run for this query), ids/scores best first,
// string attributes it set on the sequence (nearest_slv, lca_<field>, copy_<acc>_<field>; "" if absent) -- and the
// aligner's align_filter_slv
int sina_host_result_search(void *pp, uint32_t q, uint32_t *ids, float *scores, uint32_t cap) {
    const result &r = result_at(pp, q);
    if (!r.searched) return -1;
    for (size_t i = 0; i < r.sr_ids.size() && i < cap; i++) {
        ids[i] = r.sr_ids[i];
        scores[i] = r.sr_scores[i];
    }
    return (int)r.sr_ids.size();
}
const char *sina_host_result_attr(void *pp, uint32_t q, const char *name) {
    const result &r = result_at(pp, q);
    const std::string *v = r.attrs.find(name);
    return v ? v->c_str() : "";
}
// --show-dist of query q (host option show-dist, sina_host_pipeline_run_aligned): out = sps, idty, cpm, closest = the
// closest relative's reference id; have = 0 where the report has no closest relative (no alignment, no relatives, widths
// that differ) or the run had no alignment to compare with
int sina_host_result_dist(void *pp, uint32_t q, float out[3], uint32_t *closest, int *have) {
    pipeline *p = (pipeline *)pp;
    if (q >= p->n_results || !out || !closest || !have) return 1;
    const result &r = result_at(pp, q);
    memcpy(out, r.dist, sizeof r.dist);
    *closest = r.dist_closest;
    *have = r.have_dist ? 1 : 0;
    return 0;
}
double sina_host_search_seconds(void *pp) { return ((pipeline *)pp)->sf_s; }
float sina_host_result_idty(void *pp, uint32_t q) { return result_at(pp, q).idty; }
// the helix base-pair score of query q and align_bp_score_slv made of it; 0 and 0 without a helix map or an alignment
int sina_host_result_bps(void *pp, uint32_t q, float *score, int *attr) {
    pipeline *p = (pipeline *)pp;
    if (q >= p->n_results) return 1;
    const result &r = result_at(pp, q);
    if (score) *score = r.bps;
    if (attr) *attr = pair_score_attr(r.bps);
    return 0;
}
void sina_host_timings(void *pp, double *wall_s, double *famfinder_s, double *aligner_s) {
    pipeline *p = (pipeline *)pp;
    *wall_s = p->wall_s;
    *famfinder_s = p->ff_s;
    *aligner_s = p->al_s;
}

// per-phase host timings (SINA_HOST_PROFILE=1); returned string is valid until the next call
const char *sina_host_profile(int reset) {
    static thread_local std::string s;
    s = host_profile_dump(reset != 0);
    return s.c_str();
}

// host DAG build exposed for tests (compares with the oracle's mseq)
int sina_host_build_graph(const char *key, const uint32_t *ids, uint32_t F, float fs_weight, uint32_t *n_nodes,
                          uint32_t *n_edges, uint32_t *pos, uint8_t *mask, float *weight, uint32_t *pred_off,
                          uint32_t *pred, uint32_t *succ_minpos, uint32_t cap_nodes, uint32_t cap_edges) {
    return guarded([&] {
        auto st = reference_store::get(key);
        std::vector<const cseq *> fam;
        for (uint32_t i = 0; i < F; i++) fam.push_back(&st->getCseq(ids[i]));
        host_graph g;
        build_family_graph(fam, fs_weight, &g);
        *n_nodes = (uint32_t)g.pos.size();
        *n_edges = (uint32_t)g.pred.size();
        if (g.pos.size() > cap_nodes || g.pred.size() > cap_edges) throw std::runtime_error("graph buffers too small");
        std::copy(g.pos.begin(), g.pos.end(), pos);
        std::copy(g.mask.begin(), g.mask.end(), mask);
        std::copy(g.weight.begin(), g.weight.end(), weight);
        std::copy(g.pred_off.begin(), g.pred_off.end(), pred_off);
        std::copy(g.pred.begin(), g.pred.end(), pred);
        std::copy(g.succ_minpos.begin(), g.succ_minpos.end(), succ_minpos);
    });
}

// the family as a profile (--fs-no-graph): columns and the match-term table the aligner hands to the device
// (build_family_profile, stages.cpp) -- for CPU-only tests against the oracle's pseq restatement
int sina_host_build_profile(const char *key, const uint32_t *ids, uint32_t F, float match, float mismatch, float gap,
                            float gap_ext, uint32_t *n_nodes, uint32_t *pos, float *score16, float *self16,
                            uint32_t cap_nodes) {
    return guarded([&] {
        auto st = reference_store::get(key);
        std::vector<const cseq *> fam;
        for (uint32_t i = 0; i < F; i++) fam.push_back(&st->getCseq(ids[i]));
        host_graph g;
        build_family_profile(fam, match, mismatch, gap, gap_ext, &g);
        *n_nodes = (uint32_t)g.pos.size();
        if (g.pos.size() > cap_nodes) throw std::runtime_error("profile buffers too small");
        std::copy(g.pos.begin(), g.pos.end(), pos);
        std::copy(g.score16.begin(), g.score16.end(), score16);
        profile_self_scores(match, mismatch, gap, gap_ext, self16);
    });
}

// cseq_comparator on two aligned strings, for CPU-only tests against the reference's KAT table
// (src/unit_tests/cseq_comparator_test.cpp); also returns the six counters
int sina_host_compare(const char *a_aligned, const char *b_aligned, int iupac, int dist, int cover, int filter_lc,
                      float *score, int32_t *counts6) {
    return guarded([&] {
        cseq a("", a_aligned), b("", b_aligned);
        cseq_comparator cmp((CMP_IUPAC_TYPE)iupac, (CMP_DIST_TYPE)dist, (CMP_COVER_TYPE)cover, filter_lc != 0);
        sina_hip_match_counts m;
        cseq_comparator::counts(a, b, (CMP_IUPAC_TYPE)iupac, filter_lc != 0, &m);
        *score = cmp.score(m);
        const int32_t v[6] = {m.only_a_overhang, m.only_b_overhang, m.only_a, m.only_b, m.match, m.mismatch};
        memcpy(counts6, v, sizeof v);
    });
}

// Self-checks of the host containers' round-6 machinery, for the CPU suite (no GPU, no store): a "dense" sequence
// (mask bytes only) against the same sequence built base by base, under every operation that must make its packed
// words first; a lazily rendered attribute against the eagerly set one, through copies; base lists out of the block
// pool across threads.  Returns 0, or 1 with the first failed check in err.
int sina_host_selftest(char *err, uint32_t err_cap) {
    auto fail = [&](const char *what) {
        if (err && err_cap) snprintf(err, err_cap, "%s", what);
        return 1;
    };
    try {
        // ---- dense == packed
        const char *bases = "ACGUNRYacguKMSWBDHV";
        const size_t n = strlen(bases);
        std::vector<uint8_t> masks;
        cseq eager("x");
        for (size_t i = 0; i < n; i++) {
            masks.push_back(base_iupac::from_char((unsigned char)bases[i]));
            eager.append(aligned_base((uint32_t)i, (unsigned char)bases[i]));
        }
        eager.setWidth((uint32_t)n);
        auto fresh = [&] {
            cseq d("x");
            d.setDenseMasks(masks.data(), masks.size());
            return d;
        };
        {
            cseq d = fresh();
            if (d.size() != n || d.getWidth() != n || d.denseMasks() == nullptr) return fail("dense: size / width / masks");
            if (d.getBases() != eager.getBases()) return fail("dense: getBases");
            if (d.denseMasks() == nullptr) return fail("dense: getBases must not drop the masks");
            if (!(d == eager)) return fail("dense: operator==");
            if (memcmp(d.packed(), eager.packed(), 4 * n) != 0) return fail("dense: packed words");
            if (d.denseMasks() == nullptr) return fail("dense: a const read must keep the masks");
            if (d.getAligned() != eager.getAligned()) return fail("dense: getAligned");
        }
        for (int op = 0; op < 5; op++) {
            cseq d = fresh(), e = eager;
            switch (op) {
            case 0: d.setWidth(40), e.setWidth(40); break;
            case 1: d.reverse(), e.reverse(); break;
            case 2: d.complement(), e.complement(); break;
            case 3: d.upperCaseAll(), e.upperCaseAll(); break;
            default: d.append(aligned_base(30, 'A')), e.append(aligned_base(30, 'A')); break;
            }
            if (!(d == e) || d.getWidth() != e.getWidth()) return fail("dense: a changing operation differs from the packed sequence");
            if (op >= 1 && d.denseMasks() != nullptr) return fail("dense: a changed sequence still offers its old masks");
            if (op == 0 && d.denseMasks() == nullptr) return fail("dense: a wider alignment must keep the masks");
        }
        {
            cseq d = fresh(), copy(d);
            copy.complement();
            if (!(d == eager)) return fail("dense: a copy's change reached the original");
            d.clearSequence();
            if (d.size() != 0 || d.denseMasks() != nullptr) return fail("dense: clearSequence");
        }
        // ---- lazy attribute == eager attribute
        {
            auto render = [](const void *owner, const uint64_t *items, size_t cnt, std::string &out) {
                out = *static_cast<const std::string *>(owner);
                for (size_t i = 0; i < cnt; i++) out += std::to_string(items[i]) + " ";
            };
            const std::string prefix = "p:";
            cseq c("y");
            c.set_attr("aaa", 1);
            std::vector<uint64_t> &it = c.set_lazy_attr(fn::family, &prefix, +render);
            it = {3, 1, 4};
            c.set_attr("zzz", std::string("z"));
            if (c.lazy_attr(fn::family) == nullptr) return fail("lazy: not pending after set");
            cseq copy;
            copy.copy_meta(c);
            const cseq::attr_init extra[1] = {cseq::attr_init::of(cseq::attr_key(fn::qual), 77)};
            cseq merged;
            merged.copy_meta_with(c, extra, 1);
            if (copy.lazy_attr(fn::family) == nullptr || merged.lazy_attr(fn::family) == nullptr) return fail("lazy: not carried by copy_meta");
            if (c.get_attr<std::string>(fn::family) != "p:3 1 4 ") return fail("lazy: rendered text");
            if (c.lazy_attr(fn::family) != nullptr) return fail("lazy: still pending after a read");
            if (copy.get_attr<std::string>(fn::family) != "p:3 1 4 " || merged.get_attr<std::string>(fn::family) != "p:3 1 4 ")
                return fail("lazy: a copy renders differently");
            if (merged.get_attr<int>(fn::qual) != 77 || merged.get_attr<int>("aaa") != 1 || merged.get_attr<std::string>("zzz") != "z")
                return fail("copy_meta_with: merged attributes");
            std::string keys;
            for (const auto &a : merged.get_attrs()) keys += a.key() + ",";
            if (keys != std::string("aaa,") + fn::family + "," + fn::qual + ",zzz,") return fail("copy_meta_with: key order");
            c.set_attr(fn::family, std::string("plain"));
            if (c.get_attr<std::string>(fn::family) != "plain") return fail("lazy: overwritten by set_attr");
        }
        // ---- find_bases == std::string::find
        {
            uint64_t x = 88172645463325252ull;
            auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
            for (int round = 0; round < 4000; round++) {
                const size_t h = 1 + rnd() % 200, n = 1 + rnd() % 40;
                std::string hay(h, 'A'), needle;
                for (auto &ch : hay) ch = "ACGU"[rnd() % (round % 3 ? 4 : 2)];
                if (rnd() % 3 && n <= h) needle = hay.substr(rnd() % (h - n + 1), n);  // (present: anywhere, the very end included)
                else { needle.assign(n, 'A'); for (auto &ch : needle) ch = "ACGU"[rnd() % 4]; }
                if (round % 7 == 0 && n <= h) needle = hay.substr(h - n, n);
                const size_t want = hay.find(needle);
                if (find_bases(hay, needle, 0) != want || find_bases(hay, needle, 1) != want) return fail("find_bases differs from std::string::find");
            }
        }
        // ---- the block pool across threads
        {
            std::atomic<int> bad{0};
            std::vector<base_vector> handed(64);
            std::vector<std::thread> th;
            for (int t = 0; t < 4; t++)
                th.emplace_back([&, t] {
                    for (int round = 0; round < 200; round++)
                        for (int i = t; i < 64; i += 4) {
                            base_vector v;
                            v.resize((size_t)(500 + 37 * i + round));
                            for (size_t k = 0; k < v.size(); k++) v[k] = aligned_base::from_raw((uint32_t)(k * 2654435761u + (uint32_t)i));
                            handed[i].swap(v);  // (the old block is freed by this thread, the new one possibly by another)
                        }
                });
            for (auto &x : th) x.join();
            for (int i = 0; i < 64; i++)
                for (size_t k = 0; k < handed[i].size(); k++)
                    if (handed[i][k].raw != (uint32_t)(k * 2654435761u + (uint32_t)i)) bad++;
            if (bad.load()) return fail("block pool: a block was handed out twice");
        }
        return 0;
    } catch (const std::exception &e) {
        if (err && err_cap) snprintf(err, err_cap, "exception: %s", e.what());
        return 1;
    }
}

// cseq container ops exposed for CPU-only tests against the reference's cseq_test KATs.
// op: 0 none, 1 setWidth(arg), 2 reverse, 3 complement, 4 upperCaseAll
// what: 0 getAligned(nodots), 1 getAligned(dots), 2 getAligned(nodots, dna), 3 getBases
int sina_host_cseq_op(const char *aligned, int op, uint32_t arg, int what, char *out, uint32_t cap,
                      uint32_t *size, uint32_t *width) {
    try {
        cseq c("", aligned);
        switch (op) {
        case 1: c.setWidth(arg); break;
        case 2: c.reverse(); break;
        case 3: c.complement(); break;
        case 4: c.upperCaseAll(); break;
        default: break;
        }
        std::string s;
        switch (what) {
        case 0: s = c.getAligned(true, false); break;
        case 1: s = c.getAligned(false, false); break;
        case 2: s = c.getAligned(true, true); break;
        default: s = c.getBases(); break;
        }
        if (s.size() + 1 > cap) throw std::runtime_error("buffer too small");
        memcpy(out, s.c_str(), s.size() + 1);
        *size = c.size();
        *width = c.getWidth();
        return 0;
    } catch (const base_iupac::bad_character_exception &e) {
        g_err = e.what();
        return 3;
    } catch (const std::runtime_error &e) {
        g_err = e.what();
        return 2;
    } catch (const std::exception &e) {
        return fail(e);
    }
}

// The aligner's exact-relative walk on one pair, for CPU-only tests of its device twin (sina_hip_find_bases): the two
// sequences as packed words, rendered by the container (getBases) and upper-cased as prepare_tray does; hay_text /
// needle_text (optional, cap bytes each): the strings; at: find_bases' answer, 0xFFFFFFFF for npos.
int sina_host_find_bases_packed(const uint32_t *hay, uint32_t n_hay, const uint32_t *needle, uint32_t n_needle, uint32_t *at,
                                char *hay_text, char *needle_text, uint32_t cap) {
    return guarded([&] {
        if ((!hay && n_hay) || (!needle && n_needle) || !at) throw std::logic_error("find_bases_packed: null argument");
        auto rendered = [](const uint32_t *ab, uint32_t n) {
            cseq c("");
            c.setAlignedBases(reinterpret_cast<const aligned_base *>(ab), n);
            std::string s = c.getBases();
            for (auto &ch : s) ch = (char)toupper((unsigned char)ch);
            return s;
        };
        const std::string h = rendered(hay, n_hay), nd = rendered(needle, n_needle);
        const size_t pos = find_bases(h, nd);
        *at = pos == std::string::npos ? 0xFFFFFFFFu : (uint32_t)pos;
        if (hay_text && cap) snprintf(hay_text, cap, "%s", h.c_str());
        if (needle_text && cap) snprintf(needle_text, cap, "%s", nd.c_str());
    });
}

// NAST fix-up exposed for CPU-only property tests against the oracle
int sina_host_fix_duplicates(uint32_t *ab, uint32_t n, uint32_t width, int lowercase, int remove, char *log,
                             uint32_t log_cap) {
    try {
        cseq c("");
        base_vector v;
        for (uint32_t i = 0; i < n; i++) v.push_back(aligned_base::from_raw(ab[i]));
        c.setAlignedBases(v);
        c.setWidth(width);
        std::stringstream ss;
        int rc = 0;
        try {
            c.fix_duplicate_positions(ss, lowercase != 0, remove != 0);
        } catch (const std::runtime_error &) {
            rc = 2;  // "no space to left and right"
        }
        memcpy(ab, c.packed(), 4 * (size_t)n);
        const std::string s = ss.str();
        if (log && log_cap) {
            strncpy(log, s.c_str(), log_cap - 1);
            log[log_cap - 1] = 0;
        }
        return rc;
    } catch (const std::exception &e) {
        return fail(e);
    }
}

}  // extern "C"
