// Host side of the boundary: tray, reference_store, kmer_search.
// Behaviour follows the reference stage by stage (citations inline); the heavy
// lifting goes through the C ABI (include/sina_hip.h).  No CPU fallback: if the
// HIP library reports an error, the stage throws.
#include "stages_internal.h"
#include <charconv>
#include <sys/stat.h>
#include "id_order.h"
#include "../kmer_plan.h"
#include "../match_plan.h"
#include "../turn_plan.h"

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <fstream>
#include <map>
#include <tuple>
#include <unordered_map>

// (two fill constructors the library has always exported out of line: its exported names stay as they were whatever
// the compiler now inlines)
template std::vector<uint32_t>::vector(size_type, const uint32_t &, const std::allocator<uint32_t> &);
template std::vector<uint64_t>::vector(size_type, const uint64_t &, const std::allocator<uint64_t> &);
// (likewise, since the stages are a translation unit each: inline and template code that one large unit left out of
// line -- and so among the exported names, as weak symbols -- is inlined by the smaller ones)
template void sina::object_cache<sina::search::result_vector, sina::cache_any>::give(sina::search::result_vector *);
template std::string sina::annotated_cseq::get_attr<std::string>(std::string_view, std::string) const;
template void std::vector<sina::search::result_item>::reserve(size_type);
template void std::vector<sina::search::result_item>::_M_realloc_insert<float &, const sina::cseq *>(iterator, float &, const sina::cseq *&&);
template void std::vector<const sina::alignment_stats *>::_M_realloc_insert<const sina::alignment_stats *const &>(iterator, const sina::alignment_stats *const &);
template std::vector<std::vector<uint16_t>>::~vector();
template void std::vector<float>::resize(size_type);
template void std::vector<uint32_t>::resize(size_type);
template void std::string::swap(std::string &);
template unsigned long __gnu_cxx::__stoa<unsigned long, unsigned long, char, int>(unsigned long (*)(const char *, char **, int), const char *,
                                                                                  const char *, std::size_t *, int);
namespace {
using profile_row = std::pair<std::string, std::pair<double, unsigned long long>>;  // (host_profile_dump sorts them)
using profile_row_at = std::vector<profile_row>::iterator;
}  // namespace
template void std::iter_swap<profile_row_at, profile_row_at>(profile_row_at, profile_row_at);
template std::common_comparison_category_t<std::__detail::__synth3way_t<std::string>, std::__detail::__synth3way_t<std::pair<double, unsigned long long>>>
std::operator<=>(const profile_row &, const profile_row &);

namespace sina {

// ================================================================ tray (src/tray.cpp)

tray::tray(const tray &o)
    : seqno(o.seqno), input_sequence(o.input_sequence), aligned_sequence(o.aligned_sequence),
      alignment_reference(o.alignment_reference), search_result(o.search_result), astats(o.astats),
      family_scores_kmer_k(o.family_scores_kmer_k), query_kmer_count(o.query_kmer_count), bp_score(o.bp_score),
      bp_score_set(o.bp_score_set), search_row(o.search_row), dist_row(o.dist_row), dist_row_set(o.dist_row_set) {
    log.str(o.log.str());
    log.seekp(0, std::ios_base::end);
    pending_score = o.pending_score;
}
// (the stream's default float format is printf's %g = to_chars(general, 6) -- checked on 2e7 floats)
size_t tray::score_note::render(char *line, size_t cap) const {
    char *w = line, *const end = line + cap;
    auto lit = [&](const char *txt) {
        const size_t n = std::min(strlen(txt), (size_t)(end - w));  // (the line is 130 characters at most)
        memcpy(w, txt, n);
        w += n;
    };
    auto flt = [&](float v) { w = std::to_chars(w, end, v, std::chars_format::general, 6).ptr; };
    lit("scoring: raw=");
    flt(raw);
    lit(", weight=");
    flt(weight);
    lit(", query-len=");
    w = std::to_chars(w, end, len).ptr;
    lit(", aligned-bases=");
    w = std::to_chars(w, end, aligned).ptr;
    lit(", score=");
    flt(score);
    lit("; ");
    return (size_t)(w - line);
}
void tray::score_note::merge_into(std::string &text) const {
    if (!set) return;
    char line[192];
    const size_t n = render(line, sizeof line);
    text.insert(std::min<size_t>(at, text.size()), line, n);
}
std::string tray::log_text() const {
    std::string s(log.view());
    pending_score.merge_into(s);
    return s;
}
tray &tray::operator=(const tray &o) {
    seqno = o.seqno;
    input_sequence = o.input_sequence;
    aligned_sequence = o.aligned_sequence;
    alignment_reference = o.alignment_reference;
    search_result = o.search_result;
    log.str(o.log.str());
    log.seekp(0, std::ios_base::end);
    pending_score = o.pending_score;
    astats = o.astats;
    family_scores_kmer_k = o.family_scores_kmer_k;
    query_kmer_count = o.query_kmer_count;
    bp_score = o.bp_score;
    bp_score_set = o.bp_score_set;
    search_row = o.search_row;
    dist_row = o.dist_row;
    dist_row_set = o.dist_row_set;
    return *this;
}
alignment_stats *alignment_stats::shared_default() {
    static alignment_stats none;
    return &none;
}
void tray::destroy() {  // (src/tray.cpp:77-86; the objects go back to their caches, see object_cache)
    object_cache<cseq, cache_query_seq>::give(input_sequence);
    object_cache<cseq, cache_aligned_seq>::give(aligned_sequence);
    object_cache<search::result_vector>::give(alignment_reference);
    object_cache<search::result_vector>::give(search_result);
    // (astats is the store's or the shared default: not the tray's to delete, stages.h)
    input_sequence = aligned_sequence = nullptr;
    alignment_reference = search_result = nullptr;
    astats = nullptr;
    bp_score = 0.f;
    bp_score_set = false;
    search_row.reset();
    dist_row_set = false;
}

// ================================================================ reference_store

namespace {
std::mutex stores_mu;
std::map<std::string, std::shared_ptr<reference_store>> stores;
}  // namespace

std::shared_ptr<reference_store> reference_store::get(const std::string &path) {
    {
        std::lock_guard<std::mutex> lk(stores_mu);
        auto it = stores.find(path);
        if (it != stores.end()) return it->second;
    }
    return open(path);
}
std::shared_ptr<reference_store> reference_store::find(const std::string &path) {
    std::lock_guard<std::mutex> lk(stores_mu);
    auto it = stores.find(path);
    return it != stores.end() ? it->second : nullptr;
}
void reference_store::close(const std::string &path) {
    std::lock_guard<std::mutex> lk(stores_mu);
    stores.erase(path);
}

std::shared_ptr<reference_store> reference_store::from_packed(const std::string &key, const uint32_t *ab,
                                                              const uint64_t *off, uint32_t n, uint32_t width,
                                                              const char *const *names) {
    std::shared_ptr<reference_store> s(new reference_store());
    s->path = key;
    s->width = width;
    s->seqs.reserve(n);
    base_vector tmp;
    for (uint32_t i = 0; i < n; i++) {
        std::string nm = names ? std::string(names[i]) : ("ref" + std::to_string(i));
        s->seqs.emplace_back(nm.c_str());
        cseq &c = s->seqs.back();
        tmp.clear();
        for (uint64_t x = off[i]; x < off[i + 1]; x++) tmp.push_back(aligned_base::from_raw(ab[x]));
        c.setAlignedBases(tmp);
        c.setWidth(width);
        c.set_attr(fn::acc, nm);
    }
    s->fill_metas();
    std::lock_guard<std::mutex> lk(stores_mu);
    stores[key] = s;
    return s;
}
void reference_store::fill_metas() {
    metas.resize(seqs.size());
    for (size_t i = 0; i < seqs.size(); i++) {
        const cseq &c = seqs[i];
        metas[i] = ref_meta{(uint32_t)c.size(), c.size() ? c.getById(0).getPosition() : 0u,
                            c.size() ? c.getById(c.size() - 1).getPosition() : 0u};
    }
}

// Minimal aligned-FASTA reader ('>' name [description], sequence lines; '-'/'.' are gaps).
std::shared_ptr<reference_store> reference_store::open(const std::string &path, bool arb_id_order) {
    std::ifstream in(path);
    if (!in) throw std::logic_error("Reference database file " + path + " does not exist");
    std::shared_ptr<reference_store> s(new reference_store());
    s->path = path;
    std::string line, name, data;
    auto flush = [&]() {
        if (name.empty()) return;
        s->seqs.emplace_back(name.c_str(), data.c_str());
        s->seqs.back().set_attr(fn::acc, name);
        data.clear();
    };
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') {
            flush();
            size_t e = line.find_first_of(" \t", 1);
            name = line.substr(1, e == std::string::npos ? std::string::npos : e - 1);
        } else {
            data += line;
        }
    }
    flush();
    if (arb_id_order) {
        std::vector<std::string> names;
        names.reserve(s->seqs.size());
        for (const auto &c : s->seqs) names.push_back(c.getName());
        const std::vector<uint32_t> order = arb_name_order(names);
        std::vector<cseq> sorted;
        sorted.reserve(order.size());
        for (uint32_t from : order) sorted.push_back(std::move(s->seqs[from]));
        s->seqs.swap(sorted);
    }
    for (const auto &c : s->seqs) s->width = std::max(s->width, c.getWidth());
    for (auto &c : s->seqs) c.setWidth(s->width);
    s->fill_metas();
    std::lock_guard<std::mutex> lk(stores_mu);
    stores[path] = s;
    return s;
}

reference_store::~reference_store() {
    for (auto &pool : idle_forks)
        for (auto *f : pool) sina_hip_destroy(f);
    if (ctx) sina_hip_destroy(ctx);
}

reference_store::lease reference_store::worker_device(device_role role) {
    sina_hip_ctx *root = device();
    std::lock_guard<std::mutex> lk(gpu_mu);
    sina_hip_ctx *c = nullptr;
    auto &pool = idle_forks[role];
    if (!pool.empty()) {
        c = pool.front();  // (round robin: every context of the kind sees batches -- and grows -- early)
        pool.erase(pool.begin());
    } else {
        hip_check(sina_hip_fork(root, &c), "sina_hip_fork");
    }
    return lease(this, c, role);
}
void reference_store::reserve_workers(device_role role, unsigned n) {
    sina_hip_ctx *root = device();
    std::lock_guard<std::mutex> lk(gpu_mu);
    auto &pool = idle_forks[role];
    while (pool.size() < n) {
        sina_hip_ctx *c = nullptr;
        hip_check(sina_hip_fork(root, &c), "sina_hip_fork");
        pool.push_back(c);
    }
    for (sina_hip_ctx *c : pool) hip_check(sina_hip_prewarm(c, (int)role), "sina_hip_prewarm");
}
// (device() first: it takes gpu_mu itself)
template <class F>
void reference_store::for_each_context(F &&f) {
    sina_hip_ctx *root = device();
    std::lock_guard<std::mutex> lk(gpu_mu);
    f(root);
    for (auto &pool : idle_forks)
        for (sina_hip_ctx *c : pool) f(c);
}
template <class Get>
void reference_store::sum_kernel_use(const char *what, Get &&get, double *kernel_ms, uint64_t *a, uint64_t *b, uint64_t *launches) {
    *kernel_ms = 0;
    *a = *b = *launches = 0;
    for_each_context([&](sina_hip_ctx *c) {
        double ms = 0;
        uint64_t ca = 0, cb = 0, l = 0;
        hip_check(get(c, &ms, &ca, &cb, &l), what);
        *kernel_ms += ms;
        *a += ca;
        *b += cb;
        *launches += l;
    });
}
void reference_store::slow_path_queries(uint64_t *wide, uint64_t *long_kmer) {
    *wide = *long_kmer = 0;
    for_each_context([&](sina_hip_ctx *c) {
        uint64_t w = 0, l = 0;
        hip_check(sina_hip_wide_queries(c, &w), "sina_hip_wide_queries");
        hip_check(sina_hip_long_queries(c, &l), "sina_hip_long_queries");
        *wide += w;
        *long_kmer += l;
    });
}
void reference_store::big_select_queries(uint64_t *n) {
    *n = 0;
    for_each_context([&](sina_hip_ctx *c) {
        uint64_t b = 0;
        hip_check(sina_hip_big_select_queries(c, &b), "sina_hip_big_select_queries");
        *n += b;
    });
}
void reference_store::match_stats(double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches) {
    sum_kernel_use("sina_hip_match_stats", sina_hip_match_stats, kernel_ms, pairs, cand_bases, launches);
}
void reference_store::family_stats(double *kernel_ms, uint64_t *queries, uint64_t *candidates_listed, uint64_t *candidates_scanned,
                                   uint64_t *launches) {
    *kernel_ms = 0;
    *queries = *candidates_listed = *candidates_scanned = *launches = 0;
    for_each_context([&](sina_hip_ctx *c) {
        double ms = 0;
        uint64_t q = 0, listed = 0, scanned = 0, l = 0;
        hip_check(sina_hip_family_stats(c, &ms, &q, &listed, &scanned, &l), "sina_hip_family_stats");
        *kernel_ms += ms;
        *queries += q;
        *candidates_listed += listed;
        *candidates_scanned += scanned;
        *launches += l;
    });
}
const std::vector<uint32_t> &reference_store::ids_of_name(const std::string &name) {
    static const std::vector<uint32_t> none;
    std::call_once(name_ids_once, [this] {
        name_ids.reserve(seqs.size() * 2);
        for (size_t i = 0; i < seqs.size(); i++) name_ids[seqs[i].getName()].push_back((uint32_t)i);
    });
    const auto it = name_ids.find(name);
    return it == name_ids.end() ? none : it->second;
}
bool reference_store::name_order_ready() {
    int state = name_order_state.load(std::memory_order_acquire);
    if (state == 0) {
        sina_hip_ctx *root = device();
        std::lock_guard<std::mutex> lk(gpu_mu);
        state = name_order_state.load(std::memory_order_relaxed);
        if (state == 0) {
            const uint32_t n = (uint32_t)seqs.size();
            std::vector<uint32_t> by_name(n), rank(n);
            for (uint32_t i = 0; i < n; i++) by_name[i] = i;
            std::sort(by_name.begin(), by_name.end(), [&](uint32_t a, uint32_t b) { return seqs[a].getName() < seqs[b].getName(); });
            bool unique = true;
            for (uint32_t i = 0; i < n; i++) {
                rank[by_name[i]] = i;
                if (i && seqs[by_name[i]].getName() == seqs[by_name[i - 1]].getName()) unique = false;
            }
            if (unique) hip_check(sina_hip_upload_name_order(root, rank.data(), n), "sina_hip_upload_name_order");
            state = unique ? 1 : 2;
            name_order_state.store(state, std::memory_order_release);
        }
    }
    return state == 1;
}
void reference_store::rank_stats(uint64_t *ranked, uint64_t *fallen_back, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases,
                                 uint64_t *launches) {
    sum_kernel_use("sina_hip_rank_stats", sina_hip_rank_stats, kernel_ms, pairs, cand_bases, launches);
    *ranked = n_ranked.load(std::memory_order_relaxed);
    *fallen_back = n_rank_host.load(std::memory_order_relaxed);
}
void reference_store::set_pairs(const uint32_t *pairs, uint32_t n) {
    bool any = false;
    for (uint32_t i = 0; i < n && !any; i++) any = pairs[i] != 0;
    {
        std::lock_guard<std::mutex> lk(helix_mu);
        helix = any ? std::make_shared<const std::vector<uint32_t>>(pairs, pairs + n) : nullptr;
    }
    std::lock_guard<std::mutex> lk(gpu_mu);  // (a context made later uploads it itself: device())
    if (ctx) hip_check(sina_hip_upload_pairs(ctx, pairs, any ? n : 0), "sina_hip_upload_pairs");
}
reference_store::pair_map reference_store::pairs() {
    std::lock_guard<std::mutex> lk(helix_mu);
    return helix;
}
void reference_store::pair_stats(double *kernel_ms, uint64_t *sequences, uint64_t *entries_visited, uint64_t *launches) {
    sum_kernel_use("sina_hip_pair_stats", sina_hip_pair_stats, kernel_ms, sequences, entries_visited, launches);
}
void reference_store::pair_inplace_stats(uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *launches) {
    uint64_t none = 0;  // (this kernel's record has no second volume)
    sum_kernel_use("sina_hip_pair_inplace_stats",
                   [](sina_hip_ctx *c, double *ms, uint64_t *a, uint64_t *, uint64_t *l) { return sina_hip_pair_inplace_stats(c, ms, a, l); },
                   kernel_ms, sequences, &none, launches);
    *trays = n_bp_inplace.load(std::memory_order_relaxed);
}
void reference_store::identity_inplace_stats(uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    sum_kernel_use("sina_hip_identity_inplace_stats", sina_hip_identity_inplace_stats, kernel_ms, sequences, pairs, launches);
    *trays = n_idty_inplace.load(std::memory_order_relaxed);
}
void reference_store::search_inplace_stats(uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    sum_kernel_use("sina_hip_rank_inplace_stats", sina_hip_rank_inplace_stats, kernel_ms, sequences, pairs, launches);
    *trays = n_search_inplace.load(std::memory_order_relaxed);
}
void reference_store::show_dist_stats(uint64_t *trays, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches) {
    sum_kernel_use("sina_hip_show_dist_stats", sina_hip_show_dist_stats, kernel_ms, sequences, pairs, launches);
    *trays = n_show_dist.load(std::memory_order_relaxed);
}
void reference_store::copy_stats(uint64_t *pairs, double *kernel_ms, uint64_t *launches, uint64_t *trays, uint64_t *fallback_trays) {
    uint64_t ref_bases = 0;
    sum_kernel_use("sina_hip_find_bases_stats", sina_hip_find_bases_stats, kernel_ms, pairs, &ref_bases, launches);
    *trays = n_copy_trays.load(std::memory_order_relaxed);
    *fallback_trays = n_copy_fallback.load(std::memory_order_relaxed);
}
void reference_store::turn_stats(uint64_t *queries, uint64_t *turned, double *kernel_ms, uint64_t *launches, uint64_t *rows_trays,
                                 uint64_t *orient_trays, uint64_t *fallback_trays) {
    sum_kernel_use("sina_hip_turn_stats", sina_hip_turn_stats, kernel_ms, queries, turned, launches);
    *rows_trays = n_turn_rows.load(std::memory_order_relaxed);
    *orient_trays = n_turn_orient.load(std::memory_order_relaxed);
    *fallback_trays = n_turn_fallback.load(std::memory_order_relaxed);
}
void reference_store::assemble_stats(uint64_t *trays_device, uint64_t *trays_host, uint64_t *queries, uint64_t *assembled,
                                     uint64_t *shifted_queries, uint64_t *shifted_runs) {
    *queries = *assembled = *shifted_queries = *shifted_runs = 0;
    for_each_context([&](sina_hip_ctx *c) {
        uint64_t q = 0, a = 0, sq = 0, sr = 0;
        hip_check(sina_hip_assemble_stats(c, &q, &a, &sq, &sr), "sina_hip_assemble_stats");
        *queries += q;
        *assembled += a;
        *shifted_queries += sq;
        *shifted_runs += sr;
    });
    *trays_device = n_fin_device.load(std::memory_order_relaxed);
    *trays_host = n_fin_host.load(std::memory_order_relaxed);
}
bool reference_store::match_counts_too_wide() {
    if (sina_hip::match_table_bytes(width) <= sina_hip::kMatchMaxLds) return false;
    if (!too_wide_said.exchange(true))
        fprintf(stderr, "famfinder: device-msc: the alignment's %u columns are more than the device's match count takes; "
                        "identities stay with the host walk\n", width);
    return true;
}
reference_store::lease::~lease() {
    if (!c) return;
    std::lock_guard<std::mutex> lk(st->gpu_mu);
    st->idle_forks[role].push_back(c);
}

const cseq &reference_store::getCseq(const std::string &name) const {
    for (const auto &c : seqs)
        if (c.getName() == name) return c;
    throw std::runtime_error("no such sequence: " + name);
}
const std::string &reference_store::upper_bases(unsigned int id) {
    std::call_once(ubases_once, [this] {
        ubases.resize(seqs.size());
        parallel_for(seqs.size(), [this](size_t i) {
            std::string b = seqs[i].getBases();
            for (auto &ch : b) ch = (char)toupper((unsigned char)ch);
            ubases[i].swap(b);
        });
    });
    return ubases[id];
}
const std::string &reference_store::family_label(unsigned int id) {
    if (!labels_ready.load(std::memory_order_acquire)) {  // (set_attr resets it: stores are not modified while pipelines run)
        std::lock_guard<std::mutex> lk(labels_mu);
        if (!labels_ready.load(std::memory_order_relaxed)) {
            labels.assign(seqs.size(), std::string());
            for (size_t i = 0; i < seqs.size(); i++) {
                loadKey(seqs[i], fn::acc);
                loadKey(seqs[i], fn::start);
                labels[i] = seqs[i].get_attr<std::string>(fn::acc) + "." + seqs[i].get_attr<std::string>(fn::start, "0");
            }
            labels_ready.store(true, std::memory_order_release);
        }
    }
    return labels[id];
}
std::vector<std::string> reference_store::getSequenceNames() const {
    std::vector<std::string> v;
    v.reserve(seqs.size());
    for (const auto &c : seqs) v.push_back(c.getName());
    return v;
}
void reference_store::loadKey(const cseq &, const std::string &) const {
    // attributes of FASTA-backed references are loaded eagerly (acc := name); nothing to fetch
}

sina_hip_ctx *reference_store::device() {
    std::lock_guard<std::mutex> lk(gpu_mu);
    if (ctx) return ctx;
    hip_check(sina_hip_init(device_id, &ctx), "sina_hip_init");
    if (const pair_map m = pairs()) hip_check(sina_hip_upload_pairs(ctx, m->data(), (uint32_t)m->size()), "sina_hip_upload_pairs");
    if (refs_by_broadcast) return ctx;  // (filled in place by the start-up broadcast, sina_amd/dist.py)
    std::vector<uint32_t> ab;
    std::vector<uint64_t> off(seqs.size() + 1, 0);
    size_t total = 0;
    for (const auto &c : seqs) total += c.size();
    ab.reserve(total);
    for (size_t i = 0; i < seqs.size(); i++) {
        const uint32_t *p = seqs[i].packed();
        ab.insert(ab.end(), p, p + seqs[i].size());
        off[i + 1] = ab.size();
    }
    hip_check(sina_hip_upload_refs(ctx, ab.data(), off.data(), (uint32_t)seqs.size(), width), "upload_refs");
    return ctx;
}

void reference_store::ensure_index(unsigned k, bool nofast) {
    sina_hip_ctx *c = device();
    std::lock_guard<std::mutex> lk(gpu_mu);
    if (idx_k == (int)k && idx_nofast == nofast) return;
    // One index per store on the device: a second (k, fast) combination would replace the index
    // under the feet of the batches in flight (the reference keeps one kmer_search object per
    // combination; use a second store for that).
    if (idx_k != -1)
        throw std::logic_error("reference store " + path + " already has a k-mer index for k=" + std::to_string(idx_k) +
                               (idx_nofast ? " (no-fast)" : " (fast)") +
                               "; famfinder and search must use the same --fs-kmer-len / --fs-kmer-no-fast");
    // kmer_search::impl::impl (src/kmer_search.cpp:213-243): a file-backed database keeps its index
    // in <db>.sidx -- load it if it is not older than the database, else build and store it.
    // (":..." names are in-memory stores: always built.)
    std::string idxpath;
    if (!path.empty() && path[0] != ':') {
        const size_t dot = path.find_last_of('.'), slash = path.find_last_of('/');
        idxpath = (dot != std::string::npos && (slash == std::string::npos || dot > slash) ? path.substr(0, dot) : path) +
                  ".sidx";
    }
    bool loaded = false;
    if (!idxpath.empty()) {
        struct stat si, sd;
        if (stat(idxpath.c_str(), &si) == 0 && stat(path.c_str(), &sd) == 0 &&
            (si.st_mtim.tv_sec > sd.st_mtim.tv_sec ||
             (si.st_mtim.tv_sec == sd.st_mtim.tv_sec && si.st_mtim.tv_nsec >= sd.st_mtim.tv_nsec))) {
            std::vector<std::string> names;
            std::vector<uint32_t> offsets, ids;
            if (sidx_load(idxpath, k, nofast, &names, &offsets, &ids) && names.size() == seqs.size()) {
                // The file's posting ids count ITS name list (the reference resolves ids through the names it
                // stored: kmer_search.cpp try_load + getCseq(sequence_names[id])).  This store may number the
                // same database differently -- file order vs the ARB walk order of a stock-SINA .sidx
                // (reference_store::open(path, arb_id_order)) -- so: same names in the same order -> take the
                // lists as they are; the same names in another order -> renumber every list through a
                // name -> id table and re-sort it; anything else -> not this database's index, rebuild.
                bool same_order = true;
                for (size_t i = 0; i < seqs.size() && same_order; i++) same_order = names[i] == seqs[i].getName();
                bool usable = same_order;
                if (!same_order) {
                    std::unordered_map<std::string, uint32_t> id_of;
                    id_of.reserve(seqs.size() * 2);
                    for (size_t i = 0; i < seqs.size(); i++) id_of.emplace(seqs[i].getName(), (uint32_t)i);
                    std::vector<uint32_t> remap(names.size());
                    std::vector<char> hit(seqs.size(), 0);
                    usable = id_of.size() == seqs.size();
                    for (size_t i = 0; i < names.size() && usable; i++) {
                        auto it = id_of.find(names[i]);
                        usable = it != id_of.end() && !hit[it->second];
                        if (usable) {
                            remap[i] = it->second;
                            hit[it->second] = 1;
                        }
                    }
                    // (a corrupt or foreign cache may name ids beyond its own name list: rebuilt, not followed)
                    for (size_t i = 0; i < ids.size() && usable; i++) usable = ids[i] < remap.size();
                    if (usable) {
                        for (auto &id : ids) id = remap[id];
                        parallel_for(offsets.size() - 1, [&](size_t km) {
                            if (offsets[km + 1] - offsets[km] > 1) std::sort(ids.begin() + offsets[km], ids.begin() + offsets[km + 1]);
                        });
                    }
                }
                if (usable) {
                    hip_check(sina_hip_upload_index(c, k, nofast ? 1 : 0, offsets.data(), ids.data(), ids.size()),
                              "upload_index");
                    loaded = true;
                    idx_origin = std::string(same_order ? "loaded " : "loaded (ids renumbered by name) ") + idxpath;
                }
            }
        }
    }
    if (!loaded) {
        hip_check(sina_hip_build_index(c, k, nofast ? 1 : 0), "build_index");
        idx_origin = "built";
        if (!idxpath.empty()) {
            sina_hip_store_view v;
            hip_check(sina_hip_store_view_get(c, &v), "store_view_get");
            std::vector<uint32_t> offsets(((size_t)1 << (2 * k)) + 1), ids(v.n_postings ? v.n_postings : 1);
            hip_check(sina_hip_download_index(c, offsets.data(), ids.data()), "download_index");
            ids.resize(v.n_postings);
            std::vector<std::string> names;
            for (const auto &sq : seqs) names.push_back(sq.getName());
            try {
                sidx_store(idxpath, k, nofast, names, offsets, ids);
            } catch (const std::exception &) {
                // (a read-only database directory: keep the in-memory index, like a failed ofstream)
            }
        }
    }
    idx_k = (int)k;
    idx_nofast = nofast;
}

// ================================================================ kmer_search

class kmer_search::impl {
public:
    std::shared_ptr<reference_store> store;
    unsigned k;
    bool nofast;
    impl(std::shared_ptr<reference_store> s, unsigned k_, bool nofast_) : store(std::move(s)), k(k_), nofast(nofast_) {
        store->ensure_index(k, nofast);
    }
};

namespace {
struct idx_key {
    std::string path;
    int k;
    bool nofast;
    bool operator<(const idx_key &o) const { return std::tie(path, k, nofast) < std::tie(o.path, o.k, o.nofast); }
};
std::mutex indices_mu;
std::map<idx_key, std::shared_ptr<kmer_search::impl>> indices;
}  // namespace

// src/kmer_search.cpp:118-144
kmer_search *kmer_search::get_kmer_search(const std::string &filename, int k, bool nofast) {
    std::lock_guard<std::mutex> lk(indices_mu);
    idx_key key{filename, k, nofast};
    auto it = indices.find(key);
    if (it == indices.end())
        it = indices.emplace(key, std::make_shared<impl>(reference_store::get(filename), (unsigned)k, nofast)).first;
    return new kmer_search(it->second);
}
void kmer_search::release_kmer_search(const std::string &filename, int k, bool nofast) {
    std::lock_guard<std::mutex> lk(indices_mu);
    indices.erase(idx_key{filename, k, nofast});
}
kmer_search::kmer_search(std::shared_ptr<impl> p) : pimpl(std::move(p)) {}
kmer_search::~kmer_search() = default;
unsigned int kmer_search::size() const { return pimpl->store->size(); }

double kmer_search::match(result_vector &, const cseq &, int, int, float, float, reference_store *, bool, int, int,
                          int, int, bool) {
    throw std::runtime_error("Legacy family composition not implemented for internal search");
}

void kmer_search::find(const cseq &query, result_vector &results, unsigned int max) {
    std::vector<const cseq *> q{&query};
    std::vector<result_vector> r;
    find_batch(q, r, max);
    results = std::move(r[0]);
}

// src/kmer_search.cpp:366-420 for a batch of queries
// Number of k-mers of a query with multiplicity (kmer.h:188-201): windows of k bases with exactly one base bit
// each, ending before the last base; with the "fast" prefix filter only those starting with A.  Counted as
// (candidate starts) - (starts whose window holds an ambiguous base): both loops over the bytes vectorise, the
// per-window work is done for the few ambiguous bases only (a running-length loop was 2.7 us per 16S query).
static unsigned count_query_kmers(const uint8_t *m, size_t n, unsigned k, bool count_all) {
    if (n < (size_t)k + 1) return 0;
    const size_t last_start = n - 1 - k;  // window [i, i + k), i + k - 1 <= n - 2
    unsigned total = 0;
    if (count_all) total = (unsigned)(last_start + 1);
    else
        for (size_t i = 0; i <= last_start; i++) total += (m[i] & 0xfu) == 1u;
    long covered_to = -1;  // starts up to here are already taken off
    for (size_t blk = 0; blk + 1 < n; blk += 64) {
        const size_t end = std::min(n - 1, blk + 64);
        unsigned bad = 0;
        for (size_t p = blk; p < end; p++) {
            const unsigned x = m[p] & 0xfu;
            bad += (x == 0u) | ((x & (x - 1u)) != 0u);
        }
        if (bad == 0) continue;
        for (size_t p = blk; p < end; p++) {
            const unsigned x = m[p] & 0xfu;
            if (x != 0u && (x & (x - 1u)) == 0u) continue;
            const long lo = std::max<long>(std::max<long>((long)p - (long)k + 1, covered_to + 1), 0);
            const long hi = std::min<long>((long)p, (long)last_start);
            for (long i = lo; i <= hi; i++) total -= count_all ? 1u : (unsigned)((m[i] & 0xfu) == 1u);
            if (hi > covered_to) covered_to = hi;
        }
    }
    return total;
}

// Batch-level memoisation of repeated queries (distinct.h): items with the same key bytes go to the device once.
// set_batch_dedup(false) switches it off (tests compare against the un-deduplicated run).
static std::atomic<int> g_dedup{1};
void set_batch_dedup(bool on) { g_dedup.store(on ? 1 : 0); }
bool dedup_enabled() { return g_dedup.load(std::memory_order_relaxed) != 0; }
// (pack_masks, pack_words, offsets_of and columns_ascend, which the aligner and the search stage use too: stages_internal.h)

// The device's match counts ask for strictly ascending columns.  Takes a batch in which is_plain marks the queries
// without them; searches the others with counts and those through the entry without, each kind in a call of its own
// (find_batch again), and puts every result back at its query's place.  The rows of the marked queries stay empty.
static void find_by_columns(kmer_search &ks, const std::vector<const cseq *> &queries, const std::vector<char> &is_plain,
                            std::vector<search::result_vector> &results, unsigned int max, std::vector<uint32_t> *kmer_counts,
                            std::vector<std::vector<uint16_t>> &match_rows) {
    for (int pass = 0; pass < 2; pass++) {
        std::vector<size_t> at;
        std::vector<const cseq *> sub;
        for (size_t i = 0; i < queries.size(); i++)
            if ((is_plain[i] != 0) == (pass == 1)) {
                at.push_back(i);
                sub.push_back(queries[i]);
            }
        if (sub.empty()) continue;
        std::vector<search::result_vector> sub_results(sub.size());
        for (size_t x = 0; x < sub.size(); x++) sub_results[x].swap(results[at[x]]);
        std::vector<uint32_t> sub_counts;
        std::vector<std::vector<uint16_t>> sub_rows;
        ks.find_batch(sub, sub_results, max, kmer_counts ? &sub_counts : nullptr, pass == 0 ? &sub_rows : nullptr);
        if (kmer_counts && kmer_counts->size() != queries.size()) kmer_counts->assign(queries.size(), 0);
        for (size_t x = 0; x < sub.size(); x++) {
            results[at[x]].swap(sub_results[x]);
            if (kmer_counts) (*kmer_counts)[at[x]] = sub_counts[x];
            if (pass == 0) match_rows[at[x]].swap(sub_rows[x]);
        }
    }
}

// Takes the distinct queries as the device reads them -- mask bytes, or packed words where match counts are asked for
// (dev_ab and match_rows both set) -- and searches them; gives every query the `max` best of its slot: results[i], and
// the match counts by rank in (*match_rows)[i].
// Up to 4096 candidates per query the distinct queries go to the device in one call, as ever.  More (famfinder
// widening its list tenfold per round, a large search-kmer-candidates): d.n * max ids and scores are no longer one
// scratch block -- the distinct queries are taken in slices of as many as one launch range of the device's big
// select holds (kmer_plan.h: the same function, the same budget, so a slice is one launch), and `results` is filled
// slice by slice.
// turn (famfinder's device-turn; null: none): the device orients every distinct query first and the rows are those of
// its chosen orientation, slot_turn[u] (sina_hip_kmer_topk_turn).  Returns false, without a throw, if such a call fails.
static bool search_slices(reference_store &st, sina_hip_ctx *ctx, const distinct_items &d, const uint8_t *dev_mask, const uint32_t *dev_ab,
                          unsigned int max, std::vector<search::result_vector> &results, std::vector<std::vector<uint16_t>> *match_rows,
                          const kmer_search::turn_request *turn = nullptr, uint8_t *slot_turn = nullptr) {
    const size_t nu = d.n;
    const size_t slice = max > sina_hip::kKmerSelMax ? sina_hip::big_select_range((uint32_t)nu, max, sina_hip::kBigSelBudget) : nu;
    thread_local batch_scratch<uint32_t> ids_buf;
    thread_local batch_scratch<float> sc_buf;
    uint32_t *const ids = ids_buf.get(slice * max);
    float *const sc = sc_buf.get(slice * max);
    std::vector<uint32_t> cnt(slice);
    thread_local batch_scratch<uint16_t> mt_buf;
    uint16_t *const mt = match_rows ? mt_buf.get(slice * max) : nullptr;
    for (size_t u0 = 0; u0 < nu; u0 += slice) {
        const size_t u1 = std::min(nu, u0 + slice);
        {
            scoped_phase ph("ff.kmer_topk(C-ABI)");
            // (the _any entry: the class has no length limit of its own, as the reference's -- a query beyond the fast count
            // kernel's goes to the long one, per query; offsets are absolute, so a slice starts at d.off + u0)
            if (turn) {
                std::vector<float> top1(4 * (u1 - u0));
                if (sina_hip_kmer_topk_turn(ctx, dev_mask, d.off.data() + u0, (uint32_t)(u1 - u0), max, turn->all ? 1 : 0, slot_turn + u0, top1.data(),
                                            ids, sc, cnt.data()) != 0)
                    return false;
            } else if (match_rows)
                hip_check(sina_hip_kmer_topk_match(ctx, dev_ab, d.off.data() + u0, (uint32_t)(u1 - u0), max, ids, sc, cnt.data(), mt), "kmer_topk_match");
            else
                hip_check(sina_hip_kmer_topk_any(ctx, dev_mask, d.off.data() + u0, (uint32_t)(u1 - u0), max, ids, sc, cnt.data()), "kmer_topk");
        }
        parallel_for(results.size(), [&](size_t i) {
            const size_t u = d.slot_of[i];
            if (u < u0 || u >= u1) return;
            const size_t at = (u - u0) * max;
            results[i].reserve(cnt[u - u0]);
            for (uint32_t x = 0; x < cnt[u - u0]; x++) results[i].emplace_back(sc[at + x], &st.getCseq(ids[at + x]));
            if (match_rows) (*match_rows)[i].assign(mt + at, mt + at + cnt[u - u0]);
        });
    }
    return true;
}

// famfinder's device-cascade: searches the distinct (words, self list) pairs of a batch with the cascade behind the
// search (sina_hip_kmer_topk_family) and fills every query's results with its family, found by id.  More than 4096
// candidates per query: in slices of one launch range of the device's big select, like search_slices.
static void search_families(reference_store &st, sina_hip_ctx *ctx, const std::vector<const cseq *> &queries, const uint32_t *qab,
                            const uint64_t *qoff, unsigned int max, std::vector<search::result_vector> &results,
                            kmer_search::family_request &fr) {
    using request = kmer_search::family_request;
    const size_t nq = queries.size();
    // a query's self list: the references of its name.  Two trays with the same bases under different names share a row
    // only where their lists are equal
    static const std::vector<uint32_t> no_self;
    std::vector<const std::vector<uint32_t> *> selfs(nq, &no_self);
    if (fr.leave_out)
        for (size_t i = 0; i < nq; i++) selfs[i] = &st.ids_of_name(queries[i]->name_ref());
    const distinct_items d = distinct_spans(
        dedup_enabled(), parallel_for, qab, qoff, nq,
        [&](size_t i) { return hash_bytes(selfs[i]->data(), 4 * selfs[i]->size(), selfs[i]->size()); },
        [&](size_t a, size_t b) { return selfs[a] == selfs[b] || *selfs[a] == *selfs[b]; });
    thread_local batch_scratch<uint32_t> uab_buf;
    const uint32_t *const dev_ab = gather_distinct(d, parallel_for, qab, qoff, uab_buf);
    const size_t nu = d.n;
    std::vector<uint32_t> self_ids;
    std::vector<uint64_t> self_off(nu + 1, 0);
    for (size_t u = 0; u < nu; u++) {
        const std::vector<uint32_t> &s = *selfs[d.first.empty() ? u : d.first[u]];
        self_ids.insert(self_ids.end(), s.begin(), s.end());
        self_off[u + 1] = self_ids.size();
    }
    self_ids.push_back(0);  // (never empty: data() is the list's address)
    uint32_t words = 0;
    hip_check(sina_hip_family_row_words(&fr.rule, &words), "family_row_words");
    const uint32_t K = (words - 2) / 2;
    const size_t slice = max > sina_hip::kKmerSelMax ? sina_hip::big_select_range((uint32_t)nu, max, sina_hip::kBigSelBudget) : nu;
    thread_local batch_scratch<uint32_t> rows_buf;
    uint32_t *const rows = rows_buf.get(slice * words);
    for (size_t u0 = 0; u0 < nu; u0 += slice) {
        const size_t u1 = std::min(nu, u0 + slice);
        {
            scoped_phase ph("ff.kmer_topk_family(C-ABI)");
            hip_check(sina_hip_kmer_topk_family(ctx, dev_ab, d.off.data() + u0, (uint32_t)(u1 - u0), max, &fr.rule,
                                                fr.leave_out ? self_ids.data() : nullptr, fr.leave_out ? self_off.data() + u0 : nullptr, rows),
                      "kmer_topk_family");
        }
        parallel_for(nq, [&](size_t i) {
            const size_t u = d.slot_of[i];
            if (u < u0 || u >= u1) return;
            const uint32_t *row = rows + (u - u0) * words;
            results[i].reserve(row[0]);
            for (uint32_t x = 0; x < row[0]; x++) {
                float score;
                memcpy(&score, &row[2 + K + x], 4);
                results[i].emplace_back(score, &st.getCseq(row[2 + x]));
            }
            fr.state[i] = (uint8_t)(request::on_device | (row[1] & 1u ? request::enough : 0) | (row[1] & 2u ? request::empty_list : 0));
        });
    }
}

// Clears the outputs, packs the queries, finds the distinct ones, searches those and scatters what they found.
void kmer_search::find_batch(const std::vector<const cseq *> &queries, std::vector<result_vector> &results,
                             unsigned int max, std::vector<uint32_t> *kmer_counts, std::vector<std::vector<uint16_t>> *match_rows,
                             family_request *family, turn_request *turn) {
    reference_store &st = *pimpl->store;
    const size_t nq = queries.size();
    if (family) family->state.assign(nq, 0);
    if (turn) {
        if (match_rows || family) throw std::logic_error("find_batch: a turn request goes with neither match counts nor the cascade");
        turn->o.assign(nq, 0);
        turn->done = false;
    }
    // (the callers' vectors are kept -- famfinder hands in recycled ones -- and only emptied)
    results.resize(nq);
    for (auto &r : results) r.clear();
    if (match_rows) {
        match_rows->resize(nq);
        for (auto &r : *match_rows) r.clear();
    }
    if (max > st.size()) max = st.size();
    if (max == 0 || queries.empty()) return;
    // The device's match counts (famfinder's device-msc): kept from a store too wide for the kernel's table -- said
    // once, then every query keeps the host walk -- and from a query whose columns do not ascend strictly.
    if (match_rows && st.match_counts_too_wide()) match_rows = nullptr;
    if (family && family->rule.fs_msc_max < 1) {
        // the cascade's identity limit asks for strictly ascending columns too: the queries without them keep the
        // path without the request, in a call of their own
        std::vector<size_t> at[2];
        for (size_t i = 0; i < nq; i++) at[columns_ascend(*queries[i]) ? 0 : 1].push_back(i);
        if (!at[1].empty()) {
            if (kmer_counts) kmer_counts->assign(nq, 0);
            for (int pass = 0; pass < 2; pass++) {
                if (at[pass].empty()) continue;
                std::vector<const cseq *> sub;
                for (size_t i : at[pass]) sub.push_back(queries[i]);
                std::vector<result_vector> sub_results(sub.size());
                for (size_t x = 0; x < sub.size(); x++) sub_results[x].swap(results[at[pass][x]]);
                std::vector<uint32_t> sub_counts;
                family_request sub_family{family->rule, family->leave_out, {}};
                find_batch(sub, sub_results, max, kmer_counts ? &sub_counts : nullptr, nullptr, pass == 0 ? &sub_family : nullptr);
                for (size_t x = 0; x < sub.size(); x++) {
                    results[at[pass][x]].swap(sub_results[x]);
                    if (kmer_counts) (*kmer_counts)[at[pass][x]] = sub_counts[x];
                    if (pass == 0) family->state[at[pass][x]] = sub_family.state[x];
                }
            }
            return;
        }
    }
    if (match_rows && !family) {
        std::vector<char> is_plain(nq, 0);
        bool any_plain = false;
        for (size_t i = 0; i < nq; i++) any_plain |= (is_plain[i] = !columns_ascend(*queries[i]));
        if (any_plain) return find_by_columns(*this, queries, is_plain, results, max, kmer_counts, *match_rows);
    }
    st.ensure_index(pimpl->k, pimpl->nofast);
    auto seq_of = [&](size_t i) -> const cseq & { return *queries[i]; };
    const std::vector<uint64_t> qoff = offsets_of(nq, seq_of);
    thread_local batch_scratch<uint8_t> qmask_buf;
    uint8_t *const qmask = qmask_buf.get(qoff.back() + 1);
    if (kmer_counts) kmer_counts->assign(nq, 0);
    pack_masks(nq, seq_of, qoff.data(), qmask, [&, kk = pimpl->k, count_all = pimpl->nofast](size_t i, const uint8_t *m, size_t nb) {
        if (kmer_counts) (*kmer_counts)[i] = count_query_kmers(m, nb, kk, count_all);
    });
    // with match counts the device takes the queries as packed aligned bases
    thread_local batch_scratch<uint32_t> qab_buf;
    if (family) match_rows = nullptr;  // (the counts stay on the device)
    uint32_t *const qab = match_rows || family ? qab_buf.get(qoff.back() + 1) : nullptr;
    if (qab) pack_words(nq, seq_of, qoff.data(), qab);
    auto dev = st.worker_device(reference_store::dev_search);
    if (family) return search_families(st, dev.get(), queries, qab, qoff.data(), max, results, *family);
    // repeated queries (same bases, same case: the packed mask bytes) are searched once
    // (with match counts: same PACKED WORDS -- equal bases in other columns are another query there)
    const distinct_items d = qab ? distinct_spans(dedup_enabled(), parallel_for, qab, qoff.data(), nq)
                                 : distinct_spans(dedup_enabled(), parallel_for, qmask, qoff.data(), nq);
    thread_local batch_scratch<uint8_t> umask_buf;
    thread_local batch_scratch<uint32_t> uab_buf;
    const uint8_t *const dev_mask = gather_distinct(d, parallel_for, qmask, qoff.data(), umask_buf);
    const uint32_t *const dev_ab = qab ? gather_distinct(d, parallel_for, qab, qoff.data(), uab_buf) : nullptr;
    if (!turn) {
        search_slices(st, dev.get(), d, dev_mask, dev_ab, max, results, match_rows);
        return;
    }
    std::vector<uint8_t> slot_turn(d.n, 0);
    if (!search_slices(st, dev.get(), d, dev_mask, nullptr, max, results, nullptr, turn, slot_turn.data())) {
        for (auto &r : results) r.clear();  // (a later slice's call failed: nothing of the batch counts)
        return;
    }
    // the orientations, and the k-mer counts of the queries as turned (with the fast index they differ by orientation)
    parallel_for(nq, [&](size_t i) {
        const uint32_t o = slot_turn[d.slot_of[i]];
        turn->o[i] = (uint8_t)o;
        if (!o || !kmer_counts) return;
        const uint8_t *m = qmask + qoff[i];
        const size_t nb = (size_t)(qoff[i + 1] - qoff[i]);
        std::vector<uint8_t> v(nb);
        for (size_t x = 0; x < nb; x++) v[x] = sina_hip::turn_variant_byte(m, nb, o, x);
        (*kmer_counts)[i] = count_query_kmers(v.data(), nb, pimpl->k, pimpl->nofast);
    });
    turn->done = true;
}

}  // namespace sina
