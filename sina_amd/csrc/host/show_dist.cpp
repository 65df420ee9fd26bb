// --show-dist on the device (the aligner's device-dist): show_dist_batch, the batch drivers' step
// behind pair_score_batch, and the switch that says whether a run shows dist at all.  What the sink would walk for a
// tray -- its input alignment against its new one, against every relative, and the new one against the closest
// (rw_fasta.cpp, show_dist_report: about 42 merge-walks of two sequences per query) -- is counted for the whole batch
// by one sina_hip_show_dist call; the tray carries the twenty words to the sink (tray::dist_row), which turns them into
// the report's floats with cseq_comparator::score, the function the walk ends in.
//
// Trays that keep the host walk, because the device would not compare as the host does or cannot take them: a tray
// without an aligned sequence; one whose input and aligned widths differ (its report is the "Cannot show dist" line)
// or differ from the store's; one whose input or aligned columns do not ascend strictly, or that has more than 65535
// bases; one whose list has a member the store does not own; every tray when the store's names repeat (the closest
// relative among equals is chosen by name) or the device refuses the call as a limit; a tray whose row comes back
// flagged (a member without a score: the host orders its NaN as std::sort does).  Nothing of this reaches a tray's log.
#include "stages.h"
#include "stages_internal.h"
#include "../showdist_plan.h"

#include <atomic>
#include <cstring>

namespace sina {

namespace {
std::atomic<bool> g_show_dist{false};

const search::result_vector *relatives_of(const tray &t) {
    return t.search_result != nullptr ? t.search_result : t.alignment_reference;
}
bool device_takes(const cseq &c, uint32_t width) {
    return c.getWidth() == width && c.size() <= sina_hip::kShowDistMaxBases && columns_ascend(c);
}
}  // namespace

bool show_dist_wanted() { return g_show_dist.load(std::memory_order_relaxed); }
void set_show_dist(bool on) { g_show_dist.store(on, std::memory_order_relaxed); }

void show_dist_prepare() {
    if (!show_dist_wanted() || aligner::opts == nullptr || !aligner::opts->device_dist) return;
    for (const std::string &key : {aligner::opts->database, search_filter_database()})
        if (!key.empty())
            if (const std::shared_ptr<reference_store> st = reference_store::find(key)) st->name_order_ready();
}

void show_dist_batch(std::vector<tray> &batch) {
    if (!show_dist_wanted() || aligner::opts == nullptr || !aligner::opts->device_dist) return;
    // the store that owns a tray's relatives: the search stage's for a search result, the aligner's for a family
    std::shared_ptr<reference_store> st_family, st_search;
    if (!aligner::opts->database.empty()) st_family = reference_store::find(aligner::opts->database);
    std::vector<reference_store *> owner(batch.size(), nullptr);
    {
        scoped_phase ph("sd.select");
        for (const tray &t : batch)
            if (t.search_result != nullptr && !st_search) {
                st_search = reference_store::find(search_filter_database());
                break;
            }
        parallel_for(batch.size(), [&](size_t i) {
            tray &t = batch[i];
            if (t.aligned_sequence == nullptr || t.input_sequence == nullptr || t.dist_row_set) return;
            reference_store *st = (t.search_result != nullptr ? st_search : st_family).get();
            if (st == nullptr) return;
            const uint32_t width = st->getAlignmentWidth();
            if (!device_takes(*t.input_sequence, width) || !device_takes(*t.aligned_sequence, width)) return;
            if (const search::result_vector *ref = relatives_of(t))
                for (const search::result_item &r : *ref)
                    if (!st->owns(r.sequence)) return;
            owner[i] = st;
        });
    }
    reference_store *const stores[2] = {st_family.get(), st_search.get() != st_family.get() ? st_search.get() : nullptr};
    for (reference_store *st : stores) {
        if (st == nullptr) continue;
        std::vector<size_t> dev;
        for (size_t i = 0; i < batch.size(); i++)
            if (owner[i] == st) dev.push_back(i);
        if (dev.empty() || !st->name_order_ready()) continue;
        const size_t n = dev.size();
        std::vector<uint64_t> o_off(n + 1, 0), a_off(n + 1, 0), r_off(n + 1, 0);
        for (size_t x = 0; x < n; x++) {
            const tray &t = batch[dev[x]];
            const search::result_vector *ref = relatives_of(t);
            o_off[x + 1] = o_off[x] + t.input_sequence->size();
            a_off[x + 1] = a_off[x] + t.aligned_sequence->size();
            r_off[x + 1] = r_off[x] + (ref ? ref->size() : 0);
        }
        std::vector<uint32_t> o_ab((size_t)o_off[n] + 1), a_ab((size_t)a_off[n] + 1), ids((size_t)r_off[n] + 1);
        {
            scoped_phase ph("sd.pack");
            parallel_for(n, [&](size_t x) {
                const tray &t = batch[dev[x]];
                if (t.input_sequence->size()) memcpy(o_ab.data() + o_off[x], t.input_sequence->packed(), 4 * (size_t)t.input_sequence->size());
                if (t.aligned_sequence->size())
                    memcpy(a_ab.data() + a_off[x], t.aligned_sequence->packed(), 4 * (size_t)t.aligned_sequence->size());
                if (const search::result_vector *ref = relatives_of(t)) {
                    uint32_t *w = ids.data() + r_off[x];
                    for (const search::result_item &r : *ref) *w++ = st->id_of(r.sequence);
                }
            });
        }
        std::vector<uint32_t> rows(n * sina_hip::kShowDistRowWords, 0);
        {
            scoped_phase ph("sd.show_dist(C-ABI)");
            reference_store::lease dv = st->worker_device(reference_store::dev_compare);
            const int rc = sina_hip_show_dist(dv.get(), o_ab.data(), o_off.data(), a_ab.data(), a_off.data(), (uint32_t)n, ids.data(),
                                              r_off.data(), rows.data());
            if (rc != 0 && sina_hip_last_error_is_limit() == 1) continue;  // (too wide for the tables: every tray walks)
            hip_check(rc, "sina_hip_show_dist");
        }
        uint64_t taken = 0;
        for (size_t x = 0; x < n; x++) {
            const uint32_t *row = rows.data() + x * sina_hip::kShowDistRowWords;
            if ((row[sina_hip::kShowDistFlags] & (sina_hip::kShowDistFlagNan | sina_hip::kShowDistFlagComputed)) != sina_hip::kShowDistFlagComputed)
                continue;
            tray &t = batch[dev[x]];
            memcpy(t.dist_row.data(), row, 4 * sina_hip::kShowDistRowWords);
            t.dist_row_set = true;
            taken++;
        }
        st->count_show_dist(taken);
    }
}

}  // namespace sina
