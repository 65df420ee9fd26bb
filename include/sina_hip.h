/*
 * sina_hip.h -- C ABI of the MI355X (gfx950) implementation of SINA's per-query
 * hot path: k-mer reference search and partial-order ("mesh") DP alignment.
 *
 * The reference (epruesse/SINA) has no FFI; this is the boundary its stage
 * functors would bind.  Each entry point names the reference code it replaces
 * (paths under the SINA source tree).  Conventions:
 *   - plain pointers + sizes, caller-owned host buffers unless stated;
 *   - every function returns 0 on success, non-zero on error, and
 *     sina_hip_last_error() (thread-local) describes the failure -- the C++
 *     stage functors turn that into SINA's exception / tray.log conventions;
 *   - no C++ types, exceptions or torch types cross this line;
 *   - a context may be used from several host threads; calls on one context
 *     serialise on an internal mutex (one HIP stream per context).
 *
 * Sequences use SINA's own packed form (src/aligned_base.h:287-319):
 *   aligned base = uint32: (column & 0xFFFFFF) | iupac_mask << 24
 *   iupac mask   = A 1, G 2, C 4, T/U 8, lower-case bit 16 (src/aligned_base.h:47-52)
 */
#ifndef SINA_HIP_H
#define SINA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SINA_HIP_ABI_VERSION 5  /* 5: sina_hip_stats grew scout_ms, scout_launches; 4: the row-skip counters, sina_hip_debug_dp_info, _rgain */

typedef struct sina_hip_ctx sina_hip_ctx;

/* ------------------------------------------------------------------ lifecycle */

int sina_hip_abi_version(void);
const char *sina_hip_last_error(void);
/* 1 if the calling thread's last FAILED call was refused because an input exceeds one of the documented limits of
 * the fast path -- sina_hip_align_graphs: nodes, predecessors, query length, spill rows; sina_hip_align_families:
 * too wide, spill rows, exceeds device limits; sina_hip_align_profiles: too wide, exceeds device limits --, else 0.
 * Thread-local like sina_hip_last_error.  Such an input is valid: sina_hip_align_graphs_any takes it. */
int sina_hip_last_error_is_limit(void);

/* Creates a context on HIP device `device` (own stream). */
int sina_hip_init(int device, sina_hip_ctx **ctx);
/* A second context on the same device that shares `parent`'s reference store, k-mer index and
 * statistics but has its own stream and scratch buffers: calls on different contexts run
 * concurrently on the GPU (the reference gets the same effect from its TBB pipeline running
 * several famfinder/aligner filters at once, src/sina.cpp:430-470).  A fork cannot change the
 * store (upload_refs / build_index / upload_index fail on it); destroy forks before the parent,
 * and do not change the parent's store while forks are in use. */
int sina_hip_fork(sina_hip_ctx *parent, sina_hip_ctx **ctx);
/* Brings the scratch buffers ONE kind of call uses (0: k-mer search, 1: alignment, 2: search-stage comparison and ranking) to the
 * largest sizes any context of the store has needed for them so far: device allocations stall every stream of the
 * device, so a host that runs a pipeline makes its worker contexts, and warms them, before the run -- not in it
 * (the reference sizes its per-thread state the same way: one famfinder / aligner copy per worker, made before the
 * flow graph starts, src/sina.cpp:497-519).  No-op where nothing is known yet or the buffers are big enough. */
int sina_hip_prewarm(sina_hip_ctx *ctx, int kind);
void sina_hip_destroy(sina_hip_ctx *ctx);
/* Blocks until all work queued on the context's stream has finished. */
int sina_hip_sync(sina_hip_ctx *ctx);

/* ------------------------------------------------------- reference store + index
 * Replaces: the in-memory sequence cache famfinder/kmer_search read through
 * query_arb::getCseq (src/kmer_search.cpp:417, src/query_arb.cpp:742-755) and
 * kmer_search::impl::build / try_load (src/kmer_search.cpp:245-351).
 */

/* Copies n_refs packed aligned references (concatenated `ab`, offsets `off`
 * [n_refs+1]) of common alignment width `width` into HBM.  An index the store held is forgotten with the
 * references it was made from (its ids name those): build or upload one again before the next search. */
int sina_hip_upload_refs(sina_hip_ctx *ctx, const uint32_t *ab, const uint64_t *off,
                         uint32_t n_refs, uint32_t width);

/* Builds the device k-mer index from the uploaded references, on the GPU:
 * posting list of k-mer v = ascending ids of references containing v at least
 * once (unique_prefix_kmers / unique_kmers + IndexBuilder,
 * src/kmer_search.cpp:152-211,245-276).  Stored as plain
 * CSR (u32 offsets [4^k+1], u32 ids); SINA's list inversion (src/idset.h:367-384)
 * is a storage optimisation with identical scores and is not reproduced. */
int sina_hip_build_index(sina_hip_ctx *ctx, unsigned k, int nofast);

/* Copies the device index back to the host (offsets [4^k+1], ids [n_postings as reported by
 * sina_hip_store_view_get]); used to write the reference's .sidx cache file after a device build
 * (kmer_search::impl::store, src/kmer_search.cpp:279-304). */
int sina_hip_download_index(sina_hip_ctx *ctx, uint32_t *offsets, uint32_t *ids);

/* Alternative to build_index: adopt a host-built CSR index.  The index is taken as it is -- nothing is
 * checked against the references -- and the search kernels rely on this contract:
 *   - offsets has 4^k + 1 entries, starts at 0, never decreases, and offsets[4^k] == n_postings;
 *   - the ids of one list (offsets[v] .. offsets[v + 1] - 1) are strictly ascending: no duplicates -- a list is
 *     read as a sorted set, its postings of one reference tile being a prefix of what is left of it;
 *   - every id is below the number of uploaded references;
 *   - with nofast == 0 only the lists of k-mers that start with A are ever read.
 * Under it no score exceeds the query's number of windows (len - k) nor 32767, which the 16-bit counters and
 * the select kernel's histogram need.  An index outside the contract gives undefined results and can make
 * the count kernel write outside its counters: validate a foreign index on the host first
 * (tests/kmer_cases.py check_csr is such a check). */
int sina_hip_upload_index(sina_hip_ctx *ctx, unsigned k, int nofast, const uint32_t *offsets,
                          const uint32_t *ids, uint64_t n_postings);

/* Device-pointer view of the index and reference store, for the one-off
 * start-up broadcast over RCCL (torch.distributed) described in INTEGRATION.md:
 * rank 0 builds, every rank allocates with sina_hip_alloc_like, then the
 * buffers are broadcast in place. */
typedef struct sina_hip_store_view {
    void *ref_ab;       uint64_t ref_ab_bytes;    /* u32[total bases]           */
    void *ref_off;      uint64_t ref_off_bytes;   /* u64[n_refs+1]              */
    void *idx_offsets;  uint64_t idx_offsets_bytes; /* u32[4^k+1]               */
    void *idx_ids;      uint64_t idx_ids_bytes;   /* u32[n_postings]            */
    uint32_t n_refs, width, k, nofast;
    uint64_t n_postings, total_bases;
} sina_hip_store_view;
int sina_hip_store_view_get(sina_hip_ctx *ctx, sina_hip_store_view *view);
/* Allocates (uninitialised) device buffers of the sizes in `shape` so that a
 * broadcast can fill them; afterwards the context behaves as if it had built
 * the store itself. Pointer members of `shape` are ignored on input and
 * overwritten with the new device pointers. */
int sina_hip_store_alloc_like(sina_hip_ctx *ctx, sina_hip_store_view *shape);

/* ------------------------------------------------------------- k-mer search
 * Replaces kmer_search::impl::find (src/kmer_search.cpp:366-420) for a batch:
 * for every query, count shared k-mers against every reference
 * (prefix_kmers/all_kmers, duplicates counted, final k-mer dropped:
 * src/kmer.h:188-201) and return the top-`max` by (score desc, id desc)
 * (std::greater<std::pair<int16_t,int>>, src/kmer_search.cpp:412).
 *
 *   qmask/qoff : concatenated iupac masks of the queries' bases, offsets [nq+1]
 *   max        : results wanted per query (clamped to n_refs)
 *   out_ids    : [nq * max] reference ids, out_scores: [nq * max] as float
 *                (result_item.score is float, src/search.h:57-60)
 *   out_n      : [nq] number of valid results per query
 */
int sina_hip_kmer_topk(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq,
                       uint32_t max, uint32_t *out_ids, float *out_scores, uint32_t *out_n);

/* Full score vector (score+offset of src/kmer_search.cpp:405-409) of one query
 * against every reference; for tests and the search_filter stage. */
int sina_hip_kmer_scores(sina_hip_ctx *ctx, const uint8_t *qmask, uint32_t qlen, int16_t *scores);

/* The same two calls (arguments, result layout) for queries of 1..SINA_HIP_MAX_LONG_QUERY_LEN bases, as
 * sina_hip_align_graphs_any is to sina_hip_align_graphs.  Routing is per query: a query of up to
 * SINA_HIP_MAX_QUERY_LEN bases runs on the fast kernel, its results bit for bit those of sina_hip_kmer_topk; the
 * longer ones are counted by the long kernel in a launch range of their own (chunks of SINA_HIP_KMER_LONG_CHUNK
 * windows summed into the score row).  Results come back in the caller's order.  A query beyond
 * SINA_HIP_MAX_LONG_QUERY_LEN fails the call as a limit (sina_hip_last_error_is_limit() == 1). */
int sina_hip_kmer_topk_any(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq,
                           uint32_t max, uint32_t *out_ids, float *out_scores, uint32_t *out_n);
int sina_hip_kmer_scores_any(sina_hip_ctx *ctx, const uint8_t *qmask, uint32_t qlen, int16_t *scores);
/* Queries the long count kernel has counted on this context since init / fork. */
int sina_hip_long_queries(sina_hip_ctx *ctx, uint64_t *n);
/* `max` of the two top-k calls is any number >= 1 (0 gives out_n = 0 everywhere).  With M = min(max, n_refs) up to
 * 4096 a query's candidates are sorted in LDS; a larger M goes through the big select: the same cut score and tie
 * rule (the ties at the cut with the LARGEST ids), the survivors sorted by one segmented radix sort per launch range,
 * results bit for bit the same order (score desc, id desc), out_n = M.  Its launch ranges hold at most 1 GiB of keys
 * and outputs (24 bytes per candidate), one query at least.
 * sina_hip_big_select_queries: queries the big select has ranked on this context since init / fork -- a call with
 * M <= 4096 leaves it alone. */
int sina_hip_big_select_queries(sina_hip_ctx *ctx, uint64_t *n);

/* ------------------------------------------------------------- famfinder's --turn (device-turn)
 * Replaces famfinder::turn_check (src/famfinder.cpp:344-378: one top-1 search per tried orientation of the query, made
 * with cseq::reverse / cseq::complement, src/famfinder.cpp:312-341) AND the search of the chosen orientation that
 * follows it (src/famfinder.cpp:439-455), for a batch.  Orientation o = (bit 0: reversed) | (bit 1: complemented);
 * complement is base_iupac::complement on the mask byte (bits 1 <-> 8 and 2 <-> 4, the case bit kept), reverse the
 * byte order.  The queries go up once, as they are; the device makes the variants, searches them, and chooses: over
 * o = 0, 1, 2, 3 the first strictly largest top-1 score above 0, else 0.
 *
 * sina_hip_kmer_topk_turn: nq queries of 0..SINA_HIP_MAX_LONG_QUERY_LEN bases (routing per query as sina_hip_kmer_topk_any's).
 *   qmask/qoff : as sina_hip_kmer_topk takes them
 *   max        : results wanted per query, 1 or more (clamped to n_refs)
 *   all        : 0 tries o = 0 and 3 ("revcomp"), else all four, in the order 0, 3, 1, 2
 *   out_turn   : [nq] the chosen orientation
 *   out_top1   : [nq][4] the top-1 score by orientation (0 for an orientation not tried or without a result): what four
 *                sina_hip_kmer_topk_any calls with max = 1 give as scores
 *   out_ids, out_scores, out_n : as sina_hip_kmer_topk's, bit for bit what sina_hip_kmer_topk_any gives for the CHOSEN
 *                orientation's mask bytes with the same max
 * Refused with a message before anything runs: a null argument, max == 0; a query beyond SINA_HIP_MAX_LONG_QUERY_LEN
 * bases fails the call as a limit.  nq == 0 succeeds and touches nothing.
 *
 * sina_hip_turn_stats: the two kernels' own time (events around their launches) and volume on this context since init /
 * fork: queries oriented, those of them whose chosen orientation is not 0, launches (one of the orient kernel per
 * call, one of the pick kernel per launch range). */
int sina_hip_kmer_topk_turn(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *qoff, uint32_t nq,
                            uint32_t max, int all, uint8_t *out_turn, float *out_top1 /* [nq][4] */,
                            uint32_t *out_ids, float *out_scores, uint32_t *out_n);
int sina_hip_turn_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *queries, uint64_t *turned, uint64_t *launches);

/* ------------------------------------------------------------- search stage
 * Replaces the per-candidate cseq_comparator::operator() calls of search_filter::operator()
 * (src/search_filter.cpp:311-313 and :274-276; traverse + match_counter,
 * src/cseq_comparator.cpp:56-240): for every query (an ALIGNED sequence: packed aligned bases
 * u32 = column | mask << 24, bit 4 of the mask = lower case) and every candidate reference of
 * the store, the six counters the comparator derives its score from.  The float score itself
 * ((float)match / base, Jukes-Cantor) stays with the caller, as in the reference.
 *
 *   q_ab/q_off     : concatenated packed aligned bases of the queries, offsets [nq+1]
 *   cand_ids/off   : concatenated candidate reference ids per query, offsets [nq+1]
 *   iupac_rule     : SINA_CMP_IUPAC_* (base_comp_optimistic / pessimistic / exact, query first)
 *   filter_lowercase : filter_lowercase instead of filter_none
 *   out            : [cand_off[nq]] counters
 * Columns must ascend strictly within a sequence; a side without any unfiltered base gives
 * all-zero counters (the reference dereferences end() there). */
#define SINA_CMP_IUPAC_OPTIMISTIC 0
#define SINA_CMP_IUPAC_PESSIMISTIC 1
#define SINA_CMP_IUPAC_EXACT 2
typedef struct sina_hip_match_counts {
    int32_t only_a_overhang, only_b_overhang, only_a, only_b, match, mismatch;
} sina_hip_match_counts;
int sina_hip_compare(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                     const uint32_t *cand_ids, const uint64_t *cand_off, int iupac_rule, int filter_lowercase,
                     sina_hip_match_counts *out);

/* ------------------------------------------------------------- famfinder's identity filter (--fs-msc-max)
 * The `match` counter alone, under base_comp_optimistic and without the lower-case filter, for many more candidates
 * than the search stage compares: out_match[i] = number of columns where query and candidate i both have a base and
 * (mask_q & mask_c & 0xF) != 0.  Whenever both have a base, the identity the filter tests is
 * (float)match / (float)(bases of the query).
 *
 * sina_hip_match_count (singular: sina_hip_match_counts is the counter struct above): arguments as sina_hip_compare's (sub-ranges of larger offset arrays included);
 *   out_match : [cand_off[nq]] counts, written at cand_off[0] .. cand_off[nq] - 1
 * Refused with a message, before anything runs and with out_match untouched: a null argument, a reference id out of
 * range, a query of more than 65535 bases, a query whose columns do not ascend strictly.  An alignment too wide for
 * the kernel's LDS table (more than 327 680 columns) is refused as a limit (sina_hip_last_error_is_limit() == 1).
 *
 * sina_hip_kmer_topk_match: sina_hip_kmer_topk_any for queries given as packed aligned bases (the mask bytes the
 * k-mer count reads are bits 24..31 of each word), plus the match count of every candidate returned:
 *   out_ids, out_scores, out_n : bit for bit what sina_hip_kmer_topk_any gives for those mask bytes
 *   out_match : [nq * min(max, n_refs)], out_match[q * M + i] belongs to out_ids[q * M + i], i < out_n[q]
 * The counts are computed from the select's ids where they lie in device memory.  A query whose columns do not
 * ascend strictly fails the call (not a limit); a store too wide fails it as a limit.
 *
 * sina_hip_match_stats: the match-count kernel's own time (events around its launches) and volume on this context
 * since init / fork: pairs counted, bases of their candidates, launches. */
int sina_hip_match_count(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                          const uint32_t *cand_ids, const uint64_t *cand_off, uint16_t *out_match);
int sina_hip_kmer_topk_match(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                             uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint16_t *out_match);
int sina_hip_match_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches);

/* ------------------------------------------------------------- famfinder's filter cascade (device-cascade)
 * The cascade of src/famfinder.cpp:497-612 over ranked candidates, restated on the device: candidates
 * are taken in their list's order; one is removed when its reference has fewer than fs_min_len bases, when its id is
 * in the query's self list (--fs-leave-query-out), or -- only where fs_msc_max < 1 --
 * (float)match / (float)(bases of the query) > fs_msc_max (0 for a query without bases); otherwise by the stateful
 * test over have / have_full / have_cover_left / have_cover_right, the score test being `score < fs_msc` (sic).
 *
 * A query's row is 2 + 2 K 32-bit words, K = max(fs_min, fs_max) + fs_req_full + 2 * fs_cover_gene:
 *   word 0 the number kept; word 1 flags (bit 0: the cascade has enough; bit 1: the list was empty); K ids; K score
 *   bit patterns; entries beyond the number kept are zero.
 * sina_hip_family_row_words gives 2 + 2 K; a rule whose K exceeds 1024 is refused as a limit, by every entry here.
 *
 * sina_hip_family_cascade: the cascade over the caller's lists against the uploaded references.
 *   cand_ids, cand_scores, cand_match : query q's candidates at cand_off[q] .. cand_off[q + 1] - 1 (sub-ranges of larger
 *                                       offset arrays included); cand_match may be NULL when fs_msc_max >= 1 and is
 *                                       not read then
 *   q_bases   : [nq] bases of every query
 *   self_ids, self_off : the queries' self lists, like the candidates; both NULL: no leave-out
 *   out_rows  : [nq][2 + 2 K]
 * sina_hip_kmer_topk_family: sina_hip_kmer_topk_match's search with the cascade behind it, over the select's rows where
 * they lie in device memory; nothing but the rows comes to the host.  With fs_msc_max >= 1 no match count is launched
 * and the queries' columns are not checked.
 * Refused with a message, before anything runs and with out_rows untouched: a null argument, a reference id or a self
 * id out of range, and for fs_msc_max < 1 a query whose columns do not ascend strictly; as a limit: a rule over the
 * cap, and for fs_msc_max < 1 an alignment too wide for the match count's table.
 *
 * sina_hip_family_stats: the cascade kernel's own time and volume on this context since init / fork: queries,
 * candidates their lists held, candidates the kernel's steps covered before it stopped, launches. */
typedef struct sina_hip_family_rule {
    uint32_t fs_min, fs_max, fs_req_full, fs_full_len, fs_min_len, fs_cover_gene;
    float fs_msc, fs_msc_max;
} sina_hip_family_rule;
int sina_hip_family_row_words(const sina_hip_family_rule *r, uint32_t *words);
int sina_hip_family_cascade(sina_hip_ctx *ctx, const uint32_t *cand_ids, const float *cand_scores, const uint16_t *cand_match,
                            const uint64_t *cand_off, const uint32_t *q_bases, uint32_t nq, const sina_hip_family_rule *r,
                            const uint32_t *self_ids, const uint64_t *self_off, uint32_t *out_rows);
int sina_hip_kmer_topk_family(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t max,
                              const sina_hip_family_rule *r, const uint32_t *self_ids, const uint64_t *self_off,
                              uint32_t *out_rows);
int sina_hip_family_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *queries, uint64_t *candidates_listed,
                          uint64_t *candidates_scanned, uint64_t *launches);

/* ------------------------------------------------------------- search stage: score and rank on the device
 * What search_filter::operator() does with the counters above (src/search_filter.cpp:271-331): the score
 * (float)match / denom of every candidate, denom the integer the cover rule picks (cseq_comparator::score,
 * src/cseq_comparator.cpp:240-296; no Jukes-Cantor correction), and the max_result best by
 * std::greater<result_item> (src/search.h:56-68): score descending, equal scores by the reference's NAME descending
 * (byte-wise std::string order).  Only those rows come back.
 *
 * sina_hip_upload_name_order: rank[id] = position of reference id's name in ascending byte-wise order, n = the number
 * of uploaded references.  Anything but a permutation of 0..n_refs-1 is refused before anything runs; a forked context
 * cannot call it; sina_hip_upload_refs (and sina_hip_store_alloc_like) forget it -- sina_hip_upload_refs also forgets
 * the k-mer index and its bitmaps: until the next sina_hip_build_index / sina_hip_upload_index a search fails with "no
 * index", sina_hip_download_index too, and sina_hip_store_view_get shows none.  The identity permutation gives
 * "score descending, id descending", sina_hip_kmer_topk's own tie rule.
 *
 * sina_hip_compare_rank: arguments as sina_hip_compare's (sub-ranges of larger offset arrays included), plus
 *   cand_ids == NULL : every reference of the store, in id order, for every query (cand_off is not read; no id list
 *                      is uploaded)
 *   cover_rule       : SINA_CMP_COVER_* (CMP_COVER_TYPE's order, src/cseq_comparator.h)
 *   max_result       : 1..64 rows per query
 *   out_ids, out_scores : [nq * max_result], row q best first; entries from out_n[q] on are 0
 *   out_n            : [nq] min(max_result, candidates of q minus those left out)
 *   out_flag         : [nq] bit 0: some candidate of q had denom == 0 (the host's 0 / 0 = NaN).  That candidate is
 *                      left out; the caller ranks such a query itself, its rows are unspecified.
 * Scores are the correctly rounded float32 quotient, bit for bit the host's.  A duplicated id in a list is allowed:
 * both copies compete.  Refused with a message, before anything runs and with the outputs untouched: a null argument,
 * a reference id out of range, max_result outside 1..64, an unknown rule, no name order uploaded, a query whose columns
 * do not ascend strictly, a query of more than 65535 bases.  An alignment too wide for the kernel's LDS tables is
 * refused as a limit (sina_hip_last_error_is_limit() == 1).
 *
 * sina_hip_kmer_topk_rank: to sina_hip_compare_rank what sina_hip_kmer_topk_match is to sina_hip_match_count -- the
 * queries as packed aligned bases, the k-mer search sina_hip_kmer_topk_any's for their mask bytes with
 * max = kmer_candidates, and the candidates ranked from the select's id rows where they lie in device memory: no id
 * and no k-mer score crosses the bus.  More than 4096 candidates per query (min(kmer_candidates, n_refs)) are refused as
 * a limit.
 *
 * sina_hip_rank_stats: the rank (and merge) kernels' own time (events around their launches) and volume on this
 * context since init / fork: pairs scored, bases of their candidates, launches. */
#define SINA_CMP_COVER_ABS 0
#define SINA_CMP_COVER_QUERY 1
#define SINA_CMP_COVER_TARGET 2
#define SINA_CMP_COVER_OVERLAP 3
#define SINA_CMP_COVER_ALL 4
#define SINA_CMP_COVER_AVERAGE 5
#define SINA_CMP_COVER_MIN 6
#define SINA_CMP_COVER_MAX 7
#define SINA_CMP_COVER_NOGAP 8
int sina_hip_upload_name_order(sina_hip_ctx *ctx, const uint32_t *rank, uint32_t n);
int sina_hip_compare_rank(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                          const uint32_t *cand_ids, const uint64_t *cand_off, int iupac_rule, int filter_lowercase,
                          int cover_rule, uint32_t max_result, uint32_t *out_ids, float *out_scores, uint32_t *out_n,
                          uint32_t *out_flag);
int sina_hip_kmer_topk_rank(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq,
                            uint32_t kmer_candidates, int iupac_rule, int filter_lowercase, int cover_rule,
                            uint32_t max_result, uint32_t *out_ids, float *out_scores, uint32_t *out_n, uint32_t *out_flag);
int sina_hip_rank_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, uint64_t *cand_bases, uint64_t *launches);

/* ------------------------------------------------------------- helix base-pair score (align_bp_score_slv)
 * The counting behind cseq_base::calcPairScore (src/cseq.cpp:651-733), which Log::printer::operator() calls for every
 * aligned sequence (src/log.cpp:383-385): for every column i the helix map pairs with a column p = pairs[i] != 0, the
 * characters the sequence shows at i and at p -- its base's RNA IUPAC character, '-' where no word holds that column
 * (a partner of 2^24 or more included), '.' for a word without mask bits.  A visit counts unless one side is '.' or
 * both are '-'; of the counted visits the kernel tells the unordered pairs AG, AU, CG, GG, GU of upper-case
 * unambiguous bases apart (every other combination weighs nothing).  The weighted sum and the float division stay
 * with the caller (host/cseq.h, pair_score_from_counts).  The map need not be symmetric, nor as long as the alignment
 * is wide; a symmetric map visits every pair twice and both visits count.
 *
 * sina_hip_upload_pairs: the helix map, pairs[i] = partner column of column i or 0 (unpaired), compacted on the host
 * to the paired columns (csrc/pair_plan.h) and kept with the store: forked contexts see it, a forked context cannot
 * call it, a second upload replaces the first, n == 0 or an all-zero map removes it.  sina_hip_upload_refs leaves it
 * alone.  Not while pair counts are in flight on the store's contexts.
 *
 * sina_hip_pair_counts: nq finished aligned sequences as packed words (q_ab / q_off as sina_hip_match_count takes
 * them, sub-ranges of larger offset arrays included) -> counts [nq][6] = num, AG, AU, CG, GG, GU.  A word's column
 * is found by lower_bound: columns must ascend, equal neighbours are fine (the first of them is the one that is
 * read).  Refused with a message, before anything runs and with counts untouched: a null argument, no map uploaded,
 * offsets or a sequence's columns that descend.  nq == 0 succeeds and touches nothing.  One launch per range of
 * sequences (csrc/pair_plan.h: 2^26 words at most, one sequence at least).
 *
 * sina_hip_pair_stats: the pair-count kernel's own time (events around its launches) and volume on this context since
 * init / fork: sequences counted, map entries visited (sequences x entries), launches. */
int sina_hip_upload_pairs(sina_hip_ctx *ctx, const uint32_t *pairs, uint32_t n);
int sina_hip_pair_counts(sina_hip_ctx *ctx, const uint32_t *q_ab, const uint64_t *q_off, uint32_t nq, uint32_t *counts);
int sina_hip_pair_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, uint64_t *entries_visited,
                        uint64_t *launches);

/* The same six counters where the device assembles the alignment: an align call with p->assemble leaves the finished
 * words of its assembled queries in device memory, and a second kernel queued right behind the assembly counts over
 * them there -- nothing is packed, staged or uploaded again, 24 bytes per query come back with the results.
 *
 * sina_hip_align_count_pairs: the switch, per context, off after init and after fork.  With it on, every align call on
 * this context (sina_hip_align_graphs, _graphs_wsets, _graphs_any, _families, _families_wsets, _profiles) that runs
 * with p->assemble on a store that has a helix map counts: one launch per DP launch range.
 *
 * sina_hip_staged_pair_counts: [nq][6] = num, AG, AU, CG, GG, GU of the context's last align call, laid out like that
 * call's `out`.  Host memory owned by the context, valid until its next align call.  NULL if that call counted nothing:
 * the switch was off, the store had no map, or p->assemble was 0.  Row q is query q's counters where
 * out[q].assembled == 1 -- equal to what sina_hip_pair_counts gives for the same words -- and six zeros elsewhere (a
 * query the host finishes, a failed one, every query of the wide path).
 *
 * sina_hip_pair_inplace_stats: this kernel's own time (events around its launches) and volume on this context since
 * init / fork: assembled queries counted, launches.  sina_hip_pair_stats counts the re-upload route only. */
int sina_hip_align_count_pairs(sina_hip_ctx *ctx, int on);
const uint32_t *sina_hip_staged_pair_counts(sina_hip_ctx *ctx);
int sina_hip_pair_inplace_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, uint64_t *launches);

/* --calc-idty (align_ident_slv) where the device assembles the alignment.  Replaces, for the queries an align call
 * assembles: the comparator of src/align.cpp:380-382 (cseq_comparator(CMP_IUPAC_OPTIMISTIC, CMP_DIST_NONE,
 * CMP_COVER_OVERLAP, false)) and the loop of src/align.cpp:443-453 over the family's members that keeps the best
 * score -- without the second trip of sina_hip_compare (finished words packed and uploaded again, six counters per
 * (query, member) pair downloaded): the finished words, the store's references and the family lists are in device
 * memory when the assembly ends, a kernel queued right behind it scores there, 8 bytes per query come back with the
 * results.
 *
 * sina_hip_align_count_identity: the switch, per context, off after init and after fork.  With it on, every call of
 * sina_hip_align_families, _families_wsets and _profiles on this context that runs with p->assemble counts: one launch
 * per DP launch range.  The sina_hip_align_graphs* entries bring no family to the device and never count.
 *
 * sina_hip_staged_identity: [nq][2] of the context's last align call, laid out like that call's `out`.  Host memory
 * owned by the context, valid until its next align call.  NULL if that call counted nothing: the switch was off,
 * p->assemble was 0, it was a graphs entry, nq was 0, or it ended early.  Where out[q].assembled == 1, word 0 of row q
 * is the bit pattern of the best float score, match / (match + mismatch + only_a + only_b) of sina_hip_compare's
 * counters under SINA_CMP_IUPAC_OPTIMISTIC without the lower-case filter, over the members of query q's family (0 if
 * no member has a score), and word 1 the number of members that have one (a denominator of 0, the host's NaN, has
 * none); align_ident_slv is 100.f * the score.  Two zeros elsewhere (a query the host finishes, a failed one).
 *
 * sina_hip_identity_inplace_stats: this kernel's own time (events around its launches) and volume on this context
 * since init / fork: assembled queries scored, their (query, member) pairs, launches. */
int sina_hip_align_count_identity(sina_hip_ctx *ctx, int on);
const uint32_t *sina_hip_staged_identity(sina_hip_ctx *ctx);
int sina_hip_identity_inplace_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, uint64_t *pairs,
                                    uint64_t *launches);

/* The search stage's ranking (search_filter: k-mer candidates, cseq_comparator::score, the max_result best) where the
 * device assembles the alignment.  Replaces, for the queries an align call assembles, the second trip of
 * sina_hip_kmer_topk_rank -- finished words packed and uploaded again, one k-mer search and one ranking per launch
 * range of that call --: the call's queries are searched once, before its first DP launch range, the id rows stay on
 * the device, and a kernel queued right behind the assembly ranks each query's candidates against the words the
 * assembly has just left.  One row per query comes back with the results.
 *
 * sina_hip_align_rank: the switch, per context, off after init and after fork, and the rules the ranking runs with --
 * the index it expects (k, nofast), kmer_candidates (the search's max; more than 4096 after clamping to the
 * references is refused, as sina_hip_kmer_topk_rank refuses it) and sina_hip_compare_rank's iupac_rule,
 * filter_lowercase, cover_rule and max_result (1..64).  on = 0 ignores the rest.  With it on, a call of
 * sina_hip_align_graphs, _graphs_wsets, _graphs_any, _families, _families_wsets or _profiles on this context ranks if
 * it runs with p->assemble, the store has references, a name order (sina_hip_upload_name_order) and an index of
 * that k / nofast, every query has at most SINA_HIP_MAX_QUERY_LEN bases and the comparison's tables fit the LDS;
 * otherwise the call runs exactly as without the switch.  A missing precondition never fails the align call.
 *
 * sina_hip_staged_rank: [nq][130] of the context's last align call, laid out like that call's `out`.  Host memory
 * owned by the context, valid until its next align call.  NULL if that call did not rank.  Row q: word 0 the number
 * of rows n, word 1 the flags (bit 0: a candidate had a denominator of 0, the host's NaN -- rank that query on the
 * host; bit 1: ranked), words 2..65 the ids, words 66..129 the scores' bit patterns, best first, zero from n on --
 * equal to what sina_hip_kmer_topk_rank gives for the same words.  A query is ranked if out[q].status == 0,
 * out[q].assembled == 1 and out[q].n_out equals its length: the candidates are searched with the input's k-mers,
 * the reference searches with the aligned sequence's, and the two differ once a base was dropped.  Every other row
 * is all zero (bit 1 clear tells "not ranked" from "ranked, no rows").
 *
 * sina_hip_rank_inplace_stats: this kernel's own time (events around its launches) and volume on this context since
 * init / fork: queries ranked, their (query, candidate) pairs, launch ranges.  sina_hip_rank_stats counts the
 * re-upload route only. */
int sina_hip_align_rank(sina_hip_ctx *ctx, int on, unsigned k, int nofast, uint32_t kmer_candidates, int iupac_rule,
                        int filter_lowercase, int cover_rule, uint32_t max_result);
const uint32_t *sina_hip_staged_rank(sina_hip_ctx *ctx);
int sina_hip_rank_inplace_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, uint64_t *pairs,
                                uint64_t *launches);

/* ------------------------------------------------------------- --show-dist: sps, closest relative, cpm (device-dist)
 * The counting behind Log::printer::show_dist (src/log.cpp:279-325) for sequences that arrive aligned: three
 * comparisons per query under cseq_comparator(iupac, CMP_DIST_NONE, CMP_COVER_QUERY, false), the query side first --
 *   self   : the input alignment `orig` against the finished alignment `aligned`, SINA_CMP_IUPAC_EXACT;
 *   before : `orig` against the closest relative, SINA_CMP_IUPAC_OPTIMISTIC;
 *   after  : `aligned` against the same relative, SINA_CMP_IUPAC_OPTIMISTIC
 * -- the closest relative being the member of the query's list that std::sort by result_item::operator< puts last
 * (src/search.h:56-68): the largest score (float)match / (float)(match + mismatch + only_a + only_a_overhang) of
 * `orig` against it, equal scores by the reference's NAME (sina_hip_upload_name_order).  The float scores and cpm stay
 * with the caller (cseq_comparator::score of the counters): only integers come back.
 *
 * sina_hip_show_dist: nq queries.
 *   orig_ab/orig_off : concatenated packed words of the input alignments, offsets [nq+1] (as sina_hip_compare's q_ab /
 *                      q_off; sub-ranges of larger offset arrays included)
 *   al_ab/al_off     : the same for the finished alignments
 *   ref_ids/ref_off  : concatenated reference ids of the queries' relatives -- a family or a search result, in any
 *                      order --, offsets [nq+1]; ref_ids may be NULL if every list is empty
 *   rows             : [nq][20] 32-bit words: 0..5 self, 6..11 before, 12..17 after (each in sina_hip_match_counts'
 *                      order), 18 the closest relative's id or 0xFFFFFFFF, 19 flags -- bit 0: a member of the list had
 *                      a denominator of 0 (the host's NaN; it is left out: the caller walks that query itself), bit 1:
 *                      the row was computed.  Without a closest relative (an empty list, or every member left out)
 *                      before and after are zero.
 * A duplicated id in a list is allowed.  Refused with a message, before anything runs and with rows untouched: a null
 * argument, a reference id out of range, no name order uploaded, offsets that descend, an orig or aligned of more than
 * 65535 bases or whose columns do not ascend strictly.  An alignment too wide for the kernel's LDS tables is refused as
 * a limit (sina_hip_last_error_is_limit() == 1).  nq == 0 succeeds and touches nothing.  One launch per range of
 * queries (csrc/showdist_plan.h).
 *
 * sina_hip_show_dist_stats: the kernel's own time (events around its launches) and volume on this context since init /
 * fork: queries scored, (orig, member) pairs compared, launches. */
int sina_hip_show_dist(sina_hip_ctx *ctx, const uint32_t *orig_ab, const uint64_t *orig_off, const uint32_t *al_ab,
                       const uint64_t *al_off, uint32_t nq, const uint32_t *ref_ids, const uint64_t *ref_off, uint32_t *rows);
int sina_hip_show_dist_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *sequences, uint64_t *pairs, uint64_t *launches);

/* ------------------------------------------------------------- the aligner's exact-relative test (device-copy)
 * boost::icontains / ifind_first of the query's unaligned bases in a family member's (src/align.cpp:329-388), for
 * every (query, reference) pair of a batch.  Upper-cased characters of two bases are equal exactly when the four base
 * bits of their masks are (T and U share a code, bit 4 is the case), so the device compares `mask & 0xF` for EQUALITY:
 * a query N does not match a reference A.
 *
 * sina_hip_find_bases: nq queries.
 *   qmask/q_off       : concatenated mask bytes of the queries, one per base (as sina_hip_kmer_topk takes them),
 *                       offsets [nq+1]; sub-ranges of larger offset arrays included
 *   cand_ids/cand_off : concatenated reference ids of the queries' candidates, offsets [nq+1] (as
 *                       sina_hip_match_count's)
 *   out_at            : out_at[cand_off[q] + i] belongs to candidate i of query q: std::string::find's answer -- the
 *                       lowest start, in bases of the reference, at which the reference holds the query's n bases, or
 *                       0xFFFFFFFF without one or with more query bases than reference bases.  "The reference IS the
 *                       query" is at == 0 with equal lengths.
 * The call blocks until out_at is written.  Refused with a message, before anything runs and with out_at untouched:
 * a null argument, no references uploaded, a reference id out of range, offsets that descend, a query of 0 or of more
 * than 65535 bases.  cand_off[nq] == cand_off[0] succeeds and launches nothing.  One launch per range of pairs
 * (csrc/contain_plan.h).
 *
 * sina_hip_find_bases_stats: the kernel's own time (events around its launches) and volume on this context since init /
 * fork: pairs answered, bases of their references, launches. */
int sina_hip_find_bases(sina_hip_ctx *ctx, const uint8_t *qmask, const uint64_t *q_off, uint32_t nq,
                        const uint32_t *cand_ids, const uint64_t *cand_off, uint32_t *out_at);
int sina_hip_find_bases_stats(sina_hip_ctx *ctx, double *kernel_ms, uint64_t *pairs, uint64_t *ref_bases,
                              uint64_t *launches);

/* ------------------------------------------------------------- alignment
 * Replaces, for a batch of queries: mseq::mseq + sort + reduce_edges
 * (src/mseq.cpp:47-118, src/graph.h:451-488) when given family ids, compute()
 * with compute_node_simple<transition_simple|transition_aspace_aware> over
 * scoring_scheme_simple|weighted (src/mesh.h:263-528, src/scoring_schemes.h:
 * 102-241) and the walk of backtrack() (src/mesh.h:535-721).
 */
enum { SINA_OVERHANG_ATTACH = 0, SINA_OVERHANG_REMOVE = 1, SINA_OVERHANG_EDGE = 2 };
enum { SINA_LOWERCASE_NONE = 0, SINA_LOWERCASE_ORIGINAL = 1, SINA_LOWERCASE_UNALIGNED = 2 };
enum { SINA_INSERTION_SHIFT = 0, SINA_INSERTION_FORBID = 1, SINA_INSERTION_REMOVE = 2 };

typedef struct sina_hip_align_params {
    float match_score;      /* --match-score    (2)  src/align.cpp:250-252 */
    float mismatch_score;   /* --mismatch-score (-1) */
    float gap_penalty;      /* --pen-gap        (5)  */
    float gap_ext_penalty;  /* --pen-gapext     (2)  */
    float fs_weight;        /* --fs-weight      (1)  src/align.cpp:247-249 */
    int32_t overhang;       /* SINA_OVERHANG_*  */
    int32_t lowercase;      /* SINA_LOWERCASE_* */
    int32_t insertion;      /* SINA_INSERTION_* */
    const float *weights;   /* posvar weights => scoring_scheme_weighted, or NULL (the _wsets entries: n_sets vectors) */
    uint32_t n_weights;
    int32_t assemble;       /* 1: also do the cseq container steps of backtrack() on the device where they
                             * are plain (see sina_hip_align_out::assembled); 0 (default): columns only;
                             * 2 (SINA_ASSEMBLE_SHIFT): 1 plus the insertions that shift their neighbours */
} sina_hip_align_params;
void sina_hip_align_params_default(sina_hip_align_params *p);

/* assemble == SINA_ASSEMBLE_SHIFT: what assemble == 1 does, and an insertion that does not fit the free columns in
 * front of the next base is placed by the reference's widening loop (cseq_base::fix_duplicate_positions,
 * src/cseq.cpp:503-570): the range grows towards the nearer free column, left on a tie, and takes the bases it passes
 * along -- a later run of duplicates the right scan walks through included.  Every base so placed is lower-cased under
 * SINA_LOWERCASE_UNALIGNED; nast_total / nast_longest count the widened runs, nast_last_run the last run before its
 * widening.  It holds for every entry of the fast path (sina_hip_align_graphs, _graphs_wsets, _graphs_any for the
 * queries it routes there, _families, _families_wsets, _profiles); the wide path assembles nothing, as before.
 * Still left to the host (assembled = 0, out_pos as the walk wrote it): more than SINA_HIP_SHIFT_LOG shifted runs in
 * one query, no free column on either side (the reference throws), a column at or beyond the width -- appended, or
 * taken for free by a widening that reaches the last base in column width - 1 --, more than 4096 bases.
 *
 * sina_hip_staged_shift_log: [nq][1 + 3 * SINA_HIP_SHIFT_LOG] words of the context's last align call, laid out like
 * that call's `out`: word 0 of row q is the number of shifted runs of query q, then {N, B, E} per run in sequence
 * order -- the reference's "shifting bases to fit in N bases at pos B to E;", written before the run is widened.
 * Host memory owned by the context, valid until its next align call; NULL unless that call ran with assemble == 2.
 * A query with assembled == 0 has no events.
 *
 * sina_hip_assemble_stats: since init / fork, over the fast path's launches that ran with assemble != 0: their
 * queries, those the device assembled, and of these the queries with at least one shifted run and their shifted runs.
 *
 * sina_hip_debug_assemble (test hook): the assembly alone, on columns the caller made.  out[q] comes in with n_out,
 * end_s, cutoff_head, cutoff_tail, aligned_bases and status, out_pos (laid out by qoff like qmask) with the columns as
 * handed to cseq::append; both go out as after an align call with these params (p->assemble 1 or 2), and the shift log
 * is staged.  n_out may not exceed the query's length, and end_s + the kept tail overhang must name a base of the
 * query at least n_out - 1 from its start: the call fails otherwise, nothing is read out of bounds.
 * sina_hip_debug_assemble_ms: the kernel's own time in the context's last sina_hip_debug_assemble call (events
 * around its launch; 0 before the first) -- what tools/perf_shift.py compares the two instantiations with. */
#define SINA_ASSEMBLE_SHIFT 2
#define SINA_HIP_SHIFT_LOG 32u
const uint32_t *sina_hip_staged_shift_log(sina_hip_ctx *ctx);
int sina_hip_assemble_stats(sina_hip_ctx *ctx, uint64_t *queries, uint64_t *assembled, uint64_t *shifted_queries,
                            uint64_t *shifted_runs);
/* The aligned columns of the context's last sina_hip_align_graphs / sina_hip_align_families call, laid out like
 * that call's out_pos with qoff[0] taken as 0 (query q's entries start at qoff[q] - qoff[0]).  Host memory owned
 * by the context; valid until the next align call on this context (or its destruction). */
const uint32_t *sina_hip_staged_out_pos(sina_hip_ctx *ctx);

/* Longest query (bases) the fast paths take: sina_hip_kmer_topk / sina_hip_kmer_scores, family and profile
 * alignment, sina_hip_align_graphs.  (The fast k-mer count kernel keeps a query's k-mer cursors in LDS beside its
 * 64 KiB score tile: 9 bytes per base; the fast DP kernel's trace-back cell has 14 bits for the query index.)  The
 * reference aligns any length (src/mesh.h:76,119-121): sina_hip_kmer_topk_any / sina_hip_kmer_scores_any search
 * queries of up to SINA_HIP_MAX_LONG_QUERY_LEN bases and sina_hip_align_graphs_any aligns them; the stage functors
 * fail a query beyond the limit their options leave softly, alone (famfinder `long-queries`, aligner
 * `wide-fallback`). */
#define SINA_HIP_MAX_QUERY_LEN 10240u

/* Longest query (bases) the k-mer search takes at all (the _any entries).  A k-mer score is an int16_t -- in the
 * reference too, unguarded (src/idset.h:315-337): a reference that holds all k-mers of a longer query would wrap
 * there --, and the count kernels' LDS counters are 16-bit halves of a word.  A longer query is refused with
 * sina_hip_last_error_is_limit() == 1; nothing is truncated. */
#define SINA_HIP_MAX_LONG_QUERY_LEN 32767u
/* The long count kernel takes a query's k-mer windows (by the index of their last base) in chunks of this many. */
#define SINA_HIP_KMER_LONG_CHUNK 10240u

/* A batch of family DAGs in CSR form (node id == topological rank == mesh row).
 * All arrays are concatenated over the nq queries of the batch.  Limits of sina_hip_align_graphs (the call fails,
 * nothing is truncated; sina_hip_align_graphs_any has none of the first three): at most 65535 nodes per DAG, at most
 * 255 predecessors per node, queries of 1..SINA_HIP_MAX_QUERY_LEN bases; every predecessor id smaller than its
 * node's id. */
typedef struct sina_hip_graph_batch {
    uint32_t nq;
    const uint64_t *node_off;  /* [nq+1] into the node arrays                      */
    const uint64_t *edge_off;  /* [nq+1] into pred                                 */
    const uint32_t *node_pos;  /* alignment column of each node                    */
    const uint8_t *node_mask;  /* iupac mask of each node                          */
    const float *node_weight;  /* mseq_node::weight (src/mseq.cpp:113)             */
    const uint32_t *pred_off;  /* per query N+1 entries, relative to edge_off[q];
                                  stored at node_off[q] + q                        */
    const uint32_t *pred;      /* predecessor node ids, ascending per node         */
    const uint32_t *succ_minpos; /* min column over successors, 1000000 if none
                                  (src/mesh.h:480-484); may be NULL unless FORBID  */
    uint32_t width;            /* alignment width (mseq::getWidth)                 */
    /* --fs-no-graph (src/pseq.{h,cpp}, scoring_scheme_profile src/scoring_schemes.h:37-100): the family
     * as a profile -- one node per column, every node's one predecessor the node before it -- whose
     * match term is base_profile::comp(node, query base) instead of (mask & base) ? match : mismatch.
     * node_score16[16 * node + m]: that term for a query base with iupac mask m (1..15; entry 0 unused),
     * self_score16[m]: comp of a base's own profile with itself (the sum_weight term of backtrack(),
     * src/mesh.h:631-638).  Both NULL (the default) for DAG batches; node_mask / node_weight are
     * ignored when they are set. */
    const float *node_score16;
    const float *self_score16;
} sina_hip_graph_batch;

/* Per-query result of DP + backtrack walk, before the cseq container steps
 * (append rule, setWidth, reverse, fix_duplicate_positions) that the host-side
 * aligner applies (src/mesh.h:723-726). */
typedef struct sina_hip_align_out {
    uint32_t end_m, end_s;   /* start cell of the backtrack (src/mesh.h:567-592)   */
    float raw;               /* value at the end cell  (rval, :618)                */
    float sum_weight;        /* (:621,637,683)                                     */
    int32_t aligned_bases;   /* (:622)                                             */
    int32_t cutoff_head, cutoff_tail;
    uint32_t n_out;          /* number of appended bases written to pos[]          */
    int32_t status;          /* 0 ok; <0 device-side failure                       */
    /* With sina_hip_align_params::assemble: 1 if out_pos holds this query's FINISHED alignment -- n_out
     * packed aligned_base words (column | iupac mask << 24, case bit included) in sequence order,
     * after the append rule, setWidth, reverse and the NAST fix-up (src/mesh.h:603-726,
     * src/cseq.cpp:456-594) -- and the fix-up's log facts below; 0 if out_pos holds the appended
     * columns as without the switch (an insertion that does not fit its gap and makes neighbours
     * move, a column beyond the alignment, more than 4096 bases: the host finishes those; with
     * assemble == SINA_ASSEMBLE_SHIFT the first of these is the device's too, see there). */
    uint32_t assembled;
    uint32_t nast_total, nast_longest, nast_last_run; /* "total inserted bases", "longest insertion",
                                                        * "total inserted bases before shifting"     */
} sina_hip_align_out;

/* Aligns nq queries (upper-cased or not is the caller's business: masks are
 * used as given) against their DAGs.
 *   qmask/qoff : concatenated query iupac masks, offsets [nq+1]
 *   out        : [nq]
 *   out_pos    : concatenated like qmask; for query q, out_pos[qoff[q] + i] is
 *                the column handed to the i-th cseq::append() call of
 *                backtrack() (i.e. in reverse query order, tail overhang first) --
 *                or, with p->assemble and out[q].assembled, the finished alignment.
 *                May be NULL: the columns then stay where the device copied them, in the context's
 *                pinned staging buffer -- see sina_hip_staged_out_pos (spares a 6 KB copy per 16S query).
 */
int sina_hip_align_graphs(sina_hip_ctx *ctx, const sina_hip_graph_batch *g, const uint8_t *qmask,
                          const uint64_t *qoff, const sina_hip_align_params *p,
                          sina_hip_align_out *out, uint32_t *out_pos);

/* Same arguments and result layout (out_pos == NULL and sina_hip_staged_out_pos included), without the limits of the
 * fast path: any number of nodes, any number of predecessors per node, any query of at least one base -- what the
 * reference takes (src/mesh.h:76,119-121).  Routing is per query: a query the fast path can take runs there, its
 * results bit for bit those of sina_hip_align_graphs; the others -- more than 65535 nodes, a node of more than 255
 * predecessors, more than SINA_HIP_MAX_QUERY_LEN bases, more rows with far-away successors than the fast kernel keeps
 * -- go through the wide kernel: the reference's mesh, 28 bytes per cell (--insertion=forbid: 32) in device memory,
 * one workgroup per query.  Those queries are never assembled (assembled = 0 whatever p->assemble says).  The wide
 * kernel's launches hold at most SINA_HIP_WIDE_CELLS cells (of a diagonal-major mesh: (N + L - 1) * min(N, L) per
 * query, 16 GiB of planes at most); a single query beyond that fails the call with a message that names the bytes
 * it needs, nothing is truncated.  Malformed input -- a predecessor id not smaller than its node's, pred_off not
 * ascending -- is an error as before. */
#define SINA_HIP_WIDE_CELLS ((uint64_t)1 << 29)
int sina_hip_align_graphs_any(sina_hip_ctx *ctx, const sina_hip_graph_batch *g, const uint8_t *qmask,
                              const uint64_t *qoff, const sina_hip_align_params *p,
                              sina_hip_align_out *out, uint32_t *out_pos);
/* Number of queries the wide kernel has aligned on this context since sina_hip_init / sina_hip_fork. */
int sina_hip_wide_queries(sina_hip_ctx *ctx, uint64_t *n);

/* Same, but the DAGs are built on the GPU from family member ids into the
 * uploaded reference store (order of ids = family order = mseq input order).
 *   fam_ids/fam_off : concatenated reference ids, offsets [nq+1]
 * A column's nodes are keyed by the base's character, as mseq keys them (src/mseq.cpp:92-96): iupac masks 0 and 16
 * are both '.' and share a node, which keeps the mask of the first member to show it.  A family whose members hold no
 * base at all has no DAG: the call fails ("a family without a single base") before anything is launched.
 */
int sina_hip_align_families(sina_hip_ctx *ctx, const uint32_t *fam_ids, const uint64_t *fam_off,
                            uint32_t nq, const uint8_t *qmask, const uint64_t *qoff,
                            const sina_hip_align_params *p, sina_hip_align_out *out,
                            uint32_t *out_pos);

/* sina_hip_align_graphs / sina_hip_align_families with a positional weight vector PER QUERY, in one launch: the
 * reference weights every query with the filter of the group most of its relatives belong to (--auto-filter-field,
 * src/famfinder.cpp:397-429), so the queries of one batch may differ in theirs.
 *   p->weights : n_sets vectors of p->n_weights floats, one after the other (required: n_sets >= 1 vectors)
 *   weight_set : [nq] weight_set[q] < n_sets names query q's vector; NULL: every query takes the first
 * Everything else -- arguments, limits, refusals, result layout, out_pos == NULL with the staged columns, assemble --
 * is as for the entry without the suffix, and with n_sets == 1 or weight_set == NULL its bytes are returned.  A
 * vector's last entry stands for every column beyond it, within the query's own vector.  A set id that is not below
 * n_sets fails the call before anything runs (not a limit: sina_hip_last_error_is_limit() == 0); a profile batch
 * (node_score16) takes no weights and so no sets.  Queries with the same ordered family still share one DAG -- it
 * holds no positional weights -- and each reads its own vector.  sina_hip_align_graphs_any and
 * sina_hip_align_profiles keep one vector per call. */
int sina_hip_align_graphs_wsets(sina_hip_ctx *ctx, const sina_hip_graph_batch *g, const uint8_t *qmask,
                                const uint64_t *qoff, const sina_hip_align_params *p, const uint32_t *weight_set,
                                uint32_t n_sets, sina_hip_align_out *out, uint32_t *out_pos);
int sina_hip_align_families_wsets(sina_hip_ctx *ctx, const uint32_t *fam_ids, const uint64_t *fam_off,
                                  uint32_t nq, const uint8_t *qmask, const uint64_t *qoff,
                                  const sina_hip_align_params *p, const uint32_t *weight_set, uint32_t n_sets,
                                  sina_hip_align_out *out, uint32_t *out_pos);

/* Same, but the family is the template as a PROFILE (--fs-no-graph: pseq p(vcp.begin(), vcp.end()) and
 * scoring_scheme_profile, src/align.cpp:428-433; src/pseq.cpp, base_profile and base_profile::comp,
 * src/pseq.h:65-113), built on the GPU from the member ids: one node for column 0 and one per occupied column,
 * a chain; per node the match term of every query iupac mask.  Arguments, limits and refusals as for
 * sina_hip_align_families (1..128 members, every id in the store, references uploaded first, width at most
 * 524288); a profile of more than 65535 nodes fails the call like an oversized DAG.  p->weights must be NULL / 0
 * (scoring_scheme_profile takes no positional weights), p->fs_weight is ignored.  out / out_pos are byte for byte
 * what sina_hip_align_graphs returns for the same families given as node_score16 / self_score16 tables.
 * One input is outside that promise, as it is outside the reference's arithmetic: a column in which EVERY member
 * has a base without any of the four base bits has no points at all, its shares are 0 / 0, and the NaN the device
 * writes there need not have the bit pattern of the host's (both are NaN; reference stores hold no such bases). */
int sina_hip_align_profiles(sina_hip_ctx *ctx, const uint32_t *fam_ids, const uint64_t *fam_off,
                            uint32_t nq, const uint8_t *qmask, const uint64_t *qoff,
                            const sina_hip_align_params *p, sina_hip_align_out *out,
                            uint32_t *out_pos);

/* Test hook: DP planes of ONE query for bit-exact comparison with the oracle.
 * tb_vm/tb_vs: [N*L] value_midx / value_sidx; value: [N*L] float (may be NULL).
 * prune: 0 = every row of every strip is swept (the planes are the reference's cell for cell), 1 = the launch as
 * production makes it, certified row skip included (cells it proved irrelevant hold what it left there). */
int sina_hip_debug_mesh(sina_hip_ctx *ctx, const sina_hip_graph_batch *g, const uint8_t *qmask,
                        uint32_t qlen, const sina_hip_align_params *p, uint32_t *tb_vm,
                        uint32_t *tb_vs, float *value, int prune);

/* Test hook, the twin of sina_hip_debug_mesh for the wide kernel: its planes of ONE query (any size the wide path's
 * budget holds), [N*L] row-major; value may be NULL. */
int sina_hip_debug_mesh_wide(sina_hip_ctx *ctx, const sina_hip_graph_batch *g, const uint8_t *qmask,
                             uint32_t qlen, const sina_hip_align_params *p, uint32_t *tb_vm,
                             uint32_t *tb_vs, float *value);

/* Test hook: assemble_kernel alone on caller-made emitted columns -- see SINA_ASSEMBLE_SHIFT above. */
int sina_hip_debug_assemble(sina_hip_ctx *ctx, const sina_hip_align_params *p, uint32_t width, const uint8_t *qmask,
                            const uint64_t *qoff, uint32_t nq, sina_hip_align_out *out, uint32_t *out_pos);
int sina_hip_debug_assemble_ms(sina_hip_ctx *ctx, double *kernel_ms);

/* Test hooks for the certified row skip: what the DP kernel reported for query q of the context's LAST launch
 * (attempts 0: that launch swept everything), and the first n entries of the per-node bound R(m) the last launch /
 * the last sina_hip_debug_family_graph left on the device (units of 1/64; entry i belongs to node i of the launch's
 * first DAG) with C(m), the number of occupied columns right of the node's.  prune_step = the largest gain of one
 * match step the launch assumed, prune_gmin = the smallest column maximum of query q's DAG, same units.
 * kernel = which DP kernel the launch ran: the specialised one, without or with the row skip, or the generic kernel's
 * instance (simple scheme below / not below the initial value, positional weights, insertion=forbid, both). */
#define SINA_DP_KERNEL_NONE 0u
#define SINA_DP_KERNEL_SIMPLE 1u
#define SINA_DP_KERNEL_SIMPLE_SKIP 2u
#define SINA_DP_KERNEL_GENERIC_BELOW 3u
#define SINA_DP_KERNEL_GENERIC 4u
#define SINA_DP_KERNEL_WEIGHTED 5u
#define SINA_DP_KERNEL_FORBID 6u
#define SINA_DP_KERNEL_WEIGHTED_FORBID 7u
typedef struct sina_hip_dp_info {
    uint32_t end_m, end_s;
    float raw;
    int32_t status;
    uint32_t rows_swept, cells_swept, attempts;
    float gain0, ubound;
    uint32_t prune_step, prune_gmin;
    float scout;  /* what the scout pass found for this query (the first attempt's bound U; +inf: the band never met the
                   * query's last column); NaN: the launch had none */
    uint32_t kernel;  /* SINA_DP_KERNEL_* of the context's last launch */
} sina_hip_dp_info;
int sina_hip_debug_dp_info(sina_hip_ctx *ctx, uint32_t q, sina_hip_dp_info *out);
int sina_hip_debug_rgain(sina_hip_ctx *ctx, uint32_t n, uint32_t *out, uint32_t *cols_right /* C(m), may be NULL */);
/* Test hook for the scout pass: the chain the last DAG build (a launch's, or sina_hip_debug_family_graph's) left for its
 * FIRST DAG -- the node of every base of the family's first member, in base order.  *len: the member's bases; the
 * first min(*len, cap) node ids go to out. */
int sina_hip_debug_chain_rows(sina_hip_ctx *ctx, uint16_t *out, uint32_t cap, uint32_t *len);

/* Test hook: the DAG the GPU builds for ONE family (ids into the uploaded store, in family
 * order), in compact CSR form, for comparison with mseq (src/mseq.cpp:47-118).
 * ring_depth is the number of LDS row slots the DP kernel will have; spill_idx reports where each
 * finished DP row is kept: 0xFFFFFFFF nowhere, slot number, or 0x80000000 | spill row. */
int sina_hip_debug_family_graph(sina_hip_ctx *ctx, const uint32_t *fam_ids, uint32_t F, float fs_weight,
                                uint32_t ring_depth, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *pos,
                                uint8_t *mask, float *weight, uint32_t *pred_off, uint32_t *pred,
                                uint32_t *succ_minpos, uint8_t *sink, uint32_t *spill_idx, uint32_t cap_nodes,
                                uint32_t cap_edges);
/* Test hook: the same build, read back as the words the DP kernel is handed, unchanged: per node the row record's z
 * (predecessors | iupac mask << 8 | sink << 16 | fence << 17 | min(distance to the furthest predecessor, 63) << 18 |
 * (index of the first spilled predecessor + 1) << 24) and w (where the finished row is kept), the predecessor entries
 * node by node (id | (LDS slot or spill row & 0x7fff) << 16 | spilled << 31) and the build's 8 size words (nodes, raw
 * edge entries, spill rows, status, first sink row, smallest column gain, bases of the first member; the eighth is not used). */
int sina_hip_debug_family_graph_words(sina_hip_ctx *ctx, const uint32_t *fam_ids, uint32_t F, float fs_weight,
                                      uint32_t ring_depth, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *rec_z,
                                      uint32_t *rec_w, uint32_t *pred_entries, uint32_t *size_words /* [8] */,
                                      uint32_t cap_nodes, uint32_t cap_edges);

/* Test hook: the profile the GPU builds for ONE family (ids into the uploaded store, in family order), for
 * comparison with pseq (src/pseq.cpp) and base_profile::comp (src/pseq.h:100-113): the nodes' columns, the
 * [n_nodes][16] table of match terms (entry 0 of a row: +inf) and the 16 self-comparison terms.  match,
 * mismatch, gap, gap_ext are the SCHEME's arguments (-match_score, -mismatch_score, pen_gap, pen_gapext,
 * src/align.cpp:428-433).  The node counters of up to 6144 nodes are in LDS at a time (fewer for alignments of
 * more than ~300 000 columns); a longer profile is swept in several tiles (SINA_HIP_TEST=profile_tile=N, tests
 * only: tiles of at most N nodes).  The arrays start with room for 4096 nodes and keep the largest size a build of
 * the context has needed; a family with more nodes has the kernel launched again, which counts as ONE launch in
 * sina_hip_stats.  A column whose only bases have none of the four base bits has shares of 0 / 0. */
int sina_hip_debug_family_profile(sina_hip_ctx *ctx, const uint32_t *fam_ids, uint32_t F, float match,
                                  float mismatch, float gap, float gap_ext, uint32_t *n_nodes, uint32_t *pos,
                                  float *score16, float *self16, uint32_t cap_nodes);
/* Test hook: the same build, read back as the chain the DP kernel is handed, unchanged: per node the row record's four
 * words (index of its predecessor entry; node weight and mask, 0; predecessors | sink << 16 | min(distance to the
 * predecessor, 63: none) << 18; where the finished row is kept, 0xFFFFFFFF: handed on in registers) and the
 * successor's column (1000000 on the last node), the n_nodes - 1 predecessor entries (entry n: node n + 1's, = n) and
 * the build's 8 size words (nodes, edges, spill rows 0, status 0, first sink row, 0; the last two are not used). */
int sina_hip_debug_family_profile_words(sina_hip_ctx *ctx, const uint32_t *fam_ids, uint32_t F, uint32_t *n_nodes,
                                        uint32_t *rec_words /* [4 * cap_nodes] */, uint32_t *succ_min,
                                        uint32_t *pred_entries, uint32_t *size_words /* [8] */, uint32_t cap_nodes);

/* Cumulative statistics of this context and its forks since sina_hip_init (callers take
 * differences); kernel times come from HIP events on the context stream. */
typedef struct sina_hip_stats {
    double dp_ms;          /* mesh DP fill kernel(s)                  */
    double backtrack_ms;   /* backtrack walk kernel                   */
    double graph_ms;       /* device DAG build, device profile build  */
    double kmer_count_ms;  /* k-mer count kernel                      */
    double kmer_select_ms; /* top-k select kernel                     */
    uint64_t dp_cells;     /* sum of N*L over the batch               */
    uint64_t postings;     /* postings visited by the count kernel    */
    uint32_t dp_launches, kmer_launches;
    double compare_ms;       /* search-stage comparison kernel            */
    uint64_t compare_bases;  /* candidate bases streamed by it            */
    uint32_t compare_launches;
    uint32_t n_dense_lists;  /* gauge, not cumulative: posting lists the index currently also holds as
                                reference bitmaps (0 until the first search after an index change) */
    double dp_busy_ms;       /* time during which a DP kernel was resident: dp_ms minus the time a launch shared
                                the device with the launch before it (a DP launch starts when its predecessor
                                has dispatched its last workgroup, not when it has ended)                     */
    uint64_t dags_built;     /* family DAGs -- and family profiles (sina_hip_align_profiles) -- built on the device ... */
    uint64_t dags_used;      /* ... and queries aligned against them (queries with the same ordered family share one) */
    /* Certified row skip of the DP kernel (the reference fills every cell, src/mesh.h:512-528; here a row of a
     * 512-column strip whose every input provably exceeds what any path ending at the optimum can hold is not
     * swept -- the end cell, its value and the whole trace-back path are certified identical, or the query is
     * swept again): dp_cells above stays the NOMINAL N*L. */
    uint64_t dp_rows;            /* (row, strip) pairs of the launches, nominal                                  */
    uint64_t dp_rows_swept;      /* ... actually swept, second and third attempts included                       */
    uint64_t dp_cells_swept;     /* cells actually computed (= dp_cells where nothing was skipped)               */
    uint64_t dp_queries_pruned;  /* queries that went through the skipping kernel ...                            */
    uint64_t dp_second_attempts; /* ... whose first bound failed its certificate (swept again under the bound the
                                    first attempt found) ...                                                      */
    uint64_t dp_full_sweeps;     /* ... and whose second did too (swept in full)                                 */
    double dp_prune_rho;         /* gauge: the guess (optimum / bound on the whole gain) the next launch starts with */
    uint64_t graph_bytes;        /* device DAG build, algorithmic bytes: the families' packed bases read once, the DAGs
                                    (row records, columns, row-skip bounds, predecessor lists) written once; a device
                                    profile build counts the same way (its nodes carry 64 bytes of match terms each) */
    uint32_t graph_launches, kmer_queries; /* DAG-build and profile-build launches; queries searched by the k-mer count kernel */
    double scout_ms;             /* always 0: the scout pass (a bound on the optimum per query from a banded sweep) is the
                                    first thing a DP wave does and has no time of its own (kept: the struct's layout)  */
    uint32_t scout_launches, pad_; /* DP launches whose waves ran the scout pass */
} sina_hip_stats;
int sina_hip_get_stats(sina_hip_ctx *ctx, sina_hip_stats *s);

#ifdef __cplusplus
}
#endif
#endif /* SINA_HIP_H */
