// The family as the DP reads it, built on the host: build_family_graph (the DAG) and build_family_profile
// (--fs-no-graph) -- the twins of the device builders, for the aligner's host-graph route and the tests.
#include "stages.h"

#include <algorithm>
#include <limits>
#include <stdexcept>

namespace sina {

// ================================================================ host DAG build

// src/mseq.cpp:47-118 + src/graph.h:332-357,466-488, flat arrays.
// ---- --fs-no-graph: pseq + scoring_scheme_profile (src/pseq.{h,cpp}, src/scoring_schemes.h:37-100)
namespace {
struct base_shares {  // base_profile: shares of A, G, C, T/U, opened gaps, extended gaps in a column
    float v[6];
};
base_shares shares_of_base(unsigned mask) {  // base_profile(const base_iupac&), pseq.h:65-86
    base_shares b{};
    const int order = __builtin_popcount(mask & 0xfu);
    if (order > 0) {
        const float val = 1.f / (float)order;
        for (int i = 0; i < 4; i++)
            if (mask & (1u << i)) b.v[i] = val;
    }
    return b;
}
// base_profile::comp, pseq.h:100-113: sixteen products in i-outer, j-inner order, then the gap terms
float profile_comp(const base_shares &a, const base_shares &b, float match, float mismatch, float gap, float gap_ext) {
    float res = 0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            if (i == j) res += match * a.v[i] * b.v[j];
            else res += mismatch * a.v[i] * b.v[j];
        }
    return res + gap * a.v[4] + gap_ext * a.v[5];
}
}  // namespace

void profile_self_scores(float match, float mismatch, float gap, float gap_ext, float *out16) {
    out16[0] = 0.f;
    for (unsigned m = 1; m < 16; m++) {
        const base_shares b = shares_of_base(m);
        out16[m] = profile_comp(b, b, match, mismatch, gap, gap_ext);
    }
}

void build_family_profile(const std::vector<const cseq *> &fam, float match, float mismatch, float gap, float gap_ext,
                          host_graph *g) {
    const size_t F = fam.size();
    g->pos.clear(); g->mask.clear(); g->weight.clear(); g->score16.clear();
    g->pred_off.assign(1, 0); g->pred.clear(); g->succ_minpos.clear();
    g->width = F ? fam[0]->getWidth() : 0;
    std::vector<uint32_t> at(F, 0);   // next unread base of every member
    std::vector<char> in_gap(F, 1);   // (a member's leading gap counts as extended)
    base_shares code[16];
    for (unsigned m = 0; m < 16; m++) code[m] = shares_of_base(m);
    uint32_t column = 0;
    while (column < g->width) {  // column 0 first, occupied or not; then from occupied column to occupied column
        uint32_t next = g->width;
        int cnt[4] = {0, 0, 0, 0}, opened = 0, extended = 0;
        for (size_t j = 0; j < F; j++) {
            const auto &b = fam[j]->getAlignedBases();
            if (at[j] < b.size() && b[at[j]].getPosition() == column) {
                const unsigned mask = (b[at[j]].raw >> 24) & 0xfu;
                const int order = __builtin_popcount(mask);
                if (order > 0) {
                    const int points = 12 / order;
                    for (int i = 0; i < 4; i++)
                        if (mask & (1u << i)) cnt[i] += points;
                    in_gap[j] = 0;
                }
                ++at[j];
            } else if (in_gap[j]) {
                ++extended;
            } else {
                in_gap[j] = 1;
                ++opened;
            }
            if (at[j] < b.size()) next = std::min(next, (uint32_t)b[at[j]].getPosition());
        }
        base_shares col;
        {
            const int open = opened * 12, ext = extended * 12;
            const int sum = cnt[0] + cnt[1] + cnt[2] + cnt[3] + open + ext;
            for (int i = 0; i < 4; i++) col.v[i] = (float)cnt[i] / sum;
            col.v[4] = (float)open / sum;
            col.v[5] = (float)ext / sum;
        }
        const uint32_t node = (uint32_t)g->pos.size();
        g->pos.push_back(column);
        g->mask.push_back(0);
        g->weight.push_back(0.f);
        g->score16.push_back(std::numeric_limits<float>::infinity());  // (mask 0: no query base has it)
        for (unsigned m = 1; m < 16; m++) g->score16.push_back(profile_comp(col, code[m], match, mismatch, gap, gap_ext));
        if (node > 0) g->pred.push_back(node - 1);
        g->pred_off.push_back((uint32_t)g->pred.size());
        column = next;
    }
    // successor minima (for --insertion=forbid): the next node's column, 1000000 behind the last (mesh.h:480-484)
    const size_t N = g->pos.size();
    g->succ_minpos.resize(N);
    for (size_t m = 0; m < N; m++) g->succ_minpos[m] = m + 1 < N ? g->pos[m + 1] : 1000000u;
}

void build_family_graph(const std::vector<const cseq *> &fam, float fs_weight, host_graph *g) {
    const size_t F = fam.size();
    g->pos.clear(); g->mask.clear(); g->weight.clear();
    g->pred_off.assign(1, 0); g->pred.clear(); g->succ_minpos.clear();
    g->width = F ? fam[0]->getWidth() : 0;
    for (const cseq *c : fam)
        if (c->getWidth() != g->width)
            throw std::runtime_error("Aligned sequences to be stored in mseq of differ in length!");
    std::vector<uint32_t> cur(F, 0);
    std::vector<int32_t> last(F, -1);
    std::vector<float> count;
    struct ed { uint32_t b, a; };
    std::vector<ed> col_edges;
    int32_t node_of_mask[32];
    uint32_t next_col = 0xFFFFFFFFu;
    for (size_t j = 0; j < F; j++)
        if (fam[j]->size()) next_col = std::min(next_col, fam[j]->getById(0).getPosition());
    while (next_col != 0xFFFFFFFFu) {
        const uint32_t col = next_col;
        next_col = 0xFFFFFFFFu;
        for (int &x : node_of_mask) x = -1;
        const uint32_t first_node = (uint32_t)g->pos.size();
        col_edges.clear();
        for (size_t j = 0; j < F; j++) {
            const auto &b = fam[j]->getAlignedBases();
            if (cur[j] < b.size() && b[cur[j]].getPosition() == col) {
                const uint8_t m = b[cur[j]].getBase().mask() & 31;
                // (mseq keys a column's nodes by the base's CHARACTER, mseq.cpp:92-96: masks 0 and 16 are both '.' and
                // share a node, which keeps the base of the first member to show it)
                const uint8_t key = m == 16 ? 0 : m;
                int32_t node = node_of_mask[key];
                if (node < 0) {
                    node = (int32_t)g->pos.size();
                    node_of_mask[key] = node;
                    g->pos.push_back(col);
                    g->mask.push_back(m);
                    count.push_back(1.f);
                    g->succ_minpos.push_back(1000000u);
                } else {
                    count[node] += 1.f;
                }
                if (last[j] >= 0) {
                    col_edges.push_back({(uint32_t)node, (uint32_t)last[j]});
                    if (col < g->succ_minpos[last[j]]) g->succ_minpos[last[j]] = col;
                }
                last[j] = node;
                ++cur[j];
            }
            if (cur[j] < b.size()) next_col = std::min(next_col, b[cur[j]].getPosition());
        }
        // reduce_edges: per node ascending unique predecessor ids
        std::sort(col_edges.begin(), col_edges.end(),
                  [](const ed &x, const ed &y) { return x.b != y.b ? x.b < y.b : x.a < y.a; });
        size_t e = 0;
        for (uint32_t node = first_node; node < g->pos.size(); node++) {
            uint32_t prev = 0xFFFFFFFFu;
            while (e < col_edges.size() && col_edges[e].b == node) {
                if (col_edges[e].a != prev) g->pred.push_back(prev = col_edges[e].a);
                ++e;
            }
            g->pred_off.push_back((uint32_t)g->pred.size());
        }
    }
    g->weight.resize(count.size());
    for (size_t i = 0; i < count.size(); i++)  // mseq.cpp:113: double reciprocal + float product
        g->weight[i] = (float)(1.0 / (double)(fs_weight + 1) + (double)(fs_weight * (count[i] / (float)(unsigned)F)));
}

}  // namespace sina
