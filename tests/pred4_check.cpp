// prep_range's pred4 table (sina_amd/csrc/dp_plan.h; common.h, pred4_pack) of one DAG, printed for
// tests/test_pred4_cpu.py to compare with the DAG's own predecessor lists.  Built and run there under the address and
// undefined-behaviour sanitizers; no device.
//
// `pred4_check FILE KAPPA64`: FILE is text (the format of dp_plan_check --words): N E, then N columns, N masks, N weights
// (float bits), N + 1 pred_off, E predecessors.  The DAG is the SECOND query of a two-query range, behind a chain of three
// nodes, so that its rows do not start at entry 0 of the range's tables.  Prints "rgain_ok 0|1", then a line of four ids
// per row of the chain and of the DAG, as the bytes lie in memory (4 x u16).
#include <cstring>

#include "dp_plan.h"

namespace sina_hip {
static std::string g_err;
void set_error(const std::string &m) { g_err = m; }
void set_limit_error(const std::string &m) { g_err = m; }
}  // namespace sina_hip
using namespace sina_hip;

static int fail(const char *what) {
    fprintf(stderr, "pred4_check: %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 3) return fail("usage: pred4_check FILE KAPPA64");
    FILE *f = fopen(argv[1], "r");
    if (!f) return fail("cannot read the file");
    unsigned n = 0, e = 0;
    if (fscanf(f, "%u %u", &n, &e) != 2 || n == 0) return fail("header");
    const uint32_t n0 = 3, e0 = 2;  // the chain in front
    std::vector<uint32_t> pos{0, 1, 2}, pred_off{0, 0, 1, 2}, pred{0, 1};
    std::vector<uint8_t> mask{1, 1, 1};
    std::vector<float> weight{1.f, 1.f, 1.f};
    bool short_file = false;
    auto read = [&]() -> uint32_t {
        unsigned v = 0;
        if (fscanf(f, "%u", &v) != 1) short_file = true;
        return v;
    };
    for (unsigned i = 0; i < n; i++) pos.push_back(read());
    for (unsigned i = 0; i < n; i++) mask.push_back((uint8_t)read());
    for (unsigned i = 0; i < n; i++) {
        const uint32_t bits = read();
        float w;
        memcpy(&w, &bits, 4);
        weight.push_back(w);
    }
    for (unsigned i = 0; i <= n; i++) pred_off.push_back(read());  // (relative to the query's own edges)
    for (unsigned i = 0; i < e; i++) pred.push_back(read());
    fclose(f);
    if (short_file) return fail("short file");
    const uint64_t node_off[3] = {0, n0, (uint64_t)n0 + n}, edge_off[3] = {0, e0, (uint64_t)e0 + e}, qoff[3] = {0, 10, 20};
    sina_hip_graph_batch g{};
    g.nq = 2;
    g.node_off = node_off, g.edge_off = edge_off;
    g.node_pos = pos.data(), g.node_mask = mask.data(), g.node_weight = weight.data();
    g.pred_off = pred_off.data(), g.pred = pred.data();
    g.width = 100000;
    HostPrep hp;
    if (prep_range(&g, qoff, 0, 2, 512, 4, &hp, (float)atof(argv[2]), nullptr) != 0) return fail(g_err.c_str());
    if (hp.pred4.size() != (size_t)n0 + n || hp.qd[1].node_off != n0) return fail("table size / node_off");
    printf("rgain_ok %d\n", hp.rgain_ok ? 1 : 0);
    for (size_t m = 0; m < hp.pred4.size(); m++) {
        uint16_t id[4];
        static_assert(sizeof(uint2) == sizeof id, "4 x u16 in 8 bytes");
        memcpy(id, &hp.pred4[m], sizeof id);
        printf("%u %u %u %u\n", id[0], id[1], id[2], id[3]);
    }
    return 0;
}
