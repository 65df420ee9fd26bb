// Checks the gates of the DP driver (sina_amd/csrc/dp_plan.h: dp_kernel_kind, prune_plan_for, scout_allowed; common.h:
// dp_below_init, prune_gain_units) against this program's own table, without a device.  Built and run by
// tests/test_gates_cpu.py (address + undefined-behaviour sanitizers); exits non-zero with a message on the first
// difference.  The table states, row by row and by hand, what the documented rules give -- it calls nothing of the
// library to find its expectations.  argv[1], if given, is the value SINA_HIP_DP_PRUNE would have ("0": the skip is off).
#include <cmath>
#include <cstdarg>
#include <cstring>

#include "dp_plan.h"

namespace sina_hip {
void set_error(const std::string &) {}
void set_limit_error(const std::string &) {}
}  // namespace sina_hip
using namespace sina_hip;

static const char *g_case = "";
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "gate_check: %s: ", g_case);
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) \
    do {                 \
        if (!(cond)) fail(__VA_ARGS__); \
    } while (0)

// One launch: the scoring parameters, the weights' range, the longest DAG and query, and how it is run.
struct Row {
    const char *name;
    float match, mismatch, gp, gpe;
    float wmax, wmin;
    uint32_t n = 801, maxL = 284, strips = 2;
    bool weighted = false, forbid = false, profile = false, generic = false, env_off = false, has_chain = true,
         rho_fixed = false, scout_knob_off = false;
    // expected
    DpKernelKind kind = kDpKernelNone;
    int plan_on = 0;
    uint32_t step = 0;  // what sina_hip_dp_info::prune_step reports: amax where the plan is on, else 0
    bool scout = false;
};

static Row row(const char *name, float match, float mismatch, float gp, float gpe, float wmax, float wmin, DpKernelKind kind,
               int plan_on, uint32_t step, bool scout) {
    Row r{};
    r.name = name, r.match = match, r.mismatch = mismatch, r.gp = gp, r.gpe = gpe, r.wmax = wmax, r.wmin = wmin;
    r.kind = kind, r.plan_on = plan_on, r.step = step, r.scout = scout;
    return r;
}

static void check_row(const Row &r, bool env_off_arg) {
    g_case = r.name;
    const bool below = !r.weighted && !r.forbid && dp_below_init(r.n, r.gp, r.gpe);
    const PrunePlan pp = prune_plan_for(r.match, r.mismatch, r.gp, r.gpe, r.weighted, r.forbid, r.profile, r.wmax, r.wmin, r.maxL,
                                        r.env_off || env_off_arg, r.strips < 2);
    const int want_on = env_off_arg ? 0 : r.plan_on;
    CHECK(pp.on == want_on, "plan on = %d, table says %d", pp.on, want_on);
    const uint32_t step = pp.on ? pp.amax : 0u;
    CHECK(step == (env_off_arg ? 0u : r.step), "prune step %u, table says %u", step, r.step);
    const DpKernelKind kind = dp_kernel_kind(r.weighted, r.forbid, below, r.gp, r.gpe, r.generic, r.profile, pp.on != 0, r.strips);
    DpKernelKind want = r.kind;
    if (env_off_arg && want == kDpKernelSimpleSkip) want = kDpKernelSimple;
    CHECK(kind == want, "kernel %u, table says %u", (unsigned)kind, (unsigned)want);
    const bool scout = scout_allowed(r.has_chain, r.weighted, r.forbid, pp.on != 0, r.rho_fixed, below, r.gp, r.gpe, 64 * (int)r.strips,
                                     r.scout_knob_off, r.generic);
    CHECK(scout == (env_off_arg ? false : r.scout), "scout %d, table says %d", (int)scout, (int)r.scout);
}

// The bound T = U + min(a * r, R - gmin * max(0, C - r)) along a chain whose every column gains g units (R = g * C,
// gmin = g), U left out.  What the skip's induction needs of it (common.h, "the bound"): a match step -- one base, one
// column or more -- loses at least `need` units, a gap step -- a base OR columns -- loses nothing negative.
static int64_t chain_bound(int64_t a, int64_t g, int64_t r, int64_t cols) {
    return std::min(a * r, g * cols - g * std::max<int64_t>(0, cols - r));
}
static void check_induction(int64_t a, int64_t g, int64_t need) {
    for (int64_t cols = 0; cols <= 40; cols++)
        for (int64_t r = 0; r <= 40; r++) {
            const int64_t t = chain_bound(a, g, r, cols);
            CHECK(t >= 0, "negative bound");
            if (r > 0) CHECK(t >= chain_bound(a, g, r - 1, cols), "an insertion step gains (a=%ld g=%ld)", (long)a, (long)g);
            for (int64_t k = 1; k <= cols; k++) {
                CHECK(t >= chain_bound(a, g, r, cols - k), "a deletion step gains (a=%ld g=%ld)", (long)a, (long)g);
                if (r > 0)
                    CHECK(t - chain_bound(a, g, r - 1, cols - k) >= need,
                          "a match step loses less than %ld units (a=%ld g=%ld r=%ld cols=%ld k=%ld)", (long)need, (long)a, (long)g,
                          (long)r, (long)cols, (long)k);
            }
        }
}

int main(int argc, char **argv) {
    const bool env_off_arg = argc > 1 && argv[1][0] == '0';
    const float W = 1.5f, Wlo = 0.58333331f;  // a 12-member family under fs_weight 1: 1/2 + count/12
    const DpKernelKind S = kDpKernelSimple, SK = kDpKernelSimpleSkip, GB = kDpKernelGenericBelow, G = kDpKernelGeneric;
    std::vector<Row> rows = {
        // ---- the case table (tests/gate_cases.py, BASE_SETS): 801 nodes, 284 bases, two strips, device-built DAG
        // kappa64 = 64.0064 * 2 = 128.0128; 1.5 * 128.0128 = 192.02 -> 193 units + 1 of margin
        row("default", 2, -1, 5, 2, W, Wlo, SK, 1, 194, true),
        row("mismatch_gains", 2, 1, 5, 2, W, Wlo, SK, 1, 194, true),
        row("both_cost", -1, -2, 5, 2, W, Wlo, SK, 1, 1, true),                  // kappa == 0: the margin alone
        row("mismatch_above_match", -1, 2, 5, 2, W, Wlo, SK, 1, 194, true),      // kappa is the larger of the two
        row("all_zero_scores", 0, 0, 5, 2, W, Wlo, SK, 1, 1, true),
        row("free_gaps", 2, -1, 0, 0, W, Wlo, SK, 1, 194, true),                 // 0 >= 0 twice, the sum is 1
        row("free_open", 2, -1, 0, 2, W, Wlo, GB, 1, 194, false),                // open < extend
        row("extend_above_open", 2, -1, 2, 3, W, Wlo, GB, 1, 194, false),
        row("negative_gaps", 2, -1, -1, -0.5f, W, Wlo, G, 0, 0, false),
        row("free_extend", 2, -1, 5, 0, W, Wlo, SK, 1, 194, true),
        row("negative_extend", 2, -1, 5, -1, W, Wlo, G, 0, 0, false),
        // fs_weight -0.5: weights 2 - count/24, 1.5 .. 1.9583; 1.9583 * 128.0128 = 250.7 -> 251 + 1 > 250
        row("fs_weight_-0.5", 2, -1, 5, 2, 1.9583334f, 1.5f, S, 0, 0, false),
        row("fs_weight_-0.5_by_fs", 2, -1, 5, 2, 1.5f, -1.f, S, 0, 0, false),   // (align_families: the range fs_weight allows)
        row("fs_weight_-2", 2, -1, 5, 2, -1.1666666f, -3.f, S, 0, 0, false),     // negative node weights
        row("fs_weight_5", 2, -1, 5, 2, 5.1666665f, 0.5833333f, S, 0, 0, false),  // 661.4 -> 662 + 1
        row("tiny", 1e-3f, -1e-3f, 2e-3f, 1e-3f, W, Wlo, SK, 1, 2, true),       // 1.5 * 0.064 = 0.096 -> 1 + 1
        row("large", 200, -100, 500, 200, W, Wlo, S, 0, 0, false),               // 1 + 801 * 505 + 700 < 900000; amax 19203
        row("open_1200", 2, -1, 1200, 2, W, Wlo, G, 1, 194, false),              // 801 * 1212 > 900000: not below
        row("gaps_1e30", 2, -1, 1e30f, 1e30f, W, Wlo, G, 1, 194, false),
        // ---- a caller's DAG with weights of both signs; NaN and infinite weights
        row("mixed_sign_weights", 2, -1, 5, 2, 1.5f, -0.25f, S, 0, 0, false),
        row("nan_weights", 2, -1, 5, 2, NAN, NAN, S, 0, 0, false),
        row("nan_wmin", 2, -1, 5, 2, 1.5f, NAN, S, 0, 0, false),
        row("inf_weights", 2, -1, 5, 2, INFINITY, 0.5f, S, 0, 0, false),
    };
    // ---- either side of each threshold
    {
        // amax: 1.5 * (64.0064 * m) at most 249 -> 250 units; the float above gives 251 (64.0064f * 1.5f * m, m = 2.59349...)
        float m = 2.5f;
        while (prune_gain_units(W, 64.0f * 1.0001f * std::nextafterf(m, INFINITY)) <= 250u) m = std::nextafterf(m, INFINITY);
        CHECK(std::fabs(m - 249.0f / (1.5f * 64.0064f)) < 1e-4f, "the amax threshold is not where the arithmetic puts it: %g", (double)m);
        rows.push_back(row("amax_250", m, -1, 5, 2, W, Wlo, SK, 1, 250, true));
        rows.push_back(row("amax_251", std::nextafterf(m, INFINITY), -1, 5, 2, W, Wlo, S, 0, 0, false));
        // below_init: 1 + 801 * g * 1.01 + g + 2 < 900000 <=> g < 1111.09...
        float g = 1111.0f;
        CHECK(dp_below_init(801, g, 2) && !dp_below_init(801, 1111.2f, 2), "below_init is not near 1111.09");
        while (dp_below_init(801, std::nextafterf(g, INFINITY), 2)) g = std::nextafterf(g, INFINITY);
        CHECK(g > 1111.0f && g < 1111.2f, "below_init threshold %g", (double)g);
        auto own_sum = [](float gp) { return 1.0f + 801.0f * gp * 1.01f + gp + 2.0f; };  // (float32 throughout, as common.h adds it)
        CHECK(own_sum(g) < 900000.0f && own_sum(std::nextafterf(g, INFINITY)) >= 900000.0f, "the sum changes sides at %g, not at 900000",
              (double)own_sum(g));
        rows.push_back(row("below_init_in", 2, -1, g, 2, W, Wlo, SK, 1, 194, true));
        rows.push_back(row("below_init_out", 2, -1, std::nextafterf(g, INFINITY), 2, W, Wlo, G, 1, 194, false));
        rows.push_back(row("extend_equals_open", 2, -1, 5, 5, W, Wlo, SK, 1, 194, true));
        rows.push_back(row("extend_just_above_open", 2, -1, 5, std::nextafterf(5.f, INFINITY), W, Wlo, GB, 1, 194, false));
        // exact units: amax * maxL below 2^23 (194 * 43240 = 8388560, 194 * 43241 = 8388754)
        Row a = row("units_exact", 2, -1, 5, 2, W, Wlo, SK, 1, 194, true), b = row("units_inexact", 2, -1, 5, 2, W, Wlo, S, 0, 0, false);
        a.maxL = 43240, a.strips = 170, b.maxL = 43241, b.strips = 170;
        rows.push_back(a), rows.push_back(b);
    }
    // ---- how the launch is run
    {
        Row r = row("single_strip", 2, -1, 5, 2, W, Wlo, S, 0, 0, false);
        r.strips = 1;
        rows.push_back(r);
        r = row("generic_knob", 2, -1, 5, 2, W, Wlo, GB, 1, 194, false);
        r.generic = true;
        rows.push_back(r);
        r = row("generic_knob_not_below", 2, -1, 1200, 2, W, Wlo, G, 1, 194, false);
        r.generic = true;
        rows.push_back(r);
        r = row("weighted", 2, -1, 5, 2, W, Wlo, kDpKernelWeighted, 0, 0, false);
        r.weighted = true;
        rows.push_back(r);
        r = row("forbid", 2, -1, 5, 2, W, Wlo, kDpKernelForbid, 0, 0, false);
        r.forbid = true;
        rows.push_back(r);
        r = row("weighted_forbid", 2, -1, 5, 2, W, Wlo, kDpKernelWeightedForbid, 0, 0, false);
        r.weighted = r.forbid = true;
        rows.push_back(r);
        r = row("weighted_kappa0", -1, -2, 5, 2, W, Wlo, kDpKernelWeighted, 0, 0, false);
        r.weighted = true;
        rows.push_back(r);
        r = row("profile_batch", 2, -1, 5, 2, W, Wlo, GB, 0, 0, false);
        r.profile = true, r.has_chain = false;
        rows.push_back(r);
        r = row("caller_built_dag", 2, -1, 5, 2, W, Wlo, SK, 1, 194, false);  // no chain: the skip runs on the store's guess
        r.has_chain = false;
        rows.push_back(r);
        r = row("fixed_rho", 2, -1, 5, 2, W, Wlo, SK, 1, 194, false);
        r.rho_fixed = true;
        rows.push_back(r);
        r = row("scout_knob_off", 2, -1, 5, 2, W, Wlo, SK, 1, 194, false);
        r.scout_knob_off = true;
        rows.push_back(r);
        r = row("prune_env_off", 2, -1, 5, 2, W, Wlo, S, 0, 0, false);  // SINA_HIP_DP_PRUNE=0
        r.env_off = true;
        rows.push_back(r);
    }
    for (const Row &r : rows) check_row(r, env_off_arg);

    // ---- the kappa == 0 plan: what it hands the kernel, what the builders make of it
    g_case = "kappa == 0";
    {
        const PrunePlan pp = prune_plan_for(-1, -2, 5, 2, false, false, false, W, Wlo, 284, false, false);
        CHECK(pp.on == 1 && pp.amax == 1u && pp.kappa64 == 1e-30f, "plan: on %d amax %u kappa64 %g", pp.on, pp.amax, (double)pp.kappa64);
        const uint32_t node = prune_gain_units(W, pp.kappa64), light = prune_gain_units(Wlo, pp.kappa64);
        CHECK(node == 2u && light == 2u, "the builders' gain of a node: %u, %u units", node, light);
        // What the induction needs.  The bound is the smaller of two terms, a * r (every query base to come gains a
        // at most) and the column term (every column to come gains its best node's units at most), and each is a bound
        // on its own if its step is at least the TRUE gain of a match, in units and rounded up, plus the unit of margin
        // for the float rounding of the cell values.  With kappa == 0 no step gains: the true gain is 0, so both need
        // one unit.  They need not be equal -- the smaller of two bounds is a bound -- and a node gain above a only
        // loosens the column term.
        const uint32_t true_gain_units = 0, margin = 1;
        CHECK(pp.amax >= true_gain_units + margin, "a = %u is below gain + margin", pp.amax);
        CHECK(node >= true_gain_units + margin && light >= true_gain_units + margin, "a node's units are below gain + margin");
        // ... and computed: along a chain under (a = 1, node gain 2) a match step loses at least the margin
        check_induction(pp.amax, node, margin);
        // the same for the default scheme's numbers and for equal a and node gain, so that the check itself is seen to
        // hold where the suite has always run
        check_induction(194, 194, 76);  // (a 12-member family's lightest column: 0.5833 * 128.0128 -> 75 + 1)
        check_induction(2, 2, 2);
    }
    printf("gate_check: ok (%zu rows%s)\n", rows.size(), env_off_arg ? ", SINA_HIP_DP_PRUNE=0" : "");
    return 0;
}
