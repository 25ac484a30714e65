// Runs every row of csrc/admission.h, with both outcomes of a "by argument" column, against every kind of carried work, with
// counters in place of the runtime: one line per combination (tests/test_admission_cpu.py compiles, runs and checks it).
#include <cstdio>

#include "../dots_socp_amd/csrc/admission.h"

static std::string g_error;
void dots::set_error(const std::string &msg) { g_error = msg; }

using namespace dots;

static std::string g_calls;      // the callbacks in the order they ran: S select_device, D divide, R rebuild_zmid
static const Runtime COUNTING = {[](void *) -> int { g_calls += 'S'; return 0; },
                                 [](void *, double) -> int { g_calls += 'D'; return 0; },
                                 [](void *) -> int { g_calls += 'R'; return 0; }};

struct Situation {
    const char *name;
    void (*set)(Carried &);
};
static const Situation SITUATIONS[] = {
    {"nothing", [](Carried &) {}},
    {"division", [](Carried &k) { k.pending_div = 2.0; }},
    {"gathers", [](Carried &k) { k.carry_valid = 1; k.step_path = 1024; k.deep_path = 1; }},
    {"fused_sums", [](Carried &k) { k.kkt_fused_valid = 1; }},
    {"zmid_deferred", [](Carried &k) { k.zmid = ZMID_DEFERRED; }},
    {"zmid_unspecified", [](Carried &k) { k.zmid = ZMID_UNSPECIFIED; }},
    {"rhs_armed", [](Carried &k) { k.rhs_ahead_armed = 1; }},
    {"rhs_ahead_1", [](Carried &k) { k.rhs_ahead = 1; }},
    {"rhs_ahead_2", [](Carried &k) { k.rhs_ahead = 2; k.ahead_div = 2.0; }},
    {"rhs_ahead_3", [](Carried &k) { k.rhs_ahead = 3; }},
    {"rhs_ahead_4", [](Carried &k) { k.rhs_ahead = 4; k.pending_div = 2.0; }},
    {"penalty_armed", [](Carried &k) { k.penalty_armed = 1; }},
    {"halos_fresh", [](Carried &k) { k.kkt_halo_fresh = 1; }},
    {"surface_moved", [](Carried &k) { k.needs_restart = 1; }},
};

int main() {
    static_assert(sizeof ADMISSION / sizeof ADMISSION[0] == N_ENTRIES, "one row per entry");
    if (admit(nullptr, E_SYNC, COUNTING, nullptr) != DOTS_ERR_ARGUMENT || g_error != "null context" || !g_calls.empty()) return 1;
    for (int e = 0; e < N_ENTRIES; ++e) {
        const Row &row = ADMISSION[e];
        printf("row %d %s access=%s%s%s%s reads=%d refuses=%d\n", e, row.name, row.access & DROPS ? "D" : "", row.access & DUALS ? "U" : "",
               row.access & STATE ? "S" : "", row.access & SURFACE ? "F" : "", (int)row.reads, (int)row.refuses);
        const bool by_argument = row.reads == BY_ARGUMENT || row.refuses == BY_ARGUMENT;
        for (int arg = by_argument ? 0 : 1; arg < 2; ++arg)
            for (const Situation &s : SITUATIONS) {
                Carried k, before;
                s.set(k);
                before = k;
                g_calls.clear();
                g_error.clear();
                int rc = admit(&k, (Entry)e, COUNTING, &k);
                if (!rc) rc = need_zmid(k, (Entry)e, COUNTING, &k, arg != 0);
                std::string dropped;
                const struct { const char *name; int was, is; } flags[] = {
                    {"rhs_ahead", before.rhs_ahead, k.rhs_ahead}, {"rhs_ahead_armed", before.rhs_ahead_armed, k.rhs_ahead_armed},
                    {"penalty_armed", before.penalty_armed, k.penalty_armed}, {"carry_valid", before.carry_valid, k.carry_valid},
                    {"kkt_fused_valid", before.kkt_fused_valid, k.kkt_fused_valid}, {"step_path", before.step_path, k.step_path},
                    {"deep_path", before.deep_path, k.deep_path}};
                for (const auto &f : flags)
                    if (f.was && !f.is) dropped += std::string(dropped.empty() ? "" : ",") + f.name;
                printf("run %d arg=%d %s status=%d calls=%s dropped=%s after: div=%g ahead_div=%g zmid=%d halos=%d moved=%d error=%s\n", e, arg, s.name, rc,
                       g_calls.c_str(), dropped.c_str(), k.pending_div, k.ahead_div, (int)k.zmid, k.kkt_halo_fresh, k.needs_restart, g_error.c_str());
            }
    }
    // the named drops, each applied to a Carried with every flag set
    const struct { const char *name; void (Carried::*drop)(); } drops[] = {
        {"change", &Carried::drop_for_change}, {"step0", &Carried::drop_for_step0}, {"steps23", &Carried::drop_for_steps23}};
    for (const auto &d : drops) {
        Carried k;
        k.rhs_ahead = k.rhs_ahead_armed = k.penalty_armed = k.carry_valid = k.kkt_fused_valid = k.step_path = k.deep_path = 1;
        k.pending_div = 2.0; k.zmid = ZMID_DEFERRED; k.kkt_halo_fresh = k.needs_restart = 1;
        (k.*d.drop)();
        printf("drop %s keeps: rhs_ahead=%d rhs_ahead_armed=%d penalty_armed=%d carry_valid=%d kkt_fused_valid=%d step_path=%d deep_path=%d div=%g zmid=%d halos=%d moved=%d\n",
               d.name, k.rhs_ahead, k.rhs_ahead_armed, k.penalty_armed, k.carry_valid, k.kkt_fused_valid, k.step_path, k.deep_path, k.pending_div, (int)k.zmid,
               k.kkt_halo_fresh, k.needs_restart);
    }
    return 0;
}
