// fake_fit.cpp — swp_fit_pairs for the engine TEST DOUBLE (tests/fake_swp.cpp), built into a second library of its own
// (tests/fakefit.py). It is the sequential composition the real call stands for: per pair, in array order, the double's
// swp_check_node and — on a pass — its swp_commit, through the public ABI only. Like the real call it is all or nothing: before
// anything is judged it refuses the whole call the way the double refuses a single check (a template of a service named "boom...":
// SWP_ERANGE) and checks every pair's template and node. The host layer above (swarmkit_amd/csrc/swp_sched.cpp) then takes its
// batched path, and its decisions can be compared with the plain double's library, which takes the per-task path: both call the
// double's swp_check_node in the same order, so its pseudo-random verdicts line up.
#include <cstdint>
#include <cstring>

#include "../include/swp.h"

static uint64_t g_fit_calls = 0;

extern "C" {

int swp_fit_pairs(swp_engine* e, const swp_task_desc* templates, uint32_t n_templates, const swp_fit_pair* pairs, uint32_t n_pairs, int32_t* first_fail) {
    if (!e || (!templates && n_templates) || (!pairs && n_pairs) || (!first_fail && n_pairs)) return SWP_EINVAL;
    ++g_fit_calls;
    for (uint32_t t = 0; t < n_templates; ++t) {
        char name[5] = {0};
        if (swp_intern_lookup(e, SWP_SPACE_SERVICE, templates[t].service, name, sizeof name) < 0) return SWP_EINVAL;
        if (std::strncmp(name, "boom", 4) == 0) return SWP_ERANGE;
        if (templates[t].flags >> SWP_TASK_MOUNTS_SHIFT) return SWP_EUNSUPPORTED;
    }
    for (uint32_t i = 0; i < n_pairs; ++i) {
        swp_node_row row;
        if (pairs[i].tmpl >= n_templates) return SWP_EINVAL;
        if (swp_node_get(e, pairs[i].node, &row) != SWP_OK) return SWP_ENOTFOUND;
    }
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const swp_task_desc& d = templates[pairs[i].tmpl];
        if (int rc = swp_check_node(e, &d, pairs[i].node, &first_fail[i])) return rc;
        if (first_fail[i] != -1) continue;
        swp_placement p;
        std::memset(&p, 0, sizeof p);
        p.node = pairs[i].node;
        p.service = d.service;
        p.cpu = d.cpu;
        p.mem = d.mem;
        p.port_set = d.port_set;
        p.counted = (d.flags & SWP_TASK_UNCOUNTED) ? 0u : 1u;
        if (int rc = swp_commit(e, &p, 1, 1)) return rc;
    }
    return SWP_OK;
}

// test-only: how many swp_fit_pairs calls this library has seen (refused ones included)
uint64_t swp_fake_fit_calls(void) { return g_fit_calls; }

}   // extern "C"
