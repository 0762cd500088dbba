// fake_fitvol.cpp — swp_fit_pairs_volumes for the engine TEST DOUBLE (tests/fake_swp.cpp + tests/fake_fit.cpp), built into a third
// library (tests/fakefitvol.py). Like tests/fake_fit.cpp it is the sequential composition the real call stands for, through the public
// ABI only: per pair, in array order, the double's swp_check_node; on a pass of a template with cluster mounts its swp_choose_volumes;
// and — unless that choice failed — its swp_commit. A failed choice reports SWP_FIT_NO_VOLUME with the row swp_choose_volumes gave and
// books nothing. All or nothing like the real call: a template of a service named "boom..." refuses the whole call before anything is
// judged. The host layer above then keeps mount tasks inside its runs, and its answers can be compared with the plain double's
// library, which takes the per-task path: both reach the double's check / choose / commit in the same order, so the scripted
// pseudo-random verdicts and choices line up.
#include <cstdint>
#include <cstring>

#include "../include/swp.h"

static uint64_t g_fitvol_calls = 0;

extern "C" {

int swp_fit_pairs_volumes(swp_engine* e, const swp_task_desc* templates, uint32_t n_templates, const swp_fit_pair* pairs, uint32_t n_pairs, int32_t* first_fail,
                          uint32_t* out_att) {
    if (!e || (!templates && n_templates) || (!pairs && n_pairs) || ((!first_fail || !out_att) && n_pairs)) return SWP_EINVAL;
    ++g_fitvol_calls;
    for (uint32_t t = 0; t < n_templates; ++t) {
        char name[5] = {0};
        if (swp_intern_lookup(e, SWP_SPACE_SERVICE, templates[t].service, name, sizeof name) < 0) return SWP_EINVAL;
        if (std::strncmp(name, "boom", 4) == 0) return SWP_ERANGE;
    }
    for (uint32_t i = 0; i < n_pairs; ++i) {
        swp_node_row row;
        if (pairs[i].tmpl >= n_templates) return SWP_EINVAL;
        if (swp_node_get(e, pairs[i].node, &row) != SWP_OK) return SWP_ENOTFOUND;
    }
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const swp_task_desc& d = templates[pairs[i].tmpl];
        uint32_t* row = out_att + (size_t)i * SWP_MAX_MOUNTS;
        for (uint32_t m = 0; m < SWP_MAX_MOUNTS; ++m) row[m] = SWP_NO_VOLUME;
        if (int rc = swp_check_node(e, &d, pairs[i].node, &first_fail[i])) return rc;
        if (first_fail[i] != -1) continue;
        if (d.flags >> SWP_TASK_MOUNTS_SHIFT) {
            uint32_t n_out = 0, failed = 0;
            if (int rc = swp_choose_volumes(e, d.flags >> SWP_TASK_MOUNTS_SHIFT, pairs[i].node, row, &n_out, &failed)) return rc;
            if (n_out == 0) {
                first_fail[i] = SWP_FIT_NO_VOLUME;
                continue;
            }
        }
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

// test-only: how many swp_fit_pairs_volumes calls this library has seen (refused ones included)
uint64_t swp_fake_fitvol_calls(void) { return g_fitvol_calls; }

}   // extern "C"
