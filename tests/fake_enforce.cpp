// fake_enforce.cpp — swp_enforce_generic for the engine TEST DOUBLE (tests/fake_swp.cpp), built into a library of its own
// (tests/fakeenforce.py). It is the sequential composition the real call stands for, through the public ABI only: the double's
// swp_enforce for the verdicts up to line 184 of the reference's loop (the double scripts them: pseudo-random in call order), then per
// node, in task order, the last third of the loop body (constraint_enforcer.go:186-200) on the caller's arrays: HasResource per
// assignment entry, `break loop` at the first one that is gone, ConsumeNodeResources otherwise — on plain vectors that are erased from.
// The host layer above then makes ONE call for a request with assignments, and its answer can be compared with the plain double's
// library, where the host layer walks the same nodes itself after swp_enforce: both reach the double's swp_enforce once, with the same
// records, so the scripted verdicts line up.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../include/swp.h"

static uint64_t g_enforce_generic_calls = 0;

namespace {
typedef std::vector<swp_enforce_res> List;

bool has_resource(const swp_enforce_res& res, const List& resources) {   // validate.go:54-85
    for (const swp_enforce_res& r : resources) {
        if (res.kind != r.kind) continue;
        if (!r.named) return !res.named && !(res.value > r.value);
        if (!res.named) return false;
        if (res.value != r.value) continue;
        return true;
    }
    return false;
}
bool remove_one(swp_enforce_res& na, const swp_enforce_res& r) {   // helpers.go:87-111
    if (!r.named) {
        if (na.named) return false;
        na.value = (int64_t)((uint64_t)na.value - (uint64_t)r.value);
        return na.value <= 0;
    }
    return na.named && r.value == na.value;
}
void consume(List* avail, const swp_enforce_res* res, uint32_t n) {   // helpers.go:58-85
    List kept;
    for (swp_enforce_res na : *avail) {
        bool gone = false;
        for (uint32_t q = 0; q < n && !gone; ++q)
            if (na.kind == res[q].kind && remove_one(na, res[q])) gone = true;
        if (!gone) kept.push_back(na);
    }
    avail->swap(kept);
}
}   // namespace

extern "C" {

int swp_enforce_generic(swp_engine* e, const swp_enforce_node* nodes, uint32_t n_nodes, const swp_enforce_task* tasks, uint32_t n_tasks, const uint32_t* node_res_off,
                        const swp_enforce_res* node_res, const uint32_t* task_res_off, const swp_enforce_res* task_res, uint8_t* out_reject) {
    if (!e || (!nodes && n_nodes) || (!tasks && n_tasks) || (!out_reject && n_tasks)) return SWP_EINVAL;
    ++g_enforce_generic_calls;
    if ((n_nodes && !node_res_off) || (n_tasks && !task_res_off)) return SWP_EINVAL;
    for (int side = 0; side < 2; ++side) {
        const uint32_t n = side ? n_tasks : n_nodes;
        const uint32_t* off = side ? task_res_off : node_res_off;
        const swp_enforce_res* res = side ? task_res : node_res;
        if (n == 0) continue;
        for (uint32_t i = 0; i < n; ++i)
            if (off[i + 1] < off[i]) return SWP_EINVAL;
        if (off[n] > off[0] && !res) return SWP_EINVAL;
        for (uint32_t q = off[0]; q < off[n]; ++q) {
            char name[1];
            if (swp_intern_lookup(e, SWP_SPACE_GENERIC_KIND, res[q].kind, name, 0) < 0 || res[q].named > 1u) return SWP_EINVAL;
        }
    }
    for (uint32_t i = 0; i < n_nodes; ++i) {
        swp_node_row row;
        if (swp_node_get(e, nodes[i].node, &row) != SWP_OK) return SWP_ENOTFOUND;
        if ((uint64_t)nodes[i].first_task + nodes[i].n_tasks > n_tasks) return SWP_EINVAL;
    }
    std::vector<uint8_t> rej(n_tasks, 0);
    if (int rc = swp_enforce(e, nodes, n_nodes, tasks, n_tasks, rej.data())) return rc;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t t0 = nodes[i].first_task, t1 = t0 + nodes[i].n_tasks;
        if (t1 == t0 || task_res_off[t1] == task_res_off[t0]) continue;   // no assignment on this node: swp_enforce's verdicts stand
        List avail(node_res + node_res_off[i], node_res + node_res_off[i + 1]);
        bool broke = false;
        for (uint32_t t = t0; t < t1; ++t) {
            if (broke) { rej[t] = 0; continue; }
            const swp_enforce_task& tr = tasks[t];
            if (tr.desired_state < 192u || tr.desired_state > 576u || tr.state >= 576u) continue;   // :118-126 (the double's verdict stands, as in the host layer's own walk)
            const uint32_t q0 = task_res_off[t], q1 = task_res_off[t + 1];
            if (rej[t] || q0 == q1) continue;
            bool gone = false;
            for (uint32_t q = q0; q < q1 && !gone; ++q) gone = !has_resource(task_res[q], avail);
            if (gone) { rej[t] = 1; broke = true; continue; }
            consume(&avail, task_res + q0, q1 - q0);
        }
    }
    if (n_tasks) std::memcpy(out_reject, rej.data(), n_tasks);
    return SWP_OK;
}

// test-only: how many swp_enforce_generic calls this library has seen (refused ones included)
uint64_t swp_fake_enforce_generic_calls(void) { return g_enforce_generic_calls; }

}   // extern "C"
