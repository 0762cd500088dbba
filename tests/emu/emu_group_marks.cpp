// emu_group_marks.cpp — swarmkit_amd/csrc/swp_rounds.hpp alone (no HIP, no engine): the rule that says behind which groups of a
// streamed tick the kernel appends a mark (group_pub_step, group_marks — what swp_schedule_groups_streamed's driver computes up front),
// and those marks fed through StreamMarks as the driver feeds them; tests/test_group_marks_cpu.py checks what comes out.
// TEST INFRASTRUCTURE around product source; no product code path uses it.
//   tick knob min_tasks AxB ...    A groups of B tasks each, in order. Prints "step S total T groups G", one line "mark M group g" per
//                                  mark, one line "range first count" per delivery, then "end delivered top taken complete bad marks"
//   knob                           stream_group_tasks() from the environment
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

using namespace swpdev;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "knob") && argc == 2) {
        printf("%u\n", stream_group_tasks());
        return 0;
    }
    if (strcmp(argv[1], "tick") || argc < 4) return 2;
    const uint32_t knob = (uint32_t)strtoul(argv[2], nullptr, 10), min_tasks = (uint32_t)strtoul(argv[3], nullptr, 10);
    std::vector<uint32_t> sizes;   // (on the heap: the sanitizers watch the reads)
    for (int i = 4; i < argc; ++i) {
        unsigned a = 0, b = 0;
        if (sscanf(argv[i], "%ux%u", &a, &b) != 2) return 2;
        sizes.insert(sizes.end(), a, b);
    }
    uint64_t total = 0;
    for (uint32_t s : sizes) total += s;
    const uint32_t step = group_pub_step(total, (uint32_t)sizes.size(), knob);
    printf("step %u total %llu groups %zu\n", step, (unsigned long long)total, sizes.size());
    std::vector<uint32_t> marks;
    const uint32_t n = group_marks(sizes.data(), (uint32_t)sizes.size(), step, [&](uint32_t mark, uint32_t g) {
        printf("mark %u group %u\n", mark, g);
        marks.push_back(mark);
    });
    if (n != marks.size()) return 3;
    StreamMarks m((uint32_t)total, min_tasks);
    m.enqueued = n;
    for (uint32_t mark : marks) {
        uint32_t first = 0, count = 0;
        if (m.take(mark, &first, &count)) printf("range %u %u\n", first, count);
    }
    printf("end %u %u %u %d %d %u\n", m.delivered, m.top, m.taken, m.complete() ? 1 : 0, m.bad ? 1 : 0, n);
    return 0;
}
