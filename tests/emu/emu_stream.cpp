// emu_stream.cpp — swarmkit_amd/csrc/swp_rounds.hpp alone (no HIP, no engine): the streamed driver's mark arithmetic (StreamMarks) fed
// with a scripted sequence of marks, as stream_service in swp_engine.hip feeds it from the ring; tests/test_stream_cpu.py checks what
// comes out. TEST INFRASTRUCTURE around product source; no product code path uses it.
//   marks T min_tasks mark...     one line "first count" per delivery, then "end delivered top taken complete bad"
//   ring n                        n publishes enqueued without a mark taken: "room" after each, as 0 / 1
//   every                         stream_every() from the environment
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

using namespace swpdev;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    auto u = [&](int i) { return (uint32_t)strtoul(argv[i], nullptr, 10); };
    if (!strcmp(cmd, "marks") && argc >= 4) {
        StreamMarks m(u(2), u(3));
        std::vector<uint32_t> marks;   // (on the heap: the sanitizers watch the reads)
        for (int i = 4; i < argc; ++i) marks.push_back(u(i));
        m.enqueued = (uint32_t)marks.size();
        for (uint32_t mark : marks) {
            uint32_t first = 0, count = 0;
            if (m.take(mark, &first, &count)) printf("%u %u\n", first, count);
        }
        printf("end %u %u %u %d %d\n", m.delivered, m.top, m.taken, m.complete() ? 1 : 0, m.bad ? 1 : 0);
    } else if (!strcmp(cmd, "ring") && argc == 3) {
        StreamMarks m(1000, 0);
        for (uint32_t i = 0; i < u(2); ++i) {
            printf("%d\n", m.room() ? 1 : 0);
            m.enqueued += 1;
        }
        printf("%u %u\n", m.outstanding(), StreamMarks::RING);
    } else if (!strcmp(cmd, "every") && argc == 2) {
        printf("%u\n", stream_every());
    } else
        return 2;
    return 0;
}
