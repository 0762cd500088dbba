"""One process of tests/test_engine_ring.py.

    python tests/ring_gpu_child.py <rr | major>   3 000 cfg3 tasks on 4 096 nodes through the CPU oracle and through the engine, compared as
                                                  tests/test_engine_fuzz.py compares (node per task, explanation per unplaceable task)
    python tests/ring_gpu_child.py small          1 200 tasks of 4 services on 96 nodes, round-robin: levels run out all the time
    python tests/ring_gpu_child.py volumes        the volume script of tests/bigcases.py (cluster mounts: no ring by rule)
The knobs come with the environment (SWP_R6_RING, SWP_R6_BLOCK, SWP_DBG); prints one "ring-child:" line."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import parity_util as pu  # noqa: E402
from swarmkit_amd import synth  # noqa: E402


def main():
    what = sys.argv[1]
    if what == "volumes":
        import bigcases
        import orc
        from swarmkit_amd import host as swhost
        os.environ["SWP_HOST"] = "cxx"
        want = bigcases.run_volumes(orc.Oracle(), N=300, T=900, services=40)
        sched = swhost.HostScheduler()
        got = bigcases.run_volumes(sched, N=300, T=900, services=40)
        assert got["ticks"] == want["ticks"] and got["placed"] == want["placed"], (got["placed"], want["placed"])
        print("ring-child: what=volumes placed=%s resolver=%d" % (sum(got["placed"]) if isinstance(got["placed"], (list, tuple)) else got["placed"], sched.e.stats()["last_resolver"]), flush=True)
        return
    wl = synth.Workload("cfg3", T=1200, N=96, services=4, order="rr") if what == "small" else synth.Workload("cfg3", T=3000, N=4096, order=what)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, out, hist = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    print("ring-child: what=%s placed=%d unplaceable=%d resolver=%d rounds=%d" % (what, st["placed"], st["infeasible"], st["last_resolver"], st["resolve_launches"] // 2), flush=True)


if __name__ == "__main__":
    main()
