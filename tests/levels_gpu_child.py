"""One process of tests/test_engine_levels.py: 7 000 cfg3 tasks on 2 304 nodes (three laps over the node set, 72 half-words: more than
a list holds) through the CPU oracle and through the engine, compared as tests/test_engine_fuzz.py compares (node per task,
explanation per unplaceable task). The knobs come with the environment (SWP_R6_LEVELS, SWP_R6_BLOCK, SWP_DBG); prints one
"levels-child:" line with the rounds the block resolver took.

    python tests/levels_gpu_child.py <rr | major>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import parity_util as pu  # noqa: E402
from swarmkit_amd import synth  # noqa: E402


def main():
    order = sys.argv[1]
    wl = synth.Workload("cfg3", T=7000, N=2304, order=order)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, out, hist = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    print("levels-child: order=%s placed=%d unplaceable=%d resolver=%d rounds=%d" % (order, st["placed"], st["infeasible"], st["last_resolver"], st["resolve_launches"] // 2), flush=True)


if __name__ == "__main__":
    main()
