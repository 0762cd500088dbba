"""CPU model of the block resolver's rounds with LATE-STAGED list windows (swp_resolve6.hpp, r6_commit_t): how many rounds does the
headline workload take for a block size, a list length, a window length and a staging lookahead?  Decides the next block / list /
window choice without a GPU, in the style of tools/sim_k7.py.

cfg3 (or a scaled copy) in round-robin order is replayed with the list rule: at a block's start every task of the block lists the first
`list` non-empty 32-node half-words of its feasible plain nodes on their minimum level, behind the share of its identical tasks in
front of it (k_r6_propose's twins); tasks are then decided in order, each taking the first listed node nobody took (every pick
strikes). `window` (0: the whole list in LDS): of a task in 64-task group g >= 2 only the first `window` entries that are live once
group g - `lookahead` is decided are kept; groups 0 and 1 keep the list's first `window` entries. The block is cut at the first task
whose kept entries are all taken — counted as a window cut if entries had been left out — and the next block starts there.

usage: python tools/sim_window.py [--T 100000] [--N 10000] [--rows 768:32:0:2,1408:64:16:2,...]      (block:list:window:lookahead)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from swarmkit_amd import synth  # noqa: E402
from sim_k7 import static_rows  # noqa: E402

DEFAULT_ROWS = "768:32:0:2,1024:48:0:2,1408:64:16:2,1408:48:16:2,1408:64:14:2,2048:64:16:2,2048:64:12:2"


def rounds_for(wl, rows, B, H, W, look):
    N, T, S = wl.N, wl.T, wl.S
    cpu, mem = wl.node_cpu.copy(), wl.node_mem.copy()
    total = np.zeros(N, dtype=np.int64)
    on = np.zeros((S, N), dtype=bool)
    hw_of = np.arange(N) // 32
    pos = rounds = cut_list = cut_win = 0
    while pos < T:
        n = min(B, T - pos)
        lists, more = [], []   # per task: (half-word ids, candidate masks as node arrays), "the level has more"
        seen = {}
        for i in range(n):
            k = (pos + i) % S
            p = rows[k] & (cpu >= wl.svc_cpu[k]) & (mem >= wl.svc_mem[k]) & ~on[k]
            twins = seen.get(k, 0)
            seen[k] = twins + 1
            if not p.any():
                lists.append(None)
                more.append(False)
                continue
            cand = np.flatnonzero(p & (total == total[p].min()))
            cand = cand[min(twins, len(cand) - 1):]   # (a level the twins use up lists its last candidate: a cut)
            hws = np.unique(hw_of[cand])
            more.append(len(hws) > H)
            hws = hws[:H]
            lists.append([(h, cand[hw_of[cand] == h]) for h in hws])
        taken = np.zeros(N, dtype=bool)
        kept = [None] * n
        why = 0
        done = n
        for i in range(n):
            g = i // 64
            if i % 64 == 0:   # stage the windows of group g + look (and of groups 0 .. look - 1 + 1 at the start)
                for gs in ([0, 1] if g == 0 else []) + ([g + look] if g + look >= 2 else []):
                    for t in range(gs * 64, min(gs * 64 + 64, n)):
                        if lists[t] is None or kept[t] is not None:
                            continue
                        live = [e for e in lists[t] if not taken[e[1]].all()] if (W and gs >= 2) else lists[t]
                        cut_here = W if W else len(live)
                        kept[t] = (live[:cut_here], more[t] or len(live) > cut_here)
            if lists[i] is None:
                continue
            if kept[i] is None:
                kept[i] = (lists[i][:W] if W else lists[i], more[i] or (W and len(lists[i]) > W))
            pick = -1
            for h, nodes in kept[i][0]:
                free = nodes[~taken[nodes]]
                if len(free):
                    pick = int(free[0])
                    break
            if pick < 0:
                done, why = i, (2 if (W and kept[i][1] and not more[i]) or (W and len(lists[i]) > len(kept[i][0])) else 1)
                break
            taken[pick] = True
            k = (pos + i) % S
            cpu[pick] -= wl.svc_cpu[k]
            mem[pick] -= wl.svc_mem[k]
            total[pick] += 1
            on[k, pick] = True
        if done == 0:
            raise SystemExit("the model made no progress at task %d" % pos)
        cut_list += why == 1
        cut_win += why == 2
        pos += done
        rounds += 1
    return rounds, cut_list, cut_win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--rows", default=DEFAULT_ROWS)
    args = ap.parse_args()
    wl = synth.Workload("cfg3", T=args.T, N=args.N)
    rows = static_rows(wl)
    print("| block | list (half-words) | window | lookahead | rounds | cut at an exhausted list / window |")
    print("|---|---|---|---|---|---|")
    for spec in args.rows.split(","):
        B, H, W, look = (int(x) for x in spec.split(":"))
        t0 = time.time()
        r, cl, cw = rounds_for(wl, rows, B, H, W, look)
        print("| %d | %d | %s | %d | %d | %d / %d |   (%.0f s)" % (B, H, W or "all", look, r, cl, cw, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
