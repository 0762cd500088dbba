"""CPU model of the block resolver's rounds with LATE-STAGED list windows (swp_resolve6.hpp, r6_commit_t): how many rounds does the
headline workload take for a block size, a list length, a window length and a staging lookahead?  Decides the next block / list /
window choice without a GPU, in the style of tools/sim_k7.py.

cfg3 (or a scaled copy) in round-robin order is replayed with the list rule: at a block's start every task of the block lists the first
`list` non-empty 32-node half-words of its feasible plain nodes on their minimum level, behind the share of its identical tasks in
front of it (k_r6_propose's twins); tasks are then decided in order, each taking the first listed node nobody took (every pick
strikes). `window` (0: the whole list in LDS): of a task in 64-task group g >= 2 only the first `window` entries that are live once
group g - `lookahead` is decided are kept; groups 0 and 1 keep the list's first `window` entries. The block is cut at the first task
whose kept entries are all taken — counted as a window cut if entries had been left out — and the next block starts there.

An optional fifth field `:levels` (0: lists of one level, the default; 1: lists over two levels, R6Args.levels2): a list that holds its
whole level (not cut by the list length, the twins' share below the level's candidates) goes on with the task's candidates on the
NEXT level that lie in node words in front of the word of the level's first candidate (taken before the twins' share is passed over),
as far as the list has room. --check compares every pick with the sequential choice recomputed from the full state; --per-round
prints the tasks decided per round.

usage: python tools/sim_window.py [--T 100000] [--N 10000] [--rows 768:32:0:2,1408:64:16:2:1,...] [--workload cfg4] [--check] [--per-round]   (block:list:window:lookahead[:levels])
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


def rounds_for(wl, rows, B, H, W, look, levels=0, check=False, per_round=None):
    N, T, S = wl.N, wl.T, wl.S
    cpu, mem = wl.node_cpu.copy(), wl.node_mem.copy()
    total = np.zeros(N, dtype=np.int64)
    on = np.zeros((S, N), dtype=bool)
    hw_of = np.arange(N) // 32
    pos = rounds = cut_list = cut_win = 0
    wrong = 0
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
            lmin = total[p].min()
            cand = np.flatnonzero(p & (total == lmin))
            h0, used_up = hw_of[cand[0]], twins >= len(cand)
            cand = cand[min(twins, len(cand) - 1):]   # (a level the twins use up lists its last candidate: a cut)
            hws = np.unique(hw_of[cand])
            full = len(hws) > H
            hws = hws[:H]
            entries = [(h, cand[hw_of[cand] == h]) for h in hws]
            if levels and not full and not used_up and len(hws) < H and h0 // 2 > 0:
                up = np.flatnonzero(p[:64 * (h0 // 2)] & (total[:64 * (h0 // 2)] == lmin + 1))
                hws2 = np.unique(hw_of[up])
                full = len(hws2) > H - len(hws)   # (the room cut the second section: bit 31)
                entries += [(h, up[hw_of[up] == h]) for h in hws2[:H - len(hws)]]
            more.append(full)
            lists.append(entries)
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
            if check:
                pn = rows[k] & (cpu >= wl.svc_cpu[k]) & (mem >= wl.svc_mem[k]) & ~on[k]
                best = np.flatnonzero(pn & (total == total[pn].min()))[0]
                wrong += int(best != pick)
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
        if per_round is not None:
            per_round.append(done)
    return rounds, cut_list, cut_win, wrong


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--rows", default=DEFAULT_ROWS)
    ap.add_argument("--workload", default="cfg3", help="synth workload (cfg3, cfg4)")
    ap.add_argument("--check", action="store_true", help="compare every pick with the sequential choice (slower)")
    ap.add_argument("--per-round", action="store_true", help="print the tasks decided per round")
    args = ap.parse_args()
    wl = synth.Workload(args.workload, T=args.T, N=args.N)
    rows = static_rows(wl)
    lv_col = any(len(spec.split(":")) > 4 for spec in args.rows.split(","))   # (rows without the fifth field print as they always did)
    print("| block | list (half-words) | window | lookahead |%s rounds | cut at an exhausted list / window |%s" % (" levels |" if lv_col else "", " wrong picks |" if args.check else ""))
    print("|---|---|---|---|---|---|%s%s" % ("---|" if lv_col else "", "---|" if args.check else ""))
    for spec in args.rows.split(","):
        f = [int(x) for x in spec.split(":")]
        B, H, W, look = f[:4]
        levels = f[4] if len(f) > 4 else 0
        t0 = time.time()
        per = [] if args.per_round else None
        r, cl, cw, wrong = rounds_for(wl, rows, B, H, W, look, levels, args.check, per)
        print("| %d | %d | %s | %d |%s %d | %d / %d |%s   (%.0f s)" % (B, H, W or "all", look, (" %d |" % (1 + levels)) if lv_col else "", r, cl, cw, (" %d of %d |" % (wrong, wl.T)) if args.check else "", time.time() - t0), flush=True)
        if per is not None:
            print("tasks decided per round:", " ".join(str(x) for x in per), flush=True)


if __name__ == "__main__":
    main()
