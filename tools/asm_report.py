#!/usr/bin/env python3
"""Developer aid: per-kernel register use and instruction histogram from `make -C swarmkit_amd/csrc asm [ASM_TU=swp_resolve6]` (the pair
kernels k_fit_pairs / k_fit_pairs_vol are built in swp_resolve6.hip, k_check_pair and k_explain in swp_engine.hip)."""
import glob
import re
import sys
from collections import Counter

d = '/tmp/swp_asm/'
txt = open(d + 'resource_usage.txt').read()
pat = sys.argv[1] if len(sys.argv) > 1 else 'k_explain'
for b in re.split(r'Function Name: ', txt)[1:]:
    name = b.split()[0]
    if pat not in name:
        continue
    def g(k):
        m = re.search(k + r': (\d+)', b)
        return m.group(1) if m else '?'
    print(name[:56].ljust(56), 'VGPR', g('VGPRs'), 'SGPR', g('TotalSGPRs'), 'scratch', g(r'ScratchSize \[bytes/lane\]'), 'occ', g(r'Occupancy \[waves/SIMD\]'),
          'spillV', g('VGPRs Spill'))
sym = sys.argv[2] if len(sys.argv) > 2 else '_ZN6swpdev9k_explainENS_11ExplainArgsE'
s = next(t for t in (open(f).read() for f in sorted(glob.glob(d + '*-hip-amdgcn-amd-amdhsa-gfx950.s'))) if sym + ':' in t)   # (the translation unit last built there)
i = s.index(sym + ':')
j = s.index('.end_amdhsa_kernel', i) if '.end_amdhsa_kernel' in s[i:] else len(s)
lines = s[i:j].split('\n')
c = Counter()
for l in lines:
    l = l.strip()
    if not l or l.startswith(';') or l.startswith('.') or l.endswith(':'):
        continue
    c[l.split()[0]] += 1
print(sum(c.values()), 'instrs in', sym)
for k, v in c.most_common(int(sys.argv[3]) if len(sys.argv) > 3 else 30):
    print('  ', k, v)
print('vmcnt(0):', sum(1 for l in lines if 'vmcnt(0)' in l), ' any waitcnt:', sum(1 for l in lines if 's_waitcnt' in l))
