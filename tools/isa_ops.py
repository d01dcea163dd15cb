#!/usr/bin/env python3
"""Instruction histogram of one kernel in a hipcc -S listing.
Usage: tools/isa_ops.py file.s mangled-substring [topN] [--barriers A:B]

--barriers A:B counts only the lines between the kernel's A-th and B-th
s_barrier in listing order (1-based; B may be 'last').  k_inv_fast's fast
path is inlined ahead of the exact tile code, so its fast path is 1:3 with
the a-priori certificate and 1:4 without."""
import collections
import sys

args = sys.argv[1:]
bar = None
if '--barriers' in args:
    k = args.index('--barriers')
    bar = args[k + 1].split(':')
    del args[k:k + 2]
s = open(args[0]).read()
key = args[1]
top = int(args[2]) if len(args) > 2 else 40
name_line = [ln for ln in s.splitlines() if key in ln and ln.split(';')[0].rstrip().endswith(':')
             and not ln.startswith('.')][0]
i = s.index('\n' + name_line) + 1
j = s.index('.Lfunc_end', i)
lines = s[i:j].splitlines()
if bar:
    at = [n for n, ln in enumerate(lines) if ln.strip().startswith('s_barrier')]
    a = at[int(bar[0]) - 1]
    b = at[-1] if bar[1] == 'last' else at[int(bar[1]) - 1]
    lines = lines[a + 1:b]
    print(f'(between barrier {bar[0]} and {bar[1]} of {len(at)}: {len(lines)} lines)')
ops = collections.Counter()
for line in lines:
    t = line.strip().split()
    if not t or t[0].startswith(('.', ';')) or t[0].endswith(':'):
        continue
    ops[t[0]] += 1
cls = collections.Counter()
for k, v in ops.items():
    c = 'valu_f64' if k.startswith('v_') and 'f64' in k else 'valu' if k.startswith('v_') else \
        'salu' if k.startswith('s_') else 'lds' if k.startswith('ds_') else 'vmem' if k.startswith(('global_', 'buffer_', 'scratch_')) else 'other'
    cls[c] += v
print(name_line, 'total', sum(ops.values()), dict(cls))
for k, v in ops.most_common(top):
    print(f'{k:28s}{v}')
