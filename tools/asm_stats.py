#!/usr/bin/env python3
"""Instruction statistics of one kernel in a hipcc -S listing.

usage: asm_stats.py file.s kernel-substring
Prints per-basic-block instruction counts (largest blocks first) and the opcode mix of
the hottest block, which for the fused kernels is the Picard iteration body.

usage: asm_stats.py --mnemonics file.s kernel-substring
Prints the kernel's resource metadata and its multiset of instruction mnemonics, one per line:
diff the output for two builds to see whether a refactoring left the generated code alone.
"""
import re, sys
from collections import Counter

META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
        'private_segment_fixed_size', 'group_segment_fixed_size')

def mnemonics(lines, start, end):
    name = lines[start].split(':')[0]
    meta = next(b for b in '\n'.join(lines).split('\n  - .agpr_count:')[1:] if re.search(r'\.name: +' + re.escape(name) + r'\n', b))
    for k in META:
        print(f'.{k}', re.search((r'^ +(\d+)' if k == 'agpr_count' else rf'\.{k}: +(\d+)'), meta).group(1))
    ops = Counter(t.split()[0] for t in (l.strip() for l in lines[start + 1:end])
                  if t and not t.startswith((';', '.')) and not t.endswith(':'))
    for k in sorted(ops):
        print(k, ops[k])

def main():
    mn = sys.argv[1] == '--mnemonics'
    path, key = sys.argv[1 + mn], sys.argv[2 + mn]
    lines = open(path).read().split('\n')
    start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and l.rstrip().endswith(tuple([':'])) or (l.startswith('_Z') and key in l and ': ' in l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith('.Lfunc_end'))
    if mn:
        return mnemonics(lines, start, end)
    blocks, cur, name = [], [], 'entry'
    for l in lines[start + 1:end]:
        t = l.strip()
        if not t or t.startswith(';'):
            continue
        if re.match(r'^\.LBB[\w_]+:', t):
            blocks.append((name, cur)); cur = []; name = t.split(':')[0]
            continue
        if t.startswith('.'):
            continue
        cur.append(t.split()[0])
    blocks.append((name, cur))
    tot = sum(len(b) for _, b in blocks)
    print(f'total instructions: {tot}')
    for n, b in sorted(blocks, key=lambda x: -len(x[1]))[:6]:
        c = Counter(b)
        valu = sum(v for k, v in c.items() if k.startswith('v_'))
        f64 = sum(v for k, v in c.items() if k.endswith('_f64'))
        print(f'\nblock {n}: {len(b)} instr, VALU {valu}, f64 {f64}, salu {sum(v for k,v in c.items() if k.startswith("s_"))}, ds {sum(v for k,v in c.items() if k.startswith("ds_"))}')
        print('  ' + ', '.join(f'{k}:{v}' for k, v in c.most_common(24)))

main()
