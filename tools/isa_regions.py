#!/usr/bin/env python
"""Static instruction counts of the fused to_qkv + attention kernel's phases outside its MFMA loops, from a listing made with
the Makefile's flags (hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize --cuda-device-only -S qkv_attn.hip):
  hand-off, one region per column half = from the last v_mfma_f32_16x16x32 of a k-loop copy to the next MFMA of the listing
            (the first region therefore also holds the second copy's k-loop preamble),
  output stage = from the last v_mfma_f32_32x32x16 of the attention core to the end of the kernel.
Per region: instructions, VALU, SALU, LDS, VMEM, the exec-mask regions (s_*_saveexec, s_cbranch_execz)
and the LDS write instructions (a ds_write2 carries two stores).
usage: isa_regions.py file.s [mangled-name-substring ...]      (default: every qkv_attn_kernel instantiation)"""
import re, sys
s = open(sys.argv[1]).read()
keys = sys.argv[2:] or ["qkv_attn_kernel"]
names = [m.group(1) for m in re.finditer(r'^(\S+):\s*; @', s, re.M) if any(k in m.group(1) for k in keys)]


def cls(op):
    if op.startswith('v_mfma'): return 'MFMA'
    if op.startswith('ds_'): return 'LDS'
    if op.startswith(('global_', 'buffer_', 'scratch_', 'flat_')): return 'VMEM'
    if op.startswith('v_'): return 'VALU'
    if op.startswith('s_'): return 'SALU'
    return 'other'


def count(ins):
    c = {k: 0 for k in ('VALU', 'SALU', 'LDS', 'VMEM')}
    for op in ins:
        k = cls(op)
        if k in c: c[k] += 1
    ex = sum(op in ('s_and_saveexec_b64', 's_andn2_saveexec_b64', 's_or_saveexec_b64') for op in ins)
    return (f"{len(ins):5d} instr  VALU {c['VALU']:4d}  SALU {c['SALU']:4d}  LDS {c['LDS']:3d}  VMEM {c['VMEM']:3d}  "
            f"saveexec {ex:3d}  execz {sum(op == 's_cbranch_execz' for op in ins):3d}  ds_write* {sum(op.startswith('ds_write') for op in ins):3d} (write2 {sum(op.startswith('ds_write2') for op in ins):3d})")


for name in names:
    i = s.index(name + ':'); j = s.index('.Lfunc_end', i)
    ins = []
    for l in s[i:j].split('\n'):
        t = l.strip()
        if not t or t.startswith((';', '.')) or t.endswith(':'):
            continue
        ins.append(t.split()[0])
    mf = [n for n, op in enumerate(ins) if op.startswith('v_mfma')]
    k16 = [n for n in mf if '16x16x32' in ins[n]]
    # a k-loop copy ends where the next MFMA of the listing is farthest away: behind the hand-off (the two largest gaps)
    ends = sorted(sorted(k16, key=lambda n: mf[mf.index(n) + 1] - n)[-2:])
    print(name)
    for c, n in enumerate(ends):
        nxt = mf[mf.index(n) + 1]
        print(f"  hand-off, copy {c}: " + count(ins[n + 1:nxt]))
    print("  output stage:     " + count(ins[mf[-1] + 1:]))
