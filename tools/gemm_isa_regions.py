#!/usr/bin/env python
"""Static instruction counts of the persistent GEMM (gemm_kernel_p) inside and outside its k-loop, from a listing made with the
Makefile's flags (hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize --cuda-device-only -S gemm.hip):
  before 1st MFMA = the kernel's prologue and the top of a k-tile, which in a tile's last k-tile holds the next tile's operand bases,
  k-loop       = from the first to the last v_mfma of the function,
  epilogue     = from the last v_mfma to the last global store of the function,
  after stores = the rest of the function: accumulator clears, the walk's successor, the next tile's first wait.
An instantiation with the straight-line epilogue (template argument SL bit 0) holds two epilogues, the unpredicated one of
interior tiles and the predicated one of edge tiles; the region is then split at the wave-uniform branch between them (the
block with more exec regions is the edge form) and both parts are printed.
Per region: instructions, VALU, SALU, LDS, VMEM, the exec-mask regions (s_*_saveexec, s_cbranch_execz), the integer multiplies
and 64-bit address instructions, s_nop; per function the VGPR / SGPR / scratch figures of its metadata.
usage: gemm_isa_regions.py file.s [mangled-name-substring ...]      (default: every gemm_kernel_p instantiation)"""
import re, sys
s = open(sys.argv[1]).read()
keys = sys.argv[2:] or ["gemm_kernel_p"]
names = [m.group(1) for m in re.finditer(r'^(\S+):\s*; @', s, re.M) if all(k in m.group(1) for k in ["gemm_kernel_p"]) and any(k in m.group(1) for k in keys)]
SAVEEXEC = ('s_and_saveexec_b64', 's_andn2_saveexec_b64', 's_or_saveexec_b64')
ADDR = ('v_mul_lo_u32', 'v_mul_hi_u32', 'v_mad_u64_u32', 'v_mad_i64_i32', 'v_lshl_add_u64', 'v_add3_u32', 's_mul_i32', 's_mul_hi_u32', 's_mul_hi_i32', 's_addc_u32', 's_cselect_b32')


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
    n = lambda *ops: sum(op in ops for op in ins)
    return (f"{len(ins):5d} instr  VALU {c['VALU']:4d}  SALU {c['SALU']:4d}  LDS {c['LDS']:3d}  VMEM {c['VMEM']:3d}  "
            f"saveexec {n(*SAVEEXEC):3d}  execz {n('s_cbranch_execz'):3d}  stores {sum(op.startswith('global_store') for op in ins):3d}  "
            f"v_cmp {sum(op.startswith('v_cmp') for op in ins):3d}  mul/addr64 {n(*ADDR):3d}  s_nop {n('s_nop'):3d}")


for name in names:
    i = s.index(name + ':'); j = s.index('.Lfunc_end', i)
    ins, blocks = [], []  # blocks: index of the first instruction behind every label
    for l in s[i:j].split('\n'):
        t = l.strip()
        if t.startswith(('.LBB', '; %bb.')):
            blocks.append(len(ins))
        if not t or t.startswith((';', '.')) or t.endswith(':'):
            continue
        ins.append(t.split()[0])
    meta = s[i:s.index('.end_amdhsa_kernel', i)]
    g = lambda k: (re.search(r'\.amdhsa_' + k + r'\s+(\d+)', meta) or [None, '?'])[1]
    mf = [n for n, op in enumerate(ins) if op.startswith('v_mfma')]
    st = [n for n, op in enumerate(ins) if op.startswith('global_store')]
    print(name)
    lanes = sum(op in ('v_writelane_b32', 'v_readlane_b32') for op in ins)
    print(f"  VGPRs {g('next_free_vgpr')}  SGPRs {g('next_free_sgpr')}  scratch {g('private_segment_fixed_size')} B  v_writelane / v_readlane (SGPRs parked in VGPR lanes) {lanes}")
    print("  before 1st MFMA:   " + count(ins[:mf[0]]))
    print("  k-loop:            " + count(ins[mf[0]:mf[-1] + 1]))
    epi = (mf[-1] + 1, st[-1] + 1)
    print("  epilogue:          " + count(ins[epi[0]:epi[1]]))
    # the two epilogues of a straight-line instantiation: the interior form runs from the first to the last basic block that holds
    # two or more stores (the edge form has one store per exec region, so one per block); the rest of the region is the edge form
    bl = [b for b in blocks if epi[0] <= b < epi[1]]
    edges = [epi[0]] + bl + [epi[1]]
    segs = [(a, b) for a, b in zip(edges, edges[1:]) if b > a]
    has = [any(op.startswith('global_store') for op in ins[a:b]) for a, b in segs]
    dense = [sum(op.startswith('global_store') for op in ins[a:b]) >= 2 for a, b in segs]
    if any(dense) and not all(d or not h for d, h in zip(dense, has)):
        k0 = min(n for n, d in enumerate(dense) if d); k1 = max(n for n, d in enumerate(dense) if d)
        if k1 + 1 < len(segs) and has[k1 + 1]: k1 += 1  # (the last slab's partial chunk: one store in its own exec region)
        inter = ins[segs[k0][0]:segs[k1][1]]
        edge = ins[epi[0]:segs[k0][0]] + ins[segs[k1][1]:epi[1]]
        print("    interior form:   " + count(inter))
        print("    edge form, rest: " + count(edge))
    print("  after the stores:  " + count(ins[st[-1] + 1:]))
