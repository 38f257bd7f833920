#!/usr/bin/env python
"""Are two builds of one source file the same device code?  Compares two `hipcc --cuda-device-only -S` files kernel by kernel:
the instruction body and the .amdhsa_kernel block of every symbol, whatever order the kernels were emitted in (the function index
of local labels, .LBB<n>_<m> / .Lfunc_end<n>, is dropped, and so are comments).  Prints added, removed and differing kernels;
exit status 1 if any.
usage: isa_same.py old.s new.s"""
import re, sys


def kernels(path):
    s = re.sub(r'[ \t]*;.*', '', open(path).read())  # (comments name basic blocks by function index too: "in Loop: Header=BB24_33")
    s = re.sub(r'\.LBB\d+_', '.LBB_', s)
    s = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', s)
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel', s, re.M | re.S):
        name = m.group(1)
        i = s.index('\n' + name + ':')
        out[name] = (s[i:s.index('.Lfunc_end', i)], m.group(0))
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
differ = []
for name in sorted(set(old) & set(new)):
    what = [w for w, a, b in zip(('body', 'descriptor'), old[name], new[name]) if a != b]
    if what: differ.append(f'{name}: {" and ".join(what)}')
for title, names in (('removed', removed), ('added', added), ('differing', differ)):
    for n in names: print(f'{title}: {n}')
print(f'{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {len(added)} added, {len(removed)} removed, {len(differ)} differing')
sys.exit(1 if removed or added or differ else 0)
