#!/usr/bin/env python3
"""tools/isa_same.py A.s B.s -- are the kernels of two device assemblies (hipcc -S --offload-device-only) the same code?
Per kernel symbol (an .amdhsa_kernel entry) the body from its label to .Lfunc_end (the slicing of
tools/isa_blocks2.py) and its .amdhsa_ block are compared as text, comment lines and trailing comments left out.
Prints `N compared, M identical` and the names that differ; exit status 1 if any differ, the symbol sets differ or
there was nothing to compare."""
import re
import sys


def strip(text):
    lines = (l.split(';')[0].rstrip() for l in text.split('\n'))
    return [l for l in lines if l.strip()]


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', s, re.M | re.S):
        name = m.group(1)
        lab = re.search(r'^%s:[^\n]*\n' % re.escape(name), s, re.M)
        body = s[lab.end():s.index('.Lfunc_end', lab.end())]
        out[name] = (strip(body), strip(m.group(2)))
    return out


if len(sys.argv) != 3:
    sys.exit(__doc__)
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
common = sorted(set(a) & set(b))
differ = [n for n in common if a[n] != b[n]]
print('%d compared, %d identical' % (len(common), len(common) - len(differ)))
for n in differ:
    print('differs: %s (%s)' % (n, ' and '.join(w for w, i in (('body', 0), ('.amdhsa_', 1)) if a[n][i] != b[n][i])))
for n in sorted(set(a) ^ set(b)):
    print('only in %s: %s' % (sys.argv[1] if n in a else sys.argv[2], n))
sys.exit(1 if differ or set(a) != set(b) or not common else 0)
