# -*- coding: utf-8 -*-
"""Which kernels a build of one .hip file holds, and whether two builds hold the same machine code.

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 --save-temps=obj -c oriana_amd/csrc/passes.hip -o DIR/passes.o
    python tools/kernel_audit.py list DIR/passes-hip-amdgcn-amd-amdhsa-gfx950.out > A.txt
    python tools/kernel_audit.py diff A.txt B.txt          # exit status 1 if B has a kernel A lacks, or a common one differs

`list` prints one line per kernel of the device code object: demangled name, sha1 of its instruction stream (llvm-objdump -d
without addresses and encodings, symbol references dropped), instruction count, and the resource directives of its
.amdhsa_kernel block in the assembly file --save-temps leaves beside the code object (next free VGPR / SGPR, accumulator
offset, LDS and scratch bytes).  `diff` reports the kernels only in A (removed), only in B (new) and the common ones whose
line differs.
"""
import hashlib
import os
import re
import subprocess
import sys

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
RES = ('next_free_vgpr', 'next_free_sgpr', 'accum_offset', 'group_segment_fixed_size', 'private_segment_fixed_size')


def listing(out_path):
    sh = lambda *cmd: subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    table = sh(os.path.join(LLVM, 'llvm-readelf'), '--symbols', '-W', out_path)
    syms = set(re.findall(r'(\S+)\.kd$', table, re.M))
    # (address, size) of each kernel: the bytes between two symbols are alignment padding, which objdump decodes as well
    span = {m.group(3): (int(m.group(1), 16), int(m.group(2))) for m in re.finditer(r'^\s*\d+: ([0-9a-f]+)\s+(\d+) FUNC .* (\S+)$', table, re.M)}
    streams, cur, end = {}, None, 0
    for line in sh(os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', out_path).split('\n'):
        m = re.match(r'<(\S+)>:$', line)
        if m:
            cur = streams.setdefault(m.group(1), []) if m.group(1) in syms else None
            end = sum(span.get(m.group(1), (0, 0)))
        elif cur is not None and line.startswith('\t') and '//' in line and int(line.split('//')[1].split(':')[0], 16) < end:
            cur.append(re.sub(r'<[^>]*>', '', line.split('//')[0]).strip())
    res = {}
    asm = out_path[:-len('.out')] + '.s'
    for name, body in re.findall(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S):
        res[name] = ' '.join('%s=%s' % (k, re.search(r'\.amdhsa_%s (\S+)' % k, body).group(1)) for k in RES)
    names = sh('c++filt', *sorted(syms)).split('\n')
    for sym, name in sorted(zip(sorted(syms), names), key=lambda p: p[1]):
        name = name.split('(')[0].replace('void ', '').replace('oriana::', '').replace(', ', ',')
        print('%s  %s  insns=%d  %s' % (name, hashlib.sha1('\n'.join(streams[sym]).encode()).hexdigest()[:16], len(streams[sym]), res[sym]))


def diff(a_path, b_path):
    load = lambda p: dict(l.split('  ', 1) for l in open(p).read().split('\n') if '  ' in l)
    A, B = load(a_path), load(b_path)
    removed, new = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    changed = sorted(k for k in set(A) & set(B) if A[k] != B[k])
    print('%d kernels in %s, %d in %s: %d removed, %d new, %d of the %d common ones differ' % (
        len(A), a_path, len(B), b_path, len(removed), len(new), len(changed), len(set(A) & set(B))))
    for k in changed:
        print('DIFFERENT %s\n    - %s\n    + %s' % (k, A[k], B[k]))
    for k in new:
        print('NEW %s' % k)
    for k in removed:
        print('removed %s' % k)
    return 1 if new or changed else 0


if __name__ == '__main__':
    if sys.argv[1] == 'list':
        listing(sys.argv[2])
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
