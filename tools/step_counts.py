"""VALU instructions of the steady-state iteration (four unrolled steps) of the sliced K = 100 kernels in a hipcc -S
listing of csrc/passes.hip, by opcode (the design tool of the "step diet").
usage: step_counts.py listing.s [KERNEL_PREFIX READS_PER_ITERATION] ...
The steady-state body is the shortest loop of the kernel that holds exactly READS_PER_ITERATION ds_read_b128; a stretch
that a forward `s_cbranch_scc1` inside the body jumps over (the wave-uniform slow-path branch, taken when no lane failed
the den test) is not on the hot path and is left out."""
import re, sys

DEFAULT = [('_ZN6oriana4k10015k_row_pass_k100ILi1ELi0E', 48), ('_ZN6oriana4k10015k_row_pass_k100ILi1ELi2E', 48),
           ('_ZN6oriana4k10015k_row_pass_k100ILi1ELi1E', 48), ('_ZN6oriana11k_col_pass2ILi6ELi1ELb0E', 24)]


def body(lines, prefix, reads):
    start = [i for i, l in enumerate(lines) if l.startswith(prefix)][0]
    end = [i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end')][0]
    labels = {m.group(1): i for i in range(start, end) for m in [re.match(r'^(\.LBB\d+_\d+):', lines[i])] if m}
    best = None
    for i in range(start, end):
        m = re.match(r'\s+s_c?branch\w*\s+(\.LBB\d+_\d+)', lines[i])
        if m and labels.get(m.group(1), i) < i:
            h = labels[m.group(1)]
            n = sum(1 for l in lines[h:i + 1] if re.match(r'\s+ds_read_b128', l))
            if n == reads and (best is None or i - h < best[1] - best[0]):
                best = (h, i)
    out, skip_to = [], None
    for l in lines[best[0]:best[1] + 1]:
        if skip_to:
            if l.startswith(skip_to + ':'):
                skip_to = None
            continue
        out.append(l)
        m = re.match(r'\s+s_cbranch_scc1\s+(\.LBB\d+_\d+)', l)
        if m and best[0] < labels[m.group(1)] <= best[1] and labels[m.group(1)] > best[0] + len(out):
            skip_to = m.group(1)
    return out


def main():
    lines = open(sys.argv[1]).read().split('\n')
    args = sys.argv[2:]
    todo = [(args[i], int(args[i + 1])) for i in range(0, len(args), 2)] or DEFAULT
    for prefix, reads in todo:
        kinds, valu = {}, {}
        for l in body(lines, prefix, reads):
            m = re.match(r'\s+([a-z_0-9]+)', l)
            if not m:
                continue
            op = m.group(1)
            k = ('v_pk_fma' if op.startswith('v_pk_fma') else 'lds' if op.startswith('ds_') else
                 'vmem' if op.startswith(('global_', 'buffer_')) else 'valu' if op.startswith('v_') else
                 'wait/nop' if op.startswith(('s_waitcnt', 's_nop')) else 'salu' if op.startswith('s_') else 'other')
            kinds[k] = kinds.get(k, 0) + 1
            if k == 'valu':
                valu[op] = valu.get(op, 0) + 1
        print(prefix, '(4 steps)')
        print('   ', ', '.join('%s %d' % kv for kv in sorted(kinds.items())))
        print('    other VALU by opcode:', ', '.join('%s %d' % kv for kv in sorted(valu.items(), key=lambda x: (-x[1], x[0]))))
        print('    VALU per step: %.2f (%.2f without the packed FMAs)'
              % ((kinds.get('valu', 0) + kinds.get('v_pk_fma', 0)) / 4.0, kinds.get('valu', 0) / 4.0))


if __name__ == '__main__':
    main()
