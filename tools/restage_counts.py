"""Instructions of the restaging of a sliced K = 100 kernel -- from the header of its tile loop to the SECOND barrier inside it
(Stage::load, the barrier, Stage::store; with them whatever else the kernel does there: slice bookkeeping, the record prefetch)
-- in a hipcc -S listing of csrc/passes.hip, by class (the design tool of DESIGN.md section 9, "restaging"; sibling of
step_counts.py).
usage: restage_counts.py listing.s [KERNEL_PREFIX ...]
The tile loop is the innermost loop around the kernel's first s_barrier.  The region is WALKED, not scanned: an unconditional
branch is followed, a branch on the exec mask goes where lanes are active (the masked body is counted, the instruction itself
under "exec save/restore" or "branch"), and a scalar conditional branch (scc / vcc: wave-uniform) forks the walk -- every
distinct path to the second barrier is reported (one that leaves the loop or the kernel first is dropped) with the branch
directions that select it (T = taken).  A path with a v_mul_hi (the division of every element's index by 24) is the
per-element one -- the ragged tile, or every tile of the parent --, the others form their addresses from the thread's three
classes.  Also printed: the kernel's register, scratch and occupancy lines from the listing's own metadata comments."""
import re, sys

DEFAULT = ['_ZN6oriana4k10015k_row_pass_k100ILi1ELi0E', '_ZN6oriana4k10015k_row_pass_k100ILi1ELi1E',
           '_ZN6oriana4k10015k_row_pass_k100ILi1ELi2E', '_ZN6oriana4k10015k_row_pass_k100ILi0ELi0E',
           '_ZN6oriana11k_col_pass2ILi6ELi1ELb0E', '_ZN6oriana11k_col_pass2ILi6ELi0ELb0E']
MAX_PATHS = 256


def op_of(line):
    m = re.match(r'\s+([a-z_0-9]+)', line)
    return m.group(1) if m else None


def classify(op, line):
    if op == 'v_mad_u64_u32' or op == 'v_mad_i64_i32':
        return 'v_mad_u64_u32'
    if op.startswith('v_mul_hi_'):
        return 'v_mul_hi'
    if re.match(r'v_cmpx?_\w+_[iu]64', op):
        return 'v_cmp 64-bit'
    if op.startswith('v_'):
        return 'valu (other)'
    if op.startswith('ds_write') or op.startswith('ds_store'):
        return 'lds write'
    if op.startswith('ds_'):
        return 'lds other'
    if op.startswith(('global_load', 'buffer_load', 'flat_load', 's_load', 's_buffer_load')):
        return 'loads (s_load incl.)' if op.startswith('s_') else 'vmem load'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem other'
    if op.startswith(('s_waitcnt', 's_nop', 's_barrier')):
        return 'wait/nop/barrier'
    if op.startswith(('s_cbranch', 's_branch')):
        return 'branch'
    if 'saveexec' in op or (op.startswith('s_') and re.search(r'\bexec\b', line.split(';')[0])):
        return 'exec save/restore'
    if op.startswith('s_'):
        return 'salu (other)'
    return 'other'


def kernel_span(lines, prefix):
    start = [i for i, l in enumerate(lines) if l.startswith(prefix)][0]
    end = [i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end')][0]
    return start, end


def walk(lines, prefix):
    start, end = kernel_span(lines, prefix)
    labels = {m.group(1): i for i in range(start, end) for m in [re.match(r'^(\.LBB\d+_\d+):', lines[i])] if m}
    b1 = [i for i in range(start, end) if op_of(lines[i]) == 's_barrier'][0]
    head = -1
    for i in range(b1, end):
        m = re.match(r'\s+s_c?branch\w*\s+(\.LBB\d+_\d+)', lines[i])
        if m and labels[m.group(1)] < b1:
            head = max(head, labels[m.group(1)])
    assert head >= 0, 'no loop around the first barrier'
    paths = {}
    todo = [(head, 0, {}, '')]
    n = 0
    while todo and n < MAX_PATHS:
        i, barriers, cnt, dirs = todo.pop()
        cnt = dict(cnt)
        steps = 0
        left = False
        while True:
            steps += 1
            assert start <= i < end and steps < 100000, 'the walk left the kernel'
            l = lines[i]
            op = op_of(l)
            if op is None or l.lstrip().startswith((';', '.')):
                i += 1
                continue
            if op == 's_endpgm' or (i == head and steps > 1):     # the way out of the tile loop, or round to its header
                left = True
                break
            k = classify(op, l)
            cnt[k] = cnt.get(k, 0) + 1
            if op == 's_barrier':
                barriers += 1
                if barriers == 2:
                    break
            m = re.match(r'\s+(s_c?branch\w*)\s+(\.LBB\d+_\d+)', l)
            if m:
                tgt = labels[m.group(2)]
                if op == 's_branch':
                    i = tgt
                    continue
                if op == 's_cbranch_execnz':
                    i = tgt
                    continue
                if op == 's_cbranch_execz':
                    i += 1
                    continue
                todo.append((tgt, barriers, dict(cnt), dirs + 'T'))       # scalar condition: both ways
                dirs += 'n'
            i += 1
        n += 1
        if left:
            continue
        sig = tuple(sorted(cnt.items()))
        paths.setdefault(sig, []).append(dirs)
    return paths, bool(todo)


def resources(lines, prefix):
    start, end = kernel_span(lines, prefix)
    out = []
    for l in lines[end:end + 80]:
        m = re.match(r';\s*(NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize)\s*:\s*(\S+)', l)
        if m:
            out.append('%s %s' % (m.group(1), m.group(2)))
    return ', '.join(out)


def main():
    lines = open(sys.argv[1]).read().split('\n')
    for prefix in sys.argv[2:] or DEFAULT:
        paths, cut = walk(lines, prefix)
        print(prefix)
        print('    ' + resources(lines, prefix))
        order = ['valu (other)', 'v_mad_u64_u32', 'v_mul_hi', 'v_cmp 64-bit', 'salu (other)', 'exec save/restore', 'branch',
                 'vmem load', 'loads (s_load incl.)', 'vmem other', 'lds write', 'lds other', 'wait/nop/barrier', 'other']
        for sig, dirs in sorted(paths.items(), key=lambda kv: sorted(kv[1])[0]):
            cnt = dict(sig)
            kind = 'per-element path' if cnt.get('v_mul_hi') else 'class path'
            valu = sum(cnt.get(k, 0) for k in order[:4])
            print('    %s [%d way(s), e.g. %s]: VALU %d' % (kind, len(dirs), sorted(dirs)[0] or '-', valu))
            print('        ' + ', '.join('%s %d' % (k, cnt[k]) for k in order if cnt.get(k)))
        if cut:
            print('    (more than %d paths: the walk was cut)' % MAX_PATHS)


if __name__ == '__main__':
    main()
