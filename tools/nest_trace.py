# -*- coding: utf-8 -*-
"""The launch sequence of every C entry that runs a whole loop nest, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/nest_trace.py run LABELS.txt
    python tools/nest_trace.py list DIR LABELS.txt > A.txt          # ordered (kernel, grid, block) per entry
    python tools/nest_trace.py diff A.txt B.txt                     # exit status 1 if any entry differs

`run` calls the four resident entries (unit-declared and general D_hat, with and without the index quirk of zigap.py:94 and
the third output, where the entry allows) on a sliced and a hybrid handle and the four stateless entries, at K = 20, 64, 100;
every call is preceded by a marker launch (oriana_trigamma_f64 over 256 * index elements) that `list` splits the trace at.
ORIANA_CUS=2 in the environment makes the plans of the small matrix split the last round (row split + dense tail).
"""
import csv
import ctypes
import difflib
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(labels_path):
    import numpy as np
    import torch
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    st = stream_ptr()
    labels = []
    mark_in = torch.ones(256 * 400, dtype=torch.float64, device='cuda')
    mark_out = torch.empty_like(mark_in)

    def entry(label, fn, *args):
        torch.cuda.synchronize()
        labels.append(label)
        assert lib.oriana_trigamma_f64(ptr(mark_out), ptr(mark_in), 256 * len(labels), st) == 0
        rc = fn(*args)
        assert rc == 0, (label, rc)
        torch.cuda.synchronize()

    n, m = 1700, 1100
    for K in (20, 64, 100):
        rng = np.random.default_rng(K)
        dens = rng.beta(1.0, 3.0, size=m)
        X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
        D = rng.random((n, m)).astype(np.float32)
        D[X != 0] = 1.0
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        Xd, Dd, Dg = d(X), d(D), d(rng.random((n, m)))
        lu, lv = d(rng.normal(size=(n, K))), d(rng.normal(size=(m, K)))
        St, Sh = d(rng.random((m, K)) < 0.7), d(rng.random((m, K)))
        Zi, Zj, Zl = (torch.empty(r, K, device='cuda') for r in (n, m, m))
        for layout, dd in (('sliced', 0.0), ('hybrid', 0.2)):
            h = ctypes.c_void_p(None)
            assert lib.oriana_counts_create_dense_f32(ctypes.addressof(h), ptr(Xd), n, m, m, K, dd, st) == 0
            tag = 'K%d %s ' % (K, layout)
            entry(tag + 'gap_resident', lib.oriana_zq_gap_resident, h, ptr(Zi), ptr(Zj), ptr(lu), ptr(lv), st)
            for unit in (1, 0):
                if not unit and dd > 0:
                    continue                                      # (a hybrid handle serves the twins under the declaration only)
                assert lib.oriana_counts_declare_unit_dropout(h, unit) == 0
                w = tag + ('unit ' if unit else 'general ')
                Dx = Dd if unit else Dg
                for quirk in (0, 1):
                    for zl in (Zl, None):
                        entry(w + 'zigap_resident quirk=%d zlog=%d' % (quirk, zl is not None), lib.oriana_zq_zigap_resident, h, ptr(Zi),
                              ptr(Zj), ptr(zl), ptr(lu), ptr(lv), ptr(Dx), quirk, st)
                entry(w + 'sparse_gap_resident', lib.oriana_zq_sparse_gap_resident, h, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv),
                      ptr(St), ptr(Sh), st)
                entry(w + 'sparse_zigap_resident', lib.oriana_zq_sparse_zigap_resident, h, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv),
                      ptr(St), ptr(Sh), ptr(Dx), st)
            assert lib.oriana_counts_destroy(h) == 0
        nbytes = lib.oriana_zq_workspace_bytes(n, m, K, int(np.count_nonzero(X)))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
        wp = (ws.data_ptr() + 255) // 256 * 256
        tag = 'K%d stateless ' % K
        entry(tag + 'gap_f32', lib.oriana_zq_gap_f32, ptr(Zi), ptr(Zj), ptr(lu), ptr(lv), ptr(Xd), n, m, K, wp, nbytes, st)
        for quirk in (0, 1):
            entry(tag + 'zigap_f32 quirk=%d' % quirk, lib.oriana_zq_zigap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(Dg),
                  ptr(Xd), n, m, K, quirk, wp, nbytes, st)
        entry(tag + 'sparse_gap_f32', lib.oriana_zq_sparse_gap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(St), ptr(Sh),
              ptr(Xd), n, m, K, wp, nbytes, st)
        entry(tag + 'sparse_zigap_f32', lib.oriana_zq_sparse_zigap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(St), ptr(Sh),
              ptr(Dg), ptr(Xd), n, m, K, wp, nbytes, st)
    entry('end', lambda: 0)
    with open(labels_path, 'w') as f:
        f.write('\n'.join(labels) + '\n')


def listing(trace_dir, labels_path):
    """One line per entry: its launches in order as `kernel grid/block` (dimensions of 1 dropped, hipMemsetAsync = memset)."""
    labels = open(labels_path).read().split('\n')
    rows = []
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dims = lambda v: 'x'.join(str(x) for x in v if x != 1) or '1'
    out = []
    for r in rows:
        name = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('oriana::', '').replace(', ', ',')
        name = name.replace('__amd_rocclr_fillBufferAligned', 'memset')
        block = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        grid = [int(r['Grid_Size_' + a]) // max(bl, 1) for a, bl in zip('XYZ', block)]
        if 'k_map_f64<1>' in name:
            if labels[grid[0] - 1] == 'end':
                break
            out.append([labels[grid[0] - 1]])
        elif out:
            out[-1].append('%s %s/%s' % (name, dims(grid), dims(block)))
    for e in out:
        print('%s: %s' % (e[0], ' | '.join(e[1:])))


def diff(a_path, b_path):
    load = lambda p: {l.split(': ', 1)[0]: l.split(': ', 1)[1].split(' | ') for l in open(p).read().split('\n') if ': ' in l}
    A, B = load(a_path), load(b_path)
    same, kinds = [], {}
    for k in A:
        if A[k] == B.get(k):
            same.append(k)
            continue
        d = '\n'.join('    ' + l for l in difflib.unified_diff(A[k], B.get(k, []), lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('---', '+++'))
        kinds.setdefault(d, []).append(k)
    print('same (%d): %s' % (len(same), '; '.join(same)))
    for d, ks in kinds.items():               # entries with the same removed (-) and added (+) launches, once
        print('DIFFERENT (%d): %s\n%s' % (len(ks), '; '.join(ks), d))
    print('%d entries, %d differ' % (len(A), len(A) - len(same)))
    return 1 if len(same) != len(A) or set(A) != set(B) else 0


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2])
    elif sys.argv[1] == 'list':
        listing(sys.argv[2], sys.argv[3])
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
