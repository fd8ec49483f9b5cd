# -*- coding: utf-8 -*-
"""Assemble profiles/sliced_pass_errors.json from the printed figures of the sliced-pass pins:

    python -m pytest tests/test_sliced_pass_gpu.py -q -s > gpu.log       (on an MI355X: the SLICED_PIN lines)
    python -m pytest tests/test_sliced_pass_host.py -q -s > host.log     (CPU: the SLICED_PIN_HOST lines)
    python tools/sliced_pass_report.py gpu.log host.log > profiles/sliced_pass_errors.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def lines(path, tag):
    out, seen = [], set()
    for l in open(path):
        i = l.find(tag + ' {')
        if i >= 0 and l[i:] not in seen:
            seen.add(l[i:])
            out.append(json.loads(l[i + len(tag) + 1:]))
    return out


def main(gpu_log, host_log):
    import sliced_pass_reference as sr
    from helpers import ZLOG_FACTOR, ZLOG_FLOOR
    cases = lines(gpu_log, 'SLICED_PIN')
    hostc = lines(host_log, 'SLICED_PIN_HOST')
    outs = ('Z_i', 'Z_j', 'Z_log')
    worst, by_group, by_family, over = {}, {}, {}, {}

    def up(d, key, z, v):
        e = d.setdefault(key, {})
        e[z] = max(e.get(z, 0.0), v)
    for c in cases:
        for z in outs:
            if z in c:
                worst[z] = max(worst.get(z, 0.0), c[z]['ratio'])
                over[z] = max(over.get(z, 0.0), c[z]['over_bound'])
                up(by_group, c['group'], z, c[z]['ratio'])
                # Z_i is the row kernel's sum, Z_j and Z_log the column kernel's (over the row kernel's s)
                fam = ('row: ' + c['row_family']) if z == 'Z_i' else ('column: ' + c['col_family'])
                up(by_family, fam, z, c[z]['ratio'])
    doc = dict(
        what='err_colrel distance from the float64 loop nest (sliced_pass_reference.exact_nz == cavi_oracle.zq_exact) of engine.zq '
             'through the sliced row and column passes (csrc/passes_*.h) on an MI355X (hip) and of the reference float32 loop nest '
             '(ref) on the cases of tests/sliced_pass_reference.py; ratio = hip / ref, over_bound = hip / zlog_bound(ref); and, on the '
             'CPU, of sliced_pass_reference.f32_slot_eval complete, with the last record of one slice lost and with one padding slot '
             'taken for an entry (the least multiple of the bound over all slices)',
        command='python -m pytest tests/test_sliced_pass_gpu.py -q -s (the SLICED_PIN lines); python -m pytest '
                'tests/test_sliced_pass_host.py -q -s (the SLICED_PIN_HOST lines); python tools/sliced_pass_report.py gpu.log host.log',
        inputs=dict(small={s: list(sr.problem('small', s).shape) for s in ('rows', 'cols')},
                    band={s: list(sr.problem('band', s).shape) for s in ('rows', 'cols')},
                    widths=list(sr.WIDTHS), kpads=list(sr.KPADS), family_widths=list(sr.FAMILY_WIDTHS),
                    weight_widths=list(sr.WEIGHT_WIDTHS), band_widths=list(sr.BAND_WIDTHS), extra_tile_lengths=sr.EXTRA_LENGTHS),
        bound=dict(ZLOG_FACTOR=ZLOG_FACTOR, ZLOG_FLOOR=ZLOG_FLOOR),
        n_cases=len(cases), worst_hip_ratio=worst, worst_hip_ratio_by_family=by_family, worst_hip_ratio_by_group=by_group,
        worst_hip_over_bound=over, cpu_slot_eval=hostc)
    head = json.dumps(doc, indent=1)
    assert head.endswith('\n}')
    sys.stdout.write(head[:-2] + ',\n "cases": [\n' + ',\n'.join('  ' + json.dumps(c) for c in cases) + '\n ]\n}\n')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
