# -*- coding: utf-8 -*-
"""Assemble profiles/dense_pass_errors.json from the printed figures of the dense-pass pins:

    python -m pytest tests/test_dense_pass_gpu.py -q -s > gpu.log        (on an MI355X: the DENSE_PIN lines)
    python -m pytest tests/test_dense_pass_host.py -q -s > host.log      (CPU: the DENSE_PIN_HOST lines)
    python tools/dense_pass_report.py gpu.log host.log > profiles/dense_pass_errors.json
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
    import dense_pass_reference as dr
    from helpers import ZLOG_FACTOR, ZLOG_FLOOR
    cases = lines(gpu_log, 'DENSE_PIN')
    hostc = lines(host_log, 'DENSE_PIN_HOST')
    outs = ('Z_i', 'Z_j', 'Z_log')
    worst, worst_by_group = {}, {}
    for c in cases:
        for z in outs:
            if z in c:
                worst[z] = max(worst.get(z, 0.0), c[z]['ratio'])
                g = worst_by_group.setdefault(c['group'], {})
                g[z] = max(g.get(z, 0.0), c[z]['ratio'])
    mut = {}
    for h in hostc:
        for name in list(dr.MUTANTS) + ['six products']:
            for z in ('Z_i', 'Z_j'):
                e = mut.setdefault(name, {}).setdefault(z, dict(min_over_bound=float('inf'), max_over_bound=0.0))
                e['min_over_bound'] = min(e['min_over_bound'], h[z][name]['over_bound'])
                e['max_over_bound'] = max(e['max_over_bound'], h[z][name]['over_bound'])
    doc = dict(
        what='err_colrel distance from cavi_oracle.zq_exact (float64) of engine.zq / engine.zq_gap through the dense-gene kernels '
             '(csrc/dense_pass.hip) on an MI355X (hip) and of the reference float32 loop nest (ref) on the cases of '
             'tests/dense_pass_reference.py; ratio = hip / ref, over_bound = hip / zlog_bound(ref); and, on the CPU, of '
             'dense_pass_reference.six_product_eval complete and with cross products dropped',
        command='python -m pytest tests/test_dense_pass_gpu.py -q -s (the DENSE_PIN lines); python -m pytest '
                'tests/test_dense_pass_host.py -q -s (the DENSE_PIN_HOST lines); python tools/dense_pass_report.py gpu.log host.log',
        inputs=dict(n=dr.PIN_N, m=dr.PIN_M, density=dr.PIN_DENSITY, widths=list(dr.WIDTHS), kpads=list(dr.KPADS),
                    seeds={str(K): dr.SEEDS.get(K, 4000 + K) for K in dr.WIDTHS}),
        bound=dict(ZLOG_FACTOR=ZLOG_FACTOR, ZLOG_FLOOR=ZLOG_FLOOR),
        worst_hip_ratio=worst, worst_hip_ratio_by_group=worst_by_group,
        worst_hip_over_bound=max(c[z]['over_bound'] for c in cases for z in outs if z in c),
        cpu_six_product_eval_over_bound=mut, cases=cases, cpu_cases=hostc)
    json.dump(doc, sys.stdout, indent=1)
    sys.stdout.write('\n')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
