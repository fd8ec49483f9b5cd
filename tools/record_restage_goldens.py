"""Records tests/golden/restage_k100/<case>.npz for tests/test_restage_k100_gpu.py: Z_i (default mode) and Z_j of the
deterministic mode (the sliced genes' rows) of every case there, from the library that is loaded -- run it on an MI355X with the library of the commit
whose bits are to be kept (ORIANA_HIP_LIB=/path/to/liboriana_hip.so python tools/record_restage_goldens.py [OUTDIR]).
Every case runs twice per mode; the script refuses to record an output that is not the same both times (and a Z_i that differs
between the two modes: the row side does not depend on the mode)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import test_restage_k100_gpu as t
    from oriana_amd import engine, _lib
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    print('library:', _lib.LIB_PATH)
    for name in sorted(t.CASES):
        dense = t.CASES[name][3]           # (the dense genes' rows of Z_j come from the dense-gene kernels: not recorded)
        plain = [t.run(engine, name, False)[0] for _ in range(2)]
        det = [t.run(engine, name, True)[0] for _ in range(2)]
        assert plain[0][0].tobytes() == plain[1][0].tobytes(), name + ': Z_i is not repeatable'
        assert det[0][0].tobytes() == plain[0][0].tobytes(), name + ': Z_i depends on the mode'
        assert det[0][1][dense:].tobytes() == det[1][1][dense:].tobytes(), name + ': Z_j of the deterministic mode is not repeatable'
        ref = t.oracle(name)
        print('%-28s Z_i %.3e  Z_j (det) %.3e from the oracle' % (name, t.err_colrel(plain[0][0], ref[0]), t.err_colrel(det[0][1], ref[1])))
        np.savez_compressed(os.path.join(out, name + '.npz'), Z_i=plain[0][0], Z_j_det=det[0][1][dense:])
    print('recorded %d cases in %s' % (len(t.CASES), out))


if __name__ == '__main__':
    main()
