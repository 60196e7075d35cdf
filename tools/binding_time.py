"""Host cost of one C-ABI call through ctypes, two ways: every argument wrapped by the caller and no argtypes on the function (how the
package called the library before the binding read include/nc_hip.h), and plain Python numbers converted by the declared argtypes.
nc_conv_fwd_path is host arithmetic: no GPU needed.  Alternates the two, prints seconds per `--calls` calls of every repeat.

    python tools/binding_time.py [--calls 100000] [--repeats 5]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuroclear_amd import _lib  # noqa: E402
from neuroclear_amd._lib import I  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100000)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    new = _lib.lib().nc_conv_fwd_path
    old = ctypes.CDLL(_lib.LIB_PATH).nc_conv_fwd_path  # a handle of its own: its functions carry no prototypes
    old.restype = ctypes.c_int
    assert old.argtypes is None and len(new.argtypes) == 7
    n = range(args.calls)
    res = {'wrapped': [], 'plain': []}
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _i in n:
            old(I(64), I(64), I(3), I(3), I(3), I(1), I(1))
        t1 = time.perf_counter()
        for _i in n:
            new(64, 64, 3, 3, 3, 1, 1)
        t2 = time.perf_counter()
        res['wrapped'].append(t1 - t0)
        res['plain'].append(t2 - t1)
        print('wrapped, no argtypes %.4f s    plain, argtypes %.4f s    (%d calls each)' % (t1 - t0, t2 - t1, args.calls))
    for k, v in res.items():
        print('%-8s %.4f .. %.4f s, median %.4f s = %.2f us per call' % (k, min(v), max(v), sorted(v)[len(v) // 2],
                                                                         sorted(v)[len(v) // 2] / args.calls * 1e6))


if __name__ == '__main__':
    main()
