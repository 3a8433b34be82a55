"""Writes tests/golden/sweep3_streamer_parent.npz, the fixture of tests/test_gpu_sweep3_streamer_chain.py: Chain.state() and Chain.result() of that
file's cases (its case list, inputs and runner are used as they stand), computed on the GPU by WHATEVER LIBRARY IS LOADED.  The fixture is meant to
hold the bits of the commit a change to the streamers is compared with: build that commit's library, point BWGR_LIB at it and run this script --
never against the code under test.  Usage: BWGR_LIB=/path/to/parent/libbwgr_hip.so python tools/make_sweep3_streamer_golden.py [out.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # (conftest: the suite's switches and synth_small)
import numpy as np

import test_gpu_sweep3_streamer_chain as T


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    from bwgr_amd import build as B
    print("library: %s" % B.LIB)

    def delenv(k):
        os.environ.pop(k, None)

    arrays = {}
    for case in T.CASES:
        which, got = T.run_case(case, os.environ.__setitem__, delenv)
        assert which == T.FIXED, (case, which)
        d = got["state_d"]
        print("%-32s ve %.9g  included %5d  most in a block %3d" % (T.case_id(case), float(got["state_ve"]), int(d.sum()),
                                                                   max(int(d[j:j + 128].sum()) for j in range(0, case[1], 128))), flush=True)
        for k, v in got.items():
            arrays[T.case_id(case) + "/" + k] = v
    which, got = T.run_case(T.GENERIC_CASE, os.environ.__setitem__, delenv, fixed=False)   # (the two kernels are one source: the same bits, or no fixture)
    assert which == T.GENERIC
    for k, v in got.items():
        assert np.array_equal(v, arrays[T.case_id(T.GENERIC_CASE) + "/" + k]), k
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))


if __name__ == "__main__":
    main()
