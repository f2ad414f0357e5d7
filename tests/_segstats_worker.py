"""Child process of tests/test_gpu_segstats_edges.py: `SD_SEGSTATS_NO_LDS` and `SD_SEGSTATS_NO_PREFETCH` are read once per process, so
each is tried in a fresh one.  Runs a subset of the form matrix, the misaligned and the saturated cases and compares every table with
the numpy oracle; any difference ends the process with a traceback and a non-zero status.
usage: _segstats_worker.py SWITCH [SWITCH ...]      (the switches the parent has set; checked, then named in the last line)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _segstats_cases as SC                                       # noqa: E402
from syconn_amd.extraction.find_object_properties import segstats           # noqa: E402


def main():
    switches = sys.argv[1:]
    for s in switches:
        assert os.environ.get(s), f'{s} is not set in this process'
    assert 'SD_SEGSTATS_V1' not in os.environ
    dev = torch.device('cuda', 0)
    n = 0

    def both(cell, subs, what, want_props=True):
        nonlocal n
        want = SC.oracle(cell, subs) if cell is not None else (None, SC.props_cellless_np(subs), [])
        r4 = segstats(cell, subs, want_props=want_props, device=dev)
        SC.assert_equals_oracle(r4, want, want_props, what)
        os.environ['SD_SEGSTATS_V1'] = '1'                                   # read at every call, unlike the two switches
        try:
            r1 = segstats(cell, subs, want_props=want_props, device=dev)
        finally:
            del os.environ['SD_SEGSTATS_V1']
        SC.assert_equals_oracle(r1, want, want_props, what + ' (one-voxel form)')
        n += 1

    for dtype in (np.uint32, np.uint64):
        for has_cell, n_sub in ((True, 0), (True, 1), (True, 3), (True, 4), (True, 8), (False, 1), (False, 2), (False, 4), (False, 6)):
            for shape in ((9, 10, 72), (9, 10, 71), (3, 5, 12)):
                cell, subs = SC.form_case(shape, has_cell, n_sub, dtype)
                both(cell, subs, f'{shape} {has_cell} {n_sub} {dtype.__name__}')
                if has_cell and n_sub:
                    both(cell, subs, f'{shape} {has_cell} {n_sub} {dtype.__name__} counts only', want_props=False)
        cell, subs = SC.form_case((9, 10, 72), True, 2, dtype, seed=7)
        for mis in ((True, True, True), (True, False, False), (False, False, True)):
            d = [SC.device_volume(v, dev, m) for v, m in zip([cell] + subs, mis)]
            SC.assert_equals_oracle(segstats(d[0], d[1:], device=dev), SC.oracle(cell, subs), True, f'misaligned {mis}')
            n += 1
    for name in ('lcap512_lone', 'lcap256_pcap1024', 'lcap128_pcap256', 'lcap64_pcap128', 'lcap64_cellless'):
        both(*SC.saturated_case(**SC.SATURATED[name]), name)
    for name in sorted(SC.PAIR_SATURATED):
        both(*SC.saturated_case(**SC.PAIR_SATURATED[name]), name)
    both(*SC.mixed_case((9, 16, 256)), 'mixed')
    print(f'segstats worker ok: {n} cases equal the oracle with {" ".join(switches) or "no switch"}')


if __name__ == '__main__':
    main()
