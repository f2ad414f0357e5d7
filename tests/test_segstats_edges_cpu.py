"""CPU side of the label-statistics edge tests: the inputs of tests/test_gpu_segstats_edges.py really sit on the edges they claim
(checked with the launch model of tests/_segstats_cases.py, whose constants come from the kernel sources), and the vectorised oracle
equals the literal loops on cut-down versions of every case."""
import numpy as np
import pytest

from oracle.objprops_ref import find_object_properties_loops, map_subcell_extract_props_loops
from tests import _segstats_cases as SC

CONSTS = SC.kernel_constants()


def test_constants_of_the_scan_are_the_ones_the_cases_were_written_for():
    """A retuned kernel must make somebody look at the cases again: the values the edge cases were derived from."""
    assert CONSTS == {'LDS_SLOTS': 512, 'LDS_PSLOTS': 1024, 'MAX_SUB': 8, 'LDS_PROBES': 24, 'PAIR_PROBES': 16, 'WAVES_PER_WG_V4': 16,
                      'WAVES_PER_WG_V1': 64, 'GRID_CAP': 2048, 'VPW_V4': 256, 'VPW_V1': 64, 'LCAP_MIN': 32, 'GRID_FOR_ITEMS': 1 << 20}


def test_a_missing_constant_fails_loudly():
    with pytest.raises(AssertionError, match='not found in the kernel sources'):
        SC._grab('constexpr int SOMETHING_ELSE = 3;', r'constexpr int LDS_SLOTS = (\d+);', 'LDS_SLOTS')


def test_lds_shares_per_number_of_volumes():
    lcaps = [SC.launch_model((8, 8, 64), True, n, consts=CONSTS).lcap for n in range(0, 9)]
    assert lcaps == [512, 256, 128, 128, 64, 64, 64, 64, 32]
    pcaps = [SC.launch_model((8, 8, 64), True, n, consts=CONSTS).pcap for n in range(0, 9)]
    assert pcaps == [0, 1024, 512, 256, 256, 128, 128, 128, 128]
    assert SC.launch_model((8, 8, 64), False, 8, consts=CONSTS).lcap == 64 and SC.launch_model((8, 8, 64), False, 8, consts=CONSTS).pcap == 0
    assert SC.launch_model((8, 8, 64), True, 3, want_props=False, consts=CONSTS).pcap == 0


@pytest.mark.parametrize('name', sorted(SC.SATURATED))
def test_saturated_cases_exceed_the_lds_shares(name):
    kw = SC.SATURATED[name]
    cell, subs = SC.saturated_case(**kw)
    lm = SC.launch_model(kw['shape'], kw['has_cell'], kw['n_sub'], consts=CONSTS)
    assert lm.v4 and (lm.lcap, lm.pcap) == SC.EXPECTED_SHARES[name]
    ids, pairs = SC.range_distinct(lm, cell, subs)
    print(f'{name}: {ids} ids against lcap {lm.lcap}, {pairs} pairs against pcap {lm.pcap}, grid {lm.grid}, per_wg {lm.per_wg}')
    assert ids > lm.lcap
    if lm.pcap:
        assert pairs > lm.pcap
    assert lm.grid > 1                                        # several workgroups flush into the same global slots


@pytest.mark.parametrize('name', sorted(SC.PAIR_SATURATED))
def test_pair_saturated_cases_fit_the_object_tables_and_exceed_the_pair_table(name):
    kw = SC.PAIR_SATURATED[name]
    cell, subs = SC.saturated_case(**kw)
    lm = SC.launch_model(kw['shape'], True, kw['n_sub'], consts=CONSTS)
    assert lm.v4 and (lm.lcap, lm.pcap) == SC.EXPECTED_SHARES[name] and lm.grid > 1
    ids, pairs = SC.range_distinct(lm, cell, subs)
    print(f'{name}: {ids} ids against lcap {lm.lcap}, {pairs} pairs against pcap {lm.pcap}')
    assert ids <= lm.lcap // 2 and pairs > lm.pcap           # half-empty object tables: the 24-probe limit is not what sends pairs to HBM


def test_all_five_lds_shares_are_saturated_by_some_case():
    assert {SC.EXPECTED_SHARES[n][0] for n in SC.SATURATED} == {512, 256, 128, 64, 32}
    assert {SC.EXPECTED_SHARES[n][1] for n in SC.PAIR_SATURATED} == {1024, 256, 128}


def test_mixed_case_has_far_ids_in_every_range_and_more_local_ids_than_slots():
    shape = (9, 16, 256)
    cell, subs = SC.mixed_case(shape)
    lm = SC.launch_model(shape, True, 1, consts=CONSTS)
    ids, pairs = SC.range_distinct(lm, cell, subs)
    assert ids > lm.lcap and lm.grid > 4
    span = lm.per_wg * lm.vpw
    flat = cell.reshape(-1)
    for far in range(10, 15):
        assert all(np.any(flat[lo:lo + span] == far) for lo in range(0, lm.nvox, span))
    assert len(np.unique(flat)) > 4000


FORM_SHAPES = {True: (9, 10, 72), False: (9, 10, 71)}          # rows % 4 == 0 -> four-voxel forms, else the one-voxel form


@pytest.mark.parametrize('has_cell,n_sub', [(True, n) for n in range(0, 9)] + [(False, n) for n in range(1, 9)])
def test_coherent_form_cases_stay_inside_the_lds_shares(has_cell, n_sub):
    for v4 in (True, False):
        shape = FORM_SHAPES[v4]
        cell, subs = SC.form_case(shape, has_cell, n_sub, np.uint64)
        lm = SC.launch_model(shape, has_cell, n_sub, consts=CONSTS)
        assert lm.v4 == v4 and lm.grid >= 2
        ids, pairs = SC.range_distinct(lm, cell, subs)
        assert ids <= lm.lcap and (not lm.pcap or pairs <= lm.pcap)


def test_form_case_ends_inside_a_wave_and_tiny_volume_is_below_one_wave():
    lm = SC.launch_model(FORM_SHAPES[True], True, 1, consts=CONSTS)
    assert lm.v4 and lm.nvox % lm.vpw != 0 and (lm.nvox % lm.vpw) % 4 == 0       # the last wave of the volume is partly invalid
    tiny = SC.launch_model((3, 5, 12), True, 1, consts=CONSTS)
    assert tiny.v4 and tiny.nvox < 256 and tiny.nwaves == 1 and tiny.grid == 1


def test_grid_cap_case_gives_unequal_trips_and_a_short_last_range():
    for v4, nwaves, per_wg in ((True, 41321, 21), (False, 165282, 81)):
        lm = SC.launch_model(SC.GRID_CAP_SHAPE, True, 3, v4=v4, consts=CONSTS)
        assert lm.grid == CONSTS['GRID_CAP'] == 2048 and lm.nwaves == nwaves and lm.per_wg == per_wg
        assert lm.per_wg % 4 != 0                    # the four waves of a workgroup make unequal numbers of trips
        assert lm.nwaves % lm.per_wg != 0            # the last workgroup with work has a short range ...
        assert lm.per_wg * (lm.grid - 1) >= lm.nwaves or lm.nwaves - lm.per_wg * (lm.grid - 1) < lm.per_wg
    assert SC.launch_model(SC.GRID_CAP_SHAPE, True, 3, v4=True, consts=CONSTS).per_wg * 2047 > 41321   # ... and the very last ones none
    assert SC.GRID_CAP_SHAPE[2] % 4 == 0


def test_sizes_past_the_grid_stride_of_the_table_kernels():
    assert (1 << 21) > CONSTS['GRID_FOR_ITEMS'] and 128 ** 3 > CONSTS['GRID_FOR_ITEMS'] and 3_000_000 > 2 * CONSTS['GRID_FOR_ITEMS']


# ---- vectorised oracle == literal loops on cut-down versions of every case ---------------------------------------------------------------
def _loops(cell, subs):
    """The literal restatement as arrays: (cell props or None, [sub props], [pairs])."""
    def arrays(rc, bb, sz, shape):
        ids = np.array(sorted(sz), dtype=np.uint64)
        first = np.array([np.ravel_multi_index(tuple(rc[int(i)]), shape) for i in ids], dtype=np.int64)
        return (ids, first, np.array([sz[int(i)] for i in ids], dtype=np.int64),
                np.array([bb[int(i)] for i in ids], dtype=np.int64).reshape(-1, 2, 3))
    shape = (cell if cell is not None else subs[0]).shape
    if cell is None:
        return None, [arrays(*find_object_properties_loops(s), shape) for s in subs], []
    if not subs:
        return arrays(*find_object_properties_loops(cell), shape), [], []
    c, s, m = map_subcell_extract_props_loops(cell, np.stack(subs))
    pairs = []
    for d in m:
        rows = sorted((a, b, n) for a, inner in d.items() for b, n in inner.items())
        pairs.append(tuple(np.array([r[i] for r in rows], dtype=(np.uint64, np.uint64, np.int64)[i]) for i in range(3)))
    return arrays(*c, shape), [arrays(s[0][k], s[1][k], s[2][k], shape) for k in range(len(subs))], pairs


class _Res:
    def __init__(self, cell, sub, pairs):
        self.cell, self.sub, self.pairs = cell, sub, pairs


def _check(cell, subs):
    SC.assert_equals_oracle(_Res(*_loops(cell, subs)), SC.oracle(cell, subs), what='loops')


SMALL = (3, 5, 24)


@pytest.mark.parametrize('dtype', [np.uint32, np.uint64])
def test_vectorised_oracle_equals_literal_loops_on_cut_down_cases(dtype):
    for has_cell, n_sub in ((True, 0), (True, 2), (True, 8), (False, 1), (False, 5)):
        _check(*SC.form_case(SMALL, has_cell, n_sub, dtype))
        _check(*SC.form_case((3, 5, 23), has_cell, n_sub, dtype))
    for name, kw in list(SC.SATURATED.items()) + list(SC.PAIR_SATURATED.items()):
        _check(*SC.saturated_case(**dict(kw, shape=SMALL, nid=50, dtype=dtype)))
    _check(*SC.mixed_case(SMALL, dtype))
    _check(*SC.grid_cap_case((5, 9, 12), dtype))
    # every voxel its own object, the second volume counted backwards
    n = int(np.prod(SMALL))
    cell = (np.arange(n, dtype=dtype) + 1).reshape(SMALL)
    _check(cell, [(n - np.arange(n, dtype=dtype)).reshape(SMALL)])


def test_special_ids_are_present_in_the_form_cases():
    cell, subs = SC.form_case(FORM_SHAPES[True], True, 2, np.uint64)
    assert {2 ** 64 - 1, 2 ** 63 + 7, 2 ** 63} <= set(int(v) for v in np.unique(cell))
    cell, subs = SC.form_case(FORM_SHAPES[True], True, 2, np.uint32)
    assert 2 ** 32 - 1 in set(int(v) for v in np.unique(cell)) and 2 ** 32 - 1 in set(int(v) for v in np.unique(subs[1]))
