"""CPU: the numpy restatement of the dataset merge of contact sites (tests/_cs_driver_ref.py) reproduces golden g18 -- the
reference's own ``_write_props_to_syn_thread`` / ``_write_props_collect_helper`` on worker files -- exactly; ``storage_keys`` equals
the buckets the reference's ``subfold_from_ix_new`` names, ids above 2^53 included; the job-major chunk order of the driver."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_driver_ref as D  # noqa: E402

G18 = os.path.join(HERE, 'golden', 'g18_cs_driver.npz')


@pytest.fixture(scope='module')
def g18():
    return dict(np.load(G18))


def merged(g, jobs):
    return D.merge_workers([D.fold_chunks(j) for j in jobs], int(g['min_obj_vx'][0]), int(g['min_obj_vx'][1]))


def test_restatement_reproduces_golden(g18):
    cs, syn = merged(g18, D.golden_jobs(g18))
    w_cs, w_syn = D.golden_dicts(g18)
    D.assert_same(cs, w_cs, 'cs')
    D.assert_same(syn, w_syn, 'syn')
    assert all(v['bounding_box'].dtype == np.int32 for v in w_cs.values())
    assert np.array_equal(g18['syn_cs_id'], g18['syn_ids'])


def test_golden_inputs_are_meaningful(g18):
    """Three or more workers of several chunks, ids shared between chunks and workers, ids at the edges of the formats, one object
    removed by each of the three filter conditions, all type mixtures."""
    rec, cb, w = g18['in_rec'], g18['in_chunk_begin'], g18['in_chunk_worker']
    ids = rec[:, 0].view(np.uint64)
    assert len(set(w.tolist())) >= 3 and min(np.bincount(w)) >= 3
    chunk_of = np.repeat(np.arange(len(w)), np.diff(cb))
    for k in range(len(w)):                                        # an id occurs at most once per chunk
        assert len(np.unique(ids[chunk_of == k])) == (chunk_of == k).sum()
    multi_worker = [i for i in np.unique(ids) if len(set(w[chunk_of[ids == i]].tolist())) > 1]
    multi_chunk = [i for i in np.unique(ids) if len(set(chunk_of[ids == i][w[chunk_of[ids == i]] == 0].tolist())) > 1]
    assert len(multi_worker) > 10 and len(multi_chunk) > 5
    present = set(ids.tolist())
    for i in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 53 + 1, 2 ** 63, 2 ** 64 - 2):
        assert i in present and i in set(g18['cs_ids'].tolist())
    mn_cs, mn_syn = (int(v) for v in g18['min_obj_vx'])
    tot_cs = {i: int(rec[ids == i, 4].sum()) for i in np.unique(ids).tolist()}
    tot_syn = {i: int(rec[ids == i, 14].sum()) for i in np.unique(ids).tolist()}
    kept_cs, kept_syn = set(g18['cs_ids'].tolist()), set(g18['syn_ids'].tolist())
    assert any(tot_cs[i] < mn_cs and tot_syn[i] >= mn_syn and i not in kept_cs and i not in kept_syn for i in tot_cs)   # cs too small, syn alone would pass
    assert any(tot_cs[i] >= mn_cs and 0 < tot_syn[i] < mn_syn and i in kept_cs and i not in kept_syn for i in tot_cs)   # syn too small
    assert any(tot_cs[i] < mn_cs for i in tot_cs) and kept_cs == {i for i in tot_cs if tot_cs[i] >= mn_cs}
    assert kept_syn == {i for i in kept_cs if tot_syn[i] >= mn_syn}
    some = [i for i in kept_syn if (rec[ids == i, 14] == 0).any()]                                                      # syn voxels in some chunks only
    assert some
    a, s = g18['syn_asym_prop'], g18['syn_sym_prop']
    assert ((a > 0) & (s == 0)).any() and ((a == 0) & (s > 0)).any() and ((a == 0) & (s == 0)).any() and ((a > 0) & (s > 0)).any()


def test_chunk_order_changes_the_result(g18):
    """The representative coordinate is the last chunk's in job-major order: the same chunks dealt to 1 and to 3 jobs give different
    coordinates for at least one id, equal sizes and equal sets of boxes and voxels for all."""
    chunks = [c for j in D.golden_jobs(g18) for c in j]
    res = {}
    for n in (1, 3, 10 ** 6):
        res[n] = merged(g18, [[chunks[i] for i in job] for job in D.jobs_of(list(range(len(chunks))), n)])
    for t in (0, 1):
        a, b = res[1][t], res[3][t]
        assert list(a) == list(b)
        assert any(not np.array_equal(a[k]['rep_coord'], b[k]['rep_coord']) for k in a)
        for k in a:
            assert a[k]['size'] == b[k]['size'] and np.array_equal(a[k]['bounding_box'], b[k]['bounding_box'])
            assert sorted(a[k]['boxes'].tolist()) == sorted(b[k]['boxes'].tolist())
        D.assert_same(res[10 ** 6][t], a, 'one chunk per job == one job')        # both are the order of the chunk list


@pytest.mark.parametrize('n_jobs', [1, 3, None])
def test_job_major_order(n_jobs):
    from syconn_amd import global_params
    from syconn_amd.extraction.cs_extraction_steps import job_major_order
    from syconn_amd.handler.basics import chunkify
    chunk_list = list(range(100, 111))
    n = global_params.config.ncore_total * 8 if n_jobs is None else n_jobs
    got = job_major_order(chunk_list, n)
    assert got == D.job_major(chunk_list, n) == [c for job in chunkify(chunk_list, n) for c in job]
    assert sorted(got) == chunk_list
    if n_jobs == 3:
        assert got == [100, 103, 106, 109, 101, 104, 107, 110, 102, 105, 108]
    else:
        assert got == chunk_list                                   # one job, or one chunk per job: the chunk list's order
    assert global_params.config.ncore_total == global_params.config['nnodes_total'] * global_params.config['ncores_per_node']


def test_storage_keys_equal_golden_buckets(g18):
    from syconn_amd.extraction.cs_extraction_steps import storage_keys
    ids = g18['key_ids']
    assert (ids > 2 ** 53).sum() > 10
    assert storage_keys(ids, 1000) == g18['key_bucket_1000'].tolist()
    assert storage_keys(ids, 100000) == g18['key_bucket_100000'].tolist()
    # float64 arithmetic is part of the contract: for large ids the integer quotient names another bucket
    exact = ['/%02d/%d/' % divmod(int(i) // 1000 % 1000, 10) for i in ids.tolist()]
    assert exact != g18['key_bucket_1000'].tolist()
    assert storage_keys(np.array([5000, 123456], np.uint64), 1000) == ['/00/5/', '/12/3/']
