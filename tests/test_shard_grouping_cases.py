"""CPU: tests/shard_grouping_cases.py plants what it says, its shard_of is the sharded trainer's renumbering, and the cases straddle the
SpMM's automatic slice policy (asked through gss_spmm_auto_slices, a host-only entry point -- no constant is copied here)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import shard_grouping_cases as SG

DS = sorted(SG.SIZES)


@pytest.fixture(scope="module")
def lib():
    import gcn_drug_repurposing_amd as pkg
    return pkg.load()


def auto_slices(lib, d, cols):
    ns, pin = C.c_int32(-1), C.c_int32(-1)
    assert lib.gss_spmm_auto_slices(d, int(cols), C.byref(ns), C.byref(pin)) == 0, lib.gss_last_error()
    return ns.value, pin.value


@pytest.mark.parametrize("d", DS)
def test_the_builder_plants_what_it_says(d):
    c = SG.case(d)
    n, parts = SG.SIZES[d]
    assert c.a.shape == (n, n) and c.x.shape == (n, d) and c.x.dtype == np.float32 and c.a.data.dtype == np.float32
    assert c.a.has_sorted_indices and len(c.ranges) == parts and c.ranges[0][0] == 0 and c.ranges[-1][1] == n
    assert float(c.a.data.min()) >= 0.1 and float(c.a.data.max()) <= 1.0
    lens = np.diff(c.a.indptr)
    special = set()
    for k, (lo, hi) in enumerate(c.ranges):
        size = hi - lo
        assert size % 128 == 0
        assert [ln for _, ln in c.planted[k]] == [33, 64, 65, 128, 129, 257, 512, 513, 1025, min(2000, size)]
        for r, ln in c.planted[k]:
            assert lo <= r < hi and lens[r] == ln
            cols = c.a.indices[c.a.indptr[r]:c.a.indptr[r + 1]]
            assert len(np.unique(cols)) == ln and cols.min() >= lo and cols.max() < hi      # its own range: no halo from a planted row
            special.add(r)
        e = c.empty[k]
        assert lo <= e < hi and lens[e] == 0
        special.add(e)
    assert len(special) == parts * (len(SG.PLANTED) + 1)
    band = np.array([r not in special for r in range(n)])
    rows = np.repeat(np.arange(n), lens)
    off = np.abs(c.a.indices.astype(np.int64) - rows)
    assert off[band[rows]].max() <= SG.BAND
    assert 4 <= lens[band].min() and lens[band].max() <= 12 and 7.5 < lens[band].mean() < 8.5
    # lengths either side of every boundary the schedule has: p = 2 / 4 / 8 groups of 32 entries, the GPW-1 cap of 512, far beyond it
    have = {ln for _, ln in c.planted[0]}
    for edge in (64, 128, 512):
        assert edge in have and edge + 1 in have
    assert 256 + 1 in have and max(have) > 2 * 512


@pytest.mark.parametrize("d", DS)
def test_shard_of_is_the_rows_of_the_matrix_entry_for_entry(d):
    c = SG.case(d)
    a64 = sp.csr_matrix(c.a, dtype=np.float64)
    whole = a64 @ c.x.astype(np.float64)
    for lo, hi in c.ranges:
        sh = SG.shard_of(c.a, lo, hi, c.x)
        sub = c.a[lo:hi]
        assert sh.a.shape == (hi - lo, sh.n_cols) and sh.n_cols == (hi - lo) + len(sh.halo)
        assert np.array_equal(sh.a.indptr, sub.indptr)
        assert np.array_equal(SG.map_back(sh), sub.indices)                   # the same entries in the same (ascending global) order
        assert np.array_equal(sh.a.data, sub.data) and sh.a.data.dtype == np.float32
        assert np.all(np.diff(sh.halo) > 0) and not np.any((sh.halo >= lo) & (sh.halo < hi))
        assert 0 < len(sh.halo) <= 2 * SG.BAND                                # the band's reach on either side, nothing from planted rows
        assert np.array_equal(sh.x[:hi - lo], c.x[lo:hi]) and np.array_equal(sh.x[hi - lo:], c.x[sh.halo])
        # own columns first, then the halo in ascending global order
        own = sh.a.indices < hi - lo
        assert np.array_equal(sh.a.indices[own] + lo, sub.indices[own])
        local = sp.csr_matrix(sh.a, dtype=np.float64) @ sh.x.astype(np.float64)
        # fp64 sums of the same products in the same order: equal, not close
        assert np.array_equal(local, whole[lo:hi])


def test_shard_of_agrees_with_the_trainers_halo():
    """dist.Halo is what dist.sharded_plan_engine renumbers with"""
    from gcn_drug_repurposing_amd.dist import Halo, Partition
    c = SG.case(256)
    part = Partition(np.array([0] + [hi for _, hi in c.ranges], dtype=np.int64))
    for rank, (lo, hi) in enumerate(c.ranges):
        sh = SG.shard_of(c.a, lo, hi)
        sub = sp.csr_matrix(c.a[lo:hi])
        halo = Halo(sub.indices, part, rank)
        assert np.array_equal(halo.remote, sh.halo) and halo.n_halo == len(sh.halo)
        assert np.array_equal(halo.local_cols(sub.indices), sh.a.indices)


@pytest.mark.parametrize("d", DS)
def test_the_cases_straddle_the_slice_policy(lib, d):
    """sliced for the job's N, unsliced for every shard's own operand; and N is the smallest multiple of 128 rows per range that is"""
    c = SG.case(d)
    ns, _ = auto_slices(lib, d, c.n)
    assert ns > 1
    parts = len(c.ranges)
    assert auto_slices(lib, d, c.n - 128 * parts)[0] == 1
    for lo, hi in c.ranges:
        sh = SG.shard_of(c.a, lo, hi)
        assert auto_slices(lib, d, sh.n_cols) == (1, 0)
    # the two sides' lane groups per wave differ: width of a slice in float4 -> lanes per row -> groups per wave
    def gpw(d4):
        lanes = 4
        while lanes < min(d4, 64):
            lanes *= 2
        return 64 // lanes
    assert gpw(d // 4) != gpw(d // 4 // ns)


def test_single_gpu_launches_keep_their_policy(lib):
    """the benchmark's shape: two slices, pinned to XCDs; and the policy's other landmarks (a statement of what the kernel comments
    measured, through the query)"""
    assert auto_slices(lib, 128, 29960) == (2, 1)
    assert auto_slices(lib, 256, 29960) == (4, 1)
    assert auto_slices(lib, 128, 2000) == (1, 0)
    assert auto_slices(lib, 64, 10 ** 6) == (1, 0)          # narrower than two 256-B slices: never sliced
    assert auto_slices(lib, 128, 10 ** 6) == (2, 0)         # beyond the Infinity Cache: time-separated
    assert lib.gss_spmm_auto_slices(100, 1000, None, None) != 0


@pytest.mark.parametrize("d,world", [(256, 3), (1024, 2)])
def test_the_plan_level_graphs_straddle_on_every_rank(lib, d, world):
    """the sharded trainer cuts node ranges by work, not evenly: each rank's operand (own rows + halo, of A_hat and of A_hat^T) must
    still sit below the threshold that N is above"""
    from gcn_drug_repurposing_amd.dist import Halo, partition_for
    c = SG.case(d)
    adj = SG.adjacency(c)
    assert (adj != adj.T).nnz == 0 and adj.diagonal().sum() == 0
    a = sp.csr_matrix(adj + sp.eye(c.n, format="csr"))
    a.sort_indices()
    part = partition_for(a, world)
    assert auto_slices(lib, d, c.n)[0] > 1
    for rank in range(world):
        lo, hi = part.rows(rank)
        for m in (a, sp.csr_matrix(a.T)):
            halo = Halo(sp.csr_matrix(m[lo:hi]).indices, part, rank)
            assert auto_slices(lib, d, (hi - lo) + halo.n_halo) == (1, 0), (rank, lo, hi, halo.n_halo)
        lens = np.diff(a.indptr)[lo:hi]
        assert (lens > 2 * SG.REGROUP_ABOVE[d]).sum() >= 3      # every rank owns rows whose grouping is at stake
