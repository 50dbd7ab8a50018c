"""CPU: diffusion._profile_source, the one resolver of the three kinds of `profiles` (device tensor, host array [K][N], {name: vector}
dict) behind rank_profiles, top_nodes, compare_profiles and compare_profile_pairs: what it returns for one and two selections, and that
every refusal the host can make comes before the library is loaded and before anything is uploaded.  The device side of the four entry
points is checked in test_gpu_profile_*.py."""
import numpy as np
import pytest


@pytest.fixture
def no_gpu(monkeypatch):
    """the library and every upload fail the test"""
    import torch

    from gcn_drug_repurposing_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the refusal"))
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("a tensor was moved before the refusal"))


P = np.arange(30, dtype=np.float64).reshape(3, 10)
NAMED = {"a": P[0], "b": P[1], "c": P[2]}
RAGGED = {"a": P[0], "b": P[1][:9]}


def test_python_refusals_come_before_the_library(no_gpu):
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd.diffusion import compare_profile_pairs, compare_profiles, rank_profiles
    for fn in (lambda: compare_profiles(P, None, None, "kendall"), lambda: compare_profile_pairs(P, [0], [1], "kendall")):
        with pytest.raises(ValueError, match="profile distance 'kendall' is unknown"):
            fn()
    # an index outside the range, by the selection's word
    with pytest.raises(ValueError, match=r"rank_profiles: column index 3 is outside \[0, 3\)"):
        rank_profiles(P, [0, 3])
    with pytest.raises(ValueError, match=r"compare_profiles: row index -1 is outside \[0, 3\)"):
        compare_profiles(P, [0, -1], [7], "cosine")                       # rows before cols
    with pytest.raises(ValueError, match=r"compare_profiles: column index 7 is outside \[0, 3\)"):
        compare_profiles(P, [0], [7], "cosine")
    with pytest.raises(ValueError, match=r"compare_profiles: col_a index 3 is outside \[0, 3\)"):     # the prefix these two have always carried
        compare_profile_pairs(P, [3], [4], "cosine")
    with pytest.raises(ValueError, match=r"compare_profiles: col_b index 4 is outside \[0, 3\)"):
        compare_profile_pairs(P, [2], [4], "cosine")
    # a name with no profile
    with pytest.raises(ValueError, match="rank_profiles: column 'q' has no profile"):
        rank_profiles(NAMED, ["a", "q"])
    with pytest.raises(ValueError, match="compare_profiles: row 'q' has no profile"):
        compare_profiles(NAMED, ["q"], ["r"], "cosine")
    with pytest.raises(ValueError, match="compare_profiles: column 'r' has no profile"):
        compare_profiles(NAMED, ["a"], ["r"], "cosine")
    with pytest.raises(ValueError, match="compare_profiles: col_b 'q' has no profile"):
        compare_profile_pairs(NAMED, ["a"], ["q"], "cosine")
    # a dict has no "every profile"
    with pytest.raises(ValueError, match="rank_profiles: cols must name the profiles of a dict"):
        rank_profiles(NAMED)
    for rows, cols in ((None, ["a"]), (["a"], None), (None, None)):
        with pytest.raises(ValueError, match="compare_profiles: rows and cols must name the profiles of a dict"):
            compare_profiles(NAMED, rows, cols, "cosine")
    for kind in (P, NAMED):
        with pytest.raises(ValueError, match="compare_profile_pairs: col_a and col_b must list the pairs"):
            compare_profile_pairs(kind, None, [0], "cosine")
    # the source itself
    for fn, who in ((lambda p: rank_profiles(p, ["a", "b"]), "rank_profiles"), (lambda p: compare_profiles(p, ["a"], ["b"], "cosine"), "compare_profiles"),
                    (lambda p: compare_profile_pairs(p, ["a"], ["b"], "cosine"), "compare_profile_pairs")):
        with pytest.raises(ValueError, match=who + ": the profiles differ in length"):
            fn(RAGGED)
    for fn, who in ((lambda p: rank_profiles(p), "rank_profiles"), (lambda p: compare_profiles(p, None, None, "cosine"), "compare_profiles"),
                    (lambda p: compare_profile_pairs(p, [0], [0], "cosine"), "compare_profile_pairs")):
        with pytest.raises(ValueError, match=who + r": a host profile array must be \[K\]\[N\], not \(4,\)"):
            fn(np.ones(4))
    with pytest.raises(ValueError, match="compare_profile_pairs: col_a lists 2 profiles and col_b 1"):
        compare_profile_pairs(P, [0, 1], [2], "cosine")
    with pytest.raises(ValueError, match="compare_profile_pairs: col_a lists 2 profiles and col_b 1"):
        compare_profile_pairs(NAMED, ["a", "b"], ["c"], "cosine")
    with pytest.raises(ValueError, match="rank_profiles: the profiles are empty"):
        rank_profiles(np.ones((2, 0)))
    # the order: metric, device kind, source, lists
    with pytest.raises(ValueError, match="'kendall' is unknown"):
        compare_profiles(np.ones(4), [9], [9], "kendall", device="cpu")
    for fn in (lambda **k: rank_profiles(np.ones(4), [9], **k), lambda **k: compare_profiles(np.ones(4), [9], [9], "cosine", **k),
               lambda **k: compare_profile_pairs(np.ones(4), [9], [9, 9], "spearman", **k)):
        with pytest.raises(_lib.GssError, match="no CPU fallback"):
            fn(device="cpu")
        with pytest.raises(ValueError, match="a host profile array must be"):
            fn()


def test_the_resolver_on_arrays_and_dicts(no_gpu):
    from gcn_drug_repurposing_amd.diffusion import _profile_source
    n, (c,), _ = _profile_source(P, ([2, 0, 2, 1],), ("column",), "t")         # lists may repeat and be permuted
    assert n == 10 and c.dtype == np.int32 and c.tolist() == [2, 0, 2, 1]
    n, (c,), _ = _profile_source(P, (None,), ("column",), "t")                 # None: every profile of an array
    assert n == 10 and c.dtype == np.int32 and c.tolist() == [0, 1, 2]
    for labels in (("row", "column"), ("col_a", "col_b")):                     # the same profiles as an array and as a dict
        from_array = _profile_source(P, ([0, 1, 2, 0], [1, 1, 2]), labels, "t")
        from_dict = _profile_source(NAMED, (["a", "b", "c", "a"], ["b", "b", "c"]), labels, "t")
        assert from_array[0] == from_dict[0] == 10
        assert [c.tolist() for c in from_array[1]] == [c.tolist() for c in from_dict[1]] == [[0, 1, 2, 0], [1, 1, 2]]
        assert all(c.dtype == np.int32 for c in from_array[1] + from_dict[1])
    # two selections over a dict share one key table in the order of first appearance: every named profile is uploaded once
    n, (ca, cb), _ = _profile_source(NAMED, (["c", "a", "c"], ["a", "b", "c", "b"]), ("row", "column"), "t")
    assert n == 10 and ca.tolist() == [0, 1, 0] and cb.tolist() == [1, 2, 0, 2]
    n, (ca, cb), _ = _profile_source(NAMED, ([], []), ("row", "column"), "t")  # two empty selections: an empty result, no profile to measure
    assert n == 0 and len(ca) == 0 and len(cb) == 0
    with pytest.raises(ValueError, match="t: no profile is named"):
        _profile_source(NAMED, ([],), ("column",), "t")


def test_the_upload_holds_each_named_profile_once(monkeypatch):
    import torch

    from gcn_drug_repurposing_amd.diffusion import _profile_source
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)         # the "device" is the host
    _, (ca, cb), upload = _profile_source(NAMED, (["c", "a", "c"], ["a", "b", "c", "b"]), ("row", "column"), "t")
    x = upload("anywhere")
    assert tuple(x.shape) == (10, 3) and x.stride(1) == 1                       # [N][width], unit column stride
    assert np.array_equal(x.numpy().T, P[[2, 0, 1]])                            # c, a, b: first appearance, once each
    assert np.array_equal(x.numpy()[:, ca].T, P[[2, 0, 2]]) and np.array_equal(x.numpy()[:, cb].T, P[[0, 1, 2, 1]])
    _, (c,), upload = _profile_source(P, ([1],), ("column",), "t")
    assert np.array_equal(upload("anywhere").numpy().T, P)                      # an array is uploaded whole, transposed
