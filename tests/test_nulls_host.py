"""CPU: the host side the seeded nulls share (_nulls.py): the int32 refusal by name, the lists' offset overflow in the caller's word for
them, the cutting of a null into calls under a byte budget with uneven pieces on either axis, and Benjamini-Hochberg on ties."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import enrich_mirror as EM  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import _nulls as N  # noqa: E402
from gcn_drug_repurposing_amd import classes, enrich  # noqa: E402


def test_int32_array_refuses_by_name():
    assert N.int32_array("sizes", [3, 2 ** 31 - 1, -2 ** 31], "who").dtype == np.int32
    for bad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError, match="random_pair_sums: sizes holds an entry outside int32"):
            N.int32_array("sizes", [1, bad], "random_pair_sums")
    assert N.int32_array("list 0", [], "who").shape == (0,)


class Long:
    """a list of 2^30 entries that is never read: the offsets overflow before anything is packed"""

    def __len__(self):
        return 2 ** 30


@pytest.mark.parametrize("what", ("lists", "sets"))
def test_device_lists_overflow_names_what_overflowed(what):
    with pytest.raises(ValueError, match=f"scores: the {what} hold {2 ** 31} entries, int32 offsets do not reach"):
        N.device_lists([Long(), Long()], "scores", what, "cpu")
    ptr, idx = N.device_lists([np.array([4, 2], dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([7], dtype=np.int32)], "scores", what, "cpu")
    assert ptr.dtype == idx.dtype == torch.int32 and ptr.tolist() == [0, 2, 2, 3] and idx.tolist() == [4, 2, 7]
    assert N.device_lists([np.zeros(0, dtype=np.int32)], "scores", what, "cpu")[1].numel() == 1      # never an empty allocation


@pytest.mark.parametrize("axis", (0, 1))
def test_chunked_null_cuts_unevenly_and_concatenates_along_the_axis(monkeypatch, axis):
    """7 samples of 40 bytes under a budget of 3 samples and a bit: calls of 3, 3 and 1"""
    monkeypatch.setattr(N, "NULL_CHUNK_BYTES", 3 * 40 + 39)
    whole = torch.arange(2 * 7 * 5, dtype=torch.float64).reshape((7, 2, 5) if axis == 0 else (2, 7, 5))
    issued = []

    def call(count, first):
        issued.append((count, first))
        return whole.narrow(axis, first, count)
    got = N.chunked_null(call, 7, 40, axis=axis)
    assert issued == [(3, 0), (3, 3), (1, 6)]
    assert isinstance(got, np.ndarray) and np.array_equal(got, whole.numpy())
    issued.clear()
    monkeypatch.setattr(N, "NULL_CHUNK_BYTES", 1)                                                      # a budget below one sample: one at a time
    assert np.array_equal(N.chunked_null(call, 2, 40, axis=axis), whole.narrow(axis, 0, 2).numpy()) and issued == [(1, 0), (1, 1)]


def test_benjamini_hochberg_on_ties_equals_the_mirror():
    p = [0.04, 0.01, 0.04, 0.5, 0.01, 1.0, 0.04, 0.03]
    got = N.benjamini_hochberg(p)
    assert np.array_equal(got, EM.benjamini_hochberg(p))
    assert got[1] == got[4] == 0.01 * 8 / 2 and got[0] == got[2] == got[6] == 0.04 * 8 / 6      # ties share the q of their last rank
    assert np.all(got <= 1.0) and got[5] == 1.0


def test_public_names_stay_where_they_were():
    assert classes.benjamini_hochberg is N.benjamini_hochberg and classes.NULL_CHUNK_BYTES == enrich.NULL_CHUNK_BYTES == N.NULL_CHUNK_BYTES
    assert _lib.seed64(-1) == 2 ** 64 - 1 and _lib.seed64(2 ** 64 + 5) == 5
